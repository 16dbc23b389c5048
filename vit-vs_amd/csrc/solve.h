// The fp64 solvers of the control laws: the 6x6 normal equations by LDL^T, and the one-sided Jacobi SVD behind a failed pivot.
// Shared by servo.hip (one camera's law) and rig.hip (the rig law over the cameras' stacked rows); their robust laws also share
// the weighted solve step and the pair-residual pass at the end of this file.
#pragma once
#include "common.h"
#include "robust_core.h"

#pragma clang fp contract(off)

namespace vitvs {

// LDL^T solves the 6x6 normal equations only while every pivot d_j > kPivotThreshold * G_jj; below that the Jacobi SVD of L itself
// does.  G has cond(L)^2: LDL^T's error grows as 1 / (the smallest d_j / G_jj), measured 1e-12 at 2e-4 and 2e-9 (past the
// project's 1e-9 bar for a twist) at 2e-8 (tests/test_gpu_solve_handoff.py).  tests/solve_ref.py THRESHOLD mirrors it.
constexpr double kPivotThreshold = 1e-4;

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains every outstanding
// global load AND store (vmcnt(0)); this kernel is one serial chain of short phases, and its detail
// stores and prefetched loads must stay in flight across the phase boundaries.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// G = L^T W L (21, upper triangle) and g = L^T W e (6): 27 quantities x 8 row slices on 216 threads into Gs[40 ..) (fixed
// slice order -> deterministic), W = wk[pair] on both rows of a pair.
__device__ __forceinline__ void normal_equation_slices(const double* Lc, int rcap, int R, const double* wk, double* Gs, int tid) {
    const int qid = tid & 31, slice = tid >> 5;
    if (qid < 27) {
        int ca, cb;
        if (qid < 21) {
            int q = qid;
            ca = 0;
            while (q >= 6 - ca) { q -= 6 - ca; ++ca; }
            cb = ca + q;
        } else {
            ca = qid - 21;
            cb = 6;
        }
        // 4 independent chains keep 8 loads in flight (dense selections read L from the global workspace);
        // fixed combination order -> still deterministic
        double acc4[4] = {0.0, 0.0, 0.0, 0.0};
        int r = slice;
        for (; r + 24 < R; r += 32) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc4[u] += wk[(r + 8 * u) >> 1] * (Lc[ca * rcap + r + 8 * u] * Lc[cb * rcap + r + 8 * u]);
            }
        }
        for (; r < R; r += 8) {
            acc4[0] += wk[r >> 1] * (Lc[ca * rcap + r] * Lc[cb * rcap + r]);
        }
        Gs[40 + slice * 27 + qid] = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
    }
}

// One wavefront: 27 lanes add the 8 slices, every lane then factors the same 6x6 system in registers (fully unrolled: no
// private-memory arrays, no cross-lane traffic).  True, and xsol = G^-1 g, when every pivot passes the kPivotThreshold test.
__device__ __forceinline__ bool solve_ldlt(double* Gs, int lane, double xsol[6]) {
    if (lane < 27) {
        double acc = 0.0;
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) acc += Gs[40 + sl * 27 + lane];
        Gs[lane] = acc;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // same wave: LDS writes above are visible below
    double Gm[6][6], rhs[6];
    {
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { Gm[j][i] = Gs[q]; ++q; }   // lower triangle
#pragma unroll
        for (int i = 0; i < 6; ++i) rhs[i] = Gs[21 + i];
    }
    // G = L D L^T (unit lower-triangular L, no square roots, one reciprocal per pivot)
    bool good = true;
    double Lf[6][6], dinv[6], dpiv[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = Gm[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= Lf[j][k] * Lf[j][k] * dpiv[k];
        good = good && (d > kPivotThreshold * Gm[j][j]) && (Gm[j][j] > 0.0);
        dpiv[j] = d;
        dinv[j] = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = Gm[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= Lf[i][k] * Lf[j][k] * dpiv[k];
            Lf[i][j] = t * dinv[j];
        }
    }
    if (good) {
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {          // L y = rhs
            double t = rhs[i];
#pragma unroll
            for (int k = 0; k < i; ++k) t -= Lf[i][k] * y[k];
            y[i] = t;
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {         // L^T x = D^-1 y
            double t = y[i] * dinv[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) t -= Lf[k][i] * xsol[k];
            xsol[i] = t;
        }
    }
    return good;
}

// One wavefront: xsol = pinv(A) rhs by one-sided Jacobi SVD with numpy.linalg.pinv's rcond = 1e-15 cut-off; A = the 6 columns
// of Lc, rhs its 7th.  The rotations overwrite Lc.  Returns the sweeps that ran (<= 40).
__device__ __forceinline__ int solve_jacobi(double* Lc, int rcap, int R, int lane, double xsol[6]) {
    double V[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    const double tol = 4e-15;
    int sweeps;
    for (sweeps = 0; sweeps < 40; ++sweeps) {
        int rotated = 0;
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int q = p + 1; q < 6; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = lane; r < R; r += 64) {
                    const double ap = Lc[p * rcap + r], aq = Lc[q * rcap + r];
                    al += ap * ap; be += aq * aq; ga += ap * aq;
                }
                al = wave_sum(al); be = wave_sum(be); ga = wave_sum(ga);
                if (fabs(ga) > tol * sqrt(al * be) && al > 0.0 && be > 0.0) {
                    ++rotated;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                    for (int r = lane; r < R; r += 64) {
                        const double ap = Lc[p * rcap + r], aq = Lc[q * rcap + r];
                        Lc[p * rcap + r] = c * ap - s * aq;
                        Lc[q * rcap + r] = s * ap + c * aq;
                    }
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        const double vp = V[i][p], vq = V[i][q];
                        V[i][p] = c * vp - s * vq;
                        V[i][q] = s * vp + c * vq;
                    }
                }
            }
        if (rotated == 0) break;
    }
    double sig2[6], w[6], smax2 = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s2 = 0.0, dot = 0.0;
        for (int r = lane; r < R; r += 64) {
            const double aj = Lc[j * rcap + r];
            s2 += aj * aj;
            dot += aj * Lc[6 * rcap + r];
        }
        sig2[j] = wave_sum(s2);
        w[j] = wave_sum(dot);
        smax2 = fmax(smax2, sig2[j]);
    }
    const double cutoff = 1e-15 * sqrt(smax2);
#pragma unroll
    for (int i = 0; i < 6; ++i) xsol[i] = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        if (sqrt(sig2[j]) > cutoff) {
            const double coef = w[j] / sig2[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) xsol[i] += V[i][j] * coef;
        }
    }
    return sweeps;
}

// The weighted solve step of a robust law (servo_kernel<true, .>, rig_robust_kernel), wave 0 behind normal_equation_slices and a
// barrier: LDL^T of the 6 x 6 system under the pair weights wk; behind a failed pivot the Jacobi SVD of a copy of the R rows of Lc
// (capacity rcap) scaled by sqrt(w), in Lw (capacity wcap).  L and e themselves are never scaled.  Lane 0 publishes x in
// Gs[28 .. 34) and clears the two median cells Gs[34], Gs[35]; vout = -lambda x in every lane.  Returns -1 when LDL^T solved, else
// the Jacobi sweeps.  (x stays a local here: handed back through the caller's array it cost servo_kernel<true, true, .> eight
// VGPRs and an occupancy step.)
__device__ __forceinline__ int weighted_solve(const double* Lc, int rcap, int R, const double* wk, double* Gs, double* Lw, int wcap,
                                              int lane, double lambda, double (&vout)[6]) {
    double xsol[6];
    const bool solved = solve_ldlt(Gs, lane, xsol);
    int sweeps = -1;
    if (!solved) {
        // each lane scales and copies the rows it alone rotates (r = lane mod 64)
        for (int r = lane; r < R; r += 64) {
            const double sw = sqrt(wk[r >> 1]);
            for (int c = 0; c < 7; ++c) Lw[(size_t)c * wcap + r] = sw * Lc[(size_t)c * rcap + r];
        }
        sweeps = solve_jacobi(Lw, wcap, R, lane, xsol);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        vout[i] = -lambda * xsol[i];
        if (lane == 0) Gs[28 + i] = xsol[i];
    }
    if (lane == 0) { Gs[34] = 0.0; Gs[35] = 0.0; }
    return sweeps;
}

// rho[k] = |e - L x| of pairs k < n (rows 2k, 2k + 1 of Lc), x = Gs[28 .. 34).  SKIP_INF: a pair whose rho is +inf is not live and
// keeps it.
template <bool SKIP_INF>
__device__ __forceinline__ void pair_residuals(const double* Lc, int rcap, int n, const double* Gs, double* rho, int tid) {
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = Gs[28 + i];
    for (int k = tid; k < n; k += 256) {
        if constexpr (SKIP_INF) {
            if ((unsigned long long)__double_as_longlong(rho[k]) == kInfBits) continue;
        }
        double r0 = Lc[6 * rcap + 2 * k], r1 = Lc[6 * rcap + 2 * k + 1];
        double p0 = 0.0, p1 = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            p0 += Lc[c * rcap + 2 * k] * x[c];
            p1 += Lc[c * rcap + 2 * k + 1] * x[c];
        }
        r0 -= p0; r1 -= p1;
        rho[k] = sqrt(r0 * r0 + r1 * r1);
    }
}

}  // namespace vitvs
