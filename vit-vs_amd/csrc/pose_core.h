// What the pose law (pose.hip) and the pose rig law (pose_rig.hip) share: the handle's form of a point
// row, the layout of the head of their dynamic LDS, Horn's solve (a cyclic Jacobi eigen-decomposition of the 4 x 4 matrix in fp64,
// all indices compile-time: no scratch), the alignment loop around it (pose_align) and the twist.  The median and the Tukey step
// of the loop are robust_core.h's.  At the end: the three-point model of the pose law's consensus start (consensus_core.h).
#pragma once
#include "common.h"
#include "consensus_core.h"
#include "kernels.h"
#include "robust_core.h"
#include "solve.h"

#pragma clang fp contract(off)

namespace vitvs {

// dynamic LDS in doubles: slices [8][32] | 64 results (see the kPose* offsets) | ROBUST: rho [ld] | w [ld]
constexpr int kPoseHead = 8 * 32 + 64;
constexpr int kPoseSum = 256;        // [0 .. 11): the centred sums
constexpr int kPoseCen = 256 + 12;   // sw, pc [3], qc [3]
constexpr int kPoseRt = 256 + 20;    // R [9] row-major, t [3], q [4]
constexpr int kPoseMid = 256 + 36;   // the two middle values of the median
constexpr int kPoseInt = 256 + 40;   // ints: [0] solve outcome (0 ok, 1 degenerate), [1] sweeps, [2 .. 6) the waves' zero weights,
                                     //       [6 .. 10) their usable rows, [10 .. 14) their holes

// The handle's form of a point row (PoseArgs and PoseRigArgs name its arrays alike): row `row` = cam * ld + k of what camera `cam`'s
// law left -> the current point p and the goal point g in that camera's frames.  Returns the flag: 1 usable, 0 padded, -1 a hole.
template <class Args>
__device__ __forceinline__ int pose_handle_row(const Args& a, int cam, size_t row, double (&p)[3], double (&g)[3]) {
    const int tok = a.selected[row];
    if (!(tok >= 0 && tok < a.T)) return 0;
    const double Z = a.feat[row * 4 + 0], x = a.feat[row * 4 + 1], y = a.feat[row * 4 + 2];
    const unsigned ds = a.zgoal[(size_t)cam * a.zgoal_stride + tok];
    if (!(Z < 100.0 && ds != 0)) return -1;                 // a hole in either depth drops the row
    const double fx = a.K[cam * 4 + 0], fy = a.K[cam * 4 + 1], cx = a.K[cam * 4 + 2], cy = a.K[cam * 4 + 3];
    const double Zs = (double)ds / 1000.0;
    const double xs = ((double)a.s_uv[row * 4 + 0] - cx) / fx, ys = ((double)a.s_uv[row * 4 + 1] - cy) / fy;
    p[0] = Z * x; p[1] = Z * y; p[2] = Z;
    g[0] = Zs * xs; g[1] = Zs * ys; g[2] = Zs;
    return 1;
}

// One Jacobi rotation of the symmetric A in the (P, Q) plane, accumulated into V (eigenvectors in columns)
template <int P, int Q>
__device__ __forceinline__ void pose_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = c * arp - s * arq;
            A[r][Q] = A[Q][r] = s * arp + c * arq;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// Horn's solve from the sums in sm (every lane of the calling wave computes the same): R, t, the quaternion; returns false when
// the clouds are degenerate (ev_1 - ev_2 <= 1e-8 of the two scatters: collinear points leave a rotation free)
__device__ __forceinline__ bool pose_solve(const double* sm, double (&R)[9], double (&t)[3], double (&q)[4], int& sweeps) {
    const double* S = sm + kPoseSum;
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    const double scatter = S[9] + S[10];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    double normsq = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) normsq += A[i][j] * A[i][j];
    sweeps = 0;
    for (int sw = 0; sw < 32; ++sw) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) off += A[p][r] * A[p][r];
        if (off <= 1e-40 * normsq) break;
        ++sweeps;
        pose_rotate<0, 1>(A, V); pose_rotate<0, 2>(A, V); pose_rotate<0, 3>(A, V);
        pose_rotate<1, 2>(A, V); pose_rotate<1, 3>(A, V); pose_rotate<2, 3>(A, V);
    }
    int i1 = 0;
    double ev1 = A[0][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > ev1) { ev1 = A[i][i]; i1 = i; }
    double ev2 = -__builtin_huge_val();
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i != i1) ev2 = fmax(ev2, A[i][i]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        q[r] = V[r][0];
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (i == i1) q[r] = V[r][i];
    }
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sg = q[0] / qn < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = sg * (q[r] / qn);
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    R[0] = a * a + b * b - c * c - d * d; R[1] = 2.0 * (b * c - a * d);         R[2] = 2.0 * (b * d + a * c);
    R[3] = 2.0 * (b * c + a * d);         R[4] = a * a - b * b + c * c - d * d; R[5] = 2.0 * (c * d - a * b);
    R[6] = 2.0 * (b * d - a * c);         R[7] = 2.0 * (c * d + a * b);         R[8] = a * a - b * b - c * c + d * d;
    const double* cen = sm + kPoseCen;
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = cen[4 + i] - ((R[3 * i] * cen[1] + R[3 * i + 1] * cen[2]) + R[3 * i + 2] * cen[3]);
    return !(ev1 - ev2 <= 1e-8 * scatter);
}

// |Q_r - (R P_r + t)|^2: the squared residual of row r of a point block (pose_align's rho before the square root, and what the
// consensus start scores)
__device__ __forceinline__ double pose_residual_sq(const double* R, const double* t, const double* ws, int stride, int r) {
    const double p0 = ws[r], p1 = ws[(size_t)stride + r], p2 = ws[(size_t)2 * stride + r];
    const double d0 = ws[(size_t)3 * stride + r] - (((R[0] * p0 + R[1] * p1) + R[2] * p2) + t[0]);
    const double d1 = ws[(size_t)4 * stride + r] - (((R[3] * p0 + R[4] * p1) + R[5] * p2) + t[1]);
    const double d2 = ws[(size_t)5 * stride + r] - (((R[6] * p0 + R[7] * p1) + R[8] * p2) + t[2]);
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// What pose_align leaves in every thread's registers
struct PoseFit {
    double R[9], t[3], q[4];
    int status, sweeps, reweighted, n_zero, degenerate;
    double sigma;
};

// The alignment loop, 256 threads: n_iter Tukey re-weightings (ROBUST; else none) and one more solve behind the last.  ws holds
// P [3][stride] | Q [3][stride] | flag [stride]; rows [0, n) take part, n_us of them usable.  Every solve takes the weighted
// centroids first and the centred sums second, each as quantities x 8 row slices (row r belongs to slice r mod 8, ascending rows,
// the slices added in ascending order): bit-reproducible.  Wave 0 then solves and publishes R, t, q through LDS.  ROBUST: wk
// (LDS) holds the caller's first weights on entry and the last ones on return; rho (LDS) holds +inf in every row that is not usable.
// Every barrier here orders LDS only (lds_barrier): the loop writes nothing but LDS (smp, rho, wk).  The point block is global
// memory, but the caller wrote it before the __syncthreads() that follows its Phase A, and the loop only reads it.
// A consensus start (consensus_core.h) hands over its weights where the loop reads them (wk, or the flag row in the plain form)
// and n_zero0, the usable rows it left at weight 0.
template <bool ROBUST>
__device__ __forceinline__ void pose_align(const double* ws, int stride, int n, int n_us, double sigma_min, int n_iter, double* smp,
                                           double* rho, double* wk, PoseFit& fit, int n_zero0 = 0) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qid = tid & 31, slice = tid >> 5;
    const double* flag = ws + (size_t)6 * stride;
    int* iscr = reinterpret_cast<int*>(smp + kPoseInt);
    fit = PoseFit{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {1, 0, 0, 0}, ST_OK, 0, 0, 0, 0, 0.0};
    fit.n_zero = n_zero0;
    const int N = ROBUST ? n_iter : 0;
    for (int it = 0;; ++it) {
        if (n_us - fit.n_zero < 3) { fit.status = ST_TOO_FEW; break; }
        // the weighted centroids: sw, sum w P, sum w Q
        if (qid < 7) {
            double acc = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : (flag[r] > 0.0 ? 1.0 : 0.0);
                acc += qid == 0 ? w : w * ws[(size_t)(qid - 1) * stride + r];
            }
            smp[slice * 32 + qid] = acc;
        }
        lds_barrier();
        if (tid < 7) {
            double s = 0.0, s0 = 0.0;
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) { s += smp[sl * 32 + tid]; s0 += smp[sl * 32]; }
            smp[kPoseCen + tid] = tid == 0 ? s : s / s0;
        }
        lds_barrier();
        // the centred sums: S [9] = sum w (P - pc)(Q - qc)^T, sum w |P - pc|^2, sum w |Q - qc|^2
        if (qid < 11) {
            const double* cen = smp + kPoseCen;
            const int ca = qid < 9 ? qid / 3 : 0, cb = qid < 9 ? qid % 3 : 0;
            double acc = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : (flag[r] > 0.0 ? 1.0 : 0.0);
                double term;
                if (qid < 9) {
                    term = w * (ws[(size_t)ca * stride + r] - cen[1 + ca]) * (ws[(size_t)(3 + cb) * stride + r] - cen[4 + cb]);
                } else {
                    const int o = qid == 9 ? 0 : 3;
                    const double d0 = ws[(size_t)o * stride + r] - cen[1 + o], d1 = ws[(size_t)(o + 1) * stride + r] - cen[2 + o],
                                 d2 = ws[(size_t)(o + 2) * stride + r] - cen[3 + o];
                    term = w * ((d0 * d0 + d1 * d1) + d2 * d2);
                }
                acc += term;
            }
            smp[slice * 32 + qid] = acc;
        }
        lds_barrier();
        if (tid < 11) {
            double s = 0.0;
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) s += smp[sl * 32 + tid];
            smp[kPoseSum + tid] = s;
        }
        lds_barrier();
        if (wave == 0) {
            double Rn[9], tn[3], qn[4];
            int sw;
            const bool ok = pose_solve(smp, Rn, tn, qn, sw);
            if (lane == 0) {
                iscr[0] = ok ? 0 : 1;
                iscr[1] = sw;
#pragma unroll
                for (int i = 0; i < 9; ++i) smp[kPoseRt + i] = Rn[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) smp[kPoseRt + 9 + i] = tn[i];
#pragma unroll
                for (int i = 0; i < 4; ++i) smp[kPoseRt + 12 + i] = qn[i];
            }
        }
        lds_barrier();
        fit.sweeps = iscr[1];
        if (iscr[0]) { fit.degenerate = 1; fit.status = ST_TOO_FEW; break; }
#pragma unroll
        for (int i = 0; i < 9; ++i) fit.R[i] = smp[kPoseRt + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) fit.t[i] = smp[kPoseRt + 9 + i];
#pragma unroll
        for (int i = 0; i < 4; ++i) fit.q[i] = smp[kPoseRt + 12 + i];
        if (it == N) break;
        if constexpr (ROBUST) {
            for (int k = tid; k < n; k += 256) {
                if (!(flag[k] > 0.0)) continue;             // not a usable row: rho stays +inf
                rho[k] = sqrt(pose_residual_sq(fit.R, fit.t, ws, stride, k));
            }
            lds_barrier();
            median_middles(rho, n, n_us, smp + kPoseMid, tid);
            lds_barrier();
            fit.sigma = tukey_reweight<true>(rho, flag, n, smp + kPoseMid, sigma_min, wk, nullptr, iscr + 2, tid);
            lds_barrier();
            fit.n_zero = iscr[2] + iscr[3] + iscr[4] + iscr[5];
            fit.reweighted = it + 1;
        }
    }
}

// v = -lambda (R^T t, theta u): ViSP's PBVS law on a fit whose status is ST_OK
__device__ __forceinline__ void pose_twist(double lambda, const PoseFit& fit, double (&v)[6]) {
    const double* R = fit.R;
    const double* t = fit.t;
    const double* q = fit.q;
    const double nv = sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
    const double f = nv == 0.0 ? 0.0 : 2.0 * atan2(nv, q[0]) / nv;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] = -lambda * ((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
        v[3 + i] = -lambda * (f * q[1 + i]);
    }
}

// ---- the model of the consensus start ("The consensus start"; the phase itself is consensus_core.h's);
// tests/pose_consensus_ref.py restates every line below in the same order of arithmetic

// The orthonormal triad of three points: e1 along x1 - x0, e3 along the normal of their plane, e2 = e3 x e1 (rows of e).  False when
// the points are collinear or coincide: |a x b|^2 <= 1e-8 |a|^2 |b|^2.
__device__ __forceinline__ bool pose_triad(const double (&x)[3][3], double (&e)[3][3]) {
    double a[3], b[3], n[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = x[1][c] - x[0][c]; b[c] = x[2][c] - x[0][c]; }
    n[0] = a[1] * b[2] - a[2] * b[1];
    n[1] = a[2] * b[0] - a[0] * b[2];
    n[2] = a[0] * b[1] - a[1] * b[0];
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const double sa = sqrt(aa), sn = sqrt(nn);
#pragma unroll
    for (int c = 0; c < 3; ++c) { e[0][c] = a[c] / sa; e[2][c] = n[c] / sn; }
    e[1][0] = e[2][1] * e[0][2] - e[2][2] * e[0][1];
    e[1][1] = e[2][2] * e[0][0] - e[2][0] * e[0][2];
    e[1][2] = e[2][0] * e[0][1] - e[2][1] * e[0][0];
    return nn > (1e-8 * aa) * bb;
}

// The rigid displacement of the three rows `rows` in closed form: R carries the triad of the current points onto that of the goal
// points, t = qm - R pm with the means of the three.  False when either triple is collinear or an entry is not finite.
__device__ __forceinline__ bool pose_three_point(const double* ws, int stride, const int* rows, double* R, double* t) {
    double p[3][3], g[3][3], ep[3][3], eg[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[i][c] = ws[(size_t)c * stride + rows[i]];
            g[i][c] = ws[(size_t)(3 + c) * stride + rows[i]];
        }
    const bool spread = pose_triad(p, ep), spread_g = pose_triad(g, eg);
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R[3 * i + j] = (eg[0][i] * ep[0][j] + eg[1][i] * ep[1][j]) + eg[2][i] * ep[2][j];
            finite = finite && fabs(R[3 * i + j]) < __builtin_huge_val();
        }
    double pm[3], gm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pm[c] = ((p[0][c] + p[1][c]) + p[2][c]) / 3.0;
        gm[c] = ((g[0][c] + g[1][c]) + g[2][c]) / 3.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        t[i] = gm[i] - ((R[3 * i] * pm[0] + R[3 * i + 1] * pm[1]) + R[3 * i + 2] * pm[2]);
        finite = finite && fabs(t[i]) < __builtin_huge_val();
    }
    return spread && spread_g && finite;
}

// One hypothesis of the pose law's consensus start (consensus_core.h's consensus_start): three rows, the displacement in closed form
struct PoseThreePoint {
    static constexpr int kRows = 3, kFlagRow = 6, kFit = 12;                   // R row-major, t
    static __device__ __forceinline__ bool fit(const double* ws, int stride, const int* rows, double* Rt) {
        return pose_three_point(ws, stride, rows, Rt, Rt + 9);
    }
    static __device__ __forceinline__ double residual_sq(const double* Rt, const double* ws, int stride, int r) {
        return pose_residual_sq(Rt, Rt + 9, ws, stride, r);
    }
};

}  // namespace vitvs
