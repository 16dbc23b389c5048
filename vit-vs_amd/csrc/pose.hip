// The pose law: one rigid 3-D alignment of the matched points.
//   P_k = Z (x, y, 1)       the current point of feature row k in the current camera's frame (feat of the camera's law)
//   Q_k = Z* (xs, ys, 1)    its goal point in the goal camera's frame (s_uv and the handle's goal-depth table)
//   (R, t) = argmin sum_k w_k |Q_k - (R P_k + t)|^2      Horn's closed form: the unit quaternion of R is the eigenvector of the
//                                                        largest eigenvalue of the symmetric 4 x 4 matrix N(S),
//                                                        S = sum w (P - pc)(Q - qc)^T, t = qc - R pc
//   v_pose = -lambda (R^T t, theta u)                    ViSP's PBVS law, a twist in the current camera's own optical frame
// One launch, one 256-thread workgroup per pair; nothing passes between workgroups.  Phase A writes P, Q and the usable flag of
// every row into the pair's block of a global workspace that this workgroup alone writes and reads, behind __syncthreads() (as
// servo_kernel treats a global L): any max_rows works.  Every solve takes the weighted centroids first and the centred sums
// second, each as quantities x 8 row slices (row r belongs to slice r mod 8, ascending rows, the slices added in ascending order):
// bit-reproducible.  Wave 0 then solves, every lane the same arithmetic: a cyclic Jacobi eigen-decomposition of the 4 x 4 matrix
// in fp64, all indices compile-time (no scratch).  ROBUST: n_iter Tukey re-weightings with rho and w in dynamic LDS, the median by
// the rank counting of servo.hip (integer compares on the bit patterns, ties by index), one more solve behind the last.
#include "common.h"
#include "kernels.h"
#include "pose_core.h"
#include "solve.h"

#pragma clang fp contract(off)

namespace vitvs {

template <bool ROBUST>
__global__ __launch_bounds__(256) void pose_kernel(PoseArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smp[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = a.ld;
    double* ws = a.ws + (size_t)b * 7 * ld;                 // P [3][ld] | Q [3][ld] | flag [ld]: 1 usable, 0 padded, -1 a hole
    int* iscr = reinterpret_cast<int*>(smp + kPoseInt);
    double* rho = smp + kPoseHead;
    double* wk = rho + ld;
    double* vout = a.v_pose + (size_t)b * 6;

    // the early outs: the camera's own failure, the same-image shortcut (the camera is at the goal: v = 0, R = I exactly)
    const int cam = a.status ? a.status[b] : (int)ST_OK;
    const bool same = a.info && a.info[(size_t)b * 8 + 2] != 0;
    if (cam != ST_OK || same) {
        if (a.weights)
            for (int k = tid; k < a.weights_stride; k += 256) a.weights[(size_t)b * a.weights_stride + k] = 0.0;
        if (tid < 6) vout[tid] = 0.0;
        if (tid < 12 && a.pose) a.pose[(size_t)b * 12 + tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0 : 0.0;
        if (tid < 8 && a.pose_info) a.pose_info[(size_t)b * 8 + tid] = 0;
        if (tid == 0) {
            a.pose_status[b] = cam;
            if (a.sigma) a.sigma[b] = 0.0;
        }
        return;
    }

    // Phase A: the points.  n rows take part: the rows the camera's law wrote (info[1]), or every row of given points
    int n = ld, n_us = 0, holes = 0;
    if (a.P) {
        const double* Pb = a.P + (size_t)b * ld * 3;
        const double* Qb = a.Q + (size_t)b * ld * 3;
        const int32_t* ub = a.usable + (size_t)b * ld;
        for (int k = tid; k < n; k += 256) {
            const int f = ub[k] > 0 ? 1 : (ub[k] < 0 ? -1 : 0);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ws[(size_t)c * ld + k] = f > 0 ? Pb[k * 3 + c] : 0.0;
                ws[(size_t)(3 + c) * ld + k] = f > 0 ? Qb[k * 3 + c] : 0.0;
            }
            ws[(size_t)6 * ld + k] = (double)f;
            n_us += f > 0;
            holes += f < 0;
        }
    } else {
        n = min(max(a.info[(size_t)b * 8 + 1], 0), ld);
        const double fx = a.K[b * 4 + 0], fy = a.K[b * 4 + 1], cx = a.K[b * 4 + 2], cy = a.K[b * 4 + 3];
        const int32_t* sel = a.selected + (size_t)b * ld;
        const int32_t* uv = a.s_uv + (size_t)b * ld * 4;
        const double* ft = a.feat + (size_t)b * ld * 4;
        const uint16_t* tab = a.zgoal + (size_t)b * a.zgoal_stride;
        for (int k = tid; k < n; k += 256) {
            const int tok = sel[k];
            int f = 0;
            double p[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
            if (tok >= 0 && tok < a.T) {
                const double Z = ft[k * 4 + 0], x = ft[k * 4 + 1], y = ft[k * 4 + 2];
                const unsigned ds = tab[tok];
                f = (Z < 100.0 && ds != 0) ? 1 : -1;         // a hole in either depth drops the row
                if (f > 0) {
                    const double Zs = (double)ds / 1000.0;
                    const double xs = ((double)uv[k * 4 + 0] - cx) / fx, ys = ((double)uv[k * 4 + 1] - cy) / fy;
                    p[0] = Z * x; p[1] = Z * y; p[2] = Z;
                    g[0] = Zs * xs; g[1] = Zs * ys; g[2] = Zs;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ws[(size_t)c * ld + k] = p[c];
                ws[(size_t)(3 + c) * ld + k] = g[c];
            }
            ws[(size_t)6 * ld + k] = (double)f;
            n_us += f > 0;
            holes += f < 0;
        }
    }
    n_us = wave_sum(n_us);
    holes = wave_sum(holes);
    if (lane == 0) { iscr[6 + wave] = n_us; iscr[10 + wave] = holes; }
    __syncthreads();                                        // (the points are global memory: full fence)
    n_us = iscr[6] + iscr[7] + iscr[8] + iscr[9];
    holes = iscr[10] + iscr[11] + iscr[12] + iscr[13];
    const double* flag = ws + (size_t)6 * ld;

    double sigma_min = a.sigma_min;
    if constexpr (ROBUST) {
        for (int k = tid; k < n; k += 256) {
            const bool us = flag[k] > 0.0;
            wk[k] = us ? 1.0 : 0.0;
            rho[k] = us ? ws[(size_t)5 * ld + k] : __longlong_as_double((long long)kPoseInfBits);   // Z* for sigma_min's median
        }
        if (a.K && n_us > 0) {
            lds_barrier();
            pose_middles(rho, n, n_us, smp + kPoseMid, tid);
            lds_barrier();
            sigma_min = 0.5 * fmax(a.pitch_u / a.K[b * 4 + 0], a.pitch_v / a.K[b * 4 + 1]) * ((smp[kPoseMid] + smp[kPoseMid + 1]) * 0.5);
        }
        lds_barrier();
    }

    const int qid = tid & 31, slice = tid >> 5;
    int status = ST_OK, sweeps = 0, reweighted = 0, n_zero = 0, degenerate = 0;
    double sigma = 0.0;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, q[4] = {1, 0, 0, 0};
    const int N = ROBUST ? a.n_iter : 0;
    for (int it = 0;; ++it) {
        if (n_us - n_zero < 3) { status = ST_TOO_FEW; break; }
        // the weighted centroids: sw, sum w P, sum w Q
        if (qid < 7) {
            double acc = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : (flag[r] > 0.0 ? 1.0 : 0.0);
                acc += qid == 0 ? w : w * ws[(size_t)(qid - 1) * ld + r];
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
                    term = w * (ws[(size_t)ca * ld + r] - cen[1 + ca]) * (ws[(size_t)(3 + cb) * ld + r] - cen[4 + cb]);
                } else {
                    const int o = qid == 9 ? 0 : 3;
                    const double d0 = ws[(size_t)o * ld + r] - cen[1 + o], d1 = ws[(size_t)(o + 1) * ld + r] - cen[2 + o],
                                 d2 = ws[(size_t)(o + 2) * ld + r] - cen[3 + o];
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
        sweeps = iscr[1];
        if (iscr[0]) { degenerate = 1; status = ST_TOO_FEW; break; }
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = smp[kPoseRt + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = smp[kPoseRt + 9 + i];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = smp[kPoseRt + 12 + i];
        if (it == N) break;
        if constexpr (ROBUST) {
            for (int k = tid; k < n; k += 256) {
                if (!(flag[k] > 0.0)) continue;             // not a usable row: rho stays +inf
                const double p0 = ws[k], p1 = ws[(size_t)ld + k], p2 = ws[(size_t)2 * ld + k];
                const double d0 = ws[(size_t)3 * ld + k] - (((R[0] * p0 + R[1] * p1) + R[2] * p2) + t[0]);
                const double d1 = ws[(size_t)4 * ld + k] - (((R[3] * p0 + R[4] * p1) + R[5] * p2) + t[1]);
                const double d2 = ws[(size_t)5 * ld + k] - (((R[6] * p0 + R[7] * p1) + R[8] * p2) + t[2]);
                rho[k] = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            }
            lds_barrier();
            pose_middles(rho, n, n_us, smp + kPoseMid, tid);
            lds_barrier();
            sigma = fmax(1.4826 * ((smp[kPoseMid] + smp[kPoseMid + 1]) * 0.5), sigma_min);
            const double cs = 4.6851 * sigma;
            int zeros = 0;
            for (int k = tid; k < n; k += 256) {
                const bool us = flag[k] > 0.0;
                const double tt = rho[k] / cs;
                const double u = 1.0 - tt * tt;
                const double w1 = (us && tt < 1.0) ? u * u : 0.0;
                wk[k] = w1;
                zeros += (us && w1 == 0.0) ? 1 : 0;
            }
            zeros = wave_sum(zeros);
            if (lane == 0) iscr[2 + wave] = zeros;
            lds_barrier();
            n_zero = iscr[2] + iscr[3] + iscr[4] + iscr[5];
            reweighted = it + 1;
        }
    }

    if (a.weights) {
        for (int k = tid; k < a.weights_stride; k += 256) {
            double w = 0.0;
            if (k < n) w = ROBUST ? wk[k] : (flag[k] > 0.0 ? 1.0 : 0.0);
            a.weights[(size_t)b * a.weights_stride + k] = w;
        }
    }
    if (tid != 0) return;
    const bool ok = status == ST_OK;
    double v[6] = {0, 0, 0, 0, 0, 0};
    if (ok) {
        const double nv = sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
        const double f = nv == 0.0 ? 0.0 : 2.0 * atan2(nv, q[0]) / nv;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v[i] = -a.lambda * ((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
            v[3 + i] = -a.lambda * (f * q[1 + i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) vout[i] = v[i];
    a.pose_status[b] = status;
    if (a.pose) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.pose[(size_t)b * 12 + i] = ok ? R[i] : ((i & 3) == 0 ? 1.0 : 0.0);
#pragma unroll
        for (int i = 0; i < 3; ++i) a.pose[(size_t)b * 12 + 9 + i] = ok ? t[i] : 0.0;
    }
    if (a.sigma) a.sigma[b] = sigma;
    if (a.pose_info) {
        int32_t* pi = a.pose_info + (size_t)b * 8;
        pi[0] = n_us; pi[1] = sweeps; pi[2] = reweighted; pi[3] = n_zero; pi[4] = degenerate; pi[5] = holes; pi[6] = 0; pi[7] = 0;
    }
}

int plan_pose(int max_rows, int n_iter, PosePlan* plan) {
    if (!plan || max_rows < 1 || n_iter < 0 || n_iter > 16) return -2;
    plan->robust = n_iter > 0;
    plan->lds = ((size_t)kPoseHead + (plan->robust ? (size_t)2 * max_rows : 0)) * sizeof(double);
    plan->lds_opt_in = plan->lds > 64 * 1024;
    return plan->lds > 160 * 1024 ? -3 : 0;
}

size_t pose_scratch_bytes(int n_pairs, int ld) { return (size_t)n_pairs * 7 * ld * sizeof(double); }

int launch_pose(const PoseArgs& a, hipStream_t stream) {
    if (a.n_pairs < 1 || a.ld < 1 || !a.ws || !a.v_pose || !a.pose_status || (a.weights && a.weights_stride < 0)) return -2;
    if (a.P ? (!a.Q || !a.usable) : (!a.selected || !a.s_uv || !a.feat || !a.info || !a.K || !a.zgoal || a.T < 1)) return -2;
    PosePlan p;
    if (int rc = plan_pose(a.ld, a.n_iter, &p)) return rc;
    static std::atomic<unsigned long long> raised{0};
    if (p.robust) {
        if (p.lds_opt_in && raise_lds_limit(reinterpret_cast<const void*>(pose_kernel<true>), 160 * 1024, raised)) return -3;
        launch(pose_kernel<true>, dim3(a.n_pairs), dim3(256), p.lds, stream, a);
    } else {
        launch(pose_kernel<false>, dim3(a.n_pairs), dim3(256), p.lds, stream, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vitvs
