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
// in fp64, all indices compile-time (no scratch).  ROBUST: n_iter Tukey re-weightings with rho and w in dynamic LDS (median_middles
// and tukey_reweight of robust_core.h), one more solve behind the last.  The loop is pose_core.h's pose_align, which the pose rig
// law runs too; this file keeps the early outs, Phase A, sigma_min and the outputs.  CONSENSUS: a phase between Phase A and the
// loop scores n_hyp three-point hypotheses, one per thread and round, and starts the loop from the winner's consensus set
// (consensus_core.h's consensus_start on pose_core.h's PoseThreePoint); the plain form then takes the median of Z* too, for the
// cut-off T = 4.6851 sigma_min.
#include "common.h"
#include "kernels.h"
#include "pose_core.h"

#pragma clang fp contract(off)

namespace vitvs {

template <bool ROBUST, bool CONSENSUS>
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
        for (int k = tid; k < n; k += 256) {
            double p[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
            const int f = pose_handle_row(a, b, (size_t)b * ld + k, p, g);
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
    if constexpr (ROBUST || CONSENSUS) {                    // (the plain form with a consensus start: rho alone, for the cut-off T)
        for (int k = tid; k < n; k += 256) {
            const bool us = flag[k] > 0.0;
            if constexpr (ROBUST) wk[k] = us ? 1.0 : 0.0;
            rho[k] = us ? ws[(size_t)5 * ld + k] : __longlong_as_double((long long)kInfBits);   // Z* for sigma_min's median
        }
        if (a.K && n_us > 0) {
            lds_barrier();
            median_middles(rho, n, n_us, smp + kPoseMid, tid);
            lds_barrier();
            sigma_min = 0.5 * fmax(a.pitch_u / a.K[b * 4 + 0], a.pitch_v / a.K[b * 4 + 1]) * ((smp[kPoseMid] + smp[kPoseMid + 1]) * 0.5);
        }
        lds_barrier();
    }

    // the consensus start: the winner's j + 1, the rows that start at weight 1, the usable rows that start at 0
    int winner = 0, n_start = 0, n_zero0 = 0;
    if constexpr (CONSENSUS) {
        if (n_us >= 3) {
            winner = consensus_start<ROBUST, PoseThreePoint>(ws, ld, n, n_us, a.n_hyp, a.seed, 4.6851 * sigma_min,
                                                             rho + (ROBUST ? 2 : 1) * (size_t)ld, ROBUST ? wk : ws + (size_t)6 * ld,
                                                             n_start);
            if (winner) n_zero0 = n_us - n_start;
        }
    }

    PoseFit fit;
    pose_align<ROBUST>(ws, ld, n, n_us, sigma_min, a.n_iter, smp, rho, wk, fit, n_zero0);

    if (a.weights) {
        for (int k = tid; k < a.weights_stride; k += 256) {
            double w = 0.0;
            if (k < n) w = ROBUST ? wk[k] : (flag[k] > 0.0 ? 1.0 : 0.0);
            a.weights[(size_t)b * a.weights_stride + k] = w;
        }
    }
    if (tid != 0) return;
    const bool ok = fit.status == ST_OK;
    double v[6] = {0, 0, 0, 0, 0, 0};
    if (ok) pose_twist(a.lambda, fit, v);
#pragma unroll
    for (int i = 0; i < 6; ++i) vout[i] = v[i];
    a.pose_status[b] = fit.status;
    if (a.pose) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.pose[(size_t)b * 12 + i] = ok ? fit.R[i] : ((i & 3) == 0 ? 1.0 : 0.0);
#pragma unroll
        for (int i = 0; i < 3; ++i) a.pose[(size_t)b * 12 + 9 + i] = ok ? fit.t[i] : 0.0;
    }
    if (a.sigma) a.sigma[b] = fit.sigma;
    if (a.pose_info) {
        int32_t* pi = a.pose_info + (size_t)b * 8;
        pi[0] = n_us; pi[1] = fit.sweeps; pi[2] = fit.reweighted; pi[3] = fit.n_zero; pi[4] = fit.degenerate; pi[5] = holes;
        pi[6] = winner; pi[7] = n_start;
    }
}

int plan_pose(int max_rows, int n_iter, int n_hyp, PosePlan* plan) {
    if (!plan || max_rows < 1 || n_iter < 0 || n_iter > 16 || n_hyp < 0 || n_hyp > 4096) return -2;
    plan->robust = n_iter > 0;
    plan->consensus = n_hyp > 0;
    // rho and w of the robust form; the plain form with a consensus start keeps rho alone, for the median of Z* behind its cut-off
    const size_t per_row = plan->robust ? 2 : (plan->consensus ? 1 : 0);
    plan->lds = ((size_t)kPoseHead + per_row * max_rows + (plan->consensus ? consensus_lds_doubles(max_rows) : 0)) * sizeof(double);
    plan->lds_opt_in = plan->lds > 64 * 1024;
    return plan->lds > 160 * 1024 ? -3 : 0;
}

size_t pose_scratch_bytes(int n_pairs, int ld) { return (size_t)n_pairs * 7 * ld * sizeof(double); }

int launch_pose(const PoseArgs& a, hipStream_t stream) {
    if (a.n_pairs < 1 || a.ld < 1 || !a.ws || !a.v_pose || !a.pose_status || (a.weights && a.weights_stride < 0)) return -2;
    if (a.P ? (!a.Q || !a.usable) : (!a.selected || !a.s_uv || !a.feat || !a.info || !a.K || !a.zgoal || a.T < 1)) return -2;
    PosePlan p;
    if (int rc = plan_pose(a.ld, a.n_iter, a.n_hyp, &p)) return rc;
    if (p.consensus && !a.K && !(a.sigma_min > 0.0)) return -2;      // the cut-off T = 4.6851 sigma_min has to be positive
    if (p.robust) {
        return p.consensus ? launch_planned<pose_kernel<true, true>>(p, a, stream) : launch_planned<pose_kernel<true, false>>(p, a, stream);
    }
    return p.consensus ? launch_planned<pose_kernel<false, true>>(p, a, stream) : launch_planned<pose_kernel<false, false>>(p, a, stream);
}

}  // namespace vitvs
