// The pose rig law: one rigid 3-D alignment of the matched points of ALL cameras of a rigid rig.
//   camera i has pose (R_i, t_i) in the rig frame, X_rig = R_i X_cam + t_i
//   P'_k = R_i P_k + t_i, Q'_k = R_i Q_k + t_i      the points of pose.hip, carried into the rig frame: the current
//                                                   ones in the current rig's frame, the goal ones in the goal rig's
//   (R, t) = argmin sum w |Q' - (R P' + t)|^2       over the whole stack (Horn's closed form, pose_core.h): the current rig in the
//                                                   goal rig's frame
//   v_rig = -lambda (R^T t, theta u)                a twist in the rig's own frame
// ONE launch of ONE 256-thread workgroup: building the points is a dozen loads per row and the solve loop is serial on one
// workgroup anyway, so nothing passes between workgroups.  Phase A strides the n_cams * ld stack rows (row i * ld + k: a fixed
// layout) over the threads and writes P', Q' and the flag into a [7][n_cams * ld] block of global memory that this workgroup alone
// writes and reads, behind __syncthreads(); rows a camera did not write and rows of cameras that do not contribute have flag 0.
// The loop is then pose_core.h's pose_align over the n = n_cams * ld rows, as in the pose law: centroids and centred sums as
// quantities x 8 row slices, wave 0 solves, ROBUST re-weights with ONE median over the usable rows of all contributing cameras.
#include "common.h"
#include "kernels.h"
#include "pose_core.h"

#pragma clang fp contract(off)

namespace vitvs {

template <bool ROBUST>
__global__ __launch_bounds__(256) void pose_rig_kernel(PoseRigArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smp[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = a.ld, n = a.n_cams * ld;
    double* ws = a.ws;                                      // P' [3][n] | Q' [3][n] | flag [n]: 1 usable, 0 not in the stack, -1 a hole
    int* iscr = reinterpret_cast<int*>(smp + kPoseInt);
    double* rho = smp + kPoseHead;
    double* wk = rho + n;

    // the cameras (every thread the same loop): who contributes, the largest status, the coarsest pixel of the contributing ones
    int n_contrib = 0, worst = 0;
    double pix = 0.0;
    for (int i = 0; i < a.n_cams; ++i) {
        const int cam = a.status ? a.status[i] : (int)ST_OK;
        const bool same = a.info && a.info[(size_t)i * 8 + 2] != 0;
        worst = max(worst, cam);
        if (cam == ST_OK && !same) {
            ++n_contrib;
            if (a.K) pix = fmax(pix, fmax(a.pitch_u / a.K[i * 4 + 0], a.pitch_v / a.K[i * 4 + 1]));
        }
    }
    if (n_contrib == 0) {                                   // nobody: v = 0, R = I, the largest camera status
        if (a.weights)
            for (int k = tid; k < a.n_cams * a.weights_stride; k += 256) a.weights[k] = 0.0;
        if (tid < 6) a.v_rig[tid] = 0.0;
        if (tid < 12 && a.pose) a.pose[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0 : 0.0;
        if (tid < 8 && a.rig_info) a.rig_info[tid] = tid == 7 ? worst : 0;
        if (tid < 18 && a.moments) a.moments[tid] = 0.0;
        if (tid == 0) {
            *a.rig_status = worst;
            if (a.sigma) *a.sigma = 0.0;
        }
        return;
    }

    // Phase A: the stack
    int n_us = 0, holes = 0;
    for (int r = tid; r < n; r += 256) {
        const int i = r / ld, k = r - i * ld;
        const int cam = a.status ? a.status[i] : (int)ST_OK;
        const bool same = a.info && a.info[(size_t)i * 8 + 2] != 0;
        int f = 0;
        double p[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        if (cam == ST_OK && !same) {
            if (a.P) {
                const int u = a.usable[r];
                f = u > 0 ? 1 : (u < 0 ? -1 : 0);
                if (f > 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) { p[c] = a.P[(size_t)r * 3 + c]; g[c] = a.Q[(size_t)r * 3 + c]; }
                }
            } else if (k < min(max(a.info[(size_t)i * 8 + 1], 0), ld)) {
                f = pose_handle_row(a, i, (size_t)r, p, g);
            }
        }
        const double zs = g[2];                             // Z* in the camera's frame, for sigma_min's median
        if (f > 0) {
            const double* E = a.rTc + (size_t)i * 12;
            double pr[3], gr[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pr[c] = ((E[3 * c] * p[0] + E[3 * c + 1] * p[1]) + E[3 * c + 2] * p[2]) + E[9 + c];
                gr[c] = ((E[3 * c] * g[0] + E[3 * c + 1] * g[1]) + E[3 * c + 2] * g[2]) + E[9 + c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { p[c] = pr[c]; g[c] = gr[c]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ws[(size_t)c * n + r] = p[c];
            ws[(size_t)(3 + c) * n + r] = g[c];
        }
        ws[(size_t)6 * n + r] = (double)f;
        if constexpr (ROBUST) {
            wk[r] = f > 0 ? 1.0 : 0.0;
            rho[r] = f > 0 ? zs : __longlong_as_double((long long)kInfBits);
        }
        n_us += f > 0;
        holes += f < 0;
    }
    n_us = wave_sum(n_us);
    holes = wave_sum(holes);
    if (lane == 0) { iscr[6 + wave] = n_us; iscr[10 + wave] = holes; }
    __syncthreads();                                        // (the points are global memory: full fence)
    n_us = iscr[6] + iscr[7] + iscr[8] + iscr[9];
    holes = iscr[10] + iscr[11] + iscr[12] + iscr[13];
    const double* flag = ws + (size_t)6 * n;

    double sigma_min = a.sigma_min;
    if constexpr (ROBUST) {
        if (a.K && n_us > 0) {
            median_middles(rho, n, n_us, smp + kPoseMid, tid);
            __syncthreads();
            sigma_min = 0.5 * pix * ((smp[kPoseMid] + smp[kPoseMid + 1]) * 0.5);
        }
        __syncthreads();
    }

    PoseFit fit;
    pose_align<ROBUST>(ws, n, n, n_us, sigma_min, a.n_iter, smp, rho, wk, fit);

    if (a.weights) {
        for (int idx = tid; idx < a.n_cams * a.weights_stride; idx += 256) {
            const int i = idx / a.weights_stride, k = idx - i * a.weights_stride;
            double w = 0.0;
            if (k < ld) w = ROBUST ? wk[i * ld + k] : (flag[i * ld + k] > 0.0 ? 1.0 : 0.0);
            a.weights[idx] = w;
        }
    }
    // the raw sums of the final weights, for a rig spread over ranks (every exit of the loop left a barrier behind its last reads
    // of the slices)
    if (a.moments) {
        const int qid = tid & 31, slice = tid >> 5;
        if (qid < 18) {
            double acc = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : (flag[r] > 0.0 ? 1.0 : 0.0);
                double term;
                if (qid == 0) {
                    term = w;
                } else if (qid < 7) {
                    term = w * ws[(size_t)(qid - 1) * n + r];
                } else if (qid < 16) {
                    const int ca = (qid - 7) / 3, cb = (qid - 7) % 3;
                    term = (w * ws[(size_t)ca * n + r]) * ws[(size_t)(3 + cb) * n + r];
                } else {
                    const int o = qid == 16 ? 0 : 3;
                    const double d0 = ws[(size_t)o * n + r], d1 = ws[(size_t)(o + 1) * n + r], d2 = ws[(size_t)(o + 2) * n + r];
                    term = w * ((d0 * d0 + d1 * d1) + d2 * d2);
                }
                acc += term;
            }
            smp[slice * 32 + qid] = acc;
        }
        __syncthreads();
        if (tid < 18) {
            double s = 0.0;
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) s += smp[sl * 32 + tid];
            a.moments[tid] = s;
        }
    }
    if (tid != 0) return;
    const bool ok = fit.status == ST_OK;
    double v[6] = {0, 0, 0, 0, 0, 0};
    if (ok) pose_twist(a.lambda, fit, v);
#pragma unroll
    for (int i = 0; i < 6; ++i) a.v_rig[i] = v[i];
    *a.rig_status = fit.status;
    if (a.pose) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.pose[i] = ok ? fit.R[i] : ((i & 3) == 0 ? 1.0 : 0.0);
#pragma unroll
        for (int i = 0; i < 3; ++i) a.pose[9 + i] = ok ? fit.t[i] : 0.0;
    }
    if (a.sigma) *a.sigma = fit.sigma;
    if (a.rig_info) {
        int32_t* ri = a.rig_info;
        ri[0] = n_contrib; ri[1] = n_us; ri[2] = fit.sweeps; ri[3] = fit.reweighted; ri[4] = fit.n_zero; ri[5] = fit.degenerate;
        ri[6] = holes; ri[7] = worst;
    }
}

constexpr int kPoseRigMaxRows = 1 << 24;    // stack rows: every index of the [7][n_cams * ld] block stays far inside an int

int plan_pose_rig(int n_cams, int ld, int n_iter, PoseRigPlan* plan) {
    if (!plan || n_cams < 1 || ld < 1 || n_iter < 0 || n_iter > 16) return -2;
    if ((long long)n_cams * ld > kPoseRigMaxRows) return -2;
    plan->robust = n_iter > 0;
    plan->lds = ((size_t)kPoseHead + (plan->robust ? (size_t)2 * n_cams * ld : 0)) * sizeof(double);
    plan->lds_opt_in = plan->lds > 64 * 1024;
    return plan->lds > 160 * 1024 ? -3 : 0;
}

size_t pose_rig_scratch_bytes(int n_cams, int ld) { return (size_t)n_cams * 7 * ld * sizeof(double); }

int launch_pose_rig(const PoseRigArgs& a, hipStream_t stream) {
    if (a.n_cams < 1 || a.ld < 1 || !a.rTc || !a.ws || !a.v_rig || !a.rig_status || (a.weights && a.weights_stride < 0)) return -2;
    if (a.P ? (!a.Q || !a.usable) : (!a.selected || !a.s_uv || !a.feat || !a.info || !a.K || !a.zgoal || a.T < 1)) return -2;
    PoseRigPlan p;
    if (int rc = plan_pose_rig(a.n_cams, a.ld, a.n_iter, &p)) return rc;
    static std::atomic<unsigned long long> raised{0};
    if (p.robust) {
        if (p.lds_opt_in && raise_lds_limit(reinterpret_cast<const void*>(pose_rig_kernel<true>), 160 * 1024, raised)) return -3;
        launch(pose_rig_kernel<true>, dim3(1), dim3(256), p.lds, stream, a);
    } else {
        launch(pose_rig_kernel<false>, dim3(1), dim3(256), p.lds, stream, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vitvs
