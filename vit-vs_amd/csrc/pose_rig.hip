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
// The loop is then pose_kernel's with n = n_cams * ld: centroids and centred sums as quantities x 8 row slices, wave 0 solves,
// ROBUST re-weights with ONE median over the usable rows of all contributing cameras.
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
                const int tok = a.selected[r];
                if (tok >= 0 && tok < a.T) {
                    const double Z = a.feat[(size_t)r * 4 + 0], x = a.feat[(size_t)r * 4 + 1], y = a.feat[(size_t)r * 4 + 2];
                    const unsigned ds = a.zgoal[(size_t)i * a.zgoal_stride + tok];
                    f = (Z < 100.0 && ds != 0) ? 1 : -1;    // a hole in either depth drops the row
                    if (f > 0) {
                        const double fx = a.K[i * 4 + 0], fy = a.K[i * 4 + 1], cx = a.K[i * 4 + 2], cy = a.K[i * 4 + 3];
                        const double Zs = (double)ds / 1000.0;
                        const double xs = ((double)a.s_uv[(size_t)r * 4 + 0] - cx) / fx, ys = ((double)a.s_uv[(size_t)r * 4 + 1] - cy) / fy;
                        p[0] = Z * x; p[1] = Z * y; p[2] = Z;
                        g[0] = Zs * xs; g[1] = Zs * ys; g[2] = Zs;
                    }
                }
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
            rho[r] = f > 0 ? zs : __longlong_as_double((long long)kPoseInfBits);
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
            pose_middles(rho, n, n_us, smp + kPoseMid, tid);
            __syncthreads();
            sigma_min = 0.5 * pix * ((smp[kPoseMid] + smp[kPoseMid + 1]) * 0.5);
        }
        __syncthreads();
    }

    const int qid = tid & 31, slice = tid >> 5;
    int status = ST_OK, sweeps = 0, reweighted = 0, n_zero = 0, degenerate = 0;
    double sigma = 0.0;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, q[4] = {1, 0, 0, 0};
    const int N = ROBUST ? a.n_iter : 0;
    for (int it = 0;; ++it) {
        if (n_us - n_zero < 3) { status = ST_TOO_FEW; break; }
        // the weighted centroids: sw, sum w P', sum w Q'
        if (qid < 7) {
            double acc = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : (flag[r] > 0.0 ? 1.0 : 0.0);
                acc += qid == 0 ? w : w * ws[(size_t)(qid - 1) * n + r];
            }
            smp[slice * 32 + qid] = acc;
        }
        __syncthreads();
        if (tid < 7) {
            double s = 0.0, s0 = 0.0;
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) { s += smp[sl * 32 + tid]; s0 += smp[sl * 32]; }
            smp[kPoseCen + tid] = tid == 0 ? s : s / s0;
        }
        __syncthreads();
        // the centred sums: S [9] = sum w (P' - pc)(Q' - qc)^T, sum w |P' - pc|^2, sum w |Q' - qc|^2
        if (qid < 11) {
            const double* cen = smp + kPoseCen;
            const int ca = qid < 9 ? qid / 3 : 0, cb = qid < 9 ? qid % 3 : 0;
            double acc = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : (flag[r] > 0.0 ? 1.0 : 0.0);
                double term;
                if (qid < 9) {
                    term = w * (ws[(size_t)ca * n + r] - cen[1 + ca]) * (ws[(size_t)(3 + cb) * n + r] - cen[4 + cb]);
                } else {
                    const int o = qid == 9 ? 0 : 3;
                    const double d0 = ws[(size_t)o * n + r] - cen[1 + o], d1 = ws[(size_t)(o + 1) * n + r] - cen[2 + o],
                                 d2 = ws[(size_t)(o + 2) * n + r] - cen[3 + o];
                    term = w * ((d0 * d0 + d1 * d1) + d2 * d2);
                }
                acc += term;
            }
            smp[slice * 32 + qid] = acc;
        }
        __syncthreads();
        if (tid < 11) {
            double s = 0.0;
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) s += smp[sl * 32 + tid];
            smp[kPoseSum + tid] = s;
        }
        __syncthreads();
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
        __syncthreads();
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
                const double p0 = ws[k], p1 = ws[(size_t)n + k], p2 = ws[(size_t)2 * n + k];
                const double d0 = ws[(size_t)3 * n + k] - (((R[0] * p0 + R[1] * p1) + R[2] * p2) + t[0]);
                const double d1 = ws[(size_t)4 * n + k] - (((R[3] * p0 + R[4] * p1) + R[5] * p2) + t[1]);
                const double d2 = ws[(size_t)5 * n + k] - (((R[6] * p0 + R[7] * p1) + R[8] * p2) + t[2]);
                rho[k] = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            }
            __syncthreads();
            pose_middles(rho, n, n_us, smp + kPoseMid, tid);
            __syncthreads();
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
            __syncthreads();
            n_zero = iscr[2] + iscr[3] + iscr[4] + iscr[5];
            reweighted = it + 1;
        }
    }

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
    for (int i = 0; i < 6; ++i) a.v_rig[i] = v[i];
    *a.rig_status = status;
    if (a.pose) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.pose[i] = ok ? R[i] : ((i & 3) == 0 ? 1.0 : 0.0);
#pragma unroll
        for (int i = 0; i < 3; ++i) a.pose[9 + i] = ok ? t[i] : 0.0;
    }
    if (a.sigma) *a.sigma = sigma;
    if (a.rig_info) {
        int32_t* ri = a.rig_info;
        ri[0] = n_contrib; ri[1] = n_us; ri[2] = sweeps; ri[3] = reweighted; ri[4] = n_zero; ri[5] = degenerate; ri[6] = holes;
        ri[7] = worst;
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
