// The rig law: one twist for a rigid multi-camera rig from what the cameras' own laws left in memory.
//   v_ci = W_i v_r                       the rig twist v_r = (v, w), in the rig frame, as camera i's optical frame sees it
//   M = stack_i(L_i W_i), e = stack_i(e_i), v_r = -lambda * pinv(M) e      over the cameras whose status is ST_OK
// L_i, e_i: ServoArgs::L_ws of servo_kernel (zero-padded rows included, exactly as the camera's own law used them).
//
// One launch, one 256-thread workgroup per camera.  Workgroup b forms its rows m[r][j] = sum_c L[r][c] W[c][j] (fixed order
// c = 0 .. 5, no contraction), writes them and e into the stacked workspace behind the rows of the contributing cameras before
// it, and reduces its 27 normal-equation quantities (G = M^T M upper triangle, g = M^T e) in servo.hip's 27 x 8-slice scheme, in
// servo.hip's order of sums.
// The workgroups then meet through the in-launch fan-in of attention.hip's key ranges, the "sc1 loads in place of the acquire"
// form of MI355X_MICROARCH.md (Workgroup dispatch ... Valid forms), first row of its table.  Its four conditions here:
//   (1) every load of handed-off bytes (the cameras' `part` rows, the stacked rows for the Jacobi fallback) is a global_ sc1
//       load to registers (load_wt), by the last arriver's wave 0 alone; no workgroup reads the stack or `part` before that;
//   (2) every one of those bytes was stored sc1 (store_wt: 8-byte write-through stores);
//   (3) every storing wave drains its stores (s_waitcnt vmcnt(0)) and tid 0 adds to the one ticket behind the workgroup
//       barrier that follows those waits (relaxed, agent scope);
//   (4) hipMalloc memory, one workgroup per CU (n_cams <= kRigMaxCams), 8-byte sc1 stores and loads; the wave that added last
//       learns it from the add's return value and publishes it through an LDS word behind a workgroup barrier.
// Nobody waits or spins, so the workgroups need not be co-resident.  The last arriver resets the ticket (zero before the first
// launch only: captured graphs replay) and adds the cameras' sums in camera order 0 .. n - 1, not in arrival order: the result
// is bit-reproducible.  It then solves on wave 0: LDL^T of the 6 x 6 system, and behind a failed pivot the Jacobi SVD over a
// copy of the stacked rows (solve.h, the solvers of servo.hip).
// The same kernel as two plain launches (PHASE 1: the sums, PHASE 2: the solve) is the measured alternative.
#include "common.h"
#include "kernels.h"
#include "solve.h"

#pragma clang fp contract(off)

namespace vitvs {

constexpr int kRigTile = 256;   // rows per pass: one per thread

__device__ __forceinline__ void store_wt(double* p, double v) { store_out8<true>(p, __builtin_bit_cast(unsigned long long, v)); }
__device__ __forceinline__ double load_wt(const double* p) {
    return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT));
}

// PHASE 0: the whole law with the fan-in; 1: the cameras' sums only; 2: the merge and solve only (one workgroup)
template <int PHASE>
__global__ __launch_bounds__(256) void rig_kernel(RigArgs a) {
    // one LDS object: tile [7][kRigTile] | Gs [40 + 8 x 27] (solve.h's layout) | the "I am last" word
    __shared__ __attribute__((aligned(16))) double sm[7 * kRigTile + 256 + 2];
    double* tile = sm;
    double* Gs = sm + 7 * kRigTile;
    int* flag = reinterpret_cast<int*>(Gs + 256);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n_cams;

    // every workgroup recomputes the rows of the contributing cameras, its own offset among them and the rig's totals
    int off = 0, total = 0, used = 0, worst = 0, R = 0;
    for (int i = 0; i < n; ++i) {
        const int ri = min(max(a.rows[(size_t)i * a.rows_stride], 0), a.ld);
        const int st = a.status ? a.status[i] : (ri > 0 ? ST_OK : ST_TOO_FEW);
        const int eff = (st == ST_OK) ? ri : 0;
        if (i < b) off += eff;
        if (i == b) R = eff;
        total += eff;
        used += eff > 0 ? 1 : 0;
        worst = max(worst, st);
    }

    if constexpr (PHASE != 2) {
        double W[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) W[i] = a.W[(size_t)b * 36 + i];
        const double* Lb = a.L + (size_t)b * 7 * a.ld;
        const int qid = tid & 31, slice = tid >> 5;
        int ca = 0, cb = 6;
        if (qid < 21) {
            int q = qid;
            while (q >= 6 - ca) { q -= 6 - ca; ++ca; }
            cb = ca + q;
        } else {
            ca = min(qid - 21, 5);
        }
        double acc4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r0 = 0; r0 < R; r0 += kRigTile) {
            const int r = r0 + tid;
            if (r < R) {
                double l[7];
#pragma unroll
                for (int c = 0; c < 7; ++c) l[c] = Lb[(size_t)c * a.ld + r];
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    double m = 0.0;
#pragma unroll
                    for (int c = 0; c < 6; ++c) m += l[c] * W[c * 6 + j];
                    tile[j * kRigTile + tid] = m;
                    store_wt(a.stack + (size_t)j * a.cap + off + r, m);
                }
                tile[6 * kRigTile + tid] = l[6];
                store_wt(a.stack + (size_t)6 * a.cap + off + r, l[6]);
            }
            lds_barrier();
            // servo.hip's order of sums, row for row (kRigTile is a multiple of its 32-row step): row r belongs to slice r mod 8
            // and, while r + 24 < R, to chain (r / 8) mod 4; the last rows all go to chain 0.  With W = I one camera's G and g
            // are therefore its own law's, bit for bit.
            if (qid < 27) {
                const int end = min(r0 + kRigTile, R);
                int r = r0 + slice;
                for (; r + 24 < R && r < end; r += 32) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        acc4[u] += tile[ca * kRigTile + (r - r0) + 8 * u] * tile[cb * kRigTile + (r - r0) + 8 * u];
                }
                for (; r < end; r += 8) acc4[0] += tile[ca * kRigTile + (r - r0)] * tile[cb * kRigTile + (r - r0)];
            }
            lds_barrier();
        }
        if (qid < 27) Gs[40 + slice * 27 + qid] = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
        lds_barrier();
        if (tid < 28) {
            double s = (double)R;
            if (tid < 27) {
                s = 0.0;
#pragma unroll
                for (int sl = 0; sl < 8; ++sl) s += Gs[40 + sl * 27 + tid];
            }
            store_wt(a.part + (size_t)b * kRigPartDoubles + tid, s);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its stores ...
        if constexpr (PHASE == 1) return;
        __syncthreads();                                       // ... before the workgroup's one ticket
        if (tid == 0) {
            const int drawn = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (drawn == n - 1) __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
            *flag = drawn;
        }
        __syncthreads();
        if (*flag != n - 1) return;                            // another workgroup finishes the rig
    }
    if (wave != 0) return;

    // The last arriver, wave 0 from here.  The cameras' sums are read with sc1 loads, every byte of them (its own included:
    // nothing of this goes through this CU's L1), and added in camera order.
    if (lane < 28) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += load_wt(a.part + (size_t)i * kRigPartDoubles + lane);
        if (a.normal) a.normal[lane] = s;
        if (lane < 27) {
            Gs[40 + lane] = s;                                 // solve_ldlt adds eight slices: the sum and seven zeros
#pragma unroll
            for (int sl = 1; sl < 8; ++sl) Gs[40 + sl * 27 + lane] = 0.0;
        }
    }
    double xsol[6] = {0, 0, 0, 0, 0, 0};
    int sweeps = 0;
    if (total > 0) {
        sweeps = -1;
        if (!solve_ldlt(Gs, lane, xsol)) {
            // the rotations overwrite their operand: each lane copies the rows it alone reads and writes below (r = lane mod 64)
            for (int r = lane; r < total; r += 64)
#pragma unroll
                for (int c = 0; c < 7; ++c) a.work[(size_t)c * a.cap + r] = load_wt(a.stack + (size_t)c * a.cap + r);
            sweeps = solve_jacobi(a.work, a.cap, total, lane, xsol);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.v_rig[i] = total > 0 ? -a.lambda * xsol[i] : 0.0;
        *a.rig_status = total > 0 ? (int)ST_OK : max(worst, (int)ST_NO_CORRESPONDENCE);
        if (a.rig_info) {
            a.rig_info[0] = used; a.rig_info[1] = total; a.rig_info[2] = sweeps; a.rig_info[3] = n;
            a.rig_info[4] = worst; a.rig_info[5] = 0; a.rig_info[6] = 0; a.rig_info[7] = 0;
        }
    }
}

size_t rig_scratch_bytes(int n_cams, int ld) {
    return 256 + ((size_t)n_cams * kRigPartDoubles + (size_t)2 * 7 * n_cams * ld) * sizeof(double);
}

void rig_carve(void* scratch, int n_cams, int ld, RigArgs& a) {
    unsigned char* p = static_cast<unsigned char*>(scratch);
    a.ticket = reinterpret_cast<int*>(p);
    a.part = reinterpret_cast<double*>(p + 256);
    a.cap = n_cams * ld;
    a.stack = a.part + (size_t)n_cams * kRigPartDoubles;
    a.work = a.stack + (size_t)7 * a.cap;
}

int launch_rig(const RigArgs& a, hipStream_t stream, bool two_launches) {
    if (a.n_cams < 1 || a.n_cams > kRigMaxCams || a.ld < 1 || a.rows_stride < 1 || (long)a.cap < (long)a.n_cams * a.ld) return -2;
    if (!a.rows || !a.L || !a.W || !a.stack || !a.work || !a.part || !a.ticket || !a.v_rig || !a.rig_status) return -2;
    if (two_launches) {
        launch(rig_kernel<1>, dim3(a.n_cams), dim3(256), 0, stream, a);
        launch(rig_kernel<2>, dim3(1), dim3(256), 0, stream, a);
    } else {
        launch(rig_kernel<0>, dim3(a.n_cams), dim3(256), 0, stream, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the robust rig law --------------------------------------------------------------------------------------
// Tukey IRLS over the stacked system with ONE median over the live pairs of all contributing cameras: the rig law's launch shape
// and its fan-in, word for word (the four conditions of the header, with "all 256 threads of the last arriver, behind the
// workgroup barrier its wave 0 joins after the add has returned" in place of "wave 0 alone" in (1): the same row of the table
// allows both).  The cameras store their rows and e and nothing else: the first solve is weighted already (a zero-padded pair
// has weight 0), so no camera's own 27 sums are of use.  The last arriver copies the stack ONCE with sc1 loads, into LDS when
// n_cams * ld <= kRigRobustTile, else into `work` (which it alone writes and reads, plain accesses from there on), and runs
// the camera's robust loop on it, from the same functions: weighted_solve and pair_residuals (solve.h), median_middles and
// tukey_reweight (robust_core.h).  A pair that is not live carries rho = +inf from the start to the end: it ranks behind every live
// pair, takes weight 0 from the weight formula itself and is skipped by the residual pass.
// dynamic LDS, in doubles: Gs [256] (solve.h's layout; [28 .. 34) x, [34] [35] the two middle residuals) | 4: the ticket drawn
// and four counts as ints | tile [7][kRigRobustTile] when resident | rho [pairs] | w [pairs]
constexpr int kRigRobustHead = 256 + 4;

// rows (even) camera i contributes, its live pairs and its status
__device__ __forceinline__ int rig_robust_camera(const RigRobustArgs& ra, int i, int& lv, int& st) {
    const RigArgs& a = ra.r;
    const int ri = min(max(a.rows[(size_t)i * a.rows_stride], 0), a.ld) & ~1;
    st = a.status ? a.status[i] : (ri > 0 ? ST_OK : ST_TOO_FEW);
    lv = ra.live ? min(max(ra.live[(size_t)i * ra.live_stride], 0), ri >> 1) : (ri >> 1);
    const int eff = (st == ST_OK && lv > 0) ? ri : 0;
    if (eff == 0) lv = 0;
    return eff;
}

// RESIDENT: the stack's copy sits in LDS (the plan's lds_resident)
template <bool RESIDENT>
__global__ __launch_bounds__(256) void rig_robust_kernel(RigRobustArgs ra) {
    extern __shared__ __attribute__((aligned(16))) double smr[];
    const RigArgs& a = ra.r;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n_cams;
    constexpr bool resident = RESIDENT;
    double* Gs = smr;
    int* iscr = reinterpret_cast<int*>(smr + 256);              // [0] the ticket drawn, [1 .. 4] the waves' zero weights
    double* tile = smr + kRigRobustHead;
    double* rho = tile + (resident ? 7 * kRigRobustTile : 0);
    double* wk = rho + n * (a.ld >> 1);

    int off = 0, total = 0, used = 0, worst = 0, R = 0, n_live = 0;
    for (int i = 0; i < n; ++i) {
        int lv, st;
        const int eff = rig_robust_camera(ra, i, lv, st);
        if (i < b) off += eff;
        if (i == b) R = eff;
        total += eff;
        n_live += lv;
        used += eff > 0 ? 1 : 0;
        worst = max(worst, st);
    }

    // Phase A: this camera's rows of M = L W (the rig law's order of sums) and e, behind the contributing cameras before it
    if (R > 0) {
        double W[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) W[i] = a.W[(size_t)b * 36 + i];
        const double* Lb = a.L + (size_t)b * 7 * a.ld;
        for (int r = tid; r < R; r += 256) {
            double l[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) l[c] = Lb[(size_t)c * a.ld + r];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double m = 0.0;
#pragma unroll
                for (int c = 0; c < 6; ++c) m += l[c] * W[c * 6 + j];
                store_wt(a.stack + (size_t)j * a.cap + off + r, m);
            }
            store_wt(a.stack + (size_t)6 * a.cap + off + r, l[6]);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its stores ...
    __syncthreads();                                       // ... before the workgroup's one ticket
    if (tid == 0) {
        const int drawn = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (drawn == n - 1) __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        iscr[0] = drawn;
    }
    __syncthreads();
    if (iscr[0] != n - 1) return;                          // another workgroup finishes the rig

    // The last arriver, all four waves from here.  The one copy of the stack: every byte by an sc1 load to a register.
    const int rcap = resident ? kRigRobustTile : a.cap;
    double* Lc = resident ? tile : a.work;
    for (int c = 0; c < 7; ++c)
        for (int r = tid; r < total; r += 256) Lc[(size_t)c * rcap + r] = load_wt(a.stack + (size_t)c * a.cap + r);
    const int P = total >> 1;
    double sigma_min = ra.sigma_min;
    {
        int o = 0;
        double smin = 0.0;
        for (int i = 0; i < n; ++i) {
            int lv, st;
            const int eff = rig_robust_camera(ra, i, lv, st);
            for (int p = tid; p < (eff >> 1); p += 256) {
                wk[o + p] = p < lv ? 1.0 : 0.0;
                rho[o + p] = p < lv ? 0.0 : __longlong_as_double((long long)kInfBits);
            }
            if (eff > 0 && ra.K) smin = fmax(smin, 0.5 * fmax(ra.pitch_u / ra.K[i * 4 + 0], ra.pitch_v / ra.K[i * 4 + 1]));
            o += eff >> 1;
        }
        if (ra.K) sigma_min = smin;
    }
    __syncthreads();                                       // (the stack's copy may be global memory: full fence)

    double vout[6] = {0, 0, 0, 0, 0, 0};
    double sigma = 0.0;
    int sweeps = 0, reweighted = 0, n_zero = 0;
    if (total > 0) {
        const int N = ra.n_iter;
        for (int it = 0;; ++it) {
            normal_equation_slices(Lc, rcap, total, wk, Gs, tid);
            lds_barrier();
            if (wave == 0) {
                double* Lw = resident ? a.work : ra.work2;
                sweeps = weighted_solve(Lc, rcap, total, wk, Gs, Lw, a.cap, lane, a.lambda, vout);
            }
            if (it == N) break;
            lds_barrier();
            pair_residuals<true>(Lc, rcap, P, Gs, rho, tid);
            lds_barrier();
            median_middles(rho, P, n_live, Gs + 34, tid);
            lds_barrier();
            sigma = tukey_reweight<false>(rho, nullptr, P, Gs + 34, sigma_min, wk, nullptr, iscr + 1, tid);
            lds_barrier();
            n_zero = iscr[1] + iscr[2] + iscr[3] + iscr[4];
            reweighted = it + 1;
        }
    }
    if (ra.weights) {
        int o = 0;
        for (int i = 0; i < n; ++i) {
            int lv, st;
            const int eff = rig_robust_camera(ra, i, lv, st);
            for (int p = tid; p < ra.weights_stride; p += 256)
                ra.weights[(size_t)i * ra.weights_stride + p] = p < (eff >> 1) ? wk[o + p] : 0.0;
            o += eff >> 1;
        }
    }
    if (wave != 0) return;
    if (a.normal && lane < 28) a.normal[lane] = total > 0 ? (lane < 27 ? Gs[lane] : (double)total) : 0.0;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.v_rig[i] = vout[i];
        *a.rig_status = total > 0 ? (int)ST_OK : max(worst, (int)ST_NO_CORRESPONDENCE);
        if (ra.sigma) *ra.sigma = sigma;
        if (a.rig_info) {
            a.rig_info[0] = used; a.rig_info[1] = total; a.rig_info[2] = sweeps; a.rig_info[3] = n;
            a.rig_info[4] = worst; a.rig_info[5] = reweighted; a.rig_info[6] = n_zero; a.rig_info[7] = 0;
        }
    }
}

int plan_rig_robust(int n_cams, int ld, RigRobustPlan* plan) {
    if (!plan || n_cams < 1 || n_cams > kRigMaxCams || ld < 1) return -2;
    RigRobustPlan& p = *plan;
    p.lds_resident = (long)n_cams * ld <= kRigRobustTile;
    p.pairs = (int)std::min<long>((long)n_cams * (ld / 2), 1 << 28);
    p.lds = ((size_t)kRigRobustHead + (p.lds_resident ? 7 * kRigRobustTile : 0) + (size_t)2 * p.pairs) * sizeof(double);
    p.lds_opt_in = p.lds > 64 * 1024;
    return p.lds > 160 * 1024 ? -3 : 0;
}

size_t rig_robust_scratch_bytes(int n_cams, int ld) { return rig_scratch_bytes(n_cams, ld) + (size_t)7 * n_cams * ld * sizeof(double); }

void rig_robust_carve(void* scratch, int n_cams, int ld, RigRobustArgs& a) {
    rig_carve(scratch, n_cams, ld, a.r);
    a.work2 = a.r.work + (size_t)7 * a.r.cap;
}

int launch_rig_robust(const RigRobustArgs& ra, hipStream_t stream) {
    const RigArgs& a = ra.r;
    if (a.n_cams < 1 || a.n_cams > kRigMaxCams || a.ld < 1 || a.rows_stride < 1 || (long)a.cap < (long)a.n_cams * a.ld) return -2;
    if (ra.n_iter < 1 || ra.n_iter > 16 || (ra.live && ra.live_stride < 1) || (ra.weights && ra.weights_stride < 0)) return -2;
    if (!a.rows || !a.L || !a.W || !a.stack || !a.work || !ra.work2 || !a.ticket || !a.v_rig || !a.rig_status) return -2;
    RigRobustPlan p;
    if (int rc = plan_rig_robust(a.n_cams, a.ld, &p)) return rc;
    static std::atomic<unsigned long long> raised{0};
    if (p.lds_resident) {                                  // (at most 8 (260 + 7 * 384 + 384) bytes: no opt-in)
        launch(rig_robust_kernel<true>, dim3(a.n_cams), dim3(256), p.lds, stream, ra);
    } else {
        if (p.lds_opt_in && raise_lds_limit(reinterpret_cast<const void*>(rig_robust_kernel<false>), 160 * 1024, raised)) return -3;
        launch(rig_robust_kernel<false>, dim3(a.n_cams), dim3(256), p.lds, stream, ra);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vitvs
