// The consensus start of the pose law (pose.hip) and the homography law (homography.hip): the seeded
// draw and the one phase that scores the hypotheses in parallel and hands the winner's consensus set to the law's loop
// (DESIGN.md 5i).  A law supplies a model (below) and the cut-off; tests/consensus_ref.py restates every line in the same order
// of arithmetic.
#pragma once
#include "common.h"
#include "robust_core.h"
#include "solve.h"

#pragma clang fp contract(off)

namespace vitvs {

// Behind the law's own dynamic LDS: the waves' best costs [4], as ints their best j [4] and their start weights at 1 [4] | as ints
// the usable rows in ascending order [rows, rounded up to even]
constexpr int kConsCells = 8;            // doubles of the cells in front of the usable-row list
constexpr size_t consensus_lds_doubles(int max_rows) { return (size_t)kConsCells + ((size_t)max_rows + 1) / 2; }

__device__ __forceinline__ unsigned consensus_mix(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The K (3 or 4) distinct positions of hypothesis j in a list of n_us usable rows, ascending (a row set gives one fit whatever the
// order it was drawn in): r_c = mix(mix(seed 0x9e3779b9 + j) + c) mod n_us for c = 0 .. 63, repeats rejected; false when 64 draws do
// not give K.
template <int K>
__device__ __forceinline__ bool consensus_draw(unsigned seed, int j, int n_us, int* pos) {
    static_assert(K == 3 || K == 4, "three- and four-row hypotheses");
    const unsigned base = consensus_mix(seed * 0x9e3779b9u + (unsigned)j);
    int p0 = -1, p1 = -1, p2 = -1, p3 = -1, cnt = 0;
    for (unsigned c = 0; c < 64u && cnt < K; ++c) {
        const int r = (int)(consensus_mix(base + c) % (unsigned)n_us);
        if (r == p0 || r == p1 || r == p2 || (K == 4 && r == p3)) continue;
        if (cnt == 0) p0 = r; else if (cnt == 1) p1 = r; else if (cnt == 2) p2 = r; else p3 = r;
        ++cnt;
    }
    if (cnt < K) return false;
    int t;
#define VITVS_CSWAP(a, b) if (b < a) { t = a; a = b; b = t; }
    if constexpr (K == 4) {
        VITVS_CSWAP(p0, p1) VITVS_CSWAP(p2, p3) VITVS_CSWAP(p0, p2) VITVS_CSWAP(p1, p3) VITVS_CSWAP(p1, p2)
        pos[0] = p0; pos[1] = p1; pos[2] = p2; pos[3] = p3;
    } else {
        VITVS_CSWAP(p0, p1) VITVS_CSWAP(p1, p2) VITVS_CSWAP(p0, p1)
        pos[0] = p0; pos[1] = p1; pos[2] = p2;
    }
#undef VITVS_CSWAP
    return true;
}

// The consensus phase, all 256 threads, behind Phase A's barrier and with n_us >= Model::kRows.  ws is the pair's workspace block,
// rows of `stride` doubles, its row Model::kFlagRow the flags (> 0: usable); rows [0, n) take part.  A Model names, all static:
//   kRows, kFlagRow, kFit                     the rows a hypothesis draws; the flags' row of the block; the doubles of a fit
//   bool fit(ws, stride, rows, out)           the closed-form fit of the kRows usable rows `rows` into out[kFit]; false: skipped
//   double residual_sq(fit, ws, stride, r)    the squared residual of row r under fit[kFit], >= +0 (or +inf)
// (The fit is a plain array here, not a member of the model: as a struct it cost the four kernels 6 to 11 instructions each and
// homography_kernel<true, true> 6 us a call at 8 x 24 rows, profiles/consensus_shared.txt.)
// Wave 0 compacts the usable rows into an ascending list.  Thread t scores the hypotheses t, t + 256, .. with the truncated cost
// C_j = sum over the usable rows, ascending, of min(q, T^2) (a skipped hypothesis costs +inf) and keeps its best (cost, j) in
// registers; costs are >= +0, so (cost bits, j) orders by integer compares and ties go to the smallest j.  One reduction: a
// butterfly within each wave, then 4 cells in LDS.  Every thread then fits the winner again and the start weights are 1 where
// sqrt(q) <= T and 0 elsewhere, into `start` (LDS for the robust form, the flags' row of the workspace for the plain one: there a
// usable row at weight 0 reads as an unusable one).  Returns the winner's j + 1 and the number of start weights at 1, or 0 and n_us
// when every hypothesis was skipped (nothing is written: the start without consensus).  The last barrier is the phase's own.
template <bool ROBUST, class Model>
__device__ __forceinline__ int consensus_start(const double* ws, int stride, int n, int n_us, int n_hyp, unsigned seed, double T,
                                               double* cons, double* start, int& n_start) {
    constexpr int K = Model::kRows;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long* cell_cost = reinterpret_cast<unsigned long long*>(cons);
    int* cell_j = reinterpret_cast<int*>(cons + 4);
    int* cell_ones = cell_j + 4;
    int* list = reinterpret_cast<int*>(cons + kConsCells);
    const double* flag = ws + (size_t)Model::kFlagRow * stride;
    if (wave == 0) {                                        // the usable rows in ascending order: wave 0, 64 rows a step
        int base = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            const bool f = k < n && flag[k] > 0.0;
            const unsigned long long bal = __ballot(f);
            if (f) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = k;
            base += __popcll(bal);
        }
    }
    lds_barrier();
    const double T2 = T * T;
    unsigned long long best = kInfBits;
    int best_j = 0x7fffffff;
    for (int j = tid; j < n_hyp; j += 256) {
        int pos[K], rows[K];
        double fit[Model::kFit];
        if (!consensus_draw<K>(seed, j, n_us, pos)) continue;
#pragma unroll
        for (int i = 0; i < K; ++i) rows[i] = list[pos[i]];
        if (!Model::fit(ws, stride, rows, fit)) continue;
        double cost = 0.0;
        for (int p = 0; p < n_us; ++p) {                    // (every lane reads the same row: one broadcast load per point)
            const double q = Model::residual_sq(fit, ws, stride, list[p]);
            cost += q < T2 ? q : T2;
        }
        const unsigned long long key = (unsigned long long)__double_as_longlong(cost);
        if (key < best) { best = key; best_j = j; }         // (j ascends: a tie keeps the smaller one)
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long oc = shfl_xor_u64(best, o);
        const int oj = __shfl_xor(best_j, o, WAVE);
        if (oc < best || (oc == best && oj < best_j)) { best = oc; best_j = oj; }
    }
    if (lane == 0) { cell_cost[wave] = best; cell_j[wave] = best_j; }
    lds_barrier();
    best = cell_cost[0]; best_j = cell_j[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const unsigned long long oc = cell_cost[w];
        const int oj = cell_j[w];
        if (oc < best || (oc == best && oj < best_j)) { best = oc; best_j = oj; }
    }
    if (best >= kInfBits) { n_start = n_us; return 0; }     // every hypothesis skipped: the same for every thread
    int pos[K], rows[K], ones = 0;
    double fit[Model::kFit];
    consensus_draw<K>(seed, best_j, n_us, pos);
#pragma unroll
    for (int i = 0; i < K; ++i) rows[i] = list[pos[i]];
    Model::fit(ws, stride, rows, fit);
    for (int k = tid; k < n; k += 256) {
        if (!(flag[k] > 0.0)) continue;
        const double w1 = sqrt(Model::residual_sq(fit, ws, stride, k)) <= T ? 1.0 : 0.0;
        start[k] = w1;
        ones += w1 > 0.0 ? 1 : 0;
    }
    ones = wave_sum(ones);
    if (lane == 0) cell_ones[wave] = ones;
    if constexpr (ROBUST) lds_barrier(); else __syncthreads();    // (the plain form's start weights are global memory: full fence)
    n_start = cell_ones[0] + cell_ones[1] + cell_ones[2] + cell_ones[3];
    return best_j + 1;
}

}  // namespace vitvs
