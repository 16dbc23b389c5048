// The visiting order of selection mode BEST (tests/select_ref.py): the tokens of the desired frame, mutual nearest
// neighbours first, ranked by similarity and taken round-robin over a c x c grid of image cells.  The law then runs on this order
// exactly as on a caller's (SEL_PRIORITY): the first num_pairs candidates met.
//
//   class_i = 0 for a mutual nearest neighbour (0 <= nn_1[i] < T and nn_2[nn_1[i]] == i), else 1
//   cell_i  = ((i / g) * c / g) * c + ((i % g) * c / g),  c = min(cells, g)
//   rho_i   = tokens of the same class and cell in front of i: larger sim_1, or the same sim_1 and a smaller id
//   order   = the tokens sorted ascending by (class, rho, -sim_1, id)
//
// One workgroup per frame pair, two sorts of 64-bit keys in LDS: by (class, cell, -sim, id), which puts every (class, cell) group
// in one run in rank order, so rho is the distance to the run's head; then by (class, rho, -sim, id).  Up to 256 tokens (one per
// thread) a sort is rank counting, the pattern of the law's median: every thread counts the keys below its own and writes its key
// to that slot, 5 barriers in all.  Beyond, it is a bitonic network on the next power of two of T with all-ones padding, a barrier
// per stage (measured at T = 196: 13.4 us as a network, 7.4 us counting; profiles/best_selection.txt).  Integers only; the keys are
// distinct, so every LDS and output slot has one writer per phase.
#include "common.h"
#include "kernels.h"

namespace vitvs {

constexpr int kSelectGroups = 512;    // (class, cell): 2 x 16 x 16
constexpr int kSelectCount = 256;     // up to this many tokens a sort is rank counting, one token per thread

// key of one sort: [63] class | [62..48] cell (8 bits used) or rho (15 bits) | [47..16] ~ordered similarity | [15..0] token id.
// A real key is never all ones (id < 2^14), so the padding sorts behind every token.
__device__ __forceinline__ unsigned long long select_key(unsigned cls, unsigned mid, unsigned nsim, unsigned id) {
    return ((unsigned long long)cls << 63) | ((unsigned long long)mid << 48) | ((unsigned long long)nsim << 16) | id;
}

// ascending bitonic sort of keys[0 .. n), n a power of two; every thread of the workgroup calls it (barriers inside)
__device__ __forceinline__ void sort_keys(unsigned long long* keys, int n, int tid, int nt) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += nt) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;   // the pair (lo, lo ^ j) with bit j clear in lo
                const unsigned long long a = keys[lo], b = keys[hi];
                const bool up = (lo & k) == 0;
                if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    }
}

// position of `key` in the ascending order of keys[0 .. n), n even: the number of keys below it (the all-ones padding never is).
// Every thread reads the same two keys at a time (one 16-byte LDS broadcast), eight reads in flight.
__device__ __forceinline__ int rank_of(const unsigned long long* keys, int n, unsigned long long key) {
    const ulonglong2* pairs = reinterpret_cast<const ulonglong2*>(keys);
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < (n >> 1); ++j) {
        const ulonglong2 k = pairs[j];
        rank += (int)(k.x < key) + (int)(k.y < key);
    }
    return rank;
}

// the (class, cell) group of a first-sort key as an index into head[]
__device__ __forceinline__ int group_of(unsigned long long key) {
    const int grp = (int)(key >> 48);                                         // class << 15 | cell
    return ((grp >> 15) << 8) | (grp & 255);
}

__global__ __launch_bounds__(1024) void best_order_kernel(const unsigned long long* __restrict__ row_best,
                                                          const unsigned long long* __restrict__ col_best, int T, int g, int c,
                                                          int n, int small, int32_t* __restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);   // [n]
    int* head = reinterpret_cast<int*>(keys + n);                             // [kSelectGroups] first sorted position of a group
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const unsigned long long* rb = row_best + (size_t)b * T;
    const unsigned long long* cb = col_best + (size_t)b * T;

    // 1. keys of the first sort; tail slots hold the padding
    for (int i = tid; i < n; i += nt) {
        unsigned long long key = ~0ull;
        if (i < T) {
            const unsigned long long kr = rb[i];
            const int n1 = (int)best_index(kr);
            const bool mutual = n1 >= 0 && n1 < T && (int)best_index(cb[n1]) == i;
            const int cell = ((i / g) * c / g) * c + ((i % g) * c / g);
            // the comparison is on fp32 values: -0 ranks as +0
            const unsigned nsim = ~ordered_key(best_value(kr) + 0.0f);
            key = select_key(mutual ? 0u : 1u, (unsigned)cell, nsim, (unsigned)i);
        }
        keys[i] = key;
    }
    __syncthreads();
    int32_t* out = order + (size_t)b * T;
    if (small) {
        // one token per thread (nt >= T); `sorted` is a second array of n keys behind head[].  Tail threads hold nothing and only
        // meet the barriers.
        unsigned long long* sorted = reinterpret_cast<unsigned long long*>(head + kSelectGroups);
        const bool live = tid < T;
        if (live) {
            const unsigned long long key = keys[tid];
            sorted[rank_of(keys, n, key)] = key;
        }
        __syncthreads();
        unsigned long long key = 0;
        if (live) {
            key = sorted[tid];
            if (tid == 0 || group_of(sorted[tid - 1]) != group_of(key)) head[group_of(key)] = tid;
        }
        __syncthreads();
        if (live) {
            const int rho = tid - head[group_of(key)];
            key = (key & 0x8000ffffffffffffull) | ((unsigned long long)rho << 48);
            keys[tid] = key;                                                  // (every first-sort key was read before the barriers)
        }
        __syncthreads();
        if (live) out[rank_of(keys, n, key)] = (int32_t)(key & 0xffffu);
        return;
    }
    sort_keys(keys, n, tid, nt);

    // 2. rho = sorted position - position of the group's head.  Heads first (reads only), then every slot rewrites itself.
    for (int p = tid; p < T; p += nt) {
        const int grp = group_of(keys[p]);
        if (p == 0 || group_of(keys[p - 1]) != grp) head[grp] = p;
    }
    __syncthreads();
    for (int p = tid; p < T; p += nt) {
        const unsigned long long key = keys[p];
        const int rho = p - head[group_of(key)];
        keys[p] = (key & 0x8000ffffffffffffull) | ((unsigned long long)rho << 48);
    }
    __syncthreads();
    sort_keys(keys, n, tid, nt);

    // 3. the order: the ids of the sorted keys
    for (int p = tid; p < T; p += nt) out[p] = (int32_t)(keys[p] & 0xffffu);
}

int plan_best_order(int T, int cells, BestOrderPlan* plan) {
    if (!plan || T <= 0 || cells < 1 || cells > 16) return -2;
    const int g = (int)floor(sqrt((double)T));
    if (g * g != T) return -2;
    BestOrderPlan& p = *plan;
    p.T = T; p.grid = g; p.cells = cells < g ? cells : g;
    p.n = 2;
    while (p.n < T && p.n < (1 << 30)) p.n <<= 1;
    p.small = T <= kSelectCount;
    if (p.small) {                    // one token per thread, two key arrays
        p.threads = p.n < 64 ? 64 : p.n;
        p.lds = (size_t)2 * p.n * 8 + (size_t)kSelectGroups * 4;
    } else {                          // one pair of keys per thread and stage, or several
        p.threads = p.n / 2 > 1024 ? 1024 : p.n / 2;
        p.lds = (size_t)p.n * 8 + (size_t)kSelectGroups * 4;
    }
    p.lds_opt_in = p.lds > 64 * 1024;
    // (a token id has 14 bits of the key; 2^14 keys are 128 KiB, so the LDS bound is the one that binds)
    return (p.lds > 160 * 1024 || T > (1 << 14)) ? -3 : 0;
}

int launch_best_order(const BestOrderPlan& p, int n_pairs, const unsigned long long* row_best, const unsigned long long* col_best,
                      int32_t* order, hipStream_t stream) {
    if (!p.lds || n_pairs <= 0 || !row_best || !col_best || !order) return -2;
    static std::atomic<unsigned long long> raised{0};
    if (p.lds_opt_in && (p.lds > 160 * 1024 || raise_lds_limit(reinterpret_cast<const void*>(best_order_kernel), 160 * 1024, raised)))
        return -3;
    launch(best_order_kernel, dim3(n_pairs), dim3(p.threads), p.lds, stream, row_best, col_best, p.T, p.grid, p.cells, p.n,
           p.small ? 1 : 0, order);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vitvs
