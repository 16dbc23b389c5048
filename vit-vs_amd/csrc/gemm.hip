// Linear layers of the ViT forward on the gfx950 matrix cores (see gemm_core.h for the tile loop).
// Reference arithmetic being replaced (stock PyTorch ops issued by the reference):
//   qkv / proj Linear     dino_patch/attention.py:72, 79
//   fc1 -> GELU -> fc2     dino_patch/block.py:78-84 (Mlp, nn.GELU = erf form)
//   residual + LayerScale  dino_patch/block.py:90-96, 112-115
//   patch-embed Conv2d     dinov2_extractor.py:141, 259 (k = p, stride) as an im2col GEMM
#include <stdlib.h>

#include "gemm_core.h"
#include "kernels.h"
#include "probe.h"

namespace vitvs {

template <typename T, bool WT>
__device__ __forceinline__ void store4(T* dst, f32x4 v) {
    static_assert(!kSplit<T>, "f16x2 rows are addressed by logical column: store_x2");
    if constexpr (sizeof(T) == 4) {
        store_out<WT>(reinterpret_cast<float*>(dst), v);
    } else {
        const typename Vec16<T>::x4 h = {(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
        store_out<WT>(dst, h);
    }
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
// erf to ~1.5e-7 absolute (Abramowitz & Stegun 7.1.26; with fp32 rounding ~5e-7): four orders below bf16 output
// rounding and three below fp16's, a fraction of libm erff's instruction count.  Used when the layer's output is
// one of the plain 16-bit types, bf16 or fp16 (FAST_GELU below; BigStore::apply of gemm_big.hip holds a copy).
__device__ __forceinline__ float gelu_erf_fast(float v) {
    const float x = fabsf(v) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * x);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float e = 1.0f - poly * __expf(-x * x);
    return 0.5f * v * (1.0f + copysignf(e, v));
}

// Every epilogue is built inside the kernel from the same flat argument list (out, c0, c1, M, N, i0):
// flat leading kernel arguments are preloaded into SGPRs by the command processor
// (-amdgpu-kernarg-preload-count), a by-value struct would be fetched by the wave after it starts.
template <typename T>
struct EpiStore {
    T* out;
    const float* bias;
    int ldo;
    int gelu;
    __device__ __forceinline__ void set_slice(int) {}
    __device__ __forceinline__ static EpiStore make(void* out, const float* c0, const float*, int, int N, int i0) {
        return EpiStore{(T*)out, c0, N, i0};
    }
    __device__ __forceinline__ float4 column_terms(int n) const { return *reinterpret_cast<const float4*>(bias + n); }
    // staged epilogue (linear_kernel): the tile leaves through an LDS image as whole rows
    using Out = T;
    static constexpr bool STAGED = true;
    // bf16 and fp16 outputs take the fast erf (its error is orders below their output rounding; tests/test_gpu_epilogue_exact.py
    // holds both forms per element); fp32 and f16x2 keep fp32-class outputs: libm erff
    static constexpr bool FAST_GELU = sizeof(T) == 2 && !kSplit<T>;
    static constexpr int OUT_BYTES = kSplit<T> ? 4 : (int)sizeof(T);     // bytes per logical output column
    __device__ __forceinline__ f32x4 value(f32x4 v, float4 b) const {
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
        if (gelu) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = FAST_GELU ? gelu_erf_fast(v[i]) : gelu_erf(v[i]);
        }
        return v;
    }
    // first byte of logical column n0 (n0 % 32 == 0) of output row m
    __device__ __forceinline__ unsigned char* row_bytes(int m, int n0) const {
        return reinterpret_cast<unsigned char*>(out) + ((size_t)m * ldo + n0) * OUT_BYTES;
    }
    template <bool WT>
    __device__ __forceinline__ void store(int m, int n, f32x4 v, float4 b) const {
        v = value(v, b);
        if constexpr (kSplit<T>) store_x2<WT>(out + (size_t)m * ldo * 2, n, v);
        else store4<T, WT>(out + (size_t)m * ldo + n, v);
    }
};

struct EpiResidual {
    static constexpr bool STAGED = false;
    float* x;
    const float* bias;
    const float* ls;  // may be null
    int ld;
    __device__ __forceinline__ void set_slice(int) {}
    __device__ __forceinline__ static EpiResidual make(void* out, const float* c0, const float* c1, int, int N, int) {
        return EpiResidual{(float*)out, c0, c1, N};
    }
    __device__ __forceinline__ float4 column_terms(int n) const { return *reinterpret_cast<const float4*>(bias + n); }
    template <bool WT>
    __device__ __forceinline__ void store(int m, int n, f32x4 v, float4 b) const {
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
        if (ls) {
            const float4 g = *reinterpret_cast<const float4*>(ls + n);
            v[0] *= g.x; v[1] *= g.y; v[2] *= g.z; v[3] *= g.w;
        }
        float4* p = reinterpret_cast<float4*>(x + (size_t)m * ld + n);
        float4 r = *p;
        r.x += v[0]; r.y += v[1]; r.z += v[2]; r.w += v[3];
        *p = r;
    }
};

// Raw fp32 partial sums of one K slice (split-K): part[z][m][n]; bias / LayerScale / residual /
// LayerNorm are applied by residual_ln_kernel (elementwise.hip), which sums the slices in a fixed
// order, so the result does not depend on scheduling (no atomics).
struct EpiPartial {
    float* part;
    int M, N;
    __device__ __forceinline__ static EpiPartial make(void* out, const float*, const float*, int M, int N, int) {
        return EpiPartial{(float*)out, M, N};
    }
    __device__ __forceinline__ float4 column_terms(int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }
    __device__ __forceinline__ void set_slice(int z) { part += (size_t)z * M * N; }
    using Out = float;
    static constexpr bool STAGED = true;
    static constexpr int OUT_BYTES = 4;
    __device__ __forceinline__ f32x4 value(f32x4 v, float4) const { return v; }
    __device__ __forceinline__ unsigned char* row_bytes(int m, int n0) const {
        return reinterpret_cast<unsigned char*>(part + (size_t)m * N + n0);
    }
    template <bool WT>
    __device__ __forceinline__ void store(int m, int n, f32x4 v, float4) const {
        store4<float, WT>(part + (size_t)m * N + n, v);
    }
};

#ifdef VITVS_PROBE
// probe builds only (tools/gemm_probe.cpp): per-wave cycle-counter stamps of the kernel's phases (probe.h)
__device__ unsigned long long* g_gemm_probe;
extern "C" __attribute__((visibility("default"))) int vitvs_debug_set_gemm_probe(void* p) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_probe), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

#define VITVS_EPI_WT(BM) ((BM) < 128)
template <typename T, int BM, int BN, int KG, class Epi, int NS = 0>
__global__ __launch_bounds__(256 * KG) void linear_kernel(const T* __restrict__ A, const T* __restrict__ W, void* out,
                                                          const float* c0, const float* c1, int M, int N, int K,
                                                          int ks_i0) {
    // ks_i0 packs [31:24] K per split-K slice in k-tiles of 32 (fp32) / 64 (two-byte types; f16x2: 32 logical k) elements,
    // [23:19] e: f16x2 weights arrive multiplied by 2^e (api.hip upload_matrix), the sums leave multiplied by 2^-e,
    // [18] staged epilogue, [16] XCD map, [15:0] i0: one preloaded dword instead of gridDim (hidden kernel arguments the
    // wave would have to fetch) and an integer division.
    VITVS_IF_PROBE(unsigned long long ts_buf[8]; ts_buf[0] = __builtin_readcyclecounter();)
    unsigned long long* const ts = VITVS_PROBE_OR_NULL(ts_buf);   // per-phase stamps: null in the product build (folded away)
    using Tile = GemmTile<BM, BN, KG, NS>;
    Epi epi = Epi::make(out, c0, c1, M, N, ks_i0 & 0xffff);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned pk = (unsigned)ks_i0;
    const int kslice = (int)(pk >> 24) * (128 / (int)sizeof(T));
    int tx = blockIdx.x, ty = blockIdx.y, tz = blockIdx.z;
    if (pk & (1u << 16)) {
        // XCD map of the two-slice partial-sum launches (launch_one): a 1-D grid whose workgroup L runs on XCD L % 8; XCD x
        // takes K slice x / 4 and the column tiles of class x % 4, all row tiles of them.  A weight tile is then fetched by
        // ONE private L2 (every row tile that needs it is there) and an activation slice by four instead of eight.
        const int L = blockIdx.x, x = L & 7, r = L >> 3, ncq = (N / BN) >> 2;
        ty = r / ncq;
        tx = (x & 3) + 4 * (r - ty * ncq);
        tz = x >> 2;
    }
    epi.set_slice(tz);
    const int m0 = ty * BM, n0 = tx * BN;
    f32x4 acc[Tile::NT][Tile::MT];
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & 3;
    const int wm = wave & 1, wn = wave >> 1;
    const int kg = (KG == 2) ? k_group() : 0;
    // per-column epilogue terms (bias) are requested BEFORE the main loop: they are older than every tile
    // copy, so the counted waits are unaffected, and their memory round trip is off the epilogue's path
    float4 col[Tile::NT];
#pragma unroll
    for (int ni = 0; ni < Tile::NT; ++ni) col[ni] = epi.column_terms(min(n0 + wn * Tile::WN + ni * 16 + 4 * (lane >> 4), N - 4));
    gemm_mainloop<T, BM, BN, KG, NS>(A, W, K, K, M, N, m0, n0, tz * kslice, (tz + 1) * kslice, smem, acc, ts);
    VITVS_IF_PROBE(
        asm volatile("s_nop 0" ::"v"(acc[0][0][0]), "v"(acc[Tile::NT - 1][Tile::MT - 1][3]) : "memory");
        ts[4] = __builtin_readcyclecounter();
    )
    if constexpr (kSplit<T>) {
        const float ws = __uint_as_float((127u - ((pk >> 19) & 31u)) << 23);   // 2^-e, exact
#pragma unroll
        for (int ni = 0; ni < Tile::NT; ++ni)
#pragma unroll
            for (int mi = 0; mi < Tile::MT; ++mi) acc[ni][mi] *= ws;
    }
    if constexpr (BM == 64 && Epi::STAGED) {
        if (pk & (1u << 18)) {
            // Staged epilogue: a lane of the MFMA layout owns 4 consecutive columns of one row, so a wave's store instruction
            // writes 16 rows x 32 bytes (16-bit output) — four partial lines per row over the tile.  Here the tile goes through an
            // LDS image (the ring is free: every wave is past its last k-tile) and leaves as 16-byte pieces of whole rows:
            // consecutive lanes write consecutive bytes, whole 128-byte lines.
            using Out = typename Epi::Out;
            constexpr int ROWB = BN * Epi::OUT_BYTES, PITCH = ROWB + 16, CH = ROWB / 16;
            // one k-group: the barrier ends the last k-tile's reads.  Two k-groups: the ring has been free since the barrier of
            // the accumulator swap (gemm_mainloop) unless the swap area itself lives in the ring; each group stages the tiles it owns.
            if constexpr (KG == 1 || Tile::SWAP_ALIAS) __syncthreads();
#pragma unroll
            for (int ni = 0; ni < Tile::NT; ++ni)
#pragma unroll
                for (int mi = 0; mi < Tile::MT; ++mi) {
                    if (KG == 2 && tile_owner<Tile::NT, Tile::MT>(ni, mi) != kg) continue;
                    const f32x4 v = epi.value(acc[ni][mi], col[ni]);
                    const int cn = wn * Tile::WN + ni * 16 + 4 * (lane >> 4);      // tile-local column of v[0]
                    unsigned char* dst = smem + (wm * Tile::WM + mi * 16 + (lane & 15)) * PITCH +
                                         (kSplit<Out> ? 2 * x2_index(cn) : cn * (int)sizeof(Out));
                    if constexpr (kSplit<Out>) {       // the image has the row layout of memory: [hi of 32 columns | lo of them]
                        const Split4 h = split4(v);
                        *reinterpret_cast<f16x4*>(dst) = h.hi;
                        *reinterpret_cast<f16x4*>(dst + 64) = h.lo;
                    } else if constexpr (sizeof(Out) == 4) *reinterpret_cast<f32x4*>(dst) = v;
                    else {
                        const typename Vec16<Out>::x4 h = {(Out)v[0], (Out)v[1], (Out)v[2], (Out)v[3]};
                        *reinterpret_cast<typename Vec16<Out>::x4*>(dst) = h;
                    }
                }
            __syncthreads();
#pragma unroll
            for (int idx = threadIdx.x; idx < BM * CH; idx += 256 * KG) {
                const int r = idx / CH, ch = idx - r * CH;
                if (m0 + r < M) {
                    const u32x4 d = *reinterpret_cast<const u32x4*>(smem + r * PITCH + ch * 16);
                    store_out16<true>(epi.row_bytes(m0 + r, n0) + ch * 16, d);
                }
            }
            return;
        }
    }
#pragma unroll
    for (int ni = 0; ni < Tile::NT; ++ni) {
        const int n = n0 + wn * Tile::WN + ni * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int mi = 0; mi < Tile::MT; ++mi) {
            if (KG == 2 && tile_owner<Tile::NT, Tile::MT>(ni, mi) != kg) continue;
            const int m = m0 + wm * Tile::WM + mi * 16 + (lane & 15);
            if (m < M && n < N) epi.template store<VITVS_EPI_WT(BM)>(m, n, acc[ni][mi], col[ni]);   // 64-row tiles: one-wave launches
        }
    }
    VITVS_IF_PROBE(
        ts[5] = __builtin_readcyclecounter();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ts[6] = __builtin_readcyclecounter();
        if (lane == 0 && g_gemm_probe) {
            const int wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
            unsigned long long* dst = g_gemm_probe + ((size_t)wg * 8 + (threadIdx.x >> 6)) * 8;
            for (int i = 0; i < 7; ++i) dst[i] = ts[i];
        }
    )
}

static int k_tile(Precision p) { return plain16(p) ? 64 : 32; }   // logical k per 128-byte k-tile (f16x2: 32, hi and lo halves)

static bool shapes_ok(Precision p, int M, int N, int K) {
    const long long es = (long long)elem_size(p);   // operands are addressed with 32-bit byte offsets
    return M > 0 && N > 0 && K > 0 && (K % k_tile(p)) == 0 && (N % 64) == 0 && (long long)M * K * es < (1ll << 32) &&
           (long long)N * K * es < (1ll << 32);
}

// ---------------------------------------------------------------------------------------------------- the plan
// The rules below are plan_linear's; `hint` is the calling thread's updates in flight (g_updates_in_flight), read once there.

// K slices of a partial-sum layer.
static int splitk_slices(Precision p, int M, int N, int K, int hint) {
    const int bk = k_tile(p);
    // Many rows, narrow layer (8 frame pairs or a 518² input through proj / fc2): the 256x128 tiles of gemm_big.hip fill
    // well under half of the chip (78 tiles at 3152 x 768), so K is cut into the most slices that still fit one workgroup
    // per CU and leave >= 8 k-tiles per slice (3152 x 768 x 3072: 35 us on the tiles below -> 3 slices of 234 tiles).
    if (p != PREC_F32 && M >= 1024 && N % 128 == 0) {
        const long t128 = (long)((M + 255) / 256) * (N / 128);
        if (t128 >= 96) return 1;
        int pick = 1;
        for (int c : {2, 3, 4}) {
            if (K % (c * 64) != 0 || K / c < 8 * 64) continue;
            if (t128 * c <= 256) pick = c;
        }
        // Beside other queues' launches (vitvs_set_option "in_flight"), from ~2000 rows on, a third slice costs more in partial sums
        // (residual_ln is at the HBM rate there and does not overlap with anything) than it gains in fill: three in flight, same
        // box, 8 / 6 pairs 9108 -> 9578 / 8640 -> 9105 updates/s with two; 4 pairs (1576 rows, 4 slices) 7610 -> 7248: not there.
        if (hint >= 2 && pick > 2 && M >= 2048) pick = 2;
        if (pick > 1) return pick;
    }
    // The most K slices that still put at most one workgroup on every CU (each slice >= 4 k-tiles);
    // none if the tiles alone already cover the chip.
    const long tiles = (long)((M + 63) / 64) * (N / 64);
    int best = 1;
    for (int c : {2, 3, 4, 6, 8}) {
        if ((K % (c * bk)) != 0 || K / c < 4 * bk) continue;
        if (tiles * c <= 256) best = c;
    }
    // Beside other queues' launches (vitvs_set_option "in_flight") the chip is filled by THEIR workgroups: a third K slice
    // only adds partial sums for residual_ln to read (ViT-B/16 224², 4 in flight, same box: 3946 -> 4075 updates/s with 2; ONE slice:
    // 4301-4348 -> 4045-4091, round 5 — 84 workgroups with 48 k-tiles each are too long a chain; THREE slices again with four clean
    // queues: 4818-4841 -> 4420-4464).
    if (hint >= 2 && best > 2) best = 2;
    return best;
}

struct TileShape {
    int rows = 0, cols = 0;
};

// Which tile of gemm_big.hip for a many-row problem, or none (rows = 0: the tiles of gemm.hip).  Measured on MI355X
// (tools/big_ops [mid], random bf16 data, profiles/r02_big_ops*.txt): in its k-loop the 256x256 tile sustains ~1.5 PFLOP/s
// chip-wide, so what decides is how many tiles the busiest CU walks (workgroups are persistent, one per CU) and the fixed cost
// per tile (operand latency at the start, the output burst at the end: ~8 us at 6274 x 2304) — the rule below is that model
// with the relative tile costs measured.
static TileShape big_tile(Precision p, int M, int N, int K, int splits, bool partial, int hint) {
    if (p == PREC_F32 || splits < 1) return {};
    // f16x2 runs the same kernels on rows of 2 K fp16 (a k-tile = 32 logical k, three MFMAs per k-step): the tile rule below is
    // about rows, columns and rounds of workgroups, which do not change; only the k-tile count does
    const int kt = (p == PREC_X2 ? 2 : 1) * K;
    if (kt % (splits * 64) || kt / splits < 128 || kt / splits / 64 > 255) return {};
    // The 64-row tiles of gemm.hip keep the layers they cover in ONE round of <= 256 workgroups (788 x 2304: 7.9 us there,
    // 11.9 us on 256 x 128 tiles); where they need a second round the 256-row tiles win from 64 tiles up (985 x 2304: 18.4 vs
    // 11.9 us).  Between the tile families of gemm_big.hip the busiest CU's share decides (below).
    const long mt = (M + 63) / 64;
    for (int c : {128, 96, 64}) {
        if (partial && c != 64) continue;                         // the partial-sum kernels of gemm.hip are 64 wide
        if (N % c == 0 && mt * (N / c) * splits <= 256) return {};
    }
    // A little over one workgroup per CU, the 64 x 128 tiles of gemm.hip on their 2-stage ring (48 KB: three resident per CU, so
    // still one round) are ahead of every tile of gemm_big.hip: 788 x 3072 x 768 (312 workgroups) 11.4-12.5 us against 13.3 on
    // 192 x 128 tiles, 985 x 2304 (288) 11.3 / 11.8; end to end +1.6 % at 2 frame pairs.  From ~340 workgroups on the forward
    // does not gain (3 pairs, qkv 1182 x 2304: -0.4 % end to end although 11.7 / 11.8 us alone), so the rule stops at 320.
    if (!partial && splits == 1 && N % 128 == 0 && mt * (N / 128) <= 320) return {};
    const long ny = (M + 255) / 256;
    if (N % 128 != 0 || N / 128 > 255) return {};
    const long t128 = ny * (N / 128) * splits;
    if (t128 < (partial ? 96 : 64)) return {};
    // relative cost of one tile (k-loop share + the same fixed cost): 256 x 256 = 1, 256 x 192 = 0.85, 256 x 128 = 0.62
    // (3152 x 3072: 156 tiles of 256 x 256 25.1 us, 208 of 256 x 192 21.4 us, 312 of 256 x 128 29.6 us;
    //  6274 x 3072: 300 -> 51.6, 400 -> 41.9, 600 -> 44.6 us; 2740 x 3072 x 1024: 132 -> 23.9, 176 -> 20.6, 264 -> 30.3 us)
    auto rounds = [](long tiles) { return (double)((tiles + 255) / 256); };
    TileShape best{256, 128};
    double cost = 0.62 * rounds(t128);
    if (N % 192 == 0 && 0.85 * rounds(ny * (N / 192) * splits) < cost) { best = {256, 192}; cost = 0.85 * rounds(ny * (N / 192) * splits); }
    if (N % 256 == 0 && rounds(ny * (N / 256) * splits) < cost) { best = {256, 256}; cost = rounds(ny * (N / 256) * splits); }
    // 192-row x 128-column tiles: more, smaller tiles for the narrow layers — 6274 x 768 x 3072: 198 tiles 34.8 us against 150
    // of 256 x 128 37.4 us; 2740 x 1024 x 4096 in 2 K slices: 240 tiles 25.7 us against 176 -> 27.8 us; a tile costs 0.58 (its
    // waves' 96 x 32 sub-tiles read more LDS per FLOP than 64 x 64 ones, so it only pays while it stays in one round where
    // 256 x 128 leaves CUs idle: 3152 x 768 x 3072 in 3 slices, 306 tiles, 27.5 us against 234 -> 19.3 us)
    const long t192 = (long)((M + 191) / 192) * (N / 128) * splits;
    // (also ahead on wide layers while in one round: 788 .. 1576 x 3072: 13.2 .. 14.1 us against 14.8 .. 15.7; two rounds from
    //  1970 rows on: 24.8 against 16.2 us)
    if (0.58 * rounds(t192) < cost) { best = {192, 128}; cost = 0.58 * rounds(t192); }
    // 192 x 256, priced 0.9: 2740 x 4096 x 1024 (N is not a multiple of 192): 240 tiles 27.6 us against 176 of 256 x 256
    // -> 29.8 us; level with 256 x 192 where that applies (3152 x 3072: 21.7 / 21.6 us)
    if (N % 256 == 0 && 0.9 * rounds((long)((M + 191) / 192) * (N / 256) * splits) < cost) best = {192, 256};
    // Everything above balances ONE launch over the chip.  Beside other queues' launches (vitvs_set_option "in_flight") the
    // other queues' workgroups fill what a launch leaves idle, and the tile with the fewest operand bytes per FLOP wins: three
    // updates in flight, same box, 256 x 256 for every layer it divides: 8 / 6 / 4 pairs 8607 -> 9249 / 7980 -> 8730 / 7385 -> 7760
    // updates/s, ViT-B/8 448² 438 -> 460, ViT-L/14 518² 731 -> 793 (3 pairs, 1182 rows = 4.6 row tiles: 6787 -> 6664, hence the bound).
    if (hint >= 2 && N % 256 == 0 && M >= 1536) best = {256, 256};
    return best;
}

// Many-row problems (many frame pairs, 448² / 518² inputs): 128x128 tiles halve the LDS and L2 bytes per MFMA.
static bool big_problem(int M, int N, int splits) {
    // >= 256 tiles: with 2 workgroups per CU that is one round on every CU or more (measured: 294 tiles -12 %, 176 tiles
    // +37 % against 64x64 tiles)
    return splits == 1 && (N % 128) == 0 && (long)((M + 127) / 128) * (N / 128) >= 256;
}

// 64-row tiles.  In the one-frame-pair regime a launch cannot fill the chip, and a second wave of
// workgroups costs more than bigger tiles save (measured: 336 workgroups of 64x64 ran 2.4 us longer than
// 252), so: the column-tile width with the MOST workgroups that still fit the 256 CUs; if even the
// widest tile needs more than 256 workgroups the problem is large and the widest tile wins.  Two
// k-groups (8 waves, intra-workgroup split-K) whenever one workgroup per CU is all there is.
struct TilePlan {
    int bn, kg;
};
static TilePlan plan_tiles(int M, int N, int nk_per_slice, int splits, bool fixed64, int hint) {
    const long mt = (M + 63) / 64;
    int bn = 64;
    if (!fixed64) {
        long best = -1;
        for (int c : {128, 96, 64}) {
            if (N % c) continue;
            const long wgs = mt * (N / c);
            if (wgs <= 256 && wgs > best) { best = wgs; bn = c; }
        }
        if (best < 0) bn = (N % 128 == 0) ? 128 : 64;
        // (Measured in round 5 and not kept: beside other queues' launches a wider column tile for these one-round launches — fewer
        //  re-reads of the activation rows, fewer and fatter workgroups — 96 / 128 columns wherever they divide: bf16 3942 -> 3969 /
        //  3748 updates/s with three in flight, f16x2 2402 -> 2311 / 2067; again with four in flight and nothing on a fifth queue: bf16
        //  4818-4841 -> 4828-4846 / 4452-4457, f16x2 2593-2636 -> 2630-2658 / 2357: 96 inside the noise, 128 -8 %.)
    }
    const long wgs = mt * (N / bn) * splits;
    // Alone on the chip a one-round launch wants its serial k-loop short: two k-groups (8 waves, 112-144 KB of LDS, one
    // workgroup per CU).  Beside the launches of other queues (several updates in flight, vitvs_set_option) that footprint
    // keeps a second launch's workgroups off the CU until the first has left; 4-wave workgroups (64-80 KB) let two launches
    // share it: ViT-B/16 224², 3 updates in flight 3113 -> 3392 updates/s, but 2220 -> 2078 on one stream (same box,
    // profiles/r03_notes.md section 5), hence by the caller's hint and not by default.
    int kg = (hint < 2 && wgs <= 256 && nk_per_slice >= 4 && nk_per_slice % 2 == 0) ? 2 : 1;
    return TilePlan{bn, kg};
}

// Ring depth of a one-k-group 64-row launch.  Up to one workgroup per CU the deep ring (4 stages) hides the operand latency
// of the only workgroup there is.  Beyond that the LDS footprint sets how many workgroups a CU holds at once, and the other
// resident workgroups hide the latency instead (bf16, us with 4 / 3 / 2 stages; weights rotating through 19 MB | 600 MB):
//   64 x 64  (64 / 48 / 32 KB: 2 / 3 / 5 per CU)  1576 x 768 x 768, 300 workgroups:  6.1 /  6.0 /  7.6 |  7.1 /  7.3 / 10.7
//                                                 3152 x 768 x 768, 600:            12.0 / 11.5 / 10.3 | 12.1 / 11.6 / 12.0
//                                                 2740 x 1024 x 1024, 688:          14.8 / 13.1 / 12.4 | 15.4 / 14.7 / 15.4
//   64 x 128 (96 / 72 / 48 KB: 1 / 2 / 3 per CU)   788 x 3072 x 768, 312:           20.3 / 12.2 / 11.4 | 20.7 / 13.0 / 15.6
//                                                  985 x 2304 x 768, 288:           18.4 / 11.1 / 11.3 | 18.8 / 11.9 / 13.7
// In the forward (kernel trace, same box): 8-pair proj 11.40 / 11.47 / 11.31 us, 2-pair fc1 19.8 / 13.5 / 12.2 us; end to end
// against 4 stages everywhere: 8 pairs +0.9 ... +1.3 % with 3 or 2 stages, 2 pairs +1.6 % (profiles/r03_notes.md).
static int ring_stages(int bn, long wgs) {
    if (wgs <= 256) return 0;                 // the tile's default
    if (bn == 128) return 2;
    return wgs <= 512 ? 3 : 2;
}

LinearPlan plan_linear(Precision p, int M, int N, int K, LinearEpi epi, int splits, bool big_family, int rows, int cols) {
    const int hint = g_updates_in_flight;
    LinearPlan pl;
    pl.prec = p; pl.epi = epi; pl.M = M; pl.N = N; pl.K = K;
    const bool partial = epi == EPI_PARTIAL;
    pl.splits = !partial ? 1 : splits > 0 ? splits : splitk_slices(p, M, N, K, hint);
    const int s = pl.splits;
    if (!shapes_ok(p, M, N, K) || (K % (s * k_tile(p))) != 0) return pl;
    // (the residual epilogue never takes the tiles of gemm_big.hip: it has no kernel there)
    const TileShape big = rows || !big_family || epi == EPI_RESIDUAL ? TileShape{} : big_tile(p, M, N, K, s, partial, hint);
    if (rows) {   // a forced tile
        const bool known = rows == 128 ? cols == 128 && plain16(p)
                                       : p != PREC_F32 && (rows == 256 ? cols == 256 || cols == 192 || cols == 128
                                                                       : rows == 192 && (cols == 256 || cols == 128));
        if (!known || N % cols) return pl;
        pl.big = rows != 128;
        pl.rows = rows; pl.cols = cols;
    } else if (big.rows) {
        pl.big = true;
        pl.rows = big.rows; pl.cols = big.cols;
    } else if (big_problem(M, N, s)) {
        pl.rows = pl.cols = 128;
    } else {   // the partial sums and the residual epilogue are 64 wide (fewer instantiations)
        const TilePlan tp = plan_tiles(M, N, K / s / k_tile(p), s, epi != EPI_STORE, hint);
        pl.rows = 64; pl.cols = tp.bn; pl.kgroups = tp.kg;
        if (tp.kg == 1) pl.stages = ring_stages(tp.bn, (long)((M + 63) / 64) * (N / tp.bn) * s);
    }
    // The XCD map (linear_kernel) is for the two-slice partial-sum launches only (their i0 field is unused, bit 16 of the packed
    // argument is free).  Beside other queues' launches the narrow layers are bound by what their private L2s fetch, not by
    // latency (fc2 at three queues 4.48 -> 3.67 us per launch, 3932 -> 4072 updates/s); alone, XCD balance comes first (round 1:
    // the map lost).  (A column-class map for the one-slice launches — qkv's 36 column tiles over 8 XCDs — lost: 3.13 -> 3.37 us.)
    pl.xcd_map = !pl.big && partial && s == 2 && (N / pl.cols) % 4 == 0 && hint >= 2;
    return pl;
}

// ---------------------------------------------------------------------------------------------------- the launch
struct EpiArgs {   // host image of the flat epilogue arguments
    void* out;
    const float* c0;
    const float* c1;
    int i0;
    int wexp = 0;   // f16x2: the weights carry 2^wexp (linear_kernel)
};

template <typename T, int BN, int KG, class Epi, int BM = 64, int NS = 0>
static int launch_one(const LinearPlan& pl, const T* A, const T* W, int K, const EpiArgs& e, hipStream_t stream) {
    using Tile = GemmTile<BM, BN, KG, NS>;
    static std::atomic<unsigned long long> raised{0};   // > 64 KiB of dynamic LDS needs the opt-in attribute, per device
    if (raise_lds_limit(reinterpret_cast<const void*>(&linear_kernel<T, BM, BN, KG, Epi, NS>), Tile::LDS_BYTES, raised)) return -1;
    const int M = pl.M, N = pl.N, splits = pl.splits;
    dim3 grid(N / BN, (M + BM - 1) / BM, splits);
    constexpr int KU = 128 / (int)sizeof(T);   // elements per k-tile (f16x2: K counts fp16, two per logical k)
    const int kslice = K / splits;
    if (kslice % KU != 0 || kslice / KU > 255 || splits > 15 || e.i0 < 0 || e.i0 > 0xffff || e.wexp < 0 || e.wexp > 31) return -2;
    // Staged epilogue, always on for 64-row tiles.  4-wave workgroups: measured faster alone and side by side (qkv 6.00 -> 5.11
    // us alone, 3.07 -> 2.81 at three queues; fc1 8.62 -> 7.16, 3.99 -> 3.39; 2 pairs +3 % on one stream and +10 % with three
    // updates in flight; never slower).  8-wave workgroups (two k-groups, the one-stream plan): +1.4 % updates/s on one stream
    // (2202 -> 2233, three interleaved rounds).
    unsigned flags = BM == 64 ? 1u << 18 : 0u;
    if (pl.xcd_map) {
        grid = dim3(grid.x * grid.y * 2, 1, 1);
        flags |= 1u << 16;
    }
    launch(linear_kernel<T, BM, BN, KG, Epi, NS>, grid, dim3(Tile::THREADS), Tile::LDS_BYTES, stream, A, W, e.out, e.c0, e.c1,
           M, N, K, (int)(((unsigned)(kslice / KU) << 24) | ((unsigned)e.wexp << 19) | flags | (unsigned)e.i0));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <typename T, int BN, class Epi>
static int launch_ring(const LinearPlan& pl, const T* A, const T* W, int K, const EpiArgs& e, hipStream_t stream) {
    if (pl.kgroups == 2) return launch_one<T, BN, 2, Epi>(pl, A, W, K, e, stream);
    if constexpr (BN != 96) {   // (96 columns are picked only where they cover the layer in one round: the default ring)
        if (pl.stages == 3) return launch_one<T, BN, 1, Epi, 64, 3>(pl, A, W, K, e, stream);
        if (pl.stages == 2) return launch_one<T, BN, 1, Epi, 64, 2>(pl, A, W, K, e, stream);
    }
    return launch_one<T, BN, 1, Epi>(pl, A, W, K, e, stream);
}

// 128 x 128 for every epilogue; 64 rows by 64 columns for every epilogue, by 96 / 128 for the store only
template <typename T, class Epi>
static int launch_tile(const LinearPlan& pl, const T* A, const T* W, int K, const EpiArgs& e, hipStream_t stream) {
    if (pl.rows == 128 && pl.cols == 128) return launch_one<T, 128, 1, Epi, 128>(pl, A, W, K, e, stream);
    if (pl.rows != 64) return -2;
    if (pl.cols == 64) return launch_ring<T, 64, Epi>(pl, A, W, K, e, stream);
    if constexpr (std::is_same<Epi, EpiStore<T>>::value) {
        if (pl.cols == 96) return launch_ring<T, 96, Epi>(pl, A, W, K, e, stream);
        if (pl.cols == 128) return launch_ring<T, 128, Epi>(pl, A, W, K, e, stream);
    }
    return -2;
}

template <typename T>
static int launch_typed(const LinearPlan& pl, const T* A, const T* W, const float* bias, const float* ls, void* out, int K,
                        int gelu, hipStream_t stream, int wexp) {
    if (pl.big) {
        if constexpr (std::is_same<T, float>::value) return -2;
        else return launch_linear_big<T>(pl, A, W, bias, out, K, gelu, stream, wexp);
    }
    if (pl.epi == EPI_PARTIAL) return launch_tile<T, EpiPartial>(pl, A, W, K, EpiArgs{out, nullptr, nullptr, 0, wexp}, stream);
    if (pl.epi == EPI_RESIDUAL) return launch_tile<T, EpiResidual>(pl, A, W, K, EpiArgs{out, bias, ls, 0, wexp}, stream);
    return launch_tile<T, EpiStore<T>>(pl, A, W, K, EpiArgs{out, bias, nullptr, gelu, wexp}, stream);
}

int launch_linear(const LinearPlan& pl, const void* A, const void* W, const float* bias, void* out, int gelu,
                  hipStream_t stream, int wexp, const float* ls) {
    if (!pl.rows) return -2;
    switch (pl.prec) {
    case PREC_X2: return launch_typed(pl, (const hx2*)A, (const hx2*)W, bias, ls, out, 2 * pl.K, gelu, stream, wexp);
    case PREC_F32: return launch_typed(pl, (const float*)A, (const float*)W, bias, ls, out, pl.K, gelu, stream, 0);
    case PREC_F16: return launch_typed(pl, (const f16*)A, (const f16*)W, bias, ls, out, pl.K, gelu, stream, 0);
    default: return launch_typed(pl, (const bf16*)A, (const bf16*)W, bias, ls, out, pl.K, gelu, stream, 0);
    }
}

}  // namespace vitvs
