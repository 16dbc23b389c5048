// Internal launch interface between the C-ABI layer (api.cpp) and the HIP kernels.
// All pointers are device pointers; every launch is asynchronous on `stream`.
#pragma once
#include <atomic>
#include <vector>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

namespace vitvs {

int fail_hip(hipError_t e, const char* what, const char* file, int line);

#define VITVS_HIP_CHECK(expr)                                                          \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) return ::vitvs::fail_hip(_e, #expr, __FILE__, __LINE__); \
    } while (0)

// Kernel timing: when api.hip's Span arms `g_launch_timing`, the NEXT launch goes through
// hipExtLaunchKernelGGL, which stamps the two events with the dispatch's own begin / end times (what
// rocprofv3 --kernel-trace reports), so hipEventElapsedTime(start, stop) is that kernel's duration.
struct LaunchTiming {
    hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local LaunchTiming g_launch_timing;

template <typename F, typename... Args>
inline void launch(F kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
    if (g_launch_timing.start) {
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, g_launch_timing.start, g_launch_timing.stop, 0,
                              args...);
        g_launch_timing = LaunchTiming{};
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    }
}

// Updates the calling handle expects to run beside its own (vitvs_set_option "in_flight"; set by api.hip around a handle's
// launches, 1 otherwise).  From 2 on the one-round GEMM launches of gemm.hip use 4-wave workgroups (plan_linear), and the
// long-sequence attention keeps whole query blocks (plan_attention).
extern thread_local int g_updates_in_flight;

// The HIP device the calling thread's current entry point runs on (set by the C-ABI layer's DeviceScope; api.hip).
extern thread_local int g_current_device;
inline int current_device() {
    if (g_current_device < 0) (void)hipGetDevice(&g_current_device);
    return g_current_device;
}
// Kernels that need more than 64 KiB of dynamic LDS must opt in with hipFuncSetAttribute, and the attribute is kept per
// (function, DEVICE): `done` holds one bit per device for one kernel instantiation.
inline int raise_lds_limit(const void* fn, int bytes, std::atomic<unsigned long long>& done) {
    const int dev = current_device();
    if (dev < 0 || dev >= 64) return -1;
    if ((done.load(std::memory_order_relaxed) >> dev) & 1ull) return 0;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return -1;
    done.fetch_or(1ull << dev, std::memory_order_relaxed);
    return 0;
}
// The launch of a follow-on law from its plan, one 256-thread workgroup per pair: `kernel` is the instantiation the plan's booleans
// name, and the opt-in flag is that instantiation's own.  -3: the opt-in failed; -1: the launch did.
template <auto kernel, class Plan, class Args>
inline int launch_planned(const Plan& p, const Args& a, hipStream_t stream) {
    static std::atomic<unsigned long long> raised{0};
    if (p.lds_opt_in && raise_lds_limit(reinterpret_cast<const void*>(kernel), 160 * 1024, raised)) return -3;
    launch(kernel, dim3(a.n_pairs), dim3(256), p.lds, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// operand type of the GEMMs / attention; fp32 accumulate.  PREC_X2 = split-f16 (common.h hx2): every operand is an fp16
// hi / lo pair, rows are [hi of 32 columns | lo of the same 32] per 64 fp16, three f16 MFMAs per k-step: fp32-class results
enum Precision : int { PREC_F32 = 0, PREC_BF16 = 1, PREC_F16 = 2, PREC_X2 = 3 };

inline size_t elem_size(Precision p) { return (p == PREC_F32 || p == PREC_X2) ? 4 : 2; }   // bytes per LOGICAL element
inline bool plain16(Precision p) { return p == PREC_BF16 || p == PREC_F16; }

// ---- gemm.hip / gemm_big.hip: linear layers ----------------------------------------------------------
//   EPI_STORE    out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]); A, W, out in precision p; gelu: erf GELU.
//   EPI_PARTIAL  split-K form for the narrow (N = D) layers: part[z][m][n] = sum over K slice z of A[m][k] W[n][k], fp32,
//                z < splits; finished by launch_residual_ln / launch_embed_ln with the same slice count.
//   EPI_RESIDUAL x[m][n] += ls[n] * (sum_k A[m][k] W[n][k] + bias[n]); x fp32 residual stream, ls may be null.
// wexp (PREC_X2 only, 0 .. 31): W holds the weights times 2^wexp (so that their lo halves are normal fp16 numbers); the
// kernel multiplies the sums by 2^-wexp before the epilogue.
enum LinearEpi : int { EPI_STORE = 0, EPI_PARTIAL = 1, EPI_RESIDUAL = 2 };

// One linear layer's launch, decided by plan_linear and carried out by launch_linear.
struct LinearPlan {
    Precision prec = PREC_F32;
    LinearEpi epi = EPI_STORE;
    int M = 0, N = 0, K = 0;
    bool big = false;       // the linear_big_kernel tiles of gemm_big.hip, else the linear_kernel tiles of gemm.hip
    int rows = 0, cols = 0; // the tile; rows = 0: the shape cannot be launched
    int kgroups = 1;        // linear_kernel: 1 or 2 k-groups of 4 waves
    int stages = 0;         // linear_kernel, 64 rows, one k-group: ring stages (0: the tile's default)
    int splits = 1;         // K slices (EPI_PARTIAL; set even when rows = 0)
    bool xcd_map = false;   // linear_kernel: the XCD map of the two-slice partial-sum launches
};
// The plan under the calling thread's hint of updates in flight (g_updates_in_flight).  splits = 0: the library's slice count
// (EPI_PARTIAL; the other epilogues have one slice).  big_family = false: the tiles of gemm.hip only.  rows, cols != 0: that tile
// (128 x 128 of gemm.hip; 256 x 256 / 192 / 128 or 192 x 128 / 256 of gemm_big.hip) whatever the rule would pick.
LinearPlan plan_linear(Precision p, int M, int N, int K, LinearEpi epi, int splits = 0, bool big_family = true, int rows = 0,
                       int cols = 0);
int launch_linear(const LinearPlan& plan, const void* A, const void* W, const float* bias, void* out, int gelu,
                  hipStream_t stream, int wexp = 0, const float* ls = nullptr);
// gemm_big.hip's part of launch_linear, for T = hx2 (K counts fp16 per row), bf16, f16
template <typename T>
int launch_linear_big(const LinearPlan& plan, const T* A, const T* W, const float* bias, void* out, int K, int gelu,
                      hipStream_t stream, int wexp);
// The grid launch_linear_big makes for one launch, host arithmetic (gemm_big.hip; vitvs_op_linear_big_grid): the (slice, row tile,
// column tile) list, the persistent workgroups that walk it (a multiple of 8, at most 256), the XCD map (0: eighths of the list;
// XR in {1, 2, 4, 8}: an XR x 8 / XR XCD grid over (row-slices, column tiles)) and the k-tiles of a slice.
struct BigGrid {
    long tiles = 0;
    int slots = 0, xmap = 0, nk = 0, nx = 0;
};
// rows x cols: a tile of gemm_big.hip; K logical.  0, or -2 wherever launch_linear refuses the launch on that tile.
int linear_big_grid(Precision p, int rows, int cols, int M, int N, int K, int splits, BigGrid* g);

// ---- elementwise.hip -----------------------------------------------------------------------
struct PatchifyArgs {
    const uint8_t* des;   // [n_des][S][S][3] RGB u8
    const uint8_t* cur;   // [n_cur][S][S][3]
    int n_des, n_cur;
    int S, patch, stride, grid, Kp, D;
    float mean[3], std[3];
    const float* cls;     // [D]
    const float* pos;     // [1+T][D]
    int prefix = 1;       // rows in front of the patch tokens in x: cls + registers (P = 1 + R)
};
// Camera-resolution frames ([in_h][in_w][3] instead of [S][S][3]): Pillow's 8-bit bicubic resample tables of
// resize_coefficients() (resize.hip) for both axes, on the device.  rows = the most camera rows one patch's pixels draw on.
struct ResizeArgs {
    const int *xb, *xk, *yb, *yk;   // bounds [S][2] (first input sample, count) and fixed-point taps [S][ks] per axis
    int in_h, in_w, ksx, ksy, rows;
};
constexpr int kResizePrecisionBits = 32 - 8 - 2;   // Pillow Resample.c: PRECISION_BITS
__device__ __forceinline__ int resize_clip8(int v) { return min(max(v >> kResizePrecisionBits, 0), 255); }
// Ape[(img*T + t)][k] = ((u8/255) - mean_c)/std_c for k = c*p*p + py*p + px (zero for k >= 3p²);
// x[img*(T+P)][:] = cls + pos[0].  rs != nullptr: des / cur are camera frames and u8 is the pixel PIL's
// Image.resize((S, S)) would produce (vitvs_v2.py:474-475), computed while the row is built.
int launch_patchify(Precision p, const PatchifyArgs& a, const ResizeArgs* rs, void* Ape, float* x, hipStream_t stream);
// out[m][:] = LayerNorm(x[m][:]) * gamma + beta, out in precision p.
int launch_layernorm(Precision p, const float* x, const float* gamma, const float* beta, void* out, int M, int D,
                     float eps, hipStream_t stream);
// x[m][:] += ls * (sum_z part[z][m][:] + bias)  (fixed slice order), then, if gamma != null,
// out[m][:] = LayerNorm(x[m][:]) * gamma + beta in precision p.  One pass over the row.
// desc (optional, only with gamma == null, i.e. after the last block): the same launch also writes the plain
// L2-normalised descriptors dn[img][t][:] = x[img][P+t][:] / max(norm, 1e-8) (rows are [img][P+T] tokens: cls,
// the R = P - 1 register tokens, then the patches) and clears zero_count 64-bit words of zero_a / zero_b (the Gram kernel's atomicMax targets).
struct DescOut {
    float* dn = nullptr;          // may be null when sq is given
    float* sq = nullptr;          // optional: sq[img * T + t] = |x[img][P + t][:]|^2 (the stencil form of the binned Gram, correspond.hip)
    unsigned long long* zero_a = nullptr;
    unsigned long long* zero_b = nullptr;
    int T = 0;
    int P = 1;                    // prefix rows of each image: cls + register tokens
    int zero_count = 0;
};
int launch_residual_ln(Precision p, float* x, const float* part, int splits, const float* bias, const float* ls,
                       const float* gamma, const float* beta, void* out, int M, int D, float eps, hipStream_t stream,
                       const DescOut* desc = nullptr);
// Finishes a split-K patch embedding (partial rows [n_img][T], launch_linear EPI_PARTIAL) and applies block 0's norm1:
//   x[img][0][:] = cls + pos[0];  x[img][r][:] = reg[r-1] (1 <= r < P, no position embedding);
//   x[img][P+t][:] = pos[1+t] + sum_z part[z][img*T+t][:] + bias;  out = LayerNorm(x).  P = 1: no registers (reg unused).
int launch_embed_ln(Precision p, float* x, const float* part, int splits, const float* bias, const float* pos,
                    const float* cls, const float* reg, const float* gamma, const float* beta, void* out, int n_img, int T,
                    int P, int D, float eps, hipStream_t stream);
// Descriptors for the correspondence stage, fp32, L2-normalised with max(|x|,1e-8), from x rows [img][P+T]:
//   plain : dn[img][t][D]   = x[img][P+t][:] / max(norm, eps)
//   binned: dn[img][t][9D]  = 3x3 replicate-clamped neighbourhood concat, then normalised.
// raw (optional, may be null): the un-normalised descriptor in the same layout.
// zero_a / zero_b (may be null with zero_count 0): zero_count 64-bit words of each are cleared by the
// same launch (the Gram kernel's atomicMax targets), saving two memset nodes per update.
int launch_descriptors(const float* x, float* dn, float* raw, float* sqnorm_ws, int n_img, int T, int P, int grid, int D,
                       int binned, unsigned long long* zero_a, unsigned long long* zero_b, int zero_count,
                       hipStream_t stream);

// dst[0 .. bytes) = src[0 .. bytes), 16 bytes per lane (both buffers hold a multiple of 16 bytes): the host-pointer entry point's
// in-stream copy of caller frames from the handle's pinned staging memory (device-visible host memory) to device memory —
// one short launch on the update's own stream instead of a copy-engine command and its queue hops.
int launch_copy16(const void* src, void* dst, size_t bytes, hipStream_t stream);

// Experiment hook (tools/l2_warm_probe.py): every XCD's private L2 reads all `bytes` of `p` (256 workgroups,
// workgroup L on XCD L % 8 walks the 32nd share L / 8 of the buffer with 16-byte loads), so that a launch that follows finds its
// operand in L2 instead of the Infinity Cache.  share_xcds != 0: XCD x touches only the x-th eighth.
int launch_touch(const void* p, size_t bytes, int share_xcds, hipStream_t stream);

// dst[r][:] = src[r][:] / max(||src[r]||, 1e-8) for fp32 rows of width Dp (caller descriptors).
int launch_normalize_rows(const float* src, float* dst, int rows, int Dp, hipStream_t stream);

// ---- attention.hip -------------------------------------------------------------------------
// out[img*N + q][h*64 + d] = softmax_k(q.k * 64^-0.5) v ; qkv [n_img*N][3*D] in precision p.
// One attention launch, decided by plan_attention and carried out by launch_attention.  The kernels (the codes are ABI:
// vitvs_op_attention_plan): ATTN_F32 the fp32 kernel; ATTN_SHORT 16 queries per workgroup (<= 256 tokens, few workgroups);
// ATTN_Q64 / ATTN_Q64_KS2 64 queries per workgroup, one or two key groups; ATTN_LONG 128 queries per workgroup.  ATTN_NONE:
// a non-positive size.
enum AttnKernel : int { ATTN_NONE = 0, ATTN_F32, ATTN_SHORT, ATTN_Q64, ATTN_Q64_KS2, ATTN_LONG };
struct AttnPlan {
    Precision prec = PREC_F32;
    AttnKernel kernel = ATTN_NONE;
    int n_img = 0, N = 0, H = 0;
    dim3 grid;
    int threads = 0, lds = 0;     // block size, dynamic LDS bytes
    int per = 0, g_per_xcd = 0;   // ATTN_LONG: key tiles per range, workgroups per XCD
    bool divided = false;         // 16-bit ATTN_LONG cut into key ranges: needs the workspace below
    size_t ws_floats = 0, tickets = 0;
    bool ones = false;            // 16-bit ATTN_LONG: the ONES variant (VITVS_ATTN_ONES, attention.hip)
};
// The plan under the hint `in_flight` of updates in flight (by default the calling thread's, g_updates_in_flight): from 2 on
// the long kernel keeps whole query blocks.
AttnPlan plan_attention(Precision p, int n_img, int N, int H, int in_flight = g_updates_in_flight);
// A divided plan merges the key ranges of a query block inside the launch through a workspace: `state` (plan.ws_floats
// floats) and `tickets` (plan.tickets ints, ZERO before the first launch; every launch leaves them zero).  ws = nullptr: a
// per-(device, stream) workspace shared by all callers without one (the operator hook), grown on demand.
// Returns -2 for ATTN_NONE, -3 when a divided plan gets no workspace.
struct AttnWorkspace {
    float* state = nullptr;
    int* tickets = nullptr;
};
// q_prescaled (16-bit precisions only): the q third of qkv already carries hd^-0.5 * log2(e) (kAttnQScale) — the handle folds it
// into the q rows of attn.qkv.weight / bias at upload, in fp32 before the one rounding to 16 bits, so the scale costs the
// forward neither an instruction nor a rounding; raw q (the operator hook) is scaled inside the kernels.
constexpr float kAttnQScale = 0.125f * 1.44269504088896340736f;
int launch_attention(const AttnPlan& plan, const void* qkv, void* out, hipStream_t stream, const AttnWorkspace* ws = nullptr,
                     bool q_prescaled = false);

// ---- correspond.hip ------------------------------------------------------------------------
// The correspondence stage of a velocity update — from the forward's last launch to the packed arg-max keys the law reads —
// decided once by plan_gram and launched from that plan by launch_gram_step, by the product and by the operator hooks alike.
// The forms (the codes are ABI: vitvs_op_gram_plan):
//   GRAM_F32      fused Gram + row / column arg-max over the fp32 descriptors (gram_argmax_kernel<float>)
//   GRAM_SPLIT    the same on the f16 matrix cores from a hi / lo split of the descriptors (16-bit modes from 1024 tokens)
//   GRAM_STENCIL  binned descriptors: raw token Gram into the handle's T x T workspace, then the 3 x 3 stencil arg-max
//   GRAM_WIDE     binned descriptors whose raw Gram workspace would pass 8 GiB: the 9 D-wide descriptors through the fused
//                 arg-max, split as GRAM_SPLIT is
enum GramForm : int { GRAM_NONE = 0, GRAM_F32, GRAM_SPLIT, GRAM_STENCIL, GRAM_WIDE };
// The launches of a form, in order (GramPlan::steps):
//   GSTEP_DESCRIPTORS  x -> the 9 D-wide normalised descriptors dn; clears the keys (GRAM_WIDE; launch_descriptors)
//   GSTEP_SPLIT        dn -> the fp16 hi / lo rows dh (a split plan)
//   GSTEP_ARGMAX       dn or dh -> keys: for pair b, S = dn[a_img(b)] . dn[b_img(b)]^T (T x T) and its row / column arg-max
//   GSTEP_RAW_GRAM     x -> G[b][i][j] = raw dot products of the patch tokens (GRAM_STENCIL: binned descriptors without building them)
//   GSTEP_STENCIL      G, sq -> keys: the 3 x 3 "diagonal" stencil over G, normalised by the binned descriptors' norms, and its arg-max
enum GramStep : int { GSTEP_DESCRIPTORS = 0, GSTEP_SPLIT, GSTEP_ARGMAX, GSTEP_RAW_GRAM, GSTEP_STENCIL };
// What the forward's last launch writes for the stage (DescOut) while it clears the keys: the normalised descriptors, the tokens'
// squared norms, or nothing at all (GSTEP_DESCRIPTORS follows and clears the keys itself).
enum GramEmit : int { EMIT_NONE = 0, EMIT_DN, EMIT_SQ };
struct GramPlan {
    GramForm form = GRAM_NONE;
    bool split = false;                   // the Gram's operands are the fp16 hi / lo split (GSTEP_SPLIT into `dh` first)
    int rows = 0, cols = 0, kgroups = 0;  // tile of the Gram kernel (GRAM_STENCIL: of the raw Gram); rows = 0: unlaunchable
    int hb = 0, per_xcd = 0;              // band rows and workgroups per XCD of the tile order (gram_tile)
    int T = 0, Dp = 0, n_pairs = 0;       // tokens, width of the Gram's rows (GRAM_STENCIL: the model width D), pairs of the call
    GramStep steps[3] = {};               // the launches of the form, in order
    int n_steps = 0;
    GramEmit emit = EMIT_NONE;
    bool refine_from_gram = false;        // the sub-patch refinement reads G and sq (ServoArgs), else dn
    // workspaces at the handle's max_pairs (plan_gram only): G in floats; dh in fp16 elements, under 4 GiB (32-bit operand offsets)
    size_t gram_floats = 0, split_elems = 0;
};
// The stage of a handle (precision, binned descriptors, tokens, model width D, max_pairs) for a call of n_pairs pairs.
GramPlan plan_gram(Precision p, bool binned, int T, int D, int n_pairs, int max_pairs);
// What the steps read and write.  Frames are in the call's order, desired first (one desired frame when des_shared).
//   x        residual stream [frames][P + T][D] fp32, P = prefix rows of each image: cls + register tokens
//   dn, dh   normalised descriptors [frames][T][Dp] fp32 and their split [frames][T][3 Dp] fp16
//   G, sq    raw token Gram [n_pairs][T][T]; |t|^2 per token [frames][T]: DescOut::sq of the forward's last launch
//   grid     tokens per side
//   row_best, col_best   packed (max similarity, first index) keys [n_pairs][T] (common.h pack_best); zero before the arg-max
struct GramOperands {
    const float* x = nullptr;
    int P = 1, grid = 0, des_shared = 0;
    float *dn = nullptr, *G = nullptr, *sq = nullptr;
    void* dh = nullptr;
    unsigned long long *row_best = nullptr, *col_best = nullptr;
};
// Launches step i of the plan as planned.  -2: not a launchable plan or step, or operands the step cannot take (no dh, grid *
// grid != T, P < 1, rows beyond the 32-bit offsets of the main loop).
int launch_gram_step(const GramPlan& plan, int i, const GramOperands& o, hipStream_t stream);
// The whole stage.  (The product loops over the steps itself, to time each in its class: api.hip enqueue_update.)
inline int launch_gram(const GramPlan& plan, const GramOperands& o, hipStream_t stream) {
    int rc = plan.rows ? 0 : -2;
    for (int i = 0; i < plan.n_steps && !rc; ++i) rc = launch_gram_step(plan, i, o, stream);
    return rc;
}
// The Gram itself, in the tile of an unsplit plan: S[b][i][j] over fp32 rows `ld` apart of images `img_stride` apart (descriptors:
// T * Dp, Dp).  GSTEP_RAW_GRAM, and vitvs_correspond_dev's optional dense similarity matrix.
int launch_gram_dense(const GramPlan& plan, const float* src, long img_stride, int ld, int des_shared, float* S, hipStream_t stream);
// Sub-patch offsets (refine.h) of every token of one pair: d1, d2 fp32 normalised rows [T][Dp] (Dp a multiple of 4), nn1 [T]
// -> offsets [T][2] = (dr, dc); matches outside 0 .. T - 1 get (0, 0).  One wave per token.
int launch_refine(const float* d1, const float* d2, const int32_t* nn1, int T, int grid, int Dp, float* offsets, hipStream_t stream);

// packed keys <-> (nn_1, sim_1, nn_2) tables for the standalone correspondence / servo entry points
int launch_decode_best(const unsigned long long* row_best, const unsigned long long* col_best, int T, int32_t* nn1,
                       int32_t* nn2, float* sim1, hipStream_t stream);
int launch_encode_best(const int32_t* nn1, const int32_t* nn2, const float* sim1, int T, unsigned long long* row_best,
                       unsigned long long* col_best, hipStream_t stream);

// ---- select.hip ----------------------------------------------------------------------------
// Selection mode BEST: the visiting order the law then runs on as on a caller's (SEL_PRIORITY).  order [n_pairs][T] <- the tokens
// of every pair sorted by (class, rank within the token's image cell, -similarity, id), decoded from the packed keys the law
// reads; one workgroup per pair, everything in LDS.
struct BestOrderPlan {
    int T = 0, grid = 0, cells = 0;   // cells: min(option "select_cells", grid)
    int n = 0;                        // sorted keys: the next power of two of T
    bool small = false;               // T <= 256: rank counting, one token per thread; else the bitonic network
    int threads = 0;
    size_t lds = 0;                   // dynamic LDS bytes
    bool lds_opt_in = false;          // ... beyond 64 KiB
};
// -2: T not a square grid or cells outside 1 .. 16, -3: more than 160 KiB of LDS
int plan_best_order(int T, int cells, BestOrderPlan* plan);
int launch_best_order(const BestOrderPlan& plan, int n_pairs, const unsigned long long* row_best,
                      const unsigned long long* col_best, int32_t* order, hipStream_t stream);

// ---- roll.hip ------------------------------------------------------------------------------
// The roll search.  out [n][4][S][S][3] <- frames [n][S][S][3] uint8: copy k is numpy.rot90(frame, k); one launch,
// a pixel tile per workgroup through LDS.  -2: a null pointer, n outside 1 .. 65535, S < 1
int launch_quarter_turns(const uint8_t* frames, uint8_t* out, int n, int S, hipStream_t stream);
// The four candidates' keys (pairs 0 .. 3 of row_best / col_best, [4][T]) -> scores [4] (fp64 mean of sim_1 over the mutual
// nearest neighbours; NaN: not a valid candidate), roll_info [8] (k*, the four n_mutual, same-image of k*, 0, 0), *rolled = k* > 0,
// and pair 0's keys = the winner's tables in the unturned frame.  One workgroup.  -2: a null pointer, grid * grid != T
int launch_roll_pick(unsigned long long* row_best, unsigned long long* col_best, int T, int grid, double* scores,
                     int32_t* roll_info, int32_t* rolled, hipStream_t stream);

// ---- servo.hip -----------------------------------------------------------------------------
enum SelectMode : int { SEL_EXPLICIT = 0, SEL_PRIORITY = 1, SEL_DENSE = 2 };
enum Status : int { ST_OK = 0, ST_NO_CORRESPONDENCE = 1, ST_TOO_FEW = 2, ST_NO_DEPTH = 3 };
// Which interaction matrix the law inverts (option "interaction"): L(s, Z), L(s*, Z*) or their mean
enum Interaction : int { IL_CURRENT = 0, IL_DESIRED = 1, IL_MEAN = 2 };

struct ServoArgs {
    int n_pairs, T, grid;
    int num_pairs;            // K rows pairs of the control law (reference num_pairs)
    int mode;                 // SelectMode
    int input_size;           // S
    int u_max, v_max;
    int depth_h, depth_w;
    float scale_f, half_f;    // fp32 patch-centre arithmetic (reference: vitvs_v2.py:511-513)
    double scale_x, scale_y;  // camera / ViT resolution ratios (vitvs_v2.py:544-545)
    const double* K;          // device [n_pairs][4] fx, fy, cx, cy
    double lambda;
    const unsigned long long* row_best;  // [n_pairs][T]
    const unsigned long long* col_best;  // [n_pairs][T]
    const uint16_t* depth;    // [n_pairs][depth_h][depth_w] mm, may be null -> ST_NO_DEPTH
    const int32_t* selection; // EXPLICIT: [n_pairs][sel_stride] token ids; PRIORITY: [n_pairs][T] priorities
    const int32_t* n_selected;// EXPLICIT: [n_pairs] count of ids (<= num_pairs)
    int sel_stride;
    // outputs
    double* v_c;              // [n_pairs][6]
    int32_t* status;          // [n_pairs]
    int32_t* nn1;             // [n_pairs][T]
    int32_t* nn2;             // [n_pairs][T]
    float* sim1;              // [n_pairs][T]
    int32_t* info;            // [n_pairs][8]: n_mutual, n_rows_pairs, same_image, n_matched, sweeps, L rows, re-weightings, zero weights
    int32_t* sel_out;         // [n_pairs][max_rows] selected token ids (image 1)
    int32_t* s_uv;            // [n_pairs][max_rows][4]: u*, v*, u, v
    double* feat;             // [n_pairs][max_rows][4]: Z, x, y, sim
    double* L_ws;             // [n_pairs][7][rows_cap] workspace (L columns + e), also an output for tests
    int max_rows;             // capacity in feature pairs (>= num_pairs; >= T for DENSE)
    double* L_work;           // [n_pairs][7][rows_cap]: the Jacobi SVD's working copy of an L too large for LDS (L_ws keeps L)
    // Tukey IRLS (option "robust_law"); with robust_iters == 0 the plain law's instantiation runs and none of these is read
    int robust_iters;         // re-weightings N, 0 .. 16
    double pitch_u, pitch_v;  // patch pitch in camera pixels (stride * u_max / S, stride * v_max / S): sigma_min = half of it, normalised
    double* W_ws;             // [n_pairs][max_rows] final weight of every feature pair (output); the working weights when L is global
    // Sub-patch refinement (option "subpatch", refine.h); with refine == 0 none of these is read
    int refine;               // 1: the REFINE instantiation moves every selected match by its (dr, dc)
    int des_shared, Dp;       // frames of dn / sq: goal frame of pair b = (des_shared ? 0 : b), current frame = n_des + b
    double pitch_in;          // patch pitch in extractor-input pixels, S / grid
    const float* off_in;      // [n_pairs][T][2] given offsets per goal token, or null: computed from one of the sources below
    const float* dn;          // fp32 normalised descriptors [frames][T][Dp] (GRAM_F32, GRAM_SPLIT, GRAM_WIDE), or
    const float* G;           // raw token Gram [n_pairs][T][T] with
    const float* sq;          // the tokens' squared norms [frames][T] (GRAM_STENCIL)
    float* off_out;           // [n_pairs][max_rows][2] (dr, dc) of every feature row (output)
    // Goal-side interaction matrices (option "interaction"); with interaction == IL_CURRENT none of these is read.
    // IL_DESIRED never reads `depth` (null is not ST_NO_DEPTH) and reports Z* in feat[..][0]; IL_MEAN keeps Z there.
    int interaction;          // Interaction
    int zgoal_stride;         // entries between the goal images of consecutive pairs: T + 1, or 0 when one image serves all
    const uint16_t* zgoal;    // [n_goal][T + 1] mm: goal depth at every token's patch centre, entry T at pixel (0, 0)
    double* zgoal_out;        // [n_pairs][max_rows] Z* of every feature row in metres (output)
    // The roll search (roll.hip); null on every other path, and then nothing below is read
    const int32_t* rolled;    // [1] != 0: the keys are a quarter-turned winner's, carried back into the unturned frame.  Under the
                              // same-image shortcut a feature row's current-side token is then nn_1[tok], not tok, and info[2] is 0
};
// One law launch, decided by plan_servo and carried out by launch_servo.  RefineSource: where servo_kernel<., REFINE, .> takes its
// sub-patch offsets from (the codes are ABI: vitvs_op_servo_plan): a given table (off_in), the raw Gram with the squared norms
// (G, sq: GRAM_STENCIL), or the normalised descriptors (dn: every other form)
enum RefineSource : int { RS_OFF = 0, RS_TABLE, RS_GRAM, RS_DESC };
struct ServoPlan {
    int T = 0, max_rows = 0, robust_iters = 0;   // what the plan was made for: launch_servo refuses other arguments
    Interaction interaction = IL_CURRENT;
    RefineSource source = RS_OFF;
    bool robust = false, refine = false, goalz = false;   // servo_kernel<robust, refine, goalz>; writes W_ws, off_out, zgoal_out
    size_t lds = 0;                // dynamic LDS bytes
    bool lds_opt_in = false;       // ... beyond 64 KiB: the instantiation opts in (per device) before its launch
    bool reads_depth = true;       // the current depth image takes part (not IL_DESIRED): a host-pointer call stages it,
    bool depth_anywhere = false;   // whole (a refined match can lie on any pixel) or at the T patch centres only
};
// -2: an argument out of range (T, max_rows < 1; robust_iters outside 0 .. 16; source; interaction), -3: more than 160 KiB of LDS
int plan_servo(int T, int max_rows, int robust_iters, int source, int interaction, ServoPlan* plan);
// -2 also for arguments that are not the plan's, a source whose pointers are missing or not the first the kernel finds (off_in,
// then G, then dn), an output of the plan without a place
int launch_servo(const ServoPlan& plan, const ServoArgs& a, hipStream_t stream);
// table [n_goal][T + 1] <- goal depth images Z [n_goal][depth_h][depth_w] (mm) at the sites the law reads; `geom` carries
// the geometry fields of a law call (T, grid, scale_*, half_f, depth_h, depth_w)
int launch_goal_depth(const ServoArgs& geom, const uint16_t* Z, int n_goal, uint16_t* table, hipStream_t stream);

// ---- rig.hip -------------------------------------------------------------------------------
// The rig law: ONE twist for a rigid rig of cameras.  Camera i's law left L_i (rows x 6) and e_i; with W_i the
// 6 x 6 twist transform from the rig frame to camera i's optical frame, v_rig = -lambda * pinv(stack_i(L_i W_i)) stack_i(e_i)
// over the cameras whose status is ST_OK.  One launch, one workgroup per camera; the workgroup that finishes last adds the
// cameras' normal equations in camera order and solves (LDL^T, then the Jacobi SVD over the stacked rows: solve.h).
constexpr int kRigMaxCams = 256;      // one workgroup per camera, at most one per CU (the hand-off's measured form)
constexpr int kRigPartDoubles = 32;   // per camera: G (21) + g (6) + its rows, padded to 256 bytes
struct RigArgs {
    int n_cams;
    const int32_t* status;    // [n_cams] the cameras' statuses; null: a camera with rows is ST_OK, one without ST_TOO_FEW
    const int32_t* rows;      // rows of camera i (both rows of every feature pair, zero-padded ones included) at rows[i * rows_stride]
    int rows_stride;
    const double* L;          // [n_cams][7][ld] column-major: L_i's 6 columns, then e_i (ServoArgs::L_ws)
    int ld;
    const double* W;          // [n_cams][36] row-major W_i
    double lambda;
    // workspaces: cap >= n_cams * ld rows; `ticket` zero before the first launch (every launch leaves it zero)
    double* stack;            // [7][cap] the stacked M = L_i W_i and e, contributing cameras in camera order
    double* work;             // [7][cap] the Jacobi SVD's working copy
    int cap;
    double* part;             // [n_cams][kRigPartDoubles] every camera's normal equations
    int* ticket;
    // outputs
    double* v_rig;            // [6]
    int32_t* rig_status;      // ST_OK when a camera contributed, else the largest camera status (v_rig = 0)
    int32_t* rig_info;        // [8] or null: cameras used, total rows, sweeps (-1: LDL^T), n_cams, largest camera status, 0, 0, 0
    double* normal;           // [28] or null: G upper triangle row-major (21), g (6), total rows
};
// Bytes of one scratch block for n_cams cameras of ld rows each, and its parts (ticket first, on a line of its own)
size_t rig_scratch_bytes(int n_cams, int ld);
void rig_carve(void* scratch, int n_cams, int ld, RigArgs& a);
// two_launches: the partial sums and the solve as two plain launches instead of the in-launch fan-in (the alternative
// tools/rig_times.py times it against).  -2: n_cams outside 1 .. kRigMaxCams, ld < 1, cap < n_cams * ld, a null pointer
int launch_rig(const RigArgs& a, hipStream_t stream, bool two_launches = false);

// The robust rig law: Tukey IRLS over the stacked system, ONE median over the live pairs of all contributing
// cameras.  Same launch shape and fan-in as the rig law; the workgroup that arrives last copies the stack once (into LDS while
// n_cams * ld <= kRigRobustTile rows, else into `work`) and runs the n_iter re-weightings and n_iter + 1 weighted solves with all
// four waves, as servo_kernel<true, .> does for one camera.  A camera contributes when its status is ST_OK, it has rows and a
// live pair; its rows count in pairs (an odd last row is dropped).
constexpr int kRigRobustTile = 384;   // stacked rows kept in LDS: 8 cameras x 48 rows
struct RigRobustArgs {
    RigArgs r;                // as the rig law's; r.part is not used, r.normal takes the weighted G, g of the last solve
    const int32_t* live;      // live pairs of camera i at live[i * live_stride] (the first pairs of its rows); null: every pair
    int live_stride;
    const double* K;          // [n_cams][4] fx, fy, cx, cy: sigma_min = max_i 0.5 max(pitch_u / fx_i, pitch_v / fy_i); null: sigma_min
    double pitch_u, pitch_v;
    double sigma_min;
    int n_iter;               // 1 .. 16
    double* work2;            // [7][cap] the Jacobi SVD's copy when `work` holds the stack
    double* weights;          // [n_cams][weights_stride] or null: the final weights, 0 where no live pair of a contributing camera is
    int weights_stride;
    double* sigma;            // [1] or null: the last scale
};
struct RigRobustPlan {
    size_t lds;               // dynamic LDS of the launch
    bool lds_resident;        // the stack's copy sits in LDS
    bool lds_opt_in;          // > 64 KiB
    int pairs;                // n_cams * (ld / 2): the residuals and weights the LDS holds
};
// -2: n_cams outside 1 .. kRigMaxCams, ld < 1; -3 (plan filled): more than 160 KiB of LDS
int plan_rig_robust(int n_cams, int ld, RigRobustPlan* plan);
// the rig law's block and a third [7][cap] block (work2)
size_t rig_robust_scratch_bytes(int n_cams, int ld);
void rig_robust_carve(void* scratch, int n_cams, int ld, RigRobustArgs& a);
int launch_rig_robust(const RigRobustArgs& a, hipStream_t stream);

// ---- pose.hip ------------------------------------------------------------------------------
// The pose law: per pair ONE rigid displacement (R, t), X_goal = R X_cam + t, aligning the current 3-D points of
// the feature rows with their goal points (Horn's quaternion form), and v_pose = -lambda (R^T t, theta u).  One launch, one
// workgroup per pair.  The points come from what the camera's law left (selected, s_uv, feat, info, the goal-depth table) or,
// for the seam tests, from the caller (P, Q, usable).  n_hyp > 0: the consensus start, n_hyp three-point hypotheses scored in parallel
// in front of the alignment loop, which then starts from the winner's consensus set instead of every usable row.
struct PoseArgs {
    int n_pairs;
    int ld;                   // rows per pair of every per-row array (max_rows)
    const int32_t* status;    // [n_pairs] the cameras' statuses, or null (all ST_OK): a pair that is not ST_OK keeps its status, v = 0
    // the handle's form (P == null): rows k < info[b][1] of pair b
    const int32_t* selected;  // [n_pairs][ld] goal token of every row, -1 padded
    const int32_t* s_uv;      // [n_pairs][ld][4]
    const double* feat;       // [n_pairs][ld][4]: Z (100 = a hole), x, y, sim
    const int32_t* info;      // [n_pairs][8] of the camera's law: [1] rows written, [2] the same-image shortcut
    const double* K;          // [n_pairs][4] fx, fy, cx, cy; also sigma_min = 0.5 max(pitch_u / fx, pitch_v / fy) median(Z*)
    const uint16_t* zgoal;    // [n_goal][T + 1] mm (ServoArgs::zgoal), 0 = a hole
    int zgoal_stride, T;
    double pitch_u, pitch_v;
    // given points (P != null): all ld rows
    const double* P;          // [n_pairs][ld][3]
    const double* Q;          // [n_pairs][ld][3]
    const int32_t* usable;    // [n_pairs][ld]: > 0 usable, 0 padded, < 0 a hole
    double sigma_min;         // read when K is null
    double lambda;
    int n_iter;               // Tukey re-weightings, 0 .. 16
    double* ws;               // [n_pairs][7][ld] the points and their flags (pose_scratch_bytes)
    // outputs
    double* v_pose;           // [n_pairs][6]
    int32_t* pose_status;     // [n_pairs] the camera's status when that is not ST_OK; ST_TOO_FEW: < 3 rows with a weight, or degenerate
    double* pose;             // [n_pairs][12] or null: R row-major, t (identity when the status is not ST_OK)
    int32_t* pose_info;       // [n_pairs][8] or null: usable rows, sweeps, re-weightings, usable rows at weight 0, degenerate, holes,
                              // the consensus winner's j + 1 (0: consensus off, not run for fewer than 3 usable rows, or every
                              // hypothesis skipped), the start weights at 1 (0 where the phase did not run)
    double* weights;          // [n_pairs][weights_stride] or null
    int weights_stride;
    double* sigma;            // [n_pairs] or null: the last scale
    // the consensus start (behind everything the kernel read before it had one)
    int n_hyp;                // hypotheses, 0 .. 4096; 0: no consensus phase, the kernel is the one without it
    unsigned seed;            // of the draw; the positions depend on (seed, j, usable rows) only
};
struct PosePlan {
    size_t lds;               // dynamic LDS of the launch: (320 + (robust ? 2 max_rows : consensus ? max_rows : 0) +
                              // (consensus ? 8 + (max_rows + 1) / 2 : 0)) doubles, the last term consensus_core.h's
                              // consensus_lds_doubles
    bool robust;              // pose_kernel<robust, consensus>
    bool lds_opt_in;          // > 64 KiB
    bool consensus;
};
// -2: max_rows < 1, n_iter outside 0 .. 16, n_hyp outside 0 .. 4096; -3 (plan filled): more than 160 KiB of LDS
int plan_pose(int max_rows, int n_iter, int n_hyp, PosePlan* plan);
size_t pose_scratch_bytes(int n_pairs, int ld);
int launch_pose(const PoseArgs& a, hipStream_t stream);

// ---- pose_rig.hip --------------------------------------------------------------------------
// The pose rig law: ONE rigid displacement (R, t) of a rigid rig, aligning the matched 3-D points of ALL its
// cameras in the rig frame.  Camera i has pose (R_i, t_i) in the rig frame; its points P, Q (PoseArgs' rule) enter the stack as
// P' = R_i P + t_i, Q' = R_i Q + t_i at stack row i * ld + k, and v_rig = -lambda (R^T t, theta u) is a twist in the rig's own
// frame.  One launch of ONE workgroup: pose_kernel's loop over n_cams * ld rows.  A camera contributes when its status is ST_OK
// and it is not under the same-image shortcut.
struct PoseRigArgs {
    int n_cams;
    int ld;                   // rows per camera of every per-row array (max_rows)
    const int32_t* status;    // [n_cams] the cameras' statuses, or null (all ST_OK)
    const double* rTc;        // [n_cams][12] R_i row-major, then t_i
    // the handle's form (P == null): as PoseArgs'
    const int32_t* selected;
    const int32_t* s_uv;
    const double* feat;
    const int32_t* info;
    const double* K;          // [n_cams][4]; sigma_min = 0.5 max_i max(pitch_u / fx_i, pitch_v / fy_i) median(Z*), i contributing
    const uint16_t* zgoal;
    int zgoal_stride, T;
    double pitch_u, pitch_v;
    // given camera-frame points (P != null): all ld rows of every camera
    const double* P;          // [n_cams][ld][3]
    const double* Q;          // [n_cams][ld][3]
    const int32_t* usable;    // [n_cams][ld]: > 0 usable, 0 padded, < 0 a hole
    double sigma_min;         // read when K is null
    double lambda;
    int n_iter;               // Tukey re-weightings, 0 .. 16
    double* ws;               // [7][n_cams * ld] the stack: P' [3], Q' [3], the flag (pose_rig_scratch_bytes)
    // outputs
    double* v_rig;            // [6]
    int32_t* rig_status;      // ST_OK; ST_TOO_FEW: < 3 rows with a weight, or degenerate; nobody contributes: the largest camera status
    double* pose;             // [12] or null: R row-major, t (identity when the twist is zero)
    int32_t* rig_info;        // [8] or null: contributing cameras, usable rows, sweeps, re-weightings, usable rows at weight 0,
                              //              degenerate, holes, the largest camera status
    double* moments;          // [18] or null: sum w, sum w P' [3], sum w Q' [3], sum w P' Q'^T [9], sum w |P'|^2, sum w |Q'|^2 over
                              //               the stack with the final weights (zeros when nobody contributes)
    double* weights;          // [n_cams][weights_stride] or null
    int weights_stride;
    double* sigma;            // [1] or null: the last scale
};
struct PoseRigPlan {
    size_t lds;               // dynamic LDS of the launch
    bool robust;              // pose_rig_kernel<robust>
    bool lds_opt_in;          // > 64 KiB
};
// -2: n_cams, ld < 1, n_iter outside 0 .. 16; -3 (plan filled): more than 160 KiB of LDS
int plan_pose_rig(int n_cams, int ld, int n_iter, PoseRigPlan* plan);
size_t pose_rig_scratch_bytes(int n_cams, int ld);
int launch_pose_rig(const PoseRigArgs& a, hipStream_t stream);

// ---- homography.hip ------------------------------------------------------------------------
// The homography law: per pair the 3 x 3 homography H of the matched normalised image points, m* ~ H m (Hartley
// normalisation, the 9 x 9 DLT normal matrix, its smallest eigenvector by a cyclic Jacobi, det H = 1), and Benhimane and Malis'
// twist v_h = -lambda (depth_scale (H - I) m_c, (H21 - H12, H02 - H20, H10 - H01)).  No depth takes part.  One launch, one
// workgroup per pair.  The points come from what the camera's law left (selected, s_uv, feat, info) or, for the seam tests, from
// the caller (m, ms, usable).  n_hyp > 0: the consensus start, n_hyp four-point hypotheses scored in parallel in front of the solve
// loop, which then starts from the winner's consensus set instead of every usable row.
struct HomographyArgs {
    int n_pairs;
    int ld;                   // rows per pair of every per-row array (max_rows)
    const int32_t* status;    // [n_pairs] the cameras' statuses, or null: ST_NO_CORRESPONDENCE and ST_TOO_FEW are kept with v = 0,
                              // ST_NO_DEPTH does not stop this law
    // the handle's form (m == null): rows k < info[b][1] of pair b, usable when selected[k] >= 0
    const int32_t* selected;  // [n_pairs][ld] goal token of every row, -1 padded
    const int32_t* s_uv;      // [n_pairs][ld][4]
    const double* feat;       // [n_pairs][ld][4]: Z (not read), x, y, sim
    const int32_t* info;      // [n_pairs][8] of the camera's law: [1] rows written, [2] the same-image shortcut
    const double* K;          // [n_pairs][4] fx, fy, cx, cy; also sigma_min = 0.5 max(pitch_u / fx, pitch_v / fy)
    double pitch_u, pitch_v;
    // given points (m != null): all ld rows
    const double* m;          // [n_pairs][ld][2] current normalised points
    const double* ms;         // [n_pairs][ld][2] goal normalised points
    const int32_t* usable;    // [n_pairs][ld]: > 0 usable
    double sigma_min;         // read when K is null
    double lambda;
    double depth_scale;       // metres, > 0: scales the translational half only
    int n_iter;               // Tukey re-weightings, 0 .. 16
    double* ws;               // [n_pairs][5][ld] the points and their flags (homography_scratch_bytes)
    // outputs
    double* v_h;              // [n_pairs][6]
    int32_t* h_status;        // [n_pairs] ST_OK; the camera's ST_NO_CORRESPONDENCE / ST_TOO_FEW; ST_TOO_FEW: < 4 rows with a weight,
                              // or degenerate
    double* H;                // [n_pairs][9] or null: row-major, det 1 (identity when the twist is zero)
    int32_t* h_info;          // [n_pairs][8] or null: usable rows, sweeps of the last solve, re-weightings, usable rows at weight 0,
                              // degenerate, rows with rho = inf at the last re-weighting, the consensus winner's j + 1 (0: consensus
                              // off, not run for fewer than 4 usable rows, or every hypothesis skipped), the start weights at 1
    double* weights;          // [n_pairs][weights_stride] or null
    int weights_stride;
    double* sigma;            // [n_pairs] or null: the last scale
    // the consensus start (behind everything the kernel read before it had one)
    int n_hyp;                // hypotheses, 0 .. 4096; 0: no consensus phase, the kernel is the one without it
    unsigned seed;            // of the draw; the positions depend on (seed, j, usable rows) only
};
struct HomographyPlan {
    size_t lds;               // dynamic LDS of the launch: (752 + (robust ? 2 max_rows : 0) + (consensus ? 8 + (max_rows + 1) / 2 : 0))
                              // doubles, the last term consensus_core.h's consensus_lds_doubles
    bool robust;              // homography_kernel<robust, consensus>
    bool lds_opt_in;          // > 64 KiB
    bool consensus;
};
// -2: max_rows < 1, n_iter outside 0 .. 16, n_hyp outside 0 .. 4096; -3 (plan filled): more than 160 KiB of LDS
int plan_homography(int max_rows, int n_iter, int n_hyp, HomographyPlan* plan);
size_t homography_scratch_bytes(int n_pairs, int ld);
int launch_homography(const HomographyArgs& a, hipStream_t stream);

// ---- photometric.hip -----------------------------------------------------------------------
// The photometric law: per pair one interaction row per pixel of the pooled luminance image (2^level x 2^level
// blocks), v_p = -lambda (H + mu diag(H))^-1 g of H = sum L^T L, g = sum L^T (I_cur - I_des).  Reads frames, never tokens.  Two
// launches: the 28 sums per (pair, band of pooled rows), then one workgroup per pair, one wave of which adds the bands in order and solves.
struct PhotometricArgs {
    int n_pairs;
    int height, width;        // of every frame and depth image
    int level;                // 0 .. 3
    int interaction;          // IL_CURRENT or IL_DESIRED: the image the gradients are taken of, and whose depth Z_mm is
    const uint8_t* I_cur;     // [n_pairs][height][width][3]
    const uint8_t* I_des;     // [n_pairs][height][width][3]
    const uint16_t* Z_mm;     // [n_pairs][height][width] mm, 0 = hole; null: depth_scale everywhere
    double depth_scale;       // metres; Z_mm null and depth_scale <= 0: ST_NO_DEPTH
    const double* K;          // [n_pairs][4] fx, fy, cx, cy at height x width
    double mu, lambda;
    double* ws;               // [n_pairs][bands][32] the band partials (PhotometricPlan::ws_bytes)
    // outputs
    double* v_p;              // [n_pairs][6]
    int32_t* p_status;        // [n_pairs] ST_OK; ST_TOO_FEW (v = 0): fewer than 6 rows or a failed pivot; ST_NO_DEPTH (v = 0)
    double* normal;           // [n_pairs][28] or null: H upper triangle row-major (21), g (6), sum e^2
    int32_t* p_info;          // [n_pairs][8] or null: rows, pooled h, pooled w, bands, holes left out, a pivot failed, 0, 0
};
struct PhotometricPlan {
    int h, w;                 // the pooled image: height >> level, width >> level
    int rows;                 // pooled rows per band: max(1, min((2048 >> level) / w, h / 256))
    int bands;                // ceil(h / rows): the grid is bands x n_pairs
    size_t lds;               // dynamic LDS of the rows launch: 4 x 32 doubles, then ((rows + 2) 2 w + rows w) int32
    bool lds_opt_in;          // > 64 KiB (rows wider than 2048 pooled pixels)
    size_t ws_bytes;          // max_pairs x bands x 256
};
// -2: height or width outside 1 .. 4096, level outside 0 .. 3, a pooled side < 3, max_pairs < 1
int plan_photometric(int height, int width, int level, int max_pairs, PhotometricPlan* plan);
int launch_photometric(const PhotometricArgs& a, hipStream_t stream);

// The robust photometric law: the plain law's rows under the lighting model I_cur ~ (1 + gamma) I_des + beta
// (`illumination`) and Tukey weights (`iterations` re-weightings, the scale from a histogram median of the residuals, at least
// sigma_min grey levels).  3 iterations + 2 launches, no host round trip.  p.ws, hist and state are set by launch_photometric_robust
// from its block of photometric_robust_ws_bytes(max_pairs) bytes, which every call must find with its histograms zero (as the
// allocation and every call leave them); p.normal is not read.
struct PhotometricRobustArgs {
    PhotometricArgs p;        // p.ws: [n_pairs][bands][48] the band partials
    int illumination;         // 0 / 1
    int iterations;           // 0 .. 4
    double sigma_min;         // > 0
    uint32_t* hist;           // [n_pairs][4096] bins of 1 / 16 grey level
    double* state;            // [n_pairs][16] x (6), gamma, beta, sigma, (rows, failed), (median bin)
    // outputs (p.p_info slot 6: rows of final weight 0; slot 7: re-weightings run)
    double* p_robust;         // [n_pairs][4] gamma, beta, the last sigma (0: no re-weighting), the final sum of the weights
    double* normal45;         // [n_pairs][45] or null: the last pass's sums A (21), b (6), c, B (12), C (3), d (2)
};
size_t photometric_robust_ws_bytes(int max_pairs);
int launch_photometric_robust(const PhotometricRobustArgs& a, unsigned char* ws, int max_pairs, hipStream_t stream);

// The photometric rig law: the robust photometric law's rows of r.p.n_pairs = n_cams cameras of one rigid rig
// stacked into one 6 x 6 system in the rig frame, every camera with a lighting model of its own, and one median over all
// cameras' residuals.  4 iterations + 2 launches, no host round trip; the block is launch_photometric_robust's (one photometric
// call of either kind in flight per block).  The per-pair fields of r.p are per camera, except the outputs of the rig:
// r.p.v_p [6] the rig twist, r.p.p_status [1], r.p.p_info [8] = live cameras, n_total, rows of final weight 0, re-weightings run,
// holes, a pivot failed, pooled h, pooled w.  r.p_robust [n_cams][4] and r.normal45 [n_cams][45] stay per camera.
constexpr int kPhotoRigMaxCams = 16;
struct PhotometricRigArgs {
    PhotometricRobustArgs r;
    const double* cVr;        // [n_cams][6][6] rig twist -> camera twist
    const int32_t* live;      // [n_cams] or null (all live): a camera at 0 leaves no trace in any sum
    double* rig_normal;       // [28] or null: H_r (21, upper triangle, row-major), g_r (6), c_r of the last pass
};
int launch_photometric_rig(const PhotometricRigArgs& a, unsigned char* ws, int max_pairs, hipStream_t stream);

// The tile photometric law: the robust photometric law with a LOCAL lighting model, one (gamma_k, beta_k) per tile
// of a tiles_y x tiles_x grid over the pooled image (tile of pooled pixel (r, c): floor(r tiles_y / h) tiles_x + floor(c tiles_x /
// w)), always on (r.illumination is not read).  Per tile the 45 sums and the 2 x 2 elimination; the live tiles add into one 6 x 6
// system in ascending order; a tile whose 2 x 2 factor fails is dead in that pass (adds nothing, gamma = beta = 0).  One median over
// all rows.  3 iterations + 2 launches, no host round trip, in a block of its own of photometric_tile_ws_bytes(max_pairs) bytes
// that every call must find with its histograms zero.
constexpr int kPhotoTileMax = 64;
struct PhotometricTileArgs {
    PhotometricRobustArgs r;  // r.p.ws: [n_pairs][bands][slots][tiles_x][48] the segment partials; r.state: [n_pairs][16 + 128]
                              // r.p_robust [n_pairs][4]: live tiles, dead tiles, the last sigma, the live tiles' final sum of weights
                              // r.normal45 [n_pairs][T][45] or null: every tile's sums of the last pass
    int tiles_y, tiles_x;     // 1 .. 8 each, at most the pooled side
    double* p_tiles;          // [n_pairs][T][4] gamma_k, beta_k, the tile's final sum of weights, live (1.0 / 0.0)
};
struct PhotometricTilePlan {
    int h, w, rows, bands;    // plan_photometric's
    int slots;                // partials a band keeps per tile column: 2 when rows > 1 (a band may lie across one tile-row boundary;
                              // slot s is tile row floor(band rows tiles_y / h) + s), else 1
    size_t lds, lds_res;      // dynamic LDS of the rows and the residual launch: the robust law's
    size_t ws_doubles;        // per pair: bands x slots x tiles_x x 48
};
// -2: what plan_photometric refuses, tiles_y or tiles_x outside 1 .. 8 or above the pooled side
int plan_photometric_tiles(int height, int width, int level, int tiles_y, int tiles_x, int max_pairs, PhotometricTilePlan* plan);
size_t photometric_tile_ws_bytes(int max_pairs);
int launch_photometric_tiles(const PhotometricTileArgs& a, unsigned char* ws, int max_pairs, hipStream_t stream);

// The surface photometric law: the tile law's sibling for SMOOTH lighting fields, a bilinear spline of gains and
// biases on the (cells_y + 1)(cells_x + 1) nodes of the tile law's grid (node a = i (cells_x + 1) + j; unknown 2 a = gamma_a,
// 2 a + 1 = beta_a; M <= 162).  Per cell 120 sums; the cells add in ascending order into one banded node system, eliminated under
// the pivot rule with the six twist columns as a border; an unknown whose pivot fails is dead in that pass (value 0).  One median
// over all rows.  3 iterations + 2 launches, no host round trip, in a block of its own of photometric_surface_ws_bytes(max_pairs)
// bytes (4096 segment rows x 8 cell columns x 128 doubles = 32 MiB per pair, a histogram and a state) that every call must find
// with its histograms zero.
constexpr int kPhotoSurfMaxNodes = 81;
struct PhotometricSurfaceArgs {
    PhotometricRobustArgs r;  // r.p.ws: [n_pairs][bands][slots][cells_x][128] the segment partials; r.state: [n_pairs][16 + 176]
                              // r.p_robust [n_pairs][4]: live unknowns, dead unknowns, the last sigma, the final sum of weights
                              // r.normal45 is not read
    int cells_y, cells_x;     // 1 .. 8 each, at most the pooled side
    double* p_nodes;          // [n_pairs][nodes][4] gamma_a, beta_a, gamma_a live (1.0 / 0.0), beta_a live
    double* cell_sums;        // [n_pairs][cells][120] or null: A (21), b (6), c, B (6 x 8), C (36, upper triangle), d (8) of the last pass
};
struct PhotometricSurfacePlan {
    PhotometricTilePlan t;    // the tile law's bands, slots and LDS (its ws_doubles is the tile law's)
    size_t ws_doubles;        // per pair: bands x slots x cells_x x 128
    size_t lds_solve;         // dynamic LDS of the solve launch: 8 (128 cells + 32 M + 296) bytes
};
// -2: what plan_photometric_tiles refuses
int plan_photometric_surface(int height, int width, int level, int cells_y, int cells_x, int max_pairs, PhotometricSurfacePlan* plan);
size_t photometric_surface_ws_bytes(int max_pairs);
int launch_photometric_surface(const PhotometricSurfaceArgs& a, unsigned char* ws, int max_pairs, hipStream_t stream);

// out[n_img][T][D] fp32, index d*H + h <- which-th (0 q, 1 k, 2 v) third of qkv[n_img*(P+T)][3][H][64], cls and registers dropped
// q_unscale: factor that undoes a pre-scaled q third (1 / kAttnQScale for which == 0 in the 16-bit modes, else 1)
// keep_cls: 0 -> out [n_img][T][D]; 1 -> out [n_img][1 + T][D] (the cls row first, registers dropped)
int launch_facet(Precision p, const void* qkv, float* out, int n_img, int T, int P, int H, int which, float q_unscale, int keep_cls,
                 hipStream_t stream);
// Saliency maps of the extractor (dinov2_extractor.py:339-353): out fp32 [n_img][T], class-token attention of the chosen heads
// of the block whose qkv is given ([n_img][P+T] rows: softmax over all P + T keys, patch columns kept), averaged and min-max
// normalised per image.
int launch_saliency(Precision p, const void* qkv, float* out, int n_img, int T, int P, int H, const int* head_idx, int n_heads,
                    bool q_prescaled, hipStream_t stream);
// Pillow-exact bicubic resize of n RGB uint8 frames [in_h][in_w][3] -> [out][out][3] (resize.hip).  The tables come from
// resize_coefficients (host, double precision, Pillow's expressions): bounds [out][2] = (first tap, taps), coefficients
// [out][ksize] in 22-bit fixed point; x tables for the width, y tables for the height.
int resize_coefficients(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& coeffs);
int launch_resize_bicubic(const uint8_t* src, uint8_t* dst, int n, int in_h, int in_w, int out, const int* xb, const int* xk,
                          int ksx, const int* yb, const int* yk, int ksy, hipStream_t stream);

}  // namespace vitvs
