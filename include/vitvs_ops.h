/*
 * vitvs_ops.h — single-operator entry points of libvitvs_hip.so, exported so that the
 * kernel-level parity tests (tests/test_gpu_ops.py) can drive each HIP kernel through the C ABI.
 * Not part of the drop-in surface; the reference issues these as stock PyTorch ops:
 *   linear / linear_residual   nn.Linear (+ GELU, + LayerScale and residual add)  dino_patch/attention.py:72,79; block.py:78-96
 *   layernorm                  nn.LayerNorm(eps=1e-6)                              dino_patch/block.py:57,75
 *   attention                  scaled_dot_product_attention over [B,H,N,64]        dino_patch/attention.py:73-78
 *   linear_partial+residual_ln the same nn.Linear + residual (+ next LayerNorm), as K slices  dino_patch/block.py:90-115
 *   patchify / embed_ln        ToTensor + Normalize + patch extraction, cls / register / pos_embed rows, norm1 of block 0
 *                                                                                  dinov2_extractor.py:141,177-191,259
 *   residual_desc / descriptors / normalize_rows   last residual add, 3x3 log-bin, cosine normalisation
 *                                                                                  dinov2_extractor.py:289-308; vitvs_v2.py:55
 *   facet / saliency           the q / k / v facets and the class token's attention maps  dinov2_extractor.py:193-217,339-353
 * All pointers are device pointers unless a comment says host; `precision` is enum vitvs_precision; `stream` a hipStream_t.
 */
#ifndef VITVS_OPS_H
#define VITVS_OPS_H
#include <stdint.h>
#ifndef VITVS_API
#define VITVS_API __attribute__((visibility("default")))
#endif
#ifdef __cplusplus
extern "C" {
#endif

/* out[M][N] = act(A[M][K] . W[N][K]^T + bias[N]); A, W, out in `precision`; K % 64 == 0, N % 64 == 0 */
VITVS_API int vitvs_op_linear(int32_t precision, const void* A, const void* W, const float* bias, void* out, int32_t M,
                    int32_t N, int32_t K, int32_t gelu, void* stream);
/* The same operator on a chosen tile family (the library picks one by itself in vitvs_op_linear): variant 0 = the
 * library's choice, 1 = the 64/128-row tiles of gemm.hip as that file picks them, 2 = its 128 x 128 tiles whatever the shape
 * (16-bit precisions, N % 128 == 0), 256 / 192 / 128 = the 256-row tiles of gemm_big.hip with that column width, 1192 / 1256 =
 * its 192 x 128 / 192 x 256 tiles (16-bit precisions, N % width == 0, K >= 128).  For the parity tests of both families on one shape and for
 * tools/big_ops.  slices > 0 selects the split-K form: out = fp32 part[slices][M][N], bias / gelu ignored. */
VITVS_API int vitvs_op_linear_variant(int32_t precision, int32_t variant, const void* A, const void* W, const float* bias,
                            void* out, int32_t M, int32_t N, int32_t K, int32_t gelu, int32_t slices, void* stream);
/* x[M][N] (fp32) += ls[N] * (A . W^T + bias); ls may be NULL */
VITVS_API int vitvs_op_linear_residual(int32_t precision, const void* A, const void* W, const float* bias, const float* ls,
                             float* x, int32_t M, int32_t N, int32_t K, void* stream);
/* out[M][D] = LayerNorm(x[M][D]) * gamma + beta; x fp32, out in `precision`; D in {128,256,384,768,1024} */
VITVS_API int vitvs_op_layernorm(int32_t precision, const float* x, const float* gamma, const float* beta, void* out, int32_t M,
                       int32_t D, float eps, void* stream);
/* out[n_img*N][H*64] = softmax(q k^T / 8) v per (image, head); qkv [n_img*N][3*H*64].  From 512 tokens on the keys of a query
 * block may be split over several workgroups that merge through a workspace this hook owns, one per (device, stream): calls
 * on different streams do not share state (handles own their workspace).
 * vitvs_op_attention takes the raw q a plain qkv projection produces and applies 1/8 (and the log2(e) of its exp2) inside the
 * kernels; in the 16-bit precisions the long-sequence kernel does that by one more 16-bit rounding of q.
 * vitvs_op_attention_q with q_prescaled != 0 is the form the handle's forward uses in the 16-bit precisions: the q third of qkv
 * already carries 0.125 * log2(e) (the handle folds it into the q rows of attn.qkv.weight / bias in fp32, before their one
 * rounding to 16 bits), and the kernels apply nothing.  q_prescaled is ignored for VITVS_F32. */
VITVS_API int vitvs_op_attention(int32_t precision, const void* qkv, void* out, int32_t n_img, int32_t N, int32_t H,
                       void* stream);
VITVS_API int vitvs_op_attention_q(int32_t precision, const void* qkv, void* out, int32_t n_img, int32_t N, int32_t H,
                         int32_t q_prescaled, void* stream);

/* Split-K pair used for the narrow layers (proj, fc2, patch embedding):
 *   slices = vitvs_op_splitk_slices(precision, M, N, K)           (>= 1; the plan the forward uses)
 *   part[z][M][N] (fp32) = A[:, z-th K slice] . W[:, z-th K slice]^T   for z < slices
 *   x[M][D] (fp32) += ls[D] * (sum_z part[z] + bias)  (slices summed in index order); then, if gamma != NULL,
 *   out[M][D] = LayerNorm(x) * gamma + beta in `precision` (out may be NULL when gamma is NULL). */
VITVS_API int vitvs_op_splitk_slices(int32_t precision, int32_t M, int32_t N, int32_t K);
/* Measurement hook (tools/l2_warm_probe.py): the private L2 of every XCD reads all `bytes` of p (share_xcds != 0: XCD x only the
 * x-th eighth), so that a following launch finds the operand in L2 rather than in the Infinity Cache.  No result. */
VITVS_API int vitvs_op_touch(const void* p, int64_t bytes, int32_t share_xcds, void* stream);
/* VITVS_F16X2 operands of the hooks: A / qkv rows and W rows hold 2 C fp16 per C logical columns, [hi of 32 columns | lo of the
 * same 32] per 64 fp16 (csrc/common.h), outputs likewise; W may carry a power of two 2^e (e = 0 .. 31, what the handle's weight
 * upload does so that the lo halves are normal fp16 numbers): this sets e for the calling thread's later vitvs_op_linear* calls
 * (the sums leave multiplied by 2^-e).  e outside 0 .. 31 only reads.  Returns the previous value. */
VITVS_API int vitvs_op_weight_exponent(int32_t e);
/* The plan hint a handle carries as its "in_flight" option (vitvs.h), for the pointer-only hooks of this header: the calling
 * thread's later vitvs_op_* calls plan as if n updates were in flight (n >= 1; n < 1 only reads).  Returns the previous value. */
VITVS_API int vitvs_op_plan_in_flight(int32_t n);
/* the tile the library launches for a linear layer: tile[0..2] = rows, columns, k-groups (k-groups 0: the 256-row kernels of
 * gemm_big.hip); slices = 0: vitvs_op_linear, > 0: vitvs_op_linear_partial with that many K slices.  No device work. */
VITVS_API int vitvs_op_linear_tile(int32_t precision, int32_t M, int32_t N, int32_t K, int32_t slices, int32_t* tile);
/* the linear launch the library makes at this shape under the calling thread's plan hint, no device work:
 * epilogue 0 store (vitvs_op_linear), 1 partial sums (vitvs_op_linear_partial; slices 0 = the library's count);
 * out[0..6] = big family (gemm_big.hip), rows, columns, k-groups, ring stages, K slices, XCD map.  0, or -2 when unlaunchable.
 * (k-groups 0: the kernels of gemm_big.hip; ring stages 0: the tile's default ring.) */
VITVS_API int vitvs_op_linear_plan(int32_t precision, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t slices, int32_t* out);
/* the grid of a launch on a tile of gemm_big.hip (rows x cols = 256 x 256 / 192 / 128, 192 x 128 / 256), decided on the launch
 * side from the shape alone; slices as vitvs_op_linear_variant's (0: the store form, one slice).  out[0..3] = tiles (slices x row
 * tiles x column tiles), persistent workgroups (a multiple of 8, at most 256), XCD map (0: every XCD walks an eighth of the tile
 * list; XR in {1, 2, 4, 8}: the XCDs form an XR x 8 / XR grid over (slice and row tile, column tile) and each walks its block),
 * k-tiles per slice.  Returns 0, or -2 (out zeroed) wherever vitvs_op_linear_variant refuses that tile at that shape: fp32, N not
 * a multiple of cols, a slice that is not 2 .. 255 k-tiles, more than 255 column tiles or slices.  No device work. */
VITVS_API int vitvs_op_linear_big_grid(int32_t precision, int32_t rows, int32_t cols, int32_t M, int32_t N, int32_t K,
                             int32_t slices, int32_t* out);
/* the attention launch the library makes for vitvs_op_attention / _q (and the handle's forward) at this shape, under the
 * calling thread's plan hint: out[0..5] = kernel, workgroups, threads per workgroup, dynamic LDS bytes, key tiles per
 * workgroup (long kernel; 0 otherwise), divided (1: the 16-bit long kernel cuts the keys of a query block into ranges merged
 * through the workspace).  Kernels: 1 fp32; 2 short (16 queries per workgroup); 3 64 queries per workgroup; 4 the same with
 * two key groups; 5 long (128 queries per workgroup).  Returns 0, or -2 (out[0] = 0) when a size is not positive.  No device work. */
VITVS_API int vitvs_op_attention_plan(int32_t precision, int32_t n_img, int32_t N, int32_t H, int32_t* out);
/* the Gram stage a handle (precision, binned descriptors, T tokens, model width D, max_pairs) runs for a call of n_pairs pairs, no
 * device work: out[0..6] = form, tile rows, columns, k-groups, band rows, workgroups per XCD, split operands.  Forms: 1 fused
 * arg-max over fp32 descriptors; 2 the same from the fp16 hi / lo split (16-bit modes from 1024 tokens); 3 raw token Gram + 3 x 3
 * stencil arg-max (binned; the tile is the raw Gram's); 4 binned descriptors taken 9 D wide (the raw Gram workspace would pass
 * 8 GiB).  Returns 0, or -2 when unlaunchable. */
VITVS_API int vitvs_op_gram_plan(int32_t precision, int32_t binned, int32_t T, int32_t D, int32_t n_pairs, int32_t max_pairs,
                       int32_t* out);
/* the control law's launch for T tokens, max_rows feature pairs, robust_law = robust_iters, the refinement's source (0 off, 1 a
 * given table, 2 the raw Gram, 3 the normalised descriptors) and option interaction, no device work: out[0..6] = the ROBUST, REFINE
 * and GOALZ instantiation bits, dynamic LDS bytes, the source, whether the current depth image is read, and whether at any pixel
 * (else at patch centres only).  Returns 0, -2 for an argument out of range (out is the plain law's of no tokens), or -3 past
 * 160 KiB of LDS (out filled). */
VITVS_API int vitvs_op_servo_plan(int32_t T, int32_t max_rows, int32_t robust_iters, int32_t refine_source, int32_t interaction,
                        int32_t* out);
/* The rig law's kernel (vitvs_rig_velocity_dev, include/vitvs.h) on caller systems, no handle and no forward:
 *   rows    int32 [n_cams], the rows of camera i's system (0 .. ld); 0: the camera does not contribute
 *   L       double [n_cams][7][ld], column-major as vitvs_last_details returns it: L_i's six columns, then e_i
 *   W       double [n_cams][36], row-major W_i;  v_rig = -lambda pinv(stack_i(L_i W_i)) stack_i(e_i)
 *   scratch vitvs_op_rig_scratch_bytes(n_cams, ld) = 256 + 8 (32 n_cams + 14 n_cams ld) bytes of device memory (hipMalloc),
 *           zeroed by the caller before the FIRST call only (its first word is the hand-off's ticket, which every launch
 *           leaves zero; a block may serve calls of other n_cams and ld that fit it)
 *   v_rig [6], rig_status, rig_info [8] or NULL, normal [28] or NULL as vitvs_rig_velocity_dev's; a camera without rows counts
 *   as VITVS_TOO_FEW.  Everything is device memory; one launch on `stream`.
 * Returns 0, -1 (a null required pointer), -2 (n_cams outside 1 .. 256, ld < 1). */
VITVS_API int vitvs_op_rig_law(int32_t n_cams, const int32_t* rows, const double* L, int32_t ld, const double* W, double lambda,
                     void* scratch, double* v_rig, int32_t* rig_status, int32_t* rig_info, double* normal, void* stream);
VITVS_API int vitvs_op_rig_scratch_bytes(int32_t n_cams, int32_t ld);   /* -2 as above, -3 past 2 GiB */
/* Measurement hook (tools/rig_times.py): on != 0 makes the calling thread's vitvs_op_rig_law run as two plain launches (the
 * cameras' sums, then the solve) instead of the one launch with its in-launch fan-in.  Same results bit for bit.  Returns the
 * previous setting. */
VITVS_API int vitvs_op_rig_two_launches(int32_t on);
/* The robust rig law's kernel (vitvs_rig_robust_velocity_dev, include/vitvs.h) on caller systems:
 *   rows, L, ld, W, lambda, v_rig, rig_status   as vitvs_op_rig_law's; a camera's rows count in pairs (an odd last row is dropped)
 *   live    int32 [n_cams] or NULL: the live pairs of camera i, the first of its rows (clamped to rows / 2); NULL: every pair.
 *           A camera without rows or without a live pair does not contribute.
 *   n_iter  1 .. 16;  sigma_min  the floor of the scale, given directly
 *   scratch vitvs_op_rig_robust_scratch_bytes(n_cams, ld) = vitvs_op_rig_scratch_bytes + 8 * 7 n_cams ld bytes, zeroed before the
 *           FIRST call only; the plain op may use the same block
 *   rig_info [8], normal [28], sigma [1] or NULL as vitvs_rig_robust_velocity_dev's; weights double [n_cams][ld / 2] or NULL
 * Returns 0, -1 (a null required pointer), -2 (n_cams outside 1 .. 256, ld < 1, n_iter outside 1 .. 16), -3 (the plan's). */
VITVS_API int vitvs_op_rig_robust_law(int32_t n_cams, const int32_t* rows, const int32_t* live, const double* L, int32_t ld,
                            const double* W, double lambda, int32_t n_iter, double sigma_min, void* scratch, double* v_rig,
                            int32_t* rig_status, int32_t* rig_info, double* normal, double* weights, double* sigma, void* stream);
VITVS_API int vitvs_op_rig_robust_scratch_bytes(int32_t n_cams, int32_t ld);   /* -2 as above, -3 past 2 GiB */
/* The launch plan of the robust rig law for n_cams cameras of ld rows (host arithmetic, no device): out[0] the dynamic LDS bytes
 * = 8 (260 + (resident ? 7 * 384 : 0) + 2 pairs), out[1] 1 when the last arriver's copy of the stack is LDS-resident
 * (n_cams ld <= 384 rows: 8 cameras x 48), out[2] pairs = n_cams (ld / 2), the residuals and weights held in LDS, out[3] 1 when
 * the launch opts in to more than 64 KiB.  Returns 0, -1 (out NULL), -2 (n_cams outside 1 .. 256, ld < 1; out untouched but
 * zeroed), -3 (out filled): more than 160 KiB of LDS. */
VITVS_API int vitvs_op_rig_robust_plan(int32_t n_cams, int32_t ld, int32_t* out);
/* The pose law's kernel (vitvs_pose_velocity_dev, include/vitvs.h) on caller-given points:
 *   P, Q     device double [n_pairs][ld][3]: current and goal points;  usable int32 [n_pairs][ld]: > 0 usable, 0 padded, < 0 a hole
 *   n_iter   0 .. 16;  sigma_min  the floor of the scale, given directly
 *   scratch  vitvs_op_pose_scratch_bytes(n_pairs, ld) = 8 * 7 n_pairs ld bytes
 *   v_pose [n_pairs][6], pose_status [n_pairs]; pose [n_pairs][12], pose_info [n_pairs][8], weights [n_pairs][ld], sigma [n_pairs] or NULL
 * Returns 0, -1 (a null required pointer), -2 (n_pairs or ld < 1, n_iter outside 0 .. 16), -3 (the plan's). */
VITVS_API int vitvs_op_pose_law(int32_t n_pairs, int32_t ld, const double* P, const double* Q, const int32_t* usable, double lambda,
                                int32_t n_iter, double sigma_min, void* scratch, double* v_pose, int32_t* pose_status, double* pose,
                                int32_t* pose_info, double* weights, double* sigma, void* stream);
VITVS_API int vitvs_op_pose_scratch_bytes(int32_t n_pairs, int32_t ld);   /* -2 as above, -3 past 2 GiB */
/* The launch plan of the pose law (host arithmetic, no device): out[0] the dynamic LDS bytes = 8 (320 + (n_iter > 0 ? 2 max_rows :
 * 0)), out[1] 1 for the robust instantiation, out[2] 1 when the launch opts in to more than 64 KiB.  Returns 0, -1 (out NULL),
 * -2 (max_rows < 1, n_iter outside 0 .. 16; out zeroed), -3 (out filled): more than 160 KiB of LDS. */
VITVS_API int vitvs_op_pose_plan(int32_t max_rows, int32_t n_iter, int32_t* out);
/* vitvs_op_pose_law with the consensus start in front of its alignment loop (vitvs_pose_consensus_velocity_dev, include/vitvs.h):
 * n_hyp 0 .. 4096 three-point hypotheses drawn from `seed`; n_hyp = 0 is vitvs_op_pose_law bit for bit.  The cut-off is T = 4.6851
 * sigma_min.  pose_info[6] = the winner's j + 1 (0: n_hyp = 0, fewer than 3 usable rows, or every hypothesis skipped), pose_info[7]
 * = the start weights at 1.  Returns as vitvs_op_pose_law, and -2 also for n_hyp outside 0 .. 4096 and for n_hyp > 0 with
 * sigma_min <= 0. */
VITVS_API int vitvs_op_pose_consensus_law(int32_t n_pairs, int32_t ld, const double* P, const double* Q, const int32_t* usable,
                                          double lambda, int32_t n_iter, double sigma_min, void* scratch, double* v_pose,
                                          int32_t* pose_status, double* pose, int32_t* pose_info, double* weights, double* sigma,
                                          void* stream, int32_t n_hyp, uint32_t seed);
/* The launch plan with the consensus start: out[0] the dynamic LDS bytes = 8 (320 + (n_iter > 0 ? 2 max_rows : n_hyp > 0 ? max_rows
 * : 0) + (n_hyp > 0 ? 8 + (max_rows + 1) / 2 : 0)): the reduction cells (4 costs, 4 + 4 ints) and the usable rows as ints; without
 * re-weightings the consensus form keeps the rows' Z* for the median behind its cut-off.  out[1] and out[2] as vitvs_op_pose_plan's,
 * out[3] 1 for the consensus instantiation.  Returns 0, -1 (out NULL), -2 (as vitvs_op_pose_plan, or n_hyp outside 0 .. 4096; out
 * zeroed), -3 (out filled): more than 160 KiB of LDS. */
VITVS_API int vitvs_op_pose_consensus_plan(int32_t max_rows, int32_t n_iter, int32_t n_hyp, int32_t* out);
/* The homography law's kernel (vitvs_homography_velocity_dev, include/vitvs.h) on caller-given points:
 *   m, ms    device double [n_pairs][ld][2]: current and goal normalised image points;  usable int32 [n_pairs][ld]: > 0 usable
 *   depth_scale > 0 and finite;  n_iter 0 .. 16;  sigma_min  the floor of the scale, given directly
 *   scratch  vitvs_op_homography_scratch_bytes(n_pairs, ld) = 8 * 5 n_pairs ld bytes
 *   v_h [n_pairs][6], h_status [n_pairs]; H [n_pairs][9], h_info [n_pairs][8], weights [n_pairs][ld], sigma [n_pairs] or NULL
 * Returns 0, -1 (a null required pointer), -2 (n_pairs or ld < 1, n_iter outside 0 .. 16, depth_scale <= 0 or not finite), -3 (the
 * plan's). */
VITVS_API int vitvs_op_homography_law(int32_t n_pairs, int32_t ld, const double* m, const double* ms, const int32_t* usable,
                                      double lambda, double depth_scale, int32_t n_iter, double sigma_min, void* scratch, double* v_h,
                                      int32_t* h_status, double* H, int32_t* h_info, double* weights, double* sigma, void* stream);
VITVS_API int vitvs_op_homography_scratch_bytes(int32_t n_pairs, int32_t ld);   /* -2 as above, -3 past 2 GiB */
/* The launch plan of the homography law (host arithmetic, no device): out[0] the dynamic LDS bytes = 8 (752 + (n_iter > 0 ? 2
 * max_rows : 0)), out[1] 1 for the robust instantiation, out[2] 1 when the launch opts in to more than 64 KiB.  Returns 0, -1 (out
 * NULL), -2 (max_rows < 1, n_iter outside 0 .. 16; out zeroed), -3 (out filled): more than 160 KiB of LDS. */
VITVS_API int vitvs_op_homography_plan(int32_t max_rows, int32_t n_iter, int32_t* out);
/* vitvs_op_homography_law with the consensus start in front of its solve loop (vitvs_homography_consensus_velocity_dev,
 * include/vitvs.h): n_hyp 0 .. 4096 four-point hypotheses drawn from `seed`; n_hyp = 0 is vitvs_op_homography_law bit for bit.
 * The cut-off is T = 4.6851 sigma_min.  h_info[6] = the winner's j + 1 (0: n_hyp = 0, fewer than 4 usable rows, or every hypothesis
 * skipped), h_info[7] = the start weights at 1.  Returns as vitvs_op_homography_law, and -2 also for n_hyp outside 0 .. 4096 and
 * for n_hyp > 0 with sigma_min <= 0. */
VITVS_API int vitvs_op_homography_consensus_law(int32_t n_pairs, int32_t ld, const double* m, const double* ms, const int32_t* usable,
                                                double lambda, double depth_scale, int32_t n_iter, double sigma_min, void* scratch,
                                                double* v_h, int32_t* h_status, double* H, int32_t* h_info, double* weights,
                                                double* sigma, void* stream, int32_t n_hyp, uint32_t seed);
/* The launch plan with the consensus start: out[0] the dynamic LDS bytes = 8 (752 + (n_iter > 0 ? 2 max_rows : 0) + (n_hyp > 0 ?
 * 8 + (max_rows + 1) / 2 : 0)): the reduction cells (4 costs, 4 + 4 ints) and the usable rows as ints, out[1] and out[2] as
 * vitvs_op_homography_plan's, out[3] 1 for the consensus instantiation.  Returns 0, -1 (out NULL), -2 (as vitvs_op_homography_plan,
 * or n_hyp outside 0 .. 4096; out zeroed), -3 (out filled): more than 160 KiB of LDS. */
VITVS_API int vitvs_op_homography_consensus_plan(int32_t max_rows, int32_t n_iter, int32_t n_hyp, int32_t* out);
/* The pose rig law's kernel (vitvs_pose_rig_velocity_dev, include/vitvs.h) on caller-given camera-frame points:
 *   P, Q        device double [n_cams][ld][3];  usable int32 [n_cams][ld]: > 0 usable, 0 padded, < 0 a hole
 *   rTc         device double [n_cams][12]: R_i row-major, then t_i;  cam_status int32 [n_cams] or NULL (all VITVS_OK)
 *   n_iter      0 .. 16;  sigma_min  the floor of the scale, given directly
 *   scratch     vitvs_op_pose_rig_scratch_bytes(n_cams, ld) = 8 * 7 n_cams ld bytes
 *   v_rig [6], rig_status [1]; pose [12], rig_info [8], moments [18], weights [n_cams][ld], sigma [1] or NULL
 * Returns 0, -1 (a null required pointer), -2 (n_cams or ld < 1, n_iter outside 0 .. 16), -3 (the plan's). */
VITVS_API int vitvs_op_pose_rig_law(int32_t n_cams, int32_t ld, const double* P, const double* Q, const int32_t* usable,
                                    const double* rTc, const int32_t* cam_status, double lambda, int32_t n_iter, double sigma_min,
                                    void* scratch, double* v_rig, int32_t* rig_status, double* pose, int32_t* rig_info,
                                    double* moments, double* weights, double* sigma, void* stream);
VITVS_API int vitvs_op_pose_rig_scratch_bytes(int32_t n_cams, int32_t ld);   /* -2 as above, -3 past 2 GiB */
/* The launch plan of the pose rig law (host arithmetic, no device): out[0] the dynamic LDS bytes = 8 (320 + (n_iter > 0 ? 2 n_cams
 * ld : 0)), out[1] 1 for the robust instantiation, out[2] 1 when the launch opts in to more than 64 KiB.  Returns 0, -1 (out
 * NULL), -2 (n_cams or ld < 1, n_cams ld past 2^24 rows, n_iter outside 0 .. 16; out zeroed), -3 (out filled): more than 160 KiB
 * of LDS. */
VITVS_API int vitvs_op_pose_rig_plan(int32_t n_cams, int32_t ld, int32_t n_iter, int32_t* out);
/* The fused Gram arg-max of the velocity path on caller-normalised descriptors dn [n_des + n_pairs][T][Dp] fp32 (desired frames
 * first; n_des = 1 with des_shared): the plan of vitvs_op_gram_plan(precision, 0, T, Dp, n_pairs, n_pairs), the split into dh
 * (3 (n_des + n_pairs) T Dp fp16, only when the plan splits) and the keys row_best / col_best [n_pairs][T] (cleared here), decoded
 * into nn_1 / nn_2 / sim_1 [n_pairs][T]. */
VITVS_API int vitvs_op_gram_argmax(int32_t precision, const float* dn, int32_t T, int32_t Dp, int32_t n_pairs, int32_t des_shared,
                         void* dh, uint64_t* row_best, uint64_t* col_best, int32_t* nn_1, int32_t* nn_2, float* sim_1,
                         void* stream);
/* The binned form: x = residual-stream rows [n_des + n_pairs][P + T][D] fp32 (P prefix rows skipped), grid * grid = T.  Token
 * squared norms into sq [n_des + n_pairs][T], raw token Gram into G [n_pairs][T][T], stencil arg-max into the keys, decoded as
 * above. */
VITVS_API int vitvs_op_gram_stencil(const float* x, int32_t T, int32_t P, int32_t D, int32_t grid, int32_t n_pairs,
                          int32_t des_shared, float* G, float* sq, uint64_t* row_best, uint64_t* col_best, int32_t* nn_1,
                          int32_t* nn_2, float* sim_1, void* stream);
VITVS_API int vitvs_op_linear_partial(int32_t precision, const void* A, const void* W, float* part, int32_t M, int32_t N,
                            int32_t K, int32_t slices, void* stream);
VITVS_API int vitvs_op_residual_ln(int32_t precision, float* x, const float* part, int32_t slices, const float* bias,
                         const float* ls, const float* gamma, const float* beta, void* out, int32_t M, int32_t D,
                         float eps, void* stream);

/* The two ends of the forward (csrc/elementwise.hip; tests/test_gpu_ends_cover.py).  No handle, no planning: the arguments go
 * straight to the launch.  T = grid * grid patch tokens per image, P = prefix rows per image (cls + register tokens), x the fp32
 * residual stream [n_img][P + T][D], D in {128,256,384,768,1024} where a LayerNorm or a K-slice sum takes part.
 *
 * Patch rows: Ape[(img * T + t)][k] = ((u8 / 255) - mean[c]) / std[c] in `precision`, k = c p^2 + py p + px, every step rounded
 * to nearest in fp32; +0 for 3 p^2 <= k < Kp.  Images are the n_des frames of `des` then the n_cur of `cur` (either may be NULL
 * with a count of 0), RGB u8 [S][S][3]; grid = 1 + (S - patch) / stride.  Of x only the class rows x[img * (T + prefix)][:] =
 * cls + pos[0] are written.  mean / std are HOST arrays of 3.  in_h = in_w = 0: frames arrive at S x S.  Otherwise they are camera
 * frames [in_h][in_w][3] and u8 is the pixel of Pillow's bicubic resize to S x S, computed while the row is built: the hook builds
 * the tables, uploads them, launches, synchronises the stream and frees them.  -3 when the camera rows of one patch pass the
 * 64 KiB of LDS (as vitvs_set_frame_size). */
VITVS_API int vitvs_op_patchify(int32_t precision, const uint8_t* des, int32_t n_des, const uint8_t* cur, int32_t n_cur, int32_t S,
                      int32_t patch, int32_t stride, int32_t Kp, int32_t D, int32_t prefix, const float* mean, const float* std,
                      const float* cls, const float* pos, int32_t in_h, int32_t in_w, void* Ape, float* x, void* stream);
/* Finishes a split-K patch embedding, part [slices][n_img * T][D] fp32 (1 .. 8 slices, summed in index order):
 *   x[img][0] = cls + pos[0];  x[img][r] = reg[r - 1] for 1 <= r < P (no position, no bias; reg may be NULL when P = 1);
 *   x[img][P + t] = pos[1 + t] + sum_z part[z][img * T + t] + bias;  out = LayerNorm(x) * gamma + beta in `precision`.
 * x is written only (its previous contents are not read). */
VITVS_API int vitvs_op_embed_ln(int32_t precision, float* x, const float* part, int32_t slices, const float* bias, const float* pos,
                      const float* cls, const float* reg, const float* gamma, const float* beta, void* out, int32_t n_img, int32_t T,
                      int32_t P, int32_t D, float eps, void* stream);
/* The forward's last launch: vitvs_op_residual_ln without a LayerNorm on M = n_img * (T + P) rows, which also writes, for the
 * patch rows only, dn[img][t][:] = x_row / max(|x_row|, 1e-8) and / or sq[img * T + t] = |x_row|^2 of the updated row (either
 * may be NULL, not both) and clears zero_count <= M * 64 64-bit words of zero_a and zero_b.  `precision` selects the
 * instantiation only (nothing is written in it).  -2 for arguments out of range. */
VITVS_API int vitvs_op_residual_desc(int32_t precision, float* x, const float* part, int32_t slices, const float* bias, const float* ls,
                           float* dn, float* sq, uint64_t* zero_a, uint64_t* zero_b, int32_t zero_count, int32_t T, int32_t P,
                           int32_t M, int32_t D, void* stream);
/* Descriptors from x: plain (binned = 0) dn[img][t][D] = x[img][P + t] / max(norm, 1e-8) (D <= 1024, dn required); binned
 * dn[img][t][9 D] = the 3 x 3 replicate-clamped neighbourhood in row-major (dy, dx) order, normalised as a whole, through the
 * squared-norm workspace sq_ws [n_img * T] (dn may be NULL when raw is given).  raw (may be NULL): the same rows un-normalised.
 * zero_count <= n_img * T * 64 words of zero_a / zero_b are cleared.  -2 when grid * grid != T or an argument is out of range. */
VITVS_API int vitvs_op_descriptors(const float* x, float* dn, float* raw, float* sq_ws, int32_t n_img, int32_t T, int32_t P, int32_t grid,
                         int32_t D, int32_t binned, uint64_t* zero_a, uint64_t* zero_b, int32_t zero_count, void* stream);
/* out[img][t][d * H + h] (fp32) = float(qkv[img * (P + T) + P + t][which][h][d]) * unscale, which = 0 q, 1 k, 2 v; keep_cls = 0:
 * out [n_img][T][64 H]; 1: out [n_img][1 + T][64 H] with the class row first.  Register rows are dropped. */
VITVS_API int vitvs_op_facet(int32_t precision, const void* qkv, float* out, int32_t n_img, int32_t T, int32_t P, int32_t H, int32_t which,
                   float unscale, int32_t keep_cls, void* stream);
/* out[img][t] (fp32): softmax over all P + T keys of q_cls . k / 8 per chosen head (q_prescaled != 0: 2^(q_cls . k), the q third
 * carrying 0.125 * log2(e)), patch columns kept, mean over the n_heads heads of head_idx (a HOST array, 1 .. 16 entries in
 * 0 .. H - 1), min-max normalised per image.  fp32, bf16 and fp16 only; -2 for VITVS_F16X2 and for a head out of range, -3 when
 * 2 T + P floats pass 64 KiB of LDS. */
VITVS_API int vitvs_op_saliency(int32_t precision, const void* qkv, float* out, int32_t n_img, int32_t T, int32_t P, int32_t H,
                      const int32_t* head_idx, int32_t n_heads, int32_t q_prescaled, void* stream);
/* dst[r][:] = src[r][:] / max(|src[r]|, 1e-8), fp32 rows of any width Dp >= 1 */
VITVS_API int vitvs_op_normalize_rows(const float* src, float* dst, int32_t rows, int32_t Dp, void* stream);
/* The kernel of selection mode VITVS_SELECT_BEST alone on given tables (device pointers nn_1, nn_2 int32 and sim_1 fp32
 * [n_pairs][T]): order int32 [n_pairs][T] as vitvs_last_order states it, for `cells` in 1 .. 16 image cells per side.  The tables
 * are packed into the keys the law reads, as vitvs_servo_from_nn_dev packs them, in scratch memory of the call's own; the call
 * returns after the launches have finished.  -2 when T is not a square grid or an argument is out of range, -3, without a launch,
 * when T keys do not fit in 160 KiB of LDS. */
VITVS_API int vitvs_op_best_order_dev(int32_t T, int32_t cells, int32_t n_pairs, const int32_t* nn_1, const int32_t* nn_2,
                            const float* sim_1, int32_t* order, void* stream);
/* The two kernels of the roll search (vitvs_roll_velocity_dev) alone.  vitvs_op_quarter_turns: out [n][4][S][S][3] <- frames
 * [n][S][S][3] uint8 (device pointers), copy k = numpy.rot90(frame, k), for any S >= 1; -2 for an argument out of range. */
VITVS_API int vitvs_op_quarter_turns(const uint8_t* frames, int32_t n, int32_t S, uint8_t* out, void* stream);
/* vitvs_op_roll_pick: the four candidates' tables (device pointers nn_1, nn_2 int32 and sim_1 fp32 [4][T]) -> the winner's tables
 * in the unturned frame (nn_1_out, nn_2_out, sim_1_out [T]; candidate 0's when nobody is valid), roll_info int32 [8] and scores
 * double [4] as vitvs_roll_velocity_dev states them.  The tables are packed into the keys the law reads in scratch memory of the
 * call's own; the call returns after the launches have finished.  -2 when T is not a square grid. */
VITVS_API int vitvs_op_roll_pick(int32_t T, const int32_t* nn_1, const int32_t* nn_2, const float* sim_1, int32_t* nn_1_out,
                                 int32_t* nn_2_out, float* sim_1_out, int32_t* roll_info, double* scores, void* stream);

#ifdef __cplusplus
}
#endif
#endif
