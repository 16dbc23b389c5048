/*
 * vitvs.h — C ABI of the MI355X-native ViT-VS hot path (libvitvs_hip.so).
 *
 * The reference (begbaj/ViT-VS) has no FFI: the hot path sits behind Python bound methods.
 * Each entry point below names the reference interface it replaces (paths under
 * /root/reference/catkin_ws/ibvs/src unless noted).  The Python binding a maintainer adds is
 * shown in INTEGRATION.md (ctypes), and vit-vs_amd/_lib.py is exactly that binding.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in signatures (streams travel as void*).
 *   - every function returns a status: 0 ok, > 0 a servo status (enum below), < 0 an error;
 *     vitvs_last_error() gives the message.  Nothing throws across the boundary.
 *   - "_dev" functions take DEVICE pointers and enqueue work on the given hipStream_t (void*,
 *     NULL = the null stream) without synchronising; outputs are valid once the stream has reached
 *     the end of the call's work.  The un-suffixed forms take HOST pointers, copy, run and wait.
 *   - inputs are borrowed for the duration of the call; outputs go to caller-allocated buffers;
 *     the handle owns the device weights and workspaces.  A handle is bound to the HIP device that
 *     was current when it was created: every entry point that takes a handle runs on that device
 *     (and restores the caller's current device before returning), so handles of several GPUs may be
 *     driven from one thread.
 *   - ordering of the calls on ONE handle (they share its workspaces; a handle is not thread-safe):
 *     a host-pointer form orders itself behind the _dev work the handle still has pending on a
 *     caller's stream — if a _dev call was made since the last host-pointer call it synchronises the
 *     device before its first launch, else it makes no extra HIP call — and has finished when it
 *     returns, so a _dev call made after it needs nothing either.  _dev calls on one stream run in
 *     stream order.  Two _dev calls on DIFFERENT streams remain the caller's to order (an event, a
 *     synchronisation), and so does a replay of a graph the CALLER captured around a _dev call: the
 *     library sees the capture, not the replays.
 *   - images are RGB uint8, HWC, already resized to img_size x img_size (reference:
 *     vitvs_v2.py:474-475 PIL resize happens before the path; dinov2_extractor.py:177-191);
 *     vitvs_resize_frames_dev does that resize on the device, bit-identically to PIL, and after
 *     vitvs_set_frame_size the path takes camera-resolution frames and resizes while it builds its patch rows.
 *   - depth is the sensor's uint16 millimetre image, 0 = invalid (reference:
 *     realsense_gazebo_plugin/src/RealSensePlugin.cpp:250-262, consumed at vitvs_v2.py:566-586).
 */
#ifndef VITVS_H
#define VITVS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VITVS_ABI_VERSION 2   /* 2: num_pairs became a per-call argument of the velocity / servo entry points */
#define VITVS_API __attribute__((visibility("default")))

typedef struct vitvs_handle vitvs_handle;

/* operand type of the GEMMs and of attention (accumulation is always fp32, the residual stream, LayerNorm statistics,
 * descriptors and the correspondence fp32, the control law fp64): F32 = parity mode, BF16 = throughput mode, F16 = the
 * other 16-bit mode (BASELINE.json configs[4] names fp16; 11-bit significand, same speed as bf16) */
/* VITVS_F16X2 ("split-f16"): every GEMM / attention operand is kept as an fp16 hi / lo pair (22 significant bits) and every
 * contraction runs as hi.hi + hi.lo + lo.hi on the f16 matrix cores with fp32 accumulation: the reference's fp32 arithmetic
 * (dinov2_extractor.py:245-263: no autocast anywhere) to fp32 rounding, at 16-bit matrix rate instead of the fp32 matrix
 * pipe's 1/16 of it.  The parity mode at servo rate; same results class as VITVS_F32 (bit-exact arg-max tables on the
 * fixtures, tokens to 2e-5). */
enum vitvs_precision { VITVS_F32 = 0, VITVS_BF16 = 1, VITVS_F16 = 2, VITVS_F16X2 = 3 };

/* Servo status (reference error convention):
 *   NO_CORRESPONDENCE  find_correspondences_batch returned (None, None, None)   vitvs_v2.py:155, 500-505
 *   TOO_FEW            < 4 matches: calculate_uv returns all-zero features       vitvs_v2.py:539-541
 *   NO_DEPTH           no depth image: ibvs() returns early                      vitvs_v2.py:616-619 */
enum vitvs_status { VITVS_OK = 0, VITVS_NO_CORRESPONDENCE = 1, VITVS_TOO_FEW = 2, VITVS_NO_DEPTH = 3 };

/* How the servo features are drawn from the mutual-nearest-neighbour candidates
 * (reference: torch.randperm subset, vitvs_v2.py:134-141; see DESIGN.md "Selection"). */
enum vitvs_select {
    VITVS_SELECT_EXPLICIT = 0, /* caller passes the chosen token ids of the desired frame            */
    VITVS_SELECT_ORDER = 1,    /* caller passes a visiting order (permutation of 0..T-1); the first  */
                               /* num_pairs candidates met in that order are used                    */
    VITVS_SELECT_DENSE = 2,    /* every candidate, ascending token id (no zero padding)              */
    VITVS_SELECT_BEST = 3      /* an extension beyond the reference: ORDER on a visiting order made  */
                               /* on the device, deterministic: candidates ranked by similarity and  */
                               /* taken round-robin over a grid of image cells (option               */
                               /* "select_cells"); nothing comes from the caller                     */
};

typedef struct vitvs_config {
    int32_t abi_version;  /* VITVS_ABI_VERSION */
    /* extractor geometry (reference: ViTExtractor.__init__, dinov2_extractor.py:25-55) */
    int32_t img_size;     /* S */
    int32_t patch;        /* p */
    int32_t stride;       /* patch-embed stride (== patch unless the stride hack is used, :122-144) */
    int32_t dim;          /* D, multiple of 128 */
    int32_t heads;        /* H, D / H must be 64 */
    int32_t blocks;       /* blocks to run = layer + 1 (descriptor = output of blocks[layer], :226-229) */
    int32_t layerscale;   /* 1: DINOv2 layout with ls1/ls2 gammas (dino_patch/block.py:73,85) */
    float mean[3];        /* Normalize constants (dinov2_extractor.py:49-50) */
    float std[3];
    float ln_eps;         /* 1e-6 */
    int32_t precision;    /* vitvs_precision of the ViT GEMMs/attention; the correspondence and the law are fp32/fp64 */
    int32_t binned;       /* 1: 3x3 log-bin descriptors (use_feature_binning, dinov2_extractor.py:265-311).  The velocity calls take
                           * the similarities of the 9D-wide descriptors as a 3x3 stencil over the D-wide Gram of the raw tokens
                           * (same values to fp32 rounding; one T x T fp32 workspace per pair); the extract_* calls return the
                           * concatenated descriptors */
    /* control law (reference: config.yaml:1-17; vitvs_v2.py:278-295) */
    int32_t num_pairs;    /* default feature-pair count of a call that passes num_pairs <= 0 */
    int32_t u_max, v_max; /* camera resolution; also the depth image size */
    double lambda;
    /* capacity */
    int32_t max_pairs;    /* frame pairs per call (B) */
    int32_t max_rows;     /* feature pairs per frame pair the law may use (>= num_pairs; >= T enables DENSE) */
} vitvs_config;

/* --- lifetime --------------------------------------------------------------------------------
 * Replaces ViTExtractor(model_type, stride, model=...) + model.to(device) (dinov2_extractor.py:25-55). */
VITVS_API int vitvs_create(const vitvs_config* cfg, vitvs_handle** out);
/* The same for a network with register tokens (DINOv2 "_reg" models, Darcet et al. 2023: dinov2_vit{s,b,l}14_reg have 4).
 * Every image's token rows are then [cls + pos[0], reg_0 .. reg_{R-1}, patch_t + pos[1 + t]] — the registers are inserted
 * after the position embedding and carry none — so N = 1 + R + T rows go through every block.  The registers never enter a
 * descriptor, the correspondence or the control law; pos_embed stays [1 + T][D].  register_tokens is 0 ..
 * VITVS_MAX_REGISTER_TOKENS (checked before the device is touched); vitvs_create(cfg, out) is vitvs_create_ex(cfg, 0, out). */
#define VITVS_MAX_REGISTER_TOKENS 16
VITVS_API int vitvs_create_ex(const vitvs_config* cfg, int32_t register_tokens, vitvs_handle** out);
/* R of the handle (0 for vitvs_create), -1 for NULL. */
VITVS_API int vitvs_register_tokens(const vitvs_handle* h);
VITVS_API void vitvs_destroy(vitvs_handle* h);
VITVS_API const char* vitvs_last_error(const vitvs_handle* h); /* h may be NULL: last creation error */
VITVS_API int vitvs_abi_version(void);

/* --- weights ---------------------------------------------------------------------------------
 * Replaces model.load_state_dict (dinov2_extractor.py:79-82).  `name` is the DINO/timm/DINOv2
 * state-dict key (patch_embed.proj.weight, cls_token, pos_embed — already resampled to the token
 * grid, shape [1+T][D] —, blocks.{i}.norm1.weight, ... , blocks.{i}.ls2.gamma); `data` is fp32 on
 * the host.  vitvs_weights_ready returns 0 when every tensor the forward reads has been set.  A handle with R > 0 register
 * tokens (vitvs_create_ex) also needs "register_tokens", R * D elements; a wrong count, or the name on a handle with R == 0,
 * is error -5. */
VITVS_API int vitvs_set_tensor(vitvs_handle* h, const char* name, const float* data, int64_t numel);
VITVS_API int vitvs_weights_ready(const vitvs_handle* h);

/* --- the hot path ----------------------------------------------------------------------------
 * compute_velocity(I_cur, I_des, Z, K) -> v_c : Controller.detect_features() + Controller.ibvs()
 * up to the raw (pre-EMA) twist (vitvs_v2.py:464-523, 588-622).
 *   n_pairs          frame pairs in this call (<= max_pairs)
 *   I_cur, I_des     uint8 [n_pairs][S][S][3]; if des_shared != 0, I_des is ONE image used for all
 *                    pairs (rotation compensation, vitvs_v2.py:1151-1189); I_des == NULL: the goal cached by
 *                    vitvs_set_goal[_dev] (below)
 *   Z_mm             uint16 [n_pairs][v_max][u_max], or NULL -> status NO_DEPTH
 *   K                double [n_pairs][4] = fx, fy, cx, cy
 *   select_mode      vitvs_select; `selection` int32: EXPLICIT [n_pairs][num_pairs] token ids with
 *                    n_selected[n_pairs] counts; ORDER [n_pairs][T]; DENSE and BEST ignored (NULL)
 *   num_pairs        feature pairs of the control law for THIS call (the reference's Controller.num_pairs, which its
 *                    callers change between calls: 24 in the servo loop, 48 in find_and_set_best_pose,
 *                    vitvs_v2.py:1151-1189); 1 .. cfg.max_rows, or <= 0 for cfg.num_pairs
 *   v_c              double [n_pairs][6] = vx, vy, vz, wx, wy, wz (camera optical frame)
 *   status           int32 [n_pairs] vitvs_status
 * The return value is < 0 on error, else 0 (per-pair statuses are in `status`). */
VITVS_API int vitvs_compute_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                               int32_t des_shared, const uint16_t* Z_mm, const double* K, int32_t select_mode,
                               const int32_t* selection, const int32_t* n_selected, int32_t num_pairs, double* v_c,
                               int32_t* status, void* stream);
VITVS_API int vitvs_compute_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                           int32_t des_shared, const uint16_t* Z_mm, const double* K, int32_t select_mode,
                           const int32_t* selection, const int32_t* n_selected, int32_t num_pairs, double* v_c,
                           int32_t* status);
/* The host-pointer form is the reference's seam as it is called (numpy arrays in, a numpy twist out: vitvs_v2.py:464-523,
 * 588-632).  Per call the buffers are copied into a block of pinned, device-visible host memory the handle owns (plain memcpy):
 * the frames go on to device memory in one short copy launch each on the update's own stream, the depth image is copied after the
 * forward has been enqueued — only the pixels the law can read, the tokens' patch centres — and read in place by the law's
 * kernel, the twist and the status are written into the pinned block by that kernel and the detail block (vitvs_last_details:
 * everything but `selected` and `L`) follows in one copy launch: one polled wait, no copy-engine command.  Option "reuse_goal_frames" (vitvs_set_option, 0 / 1, default 0): while I_des repeats the
 * previous call's ADDRESS (and frame count and geometry) the goal frames already staged in device memory are forwarded again as
 * they are — for callers that keep the goal image in a buffer they never write to (a servo loop's goal image is fixed:
 * vitvs_v2.py:264); the goal's tokens are still recomputed on every update, like the reference does.
 *
 * vitvs_reselect: the reference draws its features on the HOST between the correspondence and the law
 * (find_correspondences_batch: sort + torch.randperm, vitvs_v2.py:127-141).  After a host-pointer velocity call the tables are
 * in host memory (vitvs_last_details: nn_1, nn_2, sim_1); the caller draws, and this entry point evaluates the law for that
 * selection on what the call left in the handle (arg-max keys on the device, depth image and intrinsics in the pinned block):
 * one launch, no forward, no staging.  selection / n_selected / num_pairs as in vitvs_compute_velocity; error -5 unless the
 * handle's last velocity call was a host-pointer one. */
VITVS_API int vitvs_reselect(vitvs_handle* h, int32_t select_mode, const int32_t* selection, const int32_t* n_selected,
                             int32_t num_pairs, double* v_c, int32_t* status);

/* --- a goal image that does not change between updates ---------------------------------------------
 * The reference recomputes the goal image's tokens on every update (vitvs_v2.py:482-487), and so does the call above
 * whenever it is given I_des (the benchmarked form).  A servo loop keeps one goal image for a whole run: these two entry
 * points forward n_goal goal frames ONCE (uint8 [n_goal][S][S][3]; n_goal = the later calls' n_pairs, or 1 for des_shared
 * calls) and keep their descriptors in the handle; a later vitvs_compute_velocity[_dev] with I_des == NULL then forwards
 * only the current frames.  The cache is dropped by any call that forwards frames of its own choice through the handle
 * (a velocity call WITH I_des, vitvs_forward_tokens_dev, vitvs_extract_*) and by vitvs_correspond_dev / vitvs_refine_dev, whose
 * descriptors overwrite the cached ones: a NULL I_des without a matching cached goal is error -5.  vitvs_reselect,
 * vitvs_servo_from_nn[_ex]_dev, the follow-on laws and vitvs_set_option keep it (a goal forwarded under another "in_flight" hint
 * keeps that plan's summation order).  vitvs_roll_velocity[_dev] follows the velocity call: WITH I_des it drops the cache; with
 * I_des == NULL it matches its four turned copies against the cached goal of one image and keeps it, so a later call with a NULL
 * I_des servoes towards the same goal.  Results equal the recomputing call's up to the summation order of the GEMMs (the row
 * count differs). */
VITVS_API int vitvs_set_goal_dev(vitvs_handle* h, int32_t n_goal, const uint8_t* I_des, void* stream);
VITVS_API int vitvs_set_goal(vitvs_handle* h, int32_t n_goal, const uint8_t* I_des);

/* --- in front of it: camera frame -> extractor input -----------------------------------------------
 * goal_image.resize((S, S)) / latest_pil_image.resize((S, S)) (vitvs_v2.py:474-475; PIL default filter BICUBIC,
 * antialiased when shrinking).  frames uint8 [n][in_h][in_w][3] -> out uint8 [n][S][S][3], bit-identical to Pillow's
 * 8-bit resample (Resample.c).  The first call with a new (in_h, in_w) builds the coefficient tables on the host and
 * uploads them (one synchronisation); later calls only enqueue one launch. */
VITVS_API int vitvs_resize_frames_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, int32_t in_h, int32_t in_w,
                            uint8_t* out, void* stream);
/* The same resize INSIDE the path ("fused into the patch-embed load"): declares that every frame argument
 * handed to this handle from now on (I_cur, I_des, frames of every entry point above and below) is a camera frame
 * uint8 [in_h][in_w][3].  The launch that builds the patch rows then computes each pixel of the img_size x img_size image
 * PIL would have produced (same integer arithmetic as vitvs_resize_frames_dev, bit-identical) from the camera frame: no
 * resized image in memory, no extra launch.  (0, 0) or (img_size, img_size) restores frames at img_size x img_size.
 * Synchronises the device and rebuilds the tables when the geometry changes; cheap when it does not.  -3: the frame is too
 * large for the kernel's 64 KB of intermediate rows (several thousand pixels high) — use vitvs_resize_frames_dev. */
VITVS_API int vitvs_set_frame_size(vitvs_handle* h, int32_t in_h, int32_t in_w);

/* --- the seams inside it (same split as the reference's callables) ------------------------------
 * ViTExtractor.extract_descriptors(batch, layer, 'token', bin) (dinov2_extractor.py:313-337):
 * frames uint8 [n][S][S][3] -> desc fp32 [n][T][D'] (D' = D, or 9D when cfg.binned); raw, un-normalised. */
VITVS_API int vitvs_extract_descriptors_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, float* desc,
                                  void* stream);
/* The same call with facet = 'query' | 'key' | 'value' (bin = False, include_cls = False; dinov2_extractor.py:193-217,
 * 326-334): q / k / v of blocks[layer] for the patch tokens, fp32 [n][T][D] with descriptor index d * H + h.
 * facet: 0 query, 1 key, 2 value.  In bf16 mode the values carry the qkv GEMM's bf16 output rounding. */
VITVS_API int vitvs_extract_facet_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, int32_t facet, float* desc,
                            void* stream);
/* The extractor's whole descriptor surface, extract_descriptors(batch, layer, facet, bin, include_cls)
 * (dinov2_extractor.py:313-337): facet 0 query, 1 key, 2 value, 3 token; bin != 0: the 3x3 log-bin of that facet (:265-311),
 * desc fp32 [n][T][9 D]; include_cls != 0: the cls row is kept, desc [n][1 + T][D] (register tokens are always dropped);
 * neither: [n][T][D].  bin together with
 * include_cls is refused like the reference's assertion (error -5).  Independent of cfg.binned (which selects what the
 * velocity path correlates).  Raw, un-normalised values, like vitvs_extract_descriptors_dev. */
VITVS_API int vitvs_extract_descriptors_ex_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, int32_t facet, int32_t bin,
                                     int32_t include_cls, float* desc, void* stream);
/* ViTExtractor.extract_saliency_maps(batch) (dinov2_extractor.py:339-353; the 'attn' facet, :230-231): the class token's
 * attention over the patch tokens in blocks[layer] — softmax over all 1 + R + T keys (cls, registers, patches), patch columns
 * kept — averaged over the
 * heads head_idxs (host array; the reference uses [0, 2, 4, 5] and supports dino_vits8 only) and min-max normalised per
 * image (the reference's broadcast of the [B] extremes is only well-formed for a batch of one; every image gets its own):
 * saliency fp32 [n][T] in [0, 1].  The handle must have been created with layer = the block wanted (the reference hooks
 * block 11). */
VITVS_API int vitvs_extract_saliency_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, int32_t n_heads,
                               const int32_t* head_idxs, float* saliency, void* stream);
/* Residual stream after block `cfg.blocks - 1`, fp32 [n][1+R+T][D] (what the forward hook captures,
 * dinov2_extractor.py:198-199; every row: cls, the R register tokens, the patches), for parity tests. */
VITVS_API int vitvs_forward_tokens_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, float* tokens, void* stream);

/* find_correspondences_batch's similarity + argmax stage (vitvs_v2.py:78-81) on caller descriptors:
 * desc1 (desired), desc2 (current) fp32 [T][Dp], Dp a multiple of 32 -> nn_1, nn_2 int32 [T], sim_1 fp32 [T].
 * Optional S_out fp32 [T][T] receives the full similarity matrix (NULL to skip). */
VITVS_API int vitvs_correspond_dev(vitvs_handle* h, int32_t T, int32_t Dp, const float* desc1, const float* desc2,
                         int32_t* nn_1, int32_t* nn_2, float* sim_1, float* S_out, void* stream);

/* The control law on given nearest-neighbour tables (vitvs_v2.py:105-155 filter/selection, :511-553,
 * :566-586, :613-659): nn_1, nn_2 int32 [T], sim_1 fp32 [T] for ONE pair. */
VITVS_API int vitvs_servo_from_nn_dev(vitvs_handle* h, int32_t T, const int32_t* nn_1, const int32_t* nn_2, const float* sim_1,
                            const uint16_t* Z_mm, const double* K, int32_t select_mode, const int32_t* selection,
                            int32_t n_selected, int32_t num_pairs, double* v_c, int32_t* status, void* stream);

/* vitvs_servo_from_nn_dev with sub-patch offsets of the matches (option "subpatch", below): `offsets` fp32 [T][2] = (dr, dc) in
 * patch pitches for every token of the desired frame, moves the match of each selected token off its patch centre before the
 * pixel features are formed, whatever the handle's option says; NULL: exactly vitvs_servo_from_nn_dev.  Replaces nothing: the
 * reference's features are patch centres (vitvs_v2.py:511-513). */
VITVS_API int vitvs_servo_from_nn_ex_dev(vitvs_handle* h, int32_t T, const int32_t* nn_1, const int32_t* nn_2, const float* sim_1,
                            const uint16_t* Z_mm, const double* K, int32_t select_mode, const int32_t* selection,
                            int32_t n_selected, int32_t num_pairs, const float* offsets, double* v_c, int32_t* status, void* stream);
/* The sub-patch offsets themselves on caller descriptors (normalised inside, like vitvs_correspond_dev): desc1 (desired), desc2
 * (current) fp32 [T][Dp], Dp a multiple of 32, T a square; nn_1 int32 [T] -> offsets fp32 [T][2] = (dr, dc) of every token (0 for
 * a match outside 0 .. T - 1).  The arithmetic the law's kernel runs under the option, without a forward.  Replaces nothing. */
VITVS_API int vitvs_refine_dev(vitvs_handle* h, int32_t T, int32_t Dp, const float* desc1, const float* desc2, const int32_t* nn_1,
                            float* offsets, void* stream);

/* --- introspection of the last compute_velocity / servo call (device -> host copies, synchronising).
 * What detect_features() returns besides v_c (vitvs_v2.py:523) and what the parity tests check.
 *   nn_1, nn_2 int32 [n_pairs][T]; sim_1 fp32 [n_pairs][T]
 *   info int32 [n_pairs][8]: n_mutual, n_feature_rows, same_image, n_matched, svd_sweeps, L_rows, reweightings, zero_weights
 *        (svd_sweeps: -1 = LDL^T, else the Jacobi sweeps, of the FINAL solve; reweightings / zero_weights: option "robust_law"
 *        below, both 0 with the option off or when a status skipped the law)
 *   selected int32 [n_pairs][max_rows] token ids of the desired frame (-1 = zero-padded row)
 *   s_uv int32 [n_pairs][max_rows][4] = u*, v*, u, v ; feat double [n_pairs][max_rows][4] = Z, x, y, sim
 *        (feat[..][3] over the first n_matched rows is the reference's sim_selected_12, vitvs_v2.py:523, 1167-1174)
 *   L double [n_pairs][7][2*max_rows] column-major: 6 columns of L_e then e.
 * A call's law uses n_feature_rows = info[1] feature pairs (num_pairs, or every candidate for DENSE); rows of
 * `selected` / `s_uv` / `feat` from n_feature_rows on, and rows of `L` from 2 * n_feature_rows on, are returned as
 * -1 / 0 / 0 / 0 whatever an earlier, larger call left in the workspace.
 * Any pointer may be NULL.  After a host-pointer velocity call (vitvs_compute_velocity, vitvs_reselect) everything but
 * `selected` and `L` is served from host memory (the handle's pinned block) without a device call. */
VITVS_API int vitvs_last_details(vitvs_handle* h, int32_t n_pairs, int32_t* nn_1, int32_t* nn_2, float* sim_1, int32_t* info,
                       int32_t* selected, int32_t* s_uv, double* feat, double* L);
/* The weight every feature pair had in the FINAL solve of the last law evaluation (option "robust_law", below):
 *   w double [n_pairs][max_rows]; with the option off 1 for every live pair; 0 for zero-padded pairs (rows from n_matched on
 *   of a short selection) and from n_feature_rows on.  `L` and `e` of vitvs_last_details stay the unweighted ones.
 * Synchronising, always read from the device.  Replaces nothing: the reference's law has no weights (vitvs_v2.py:613-622). */
VITVS_API int vitvs_last_weights(vitvs_handle* h, int32_t n_pairs, double* w);
/* The sub-patch offsets (dr, dc), in patch pitches, every feature row's match had in the last law evaluation (option "subpatch",
 * below): offsets float [n_pairs][max_rows][2]; 0 for zero-padded rows, from n_feature_rows on, under the same-image shortcut
 * and with the option off.  With the option on, s_uv[..][2:4], feat (Z, x, y) and L of vitvs_last_details are those of the
 * moved matches.  Synchronising, always read from the device.  Replaces nothing (vitvs_v2.py:511-513: patch centres). */
VITVS_API int vitvs_last_offsets(vitvs_handle* h, int32_t n_pairs, float* offsets);
/* The visiting order the last law evaluation ran on when its select_mode was VITVS_SELECT_BEST: order int32 [n_pairs][T], a
 * permutation of 0 .. T-1 per pair (T of that call), the tokens of the desired frame sorted ascending by (class, rho, -sim_1, id):
 * class 0 for a mutual nearest neighbour (0 <= nn_1[i] < T and nn_2[nn_1[i]] == i) and 1 otherwise; rho the number of tokens of
 * the same class in the same image cell with a larger sim_1, or the same sim_1 and a smaller id; cell of token i on the g x g
 * grid = ((i / g) * c / g) * c + (i % g) * c / g in integer arithmetic, c = min(option "select_cells", g).  The law takes the
 * first num_pairs candidates met in it, exactly as for VITVS_SELECT_ORDER.  Synchronising, always read from the device.  Error -5
 * when the last law evaluation ran in another mode. */
VITVS_API int vitvs_last_order(vitvs_handle* h, int32_t n_pairs, int32_t* order);

/* --- the goal depth (option "interaction", below) ------------------------------------------------
 * Z_des_mm uint16 [n_goal][v_max][u_max], the depth image(s) taken at the goal pose, in the sensor's millimetres (device memory
 * for _dev, host memory for the other form, which may synchronise).  One launch reduces them to what the law reads: per goal
 * image the depth at every token's patch centre (the pixel of the goal feature s*, vitvs_v2.py:511-513, 544-549) and at pixel
 * (0, 0), the goal pixel of a zero-padded row; 0 or outside the image means 100 m, as for the current depth (:566-586).  The
 * table lives in the handle, allocated by the first call; later calls with the same n_goal rewrite it in place, in stream
 * order, and captured graphs stay valid; a call that changes n_goal (the first, a clear with n_goal = 0, another count) drains
 * the device and drops the handle's graphs.  A velocity call of n_pairs pairs reads image b for pair b when n_goal == n_pairs,
 * image 0 for every pair when n_goal == 1, and is error -5 otherwise.  Independent of vitvs_set_goal's token cache; no other
 * call drops it.  Replaces nothing: the reference evaluates L at the current features only (vitvs_v2.py:650-659).
 * Returns 0, -1 (null), -3 (n_goal outside 0 .. max_pairs). */
VITVS_API int vitvs_set_goal_depth_dev(vitvs_handle* h, int32_t n_goal, const uint16_t* Z_des_mm, void* stream);
VITVS_API int vitvs_set_goal_depth(vitvs_handle* h, int32_t n_goal, const uint16_t* Z_des_mm);
/* Z* of every feature row of the last law evaluation, in metres: z double [n_pairs][max_rows]; 0 from n_feature_rows on, and
 * everywhere with option "interaction" at 0.  Synchronising, always read from the device. */
VITVS_API int vitvs_last_goal_depth(vitvs_handle* h, int32_t n_pairs, double* z);

/* --- the rig law: one twist for a rigid multi-camera rig ------------------------------------------
 * A velocity call of N pairs whose current frames are the N cameras of one rigid rig leaves N camera twists; this evaluates the
 * ONE twist the rig should execute, the least-squares solution of the stacked problem (ViSP's cVe per feature set).  Camera i
 * has pose (R_i, t_i) in the rig frame, X_rig = R_i X_cam + t_i; a rig twist v_r = (v, w), expressed in the rig frame, moves
 * camera i with the twist, in its own optical frame,
 *     v_ci = W_i v_r,   W_i = [[R_i^T, -R_i^T [t_i]x], [0, R_i^T]]      (6 x 6)
 * and with L_i (rows x 6), e_i what camera i's law built — under whichever of "subpatch" / "interaction" is on, zero-padded
 * rows included, exactly as the camera's own law used them (L and e of vitvs_last_details) —
 *     M = stack_i(L_i W_i),  e = stack_i(e_i),  v_r = -lambda pinv(M) e
 * over the cameras whose status is VITVS_OK, in fp64: the 6 x 6 normal equations G = M^T M, g = M^T e by the LDL^T
 * factorisation of the camera law with its pivot test d > 1e-4 G_jj, and behind a failed pivot the one-sided Jacobi SVD of the
 * stacked M with numpy.linalg.pinv's rcond = 1e-15.  The average of the cameras' twists mapped back to the rig frame is NOT this
 * solution, and is wrong whenever one camera alone cannot observe all six degrees of freedom.
 *   cVr      double [n_cams][36], row-major W_i
 *   status   int32 [n_cams], the array the velocity call wrote: a camera whose status is not VITVS_OK contributes no rows
 *   v_rig    double [6]; 0 when no camera contributes
 *   rig_status  int32: VITVS_OK when a camera contributed, else the largest camera status
 *   rig_info int32 [8] or NULL: cameras used, total rows of M, Jacobi sweeps (-1: the LDL^T path), n_cams, the largest camera
 *            status, 0, 0, 0
 *   normal   double [28] or NULL: G's upper triangle row-major (21), g (6), the total rows as a double — what a rig spread over
 *            several GPUs sums across them (vit-vs_amd/dist.py rig_velocity)
 * All pointers are device memory (_dev; one launch on `stream`, asynchronous) or host memory (the other form: copy in, run,
 * wait, copy out).  Evaluated on what the handle's last law evaluation left on the device, with the handle's lambda: valid after
 * vitvs_compute_velocity[_dev] / vitvs_reselect with n_pairs == n_cams, in stream order behind it; it changes nothing that call
 * left (v_c, status, vitvs_last_*).  The result is bit-reproducible: the cameras' sums are added in camera order.
 * The stacked workspace lives in the handle, sized for max_pairs cameras and allocated by the first rig call, which therefore
 * synchronises and must not be made inside a stream capture; later calls may be captured and replayed.
 * With option "robust_law" on the call is error -5: a robust rig law needs ONE median over all cameras' residuals, which the
 * cameras' own re-weighted laws do not give; that law is vitvs_rig_robust_velocity[_dev] below.
 * Returns 0, -1 (a null required pointer), -5 (no law evaluation yet, n_cams is not its pair count, more than 256 cameras,
 * robust_law on).  Replaces nothing: the reference runs one controller per camera (vitvs_v2.py:702-819). */
VITVS_API int vitvs_rig_velocity_dev(vitvs_handle* h, int32_t n_cams, const double* cVr, const int32_t* status, double* v_rig,
                                     int32_t* rig_status, int32_t* rig_info, double* normal, void* stream);
VITVS_API int vitvs_rig_velocity(vitvs_handle* h, int32_t n_cams, const double* cVr, const int32_t* status, double* v_rig,
                                 int32_t* rig_status, int32_t* rig_info, double* normal);

/* --- the robust rig law: Tukey IRLS over the stacked rig system --------------------------------
 * The rig law above with the re-weighting of option "robust_law" applied to the STACK: one scale, from one median over the live
 * feature pairs of all contributing cameras.  (Re-weighting every camera by itself and stacking is not this law: a camera whose
 * own matches are mostly wrong has a median that sits among its outliers; the rig's median does not.)  In fp64, on the same
 * L_i, e_i, rows and statuses as vitvs_rig_velocity_dev (L_i and e_i are never scaled, also when "robust_law" ran), with
 * live_i = the camera's matched pairs (vitvs_last_details info[3]; its zero-padded pairs have weight 0 throughout).  A camera
 * contributes when its status is VITVS_OK and it has rows and a live pair.  M = stack_i(L_i W_i), e = stack_i(e_i); pair k of the
 * stack is its rows 2k, 2k + 1:
 *     w_k = 1 on live pairs;   n_iter times:  x = pinv(sqrt(W) M) sqrt(W) e,  rho_k = |e_k - M_k x|_2,
 *         sigma = max(1.4826 median(rho over ALL live pairs), sigma_min),  t = rho_k / (4.6851 sigma),  w_k = (1 - t^2)^2 or 0 (t >= 1);
 *     x once more;  v_rig = -lambda x
 * sigma_min = the largest, over the contributing cameras, of 0.5 max(pitch_u / fx_i, pitch_v / fy_i) ("robust_law"'s floor;
 * residuals are in normalised image coordinates and compare across cameras).  The median of an even count is the mean of the
 * two middle values.  Solves as the rig law's: LDL^T of the weighted normal equations (the weight as a factor, pivot test
 * d > 1e-4 G_jj), behind a failed pivot the Jacobi SVD (rcond 1e-15) of a copy of the rows scaled by sqrt(w).
 *   cVr, status, v_rig, rig_status   as vitvs_rig_velocity_dev's
 *   K        double [n_cams][4]: fx, fy, cx, cy of camera i
 *   n_iter   re-weightings, 1 .. 16
 *   rig_info int32 [8] or NULL: [0..4] as vitvs_rig_velocity_dev's (cameras used and total rows count contributing cameras),
 *            [5] the re-weightings done, [6] the pairs of contributing cameras whose final weight is 0, padded ones included, [7] 0
 *   normal   double [28] or NULL: the weighted G = M^T W M (21), g = M^T W e (6) of the last solve, the total rows
 *   weights  double [n_cams][max_rows] or NULL: the final weights; 0 on padded pairs, unused pairs and non-contributing cameras
 *   sigma    double [1] or NULL: the last scale; 0 when no re-weighting ran (no camera contributed)
 * One launch on `stream`; valid behind the same calls as vitvs_rig_velocity_dev, whether the last law was robust or not, and it
 * changes nothing that call left.  Bit-reproducible.  Workspace and capture rules as vitvs_rig_velocity_dev's (the two share
 * the handle's block).  The residuals and weights of the whole rig sit in LDS: n_cams * max_rows pairs beyond ~10,000 are -3.
 * Returns 0, -1 (a null required pointer), -2 (n_iter outside 1 .. 16), -3, -5 (no law evaluation yet, n_cams is not its pair
 * count, more than 256 cameras).  No counterpart in the reference. */
VITVS_API int vitvs_rig_robust_velocity_dev(vitvs_handle* h, int32_t n_cams, const double* cVr, const int32_t* status,
                                            const double* K, int32_t n_iter, double* v_rig, int32_t* rig_status, int32_t* rig_info,
                                            double* normal, double* weights, double* sigma, void* stream);
VITVS_API int vitvs_rig_robust_velocity(vitvs_handle* h, int32_t n_cams, const double* cVr, const int32_t* status, const double* K,
                                        int32_t n_iter, double* v_rig, int32_t* rig_status, int32_t* rig_info, double* normal,
                                        double* weights, double* sigma);

/* --- the pose law --------------------------------------------------------------------------------
 * A position-based law from what the camera's law left in the handle.  Every usable feature row k of pair b gives a
 * current 3-D point P_k = Z (x, y, 1) (feat) in the current camera's frame and a goal point Q_k = Z* (xs, ys, 1) in the goal
 * camera's (xs = (u* - cx) / fx, ys = (v* - cy) / fy from s_uv; Z* = the goal-depth table's entry of the row's goal token / 1000).
 * A row is usable when its token is selected (>= 0), its current depth is not a hole (Z < 100) and its table entry is not 0.
 * (R, t) minimises sum w |Q - (R P + t)|^2 — the pose of the current camera in the goal camera's frame, X_goal = R X_cam + t —
 * by Horn's closed form (weighted centroids, S = sum w (P - pc)(Q - qc)^T, the eigenvector of the largest eigenvalue of the
 * symmetric 4 x 4 N(S) as the unit quaternion with q_w >= 0), and
 *   v_pose = -lambda (R^T t, theta u)      theta u = 2 atan2(|q_v|, q_w) q_v / |q_v|
 * is ViSP's PBVS twist in the current camera's own optical frame, the convention of v_c.  n_iter > 0: Tukey IRLS as the robust
 * control law's (c = 4.6851), rho = |Q - (R P + t)|, sigma = max(1.4826 median(rho over usable rows), sigma_min), sigma_min =
 * 0.5 max(pitch_u / fx, pitch_v / fy) median(Z* over usable rows); one more solve after the last re-weighting.
 *   K, status    device double [n_pairs][4] and int32 [n_pairs]: the K and the status of the velocity call
 *   n_iter       re-weightings, 0 .. 16
 *   v_pose       double [n_pairs][6];  pose_status int32 [n_pairs]: the camera's status when that is not VITVS_OK (v_pose = 0);
 *                VITVS_OK with v_pose = 0, R = I under the same-image shortcut; VITVS_TOO_FEW (v_pose = 0, R = I) when fewer
 *                than 3 rows are usable or keep a weight > 0, or the clouds are degenerate: ev_1 - ev_2 <= 1e-8 (sum w |P - pc|^2
 *                + sum w |Q - qc|^2) (collinear points leave a rotation free); VITVS_OK otherwise
 *   pose         double [n_pairs][12] or NULL: R row-major, then t
 *   pose_info    int32 [n_pairs][8] or NULL: usable rows, Jacobi sweeps of the last solve, re-weightings done, usable rows with
 *                final weight 0, degenerate flag, rows dropped for a hole, 0, 0
 *   weights      double [n_pairs][max_rows] or NULL;  sigma double [n_pairs] or NULL: the last scale
 * One launch on `stream`; valid in stream order behind any law evaluation of the handle with n_pairs pairs, replayed graphs
 * included, and it changes nothing that call left.  Bit-reproducible.  Needs a goal depth that pairs with the call (n_goal ==
 * n_pairs or 1).  The first call allocates the workspace and synchronises the device: make it outside any stream capture.
 * Returns 0, -1 (a null required pointer), -2 (n_iter outside 0 .. 16), -3 (max_rows too large for the robust form's LDS),
 * -5 (no law evaluation yet, n_pairs is not its pair count, no goal depth or one that does not pair, a law evaluation with option
 * interaction at 1: its feature rows hold Z*, not Z).  No counterpart in the reference. */
VITVS_API int vitvs_pose_velocity_dev(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, int32_t n_iter,
                                      double* v_pose, int32_t* pose_status, double* pose, int32_t* pose_info, double* weights,
                                      double* sigma, void* stream);
/* The host-pointer form: every pointer is host memory; synchronous. */
VITVS_API int vitvs_pose_velocity(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, int32_t n_iter,
                                  double* v_pose, int32_t* pose_status, double* pose, int32_t* pose_info, double* weights,
                                  double* sigma);

/* The pose law with a consensus start ("The consensus start"): n_hyp three-point hypotheses, each the closed-form
 * rigid displacement of 3 usable rows drawn from `seed` (an integer hash of (seed, j, usable rows): the same frames give the same
 * twist), are scored in parallel with the truncated cost sum min(rho^2, T^2), T = 4.6851 sigma_min; the rows within T of the winner
 * start at weight 1 and the others at 0, and the law goes on from there as above (n_iter = 0: the alignment of the consensus set
 * alone, the setting for more than half of wrong matches).  When every hypothesis is degenerate the start is the one without
 * consensus.  pose_info[6] = the winner's j + 1 (0: no consensus start), pose_info[7] = the start weights at 1; pose_info[3]
 * counts the rows the consensus start left out as weights of 0.  n_hyp is 0 .. 4096; 0 is vitvs_pose_velocity_dev bit for bit.
 * Still one launch.  Returns as vitvs_pose_velocity_dev, and -2 also for n_hyp outside its range; -3 counts half a double per
 * feature row more of LDS (one and a half with n_iter = 0). */
VITVS_API int vitvs_pose_consensus_velocity_dev(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status,
                                                int32_t n_iter, int32_t n_hyp, uint32_t seed, double* v_pose, int32_t* pose_status,
                                                double* pose, int32_t* pose_info, double* weights, double* sigma, void* stream);
/* The host-pointer form: every pointer is host memory; synchronous. */
VITVS_API int vitvs_pose_consensus_velocity(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, int32_t n_iter,
                                            int32_t n_hyp, uint32_t seed, double* v_pose, int32_t* pose_status, double* pose,
                                            int32_t* pose_info, double* weights, double* sigma);

/* --- the homography law --------------------------------------------------------------------------
 * A law for a planar target that needs no depth at all (Benhimane and Malis, "Homography-based 2D visual servoing",
 * IJRR 2007).  Every feature row k < info[1] of pair b whose token is selected (>= 0) gives a current normalised image point
 * m_k = (x, y) (feat; the moved match under option subpatch) and a goal point m*_k = ((u* - cx) / fx, (v* - cy) / fy) (s_uv).  H, the
 * 3 x 3 homography with m* ~ H m, is the eigenvector of the smallest eigenvalue of the 9 x 9 DLT normal matrix of the Hartley-
 * normalised points (cyclic Jacobi in fp64), denormalised and scaled to det H = 1, and
 *   v_h = -lambda (depth_scale (H - I) m_c, (H21 - H12, H02 - H20, H10 - H01))      m_c = (sum w x / sum w, sum w y / sum w, 1)
 * is a twist in the current camera's own optical frame, the convention of v_c.  depth_scale (metres) is a rough guess of the
 * distance to the target: it scales the translational gain, not the fixed point.  n_iter > 0: Tukey IRLS (c = 4.6851) on the
 * transfer error rho = |pi(H m) - m*| (+inf when the third component of H m is <= 0), sigma = max(1.4826 median(rho over usable
 * rows), sigma_min), sigma_min = 0.5 max(pitch_u / fx, pitch_v / fy); one more solve after the last re-weighting.
 *   K, status    device double [n_pairs][4] and int32 [n_pairs]: the K and the status of the velocity call
 *   depth_scale  > 0 and finite;  n_iter  re-weightings, 0 .. 16
 *   v_h          double [n_pairs][6];  h_status int32 [n_pairs]: the camera's status with v_h = 0 when that is
 *                VITVS_NO_CORRESPONDENCE or VITVS_TOO_FEW (VITVS_NO_DEPTH does NOT stop this law: the camera's law writes its rows
 *                before it looks for a depth); VITVS_OK with v_h = 0, H = I under the same-image shortcut; VITVS_TOO_FEW (v_h = 0,
 *                H = I) when fewer than 4 rows are usable or keep a weight > 0, or the set is degenerate: a mean distance of 0, the
 *                second-smallest eigenvalue <= 1e-8 trace(M) (collinear points), or |det H| <= 1e-8 |H|_F^3; VITVS_OK otherwise
 *   H            double [n_pairs][9] or NULL: row-major
 *   h_info       int32 [n_pairs][8] or NULL: usable rows, Jacobi sweeps of the last solve, re-weightings done, usable rows with
 *                final weight 0, degenerate flag, rows with rho = +inf at the last re-weighting, 0, 0
 *   weights      double [n_pairs][max_rows] or NULL;  sigma double [n_pairs] or NULL: the last scale
 * One launch on `stream`; valid in stream order behind any law evaluation of the handle with n_pairs pairs under every value of
 * option interaction, replayed graphs included, and it changes nothing that call left.  Bit-reproducible.  The first call
 * allocates the workspace and synchronises the device: make it outside any stream capture.
 * Returns 0, -1 (a null required pointer), -2 (n_iter outside 0 .. 16, depth_scale <= 0 or not finite), -3 (max_rows too large
 * for the robust form's LDS), -5 (no law evaluation yet, or n_pairs is not its pair count).  No counterpart in the reference. */
VITVS_API int vitvs_homography_velocity_dev(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status,
                                            double depth_scale, int32_t n_iter, double* v_h, int32_t* h_status, double* H,
                                            int32_t* h_info, double* weights, double* sigma, void* stream);
/* The host-pointer form: every pointer is host memory; synchronous. */
VITVS_API int vitvs_homography_velocity(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, double depth_scale,
                                        int32_t n_iter, double* v_h, int32_t* h_status, double* H, int32_t* h_info, double* weights,
                                        double* sigma);

/* The homography law with a consensus start ("The consensus start"): n_hyp four-point hypotheses, each a closed-form
 * homography of 4 usable rows drawn from `seed` (an integer hash of (seed, j, usable rows): the same frames give the same twist),
 * are scored in parallel with the truncated cost sum min(rho^2, T^2), T = 4.6851 sigma_min; the rows within T of the winner start
 * at weight 1 and the others at 0, and the law goes on from there as above (n_iter = 0: the DLT over the consensus set).  When
 * every hypothesis is degenerate the start is the one without consensus.  h_info[6] = the winner's j + 1 (0: no consensus start),
 * h_info[7] = the start weights at 1; h_info[3] counts the rows the consensus start left out as weights of 0.  n_hyp is 0 .. 4096;
 * 0 is vitvs_homography_velocity_dev bit for bit.  Still one launch.  Returns as vitvs_homography_velocity_dev, and -2 also for
 * n_hyp outside its range; -3 counts half a double per feature row more of LDS. */
VITVS_API int vitvs_homography_consensus_velocity_dev(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status,
                                                      double depth_scale, int32_t n_iter, int32_t n_hyp, uint32_t seed, double* v_h,
                                                      int32_t* h_status, double* H, int32_t* h_info, double* weights, double* sigma,
                                                      void* stream);
/* The host-pointer form: every pointer is host memory; synchronous. */
VITVS_API int vitvs_homography_consensus_velocity(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status,
                                                  double depth_scale, int32_t n_iter, int32_t n_hyp, uint32_t seed, double* v_h,
                                                  int32_t* h_status, double* H, int32_t* h_info, double* weights, double* sigma);

/* --- the pose rig law ----------------------------------------------------------------------------
 * ONE rigid 3-D alignment over the matched points of ALL cameras of a rigid rig, for a rig whose cameras were the
 * pairs of the last law evaluation.  Camera i has pose (R_i, t_i) in the rig frame, X_rig = R_i X_cam + t_i (the (R, t) of
 * vitvs_rig_velocity_dev's cVr).  A camera contributes when its status is VITVS_OK and it is not under the same-image shortcut;
 * its usable rows (the pose law's rule) give P_k, Q_k as the pose law's, and the stack holds P'_k = R_i P_k + t_i and Q'_k =
 * R_i Q_k + t_i at stack row i * max_rows + k.  (R, t) minimises sum w |Q' - (R P' + t)|^2 over the whole stack by the pose law's
 * solve (same sums, Jacobi, degeneracy rule): the current rig in the goal rig's frame, and
 *   v_rig = -lambda (R^T t, theta u)
 * is a twist in the rig's own frame, the convention of vitvs_rig_velocity_dev's v_rig.  n_iter > 0: Tukey IRLS with ONE median
 * over the usable rows of all contributing cameras, sigma = max(1.4826 median(rho), sigma_min), sigma_min = 0.5 max_i max(pitch_u
 * / fx_i, pitch_v / fy_i) median(Z* over all usable rows), Z* in the camera's frame, i over the contributing cameras.
 *   rTc          device double [n_cams][12]: R_i row-major, then t_i
 *   K, status    device double [n_cams][4] and int32 [n_cams]: the K and the status of the velocity call
 *   n_iter       re-weightings, 0 .. 16
 *   v_rig        double [6];  rig_status int32 [1]: VITVS_OK; VITVS_TOO_FEW (v_rig = 0, R = I) when fewer than 3 rows of the stack
 *                are usable or keep a weight > 0, or the stack is degenerate; when no camera contributes v_rig = 0, R = I and
 *                the status is the largest camera status (VITVS_OK when every camera is at its goal by the shortcut)
 *   pose         double [12] or NULL: R row-major, then t
 *   rig_info     int32 [8] or NULL: contributing cameras, usable rows, Jacobi sweeps of the last solve, re-weightings done,
 *                usable rows with final weight 0, degenerate flag, rows dropped for a hole, the largest camera status
 *   moments      double [18] or NULL, for a rig spread over ranks: the raw sums of the final weights over the stack: sum w,
 *                sum w P' [3], sum w Q' [3], sum w P' Q'^T [9] row-major, sum w |P'|^2, sum w |Q'|^2 (zeros when nobody contributes)
 *   weights      double [n_cams][max_rows] or NULL;  sigma double [1] or NULL: the last scale
 * One launch of one workgroup on `stream`; valid exactly where vitvs_pose_velocity_dev is, with n_cams the pair count of the law
 * evaluation, and it changes nothing that call left.  Bit-reproducible.  The first call allocates the workspace and synchronises
 * the device: make it outside any stream capture.  Returns 0, -1 (a null required pointer), -2 (n_iter outside 0 .. 16, n_cams
 * < 1), -3 (n_cams * max_rows too large for the robust form's LDS), -5 (vitvs_pose_velocity_dev's cases).  No counterpart in the
 * reference. */
VITVS_API int vitvs_pose_rig_velocity_dev(vitvs_handle* h, int32_t n_cams, const double* rTc, const double* K, const int32_t* status,
                                          int32_t n_iter, double* v_rig, int32_t* rig_status, double* pose, int32_t* rig_info,
                                          double* moments, double* weights, double* sigma, void* stream);
/* The host-pointer form: every pointer is host memory; synchronous. */
VITVS_API int vitvs_pose_rig_velocity(vitvs_handle* h, int32_t n_cams, const double* rTc, const double* K, const int32_t* status,
                                      int32_t n_iter, double* v_rig, int32_t* rig_status, double* pose, int32_t* rig_info,
                                      double* moments, double* weights, double* sigma);

/* --- the roll search -----------------------------------------------------------------------------
 * ViT tokens are not rotation invariant: past ~45 degrees of in-plane rotation between the current frame and the goal the matches
 * degrade.  The reference turns the robot to four poses and scores the views (find_and_set_best_pose, vitvs_v2.py:1151-1189).
 * The search needs no motion: a quarter turn of a square frame is lossless and a quarter turn of its token grid is a permutation
 * of token ids.
 *
 * vitvs_quarter_turns_dev: out [n_frames][4][S][S][3] <- frames [n_frames][S][S][3] uint8, S = img_size, copy k =
 * numpy.rot90(frame, k) (k = 1: out[r][c] = in[c][S-1-r]).  One launch on `stream`; independent of vitvs_set_frame_size.
 * Returns 0, -1 (null), -5 (n_frames < 1). */
VITVS_API int vitvs_quarter_turns_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, uint8_t* out, void* stream);
/* vitvs_roll_velocity_dev: ONE frame pair, from any in-plane rotation.  The current frame's four quarter-turned copies are matched
 * against the goal exactly as a des_shared call of four pairs matches them (I_des NULL: a cached goal of ONE image); candidate k's
 * score is the fp64 mean of sim_1 over its mutual nearest neighbours, a candidate is valid when 0 < n_mutual < T or under the
 * same-image shortcut, the winner k* is the largest score (the smallest k on an exact tie; -1 without a valid candidate).  With P =
 * numpy.rot90(arange(T).reshape(g, g), k*).reshape(-1) the winner's tables are carried back into the unturned frame, nn_1'[i] =
 * P[nn_1[i]], nn_2'[P[j]] = nn_2[j], sim_1' = sim_1, and the law runs on them for one pair with the caller's depth image, K and
 * selection (arguments as vitvs_compute_velocity_dev's for n_pairs = 1).  When the winner is a turned copy under the same-image
 * shortcut (the camera sits a quarter turn from the goal), a feature row's current-side token is nn_1'[i] instead of i and info[2]
 * is 0: the twist turns the camera, and the follow-on laws do not take their at-goal early out.
 *   roll_info    device int32 [8]: k*, the four n_mutual, the same-image flag of k*, 0, 0
 *   scores       device double [4]: NaN for a candidate that is not valid
 * Afterwards the handle's last law evaluation is a one-pair one: vitvs_last_details(1) returns the carried-back tables, and the
 * pose and homography laws with n_pairs = 1 are valid behind it; "robust_law", "interaction" and every select_mode compose.
 * With k* = -1 pair 0 keeps candidate 0's keys and the law reports VITVS_NO_CORRESPONDENCE by itself.  Option "graph_replay"
 * does not replay this call.  The first call allocates the turned copies' buffer and synchronises the device: make it outside
 * any stream capture.  Returns 0, -1 (null), -3 (max_pairs < 4), -4, -5 (option "subpatch" on; a frame size other than S x S set
 * with vitvs_set_frame_size; a token grid that is not symmetric under the turn, (S - patch) % stride != 0; I_des NULL without a
 * cached goal of one image; a bad selection).  No counterpart in the reference. */
VITVS_API int vitvs_roll_velocity_dev(vitvs_handle* h, const uint8_t* I_cur, const uint8_t* I_des, const uint16_t* Z_mm,
                                      const double* K, int32_t select_mode, const int32_t* selection, const int32_t* n_selected,
                                      int32_t num_pairs, double* v_c, int32_t* status, int32_t* roll_info, double* scores,
                                      void* stream);
/* The host-pointer form: every pointer is host memory; synchronous; ordered behind the handle's pending _dev work. */
VITVS_API int vitvs_roll_velocity(vitvs_handle* h, const uint8_t* I_cur, const uint8_t* I_des, const uint16_t* Z_mm, const double* K,
                                  int32_t select_mode, const int32_t* selection, const int32_t* n_selected, int32_t num_pairs,
                                  double* v_c, int32_t* status, int32_t* roll_info, double* scores);

/* --- the photometric law: a dense final approach (photometric.hip) -----------------------------
 * Direct visual servoing on the luminance of every pixel (Collewet & Marchand; ViSP's vpFeatureLuminance), DESIGN.md 5k: the
 * law to hand over to once a ViT law stands in its dead zone of one patch pitch.  It reads frames, never tokens: no forward, no
 * weights, no preceding velocity call; it uses workspaces of its own and leaves everything the velocity path, vitvs_last_details,
 * vitvs_reselect and the other follow-on laws read and write alone.  Its convergence domain is small: outside it the twist is wrong,
 * not zero.
 *   I_cur, I_des  uint8 [n_pairs][height][width][3] interleaved RGB, height and width 1 .. 4096
 *   Z_mm          uint16 [n_pairs][height][width] millimetres, 0 = hole, or NULL.  It is the depth of the image the gradients are
 *                 taken of: the current depth for interaction 0, the goal depth for 1
 *   depth_scale   metres: the depth of every pixel when Z_mm is NULL (RGB only); then <= 0 gives VITVS_NO_DEPTH
 *   K             double [n_pairs][4] fx, fy, cx, cy at height x width
 *   level         0 .. 3, s = 2^level: Y = 77 R + 150 G + 29 B is summed over s x s blocks (h = height / s, w = width / s rounded
 *                 down, the tail ignored), I = Ysum / (256 s^2); the pooled image is at least 3 x 3
 *   interaction   0: gradients of I_cur; 1: of I_des
 * Per pooled pixel (r, c) inside the one-pixel border whose depth block holds a non-zero sample (Z = their mean / 1000), with
 * gx = (G(r, c+1) - G(r, c-1)) / 2, gy likewise, fx' = fx / s, cx' = (cx + 0.5) / s - 0.5, x = (c - cx') / fx', a = gx fx' (y, b
 * likewise): L = [a/Z, b/Z, -(x a + y b)/Z, -(x y a + (1 + y^2) b), (1 + x^2) a + x y b, x b - y a], e = I_cur - I_des, and
 * v_p = -lambda (H + mu diag(H))^-1 g of H = sum L^T L, g = sum L^T e (mu = 0: Gauss-Newton), by LDL^T.
 *   v_p        double [n_pairs][6];  p_status int32 [n_pairs]: VITVS_OK; VITVS_TOO_FEW (v_p = 0) with fewer than 6 rows or a failed
 *              pivot (a textureless frame, every depth a hole); VITVS_NO_DEPTH (v_p = 0).  Identical frames: VITVS_OK, v_p = 0
 *   normal     double [n_pairs][28] or NULL: H (upper triangle, row-major, 21), g (6), sum e^2
 *   p_info     int32 [n_pairs][8] or NULL: rows, pooled h, pooled w, bands of the launch, holes left out, a pivot failed, 0, 0
 * The sums are the same bits from call to call, and for a pair alone or at any place of a batch.  Two launches on `stream`; the
 * handle's first call allocates the law's blocks (1 MiB of band partials per pair of max_pairs, and the host form's staging) and
 * synchronises the device: make it outside any stream capture.  Calls on different streams of one handle share the partials: one
 * call in flight per handle, as for the other laws.  Returns 0, -1 (null), -2 (n_pairs outside 1 .. max_pairs, level, interaction, mu < 0, a scalar that
 * is not finite, height or width outside 1 .. 4096, a pooled side < 3; the host-pointer form: height x width > v_max x u_max).  No
 * counterpart in the reference. */
VITVS_API int vitvs_photometric_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                                             int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K,
                                             int32_t level, int32_t interaction, double mu, double lambda, double* v_p,
                                             int32_t* p_status, double* normal, int32_t* p_info, void* stream);
/* The host-pointer form: every pointer is host memory; synchronous; ordered behind the handle's pending _dev work. */
VITVS_API int vitvs_photometric_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                         int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                                         int32_t interaction, double mu, double lambda, double* v_p, int32_t* p_status,
                                         double* normal, int32_t* p_info);
/* --- the robust photometric law: lighting gain / bias and Tukey weights (photometric.hip) ------
 * The photometric law above under a change of exposure and with objects entering the view, DESIGN.md 5l.  Every argument of
 * vitvs_photometric_velocity_dev means what it means there; D is the pooled goal luminance I_des at a row's pixel.
 *   illumination       0 / 1: the model I_cur ~ (1 + gamma) I_des + beta along the motion; (gamma, beta) are eliminated from the
 *                      normal equations by a 2 x 2 LDL^T under the 6 x 6 one's pivot rule (a failed pivot: VITVS_TOO_FEW)
 *   robust_iterations  N = 0 .. 4 re-weightings: N + 1 weighted solves x = -(H' + mu diag H')^-1 g', between two of them
 *                      rho = |e + L x - gamma D - beta| per row, its median from a histogram of 4096 bins of 1/16 grey level
 *                      (the first bin whose cumulative count reaches ceil(n / 2), its centre), sigma = max(1.4826 median,
 *                      sigma_min), t = rho / (4.6851 sigma), w = (1 - t^2)^2 below t = 1, else 0
 *   sigma_min          > 0, grey levels
 *   v_p        lambda x of the last solve; p_status as the plain law's, VITVS_TOO_FEW (v_p = 0, p_robust = 0) also when fewer than
 *              6 rows keep a weight or any pivot of any pass fails
 *   p_robust   double [n_pairs][4]: gamma, beta, the last sigma (0 with N = 0), the final sum of the weights
 *   normal45   double [n_pairs][45] or NULL, the last pass's weighted sums: A = sum w L^T L (21, upper triangle, row-major),
 *              b = sum w L^T e (6), c = sum w e^2, B = sum w L^T [D, 1] (12, row-major), C = sum w [D,1]^T [D,1] (DD, D, sum w),
 *              d = sum w [D,1]^T e (2)
 *   p_info     int32 [n_pairs][8] or NULL: the plain law's six, then the rows of final weight 0 and the re-weightings run
 * With illumination 0 and N = 0, v_p, p_status, p_info[0 .. 6) and normal45[0 .. 28) are the plain law's bit for bit.  The same
 * bits from call to call and for a pair alone or at any place of a batch (integer atomics only).  3 N + 2 launches on `stream`,
 * no host round trip, capturable; the handle's first call allocates the law's own blocks (1.5 MiB of band partials, a 16 KiB
 * histogram and a state per pair of max_pairs, and the host form's staging) and synchronises the device: make it outside any
 * stream capture.  It shares nothing with the plain law, the velocity path or the other follow-on laws; one call in flight per
 * handle.  Returns 0, -1 (null), -2 (what the plain law refuses; illumination outside 0 / 1; robust_iterations outside 0 .. 4;
 * sigma_min not finite or <= 0).  No counterpart in the reference. */
VITVS_API int vitvs_photometric_robust_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                                                    int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale,
                                                    const double* K, int32_t level, int32_t interaction, double mu, double lambda,
                                                    int32_t illumination, int32_t robust_iterations, double sigma_min, double* v_p,
                                                    int32_t* p_status, double* p_robust, double* normal45, int32_t* p_info,
                                                    void* stream);
/* The host-pointer form: every pointer is host memory; synchronous; ordered behind the handle's pending _dev work. */
VITVS_API int vitvs_photometric_robust_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                                                int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale,
                                                const double* K, int32_t level, int32_t interaction, double mu, double lambda,
                                                int32_t illumination, int32_t robust_iterations, double sigma_min, double* v_p,
                                                int32_t* p_status, double* p_robust, double* normal45, int32_t* p_info);
/* --- the photometric rig law: one dense final approach for a rigid multi-camera rig (photometric.hip) ------
 * The robust photometric law above for n_cams cameras of one rigid rig, DESIGN.md 5m: ONE twist of the rig from every camera's
 * rows, every camera with a lighting model of its own, and ONE median over all cameras' residuals.  Per camera the arguments of
 * vitvs_photometric_robust_velocity_dev, a camera in the place of a pair: I_cur, I_des uint8 [n_cams][height][width][3], Z_mm uint16
 * [n_cams][height][width] or NULL with depth_scale, K double [n_cams][4].
 *   cVr        double [n_cams][6][6]: W_i, the twist transform from the rig frame to camera i (v_cam_i = W_i v_rig)
 *   live       int32 [n_cams] or NULL (all live): a camera at 0 leaves no trace in any sum, count or median
 * One solve: per live camera the 45 weighted sums over its own rows; with illumination its own (gamma_i, beta_i) eliminated by the
 * 2 x 2 LDL^T (H'_i, g'_i; without: A_i, b_i); T_i = W_i^T (H'_i W_i) and W_i^T g'_i, every inner sum in ascending index;
 * H_r = sum T_i, g_r = sum W_i^T g'_i, c_r = sum c_i over the cameras in ascending order; x = -(H_r + mu diag H_r)^-1 g_r by LDL^T;
 * x_i = W_i x, (gamma_i, beta_i) = C_i^-1 (d_i + B_i^T x_i).  One re-weighting: rho = |e + L_i x_i - gamma_i D - beta_i| of every row
 * of every live camera into one histogram (the robust law's bins), the median at ceil(n_total / 2), one sigma, Tukey weights.
 *   v_rig      double [6]: lambda x of the last solve, in the rig frame
 *   rig_status int32 [1]: VITVS_OK; VITVS_TOO_FEW (v_rig = 0, p_robust = 0) when the live cameras have fewer than 6 rows between
 *              them, fewer than 6 rows keep a weight, a live camera's 2 x 2 pivot fails or the 6 x 6 factorisation fails;
 *              VITVS_NO_DEPTH as the plain law.  A live camera without a row (all holes) adds nothing and fails nothing.
 *   p_robust   double [n_cams][4]: gamma_i, beta_i, the last sigma (the stack's; 0 with N = 0), the camera's final sum of weights;
 *              0 for a camera that is not live or has no row
 *   normal45   double [n_cams][45] or NULL: each camera's own sums of the last pass, as the robust law's (0 for a dead camera)
 *   rig_normal double [28] or NULL: H_r (21, upper triangle, row-major), g_r (6), c_r of the last pass: what a form across ranks
 *              would add up
 *   rig_info   int32 [8] or NULL: live cameras, n_total, rows of final weight 0, re-weightings run, holes, a pivot failed, the
 *              pooled h and w
 * With n_cams = 1 and cVr = I, v_rig, p_robust, rig_status and normal45 are vitvs_photometric_robust_velocity_dev's bit for bit.
 * Each camera's 45 sums do not depend on its place among the cameras; v_rig depends on the cameras' order only through the order
 * of the sum over them.  The same bits from call to call (integer atomics only).  4 N + 2 launches on `stream`, no host round
 * trip, capturable.  The call runs in the robust photometric law's blocks (allocated by the handle's first call of either, which
 * synchronises the device: make it outside any stream capture), so one photometric call of either kind is in flight per handle;
 * the host form's staging is its own.  Returns 0, -1 (null, cVr too), -2 (what the robust law refuses, n_cams in the place of
 * n_pairs; n_cams above 16).  No counterpart in the reference. */
VITVS_API int vitvs_photometric_rig_velocity_dev(vitvs_handle* h, int32_t n_cams, const uint8_t* I_cur, const uint8_t* I_des,
                                                 int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale,
                                                 const double* K, const double* cVr, const int32_t* live, int32_t level,
                                                 int32_t interaction, double mu, double lambda, int32_t illumination,
                                                 int32_t robust_iterations, double sigma_min, double* v_rig, int32_t* rig_status,
                                                 double* p_robust, double* normal45, double* rig_normal, int32_t* rig_info,
                                                 void* stream);
/* The host-pointer form: every pointer is host memory; synchronous; ordered behind the handle's pending _dev work. */
VITVS_API int vitvs_photometric_rig_velocity(vitvs_handle* h, int32_t n_cams, const uint8_t* I_cur, const uint8_t* I_des,
                                             int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale,
                                             const double* K, const double* cVr, const int32_t* live, int32_t level,
                                             int32_t interaction, double mu, double lambda, int32_t illumination,
                                             int32_t robust_iterations, double sigma_min, double* v_rig, int32_t* rig_status,
                                             double* p_robust, double* normal45, double* rig_normal, int32_t* rig_info);
/* --- the tile photometric law: a local lighting model, one gain / bias per tile (photometric.hip) ------
 * The robust photometric law above with the lighting model LOCAL, DESIGN.md 5n: a cast shadow, a lamp on half the target or a
 * regional exposure change breaks the one-gain model and is read as motion.  Every argument of vitvs_photometric_robust_velocity_dev
 * means what it means there; the lighting model is always on, so there is no `illumination`.
 *   tiles_y, tiles_x   gy, gx = 1 .. 8 each, at most the pooled image's sides; T = gy gx.  The row at pooled pixel (r, c) belongs to
 *                      tile k = floor(r gy / h) gx + floor(c gx / w) (the one-pixel border counts in the indexing, it has no row)
 * One solve: per tile the 45 weighted sums over its rows, C_k = l d l^T under the pivot rule.  A tile whose factor fails (flat,
 * empty, every weight 0) is DEAD in this pass: it adds nothing, gamma_k = beta_k = 0, and its rows stay in the next re-weighting with
 * those zeros.  The live tiles add, from zero and in ascending k, H' += A_k - B_k C_k^-1 B_k^T and g' += b_k - B_k C_k^-1 d_k;
 * x = -(H' + mu diag H')^-1 g' by LDL^T; (gamma_k, beta_k) = C_k^-1 (d_k + B_k^T x).  One re-weighting: rho = |e + L x - gamma_k D -
 * beta_k| with the row's own tile's pair, ONE histogram, median and sigma over all rows of the pair, Tukey's weights.
 *   v_p        lambda x of the last solve; VITVS_TOO_FEW (every output 0) with fewer than 6 rows, fewer than 6 rows that keep a
 *              weight, no live tile, or a failed 6 x 6 pivot in any pass; VITVS_NO_DEPTH as the plain law
 *   p_robust   double [n_pairs][4]: live tiles, dead tiles, the last sigma (0 with N = 0), the live tiles' final sum of weights
 *   p_tiles    double [n_pairs][T][4]: gamma_k, beta_k, the tile's final sum of weights, live (1.0 / 0.0)
 *   normal45   double [n_pairs][T][45] or NULL: every tile's sums of the last pass, laid out as the robust law's
 *   p_info     int32 [n_pairs][8] or NULL: the robust law's
 * A smooth lighting field (a ramp, a spot) is NOT what a piecewise-constant model fits: the tiles only slow that failure
 * (DESIGN.md 5n has the numbers).  The same bits from call to call and for a pair alone or at any place of a batch (integer
 * atomics only).  3 N + 2 launches on `stream`, no host round trip, capturable; the handle's first call allocates the law's own
 * blocks (12 MiB of segment partials, a 16 KiB histogram and a state per pair of max_pairs, and the host form's staging) and
 * synchronises the device: make it outside any stream capture.  It shares nothing with the other laws or the velocity path; one
 * call in flight per handle.  Returns 0, -1 (null), -2 (what the robust law refuses; tiles_y or tiles_x outside 1 .. 8 or above
 * the pooled side).  No counterpart in the reference. */
VITVS_API int vitvs_photometric_tile_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                                                  int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale,
                                                  const double* K, int32_t level, int32_t interaction, double mu, double lambda,
                                                  int32_t tiles_y, int32_t tiles_x, int32_t robust_iterations, double sigma_min,
                                                  double* v_p, int32_t* p_status, double* p_robust, double* p_tiles, double* normal45,
                                                  int32_t* p_info, void* stream);
/* The host-pointer form: every pointer is host memory; synchronous; ordered behind the handle's pending _dev work. */
VITVS_API int vitvs_photometric_tile_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                                              int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale,
                                              const double* K, int32_t level, int32_t interaction, double mu, double lambda,
                                              int32_t tiles_y, int32_t tiles_x, int32_t robust_iterations, double sigma_min,
                                              double* v_p, int32_t* p_status, double* p_robust, double* p_tiles, double* normal45,
                                              int32_t* p_info);
/* --- the surface photometric law: a smooth lighting model, a bilinear spline of gains and biases (photometric.hip) ------
 * The tile law's sibling, DESIGN.md 5o: a lamp beside the target, vignetting that changes with exposure or a window at one side of
 * the room are SMOOTH lighting fields, which a gain and a bias per tile do not fit.  Every argument of
 * vitvs_photometric_tile_velocity_dev means what it means there; the grid is the tile law's.
 *   cells_y, cells_x   gy, gx = 1 .. 8 each, at most the pooled image's sides.  (gy + 1)(gx + 1) nodes, node a = i (gx + 1) + j;
 *                      unknown 2 a is gamma_a and 2 a + 1 is beta_a, M = 2 (gy + 1)(gx + 1) <= 162.  The row at pooled pixel (r, c)
 *                      lies in cell (i, j) = (floor(r gy / h), floor(c gx / w)), v = (r gy - i h) / h, u = (c gx - j w) / w,
 *                      phi = [(1-v)(1-u), (1-v) u, v (1-u), v u] for the nodes (i, j), (i, j+1), (i+1, j), (i+1, j+1), and
 *                      I_cur ~ (1 + sum phi_a gamma_a) I_des + sum phi_a beta_a
 * One solve: per cell 120 weighted sums over its rows (below); the cells add from zero and in ascending index into the node system
 * C_g (M x M, half-bandwidth 2 gx + 5), B_g (6 x M), d_g and A, b, c.  C_g = L D L^T in ascending index under the pivot rule:
 * unknown j is live iff C_jj > 0 and d_j > 1e-4 C_jj, else DEAD in this pass: its row and column are left out, its value is 0, and
 * its rows stay in every sum and in the next re-weighting with that zero.  H' = A - B_g C_g^-1 B_g^T, g' = b - B_g C_g^-1 d_g,
 * x = -(H' + mu diag H')^-1 g' by LDL^T, the node values q = C_g^-1 (d_g + B_g^T x).  One re-weighting: rho = |e + L x -
 * gamma(r,c) D - beta(r,c)| with the phi-sums of the pixel's four nodes, ONE histogram, median and sigma over all rows, Tukey's weights.
 *   v_p        lambda x of the last solve; VITVS_TOO_FEW (every output 0) with fewer than 6 rows, fewer than 6 rows that keep a
 *              weight, every unknown dead, or a failed 6 x 6 pivot in any pass; VITVS_NO_DEPTH as the plain law
 *   p_robust   double [n_pairs][4]: live unknowns, dead unknowns, the last sigma (0 with N = 0), the final sum of weights
 *   p_nodes    double [n_pairs][(gy + 1)(gx + 1)][4]: gamma_a, beta_a, gamma_a live (1.0 / 0.0), beta_a live
 *   cell_sums  double [n_pairs][gy gx][120] or NULL: every cell's sums of the last pass, with wv = w [L, e] and wm = w m,
 *              m = [D phi0, phi0, D phi1, phi1, D phi2, phi2, D phi3, phi3]: A = sum wv_i L_j (21, upper triangle, row-major),
 *              b = sum wv_i e (6), c = sum wv_e e, B = sum wv_i m_k (6 x 8, row-major), C = sum wm_k m_l (36, upper triangle,
 *              row-major), d = sum wm_k e (8)
 *   p_info     int32 [n_pairs][8] or NULL: the robust law's
 * An EDGE in the lighting (a cast shadow) is what the tile law is for and this one is not (DESIGN.md 5o has the numbers).  The same
 * bits from call to call and for a pair alone or at any place of a batch (integer atomics only).  3 N + 2 launches on `stream`, no
 * host round trip, capturable; the handle's first call allocates the law's own blocks (32 MiB of segment partials = 4096 segment
 * rows x 8 cell columns x 128 doubles, a 16 KiB histogram and a state per pair of max_pairs, and the host form's staging) and
 * synchronises the device: make it outside any stream capture.  It shares nothing with the other laws or the velocity path; one
 * call in flight per handle.  Returns 0, -1 (null), -2 (what the robust law refuses; cells_y or cells_x outside 1 .. 8 or above
 * the pooled side).  No counterpart in the reference. */
VITVS_API int vitvs_photometric_surface_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                                                     int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale,
                                                     const double* K, int32_t level, int32_t interaction, double mu, double lambda,
                                                     int32_t cells_y, int32_t cells_x, int32_t robust_iterations, double sigma_min,
                                                     double* v_p, int32_t* p_status, double* p_robust, double* p_nodes,
                                                     double* cell_sums, int32_t* p_info, void* stream);
/* The host-pointer form: every pointer is host memory; synchronous; ordered behind the handle's pending _dev work. */
VITVS_API int vitvs_photometric_surface_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                                                 int32_t height, int32_t width, const uint16_t* Z_mm, double depth_scale,
                                                 const double* K, int32_t level, int32_t interaction, double mu, double lambda,
                                                 int32_t cells_y, int32_t cells_x, int32_t robust_iterations, double sigma_min,
                                                 double* v_p, int32_t* p_status, double* p_robust, double* p_nodes, double* cell_sums,
                                                 int32_t* p_info);
/* The launch plan of the photometric law as host arithmetic, for one pair (no handle, no device).  It is declared here, beside the
 * calls it plans, and not among the operator hooks of include/vitvs_ops.h: out int32 [8] = the
 * pooled h = height >> level and w = width >> level, the pooled rows per band max(1, min((2048 >> level) / w, h / 256)), the bands
 * ceil(h / rows) (the grid is bands x n_pairs workgroups of 256 threads), the dynamic LDS bytes 1024 + 4 ((rows + 2) 2 w + rows w),
 * the workspace bytes per pair 256 bands, 1 when the LDS needs the opt-in past 64 KiB, 0.  Returns 0, -1 (out NULL), -2 (height
 * or width outside 1 .. 4096, level outside 0 .. 3, a pooled side < 3; out is zeros). */
VITVS_API int vitvs_op_photometric_plan(int32_t height, int32_t width, int32_t level, int32_t* out);
/* The tile law's plan, likewise: out int32 [8] = the pooled h and w, the rows per band and the bands (the plain law's), the slots
 * per band, the dynamic LDS bytes of the rows launch 1536 + 4 ((rows + 2) 2 w + rows w) and of the residual launch (16384 more),
 * the workspace doubles per pair bands x slots x tiles_x x 48.  A band of more than one row (pooled h >= 512) may lie across ONE
 * tile-row boundary, since rows <= h / 256 and a tile row has at least floor(h / 8) rows: such a plan has 2 slots, slot s of a band
 * for tile row floor(band rows tiles_y / h) + s; a plan of one-row bands has 1.  The partial of (band, slot, tile column) is 48
 * doubles at ((band slots + slot) tiles_x + tile column) 48; wave v of a band's workgroup takes the (slot, tile column) segments
 * v, v + 4, .. in slot-major order and its lanes stride over the segment's pixels row-major.  Returns 0, -1 (out NULL), -2 (what
 * vitvs_op_photometric_plan refuses; tiles_y or tiles_x outside 1 .. 8 or above the pooled side; out is zeros). */
VITVS_API int vitvs_op_photometric_tile_plan(int32_t height, int32_t width, int32_t level, int32_t tiles_y, int32_t tiles_x,
                                             int32_t* out);
/* The surface law's plan, likewise: the tile plan's out [0 .. 7) with cells in the place of tiles (the bands, the slots and both
 * LDS sizes are the tile law's), and out [7] = the workspace doubles per pair bands x slots x cells_x x 128: the partial of (band,
 * slot, cell column) is 128 doubles (the 120 sums, sum w, the counts) at ((band slots + slot) cells_x + cell column) 128.  Returns
 * what vitvs_op_photometric_tile_plan returns. */
VITVS_API int vitvs_op_photometric_surface_plan(int32_t height, int32_t width, int32_t level, int32_t cells_y, int32_t cells_x,
                                                int32_t* out);

/* --- several updates in flight ------------------------------------------------------------------
 * One update at one frame pair is a chain of 86 dependent launches; each pays the device's launch-to-launch floor and its own
 * ramp, so the chain leaves most of the chip idle most of the time.  Updates that do not depend on each other (several
 * cameras / control loops sharing the GPU, or a frame stream run as a pipeline) overlap when they are enqueued through
 * DIFFERENT handles on DIFFERENT streams: one call in flight per handle, any number of handles (vit-vs_amd/pipeline.py is
 * that arrangement; measured: profiles/r03_notes.md section 5).  Per-handle options for it:
 *   "graph_replay" 0 / 1   velocity calls replay a hipGraph captured per argument tuple — up to 32 tuples per handle, least
 *                          recently used evicted; evicting a tuple drains the device, like every other event that drops a
 *                          capture — (host cost ~50 us per update
 *                          instead of ~370 us of launch calls, so ONE host thread keeps several streams busy; on a single
 *                          stream plain launches are ~2 % faster, hence the default 0, or the VITVS_GRAPH environment variable
 *                          at creation).  The reference has no counterpart (one torch call chain per update, vitvs_v2.py:464-523).
 *   "in_flight"    n >= 1  a hint: this handle's updates run beside n - 1 others.  From 2 on the one-round GEMM launches
 *                          use 4-wave workgroups (half the LDS: two launches of different queues share a CU), the narrow
 *                          layers two K slices and a grid order that keeps a weight tile in one XCD's L2, and the
 *                          long-sequence attention whole query blocks (no key ranges to merge), the many-row layers
 *                          256 x 256 tiles wherever they divide (fewest operand bytes per FLOP instead of launch balance)
 *                          and at most two K slices.
 *   "reuse_goal_frames" 0 / 1  host-pointer calls: see vitvs_compute_velocity above.
 *   "robust_law"   0 .. 16 an extension beyond the reference (its law is plain least squares, vitvs_v2.py:613-622, with no
 *                          defence against a wrong match).  0 (default): that law, bit for bit.  N >= 1: iteratively
 *                          re-weighted least squares with N re-weightings (N + 1 solves) inside the law's kernel, in fp64:
 *                          per feature pair the residual rho = |e_k - L_k x|, the scale sigma = max(1.4826 median(rho),
 *                          sigma_min) over the live pairs, sigma_min = half a patch pitch in normalised image coordinates
 *                          (0.5 max(stride u_max / S / fx, stride v_max / S / fy)), Tukey's biweight with c = 4.6851:
 *                          w = (1 - t^2)^2 for t = rho / (c sigma) < 1, else 0; v_c = -lambda x of the last weighted solve.
 *                          Zero-padded pairs have weight 0.  Applies to every entry point that evaluates the law; changing
 *                          it drops the handle's captured graphs.  vitvs_last_weights returns the final weights.
 *   "subpatch"     0 / 1   an extension beyond the reference (its features are patch centres, vitvs_v2.py:511-513, so a match
 *                          moves in steps of one patch pitch).  0 (default): that, bit for bit.  1: inside the law's kernel
 *                          every selected match j = nn_1[i] is moved by (dr, dc) patch pitches, per axis the vertex of the
 *                          parabola through the similarities of goal token i to j and its two neighbours (a, m, p):
 *                          den = a - 2 m + p, delta = clamp(0.5 (a - p) / den, -1/2, 1/2) when den < 0, else 0, and 0 on the
 *                          border row / column; the similarities are the ones the arg-max used, recomputed in fp32 from the
 *                          handle's normalised descriptors (binned descriptors: from the raw Gram).  The current-frame pixel is
 *                          rint((centre + delta S / grid) scale), the depth is read there; the goal side stays the patch
 *                          centre.  Applies to every entry point that evaluates the law from the handle's own forward
 *                          (vitvs_compute_velocity[_dev], vitvs_reselect), composes with "robust_law", and drops the handle's
 *                          captured graphs when changed.  vitvs_last_offsets returns the offsets.
 *   "interaction"  0 / 1 / 2  which interaction matrix the law inverts; 1 and 2 are extensions beyond the reference (ViSP's DESIRED
 *                          and MEAN).  With rows(x, y, Z) the two rows of vitvs_v2.py:650-659, (x, y) / (xs, ys) the normalised
 *                          current / goal point of a feature pair, Z the current depth at (u, v) and Z* the goal depth at
 *                          (u*, v*) (vitvs_set_goal_depth_dev): 0 (default) rows(x, y, Z), the reference, bit for bit;
 *                          1 rows(xs, ys, Z*): the current depth is never read, Z_mm may be NULL (no VITVS_NO_DEPTH) and
 *                          feat[..][0] of vitvs_last_details reports Z*; 2 the element-wise mean 0.5 (rows(x, y, Z) +
 *                          rows(xs, ys, Z*)) in fp64, Z_mm required as for 0.  e = s - s*, the selection, the statuses and the
 *                          solve are unchanged; zero-padded rows use the same formulas at pixel (0, 0).  1 and 2 without a goal
 *                          depth that pairs with the call are error -5 before anything is enqueued.  Applies to every entry
 *                          point that evaluates the law (vitvs_compute_velocity[_dev], vitvs_servo_from_nn[_ex]_dev,
 *                          vitvs_reselect), composes with "robust_law" and "subpatch" (the goal side of a refined match stays
 *                          the patch centre), and drops the handle's captured graphs when changed.  vitvs_last_goal_depth
 *                          returns Z*; L of vitvs_last_details is the matrix the mode built.
 *   "select_cells" 1 .. 16  image cells per side of selection mode VITVS_SELECT_BEST (default 4; a token grid with fewer rows
 *                          than that has one cell per row).  1: the num_pairs most similar mutual matches.  n: the best match
 *                          of every non-empty cell first, then every cell's second best, and so on (vitvs_last_order states the
 *                          order exactly).  Read by every entry point that takes a select_mode; changing it drops the handle's
 *                          captured graphs.  The mode is one more launch in front of the law's (87 per update instead of 86),
 *                          measured on an MI355X at 7.4 us for 196 tokens, 18.0 us for 484 and 69.5 us for 3136
 *                          (profiles/best_selection.txt): more than the law it feeds at every size.
 * Returns 0, or -5 for an unknown name / a value out of range. */
VITVS_API int vitvs_set_option(vitvs_handle* h, const char* name, int64_t value);
/* The handles of such an arrangement run ONE network: `h` (created with the same network, input geometry and precision, no
 * tensors uploaded) borrows the device weights of `src` instead of holding a copy — one set of weights stays resident in
 * the Infinity Cache for all queues (a copy per handle: 4 x 172 MB cycle through its 256 MB).  `src` must own its weights and
 * have all of them (vitvs_weights_ready); uploads go to `src` only (vitvs_set_tensor on `h` is error -5).  Ownership is shared:
 * the device memory is released when the LAST handle holding it is destroyed, so `src` and `h` may be destroyed in any order
 * (a borrower whose lender is gone keeps working; nothing can upload to those weights any more).  A borrower may borrow
 * again, from another owner: the call drains the device and drops the updates captured over the previous weights. */
VITVS_API int vitvs_share_weights(vitvs_handle* h, const vitvs_handle* src);

/* --- measurement hooks (bench.py roofline leg) --------------------------------------------------
 * With timing enabled every kernel of the path is dispatched with a HIP event pair that the dispatch
 * itself stamps with its begin / end times (hipExtLaunchKernelGGL on the launch stream; hipGraph replay
 * is bypassed).  vitvs_timing_collect synchronises and returns, per kernel class, the summed kernel
 * milliseconds and the number of launches since the last collect; class names come from vitvs_timing_class_name(0 .. vitvs_timing_classes()-1). */
VITVS_API int vitvs_timing_enable(vitvs_handle* h, int32_t on);
VITVS_API int vitvs_timing_classes(void);
VITVS_API const char* vitvs_timing_class_name(int32_t cls);
VITVS_API int vitvs_timing_collect(vitvs_handle* h, int32_t n_classes, double* total_ms, int32_t* launches);

/* Token count T and descriptor width D' for this handle. */
VITVS_API int vitvs_tokens(const vitvs_handle* h);
VITVS_API int vitvs_desc_dim(const vitvs_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* VITVS_H */
