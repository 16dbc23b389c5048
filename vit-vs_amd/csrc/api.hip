// C ABI of libvitvs_hip.so (include/vitvs.h, include/vitvs_ops.h): handle, weights, the
// compute_velocity path and its seams.  Host-side orchestration only; all arithmetic is in the
// kernels (gemm.hip, attention.hip, elementwise.hip, correspond.hip, servo.hip).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vitvs.h"
#include "../../include/vitvs_ops.h"
#include "io_layout.h"
#include "kernels.h"

namespace vitvs {

static thread_local std::string g_last_error;
thread_local LaunchTiming g_launch_timing;
thread_local int g_current_device = -1;
thread_local int g_updates_in_flight = 1;
static thread_local bool g_op_rig_two_launches = false;   // vitvs_op_rig_two_launches: vitvs_op_rig_law as two plain launches (the measured alternative)
static thread_local int g_op_wexp = 0;   // vitvs_op_weight_exponent: the 2^e the f16x2 weights of the operator hooks carry

int fail_hip(hipError_t e, const char* what, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof(buf), "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
    g_last_error = buf;
    return -100 - (int)e;
}

static inline Precision to_prec(int32_t p) {
    return p == VITVS_F32 ? PREC_F32 : (p == VITVS_F16 ? PREC_F16 : (p == VITVS_F16X2 ? PREC_X2 : PREC_BF16));
}

static inline uint16_t f32_to_f16_host(float f) {   // round to nearest even, as the device's v_cvt_f16_f32
    const _Float16 hval = (_Float16)f;
    uint16_t bits;
    memcpy(&bits, &hval, 2);
    return bits;
}

static inline uint16_t f32_to_bf16_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

struct Block {
    float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr;
    float *qkvb = nullptr, *projb = nullptr, *fc1b = nullptr, *fc2b = nullptr, *ls1 = nullptr, *ls2 = nullptr;
    void *qkvw = nullptr, *projw = nullptr, *fc1w = nullptr, *fc2w = nullptr;
    int qkve = 0, proje = 0, fc1e = 0, fc2e = 0;   // f16x2: each matrix is stored times 2^e (upload_matrix)
};

// Device memory of one set of weights.  Held through a shared_ptr by the handle that uploaded it AND by every handle that
// borrows it (vitvs_share_weights): the memory is freed when the LAST holder is destroyed, in whatever order the handles go,
// so a borrower's kernels and captured graphs never read freed weights.
struct WeightStore {
    int device = 0;
    std::vector<void*> allocs;
    ~WeightStore() {
        int prev = -1;
        (void)hipGetDevice(&prev);
        if (prev != device) (void)hipSetDevice(device);
        for (void* p : allocs) (void)hipFree(p);
        if (prev != device && prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace vitvs

using namespace vitvs;

#include <stddef.h>
static_assert(sizeof(vitvs_config) == 96 && offsetof(vitvs_config, lambda) == 80, "vitvs_config layout is part of the ABI");

struct vitvs_handle {
    vitvs_config cfg;
    Precision prec;
    int device = 0;
    int grid = 0, T = 0, N = 0, Kp = 0, Dp = 0, hidden = 0, n_img_max = 0;
    int R = 0;                // register tokens (vitvs_create_ex): token rows are [cls, R registers, T patches], N = 1 + R + T
    std::string err;
    std::vector<void*> allocs;                      // workspaces, outputs, staging: this handle's own
    std::shared_ptr<WeightStore> wstore;            // the weights: shared with the handles that borrow them
    std::map<std::string, bool> have;
    int desc_keys = -1;   // >= 0 while a velocity update runs: the forward's last launch emits the descriptors and clears this many keys
    bool ready = false;       // cached result of vitvs_weights_ready (reset by vitvs_set_tensor)
    // Pillow-exact resize tables: `rs` of the last camera frame size seen by vitvs_resize_frames_dev, `fr` of the frame
    // geometry declared with vitvs_set_frame_size (fr.in_h == 0: frames arrive at img_size x img_size)
    ResizeArgs rs{}, fr{};
    size_t staged_frame_bytes = 0;   // capacity per frame of st_cur / st_des
    // weights
    std::vector<Block> blk;
    void* pe_w = nullptr;
    int pe_e = 0;
    float *pe_b = nullptr, *cls = nullptr, *pos = nullptr, *reg = nullptr;   // reg: register tokens [R][D] (R > 0 only)
    // activations
    void *Ape = nullptr, *xn = nullptr, *qkv = nullptr, *attn = nullptr, *hid = nullptr;
    float *x = nullptr, *dn = nullptr, *sq = nullptr, *part = nullptr;  // part: split-K partial sums [8][M][D]
    // The correspondence stage at max_pairs pairs (plan_gram): dh and gram_ws are its workspaces, and the forward and the law read
    // `emit` and `refine_from_gram` from it — form and split, and all that follows from them, do not depend on the pairs of a
    // call; only the tile does, which is why enqueue_update plans the call's own launches.
    GramPlan gram;
    unsigned short* dh = nullptr;   // fp16 hi / lo split of dn for the many-token Gram of the 16-bit modes (null: fp32 Gram)
    float* gram_ws = nullptr;       // binned descriptors: raw token Gram [max_pairs][T][T] for the stencil form (correspond.hip; null: the 9 D-wide Gram)
    AttnWorkspace attn_ws;    // key-split states / tickets of the long-sequence attention, sized for every image count <= n_img_max
    size_t dn_elems = 0;
    unsigned long long *row_best = nullptr, *col_best = nullptr;
    size_t best_elems = 0;
    // servo outputs / details
    int32_t *nn1 = nullptr, *nn2 = nullptr, *info = nullptr, *sel_out = nullptr, *s_uv = nullptr;
    float* sim1 = nullptr;
    double *feat = nullptr, *Lws = nullptr;
    double* Wws = nullptr;    // [max_pairs][max_rows] the robust law's final weights (vitvs_last_weights)
    int robust_iters = 0;     // option "robust_law": Tukey re-weightings of the control law, 0 = the reference's plain law
    float* off_ws = nullptr;  // [max_pairs][max_rows][2] the sub-patch offsets of the last law evaluation (vitvs_last_offsets)
    int subpatch = 0;         // option "subpatch": matches are refined off their patch centres, 0 = the reference's patch centres
    int interaction = 0;      // option "interaction": 0 L(s, Z) (the reference), 1 L(s*, Z*), 2 their mean
    uint16_t* zgoal = nullptr;  // [max_pairs][T + 1] mm, goal depth at every token's patch centre and at pixel (0, 0) (vitvs_set_goal_depth_dev)
    int n_goal_depth = 0;     // goal depth images held in zgoal, 0: none
    double* zgoal_ws = nullptr; // [max_pairs][max_rows] Z* of the last law evaluation's feature rows (vitvs_last_goal_depth)
    // The follow-on laws (vitvs_{rig,rig_robust,pose,homography,pose_rig}_velocity[_dev]), each with two blocks that its first
    // call allocates (law_blocks): *_ws, the kernels' own scratch at max_pairs x max_rows (rig.hip's begins with a ticket that
    // every launch must find zero: the laws share nothing), and *_io, the device side of the host-pointer form, laid out by
    // io_layout.h's list of that law.
    unsigned char *rig_ws = nullptr, *rig_io = nullptr;             // RigIo: both forms of the rig law
    unsigned char *pose_ws = nullptr, *pose_io = nullptr;           // PoseIo
    unsigned char *hom_ws = nullptr, *hom_io = nullptr;             // HomographyIo
    unsigned char *pose_rig_ws = nullptr, *pose_rig_io = nullptr;   // PoseRigIo
    // The roll search (vitvs_roll_velocity[_dev], roll.hip), the same arrangement: roll_ws = the flag `rolled` the pick leaves for
    // the law (one int32 on a 256-byte line of its own), then the current frame's four quarter-turned copies [4][S][S][3]
    unsigned char *roll_ws = nullptr, *roll_io = nullptr;           // RollIo
    // The photometric law (vitvs_photometric_velocity[_dev], photometric.hip) reads frames, not what a velocity call left: photo_ws =
    // its band partials at max_pairs pairs of the most bands a frame can have, photo_io = PhotometricIo at max_pairs frames of
    // v_max x u_max
    unsigned char *photo_ws = nullptr, *photo_io = nullptr;
    // its robust form (vitvs_photometric_robust_velocity[_dev]) shares nothing with it: photo_robust_ws = the 48-double band partials,
    // one histogram and one state per pair (photometric_robust_ws_bytes), photo_robust_io = PhotometricRobustIo
    unsigned char *photo_robust_ws = nullptr, *photo_robust_io = nullptr;
    // the rig form (vitvs_photometric_rig_velocity[_dev]) runs in photo_robust_ws; photo_rig_io = PhotometricRigIo
    unsigned char* photo_rig_io = nullptr;
    // the tile form (vitvs_photometric_tile_velocity[_dev]) shares nothing with them: photo_tile_ws = the 48-double segment partials,
    // one histogram and one state per pair (photometric_tile_ws_bytes), photo_tile_io = PhotometricTileIo
    unsigned char *photo_tile_ws = nullptr, *photo_tile_io = nullptr;
    // the surface form (vitvs_photometric_surface_velocity[_dev]) likewise: photo_surface_ws = the 128-double segment partials, one
    // histogram and one state per pair (photometric_surface_ws_bytes), photo_surface_io = PhotometricSurfaceIo
    unsigned char *photo_surface_ws = nullptr, *photo_surface_io = nullptr;
    // the last law evaluation, eager or replayed (note_law); its plan says which of Wws, off_ws and zgoal_ws it wrote
    int last_pairs = 0, last_T = 0;
    ServoPlan last_law;
    // Selection mode BEST (select.hip): the visiting order its kernel leaves for the law, laid out as nn1 is ([pairs][T] of the call,
    // best_elems entries), the option "select_cells", and whether the last law evaluation ran on it (vitvs_last_order)
    int32_t* order_ws = nullptr;
    int select_cells = 4;
    bool last_best = false;
    // device copies of the frames a host-pointer call hands over (filled from the pinned block, HostStage below), and the
    // graph replays' own copy of the selection
    uint8_t *st_cur = nullptr, *st_des = nullptr;
    int32_t *st_sel = nullptr, *st_nsel = nullptr;
    // per-kernel-class timing (HIP events on the launch stream), see vitvs_timing_*
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_class;      // class of event pair i (events 2i, 2i+1)
    size_t ev_used = 0;
    // captured hipGraphs of compute_velocity_dev (opt-in, VITVS_GRAPH=1), keyed on the argument tuple
    struct GraphEntry {
        std::vector<uintptr_t> key;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        uint64_t last_use = 0;
    };
    std::vector<GraphEntry> graphs;
    uint64_t graph_clock = 0;
    bool use_graphs = false;
    bool borrowed = false;    // weights belong to another handle (vitvs_share_weights): never uploaded to, never freed here
    int in_flight = 1;        // vitvs_set_option "in_flight": updates expected to run beside this handle's (tile plan hint)
    int goal_frames = 0;      // goal frames whose tokens / descriptors are cached in rows [0, goal_frames) (vitvs_set_goal_dev)
    // Host-pointer entry points (vitvs_compute_velocity, vitvs_set_goal): ONE block of pinned, device-visible host memory,
    // allocated on first use.  Caller buffers are copied into it with memcpy; the frames then reach device memory through a
    // short copy launch on the update's own stream (launch_copy16), the intrinsics / visiting order / depth image are read by
    // the law's kernel in place (it touches <= max_rows depth pixels), and v_c / status / the feature rows are written back
    // into it by the device — no copy-engine command, no pageable transfer, one wait at the end.
    struct HostStage {
        unsigned char* base = nullptr;
        size_t frame_cap = 0;     // bytes per staged frame
        uint8_t *cur = nullptr, *des = nullptr;
        uint16_t* depth = nullptr;
        double *K = nullptr, *vc = nullptr;
        int32_t *sel = nullptr, *nsel = nullptr, *status = nullptr;
        unsigned char* det = nullptr;   // image of the device's detail block (info | s_uv | feat) of the last host-pointer call
    } hs;
    hipStream_t host_stream = nullptr;
    bool details_pinned = false;        // hs.det holds the last call's detail block (vitvs_last_details serves it from there)
    struct HostTables { int n_pairs = 0, T = 0; bool have_depth = false; int des_shared = 0; } host_tables;   // what vitvs_reselect may build on
    unsigned char* det_block = nullptr; // device copy of the detail block (detail_pointers), one allocation
    size_t det_bytes = 0;
    std::vector<int32_t> depth_sites;   // linear pixel index of every token's patch centre that lies inside the depth image, and of pixel
                                        // (0, 0), which a zero-padded row reads (the only pixels the law reads: servo.hip token_pixel,
                                        // restated on the host at creation)
    bool reuse_goal = false;            // option "reuse_goal_frames": I_des of a host-pointer call is not staged again while its address repeats
    const void* staged_des = nullptr;   // host address, frame count and geometry of the goal frames in st_des
    size_t staged_des_bytes = 0;
    // A _dev call returns once its work is enqueued on the CALLER's stream, and nothing orders that stream against host_stream (non-
    // blocking) or the null stream.  Every _dev entry point that touches the workspace, the arg-max keys, the goal rows, the detail
    // block or the goal-depth table sets this; a host-pointer form that finds it set drains the device before its first launch
    // (order_behind_dev) and clears it.  A flag, not an event or the stream: nothing may be recorded inside a caller's capture, and
    // the caller may destroy the stream when the call has returned.
    bool dev_pending = false;
};

namespace {

// The detail block — what vitvs_last_details hands out except `selected` and L — is one allocation laid out
// info [P][8] i32 | s_uv [P][R][4] i32 | feat [P][R][4] f64 | nn_1 [P][T] i32 | nn_2 [P][T] i32 | sim_1 [P][T] f32, so that a host-pointer
// call can hand the reference's return values (s_uv*, s_uv, the selected similarities, and the tables its host-side draw needs)
// to the host with ONE copy launch into the handle's pinned block (same layout) behind the law's kernel.
void detail_pointers(vitvs_handle* h, unsigned char* base) {
    const size_t P = h->cfg.max_pairs, R = h->cfg.max_rows;
    h->info = reinterpret_cast<int32_t*>(base);
    h->s_uv = reinterpret_cast<int32_t*>(base + P * 32);
    h->feat = reinterpret_cast<double*>(base + P * 32 + P * R * 16);
    h->nn1 = reinterpret_cast<int32_t*>(base + P * 32 + P * R * 48);
    h->nn2 = h->nn1 + h->best_elems;
    h->sim1 = reinterpret_cast<float*>(h->nn2 + h->best_elems);
}

int set_err(vitvs_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    g_last_error = msg;
    return code;
}

// Every entry point that takes a handle runs on the handle's device, whatever device the calling thread had current
// (include/vitvs.h: "a handle is bound to the HIP device that was current when it was created"); the caller's device is
// restored on return.  The pointer-only operator hooks (vitvs_op_*) run on the caller's current device.
struct DeviceScope {
    int prev = -1, prev_hint = 1;
    bool switched = false;
    explicit DeviceScope(const vitvs_handle* h) {
        prev_hint = g_updates_in_flight;
        (void)hipGetDevice(&prev);
        const int want = h ? h->device : prev;
        if (want != prev) switched = hipSetDevice(want) == hipSuccess;
        g_current_device = switched ? want : prev;
        if (h) g_updates_in_flight = h->in_flight;    // the tile plan of this handle's launches (kernels.h); the pointer-only
                                                      // operator hooks keep the thread's own hint (vitvs_op_plan_in_flight)
    }
    ~DeviceScope() {
        if (switched) { (void)hipSetDevice(prev); g_current_device = prev; }
        g_updates_in_flight = prev_hint;
    }
};

template <typename T>
int dev_alloc_into(std::vector<void*>& owner, T** out, size_t count) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, count * sizeof(T) + 256);
    if (e != hipSuccess) return fail_hip(e, "hipMalloc", __FILE__, __LINE__);
    owner.push_back(p);
    (void)hipMemset(p, 0, count * sizeof(T) + 256);   // detail rows a call does not write read as zeros, not as stale memory
    *out = reinterpret_cast<T*>(p);
    return 0;
}
template <typename T>
int dev_alloc(vitvs_handle* h, T** out, size_t count) { return dev_alloc_into(h->allocs, out, count); }

// frees one of the handle's own blocks (not a weight) and forgets it
void dev_free(vitvs_handle* h, void* p) {
    if (!p) return;
    h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), p), h->allocs.end());
    (void)hipFree(p);
}

// ---- what the follow-on laws' entry points share (the rig law .. the pose rig law below) ----
// A law's two blocks, allocated by its first call: set-up, not the call path (and never inside a capture), as
// vitvs_set_goal_depth_dev's.
int law_blocks(vitvs_handle* h, const char* law, unsigned char** ws, size_t ws_bytes, unsigned char** io, size_t io_bytes) {
    if (*ws) return 0;
    int rc = dev_alloc(h, ws, ws_bytes);
    if (!rc) rc = dev_alloc(h, io, io_bytes);
    if (rc) return set_err(h, rc, std::string(law) + " workspace allocation failed");
    VITVS_HIP_CHECK(hipDeviceSynchronize());   // the blocks (the rig law's ticket above all) are zero before any stream uses them
    return 0;
}

// A law evaluates what the last velocity call left: there was one, and `n` (the entry point's `count`) is its pair count.
int follows_velocity_call(vitvs_handle* h, const char* entry, const char* count, int n) {
    if (!h->last_pairs) return set_err(h, -5, std::string(entry) + " follows a velocity call on the same handle");
    if (n != h->last_pairs)
        return set_err(h, -5, std::string(count) + " (" + std::to_string(n) + ") is not the pair count of the last law evaluation (" +
                                  std::to_string(h->last_pairs) + ")");
    return 0;
}

// the token grid's pitch along an image side of `extent` sensor pixels, in those pixels
double token_pitch(const vitvs_config& c, int extent) { return (double)(c.stride * extent) / (double)c.img_size; }

// What the camera's law left in the handle, as PoseArgs, PoseRigArgs and HomographyArgs read it ...
template <typename Args>
void camera_law_state(const vitvs_handle* h, const double* K, int n_iter, Args& a) {
    const vitvs_config& c = h->cfg;
    a.selected = h->sel_out; a.s_uv = h->s_uv; a.feat = h->feat; a.info = h->info; a.K = K;
    a.pitch_u = token_pitch(c, c.u_max); a.pitch_v = token_pitch(c, c.v_max);
    a.lambda = c.lambda; a.n_iter = n_iter; a.weights_stride = c.max_rows;
}
// ... and the goal depth, for the two laws that read it
template <typename Args>
void goal_depth_state(const vitvs_handle* h, Args& a) {
    a.zgoal = h->zgoal; a.zgoal_stride = h->n_goal_depth == 1 ? 0 : h->T + 1; a.T = h->T;
}

// The host-pointer form of a follow-on law over its list `io`, placed in the handle's `block` of that law: the inputs up at the
// call's counts, the law's _dev form on the handle's host stream, the outputs the caller asked for down.  A failing _dev form
// returns before anything is copied back.
template <typename DevForm>
int host_call(vitvs_handle* h, IoList io, unsigned char* block, DevForm dev_form) {
    io_place(io, block);
    VITVS_HIP_CHECK(hipDeviceSynchronize());    // the law evaluation this builds on may still run on a stream of the caller's
    for (const IoField* f = io.f; f != io.f + io.n; ++f)
        if (f->input && f->host) VITVS_HIP_CHECK(hipMemcpy(f->dev, f->host, f->count * f->elem, hipMemcpyHostToDevice));
    hipStream_t st = h->host_stream;            // (null before the first host-pointer velocity call: the default stream)
    if (int rc = dev_form(st)) return rc;
    VITVS_HIP_CHECK(hipStreamSynchronize(st));
    h->dev_pending = false;                     // (the device was drained above, and this call's own work just now)
    for (const IoField* f = io.f; f != io.f + io.n; ++f)
        if (!f->input && f->host) VITVS_HIP_CHECK(hipMemcpy(f->host, f->dev, f->count * f->elem, hipMemcpyDeviceToHost));
    return 0;
}

// the laws' operator hooks: a scratch size as the int32 they return, and the pose, pose rig and homography plans' common output
int bytes_i32(size_t b) { return b > 0x7fffffffu ? -3 : (int)b; }
template <typename Plan>
int plan_out(int rc, const Plan& pl, int32_t* out) {
    out[0] = (int32_t)pl.lds; out[1] = pl.robust; out[2] = pl.lds_opt_in;
    return rc;
}

int upload_f32(vitvs_handle* h, float** dst, const float* src, size_t n) {
    if (!*dst) {
        int rc = dev_alloc_into(h->wstore->allocs, dst, n);
        if (rc) return rc;
    }
    VITVS_HIP_CHECK(hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// matrix [rows][cols] fp32 host -> device in the handle's precision, row stride `ld` (zero padded).
// f16x2 (PREC_X2): every element becomes an fp16 pair hi = fp16(w 2^e), lo = fp16(w 2^e - hi), rows laid out as [hi of 32
// columns | lo of the same 32] per 64 fp16 (csrc/common.h); e is the power of two that puts the matrix's largest magnitude in
// [2^12, 2^13), so the lo halves of all but negligible weights are NORMAL fp16 numbers (22 significant bits) and nothing
// overflows; the GEMM multiplies its sums by 2^-e (*wexp, 0 .. 31).
int upload_matrix(vitvs_handle* h, void** dst, const float* src, size_t rows, size_t cols, size_t ld, int* wexp = nullptr) {
    const size_t es = elem_size(h->prec);
    if (!*dst) {
        unsigned char* p = nullptr;
        int rc = dev_alloc_into(h->wstore->allocs, &p, rows * ld * es);
        if (rc) return rc;
        *dst = p;
    }
    std::vector<unsigned char> tmp(rows * ld * es, 0);
    if (h->prec == PREC_X2) {
        if (ld % 32 != 0) return set_err(h, -6, "f16x2 rows are multiples of 32 columns");
        float amax = 0.f;
        for (size_t i = 0; i < rows * cols; ++i) amax = std::max(amax, fabsf(src[i]));
        int e = 0;
        if (amax > 0.f && std::isfinite(amax)) {
            int ex = 0;
            (void)frexpf(amax, &ex);                       // amax = f 2^ex, f in [0.5, 1)
            e = std::min(31, std::max(0, 13 - ex));        // amax 2^e in [2^12, 2^13)
        }
        if (wexp) *wexp = e;
        const float sc = ldexpf(1.0f, e);
        uint16_t* d = reinterpret_cast<uint16_t*>(tmp.data());
        for (size_t r = 0; r < rows; ++r)
            for (size_t c = 0; c < cols; ++c) {
                const float v = src[r * cols + c] * sc;    // exact (power of two)
                const float vc = std::min(65504.0f, std::max(-65504.0f, v));
                const _Float16 hi = (_Float16)vc;
                const size_t at = r * 2 * ld + ((c >> 5) << 6) + (c & 31);
                d[at] = f32_to_f16_host((float)hi);
                d[at + 32] = f32_to_f16_host(v - (float)hi);
            }
        VITVS_HIP_CHECK(hipMemcpy(*dst, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
        return 0;
    }
    for (size_t r = 0; r < rows; ++r) {
        if (h->prec == PREC_F32) {
            memcpy(tmp.data() + r * ld * 4, src + r * cols, cols * 4);
        } else {
            uint16_t* d = reinterpret_cast<uint16_t*>(tmp.data()) + r * ld;
            if (h->prec == PREC_F16) for (size_t c = 0; c < cols; ++c) d[c] = f32_to_f16_host(src[r * cols + c]);
            else for (size_t c = 0; c < cols; ++c) d[c] = f32_to_bf16_host(src[r * cols + c]);
        }
    }
    VITVS_HIP_CHECK(hipMemcpy(*dst, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
    return 0;
}

int check_cfg(const vitvs_config* c, std::string& why) {
    if (c->abi_version != VITVS_ABI_VERSION) { why = "abi_version mismatch"; return -1; }
    if (c->dim <= 0 || c->dim % 128 != 0) { why = "dim must be a positive multiple of 128"; return -1; }
    if (c->heads <= 0 || c->dim != c->heads * 64) { why = "dim / heads must be 64"; return -1; }
    if (c->patch <= 0 || c->stride <= 0 || c->img_size < c->patch) { why = "bad patch/stride/img_size"; return -1; }
    if ((c->img_size - c->patch) % c->stride != 0) { why = "img_size - patch must be a multiple of stride"; return -1; }
    if (c->blocks <= 0) { why = "blocks must be >= 1"; return -1; }
    if (c->precision != VITVS_F32 && c->precision != VITVS_BF16 && c->precision != VITVS_F16 && c->precision != VITVS_F16X2) { why = "unknown precision"; return -1; }
    if (c->max_pairs <= 0 || c->num_pairs <= 0 || c->max_rows < c->num_pairs) { why = "bad capacity"; return -1; }
    if (c->u_max <= 0 || c->v_max <= 0) { why = "bad camera resolution"; return -1; }
    if (c->dim != 128 && c->dim != 256 && c->dim != 384 && c->dim != 768 && c->dim != 1024) {
        why = "dim must be one of 128, 256, 384, 768, 1024";
        return -1;
    }
    return 0;
}

hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// The stream of a _dev entry point: work on any stream but the handle's own host stream is the caller's to wait for, so it counts as
// pending until a host-pointer form has drained the device (vitvs_handle::dev_pending).  The host-pointer forms that pass the null
// stream through a _dev form (host_call before the first host-pointer velocity call, vitvs_set_goal_depth) drain it themselves.
hipStream_t dev_stream(vitvs_handle* h, void* s) {
    hipStream_t st = as_stream(s);
    if (!st || st != h->host_stream) h->dev_pending = true;
    return st;
}
// What a host-pointer form does before its first launch: wait for the _dev work this handle may still have on a caller's stream.
// A loop of host-pointer calls alone finds the flag clear and makes no HIP call here.
int order_behind_dev(vitvs_handle* h) {
    if (!h->dev_pending) return 0;
    VITVS_HIP_CHECK(hipDeviceSynchronize());
    h->dev_pending = false;
    return 0;
}

// Captured updates hold addresses (weights, resize tables) and a tile plan: whoever changes one of those drops them, after
// the device has drained (a replay may still be running).
void drop_graphs(vitvs_handle* h) {
    for (auto& g : h->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    h->graphs.clear();
}

enum KernelClass : int {
    KC_PATCHIFY = 0, KC_PATCH_EMBED, KC_LAYERNORM, KC_QKV, KC_ATTENTION, KC_PROJ, KC_FC1, KC_FC2, KC_DESCRIPTORS,
    KC_GRAM, KC_SERVO, KC_RESIDUAL_LN, KC_GRAM_STENCIL, KC_COUNT
};
const char* const kClassNames[KC_COUNT] = {"patchify", "patch_embed", "layernorm", "qkv", "attention", "proj",
                                           "fc1", "fc2", "descriptors", "gram_argmax", "servo",
                                           "residual_ln", "gram_stencil"};

// the class each step of the correspondence stage is timed in, by GramStep; the split of the descriptors is not timed (-1)
const int kGramStepClass[] = {KC_DESCRIPTORS, -1, KC_GRAM, KC_GRAM, KC_GRAM_STENCIL};

// When timing is enabled, arms the launch helper (kernels.h) so that the next kernel launched inside the span
// is dispatched with an event pair stamped with its own begin / end times.
struct Span {
    vitvs_handle* h;
    bool armed = false;
    Span(vitvs_handle* h_, int cls, hipStream_t) : h(h_) {
        if (!h->timing || cls < 0) return;
        if (h->ev_used + 2 > h->ev_pool.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            h->ev_pool.push_back(a);
            h->ev_pool.push_back(b);
        }
        g_launch_timing.start = h->ev_pool[h->ev_used];
        g_launch_timing.stop = h->ev_pool[h->ev_used + 1];
        h->ev_used += 2;
        h->ev_class.push_back(cls);
        armed = true;
    }
    ~Span() {
        if (armed && g_launch_timing.start) {   // nothing was launched inside the span: drop the pair
            g_launch_timing = LaunchTiming{};
            h->ev_used -= 2;
            h->ev_class.pop_back();
        }
    }
};

// Bytes of one frame as the caller hands it over: img_size x img_size x 3, or the declared camera geometry.
static size_t frame_bytes(const vitvs_handle* h) {
    return h->fr.in_h ? (size_t)h->fr.in_h * h->fr.in_w * 3 : (size_t)h->cfg.img_size * h->cfg.img_size * 3;
}

// One launch chain's view of the workspaces (a contiguous range of images).
struct ChainCtx {
    int cnt = 0, M = 0;
    float* x = nullptr;
    unsigned char *xn = nullptr, *qkv = nullptr, *attn = nullptr, *hid = nullptr, *Ape = nullptr;
    float* part = nullptr;
    PatchifyArgs pa;
    const ResizeArgs* rs = nullptr;   // camera-resolution frames (vitvs_set_frame_size): resize inside the patch-row build
    bool want_desc = false;   // the last residual_ln also writes what the Gram plan asks of it (GramEmit; launch_residual_ln)
    DescOut desc;
    struct { LinearPlan embed, qkv, proj, fc1, fc2; AttnPlan attn; } plan;   // of the chain's six launch shapes (forward_chain)
};

// The forward, operator by operator, on one stream.  (The two FRAMES of one update as two chains — on two streams, or in
// lockstep on one stream with hipExtAnyOrderLaunch — were measured in round 1 and gained nothing: half-size launches cost
// nearly what full-size ones do, gfx9 ignores the any-order flag, and the kernel-trace timelines that showed the queues
// taking turns were the profiler's own serialisation (profiles/r03_notes.md section 5).  What does overlap is whole,
// independent UPDATES on separate handles and queues: include/vitvs.h "several updates in flight", vit-vs_amd/pipeline.py.)
int forward_launches(vitvs_handle* h, const ChainCtx& cx, hipStream_t st) {
    const vitvs_config& c = h->cfg;
    const int D = c.dim;
    int rc = 0;
    { Span sp(h, KC_PATCHIFY, st);
        rc = launch_patchify(h->prec, cx.pa, cx.rs, cx.Ape, cx.x, st); }
    // Patch embedding as a split-K GEMM (more workgroups than its 84 output tiles), finished together with
    // cls / pos_embed and block 0's norm1 by one residual_ln-style launch.
    // Block i: qkv -> attention -> proj (split-K partials) -> [residual + norm2] -> fc1+GELU ->
    // fc2 (split-K partials) -> [residual + norm1 of block i+1].
    if (!rc) { Span sp(h, KC_PATCH_EMBED, st);
        rc = launch_linear(cx.plan.embed, cx.Ape, h->pe_w, nullptr, cx.part, 0, st, h->pe_e); }
    if (!rc) { Span sp(h, KC_LAYERNORM, st);
        rc = launch_embed_ln(h->prec, cx.x, cx.part, cx.plan.embed.splits, h->pe_b, h->pos, h->cls, h->reg, h->blk[0].n1w,
                             h->blk[0].n1b, cx.xn, cx.cnt, h->T, 1 + h->R, D, c.ln_eps, st); }
    for (int i = 0; i < c.blocks && !rc; ++i) {
        const Block& b = h->blk[i];
        const Block* nx = (i + 1 < c.blocks) ? &h->blk[i + 1] : nullptr;
        { Span sp(h, KC_QKV, st);
            rc = launch_linear(cx.plan.qkv, cx.xn, b.qkvw, b.qkvb, cx.qkv, 0, st, b.qkve); }
        if (!rc) { Span sp(h, KC_ATTENTION, st);
            rc = launch_attention(cx.plan.attn, cx.qkv, cx.attn, st, &h->attn_ws, plain16(h->prec)); }
        if (!rc) { Span sp(h, KC_PROJ, st);
            rc = launch_linear(cx.plan.proj, cx.attn, b.projw, nullptr, cx.part, 0, st, b.proje); }
        if (!rc) { Span sp(h, KC_RESIDUAL_LN, st);
            rc = launch_residual_ln(h->prec, cx.x, cx.part, cx.plan.proj.splits, b.projb, b.ls1, b.n2w, b.n2b, cx.xn, cx.M, D,
                                    c.ln_eps, st); }
        if (!rc) { Span sp(h, KC_FC1, st);
            rc = launch_linear(cx.plan.fc1, cx.xn, b.fc1w, b.fc1b, cx.hid, 1, st, b.fc1e); }
        if (!rc) { Span sp(h, KC_FC2, st);
            rc = launch_linear(cx.plan.fc2, cx.hid, b.fc2w, nullptr, cx.part, 0, st, b.fc2e); }
        if (!rc) { Span sp(h, KC_RESIDUAL_LN, st);
            rc = launch_residual_ln(h->prec, cx.x, cx.part, cx.plan.fc2.splits, b.fc2b, b.ls2, nx ? nx->n1w : nullptr,
                                    nx ? nx->n1b : nullptr, cx.xn, cx.M, D, c.ln_eps, st,
                                    (!nx && cx.want_desc) ? &cx.desc : nullptr); }
    }
    if (rc) return set_err(h, rc, "forward launch failed");
    return 0;
}

ChainCtx fill_ctx(vitvs_handle* h, int i0, int cnt, int n_des, const uint8_t* des, const uint8_t* cur, float* part) {
    const vitvs_config& c = h->cfg;
    const int D = c.dim;
    const size_t es = elem_size(h->prec);
    const size_t img_bytes = frame_bytes(h);
    const size_t row0 = (size_t)i0 * h->N;
    ChainCtx cx;
    cx.rs = h->fr.in_h ? &h->fr : nullptr;
    cx.cnt = cnt; cx.M = cnt * h->N; cx.part = part;
    cx.x = h->x + row0 * D;
    cx.xn = (unsigned char*)h->xn + row0 * D * es;
    cx.qkv = (unsigned char*)h->qkv + row0 * 3 * D * es;
    cx.attn = (unsigned char*)h->attn + row0 * D * es;
    cx.hid = (unsigned char*)h->hid + row0 * h->hidden * es;
    cx.Ape = (unsigned char*)h->Ape + (size_t)i0 * h->T * h->Kp * es;
    PatchifyArgs& pa = cx.pa;
    pa.n_des = std::max(0, std::min(i0 + cnt, n_des) - i0);
    pa.n_cur = cnt - pa.n_des;
    pa.des = des ? des + (size_t)std::min(i0, n_des) * img_bytes : nullptr;
    pa.cur = cur ? cur + (size_t)std::max(i0 - n_des, 0) * img_bytes : nullptr;
    pa.S = c.img_size; pa.patch = c.patch; pa.stride = c.stride; pa.grid = h->grid; pa.Kp = h->Kp; pa.D = D;
    for (int i = 0; i < 3; ++i) { pa.mean[i] = c.mean[i]; pa.std[i] = c.std[i]; }
    pa.cls = h->cls; pa.pos = h->pos; pa.prefix = 1 + h->R;
    return cx;
}

// Forward of images [i0, i0 + cnt) of the call's image list (desired frames first, then current
// frames) on stream `st`: an independent chain of launches touching only those images' rows.
int forward_chain(vitvs_handle* h, int i0, int cnt, int n_des, const uint8_t* des, const uint8_t* cur, float* part,
                  hipStream_t st) {
    if (i0 == 0) h->goal_frames = 0;            // rows of a cached goal are about to be overwritten (vitvs_set_goal_dev re-arms)
    h->details_pinned = false;                  // the arg-max keys vitvs_reselect builds on are cleared or rewritten from here on
    h->host_tables = vitvs_handle::HostTables{};
    ChainCtx cx = fill_ctx(h, i0, cnt, n_des, des, cur, part);
    const Precision p = h->prec;
    const int D = h->cfg.dim;
    cx.plan.embed = plan_linear(p, cnt * h->T, D, h->Kp, EPI_PARTIAL);
    cx.plan.qkv = plan_linear(p, cx.M, 3 * D, D, EPI_STORE);
    cx.plan.proj = plan_linear(p, cx.M, D, D, EPI_PARTIAL);
    cx.plan.fc1 = plan_linear(p, cx.M, h->hidden, D, EPI_STORE);
    cx.plan.fc2 = plan_linear(p, cx.M, D, h->hidden, EPI_PARTIAL);
    cx.plan.attn = plan_attention(p, cnt, h->N, h->cfg.heads);
    if (h->desc_keys >= 0 && h->gram.emit != EMIT_NONE) {
        cx.want_desc = true;
        if (h->gram.emit == EMIT_SQ) cx.desc.sq = h->sq + (size_t)i0 * h->T;
        else cx.desc.dn = h->dn + (size_t)i0 * h->T * h->Dp;
        cx.desc.zero_a = h->row_best; cx.desc.zero_b = h->col_best;
        cx.desc.T = h->T;
        cx.desc.P = 1 + h->R;
        cx.desc.zero_count = (i0 == 0 || h->goal_frames > 0) ? h->desc_keys : 0;   // the call's only chain clears the arg-max keys
    }
    return forward_launches(h, cx, st);
}

int forward(vitvs_handle* h, int n_des, const uint8_t* des, int n_cur, const uint8_t* cur, hipStream_t st) {
    const int n_img = n_des + n_cur;
    if (n_img <= 0 || n_img > h->n_img_max) return set_err(h, -3, "frame count exceeds the handle's capacity");
    if (vitvs_weights_ready(h) != 0) return set_err(h, -4, "weights not fully loaded: " + h->err);
    return forward_chain(h, 0, n_img, n_des, des, cur, h->part, st);
}

// num_pairs of one call: <= 0 means the handle's default (cfg.num_pairs); the reference changes it per call site
// (24 in the servo loop, 48 in the rotation search, vitvs_v2.py:1151-1189), so it is a per-call argument.
int call_num_pairs(const vitvs_handle* h, int32_t num_pairs) { return num_pairs > 0 ? num_pairs : h->cfg.num_pairs; }

// The sub-patch refinement of one law evaluation: OFF, from a caller's offset table, or from the handle's own forward
struct RefineSpec {
    const float* table = nullptr;   // [T][2] (vitvs_servo_from_nn_ex_dev)
    bool from_forward = false;      // option "subpatch": the descriptors / raw Gram the forward left in the handle
    int des_shared = 0;
};
// The law of one call over T tokens, planned once from the handle's options and the call's refinement (plan_servo): what
// run_servo launches, what a replay "last ran", and what a host-pointer call stages of the depth image
int plan_law(vitvs_handle* h, int T, const RefineSpec& rf, ServoPlan& plan) {
    const RefineSource src = rf.table ? RS_TABLE : !rf.from_forward ? RS_OFF : h->gram.refine_from_gram ? RS_GRAM : RS_DESC;
    const int rc = plan_servo(T, h->cfg.max_rows, h->robust_iters, src, h->interaction, &plan);
    return rc ? set_err(h, rc, "servo launch failed (LDS budget or bad arguments)") : 0;
}

// The one place that records which law the handle's per-row workspaces and detail block are about to hold
void note_law(vitvs_handle* h, int n_pairs, int T, const ServoPlan& plan, int select_mode) {
    h->last_pairs = n_pairs; h->last_T = T; h->last_law = plan;
    h->last_best = select_mode == VITVS_SELECT_BEST;
}

// The geometry of a law call over T = g * g tokens: what token_pixel (servo.hip) reads
void servo_geometry(const vitvs_handle* h, int T, int g, ServoArgs& a) {
    const vitvs_config& c = h->cfg;
    a.T = T; a.grid = g;
    a.input_size = c.img_size; a.u_max = c.u_max; a.v_max = c.v_max; a.depth_h = c.v_max; a.depth_w = c.u_max;
    const double scale = (double)c.img_size / (double)g;                 // vitvs_v2.py:511
    a.scale_f = (float)scale; a.half_f = (float)(scale / 2.0);
    a.scale_x = (double)c.u_max / (double)c.img_size;                    // vitvs_v2.py:544
    a.scale_y = (double)c.v_max / (double)c.img_size;                    // vitvs_v2.py:545
}

// Option "interaction" != 0: the law of a call of n_pairs pairs over T tokens needs a goal depth that pairs with it.  Host-side
// state, checked by every entry point before it enqueues anything (and never inside a body that a hipGraph captures).
int check_interaction(vitvs_handle* h, int n_pairs, int T) {
    if (!h->interaction) return 0;
    if (!h->n_goal_depth) return set_err(h, -5, "option interaction needs a goal depth (vitvs_set_goal_depth_dev)");
    if (T != h->T) return set_err(h, -5, "the goal depth table is laid out for the handle's own token grid");
    if (h->n_goal_depth != n_pairs && h->n_goal_depth != 1)
        return set_err(h, -5, "the goal depth holds " + std::to_string(h->n_goal_depth) + " images: one per pair, or one for all");
    return 0;
}

// What every entry point asks of a call's selection over T tokens, before it stages or enqueues anything
int check_selection(vitvs_handle* h, int T, int mode, const int32_t* selection, const int32_t* n_selected, int num_pairs) {
    if (num_pairs <= 0 || num_pairs > h->cfg.max_rows) return set_err(h, -5, "num_pairs must be in 1 .. max_rows");
    if (mode < 0 || mode > VITVS_SELECT_BEST) return set_err(h, -5, "unknown selection mode");
    if (mode == VITVS_SELECT_BEST) {            // the order is made on the device: selection and n_selected are not read
        BestOrderPlan bp;
        const int rc = plan_best_order(T, h->select_cells, &bp);
        return rc ? set_err(h, rc == -3 ? -3 : -5, "BEST selection needs a square token grid whose keys fit in LDS") : 0;
    }
    if (mode != VITVS_SELECT_DENSE && !selection) return set_err(h, -5, "selection array required for this mode");
    if (mode == VITVS_SELECT_EXPLICIT && !n_selected) return set_err(h, -5, "n_selected required for EXPLICIT");
    if (mode == VITVS_SELECT_DENSE && h->cfg.max_rows < T) return set_err(h, -5, "DENSE selection needs max_rows >= T");
    return 0;
}

// The law on the arg-max keys in the handle, for a selection the entry point has checked (check_selection)
int run_servo(vitvs_handle* h, int n_pairs, int T, const uint16_t* Z, const double* K, int mode, int num_pairs,
              const int32_t* selection, const int32_t* n_selected, double* v_c, int32_t* status, hipStream_t st,
              const RefineSpec& rf = RefineSpec{}, const int32_t* rolled = nullptr) {
    const vitvs_config& c = h->cfg;
    const int g = (int)floor(sqrt((double)T));  // reference: int(np.sqrt(T)), vitvs_v2.py:75
    if (g * g != T) return set_err(h, -5, "token count is not a square grid");
    ServoPlan plan;
    if (int rc = plan_law(h, T, rf, plan)) return rc;
    const bool best = mode == VITVS_SELECT_BEST;
    if (best) {
        // the visiting order from the keys themselves (select.hip), then the law exactly as on a caller's order
        BestOrderPlan bp;
        if (int rc = plan_best_order(T, h->select_cells, &bp)) return set_err(h, rc, "BEST selection: the token count does not fit in LDS");
        if ((size_t)n_pairs * T > h->best_elems) return set_err(h, -3, "T exceeds the handle's workspace");
        int rc = 0;
        { Span sp(h, KC_SERVO, st); rc = launch_best_order(bp, n_pairs, h->row_best, h->col_best, h->order_ws, st); }
        if (rc) return set_err(h, rc, "best-order launch failed");
        selection = h->order_ws; n_selected = nullptr;
    }
    ServoArgs a;
    memset(&a, 0, sizeof(a));
    a.n_pairs = n_pairs; a.num_pairs = num_pairs; a.mode = best ? (int)VITVS_SELECT_ORDER : mode;
    servo_geometry(h, T, g, a);
    a.K = K; a.lambda = c.lambda;
    a.row_best = h->row_best; a.col_best = h->col_best; a.depth = Z;
    a.selection = selection; a.n_selected = n_selected;
    a.sel_stride = (mode == VITVS_SELECT_EXPLICIT) ? num_pairs : T;
    a.v_c = v_c; a.status = status; a.nn1 = h->nn1; a.nn2 = h->nn2; a.sim1 = h->sim1; a.info = h->info;
    a.sel_out = h->sel_out; a.s_uv = h->s_uv; a.feat = h->feat; a.L_ws = h->Lws; a.max_rows = c.max_rows;
    a.L_work = h->Lws + (size_t)c.max_pairs * 7 * 2 * c.max_rows;
    a.robust_iters = plan.robust_iters; a.W_ws = h->Wws;
    a.pitch_u = (double)(c.stride * c.u_max) / (double)c.img_size;
    a.pitch_v = (double)(c.stride * c.v_max) / (double)c.img_size;
    a.refine = plan.refine;
    if (plan.refine) {
        a.pitch_in = (double)c.img_size / (double)g; a.off_out = h->off_ws; a.des_shared = rf.des_shared;
        if (plan.source == RS_TABLE) a.off_in = rf.table;
        else if (plan.source == RS_GRAM) { a.G = h->gram_ws; a.sq = h->sq; }
        else { a.dn = h->dn; a.Dp = h->Dp; }
    }
    if (plan.goalz) {                           // (the entry points have checked the goal depth: check_interaction)
        a.interaction = plan.interaction; a.zgoal = h->zgoal; a.zgoal_out = h->zgoal_ws;
        a.zgoal_stride = h->n_goal_depth == 1 ? 0 : T + 1;
    }
    a.rolled = rolled;                          // (the roll search only; null: the law as it always was)
    note_law(h, n_pairs, T, plan, mode);
    int rc = 0;
    { Span sp(h, KC_SERVO, st); rc = launch_servo(plan, a, st); }
    if (rc) return set_err(h, rc, "servo launch failed (LDS budget or bad arguments)");
    return 0;
}

// The pinned staging block of the host-pointer entry points, sized for the handle's capacity and current frame geometry.
int ensure_host_stage(vitvs_handle* h) {
    const vitvs_config& c = h->cfg;
    if (h->hs.base && h->hs.frame_cap >= h->staged_frame_bytes) return 0;
    if (h->hs.base) {
        VITVS_HIP_CHECK(hipDeviceSynchronize());            // a launch may still read the previous block
        (void)hipHostFree(h->hs.base);
        h->hs = vitvs_handle::HostStage{};
        h->details_pinned = false;
        h->staged_des = nullptr;
    }
    const size_t P = c.max_pairs, fb = (h->staged_frame_bytes + 255) & ~(size_t)255;
    const size_t sel_cap = P * (size_t)(h->T > c.max_rows ? h->T : c.max_rows);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_cur = 0, o_des = o_cur + P * fb, o_depth = o_des + P * fb, o_K = o_depth + up(P * (size_t)c.u_max * c.v_max * 2),
                 o_vc = o_K + up(P * 32), o_sel = o_vc + up(P * 48), o_nsel = o_sel + up(sel_cap * 4), o_st = o_nsel + up(P * 4),
                 o_det = o_st + up(P * 4), total = o_det + up(h->det_bytes) + 256;
    void* p = nullptr;
    VITVS_HIP_CHECK(hipHostMalloc(&p, total, hipHostMallocDefault));
    memset(p, 0, total);
    unsigned char* b = static_cast<unsigned char*>(p);
    h->hs.base = b; h->hs.frame_cap = h->staged_frame_bytes;
    h->hs.cur = b + o_cur; h->hs.des = b + o_des; h->hs.depth = reinterpret_cast<uint16_t*>(b + o_depth);
    h->hs.K = reinterpret_cast<double*>(b + o_K); h->hs.vc = reinterpret_cast<double*>(b + o_vc);
    h->hs.sel = reinterpret_cast<int32_t*>(b + o_sel); h->hs.nsel = reinterpret_cast<int32_t*>(b + o_nsel);
    h->hs.status = reinterpret_cast<int32_t*>(b + o_st); h->hs.det = b + o_det;
    if (!h->host_stream) VITVS_HIP_CHECK(hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking));
    return 0;
}

// Wait for a stream the way a control loop wants it: poll (the update takes ~0.5 ms; a blocking wait adds its wake-up
// latency to every update), then hand over to the blocking wait if the device is far behind.
int wait_stream(hipStream_t st) {
    for (int i = 0; i < 200000; ++i) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) return fail_hip(e, "hipStreamQuery", __FILE__, __LINE__);
    }
    VITVS_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// Head and tail of a host-pointer law evaluation (vitvs_compute_velocity, vitvs_reselect).  The call's selection goes into the
// pinned block, where the law's kernel reads it in place
void stage_selection(vitvs_handle* h, int n_pairs, int T, int mode, const int32_t* selection, const int32_t* n_selected, int num_pairs) {
    if (mode == VITVS_SELECT_EXPLICIT) {
        memcpy(h->hs.sel, selection, (size_t)n_pairs * num_pairs * 4);
        memcpy(h->hs.nsel, n_selected, (size_t)n_pairs * 4);
    } else if (mode == VITVS_SELECT_ORDER) {
        memcpy(h->hs.sel, selection, (size_t)n_pairs * T * 4);
    }
}
// ... and behind the law: the detail block of this call -> the pinned block, one copy launch of 16-byte stores (measured: the
// law's kernel writing its ~20 small detail stores straight into host memory cost 60 us per update; one coalesced copy costs 3),
// one polled wait, v_c and status out
int finish_host_call(vitvs_handle* h, int n_pairs, double* v_c, int32_t* status) {
    const int rc = launch_copy16(h->det_block, h->hs.det, h->det_bytes, h->host_stream);
    if (rc) return set_err(h, rc, "detail copy launch failed");
    if (int w = wait_stream(h->host_stream)) return w;
    memcpy(v_c, h->hs.vc, (size_t)n_pairs * 6 * sizeof(double));
    memcpy(status, h->hs.status, (size_t)n_pairs * 4);
    return 0;
}

// What the vitvs_last_* getters start with: n_pairs against the last call, the device drained, every pair's info.  pinned: info
// comes from the pinned block of the last host-pointer call, without a HIP call (vitvs_last_details)
int last_info(vitvs_handle* h, int n_pairs, bool pinned, std::vector<int32_t>& inf) {
    if (n_pairs <= 0 || n_pairs > h->last_pairs) return set_err(h, -3, "no such pairs in the last call");
    inf.resize((size_t)n_pairs * 8);
    if (pinned) {
        memcpy(inf.data(), h->hs.det, inf.size() * 4);
        return 0;
    }
    VITVS_HIP_CHECK(hipDeviceSynchronize());
    VITVS_HIP_CHECK(hipMemcpy(inf.data(), h->info, inf.size() * 4, hipMemcpyDeviceToHost));
    return 0;
}
// The kernel writes the first n_feature_rows (info[1]) rows of a pair; the workspace rows behind them may still hold an earlier,
// larger call's values.  The copies handed out are defined everywhere: selected = -1, everything else 0.
size_t feature_rows(const vitvs_handle* h, const std::vector<int32_t>& inf, size_t b) {
    return std::min<size_t>(h->cfg.max_rows, (size_t)std::max(inf[b * 8 + 1], 0));
}
// A per-row workspace [max_pairs][max_rows][width] of the last law: copied out when that law wrote it, zeros when it did not
template <typename V>
int last_row_output(vitvs_handle* h, int n_pairs, bool written, const V* ws, size_t width, V* out) {
    DeviceScope dev(h);
    std::vector<int32_t> inf;
    if (int rc = last_info(h, n_pairs, false, inf)) return rc;
    const size_t R = h->cfg.max_rows, P = n_pairs;
    if (written) VITVS_HIP_CHECK(hipMemcpy(out, ws, P * R * width * sizeof(V), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < P; ++b) {
        const size_t n = written ? feature_rows(h, inf, b) : 0;
        memset(out + (b * R + n) * width, 0, (R - n) * width * sizeof(V));
    }
    return 0;
}

// The plan of vitvs_op_linear_variant's tile codes; slices > 0: the partial-sum form with that many K slices.
LinearPlan variant_plan(Precision p, int variant, int M, int N, int K, int slices) {
    const LinearEpi epi = slices > 0 ? EPI_PARTIAL : EPI_STORE;
    switch (variant) {
    case 0: return plan_linear(p, M, N, K, epi, slices);
    case 1: return plan_linear(p, M, N, K, epi, slices, false);
    case 2: return plan_linear(p, M, N, K, epi, slices, false, 128, 128);
    case 128: case 192: case 256: return plan_linear(p, M, N, K, epi, slices, true, 256, variant);
    case 1192: return plan_linear(p, M, N, K, epi, slices, true, 192, 128);
    case 1256: return plan_linear(p, M, N, K, epi, slices, true, 192, 256);
    default: return LinearPlan{};
    }
}

}  // namespace

extern "C" {

int vitvs_abi_version(void) { return VITVS_ABI_VERSION; }

const char* vitvs_last_error(const vitvs_handle* h) {
    if (h && !h->err.empty()) return h->err.c_str();
    return g_last_error.c_str();
}

int vitvs_tokens(const vitvs_handle* h) { return h ? h->T : -1; }
int vitvs_desc_dim(const vitvs_handle* h) { return h ? h->Dp : -1; }

int vitvs_register_tokens(const vitvs_handle* h) { return h ? h->R : -1; }

int vitvs_create(const vitvs_config* cfg, vitvs_handle** out) { return vitvs_create_ex(cfg, 0, out); }

int vitvs_create_ex(const vitvs_config* cfg, int32_t register_tokens, vitvs_handle** out) {
    if (!cfg || !out) return set_err(nullptr, -1, "null argument");
    std::string why;
    if (check_cfg(cfg, why)) return set_err(nullptr, -1, "bad config: " + why);
    if (register_tokens < 0 || register_tokens > VITVS_MAX_REGISTER_TOKENS)
        return set_err(nullptr, -1, "bad config: register_tokens must be 0 .. " + std::to_string(VITVS_MAX_REGISTER_TOKENS) +
                                        ", got " + std::to_string(register_tokens));
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return set_err(nullptr, -2, "no HIP device available");
    vitvs_handle* h = new vitvs_handle();
    h->cfg = *cfg;
    h->prec = to_prec(cfg->precision);
    (void)hipGetDevice(&h->device);
    g_current_device = h->device;
    h->wstore = std::make_shared<WeightStore>();
    h->wstore->device = h->device;
    h->grid = 1 + (cfg->img_size - cfg->patch) / cfg->stride;
    h->T = h->grid * h->grid;
    h->R = register_tokens;
    h->N = h->T + 1 + h->R;
    const int pk = 3 * cfg->patch * cfg->patch;
    h->Kp = (pk + 63) / 64 * 64;
    h->Dp = cfg->binned ? 9 * cfg->dim : cfg->dim;
    h->hidden = 4 * cfg->dim;
    h->n_img_max = 2 * cfg->max_pairs;
    h->blk.resize(cfg->blocks);
    {   // The depth pixels the law can read: the patch centre of each token in camera resolution — servo.hip token_pixel, the
        // same operations in the same precisions (fp32 centre, fp64 scale, round half to even; vitvs_v2.py:511-513, 544-549).
        // tests/test_gpu_path.py::test_host_pointer_entry_point_matches_device_entry_point holds the two restatements together at
        // 640 x 480, tests/test_gpu_geometry.py where every product is a rounding tie, where the order of the fp64 operations
        // shows, and where patch centres fall on the image's edge.
        const int g = (int)floor(sqrt((double)h->T));
        if (g * g == h->T) {
            const double scale = (double)cfg->img_size / (double)g;
            const float scale_f = (float)scale, half_f = (float)(scale / 2.0);
            const double sx = (double)cfg->u_max / (double)cfg->img_size, sy = (double)cfg->v_max / (double)cfg->img_size;
            for (int tok = 0; tok < h->T; ++tok) {
                volatile float rm = (float)(tok / g) * scale_f, cm = (float)(tok % g) * scale_f;   // (separately rounded product)
                const float r = rm + half_f, cc = cm + half_f;
                const long u = (long)rint((double)cc * sx), v = (long)rint((double)r * sy);
                if (u >= 0 && u < cfg->u_max && v >= 0 && v < cfg->v_max) h->depth_sites.push_back((int32_t)(v * cfg->u_max + u));
            }
            // and pixel (0, 0): a zero-padded row (4 <= matches < num_pairs) has the pixel (0, 0) and reads the depth there, as
            // get_depth does in the reference (vitvs_v2.py:525-553, 566-586).  It is a patch centre in no ordinary geometry; where
            // it is one, the site is listed twice, which costs one more 2-byte copy.
            if (cfg->u_max > 0 && cfg->v_max > 0) h->depth_sites.push_back(0);
        }
    }
    // hipGraph replay of the update is opt-in (VITVS_GRAPH=1, read once per handle): with kernel arguments in device
    // memory (HIP_FORCE_DEV_KERNARG=1, set by the Python package before HIP initialises) plain stream launches measured
    // 2 % FASTER than replaying the captured graph; the graph's use is a caller whose host thread cannot spare the
    // ~0.35 ms of launch calls per update.
    const char* ng = getenv("VITVS_GRAPH");
    h->use_graphs = (ng && ng[0] == '1');
    const size_t M = (size_t)h->n_img_max * h->N, D = cfg->dim, es = elem_size(h->prec);
    int rc = 0;
    unsigned char* p8 = nullptr;
#define ALLOC_BYTES(field, bytes) \
    if (!rc) { rc = dev_alloc(h, &p8, (bytes)); h->field = reinterpret_cast<decltype(h->field)>(p8); }
    ALLOC_BYTES(Ape, (size_t)h->n_img_max * h->T * h->Kp * es);
    ALLOC_BYTES(xn, M * D * es);
    ALLOC_BYTES(qkv, M * 3 * D * es);
    ALLOC_BYTES(attn, M * D * es);
    ALLOC_BYTES(hid, M * h->hidden * es);
#undef ALLOC_BYTES
    if (!rc) rc = dev_alloc(h, &h->x, M * D);
    if (!rc) rc = dev_alloc(h, &h->part, (size_t)8 * M * D);   // at most 8 split-K slices (splitk_slices)
    {   // the key-split plan depends on the image count of a call: size for the largest need over 1 .. n_img_max, under the
        // plan of a handle that runs ALONE (in_flight 1: the divided plan, the only one that needs a workspace) — whatever hint
        // the calling thread carries (vitvs_op_plan_in_flight) and whatever `in_flight` the handle is given later
        size_t f = 0, t = 0;
        for (int n = 1; n <= h->n_img_max; ++n) {
            const AttnPlan pl = plan_attention(h->prec, n, h->N, cfg->heads, /*in_flight=*/1);
            f = std::max(f, pl.ws_floats);
            t = std::max(t, pl.tickets);
        }
        if (!rc && f) rc = dev_alloc(h, &h->attn_ws.state, f);
        if (!rc && t) rc = dev_alloc(h, &h->attn_ws.tickets, t);   // dev_alloc zeroes: the tickets start at 0
    }
    h->dn_elems = (size_t)h->n_img_max * h->T * h->Dp;
    if (!rc) rc = dev_alloc(h, &h->dn, h->dn_elems);
    // the workspaces of the Gram stage (correspond.hip plan_gram): the raw token Gram [max_pairs][T][T] of the stencil form, the
    // fp16 hi / lo split of every frame's descriptors
    h->gram = plan_gram(h->prec, cfg->binned != 0, h->T, cfg->dim, cfg->max_pairs, cfg->max_pairs);
    if (!rc && h->gram.gram_floats) rc = dev_alloc(h, &h->gram_ws, h->gram.gram_floats);
    if (!rc && h->gram.split_elems) rc = dev_alloc(h, &h->dh, h->gram.split_elems);
    if (!rc) rc = dev_alloc(h, &h->sq, (size_t)h->n_img_max * h->T);

    h->best_elems = (size_t)cfg->max_pairs * h->T;
    if (!rc) rc = dev_alloc(h, &h->row_best, h->best_elems);
    if (!rc) rc = dev_alloc(h, &h->col_best, h->best_elems);
    const size_t P = cfg->max_pairs, R = cfg->max_rows;
    h->det_bytes = P * 32 + P * R * 16 + P * R * 32 + 3 * h->best_elems * 4;
    if (!rc) rc = dev_alloc(h, &h->det_block, h->det_bytes);
    if (!rc) detail_pointers(h, h->det_block);
    if (!rc) rc = dev_alloc(h, &h->sel_out, P * R);
    if (!rc) rc = dev_alloc(h, &h->Lws, 2 * P * 7 * 2 * R);   // L and e per pair, then the Jacobi SVD's working copies
    if (!rc) rc = dev_alloc(h, &h->Wws, P * R);
    if (!rc) rc = dev_alloc(h, &h->off_ws, P * R * 2);
    const size_t img_bytes = (size_t)cfg->img_size * cfg->img_size * 3;
    h->staged_frame_bytes = img_bytes;
    if (!rc) rc = dev_alloc(h, &h->st_cur, P * img_bytes);
    if (!rc) rc = dev_alloc(h, &h->st_des, P * img_bytes);
    const size_t sel_cap = P * (size_t)(h->T > cfg->max_rows ? h->T : cfg->max_rows);
    if (!rc) rc = dev_alloc(h, &h->st_sel, sel_cap);
    if (!rc) rc = dev_alloc(h, &h->st_nsel, P);
    if (!rc) rc = dev_alloc(h, &h->order_ws, h->best_elems);
    if (rc) {
        std::string msg = g_last_error;
        vitvs_destroy(h);
        return set_err(nullptr, rc, "allocation failed: " + msg);
    }
    *out = h;
    return 0;
}

void vitvs_destroy(vitvs_handle* h) {
    if (!h) return;
    DeviceScope dev(h);
    (void)hipDeviceSynchronize();               // nothing of this handle's is in flight when its graphs and memory go
    drop_graphs(h);
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->hs.base) (void)hipHostFree(h->hs.base);
    if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
    delete h;
}

int vitvs_share_weights(vitvs_handle* h, const vitvs_handle* src) {
    if (!h || !src || h == src) return set_err(h, -1, "null argument");
    const vitvs_config &a = h->cfg, &b = src->cfg;
    if (h->device != src->device) return set_err(h, -5, "handles of different devices cannot share weights");
    if (a.img_size != b.img_size || a.patch != b.patch || a.stride != b.stride || a.dim != b.dim || a.heads != b.heads ||
        a.blocks != b.blocks || a.layerscale != b.layerscale || a.precision != b.precision || h->R != src->R)
        return set_err(h, -5, "weights are shared between handles of one network (register tokens included), input geometry and precision");
    if (!h->have.empty() && !h->borrowed) return set_err(h, -5, "this handle already holds weights of its own");
    if (src->borrowed) return set_err(h, -5, "share from the handle that owns the weights");
    if (vitvs_weights_ready(src) != 0) return set_err(h, -4, "the source handle's weights are not fully loaded");
    if (!h->graphs.empty()) {                   // borrowed before, from another owner: captured updates read THOSE weights
        DeviceScope dev(h);
        VITVS_HIP_CHECK(hipDeviceSynchronize());
        drop_graphs(h);
    }
    h->blk = src->blk;
    h->pe_w = src->pe_w; h->pe_e = src->pe_e; h->pe_b = src->pe_b; h->cls = src->cls; h->pos = src->pos;
    h->reg = src->reg;
    h->have = src->have;
    h->wstore = src->wstore;                    // shared ownership: the weights outlive whichever of the two is destroyed first
    h->ready = true;
    h->borrowed = true;
    return 0;
}

int vitvs_set_tensor(vitvs_handle* h, const char* name, const float* data, int64_t numel) {
    if (!h || !name || !data) return set_err(h, -1, "null argument");
    if (h->borrowed) return set_err(h, -5, "this handle borrows its weights (vitvs_share_weights): upload to their owner");
    DeviceScope dev(h);
    const vitvs_config& c = h->cfg;
    const size_t D = c.dim, H4 = h->hidden;
    const std::string nm(name);
    auto want = [&](size_t n) -> int {
        if ((size_t)numel != n) return set_err(h, -6, nm + ": expected " + std::to_string(n) + " elements, got " + std::to_string(numel));
        return 0;
    };
    int rc = 0;
    if (nm == "patch_embed.proj.weight") {
        const size_t pk = 3 * (size_t)c.patch * c.patch;
        if ((rc = want(D * pk))) return rc;
        rc = upload_matrix(h, &h->pe_w, data, D, pk, h->Kp, &h->pe_e);
    } else if (nm == "patch_embed.proj.bias") {
        if ((rc = want(D))) return rc;
        rc = upload_f32(h, &h->pe_b, data, D);
    } else if (nm == "cls_token") {
        if ((rc = want(D))) return rc;
        rc = upload_f32(h, &h->cls, data, D);
    } else if (nm == "pos_embed") {   // cls + patches only: the register tokens carry no position embedding
        if ((rc = want((size_t)(1 + h->T) * D))) return rc;
        rc = upload_f32(h, &h->pos, data, (size_t)(1 + h->T) * D);
    } else if (nm == "register_tokens") {
        if (h->R == 0) return set_err(h, -5, "register_tokens given to a handle created without register tokens (vitvs_create_ex)");
        if ((size_t)numel != (size_t)h->R * D)
            return set_err(h, -5, "register_tokens: the handle has " + std::to_string(h->R) + " register tokens, expected " +
                                      std::to_string((size_t)h->R * D) + " elements, got " + std::to_string(numel));
        rc = upload_f32(h, &h->reg, data, (size_t)h->R * D);
    } else if (nm.rfind("blocks.", 0) == 0) {
        const size_t dot = nm.find('.', 7);
        if (dot == std::string::npos) return set_err(h, -6, "unknown tensor " + nm);
        const int i = atoi(nm.substr(7, dot - 7).c_str());
        if (i >= c.blocks) return 0;  // blocks after the descriptor layer are never run
        if (i < 0) return set_err(h, -6, "unknown tensor " + nm);
        Block& b = h->blk[i];
        const std::string leaf = nm.substr(dot + 1);
        if (leaf == "norm1.weight") { if ((rc = want(D))) return rc; rc = upload_f32(h, &b.n1w, data, D); }
        else if (leaf == "norm1.bias") { if ((rc = want(D))) return rc; rc = upload_f32(h, &b.n1b, data, D); }
        else if (leaf == "norm2.weight") { if ((rc = want(D))) return rc; rc = upload_f32(h, &b.n2w, data, D); }
        else if (leaf == "norm2.bias") { if ((rc = want(D))) return rc; rc = upload_f32(h, &b.n2b, data, D); }
        else if (leaf == "attn.qkv.weight" || leaf == "attn.qkv.bias") {
            // 16-bit modes: the q rows carry hd^-0.5 * log2(e) (kernels.h kAttnQScale), folded in here in fp32, before the one
            // rounding of the weights to 16 bits: the attention kernels then find s * scale * log2(e) in their accumulators
            const bool w = leaf == "attn.qkv.weight";
            const size_t n = w ? 3 * D * D : 3 * D, nq = w ? D * D : D;
            if ((rc = want(n))) return rc;
            std::vector<float> scaled;
            const float* src = data;
            if (plain16(h->prec)) {
                scaled.assign(data, data + n);
                for (size_t i = 0; i < nq; ++i) scaled[i] *= kAttnQScale;
                src = scaled.data();
            }
            rc = w ? upload_matrix(h, &b.qkvw, src, 3 * D, D, D, &b.qkve) : upload_f32(h, &b.qkvb, src, 3 * D);
        }
        else if (leaf == "attn.proj.weight") { if ((rc = want(D * D))) return rc; rc = upload_matrix(h, &b.projw, data, D, D, D, &b.proje); }
        else if (leaf == "attn.proj.bias") { if ((rc = want(D))) return rc; rc = upload_f32(h, &b.projb, data, D); }
        else if (leaf == "mlp.fc1.weight") { if ((rc = want(H4 * D))) return rc; rc = upload_matrix(h, &b.fc1w, data, H4, D, D, &b.fc1e); }
        else if (leaf == "mlp.fc1.bias") { if ((rc = want(H4))) return rc; rc = upload_f32(h, &b.fc1b, data, H4); }
        else if (leaf == "mlp.fc2.weight") { if ((rc = want(D * H4))) return rc; rc = upload_matrix(h, &b.fc2w, data, D, H4, H4, &b.fc2e); }
        else if (leaf == "mlp.fc2.bias") { if ((rc = want(D))) return rc; rc = upload_f32(h, &b.fc2b, data, D); }
        else if (leaf == "ls1.gamma") { if ((rc = want(D))) return rc; rc = upload_f32(h, &b.ls1, data, D); }
        else if (leaf == "ls2.gamma") { if ((rc = want(D))) return rc; rc = upload_f32(h, &b.ls2, data, D); }
        else return set_err(h, -6, "unknown tensor " + nm);
    } else if (nm == "norm.weight" || nm == "norm.bias" || nm.rfind("head.", 0) == 0 || nm == "mask_token") {
        return 0;  // final norm / head are dead work for the descriptor
    } else {
        return set_err(h, -6, "unknown tensor " + nm);
    }
    if (rc == 0) {
        h->have[nm] = true;
        h->ready = false;
    }
    return rc;
}

int vitvs_weights_ready(const vitvs_handle* hc) {
    vitvs_handle* h = const_cast<vitvs_handle*>(hc);
    if (!h) return -1;
    if (h->ready) return 0;
    std::vector<std::string> need = {"patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed"};
    if (h->R > 0) need.push_back("register_tokens");
    static const char* leaves[] = {"norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                                   "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                                   "mlp.fc2.weight", "mlp.fc2.bias"};
    for (int i = 0; i < h->cfg.blocks; ++i) {
        for (const char* l : leaves) need.push_back("blocks." + std::to_string(i) + "." + l);
        if (h->cfg.layerscale) {
            need.push_back("blocks." + std::to_string(i) + ".ls1.gamma");
            need.push_back("blocks." + std::to_string(i) + ".ls2.gamma");
        }
    }
    for (const auto& n : need)
        if (!h->have.count(n)) {
            h->err = "missing tensor " + n;
            return -4;
        }
    h->ready = true;
    return 0;
}

int vitvs_forward_tokens_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, float* tokens, void* stream) {
    if (!h || !frames || !tokens) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    hipStream_t st = dev_stream(h, stream);
    int rc = forward(h, n_frames, frames, 0, nullptr, st);
    if (rc) return rc;
    VITVS_HIP_CHECK(hipMemcpyAsync(tokens, h->x, (size_t)n_frames * h->N * h->cfg.dim * sizeof(float),
                                   hipMemcpyDeviceToDevice, st));
    return 0;
}

static int upload_table(vitvs_handle* h, const std::vector<int>& v, int** dev) {
    void* p = nullptr;
    VITVS_HIP_CHECK(hipMalloc(&p, v.size() * sizeof(int)));
    h->allocs.push_back(p);
    VITVS_HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    *dev = static_cast<int*>(p);
    return 0;
}

// ResizeArgs::rows from Pillow's bounds `yb` of the height: the most camera rows the pixels of one patch draw on.
// The patch-row build (patchify_resize_kernel) takes the camera rows of a patch from its first and last pixel row: both
// bounds of Pillow's windows grow with the output row (they do: the centre does), checked here rather than assumed (-1).
static int resize_patch_rows(const std::vector<int>& yb, int S, int patch) {
    int rows = 0;
    for (int y = 0; y + 1 < S; ++y)
        if (yb[2 * y] > yb[2 * y + 2] || yb[2 * y] + yb[2 * y + 1] > yb[2 * y + 2] + yb[2 * y + 3]) return -1;
    for (int y = 0; y + patch <= S; ++y) rows = std::max(rows, yb[2 * (y + patch - 1)] + yb[2 * (y + patch - 1) + 1] - yb[2 * y]);
    return rows;
}

// Pillow's tables for (in_h, in_w) -> img_size in `t` (a new resolution replaces the previous tables; synchronises once).
static int resize_tables(vitvs_handle* h, ResizeArgs& t, int in_h, int in_w) {
    if (in_h == t.in_h && in_w == t.in_w) return 0;
    for (const int** d : {&t.xb, &t.xk, &t.yb, &t.yk}) {
        if (*d) {
            VITVS_HIP_CHECK(hipDeviceSynchronize());   // a launch on ANY stream may still read them
            dev_free(h, (void*)*d);
            *d = nullptr;
        }
    }
    t = ResizeArgs{};
    if (in_h == 0 && in_w == 0) return 0;
    const int S = h->cfg.img_size, patch = h->cfg.patch;
    std::vector<int> xb, xk, yb, yk;
    const int ksx = resize_coefficients(in_w, S, xb, xk);
    const int ksy = resize_coefficients(in_h, S, yb, yk);
    const int rows = resize_patch_rows(yb, S, patch);
    if (rows < 0) return set_err(h, -5, "resize windows are not monotone");
    int *dxb = nullptr, *dxk = nullptr, *dyb = nullptr, *dyk = nullptr;
    if (upload_table(h, xb, &dxb) || upload_table(h, xk, &dxk) || upload_table(h, yb, &dyb) || upload_table(h, yk, &dyk))
        return set_err(h, -6, "resize table upload failed");
    t.xb = dxb; t.xk = dxk; t.yb = dyb; t.yk = dyk;
    t.in_h = in_h; t.in_w = in_w; t.ksx = ksx; t.ksy = ksy; t.rows = rows;
    return 0;
}

int vitvs_resize_frames_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, int32_t in_h, int32_t in_w,
                            uint8_t* out, void* stream) {
    if (!h || !frames || !out) return set_err(h, -1, "null argument");
    if (n_frames <= 0 || in_h <= 0 || in_w <= 0) return set_err(h, -5, "bad frame geometry");
    DeviceScope dev(h);
    if (int rc = resize_tables(h, h->rs, in_h, in_w)) return rc;
    const int rc = launch_resize_bicubic(frames, out, n_frames, in_h, in_w, h->cfg.img_size, h->rs.xb, h->rs.xk, h->rs.ksx,
                                         h->rs.yb, h->rs.yk, h->rs.ksy, as_stream(stream));
    if (rc) return set_err(h, rc, "resize launch failed");
    return 0;
}

int vitvs_set_frame_size(vitvs_handle* h, int32_t in_h, int32_t in_w) {
    if (!h) return set_err(h, -1, "null argument");
    if (in_h < 0 || in_w < 0 || (in_h == 0) != (in_w == 0)) return set_err(h, -5, "bad frame geometry");
    DeviceScope dev(h);
    if (in_h == h->cfg.img_size && in_w == h->cfg.img_size) in_h = in_w = 0;   // nothing to resize: the plain patch-row build
    if (in_h == h->fr.in_h && in_w == h->fr.in_w) return 0;
    // Everything the new geometry needs is built FIRST; the handle changes only once nothing can fail any more, so an error
    // (tables, the LDS limit of the fused resize, the staging allocation) leaves the previous geometry fully usable.
    ResizeArgs fresh{};
    if (int rc = resize_tables(h, fresh, in_h, in_w)) return rc;
    if (fresh.in_h && (size_t)fresh.rows * h->cfg.patch * 3 > 64 * 1024) {
        (void)resize_tables(h, fresh, 0, 0);
        return set_err(h, -3, "camera frame too large for the fused resize (use vitvs_resize_frames_dev)");
    }
    const size_t need = fresh.in_h ? (size_t)fresh.in_h * fresh.in_w * 3 : (size_t)h->cfg.img_size * h->cfg.img_size * 3;
    uint8_t *new_cur = nullptr, *new_des = nullptr;
    if (need > h->staged_frame_bytes) {             // host-buffer entry points stage whole frames
        const size_t P = (size_t)h->cfg.max_pairs;
        if (dev_alloc(h, &new_cur, P * need) || dev_alloc(h, &new_des, P * need)) {
            dev_free(h, new_cur);
            (void)resize_tables(h, fresh, 0, 0);
            return set_err(h, -6, "frame staging allocation failed (the previous frame geometry stays in place)");
        }
    }
    // commit.  Captured updates hold the previous tables' addresses: they go (a cached goal's tokens do not depend on the
    // geometry and stay)
    VITVS_HIP_CHECK(hipDeviceSynchronize());
    drop_graphs(h);
    (void)resize_tables(h, h->fr, 0, 0);            // frees the previous tables
    h->fr = fresh;
    h->staged_des = nullptr;                        // frames of another geometry
    if (new_cur) {
        dev_free(h, h->st_cur);
        dev_free(h, h->st_des);
        h->st_cur = new_cur;
        h->st_des = new_des;
        h->staged_frame_bytes = need;
    }
    return 0;
}

int vitvs_extract_descriptors_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, float* desc, void* stream) {
    if (!h || !frames || !desc) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    hipStream_t st = dev_stream(h, stream);
    int rc = forward(h, n_frames, frames, 0, nullptr, st);
    if (rc) return rc;
    rc = launch_descriptors(h->x, h->dn, desc, h->sq, n_frames, h->T, 1 + h->R, h->grid, h->cfg.dim, h->cfg.binned, nullptr, nullptr,
                            0, st);
    if (rc) return set_err(h, rc, "descriptor launch failed");
    return 0;
}

int vitvs_extract_facet_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, int32_t facet, float* desc,
                            void* stream) {
    if (facet < 0 || facet > 2) return set_err(h, -5, "facet must be 0 (query), 1 (key) or 2 (value)");
    return vitvs_extract_descriptors_ex_dev(h, n_frames, frames, facet, 0, 0, desc, stream);
}

int vitvs_extract_descriptors_ex_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, int32_t facet, int32_t bin,
                                     int32_t include_cls, float* desc, void* stream) {
    if (!h || !frames || !desc) return set_err(h, -1, "null argument");
    if (facet < 0 || facet > 3) return set_err(h, -5, "facet must be 0 (query), 1 (key), 2 (value) or 3 (token)");
    if (bin && include_cls)   // the reference's assertion (dinov2_extractor.py:330-331)
        return set_err(h, -5, "bin = True and include_cls = True are not supported together, set one of them False.");
    DeviceScope dev(h);
    hipStream_t st = dev_stream(h, stream);
    int rc = forward(h, n_frames, frames, 0, nullptr, st);   // the last block's qkv launch leaves its output in h->qkv
    if (rc) return rc;
    const int T = h->T, D = h->cfg.dim;
    const float* src = h->x;                                  // token facet: the residual stream itself, [n][P + T][D]
    int P = 1 + h->R;                                         // rows in front of each image's patch rows in src
    if (facet < 3) {
        // q / k / v of blocks[layer] in the reference's layout (index d * H + h), fp32, WITH the cls row (registers dropped),
        // over the residual stream's own buffer (the forward is done with it; any cached goal was dropped by the forward above)
        rc = launch_facet(h->prec, h->qkv, h->x, n_frames, T, P, h->cfg.heads, facet,
                          (facet == 0 && plain16(h->prec)) ? 1.0f / kAttnQScale : 1.0f, 1, st);   // the q rows carry the attention scale
        if (rc) return set_err(h, rc, "facet launch failed");
        P = 1;                                                // src is now [n][1 + T][D]
    }
    const size_t row_bytes = (size_t)D * sizeof(float);
    if (bin) {
        rc = launch_descriptors(src, nullptr, desc, h->sq, n_frames, T, P, h->grid, D, 1, nullptr, nullptr, 0, st);
        if (rc) return set_err(h, rc, "descriptor launch failed");
    } else if (include_cls && P == 1) {
        VITVS_HIP_CHECK(hipMemcpyAsync(desc, src, (size_t)n_frames * (T + 1) * row_bytes, hipMemcpyDeviceToDevice, st));
    } else if (include_cls) {                                 // [cls, patches]: the register rows are dropped
        VITVS_HIP_CHECK(hipMemcpy2DAsync(desc, (T + 1) * row_bytes, src, (T + P) * row_bytes, row_bytes, n_frames,
                                         hipMemcpyDeviceToDevice, st));
        VITVS_HIP_CHECK(hipMemcpy2DAsync(desc + D, (T + 1) * row_bytes, src + (size_t)P * D, (T + P) * row_bytes, T * row_bytes,
                                         n_frames, hipMemcpyDeviceToDevice, st));
    } else {
        VITVS_HIP_CHECK(hipMemcpy2DAsync(desc, T * row_bytes, src + (size_t)P * D, (T + P) * row_bytes, T * row_bytes, n_frames,
                                         hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

int vitvs_extract_saliency_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, int32_t n_heads, const int32_t* head_idxs,
                               float* saliency, void* stream) {
    if (!h || !frames || !head_idxs || !saliency) return set_err(h, -1, "null argument");
    if (n_heads <= 0 || n_heads > 16) return set_err(h, -5, "1 .. 16 heads");
    for (int i = 0; i < n_heads; ++i)
        if (head_idxs[i] < 0 || head_idxs[i] >= h->cfg.heads) return set_err(h, -5, "head index outside the model's heads");
    // (refused before the forward: a call that fails leaves the handle as it found it, a cached goal included)
    if (h->prec == PREC_X2) return set_err(h, -5, "saliency maps are not available in the f16x2 precision (use fp32)");
    DeviceScope dev(h);
    hipStream_t st = dev_stream(h, stream);
    int rc = forward(h, n_frames, frames, 0, nullptr, st);   // the last block's qkv launch leaves its output in h->qkv
    if (rc) return rc;
    rc = launch_saliency(h->prec, h->qkv, saliency, n_frames, h->T, 1 + h->R, h->cfg.heads, head_idxs, n_heads, plain16(h->prec),
                         st);
    if (rc) return set_err(h, rc, rc == -3 ? "too many tokens for the saliency kernel's LDS rows" : "saliency launch failed");
    return 0;
}

int vitvs_correspond_dev(vitvs_handle* h, int32_t T, int32_t Dp, const float* desc1, const float* desc2, int32_t* nn_1,
                         int32_t* nn_2, float* sim_1, float* S_out, void* stream) {
    if (!h || !desc1 || !desc2 || !nn_1 || !nn_2 || !sim_1) return set_err(h, -1, "null argument");
    if (T <= 0 || Dp <= 0 || Dp % 32 != 0) return set_err(h, -5, "Dp must be a positive multiple of 32");
    if ((size_t)2 * T * Dp > h->dn_elems || (size_t)T > h->best_elems)
        return set_err(h, -3, "descriptors exceed the handle's workspace");
    DeviceScope dev(h);
    hipStream_t st = dev_stream(h, stream);
    h->goal_frames = 0;                         // the descriptor workspace is overwritten
    h->details_pinned = false;                  // and the arg-max keys: nothing left for vitvs_reselect
    h->host_tables = vitvs_handle::HostTables{};
    int rc = launch_normalize_rows(desc1, h->dn, T, Dp, st);
    if (!rc) rc = launch_normalize_rows(desc2, h->dn + (size_t)T * Dp, T, Dp, st);
    if (rc) return set_err(h, rc, "normalise launch failed");
    VITVS_HIP_CHECK(hipMemsetAsync(h->row_best, 0, (size_t)T * 8, st));
    VITVS_HIP_CHECK(hipMemsetAsync(h->col_best, 0, (size_t)T * 8, st));
    const GramPlan gp = plan_gram(PREC_F32, false, T, Dp, 1, 1);   // caller's descriptors: the exact fp32 Gram in every precision
    GramOperands go;
    go.dn = h->dn; go.row_best = h->row_best; go.col_best = h->col_best;
    rc = launch_gram(gp, go, st);
    if (!rc) rc = launch_decode_best(h->row_best, h->col_best, T, nn_1, nn_2, sim_1, st);
    if (!rc && S_out) rc = launch_gram_dense(gp, h->dn, (long)T * Dp, Dp, 0, S_out, st);
    if (rc) return set_err(h, rc, "correspondence launch failed");
    return 0;
}

int vitvs_refine_dev(vitvs_handle* h, int32_t T, int32_t Dp, const float* desc1, const float* desc2, const int32_t* nn_1,
                     float* offsets, void* stream) {
    if (!h || !desc1 || !desc2 || !nn_1 || !offsets) return set_err(h, -1, "null argument");
    if (T <= 0 || Dp <= 0 || Dp % 32 != 0) return set_err(h, -5, "Dp must be a positive multiple of 32");
    const int g = (int)floor(sqrt((double)T));
    if (g * g != T) return set_err(h, -5, "token count is not a square grid");
    if ((size_t)2 * T * Dp > h->dn_elems) return set_err(h, -3, "descriptors exceed the handle's workspace");
    DeviceScope dev(h);
    hipStream_t st = dev_stream(h, stream);
    h->goal_frames = 0;                         // the descriptor workspace is overwritten
    h->host_tables = vitvs_handle::HostTables{};   // and with it what vitvs_reselect would refine from
    int rc = launch_normalize_rows(desc1, h->dn, T, Dp, st);
    if (!rc) rc = launch_normalize_rows(desc2, h->dn + (size_t)T * Dp, T, Dp, st);
    if (rc) return set_err(h, rc, "normalise launch failed");
    rc = launch_refine(h->dn, h->dn + (size_t)T * Dp, nn_1, T, g, Dp, offsets, st);
    if (rc) return set_err(h, rc, "refine launch failed");
    return 0;
}

int vitvs_servo_from_nn_dev(vitvs_handle* h, int32_t T, const int32_t* nn_1, const int32_t* nn_2, const float* sim_1,
                            const uint16_t* Z_mm, const double* K, int32_t select_mode, const int32_t* selection,
                            int32_t n_selected, int32_t num_pairs, double* v_c, int32_t* status, void* stream) {
    return vitvs_servo_from_nn_ex_dev(h, T, nn_1, nn_2, sim_1, Z_mm, K, select_mode, selection, n_selected, num_pairs, nullptr, v_c,
                                      status, stream);
}

int vitvs_servo_from_nn_ex_dev(vitvs_handle* h, int32_t T, const int32_t* nn_1, const int32_t* nn_2, const float* sim_1,
                               const uint16_t* Z_mm, const double* K, int32_t select_mode, const int32_t* selection,
                               int32_t n_selected, int32_t num_pairs, const float* offsets, double* v_c, int32_t* status,
                               void* stream) {
    if (!h || !nn_1 || !nn_2 || !sim_1 || !K || !v_c || !status) return set_err(h, -1, "null argument");
    if ((size_t)T > h->best_elems) return set_err(h, -3, "T exceeds the handle's workspace");
    const int np = call_num_pairs(h, num_pairs);
    if (int rc = check_selection(h, T, select_mode, selection, h->st_nsel, np)) return rc;
    if (int rc = check_interaction(h, 1, T)) return rc;
    DeviceScope dev(h);
    hipStream_t st = dev_stream(h, stream);
    h->details_pinned = false;
    int rc = launch_encode_best(nn_1, nn_2, sim_1, T, h->row_best, h->col_best, st);
    if (rc) return set_err(h, rc, "encode launch failed");
    VITVS_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->st_nsel), n_selected, 1, st));
    return run_servo(h, 1, T, Z_mm, K, select_mode, np, selection, h->st_nsel, v_c, status, st, RefineSpec{offsets});
}

// One update = forward of the call's image list (desired frames first, then current frames) + the tail
// (descriptors when binned, Gram + arg-max, control law), all on the caller's stream.
struct UpdateArgs {
    int32_t n_pairs, des_shared, select_mode, num_pairs;
    const uint8_t *I_cur, *I_des;
    const uint16_t* Z_mm;
    const double* K;
    const int32_t *selection, *n_selected;
    double* v_c;
    int32_t* status;
    // host-pointer entry point: the caller's depth image (late_src) is copied into the pinned staging block on the HOST, after the
    // forward's launches have been enqueued and before the law's launch (the only kernel that reads it): off the critical path
    // Only the pixels the law can ask for are copied: it looks the depth up at the patch CENTRE of a current-frame token
    // (vitvs_v2.py:511-553, 566-586), i.e. at one of T fixed sites of the image (linear pixel indices, the handle's depth_sites),
    // or, for a zero-padded row (4 <= matches < num_pairs), at pixel (0, 0), which is one of the sites for that reason: T + 1
    // 2-byte gathers stand for the 614 KB image.  A law whose plan reads the depth anywhere (a refined match can lie on any
    // pixel) has the whole image copied; one that does not read it (L(s*, Z*)) none of it.
    const uint16_t* late_src = nullptr;
    ServoPlan law;                              // the law of this update (velocity_update)
};
static inline void late_inputs(vitvs_handle* h, const UpdateArgs& u) {
    if (!u.late_src || !u.law.reads_depth) return;
    const size_t stride = (size_t)h->cfg.u_max * h->cfg.v_max;   // pixels per depth image
    for (int b = 0; b < u.n_pairs; ++b) {
        const uint16_t* src = u.late_src + (size_t)b * stride;
        uint16_t* dst = h->hs.depth + (size_t)b * stride;
        if (u.law.depth_anywhere) { memcpy(dst, src, stride * sizeof(uint16_t)); continue; }
        for (const int32_t site : h->depth_sites) dst[site] = src[site];
    }
}

// The first half of an update: the forward of the call's frames and the correspondence stage, up to the packed arg-max keys of
// its n_pairs pairs in h->row_best / col_best (of `u` it reads the frames, n_pairs and des_shared)
static int enqueue_forward_gram(vitvs_handle* h, const UpdateArgs& u, hipStream_t st) {
    const int n_des = u.des_shared ? 1 : u.n_pairs, n_img = n_des + u.n_pairs;
    h->desc_keys = u.n_pairs * h->T;
    // cached goal: only the current frames (images n_des .. n_img - 1 of the call's list) go through the network
    int rc = u.I_des ? forward_chain(h, 0, n_img, n_des, u.I_des, u.I_cur, h->part, st)
                     : forward_chain(h, n_des, u.n_pairs, n_des, nullptr, u.I_cur, h->part, st);
    h->desc_keys = -1;
    if (rc) return rc;
    // the forward's last launch wrote what the plan asked of it (GramEmit) and cleared the arg-max keys
    const GramPlan gp = plan_gram(h->prec, h->cfg.binned != 0, h->T, h->cfg.dim, u.n_pairs, h->cfg.max_pairs);
    GramOperands go;
    go.x = h->x; go.P = 1 + h->R; go.dn = h->dn; go.dh = h->dh; go.G = h->gram_ws; go.sq = h->sq; go.grid = h->grid;
    go.des_shared = u.des_shared ? 1 : 0; go.row_best = h->row_best; go.col_best = h->col_best;
    for (int i = 0; i < gp.n_steps && !rc; ++i) {
        Span sp(h, kGramStepClass[gp.steps[i]], st);
        rc = launch_gram_step(gp, i, go, st);
    }
    if (rc) return set_err(h, rc, "correspondence launch failed");
    return 0;
}

static int enqueue_update(vitvs_handle* h, const UpdateArgs& u, hipStream_t st) {
    const RefineSpec rf{nullptr, h->subpatch != 0, u.des_shared ? 1 : 0};
    if (int rc = enqueue_forward_gram(h, u, st)) return rc;
    late_inputs(h, u);
    return run_servo(h, u.n_pairs, h->T, u.Z_mm, u.K, u.select_mode, u.num_pairs, u.selection, u.n_selected, u.v_c, u.status, st, rf);
}

// VITVS_GRAPH=1: the update is captured once per argument tuple and replayed.  The selection array is the one argument
// a control loop changes every update (a fresh visiting order), so it is not part of the key: the graph reads the
// handle's own copy (st_sel / st_nsel), refreshed by two small device-to-device copies ahead of each replay.
static int replay_update(vitvs_handle* h, UpdateArgs u, hipStream_t st) {
    const size_t sel_elems = u.select_mode == VITVS_SELECT_EXPLICIT ? (size_t)u.n_pairs * u.num_pairs
                             : (u.select_mode == VITVS_SELECT_ORDER ? (size_t)u.n_pairs * h->T : 0);
    if (sel_elems && u.selection && u.selection != h->st_sel)
        VITVS_HIP_CHECK(hipMemcpyAsync(h->st_sel, u.selection, sel_elems * 4, hipMemcpyDefault, st));
    if (u.select_mode == VITVS_SELECT_EXPLICIT && u.n_selected && u.n_selected != h->st_nsel)
        VITVS_HIP_CHECK(hipMemcpyAsync(h->st_nsel, u.n_selected, (size_t)u.n_pairs * 4, hipMemcpyDefault, st));
    late_inputs(h, u);                          // a replay has no seam to do this later: before the launch
    if (u.selection) u.selection = h->st_sel;
    if (u.n_selected) u.n_selected = h->st_nsel;
    const std::vector<uintptr_t> key = {(uintptr_t)u.n_pairs, (uintptr_t)u.I_cur, (uintptr_t)u.I_des, (uintptr_t)u.des_shared,
                                        (uintptr_t)u.Z_mm, (uintptr_t)u.K, (uintptr_t)u.select_mode, (uintptr_t)u.num_pairs,
                                        (uintptr_t)(u.selection != nullptr), (uintptr_t)(u.n_selected != nullptr),
                                        (uintptr_t)u.v_c, (uintptr_t)u.status, (uintptr_t)h->fr.in_h, (uintptr_t)h->fr.in_w,
                                        (uintptr_t)h->info};
    vitvs_handle::GraphEntry* ge = nullptr;
    for (auto& g : h->graphs)
        if (g.key == key) ge = &g;
    if (!ge) {
        if (h->graphs.size() >= 32) {  // evict the least recently used entry (8 cameras sharing a pipeline slot = 8 keys)
            size_t victim = 0;
            for (size_t i = 1; i < h->graphs.size(); ++i)
                if (h->graphs[i].last_use < h->graphs[victim].last_use) victim = i;
            VITVS_HIP_CHECK(hipDeviceSynchronize());   // the victim's last replay may still be queued on a stream of the caller's
            if (h->graphs[victim].exec) (void)hipGraphExecDestroy(h->graphs[victim].exec);
            if (h->graphs[victim].graph) (void)hipGraphDestroy(h->graphs[victim].graph);
            h->graphs.erase(h->graphs.begin() + victim);
        }
        vitvs_handle::GraphEntry fresh;
        fresh.key = key;
        VITVS_HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        UpdateArgs cap = u;
        cap.late_src = nullptr;                 // (done above)
        const int rc = enqueue_update(h, cap, st);
        hipError_t e = hipStreamEndCapture(st, &fresh.graph);
        if (rc) {
            if (fresh.graph) (void)hipGraphDestroy(fresh.graph);
            return rc;
        }
        if (e != hipSuccess) return fail_hip(e, "hipStreamEndCapture", __FILE__, __LINE__);
        e = hipGraphInstantiate(&fresh.exec, fresh.graph, nullptr, nullptr, 0);
        if (e != hipSuccess) {
            (void)hipGraphDestroy(fresh.graph);
            return fail_hip(e, "hipGraphInstantiate", __FILE__, __LINE__);
        }
        h->graphs.push_back(fresh);
        ge = &h->graphs.back();
    }
    ge->last_use = ++h->graph_clock;
    note_law(h, u.n_pairs, h->T, u.law, u.select_mode);   // (a replay runs none of run_servo's host code)
    VITVS_HIP_CHECK(hipGraphLaunch(ge->exec, st));
    return 0;
}

int vitvs_set_goal_dev(vitvs_handle* h, int32_t n_goal, const uint8_t* I_des, void* stream) {
    if (!h || !I_des) return set_err(h, -1, "null argument");
    if (n_goal <= 0 || n_goal > h->cfg.max_pairs) return set_err(h, -3, "n_goal exceeds max_pairs");
    DeviceScope dev(h);
    if (vitvs_weights_ready(h) != 0) return set_err(h, -4, "weights not fully loaded: " + h->err);
    hipStream_t st = dev_stream(h, stream);
    h->desc_keys = 0;                           // plain descriptors come out of the forward's last launch; no keys to clear
    int rc = forward_chain(h, 0, n_goal, n_goal, I_des, nullptr, h->part, st);
    h->desc_keys = -1;
    if (rc) return rc;
    h->goal_frames = n_goal;                    // (binned: the goal's token norms stay in h->sq, its token rows in h->x)
    return 0;
}

int vitvs_set_goal(vitvs_handle* h, int32_t n_goal, const uint8_t* I_des) {
    if (!h || !I_des) return set_err(h, -1, "null argument");
    if (n_goal <= 0 || n_goal > h->cfg.max_pairs) return set_err(h, -3, "n_goal exceeds max_pairs");
    DeviceScope dev(h);
    if (int rc = ensure_host_stage(h)) return rc;
    if (int rc = order_behind_dev(h)) return rc;
    const size_t img = frame_bytes(h);
    memcpy(h->hs.des, I_des, n_goal * img);
    h->staged_des = nullptr;
    int rc = launch_copy16(h->hs.des, h->st_des, n_goal * img, h->host_stream);
    if (rc) return set_err(h, rc, "frame staging launch failed");
    rc = vitvs_set_goal_dev(h, n_goal, h->st_des, h->host_stream);
    if (rc) return rc;
    return wait_stream(h->host_stream);
}

// Validation + dispatch shared by the device-pointer and the host-pointer entry points (`u` carries the latter's late input).
static int velocity_update(vitvs_handle* h, UpdateArgs u, hipStream_t st) {
    if (!u.I_cur || !u.K || !u.v_c || !u.status) return set_err(h, -1, "null argument");   // I_des NULL: the cached goal
    if (u.n_pairs <= 0 || u.n_pairs > h->cfg.max_pairs) return set_err(h, -3, "n_pairs exceeds max_pairs");
    u.num_pairs = call_num_pairs(h, u.num_pairs);
    if (int rc = check_selection(h, h->T, u.select_mode, u.selection, u.n_selected, u.num_pairs)) return rc;
    if (vitvs_weights_ready(h) != 0) return set_err(h, -4, "weights not fully loaded: " + h->err);
    if (int rc = check_interaction(h, u.n_pairs, h->T)) return rc;
    if (int rc = plan_law(h, h->T, RefineSpec{nullptr, h->subpatch != 0, u.des_shared ? 1 : 0}, u.law)) return rc;
    // The goal cache is host-side state of the handle: it is checked and invalidated here, on every call, and never
    // inside the body that a hipGraph captures (a replay runs none of the body's host code).
    if (!u.I_des && h->goal_frames != (u.des_shared ? 1 : u.n_pairs))
        return set_err(h, -5, "I_des is NULL and no goal of this shape is cached (vitvs_set_goal_dev)");
    if (u.I_des) h->goal_frames = 0;            // the call forwards goal frames of its own over the cached rows
    h->details_pinned = false;                  // the detail block on the device is about to change
    h->host_tables = vitvs_handle::HostTables{};
    if (h->use_graphs && !h->timing && st != nullptr) return replay_update(h, u, st);
    return enqueue_update(h, u, st);
}

int vitvs_compute_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                               int32_t des_shared, const uint16_t* Z_mm, const double* K, int32_t select_mode,
                               const int32_t* selection, const int32_t* n_selected, int32_t num_pairs, double* v_c,
                               int32_t* status, void* stream) {
    if (!h) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    UpdateArgs u{n_pairs, des_shared, select_mode, num_pairs, I_cur, I_des, Z_mm, K, selection, n_selected, v_c, status};
    return velocity_update(h, u, dev_stream(h, stream));
}

// The reference's seam as it is called (vitvs_v2.py:464-523, 588-632: numpy arrays in, a numpy twist out).  Per call: the
// frames, intrinsics and selection are copied into the handle's pinned block by memcpy; the frames go on to device memory
// in one short launch on the update's stream; the forward is enqueued; THEN the depth image is copied (host) — the law's
// kernel is the only reader, it is enqueued last and reads the <= max_rows pixels it needs in place; v_c, status and the
// feature rows come back through the pinned block; one polled wait.
int vitvs_compute_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des,
                           int32_t des_shared, const uint16_t* Z_mm, const double* K, int32_t select_mode,
                           const int32_t* selection, const int32_t* n_selected, int32_t num_pairs, double* v_c,
                           int32_t* status) {
    if (!h || !I_cur || !K || !v_c || !status) return set_err(h, -1, "null argument");   // I_des NULL: the cached goal
    if (n_pairs <= 0 || n_pairs > h->cfg.max_pairs) return set_err(h, -3, "n_pairs exceeds max_pairs");
    const int np = call_num_pairs(h, num_pairs);
    if (int rc = check_selection(h, h->T, select_mode, selection, n_selected, np)) return rc;   // (before the frames are staged)
    if (int rc = check_interaction(h, n_pairs, h->T)) return rc;
    DeviceScope dev(h);
    if (int rc = ensure_host_stage(h)) return rc;
    if (int rc = order_behind_dev(h)) return rc;
    vitvs_handle::HostStage& hs = h->hs;
    hipStream_t st = h->host_stream;
    const size_t img = frame_bytes(h), n_des = des_shared ? 1 : n_pairs;
    memcpy(hs.cur, I_cur, n_pairs * img);
    int rc = launch_copy16(hs.cur, h->st_cur, n_pairs * img, st);
    // option "reuse_goal_frames": a control loop's goal image does not change — while the caller passes the same address (and
    // count, and geometry) the goal frames staged by the previous call are still in device memory and are forwarded again as they are
    const bool goal_staged = h->reuse_goal && I_des && I_des == h->staged_des && n_des * img == h->staged_des_bytes;
    if (!rc && I_des && !goal_staged) {
        memcpy(hs.des, I_des, n_des * img);
        h->staged_des = nullptr;                // st_des changes hands; the address counts as staged once the copy is enqueued
        rc = launch_copy16(hs.des, h->st_des, n_des * img, st);
        if (!rc) {
            h->staged_des = I_des;
            h->staged_des_bytes = n_des * img;
        }
    }
    if (rc) {
        h->staged_des = nullptr;
        return set_err(h, rc, "frame staging launch failed");
    }
    memcpy(hs.K, K, (size_t)n_pairs * 4 * sizeof(double));
    stage_selection(h, n_pairs, h->T, select_mode, selection, n_selected, np);
    UpdateArgs u{n_pairs, des_shared, select_mode, np, h->st_cur, I_des ? h->st_des : nullptr, Z_mm ? hs.depth : nullptr, hs.K,
                 hs.sel, hs.nsel, hs.vc, hs.status, Z_mm};
    rc = velocity_update(h, u, st);
    if (!rc) rc = finish_host_call(h, n_pairs, v_c, status);
    if (rc) {
        h->staged_des = nullptr;                // a call that failed vouches for nothing in st_des
        return rc;
    }
    h->details_pinned = true;
    h->host_tables = vitvs_handle::HostTables{n_pairs, h->T, Z_mm != nullptr, des_shared ? 1 : 0};
    return 0;
}

// The reference draws its feature tokens on the HOST, between the correspondence and the law (find_correspondences_batch:
// sort + torch.randperm, vitvs_v2.py:127-141): a host-pointer call gives the tables (vitvs_last_details serves nn_1 / nn_2 /
// sim_1 of a host-pointer call from host memory), the caller draws, and this entry point runs the law again for that draw on
// what the call left in the handle — the arg-max keys on the device, the depth image and intrinsics in the pinned block: one
// short launch, no forward, no staging.
int vitvs_reselect(vitvs_handle* h, int32_t select_mode, const int32_t* selection, const int32_t* n_selected, int32_t num_pairs,
                   double* v_c, int32_t* status) {
    if (!h || !v_c || !status) return set_err(h, -1, "null argument");
    if (!h->details_pinned || h->host_tables.n_pairs <= 0 || !h->hs.base)
        return set_err(h, -5, "vitvs_reselect follows a host-pointer velocity call on the same handle (vitvs_compute_velocity)");
    const int n_pairs = h->host_tables.n_pairs, T = h->host_tables.T;
    const int np = call_num_pairs(h, num_pairs);
    if (int rc = check_selection(h, T, select_mode, selection, n_selected, np)) return rc;
    if (int rc = check_interaction(h, n_pairs, T)) return rc;
    DeviceScope dev(h);
    if (int rc = order_behind_dev(h)) return rc;
    vitvs_handle::HostStage& hs = h->hs;
    stage_selection(h, n_pairs, T, select_mode, selection, n_selected, np);
    const int rc = run_servo(h, n_pairs, T, h->host_tables.have_depth ? hs.depth : nullptr, hs.K, select_mode, np, hs.sel, hs.nsel,
                             hs.vc, hs.status, h->host_stream, RefineSpec{nullptr, h->subpatch != 0, h->host_tables.des_shared});
    return rc ? rc : finish_host_call(h, n_pairs, v_c, status);
}

int vitvs_last_details(vitvs_handle* h, int32_t n_pairs, int32_t* nn_1, int32_t* nn_2, float* sim_1, int32_t* info,
                       int32_t* selected, int32_t* s_uv, double* feat, double* L) {
    if (!h) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    const size_t T = h->last_T, R = h->cfg.max_rows, P = n_pairs;
    // after a host-pointer call the feature rows are already in host memory (the handle's pinned block): a caller that asks
    // for those alone (the reference's detect_features return value: s_uv*, s_uv, the selected similarities) costs no HIP call
    const bool pinned = h->details_pinned;
    std::vector<int32_t> inf;
    if (int rc = last_info(h, n_pairs, pinned, inf)) return rc;
    if (pinned && (selected || L)) VITVS_HIP_CHECK(hipDeviceSynchronize());
    // a part of the detail block: from its image in the pinned block (same layout, detail_pointers) or from the device
    auto part = [&](void* dst, const void* src, size_t bytes) -> int {
        if (dst && pinned) memcpy(dst, h->hs.det + (static_cast<const unsigned char*>(src) - h->det_block), bytes);
        else if (dst) VITVS_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return 0;
    };
    int rc = part(nn_1, h->nn1, P * T * 4);
    if (!rc) rc = part(nn_2, h->nn2, P * T * 4);
    if (!rc) rc = part(sim_1, h->sim1, P * T * 4);
    if (!rc) rc = part(s_uv, h->s_uv, P * R * 16);
    if (!rc) rc = part(feat, h->feat, P * R * 32);
    if (rc) return rc;
    if (info) memcpy(info, inf.data(), P * 8 * 4);
    if (selected) VITVS_HIP_CHECK(hipMemcpy(selected, h->sel_out, P * R * 4, hipMemcpyDeviceToHost));
    if (L) VITVS_HIP_CHECK(hipMemcpy(L, h->Lws, P * 7 * 2 * R * 8, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < P; ++b) {
        const size_t n = feature_rows(h, inf, b);
        for (size_t k = n; k < R; ++k) {
            if (selected) selected[b * R + k] = -1;
            if (s_uv) memset(s_uv + (b * R + k) * 4, 0, 16);
            if (feat) memset(feat + (b * R + k) * 4, 0, 32);
        }
        if (L)
            for (size_t c = 0; c < 7; ++c) memset(L + (b * 7 + c) * 2 * R + 2 * n, 0, (2 * R - 2 * n) * 8);
    }
    return 0;
}

// An option that captured updates depend on: those of the control law (they hold the previous law's kernel and arguments) and
// the tile plan hint.  staged_depth: the pinned depth image of the last host-pointer call holds only what the previous setting
// reads, so vitvs_reselect may not build on it
static int set_captured_option(vitvs_handle* h, int& option, int value, bool staged_depth) {
    if (value == option) return 0;
    DeviceScope dev(h);
    VITVS_HIP_CHECK(hipDeviceSynchronize());
    drop_graphs(h);
    option = value;
    if (staged_depth) {
        h->details_pinned = false;
        h->host_tables = vitvs_handle::HostTables{};
    }
    return 0;
}

int vitvs_set_option(vitvs_handle* h, const char* name, int64_t value) {
    if (!h || !name) return set_err(h, -1, "null argument");
    const std::string nm(name);
    if (nm == "graph_replay") {
        if (value != 0 && value != 1) return set_err(h, -5, "graph_replay takes 0 or 1");
        h->use_graphs = value == 1;
        return 0;
    }
    if (nm == "reuse_goal_frames") {
        if (value != 0 && value != 1) return set_err(h, -5, "reuse_goal_frames takes 0 or 1");
        h->reuse_goal = value == 1;
        h->staged_des = nullptr;
        return 0;
    }
    if (nm == "in_flight") {
        if (value < 1 || value > 64) return set_err(h, -5, "in_flight takes 1 .. 64");
        return set_captured_option(h, h->in_flight, (int)value, false);   // captured updates hold the previous plan's launches
    }
    const struct { const char* name; int* option; int lo, hi; bool staged_depth; const char* takes; } law[] = {
        {"robust_law", &h->robust_iters, 0, 16, false, "robust_law takes 0 (the plain law) or 1 .. 16 re-weightings"},
        {"subpatch", &h->subpatch, 0, 1, true, "subpatch takes 0 (patch centres) or 1 (refined matches)"},
        {"interaction", &h->interaction, IL_CURRENT, IL_MEAN, true, "interaction takes 0 (current, L(s, Z)), 1 (desired, L(s*, Z*)) or 2 (their mean)"},
        {"select_cells", &h->select_cells, 1, 16, false, "select_cells takes 1 .. 16 image cells per side (selection mode BEST)"}};
    for (const auto& o : law) {
        if (nm != o.name) continue;
        if (value < o.lo || value > o.hi) return set_err(h, -5, o.takes);
        return set_captured_option(h, *o.option, (int)value, o.staged_depth);
    }
    return set_err(h, -5, "unknown option " + nm);
}

int vitvs_set_goal_depth_dev(vitvs_handle* h, int32_t n_goal, const uint16_t* Z_des_mm, void* stream) {
    if (!h || (n_goal > 0 && !Z_des_mm)) return set_err(h, -1, "null argument");
    if (n_goal < 0 || n_goal > h->cfg.max_pairs) return set_err(h, -3, "n_goal exceeds max_pairs");
    if (h->grid * h->grid != h->T) return set_err(h, -5, "token count is not a square grid");
    DeviceScope dev(h);
    if (n_goal != h->n_goal_depth) {            // the first set, a clear, another pairing: captured updates hold the table's
        VITVS_HIP_CHECK(hipDeviceSynchronize());  // address and its stride between pairs.  Set-up, not the call path.
        drop_graphs(h);
        if (n_goal && !h->zgoal) {
            int rc = dev_alloc(h, &h->zgoal, (size_t)h->cfg.max_pairs * (h->T + 1));
            if (!rc) rc = dev_alloc(h, &h->zgoal_ws, (size_t)h->cfg.max_pairs * h->cfg.max_rows);
            if (rc) return set_err(h, rc, "goal depth allocation failed");
        }
        h->n_goal_depth = n_goal;
    }
    if (!n_goal) return 0;
    ServoArgs geom;
    memset(&geom, 0, sizeof(geom));
    servo_geometry(h, h->T, h->grid, geom);
    // same count as before: the table is rewritten in place, in stream order — captured updates read the new goal
    const int rc = launch_goal_depth(geom, Z_des_mm, n_goal, h->zgoal, dev_stream(h, stream));
    if (rc) return set_err(h, rc, "goal depth launch failed");
    return 0;
}

int vitvs_set_goal_depth(vitvs_handle* h, int32_t n_goal, const uint16_t* Z_des_mm) {
    if (!h || (n_goal > 0 && !Z_des_mm)) return set_err(h, -1, "null argument");
    if (n_goal < 0 || n_goal > h->cfg.max_pairs) return set_err(h, -3, "n_goal exceeds max_pairs");
    if (n_goal == 0) return vitvs_set_goal_depth_dev(h, 0, nullptr, nullptr);
    DeviceScope dev(h);
    // a _dev velocity call made earlier may still be waiting on a stream the null stream does not order (a non-blocking one):
    // it reads the table as it was when it was made
    if (int rc = order_behind_dev(h)) return rc;
    // set-up: a device copy of the images for the one launch that reads them, released again behind it
    const size_t bytes = (size_t)n_goal * h->cfg.u_max * h->cfg.v_max * sizeof(uint16_t);
    void* tmp = nullptr;
    VITVS_HIP_CHECK(hipMalloc(&tmp, bytes));
    hipError_t e = hipMemcpy(tmp, Z_des_mm, bytes, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? vitvs_set_goal_depth_dev(h, n_goal, static_cast<const uint16_t*>(tmp), nullptr)
                             : fail_hip(e, "hipMemcpy", __FILE__, __LINE__);
    if (!rc) {
        e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = fail_hip(e, "hipDeviceSynchronize", __FILE__, __LINE__);
        else h->dev_pending = false;            // (the _dev form above ran on the null stream: drained with everything else)
    }
    (void)hipFree(tmp);
    return rc;
}

// --- the rig law ---------------------------------------------------------------------------------
static int rig_prepare(vitvs_handle* h, int n_cams, bool robust_form = false) {
    if (int rc = follows_velocity_call(h, "vitvs_rig_velocity", "n_cams", n_cams)) return rc;
    if (!robust_form && (h->last_law.robust || h->robust_iters))
        return set_err(h, -5, "the rig law does not combine with option robust_law (one median over all cameras' residuals: "
                              "vitvs_rig_robust_velocity)");
    if (n_cams > kRigMaxCams) return set_err(h, -5, "the rig law takes at most " + std::to_string(kRigMaxCams) + " cameras");
    const vitvs_config& c = h->cfg;
    RigIo io = rig_io(c.max_pairs, c.max_rows);
    // (sized for the robust form, a third block of stacked rows, whichever form comes first: allocated once)
    return law_blocks(h, "rig", &h->rig_ws, rig_robust_scratch_bytes(c.max_pairs, 2 * c.max_rows), &h->rig_io,
                      io_place(io_list(io), nullptr));
}

int vitvs_rig_velocity_dev(vitvs_handle* h, int32_t n_cams, const double* cVr, const int32_t* status, double* v_rig,
                           int32_t* rig_status, int32_t* rig_info, double* normal, void* stream) {
    if (!h || !cVr || !status || !v_rig || !rig_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = rig_prepare(h, n_cams)) return rc;
    RigArgs a;
    memset(&a, 0, sizeof(a));
    a.n_cams = n_cams; a.status = status; a.rows = h->info + 5; a.rows_stride = 8;
    a.L = h->Lws; a.ld = 2 * h->cfg.max_rows; a.W = cVr; a.lambda = h->cfg.lambda;
    rig_carve(h->rig_ws, h->cfg.max_pairs, a.ld, a);
    a.v_rig = v_rig; a.rig_status = rig_status; a.rig_info = rig_info; a.normal = normal;
    const int rc = launch_rig(a, dev_stream(h, stream));
    return rc ? set_err(h, rc, "rig law launch failed") : 0;
}

int vitvs_rig_velocity(vitvs_handle* h, int32_t n_cams, const double* cVr, const int32_t* status, double* v_rig,
                       int32_t* rig_status, int32_t* rig_info, double* normal) {
    if (!h || !cVr || !status || !v_rig || !rig_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = rig_prepare(h, n_cams)) return rc;
    RigIo io = rig_io(h->cfg.max_pairs, h->cfg.max_rows, n_cams, cVr, status, nullptr, v_rig, rig_status, rig_info, normal);
    return host_call(h, io_list(io), h->rig_io, [&](hipStream_t st) {
        return vitvs_rig_velocity_dev(h, n_cams, io.cVr.f64(), io.status.i32(), io.v_rig.f64(), io.rig_status.i32(),
                                      io.rig_info.i32(), io.normal.f64(), st);
    });
}

// --- the robust rig law ----------------------------------------------------------------------------
int vitvs_rig_robust_velocity_dev(vitvs_handle* h, int32_t n_cams, const double* cVr, const int32_t* status, const double* K,
                                  int32_t n_iter, double* v_rig, int32_t* rig_status, int32_t* rig_info, double* normal,
                                  double* weights, double* sigma, void* stream) {
    if (!h || !cVr || !status || !K || !v_rig || !rig_status) return set_err(h, -1, "null argument");
    if (n_iter < 1 || n_iter > 16) return set_err(h, -2, "n_iter is 1 .. 16");
    DeviceScope dev(h);
    if (int rc = rig_prepare(h, n_cams, true)) return rc;
    const vitvs_config& c = h->cfg;
    RigRobustArgs ra;
    memset(&ra, 0, sizeof(ra));
    RigArgs& a = ra.r;
    a.n_cams = n_cams; a.status = status; a.rows = h->info + 5; a.rows_stride = 8;
    a.L = h->Lws; a.ld = 2 * c.max_rows; a.W = cVr; a.lambda = c.lambda;
    rig_robust_carve(h->rig_ws, c.max_pairs, a.ld, ra);
    a.v_rig = v_rig; a.rig_status = rig_status; a.rig_info = rig_info; a.normal = normal;
    ra.live = h->info + 3; ra.live_stride = 8; ra.K = K; ra.n_iter = n_iter;
    ra.pitch_u = token_pitch(c, c.u_max); ra.pitch_v = token_pitch(c, c.v_max);
    ra.weights = weights; ra.weights_stride = c.max_rows; ra.sigma = sigma;
    const int rc = launch_rig_robust(ra, dev_stream(h, stream));
    if (rc == -3) return set_err(h, rc, "the robust rig law keeps two doubles per feature pair of the rig in LDS: n_cams * max_rows is too large");
    return rc ? set_err(h, rc, "robust rig law launch failed") : 0;
}

int vitvs_rig_robust_velocity(vitvs_handle* h, int32_t n_cams, const double* cVr, const int32_t* status, const double* K,
                              int32_t n_iter, double* v_rig, int32_t* rig_status, int32_t* rig_info, double* normal,
                              double* weights, double* sigma) {
    if (!h || !cVr || !status || !K || !v_rig || !rig_status) return set_err(h, -1, "null argument");
    if (n_iter < 1 || n_iter > 16) return set_err(h, -2, "n_iter is 1 .. 16");
    DeviceScope dev(h);
    if (int rc = rig_prepare(h, n_cams, true)) return rc;
    RigIo io = rig_io(h->cfg.max_pairs, h->cfg.max_rows, n_cams, cVr, status, K, v_rig, rig_status, rig_info, normal, weights, sigma);
    return host_call(h, io_list(io), h->rig_io, [&](hipStream_t st) {
        return vitvs_rig_robust_velocity_dev(h, n_cams, io.cVr.f64(), io.status.i32(), io.K.f64(), n_iter, io.v_rig.f64(),
                                             io.rig_status.i32(), io.rig_info.i32(), io.normal.f64(), io.weights.f64(),
                                             io.sigma.f64(), st);
    });
}

// --- the pose law --------------------------------------------------------------------------------
static int pose_prepare(vitvs_handle* h, int n_pairs, int n_iter, int n_hyp = 0) {
    if (n_iter < 0 || n_iter > 16) return set_err(h, -2, "n_iter is 0 .. 16");
    if (n_hyp < 0 || n_hyp > 4096) return set_err(h, -2, "n_hyp is 0 .. 4096");
    if (int rc = follows_velocity_call(h, "vitvs_pose_velocity", "n_pairs", n_pairs)) return rc;
    if (!h->n_goal_depth) return set_err(h, -5, "the pose law needs a goal depth (vitvs_set_goal_depth_dev)");
    if (h->last_T != h->T) return set_err(h, -5, "the goal depth table is laid out for the handle's own token grid");
    if (h->n_goal_depth != n_pairs && h->n_goal_depth != 1)
        return set_err(h, -5, "the goal depth holds " + std::to_string(h->n_goal_depth) + " images: one per pair, or one for all");
    if (h->last_law.interaction == IL_DESIRED)
        return set_err(h, -5, "the pose law needs the current depth: with option interaction at 1 the feature rows hold Z*, not Z");
    const vitvs_config& c = h->cfg;
    PosePlan pl;
    if (plan_pose(c.max_rows, n_iter, n_hyp, &pl))
        return set_err(h, -3, "the robust pose law keeps two doubles per feature row in LDS, its consensus start half a double more (one "
                              "and a half without re-weightings): max_rows is too large");
    PoseIo io = pose_io(c.max_pairs, c.max_rows);
    return law_blocks(h, "pose", &h->pose_ws, pose_scratch_bytes(c.max_pairs, c.max_rows), &h->pose_io, io_place(io_list(io), nullptr));
}

int vitvs_pose_consensus_velocity_dev(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, int32_t n_iter,
                                      int32_t n_hyp, uint32_t seed, double* v_pose, int32_t* pose_status, double* pose,
                                      int32_t* pose_info, double* weights, double* sigma, void* stream) {
    if (!h || !K || !status || !v_pose || !pose_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = pose_prepare(h, n_pairs, n_iter, n_hyp)) return rc;
    PoseArgs a;
    memset(&a, 0, sizeof(a));
    a.n_pairs = n_pairs; a.ld = h->cfg.max_rows; a.status = status; a.ws = reinterpret_cast<double*>(h->pose_ws);
    camera_law_state(h, K, n_iter, a);
    goal_depth_state(h, a);
    a.n_hyp = n_hyp; a.seed = seed;
    a.v_pose = v_pose; a.pose_status = pose_status; a.pose = pose; a.pose_info = pose_info; a.weights = weights; a.sigma = sigma;
    const int rc = launch_pose(a, dev_stream(h, stream));
    return rc ? set_err(h, rc, "pose law launch failed") : 0;
}

int vitvs_pose_velocity_dev(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, int32_t n_iter, double* v_pose,
                            int32_t* pose_status, double* pose, int32_t* pose_info, double* weights, double* sigma, void* stream) {
    return vitvs_pose_consensus_velocity_dev(h, n_pairs, K, status, n_iter, 0, 0, v_pose, pose_status, pose, pose_info, weights, sigma,
                                             stream);
}

int vitvs_pose_consensus_velocity(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, int32_t n_iter,
                                  int32_t n_hyp, uint32_t seed, double* v_pose, int32_t* pose_status, double* pose, int32_t* pose_info,
                                  double* weights, double* sigma) {
    if (!h || !K || !status || !v_pose || !pose_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = pose_prepare(h, n_pairs, n_iter, n_hyp)) return rc;
    PoseIo io = pose_io(h->cfg.max_pairs, h->cfg.max_rows, n_pairs, K, status, v_pose, pose_status, pose, pose_info, weights, sigma);
    return host_call(h, io_list(io), h->pose_io, [&](hipStream_t st) {
        return vitvs_pose_consensus_velocity_dev(h, n_pairs, io.K.f64(), io.status.i32(), n_iter, n_hyp, seed, io.v_pose.f64(),
                                                 io.pose_status.i32(), io.pose.f64(), io.pose_info.i32(), io.weights.f64(),
                                                 io.sigma.f64(), st);
    });
}

int vitvs_pose_velocity(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, int32_t n_iter, double* v_pose,
                        int32_t* pose_status, double* pose, int32_t* pose_info, double* weights, double* sigma) {
    return vitvs_pose_consensus_velocity(h, n_pairs, K, status, n_iter, 0, 0, v_pose, pose_status, pose, pose_info, weights, sigma);
}

// --- the homography law --------------------------------------------------------------------------
static int homography_prepare(vitvs_handle* h, int n_pairs, double depth_scale, int n_iter, int n_hyp = 0) {
    if (n_iter < 0 || n_iter > 16) return set_err(h, -2, "n_iter is 0 .. 16");
    if (n_hyp < 0 || n_hyp > 4096) return set_err(h, -2, "n_hyp is 0 .. 4096");
    if (!(depth_scale > 0.0) || !std::isfinite(depth_scale)) return set_err(h, -2, "depth_scale is a positive, finite length in metres");
    if (int rc = follows_velocity_call(h, "vitvs_homography_velocity", "n_pairs", n_pairs)) return rc;
    const vitvs_config& c = h->cfg;
    HomographyPlan pl;
    if (plan_homography(c.max_rows, n_iter, n_hyp, &pl))
        return set_err(h, -3, "the robust homography law keeps two doubles per feature row in LDS, its consensus start half a double "
                              "more: max_rows is too large");
    HomographyIo io = homography_io(c.max_pairs, c.max_rows);
    return law_blocks(h, "homography", &h->hom_ws, homography_scratch_bytes(c.max_pairs, c.max_rows), &h->hom_io,
                      io_place(io_list(io), nullptr));
}

int vitvs_homography_consensus_velocity_dev(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status,
                                            double depth_scale, int32_t n_iter, int32_t n_hyp, uint32_t seed, double* v_h,
                                            int32_t* h_status, double* H, int32_t* h_info, double* weights, double* sigma,
                                            void* stream) {
    if (!h || !K || !status || !v_h || !h_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = homography_prepare(h, n_pairs, depth_scale, n_iter, n_hyp)) return rc;
    HomographyArgs a;
    memset(&a, 0, sizeof(a));
    a.n_pairs = n_pairs; a.ld = h->cfg.max_rows; a.status = status; a.ws = reinterpret_cast<double*>(h->hom_ws);
    camera_law_state(h, K, n_iter, a);
    a.depth_scale = depth_scale; a.n_hyp = n_hyp; a.seed = seed;
    a.v_h = v_h; a.h_status = h_status; a.H = H; a.h_info = h_info; a.weights = weights; a.sigma = sigma;
    const int rc = launch_homography(a, dev_stream(h, stream));
    return rc ? set_err(h, rc, "homography law launch failed") : 0;
}

int vitvs_homography_velocity_dev(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, double depth_scale,
                                  int32_t n_iter, double* v_h, int32_t* h_status, double* H, int32_t* h_info, double* weights,
                                  double* sigma, void* stream) {
    return vitvs_homography_consensus_velocity_dev(h, n_pairs, K, status, depth_scale, n_iter, 0, 0, v_h, h_status, H, h_info, weights,
                                                   sigma, stream);
}

int vitvs_homography_consensus_velocity(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, double depth_scale,
                                        int32_t n_iter, int32_t n_hyp, uint32_t seed, double* v_h, int32_t* h_status, double* H,
                                        int32_t* h_info, double* weights, double* sigma) {
    if (!h || !K || !status || !v_h || !h_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = homography_prepare(h, n_pairs, depth_scale, n_iter, n_hyp)) return rc;
    HomographyIo io = homography_io(h->cfg.max_pairs, h->cfg.max_rows, n_pairs, K, status, v_h, h_status, H, h_info, weights, sigma);
    return host_call(h, io_list(io), h->hom_io, [&](hipStream_t st) {
        return vitvs_homography_consensus_velocity_dev(h, n_pairs, io.K.f64(), io.status.i32(), depth_scale, n_iter, n_hyp, seed,
                                                       io.v_h.f64(), io.h_status.i32(), io.H.f64(), io.h_info.i32(),
                                                       io.weights.f64(), io.sigma.f64(), st);
    });
}

int vitvs_homography_velocity(vitvs_handle* h, int32_t n_pairs, const double* K, const int32_t* status, double depth_scale,
                              int32_t n_iter, double* v_h, int32_t* h_status, double* H, int32_t* h_info, double* weights,
                              double* sigma) {
    return vitvs_homography_consensus_velocity(h, n_pairs, K, status, depth_scale, n_iter, 0, 0, v_h, h_status, H, h_info, weights,
                                               sigma);
}

// --- the pose rig law ----------------------------------------------------------------------------
static int pose_rig_prepare(vitvs_handle* h, int n_cams, int n_iter) {
    if (n_cams < 1) return set_err(h, -2, "n_cams is at least 1");
    if (int rc = pose_prepare(h, n_cams, n_iter)) return rc;     // valid exactly where the pose law is, n_cams == last_pairs
    const vitvs_config& c = h->cfg;
    PoseRigPlan pl;
    if (plan_pose_rig(n_cams, c.max_rows, n_iter, &pl))
        return set_err(h, -3, "the robust pose rig law keeps two doubles per feature row of the rig in LDS: n_cams * max_rows is too large");
    PoseRigIo io = pose_rig_io(c.max_pairs, c.max_rows);
    return law_blocks(h, "pose rig", &h->pose_rig_ws, pose_rig_scratch_bytes(c.max_pairs, c.max_rows), &h->pose_rig_io,
                      io_place(io_list(io), nullptr));
}

int vitvs_pose_rig_velocity_dev(vitvs_handle* h, int32_t n_cams, const double* rTc, const double* K, const int32_t* status,
                                int32_t n_iter, double* v_rig, int32_t* rig_status, double* pose, int32_t* rig_info, double* moments,
                                double* weights, double* sigma, void* stream) {
    if (!h || !rTc || !K || !status || !v_rig || !rig_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = pose_rig_prepare(h, n_cams, n_iter)) return rc;
    PoseRigArgs a;
    memset(&a, 0, sizeof(a));
    a.n_cams = n_cams; a.ld = h->cfg.max_rows; a.status = status; a.rTc = rTc; a.ws = reinterpret_cast<double*>(h->pose_rig_ws);
    camera_law_state(h, K, n_iter, a);
    goal_depth_state(h, a);
    a.v_rig = v_rig; a.rig_status = rig_status; a.pose = pose; a.rig_info = rig_info; a.moments = moments;
    a.weights = weights; a.sigma = sigma;
    const int rc = launch_pose_rig(a, dev_stream(h, stream));
    return rc ? set_err(h, rc, "pose rig law launch failed") : 0;
}

int vitvs_pose_rig_velocity(vitvs_handle* h, int32_t n_cams, const double* rTc, const double* K, const int32_t* status, int32_t n_iter,
                            double* v_rig, int32_t* rig_status, double* pose, int32_t* rig_info, double* moments, double* weights,
                            double* sigma) {
    if (!h || !rTc || !K || !status || !v_rig || !rig_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = pose_rig_prepare(h, n_cams, n_iter)) return rc;
    PoseRigIo io = pose_rig_io(h->cfg.max_pairs, h->cfg.max_rows, n_cams, rTc, K, status, v_rig, rig_status, pose, rig_info, moments,
                               weights, sigma);
    return host_call(h, io_list(io), h->pose_rig_io, [&](hipStream_t st) {
        return vitvs_pose_rig_velocity_dev(h, n_cams, io.rTc.f64(), io.K.f64(), io.status.i32(), n_iter, io.v_rig.f64(),
                                           io.rig_status.i32(), io.pose.f64(), io.rig_info.i32(), io.moments.f64(), io.weights.f64(),
                                           io.sigma.f64(), st);
    });
}

// --- the roll search -----------------------------------------------------------------------------
int vitvs_quarter_turns_dev(vitvs_handle* h, int32_t n_frames, const uint8_t* frames, uint8_t* out, void* stream) {
    if (!h || !frames || !out) return set_err(h, -1, "null argument");
    if (n_frames <= 0) return set_err(h, -5, "n_frames is at least 1");
    DeviceScope dev(h);
    int rc = 0;
    { Span sp(h, KC_PATCHIFY, as_stream(stream)); rc = launch_quarter_turns(frames, out, n_frames, h->cfg.img_size, as_stream(stream)); }
    return rc ? set_err(h, rc, "quarter-turn launch failed") : 0;
}

// What a roll call asks of the handle and of the call's selection, before anything is staged or enqueued; the first call allocates
static int roll_prepare(vitvs_handle* h, int select_mode, const int32_t* selection, const int32_t* n_selected, int np) {
    const vitvs_config& c = h->cfg;
    if (c.max_pairs < 4) return set_err(h, -3, "the roll search matches four turned copies at once: max_pairs must be at least 4");
    if (h->subpatch) return set_err(h, -5, "the roll search does not combine with option subpatch (the offsets would have to be turned too)");
    if (h->fr.in_h) return set_err(h, -5, "the roll search takes frames at img_size x img_size: clear vitvs_set_frame_size first");
    if ((c.img_size - c.patch) % c.stride != 0 || h->grid * h->grid != h->T)
        return set_err(h, -5, "the token grid is not symmetric under a quarter turn ((img_size - patch) % stride != 0)");
    if (int rc = check_selection(h, h->T, select_mode, selection, n_selected, np)) return rc;
    if (vitvs_weights_ready(h) != 0) return set_err(h, -4, "weights not fully loaded: " + h->err);
    if (int rc = check_interaction(h, 1, h->T)) return rc;
    const size_t frame = (size_t)c.img_size * c.img_size * 3;
    RollIo io = roll_io(h->T, c.max_rows, frame, (size_t)c.u_max * c.v_max);
    return law_blocks(h, "roll search", &h->roll_ws, 256 + 4 * frame, &h->roll_io, io_place(io_list(io), nullptr));
}

int vitvs_roll_velocity_dev(vitvs_handle* h, const uint8_t* I_cur, const uint8_t* I_des, const uint16_t* Z_mm, const double* K,
                            int32_t select_mode, const int32_t* selection, const int32_t* n_selected, int32_t num_pairs, double* v_c,
                            int32_t* status, int32_t* roll_info, double* scores, void* stream) {
    if (!h || !I_cur || !K || !v_c || !status || !roll_info || !scores) return set_err(h, -1, "null argument");   // I_des NULL: the cached goal
    const int np = call_num_pairs(h, num_pairs);
    DeviceScope dev(h);
    if (int rc = roll_prepare(h, select_mode, selection, n_selected, np)) return rc;
    ServoPlan law;
    if (int rc = plan_law(h, h->T, RefineSpec{}, law)) return rc;
    if (!I_des && h->goal_frames != 1) return set_err(h, -5, "I_des is NULL and no goal of one image is cached (vitvs_set_goal_dev)");
    if (I_des) h->goal_frames = 0;              // the call forwards a goal frame of its own over the cached rows
    h->details_pinned = false;
    h->host_tables = vitvs_handle::HostTables{};
    hipStream_t st = dev_stream(h, stream);
    int32_t* rolled = reinterpret_cast<int32_t*>(h->roll_ws);
    uint8_t* turned = h->roll_ws + 256;
    int rc = 0;
    { Span sp(h, KC_PATCHIFY, st); rc = launch_quarter_turns(I_cur, turned, 1, h->cfg.img_size, st); }
    if (rc) return set_err(h, rc, "quarter-turn launch failed");
    // the four copies against the one goal: the forward and the correspondence stage of a des_shared call of four pairs
    UpdateArgs u{4, 1, select_mode, np, turned, I_des, Z_mm, K, selection, n_selected, v_c, status};
    if ((rc = enqueue_forward_gram(h, u, st))) return rc;
    { Span sp(h, KC_SERVO, st); rc = launch_roll_pick(h->row_best, h->col_best, h->T, h->grid, scores, roll_info, rolled, st); }
    if (rc) return set_err(h, rc, "roll pick launch failed");
    // the law for ONE pair on pair 0's keys: the winner's tables in the unturned frame
    return run_servo(h, 1, h->T, Z_mm, K, select_mode, np, selection, n_selected, v_c, status, st, RefineSpec{}, rolled);
}

int vitvs_roll_velocity(vitvs_handle* h, const uint8_t* I_cur, const uint8_t* I_des, const uint16_t* Z_mm, const double* K,
                        int32_t select_mode, const int32_t* selection, const int32_t* n_selected, int32_t num_pairs, double* v_c,
                        int32_t* status, int32_t* roll_info, double* scores) {
    if (!h || !I_cur || !K || !v_c || !status || !roll_info || !scores) return set_err(h, -1, "null argument");
    const int np = call_num_pairs(h, num_pairs);
    DeviceScope dev(h);
    if (int rc = roll_prepare(h, select_mode, selection, n_selected, np)) return rc;
    const vitvs_config& c = h->cfg;
    const size_t n_sel = select_mode == VITVS_SELECT_EXPLICIT ? (size_t)np : select_mode == VITVS_SELECT_ORDER ? (size_t)h->T : 0;
    RollIo io = roll_io(h->T, c.max_rows, (size_t)c.img_size * c.img_size * 3, (size_t)c.u_max * c.v_max, n_sel, K,
                        n_sel ? selection : nullptr, select_mode == VITVS_SELECT_EXPLICIT ? n_selected : nullptr, Z_mm, I_cur, I_des,
                        v_c, status, roll_info, scores);
    return host_call(h, io_list(io), h->roll_io, [&](hipStream_t st) {
        return vitvs_roll_velocity_dev(h, io.I_cur.dev, I_des ? io.I_des.dev : nullptr,
                                       Z_mm ? reinterpret_cast<const uint16_t*>(io.Z.dev) : nullptr, io.K.f64(), select_mode,
                                       io.selection.i32(), io.n_selected.i32(), np, io.v_c.f64(), io.status.i32(), io.roll_info.i32(),
                                       io.scores.f64(), st);
    });
}

// --- the photometric law -------------------------------------------------------------------------
// What a photometric call asks of its arguments, before anything is staged or enqueued; the first call allocates the law's two
// blocks: the band partials at max_pairs pairs of the most bands a frame can have (4096 rows in bands of one: 1 MiB per pair), so
// no later call allocates, and PhotometricIo at max_pairs frames of v_max x u_max.  As with the other laws, calls on different
// streams of one handle share the partials: one call in flight per handle.
constexpr size_t kPhotoWsPerPair = (size_t)4096 * 32 * sizeof(double);
static int photometric_check(vitvs_handle* h, int n_pairs, int height, int width, int level, int interaction, double depth_scale,
                             double mu, double lambda, bool host_form) {
    const vitvs_config& c = h->cfg;
    if (n_pairs < 1 || n_pairs > c.max_pairs) return set_err(h, -2, "n_pairs is 1 .. max_pairs");
    if (level < 0 || level > 3) return set_err(h, -2, "level is 0 .. 3");
    if (interaction != IL_CURRENT && interaction != IL_DESIRED) return set_err(h, -2, "interaction is 0 (current) or 1 (desired)");
    if (!std::isfinite(mu) || !std::isfinite(lambda) || !std::isfinite(depth_scale))
        return set_err(h, -2, "mu, lambda and depth_scale are finite");
    if (mu < 0.0) return set_err(h, -2, "mu is not negative");
    if (height < 1 || width < 1 || height > 4096 || width > 4096) return set_err(h, -2, "height and width are 1 .. 4096");
    if ((height >> level) < 3 || (width >> level) < 3) return set_err(h, -2, "the pooled image is at least 3 x 3 pixels");
    const size_t px_max = (size_t)c.u_max * c.v_max;
    if (host_form && (size_t)height * width > px_max)
        return set_err(h, -2, "the host-pointer form stages frames of at most v_max x u_max pixels");
    PhotometricPlan pl;
    if (int rc = plan_photometric(height, width, level, c.max_pairs, &pl)) return set_err(h, rc, "no photometric plan");
    if (pl.ws_bytes > (size_t)c.max_pairs * kPhotoWsPerPair) return set_err(h, -3, "the photometric plan has more bands than the workspace");
    return 0;
}
static int photometric_prepare(vitvs_handle* h, int n_pairs, int height, int width, int level, int interaction, double depth_scale,
                               double mu, double lambda, bool host_form) {
    if (int rc = photometric_check(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, host_form)) return rc;
    const vitvs_config& c = h->cfg;
    const size_t px_max = (size_t)c.u_max * c.v_max;
    PhotometricIo io = photometric_io(c.max_pairs, px_max * 3, px_max);
    return law_blocks(h, "photometric", &h->photo_ws, (size_t)c.max_pairs * kPhotoWsPerPair, &h->photo_io, io_place(io_list(io), nullptr));
}

int vitvs_photometric_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                   int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                                   int32_t interaction, double mu, double lambda, double* v_p, int32_t* p_status, double* normal,
                                   int32_t* p_info, void* stream) {
    if (!h || !I_cur || !I_des || !K || !v_p || !p_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_prepare(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, false)) return rc;
    PhotometricArgs a;
    memset(&a, 0, sizeof(a));
    a.n_pairs = n_pairs; a.height = height; a.width = width; a.level = level; a.interaction = interaction;
    a.I_cur = I_cur; a.I_des = I_des; a.Z_mm = Z_mm; a.depth_scale = depth_scale; a.K = K; a.mu = mu; a.lambda = lambda;
    a.ws = reinterpret_cast<double*>(h->photo_ws);
    a.v_p = v_p; a.p_status = p_status; a.normal = normal; a.p_info = p_info;
    const int rc = launch_photometric(a, dev_stream(h, stream));
    return rc ? set_err(h, rc, "photometric law launch failed") : 0;
}

int vitvs_photometric_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                               int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                               int32_t interaction, double mu, double lambda, double* v_p, int32_t* p_status, double* normal,
                               int32_t* p_info) {
    if (!h || !I_cur || !I_des || !K || !v_p || !p_status) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_prepare(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, true)) return rc;
    const vitvs_config& c = h->cfg;
    const size_t px_max = (size_t)c.u_max * c.v_max, px = (size_t)height * width;
    PhotometricIo io = photometric_io(c.max_pairs, px_max * 3, px_max, n_pairs, px * 3, px, K, Z_mm, I_cur, I_des, v_p, p_status, normal,
                                      p_info);
    return host_call(h, io_list(io), h->photo_io, [&](hipStream_t st) {
        return vitvs_photometric_velocity_dev(h, n_pairs, io.I_cur.dev, io.I_des.dev, height, width,
                                              Z_mm ? reinterpret_cast<const uint16_t*>(io.Z.dev) : nullptr, depth_scale, io.K.f64(), level,
                                              interaction, mu, lambda, io.v_p.f64(), io.p_status.i32(), normal ? io.normal.f64() : nullptr,
                                              p_info ? io.p_info.i32() : nullptr, st);
    });
}

// --- the robust photometric law ------------------------------------------------------------------
// Everything the plain law refuses, and the three parameters of its own; the first call allocates the law's own two blocks (the
// 48-double band partials at 4096 bands, a histogram and a state per pair of max_pairs; PhotometricRobustIo), zeroed, so no later
// call allocates.
static int photometric_robust_prepare(vitvs_handle* h, int n_pairs, int height, int width, int level, int interaction,
                                      double depth_scale, double mu, double lambda, int illumination, int robust_iterations,
                                      double sigma_min, bool host_form) {
    if (int rc = photometric_check(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, host_form)) return rc;
    if (illumination != 0 && illumination != 1) return set_err(h, -2, "illumination is 0 or 1");
    if (robust_iterations < 0 || robust_iterations > 4) return set_err(h, -2, "robust_iterations is 0 .. 4");
    if (!std::isfinite(sigma_min) || !(sigma_min > 0.0)) return set_err(h, -2, "sigma_min is finite and > 0");
    const vitvs_config& c = h->cfg;
    const size_t px_max = (size_t)c.u_max * c.v_max;
    PhotometricRobustIo io = photometric_robust_io(c.max_pairs, px_max * 3, px_max);
    return law_blocks(h, "robust photometric", &h->photo_robust_ws, photometric_robust_ws_bytes(c.max_pairs), &h->photo_robust_io,
                      io_place(io_list(io), nullptr));
}

int vitvs_photometric_robust_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                          int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                                          int32_t interaction, double mu, double lambda, int32_t illumination,
                                          int32_t robust_iterations, double sigma_min, double* v_p, int32_t* p_status, double* p_robust,
                                          double* normal45, int32_t* p_info, void* stream) {
    if (!h || !I_cur || !I_des || !K || !v_p || !p_status || !p_robust) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_robust_prepare(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, illumination,
                                            robust_iterations, sigma_min, false))
        return rc;
    PhotometricRobustArgs ra;
    memset(&ra, 0, sizeof(ra));
    PhotometricArgs& a = ra.p;
    a.n_pairs = n_pairs; a.height = height; a.width = width; a.level = level; a.interaction = interaction;
    a.I_cur = I_cur; a.I_des = I_des; a.Z_mm = Z_mm; a.depth_scale = depth_scale; a.K = K; a.mu = mu; a.lambda = lambda;
    a.v_p = v_p; a.p_status = p_status; a.p_info = p_info;
    ra.illumination = illumination; ra.iterations = robust_iterations; ra.sigma_min = sigma_min;
    ra.p_robust = p_robust; ra.normal45 = normal45;
    const int rc = launch_photometric_robust(ra, h->photo_robust_ws, h->cfg.max_pairs, dev_stream(h, stream));
    return rc ? set_err(h, rc, "robust photometric law launch failed") : 0;
}

int vitvs_photometric_robust_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                      int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                                      int32_t interaction, double mu, double lambda, int32_t illumination, int32_t robust_iterations,
                                      double sigma_min, double* v_p, int32_t* p_status, double* p_robust, double* normal45,
                                      int32_t* p_info) {
    if (!h || !I_cur || !I_des || !K || !v_p || !p_status || !p_robust) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_robust_prepare(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, illumination,
                                            robust_iterations, sigma_min, true))
        return rc;
    const vitvs_config& c = h->cfg;
    const size_t px_max = (size_t)c.u_max * c.v_max, px = (size_t)height * width;
    PhotometricRobustIo io = photometric_robust_io(c.max_pairs, px_max * 3, px_max, n_pairs, px * 3, px, K, Z_mm, I_cur, I_des, v_p,
                                                   p_status, p_robust, normal45, p_info);
    return host_call(h, io_list(io), h->photo_robust_io, [&](hipStream_t st) {
        return vitvs_photometric_robust_velocity_dev(h, n_pairs, io.I_cur.dev, io.I_des.dev, height, width,
                                                     Z_mm ? reinterpret_cast<const uint16_t*>(io.Z.dev) : nullptr, depth_scale,
                                                     io.K.f64(), level, interaction, mu, lambda, illumination, robust_iterations,
                                                     sigma_min, io.v_p.f64(), io.p_status.i32(), io.p_robust.f64(),
                                                     normal45 ? io.normal45.f64() : nullptr, p_info ? io.p_info.i32() : nullptr, st);
    });
}

// --- the photometric rig law ----------------------------------------------------------------------
// The robust photometric law's refusals with the cameras in the place of the pairs, and at most kPhotoRigMaxCams of them.  It
// runs in the robust law's workspace block (allocated here if no robust call came first); only PhotometricRigIo is its own.
static int photometric_rig_prepare(vitvs_handle* h, int n_cams, int height, int width, int level, int interaction, double depth_scale,
                                   double mu, double lambda, int illumination, int robust_iterations, double sigma_min, bool host_form) {
    const vitvs_config& c = h->cfg;
    if (n_cams < 1 || n_cams > c.max_pairs || n_cams > kPhotoRigMaxCams)
        return set_err(h, -2, "n_cams is 1 .. min(max_pairs, " + std::to_string(kPhotoRigMaxCams) + ")");
    if (int rc = photometric_robust_prepare(h, n_cams, height, width, level, interaction, depth_scale, mu, lambda, illumination,
                                            robust_iterations, sigma_min, host_form))
        return rc;
    if (h->photo_rig_io) return 0;
    const size_t px_max = (size_t)c.u_max * c.v_max;
    PhotometricRigIo io = photometric_rig_io(c.max_pairs, px_max * 3, px_max);
    if (int rc = dev_alloc(h, &h->photo_rig_io, io_place(io_list(io), nullptr)))
        return set_err(h, rc, "photometric rig workspace allocation failed");
    VITVS_HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

int vitvs_photometric_rig_velocity_dev(vitvs_handle* h, int32_t n_cams, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                       int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, const double* cVr,
                                       const int32_t* live, int32_t level, int32_t interaction, double mu, double lambda,
                                       int32_t illumination, int32_t robust_iterations, double sigma_min, double* v_rig,
                                       int32_t* rig_status, double* p_robust, double* normal45, double* rig_normal, int32_t* rig_info,
                                       void* stream) {
    if (!h || !I_cur || !I_des || !K || !cVr || !v_rig || !rig_status || !p_robust) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_rig_prepare(h, n_cams, height, width, level, interaction, depth_scale, mu, lambda, illumination,
                                         robust_iterations, sigma_min, false))
        return rc;
    PhotometricRigArgs ga;
    memset(&ga, 0, sizeof(ga));
    PhotometricRobustArgs& ra = ga.r;
    PhotometricArgs& a = ra.p;
    a.n_pairs = n_cams; a.height = height; a.width = width; a.level = level; a.interaction = interaction;
    a.I_cur = I_cur; a.I_des = I_des; a.Z_mm = Z_mm; a.depth_scale = depth_scale; a.K = K; a.mu = mu; a.lambda = lambda;
    a.v_p = v_rig; a.p_status = rig_status; a.p_info = rig_info;
    ra.illumination = illumination; ra.iterations = robust_iterations; ra.sigma_min = sigma_min;
    ra.p_robust = p_robust; ra.normal45 = normal45;
    ga.cVr = cVr; ga.live = live; ga.rig_normal = rig_normal;
    const int rc = launch_photometric_rig(ga, h->photo_robust_ws, h->cfg.max_pairs, dev_stream(h, stream));
    return rc ? set_err(h, rc, "photometric rig law launch failed") : 0;
}

int vitvs_photometric_rig_velocity(vitvs_handle* h, int32_t n_cams, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                   int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, const double* cVr,
                                   const int32_t* live, int32_t level, int32_t interaction, double mu, double lambda,
                                   int32_t illumination, int32_t robust_iterations, double sigma_min, double* v_rig, int32_t* rig_status,
                                   double* p_robust, double* normal45, double* rig_normal, int32_t* rig_info) {
    if (!h || !I_cur || !I_des || !K || !cVr || !v_rig || !rig_status || !p_robust) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_rig_prepare(h, n_cams, height, width, level, interaction, depth_scale, mu, lambda, illumination,
                                         robust_iterations, sigma_min, true))
        return rc;
    const vitvs_config& c = h->cfg;
    const size_t px_max = (size_t)c.u_max * c.v_max, px = (size_t)height * width;
    PhotometricRigIo io = photometric_rig_io(c.max_pairs, px_max * 3, px_max, n_cams, px * 3, px, K, cVr, live, Z_mm, I_cur, I_des, v_rig,
                                             rig_status, p_robust, normal45, rig_normal, rig_info);
    return host_call(h, io_list(io), h->photo_rig_io, [&](hipStream_t st) {
        return vitvs_photometric_rig_velocity_dev(h, n_cams, io.I_cur.dev, io.I_des.dev, height, width,
                                                  Z_mm ? reinterpret_cast<const uint16_t*>(io.Z.dev) : nullptr, depth_scale, io.K.f64(),
                                                  io.cVr.f64(), live ? io.live.i32() : nullptr, level, interaction, mu, lambda,
                                                  illumination, robust_iterations, sigma_min, io.v_rig.f64(), io.rig_status.i32(),
                                                  io.p_robust.f64(), normal45 ? io.normal45.f64() : nullptr,
                                                  rig_normal ? io.rig_normal.f64() : nullptr, rig_info ? io.rig_info.i32() : nullptr, st);
    });
}

// --- the tile photometric law ---------------------------------------------------------------------
// Everything the robust law refuses (the lighting model is always on), and the tile grid; the first call allocates the law's own
// two blocks (the 48-double segment partials at 4096 segment rows of 8 tile columns, a histogram and a state per pair of max_pairs;
// PhotometricTileIo at 64 tiles per pair), zeroed, so no later call allocates.
static int photometric_tile_prepare(vitvs_handle* h, int n_pairs, int height, int width, int level, int interaction, double depth_scale,
                                    double mu, double lambda, int tiles_y, int tiles_x, int robust_iterations, double sigma_min,
                                    bool host_form) {
    if (int rc = photometric_check(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, host_form)) return rc;
    if (tiles_y < 1 || tiles_y > 8 || tiles_x < 1 || tiles_x > 8) return set_err(h, -2, "tiles_y and tiles_x are 1 .. 8");
    if (tiles_y > (height >> level) || tiles_x > (width >> level))
        return set_err(h, -2, "tiles_y and tiles_x are at most the pooled image's sides");
    if (robust_iterations < 0 || robust_iterations > 4) return set_err(h, -2, "robust_iterations is 0 .. 4");
    if (!std::isfinite(sigma_min) || !(sigma_min > 0.0)) return set_err(h, -2, "sigma_min is finite and > 0");
    const vitvs_config& c = h->cfg;
    PhotometricTilePlan pl;
    if (int rc = plan_photometric_tiles(height, width, level, tiles_y, tiles_x, c.max_pairs, &pl)) return set_err(h, rc, "no tile photometric plan");
    const size_t px_max = (size_t)c.u_max * c.v_max;
    PhotometricTileIo io = photometric_tile_io(c.max_pairs, px_max * 3, px_max);
    return law_blocks(h, "tile photometric", &h->photo_tile_ws, photometric_tile_ws_bytes(c.max_pairs), &h->photo_tile_io,
                      io_place(io_list(io), nullptr));
}

int vitvs_photometric_tile_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                        int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                                        int32_t interaction, double mu, double lambda, int32_t tiles_y, int32_t tiles_x,
                                        int32_t robust_iterations, double sigma_min, double* v_p, int32_t* p_status, double* p_robust,
                                        double* p_tiles, double* normal45, int32_t* p_info, void* stream) {
    if (!h || !I_cur || !I_des || !K || !v_p || !p_status || !p_robust || !p_tiles) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_tile_prepare(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, tiles_y, tiles_x,
                                          robust_iterations, sigma_min, false))
        return rc;
    PhotometricTileArgs ta;
    memset(&ta, 0, sizeof(ta));
    PhotometricRobustArgs& ra = ta.r;
    PhotometricArgs& a = ra.p;
    a.n_pairs = n_pairs; a.height = height; a.width = width; a.level = level; a.interaction = interaction;
    a.I_cur = I_cur; a.I_des = I_des; a.Z_mm = Z_mm; a.depth_scale = depth_scale; a.K = K; a.mu = mu; a.lambda = lambda;
    a.v_p = v_p; a.p_status = p_status; a.p_info = p_info;
    ra.illumination = 1; ra.iterations = robust_iterations; ra.sigma_min = sigma_min;
    ra.p_robust = p_robust; ra.normal45 = normal45;
    ta.tiles_y = tiles_y; ta.tiles_x = tiles_x; ta.p_tiles = p_tiles;
    const int rc = launch_photometric_tiles(ta, h->photo_tile_ws, h->cfg.max_pairs, dev_stream(h, stream));
    return rc ? set_err(h, rc, "tile photometric law launch failed") : 0;
}

int vitvs_photometric_tile_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                    int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                                    int32_t interaction, double mu, double lambda, int32_t tiles_y, int32_t tiles_x,
                                    int32_t robust_iterations, double sigma_min, double* v_p, int32_t* p_status, double* p_robust,
                                    double* p_tiles, double* normal45, int32_t* p_info) {
    if (!h || !I_cur || !I_des || !K || !v_p || !p_status || !p_robust || !p_tiles) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_tile_prepare(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, tiles_y, tiles_x,
                                          robust_iterations, sigma_min, true))
        return rc;
    const vitvs_config& c = h->cfg;
    const size_t px_max = (size_t)c.u_max * c.v_max, px = (size_t)height * width, T = (size_t)tiles_y * tiles_x;
    PhotometricTileIo io = photometric_tile_io(c.max_pairs, px_max * 3, px_max, n_pairs, T, px * 3, px, K, Z_mm, I_cur, I_des, v_p,
                                               p_status, p_robust, p_tiles, normal45, p_info);
    return host_call(h, io_list(io), h->photo_tile_io, [&](hipStream_t st) {
        return vitvs_photometric_tile_velocity_dev(h, n_pairs, io.I_cur.dev, io.I_des.dev, height, width,
                                                   Z_mm ? reinterpret_cast<const uint16_t*>(io.Z.dev) : nullptr, depth_scale, io.K.f64(),
                                                   level, interaction, mu, lambda, tiles_y, tiles_x, robust_iterations, sigma_min,
                                                   io.v_p.f64(), io.p_status.i32(), io.p_robust.f64(), io.p_tiles.f64(),
                                                   normal45 ? io.normal45.f64() : nullptr, p_info ? io.p_info.i32() : nullptr, st);
    });
}

// --- the surface photometric law ------------------------------------------------------------------
// Everything the robust law refuses (the lighting model is always on), and the cell grid; the first call allocates the law's own
// two blocks (the 128-double segment partials at 4096 segment rows of 8 cell columns = 32 MiB, a histogram and a state per pair of
// max_pairs; PhotometricSurfaceIo at 64 cells and 82 nodes per pair), zeroed, so no later call allocates.
static int photometric_surface_prepare(vitvs_handle* h, int n_pairs, int height, int width, int level, int interaction,
                                       double depth_scale, double mu, double lambda, int cells_y, int cells_x, int robust_iterations,
                                       double sigma_min, bool host_form) {
    if (int rc = photometric_check(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, host_form)) return rc;
    if (cells_y < 1 || cells_y > 8 || cells_x < 1 || cells_x > 8) return set_err(h, -2, "cells_y and cells_x are 1 .. 8");
    if (cells_y > (height >> level) || cells_x > (width >> level))
        return set_err(h, -2, "cells_y and cells_x are at most the pooled image's sides");
    if (robust_iterations < 0 || robust_iterations > 4) return set_err(h, -2, "robust_iterations is 0 .. 4");
    if (!std::isfinite(sigma_min) || !(sigma_min > 0.0)) return set_err(h, -2, "sigma_min is finite and > 0");
    const vitvs_config& c = h->cfg;
    PhotometricSurfacePlan pl;
    if (int rc = plan_photometric_surface(height, width, level, cells_y, cells_x, c.max_pairs, &pl))
        return set_err(h, rc, "no surface photometric plan");
    const size_t px_max = (size_t)c.u_max * c.v_max;
    PhotometricSurfaceIo io = photometric_surface_io(c.max_pairs, px_max * 3, px_max);
    return law_blocks(h, "surface photometric", &h->photo_surface_ws, photometric_surface_ws_bytes(c.max_pairs), &h->photo_surface_io,
                      io_place(io_list(io), nullptr));
}

int vitvs_photometric_surface_velocity_dev(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                           int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                                           int32_t interaction, double mu, double lambda, int32_t cells_y, int32_t cells_x,
                                           int32_t robust_iterations, double sigma_min, double* v_p, int32_t* p_status, double* p_robust,
                                           double* p_nodes, double* cell_sums, int32_t* p_info, void* stream) {
    if (!h || !I_cur || !I_des || !K || !v_p || !p_status || !p_robust || !p_nodes) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_surface_prepare(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, cells_y, cells_x,
                                             robust_iterations, sigma_min, false))
        return rc;
    PhotometricSurfaceArgs sa;
    memset(&sa, 0, sizeof(sa));
    PhotometricRobustArgs& ra = sa.r;
    PhotometricArgs& a = ra.p;
    a.n_pairs = n_pairs; a.height = height; a.width = width; a.level = level; a.interaction = interaction;
    a.I_cur = I_cur; a.I_des = I_des; a.Z_mm = Z_mm; a.depth_scale = depth_scale; a.K = K; a.mu = mu; a.lambda = lambda;
    a.v_p = v_p; a.p_status = p_status; a.p_info = p_info;
    ra.illumination = 1; ra.iterations = robust_iterations; ra.sigma_min = sigma_min;
    ra.p_robust = p_robust;
    sa.cells_y = cells_y; sa.cells_x = cells_x; sa.p_nodes = p_nodes; sa.cell_sums = cell_sums;
    const int rc = launch_photometric_surface(sa, h->photo_surface_ws, h->cfg.max_pairs, dev_stream(h, stream));
    return rc ? set_err(h, rc, "surface photometric law launch failed") : 0;
}

int vitvs_photometric_surface_velocity(vitvs_handle* h, int32_t n_pairs, const uint8_t* I_cur, const uint8_t* I_des, int32_t height,
                                       int32_t width, const uint16_t* Z_mm, double depth_scale, const double* K, int32_t level,
                                       int32_t interaction, double mu, double lambda, int32_t cells_y, int32_t cells_x,
                                       int32_t robust_iterations, double sigma_min, double* v_p, int32_t* p_status, double* p_robust,
                                       double* p_nodes, double* cell_sums, int32_t* p_info) {
    if (!h || !I_cur || !I_des || !K || !v_p || !p_status || !p_robust || !p_nodes) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    if (int rc = photometric_surface_prepare(h, n_pairs, height, width, level, interaction, depth_scale, mu, lambda, cells_y, cells_x,
                                             robust_iterations, sigma_min, true))
        return rc;
    const vitvs_config& c = h->cfg;
    const size_t px_max = (size_t)c.u_max * c.v_max, px = (size_t)height * width, T = (size_t)cells_y * cells_x;
    const size_t Q = (size_t)(cells_y + 1) * (cells_x + 1);
    PhotometricSurfaceIo io = photometric_surface_io(c.max_pairs, px_max * 3, px_max, n_pairs, T, Q, px * 3, px, K, Z_mm, I_cur, I_des,
                                                     v_p, p_status, p_robust, p_nodes, cell_sums, p_info);
    return host_call(h, io_list(io), h->photo_surface_io, [&](hipStream_t st) {
        return vitvs_photometric_surface_velocity_dev(h, n_pairs, io.I_cur.dev, io.I_des.dev, height, width,
                                                      Z_mm ? reinterpret_cast<const uint16_t*>(io.Z.dev) : nullptr, depth_scale,
                                                      io.K.f64(), level, interaction, mu, lambda, cells_y, cells_x, robust_iterations,
                                                      sigma_min, io.v_p.f64(), io.p_status.i32(), io.p_robust.f64(), io.p_nodes.f64(),
                                                      cell_sums ? io.cell_sums.f64() : nullptr, p_info ? io.p_info.i32() : nullptr, st);
    });
}

int vitvs_last_goal_depth(vitvs_handle* h, int32_t n_pairs, double* z) {
    if (!h || !z) return set_err(h, -1, "null argument");
    return last_row_output(h, n_pairs, h->last_law.goalz, h->zgoal_ws, 1, z);
}

int vitvs_last_weights(vitvs_handle* h, int32_t n_pairs, double* w) {
    if (!h || !w) return set_err(h, -1, "null argument");
    if (h->last_law.robust) return last_row_output(h, n_pairs, true, h->Wws, 1, w);
    DeviceScope dev(h);
    std::vector<int32_t> inf;
    if (int rc = last_info(h, n_pairs, false, inf)) return rc;
    const size_t R = h->cfg.max_rows;
    for (size_t b = 0; b < (size_t)n_pairs; ++b) {
        // the plain law: weight 1 on every live pair; fewer than 4 matches of a short selection leave none (TOO_FEW)
        const size_t n = feature_rows(h, inf, b);
        size_t live = std::min<size_t>(n, (size_t)std::max(inf[b * 8 + 3], 0));
        if (live < n && live < 4) live = 0;
        for (size_t k = 0; k < R; ++k) w[b * R + k] = k < live ? 1.0 : 0.0;
    }
    return 0;
}

int vitvs_last_offsets(vitvs_handle* h, int32_t n_pairs, float* offsets) {
    if (!h || !offsets) return set_err(h, -1, "null argument");
    return last_row_output(h, n_pairs, h->last_law.refine, h->off_ws, 2, offsets);
}

int vitvs_last_order(vitvs_handle* h, int32_t n_pairs, int32_t* order) {
    if (!h || !order) return set_err(h, -1, "null argument");
    if (!h->last_best) return set_err(h, -5, "the last law evaluation did not run in selection mode BEST");
    if (n_pairs <= 0 || n_pairs > h->last_pairs) return set_err(h, -3, "no such pairs in the last call");
    DeviceScope dev(h);
    VITVS_HIP_CHECK(hipDeviceSynchronize());
    VITVS_HIP_CHECK(hipMemcpy(order, h->order_ws, (size_t)n_pairs * h->last_T * 4, hipMemcpyDeviceToHost));
    return 0;
}

int vitvs_timing_enable(vitvs_handle* h, int32_t on) {
    if (!h) return set_err(h, -1, "null argument");
    DeviceScope dev(h);
    VITVS_HIP_CHECK(hipDeviceSynchronize());
    h->timing = on != 0;
    h->ev_used = 0;
    h->ev_class.clear();
    return 0;
}

int vitvs_timing_classes(void) { return KC_COUNT; }

const char* vitvs_timing_class_name(int32_t cls) { return (cls >= 0 && cls < KC_COUNT) ? kClassNames[cls] : ""; }

int vitvs_timing_collect(vitvs_handle* h, int32_t n_classes, double* total_ms, int32_t* launches) {
    if (!h || !total_ms || !launches || n_classes < KC_COUNT) return set_err(h, -1, "bad argument");
    DeviceScope dev(h);
    VITVS_HIP_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < n_classes; ++i) { total_ms[i] = 0.0; launches[i] = 0; }
    for (size_t i = 0; i < h->ev_class.size(); ++i) {
        float ms = 0.f;
        VITVS_HIP_CHECK(hipEventElapsedTime(&ms, h->ev_pool[2 * i], h->ev_pool[2 * i + 1]));
        total_ms[h->ev_class[i]] += ms;
        launches[h->ev_class[i]] += 1;
    }
    h->ev_used = 0;
    h->ev_class.clear();
    return 0;
}

// ---- include/vitvs_ops.h: single-operator entry points for the kernel-level parity tests ----
int vitvs_op_linear(int32_t precision, const void* A, const void* W, const float* bias, void* out, int32_t M,
                    int32_t N, int32_t K, int32_t gelu, void* stream) {
    DeviceScope dev(nullptr);
    return launch_linear(plan_linear(to_prec(precision), M, N, K, EPI_STORE), A, W, bias, out, gelu, as_stream(stream), g_op_wexp);
}
int vitvs_op_weight_exponent(int32_t e) {
    const int prev = g_op_wexp;
    if (e >= 0 && e <= 31) g_op_wexp = e;
    return prev;
}
int vitvs_op_linear_variant(int32_t precision, int32_t variant, const void* A, const void* W, const float* bias, void* out,
                            int32_t M, int32_t N, int32_t K, int32_t gelu, int32_t slices, void* stream) {
    DeviceScope dev(nullptr);
    return launch_linear(variant_plan(to_prec(precision), variant, M, N, K, slices), A, W, bias, out, gelu, as_stream(stream),
                         g_op_wexp);
}
int vitvs_op_linear_residual(int32_t precision, const void* A, const void* W, const float* bias, const float* ls,
                             float* x, int32_t M, int32_t N, int32_t K, void* stream) {
    DeviceScope dev(nullptr);
    return launch_linear(plan_linear(to_prec(precision), M, N, K, EPI_RESIDUAL), A, W, bias, x, 0, as_stream(stream), g_op_wexp,
                         ls);
}
int vitvs_op_layernorm(int32_t precision, const float* x, const float* gamma, const float* beta, void* out, int32_t M,
                       int32_t D, float eps, void* stream) {
    DeviceScope dev(nullptr);
    return launch_layernorm(to_prec(precision), x, gamma, beta, out, M, D, eps, as_stream(stream));
}
int vitvs_op_attention(int32_t precision, const void* qkv, void* out, int32_t n_img, int32_t N, int32_t H,
                       void* stream) {
    DeviceScope dev(nullptr);
    return launch_attention(plan_attention(to_prec(precision), n_img, N, H), qkv, out, as_stream(stream));
}
int vitvs_op_attention_q(int32_t precision, const void* qkv, void* out, int32_t n_img, int32_t N, int32_t H,
                         int32_t q_prescaled, void* stream) {
    DeviceScope dev(nullptr);
    const Precision p = to_prec(precision);
    return launch_attention(plan_attention(p, n_img, N, H), qkv, out, as_stream(stream), nullptr, q_prescaled != 0 && plain16(p));
}
int vitvs_op_linear_tile(int32_t precision, int32_t M, int32_t N, int32_t K, int32_t slices, int32_t* tile) {
    if (!tile) return -1;
    const LinearPlan pl = plan_linear(to_prec(precision), M, N, K, slices > 0 ? EPI_PARTIAL : EPI_STORE, slices);
    tile[0] = pl.rows; tile[1] = pl.cols; tile[2] = pl.rows && !pl.big ? pl.kgroups : 0;
    return pl.rows ? 0 : -2;
}
int vitvs_op_linear_plan(int32_t precision, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t slices, int32_t* out) {
    if (!out || (epilogue != EPI_STORE && epilogue != EPI_PARTIAL) || slices < 0) return -1;
    const LinearPlan pl = plan_linear(to_prec(precision), M, N, K, (LinearEpi)epilogue, slices);
    out[0] = pl.big; out[1] = pl.rows; out[2] = pl.cols; out[3] = pl.rows && !pl.big ? pl.kgroups : 0; out[4] = pl.stages;
    out[5] = pl.splits; out[6] = pl.xcd_map;
    return pl.rows ? 0 : -2;
}
int vitvs_op_linear_big_grid(int32_t precision, int32_t rows, int32_t cols, int32_t M, int32_t N, int32_t K, int32_t slices,
                             int32_t* out) {
    if (!out || slices < 0) return -1;
    BigGrid g;
    const int rc = linear_big_grid(to_prec(precision), rows, cols, M, N, K, slices > 0 ? slices : 1, &g);
    out[0] = (int32_t)std::min<long>(g.tiles, INT32_MAX); out[1] = g.slots; out[2] = g.xmap; out[3] = g.nk;
    return rc;
}
int vitvs_op_attention_plan(int32_t precision, int32_t n_img, int32_t N, int32_t H, int32_t* out) {
    if (!out) return -1;
    const AttnPlan pl = plan_attention(to_prec(precision), n_img, N, H);
    out[0] = pl.kernel; out[1] = (int32_t)(pl.grid.x * pl.grid.y * pl.grid.z); out[2] = pl.threads; out[3] = pl.lds;
    out[4] = pl.per; out[5] = pl.divided;
    return pl.kernel == ATTN_NONE ? -2 : 0;
}
int vitvs_op_gram_plan(int32_t precision, int32_t binned, int32_t T, int32_t D, int32_t n_pairs, int32_t max_pairs, int32_t* out) {
    if (!out) return -1;
    const GramPlan pl = plan_gram(to_prec(precision), binned != 0, T, D, n_pairs, max_pairs);
    out[0] = pl.form; out[1] = pl.rows; out[2] = pl.cols; out[3] = pl.kgroups; out[4] = pl.hb; out[5] = pl.per_xcd;
    out[6] = pl.split;
    return pl.rows ? 0 : -2;
}
int vitvs_op_servo_plan(int32_t T, int32_t max_rows, int32_t robust_iters, int32_t refine_source, int32_t interaction, int32_t* out) {
    if (!out) return -1;
    ServoPlan pl;
    const int rc = plan_servo(T, max_rows, robust_iters, refine_source, interaction, &pl);
    out[0] = pl.robust; out[1] = pl.refine; out[2] = pl.goalz; out[3] = (int32_t)pl.lds; out[4] = pl.source;
    out[5] = pl.reads_depth; out[6] = pl.depth_anywhere;
    return rc;
}
// the arg-max keys of n_pairs pairs -> nn_1 / nn_2 / sim_1 [n_pairs][T], as the law's kernel decodes them
int vitvs_op_rig_law(int32_t n_cams, const int32_t* rows, const double* L, int32_t ld, const double* W, double lambda,
                     void* scratch, double* v_rig, int32_t* rig_status, int32_t* rig_info, double* normal, void* stream) {
    if (!rows || !L || !W || !scratch || !v_rig || !rig_status) return -1;
    if (n_cams < 1 || n_cams > kRigMaxCams || ld < 1) return -2;
    RigArgs a;
    memset(&a, 0, sizeof(a));
    a.n_cams = n_cams; a.rows = rows; a.rows_stride = 1; a.L = L; a.ld = ld; a.W = W; a.lambda = lambda;
    rig_carve(scratch, n_cams, ld, a);
    a.v_rig = v_rig; a.rig_status = rig_status; a.rig_info = rig_info; a.normal = normal;
    return launch_rig(a, as_stream(stream), g_op_rig_two_launches);
}

int vitvs_op_rig_scratch_bytes(int32_t n_cams, int32_t ld) {
    return (n_cams < 1 || n_cams > kRigMaxCams || ld < 1) ? -2 : bytes_i32(rig_scratch_bytes(n_cams, ld));
}

int vitvs_op_rig_robust_law(int32_t n_cams, const int32_t* rows, const int32_t* live, const double* L, int32_t ld, const double* W,
                            double lambda, int32_t n_iter, double sigma_min, void* scratch, double* v_rig, int32_t* rig_status,
                            int32_t* rig_info, double* normal, double* weights, double* sigma, void* stream) {
    if (!rows || !L || !W || !scratch || !v_rig || !rig_status) return -1;
    if (n_cams < 1 || n_cams > kRigMaxCams || ld < 1 || n_iter < 1 || n_iter > 16) return -2;
    RigRobustArgs ra;
    memset(&ra, 0, sizeof(ra));
    RigArgs& a = ra.r;
    a.n_cams = n_cams; a.rows = rows; a.rows_stride = 1; a.L = L; a.ld = ld; a.W = W; a.lambda = lambda;
    rig_robust_carve(scratch, n_cams, ld, ra);
    a.v_rig = v_rig; a.rig_status = rig_status; a.rig_info = rig_info; a.normal = normal;
    ra.live = live; ra.live_stride = 1; ra.n_iter = n_iter; ra.sigma_min = sigma_min;
    ra.weights = weights; ra.weights_stride = ld / 2; ra.sigma = sigma;
    return launch_rig_robust(ra, as_stream(stream));
}

int vitvs_op_rig_robust_scratch_bytes(int32_t n_cams, int32_t ld) {
    return (n_cams < 1 || n_cams > kRigMaxCams || ld < 1) ? -2 : bytes_i32(rig_robust_scratch_bytes(n_cams, ld));
}

int vitvs_op_rig_robust_plan(int32_t n_cams, int32_t ld, int32_t* out) {
    if (!out) return -1;
    RigRobustPlan pl;
    memset(&pl, 0, sizeof(pl));
    const int rc = plan_rig_robust(n_cams, ld, &pl);
    out[0] = (int32_t)pl.lds; out[1] = pl.lds_resident; out[2] = pl.pairs; out[3] = pl.lds_opt_in;
    return rc;
}

int vitvs_op_pose_consensus_law(int32_t n_pairs, int32_t ld, const double* P, const double* Q, const int32_t* usable, double lambda,
                                int32_t n_iter, double sigma_min, void* scratch, double* v_pose, int32_t* pose_status, double* pose,
                                int32_t* pose_info, double* weights, double* sigma, void* stream, int32_t n_hyp, uint32_t seed) {
    if (!P || !Q || !usable || !scratch || !v_pose || !pose_status) return -1;
    if (n_pairs < 1 || ld < 1 || n_iter < 0 || n_iter > 16) return -2;
    if (n_hyp < 0 || n_hyp > 4096 || (n_hyp > 0 && !(sigma_min > 0.0))) return -2;
    PoseArgs a;
    memset(&a, 0, sizeof(a));
    a.n_pairs = n_pairs; a.ld = ld; a.P = P; a.Q = Q; a.usable = usable; a.lambda = lambda; a.n_iter = n_iter;
    a.sigma_min = sigma_min; a.ws = static_cast<double*>(scratch); a.n_hyp = n_hyp; a.seed = seed;
    a.v_pose = v_pose; a.pose_status = pose_status; a.pose = pose; a.pose_info = pose_info;
    a.weights = weights; a.weights_stride = ld; a.sigma = sigma;
    return launch_pose(a, as_stream(stream));
}

int vitvs_op_pose_law(int32_t n_pairs, int32_t ld, const double* P, const double* Q, const int32_t* usable, double lambda,
                      int32_t n_iter, double sigma_min, void* scratch, double* v_pose, int32_t* pose_status, double* pose,
                      int32_t* pose_info, double* weights, double* sigma, void* stream) {
    return vitvs_op_pose_consensus_law(n_pairs, ld, P, Q, usable, lambda, n_iter, sigma_min, scratch, v_pose, pose_status, pose,
                                       pose_info, weights, sigma, stream, 0, 0);
}

int vitvs_op_pose_scratch_bytes(int32_t n_pairs, int32_t ld) {
    return (n_pairs < 1 || ld < 1) ? -2 : bytes_i32(pose_scratch_bytes(n_pairs, ld));
}

int vitvs_op_pose_plan(int32_t max_rows, int32_t n_iter, int32_t* out) {
    if (!out) return -1;
    PosePlan pl;
    memset(&pl, 0, sizeof(pl));
    return plan_out(plan_pose(max_rows, n_iter, 0, &pl), pl, out);
}

int vitvs_op_pose_consensus_plan(int32_t max_rows, int32_t n_iter, int32_t n_hyp, int32_t* out) {
    if (!out) return -1;
    PosePlan pl;
    memset(&pl, 0, sizeof(pl));
    const int rc = plan_out(plan_pose(max_rows, n_iter, n_hyp, &pl), pl, out);
    out[3] = pl.consensus;
    return rc;
}

int vitvs_op_pose_rig_law(int32_t n_cams, int32_t ld, const double* P, const double* Q, const int32_t* usable, const double* rTc,
                          const int32_t* cam_status, double lambda, int32_t n_iter, double sigma_min, void* scratch, double* v_rig,
                          int32_t* rig_status, double* pose, int32_t* rig_info, double* moments, double* weights, double* sigma,
                          void* stream) {
    if (!P || !Q || !usable || !rTc || !scratch || !v_rig || !rig_status) return -1;
    if (n_cams < 1 || ld < 1 || n_iter < 0 || n_iter > 16) return -2;
    PoseRigArgs a;
    memset(&a, 0, sizeof(a));
    a.n_cams = n_cams; a.ld = ld; a.status = cam_status; a.rTc = rTc; a.P = P; a.Q = Q; a.usable = usable; a.lambda = lambda;
    a.n_iter = n_iter; a.sigma_min = sigma_min; a.ws = static_cast<double*>(scratch);
    a.v_rig = v_rig; a.rig_status = rig_status; a.pose = pose; a.rig_info = rig_info; a.moments = moments;
    a.weights = weights; a.weights_stride = ld; a.sigma = sigma;
    return launch_pose_rig(a, as_stream(stream));
}

int vitvs_op_pose_rig_scratch_bytes(int32_t n_cams, int32_t ld) {
    return (n_cams < 1 || ld < 1) ? -2 : bytes_i32(pose_rig_scratch_bytes(n_cams, ld));
}

int vitvs_op_pose_rig_plan(int32_t n_cams, int32_t ld, int32_t n_iter, int32_t* out) {
    if (!out) return -1;
    PoseRigPlan pl;
    memset(&pl, 0, sizeof(pl));
    return plan_out(plan_pose_rig(n_cams, ld, n_iter, &pl), pl, out);
}

int vitvs_op_homography_consensus_law(int32_t n_pairs, int32_t ld, const double* m, const double* ms, const int32_t* usable,
                                      double lambda, double depth_scale, int32_t n_iter, double sigma_min, void* scratch, double* v_h,
                                      int32_t* h_status, double* H, int32_t* h_info, double* weights, double* sigma, void* stream,
                                      int32_t n_hyp, uint32_t seed) {
    if (!m || !ms || !usable || !scratch || !v_h || !h_status) return -1;
    if (n_pairs < 1 || ld < 1 || n_iter < 0 || n_iter > 16 || !(depth_scale > 0.0) || !std::isfinite(depth_scale)) return -2;
    if (n_hyp < 0 || n_hyp > 4096 || (n_hyp > 0 && !(sigma_min > 0.0))) return -2;
    HomographyArgs a;
    memset(&a, 0, sizeof(a));
    a.n_pairs = n_pairs; a.ld = ld; a.m = m; a.ms = ms; a.usable = usable; a.lambda = lambda; a.depth_scale = depth_scale;
    a.n_iter = n_iter; a.sigma_min = sigma_min; a.ws = static_cast<double*>(scratch); a.n_hyp = n_hyp; a.seed = seed;
    a.v_h = v_h; a.h_status = h_status; a.H = H; a.h_info = h_info;
    a.weights = weights; a.weights_stride = ld; a.sigma = sigma;
    return launch_homography(a, as_stream(stream));
}

int vitvs_op_homography_law(int32_t n_pairs, int32_t ld, const double* m, const double* ms, const int32_t* usable, double lambda,
                            double depth_scale, int32_t n_iter, double sigma_min, void* scratch, double* v_h, int32_t* h_status,
                            double* H, int32_t* h_info, double* weights, double* sigma, void* stream) {
    return vitvs_op_homography_consensus_law(n_pairs, ld, m, ms, usable, lambda, depth_scale, n_iter, sigma_min, scratch, v_h,
                                             h_status, H, h_info, weights, sigma, stream, 0, 0);
}

int vitvs_op_homography_scratch_bytes(int32_t n_pairs, int32_t ld) {
    return (n_pairs < 1 || ld < 1) ? -2 : bytes_i32(homography_scratch_bytes(n_pairs, ld));
}

int vitvs_op_homography_plan(int32_t max_rows, int32_t n_iter, int32_t* out) {
    if (!out) return -1;
    HomographyPlan pl;
    memset(&pl, 0, sizeof(pl));
    return plan_out(plan_homography(max_rows, n_iter, 0, &pl), pl, out);
}

int vitvs_op_homography_consensus_plan(int32_t max_rows, int32_t n_iter, int32_t n_hyp, int32_t* out) {
    if (!out) return -1;
    HomographyPlan pl;
    memset(&pl, 0, sizeof(pl));
    const int rc = plan_out(plan_homography(max_rows, n_iter, n_hyp, &pl), pl, out);
    out[3] = pl.consensus;
    return rc;
}

int vitvs_op_photometric_plan(int32_t height, int32_t width, int32_t level, int32_t* out) {
    if (!out) return -1;
    PhotometricPlan pl;
    memset(&pl, 0, sizeof(pl));
    const int rc = plan_photometric(height, width, level, 1, &pl);
    out[0] = pl.h; out[1] = pl.w; out[2] = pl.rows; out[3] = pl.bands; out[4] = (int32_t)pl.lds; out[5] = (int32_t)pl.ws_bytes;
    out[6] = pl.lds_opt_in; out[7] = 0;
    return rc;
}

int vitvs_op_photometric_tile_plan(int32_t height, int32_t width, int32_t level, int32_t tiles_y, int32_t tiles_x, int32_t* out) {
    if (!out) return -1;
    PhotometricTilePlan pl;
    memset(&pl, 0, sizeof(pl));
    const int rc = plan_photometric_tiles(height, width, level, tiles_y, tiles_x, 1, &pl);
    if (rc) memset(&pl, 0, sizeof(pl));
    out[0] = pl.h; out[1] = pl.w; out[2] = pl.rows; out[3] = pl.bands; out[4] = pl.slots; out[5] = (int32_t)pl.lds;
    out[6] = (int32_t)pl.lds_res; out[7] = (int32_t)pl.ws_doubles;
    return rc;
}

int vitvs_op_photometric_surface_plan(int32_t height, int32_t width, int32_t level, int32_t cells_y, int32_t cells_x, int32_t* out) {
    if (!out) return -1;
    PhotometricSurfacePlan pl;
    memset(&pl, 0, sizeof(pl));
    const int rc = plan_photometric_surface(height, width, level, cells_y, cells_x, 1, &pl);
    if (rc) memset(&pl, 0, sizeof(pl));
    out[0] = pl.t.h; out[1] = pl.t.w; out[2] = pl.t.rows; out[3] = pl.t.bands; out[4] = pl.t.slots; out[5] = (int32_t)pl.t.lds;
    out[6] = (int32_t)pl.t.lds_res; out[7] = (int32_t)pl.ws_doubles;
    return rc;
}

int vitvs_op_rig_two_launches(int32_t on) {
    const int prev = g_op_rig_two_launches ? 1 : 0;
    g_op_rig_two_launches = on != 0;
    return prev;
}

static int decode_pairs(const unsigned long long* row_best, const unsigned long long* col_best, int T, int n_pairs, int32_t* nn_1,
                        int32_t* nn_2, float* sim_1, hipStream_t st) {
    int rc = 0;
    for (int b = 0; !rc && b < n_pairs; ++b) {
        const size_t o = (size_t)b * T;
        rc = launch_decode_best(row_best + o, col_best + o, T, nn_1 + o, nn_2 + o, sim_1 + o, st);
    }
    return rc;
}
int vitvs_op_gram_argmax(int32_t precision, const float* dn, int32_t T, int32_t Dp, int32_t n_pairs, int32_t des_shared, void* dh,
                         uint64_t* row_best, uint64_t* col_best, int32_t* nn_1, int32_t* nn_2, float* sim_1, void* stream) {
    if (!dn || !row_best || !col_best || !nn_1 || !nn_2 || !sim_1) return -1;
    const GramPlan pl = plan_gram(to_prec(precision), false, T, Dp, n_pairs, n_pairs);
    if (!pl.rows) return -2;
    if (pl.split && !dh) return -1;
    DeviceScope dev(nullptr);
    hipStream_t st = as_stream(stream);
    unsigned long long *rb = reinterpret_cast<unsigned long long*>(row_best), *cb = reinterpret_cast<unsigned long long*>(col_best);
    VITVS_HIP_CHECK(hipMemsetAsync(rb, 0, (size_t)n_pairs * T * 8, st));
    VITVS_HIP_CHECK(hipMemsetAsync(cb, 0, (size_t)n_pairs * T * 8, st));
    GramOperands go;                            // (dn is written only by the descriptor step of a binned plan)
    go.dn = const_cast<float*>(dn); go.dh = dh; go.des_shared = des_shared; go.row_best = rb; go.col_best = cb;
    const int rc = launch_gram(pl, go, st);
    return rc ? rc : decode_pairs(rb, cb, T, n_pairs, nn_1, nn_2, sim_1, st);
}
int vitvs_op_gram_stencil(const float* x, int32_t T, int32_t P, int32_t D, int32_t grid, int32_t n_pairs, int32_t des_shared,
                          float* G, float* sq, uint64_t* row_best, uint64_t* col_best, int32_t* nn_1, int32_t* nn_2, float* sim_1,
                          void* stream) {
    if (!x || !G || !sq || !row_best || !col_best || !nn_1 || !nn_2 || !sim_1) return -1;
    const GramPlan pl = plan_gram(PREC_F32, true, T, D, n_pairs, n_pairs);
    if (pl.form != GRAM_STENCIL || !pl.rows || grid * grid != T || P < 1) return -2;
    DeviceScope dev(nullptr);
    hipStream_t st = as_stream(stream);
    unsigned long long *rb = reinterpret_cast<unsigned long long*>(row_best), *cb = reinterpret_cast<unsigned long long*>(col_best);
    const int n_frames = (des_shared ? 1 : n_pairs) + n_pairs;
    // the tokens' squared norms; the same launch clears the keys (what the forward's last launch does on the velocity path)
    int rc = launch_descriptors(x, nullptr, nullptr, sq, n_frames, T, P, grid, D, 1, rb, cb, n_pairs * T, st);
    GramOperands go;
    go.x = x; go.P = P; go.G = G; go.sq = sq; go.grid = grid; go.des_shared = des_shared; go.row_best = rb; go.col_best = cb;
    if (!rc) rc = launch_gram(pl, go, st);
    return rc ? rc : decode_pairs(rb, cb, T, n_pairs, nn_1, nn_2, sim_1, st);
}
int vitvs_op_best_order_dev(int32_t T, int32_t cells, int32_t n_pairs, const int32_t* nn_1, const int32_t* nn_2, const float* sim_1,
                            int32_t* order, void* stream) {
    if (!nn_1 || !nn_2 || !sim_1 || !order) return -1;
    if (n_pairs < 1) return -2;
    BestOrderPlan bp;
    if (int rc = plan_best_order(T, cells, &bp)) return rc;    // (before anything is allocated or launched)
    DeviceScope dev(nullptr);
    hipStream_t st = as_stream(stream);
    // the packed keys the law reads, made from the tables as vitvs_servo_from_nn_dev makes them; freed behind the launches
    unsigned long long* keys = nullptr;
    if (hipMalloc((void**)&keys, (size_t)2 * n_pairs * T * 8) != hipSuccess) return -6;
    unsigned long long *rb = keys, *cb = keys + (size_t)n_pairs * T;
    int rc = 0;
    for (int b = 0; !rc && b < n_pairs; ++b) {
        const size_t o = (size_t)b * T;
        rc = launch_encode_best(nn_1 + o, nn_2 + o, sim_1 + o, T, rb + o, cb + o, st);
    }
    if (!rc) rc = launch_best_order(bp, n_pairs, rb, cb, order, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = -1;
    (void)hipFree(keys);
    return rc;
}
int vitvs_op_quarter_turns(const uint8_t* frames, int32_t n, int32_t S, uint8_t* out, void* stream) {
    DeviceScope dev(nullptr);
    return launch_quarter_turns(frames, out, n, S, as_stream(stream));
}
int vitvs_op_roll_pick(int32_t T, const int32_t* nn_1, const int32_t* nn_2, const float* sim_1, int32_t* nn_1_out, int32_t* nn_2_out,
                       float* sim_1_out, int32_t* roll_info, double* scores, void* stream) {
    if (!nn_1 || !nn_2 || !sim_1 || !nn_1_out || !nn_2_out || !sim_1_out || !roll_info || !scores) return -1;
    const int g = T > 0 ? (int)floor(sqrt((double)T)) : 0;
    if (T <= 0 || g * g != T) return -2;
    DeviceScope dev(nullptr);
    hipStream_t st = as_stream(stream);
    // the packed keys of the four candidates, made from the tables as vitvs_servo_from_nn_dev makes them, and the flag the pick
    // leaves for the law; freed behind the launches
    unsigned long long* keys = nullptr;
    if (hipMalloc((void**)&keys, (size_t)2 * 4 * T * 8 + 256) != hipSuccess) return -6;
    unsigned long long *rb = keys, *cb = keys + (size_t)4 * T;
    int32_t* rolled = reinterpret_cast<int32_t*>(keys + (size_t)8 * T);
    int rc = 0;
    for (int k = 0; !rc && k < 4; ++k) {
        const size_t o = (size_t)k * T;
        rc = launch_encode_best(nn_1 + o, nn_2 + o, sim_1 + o, T, rb + o, cb + o, st);
    }
    if (!rc) rc = launch_roll_pick(rb, cb, T, g, scores, roll_info, rolled, st);
    if (!rc) rc = launch_decode_best(rb, cb, T, nn_1_out, nn_2_out, sim_1_out, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = -1;
    (void)hipFree(keys);
    return rc;
}
int vitvs_op_touch(const void* p, int64_t bytes, int32_t share_xcds, void* stream) {
    DeviceScope dev(nullptr);
    return launch_touch(p, (size_t)bytes, share_xcds, as_stream(stream));
}
int vitvs_op_plan_in_flight(int32_t n) {
    const int prev = g_updates_in_flight;
    if (n >= 1) g_updates_in_flight = n;
    return prev;
}
int vitvs_op_splitk_slices(int32_t precision, int32_t M, int32_t N, int32_t K) {
    return plan_linear(to_prec(precision), M, N, K, EPI_PARTIAL).splits;
}
int vitvs_op_linear_partial(int32_t precision, const void* A, const void* W, float* part, int32_t M, int32_t N,
                            int32_t K, int32_t slices, void* stream) {
    DeviceScope dev(nullptr);
    if (slices < 1) return -2;
    return launch_linear(plan_linear(to_prec(precision), M, N, K, EPI_PARTIAL, slices), A, W, nullptr, part, 0, as_stream(stream),
                         g_op_wexp);
}
int vitvs_op_residual_ln(int32_t precision, float* x, const float* part, int32_t slices, const float* bias,
                         const float* ls, const float* gamma, const float* beta, void* out, int32_t M, int32_t D,
                         float eps, void* stream) {
    DeviceScope dev(nullptr);
    return launch_residual_ln(to_prec(precision), x, part, slices, bias, ls, gamma, beta, out, M, D,
                              eps, as_stream(stream));
}

// ---- the two ends of the forward (elementwise.hip), pointer-only: arguments go straight to the launch_* function ----
int vitvs_op_patchify(int32_t precision, const uint8_t* des, int32_t n_des, const uint8_t* cur, int32_t n_cur, int32_t S,
                      int32_t patch, int32_t stride, int32_t Kp, int32_t D, int32_t prefix, const float* mean, const float* std,
                      const float* cls, const float* pos, int32_t in_h, int32_t in_w, void* Ape, float* x, void* stream) {
    if (!mean || !std || !cls || !pos || !Ape || !x || (n_des > 0 && !des) || (n_cur > 0 && !cur)) return -1;
    if (n_des < 0 || n_cur < 0 || S <= 0 || patch <= 0 || patch > S || stride <= 0 || D <= 0 || prefix < 1 || in_h < 0 || in_w < 0 ||
        (in_h == 0) != (in_w == 0))
        return -2;
    DeviceScope dev(nullptr);
    hipStream_t st = as_stream(stream);
    PatchifyArgs pa{};
    pa.des = des; pa.cur = cur; pa.n_des = n_des; pa.n_cur = n_cur;
    pa.S = S; pa.patch = patch; pa.stride = stride; pa.grid = 1 + (S - patch) / stride; pa.Kp = Kp; pa.D = D;
    for (int i = 0; i < 3; ++i) { pa.mean[i] = mean[i]; pa.std[i] = std[i]; }
    pa.cls = cls; pa.pos = pos; pa.prefix = prefix;
    if (in_h == 0) return launch_patchify(to_prec(precision), pa, nullptr, Ape, x, st);
    // the fused resize: Pillow's tables for (in_h, in_w) -> S, as vitvs_set_frame_size builds them, for this launch only
    std::vector<int> tab[4];   // xb, xk, yb, yk
    ResizeArgs rs{};
    rs.ksx = resize_coefficients(in_w, S, tab[0], tab[1]);
    rs.ksy = resize_coefficients(in_h, S, tab[2], tab[3]);
    rs.in_h = in_h; rs.in_w = in_w;
    rs.rows = resize_patch_rows(tab[2], S, patch);
    if (rs.rows < 0) return -5;
    if ((size_t)rs.rows * patch * 3 > 64 * 1024) return -3;
    int* d[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    for (int i = 0; i < 4 && !rc; ++i) {
        if (hipMalloc((void**)&d[i], tab[i].size() * sizeof(int)) != hipSuccess ||
            hipMemcpyAsync(d[i], tab[i].data(), tab[i].size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
            rc = -6;
    }
    rs.xb = d[0]; rs.xk = d[1]; rs.yb = d[2]; rs.yk = d[3];
    if (!rc) rc = launch_patchify(to_prec(precision), pa, &rs, Ape, x, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = -1;   // the launch is done with the tables before they go
    for (int i = 0; i < 4; ++i)
        if (d[i]) (void)hipFree(d[i]);
    return rc;
}
int vitvs_op_embed_ln(int32_t precision, float* x, const float* part, int32_t slices, const float* bias, const float* pos,
                      const float* cls, const float* reg, const float* gamma, const float* beta, void* out, int32_t n_img, int32_t T,
                      int32_t P, int32_t D, float eps, void* stream) {
    DeviceScope dev(nullptr);
    return launch_embed_ln(to_prec(precision), x, part, slices, bias, pos, cls, reg, gamma, beta, out, n_img, T, P, D, eps,
                           as_stream(stream));
}
int vitvs_op_residual_desc(int32_t precision, float* x, const float* part, int32_t slices, const float* bias, const float* ls,
                           float* dn, float* sq, uint64_t* zero_a, uint64_t* zero_b, int32_t zero_count, int32_t T, int32_t P,
                           int32_t M, int32_t D, void* stream) {
    if (zero_count < 0 || (zero_count > 0 && (!zero_a || !zero_b))) return -2;
    DeviceScope dev(nullptr);
    DescOut d;
    d.dn = dn; d.sq = sq; d.T = T; d.P = P; d.zero_count = zero_count;
    d.zero_a = reinterpret_cast<unsigned long long*>(zero_a);
    d.zero_b = reinterpret_cast<unsigned long long*>(zero_b);
    return launch_residual_ln(to_prec(precision), x, part, slices, bias, ls, nullptr, nullptr, nullptr, M, D, 0.f, as_stream(stream),
                              &d);
}
int vitvs_op_descriptors(const float* x, float* dn, float* raw, float* sq_ws, int32_t n_img, int32_t T, int32_t P, int32_t grid,
                         int32_t D, int32_t binned, uint64_t* zero_a, uint64_t* zero_b, int32_t zero_count, void* stream) {
    // the plain kernel always writes dn and keeps a row in 4 float4 per lane; the binned one reads the squared-norm workspace
    if (!x || D <= 0 || D % 4 != 0 || zero_count < 0 || (zero_count > 0 && (!zero_a || !zero_b))) return -2;
    if (binned ? (!sq_ws || (!dn && !raw)) : (!dn || D > 1024)) return -2;
    DeviceScope dev(nullptr);
    return launch_descriptors(x, dn, raw, sq_ws, n_img, T, P, grid, D, binned, reinterpret_cast<unsigned long long*>(zero_a),
                              reinterpret_cast<unsigned long long*>(zero_b), zero_count, as_stream(stream));
}
int vitvs_op_facet(int32_t precision, const void* qkv, float* out, int32_t n_img, int32_t T, int32_t P, int32_t H, int32_t which,
                   float unscale, int32_t keep_cls, void* stream) {
    DeviceScope dev(nullptr);
    return launch_facet(to_prec(precision), qkv, out, n_img, T, P, H, which, unscale, keep_cls, as_stream(stream));
}
int vitvs_op_saliency(int32_t precision, const void* qkv, float* out, int32_t n_img, int32_t T, int32_t P, int32_t H,
                      const int32_t* head_idx, int32_t n_heads, int32_t q_prescaled, void* stream) {
    if (!head_idx) return -1;
    DeviceScope dev(nullptr);
    return launch_saliency(to_prec(precision), qkv, out, n_img, T, P, H, head_idx, n_heads, q_prescaled != 0, as_stream(stream));
}
int vitvs_op_normalize_rows(const float* src, float* dst, int32_t rows, int32_t Dp, void* stream) {
    DeviceScope dev(nullptr);
    return launch_normalize_rows(src, dst, rows, Dp, as_stream(stream));
}

}  // extern "C"
