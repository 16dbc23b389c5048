// The device side of the follow-on laws' host-pointer entry points (api.hip): per law ONE list of the fields its block holds,
// in the block's order.  io_place turns a list into the block's size and every field's device pointer, so the allocation and the
// pointers cannot disagree; host_call (api.hip) copies along the same list.  No HIP here: tools/io_layout_check.cpp checks the
// lists on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vitvs {

struct IoField {
    size_t elem;                  // bytes per element: 8 (f64) or 4 (i32) (the roll search's and the photometric law's lists: also 2 (u16) and 1 (u8)); a list
                                  // holds its widest fields first, so nothing is padded
    size_t cap;                   // elements the block reserves: the field at max_pairs / max_rows
    size_t count;                 // elements of the call at hand: what is copied
    bool input;                   // copied to the device before the launch; an output is copied back after it
    void* host;                   // the caller's array; null: an optional output nobody asked for
    unsigned char* dev = nullptr; // io_place
    double* f64() const { return reinterpret_cast<double*>(dev); }
    int32_t* i32() const { return reinterpret_cast<int32_t*>(dev); }
};

inline IoField io_in(size_t elem, size_t cap, size_t count, const void* host) {
    return IoField{elem, cap, count, true, const_cast<void*>(host)};
}
inline IoField io_out(size_t elem, size_t cap, size_t count, void* host) { return IoField{elem, cap, count, false, host}; }

// A law's list is a struct of IoFields and nothing else: its members, in declaration order, are the block.
struct IoList {
    IoField* f;
    size_t n;
};
template <typename Io>
IoList io_list(Io& io) {
    static_assert(sizeof(Io) % sizeof(IoField) == 0 && alignof(Io) == alignof(IoField), "a struct of IoFields only");
    return IoList{reinterpret_cast<IoField*>(&io), sizeof(Io) / sizeof(IoField)};
}

// The fields one after the other from `base` (null: sizes only); returns the block's bytes.
inline size_t io_place(IoList l, unsigned char* base) {
    size_t off = 0;
    for (size_t i = 0; i < l.n; ++i) {
        l.f[i].dev = base ? base + off : nullptr;
        off += l.f[i].cap * l.f[i].elem;
    }
    return off;
}

// P = max_pairs, R = max_rows, n = the call's pairs / cameras.  A list of P and R alone still sizes the block (*_prepare).

// the rig law and its robust form (K, sigma and weights are the robust form's: null, nothing copied, in the plain one)
struct RigIo {
    IoField cVr, v_rig, normal, K, sigma, weights, status, rig_status, rig_info;
};
inline RigIo rig_io(size_t P, size_t R, size_t n = 0, const double* cVr = nullptr, const int32_t* status = nullptr,
                    const double* K = nullptr, double* v_rig = nullptr, int32_t* rig_status = nullptr, int32_t* rig_info = nullptr,
                    double* normal = nullptr, double* weights = nullptr, double* sigma = nullptr) {
    return RigIo{io_in(8, P * 36, n * 36, cVr), io_out(8, 6, 6, v_rig),        io_out(8, 28, 28, normal),
                 io_in(8, P * 4, n * 4, K),     io_out(8, 1, 1, sigma),        io_out(8, P * R, n * R, weights),
                 io_in(4, P, n, status),        io_out(4, 1, 1, rig_status),   io_out(4, 8, 8, rig_info)};
}

// the pose law
struct PoseIo {
    IoField K, v_pose, pose, sigma, weights, status, pose_status, pose_info;
};
inline PoseIo pose_io(size_t P, size_t R, size_t n = 0, const double* K = nullptr, const int32_t* status = nullptr,
                      double* v_pose = nullptr, int32_t* pose_status = nullptr, double* pose = nullptr, int32_t* pose_info = nullptr,
                      double* weights = nullptr, double* sigma = nullptr) {
    return PoseIo{io_in(8, P * 4, n * 4, K),        io_out(8, P * 6, n * 6, v_pose), io_out(8, P * 12, n * 12, pose),
                  io_out(8, P, n, sigma),           io_out(8, P * R, n * R, weights), io_in(4, P, n, status),
                  io_out(4, P, n, pose_status),     io_out(4, P * 8, n * 8, pose_info)};
}

// the homography law
struct HomographyIo {
    IoField K, v_h, H, sigma, weights, status, h_status, h_info;
};
inline HomographyIo homography_io(size_t P, size_t R, size_t n = 0, const double* K = nullptr, const int32_t* status = nullptr,
                                  double* v_h = nullptr, int32_t* h_status = nullptr, double* H = nullptr, int32_t* h_info = nullptr,
                                  double* weights = nullptr, double* sigma = nullptr) {
    return HomographyIo{io_in(8, P * 4, n * 4, K),    io_out(8, P * 6, n * 6, v_h),     io_out(8, P * 9, n * 9, H),
                        io_out(8, P, n, sigma),       io_out(8, P * R, n * R, weights), io_in(4, P, n, status),
                        io_out(4, P, n, h_status),    io_out(4, P * 8, n * 8, h_info)};
}

// the pose rig law
struct PoseRigIo {
    IoField rTc, K, v_rig, pose, moments, sigma, weights, status, rig_status, rig_info;
};
inline PoseRigIo pose_rig_io(size_t P, size_t R, size_t n = 0, const double* rTc = nullptr, const double* K = nullptr,
                             const int32_t* status = nullptr, double* v_rig = nullptr, int32_t* rig_status = nullptr,
                             double* pose = nullptr, int32_t* rig_info = nullptr, double* moments = nullptr, double* weights = nullptr,
                             double* sigma = nullptr) {
    return PoseRigIo{io_in(8, P * 12, n * 12, rTc), io_in(8, P * 4, n * 4, K),        io_out(8, 6, 6, v_rig),
                     io_out(8, 12, 12, pose),       io_out(8, 18, 18, moments),       io_out(8, 1, 1, sigma),
                     io_out(8, P * R, n * R, weights), io_in(4, P, n, status),        io_out(4, 1, 1, rig_status),
                     io_out(4, 8, 8, rig_info)};
}

// the roll search (vitvs_roll_velocity): ONE pair.  T tokens, R = max_rows, `frame` = S * S * 3 bytes, `depth` = u_max * v_max
// pixels.  Behind the 8- and 4-byte fields come the depth image (2-byte elements) and the two frames (bytes); the capacities are
// rounded so that each of the three begins on a 16-byte boundary of the block.  n_sel = the ids / order entries the call's
// selection mode hands over (0: none).  Z and I_des are optional INPUTS: null, nothing is copied and the _dev form gets null.
struct RollIo {
    IoField K, v_c, scores, status, roll_info, n_selected, selection, Z, I_cur, I_des;
};
inline RollIo roll_io(size_t T, size_t R, size_t frame, size_t depth, size_t n_sel = 0, const double* K = nullptr,
                      const int32_t* selection = nullptr, const int32_t* n_selected = nullptr, const uint16_t* Z = nullptr,
                      const uint8_t* I_cur = nullptr, const uint8_t* I_des = nullptr, double* v_c = nullptr, int32_t* status = nullptr,
                      int32_t* roll_info = nullptr, double* scores = nullptr) {
    const size_t sel_cap = ((T > R ? T : R) + 3) & ~(size_t)3, z_cap = (depth + 7) & ~(size_t)7, f_cap = (frame + 15) & ~(size_t)15;
    return RollIo{io_in(8, 4, 4, K),               io_out(8, 6, 6, v_c),              io_out(8, 4, 4, scores),
                  io_out(4, 4, 1, status),         io_out(4, 8, 8, roll_info),        io_in(4, 4, 1, n_selected),
                  io_in(4, sel_cap, n_sel, selection), io_in(2, z_cap, depth, Z),     io_in(1, f_cap, frame, I_cur),
                  io_in(1, f_cap, frame, I_des)};
}

// the photometric law (vitvs_photometric_velocity): n pairs of frames of `frame` = height * width * 3 bytes and depth images of
// `depth` = height * width pixels each, one pair behind the other; the block holds P pairs at the handle's v_max x u_max (`frame_max`,
// `depth_max`).  Behind the 8- and 4-byte fields (the statuses' capacity rounded to four entries) come the depth images and the
// frames, each on a 16-byte boundary of the block as in RollIo.  Z is an optional INPUT.
struct PhotometricIo {
    IoField K, v_p, normal, p_status, p_info, Z, I_cur, I_des;
};
inline PhotometricIo photometric_io(size_t P, size_t frame_max, size_t depth_max, size_t n = 0, size_t frame = 0, size_t depth = 0,
                                    const double* K = nullptr, const uint16_t* Z = nullptr, const uint8_t* I_cur = nullptr,
                                    const uint8_t* I_des = nullptr, double* v_p = nullptr, int32_t* p_status = nullptr,
                                    double* normal = nullptr, int32_t* p_info = nullptr) {
    const size_t st_cap = (P + 3) & ~(size_t)3, z_cap = (P * depth_max + 7) & ~(size_t)7, f_cap = (P * frame_max + 15) & ~(size_t)15;
    return PhotometricIo{io_in(8, P * 4, n * 4, K),          io_out(8, P * 6, n * 6, v_p),       io_out(8, P * 28, n * 28, normal),
                         io_out(4, st_cap, n, p_status),     io_out(4, P * 8, n * 8, p_info),    io_in(2, z_cap, n * depth, Z),
                         io_in(1, f_cap, n * frame, I_cur),  io_in(1, f_cap, n * frame, I_des)};
}

// the robust photometric law (vitvs_photometric_robust_velocity): PhotometricIo with the 45 sums in place of the 28 and p_robust
// (gamma, beta, sigma, sum w per pair).  The 45 sums' capacity is rounded to an even count, so that the images still begin on
// 16-byte boundaries.
struct PhotometricRobustIo {
    IoField K, v_p, normal45, p_robust, p_status, p_info, Z, I_cur, I_des;
};
inline PhotometricRobustIo photometric_robust_io(size_t P, size_t frame_max, size_t depth_max, size_t n = 0, size_t frame = 0,
                                                 size_t depth = 0, const double* K = nullptr, const uint16_t* Z = nullptr,
                                                 const uint8_t* I_cur = nullptr, const uint8_t* I_des = nullptr, double* v_p = nullptr,
                                                 int32_t* p_status = nullptr, double* p_robust = nullptr, double* normal45 = nullptr,
                                                 int32_t* p_info = nullptr) {
    const size_t st_cap = (P + 3) & ~(size_t)3, z_cap = (P * depth_max + 7) & ~(size_t)7, f_cap = (P * frame_max + 15) & ~(size_t)15;
    const size_t n45_cap = (P * 45 + 1) & ~(size_t)1;
    return PhotometricRobustIo{io_in(8, P * 4, n * 4, K),          io_out(8, P * 6, n * 6, v_p),      io_out(8, n45_cap, n * 45, normal45),
                               io_out(8, P * 4, n * 4, p_robust),  io_out(4, st_cap, n, p_status),    io_out(4, P * 8, n * 8, p_info),
                               io_in(2, z_cap, n * depth, Z),      io_in(1, f_cap, n * frame, I_cur), io_in(1, f_cap, n * frame, I_des)};
}

// the photometric rig law (vitvs_photometric_rig_velocity): PhotometricRobustIo's per-camera fields, the cameras' twist transforms
// and live flags (null: nothing copied, all live), and the rig's one twist, status, 28 sums and info.  rig_status reserves four
// int32 so that the fields behind it keep their 16-byte boundaries.
struct PhotometricRigIo {
    IoField K, cVr, v_rig, rig_normal, normal45, p_robust, live, rig_status, rig_info, Z, I_cur, I_des;
};
inline PhotometricRigIo photometric_rig_io(size_t P, size_t frame_max, size_t depth_max, size_t n = 0, size_t frame = 0, size_t depth = 0,
                                           const double* K = nullptr, const double* cVr = nullptr, const int32_t* live = nullptr,
                                           const uint16_t* Z = nullptr, const uint8_t* I_cur = nullptr, const uint8_t* I_des = nullptr,
                                           double* v_rig = nullptr, int32_t* rig_status = nullptr, double* p_robust = nullptr,
                                           double* normal45 = nullptr, double* rig_normal = nullptr, int32_t* rig_info = nullptr) {
    const size_t st_cap = (P + 3) & ~(size_t)3, z_cap = (P * depth_max + 7) & ~(size_t)7, f_cap = (P * frame_max + 15) & ~(size_t)15;
    const size_t n45_cap = (P * 45 + 1) & ~(size_t)1;
    return PhotometricRigIo{io_in(8, P * 4, n * 4, K),          io_in(8, P * 36, n * 36, cVr),       io_out(8, 6, 6, v_rig),
                            io_out(8, 28, 28, rig_normal),      io_out(8, n45_cap, n * 45, normal45), io_out(8, P * 4, n * 4, p_robust),
                            io_in(4, st_cap, n, live),          io_out(4, 4, 1, rig_status),         io_out(4, 8, 8, rig_info),
                            io_in(2, z_cap, n * depth, Z),      io_in(1, f_cap, n * frame, I_cur),   io_in(1, f_cap, n * frame, I_des)};
}

// the tile photometric law (vitvs_photometric_tile_velocity): PhotometricRobustIo with the sums and the lighting per tile.  T =
// tiles_y * tiles_x of the call; the block reserves 64 tiles per pair (even capacities: the images keep their 16-byte boundaries).
struct PhotometricTileIo {
    IoField K, v_p, normal45, p_tiles, p_robust, p_status, p_info, Z, I_cur, I_des;
};
inline PhotometricTileIo photometric_tile_io(size_t P, size_t frame_max, size_t depth_max, size_t n = 0, size_t T = 0, size_t frame = 0,
                                             size_t depth = 0, const double* K = nullptr, const uint16_t* Z = nullptr,
                                             const uint8_t* I_cur = nullptr, const uint8_t* I_des = nullptr, double* v_p = nullptr,
                                             int32_t* p_status = nullptr, double* p_robust = nullptr, double* p_tiles = nullptr,
                                             double* normal45 = nullptr, int32_t* p_info = nullptr) {
    const size_t st_cap = (P + 3) & ~(size_t)3, z_cap = (P * depth_max + 7) & ~(size_t)7, f_cap = (P * frame_max + 15) & ~(size_t)15;
    return PhotometricTileIo{io_in(8, P * 4, n * 4, K),          io_out(8, P * 6, n * 6, v_p),
                             io_out(8, P * 64 * 45, n * T * 45, normal45), io_out(8, P * 64 * 4, n * T * 4, p_tiles),
                             io_out(8, P * 4, n * 4, p_robust),  io_out(4, st_cap, n, p_status),    io_out(4, P * 8, n * 8, p_info),
                             io_in(2, z_cap, n * depth, Z),      io_in(1, f_cap, n * frame, I_cur), io_in(1, f_cap, n * frame, I_des)};
}

// the surface photometric law (vitvs_photometric_surface_velocity): PhotometricTileIo with the 120 sums per cell and the lighting
// per node.  T = cells_y * cells_x and Q = (cells_y + 1)(cells_x + 1) of the call; the block reserves 64 cells and 82 nodes (81,
// kept even) per pair.
struct PhotometricSurfaceIo {
    IoField K, v_p, cell_sums, p_nodes, p_robust, p_status, p_info, Z, I_cur, I_des;
};
inline PhotometricSurfaceIo photometric_surface_io(size_t P, size_t frame_max, size_t depth_max, size_t n = 0, size_t T = 0, size_t Q = 0,
                                                   size_t frame = 0, size_t depth = 0, const double* K = nullptr,
                                                   const uint16_t* Z = nullptr, const uint8_t* I_cur = nullptr,
                                                   const uint8_t* I_des = nullptr, double* v_p = nullptr, int32_t* p_status = nullptr,
                                                   double* p_robust = nullptr, double* p_nodes = nullptr, double* cell_sums = nullptr,
                                                   int32_t* p_info = nullptr) {
    const size_t st_cap = (P + 3) & ~(size_t)3, z_cap = (P * depth_max + 7) & ~(size_t)7, f_cap = (P * frame_max + 15) & ~(size_t)15;
    return PhotometricSurfaceIo{io_in(8, P * 4, n * 4, K),          io_out(8, P * 6, n * 6, v_p),
                                io_out(8, P * 64 * 120, n * T * 120, cell_sums), io_out(8, P * 82 * 4, n * Q * 4, p_nodes),
                                io_out(8, P * 4, n * 4, p_robust),  io_out(4, st_cap, n, p_status),    io_out(4, P * 8, n * 8, p_info),
                                io_in(2, z_cap, n * depth, Z),      io_in(1, f_cap, n * frame, I_cur), io_in(1, f_cap, n * frame, I_des)};
}

}  // namespace vitvs
