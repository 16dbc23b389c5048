// Checks csrc/io_layout.h's lists on the CPU (no GPU, no HIP): for every follow-on law at a few (max_pairs, max_rows, n), placed
// in a host buffer of exactly the computed size, the fields do not overlap, each is aligned to its element size, the last one
// ends at the computed total, no call copies more than a field reserves, and writing every field end to end stays inside the
// buffer (which is what the sanitizers watch).
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o io_layout_check io_layout_check.cpp && ./io_layout_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../vit-vs_amd/csrc/io_layout.h"

using namespace vitvs;

static int failures = 0;
#define EXPECT(cond, ...)                          \
    do {                                           \
        if (!(cond)) {                             \
            ++failures;                            \
            printf("FAILED %s: ", #cond);          \
            printf(__VA_ARGS__);                   \
            printf("\n");                          \
        }                                          \
    } while (0)

static void check(const char* law, IoList l, size_t P, size_t R, size_t n) {
    const size_t total = io_place(l, nullptr);
    for (size_t i = 0; i < l.n; ++i) EXPECT(l.f[i].dev == nullptr, "%s field %zu: a pointer without a block", law, i);
    std::vector<unsigned char> block(total);      // exactly the allocation: a byte past it is the sanitizer's
    EXPECT(io_place(l, block.data()) == total, "%s: the size depends on the base", law);
    size_t end = 0, seen8 = 0, seen4 = 0, widest = 8;
    for (size_t i = 0; i < l.n; ++i) {
        const IoField& f = l.f[i];
        const size_t off = (size_t)(f.dev - block.data());
        // 8- and 4-byte fields; the roll search's list ends with its depth image (2-byte elements) and its frames (bytes)
        EXPECT(f.elem == 8 || f.elem == 4 || f.elem == 2 || f.elem == 1, "%s field %zu: element size %zu", law, i, f.elem);
        EXPECT(f.elem <= widest, "%s field %zu: a %zu-byte field behind a %zu-byte one", law, i, f.elem, widest);
        widest = f.elem;
        if (f.elem == 8) seen8 += 1;
        if (f.elem == 4) seen4 += 1;
        if (f.elem < 4) EXPECT(off % 16 == 0, "%s field %zu (an image) at offset %zu is not on a 16-byte boundary", law, i, off);
        EXPECT(off == end, "%s field %zu begins at %zu, the one before it ends at %zu (P %zu R %zu)", law, i, off, end, P, R);
        EXPECT(off % f.elem == 0, "%s field %zu at offset %zu is not aligned to %zu (P %zu R %zu)", law, i, off, f.elem, P, R);
        EXPECT(f.cap > 0 && f.count <= f.cap, "%s field %zu: count %zu, capacity %zu (P %zu R %zu n %zu)", law, i, f.count, f.cap, P, R, n);
        memset(f.dev, (int)(i + 1), f.cap * f.elem);
        end = off + f.cap * f.elem;
    }
    EXPECT(end == total, "%s: the last field ends at %zu, the block at %zu (P %zu R %zu)", law, end, total, P, R);
    for (size_t i = 0; i < l.n; ++i)              // nobody wrote over a neighbour
        for (size_t b = 0; b < l.f[i].cap * l.f[i].elem; ++b)
            if (l.f[i].dev[b] != (unsigned char)(i + 1)) { EXPECT(false, "%s field %zu byte %zu was overwritten", law, i, b); break; }
    EXPECT(seen8 > 0 && seen4 > 0, "%s: %zu 8-byte and %zu 4-byte fields", law, seen8, seen4);
}

int main() {
    const size_t shapes[][3] = {{1, 1, 1}, {3, 8, 2}, {3, 8, 3}, {8, 24, 5}, {256, 48, 3}, {256, 3136, 256}};
    double d = 0;                                  // any non-null caller pointer: the layout does not read it
    int32_t i = 0;
    for (const auto& s : shapes) {
        const size_t P = s[0], R = s[1], n = s[2];
        RigIo rig = rig_io(P, R, n, &d, &i, nullptr, &d, &i, &i, &d);
        check("rig", io_list(rig), P, R, n);
        RigIo robust = rig_io(P, R, n, &d, &i, &d, &d, &i, &i, &d, &d, &d);
        check("rig robust", io_list(robust), P, R, n);
        EXPECT(io_place(io_list(rig), nullptr) == io_place(io_list(robust), nullptr), "the rig law's two forms share one block");
        PoseIo pose = pose_io(P, R, n, &d, &i, &d, &i, &d, &i, &d, &d);
        check("pose", io_list(pose), P, R, n);
        HomographyIo hom = homography_io(P, R, n, &d, &i, &d, &i, &d, &i, &d, &d);
        check("homography", io_list(hom), P, R, n);
        PoseRigIo pose_rig = pose_rig_io(P, R, n, &d, &d, &i, &d, &i, &d, &i, &d, &d, &d);
        check("pose rig", io_list(pose_rig), P, R, n);
        // the sizes *_prepare allocates (the lists of P and R alone) are the sizes the calls place their fields in
        RigIo rig0 = rig_io(P, R);
        PoseIo pose0 = pose_io(P, R);
        HomographyIo hom0 = homography_io(P, R);
        PoseRigIo pose_rig0 = pose_rig_io(P, R);
        EXPECT(io_place(io_list(rig0), nullptr) == io_place(io_list(rig), nullptr), "rig: allocation and call disagree");
        EXPECT(io_place(io_list(pose0), nullptr) == io_place(io_list(pose), nullptr), "pose: allocation and call disagree");
        EXPECT(io_place(io_list(hom0), nullptr) == io_place(io_list(hom), nullptr), "homography: allocation and call disagree");
        EXPECT(io_place(io_list(pose_rig0), nullptr) == io_place(io_list(pose_rig), nullptr), "pose rig: allocation and call disagree");
        // and the sizes in closed form, from the fields' shapes in include/vitvs.h
        EXPECT(io_place(io_list(pose0), nullptr) == (P * (4 + 6 + 12 + 1 + R)) * 8 + P * 10 * 4, "pose: %zu %zu", P, R);
        EXPECT(io_place(io_list(hom0), nullptr) == (P * (4 + 6 + 9 + 1 + R)) * 8 + P * 10 * 4, "homography: %zu %zu", P, R);
        EXPECT(io_place(io_list(pose_rig0), nullptr) == (P * (12 + 4 + R) + 6 + 12 + 18 + 1) * 8 + (P + 9) * 4, "pose rig: %zu %zu", P, R);
        EXPECT(io_place(io_list(rig0), nullptr) == (P * 36 + 34 + P * 4 + 1 + P * R) * 8 + (P + 9) * 4, "rig: %zu %zu", P, R);
    }
    // the roll search: one pair; T tokens, R rows, S x S x 3 frame bytes, u_max x v_max depth pixels
    const size_t rolls[][5] = {{16, 48, 64, 640, 480}, {196, 48, 224, 640, 480}, {196, 196, 224, 480, 480}, {484, 24, 308, 641, 479},
                               {3136, 3136, 448, 1280, 720}, {1, 1, 16, 1, 1}};
    uint8_t b8 = 0;
    uint16_t b16 = 0;
    for (const auto& r : rolls) {
        const size_t T = r[0], R = r[1], frame = r[2] * r[2] * 3, depth = r[3] * r[4];
        for (size_t n_sel : {(size_t)0, R < T ? R : T, T}) {
            RollIo roll = roll_io(T, R, frame, depth, n_sel, &d, &i, &i, &b16, &b8, &b8, &d, &i, &i, &d);
            check("roll", io_list(roll), T, R, n_sel);
            RollIo roll0 = roll_io(T, R, frame, depth);
            EXPECT(io_place(io_list(roll0), nullptr) == io_place(io_list(roll), nullptr), "roll: allocation and call disagree");
            EXPECT(roll.Z.count == depth && roll.I_cur.count == frame && roll.selection.count == n_sel, "roll: counts");
        }
    }
    // the photometric law: P pairs at v_max x u_max, a call of n pairs at height x width
    const size_t photos[][6] = {{1, 640, 480, 1, 640, 480}, {1, 640, 480, 1, 37, 29}, {3, 641, 479, 2, 96, 88}, {8, 640, 480, 8, 224, 224},
                                {8, 1280, 720, 5, 1, 1}, {2, 3, 3, 2, 3, 3}};
    for (const auto& q : photos) {
        const size_t P = q[0], px_max = q[1] * q[2], n = q[3], px = q[4] * q[5];
        PhotometricIo ph = photometric_io(P, px_max * 3, px_max, n, px * 3, px, &d, &b16, &b8, &b8, &d, &i, &d, &i);
        check("photometric", io_list(ph), P, px_max, n);
        PhotometricIo ph0 = photometric_io(P, px_max * 3, px_max);
        EXPECT(io_place(io_list(ph0), nullptr) == io_place(io_list(ph), nullptr), "photometric: allocation and call disagree");
        EXPECT(ph.Z.count == n * px && ph.I_cur.count == n * px * 3 && ph.I_des.count == n * px * 3 && ph.normal.count == n * 28,
               "photometric: counts");
        EXPECT(io_place(io_list(ph0), nullptr) == P * (4 + 6 + 28) * 8 + (((P + 3) & ~(size_t)3) + P * 8) * 4 +
                                                      ((P * px_max + 7) & ~(size_t)7) * 2 + 2 * ((P * px_max * 3 + 15) & ~(size_t)15),
               "photometric: %zu %zu", P, px_max);
        // its robust form: the 45 sums (an even capacity) and p_robust
        PhotometricRobustIo pr = photometric_robust_io(P, px_max * 3, px_max, n, px * 3, px, &d, &b16, &b8, &b8, &d, &i, &d, &d, &i);
        check("photometric robust", io_list(pr), P, px_max, n);
        PhotometricRobustIo pr0 = photometric_robust_io(P, px_max * 3, px_max);
        EXPECT(io_place(io_list(pr0), nullptr) == io_place(io_list(pr), nullptr), "photometric robust: allocation and call disagree");
        EXPECT(pr.Z.count == n * px && pr.I_cur.count == n * px * 3 && pr.I_des.count == n * px * 3 && pr.normal45.count == n * 45 &&
                   pr.p_robust.count == n * 4,
               "photometric robust: counts");
        EXPECT(io_place(io_list(pr0), nullptr) == (P * (4 + 6 + 4) + ((P * 45 + 1) & ~(size_t)1)) * 8 + (((P + 3) & ~(size_t)3) + P * 8) * 4 +
                                                      ((P * px_max + 7) & ~(size_t)7) * 2 + 2 * ((P * px_max * 3 + 15) & ~(size_t)15),
               "photometric robust: %zu %zu", P, px_max);
        // the rig form: the cameras' twist transforms and live flags, and the rig's twist, 28 sums, status (four reserved) and info
        PhotometricRigIo pg = photometric_rig_io(P, px_max * 3, px_max, n, px * 3, px, &d, &d, &i, &b16, &b8, &b8, &d, &i, &d, &d, &d, &i);
        check("photometric rig", io_list(pg), P, px_max, n);
        PhotometricRigIo pg0 = photometric_rig_io(P, px_max * 3, px_max);
        EXPECT(io_place(io_list(pg0), nullptr) == io_place(io_list(pg), nullptr), "photometric rig: allocation and call disagree");
        EXPECT(pg.Z.count == n * px && pg.I_cur.count == n * px * 3 && pg.I_des.count == n * px * 3 && pg.normal45.count == n * 45 &&
                   pg.p_robust.count == n * 4 && pg.cVr.count == n * 36 && pg.live.count == n && pg.v_rig.count == 6 &&
                   pg.rig_normal.count == 28 && pg.rig_status.count == 1 && pg.rig_info.count == 8,
               "photometric rig: counts");
        EXPECT(io_place(io_list(pg0), nullptr) ==
                   (P * (4 + 36 + 4) + 6 + 28 + ((P * 45 + 1) & ~(size_t)1)) * 8 + (((P + 3) & ~(size_t)3) + 4 + 8) * 4 +
                       ((P * px_max + 7) & ~(size_t)7) * 2 + 2 * ((P * px_max * 3 + 15) & ~(size_t)15),
               "photometric rig: %zu %zu", P, px_max);
        // the tile form: the sums and the lighting per tile, 64 tiles reserved per pair, T of them in a call
        for (size_t T : {(size_t)1, (size_t)15, (size_t)64}) {
            PhotometricTileIo pt = photometric_tile_io(P, px_max * 3, px_max, n, T, px * 3, px, &d, &b16, &b8, &b8, &d, &i, &d, &d, &d, &i);
            check("photometric tile", io_list(pt), P, px_max, n);
            PhotometricTileIo pt0 = photometric_tile_io(P, px_max * 3, px_max);
            EXPECT(io_place(io_list(pt0), nullptr) == io_place(io_list(pt), nullptr), "photometric tile: allocation and call disagree");
            EXPECT(pt.Z.count == n * px && pt.I_cur.count == n * px * 3 && pt.I_des.count == n * px * 3 &&
                       pt.normal45.count == n * T * 45 && pt.p_tiles.count == n * T * 4 && pt.p_robust.count == n * 4,
                   "photometric tile: counts");
            EXPECT(io_place(io_list(pt0), nullptr) == P * (4 + 6 + 64 * 45 + 64 * 4 + 4) * 8 + (((P + 3) & ~(size_t)3) + P * 8) * 4 +
                                                          ((P * px_max + 7) & ~(size_t)7) * 2 + 2 * ((P * px_max * 3 + 15) & ~(size_t)15),
                   "photometric tile: %zu %zu", P, px_max);
        }
        // the surface form: the 120 sums per cell and the lighting per node, 64 cells and 82 nodes reserved per pair
        for (size_t g : {(size_t)1, (size_t)3, (size_t)8}) {
            const size_t T = g * g, Q = (g + 1) * (g + 1);
            PhotometricSurfaceIo ps = photometric_surface_io(P, px_max * 3, px_max, n, T, Q, px * 3, px, &d, &b16, &b8, &b8, &d, &i, &d, &d, &d, &i);
            check("photometric surface", io_list(ps), P, px_max, n);
            PhotometricSurfaceIo ps0 = photometric_surface_io(P, px_max * 3, px_max);
            EXPECT(io_place(io_list(ps0), nullptr) == io_place(io_list(ps), nullptr), "photometric surface: allocation and call disagree");
            EXPECT(ps.Z.count == n * px && ps.I_cur.count == n * px * 3 && ps.I_des.count == n * px * 3 &&
                       ps.cell_sums.count == n * T * 120 && ps.p_nodes.count == n * Q * 4 && ps.p_robust.count == n * 4,
                   "photometric surface: counts");
            EXPECT(io_place(io_list(ps0), nullptr) == P * (4 + 6 + 64 * 120 + 82 * 4 + 4) * 8 + (((P + 3) & ~(size_t)3) + P * 8) * 4 +
                                                          ((P * px_max + 7) & ~(size_t)7) * 2 + 2 * ((P * px_max * 3 + 15) & ~(size_t)15),
                   "photometric surface: %zu %zu", P, px_max);
        }
    }
    if (failures) printf("io_layout_check: %d FAILED\n", failures);
    else printf("io_layout_check: ok\n");
    return failures ? 1 : 0;
}
