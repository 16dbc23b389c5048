// The photometric law: direct visual servoing on the luminance of every pixel (Collewet & Marchand), the dense final
// approach behind the ViT laws' dead zone.  Per pair, at pyramid level `level` (s = 2^level): the pooled luminances I of both
// frames, e = I_cur - I_des, the gradient (gx, gy) of the current (interaction 0) or the goal image (1), one interaction row L per
// pooled pixel inside the one-pixel border whose depth is not a hole, and v = -lambda (H + mu diag(H))^-1 g of H = sum L^T L,
// g = sum L^T e.  Two launches:
//   photometric_rows_kernel    one 256-thread workgroup per (band of pooled rows, pair): the integer pooled luminances of the band
//                              and its two halo rows in LDS, the 28 sums of its pixels in fp64 -> one partial per (pair, band)
//   photometric_solve_kernel   one workgroup per pair: four waves fetch the band partials into LDS, one wave adds them in
//                              ascending band order, damps and runs LDL^T (solve.h)
// No float atomics: pixel -> thread -> wave -> band is a function of (H, W, level) alone (plan_photometric), so the sums are the
// same bits from call to call and for a pair alone or anywhere in a batch.  (One launch with a last-arriver ticket in place of the
// second: priced and not built)
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "solve.h"

#pragma clang fp contract(off)

namespace vitvs {

constexpr int kPhotoPart = 32;       // doubles per (pair, band) partial: the 28 sums, then the rows and the holes as two int32

// Y = 77 R + 150 G + 29 B of PX consecutive pixels at p, read as the widest units the caller found p and the row pitch aligned to:
// 16 pixels = three 16-byte loads, 4 pixels = three dwords, 1 pixel = three bytes
template <int PX>
__device__ __forceinline__ void load_luminance(const uint8_t* __restrict__ p, int (&Y)[PX]) {
    if constexpr (PX == 1) {
        Y[0] = 77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2];
    } else {
        unsigned dw[PX * 3 / 4];
        if constexpr (PX == 16) {
            const u32x4* q = reinterpret_cast<const u32x4*>(p);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const u32x4 d = q[i];
                dw[4 * i] = d[0]; dw[4 * i + 1] = d[1]; dw[4 * i + 2] = d[2]; dw[4 * i + 3] = d[3];
            }
        } else {
            const unsigned* q = reinterpret_cast<const unsigned*>(p);
#pragma unroll
            for (int i = 0; i < 3; ++i) dw[i] = q[i];
        }
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int k = 3 * i;
            const int R = (int)((dw[k >> 2] >> (8 * (k & 3))) & 255u);
            const int G = (int)((dw[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 255u);
            const int B = (int)((dw[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 255u);
            Y[i] = 77 * R + 150 * G + 29 * B;
        }
    }
}

// PX consecutive depth samples as (z << 7) + (z != 0): a block's sum of them is its sum of millimetres (< 2^22) over its count of
// non-zero samples (<= 64)
template <int PX>
__device__ __forceinline__ void load_depth(const uint16_t* __restrict__ p, int (&Zs)[PX]) {
    if constexpr (PX == 1) {
        Zs[0] = ((int)p[0] << 7) + (p[0] != 0 ? 1 : 0);
    } else {
        unsigned dw[PX / 2];
        if constexpr (PX == 8) {
            const u32x4 d = *reinterpret_cast<const u32x4*>(p);
            dw[0] = d[0]; dw[1] = d[1]; dw[2] = d[2]; dw[3] = d[3];
        } else {
            dw[0] = *reinterpret_cast<const unsigned*>(p);
        }
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int z = (int)((dw[i >> 1] >> (16 * (i & 1))) & 0xffffu);
            Zs[i] = (z << 7) + (z != 0 ? 1 : 0);
        }
    }
}

// The values of PX consecutive image columns from col0 on, added into their pooled bins of one LDS row (integer adds: any order);
// at level 0 a bin is one pixel and the value is stored
template <int PX>
__device__ __forceinline__ void add_to_bins(int* __restrict__ lds_row, const int (&val)[PX], int col0, int cols, int level) {
    if (level == 0) {
#pragma unroll
        for (int i = 0; i < PX; ++i)
            if (col0 + i < cols) lds_row[col0 + i] = val[i];
        return;
    }
    int acc = 0, bin = col0 >> level;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        const int col = col0 + i;
        if (col < cols) {
            const int b = col >> level;
            if (b != bin) { atomicAdd(&lds_row[bin], acc); acc = 0; bin = b; }
            acc += val[i];
        }
    }
    atomicAdd(&lds_row[bin], acc);      // (col0 < cols: the unit has a first column, and `bin` is inside the row)
}

// Image rows [fr0, fr1) of one frame (pitch W pixels), columns [0, cols): pooled into LDS rows of w bins, image row fr into LDS row
// (fr >> level) - lr0
template <int PX>
__device__ __forceinline__ void pool_frame(const uint8_t* __restrict__ img, int W, int fr0, int fr1, int cols, int level, int lr0,
                                           int w, int* __restrict__ lum, int tid) {
    const int units = (cols + PX - 1) / PX, total = (fr1 - fr0) * units;
    for (int u = tid; u < total; u += 256) {
        const int k = u / units, cu = u - k * units, fr = fr0 + k, col0 = cu * PX;
        int Y[PX];
        load_luminance<PX>(img + ((size_t)fr * W + col0) * 3, Y);
        add_to_bins<PX>(lum + ((fr >> level) - lr0) * w, Y, col0, cols, level);
    }
}
template <int PX>
__device__ __forceinline__ void pool_depth(const uint16_t* __restrict__ img, int W, int fr0, int fr1, int cols, int level, int lr0,
                                           int w, int* __restrict__ zs, int tid) {
    const int units = (cols + PX - 1) / PX, total = (fr1 - fr0) * units;
    for (int u = tid; u < total; u += 256) {
        const int k = u / units, cu = u - k * units, fr = fr0 + k, col0 = cu * PX;
        int Zs[PX];
        load_depth<PX>(img + (size_t)fr * W + col0, Zs);
        add_to_bins<PX>(zs + ((fr >> level) - lr0) * w, Zs, col0, cols, level);
    }
}

__global__ __launch_bounds__(256) void photometric_rows_kernel(PhotometricArgs a, int h, int w, int rows, int bands) {
    extern __shared__ double photo_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int band = blockIdx.x, pair = blockIdx.y;
    const int H = a.height, W = a.width, level = a.level, s = 1 << level;
    const int r0 = band * rows;                         // the band's pooled rows [r0, r1)
    const int r1 = min(r0 + rows, h);
    double* red = photo_lds;                            // [4][32] the waves' sums; their rows and holes as two int32 in slot 28
                                                        // (no static LDS: the opt-in past 64 KiB counts it on top of the dynamic)
    int* lum_cur = reinterpret_cast<int*>(photo_lds + 4 * kPhotoPart);   // [rows + 2][w], LDS row 0 = pooled row r0 - 1
    int* lum_des = lum_cur + (rows + 2) * w;
    int* zs = lum_des + (rows + 2) * w;                 // [rows][w], LDS row 0 = pooled row r0
    for (int i = tid; i < ((rows + 2) * 2 + rows) * w; i += 256) lum_cur[i] = 0;
    __syncthreads();
    {
        const int p0 = max(r0 - 1, 0), p1 = min(r1 + 1, h), cols = w * s;
        const uint8_t* cur = a.I_cur + (size_t)pair * H * W * 3;
        const uint8_t* des = a.I_des + (size_t)pair * H * W * 3;
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const uint8_t* img = which ? des : cur;
            int* lum = which ? lum_des : lum_cur;
            const unsigned long long addr = (unsigned long long)(uintptr_t)img;
            // the halo rows of the gradient image only: e reads the band's own rows
            const bool halo = which == (a.interaction ? 1 : 0);
            const int f0 = (halo ? p0 : r0) * s, f1 = (halo ? p1 : r1) * s;
            if (W % 16 == 0 && addr % 16 == 0) pool_frame<16>(img, W, f0, f1, cols, level, r0 - 1, w, lum, tid);
            else if (W % 4 == 0 && addr % 4 == 0) pool_frame<4>(img, W, f0, f1, cols, level, r0 - 1, w, lum, tid);
            else pool_frame<1>(img, W, f0, f1, cols, level, r0 - 1, w, lum, tid);
        }
        if (a.Z_mm) {
            const uint16_t* z = a.Z_mm + (size_t)pair * H * W;
            const unsigned long long addr = (unsigned long long)(uintptr_t)z;
            if (W % 8 == 0 && addr % 16 == 0) pool_depth<8>(z, W, r0 * s, r1 * s, cols, level, r0, w, zs, tid);
            else if (W % 2 == 0 && addr % 4 == 0) pool_depth<2>(z, W, r0 * s, r1 * s, cols, level, r0, w, zs, tid);
            else pool_depth<1>(z, W, r0 * s, r1 * s, cols, level, r0, w, zs, tid);
        }
    }
    __syncthreads();
    // the rows of the band's pixels: pixel idx of the band (row-major) belongs to thread idx mod 256, which adds its pixels in
    // ascending idx
    const double* K = a.K + (size_t)pair * 4;
    const double sd = (double)s, inv = 1.0 / (256.0 * sd * sd);          // exact: powers of two
    const double fxp = K[0] / sd, fyp = K[1] / sd;
    const double cxp = (K[2] + 0.5) / sd - 0.5, cyp = (K[3] + 0.5) / sd - 0.5;
    const int* grad = a.interaction ? lum_des : lum_cur;
    const bool have_z = a.Z_mm != nullptr;
    double acc[28];
#pragma unroll
    for (int q = 0; q < 28; ++q) acc[q] = 0.0;
    int n = 0, holes = 0;
    for (int idx = tid; idx < (r1 - r0) * w; idx += 256) {
        const int lr = idx / w, c = idx - lr * w, r = r0 + lr;
        if (r < 1 || r > h - 2 || c < 1 || c > w - 2) continue;
        const int at = (lr + 1) * w + c;
        double Z = a.depth_scale;
        if (have_z) {
            const int zp = zs[lr * w + c], count = zp & 127;
            if (count == 0) { ++holes; continue; }
            Z = (double)(zp >> 7) / ((double)count * 1000.0);
        }
        const double gx = (double)(grad[at + 1] - grad[at - 1]) * inv * 0.5;      // exact, as the differences of the doubles are
        const double gy = (double)(grad[at + w] - grad[at - w]) * inv * 0.5;
        const double e = (double)(lum_cur[at] - lum_des[at]) * inv;
        const double x = ((double)c - cxp) / fxp, y = ((double)r - cyp) / fyp;
        const double ga = gx * fxp, gb = gy * fyp;
        double L[7];
        L[0] = ga / Z;
        L[1] = gb / Z;
        L[2] = -(x * ga + y * gb) / Z;
        L[3] = -(x * y * ga + (1.0 + y * y) * gb);
        L[4] = (1.0 + x * x) * ga + x * y * gb;
        L[5] = x * gb - y * ga;
        L[6] = e;
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { acc[q] += L[i] * L[j]; ++q; }
#pragma unroll
        for (int i = 0; i < 7; ++i) acc[21 + i] += L[i] * e;
        ++n;
    }
#pragma unroll
    for (int q = 0; q < 28; ++q) {
        const double t = wave_sum(acc[q]);
        if (lane == 0) red[wave * kPhotoPart + q] = t;
    }
    n = wave_sum(n);
    holes = wave_sum(holes);
    if (lane == 0) { int* c = reinterpret_cast<int*>(red + wave * kPhotoPart + 28); c[0] = n; c[1] = holes; }
    __syncthreads();
    double* part = a.ws + ((size_t)pair * bands + band) * kPhotoPart;
    if (tid < 28) {                                     // the four waves in wave order
        double t = red[tid];
        t += red[kPhotoPart + tid];
        t += red[2 * kPhotoPart + tid];
        t += red[3 * kPhotoPart + tid];
        part[tid] = t;
    } else if (tid < 30) {
        const int k = tid - 28;
        const int* c = reinterpret_cast<const int*>(red + 28) + k;
        reinterpret_cast<int32_t*>(part + 28)[k] = c[0] + c[2 * kPhotoPart] + c[4 * kPhotoPart] + c[6 * kPhotoPart];
    }
}

// One workgroup per pair; wave 0 adds and solves.  The band partials come through LDS in chunks of kPhotoChunk bands, which all four
// waves fetch (the next chunk is in flight while wave 0 adds the one before it), so that the adding lanes do not wait a memory
// round trip per band.
constexpr int kPhotoChunk = 64;      // bands per chunk: 64 x 32 doubles = 8 per thread

__global__ __launch_bounds__(256) void photometric_solve_kernel(PhotometricArgs a, int h, int w, int bands, int no_depth) {
    __shared__ double Gs[40 + 8 * 27];                  // solve_ldlt's: the system in [0, 27), its eight slices from 40 on
    __shared__ double chunk[kPhotoChunk * kPhotoPart];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x;
    for (int i = tid; i < 40 + 8 * 27; i += 256) Gs[i] = 0.0;
    const double* part = a.ws + (size_t)pair * bands * kPhotoPart;
    double sum = 0.0;                                   // lanes 0 .. 27 of wave 0: one of the 28 sums each
    int count = 0;                                      // lane 28 of wave 0: the rows; lane 29: the holes
    const int total = no_depth ? 0 : bands * kPhotoPart;
    double held[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int i = tid + 256 * u; held[u] = i < total ? part[i] : 0.0; }
    for (int c0 = 0; c0 < total; c0 += kPhotoChunk * kPhotoPart) {
        __syncthreads();                                // wave 0 is done with the chunk before
#pragma unroll
        for (int u = 0; u < 8; ++u) chunk[tid + 256 * u] = held[u];
        __syncthreads();
        const int next = c0 + kPhotoChunk * kPhotoPart;
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = next + tid + 256 * u; held[u] = i < total ? part[i] : 0.0; }
        if (wave == 0) {
            const int nb = min(kPhotoChunk, bands - c0 / kPhotoPart);
            if (lane < 28) {
                for (int b = 0; b < nb; ++b) sum += chunk[b * kPhotoPart + lane];          // ascending band order
            } else if (lane < 30) {
                const int32_t* c = reinterpret_cast<const int32_t*>(chunk + 28) + (lane - 28);
                for (int b = 0; b < nb; ++b) count += c[b * kPhotoPart * 2];
            }
        }
    }
    if (wave != 0) return;
    const int n = __builtin_amdgcn_readlane(count, 28), holes = __builtin_amdgcn_readlane(count, 29);
    if (a.normal && lane < 28) a.normal[(size_t)pair * 28 + lane] = sum;
    if (lane < 27) {
        // the diagonal of the upper triangle, row-major: 0, 6, 11, 15, 18, 20
        const bool diag = lane == 0 || lane == 6 || lane == 11 || lane == 15 || lane == 18 || lane == 20;
        Gs[40 + lane] = diag ? sum + a.mu * sum : sum;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // same wave: the LDS writes above are visible below
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool solved = false;
    const bool tried = !no_depth && n >= 6;
    if (tried) solved = solve_ldlt(Gs, lane, x);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.v_p[(size_t)pair * 6 + i] = solved ? -a.lambda * x[i] : 0.0;
        a.p_status[pair] = no_depth ? ST_NO_DEPTH : solved ? ST_OK : ST_TOO_FEW;
        if (a.p_info) {
            int32_t* pi = a.p_info + (size_t)pair * 8;
            pi[0] = n; pi[1] = h; pi[2] = w; pi[3] = bands; pi[4] = holes; pi[5] = (tried && !solved) ? 1 : 0; pi[6] = 0; pi[7] = 0;
        }
    }
}

int plan_photometric(int height, int width, int level, int max_pairs, PhotometricPlan* plan) {
    if (!plan || height < 1 || width < 1 || height > 4096 || width > 4096 || level < 0 || level > 3 || max_pairs < 1) return -2;
    const int h = height >> level, w = width >> level;
    if (h < 3 || w < 3) return -2;
    plan->h = h;
    plan->w = w;
    // at most 2048 >> level pooled pixels per band (its LDS), and bands of one row until the image has more than one band per CU
    plan->rows = std::max(1, std::min((2048 >> level) / w, h / 256));
    plan->bands = (h + plan->rows - 1) / plan->rows;
    plan->lds = ((size_t)(plan->rows + 2) * w * 2 + (size_t)plan->rows * w) * sizeof(int) + 4 * kPhotoPart * sizeof(double);
    plan->lds_opt_in = plan->lds > 64 * 1024;
    plan->ws_bytes = (size_t)max_pairs * plan->bands * kPhotoPart * sizeof(double);
    return 0;
}

int launch_photometric(const PhotometricArgs& a, hipStream_t stream) {
    if (a.n_pairs < 1 || a.n_pairs > 65535 || !a.I_cur || !a.I_des || !a.K || !a.ws || !a.v_p || !a.p_status) return -2;
    if (a.interaction < 0 || a.interaction > 1 || !(a.mu >= 0.0) || !(a.mu < __builtin_huge_val())) return -2;
    if (!(a.lambda == a.lambda) || !(a.depth_scale == a.depth_scale)) return -2;
    PhotometricPlan p;
    if (int rc = plan_photometric(a.height, a.width, a.level, a.n_pairs, &p)) return rc;
    const int no_depth = (!a.Z_mm && !(a.depth_scale > 0.0)) ? 1 : 0;
    if (!no_depth) {
        static std::atomic<unsigned long long> raised{0};
        if (p.lds_opt_in && raise_lds_limit(reinterpret_cast<const void*>(photometric_rows_kernel), 160 * 1024, raised)) return -3;
        launch(photometric_rows_kernel, dim3(p.bands, a.n_pairs), dim3(256), p.lds, stream, a, p.h, p.w, p.rows, p.bands);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    launch(photometric_solve_kernel, dim3(a.n_pairs), dim3(256), 0, stream, a, p.h, p.w, p.bands, no_depth);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vitvs
