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
// second: priced and not built)  The law's robust form has kernels of its own further down, and its
// rig form two more behind them, and its tile form three at the end of the file.
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

// ---- the robust photometric law ---------------------------------------------------------------------------------
// The plain law's rows under a lighting model I_cur ~ (1 + gamma) I_des + beta and Tukey weights: N + 1 weighted solves with a
// re-weighting between two of them, 3 N + 2 launches and no host round trip (kernels.h PhotometricRobustArgs).  The same band plan
// and the same pixel -> thread -> wave -> band order as above; the median of the residuals comes from a histogram of integer
// counts (integer atomics only: order-free), so every pass is the same bits from call to call.
//   photometric_robust_rows_kernel<WEIGHTED>   the 45 weighted sums of a band; WEIGHTED (passes >= 1): sigma from the pair's
//                                              histogram (every workgroup for itself), w from the state of the solve before
//   photometric_residual_kernel                rho of the band's rows into an LDS histogram, its non-empty bins into the pair's
//   photometric_robust_solve_kernel            the bands in ascending order, the 2 x 2 elimination of (gamma, beta), LDL^T; writes
//                                              the state and clears the histogram
constexpr int kPhotoRPart = 48;      // doubles per (pair, band) partial: the 45 sums, rows and holes as two int32, the zero weights
constexpr int kPhotoBins = 4096;     // histogram bins of 1 / 16 grey level; the last one takes everything from 256 grey levels on
constexpr int kPhotoState = 16;      // doubles per pair: x (6), gamma, beta, sigma, (int32 rows, int32 failed), (int32 median bin)
constexpr double kTukeyC = 4.6851, kMadScale = 1.4826;

// the pooled luminances (and depth) of the band [r0, r1) into LDS, as photometric_rows_kernel's first half; ends on a barrier
__device__ __forceinline__ void pool_band(const PhotometricArgs& a, int pair, int h, int w, int rows, int r0, int r1, int* lum_cur,
                                          int* lum_des, int* zs, int tid) {
    const int H = a.height, W = a.width, level = a.level, s = 1 << level;
    for (int i = tid; i < ((rows + 2) * 2 + rows) * w; i += 256) lum_cur[i] = 0;
    __syncthreads();
    const int p0 = max(r0 - 1, 0), p1 = min(r1 + 1, h), cols = w * s;
    const uint8_t* cur = a.I_cur + (size_t)pair * H * W * 3;
    const uint8_t* des = a.I_des + (size_t)pair * H * W * 3;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        const uint8_t* img = which ? des : cur;
        int* lum = which ? lum_des : lum_cur;
        const unsigned long long addr = (unsigned long long)(uintptr_t)img;
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
    __syncthreads();
}

// what a row needs of the intrinsics at the pooled scale
struct PhotoCamera {
    double fxp, fyp, cxp, cyp, inv;
};
__device__ __forceinline__ PhotoCamera photo_camera(const double* K, int level) {
    const double sd = (double)(1 << level);
    return PhotoCamera{K[0] / sd, K[1] / sd, (K[2] + 0.5) / sd - 0.5, (K[3] + 0.5) / sd - 0.5, 1.0 / (256.0 * sd * sd)};
}

// The row of pooled pixel (r, c), LDS row lr of the band: L, e and D in photometric_rows_kernel's operations.  0: a row; 1: the
// border, no row; 2: a hole, no row.
__device__ __forceinline__ int photo_row(const PhotoCamera& k, const int* grad, const int* lum_cur, const int* lum_des, const int* zs,
                                         bool have_z, double depth_scale, int h, int w, int lr, int c, int r, double (&L)[6], double& e,
                                         double& D) {
    if (r < 1 || r > h - 2 || c < 1 || c > w - 2) return 1;
    const int at = (lr + 1) * w + c;
    double Z = depth_scale;
    if (have_z) {
        const int zp = zs[lr * w + c], count = zp & 127;
        if (count == 0) return 2;
        Z = (double)(zp >> 7) / ((double)count * 1000.0);
    }
    const double gx = (double)(grad[at + 1] - grad[at - 1]) * k.inv * 0.5;
    const double gy = (double)(grad[at + w] - grad[at - w]) * k.inv * 0.5;
    e = (double)(lum_cur[at] - lum_des[at]) * k.inv;
    D = (double)lum_des[at] * k.inv;
    const double x = ((double)c - k.cxp) / k.fxp, y = ((double)r - k.cyp) / k.fyp;
    const double ga = gx * k.fxp, gb = gy * k.fyp;
    L[0] = ga / Z;
    L[1] = gb / Z;
    L[2] = -(x * ga + y * gb) / Z;
    L[3] = -(x * y * ga + (1.0 + y * y) * gb);
    L[4] = (1.0 + x * x) * ga + x * y * gb;
    L[5] = x * gb - y * ga;
    return 0;
}

// rho = |((e + L.x) - gamma D) - beta|, st = the pair's state
__device__ __forceinline__ double photo_rho(const double (&L)[6], double e, double D, const double (&st)[8]) {
    double p = L[0] * st[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) p += L[i] * st[i];
    return fabs(((e + p) - st[6] * D) - st[7]);
}

// The first bin at which the cumulative count of the pair's histogram reaches `need`, by all 256 threads (16 bins each); scan[257]
// is LDS.  Ends on a barrier.  (need < 1 or past the total: 0)
__device__ __forceinline__ int photo_median_bin(const uint32_t* __restrict__ hist, int need, int* scan, int tid) {
    unsigned c[16];
    const u32x4* q = reinterpret_cast<const u32x4*>(hist + tid * 16);
    int mine = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u32x4 d = q[i];
        c[4 * i] = d[0]; c[4 * i + 1] = d[1]; c[4 * i + 2] = d[2]; c[4 * i + 3] = d[3];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) mine += (int)c[i];
    scan[tid] = mine;
    if (tid == 0) scan[256] = 0;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int below = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += below;
        __syncthreads();
    }
    const int upto = scan[tid], before = upto - mine;
    if (before < need && upto >= need) {                // one thread: the counts are integers
        int cum = before, bin = 15;
        bool found = false;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            cum += (int)c[i];
            if (!found && cum >= need) { bin = i; found = true; }
        }
        scan[256] = tid * 16 + bin;
    }
    __syncthreads();
    return scan[256];
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void photometric_robust_rows_kernel(PhotometricRobustArgs ra, int h, int w, int rows, int bands) {
    extern __shared__ double photo_lds[];
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int band = blockIdx.x, pair = blockIdx.y;
    const int r0 = band * rows, r1 = min(r0 + rows, h);
    double* red = photo_lds;                            // [4][48]; before the sums, the scan of the histogram (257 int32)
    int* lum_cur = reinterpret_cast<int*>(photo_lds + 4 * kPhotoRPart);
    int* lum_des = lum_cur + (rows + 2) * w;
    int* zs = lum_des + (rows + 2) * w;
    double st[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double scale = 1.0;                                 // kTukeyC * sigma
    if constexpr (WEIGHTED) {
        double* state = ra.state + (size_t)pair * kPhotoState;
        const int32_t* si = reinterpret_cast<const int32_t*>(state + 9);
        if (si[1]) return;                              // a solve before this one failed: the call's answer is written
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = state[i];
        const int bin = photo_median_bin(ra.hist + (size_t)pair * kPhotoBins, (si[0] + 1) / 2, reinterpret_cast<int*>(red), tid);
        const double median = ((double)bin + 0.5) / 16.0;
        const double sigma = fmax(kMadScale * median, ra.sigma_min);
        scale = kTukeyC * sigma;
        if (band == 0 && tid == 0) { state[8] = sigma; reinterpret_cast<int32_t*>(state + 10)[0] = bin; }
    }
    pool_band(a, pair, h, w, rows, r0, r1, lum_cur, lum_des, zs, tid);
    const PhotoCamera cam = photo_camera(a.K + (size_t)pair * 4, a.level);
    const int* grad = a.interaction ? lum_des : lum_cur;
    const bool have_z = a.Z_mm != nullptr;
    double acc[45];
#pragma unroll
    for (int q = 0; q < 45; ++q) acc[q] = 0.0;
    int n = 0, holes = 0, zeros = 0;
    for (int idx = tid; idx < (r1 - r0) * w; idx += 256) {
        const int lr = idx / w, c = idx - lr * w, r = r0 + lr;
        double L[6], e, D;
        const int kind = photo_row(cam, grad, lum_cur, lum_des, zs, have_z, a.depth_scale, h, w, lr, c, r, L, e, D);
        if (kind == 2) ++holes;
        if (kind != 0) continue;
        double wt = 1.0;
        if constexpr (WEIGHTED) {
            const double t = photo_rho(L, e, D, st) / scale;
            const double u = 1.0 - t * t;
            wt = t < 1.0 ? u * u : 0.0;
            if (wt == 0.0) ++zeros;
        }
        double wv[8];
#pragma unroll
        for (int i = 0; i < 6; ++i) wv[i] = wt * L[i];
        wv[6] = wt * e;
        wv[7] = wt * D;
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { acc[q] += wv[i] * L[j]; ++q; }
#pragma unroll
        for (int i = 0; i < 7; ++i) acc[21 + i] += wv[i] * e;
#pragma unroll
        for (int i = 0; i < 6; ++i) { acc[28 + 2 * i] += wv[i] * D; acc[29 + 2 * i] += wv[i]; }
        acc[40] += wv[7] * D;
        acc[41] += wv[7];
        acc[42] += wt;
        acc[43] += wv[7] * e;
        acc[44] += wv[6];
        ++n;
    }
    __syncthreads();                                    // (WEIGHTED: the scan is read; `red` is the sums' from here)
#pragma unroll
    for (int q = 0; q < 45; ++q) {
        const double t = wave_sum(acc[q]);
        if (lane == 0) red[wave * kPhotoRPart + q] = t;
    }
    n = wave_sum(n);
    holes = wave_sum(holes);
    zeros = wave_sum(zeros);
    if (lane == 0) { int* c = reinterpret_cast<int*>(red + wave * kPhotoRPart + 45); c[0] = n; c[1] = holes; c[2] = zeros; c[3] = 0; }
    __syncthreads();
    double* part = a.ws + ((size_t)pair * bands + band) * kPhotoRPart;
    if (tid < 45) {                                     // the four waves in wave order
        double t = red[tid];
        t += red[kPhotoRPart + tid];
        t += red[2 * kPhotoRPart + tid];
        t += red[3 * kPhotoRPart + tid];
        part[tid] = t;
    } else if (tid < 49) {
        const int k = tid - 45;
        const int* c = reinterpret_cast<const int*>(red + 45) + k;
        reinterpret_cast<int32_t*>(part + 45)[k] = c[0] + c[2 * kPhotoRPart] + c[4 * kPhotoRPart] + c[6 * kPhotoRPart];
    }
}

__global__ __launch_bounds__(256) void photometric_residual_kernel(PhotometricRobustArgs ra, int h, int w, int rows, int bands) {
    extern __shared__ double photo_lds[];
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, band = blockIdx.x, pair = blockIdx.y;
    const int r0 = band * rows, r1 = min(r0 + rows, h);
    int* lum_cur = reinterpret_cast<int*>(photo_lds + 4 * kPhotoRPart);          // the rows launch's layout, the histogram behind it
    int* lum_des = lum_cur + (rows + 2) * w;
    int* zs = lum_des + (rows + 2) * w;
    unsigned* bins = reinterpret_cast<unsigned*>(zs + rows * w);
    const double* state = ra.state + (size_t)pair * kPhotoState;
    if (reinterpret_cast<const int32_t*>(state + 9)[1]) return;
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = state[i];
    for (int i = tid; i < kPhotoBins; i += 256) bins[i] = 0u;
    pool_band(a, pair, h, w, rows, r0, r1, lum_cur, lum_des, zs, tid);          // (its barriers order the zeros above too)
    const PhotoCamera cam = photo_camera(a.K + (size_t)pair * 4, a.level);
    const int* grad = a.interaction ? lum_des : lum_cur;
    const bool have_z = a.Z_mm != nullptr;
    for (int idx = tid; idx < (r1 - r0) * w; idx += 256) {
        const int lr = idx / w, c = idx - lr * w, r = r0 + lr;
        double L[6], e, D;
        if (photo_row(cam, grad, lum_cur, lum_des, zs, have_z, a.depth_scale, h, w, lr, c, r, L, e, D) != 0) continue;
        const double rho = photo_rho(L, e, D, st);
        const int q = rho < (double)(kPhotoBins / 16) ? (int)(16.0 * rho) : kPhotoBins - 1;      // (a NaN: the last bin)
        atomicAdd(&bins[q], 1u);
    }
    __syncthreads();
    unsigned* hist = ra.hist + (size_t)pair * kPhotoBins;
    for (int i = tid; i < kPhotoBins; i += 256) {
        const unsigned cnt = bins[i];
        if (cnt) atomicAdd(&hist[i], cnt);
    }
}

constexpr int kPhotoRChunk = 64;     // bands per chunk: 64 x 48 doubles = 12 per thread

__global__ __launch_bounds__(256) void photometric_robust_solve_kernel(PhotometricRobustArgs ra, int h, int w, int bands, int no_depth,
                                                                       int pass) {
    __shared__ double Gs[40 + 8 * 27];
    __shared__ double S[kPhotoRPart];
    __shared__ double chunk[kPhotoRChunk * kPhotoRPart];
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x;
    unsigned* hist = ra.hist + (size_t)pair * kPhotoBins;                         // read by this pass's rows launch; the next
    for (int i = tid; i < kPhotoBins; i += 256) hist[i] = 0u;                    // re-weighting (this call's or the next's) fills it
    double* state = ra.state + (size_t)pair * kPhotoState;
    int32_t* si = reinterpret_cast<int32_t*>(state + 9);
    if (pass > 0 && si[1]) return;
    for (int i = tid; i < 40 + 8 * 27; i += 256) Gs[i] = 0.0;
    const double* part = a.ws + (size_t)pair * bands * kPhotoRPart;
    double sum = 0.0;                                   // lanes 0 .. 44 of wave 0: one of the 45 sums each
    int count = 0;                                      // lane 45: the rows; 46: the holes; 47: the rows of weight 0
    const int total = no_depth ? 0 : bands * kPhotoRPart;
    double held[12];
#pragma unroll
    for (int u = 0; u < 12; ++u) { const int i = tid + 256 * u; held[u] = i < total ? part[i] : 0.0; }
    for (int c0 = 0; c0 < total; c0 += kPhotoRChunk * kPhotoRPart) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 12; ++u) chunk[tid + 256 * u] = held[u];
        __syncthreads();
        const int next = c0 + kPhotoRChunk * kPhotoRPart;
#pragma unroll
        for (int u = 0; u < 12; ++u) { const int i = next + tid + 256 * u; held[u] = i < total ? part[i] : 0.0; }
        if (wave == 0) {
            const int nb = min(kPhotoRChunk, bands - c0 / kPhotoRPart);
            if (lane < 45) {
                for (int b = 0; b < nb; ++b) sum += chunk[b * kPhotoRPart + lane];         // ascending band order
            } else if (lane < 48) {
                const int32_t* c = reinterpret_cast<const int32_t*>(chunk + 45) + (lane - 45);
                for (int b = 0; b < nb; ++b) count += c[b * kPhotoRPart * 2];
            }
        }
    }
    if (wave != 0) return;
    const int n = __builtin_amdgcn_readlane(count, 45), holes = __builtin_amdgcn_readlane(count, 46);
    const int zeros = __builtin_amdgcn_readlane(count, 47);
    if (ra.normal45 && lane < 45) ra.normal45[(size_t)pair * 45 + lane] = sum;
    if (lane < 45) S[lane] = sum;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // same wave: the LDS writes above are visible below
    // C = [[S40, S41], [S41, S42]] = l d l^T under solve_ldlt's pivot rule; z = C^-1 (p, q): z1 = (q - l p) / d1, z0 = p / d0 - l z1
    bool cgood = true;
    double l = 0.0, i0 = 0.0, i1 = 0.0;
    if (ra.illumination) {
        const double DD = S[40], Dm = S[41], Sw = S[42];
        const double d0 = DD;
        cgood = (d0 > kPivotThreshold * DD) && (DD > 0.0);
        i0 = 1.0 / d0;
        l = Dm * i0;
        const double d1 = Sw - l * l * d0;
        cgood = cgood && (d1 > kPivotThreshold * Sw) && (Sw > 0.0);
        i1 = 1.0 / d1;
    }
    if (lane < 27) {
        double val = sum;
        if (ra.illumination) {
            int i, j = 0;
            if (lane < 21) {
                int q = lane;
                i = 0;
                while (q >= 6 - i) { q -= 6 - i; ++i; }
                j = i + q;
            } else {
                i = lane - 21;
            }
            const double p = S[28 + 2 * i], q1 = S[29 + 2 * i];
            const double u1 = (q1 - l * p) * i1, u0 = p * i0 - l * u1;
            const double o0 = lane < 21 ? S[28 + 2 * j] : S[43], o1 = lane < 21 ? S[29 + 2 * j] : S[44];
            val = sum - (u0 * o0 + u1 * o1);
        }
        const bool diag = lane == 0 || lane == 6 || lane == 11 || lane == 15 || lane == 18 || lane == 20;
        Gs[40 + lane] = diag ? val + a.mu * val : val;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool solved = false;
    const bool tried = !no_depth && n >= 6 && n - zeros >= 6;
    if (tried && cgood) solved = solve_ldlt(Gs, lane, x);
    double gamma = 0.0, beta = 0.0;
    if (solved && ra.illumination) {
        double t0 = S[43], t1 = S[44];
#pragma unroll
        for (int i = 0; i < 6; ++i) { t0 = t0 + S[28 + 2 * i] * -x[i]; t1 = t1 + S[29 + 2 * i] * -x[i]; }
        beta = (t1 - l * t0) * i1;
        gamma = t0 * i0 - l * beta;
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            state[i] = -x[i];
            a.v_p[(size_t)pair * 6 + i] = solved ? -a.lambda * x[i] : 0.0;
        }
        state[6] = gamma;
        state[7] = beta;
        si[0] = n;
        si[1] = solved ? 0 : 1;
        a.p_status[pair] = no_depth ? ST_NO_DEPTH : solved ? ST_OK : ST_TOO_FEW;
        if (a.p_info) {
            int32_t* pi = a.p_info + (size_t)pair * 8;
            pi[0] = n; pi[1] = h; pi[2] = w; pi[3] = bands; pi[4] = holes; pi[5] = (tried && !solved) ? 1 : 0; pi[6] = zeros; pi[7] = pass;
        }
        double* pr = ra.p_robust + (size_t)pair * 4;
        pr[0] = gamma;
        pr[1] = beta;
        pr[2] = (solved && pass > 0) ? state[8] : 0.0;
        pr[3] = solved ? S[42] : 0.0;
    }
}

size_t photometric_robust_ws_bytes(int max_pairs) {
    return (size_t)max_pairs * ((size_t)4096 * kPhotoRPart * sizeof(double) + kPhotoBins * sizeof(uint32_t) + kPhotoState * sizeof(double));
}

int launch_photometric_robust(const PhotometricRobustArgs& ra_in, unsigned char* ws, int max_pairs, hipStream_t stream) {
    PhotometricRobustArgs ra = ra_in;
    PhotometricArgs& a = ra.p;
    if (a.n_pairs < 1 || a.n_pairs > 65535 || a.n_pairs > max_pairs || !a.I_cur || !a.I_des || !a.K || !ws || !a.v_p || !a.p_status ||
        !ra.p_robust)
        return -2;
    if (a.interaction < 0 || a.interaction > 1 || !(a.mu >= 0.0) || !(a.mu < __builtin_huge_val())) return -2;
    if (!(a.lambda == a.lambda) || !(a.depth_scale == a.depth_scale)) return -2;
    if (ra.illumination < 0 || ra.illumination > 1 || ra.iterations < 0 || ra.iterations > 4) return -2;
    if (!(ra.sigma_min > 0.0) || !(ra.sigma_min < __builtin_huge_val())) return -2;
    PhotometricPlan p;
    if (int rc = plan_photometric(a.height, a.width, a.level, a.n_pairs, &p)) return rc;
    // the block: the partials of max_pairs pairs at 4096 bands, then the histograms, then the states
    a.ws = reinterpret_cast<double*>(ws);
    ra.hist = reinterpret_cast<uint32_t*>(ws + (size_t)max_pairs * 4096 * kPhotoRPart * sizeof(double));
    ra.state = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(ra.hist) + (size_t)max_pairs * kPhotoBins * sizeof(uint32_t));
    const size_t lds = p.lds - 4 * kPhotoPart * sizeof(double) + 4 * kPhotoRPart * sizeof(double);
    const size_t lds_res = lds + kPhotoBins * sizeof(uint32_t);
    const int no_depth = (!a.Z_mm && !(a.depth_scale > 0.0)) ? 1 : 0;
    if (no_depth) {
        launch(photometric_robust_solve_kernel, dim3(a.n_pairs), dim3(256), 0, stream, ra, p.h, p.w, p.bands, 1, 0);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    static std::atomic<unsigned long long> raised0{0}, raised1{0}, raised2{0};
    if (lds > 64 * 1024 &&
        (raise_lds_limit(reinterpret_cast<const void*>(photometric_robust_rows_kernel<false>), 160 * 1024, raised0) ||
         raise_lds_limit(reinterpret_cast<const void*>(photometric_robust_rows_kernel<true>), 160 * 1024, raised1)))
        return -3;
    if (ra.iterations > 0 && lds_res > 64 * 1024 &&
        raise_lds_limit(reinterpret_cast<const void*>(photometric_residual_kernel), 160 * 1024, raised2))
        return -3;
    const dim3 grid(p.bands, a.n_pairs);
    for (int pass = 0; pass <= ra.iterations; ++pass) {
        if (pass > 0) {
            launch(photometric_residual_kernel, grid, dim3(256), lds_res, stream, ra, p.h, p.w, p.rows, p.bands);
            launch(photometric_robust_rows_kernel<true>, grid, dim3(256), lds, stream, ra, p.h, p.w, p.rows, p.bands);
        } else {
            launch(photometric_robust_rows_kernel<false>, grid, dim3(256), lds, stream, ra, p.h, p.w, p.rows, p.bands);
        }
        if (hipGetLastError() != hipSuccess) return -1;
        launch(photometric_robust_solve_kernel, dim3(a.n_pairs), dim3(256), 0, stream, ra, p.h, p.w, p.bands, 0, pass);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

// ---- the photometric rig law --------------------------------------------------------------------------------------
// The robust law's rows of n_cams cameras of one rigid rig in ONE system: camera i's 45 sums, its own (gamma_i, beta_i) eliminated,
// carried into the rig frame by its twist transform W_i = cVr[i] (T_i = W_i^T H'_i W_i, W_i^T g'_i) and added in camera order; one
// 6 x 6 solve, and one median over all cameras' residuals.  The rows and residual launches are the robust law's own, a camera being
// a pair: they read (x_i, gamma_i, beta_i, rows, failed) from the camera's state block and the median at (rows + 1) / 2 of the
// camera's histogram, so the rig solve writes n_total into every camera's rows field and the merge launch makes every live
// camera's histogram the stack's.  4 N + 2 launches (kernels.h PhotometricRigArgs).
//   photometric_rig_solve_kernel   one workgroup per call: wave v takes cameras v, v + 4, ..: the bands in ascending order, the
//                                  2 x 2 elimination, T_i and W_i^T g'_i into LDS; wave 0 adds the cameras in ascending order,
//                                  LDL^T, every camera's x_i, gamma_i, beta_i; writes the states and clears the histograms
//   photometric_rig_merge_kernel   every live camera's histogram <- the integer sum over the live cameras
constexpr int kPhotoRigChunk = 16;   // bands per chunk and wave: 16 x 48 doubles = 12 per lane
constexpr int kPhotoRigDepth = 2;    // chunks a wave holds in flight
constexpr int kPhotoRigCam = 120;    // LDS doubles per camera: S (48), T / W^T g' / c (28), W (36), l, 1 / d0, 1 / d1, (int32 adds, good)

// same wave: the LDS writes above are visible below, and the reads above are done before the writes below
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// lane q < 21 of the upper triangle, row-major -> (i, j)
__device__ __forceinline__ void triu_index(int q, int& i, int& j) {
    i = 0;
    while (q >= 6 - i) { q -= 6 - i; ++i; }
    j = i + q;
}

__global__ __launch_bounds__(256) void photometric_rig_solve_kernel(PhotometricRigArgs ga, int h, int w, int bands, int no_depth,
                                                                    int pass) {
    __shared__ double Gs[40 + 8 * 27];
    __shared__ double chunks[4][kPhotoRigChunk * kPhotoRPart];
    __shared__ double cams[kPhotoRigMaxCams * kPhotoRigCam];
    __shared__ double scratch[4][80];                   // per wave: H' (36, full), g' (6), M = H' W (36)
    const PhotometricRobustArgs& ra = ga.r;
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, lane = tid & 63, n_cams = a.n_pairs;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                   // uniform: the loops over a wave's cameras and bands branch as one
    {
        u32x4* hz = reinterpret_cast<u32x4*>(ra.hist);  // the cameras' histograms are one block
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (int i = tid; i < n_cams * (kPhotoBins / 4); i += 256) hz[i] = zero;
    }
    int32_t* rig_failed = reinterpret_cast<int32_t*>(ra.state + 11);             // camera 0's block: the call's failed flag
    if (pass > 0 && rig_failed[0]) return;
    for (int i = tid; i < 40 + 8 * 27; i += 256) Gs[i] = 0.0;
    double* chunk = chunks[wave];
    double* Hs = scratch[wave];
    double* gs = Hs + 36;
    double* Ms = Hs + 42;
    for (int cam = wave; cam < n_cams; cam += 4) {
        double* Sc = cams + cam * kPhotoRigCam;
        double* TW = Sc + 48;
        double* Wc = Sc + 76;
        const bool alive = !ga.live || ga.live[cam] != 0;
        if (lane < 36) Wc[lane] = ga.cVr[(size_t)cam * 36 + lane];
        const double* part = a.ws + (size_t)cam * bands * kPhotoRPart;
        double sum = 0.0;                               // lanes 0 .. 44: one of the camera's 45 sums each
        int count = 0;                                  // lane 45: the rows; 46: the holes; 47: the rows of weight 0
        const int total = (no_depth || !alive) ? 0 : bands * kPhotoRPart;
        // kPhotoRigDepth chunks in flight in registers: one wave fetches for itself, and a chunk's round trip is longer than its adds
        constexpr int kStep = kPhotoRigChunk * kPhotoRPart;
        double held[kPhotoRigDepth][12];
#pragma unroll
        for (int d = 0; d < kPhotoRigDepth; ++d)
#pragma unroll
            for (int u = 0; u < 12; ++u) { const int i = d * kStep + lane + 64 * u; held[d][u] = i < total ? part[i] : 0.0; }
        for (int c0 = 0; c0 < total; c0 += kPhotoRigDepth * kStep) {
#pragma unroll
            for (int d = 0; d < kPhotoRigDepth; ++d) {
                const int at = c0 + d * kStep;
                if (at >= total) break;
                wave_lds_fence();
#pragma unroll
                for (int u = 0; u < 12; ++u) chunk[lane + 64 * u] = held[d][u];
                wave_lds_fence();
                const int next = at + kPhotoRigDepth * kStep;
#pragma unroll
                for (int u = 0; u < 12; ++u) { const int i = next + lane + 64 * u; held[d][u] = i < total ? part[i] : 0.0; }
                const int nb = min(kPhotoRigChunk, bands - at / kPhotoRPart);
                if (lane < 45) {
#pragma unroll 8
                    for (int b = 0; b < nb; ++b) sum += chunk[b * kPhotoRPart + lane];     // ascending band order
                } else if (lane < 48) {
                    const int32_t* c = reinterpret_cast<const int32_t*>(chunk + 45) + (lane - 45);
#pragma unroll 8
                    for (int b = 0; b < nb; ++b) count += c[b * kPhotoRPart * 2];
                }
            }
        }
        if (ra.normal45 && lane < 45) ra.normal45[(size_t)cam * 45 + lane] = sum;
        if (lane < 45) Sc[lane] = sum;
        else if (lane < 48) reinterpret_cast<int32_t*>(Sc + 45)[lane - 45] = count;
        wave_lds_fence();
        const int n = reinterpret_cast<const int32_t*>(Sc + 45)[0];
        const bool adds = alive && n > 0;               // a live camera without a row adds nothing and fails nothing
        // C_i = l d l^T as photometric_robust_solve_kernel's
        bool cgood = true;
        double l = 0.0, i0 = 0.0, i1 = 0.0;
        if (ra.illumination) {
            const double DD = Sc[40], Dm = Sc[41], Sw = Sc[42];
            const double d0 = DD;
            cgood = (d0 > kPivotThreshold * DD) && (DD > 0.0);
            i0 = 1.0 / d0;
            l = Dm * i0;
            const double d1 = Sw - l * l * d0;
            cgood = cgood && (d1 > kPivotThreshold * Sw) && (Sw > 0.0);
            i1 = 1.0 / d1;
        }
        if (lane < 27) {
            double val = sum;
            int i, j = 0;
            if (lane < 21) triu_index(lane, i, j);
            else i = lane - 21;
            if (ra.illumination) {
                const double p = Sc[28 + 2 * i], q1 = Sc[29 + 2 * i];
                const double u1 = (q1 - l * p) * i1, u0 = p * i0 - l * u1;
                const double o0 = lane < 21 ? Sc[28 + 2 * j] : Sc[43], o1 = lane < 21 ? Sc[29 + 2 * j] : Sc[44];
                val = sum - (u0 * o0 + u1 * o1);
            }
            if (lane < 21) { Hs[i * 6 + j] = val; Hs[j * 6 + i] = val; }
            else gs[i] = val;
        }
        wave_lds_fence();
        if (lane < 36) {                                // M = H' W
            const int r = lane / 6, k = lane - r * 6;
            double t = Hs[r * 6] * Wc[k];
#pragma unroll
            for (int b = 1; b < 6; ++b) t += Hs[r * 6 + b] * Wc[b * 6 + k];
            Ms[lane] = t;
        }
        wave_lds_fence();
        if (lane < 28) {                                // T_i = W^T M (upper triangle), W^T g', c
            double t;
            if (lane < 21) {
                int j, k;
                triu_index(lane, j, k);
                t = Wc[j] * Ms[k];
#pragma unroll
                for (int r = 1; r < 6; ++r) t += Wc[r * 6 + j] * Ms[r * 6 + k];
            } else if (lane < 27) {
                const int k = lane - 21;
                t = Wc[k] * gs[0];
#pragma unroll
                for (int r = 1; r < 6; ++r) t += Wc[r * 6 + k] * gs[r];
            } else {
                t = Sc[27];
            }
            TW[lane] = t;
        }
        if (lane == 0) {
            Sc[112] = l; Sc[113] = i0; Sc[114] = i1;
            int32_t* f = reinterpret_cast<int32_t*>(Sc + 115);
            f[0] = adds ? 1 : 0; f[1] = cgood ? 1 : 0;
        }
        wave_lds_fence();
    }
    __syncthreads();
    if (wave != 0) return;
    // the cameras in ascending order: which wave held which does not show
    double sum = 0.0;
    int n = 0, holes = 0, zeros = 0, n_live = 0;
    bool cgood = true;
    for (int cam = 0; cam < n_cams; ++cam) {
        const double* Sc = cams + cam * kPhotoRigCam;
        const int32_t* f = reinterpret_cast<const int32_t*>(Sc + 115);
        const int32_t* c = reinterpret_cast<const int32_t*>(Sc + 45);
        if (!ga.live || ga.live[cam] != 0) { ++n_live; holes += c[1]; }
        if (!f[0]) continue;
        if (lane < 28) sum += Sc[48 + lane];
        n += c[0];
        zeros += c[2];
        cgood = cgood && f[1] != 0;
    }
    if (ga.rig_normal && lane < 28) ga.rig_normal[lane] = sum;
    if (lane < 27) {
        const bool diag = lane == 0 || lane == 6 || lane == 11 || lane == 15 || lane == 18 || lane == 20;
        Gs[40 + lane] = diag ? sum + a.mu * sum : sum;
    }
    wave_lds_fence();
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool solved = false;
    const bool tried = !no_depth && n >= 6 && n - zeros >= 6;
    if (tried && cgood) solved = solve_ldlt(Gs, lane, x);
    if (lane < n_cams) {                                // lane = camera: its step, lighting and state
        const int cam = lane;
        const double* Sc = cams + cam * kPhotoRigCam;
        const double* Wc = Sc + 76;
        const bool alive = !ga.live || ga.live[cam] != 0;
        const bool adds = reinterpret_cast<const int32_t*>(Sc + 115)[0] != 0;
        double xi[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double t = Wc[r * 6] * -x[0];
#pragma unroll
            for (int k = 1; k < 6; ++k) t += Wc[r * 6 + k] * -x[k];
            xi[r] = solved ? t : 0.0;
        }
        double gamma = 0.0, beta = 0.0;
        if (solved && adds && ra.illumination) {
            const double l = Sc[112], i0 = Sc[113], i1 = Sc[114];
            double t0 = Sc[43], t1 = Sc[44];
#pragma unroll
            for (int i = 0; i < 6; ++i) { t0 = t0 + Sc[28 + 2 * i] * xi[i]; t1 = t1 + Sc[29 + 2 * i] * xi[i]; }
            beta = (t1 - l * t0) * i1;
            gamma = t0 * i0 - l * beta;
        }
        double* state = ra.state + (size_t)cam * kPhotoState;
        int32_t* si = reinterpret_cast<int32_t*>(state + 9);
#pragma unroll
        for (int i = 0; i < 6; ++i) state[i] = xi[i];
        state[6] = gamma;
        state[7] = beta;
        si[0] = n;                                      // the stack's rows: the rows launch takes the median at (n + 1) / 2
        si[1] = (solved && alive) ? 0 : 1;              // a dead camera: the residual and weighted rows launches pass it by
        double* pr = ra.p_robust + (size_t)cam * 4;
        pr[0] = gamma;
        pr[1] = beta;
        pr[2] = (solved && adds && pass > 0) ? state[8] : 0.0;
        pr[3] = (solved && adds) ? Sc[42] : 0.0;
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.v_p[i] = solved ? -a.lambda * x[i] : 0.0;
        rig_failed[0] = solved ? 0 : 1;
        a.p_status[0] = no_depth ? ST_NO_DEPTH : solved ? ST_OK : ST_TOO_FEW;
        if (a.p_info) {
            int32_t* pi = a.p_info;
            pi[0] = n_live; pi[1] = n; pi[2] = zeros; pi[3] = pass; pi[4] = holes; pi[5] = (tried && !solved) ? 1 : 0; pi[6] = h; pi[7] = w;
        }
    }
}

__global__ __launch_bounds__(256) void photometric_rig_merge_kernel(PhotometricRigArgs ga) {
    const PhotometricRobustArgs& ra = ga.r;
    if (reinterpret_cast<const int32_t*>(ra.state + 11)[0]) return;
    const int bin = blockIdx.x * 256 + threadIdx.x, n_cams = ra.p.n_pairs;
    unsigned total = 0u;
    for (int cam = 0; cam < n_cams; ++cam)
        if (!ga.live || ga.live[cam] != 0) total += ra.hist[(size_t)cam * kPhotoBins + bin];
    for (int cam = 0; cam < n_cams; ++cam)
        if (!ga.live || ga.live[cam] != 0) ra.hist[(size_t)cam * kPhotoBins + bin] = total;
}

int launch_photometric_rig(const PhotometricRigArgs& ga_in, unsigned char* ws, int max_pairs, hipStream_t stream) {
    PhotometricRigArgs ga = ga_in;
    PhotometricRobustArgs& ra = ga.r;
    PhotometricArgs& a = ra.p;
    if (a.n_pairs < 1 || a.n_pairs > kPhotoRigMaxCams || a.n_pairs > max_pairs || !a.I_cur || !a.I_des || !a.K || !ws || !a.v_p ||
        !a.p_status || !ra.p_robust || !ga.cVr)
        return -2;
    if (a.interaction < 0 || a.interaction > 1 || !(a.mu >= 0.0) || !(a.mu < __builtin_huge_val())) return -2;
    if (!(a.lambda == a.lambda) || !(a.depth_scale == a.depth_scale)) return -2;
    if (ra.illumination < 0 || ra.illumination > 1 || ra.iterations < 0 || ra.iterations > 4) return -2;
    if (!(ra.sigma_min > 0.0) || !(ra.sigma_min < __builtin_huge_val())) return -2;
    PhotometricPlan p;
    if (int rc = plan_photometric(a.height, a.width, a.level, a.n_pairs, &p)) return rc;
    // the robust law's block, laid out as launch_photometric_robust lays it out
    a.ws = reinterpret_cast<double*>(ws);
    ra.hist = reinterpret_cast<uint32_t*>(ws + (size_t)max_pairs * 4096 * kPhotoRPart * sizeof(double));
    ra.state = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(ra.hist) + (size_t)max_pairs * kPhotoBins * sizeof(uint32_t));
    const size_t lds = p.lds - 4 * kPhotoPart * sizeof(double) + 4 * kPhotoRPart * sizeof(double);
    const size_t lds_res = lds + kPhotoBins * sizeof(uint32_t);
    const int no_depth = (!a.Z_mm && !(a.depth_scale > 0.0)) ? 1 : 0;
    if (no_depth) {
        launch(photometric_rig_solve_kernel, dim3(1), dim3(256), 0, stream, ga, p.h, p.w, p.bands, 1, 0);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    static std::atomic<unsigned long long> raised0{0}, raised1{0}, raised2{0};
    if (lds > 64 * 1024 &&
        (raise_lds_limit(reinterpret_cast<const void*>(photometric_robust_rows_kernel<false>), 160 * 1024, raised0) ||
         raise_lds_limit(reinterpret_cast<const void*>(photometric_robust_rows_kernel<true>), 160 * 1024, raised1)))
        return -3;
    if (ra.iterations > 0 && lds_res > 64 * 1024 &&
        raise_lds_limit(reinterpret_cast<const void*>(photometric_residual_kernel), 160 * 1024, raised2))
        return -3;
    const dim3 grid(p.bands, a.n_pairs);
    for (int pass = 0; pass <= ra.iterations; ++pass) {
        if (pass > 0) {
            launch(photometric_residual_kernel, grid, dim3(256), lds_res, stream, ra, p.h, p.w, p.rows, p.bands);
            launch(photometric_rig_merge_kernel, dim3(kPhotoBins / 256), dim3(256), 0, stream, ga);
            launch(photometric_robust_rows_kernel<true>, grid, dim3(256), lds, stream, ra, p.h, p.w, p.rows, p.bands);
        } else {
            launch(photometric_robust_rows_kernel<false>, grid, dim3(256), lds, stream, ra, p.h, p.w, p.rows, p.bands);
        }
        if (hipGetLastError() != hipSuccess) return -1;
        launch(photometric_rig_solve_kernel, dim3(1), dim3(256), 0, stream, ga, p.h, p.w, p.bands, 0, pass);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

// ---- the tile photometric law -------------------------------------------------------------------------------------
// The robust law with a LOCAL lighting model: one (gamma_k, beta_k) per tile of a gy x gx grid over the pooled image, the tile of
// pooled pixel (r, c) being floor(r gy / h) gx + floor(c gx / w).  Per tile the 45 sums and the 2 x 2 elimination; the live tiles'
// Schur terms add into ONE 6 x 6 system in ascending tile order; one median over all rows.  A tile whose 2 x 2 factor fails is dead
// in that pass.  3 N + 2 launches as the robust law's, in a block of its own (kernels.h PhotometricTileArgs).  pool_band,
// photo_row, photo_camera and photo_median_bin are the robust law's; the band plan is the plain law's (plan_photometric_tiles).
//   photometric_tile_rows_kernel<WEIGHTED>   per (band, pair): the band's (slot, tile column) segments, wave v taking segments
//                                            v, v + 4, ..; the lanes stride over a segment's pixels row-major, one wave_sum per
//                                            sum, one 48-double partial per segment and no step across waves
//   photometric_tile_residual_kernel         the robust law's, (gamma, beta) looked up by the pixel's tile
//   photometric_tile_solve_kernel            one workgroup of 16 waves per pair: wave v takes tiles v, v + 16, .. (the bands of the tile's rows
//                                            in ascending order, the 2 x 2 factor, the Schur terms into LDS); wave 0 adds the
//                                            live tiles in ascending order, LDL^T, every tile's (gamma_k, beta_k)
constexpr int kPhotoTileState = 16 + 2 * kPhotoTileMax;     // doubles per pair: the robust law's 16 (its gamma, beta slots unused), T x (gamma, beta)
constexpr int kPhotoTileSegs = 4096;                        // the most bands x slots a plan has
constexpr int kPhotoTileTerm = 32;                          // LDS doubles per tile: H'_k (21), g'_k (6), -, l, 1 / d0, 1 / d1, (int32 live)

// the first index of tile t of g over n indices: ceil(t n / g); tile t is [tile_begin(t), tile_begin(t + 1))
__host__ __device__ inline int tile_begin(int t, int n, int g) { return (t * n + g - 1) / g; }

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void photometric_tile_rows_kernel(PhotometricTileArgs ta, int h, int w, int rows, int bands,
                                                                    int slots) {
    extern __shared__ double photo_lds[];
    const PhotometricRobustArgs& ra = ta.r;
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                   // uniform: a wave's segments branch as one
    const int band = blockIdx.x, pair = blockIdx.y;
    const int gy = ta.tiles_y, gx = ta.tiles_x;
    const int r0 = band * rows, r1 = min(r0 + rows, h);
    double* red = photo_lds;                            // [4][48]: before the sums, the scan of the histogram (257 int32); then each wave's own 48
    int* lum_cur = reinterpret_cast<int*>(photo_lds + 4 * kPhotoRPart);
    int* lum_des = lum_cur + (rows + 2) * w;
    int* zs = lum_des + (rows + 2) * w;
    double* state = ra.state + (size_t)pair * kPhotoTileState;
    double st[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double scale = 1.0;                                 // kTukeyC * sigma
    if constexpr (WEIGHTED) {
        const int32_t* si = reinterpret_cast<const int32_t*>(state + 9);
        if (si[1]) return;                              // a solve before this one failed: the call's answer is written
#pragma unroll
        for (int i = 0; i < 6; ++i) st[i] = state[i];
        const int bin = photo_median_bin(ra.hist + (size_t)pair * kPhotoBins, (si[0] + 1) / 2, reinterpret_cast<int*>(red), tid);
        const double median = ((double)bin + 0.5) / 16.0;
        const double sigma = fmax(kMadScale * median, ra.sigma_min);
        scale = kTukeyC * sigma;
        if (band == 0 && tid == 0) { state[8] = sigma; reinterpret_cast<int32_t*>(state + 10)[0] = bin; }
    }
    pool_band(a, pair, h, w, rows, r0, r1, lum_cur, lum_des, zs, tid);
    const PhotoCamera cam = photo_camera(a.K + (size_t)pair * 4, a.level);
    const int* grad = a.interaction ? lum_des : lum_cur;
    const bool have_z = a.Z_mm != nullptr;
    const int ty0 = r0 * gy / h;                        // slot s of the band is tile row ty0 + s
    for (int seg = wave; seg < slots * gx; seg += 4) {
        const int slot = seg / gx, tx = seg - slot * gx, ty = ty0 + slot;
        if (ty >= gy) continue;
        const int ra0 = max(r0, tile_begin(ty, h, gy)), ra1 = min(r1, tile_begin(ty + 1, h, gy));
        if (ra1 <= ra0) continue;                       // the band does not cross into that tile row: the slot is not read either
        const int c0 = tile_begin(tx, w, gx), sw = tile_begin(tx + 1, w, gx) - c0;
        if constexpr (WEIGHTED) {
            const int k = ty * gx + tx;
            st[6] = state[16 + 2 * k];
            st[7] = state[17 + 2 * k];
        }
        double acc[45];
#pragma unroll
        for (int q = 0; q < 45; ++q) acc[q] = 0.0;
        int n = 0, holes = 0, zeros = 0;
        for (int idx = lane; idx < (ra1 - ra0) * sw; idx += 64) {
            const int q0 = idx / sw, c = c0 + (idx - q0 * sw), r = ra0 + q0, lr = r - r0;
            double L[6], e, D;
            const int kind = photo_row(cam, grad, lum_cur, lum_des, zs, have_z, a.depth_scale, h, w, lr, c, r, L, e, D);
            if (kind == 2) ++holes;
            if (kind != 0) continue;
            double wt = 1.0;
            if constexpr (WEIGHTED) {
                const double t = photo_rho(L, e, D, st) / scale;
                const double u = 1.0 - t * t;
                wt = t < 1.0 ? u * u : 0.0;
                if (wt == 0.0) ++zeros;
            }
            double wv[8];
#pragma unroll
            for (int i = 0; i < 6; ++i) wv[i] = wt * L[i];
            wv[6] = wt * e;
            wv[7] = wt * D;
            int q = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) { acc[q] += wv[i] * L[j]; ++q; }
#pragma unroll
            for (int i = 0; i < 7; ++i) acc[21 + i] += wv[i] * e;
#pragma unroll
            for (int i = 0; i < 6; ++i) { acc[28 + 2 * i] += wv[i] * D; acc[29 + 2 * i] += wv[i]; }
            acc[40] += wv[7] * D;
            acc[41] += wv[7];
            acc[42] += wt;
            acc[43] += wv[7] * e;
            acc[44] += wv[6];
            ++n;
        }
        double* mine_red = red + wave * kPhotoRPart;    // the wave's own 48 doubles: no step across waves
#pragma unroll
        for (int q = 0; q < 45; ++q) {
            const double t = wave_sum(acc[q]);
            if (lane == 0) mine_red[q] = t;
        }
        wave_lds_fence();
        double mine = lane < 45 ? mine_red[lane] : 0.0; // lane q < 45: sum q; lane 45: (rows, holes); lane 46: (zero weights, 0)
        wave_lds_fence();
        n = wave_sum(n);
        holes = wave_sum(holes);
        zeros = wave_sum(zeros);
        if (lane == 45) mine = __builtin_bit_cast(double, ((unsigned long long)(unsigned)holes << 32) | (unsigned)n);
        if (lane == 46) mine = __builtin_bit_cast(double, (unsigned long long)(unsigned)zeros);
        double* part = a.ws + ((((size_t)pair * bands + band) * slots + slot) * gx + tx) * kPhotoRPart;
        if (lane < kPhotoRPart) part[lane] = mine;
    }
}

__global__ __launch_bounds__(256) void photometric_tile_residual_kernel(PhotometricTileArgs ta, int h, int w, int rows, int bands) {
    extern __shared__ double photo_lds[];
    const PhotometricRobustArgs& ra = ta.r;
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, band = blockIdx.x, pair = blockIdx.y;
    const int gy = ta.tiles_y, gx = ta.tiles_x;
    const int r0 = band * rows, r1 = min(r0 + rows, h);
    int* lum_cur = reinterpret_cast<int*>(photo_lds + 4 * kPhotoRPart);          // the rows launch's layout, the histogram behind it
    int* lum_des = lum_cur + (rows + 2) * w;
    int* zs = lum_des + (rows + 2) * w;
    unsigned* bins = reinterpret_cast<unsigned*>(zs + rows * w);
    const double* state = ra.state + (size_t)pair * kPhotoTileState;
    if (reinterpret_cast<const int32_t*>(state + 9)[1]) return;
    double st[8];
#pragma unroll
    for (int i = 0; i < 6; ++i) st[i] = state[i];
    for (int i = tid; i < kPhotoBins; i += 256) bins[i] = 0u;
    pool_band(a, pair, h, w, rows, r0, r1, lum_cur, lum_des, zs, tid);          // (its barriers order the zeros above too)
    const PhotoCamera cam = photo_camera(a.K + (size_t)pair * 4, a.level);
    const int* grad = a.interaction ? lum_des : lum_cur;
    const bool have_z = a.Z_mm != nullptr;
    for (int idx = tid; idx < (r1 - r0) * w; idx += 256) {
        const int lr = idx / w, c = idx - lr * w, r = r0 + lr;
        double L[6], e, D;
        if (photo_row(cam, grad, lum_cur, lum_des, zs, have_z, a.depth_scale, h, w, lr, c, r, L, e, D) != 0) continue;
        const int k = (r * gy / h) * gx + c * gx / w;   // the pixel's tile: its own lighting pair
        st[6] = state[16 + 2 * k];
        st[7] = state[17 + 2 * k];
        const double rho = photo_rho(L, e, D, st);
        const int q = rho < (double)(kPhotoBins / 16) ? (int)(16.0 * rho) : kPhotoBins - 1;      // (a NaN: the last bin)
        atomicAdd(&bins[q], 1u);
    }
    __syncthreads();
    unsigned* hist = ra.hist + (size_t)pair * kPhotoBins;
    for (int i = tid; i < kPhotoBins; i += 256) {
        const unsigned cnt = bins[i];
        if (cnt) atomicAdd(&hist[i], cnt);
    }
}

constexpr int kPhotoTileDepth = 8;   // band partials a wave holds in flight per tile (16 measured slower)
constexpr int kPhotoTileSolveThreads = 1024;     // 16 waves: 4 x 4 tiles are one tile per wave, 8 x 8 four

__global__ __launch_bounds__(kPhotoTileSolveThreads) void photometric_tile_solve_kernel(PhotometricTileArgs ta, int h, int w, int rows, int bands,
                                                                     int slots, int no_depth, int pass) {
    __shared__ double Gs[40 + 8 * 27];
    __shared__ double St[kPhotoTileMax * kPhotoRPart];  // every tile's 45 sums and counts: 24 KiB
    __shared__ double Tm[kPhotoTileMax * kPhotoTileTerm];
    const PhotometricRobustArgs& ra = ta.r;
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gy = ta.tiles_y, gx = ta.tiles_x, T = gy * gx;
    unsigned* hist = ra.hist + (size_t)pair * kPhotoBins;                         // as photometric_robust_solve_kernel clears it
    for (int i = tid; i < kPhotoBins; i += kPhotoTileSolveThreads) hist[i] = 0u;
    double* state = ra.state + (size_t)pair * kPhotoTileState;
    int32_t* si = reinterpret_cast<int32_t*>(state + 9);
    if (pass > 0 && si[1]) return;
    for (int i = tid; i < 40 + 8 * 27; i += kPhotoTileSolveThreads) Gs[i] = 0.0;
    const double* pair_ws = a.ws + (size_t)pair * bands * slots * gx * kPhotoRPart;
    for (int k = wave; k < T; k += kPhotoTileSolveThreads / 64) {
        const int ty = k / gx, tx = k - ty * gx;
        const int tr0 = tile_begin(ty, h, gy), tr1 = tile_begin(ty + 1, h, gy);
        const int b0 = tr0 / rows, b1 = no_depth ? b0 : (tr1 - 1) / rows + 1;      // the bands that hold rows of the tile
        double sum = 0.0;                               // lanes 0 .. 44: one of the tile's 45 sums each
        int cnt0 = 0, cnt1 = 0;                         // lane 45: rows, holes; lane 46: rows of weight 0
        for (int b = b0; b < b1; b += kPhotoTileDepth) {
            double held[kPhotoTileDepth];
#pragma unroll
            for (int u = 0; u < kPhotoTileDepth; ++u) {
                const int bb = min(b + u, b1 - 1);
                const int slot = (slots > 1 && bb * rows < tr0) ? 1 : 0;      // the band began in the tile row before: its second slot
                held[u] = (b + u < b1 && lane < kPhotoRPart) ? pair_ws[((size_t)(bb * slots + slot) * gx + tx) * kPhotoRPart + lane] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kPhotoTileDepth; ++u) {
                if (b + u >= b1) break;
                if (lane < 45) {
                    sum += held[u];                     // ascending band order
                } else {
                    const unsigned long long bits = __builtin_bit_cast(unsigned long long, held[u]);
                    cnt0 += (int)(unsigned)bits;
                    cnt1 += (int)(unsigned)(bits >> 32);
                }
            }
        }
        if (ra.normal45 && lane < 45) ra.normal45[((size_t)pair * T + k) * 45 + lane] = sum;
        double* Sk = St + k * kPhotoRPart;
        double* Tk = Tm + k * kPhotoTileTerm;
        if (lane < 45) Sk[lane] = sum;
        else if (lane == 45) { int32_t* c = reinterpret_cast<int32_t*>(Sk + 45); c[0] = cnt0; c[1] = cnt1; }
        else if (lane == 46) { int32_t* c = reinterpret_cast<int32_t*>(Sk + 46); c[0] = cnt0; c[1] = 0; }
        wave_lds_fence();
        // C_k = l d l^T as photometric_robust_solve_kernel's
        const double DD = Sk[40], Dm = Sk[41], Sw = Sk[42];
        const double d0 = DD;
        bool cgood = (d0 > kPivotThreshold * DD) && (DD > 0.0);
        const double i0 = 1.0 / d0;
        const double l = Dm * i0;
        const double d1 = Sw - l * l * d0;
        cgood = cgood && (d1 > kPivotThreshold * Sw) && (Sw > 0.0);
        const double i1 = 1.0 / d1;
        if (lane < 27) {
            int i, j = 0;
            if (lane < 21) triu_index(lane, i, j);
            else i = lane - 21;
            const double p = Sk[28 + 2 * i], q1 = Sk[29 + 2 * i];
            const double u1 = (q1 - l * p) * i1, u0 = p * i0 - l * u1;
            const double o0 = lane < 21 ? Sk[28 + 2 * j] : Sk[43], o1 = lane < 21 ? Sk[29 + 2 * j] : Sk[44];
            Tk[lane] = sum - (u0 * o0 + u1 * o1);
        }
        if (lane == 0) {
            Tk[28] = l; Tk[29] = i0; Tk[30] = i1;
            reinterpret_cast<int32_t*>(Tk + 31)[0] = cgood ? 1 : 0;
        }
        wave_lds_fence();
    }
    __syncthreads();
    if (wave != 0) return;
    // the live tiles in ascending order: which wave held which does not show.  Lane k holds tile k's counts and flag; the sums
    // run over all T tiles with the reads in flight together, a dead tile adding +0.0 (exact: a sum that starts at +0.0 is never -0.0)
    int n = 0, holes = 0, zeros = 0;
    bool mine_live = false;
    if (lane < T) {
        const int32_t* c = reinterpret_cast<const int32_t*>(St + lane * kPhotoRPart + 45);
        n = c[0];
        holes = c[1];
        zeros = c[2];
        mine_live = reinterpret_cast<const int32_t*>(Tm + lane * kPhotoTileTerm + 31)[0] != 0;
    }
    n = wave_sum(n);
    holes = wave_sum(holes);
    zeros = wave_sum(zeros);
    const unsigned long long live_mask = __ballot(mine_live);
    const int n_live = __popcll(live_mask);
    double sum = 0.0, wtotal = 0.0;
    const int term = lane < 27 ? lane : 0;
#pragma unroll 8
    for (int k = 0; k < T; ++k) {
        const double t = Tm[k * kPhotoTileTerm + term], wk = St[k * kPhotoRPart + 42];
        const bool live = (live_mask >> k) & 1ull;
        sum += live ? t : 0.0;
        wtotal += live ? wk : 0.0;
    }
    if (lane < 27) {
        const bool diag = lane == 0 || lane == 6 || lane == 11 || lane == 15 || lane == 18 || lane == 20;
        Gs[40 + lane] = diag ? sum + a.mu * sum : sum;
    }
    wave_lds_fence();
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool solved = false;
    const bool tried = !no_depth && n >= 6 && n - zeros >= 6;
    if (tried && n_live > 0) solved = solve_ldlt(Gs, lane, x);
    if (lane < T) {                                     // lane = tile: its lighting pair
        const int k = lane;
        const double* Sk = St + k * kPhotoRPart;
        const double* Tk = Tm + k * kPhotoTileTerm;
        const bool live = reinterpret_cast<const int32_t*>(Tk + 31)[0] != 0;
        double gamma = 0.0, beta = 0.0;
        if (solved && live) {
            const double l = Tk[28], i0 = Tk[29], i1 = Tk[30];
            double t0 = Sk[43], t1 = Sk[44];
#pragma unroll
            for (int i = 0; i < 6; ++i) { t0 = t0 + Sk[28 + 2 * i] * -x[i]; t1 = t1 + Sk[29 + 2 * i] * -x[i]; }
            beta = (t1 - l * t0) * i1;
            gamma = t0 * i0 - l * beta;
        }
        state[16 + 2 * k] = gamma;
        state[17 + 2 * k] = beta;
        double* pt = ta.p_tiles + ((size_t)pair * T + k) * 4;
        pt[0] = gamma;
        pt[1] = beta;
        pt[2] = solved ? Sk[42] : 0.0;
        pt[3] = (solved && live) ? 1.0 : 0.0;
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            state[i] = -x[i];
            a.v_p[(size_t)pair * 6 + i] = solved ? -a.lambda * x[i] : 0.0;
        }
        state[6] = 0.0;
        state[7] = 0.0;
        si[0] = n;
        si[1] = solved ? 0 : 1;
        a.p_status[pair] = no_depth ? ST_NO_DEPTH : solved ? ST_OK : ST_TOO_FEW;
        if (a.p_info) {
            int32_t* pi = a.p_info + (size_t)pair * 8;
            pi[0] = n; pi[1] = h; pi[2] = w; pi[3] = bands; pi[4] = holes; pi[5] = (tried && !solved) ? 1 : 0; pi[6] = zeros; pi[7] = pass;
        }
        double* pr = ra.p_robust + (size_t)pair * 4;
        pr[0] = solved ? (double)n_live : 0.0;
        pr[1] = solved ? (double)(T - n_live) : 0.0;
        pr[2] = (solved && pass > 0) ? state[8] : 0.0;
        pr[3] = solved ? wtotal : 0.0;
    }
}

int plan_photometric_tiles(int height, int width, int level, int tiles_y, int tiles_x, int max_pairs, PhotometricTilePlan* plan) {
    if (!plan || tiles_y < 1 || tiles_y > 8 || tiles_x < 1 || tiles_x > 8) return -2;
    PhotometricPlan p;
    if (int rc = plan_photometric(height, width, level, max_pairs, &p)) return rc;
    if (tiles_y > p.h || tiles_x > p.w) return -2;
    plan->h = p.h;
    plan->w = p.w;
    plan->rows = p.rows;
    plan->bands = p.bands;
    // A band of more than one row (h >= 512) may lie across ONE tile-row boundary: rows <= h / 256 and a tile row has at least
    // floor(h / 8) >= 64 rows.  Such a plan gives every band a second slot; one-row bands have one.  rows > 1 means bands <= h / 2
    // + 1, so bands x slots stays within kPhotoTileSegs either way.
    plan->slots = p.rows > 1 ? 2 : 1;
    plan->lds = p.lds - 4 * kPhotoPart * sizeof(double) + 4 * kPhotoRPart * sizeof(double);
    plan->lds_res = plan->lds + kPhotoBins * sizeof(uint32_t);
    plan->ws_doubles = (size_t)plan->bands * plan->slots * tiles_x * kPhotoRPart;
    return plan->bands * plan->slots <= kPhotoTileSegs ? 0 : -3;
}

size_t photometric_tile_ws_bytes(int max_pairs) {
    return (size_t)max_pairs * ((size_t)kPhotoTileSegs * 8 * kPhotoRPart * sizeof(double) + kPhotoBins * sizeof(uint32_t) +
                                kPhotoTileState * sizeof(double));
}

int launch_photometric_tiles(const PhotometricTileArgs& ta_in, unsigned char* ws, int max_pairs, hipStream_t stream) {
    PhotometricTileArgs ta = ta_in;
    PhotometricRobustArgs& ra = ta.r;
    PhotometricArgs& a = ra.p;
    if (a.n_pairs < 1 || a.n_pairs > 65535 || a.n_pairs > max_pairs || !a.I_cur || !a.I_des || !a.K || !ws || !a.v_p || !a.p_status ||
        !ra.p_robust || !ta.p_tiles)
        return -2;
    if (a.interaction < 0 || a.interaction > 1 || !(a.mu >= 0.0) || !(a.mu < __builtin_huge_val())) return -2;
    if (!(a.lambda == a.lambda) || !(a.depth_scale == a.depth_scale)) return -2;
    if (ra.iterations < 0 || ra.iterations > 4) return -2;
    if (!(ra.sigma_min > 0.0) || !(ra.sigma_min < __builtin_huge_val())) return -2;
    PhotometricTilePlan p;
    if (int rc = plan_photometric_tiles(a.height, a.width, a.level, ta.tiles_y, ta.tiles_x, a.n_pairs, &p)) return rc;
    ra.illumination = 1;
    // the block: the partials of max_pairs pairs at kPhotoTileSegs segments rows of 8 tile columns, then the histograms, then the states
    const size_t part_bytes = (size_t)max_pairs * kPhotoTileSegs * 8 * kPhotoRPart * sizeof(double);
    a.ws = reinterpret_cast<double*>(ws);
    ra.hist = reinterpret_cast<uint32_t*>(ws + part_bytes);
    ra.state = reinterpret_cast<double*>(ws + part_bytes + (size_t)max_pairs * kPhotoBins * sizeof(uint32_t));
    const int no_depth = (!a.Z_mm && !(a.depth_scale > 0.0)) ? 1 : 0;
    if (no_depth) {
        launch(photometric_tile_solve_kernel, dim3(a.n_pairs), dim3(kPhotoTileSolveThreads), 0, stream, ta, p.h, p.w, p.rows, p.bands, p.slots, 1, 0);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    static std::atomic<unsigned long long> raised0{0}, raised1{0}, raised2{0};
    if (p.lds > 64 * 1024 &&
        (raise_lds_limit(reinterpret_cast<const void*>(photometric_tile_rows_kernel<false>), 160 * 1024, raised0) ||
         raise_lds_limit(reinterpret_cast<const void*>(photometric_tile_rows_kernel<true>), 160 * 1024, raised1)))
        return -3;
    if (ra.iterations > 0 && p.lds_res > 64 * 1024 &&
        raise_lds_limit(reinterpret_cast<const void*>(photometric_tile_residual_kernel), 160 * 1024, raised2))
        return -3;
    const dim3 grid(p.bands, a.n_pairs);
    for (int pass = 0; pass <= ra.iterations; ++pass) {
        if (pass > 0) {
            launch(photometric_tile_residual_kernel, grid, dim3(256), p.lds_res, stream, ta, p.h, p.w, p.rows, p.bands);
            launch(photometric_tile_rows_kernel<true>, grid, dim3(256), p.lds, stream, ta, p.h, p.w, p.rows, p.bands, p.slots);
        } else {
            launch(photometric_tile_rows_kernel<false>, grid, dim3(256), p.lds, stream, ta, p.h, p.w, p.rows, p.bands, p.slots);
        }
        if (hipGetLastError() != hipSuccess) return -1;
        launch(photometric_tile_solve_kernel, dim3(a.n_pairs), dim3(kPhotoTileSolveThreads), 0, stream, ta, p.h, p.w, p.rows, p.bands, p.slots, 0, pass);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

// ---- the surface photometric law ----------------------------------------------------------------------------------
// The tile law's sibling for SMOOTH lighting fields: a bilinear spline of gains and biases on the (gy + 1)(gx + 1) nodes of the
// same grid, I_cur ~ (1 + sum phi_a gamma_a) I_des + sum phi_a beta_a over the four nodes of the pixel's cell.  Unknown 2 a = gamma_a,
// 2 a + 1 = beta_a, node a = i (gx + 1) + j, M = 2 (gy + 1)(gx + 1) <= 162.  Per cell 120 weighted sums (A 21, b 6, c, B 6 x 8, C 36,
// d 8) and sum w; the cells add in ascending order into the bordered system [[C_g, R^T], [R, S]] (R = B_g and d_g, S = A, b, c),
// which ONE right-looking banded LDL^T (half-bandwidth 2 gx + 5) eliminates under the pivot rule: what is left of S is H', g'.  An
// unknown whose pivot fails is DEAD in that pass (column skipped, value 0).  3 N + 2 launches in a block of its own (kernels.h
// PhotometricSurfaceArgs); the bands, slots and segments are the tile law's (plan_photometric_tiles).
//   photometric_surface_rows_kernel<WEIGHTED>   the tile rows kernel's mapping; a wave walks its segment of the LDS-resident band
//                                               TWICE (A, b, c, C, d, sum w: 73 accumulators; then B: 48), so that no pass holds
//                                               all 121 in registers; one 128-double partial per segment
//   photometric_surface_residual_kernel         the tile law's, the pixel's four node pairs interpolated
//   photometric_surface_solve_kernel            one workgroup of 8 waves per pair: wave v adds the bands of cells v, v + 8, ..; the
//                                               node system gathered into LDS (every entry over its <= 4 cells in ascending order);
//                                               per column 231 + 147 + 28 independent updates behind one barrier; wave 0 solves the
//                                               6 x 6 system and back-substitutes
// The workspace: 4096 segment rows x 8 cell columns x 128 doubles = 32 MiB per pair of max_pairs, a histogram and a state.
constexpr int kPhotoSurfPart = 128;       // doubles per partial: the 120 sums, sum w, (int32 rows, holes), (int32 zero weights, 0), 5 unused
constexpr int kPhotoSurfState = 16 + 176; // doubles per pair: the robust law's 16 (gamma, beta unused), then the M unknowns
constexpr int kPhotoSurfBand = 22;        // LDS doubles per column of C_g: the diagonal and the 21 entries below it
constexpr int kPhotoSurfSolveThreads = 512;
constexpr int kPhotoSurfDepth = 8;        // band partials a wave holds in flight per cell

// the bilinear weights of pooled pixel (r, c) in cell (ty, tx): exact integer numerators, one division each
__device__ __forceinline__ void surface_phi(int r, int c, int ty, int tx, int gy, int gx, int h, int w, double (&phi)[4]) {
    const double v = (double)(r * gy - ty * h) / (double)h, u = (double)(c * gx - tx * w) / (double)w;
    const double v1 = 1.0 - v, u1 = 1.0 - u;
    phi[0] = v1 * u1;
    phi[1] = v1 * u;
    phi[2] = v * u1;
    phi[3] = v * u;
}

// (gamma, beta) at a pixel: the phi-sums over the cell's four node pairs nd = (gamma, beta) x 4, in node order
__device__ __forceinline__ void surface_lighting(const double (&phi)[4], const double (&nd)[8], double& gamma, double& beta) {
    gamma = phi[0] * nd[0];
    beta = phi[0] * nd[1];
#pragma unroll
    for (int s = 1; s < 4; ++s) {
        gamma = gamma + phi[s] * nd[2 * s];
        beta = beta + phi[s] * nd[2 * s + 1];
    }
}

// the four node pairs of cell (ty, tx) from the pair's state block
__device__ __forceinline__ void surface_nodes(const double* state, int ty, int tx, int gx, double (&nd)[8]) {
    const int a0 = ty * (gx + 1) + tx;
    const int at[4] = {a0, a0 + 1, a0 + gx + 1, a0 + gx + 2};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        nd[2 * s] = state[16 + 2 * at[s]];
        nd[2 * s + 1] = state[17 + 2 * at[s]];
    }
}

// lane (pos mod 64) keeps the wave-uniform t in its half pos / 64 of the partial
__device__ __forceinline__ void surface_keep(double t, int pos, int lane, double& lo, double& hi) {
    if (lane == (pos & 63)) {
        if (pos < 64) lo = t;
        else hi = t;
    }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void photometric_surface_rows_kernel(PhotometricSurfaceArgs sa, int h, int w, int rows, int bands,
                                                                       int slots) {
    extern __shared__ double photo_lds[];
    const PhotometricRobustArgs& ra = sa.r;
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int band = blockIdx.x, pair = blockIdx.y;
    const int gy = sa.cells_y, gx = sa.cells_x;
    const int r0 = band * rows, r1 = min(r0 + rows, h);
    int* scan = reinterpret_cast<int*>(photo_lds);      // the tile law's layout: 4 x 48 doubles, here only the histogram's scan
    int* lum_cur = reinterpret_cast<int*>(photo_lds + 4 * kPhotoRPart);
    int* lum_des = lum_cur + (rows + 2) * w;
    int* zs = lum_des + (rows + 2) * w;
    double* state = ra.state + (size_t)pair * kPhotoSurfState;
    double st[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double scale = 1.0;                                 // kTukeyC * sigma
    if constexpr (WEIGHTED) {
        const int32_t* si = reinterpret_cast<const int32_t*>(state + 9);
        if (si[1]) return;                              // a solve before this one failed: the call's answer is written
#pragma unroll
        for (int i = 0; i < 6; ++i) st[i] = state[i];
        const int bin = photo_median_bin(ra.hist + (size_t)pair * kPhotoBins, (si[0] + 1) / 2, scan, tid);
        const double median = ((double)bin + 0.5) / 16.0;
        const double sigma = fmax(kMadScale * median, ra.sigma_min);
        scale = kTukeyC * sigma;
        if (band == 0 && tid == 0) { state[8] = sigma; reinterpret_cast<int32_t*>(state + 10)[0] = bin; }
    }
    pool_band(a, pair, h, w, rows, r0, r1, lum_cur, lum_des, zs, tid);
    const PhotoCamera cam = photo_camera(a.K + (size_t)pair * 4, a.level);
    const int* grad = a.interaction ? lum_des : lum_cur;
    const bool have_z = a.Z_mm != nullptr;
    const int ty0 = r0 * gy / h;                        // slot s of the band is cell row ty0 + s
    for (int seg = wave; seg < slots * gx; seg += 4) {
        const int slot = seg / gx, tx = seg - slot * gx, ty = ty0 + slot;
        if (ty >= gy) continue;
        const int ra0 = max(r0, tile_begin(ty, h, gy)), ra1 = min(r1, tile_begin(ty + 1, h, gy));
        if (ra1 <= ra0) continue;                       // the band does not cross into that cell row: the slot is not read either
        const int c0 = tile_begin(tx, w, gx), sw = tile_begin(tx + 1, w, gx) - c0;
        double nd[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if constexpr (WEIGHTED) surface_nodes(state, ty, tx, gx, nd);
        double lo = 0.0, hi = 0.0;                      // lane q: sums q and 64 + q of the partial
        // the first walk: A (21), b (6), c, then C (36), d (8), sum w
        {
            double acc[73];
#pragma unroll
            for (int q = 0; q < 73; ++q) acc[q] = 0.0;
            int n = 0, holes = 0, zeros = 0;
            for (int idx = lane; idx < (ra1 - ra0) * sw; idx += 64) {
                const int q0 = idx / sw, c = c0 + (idx - q0 * sw), r = ra0 + q0, lr = r - r0;
                double L[6], e, D;
                const int kind = photo_row(cam, grad, lum_cur, lum_des, zs, have_z, a.depth_scale, h, w, lr, c, r, L, e, D);
                if (kind == 2) ++holes;
                if (kind != 0) continue;
                double phi[4];
                surface_phi(r, c, ty, tx, gy, gx, h, w, phi);
                double wt = 1.0;
                if constexpr (WEIGHTED) {
                    surface_lighting(phi, nd, st[6], st[7]);
                    const double t = photo_rho(L, e, D, st) / scale;
                    const double u = 1.0 - t * t;
                    wt = t < 1.0 ? u * u : 0.0;
                    if (wt == 0.0) ++zeros;
                }
                double wv[7], m[8], wm[8];
#pragma unroll
                for (int i = 0; i < 6; ++i) wv[i] = wt * L[i];
                wv[6] = wt * e;
#pragma unroll
                for (int s = 0; s < 4; ++s) { m[2 * s] = D * phi[s]; m[2 * s + 1] = phi[s]; }
#pragma unroll
                for (int k = 0; k < 8; ++k) wm[k] = wt * m[k];
                int q = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = i; j < 6; ++j) { acc[q] += wv[i] * L[j]; ++q; }
#pragma unroll
                for (int i = 0; i < 7; ++i) acc[21 + i] += wv[i] * e;
                q = 28;
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int l = k; l < 8; ++l) { acc[q] += wm[k] * m[l]; ++q; }
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[64 + k] += wm[k] * e;
                acc[72] += wt;
                ++n;
            }
#pragma unroll
            for (int q = 0; q < 28; ++q) surface_keep(wave_sum(acc[q]), q, lane, lo, hi);
#pragma unroll
            for (int q = 28; q < 72; ++q) surface_keep(wave_sum(acc[q]), 48 + q, lane, lo, hi);      // C at 76, d at 112
            surface_keep(wave_sum(acc[72]), 120, lane, lo, hi);
            n = wave_sum(n);
            holes = wave_sum(holes);
            zeros = wave_sum(zeros);
            if (lane == 57) hi = __builtin_bit_cast(double, ((unsigned long long)(unsigned)holes << 32) | (unsigned)n);
            if (lane == 58) hi = __builtin_bit_cast(double, (unsigned long long)(unsigned)zeros);
        }
        // the second walk: B (6 x 8), the same rows and the same weights
        {
            double acc[48];
#pragma unroll
            for (int q = 0; q < 48; ++q) acc[q] = 0.0;
            for (int idx = lane; idx < (ra1 - ra0) * sw; idx += 64) {
                const int q0 = idx / sw, c = c0 + (idx - q0 * sw), r = ra0 + q0, lr = r - r0;
                double L[6], e, D;
                if (photo_row(cam, grad, lum_cur, lum_des, zs, have_z, a.depth_scale, h, w, lr, c, r, L, e, D) != 0) continue;
                double phi[4];
                surface_phi(r, c, ty, tx, gy, gx, h, w, phi);
                double wt = 1.0;
                if constexpr (WEIGHTED) {
                    surface_lighting(phi, nd, st[6], st[7]);
                    const double t = photo_rho(L, e, D, st) / scale;
                    const double u = 1.0 - t * t;
                    wt = t < 1.0 ? u * u : 0.0;
                }
                double m[8];
#pragma unroll
                for (int s = 0; s < 4; ++s) { m[2 * s] = D * phi[s]; m[2 * s + 1] = phi[s]; }
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double wvi = wt * L[i];
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[8 * i + k] += wvi * m[k];
                }
            }
#pragma unroll
            for (int q = 0; q < 48; ++q) surface_keep(wave_sum(acc[q]), 28 + q, lane, lo, hi);
        }
        double* part = a.ws + ((((size_t)pair * bands + band) * slots + slot) * gx + tx) * kPhotoSurfPart;
        part[lane] = lo;
        part[64 + lane] = hi;
    }
}

__global__ __launch_bounds__(256) void photometric_surface_residual_kernel(PhotometricSurfaceArgs sa, int h, int w, int rows, int bands) {
    extern __shared__ double photo_lds[];
    const PhotometricRobustArgs& ra = sa.r;
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, band = blockIdx.x, pair = blockIdx.y;
    const int gy = sa.cells_y, gx = sa.cells_x;
    const int r0 = band * rows, r1 = min(r0 + rows, h);
    int* lum_cur = reinterpret_cast<int*>(photo_lds + 4 * kPhotoRPart);          // the rows launch's layout, the histogram behind it
    int* lum_des = lum_cur + (rows + 2) * w;
    int* zs = lum_des + (rows + 2) * w;
    unsigned* bins = reinterpret_cast<unsigned*>(zs + rows * w);
    const double* state = ra.state + (size_t)pair * kPhotoSurfState;
    if (reinterpret_cast<const int32_t*>(state + 9)[1]) return;
    double st[8];
#pragma unroll
    for (int i = 0; i < 6; ++i) st[i] = state[i];
    for (int i = tid; i < kPhotoBins; i += 256) bins[i] = 0u;
    pool_band(a, pair, h, w, rows, r0, r1, lum_cur, lum_des, zs, tid);          // (its barriers order the zeros above too)
    const PhotoCamera cam = photo_camera(a.K + (size_t)pair * 4, a.level);
    const int* grad = a.interaction ? lum_des : lum_cur;
    const bool have_z = a.Z_mm != nullptr;
    for (int idx = tid; idx < (r1 - r0) * w; idx += 256) {
        const int lr = idx / w, c = idx - lr * w, r = r0 + lr;
        double L[6], e, D;
        if (photo_row(cam, grad, lum_cur, lum_des, zs, have_z, a.depth_scale, h, w, lr, c, r, L, e, D) != 0) continue;
        const int ty = r * gy / h, tx = c * gx / w;     // the pixel's cell: its four node pairs, interpolated
        double phi[4], nd[8];
        surface_phi(r, c, ty, tx, gy, gx, h, w, phi);
        surface_nodes(state, ty, tx, gx, nd);
        surface_lighting(phi, nd, st[6], st[7]);
        const double rho = photo_rho(L, e, D, st);
        const int q = rho < (double)(kPhotoBins / 16) ? (int)(16.0 * rho) : kPhotoBins - 1;      // (a NaN: the last bin)
        atomicAdd(&bins[q], 1u);
    }
    __syncthreads();
    unsigned* hist = ra.hist + (size_t)pair * kPhotoBins;
    for (int i = tid; i < kPhotoBins; i += 256) {
        const unsigned cnt = bins[i];
        if (cnt) atomicAdd(&hist[i], cnt);
    }
}

// the LDS doubles of the solve: the cells' partials, C_g's columns, R (7 rows), the original diagonal, 1 / d_j, t / q, S (32),
// solve_ldlt's 256 and 8 of counts
__host__ __device__ inline size_t surface_solve_lds_doubles(int gy, int gx) {
    const size_t T = (size_t)gy * gx, M = 2 * (size_t)(gy + 1) * (gx + 1);
    return T * kPhotoSurfPart + M * (kPhotoSurfBand + 7 + 3) + 32 + 256 + 8;
}

__global__ __launch_bounds__(kPhotoSurfSolveThreads) void photometric_surface_solve_kernel(PhotometricSurfaceArgs sa, int h, int w,
                                                                                            int rows, int bands, int slots,
                                                                                            int no_depth, int pass) {
    extern __shared__ double photo_lds[];
    const PhotometricRobustArgs& ra = sa.r;
    const PhotometricArgs& a = ra.p;
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gy = sa.cells_y, gx = sa.cells_x, T = gy * gx, nodes = (gy + 1) * (gx + 1), M = 2 * nodes, bw = 2 * gx + 5;
    double* cs = photo_lds;                             // [T][128]
    double* Cc = cs + (size_t)T * kPhotoSurfPart;       // [M][22]: column j = C_jj, C_{j+1, j} .. C_{j+21, j}
    double* R = Cc + (size_t)M * kPhotoSurfBand;        // [7][M]: B_g's six rows, d_g
    double* diag0 = R + 7 * M;                          // [M] the assembled diagonal
    double* dinv = diag0 + M;                           // [M] 1 / d_j, 0 for a dead unknown
    double* tq = dinv + M;                              // [M] t, then q
    double* S = tq + M;                                 // [32]: H' (21), g' (6), c', sum w
    double* Gs = S + 32;                                // [256] solve_ldlt's
    int* cnt = reinterpret_cast<int*>(Gs + 256);        // rows, holes, zero weights, live unknowns
    unsigned* hist = ra.hist + (size_t)pair * kPhotoBins;                         // as photometric_robust_solve_kernel clears it
    for (int i = tid; i < kPhotoBins; i += kPhotoSurfSolveThreads) hist[i] = 0u;
    double* state = ra.state + (size_t)pair * kPhotoSurfState;
    int32_t* si = reinterpret_cast<int32_t*>(state + 9);
    if (pass > 0 && si[1]) return;
    for (int i = tid; i < 256; i += kPhotoSurfSolveThreads) Gs[i] = 0.0;
    // 1. every cell's bands in ascending order
    const double* pair_ws = a.ws + (size_t)pair * bands * slots * gx * kPhotoSurfPart;
    for (int k = wave; k < T; k += kPhotoSurfSolveThreads / 64) {
        const int ty = k / gx, tx = k - ty * gx;
        const int tr0 = tile_begin(ty, h, gy), tr1 = tile_begin(ty + 1, h, gy);
        const int b0 = tr0 / rows, b1 = no_depth ? b0 : (tr1 - 1) / rows + 1;
        double lo = 0.0, hi = 0.0;                      // lane q: sums q and 64 + q; lanes 57, 58 of hi: the counts
        int cnt0 = 0, cnt1 = 0;
        for (int b = b0; b < b1; b += kPhotoSurfDepth) {
            double hl[kPhotoSurfDepth], hh[kPhotoSurfDepth];
#pragma unroll
            for (int u = 0; u < kPhotoSurfDepth; ++u) {
                const int bb = min(b + u, b1 - 1);
                const int slot = (slots > 1 && bb * rows < tr0) ? 1 : 0;      // the band began in the cell row before: its second slot
                const double* p = pair_ws + ((size_t)(bb * slots + slot) * gx + tx) * kPhotoSurfPart;
                hl[u] = b + u < b1 ? p[lane] : 0.0;
                hh[u] = b + u < b1 ? p[64 + lane] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kPhotoSurfDepth; ++u) {
                if (b + u >= b1) break;
                lo += hl[u];                            // ascending band order
                if (lane < 57) {
                    hi += hh[u];
                } else {
                    const unsigned long long bits = __builtin_bit_cast(unsigned long long, hh[u]);
                    cnt0 += (int)(unsigned)bits;
                    cnt1 += (int)(unsigned)(bits >> 32);
                }
            }
        }
        double* ck = cs + (size_t)k * kPhotoSurfPart;
        ck[lane] = lo;
        if (lane < 57) ck[64 + lane] = hi;
        else if (lane == 57) { int32_t* c = reinterpret_cast<int32_t*>(ck + 121); c[0] = cnt0; c[1] = cnt1; }
        else if (lane == 58) { int32_t* c = reinterpret_cast<int32_t*>(ck + 122); c[0] = cnt0; c[1] = 0; }
        if (sa.cell_sums) {
            double* out = sa.cell_sums + ((size_t)pair * T + k) * 120;
            out[lane] = lo;
            if (lane < 56) out[64 + lane] = hi;
        }
    }
    __syncthreads();
    // 2. the bordered system, every entry over its cells in ascending order from zero
    if (tid < 29) {
        const int q = tid < 28 ? tid : 120;
        double t = 0.0;
        for (int k = 0; k < T; ++k) t = t + cs[(size_t)k * kPhotoSurfPart + q];
        S[tid] = t;
    } else if (tid >= 32 && tid < 35) {
        int t = 0;
        for (int k = 0; k < T; ++k) t += reinterpret_cast<const int32_t*>(cs + (size_t)k * kPhotoSurfPart + 121)[tid - 32];
        cnt[tid - 32] = t;
    }
    for (int at = tid; at < M * kPhotoSurfBand; at += kPhotoSurfSolveThreads) {
        const int p = at / kPhotoSurfBand, o = at - p * kPhotoSurfBand, q = p + o;
        double t = 0.0;
        if (q < M && o <= bw) {
            const int na = p >> 1, nb = q >> 1;
            const int ia = na / (gx + 1), ja = na - ia * (gx + 1), ib = nb / (gx + 1), jb = nb - ib * (gx + 1);
            for (int ci = max(ib - 1, 0); ci <= min(ia, gy - 1); ++ci)
                for (int cj = max(max(ja, jb) - 1, 0); cj <= min(min(ja, jb), gx - 1); ++cj) {
                    const int s = 2 * ((ia - ci) * 2 + (ja - cj)) + (p & 1), u = 2 * ((ib - ci) * 2 + (jb - cj)) + (q & 1);
                    t = t + cs[(size_t)(ci * gx + cj) * kPhotoSurfPart + 76 + s * 8 - s * (s - 1) / 2 + (u - s)];
                }
        }
        Cc[at] = t;
        if (o == 0) { diag0[p] = t; dinv[p] = 0.0; tq[p] = 0.0; }
    }
    for (int at = tid; at < 7 * M; at += kPhotoSurfSolveThreads) {
        const int r = at / M, p = at - r * M, na = p >> 1;
        const int ia = na / (gx + 1), ja = na - ia * (gx + 1);
        double t = 0.0;
        for (int ci = max(ia - 1, 0); ci <= min(ia, gy - 1); ++ci)
            for (int cj = max(ja - 1, 0); cj <= min(ja, gx - 1); ++cj) {
                const int s = 2 * ((ia - ci) * 2 + (ja - cj)) + (p & 1);
                t = t + cs[(size_t)(ci * gx + cj) * kPhotoSurfPart + (r < 6 ? 28 + 8 * r + s : 112 + s)];
            }
        R[at] = t;
    }
    __syncthreads();
    const int n = cnt[0], holes = cnt[1], zeros = cnt[2];
    const bool tried = !no_depth && n >= 6 && n - zeros >= 6;
    // 3. the elimination, column by column: thread -> one entry behind the column
    int kind = 3, ua = 0, ub = 0;                       // 0: C (row ua, column ub of the window); 1: R (row ua, column ub); 2: S (ua, ub)
    {
        const int nwin = bw * (bw + 1) / 2;
        if (tid < nwin) {
            kind = 0;
            int q = tid;
            while (q > ua) { q -= ua + 1; ++ua; }       // row ua of the lower triangle has ua + 1 entries
            ub = q;
        } else if (tid < nwin + 7 * bw) {
            kind = 1;
            ua = (tid - nwin) / bw;
            ub = (tid - nwin) - ua * bw;
        } else if (tid < nwin + 7 * bw + 28) {
            kind = 2;
            const int q = tid - nwin - 7 * bw;
            if (q < 21) triu_index(q, ua, ub);
            else if (q < 27) { ua = q - 21; ub = 6; }
            else { ua = 6; ub = 6; }
        }
    }
    if (tried) {
        for (int j = 0; j < M; ++j) {
            const double d = Cc[j * kPhotoSurfBand], c0 = diag0[j];
            const bool live = (c0 > 0.0) && (d > kPivotThreshold * c0);
            if (live) {
                const double di = 1.0 / d;
                if (tid == 0) dinv[j] = di;
                if (kind == 0) {
                    if (j + 1 + ua < M) {
                        const double la = Cc[j * kPhotoSurfBand + 1 + ua] * di, lb = Cc[j * kPhotoSurfBand + 1 + ub] * di;
                        Cc[(j + 1 + ub) * kPhotoSurfBand + (ua - ub)] -= (la * lb) * d;
                    }
                } else if (kind == 1) {
                    if (j + 1 + ub < M) {
                        const double lr = R[ua * M + j] * di, lb = Cc[j * kPhotoSurfBand + 1 + ub] * di;
                        R[ua * M + j + 1 + ub] -= (lr * lb) * d;
                    }
                } else if (kind == 2) {
                    const double lr = R[ua * M + j] * di, ls = R[ub * M + j] * di;
                    const int q = ub < 6 ? ua * 6 - ua * (ua - 1) / 2 + (ub - ua) : (ua < 6 ? 21 + ua : 27);
                    S[q] -= (lr * ls) * d;
                }
            }
            lds_barrier();
        }
    }
    if (wave != 0) return;
    // 4. the 6 x 6 system, the unknowns
    int n_live = 0;
    for (int j = lane; j < M; j += 64) n_live += dinv[j] != 0.0 ? 1 : 0;
    n_live = wave_sum(n_live);
    if (lane < 27) {
        const double val = S[lane];
        const bool diag = lane == 0 || lane == 6 || lane == 11 || lane == 15 || lane == 18 || lane == 20;
        Gs[40 + lane] = diag ? val + a.mu * val : val;
    }
    wave_lds_fence();
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool solved = false;
    if (tried && n_live > 0) solved = solve_ldlt(Gs, lane, x);
    for (int j = lane; j < M; j += 64) {
        const double di = dinv[j];
        double t = 0.0;
        if (solved && di != 0.0) {
            t = R[6 * M + j] * di;
#pragma unroll
            for (int i = 0; i < 6; ++i) t = t + (R[i * M + j] * di) * -x[i];
        }
        tq[j] = t;
    }
    wave_lds_fence();
    if (solved) {
        for (int i = M - 1; i > 0; --i) {               // q_i is final; the live unknowns in front of it lose l_ij q_i
            const double qi = tq[i];
            const int j = i - 1 - lane;
            if (lane < bw && j >= 0) {
                const double di = dinv[j];
                if (di != 0.0) tq[j] -= (Cc[j * kPhotoSurfBand + 1 + lane] * di) * qi;
            }
            wave_lds_fence();
        }
    }
    for (int j = lane; j < M; j += 64) state[16 + j] = tq[j];
    for (int nd = lane; nd < nodes; nd += 64) {
        double* pn = sa.p_nodes + ((size_t)pair * nodes + nd) * 4;
        pn[0] = tq[2 * nd];
        pn[1] = tq[2 * nd + 1];
        pn[2] = (solved && dinv[2 * nd] != 0.0) ? 1.0 : 0.0;
        pn[3] = (solved && dinv[2 * nd + 1] != 0.0) ? 1.0 : 0.0;
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            state[i] = -x[i];
            a.v_p[(size_t)pair * 6 + i] = solved ? -a.lambda * x[i] : 0.0;
        }
        state[6] = 0.0;
        state[7] = 0.0;
        si[0] = n;
        si[1] = solved ? 0 : 1;
        a.p_status[pair] = no_depth ? ST_NO_DEPTH : solved ? ST_OK : ST_TOO_FEW;
        if (a.p_info) {
            int32_t* pi = a.p_info + (size_t)pair * 8;
            pi[0] = n; pi[1] = h; pi[2] = w; pi[3] = bands; pi[4] = holes; pi[5] = (tried && !solved) ? 1 : 0; pi[6] = zeros; pi[7] = pass;
        }
        double* pr = ra.p_robust + (size_t)pair * 4;
        pr[0] = solved ? (double)n_live : 0.0;
        pr[1] = solved ? (double)(M - n_live) : 0.0;
        pr[2] = (solved && pass > 0) ? state[8] : 0.0;
        pr[3] = solved ? S[28] : 0.0;
    }
}

int plan_photometric_surface(int height, int width, int level, int cells_y, int cells_x, int max_pairs, PhotometricSurfacePlan* plan) {
    if (!plan) return -2;
    if (int rc = plan_photometric_tiles(height, width, level, cells_y, cells_x, max_pairs, &plan->t)) return rc;
    plan->ws_doubles = (size_t)plan->t.bands * plan->t.slots * cells_x * kPhotoSurfPart;
    plan->lds_solve = surface_solve_lds_doubles(cells_y, cells_x) * sizeof(double);
    return 0;
}

size_t photometric_surface_ws_bytes(int max_pairs) {
    return (size_t)max_pairs * ((size_t)kPhotoTileSegs * 8 * kPhotoSurfPart * sizeof(double) + kPhotoBins * sizeof(uint32_t) +
                                kPhotoSurfState * sizeof(double));
}

int launch_photometric_surface(const PhotometricSurfaceArgs& sa_in, unsigned char* ws, int max_pairs, hipStream_t stream) {
    PhotometricSurfaceArgs sa = sa_in;
    PhotometricRobustArgs& ra = sa.r;
    PhotometricArgs& a = ra.p;
    if (a.n_pairs < 1 || a.n_pairs > 65535 || a.n_pairs > max_pairs || !a.I_cur || !a.I_des || !a.K || !ws || !a.v_p || !a.p_status ||
        !ra.p_robust || !sa.p_nodes)
        return -2;
    if (a.interaction < 0 || a.interaction > 1 || !(a.mu >= 0.0) || !(a.mu < __builtin_huge_val())) return -2;
    if (!(a.lambda == a.lambda) || !(a.depth_scale == a.depth_scale)) return -2;
    if (ra.iterations < 0 || ra.iterations > 4) return -2;
    if (!(ra.sigma_min > 0.0) || !(ra.sigma_min < __builtin_huge_val())) return -2;
    PhotometricSurfacePlan sp;
    if (int rc = plan_photometric_surface(a.height, a.width, a.level, sa.cells_y, sa.cells_x, a.n_pairs, &sp)) return rc;
    const PhotometricTilePlan& p = sp.t;
    ra.illumination = 1;
    // the block: the partials of max_pairs pairs at kPhotoTileSegs segment rows of 8 cell columns, then the histograms, then the states
    const size_t part_bytes = (size_t)max_pairs * kPhotoTileSegs * 8 * kPhotoSurfPart * sizeof(double);
    a.ws = reinterpret_cast<double*>(ws);
    ra.hist = reinterpret_cast<uint32_t*>(ws + part_bytes);
    ra.state = reinterpret_cast<double*>(ws + part_bytes + (size_t)max_pairs * kPhotoBins * sizeof(uint32_t));
    const int no_depth = (!a.Z_mm && !(a.depth_scale > 0.0)) ? 1 : 0;
    static std::atomic<unsigned long long> raised0{0}, raised1{0}, raised2{0}, raised3{0};
    if (sp.lds_solve > 64 * 1024 &&
        raise_lds_limit(reinterpret_cast<const void*>(photometric_surface_solve_kernel), 160 * 1024, raised3))
        return -3;
    if (no_depth) {
        launch(photometric_surface_solve_kernel, dim3(a.n_pairs), dim3(kPhotoSurfSolveThreads), sp.lds_solve, stream, sa, p.h, p.w, p.rows,
               p.bands, p.slots, 1, 0);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    if (p.lds > 64 * 1024 &&
        (raise_lds_limit(reinterpret_cast<const void*>(photometric_surface_rows_kernel<false>), 160 * 1024, raised0) ||
         raise_lds_limit(reinterpret_cast<const void*>(photometric_surface_rows_kernel<true>), 160 * 1024, raised1)))
        return -3;
    if (ra.iterations > 0 && p.lds_res > 64 * 1024 &&
        raise_lds_limit(reinterpret_cast<const void*>(photometric_surface_residual_kernel), 160 * 1024, raised2))
        return -3;
    const dim3 grid(p.bands, a.n_pairs);
    for (int pass = 0; pass <= ra.iterations; ++pass) {
        if (pass > 0) {
            launch(photometric_surface_residual_kernel, grid, dim3(256), p.lds_res, stream, sa, p.h, p.w, p.rows, p.bands);
            launch(photometric_surface_rows_kernel<true>, grid, dim3(256), p.lds, stream, sa, p.h, p.w, p.rows, p.bands, p.slots);
        } else {
            launch(photometric_surface_rows_kernel<false>, grid, dim3(256), p.lds, stream, sa, p.h, p.w, p.rows, p.bands, p.slots);
        }
        if (hipGetLastError() != hipSuccess) return -1;
        launch(photometric_surface_solve_kernel, dim3(a.n_pairs), dim3(kPhotoSurfSolveThreads), sp.lds_solve, stream, sa, p.h, p.w, p.rows,
               p.bands, p.slots, 0, pass);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

}  // namespace vitvs
