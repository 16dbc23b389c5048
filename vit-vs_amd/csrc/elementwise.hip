// Bandwidth-bound pieces of the forward: image -> patch rows, LayerNorm, descriptor preparation.
// Reference arithmetic being replaced:
//   ToTensor + Normalize            dinov2_extractor.py:177-191 (mean/std :49-50)
//   patch extraction (Conv2d input) dinov2_extractor.py:141, 259; cls + pos_embed from the 3rd-party prepare_tokens
//   nn.LayerNorm(eps=1e-6)          dino_patch/block.py:57,75 (norm1 / norm2)
//   descriptor = blocks[11] output minus cls   dinov2_extractor.py:326-334; 3x3 log-bin :289-308
//   cosine normalisation x / max(|x|, 1e-8)    vitvs_v2.py:55 (torch CosineSimilarity)
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace vitvs {

// ------------------------------------------------------------------------------------ patchify
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(PatchifyArgs a, T* __restrict__ Ape, float* __restrict__ x) {
    const int Tn = a.grid * a.grid;
    const int n_img = a.n_des + a.n_cur;
    const int row = blockIdx.x;
    if (row >= n_img * Tn) {  // cls rows: x[img][0][:] = cls + pos[0]
        const int img = row - n_img * Tn;
        const size_t xrow = (size_t)img * (Tn + a.prefix);
        float* dst = x + xrow * a.D;
        for (int d = threadIdx.x; d < a.D; d += blockDim.x) dst[d] = a.cls[d] + a.pos[d];
        return;
    }
    const int img = row / Tn, t = row - img * Tn;
    const int ty = t / a.grid, tx = t - ty * a.grid;
    const uint8_t* src = (img < a.n_des) ? a.des + (size_t)img * a.S * a.S * 3
                                         : a.cur + (size_t)(img - a.n_des) * a.S * a.S * 3;
    const int pp = a.patch * a.patch;
    T* dst = Ape + (size_t)row * a.Kp * (kSplit<T> ? 2 : 1);   // f16x2 rows: 2 Kp fp16 (common.h)
    // 4 consecutive k per thread (same channel and patch row when patch % 4 == 0): one 8- or 16-byte write-through store
    // instead of four 2- or 4-byte stores; the patch-embedding GEMM reads these rows in the next launch
    if ((a.patch & 3) == 0) {
        for (int k4 = threadIdx.x * 4; k4 < a.Kp; k4 += blockDim.x * 4) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (k4 < 3 * pp) {
                const int c = k4 / pp, rem = k4 - c * pp;
                const int py = rem / a.patch, px = rem - py * a.patch;
                const uint8_t* s = src + ((size_t)(ty * a.stride + py) * a.S + tx * a.stride + px) * 3 + c;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)s[3 * j], 255.0f), a.mean[c]), a.std[c]);
            }
            if constexpr (kSplit<T>) {
                store_x2<true>(dst, k4, f32x4{v[0], v[1], v[2], v[3]});
            } else if constexpr (sizeof(T) == 4) {
                store_out<true>(reinterpret_cast<float*>(dst + k4), make_float4(v[0], v[1], v[2], v[3]));
            } else {
                const typename Vec16<T>::x4 h = {(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
                store_out<true>(dst + k4, h);
            }
        }
        return;
    }
    for (int k = threadIdx.x; k < a.Kp; k += blockDim.x) {
        float v = 0.f;
        if (k < 3 * pp) {
            const int c = k / pp, rem = k - c * pp;
            const int py = rem / a.patch, px = rem - py * a.patch;
            const int yy = ty * a.stride + py, xx = tx * a.stride + px;
            const float u = (float)src[((size_t)yy * a.S + xx) * 3 + c];
            v = __fdiv_rn(__fsub_rn(__fdiv_rn(u, 255.0f), a.mean[c]), a.std[c]);
        }
        if constexpr (kSplit<T>) store_x2_one(dst, k, v);
        else dst[k] = from_float<T>(v);
    }
}

// Camera-resolution frames: the reference's PIL resize in front of the path (vitvs_v2.py:474-475) applied while the patch
// rows are built — the resized image never exists in memory.  Workgroup = one token: the camera rows its
// patch draws on are filtered horizontally, for the patch's columns only, into LDS (Pillow's intermediate image: uint8,
// rounded and clipped as in Resample.c), then combined vertically, normalised and stored.  Same integer arithmetic as
// resize_bicubic_kernel (resize.hip), so every pixel is the one PIL produces, bit for bit; a camera row is filtered again by
// the ~1.5 patches above / below that share it (about 10 MFLOP of integer work per frame pair instead of a launch and a
// round trip of the resized image).
template <typename T>
__global__ __launch_bounds__(256) void patchify_resize_kernel(PatchifyArgs a, ResizeArgs r, T* __restrict__ Ape,
                                                              float* __restrict__ x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [rows][patch][3] intermediate pixels
    const int Tn = a.grid * a.grid;
    const int n_img = a.n_des + a.n_cur;
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= n_img * Tn) {  // cls rows: x[img][0][:] = cls + pos[0]
        const int img = row - n_img * Tn;
        float* dst = x + (size_t)img * (Tn + a.prefix) * a.D;
        for (int d = tid; d < a.D; d += blockDim.x) dst[d] = a.cls[d] + a.pos[d];
        return;
    }
    const int img = row / Tn, t = row - img * Tn;
    const int ty = t / a.grid, tx = t - ty * a.grid;
    const size_t frame = (size_t)r.in_h * r.in_w * 3;
    const uint8_t* im = (img < a.n_des) ? a.des + (size_t)img * frame : a.cur + (size_t)(img - a.n_des) * frame;
    const int y0 = ty * a.stride, x0 = tx * a.stride, row3 = a.patch * 3;
    const int ylast = y0 + a.patch - 1;
    const int rmin = r.yb[2 * y0];
    const int nrows = r.yb[2 * ylast] + r.yb[2 * ylast + 1] - rmin;   // <= r.rows: both bounds grow with y (checked on the host)
    for (int idx = tid; idx < nrows * row3; idx += 256) {
        const int rr = idx / row3, rem = idx - rr * row3;
        const int px = rem / 3, c = rem - px * 3;
        const int xx = x0 + px;
        const int xmin = r.xb[2 * xx], xcnt = r.xb[2 * xx + 1];
        const uint8_t* p = im + ((size_t)(rmin + rr) * r.in_w + xmin) * 3 + c;
        const int* k = r.xk + xx * r.ksx;
        int ss = 1 << (kResizePrecisionBits - 1);
        for (int i = 0; i < xcnt; ++i) ss += (int)p[3 * i] * k[i];
        smem[idx] = (unsigned char)resize_clip8(ss);
    }
    __syncthreads();
    const int pp = a.patch * a.patch;
    T* dst = Ape + (size_t)row * a.Kp * (kSplit<T> ? 2 : 1);
    for (int k = tid; k < a.Kp; k += 256) {
        float v = 0.f;
        if (k < 3 * pp) {
            const int c = k / pp, rem = k - c * pp;
            const int py = rem / a.patch, px = rem - py * a.patch;
            const int y = y0 + py;
            const int ymin = r.yb[2 * y] - rmin, ycnt = r.yb[2 * y + 1];
            const int* kk = r.yk + y * r.ksy;
            const unsigned char* col = smem + (ymin * a.patch + px) * 3 + c;
            int ss = 1 << (kResizePrecisionBits - 1);
            for (int i = 0; i < ycnt; ++i) ss += (int)col[i * row3] * kk[i];
            v = __fdiv_rn(__fsub_rn(__fdiv_rn((float)resize_clip8(ss), 255.0f), a.mean[c]), a.std[c]);
        }
        if constexpr (kSplit<T>) store_x2_one(dst, k, v);
        else dst[k] = from_float<T>(v);
    }
}

int launch_patchify(Precision p, const PatchifyArgs& a, const ResizeArgs* rs, void* Ape, float* x, hipStream_t stream) {
    const int n_img = a.n_des + a.n_cur;
    const int rows = n_img * a.grid * a.grid + n_img;
    if (rows <= 0 || a.Kp < 3 * a.patch * a.patch) return -2;
    if (rs) {
        const size_t lds = (size_t)rs->rows * a.patch * 3;
        if (lds == 0 || lds > 64 * 1024) return -3;
        if (p == PREC_X2)
            launch(patchify_resize_kernel<hx2>, dim3(rows), dim3(256), lds, stream, a, *rs, (hx2*)Ape, x);
        else if (p == PREC_F32)
            launch(patchify_resize_kernel<float>, dim3(rows), dim3(256), lds, stream, a, *rs, (float*)Ape, x);
        else if (p == PREC_F16)
            launch(patchify_resize_kernel<f16>, dim3(rows), dim3(256), lds, stream, a, *rs, (f16*)Ape, x);
        else
            launch(patchify_resize_kernel<bf16>, dim3(rows), dim3(256), lds, stream, a, *rs, (bf16*)Ape, x);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    if (p == PREC_X2)
        launch(patchify_kernel<hx2>, dim3(rows), dim3(256), 0, stream, a, (hx2*)Ape, x);
    else if (p == PREC_F32)
        launch(patchify_kernel<float>, dim3(rows), dim3(256), 0, stream, a, (float*)Ape, x);
    else if (p == PREC_F16)
        launch(patchify_kernel<f16>, dim3(rows), dim3(256), 0, stream, a, (f16*)Ape, x);
    else
        launch(patchify_kernel<bf16>, dim3(rows), dim3(256), 0, stream, a, (bf16*)Ape, x);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------ LayerNorm
// One wave per row; each lane owns NV float2 (D = 128*NV).  Two-pass moments in registers.
template <typename T, int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, T* __restrict__ out, int M,
                                                        float eps) {
    constexpr int D = 128 * NV;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= M) return;
    const float2* src = reinterpret_cast<const float2*>(x + (size_t)row * D);
    float2 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = src[i * 64 + lane];
        s += v[i].x + v[i].y;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float a = v[i].x - mean, b = v[i].y - mean;
        q += a * a + b * b;
    }
    const float var = wave_sum(q) / (float)D;
    const float rstd = 1.0f / sqrtf(var + eps);
    const float2* g2 = reinterpret_cast<const float2*>(gamma);
    const float2* b2 = reinterpret_cast<const float2*>(beta);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float2 g = g2[i * 64 + lane], b = b2[i * 64 + lane];
        const float y0 = (v[i].x - mean) * rstd * g.x + b.x;
        const float y1 = (v[i].y - mean) * rstd * g.y + b.y;
        T* dst = out + (size_t)row * D + 2 * (i * 64 + lane);
        if constexpr (kSplit<T>) {
            store_x2_one(out + (size_t)row * D * 2, 2 * (i * 64 + lane), y0);
            store_x2_one(out + (size_t)row * D * 2, 2 * (i * 64 + lane) + 1, y1);
        } else if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float2*>(dst) = make_float2(y0, y1);
        } else {
            typedef T t16x2 __attribute__((ext_vector_type(2)));
            const t16x2 h = {(T)y0, (T)y1};
            *reinterpret_cast<t16x2*>(dst) = h;
        }
    }
}

template <typename T>
static int launch_ln_t(const float* x, const float* g, const float* b, T* out, int M, int D, float eps,
                       hipStream_t stream) {
    dim3 grid(M), block(64);  // one wave per workgroup: 394 rows spread over all CUs
    switch (D) {
        case 384: launch((layernorm_kernel<T, 3>), grid, block, 0, stream, x, g, b, out, M, eps); break;
        case 768: launch((layernorm_kernel<T, 6>), grid, block, 0, stream, x, g, b, out, M, eps); break;
        case 1024: launch((layernorm_kernel<T, 8>), grid, block, 0, stream, x, g, b, out, M, eps); break;
        case 128: launch((layernorm_kernel<T, 1>), grid, block, 0, stream, x, g, b, out, M, eps); break;
        case 256: launch((layernorm_kernel<T, 2>), grid, block, 0, stream, x, g, b, out, M, eps); break;
        default: return -2;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_layernorm(Precision p, const float* x, const float* gamma, const float* beta, void* out, int M, int D,
                     float eps, hipStream_t stream) {
    if (M <= 0) return -2;
    if (p == PREC_X2) return launch_ln_t<hx2>(x, gamma, beta, (hx2*)out, M, D, eps, stream);
    if (p == PREC_F32) return launch_ln_t<float>(x, gamma, beta, (float*)out, M, D, eps, stream);
    if (p == PREC_F16) return launch_ln_t<f16>(x, gamma, beta, (f16*)out, M, D, eps, stream);
    return launch_ln_t<bf16>(x, gamma, beta, (bf16*)out, M, D, eps, stream);
}

// ------------------------------------------------------------------------------------ residual + LayerNorm
// Finishes a split-K linear layer: x += ls * (sum_z part[z] + bias), slices summed in index order,
// then (optionally) the next LayerNorm of the freshly updated row — one pass, one wave per row.
// Reference: dino_patch/block.py:90-96,112-115 (x + ls(f(norm(x)))), followed by the next norm.
// A row is D/4 float4; lane l < LANES owns float4 l, l + LANES, ... (NV4 of them): 16-byte accesses, every
// load of the row (x, every slice, the four parameter vectors) issued before the first add.
constexpr int SMAX = 8;  // most K slices splitk_slices() ever picks

// Split-K partial sums are written by the previous launch and read exactly once: non-temporal loads (+1.1 % updates/s).
__device__ __forceinline__ float4 load_once(const float4* p) {
    const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(t[0], t[1], t[2], t[3]);
}

enum RlnMode { RLN_PLAIN = 0, RLN_DESC = 1, RLN_EMBED = 2 };
struct RlnExtra {   // by-value tail argument of the DESC / EMBED variants
    DescOut desc;
    const float* pos = nullptr;   // EMBED: position embedding [1 + T][D]
    const float* cls = nullptr;   // EMBED: class token [D]
    const float* reg = nullptr;   // EMBED: register tokens [P - 1][D] (desc.P > 1 only)
};

// MODE = RLN_EMBED finishes the patch embedding instead of a block: x (write-only) = pos_embed + split-K sum +
// bias for the patch tokens (partial rows are [img][T], x rows [img][P + T]), cls + pos[0] for the class
// token, the register tokens as they are for rows 1 .. P - 1 (inserted after the position embedding: DINOv2's
// prepare_tokens_with_masks), followed by block 0's norm1 — so neither the embedding epilogue nor a LayerNorm
// launch is needed.
template <typename T, int NV4, int LANES, int MODE = RLN_PLAIN>
__global__ __launch_bounds__(64) void residual_ln_kernel(float* __restrict__ x, const float* __restrict__ part,
                                                         const float* __restrict__ bias, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, T* __restrict__ out, int splits,
                                                         int M, const float* __restrict__ ls, float eps, RlnExtra ex) {
    // argument order: the first 14 dwords are preloaded into SGPRs (kernarg preload); `ls` and `eps` are
    // fetched by the wave and first used after every other load is in flight
    constexpr bool DESC = MODE == RLN_DESC;
    constexpr int D = 4 * NV4 * LANES;
    const bool wt = M <= 2048;   // few rows: the launch is latency-bound, write-through stores help the consumer (common.h)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x;
    const bool on = lane < LANES;
    const int l = on ? lane : 0;
    float4* xr = reinterpret_cast<float4*>(x + (size_t)row * D);
    float4 v[NV4], pv[SMAX][NV4], bb[NV4], ll[NV4], gg[NV4], be[NV4];
    if constexpr (MODE == RLN_EMBED) {
        const int Tn = ex.desc.T, P = ex.desc.P, img = row / (Tn + P), j = row - img * (Tn + P), t = j - P;
        const int Mp = (M / (Tn + P)) * Tn;                       // rows of one partial slice
        const int prow = img * Tn + max(t, 0);
        const bool reg = t < 0 && j > 0;                          // register token j - 1: no pos, no bias
        const float4* posr = reinterpret_cast<const float4*>(reg ? ex.reg + (size_t)(j - 1) * D : ex.pos + (size_t)max(t + 1, 0) * D);
#pragma unroll
        for (int z = 0; z < SMAX; ++z)
            if (z < splits) {
                const float4* pz = reinterpret_cast<const float4*>(part + ((size_t)z * Mp + prow) * D);
#pragma unroll
                for (int i = 0; i < NV4; ++i) pv[z][i] = load_once(pz + i * LANES + l);
            }
#pragma unroll
        for (int i = 0; i < NV4; ++i) {
            const int c = i * LANES + l;
            v[i] = posr[c];
            bb[i] = reg ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(t >= 0 ? bias : ex.cls)[c];
            gg[i] = reinterpret_cast<const float4*>(gamma)[c];
            be[i] = reinterpret_cast<const float4*>(beta)[c];
        }
        if (t < 0) {   // class token (cls + pos[0]) or register: no patch-embedding terms
#pragma unroll
            for (int z = 0; z < SMAX; ++z)
#pragma unroll
                for (int i = 0; i < NV4; ++i) pv[z][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
#pragma unroll
        for (int z = 0; z < SMAX; ++z)
            if (z < splits) {
                const float4* pz = reinterpret_cast<const float4*>(part + ((size_t)z * M + row) * D);
#pragma unroll
                for (int i = 0; i < NV4; ++i) pv[z][i] = load_once(pz + i * LANES + l);
            }
#pragma unroll
        for (int i = 0; i < NV4; ++i) {
            const int c = i * LANES + l;
            v[i] = xr[c];
            bb[i] = reinterpret_cast<const float4*>(bias)[c];
            if (gamma) {
                gg[i] = reinterpret_cast<const float4*>(gamma)[c];
                be[i] = reinterpret_cast<const float4*>(beta)[c];
            }
        }
    }
    if (ls) {
#pragma unroll
        for (int i = 0; i < NV4; ++i) ll[i] = reinterpret_cast<const float4*>(ls)[i * LANES + l];
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        float4 acc = pv[0][i];
#pragma unroll
        for (int z = 1; z < SMAX; ++z)
            if (z < splits) {
                acc.x += pv[z][i].x; acc.y += pv[z][i].y; acc.z += pv[z][i].z; acc.w += pv[z][i].w;
            }
        acc.x += bb[i].x; acc.y += bb[i].y; acc.z += bb[i].z; acc.w += bb[i].w;
        if (ls) { acc.x *= ll[i].x; acc.y *= ll[i].y; acc.z *= ll[i].z; acc.w *= ll[i].w; }
        float4 r = v[i];
        r.x += acc.x; r.y += acc.y; r.z += acc.z; r.w += acc.w;
        if (on) {
            if (wt) store_out<true>(reinterpret_cast<float*>(xr + i * LANES + l), r);
            else store_out<false>(reinterpret_cast<float*>(xr + i * LANES + l), r);
        }
        v[i] = r;
        if (on) s += (r.x + r.y) + (r.z + r.w);
    }
    if constexpr (DESC) {
        // last block: the row is final; emit its L2-normalised descriptor (patch tokens only) and clear the
        // correspondence keys.  Same arithmetic as desc_plain_kernel; the same summation order, hence the same bits, where a
        // lane owns the same float4s as there (LANES = 64: D = 256, 768, 1024).  At D = 128 and 384 (LANES = 32) the 32 lanes
        // sum other partial sums: equal to fp32 rounding only (tests/test_gpu_ends_cover.py checks both)
        const DescOut& desc = ex.desc;
        const int gid = blockIdx.x * 64 + lane;
        if (gid < desc.zero_count) { desc.zero_a[gid] = 0ull; desc.zero_b[gid] = 0ull; }
        const int img = row / (desc.T + desc.P), t = row - img * (desc.T + desc.P) - desc.P;
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV4; ++i)
            if (on) s2 += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        const float sq = wave_sum(s2);
        const float nrm = fmaxf(sqrtf(sq), 1e-8f);
        if (desc.sq && t >= 0 && lane == 0) desc.sq[(size_t)img * desc.T + t] = sq;
        if (desc.dn && t >= 0 && on) {
            float4* dst = reinterpret_cast<float4*>(desc.dn + ((size_t)img * desc.T + t) * D);
#pragma unroll
            for (int i = 0; i < NV4; ++i)
                store_out<true>(reinterpret_cast<float*>(dst + i * LANES + l),
                                make_float4(__fdiv_rn(v[i].x, nrm), __fdiv_rn(v[i].y, nrm), __fdiv_rn(v[i].z, nrm),
                                            __fdiv_rn(v[i].w, nrm)));
        }
    }
    if (!gamma) return;
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
        if (on) q += (a * a + b * b) + (c * c + d * d);
    }
    const float var = wave_sum(q) / (float)D;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (!on) return;
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        const float y0 = (v[i].x - mean) * rstd * gg[i].x + be[i].x;
        const float y1 = (v[i].y - mean) * rstd * gg[i].y + be[i].y;
        const float y2 = (v[i].z - mean) * rstd * gg[i].z + be[i].z;
        const float y3 = (v[i].w - mean) * rstd * gg[i].w + be[i].w;
        T* dst = out + (size_t)row * D + 4 * (i * LANES + l);
        if constexpr (kSplit<T>) {
            if (wt) store_x2<true>(out + (size_t)row * D * 2, 4 * (i * LANES + l), f32x4{y0, y1, y2, y3});
            else store_x2<false>(out + (size_t)row * D * 2, 4 * (i * LANES + l), f32x4{y0, y1, y2, y3});
        } else if constexpr (sizeof(T) == 4) {
            if (wt) store_out<true>(dst, make_float4(y0, y1, y2, y3));
            else store_out<false>(dst, make_float4(y0, y1, y2, y3));
        } else {
            const typename Vec16<T>::x4 h = {(T)y0, (T)y1, (T)y2, (T)y3};
            if (wt) store_out<true>(dst, h);
            else store_out<false>(dst, h);
        }
    }
}

template <typename T, int MODE>
static int launch_rln_t(float* x, const float* part, int splits, const float* bias, const float* ls, const float* g,
                        const float* b, T* out, int M, int D, float eps, hipStream_t stream, const RlnExtra& ex) {
    const dim3 grid(M), block(64);   // one wave per workgroup: 394 rows spread over all CUs
#define VITVS_RLN(NV4, LANES) \
    launch((residual_ln_kernel<T, NV4, LANES, MODE>), grid, block, 0, stream, x, part, bias, g, b, out, splits, M, ls, eps, ex)
    switch (D) {
        case 128: VITVS_RLN(1, 32); break;
        case 256: VITVS_RLN(1, 64); break;
        case 384: VITVS_RLN(3, 32); break;
        case 768: VITVS_RLN(3, 64); break;
        case 1024: VITVS_RLN(4, 64); break;
        default: return -2;
    }
#undef VITVS_RLN
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int MODE>
static int launch_rln_p(Precision p, float* x, const float* part, int splits, const float* bias, const float* ls,
                        const float* g, const float* b, void* out, int M, int D, float eps, hipStream_t stream,
                        const RlnExtra& ex) {
    if (p == PREC_X2) return launch_rln_t<hx2, MODE>(x, part, splits, bias, ls, g, b, (hx2*)out, M, D, eps, stream, ex);
    if (p == PREC_F32) return launch_rln_t<float, MODE>(x, part, splits, bias, ls, g, b, (float*)out, M, D, eps, stream, ex);
    if (p == PREC_F16) return launch_rln_t<f16, MODE>(x, part, splits, bias, ls, g, b, (f16*)out, M, D, eps, stream, ex);
    return launch_rln_t<bf16, MODE>(x, part, splits, bias, ls, g, b, (bf16*)out, M, D, eps, stream, ex);
}

int launch_residual_ln(Precision p, float* x, const float* part, int splits, const float* bias, const float* ls,
                       const float* gamma, const float* beta, void* out, int M, int D, float eps, hipStream_t stream,
                       const DescOut* desc) {
    if (M <= 0 || splits < 1 || splits > SMAX) return -2;
    RlnExtra ex;
    if (!desc) return launch_rln_p<RLN_PLAIN>(p, x, part, splits, bias, ls, gamma, beta, out, M, D, eps, stream, ex);
    if (gamma || (!desc->dn && !desc->sq) || desc->T <= 0 || desc->P < 1 || M % (desc->T + desc->P) != 0 || desc->zero_count > M * 64) return -2;
    ex.desc = *desc;
    return launch_rln_p<RLN_DESC>(p, x, part, splits, bias, ls, gamma, beta, out, M, D, eps, stream, ex);
}

int launch_embed_ln(Precision p, float* x, const float* part, int splits, const float* bias, const float* pos,
                    const float* cls, const float* reg, const float* gamma, const float* beta, void* out, int n_img, int T,
                    int P, int D, float eps, hipStream_t stream) {
    if (n_img <= 0 || T <= 0 || P < 1 || splits < 1 || splits > SMAX || !gamma || !beta || !pos || !cls || (P > 1 && !reg))
        return -2;
    RlnExtra ex;
    ex.desc.T = T;
    ex.desc.P = P;
    ex.pos = pos;
    ex.cls = cls;
    ex.reg = reg;
    return launch_rln_p<RLN_EMBED>(p, x, part, splits, bias, nullptr, gamma, beta, out, n_img * (T + P), D, eps, stream, ex);
}

// ------------------------------------------------------------------------------------ descriptors
// plain: one wave per patch token: dn = x / max(||x||, 1e-8)
__global__ __launch_bounds__(256) void desc_plain_kernel(const float* __restrict__ x, float* __restrict__ dn,
                                                         float* __restrict__ raw, int n_img, int T, int P, int D,
                                                         unsigned long long* zero_a, unsigned long long* zero_b,
                                                         int zero_count) {
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    {   // clears the packed (similarity, index) keys the Gram kernel will atomicMax into
        const int gid = blockIdx.x * blockDim.x + threadIdx.x;
        if (gid < zero_count) { zero_a[gid] = 0ull; zero_b[gid] = 0ull; }
    }
    if (tok >= n_img * T) return;
    const int img = tok / T, t = tok - img * T;
    const float4* src = reinterpret_cast<const float4*>(x + ((size_t)img * (T + P) + P + t) * D);
    // the row is read once, 16 bytes per lane (D <= 1024 -> at most 4 float4 per lane), and kept in registers
    const int n4 = D >> 2;
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = i * 64 + lane;
        v[i] = (c < n4) ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
    const float nrm = fmaxf(sqrtf(wave_sum(s)), 1e-8f);
    float4* dst = reinterpret_cast<float4*>(dn + (size_t)tok * D);
    float4* rw = raw ? reinterpret_cast<float4*>(raw + (size_t)tok * D) : nullptr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = i * 64 + lane;
        if (c < n4) {
            dst[c] = make_float4(__fdiv_rn(v[i].x, nrm), __fdiv_rn(v[i].y, nrm), __fdiv_rn(v[i].z, nrm),
                                 __fdiv_rn(v[i].w, nrm));
            if (rw) rw[c] = v[i];
        }
    }
}

__global__ __launch_bounds__(256) void token_sqnorm_kernel(const float* __restrict__ x, float* __restrict__ sq,
                                                           int n_img, int T, int P, int D, unsigned long long* zero_a,
                                                           unsigned long long* zero_b, int zero_count) {
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    {
        const int gid = blockIdx.x * blockDim.x + threadIdx.x;
        if (gid < zero_count) { zero_a[gid] = 0ull; zero_b[gid] = 0ull; }
    }
    if (tok >= n_img * T) return;
    const int img = tok / T, t = tok - img * T;
    const float* src = x + ((size_t)img * (T + P) + P + t) * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float v = src[d];
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) sq[tok] = s;
}

// binned: block per token; the 9 neighbour tokens (row-major dy,dx, replicate-clamped) are
// concatenated and the 9D vector normalised.
__global__ __launch_bounds__(256) void desc_binned_kernel(const float* __restrict__ x, const float* __restrict__ sq,
                                                          float* __restrict__ dn, float* __restrict__ raw, int n_img,
                                                          int T, int P, int grid, int D) {
    const int tok = blockIdx.x;
    const int img = tok / T, t = tok - img * T;
    const int ty = t / grid, tx = t - ty * grid;
    int nb[9];
    float tot = 0.f;
#pragma unroll
    for (int o = 0; o < 9; ++o) {
        const int yy = min(max(ty + o / 3 - 1, 0), grid - 1);
        const int xx = min(max(tx + o % 3 - 1, 0), grid - 1);
        nb[o] = yy * grid + xx;
        tot += sq[img * T + nb[o]];
    }
    const float nrm = fmaxf(sqrtf(tot), 1e-8f);
    float* dst = dn + (size_t)tok * 9 * D;
    for (int e = threadIdx.x; e < 9 * D; e += blockDim.x) {
        const int o = e / D, d = e - o * D;
        const float v = x[((size_t)img * (T + P) + P + nb[o]) * D + d];
        if (dn) dst[e] = __fdiv_rn(v, nrm);
        if (raw) raw[(size_t)tok * 9 * D + e] = v;
    }
}

__global__ __launch_bounds__(256) void normalize_rows_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                             int rows, int Dp) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* s = src + (size_t)row * Dp;
    float acc = 0.f;
    for (int d = lane; d < Dp; d += 64) acc += s[d] * s[d];
    const float nrm = fmaxf(sqrtf(wave_sum(acc)), 1e-8f);
    for (int d = lane; d < Dp; d += 64) dst[(size_t)row * Dp + d] = __fdiv_rn(s[d], nrm);
}

__global__ __launch_bounds__(256) void copy16_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, unsigned n16) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u) dst[i] = __builtin_nontemporal_load(src + i);
}

int launch_copy16(const void* src, void* dst, size_t bytes, hipStream_t stream) {
    const size_t n16 = (bytes + 15) / 16;
    if (n16 == 0 || n16 >= (1ull << 32)) return -2;
    const unsigned wgs = (unsigned)std::min<size_t>((n16 + 255) / 256, 1024);
    launch(copy16_kernel, dim3(wgs), dim3(256), 0, stream, (const u32x4*)src, (u32x4*)dst, (unsigned)n16);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

__global__ __launch_bounds__(256) void touch_kernel(const u32x4* __restrict__ p, unsigned n16, int share, unsigned* __restrict__ sink) {
    const unsigned xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;
    unsigned lo = 0, hi = n16;
    if (share) { lo = (unsigned)((unsigned long long)n16 * xcd / 8); hi = (unsigned)((unsigned long long)n16 * (xcd + 1) / 8); }
    unsigned acc = 0;
    for (unsigned i = lo + slot * 256u + threadIdx.x; i < hi; i += slots * 256u) {
        const u32x4 v = p[i];
        acc ^= v[0] ^ v[1] ^ v[2] ^ v[3];
    }
    if (acc == 0x9e3779b9u && sink) *sink = acc;       // keeps the loads; practically never taken
}

int launch_touch(const void* p, size_t bytes, int share_xcds, hipStream_t stream) {
    const size_t n16 = bytes / 16;
    if (n16 == 0 || n16 >= (1ull << 32)) return -2;
    launch(touch_kernel, dim3(256), dim3(256), 0, stream, (const u32x4*)p, (unsigned)n16, share_xcds, (unsigned*)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_normalize_rows(const float* src, float* dst, int rows, int Dp, hipStream_t stream) {
    if (rows <= 0 || Dp <= 0) return -2;
    launch(normalize_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, src, dst, rows, Dp);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Facet descriptors (query / key / value of blocks[layer], dinov2_extractor.py:193-217, 326-334): from the qkv
// GEMM's output [n_img*(P+T)][3][H][64] to fp32 [n_img][T][D] with descriptor index d * H + h, cls and register tokens dropped.
template <typename T>
__global__ __launch_bounds__(256) void facet_kernel(const T* __restrict__ qkv, float* __restrict__ out, int Tn, int P, int H,
                                                    int which, float unscale, int keep_cls) {
    // keep_cls = 0: out [n_img][T][D] (cls dropped); 1: out [n_img][1 + T][D] (registers dropped)
    const int rows = Tn + keep_cls;
    const int tok = blockIdx.x, img = tok / rows, t = tok - img * rows;
    const int D = H * 64;
    const size_t qrow = (size_t)img * (Tn + P) + ((keep_cls && t == 0) ? 0 : P - keep_cls + t);
    float* dst = out + (size_t)tok * D;
    for (int j = threadIdx.x; j < D; j += 256) {
        const int h = j % H, d = j / H;
        if constexpr (kSplit<T>) dst[j] = load_x2(qkv + qrow * 3 * D * 2, which * D + h * 64 + d) * unscale;
        else dst[j] = (float)qkv[qrow * 3 * D + (size_t)which * D + h * 64 + d] * unscale;
    }
}

int launch_facet(Precision p, const void* qkv, float* out, int n_img, int T, int P, int H, int which, float q_unscale, int keep_cls,
                 hipStream_t stream) {
    if (n_img <= 0 || T <= 0 || P < 1 || H <= 0 || which < 0 || which > 2) return -2;
    const dim3 grid(n_img * (T + (keep_cls ? 1 : 0)));
    const int kc = keep_cls ? 1 : 0;
    if (p == PREC_X2) launch(facet_kernel<hx2>, grid, dim3(256), 0, stream, (const hx2*)qkv, out, T, P, H, which, q_unscale, kc);
    else if (p == PREC_F32) launch(facet_kernel<float>, grid, dim3(256), 0, stream, (const float*)qkv, out, T, P, H, which, q_unscale, kc);
    else if (p == PREC_F16) launch(facet_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)qkv, out, T, P, H, which, q_unscale, kc);
    else launch(facet_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)qkv, out, T, P, H, which, q_unscale, kc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Saliency maps (ViTExtractor.extract_saliency_maps, dinov2_extractor.py:339-353: the 'attn' facet of the last block, hooked
// behind attn_drop): the class token's attention row softmax(q_cls . K^T * hd^-0.5) over ALL P + T keys (cls, registers,
// patches), patch columns only,
// averaged over the chosen heads, then min-max normalised per image.  One workgroup per image; the row of each head is formed
// in LDS (scores, max, exp, sum) — P + T dot products of 64 per head, nothing worth the matrix pipe.
struct SaliencyHeads { int n; int idx[16]; };
template <typename T>
__global__ __launch_bounds__(256) void saliency_kernel(const T* __restrict__ qkv, float* __restrict__ out, int Tn, int P, int H,
                                                       SaliencyHeads heads, float scale, int base2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* row = reinterpret_cast<float*>(smem);          // [P + T] scores, then probabilities of one head
    float* acc = row + (Tn + P);                          // [T] sum over the heads
    __shared__ float red[8];
    __shared__ float qs[64];
    const int img = blockIdx.x, tid = threadIdx.x, N = Tn + P, D = H * 64;
    const T* base = qkv + (size_t)img * N * 3 * D;
    for (int j = tid; j < Tn; j += 256) acc[j] = 0.f;
    auto block_reduce = [&](float v, bool is_max) {
        v = is_max ? wave_max(v) : wave_sum(v);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
    };
    for (int hi = 0; hi < heads.n; ++hi) {
        const int h = heads.idx[hi];
        __syncthreads();
        if (tid < 64) qs[tid] = (float)base[h * 64 + tid];                        // q of the class token (row 0)
        __syncthreads();
        float mx = -INFINITY;
        for (int j = tid; j < N; j += 256) {
            const T* k = base + (size_t)j * 3 * D + D + h * 64;
            float s = 0.f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) s = fmaf(qs[d], (float)k[d], s);
            s *= scale;
            row[j] = s;
            mx = fmaxf(mx, s);
        }
        mx = block_reduce(mx, true);
        float sum = 0.f;
        for (int j = tid; j < N; j += 256) {
            const float e = base2 ? exp2f(row[j] - mx) : expf(row[j] - mx);
            row[j] = e;
            sum += e;
        }
        sum = block_reduce(sum, false);
        for (int j = tid; j < Tn; j += 256) acc[j] += __fdiv_rn(row[j + P], sum);
    }
    __syncthreads();
    float lo = INFINITY, hi = -INFINITY;
    for (int j = tid; j < Tn; j += 256) {
        const float m = __fdiv_rn(acc[j], (float)heads.n);                        // .mean(dim=1)
        acc[j] = m;
        lo = fminf(lo, m);
        hi = fmaxf(hi, m);
    }
    hi = block_reduce(hi, true);
    lo = -block_reduce(-lo, true);
    for (int j = tid; j < Tn; j += 256) out[(size_t)img * Tn + j] = __fdiv_rn(acc[j] - lo, hi - lo);
}

int launch_saliency(Precision p, const void* qkv, float* out, int n_img, int T, int P, int H, const int* head_idx, int n_heads,
                    bool q_prescaled, hipStream_t stream) {
    if (n_img <= 0 || T <= 0 || P < 1 || H <= 0 || n_heads <= 0 || n_heads > 16) return -2;
    if (p == PREC_X2) return -2;   // the saliency surface is frozen (outside SURVEY section 8): fp32 / bf16 / fp16 handles only
    SaliencyHeads hs;
    hs.n = n_heads;
    for (int i = 0; i < n_heads; ++i) {
        if (head_idx[i] < 0 || head_idx[i] >= H) return -2;
        hs.idx[i] = head_idx[i];
    }
    const size_t lds = (size_t)(2 * T + P) * sizeof(float);
    if (lds > 64 * 1024) return -3;
    // 16-bit modes: the q rows of the qkv weights carry hd^-0.5 * log2(e) (kAttnQScale), so the scores are in log2 units
    const float scale = q_prescaled ? 1.0f : 0.125f;
    const int base2 = q_prescaled ? 1 : 0;
    if (p == PREC_F32) launch(saliency_kernel<float>, dim3(n_img), dim3(256), lds, stream, (const float*)qkv, out, T, P, H, hs, scale, base2);
    else if (p == PREC_F16) launch(saliency_kernel<f16>, dim3(n_img), dim3(256), lds, stream, (const f16*)qkv, out, T, P, H, hs, scale, base2);
    else launch(saliency_kernel<bf16>, dim3(n_img), dim3(256), lds, stream, (const bf16*)qkv, out, T, P, H, hs, scale, base2);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_descriptors(const float* x, float* dn, float* raw, float* sqnorm_ws, int n_img, int T, int P, int grid, int D,
                       int binned, unsigned long long* zero_a, unsigned long long* zero_b, int zero_count,
                       hipStream_t stream) {
    const int toks = n_img * T;
    if (toks <= 0 || P < 1 || grid * grid != T || zero_count > toks * 64) return -2;
    if (!binned) {
        launch(desc_plain_kernel, dim3((toks + 3) / 4), dim3(256), 0, stream, x, dn, raw, n_img, T, P, D,
                           zero_a, zero_b, zero_count);
    } else {
        launch(token_sqnorm_kernel, dim3((toks + 3) / 4), dim3(256), 0, stream, x, sqnorm_ws, n_img, T, P, D,
                           zero_a, zero_b, zero_count);
        launch(desc_binned_kernel, dim3(toks), dim3(256), 0, stream, x, sqnorm_ws, dn, raw, n_img, T, P, grid,
                           D);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vitvs
