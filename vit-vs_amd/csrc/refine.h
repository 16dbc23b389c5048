// Sub-patch refinement of a match (option "subpatch"; no counterpart in the reference): the similarity of a
// goal token to the four neighbours of its best current-frame token says on which side of the patch centre the true match
// lies.  Per axis, the vertex of the parabola through the three neighbouring similarities (a, m, p at -1, 0, +1):
//   den = a - 2 m + p,   delta = clamp(0.5 (a - p) / den, -1/2, +1/2) when den < 0, else 0;   0 on the border row / column.
// One wavefront per goal token for the descriptor forms (every similarity a fixed-order reduction: per-lane chains of 16-byte
// loads, then wave_sum), one thread per goal token for the stencil form: deterministic either way.  Shared by the law's kernel
// (servo.hip, REFINE instantiations) and the stand-alone seam (correspond.hip refine_kernel, vitvs_refine_dev).
#pragma once
#include "common.h"

namespace vitvs {

__device__ __forceinline__ float refine_parabola(float a, float m, float p) {
    const float den = __fadd_rn(__fsub_rn(a, __fmul_rn(2.0f, m)), p);
    if (!(den < 0.f)) return 0.f;
    const float d = __fdiv_rn(__fmul_rn(0.5f, __fsub_rn(a, p)), den);
    return fminf(fmaxf(d, -0.5f), 0.5f);
}

// The match j (0 <= j < grid * grid) and its left / right and upper / lower neighbours (the match itself where there is none)
struct RefineSites {
    int nb[5];
    bool in_c, in_r;
};
__device__ __forceinline__ RefineSites refine_sites(int j, int grid) {
    const int r = j / grid, c = j - r * grid;
    RefineSites t;
    t.in_c = c > 0 && c < grid - 1;
    t.in_r = r > 0 && r < grid - 1;
    t.nb[0] = j;
    t.nb[1] = t.in_c ? j - 1 : j;
    t.nb[2] = t.in_c ? j + 1 : j;
    t.nb[3] = t.in_r ? j - grid : j;
    t.nb[4] = t.in_r ? j + grid : j;
    return t;
}
// (dr, dc) from the similarities of a goal token to the five sites of its match
__device__ __forceinline__ void refine_from_sims(const RefineSites& t, const float s[5], float& dr, float& dc) {
    dc = t.in_c ? refine_parabola(s[1], s[0], s[2]) : 0.f;
    dr = t.in_r ? refine_parabola(s[3], s[0], s[4]) : 0.f;
}

// Similarities from the descriptor forms (GRAM_F32, GRAM_SPLIT, GRAM_WIDE): L2-normalised fp32 rows, Dp a multiple of 4 and the
// rows 16-byte aligned.  One wave, one goal token: the five dot products share the loads of the goal row; each is a per-lane
// chain over the lane's 16-byte pieces in ascending order, then wave_sum.  (Measured: one workgroup draws ~28 GB/s of rows that
// miss its L2, whatever the number of loads in flight — four rows of a wave at once, all loads issued up front, was no faster —
// so the cost is the 6 Dp floats a row reads; profiles/subpatch.txt.)
__device__ __forceinline__ void refine_wave_sims(const float* __restrict__ d1, const float* __restrict__ d2, const RefineSites& t,
                                                 int Dp, int lane, float s[5]) {
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = lane * 4; k < Dp; k += 256) {
        const float4 x = *reinterpret_cast<const float4*>(d1 + k);
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const float4 y = *reinterpret_cast<const float4*>(d2 + (size_t)t.nb[q] * Dp + k);
            acc[q] = __fmaf_rn(x.x, y.x, acc[q]);
            acc[q] = __fmaf_rn(x.y, y.y, acc[q]);
            acc[q] = __fmaf_rn(x.z, y.z, acc[q]);
            acc[q] = __fmaf_rn(x.w, y.w, acc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] = wave_sum(acc[q]);
}

// Similarity source of the stencil form (GRAM_STENCIL): the raw Gram G [T][T] of the pair and the tokens' squared norms, nine
// reads per similarity in the arithmetic and summation order of gram_stencil_argmax_kernel.  No cross-lane traffic: a thread works on a token of its own.
struct RefineStencil {
    const float* G;
    const float* sq1;  // |t|^2 of the goal frame's tokens
    const float* sq2;  // of the current frame's
    int T, grid, i;
    __device__ __forceinline__ int clampi(int v) const { return min(max(v, 0), grid - 1); }
    __device__ __forceinline__ float rnorm(const float* s, int tok) const {
        const int y = tok / grid, x = tok - y * grid;
        float tot = 0.f;
#pragma unroll
        for (int o = 0; o < 9; ++o) tot += s[clampi(y + o / 3 - 1) * grid + clampi(x + o % 3 - 1)];
        return __fdiv_rn(1.0f, fmaxf(sqrtf(tot), 1e-8f));
    }
    __device__ __forceinline__ float operator()(int j) const {
        const int iy = i / grid, ix = i - iy * grid, jy = j / grid, jx = j - jy * grid;
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < 9; ++o)
            acc += G[(size_t)(clampi(iy + o / 3 - 1) * grid + clampi(ix + o % 3 - 1)) * T + clampi(jy + o / 3 - 1) * grid +
                     clampi(jx + o % 3 - 1)];
        return __fmul_rn(__fmul_rn(acc, rnorm(sq1, i)), rnorm(sq2, j));
    }
};

}  // namespace vitvs
