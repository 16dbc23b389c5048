// The robust core of the five Tukey IRLS laws (servo.hip, rig.hip, pose.hip, pose_rig.hip, homography.hip): the
// median of the residuals by rank counting and the re-weighting step.  The laws keep what differs between them: their residuals,
// their solves, the barriers around these two steps and where in LDS the cells sit.  At the end: the seeded draw of the two
// consensus starts (homography.hip, pose_core.h).
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace vitvs {

// the residual of a row or pair that takes no part: it ranks behind every live one and takes weight 0 from the weight formula
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;

// The two middle values (the same one for an odd count) of rho[0 .. n) among its n_live smallest into mid[0], mid[1], 256 threads.
// Rank counting: the values are >= +0, so their bit patterns order like the values (integer compares, no branches); ties are
// ordered by index, so every value has a rank of its own and each cell exactly one writer.
__device__ __forceinline__ void median_middles(const double* rho, int n, int n_live, double* mid, int tid) {
    const int m_lo = (n_live - 1) >> 1, m_hi = n_live >> 1;
    if (n <= 256) {
        if (tid < n) {
            const long long ki = __double_as_longlong(rho[tid]);
            int rank = 0;
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const long long kj = __double_as_longlong(rho[j]);
                rank += (int)(kj < ki) | ((int)(kj == ki) & (int)(j < tid));
            }
            if (rank == m_lo) mid[0] = __longlong_as_double(ki);
            if (rank == m_hi) mid[1] = __longlong_as_double(ki);
        }
    } else {
        // thousands of values: 4 per thread and pass over the others
        for (int i0 = tid; i0 < n; i0 += 4 * 256) {
            long long ki[4];
            int rank[4] = {0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < 4; ++u) ki[u] = __double_as_longlong(rho[min(i0 + 256 * u, n - 1)]);
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const long long kj = __double_as_longlong(rho[j]);
#pragma unroll
                for (int u = 0; u < 4; ++u) rank[u] += (int)(kj < ki[u]) | ((int)(kj == ki[u]) & (int)(j < i0 + 256 * u));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + 256 * u < n && rank[u] == m_lo) mid[0] = __longlong_as_double(ki[u]);
                if (i0 + 256 * u < n && rank[u] == m_hi) mid[1] = __longlong_as_double(ki[u]);
            }
        }
    }
}

// The Tukey step behind the median: sigma = max(1.4826 median, sigma_min), w = (1 - (rho / 4.6851 sigma)^2)^2 inside the cut-off
// and 0 outside, into wk[0 .. n) (and into `mirror` where that is not null); the zero weights of wave w are counted into
// zeros[w].  FLAGGED: only rows with flag > 0 take a weight or count as a zero.  Returns sigma.  The caller's barrier follows.
template <bool FLAGGED>
__device__ __forceinline__ double tukey_reweight(const double* rho, const double* flag, int n, const double* mid, double sigma_min,
                                                 double* wk, double* mirror, int* zeros, int tid) {
    const double sigma = fmax(1.4826 * ((mid[0] + mid[1]) * 0.5), sigma_min);
    const double cs = 4.6851 * sigma;
    int z = 0;
    for (int k = tid; k < n; k += 256) {
        const double t = rho[k] / cs;
        const double u = 1.0 - t * t;
        double w1;
        if constexpr (FLAGGED) {
            const bool us = flag[k] > 0.0;
            w1 = (us && t < 1.0) ? u * u : 0.0;
            z += (us && w1 == 0.0) ? 1 : 0;
        } else {
            w1 = t < 1.0 ? u * u : 0.0;
            z += w1 == 0.0 ? 1 : 0;
        }
        wk[k] = w1;
        if (mirror) mirror[k] = w1;
    }
    z = wave_sum(z);
    if ((tid & 63) == 0) zeros[tid >> 6] = z;
    return sigma;
}

// ---- the draw of the consensus starts (homography.hip: 4 rows; pose_core.h: 3 rows)
__device__ __forceinline__ unsigned consensus_mix(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The K (3 or 4) distinct positions of hypothesis j in a list of n_us usable rows, ascending (a row set gives one fit whatever the
// order it was drawn in): r_c = mix(mix(seed 0x9e3779b9 + j) + c) mod n_us for c = 0 .. 63, repeats rejected; false when 64 draws do
// not give K.
template <int K>
__device__ __forceinline__ bool consensus_draw(unsigned seed, int j, int n_us, int* pos) {
    static_assert(K == 3 || K == 4, "three- and four-row hypotheses");
    const unsigned base = consensus_mix(seed * 0x9e3779b9u + (unsigned)j);
    int p0 = -1, p1 = -1, p2 = -1, p3 = -1, cnt = 0;
    for (unsigned c = 0; c < 64u && cnt < K; ++c) {
        const int r = (int)(consensus_mix(base + c) % (unsigned)n_us);
        if (r == p0 || r == p1 || r == p2 || (K == 4 && r == p3)) continue;
        if (cnt == 0) p0 = r; else if (cnt == 1) p1 = r; else if (cnt == 2) p2 = r; else p3 = r;
        ++cnt;
    }
    if (cnt < K) return false;
    int t;
#define VITVS_CSWAP(a, b) if (b < a) { t = a; a = b; b = t; }
    if constexpr (K == 4) {
        VITVS_CSWAP(p0, p1) VITVS_CSWAP(p2, p3) VITVS_CSWAP(p0, p2) VITVS_CSWAP(p1, p3) VITVS_CSWAP(p1, p2)
        pos[0] = p0; pos[1] = p1; pos[2] = p2; pos[3] = p3;
    } else {
        VITVS_CSWAP(p0, p1) VITVS_CSWAP(p1, p2) VITVS_CSWAP(p0, p1)
        pos[0] = p0; pos[1] = p1; pos[2] = p2;
    }
#undef VITVS_CSWAP
    return true;
}

}  // namespace vitvs
