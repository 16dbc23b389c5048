// The robust core of the five Tukey IRLS laws (servo.hip, rig.hip, pose.hip, pose_rig.hip, homography.hip): the
// median of the residuals by rank counting and the re-weighting step.  The laws keep what differs between them: their residuals,
// their solves, the barriers around these two steps and where in LDS the cells sit.  (The consensus start of the pose and the
// homography law is consensus_core.h's.)
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

}  // namespace vitvs
