// The roll search: ViT tokens are not rotation invariant, so a current frame more than ~45 degrees of in-plane
// rotation away from the goal matches badly.  A quarter turn of a square frame is lossless and a quarter turn of its token grid
// is a permutation of token ids: the current frame is matched against the goal as its four quarter-turned copies (one des_shared
// call of four pairs), the best copy is picked, and its matches are carried back into the unturned frame, where the law runs.
//   quarter_turns_kernel   frames [n][S][S][3] -> [n][4][S][S][3], copy k = numpy.rot90(frame, k)
//   roll_pick_kernel       the four candidates' arg-max keys -> the winner k*, and pair 0's keys = the winner's tables in the
//                          unturned frame
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace vitvs {

constexpr int kTurnTile = 32;                       // pixels per tile side
constexpr int kTurnRow = kTurnTile * 3 + 4;         // LDS bytes per tile row (padded: a transposed read walks rows)

// One workgroup takes a tile of up to 32 x 32 pixels of one frame through LDS and writes it into all four copies: the reads and
// the writes of every copy are runs of bytes along image rows.  The last tile of a row / column is narrower when S % 32 != 0.
__global__ __launch_bounds__(256) void quarter_turns_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int S) {
    __shared__ uint8_t tile[kTurnTile * kTurnRow];
    const int tid = threadIdx.x, f = blockIdx.z;
    const int r0 = blockIdx.y * kTurnTile, c0 = blockIdx.x * kTurnTile;
    const int th = min(kTurnTile, S - r0), tw = min(kTurnTile, S - c0);
    const uint8_t* src = in + (size_t)f * S * S * 3;
    for (int idx = tid; idx < th * tw * 3; idx += 256) {
        const int r = idx / (tw * 3), rem = idx - r * (tw * 3);
        tile[r * kTurnRow + rem] = src[((size_t)(r0 + r) * S + c0) * 3 + rem];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the tile's place in copy k: origin (or0, oc0), oh x ow pixels (turned by an odd k: tw x th)
        const int oh = (k & 1) ? tw : th, ow = (k & 1) ? th : tw;
        const int or0 = k == 0 ? r0 : k == 1 ? S - c0 - tw : k == 2 ? S - r0 - th : c0;
        const int oc0 = k == 0 ? c0 : k == 1 ? r0 : k == 2 ? S - c0 - tw : S - r0 - th;
        uint8_t* dst = out + ((size_t)f * 4 + k) * S * S * 3;
        for (int idx = tid; idx < oh * ow * 3; idx += 256) {
            const int a = idx / (ow * 3), rem = idx - a * (ow * 3), b = rem / 3, ch = rem - 3 * b;
            // out[or0 + a][oc0 + b] = in[..]: k = 1: in[c][S-1-r], k = 2: in[S-1-r][S-1-c], k = 3: in[S-1-c][r], in tile coordinates
            const int lr = k == 0 ? a : k == 1 ? b : k == 2 ? th - 1 - a : th - 1 - b;
            const int lc = k == 0 ? b : k == 1 ? tw - 1 - a : k == 2 ? tw - 1 - b : a;
            dst[((size_t)(or0 + a) * S + oc0) * 3 + rem] = tile[lr * kTurnRow + lc * 3 + ch];
        }
    }
}

int launch_quarter_turns(const uint8_t* frames, uint8_t* out, int n, int S, hipStream_t stream) {
    if (!frames || !out || n <= 0 || n > 65535 || S <= 0) return -2;
    const int tiles = (S + kTurnTile - 1) / kTurnTile;
    if (tiles > 65535) return -2;
    launch(quarter_turns_kernel, dim3(tiles, tiles, n), dim3(256), 0, stream, frames, out, S);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// P_k(o) = numpy.rot90(arange(T).reshape(g, g), k).reshape(-1)[o]: the token of the unturned frame that sits at position o of
// the copy turned by k quarter turns
__device__ __forceinline__ int turned_token(int o, int g, int k) {
    const int r = o / g, c = o - r * g;
    return k == 1 ? c * g + (g - 1 - r) : k == 2 ? (g - 1 - r) * g + (g - 1 - c) : k == 3 ? (g - 1 - c) * g + r : o;
}

// One workgroup.  Candidate k's keys are pair k's rows of row_best / col_best ([4][T]).  Per candidate: n_mutual (the law's count),
// the fp64 mean of sim_1 over the mutual tokens, and the law's own same-image test (servo.hip phase 1: the same per-thread
// order, wave sum and sum of the four waves in fp32).  Every candidate goes through the same reduction tree, so equal tables give
// equal scores and the tie rule (the smallest k) is exact.
__global__ __launch_bounds__(256) void roll_pick_kernel(unsigned long long* row_best, unsigned long long* col_best, int T, int g,
                                                        double* __restrict__ scores, int32_t* __restrict__ roll_info,
                                                        int32_t* __restrict__ rolled) {
    __shared__ float fscr[4][4];
    __shared__ int iscr[4][4];
    __shared__ double dscr[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = 0; k < 4; ++k) {
        const unsigned long long* rb = row_best + (size_t)k * T;
        const unsigned long long* cb = col_best + (size_t)k * T;
        float ssum = 0.f;
        double msum = 0.0;
        int cnt = 0;
        for (int i = tid; i < T; i += 256) {
            const unsigned long long kr = rb[i];
            const int n1 = (int)best_index(kr);
            const float s1 = best_value(kr);
            ssum += s1;
            if (n1 >= 0 && n1 < T && (int)best_index(cb[n1]) == i) {
                ++cnt;
                msum += (double)s1;
            }
        }
        ssum = wave_sum(ssum);
        msum = wave_sum(msum);
        cnt = wave_sum(cnt);
        if (lane == 0) { fscr[k][wave] = ssum; dscr[k][wave] = msum; iscr[k][wave] = cnt; }
    }
    __syncthreads();
    // every thread decides alike
    int best = -1, same_best = 0;
    double best_score = 0.0;
    for (int k = 0; k < 4; ++k) {
        const float mean_sim = (fscr[k][0] + fscr[k][1] + fscr[k][2] + fscr[k][3]) / (float)T;
        const bool same_image = mean_sim > 0.99f;
        const int n_mutual = iscr[k][0] + iscr[k][1] + iscr[k][2] + iscr[k][3];
        const bool valid = same_image || (n_mutual > 0 && n_mutual < T);
        const double total = (dscr[k][0] + dscr[k][1]) + (dscr[k][2] + dscr[k][3]);
        const double score = (valid && n_mutual > 0) ? total / (double)n_mutual : __builtin_nan("");
        if (score == score && (best < 0 || score > best_score)) { best = k; best_score = score; same_best = same_image ? 1 : 0; }
        if (tid == 0) { scores[k] = score; roll_info[1 + k] = n_mutual; }
    }
    if (tid == 0) {
        roll_info[0] = best; roll_info[5] = same_best; roll_info[6] = 0; roll_info[7] = 0;
        *rolled = best > 0 ? 1 : 0;
    }
    if (best <= 0) return;                          // nothing to carry back: pair 0 keeps candidate 0's keys
    // the winner's tables in the unturned frame, into pair 0's rows (the winner's are another pair's: nothing is read after it
    // is overwritten): nn_1'[i] = P(nn_1[i]), sim_1' = sim_1, nn_2'[P(j)] = nn_2[j]
    const unsigned long long* rb = row_best + (size_t)best * T;
    const unsigned long long* cb = col_best + (size_t)best * T;
    for (int i = tid; i < T; i += 256) {
        const unsigned long long kr = rb[i];
        const int n1 = (int)best_index(kr);
        const int m1 = (n1 >= 0 && n1 < T) ? turned_token(n1, g, best) : n1;
        row_best[i] = (kr & 0xffffffff00000000ull) | (unsigned long long)(0xffffffffu - (unsigned)m1);
        col_best[turned_token(i, g, best)] = cb[i];
    }
}

int launch_roll_pick(unsigned long long* row_best, unsigned long long* col_best, int T, int grid, double* scores,
                     int32_t* roll_info, int32_t* rolled, hipStream_t stream) {
    if (!row_best || !col_best || !scores || !roll_info || !rolled || T <= 0 || grid <= 0 || grid * grid != T) return -2;
    launch(roll_pick_kernel, dim3(1), dim3(256), 0, stream, row_best, col_best, T, grid, scores, roll_info, rolled);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vitvs
