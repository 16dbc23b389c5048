// The homography law: servo a planar target from the matched image points alone, no depth.
//   m_k  = (x, y)      the current normalised image point of feature row k (feat of the camera's law; the moved match under subpatch)
//   m*_k = (xs, ys)    its goal point, from s_uv and K
//   H, m* ~ H m        the 3 x 3 homography of the plane: Hartley normalisation of either point set, the 9 x 9 DLT normal matrix
//                      M = sum w (r0 r0^T + r1 r1^T), its eigenvector of the smallest eigenvalue, H = T*^-1 H^ T, det H = 1
//   v_h = -lambda (z^ (H - I) m_c, (H21 - H12, H02 - H20, H10 - H01))      Benhimane and Malis' law (IJRR 2007), a twist in the
//                      current camera's own optical frame; m_c the weighted centroid of the current points, z^ the depth scale
// One launch, one 256-thread workgroup per pair; nothing passes between workgroups.  Phase A writes the points and the usable flag
// of every row into the pair's block of a global workspace that this workgroup alone writes and reads, behind __syncthreads() (as
// pose_kernel does): any max_rows works.  Every solve takes three passes over the rows (centroids, mean distances, the 45 sums of
// M), each as quantities x 8 row slices (row r belongs to slice r mod 8, ascending rows, the slices added in ascending order):
// bit-reproducible.  Wave 0 then runs the cyclic Jacobi eigen-decomposition of M with M and V (162 doubles) in LDS: every lane
// computes the same rotation, lanes 0 .. 8 turn the rows of M and lanes 16 .. 24 the rows of V, in the reference's order of
// arithmetic.  ROBUST: n_iter Tukey re-weightings on the transfer error with rho and w in dynamic LDS (median_middles and
// tukey_reweight of robust_core.h), one more solve behind the last.  CONSENSUS: a phase between Phase A and the solve loop scores
// n_hyp four-point hypotheses, one per thread and round, and starts the loop from the winner's consensus set (consensus_core.h's
// consensus_start on the model HomFourPoint below).
#include "common.h"
#include "consensus_core.h"
#include "kernels.h"
#include "robust_core.h"
#include "solve.h"

#pragma clang fp contract(off)

namespace vitvs {

// dynamic LDS in doubles: slices [8][64] | the results below | ROBUST: rho [ld] | w [ld] | CONSENSUS: consensus_core.h's cells and
// row list
constexpr int kHomSum = 8 * 64;          // [0 .. 45): the upper triangle of M, row-major
constexpr int kHomCen = kHomSum + 48;    // sw, c [2], c* [2], dbar, dbar*, trace(M)
constexpr int kHomA = kHomCen + 8;       // M [9][9], turned in place
constexpr int kHomV = kHomA + 81;        // V [9][9], eigenvectors in columns
constexpr int kHomH = kHomV + 81;        // H [9] row-major, m_c [2]
constexpr int kHomMid = kHomH + 12;      // the two middle values of the median
constexpr int kHomInt = kHomMid + 2;     // ints: [0] solve outcome (0 ok, 1 degenerate), [1] sweeps, [2 .. 6) the waves' zero weights,
                                         //       [6 .. 10) their usable rows, [10 .. 14) their rows with rho = inf
constexpr int kHomHead = kHomInt + 8;

// Orders the LDS traffic of ONE wave: its lanes run in lock step and the LDS serves a wave's accesses in issue order, so this
// only has to keep the compiler from moving them.
__device__ __forceinline__ void hom_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Element e of the two DLT rows of a normalised pair: r0 = (-x, -y, -1, 0, 0, 0, xs x, xs y, xs), r1 = (0, 0, 0, -x, -y, -1, ys x,
// ys y, ys)
__device__ __forceinline__ void hom_dlt(int e, double x, double y, double xs, double ys, double& r0, double& r1) {
    const int blk = e / 3, c = e - 3 * blk;
    const double ac = c == 0 ? x : (c == 1 ? y : 1.0);
    r0 = blk == 0 ? -ac : (blk == 1 ? 0.0 : xs * ac);
    r1 = blk == 0 ? 0.0 : (blk == 1 ? -ac : ys * ac);
}

// (i, j), i <= j, of entry q of the row-major upper triangle of a 9 x 9 matrix
__device__ __forceinline__ void hom_pair(int q, int& i, int& j) {
    i = 0;
    while (q >= 9 - i) { q -= 9 - i; ++i; }
    j = i + q;
}

// Wave 0, all 64 lanes: the eigenvector of M's smallest eigenvalue -> H with det H = 1 into sm[kHomH ..) (lane 0 writes); returns
// false when the set is degenerate.  Every lane returns the same.
__device__ __forceinline__ bool hom_solve(double* sm, int lane, int& sweeps) {
    double* A = sm + kHomA;
    double* V = sm + kHomV;
    for (int e = lane; e < 81; e += 64) {
        const int i = e / 9, j = e - 9 * i, lo = min(i, j), hi = max(i, j);
        A[e] = sm[kHomSum + lo * 9 - (lo * (lo - 1)) / 2 + (hi - lo)];
        V[e] = i == j ? 1.0 : 0.0;
    }
    hom_wave_sync();
    double normsq = 0.0, trace = 0.0;
    for (int e = 0; e < 81; ++e) normsq += A[e] * A[e];
    for (int i = 0; i < 9; ++i) trace += A[i * 10];
    sweeps = 0;
    for (int sw = 0; sw < 32; ++sw) {
        double off = 0.0;
        for (int p = 0; p < 9; ++p)
            for (int r = p + 1; r < 9; ++r) off += A[p * 9 + r] * A[p * 9 + r];
        if (off <= 1e-40 * normsq) break;
        ++sweeps;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = A[p * 9 + q];
                if (apq == 0.0) continue;
                const double app = A[p * 10], aqq = A[q * 10];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                hom_wave_sync();                                // (every lane has read its three before anyone writes)
                if (lane < 9) {
                    const int r = lane;
                    if (r == p) {
                        A[p * 10] = app - t * apq;
                        A[q * 10] = aqq + t * apq;
                        A[p * 9 + q] = 0.0;
                        A[q * 9 + p] = 0.0;
                    } else if (r != q) {
                        const double arp = A[r * 9 + p], arq = A[r * 9 + q];
                        const double np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
                        A[r * 9 + p] = np_; A[p * 9 + r] = np_;
                        A[r * 9 + q] = nq_; A[q * 9 + r] = nq_;
                    }
                } else if (lane >= 16 && lane < 25) {
                    const int r = lane - 16;
                    const double vrp = V[r * 9 + p], vrq = V[r * 9 + q];
                    V[r * 9 + p] = c * vrp - s * vrq;
                    V[r * 9 + q] = s * vrp + c * vrq;
                }
                hom_wave_sync();
            }
    }
    // the smallest eigenvalue (ties: the lowest index) and the second smallest
    int i0 = 0;
    double ev0 = A[0];
    for (int i = 1; i < 9; ++i) {
        const double d = A[i * 10];
        if (d < ev0) { ev0 = d; i0 = i; }
    }
    double ev1 = __builtin_huge_val();
    for (int i = 0; i < 9; ++i)
        if (i != i0) ev1 = fmin(ev1, A[i * 10]);
    bool ok = !(ev1 <= 1e-8 * trace);
    double hh[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) hh[k] = V[k * 9 + i0];
    // H = T*^-1 H^ T, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
    const double* cen = sm + kHomCen;
    const double s = 1.4142135623730951 / cen[5], ss = 1.4142135623730951 / cen[6];
    double G[9], H[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        G[3 * i] = hh[3 * i] * s;
        G[3 * i + 1] = hh[3 * i + 1] * s;
        G[3 * i + 2] = hh[3 * i + 2] - (G[3 * i] * cen[1] + G[3 * i + 1] * cen[2]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        H[j] = G[j] / ss + cen[3] * G[6 + j];
        H[3 + j] = G[3 + j] / ss + cen[4] * G[6 + j];
        H[6 + j] = G[6 + j];
    }
    const double det = (H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6])) + H[2] * (H[3] * H[7] - H[4] * H[6]);
    double fro2 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) fro2 += H[k] * H[k];
    const double fro = sqrt(fro2);
    if (fabs(det) <= 1e-8 * (fro * fro * fro)) ok = false;
    const double sc = cbrt(det);
    if (lane == 0 && ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) sm[kHomH + k] = H[k] / sc;
        sm[kHomH + 9] = cen[1];
        sm[kHomH + 10] = cen[2];
    }
    return ok;
}

// ---- the model of the consensus start ("The consensus start"; the phase itself is consensus_core.h's);
// tests/homography_consensus_ref.py restates every line below in the same order of arithmetic

// B = A diag(adj(A) (x3, y3, 1)), A with the columns (x_i, y_i, 1), i = 0 .. 2: the map of the projective basis onto four points.
// The l_i and their sum (det A) are twice the signed areas of the four triangles of the points: false when one of them is <= 1e-8
// of the squared extent, i.e. three points are collinear (of four collinear points every l_i is rounding noise, and so would be H
// and its determinant: the rule on det H cannot see that case).
__device__ __forceinline__ bool hom_basis(const double* x, const double* y, double* B) {
    const double l0 = ((y[1] - y[2]) * x[3] + (x[2] - x[1]) * y[3]) + (x[1] * y[2] - x[2] * y[1]);
    const double l1 = ((y[2] - y[0]) * x[3] + (x[0] - x[2]) * y[3]) + (x[2] * y[0] - x[0] * y[2]);
    const double l2 = ((y[0] - y[1]) * x[3] + (x[1] - x[0]) * y[3]) + (x[0] * y[1] - x[1] * y[0]);
    B[0] = x[0] * l0; B[1] = x[1] * l1; B[2] = x[2] * l2;
    B[3] = y[0] * l0; B[4] = y[1] * l1; B[5] = y[2] * l2;
    B[6] = l0; B[7] = l1; B[8] = l2;
    const double ex = fmax(fmax(x[0], x[1]), fmax(x[2], x[3])) - fmin(fmin(x[0], x[1]), fmin(x[2], x[3]));
    const double ey = fmax(fmax(y[0], y[1]), fmax(y[2], y[3])) - fmin(fmin(y[0], y[1]), fmin(y[2], y[3]));
    const double ext = ex + ey;
    const double area = fmin(fmin(fabs(l0), fabs(l1)), fmin(fabs(l2), fabs((l0 + l1) + l2)));
    return area > 1e-8 * (ext * ext);
}

// The homography of the four usable rows `rows` in closed form, H = B(m*) adj(B(m)) on the raw normalised points, with the sign
// that makes det H > 0 (what the law's det-1 scaling does); false when three of the points are collinear in either image, an entry
// is not finite or |det H| <= 1e-8 |H|_F^3
__device__ __forceinline__ bool hom_four_point(const double* ws, int ld, const int* rows, double* H) {
    double x[4], y[4], xs[4], ys[4], B[9], S[9], J[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[i] = ws[rows[i]]; y[i] = ws[(size_t)ld + rows[i]];
        xs[i] = ws[(size_t)2 * ld + rows[i]]; ys[i] = ws[(size_t)3 * ld + rows[i]];
    }
    const bool spread = hom_basis(x, y, B), spread_s = hom_basis(xs, ys, S);
    J[0] = B[4] * B[8] - B[5] * B[7]; J[1] = B[2] * B[7] - B[1] * B[8]; J[2] = B[1] * B[5] - B[2] * B[4];
    J[3] = B[5] * B[6] - B[3] * B[8]; J[4] = B[0] * B[8] - B[2] * B[6]; J[5] = B[2] * B[3] - B[0] * B[5];
    J[6] = B[3] * B[7] - B[4] * B[6]; J[7] = B[1] * B[6] - B[0] * B[7]; J[8] = B[0] * B[4] - B[1] * B[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) H[3 * i + k] = (S[3 * i] * J[k] + S[3 * i + 1] * J[3 + k]) + S[3 * i + 2] * J[6 + k];
    const double det = (H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6])) + H[2] * (H[3] * H[7] - H[4] * H[6]);
    double fro2 = 0.0;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        fro2 += H[k] * H[k];
        finite = finite && fabs(H[k]) < __builtin_huge_val();
    }
    const double fro = sqrt(fro2);
    if (!spread || !spread_s || !finite || !(fabs(det) > 1e-8 * (fro * fro * fro))) return false;
    if (det < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = -H[k];
    }
    return true;
}

// The squared transfer error of row r under H: |pi(H m) - m*|^2, or +inf where the third component of H m is <= 0
__device__ __forceinline__ double hom_transfer_sq(const double* H, const double* ws, int ld, int r) {
    const double x = ws[r], y = ws[(size_t)ld + r];
    const double X = (H[0] * x + H[1] * y) + H[2], Y = (H[3] * x + H[4] * y) + H[5], Z = (H[6] * x + H[7] * y) + H[8];
    if (!(Z > 0.0)) return __longlong_as_double((long long)kInfBits);
    const double d0 = X / Z - ws[(size_t)2 * ld + r], d1 = Y / Z - ws[(size_t)3 * ld + r];
    return d0 * d0 + d1 * d1;
}

// One hypothesis of the law's consensus start (consensus_core.h's consensus_start): four rows, the homography in closed form
struct HomFourPoint {
    static constexpr int kRows = 4, kFlagRow = 4, kFit = 9;                    // H, row-major
    static __device__ __forceinline__ bool fit(const double* ws, int ld, const int* rows, double* H) {
        return hom_four_point(ws, ld, rows, H);
    }
    static __device__ __forceinline__ double residual_sq(const double* H, const double* ws, int ld, int r) {
        return hom_transfer_sq(H, ws, ld, r);
    }
};

template <bool ROBUST, bool CONSENSUS>
__global__ __launch_bounds__(256) void homography_kernel(HomographyArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smh[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = a.ld;
    double* ws = a.ws + (size_t)b * 5 * ld;                 // x [ld] | y [ld] | xs [ld] | ys [ld] | flag [ld]: 1 usable, else 0
    int* iscr = reinterpret_cast<int*>(smh + kHomInt);
    double* rho = smh + kHomHead;
    double* wk = rho + ld;
    double* vout = a.v_h + (size_t)b * 6;

    // the early outs: a camera without matches, the same-image shortcut (the camera is at the goal: v = 0, H = I exactly).  A
    // camera that only lacks a depth image (ST_NO_DEPTH) has written its rows all the same and goes on
    const int cam = a.status ? a.status[b] : (int)ST_OK;
    const bool stop = cam == ST_NO_CORRESPONDENCE || cam == ST_TOO_FEW;
    const bool same = a.info && a.info[(size_t)b * 8 + 2] != 0;
    if (stop || same) {
        if (a.weights)
            for (int k = tid; k < a.weights_stride; k += 256) a.weights[(size_t)b * a.weights_stride + k] = 0.0;
        if (tid < 6) vout[tid] = 0.0;
        if (tid < 9 && a.H) a.H[(size_t)b * 9 + tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0 : 0.0;
        if (tid < 8 && a.h_info) a.h_info[(size_t)b * 8 + tid] = 0;
        if (tid == 0) {
            a.h_status[b] = stop ? cam : (int)ST_OK;
            if (a.sigma) a.sigma[b] = 0.0;
        }
        return;
    }

    // Phase A: the points.  n rows take part: the rows the camera's law wrote (info[1]), or every row of given points
    int n = ld, n_us = 0;
    if (a.m) {
        const double* mb = a.m + (size_t)b * ld * 2;
        const double* sb = a.ms + (size_t)b * ld * 2;
        const int32_t* ub = a.usable + (size_t)b * ld;
        for (int k = tid; k < n; k += 256) {
            const bool f = ub[k] > 0;
            ws[k] = f ? mb[k * 2] : 0.0;
            ws[(size_t)ld + k] = f ? mb[k * 2 + 1] : 0.0;
            ws[(size_t)2 * ld + k] = f ? sb[k * 2] : 0.0;
            ws[(size_t)3 * ld + k] = f ? sb[k * 2 + 1] : 0.0;
            ws[(size_t)4 * ld + k] = f ? 1.0 : 0.0;
            n_us += f;
        }
    } else {
        n = min(max(a.info[(size_t)b * 8 + 1], 0), ld);
        const double fx = a.K[b * 4 + 0], fy = a.K[b * 4 + 1], cx = a.K[b * 4 + 2], cy = a.K[b * 4 + 3];
        const int32_t* sel = a.selected + (size_t)b * ld;
        const int32_t* uv = a.s_uv + (size_t)b * ld * 4;
        const double* ft = a.feat + (size_t)b * ld * 4;
        for (int k = tid; k < n; k += 256) {
            const bool f = sel[k] >= 0;
            ws[k] = f ? ft[k * 4 + 1] : 0.0;
            ws[(size_t)ld + k] = f ? ft[k * 4 + 2] : 0.0;
            ws[(size_t)2 * ld + k] = f ? ((double)uv[k * 4 + 0] - cx) / fx : 0.0;
            ws[(size_t)3 * ld + k] = f ? ((double)uv[k * 4 + 1] - cy) / fy : 0.0;
            ws[(size_t)4 * ld + k] = f ? 1.0 : 0.0;
            n_us += f;
        }
    }
    n_us = wave_sum(n_us);
    if (lane == 0) iscr[6 + wave] = n_us;
    __syncthreads();                                        // (the points are global memory: full fence)
    n_us = iscr[6] + iscr[7] + iscr[8] + iscr[9];
    const double* flag = ws + (size_t)4 * ld;

    double sigma_min = a.sigma_min;
    if (a.K) sigma_min = 0.5 * fmax(a.pitch_u / a.K[b * 4 + 0], a.pitch_v / a.K[b * 4 + 1]);
    if constexpr (ROBUST) {
        for (int k = tid; k < n; k += 256) {
            wk[k] = flag[k];
            rho[k] = __longlong_as_double((long long)kInfBits);
        }
        lds_barrier();
    }

    const int qid = tid & 31, slice = tid >> 5;
    int status = ST_OK, sweeps = 0, reweighted = 0, n_zero = 0, degenerate = 0, n_inf = 0;
    double sigma = 0.0;
    int winner = 0, n_start = 0;
    if constexpr (CONSENSUS) {
        if (n_us >= 4) {
            winner = consensus_start<ROBUST, HomFourPoint>(ws, ld, n, n_us, a.n_hyp, a.seed, 4.6851 * sigma_min,
                                                           rho + (ROBUST ? 2 * ld : 0), ROBUST ? wk : ws + (size_t)4 * ld, n_start);
            if (winner) n_zero = n_us - n_start;            // the rows outside the consensus set start at weight 0
        }
    }
    const int N = ROBUST ? a.n_iter : 0;
    for (int it = 0;; ++it) {
        if (n_us - n_zero < 4) { status = ST_TOO_FEW; break; }
        // the weighted centroids: sw, sum w m, sum w m*
        if (qid < 5) {
            double acc = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : flag[r];
                acc += qid == 0 ? w : w * ws[(size_t)(qid - 1) * ld + r];
            }
            smh[slice * 64 + qid] = acc;
        }
        lds_barrier();
        if (tid < 5) {
            double s = 0.0, s0 = 0.0;
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) { s += smh[sl * 64 + tid]; s0 += smh[sl * 64]; }
            smh[kHomCen + tid] = tid == 0 ? s : s / s0;
        }
        lds_barrier();
        // the mean distances from the centroids
        if (qid < 2) {
            const int o = 2 * qid;
            const double c0 = smh[kHomCen + 1 + o], c1 = smh[kHomCen + 2 + o];
            double acc = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : flag[r];
                const double d0 = ws[(size_t)o * ld + r] - c0, d1 = ws[(size_t)(o + 1) * ld + r] - c1;
                acc += w * sqrt(d0 * d0 + d1 * d1);
            }
            smh[slice * 64 + qid] = acc;
        }
        lds_barrier();
        if (tid < 2) {
            double s = 0.0;
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) s += smh[sl * 64 + tid];
            smh[kHomCen + 5 + tid] = s / smh[kHomCen];
        }
        lds_barrier();
        const double db = smh[kHomCen + 5], dbs = smh[kHomCen + 6];
        if (!(db > 0.0) || !(dbs > 0.0)) { sweeps = 0; degenerate = 1; status = ST_TOO_FEW; break; }
        // M: entries qid and qid + 32 of its upper triangle
        {
            const double* cen = smh + kHomCen;
            const double s = 1.4142135623730951 / db, ss = 1.4142135623730951 / dbs;
            int i0, j0, i1, j1;
            hom_pair(qid, i0, j0);
            hom_pair(min(qid + 32, 44), i1, j1);
            double acc0 = 0.0, acc1 = 0.0;
            for (int r = slice; r < n; r += 8) {
                const double w = ROBUST ? wk[r] : flag[r];
                const double x = (ws[r] - cen[1]) * s, y = (ws[(size_t)ld + r] - cen[2]) * s;
                const double xs = (ws[(size_t)2 * ld + r] - cen[3]) * ss, ys = (ws[(size_t)3 * ld + r] - cen[4]) * ss;
                double p0, p1, q0, q1;
                hom_dlt(i0, x, y, xs, ys, p0, p1);
                hom_dlt(j0, x, y, xs, ys, q0, q1);
                acc0 += w * (p0 * q0 + p1 * q1);
                hom_dlt(i1, x, y, xs, ys, p0, p1);
                hom_dlt(j1, x, y, xs, ys, q0, q1);
                acc1 += w * (p0 * q0 + p1 * q1);
            }
            smh[slice * 64 + qid] = acc0;
            smh[slice * 64 + 32 + qid] = acc1;
        }
        lds_barrier();
        if (tid < 45) {
            double s = 0.0;
#pragma unroll
            for (int sl = 0; sl < 8; ++sl) s += smh[sl * 64 + tid];
            smh[kHomSum + tid] = s;
        }
        lds_barrier();
        if (wave == 0) {
            int sw;
            const bool ok = hom_solve(smh, lane, sw);
            if (lane == 0) {
                iscr[0] = ok ? 0 : 1;
                iscr[1] = sw;
            }
        }
        lds_barrier();
        sweeps = iscr[1];
        if (iscr[0]) { degenerate = 1; status = ST_TOO_FEW; break; }
        if (it == N) break;
        if constexpr (ROBUST) {
            double H[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) H[i] = smh[kHomH + i];
            int infs = 0;
            for (int k = tid; k < n; k += 256) {
                if (!(flag[k] > 0.0)) continue;             // not a usable row: rho stays +inf
                const double x = ws[k], y = ws[(size_t)ld + k];
                const double X = (H[0] * x + H[1] * y) + H[2], Y = (H[3] * x + H[4] * y) + H[5], Z = (H[6] * x + H[7] * y) + H[8];
                double r = __longlong_as_double((long long)kInfBits);
                if (Z > 0.0) {
                    const double d0 = X / Z - ws[(size_t)2 * ld + k], d1 = Y / Z - ws[(size_t)3 * ld + k];
                    r = sqrt(d0 * d0 + d1 * d1);
                } else {
                    ++infs;
                }
                rho[k] = r;
            }
            infs = wave_sum(infs);
            if (lane == 0) iscr[10 + wave] = infs;
            lds_barrier();
            median_middles(rho, n, n_us, smh + kHomMid, tid);
            lds_barrier();
            sigma = tukey_reweight<true>(rho, flag, n, smh + kHomMid, sigma_min, wk, nullptr, iscr + 2, tid);
            lds_barrier();
            n_zero = iscr[2] + iscr[3] + iscr[4] + iscr[5];
            n_inf = iscr[10] + iscr[11] + iscr[12] + iscr[13];
            reweighted = it + 1;
        }
    }

    if (a.weights) {
        for (int k = tid; k < a.weights_stride; k += 256) {
            double w = 0.0;
            if (k < n) w = ROBUST ? wk[k] : flag[k];
            a.weights[(size_t)b * a.weights_stride + k] = w;
        }
    }
    if (tid != 0) return;
    const bool ok = status == ST_OK;
    double v[6] = {0, 0, 0, 0, 0, 0}, H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (ok) {
#pragma unroll
        for (int i = 0; i < 9; ++i) H[i] = smh[kHomH + i];
        const double mx = smh[kHomH + 9], my = smh[kHomH + 10];
        const double en[3] = {((H[0] - 1.0) * mx + H[1] * my) + H[2], (H[3] * mx + (H[4] - 1.0) * my) + H[5],
                              (H[6] * mx + H[7] * my) + (H[8] - 1.0)};
        const double ew[3] = {H[7] - H[5], H[2] - H[6], H[3] - H[1]};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v[i] = -a.lambda * (a.depth_scale * en[i]);
            v[3 + i] = -a.lambda * ew[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) vout[i] = v[i];
    a.h_status[b] = status;
    if (a.H) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.H[(size_t)b * 9 + i] = H[i];
    }
    if (a.sigma) a.sigma[b] = sigma;
    if (a.h_info) {
        int32_t* hi = a.h_info + (size_t)b * 8;
        hi[0] = n_us; hi[1] = sweeps; hi[2] = reweighted; hi[3] = n_zero; hi[4] = degenerate; hi[5] = n_inf;
        hi[6] = CONSENSUS ? winner : 0; hi[7] = CONSENSUS ? n_start : 0;
    }
}

int plan_homography(int max_rows, int n_iter, int n_hyp, HomographyPlan* plan) {
    if (!plan || max_rows < 1 || n_iter < 0 || n_iter > 16 || n_hyp < 0 || n_hyp > 4096) return -2;
    plan->robust = n_iter > 0;
    plan->consensus = n_hyp > 0;
    plan->lds = ((size_t)kHomHead + (plan->robust ? (size_t)2 * max_rows : 0) + (plan->consensus ? consensus_lds_doubles(max_rows) : 0)) *
                sizeof(double);
    plan->lds_opt_in = plan->lds > 64 * 1024;
    return plan->lds > 160 * 1024 ? -3 : 0;
}

size_t homography_scratch_bytes(int n_pairs, int ld) { return (size_t)n_pairs * 5 * ld * sizeof(double); }

int launch_homography(const HomographyArgs& a, hipStream_t stream) {
    if (a.n_pairs < 1 || a.ld < 1 || !a.ws || !a.v_h || !a.h_status || (a.weights && a.weights_stride < 0)) return -2;
    if (a.m ? (!a.ms || !a.usable) : (!a.selected || !a.s_uv || !a.feat || !a.info || !a.K)) return -2;
    if (!(a.depth_scale > 0.0) || !(a.depth_scale < __builtin_huge_val())) return -2;
    HomographyPlan p;
    if (int rc = plan_homography(a.ld, a.n_iter, a.n_hyp, &p)) return rc;
    if (p.consensus && !a.K && !(a.sigma_min > 0.0)) return -2;      // the cut-off T = 4.6851 sigma_min has to be positive
    if (p.robust) {
        return p.consensus ? launch_planned<homography_kernel<true, true>>(p, a, stream)
                           : launch_planned<homography_kernel<true, false>>(p, a, stream);
    }
    return p.consensus ? launch_planned<homography_kernel<false, true>>(p, a, stream)
                       : launch_planned<homography_kernel<false, false>>(p, a, stream);
}

}  // namespace vitvs
