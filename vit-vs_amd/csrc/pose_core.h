// What the pose law (pose.hip) and the pose rig law (pose_rig.hip) share: the layout of the head of
// their dynamic LDS, the rank-counting median and Horn's solve (a cyclic Jacobi eigen-decomposition of the 4 x 4 matrix in fp64,
// all indices compile-time: no scratch).
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace vitvs {

constexpr unsigned long long kPoseInfBits = 0x7ff0000000000000ull;
// dynamic LDS in doubles: slices [8][32] | 64 results (see the kPose* offsets) | ROBUST: rho [ld] | w [ld]
constexpr int kPoseHead = 8 * 32 + 64;
constexpr int kPoseSum = 256;        // [0 .. 11): the centred sums
constexpr int kPoseCen = 256 + 12;   // sw, pc [3], qc [3]
constexpr int kPoseRt = 256 + 20;    // R [9] row-major, t [3], q [4]
constexpr int kPoseMid = 256 + 36;   // the two middle values of the median
constexpr int kPoseInt = 256 + 40;   // ints: [0] solve outcome (0 ok, 1 degenerate), [1] sweeps, [2 .. 6) the waves' zero weights,
                                     //       [6 .. 10) their usable rows, [10 .. 14) their holes

// The two middle values of rho[0 .. n) among its n_live smallest into mid[0], mid[1] (rig.hip's form of servo.hip's rank
// counting: every value has a rank of its own and each cell one writer).
__device__ __forceinline__ void pose_middles(const double* rho, int n, int n_live, double* mid, int tid) {
    const int m_lo = (n_live - 1) >> 1, m_hi = n_live >> 1;
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

// One Jacobi rotation of the symmetric A in the (P, Q) plane, accumulated into V (eigenvectors in columns)
template <int P, int Q>
__device__ __forceinline__ void pose_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = c * arp - s * arq;
            A[r][Q] = A[Q][r] = s * arp + c * arq;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// Horn's solve from the sums in sm (every lane of the calling wave computes the same): R, t, the quaternion; returns false when
// the clouds are degenerate (ev_1 - ev_2 <= 1e-8 of the two scatters: collinear points leave a rotation free)
__device__ __forceinline__ bool pose_solve(const double* sm, double (&R)[9], double (&t)[3], double (&q)[4], int& sweeps) {
    const double* S = sm + kPoseSum;
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    const double scatter = S[9] + S[10];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    double normsq = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) normsq += A[i][j] * A[i][j];
    sweeps = 0;
    for (int sw = 0; sw < 32; ++sw) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) off += A[p][r] * A[p][r];
        if (off <= 1e-40 * normsq) break;
        ++sweeps;
        pose_rotate<0, 1>(A, V); pose_rotate<0, 2>(A, V); pose_rotate<0, 3>(A, V);
        pose_rotate<1, 2>(A, V); pose_rotate<1, 3>(A, V); pose_rotate<2, 3>(A, V);
    }
    int i1 = 0;
    double ev1 = A[0][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > ev1) { ev1 = A[i][i]; i1 = i; }
    double ev2 = -__builtin_huge_val();
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i != i1) ev2 = fmax(ev2, A[i][i]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        q[r] = V[r][0];
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (i == i1) q[r] = V[r][i];
    }
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sg = q[0] / qn < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = sg * (q[r] / qn);
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    R[0] = a * a + b * b - c * c - d * d; R[1] = 2.0 * (b * c - a * d);         R[2] = 2.0 * (b * d + a * c);
    R[3] = 2.0 * (b * c + a * d);         R[4] = a * a - b * b + c * c - d * d; R[5] = 2.0 * (c * d - a * b);
    R[6] = 2.0 * (b * d - a * c);         R[7] = 2.0 * (c * d + a * b);         R[8] = a * a - b * b - c * c + d * d;
    const double* cen = sm + kPoseCen;
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = cen[4 + i] - ((R[3 * i] * cen[1] + R[3 * i + 1] * cen[2]) + R[3 * i + 2] * cen[3]);
    return !(ev1 - ev2 <= 1e-8 * scatter);
}

}  // namespace vitvs
