// consumer_device.hpp -- device helpers of the consumers' kernels that more than one unit compiles (consumer_kernels.hpp,
// cov_kernels.hpp): the lane / wave split of a point-major sweep and the cyclic Jacobi on a register matrix
// (DESIGN.md section 17).  Every helper is inlined and keeps no state; no kernel is defined here.
#pragma once
#include "ba_device.hpp"

namespace sfmba {

// A lane takes a run shorter than kStatsLongTrack; the runs it leaves (is_long) are taken by the whole wave afterwards,
// one after the other: run(q, b, e, X, Y, Z) with lane q's run [b, e) and point on every lane.  Uniform over the wave.
// (kStatsLongTrack itself stays in consumer_kernels.hpp, where the tests read it; restated here for cov_kernels.hpp, and
// consumer_kernels.hpp holds the two together.)
namespace restated { constexpr int kStatsLongTrack = 32; }
template <class Run>
__device__ __forceinline__ void for_each_long_run(bool is_long, int b, int e, double X, double Y, double Z, Run run) {
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int q = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int qb = __shfl(b, q), qe = __shfl(e, q);
        const double qX = __shfl(X, q), qY = __shfl(Y, q), qZ = __shfl(Z, q);
        run(q, qb, qe, qX, qY, qZ);
    }
}

// Cyclic Jacobi on a symmetric N x N matrix in registers, upper triangle row by row: sym<N>(i, j) is entry (i, j)'s place
template <int N>
__host__ __device__ constexpr int sym(int i, int j) {
    return i <= j ? N * i - i * (i - 1) / 2 + (j - i) : N * j - j * (j - 1) / 2 + (i - j);
}
// the rotation that annihilates a_pq (theta^2 = inf: t = 0; a zero pair: the identity, without a branch round live state)
__device__ __forceinline__ void jacobi_cs(double app, double aqq, double apq, double& t, double& c, double& s) {
    const double theta = (aqq - app) / (2.0 * apq);
    t = apq == 0.0 ? 0.0 : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}
// one rotation in the (P, Q) plane: a <- G^T a G, v <- v G
template <int N, int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[N * (N + 1) / 2], double (&v)[N * N]) {
    const double apq = a[sym<N>(P, Q)];
    double t, c, s;
    jacobi_cs(a[sym<N>(P, P)], a[sym<N>(Q, Q)], apq, t, c, s);
    a[sym<N>(P, P)] -= t * apq;
    a[sym<N>(Q, Q)] += t * apq;
    a[sym<N>(P, Q)] = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        if (r != P && r != Q) {
            const double arp = a[sym<N>(r, P)], arq = a[sym<N>(r, Q)];
            a[sym<N>(r, P)] = c * arp - s * arq;
            a[sym<N>(r, Q)] = s * arp + c * arq;
        }
        const double vrp = v[N * r + P], vrq = v[N * r + Q];
        v[N * r + P] = c * vrp - s * vrq;
        v[N * r + Q] = s * vrp + c * vrq;
    }
}
// the rotations of one sweep: (0, 1), (0, 2), ..., (0, N - 1), (1, 2), ..., (N - 2, N - 1)
template <int N, int P = 0, int Q = 1>
__device__ __forceinline__ void jacobi_rotate_all(double (&a)[N * (N + 1) / 2], double (&v)[N * N]) {
    jacobi_rotate<N, P, Q>(a, v);
    if constexpr (Q + 1 < N) jacobi_rotate_all<N, P, Q + 1>(a, v);
    else if constexpr (P + 2 < N) jacobi_rotate_all<N, P + 1, P + 2>(a, v);
}
// a <- eigenvalues on the diagonal, v (I on entry) <- eigenvectors in its columns: sweeps until the off-diagonal part is
// 1e-40 of the diagonal (a sweep squares that ratio) or has vanished
constexpr int kJacobiRegSweeps = 12;  // cap of the sweeps of a register matrix (a 4x4 converges in 4..7)
template <int N>
__device__ __forceinline__ void jacobi_sweeps(double (&a)[N * (N + 1) / 2], double (&v)[N * N]) {
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiRegSweeps; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = i + 1; j < N; ++j) off += fabs(a[sym<N>(i, j)]);
            dia += fabs(a[sym<N>(i, i)]);
        }
        if (!(off > 1e-40 * dia)) break;                         // (a NaN ends the loop too)
        jacobi_rotate_all<N>(a, v);
    }
}

}  // namespace sfmba
