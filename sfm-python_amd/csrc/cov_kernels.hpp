// cov_kernels.hpp -- the kernels of sfmba_covariance (covariance.hip): the undamped linearisation
// at x (V_p^-1 with a pivot test, U_c), the Cholesky factorisation and in-place inverse of the reduced camera matrix S in
// LDS, the point blocks Sigma_pp by a point-major sweep, and the per-camera blocks and standard deviations.  The blocks of
// W V^-1 W^T come from the solver's k_schur_blocks through its launcher (handle.hpp).  No atomics; every sum runs in a
// fixed order: same input, same bits.
#pragma once
#include "consumer_device.hpp"

namespace sfmba {

constexpr int kCovThreads = 256;                             // the point-major kernels and k_cov_reduce
constexpr int kCovMaxN = restated::kDenseMaxN;               // unknowns of the factorisation: S in LDS
constexpr int kCovFactorThreads = restated::kDenseThreads;
constexpr int kCovFactorLanes = 4;                           // lanes per column of the triangular inverse
static_assert(kCovMaxN * kCovFactorLanes <= kCovFactorThreads, "one quad per column");
constexpr int kCovLongTrack = restated::kStatsLongTrack;     // the lane / wave switch-over of the consumers
// scal: sum r^2 | sigma^2 | smallest relative pivot;  ints: undetermined points | the first of them | failing parameter
constexpr int kCovScal = 4, kCovInts = 4;

__host__ __device__ constexpr int cov_block_index(int a, int b, int C) { return a * C - a * (a - 1) / 2 + (b - a); }   // a <= b

// W = Jc^T Jp of one observation (as k_schur_blocks forms it) times the packed symmetric 3x3 vi: Y = W vi, 6x3
__device__ __forceinline__ void cov_obs_y(const double* __restrict__ row, double X, double Y, double Z, const double (&vi)[6],
                                          const KMat& K, double (&Yo)[6][3]) {
    double jc[12], jp[6], rx, ry;
    observe<true>(row, X, Y, Z, 0.0, 0.0, K, rx, ry, jc, jp);
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const double w0 = jc[u] * jp[0] + jc[6 + u] * jp[3], w1 = jc[u] * jp[1] + jc[6 + u] * jp[4],
                     w2 = jc[u] * jp[2] + jc[6 + u] * jp[5];
        Yo[u][0] = w0 * vi[0] + w1 * vi[1] + w2 * vi[2];
        Yo[u][1] = w0 * vi[1] + w1 * vi[3] + w2 * vi[4];
        Yo[u][2] = w0 * vi[2] + w1 * vi[4] + w2 * vi[5];
    }
}
// Z += S Yb for the 6x6 block S at `blk` of a matrix of leading dimension n
__device__ __forceinline__ void cov_block_apply(const double* __restrict__ blk, int n, const double (&Yb)[6][3], double (&Zc)[6][3]) {
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int w = 0; w < 6; ++w) {
            const double s = blk[(size_t)u * n + w];
#pragma unroll
            for (int k = 0; k < 3; ++k) Zc[u][k] = fma(s, Yb[w][k], Zc[u][k]);
        }
}
// acc += upper triangle of Ya^T Z (00 01 02 11 12 22): the sum over the observations is symmetric, so only this half is formed
__device__ __forceinline__ void cov_upper_add(const double (&Ya)[6][3], const double (&Zc)[6][3], double (&acc)[6]) {
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        acc[0] = fma(Ya[u][0], Zc[u][0], acc[0]); acc[1] = fma(Ya[u][0], Zc[u][1], acc[1]); acc[2] = fma(Ya[u][0], Zc[u][2], acc[2]);
        acc[3] = fma(Ya[u][1], Zc[u][1], acc[3]); acc[4] = fma(Ya[u][1], Zc[u][2], acc[4]); acc[5] = fma(Ya[u][2], Zc[u][2], acc[5]);
    }
}
// sqrt of the largest eigenvalue of a packed symmetric 3x3 (NaN in, NaN out)
__device__ __forceinline__ double cov_sigma3(const double (&s)[6]) {
    double a[6], v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = s[k];
    jacobi_sweeps<3>(a, v);
    const double m = fmax(a[sym<3>(0, 0)], fmax(a[sym<3>(1, 1)], a[sym<3>(2, 2)]));
    return (s[0] == s[0] && s[3] == s[3] && s[5] == s[5]) ? sqrt(m) : NAN;      // (fmax would drop a NaN)
}

// ---- 1. linearisation at x, undamped ---------------------------------------------------------------------------------------
// One lane per point over its run in stored order: sum r^2 of the run, V_p = sum Jp^T Jp, its Cholesky with the pivot
// test d_k > point_tol max diag V_p, V_p^-1 (zero when the test fails) and the point record k_schur_blocks gathers.
// pt_status: 0 fine, 1 undetermined (a pivot failed), 3 no observation.
struct CovLinOut {
    double* __restrict__ rec;          // [P][rec_stride] X Y Z 0 0 0
    double* __restrict__ Vinv;         // [P][vinv_stride] packed upper
    double* __restrict__ pt_cost;      // [P]
    int* __restrict__ pt_status;       // [P]
    int rec_stride, vinv_stride;
};
__global__ __launch_bounds__(kCovThreads) void k_cov_linearize(const int* __restrict__ pt_ptr, const int* __restrict__ cam_idx,
                                                               const double* __restrict__ uv, const double* __restrict__ camtab,
                                                               const double* __restrict__ pts, int P, KMat K, double point_tol,
                                                               CovLinOut out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int b = pt_ptr[p], e = pt_ptr[p + 1];
    const double X = pts[3 * (size_t)p], Y = pts[3 * (size_t)p + 1], Z = pts[3 * (size_t)p + 2];
    double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, cost = 0.0;
    for (int k = b; k < e; ++k) {
        const double2 px = reinterpret_cast<const double2*>(uv)[k];
        double jc[12], jp[6], rx, ry;
        observe<true>(camtab + (size_t)cam_idx[k] * kCamRow, X, Y, Z, px.x, px.y, K, rx, ry, jc, jp);
        cost += rx * rx + ry * ry;
        V[0] += jp[0] * jp[0] + jp[3] * jp[3]; V[1] += jp[0] * jp[1] + jp[3] * jp[4]; V[2] += jp[0] * jp[2] + jp[3] * jp[5];
        V[3] += jp[1] * jp[1] + jp[4] * jp[4]; V[4] += jp[1] * jp[2] + jp[4] * jp[5]; V[5] += jp[2] * jp[2] + jp[5] * jp[5];
    }
    // the pivots of chol3_inverse's factorisation (a NaN fails every test)
    const double thr = point_tol * fmax(V[0], fmax(V[3], V[5]));
    const double d0 = V[0], l10 = V[1] / sqrt(d0), l20 = V[2] / sqrt(d0);
    const double d1 = V[3] - l10 * l10, l21 = (V[4] - l20 * l10) / sqrt(d1);
    const double d2 = V[5] - l20 * l20 - l21 * l21;
    const bool ok = e > b && d0 > thr && d1 > thr && d2 > thr;
    double inv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ok) chol3_inverse(V, inv);
#pragma unroll
    for (int k = 0; k < 6; ++k) out.Vinv[(size_t)p * out.vinv_stride + k] = inv[k];
    double* __restrict__ r = out.rec + (size_t)p * out.rec_stride;
    r[0] = X; r[1] = Y; r[2] = Z; r[3] = 0.0; r[4] = 0.0; r[5] = 0.0;
    out.pt_cost[p] = cost;
    out.pt_status[p] = e == b ? 3 : (ok ? 0 : 1);
}

// One workgroup: sum r^2 over the points (a thread adds its points in ascending order, wave_sum, the waves in wave
// order), the number of undetermined points and the first of them, and sigma^2 = the caller's if > 0, else
// sum r^2 / dof, else (dof <= 0) 1.
__global__ __launch_bounds__(kCovThreads) void k_cov_reduce(const double* __restrict__ pt_cost, const int* __restrict__ pt_status,
                                                            int P, double sigma2_opt, double dof, double* __restrict__ scal,
                                                            int* __restrict__ ints) {
    __shared__ double red[kCovThreads / 64];
    __shared__ int redi[2 * (kCovThreads / 64)];
    double s = 0.0;
    int nbad = 0, first = P;
    for (int p = threadIdx.x; p < P; p += kCovThreads) {
        s += pt_cost[p];
        if (pt_status[p] == 1) { ++nbad; first = min(first, p); }
    }
    s = wave_sum(s);
    nbad = wave_reduce_xor(nbad, [](int a, int b) { return a + b; });
    first = wave_reduce_xor(first, [](int a, int b) { return min(a, b); });
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; redi[2 * (threadIdx.x >> 6)] = nbad; redi[2 * (threadIdx.x >> 6) + 1] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        int nb = 0, f = P;
        for (int w = 0; w < kCovThreads / 64; ++w) { t += red[w]; nb += redi[2 * w]; f = min(f, redi[2 * w + 1]); }
        scal[0] = t;
        scal[1] = sigma2_opt > 0.0 ? sigma2_opt : (dof > 0.0 ? t / dof : 1.0);
        ints[0] = nb;
        ints[1] = nb ? f : -1;
    }
}

// U_c = sum Jc^T Jc over ALL observations of camera c (the camera-major permutation of the statistics call; the pixel
// does not enter the Jacobian), packed upper 21 as in Ugc.  One workgroup per camera: lanes, then the waves in wave order.
__global__ __launch_bounds__(kCamThreads) void k_cov_cam_u(const int* __restrict__ cam_ptr, const int* __restrict__ perm,
                                                           const int* __restrict__ pt_idx, const double* __restrict__ camtab,
                                                           const double* __restrict__ pts, KMat K, double* __restrict__ U) {
    __shared__ double red[kCamWaves * 21];
    const int c = blockIdx.x;
    double t[kCamTab];
#pragma unroll
    for (int k = 0; k < kCamTab; ++k) t[k] = camtab[(size_t)c * kCamRow + k];
    double a[21];
#pragma unroll
    for (int q = 0; q < 21; ++q) a[q] = 0.0;
    for (int k = cam_ptr[c] + (int)threadIdx.x; k < cam_ptr[c + 1]; k += kCamThreads) {
        const double* __restrict__ Xp = pts + 3 * (size_t)pt_idx[perm[k]];
        double jc[12], jp[6], rx, ry;
        observe<true>(t, Xp[0], Xp[1], Xp[2], 0.0, 0.0, K, rx, ry, jc, jp);
#pragma unroll
        for (int u = 0; u < 6; ++u)
#pragma unroll
            for (int v = u; v < 6; ++v) a[sym<6>(u, v)] += jc[u] * jc[v] + jc[6 + u] * jc[6 + v];
    }
    block_sum<21>(a, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 21; ++q) U[(size_t)c * 21 + q] = a[q];
    }
}

// ---- 2. factorisation and inverse of S ---------------------------------------------------------------------------------
// One workgroup, S = U - W V^-1 W^T assembled in LDS as k_dense_pcg does it (n x (n | 1) doubles; diagonal blocks from
// their half u <= v), rows and columns of held parameters replaced by identity.  Right-looking Cholesky on the lower
// triangle with the relative pivot test d_k > rank_tol S_kk (a failure ends the kernel: ints[2] = k); L^-1 in place row by
// row (row i of L is set aside, then a quad per column j forms -(1 / L_ii) sum_k L_ik M_kj from the rows already done);
// Sigma = L^-T L^-1 into the unused strict upper triangle and a diagonal of its own, so no second matrix is needed.
// Written to `full` (n x n, symmetric by mirroring) scaled by sigma^2, held rows and columns zero, those of cameras
// nobody observes NaN.  scal[2] = smallest d_k / S_kk.
__global__ __launch_bounds__(kCovFactorThreads) void k_cov_factor(const double* __restrict__ Sblk, const double* __restrict__ U,
                                                                  const unsigned char* __restrict__ held, int C, double rank_tol,
                                                                  double* __restrict__ scal, int* __restrict__ ints,
                                                                  double* __restrict__ full) {
    extern __shared__ __align__(16) double A[];
    const int n = 6 * C, ld = n | 1, tid = threadIdx.x;
    double* const d0 = A + (size_t)n * ld;      // S_kk | row i of L | diagonal of Sigma
    double* const rowb = d0 + kCovMaxN;
    double* const dg = rowb + kCovMaxN;
    auto at = [&](int r, int c) -> double& { return A[(size_t)r * ld + c]; };
    for (int e = tid; e < n * n; e += kCovFactorThreads) {
        const int r = e / n, c = e - r * n;
        double val = r == c ? 1.0 : 0.0;
        if (!held[r] && !held[c]) {
            const int a = r / 6, u = r - 6 * a, b = c / 6, v = c - 6 * b;
            int lo = a, hi = b, uu = u, vv = v;
            if (a > b) { lo = b; hi = a; uu = v; vv = u; }
            if (a == b && u > v) { uu = v; vv = u; }
            val = -Sblk[(size_t)cov_block_index(lo, hi, C) * 36 + 6 * uu + vv];
            if (a == b) val += U[(size_t)a * 21 + sym<6>(uu, vv)];
        }
        at(r, c) = val;
    }
    __syncthreads();
    if (tid < n) d0[tid] = at(tid, tid);
    __syncthreads();
    double minrel = INFINITY;
    int bad = -1;
    for (int k = 0; k < n; ++k) {
        const double d = at(k, k), s = d0[k];                      // the same words on every thread: a uniform verdict
        if (!(d > rank_tol * s)) { bad = k; break; }
        minrel = fmin(minrel, d / s);                              // (a held parameter: 1; a pivot never exceeds S_kk)
        const double l = sqrt(d), il = 1.0 / l;
        __syncthreads();
        for (int i = k + tid; i < n; i += kCovFactorThreads) at(i, k) = i == k ? l : at(i, k) * il;
        __syncthreads();
        const int m = n - k - 1;
        for (int e = tid; e < m * m; e += kCovFactorThreads) {
            const int i = k + 1 + e / m, j = k + 1 + (e - (e / m) * m);
            if (j <= i) at(i, j) = fma(-at(i, k), at(j, k), at(i, j));
        }
        __syncthreads();
    }
    if (bad >= 0) {
        if (tid == 0) { scal[2] = minrel; ints[2] = bad; }
        return;
    }
    {   // M = L^-1, row by row
        const int j = tid / kCovFactorLanes, sub = tid & (kCovFactorLanes - 1);
        for (int i = 0; i < n; ++i) {
            if (tid <= i) rowb[tid] = at(i, tid);
            __syncthreads();
            const double il = 1.0 / rowb[i];
            double t = 0.0;
            if (j < i)
                for (int k = j + sub; k < i; k += kCovFactorLanes) t = fma(rowb[k], at(k, j), t);
            t = quad_sum(t);
            if (sub == 0) {
                if (j < i) at(i, j) = -t * il;
                else if (j == i) at(i, i) = il;
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < n * n; e += kCovFactorThreads) {         // Sigma_ij = sum_{k >= j} M_ki M_kj, i <= j
        const int i = e / n, j = e - i * n;
        if (j < i) continue;
        double t = 0.0;
        for (int k = j; k < n; ++k) t = fma(at(k, i), at(k, j), t);
        if (i == j) dg[i] = t; else at(i, j) = t;
    }
    __syncthreads();
    const double sigma2 = scal[1];
    for (int e = tid; e < n * n; e += kCovFactorThreads) {
        const int r = e / n, c = e - r * n;
        double val = r == c ? dg[r] : at(min(r, c), max(r, c));
        const unsigned char hr = held[r], hc = held[c];
        val = (hr == 2 || hc == 2) ? NAN : ((hr || hc) ? 0.0 : sigma2 * val);
        full[e] = val;
    }
    if (tid == 0) { scal[2] = minrel; ints[2] = -1; }
}

// ---- 3. the point blocks -------------------------------------------------------------------------------------------------
// Sigma_pp = sigma^2 V_p^-1 + sum_a Y_a^T Z_a,  Y_a = W_a V_p^-1,  Z_a = sum_b Sigma_cc[a, b] Y_b over the observations b
// of the point in stored order (a camera that sees the point twice contributes twice); kind = 1: the first term alone.
// A lane takes a run shorter than kCovLongTrack and recomputes Y_b inside its double loop (nothing of a run is kept
// but Y_a, Z_a and the six sums); the wave takes the longer runs afterwards (for_each_long_run): every lane holds Y_a of one
// observation of a block of 64 and meets the Y_b of every block, handed round with v_readlane in stored order; the lanes'
// sums are added by wave_sum.  Sigma_cc (already scaled by sigma^2; 127 KB at 21 cameras) is staged in LDS by every
// workgroup first (LDS; the form that runs: 10-12 % faster for the whole call) or read from global
// memory, where it is resident in L2 ("cov_lds" = 0).
// pt_sigma = sqrt of the largest eigenvalue (3x3 Jacobi in registers).
struct CovPointOut { double* __restrict__ cov; double* __restrict__ sigma; };
template <bool LDS>
__global__ __launch_bounds__(kCovThreads) void k_cov_points(const int* __restrict__ pt_ptr, const int* __restrict__ cam_idx,
                                                            const double* __restrict__ camtab, const double* __restrict__ pts,
                                                            const double* __restrict__ Vinv, int vinv_stride,
                                                            const int* __restrict__ pt_status, const double* __restrict__ full_g,
                                                            int n, const double* __restrict__ scal, int kind, int P, KMat K,
                                                            CovPointOut out) {
    extern __shared__ __align__(16) double smem[];
    if (LDS) stage_table(full_g, n * n, smem);                   // (n = 6 C is even; ends with a barrier)
    const double* __restrict__ full = LDS ? smem : full_g;
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    int b = 0, e = 0, st = 3;
    double X = 0.0, Y = 0.0, Z = 0.0;
    double vi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < P) {
        b = pt_ptr[p]; e = pt_ptr[p + 1]; st = pt_status[p];
        X = pts[3 * (size_t)p]; Y = pts[3 * (size_t)p + 1]; Z = pts[3 * (size_t)p + 2];
#pragma unroll
        for (int k = 0; k < 6; ++k) vi[k] = Vinv[(size_t)p * vinv_stride + k];
    }
    const bool work = p < P && st == 0 && kind == 0;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (work && e - b < kCovLongTrack) {
        for (int ka = b; ka < e; ++ka) {
            const int ca = cam_idx[ka];
            double Ya[6][3], Zc[6][3];
            cov_obs_y(camtab + (size_t)ca * kCamRow, X, Y, Z, vi, K, Ya);
#pragma unroll
            for (int u = 0; u < 6; ++u) { Zc[u][0] = 0.0; Zc[u][1] = 0.0; Zc[u][2] = 0.0; }
            for (int kb = b; kb < e; ++kb) {
                const int cb = cam_idx[kb];
                double Yb[6][3];
                cov_obs_y(camtab + (size_t)cb * kCamRow, X, Y, Z, vi, K, Yb);
                cov_block_apply(full + (size_t)(6 * ca) * n + 6 * cb, n, Yb, Zc);
            }
            cov_upper_add(Ya, Zc, acc);
        }
    }
    for_each_long_run(work && e - b >= kCovLongTrack, b, e, X, Y, Z, [&](int q, int qb_, int qe_, double qX, double qY, double qZ) {
        const int qb = __builtin_amdgcn_readfirstlane(qb_), qe = __builtin_amdgcn_readfirstlane(qe_);     // scalar loop bounds
        double qv[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) qv[k] = __shfl(vi[k], q);
        double wacc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int B0 = qb; B0 < qe; B0 += 64) {
            const int ka = B0 + lane;
            const bool on = ka < qe;
            const int ca = on ? cam_idx[ka] : 0;
            double Ya[6][3], Zc[6][3];
            cov_obs_y(camtab + (size_t)ca * kCamRow, qX, qY, qZ, qv, K, Ya);
#pragma unroll
            for (int u = 0; u < 6; ++u) { Zc[u][0] = 0.0; Zc[u][1] = 0.0; Zc[u][2] = 0.0; }
            for (int A0 = qb; A0 < qe; A0 += 64) {
                const int kb = A0 + lane;
                const int cb = kb < qe ? cam_idx[kb] : 0;
                double Yb[6][3];
                cov_obs_y(camtab + (size_t)cb * kCamRow, qX, qY, qZ, qv, K, Yb);
                const int cnt = min(64, qe - A0);
                for (int l = 0; l < cnt; ++l) {                      // stored order; l is uniform: v_readlane
                    const int cl = __builtin_amdgcn_readlane(cb, l);
                    double Yl[6][3];
#pragma unroll
                    for (int u = 0; u < 6; ++u)
#pragma unroll
                        for (int k = 0; k < 3; ++k) Yl[u][k] = readlane_double(Yb[u][k], l);
                    if (on) cov_block_apply(full + (size_t)(6 * ca) * n + 6 * cl, n, Yl, Zc);
                }
            }
            if (on) cov_upper_add(Ya, Zc, wacc);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double t = wave_sum(wacc[k]);
            if (lane == q) acc[k] = t;
        }
    });
    if (p >= P) return;
    const double sigma2 = scal[1];
    double s6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) s6[k] = st == 0 ? fma(sigma2, vi[k], acc[k]) : NAN;
    double* __restrict__ o = out.cov + 9 * (size_t)p;
    o[0] = s6[0]; o[1] = s6[1]; o[2] = s6[2];
    o[3] = s6[1]; o[4] = s6[3]; o[5] = s6[4];
    o[6] = s6[2]; o[7] = s6[4]; o[8] = s6[5];
    out.sigma[p] = cov_sigma3(s6);
}

// ---- 4. per camera ---------------------------------------------------------------------------------------------------------
// One lane per camera.  kind = 0: the 6x6 diagonal block of Sigma_cc as it stands in `full`.  kind = 1: sigma^2 times the
// inverse of U_c restricted to the camera's free parameters (held ones replaced by identity, then zeroed), by the 6x6
// Cholesky of spd6_inverse with the pivot test of k_cov_factor; piv[c] = smallest relative pivot | failing parameter or -1.
// A camera nobody observes (held = 2) reports NaN.  cam_sigma = sqrt of the largest eigenvalue of the w and of the T block.
__global__ __launch_bounds__(kCovThreads) void k_cov_cams(const double* __restrict__ full, const double* __restrict__ U,
                                                          const unsigned char* __restrict__ held, int C, int kind,
                                                          double rank_tol, const double* __restrict__ scal,
                                                          double* __restrict__ cam_cov, double* __restrict__ cam_sigma,
                                                          double* __restrict__ piv) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int n = 6 * C;
    double S[6][6];
    if (kind == 0) {
#pragma unroll
        for (int u = 0; u < 6; ++u)
#pragma unroll
            for (int v = 0; v < 6; ++v) S[u][v] = full[(size_t)(6 * c + u) * n + 6 * c + v];
    } else {
        bool hd[6];
        bool none = false;
#pragma unroll
        for (int u = 0; u < 6; ++u) { const unsigned char hv = held[6 * c + u]; hd[u] = hv != 0; none = none || hv == 2; }
        double B[6][6];
#pragma unroll
        for (int u = 0; u < 6; ++u)
#pragma unroll
            for (int v = 0; v < 6; ++v) B[u][v] = (hd[u] || hd[v]) ? (u == v ? 1.0 : 0.0) : U[(size_t)c * 21 + sym<6>(u, v)];
        double Lm[6][6], minrel = INFINITY;
        int bad = -1;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double sj = B[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) sj -= Lm[j][k] * Lm[j][k];
            if (!(sj > rank_tol * B[j][j]) && bad < 0) bad = 6 * c + j;
            minrel = fmin(minrel, sj / B[j][j]);
            const double ljj = sqrt(sj);
            Lm[j][j] = ljj;
            const double inv = 1.0 / ljj;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double t = B[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) t -= Lm[i][k] * Lm[j][k];
                Lm[i][j] = t * inv;
            }
        }
        double M[6][6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            M[j][j] = 1.0 / Lm[j][j];
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double t = 0.0;
#pragma unroll
                for (int k = j; k < i; ++k) t -= Lm[i][k] * M[k][j];
                M[i][j] = t / Lm[i][i];
            }
        }
        const double sigma2 = scal[1];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) {
                double t = 0.0;
#pragma unroll
                for (int k = b; k < 6; ++k) t += M[k][a] * M[k][b];
                t = (none || bad >= 0) ? NAN : ((hd[a] || hd[b]) ? 0.0 : sigma2 * t);
                S[a][b] = t; S[b][a] = t;
            }
        if (none) { bad = -1; minrel = INFINITY; }
        piv[2 * (size_t)c] = minrel;
        piv[2 * (size_t)c + 1] = (double)bad;
    }
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = 0; v < 6; ++v) cam_cov[(size_t)c * 36 + 6 * u + v] = S[u][v];
    const double sw[6] = {S[0][0], S[0][1], S[0][2], S[1][1], S[1][2], S[2][2]};
    const double sT[6] = {S[3][3], S[3][4], S[3][5], S[4][4], S[4][5], S[5][5]};
    cam_sigma[2 * (size_t)c] = cov_sigma3(sw);
    cam_sigma[2 * (size_t)c + 1] = cov_sigma3(sT);
}

}  // namespace sfmba
