// ba_device.hpp -- the device-side pieces the solver's kernels (ba_kernels.hpp) share with the consumers' kernels
// (consumer_kernels.hpp), and the types and constants of theirs that the handle (handle.hpp) holds: the camera-table
// layout, wave and block reductions, `observe`, the row-slab helpers, the small dense inverses.  No kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sfmba {

constexpr int kCamTab = 17;          // entries of a camera-table row: R (9) T (3) w (3) b c
constexpr int kCamRow = 18;          // ... and its stride: rows are 16-byte aligned (nine 16-byte loads per row)
constexpr int kSweepThreads = 1024;  // one workgroup per CU, 16 waves sharing one LDS camera table
constexpr int kWavesPerSweepBlock = kSweepThreads / 64;
struct KMat { double k[9]; };
struct Origin { double x, y, z; };   // of the fp32 operands (MixedPrep)
constexpr int kP2pMaxRanks = 16;    // of the direct all-reduce (P2pArgs)
// two constants of the dense path for the units that do not include ba_kernels.hpp (covariance.hip); they stay defined
// there, where the tests read them, and ba_kernels.hpp holds the pairs together
namespace restated { constexpr int kDenseMaxN = 128; constexpr int kDenseThreads = 512; }

// Cross-lane moves that stay in the VALU (DPP row shifts, v_readlane) instead of going through the LDS pipe
// as ds_bpermute does; row_shl:N makes lane i read lane i+N of its 16-lane row (0 when that leaves the row).
template <int CTRL>
__device__ __forceinline__ int dpp_int(int x) {        // source lane out of the row: 0
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double dpp_double(double x) {
    const int lo = dpp_int<CTRL>(__double2loint(x)), hi = dpp_int<CTRL>(__double2hiint(x));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_double(double x, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
    return __hiloint2double(hi, lo);
}

// Sum over the wave, result on every lane: suffix sums inside the four rows, then the four row totals.
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_double<0x101>(v);
    v += dpp_double<0x102>(v);
    v += dpp_double<0x104>(v);
    v += dpp_double<0x108>(v);
    return ((readlane_double(v, 0) + readlane_double(v, 16)) + readlane_double(v, 32)) + readlane_double(v, 48);
}
__device__ __forceinline__ double quad_sum(double v) {        // sum over the four lanes of a quad, on every lane
    v += dpp_double<0xB1>(v);                                  // quad_perm [1,0,3,2]
    v += dpp_double<0x4E>(v);                                  // quad_perm [2,3,0,1]
    return v;
}
// The xor butterfly over the wave with any commutative operator: the same bits on every lane.  (A sum by it adds in
// another order than wave_sum.)
template <class T, class Op>
__device__ __forceinline__ T wave_reduce_xor(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) { return wave_reduce_xor(v, [](double a, double b) { return fmax(a, b); }); }

// Block-wide sum of NQ values per thread; result valid on thread 0.  `red` holds >= 16*NQ doubles.
template <int NQ>
__device__ __forceinline__ void block_sum(double (&v)[NQ], double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = wave_sum(v[q]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) red[w * NQ + q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double s = 0.0;
            for (int k = 0; k < nw; ++k) s += red[k * NQ + q];   // fixed order
            v[q] = s;
        }
    }
}

// Block-wide sum of one value per thread, result on EVERY thread, one barrier: each wave leaves its sum in
// `slots` (an array no other reduction of the kernel uses, so nothing has to be fenced before the write) and
// every thread adds the slots in the same fixed order.
__device__ __forceinline__ double block_sum_all(double v, double* slots) {
    const int nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < nw; ++k) s += slots[k];
    return s;
}

// element i of an array of pairs stored as double2 (f32 = 0) or float2 (f32 = 1)
__device__ __forceinline__ double2 load_pair(const double* __restrict__ base, int f32, int i) {
    if (f32) {
        const float2 v = reinterpret_cast<const float2*>(base)[i];
        return make_double2((double)v.x, (double)v.y);
    }
    return reinterpret_cast<const double2*>(base)[i];
}
__device__ __forceinline__ void store_pair(double* __restrict__ base, int f32, int i, double a, double b) {
    if (f32) reinterpret_cast<float2*>(base)[i] = make_float2((float)a, (float)b);
    else reinterpret_cast<double2*>(base)[i] = make_double2(a, b);
}

// The table buffer holds three views of the same data: rows [C][17] (K1, K2, the camera-major passes), the
// compact [C][12] = R | T that the recomputing Schur pass stages in LDS, and w, b, c plane-major [5][C] for its
// one-thread-per-camera prologue.  Between the last two a fourth, compact [C][12] = M | T with M = K R (the intrinsics
// carried through the rotation once per camera; 16-byte aligned for every C): what the fp64 row-form kernels stage
// instead of R | T, since the projection and the rows of d r/d X need R only as K R:
//     p = M v,   j_k = (M_k - (p_k / p_z) M_3) / p_z.
constexpr int kCamRT = 12, kCamWbc = 5;
__host__ __device__ constexpr size_t cam_rt_offset(int C) { return (size_t)C * kCamRow; }
__host__ __device__ constexpr size_t cam_mt_offset(int C) { return cam_rt_offset(C) + (size_t)C * kCamRT; }
__host__ __device__ constexpr size_t cam_wbc_offset(int C) { return cam_mt_offset(C) + (size_t)C * kCamRT; }
__host__ __device__ constexpr size_t cam_table_doubles(int C) { return cam_wbc_offset(C) + (size_t)C * kCamWbc; }
// the 17 entries of one camera's row: R (9), T (3), w (3), b, c  (t may be global or LDS)
__device__ __forceinline__ void cam_row_values(const double* __restrict__ prm, double* __restrict__ t) {
    const double wx = prm[0], wy = prm[1], wz = prm[2];
    const double th2 = wx * wx + wy * wy + wz * wz;
    const double th = sqrt(th2);
    double a, b, cc;
    if (th < 1e-4) {
        a = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
        b = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
    } else {
        a = sin(th) / th;
        const double h = 0.5 * th;
        const double s = sin(h) / h;
        b = 0.5 * s * s;                       // (1 - cos t)/t^2 without cancellation
    }
    if (th < 0.3) {
        cc = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0 - th2 * th2 * th2 / 362880.0 +
             th2 * th2 * th2 * th2 / 39916800.0 - th2 * th2 * th2 * th2 * th2 / 6227020800.0;
    } else {
        cc = (th - sin(th)) / (th2 * th);
    }
    t[0] = 1.0 + b * (wx * wx - th2); t[1] = -a * wz + b * wx * wy;     t[2] = a * wy + b * wx * wz;
    t[3] = a * wz + b * wx * wy;      t[4] = 1.0 + b * (wy * wy - th2); t[5] = -a * wx + b * wy * wz;
    t[6] = -a * wy + b * wx * wz;     t[7] = a * wx + b * wy * wz;      t[8] = 1.0 + b * (wz * wz - th2);
    t[9] = prm[3]; t[10] = prm[4]; t[11] = prm[5];
    t[12] = wx; t[13] = wy; t[14] = wz;
    t[15] = b; t[16] = cc;
}

// One observation: residual and (JAC) the 2x6 / 2x3 blocks.
//   v = X - T, q = R v, p = K q, A = dpi/dp K;  dr/dX = A R;  dr/dT = -A R;
//   row k of dr/dw = -(m - b (m x w) + c ((m x w) x w)),  m = (row k of A R) x v.
template <bool JAC>
__device__ __forceinline__ void observe(const double* __restrict__ t, double X, double Y, double Z,
                                        double u, double v, const KMat& K, double& rx, double& ry,
                                        double* __restrict__ jc, double* __restrict__ jp) {
    const double vx = X - t[9], vy = Y - t[10], vz = Z - t[11];
    const double qx = t[0] * vx + t[1] * vy + t[2] * vz;
    const double qy = t[3] * vx + t[4] * vy + t[5] * vz;
    const double qz = t[6] * vx + t[7] * vy + t[8] * vz;
    const double px = K.k[0] * qx + K.k[1] * qy + K.k[2] * qz;
    const double py = K.k[3] * qx + K.k[4] * qy + K.k[5] * qz;
    const double pz = K.k[6] * qx + K.k[7] * qy + K.k[8] * qz;
    const double iz = 1.0 / pz;
    const double u0 = px * iz, u1 = py * iz;
    rx = u0 - u;
    ry = u1 - v;
    if (JAC) {
        const double wx = t[12], wy = t[13], wz = t[14], b = t[15], c = t[16];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double pk = k == 0 ? u0 : u1;
            const double a0 = (K.k[3 * k + 0] - pk * K.k[6]) * iz;
            const double a1 = (K.k[3 * k + 1] - pk * K.k[7]) * iz;
            const double a2 = (K.k[3 * k + 2] - pk * K.k[8]) * iz;
            const double j0 = a0 * t[0] + a1 * t[3] + a2 * t[6];      // row k of A R
            const double j1 = a0 * t[1] + a1 * t[4] + a2 * t[7];
            const double j2 = a0 * t[2] + a1 * t[5] + a2 * t[8];
            jp[3 * k + 0] = j0; jp[3 * k + 1] = j1; jp[3 * k + 2] = j2;
            const double m0 = j1 * vz - j2 * vy, m1 = j2 * vx - j0 * vz, m2 = j0 * vy - j1 * vx;
            const double s0 = m1 * wz - m2 * wy, s1 = m2 * wx - m0 * wz, s2 = m0 * wy - m1 * wx;
            const double t0 = s1 * wz - s2 * wy, t1 = s2 * wx - s0 * wz, t2 = s0 * wy - s1 * wx;
            jc[6 * k + 0] = -(m0 - b * s0 + c * t0);
            jc[6 * k + 1] = -(m1 - b * s1 + c * t1);
            jc[6 * k + 2] = -(m2 - b * s2 + c * t2);
            jc[6 * k + 3] = -j0; jc[6 * k + 4] = -j1; jc[6 * k + 5] = -j2;
        }
    }
}

// 16-byte streaming store of two doubles (one global_store_dwordx4)
__device__ __forceinline__ void st16(double* __restrict__ p, double a, double b) {
    *reinterpret_cast<double2*>(p) = make_double2(a, b);
}

// Camera rows of one 64-observation tile gathered THROUGH the LDS (more cameras than the LDS holds a table of, BASELINE
// config 5): the wave requests the 64 rows its lanes need -- 64 x 144 B = nine 1-KiB pieces -- with LDS-DMA loads whose
// per-lane SOURCE address walks the rows piece by piece (lane l of piece k fetches 16-byte piece (64 k + l) mod 9 of the
// row of lane (64 k + l) / 9), so that one wave instruction touches the ~8 rows of 7-8 lanes contiguously instead of 64
// rows at a stride (nine lane-divergent 16-byte loads per observation kept the texture addresser busy for 387 us of
// K1 at 10M observations: 0.26 of the HBM roofline).  The rows land in lane order in the wave's private 9 KiB slab and
// every lane reads its own row back with nine ds_read_b128 (rows at a stride of 36 dwords: conflict-free).  No
// registers are held while the pieces fly; the request for tile i + 1 is issued as soon as tile i's rows have been read
// out of the slab.
constexpr int kRowPieces = kCamRow / 2;                       // 16-byte pieces per row
constexpr size_t kRowSlabDoubles = 64 * (size_t)kCamRow;      // per wave
// (Tried and dropped, A/B on one box: the pieces issued from inline assembly with counted waits, so that the stores of a
// tile need not be acknowledged before the next request -- while a builtin LDS-DMA load is in flight hipcc waits vmcnt(0)
// at the next use of any loaded register -- and every load of k_resjac's loop issued from inline assembly with one
// counted wait per tile.  Same durations to within 2 %: these sweeps are not waiting on their own stores.)
__device__ __forceinline__ void rows_request(const double* __restrict__ table, int cam, int lane, double* slab) {
#pragma unroll
    for (int k = 0; k < kRowPieces; ++k) {
        const int q = k * 64 + lane;
        const int row = q / kRowPieces, piece = q - kRowPieces * row;
        const int cr = __shfl(cam, row);
        __builtin_amdgcn_global_load_lds(table + (size_t)cr * kCamRow + 2 * piece,
                                         (__attribute__((address_space(3))) void*)(slab + 2 * 64 * k), 16, 0, 0);
        __builtin_amdgcn_sched_barrier(0);       // piece by piece: nine address computations in flight together spill
    }
}
// the pieces have landed (every earlier vector-memory operation of the wave has completed) ...
__device__ __forceinline__ void rows_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// ... and, before the slab is requested again, the reads of it have returned
__device__ __forceinline__ void rows_read_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Mailbox: the hand-off of an outer iteration.  One wave copies the 32 exchange scalars and the PCG
// control block into coherent host memory and raises a sequence number behind them; the host polls
// that word instead of waiting on an event behind two blit copies.  mbox = [0..31] scalars,
// [32..] control block, [63] sequence number.
constexpr int kMboxCtrl = 32, kMboxErr = 62, kMboxSeq = 63;
struct PcgCtrl;                           // (ba_kernels.hpp)
struct Mailbox {
    double* __restrict__ host;            // device-visible address of the pinned block; null: no post
    const double* __restrict__ sc;
    const PcgCtrl* __restrict__ ctrl;
    unsigned long long seq;
    const unsigned* __restrict__ err;     // error word of the direct all-reduce (null: none): travels with every post,
};                                        // so that a collective that timed out aborts the solve at the next hand-off

constexpr int kCamThreads = 256;
constexpr int kCamWaves = kCamThreads / 64;
constexpr int kCamUnroll = 4;
constexpr int kSortSlices = 512;     // slices of the counting sort by camera (k_cam_hist)

// n doubles (n even, both ends 16-byte aligned) into LDS by the whole workgroup, 16 bytes per lane; ends with a barrier
__device__ __forceinline__ void stage_table(const double* __restrict__ tab, int n, double* __restrict__ smem) {
    const int n2 = n >> 1;
    const double2* __restrict__ src = reinterpret_cast<const double2*>(tab);
    double2* __restrict__ dst = reinterpret_cast<double2*>(smem);
    for (int k = threadIdx.x; k < n2; k += blockDim.x) dst[k] = src[k];
    __syncthreads();
}
__device__ __forceinline__ void stage_cam_table(const double* __restrict__ camtab, int C, double* __restrict__ smem) {
    stage_table(camtab, C * kCamRow, smem);
}

__device__ __forceinline__ void chol3_inverse(const double* a /*upper 6*/, double* inv /*upper 6*/) {
    // A = L L^T, inv = L^-T L^-1
    const double l00 = sqrt(a[0]);
    const double l10 = a[1] / l00, l20 = a[2] / l00;
    const double l11 = sqrt(a[3] - l10 * l10);
    const double l21 = (a[4] - l20 * l10) / l11;
    const double l22 = sqrt(a[5] - l20 * l20 - l21 * l21);
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;      // M = L^-1 (lower)
    const double m10 = -l10 * m00 * m11;
    const double m21 = -l21 * m11 * m22;
    const double m20 = -(l20 * m00 + l21 * m10) * m22;
    inv[0] = m00 * m00 + m10 * m10 + m20 * m20;
    inv[1] = m10 * m11 + m20 * m21;
    inv[2] = m20 * m22;
    inv[3] = m11 * m11 + m21 * m21;
    inv[4] = m21 * m22;
    inv[5] = m22 * m22;
}

// out = packed upper triangle of A^-1 for a symmetric positive definite 6x6 A (Cholesky, inverse of the factor)
__device__ __forceinline__ void spd6_inverse(const double (&A)[6][6], double (&out)[21]) {
    double Lm[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double sj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) sj -= Lm[j][k] * Lm[j][k];
        const double ljj = sqrt(sj);
        Lm[j][j] = ljj;
        const double inv = 1.0 / ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= Lm[i][k] * Lm[j][k];
            Lm[i][j] = t * inv;
        }
    }
    double M[6][6];                         // M = L^-1 (lower triangular)
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
    int n = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double t = 0.0;
#pragma unroll
            for (int k = b; k < 6; ++k) t += M[k][a] * M[k][b];
            out[n++] = t;
        }
}

}  // namespace sfmba
