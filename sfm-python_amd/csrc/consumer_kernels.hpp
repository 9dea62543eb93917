// The consumers of a solved scene: reprojection statistics, triangulation, resection (DESIGN.md sections 13, 15, 16).
// None touches a buffer of the solver's.  What they share comes first: every helper is inlined
// and keeps no state, so a call site compiles to what was written out there before.
#pragma once
#include "ba_device.hpp"
#include "consumer_device.hpp"   // for_each_long_run, the register Jacobi: shared with cov_kernels.hpp
#include "tri_pairs.hpp"         // the pair numbering of k_tri_ransac, host and device

// The workgroup scan of the feature tracks (track_scan.hpp), for k_tri_ransac.  Its three sizes as track_kernels.hpp
// defines them (plan_kernels.hpp restates them likewise); only track_block_scan is used here, no launch of the scan.
constexpr int kTrackBlock = 256;
constexpr int kTrackScanPerThread = 4;
constexpr int kTrackScanItems = 1024;
static_assert(kTrackScanItems == kTrackBlock * kTrackScanPerThread, "a thread scans kTrackScanPerThread consecutive entries");
#include "track_scan.hpp"

namespace sfmba {

// the xor butterfly (wave_reduce_xor, beside wave_max): same bits on every lane
__device__ __forceinline__ int wave_isum(int v) { return wave_reduce_xor(v, [](int a, int b) { return a + b; }); }
__device__ __forceinline__ double wave_min(double v) { return wave_reduce_xor(v, [](double a, double b) { return fmin(a, b); }); }
__device__ __forceinline__ double wave_butterfly_sum(double v) { return wave_reduce_xor(v, [](double a, double b) { return a + b; }); }

// depth of (X, Y, Z) in the camera of table row tl: the third row of R times (X - T)
__device__ __forceinline__ double cam_depth(const double* tl, double X, double Y, double Z) {
    return tl[6] * (X - tl[9]) + tl[7] * (Y - tl[10]) + tl[8] * (Z - tl[11]);
}
// (The 16-byte loads of a table row into registers are NOT shared: through a helper the compiler schedules and contracts
// the arithmetic behind them differently -- k_resect's last bits changed, k_obs_stats' slab form lost 5 % -- so
// k_obs_stats, tri_load_row and k_resect write them out.  k_obs_stats also keeps its own staging loop: with stage_table
// its instructions are the same but for register numbers, and two of four timing windows fell 1-2 % outside the parent's.)

// where the lane / wave split of a point-major sweep switches over (for_each_long_run, consumer_device.hpp)
constexpr int kStatsLongTrack = 32;
static_assert(restated::kStatsLongTrack == kStatsLongTrack, "consumer_device.hpp restates it for cov_kernels.hpp");

// The widest angle between the rays X - T of the used observations of a run, tracked as the pair (|a x b|, a . b) and
// compared by the sign of sin(theta1 - theta2) = s1 d2 - d1 s2 (both angles in [0, pi]); atan2 once per run (per lane in
// the wave form).  The order of the comparisons decides which of two equal angles' pairs is kept, hence the result's
// bits.  used(k): observation k counts; centre(k): the three doubles of its camera centre.
__device__ __forceinline__ void widest_pair(double ax, double ay, double az, double bx, double by, double bz,
                                            double& sb, double& db) {
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double s = sqrt(cx * cx + cy * cy + cz * cz), d = ax * bx + ay * by + az * bz;
    if (s * db - d * sb > 0.0) { sb = s; db = d; }
}
// all pairs by one lane: two dependent gathers and ~30 flops per pair, n (n - 1) / 2 times
template <class Used, class Centre>
__device__ __forceinline__ double widest_angle_lane(int b, int e, double X, double Y, double Z, Used used, Centre centre) {
    double sb = 0.0, db = 1.0;
    for (int i = b; i + 1 < e; ++i) {
        if (!used(i)) continue;
        const double* __restrict__ Ta = centre(i);
        const double ax = X - Ta[0], ay = Y - Ta[1], az = Z - Ta[2];
        for (int k = i + 1; k < e; ++k) {
            if (!used(k)) continue;
            const double* __restrict__ Tb = centre(k);
            widest_pair(ax, ay, az, X - Tb[0], Y - Tb[1], Z - Tb[2], sb, db);
        }
    }
    return atan2(sb, db);
}
// by the wave: the run is cut into blocks of 64 observations, every lane holds the ray of one observation of block B and
// meets the rays of every block A <= B, handed round with v_readlane -- n^2 / 64 steps per lane instead of n^2 / 2.
// block(k, on, used): called once per block B with this lane's observation k of it (on: k < e), for a caller that has
// sums of its own over the run and wants the observation's loads issued once.  Same result on every lane.
template <class Used, class Centre, class Block>
__device__ __forceinline__ double widest_angle_wave(int b, int e, int lane, double X, double Y, double Z, Used used,
                                                    Centre centre, Block block) {
    double sb = 0.0, db = 1.0;
    for (int B0 = b; B0 < e; B0 += 64) {
        const int kb = B0 + lane;
        bool fb = false;
        double bx = 0.0, by = 0.0, bz = 0.0;
        if (kb < e) {
            fb = used(kb);
            const double* __restrict__ T = centre(kb);
            bx = X - T[0]; by = Y - T[1]; bz = Z - T[2];
        }
        block(kb, kb < e, fb);
        for (int A0 = b; A0 <= B0; A0 += 64) {
            double ax = bx, ay = by, az = bz;
            bool fa = fb;
            if (A0 != B0) {                                      // a full block: A0 + 63 < B0 <= e - 1
                const int ka = A0 + lane;
                fa = used(ka);
                const double* __restrict__ T = centre(ka);
                ax = X - T[0]; ay = Y - T[1]; az = Z - T[2];
            }
            for (unsigned long long m = __ballot(fa); m; m &= m - 1) {
                const int k = __ffsll((long long)m) - 1;
                const double rx = readlane_double(ax, k), ry = readlane_double(ay, k), rz = readlane_double(az, k);
                if (fb) widest_pair(rx, ry, rz, bx, by, bz, sb, db);       // (a ray with itself: angle 0, never wider)
            }
        }
    }
    return wave_max(atan2(sb, db));
}

// The damped Gauss-Newton refinements (a point in k_triangulate, a pose in k_resect): the damping after an accepted
// trial (cost not raised) and after a rejected one; the stops: |step| dn below xtol relative to the parameters' norm, and
// a trial rejected although the model (gd = g . d, dHd = d^T H d) promised less than 1e-12 of cost = sum |r|^2 --
// rounding of the cost's own evaluation (differences of ~1e3-pixel numbers) decides such trials, more damping does not.
__device__ __forceinline__ double gn_damping_after_accept(double lam) { return lam > 1e-6 ? 0.1 * lam : 0.0; }
__device__ __forceinline__ double gn_damping_after_reject(double lam) { return lam == 0.0 ? 1e-3 : 10.0 * lam; }
__device__ __forceinline__ bool gn_step_below_tol(double dn, double norm, double xtol) { return dn <= xtol * (norm + xtol); }
__device__ __forceinline__ bool gn_gain_negligible(double gd, double dHd, double cost) { return -(gd + 0.5 * dHd) <= 1e-12 * 0.5 * cost; }

// ---------------------------------------------------------------------------------------------
// Reprojection statistics and track filtering (sfmba_reprojection_stats).  Three sweeps over
// buffers of their own -- nothing a solver form reads or writes is touched:
//   k_obs_stats    per observation, point-major: err = |r|, depth = z of R (X - T), keep = the observation's own test
//   k_point_stats  per point over its run: views, max err, sum err^2, min depth, widest ray angle, the point's verdict,
//                  and the FINAL mask of its observations (own test and point kept); one row of partial sums per workgroup
//   k_cam_stats    per camera over a camera-major permutation of ALL observations (cameras held still included,
//                  which the solver's camera-major lists leave out): kept views, sum and max err, observations behind
//   k_stats_summary  one workgroup adds the rows of k_point_stats in row order
// No atomics: a point's sums run over its observations in stored order, a camera's and the summary's are added in a
// fixed order; maxima, minima and counts do not depend on the order at all.
// ---------------------------------------------------------------------------------------------
struct StatsFilter { double max_err, min_depth, min_angle_deg; int min_views; };

// The residual-only sweep (k_resjac<.., false, true, ..>) with other stores: same persistent workgroups, same camera
// table in LDS (or rows gathered through the wave's slab), same pipeline -- indices two batches ahead, pixel and point
// one batch ahead, so three observations per lane are in flight -- and the same observe<false>, so rx, ry are the
// solver's residual bit for bit.  Per observation it reads 4 + 4 + 16 (8 in fp32 storage) bytes and the gathered point,
// and writes err | depth as one 16-byte store and the mask byte.
// A non-finite err fails the test whatever the threshold (+inf <= +inf would pass it).
template <bool LDS_TAB, bool F32>
__global__ __launch_bounds__(kSweepThreads) void k_obs_stats(
    const double* __restrict__ camtab, const double* __restrict__ pts, const int* __restrict__ cam_idx,
    const int* __restrict__ pt_idx, const double* __restrict__ uv, double* __restrict__ ed,
    unsigned char* __restrict__ keep, int N, int C, KMat K, double max_err, double min_depth) {
    extern __shared__ __align__(16) double smem[];
    const int stride = gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int c0 = 0, p0 = 0, c1 = 0, p1 = 0;
    double2 uv0 = make_double2(0.0, 0.0);
    double X0 = 0.0, Y0 = 0.0, Z0 = 0.0;
    if (i < N) { c0 = cam_idx[i]; p0 = pt_idx[i]; uv0 = load_pair(uv, F32, i); }
    if (i + stride < N) { c1 = cam_idx[i + stride]; p1 = pt_idx[i + stride]; }
    if (i < N) { const double* __restrict__ Xp = pts + 3 * (size_t)p0; X0 = Xp[0]; Y0 = Xp[1]; Z0 = Xp[2]; }
    if (LDS_TAB) {                               // (written out like the row loads below: see the note at cam_depth)
        const int n2 = (C * kCamRow) >> 1;
        const double2* __restrict__ src = reinterpret_cast<const double2*>(camtab);
        double2* __restrict__ dst = reinterpret_cast<double2*>(smem);
        for (int k = threadIdx.x; k < n2; k += blockDim.x) dst[k] = src[k];
        __syncthreads();
    }
    double* const slab = smem + (size_t)(threadIdx.x >> 6) * kRowSlabDoubles;
    if (!LDS_TAB && i - lane < N) rows_request(camtab, c0, lane, slab);
    while (i - lane < N) {                       // wave-uniform: rows_request shuffles over all 64 lanes
        const bool on = i < N;
        const int in = i + stride, in2 = in + stride;
        double tl[kCamRow];
        if (!LDS_TAB) rows_wait();
        {
            const double2* __restrict__ trow = reinterpret_cast<const double2*>(LDS_TAB ? smem + (size_t)c0 * kCamRow
                                                                                         : slab + (size_t)lane * kCamRow);
#pragma unroll
            for (int k = 0; k < kCamRow / 2; ++k) { const double2 q = trow[k]; tl[2 * k] = q.x; tl[2 * k + 1] = q.y; }
        }
        if (!LDS_TAB) {
            rows_read_done();
            if (in - lane < N) rows_request(camtab, c1, lane, slab);
        }
        int c2 = 0, p2 = 0;
        double2 uv1 = make_double2(0.0, 0.0);
        double X1 = 0.0, Y1 = 0.0, Z1 = 0.0;
        if (in2 < N) { c2 = cam_idx[in2]; p2 = pt_idx[in2]; }
        if (in < N) {
            uv1 = load_pair(uv, F32, in);
            const double* __restrict__ Xp = pts + 3 * (size_t)p1;
            X1 = Xp[0]; Y1 = Xp[1]; Z1 = Xp[2];
        }
        double jc[12], jp[6], rx, ry;
        observe<false>(tl, X0, Y0, Z0, uv0.x, uv0.y, K, rx, ry, jc, jp);
        const double depth = cam_depth(tl, X0, Y0, Z0);
        const double err = sqrt(rx * rx + ry * ry);
        if (on) {
            st16(ed + 2 * (size_t)i, err, depth);
            keep[i] = (err <= max_err && err < INFINITY && depth > min_depth) ? 1 : 0;
        }
        i = in;
        c0 = c1; p0 = p1; c1 = c2; p1 = p2;
        uv0 = uv1; X0 = X1; Y0 = Y1; Z0 = Z1;
    }
}

// One lane per point while the run is shorter than kStatsLongTrack (widest_angle_lane), and the other 63 lanes of the
// wave wait for the longest run among them.  From kStatsLongTrack on the WAVE takes the point after its lanes have
// finished their short ones (for_each_long_run, widest_angle_wave with the run's other sums as its per-block work).
// A wave-handled run of n <= 64 costs about n steps of the whole wave, a lane-handled one n^2 / 2 steps of a
// wave whose other lanes may be idle: a lone long run gains from n = 2 on, 64 equally long ones only from n = 128 on;
// 32 sits between (a lone run of 31 holds its wave for 465 steps, 64 runs of 32 cost 2048 instead of 496).
constexpr int kStatsPtThreads = 256;
constexpr int kStatsPart = 6;        // partial row of a workgroup: points kept, observations kept, behind, sum err, sum err^2, max err
static_assert(kStatsLongTrack <= 32, "the lane form keeps the run's mask in 32 bits");

struct PointStatsOut {
    int* __restrict__ views;
    double* __restrict__ max_err;
    double* __restrict__ sum_err2;
    double* __restrict__ min_depth;
    double* __restrict__ angle_deg;
    unsigned char* __restrict__ keep;
};

__global__ __launch_bounds__(kStatsPtThreads) void k_point_stats(
    const int* __restrict__ pt_ptr, const int* __restrict__ cam_idx, const double* __restrict__ camtab,
    const double* __restrict__ pts, const double* __restrict__ ed, const unsigned char* __restrict__ keep, int P,
    StatsFilter flt, PointStatsOut out, unsigned char* __restrict__ keep_final, double* __restrict__ part) {
    __shared__ double red[(kStatsPtThreads / 64) * kStatsPart];
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const double2* __restrict__ ed2 = reinterpret_cast<const double2*>(ed);
    constexpr double kDeg = 57.295779513082320877;
    int b = 0, e = 0;
    double X = 0.0, Y = 0.0, Z = 0.0;
    if (p < P) { b = pt_ptr[p]; e = pt_ptr[p + 1]; X = pts[3 * (size_t)p]; Y = pts[3 * (size_t)p + 1]; Z = pts[3 * (size_t)p + 2]; }
    const int n = e - b;
    int views = 0, behind = 0;
    double maxe = 0.0, s1 = 0.0, s2 = 0.0, mind = INFINITY, ang = 0.0;
    const auto centre = [&](int k) { return camtab + (size_t)cam_idx[k] * kCamRow + 9; };
    if (n < kStatsLongTrack) {
        unsigned mask = 0u;
        for (int k = 0; k < n; ++k) {
            const double2 q = ed2[b + k];
            mind = fmin(mind, q.y);
            behind += q.y <= 0.0 ? 1 : 0;
            if (keep[b + k]) {
                mask |= 1u << k;
                ++views;
                maxe = fmax(maxe, q.x);
                s2 += q.x * q.x;
                s1 += q.x;
            }
        }
        ang = widest_angle_lane(b, e, X, Y, Z, [&](int k) { return ((mask >> (k - b)) & 1u) != 0u; }, centre);
    }
    for_each_long_run(n >= kStatsLongTrack, b, e, X, Y, Z, [&](int q, int qb, int qe, double qX, double qY, double qZ) {
        int wv = 0, wbeh = 0;
        double wmax = 0.0, wmin = INFINITY, ws1 = 0.0, ws2 = 0.0;
        const double wang = widest_angle_wave(qb, qe, lane, qX, qY, qZ, [&](int k) { return keep[k] != 0; }, centre,
                                              [&](int kb, bool on, bool fb) {
            double2 eb = make_double2(0.0, INFINITY);
            if (on) {
                eb = ed2[kb];
                wmin = fmin(wmin, eb.y);
                wbeh += eb.y <= 0.0 ? 1 : 0;
            }
            if (fb) { ++wv; wmax = fmax(wmax, eb.x); }
            for (unsigned long long m = __ballot(fb); m; m &= m - 1) {     // the two sums in stored order, on every lane alike
                const double v = readlane_double(eb.x, __ffsll((long long)m) - 1);
                ws2 += v * v;
                ws1 += v;
            }
        });
        wv = wave_isum(wv);
        wbeh = wave_isum(wbeh);
        wmax = wave_max(wmax);
        wmin = wave_min(wmin);
        const unsigned char qk = (wv >= flt.min_views && wang * kDeg >= flt.min_angle_deg) ? 1 : 0;
        for (int k = qb + lane; k < qe; k += 64) keep_final[k] = keep[k] & qk;
        if (lane == q) { views = wv; behind = wbeh; maxe = wmax; mind = wmin; s1 = ws1; s2 = ws2; ang = wang; }
    });
    const double deg = ang * kDeg;
    const bool pk = p < P && views >= flt.min_views && deg >= flt.min_angle_deg;
    if (p < P) {
        out.views[p] = views; out.max_err[p] = maxe; out.sum_err2[p] = s2; out.min_depth[p] = mind;
        out.angle_deg[p] = deg; out.keep[p] = pk ? 1 : 0;
        if (n < kStatsLongTrack)
            for (int k = 0; k < n; ++k) keep_final[b + k] = keep[b + k] & (pk ? 1 : 0);
    }
    // the workgroup's row: sums over its points in lane order inside a wave, wave by wave
    double v[kStatsPart - 1] = {pk ? 1.0 : 0.0, pk ? (double)views : 0.0, (double)behind, pk ? s1 : 0.0, pk ? s2 : 0.0};
    const double vmax = wave_max(pk ? maxe : 0.0);
    block_sum<kStatsPart - 1>(v, red);
    __shared__ double redmax[kStatsPtThreads / 64];
    if (lane == 0) redmax[threadIdx.x >> 6] = vmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* __restrict__ row = part + (size_t)blockIdx.x * kStatsPart;
#pragma unroll
        for (int k = 0; k < kStatsPart - 1; ++k) row[k] = v[k];
        double m = 0.0;
        for (int k = 0; k < kStatsPtThreads / 64; ++k) m = fmax(m, redmax[k]);
        row[kStatsPart - 1] = m;
    }
}

// rows of k_point_stats -> out[0..5] (points kept, observations kept, behind, sum err, sum err^2, max err): every thread
// adds rows tid, tid + 256, ... in that order, then the 256 sums are added in thread order
__global__ __launch_bounds__(256) void k_stats_summary(const double* __restrict__ part, int rows, double* __restrict__ out) {
    __shared__ double red[4 * kStatsPart];
    double v[kStatsPart - 1] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double m = 0.0;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const double* __restrict__ row = part + (size_t)r * kStatsPart;
#pragma unroll
        for (int k = 0; k < kStatsPart - 1; ++k) v[k] += row[k];
        m = fmax(m, row[kStatsPart - 1]);
    }
    m = wave_max(m);
    block_sum<kStatsPart - 1>(v, red);
    __shared__ double redmax[4];
    if ((threadIdx.x & 63) == 0) redmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kStatsPart - 1; ++k) out[k] = v[k];
        out[kStatsPart - 1] = fmax(fmax(redmax[0], redmax[1]), fmax(redmax[2], redmax[3]));
    }
}

// One workgroup per camera over its slice of the permutation (camera-major position -> point-major position): thread t
// takes entries t, t + 256, ... in that order (four gathers in flight), the 256 partial sums are added in thread order.
__global__ __launch_bounds__(kCamThreads) void k_cam_stats(const int* __restrict__ cam_ptr, const int* __restrict__ perm,
                                                           const double* __restrict__ ed, const unsigned char* __restrict__ keep_final,
                                                           int* __restrict__ views, double* __restrict__ sum_err,
                                                           double* __restrict__ max_err, int* __restrict__ n_behind) {
    __shared__ double red[kCamWaves];
    __shared__ double redmax[kCamWaves];
    __shared__ int redi[2 * kCamWaves];
    const int c = blockIdx.x;
    const int b = cam_ptr[c], e = cam_ptr[c + 1];
    const double2* __restrict__ ed2 = reinterpret_cast<const double2*>(ed);
    int nv = 0, nb = 0;
    double s = 0.0, m = 0.0;
    for (int j0 = b + (int)threadIdx.x; j0 < e; j0 += kCamThreads * kCamUnroll) {
        int idx[kCamUnroll];
        double2 q[kCamUnroll];
        unsigned char kf[kCamUnroll];
#pragma unroll
        for (int u = 0; u < kCamUnroll; ++u) { const int j = j0 + u * kCamThreads; idx[u] = j < e ? perm[j] : -1; }
#pragma unroll
        for (int u = 0; u < kCamUnroll; ++u) {
            q[u] = make_double2(0.0, 1.0); kf[u] = 0;
            if (idx[u] >= 0) { q[u] = ed2[idx[u]]; kf[u] = keep_final[idx[u]]; }
        }
#pragma unroll
        for (int u = 0; u < kCamUnroll; ++u) {
            if (idx[u] >= 0 && q[u].y <= 0.0) ++nb;
            if (kf[u]) { ++nv; s += q[u].x; m = fmax(m, q[u].x); }
        }
    }
    s = wave_sum(s); m = wave_max(m); nv = wave_isum(nv); nb = wave_isum(nb);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w] = s; redmax[w] = m; redi[2 * w] = nv; redi[2 * w + 1] = nb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0, tm = 0.0;
        int tv = 0, tb = 0;
        for (int k = 0; k < kCamWaves; ++k) { ts += red[k]; tm = fmax(tm, redmax[k]); tv += redi[2 * k]; tb += redi[2 * k + 1]; }
        views[c] = tv; sum_err[c] = ts; max_err[c] = tm; n_behind[c] = tb;
    }
}

// The permutation k_cam_stats walks: the stable counting sort of k_cam_hist / k_cam_offsets with no camera left out.
//   k_stats_cam_count  hist[slice][C] -> cnt[c], one thread per camera
//   k_stats_cam_scan   one workgroup: cam_ptr = exclusive prefix sums of cnt (every thread a contiguous piece)
//   k_stats_cam_scatter  k_cam_scatter's walk, storing the point-major position itself
__global__ __launch_bounds__(256) void k_stats_cam_count(const int* __restrict__ hist, int B, int C, int* __restrict__ cnt) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    int total = 0;
    for (int b0 = 0; b0 < B; b0 += 16) {
        int n[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) n[u] = b0 + u < B ? hist[(size_t)(b0 + u) * C + c] : 0;
#pragma unroll
        for (int u = 0; u < 16; ++u) total += n[u];
    }
    cnt[c] = total;
}
__global__ __launch_bounds__(1024) void k_stats_cam_scan(const int* __restrict__ cnt, int C, int* __restrict__ cam_ptr) {
    __shared__ int tot[1024];
    const int per = (C + 1023) / 1024;
    const int c0 = min(C, (int)threadIdx.x * per), c1 = min(C, c0 + per);
    int s = 0;
    for (int c = c0; c < c1; ++c) s += cnt[c];
    tot[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                       // inclusive scan of the 1024 piece totals
        const int add = (int)threadIdx.x >= o ? tot[threadIdx.x - o] : 0;
        __syncthreads();
        tot[threadIdx.x] += add;
        __syncthreads();
    }
    int run = tot[threadIdx.x] - s;
    for (int c = c0; c < c1; ++c) { cam_ptr[c] = run; run += cnt[c]; }
    if (threadIdx.x == 1023) cam_ptr[C] = tot[1023];
}
__global__ __launch_bounds__(64) void k_stats_cam_scatter(const int* __restrict__ cam_idx, int N, int C, int per, int key_bits,
                                                          const int* __restrict__ off, int* __restrict__ perm) {
    extern __shared__ int cur[];
    for (int c = threadIdx.x; c < C; c += 64) cur[c] = off[(size_t)blockIdx.x * C + c];
    __syncthreads();
    const int lane = threadIdx.x;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int b0 = blockIdx.x * per, b1 = min(N, b0 + per);
    int cn = b0 + lane < b1 ? cam_idx[b0 + lane] : -1;
    for (int k0 = b0; k0 < b1; k0 += 64) {
        const int c = cn;
        cn = k0 + 64 + lane < b1 ? cam_idx[k0 + 64 + lane] : -1;
        const bool act = c >= 0;
        unsigned long long eq = __ballot(act);                 // lanes with the same camera as this one
        for (int bit = 0; bit < key_bits; ++bit) {
            const unsigned long long m = __ballot(act && ((c >> bit) & 1));
            eq &= ((c >> bit) & 1) ? m : ~m;
        }
        if (act) {
            perm[cur[c] + __popcll(eq & lt)] = k0 + lane;
            if ((eq >> lane) == 1ull) cur[c] += __popcll(eq);   // the highest lane of the group advances the offset
        }
        __builtin_amdgcn_wave_barrier();                         // (one wave: LDS operations execute in program order)
    }
}

// ---------------------------------------------------------------------------------------------
// Triangulation (sfmba_triangulate): per selected point, over the used observations of its run,
//   linear stage  the n-view DLT of cv2.triangulatePoints: rows u M3 - M1, v M3 - M2 with M = K R [I | -T], A^T A as ten
//                 sums, its smallest eigenvector by cyclic Jacobi rotations, X = v[:3] / v[3] (unknowns neither
//                 translated nor rescaled: for two views this is the reference's minimiser)
//   refinement    damped Gauss-Newton on 1/2 sum |r|^2 over X, r and d r / d X from observe<> (the solver's residual);
//                 one pass over the run per trial point, which yields its cost and the next linearisation
//   verdict       at the result: depth and err of every used observation, the widest ray angle (widest_angle_lane / _wave)
// A lane takes a run shorter than kStatsLongTrack, the wave the longer ones afterwards (for_each_long_run), lanes
// striding the run and the sums combined by an xor butterfly, which leaves the same bits on every lane -- so the wave's
// lanes take every decision alike.  The 4x4 eigenproblem is jacobi_sweeps<4>, the schedule of the refinement gn_*.  Camera rows are the compact R | T rows of the table (six 16-byte
// loads), staged in LDS by persistent workgroups when the table fits (forms.lds_tab), else read through L2.
// No atomics; nothing of the solver's is read but the structure arrays and the pixels.
// ---------------------------------------------------------------------------------------------
constexpr int kTriThreads = 512;     // two waves per SIMD: the Jacobi state (26 doubles) and a linearisation stay in registers
constexpr int kTriOk = 0, kTriFewViews = 1, kTriAtInfinity = 2, kTriBehind = 3, kTriLowAngle = 4, kTriHighError = 5,
              kTriNotSelected = -1;
struct TriOptions { int max_iter, min_views; double xtol, min_angle_deg, min_depth, max_err; };
struct TriIn {
    const int* __restrict__ pt_ptr;
    const int* __restrict__ cam_idx;
    const double* __restrict__ uv;
    const unsigned char* __restrict__ use;       // [N] stored order, or null: every observation
    const unsigned char* __restrict__ select;    // [P], or null: every point
    const double* __restrict__ pts;              // the points of x
};
struct TriOut {
    double* __restrict__ X;
    int* __restrict__ status;
    int* __restrict__ views;
    int* __restrict__ iters;
    double* __restrict__ rms;
    double* __restrict__ angle_deg;
    int* __restrict__ ok_part;                   // [workgroups] points with status OK
};
struct TriResult { int status, views, iters; double X, Y, Z, rms, ang; };

// eigenvector of the smallest eigenvalue of a (destroyed)
__device__ __forceinline__ void smallest_eigenvector4(double (&a)[10], double& w0, double& w1, double& w2, double& w3) {
    double v[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    jacobi_sweeps<4>(a, v);
    double lo = a[0];
    w0 = v[0]; w1 = v[4]; w2 = v[8]; w3 = v[12];
    if (a[4] < lo) { lo = a[4]; w0 = v[1]; w1 = v[5]; w2 = v[9]; w3 = v[13]; }
    if (a[7] < lo) { lo = a[7]; w0 = v[2]; w1 = v[6]; w2 = v[10]; w3 = v[14]; }
    if (a[9] < lo) { lo = a[9]; w0 = v[3]; w1 = v[7]; w2 = v[11]; w3 = v[15]; }
}

// R | T of camera c into the first twelve entries of an observe<> row (w, b, c are not needed for d r / d X)
__device__ __forceinline__ void tri_load_row(const double* __restrict__ rt, int c, double* __restrict__ tl) {
    const double2* __restrict__ row = reinterpret_cast<const double2*>(rt + (size_t)c * kCamRT);
#pragma unroll
    for (int k = 0; k < kCamRT / 2; ++k) { const double2 q = row[k]; tl[2 * k] = q.x; tl[2 * k + 1] = q.y; }
#pragma unroll
    for (int k = kCamRT; k < kCamRow; ++k) tl[k] = 0.0;
}

// a += the two DLT rows of the observation stored at k: the body of the n-view pass below and of the two-view
// hypotheses of k_tri_ransac
template <bool F32>
__device__ __forceinline__ void tri_dlt_rows(const double* __restrict__ rt, const TriIn& in, int k, const KMat& K, double (&a)[10]) {
    double tl[kCamRow];
    tri_load_row(rt, in.cam_idx[k], tl);
    const double2 px = load_pair(in.uv, F32, k);
    double m[12];                                                // M = K R [I | -T], row-major 3x4
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) m[4 * i + j] = K.k[3 * i] * tl[j] + K.k[3 * i + 1] * tl[3 + j] + K.k[3 * i + 2] * tl[6 + j];
        m[4 * i + 3] = -(m[4 * i] * tl[9] + m[4 * i + 1] * tl[10] + m[4 * i + 2] * tl[11]);
    }
    double ru[4], rv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { ru[j] = px.x * m[8 + j] - m[j]; rv[j] = px.y * m[8 + j] - m[4 + j]; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) a[sym<4>(i, j)] += ru[i] * ru[j] + rv[i] * rv[j];
}

// the linear stage's pass: a += the two DLT rows of every used observation; used = their number
template <bool F32, bool WAVE>
__device__ __forceinline__ void tri_dlt_pass(const double* __restrict__ rt, const TriIn& in, int b, int e, int lane,
                                             const KMat& K, double (&a)[10], int& used) {
#pragma unroll
    for (int q = 0; q < 10; ++q) a[q] = 0.0;
    used = 0;
#pragma unroll 1
    for (int k = WAVE ? b + lane : b; k < e; k += WAVE ? 64 : 1) {
        if (in.use != nullptr && !in.use[k]) continue;
        tri_dlt_rows<F32>(rt, in, k, K, a);
        ++used;
    }
    if (WAVE) {
#pragma unroll
        for (int q = 0; q < 10; ++q) a[q] = wave_butterfly_sum(a[q]);
        used = wave_isum(used);
    }
}

// one pass at (X, Y, Z): s = sum |r|^2, g = sum Jp^T r (3), H = sum Jp^T Jp (6, upper); smallest depth, largest err
template <bool F32, bool WAVE>
__device__ __forceinline__ void tri_linearise(const double* __restrict__ rt, const TriIn& in, int b, int e, int lane,
                                              const KMat& K, double X, double Y, double Z, double (&s)[10],
                                              double& mind, double& maxe) {
#pragma unroll
    for (int q = 0; q < 10; ++q) s[q] = 0.0;
    mind = INFINITY; maxe = 0.0;
#pragma unroll 1
    for (int k = WAVE ? b + lane : b; k < e; k += WAVE ? 64 : 1) {
        if (in.use != nullptr && !in.use[k]) continue;
        double tl[kCamRow];
        tri_load_row(rt, in.cam_idx[k], tl);
        const double2 px = load_pair(in.uv, F32, k);
        double jc[12], jp[6], rx, ry;
        observe<true>(tl, X, Y, Z, px.x, px.y, K, rx, ry, jc, jp);
        const double depth = cam_depth(tl, X, Y, Z);
        const double e2 = rx * rx + ry * ry;
        s[0] += e2;
        s[1] += jp[0] * rx + jp[3] * ry; s[2] += jp[1] * rx + jp[4] * ry; s[3] += jp[2] * rx + jp[5] * ry;
        s[4] += jp[0] * jp[0] + jp[3] * jp[3]; s[5] += jp[0] * jp[1] + jp[3] * jp[4]; s[6] += jp[0] * jp[2] + jp[3] * jp[5];
        s[7] += jp[1] * jp[1] + jp[4] * jp[4]; s[8] += jp[1] * jp[2] + jp[4] * jp[5];
        s[9] += jp[2] * jp[2] + jp[5] * jp[5];
        mind = fmin(mind, depth);
        maxe = fmax(maxe, sqrt(e2));
    }
    if (WAVE) {
#pragma unroll
        for (int q = 0; q < 10; ++q) s[q] = wave_butterfly_sum(s[q]);
        mind = wave_min(mind);
        maxe = wave_max(maxe);
    }
}

// widest angle (radians) between the rays X - T of the used observations of the run
template <bool WAVE>
__device__ __forceinline__ double tri_widest_angle(const double* __restrict__ rt, const TriIn& in, int b, int e, int lane,
                                                   double X, double Y, double Z) {
    const auto used = [&](int k) { return in.use == nullptr || in.use[k] != 0; };
    const auto centre = [&](int k) { return rt + (size_t)in.cam_idx[k] * kCamRT + 9; };
    if (!WAVE) return widest_angle_lane(b, e, X, Y, Z, used, centre);
    return widest_angle_wave(b, e, lane, X, Y, Z, used, centre, [](int, bool, bool) {});
}

// One point.  WAVE: called by all 64 lanes with the same arguments; every lane leaves with the same result.
// (X0, Y0, Z0): the point of x, handed back whenever the status is not OK.
template <bool F32, bool WAVE>
__device__ __forceinline__ void tri_point(const double* __restrict__ rt, const TriIn& in, int b, int e, int lane, const KMat& K,
                                          const TriOptions& o, double X0, double Y0, double Z0, TriResult& r) {
    constexpr double kDeg = 57.295779513082320877;
    r.status = kTriFewViews; r.iters = 0;
    r.X = X0; r.Y = Y0; r.Z = Z0;
    r.rms = NAN; r.ang = NAN;
    double X, Y, Z;
    {
        double a[10];
        tri_dlt_pass<F32, WAVE>(rt, in, b, e, lane, K, a, r.views);
        if (r.views < max(2, o.min_views)) return;
        double w0, w1, w2, w3;
        smallest_eigenvector4(a, w0, w1, w2, w3);
        const double nw = sqrt(w0 * w0 + w1 * w1 + w2 * w2 + w3 * w3);
        r.status = kTriAtInfinity;
        if (!(fabs(w3) > 1e-12 * nw)) return;                    // (false for a NaN as well)
        X = w0 / w3; Y = w1 / w3; Z = w2 / w3;
    }
    double s[10], mind, maxe;
    tri_linearise<F32, WAVE>(rt, in, b, e, lane, K, X, Y, Z, s, mind, maxe);
    if (!(fabs(s[0]) < INFINITY && fabs(X) + fabs(Y) + fabs(Z) < INFINITY)) return;
    double lam = 0.0;
    int it = 0;
#pragma unroll 1
    while (it < o.max_iter) {
        const double hd[6] = {s[4] * (1.0 + lam), s[5], s[6], s[7] * (1.0 + lam), s[8], s[9] * (1.0 + lam)};
        double inv[6];
        chol3_inverse(hd, inv);
        const double d0 = -(inv[0] * s[1] + inv[1] * s[2] + inv[2] * s[3]);
        const double d1 = -(inv[1] * s[1] + inv[3] * s[2] + inv[4] * s[3]);
        const double d2 = -(inv[2] * s[1] + inv[4] * s[2] + inv[5] * s[3]);
        const double dn = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (gn_step_below_tol(dn, sqrt(X * X + Y * Y + Z * Z), o.xtol)) break;     // the step on offer is below the tolerance already
        const double Xt = X + d0, Yt = Y + d1, Zt = Z + d2;
        double st[10], mt, et;
        tri_linearise<F32, WAVE>(rt, in, b, e, lane, K, Xt, Yt, Zt, st, mt, et);
        ++it;
        if (st[0] <= s[0]) {                                     // (a non-finite trial cost is a rejection)
            X = Xt; Y = Yt; Z = Zt;
#pragma unroll
            for (int q = 0; q < 10; ++q) s[q] = st[q];
            mind = mt; maxe = et;
            lam = gn_damping_after_accept(lam);
            if (gn_step_below_tol(dn, sqrt(X * X + Y * Y + Z * Z), o.xtol)) break;
        } else {
            const double gd = s[1] * d0 + s[2] * d1 + s[3] * d2;
            const double dHd = d0 * (s[4] * d0 + s[5] * d1 + s[6] * d2) + d1 * (s[5] * d0 + s[7] * d1 + s[8] * d2) +
                               d2 * (s[6] * d0 + s[8] * d1 + s[9] * d2);
            if (gn_gain_negligible(gd, dHd, s[0])) break;
            lam = gn_damping_after_reject(lam);
        }
    }
    r.iters = it;
    r.rms = sqrt(s[0] / (double)r.views);
    r.ang = kDeg * tri_widest_angle<WAVE>(rt, in, b, e, lane, X, Y, Z);
    if (!(r.ang == r.ang)) return;
    if (mind <= o.min_depth) { r.status = kTriBehind; return; }
    if (r.ang < o.min_angle_deg) { r.status = kTriLowAngle; return; }
    if (maxe > o.max_err) { r.status = kTriHighError; return; }
    r.status = kTriOk;
    r.X = X; r.Y = Y; r.Z = Z;
}

template <bool LDS_TAB, bool F32>
__global__ __launch_bounds__(kTriThreads) void k_triangulate(const double* __restrict__ camtab, TriIn in, int P, int C, KMat K,
                                                              TriOptions opt, TriOut out) {
    extern __shared__ __align__(16) double smem[];
    __shared__ int red[kTriThreads / 64];
    const int lane = threadIdx.x & 63;
    const double* __restrict__ rt_global = camtab + cam_rt_offset(C);
    if (LDS_TAB) stage_table(rt_global, C * kCamRT, smem);
    const double* __restrict__ rt = LDS_TAB ? smem : rt_global;
    int n_ok = 0;
    for (int base = blockIdx.x * kTriThreads; base < P; base += gridDim.x * kTriThreads) {     // uniform over the workgroup
        const int p = base + (int)threadIdx.x;
        int b = 0, e = 0;
        double X0 = 0.0, Y0 = 0.0, Z0 = 0.0;
        bool sel = false;
        if (p < P) {
            b = in.pt_ptr[p]; e = in.pt_ptr[p + 1];
            X0 = in.pts[3 * (size_t)p]; Y0 = in.pts[3 * (size_t)p + 1]; Z0 = in.pts[3 * (size_t)p + 2];
            sel = in.select == nullptr || in.select[p] != 0;
        }
        const int n = e - b;
        TriResult r;
        r.status = kTriNotSelected; r.views = 0; r.iters = 0;
        r.X = X0; r.Y = Y0; r.Z = Z0; r.rms = NAN; r.ang = NAN;
        if (sel && n < kStatsLongTrack) tri_point<F32, false>(rt, in, b, e, 0, K, opt, X0, Y0, Z0, r);
        for_each_long_run(sel && n >= kStatsLongTrack, b, e, X0, Y0, Z0,
                          [&](int q, int qb, int qe, double qX, double qY, double qZ) {
            TriResult w;
            tri_point<F32, true>(rt, in, qb, qe, lane, K, opt, qX, qY, qZ, w);
            if (lane == q) r = w;
        });
        if (p < P) {
            out.X[3 * (size_t)p] = r.X; out.X[3 * (size_t)p + 1] = r.Y; out.X[3 * (size_t)p + 2] = r.Z;
            out.status[p] = r.status; out.views[p] = r.views; out.iters[p] = r.iters;
            out.rms[p] = r.rms; out.angle_deg[p] = r.ang;
            n_ok += r.status == kTriOk ? 1 : 0;
        }
    }
    // points with status OK of this workgroup: wave sums, added in wave order
    n_ok = wave_isum(n_ok);
    if (lane == 0) red[threadIdx.x >> 6] = n_ok;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < kTriThreads / 64; ++k) t += red[k];
        out.ok_part[blockIdx.x] = t;
    }
}

// ---------------------------------------------------------------------------------------------
// Resection (sfmba_resect): per selected camera, over its used observations in camera-major stored
// order (the permutation of stats_cam_perm),
//   linear stage  the n-point DLT of the reference's _solve_pnp_linear: pixels normalised by K^-1, rows [P, 0, -u P],
//                 [0, P, -v P] with P = (X, Y, Z, 1), A^T A from forty sums (S, S_u, S_v, S_w, each a symmetric 4x4), its
//                 smallest eigenvector by cyclic Jacobi rotations on the 12x12 matrix in LDS (one wave, lane r owns row
//                 r; pairs (0,1), (0,2), ..., (0,11), (1,2), ..., (10,11)), h = [M | m], R = M (M^T M)^(-1/2) by a 3x3
//                 Jacobi, t = m / (mean singular value of M), both negated when det M < 0, T = -R^T t, omega through a
//                 quaternion
//   refinement    damped Gauss-Newton on 1/2 sum |r|^2 over (omega, T): r and the 2x6 block from observe<true>, the
//                 trial pose's table row made by thread 0 (cam_row_values) and shared through LDS; one pass over the
//                 slice per trial pose, which yields its cost and the next linearisation.  Damping, rejection and the
//                 stops are the shared gn_* schedule.
//   verdict       at the result: used observations, finiteness / the gap of A^T A, smallest depth, rms error
// One 256-thread workgroup per camera over its slice of the permutation, as in k_cam_stats: thread t takes entries t, t + 256, ... of the slice,
// kResectUnroll gathers in flight (entry -> stored position -> pixel, point index -> point); partial sums are combined
// by wave_sum and then over the waves in wave order (block_sum): same input, same bits.  Every decision is taken by
// thread 0 and handed to the workgroup through LDS.  No atomics; nothing of the solver's is read but the structure
// arrays and the pixels.
// ---------------------------------------------------------------------------------------------
constexpr int kResectUnroll = 4;
constexpr int kResectSweeps = 30;    // cap of the Jacobi sweeps of the 12x12 matrix (it converges in 6..10)
constexpr int kResOk = 0, kResFewViews = 1, kResDegenerate = 2, kResBehind = 3, kResHighError = 4, kResNotSelected = -1;
struct ResectOptions { int max_iter, min_views, start; double xtol, min_depth, max_rms; };
struct ResectIn {
    const int* __restrict__ cam_ptr;             // [C + 1] slices of perm
    const int* __restrict__ perm;                // camera-major position -> stored position
    const int* __restrict__ pt_idx;              // [N] stored order
    const double* __restrict__ uv;
    const unsigned char* __restrict__ use;       // [N] stored order, or null: every observation
    const unsigned char* __restrict__ select;    // [C], or null: every camera
    const double* __restrict__ x;                // the parameter vector: 6C camera parameters, then the points
};
struct ResectOut {
    double* __restrict__ cam;                    // [C][6]
    int* __restrict__ status;
    int* __restrict__ views;
    int* __restrict__ iters;
    double* __restrict__ rms;
    int* __restrict__ ok_part;                   // [C] 1 where the status is OK
};
struct ResectObs { double X, Y, Z, u, v; bool on; };

// entries j0, j0 + 256, ... of the slice [.., e): all index loads, then all pixel / point-index loads, then the points
template <bool F32>
__device__ __forceinline__ void resect_gather(const ResectIn& in, const double* __restrict__ pts, int j0, int e,
                                              ResectObs (&o)[kResectUnroll]) {
    int idx[kResectUnroll], p[kResectUnroll];
#pragma unroll
    for (int u = 0; u < kResectUnroll; ++u) { const int j = j0 + u * kCamThreads; idx[u] = j < e ? in.perm[j] : -1; }
    if (in.use != nullptr) {
        unsigned char f[kResectUnroll];
#pragma unroll
        for (int u = 0; u < kResectUnroll; ++u) f[u] = idx[u] >= 0 ? in.use[idx[u]] : 0;
#pragma unroll
        for (int u = 0; u < kResectUnroll; ++u) if (!f[u]) idx[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < kResectUnroll; ++u) {
        o[u].on = idx[u] >= 0;
        p[u] = 0; o[u].u = 0.0; o[u].v = 0.0;
        if (o[u].on) { p[u] = in.pt_idx[idx[u]]; const double2 q = load_pair(in.uv, F32, idx[u]); o[u].u = q.x; o[u].v = q.y; }
    }
#pragma unroll
    for (int u = 0; u < kResectUnroll; ++u) {
        o[u].X = 0.0; o[u].Y = 0.0; o[u].Z = 1.0;
        if (o[u].on) { const double* __restrict__ Xp = pts + 3 * (size_t)p[u]; o[u].X = Xp[0]; o[u].Y = Xp[1]; o[u].Z = Xp[2]; }
    }
}

// the linear stage's pass: v = S (10) | S_u (10) | S_v (10) | S_w (10), upper triangles row by row; thread 0 leaves with
// the workgroup's sums and the number of used observations
template <bool F32>
__device__ __forceinline__ void resect_dlt_pass(const ResectIn& in, const double* __restrict__ pts, int b, int e, const KMat& Kinv,
                                                double (&v)[40], int& used, double* red, int* redi) {
#pragma unroll
    for (int q = 0; q < 40; ++q) v[q] = 0.0;
    used = 0;
#pragma unroll 1
    for (int j0 = b + (int)threadIdx.x; j0 < e; j0 += kCamThreads * kResectUnroll) {
        ResectObs o[kResectUnroll];
        resect_gather<F32>(in, pts, j0, e, o);
#pragma unroll
        for (int u = 0; u < kResectUnroll; ++u) {
            if (!o[u].on) continue;
            const double un = Kinv.k[0] * o[u].u + Kinv.k[1] * o[u].v + Kinv.k[2];
            const double vn = Kinv.k[3] * o[u].u + Kinv.k[4] * o[u].v + Kinv.k[5];
            const double w2 = un * un + vn * vn;
            const double P[4] = {o[u].X, o[u].Y, o[u].Z, 1.0};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i; j < 4; ++j) {
                    const double pp = P[i] * P[j];
                    v[sym<4>(i, j)] += pp;
                    v[10 + sym<4>(i, j)] += un * pp;
                    v[20 + sym<4>(i, j)] += vn * pp;
                    v[30 + sym<4>(i, j)] += w2 * pp;
                }
            ++used;
        }
    }
    used = wave_isum(used);
    if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = used;
    block_sum<40>(v, red);
    if (threadIdx.x == 0) {
        used = 0;
        for (int k = 0; k < kCamWaves; ++k) used += redi[k];
    }
}

// one pass at the pose of the table row tl: s[0] = sum |r|^2, s[1..6] = sum Jc^T r, s[7..27] = sum Jc^T Jc (upper, row by
// row); thread 0 leaves with the workgroup's sums, the smallest depth and the number of used observations
template <bool F32>
__device__ __forceinline__ void resect_linearise(const ResectIn& in, const double* __restrict__ pts, int b, int e, const KMat& K,
                                                 const double* __restrict__ tl, double (&s)[28], double& mind, int& used,
                                                 double* red, double* redm, int* redi) {
#pragma unroll
    for (int q = 0; q < 28; ++q) s[q] = 0.0;
    mind = INFINITY;
    used = 0;
#pragma unroll 1
    for (int j0 = b + (int)threadIdx.x; j0 < e; j0 += kCamThreads * kResectUnroll) {
        ResectObs o[kResectUnroll];
        resect_gather<F32>(in, pts, j0, e, o);
#pragma unroll
        for (int u = 0; u < kResectUnroll; ++u) {
            if (!o[u].on) continue;
            double jc[12], jp[6], rx, ry;
            observe<true>(tl, o[u].X, o[u].Y, o[u].Z, o[u].u, o[u].v, K, rx, ry, jc, jp);
            const double depth = cam_depth(tl, o[u].X, o[u].Y, o[u].Z);
            s[0] += rx * rx + ry * ry;
            int n = 7;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                s[1 + a] += jc[a] * rx + jc[6 + a] * ry;
#pragma unroll
                for (int c = a; c < 6; ++c) s[n++] += jc[a] * jc[c] + jc[6 + a] * jc[6 + c];
            }
            mind = fmin(mind, depth);
            ++used;
        }
    }
    mind = wave_min(mind);
    used = wave_isum(used);
    if ((threadIdx.x & 63) == 0) { redm[threadIdx.x >> 6] = mind; redi[threadIdx.x >> 6] = used; }
    block_sum<28>(s, red);
    if (threadIdx.x == 0) {
        used = 0; mind = INFINITY;
        for (int k = 0; k < kCamWaves; ++k) { used += redi[k]; mind = fmin(mind, redm[k]); }
    }
}

// Cyclic Jacobi on the symmetric 12x12 matrix A (full storage, LDS), eigenvectors in the columns of V, by ONE wave: lane
// r < 12 owns row r of both.  The LDS operations of one wave execute in program order (volatile keeps the compiler to it):
// within a rotation every lane reads before any lane writes.
__device__ __forceinline__ void resect_jacobi12(volatile double* A, volatile double* V, int lane) {
#pragma unroll 1
    for (int sweep = 0; sweep < kResectSweeps; ++sweep) {
        double off = 0.0, dia = 0.0;
        if (lane < 12) {
            for (int j = lane + 1; j < 12; ++j) off += fabs(A[12 * lane + j]);
            dia = fabs(A[13 * lane]);
        }
        off = wave_sum(off);
        dia = wave_sum(dia);
        if (!(off > 1e-40 * dia)) break;                         // (a NaN ends the loop too)
#pragma unroll 1
        for (int p = 0; p < 11; ++p)
#pragma unroll 1
            for (int q = p + 1; q < 12; ++q) {
                const double app = A[13 * p], aqq = A[13 * q], apq = A[12 * p + q];
                double t, c, s;
                jacobi_cs(app, aqq, apq, t, c, s);
                double arp = 0.0, arq = 0.0, vrp = 0.0, vrq = 0.0;
                if (lane < 12) { arp = A[12 * lane + p]; arq = A[12 * lane + q]; vrp = V[12 * lane + p]; vrq = V[12 * lane + q]; }
                if (lane < 12) {
                    V[12 * lane + p] = c * vrp - s * vrq;
                    V[12 * lane + q] = s * vrp + c * vrq;
                    if (lane == p) { A[13 * p] = app - t * apq; A[12 * p + q] = 0.0; }
                    else if (lane == q) { A[13 * q] = aqq + t * apq; A[12 * q + p] = 0.0; }
                    else {
                        const double n1 = c * arp - s * arq, n2 = s * arp + c * arq;
                        A[12 * lane + p] = n1; A[12 * p + lane] = n1;
                        A[12 * lane + q] = n2; A[12 * q + lane] = n2;
                    }
                }
            }
    }
}

// h = [M | m] (rows of 4) -> the six parameters (omega, T) of the pose R = M (M^T M)^(-1/2), t = m / s, T = -R^T t
__device__ __forceinline__ void resect_pose_from_h(const double (&h)[12], double (&prm)[6]) {
    double M[9], m[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = h[4 * i + j];
        m[i] = h[4 * i + 3];
    }
    const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
    if (det < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = -M[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = -m[k];
    }
    double a[6], w[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) a[sym<3>(i, j)] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
    jacobi_sweeps<3>(a, w);
    const double s0 = sqrt(a[0]), s1 = sqrt(a[3]), s2 = sqrt(a[5]);
    const double i0 = 1.0 / s0, i1 = 1.0 / s1, i2 = 1.0 / s2;
    const double scale = (s0 + s1 + s2) / 3.0;
    double Bi[9];                                                // (M^T M)^(-1/2) = W diag(1 / sigma) W^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Bi[3 * i + j] = w[3 * i] * i0 * w[3 * j] + w[3 * i + 1] * i1 * w[3 * j + 1] + w[3 * i + 2] * i2 * w[3 * j + 2];
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = M[3 * i] * Bi[j] + M[3 * i + 1] * Bi[3 + j] + M[3 * i + 2] * Bi[6 + j];
    const double t0 = m[0] / scale, t1 = m[1] / scale, t2 = m[2] / scale;
    prm[3] = -(R[0] * t0 + R[3] * t1 + R[6] * t2);
    prm[4] = -(R[1] * t0 + R[4] * t1 + R[7] * t2);
    prm[5] = -(R[2] * t0 + R[5] * t1 + R[8] * t2);
    // rotation vector through the quaternion, the largest component first (angles near 0 and near pi are both safe)
    const double tr = R[0] + R[4] + R[8];
    double qw, qx, qy, qz;
    if (tr > 0.0) {
        const double s = sqrt(tr + 1.0) * 2.0;
        qw = 0.25 * s; qx = (R[7] - R[5]) / s; qy = (R[2] - R[6]) / s; qz = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
        qw = (R[7] - R[5]) / s; qx = 0.25 * s; qy = (R[1] + R[3]) / s; qz = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
        qw = (R[2] - R[6]) / s; qx = (R[1] + R[3]) / s; qy = 0.25 * s; qz = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
        qw = (R[3] - R[1]) / s; qx = (R[2] + R[6]) / s; qy = (R[5] + R[7]) / s; qz = 0.25 * s;
    }
    if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    const double n = sqrt(qx * qx + qy * qy + qz * qz);
    const double f = n < 1e-12 ? 2.0 : 2.0 * atan2(n, qw) / n;
    prm[0] = qx * f; prm[1] = qy * f; prm[2] = qz * f;
}

template <bool F32>
__global__ __launch_bounds__(kCamThreads) void k_resect(ResectIn in, int C, KMat K, KMat Kinv, ResectOptions opt, ResectOut out) {
    __shared__ double red[kCamWaves * 40];
    __shared__ double redm[kCamWaves];
    __shared__ int redi[kCamWaves];
    __shared__ __align__(16) double row[kCamRow];
    __shared__ double jA[144], jV[144];
    __shared__ int ctl;
    __shared__ double s[28], p[6];                               // thread 0's: the accepted pose and its sums
    const int c = blockIdx.x;
    const int b = in.cam_ptr[c], e = in.cam_ptr[c + 1];
    const double* __restrict__ pts = in.x + 6 * (size_t)C;
    const bool first = threadIdx.x == 0;
    if (first) {
#pragma unroll
        for (int k = 0; k < 6; ++k) p[k] = in.x[6 * (size_t)c + k];
    }
    // what thread 0 reports: the camera of x unless the status becomes OK
    int status = kResNotSelected, views = 0, iters = 0;
    double rms = NAN;
    auto report = [&](bool ok) {
        if (!first) return;
#pragma unroll
        for (int k = 0; k < 6; ++k) out.cam[6 * (size_t)c + k] = ok ? p[k] : in.x[6 * (size_t)c + k];
        out.status[c] = status; out.views[c] = views; out.iters[c] = iters; out.rms[c] = rms;
        out.ok_part[c] = ok ? 1 : 0;
    };
    if (in.select != nullptr && !in.select[c]) { report(false); return; }          // (uniform over the workgroup)
    const int need = max(opt.min_views, opt.start == 0 ? 6 : 3);
    if (first) { row[kCamTab] = 0.0; ctl = 1; }
    if (opt.start == 0) {
        {
            double v[40];
            resect_dlt_pass<F32>(in, pts, b, e, Kinv, v, views, red, redi);
            if (first) {
                // A^T A = [[S, 0, -S_u], [0, S, -S_v], [-S_u, -S_v, S_w]], V = I
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int q = sym<4>(i, j);
                        jA[12 * i + j] = v[q];           jA[12 * i + 4 + j] = 0.0;        jA[12 * i + 8 + j] = -v[10 + q];
                        jA[12 * (4 + i) + j] = 0.0;      jA[12 * (4 + i) + 4 + j] = v[q]; jA[12 * (4 + i) + 8 + j] = -v[20 + q];
                        jA[12 * (8 + i) + j] = -v[10 + q]; jA[12 * (8 + i) + 4 + j] = -v[20 + q]; jA[12 * (8 + i) + 8 + j] = v[30 + q];
                    }
                for (int k = 0; k < 144; ++k) jV[k] = (k % 13) == 0 ? 1.0 : 0.0;
            }
        }
        if (threadIdx.x < 64) {                                  // wave 0: thread 0's stores above are its own
            resect_jacobi12(jA, jV, (int)threadIdx.x);
            if (first) {
                status = kResFewViews;
                bool go = views >= need;
                if (go) {
                    status = kResDegenerate;
                    const volatile double* vA = jA;
                    const volatile double* vV = jV;
                    int lo = 0;
                    double hi = vA[0];
                    for (int k = 1; k < 12; ++k) { if (vA[13 * k] < vA[13 * lo]) lo = k; hi = fmax(hi, vA[13 * k]); }
                    double second = INFINITY;
                    for (int k = 0; k < 12; ++k) if (k != lo) second = fmin(second, vA[13 * k]);
                    go = second > 1e-12 * hi;                    // (false for a NaN as well)
                    double hv[12];
#pragma unroll
                    for (int k = 0; k < 12; ++k) hv[k] = vV[12 * k + lo];
                    resect_pose_from_h(hv, p);
                    double sum = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) sum += fabs(p[k]);
                    go = go && sum < INFINITY;
                    if (go) cam_row_values(p, row);
                }
                ctl = go ? 1 : 0;
            }
        }
    } else if (first) {
        cam_row_values(p, row);
    }
    __syncthreads();
    if (!ctl) { report(false); return; }
    // refinement: thread 0 holds the accepted pose p, its sums s and smallest depth, the damping and the step on trial
    // (the accepted sums live in LDS: with the trial's 28 in registers beside the 6x6 factorisation the kernel spilled)
    double mind = INFINITY, lam = 0.0, d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, dn = 0.0;
    bool have = false;
#pragma unroll 1
    for (;;) {
        double tl[kCamRow];
        {
            const double2* __restrict__ r2 = reinterpret_cast<const double2*>(row);
#pragma unroll
            for (int k = 0; k < kCamRow / 2; ++k) { const double2 q = r2[k]; tl[2 * k] = q.x; tl[2 * k + 1] = q.y; }
        }
        double st[28], mt;
        int used;
        resect_linearise<F32>(in, pts, b, e, K, tl, st, mt, used, red, redm, redi);
        if (first) {
            bool stop = false;
            if (!have) {                                         // the start pose
                have = true;
                views = used;
#pragma unroll
                for (int q = 0; q < 28; ++q) s[q] = st[q];
                mind = mt;
                double sum = fabs(s[0]);
#pragma unroll
                for (int k = 0; k < 6; ++k) sum += fabs(p[k]);
                if (views < need) { status = kResFewViews; stop = true; }
                else if (!(sum < INFINITY)) { status = kResDegenerate; stop = true; }
                else status = kResOk;
            } else {
                ++iters;
                if (st[0] <= s[0]) {                             // (a non-finite trial cost is a rejection)
#pragma unroll
                    for (int k = 0; k < 6; ++k) p[k] += d[k];
#pragma unroll
                    for (int q = 0; q < 28; ++q) s[q] = st[q];
                    mind = mt;
                    lam = gn_damping_after_accept(lam);
                    double pn = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) pn += p[k] * p[k];
                    if (gn_step_below_tol(dn, sqrt(pn), opt.xtol)) stop = true;
                } else {
                    double gd = 0.0, dHd = 0.0;
                    int n = 7;
#pragma unroll
                    for (int a = 0; a < 6; ++a) {
                        gd += s[1 + a] * d[a];
#pragma unroll
                        for (int q = a; q < 6; ++q) { dHd += (q == a ? 1.0 : 2.0) * s[n] * d[a] * d[q]; ++n; }
                    }
                    if (gn_gain_negligible(gd, dHd, s[0])) stop = true;
                    lam = gn_damping_after_reject(lam);
                }
            }
            if (!stop && iters >= opt.max_iter) stop = true;
            if (!stop) {
                double A[6][6], inv[21];
                int n = 7;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int q = a; q < 6; ++q) { A[a][q] = A[q][a] = q == a ? s[n] * (1.0 + lam) : s[n]; ++n; }
                spd6_inverse(A, inv);
                double full[6][6];
                n = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int q = a; q < 6; ++q) { full[a][q] = full[q][a] = inv[n]; ++n; }
                double pn = 0.0;
                dn = 0.0;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    double t = 0.0;
#pragma unroll
                    for (int q = 0; q < 6; ++q) t += full[a][q] * s[1 + q];
                    d[a] = -t;
                    dn += t * t;
                    pn += p[a] * p[a];
                }
                dn = sqrt(dn);
                if (gn_step_below_tol(dn, sqrt(pn), opt.xtol)) stop = true;    // the step on offer is below the tolerance already
                else {
                    double pt[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) pt[k] = p[k] + d[k];
                    cam_row_values(pt, row);
                }
            }
            ctl = stop ? 0 : 1;
        }
        __syncthreads();
        if (!ctl) break;
    }
    if (first && status == kResOk) {
        rms = sqrt(s[0] / (double)views);
        double sum = fabs(rms) + fabs(mind);
#pragma unroll
        for (int k = 0; k < 6; ++k) sum += fabs(p[k]);
        if (!(sum < INFINITY)) status = kResDegenerate;
        else if (mind <= opt.min_depth) status = kResBehind;
        else if (rms > opt.max_rms) status = kResHighError;
    }
    report(status == kResOk);
}

// ---------------------------------------------------------------------------------------------
// Two-view geometry (sfmba_fundamental_ransac, sfmba_recover_pose).  A batch of edges (image
// pairs), each a run of used pixel pairs x1 y1 x2 y2 (32 bytes, packed by the host in stored order); nothing of a
// bundle-adjustment problem is read.
// The grid, slots and ties of the RANSAC are the shell's (below); F and H put into it what is written
// once over a model (FundModel, HomogModel: what a model supplies is listed above them); then the finish of an edge:
//   k_fund_ransac, k_homog_ransac   twoview_ransac<M> binds twoview_slice<M>: a wave takes one hypothesis at a time, M::S
//                   sampled pairs (ransac_sample) -> one-scale normalisation, A^T A of the model's eight rows, its smallest
//                   eigenvector by jacobi_lds<9>, M::from_jacobi (F, the reference's estimate_fundamental_matrix: rank 2 by
//                   a 3x3 Jacobi in registers, T2^T F T1; H: T2^-1 Hn T1), then the lanes stride the edge's pairs and count
//                   M::inlier (F: |x2^T F x1| / |(F x1)_xy| < threshold; H: the squared transfer distance in image 2) by
//                   ballot / popcount.
//   k_fund_finish, k_homog_finish   twoview_finish<M>: one workgroup per edge: twoview_verdict (best slot, the mask of that
//                   matrix and the count from it, status; k_ess_finish shares it), then unit norm and sign and the refit
//                   over all inliers (sums by block_sum, the 9x9 Jacobi by wave 0); a model with kRefitMask (H) adds the
//                   mask and count of the refit.
//   k_recover_pose  one workgroup per edge: wave 0 decomposes E into the four (R, t), every pair is triangulated against
//                   each (two-view DLT, smallest_eigenvector4) and counted in front; thread 0 decides; a second pass
//                   writes the winner's points, mask, ray angles and the summed reprojection error.
// No atomics; sums in a fixed order (wave_sum, then the waves in wave order); counts do not depend on the order.
// ---------------------------------------------------------------------------------------------
constexpr int kTwoViewThreads = 256;
constexpr int kTwoViewWaves = 4;
constexpr int kTwoViewLdsPairs = 4096;   // an edge of up to this many used pairs is staged in LDS (128 KiB of the 160)
constexpr int kTwoViewMinSlice = 8;      // fewest hypotheses of a workgroup's slice (two per wave)
constexpr int kRansacHead = 3;           // doubles of a slot before its payload: count, h, one auxiliary integer (the shell, below)
constexpr int kTwoViewSlot = kRansacHead + 9;    // doubles of a slot: the payload is F or H
constexpr int kJacobiLdsSweeps = 30;     // cap of the sweeps of jacobi_lds (a 9x9 converges in 5..9)
constexpr int kFundOk = 0, kFundFewPairs = 1, kFundDegenerate = 2;
constexpr int kPoseOk = 0, kPoseFewPairs = 1, kPoseDegenerate = 2, kPoseTie = 3;

// resect_jacobi12 for any N <= 64: cyclic Jacobi on the symmetric N x N matrix A (full storage, LDS), eigenvectors in the
// columns of V, by ONE wave, lane r < N owning row r of both.  (k_resect keeps resect_jacobi12 as it is written.)
template <int N>
__device__ __forceinline__ void jacobi_lds(volatile double* A, volatile double* V, int lane) {
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiLdsSweeps; ++sweep) {
        double off = 0.0, dia = 0.0;
        if (lane < N) {
            for (int j = lane + 1; j < N; ++j) off += fabs(A[N * lane + j]);
            dia = fabs(A[(N + 1) * lane]);
        }
        off = wave_sum(off);
        dia = wave_sum(dia);
        if (!(off > 1e-40 * dia)) break;                         // (a NaN ends the loop too)
#pragma unroll 1
        for (int p = 0; p < N - 1; ++p)
#pragma unroll 1
            for (int q = p + 1; q < N; ++q) {
                const double app = A[(N + 1) * p], aqq = A[(N + 1) * q], apq = A[N * p + q];
                double t, c, s;
                jacobi_cs(app, aqq, apq, t, c, s);
                double arp = 0.0, arq = 0.0, vrp = 0.0, vrq = 0.0;
                if (lane < N) { arp = A[N * lane + p]; arq = A[N * lane + q]; vrp = V[N * lane + p]; vrq = V[N * lane + q]; }
                if (lane < N) {
                    V[N * lane + p] = c * vrp - s * vrq;
                    V[N * lane + q] = s * vrp + c * vrq;
                    if (lane == p) { A[(N + 1) * p] = app - t * apq; A[N * p + q] = 0.0; }
                    else if (lane == q) { A[(N + 1) * q] = aqq + t * apq; A[N * q + p] = 0.0; }
                    else {
                        const double n1 = c * arp - s * arq, n2 = s * arp + c * arq;
                        A[N * lane + p] = n1; A[N * p + lane] = n1;
                        A[N * lane + q] = n2; A[N * q + lane] = n2;
                    }
                }
            }
    }
}

// the counter-based sample rule (include/sfmba.h): S distinct positions among n >= S, a function of (seed, e, h) alone
__host__ __device__ __forceinline__ unsigned long long twoview_mix(unsigned long long z) {
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}
// (S = 8 for F, S = 4 for a homography)
template <int S>
__device__ __forceinline__ void twoview_draw(unsigned long long seed, unsigned e, unsigned h, int n, int (&idx)[S]) {
    const unsigned long long key = twoview_mix(seed ^ twoview_mix(((unsigned long long)e << 32) | (unsigned long long)h));
    int srt[S];                                                  // the earlier choices, ascending
#pragma unroll
    for (int j = 0; j < S; ++j) {
        int k = (int)(twoview_mix(key + (unsigned long long)(j + 1) * 0x9e3779b97f4a7c15ull) % (unsigned long long)(n - j));
#pragma unroll
        for (int i = 0; i < j; ++i) if (k >= srt[i]) ++k;
        idx[j] = k;
        int v = k;
#pragma unroll
        for (int i = 0; i < j; ++i) if (v < srt[i]) { const int t = srt[i]; srt[i] = v; v = t; }
        srt[j] = v;
    }
}

// The S positions of hypothesis h of item b (an edge, a camera) among its n >= S entries: the caller's (samples
// [batch][H][S]; false when one lies outside 0 .. n - 1 or two are equal) or, samples null, drawn by twoview_draw
template <int S>
__device__ __forceinline__ bool ransac_sample(const int* __restrict__ samples, int b, int H, int h, int n, unsigned long long seed,
                                              int (&idx)[S]) {
    bool valid = true;
    if (samples != nullptr) {
        const int* __restrict__ sp = samples + ((size_t)b * (size_t)H + (size_t)h) * S;
#pragma unroll
        for (int j = 0; j < S; ++j) { idx[j] = sp[j]; valid = valid && idx[j] >= 0 && idx[j] < n; }
#pragma unroll
        for (int j = 1; j < S; ++j)
#pragma unroll
            for (int i = 0; i < j; ++i) valid = valid && idx[i] != idx[j];
    } else {
        twoview_draw(seed, (unsigned)b, (unsigned)h, n, idx);
    }
    return valid;
}

// ---- The shell of the two-view RANSAC kernels (F, H, E).  A grid over (edge, slice of its H hypotheses): a workgroup leaves
// the best of the hypotheses [h0, h1) of one edge in a slot of its own: count, h, one auxiliary integer (E: the root), P doubles.
// THE RULE every caller-visible tie rests on: the largest count wins, among equal counts the lowest h.  A slice meets its
// hypotheses in ascending h and replaces the wave's best only by a strictly larger count; waves: ransac_better; slots ascend
// in h, so the first of equal counts is the one (ransac_best_slot).  A family supplies a slice function (twoview_slice<M>,
// ess_slice: untouched by the shell, their loops are sensitive to anything live across them) and a kernel that binds it:
// ransac_block; too few pairs: ransac_no_hypothesis per array, ransac_empty_slot; else the slice over staged or global pairs,
// the wave's best packed into a RansacBest, ransac_store.
constexpr int kRansacNone = -1;          // count and auxiliary integer of no hypothesis

template <int P> struct RansacBest { int count = kRansacNone, h = 0x7fffffff, aux = kRansacNone; double v[P] = {}; };

__device__ __forceinline__ bool ransac_better(double count, double h, double than_count, double than_h) {
    return count > than_count || (count == than_count && h < than_h);
}

struct RansacBlock { int item, h0, h1; };
__device__ __forceinline__ RansacBlock ransac_block(int H, int hs, int n_slices) {
    const int item = blockIdx.x / n_slices, sl = blockIdx.x - item * n_slices;
    return RansacBlock{item, sl * hs, min(H, sl * hs + hs)};
}

// -1 into the workgroup's part of a per-hypothesis array [batch][H] (null: not asked for)
__device__ __forceinline__ void ransac_no_hypothesis(const RansacBlock& rb, int H, int* hyp) {
    if (hyp != nullptr)
        for (int h = rb.h0 + (int)threadIdx.x; h < rb.h1; h += kTwoViewThreads) hyp[(size_t)rb.item * (size_t)H + (size_t)h] = -1;
}

template <int P>
__device__ __forceinline__ void ransac_empty_slot(double* slots) {
    constexpr int kSlot = kRansacHead + P;
    if (threadIdx.x < kSlot) slots[(size_t)blockIdx.x * kSlot + threadIdx.x] = threadIdx.x == 0 || threadIdx.x == 2 ? (double)kRansacNone : 0.0;
}

// the waves' bests through LDS into the workgroup's slot: thread t stores entry t of the winner
template <int P>
__device__ __forceinline__ void ransac_store(const RansacBest<P>& best, double* slots) {
    constexpr int kSlot = kRansacHead + P;
    __shared__ double wbest[kTwoViewWaves][kSlot];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        wbest[w][0] = (double)best.count; wbest[w][1] = (double)best.h; wbest[w][2] = (double)best.aux;
#pragma unroll
        for (int k = 0; k < P; ++k) wbest[w][kRansacHead + k] = best.v[k];
    }
    __syncthreads();
    if (threadIdx.x < kSlot) {
        int win = 0;
        for (int k = 1; k < kTwoViewWaves; ++k)
            if (ransac_better(wbest[k][0], wbest[k][1], wbest[win][0], wbest[win][1])) win = k;
        slots[(size_t)blockIdx.x * kSlot + threadIdx.x] = wbest[win][threadIdx.x];
    }
}

// the winner among the n_slices slots of an item (see THE RULE)
template <int P>
__device__ __forceinline__ const double* ransac_best_slot(const double* slots, int item, int n_slices) {
    constexpr int kSlot = kRansacHead + P;
    const double* __restrict__ sl = slots + (size_t)item * (size_t)n_slices * kSlot;
    int best = 0;
    for (int k = 1; k < n_slices; ++k)
        if (sl[(size_t)k * kSlot] > sl[(size_t)best * kSlot]) best = k;
    return sl + (size_t)best * kSlot;
}

// ---- The model of a two-view RANSAC: what twoview_slice, twoview_verdict, twoview_ata_rows and twoview_finish below ask of
// an estimator.  A model is a 3x3 matrix, the null vector of a 9-column system of normalised pairs:
//   S            pairs of a sample, and the fewest inliers of an estimate
//   kRefitMask   whether the finish also returns the mask and count of the refit (a second mask, a fifth integer per edge)
//   kOk, kFewPairs, kDegenerate   its status values
//   kRows, rows  the rows a normalised pair gives the system (kRows * S = 8).  Pair j of a sample stores row q at
//                S q + j of the wave's R (F: j; H: the four first rows, then the four second rows); the refit adds a
//                pair's rows to the sums of A^T A in the order q = 0, 1
//   from_jacobi after jacobi_lds<9>: the matrix in pixel coordinates, the same on every lane of the calling wave
//   inlier       the one-sided score of a pixel pair against the matrix, strictly below `score` (the host's argument:
//                the threshold for F, its square for H); a non-finite distance is no inlier
constexpr int kHomogOk = 0, kHomogFewPairs = 1, kHomogDegenerate = 2;

// the reference's estimate_fundamental_matrix: eight pairs, a row of construct_matrix_A each, the distance to the epipolar line
struct FundModel {
    static constexpr int S = 8;
    static constexpr bool kRefitMask = false;
    static constexpr int kOk = kFundOk, kFewPairs = kFundFewPairs, kDegenerate = kFundDegenerate;

    static constexpr int kRows = 1;
    static __device__ __forceinline__ void rows(double x1, double y1, double x2, double y2, double (&r)[1][9]) {
        r[0][0] = x2 * x1; r[0][1] = x2 * y1; r[0][2] = x2; r[0][3] = y2 * x1; r[0][4] = y2 * y1; r[0][5] = y2; r[0][6] = x1; r[0][7] = y1; r[0][8] = 1.0;
    }
    // f = the eigenvector of the smallest eigenvalue, rank 2 forced by removing the smallest singular direction
    // (F <- F - (F v3) v3^T, v3 the smallest eigenvector of F^T F), then T2^T F T1 with T = [[1/s, 0, -mx/s],
    // [0, 1/s, -my/s], [0, 0, 1]]
    static __device__ __forceinline__ void from_jacobi(const volatile double* A, const volatile double* V, double m1x, double m1y,
                                                       double s1, double m2x, double m2y, double s2, double (&F)[9]) {
        int lo = 0;
        double least = A[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) { const double d = A[10 * k]; if (d < least) { least = d; lo = k; } }
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = V[9 * k + lo];
        double a[6], w[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) a[sym<3>(i, j)] = F[i] * F[j] + F[3 + i] * F[3 + j] + F[6 + i] * F[6 + j];
        jacobi_sweeps<3>(a, w);
        // (the columns as values behind an empty statement: without it the compiler selects an ADDRESS by the comparisons
        // below and reads the column from scratch memory)
        double w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4], w5 = w[5], w6 = w[6], w7 = w[7], w8 = w[8];
        asm volatile("" : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3), "+v"(w4), "+v"(w5), "+v"(w6), "+v"(w7), "+v"(w8));
        double l3 = a[0], v0 = w0, v1 = w3, v2 = w6;
        if (a[3] < l3) { l3 = a[3]; v0 = w1; v1 = w4; v2 = w7; }
        if (a[5] < l3) { l3 = a[5]; v0 = w2; v1 = w5; v2 = w8; }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double fv = F[3 * i] * v0 + F[3 * i + 1] * v1 + F[3 * i + 2] * v2;
            F[3 * i] -= fv * v0; F[3 * i + 1] -= fv * v1; F[3 * i + 2] -= fv * v2;
        }
        const double a1 = 1.0 / s1, b1 = -m1x / s1, c1 = -m1y / s1, a2 = 1.0 / s2, b2 = -m2x / s2, c2 = -m2y / s2;
        double G[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            G[3 * i] = F[3 * i] * a1; G[3 * i + 1] = F[3 * i + 1] * a1;
            G[3 * i + 2] = F[3 * i] * b1 + F[3 * i + 1] * c1 + F[3 * i + 2];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            F[j] = a2 * G[j]; F[3 + j] = a2 * G[3 + j];
            F[6 + j] = b2 * G[j] + c2 * G[3 + j] + G[6 + j];
        }
    }
    // the reference's score: the distance of x2 from the line F x1 (NaN compares false; +inf < thr is false)
    static __device__ __forceinline__ bool inlier(const double (&F)[9], double x1, double y1, double x2, double y2, double thr) {
        const double l0 = F[0] * x1 + F[1] * y1 + F[2], l1 = F[3] * x1 + F[4] * y1 + F[5], l2 = F[6] * x1 + F[7] * y1 + F[8];
        const double d = fabs(x2 * l0 + y2 * l1 + l2) / sqrt(l0 * l0 + l1 * l1);
        return d < thr && d < INFINITY;
    }
};

// a four-pair DLT homography x2 ~ H x1 (sfmba_homography_ransac): two rows a pair, the transfer distance in image 2
struct HomogModel {
    static constexpr int S = 4;
    static constexpr bool kRefitMask = true;
    static constexpr int kOk = kHomogOk, kFewPairs = kHomogFewPairs, kDegenerate = kHomogDegenerate;

    static constexpr int kRows = 2;
    static __device__ __forceinline__ void rows(double x, double y, double u, double v, double (&r)[2][9]) {
        r[0][0] = -x; r[0][1] = -y; r[0][2] = -1.0; r[0][3] = 0.0; r[0][4] = 0.0; r[0][5] = 0.0; r[0][6] = u * x; r[0][7] = u * y; r[0][8] = u;
        r[1][0] = 0.0; r[1][1] = 0.0; r[1][2] = 0.0; r[1][3] = -x; r[1][4] = -y; r[1][5] = -1.0; r[1][6] = v * x; r[1][7] = v * y; r[1][8] = v;
    }
    // Hn = the eigenvector of the smallest eigenvalue, then T2^-1 Hn T1 with T1 = [[1/s1, 0, -m1x/s1], [0, 1/s1, -m1y/s1],
    // [0, 0, 1]] and T2^-1 = [[s2, 0, m2x], [0, s2, m2y], [0, 0, 1]]
    static __device__ __forceinline__ void from_jacobi(const volatile double* A, const volatile double* V, double m1x, double m1y,
                                                       double s1, double m2x, double m2y, double s2, double (&Hm)[9]) {
        int lo = 0;
        double least = A[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) { const double d = A[10 * k]; if (d < least) { least = d; lo = k; } }
        double Hn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Hn[k] = V[9 * k + lo];
        const double a1 = 1.0 / s1, b1 = -m1x / s1, c1 = -m1y / s1;
        double G[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            G[3 * i] = Hn[3 * i] * a1; G[3 * i + 1] = Hn[3 * i + 1] * a1;
            G[3 * i + 2] = Hn[3 * i] * b1 + Hn[3 * i + 1] * c1 + Hn[3 * i + 2];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Hm[j] = s2 * G[j] + m2x * G[6 + j]; Hm[3 + j] = s2 * G[3 + j] + m2y * G[6 + j];
            Hm[6 + j] = G[6 + j];
        }
    }
    // the squared distance of x2 from the transferred H x1 (NaN compares false; +inf < thr2 is false)
    static __device__ __forceinline__ bool inlier(const double (&Hm)[9], double x1, double y1, double x2, double y2, double thr2) {
        const double q0 = Hm[0] * x1 + Hm[1] * y1 + Hm[2], q1 = Hm[3] * x1 + Hm[4] * y1 + Hm[5], q2 = Hm[6] * x1 + Hm[7] * y1 + Hm[8];
        const double dx = q0 / q2 - x2, dy = q1 / q2 - y2;
        const double d2 = dx * dx + dy * dy;
        return d2 < thr2 && d2 < INFINITY;
    }
};

// unit Frobenius norm, the entry of largest magnitude (the first of equals) positive
__device__ __forceinline__ void fund_unit(double (&F)[9]) {
    double ss = 0.0, big = 0.0, sgn = 1.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) { ss += F[k] * F[k]; if (fabs(F[k]) > big) { big = fabs(F[k]); sgn = F[k] < 0.0 ? -1.0 : 1.0; } }
    const double nrm = sqrt(ss) * sgn;
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = F[k] / nrm;
}

struct FundIn {
    const double* __restrict__ pairs;            // [M_used][4] x1 y1 x2 y2
    const int* __restrict__ uptr;                // [n_edges + 1] runs of used pairs
    const int* __restrict__ samples;             // [n_edges][H][S] positions among the used pairs, or null: drawn
};

// the hypotheses h0 + w, h0 + w + 4, ... < h1 of edge e by wave w; P: the edge's pairs (LDS or global)
template <class M>
__device__ __forceinline__ void twoview_slice(const double* P, const int* __restrict__ samples, int e, int n, int H, int h0, int h1,
                                              unsigned long long seed, double score, volatile double* A, volatile double* V,
                                              volatile double* R, int* __restrict__ hyp, int& bc, int& bh, double (&bM)[9]) {
    constexpr int S = M::S;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double2* __restrict__ P2 = reinterpret_cast<const double2*>(P);
    bc = -1; bh = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 9; ++k) bM[k] = 0.0;
#pragma unroll 1
    for (int h = h0 + w; h < h1; h += kTwoViewWaves) {
        int idx[S];
        if (!ransac_sample(samples, e, H, h, n, seed, idx)) {    // (uniform over the wave)
            if (lane == 0 && hyp != nullptr) hyp[(size_t)e * (size_t)H + (size_t)h] = -1;
            continue;
        }
        double x1[S], y1[S], x2[S], y2[S];
        double m1x = 0.0, m1y = 0.0, m2x = 0.0, m2y = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const double2 qa = P2[2 * idx[j]], qb = P2[2 * idx[j] + 1];
            x1[j] = qa.x; y1[j] = qa.y; x2[j] = qb.x; y2[j] = qb.y;
            m1x += qa.x; m1y += qa.y; m2x += qb.x; m2y += qb.y;
        }
        const double g1 = (m1x + m1y) / (2.0 * S), g2 = (m2x + m2y) / (2.0 * S);   // np.std: about the mean of all 2 S coordinates
        m1x /= (double)S; m1y /= (double)S; m2x /= (double)S; m2y /= (double)S;
        double q1 = 0.0, q2 = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            q1 += (x1[j] - g1) * (x1[j] - g1) + (y1[j] - g1) * (y1[j] - g1);
            q2 += (x2[j] - g2) * (x2[j] - g2) + (y2[j] - g2) * (y2[j] - g2);
        }
        const double s1 = sqrt(q1 / (2.0 * S)), s2 = sqrt(q2 / (2.0 * S));
        // the eight rows through LDS (lane 0 stores them), then lane i < 9 sums row i of A^T A over the rows 0..7
#pragma unroll
        for (int j = 0; j < S; ++j) {
            double r[M::kRows][9];
            M::rows((x1[j] - m1x) / s1, (y1[j] - m1y) / s1, (x2[j] - m2x) / s2, (y2[j] - m2y) / s2, r);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i)
#pragma unroll
                    for (int q = 0; q < M::kRows; ++q) R[9 * (S * q + j) + i] = r[q][i];
            }
        }
        if (lane < 9) {
            double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const double ri = R[9 * j + lane];
#pragma unroll
                for (int c = 0; c < 9; ++c) acc[c] += ri * R[9 * j + c];
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) { A[9 * lane + c] = acc[c]; V[9 * lane + c] = c == lane ? 1.0 : 0.0; }
        }
        jacobi_lds<9>(A, V, lane);
        double Mh[9];
        M::from_jacobi(A, V, m1x, m1y, s1, m2x, m2y, s2, Mh);
        int cnt = 0;
#pragma unroll 1
        for (int k0 = 0; k0 < n; k0 += 64) {                     // uniform over the wave: the ballot needs every lane
            const int k = k0 + lane;
            bool inl = false;
            if (k < n) { const double2 qa = P2[2 * k], qb = P2[2 * k + 1]; inl = M::inlier(Mh, qa.x, qa.y, qb.x, qb.y, score); }
            cnt += __popcll(__ballot(inl));
        }
        if (lane == 0 && hyp != nullptr) hyp[(size_t)e * (size_t)H + (size_t)h] = cnt;
        if (cnt > bc) {                                          // (h ascends: the lowest h of equal counts stays)
            bc = cnt; bh = h;
#pragma unroll
            for (int k = 0; k < 9; ++k) bM[k] = Mh[k];
        }
    }
}

// The F / H binding of the shell.  (This body and twoview_finish take plain pointers: the kernels' own
// parameters carry __restrict__, and saying it again here moves their code away from what it was as one function)
template <class M>
__device__ __forceinline__ void twoview_ransac(const double* pairs, const int* uptr, const int* samples, int H, int hs, int n_slices,
                                               unsigned long long seed, double score, double* slots, int* hyp) {
    extern __shared__ __align__(16) double smem[];
    __shared__ double jA[kTwoViewWaves][81], jV[kTwoViewWaves][81], jR[kTwoViewWaves][72];
    const RansacBlock rb = ransac_block(H, hs, n_slices);
    const int b = uptr[rb.item], n = uptr[rb.item + 1] - b, w = threadIdx.x >> 6;
    const double* __restrict__ gp = pairs + 4 * (size_t)b;
    if (n < M::S) { ransac_no_hypothesis(rb, H, hyp); ransac_empty_slot<9>(slots); return; }    // (uniform) FEW_PAIRS: no hypothesis
    int bc, bh;
    double bM[9];
    if (n <= kTwoViewLdsPairs) {
        stage_table(gp, 4 * n, smem);
        twoview_slice<M>(smem, samples, rb.item, n, H, rb.h0, rb.h1, seed, score, jA[w], jV[w], jR[w], hyp, bc, bh, bM);
    } else {
        twoview_slice<M>(gp, samples, rb.item, n, H, rb.h0, rb.h1, seed, score, jA[w], jV[w], jR[w], hyp, bc, bh, bM);
    }
    RansacBest<9> best{bc, bh};
#pragma unroll
    for (int k = 0; k < 9; ++k) best.v[k] = bM[k];
    ransac_store(best, slots);
}

// rows I0 .. I1 - 1 of the upper triangle of A^T A over the pairs of the mask mk (its own stores), thread t taking pairs t, t + 256, ...; thread 0
// stores them (and their mirror) into A
template <class M, int I0, int I1>
__device__ __forceinline__ void twoview_ata_rows(const double2* __restrict__ P2, int n, const unsigned char* mk, double m1x,
                                                 double m1y, double s1, double m2x, double m2y, double s2, double* red, double* A) {
    constexpr int NS = sym<9>(I1 - 1, 8) - sym<9>(I0, I0) + 1, Q0 = sym<9>(I0, I0);
    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;
#pragma unroll 1
    for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
        const double2 qa = P2[2 * k], qb = P2[2 * k + 1];
        if (!mk[k]) continue;
        double r[M::kRows][9];
        M::rows((qa.x - m1x) / s1, (qa.y - m1y) / s1, (qb.x - m2x) / s2, (qb.y - m2y) / s2, r);
#pragma unroll
        for (int i = I0; i < I1; ++i)
#pragma unroll
            for (int c = i; c < 9; ++c)
#pragma unroll
                for (int q = 0; q < M::kRows; ++q) s[sym<9>(i, c) - Q0] += r[q][i] * r[q][c];
    }
    block_sum<NS>(s, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = I0; i < I1; ++i)
#pragma unroll
            for (int c = i; c < 9; ++c) { A[9 * i + c] = s[sym<9>(i, c) - Q0]; A[9 * c + i] = s[sym<9>(i, c) - Q0]; }
    }
}

// The verdict of an edge, the first half of its finish kernel: the best of its slots, the mask of that slot's matrix (the
// first nine doubles of the payload) and the count FROM that mask, status, success, oi[0..3] = inliers, best h, status,
// success (with M::kRefitMask the refit's mask and count oi[4] start as copies: refit = 0 and DEGENERATE leave them so).  Of a
// model it asks S, the status values, kRefitMask and inlier.
struct TwoViewVerdict { int status, cnt, aux; };
template <class M, int P>
__device__ __forceinline__ TwoViewVerdict twoview_verdict(const double2* P2, int e, size_t b, int n, int n_slices, double score,
                                                          double confidence, const double* slots, unsigned char* omask,
                                                          unsigned char* orefit_mask, int* oi, double (&pay)[P]) {
    __shared__ double red[kTwoViewWaves];
    __shared__ double sp[P];
    __shared__ int ctl[4];                                       // status, best h, auxiliary integer, count
    const bool first = threadIdx.x == 0;
    if (first) {
        const double* __restrict__ bs = ransac_best_slot<P>(slots, e, n_slices);
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) { sp[k] = bs[kRansacHead + k]; sum += fabs(bs[kRansacHead + k]); }
        ctl[0] = n < M::S ? M::kFewPairs : (sum < INFINITY ? M::kOk : M::kDegenerate);
        ctl[1] = bs[0] >= 0.0 ? (int)bs[1] : -1;                 // (-1: no valid sample in any slot)
        ctl[2] = bs[0] >= 0.0 ? (int)bs[2] : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < P; ++k) pay[k] = sp[k];
    if (ctl[0] == M::kFewPairs) {                                // (uniform over the workgroup)
        for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
            omask[b + k] = 0;
            if constexpr (M::kRefitMask) orefit_mask[b + k] = 0;
        }
        if (first) {
            oi[0] = 0; oi[1] = -1; oi[2] = M::kFewPairs; oi[3] = 0;
            if constexpr (M::kRefitMask) oi[4] = 0;
        }
        return TwoViewVerdict{M::kFewPairs, 0, -1};
    }
    // edge_inliers, edge_success, the status and a refit all rest on this one evaluation (the count in the slot came from another
    // copy of the expression, which the compiler may have contracted differently for a pair within an ulp of the threshold)
    double Mb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Mb[k] = pay[k];
    double c[1] = {0.0};
    for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
        const double2 qa = P2[2 * k], qb = P2[2 * k + 1];
        const bool inl = ctl[1] >= 0 && M::inlier(Mb, qa.x, qa.y, qb.x, qb.y, score);
        omask[b + k] = inl ? 1 : 0;
        if constexpr (M::kRefitMask) orefit_mask[b + k] = inl ? 1 : 0;
        c[0] += inl ? 1.0 : 0.0;
    }
    block_sum<1>(c, red);
    if (first) {
        const int cnt = (int)c[0];
        if (ctl[0] == M::kOk && cnt < M::S) ctl[0] = M::kDegenerate;
        ctl[3] = cnt;
        // (DEGENERATE still reports the count, h and mask of its best hypothesis; only the matrix is withheld)
        oi[0] = cnt; oi[1] = ctl[1]; oi[2] = ctl[0];
        oi[3] = (ctl[1] >= 0 && (double)cnt / (double)n >= confidence) ? 1 : 0;
        if constexpr (M::kRefitMask) oi[4] = cnt;
    }
    __syncthreads();
    return TwoViewVerdict{ctl[0], ctl[3], ctl[2]};
}

// One workgroup per edge: the verdict, the matrix with unit norm and sign, the refit, with M::kRefitMask its mask and count.
// oM, oM_refit [E][9]; omask, orefit_mask [M_used]; oints [E][4 or 5] inliers, best h, status, success, refit inliers.
template <class M>
__device__ __forceinline__ void twoview_finish(const double* pairs, const int* uptr, int n_slices, double score, double confidence,
                                               int refit, const double* slots, double* oM, double* oM_refit, unsigned char* omask,
                                               unsigned char* orefit_mask, int* oints) {
    __shared__ double red[kTwoViewWaves * 18];
    __shared__ double jA[81], jV[81];
    __shared__ double sM[9], sm[8];
    const int e = blockIdx.x;
    const int b = uptr[e], n = uptr[e + 1] - b;
    const bool first = threadIdx.x == 0;
    const double2* __restrict__ P2 = reinterpret_cast<const double2*>(pairs + 4 * (size_t)b);
    int* __restrict__ oi = oints + (M::kRefitMask ? 5 : 4) * (size_t)e;
    const unsigned char* mk = omask + (size_t)b;                 // a thread reads back only what it stored itself
    double Mb[9];
    const TwoViewVerdict vd = twoview_verdict<M>(P2, e, (size_t)b, n, n_slices, score, confidence, slots, omask, orefit_mask, oi, Mb);
    if (vd.status != M::kOk) {
        if (threadIdx.x < 9) { oM[9 * (size_t)e + threadIdx.x] = 0.0; oM_refit[9 * (size_t)e + threadIdx.x] = 0.0; }
        return;
    }
    double Mu[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Mu[k] = Mb[k];
    fund_unit(Mu);
    if (first) {
#pragma unroll
        for (int k = 0; k < 9; ++k) oM[9 * (size_t)e + k] = Mu[k];
    }
    if (!refit) {
        if (first) {
#pragma unroll
            for (int k = 0; k < 9; ++k) oM_refit[9 * (size_t)e + k] = Mu[k];
        }
        return;
    }
    // the same estimate over the cnt >= S inliers: thread t takes pairs t, t + 256, ...
    {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
            const double2 qa = P2[2 * k], qb = P2[2 * k + 1];
            if (mk[k]) { v[0] += qa.x; v[1] += qa.y; v[2] += qb.x; v[3] += qb.y; }
        }
        block_sum<4>(v, red);
        if (first) {
            const double c = (double)vd.cnt;
            sm[0] = v[0] / c; sm[1] = v[1] / c; sm[2] = v[2] / c; sm[3] = v[3] / c;
            sm[4] = (v[0] + v[1]) / (2.0 * c); sm[5] = (v[2] + v[3]) / (2.0 * c);
        }
        __syncthreads();
    }
    const double m1x = sm[0], m1y = sm[1], m2x = sm[2], m2y = sm[3];
    {
        const double g1 = sm[4], g2 = sm[5];
        double v[2] = {0.0, 0.0};
        for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
            const double2 qa = P2[2 * k], qb = P2[2 * k + 1];
            if (mk[k]) {
                v[0] += (qa.x - g1) * (qa.x - g1) + (qa.y - g1) * (qa.y - g1);
                v[1] += (qb.x - g2) * (qb.x - g2) + (qb.y - g2) * (qb.y - g2);
            }
        }
        block_sum<2>(v, red);
        if (first) { sm[6] = sqrt(v[0] / (2.0 * (double)vd.cnt)); sm[7] = sqrt(v[1] / (2.0 * (double)vd.cnt)); }
        __syncthreads();
    }
    const double s1 = sm[6], s2 = sm[7];
    // the 45 sums in three passes (rows 0-1, 2-4, 5-8 of the upper triangle): all of them at once in registers spilled
    twoview_ata_rows<M, 0, 2>(P2, n, mk, m1x, m1y, s1, m2x, m2y, s2, red, jA);
    twoview_ata_rows<M, 2, 5>(P2, n, mk, m1x, m1y, s1, m2x, m2y, s2, red, jA);
    twoview_ata_rows<M, 5, 9>(P2, n, mk, m1x, m1y, s1, m2x, m2y, s2, red, jA);
    if (first)
        for (int k = 0; k < 81; ++k) jV[k] = (k % 10) == 0 ? 1.0 : 0.0;
    if (threadIdx.x < 64) {                                      // wave 0: thread 0's stores above are its own
        jacobi_lds<9>(jA, jV, (int)threadIdx.x);
        double Mr[9];
        M::from_jacobi(jA, jV, m1x, m1y, s1, m2x, m2y, s2, Mr);
        fund_unit(Mr);
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) sum += fabs(Mr[k]);
        if (first) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const double v = sum < INFINITY ? Mr[k] : Mu[k];
                oM_refit[9 * (size_t)e + k] = v;
                if constexpr (M::kRefitMask) sM[k] = v;
            }
        }
    }
    if constexpr (M::kRefitMask) {
        __syncthreads();
        // refit_mask and its count: the used pairs against the refit as it is returned, the same expression
        double Mr[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Mr[k] = sM[k];
        double c[1] = {0.0};
        for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
            const double2 qa = P2[2 * k], qb = P2[2 * k + 1];
            const bool inl = M::inlier(Mr, qa.x, qa.y, qb.x, qb.y, score);
            orefit_mask[(size_t)b + k] = inl ? 1 : 0;
            c[0] += inl ? 1.0 : 0.0;
        }
        block_sum<1>(c, red);
        if (first) oi[4] = (int)c[0];
    }
}

// ---- the kernels of the two models (their names and arguments are what the host and the profiles know) ----
struct FundOut {
    double* __restrict__ F;                      // [E][9]
    double* __restrict__ F_refit;                // [E][9]
    unsigned char* __restrict__ mask;            // [M_used]
    int* __restrict__ ints;                      // [E][4] inliers, best h, status, success
};
struct HomogOut {
    double* __restrict__ Hm;                     // [E][9]
    double* __restrict__ H_refit;                // [E][9]
    unsigned char* __restrict__ mask;            // [M_used] of the best hypothesis
    unsigned char* __restrict__ refit_mask;      // [M_used] of H_refit
    int* __restrict__ ints;                      // [E][5] inliers, best h, status, success, refit inliers
};

__global__ __launch_bounds__(kTwoViewThreads) void k_fund_ransac(FundIn in, int H, int hs, int n_slices, unsigned long long seed,
                                                                 double thr, double* __restrict__ slots, int* __restrict__ hyp) {
    twoview_ransac<FundModel>(in.pairs, in.uptr, in.samples, H, hs, n_slices, seed, thr, slots, hyp);
}
__global__ __launch_bounds__(kTwoViewThreads) void k_fund_finish(FundIn in, int n_slices, double thr, double confidence, int refit,
                                                                 const double* __restrict__ slots, FundOut out) {
    twoview_finish<FundModel>(in.pairs, in.uptr, n_slices, thr, confidence, refit, slots, out.F, out.F_refit, out.mask, nullptr, out.ints);
}
__global__ __launch_bounds__(kTwoViewThreads) void k_homog_ransac(FundIn in, int H, int hs, int n_slices, unsigned long long seed,
                                                                  double thr2, double* __restrict__ slots, int* __restrict__ hyp) {
    twoview_ransac<HomogModel>(in.pairs, in.uptr, in.samples, H, hs, n_slices, seed, thr2, slots, hyp);
}
__global__ __launch_bounds__(kTwoViewThreads) void k_homog_finish(FundIn in, int n_slices, double thr2, double confidence, int refit,
                                                                  const double* __restrict__ slots, HomogOut out) {
    twoview_finish<HomogModel>(in.pairs, in.uptr, n_slices, thr2, confidence, refit, slots, out.Hm, out.H_refit, out.mask, out.refit_mask,
                               out.ints);
}

// ---- sfmba_essential_ransac (include/sfmba.h): the calibrated model, five pairs a sample ----
// k_ess_ransac   binds ess_slice to the shell, a wave per hypothesis.  A hypothesis: five pairs in camera
//                coordinates (K^-1), A^T A of their FundModel::rows, jacobi_lds<9>, the four eigenvectors of the smallest
//                eigenvalues X Y Z W; the ten cubic constraints on E = xX + yY + zZ + W, one coefficient per lane and round
//                (200 of them); Gauss-Jordan with partial pivoting, one entry per lane and round; B(z), its cofactor
//                polynomials and det B(z) by lanes over the coefficients; every real root of det B(z) by the tower of its
//                derivatives (ess_real_roots), an interval per lane; a candidate (E, F_pix) per lane; then ONE pass over
//                the edge's pairs: a lane loads a pair and tests it against every candidate.
// k_ess_finish   one workgroup per edge: twoview_verdict on the slot's F_pix, then the root, the status and E by fund_unit.
// Everything a wave indexes at run time is in its table of kEssWaveDoubles doubles of LDS (the map below): no scratch.
constexpr int kEssS = 5;                  // pairs of a sample, and the fewest inliers of an estimate
constexpr int kEssPayload = 18;           // of a slot (its auxiliary integer: the root): F_pix (9), E (9)
constexpr int kEssSlot = kRansacHead + kEssPayload;
constexpr int kEssMaxRoots = 10;
constexpr int kEssRootIters = 100;        // cap of the safeguarded Newton steps of one root (a bisection at the worst: 2^-100)
constexpr double kEssRankTol = 1e-12;     // a sample's A^T A has rank 5 when its fifth-smallest eigenvalue is above this times the largest
constexpr int kEssOk = 0, kEssFewPairs = 1, kEssDegenerate = 2;
// a wave's table, in doubles
constexpr int kEssOffA = 0;               // [9][9] A^T A, its diagonal the eigenvalues after jacobi_lds
constexpr int kEssOffV = 81;              // [9][9] eigenvectors in columns
constexpr int kEssOffR = 162;             // [5][9] rows of the sample
constexpr int kEssOffB = 207;             // [4][9] X Y Z W
constexpr int kEssOffSys = 243;           // [10][20] the constraints in Nister's monomial order
constexpr int kEssOffBz = 443;            // [3][3][5] B(z), ascending powers
constexpr int kEssOffP = 488;             // [3][8] the cofactor polynomials of rows 0 and 1
constexpr int kEssOffC = 512;             // [11] det B(z), ascending powers
constexpr int kEssOffG = 523;             // [11] the derivative of the current level
constexpr int kEssOffRoots = 534;         // [2][10] roots of the previous and of the current level
constexpr int kEssOffF = 554;             // [10][9] F_pix of the candidates
constexpr int kEssOffE = 644;             // [10][9] E of the candidates
constexpr int kEssOffM = 736;             // [10][20] the constraints as they were before the elimination (ess_polish)
constexpr int kEssWaveDoubles = 936;
constexpr int kEssPolishSteps = 2;
static_assert(kEssOffE + 9 * kEssMaxRoots <= kEssOffM && kEssOffM + 200 <= kEssWaveDoubles, "a wave's table holds its candidates");
static_assert(sizeof(double) * (4 * kTwoViewLdsPairs + kTwoViewWaves * (kEssWaveDoubles + kEssSlot)) <= 160 * 1024,
              "staged pairs and the waves' tables must fit the LDS of a CU");

// Nister's order x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1 as triples a <= b <= c of
// variable numbers (x y z 1 = 0 1 2 3), six bits a monomial, ten monomials a word
constexpr unsigned long long ess_mono_word(int first) {
    constexpr int mono[20][3] = {{0, 0, 0}, {1, 1, 1}, {0, 0, 1}, {0, 1, 1}, {0, 0, 2}, {0, 0, 3}, {1, 1, 2}, {1, 1, 3}, {0, 1, 2}, {0, 1, 3},
                                 {0, 2, 2}, {0, 2, 3}, {0, 3, 3}, {1, 2, 2}, {1, 2, 3}, {1, 3, 3}, {2, 2, 2}, {2, 2, 3}, {2, 3, 3}, {3, 3, 3}};
    unsigned long long v = 0;
    for (int m = 0; m < 10; ++m)
        v |= (unsigned long long)(mono[first + m][0] | (mono[first + m][1] << 2) | (mono[first + m][2] << 4)) << (6 * m);
    return v;
}
constexpr unsigned long long kEssMonoLo = ess_mono_word(0), kEssMonoHi = ess_mono_word(10);

// (the waves' tables through pointers that say LDS: a volatile access through a generic pointer is a flat one with a 64-bit
// address of its own, and this code has hundreds)
typedef __attribute__((address_space(3))) volatile double EssLds;

// the trilinear forms of the constraints: det(P row 0, Q row 1, R row 2), and entry (i, j) of 2 P Q^T R - tr(P Q^T) R
__device__ __forceinline__ double ess_det3(const EssLds* P, const EssLds* Q, const EssLds* R) {
    return P[0] * (Q[4] * R[8] - Q[5] * R[7]) - P[1] * (Q[3] * R[8] - Q[5] * R[6]) + P[2] * (Q[3] * R[7] - Q[4] * R[6]);
}
__device__ __forceinline__ double ess_trace3(const EssLds* P, const EssLds* Q, const EssLds* R, int i, int j) {
    double acc = 0.0, tr = 0.0;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const double s = P[3 * i] * Q[3 * l] + P[3 * i + 1] * Q[3 * l + 1] + P[3 * i + 2] * Q[3 * l + 2];
        acc += s * R[3 * l + j];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) tr += P[k] * Q[k];
    return 2.0 * acc - tr * R[3 * i + j];
}

// p(x) and p'(x) of the polynomial g of degree L (ascending powers, LDS)
__device__ __forceinline__ void ess_horner(const EssLds* g, int L, double x, double& p, double& dp) {
    p = g[L]; dp = 0.0;
#pragma unroll 1
    for (int j = L - 1; j >= 0; --j) { dp = dp * x + p; p = p * x + g[j]; }
}

// Every real root of c (degree <= 10, ascending powers, in T + kEssOffC) by ONE wave, ascending, into T + kEssOffRoots
// + 10 * half (half = n & 1); -> their number.  The tower of derivatives: level L = 1 .. n takes g = c^(n - L) / (n - L)!, of degree L;
// the roots of level L - 1 are its critical points and cut [-R, R] (R the Cauchy bound of c, which holds every root of
// every derivative) into at most L intervals, on each of which g is monotonic: lane i takes interval i, and a sign change
// is one root, found by Newton steps that a bisection safeguards.  A simple real root is never missed: it lies alone between
// two critical points and changes the sign there.  A critical point that is a root itself (a double root) counts once.
__device__ __forceinline__ int ess_real_roots(EssLds* T, int lane, int& half) {
    const EssLds* c = T + kEssOffC;
    EssLds* g = T + kEssOffG;
    int n = -1;
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k <= 10; ++k) { const double v = c[k]; sum += fabs(v); if (v != 0.0) n = k; }
    half = n & 1;
    if (!(sum < INFINITY) || n < 1) return 0;                   // (uniform over the wave)
    const double cn = c[n];
    double R = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) { const double q = fabs(c[k] / cn); if (k < n && q > R) R = q; }
    R = fmin(1.0 + R, 1e150);
    int m = 0;
#pragma unroll 1
    for (int L = 1; L <= n; ++L) {
        const int k = n - L;
        const EssLds* prev = T + kEssOffRoots + 10 * ((L - 1) & 1);
        EssLds* next = T + kEssOffRoots + 10 * (L & 1);
        if (lane <= L) {                                         // g_j = c_(j + k) binom(j + k, k): exact integers
            double b = 1.0;
            for (int i = 1; i <= k; ++i) b = b * (double)(lane + i) / (double)i;
            g[lane] = c[lane + k] * b;
        }
        bool found = false;
        double root = 0.0;
        if (lane <= m) {
            double a = lane == 0 ? -R : prev[lane - 1], bb = lane == m ? R : prev[lane];
            double fa, fb, d;
            ess_horner(g, L, a, fa, d);
            ess_horner(g, L, bb, fb, d);
            if (fa == 0.0) { found = true; root = a; }           // (its left neighbour leaves it to this interval)
            else if (fb != 0.0 && ((fa < 0.0) != (fb < 0.0)) && fa == fa && fb == fb) {
                const bool neg_a = fa < 0.0;
                double x = 0.5 * a + 0.5 * bb, dxo = bb - a;
                found = true;
#pragma unroll 1
                for (int it = 0; it < kEssRootIters; ++it) {
                    double p, dp;
                    ess_horner(g, L, x, p, dp);
                    if (p == 0.0) break;
                    if ((p < 0.0) == neg_a) a = x; else bb = x;
                    double dx = p / dp, xn = x - dx;
                    if (!(xn > a && xn < bb) || !(fabs(2.0 * dx) < fabs(dxo))) { xn = 0.5 * a + 0.5 * bb; dx = x - xn; }
                    dxo = dx;
                    if (!(xn > a && xn < bb) || xn == x) break;  // the bracket is two neighbouring doubles, or the step is nothing
                    x = xn;
                }
                root = x;
            }
        }
        const unsigned long long have = __ballot(found);
        if (found) next[__popcll(have & ((1ull << lane) - 1ull))] = root;
        m = __popcll(have);
    }
    return m;
}

// The candidate Ec of the wave's table once more, in homogeneous coordinates: v = (<X, Ec>, <Y, Ec>, <Z, Ec>, <W, Ec>) of unit
// length, kEssPolishSteps Gauss-Newton steps on the ten cubics c(v) = 0 with the step kept orthogonal to v,
// (J^T J + v v^T) d = -J^T c, v <- (v + d) / |v + d|; E = v0 X + v1 Y + v2 Z + v3 W.  The chart w = 1 loses digits when the
// solution has a small W part in the basis that the eigensolver happened to return; this form does not.  The same on every
// lane (everything it reads is the wave's own).
__device__ __forceinline__ void ess_polish(const EssLds* T, const EssLds* Ec, double (&Em)[9]) {
    const EssLds* Bs = T + kEssOffB;
    const EssLds* M0 = T + kEssOffM;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { const double ei = Ec[i]; v0 += Bs[i] * ei; v1 += Bs[9 + i] * ei; v2 += Bs[18 + i] * ei; v3 += Bs[27 + i] * ei; }
    {
        const double nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3);
        v0 /= nv; v1 /= nv; v2 /= nv; v3 /= nv;
    }
#pragma unroll 1
    for (int step = 0; step < kEssPolishSteps; ++step) {
        // the normal equations, upper triangle a[i][j], and the right-hand side a[i][4]
        double a[4][5] = {{v0 * v0, v0 * v1, v0 * v2, v0 * v3, 0.0}, {0.0, v1 * v1, v1 * v2, v1 * v3, 0.0},
                          {0.0, 0.0, v2 * v2, v2 * v3, 0.0}, {0.0, 0.0, 0.0, v3 * v3, 0.0}};
#pragma unroll 1
        for (int q = 0; q < 10; ++q) {
            double c = 0.0, j0 = 0.0, j1 = 0.0, j2 = 0.0, j3 = 0.0;
#pragma unroll 1
            for (int m = 0; m < 20; ++m) {
                const int code = (int)((m < 10 ? kEssMonoLo >> (6 * m) : kEssMonoHi >> (6 * (m - 10))) & 63ull);
                const int ia = code & 3, ib = (code >> 2) & 3, ic = code >> 4;
                const double xa = ia == 0 ? v0 : (ia == 1 ? v1 : (ia == 2 ? v2 : v3));
                const double xb = ib == 0 ? v0 : (ib == 1 ? v1 : (ib == 2 ? v2 : v3));
                const double xc = ic == 0 ? v0 : (ic == 1 ? v1 : (ic == 2 ? v2 : v3));
                const double k = M0[20 * q + m], da = k * xb * xc, db = k * xa * xc, dc = k * xa * xb;
                c += da * xa;
                j0 += (ia == 0 ? da : 0.0) + (ib == 0 ? db : 0.0) + (ic == 0 ? dc : 0.0);
                j1 += (ia == 1 ? da : 0.0) + (ib == 1 ? db : 0.0) + (ic == 1 ? dc : 0.0);
                j2 += (ia == 2 ? da : 0.0) + (ib == 2 ? db : 0.0) + (ic == 2 ? dc : 0.0);
                j3 += (ia == 3 ? da : 0.0) + (ib == 3 ? db : 0.0) + (ic == 3 ? dc : 0.0);
            }
            a[0][0] += j0 * j0; a[0][1] += j0 * j1; a[0][2] += j0 * j2; a[0][3] += j0 * j3; a[0][4] -= j0 * c;
            a[1][1] += j1 * j1; a[1][2] += j1 * j2; a[1][3] += j1 * j3; a[1][4] -= j1 * c;
            a[2][2] += j2 * j2; a[2][3] += j2 * j3; a[2][4] -= j2 * c;
            a[3][3] += j3 * j3; a[3][4] -= j3 * c;
        }
        a[1][0] = a[0][1]; a[2][0] = a[0][2]; a[3][0] = a[0][3]; a[2][1] = a[1][2]; a[3][1] = a[1][3]; a[3][2] = a[2][3];
        // positive definite: elimination without pivoting, then back-substitution
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = i + 1; r < 4; ++r) {
                const double f = a[r][i] / a[i][i];
#pragma unroll
                for (int cc = i; cc < 5; ++cc) a[r][cc] -= f * a[i][cc];
            }
        const double d3 = a[3][4] / a[3][3];
        const double d2 = (a[2][4] - a[2][3] * d3) / a[2][2];
        const double d1 = (a[1][4] - a[1][2] * d2 - a[1][3] * d3) / a[1][1];
        const double d0 = (a[0][4] - a[0][1] * d1 - a[0][2] * d2 - a[0][3] * d3) / a[0][0];
        v0 += d0; v1 += d1; v2 += d2; v3 += d3;
        const double nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3);
        v0 /= nv; v1 /= nv; v2 /= nv; v3 /= nv;
    }
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { Em[i] = v0 * Bs[i] + v1 * Bs[9 + i] + v2 * Bs[18 + i] + v3 * Bs[27 + i]; sum += fabs(Em[i]); }
    if (!(sum < INFINITY)) {                                     // (uniform) a step that went nowhere: the candidate as it was
#pragma unroll
        for (int i = 0; i < 9; ++i) Em[i] = Ec[i];
    }
}

// the hypotheses h0 + w, h0 + w + 4, ... < h1 of edge e by wave w; P: the edge's pairs (LDS or global); T: the wave's table
__device__ __forceinline__ void ess_slice(const double* P, const int* __restrict__ samples, int e, int n, int H, int h0, int h1,
                                          unsigned long long seed, double thr, const KMat& Ki, volatile double* Tg,
                                          int* __restrict__ hyp, int* __restrict__ hyp_roots, int& bc, int& bh, int& br,
                                          double (&bF)[9], double (&bE)[9]) {
    constexpr int S = kEssS;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double2* __restrict__ P2 = reinterpret_cast<const double2*>(P);
    EssLds* T = (EssLds*)Tg;
    EssLds* A = T + kEssOffA;
    EssLds* V = T + kEssOffV;
    EssLds* R = T + kEssOffR;
    EssLds* Bs = T + kEssOffB;
    EssLds* sys = T + kEssOffSys;
    EssLds* Bz = T + kEssOffBz;
    EssLds* Pc = T + kEssOffP;
    EssLds* cF = T + kEssOffF;
    EssLds* cE = T + kEssOffE;
    bc = -1; bh = 0x7fffffff; br = -1;
#pragma unroll
    for (int k = 0; k < 9; ++k) { bF[k] = 0.0; bE[k] = 0.0; }
#pragma unroll 1
    for (int h = h0 + w; h < h1; h += kTwoViewWaves) {
        const size_t at = (size_t)e * (size_t)H + (size_t)h;
        int idx[S];
        if (!ransac_sample(samples, e, H, h, n, seed, idx)) {    // (uniform over the wave)
            if (lane == 0 && hyp != nullptr) hyp[at] = -1;
            if (lane == 0 && hyp_roots != nullptr) hyp_roots[at] = -1;
            continue;
        }
        // the five rows in camera coordinates through LDS (lane 0 stores them), then lane i < 9 sums row i of A^T A
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const double2 qa = P2[2 * idx[j]], qb = P2[2 * idx[j] + 1];
            const double w1 = Ki.k[6] * qa.x + Ki.k[7] * qa.y + Ki.k[8], w2 = Ki.k[6] * qb.x + Ki.k[7] * qb.y + Ki.k[8];
            double r[1][9];
            FundModel::rows((Ki.k[0] * qa.x + Ki.k[1] * qa.y + Ki.k[2]) / w1, (Ki.k[3] * qa.x + Ki.k[4] * qa.y + Ki.k[5]) / w1,
                            (Ki.k[0] * qb.x + Ki.k[1] * qb.y + Ki.k[2]) / w2, (Ki.k[3] * qb.x + Ki.k[4] * qb.y + Ki.k[5]) / w2, r);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) R[9 * j + i] = r[0][i];
            }
        }
        if (lane < 9) {
            double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const double ri = R[9 * j + lane];
#pragma unroll
                for (int c = 0; c < 9; ++c) acc[c] += ri * R[9 * j + c];
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) { A[9 * lane + c] = acc[c]; V[9 * lane + c] = c == lane ? 1.0 : 0.0; }
        }
        jacobi_lds<9>(Tg + kEssOffA, Tg + kEssOffV, lane);
        // X Y Z W: the columns of the four smallest eigenvalues, ascending, the lower column first among equals.  The fifth
        // eigenvalue says whether the five rows have rank 5: a sample without it (collinear points) has no candidate
        bool rank5;
        {
            const int r = lane < 36 ? lane / 9 : 4, i = lane < 36 ? lane - 9 * r : 0;
            double d[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) d[k] = Tg[kEssOffA + 10 * k];    // (read as jacobi_lds wrote them: through the generic pointer)
            int col = 0;
            double fifth = 0.0, most = d[0];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                int rank = 0;
#pragma unroll
                for (int j = 0; j < 9; ++j) rank += (d[j] < d[k] || (d[j] == d[k] && j < k)) ? 1 : 0;
                if (rank == r) col = k;
                if (rank == 4) fifth = d[k];
                most = d[k] > most ? d[k] : most;
            }
            rank5 = fifth > kEssRankTol * most;                  // (the same on every lane; false for a NaN)
            if (lane < 36) Bs[lane] = Tg[kEssOffV + 9 * i + col];
        }
        // the 200 coefficients: entry t = 20 eq + m is the coefficient of monomial m in constraint eq (0: det E; 1 + 3 i + j:
        // entry (i, j) of 2 E E^T E - tr(E E^T) E), the sum of the trilinear form over the six orders of the monomial's three
        // variables over the number of orders that coincide
#pragma unroll 1
        for (int t = lane; t < 200; t += 64) {
            const int eq = t / 20, m = t - 20 * eq;
            const int code = (int)((m < 10 ? kEssMonoLo >> (6 * m) : kEssMonoHi >> (6 * (m - 10))) & 63ull);
            const int a = code & 3, b = (code >> 2) & 3, c = code >> 4;
            const double mult = (a == b && b == c) ? 6.0 : ((a == b || b == c) ? 2.0 : 1.0);
            const int ij = eq > 0 ? eq - 1 : 0, i = ij / 3, j = ij - 3 * i;
            double s = 0.0;
#pragma unroll 1
            for (int p = 0; p < 6; ++p) {
                const int first = p < 2 ? a : (p < 4 ? b : c);
                const int second = p == 0 ? b : (p == 1 ? c : (p == 2 ? a : (p == 3 ? c : (p == 4 ? a : b))));
                const int third = a + b + c - first - second;
                const EssLds* Pm = Bs + 9 * first;
                const EssLds* Qm = Bs + 9 * second;
                const EssLds* Rm = Bs + 9 * third;
                s += eq == 0 ? ess_det3(Pm, Qm, Rm) : ess_trace3(Pm, Qm, Rm, i, j);
            }
            sys[t] = s / mult;
            T[kEssOffM + t] = s / mult;
        }
        // Gauss-Jordan on the left 10 x 10 block with partial pivoting (the first of equal magnitudes); lane = 20 r3 + j
        // takes column j of the rows r3, r3 + 3, r3 + 6, r3 + 9
        {
            const int r3 = lane / 20, j = lane - 20 * r3;
#pragma unroll 1
            for (int c = 0; c < 10; ++c) {
                int p = c;
                double big = fabs(sys[21 * c]);
                for (int r = c + 1; r < 10; ++r) { const double v = fabs(sys[20 * r + c]); if (v > big) { big = v; p = r; } }
                if (lane < 20) { const double u = sys[20 * c + lane], v = sys[20 * p + lane]; sys[20 * c + lane] = v; sys[20 * p + lane] = u; }
                const double piv = sys[21 * c];
                if (lane < 20) sys[20 * c + lane] = sys[20 * c + lane] / piv;
                if (lane < 60) {
                    const double pj = sys[20 * c + j];
                    double f[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { const int r = r3 + 3 * q; f[q] = (r < 10 && r != c) ? sys[20 * r + c] : 0.0; }
#pragma unroll
                    for (int q = 0; q < 4; ++q) { const int r = r3 + 3 * q; if (r < 10 && r != c) sys[20 * r + j] = sys[20 * r + j] - f[q] * pj; }
                }
            }
        }
        // B(z): row q from the rows 4 + 2 q and 5 + 2 q of the system, (row 4 + 2 q) - z (row 5 + 2 q); column 0 1 2 the
        // coefficient of x, y, 1 (the right-hand columns 10.., 13.., 16..), of degree 3, 3, 4
        if (lane < 45) {
            const int q = lane / 15, rest = lane - 15 * q, col = rest / 5, d = rest - 5 * col;
            const int D = col == 2 ? 3 : 2, base = 10 + 3 * col;
            const EssLds* ra = sys + 20 * (4 + 2 * q);
            const EssLds* rb = ra + 20;
            const double va = d <= D ? ra[base + D - d] : 0.0, vb = (d >= 1 && d - 1 <= D) ? rb[base + D - d + 1] : 0.0;
            Bz[lane] = va - vb;
        }
        // (p0, p1, p2) = row 0 x row 1 of B(z) as polynomials (degrees 7, 7, 6); det B(z) = p0 b20 + p1 b21 + p2 b22
        if (lane < 24) {
            const int q = lane >> 3, k = lane & 7;
            const int eu = q == 0 ? 1 : (q == 1 ? 2 : 0), ev = q == 0 ? 5 : (q == 1 ? 3 : 4);
            const int es = q == 0 ? 2 : (q == 1 ? 0 : 1), et = q == 0 ? 4 : (q == 1 ? 5 : 3);
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 5; ++i)
                if (k - i >= 0 && k - i < 5) s += Bz[5 * eu + i] * Bz[5 * ev + k - i] - Bz[5 * es + i] * Bz[5 * et + k - i];
            Pc[lane] = s;
        }
        if (lane < 11) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (lane - i >= 0 && lane - i < 5) s += Pc[8 * q + i] * Bz[5 * (6 + q) + lane - i];
            T[kEssOffC + lane] = s;
        }
        int half = 0;
        const int nr = rank5 ? ess_real_roots(T, lane, half) : 0;
        // a candidate per root, ascending z: (x, y, 1) the null vector of B(z) as the cross product of two of its rows, the
        // pair whose product is the longest (the first of equals); E = xX + yY + zZ + W; F_pix = K^-T E K^-1
        const EssLds* roots = T + kEssOffRoots + 10 * half;
        if (lane < nr) {
            const double z = roots[lane];
            double b[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) b[q] = (((Bz[5 * q + 4] * z + Bz[5 * q + 3]) * z + Bz[5 * q + 2]) * z + Bz[5 * q + 1]) * z + Bz[5 * q];
            const double n0[3] = {b[1] * b[5] - b[2] * b[4], b[2] * b[3] - b[0] * b[5], b[0] * b[4] - b[1] * b[3]};
            const double n1[3] = {b[1] * b[8] - b[2] * b[7], b[2] * b[6] - b[0] * b[8], b[0] * b[7] - b[1] * b[6]};
            const double n2[3] = {b[4] * b[8] - b[5] * b[7], b[5] * b[6] - b[3] * b[8], b[3] * b[7] - b[4] * b[6]};
            const double l0 = n0[0] * n0[0] + n0[1] * n0[1] + n0[2] * n0[2], l1 = n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2],
                         l2 = n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2];
            double vx = n0[0], vy = n0[1], vw = n0[2], best = l0;
            if (l1 > best) { vx = n1[0]; vy = n1[1]; vw = n1[2]; best = l1; }
            if (l2 > best) { vx = n2[0]; vy = n2[1]; vw = n2[2]; }
            const double x = vx / vw, y = vy / vw;
            double Em[9], G[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) Em[k] = x * Bs[k] + y * Bs[9 + k] + z * Bs[18 + k] + Bs[27 + k];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) G[3 * i + j] = Em[3 * i] * Ki.k[j] + Em[3 * i + 1] * Ki.k[3 + j] + Em[3 * i + 2] * Ki.k[6 + j];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) cF[9 * lane + 3 * i + j] = Ki.k[i] * G[j] + Ki.k[3 + i] * G[3 + j] + Ki.k[6 + i] * G[6 + j];
#pragma unroll
            for (int k = 0; k < 9; ++k) cE[9 * lane + k] = Em[k];
        }
        // one pass over the pairs: a lane loads a pair and tests it against every candidate; lane c keeps the count of candidate c
        int mine = 0;
#pragma unroll 1
        for (int k0 = 0; k0 < n; k0 += 64) {                     // uniform over the wave: the ballot needs every lane
            const int k = k0 + lane;
            double2 qa = make_double2(0.0, 0.0), qb = make_double2(0.0, 0.0);
            if (k < n) { qa = P2[2 * k]; qb = P2[2 * k + 1]; }
#pragma unroll 1
            for (int c = 0; c < nr; ++c) {
                double Fc[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) Fc[q] = cF[9 * c + q];
                const bool inl = k < n && FundModel::inlier(Fc, qa.x, qa.y, qb.x, qb.y, thr);
                const int pop = __popcll(__ballot(inl));
                mine += lane == c ? pop : 0;
            }
        }
        int cb = -1, best = 0;
#pragma unroll 1
        for (int c = 0; c < nr; ++c) {
            const int v = __shfl(mine, c);
            if (cb < 0 || v > best) { best = v; cb = c; }        // (z ascends: the lowest of equal counts stays)
        }
        if (lane == 0 && hyp != nullptr) hyp[at] = best;
        if (lane == 0 && hyp_roots != nullptr) hyp_roots[at] = nr;
        if (best > bc) {                                         // (h ascends: the lowest h of equal counts stays)
            bc = best; bh = h; br = cb;
#pragma unroll
            for (int k = 0; k < 9; ++k) { bF[k] = 0.0; bE[k] = 0.0; }
            if (cb >= 0) {                                       // the wave's best so far is kept polished (the edge's best always is one)
                double G[9];
                ess_polish(T, cE + 9 * cb, bE);
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) G[3 * i + j] = bE[3 * i] * Ki.k[j] + bE[3 * i + 1] * Ki.k[3 + j] + bE[3 * i + 2] * Ki.k[6 + j];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) bF[3 * i + j] = Ki.k[i] * G[j] + Ki.k[3 + i] * G[3 + j] + Ki.k[6 + i] * G[6 + j];
            }
        }
    }
}

struct EssOut {
    double* __restrict__ E;                      // [E][9]
    unsigned char* __restrict__ mask;            // [M_used]
    int* __restrict__ ints;                      // [E][5] inliers, best h, status, success, best root
};

__global__ __launch_bounds__(kTwoViewThreads) void k_ess_ransac(FundIn in, int H, int hs, int n_slices, unsigned long long seed, double thr,
                                                                KMat Ki, double* __restrict__ slots, int* __restrict__ hyp,
                                                                int* __restrict__ hyp_roots) {
    extern __shared__ __align__(16) double smem[];
    __shared__ double tab[kTwoViewWaves][kEssWaveDoubles];
    const RansacBlock rb = ransac_block(H, hs, n_slices);
    const int b = in.uptr[rb.item], n = in.uptr[rb.item + 1] - b, w = threadIdx.x >> 6;
    const double* __restrict__ gp = in.pairs + 4 * (size_t)b;
    if (n < kEssS) { ransac_no_hypothesis(rb, H, hyp); ransac_no_hypothesis(rb, H, hyp_roots); ransac_empty_slot<kEssPayload>(slots); return; }   // (uniform) FEW_PAIRS
    int bc, bh, br;
    double bF[9], bE[9];
    if (n <= kTwoViewLdsPairs) {
        stage_table(gp, 4 * n, smem);
        ess_slice(smem, in.samples, rb.item, n, H, rb.h0, rb.h1, seed, thr, Ki, tab[w], hyp, hyp_roots, bc, bh, br, bF, bE);
    } else {
        ess_slice(gp, in.samples, rb.item, n, H, rb.h0, rb.h1, seed, thr, Ki, tab[w], hyp, hyp_roots, bc, bh, br, bF, bE);
    }
    RansacBest<kEssPayload> best{bc, bh, br};
#pragma unroll
    for (int k = 0; k < 9; ++k) { best.v[k] = bF[k]; best.v[9 + k] = bE[k]; }
    ransac_store(best, slots);
}

// what twoview_verdict asks of a model: E is scored as F, by its F_pix (the first nine doubles of the payload)
struct EssVerdict : FundModel { static constexpr int S = kEssS; };
static_assert(kEssOk == kFundOk && kEssFewPairs == kFundFewPairs && kEssDegenerate == kFundDegenerate, "EssVerdict reports F's status values");

// One workgroup per edge: twoview_verdict, then what is E's own: the status also needs a root (the fifth integer), E by fund_unit.
__global__ __launch_bounds__(kTwoViewThreads) void k_ess_finish(FundIn in, int n_slices, double thr, double confidence,
                                                                const double* __restrict__ slots, EssOut out) {
    const int e = blockIdx.x;
    const int b = in.uptr[e], n = in.uptr[e + 1] - b;
    const double2* __restrict__ P2 = reinterpret_cast<const double2*>(in.pairs + 4 * (size_t)b);
    int* __restrict__ oi = out.ints + 5 * (size_t)e;
    double pay[kEssPayload];
    const TwoViewVerdict vd = twoview_verdict<EssVerdict>(P2, e, (size_t)b, n, n_slices, thr, confidence, slots, out.mask, nullptr, oi, pay);
    if (threadIdx.x == 0) {
        // (DEGENERATE still reports the count, h, root and mask of its best hypothesis; only the matrix is withheld)
        const int status = vd.status == kEssOk && vd.aux < 0 ? kEssDegenerate : vd.status;
        oi[2] = status; oi[4] = vd.aux;
        double Eu[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Eu[k] = pay[9 + k];
        fund_unit(Eu);
#pragma unroll
        for (int k = 0; k < 9; ++k) out.E[9 * (size_t)e + k] = status == kEssOk ? Eu[k] : 0.0;
    }
}

// ---- sfmba_recover_pose ----
struct PoseOut {
    double* __restrict__ Rt;                     // [E][12] R (9), t (3)
    double* __restrict__ sum_err;                // [E]
    int* __restrict__ ints;                      // [E][6] front of the winner, front of the four candidates, status
    unsigned char* __restrict__ front;           // [M_used]
    double* __restrict__ X;                      // [M_used][3]
    double* __restrict__ angle_deg;              // [M_used]
};

// The two-view DLT of one pair against M1 = [K | 0] and M2 (rows of 4): the rows of triangulate_points_linear2,
// the smallest eigenvector of their A^T A, X = w[:3] / w[3]
__device__ __forceinline__ void pose_dlt(const KMat& K, const double* __restrict__ M2, double x1, double y1, double x2, double y2,
                                         double& X, double& Y, double& Z) {
    double rows[4][4];
#pragma unroll
    for (int j = 0; j < 3; ++j) { rows[0][j] = x1 * K.k[6 + j] - K.k[j]; rows[1][j] = y1 * K.k[6 + j] - K.k[3 + j]; }
    rows[0][3] = 0.0; rows[1][3] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { rows[2][j] = x2 * M2[8 + j] - M2[j]; rows[3][j] = y2 * M2[8 + j] - M2[4 + j]; }
    double a[10];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j)
            a[sym<4>(i, j)] = rows[0][i] * rows[0][j] + rows[1][i] * rows[1][j] + rows[2][i] * rows[2][j] + rows[3][i] * rows[3][j];
    double w0, w1, w2, w3;
    smallest_eigenvector4(a, w0, w1, w2, w3);
    X = w0 / w3; Y = w1 / w3; Z = w2 / w3;
}
// candidate row c of LDS: R (9), t (3), M2 = K [R | t] (12)
constexpr int kPoseCand = 24;
__device__ __forceinline__ bool pose_in_front(const double* __restrict__ cd, double X, double Y, double Z, double min_depth) {
    const double d2 = cd[6] * X + cd[7] * Y + cd[8] * Z + cd[11];
    return Z > min_depth && d2 > min_depth && Z < INFINITY && d2 < INFINITY;
}

__global__ __launch_bounds__(kTwoViewThreads) void k_recover_pose(const double* __restrict__ pairs, const int* __restrict__ uptr,
                                                                  const double* __restrict__ Emat, KMat K, double min_depth, PoseOut out) {
    __shared__ double cand[4 * kPoseCand];
    __shared__ double red[kTwoViewWaves];
    __shared__ int redi[kTwoViewWaves][4];
    __shared__ int ctl[2];
    constexpr double kDeg = 57.295779513082320877;
    const int e = blockIdx.x;
    const int b = uptr[e], n = uptr[e + 1] - b;
    const bool first = threadIdx.x == 0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double2* __restrict__ P2 = reinterpret_cast<const double2*>(pairs + 4 * (size_t)b);
    if (threadIdx.x < 64) {                                      // wave 0, every lane alike; lane 0 stores
        double E[9], sum = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) { E[k] = Emat[9 * (size_t)e + k]; sum += fabs(E[k]); }
        double a[6], v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) a[sym<3>(i, j)] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
        jacobi_sweeps<3>(a, v);
        // eigenpairs by descending eigenvalue (the first of equals first)
        double l0 = a[0], l1 = a[3], l2 = a[5];
        double c0[3] = {v[0], v[3], v[6]}, c1[3] = {v[1], v[4], v[7]}, c2[3] = {v[2], v[5], v[8]};
        auto order = [](double& la, double& lb, double (&ca)[3], double (&cb)[3]) {
            if (lb > la) {
                const double t = la; la = lb; lb = t;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double u = ca[k]; ca[k] = cb[k]; cb[k] = u; }
            }
        };
        order(l0, l1, c0, c1); order(l1, l2, c1, c2); order(l0, l1, c0, c1);
        // the sign of an eigenvector is the solver's accident, and flipping v1 swaps R1 with R2 and t with -t: v1 and v2
        // get their component of largest magnitude (the first of equals) positive, v3 follows from det V = +1
        auto positive = [](double (&c)[3]) {
            double big = fabs(c[0]), sg = c[0];
            if (fabs(c[1]) > big) { big = fabs(c[1]); sg = c[1]; }
            if (fabs(c[2]) > big) { big = fabs(c[2]); sg = c[2]; }
            if (sg < 0.0) { c[0] = -c[0]; c[1] = -c[1]; c[2] = -c[2]; }
        };
        positive(c0); positive(c1);
        const double det = c0[0] * (c1[1] * c2[2] - c1[2] * c2[1]) - c0[1] * (c1[0] * c2[2] - c1[2] * c2[0]) +
                           c0[2] * (c1[0] * c2[1] - c1[1] * c2[0]);
        if (det < 0.0) { c2[0] = -c2[0]; c2[1] = -c2[1]; c2[2] = -c2[2]; }
        // s_i = |E v_i|, not sqrt(lambda_i): an eigenvalue of E^T E carries eps s1^2 of rounding, so its root cannot tell an
        // s2 below 1e-8 s1 from zero, while |E v2| is good to a few eps s1
        double u1[3], u2[3], u3[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u1[i] = E[3 * i] * c0[0] + E[3 * i + 1] * c0[1] + E[3 * i + 2] * c0[2];
            u2[i] = E[3 * i] * c1[0] + E[3 * i + 1] * c1[1] + E[3 * i + 2] * c1[2];
        }
        const double sg1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]), sg2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
        const bool good = sum < INFINITY && sg2 > 1e-12 * sg1;   // (false for a NaN as well)
#pragma unroll
        for (int i = 0; i < 3; ++i) { u1[i] /= sg1; u2[i] /= sg2; }
        const double d12 = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) u2[i] -= d12 * u1[i];
        const double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) u2[i] /= n2;
        u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
        if (first) {
            ctl[0] = n < 1 ? kPoseFewPairs : (good ? kPoseOk : kPoseDegenerate);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double* __restrict__ cd = cand + c * kPoseCand;
                const double sr = c < 2 ? 1.0 : -1.0, st = (c & 1) ? -1.0 : 1.0;
                // R1 = U W V^T = u2 v1^T - u1 v2^T + u3 v3^T, R2 = U W^T V^T = -u2 v1^T + u1 v2^T + u3 v3^T
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) cd[3 * i + j] = sr * (u2[i] * c0[j] - u1[i] * c1[j]) + u3[i] * c2[j];
                    cd[9 + i] = st * u3[i];
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) cd[12 + 4 * i + j] = K.k[3 * i] * cd[j] + K.k[3 * i + 1] * cd[3 + j] + K.k[3 * i + 2] * cd[6 + j];
                    cd[12 + 4 * i + 3] = K.k[3 * i] * cd[9] + K.k[3 * i + 1] * cd[10] + K.k[3 * i + 2] * cd[11];
                }
            }
        }
    }
    __syncthreads();
    if (ctl[0] != kPoseOk) {                                     // (uniform over the workgroup)
        for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
            out.front[(size_t)b + k] = 0;
            out.X[3 * ((size_t)b + k)] = NAN; out.X[3 * ((size_t)b + k) + 1] = NAN; out.X[3 * ((size_t)b + k) + 2] = NAN;
            out.angle_deg[(size_t)b + k] = NAN;
        }
        if (first) {
#pragma unroll
            for (int k = 0; k < 12; ++k) out.Rt[12 * (size_t)e + k] = 0.0;
            out.sum_err[e] = NAN;
            int* __restrict__ oi = out.ints + 6 * (size_t)e;
            oi[0] = 0; oi[1] = 0; oi[2] = 0; oi[3] = 0; oi[4] = 0; oi[5] = ctl[0];
        }
        return;
    }
    // pass 1: pairs in front of each candidate
    int cnt[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
        const double2 qa = P2[2 * k], qb = P2[2 * k + 1];
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
            const double* __restrict__ cd = cand + c * kPoseCand;
            double X, Y, Z;
            pose_dlt(K, cd + 12, qa.x, qa.y, qb.x, qb.y, X, Y, Z);
            const int f = pose_in_front(cd, X, Y, Z, min_depth) ? 1 : 0;
            cnt[0] += c == 0 ? f : 0; cnt[1] += c == 1 ? f : 0; cnt[2] += c == 2 ? f : 0; cnt[3] += c == 3 ? f : 0;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) cnt[c] = wave_isum(cnt[c]);
    if (lane == 0) { redi[w][0] = cnt[0]; redi[w][1] = cnt[1]; redi[w][2] = cnt[2]; redi[w][3] = cnt[3]; }
    __syncthreads();
    if (first) {
        int tot[4], win = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) { tot[c] = 0; for (int k = 0; k < kTwoViewWaves; ++k) tot[c] += redi[k][c]; }
#pragma unroll
        for (int c = 1; c < 4; ++c) if (tot[c] > tot[win]) win = c;            // the earliest of equal counts
        int second = -1;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c != win && tot[c] > second) second = tot[c];
        ctl[1] = win;
        int* __restrict__ oi = out.ints + 6 * (size_t)e;
        oi[0] = tot[win]; oi[1] = tot[0]; oi[2] = tot[1]; oi[3] = tot[2]; oi[4] = tot[3];
        oi[5] = tot[win] > second ? kPoseOk : kPoseTie;
    }
    __syncthreads();
    // pass 2: the winner's points, mask, ray angles and the reference's reproj_err total
    const double* __restrict__ cd = cand + ctl[1] * kPoseCand;
    const double O2x = -(cd[0] * cd[9] + cd[3] * cd[10] + cd[6] * cd[11]), O2y = -(cd[1] * cd[9] + cd[4] * cd[10] + cd[7] * cd[11]),
                 O2z = -(cd[2] * cd[9] + cd[5] * cd[10] + cd[8] * cd[11]);
    double err[1] = {0.0};
#pragma unroll 1
    for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
        const double2 qa = P2[2 * k], qb = P2[2 * k + 1];
        double X, Y, Z;
        pose_dlt(K, cd + 12, qa.x, qa.y, qb.x, qb.y, X, Y, Z);
        const bool f = pose_in_front(cd, X, Y, Z, min_depth);
        const double bx = X - O2x, by = Y - O2y, bz = Z - O2z;
        const double cx = Y * bz - Z * by, cy = Z * bx - X * bz, cz = X * by - Y * bx;
        const double ang = kDeg * atan2(sqrt(cx * cx + cy * cy + cz * cz), X * bx + Y * by + Z * bz);
        const double p1w = K.k[6] * X + K.k[7] * Y + K.k[8] * Z;
        const double e1x = qa.x - (K.k[0] * X + K.k[1] * Y + K.k[2] * Z) / p1w, e1y = qa.y - (K.k[3] * X + K.k[4] * Y + K.k[5] * Z) / p1w;
        const double* __restrict__ M2 = cd + 12;
        const double p2w = M2[8] * X + M2[9] * Y + M2[10] * Z + M2[11];
        const double e2x = qb.x - (M2[0] * X + M2[1] * Y + M2[2] * Z + M2[3]) / p2w, e2y = qb.y - (M2[4] * X + M2[5] * Y + M2[6] * Z + M2[7]) / p2w;
        err[0] += sqrt(e1x * e1x + e1y * e1y) + sqrt(e2x * e2x + e2y * e2y);
        const size_t o = (size_t)b + k;
        out.front[o] = f ? 1 : 0;
        out.X[3 * o] = X; out.X[3 * o + 1] = Y; out.X[3 * o + 2] = Z;
        out.angle_deg[o] = f ? ang : NAN;
    }
    block_sum<1>(err, red);
    if (first) {
#pragma unroll
        for (int k = 0; k < 12; ++k) out.Rt[12 * (size_t)e + k] = cd[k];
        out.sum_err[e] = err[0];
    }
}

// ---- sfmba_similarity_ransac (include/sfmba.h): dst ~ s R src + t between two 3-D point sets ----
// A batch of SETS plays the part of the edges: each a run of used pairs sx sy sz dx dy dz (48 bytes, packed by the host in
// stored order); nothing of a bundle-adjustment problem is read.  The fifth model of the shell, in the form of k_pnp_ransac:
//   k_sim_ransac   grid over (set, slice of its hypotheses).  Every LANE draws three pairs (ransac_sample<3>) and solves its
//                  own hypothesis by Horn's closed form (sim_from_sums: the 4x4 matrix N of the nine centred sums, the
//                  quaternion of its largest eigenvalue by smallest_eigenvector4 on -N, R, s, t), then the wave walks the
//                  set's pairs with ONE index: every lane reads the same address (LDS broadcasts it without a conflict; past
//                  kSimLdsPairs the pairs are read at their global address, the same on every lane) and counts the inliers
//                  of its own (s, R, t) in a register.  No slab, no readlane / ballot loop per hypothesis, and 64 lanes
//                  busy however few pairs the set has.  The wave's best of a round is the largest count, the lowest lane
//                  among equals; rounds ascend in h.
//   k_sim_finish   one workgroup per set, the sequence of twoview_verdict: best slot, the mask of that similarity in stored
//                  order and the count FROM that mask, status; refit = 1: means, then the nine centred sums and |a'|^2 over
//                  the inliers (block_sum, a fixed order), the same sim_from_sums by thread 0, the refit's mask and count.
// No atomics; sums in a fixed order; counts do not depend on the order.
constexpr int kSimLdsPairs = 3072;        // a set of up to this many used pairs is staged in LDS: 144 KiB of the 160, beside
                                          // the 512 bytes of ransac_store; the launch asks for the largest set's 48 n bytes
                                          // only, so sets of up to 1706 pairs (80 KiB) leave room for two workgroups a CU
constexpr int kSimMinSlice = 64;          // fewest hypotheses of a workgroup's slice (one per lane of one wave)
constexpr int kSimPair = 6;               // doubles of a packed pair
constexpr int kSimPayload = 13;           // of a slot: s, R (9, row-major), t (3)
constexpr int kSimOk = 0, kSimFewPairs = 1, kSimDegenerate = 2;
constexpr double kSimEigenGap = 1e-9;     // the rotation is determined when l1 - l2 of N is above this times l1 - l4
static_assert(sizeof(double) * kSimPair * kSimLdsPairs + sizeof(double) * kTwoViewWaves * (kRansacHead + kSimPayload) <= 160 * 1024,
              "the staged pairs and ransac_store's table fit the LDS of a CU");

// Horn (1987) from the sums of a set of pairs a -> b: S[3 i + j] = sum a'_i b'_j and saa = sum |a'|^2 about the means am,
// bm.  m <- s, R, t; false (m is then not to be used): the two largest eigenvalues of N are not kSimEigenGap of the spread
// apart (a collinear or repeated set: the rotation about the line is free), saa or s is not positive, anything non-finite.
__device__ __forceinline__ bool sim_from_sums(const double (&S)[9], double saa, const double (&am)[3], const double (&bm)[3],
                                              double (&m)[kSimPayload]) {
    double a[10];                                                // -N, upper triangle row by row
    a[0] = -(S[0] + S[4] + S[8]); a[1] = -(S[5] - S[7]); a[2] = -(S[6] - S[2]); a[3] = -(S[1] - S[3]);
    a[4] = -(S[0] - S[4] - S[8]); a[5] = -(S[1] + S[3]); a[6] = -(S[6] + S[2]);
    a[7] = -(S[4] - S[0] - S[8]); a[8] = -(S[5] + S[7]);
    a[9] = -(S[8] - S[0] - S[4]);
    double qw, qx, qy, qz;
    smallest_eigenvector4(a, qw, qx, qy, qz);
    // the eigenvalues of -N are on a's diagonal: the smallest, the second smallest and the largest
    const double l01 = fmin(a[0], a[4]), h01 = fmax(a[0], a[4]), l23 = fmin(a[7], a[9]), h23 = fmax(a[7], a[9]);
    const double lo = fmin(l01, l23), hi = fmax(h01, h23), second = fmin(fmax(l01, l23), fmin(h01, h23));
    if (!(second - lo > kSimEigenGap * (hi - lo))) return false;
    const double nq = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= nq; qx /= nq; qy /= nq; qz /= nq;
    double* R = m + 1;
    R[0] = qw * qw + qx * qx - qy * qy - qz * qz; R[1] = 2.0 * (qx * qy - qw * qz); R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz); R[4] = qw * qw - qx * qx + qy * qy - qz * qz; R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy); R[7] = 2.0 * (qy * qz + qw * qx); R[8] = qw * qw - qx * qx - qy * qy + qz * qz;
    // sum b' . (R a') = sum_ij R_ji S_ij
    const double num = R[0] * S[0] + R[1] * S[3] + R[2] * S[6] + R[3] * S[1] + R[4] * S[4] + R[5] * S[7] + R[6] * S[2] + R[7] * S[5] +
                       R[8] * S[8];
    const double s = num / saa;
    if (!(saa > 0.0) || !(s > 0.0)) return false;
    m[0] = s;
    m[10] = bm[0] - s * (R[0] * am[0] + R[1] * am[1] + R[2] * am[2]);
    m[11] = bm[1] - s * (R[3] * am[0] + R[4] * am[1] + R[5] * am[2]);
    m[12] = bm[2] - s * (R[6] * am[0] + R[7] * am[1] + R[8] * am[2]);
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kSimPayload; ++k) sum += fabs(m[k]);
    return sum < INFINITY;
}

// the score's test: |s R a + t - b|^2 STRICTLY below thr2; a non-finite value is no inlier
__device__ __forceinline__ bool sim_inlier(const double (&m)[kSimPayload], const double (&o)[kSimPair], double thr2) {
    const double px = m[1] * o[0] + m[2] * o[1] + m[3] * o[2], py = m[4] * o[0] + m[5] * o[1] + m[6] * o[2],
                 pz = m[7] * o[0] + m[8] * o[1] + m[9] * o[2];
    const double dx = m[0] * px + m[10] - o[3], dy = m[0] * py + m[11] - o[4], dz = m[0] * pz + m[12] - o[5];
    const double d2 = dx * dx + dy * dy + dz * dz;
    return d2 < thr2 && d2 < INFINITY;
}

// pair k of the set: staged at the head of the dynamic LDS (addressed through smem, see pnp_p3p) or at g2
template <bool LDS_PAIRS>
__device__ __forceinline__ void sim_pair(const double2* __restrict__ g2, int k, double (&o)[kSimPair]) {
    extern __shared__ __align__(16) double smem[];
    double2 q0, q1, q2;
    if constexpr (LDS_PAIRS) {
        const double2* s2 = reinterpret_cast<const double2*>(smem);
        q0 = s2[3 * k]; q1 = s2[3 * k + 1]; q2 = s2[3 * k + 2];
    } else {
        q0 = g2[3 * (size_t)k]; q1 = g2[3 * (size_t)k + 1]; q2 = g2[3 * (size_t)k + 2];
    }
    o[0] = q0.x; o[1] = q0.y; o[2] = q1.x; o[3] = q1.y; o[4] = q2.x; o[5] = q2.y;
}

// the hypotheses h0 + 64 w + lane, + 256, ... < h1 of set e, one per lane; leaves the wave's best on every lane
template <bool LDS_PAIRS>
__device__ __forceinline__ void sim_slice(const double* __restrict__ gp, const int* __restrict__ samples, int e, int n, int H, int h0,
                                          int h1, unsigned long long seed, double thr2, int* __restrict__ hyp,
                                          RansacBest<kSimPayload>& best) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double2* __restrict__ g2 = reinterpret_cast<const double2*>(gp);
#pragma unroll 1
    for (int hb = h0 + 64 * w; hb < h1; hb += 64 * kTwoViewWaves) {   // uniform over the wave
        const int h = hb + lane;
        int hcount = -2;                                         // (a lane past h1: below every hypothesis)
        bool solved = false;
        double m[kSimPayload];
        if (h < h1) {
            int idx[3];
            hcount = kRansacNone;
            if (ransac_sample(samples, e, H, h, n, seed, idx)) {
                double a[9], b[9];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double o[kSimPair];
                    sim_pair<LDS_PAIRS>(g2, idx[j], o);
                    a[3 * j] = o[0]; a[3 * j + 1] = o[1]; a[3 * j + 2] = o[2]; b[3 * j] = o[3]; b[3 * j + 1] = o[4]; b[3 * j + 2] = o[5];
                }
                double am[3], bm[3], S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, saa = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) { am[i] = (a[i] + a[3 + i] + a[6 + i]) / 3.0; bm[i] = (b[i] + b[3 + i] + b[6 + i]) / 3.0; }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double ac[3] = {a[3 * k] - am[0], a[3 * k + 1] - am[1], a[3 * k + 2] - am[2]};
                    const double bc[3] = {b[3 * k] - bm[0], b[3 * k + 1] - bm[1], b[3 * k + 2] - bm[2]};
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) S[3 * i + j] += ac[i] * bc[j];
                    saa += ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2];
                }
                solved = sim_from_sums(S, saa, am, bm, m);
                hcount = 0;                                      // a valid sample; without a solution it stays 0
            }
        }
        if (!solved) {
#pragma unroll
            for (int k = 0; k < kSimPayload; ++k) m[k] = 0.0;
        }
        if (__ballot(solved)) {                                  // (uniform over the wave)
            int cnt = 0;
#pragma unroll 4
            for (int k = 0; k < n; ++k) {                        // one index for the wave: every lane reads the same pair
                double o[kSimPair];
                sim_pair<LDS_PAIRS>(g2, k, o);
                cnt += sim_inlier(m, o, thr2) ? 1 : 0;
            }
            if (solved) hcount = cnt;
        }
        if (h < h1 && hyp != nullptr) hyp[(size_t)e * (size_t)H + (size_t)h] = hcount;
        // the round's best: the largest count, the lowest lane (h) among equals; rounds ascend in h
        const int top = wave_reduce_xor(hcount, [](int x, int y) { return max(x, y); });
        if (top > best.count) {
            const int lb = __ffsll((long long)__ballot(hcount == top)) - 1;
            best.count = top; best.h = hb + lb;
#pragma unroll
            for (int k = 0; k < kSimPayload; ++k) best.v[k] = __shfl(m[k], lb);
        }
    }
}

// dynamic LDS: the set's pairs when they fit (the host sizes it by the largest set of the batch, kSimLdsPairs at the most)
__global__ __launch_bounds__(kTwoViewThreads) void k_sim_ransac(FundIn in, int H, int hs, int n_slices, unsigned long long seed,
                                                                double thr2, double* __restrict__ slots, int* __restrict__ hyp) {
    extern __shared__ __align__(16) double smem[];
    const RansacBlock rb = ransac_block(H, hs, n_slices);
    const int b = in.uptr[rb.item], n = in.uptr[rb.item + 1] - b;
    const double* __restrict__ gp = in.pairs + kSimPair * (size_t)b;
    if (n < 3) { ransac_no_hypothesis(rb, H, hyp); ransac_empty_slot<kSimPayload>(slots); return; }   // (uniform) FEW_PAIRS
    RansacBest<kSimPayload> best;
    if (n <= kSimLdsPairs) {
        stage_table(gp, kSimPair * n, smem);
        sim_slice<true>(gp, in.samples, rb.item, n, H, rb.h0, rb.h1, seed, thr2, hyp, best);
    } else {
        sim_slice<false>(gp, in.samples, rb.item, n, H, rb.h0, rb.h1, seed, thr2, hyp, best);
    }
    ransac_store(best, slots);
}

struct SimOut {
    double* __restrict__ sim;                    // [E][13] s, R, t of the best hypothesis
    double* __restrict__ sim_refit;              // [E][13]
    unsigned char* __restrict__ mask;            // [M_used] of the best hypothesis
    unsigned char* __restrict__ refit_mask;      // [M_used] of sim_refit
    int* __restrict__ ints;                      // [E][5] inliers, best h, status, success, refit inliers
};

__global__ __launch_bounds__(kTwoViewThreads) void k_sim_finish(FundIn in, int n_slices, double thr2, double confidence, int refit,
                                                                const double* __restrict__ slots, SimOut out) {
    __shared__ double red[kTwoViewWaves * 10];
    __shared__ double sp[kSimPayload], sm[6];
    __shared__ int ctl[4];                                       // status, best h, has a similarity, count
    const int e = blockIdx.x;
    const int b = in.uptr[e], n = in.uptr[e + 1] - b;
    const bool first = threadIdx.x == 0;
    const double2* __restrict__ g2 = reinterpret_cast<const double2*>(in.pairs + kSimPair * (size_t)b);
    int* __restrict__ oi = out.ints + 5 * (size_t)e;
    double* __restrict__ om = out.sim + kSimPayload * (size_t)e;
    double* __restrict__ orf = out.sim_refit + kSimPayload * (size_t)e;
    unsigned char* __restrict__ mk = out.mask + (size_t)b;       // a thread reads back only what it stored itself
    unsigned char* __restrict__ rmk = out.refit_mask + (size_t)b;
    if (n < 3) {                                                 // (uniform over the workgroup) FEW_PAIRS
        for (int k = threadIdx.x; k < n; k += kTwoViewThreads) { mk[k] = 0; rmk[k] = 0; }
        if (threadIdx.x < kSimPayload) { om[threadIdx.x] = 0.0; orf[threadIdx.x] = 0.0; }
        if (first) { oi[0] = 0; oi[1] = -1; oi[2] = kSimFewPairs; oi[3] = 0; oi[4] = 0; }
        return;
    }
    if (first) {
        const double* __restrict__ bs = ransac_best_slot<kSimPayload>(slots, e, n_slices);
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < kSimPayload; ++k) { sp[k] = bs[kRansacHead + k]; sum += fabs(bs[kRansacHead + k]); }
        ctl[1] = bs[0] >= 0.0 ? (int)bs[1] : -1;                 // (-1: no valid sample in any slot)
        ctl[2] = (bs[0] >= 0.0 && sum < INFINITY && bs[kRansacHead] > 0.0) ? 1 : 0;      // (s = 0: a sample without a solution)
    }
    __syncthreads();
    const bool has = ctl[2] != 0;
    double mb[kSimPayload];
#pragma unroll
    for (int k = 0; k < kSimPayload; ++k) mb[k] = sp[k];
    // set_inliers, set_success, the status and the refit's pairs all rest on this one evaluation (the count in the slot came
    // from another copy of the expression)
    double c[1] = {0.0};
    for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
        double o[kSimPair];
        sim_pair<false>(g2, k, o);
        const bool inl = has && sim_inlier(mb, o, thr2);
        mk[k] = inl ? 1 : 0; rmk[k] = inl ? 1 : 0;
        c[0] += inl ? 1.0 : 0.0;
    }
    block_sum<1>(c, red);
    if (first) {
        const int cnt = (int)c[0];
        ctl[0] = (has && cnt >= 3) ? kSimOk : kSimDegenerate;
        ctl[3] = cnt;
        // (DEGENERATE still reports the count, h and mask of its best hypothesis; only the similarity is withheld)
        oi[0] = cnt; oi[1] = ctl[1]; oi[2] = ctl[0];
        oi[3] = (ctl[1] >= 0 && (double)cnt / (double)n >= confidence) ? 1 : 0;
        oi[4] = cnt;
    }
    __syncthreads();
    if (ctl[0] != kSimOk) {
        if (threadIdx.x < kSimPayload) { om[threadIdx.x] = 0.0; orf[threadIdx.x] = 0.0; }
        return;
    }
    if (threadIdx.x < kSimPayload) om[threadIdx.x] = sp[threadIdx.x];
    if (!refit) {
        if (threadIdx.x < kSimPayload) orf[threadIdx.x] = sp[threadIdx.x];
        return;
    }
    // the same estimate over the cnt >= 3 inliers: thread t takes pairs t, t + 256, ...; the means first
    const double cnt = (double)ctl[3];
    {
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
            double o[kSimPair];
            sim_pair<false>(g2, k, o);
            if (mk[k]) {
#pragma unroll
                for (int i = 0; i < 6; ++i) v[i] += o[i];
            }
        }
        block_sum<6>(v, red);
        if (first) {
#pragma unroll
            for (int i = 0; i < 6; ++i) sm[i] = v[i] / cnt;
        }
        __syncthreads();
    }
    {
        const double am[3] = {sm[0], sm[1], sm[2]}, bm[3] = {sm[3], sm[4], sm[5]};
        double v[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // S (9), sum |a'|^2
        for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
            double o[kSimPair];
            sim_pair<false>(g2, k, o);
            if (mk[k]) {
                const double ac[3] = {o[0] - am[0], o[1] - am[1], o[2] - am[2]}, bc[3] = {o[3] - bm[0], o[4] - bm[1], o[5] - bm[2]};
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) v[3 * i + j] += ac[i] * bc[j];
                v[9] += ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2];
            }
        }
        block_sum<10>(v, red);
        if (first) {
            const double S[9] = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
            double mr[kSimPayload];
            const bool ok = sim_from_sums(S, v[9], am, bm, mr);
#pragma unroll
            for (int k = 0; k < kSimPayload; ++k) {              // (no solution: a copy of the best)
                const double r = ok ? mr[k] : sp[k];
                orf[k] = r;
                sp[k] = r;
            }
        }
        __syncthreads();
    }
    // refit_mask and its count: the used pairs against the refit as it is returned, the same expression
    double mr[kSimPayload];
#pragma unroll
    for (int k = 0; k < kSimPayload; ++k) mr[k] = sp[k];
    double cr[1] = {0.0};
    for (int k = threadIdx.x; k < n; k += kTwoViewThreads) {
        double o[kSimPair];
        sim_pair<false>(g2, k, o);
        const bool inl = sim_inlier(mr, o, thr2);
        rmk[k] = inl ? 1 : 0;
        cr[0] += inl ? 1.0 : 0.0;
    }
    block_sum<1>(cr, red);
    if (first) oi[4] = (int)cr[0];
}

// ---------------------------------------------------------------------------------------------
// Robust resection (sfmba_resect_ransac): P3P inside RANSAC per selected camera, over its used
// observations in camera-major stored order, then k_resect (start = 1) over the inliers.
//   k_pnp_gather   one workgroup per camera walks its slice of the permutation as k_resect does and compacts the used
//                  observations by ballot prefix, in stored order, into packed correspondences X Y Z u v (40 bytes) with
//                  their stored positions (the others' positions behind them) and their number; it also clears the
//                  camera's part of the inlier mask.  No later kernel of the RANSAC chases entry -> stored position ->
//                  point index -> point again, and k_resect walks the compacted positions as its permutation.
//   k_pnp_ransac   grid over (camera, slice of hypotheses).  Every LANE draws and solves one hypothesis (Grunert's P3P:
//                  the quartic in v = s3 / s1 by Ferrari through the largest root of the resolvent cubic, two Newton
//                  steps, the pose by aligning the two triangles) and leaves its up to four poses in the wave's LDS slab;
//                  the WAVE then scores them one after the other, the lanes striding the camera's correspondences
//                  (staged in LDS up to kPnpLdsObs of them), counts by ballot / popcount.  A workgroup leaves the best
//                  (count, h, solution, pose) of its slice in a slot of its own.
//   k_pnp_finish   one workgroup per camera: best slot (largest count, lowest h), the mask of that pose in stored order
//                  and the count FROM that mask, the pose as six parameters into the camera's row of the call's x, the
//                  byte that selects the camera for k_resect, the integers.
// No atomics: counts do not depend on the order, and the only sums are k_resect's, in its fixed order.
// ---------------------------------------------------------------------------------------------
constexpr int kPnpThreads = 256;
constexpr int kPnpWaves = 4;
constexpr int kPnpLdsObs = 1024;     // a camera of up to this many used observations is staged in LDS (40 KiB)
constexpr int kPnpMinSlice = 64;     // fewest hypotheses of a workgroup's slice (one per lane of one wave)
constexpr int kPnpSlot = 16;         // doubles of a slot: count, h, solution, R (9), T (3), unused
constexpr int kPnpCorr = 5;          // doubles of a packed correspondence
constexpr int kPnpPose = 12;         // R (9, row-major), T (3): x_cam = R (X - T)
constexpr int kPnpSlabDoubles = 4 * kPnpPose * 64;               // a wave's slab: [solution][entry][lane]
constexpr int kPnpOk = 0, kPnpFewViews = 1, kPnpDegenerate = 2, kPnpNotSelected = -1;

__device__ __forceinline__ void pnp_order(double& a, double& b) {
    if (a > b) { const double t = a; a = b; b = t; }
}
// unit vectors e1 = (A2 - A1) / |.|, e3 = e1 x (A3 - A1) normalised, e2 = e3 x e1, as E[3 k + i] = (e_k)_i; -> the sine of
// the angle at A1 (a collinear triple: zero but for rounding)
constexpr double kPnpCollinear = 1e-9;
__device__ __forceinline__ double pnp_frame(const double* A1, const double* A2, const double* A3, double (&E)[9]) {
    const double dx = A2[0] - A1[0], dy = A2[1] - A1[1], dz = A2[2] - A1[2];
    const double n1 = sqrt(dx * dx + dy * dy + dz * dz);
    E[0] = dx / n1; E[1] = dy / n1; E[2] = dz / n1;
    const double fx = A3[0] - A1[0], fy = A3[1] - A1[1], fz = A3[2] - A1[2];
    const double cx = E[1] * fz - E[2] * fy, cy = E[2] * fx - E[0] * fz, cz = E[0] * fy - E[1] * fx;
    const double n3 = sqrt(cx * cx + cy * cy + cz * cz);
    E[6] = cx / n3; E[7] = cy / n3; E[8] = cz / n3;
    E[3] = E[7] * E[2] - E[8] * E[1]; E[4] = E[8] * E[0] - E[6] * E[2]; E[5] = E[6] * E[1] - E[7] * E[0];
    return n3 / sqrt(fx * fx + fy * fy + fz * fz);
}

// Grunert's P3P by one lane: Pw the three points, px their pixels.  The solutions (at most four, ascending in v) go to
// the wave's slab in dynamic LDS, smem[slab + (kPnpPose s + k) 64 + lane]; -> their number.  Anything non-finite is no
// solution.  (LDS is addressed through smem and offsets: a pointer into it that reaches this code as a generic one
// costs a null test per access.)
__device__ __forceinline__ int pnp_p3p(const double (&Pw)[9], const double (&px)[6], const KMat& Kinv, int slab, int lane) {
    extern __shared__ __align__(16) double smem[];
    double j[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double u = px[2 * i], v = px[2 * i + 1];
        const double x = Kinv.k[0] * u + Kinv.k[1] * v + Kinv.k[2], y = Kinv.k[3] * u + Kinv.k[4] * v + Kinv.k[5],
                     z = Kinv.k[6] * u + Kinv.k[7] * v + Kinv.k[8];
        const double nn = sqrt(x * x + y * y + z * z);
        j[3 * i] = x / nn; j[3 * i + 1] = y / nn; j[3 * i + 2] = z / nn;
    }
    const double ca = j[3] * j[6] + j[4] * j[7] + j[5] * j[8], cb = j[0] * j[6] + j[1] * j[7] + j[2] * j[8],
                 cg = j[0] * j[3] + j[1] * j[4] + j[2] * j[5];
    auto dist2 = [&](int a, int b) {
        const double x = Pw[3 * a] - Pw[3 * b], y = Pw[3 * a + 1] - Pw[3 * b + 1], z = Pw[3 * a + 2] - Pw[3 * b + 2];
        return x * x + y * y + z * z;
    };
    const double a2 = dist2(1, 2), b2 = dist2(0, 2), c2 = dist2(0, 1);
    const double p = (a2 - c2) / b2, q = (a2 + c2) / b2;
    const double A4 = (p - 1.0) * (p - 1.0) - 4.0 * (c2 / b2) * ca * ca;
    const double A3 = 4.0 * (p * (1.0 - p) * cb - (1.0 - q) * ca * cg + 2.0 * (c2 / b2) * ca * ca * cb);
    const double A2 = 2.0 * (p * p - 1.0 + 2.0 * p * p * cb * cb + 2.0 * ((b2 - c2) / b2) * ca * ca - 4.0 * q * ca * cb * cg +
                             2.0 * ((b2 - a2) / b2) * cg * cg);
    const double A1 = 4.0 * (-p * (1.0 + p) * cb + 2.0 * (a2 / b2) * cg * cg * cb - (1.0 - q) * ca * cg);
    const double A0 = (1.0 + p) * (1.0 + p) - 4.0 * (a2 / b2) * cg * cg;
    const double b = A3 / A4, c = A2 / A4, d = A1 / A4, e = A0 / A4;
    if (!(fabs(b) + fabs(c) + fabs(d) + fabs(e) < INFINITY)) return 0;
    // depressed quartic y^4 + dp y^2 + dq y + dr with v = y - b / 4
    const double dp = c - 0.375 * b * b;
    const double dq = d - 0.5 * b * c + 0.125 * b * b * b;
    const double dr = e - 0.25 * b * d + 0.0625 * b * b * c - (3.0 / 256.0) * b * b * b * b;
    // resolvent cubic z^3 + 2 dp z^2 + (dp^2 - 4 dr) z - dq^2: its largest real root
    const double B = 2.0 * dp, Cc = dp * dp - 4.0 * dr, D = -dq * dq;
    const double P3 = Cc - B * B / 3.0;
    const double Q3 = 2.0 * B * B * B / 27.0 - B * Cc / 3.0 + D;
    const double disc = 0.25 * Q3 * Q3 + P3 * P3 * P3 / 27.0;
    double w;
    if (disc > 0.0) {
        const double sq = sqrt(disc);
        w = cbrt(-0.5 * Q3 + sq) + cbrt(-0.5 * Q3 - sq);
    } else {
        const double m = sqrt(-P3 / 3.0);
        double arg = m > 0.0 ? 3.0 * Q3 / (2.0 * P3 * m) : 0.0;
        arg = fmin(1.0, fmax(-1.0, arg));
        w = 2.0 * m * cos(acos(arg) / 3.0);
    }
    const double z = w - B / 3.0;
    if (!(z > 0.0)) return 0;
    const double s = sqrt(z), qs = dq / s;
    const double t1 = 0.5 * (dp + z - qs), t2 = 0.5 * (dp + z + qs);
    const double d1 = z - 4.0 * t1, d2 = z - 4.0 * t2;
    double r0 = INFINITY, r1 = INFINITY, r2 = INFINITY, r3 = INFINITY;
    if (d1 >= 0.0) { const double rt = sqrt(d1); r0 = 0.5 * (-s - rt) - 0.25 * b; r1 = 0.5 * (-s + rt) - 0.25 * b; }
    if (d2 >= 0.0) { const double rt = sqrt(d2); r2 = 0.5 * (s - rt) - 0.25 * b; r3 = 0.5 * (s + rt) - 0.25 * b; }
    auto newton = [&](double v) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const double f = (((v + b) * v + c) * v + d) * v + e;
            const double fp = ((4.0 * v + 3.0 * b) * v + 2.0 * c) * v + d;
            v = v - f / fp;
        }
        return fabs(v) < INFINITY ? v : INFINITY;                // (a NaN as well)
    };
    r0 = newton(r0); r1 = newton(r1); r2 = newton(r2); r3 = newton(r3);
    pnp_order(r0, r1); pnp_order(r2, r3); pnp_order(r0, r2); pnp_order(r1, r3); pnp_order(r1, r2);
    double EP[9];
    if (!(pnp_frame(&Pw[0], &Pw[3], &Pw[6], EP) > kPnpCollinear)) return 0;      // (a repeated point: NaN)
    int ns = 0;
    auto solution = [&](double v) {
        const double u = ((p - 1.0) * v * v - 2.0 * p * cb * v + 1.0 + p) / (2.0 * (cg - v * ca));
        if (!(v > 0.0 && u > 0.0 && u < INFINITY && v < INFINITY)) return;
        const double s1 = sqrt(b2 / (1.0 + v * v - 2.0 * v * cb)), s2 = u * s1, s3 = v * s1;
        const double Q[9] = {s1 * j[0], s1 * j[1], s1 * j[2], s2 * j[3], s2 * j[4], s2 * j[5], s3 * j[6], s3 * j[7], s3 * j[8]};
        double EQ[9], R[9];
        pnp_frame(&Q[0], &Q[3], &Q[6], EQ);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) R[3 * i + k] = EQ[i] * EP[k] + EQ[3 + i] * EP[3 + k] + EQ[6 + i] * EP[6 + k];
        const double T0 = Pw[0] - (R[0] * Q[0] + R[3] * Q[1] + R[6] * Q[2]), T1 = Pw[1] - (R[1] * Q[0] + R[4] * Q[1] + R[7] * Q[2]),
                     T2 = Pw[2] - (R[2] * Q[0] + R[5] * Q[1] + R[8] * Q[2]);
        double sum = fabs(T0) + fabs(T1) + fabs(T2);
#pragma unroll
        for (int k = 0; k < 9; ++k) sum += fabs(R[k]);
        if (!(sum < INFINITY)) return;
        const int dst = slab + kPnpPose * ns * 64 + lane;
#pragma unroll
        for (int k = 0; k < 9; ++k) smem[dst + 64 * k] = R[k];
        smem[dst + 64 * 9] = T0; smem[dst + 64 * 10] = T1; smem[dst + 64 * 11] = T2;
        ++ns;
    };
#pragma unroll 1
    for (int i = 0; i < 4; ++i) solution(i == 0 ? r0 : (i == 1 ? r1 : (i == 2 ? r2 : r3)));   // (selects: an indexed array would live in scratch)
    return ns;
}

// |pi(K R (X - T)) - uv|^2 of one correspondence at the pose ps (R | T); depth: the third entry of R (X - T)
__device__ __forceinline__ double pnp_err2(const double (&ps)[kPnpPose], const KMat& K, double X, double Y, double Z, double u,
                                           double v, double& depth) {
    const double vx = X - ps[9], vy = Y - ps[10], vz = Z - ps[11];
    const double qx = ps[0] * vx + ps[1] * vy + ps[2] * vz, qy = ps[3] * vx + ps[4] * vy + ps[5] * vz,
                 qz = ps[6] * vx + ps[7] * vy + ps[8] * vz;
    const double pxx = K.k[0] * qx + K.k[1] * qy + K.k[2] * qz, pyy = K.k[3] * qx + K.k[4] * qy + K.k[5] * qz,
                 pzz = K.k[6] * qx + K.k[7] * qy + K.k[8] * qz;
    const double iz = 1.0 / pzz;
    const double rx = pxx * iz - u, ry = pyy * iz - v;
    depth = qz;
    return rx * rx + ry * ry;
}
// the score's test: squared error STRICTLY below thr2 and depth above min_depth; a non-finite value is no inlier
__device__ __forceinline__ bool pnp_inlier(const double (&ps)[kPnpPose], const KMat& K, const double* __restrict__ o, double thr2,
                                           double min_depth) {
    double depth;
    const double e2 = pnp_err2(ps, K, o[0], o[1], o[2], o[3], o[4], depth);
    return e2 < thr2 && e2 < INFINITY && depth > min_depth;
}

struct PnpIn {
    const double* __restrict__ corr;             // [N][5] packed per camera from cam_ptr[c] on
    const int* __restrict__ cam_ptr;             // [C + 1]
    const int* __restrict__ cn;                  // [C] used observations (0: not selected)
    const int* __restrict__ samples;             // [C][H][3] positions among the used observations, or null: drawn
};
struct PnpScore { double thr2, min_depth; int need; };

// the hypotheses h0 + 64 w + lane, + 256, ... < h1 of camera c, one per lane; the camera's correspondences are staged
// in LDS behind the slabs (LDS_OBS) or read at go.  Leaves the wave's best (count, h, solution, pose) on every lane.
template <bool LDS_OBS>
__device__ __forceinline__ void pnp_slice(const double* __restrict__ go, const PnpIn& in, int c, int n, int H, int h0, int h1,
                                          unsigned long long seed, const KMat& K, const KMat& Kinv, const PnpScore& sc,
                                          int* __restrict__ hyp, int& bc, int& bh, int& bs, double (&bp)[kPnpPose]) {
    extern __shared__ __align__(16) double smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int slab = w * kPnpSlabDoubles;
    const auto obs = [&](int k, double (&o)[kPnpCorr]) {
#pragma unroll
        for (int i = 0; i < kPnpCorr; ++i) o[i] = LDS_OBS ? smem[kPnpWaves * kPnpSlabDoubles + kPnpCorr * k + i] : go[(size_t)kPnpCorr * k + i];
    };
    bc = -2; bh = 0x7fffffff; bs = -1;
#pragma unroll
    for (int k = 0; k < kPnpPose; ++k) bp[k] = 0.0;
#pragma unroll 1
    for (int hb = h0 + 64 * w; hb < h1; hb += 64 * kPnpWaves) {  // uniform over the wave
        const int h = hb + lane;
        int ns = 0, hcount = -1, hsol = -1;
        if (h < h1) {
            int idx[3];
            const bool valid = ransac_sample(in.samples, c, H, h, n, seed, idx);
            if (valid) {
                double Pw[9], px[6];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double o[kPnpCorr];
                    obs(idx[k], o);
                    Pw[3 * k] = o[0]; Pw[3 * k + 1] = o[1]; Pw[3 * k + 2] = o[2]; px[2 * k] = o[3]; px[2 * k + 1] = o[4];
                }
                hcount = 0;
                ns = pnp_p3p(Pw, px, Kinv, slab, lane);
            }
        }
        __builtin_amdgcn_wave_barrier();                         // (one wave: its LDS operations execute in program order)
        for (unsigned long long todo = __ballot(ns > 0); todo; todo &= todo - 1) {
            const int l = __ffsll((long long)todo) - 1;
            const int nl = __builtin_amdgcn_readlane(ns, l);
#pragma unroll 1
            for (int s = 0; s < nl; ++s) {
                double ps[kPnpPose];
#pragma unroll
                for (int k = 0; k < kPnpPose; ++k) ps[k] = smem[slab + (kPnpPose * s + k) * 64 + l];
                int cnt = 0;
#pragma unroll 1
                for (int k0 = 0; k0 < n; k0 += 64) {             // uniform over the wave: the ballot needs every lane
                    const int k = k0 + lane;
                    bool inl = false;
                    if (k < n) {
                        double o[kPnpCorr];
                        obs(k, o);
                        inl = pnp_inlier(ps, K, o, sc.thr2, sc.min_depth);
                    }
                    cnt += __popcll(__ballot(inl));
                }
                if (lane == l && (hsol < 0 || cnt > hcount)) { hcount = cnt; hsol = s; }   // the lowest solution of equal counts
            }
        }
        if (h < h1 && hyp != nullptr) hyp[(size_t)c * (size_t)H + (size_t)h] = hcount;
        // the round's best: the largest count, the lowest lane (h) among equals; rounds ascend in h
        const int top = wave_reduce_xor(h < h1 ? hcount : -2, [](int a, int b) { return max(a, b); });
        if (top > bc) {
            const int lb = __ffsll((long long)__ballot(h < h1 && hcount == top)) - 1;
            bc = top; bh = hb + lb; bs = __builtin_amdgcn_readlane(hsol, lb);
            if (bs >= 0) {
#pragma unroll
                for (int k = 0; k < kPnpPose; ++k) bp[k] = smem[slab + (kPnpPose * bs + k) * 64 + lb];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// dynamic LDS: the four waves' slabs, then the camera's correspondences when they fit
__global__ __launch_bounds__(kPnpThreads) void k_pnp_ransac(PnpIn in, int H, int hs, int n_slices, unsigned long long seed,
                                                            KMat K, KMat Kinv, PnpScore sc, double* __restrict__ slots,
                                                            int* __restrict__ hyp) {
    extern __shared__ __align__(16) double smem[];
    __shared__ double wbest[kPnpWaves][kPnpSlot];
    const int c = blockIdx.x / n_slices, sl = blockIdx.x - c * n_slices;
    const int b = in.cam_ptr[c], n = in.cn[c];
    const int h0 = sl * hs, h1 = min(H, h0 + hs);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double* __restrict__ slot = slots + (size_t)blockIdx.x * kPnpSlot;
    if (n < sc.need) {                                           // (uniform over the workgroup) no hypothesis
        if (hyp != nullptr)
            for (int h = h0 + (int)threadIdx.x; h < h1; h += kPnpThreads) hyp[(size_t)c * (size_t)H + (size_t)h] = -1;
        if (threadIdx.x < kPnpSlot) slot[threadIdx.x] = threadIdx.x == 0 ? -2.0 : (threadIdx.x == 2 ? -1.0 : 0.0);
        return;
    }
    const double* __restrict__ go = in.corr + (size_t)kPnpCorr * (size_t)b;
    int bc, bh, bs;
    double bp[kPnpPose];
    if (n <= kPnpLdsObs) {
        for (int k = threadIdx.x; k < kPnpCorr * n; k += kPnpThreads) smem[kPnpWaves * kPnpSlabDoubles + k] = go[k];
        __syncthreads();
        pnp_slice<true>(go, in, c, n, H, h0, h1, seed, K, Kinv, sc, hyp, bc, bh, bs, bp);
    } else {
        pnp_slice<false>(go, in, c, n, H, h0, h1, seed, K, Kinv, sc, hyp, bc, bh, bs, bp);
    }
    if (lane == 0) {
        wbest[w][0] = (double)bc; wbest[w][1] = (double)bh; wbest[w][2] = (double)bs;
#pragma unroll
        for (int k = 0; k < kPnpPose; ++k) wbest[w][3 + k] = bp[k];
        wbest[w][15] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < kPnpSlot) {
        int best = 0;
        for (int k = 1; k < kPnpWaves; ++k)
            if (wbest[k][0] > wbest[best][0] || (wbest[k][0] == wbest[best][0] && wbest[k][1] < wbest[best][1])) best = k;
        slot[threadIdx.x] = wbest[best][threadIdx.x];
    }
}

template <bool F32>
__global__ __launch_bounds__(kPnpThreads) void k_pnp_gather(ResectIn in, int C, double* __restrict__ corr, int* __restrict__ cpos,
                                                            int* __restrict__ cn, unsigned char* __restrict__ mask) {
    __shared__ int wcnt[2 * kPnpWaves];
    const int c = blockIdx.x;
    const int b = in.cam_ptr[c], e = in.cam_ptr[c + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double* __restrict__ pts = in.x + 6 * (size_t)C;
    const bool sel = in.select == nullptr || in.select[c] != 0;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int base = 0, rest = 0;
#pragma unroll 1
    for (int j0 = b; j0 < e; j0 += kPnpThreads) {                // uniform over the workgroup
        const int j = j0 + (int)threadIdx.x;
        const int idx = j < e ? in.perm[j] : -1;
        const bool on = idx >= 0 && sel && (in.use == nullptr || in.use[idx] != 0);
        const bool out = idx >= 0 && !on;
        if (idx >= 0) mask[idx] = 0;
        const unsigned long long m = __ballot(on), mo = __ballot(out);
        if (lane == 0) { wcnt[w] = __popcll(m); wcnt[kPnpWaves + w] = __popcll(mo); }
        __syncthreads();
        int off = base + __popcll(m & below), tot = 0, offo = rest + __popcll(mo & below), toto = 0;
#pragma unroll
        for (int k = 0; k < kPnpWaves; ++k) {
            off += k < w ? wcnt[k] : 0; tot += wcnt[k];
            offo += k < w ? wcnt[kPnpWaves + k] : 0; toto += wcnt[kPnpWaves + k];
        }
        // the observations that take no part fill the slice from its end: their mask byte stays 0, so k_resect, walking
        // cpos as its permutation, meets the used ones first and in stored order -- thread for thread what it meets in the
        // problem without the others
        if (out) cpos[e - 1 - offo] = idx;
        rest += toto;
        if (on) {
            const int p = in.pt_idx[idx];
            const double2 q = load_pair(in.uv, F32, idx);
            const double* __restrict__ Xp = pts + 3 * (size_t)p;
            double* __restrict__ dst = corr + (size_t)kPnpCorr * (size_t)(b + off);
            dst[0] = Xp[0]; dst[1] = Xp[1]; dst[2] = Xp[2]; dst[3] = q.x; dst[4] = q.y;
            cpos[b + off] = idx;
        }
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) cn[c] = base;
}

// the rotation vector of R through the quaternion, the largest component first (as resect_pose_from_h ends)
__device__ __forceinline__ void pnp_rotvec(const double* R, double* w) {
    const double tr = R[0] + R[4] + R[8];
    double qw, qx, qy, qz;
    if (tr > 0.0) {
        const double s = sqrt(tr + 1.0) * 2.0;
        qw = 0.25 * s; qx = (R[7] - R[5]) / s; qy = (R[2] - R[6]) / s; qz = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
        qw = (R[7] - R[5]) / s; qx = 0.25 * s; qy = (R[1] + R[3]) / s; qz = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
        qw = (R[2] - R[6]) / s; qx = (R[1] + R[3]) / s; qy = 0.25 * s; qz = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
        qw = (R[3] - R[1]) / s; qx = (R[2] + R[6]) / s; qy = (R[5] + R[7]) / s; qz = 0.25 * s;
    }
    if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    const double n = sqrt(qx * qx + qy * qy + qz * qz);
    const double f = n < 1e-12 ? 2.0 : 2.0 * atan2(n, qw) / n;
    w[0] = qx * f; w[1] = qy * f; w[2] = qz * f;
}

struct PnpOut {
    double* __restrict__ x;                      // the call's parameter vector: the best pose goes into the camera's row
    double* __restrict__ hyp;                    // [C][6]
    unsigned char* __restrict__ mask;            // [N] stored order
    unsigned char* __restrict__ ok;              // [C] k_resect's select mask: RANSAC succeeded
    int* __restrict__ ints;                      // [C][6] status, views, inliers, best h, best solution, success
};

__global__ __launch_bounds__(kPnpThreads) void k_pnp_finish(PnpIn in, const int* __restrict__ cpos,
                                                            const unsigned char* __restrict__ select, int n_slices, KMat K,
                                                            PnpScore sc, double confidence, const double* __restrict__ slots,
                                                            PnpOut out) {
    __shared__ double red[kPnpWaves];
    __shared__ double sp[kPnpPose];
    __shared__ int ctl[3];
    const int c = blockIdx.x;
    const int b = in.cam_ptr[c], n = in.cn[c];
    const bool first = threadIdx.x == 0;
    const bool sel = select == nullptr || select[c] != 0;
    int* __restrict__ oi = out.ints + 6 * (size_t)c;
    if (!sel || n < sc.need) {                                   // (uniform over the workgroup; k_pnp_gather cleared the mask)
        if (first) {
            oi[0] = sel ? kPnpFewViews : kPnpNotSelected; oi[1] = n; oi[2] = 0; oi[3] = -1; oi[4] = -1; oi[5] = 0;
            out.ok[c] = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) out.hyp[6 * (size_t)c + k] = out.x[6 * (size_t)c + k];
        }
        return;
    }
    if (first) {
        const double* __restrict__ sl = slots + (size_t)c * (size_t)n_slices * kPnpSlot;
        int best = 0;
        for (int k = 1; k < n_slices; ++k)                       // slots ascend in h: the first of equal counts has the lowest
            if (sl[(size_t)k * kPnpSlot] > sl[(size_t)best * kPnpSlot]) best = k;
        const double* __restrict__ bs = sl + (size_t)best * kPnpSlot;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < kPnpPose; ++k) { sp[k] = bs[3 + k]; sum += fabs(bs[3 + k]); }
        const bool any = bs[0] >= 0.0;                           // (below: no valid sample in any slot)
        ctl[0] = (any && bs[2] >= 0.0 && sum < INFINITY) ? 1 : 0;
        ctl[1] = any ? (int)bs[1] : -1;
        ctl[2] = any ? (int)bs[2] : -1;
    }
    __syncthreads();
    const bool has = ctl[0] != 0;
    double ps[kPnpPose];
#pragma unroll
    for (int k = 0; k < kPnpPose; ++k) ps[k] = sp[k];
    // The mask of the best pose, and the count FROM that mask: cam_inliers, cam_success, the status and k_resect's input
    // all rest on this one evaluation (the count in the slot came from another copy of the expression).
    const double* __restrict__ go = in.corr + (size_t)kPnpCorr * (size_t)b;
    double cs[1] = {0.0};
    for (int k = threadIdx.x; k < n; k += kPnpThreads) {
        const bool inl = has && pnp_inlier(ps, K, go + (size_t)kPnpCorr * k, sc.thr2, sc.min_depth);
        out.mask[cpos[b + k]] = inl ? 1 : 0;
        cs[0] += inl ? 1.0 : 0.0;
    }
    block_sum<1>(cs, red);
    if (first) {
        const int cnt = (int)cs[0];
        const bool ok = has && cnt >= sc.need;
        oi[0] = ok ? kPnpOk : kPnpDegenerate; oi[1] = n; oi[2] = cnt; oi[3] = ctl[1]; oi[4] = ctl[2];
        oi[5] = (has && (double)cnt / (double)n >= confidence) ? 1 : 0;
        out.ok[c] = ok ? 1 : 0;
        double prm[6];
        if (has) {
            pnp_rotvec(ps, prm);
            prm[3] = ps[9]; prm[4] = ps[10]; prm[5] = ps[11];
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) prm[k] = out.x[6 * (size_t)c + k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            out.hyp[6 * (size_t)c + k] = prm[k];
            if (ok) out.x[6 * (size_t)c + k] = prm[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Robust triangulation (sfmba_triangulate_ransac): per selected point, hypotheses from PAIRS of its
// used observations -- all of them in lexicographic order while there are at most H (tri_pair_unrank), else H drawn by the
// counter rule with two draws (ransac_sample<2>) --, each the two-view case of the n-view DLT above (tri_dlt_rows twice,
// smallest_eigenvector4) and scored over every used observation of the point; the largest count wins, the lowest h among
// equals; the best is evaluated once more for the mask.  k_triangulate then runs over the mask (launch_triangulate).
//   k_tri_ransac   a workgroup takes kTriRansacThreads consecutive points, one per thread.  SHORT runs (fewer than
//                  kStatsLongTrack stored observations): the points' hypothesis numbers m_p are scanned over the
//                  workgroup (track_block_scan) and the hypotheses handed out ONE PER LANE in rounds of the workgroup's
//                  width -- a lane finds its point by bisection of the prefix array in LDS --, so a wave is full whatever
//                  the mix of track lengths (a lane per point would wait for the longest track with the Jacobi state idle
//                  in 63 lanes, a wave per point wastes it below 12 views).  A lane leaves its count in LDS; after
//                  a round the point's own thread walks its piece of the round in ascending h and keeps the first
//                  largest, then evaluates that hypothesis again: X_hyp, the mask in stored order, the count from the mask.
//                  LONG runs are taken by the wave afterwards, one after the other (for_each_long_run): lanes are
//                  hypotheses, every lane walks the same observations (uniform addresses), the wave's best by a maximum
//                  and a ballot, the mask by lanes striding the run.
// A hypothesis is computed by one lane from the point's own inputs in both forms and counts are integers: a point's
// results do not depend on its chunk, round, wave or neighbours.  No atomics.
// ---------------------------------------------------------------------------------------------
constexpr int kTriRansacThreads = 256;
static_assert(kTriRansacThreads == kTrackBlock, "track_block_scan scans a workgroup of kTrackBlock threads");
static_assert((long long)kTriRansacThreads * (kStatsLongTrack - 1) * (kStatsLongTrack - 2) / 2 < (1ll << 31),
              "the hypotheses of a chunk's short runs are numbered with an int");
constexpr int kTriNoConsensus = 6;
constexpr size_t kTriRansacStaticLds = 4096;     // room for k_tri_ransac's static LDS (prefix, used counts, a round's counts, the scan's sums)
struct TriRansacOptions { int H, need; double thr2, min_depth, min_pair_angle_deg; unsigned long long seed; };
struct TriRansacOut {
    double* __restrict__ X_hyp;                  // [P][3]
    unsigned char* __restrict__ mask;            // [N] stored order; ZERO on entry: only a valid best hypothesis writes its run
    unsigned char* __restrict__ ok;              // [P] the best count reaches the need: k_triangulate's select
    int* __restrict__ status;                    // [P] -1, FEW_VIEWS, NO_CONSENSUS, or 0: k_triangulate's verdict counts
    int* __restrict__ views;
    int* __restrict__ inliers;
    int* __restrict__ best;
    int* __restrict__ hyp;                       // [P][H], -1 on entry, or null
};
struct TriRansacResult { int status, views, inliers, best; double X, Y, Z; };

// stored position of the i-th used observation of the run [b, e)
__device__ __forceinline__ int tri_used_position(const TriIn& in, int b, int e, int i) {
    if (in.use == nullptr) return b + i;
    int k = b;
#pragma unroll 1
    for (; k < e; ++k)
        if (in.use[k] && i-- == 0) break;
    return k;
}

// The point of the observations stored at ka and kb (in this order): false when it is not valid -- not finite,
// |w3| <= 1e-12 |w|, a depth of the two at most min_depth, or the angle between the two rays below the limit.
template <bool F32>
__device__ __forceinline__ bool tri_pair_point(const double* __restrict__ rt, const TriIn& in, const KMat& K, int ka, int kb,
                                               const TriRansacOptions& o, double& X, double& Y, double& Z) {
    constexpr double kDeg = 57.295779513082320877;
    double a[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) a[q] = 0.0;
    tri_dlt_rows<F32>(rt, in, ka, K, a);
    tri_dlt_rows<F32>(rt, in, kb, K, a);
    double w0, w1, w2, w3;
    smallest_eigenvector4(a, w0, w1, w2, w3);
    const double nw = sqrt(w0 * w0 + w1 * w1 + w2 * w2 + w3 * w3);
    X = w0 / w3; Y = w1 / w3; Z = w2 / w3;
    if (!(fabs(w3) > 1e-12 * nw)) return false;                  // (false for a NaN as well)
    if (!(fabs(X) + fabs(Y) + fabs(Z) < INFINITY)) return false;
    const double* __restrict__ ra = rt + (size_t)in.cam_idx[ka] * kCamRT;
    const double* __restrict__ rb = rt + (size_t)in.cam_idx[kb] * kCamRT;
    if (!(cam_depth(ra, X, Y, Z) > o.min_depth && cam_depth(rb, X, Y, Z) > o.min_depth)) return false;
    const double ax = X - ra[9], ay = Y - ra[10], az = Z - ra[11], bx = X - rb[9], by = Y - rb[10], bz = Z - rb[11];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double ang = kDeg * atan2(sqrt(cx * cx + cy * cy + cz * cz), ax * bx + ay * by + az * bz);
    return ang >= o.min_pair_angle_deg;
}

// used observations of [b, e), every step-th from b + first, with squared error strictly below thr2 and depth above
// min_depth at (X, Y, Z); WRITE: each one's verdict into mask
template <bool F32, bool WRITE>
__device__ __forceinline__ int tri_count_inliers(const double* __restrict__ rt, const TriIn& in, const KMat& K, int b, int e,
                                                 int first, int step, double X, double Y, double Z, const TriRansacOptions& o,
                                                 unsigned char* __restrict__ mask) {
    int count = 0;
#pragma unroll 1
    for (int k = b + first; k < e; k += step) {
        if (in.use != nullptr && !in.use[k]) continue;
        double tl[kCamRow];
        tri_load_row(rt, in.cam_idx[k], tl);
        const double2 px = load_pair(in.uv, F32, k);
        double rx, ry;
        observe<false>(tl, X, Y, Z, px.x, px.y, K, rx, ry, nullptr, nullptr);
        const bool inl = rx * rx + ry * ry < o.thr2 && cam_depth(tl, X, Y, Z) > o.min_depth;     // (a NaN: no inlier)
        if (WRITE) mask[k] = inl ? 1 : 0;
        count += inl ? 1 : 0;
    }
    return count;
}

// the pair of hypothesis h of point p with n used observations in [b, e): stored positions, in the hypothesis' order
__device__ __forceinline__ void tri_hypothesis_pair(const TriIn& in, const TriRansacOptions& o, int p, int b, int e, int n, int h,
                                                    int& ka, int& kb) {
    int i, j;
    if (tri_pair_count(n) <= (long long)o.H) {
        tri_pair_unrank(n, h, i, j);
    } else {
        int idx[2];
        ransac_sample<2>(nullptr, p, o.H, h, n, o.seed, idx);
        i = idx[0]; j = idx[1];
    }
    ka = tri_used_position(in, b, e, i);
    kb = tri_used_position(in, b, e, j);
}

// count of hypothesis h (0: its point is not valid)
template <bool F32>
__device__ __forceinline__ int tri_hypothesis(const double* __restrict__ rt, const TriIn& in, const KMat& K,
                                              const TriRansacOptions& o, int p, int b, int e, int n, int h) {
    int ka, kb;
    tri_hypothesis_pair(in, o, p, b, e, n, h, ka, kb);
    double X, Y, Z;
    if (!tri_pair_point<F32>(rt, in, K, ka, kb, o, X, Y, Z)) return 0;
    return tri_count_inliers<F32, false>(rt, in, K, b, e, 0, 1, X, Y, Z, o, nullptr);
}

// hypotheses of a point with n used observations (0: fewer than the need)
__device__ __forceinline__ int tri_hypotheses(const TriRansacOptions& o, int n) {
    return n < o.need ? 0 : (int)min(tri_pair_count(n), (long long)o.H);
}

template <bool LDS_TAB, bool F32>
__global__ __launch_bounds__(kTriRansacThreads) void k_tri_ransac(const double* __restrict__ camtab, TriIn in, int P, int C, KMat K,
                                                                  TriRansacOptions o, TriRansacOut out) {
    extern __shared__ __align__(16) double smem[];
    __shared__ int pre[kTriRansacThreads + 1];                   // exclusive scan of the chunk's hypothesis numbers
    __shared__ int nus[kTriRansacThreads];                       // used observations of the chunk's points
    __shared__ int cnt[kTriRansacThreads];                       // the counts of a round
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const double* __restrict__ rt_global = camtab + cam_rt_offset(C);
    if (LDS_TAB) stage_table(rt_global, C * kCamRT, smem);
    const double* __restrict__ rt = LDS_TAB ? smem : rt_global;
    for (int base = blockIdx.x * kTriRansacThreads; base < P; base += gridDim.x * kTriRansacThreads) {     // uniform over the workgroup
        const int p = base + tid;
        int b = 0, e = 0;
        double X0 = 0.0, Y0 = 0.0, Z0 = 0.0;
        bool sel = false;
        if (p < P) {
            b = in.pt_ptr[p]; e = in.pt_ptr[p + 1];
            X0 = in.pts[3 * (size_t)p]; Y0 = in.pts[3 * (size_t)p + 1]; Z0 = in.pts[3 * (size_t)p + 2];
            sel = in.select == nullptr || in.select[p] != 0;
        }
        const bool is_long = sel && e - b >= kStatsLongTrack;
        TriRansacResult r;
        r.status = kTriNotSelected; r.views = 0; r.inliers = 0; r.best = -1;
        r.X = X0; r.Y = Y0; r.Z = Z0;
        // ---- short runs: one hypothesis per lane
        int n = 0;
        if (sel && !is_long) {
            n = e - b;
            if (in.use != nullptr) {
                n = 0;
                for (int k = b; k < e; ++k) n += in.use[k] ? 1 : 0;
            }
            r.views = n;
            r.status = kTriFewViews;
        }
        const int m = sel && !is_long ? tri_hypotheses(o, n) : 0;
        long long c_ex, s_ex, c_tot, s_tot;
        track_block_scan(m ? 1 : 0, m, c_ex, s_ex, c_tot, s_tot);
        const int mine = (int)s_ex, total = (int)s_tot;
        pre[tid] = mine;
        nus[tid] = n;
        if (tid == 0) pre[kTriRansacThreads] = total;
        __syncthreads();
        int bc = -1, bh = 0;                                     // the point's best so far: count, h
        for (int r0 = 0; r0 < total; r0 += kTriRansacThreads) {  // (uniform over the workgroup)
            const int g = r0 + tid;
            int c = 0;
            if (g < total) {
                int lo = 0, hi = kTriRansacThreads;              // pre[lo] <= g < pre[hi]: the last lo has hypotheses
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (pre[mid] <= g) lo = mid; else hi = mid;
                }
                const int q = base + lo, h = g - pre[lo];
                c = tri_hypothesis<F32>(rt, in, K, o, q, in.pt_ptr[q], in.pt_ptr[q + 1], nus[lo], h);
                if (out.hyp != nullptr) out.hyp[(size_t)q * (size_t)o.H + (size_t)h] = c;
            }
            cnt[tid] = c;
            __syncthreads();
            const int g0 = max(mine, r0), g1 = min(mine + m, r0 + kTriRansacThreads);
            for (int k = g0; k < g1; ++k) {                      // ascending h: only a larger count replaces
                const int ck = cnt[k - r0];
                if (ck > bc) { bc = ck; bh = k - mine; }
            }
            __syncthreads();
        }
        if (m > 0) {
            int ka, kb;
            tri_hypothesis_pair(in, o, p, b, e, n, bh, ka, kb);
            double X, Y, Z;
            const bool valid = tri_pair_point<F32>(rt, in, K, ka, kb, o, X, Y, Z);
            r.best = bh;
            if (valid) {
                r.inliers = tri_count_inliers<F32, true>(rt, in, K, b, e, 0, 1, X, Y, Z, o, out.mask);
                r.X = X; r.Y = Y; r.Z = Z;
            }
            r.status = valid && r.inliers >= o.need ? kTriOk : kTriNoConsensus;
        }
        // ---- long runs: the wave, lanes are hypotheses
        for_each_long_run(is_long, b, e, X0, Y0, Z0, [&](int ql, int qb, int qe, double qX, double qY, double qZ) {
            const int q = base + (tid - lane) + ql;
            TriRansacResult w;
            w.status = kTriFewViews; w.inliers = 0; w.best = -1;
            w.X = qX; w.Y = qY; w.Z = qZ;
            int nq = qe - qb;
            if (in.use != nullptr) {
                nq = 0;
                for (int k = qb + lane; k < qe; k += 64) nq += in.use[k] ? 1 : 0;
                nq = wave_isum(nq);
            }
            w.views = nq;
            const int mq = tri_hypotheses(o, nq);
            if (mq > 0) {
                int wc = -1, wh = 0;
                for (int hb = 0; hb < mq; hb += 64) {
                    const int h = hb + lane;
                    int c = -2;
                    if (h < mq) {
                        c = tri_hypothesis<F32>(rt, in, K, o, q, qb, qe, nq, h);
                        if (out.hyp != nullptr) out.hyp[(size_t)q * (size_t)o.H + (size_t)h] = c;
                    }
                    const int top = wave_reduce_xor(c, [](int x, int y) { return max(x, y); });
                    if (top > wc) { wc = top; wh = hb + __ffsll((long long)__ballot(c == top)) - 1; }
                }
                int ka, kb;
                tri_hypothesis_pair(in, o, q, qb, qe, nq, wh, ka, kb);
                double X, Y, Z;
                const bool valid = tri_pair_point<F32>(rt, in, K, ka, kb, o, X, Y, Z);    // (every lane alike)
                w.best = wh;
                if (valid) {
                    w.inliers = wave_isum(tri_count_inliers<F32, true>(rt, in, K, qb, qe, lane, 64, X, Y, Z, o, out.mask));
                    w.X = X; w.Y = Y; w.Z = Z;
                }
                w.status = valid && w.inliers >= o.need ? kTriOk : kTriNoConsensus;
            }
            if (lane == ql) r = w;
        });
        if (p < P) {
            out.X_hyp[3 * (size_t)p] = r.X; out.X_hyp[3 * (size_t)p + 1] = r.Y; out.X_hyp[3 * (size_t)p + 2] = r.Z;
            out.status[p] = r.status; out.views[p] = r.views; out.inliers[p] = r.inliers; out.best[p] = r.best;
            out.ok[p] = r.status == kTriOk ? 1 : 0;
        }
    }
}

}  // namespace sfmba
