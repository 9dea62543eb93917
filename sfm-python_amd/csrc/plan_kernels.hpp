// View planning and problem assembly (sfmba_plan_views, sfmba_assemble_problem, sfmba_get_assembled): sweeps over what
// sfmba_build_tracks left on the device -- feat_track (image-major) and the CSR track_ptr / track_feat / track_image
// (point-major) -- under the caller's masks.  DESIGN.md section 25.
//
// Every output is an integer (or a copied double), every sum an integer sum, and every place an entry is written to
// comes from an exclusive scan: the same input gives the same bits whatever the grid and the schedule.  The only atomics
// are integer adds into the totals block.  Indices are 32-bit into features, tracks and images, 64-bit into observations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kPlanBlock = 256;                  // threads of every workgroup here
constexpr int kPlanLong = 32;                    // a lane walks a track shorter than this, the wave a longer one
// The scan is the feature tracks' (track_scan.hpp).  Its three sizes as track_kernels.hpp defines them: the middle launch
// is compiled there, launch_k_track_scan_sums compares, and tests/test_host_plan.py reads both files.
constexpr int kTrackBlock = 256;
constexpr int kTrackScanPerThread = 4;
constexpr int kTrackScanItems = 1024;
static_assert(kTrackScanItems == kTrackBlock * kTrackScanPerThread, "a thread scans kTrackScanPerThread consecutive entries");
#include "track_scan.hpp"

// slots of the totals block (long long): zeroed by every call; a scan writes its slot and the one behind it
constexpr int kPlanTotReg = 0, kPlanTotKnown = 1, kPlanTotReady = 2;      // sfmba_plan_views
constexpr int kPlanTotPoints = 3, kPlanTotObs = 4, kPlanTotCams = 5;      // sfmba_assemble_problem (6: the camera scan's sum)
constexpr int kPlanTotSlots = 8;

// The number of observations of a lane's track [b, b + n) whose image has mask != 0.  The long-run pattern of
// k_track_sort: a lane counts a track shorter than kPlanLong by itself; the longer ones of the wave's 64 tracks are
// taken by the whole wave afterwards, one after the other.  Every lane of the wave calls this (an idle one with
// active = false).
__device__ __forceinline__ int plan_count_views(bool active, long long b, int n, const int* __restrict__ track_image,
                                                const unsigned char* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    if (active && n < kPlanLong)
        for (int k = 0; k < n; ++k) cnt += mask[track_image[b + k]] != 0;
    unsigned long long todo = __ballot(active && n >= kPlanLong);
    while (todo) {
        const int q = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long qb = __shfl(b, q);
        const int qn = __shfl(n, q);
        int c = 0;
        for (int k = lane; k < qn; k += 64) c += mask[track_image[qb + k]] != 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
        if (lane == q) cnt = c;
    }
    return cnt;
}

// sums of three ints over the workgroup, valid in thread 0
__device__ __forceinline__ void plan_block_sum3(int& a, int& b, int& c) {
    __shared__ int part[kPlanBlock / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); c += __shfl_xor(c, d); }
    if (lane == 0) { part[wave][0] = a; part[wave][1] = b; part[wave][2] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = c = 0;
#pragma unroll
        for (int w = 0; w < kPlanBlock / 64; ++w) { a += part[w][0]; b += part[w][1]; c += part[w][2]; }
    }
    __syncthreads();                                            // (the array is free for the next call)
}

// ---- sfmba_plan_views ----------------------------------------------------------------------------------------------------
// one lane per track: the registered images among its views; the known tracks and the unknown ones with two registered
// views or more are counted by the wave and added to the totals
__global__ __launch_bounds__(kPlanBlock) void k_plan_track_views(int n_tracks, const long long* __restrict__ track_ptr,
                                                                 const int* __restrict__ track_image,
                                                                 const unsigned char* __restrict__ cam_reg,
                                                                 const unsigned char* __restrict__ trk_known,
                                                                 int* __restrict__ trk_reg_views, long long* __restrict__ tot) {
    const unsigned t = blockIdx.x * (unsigned)kPlanBlock + threadIdx.x;
    const bool active = t < (unsigned)n_tracks;
    const long long b = active ? track_ptr[t] : 0;
    const int n = active ? (int)(track_ptr[t + 1] - b) : 0;
    const int v = plan_count_views(active, b, n, track_image, cam_reg);
    const bool known = active && trk_known[t] != 0;
    if (active) trk_reg_views[t] = v;
    const int n_known = __popcll(__ballot(known)), n_ready = __popcll(__ballot(active && !known && v >= 2));
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* const u = reinterpret_cast<unsigned long long*>(tot);
        if (n_known) atomicAdd(u + kPlanTotKnown, (unsigned long long)n_known);
        if (n_ready) atomicAdd(u + kPlanTotReady, (unsigned long long)n_ready);
    }
}

// one workgroup per image: its features in a kept track, those whose track is known, and those whose track is not known
// and has a registered view besides this image
__global__ __launch_bounds__(kPlanBlock) void k_plan_image_views(const int* __restrict__ img_ptr, const int* __restrict__ feat_track,
                                                                 const unsigned char* __restrict__ cam_reg,
                                                                 const unsigned char* __restrict__ trk_known,
                                                                 const int* __restrict__ trk_reg_views, int* __restrict__ img_tracks,
                                                                 int* __restrict__ img_known, int* __restrict__ img_gain,
                                                                 long long* __restrict__ tot) {
    const unsigned i = blockIdx.x;
    const int reg = cam_reg[i] != 0;
    const unsigned end = (unsigned)img_ptr[i + 1];
    int in_track = 0, known = 0, gain = 0;
    for (unsigned f = (unsigned)img_ptr[i] + threadIdx.x; f < end; f += kPlanBlock) {
        const int t = feat_track[f];
        if (t < 0) continue;
        ++in_track;
        if (trk_known[t] != 0) ++known;
        else if (trk_reg_views[t] - reg >= 1) ++gain;
    }
    plan_block_sum3(in_track, known, gain);
    if (threadIdx.x == 0) {
        img_tracks[i] = in_track; img_known[i] = known; img_gain[i] = gain;
        if (reg) atomicAdd(reinterpret_cast<unsigned long long*>(tot) + kPlanTotReg, 1ull);
    }
}

// ---- sfmba_assemble_problem ------------------------------------------------------------------------------------------------
// one lane per track: its used observations when the track is used and has min_views of them, else 0
__global__ __launch_bounds__(kPlanBlock) void k_plan_used(int n_tracks, const long long* __restrict__ track_ptr,
                                                          const int* __restrict__ track_image, const unsigned char* __restrict__ cam_use,
                                                          const unsigned char* __restrict__ trk_use, int min_views,
                                                          int* __restrict__ kept) {
    const unsigned t = blockIdx.x * (unsigned)kPlanBlock + threadIdx.x;
    const bool in_range = t < (unsigned)n_tracks, active = in_range && trk_use[t] != 0;
    const long long b = active ? track_ptr[t] : 0;
    const int n = active ? (int)(track_ptr[t + 1] - b) : 0;
    const int v = plan_count_views(active, b, n, track_image, cam_use);
    if (in_range) kept[t] = v >= min_views ? v : 0;
}

// entry t of the scan over tracks: a track of the sub-problem and its used observations
struct PlanPointSrc {
    const int* kept; int n_tracks; int* pt_id; long long* obs_off; int* pt_of;
    __device__ unsigned n() const { return (unsigned)n_tracks; }
    __device__ int value(unsigned t) const { return kept[t]; }
    __device__ void put(unsigned t, int v, long long c_ex, long long s_ex) const {
        pt_id[t] = v ? (int)c_ex : -1;
        if (v) { obs_off[t] = s_ex; pt_of[c_ex] = (int)t; }
    }
    __device__ void finish() const {}
};

// one workgroup per image: it is in the sub-problem when it is used and one of its features lies in a track of it
__global__ __launch_bounds__(kPlanBlock) void k_plan_present(const int* __restrict__ img_ptr, const int* __restrict__ feat_track,
                                                             const unsigned char* __restrict__ cam_use, const int* __restrict__ kept,
                                                             int* __restrict__ present) {
    const unsigned i = blockIdx.x;
    const unsigned end = cam_use[i] != 0 ? (unsigned)img_ptr[i + 1] : 0u;     // (the same for the whole workgroup)
    int hit = 0, z0 = 0, z1 = 0;
    for (unsigned f = (unsigned)img_ptr[i] + threadIdx.x; f < end; f += kPlanBlock) {
        const int t = feat_track[f];
        if (t >= 0 && kept[t] > 0) ++hit;
    }
    plan_block_sum3(hit, z0, z1);
    if (threadIdx.x == 0) present[i] = hit > 0 ? 1 : 0;
}

// entry i of the scan over images: an image of the sub-problem
struct PlanCamSrc {
    const int* present; int n_images; int* cam_id; int* cam_of;
    __device__ unsigned n() const { return (unsigned)n_images; }
    __device__ int value(unsigned i) const { return present[i]; }
    __device__ void put(unsigned i, int v, long long c_ex, long long) const {
        cam_id[i] = v ? (int)c_ex : -1;
        if (v) cam_of[c_ex] = (int)i;
    }
    __device__ void finish() const {}
};

// one lane per track of the sub-problem: its used observations in the order of the CSR (a lane writes a track shorter
// than kPlanLong, the wave the longer ones afterwards: 64 observations a round, places by the ballot's prefix count)
__global__ __launch_bounds__(kPlanBlock) void k_plan_write(int n_tracks, const long long* __restrict__ track_ptr,
                                                           const int* __restrict__ track_feat, const int* __restrict__ track_image,
                                                           const unsigned char* __restrict__ cam_use, const int* __restrict__ kept,
                                                           const int* __restrict__ pt_id, const long long* __restrict__ obs_off,
                                                           const int* __restrict__ cam_id, long long* __restrict__ camera_indices,
                                                           long long* __restrict__ point_indices, int* __restrict__ obs_feat) {
    const unsigned t = blockIdx.x * (unsigned)kPlanBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = t < (unsigned)n_tracks && kept[t] > 0;
    const long long b = active ? track_ptr[t] : 0;
    const int n = active ? (int)(track_ptr[t + 1] - b) : 0;
    const int p = active ? pt_id[t] : 0;
    long long o = active ? obs_off[t] : 0;
    if (active && n < kPlanLong) {
        for (int k = 0; k < n; ++k) {
            const int img = track_image[b + k];
            if (cam_use[img] == 0) continue;
            camera_indices[o] = cam_id[img]; point_indices[o] = p; obs_feat[o] = track_feat[b + k];
            ++o;
        }
    }
    unsigned long long todo = __ballot(active && n >= kPlanLong);
    while (todo) {
        const int q = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long qb = __shfl(b, q);
        long long qo = __shfl(o, q);
        const int qn = __shfl(n, q), qp = __shfl(p, q);
        for (int base = 0; base < qn; base += 64) {
            const int k = base + lane;
            const int img = k < qn ? track_image[qb + k] : 0;
            const bool used = k < qn && cam_use[img] != 0;
            const unsigned long long m = __ballot(used);
            if (used) {
                const long long at = qo + __popcll(m & ((1ull << lane) - 1ull));
                camera_indices[at] = cam_id[img]; point_indices[at] = qp; obs_feat[at] = track_feat[qb + k];
            }
            qo += __popcll(m);
        }
    }
}

// ---- sfmba_get_assembled -----------------------------------------------------------------------------------------------------
// one lane per observation of the sub-problem: the pixel of its feature, copied
__global__ __launch_bounds__(kPlanBlock) void k_plan_gather(long long n_obs, const int* __restrict__ obs_feat,
                                                            const double2* __restrict__ keypoints, double2* __restrict__ points_2d) {
    const long long k = (long long)blockIdx.x * kPlanBlock + threadIdx.x;
    if (k < n_obs) points_2d[k] = keypoints[obs_feat[k]];
}
