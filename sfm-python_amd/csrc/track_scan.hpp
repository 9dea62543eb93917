// The exclusive scan of (count, sum) pairs that the feature tracks and the plan stage share: the workgroup scan and the two
// launches that are templates over the source of the entries.  The text is what track_kernels.hpp held, moved unchanged.
// The middle launch, k_track_scan_sums, is no template: it stays in track_kernels.hpp, in the code object of tracks.hip,
// and a second source reaches it through launch_k_track_scan_sums (handle.hpp).  DESIGN.md sections 23 and 25.
//
// The includer defines kTrackBlock, kTrackScanPerThread and kTrackScanItems before this header: track_kernels.hpp holds
// the definitions (the tests read them there), plan_kernels.hpp restates them, and launch_k_track_scan_sums refuses a
// caller whose values differ from those the middle launch was compiled with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- exclusive scan of (count, sum) pairs in three launches: per-workgroup sums, their scan by one workgroup, the
// ---- downsweep.  No launch waits for another workgroup.
// exclusive prefix and total of (c, s) over the workgroup, in thread order
__device__ __forceinline__ void track_block_scan(long long c, long long s, long long& c_ex, long long& s_ex, long long& c_tot,
                                                 long long& s_tot) {
    __shared__ long long wc[kTrackBlock / 64], ws[kTrackBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long ci = c, si = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long tc = __shfl_up(ci, d), ts = __shfl_up(si, d);
        if (lane >= d) { ci += tc; si += ts; }
    }
    if (lane == 63) { wc[wave] = ci; ws[wave] = si; }
    __syncthreads();
    long long cb = 0, sb = 0;
    c_tot = 0; s_tot = 0;
#pragma unroll
    for (int w = 0; w < kTrackBlock / 64; ++w) {
        if (w < wave) { cb += wc[w]; sb += ws[w]; }
        c_tot += wc[w]; s_tot += ws[w];
    }
    c_ex = cb + ci - c; s_ex = sb + si - s;
    __syncthreads();                                            // (the arrays are free for the next call)
}

template <class Src>
__global__ __launch_bounds__(kTrackBlock) void k_track_scan_reduce(Src src, long long* __restrict__ sums) {
    const unsigned n = src.n(), i0 = blockIdx.x * (unsigned)kTrackScanItems + threadIdx.x * kTrackScanPerThread;
    long long c = 0, s = 0;
#pragma unroll
    for (int k = 0; k < kTrackScanPerThread; ++k) {
        const int v = i0 + k < n ? src.value(i0 + k) : 0;
        c += v ? 1 : 0; s += v;
    }
    long long c_ex, s_ex, c_tot, s_tot;
    track_block_scan(c, s, c_ex, s_ex, c_tot, s_tot);
    if (threadIdx.x == 0) { sums[2 * (size_t)blockIdx.x] = c_tot; sums[2 * (size_t)blockIdx.x + 1] = s_tot; }
}

template <class Src>
__global__ __launch_bounds__(kTrackBlock) void k_track_scan_apply(Src src, const long long* __restrict__ sums) {
    const unsigned n = src.n(), i0 = blockIdx.x * (unsigned)kTrackScanItems + threadIdx.x * kTrackScanPerThread;
    int v[kTrackScanPerThread];
    long long c = 0, s = 0;
#pragma unroll
    for (int k = 0; k < kTrackScanPerThread; ++k) {
        v[k] = i0 + k < n ? src.value(i0 + k) : 0;
        c += v[k] ? 1 : 0; s += v[k];
    }
    long long c_ex, s_ex, c_tot, s_tot;
    track_block_scan(c, s, c_ex, s_ex, c_tot, s_tot);
    c_ex += sums[2 * (size_t)blockIdx.x]; s_ex += sums[2 * (size_t)blockIdx.x + 1];
#pragma unroll
    for (int k = 0; k < kTrackScanPerThread; ++k) {
        if (i0 + k < n) src.put(i0 + k, v[k], c_ex, s_ex);
        c_ex += v[k] ? 1 : 0; s_ex += v[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) src.finish();
}
