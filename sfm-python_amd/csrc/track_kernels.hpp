// Feature tracks (sfmba_build_tracks): the connected components of the graph whose vertices are features and whose edges
// are the used match pairs, as a CSR of tracks in point-major order.  DESIGN.md section 23.
//
// Labels.  A union-find forest over the features in one int per feature.  parent[f] <= f always; a hook puts the LARGER
// root under the smaller, so the root of a finished component is its smallest feature id: a label that depends on the
// input alone, whatever the schedule did on the way.
//
// Concurrency.  k_track_union and k_track_flatten read and write `parent` while other workgroups do; every such access
// is a relaxed agent-scope atomic (the L2s of the XCDs are not coherent for plain loads within a launch).  A stale read
// is harmless: a value ever stored in parent[x] is an ancestor of x then and for ever after, and the compare-and-swap
// on a root is the only arbiter of a hook.  No kernel waits for another workgroup; the phases are separate launches.
//
// What atomics decide never shows: integer adds commute (component sizes, counters), and the slots k_track_fill hands
// out inside a component are sorted away by k_track_sort.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kTrackBlock = 256;                 // threads of every workgroup here
constexpr int kTrackScanPerThread = 4;
constexpr int kTrackScanItems = 1024;            // entries one workgroup scans
static_assert(kTrackScanItems == kTrackBlock * kTrackScanPerThread, "a thread scans kTrackScanPerThread consecutive entries");
constexpr int kTrackLong = 32;                   // a lane sorts a component shorter than this, the wave a longer one
// slots of the totals block (long long): written by the scans and k_track_sort, read by later launches and by the host
constexpr int kTrackTotComps = 0, kTrackTotMembers = 1, kTrackTotKept = 2, kTrackTotObs = 3;
constexpr int kTrackTotShort = 4, kTrackTotLong = 5, kTrackTotConflict = 6, kTrackTotSlots = 8;
constexpr int kTrackUnmatched = -1, kTrackShort = -2, kTrackConflict = -3;

#define TRACK_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// The root of x's tree at some moment of the call, with path halving.
// Terminates: parent[y] <= y for every y at every moment, with equality only at a root, and a stored value only ever
// decreases (hooks lower a root, fetch_min lowers the rest); a stale read returns an earlier, that is a larger, value
// that is still below y.  So x strictly decreases from one round to the next until it meets a root: at most x rounds.
__device__ __forceinline__ int track_find(int* __restrict__ parent, int x) {
    for (;;) {
        const int p = TRACK_LOAD(parent + x);
        if (p == x) return x;
        const int g = TRACK_LOAD(parent + p);
        if (g != p) (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

// image of feature f: the i with ptr[i] <= f < ptr[i + 1] (images without features are stepped over)
__device__ __forceinline__ int track_image_of(const int* __restrict__ ptr, int n_images, int f) {
    int lo = 0, hi = n_images;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one lane per feature
__global__ __launch_bounds__(kTrackBlock) void k_track_init(int N, const int* __restrict__ img_ptr, int n_images,
                                                            int* __restrict__ parent, int* __restrict__ size,
                                                            int* __restrict__ img, int* __restrict__ feat_track) {
    const unsigned f = blockIdx.x * (unsigned)kTrackBlock + threadIdx.x;
    if (f >= (unsigned)N) return;
    parent[f] = (int)f;
    size[f] = 0;
    img[f] = track_image_of(img_ptr, n_images, (int)f);
    feat_track[f] = kTrackUnmatched;
}

// one lane per used pair (a, b) of global feature ids
__global__ __launch_bounds__(kTrackBlock) void k_track_union(long long Mu, const int2* __restrict__ pairs, int* __restrict__ parent) {
    const long long k = (long long)blockIdx.x * kTrackBlock + threadIdx.x;
    if (k >= Mu) return;
    const int2 pr = pairs[k];
    int a = pr.x, b = pr.y;
    // Terminates: a round either ends the loop or replaces the root `a` by what the failed compare-and-swap found in
    // parent[a], which is below a (a parent only ever decreases); track_find never returns more than it was given.
    for (;;) {
        a = track_find(parent, a);
        b = track_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }           // a: the larger root, to hang under b
        int expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = expected;
    }
}

// one lane per feature: parent[f] = the root (the component's smallest id), and the sizes summed at the roots
__global__ __launch_bounds__(kTrackBlock) void k_track_flatten(int N, int* __restrict__ parent, int* __restrict__ size) {
    const unsigned f = blockIdx.x * (unsigned)kTrackBlock + threadIdx.x;
    if (f >= (unsigned)N) return;
    const int r = track_find(parent, (int)f);                  // (no hook runs in this launch: roots stay roots)
    __hip_atomic_store(parent + f, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(size + r, 1);
}

// ---- the exclusive scan of (count, sum) pairs in three launches: track_block_scan, k_track_scan_reduce and
// ---- k_track_scan_apply are in track_scan.hpp (the plan stage scans with them too), the middle launch is below
#include "track_scan.hpp"

// entry i of the first scan: a root of a component of two or more features, and its size
struct TrackCompSrc {
    const int* parent; int* size; int N; long long* comp_off; const long long* tot;
    __device__ unsigned n() const { return (unsigned)N; }
    __device__ int value(unsigned i) const { return parent[i] == (int)i && size[i] >= 2 ? size[i] : 0; }
    // a root learns its component's number; everything else -1
    __device__ void put(unsigned i, int v, long long c_ex, long long s_ex) const {
        size[i] = v ? (int)c_ex : -1;
        if (v) comp_off[c_ex] = s_ex;
    }
    __device__ void finish() const { comp_off[tot[kTrackTotComps]] = tot[kTrackTotMembers]; }
};
// entry c of the second scan: a kept component and its length
struct TrackKeepSrc {
    const int* kept_len; int* track_id; long long* track_off; const long long* tot;
    __device__ unsigned n() const { return (unsigned)tot[kTrackTotComps]; }
    __device__ int value(unsigned c) const { return kept_len[c]; }
    __device__ void put(unsigned c, int v, long long c_ex, long long s_ex) const {
        if (v) { track_id[c] = (int)c_ex; track_off[c] = s_ex; }
    }
    __device__ void finish() const {}
};

// one workgroup: sums[nb][2] to their exclusive prefixes in place, the totals to tot[slot], tot[slot + 1]
__global__ __launch_bounds__(kTrackBlock) void k_track_scan_sums(long long* __restrict__ sums, unsigned nb, long long* __restrict__ tot,
                                                                 int slot) {
    long long cc = 0, cs = 0;
    for (unsigned base = 0; base < nb; base += kTrackBlock) {
        const unsigned i = base + threadIdx.x;
        const long long c = i < nb ? sums[2 * (size_t)i] : 0, s = i < nb ? sums[2 * (size_t)i + 1] : 0;
        long long c_ex, s_ex, c_tot, s_tot;
        track_block_scan(c, s, c_ex, s_ex, c_tot, s_tot);
        if (i < nb) { sums[2 * (size_t)i] = cc + c_ex; sums[2 * (size_t)i + 1] = cs + s_ex; }
        cc += c_tot; cs += s_tot;
    }
    if (threadIdx.x == 0) { tot[slot] = cc; tot[slot + 1] = cs; }
}

// one lane per feature: a member of a component of two or more claims a place in its segment (any order: sorted next)
__global__ __launch_bounds__(kTrackBlock) void k_track_fill(int N, const int* __restrict__ parent, const int* __restrict__ comp_of_root,
                                                            const long long* __restrict__ comp_off, int* __restrict__ cursor,
                                                            int* __restrict__ members) {
    const unsigned f = blockIdx.x * (unsigned)kTrackBlock + threadIdx.x;
    if (f >= (unsigned)N) return;
    const int c = comp_of_root[parent[f]];
    if (c < 0) return;
    members[comp_off[c] + atomicAdd(cursor + c, 1)] = (int)f;
}

// m[0..n) ascending, by the wave: a bitonic network in which every exchange puts the smaller value at the lower place,
// so that the places from n up to the next power of two behave as +infinity without existing.  Every pair of a stage is
// one lane's, and a stage is fenced from the next (same wave, same CU: the wait for the stores is all it takes).
__device__ __forceinline__ void track_sort_wave(int* __restrict__ m, int n, int lane) {
    for (unsigned k = 2; k != 0 && (k >> 1) < (unsigned)n; k <<= 1) {          // (k = 2^31 is the last that exists)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            const bool flip = j == (k >> 1);
            for (unsigned i = lane; i < (unsigned)n; i += 64) {
                const unsigned l = flip ? i ^ (k - 1) : i ^ j;
                if (l > i && l < (unsigned)n) {
                    const int x = m[i], y = m[l];
                    if (y < x) { m[i] = y; m[l] = x; }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
}

// One lane per component: its members sorted by feature id (a lane takes a component shorter than kTrackLong, the wave
// the longer ones afterwards, one after the other), conflicts found as two neighbours of one image, and the verdict:
// 0 kept, kTrackShort for either length test, kTrackConflict (which wins over the length).  kept_len: the length of a
// kept component, else 0.
__global__ __launch_bounds__(kTrackBlock) void k_track_sort(const long long* __restrict__ comp_off, int* __restrict__ members,
                                                            const int* __restrict__ img, int min_length, int max_length,
                                                            int keep_conflicts, int* __restrict__ verdict,
                                                            int* __restrict__ kept_len, long long* __restrict__ tot) {
    const unsigned c = blockIdx.x * (unsigned)kTrackBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = c < (unsigned)tot[kTrackTotComps];
    const long long b = active ? comp_off[c] : 0;
    const int n = active ? (int)(comp_off[c + 1] - b) : 0;
    bool conflict = false;
    if (active && n < kTrackLong) {
        int* const m = members + b;
        for (int i = 1; i < n; ++i) {                           // insertion sort
            const int x = m[i];
            int j = i;
            for (; j > 0 && m[j - 1] > x; --j) m[j] = m[j - 1];
            m[j] = x;
        }
        int prev = img[m[0]];
        for (int i = 1; i < n; ++i) {
            const int cur = img[m[i]];
            conflict |= cur == prev;
            prev = cur;
        }
    }
    unsigned long long todo = __ballot(active && n >= kTrackLong);
    while (todo) {
        const int q = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long qb = __shfl(b, q);
        const int qn = __shfl(n, q);
        int* const m = members + qb;
        track_sort_wave(m, qn, lane);
        bool cf = false;
        for (int i = lane; i + 1 < qn; i += 64) cf |= img[m[i]] == img[m[i + 1]];
        cf = __any(cf);
        if (lane == q) conflict = cf;
    }
    if (!active) return;
    const bool is_short = n < min_length, is_long = max_length > 0 && n > max_length;
    const bool drop_conflict = conflict && !keep_conflicts;
    const int v = drop_conflict ? kTrackConflict : (is_short || is_long ? kTrackShort : 0);
    verdict[c] = v;
    kept_len[c] = v == 0 ? n : 0;
    unsigned long long* const t = reinterpret_cast<unsigned long long*>(tot);
    if (drop_conflict) atomicAdd(t + kTrackTotConflict, 1ull);
    else if (is_short) atomicAdd(t + kTrackTotShort, 1ull);
    else if (is_long) atomicAdd(t + kTrackTotLong, 1ull);
}

// one lane per member of a component, in the sorted order: the CSR of the kept tracks and every member's feat_track
__global__ __launch_bounds__(kTrackBlock) void k_track_write(const int* __restrict__ members, const int* __restrict__ parent,
                                                             const int* __restrict__ comp_of_root, const long long* __restrict__ comp_off,
                                                             const int* __restrict__ verdict, const int* __restrict__ track_id,
                                                             const long long* __restrict__ track_off, const int* __restrict__ img,
                                                             const long long* __restrict__ tot, int* __restrict__ feat_track,
                                                             long long* __restrict__ track_ptr, int* __restrict__ track_feat,
                                                             int* __restrict__ track_image) {
    const long long j = (long long)blockIdx.x * kTrackBlock + threadIdx.x;
    if (j == 0) track_ptr[tot[kTrackTotKept]] = tot[kTrackTotObs];
    if (j >= tot[kTrackTotMembers]) return;
    const int f = members[j];
    const int c = comp_of_root[parent[f]];
    const int v = verdict[c];
    if (v != 0) { feat_track[f] = v; return; }
    const int t = track_id[c];
    const long long first = comp_off[c], o = track_off[c] + (j - first);
    feat_track[f] = t;
    track_feat[o] = f;
    track_image[o] = img[f];
    if (j == first) track_ptr[t] = track_off[c];
}
