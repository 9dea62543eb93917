// problem_tables.hpp -- the structure tables of a problem, built on the host: arrays in, tables out.
//
// sfmba_set_problem (sfmba.hip) converts the caller's observation arrays into staged arrays it owns (pinned memory),
// calls build_problem_tables() and uploads what comes out.  Nothing here knows of a device: the header compiles with a
// plain C++17 compiler, and tests/host/problem_tables_check.cpp runs the same code on std::vector staging under the host
// sanitizers (tests/test_host_tables.py).  The few constants the tables share with the kernels are defined here, once,
// and ba_kernels.hpp includes this header.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

#if defined(__HIPCC__)
#define SFMBA_HOST_DEVICE __host__ __device__
#else
#define SFMBA_HOST_DEVICE
#endif

namespace sfmba {

constexpr int kWaveChunkCams = 4, kWaveChunkRanges = 8;      // the XCD-aware chunk table (k_cam_schur_w, k_cam_blocks_w, k_cam_rhs_diag_w)
SFMBA_HOST_DEVICE constexpr int dense_block_index(int a, int b, int C) {      // a <= b, row-major upper triangle
    return a * C - a * (a - 1) / 2 + (b - a);
}

inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// A few persistent host threads for set_problem's passes over the observation arrays (spawning threads per
// call cost more than the passes themselves at a million observations).  run(parts, fn) calls fn(0..parts-1),
// part 0 on the calling thread, and returns when all are done.
class HostPool {
public:
    static constexpr int kMax = 16;
    ~HostPool() {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; ++gen_; }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    int parts_for(int64_t n) const {
        const int hw = (int)std::thread::hardware_concurrency();
        return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(kMax, hw > 0 ? hw : 1), n / 65536));
    }
    template <class Fn>
    void run(int parts, Fn fn) {
        if (parts <= 1) { fn(0); return; }
        while ((int)th_.size() < parts - 1) {
            const int id = (int)th_.size() + 1;
            th_.emplace_back([this, id] { worker(id); });
        }
        std::function<void(int)> f = fn;
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = &f; job_parts_ = parts; pending_ = parts - 1; ++gen_;
        }
        cv_.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
    }
private:
    void worker(int id) {
        unsigned long long seen = 0;
        for (;;) {
            std::function<void(int)>* f = nullptr;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                if (id >= job_parts_ || job_ == nullptr) continue;
                f = job_;
            }
            (*f)(id);
            {
                std::lock_guard<std::mutex> lk(m_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::function<void(int)>* job_ = nullptr;
    int job_parts_ = 0, pending_ = 0;
    unsigned long long gen_ = 0;
    bool stop_ = false;
};

// rows of the uploaded tables: the layouts of HIP's int2 / int4 (sfmba.hip asserts it), so that the upload stays a memcpy
struct alignas(8) TableRow2 { int x, y; };
struct alignas(16) TableRow4 { int x, y, z, w; };

struct ProblemFacts {                    // what only the build of the tables can tell
    bool pixels_int16 = true;            // every pixel coordinate is an int16 integer
    bool cam_multi = false;              // some camera's list was cut into several chunks
    int64_t pair_entries = 0;            // length of the pair lists of the dense path
};

// What the build reads of the forms as planned (decide_problem_forms with the facts assumed favourable) and of the device;
// packed_upload is the caller's to act on: it stages ci16 / uv16 when the packed upload is planned
struct TablePlan {
    bool dense = false, xcd_b = false, cm_device = false, packed_upload = false;
    int64_t cam_chunk_len = 4096;
    int64_t total_waves = 0;             // waves of a point-major sweep over the whole device
    int parts = 1;                       // threads of the passes over the observations (HostPool::parts_for(N))
    int pair_parts = 1;                  // threads of the pair lists (P >= 32768 ? 4 : 1)
};

// The caller's arguments, the cameras held still, and how much of the staged arrays the previous call left valid
struct ProblemInput {
    int64_t C = 0, P = 0, N = 0;
    const int64_t *cam = nullptr, *pt = nullptr;
    const double* uv = nullptr;          // pixels as doubles, or
    const int64_t* uv_i64 = nullptr;     // ... as integers
    const char* fixed = nullptr;         // [C] camera held still
    int64_t n_cmp = 0;                   // leading observations to compare with the staged arrays of the previous problem
    bool packed_prefix_ok = false;       // ... and their packed entries are valid too
};

// The converted arrays, owned by the caller (pinned memory in the library): [ld] observations, ld = N rounded up to 256
struct StagedArrays {
    int *ci = nullptr, *pi = nullptr;    // [ld] camera / point index in stored (point-major) order
    double* uvs = nullptr;               // [ld][2] pixels
    float* uvf = nullptr;                // ... in fp32 storage (null: fp64)
    unsigned short* ci16 = nullptr;      // [ld] packed upload (null: not planned)
    short* uv16 = nullptr;               // [ld][2]
    int* perm = nullptr;                 // [ld] camera-major permutation (written unless the device sorts)
    int* ptr = nullptr;                  // [P + 1] run offsets of the points
};

// Everything build_problem_tables() returns.  The vectors keep their capacity from call to call.
struct ProblemTables {
    std::vector<int> cam_ptr;                            // [C + 1]
    std::vector<TableRow2> ranges, wsteps, steps;
    std::vector<TableRow4> chunks, chunks_b;
    std::vector<int> chunk_ptr, chunk_ptr_b;
    std::vector<int> cov_ptr, cov_pt;                    // dense path: per block pair (a <= b) the points both cameras see
    std::vector<TableRow2> blk_ab;
    std::vector<int64_t> order;                          // sorted position -> caller's observation index (empty: identity)
    bool sorted = true;
    int64_t fdiff = 0;                                   // leading observations equal to the previous problem's
    ProblemFacts facts;
    int64_t bad = -1;                                    // first observation with an index out of range (then nothing else is valid)
    double t_convert = 0, t_sort = 0, t_ranges = 0, t_steps = 0, t_end = 0;     // now_s() at the end of the phases
    // per part of the conversion pass: [parts][C] camera counts, then scatter offsets; first bad index, first changed
    // observation, order broken, a pixel that is no int16
    std::vector<int> hist;
    std::vector<int64_t> bad_part, first_diff;
    std::vector<char> unsorted, not16;
};

// The phases of the build, in order; run() is build_problem_tables().
struct TableBuild {
    const ProblemInput& in;
    const TablePlan& plan;
    const StagedArrays& st;
    HostPool& pool;
    ProblemTables& tb;
    const int64_t C = in.C, P = in.P, N = in.N;
    const int64_t *const cam = in.cam, *const pt = in.pt;
    const double* const uv = in.uv;
    const int64_t* const uv_i64 = in.uv_i64;
    const char* const fixed = in.fixed;
    const int64_t ld = (N + 255) / 256 * 256;
    const size_t ldz = (size_t)ld;
    const int parts = plan.parts;
    const int64_t per = (N + parts - 1) / parts;
    double* const uvs = st.uvs; float* const uvf = st.uvf;
    int *const ci = st.ci, *const pi = st.pi, *const perm = st.perm, *const ptr = st.ptr;
    unsigned short* const ci16 = st.ci16; short* const uv16 = st.uv16;

    bool run();
    void convert(const int64_t* ord, int64_t n_compare);
    bool convert_and_compare();     // ... and the point-major order
    void camera_major_sort();
    void wave_ranges(), step_tables(), chunk_tables(), pair_lists();
};

// pass 1 (parallel): range check, order check, conversion with comparison, camera histogram
inline void TableBuild::convert(const int64_t* ord, int64_t n_compare) {
    const bool packed_prefix_ok = in.packed_prefix_ok;
    std::vector<int>& hist = tb.hist;
    pool.run(parts, [&](int t) {
        const int64_t b = std::min<int64_t>(N, t * per), e = std::min<int64_t>(N, (t + 1) * per);
        int* hc = hist.data() + (size_t)t * (size_t)C;
        for (int64_t c = 0; c < C; ++c) hc[c] = 0;
        int64_t fd = N;
        for (int64_t k = b; k < e; ++k) {
            const int64_t s = ord ? ord[k] : k;
            const int64_t cv = cam[s], pv = pt[s];
            if (cv < 0 || cv >= C || pv < 0 || pv >= P) { if (tb.bad_part[t] < 0) tb.bad_part[t] = s; continue; }
            if (!ord && k > 0 && pv < pt[k - 1]) tb.unsorted[t] = 1;
            double u0, u1;
            if (uv) { u0 = uv[2 * s]; u1 = uv[2 * s + 1]; }
            else { u0 = (double)uv_i64[2 * s]; u1 = (double)uv_i64[2 * s + 1]; }          // as numpy promotes
            if (!fixed[(size_t)cv]) ++hc[cv];
            const bool same = k < n_compare && ci[k] == (int)cv && pi[k] == (int)pv && uvs[2 * k] == u0 && uvs[2 * k + 1] == u1;
            if (ci16 && !(same && packed_prefix_ok)) {     // (an unchanged entry is packed already, if the previous call packed)
                const bool in16 = std::fabs(u0) < 32768.0 && std::fabs(u1) < 32768.0;
                const short q0 = in16 ? (short)u0 : (short)0, q1 = in16 ? (short)u1 : (short)0;
                if (!in16 || (double)q0 != u0 || (double)q1 != u1) tb.not16[t] = 1;
                ci16[k] = (unsigned short)cv; uv16[2 * k] = q0; uv16[2 * k + 1] = q1;
            }
            if (same) continue;
            if (fd == N) fd = k;
            ci[k] = (int)cv; pi[k] = (int)pv; uvs[2 * k] = u0; uvs[2 * k + 1] = u1;
            if (uvf) { uvf[2 * k] = (float)u0; uvf[2 * k + 1] = (float)u1; }    // integer pixels up to 2^24 are exact
        }
        tb.first_diff[t] = fd;
    });
}

// ---- incremental re-use ---------------------------------------------------------
// The reference calls BA once per fused edge on a growing reconstruction (sfm_lite/sfm.py:59-71 of the reference):
// once every camera is registered, a new edge only appends points and their observations, so the argument
// arrays of one call start with those of the previous call.  The converted arrays of the last problem stay in
// pinned host memory and in HBM; this call compares as it converts, finds the first observation that differs
// and uploads from there on only.  The structure tables are always rebuilt from the (complete) host arrays, by
// the same code whatever was re-used: results are bitwise those of a fresh handle.
// Then the point-major order: any order is accepted, the kernels want point-major.
// False: an index is out of range (tb.bad).
inline bool TableBuild::convert_and_compare() {
    const int64_t n_cmp = in.n_cmp;
    tb.hist.assign((size_t)parts * (size_t)C, 0);
    tb.bad_part.assign((size_t)parts, -1);
    tb.first_diff.assign((size_t)parts, N);
    tb.unsorted.assign((size_t)parts, 0);
    tb.not16.assign((size_t)parts, 0);
    tb.bad = -1;
    convert(nullptr, n_cmp);
    for (int t = 0; t < parts; ++t) {       // (numpy's fancy indexing would raise IndexError in the reference)
        if (tb.bad_part[t] < 0) continue;
        tb.bad = tb.bad_part[t];
        return false;
    }
    tb.sorted = true;
    for (int t = 0; t < parts; ++t) tb.sorted = tb.sorted && !tb.unsorted[t];
    tb.order.clear();
    if (!tb.sorted) {                    // No re-use on this path.
        tb.order.resize(N);
        std::iota(tb.order.begin(), tb.order.end(), (int64_t)0);
        std::stable_sort(tb.order.begin(), tb.order.end(), [&](int64_t a, int64_t b) { return pt[a] < pt[b]; });
        convert(tb.order.data(), 0);
    }
    tb.fdiff = N;
    for (int t = 0; t < parts; ++t) tb.fdiff = std::min(tb.fdiff, tb.first_diff[t]);
    tb.fdiff = std::min(tb.fdiff, n_cmp);      // nothing beyond the compared prefix is on the device
    for (size_t k = (size_t)N; k < ldz; ++k) {                       // padding up to the next multiple of 256
        ci[k] = 0; pi[k] = 0; uvs[2 * k] = 0.0; uvs[2 * k + 1] = 0.0;
        if (uvf) { uvf[2 * k] = 0.f; uvf[2 * k + 1] = 0.f; }
        if (ci16) { ci16[k] = 0; uv16[2 * k] = 0; uv16[2 * k + 1] = 0; }
    }
    tb.facts = ProblemFacts{};
    for (char f : tb.not16) tb.facts.pixels_int16 = tb.facts.pixels_int16 && !f;
    return true;
}

// camera-major order: stable counting sort of the positions by camera (per-part histograms, so that the parts scatter
// independently and the order inside a camera stays the point-major one), and the run offsets of the points
inline void TableBuild::camera_major_sort() {
    std::vector<int>& hist = tb.hist;
    std::vector<int>& cam_ptr = tb.cam_ptr;
    cam_ptr.resize((size_t)C + 1);
    int run = 0;
    for (int64_t c = 0; c < C; ++c) {
        cam_ptr[c] = run;
        for (int t = 0; t < parts; ++t) { int& v = hist[(size_t)t * (size_t)C + c]; const int n = v; v = run; run += n; }
    }
    cam_ptr[C] = run;
    // pass 2 (parallel): ptr[p] = first position whose point index is >= p (pi is non-decreasing): every run start k
    // writes the entries (pi[k-1], pi[k]], so the parts touch disjoint pieces of ptr.
    // The camera-major order itself is sorted on the DEVICE (k_cam_hist / k_cam_offsets / k_cam_scatter: the same stable
    // order) unless the camera counters do not fit the LDS; the host then only needs the run offsets.
    const bool on_host = !plan.cm_device;
    pool.run(parts, [&](int t) {
        const int64_t b = std::min<int64_t>(N, t * per), e = std::min<int64_t>(N, (t + 1) * per);
        int* off = hist.data() + (size_t)t * (size_t)C;
        for (int64_t k = b; k < e; ++k) {
            const int lo = k == 0 ? -1 : pi[k - 1];
            for (int q = lo + 1; q <= pi[k]; ++q) ptr[q] = (int)k;
            if (on_host && !fixed[(size_t)ci[k]]) perm[off[ci[k]]++] = (int)k;
        }
    });
    for (int64_t q = (int64_t)pi[N - 1] + 1; q <= P; ++q) ptr[q] = (int)N;
    if (on_host)
        for (size_t k = (size_t)cam_ptr[C]; k < ldz; ++k) perm[k] = 0;  // (shorter than N when cameras are held still)
}

// wave ranges: cut at point boundaries, >= T observations each
inline void TableBuild::wave_ranges() {
    const int64_t total_waves = plan.total_waves;
    const int64_t T = std::max<int64_t>(64, (N + total_waves - 1) / total_waves);
    std::vector<TableRow2>& ranges = tb.ranges;
    ranges.clear();
    int64_t start = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t endp = ptr[p + 1];
        if (endp - start >= T || (p == P - 1 && endp > start)) {
            ranges.push_back(TableRow2{(int)start, (int)endp});
            start = endp;
        }
    }
}

// step table of the sweeps: per wave range, batches of <= 64 observations that end on a point
// boundary; a point with more than 64 observations is one step of its own
inline void TableBuild::step_tables() {
    const std::vector<TableRow2>& ranges = tb.ranges;
    std::vector<TableRow2>& wsteps = tb.wsteps;
    std::vector<TableRow2>& steps = tb.steps;
    wsteps.resize(ranges.size());
    steps.clear();
    // the ranges are independent: every worker walks a slice of them into its own list (the walk is a chain of
    // dependent reads of pi / ptr -- 1.2-1.4 ms of a 3.6 ms call at 1M observations when one thread did all of it),
    // the lists are concatenated in range order afterwards
    const int sparts = (int)std::max<size_t>(1, std::min<size_t>((size_t)parts, ranges.size() / 64));
    std::vector<std::vector<TableRow2>> local((size_t)sparts);
    const size_t rper = (ranges.size() + (size_t)sparts - 1) / (size_t)sparts;
    pool.run(sparts, [&](int t) {
        std::vector<TableRow2>& out = local[(size_t)t];
        const size_t w0 = std::min(ranges.size(), (size_t)t * rper), w1 = std::min(ranges.size(), w0 + rper);
        out.reserve((w1 - w0) * 6);
        for (size_t w = w0; w < w1; ++w) {
            const int first = (int)out.size();                       // (relative to the slice; rebased below)
            int64_t pos = ranges[w].x;
            const int64_t end = ranges[w].y;
            while (pos < end) {
                const int64_t pfirst = pi[pos];
                if (ptr[pfirst + 1] - pos > 64) {                    // long run (pos is always a run start)
                    out.push_back(TableRow2{(int)pos, (int)(ptr[pfirst + 1] - pos)});
                    pos = ptr[pfirst + 1];
                    continue;
                }
                // largest run boundary <= pos + 64
                int64_t lim = std::min<int64_t>(pos + 64, end), cut;
                if (lim == end) cut = end;
                else { const int64_t pl = pi[lim]; cut = (ptr[pl] == lim) ? lim : ptr[pl]; }   // lim inside a run -> its start
                out.push_back(TableRow2{(int)pos, (int)(cut - pos)});
                pos = cut;
            }
            wsteps[w] = TableRow2{first, (int)out.size() - first};
        }
    });
    size_t total = 0;
    for (auto& v : local) total += v.size();
    steps.reserve(total);
    for (int t = 0; t < sparts; ++t) {
        const int base = (int)steps.size();
        const size_t w0 = std::min(ranges.size(), (size_t)t * rper), w1 = std::min(ranges.size(), w0 + rper);
        for (size_t w = w0; w < w1; ++w) wsteps[w].x += base;
        steps.insert(steps.end(), local[(size_t)t].begin(), local[(size_t)t].end());
    }
}

// chunk table of the camera-major kernels: every camera gets at least one chunk (an empty one writes its
// zeros), runs longer than the chunk length are cut; one 256-thread workgroup per chunk
inline void TableBuild::chunk_tables() {
    const std::vector<int>& cam_ptr = tb.cam_ptr;
    std::vector<TableRow4>& chunks = tb.chunks;
    std::vector<int>& chunk_ptr = tb.chunk_ptr;
    chunks.clear();
    chunk_ptr.resize((size_t)C + 1);
    const int64_t chunk_len = plan.cam_chunk_len;
    for (int64_t c = 0; c < C; ++c) {
        chunk_ptr[c] = (int)chunks.size();
        const int b = cam_ptr[c], e = cam_ptr[c + 1];
        const int nch = std::max<int>(1, (int)((e - b + chunk_len - 1) / chunk_len));
        if (nch > 1) tb.facts.cam_multi = true;
        for (int j = 0; j < nch; ++j)
            chunks.push_back(TableRow4{(int)c, (int)std::min<int64_t>(e, b + j * chunk_len),
                                       (int)std::min<int64_t>(e, b + (j + 1) * chunk_len), nch});
    }
    chunk_ptr[C] = (int)chunks.size();
    // XCD-aware chunks for pass B of the Schur product (many points).  Every camera-major pass gathers one record
    // per observation from a table of P x 48 bytes; workgroup i runs on XCD i mod 8 and each XCD has its own 4 MiB
    // L2: with one chunk per camera every L2 sees the WHOLE table (48 MB at a million points).  A camera's list is
    // ascending in the point index, so it is cut at the eight point-range boundaries P k / 8: chunk 8 c + k runs on
    // XCD k and touches points of range k only, each L2 serves an eighth of the table (pass B at 5000 / 1M / 10M:
    // 201 -> 134 us); the eight partial rows of a camera are added by k_cam_combine and the PCG tail runs behind
    // it (k_pcg_tail).  Pass B only: the passes with 27 sums per workgroup (K3, rhs + preconditioner) lose more to
    // eight times as many block reductions than they gain (208 -> 320 us, 188 -> 257 us).
    std::vector<TableRow4>& chunks_b = tb.chunks_b;
    chunks_b.clear();
    tb.chunk_ptr_b.clear();
    if (plan.xcd_b) {
        // row (8 g + k) 4 + j = camera 4 g + j, range k: the four waves of workgroup 8 g + k (XCD k) take the pieces of
        // four cameras over the same point range (k_cam_schur_w); cameras behind the last one are padding (camera -1)
        constexpr int kX = kWaveChunkRanges, kG = kWaveChunkCams;
        static_assert(kX == 8, "one range per XCD");
        const int64_t groups = (C + kG - 1) / kG;
        chunks_b.assign((size_t)(groups * kX * kG), TableRow4{-1, 0, 0, kX});
        for (int64_t c = 0; c < C && !plan.cm_device; ++c) {       // (device-side sort: k_xcd_chunks fills the table)
            const int b = cam_ptr[c], e = cam_ptr[c + 1];
            int prev = b;
            for (int k = 0; k < kX; ++k) {
                int bound = e;
                if (k + 1 < kX) {
                    const int64_t p_hi = P * (int64_t)(k + 1) / kX;          // first point of the next range
                    int lo = prev, hi = e;                                   // lower bound over pi[perm[.]] (ascending)
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (pi[perm[mid]] < p_hi) lo = mid + 1; else hi = mid; }
                    bound = lo;
                }
                chunks_b[(size_t)(((c / kG) * kX + k) * kG + c % kG)] = TableRow4{(int)c, prev, bound, kX};
                prev = bound;
            }
        }
    }
}

// few cameras: for every block pair (a <= b) the points seen by both cameras, with multiplicity (a point seen
// m_a, m_b times contributes m_a m_b times); two counting passes over the runs.  The diagonal pairs' workgroups
// also sum the reduced right-hand side of their camera, over the entries that pair an observation with itself.
inline void TableBuild::pair_lists() {
    std::vector<int>&cov_ptr = tb.cov_ptr, &cov_pt = tb.cov_pt;
    std::vector<TableRow2>& blk_ab = tb.blk_ab;
    cov_ptr.clear(); cov_pt.clear(); blk_ab.clear();
    if (!plan.dense) return;
    const int nblk = (int)(C * (C + 1) / 2);
    cov_ptr.assign((size_t)nblk + 1, 0);
    // (unordered pairs i <= j: a pair of different cameras is one entry of its block, two observations of the same
    // camera by the same point are two, an observation with itself one -- what the ordered double loop counted)
    // Two passes over the points, count and fill; from 32k points on split over a few threads by contiguous point
    // ranges: per-part counts per block, then part t's entries of a block follow part t - 1's -- ascending point order
    // inside a block, whatever the number of parts.  (Below that size waking the pool costs more than the passes:
    // measured at the SceauxCastle scale, 0.10 ms single-threaded against 0.13 ms on four threads.)
    const int pp = plan.pair_parts;
    std::vector<int> cnt((size_t)pp * (size_t)nblk, 0);
    const int64_t pper = (P + pp - 1) / pp;
    auto each_pair = [&](int t, auto&& visit) {
        const int64_t p0 = std::min<int64_t>(P, t * pper), p1 = std::min<int64_t>(P, p0 + pper);
        for (int64_t p = p0; p < p1; ++p)
            for (int i = ptr[p]; i < ptr[p + 1]; ++i)
                for (int j = i; j < ptr[p + 1]; ++j) {
                    const int a = std::min(ci[i], ci[j]), b = std::max(ci[i], ci[j]);
                    if (fixed[(size_t)a] || fixed[(size_t)b]) continue;
                    visit((int)p, dense_block_index(a, b, (int)C), i == j, a == b);
                }
    };
    pool.run(pp, [&](int t) {
        int* ct = cnt.data() + (size_t)t * (size_t)nblk;
        each_pair(t, [&](int, int blk, bool self, bool same_cam) { ct[blk] += (self || !same_cam) ? 1 : 2; });
    });
    int64_t total = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        cov_ptr[(size_t)blk] = (int)std::min<int64_t>(total, INT32_MAX);
        for (int t = 0; t < pp; ++t) { int& v = cnt[(size_t)t * (size_t)nblk + blk]; const int n_e = v; v = (int)std::min<int64_t>(total, INT32_MAX); total += n_e; }
    }
    cov_ptr[(size_t)nblk] = (int)std::min<int64_t>(total, INT32_MAX);
    tb.facts.pair_entries = total;
    if (total > ((int64_t)1 << 26)) return;                  // very long tracks: the pair lists would not pay (-> PCG)
    cov_pt.resize((size_t)std::max<int64_t>(1, total));
    pool.run(pp, [&](int t) {
        int* fill = cnt.data() + (size_t)t * (size_t)nblk;
        each_pair(t, [&](int p, int blk, bool self, bool same_cam) {
            int& f = fill[blk];
            cov_pt[(size_t)f++] = self ? ~p : p;                       // (~p: the term of the right-hand side)
            if (!self && same_cam) cov_pt[(size_t)f++] = p;
        });
    });
    blk_ab.resize((size_t)nblk);
    for (int a = 0; a < (int)C; ++a)
        for (int b = a; b < (int)C; ++b) blk_ab[(size_t)dense_block_index(a, b, (int)C)] = TableRow2{a, b};
}

inline bool TableBuild::run() {
    if (!convert_and_compare()) return false;
    tb.t_convert = now_s();
    camera_major_sort();
    tb.t_sort = now_s();
    wave_ranges();
    tb.t_ranges = now_s();
    step_tables();
    tb.t_steps = now_s();
    chunk_tables();
    pair_lists();
    tb.t_end = now_s();
    return true;
}

// Converts the caller's arrays into `st` and builds every table into `tb`.  False: an index is out of range, tb.bad is
// the first such observation and nothing else of tb is valid.
inline bool build_problem_tables(const ProblemInput& in, const TablePlan& plan, const StagedArrays& st, HostPool& pool,
                                 ProblemTables& tb) {
    return TableBuild{in, plan, st, pool, tb}.run();
}

}  // namespace sfmba
