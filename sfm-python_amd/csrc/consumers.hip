// consumers.hip -- host code of the consumers of a solved scene (kernels: consumer_kernels.hpp): reprojection statistics,
// triangulation, robust triangulation, resection, robust resection and two-view geometry.  None touches a buffer of the solver's.
#include "handle.hpp"
#include "consumer_kernels.hpp"

namespace {
// ---- reprojection statistics (sfmba_reprojection_stats; kernels: consumer_kernels.hpp, "Reprojection statistics") ------
int stats_allocate(sfmba_handle* h, int* pt_blocks) {
    auto& s = h->stats;
    const size_t ldz = (size_t)h->ld, P = (size_t)h->P, C = (size_t)h->C;
    *pt_blocks = (int)std::max<size_t>(1, (P + kStatsPtThreads - 1) / kStatsPtThreads);
    return ensure_all(h, {
        {&s.x, sizeof(double) * (size_t)h->n}, {&s.tab, sizeof(double) * cam_table_doubles((int)C)},
        {&s.ed, sizeof(double) * 2 * ldz}, {&s.keep, ldz}, {&s.keep_final, ldz},
        {&s.pt_views, sizeof(int) * P}, {&s.pt_d, sizeof(double) * 4 * P}, {&s.pt_keep, P},
        {&s.cam_i, sizeof(int) * 2 * C}, {&s.cam_d, sizeof(double) * 2 * C},
        {&s.part, sizeof(double) * kStatsPart * (size_t)*pt_blocks}, {&s.sum, sizeof(double) * kStatsPart}});
}

// x into the call's own buffer, and its camera table
int stats_prepare(sfmba_handle* h, const double* x) {
    auto& s = h->stats;
    CHK(upload_x(h, x, s.x.as<double>()));
    return launch_k_cam_table(h, s.x.as<double>(), s.tab.as<double>());
}

// the per-observation sweep: grid, workgroup and LDS of the residual-only sweep (launch_resjac)
int launch_obs_stats(sfmba_handle* h, const StatsFilter& flt) {
    auto& s = h->stats;
    const bool lds_tab = h->forms.lds_tab;
    const int grid = grid_1d(h->N, kSweepThreads, h->n_cu);
    const size_t lds = lds_tab ? (size_t)h->C * kCamRow * sizeof(double) : sizeof(double) * kRowSlabDoubles * kWavesPerSweepBlock;
    auto kern = lds_tab ? (h->f32 ? k_obs_stats<true, true> : k_obs_stats<true, false>)
                        : (h->f32 ? k_obs_stats<false, true> : k_obs_stats<false, false>);
    CHK(set_lds(h, kern, lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kSweepThreads), lds, h->stream, (const double*)s.tab.as<double>(),
                       (const double*)(s.x.as<double>() + 6 * h->C), (const int*)h->cam_idx.as<int>(),
                       (const int*)h->pt_idx.as<int>(), (const double*)h->uv.as<double>(), s.ed.as<double>(),
                       s.keep.as<unsigned char>(), (int)h->N, (int)h->C, h->K, flt.max_err, flt.min_depth);
    LAUNCHED(h);
    return 0;
}

int launch_point_stats(sfmba_handle* h, const StatsFilter& flt, int pt_blocks) {
    auto& s = h->stats;
    double* d = s.pt_d.as<double>();
    const size_t P = (size_t)h->P;
    const PointStatsOut out{s.pt_views.as<int>(), d, d + P, d + 2 * P, d + 3 * P, s.pt_keep.as<unsigned char>()};
    hipLaunchKernelGGL(k_point_stats, dim3(pt_blocks), dim3(kStatsPtThreads), 0, h->stream, (const int*)h->pt_ptr.as<int>(),
                       (const int*)h->cam_idx.as<int>(), (const double*)s.tab.as<double>(),
                       (const double*)(s.x.as<double>() + 6 * h->C), (const double*)s.ed.as<double>(),
                       (const unsigned char*)s.keep.as<unsigned char>(), (int)h->P, flt, out,
                       s.keep_final.as<unsigned char>(), s.part.as<double>());
    LAUNCHED(h);
    return 0;
}

int launch_stats_summary(sfmba_handle* h, int pt_blocks) {
    auto& s = h->stats;
    hipLaunchKernelGGL(k_stats_summary, dim3(1), dim3(256), 0, h->stream, (const double*)s.part.as<double>(), pt_blocks,
                       s.sum.as<double>());
    LAUNCHED(h);
    return 0;
}

// The camera-major permutation of all observations of the current problem: built at the first call that asks for
// per-camera figures and kept until the problem's arrays change (the solver's own lists leave out cameras held still
// and, sorted on the device, come without the permutation).
}  // namespace
int sfmba::stats_cam_perm(sfmba_handle* h) {
    auto& s = h->stats;
    const int64_t N = h->N, C = h->C;
    if (s.perm_gen != 0 && s.perm_gen == h->problem_gen && s.perm_N == N && s.perm_C == C) return 0;
    const size_t lds = sizeof(int) * (size_t)C;
    if (lds > kLdsDynMax)
        return fail(h, -1, "per-camera statistics sort with one LDS counter per camera: at most %d cameras", (int)(kLdsDynMax / sizeof(int)));
    const int B = (int)std::min<int64_t>(kSortSlices, (N + 63) / 64);
    const int per_slice = (int)(((N + B - 1) / B + 63) / 64 * 64);
    int key_bits = 0;
    while (((int64_t)1 << key_bits) < C) ++key_bits;
    CHK(ensure_all(h, {{&s.hist, sizeof(int) * 2 * (size_t)B * (size_t)C},               // counts | offsets
                       {&s.cnt, sizeof(int) * (size_t)C}, {&s.cam_ptr, sizeof(int) * ((size_t)C + 1)},
                       {&s.perm, sizeof(int) * (size_t)h->ld}}));
    int* off = s.hist.as<int>() + (size_t)B * (size_t)C;
    const unsigned cblocks = (unsigned)((C + 255) / 256);
    CHK(set_lds(h, k_stats_cam_scatter, lds));
    CHK(launch_k_cam_hist(h, nullptr, B, per_slice, s.hist.as<int>()));
    hipLaunchKernelGGL(k_stats_cam_count, dim3(cblocks), dim3(256), 0, h->stream, (const int*)s.hist.as<int>(), B, (int)C,
                       s.cnt.as<int>());
    LAUNCHED(h);
    hipLaunchKernelGGL(k_stats_cam_scan, dim3(1), dim3(1024), 0, h->stream, (const int*)s.cnt.as<int>(), (int)C, s.cam_ptr.as<int>());
    LAUNCHED(h);
    CHK(launch_k_cam_offsets(h, s.hist.as<int>(), s.cam_ptr.as<int>(), B, off));
    hipLaunchKernelGGL(k_stats_cam_scatter, dim3(B), dim3(64), lds, h->stream, (const int*)h->cam_idx.as<int>(), (int)N, (int)C,
                       per_slice, key_bits, (const int*)off, s.perm.as<int>());
    LAUNCHED(h);
    s.perm_gen = h->problem_gen; s.perm_N = N; s.perm_C = C;
    return 0;
}
namespace {

int launch_cam_stats(sfmba_handle* h) {
    auto& s = h->stats;
    const size_t C = (size_t)h->C;
    hipLaunchKernelGGL(k_cam_stats, dim3((unsigned)C), dim3(kCamThreads), 0, h->stream, (const int*)s.cam_ptr.as<int>(),
                       (const int*)s.perm.as<int>(), (const double*)s.ed.as<double>(),
                       (const unsigned char*)s.keep_final.as<unsigned char>(), s.cam_i.as<int>(), s.cam_d.as<double>(),
                       s.cam_d.as<double>() + C, s.cam_i.as<int>() + C);
    LAUNCHED(h);
    return 0;
}

StatsFilter stats_filter(const sfmba_filter_options& o) {
    return StatsFilter{o.max_error_px, o.min_depth, o.min_angle_deg, (int)o.min_views};
}

// ---- what triangulation and resection share on the host ------------------------------------------------------------------
// The masks of a call onto the device, both through pinned staging (stats.mask_host): obs_use [N] into stored order
// (h->tb.order: stored position -> caller's) -> stats.use, the select mask [n_sel] as it is -> select_dev; null: not
// given.  *counts: room for n_counts ints behind them in the staging, for finish_with_ok_count.
int stage_masks(sfmba_handle* h, const uint8_t* obs_use, const uint8_t* select, size_t n_sel, DevBuf& select_dev,
                size_t n_counts, int** counts) {
    auto& s = h->stats;
    const size_t N = (size_t)h->N;
    const size_t off_sel = (N + 63) / 64 * 64, off_ok = off_sel + (n_sel + 63) / 64 * 64;
    HIPCHK(h, s.mask_host.ensure(off_ok + sizeof(int) * n_counts, 0));
    unsigned char* const st = s.mask_host.as<unsigned char>();
    if (obs_use && N) {
        for (size_t k = 0; k < N; ++k) st[k] = obs_use[caller_position(h, k)] ? 1 : 0;
        HIPCHK(h, hipMemcpyAsync(s.use.p, st, N, hipMemcpyHostToDevice, h->stream));
    }
    if (select && n_sel) {
        for (size_t k = 0; k < n_sel; ++k) st[off_sel + k] = select[k] ? 1 : 0;
        HIPCHK(h, hipMemcpyAsync(select_dev.p, st + off_sel, n_sel, hipMemcpyHostToDevice, h->stream));
    }
    *counts = reinterpret_cast<int*>(st + off_ok);
    return 0;
}

// the end of such a call: the n OK counts at src (device) through `counts` (stage_masks), the stream waited for, their
// sum -> *n_ok (null: not asked for)
int finish_with_ok_count(sfmba_handle* h, const int* src, size_t n, int* counts, int64_t* n_ok) {
    if (n_ok) HIPCHK(h, download(h, counts, src, sizeof(int) * n));
    CHK(wait_stream(h));
    if (n_ok) {
        *n_ok = 0;
        for (size_t k = 0; k < n; ++k) *n_ok += counts[k];
    }
    return 0;
}

// ---- triangulation (sfmba_triangulate; kernel: consumer_kernels.hpp, "Triangulation") ------------------------------------
int tri_allocate(sfmba_handle* h, int* grid) {
    auto& s = h->stats;
    auto& t = h->tri;
    const size_t ldz = (size_t)h->ld, P = (size_t)h->P;
    *grid = grid_1d(h->P, kTriThreads, h->n_cu);
    return ensure_all(h, {
        {&s.x, sizeof(double) * (size_t)h->n}, {&s.tab, sizeof(double) * cam_table_doubles((int)h->C)},
        {&s.use, ldz}, {&t.select, P}, {&t.X, sizeof(double) * 3 * P}, {&t.ints, sizeof(int) * 3 * P},
        {&t.dbl, sizeof(double) * 2 * P}, {&t.ok_part, sizeof(int) * (size_t)*grid}});
}

TriOptions tri_options(const sfmba_triangulate_options& o) {
    return TriOptions{(int)o.max_iter, (int)o.min_views, o.xtol, o.min_angle_deg, o.min_depth, o.max_error_px};
}

// the table of stats_prepare(h, x) must be in place; use [ld, stored order] / select [P]: masks on the device, null: all
int launch_triangulate(sfmba_handle* h, const TriOptions& opt, const unsigned char* use, const unsigned char* select, int grid) {
    auto& s = h->stats;
    auto& t = h->tri;
    const size_t P = (size_t)h->P;
    const bool lds_tab = h->forms.lds_tab;
    const size_t lds = lds_tab ? (size_t)h->C * kCamRT * sizeof(double) : 0;
    auto kern = lds_tab ? (h->f32 ? k_triangulate<true, true> : k_triangulate<true, false>)
                        : (h->f32 ? k_triangulate<false, true> : k_triangulate<false, false>);
    CHK(set_lds(h, kern, lds));
    const TriIn in{h->pt_ptr.as<int>(), h->cam_idx.as<int>(), h->uv.as<double>(),
                   use, select, s.x.as<double>() + 6 * h->C};
    const TriOut out{t.X.as<double>(), t.ints.as<int>(), t.ints.as<int>() + P, t.ints.as<int>() + 2 * P,
                     t.dbl.as<double>(), t.dbl.as<double>() + P, t.ok_part.as<int>()};
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kTriThreads), lds, h->stream, (const double*)s.tab.as<double>(), in, (int)h->P,
                       (int)h->C, h->K, opt, out);
    LAUNCHED(h);
    return 0;
}

}  // namespace

void sfmba_default_triangulate_options(sfmba_triangulate_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_iter = 10; o->min_views = 2; o->xtol = 1e-10; o->min_angle_deg = 1.0; o->min_depth = 0.0; o->max_error_px = INFINITY;
}

int sfmba_triangulate(sfmba_handle* h, const double* x, const uint8_t* pt_select, const uint8_t* obs_use,
                      const sfmba_triangulate_options* opt, double* X_out, int32_t* pt_status, int32_t* pt_views,
                      int32_t* pt_iters, double* pt_rms_err, double* pt_angle_deg, int64_t* n_ok) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    sfmba_triangulate_options o;
    if (opt) o = *opt; else sfmba_default_triangulate_options(&o);
    if (std::isnan(o.xtol) || std::isnan(o.min_angle_deg) || std::isnan(o.min_depth) || std::isnan(o.max_error_px))
        return fail(h, -1, "an option of sfmba_triangulate is NaN");
    auto& t = h->tri;
    const size_t P = (size_t)h->P;
    int grid = 1, *counts = nullptr;
    CHK(tri_allocate(h, &grid));
    CHK(stats_prepare(h, x));
    CHK(stage_masks(h, obs_use, pt_select, P, t.select, (size_t)grid, &counts));
    CHK(launch_triangulate(h, tri_options(o), obs_use ? h->stats.use.as<unsigned char>() : nullptr,
                           pt_select ? t.select.as<unsigned char>() : nullptr, grid));
    const int* pi = t.ints.as<int>();
    HIPCHK(h, download(h, X_out, t.X.p, sizeof(double) * 3 * P));
    HIPCHK(h, download(h, pt_status, pi, sizeof(int32_t) * P));
    HIPCHK(h, download(h, pt_views, pi + P, sizeof(int32_t) * P));
    HIPCHK(h, download(h, pt_iters, pi + 2 * P, sizeof(int32_t) * P));
    HIPCHK(h, download(h, pt_rms_err, t.dbl.p, sizeof(double) * P));
    HIPCHK(h, download(h, pt_angle_deg, t.dbl.as<double>() + P, sizeof(double) * P));
    return finish_with_ok_count(h, t.ok_part.as<int>(), (size_t)grid, counts, n_ok);
}

namespace {
// ---- robust triangulation (sfmba_triangulate_ransac; kernel: consumer_kernels.hpp, "Robust triangulation") ---------------
TriRansacOptions tri_ransac_options(const sfmba_tri_ransac_options& o) {
    return TriRansacOptions{(int)o.max_pairs, std::max((int)o.min_views, 2), o.threshold * o.threshold, o.min_depth,
                            o.min_pair_angle_deg, (unsigned long long)o.seed};
}

// sfmba_triangulate's buffers (k_triangulate runs last) and the call's own
int tri_ransac_allocate(sfmba_handle* h, int H, bool hyp, int* grid, int* tri_grid) {
    auto& q = h->tri_ransac;
    const size_t ldz = (size_t)h->ld, P = (size_t)h->P;
    *grid = grid_1d(h->P, kTriRansacThreads, h->n_cu);
    CHK(tri_allocate(h, tri_grid));
    return ensure_all(h, {{&q.mask, ldz}, {&q.ok, P}, {&q.X_hyp, sizeof(double) * 3 * P}, {&q.ints, sizeof(int) * 4 * P},
                          {&q.hyp, hyp ? sizeof(int) * P * (size_t)H : 0}});
}

// what k_tri_ransac finds in place: a mask of zeros (only a valid best hypothesis writes its run), counts of -1
int tri_ransac_clear(sfmba_handle* h, int H, bool hyp) {
    auto& q = h->tri_ransac;
    if (h->ld) HIPCHK(h, hipMemsetAsync(q.mask.p, 0, (size_t)h->ld, h->stream));
    if (hyp && h->P) HIPCHK(h, hipMemsetAsync(q.hyp.p, 0xff, sizeof(int) * (size_t)h->P * (size_t)H, h->stream));
    return 0;
}

// k_tri_ransac, then k_triangulate over its mask for the points whose best count reaches the need.  The table of
// stats_prepare(h, x) and the cleared buffers must be in place; use / select: the caller's masks are on the device
int launch_tri_ransac(sfmba_handle* h, const TriRansacOptions& ro, const TriOptions& to, bool use, bool select, bool hyp, int grid,
                      int tri_grid) {
    auto& s = h->stats;
    auto& q = h->tri_ransac;
    const size_t P = (size_t)h->P;
    const bool lds_tab = h->forms.lds_tab;
    const size_t lds = lds_tab ? (size_t)h->C * kCamRT * sizeof(double) : 0;
    auto kern = lds_tab ? (h->f32 ? k_tri_ransac<true, true> : k_tri_ransac<true, false>)
                        : (h->f32 ? k_tri_ransac<false, true> : k_tri_ransac<false, false>);
    // About 3 KiB of static LDS (kTriRansacStaticLds bounds it) stand beside the table: the opt-in is asked for as soon as
    // the two together pass 64 KiB, and leaves that room below the 160 KiB of a CU.
    static_assert(sizeof(int) * (3 * kTriRansacThreads + 1) + 2 * sizeof(long long) * (kTrackBlock / 64) <= kTriRansacStaticLds, "");
    if (lds + kTriRansacStaticLds > 64 * 1024)
        CHK(opt_in_lds(h, reinterpret_cast<const void*>(kern), kLdsDynMax + 2048 - kTriRansacStaticLds));
    const TriIn in{h->pt_ptr.as<int>(), h->cam_idx.as<int>(), h->uv.as<double>(), use ? s.use.as<unsigned char>() : nullptr,
                   select ? h->tri.select.as<unsigned char>() : nullptr, s.x.as<double>() + 6 * h->C};
    int* const qi = q.ints.as<int>();
    const TriRansacOut out{q.X_hyp.as<double>(), q.mask.as<unsigned char>(), q.ok.as<unsigned char>(), qi, qi + P, qi + 2 * P,
                           qi + 3 * P, hyp ? q.hyp.as<int>() : nullptr};
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kTriRansacThreads), lds, h->stream, (const double*)s.tab.as<double>(), in, (int)h->P,
                       (int)h->C, h->K, ro, out);
    LAUNCHED(h);
    return launch_triangulate(h, to, q.mask.as<unsigned char>(), q.ok.as<unsigned char>(), tri_grid);
}

}  // namespace

void sfmba_default_tri_ransac_options(sfmba_tri_ransac_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->threshold = 4.0; o->min_depth = 0.0; o->min_pair_angle_deg = 1.0; o->seed = 0; o->max_pairs = 64; o->min_views = 2;
    o->refine = 1; o->profile = 0; o->max_iter = 10; o->xtol = 1e-10; o->min_angle_deg = 1.0; o->max_error_px = INFINITY;
}

int sfmba_triangulate_ransac(sfmba_handle* h, const double* x, const uint8_t* pt_select, const uint8_t* obs_use,
                             const sfmba_tri_ransac_options* opt, double* X_out, double* X_hyp, uint8_t* inlier_mask,
                             int32_t* pt_status, int32_t* pt_views, int32_t* pt_inliers, int32_t* pt_best, int32_t* pt_iters,
                             double* pt_rms_err, double* pt_angle_deg, int32_t* hyp_inliers, int64_t* n_ok, double* kernel_us) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    sfmba_tri_ransac_options o;
    if (opt) o = *opt; else sfmba_default_tri_ransac_options(&o);
    if (std::isnan(o.threshold) || std::isnan(o.min_depth) || std::isnan(o.min_pair_angle_deg) || std::isnan(o.xtol) ||
        std::isnan(o.min_angle_deg) || std::isnan(o.max_error_px))
        return fail(h, -1, "an option of sfmba_triangulate_ransac is NaN");
    if (o.max_pairs < 1) return fail(h, -1, "sfmba_triangulate_ransac: max_pairs must be at least 1");
    const size_t P = (size_t)h->P, N = (size_t)h->N, H = (size_t)o.max_pairs;
    if (hyp_inliers && P * H >= (size_t)1 << 31)
        return fail(h, -1, "sfmba_triangulate_ransac: hyp_inliers of %zu points x %zu pairs passes 2^31 entries", P, H);
    if (n_ok) *n_ok = 0;
    if (kernel_us) *kernel_us = 0.0;
    auto& t = h->tri;
    auto& q = h->tri_ransac;
    const TriRansacOptions ro = tri_ransac_options(o);
    const TriOptions to{o.refine != 0 ? (int)o.max_iter : 0, (int)o.min_views, o.xtol, o.min_angle_deg, o.min_depth, o.max_error_px};
    int grid = 1, tri_grid = 1, *counts = nullptr;
    CHK(tri_ransac_allocate(h, ro.H, hyp_inliers != nullptr, &grid, &tri_grid));
    CHK(stats_prepare(h, x));
    CHK(stage_masks(h, obs_use, pt_select, P, t.select, 0, &counts));
    // the staging of what the host combines: status, views, inliers, best | k_triangulate's status; the mask
    const size_t off_mask = sizeof(int) * 5 * P;
    HIPCHK(h, q.host.ensure(off_mask + N + 64, 0));
    int* const hi = q.host.as<int>();
    unsigned char* const hm = q.host.as<unsigned char>() + off_mask;
    EventPair timer;
    CHK(timer.start(h, o.profile != 0));
    CHK(tri_ransac_clear(h, ro.H, hyp_inliers != nullptr));
    CHK(launch_tri_ransac(h, ro, to, obs_use != nullptr, pt_select != nullptr, hyp_inliers != nullptr, grid, tri_grid));
    CHK(timer.stop(h));
    // k_triangulate leaves the point of x, 0, NaN, NaN wherever it did not run or gave no new point: those four as they are
    const int* ti = t.ints.as<int>();
    HIPCHK(h, download(h, X_out, t.X.p, sizeof(double) * 3 * P));
    HIPCHK(h, download(h, X_hyp, q.X_hyp.p, sizeof(double) * 3 * P));
    HIPCHK(h, download(h, pt_iters, ti + 2 * P, sizeof(int32_t) * P));
    HIPCHK(h, download(h, pt_rms_err, t.dbl.p, sizeof(double) * P));
    HIPCHK(h, download(h, pt_angle_deg, t.dbl.as<double>() + P, sizeof(double) * P));
    HIPCHK(h, download(h, hyp_inliers, q.hyp.p, sizeof(int32_t) * P * H));
    if (P) {
        HIPCHK(h, hipMemcpyAsync(hi, q.ints.p, sizeof(int) * 4 * P, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(hi + 4 * P, ti, sizeof(int) * P, hipMemcpyDeviceToHost, h->stream));
    }
    if (inlier_mask && N) HIPCHK(h, hipMemcpyAsync(hm, q.mask.p, N, hipMemcpyDeviceToHost, h->stream));
    CHK(wait_stream(h));
    CHK(timer.read(h, kernel_us));
    if (inlier_mask)
        for (size_t k = 0; k < N; ++k) inlier_mask[caller_position(h, k)] = hm[k];
    int64_t ok = 0;
    for (size_t p = 0; p < P; ++p) {
        const int status = hi[p] == kTriOk ? hi[4 * P + p] : hi[p];      // RANSAC found a consensus: k_triangulate's verdict counts
        if (pt_status) pt_status[p] = status;
        if (pt_views) pt_views[p] = hi[P + p];
        if (pt_inliers) pt_inliers[p] = hi[2 * P + p];
        if (pt_best) pt_best[p] = hi[3 * P + p];
        ok += status == kTriOk ? 1 : 0;
    }
    if (n_ok) *n_ok = ok;
    return 0;
}

namespace {
// ---- resection (sfmba_resect; kernel: consumer_kernels.hpp, "Resection") ----------------------------------------------------
int resect_allocate(sfmba_handle* h) {
    auto& r = h->resect;
    const size_t ldz = (size_t)h->ld, C = (size_t)h->C;
    return ensure_all(h, {
        {&h->stats.x, sizeof(double) * (size_t)h->n}, {&h->stats.use, ldz}, {&r.select, C}, {&r.cam, sizeof(double) * 6 * C},
        {&r.ints, sizeof(int) * 4 * C}, {&r.rms, sizeof(double) * C}});
}

ResectOptions resect_options(const sfmba_resect_options& o) {
    return ResectOptions{(int)o.max_iter, (int)o.min_views, o.start != 0 ? 1 : 0, o.xtol, o.min_depth, o.max_rms_px};
}

// K^-1 by the adjugate (the pixels of the linear stage are normalised with it)
KMat inverse_k(const KMat& K) {
    const double* k = K.k;
    const double c00 = k[4] * k[8] - k[5] * k[7], c01 = k[5] * k[6] - k[3] * k[8], c02 = k[3] * k[7] - k[4] * k[6];
    const double det = k[0] * c00 + k[1] * c01 + k[2] * c02;
    KMat inv;
    inv.k[0] = c00 / det; inv.k[1] = (k[2] * k[7] - k[1] * k[8]) / det; inv.k[2] = (k[1] * k[5] - k[2] * k[4]) / det;
    inv.k[3] = c01 / det; inv.k[4] = (k[0] * k[8] - k[2] * k[6]) / det; inv.k[5] = (k[2] * k[3] - k[0] * k[5]) / det;
    inv.k[6] = c02 / det; inv.k[7] = (k[1] * k[6] - k[0] * k[7]) / det; inv.k[8] = (k[0] * k[4] - k[1] * k[3]) / det;
    return inv;
}

// x must be in stats.x and the permutation of stats_cam_perm(h) in place; use / select: the masks on the device ([ld]
// stored order / [C]), null: every observation / camera; perm: another order of the entries inside the cameras' slices
// (null: the permutation itself)
int launch_resect(sfmba_handle* h, const ResectOptions& opt, const unsigned char* use, const unsigned char* select,
                  const int* perm = nullptr) {
    auto& s = h->stats;
    auto& r = h->resect;
    const size_t C = (size_t)h->C;
    if (C == 0) return 0;
    const ResectIn in{s.cam_ptr.as<int>(), perm ? perm : s.perm.as<int>(), h->pt_idx.as<int>(), h->uv.as<double>(),
                      use, select, s.x.as<double>()};
    const ResectOut out{r.cam.as<double>(), r.ints.as<int>(), r.ints.as<int>() + C, r.ints.as<int>() + 2 * C,
                        r.rms.as<double>(), r.ints.as<int>() + 3 * C};
    auto kern = h->f32 ? k_resect<true> : k_resect<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)C), dim3(kCamThreads), 0, h->stream, in, (int)h->C, h->K, inverse_k(h->K), opt, out);
    LAUNCHED(h);
    return 0;
}

int resect_check_single(sfmba_handle* h) {
    if (multi_rank(h) || h->N_total != h->N)
        return fail(h, -1, "sfmba_resect needs every observation of a camera: this handle holds a shard of the problem");
    return 0;
}

}  // namespace

void sfmba_default_resect_options(sfmba_resect_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_iter = 20; o->min_views = 6; o->start = 0; o->xtol = 1e-10; o->min_depth = 0.0; o->max_rms_px = INFINITY;
}

int sfmba_resect(sfmba_handle* h, const double* x, const uint8_t* cam_select, const uint8_t* obs_use,
                 const sfmba_resect_options* opt, double* cam_out, int32_t* cam_status, int32_t* cam_views,
                 int32_t* cam_iters, double* cam_rms_err, int64_t* n_ok) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    sfmba_resect_options o;
    if (opt) o = *opt; else sfmba_default_resect_options(&o);
    if (std::isnan(o.xtol) || std::isnan(o.min_depth) || std::isnan(o.max_rms_px))
        return fail(h, -1, "an option of sfmba_resect is NaN");
    CHK(resect_check_single(h));
    auto& r = h->resect;
    const size_t C = (size_t)h->C;
    int* counts = nullptr;
    CHK(resect_allocate(h));
    CHK(upload_x(h, x, h->stats.x.as<double>()));
    CHK(stats_cam_perm(h));
    CHK(stage_masks(h, obs_use, cam_select, C, r.select, C, &counts));
    CHK(launch_resect(h, resect_options(o), obs_use ? h->stats.use.as<unsigned char>() : nullptr,
                      cam_select ? r.select.as<unsigned char>() : nullptr));
    const int* pi = r.ints.as<int>();
    HIPCHK(h, download(h, cam_out, r.cam.p, sizeof(double) * 6 * C));
    HIPCHK(h, download(h, cam_status, pi, sizeof(int32_t) * C));
    HIPCHK(h, download(h, cam_views, pi + C, sizeof(int32_t) * C));
    HIPCHK(h, download(h, cam_iters, pi + 2 * C, sizeof(int32_t) * C));
    HIPCHK(h, download(h, cam_rms_err, r.rms.p, sizeof(double) * C));
    return finish_with_ok_count(h, pi + 3 * C, C, counts, n_ok);
}

namespace {
// ---- two-view geometry (sfmba_fundamental_ransac, sfmba_recover_pose; kernels: consumer_kernels.hpp, "Two-view geometry") ----
struct TwoViewBatch { size_t E = 0, M = 0, Mu = 0; bool masked = false; int max_n = 0; };

// The batch onto the device: the used pairs of every edge packed x1 y1 x2 y2 in stored order -> twoview.pairs, their runs
// -> twoview.uptr; twoview.pos maps a used pair back to its stored place when there is a mask.  dim: the coordinates of a
// point (2: pixels; 3: the sets of sfmba_similarity_ransac, packed sx sy sz dx dy dz).
int twoview_stage(sfmba_handle* h, const char* who, int64_t n_edges, const int64_t* edge_ptr, const double* pts1,
                  const double* pts2, const uint8_t* pair_use, TwoViewBatch* bt, size_t dim = 2) {
    auto& t = h->twoview;
    if (n_edges < 0 || !edge_ptr) return fail(h, -1, "%s: n_edges is negative or edge_ptr is NULL", who);
    if (edge_ptr[0] != 0) return fail(h, -1, "%s: edge_ptr[0] must be 0", who);
    for (int64_t e = 0; e < n_edges; ++e)
        if (edge_ptr[e + 1] < edge_ptr[e]) return fail(h, -1, "%s: edge_ptr must ascend (edge %lld)", who, (long long)e);
    const size_t E = (size_t)n_edges, M = (size_t)edge_ptr[n_edges];
    if (M >= (size_t)1 << 31 || E >= (size_t)1 << 31) return fail(h, -1, "%s: the batch has 2^31 pairs or edges, or more", who);
    if (M && (!pts1 || !pts2)) return fail(h, -1, "%s: pts1 or pts2 is NULL", who);
    const size_t off_ptr = sizeof(double) * 2 * dim * M;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, t.in_host.ensure(off_ptr + sizeof(int) * (E + 1), 0));
    double* const pk = t.in_host.as<double>();
    int* const up = reinterpret_cast<int*>(t.in_host.as<unsigned char>() + off_ptr);
    t.pos.clear();
    size_t u = 0;
    int max_n = 0;
    for (size_t e = 0; e < E; ++e) {
        up[e] = (int)u;
        for (size_t k = (size_t)edge_ptr[e]; k < (size_t)edge_ptr[e + 1]; ++k) {
            if (pair_use && !pair_use[k]) continue;
            for (size_t i = 0; i < dim; ++i) { pk[2 * dim * u + i] = pts1[dim * k + i]; pk[2 * dim * u + dim + i] = pts2[dim * k + i]; }
            if (pair_use) t.pos.push_back((int64_t)k);
            ++u;
        }
        max_n = std::max(max_n, (int)u - up[e]);
    }
    up[E] = (int)u;
    CHK(ensure_all(h, {{&t.pairs, sizeof(double) * 2 * dim * std::max<size_t>(u, 1)}, {&t.uptr, sizeof(int) * (E + 1)}}));
    if (u) HIPCHK(h, hipMemcpyAsync(t.pairs.p, pk, sizeof(double) * 2 * dim * u, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(t.uptr.p, up, sizeof(int) * (E + 1), hipMemcpyHostToDevice, h->stream));
    bt->E = E; bt->M = M; bt->Mu = u; bt->masked = pair_use != nullptr; bt->max_n = max_n;
    return 0;
}

// a per-pair result from its packed order in the staging (src) into the caller's stored order, `bytes` per pair; pairs
// that took no part get the `bytes` at `fill`
void twoview_scatter(const sfmba_handle* h, const TwoViewBatch& bt, const void* src, void* dst, size_t bytes, const void* fill) {
    if (!dst) return;
    if (!bt.masked) { memcpy(dst, src, bytes * bt.Mu); return; }
    unsigned char* const d = static_cast<unsigned char*>(dst);
    const unsigned char* const sp = static_cast<const unsigned char*>(src);
    for (size_t k = 0; k < bt.M; ++k) memcpy(d + bytes * k, fill, bytes);
    const auto& pos = h->twoview.pos;
    for (size_t u = 0; u < bt.Mu; ++u) memcpy(d + bytes * (size_t)pos[u], sp + bytes * u, bytes);
}

// The H hypotheses of one item of a RANSAC batch (an edge, a camera) in slices of *hs, a workgroup each: about two per CU over
// the batch, no slice below min_slice -- at most H / min_slice slices, rounded up (two-view) or down to at least one (P3P)
void ransac_slices(int n_cu, size_t batch, int H, int min_slice, bool round_up, int* hs, int* n_slices) {
    const size_t want = (2 * (size_t)n_cu + batch - 1) / std::max<size_t>(batch, 1);
    const int most = round_up ? (H + min_slice - 1) / min_slice : std::max(H / min_slice, 1);
    const int sl = (int)std::min<size_t>(std::max<size_t>(want, 1), (size_t)most);
    *hs = (H + sl - 1) / sl;
    *n_slices = (H + *hs - 1) / *hs;
}

// caller-given samples [batch][H][S]: the positions of an item with count(i) >= need entries (else not read) lie inside them
template <class Count>
int check_samples(sfmba_handle* h, const int32_t* samples, size_t batch, size_t H, size_t S, Count count, int need, const char* who,
                  const char* item, const char* entries) {
    for (size_t i = 0; i < batch; ++i) {
        const int n = count(i);
        if (n < need) continue;
        const int32_t* sp = samples + i * H * S;
        for (size_t k = 0; k < S * H; ++k)
            if (sp[k] < 0 || sp[k] >= n)
                return fail(h, -1, "%s: samples of %s %zu, hypothesis %zu: position %d is outside its %d used %s", who, item, i, k / S,
                            (int)sp[k], n, entries);
    }
    return 0;
}

// What sfmba_fundamental_ransac (S = 8 positions a sample), sfmba_homography_ransac (S = 4) and sfmba_essential_ransac (S = 5)
// do alike before their kernels: options, the batch onto the device, the slices, slots / counts / samples buffers, the
// caller's samples checked and uploaded, the LDS opt-in of the RANSAC kernel.
struct TwoViewRansac {
    size_t slot_doubles = kTwoViewSlot;          // of a slot of the RANSAC kernel
    size_t hyp_arrays = 1;                       // per-hypothesis integer arrays [n_edges][H] in twoview.hyp, one behind the other
    size_t dim = 2;                              // coordinates of a point of a pair (3: sfmba_similarity_ransac)
    size_t model_doubles = 9;                    // of the model and of its refit in twoview.F
    int min_slice = kTwoViewMinSlice, lds_pairs = kTwoViewLdsPairs;      // of the RANSAC kernel
    const char* item = "edge";                   // what an entry of the batch is called in an error text
    sfmba_ransac_options o;
    TwoViewBatch bt;
    size_t E = 0, H = 0;
    int hs = 1, n_slices = 1;
    FundIn in{};
};

// (E = 0 on return: the batch has no edge and nothing was launched)
int twoview_ransac_begin(sfmba_handle* h, const char* who, const void* lds_kernel, int S, int64_t n_edges, const int64_t* edge_ptr, const double* pts1,
                         const double* pts2, const uint8_t* pair_use, const int32_t* samples, const sfmba_ransac_options* opt,
                         bool hyp, int64_t* n_ok, double* kernel_us, TwoViewRansac* c) {
    if (opt) c->o = *opt; else sfmba_default_ransac_options(&c->o);
    if (std::isnan(c->o.threshold) || std::isnan(c->o.confidence)) return fail(h, -1, "an option of %s is NaN", who);
    if (c->o.max_iters < 1) return fail(h, -1, "%s: max_iters must be at least 1", who);
    auto& t = h->twoview;
    CHK(twoview_stage(h, who, n_edges, edge_ptr, pts1, pts2, pair_use, &c->bt, c->dim));
    if (n_ok) *n_ok = 0;
    if (kernel_us) *kernel_us = 0.0;
    const size_t E = c->bt.E, H = (size_t)c->o.max_iters;
    c->H = H;
    if (E == 0) return 0;
    ransac_slices(h->n_cu, E, (int)H, c->min_slice, true, &c->hs, &c->n_slices);
    if (E * (size_t)c->n_slices >= (size_t)1 << 31) return fail(h, -1, "%s: too many edges for one launch", who);
    CHK(ensure_all(h, {{&t.slots, sizeof(double) * c->slot_doubles * E * (size_t)c->n_slices},
                       {&t.hyp, hyp ? sizeof(int) * c->hyp_arrays * E * H : 0},
                       {&t.samples, samples ? sizeof(int) * (size_t)S * E * H : 0}}));
    if (samples) {
        const int* up = reinterpret_cast<const int*>(t.in_host.as<unsigned char>() + sizeof(double) * 2 * c->dim * c->bt.M);
        CHK(check_samples(h, samples, E, H, (size_t)S, [&](size_t e) { return up[e + 1] - up[e]; }, S,   // (below: FEW_PAIRS)
                          who, c->item, "pairs"));
        HIPCHK(h, hipMemcpyAsync(t.samples.p, samples, sizeof(int) * (size_t)S * E * H, hipMemcpyHostToDevice, h->stream));
    }
    // the kernel's static LDS (about 8 KiB, above the 2 KiB that set_lds assumes) counts: opted in whatever this call stages
    CHK(opt_in_lds(h, lds_kernel, sizeof(double) * 2 * c->dim * (size_t)c->lds_pairs));
    c->in = FundIn{t.pairs.as<double>(), t.uptr.as<int>(), samples ? t.samples.as<int>() : nullptr};
    c->E = E;
    return 0;
}

// a model's RANSAC kernel over the (edge, slice) grid: the arguments the kernels begin with alike, then the model's `own`
template <class Kern, class... Own>
int launch_twoview_ransac(sfmba_handle* h, const TwoViewRansac& c, Kern kern, double score, Own... own) {
    const size_t lds = sizeof(double) * 2 * c.dim * (size_t)std::min(c.bt.max_n, c.lds_pairs);
    hipLaunchKernelGGL(kern, dim3((unsigned)(c.E * (size_t)c.n_slices)), dim3(kTwoViewThreads), lds, h->stream, c.in, (int)c.H, c.hs,
                       c.n_slices, (unsigned long long)c.o.seed, score, own...);
    LAUNCHED(h);
    return 0;
}

// the caller's arrays of a two-view RANSAC call (any may be null): the model and its refit [E][9], the masks [M] (the
// second: of the refit, a model with two), the per-edge integers in the kernel's order with success as bytes
struct TwoViewResults {
    double *M, *M_refit;
    uint8_t* mask[2];
    int32_t *inliers, *best, *status;
    uint8_t* success;
    int32_t *refit_inliers, *hyp;                // (refit_inliers: the fifth integer of an edge, whatever the model keeps there)
    int64_t* n_ok;
    double* kernel_us;
    int32_t* hyp2 = nullptr;                     // the second per-hypothesis array of a call with two
};

// What the three calls do alike after twoview_ransac_begin: the result buffers (twoview.F the model and its refit,
// twoview.mask n_masks masks, twoview.ints n_ints integers per edge), `launch` (the model's RANSAC and finish kernels on
// these buffers) between the event pair, the downloads, the masks scattered, the integers handed out.
template <class Launch>
int twoview_ransac_end(sfmba_handle* h, const TwoViewRansac& c, double score, size_t n_ints, size_t n_masks, int ok_status,
                       const TwoViewResults& r, Launch launch) {
    if (c.E == 0) return wait_stream(h);
    auto& t = h->twoview;
    const TwoViewBatch& bt = c.bt;
    const size_t E = c.E, H = c.H, Mu = bt.Mu;
    const size_t P = c.model_doubles;
    CHK(ensure_all(h, {{&t.F, sizeof(double) * 2 * P * E}, {&t.ints, sizeof(int) * n_ints * E}, {&t.mask, n_masks * std::max<size_t>(Mu, 1)}}));
    EventPair timer;
    CHK(timer.start(h, c.o.profile != 0));
    CHK(launch(t.F.as<double>(), t.mask.as<unsigned char>(), t.ints.as<int>(), score));
    CHK(timer.stop(h));
    // the per-edge integers always come (n_ok); the masks through the staging when they have to be scattered
    const size_t off_mask = sizeof(int) * n_ints * E;
    HIPCHK(h, t.out_host.ensure(off_mask + n_masks * Mu, 0));
    int* const hi = t.out_host.as<int>();
    unsigned char* const hm = t.out_host.as<unsigned char>() + off_mask;
    HIPCHK(h, hipMemcpyAsync(hi, t.ints.p, sizeof(int) * n_ints * E, hipMemcpyDeviceToHost, h->stream));
    if ((r.mask[0] || r.mask[1]) && Mu) HIPCHK(h, hipMemcpyAsync(hm, t.mask.p, n_masks * Mu, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, download(h, r.M, t.F.p, sizeof(double) * P * E));
    HIPCHK(h, download(h, r.M_refit, t.F.as<double>() + P * E, sizeof(double) * P * E));
    HIPCHK(h, download(h, r.hyp, t.hyp.p, sizeof(int) * E * H));
    if (r.hyp2) HIPCHK(h, download(h, r.hyp2, t.hyp.as<int>() + E * H, sizeof(int) * E * H));
    CHK(wait_stream(h));
    CHK(timer.read(h, r.kernel_us));
    const uint8_t zero = 0;
    for (size_t m = 0; m < n_masks; ++m) twoview_scatter(h, bt, hm + m * Mu, r.mask[m], 1, &zero);
    int64_t ok = 0;
    for (size_t e = 0; e < E; ++e) {
        const int* const ei = hi + n_ints * e;
        if (r.inliers) r.inliers[e] = ei[0];
        if (r.best) r.best[e] = ei[1];
        if (r.status) r.status[e] = ei[2];
        if (r.success) r.success[e] = (uint8_t)ei[3];
        if (r.refit_inliers) r.refit_inliers[e] = ei[4];
        ok += ei[2] == ok_status ? 1 : 0;
    }
    if (r.n_ok) *r.n_ok = ok;
    return 0;
}

// ---- robust resection (sfmba_resect_ransac; kernels: consumer_kernels.hpp, "Robust resection") ----------------------------
struct PnpCall { int H, hs, n_slices; PnpScore sc; double confidence; unsigned long long seed; };

PnpCall pnp_call(const sfmba_handle* h, const sfmba_pnp_ransac_options& o) {
    PnpCall pc{};
    pc.H = (int)o.max_iters;
    ransac_slices(h->n_cu, (size_t)h->C, pc.H, kPnpMinSlice, false, &pc.hs, &pc.n_slices);
    pc.sc = PnpScore{o.threshold * o.threshold, o.min_depth, std::max((int)o.min_views, 4)};
    pc.confidence = o.confidence;
    pc.seed = (unsigned long long)o.seed;
    return pc;
}

int pnp_allocate(sfmba_handle* h, const PnpCall& pc, bool samples, bool hyp) {
    auto& q = h->pnp;
    const size_t ldz = (size_t)h->ld, C = (size_t)h->C, H = (size_t)pc.H;
    if (C * (size_t)pc.n_slices >= (size_t)1 << 31) return fail(h, -1, "sfmba_resect_ransac: too many cameras for one launch");
    CHK(resect_allocate(h));
    return ensure_all(h, {
        {&q.select, C}, {&q.ok, C}, {&q.mask, ldz}, {&q.corr, sizeof(double) * kPnpCorr * ldz}, {&q.cpos, sizeof(int) * ldz},
        {&q.cn, sizeof(int) * C}, {&q.samples, samples ? sizeof(int) * 3 * C * H : 0},
        {&q.slots, sizeof(double) * kPnpSlot * C * (size_t)pc.n_slices}, {&q.hyp, hyp ? sizeof(int) * C * H : 0},
        {&q.pose, sizeof(double) * 6 * C}, {&q.ints, sizeof(int) * 6 * C}});
}

PnpIn pnp_in(sfmba_handle* h, bool samples) {
    auto& q = h->pnp;
    return PnpIn{q.corr.as<double>(), h->stats.cam_ptr.as<int>(), q.cn.as<int>(), samples ? q.samples.as<int>() : nullptr};
}

// x must be in stats.x and the permutation of stats_cam_perm(h) in place; use / select: the masks are on the device
int launch_pnp_gather(sfmba_handle* h, bool use, bool select) {
    auto& s = h->stats;
    auto& q = h->pnp;
    const ResectIn in{s.cam_ptr.as<int>(), s.perm.as<int>(), h->pt_idx.as<int>(), h->uv.as<double>(),
                      use ? s.use.as<unsigned char>() : nullptr, select ? q.select.as<unsigned char>() : nullptr,
                      s.x.as<double>()};
    auto kern = h->f32 ? k_pnp_gather<true> : k_pnp_gather<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)h->C), dim3(kPnpThreads), 0, h->stream, in, (int)h->C, q.corr.as<double>(),
                       q.cpos.as<int>(), q.cn.as<int>(), q.mask.as<unsigned char>());
    LAUNCHED(h);
    return 0;
}

// k_pnp_ransac and k_pnp_finish behind k_pnp_gather
int launch_pnp_ransac(sfmba_handle* h, const PnpCall& pc, bool samples, bool hyp, bool select) {
    auto& q = h->pnp;
    const size_t C = (size_t)h->C;
    constexpr size_t lds = sizeof(double) * ((size_t)kPnpWaves * kPnpSlabDoubles + (size_t)kPnpCorr * kPnpLdsObs);
    static_assert(lds + 1024 <= 160 * 1024, "slabs and staged correspondences must fit the LDS of a CU");
    CHK(opt_in_lds(h, reinterpret_cast<const void*>(k_pnp_ransac), lds));       // more than 64 KiB of LDS
    const PnpIn in = pnp_in(h, samples);
    hipLaunchKernelGGL(k_pnp_ransac, dim3((unsigned)(C * (size_t)pc.n_slices)), dim3(kPnpThreads), lds, h->stream, in, pc.H, pc.hs,
                       pc.n_slices, pc.seed, h->K, inverse_k(h->K), pc.sc, q.slots.as<double>(), hyp ? q.hyp.as<int>() : nullptr);
    LAUNCHED(h);
    const PnpOut out{h->stats.x.as<double>(), q.pose.as<double>(), q.mask.as<unsigned char>(), q.ok.as<unsigned char>(),
                     q.ints.as<int>()};
    hipLaunchKernelGGL(k_pnp_finish, dim3((unsigned)C), dim3(kPnpThreads), 0, h->stream, in, (const int*)q.cpos.as<int>(),
                       (const unsigned char*)(select ? q.select.as<unsigned char>() : nullptr), pc.n_slices, h->K, pc.sc,
                       pc.confidence, (const double*)q.slots.as<double>(), out);
    LAUNCHED(h);
    return 0;
}

}  // namespace

void sfmba_default_pnp_ransac_options(sfmba_pnp_ransac_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->threshold = 8.0; o->confidence = 0.99; o->min_depth = 0.0; o->seed = 0; o->max_iters = 256; o->min_views = 6;
    o->refine = 1; o->profile = 0; o->max_iter = 20; o->xtol = 1e-10; o->max_rms_px = INFINITY;
}

int sfmba_resect_ransac(sfmba_handle* h, const double* x, const uint8_t* cam_select, const uint8_t* obs_use, const int32_t* samples,
                        const sfmba_pnp_ransac_options* opt, double* cam_out, double* cam_hyp, uint8_t* inlier_mask,
                        int32_t* cam_status, int32_t* cam_views, int32_t* cam_inliers, int32_t* cam_best, int32_t* cam_best_sol,
                        uint8_t* cam_success, int32_t* cam_iters, double* cam_rms_err, int32_t* hyp_inliers, int64_t* n_ok,
                        double* kernel_us) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    sfmba_pnp_ransac_options o;
    if (opt) o = *opt; else sfmba_default_pnp_ransac_options(&o);
    if (std::isnan(o.threshold) || std::isnan(o.confidence) || std::isnan(o.min_depth) || std::isnan(o.xtol) || std::isnan(o.max_rms_px))
        return fail(h, -1, "an option of sfmba_resect_ransac is NaN");
    if (o.max_iters < 1) return fail(h, -1, "sfmba_resect_ransac: max_iters must be at least 1");
    CHK(resect_check_single(h));
    if (n_ok) *n_ok = 0;
    if (kernel_us) *kernel_us = 0.0;
    auto& q = h->pnp;
    auto& r = h->resect;
    const size_t C = (size_t)h->C, N = (size_t)h->N;
    if (C == 0) return wait_stream(h);
    const PnpCall pc = pnp_call(h, o);
    const size_t H = (size_t)pc.H;
    int* counts = nullptr;
    CHK(pnp_allocate(h, pc, samples != nullptr, hyp_inliers != nullptr));
    CHK(upload_x(h, x, h->stats.x.as<double>()));
    CHK(stats_cam_perm(h));
    CHK(stage_masks(h, obs_use, cam_select, C, q.select, 0, &counts));
    // the results' staging: doubles first (pose, k_resect's pose and rms), then the integers (ours, k_resect's), the mask
    const size_t off_ints = sizeof(double) * 13 * C, off_mask = off_ints + sizeof(int) * 10 * C;
    HIPCHK(h, q.host.ensure(off_mask + N + 64, 0));
    double* const hd = q.host.as<double>();
    int* const hi = reinterpret_cast<int*>(q.host.as<unsigned char>() + off_ints);
    unsigned char* const hm = q.host.as<unsigned char>() + off_mask;
    EventPair timer;
    CHK(timer.start(h, o.profile != 0));
    CHK(launch_pnp_gather(h, obs_use != nullptr, cam_select != nullptr));
    if (samples) {                                               // positions are checked against the cameras' counts
        HIPCHK(h, hipMemcpyAsync(hi, q.cn.p, sizeof(int) * C, hipMemcpyDeviceToHost, h->stream));
        CHK(wait_stream(h));
        CHK(check_samples(h, samples, C, H, 3, [&](size_t c) { return hi[c]; }, pc.sc.need,     // (below: not selected or FEW_VIEWS)
                          "sfmba_resect_ransac", "camera", "observations"));
        HIPCHK(h, hipMemcpyAsync(q.samples.p, samples, sizeof(int) * 3 * C * H, hipMemcpyHostToDevice, h->stream));
    }
    CHK(launch_pnp_ransac(h, pc, samples != nullptr, hyp_inliers != nullptr, cam_select != nullptr));
    // the verdict and (refine = 1) the refinement: k_resect from the pose in x over the inlier mask, for the cameras that
    // succeeded -- both masks were written by k_pnp_finish
    ResectOptions ro{o.refine != 0 ? (int)o.max_iter : 0, (int)o.min_views, 1, o.xtol, o.min_depth, o.max_rms_px};
    // (over the compacted positions of k_pnp_gather: a masked call sums in the order of the problem without the masked)
    CHK(launch_resect(h, ro, q.mask.as<unsigned char>(), q.ok.as<unsigned char>(), q.cpos.as<int>()));
    CHK(timer.stop(h));
    HIPCHK(h, hipMemcpyAsync(hd, q.pose.p, sizeof(double) * 6 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hd + 6 * C, r.cam.p, sizeof(double) * 6 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hd + 12 * C, r.rms.p, sizeof(double) * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hi, q.ints.p, sizeof(int) * 6 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hi + 6 * C, r.ints.p, sizeof(int) * 4 * C, hipMemcpyDeviceToHost, h->stream));
    if (inlier_mask && N) HIPCHK(h, hipMemcpyAsync(hm, q.mask.p, N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, download(h, hyp_inliers, q.hyp.p, sizeof(int) * C * H));
    CHK(wait_stream(h));
    CHK(timer.read(h, kernel_us));
    if (inlier_mask)
        for (size_t k = 0; k < N; ++k) inlier_mask[caller_position(h, k)] = hm[k];
    const int* const ri = hi + 6 * C;                            // k_resect's status, views, iters, ok
    int64_t ok = 0;
    for (size_t c = 0; c < C; ++c) {
        const int* pi = hi + 6 * c;
        const bool refined = pi[0] == kPnpOk;                    // RANSAC succeeded: k_resect's verdict counts
        const int status = refined ? ri[c] : pi[0];
        if (cam_status) cam_status[c] = status;
        if (cam_views) cam_views[c] = pi[1];
        if (cam_inliers) cam_inliers[c] = pi[2];
        if (cam_best) cam_best[c] = pi[3];
        if (cam_best_sol) cam_best_sol[c] = pi[4];
        if (cam_success) cam_success[c] = (uint8_t)pi[5];
        if (cam_iters) cam_iters[c] = refined ? ri[2 * C + c] : 0;
        if (cam_rms_err) cam_rms_err[c] = refined ? hd[12 * C + c] : NAN;
        if (cam_hyp) memcpy(cam_hyp + 6 * c, hd + 6 * c, sizeof(double) * 6);
        if (cam_out) memcpy(cam_out + 6 * c, status == kResOk ? hd + 6 * C + 6 * c : x + 6 * c, sizeof(double) * 6);
        ok += status == kResOk ? 1 : 0;
    }
    if (n_ok) *n_ok = ok;
    return 0;
}

void sfmba_default_ransac_options(sfmba_ransac_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->threshold = 1.0; o->confidence = 0.99; o->seed = 0; o->max_iters = 1000; o->refit = 0; o->profile = 0;
}

int sfmba_fundamental_ransac(sfmba_handle* h, int64_t n_edges, const int64_t* edge_ptr, const double* pts1, const double* pts2,
                             const uint8_t* pair_use, const int32_t* samples, const sfmba_ransac_options* opt, double* F,
                             double* F_refit, uint8_t* inlier_mask, int32_t* edge_inliers, int32_t* edge_best,
                             uint8_t* edge_success, int32_t* edge_status, int32_t* hyp_inliers, int64_t* n_ok, double* kernel_us) {
    CHK(enter(h));
    TwoViewRansac c;
    CHK(twoview_ransac_begin(h, "sfmba_fundamental_ransac", reinterpret_cast<const void*>(k_fund_ransac), 8, n_edges, edge_ptr, pts1, pts2, pair_use, samples, opt,
                             hyp_inliers != nullptr, n_ok, kernel_us, &c));
    const TwoViewResults r{F, F_refit, {inlier_mask, nullptr}, edge_inliers, edge_best, edge_status, edge_success, nullptr, hyp_inliers,
                           n_ok, kernel_us};
    return twoview_ransac_end(h, c, c.o.threshold, 4, 1, kFundOk, r, [&](double* M, unsigned char* mask, int* ints, double score) {
        auto& t = h->twoview;
        CHK(launch_twoview_ransac(h, c, k_fund_ransac, score, t.slots.as<double>(), hyp_inliers ? t.hyp.as<int>() : nullptr));
        hipLaunchKernelGGL(k_fund_finish, dim3((unsigned)c.E), dim3(kTwoViewThreads), 0, h->stream, c.in, c.n_slices, score, c.o.confidence,
                           c.o.refit != 0 ? 1 : 0, (const double*)t.slots.as<double>(), FundOut{M, M + 9 * c.E, mask, ints});
        LAUNCHED(h);
        return 0;
    });
}

// The F call with k_homog_ransac / k_homog_finish and samples of four positions: twoview.F holds H and H_refit, twoview.mask
// both masks, twoview.ints five integers per edge.
int sfmba_homography_ransac(sfmba_handle* h, int64_t n_edges, const int64_t* edge_ptr, const double* pts1, const double* pts2,
                            const uint8_t* pair_use, const int32_t* samples, const sfmba_ransac_options* opt, double* Hm,
                            double* H_refit, uint8_t* inlier_mask, uint8_t* refit_mask, int32_t* edge_inliers,
                            int32_t* edge_refit_inliers, int32_t* edge_best, uint8_t* edge_success, int32_t* edge_status,
                            int32_t* hyp_inliers, int64_t* n_ok, double* kernel_us) {
    CHK(enter(h));
    TwoViewRansac c;
    CHK(twoview_ransac_begin(h, "sfmba_homography_ransac", reinterpret_cast<const void*>(k_homog_ransac), 4, n_edges, edge_ptr, pts1, pts2, pair_use, samples, opt,
                             hyp_inliers != nullptr, n_ok, kernel_us, &c));
    const TwoViewResults r{Hm, H_refit, {inlier_mask, refit_mask}, edge_inliers, edge_best, edge_status, edge_success, edge_refit_inliers,
                           hyp_inliers, n_ok, kernel_us};
    return twoview_ransac_end(h, c, c.o.threshold * c.o.threshold, 5, 2, kHomogOk, r, [&](double* M, unsigned char* mask, int* ints, double score) {
        auto& t = h->twoview;
        CHK(launch_twoview_ransac(h, c, k_homog_ransac, score, t.slots.as<double>(), hyp_inliers ? t.hyp.as<int>() : nullptr));
        hipLaunchKernelGGL(k_homog_finish, dim3((unsigned)c.E), dim3(kTwoViewThreads), 0, h->stream, c.in, c.n_slices, score, c.o.confidence,
                           c.o.refit != 0 ? 1 : 0, (const double*)t.slots.as<double>(), HomogOut{M, M + 9 * c.E, mask, mask + c.bt.Mu, ints});
        LAUNCHED(h);
        return 0;
    });
}

// The H call with k_sim_ransac / k_sim_finish over sets of 3-D pairs (six doubles a pair) and samples of three positions:
// twoview.F holds sim and sim_refit, 13 doubles each.
int sfmba_similarity_ransac(sfmba_handle* h, int64_t n_sets, const int64_t* set_ptr, const double* src, const double* dst,
                            const uint8_t* pair_use, const int32_t* samples, const sfmba_ransac_options* opt, double* sim,
                            double* sim_refit, uint8_t* inlier_mask, uint8_t* refit_mask, int32_t* set_inliers,
                            int32_t* set_refit_inliers, int32_t* set_best, uint8_t* set_success, int32_t* set_status,
                            int32_t* hyp_inliers, int64_t* n_ok, double* kernel_us) {
    CHK(enter(h));
    TwoViewRansac c;
    c.slot_doubles = kRansacHead + kSimPayload;
    c.dim = 3;
    c.model_doubles = kSimPayload;
    c.min_slice = kSimMinSlice;
    c.lds_pairs = kSimLdsPairs;
    c.item = "set";
    CHK(twoview_ransac_begin(h, "sfmba_similarity_ransac", reinterpret_cast<const void*>(k_sim_ransac), 3, n_sets, set_ptr, src, dst, pair_use, samples, opt,
                             hyp_inliers != nullptr, n_ok, kernel_us, &c));
    const TwoViewResults r{sim, sim_refit, {inlier_mask, refit_mask}, set_inliers, set_best, set_status, set_success, set_refit_inliers,
                           hyp_inliers, n_ok, kernel_us};
    return twoview_ransac_end(h, c, c.o.threshold * c.o.threshold, 5, 2, kSimOk, r, [&](double* M, unsigned char* mask, int* ints, double score) {
        auto& t = h->twoview;
        CHK(launch_twoview_ransac(h, c, k_sim_ransac, score, t.slots.as<double>(), hyp_inliers ? t.hyp.as<int>() : nullptr));
        hipLaunchKernelGGL(k_sim_finish, dim3((unsigned)c.E), dim3(kTwoViewThreads), 0, h->stream, c.in, c.n_slices, score, c.o.confidence,
                           c.o.refit != 0 ? 1 : 0, (const double*)t.slots.as<double>(),
                           SimOut{M, M + kSimPayload * c.E, mask, mask + c.bt.Mu, ints});
        LAUNCHED(h);
        return 0;
    });
}

// The F call with k_ess_ransac / k_ess_finish and samples of five positions: twoview.F holds E, twoview.ints five integers
// per edge (the fifth: the root of the best candidate), twoview.hyp the counts and, behind them, the root counts.
int sfmba_essential_ransac(sfmba_handle* h, int64_t n_edges, const int64_t* edge_ptr, const double* pts1, const double* pts2,
                           const uint8_t* pair_use, const int32_t* samples, const double* K, const sfmba_ransac_options* opt,
                           double* E_out, uint8_t* inlier_mask, int32_t* edge_inliers, int32_t* edge_best, int32_t* edge_best_root,
                           uint8_t* edge_success, int32_t* edge_status, int32_t* hyp_inliers, int32_t* hyp_roots, int64_t* n_ok,
                           double* kernel_us) {
    CHK(enter(h));
    if (!K) return fail(h, -1, "sfmba_essential_ransac: K is NULL");
    KMat Km;
    for (int k = 0; k < 9; ++k) Km.k[k] = K[k];
    const KMat Ki = inverse_k(Km);
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(K[k]) || !std::isfinite(Ki.k[k])) return fail(h, -1, "sfmba_essential_ransac: K is not finite or is singular");
    if (opt && opt->refit != 0) return fail(h, -1, "sfmba_essential_ransac: refit must be 0 (there is no refit of an essential matrix)");
    TwoViewRansac c;
    c.slot_doubles = kEssSlot;
    c.hyp_arrays = 2;
    const bool hyp = hyp_inliers != nullptr || hyp_roots != nullptr;
    CHK(twoview_ransac_begin(h, "sfmba_essential_ransac", reinterpret_cast<const void*>(k_ess_ransac), kEssS, n_edges, edge_ptr,
                             pts1, pts2, pair_use, samples, opt, hyp, n_ok, kernel_us, &c));
    const TwoViewResults r{E_out, nullptr, {inlier_mask, nullptr}, edge_inliers, edge_best, edge_status, edge_success, edge_best_root,
                           hyp_inliers, n_ok, kernel_us, hyp_roots};
    return twoview_ransac_end(h, c, c.o.threshold, 5, 1, kEssOk, r, [&](double* M, unsigned char* mask, int* ints, double score) {
        auto& t = h->twoview;
        int* const hy = hyp ? t.hyp.as<int>() : nullptr;
        CHK(launch_twoview_ransac(h, c, k_ess_ransac, score, Ki, t.slots.as<double>(), hy, hy ? hy + c.E * c.H : nullptr));
        hipLaunchKernelGGL(k_ess_finish, dim3((unsigned)c.E), dim3(kTwoViewThreads), 0, h->stream, c.in, c.n_slices, score, c.o.confidence,
                           (const double*)t.slots.as<double>(), EssOut{M, mask, ints});
        LAUNCHED(h);
        return 0;
    });
}

void sfmba_default_pose_options(sfmba_pose_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->min_depth = 0.0; o->profile = 0;
}

int sfmba_recover_pose(sfmba_handle* h, int64_t n_edges, const int64_t* edge_ptr, const double* pts1, const double* pts2,
                       const uint8_t* pair_use, const double* E_in, const double* K, const sfmba_pose_options* opt, double* R,
                       double* t_out, uint8_t* front_mask, double* X, double* angle_deg, int32_t* edge_front,
                       int32_t* edge_front_all, double* edge_sum_err, int32_t* edge_status, int64_t* n_ok, double* kernel_us) {
    CHK(enter(h));
    sfmba_pose_options o;
    if (opt) o = *opt; else sfmba_default_pose_options(&o);
    if (std::isnan(o.min_depth)) return fail(h, -1, "an option of sfmba_recover_pose is NaN");
    if (!K) return fail(h, -1, "sfmba_recover_pose: K is NULL");
    auto& t = h->twoview;
    TwoViewBatch bt;
    CHK(twoview_stage(h, "sfmba_recover_pose", n_edges, edge_ptr, pts1, pts2, pair_use, &bt));
    if (n_ok) *n_ok = 0;
    if (kernel_us) *kernel_us = 0.0;
    const size_t E = bt.E, Mu = bt.Mu;
    if (E == 0) return wait_stream(h);
    if (!E_in) return fail(h, -1, "sfmba_recover_pose: E is NULL");
    const size_t M1 = std::max<size_t>(Mu, 1);
    CHK(ensure_all(h, {{&t.E, sizeof(double) * 9 * E}, {&t.Rt, sizeof(double) * 12 * E}, {&t.err, sizeof(double) * E},
                       {&t.pose_ints, sizeof(int) * 6 * E}, {&t.mask, M1}, {&t.X, sizeof(double) * 3 * M1}, {&t.ang, sizeof(double) * M1}}));
    // E through the staging of the results (pinned; nothing of this call is in it yet)
    const size_t off_rt = 0, off_err = sizeof(double) * 12 * E, off_X = off_err + sizeof(double) * E,
                 off_ang = off_X + sizeof(double) * 3 * Mu, off_int = off_ang + sizeof(double) * Mu, off_mask = off_int + sizeof(int) * 6 * E;
    HIPCHK(h, t.out_host.ensure(off_mask + Mu, 0));
    unsigned char* const st = t.out_host.as<unsigned char>();
    memcpy(st, E_in, sizeof(double) * 9 * E);
    HIPCHK(h, hipMemcpyAsync(t.E.p, st, sizeof(double) * 9 * E, hipMemcpyHostToDevice, h->stream));
    KMat Km;
    for (int k = 0; k < 9; ++k) Km.k[k] = K[k];
    const PoseOut out{t.Rt.as<double>(), t.err.as<double>(), t.pose_ints.as<int>(), t.mask.as<unsigned char>(), t.X.as<double>(),
                      t.ang.as<double>()};
    EventPair timer;
    CHK(timer.start(h, o.profile != 0));
    hipLaunchKernelGGL(k_recover_pose, dim3((unsigned)E), dim3(kTwoViewThreads), 0, h->stream, (const double*)t.pairs.as<double>(),
                       (const int*)t.uptr.as<int>(), (const double*)t.E.as<double>(), Km, o.min_depth, out);
    LAUNCHED(h);
    CHK(timer.stop(h));
    HIPCHK(h, hipMemcpyAsync(st + off_rt, t.Rt.p, sizeof(double) * 12 * E, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(st + off_int, t.pose_ints.p, sizeof(int) * 6 * E, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, download(h, edge_sum_err, t.err.p, sizeof(double) * E));
    if (X && Mu) HIPCHK(h, hipMemcpyAsync(st + off_X, t.X.p, sizeof(double) * 3 * Mu, hipMemcpyDeviceToHost, h->stream));
    if (angle_deg && Mu) HIPCHK(h, hipMemcpyAsync(st + off_ang, t.ang.p, sizeof(double) * Mu, hipMemcpyDeviceToHost, h->stream));
    if (front_mask && Mu) HIPCHK(h, hipMemcpyAsync(st + off_mask, t.mask.p, Mu, hipMemcpyDeviceToHost, h->stream));
    CHK(wait_stream(h));
    CHK(timer.read(h, kernel_us));
    const double* rt = reinterpret_cast<const double*>(st + off_rt);
    const int* hi = reinterpret_cast<const int*>(st + off_int);
    const double nan3[3] = {NAN, NAN, NAN};
    const uint8_t zero = 0;
    twoview_scatter(h, bt, st + off_X, X, sizeof(double) * 3, nan3);
    twoview_scatter(h, bt, st + off_ang, angle_deg, sizeof(double), nan3);
    twoview_scatter(h, bt, st + off_mask, front_mask, 1, &zero);
    int64_t ok = 0;
    for (size_t e = 0; e < E; ++e) {
        if (R) memcpy(R + 9 * e, rt + 12 * e, sizeof(double) * 9);
        if (t_out) memcpy(t_out + 3 * e, rt + 12 * e + 9, sizeof(double) * 3);
        if (edge_front) edge_front[e] = hi[6 * e];
        if (edge_front_all) memcpy(edge_front_all + 4 * e, hi + 6 * e + 1, sizeof(int) * 4);
        if (edge_status) edge_status[e] = hi[6 * e + 5];
        ok += hi[6 * e + 5] == kPoseOk ? 1 : 0;
    }
    if (n_ok) *n_ok = ok;
    return 0;
}

void sfmba_default_filter_options(sfmba_filter_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_error_px = INFINITY; o->min_depth = -INFINITY; o->min_angle_deg = 0.0; o->min_views = 0;
}

int sfmba_reprojection_stats(sfmba_handle* h, const double* x, const sfmba_filter_options* opt, double* obs_err,
                             double* obs_depth, uint8_t* obs_keep, int32_t* pt_views, double* pt_max_err, double* pt_sum_err2,
                             double* pt_min_depth, double* pt_max_angle_deg, uint8_t* pt_keep, int32_t* cam_views,
                             double* cam_sum_err, double* cam_max_err, int32_t* cam_behind, sfmba_stats_summary* summary) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    sfmba_filter_options o;
    if (opt) o = *opt; else sfmba_default_filter_options(&o);
    if (std::isnan(o.max_error_px) || std::isnan(o.min_depth) || std::isnan(o.min_angle_deg))
        return fail(h, -1, "a threshold of the filter options is NaN");
    const StatsFilter flt = stats_filter(o);
    auto& s = h->stats;
    const size_t N = (size_t)h->N, P = (size_t)h->P, C = (size_t)h->C;
    const bool want_cam = cam_views || cam_sum_err || cam_max_err || cam_behind;
    int pt_blocks = 1;
    CHK(stats_allocate(h, &pt_blocks));
    CHK(stats_prepare(h, x));
    if (want_cam) CHK(stats_cam_perm(h));
    CHK(launch_obs_stats(h, flt));
    CHK(launch_point_stats(h, flt, pt_blocks));
    if (summary) CHK(launch_stats_summary(h, pt_blocks));
    if (want_cam) CHK(launch_cam_stats(h));
    // downloads: only what was asked for; the per-observation arrays through pinned staging, then into the caller's order
    const bool want_ed = obs_err || obs_depth;
    if (want_ed || obs_keep) HIPCHK(h, s.host.ensure(17 * N + 64, 0));
    double* const st_ed = s.host.as<double>();
    unsigned char* const st_keep = s.host.as<unsigned char>() + 16 * N;
    if (want_ed) HIPCHK(h, download(h, st_ed, s.ed.p, 16 * N));
    if (obs_keep) HIPCHK(h, download(h, st_keep, s.keep_final.p, N));
    const double* pd = s.pt_d.as<double>();
    HIPCHK(h, download(h, pt_views, s.pt_views.p, sizeof(int32_t) * P));
    HIPCHK(h, download(h, pt_max_err, pd, sizeof(double) * P));
    HIPCHK(h, download(h, pt_sum_err2, pd + P, sizeof(double) * P));
    HIPCHK(h, download(h, pt_min_depth, pd + 2 * P, sizeof(double) * P));
    HIPCHK(h, download(h, pt_max_angle_deg, pd + 3 * P, sizeof(double) * P));
    HIPCHK(h, download(h, pt_keep, s.pt_keep.p, P));
    HIPCHK(h, download(h, cam_views, s.cam_i.p, sizeof(int32_t) * C));
    HIPCHK(h, download(h, cam_behind, s.cam_i.as<int>() + C, sizeof(int32_t) * C));
    HIPCHK(h, download(h, cam_sum_err, s.cam_d.p, sizeof(double) * C));
    HIPCHK(h, download(h, cam_max_err, s.cam_d.as<double>() + C, sizeof(double) * C));
    double sums[kStatsPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (summary) HIPCHK(h, download(h, sums, s.sum.p, sizeof sums));
    CHK(wait_stream(h));
    if (want_ed || obs_keep) {
        for (size_t k = 0; k < N; ++k) {
            const size_t d = caller_position(h, k);
            if (obs_err) obs_err[d] = st_ed[2 * k];
            if (obs_depth) obs_depth[d] = st_ed[2 * k + 1];
            if (obs_keep) obs_keep[d] = st_keep[k];
        }
    }
    if (summary) {
        summary->n_obs = h->N;
        summary->n_points_kept = (int64_t)sums[0]; summary->n_obs_kept = (int64_t)sums[1]; summary->n_behind = (int64_t)sums[2];
        summary->sum_err = sums[3]; summary->sum_err2 = sums[4]; summary->max_err = sums[5];
    }
    return 0;
}

// sfmba_time_kernel, which = 13 / 14: the per-observation sweep / the per-point reduction at x, default thresholds
int sfmba::stats_time_kernel(sfmba_handle* h, const double* x, int32_t which, int32_t reps, double* avg_us) {
    sfmba_filter_options o;
    sfmba_default_filter_options(&o);
    const StatsFilter flt = stats_filter(o);
    int pt_blocks = 1;
    CHK(stats_allocate(h, &pt_blocks));
    CHK(stats_prepare(h, x));
    CHK(launch_obs_stats(h, flt));                      // (the reduction's input)
    return time_reps(h, reps, avg_us, [&] { return which == 13 ? launch_obs_stats(h, flt) : launch_point_stats(h, flt, pt_blocks); });
}

// sfmba_time_kernel, which = 15: k_triangulate at x over every point and observation, default options
int sfmba::tri_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us) {
    sfmba_triangulate_options o;
    sfmba_default_triangulate_options(&o);
    const TriOptions opt = tri_options(o);
    int grid = 1;
    CHK(tri_allocate(h, &grid));
    CHK(stats_prepare(h, x));
    return time_reps(h, reps, avg_us, [&] { return launch_triangulate(h, opt, nullptr, nullptr, grid); });
}

// sfmba_time_kernel, which = 16: k_resect at x over every camera and observation, default options
int sfmba::resect_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us) {
    sfmba_resect_options o;
    sfmba_default_resect_options(&o);
    const ResectOptions opt = resect_options(o);
    CHK(resect_check_single(h));
    CHK(resect_allocate(h));
    CHK(upload_x(h, x, h->stats.x.as<double>()));
    CHK(stats_cam_perm(h));
    return time_reps(h, reps, avg_us, [&] { return launch_resect(h, opt, nullptr, nullptr); });
}

// sfmba_time_kernel, which = 17: k_pnp_ransac + k_pnp_finish at x over every camera and observation, default options
int sfmba::pnp_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us) {
    sfmba_pnp_ransac_options o;
    sfmba_default_pnp_ransac_options(&o);
    CHK(resect_check_single(h));
    if (h->C == 0) { *avg_us = 0.0; return 0; }
    const PnpCall pc = pnp_call(h, o);
    CHK(pnp_allocate(h, pc, false, false));
    CHK(upload_x(h, x, h->stats.x.as<double>()));
    CHK(stats_cam_perm(h));
    CHK(launch_pnp_gather(h, false, false));
    return time_reps(h, reps, avg_us, [&] { return launch_pnp_ransac(h, pc, false, false, false); });
}

// sfmba_time_kernel, which = 19: k_tri_ransac + k_triangulate over its mask at x, every point and observation, default options
int sfmba::tri_ransac_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us) {
    sfmba_tri_ransac_options o;
    sfmba_default_tri_ransac_options(&o);
    const TriRansacOptions ro = tri_ransac_options(o);
    const TriOptions to{(int)o.max_iter, (int)o.min_views, o.xtol, o.min_angle_deg, o.min_depth, o.max_error_px};
    int grid = 1, tri_grid = 1;
    CHK(tri_ransac_allocate(h, ro.H, false, &grid, &tri_grid));
    CHK(stats_prepare(h, x));
    CHK(tri_ransac_clear(h, ro.H, false));
    return time_reps(h, reps, avg_us, [&] { return launch_tri_ransac(h, ro, to, false, false, false, grid, tri_grid); });
}
