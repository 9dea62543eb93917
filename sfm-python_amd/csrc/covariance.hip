// covariance.hip -- host code of sfmba_covariance (kernels: cov_kernels.hpp; device-free checks: cov_inputs.hpp; DESIGN.md
// section 28): camera and point covariance blocks of a bundle-adjustment solution.  Like the other consumers it works on
// buffers of its own (the statistics call's x and camera table among them) and touches none of the solver's.
#include "handle.hpp"
#include "cov_kernels.hpp"
#include "cov_inputs.hpp"

namespace {

struct CovPlan {
    sfmba_covariance_options opt;
    CovCounts counts;
    CovGauge gauge;
    bool points = false;             // a point output is asked for: the point sweep runs
    int pt_blocks = 1, cam_blocks = 1;
};

int cov_check_options(sfmba_handle* h, const sfmba_covariance_options& o) {
    if (std::isnan(o.sigma2) || std::isnan(o.rank_tol) || std::isnan(o.point_tol))
        return fail(h, -1, "an option of sfmba_covariance is NaN");
    if (o.sigma2 < 0.0 || o.rank_tol < 0.0 || o.point_tol < 0.0 || o.kind < 0 || o.gauge < 0)
        return fail(h, -1, "an option of sfmba_covariance is negative");
    if (o.kind > 1 || o.gauge > 1) return fail(h, -1, "sfmba_covariance: kind and gauge are 0 or 1");
    return 0;
}

// the checks that need no device, the held mask (-> cov.held, and held_out), the buffers, x and its camera table
int cov_prepare(sfmba_handle* h, const double* x, const int32_t* hold, int32_t n_hold, CovPlan* pl, uint8_t* held_out) {
    auto& cv = h->cov;
    const sfmba_covariance_options& o = pl->opt;
    CHK(cov_check_options(h, o));
    if (multi_rank(h) || h->N_total != h->N)
        return fail(h, -1, "sfmba_covariance needs the whole problem: this handle holds a shard, and a shard's covariance is not the problem's");
    if (h->f32) return fail(h, -1, "sfmba_covariance needs fp64 storage (sfmba_set_precision(h, 64))");
    const std::string bad_hold = cov_check_hold(hold, n_hold, h->C);
    if (!bad_hold.empty()) return fail(h, -1, "sfmba_covariance: %s", bad_hold.c_str());
    if (o.kind == 0 && !(h->forms.dense && h->n_blk > 0))
        return fail(h, -1, "the marginal covariance (kind = 0) factorises the reduced camera matrix in LDS: it needs "
                           "6 * n_cameras <= %d and the pair lists of the dense path; kind = 1 has no such limit", kCovMaxN);
    const size_t C = (size_t)h->C, P = (size_t)h->P, n6 = 6 * C;
    const int* ci = h->stage.ci.as<int>();
    std::vector<int> views(C, 0);
    for (int64_t k = 0; k < h->N; ++k) ++views[(size_t)ci[k]];
    HIPCHK(h, cv.host.ensure(n6 + 64 + sizeof(double) * (kCovScal + 2 * C) + sizeof(int) * kCovInts, 0));
    unsigned char* const mask = cv.host.as<unsigned char>();
    pl->counts = cov_held_mask(x, h->C, h->P, h->N, h->fixed_cur.data(), views.data(), h->stage.ptr.as<int>(), hold, n_hold,
                               o.gauge != 0, mask, &pl->gauge);
    if (held_out) memcpy(held_out, mask, n6);
    pl->pt_blocks = (int)std::max<size_t>(1, (P + kCovThreads - 1) / kCovThreads);
    pl->cam_blocks = (int)std::max<size_t>(1, (C + kCovThreads - 1) / kCovThreads);
    const bool marginal = o.kind == 0;
    CHK(ensure_all(h, {
        {&h->stats.x, sizeof(double) * (size_t)h->n}, {&h->stats.tab, sizeof(double) * cam_table_doubles((int)C)},
        {&cv.rec, sizeof(double) * (size_t)kRecStride * P}, {&cv.Vinv, sizeof(double) * (size_t)kVinvStride * P},
        {&cv.U, sizeof(double) * 21 * C}, {&cv.pt_cost, sizeof(double) * P}, {&cv.pt_status, sizeof(int) * P},
        {&cv.held, n6}, {&cv.scal, sizeof(double) * kCovScal}, {&cv.ints, sizeof(int) * kCovInts},
        {&cv.Sblk, marginal ? sizeof(double) * 36 * (size_t)h->n_blk : 0}, {&cv.full, marginal ? sizeof(double) * n6 * n6 : 0},
        {&cv.cam_cov, sizeof(double) * 36 * C}, {&cv.cam_sigma, sizeof(double) * 2 * C}, {&cv.cam_piv, sizeof(double) * 2 * C},
        {&cv.pt_cov, sizeof(double) * 9 * P}, {&cv.pt_sigma, sizeof(double) * P}}));
    CHK(upload_x(h, x, h->stats.x.as<double>()));
    HIPCHK(h, hipMemcpyAsync(cv.held.p, mask, n6, hipMemcpyHostToDevice, h->stream));
    return 0;
}

// camera table, V_p^-1 and the point records, the sums and sigma^2, U_c
int cov_launch_linearize(sfmba_handle* h, const CovPlan& pl) {
    auto& cv = h->cov;
    auto& s = h->stats;
    CHK(launch_k_cam_table(h, s.x.as<double>(), s.tab.as<double>()));
    const double* pts = s.x.as<double>() + 6 * h->C;
    const CovLinOut out{cv.rec.as<double>(), cv.Vinv.as<double>(), cv.pt_cost.as<double>(), cv.pt_status.as<int>(), kRecStride,
                        kVinvStride};
    hipLaunchKernelGGL(k_cov_linearize, dim3(pl.pt_blocks), dim3(kCovThreads), 0, h->stream, (const int*)h->pt_ptr.as<int>(),
                       (const int*)h->cam_idx.as<int>(), (const double*)h->uv.as<double>(), (const double*)s.tab.as<double>(), pts,
                       (int)h->P, h->K, pl.opt.point_tol, out);
    LAUNCHED(h);
    hipLaunchKernelGGL(k_cov_reduce, dim3(1), dim3(kCovThreads), 0, h->stream, (const double*)cv.pt_cost.as<double>(),
                       (const int*)cv.pt_status.as<int>(), (int)h->P, pl.opt.sigma2, (double)pl.counts.dof, cv.scal.as<double>(),
                       cv.ints.as<int>());
    LAUNCHED(h);
    CHK(stats_cam_perm(h));
    hipLaunchKernelGGL(k_cov_cam_u, dim3((unsigned)h->C), dim3(kCamThreads), 0, h->stream, (const int*)s.cam_ptr.as<int>(),
                       (const int*)s.perm.as<int>(), (const int*)h->pt_idx.as<int>(), (const double*)s.tab.as<double>(), pts, h->K,
                       cv.U.as<double>());
    LAUNCHED(h);
    return 0;
}

// kind = 0: the blocks of W V^-1 W^T over the pair lists, then S factorised and inverted in LDS -> cov.full
int cov_launch_factor(sfmba_handle* h, const CovPlan& pl) {
    auto& cv = h->cov;
    CHK(launch_k_schur_blocks(h, h->stats.tab.as<double>(), cv.rec.as<double>(), cv.Vinv.as<double>(), cv.Sblk.as<double>()));
    const int n = 6 * (int)h->C;
    const size_t lds = sizeof(double) * ((size_t)n * (size_t)(n | 1) + 3 * kCovMaxN);
    CHK(set_lds(h, k_cov_factor, lds));
    hipLaunchKernelGGL(k_cov_factor, dim3(1), dim3(kCovFactorThreads), lds, h->stream, (const double*)cv.Sblk.as<double>(),
                       (const double*)cv.U.as<double>(), (const unsigned char*)cv.held.as<unsigned char>(), (int)h->C,
                       pl.opt.rank_tol, cv.scal.as<double>(), cv.ints.as<int>(), cv.full.as<double>());
    LAUNCHED(h);
    return 0;
}

int cov_launch_cams(sfmba_handle* h, const CovPlan& pl) {
    auto& cv = h->cov;
    hipLaunchKernelGGL(k_cov_cams, dim3(pl.cam_blocks), dim3(kCovThreads), 0, h->stream, (const double*)cv.full.as<double>(),
                       (const double*)cv.U.as<double>(), (const unsigned char*)cv.held.as<unsigned char>(), (int)h->C,
                       (int)pl.opt.kind, pl.opt.rank_tol, (const double*)cv.scal.as<double>(), cv.cam_cov.as<double>(),
                       cv.cam_sigma.as<double>(), cv.cam_piv.as<double>());
    LAUNCHED(h);
    return 0;
}

int cov_launch_points(sfmba_handle* h, const CovPlan& pl) {
    auto& cv = h->cov;
    auto& s = h->stats;
    const CovPointOut out{cv.pt_cov.as<double>(), cv.pt_sigma.as<double>()};
    const bool lds_full = pl.opt.kind == 0 && h->dbg.cov_lds != 0;         // (measured: DESIGN.md section 28)
    const size_t lds = lds_full ? sizeof(double) * 36 * (size_t)h->C * (size_t)h->C : 0;
    auto kern = lds_full ? k_cov_points<true> : k_cov_points<false>;
    CHK(set_lds(h, kern, lds));
    hipLaunchKernelGGL(kern, dim3(pl.pt_blocks), dim3(kCovThreads), lds, h->stream, (const int*)h->pt_ptr.as<int>(),
                       (const int*)h->cam_idx.as<int>(), (const double*)s.tab.as<double>(),
                       (const double*)(s.x.as<double>() + 6 * h->C), (const double*)cv.Vinv.as<double>(), kVinvStride,
                       (const int*)cv.pt_status.as<int>(), (const double*)cv.full.as<double>(), 6 * (int)h->C,
                       (const double*)cv.scal.as<double>(), (int)pl.opt.kind, (int)h->P, h->K, out);
    LAUNCHED(h);
    return 0;
}

// the small read-back: scal | ints (| the per-camera pivots of kind = 1) through the pinned staging, stream waited for
int cov_read_back(sfmba_handle* h, bool with_piv, double** scal, int** ints, double** piv) {
    auto& cv = h->cov;
    const size_t C = (size_t)h->C, off = (6 * C + 63) / 64 * 64;
    double* const sc = reinterpret_cast<double*>(cv.host.as<unsigned char>() + off);
    double* const pv = sc + kCovScal;
    int* const in = reinterpret_cast<int*>(pv + 2 * C);
    HIPCHK(h, download(h, sc, cv.scal.p, sizeof(double) * kCovScal));
    HIPCHK(h, download(h, in, cv.ints.p, sizeof(int) * kCovInts));
    if (with_piv) HIPCHK(h, download(h, pv, cv.cam_piv.p, sizeof(double) * 2 * C));
    CHK(wait_stream(h));
    *scal = sc; *ints = in; *piv = pv;
    return 0;
}

void fill_nan(double* p, size_t n) {
    if (p) std::fill(p, p + n, (double)NAN);
}

}  // namespace

void sfmba_default_covariance_options(sfmba_covariance_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->kind = 0; o->gauge = 1; o->sigma2 = 0.0; o->rank_tol = 1e-10; o->point_tol = 1e-12; o->profile = 0;
}

int sfmba_covariance(sfmba_handle* h, const double* x, const int32_t* hold, int32_t n_hold, const sfmba_covariance_options* opt,
                     double* cam_cov, double* cam_full, double* cam_sigma, double* pt_cov, double* pt_sigma, int32_t* pt_status,
                     uint8_t* held_out, sfmba_covariance_info* info) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    CovPlan pl;
    if (opt) pl.opt = *opt; else sfmba_default_covariance_options(&pl.opt);
    pl.points = pt_cov != nullptr || pt_sigma != nullptr;
    CHK(cov_prepare(h, x, hold, n_hold, &pl, held_out));
    auto& cv = h->cov;
    const size_t C = (size_t)h->C, P = (size_t)h->P, n6 = 6 * C;
    const bool marginal = pl.opt.kind == 0;
    sfmba_covariance_info out;
    memset(&out, 0, sizeof out);
    out.g0 = pl.gauge.g0; out.g1 = pl.gauge.g1; out.g1_axis = pl.gauge.axis;
    out.n_free = pl.counts.n_free; out.n_held = pl.counts.n_held; out.dof = pl.counts.dof;
    out.bad_param = -1; out.bad_point = -1; out.min_pivot_rel = NAN;
    EventPair ev;
    CHK(ev.start(h, pl.opt.profile != 0));
    double *scal = nullptr, *piv = nullptr;
    int* ints = nullptr;
    CHK(cov_launch_linearize(h, pl));
    CHK(cov_read_back(h, false, &scal, &ints, &piv));
    out.cost = 0.5 * scal[0]; out.sigma2 = scal[1];
    out.n_bad_points = ints[0]; out.bad_point = ints[1];
    if (ints[0] > 0) out.status = 2;
    if (out.status == 0) {
        if (marginal) CHK(cov_launch_factor(h, pl)); else CHK(cov_launch_cams(h, pl));
        CHK(cov_read_back(h, !marginal, &scal, &ints, &piv));
        if (marginal) {
            out.min_pivot_rel = scal[2]; out.bad_param = ints[2];
        } else {
            double m = INFINITY;
            for (size_t c = 0; c < C; ++c) {
                m = std::fmin(m, piv[2 * c]);
                if (piv[2 * c + 1] >= 0.0 && out.bad_param < 0) out.bad_param = (int32_t)piv[2 * c + 1];
            }
            out.min_pivot_rel = m;
        }
        if (out.bad_param >= 0) out.status = 1;
    }
    if (out.status == 0) {
        if (marginal) CHK(cov_launch_cams(h, pl));
        if (pl.points) CHK(cov_launch_points(h, pl));
        CHK(ev.stop(h));
        HIPCHK(h, download(h, cam_cov, cv.cam_cov.p, sizeof(double) * 36 * C));
        HIPCHK(h, download(h, cam_sigma, cv.cam_sigma.p, sizeof(double) * 2 * C));
        if (marginal) HIPCHK(h, download(h, cam_full, cv.full.p, sizeof(double) * n6 * n6));
        HIPCHK(h, download(h, pt_cov, cv.pt_cov.p, sizeof(double) * 9 * P));
        HIPCHK(h, download(h, pt_sigma, cv.pt_sigma.p, sizeof(double) * P));
    } else {
        CHK(ev.stop(h));
    }
    HIPCHK(h, download(h, pt_status, cv.pt_status.p, sizeof(int32_t) * P));
    CHK(wait_stream(h));
    CHK(ev.read(h, &out.kernel_us));
    if (out.status != 0) {                   // rank failure: every matrix NaN; pt_status and held_out are valid
        fill_nan(cam_cov, 36 * C); fill_nan(cam_sigma, 2 * C); fill_nan(cam_full, n6 * n6);
        fill_nan(pt_cov, 9 * P); fill_nan(pt_sigma, P);
    } else if (!marginal && cam_full) {      // kind = 1 has no cross blocks: the block-diagonal matrix
        std::fill(cam_full, cam_full + n6 * n6, 0.0);
        std::vector<double> blk(36 * C);
        HIPCHK(h, hipMemcpy(blk.data(), cv.cam_cov.p, sizeof(double) * 36 * C, hipMemcpyDeviceToHost));
        for (size_t c = 0; c < C; ++c)
            for (int u = 0; u < 6; ++u)
                for (int v = 0; v < 6; ++v) cam_full[(6 * c + u) * n6 + 6 * c + v] = blk[36 * c + 6 * u + v];
    }
    if (info) *info = out;
    return 0;
}

// sfmba_time_kernel, which = 18: the kernel group of one call with the default options (kind = 0 where the problem is on
// the dense form, else kind = 1), point sweep included, without the read-backs between its stages
int sfmba::cov_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us) {
    CovPlan pl;
    sfmba_default_covariance_options(&pl.opt);
    if (!(h->forms.dense && h->n_blk > 0)) pl.opt.kind = 1;
    pl.points = true;
    CHK(cov_prepare(h, x, nullptr, 0, &pl, nullptr));
    return time_reps(h, reps, avg_us, [&]() -> int {
        CHK(cov_launch_linearize(h, pl));
        if (pl.opt.kind == 0) CHK(cov_launch_factor(h, pl));
        CHK(cov_launch_cams(h, pl));
        return cov_launch_points(h, pl);
    });
}
