// plan.hip -- host code of view planning and problem assembly (kernels: plan_kernels.hpp, argument checks: plan_inputs.hpp)
#include "handle.hpp"
#include "plan_inputs.hpp"
#include "plan_kernels.hpp"

namespace {
// the three launches of one scan over n entries (the middle one lives in tracks.hip)
template <class Src>
int plan_scan(sfmba_handle* h, const Src& src, size_t n, int slot) {
    auto& p = h->plan;
    const unsigned nb = (unsigned)std::max<size_t>((n + kTrackScanItems - 1) / kTrackScanItems, 1);
    hipLaunchKernelGGL(k_track_scan_reduce<Src>, dim3(nb), dim3(kTrackBlock), 0, h->stream, src, p.sums.as<long long>());
    LAUNCHED(h);
    CHK(launch_k_track_scan_sums(h, p.sums.as<long long>(), nb, p.tot.as<long long>(), slot, kTrackBlock, kTrackScanItems));
    hipLaunchKernelGGL(k_track_scan_apply<Src>, dim3(nb), dim3(kTrackBlock), 0, h->stream, src, (const long long*)p.sums.as<long long>());
    LAUNCHED(h);
    return 0;
}

// the checks every call shares, and the two masks on the device
int plan_begin(sfmba_handle* h, const char* fn, int64_t n_images, const uint8_t* cam_mask, int64_t n_tracks, const uint8_t* trk_mask) {
    auto& t = h->tracks;
    if (!t.built) return fail(h, -1, "%s: no tracks built (call sfmba_build_tracks first)", fn);
    std::string why;
    if (plan_check_masks(fn, n_images, cam_mask, n_tracks, trk_mask, t.n_images, t.n_tracks, &why) != 0)
        return fail(h, -1, "%s", why.c_str());
    return 0;
}
int plan_upload_masks(sfmba_handle* h, const uint8_t* cam_mask, const uint8_t* trk_mask) {
    auto& t = h->tracks;
    auto& p = h->plan;
    const size_t nb = std::max<size_t>(((size_t)std::max(t.n_tracks, t.n_images) + kTrackScanItems - 1) / kTrackScanItems, 1);
    CHK(ensure_all(h, {{&p.cam_mask, (size_t)t.n_images}, {&p.trk_mask, (size_t)t.n_tracks},
                       {&p.sums, sizeof(long long) * 2 * nb}, {&p.tot, sizeof(long long) * kPlanTotSlots}}));
    HIPCHK(h, hipMemcpyAsync(p.cam_mask.p, cam_mask, (size_t)t.n_images, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(p.trk_mask.p, trk_mask, (size_t)t.n_tracks, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                  // (both sources are pageable and the caller's)
    return 0;
}
inline unsigned plan_grid(int64_t n) { return (unsigned)((n + kPlanBlock - 1) / kPlanBlock); }
}  // namespace

void sfmba_default_plan_options(sfmba_plan_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->min_views = 2; o->profile = 0;
}

int sfmba_set_keypoints(sfmba_handle* h, int64_t n_images, const int64_t* img_ptr, const double* pts) {
    CHK(enter(h));
    auto& p = h->plan;
    std::string why;
    int64_t N = 0;
    if (plan_check_keypoints(n_images, img_ptr, pts, &N, &why) != 0) return fail(h, -1, "%s", why.c_str());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    p.have_kp = false;
    CHK(ensure_all(h, {{&p.kp, sizeof(double) * 2 * (size_t)N}}));
    if (N) {
        HIPCHK(h, hipMemcpyAsync(p.kp.p, pts, sizeof(double) * 2 * (size_t)N, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));              // (the source is pageable and the caller's)
    }
    p.kp_img_ptr.assign(img_ptr, img_ptr + n_images + 1);
    p.have_kp = true;
    return 0;
}

int sfmba_plan_views(sfmba_handle* h, int64_t n_images, const uint8_t* cam_reg, int64_t n_tracks, const uint8_t* trk_known,
                     const sfmba_plan_options* opt, int32_t* trk_reg_views, int32_t* img_tracks, int32_t* img_known,
                     int32_t* img_gain, int64_t* totals, double* kernel_us) {
    CHK(enter(h));
    sfmba_plan_options o;
    if (opt) o = *opt; else sfmba_default_plan_options(&o);
    CHK(plan_begin(h, "sfmba_plan_views", n_images, cam_reg, n_tracks, trk_known));
    auto& t = h->tracks;
    auto& p = h->plan;
    if (kernel_us) *kernel_us = 0.0;
    if (n_tracks == 0) {                                         // no track: nothing on the device to sweep
        for (int32_t* a : {img_tracks, img_known, img_gain})
            if (a) std::fill(a, a + n_images, (int32_t)0);
        if (totals) {
            totals[0] = totals[1] = totals[2] = 0;
            for (int64_t i = 0; i < n_images; ++i) totals[0] += cam_reg[i] != 0;
        }
        return 0;
    }
    const size_t C = (size_t)n_images, P = (size_t)n_tracks;
    CHK(ensure_all(h, {{&p.trk_views, sizeof(int) * P}, {&p.img_out, sizeof(int) * 3 * C}}));
    CHK(plan_upload_masks(h, cam_reg, trk_known));
    EventPair timer;
    CHK(timer.start(h, o.profile != 0));
    long long* const tot = p.tot.as<long long>();
    int* const img_out = p.img_out.as<int>();
    HIPCHK(h, hipMemsetAsync(tot, 0, sizeof(long long) * kPlanTotSlots, h->stream));
    hipLaunchKernelGGL(k_plan_track_views, dim3(plan_grid(n_tracks)), dim3(kPlanBlock), 0, h->stream, (int)n_tracks,
                       (const long long*)t.track_ptr.as<long long>(), (const int*)t.track_image.as<int>(),
                       (const unsigned char*)p.cam_mask.as<unsigned char>(), (const unsigned char*)p.trk_mask.as<unsigned char>(),
                       p.trk_views.as<int>(), tot);
    LAUNCHED(h);
    hipLaunchKernelGGL(k_plan_image_views, dim3((unsigned)n_images), dim3(kPlanBlock), 0, h->stream, (const int*)t.img_ptr.as<int>(),
                       (const int*)t.feat_track.as<int>(), (const unsigned char*)p.cam_mask.as<unsigned char>(),
                       (const unsigned char*)p.trk_mask.as<unsigned char>(), (const int*)p.trk_views.as<int>(), img_out,
                       img_out + C, img_out + 2 * C, tot);
    LAUNCHED(h);
    CHK(timer.stop(h));
    long long sums[kPlanTotSlots];
    HIPCHK(h, download(h, sums, tot, sizeof sums));
    HIPCHK(h, download(h, trk_reg_views, p.trk_views.p, sizeof(int) * P));
    HIPCHK(h, download(h, img_tracks, img_out, sizeof(int) * C));
    HIPCHK(h, download(h, img_known, img_out + C, sizeof(int) * C));
    HIPCHK(h, download(h, img_gain, img_out + 2 * C, sizeof(int) * C));
    CHK(wait_stream(h));
    CHK(timer.read(h, kernel_us));
    if (totals) { totals[0] = sums[kPlanTotReg]; totals[1] = sums[kPlanTotKnown]; totals[2] = sums[kPlanTotReady]; }
    return 0;
}

int sfmba_assemble_problem(sfmba_handle* h, int64_t n_images, const uint8_t* cam_use, int64_t n_tracks, const uint8_t* trk_use,
                           const sfmba_plan_options* opt, int64_t* counts, double* kernel_us) {
    CHK(enter(h));
    sfmba_plan_options o;
    if (opt) o = *opt; else sfmba_default_plan_options(&o);
    CHK(plan_begin(h, "sfmba_assemble_problem", n_images, cam_use, n_tracks, trk_use));
    std::string why;
    if (plan_check_min_views("sfmba_assemble_problem", o.min_views, &why) != 0) return fail(h, -1, "%s", why.c_str());
    auto& t = h->tracks;
    auto& p = h->plan;
    p.assembled = false;
    if (kernel_us) *kernel_us = 0.0;
    std::fill(p.counts, p.counts + 3, (int64_t)0);
    if (n_tracks > 0) {
        const size_t C = (size_t)n_images, P = (size_t)n_tracks, T = (size_t)t.T;
        CHK(ensure_all(h, {{&p.kept, sizeof(int) * P}, {&p.pt_id, sizeof(int) * P}, {&p.obs_off, sizeof(long long) * P},
                           {&p.pt_of, sizeof(int) * P}, {&p.present, sizeof(int) * C}, {&p.cam_id, sizeof(int) * C},
                           {&p.cam_of, sizeof(int) * C}, {&p.ci, sizeof(long long) * T}, {&p.pi, sizeof(long long) * T},
                           {&p.of, sizeof(int) * T}}));
        CHK(plan_upload_masks(h, cam_use, trk_use));
        EventPair timer;
        CHK(timer.start(h, o.profile != 0));
        long long* const tot = p.tot.as<long long>();
        const long long* const track_ptr = t.track_ptr.as<long long>();
        const int* const track_image = t.track_image.as<int>();
        const unsigned char* const cam = p.cam_mask.as<unsigned char>();
        HIPCHK(h, hipMemsetAsync(tot, 0, sizeof(long long) * kPlanTotSlots, h->stream));
        hipLaunchKernelGGL(k_plan_used, dim3(plan_grid(n_tracks)), dim3(kPlanBlock), 0, h->stream, (int)n_tracks, track_ptr,
                           track_image, cam, (const unsigned char*)p.trk_mask.as<unsigned char>(), o.min_views, p.kept.as<int>());
        LAUNCHED(h);
        CHK(plan_scan(h, PlanPointSrc{p.kept.as<int>(), (int)n_tracks, p.pt_id.as<int>(), p.obs_off.as<long long>(), p.pt_of.as<int>()},
                      P, kPlanTotPoints));
        hipLaunchKernelGGL(k_plan_present, dim3((unsigned)n_images), dim3(kPlanBlock), 0, h->stream, (const int*)t.img_ptr.as<int>(),
                           (const int*)t.feat_track.as<int>(), cam, (const int*)p.kept.as<int>(), p.present.as<int>());
        LAUNCHED(h);
        CHK(plan_scan(h, PlanCamSrc{p.present.as<int>(), (int)n_images, p.cam_id.as<int>(), p.cam_of.as<int>()}, C, kPlanTotCams));
        hipLaunchKernelGGL(k_plan_write, dim3(plan_grid(n_tracks)), dim3(kPlanBlock), 0, h->stream, (int)n_tracks, track_ptr,
                           (const int*)t.track_feat.as<int>(), track_image, cam, (const int*)p.kept.as<int>(),
                           (const int*)p.pt_id.as<int>(), (const long long*)p.obs_off.as<long long>(), (const int*)p.cam_id.as<int>(),
                           p.ci.as<long long>(), p.pi.as<long long>(), p.of.as<int>());
        LAUNCHED(h);
        CHK(timer.stop(h));
        long long sums[kPlanTotSlots];
        HIPCHK(h, download(h, sums, tot, sizeof sums));
        CHK(wait_stream(h));
        CHK(timer.read(h, kernel_us));
        p.counts[0] = sums[kPlanTotCams]; p.counts[1] = sums[kPlanTotPoints]; p.counts[2] = sums[kPlanTotObs];
    }
    p.assembled = true;
    if (counts) std::copy(p.counts, p.counts + 3, counts);
    return 0;
}

int sfmba_get_assembled(sfmba_handle* h, int32_t* cam_of, int32_t* pt_of, int64_t* camera_indices, int64_t* point_indices,
                        int32_t* obs_feat, double* points_2d) {
    CHK(enter(h));
    auto& t = h->tracks;
    auto& p = h->plan;
    if (!t.built) return fail(h, -1, "sfmba_get_assembled: no tracks built (call sfmba_build_tracks first)");
    if (!p.assembled) return fail(h, -1, "sfmba_get_assembled: no problem assembled over these tracks (call sfmba_assemble_problem first)");
    if (points_2d) {
        if (!p.have_kp) return fail(h, -1, "sfmba_get_assembled: points_2d needs the keypoints (call sfmba_set_keypoints first)");
        std::string why;
        if (plan_check_same_images("sfmba_get_assembled", (int64_t)p.kp_img_ptr.size() - 1, p.kp_img_ptr.data(), t.n_images,
                                   t.img_ptr_host.data(), &why) != 0)
            return fail(h, -1, "%s", why.c_str());
    }
    const size_t C = (size_t)p.counts[0], P = (size_t)p.counts[1], N = (size_t)p.counts[2];
    if (N == 0) return 0;                                        // (no observation: no camera and no point either)
    static_assert(sizeof(long long) == sizeof(int64_t), "the index arrays are downloaded as they are");
    if (points_2d) {
        CHK(ensure_all(h, {{&p.p2d, sizeof(double) * 2 * (size_t)t.T}}));
        hipLaunchKernelGGL(k_plan_gather, dim3(plan_grid((int64_t)N)), dim3(kPlanBlock), 0, h->stream, (long long)N,
                           (const int*)p.of.as<int>(), (const double2*)p.kp.as<double2>(), p.p2d.as<double2>());
        LAUNCHED(h);
    }
    HIPCHK(h, download(h, cam_of, p.cam_of.p, sizeof(int32_t) * C));
    HIPCHK(h, download(h, pt_of, p.pt_of.p, sizeof(int32_t) * P));
    HIPCHK(h, download(h, camera_indices, p.ci.p, sizeof(int64_t) * N));
    HIPCHK(h, download(h, point_indices, p.pi.p, sizeof(int64_t) * N));
    HIPCHK(h, download(h, obs_feat, p.of.p, sizeof(int32_t) * N));
    if (points_2d) HIPCHK(h, download(h, points_2d, p.p2d.p, sizeof(double) * 2 * N));
    CHK(wait_stream(h));
    return 0;
}
