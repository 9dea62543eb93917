// tracks.hip -- host code of the feature tracks (kernels: track_kernels.hpp, argument checks: track_inputs.hpp)
#include "handle.hpp"
#include "track_inputs.hpp"
#include "track_kernels.hpp"

namespace {
void track_release(sfmba_handle* h) {
    auto& t = h->tracks;
    for (DevBuf* b : {&t.img_ptr, &t.pairs, &t.parent, &t.size, &t.img, &t.feat_track, &t.members, &t.cursor, &t.comp_off,
                      &t.verdict, &t.kept_len, &t.track_id, &t.track_off, &t.track_ptr, &t.track_feat, &t.track_image,
                      &t.sums, &t.tot})
        b->release();
    t.built = false;
    t.n_tracks = t.T = 0;
}

// the three launches of one scan over `n_max` entries at the most
template <class Src>
int track_scan(sfmba_handle* h, const Src& src, size_t n_max, int slot) {
    auto& t = h->tracks;
    const unsigned nb = (unsigned)std::max<size_t>((n_max + kTrackScanItems - 1) / kTrackScanItems, 1);
    hipLaunchKernelGGL(k_track_scan_reduce<Src>, dim3(nb), dim3(kTrackBlock), 0, h->stream, src, t.sums.as<long long>());
    LAUNCHED(h);
    hipLaunchKernelGGL(k_track_scan_sums, dim3(1), dim3(kTrackBlock), 0, h->stream, t.sums.as<long long>(), nb,
                       t.tot.as<long long>(), slot);
    LAUNCHED(h);
    hipLaunchKernelGGL(k_track_scan_apply<Src>, dim3(nb), dim3(kTrackBlock), 0, h->stream, src, (const long long*)t.sums.as<long long>());
    LAUNCHED(h);
    return 0;
}
}  // namespace

int sfmba::launch_k_track_scan_sums(sfmba_handle* h, long long* sums, unsigned nb, long long* tot, int slot, int block, int items) {
    if (block != kTrackBlock || items != kTrackScanItems)
        return fail(h, -3, "launch_k_track_scan_sums: the caller scans %d entries with %d threads, the kernel %d with %d", items,
                    block, kTrackScanItems, kTrackBlock);
    hipLaunchKernelGGL(k_track_scan_sums, dim3(1), dim3(kTrackBlock), 0, h->stream, sums, nb, tot, slot);
    LAUNCHED(h);
    return 0;
}

void sfmba_default_track_options(sfmba_track_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->min_length = 2; o->max_length = 0; o->conflicts = 0; o->profile = 0;
}

int sfmba_build_tracks(sfmba_handle* h, int64_t n_images, const int64_t* img_ptr, int64_t n_edges, const int32_t* edges,
                       const int64_t* pair_ptr, const int32_t* pairs, const uint8_t* pair_use, const sfmba_track_options* opt,
                       int32_t* feat_track, int64_t* counts, double* kernel_us) {
    CHK(enter(h));
    sfmba_track_options o;
    if (opt) o = *opt; else sfmba_default_track_options(&o);
    TrackBatch bt;
    std::string why;
    if (track_check_inputs(n_images, img_ptr, n_edges, edges, pair_ptr, pairs, pair_use, o.min_length, o.max_length,
                           o.conflicts, true, &bt, &why) != 0)
        return fail(h, -1, "%s", why.c_str());
    if (n_images >= ((int64_t)1 << 31) - 1) return fail(h, -1, "sfmba_build_tracks: too many images");
    const size_t N = (size_t)bt.N, Mu = (size_t)bt.Mu;
    if ((Mu + kTrackBlock - 1) / kTrackBlock >= (size_t)1 << 31) return fail(h, -1, "sfmba_build_tracks: 2^39 used pairs or more");
    auto& t = h->tracks;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    track_release(h);
    // the plan stage: a sub-problem assembled over the previous tracks is gone, and so is a keypoint table of another img_ptr
    t.n_images = n_images; t.N = bt.N;
    t.img_ptr_host.assign(img_ptr, img_ptr + n_images + 1);
    h->plan.assembled = false;
    if (h->plan.have_kp && h->plan.kp_img_ptr != t.img_ptr_host) h->plan.have_kp = false;
    if (kernel_us) *kernel_us = 0.0;
    if (counts) std::fill(counts, counts + 6, (int64_t)0);
    if (Mu == 0) {                                               // no used pair: no component, every feature unmatched
        if (feat_track) std::fill(feat_track, feat_track + N, (int32_t)kTrackUnmatched);
        t.built = true;
        return 0;
    }
    // a component has two members or more and every member is an end of a used pair
    const size_t comps = std::min(N / 2, Mu), memb = std::min(N, 2 * Mu);
    const size_t nb = std::max<size_t>((N + kTrackScanItems - 1) / kTrackScanItems, 1);
    CHK(ensure_all(h, {{&t.img_ptr, sizeof(int) * (size_t)(n_images + 1)}, {&t.pairs, sizeof(int2) * Mu},
                       {&t.parent, sizeof(int) * N}, {&t.size, sizeof(int) * N}, {&t.img, sizeof(int) * N},
                       {&t.feat_track, sizeof(int) * N}, {&t.members, sizeof(int) * memb}, {&t.cursor, sizeof(int) * comps},
                       {&t.comp_off, sizeof(long long) * (comps + 1)}, {&t.verdict, sizeof(int) * comps},
                       {&t.kept_len, sizeof(int) * comps}, {&t.track_id, sizeof(int) * comps},
                       {&t.track_off, sizeof(long long) * comps}, {&t.track_ptr, sizeof(long long) * (comps + 1)},
                       {&t.track_feat, sizeof(int) * memb}, {&t.track_image, sizeof(int) * memb},
                       {&t.sums, sizeof(long long) * 2 * nb}, {&t.tot, sizeof(long long) * kTrackTotSlots}}));
    std::vector<int> ptr32((size_t)n_images + 1);
    for (int64_t i = 0; i <= n_images; ++i) ptr32[(size_t)i] = (int)img_ptr[i];
    HIPCHK(h, hipMemcpyAsync(t.img_ptr.p, ptr32.data(), sizeof(int) * ptr32.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(t.pairs.p, bt.packed.data(), sizeof(int2) * Mu, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                  // (both sources are pageable and die with this call)
    EventPair timer;
    CHK(timer.start(h, o.profile != 0));
    HIPCHK(h, hipMemsetAsync(t.tot.p, 0, sizeof(long long) * kTrackTotSlots, h->stream));
    HIPCHK(h, hipMemsetAsync(t.cursor.p, 0, sizeof(int) * comps, h->stream));
    const unsigned gN = (unsigned)((N + kTrackBlock - 1) / kTrackBlock);
    int* const parent = t.parent.as<int>();
    int* const size = t.size.as<int>();
    long long* const tot = t.tot.as<long long>();
    hipLaunchKernelGGL(k_track_init, dim3(gN), dim3(kTrackBlock), 0, h->stream, (int)N, (const int*)t.img_ptr.as<int>(),
                       (int)n_images, parent, size, t.img.as<int>(), t.feat_track.as<int>());
    LAUNCHED(h);
    hipLaunchKernelGGL(k_track_union, dim3((unsigned)((Mu + kTrackBlock - 1) / kTrackBlock)), dim3(kTrackBlock), 0, h->stream,
                       (long long)Mu, (const int2*)t.pairs.as<int2>(), parent);
    LAUNCHED(h);
    hipLaunchKernelGGL(k_track_flatten, dim3(gN), dim3(kTrackBlock), 0, h->stream, (int)N, parent, size);
    LAUNCHED(h);
    CHK(track_scan(h, TrackCompSrc{parent, size, (int)N, t.comp_off.as<long long>(), tot}, N, kTrackTotComps));
    hipLaunchKernelGGL(k_track_fill, dim3(gN), dim3(kTrackBlock), 0, h->stream, (int)N, (const int*)parent, (const int*)size,
                       (const long long*)t.comp_off.as<long long>(), t.cursor.as<int>(), t.members.as<int>());
    LAUNCHED(h);
    hipLaunchKernelGGL(k_track_sort, dim3((unsigned)((comps + kTrackBlock - 1) / kTrackBlock)), dim3(kTrackBlock), 0, h->stream,
                       (const long long*)t.comp_off.as<long long>(), t.members.as<int>(), (const int*)t.img.as<int>(),
                       o.min_length, o.max_length, o.conflicts, t.verdict.as<int>(), t.kept_len.as<int>(), tot);
    LAUNCHED(h);
    CHK(track_scan(h, TrackKeepSrc{t.kept_len.as<int>(), t.track_id.as<int>(), t.track_off.as<long long>(), tot}, comps,
                   kTrackTotKept));
    hipLaunchKernelGGL(k_track_write, dim3((unsigned)((memb + kTrackBlock - 1) / kTrackBlock)), dim3(kTrackBlock), 0, h->stream,
                       (const int*)t.members.as<int>(), (const int*)parent, (const int*)size,
                       (const long long*)t.comp_off.as<long long>(), (const int*)t.verdict.as<int>(),
                       (const int*)t.track_id.as<int>(), (const long long*)t.track_off.as<long long>(),
                       (const int*)t.img.as<int>(), (const long long*)tot, t.feat_track.as<int>(),
                       t.track_ptr.as<long long>(), t.track_feat.as<int>(), t.track_image.as<int>());
    LAUNCHED(h);
    CHK(timer.stop(h));
    long long totals[kTrackTotSlots];
    HIPCHK(h, download(h, totals, tot, sizeof totals));
    HIPCHK(h, download(h, feat_track, t.feat_track.p, sizeof(int) * N));
    CHK(wait_stream(h));
    CHK(timer.read(h, kernel_us));
    t.n_tracks = totals[kTrackTotKept];
    t.T = totals[kTrackTotObs];
    t.built = true;
    if (counts) {
        counts[0] = totals[kTrackTotComps]; counts[1] = totals[kTrackTotKept]; counts[2] = totals[kTrackTotShort];
        counts[3] = totals[kTrackTotLong]; counts[4] = totals[kTrackTotConflict]; counts[5] = totals[kTrackTotObs];
    }
    return 0;
}

int sfmba_get_tracks(sfmba_handle* h, int64_t* track_ptr, int32_t* track_feat, int32_t* track_image) {
    CHK(enter(h));
    auto& t = h->tracks;
    if (!t.built) return fail(h, -1, "sfmba_get_tracks: no tracks built (call sfmba_build_tracks first)");
    if (t.n_tracks == 0) {
        if (track_ptr) track_ptr[0] = 0;
        return 0;
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "track_ptr is downloaded as it is");
    HIPCHK(h, download(h, track_ptr, t.track_ptr.p, sizeof(int64_t) * (size_t)(t.n_tracks + 1)));
    HIPCHK(h, download(h, track_feat, t.track_feat.p, sizeof(int32_t) * (size_t)t.T));
    HIPCHK(h, download(h, track_image, t.track_image.p, sizeof(int32_t) * (size_t)t.T));
    CHK(wait_stream(h));
    return 0;
}
