// Validation of the arguments of sfmba_build_tracks, without a device: plain C++ that tracks.hip calls before any kernel
// reads a pair, and that tests/host/track_inputs_check.cpp runs as a stand-alone program under the host sanitizers.
// DESIGN.md section 23.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <string>
#include <vector>

namespace sfmba {

struct TrackBatch {
    int64_t N = 0, M = 0, Mu = 0;        // features, pairs, used pairs
    std::vector<int32_t> packed;         // [Mu][2] global feature ids of the used pairs, in the order given
};

inline int track_fail(std::string* err, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    if (err) *err = buf;
    return -1;
}

// 0: the input is well formed and `out` holds its sizes and (want_packed) the used pairs as global feature ids;
// -1 with the reason in *err otherwise.  Every pair is checked, used or not.
inline int track_check_inputs(int64_t n_images, const int64_t* img_ptr, int64_t n_edges, const int32_t* edges,
                              const int64_t* pair_ptr, const int32_t* pairs, const uint8_t* pair_use, int32_t min_length,
                              int32_t max_length, int32_t conflicts, bool want_packed, TrackBatch* out, std::string* err) {
    if (n_images < 0 || !img_ptr) return track_fail(err, "sfmba_build_tracks: n_images is negative or img_ptr is NULL");
    if (n_edges < 0 || !pair_ptr || (n_edges && !edges))
        return track_fail(err, "sfmba_build_tracks: n_edges is negative, or edges or pair_ptr is NULL");
    if (min_length < 1) return track_fail(err, "sfmba_build_tracks: min_length must be at least 1, got %lld", min_length);
    if (max_length < 0 || (max_length != 0 && max_length < min_length))
        return track_fail(err, "sfmba_build_tracks: max_length %lld is below min_length %lld (0 = no limit)", max_length, min_length);
    if (conflicts != 0 && conflicts != 1)
        return track_fail(err, "sfmba_build_tracks: conflicts must be 0 (drop) or 1 (keep), got %lld", conflicts);
    if (img_ptr[0] != 0) return track_fail(err, "sfmba_build_tracks: img_ptr[0] must be 0");
    for (int64_t i = 0; i < n_images; ++i)
        if (img_ptr[i + 1] < img_ptr[i]) return track_fail(err, "sfmba_build_tracks: img_ptr must ascend (image %lld)", i);
    const int64_t N = img_ptr[n_images];
    if (N >= ((int64_t)1 << 31)) return track_fail(err, "sfmba_build_tracks: %lld features, the limit is 2^31 - 1", N);
    if (pair_ptr[0] != 0) return track_fail(err, "sfmba_build_tracks: pair_ptr[0] must be 0");
    for (int64_t e = 0; e < n_edges; ++e)
        if (pair_ptr[e + 1] < pair_ptr[e]) return track_fail(err, "sfmba_build_tracks: pair_ptr must ascend (edge %lld)", e);
    const int64_t M = pair_ptr[n_edges];
    if (M && !pairs) return track_fail(err, "sfmba_build_tracks: pairs is NULL");
    out->N = N; out->M = M; out->Mu = 0;
    out->packed.clear();
    if (want_packed) out->packed.reserve(2 * (size_t)M);
    for (int64_t e = 0; e < n_edges; ++e) {
        const int64_t u = edges[2 * e], v = edges[2 * e + 1];
        if (u < 0 || u >= n_images || v < 0 || v >= n_images)
            return track_fail(err, "sfmba_build_tracks: edge %lld names image %lld, there are %lld", e,
                              u < 0 || u >= n_images ? u : v, n_images);
        if (u == v) return track_fail(err, "sfmba_build_tracks: edge %lld joins image %lld to itself", e, u);
        const int64_t bu = img_ptr[u], nu = img_ptr[u + 1] - bu, bv = img_ptr[v], nv = img_ptr[v + 1] - bv;
        for (int64_t k = pair_ptr[e]; k < pair_ptr[e + 1]; ++k) {
            const int64_t a = pairs[2 * k], b = pairs[2 * k + 1];
            if (a < 0 || a >= nu) return track_fail(err, "sfmba_build_tracks: pair %lld names row %lld of image %lld", k, a, u);
            if (b < 0 || b >= nv) return track_fail(err, "sfmba_build_tracks: pair %lld names row %lld of image %lld", k, b, v);
            if (pair_use && !pair_use[k]) continue;
            ++out->Mu;
            if (want_packed) {
                out->packed.push_back((int32_t)(bu + a));
                out->packed.push_back((int32_t)(bv + b));
            }
        }
    }
    return 0;
}

}  // namespace sfmba
