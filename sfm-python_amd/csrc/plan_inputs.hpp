// Validation of the arguments of the plan stage (sfmba_plan_views, sfmba_assemble_problem, sfmba_set_keypoints), without a
// device: plain C++ that plan.hip calls before anything is uploaded, and that tests/host/plan_inputs_check.cpp runs as a
// stand-alone program under the host sanitizers.  DESIGN.md section 25.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <string>

namespace sfmba {

// -1 with "<function>: <reason>" in *err
inline int plan_fail(std::string* err, const char* fn, const char* fmt, long long a = 0, long long b = 0) {
    char why[200], buf[256];
    snprintf(why, sizeof why, fmt, a, b);
    snprintf(buf, sizeof buf, "%s: %s", fn, why);
    if (err) *err = buf;
    return -1;
}

// the two masks of a call against the sizes of the last build: one entry per image, one per kept track
inline int plan_check_masks(const char* fn, int64_t n_images, const uint8_t* cam_mask, int64_t n_tracks, const uint8_t* trk_mask,
                            int64_t built_images, int64_t built_tracks, std::string* err) {
    if (n_images != built_images)
        return plan_fail(err, fn, "the image mask has %lld entries, the tracks were built over %lld images", n_images, built_images);
    if (n_tracks != built_tracks)
        return plan_fail(err, fn, "the track mask has %lld entries, the last build kept %lld tracks", n_tracks, built_tracks);
    if (n_images > 0 && !cam_mask) return plan_fail(err, fn, "the image mask is NULL");
    if (n_tracks > 0 && !trk_mask) return plan_fail(err, fn, "the track mask is NULL");
    return 0;
}

inline int plan_check_min_views(const char* fn, int32_t min_views, std::string* err) {
    if (min_views < 1) return plan_fail(err, fn, "min_views must be at least 1, got %lld", min_views);
    return 0;
}

// img_ptr (n_images + 1) ascending from 0 to N < 2^31, pts (N, 2) finite; 0 with N in *n_features
inline int plan_check_keypoints(int64_t n_images, const int64_t* img_ptr, const double* pts, int64_t* n_features, std::string* err) {
    const char* const fn = "sfmba_set_keypoints";
    if (n_images < 0 || !img_ptr) return plan_fail(err, fn, "n_images is negative or img_ptr is NULL");
    if (img_ptr[0] != 0) return plan_fail(err, fn, "img_ptr[0] must be 0");
    for (int64_t i = 0; i < n_images; ++i)
        if (img_ptr[i + 1] < img_ptr[i]) return plan_fail(err, fn, "img_ptr must ascend (image %lld)", i);
    const int64_t N = img_ptr[n_images];
    if (N >= ((int64_t)1 << 31)) return plan_fail(err, fn, "%lld features, the limit is 2^31 - 1", N);
    if (N && !pts) return plan_fail(err, fn, "pts is NULL");
    for (int64_t k = 0; k < 2 * N; ++k)
        if (!std::isfinite(pts[k])) return plan_fail(err, fn, "the pixel of feature %lld is not finite", k / 2);
    if (n_features) *n_features = N;
    return 0;
}

// the table of sfmba_set_keypoints against the img_ptr of the last build, where a call reads the table
inline int plan_check_same_images(const char* fn, int64_t n_kp, const int64_t* kp_img_ptr, int64_t n_built, const int64_t* built_img_ptr,
                                  std::string* err) {
    if (n_kp != n_built) return plan_fail(err, fn, "the keypoints are of %lld images, the tracks of %lld", n_kp, n_built);
    for (int64_t i = 0; i <= n_built; ++i)
        if (kp_img_ptr[i] != built_img_ptr[i])
            return plan_fail(err, fn, "the keypoints' img_ptr differs from the tracks' at image %lld", i);
    return 0;
}

}  // namespace sfmba
