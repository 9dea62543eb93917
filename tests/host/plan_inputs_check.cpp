// plan_inputs_check -- runs the argument checks of the plan stage (csrc/plan_inputs.hpp) without a device, so that they
// can be compiled with the host sanitizers.  Every array is a heap block of exactly the size the interface states: a read
// past an end is the sanitizer's to see.  Exit status 0: every well-formed input was accepted, every malformed one
// refused with a reason that starts with the function's name.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "plan_inputs.hpp"

using namespace sfmba;

namespace {

int failures = 0;

void expect(const char* name, int rc, const std::string& why, bool ok, const char* fn) {
    const bool named = why.compare(0, strlen(fn), fn) == 0 && why.size() > strlen(fn) + 2;
    if (ok ? rc != 0 : (rc != -1 || !named)) {
        fprintf(stderr, "%s: rc %d, reason '%s'\n", name, rc, why.c_str());
        ++failures;
    }
}

void masks(const char* name, bool ok, std::vector<uint8_t> cam, std::vector<uint8_t> trk, int64_t built_images, int64_t built_tracks,
           bool null_cam = false, bool null_trk = false) {
    std::string why;
    const int rc = plan_check_masks("sfmba_plan_views", (int64_t)cam.size(), null_cam ? nullptr : cam.data(), (int64_t)trk.size(),
                                    null_trk ? nullptr : trk.data(), built_images, built_tracks, &why);
    expect(name, rc, why, ok, "sfmba_plan_views");
}

void keypoints(const char* name, bool ok, std::vector<int64_t> img_ptr, std::vector<double> pts, int64_t want_N = 0, bool null_pts = false) {
    std::string why;
    int64_t N = -1;
    const int rc = plan_check_keypoints((int64_t)img_ptr.size() - 1, img_ptr.data(), null_pts ? nullptr : pts.data(), &N, &why);
    expect(name, rc, why, ok, "sfmba_set_keypoints");
    if (ok && N != want_N) { fprintf(stderr, "%s: N %lld, expected %lld\n", name, (long long)N, (long long)want_N); ++failures; }
}

void same(const char* name, bool ok, std::vector<int64_t> a, std::vector<int64_t> b) {
    std::string why;
    const int rc = plan_check_same_images("sfmba_get_assembled", (int64_t)a.size() - 1, a.data(), (int64_t)b.size() - 1, b.data(), &why);
    expect(name, rc, why, ok, "sfmba_get_assembled");
}

}  // namespace

int main() {
    masks("masks", true, {1, 0, 1}, {0, 1}, 3, 2);
    masks("any non-zero byte", true, {255, 0, 2}, {7, 0}, 3, 2);
    masks("no tracks", true, {1, 0, 1}, {}, 3, 0, false, true);
    masks("nothing at all", true, {}, {}, 0, 0, true, true);
    masks("short image mask", false, {1, 0}, {0, 1}, 3, 2);
    masks("long image mask", false, {1, 0, 1, 1}, {0, 1}, 3, 2);
    masks("short track mask", false, {1, 0, 1}, {0}, 3, 2);
    masks("long track mask", false, {1, 0, 1}, {0, 1, 1}, 3, 2);
    masks("NULL image mask", false, {1, 0, 1}, {0, 1}, 3, 2, true, false);
    masks("NULL track mask", false, {1, 0, 1}, {0, 1}, 3, 2, false, true);

    for (int32_t mv : {1, 2, 3, 1 << 30}) {
        std::string why;
        expect("min_views accepted", plan_check_min_views("sfmba_assemble_problem", mv, &why), why, true, "sfmba_assemble_problem");
    }
    for (int32_t mv : {0, -1, std::numeric_limits<int32_t>::min()}) {
        std::string why;
        expect("min_views refused", plan_check_min_views("sfmba_assemble_problem", mv, &why), why, false, "sfmba_assemble_problem");
    }

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    keypoints("keypoints", true, {0, 2, 2, 3}, {1, 2, 3, 4, 5, 6}, 3);
    keypoints("no features", true, {0, 0, 0}, {}, 0, true);
    keypoints("no images", true, {0}, {}, 0, true);
    keypoints("img_ptr from 1", false, {1, 2, 3}, {1, 2, 3, 4, 5, 6});
    keypoints("img_ptr descends", false, {0, 2, 1}, {1, 2, 3, 4});
    keypoints("2^31 features", false, {0, (int64_t)1 << 31}, {1, 2});
    keypoints("NULL pts", false, {0, 1}, {1, 2}, 0, true);
    keypoints("infinite pixel", false, {0, 2}, {1, 2, 3, inf});
    keypoints("negative infinite pixel", false, {0, 2}, {-inf, 2, 3, 4});
    keypoints("NaN pixel", false, {0, 2}, {1, nan, 3, 4});
    {
        std::string why;
        expect("NULL img_ptr", plan_check_keypoints(1, nullptr, nullptr, nullptr, &why), why, false, "sfmba_set_keypoints");
        std::vector<int64_t> p = {0};
        expect("negative n_images", plan_check_keypoints(-1, p.data(), nullptr, nullptr, &why), why, false, "sfmba_set_keypoints");
    }

    same("same img_ptr", true, {0, 2, 2, 5}, {0, 2, 2, 5});
    same("another image count", false, {0, 2, 5}, {0, 2, 2, 5});
    same("another img_ptr", false, {0, 2, 3, 5}, {0, 2, 2, 5});
    same("another end", false, {0, 2, 2, 6}, {0, 2, 2, 5});

    if (failures) { fprintf(stderr, "%d case(s) failed\n", failures); return 1; }
    printf("plan_inputs_check: ok\n");
    return 0;
}
