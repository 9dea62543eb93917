// cov_inputs_check -- runs the device-free part of sfmba_covariance (csrc/cov_inputs.hpp) so that it can be compiled with
// the host sanitizers: the checks of the hold list, the gauge choice, the held mask and the counts.  Every array is a heap
// block of exactly the size the interface states: a read or write past an end is the sanitizer's to see.  Exit status 0:
// every case gave the expected mask, gauge and counts, every malformed hold list was refused with a reason.
#include <cstdio>
#include <cstring>

#include "cov_inputs.hpp"

using namespace sfmba;

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "cov_inputs_check: %s\n", what); ++failures; }
}

// C cameras with T_c = t[c], P points with the given run offsets, views per camera
struct Scene {
    std::vector<double> x;
    std::vector<char> fixed;
    std::vector<int> views, ptr;
    int64_t C, P, N;
    Scene(const std::vector<std::vector<double>>& t, const std::vector<int>& views_, const std::vector<int>& ptr_)
        : fixed(t.size(), 0), views(views_), ptr(ptr_), C((int64_t)t.size()), P((int64_t)ptr_.size() - 1), N(ptr_.back()) {
        x.assign((size_t)(6 * C + 3 * P), 0.25);
        for (int64_t c = 0; c < C; ++c)
            for (int k = 0; k < 3; ++k) x[(size_t)(6 * c + 3 + k)] = t[(size_t)c][(size_t)k];
    }
    CovCounts mask(const std::vector<int32_t>& hold, bool gauge_on, std::vector<unsigned char>* held, CovGauge* g) const {
        held->assign((size_t)(6 * C), 0xEE);
        return cov_held_mask(x.data(), C, P, N, fixed.data(), views.data(), ptr.data(), hold.empty() ? nullptr : hold.data(),
                             (int32_t)hold.size(), gauge_on, held->data(), g);
    }
};

int count(const std::vector<unsigned char>& m, unsigned char v) {
    int n = 0;
    for (unsigned char q : m) n += q == v;
    return n;
}

}  // namespace

int main() {
    // ---- the hold list
    {
        const std::vector<int32_t> good = {0, 5, 17}, rep = {3, 4, 3}, low = {-1}, high = {18};
        expect(cov_check_hold(good.data(), 3, 3).empty(), "a valid hold list was refused");
        expect(cov_check_hold(nullptr, 0, 3).empty(), "an empty hold list was refused");
        expect(cov_check_hold(rep.data(), 3, 3).find("repeated") != std::string::npos, "a repeated index was accepted");
        expect(cov_check_hold(low.data(), 1, 3).find("out of range") != std::string::npos, "index -1 was accepted");
        expect(cov_check_hold(high.data(), 1, 3).find("out of range") != std::string::npos, "index 6 C was accepted");
        expect(!cov_check_hold(nullptr, 2, 3).empty(), "a NULL list with n_hold > 0 was accepted");
        expect(!cov_check_hold(good.data(), -1, 3).empty(), "a negative n_hold was accepted");
    }
    // ---- the default gauge: camera 0 and the farthest camera's largest component; ties go to the lowest index / axis
    {
        Scene s({{0, 0, 0}, {1, 0, 0}, {0, -3, 1}, {0, 3, -1}}, {2, 2, 2, 2}, {0, 4, 8});
        std::vector<unsigned char> held;
        CovGauge g;
        const CovCounts n = s.mask({}, true, &held, &g);
        expect(g.g0 == 0 && g.g1 == 2 && g.axis == 1, "gauge of the four-camera scene (tie between cameras 2 and 3)");
        expect(count(held, kCovHeld) == 7 && held[6 * 2 + 3 + 1] == kCovHeld && held[5] == kCovHeld, "mask of the default gauge");
        expect(n.n_free == 17 && n.n_held == 7 && n.obs_points == 2 && n.dof == 2 * 8 - 17 - 6, "counts of the default gauge");
        Scene t({{0, 0, 0}, {2, -2, 1}}, {1, 1}, {0, 2});
        t.mask({}, true, &held, &g);
        expect(g.g1 == 1 && g.axis == 0, "equal components: the lowest axis");
    }
    // ---- one camera held by the problem: it is g0; two held: no gauge; a hold list: no gauge; gauge off: nothing
    {
        Scene s({{0, 0, 0}, {1, 0, 0}, {0, 0, 5}}, {3, 3, 3}, {0, 3, 6, 9});
        std::vector<unsigned char> held;
        CovGauge g;
        s.fixed[1] = 1;
        CovCounts n = s.mask({}, true, &held, &g);
        expect(g.g0 == 1 && g.g1 == 2 && g.axis == 2 && n.n_held == 7, "one held camera is the gauge's first");
        s.fixed[2] = 1;
        n = s.mask({}, true, &held, &g);
        expect(g.g0 == -1 && g.g1 == -1 && n.n_held == 12 && n.n_free == 6, "two held cameras: no gauge is added");
        s.fixed[1] = s.fixed[2] = 0;
        n = s.mask({4}, true, &held, &g);
        expect(g.g0 == -1 && n.n_held == 1 && held[4] == kCovHeld, "a hold list switches the default gauge off");
        n = s.mask({}, false, &held, &g);
        expect(g.g0 == -1 && n.n_held == 0 && n.n_free == 18 && n.dof == 18 - 18 - 9, "gauge = 0 adds nothing");
    }
    // ---- cameras and points nobody observes
    {
        Scene s({{0, 0, 0}, {9, 9, 9}, {1, 0, 0}}, {4, 0, 4}, {0, 4, 4, 8});       // camera 1 and point 1 are unobserved
        std::vector<unsigned char> held;
        CovGauge g;
        const CovCounts n = s.mask({7}, false, &held, &g);
        expect(count(held, kCovUnobserved) == 6 && held[7] == kCovUnobserved, "an unobserved camera is 2, held or not");
        expect(n.n_free == 12 && n.n_held == 0 && n.obs_points == 2 && n.dof == 16 - 12 - 6, "counts with unobserved parameters");
        s.mask({}, true, &held, &g);
        expect(g.g1 == 2, "an unobserved camera is never the gauge's second");
        Scene one({{1, 2, 3}}, {5}, {0, 5});
        const CovCounts m = one.mask({}, true, &held, &g);
        expect(g.g0 == 0 && g.g1 == -1 && m.n_held == 6 && m.n_free == 0, "a single camera: all of it is held");
    }
    if (failures) return 1;
    printf("cov_inputs_check: ok\n");
    return 0;
}
