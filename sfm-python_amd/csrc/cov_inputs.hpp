// cov_inputs.hpp -- the device-free part of sfmba_covariance (covariance.hip): the checks of the `hold` list, the gauge
// chosen from x, the held mask and the counts that follow from it.  Plain C++ (no HIP header), so that
// tests/host/cov_inputs_check.cpp compiles it as a stand-alone program under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace sfmba {

enum : unsigned char { kCovFree = 0, kCovHeld = 1, kCovUnobserved = 2 };

// hold[k] in [0, 6 C), no index twice.  Empty string: fine; else what is wrong.
inline std::string cov_check_hold(const int32_t* hold, int32_t n_hold, int64_t C) {
    char buf[160];
    if (n_hold < 0) return "n_hold is negative";
    if (n_hold > 0 && !hold) return "hold is NULL although n_hold > 0";
    std::vector<char> seen((size_t)(6 * C), 0);
    for (int32_t k = 0; k < n_hold; ++k) {
        const int64_t q = hold[k];
        if (q < 0 || q >= 6 * C) {
            snprintf(buf, sizeof buf, "hold[%d] = %lld is out of range [0, %lld)", (int)k, (long long)q, (long long)(6 * C));
            return buf;
        }
        if (seen[(size_t)q]) {
            snprintf(buf, sizeof buf, "hold[%d] = %lld is repeated", (int)k, (long long)q);
            return buf;
        }
        seen[(size_t)q] = 1;
    }
    return std::string();
}

// The default gauge ("first camera plus one baseline coordinate"): g0 = the camera the problem holds if there is one,
// else camera 0; g1 = the observed camera whose centre parameter T is farthest from T_g0 (ties: the lowest index);
// axis = the largest |T_g1 - T_g0| component (ties: the lowest axis).  g1 = -1: no second camera to hold.
struct CovGauge { int32_t g0 = -1, g1 = -1, axis = -1; };
inline CovGauge cov_choose_gauge(const double* x, int64_t C, const char* fixed, const char* observed) {
    CovGauge g;
    if (C <= 0) return g;
    g.g0 = 0;
    for (int64_t c = 0; c < C; ++c)
        if (fixed[c]) { g.g0 = (int32_t)c; break; }
    const double* T0 = x + 6 * (int64_t)g.g0 + 3;
    double best = -1.0;
    for (int64_t c = 0; c < C; ++c) {
        if (c == g.g0 || !observed[c]) continue;
        const double* T = x + 6 * c + 3;
        const double dx = T[0] - T0[0], dy = T[1] - T0[1], dz = T[2] - T0[2];
        const double d = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (d > best) { best = d; g.g1 = (int32_t)c; }          // (a NaN distance never wins)
    }
    if (g.g1 >= 0) {
        const double* T = x + 6 * (int64_t)g.g1 + 3;
        double bd = -1.0;
        for (int k = 0; k < 3; ++k) {
            const double d = std::fabs(T[k] - T0[k]);
            if (d > bd) { bd = d; g.axis = k; }
        }
        if (g.axis < 0) g.axis = 0;
    }
    return g;
}

struct CovCounts {
    int32_t n_free = 0, n_held = 0;      // entries 0 / 1 of the mask
    int64_t obs_points = 0;              // points with at least one observation
    int64_t dof = 0;                     // 2 N - free observed camera parameters - 3 observed points
};

// held[6 C]: 2 for the parameters of a camera nobody observes, else 1 for a parameter in the held set D = the cameras the
// problem holds | the hold list | the default gauge (gauge_on, no hold list, fewer than two cameras held), else 0.
// cam_views[C]: observations per camera; pt_ptr[P + 1]: run offsets of the points.
inline CovCounts cov_held_mask(const double* x, int64_t C, int64_t P, int64_t N, const char* fixed, const int* cam_views,
                               const int* pt_ptr, const int32_t* hold, int32_t n_hold, bool gauge_on, unsigned char* held,
                               CovGauge* gauge_out) {
    std::vector<char> observed((size_t)C, 0);
    int64_t n_fixed = 0;
    for (int64_t c = 0; c < C; ++c) { observed[(size_t)c] = cam_views[c] > 0; n_fixed += fixed[c] ? 1 : 0; }
    for (int64_t q = 0; q < 6 * C; ++q) held[q] = fixed[q / 6] ? kCovHeld : kCovFree;
    for (int32_t k = 0; k < n_hold; ++k) held[hold[k]] = kCovHeld;
    CovGauge g;
    if (gauge_on && n_hold == 0 && n_fixed < 2) {
        g = cov_choose_gauge(x, C, fixed, observed.data());
        if (g.g0 >= 0)
            for (int k = 0; k < 6; ++k) held[6 * (int64_t)g.g0 + k] = kCovHeld;
        if (g.g1 >= 0) held[6 * (int64_t)g.g1 + 3 + g.axis] = kCovHeld;
    }
    for (int64_t q = 0; q < 6 * C; ++q)
        if (!observed[(size_t)(q / 6)]) held[q] = kCovUnobserved;
    CovCounts n;
    for (int64_t q = 0; q < 6 * C; ++q) { n.n_free += held[q] == kCovFree; n.n_held += held[q] == kCovHeld; }
    for (int64_t p = 0; p < P; ++p) n.obs_points += pt_ptr[p + 1] > pt_ptr[p] ? 1 : 0;
    n.dof = 2 * N - (int64_t)n.n_free - 3 * n.obs_points;
    if (gauge_out) *gauge_out = g;
    return n;
}

}  // namespace sfmba
