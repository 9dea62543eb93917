// track_inputs_check -- runs the argument checks of sfmba_build_tracks (csrc/track_inputs.hpp) without a device, so that
// they can be compiled with the host sanitizers.  Every array is a heap block of exactly the size the interface states:
// a read past an end is the sanitizer's to see.  Exit status 0: every well-formed input was accepted with the expected
// packed pairs, every malformed one refused with a reason.
#include <cstdio>
#include <cstring>

#include "track_inputs.hpp"

using namespace sfmba;

namespace {

struct Case {
    std::vector<int64_t> img_ptr;
    std::vector<int32_t> edges;
    std::vector<int64_t> pair_ptr;
    std::vector<int32_t> pairs;
    std::vector<uint8_t> use;
    bool masked = false;
    int32_t min_length = 2, max_length = 0, conflicts = 0;
};

int failures = 0;

int run(const Case& c, TrackBatch* bt, std::string* why, bool packed = true) {
    return track_check_inputs((int64_t)c.img_ptr.size() - 1, c.img_ptr.data(), (int64_t)c.pair_ptr.size() - 1,
                              c.edges.empty() ? nullptr : c.edges.data(), c.pair_ptr.data(), c.pairs.empty() ? nullptr : c.pairs.data(),
                              c.masked ? c.use.data() : nullptr, c.min_length, c.max_length, c.conflicts, packed, bt, why);
}

void expect_ok(const char* name, const Case& c, int64_t N, const std::vector<int32_t>& packed) {
    TrackBatch bt;
    std::string why;
    const int rc = run(c, &bt, &why);
    const int64_t M = (int64_t)c.pairs.size() / 2;
    if (rc != 0 || bt.N != N || bt.M != M || bt.Mu != (int64_t)packed.size() / 2 || bt.packed != packed) {
        fprintf(stderr, "%s: rc %d (%s), N %lld M %lld Mu %lld\n", name, rc, why.c_str(), (long long)bt.N, (long long)bt.M,
                (long long)bt.Mu);
        ++failures;
    }
    TrackBatch sizes;
    if (run(c, &sizes, &why, false) != 0 || sizes.Mu != bt.Mu || !sizes.packed.empty()) {
        fprintf(stderr, "%s: the call without packed pairs disagrees\n", name);
        ++failures;
    }
}

void expect_bad(const char* name, const Case& c) {
    TrackBatch bt;
    std::string why;
    const int rc = run(c, &bt, &why);
    if (rc != -1 || why.empty()) {
        fprintf(stderr, "%s: rc %d, reason '%s'\n", name, rc, why.c_str());
        ++failures;
    }
}

// three images of 2, 0 and 3 features; edge (0, 2) with two pairs, edge (2, 0) with one
Case base() {
    Case c;
    c.img_ptr = {0, 2, 2, 5};
    c.edges = {0, 2, 2, 0};
    c.pair_ptr = {0, 2, 3};
    c.pairs = {0, 1, 1, 2, 0, 1};
    return c;
}

}  // namespace

int main() {
    expect_ok("base", base(), 5, {0, 3, 1, 4, 2, 1});
    { Case c = base(); c.masked = true; c.use = {1, 0, 1}; expect_ok("masked", c, 5, {0, 3, 2, 1}); }
    { Case c = base(); c.masked = true; c.use = {0, 0, 0}; expect_ok("all masked", c, 5, {}); }
    { Case c = base(); c.edges.clear(); c.pair_ptr = {0}; c.pairs.clear(); expect_ok("no edges", c, 5, {}); }
    { Case c = base(); c.pair_ptr = {0, 0, 0}; c.pairs.clear(); expect_ok("no pairs", c, 5, {}); }
    { Case c; c.img_ptr = {0}; c.pair_ptr = {0}; expect_ok("no images", c, 0, {}); }
    { Case c = base(); c.edges = {0, 2, 0, 2}; c.pairs = {0, 1, 0, 1, 0, 1}; expect_ok("repeats", c, 5, {0, 3, 0, 3, 0, 3}); }
    { Case c = base(); c.min_length = 1; c.max_length = 1; c.conflicts = 1; expect_ok("options at their edges", c, 5, {0, 3, 1, 4, 2, 1}); }
    { Case c = base(); c.min_length = 3; c.max_length = 3; expect_ok("max equals min", c, 5, {0, 3, 1, 4, 2, 1}); }

    { Case c = base(); c.img_ptr[0] = 1; expect_bad("img_ptr from 1", c); }
    { Case c = base(); c.img_ptr = {0, 3, 2, 5}; expect_bad("img_ptr descends", c); }
    { Case c = base(); c.pair_ptr[0] = 1; expect_bad("pair_ptr from 1", c); }
    { Case c = base(); c.pair_ptr = {0, 3, 2}; expect_bad("pair_ptr descends", c); }
    { Case c = base(); c.edges[1] = 3; expect_bad("image past the end", c); }
    { Case c = base(); c.edges[2] = -1; expect_bad("negative image", c); }
    { Case c = base(); c.edges[3] = 2; expect_bad("u == v", c); }
    { Case c = base(); c.pairs[0] = 2; expect_bad("row past u", c); }
    { Case c = base(); c.pairs[3] = 3; expect_bad("row past v", c); }
    { Case c = base(); c.pairs[4] = -1; expect_bad("negative row", c); }
    { Case c = base(); c.edges = {0, 1, 2, 0}; expect_bad("row of an empty image", c); }
    { Case c = base(); c.masked = true; c.use = {1, 0, 1}; c.pairs[2] = 2; expect_bad("bad row of an unused pair", c); }
    { Case c = base(); c.img_ptr = {0, 2, 2, (int64_t)1 << 31}; expect_bad("2^31 features", c); }
    { Case c = base(); c.min_length = 0; expect_bad("min_length 0", c); }
    { Case c = base(); c.min_length = 3; c.max_length = 2; expect_bad("max below min", c); }
    { Case c = base(); c.max_length = -1; expect_bad("negative max_length", c); }
    { Case c = base(); c.conflicts = 2; expect_bad("conflicts 2", c); }
    {   // the largest feature count that is allowed, in an image nothing points into
        Case c = base(); c.img_ptr = {0, 2, 2, 5, ((int64_t)1 << 31) - 1};
        expect_ok("2^31 - 1 features", c, ((int64_t)1 << 31) - 1, {0, 3, 1, 4, 2, 1});
    }
    if (failures) { fprintf(stderr, "%d case(s) failed\n", failures); return 1; }
    printf("track_inputs_check: ok\n");
    return 0;
}
