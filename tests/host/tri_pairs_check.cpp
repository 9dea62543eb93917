// tri_pairs_check -- runs the pair numbering of sfmba_triangulate_ransac (csrc/tri_pairs.hpp) without a device, so that it
// can be compiled with the host sanitizers (signed overflow is the undefined-behaviour sanitizer's to see).  Exit status
// 0: for n = 2 .. 2000 every h gave the pair that a plain double loop meets h-th and ranked back to h; for n whose pair
// count lies near 2^31 the ends, the row starts and a stride of values did.
#include <cstdio>

#include "tri_pairs.hpp"

using namespace sfmba;

namespace {

int failures = 0;

void expect(bool ok, const char* what, long long n, long long h, int i, int j) {
    if (ok) return;
    if (failures < 20) fprintf(stderr, "%s: n %lld h %lld -> (%d, %d)\n", what, n, h, i, j);
    ++failures;
}

// one h of n views: in range, ordered, and the rank of the pair is h again
void spot(long long n, long long h) {
    int i = -1, j = -1;
    tri_pair_unrank(n, h, i, j);
    expect(0 <= i && i < j && j < n, "pair out of range", n, h, i, j);
    expect(tri_pair_rank(n, i, j) == h, "round trip", n, h, i, j);
}

}  // namespace

int main() {
    if (tri_pair_count(0) != 0 || tri_pair_count(1) != 0 || tri_pair_count(2) != 1 || tri_pair_count(12) != 66) {
        fprintf(stderr, "tri_pair_count is wrong for a small n\n");
        ++failures;
    }
    for (long long v = 0; v < 70000; ++v) {
        const long long r = tri_isqrt(v);
        if (r * r > v || (r + 1) * (r + 1) <= v) { fprintf(stderr, "tri_isqrt(%lld) = %lld\n", v, r); ++failures; }
    }
    for (long long n = 2; n <= 2000; ++n) {
        long long h = 0;
        for (int a = 0; a + 1 < n; ++a)
            for (int b = a + 1; b < n; ++b, ++h) {
                int i = -1, j = -1;
                tri_pair_unrank(n, h, i, j);
                expect(i == a && j == b, "not the h-th pair of the double loop", n, h, i, j);
                expect(tri_pair_rank(n, a, b) == h, "rank", n, h, a, b);
            }
        if (h != tri_pair_count(n)) { fprintf(stderr, "n %lld: %lld pairs counted, %lld stated\n", n, h, tri_pair_count(n)); ++failures; }
    }
    // M just below, at and above 2^31: n = 65536 has 2^31 - 32768 pairs, n = 65537 has 2^31 + 32768
    const long long big[] = {46341, 65535, 65536, 65537, 65538, 92682};
    for (long long n : big) {
        const long long M = tri_pair_count(n);
        if (M != n * (n - 1) / 2) { fprintf(stderr, "tri_pair_count(%lld)\n", n); ++failures; }
        spot(n, 0); spot(n, 1); spot(n, M - 1); spot(n, M - 2); spot(n, M / 2);
        if (M > ((long long)1 << 31)) { spot(n, ((long long)1 << 31) - 1); spot(n, (long long)1 << 31); spot(n, ((long long)1 << 31) + 1); }
        for (long long a = 0; a + 1 < n; a += 257) {             // the first and the last pair of a row, and the one before
            const long long h0 = tri_pair_rank(n, a, a + 1);
            int i = -1, j = -1;
            tri_pair_unrank(n, h0, i, j);
            expect(i == a && j == a + 1, "row start", n, h0, i, j);
            tri_pair_unrank(n, h0 + (n - a - 2), i, j);
            expect(i == a && j == n - 1, "row end", n, h0 + (n - a - 2), i, j);
            if (h0 > 0) {
                tri_pair_unrank(n, h0 - 1, i, j);
                expect(i == a - 1 && j == n - 1, "end of the row before", n, h0 - 1, i, j);
            }
        }
        for (long long h = 0; h < M; h += 1000003) spot(n, h);
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("tri_pairs_check: ok\n");
    return 0;
}
