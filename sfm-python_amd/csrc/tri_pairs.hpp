// tri_pairs.hpp -- the view pairs of a track, for host and device: how many there are and which pair (i < j) carries the
// number h in lexicographic order -- (0,1), (0,2), ..., (0,n-1), (1,2), ..., (n-2,n-1).  Plain integer code without a
// device call: k_tri_ransac (consumer_kernels.hpp) numbers its exhaustive hypotheses with it and
// tests/host/tri_pairs_check.cpp runs it as a stand-alone program under the host sanitizers.  DESIGN.md section 30.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFMBA_TRI_HD __host__ __device__
#else
#define SFMBA_TRI_HD
#endif

namespace sfmba {

// M = n (n - 1) / 2 (0 for n < 2); 64 bits: n = 65537 passes 2^31
SFMBA_TRI_HD inline long long tri_pair_count(long long n) { return n < 2 ? 0 : n * (n - 1) / 2; }

// floor(sqrt(v)) for 0 <= v < 2^62: the double root, corrected by at most a step either way
SFMBA_TRI_HD inline long long tri_isqrt(long long v) {
    long long r = (long long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// number of the pair (i < j) among the pairs of n views
SFMBA_TRI_HD inline long long tri_pair_rank(long long n, long long i, long long j) {
    return i * (2 * n - i - 1) / 2 + (j - i - 1);
}

// the pair of number h, 0 <= h < M.  Counted from the END the rows have 1, 2, 3, ... pairs: with r = M - 1 - h, the
// row from the end is k = floor((sqrt(8 r + 1) - 1) / 2), and r - k (k + 1) / 2 the place in it, from its end.
SFMBA_TRI_HD inline void tri_pair_unrank(long long n, long long h, int& i, int& j) {
    const long long r = tri_pair_count(n) - 1 - h;
    const long long k = (tri_isqrt(8 * r + 1) - 1) / 2;
    i = (int)(n - 2 - k);
    j = (int)(n - 1 - (r - k * (k + 1) / 2));
}

}  // namespace sfmba
