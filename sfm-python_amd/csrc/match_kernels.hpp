// Descriptor matching (sfmba_set_descriptors, sfmba_match_descriptors): brute-force 2-nearest-neighbour search by
// squared L2 distance with Lowe's ratio test, for a batch of (query image, train image) edges.  DESIGN.md section 21.
//
// d^2 = |a|^2 + |b|^2 - 2 a.b.  The dot products of a 32-query x 32-train block come from one MFMA accumulator; every
// lane reduces its 16 entries into a private top-2 of ONE query at once, so the distance matrix exists in registers only.
//   form A  integer descriptors 0..255 as fp16, v_mfma_f32_32x32x16_f16: every product and partial sum is an integer
//           below 2^24, so the fp32 accumulator, |b|^2 - 2 a.b (one fma) and the final integer d^2 are exact
//   form B  any fp32 descriptors, v_mfma_f32_32x32x2_f32 (an fp32 fma chain); norms and the combination in fp64; the two
//           winners' distances are then recomputed as sum (a - b)^2 in fp64
// Train rows are the MFMA's A operand (rows), queries its B operand (columns): accumulator register `reg` of lane l holds
// train row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) against query l & 31, so a lane meets the rows of its query in ascending
// order and a strict comparison keeps the lower index among equal distances; the two half-waves of a query are merged
// once, at the end, by (d^2, index).
//
// Operand slots.  Both MFMAs sum over "slots" (half-wave h, element j); which k a slot stands for is free as long as
// both operands agree.  A 16-byte piece at byte g * 32 + h * 16 of a row is what lane half h feeds to group g: eight
// fp16 values for one 32x32x16 MFMA, or four fp32 values for four 32x32x2 MFMAs.  The same addressing serves the
// queries (global memory -> registers, once per workgroup) and the train tile (LDS -> registers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

constexpr int MATCH_TQ = 128;            // queries per workgroup: four waves with 32 queries each
constexpr int MATCH_TT = 64;             // train rows per LDS tile: two 32-row MFMA blocks
constexpr int MATCH_MFMA_ROWS = 32;      // rows (and columns) of one MFMA block
constexpr int kMatchThreads = 256;
constexpr int kMatchRowBytes = 512;      // most bytes of a row in one LDS tile: 256 fp16 (all of form A) or 128 fp32 (one chunk)
constexpr int kMatchGroups = kMatchRowBytes / 32;
constexpr int kMatchPad = 16;            // bytes between two rows of the LDS tile (spreads the 16-byte reads of a column over the banks)
// rows come in NG groups of 32 bytes, NG one of these (the row is padded with zeros up to the next): the kernel is
// compiled once per NG, so that its MFMA chain is straight-line code over registers
#define MATCH_FOR_EACH_NG(X) X(1) X(2) X(4) X(8) X(12) X(16)
__host__ __device__ constexpr int match_pieces(int ng) { return (MATCH_TT * ng * 2 + kMatchThreads - 1) / kMatchThreads; }   // 16-byte pieces a thread stages per tile
constexpr int kMatchMaxDim = 512;
constexpr int kMatchNone = 0x7fffffff;   // index of an empty top-2 place

// one edge of the batch: first row of its query and train image in the descriptor set, their row counts, first query's
// place in the outputs
struct MatchEdge { long long qrow, trow, out; int nq, nt; };

// LDS of one workgroup: two tiles of MATCH_TT padded rows with their MATCH_TT norms (8 bytes each) behind them
__host__ __device__ inline size_t match_tile_bytes(int row_bytes) {
    return (size_t)MATCH_TT * (size_t)(row_bytes + kMatchPad) + (size_t)MATCH_TT * 8;
}

typedef _Float16 match_h8 __attribute__((ext_vector_type(8)));
typedef float match_f16 __attribute__((ext_vector_type(16)));

// float32 input: 1 -> *flag when a value is not an integer in 0..255 (every writer stores the same value)
__global__ __launch_bounds__(256) void k_match_check(const float* __restrict__ x, size_t n, int* __restrict__ flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        bad |= !(v >= 0.f && v <= 255.f && v == truncf(v));
    }
    if (bad) *flag = 1;
}

// One thread per descriptor: the row converted (fp16 / fp32) and padded with zeros to row_bytes, and its squared norm
// (form A: the exact integer as fp32; form B: fp64, summed in ascending k)
template <bool FB>
__global__ __launch_bounds__(256) void k_match_convert(const void* __restrict__ raw, int is_f32, size_t N, int D, int row_bytes,
                                                       unsigned char* __restrict__ rows, void* __restrict__ norms) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* rf = static_cast<const float*>(raw) + i * (size_t)D;
    const unsigned char* rb = static_cast<const unsigned char*>(raw) + i * (size_t)D;
    unsigned char* out = rows + i * (size_t)row_bytes;
    if (FB) {
        float* o = reinterpret_cast<float*>(out);
        const int Dp = row_bytes / 4;
        double s = 0.0;
        for (int k = 0; k < Dp; ++k) {
            const float v = k < D ? (is_f32 ? rf[k] : (float)rb[k]) : 0.f;
            o[k] = v;
            s += (double)v * (double)v;
        }
        static_cast<double*>(norms)[i] = s;
    } else {
        _Float16* o = reinterpret_cast<_Float16*>(out);
        const int Dp = row_bytes / 2;
        int s = 0;
        for (int k = 0; k < Dp; ++k) {
            const int v = k < D ? (is_f32 ? (int)rf[k] : (int)rb[k]) : 0;
            o[k] = (_Float16)(float)v;
            s += v * v;
        }
        static_cast<float*>(norms)[i] = (float)s;
    }
}

template <class T>
__device__ __forceinline__ bool match_less(T ka, int ia, T kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// (t, idx) into the sorted pair (k1, i1), (k2, i2) of a lane; candidates arrive in ascending idx, so `<` keeps the
// earlier one among equals.  A key that is not finite is no candidate.
template <class T>
__device__ __forceinline__ void match_insert(T t, int idx, bool ok, T& k1, int& i1, T& k2, int& i2) {
    const bool c2 = ok && t < k2 && t > -INFINITY;
    const bool c1 = c2 && t < k1;
    k2 = c1 ? k1 : (c2 ? t : k2);
    i2 = c1 ? i1 : (c2 ? idx : i2);
    k1 = c1 ? t : k1;
    i1 = c1 ? idx : i1;
}

// The 16 entries of one accumulator (train rows tile0 + rb * 32 + ..., this lane's query) into the lane's top-2.
// nrm: the tile's norms in LDS.  The whole wave skips the insertion when no lane has a candidate below its second place.
template <bool FB, class T>
__device__ __forceinline__ void match_reduce(const match_f16& acc, const unsigned char* nrm, int row0, int h, int nt,
                                             T& k1, int& i1, T& k2, int& i2) {
    T t[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rl = 8 * j + 4 * h;                            // first of this lane's four consecutive rows of group j
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int reg = 4 * j + c;
            if (FB) t[reg] = (T)fma(-2.0, (double)acc[reg], reinterpret_cast<const double*>(nrm)[rl + c]);
            else    t[reg] = (T)fmaf(-2.f, acc[reg], reinterpret_cast<const float*>(nrm)[rl + c]);
        }
    }
    T m = INFINITY;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) m = FB ? (T)fmin((double)m, (double)t[reg]) : (T)fminf((float)m, (float)t[reg]);   // (a NaN never becomes the minimum)
    if (!__any(m < k2)) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int idx = row0 + 8 * (reg >> 2) + 4 * h + (reg & 3);
        match_insert<T>(t[reg], idx, idx < nt, k1, i1, k2, i2);
    }
}

// grid: one workgroup per (edge, tile of MATCH_TQ queries) of `wgs`; dynamic LDS: 2 * match_tile_bytes(row_bytes).
// rows: the converted descriptors, n_chunk * row_bytes bytes each, row_bytes = 32 NG; a row is swept in n_chunk pieces of
// row_bytes (form A: always one).  Outputs per query: idx (2), dist (2), good.
template <bool FB, int NG>
__global__ __launch_bounds__(kMatchThreads) void k_match(const unsigned char* __restrict__ rows, const void* __restrict__ norms,
                                                        const MatchEdge* __restrict__ edges, const int2* __restrict__ wgs,
                                                        int n_chunk_arg, double ratio2, int* __restrict__ idx_out,
                                                        double* __restrict__ dist_out, unsigned char* __restrict__ good_out) {
    using T = typename std::conditional<FB, double, float>::type;
    extern __shared__ uint4 match_lds[];
    unsigned char* const lds = reinterpret_cast<unsigned char*>(match_lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int2 wg = wgs[blockIdx.x];
    const MatchEdge ed = edges[wg.x];
    const int q = wg.y + 32 * wave + r;                          // this lane's query, within its image
    const bool qok = q < ed.nq;
    constexpr int row_bytes = 32 * NG, lstride = row_bytes + kMatchPad, cpr = row_bytes >> 4;     // cpr: 16-byte pieces per row
    constexpr int kPieces = match_pieces(NG);
    const int n_chunk = FB ? n_chunk_arg : 1;
    const size_t gstride = (size_t)row_bytes * (size_t)n_chunk;
    const size_t tile_bytes = match_tile_bytes(row_bytes);
    const int n_tiles = (ed.nt + MATCH_TT - 1) / MATCH_TT;
    const int n_units = n_tiles * n_chunk;                       // a unit: one chunk of one tile

    // the pieces this thread stages of every unit: row in the tile and byte in the row
    int prow[kPieces], pcol[kPieces];
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
        const int c = tid + kMatchThreads * i;
        prow[i] = c / cpr;                                       // (>= MATCH_TT: no such piece at this row length)
        pcol[i] = (c - prow[i] * cpr) * 16;
    }
    const unsigned char* const tbase = rows + (size_t)ed.trow * gstride;
    const unsigned char* const qptr = rows + (size_t)(ed.qrow + (qok ? q : 0)) * gstride;

    uint4 st[kPieces];
    T stn = 0;
    uint4 bq[NG];
    match_f16 acc[2];
    T k1 = INFINITY, k2 = INFINITY;
    int i1 = kMatchNone, i2 = kMatchNone;

#define MATCH_GLOAD(u)                                                                                               \
    do {                                                                                                             \
        const int tile_ = (u) / n_chunk, ch_ = (u) - tile_ * n_chunk;                                                \
        _Pragma("unroll") for (int i = 0; i < kPieces; ++i) {                                                   \
            const int row_ = tile_ * MATCH_TT + prow[i];                                                             \
            st[i] = make_uint4(0, 0, 0, 0);                                                                          \
            if (prow[i] < MATCH_TT && row_ < ed.nt)                                                                  \
                st[i] = *reinterpret_cast<const uint4*>(tbase + (size_t)row_ * gstride + (size_t)ch_ * row_bytes + pcol[i]); \
        }                                                                                                            \
        stn = 0;                                                                                                     \
        if (tid < MATCH_TT && tile_ * MATCH_TT + tid < ed.nt)                                                        \
            stn = static_cast<const T*>(norms)[ed.trow + tile_ * MATCH_TT + tid];                                    \
    } while (0)
#define MATCH_LSTORE(buf)                                                                                            \
    do {                                                                                                             \
        unsigned char* const b_ = lds + (size_t)(buf) * tile_bytes;                                                  \
        _Pragma("unroll") for (int i = 0; i < kPieces; ++i)                                                     \
            if (prow[i] < MATCH_TT) *reinterpret_cast<uint4*>(b_ + prow[i] * lstride + pcol[i]) = st[i];            \
        if (tid < MATCH_TT) reinterpret_cast<T*>(b_ + MATCH_TT * lstride)[tid] = stn;                                \
    } while (0)

#pragma unroll
    for (int g = 0; g < NG; ++g) {
        bq[g] = make_uint4(0, 0, 0, 0);
        if (qok) bq[g] = *reinterpret_cast<const uint4*>(qptr + g * 32 + h * 16);
    }
    MATCH_GLOAD(0);
    MATCH_LSTORE(0);
    __syncthreads();
    for (int u = 0; u < n_units; ++u) {
        const int tile = u / n_chunk, ch = u - tile * n_chunk;
        if (u + 1 < n_units) MATCH_GLOAD(u + 1);
        if (ch == 0) {
#pragma unroll
            for (int k = 0; k < 16; ++k) { acc[0][k] = 0.f; acc[1][k] = 0.f; }
        }
        if (n_chunk > 1) {                                       // the query's pieces of this chunk (one chunk: loaded once, above)
#pragma unroll
            for (int g = 0; g < NG; ++g)
                if (qok) bq[g] = *reinterpret_cast<const uint4*>(qptr + (size_t)ch * row_bytes + g * 32 + h * 16);
        }
        const unsigned char* const buf = lds + (size_t)(u & 1) * tile_bytes;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            {
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    const uint4 a = *reinterpret_cast<const uint4*>(buf + (rb * 32 + r) * lstride + g * 32 + h * 16);
                    if (FB) {
                        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(bq[g].x), acc[rb], 0, 0, 0);
                        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(bq[g].y), acc[rb], 0, 0, 0);
                        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(bq[g].z), acc[rb], 0, 0, 0);
                        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(bq[g].w), acc[rb], 0, 0, 0);
                    } else {
                        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(match_h8, a),
                                                                         __builtin_bit_cast(match_h8, bq[g]), acc[rb], 0, 0, 0);
                    }
                }
            }
        }
        if (ch == n_chunk - 1) {
            const unsigned char* const nrm = buf + MATCH_TT * lstride;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                match_reduce<FB, T>(acc[rb], nrm + rb * 32 * sizeof(T), tile * MATCH_TT + rb * 32, h, ed.nt, k1, i1, k2, i2);
        }
        if (u + 1 < n_units) MATCH_LSTORE((u + 1) & 1);
        __syncthreads();
    }
#undef MATCH_GLOAD
#undef MATCH_LSTORE

    // the two half-waves of a query, merged by (key, index); both halves end with the same pair
    {
        const T ok1 = __shfl_xor(k1, 32), ok2 = __shfl_xor(k2, 32);
        const int oi1 = __shfl_xor(i1, 32), oi2 = __shfl_xor(i2, 32);
        T f, s;
        int fi, si;
        if (match_less<T>(k1, i1, ok1, oi1)) {
            f = k1; fi = i1;
            const bool own = match_less<T>(k2, i2, ok1, oi1);
            s = own ? k2 : ok1; si = own ? i2 : oi1;
        } else {
            f = ok1; fi = oi1;
            const bool oth = match_less<T>(ok2, oi2, k1, i1);
            s = oth ? ok2 : k1; si = oth ? oi2 : i1;
        }
        k1 = f; i1 = fi; k2 = s; i2 = si;
    }

    double d1, d2;
    if (FB) {
        // half-wave h recomputes winner h directly: sum (a - b)^2 in fp64 over the fp32 values, ascending k
        const int w = h ? i2 : i1;
        double d = INFINITY;
        if (qok && w != kMatchNone) {
            const float4* a = reinterpret_cast<const float4*>(qptr);
            const float4* b = reinterpret_cast<const float4*>(tbase + (size_t)w * gstride);
            d = 0.0;
            for (int k = 0; k < (int)(gstride >> 4); ++k) {
                const float4 x = a[k], y = b[k];
                const double e0 = (double)x.x - (double)y.x, e1 = (double)x.y - (double)y.y;
                const double e2 = (double)x.z - (double)y.z, e3 = (double)x.w - (double)y.w;
                d = fma(e0, e0, d); d = fma(e1, e1, d); d = fma(e2, e2, d); d = fma(e3, e3, d);
            }
        }
        const double other = __shfl_xor(d, 32);
        d1 = d; d2 = other;                                      // (as half-wave 0 sees them; only it writes)
        if (!(fabs(d1) < INFINITY)) { d1 = d2; i1 = i2; d2 = INFINITY; i2 = kMatchNone; }
        if (!(fabs(d2) < INFINITY)) { d2 = INFINITY; i2 = kMatchNone; }
        if (!(fabs(d1) < INFINITY)) { d1 = INFINITY; i1 = kMatchNone; }
        if (i2 != kMatchNone && match_less<double>(d2, i2, d1, i1)) {
            const double td = d1; d1 = d2; d2 = td;
            const int ti = i1; i1 = i2; i2 = ti;
        }
    } else {
        // |a|^2 + (|b|^2 - 2 a.b): integers below 2^25 in magnitude, exact
        const int an = qok ? (int)static_cast<const float*>(norms)[ed.qrow + q] : 0;
        d1 = i1 != kMatchNone ? (double)(an + (int)k1) : (double)INFINITY;
        d2 = i2 != kMatchNone ? (double)(an + (int)k2) : (double)INFINITY;
    }
    if (h == 0 && qok) {
        const size_t o = (size_t)ed.out + (size_t)q;
        const bool both = i1 != kMatchNone && i2 != kMatchNone;
        *reinterpret_cast<int2*>(idx_out + 2 * o) = make_int2(i1 != kMatchNone ? i1 : -1, i2 != kMatchNone ? i2 : -1);
        *reinterpret_cast<double2*>(dist_out + 2 * o) = make_double2(d1, d2);
        good_out[o] = both && d1 < ratio2 * d2 ? 1 : 0;
    }
}
