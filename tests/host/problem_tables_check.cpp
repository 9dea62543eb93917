// problem_tables_check -- runs the table build of sfmba_set_problem (csrc/problem_tables.hpp) without a device, so that
// it can be compiled with the host sanitizers.  Usage: problem_tables_check CASES OUT
//
// CASES (int64 words): the number of calls, then per call
//   C P N n_fixed uv_is_int64 f32 | dense xcd_b cm_device packed_upload cam_chunk_len total_waves parts pair_parts
//   cam[N] pt[N] uv[2 N] (double or int64) fixed[n_fixed]
// The calls run in order on ONE set of staged arrays, as consecutive sfmba_set_problem calls on a handle do: a call is
// compared with what the call before it left.  Every staged array is reallocated at exactly the size the library asks
// for, filled with a pattern, and given the prefix the library would keep: a write past an end is the sanitizer's to see,
// an entry the build forgets to write shows in the output.
// OUT, per call: ok bad sorted fdiff pixels_int16 cam_multi pair_entries ld, then (ok only) every array as its length and
// its elements: ptr perm order cam_ptr ranges wsteps steps chunks chunk_ptr chunks_b chunk_ptr_b cov_ptr cov_pt blk_ab
// ci pi uvs uvf ci16 uv16.
#include <cstdio>
#include <cstring>

#include "problem_tables.hpp"

using namespace sfmba;

namespace {

template <class T>
void regrow(std::vector<T>& v, size_t n, size_t keep) {
    std::vector<T> q(n);
    if (n) memset(q.data(), 0x5a, sizeof(T) * n);
    std::copy(v.begin(), v.begin() + (ptrdiff_t)std::min(std::min(keep, n), v.size()), q.begin());
    v.swap(q);
}

template <class T>
std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}

template <class T>
void put(FILE* f, const T* p, size_t n) {
    const int64_t len = (int64_t)n;
    fwrite(&len, sizeof len, 1, f);
    if (n) fwrite(p, sizeof(T), n, f);
}
template <class T>
void put(FILE* f, const std::vector<T>& v) { put(f, v.data(), v.size()); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CASES OUT\n", argv[0]); return 2; }
    FILE* fin = fopen(argv[1], "rb");
    FILE* fout = fopen(argv[2], "wb");
    if (!fin || !fout) { fprintf(stderr, "cannot open the files\n"); return 2; }
    HostPool pool;
    ProblemTables tb;
    std::vector<int> ci, pi, perm, ptr;
    std::vector<double> uvs;
    std::vector<float> uvf;
    std::vector<unsigned short> ci16;
    std::vector<short> uv16;
    struct { bool valid = false, f32 = false, packed = false; int64_t N = 0; } prev;     // as sfmba_handle::Prev

    const int64_t n_calls = take<int64_t>(fin, 1)[0];
    for (int64_t call = 0; call < n_calls; ++call) {
        const std::vector<int64_t> hd = take<int64_t>(fin, 14);
        const int64_t C = hd[0], P = hd[1], N = hd[2], n_fixed = hd[3];
        const bool uv_i64 = hd[4] != 0, f32 = hd[5] != 0;
        TablePlan plan;
        plan.dense = hd[6] != 0; plan.xcd_b = hd[7] != 0; plan.cm_device = hd[8] != 0; plan.packed_upload = hd[9] != 0;
        plan.cam_chunk_len = hd[10]; plan.total_waves = hd[11]; plan.parts = (int)hd[12]; plan.pair_parts = (int)hd[13];
        const std::vector<int64_t> cam = take<int64_t>(fin, (size_t)N), pt = take<int64_t>(fin, (size_t)N);
        const std::vector<double> uvd = take<double>(fin, uv_i64 ? 0 : 2 * (size_t)N);
        const std::vector<int64_t> uvi = take<int64_t>(fin, uv_i64 ? 2 * (size_t)N : 0);
        std::vector<char> fixed((size_t)C, 0);
        for (int64_t c : take<int64_t>(fin, (size_t)n_fixed)) fixed[(size_t)c] = 1;

        // the staging, as ProblemBuild::stage_and_build sizes and keeps it
        const size_t ld = ((size_t)N + 255) / 256 * 256;
        const int64_t n_cmp = (prev.valid && prev.f32 == f32) ? std::min(prev.N, N) : 0;
        prev.valid = false;
        const size_t keep = (size_t)n_cmp;
        regrow(uvs, 2 * ld, 2 * keep); regrow(ci, ld, keep); regrow(pi, ld, keep);
        regrow(perm, ld, 0); regrow(ptr, (size_t)P + 1, 0);
        if (f32) regrow(uvf, 2 * ld, 2 * keep);
        if (plan.packed_upload) { regrow(ci16, ld, keep); regrow(uv16, 2 * ld, 2 * keep); }
        StagedArrays st;
        st.ci = ci.data(); st.pi = pi.data(); st.uvs = uvs.data(); st.perm = perm.data(); st.ptr = ptr.data();
        st.uvf = f32 ? uvf.data() : nullptr;
        st.ci16 = plan.packed_upload ? ci16.data() : nullptr;
        st.uv16 = plan.packed_upload ? uv16.data() : nullptr;
        ProblemInput in;
        in.C = C; in.P = P; in.N = N; in.cam = cam.data(); in.pt = pt.data();
        in.uv = uv_i64 ? nullptr : uvd.data(); in.uv_i64 = uv_i64 ? uvi.data() : nullptr;
        in.fixed = fixed.data();
        in.n_cmp = n_cmp;
        in.packed_prefix_ok = plan.packed_upload && prev.packed && n_cmp > 0;

        const bool ok = build_problem_tables(in, plan, st, pool, tb);
        const int64_t head[8] = {ok, tb.bad, tb.sorted, tb.fdiff, tb.facts.pixels_int16, tb.facts.cam_multi,
                                 tb.facts.pair_entries, (int64_t)ld};
        fwrite(head, sizeof head, 1, fout);
        if (!ok) continue;
        put(fout, ptr);
        put(fout, perm.data(), plan.cm_device ? 0 : ld);
        put(fout, tb.order);
        put(fout, tb.cam_ptr);
        put(fout, reinterpret_cast<const int*>(tb.ranges.data()), 2 * tb.ranges.size());
        put(fout, reinterpret_cast<const int*>(tb.wsteps.data()), 2 * tb.wsteps.size());
        put(fout, reinterpret_cast<const int*>(tb.steps.data()), 2 * tb.steps.size());
        put(fout, reinterpret_cast<const int*>(tb.chunks.data()), 4 * tb.chunks.size());
        put(fout, tb.chunk_ptr);
        put(fout, reinterpret_cast<const int*>(tb.chunks_b.data()), 4 * tb.chunks_b.size());
        put(fout, tb.chunk_ptr_b);
        put(fout, tb.cov_ptr);
        put(fout, tb.cov_pt);
        put(fout, reinterpret_cast<const int*>(tb.blk_ab.data()), 2 * tb.blk_ab.size());
        put(fout, ci); put(fout, pi); put(fout, uvs);
        put(fout, uvf.data(), f32 ? 2 * ld : 0);
        put(fout, ci16.data(), plan.packed_upload ? ld : 0);
        put(fout, uv16.data(), plan.packed_upload ? 2 * ld : 0);
        // what the end of a sfmba_set_problem call records for the next one (the final packed_upload: planned, and the pixels allow it)
        if (tb.sorted) { prev.valid = true; prev.f32 = f32; prev.N = N; }
        prev.packed = tb.sorted && plan.packed_upload && tb.facts.pixels_int16;
    }
    fclose(fin);
    return fclose(fout) == 0 ? 0 : 2;
}
