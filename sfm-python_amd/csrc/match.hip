// match.hip -- host code of descriptor matching (kernels: match_kernels.hpp).  Nothing of it needs a problem.
#include "handle.hpp"
#include "match_kernels.hpp"

namespace {
void match_release(sfmba_handle* h) {
    auto& m = h->match;
    for (DevBuf* b : {&m.raw, &m.rows[0], &m.rows[1], &m.norms[0], &m.norms[1]}) b->release();
    m.have[0] = m.have[1] = false;
    m.form = 0;
    m.img_ptr.clear();
}

template <bool FB, int NG>
int match_launch(sfmba_handle* h, size_t n_wg, int f, double ratio2) {
    auto& m = h->match;
    const size_t lds = 2 * match_tile_bytes(32 * NG);
    if (lds > 65536) CHK(opt_in_lds(h, reinterpret_cast<const void*>(k_match<FB, NG>), lds));
    hipLaunchKernelGGL((k_match<FB, NG>), dim3((unsigned)n_wg), dim3(kMatchThreads), lds, h->stream,
                       (const unsigned char*)m.rows[f].as<unsigned char>(), (const void*)m.norms[f].p,
                       (const MatchEdge*)m.edges.as<MatchEdge>(), (const int2*)m.wgs.as<int2>(), m.n_chunk[f], ratio2,
                       m.idx.as<int>(), m.dist.as<double>(), m.good.as<unsigned char>());
    LAUNCHED(h);
    return 0;
}

// the set in form f (0 = A, 1 = B) from the raw array on the device
int match_convert(sfmba_handle* h, int f) {
    auto& m = h->match;
    if (m.have[f]) return 0;
    const size_t N = (size_t)m.img_ptr.back();
    const int D = m.dim;
    const int bytes = (f == 0 ? 2 : 4) * D;                      // of a row; in 32-byte groups, their number one the kernel is built for
    int ng = kMatchGroups;
#define X(n) if (32 * n >= bytes && n < ng) ng = n;
    MATCH_FOR_EACH_NG(X)
#undef X
    m.row_bytes[f] = 32 * ng;
    m.n_chunk[f] = (bytes + kMatchRowBytes - 1) / kMatchRowBytes;      // (more than one: form B beyond 128 values, full rows)
    const size_t stride = (size_t)m.row_bytes[f] * (size_t)m.n_chunk[f];
    CHK(ensure_all(h, {{&m.rows[f], std::max<size_t>(stride * N, 16)}, {&m.norms[f], std::max<size_t>(8 * N, 16)}}));
    if (N) {
        const unsigned grid = (unsigned)((N + 255) / 256);
        if (f == 0)
            hipLaunchKernelGGL(k_match_convert<false>, dim3(grid), dim3(256), 0, h->stream, (const void*)m.raw.p, m.dtype, N, D,
                               (int)stride, m.rows[0].as<unsigned char>(), m.norms[0].p);
        else
            hipLaunchKernelGGL(k_match_convert<true>, dim3(grid), dim3(256), 0, h->stream, (const void*)m.raw.p, m.dtype, N, D,
                               (int)stride, m.rows[1].as<unsigned char>(), m.norms[1].p);
        LAUNCHED(h);
    }
    m.have[f] = true;
    return 0;
}
}  // namespace

int sfmba_set_descriptors(sfmba_handle* h, int64_t n_images, const int64_t* img_ptr, const void* desc, int32_t dtype,
                          int32_t dim, int32_t* form_out) {
    CHK(enter(h));
    if (n_images < 0 || !img_ptr) return fail(h, -1, "sfmba_set_descriptors: n_images is negative or img_ptr is NULL");
    if (n_images >= ((int64_t)1 << 31)) return fail(h, -1, "sfmba_set_descriptors: too many images");
    if (dim < 1 || dim > kMatchMaxDim) return fail(h, -1, "sfmba_set_descriptors: dim must be 1..%d, got %d", kMatchMaxDim, (int)dim);
    if (dtype != 0 && dtype != 1) return fail(h, -1, "sfmba_set_descriptors: dtype must be 0 (uint8) or 1 (float32)");
    if (img_ptr[0] != 0) return fail(h, -1, "sfmba_set_descriptors: img_ptr[0] must be 0");
    for (int64_t i = 0; i < n_images; ++i) {
        if (img_ptr[i + 1] < img_ptr[i]) return fail(h, -1, "sfmba_set_descriptors: img_ptr must ascend (image %lld)", (long long)i);
        if (img_ptr[i + 1] - img_ptr[i] >= ((int64_t)1 << 30))
            return fail(h, -1, "sfmba_set_descriptors: image %lld has 2^30 descriptors or more", (long long)i);
    }
    const size_t N = (size_t)img_ptr[n_images];
    if (N && !desc) return fail(h, -1, "sfmba_set_descriptors: desc is NULL");
    auto& m = h->match;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    match_release(h);
    m.img_ptr.assign(img_ptr, img_ptr + n_images + 1);
    m.dim = dim; m.dtype = dtype;
    const size_t raw_bytes = N * (size_t)dim * (dtype ? 4 : 1);
    CHK(ensure_all(h, {{&m.raw, std::max<size_t>(raw_bytes, 16)}, {&m.flag, sizeof(int)}}));
    if (raw_bytes) HIPCHK(h, hipMemcpyAsync(m.raw.p, desc, raw_bytes, hipMemcpyHostToDevice, h->stream));
    // form A: integers 0..255 whose padded row fits one LDS row of fp16
    bool integer = dim <= kMatchRowBytes / 2;
    if (integer && dtype == 1 && N) {
        int flag = 0;
        HIPCHK(h, hipMemsetAsync(m.flag.p, 0, sizeof(int), h->stream));
        const size_t n = N * (size_t)dim;
        const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)h->n_cu * 8);
        hipLaunchKernelGGL(k_match_check, dim3(grid), dim3(256), 0, h->stream, (const float*)m.raw.as<float>(), n, m.flag.as<int>());
        LAUNCHED(h);
        HIPCHK(h, hipMemcpyAsync(&flag, m.flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        integer = flag == 0;
    }
    m.form = integer ? 1 : 2;
    const int rc = match_convert(h, m.form - 1);
    if (rc != 0) { match_release(h); return rc; }
    const int rw = wait_stream(h);
    if (rw != 0) { match_release(h); return rw; }
    if (form_out) *form_out = m.form;
    return 0;
}

void sfmba_default_match_options(sfmba_match_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->ratio = 0.5; o->form = 0; o->profile = 0;
}

int sfmba_match_descriptors(sfmba_handle* h, int64_t n_edges, const int32_t* edges, const sfmba_match_options* opt,
                            int64_t* query_ptr, int32_t* idx, double* dist_sq, uint8_t* good, int32_t* edge_good,
                            int32_t* edge_status, int64_t* n_ok, double* kernel_us) {
    CHK(enter(h));
    sfmba_match_options o;
    if (opt) o = *opt; else sfmba_default_match_options(&o);
    if (!(o.ratio > 0.0)) return fail(h, -1, "sfmba_match_descriptors: ratio must be positive, got %g", o.ratio);
    if (o.form < 0 || o.form > 2) return fail(h, -1, "sfmba_match_descriptors: form must be 0, 1 or 2");
    auto& m = h->match;
    if (!m.form) return fail(h, -1, "sfmba_match_descriptors: call sfmba_set_descriptors first");
    if (n_edges < 0 || (n_edges && !edges)) return fail(h, -1, "sfmba_match_descriptors: n_edges is negative or edges is NULL");
    if (o.form == 1 && m.form != 1)
        return fail(h, -1, "sfmba_match_descriptors: form A asked for, but the descriptors are not integers 0..255 of dim <= %d",
                    kMatchRowBytes / 2);
    const int f = o.form == 2 ? 1 : m.form - 1;
    const int64_t n_images = (int64_t)m.img_ptr.size() - 1;
    const size_t E = (size_t)n_edges;
    if (n_ok) *n_ok = 0;
    if (kernel_us) *kernel_us = 0.0;
    std::vector<MatchEdge> ed(E);
    std::vector<int2> wgs;
    std::vector<int32_t> status(E);
    size_t Q = 0;
    for (size_t e = 0; e < E; ++e) {
        const int64_t u = edges[2 * e], v = edges[2 * e + 1];
        if (u < 0 || u >= n_images || v < 0 || v >= n_images)
            return fail(h, -1, "sfmba_match_descriptors: edge %zu names image %lld, the set has %lld", e,
                        (long long)(u < 0 || u >= n_images ? u : v), (long long)n_images);
        MatchEdge& d = ed[e];
        d.qrow = m.img_ptr[u]; d.trow = m.img_ptr[v]; d.out = (long long)Q;
        d.nq = (int)(m.img_ptr[u + 1] - m.img_ptr[u]); d.nt = (int)(m.img_ptr[v + 1] - m.img_ptr[v]);
        status[e] = d.nq < 1 || d.nt < 2 ? 1 : 0;
        if (query_ptr) query_ptr[e] = (int64_t)Q;
        if (!status[e])
            for (int q0 = 0; q0 < d.nq; q0 += MATCH_TQ) wgs.push_back(make_int2((int)e, q0));
        Q += (size_t)d.nq;
    }
    if (query_ptr) query_ptr[E] = (int64_t)Q;
    if (Q >= (size_t)1 << 30 || wgs.size() >= (size_t)1 << 31)
        return fail(h, -1, "sfmba_match_descriptors: the batch has 2^30 queries or more");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    CHK(match_convert(h, f));
    if (!wgs.empty()) {
        CHK(ensure_all(h, {{&m.edges, sizeof(MatchEdge) * E}, {&m.wgs, sizeof(int2) * wgs.size()}, {&m.idx, sizeof(int) * 2 * Q},
                           {&m.dist, sizeof(double) * 2 * Q}, {&m.good, Q}}));
        HIPCHK(h, hipMemcpyAsync(m.edges.p, ed.data(), sizeof(MatchEdge) * E, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(m.wgs.p, wgs.data(), sizeof(int2) * wgs.size(), hipMemcpyHostToDevice, h->stream));
        const double ratio2 = o.ratio * o.ratio;
        EventPair timer;
        CHK(timer.start(h, o.profile != 0));
        switch ((f ? 100 : 0) + m.row_bytes[f] / 32) {
#define X(n) case n: CHK((match_launch<false, n>(h, wgs.size(), f, ratio2))); break; \
             case 100 + n: CHK((match_launch<true, n>(h, wgs.size(), f, ratio2))); break;
            MATCH_FOR_EACH_NG(X)
#undef X
            default: return fail(h, -3, "sfmba_match_descriptors: no kernel for rows of %d bytes", m.row_bytes[f]);
        }
        CHK(timer.stop(h));
        if (!good && edge_good) m.good_host.resize(Q);
        HIPCHK(h, download(h, idx, m.idx.p, sizeof(int) * 2 * Q));
        HIPCHK(h, download(h, dist_sq, m.dist.p, sizeof(double) * 2 * Q));
        HIPCHK(h, download(h, good ? good : (edge_good ? m.good_host.data() : nullptr), m.good.p, Q));
        CHK(wait_stream(h));
        CHK(timer.read(h, kernel_us));
    }
    // edges with too few rows: the device wrote nothing of theirs
    const unsigned char* gsrc = good ? good : m.good_host.data();
    int64_t ok = 0;
    for (size_t e = 0; e < E; ++e) {
        const size_t b = (size_t)ed[e].out, n = (size_t)ed[e].nq;
        if (status[e]) {
            if (idx) std::fill(idx + 2 * b, idx + 2 * (b + n), -1);
            if (dist_sq) std::fill(dist_sq + 2 * b, dist_sq + 2 * (b + n), (double)INFINITY);
            if (good) std::fill(good + b, good + b + n, (uint8_t)0);
        }
        if (edge_good) {
            int32_t c = 0;
            if (!status[e]) for (size_t k = b; k < b + n; ++k) c += gsrc[k] ? 1 : 0;
            edge_good[e] = c;
        }
        if (edge_status) edge_status[e] = status[e];
        ok += status[e] == 0 ? 1 : 0;
    }
    if (n_ok) *n_ok = ok;
    return 0;
}
