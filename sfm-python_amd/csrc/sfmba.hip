// sfmba.hip -- C-ABI (include/sfmba.h) and the host controller of the MI355X bundle-adjustment path.
//
// The controller restates scipy's trf_no_bounds (SCIPY/optimize/_lsq/trf.py:401-560, the code behind
// the least_squares(method='trf', x_scale='jac') call of /root/reference/sfm_lite/sfm.py:266-268):
// same scaling, same 1-D Cauchy regularisation, same 2-D subspace trust-region step, same radius
// update and termination tests.  Two things differ by design: the Jacobian is analytic (K1) instead
// of forward-differenced, and the damped Gauss-Newton step of trf.py:480 is obtained from the Schur
// complement on the cameras with block-Jacobi PCG (K4-K6) instead of LSMR on the full system.
// Only scalars and 2x2 systems are handled on the host; every n- or m-vector stays in HBM.
#include "handle.hpp"

#include <hip/hip_ext.h>
#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "ba_kernels.hpp"

namespace {
// Scalars at the end of the exchange arena (32 doubles):
//   summed over ranks [0..11]: 0 sum r^2 | 1 G11 | 2 G12 | 3 G22 | 4..7 q5..q8 | 8..11 q1..q4 of the point
//                              slice (grouped so that each phase all-reduces one contiguous run of fresh values)
//   max over ranks    [12]   : q0 = max|g| of the point slice
//   device-local      [13]   : regularisation term of this iteration (k_prep)
//                     [14,15]: |g_h|^2 of the previous iterate, forcing term of this iteration's PCG (k_prep)
//   never exchanged   [16..24]: q0..q8 of the camera slice (replicated on every rank)
constexpr int kScalSlots = 32;
// Per-workgroup partial sums live in two halves of one buffer: A (k_update_scale, the cost of
// k_resjac) and B (k_jdot, k_backsub).  Consecutive producers alternate halves, so the final sums of one
// producer can ride along with the NEXT producer's launch (Piggyback) without a race on the rows.
constexpr int kPartRows = 2048;
//   written by k_tr_step [25..31]: c1, c2, predicted reduction, |step_h|, |step| of the step it chose; its verdict
//                              (non-zero: the trial launches behind it are void); the radius it used
constexpr int kCostSlot = 0, kG11Slot = 1, kTailSlot = 2, kQ1Slot = 8;      // sum r^2 | G11 | G12, G22, q5..q8 | q1..q4
constexpr int kMaxSlot = 12, kRegSlot = 13, kGhPrevSlot = 14, kEtaSlot = 15, kCamSlot = 16;
constexpr int kStepSlot = 25, kSkipSlot = 30, kRadiusSlot = 31;
// the pinned block h_scal (64 doubles): the scalars, then staging for small read-backs
constexpr int kPinCtrl = 40;             // a PcgCtrl (pcg_read)
constexpr int kPinP2pErr = 62;           // the error word of the direct link at the end of a solve
constexpr int kPointSlot[9] = {12, 8, 9, 10, 11, 4, 5, 6, 7};     // slot of q0..q8 of the point slice

// RCCL entry points, resolved at run time so that libsfmba.so has no load-time dependency on RCCL
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi* rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (lib) {
            api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
            api.CommInitRank = (decltype(api.CommInitRank))dlsym(lib, "ncclCommInitRank");
            api.AllReduce = (decltype(api.AllReduce))dlsym(lib, "ncclAllReduce");
            api.CommDestroy = (decltype(api.CommDestroy))dlsym(lib, "ncclCommDestroy");
            api.GetErrorString = (decltype(api.GetErrorString))dlsym(lib, "ncclGetErrorString");
            if (api.GetUniqueId && api.CommInitRank && api.AllReduce && api.CommDestroy && api.GetErrorString)
                api.lib = lib;
        }
    }
    return api.lib ? &api : nullptr;
}

// name -> member, from the same list: an option cannot exist without a setter
const struct { const char* name; int Debug::*member; } kDebugOptions[] = {
#define X(name, init) {#name, &Debug::name},
    SFMBA_DEBUG_OPTIONS(X)
#undef X
};
void decide_solve_forms(sfmba_handle* h);           // (defined with its table, below)

}  // namespace

// the rows of the host's tables are uploaded as they are
static_assert(sizeof(TableRow2) == sizeof(int2) && alignof(TableRow2) == alignof(int2) && offsetof(TableRow2, x) == offsetof(int2, x) &&
              offsetof(TableRow2, y) == offsetof(int2, y), "TableRow2 is int2");
static_assert(sizeof(TableRow4) == sizeof(int4) && alignof(TableRow4) == alignof(int4) && offsetof(TableRow4, x) == offsetof(int4, x) &&
              offsetof(TableRow4, y) == offsetof(int4, y) && offsetof(TableRow4, z) == offsetof(int4, z) &&
              offsetof(TableRow4, w) == offsetof(int4, w), "TableRow4 is int4");

namespace sfmba {
constexpr size_t kLdsBytes = 160 * 1024;       // gfx950: 160 KiB LDS per workgroup
const size_t kLdsDynMax = kLdsBytes - 2048;     // dynamic part; every kernel that asks for it has <= 2 KiB static LDS (k_backsub: 1280 B); k_tri_ransac (3152 B) asks for less: launch_tri_ransac
const int kRecStride = kRec, kVinvStride = kVinvRow;

int fail(sfmba_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

int ensure_all(sfmba_handle* h, std::initializer_list<SizedBuf> sized) {
    for (const auto& b : sized)
        if (b.bytes) HIPCHK(h, b.buf->ensure(b.bytes));
    return 0;
}

int enter(sfmba_handle* h) {
    if (!h) return -1;
    h->err.clear();
    HIPCHK(h, hipSetDevice(h->device));
    return 0;
}

int opt_in_lds(sfmba_handle* h, const void* kernel, size_t bytes) {
    if (std::find(h->lds_ready.begin(), h->lds_ready.end(), kernel) != h->lds_ready.end()) return 0;
    HIPCHK(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    h->lds_ready.push_back(kernel);
    return 0;
}

int launch_k_cam_table(sfmba_handle* h, const double* x, double* tab) {
    hipLaunchKernelGGL(k_cam_table, dim3((unsigned)((h->C + 255) / 256)), dim3(256), 0, h->stream, x, (int)h->C, h->K, tab);
    LAUNCHED(h);
    return 0;
}
// the first two launches of the counting sort by camera (see k_cam_hist): sfmba_set_problem's and the statistics' own
int launch_k_cam_hist(sfmba_handle* h, const unsigned char* fixed, int B, int per_slice, int* hist) {
    const size_t lds = sizeof(int) * (size_t)h->C;
    CHK(set_lds(h, k_cam_hist, lds));
    hipLaunchKernelGGL(k_cam_hist, dim3(B), dim3(64), lds, h->stream, (const int*)h->cam_idx.as<int>(), fixed, (int)h->N, (int)h->C,
                       per_slice, hist);
    LAUNCHED(h);
    return 0;
}
int launch_k_schur_blocks(sfmba_handle* h, const double* tab, const double* rec, const double* Vinv, double* Sblk) {
    hipLaunchKernelGGL(k_schur_blocks, dim3(h->n_blk), dim3(kCamThreads), 0, h->stream, (const int*)h->cov_ptr.as<int>(),
                       (const int*)h->cov_pt.as<int>(), (const int2*)h->blk_ab.as<int2>(), tab, rec, Vinv, h->K, (int)h->C, Sblk,
                       (double*)nullptr);
    LAUNCHED(h);
    return 0;
}
int launch_k_cam_offsets(sfmba_handle* h, const int* hist, const int* cam_ptr, int B, int* off) {
    hipLaunchKernelGGL(k_cam_offsets, dim3((unsigned)((h->C + 255) / 256)), dim3(256), 0, h->stream, hist, cam_ptr, B, (int)h->C, off);
    LAUNCHED(h);
    return 0;
}

// `reps` back-to-back calls of `launch` on the handle's stream between two events -> average microseconds of one
int time_reps(sfmba_handle* h, int32_t reps, double* avg_us, const std::function<int()>& launch) {
    EventPair ev;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    CHK(ev.start(h, true));
    for (int k = 0; k < reps; ++k) CHK(launch());
    CHK(ev.stop(h));
    HIPCHK(h, hipEventSynchronize(ev.b));
    CHK(ev.read(h, avg_us));
    *avg_us /= reps;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// Host/device hand-off: poll the stream instead of sleeping in hipStreamSynchronize.  The solver
// hands control back to the host two to three times per outer iteration for ~30 us of GPU work each;
// a blocking wait that parks the thread costs up to a millisecond per wake-up on an idle host.
static void report_stall(const sfmba_handle* h, const char* where, double seconds) {   // trace_stalls: waits longer than 2 ms
    if (h->dbg.trace_stalls && seconds > 2e-3) fprintf(stderr, "sfmba: waited %.2f ms in %s\n", 1e3 * seconds, where);
}
// `ev` null: the handle's stream; else one event of the copy stream
int wait_stream(sfmba_handle* h, hipEvent_t ev) {
    const char* what = ev ? "hipEventQuery" : "hipStreamQuery";
    const double t0 = now_s();
    for (;;) {
        const hipError_t e = ev ? hipEventQuery(ev) : hipStreamQuery(h->stream);
        if (e == hipSuccess) { report_stall(h, ev ? "wait_event" : "wait_stream", now_s() - t0); return 0; }
        if (e != hipErrorNotReady) return fail(h, -3, "%s failed: %s", what, hipGetErrorString(e));
        if (now_s() - t0 > 0.05) break;          // long wait: stop burning the core
    }
    if (ev) HIPCHK(h, hipEventSynchronize(ev));
    else HIPCHK(h, hipStreamSynchronize(h->stream));
    report_stall(h, ev ? "wait_event (blocking)" : "wait_stream (blocking)", now_s() - t0);
    return 0;
}

// x crosses PCIe through a pinned staging buffer (an async copy from pageable memory is staged by the
// runtime anyway, synchronously and in small pieces)
static int ensure_h_x(sfmba_handle* h) {
    const size_t need = (size_t)std::max<int64_t>(h->n, 2 * h->N);      // also stages the residual vector
    if (h->h_x && h->h_x_doubles >= need) return 0;
    if (h->h_x) { (void)hipHostFree(h->h_x); h->h_x = nullptr; h->h_x_doubles = 0; }
    HIPCHK(h, hipHostMalloc((void**)&h->h_x, sizeof(double) * need, hipHostMallocDefault));
    h->h_x_doubles = need;
    return 0;
}

// pageable <-> pinned copy of a parameter vector: a few host threads from 1 MB on (one thread moves 2.4 MB in 85-115 us,
// which was 9 % of a solve at 306k parameters).  `chunk_done(k, offset, bytes)` (optional) is called on the calling
// thread, in chunk order, as soon as chunk k has arrived: the upload enqueues that chunk's DMA while the others are
// still being copied.
template <class Fn>
static void staging_copy(sfmba_handle* h, void* dst, const void* src, size_t bytes, Fn chunk_done) {
    const int parts = (int)std::min<size_t>(4, bytes >> 19);
    if (parts <= 1) { memcpy(dst, src, bytes); chunk_done(0, (size_t)0, bytes); return; }
    const size_t per = ((bytes + parts - 1) / parts + 63) & ~(size_t)63;
    std::atomic<int> done[8];
    for (auto& d : done) d.store(0, std::memory_order_relaxed);
    h->pool.run(parts, [&](int t) {
        const size_t b = std::min(bytes, (size_t)t * per), e = std::min(bytes, b + per);
        if (e > b) memcpy(static_cast<char*>(dst) + b, static_cast<const char*>(src) + b, e - b);
        if (t != 0) { done[t].store(1, std::memory_order_release); return; }
        chunk_done(0, b, e - b);
        for (int k = 1; k < parts; ++k) {
            while (done[k].load(std::memory_order_acquire) == 0) { }
            const size_t bk = std::min(bytes, (size_t)k * per), ek = std::min(bytes, bk + per);
            chunk_done(k, bk, ek - bk);
        }
    });
}
static void staging_copy(sfmba_handle* h, void* dst, const void* src, size_t bytes) {
    staging_copy(h, dst, src, bytes, [](int, size_t, size_t) {});
}

// `dst` null: the solver's current parameter vector h->x; else a buffer of the caller's (sfmba_reprojection_stats), which
// leaves h->x and the origin of the fp32 operands alone
int upload_x(sfmba_handle* h, const double* x_host, double* dst) {
    CHK(ensure_h_x(h));
    if (h->forms.mixed && !dst) {                    // origin of the fp32 operands: mean of (a sample of) this vector's points
        const double* pts = x_host + 6 * h->C;
        const int64_t stride = std::max<int64_t>(1, h->P / 1024);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int64_t cnt = 0;
        for (int64_t q = 0; q < h->P; q += stride, ++cnt) { sx += pts[3 * q]; sy += pts[3 * q + 1]; sz += pts[3 * q + 2]; }
        h->origin = Origin{sx / (double)cnt, sy / (double)cnt, sz / (double)cnt};
        if (!std::isfinite(h->origin.x + h->origin.y + h->origin.z)) h->origin = Origin{0.0, 0.0, 0.0};
    }
    // The staging buffer's readers and writers on the stream: every call waits for its own before it returns (the solve
    // for a post behind its upload and for the result's copy); synchronising an idle stream costs about 1 us and is kept.
    // The early result copy of a solve runs on the copy stream: only a solve that failed leaves one behind.
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->result_in_flight && h->copy_stream) HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    h->result_in_flight = false;
    const double t0 = now_s();
    hipError_t err = hipSuccess;
    staging_copy(h, h->h_x, x_host, sizeof(double) * h->n, [&](int, size_t off, size_t bytes) {
        if (bytes == 0 || err != hipSuccess) return;
        err = hipMemcpyAsync(reinterpret_cast<char*>(dst ? dst : h->x) + off, reinterpret_cast<const char*>(h->h_x) + off, bytes,
                             hipMemcpyHostToDevice, h->stream);
    });
    HIPCHK(h, err);
    if (h->dbg.trace_timing) fprintf(stderr, "sfmba: upload_x  staging copy + enqueue %.1f us\n", 1e6 * (now_s() - t0));
    return 0;
}

// every compute entry: is the handle ready, and which forms does this call run (the solve stage of the decision)
int begin_compute(sfmba_handle* h, const void* x) {
    if (!h->have_problem) return fail(h, -1, "sfmba_set_problem has not been called");
    if (h->transport_dropped)
        return fail(h, -1, "sfmba_set_problem removed this handle's multi-rank transport (direct link / RCCL communicator / "
                           "callback): set it up again for the new problem, or call sfmba_set_exchange(h, NULL, 0, NULL, NULL, 0) "
                           "to solve the shard on its own");
    if (!x) return fail(h, -1, "x is NULL");
    decide_solve_forms(h);
    return 0;
}
}  // namespace sfmba

namespace {

// All-reduce `count` doubles of the exchange arena in place over the ranks, on the handle's stream:
// natively with RCCL when a communicator is set, else through the host callback, else a no-op.
void p2p_release(sfmba_handle* h);
void p2p_close_peers(sfmba_handle* h);
const unsigned* p2p_error_word(const sfmba_handle* h) { return h->p2p.ready ? h->p2p.words + 1 : nullptr; }

constexpr long long kP2pFirstTicks = 6000000000ll, kP2pSteadyTicks = 3000000000ll;      // 60 s, 30 s at 100 MHz
constexpr size_t kP2pFlagBytes = sizeof(unsigned long long) * 2 * kP2pMaxRanks * kP2pFlagStride;

long long p2p_timeout(sfmba_handle* h) {
    // Ticks of the 100 MHz wall clock.  The FIRST collective of a solve is the rendezvous of ranks that entered
    // sfmba_solve at different times (Python skew, first-use code-object loads; no barrier is required before a solve):
    // it waits up to 60 s.  Steady state: 30 s -- the devices run in lockstep there, but a host thread that stalls between
    // two launches (a cold page of a runtime library on a fresh machine, a descheduled process) holds its peers up for as
    // long; the bound only decides how soon a dead peer is noticed (round 4: 3 s gave one spurious failure in a first solve
    // on a fresh box).
    const long long ticks = h->p2p.first_in_solve ? kP2pFirstTicks : kP2pSteadyTicks;
    h->p2p.first_in_solve = false;
    return h->dbg.p2p_timeout_ms > 0 ? 100000ll * h->dbg.p2p_timeout_ms : ticks;       // test hook
}
void p2p_fill_args(sfmba_handle* h, P2pArgs& a) {
    auto& p = h->p2p;
    for (int q = 0; q < p.world; ++q) { a.data[q] = p.data[q]; a.flags[q] = p.flags[q]; }
    a.rank = p.rank; a.world = p.world; a.stride = p.stride;
    a.seq = reinterpret_cast<unsigned long long*>(p.words + 2);
    a.ticket = p.words; a.error = p.words + 1;
    a.timeout = p2p_timeout(h);
}

// ==== the form decision =================================================================================================
// Problem stage.  sfmba_set_problem calls it twice: once to plan the build of the tables, with the facts that only the
// build can find assumed favourable, and once at its end with the facts as found; that result stays in h->forms.
//   form                      | runs when                                                        | overriding option
//   packed_upload             | N >= 65536, C <= 65535 and every pixel an int16 integer          | packed_upload = 1 / 0
//   cm_device                 | N >= 65536 and the camera counters fit the LDS                   | cm_device = 1 / 0
//   cam_chunk_len             | max(4096, N / (2 CUs))                                           | cam_chunk = length
//   xcd_b (table of pass B)   | P >= 250000                                                      | xcd_chunks = 1 / 0
//   lds_tab (K1, K2)          | the camera table fits the LDS                                    | tab_lds = 0
//   lds_vec (sweeps)          | a camera vector fits the LDS                                     | vec_lds = 0
//   pass A: sweep_rc          | C <= kRcMaxCams and its table fits the LDS: blocks recomputed    | sweep_rc = 0 (stored J), 2 (sweep_rc_g)
//           sweep_rc_g        | else: blocks recomputed from a table in global memory            | sweep_rc = 0 (stored J)
//           stored Jacobian   | on request only                                                  |
//   round_blocks              | stored Jacobian in fp32 storage (passes B, K3, rhs round alike)  | --
//   pass B                    | k_cam_schur_w over the XCD-aware table if xcd_b, else k_cam_schur over the chunk list; fp32 records
//                             | if mixed_b, blocks rounded to fp32 if round_blocks, else fp64     | (those of xcd_b, mixed_b)
//   pcg_fused                 | (lds_vec or sweep_rc) and C <= 1024: update in pass A's prologue | pcg_fused = 0
//   mixed (pass A fp32 ops)   | fp32 storage and a recomputing pass A                            | pcg_mixed = 1 / 0
//   mixed_b (pass B too)      | mixed                                                            | pcg_mixed_b = 0
//   jfree                     | on request, with lds_tab                                         | jfree = 1
//   rc_cons (k_jdot, k_backsub in row form) | N >= 65536, 64-bit storage and sweep_rc (FinalUpdate needs a thread per camera: skip_last = 2 implies pcg_fused, C <= 1024) | rc_consumers = 0; 1 (whatever N)
//           stored Jacobian   | else: fp32 storage (the stored, rounded blocks are the operator), more cameras than the LDS table takes, sweep_rc = 0 |
//   dense                     | 6 C <= kDenseMaxN and at most 2^26 pair-list entries             | dense = 0
//   use_rhsrec (rhs pass)     | P >= 250000                                                      | rhsrec = 1 / 0
// So cfg4 (1000 cameras / 100k points / 1M observations, fp64): pass A k_point_sweep_rc<FUSED> (sweep_rc, pcg_fused), pass B
// k_cam_schur over the chunk list; cfg5 in fp32 storage (5000 / 1M / 10M): pass A k_rc_table32 + k_point_sweep_rc32 (sweep_rc_g,
// mixed), pass B k_cam_schur_w on fp32 records over the XCD-aware table + k_cam_combine_w (xcd_b, mixed_b), rhs pass from rhsrec.
Forms decide_problem_forms(int64_t C, int64_t P, int64_t N, bool f32, int n_cu, const ProblemFacts& facts, const Debug& dbg) {
    const auto by_size = [](int option, bool fits) { return option == 1 || (option != 0 && fits); };     // 1 forces, 0 forbids
    Forms f;
    f.packed_upload = by_size(dbg.packed_upload, N >= 65536) && C <= 65535 && facts.pixels_int16;   // (small: two launches > the bytes)
    // (from 64k observations on: below that the three launches cost more than the host's sort)
    f.cm_device = by_size(dbg.cm_device, N >= 65536) && sizeof(int) * (size_t)C <= kLdsDynMax;
    // a camera of up to 4096 observations is one workgroup (16 per lane) and needs no combine launch
    f.cam_chunk_len = dbg.cam_chunk > 0 ? dbg.cam_chunk : std::max<int64_t>(4096, (N + 2 * n_cu - 1) / (2 * n_cu));
    f.cam_multi = facts.cam_multi;
    f.xcd_b = by_size(dbg.xcd_chunks, P >= 250000);
    f.lds_tab = (size_t)C * kCamRow * sizeof(double) <= kLdsDynMax && dbg.tab_lds != 0;
    f.lds_vec = (size_t)C * 6 * sizeof(double) <= kLdsDynMax && dbg.vec_lds != 0;
    f.sweep_rc = C <= kRcMaxCams && (size_t)C * kRcRow * sizeof(double) <= kLdsDynMax && dbg.sweep_rc != 0 && dbg.sweep_rc != 2;
    f.sweep_rc_g = !f.sweep_rc && dbg.sweep_rc != 0;
    f.round_blocks = f32 && !f.sweep_rc && !f.sweep_rc_g;
    f.pcg_fused = (f.lds_vec || f.sweep_rc) && C <= kSweepThreads && dbg.pcg_fused != 0;
    // fp32 operands in the implicit Schur product: with fp32 storage (BASELINE config 5 names it), or on request
    f.mixed = (f.sweep_rc || f.sweep_rc_g) && by_size(dbg.pcg_mixed, f32);
    f.mixed_b = f.mixed && dbg.pcg_mixed_b != 0;
    f.jfree = dbg.jfree == 1 && f.lds_tab;
    // (the row form saves the 96 bytes of J per observation and pays a 144-byte table prologue per workgroup and a longer
    // dependent chain per observation: even at 30k observations, 1 % ahead at 64k, 3-4 % of a solve from 100k on)
    f.rc_cons = !f32 && f.sweep_rc && by_size(dbg.rc_consumers, N >= 65536);
    f.dense = 6 * C <= kDenseMaxN && dbg.dense != 0 && facts.pair_entries <= ((int64_t)1 << 26);   // (very long tracks: the pair lists would not pay)
    // One 128-byte gather record per point for k_cam_rhs_diag pays once the point tables no longer sit in the L2s
    // (1M points: 432 -> 188 us); at 100k points the two 4.8 MB tables it replaces are L2-resident and k_prep's 11 MB of
    // extra writes cost what the pass gains
    f.use_rhsrec = by_size(dbg.rhsrec, P >= 250000);
    return f;
}

// Solve stage, at the start of every compute call (begin_compute): the transport is attached between sfmba_set_problem
// and the call, and these options are read live.  Nothing it reads changes inside a call: a direct link that fails is
// closed by sfmba_solve_from only after the solve has returned.
//   spread = several ranks, cam_multi or xcd_b: the sums of a camera come from several workgroups
//   link   = direct link, single-chunk cameras on every rank, and few cameras where ranks share a GPU (note below)
//   local  = pcg_local != 0, precond != 0 and a PCG form with per-camera bookkeeping (pcg_fused or sweep_rc_g)
//   form                      | runs when                                                        | overriding option
//   precond (Schur diagonal)  | always                                                           | precond = 0
//   K3, rhs pass: xcd_cam     | xcd_b: XCD-aware table, one wave per chunk, sums by collective   | xcd_cam = 0
//                 cam_inline  | link, single-chunk cameras, not xcd_cam: exchanged per camera    | pcg_inline = 0
//                 own_inverse | single-chunk cameras and (one rank or cam_inline)                | --
//   product reduced: pcg_inline, inside pass B camera by camera | link, local, not cam_multi / xcd_b | pcg_inline = 0, pcg_split = 1
//     else pcg_split: k_p2p_pcg, or collective + k_pcg_tail     | local and spread                   | pcg_split = 0 (1: not spread too)
//     else collective + k_pcg_update (fused: pass A's prologue) | spread; one rank: nothing to reduce |
//   pcg_local, pcg_local2     | pcg_fused / sweep_rc_g without it; not spread, or split / inline | pcg_local = 0
//   skip_last                 | pcg_fused and (one rank or pcg_inline): 2 if pcg_local and (rc_cons, or lds_vec and not jfree), else 1 | pcg_skip_last = 0, 2 (-> 1)
//   dense_solve               | dense and one rank                                               | dense = 0
//   quick_start, spec_scale, cost_rider | one rank                     | start_handoff = 0 or cost_rider = 0; spec_scale = 0; cost_rider = 0
//   early_download            | the copy stream exists                                           | early_download = 0
// So cfg4 on one rank: not spread, pcg_local -- pass B does the per-camera bookkeeping and nothing is reduced; cfg5: spread by
// xcd_b, pcg_split with pcg_local2 -- k_pcg_tail behind k_cam_combine_w, then k_pcg_update_local; cfg4 / 8 over the direct link:
// pcg_inline with pcg_local -- the product is summed over the ranks inside pass B, K3 and the rhs pass exchange per camera.
// sharded over the direct link, every camera a single chunk: per-camera sums are all-reduced by the workgroup that
// forms them (CamExchange) instead of by a collective launch behind the kernel
// -- on EVERY rank (the chunking is a property of the shard; ranks that disagreed would wait for each other in different
// kernels), and practically never between ranks that SHARE one GPU (`link` of decide_solve_forms).  With a GPU per rank a waiting
// workgroup costs its own device a slot and nothing else.  On a shared device the ranks compete for the CUs: a camera
// workgroup that waits for its peer holds registers on its CU, and the peer -- if it is one kernel behind, which two
// processes drift apart by easily -- first has to run pass A, whose 1024-thread workgroups need the whole register file of
// a CU.  Three hundred waiting workgroups sit on every CU of the card, pass A of the other rank then never starts, and
// both time out (seen at 2 x 300 and 2 x 1000 cameras, one run in four; the collective LAUNCHES never had the problem:
// they are one or a few workgroups).  So rehearsals on one device take the exchange inside the kernels only while the
// waiting workgroups of all other ranks leave half the CUs alone -- small tests -- and the collective launches otherwise.
constexpr int64_t kSharedDeviceCams = 128;         // (ranks - 1) x cameras: at most half of the 256 CUs hold a waiting workgroup
void decide_solve_forms(sfmba_handle* h) {
    Forms& f = h->forms;
    const Debug& d = h->dbg;
    const auto& p = h->p2p;
    f.one_rank = !multi_rank(h);
    const bool link = p.ready && !p.any_multi && !(p.shared_device > 1 && h->C * (p.shared_device - 1) > kSharedDeviceCams);
    const bool spread = !f.one_rank || f.cam_multi || f.xcd_b;
    const bool local = d.pcg_local != 0 && d.precond != 0 && (f.pcg_fused || f.sweep_rc_g);
    f.precond = d.precond != 0;
    f.xcd_cam = f.xcd_b && d.xcd_cam != 0;
    f.cam_inline = link && !f.cam_multi && !f.xcd_cam && d.pcg_inline != 0;
    f.own_inverse = !f.cam_multi && (f.one_rank || f.cam_inline);
    f.pcg_inline = link && !f.cam_multi && !f.xcd_b && d.pcg_inline != 0 && local && d.pcg_split != 1;
    f.pcg_split = !f.pcg_inline && local && (spread ? d.pcg_split != 0 : d.pcg_split == 1);
    const bool own_cameras = !spread || f.pcg_split || f.pcg_inline;
    f.pcg_local = f.pcg_fused && d.pcg_local != 0 && own_cameras;
    f.pcg_local2 = !f.pcg_fused && f.sweep_rc_g && d.pcg_local != 0 && own_cameras;
    // (several ranks: only where the product's exchange sits inside pass B -- every rank then takes the same
    // decision from the same record, and a launch that is not enqueued exchanges nothing on any of them)
    f.skip_last = !(f.pcg_fused && (f.one_rank || f.pcg_inline) && d.pcg_skip_last != 0) ? 0
                  : (f.pcg_local && (f.rc_cons || (f.lds_vec && !f.jfree)) && d.pcg_skip_last != 2) ? 2 : 1;
    f.dense_solve = f.dense && f.one_rank;
    // (single rank only -- with several ranks the cost and the scale sums pass through collectives between these launches)
    f.quick_start = f.one_rank && d.start_handoff != 0 && d.cost_rider != 0;
    f.spec_scale = f.one_rank && d.spec_scale != 0;
    f.cost_rider = d.cost_rider != 0;
    f.early_download = h->copy_stream != nullptr && d.early_download != 0;
}

CamExchange cam_exchange(sfmba_handle* h) {
    CamExchange cx{};
    auto& p = h->p2p;
    for (int q = 0; q < p.world; ++q) cx.data[q] = p.camdata[q];
    cx.rank = p.rank; cx.world = p.world; cx.C = (int)h->C; cx.error = p.words + 1;
    cx.timeout = p2p_timeout(h);
    return cx;
}

int p2p_allreduce(sfmba_handle* h, double* ptr, int64_t count, int op, const int* cancel,
                  unsigned long long max_mask = 0, const Piggyback* rider = nullptr, const Mailbox* post = nullptr,
                  const double* skip = nullptr) {
    auto& p = h->p2p;
    P2pArgs a{};
    p2p_fill_args(h, a);
    a.cancel = cancel;
    a.max_mask = max_mask;
    if (rider) a.rider = *rider;
    if (post) a.post = *post;
    a.skip = skip;
    if ((rider || post) && count > 512) return fail(h, -1, "rider / post need a single-workgroup collective");
    const int grid = (int)std::min<int64_t>(kP2pMaxBlocks, std::max<int64_t>(1, (count + 511) / 512));
    hipLaunchKernelGGL(k_p2p_allreduce, dim3(grid), dim3(256), 0, h->stream, ptr, (int)count, op, a);
    LAUNCHED(h);
    ++p.calls;
    return 0;
}

// `cancel` (device pointer, may be null): when it reads non-zero the collective is void on every rank -- it
// follows a PCG launch that did nothing.  Only the direct path can act on it; RCCL and the callback reduce
// the stale vector, which is harmless.
int exchange(sfmba_handle* h, double* ptr, int64_t count, int op, const int* cancel = nullptr) {
    if (h->p2p.ready && count <= h->p2p.stride) {
        CHK(p2p_allreduce(h, ptr, count, op, cancel));
        ++h->n_collectives;
        return 0;
    }
    if (h->comm) {
        RcclApi* api = rccl_api();
        const ncclResult_t rc = api->AllReduce(ptr, ptr, (size_t)count, ncclDouble, op == 0 ? ncclSum : ncclMax,
                                               h->comm, h->stream);
        if (rc != ncclSuccess) return fail(h, -5, "ncclAllReduce failed: %s", api->GetErrorString(rc));
        ++h->n_collectives;
        return 0;
    }
    if (!h->ar_fn) return 0;
    if (h->ar_fn(h->ar_ctx, ptr, count, op) != 0) return fail(h, -5, "all-reduce callback failed");
    ++h->n_collectives;
    return 0;
}

// inverse point blocks: an array of their own, or (record layout 2) a slot of the CURRENT parameter vector's point
// records -- written by k_prep / k_point_prep for h->rec before every consumer of the iteration
double* vinv_ptr(const sfmba_handle* h) { return kVinvInRec < 0 ? h->Vinv.as<double>() : h->rec + kVinvInRec; }

MixedPrep mixed_prep(const sfmba_handle* h, const double* tab) {
    if (!h->forms.mixed) return MixedPrep{nullptr, nullptr, nullptr, nullptr, Origin{0.0, 0.0, 0.0}};
    return MixedPrep{tab, h->rt32.as<float>(), h->rec32.as<float>(), h->rtd.as<double>(), h->origin};
}
// fp32 operands of (x, tab) outside a solve (inside, k_prep writes them)
int launch_mixed_prep(sfmba_handle* h, const double* x, const double* tab) {
    if (!h->forms.mixed) return 0;
    const int bc = (int)((h->C + 255) / 256), bp = (int)((h->P + 255) / 256);
    hipLaunchKernelGGL(k_mixed_prep, dim3(bc + bp), dim3(256), 0, h->stream, mixed_prep(h, tab), x + 6 * h->C, (int)h->C, (int)h->P, bc);
    LAUNCHED(h);
    return 0;
}

ObsArrays obs_arrays(const sfmba_handle* h) {
    return ObsArrays{h->cam_idx.as<int>(), h->pt_idx.as<int>(), h->pt_ptr.as<int>(),
                     h->J.as<double>(), h->ld, h->f32 ? 1 : 0};
}

StepTable step_table(const sfmba_handle* h) {
    return StepTable{h->wsteps.as<int2>(), h->steps.as<int2>(), h->n_ranges};
}

double* partB(const sfmba_handle* h) { return h->part.as<double>() + (size_t)kPartRows * kNQ; }

// The hand-off of an outer iteration: the device posts scalars + PCG control block into the mailbox and
// raises its sequence number (post_mailbox); the host polls that word and nothing else: every
// hipStreamQuery on a busy stream leaves a marker packet in the queue, and a dozen of them behind the
// speculative launches cost 5.8 us before the first kernel of the next iteration.  The post of an iteration
// arrives a few hundred microseconds after the host has finished enqueueing it; only past 5 ms is the stream
// queried (every millisecond), to notice a failed launch instead of spinning forever.
int p2p_timed_out(sfmba_handle* h, unsigned code);
int mailbox_arrived(sfmba_handle* h, const char* where, double t0) {
    report_stall(h, where, now_s() - t0);
    if (h->mbox[kMboxErr] != 0.0)          // published with every post: a direct all-reduce gave up waiting for a peer
        return p2p_timed_out(h, (unsigned)h->mbox[kMboxErr]);
    return 0;
}

// the error word of the direct link (k_p2p_allreduce: 1; cam_exchange_value: which exchange, value and camera) as text
int p2p_timed_out(sfmba_handle* h, unsigned code) {
    if ((code & 0x80000000u) == 0u) return fail(h, -5, "a direct all-reduce timed out waiting for a peer rank");
    static const char* const kinds[8] = {"?", "?", "Schur product (pass B)", "camera blocks (K3)", "reduced right-hand side", "?", "?", "?"};
    return fail(h, -5, "a direct all-reduce timed out waiting for a peer rank: the per-camera exchange of the %s, value %u of "
                       "camera %u", kinds[(code >> 28) & 7u], (code >> 23) & 31u, code & 0x7FFFFFu);
}

int wait_mailbox(sfmba_handle* h, unsigned long long seq) {
    unsigned long long* word = reinterpret_cast<unsigned long long*>(h->mbox + kMboxSeq);
    const double t0 = now_s();
    double t_check = t0 + 5e-3;
    for (int spin = 0;; ++spin) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return mailbox_arrived(h, "wait_mailbox", t0);
        __builtin_ia32_pause();
        if ((spin & 15) != 15) continue;
        const double t = now_s();
        if (t < t_check) continue;
        const hipError_t e = hipStreamQuery(h->stream);
        if (e == hipSuccess) {                               // everything enqueued has run: the post is visible
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return mailbox_arrived(h, "wait_mailbox (stream idle)", t0);
            return fail(h, -3, "hand-off mailbox was not written");
        }
        if (e != hipErrorNotReady) return fail(h, -3, "hipStreamQuery failed: %s", hipGetErrorString(e));
        if (t - t0 > h->dbg.wait_deadline_s)   // a kernel that never drains, a peer that died inside a library collective
            return fail(h, -3, "hand-off not posted within %d s: the device queue is stuck", h->dbg.wait_deadline_s);
        t_check = t + 1e-3;
    }
}

// ---- kernel launch wrappers --------------------------------------------------------------------

// camera table and point records of a freshly uploaded parameter vector
int launch_cam_table(sfmba_handle* h, const double* x, double* tab, double* rec, bool one_launch = false) {
    if (one_launch) {
        const int bc = (int)((h->C + 255) / 256);
        hipLaunchKernelGGL(k_cam_table_rec, dim3((unsigned)(bc + (3 * h->P + 255) / 256)), dim3(256), 0, h->stream, x,
                           (int)h->C, (int)h->P, bc, h->K, tab, rec);
        LAUNCHED(h);
        return 0;
    }
    CHK(launch_k_cam_table(h, x, tab));
    hipLaunchKernelGGL(k_fill_rec, dim3((unsigned)((3 * h->P + 255) / 256)), dim3(256), 0, h->stream, x + 6 * h->C, (int)h->P, rec);
    LAUNCHED(h);
    return 0;
}

// residual (+Jacobian) sweep at x (camera table must be current); leaves the
// sum r^2 partials in `part` and returns the number of partials.  With ev0/ev1 the dispatch itself
// is bracketed (hipExtLaunchKernelGGL: start/stop taken from the kernel's own dispatch, as rocprofv3
// does), so the measured duration is the kernel's and not host launch latency.
PointBlocksOut point_blocks_out(sfmba_handle* h) {
    return PointBlocksOut{h->V.as<double>(), h->gp.as<double>(), h->edge.as<double>()};
}

// the instantiation of K1: BLOCKS only with JAC, and without the Jacobian stores (J-free iteration: the blocks feed the
// point sums only) only where that iteration can run
template <bool LDS, bool JAC, bool STORE_R, bool F32>
auto resjac_kernel(bool blocks, bool jfree) {
    if constexpr (JAC) {
        if constexpr (LDS && STORE_R) { if (blocks && jfree) return k_resjac<LDS, JAC, STORE_R, F32, true, false>; }
        if (blocks) return k_resjac<LDS, JAC, STORE_R, F32, true>;
    }
    return k_resjac<LDS, JAC, STORE_R, F32, false>;
}

// `blocks`: the Jacobian launch also leaves V_p, g_p of x (the point half of the normal equations; the camera half
// and the pieces of runs cut by tile boundaries follow in launch_normal_blocks)
template <bool JAC, bool STORE_R>
int launch_resjac(sfmba_handle* h, const double* x, const double* tab, int* nparts,
                  hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, bool blocks = JAC) {
    const Forms& f = h->forms;
    const int grid = grid_1d(h->N, kSweepThreads, h->n_cu);
    *nparts = grid;
    // the camera table staged in LDS, or its rows gathered through the LDS
    const size_t lds = f.lds_tab ? (size_t)h->C * kCamRow * sizeof(double) : sizeof(double) * kRowSlabDoubles * kWavesPerSweepBlock;
    auto kern = f.lds_tab ? (h->f32 ? resjac_kernel<true, JAC, STORE_R, true>(blocks, f.jfree) : resjac_kernel<true, JAC, STORE_R, false>(blocks, f.jfree))
                          : (h->f32 ? resjac_kernel<false, JAC, STORE_R, true>(blocks, false) : resjac_kernel<false, JAC, STORE_R, false>(blocks, false));
    const double* pts = x + 6 * h->C;
    const PointBlocksOut pb = (JAC && blocks) ? point_blocks_out(h) : PointBlocksOut{nullptr, nullptr, nullptr};
    CHK(set_lds(h, kern, lds));
    if (ev0) {
        hipExtLaunchKernelGGL(kern, dim3(grid), dim3(kSweepThreads), (uint32_t)lds, h->stream, ev0, ev1, 0u, tab, pts,
                              (const int*)h->cam_idx.as<int>(), (const int*)h->pt_idx.as<int>(),
                              (const double*)h->uv.as<double>(), h->r.as<double>(), h->J.as<double>(),
                              (int)h->N, h->ld, (int)h->C, h->K, h->part.as<double>(), h->skip, pb);
    } else {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kSweepThreads), lds, h->stream, tab, pts,
                           h->cam_idx.as<int>(), h->pt_idx.as<int>(), h->uv.as<double>(),
                           h->r.as<double>(), h->J.as<double>(), (int)h->N,
                           h->ld, (int)h->C, h->K, h->part.as<double>(), h->skip, pb);
    }
    LAUNCHED(h);
    return 0;
}

// "sum the partial rows [0, n) of `part`, one column, into scalar s": as a rider workgroup of the launch behind the
// producer (Piggyback), or as a k_finish launch of its own (launch_finish)
Piggyback sum_rider(sfmba_handle* h, const double* part, int n, int s) {
    Piggyback pb{part, h->scal(), FinishJob{}, 1, 1, 0};
    pb.job.row0[0] = 0; pb.job.nrows[0] = n;
    for (int k = 0; k < kFinishCols; ++k) { pb.job.slot[0][k] = k == 0 ? s : -1; pb.job.slot[1][k] = -1; }
    return pb;
}
// the sums of a rider as a launch of their own: one workgroup per slice, one wave per quantity
int launch_finish(sfmba_handle* h, const Piggyback& pb, const double* skip = nullptr, const Mailbox& post = Mailbox{}) {
    hipLaunchKernelGGL(k_finish, dim3(pb.ny), dim3(64 * pb.nq), 0, h->stream, pb.part, pb.job, pb.nq, pb.first_sum, pb.out, skip, post);
    LAUNCHED(h);
    return 0;
}

// the two-slice (cameras | points) reduction of k_update_scale; the point slice publishes only q0..q4 (the
// others keep their already rank-reduced values)
FinishJob slices_job(const sfmba_handle* h) {
    FinishJob job{};
    job.row0[0] = 0;         job.nrows[0] = h->red_bc;
    job.row0[1] = h->red_bc; job.nrows[1] = h->red_grid - h->red_bc;
    for (int k = 0; k < kFinishCols; ++k) {
        job.slot[0][k] = k < kNQ ? kCamSlot + k : -1;
        job.slot[1][k] = k <= 4 ? kPointSlot[k] : -1;
    }
    return job;
}
Piggyback slices_rider(sfmba_handle* h) { return Piggyback{h->part.as<double>(), h->scal(), slices_job(h), 2, kNQ, 1}; }

CamMajor cam_major(const sfmba_handle* h) {
    return CamMajor{h->cam_chunks.as<int4>(), h->cm_pt.as<int>(), h->cm_uv.as<double>()};
}
CamMajor cam_major_b(const sfmba_handle* h) {           // the XCD-aware table; its kernels take n_chunks_b / kWaveChunkCams workgroups
    return CamMajor{h->cam_chunks_b.as<int4>(), h->cm_pt.as<int>(), h->cm_uv.as<double>()};
}

// chunk rows of cameras with several chunks -> out[c * cs + col * ks]
int launch_cam_combine(sfmba_handle* h, int ncols, double* out, int cs, int ks, const double* skip, const int* done) {
    if (!h->forms.cam_multi) return 0;
    hipLaunchKernelGGL(k_cam_combine, dim3((int)((h->C * ncols + 255) / 256)), dim3(256), 0, h->stream,
                       h->cam_chunk_ptr.as<int>(), h->cam_partial.as<double>(), (int)h->C, ncols, out, cs, ks, skip, done);
    LAUNCHED(h);
    return 0;
}
// the same for the eight rows per camera of the XCD-aware table
template <int NCOLS>
int launch_cam_combine_w(sfmba_handle* h, double* out, int cs, int ks, const int* done, const double* skip) {
    hipLaunchKernelGGL(k_cam_combine_w<NCOLS>, dim3((unsigned)((NCOLS * h->C + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)h->cam_partial.as<double>(), (int)h->C, out, cs, ks, done, skip);
    LAUNCHED(h);
    return 0;
}

// K3 at (tab, rec): [U_c | g_c] over the camera-major order, blocks recomputed from the camera table and the point
// records.  V_p, g_p were left by the residual+Jacobian launch at the same x (launch_resjac with `blocks`), except
// for the runs its 64-observation tiles cut: their pieces are added by a few extra workgroups of this launch.
// `cost_parts` > 0: the launch also sums that many cost partials (left in `part` by the residual launch before it) into
// scalar slot 0 and posts the hand-off `mb` (one more rider workgroup instead of a k_finish launch)
int launch_normal_blocks(sfmba_handle* h, const double* tab, const double* rec, int cost_parts = 0, const Mailbox& mb = Mailbox{}) {
    const Forms& f = h->forms;
    const int tiles = (int)((h->N + 63) / 64);
    const int extra = (tiles + kCamThreads - 1) / kCamThreads + (cost_parts > 0 ? 1 : 0);
    CamExchange cx{};
    if (f.cam_inline) { cx = cam_exchange(h); ++h->p2p.calls; ++h->n_collectives; }
    const Piggyback fin = cost_parts > 0 ? sum_rider(h, h->part.as<double>(), cost_parts, kCostSlot) : Piggyback{};
    if (f.xcd_cam) {                                            // many points: one wave per chunk of the XCD-aware table
        const int wgrid = h->n_chunks_b / kWaveChunkCams;
        hipLaunchKernelGGL(h->f32 ? k_cam_blocks_w<true> : k_cam_blocks_w<false>, dim3(wgrid + extra), dim3(kCamThreads), 0, h->stream,
                           cam_major_b(h), tab, rec, h->K, h->cam_partial.as<double>(), h->skip, wgrid,
                           (const int*)h->pt_idx.as<int>(), (int)h->N, point_blocks_out(h), fin, mb);
        LAUNCHED(h);
        CHK(launch_cam_combine_w<27>(h, h->Ugc(), 27, 1, nullptr, h->skip));
        return exchange(h, h->Ugc(), 27 * h->C, 0);
    }
    hipLaunchKernelGGL(h->f32 ? k_cam_blocks<true> : k_cam_blocks<false>, dim3(h->n_chunks + extra), dim3(kCamThreads), 0, h->stream,
                       cam_major(h), tab, rec, h->K, h->Ugc(), h->cam_partial.as<double>(), h->skip, (int)h->n_chunks,
                       (const int*)h->pt_idx.as<int>(), (int)h->N, point_blocks_out(h), fin, mb, cx);
    LAUNCHED(h);
    CHK(launch_cam_combine(h, 27, h->Ugc(), 27, 1, h->skip, nullptr));
    if (f.cam_inline) return 0;                                 // [U | g_c] was summed over the ranks camera by camera
    return exchange(h, h->Ugc(), 27 * h->C, 0);
}

// Pass A of the implicit Schur product (z_p for every point).  FUSED: with the PCG update of the previous product in
// its prologue (one launch; vin = base of the vector sets, ctrl2 = the control blocks).  Else inside the two-kernel
// PCG the same vin / ctrl2, and L selects the set on the device; standalone (test entry): vin = the vector itself,
// plane-major when it is staged in LDS, camera-major otherwise; ctrl2 = nullptr.
template <bool FUSED>
int launch_pass_a(sfmba_handle* h, const double* vin, const PcgCtrl* ctrl2, int L) {
    const Forms& f = h->forms;
    const dim3 grid((h->n_ranges + kWavesPerSweepBlock - 1) / kWavesPerSweepBlock), block(kSweepThreads);
    const int C = (int)h->C;
    const int *ci = h->cam_idx.as<int>(), *pi = h->pt_idx.as<int>();
    const double *tab = h->tab, *pts = h->x + 6 * h->C, *vinv = vinv_ptr(h), *acc = h->acc();
    const float* rt32 = h->rt32.as<float>();
    PcgFused pf{};
    if constexpr (FUSED)
        pf = PcgFused{h->Dc.as<double>(), h->Minv.as<double>(), h->Ugc(), h->vecs.as<double>(), h->ctrl.as<PcgCtrl>(),
                      h->pcg_tol, h->pcg_cap, (const double*)(h->scal() + kEtaSlot),
                      f.pcg_local ? h->pcg_part.as<double>() : (double*)nullptr};
    // the three families of pass A; `table`: the recomputing forms' table in global memory (null: built in LDS)
    auto rc32 = [&](auto kern, size_t lds, const float* table) -> int {      // fp32 operands
        CHK(set_lds(h, kern, lds));
        hipLaunchKernelGGL(kern, grid, block, lds, h->stream, step_table(h), ci, pi, tab, rt32, h->K, vin, vinv,
                           h->rec32.as<float>(), acc, C, ctrl2, L, pf, table, h->rec);
        LAUNCHED(h);
        return 0;
    };
    auto rc = [&](auto kern, size_t lds, const double* table) -> int {       // blocks recomputed in fp64
        CHK(set_lds(h, kern, lds));
        hipLaunchKernelGGL(kern, grid, block, lds, h->stream, step_table(h), ci, pi, tab, pts, h->K, vin, vinv, h->rec, acc, C,
                           ctrl2, L, pf, table);
        LAUNCHED(h);
        return 0;
    };
    auto stored = [&](auto kern, size_t lds) -> int {                        // the stored Jacobian
        CHK(set_lds(h, kern, lds));
        hipLaunchKernelGGL(kern, grid, block, lds, h->stream, step_table(h), obs_arrays(h), vin, vinv, h->rec, acc, C, ctrl2, L, pf);
        LAUNCHED(h);
        return 0;
    };
    if (f.mixed && f.sweep_rc)
        return rc32(f.mixed_b ? k_point_sweep_rc32<FUSED, false, false> : k_point_sweep_rc32<FUSED, false, true>,
                    sizeof(float) * kRc32Row * (size_t)C, nullptr);
    if (f.sweep_rc) return rc(k_point_sweep_rc<FUSED>, sizeof(double) * kRcRow * (size_t)C, nullptr);
    if constexpr (FUSED) {
        return stored(k_point_sweep<true, true>, sizeof(double) * 6 * (size_t)C);
    } else {
        if (f.mixed && f.sweep_rc_g) {        // table in global memory: one small launch builds it
            hipLaunchKernelGGL(k_rc_table32, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, h->stream, tab, rt32, vin, ctrl2, L, C,
                               h->rctab32.as<float>());
            LAUNCHED(h);
            return rc32(f.mixed_b ? k_point_sweep_rc32<false, true, false> : k_point_sweep_rc32<false, true, true>,
                        sizeof(float) * kRow32SlabFloats * kWavesPerSweepBlock, h->rctab32.as<float>());
        }
        if (f.sweep_rc_g) {
            hipLaunchKernelGGL(k_rc_table, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, h->stream, tab, vin, ctrl2, L, C,
                               h->rctab.as<double>());
            LAUNCHED(h);
            return rc(k_point_sweep_rc<false, true>, sizeof(double) * kRowSlabDoubles * kWavesPerSweepBlock,    // rows gathered through the LDS
                      h->rctab.as<double>());
        }
        return f.lds_vec ? stored(k_point_sweep<true, false>, sizeof(double) * 6 * (size_t)C) : stored(k_point_sweep<false, false>, 0);
    }
}
// Pass B (camera-major): MODE 0  acc = sum Jc^T (Jc v - Jp z) with z from pass A; MODE 1  acc = -sum Jc^T Jp e.
// ctrl_done / set: see k_cam_schur.
template <int MODE>
int launch_cam_schur(sfmba_handle* h, const double* vin, const PcgCtrl* ctrl_done, int set, bool local = false,
                     bool inline_exchange = false) {
    const Forms& f = h->forms;
    const PcgLocal pl{h->Dc.as<double>(), h->Minv.as<double>(), h->vecs.as<double>(),
                      local ? h->pcg_part.as<double>() : (double*)nullptr};
    CamExchange cx{};
    if (MODE == 0 && inline_exchange) { cx = cam_exchange(h); ++h->p2p.calls; ++h->n_collectives; }
    const MixedB mxb{h->rtd.as<double>()};
    // fp32 operands: the same rounded R, T - o, X - o, a', u_T as pass A
    const bool mixed = MODE == 0 && f.mixed_b;
    const double* rec = mixed ? reinterpret_cast<const double*>(h->rec32.as<float>()) : (const double*)h->rec;
    const int* done = ctrl_done ? &ctrl_done->done : nullptr;
    // MODE 0 with the XCD-aware table: chunk 8 c + k runs on XCD k and gathers records of point range k only, one wave per chunk
    if (MODE == 0 && f.xcd_b) {
        if (f.round_blocks) return fail(h, -1, "XCD-aware chunks need the recomputing form of pass A");
        hipLaunchKernelGGL(mixed ? k_cam_schur_w<true> : k_cam_schur_w<false>, dim3(h->n_chunks_b / kWaveChunkCams), dim3(kCamThreads), 0,
                           h->stream, cam_major_b(h), (const double*)h->tab, rec, h->K, vin, (int)h->C, h->cam_partial.as<double>(),
                           ctrl_done, set, mxb);
        LAUNCHED(h);
        return launch_cam_combine_w<6>(h, h->acc(), 1, (int)h->C, done, nullptr);
    }
    // (round_blocks: pass A applies the stored fp32 blocks, pass B rounds its own the same way)
    auto kern = f.round_blocks ? k_cam_schur<MODE, true> : mixed ? k_cam_schur<0, false, true> : k_cam_schur<MODE, false>;
    hipLaunchKernelGGL(kern, dim3(h->n_chunks), dim3(kCamThreads), 0, h->stream, cam_major(h), (const double*)h->tab,
                       rec, h->K, vin, (int)h->C, h->acc(), h->cam_partial.as<double>(),
                       ctrl_done, set, pl, mxb, cx);
    LAUNCHED(h);
    return launch_cam_combine(h, 6, h->acc(), 1, (int)h->C, nullptr, done);
}

// all-reduced [U | g_c], acc | sd -> Dc-damped block inverses of the Schur-diagonal preconditioner
int launch_cam_prep_schur(sfmba_handle* h) {
    hipLaunchKernelGGL(k_cam_prep_schur, dim3((unsigned)((h->C + 63) / 64)), dim3(64), 0, h->stream, (const double*)h->Ugc(),
                       (const double*)h->sd(), (int)h->C, h->Dc.as<double>(), h->Minv.as<double>());
    LAUNCHED(h);
    return 0;
}

// Reduced right-hand side term -> acc and, with the Schur-diagonal preconditioner, the diagonal blocks of
// W Vinv W^T -> sd in the same pass; all-reduce; block inverses.  (k_prep has written e into the records and, for
// the block-Jacobi-of-U form, Minv itself.)
int launch_rhs_and_preconditioner(sfmba_handle* h) {
    const Forms& f = h->forms;
    const int64_t C = h->C;
    if (!f.precond) {
        CHK(launch_cam_schur<1>(h, nullptr, nullptr, 0));
        return exchange(h, h->acc(), 6 * C, 0);
    }
    // single-chunk cameras on one rank, or sharded with the sums exchanged camera by camera inside the pass
    // (CamExchange): every workgroup holds its camera's complete sums and inverts its own preconditioner block (RhsPrecond)
    CamExchange cx{};
    if (f.cam_inline) { cx = cam_exchange(h); ++h->p2p.calls; ++h->n_collectives; }
    const double* rr = f.use_rhsrec ? (const double*)h->rhsrec.as<double>() : (const double*)nullptr;
    if (f.xcd_cam) {
        hipLaunchKernelGGL(f.round_blocks ? k_cam_rhs_diag_w<true> : k_cam_rhs_diag_w<false>, dim3(h->n_chunks_b / kWaveChunkCams),
                           dim3(kCamThreads), 0, h->stream, cam_major_b(h), (const double*)h->tab, (const double*)h->rec,
                           (const double*)vinv_ptr(h), h->K, h->cam_partial.as<double>(), rr);
        LAUNCHED(h);
        CHK(launch_cam_combine_w<27>(h, h->acc(), 1, (int)C, nullptr, nullptr));
        CHK(exchange(h, h->acc(), 27 * C, 0));                  // acc | sd: one contiguous plane-major vector
        return launch_cam_prep_schur(h);
    }
    const RhsPrecond mp = f.own_inverse ? RhsPrecond{h->Ugc(), h->Dc.as<double>(), h->Minv.as<double>()} : RhsPrecond{nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(f.round_blocks ? k_cam_rhs_diag<true> : k_cam_rhs_diag<false>, dim3(h->n_chunks), dim3(kRhsThreads), 0, h->stream,
                       cam_major(h), (const double*)h->tab, (const double*)h->rec, (const double*)vinv_ptr(h), h->K, (int)C,
                       h->acc(), h->cam_partial.as<double>(), mp, rr, cx);
    LAUNCHED(h);
    if (f.own_inverse) return 0;
    CHK(launch_cam_combine(h, 27, h->acc(), 1, (int)C, nullptr, nullptr));
    CHK(exchange(h, h->acc(), 27 * C, 0));                  // acc | sd: one contiguous plane-major vector
    return launch_cam_prep_schur(h);
}

// Few cameras: form the block pairs of W V^-1 W^T, then run the PCG on S = U + Dc - (...) inside one workgroup with
// S in LDS; the camera step and the control block are left where the implicit PCG leaves them (x of vector set 0).
// acc must hold the reduced right-hand-side term (pass B, MODE 1).
constexpr double kDenseTolFactor = 0.1;
// `rhs`: the workgroups of the diagonal pairs also leave the reduced right-hand-side term -sum W e in acc (e in the
// z half of the point records, k_prep); false: acc is the caller's (test entry).
int launch_dense_solve(sfmba_handle* h, double tol, int max_iters, bool rhs) {
    hipLaunchKernelGGL(k_schur_blocks, dim3(h->n_blk), dim3(kCamThreads), 0, h->stream, (const int*)h->cov_ptr.as<int>(),
                       (const int*)h->cov_pt.as<int>(), (const int2*)h->blk_ab.as<int2>(), (const double*)h->tab,
                       (const double*)h->rec, (const double*)vinv_ptr(h), h->K, (int)h->C,
                       h->Sblk.as<double>(), rhs ? h->acc() : (double*)nullptr);
    LAUNCHED(h);
    const int n = 6 * (int)h->C;
    const size_t lds = sizeof(double) * ((size_t)n * (size_t)(n | 1) + 2 * kDenseMaxN + ((21 * kDenseMaxN / 6 + 1) & ~1) +
                                         4 * (kDenseThreads / 64));      // matrix | r u | 6x6 inverses | reduction slots
    CHK(set_lds(h, k_dense_pcg, lds));
    hipLaunchKernelGGL(k_dense_pcg, dim3(1), dim3(kDenseThreads), lds, h->stream, (const double*)h->Sblk.as<double>(),
                       (const double*)h->Ugc(), (const double*)h->Dc.as<double>(),
                       (const double*)h->acc(), (int)h->C, tol, max_iters, h->vecs.as<double>(), h->ctrl.as<PcgCtrl>());
    LAUNCHED(h);
    h->pcg_L = 0;
    return 0;
}

// acc = (S - Dc) v for a plane-major vector v outside the PCG (test and timing entries): pass A, pass B
int schur_product_standalone(sfmba_handle* h, const double* v_planes) {
    const double* va = v_planes;
    if (!h->forms.lds_vec && !h->forms.sweep_rc && !h->forms.sweep_rc_g) {    // pass A gathers v from a camera-major copy in L2
        hipLaunchKernelGGL(k_transpose, dim3((unsigned)((6 * h->C + 255) / 256)), dim3(256), 0, h->stream, v_planes,
                           6, (int)h->C, h->vcm.as<double>(), (const PcgCtrl*)nullptr, 0);
        LAUNCHED(h);
        va = h->vcm.as<double>();
    }
    CHK(launch_pass_a<false>(h, va, nullptr, 0));
    return launch_cam_schur<0>(h, v_planes, nullptr, 0);
}

// partials -> half B.  When k_update_scale's final sums are still pending they ride along (one extra workgroup).
int launch_jdot(sfmba_handle* h, int* nparts) {
    const int grid = grid_1d(h->N, kSweepThreads, h->n_cu);
    const double* sgc = h->sg_cur;
    const double* sgp = sgc + 6 * h->C;
    Piggyback pb{};
    if (h->pending_scale_sums) pb = slices_rider(h);
    const int launch_grid = grid + (pb.part != nullptr ? 1 : 0);
    const Recompute rc{h->tab, h->x + 6 * h->C, h->K};
    auto run = [&](auto kern, size_t lds) -> int {
        CHK(set_lds(h, kern, lds));
        hipLaunchKernelGGL(kern, dim3(launch_grid), dim3(kSweepThreads), lds, h->stream, obs_arrays(h), sgc, sgp,
                           (int)h->N, (int)h->C, h->t1.as<double>(), partB(h), pb, rc);
        LAUNCHED(h);
        return 0;
    };
    if (h->forms.rc_cons) {
        const size_t lds = sizeof(double) * kRcRow * (size_t)h->C;
        CHK(set_lds(h, k_jdot_rc, lds));
        hipLaunchKernelGGL(k_jdot_rc, dim3(launch_grid), dim3(kSweepThreads), lds, h->stream, (const int*)h->cam_idx.as<int>(),
                           (const int*)h->pt_idx.as<int>(), rc.camtab, rc.pts, h->K, sgc, sgp, (int)h->N, (int)h->C,
                           h->t1.as<double>(), partB(h), pb);
        LAUNCHED(h);
    } else
    CHK(h->forms.jfree ? run(k_jdot<false, true>, sizeof(double) * kCamRow * (size_t)h->C)
        : h->forms.lds_vec ? run(k_jdot<true>, sizeof(double) * 6 * (size_t)h->C) : run(k_jdot<false>, 0));
    h->pending_scale_sums = false;
    *nparts = grid;
    return 0;
}

// `planes` (test and timing entries): the camera step as a plane-major vector of its own instead of x of the PCG's final set
int launch_backsub(sfmba_handle* h, int* nparts, const double* planes = nullptr) {
    const int grid = (h->n_ranges + kWavesPerSweepBlock - 1) / kWavesPerSweepBlock;
    double* dc = h->p.as<double>();
    double* dp = dc + 6 * h->C;
    const PcgCtrl* ctrl2 = planes ? (const PcgCtrl*)nullptr : h->ctrl.as<PcgCtrl>();
    const double* step_planes = planes ? planes : (const double*)h->vecs.as<double>();
    const Recompute rc{h->tab, h->x + 6 * h->C, h->K};
    // dc from the device-selected vector set: read from the LDS copy of the sets (`in_lds`), or transposed first
    auto run = [&](auto kern, size_t lds, bool in_lds) -> int {
        if (!in_lds) {
            hipLaunchKernelGGL(k_transpose, dim3((6 * h->C + 255) / 256), dim3(256), 0, h->stream,
                               step_planes, 6, (int)h->C, dc, ctrl2, h->pcg_L);
            LAUNCHED(h);
        }
        CHK(set_lds(h, kern, lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kSweepThreads), lds, h->stream, h->ranges.as<int2>(), h->n_ranges, obs_arrays(h),
                           step_planes, dc, vinv_ptr(h), h->gp.as<double>(), h->t1.as<double>(), dp, partB(h),
                           (int)h->C, in_lds ? ctrl2 : (const PcgCtrl*)nullptr, in_lds ? h->pcg_L : 0, h->g_cur, h->si_cur, h->sg_cur, rc,
                           in_lds && h->pcg_a_owed && !planes ? FinalUpdate{h->pcg_part.as<double>(), h->vecs.as<double>(), h->ctrl.as<PcgCtrl>(), h->pcg_L - 1}
                                                   : FinalUpdate{});
        LAUNCHED(h);
        return 0;
    };
    if (h->forms.rc_cons) {
        const size_t lds = sizeof(double) * kRcRow * (size_t)h->C;
        CHK(set_lds(h, k_backsub_rc, lds));
        hipLaunchKernelGGL(k_backsub_rc, dim3(grid), dim3(kSweepThreads), lds, h->stream, (const int2*)h->ranges.as<int2>(), h->n_ranges,
                           (const int*)h->cam_idx.as<int>(), (const int*)h->pt_idx.as<int>(), (const int*)h->pt_ptr.as<int>(),
                           rc.camtab, rc.pts, h->K, step_planes, dc, (const double*)vinv_ptr(h),
                           (const double*)h->gp.as<double>(), (const double*)h->t1.as<double>(), dp, partB(h), (int)h->C, ctrl2, h->pcg_L,
                           (const double*)h->g_cur, (const double*)h->si_cur, (const double*)h->sg_cur,
                           h->pcg_a_owed && !planes ? FinalUpdate{h->pcg_part.as<double>(), h->vecs.as<double>(), h->ctrl.as<PcgCtrl>(), h->pcg_L - 1}
                                                    : FinalUpdate{});
        LAUNCHED(h);
    } else
    CHK(h->forms.jfree ? run(k_backsub<false, true>, sizeof(double) * kCamRow * (size_t)h->C, false)
        : h->forms.lds_vec ? run(k_backsub<true>, sizeof(double) * 6 * (size_t)h->C, true) : run(k_backsub<false>, 0, false));
    *nparts = grid;
    return 0;
}

// column scale + gradient + q0..q4 of the new iterate (after the normal blocks are complete)
// `defer`: the final sums are left to ride with the next k_jdot launch (flush_scale_sums if none follows)
// `speculative`: the trial point h->x_new, enqueued before the host has decided on it.  The accepted point's si, g, sg
// are only read (the running maximum) and the results go to the second buffer set, which the host swaps in when it
// accepts the step; on a rejection nothing is swapped and the next trial's launch overwrites them.  The launch
// honours h->skip (k_tr_step cancelled the trial: K3 wrote no blocks).  The partial rows (half A) are NOT summed by
// this launch: exchange slots 8..12 and kCamSlot + 0..4 always describe the ACCEPTED point when the host or k_prep
// read them -- the sums run (riding with k_jdot, or flush_scale_sums) only after the host has accepted the point,
// i.e. set pending_scale_sums; a rejected trial's rows are overwritten by the next K1 / k_update_scale.
int launch_update_scale(sfmba_handle* h, int first, bool defer = false, bool speculative = false) {
    const double* x = speculative ? h->x_new : h->x;
    double* si = speculative ? h->si_new : h->si_cur;
    double* g = speculative ? h->g_new : h->g_cur;
    double* sg = speculative ? h->sg_new : h->sg_cur;
    const double* skip = speculative ? h->skip : (const double*)nullptr;
    hipLaunchKernelGGL(h->scale_pts == 2 ? k_update_scale<2> : k_update_scale<1>, dim3(h->red_grid), dim3(256), 0, h->stream, h->Ugc(),
                       h->V.as<double>(), h->gp.as<double>(), x, (int)h->C, (int)h->P, first, h->red_bc, (const double*)h->si_cur, si,
                       g, sg, h->part.as<double>(), skip);
    LAUNCHED(h);
    if (speculative) return 0;
    if (defer) { h->pending_scale_sums = true; return 0; }
    return launch_finish(h, slices_rider(h));
}

// q0..q8 with the step vector p
// Final sums of k_backsub's partial rows (half B, kBacksubCols wide): G12, G22 -> slots 2, 3; q5..q8 of the
// point slice -> 4..7 (the run the tail of the linear phase reduces over ranks); q5..q8 of the camera slice -> 21..24.
Piggyback backsub_rider(sfmba_handle* h, int nparts) {
    Piggyback pb{partB(h), h->scal(), FinishJob{}, 1, kBacksubCols, 0};
    pb.job.row0[0] = 0; pb.job.nrows[0] = nparts;
    for (int k = 0; k < kFinishCols; ++k) { pb.job.slot[0][k] = -1; pb.job.slot[1][k] = -1; }
    for (int k = 0; k < 6; ++k) pb.job.slot[0][k] = 2 + k;
    for (int k = 0; k < 4; ++k) pb.job.slot[0][6 + k] = kCamSlot + 5 + k;
    return pb;
}

// all-reduce freshly written exchange scalars over ranks (no-op on one GPU); stays on the stream.
// Only slots written since their last reduction may be included.
int flush_scale_sums(sfmba_handle* h) {         // no k_jdot follows the last k_update_scale: finish on its own
    if (!h->pending_scale_sums) return 0;
    h->pending_scale_sums = false;
    return launch_finish(h, slices_rider(h));
}
int exchange_linearise(sfmba_handle* h) {       // q1..q4 and max|g| of the point slice
    CHK(exchange(h, h->scal() + kQ1Slot, 4, 0));
    CHK(exchange(h, h->scal() + kMaxSlot, 1, 1));
    return 0;
}

// bring all 32 scalars to the host (h_scal) and wait: one small kernel posts them into the mailbox (no blit
// copy, no marker packet in the queue, no stream polling)
int fetch_scalars(sfmba_handle* h) {
    const Mailbox mb{h->mbox_dev, h->scal(), nullptr, ++h->mbox_seq, p2p_error_word(h)};
    hipLaunchKernelGGL(k_post, dim3(1), dim3(64), 0, h->stream, mb);
    LAUNCHED(h);
    CHK(wait_mailbox(h, h->mbox_seq));
    memcpy(h->h_scal, h->mbox, sizeof(double) * kScalSlots);
    return 0;
}

// residual vector of the current buffer set into the caller's array (2N doubles, caller's observation
// order), through the pinned staging buffer
int download_residuals(sfmba_handle* h, double* r_out) {
    CHK(ensure_h_x(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t bytes = (h->f32 ? sizeof(float) : sizeof(double)) * 2 * (size_t)h->N;
    HIPCHK(h, hipMemcpyAsync(h->h_x, h->r.p, bytes, hipMemcpyDeviceToHost, h->stream));
    CHK(wait_stream(h));
    if (!h->f32 && !h->permuted) { memcpy(r_out, h->h_x, bytes); return 0; }
    const float* sf = reinterpret_cast<const float*>(h->h_x);
    for (int64_t k = 0; k < h->N; ++k) {
        const size_t d = caller_position(h, (size_t)k);
        r_out[2 * d] = h->f32 ? (double)sf[2 * k] : h->h_x[2 * k];
        r_out[2 * d + 1] = h->f32 ? (double)sf[2 * k + 1] : h->h_x[2 * k + 1];
    }
    return 0;
}

int pcg_max_iters(const sfmba_handle* h, const sfmba_options& opt) {
    return opt.pcg_max_iter > 0 ? opt.pcg_max_iter : (int)std::max<int64_t>(20, 2 * 6 * h->C);
}

// x = 0, r = rhs, u = Minv r (acc holds the reduced right-hand side term of pass B, MODE 1)
int pcg_start(sfmba_handle* h, const sfmba_options& opt) {
    h->pcg_L = 0;
    h->pcg_b_owed = false;
    h->pcg_a_owed = false;
    if (h->forms.pcg_fused) {                   // launch 0 of the fused form initialises the solve itself
        h->pcg_tol = opt.pcg_tol;
        h->pcg_cap = pcg_max_iters(h, opt);
        return 0;
    }
    if (h->forms.pcg_local2)                    // its update takes gamma from the iterate: no reduction at the start
        hipLaunchKernelGGL(k_pcg_init_local, dim3((unsigned)((h->C + 63) / 64)), dim3(64), 0, h->stream, (const double*)h->Ugc(),
                           (const double*)h->acc(), (const double*)h->Minv.as<double>(), (int)h->C, h->vecs.as<double>(),
                           (const double*)(h->scal() + kEtaSlot), pcg_max_iters(h, opt), h->ctrl.as<PcgCtrl>());
    else
        hipLaunchKernelGGL(k_pcg_init, dim3(1), dim3(1024), 0, h->stream, h->Ugc(), (const double*)h->acc(),
                           h->Minv.as<double>(), (int)h->C, h->vecs.as<double>(), (const double*)(h->scal() + kEtaSlot),
                           pcg_max_iters(h, opt), h->ctrl.as<PcgCtrl>());
    LAUNCHED(h);
    return 0;
}

// The product of pass B (camera chunks already combined) summed over the ranks, and the per-camera tail of the local form
// behind it: one launch on the direct path (k_p2p_pcg), else the collective of the transport and k_pcg_tail.
int launch_reduce_and_tail(sfmba_handle* h, const PcgCtrl* cd, int set) {
    const int C = (int)h->C;
    const PcgLocal pl{h->Dc.as<double>(), h->Minv.as<double>(), h->vecs.as<double>(), h->pcg_part.as<double>()};
    const int grid = std::max((C + kP2pPcgThreads - 1) / kP2pPcgThreads, std::min(kP2pMaxBlocks, (C + 63) / 64));
    if (h->p2p.ready && 6 * h->C <= h->p2p.stride && grid <= kP2pMaxBlocks) {
        P2pArgs a{};
        p2p_fill_args(h, a);
        hipLaunchKernelGGL(k_p2p_pcg, dim3(grid), dim3(kP2pPcgThreads), 0, h->stream, h->acc(), (const double*)h->vecs.as<double>(),
                           C, cd, set, pl, a);
        LAUNCHED(h);
        ++h->p2p.calls;
        ++h->n_collectives;
        return 0;
    }
    CHK(exchange(h, h->acc(), 6 * h->C, 0, &cd->done));
    hipLaunchKernelGGL(k_pcg_tail, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, h->stream, (const double*)h->acc(),
                       (const double*)h->vecs.as<double>(), C, cd, set, pl);
    LAUNCHED(h);
    return 0;
}

// enqueue `count` PCG iterations (pass A [+ update], pass B, all-reduce [, update]); iterations after
// convergence are device-side no-ops, so over-enqueueing is harmless and deterministic.
// `speculative` (fused form, one rank): the batch is the whole guess of an outer iteration and k_backsub follows it.  In
// the fused form k iterations need k + 1 launches of pass A -- the last one only applies the update of iteration k - 1 and
// finds the solve finished -- and the pass B behind that launch returns at its first instruction.  That last pair is not
// enqueued: in the local form k_backsub's prologue does the update itself (FinalUpdate: alpha, x += alpha p, the control
// block -- 8 us of launch less per outer iteration), otherwise pass A is launched and only its pass B is left out
// (4.5 us).  Either way the control block tells whether the guess sufficed; if it did not, the pair is OWED: the next
// call here starts with it (pass A / pass B of launch L need nothing but the vector sets, the partial sums and, for pass
// B, the z of pass A of launch L, all untouched since).
int pcg_pass_b(sfmba_handle* h, int L) {
    const PcgCtrl* cd = h->ctrl.as<PcgCtrl>() + ((L + 1) & 1);
    CHK(launch_cam_schur<0>(h, h->vecs.as<double>(), cd, L & 1, h->forms.pcg_local && !h->forms.pcg_split, h->forms.pcg_inline));
    if (h->forms.pcg_split) CHK(launch_reduce_and_tail(h, cd, L & 1));
    else if (!h->forms.pcg_inline) CHK(exchange(h, h->acc(), 6 * h->C, 0, &cd->done));
    return 0;
}

int pcg_enqueue(sfmba_handle* h, int count, bool speculative = false) {
    PcgCtrl* ctrl2 = h->ctrl.as<PcgCtrl>();
    if (h->pcg_a_owed) {                                        // (k_backsub stood in for this launch and found work left)
        h->pcg_a_owed = false;
        h->pcg_b_owed = true;
        CHK(launch_pass_a<true>(h, h->vecs.as<double>(), ctrl2, h->pcg_L - 1));
    }
    if (h->pcg_b_owed) {
        h->pcg_b_owed = false;
        CHK(pcg_pass_b(h, h->pcg_L - 1));
    }
    for (int k = 0; k < count; ++k) {
        const int L = h->pcg_L;
        if (h->forms.pcg_fused) {
            const bool last = speculative && k == count - 1 && h->forms.skip_last != 0;
            // ... and in the local form with the step vector in k_backsub's LDS not even that pass A: k_backsub's prologue
            // does its update (FinalUpdate)
            if (last && L > 0 && h->forms.skip_last == 2) {
                h->pcg_L = L + 1;
                h->pcg_a_owed = true;
                break;
            }
            CHK(launch_pass_a<true>(h, h->vecs.as<double>(), ctrl2, L));
            // a launch that found the solve finished (or finished it) produced no z: its control block (written
            // to slot (L+1)&1) says so, and pass B and the collective behind it are void as well
            h->pcg_L = L + 1;
            if (last) { h->pcg_b_owed = true; break; }
            CHK(pcg_pass_b(h, L));
            continue;
        }
        const PcgCtrl* cd = ctrl2 + (L & 1);                     // current until k_pcg_update writes the other one
        CHK(launch_pass_a<false>(h, h->vecs.as<double>(), ctrl2, L));
        CHK(launch_cam_schur<0>(h, h->vecs.as<double>(), cd, -1, h->forms.pcg_local2 && !h->forms.pcg_split, h->forms.pcg_inline));
        if (h->forms.pcg_local2 && h->forms.pcg_split) CHK(launch_reduce_and_tail(h, cd, -1));
        if (h->forms.pcg_local2) {                                    // pass B / the tail did the bookkeeping: the light update
            hipLaunchKernelGGL(k_pcg_update_local, dim3((unsigned)((h->C + 1023) / 1024)), dim3(1024), 0, h->stream,
                               h->vecs.as<double>(), (const double*)h->pcg_part.as<double>(), ctrl2, L, (int)h->C);
            LAUNCHED(h);
            h->pcg_L = L + 1;
            continue;
        }
        CHK(exchange(h, h->acc(), 6 * h->C, 0, &cd->done));
        hipLaunchKernelGGL(k_pcg_update, dim3(kPcgUpdateBlocks), dim3(1024), 0, h->stream, (const double*)h->acc(),
                           h->Dc.as<double>(), h->Minv.as<double>(), (int)h->C, h->vecs.as<double>(), ctrl2, L);
        LAUNCHED(h);
        h->pcg_L = L + 1;
    }
    return 0;
}

int pcg_read(sfmba_handle* h, PcgCtrl* hc) {
    static_assert(sizeof(PcgCtrl) <= 24 * sizeof(double), "PcgCtrl fits the pinned tail");
    HIPCHK(h, hipMemcpyAsync(h->h_scal + kPinCtrl, h->ctrl.as<PcgCtrl>() + (h->pcg_L & 1), sizeof *hc,
                             hipMemcpyDeviceToHost, h->stream));
    CHK(wait_stream(h));
    memcpy(hc, h->h_scal + kPinCtrl, sizeof *hc);
    return 0;
}

// poll until the device reports the PCG finished
int pcg_finish_polling(sfmba_handle* h, const sfmba_options& opt, PcgCtrl* hc) {
    const int every = std::max(1, opt.pcg_check_every);
    const int cap = pcg_max_iters(h, opt) + every + 1;
    int launched = 0;
    for (;;) {
        CHK(pcg_enqueue(h, every));
        launched += every;
        CHK(pcg_read(h, hc));
        if (hc->done != 0 || launched > cap) return 0;
    }
}

void append_center(std::string& line, const char* s) {          // Python's format spec ^15
    const int w = 15, len = (int)strlen(s);
    const int left = (w - len) / 2 > 0 ? (w - len) / 2 : 0;
    const int right = w - len - left > 0 ? w - len - left : 0;
    line.append((size_t)left, ' ').append(s).append((size_t)right, ' ');
}
void emit_line(sfmba_handle* h, const std::string& line) {
    if (h->print_fn) { h->print_fn(h->print_ctx, line.c_str()); return; }
    fputs(line.c_str(), stdout);
    fputc('\n', stdout);
    fflush(stdout);
}

// scipy's iteration table (SCIPY common.py:545-563: print_header_nonlinear / print_iteration_nonlinear)
void print_header(sfmba_handle* h) {
    const char* cols[6] = {"Iteration", "Total nfev", "Cost", "Cost reduction", "Step norm", "Optimality"};
    std::string line;
    for (auto c : cols) append_center(line, c);
    emit_line(h, line);
}
void print_iter(sfmba_handle* h, int64_t it, int64_t nfev, double cost, bool have, double red, double step, double opt) {
    char b[64];
    std::string line;
    snprintf(b, sizeof b, "%lld", (long long)it); append_center(line, b);
    snprintf(b, sizeof b, "%lld", (long long)nfev); append_center(line, b);
    snprintf(b, sizeof b, "%.4e", cost); append_center(line, b);
    if (have) { snprintf(b, sizeof b, "%.2e", red); append_center(line, b); snprintf(b, sizeof b, "%.2e", step); append_center(line, b); }
    else { append_center(line, ""); append_center(line, ""); }
    snprintf(b, sizeof b, "%.2e", opt); append_center(line, b);
    emit_line(h, line);
}

}  // namespace

// ==== C-ABI ===============================================================================================================

void sfmba_default_options(sfmba_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->ftol = 1e-8; o->xtol = 1e-8; o->gtol = 1e-8;
    o->max_nfev = 0; o->verbose = 0; o->max_iter = 0;
    o->pcg_tol = 1e-2; o->pcg_max_iter = 0; o->pcg_check_every = 2;
    o->reg_min = 1e-6; o->profile = 0; o->reserved = 0; o->pcg_tol_max = 0.1;
}

int sfmba_create(sfmba_handle** out, int device_id) {
    if (!out) return -1;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return -3;      // no HIP device: the product path fails loudly
    if (device_id < 0 || device_id >= ndev) return -1;
    auto* h = new sfmba_handle();
    h->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) { delete h; return -3; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) h->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return -3; }
    h->own_stream = true;
    if (hipHostMalloc((void**)&h->h_scal, sizeof(double) * 64, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&h->mbox, sizeof(double) * 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->mbox_dev, h->mbox, 0) != hipSuccess) {
        (void)hipStreamDestroy(h->stream); delete h; return -4;
    }
    memset(h->mbox, 0, sizeof(double) * 64);
    {   // lowest priority: where the copy runs as a kernel its waves yield to the evaluation it overlaps
        int prio_low = 0, prio_high = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_low, &prio_high) != hipSuccess) prio_low = 0;
        if (hipStreamCreateWithPriority(&h->copy_stream, hipStreamNonBlocking, prio_low) != hipSuccess) h->copy_stream = nullptr;
    }
    if (h->copy_stream &&
        (hipEventCreateWithFlags(&h->ev_written, hipEventDisableTiming) != hipSuccess ||
         hipEventCreateWithFlags(&h->ev_copied[0], hipEventDisableTiming) != hipSuccess ||
         hipEventCreateWithFlags(&h->ev_copied[1], hipEventDisableTiming) != hipSuccess)) {
        (void)hipStreamDestroy(h->copy_stream);            // (the solve then returns x the plain way)
        h->copy_stream = nullptr;
    }
    *out = h;
    return 0;
}

void sfmba_destroy(sfmba_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->comm) { if (RcclApi* api = rccl_api()) (void)api->CommDestroy(h->comm); h->comm = nullptr; }
    p2p_release(h);
    if (h->copy_stream) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamDestroy(h->copy_stream); }
    if (h->ev_written) (void)hipEventDestroy(h->ev_written);
    for (auto& ev : h->ev_copied) if (ev) (void)hipEventDestroy(ev);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    if (h->h_scal) (void)hipHostFree(h->h_scal);
    if (h->mbox) (void)hipHostFree(h->mbox);
    if (h->h_x) (void)hipHostFree(h->h_x);
    delete h;
}

const char* sfmba_last_error(const sfmba_handle* h) { return h ? h->err.c_str() : "null handle"; }

int sfmba_set_stream(sfmba_handle* h, void* hip_stream) {
    CHK(enter(h));
    if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = static_cast<hipStream_t>(hip_stream);
    h->own_stream = false;
    return 0;
}

int sfmba_set_print(sfmba_handle* h, sfmba_print_fn fn, void* ctx) {
    CHK(enter(h));
    h->print_fn = fn;
    h->print_ctx = ctx;
    return 0;
}

int sfmba_debug_option(sfmba_handle* h, const char* name, int64_t value) {
    CHK(enter(h));
    if (!name) return fail(h, -1, "option name is NULL");
    for (const auto& o : kDebugOptions)
        if (strcmp(name, o.name) == 0) { h->dbg.*o.member = (int)value; return 0; }
    return fail(h, -1, "unknown debug option '%s'", name);
}

int sfmba_get_form(sfmba_handle* h, const char* name, int32_t* value) {
    CHK(enter(h));
    if (!name || !value) return fail(h, -1, "NULL argument");
    if (strcmp(name, "match_form") == 0) {           // of the descriptor set, not of the problem: 1 = A, 2 = B
        if (!h->match.form) return fail(h, -1, "no descriptors set");
        *value = h->match.form;
        return 0;
    }
    if (!h->have_problem) return fail(h, -1, "no problem set");
    decide_solve_forms(h);                          // the solve stage as the next compute call would decide it
    const Forms& f = h->forms;
    const struct { const char* name; int value; } forms[] = {
        {"lds_tab", f.lds_tab}, {"lds_vec", f.lds_vec}, {"sweep_rc", f.sweep_rc}, {"sweep_rc_g", f.sweep_rc_g},
        {"pcg_fused", f.pcg_fused}, {"mixed", f.mixed}, {"mixed_b", f.mixed_b}, {"jfree", f.jfree}, {"rc_cons", f.rc_cons}, {"dense", f.dense},
        {"cam_multi", f.cam_multi}, {"xcd_b", f.xcd_b}, {"rhsrec", f.use_rhsrec}, {"round_blocks", f.round_blocks},
        {"xcd_cam", f.xcd_cam}, {"own_inverse", f.own_inverse},
        {"one_rank", f.one_rank}, {"precond", f.precond}, {"dense_solve", f.dense_solve}, {"pcg_local", f.pcg_local},
        {"pcg_local2", f.pcg_local2}, {"pcg_split", f.pcg_split}, {"skip_last", f.skip_last}, {"quick_start", f.quick_start},
        {"spec_scale", f.spec_scale}, {"cost_rider", f.cost_rider},
    };
    for (const auto& e : forms)
        if (strcmp(name, e.name) == 0) { *value = e.value; return 0; }
    return fail(h, -1, "unknown form '%s'", name);
}

int sfmba_set_precision(sfmba_handle* h, int32_t storage_bits) {
    CHK(enter(h));
    if (storage_bits != 64 && storage_bits != 32) return fail(h, -1, "storage_bits must be 64 or 32");
    h->f32_next = storage_bits == 32;
    return 0;
}

int sfmba_set_fixed_cameras(sfmba_handle* h, const int64_t* camera_indices, int64_t n_fixed) {
    CHK(enter(h));
    if (n_fixed < 0 || (n_fixed > 0 && !camera_indices)) return fail(h, -1, "bad fixed-camera list");
    h->fixed_next.assign(camera_indices, camera_indices + n_fixed);
    return 0;
}

int64_t sfmba_exchange_doubles(int64_t n_cameras) { return 54 * n_cameras + kScalSlots; }   // kScalSlots = 32

int sfmba_set_exchange(sfmba_handle* h, void* arena, int64_t arena_doubles, sfmba_allreduce_fn fn,
                       void* ctx, int64_t n_obs_total) {
    CHK(enter(h));
    if (!h->have_problem) return fail(h, -1, "call sfmba_set_problem before sfmba_set_exchange");
    h->transport_dropped = false;
    if (!fn) {
        h->ar_fn = nullptr; h->ar_ctx = nullptr;
        h->arena = h->arena_own.as<double>();
        h->N_total = h->N;
        return 0;
    }
    if (!arena || arena_doubles < sfmba_exchange_doubles(h->C))
        return fail(h, -1, "exchange arena too small: need %lld doubles", (long long)sfmba_exchange_doubles(h->C));
    if (n_obs_total < h->N) return fail(h, -1, "n_obs_total is smaller than the local shard");
    h->arena = static_cast<double*>(arena);
    h->arena_doubles = arena_doubles;
    h->ar_fn = fn; h->ar_ctx = ctx;
    h->N_total = n_obs_total;
    return 0;
}

int sfmba_comm_get_unique_id(void* id128_out) {
    RcclApi* api = rccl_api();
    if (!api || !id128_out) return -5;
    ncclUniqueId id;
    if (api->GetUniqueId(&id) != ncclSuccess) return -5;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id128_out, &id, sizeof id);
    return 0;
}

int sfmba_comm_init(sfmba_handle* h, const void* id128, int32_t rank, int32_t world, int64_t n_obs_total) {
    CHK(enter(h));
    if (!h->have_problem) return fail(h, -1, "call sfmba_set_problem before sfmba_comm_init");
    if (!id128 || world < 1 || rank < 0 || rank >= world) return fail(h, -1, "bad communicator arguments");
    if (n_obs_total < h->N) return fail(h, -1, "n_obs_total is smaller than the local shard");
    RcclApi* api = rccl_api();
    if (!api) return fail(h, -5, "librccl.so.1 could not be loaded: %s", dlerror());
    if (h->comm) { (void)api->CommDestroy(h->comm); h->comm = nullptr; }
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    const ncclResult_t rc = api->CommInitRank(&h->comm, world, id, rank);
    if (rc != ncclSuccess) { h->comm = nullptr; return fail(h, -5, "ncclCommInitRank failed: %s", api->GetErrorString(rc)); }
    h->ar_fn = nullptr; h->ar_ctx = nullptr;
    h->arena = h->arena_own.as<double>();
    h->N_total = n_obs_total;
    h->transport_dropped = false;
    return 0;
}

int sfmba_comm_destroy(sfmba_handle* h) {
    CHK(enter(h));
    h->transport_dropped = false;
    if (h->comm) {
        if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
        if (RcclApi* api = rccl_api()) (void)api->CommDestroy(h->comm);
        h->comm = nullptr;
    }
    h->N_total = h->N;
    return 0;
}

// ---- direct all-reduce over peer-mapped memory ---------------------------------------------------------
namespace {
// unmap the peers; this rank's own buffer stays allocated (peers may still be storing into it)
void p2p_close_peers(sfmba_handle* h) {
    auto& p = h->p2p;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (int q = 0; q < kP2pMaxRanks; ++q) {
        if (p.opened[q]) (void)hipIpcCloseMemHandle(p.opened[q]);
        p.opened[q] = nullptr; p.data[q] = nullptr; p.flags[q] = nullptr; p.camdata[q] = nullptr;
    }
    p.ready = false;
}
void p2p_release(sfmba_handle* h) {
    auto& p = h->p2p;
    p2p_close_peers(h);
    if (p.own) (void)hipFree(p.own);
    if (p.words) (void)hipFree(p.words);
    p.own = nullptr; p.words = nullptr; p.ready = false; p.world = 0; p.stride = 0;
    p.shared_device = 1; p.any_multi = false;
}
}  // namespace

int sfmba_p2p_export(sfmba_handle* h, int32_t world, void* handle64_out) {
    CHK(enter(h));
    if (!h->have_problem) return fail(h, -1, "call sfmba_set_problem before sfmba_p2p_export");
    if (!handle64_out || world < 1 || world > kP2pMaxRanks) return fail(h, -1, "bad arguments (1 <= world <= %d)", kP2pMaxRanks);
    p2p_release(h);
    auto& p = h->p2p;
    p.world = world;
    p.stride = (27 * h->C + 15) / 16 * 16;                // the largest vector exchanged: [U | g_c]
    const size_t bytes = kP2pFlagBytes + sizeof(double) * 2 * (size_t)world * (size_t)p.stride +
                         sizeof(double) * cam_slots_total(world, (int)h->C);          // + the per-camera slots (CamExchange)
    // uncached device memory: remote stores land in HBM and local loads do not see stale cache lines
    if (hipExtMallocWithFlags(&p.own, bytes, hipDeviceMallocUncached) != hipSuccess) {
        p.own = nullptr; (void)hipGetLastError();
        return fail(h, -5, "hipExtMallocWithFlags(uncached, %zu bytes) failed", bytes);
    }
    HIPCHK(h, hipMalloc((void**)&p.words, 4 * sizeof(unsigned)));
    HIPCHK(h, hipMemset(p.own, 0, bytes));
    {   // the per-camera slots start EMPTY (CamExchange)
        const size_t cam_off = kP2pFlagBytes + sizeof(double) * 2 * (size_t)world * (size_t)p.stride;
        HIPCHK(h, hipMemsetD32((hipDeviceptr_t)(static_cast<char*>(p.own) + cam_off), (int)0xFFF8A5A5u, (bytes - cam_off) / 4));
    }
    HIPCHK(h, hipMemset(p.words, 0, 4 * sizeof(unsigned)));
    HIPCHK(h, hipDeviceSynchronize());
    hipIpcMemHandle_t mh;
    if (hipIpcGetMemHandle(&mh, p.own) != hipSuccess) {
        (void)hipGetLastError(); p2p_release(h);
        return fail(h, -5, "hipIpcGetMemHandle failed");
    }
    static_assert(sizeof mh == 64, "hipIpcMemHandle_t is 64 bytes");
    memcpy(handle64_out, &mh, sizeof mh);
    return 0;
}

int sfmba_p2p_attach(sfmba_handle* h, const void* handles, int32_t rank, int32_t world) {
    CHK(enter(h));
    auto& p = h->p2p;
    if (!p.own || world != p.world) return fail(h, -1, "sfmba_p2p_export(world) must precede sfmba_p2p_attach");
    if (!handles || rank < 0 || rank >= world) return fail(h, -1, "bad arguments");
    p.rank = rank;
    for (int q = 0; q < world; ++q) {
        void* base = p.own;
        if (q != rank) {
            hipIpcMemHandle_t mh;
            memcpy(&mh, static_cast<const char*>(handles) + 64 * (size_t)q, sizeof mh);
            if (hipIpcOpenMemHandle(&base, mh, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
                (void)hipGetLastError(); p2p_close_peers(h);
                return fail(h, -5, "hipIpcOpenMemHandle failed for rank %d", q);
            }
            p.opened[q] = base;
        }
        p.flags[q] = static_cast<unsigned long long*>(base);
        p.data[q] = reinterpret_cast<double*>(static_cast<char*>(base) + kP2pFlagBytes);
        p.camdata[q] = p.data[q] + 2 * (size_t)world * (size_t)p.stride;
    }
    // Self-test: 24 rounds over the three message sizes the solver uses (a few scalars, 6 C, 27 C), each a
    // chain of one to three back-to-back collectives on the same vector (parity and sequence protocol without
    // the host in between).  Rank r contributes (r + 1 + round)(i mod 97 + 1): every sum is exact in fp64.
    const int64_t sizes[3] = {7, 6 * h->C, std::min<int64_t>(27 * h->C, p.stride)};
    std::vector<double> v((size_t)sizes[2]);
    double* dev = h->arena;                                    // 45 C + 32 doubles: room for 27 C
    bool ok = true;
    for (int round = 0; round < 24 && ok; ++round) {
        const int nt = (int)sizes[round % 3], chain = 1 + round % 3;
        for (int i = 0; i < nt; ++i) v[i] = (double)(rank + 1 + round) * (double)(i % 97 + 1);
        HIPCHK(h, hipMemcpyAsync(dev, v.data(), sizeof(double) * nt, hipMemcpyHostToDevice, h->stream));
        for (int k = 0; k < chain; ++k) CHK(p2p_allreduce(h, dev, nt, 0, nullptr));
        HIPCHK(h, hipMemcpyAsync(v.data(), dev, sizeof(double) * nt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        double wsum = 0.5 * world * (world + 1) + (double)round * world;
        for (int k = 1; k < chain; ++k) wsum *= world;
        for (int i = 0; i < nt; ++i) ok = ok && v[i] == wsum * (double)(i % 97 + 1);
    }
    // What the ranks have to agree on before the per-camera exchanges may run inside the producing kernels (cam_inline):
    // slot q = the identity of rank q's GPU (ranks sharing one: a rehearsal), slot `world` = how many ranks hold a shard
    // whose cameras need combine launches.  One more sum over the link; exact (40-bit integers).
    {
        char bus[64] = {0};
        (void)hipDeviceGetPCIBusId(bus, (int)sizeof bus - 1, h->device);
        unsigned long long id = 1469598103934665603ull;
        for (const char* c = bus; *c; ++c) id = (id ^ (unsigned char)*c) * 1099511628211ull;
        std::fill(v.begin(), v.begin() + world + 1, 0.0);
        v[(size_t)rank] = (double)(1 + (id >> 24));
        v[(size_t)world] = (h->forms.cam_multi || h->forms.xcd_b) ? 1.0 : 0.0;
        HIPCHK(h, hipMemcpyAsync(dev, v.data(), sizeof(double) * (world + 1), hipMemcpyHostToDevice, h->stream));
        CHK(p2p_allreduce(h, dev, world + 1, 0, nullptr));
        HIPCHK(h, hipMemcpyAsync(v.data(), dev, sizeof(double) * (world + 1), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        p.shared_device = 0;
        for (int q = 0; q < world; ++q) p.shared_device += v[(size_t)q] == v[(size_t)rank] ? 1 : 0;
        p.any_multi = v[(size_t)world] != 0.0;
    }
    const int nt = (int)sizes[2];
    unsigned words[2] = {0, 0};
    HIPCHK(h, hipMemcpy(words, p.words, sizeof words, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemsetAsync(dev, 0, sizeof(double) * nt, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!ok || words[1] != 0) {
        p2p_close_peers(h);                                // own buffer is freed by sfmba_p2p_detach, once all ranks agree
        return fail(h, -5, "direct all-reduce self-test failed (%s)", words[1] ? "timeout waiting for a peer" : "wrong sum");
    }
    p.ready = true;
    h->transport_dropped = false;
    return 0;
}

int sfmba_p2p_detach(sfmba_handle* h) {
    CHK(enter(h));
    h->transport_dropped = false;
    p2p_release(h);
    return 0;
}

int64_t sfmba_p2p_calls(const sfmba_handle* h) { return h ? h->p2p.calls : 0; }

int sfmba_problem_reuse(const sfmba_handle* h, int64_t* obs_reused, int64_t* obs_uploaded) {
    if (!h) return -1;
    if (obs_reused) *obs_reused = h->obs_reused;
    if (obs_uploaded) *obs_uploaded = h->obs_uploaded;
    return 0;
}

int32_t sfmba_get_pcg_history(const sfmba_handle* h, int32_t* out, int32_t cap) {
    if (!h) return -1;
    const int32_t n = (int32_t)h->pcg_hist.size();
    for (int32_t k = 0; k < n && k < cap && out; ++k) out[k] = h->pcg_hist[(size_t)k];
    return n;
}

int sfmba_get_counters(const sfmba_handle* h, int64_t* kernel_launches, int64_t* collectives) {
    if (!h) return -1;
    if (kernel_launches) *kernel_launches = h->n_launches;
    if (collectives) *collectives = h->n_collectives;
    return 0;
}

// ---- sfmba_set_problem ---------------------------------------------------------------------------------------------
namespace {
// What the phases of a sfmba_set_problem call share; run() is the call, the members below it are its phases in order.
struct ProblemBuild {
    sfmba_handle* const h;
    const int64_t C, P, N;
    const int64_t *const cam, *const pt;
    const double* const uv;
    const int64_t* const uv_i64;
    const double* const K;
    const int64_t ld = (N + 255) / 256 * 256;
    const size_t ldz = (size_t)ld;
    const bool f32 = h->f32_next;
    Forms plan;                              // the forms with the facts of the tables still assumed favourable
    std::vector<char> fixed;                 // [C] camera held still
    int64_t n_cmp = 0;                       // observations compared with the previous problem's
    ProblemTables& tb = h->tb;               // the tables, the order, the facts and the re-used prefix (tb.fdiff)
    StagedArrays st;                         // the converted arrays in pinned memory (h->stage)
    int64_t p_keep = 0;                      // run offsets that are unchanged on the device
    size_t tables_bytes = 0;

    int run();
    // the phases, in order (the form decision sits between stage_and_build and allocate)
    int check_and_reset();
    int stage_and_build();          // pinned staging, then build_problem_tables()
    int allocate(), upload_and_zero(), enqueue_camera_major();
    hipError_t up(void* dst, const void* src, size_t elem, size_t from, size_t to) {
        if (to <= from) return hipSuccess;
        return hipMemcpyAsync(static_cast<char*>(dst) + elem * from, static_cast<const char*>(src) + elem * from,
                              elem * (to - from), hipMemcpyHostToDevice, h->stream);
    }
};

int ProblemBuild::check_and_reset() {
    if (C <= 0 || P <= 0 || N <= 0) return fail(h, -1, "n_cameras, n_points, n_obs must be positive");
    if (!cam || !pt || (!uv && !uv_i64) || !K) return fail(h, -1, "NULL array argument");
    if (N >= (int64_t)1 << 30 || 6 * C + 3 * P >= (int64_t)1 << 31)
        return fail(h, -1, "problem too large for 32-bit observation indices");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(K[k])) return fail(h, -1, "K is not finite");
    // Cameras held still (create_sparsity_matrix(..., fixed_camera_indices), bundle_adjustment.py:6,13-14: their six
    // Jacobian columns are structurally zero, so scipy's finite differences leave them zero, the gradient and the
    // step of those parameters are zero and x_scale='jac' gives them scale 1).  Here: their observations are left out
    // of the CAMERA-MAJOR lists (and of the block-pair lists of the few-camera path), so every per-camera sum --
    // U_c, g_c, the reduced right-hand side, the Schur-diagonal block, the product of pass B -- is empty for them,
    // exactly as for a camera nobody observes; the point-major sweeps keep the observations (residual, cost, V_p,
    // g_p) and only ever multiply the camera part of their Jacobian with a camera vector that stays zero.
    fixed.assign((size_t)C, 0);
    for (int64_t c : h->fixed_next) {
        if (c < 0 || c >= C) return fail(h, -1, "fixed camera index %lld out of range [0,%lld)", (long long)c, (long long)C);
        fixed[(size_t)c] = 1;
    }
    h->n_fixed = 0;
    for (char f : fixed) h->n_fixed += f;
    h->fixed_cur.assign(fixed.begin(), fixed.end());
    // A new problem returns the handle to single-process operation: every transport (direct link, RCCL
    // communicator, callback) is torn down and has to be set up again after this call (include/sfmba.h).  The
    // staging buffer of the direct link stays allocated until sfmba_p2p_detach / _export / _destroy, because
    // peers may still have it mapped.
    // The drop is not silent: the next compute call on this handle fails (-1) until a transport is attached again
    // or single-rank operation is acknowledged (begin_compute).
    const bool had_transport = multi_rank(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));                  // collectives in flight; a previous upload may still read the staging
    if (h->p2p.ready) p2p_close_peers(h);
    if (h->comm) { if (RcclApi* api = rccl_api()) (void)api->CommDestroy(h->comm); h->comm = nullptr; }
    if (had_transport) h->transport_dropped = true;
    return 0;
}

// The converted arrays of the last problem stay in pinned host memory and in HBM (incremental re-use, problem_tables.hpp):
// the staging keeps the prefix this call is compared with when it grows.  Then the tables, from the host arrays alone.
int ProblemBuild::stage_and_build() {
    auto& prev = h->prev;
    auto& sg = h->stage;
    n_cmp = (prev.valid && prev.f32 == f32) ? std::min(prev.N, N) : 0;
    prev.valid = false;                                          // until this call has completed
    const size_t keep_obs = (size_t)n_cmp;
    HIPCHK(h, sg.uv.ensure(sizeof(double) * 2 * ldz, sizeof(double) * 2 * keep_obs));
    HIPCHK(h, sg.ci.ensure(sizeof(int) * ldz, sizeof(int) * keep_obs));
    HIPCHK(h, sg.pi.ensure(sizeof(int) * ldz, sizeof(int) * keep_obs));
    HIPCHK(h, sg.perm.ensure(sizeof(int) * ldz, 0));
    HIPCHK(h, sg.ptr.ensure(sizeof(int) * ((size_t)P + 1), 0));
    if (f32) HIPCHK(h, sg.uvf.ensure(sizeof(float) * 2 * ldz, sizeof(float) * 2 * keep_obs));
    const bool try_pack = plan.packed_upload;
    if (try_pack) {
        HIPCHK(h, sg.ci16.ensure(sizeof(unsigned short) * ldz, sizeof(unsigned short) * keep_obs));
        HIPCHK(h, sg.uv16.ensure(sizeof(short) * 2 * ldz, sizeof(short) * 2 * keep_obs));
    }
    st.ci16 = try_pack ? sg.ci16.as<unsigned short>() : nullptr;
    st.uv16 = try_pack ? sg.uv16.as<short>() : nullptr;
    st.uvs = sg.uv.as<double>();
    st.uvf = f32 ? sg.uvf.as<float>() : nullptr;
    st.ci = sg.ci.as<int>(); st.pi = sg.pi.as<int>(); st.perm = sg.perm.as<int>(); st.ptr = sg.ptr.as<int>();

    ProblemInput in;
    in.C = C; in.P = P; in.N = N; in.cam = cam; in.pt = pt; in.uv = uv; in.uv_i64 = uv_i64; in.fixed = fixed.data();
    in.n_cmp = n_cmp;
    in.packed_prefix_ok = try_pack && prev.packed && n_cmp > 0;      // the staged prefix holds valid packed entries
    TablePlan tp;
    tp.dense = plan.dense; tp.xcd_b = plan.xcd_b; tp.cm_device = plan.cm_device; tp.packed_upload = plan.packed_upload;
    tp.cam_chunk_len = plan.cam_chunk_len;
    tp.total_waves = (int64_t)h->n_cu * kWavesPerSweepBlock;
    tp.parts = h->pool.parts_for(N);
    tp.pair_parts = P >= 32768 ? 4 : 1;
    if (!build_problem_tables(in, tp, st, h->pool, tb)) {       // (numpy's fancy indexing would raise IndexError in the reference)
        const int64_t i = tb.bad;
        if (cam[i] < 0 || cam[i] >= C)
            return fail(h, -1, "camera_indices[%lld]=%lld out of range [0,%lld)", (long long)i, (long long)cam[i], (long long)C);
        return fail(h, -1, "point_indices[%lld]=%lld out of range [0,%lld)", (long long)i, (long long)pt[i], (long long)P);
    }
    h->permuted = !tb.sorted;
    h->n_ranges = (int)tb.ranges.size(); h->n_steps = (int)tb.steps.size();
    h->n_chunks = (int)tb.chunks.size(); h->n_chunks_b = (int)tb.chunks_b.size();
    h->n_blk = (int)tb.blk_ab.size();
    return 0;
}

// device arrays: grow-only; the index / pixel arrays keep their re-used prefix when they grow
int ProblemBuild::allocate() {
    const Forms& f = h->forms;
    auto& sg = h->stage;
    const size_t esz = f32 ? sizeof(float) : sizeof(double);     // element size of the per-observation streams
    const size_t keep = (size_t)tb.fdiff;
    HIPCHK(h, h->cam_idx.ensure_keep(sizeof(int) * ldz, sizeof(int) * keep));
    HIPCHK(h, h->pt_idx.ensure_keep(sizeof(int) * ldz, sizeof(int) * keep));
    HIPCHK(h, h->uv.ensure_keep(esz * 2 * ldz, esz * 2 * keep));
    // run offsets of the points before the first changed observation's point are unchanged
    // (entries up to the point of the last unchanged observation are determined by unchanged positions alone)
    p_keep = keep == 0 ? 0 : std::min<int64_t>(std::min<int64_t>(h->prev.P, P), (int64_t)st.pi[tb.fdiff - 1] + 1);
    HIPCHK(h, h->pt_ptr.ensure_keep(sizeof(int) * ((size_t)P + 1), sizeof(int) * (size_t)p_keep));
    // the structure tables: one device buffer, one pinned staging buffer, one copy
    struct Piece { const void* src; size_t bytes; DevView* view; size_t off; };
    Piece pieces[11] = {
        {tb.cam_ptr.data(), sizeof(int) * tb.cam_ptr.size(), &h->cam_ptr_dev, 0},
        {tb.ranges.data(), sizeof(int2) * tb.ranges.size(), &h->ranges, 0},
        {tb.wsteps.data(), sizeof(int2) * tb.wsteps.size(), &h->wsteps, 0},
        {tb.steps.data(), sizeof(int2) * tb.steps.size(), &h->steps, 0},
        {tb.chunks.data(), sizeof(int4) * tb.chunks.size(), &h->cam_chunks, 0},
        {tb.chunk_ptr.data(), sizeof(int) * tb.chunk_ptr.size(), &h->cam_chunk_ptr, 0},
        {tb.cov_ptr.data(), f.dense ? sizeof(int) * tb.cov_ptr.size() : 0, &h->cov_ptr, 0},
        {tb.cov_pt.data(), f.dense ? sizeof(int) * tb.cov_pt.size() : 0, &h->cov_pt, 0},
        {tb.blk_ab.data(), f.dense ? sizeof(int2) * tb.blk_ab.size() : 0, &h->blk_ab, 0},
        {tb.chunks_b.data(), sizeof(int4) * tb.chunks_b.size(), &h->cam_chunks_b, 0},
        {tb.chunk_ptr_b.data(), sizeof(int) * tb.chunk_ptr_b.size(), &h->cam_chunk_ptr_b, 0}};
    tables_bytes = 0;
    for (auto& pc : pieces) { pc.off = tables_bytes; tables_bytes += (pc.bytes + 255) / 256 * 256; }
    HIPCHK(h, h->tables.ensure(tables_bytes + 256));
    HIPCHK(h, sg.tables.ensure(tables_bytes + 256, 0));
    for (auto& pc : pieces) {
        if (pc.bytes) memcpy(sg.tables.as<char>() + pc.off, pc.src, pc.bytes);
        pc.view->p = h->tables.as<char>() + pc.off;
    }
    const size_t n8 = sizeof(double) * (size_t)h->n, cam_tab = sizeof(double) * cam_table_doubles((int)C);
    CHK(ensure_all(h, {
        {&h->xa, n8}, {&h->xb, n8}, {&h->tabA, cam_tab}, {&h->tabB, cam_tab}, {&h->r, esz * 2 * ldz}, {&h->J, esz * 12 * ldz},
        {&h->cm_perm, sizeof(int) * ldz}, {&h->cm_pt, sizeof(int) * ldz}, {&h->cm_uv, esz * 2 * ldz},
        {&h->cam_partial, sizeof(double) * std::max<size_t>(27 * tb.chunks.size(), 27 * tb.chunks_b.size())},
        {&h->recA, sizeof(double) * kRec * P}, {&h->recB, sizeof(double) * kRec * P},
        {&h->rhsrec, f.use_rhsrec ? sizeof(double) * kRhsRec * P : 0}, {&h->Sblk, f.dense ? sizeof(double) * 36 * tb.blk_ab.size() : 0},
        {&h->t1, esz * 2 * ldz}, {&h->V, sizeof(double) * 6 * P}, {&h->Vinv, sizeof(double) * (kVinvInRec < 0 ? kVinvRow * P : 8)},
        {&h->gp, sizeof(double) * 3 * P + 16},                  // (+16: zeroed in 16-byte units)
        {&h->edge, sizeof(double) * 2 * kEdgeRow * (size_t)((N + 63) / 64)}, {&h->e, sizeof(double) * 3 * P},
        {&h->g, n8}, {&h->si, n8}, {&h->sg, n8}, {&h->g2, n8}, {&h->si2, n8}, {&h->sg2, n8}, {&h->p, n8 + 16},
        {&h->Dc, sizeof(double) * 6 * C}, {&h->Minv, sizeof(double) * 21 * C}, {&h->vecs, sizeof(double) * 2 * kPcgVecs * 6 * C},
        {&h->vtmp, sizeof(double) * 6 * C}, {&h->vcm, sizeof(double) * 6 * C},
        {&h->rctab, f.sweep_rc_g ? sizeof(double) * kRcRow * (size_t)C : 0},
        {&h->rt32, f.mixed ? sizeof(float) * kRt32 * (size_t)C : 0}, {&h->rtd, f.mixed ? sizeof(double) * kRt32 * (size_t)C : 0},
        {&h->rec32, f.mixed ? sizeof(float) * kRec32 * (size_t)P : 0},
        {&h->rctab32, f.mixed && f.sweep_rc_g ? sizeof(float) * kRc32Row * (size_t)C : 0},
        {&h->part, sizeof(double) * (size_t)(2 * kPartRows * kNQ)}, {&h->ctrl, 2 * sizeof(PcgCtrl)},
        {&h->pcg_part, sizeof(double) * 4 * C}, {&h->arena_own, sizeof(double) * (size_t)sfmba_exchange_doubles(C)}}));
    h->g_cur = h->g.as<double>(); h->si_cur = h->si.as<double>(); h->sg_cur = h->sg.as<double>();
    h->g_new = h->g2.as<double>(); h->si_new = h->si2.as<double>(); h->sg_new = h->sg2.as<double>();
    // k_update_scale: cameras one element per thread, points kScalePts points per thread (all loads of a thread in flight
    // together); at most 1024 partial rows, summed by k_jdot's rider workgroup
    h->scale_pts = P >= 65536 ? 2 : 1;
    h->red_bc = grid_1d(6 * C, 256, 32);
    h->red_grid = h->red_bc + grid_1d(P, 256 * h->scale_pts, 992);
    h->arena = h->arena_own.as<double>();
    h->ar_fn = nullptr; h->ar_ctx = nullptr;
    h->x = h->xa.as<double>(); h->x_new = h->xb.as<double>();
    h->tab = h->tabA.as<double>(); h->tab_new = h->tabB.as<double>();
    h->rec = h->recA.as<double>(); h->rec_new = h->recB.as<double>();
    return 0;
}

// uploads: observations from the first changed one on, run offsets from its point on, structure tables; then every
// zero-initialised array in ONE launch
int ProblemBuild::upload_and_zero() {
    const size_t esz = f32 ? sizeof(float) : sizeof(double);
    const size_t keep = (size_t)tb.fdiff;
    if (h->forms.packed_upload) {
        HIPCHK(h, h->ci16_dev.ensure(sizeof(unsigned short) * ldz));
        HIPCHK(h, h->uv16_dev.ensure(sizeof(short) * 2 * ldz));
        HIPCHK(h, up(h->ci16_dev.p, st.ci16, sizeof(unsigned short), keep, ldz));
        HIPCHK(h, up(h->uv16_dev.p, st.uv16, 2 * sizeof(short), keep, ldz));
    } else {
        HIPCHK(h, up(h->cam_idx.p, st.ci, sizeof(int), keep, ldz));
        HIPCHK(h, up(h->pt_idx.p, st.pi, sizeof(int), keep, ldz));
        HIPCHK(h, up(h->uv.p, f32 ? (const void*)st.uvf : (const void*)st.uvs, 2 * esz, keep, ldz));
    }
    HIPCHK(h, up(h->pt_ptr.p, st.ptr, sizeof(int), (size_t)p_keep, (size_t)P + 1));
    if (h->forms.packed_upload && keep < ldz) {
        hipLaunchKernelGGL(k_unpack_obs, dim3((unsigned)((ldz - keep + 255) / 256)), dim3(256), 0, h->stream,
                           (const unsigned short*)h->ci16_dev.as<unsigned short>(), (const short2*)h->uv16_dev.as<short2>(),
                           (int)keep, (int)ldz, f32 ? 1 : 0, h->cam_idx.as<int>(), h->uv.as<double>());
        LAUNCHED(h);
        hipLaunchKernelGGL(k_expand_pt_idx, dim3((unsigned)((P + 1 + 255) / 256)), dim3(256), 0, h->stream,
                           (const int*)h->pt_ptr.as<int>(), (int)P, (int)N, (int)ld, h->pt_idx.as<int>());
        LAUNCHED(h);
    }
    h->obs_reused = tb.fdiff;
    h->obs_uploaded = ld - tb.fdiff;
    if (!(tb.fdiff == N && n_cmp == N && h->prev.N == N && h->prev.P == P)) ++h->problem_gen;
    HIPCHK(h, hipMemcpyAsync(h->tables.p, h->stage.tables.p, tables_bytes, hipMemcpyHostToDevice, h->stream));
    // zeroed: the exchange arena; V, g_p (points without observations are never written by the normal-block kernels:
    // their blocks must be 0) and p (... and their step is 0); r; the point records
    ZeroJob z{};
    auto put = [&](int k, void* ptr_, size_t bytes) { z.p[k] = ptr_; z.n16[k] = (int64_t)(bytes / 16); };
    put(0, h->arena, sizeof(double) * (size_t)sfmba_exchange_doubles(C));
    put(1, h->V.p, sizeof(double) * 6 * P);
    put(2, h->gp.p, (sizeof(double) * 3 * P + 15) / 16 * 16);
    put(3, h->p.p, (sizeof(double) * h->n + 15) / 16 * 16);
    put(4, h->r.p, esz * 2 * ldz);
    put(5, h->recA.p, sizeof(double) * kRec * P);
    put(6, h->recB.p, sizeof(double) * kRec * P);
    int64_t most = 0;
    for (int k = 0; k < 7; ++k) most = std::max(most, z.n16[k]);
    hipLaunchKernelGGL(k_zero_many, dim3((unsigned)grid_1d(most, 256 * 4, 2048), 7), dim3(256), 0, h->stream, z);
    LAUNCHED(h);
    return 0;
}

// the camera-major copies of point index and pixel: sorted on the device, or gathered through the host's permutation
int ProblemBuild::enqueue_camera_major() {
    if (!h->forms.cm_device) {
        HIPCHK(h, hipMemcpyAsync(h->cm_perm.p, st.perm, sizeof(int) * ldz, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_build_cam_major, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, h->cm_perm.as<int>(),
                           h->pt_idx.as<int>(), h->uv.as<double>(), f32 ? 1 : 0, (int)N, h->cm_pt.as<int>(),
                           h->cm_uv.as<double>());
        LAUNCHED(h);
        return 0;
    }
    const int B = (int)std::min<int64_t>(kSortSlices, (N + 63) / 64);
    const int per_slice = (int)(((N + B - 1) / B + 63) / 64 * 64);
    int key_bits = 0;
    while (((int64_t)1 << key_bits) < C) ++key_bits;
    HIPCHK(h, h->sort_hist.ensure(sizeof(int) * 2 * (size_t)B * (size_t)C));          // counts | offsets
    int* sort_off = h->sort_hist.as<int>() + (size_t)B * (size_t)C;
    const unsigned char* fixed_dev = nullptr;
    if (h->n_fixed > 0) {
        HIPCHK(h, h->fixed_dev.ensure((size_t)C));
        HIPCHK(h, hipMemcpyAsync(h->fixed_dev.p, fixed.data(), (size_t)C, hipMemcpyHostToDevice, h->stream));
        fixed_dev = h->fixed_dev.as<unsigned char>();
    }
    const size_t lds = sizeof(int) * (size_t)C;
    CHK(set_lds(h, k_cam_scatter, lds));
    CHK(launch_k_cam_hist(h, fixed_dev, B, per_slice, h->sort_hist.as<int>()));
    CHK(launch_k_cam_offsets(h, h->sort_hist.as<int>(), h->cam_ptr_dev.as<int>(), B, sort_off));
    hipLaunchKernelGGL(k_cam_scatter, dim3(B), dim3(64), lds, h->stream, (const int*)h->cam_idx.as<int>(), fixed_dev,
                       (const int*)h->pt_idx.as<int>(), (const double*)h->uv.as<double>(), f32 ? 1 : 0, (int)N, (int)C, per_slice,
                       key_bits, (const int*)sort_off, h->cm_pt.as<int>(), h->cm_uv.as<double>());
    LAUNCHED(h);
    if (h->forms.xcd_b) {
        hipLaunchKernelGGL(k_xcd_chunks, dim3((unsigned)((h->n_chunks_b + 255) / 256)), dim3(256), 0, h->stream,
                           (const int*)h->cam_ptr_dev.as<int>(), (const int*)h->cm_pt.as<int>(), (int)C, (int)P,
                           h->cam_chunks_b.as<int4>());
        LAUNCHED(h);
    }
    return 0;
}

int ProblemBuild::run() {
    const bool timing = h->dbg.trace_timing != 0;
    const double tp0 = now_s();
    h->have_problem = false;
    h->solved = false;
    CHK(check_and_reset());
    plan = decide_problem_forms(C, P, N, f32, h->n_cu, ProblemFacts{}, h->dbg);
    CHK(stage_and_build());
    const double tp1 = tb.t_convert, ts1 = tb.t_sort, ts2 = tb.t_ranges, ts3 = tb.t_steps, tp2 = tb.t_end;
    for (int k = 0; k < 9; ++k) h->K.k[k] = K[k];
    h->f32 = f32;
    h->C = C; h->P = P; h->N = N; h->n = 6 * C + 3 * P;
    h->N_total = N;
    h->ld = ld;
    h->forms = decide_problem_forms(C, P, N, f32, h->n_cu, tb.facts, h->dbg);   // THE decision: the facts are in
    CHK(allocate());
    CHK(upload_and_zero());
    CHK(enqueue_camera_major());
    const double tp3 = now_s();
    HIPCHK(h, hipStreamSynchronize(h->stream));     // the host tables are rebuilt by the next call
    if (timing)
        fprintf(stderr, "sfmba: set_problem  structure = run offsets + camera-major permutation %.2f ms, wave ranges %.2f ms, step table %.2f ms, "
                        "chunks + pair lists %.2f ms\n", 1e3 * (ts1 - tp1), 1e3 * (ts2 - ts1), 1e3 * (ts3 - ts2), 1e3 * (tp2 - ts3));
    if (timing)
        fprintf(stderr, "sfmba: set_problem  convert+compare %.2f ms  structure %.2f ms  allocate+enqueue %.2f ms  upload wait %.2f ms"
                        "  (%lld of %lld observations re-used)\n",
                1e3 * (tp1 - tp0), 1e3 * (tp2 - tp1), 1e3 * (tp3 - tp2), 1e3 * (now_s() - tp3), (long long)tb.fdiff, (long long)N);
    auto& prev = h->prev;
    if (tb.sorted) { prev.valid = true; prev.f32 = f32; prev.N = N; prev.P = P; }
    prev.packed = tb.sorted && h->forms.packed_upload;
    h->have_problem = true;
    return 0;
}

int set_problem_impl(sfmba_handle* h, int64_t C, int64_t P, int64_t N, const int64_t* cam, const int64_t* pt,
                     const double* uv, const int64_t* uv_i64, const double* K) {
    CHK(enter(h));
    ProblemBuild b{h, C, P, N, cam, pt, uv, uv_i64, K};
    return b.run();
}
}  // namespace

int sfmba_set_problem(sfmba_handle* h, int64_t C, int64_t P, int64_t N, const int64_t* cam, const int64_t* pt,
                      const double* uv, const double* K) {
    return set_problem_impl(h, C, P, N, cam, pt, uv, nullptr, K);
}

int sfmba_set_problem_i64(sfmba_handle* h, int64_t C, int64_t P, int64_t N, const int64_t* cam, const int64_t* pt,
                          const int64_t* uv, const double* K) {
    return set_problem_impl(h, C, P, N, cam, pt, nullptr, uv, K);
}

namespace {
// test / timing entries: x on the device, its camera table and point records, residual + Jacobian, normal blocks
int linearise_at(sfmba_handle* h, const double* x, bool blocks = true) {
    CHK(upload_x(h, x));
    CHK(launch_cam_table(h, h->x, h->tab, h->rec));
    int np = 0;
    CHK((launch_resjac<true, true>(h, h->x, h->tab, &np)));
    return blocks ? launch_normal_blocks(h, h->tab, h->rec) : 0;
}
// k_point_prep: V_p^-1 and the point records' z half outside a solve (inside one, k_prep does this work)
int launch_point_prep(sfmba_handle* h, const double* si_pts, const double* e_in, double reg, double* z_out, const double* pts, double* rhsrec) {
    hipLaunchKernelGGL(k_point_prep, dim3((h->P + 255) / 256), dim3(256), 0, h->stream, h->V.as<double>(),
                       h->gp.as<double>(), si_pts, e_in, (int)h->P, reg, vinv_ptr(h), z_out, pts, rhsrec);
    LAUNCHED(h);
    return 0;
}
}  // namespace

int sfmba_residuals(sfmba_handle* h, const double* x, double* r_out) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    if (!r_out) return fail(h, -1, "r_out is NULL");
    CHK(upload_x(h, x));
    CHK(launch_cam_table(h, h->x, h->tab, h->rec));
    int np = 0;
    CHK((launch_resjac<false, true>(h, h->x, h->tab, &np)));
    return download_residuals(h, r_out);
}

int sfmba_residual_jacobian(sfmba_handle* h, const double* x, double* r_out, double* Jc_out, double* Jp_out) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    if (!r_out || !Jc_out || !Jp_out) return fail(h, -1, "NULL output");
    CHK(upload_x(h, x));
    CHK(launch_cam_table(h, h->x, h->tab, h->rec));
    int np = 0;
    CHK((launch_resjac<true, true>(h, h->x, h->tab, &np, nullptr, nullptr, /*blocks=*/false)));   // (blocks = false: always stored)
    DevBuf jc_rm, jp_rm;
    HIPCHK(h, jc_rm.ensure(sizeof(double) * 12 * h->N));
    HIPCHK(h, jp_rm.ensure(sizeof(double) * 6 * h->N));
    hipLaunchKernelGGL(k_unpack_jac, dim3((h->N + 255) / 256), dim3(256), 0, h->stream, h->J.as<double>(),
                       (int)h->N, h->ld, h->f32 ? 1 : 0, jc_rm.as<double>(), jp_rm.as<double>());
    LAUNCHED(h);
    std::vector<double> tc(12 * h->N), tp(6 * h->N);
    CHK(download_residuals(h, r_out));
    HIPCHK(h, hipMemcpyAsync(tc.data(), jc_rm.p, sizeof(double) * 12 * h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(tp.data(), jp_rm.p, sizeof(double) * 6 * h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t k = 0; k < h->N; ++k) {
        const int64_t d = h->permuted ? h->tb.order[k] : k;
        memcpy(Jc_out + 12 * d, tc.data() + 12 * k, sizeof(double) * 12);
        memcpy(Jp_out + 6 * d, tp.data() + 6 * k, sizeof(double) * 6);
    }
    return 0;
}

int sfmba_normal_blocks(sfmba_handle* h, const double* x, double* U, double* V, double* gc, double* gp) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    CHK(linearise_at(h, x));
    std::vector<double> ugc(27 * h->C);
    HIPCHK(h, hipMemcpyAsync(ugc.data(), h->Ugc(), sizeof(double) * 27 * h->C, hipMemcpyDeviceToHost, h->stream));
    if (V) HIPCHK(h, hipMemcpyAsync(V, h->V.p, sizeof(double) * 6 * h->P, hipMemcpyDeviceToHost, h->stream));
    if (gp) HIPCHK(h, hipMemcpyAsync(gp, h->gp.p, sizeof(double) * 3 * h->P, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t c = 0; c < h->C; ++c) {
        if (U) memcpy(U + 21 * c, ugc.data() + 27 * c, sizeof(double) * 21);
        if (gc) memcpy(gc + 6 * c, ugc.data() + 27 * c + 21, sizeof(double) * 6);
    }
    return 0;
}

int sfmba_schur_matvec(sfmba_handle* h, const double* x, const double* dc, const double* dp, const double* v, double* y) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    if (!dc || !dp || !v || !y) return fail(h, -1, "NULL argument");
    CHK(linearise_at(h, x));
    // stage dp in e (as explicit diagonal), v in pk -- camera vectors are plane-major on the device
    const int64_t C = h->C;
    std::vector<double> vp(6 * C);
    for (int64_t c = 0; c < C; ++c)
        for (int k = 0; k < 6; ++k) vp[k * C + c] = v[6 * c + k];
    HIPCHK(h, hipMemcpyAsync(h->e.p, dp, sizeof(double) * 3 * h->P, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->vtmp.p, vp.data(), sizeof(double) * 6 * C, hipMemcpyHostToDevice, h->stream));
    CHK(launch_point_prep(h, nullptr, h->e.as<double>(), 0.0, nullptr, nullptr, nullptr));
    CHK(launch_mixed_prep(h, h->x, h->tab));
    CHK(schur_product_standalone(h, h->vtmp.as<double>()));
    CHK(exchange(h, h->acc(), 6 * C, 0));
    std::vector<double> a(6 * C);
    HIPCHK(h, hipMemcpyAsync(a.data(), h->acc(), sizeof(double) * 6 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t c = 0; c < C; ++c)
        for (int k = 0; k < 6; ++k) y[6 * c + k] = a[k * C + c] + dc[6 * c + k] * v[6 * c + k];
    HIPCHK(h, hipMemsetAsync(h->acc(), 0, sizeof(double) * 6 * C, h->stream));
    return 0;
}

int sfmba_step_products(sfmba_handle* h, const double* x, const double* sg, const double* dc, const double* dp_diag,
                        double* t1_out, double* g11_out, double* dp_out, double* sums_out, double* g_out, double* si_out) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    if (!sg || !dc || !dp_diag || !t1_out || !g11_out || !dp_out || !sums_out) return fail(h, -1, "NULL argument");
    if (!h->forms.one_rank) return fail(h, -1, "sfmba_step_products is a single-rank entry");
    const int64_t C = h->C, P = h->P, N = h->N;
    CHK(linearise_at(h, x));
    CHK(launch_update_scale(h, 1));                             // s, g of the point (and D^2 g, replaced by the caller's below)
    std::vector<double> planes(6 * C);
    for (int64_t c = 0; c < C; ++c)
        for (int k = 0; k < 6; ++k) planes[k * C + c] = dc[6 * c + k];
    HIPCHK(h, hipMemcpyAsync(h->sg_cur, sg, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->e.p, dp_diag, sizeof(double) * 3 * P, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->vtmp.p, planes.data(), sizeof(double) * 6 * C, hipMemcpyHostToDevice, h->stream));
    CHK(launch_point_prep(h, nullptr, h->e.as<double>(), 0.0, nullptr, nullptr, nullptr));
    int np1 = 0, np2 = 0;
    CHK(launch_jdot(h, &np1));
    std::vector<double> part1((size_t)np1), t1(h->f32 ? 0 : (size_t)2 * N);
    std::vector<float> t1f(h->f32 ? (size_t)2 * N : 0);        // 32-bit storage: t1 holds 2N floats, widened below
    HIPCHK(h, hipMemcpyAsync(part1.data(), partB(h), sizeof(double) * np1, hipMemcpyDeviceToHost, h->stream));
    CHK(launch_backsub(h, &np2, h->vtmp.as<double>()));
    std::vector<double> part2((size_t)np2 * kBacksubCols);
    HIPCHK(h, hipMemcpyAsync(part2.data(), partB(h), sizeof(double) * part2.size(), hipMemcpyDeviceToHost, h->stream));
    if (h->f32) HIPCHK(h, hipMemcpyAsync(t1f.data(), h->t1.p, sizeof(float) * 2 * N, hipMemcpyDeviceToHost, h->stream));
    else HIPCHK(h, hipMemcpyAsync(t1.data(), h->t1.p, sizeof(double) * 2 * N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(dp_out, h->p.as<double>() + 6 * C, sizeof(double) * 3 * P, hipMemcpyDeviceToHost, h->stream));
    if (g_out) HIPCHK(h, hipMemcpyAsync(g_out, h->g_cur, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    if (si_out) HIPCHK(h, hipMemcpyAsync(si_out, h->si_cur, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t k = 0; k < N; ++k) {
        const int64_t d = h->permuted ? h->tb.order[k] : k;
        if (h->f32) { t1_out[2 * d] = (double)t1f[2 * k]; t1_out[2 * d + 1] = (double)t1f[2 * k + 1]; }
        else { t1_out[2 * d] = t1[2 * k]; t1_out[2 * d + 1] = t1[2 * k + 1]; }
    }
    *g11_out = 0.0;                                             // the partial rows in the order the device sums them
    for (int b = 0; b < np1; ++b) *g11_out += part1[b];
    for (int k = 0; k < kBacksubCols; ++k) {
        sums_out[k] = 0.0;
        for (int b = 0; b < np2; ++b) sums_out[k] += part2[(size_t)b * kBacksubCols + k];
    }
    return 0;
}

int sfmba_rhs_precond(sfmba_handle* h, const double* x, const double* dc, const double* dp, double* rhs_out, double* sd_out,
                      double* minv_out) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    if (!dc || !dp || !rhs_out || !sd_out || !minv_out) return fail(h, -1, "NULL argument");
    // (32-bit storage with a recomputing pass A: the pass forms its blocks in fp64 from the camera table and the fp64 point
    // records and reads nothing rounded but the pixels behind g_p; with the stored Jacobian it rounds them: refused below)
    if (!h->forms.one_rank) return fail(h, -1, "sfmba_rhs_precond is a single-rank entry");
    if (!h->forms.precond) return fail(h, -1, "sfmba_rhs_precond needs the Schur-diagonal preconditioner (debug option precond)");
    if (h->forms.round_blocks) return fail(h, -1, "sfmba_rhs_precond: blocks rounded to fp32 are not the blocks its header states");
    const int64_t C = h->C, P = h->P;
    CHK(linearise_at(h, x));
    std::vector<double> planes(6 * C);
    for (int64_t c = 0; c < C; ++c)
        for (int k = 0; k < 6; ++k) planes[k * C + c] = dc[6 * c + k];
    HIPCHK(h, hipMemcpyAsync(h->e.p, dp, sizeof(double) * 3 * P, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->Dc.p, planes.data(), sizeof(double) * 6 * C, hipMemcpyHostToDevice, h->stream));
    // Vinv and e = Vinv g_p into the z half of the point records (and the 128-byte records of the form that gathers them)
    CHK(launch_point_prep(h, nullptr, h->e.as<double>(), 0.0, h->rec + 3, h->x + 6 * C,
                          h->forms.use_rhsrec ? h->rhsrec.as<double>() : (double*)nullptr));
    CHK(launch_rhs_and_preconditioner(h));
    std::vector<double> a(27 * C), m(21 * C);                   // acc | sd and Minv: plane-major over the cameras
    HIPCHK(h, hipMemcpyAsync(a.data(), h->acc(), sizeof(double) * 27 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(m.data(), h->Minv.p, sizeof(double) * 21 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t c = 0; c < C; ++c) {
        for (int k = 0; k < 6; ++k) rhs_out[6 * c + k] = a[k * C + c];
        for (int k = 0; k < 21; ++k) { sd_out[21 * c + k] = a[(6 + k) * C + c]; minv_out[21 * c + k] = m[k * C + c]; }
    }
    HIPCHK(h, hipMemsetAsync(h->acc(), 0, sizeof(double) * 6 * C, h->stream));
    return 0;
}

int sfmba_get_mixed_operands(sfmba_handle* h, double* origin, float* rt32, float* rec32, double* rtd) {
    CHK(enter(h));
    if (!h->have_problem) return fail(h, -1, "sfmba_set_problem has not been called");
    if (!h->forms.mixed) return fail(h, -1, "sfmba_get_mixed_operands: the problem does not run the mixed-precision product (form \"mixed\")");
    const size_t C = (size_t)h->C, P = (size_t)h->P;
    if (rt32) HIPCHK(h, hipMemcpyAsync(rt32, h->rt32.p, sizeof(float) * kRt32 * C, hipMemcpyDeviceToHost, h->stream));
    if (rec32) HIPCHK(h, hipMemcpyAsync(rec32, h->rec32.p, sizeof(float) * kRec32 * P, hipMemcpyDeviceToHost, h->stream));
    if (rtd) HIPCHK(h, hipMemcpyAsync(rtd, h->rtd.p, sizeof(double) * kRt32 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (origin) { origin[0] = h->origin.x; origin[1] = h->origin.y; origin[2] = h->origin.z; }
    return 0;
}

int sfmba_dense_schur(sfmba_handle* h, const double* x, const double* dc, const double* dp, const double* rhs,
                      double* S_out, double* sol_out) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    if (!dc || !dp || !rhs || !sol_out) return fail(h, -1, "NULL argument");
    if (!h->forms.dense) return fail(h, -1, "the dense reduced-camera path needs 6 * n_cameras <= %d", kDenseMaxN);
    const int64_t C = h->C;
    CHK(linearise_at(h, x));
    std::vector<double> ugc(27 * C), planes(6 * C), accp(6 * C);
    HIPCHK(h, hipMemcpyAsync(ugc.data(), h->Ugc(), sizeof(double) * 27 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t c = 0; c < C; ++c)
        for (int k = 0; k < 6; ++k) {
            planes[k * C + c] = dc[6 * c + k];
            accp[k * C + c] = -ugc[27 * c + 21 + k] - rhs[6 * c + k];      // the kernel solves S y = -g_c - acc
        }
    HIPCHK(h, hipMemcpyAsync(h->e.p, dp, sizeof(double) * 3 * h->P, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->Dc.p, planes.data(), sizeof(double) * 6 * C, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->acc(), accp.data(), sizeof(double) * 6 * C, hipMemcpyHostToDevice, h->stream));
    CHK(launch_point_prep(h, nullptr, h->e.as<double>(), 0.0, nullptr, nullptr, nullptr));
    CHK(launch_dense_solve(h, 1e-14, 40 * 6 * (int)C, /*rhs=*/false));   // (test entry: to the end, to be compared with a direct solve)
    std::vector<double> blk(36 * (size_t)h->n_blk), sol(6 * C);
    HIPCHK(h, hipMemcpyAsync(blk.data(), h->Sblk.p, sizeof(double) * blk.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(sol.data(), h->vecs.p, sizeof(double) * 6 * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t c = 0; c < C; ++c)
        for (int k = 0; k < 6; ++k) sol_out[6 * c + k] = sol[k * C + c];
    if (S_out) {
        const int64_t n = 6 * C;
        for (int64_t a = 0; a < C; ++a)
            for (int64_t b = a; b < C; ++b) {
                const double* B = blk.data() + 36 * (size_t)dense_block_index((int)a, (int)b, (int)C);
                for (int u = 0; u < 6; ++u)
                    for (int v = 0; v < 6; ++v) {
                        double val = -B[6 * u + v];
                        if (a == b) {
                            const int lo = std::min(u, v), hi = std::max(u, v);
                            val += ugc[27 * a + (lo * 6 - lo * (lo - 1) / 2 + (hi - lo))];
                            if (u == v) val += dc[6 * a + u];
                        }
                        S_out[(6 * a + u) * n + 6 * b + v] = val;
                        if (a != b) S_out[(6 * b + v) * n + 6 * a + u] = val;
                    }
            }
    }
    return 0;
}

int sfmba_time_kernel(sfmba_handle* h, const double* x, int32_t which, int32_t reps, double* avg_us) {
    CHK(enter(h));
    CHK(begin_compute(h, x));
    if (!avg_us || reps <= 0) return fail(h, -1, "bad reps / avg_us");
    if (which == 13 || which == 14) return stats_time_kernel(h, x, which, reps, avg_us);
    if (which == 15) return tri_time_kernel(h, x, reps, avg_us);
    if (which == 16) return resect_time_kernel(h, x, reps, avg_us);
    if (which == 17) return pnp_time_kernel(h, x, reps, avg_us);
    if (which == 18) return cov_time_kernel(h, x, reps, avg_us);
    if (which == 19) return tri_ransac_time_kernel(h, x, reps, avg_us);
    int np = 0;
    CHK(linearise_at(h, x, which >= 2));
    if (which >= 2) {
        CHK(launch_update_scale(h, 1));
        CHK(launch_point_prep(h, h->si_cur + 6 * h->C, nullptr, 1e-6, h->rec + 3, h->x + 6 * h->C,
                              h->forms.use_rhsrec ? h->rhsrec.as<double>() : (double*)nullptr));
        CHK(launch_mixed_prep(h, h->x, h->tab));
        // v = the camera slice of the gradient, as plane-major planes (and camera-major when v is not staged in LDS)
        hipLaunchKernelGGL(k_transpose, dim3((unsigned)((6 * h->C + 255) / 256)), dim3(256), 0, h->stream,
                           (const double*)h->g_cur, (int)h->C, 6, h->vtmp.as<double>(), (const PcgCtrl*)nullptr, 0);
        HIPCHK(h, hipMemcpyAsync(h->vcm.p, h->g_cur, sizeof(double) * 6 * h->C, hipMemcpyDeviceToDevice, h->stream));
        CHK(schur_product_standalone(h, h->vtmp.as<double>()));          // leaves a valid z for case 5
        if (which == 12) CHK(launch_jdot(h, &np));
    }
    return time_reps(h, reps, avg_us, [&]() -> int {
        switch (which) {
            case 0: CHK((launch_resjac<true, true>(h, h->x, h->tab, &np))); break;
            case 1: CHK((launch_resjac<false, false>(h, h->x, h->tab, &np))); break;
            case 2: CHK(launch_normal_blocks(h, h->tab, h->rec)); break;
            case 3: CHK(schur_product_standalone(h, h->vtmp.as<double>())); break;
            case 4: CHK(launch_pass_a<false>(h, (h->forms.lds_vec || h->forms.sweep_rc || h->forms.sweep_rc_g) ? h->vtmp.as<double>() : h->vcm.as<double>(), nullptr, 0)); break;
            case 5: CHK(launch_cam_schur<0>(h, h->vtmp.as<double>(), nullptr, 0)); break;
            case 6: CHK(launch_cam_schur<1>(h, nullptr, nullptr, 0)); break;
            case 7: CHK((launch_resjac<true, true>(h, h->x, h->tab, &np, nullptr, nullptr, /*blocks=*/false))); break;
            case 8:    // reduced right-hand side + Schur-diagonal blocks (without the 6x6 inverses)
                if (h->forms.xcd_cam) { CHK(launch_rhs_and_preconditioner(h)); break; }      // (wave-per-chunk form: with combine + inverses)
                hipLaunchKernelGGL((k_cam_rhs_diag<false>), dim3(h->n_chunks), dim3(kRhsThreads), 0, h->stream, cam_major(h),
                                   (const double*)h->tab, (const double*)h->rec, (const double*)vinv_ptr(h), h->K, (int)h->C,
                                   h->acc(), h->cam_partial.as<double>(), RhsPrecond{nullptr, nullptr, nullptr},
                                   h->forms.use_rhsrec ? (const double*)h->rhsrec.as<double>() : (const double*)nullptr, CamExchange{});
                LAUNCHED(h);
                break;
            case 11: CHK(launch_jdot(h, &np)); break;                                   // the selected form (rc_consumers)
            case 12: CHK(launch_backsub(h, &np, h->vtmp.as<double>())); break;         // after one k_jdot (below): t1 is valid
            case 10:   // streaming-store ceiling: fill the Jacobian planes, 16 B per lane, one stream
                hipLaunchKernelGGL(k_fill16, dim3(h->n_cu * 2), dim3(1024), 0, h->stream, h->J.as<double>(),
                                   (int64_t)((h->f32 ? 3 : 6) * h->ld), 1.0);
                break;
            default: return fail(h, -1, "unknown kernel id %d", which);
        }
        return 0;
    });
}

namespace {
// One sfmba_solve call: the state its phases share, and the phases in the order run() goes through them.
// Host/device hand-offs per outer iteration: ONE read-back after the whole linear phase
// (Cauchy product, Schur PCG, back-substitution, Gram/dot reductions are enqueued without the
// host seeing intermediate values: the regularisation term is computed by k_prep on the device
// and the PCG stops itself through its device-side control block) and ONE per trial step.
struct Solve {
    sfmba_handle* const h;
    const sfmba_options opt;
    sfmba_result* const out;
    const Forms& f = h->forms;
    const int64_t C = h->C, P = h->P, n = h->n;
    const int64_t max_nfev = opt.max_nfev > 0 ? opt.max_nfev : 100 * (6 * C + 3 * P);
    const double m_total = 2.0 * (double)h->N_total;
    double* const sc = h->scal();
    const double* const hs = h->h_scal;                         // the scalars as last brought to the host
    struct EventList : std::vector<std::pair<hipEvent_t, hipEvent_t>> {     // destroyed on every exit path
        ~EventList() { for (auto& pr : *this) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); } }
    } evs;                                                      // opt.profile: one pair per K1 launch
    int np_cost = 0;                                            // partial rows of the last K1 launch
    int np_tail = 0;                                            // ... of the last k_backsub launch
    double cost = 0.0, Delta = -1.0;
    unsigned long long start_seq = 0;                           // quick start: the post the host still has to wait for
    int64_t nfev = 1, njev = 1, iteration = 0, pcg_total = 0, pcg_breakdowns = 0;
    int status = -1;
    double step_norm = 0.0, actual_reduction = 0.0, g_norm = 0.0, reg_term = 0.0, cost_new = 0.0;
    bool have_red = false;
    // the record of PCG counts and the guess taken from it
    int pcg_guess = h->pcg_hint;                                // iterations to enqueue without reading back
    bool guess_exact = false;                                   // pcg_guess comes from the record: no spare launch
    bool hist_same = false;
    unsigned long long sig = 0;
    std::vector<int> pcg_hist_new;
    int pcg_enqueued = 0;
    bool missed = false;
    PcgCtrl hc{};                                               // control block of this iteration's PCG, as handed off
    bool nb_valid = true;                                       // V, g_p, [U|g_c] (and, single-buffered, J and r) belong to h->x
    // Single-buffered Jacobian: the trial point is evaluated into the SAME J / r buffers the sweeps of
    // this iteration have just read, so K1's stores land on lines that are still resident in the
    // Infinity Cache instead of cold ones.  A rejected step leaves J / r describing the rejected point;
    // nothing uses them before the next trial overwrites them, except the rare exits handled below.
    Mailbox trial_post{};                                       // one rank: the post that rides with the trial point's K3
    bool trial_post_pending = false;
    bool result_sent = false;                                   // x is already on its way to h_x (ev_copied[0])
    double t_begin = 0.0, t_dev0 = 0.0, t_sent0 = 0.0, t_sent1 = 0.0;

    int run(const double* x_start, double* x_out);
    // the phases, in order, and what they share
    int start(const double* x_start), start_values();
    void recall_pcg_record(const double* x_start);
    int linear_phase(), tail();
    int device_trial();
    void record_pcg_count();
    int step_loop(), accept_or_reject(), terminate();
    int deliver(double* x_out);
    int eval_jac(const double* x, double* tab, bool table_ready, bool finish = true);
    int enqueue_trial(const double* coef_dev, double c1, double c2), handoff(bool with_ctrl);
    int fetch() {                                               // the scalars of a post that has arrived
        CHK(wait_mailbox(h, h->mbox_seq));
        memcpy(h->h_scal, h->mbox, sizeof(double) * kScalSlots);
        return 0;
    }
    double qsum(int q) const { return hs[kPointSlot[q]] + hs[kCamSlot + q]; }   // camera slice + (rank-reduced) point slice
    int guess_launches() const { return pcg_guess + (f.pcg_fused ? 1 : 0) + (guess_exact ? 0 : 1); }
};

// K0 + K1, sum r^2 -> the cost slot
int Solve::eval_jac(const double* x, double* tab, bool table_ready, bool finish) {
    if (!table_ready) CHK(launch_cam_table(h, x, tab, h->rec, f.quick_start));
    if (opt.profile) {
        hipEvent_t a, b;
        // timing-only events (hip_runtime_api.h: hipEventDisableSystemFence): no system-scope cache write-back and
        // invalidation when they are recorded, which otherwise lands inside the measured interval (+1.3 us)
        // and delays the launches around the kernel
        HIPCHK(h, hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
        if (hipEventCreateWithFlags(&b, hipEventDisableSystemFence) != hipSuccess) {
            (void)hipEventDestroy(a);
            return fail(h, -3, "hipEventCreateWithFlags failed");
        }
        evs.emplace_back(a, b);
        CHK((launch_resjac<true, true>(h, x, tab, &np_cost, a, b)));
    } else {
        CHK((launch_resjac<true, true>(h, x, tab, &np_cost)));
    }
    if (finish) CHK(launch_finish(h, sum_rider(h, h->part.as<double>(), np_cost, kCostSlot), h->skip, h->post));
    return 0;
}

int Solve::start_values() {                                     // cost0 is on the host
    cost = 0.5 * hs[kCostSlot];
    if (!std::isfinite(cost)) return fail(h, -2, "Residuals are not finite in the initial point.");
    out->cost0 = cost;
    out->rmse0 = std::sqrt(2.0 * cost / m_total);
    return 0;
}

// upload, f0, J0 (least_squares.py:838, 903-912)
int Solve::start(const double* x_start) {
    h->solved = false;
    h->skip = nullptr; h->post = Mailbox{};
    h->pending_scale_sums = false;
    h->p2p.first_in_solve = true;
    if (h->dbg.p2p_delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(h->dbg.p2p_delay_ms));
    t_begin = now_s();
    h->x = h->xa.as<double>(); h->x_new = h->xb.as<double>();
    h->tab = h->tabA.as<double>(); h->tab_new = h->tabB.as<double>();
    h->rec = h->recA.as<double>(); h->rec_new = h->recB.as<double>();
    CHK(upload_x(h, x_start));
    h->mirror_on = h->copy_stream != nullptr && n >= 2000000;           // (see the note at copy_stream)
    h->x_tag = 0; h->mirror_tag[0] = h->mirror_tag[1] = 0;
    if (h->mirror_on) {
        HIPCHK(h, h->mirror[0].ensure(sizeof(double) * n, 0));
        HIPCHK(h, h->mirror[1].ensure(sizeof(double) * n, 0));
    }
    HIPCHK(h, hipMemsetAsync(sc + kGhPrevSlot, 0, 2 * sizeof(double), h->stream));   // forcing-term memory of k_prep
    t_dev0 = now_s();
    report_stall(h, "upload_x", t_dev0 - t_begin);
    if (f.quick_start) {
        // No blocking hand-off: the launches take the form of a trial evaluation (the cost sum and its post ride with
        // K3), k_update_scale's sums ride with the first k_jdot, and k_prep / k_tr_step derive the first radius from
        // the exchange scalars themselves (Delta < 0).  The host picks the cost up behind the k_jdot launch
        // (linear_phase) and the radius at the first regular hand-off.
        CHK(eval_jac(h->x, h->tab, false, /*finish=*/false));
        start_seq = ++h->mbox_seq;
        CHK(launch_normal_blocks(h, h->tab, h->rec, np_cost, Mailbox{h->mbox_dev, sc, nullptr, start_seq, p2p_error_word(h)}));
        return launch_update_scale(h, 1, /*defer=*/true);
    }
    CHK(eval_jac(h->x, h->tab, false));
    CHK(exchange(h, sc + kCostSlot, 1, 0));                     // sum r^2
    CHK(launch_normal_blocks(h, h->tab, h->rec));               // normal blocks, scale, gradient, q0..q4 at h->x
    CHK(launch_update_scale(h, 1));
    CHK(exchange_linearise(h));
    CHK(fetch_scalars(h));
    CHK(start_values());
    Delta = std::sqrt(qsum(2));                                 // |x0 * scale_inv|, trf.py:428
    if (Delta == 0.0) Delta = 1.0;
    return 0;
}

// The record is trusted count for count only on the problem it was recorded on; on a neighbouring problem (the
// reference's growing reconstruction: a camera or a few hundred observations more) it is a guess with a spare
// launch; on an unrelated problem it is dropped together with the running hint.
// (content, not only sizes: the problem arrays' generation and a checksum of the start vector -- a different start on
// the same problem, or another problem of the same sizes, is a "neighbouring" one and gets the spare launch)
void Solve::recall_pcg_record(const double* x_start) {
    sig = h->problem_gen * 0x9E3779B97F4A7C15ull;
    const int64_t stride = std::max<int64_t>(1, n / 509);
    for (int64_t k = 0; k < n; k += stride) {
        unsigned long long bits;
        memcpy(&bits, x_start + k, sizeof bits);
        sig = (sig ^ bits) * 0x100000001B3ull;
    }
    hist_same = h->hist_C == C && h->hist_P == P && h->hist_N == h->N && h->hist_sig == sig;
    const bool hist_near = hist_same || (h->hist_N > 0 && std::llabs(h->hist_C - C) <= 1 && 2 * h->N >= h->hist_N && h->N <= 2 * h->hist_N);
    if (!hist_near) { h->pcg_hist.clear(); h->pcg_hint = 0; pcg_guess = 0; }
    if (!h->pcg_hist.empty() && h->pcg_hist[0] > 0) { pcg_guess = h->pcg_hist[0]; guess_exact = hist_same; }
}

// ---- enqueue the whole linear phase ---------------------------------------------------
// Final sums of per-workgroup partials are not launches of their own where a neighbour can carry
// them: k_update_scale's ride with k_jdot; on a single rank k_jdot's are repeated by every workgroup
// of k_prep and k_backsub's are done by k_tr_step (with several
// ranks the all-reduce has to sit between producer and consumer, so those two stay launches).
int Solve::linear_phase() {
    if (!nb_valid) {                                            // a rejected trial overwrote the blocks and no
        CHK(eval_jac(h->x, h->tab, true));                      // step was accepted afterwards
        CHK(launch_normal_blocks(h, h->tab, h->rec));           // (nfev limit)
        nb_valid = true;
    }
    int np = 0;
    const bool scale_sums_rode = h->pending_scale_sums;
    CHK(launch_jdot(h, &np));                                   // t1 = J D^2 g, G11 = |t1|^2
    if (start_seq != 0) {                                       // quick start: cost0 was posted by K3 a while ago
        start_seq = 0;
        CHK(fetch());
        CHK(start_values());
    }
    if (!f.one_rank && h->p2p.ready) {
        // direct path: the collective's own workgroup first sums k_jdot's partials into slot 1, then reduces
        // slots 1..12 over the ranks when an accepted step left fresh q1..q4 (8..11, sums) and max|g| (12, a
        // maximum by the mask), G11 alone otherwise.  Slots 2..7 (G12, G22, q5..q8 of the previous iteration)
        // are summed once more along the way; nothing reads them before k_backsub's sums rewrite them.
        const Piggyback pb = sum_rider(h, partB(h), np, kG11Slot);
        static_assert(kMaxSlot == 12 && kG11Slot == 1, "mask below assumes the maximum sits at the end of the run");
        CHK(p2p_allreduce(h, sc + kG11Slot, scale_sums_rode ? kMaxSlot : 1, 0, nullptr,
                          scale_sums_rode ? 1ull << (kMaxSlot - 1) : 0ull, &pb));
        ++h->n_collectives;
    } else if (!f.one_rank) {
        CHK(launch_finish(h, sum_rider(h, partB(h), np, kG11Slot), h->skip, h->post));
        if (scale_sums_rode) CHK(exchange_linearise(h));        // q1..q4, max|g| of the accepted point
        CHK(exchange(h, sc + kG11Slot, 1, 0));
    }
    {   // regularisation (trf.py:471-475), Vinv/e per point, Dc/Minv per camera, acc0 = 0: one launch
        const int bc = (int)((C + 63) / 64), bp = (int)((P + 63) / 64);
        hipLaunchKernelGGL(k_prep, dim3(bc + bp), dim3(64), 0, h->stream, sc, Delta, opt.reg_min, h->Ugc(),
                           h->V.as<double>(), h->gp.as<double>(), h->si_cur, (int)C, (int)P, bc,
                           h->Dc.as<double>(), (f.precond ? (double*)nullptr : h->Minv.as<double>()),
                           vinv_ptr(h), h->rec + 3,
                           f.one_rank ? (const double*)partB(h) : (const double*)nullptr, np, opt.pcg_tol,
                           std::max(opt.pcg_tol, opt.pcg_tol_max), (const double*)(h->x + 6 * C),
                           (f.use_rhsrec && !f.dense_solve) ? h->rhsrec.as<double>() : (double*)nullptr,   // (read by k_cam_rhs_diag only)
                           f.dense_solve ? MixedPrep{nullptr, nullptr, nullptr, nullptr, Origin{0.0, 0.0, 0.0}} : mixed_prep(h, h->tab));
        LAUNCHED(h);
    }
    hc = PcgCtrl{};
    pcg_enqueued = 0;
    if (f.dense_solve) {
        // few cameras: the reduced rhs term and the preconditioner blocks are formed inside launch_dense_solve, and
        // the same PCG runs inside one workgroup; an iteration there costs a twentieth of the two launches of the
        // implicit product, so the forcing term is a decade tighter (cfg2: 5 outer iterations instead of 7)
        CHK(launch_dense_solve(h, kDenseTolFactor * opt.pcg_tol, pcg_max_iters(h, opt), /*rhs=*/true));
        return tail();
    }
    CHK(launch_rhs_and_preconditioner(h));                      // reduced rhs term -> acc, preconditioner blocks
    CHK(pcg_start(h, opt));                                     // replaces lsmr, trf.py:477-480
    if (pcg_guess > 0) {
        // speculative: no read-back; surplus launches are no-ops.  Fused launches apply the update of
        // iteration k in launch k + 1, so k iterations need k + 1 launches; one spare either way.
        pcg_enqueued = guess_launches();
        CHK(pcg_enqueue(h, pcg_enqueued, true));
    } else {
        CHK(pcg_finish_polling(h, opt, &hc));
    }
    return tail();
}

// back-substitution + model products (all in k_backsub); k_tr_step follows and (single rank) sums k_backsub's
// partial rows itself
int Solve::tail() {
    CHK(launch_backsub(h, &np_tail));
    if (!f.one_rank && h->p2p.ready) {                          // the sums run inside the collective's workgroup
        const Piggyback pb = backsub_rider(h, np_tail);
        CHK(p2p_allreduce(h, sc + kTailSlot, 6, 0, nullptr, 0, &pb));
        ++h->n_collectives;
        return 0;
    }
    if (!f.one_rank) CHK(launch_finish(h, backsub_rider(h, np_tail)));
    return exchange(h, sc + kTailSlot, 6, 0);                   // G12, G22, q5..q8
}

// the trial point x + step (coefficients from the device, or c1, c2) and its evaluation
int Solve::enqueue_trial(const double* coef_dev, double c1, double c2) {
    const int bc = (int)((C + 255) / 256);
    hipLaunchKernelGGL(k_step_table, dim3(bc + grid_1d(3 * P, 256, 2048)), dim3(256), 0, h->stream, h->x,
                       h->sg_cur, h->p.as<double>(), c1, c2, coef_dev, (int)C, n, bc, h->K, h->x_new,
                       h->tab_new, h->rec_new, h->skip);
    LAUNCHED(h);
    if (h->mirror_on) {                                         // x_new to its host mirror, beside the evaluation below
        const int w = h->x_new == h->xa.as<double>() ? 0 : 1;
        HIPCHK(h, hipEventRecord(h->ev_written, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->ev_written, 0));
        HIPCHK(h, hipMemcpyAsync(h->mirror[w].p, h->x_new, sizeof(double) * n, hipMemcpyDeviceToHost, h->copy_stream));
        HIPCHK(h, hipEventRecord(h->ev_copied[w], h->copy_stream));
        h->mirror_tag[w] = ++h->copy_count;
    }
    // the trial point is evaluated WITH its Jacobian, into the same buffers: when
    // the step is accepted (the common case) nothing has to be recomputed
    // The cost reduction that ends the evaluation also posts the hand-off (scalars + PCG control
    // block) into the host mailbox; with several ranks the post follows the all-reduce of the cost.
    const Mailbox mb{h->mbox_dev, sc, h->ctrl.as<PcgCtrl>() + (h->pcg_L & 1), ++h->mbox_seq, p2p_error_word(h)};
    if (!f.one_rank && h->p2p.ready) {
        // direct path: ONE single-workgroup launch sums K1's cost partials, reduces the cost over the
        // ranks and posts the hand-off (or only posts, when k_tr_step cancelled the trial)
        CHK(eval_jac(h->x_new, h->tab_new, true, /*finish=*/false));
        const Piggyback pb = sum_rider(h, h->part.as<double>(), np_cost, kCostSlot);
        CHK(p2p_allreduce(h, sc + kCostSlot, 1, 0, nullptr, 0, &pb, &mb, h->skip));
        ++h->n_collectives;
        return 0;
    }
    if (f.one_rank && !f.cost_rider) {
        h->post = mb;
        const int rc = eval_jac(h->x_new, h->tab_new, true);
        h->post = Mailbox{};
        return rc;
    }
    if (f.one_rank) {
        // single rank: the cost sum and the post ride with the launch that builds the trial point's blocks
        // (handoff), one launch less per iteration
        CHK(eval_jac(h->x_new, h->tab_new, true, /*finish=*/false));
        trial_post = mb;
        trial_post_pending = true;
        return 0;
    }
    CHK(eval_jac(h->x_new, h->tab_new, true));
    CHK(exchange(h, sc + kCostSlot, 1, 0));
    hipLaunchKernelGGL(k_post, dim3(1), dim3(64), 0, h->stream, mb);
    LAUNCHED(h);
    return 0;
}

// While the host waits, the GPU already builds the normal-equation blocks of the trial point
// (speculating on acceptance, the common case).  They overwrite V / g_p / [U|g_c], which a
// rejected step does not need: a retry only re-solves the 2-D model (host scalars) and
// re-applies k_step_table to x, D^2 g and p, all untouched.
int Solve::handoff(bool with_ctrl) {
    if (trial_post_pending) CHK(launch_normal_blocks(h, h->tab_new, h->rec_new, np_cost, trial_post));
    else CHK(launch_normal_blocks(h, h->tab_new, h->rec_new));
    trial_post_pending = false;
    nb_valid = false;
    // ... and, behind them, scale, gradient and partial sums of the trial point into the second buffer set
    if (f.spec_scale) CHK(launch_update_scale(h, 0, /*defer=*/true, /*speculative=*/true));
    CHK(fetch());
    if (with_ctrl) memcpy(&hc, h->mbox + kMboxCtrl, sizeof hc);
    return 0;
}

// ---- the first trial step is decided ON THE DEVICE (k_tr_step) and evaluated right away -------
// so that an outer iteration hands control to the host ONCE, after the trial cost is known.
int Solve::device_trial() {
    missed = false;
    for (bool speculative = pcg_guess > 0 || f.dense_solve;;) {        // dense: the control block always says "finished"
        hipLaunchKernelGGL(k_tr_step, dim3(1), dim3(f.one_rank ? 1024 : 64), 0, h->stream, sc, Delta,
                           speculative ? (const PcgCtrl*)(h->ctrl.as<PcgCtrl>() + (h->pcg_L & 1)) : (const PcgCtrl*)nullptr,
                           f.one_rank ? backsub_rider(h, np_tail) : Piggyback{});
        LAUNCHED(h);
        h->skip = sc + kSkipSlot;                               // k_tr_step's verdict gates every launch below
        int rc_trial = enqueue_trial(sc + kStepSlot, 0.0, 0.0);
        if (rc_trial == 0) rc_trial = handoff(speculative);     // THE hand-off of this iteration
        h->skip = nullptr;
        CHK(rc_trial);
        if (!(speculative && hc.done == 0)) break;
        // The PCG needed more iterations than were enqueued.  k_tr_step saw that on the device and
        // cancelled the trial launches, so J, r and the normal blocks still describe x: finish the
        // PCG (host-polled), redo the tail and decide the step on the device again -- the arithmetic of
        // an iteration does not depend on whether its guess sufficed.
        missed = true;
        nb_valid = true;
        if (opt.profile && !evs.empty()) {                      // the cancelled launch is not a K1 timing sample
            (void)hipEventDestroy(evs.back().first);
            (void)hipEventDestroy(evs.back().second);
            evs.pop_back();
        }
        CHK(pcg_finish_polling(h, opt, &hc));
        CHK(tail());
        speculative = false;
    }
    // hc.done == 3: the CG recurrences lost positive definiteness (rounding, typically on a converged
    // system whose right-hand side is noise).  The iterate of the last good step is kept -- it is
    // zero when the very first step failed, in which case the 2-D model degenerates to the
    // steepest-descent line, exactly scipy's fallback when gn_h adds nothing to span(g_h).
    if (hc.done == 3) ++pcg_breakdowns;
    if (Delta < 0.0) Delta = hs[kRadiusSlot];                   // quick start: the radius k_tr_step derived and used
    return 0;
}

// Next guess: the largest recent count, forgotten by one iteration per outer iteration.  A surplus
// iteration costs two empty launches (~10 us); a miss costs a hand-off per polled batch.
void Solve::record_pcg_count() {
    pcg_total += hc.iters;
    if (h->dbg.trace_pcg && f.dense_solve)
        fprintf(stderr, "sfmba: iteration %lld: PCG in LDS, %d iterations, outcome %d, reg %.3e\n", (long long)iteration,
                hc.iters, hc.done, hs[kRegSlot]);
    else if (h->dbg.trace_pcg)
        fprintf(stderr, "sfmba: iteration %lld: PCG enqueued %d, needed %d%s\n", (long long)iteration,
                pcg_enqueued, hc.iters, missed ? " (miss)" : "");
    h->pcg_hint = std::max(hc.iters, h->pcg_hint - 1);
    pcg_hist_new.push_back(hc.iters);
    const int bias = h->dbg.pcg_guess_bias;                     // test hook (sfmba_debug_option)
    const int rec = (iteration + 1 < (int64_t)h->pcg_hist.size()) ? h->pcg_hist[iteration + 1] : 0;
    guess_exact = rec > 0 && bias == 0 && hist_same;
    pcg_guess = std::max(1, (guess_exact ? rec : h->pcg_hint) + bias);
    reg_term = hs[kRegSlot];
}

// trf.py:488: the first trial was decided and evaluated on the device (device_trial); a retry after a rejected step
// (or fallback) is solved on the host from the same 2-D model
int Solve::step_loop() {
    const double x_norm = std::sqrt(qsum(3));
    const TrModel model = tr_build_model(hs[kG11Slot], hs[kTailSlot], hs[kTailSlot + 1], qsum(1), qsum(5), qsum(6), qsum(4),
                                         qsum(7), qsum(8));
    actual_reduction = -1.0;
    cost_new = cost;
    for (bool first = true; actual_reduction <= 0.0 && nfev < max_nfev; first = false) {
        TrStep st;
        if (first) {
            st.c1 = hs[kStepSlot]; st.c2 = hs[kStepSlot + 1]; st.predicted = hs[kStepSlot + 2];
            st.step_h_norm = hs[kStepSlot + 3]; st.step_norm = hs[kStepSlot + 4];
        } else {
            st = tr_solve_step(model, Delta);
            CHK(enqueue_trial(nullptr, st.c1, st.c2));
            CHK(handoff(false));
        }
        ++nfev;
        cost_new = 0.5 * hs[kCostSlot];
        if (!std::isfinite(cost_new)) {                         // trf.py:504-506
            Delta = 0.25 * st.step_h_norm;
            continue;
        }
        actual_reduction = cost - cost_new;
        double ratio;
        const double Delta_new = update_tr_radius(Delta, actual_reduction, st.predicted, st.step_h_norm,
                                                  st.step_h_norm > 0.95 * Delta, &ratio);
        step_norm = st.step_norm;
        const int term = check_termination(actual_reduction, cost, step_norm, x_norm, ratio, opt.ftol, opt.xtol);
        if (term != 0) { status = term; break; }
        Delta = Delta_new;
    }
    have_red = true;
    return 0;
}

int Solve::accept_or_reject() {
    if (!(actual_reduction > 0.0)) {
        step_norm = 0.0;
        actual_reduction = 0.0;
        return 0;
    }
    std::swap(h->x, h->x_new);                                  // trf.py:528
    std::swap(h->tab, h->tab_new);
    std::swap(h->rec, h->rec_new);
    h->x_tag = h->mirror_tag[h->x == h->xa.as<double>() ? 0 : 1];      // (0 when no mirror copy was made)
    nb_valid = true;                                            // J, f and the normal blocks of the accepted
                                                                // point are already there / in flight
    cost = cost_new;
    ++njev;
    if (status != -1 && f.early_download && !h->mirror_on) {
        // The solve ends on this point.  x was written by k_step_table, which the stream ran before the K1 / K3
        // whose post the host has just read, and nothing from here on writes it: the result leaves on the copy
        // stream now, beside what is left of K3, k_update_scale, the final sums and the last post.
        CHK(ensure_h_x(h));
        t_sent0 = now_s();
        // (in ONE piece: two halves, the first half's pinned -> pageable copy beside the second half's transfer,
        // measured 1.805-1.822 ms per cfg4 solve against 1.792-1.849 -- no gain, two blit launches)
        HIPCHK(h, hipMemcpyAsync(h->h_x, h->x, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->copy_stream));
        HIPCHK(h, hipEventRecord(h->ev_copied[0], h->copy_stream));
        h->result_in_flight = true;
        result_sent = true;
        t_sent1 = now_s();
    }
    if (!f.spec_scale) return launch_update_scale(h, 0, /*defer=*/true);
    std::swap(h->g_cur, h->g_new);                              // already enqueued behind K3 (handoff): take its outputs
    std::swap(h->si_cur, h->si_new);
    std::swap(h->sg_cur, h->sg_new);
    h->pending_scale_sums = true;                               // its final sums ride with the next k_jdot and
    return 0;                                                   // are read with the next hand-off
}

int Solve::terminate() {                                        // terminated inside the step loop
    if (h->pending_scale_sums) {                                // no k_jdot follows
        CHK(flush_scale_sums(h));
        CHK(exchange_linearise(h));
    }
    CHK(fetch_scalars(h));
    g_norm = std::max(hs[kMaxSlot], hs[kCamSlot + 0]);
    if (opt.verbose >= 2) print_iter(h, iteration, nfev, cost, have_red, actual_reduction, step_norm, g_norm);
    return 0;
}

// the result vector into the caller's array, the record of this solve, the result struct
int Solve::deliver(double* x_out) {
    if (!nb_valid) {                                            // last trial was not accepted: result.fun is f(x)
        int np = 0;
        CHK((launch_resjac<false, true>(h, h->x, h->tab, &np)));
    }
    CHK(ensure_h_x(h));
    const double t_dl0 = now_s();
    const int xw = h->x == h->xa.as<double>() ? 0 : 1;
    const bool mirrored = h->mirror_on && h->x_tag != 0 && h->mirror_tag[xw] == h->x_tag;     // x is on the host already
    const size_t xbytes = sizeof(double) * (size_t)n;
    if (!mirrored && !result_sent) HIPCHK(h, hipMemcpyAsync(h->h_x, h->x, xbytes, hipMemcpyDeviceToHost, h->stream));
    if (h->p2p.ready)                                           // did a direct all-reduce give up waiting for a peer?
        HIPCHK(h, hipMemcpyAsync(h->h_scal + kPinP2pErr, h->p2p.words + 1, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    // (result_sent: the last launch of the stream is the k_post whose post fetch_scalars has waited for; the query
    // still lets the runtime retire the solve's launches while the copy is in flight)
    CHK(wait_stream(h));
    const double t_ws = now_s();
    if (result_sent) {
        CHK(wait_stream(h, h->ev_copied[0]));
        h->result_in_flight = false;
    }
    if (mirrored) HIPCHK(h, hipEventSynchronize(h->ev_copied[xw]));
    const double t_dl1 = now_s();
    if (h->p2p.ready) {
        unsigned err = 0;
        memcpy(&err, h->h_scal + kPinP2pErr, sizeof err);
        if (err != 0) return p2p_timed_out(h, err);
    }
    staging_copy(h, x_out, mirrored ? h->mirror[xw].p : (const void*)h->h_x, xbytes);
    if (h->mirror_on) HIPCHK(h, hipStreamSynchronize(h->copy_stream));     // (a copy of a rejected last trial may still run)
    const double t_end = now_s();
    if (h->dbg.trace_timing && result_sent)
        fprintf(stderr, "sfmba: early result copy: enqueue %.1f us, then %.1f us to the last post, stream query %.1f us, copy event %.1f us\n",
                1e6 * (t_sent1 - t_sent0), 1e6 * (t_dl0 - t_sent1), 1e6 * (t_ws - t_dl0), 1e6 * (t_dl1 - t_ws));
    if (h->dbg.trace_timing)
        fprintf(stderr, "sfmba: solve  %.3f ms total, upload %.1f us, result: copy + wait %.1f us, staging copy %.1f us\n", 1e3 * (t_end - t_begin),
                1e6 * (t_dev0 - t_begin), 1e6 * (t_dl1 - t_dl0), 1e6 * (t_end - t_dl1));
    if (!evs.empty()) {
        double tot = 0.0;
        for (auto& pr : evs) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) tot += ms;
        }
        out->resjac_avg_us = 1e3 * tot / (double)evs.size();
        out->resjac_launches = (int64_t)evs.size();
    }
    h->pcg_hist.swap(pcg_hist_new);
    h->hist_C = C; h->hist_P = P; h->hist_N = h->N; h->hist_sig = sig;
    out->cost = cost;
    out->optimality = g_norm;
    out->rmse = std::sqrt(2.0 * cost / m_total);
    out->nfev = nfev; out->njev = njev; out->iterations = iteration; out->pcg_iterations = pcg_total;
    out->status = status == -1 ? 0 : status;
    out->seconds_total = t_end - t_begin;
    out->seconds_device = t_end - t_dev0;
    out->last_step_norm = step_norm;
    out->last_reg = reg_term;
    out->reserved = (int32_t)pcg_breakdowns;
    h->solved = true;
    return 0;
}

int Solve::run(const double* x_start, double* x_out) {
    CHK(start(x_start));
    recall_pcg_record(x_start);
    if (opt.verbose >= 2) print_header(h);
    for (;;) {                                                  // trf.py:450
        CHK(linear_phase());
        CHK(device_trial());
        // ---- loop head of trf.py:450-459, evaluated now that the scalars are on the host -----------
        g_norm = std::max(hs[kMaxSlot], hs[kCamSlot + 0]);
        if (g_norm < opt.gtol) status = 1;
        if (opt.verbose >= 2) print_iter(h, iteration, nfev, cost, have_red, actual_reduction, step_norm, g_norm);
        if (status != -1 || nfev >= max_nfev || (opt.max_iter > 0 && iteration >= opt.max_iter)) break;
        record_pcg_count();
        CHK(step_loop());
        CHK(accept_or_reject());
        ++iteration;
        if (status != -1) { CHK(terminate()); break; }
    }
    return deliver(x_out);
}

int solve_impl(sfmba_handle* h, const double* x_start, double* x_inout, const sfmba_options* opt_in, sfmba_result* out) {
    CHK(enter(h));
    CHK(begin_compute(h, x_start));
    if (!x_inout) return fail(h, -1, "x_out is NULL");
    if (!out) return fail(h, -1, "result is NULL");
    sfmba_options opt;
    if (opt_in) opt = *opt_in; else sfmba_default_options(&opt);
    memset(out, 0, sizeof *out);
    Solve s{h, opt, out};
    return s.run(x_start, x_inout);
}
}  // namespace

int sfmba_solve(sfmba_handle* h, double* x_inout, const sfmba_options* opt_in, sfmba_result* out) {
    return sfmba_solve_from(h, x_inout, x_inout, opt_in, out);
}

int sfmba_solve_from(sfmba_handle* h, const double* x0, double* x_out, const sfmba_options* opt_in, sfmba_result* out) {
    const int rc = solve_impl(h, x0, x_out, opt_in, out);
    if (rc != 0 && h) {
        // Leave the handle reusable: drain what was enqueued (speculative launches may still be in flight) and,
        // after a collective failure, unmap the peers -- sequence numbers no longer agree across ranks, so the
        // direct link is dead; the transport registered before it (RCCL / callback) serves later solves.
        const std::string msg = h->err;
        h->skip = nullptr; h->post = Mailbox{};
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
        if (rc == -5 && h->p2p.ready) {
            p2p_close_peers(h);
            if (h->p2p.words) (void)hipMemset(h->p2p.words, 0, 4 * sizeof(unsigned));
        }
        h->err = msg;
    }
    return rc;
}

// Test entry: the state the last outer iteration of the last solve left on the handle (include/sfmba.h).  Copies only.
int sfmba_get_iteration_state(sfmba_handle* h, double* scalars, double* ctrl, double* si, double* g, double* sg,
                              double* si2, double* g2, double* sg2, double* Dc, double* Minv, double* Vinv, double* e,
                              double* pcg_x, double* pcg_r, double* p, double* x_new) {
    CHK(enter(h));
    if (!h->have_problem || !h->solved) return fail(h, -1, "sfmba_get_iteration_state: no completed sfmba_solve on this handle");
    const Forms& f = h->forms;
    const bool local = f.pcg_local || f.pcg_local2;
    if (Minv && f.dense_solve) return fail(h, -1, "sfmba_get_iteration_state: Minv is not kept on the dense path (the inverses live in LDS)");
    if (e && !f.dense_solve && !f.use_rhsrec) return fail(h, -1, "sfmba_get_iteration_state: e is not kept (pass A has overwritten it with its z)");
    if (pcg_r && (f.dense_solve || local)) return fail(h, -1, "sfmba_get_iteration_state: pcg_r is not kept (%s)", f.dense_solve ? "the dense path holds r in LDS" : "the local form's r lags one update behind");
    if (pcg_x && h->pcg_a_owed) return fail(h, -1, "sfmba_get_iteration_state: pcg_x is not kept (k_backsub's prologue did the last update: the final x is dc of p)");
    const size_t C = (size_t)h->C, P = (size_t)h->P, n = (size_t)h->n, n6 = 6 * C;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    auto fetch = [&](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); };
    PcgCtrl hc{};
    HIPCHK(h, fetch(&hc, h->ctrl.as<PcgCtrl>() + (h->pcg_L & 1), sizeof hc));
    if (scalars) HIPCHK(h, fetch(scalars, h->scal(), sizeof(double) * kScalSlots));
    if (ctrl) {
        const double c8[8] = {hc.rz, hc.rz0, hc.tol2, hc.rz_prev, hc.alpha_prev, (double)hc.iters, (double)hc.max_iters, (double)hc.done};
        memcpy(ctrl, c8, sizeof c8);
    }
    const struct { double* dst; const double* src; } whole[] = {{si, h->si_cur}, {g, h->g_cur}, {sg, h->sg_cur}, {si2, h->si_new},
                                                                {g2, h->g_new}, {sg2, h->sg_new}, {p, h->p.as<double>()}, {x_new, h->x_new}};
    for (const auto& w : whole)
        if (w.dst) HIPCHK(h, fetch(w.dst, w.src, sizeof(double) * n));
    std::vector<double> buf;
    auto planes = [&](double* dst, const double* src, size_t rows) -> int {        // plane-major [rows][C] -> [C][rows]
        if (!dst) return 0;
        buf.resize(rows * C);
        HIPCHK(h, fetch(buf.data(), src, sizeof(double) * rows * C));
        for (size_t c = 0; c < C; ++c)
            for (size_t k = 0; k < rows; ++k) dst[rows * c + k] = buf[k * C + c];
        return 0;
    };
    auto records = [&](double* dst, const double* src, size_t stride, size_t width) -> int {    // [P][stride] -> [P][width]
        if (!dst) return 0;
        buf.resize(stride * P);
        HIPCHK(h, fetch(buf.data(), src, sizeof(double) * (stride * (P - 1) + width)));
        for (size_t q = 0; q < P; ++q)
            for (size_t k = 0; k < width; ++k) dst[width * q + k] = buf[stride * q + k];
        return 0;
    };
    CHK(planes(Dc, h->Dc.as<double>(), 6));
    CHK(planes(Minv, h->Minv.as<double>(), 21));
    if (P > 0) {
        CHK(records(Vinv, vinv_ptr(h), kVinvRow, 6));
        if (f.dense_solve) CHK(records(e, h->rec + 3, kRec, 3));
        else CHK(records(e, h->rhsrec.as<double>() + 3, kRhsRec, 3));
    }
    const double* set = h->vecs.as<double>() + (size_t)(hc.iters & 1) * kPcgVecs * n6;      // (k_transpose, k_backsub: x of the final set)
    CHK(planes(pcg_x, set + kPcgX * n6, 6));
    CHK(planes(pcg_r, set + kPcgR * n6, 6));
    return 0;
}

int sfmba_get_fun_grad(sfmba_handle* h, double* fun_out, double* grad_out) {
    CHK(enter(h));
    if (!h->have_problem || !h->solved) return fail(h, -1, "no completed sfmba_solve on this handle");
    if (fun_out) CHK(download_residuals(h, fun_out));
    if (grad_out) {
        CHK(ensure_h_x(h));
        HIPCHK(h, hipMemcpyAsync(h->h_x, h->g_cur, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
        CHK(wait_stream(h));
        memcpy(grad_out, h->h_x, sizeof(double) * h->n);
    }
    return 0;
}

// Host-only helper exported for the CPU test-suite (no GPU needed): the 2-D trust-region solve.
int sfmba_tr2d_solve(const double* B3, const double* g2, double Delta, double* p2) {
    return solve_trust_region_2d(B3, g2, Delta, p2) ? 1 : 0;
}
