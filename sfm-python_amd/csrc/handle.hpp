// handle.hpp -- the handle behind include/sfmba.h and what the library's sources share on the host (internal, host only).
// sfmba.hip defines every function declared here but one (launch_k_track_scan_sums: tracks.hip); consumers.hip, match.hip,
// tracks.hip and plan.hip hold their stages.
#pragma once
#include "../../include/sfmba.h"
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: librccl.so.1 is dlopen()ed by sfmba_comm_init
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "ba_device.hpp"
#include "problem_tables.hpp"

namespace sfmba {
extern const size_t kLdsDynMax;                // dynamic LDS a workgroup may ask for (sfmba.hip, where the tests read it)
extern const int kRecStride, kVinvStride;      // doubles per point record / inverse point block as k_schur_blocks reads them (sfmba.hip)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        release();
        if (n == 0) n = 8;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    // grow-only like ensure(), but the first `keep` bytes survive a reallocation (device-to-device copy) and the new
    // block has headroom, so that a problem that grows call by call does not reallocate every time
    hipError_t ensure_keep(size_t n, size_t keep) {
        if (n <= bytes && p) return hipSuccess;
        if (keep == 0 || !p) return ensure(n + n / 2);
        void* q = nullptr;
        const size_t cap = n + n / 2;
        hipError_t e = hipMalloc(&q, cap);
        if (e != hipSuccess) return e;
        e = hipMemcpy(q, p, std::min(keep, bytes), hipMemcpyDeviceToDevice);
        (void)hipFree(p);
        p = q; bytes = cap;
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// a piece of a larger device allocation (the structure tables of a problem share one buffer and one upload)
struct DevView {
    void* p = nullptr;
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// pinned host memory, grow-only, optionally keeping a prefix across a reallocation
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t n, size_t keep) {
        if (n <= bytes && p) return hipSuccess;
        void* q = nullptr;
        const size_t cap = n + n / 2 + 64;
        hipError_t e = hipHostMalloc(&q, cap, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if (p && keep) memcpy(q, p, std::min(keep, bytes));
        if (p) (void)hipHostFree(p);
        p = q; bytes = cap;
        return hipSuccess;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// test / diagnostic hooks, set through sfmba_debug_option only (nothing reads the environment)
#define SFMBA_DEBUG_OPTIONS(X) \
    X(pcg_fused, -1)      /* 0: two-kernel PCG although the fused launch would fit */ \
    X(tab_lds, -1)        /* 0: camera table read from L2 although LDS would fit */ \
    X(vec_lds, -1)        /* 0: camera vector read from L2 although LDS would fit */ \
    X(sweep_rc, -1)       /* 0: pass A reads the stored Jacobian although the recomputing form would fit; 2: its table in global memory whatever the size */ \
    X(dense, -1)          /* 0: PCG although the dense reduced-camera path would apply */ \
    X(precond, -1)        /* 0: block-Jacobi preconditioner from U + Dc instead of the Schur diagonal */ \
    X(pcg_local, -1)      /* 0: the fused PCG keeps its whole update in pass A's prologue */ \
    X(xcd_chunks, -1)     /* 1 / 0: camera lists cut at the eight point-range boundaries (one chunk per XCD) whatever the size */ \
    X(rhsrec, -1)         /* 1 / 0: the rhs + preconditioner pass gathers its own 128-byte records whatever the size */ \
    X(cost_rider, -1)     /* 0: the trial cost is summed and posted by a k_finish launch of its own */ \
    X(packed_upload, -1)  /* 0: the observation arrays are uploaded as int32 / fp64 although they would pack */ \
    X(jfree, -1)          /* 1: the J-free iteration (measurement): K1 does not write the Jacobian, k_jdot and k_backsub recompute its blocks from the LDS camera table */ \
    X(rc_consumers, -1)   /* 0: k_jdot and k_backsub read the stored Jacobian although their row form would apply; 1: the row form wherever it is legal, whatever the size */ \
    X(cm_device, -1)      /* 0: the camera-major order is sorted on the host and its permutation uploaded */ \
    X(pcg_inline, -1)     /* 0: sharded solves keep the collective of the product as a launch of its own */ \
    X(xcd_cam, -1)        /* 0: K3 and the rhs pass keep the one-chunk-per-camera table where pass B takes the XCD-aware one */ \
    X(pcg_skip_last, -1)  /* 0: the pass B behind the launch the record says is the last one is enqueued all the same; 2: only that pass B is left out */ \
    X(pcg_mixed_b, -1)    /* 0: pass B keeps fp64 point records although pass A runs on fp32 operands */ \
    X(pcg_mixed, -1)      /* 1 / 0: fp32 operands in the implicit Schur product whatever the storage mode */ \
    X(pcg_split, -1)      /* 1: the local form with its tail in a kernel of its own (k_pcg_tail) on a single rank too; 0: sharded / multi-chunk solves keep the round-2 forms (whole update in every workgroup of pass A, or k_pcg_update) */ \
    X(spec_scale, -1)     /* 0: k_update_scale is launched after the host has accepted the trial point */ \
    X(start_handoff, -1)  /* 0: a solve starts with a blocking read-back of the cost and the scale sums */ \
    X(early_download, -1) /* 0: the result is copied to the host behind the last launch of the solve */ \
    X(cov_lds, -1)        /* 0: the point sweep of sfmba_covariance reads Sigma_cc from L2 instead of staging it in LDS */ \
    X(cam_chunk, 0)       /* > 0: chunk length of the camera-major kernels */ \
    X(pcg_guess_bias, 0)  /* added to the number of speculatively enqueued PCG iterations */ \
    X(trace_pcg, 0) X(trace_stalls, 0) X(trace_timing, 0)   /* stderr diagnostics */ \
    X(wait_deadline_s, 120) /* a hand-off that does not arrive within this many seconds fails the solve (-3) */ \
    X(p2p_delay_ms, 0)    /* test: sleep this long before the first collective of a solve */ \
    X(p2p_timeout_ms, 0)  /* test: > 0 overrides both time-outs of the direct all-reduce */
struct Debug {
#define X(name, init) int name = init;
    SFMBA_DEBUG_OPTIONS(X)
#undef X
};

// Which form of every kernel runs.  Two functions below the handle fill it and nothing else writes it:
// decide_problem_forms (sfmba_set_problem) and decide_solve_forms (start of every compute call).
struct Forms {
    // ---- problem stage: frozen until the next sfmba_set_problem
    bool packed_upload = false;              // observation arrays cross PCIe as uint16 / int16 (k_unpack_obs)
    bool cm_device = false;                  // camera-major order sorted on the device
    int64_t cam_chunk_len = 4096;            // chunk length of the camera-major kernels
    bool lds_tab = true, lds_vec = true;     // camera table (K1, K2) / camera vector (sweeps) staged in LDS
    bool sweep_rc = false;                   // pass A recomputes the blocks from an LDS table (k_point_sweep_rc)
    bool sweep_rc_g = false;                 // ... from a table in global memory (more cameras than the LDS holds)
    bool round_blocks = false;               // pass A applies stored fp32 blocks: the camera-major passes round theirs the same way
    bool pcg_fused = false;                  // PCG update fused into the launch of pass A (v in LDS, C <= 1024)
    // mixed-precision Schur product (ba_kernels.hpp: MixedPrep): fp32 operands, fp64 arithmetic
    bool mixed = false;                      // pass A
    bool mixed_b = false;                    // ... and pass B (fp32 point records)
    bool jfree = false;                      // J-free iteration (needs the camera table in LDS)
    bool rc_cons = false;                    // k_jdot / k_backsub in row form (k_jdot_rc, k_backsub_rc): the stored Jacobian is not read
    bool dense = false;                      // reduced camera matrix formed and factorised (6 C <= kDenseMaxN) instead of PCG
    bool xcd_b = false;                      // pass B takes the XCD-aware chunk table (every camera's list cut at eight point ranges)
    bool use_rhsrec = false;                 // the rhs + preconditioner pass gathers its own 128-byte records (many points)
    bool cam_multi = false;                  // some camera has more than one chunk: k_cam_combine runs
    // ---- solve stage: from the above, the transport as it stands and the options read live
    bool one_rank = true;                    // no transport: nothing is exchanged
    bool dense_solve = false;                // dense, on one rank (sharded: the block pairs would need their own all-reduce)
    bool precond = true;                     // Schur-diagonal preconditioner (false: block-Jacobi of U + Dc)
    bool xcd_cam = false;                    // K3 and the rhs pass over the XCD-aware table too, one wave per chunk
    bool cam_inline = false;                 // per-camera sums of K3 / the rhs pass all-reduced by the workgroup that forms them
    bool own_inverse = false;                // the rhs pass inverts its camera's preconditioner block itself (RhsPrecond)
    // where the product is reduced: inside pass B, camera by camera (CamExchange) / behind it, with the per-camera tail of
    // the local form (k_p2p_pcg / k_pcg_tail); else by a collective and k_pcg_update or pass A's prologue
    bool pcg_inline = false, pcg_split = false;
    // per-camera bookkeeping in pass B or the tail: the fused form / the light update as a kernel of its own (> 1024 cameras)
    bool pcg_local = false, pcg_local2 = false;
    int skip_last = 0;                       // of the last speculative launch pair: 0 nothing is left out, 1 its pass B, 2 pass A too (FinalUpdate)
    // hand-offs: no blocking one at the start; k_update_scale of the trial point enqueued before the verdict; (one rank) the
    // trial cost and its post ride with K3; the result leaves on the copy stream as soon as the solve is decided
    bool quick_start = false, spec_scale = false, cost_rider = true, early_download = false;
};

}  // namespace sfmba
using namespace sfmba;

struct sfmba_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    int n_cu = 256;

    // problem
    bool have_problem = false;
    int64_t C = 0, P = 0, N = 0, ld = 0, n = 0;
    int64_t N_total = 0;
    KMat K{};
    bool permuted = false;
    int n_ranges = 0;
    bool f32 = false;                        // fp32 storage of uv, r, t1 and the Jacobian (arithmetic stays fp64)
    bool f32_next = false;                   // takes effect at the next sfmba_set_problem
    std::vector<int64_t> fixed_next;         // sfmba_set_fixed_cameras: cameras held still from the next sfmba_set_problem on
    int64_t n_fixed = 0;                     // ... of the current problem
    std::vector<char> fixed_cur;             // [C] camera held still in the current problem
    Forms forms;                            // which kernel forms run (decide_problem_forms / decide_solve_forms)
    DevBuf rctab;                            // [C][18], k_rc_table
    DevBuf rt32, rec32, rctab32, rtd;        // [C][12], [P][8], [C][20] floats; [C][12] doubles
    Origin origin{0.0, 0.0, 0.0};            // coordinates are rounded relative to it (set with every uploaded x)
    DevView cov_ptr, cov_pt, blk_ab;         // dense path: per block pair (a <= b) the points both cameras see
    DevBuf Sblk;
    DevBuf tables;                           // ranges | wsteps | steps | chunk table | chunk offsets | pair lists: ONE upload
    int n_blk = 0;
    Debug dbg;                               // test / diagnostic hooks (sfmba_debug_option)

    DevBuf cam_idx, pt_idx, pt_ptr, uv;
    DevView ranges, wsteps, steps;
    int n_steps = 0;
    // camera-major order of the same observations (structure only): per-camera sums without atomics
    DevBuf cm_perm, cm_pt, cm_uv, cam_partial;
    DevBuf sort_hist, fixed_dev;             // device-side camera-major sort: [kSortSlices][C] counts -> offsets; held cameras
    DevView cam_ptr_dev;                     // [C + 1]
    DevView cam_chunks, cam_chunk_ptr;
    int n_chunks = 0;
    // a second chunk table for pass B of the Schur product alone (many points): every camera's list cut at the eight
    // point-range boundaries, chunk 8 c + k on XCD k (see set_problem)
    DevView cam_chunks_b, cam_chunk_ptr_b;
    int n_chunks_b = 0;
    DevBuf xa, xb, tabA, tabB, r, J, t1;     // ONE Jacobian / residual buffer set
    DevBuf rhsrec;                           // [P][kRhsRec]: what k_cam_rhs_diag gathers (written by k_prep)
    DevBuf V, Vinv, gp, e, recA, recB;       // rec: point records X Y Z | z (k_fill_rec), one per parameter vector
    DevBuf edge;                             // pieces of the point rows cut by K1's tiles (PointBlocksOut)
    DevBuf g, si, sg, p;                     // n-vectors; p = [dc | dp]
    DevBuf g2, si2, sg2;                     // second set of g, si, sg: a speculative k_update_scale writes the trial
                                             // point's there (see g_cur below)
    DevBuf Dc, Minv, vecs, vtmp, vcm;               // camera-sized, plane-major [k][C]; vecs = 2 sets x (x r p s u)
    DevBuf part, ctrl;
    DevBuf arena_own;
    double* arena = nullptr;                 // [acc 6C | sd 21C | Ugc 27C | 32 scalars]; acc | sd are plane-major [27][C]
    int64_t arena_doubles = 0;
    sfmba_allreduce_fn ar_fn = nullptr;
    void* ar_ctx = nullptr;
    sfmba_print_fn print_fn = nullptr;       // verbose = 2 lines go here (null: stdout of the C library)
    void* print_ctx = nullptr;
    ncclComm_t comm = nullptr;               // native RCCL communicator (sfmba_comm_init)
    int64_t n_collectives = 0, n_launches = 0;
    // direct all-reduce over peer-mapped staging buffers (k_p2p_allreduce); preferred over RCCL / the
    // callback for every vector that fits a slot
    struct P2p {
        bool ready = false;
        int rank = 0, world = 0;
        int64_t stride = 0;                  // doubles per slot
        void* own = nullptr;                 // this rank's staging buffer (flags, then data)
        void* opened[kP2pMaxRanks] = {};     // peers' buffers as mapped here (null for own)
        double* data[kP2pMaxRanks] = {};
        unsigned long long* flags[kP2pMaxRanks] = {};
        double* camdata[kP2pMaxRanks] = {};  // [2][W][6 C]: the product's per-camera exchange inside pass B (CamExchange)
        unsigned* words = nullptr;           // [0] ticket, [1] error, [2..3] uint64 count of performed collectives
        int64_t calls = 0;
        bool first_in_solve = true;          // the next collective is the rendezvous of a solve (long timeout)
        // agreed over the link itself at attach (every rank holds the same two values):
        int shared_device = 1;               // ranks whose handle sits on the same physical GPU as this one's (rehearsals)
        bool any_multi = false;              // some rank's shard has a camera of several chunks / the XCD-aware chunk table
    } p2p;
    double* h_scal = nullptr;                // pinned
    // set_problem: converted arrays of the current problem in pinned memory (upload source, and what the next
    // call is compared with), host copies of the structure tables, worker threads
    struct Stage { PinnedBuf uv, ci, pi, perm, ptr, uvf, tables, ci16, uv16; } stage;
    DevBuf ci16_dev, uv16_dev;               // packed upload of the observation arrays (k_unpack_obs)
    struct Prev { bool valid = false; bool f32 = false; bool packed = false; int64_t N = 0, P = 0; } prev;
    ProblemTables tb;                        // what build_problem_tables() made of the arguments (problem_tables.hpp)
    HostPool pool;
    int64_t obs_reused = 0, obs_uploaded = 0;    // of the last sfmba_set_problem
    double* mbox = nullptr;                  // coherent pinned block the device posts the hand-off into (Mailbox)
    double* mbox_dev = nullptr;              // its device-visible address
    unsigned long long mbox_seq = 0;
    Mailbox post{};                          // set while the launch that ends a hand-off is enqueued; else empty
    double* h_x = nullptr;                   // pinned staging of the parameter vector
    size_t h_x_doubles = 0;
    // Large problems (>= 2M parameters): the result leaves the device while the solve still runs -- every trial point is
    // copied to a pinned mirror of its buffer on a second stream, behind the launch that wrote it and beside the
    // evaluation of that point, so that the accepted x of the LAST iteration is already on the host when the solve ends
    // (24 MB = 0.45 ms at 3M parameters).  Not below that size: there the runtime performs the copy as a blit KERNEL,
    // which shares the CUs with the residual + Jacobian kernel it overlaps (K1 30 -> 32 us at 306k parameters, 60 us
    // under rocprofv3).  (Also tried there: the result in four chunks whose staging copies overlap the later chunks'
    // DMA -- 145 us against 130-150 us for one copy + a four-thread staging copy: four blit launches, no gain.)
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_written = nullptr, ev_copied[2] = {nullptr, nullptr};
    bool result_in_flight = false;           // a solve's early result copy (copy stream -> h_x) has not been waited for
    PinnedBuf mirror[2];
    unsigned long long mirror_tag[2] = {0, 0}, copy_count = 0, x_tag = 0;
    bool mirror_on = false;
    const double* skip = nullptr;         // device flag gating speculative trial launches (sfmba_solve); else null
    double pcg_tol = 0.0; int pcg_cap = 0; // options of the running PCG (fused launch 0 writes the control block)
    bool pcg_b_owed = false;              // the pass B behind the last enqueued pass A was left out (pcg_enqueue)
    bool pcg_a_owed = false;              // ... and that pass A too: k_backsub does its update (FinalUpdate)
    DevBuf pcg_part;                      // [4][C] partial dot products of the local form
    int pcg_hint = 0;                     // largest PCG iteration count a solve on this handle has needed
    std::vector<int> pcg_hist;            // PCG iterations of outer iteration k in the previous solve on this handle: the
                                          // reference solves a slightly grown problem from a nearby start call after
                                          // call (sfm.py:59-71), and the counts repeat; with a record the speculative
                                          // batch is that count (+1 launch for the fused update), without the spare
    int64_t hist_C = 0, hist_P = 0, hist_N = 0;   // the problem pcg_hist was recorded on
    unsigned long long hist_sig = 0;         // ... and its content: problem generation + a checksum of the start vector
    unsigned long long problem_gen = 0;      // raised by every sfmba_set_problem whose arrays differ from the previous ones
    bool solved = false;
    bool transport_dropped = false;          // sfmba_set_problem tore down an active transport: the next compute call
                                             // fails until one is set up again (or single-rank use is acknowledged)
    std::vector<const void*> lds_ready;      // kernels already opted in to 160 KiB dynamic LDS
    int last_pcg_iters = 0;

    double *x = nullptr, *x_new = nullptr;   // current / trial parameter vectors (alias xa/xb)
    double *tab = nullptr, *tab_new = nullptr;
    double *rec = nullptr, *rec_new = nullptr;   // point records of x / x_new (swapped together with them)
    // gradient, column scale and D^2 g of the ACCEPTED point (alias g / si / sg or g2 / si2 / sg2) and the set a
    // speculative k_update_scale fills for the trial point; swapped where x / tab / rec are, on acceptance only
    double *g_cur = nullptr, *si_cur = nullptr, *sg_cur = nullptr;
    double *g_new = nullptr, *si_new = nullptr, *sg_new = nullptr;

    double* acc() const { return arena; }    // product of the implicit Schur complement / reduced rhs term (6C)
    double* sd() const { return arena + 6 * C; }       // diagonal blocks of W Vinv W^T (Schur-diagonal preconditioner)
    double* Ugc() const { return arena + 27 * C; }
    double* scal() const { return arena + 54 * C; }
    int pcg_L = 0;                           // launches (sweep+update pairs) since pcg_start
    int red_bc = 1, red_grid = 2;            // block split of k_update_scale's reduction (cameras | points)
    int scale_pts = 1;                       // points per thread of k_update_scale
    bool pending_scale_sums = false;         // k_update_scale ran, its final sums ride with the next k_jdot
    // sfmba_reprojection_stats: a parameter vector, camera table and result arrays of its own (grow-only), so that the
    // solver's buffers -- x, tab, rec, r, J, the normal blocks -- are as the last solve left them after a statistics call
    struct Stats {
        DevBuf x, tab;                       // the call's parameter vector and its camera table
        DevBuf ed, keep, keep_final;         // [ld] err | depth pairs; [ld] own test; [ld] own test and point kept
        DevBuf pt_views, pt_d, pt_keep;      // [P]; [4][P] max err, sum err^2, min depth, angle; [P]
        DevBuf cam_i, cam_d;                 // [2][C] views, behind; [2][C] sum err, max err
        DevBuf part, sum;                    // [point workgroups][kStatsPart]; [kStatsPart]
        DevBuf perm, cam_ptr, hist, cnt;     // camera-major permutation of ALL observations, built at the first call of a problem
        unsigned long long perm_gen = 0;     // ... for the problem of this generation and size (0: none)
        int64_t perm_N = -1, perm_C = -1;
        PinnedBuf host;                      // staging of the per-observation downloads
        // the masks of sfmba_triangulate / sfmba_resect (calls on a handle are serialised: one pair serves both)
        DevBuf use;                          // [ld] obs_use in stored order
        PinnedBuf mask_host;                 // staging of obs_use, of the select mask and of the OK counts
    } stats;
    // sfmba_triangulate: works on stats.x / stats.tab (the parameter vector and camera table of a call outside the
    // solver), stats.use and on result arrays of its own
    struct Tri {
        DevBuf select;                       // [P]
        DevBuf X, ints, dbl, ok_part;        // [P][3]; [3][P] status, views, iters; [2][P] rms err, angle; [workgroups]
    } tri;
    // sfmba_triangulate_ransac: works on stats.x / stats.tab and stats.use as sfmba_triangulate does, on
    // sfmba_triangulate's select mask and result arrays (k_triangulate runs last) and on buffers of its own
    struct TriRansac {
        DevBuf mask, ok;                     // [ld] inlier mask, stored order; [P] the best count reaches the need
        DevBuf X_hyp, ints, hyp;             // [P][3]; [4][P] status, views, inliers, best h; [P][H]
        PinnedBuf host;                      // staging of the integers and the mask
    } tri_ransac;
    // sfmba_resect: works on stats.x (the parameter vector of a call outside the solver), the camera-major permutation
    // of the statistics call, stats.use and on result arrays of its own
    struct Resect {
        DevBuf select;                       // [C]
        DevBuf cam, ints, rms;               // [C][6]; [4][C] status, views, iters, ok; [C]
    } resect;
    // sfmba_fundamental_ransac / sfmba_homography_ransac / sfmba_recover_pose: a batch of edges that has nothing to do
    // with the problem; every buffer is the three calls' own.  sfmba_similarity_ransac shares them: pairs [M_used][6]
    // sx sy sz dx dy dz, samples [n_sets][H][3], slots of 16 doubles, F [2][n_sets][13], ints [n_sets][5], mask [2][M_used]
    struct TwoView {
        DevBuf pairs, uptr, samples, E;      // [M_used][4] x1 y1 x2 y2; [n_edges + 1]; [n_edges][H][8 (F) or 4 (H)]; [n_edges][9]
        DevBuf slots, hyp;                   // [n_edges][slices][kTwoViewSlot]; [n_edges][H]
        DevBuf F, ints, mask;                // [2][n_edges][9] F, F_refit (H, H_refit); [n_edges][4 (F) or 5 (H)]; [M_used] ([2][M_used] for H)
        DevBuf Rt, err, pose_ints, X, ang;   // [n_edges][12]; [n_edges]; [n_edges][6]; [M_used][3]; [M_used]
        PinnedBuf in_host, out_host;         // staging of the packed batch; of the results
        std::vector<int64_t> pos;            // used pair -> stored pair, when the call has a pair_use mask
    } twoview;
    // sfmba_resect_ransac: works on stats.x, the camera-major permutation of the statistics call and stats.use as
    // sfmba_resect does, on sfmba_resect's result arrays (k_resect runs last) and on buffers of its own
    struct Pnp {
        DevBuf select, ok, mask;             // [C] the caller's select mask; [C] RANSAC succeeded; [ld] inlier mask, stored order
        DevBuf corr, cpos, cn;               // [N][5] packed X Y Z u v per camera; [N] their stored positions; [C] their number
        DevBuf samples, slots, hyp;          // [C][H][3]; [C][slices][kPnpSlot]; [C][H]
        DevBuf pose, ints;                   // [C][6] best hypothesis; [C][6] status, views, inliers, best h, best solution, success
        PinnedBuf host;                      // staging of the results
    } pnp;
    // sfmba_set_descriptors / sfmba_match_descriptors: the descriptor set in the form(s) the kernels read and the
    // buffers of a batch of edges; nothing of it is shared with the problem
    struct Match {
        DevBuf raw, flag;                    // the caller's (N, dim) array as given; the verdict of k_match_check
        DevBuf rows[2], norms[2];            // [form A, form B]: converted, padded rows; squared norms (fp32 / fp64)
        bool have[2] = {false, false};
        int row_bytes[2] = {0, 0}, n_chunk[2] = {1, 1};
        DevBuf edges, wgs, idx, dist, good;  // [n_edges] MatchEdge; [workgroups] int2; [Q][2]; [Q][2]; [Q]
        std::vector<int64_t> img_ptr;        // n_images + 1
        std::vector<unsigned char> good_host;
        int dim = 0, dtype = 0, form = 0;    // form: 0 no set, 1 A, 2 B (what the set qualifies for)
    } match;
    // sfmba_build_tracks / sfmba_get_tracks: the union-find forest, the component and track tables and the results of
    // the last build; nothing of it is shared with the problem or with the descriptor set
    struct Tracks {
        DevBuf img_ptr, pairs;               // [n_images + 1] int; [Mu] int2 global feature ids
        DevBuf parent, size, img, feat_track;        // [N] each (size: the component's number at a root after the first scan)
        DevBuf members, cursor, comp_off;    // [members] feature ids by component; [components]; [components + 1]
        DevBuf verdict, kept_len, track_id, track_off;       // [components] each
        DevBuf track_ptr, track_feat, track_image;   // the CSR: [components + 1]; [members]; [members]
        DevBuf sums, tot;                    // [scan workgroups][2]; [kTrackTotSlots]
        bool built = false;
        int64_t n_tracks = 0, T = 0;
        // what the plan stage reads of the last build besides the tables: its sizes and its img_ptr
        int64_t n_images = 0, N = 0;
        std::vector<int64_t> img_ptr_host;
    } tracks;
    // sfmba_plan_views / sfmba_assemble_problem / sfmba_get_assembled / sfmba_set_keypoints: they read the tables of
    // `tracks` and write buffers of their own (grow-only), so the tracks, the problem and a solve stay as they are
    struct Plan {
        DevBuf cam_mask, trk_mask;           // [n_images], [n_tracks]: the masks of the running call
        DevBuf trk_views, img_out;           // [n_tracks]; [3][n_images] tracks, known, gain
        DevBuf kept, pt_id, obs_off, pt_of;  // [n_tracks] used observations of a track of the sub-problem or 0; its number; its first observation; sub-point -> track
        DevBuf present, cam_id, cam_of;      // [n_images] in the sub-problem; its number; sub-camera -> image
        DevBuf ci, pi, of, p2d;              // [T] camera_indices, point_indices (64-bit), obs_feat; [T][2] gathered pixels
        DevBuf sums, tot;                    // [scan workgroups][2]; [kPlanTotSlots]
        DevBuf kp;                           // [N][2] the keypoint table of sfmba_set_keypoints
        std::vector<int64_t> kp_img_ptr;     // ... and its img_ptr
        bool have_kp = false;
        bool assembled = false;              // counts and the buffers hold a sub-problem of the current tracks
        int64_t counts[3] = {0, 0, 0};       // cameras, points, observations
    } plan;
    // sfmba_covariance: works on stats.x / stats.tab and the camera-major permutation of the statistics call (kind = 1 and
    // the U blocks) and on buffers of its own, so the solver's buffers stay as the last solve left them
    struct Cov {
        DevBuf rec, Vinv, Sblk, U;           // [P][kRecStride] X Y Z 0 0 0; [P][kVinvStride]; [n_blk][36]; [C][21]
        DevBuf pt_cost, pt_status, held;     // [P] sum r^2 of the point's run; [P]; [6 C]
        DevBuf scal, ints;                   // [kCovScal] doubles, [kCovInts] ints: the sums, sigma^2, pivots, failures
        DevBuf full, cam_cov, cam_sigma, cam_piv;    // [6C][6C]; [C][36]; [C][2]; [C][2] min relative pivot, failing parameter
        DevBuf pt_cov, pt_sigma;             // [P][9]; [P]
        PinnedBuf host;                      // staging of the mask and of the small read-backs
    } cov;
};

namespace sfmba {
int fail(sfmba_handle* h, int code, const char* fmt, ...);

#define HIPCHK(h, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(h, e_ == hipErrorOutOfMemory ? -4 : -3, "%s failed: %s (%s:%d)", #call,  \
                        hipGetErrorString(e_), __FILE__, __LINE__);                             \
    } while (0)

// after every kernel launch: count it (sfmba_get_counters) and pick up a launch failure
#define LAUNCHED(h)                            \
    do {                                       \
        ++(h)->n_launches;                     \
        HIPCHK(h, hipGetLastError());          \
    } while (0)

#define CHK(expr)                  \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != 0) return rc_;  \
    } while (0)

// every buffer of the list at (at least) its size; 0: a form that is not taken needs no buffer
struct SizedBuf { DevBuf* buf; size_t bytes; };
int ensure_all(sfmba_handle* h, std::initializer_list<SizedBuf> sized);
int enter(sfmba_handle* h);
int begin_compute(sfmba_handle* h, const void* x);
int wait_stream(sfmba_handle* h, hipEvent_t ev = nullptr);
int upload_x(sfmba_handle* h, const double* x_host, double* dst = nullptr);
int time_reps(sfmba_handle* h, int32_t reps, double* avg_us, const std::function<int()>& launch);
int launch_k_cam_table(sfmba_handle* h, const double* x, double* tab);        // the solver's kernels that the consumers launch too
int launch_k_cam_hist(sfmba_handle* h, const unsigned char* fixed, int B, int per_slice, int* hist);       // (with its LDS opt-in)
int launch_k_cam_offsets(sfmba_handle* h, const int* hist, const int* cam_ptr, int B, int* off);
int stats_time_kernel(sfmba_handle* h, const double* x, int32_t which, int32_t reps, double* avg_us);     // sfmba_time_kernel, 13 .. 17
int tri_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us);
int resect_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us);
int pnp_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us);
int cov_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us);                      // 18 (covariance.hip)
int tri_ransac_time_kernel(sfmba_handle* h, const double* x, int32_t reps, double* avg_us);               // 19 (consumers.hip)
// k_schur_blocks over the problem's pair lists at zero damping: blocks of W Vinv W^T -> Sblk [n_blk][36] (no rhs term)
int launch_k_schur_blocks(sfmba_handle* h, const double* tab, const double* rec, const double* Vinv, double* Sblk);
// the camera-major permutation of ALL observations (stats.perm / stats.cam_ptr), built once per problem (consumers.hip)
int stats_cam_perm(sfmba_handle* h);
// the middle launch of the scan of track_scan.hpp, compiled in tracks.hip, for the plan stage: `block` and `items` are the
// caller's kTrackBlock and kTrackScanItems, refused (-3) when they are not the ones the kernel was compiled with
int launch_k_track_scan_sums(sfmba_handle* h, long long* sums, unsigned nb, long long* tot, int slot, int block, int items);

// device -> host on the handle's stream; an array the caller did not ask for (null) is left out
inline hipError_t download(sfmba_handle* h, void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
}
inline bool multi_rank(const sfmba_handle* h) { return h->p2p.ready || h->comm != nullptr || h->ar_fn != nullptr; }
inline int grid_1d(int64_t n, int block, int cap) { return (int)std::min<int64_t>(std::max<int64_t>((n + block - 1) / block, 1), cap); }
// caller's position of the observation stored at k (h->tb.order: stored position -> caller's)
inline size_t caller_position(const sfmba_handle* h, size_t k) { return h->permuted ? (size_t)h->tb.order[k] : k; }

// Dynamic LDS above 64 KiB needs the per-kernel opt-in; it is set ONCE per kernel and handle (h->lds_ready): the call costs
// tens of microseconds to a millisecond.  set_lds: to the full 160 KiB, for the kernels with at most 2 KiB of static LDS
int opt_in_lds(sfmba_handle* h, const void* kernel, size_t bytes);
template <class Kern>
int set_lds(sfmba_handle* h, Kern k, size_t bytes) {
    return bytes <= 64 * 1024 ? 0 : opt_in_lds(h, reinterpret_cast<const void*>(k), kLdsDynMax);
}

// two events on the handle's stream round a run of launches: time_reps, and a stage's call with profile = 1
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    int start(sfmba_handle* h, bool on) {
        if (!on) return 0;
        HIPCHK(h, hipEventCreate(&a));
        HIPCHK(h, hipEventCreate(&b));
        HIPCHK(h, hipEventRecord(a, h->stream));
        return 0;
    }
    int stop(sfmba_handle* h) { if (a) HIPCHK(h, hipEventRecord(b, h->stream)); return 0; }
    int read(sfmba_handle* h, double* us) {                      // after the stream has been waited for
        if (!us || !a) return 0;                                 // (not asked for / profile = 0: the caller's zero stays)
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, a, b));
        *us = 1e3 * (double)ms;
        return 0;
    }
};

}  // namespace sfmba
