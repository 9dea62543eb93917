/*
 * sfmba.h -- C-ABI of libsfmba.so, the MI355X (gfx950) bundle-adjustment back end.
 *
 * Drop-in boundary: the one call the reference makes into its optimiser,
 *
 *     result = least_squares(compute_residuals, x0, jac_sparsity=..., verbose=..., x_scale='jac',
 *                            ftol=tol, method='trf',
 *                            args=(n_cam, n_points, camera_indices, pt_indices, pt2ds, K))
 *                                                     -- /root/reference/sfm_lite/sfm.py:266-268
 *
 * plus the model function it hands over, compute_residuals
 *                                                     -- /root/reference/sfm_lite/bundle_adjustment.py:35-42
 *
 * The reference is pure Python, so the "FFI" a maintainer adds is a ctypes binding of exactly these
 * entry points (shown in INTEGRATION.md; shipped as sfm-python_amd/sfmba/_capi.py).  Plain C types
 * only: caller-owned, C-contiguous HOST arrays are borrowed for the duration of a call and copied to
 * HBM inside it; nothing returned is library-owned except the handle and the error string.
 *
 * Return codes: 0 OK; -1 bad argument / shape / index out of range; -2 residuals not finite at x0
 * (scipy raises ValueError there, SCIPY/optimize/_lsq/least_squares.py:844-845); -3 HIP failure;
 * -4 out of memory; -5 collective failure (RCCL, the all-reduce callback, peer mapping, or a direct
 * all-reduce that gave up waiting for a peer).  The solver outcome is NOT an error:
 * it is sfmba_result.status, scipy's 0..4 (SCIPY/optimize/_lsq/least_squares.py:18-25).
 *
 * Threading: one handle is not thread-safe; distinct handles are independent; every entry point
 * selects the handle's device on entry, so it may be called from any thread (the reference's GUI runs
 * BA on a worker thread, /root/reference/app.py:80-85).
 */
#ifndef SFMBA_H
#define SFMBA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfmba_handle sfmba_handle;

/* Options of sfmba_solve.  Fill with sfmba_default_options() first.
 * ftol/xtol/gtol/max_nfev/verbose mirror the least_squares kwargs of sfm.py:266-268 (xtol, gtol,
 * max_nfev at scipy's defaults 1e-8, 1e-8, 100*n when the caller passes none). */
typedef struct sfmba_options {
    double  ftol;          /* scipy ftol; reference passes ba_tol (1e-10)                         */
    double  xtol;          /* 1e-8                                                               */
    double  gtol;          /* 1e-8                                                               */
    int64_t max_nfev;      /* <=0: 100 * n  (SCIPY trf.py:437-438)                               */
    int32_t verbose;       /* 0 silent, 1 summary (printed by the host shim), 2 iteration table  */
    int32_t max_iter;      /* <=0: unlimited; otherwise stop after this many outer iterations    */
    double  pcg_tol;       /* forcing term of the inexact step: the Schur PCG stops when the
                              preconditioned residual norm has dropped by this factor (default 1e-2;
                              a tenth of it when 6 n_cameras <= 128 and the iterations run inside one
                              workgroup; DESIGN.md section 3 compares this with scipy's LSMR)        */
    int32_t pcg_max_iter;  /* <=0: 2 * 6 * n_cameras                                             */
    int32_t pcg_check_every; /* host polls the device-side convergence flag every k iterations   */
    double  reg_min;       /* floor of the Levenberg-Marquardt term (1e-6), see DESIGN.md         */
    int32_t profile;       /* 1: bracket every residual+Jacobian launch with HIP events          */
    int32_t reserved;
    double  pcg_tol_max;   /* > pcg_tol: the forcing term adapts to the progress of the outer iteration,
                              eta_k = min(pcg_tol_max, max(pcg_tol, |g_h(x_k)| / |g_h(x_k-1)|)), eta_0 =
                              pcg_tol_max (default 0.1; Eisenstat-Walker: loose while the scaled gradient
                              still drops slowly, pcg_tol once it drops fast).  <= pcg_tol: fixed term.
                              Not applied to the in-workgroup iterations of the few-camera path.    */
} sfmba_options;

typedef struct sfmba_result {
    double  cost;          /* 0.5 |f|^2 at the returned x                                        */
    double  cost0;         /* 0.5 |f|^2 at x0                                                    */
    double  optimality;    /* |J^T f|_inf                                                        */
    double  rmse;          /* sqrt(2 cost / (2 N_total))                                         */
    double  rmse0;
    int64_t nfev;
    int64_t njev;
    int64_t iterations;    /* outer (trust-region) iterations                                    */
    int64_t pcg_iterations;/* total inner PCG iterations                                         */
    int32_t status;        /* 0 max_nfev/max_iter, 1 gtol, 2 ftol, 3 xtol, 4 ftol+xtol           */
    int32_t reserved;      /* number of PCG solves that stopped on a numerical breakdown         */
    double  seconds_total; /* wall time of the call, host clock, H2D/D2H included                */
    double  seconds_device;/* wall time between upload and download                              */
    double  resjac_avg_us; /* HIP-event average of the residual+Jacobian kernel (profile=1)      */
    int64_t resjac_launches;
    double  last_step_norm;
    double  last_reg;
} sfmba_result;

/* All-reduce hook for observation-sharded problems (one process per GPU).  `dev_ptr` points into the
 * exchange arena registered with sfmba_set_exchange; `count` doubles are reduced in place over all
 * ranks on the handle's stream; op 0 = sum, 1 = max.  Return 0 on success. */
typedef int (*sfmba_allreduce_fn)(void* ctx, void* dev_ptr, int64_t count, int32_t op);

/* Sink for the lines of the verbose = 2 iteration table (scipy prints it through Python's sys.stdout,
 * SCIPY/optimize/_lsq/common.py:545-563; the host shim registers a callback that does the same, so that
 * redirect_stdout / notebook capture see the table in order with the summary).  `line` has no trailing newline and
 * is valid during the call only.  fn = NULL: the C library's stdout. */
typedef void (*sfmba_print_fn)(void* ctx, const char* line);

/* ---- lifetime ---------------------------------------------------------------------------- */
int  sfmba_create(sfmba_handle** out, int device_id);
void sfmba_destroy(sfmba_handle* h);
const char* sfmba_last_error(const sfmba_handle* h);     /* valid until the next call on h */
void sfmba_default_options(sfmba_options* opt);
int  sfmba_set_print(sfmba_handle* h, sfmba_print_fn fn, void* ctx);
/* Run every kernel of `h` on this hipStream_t (default: a stream the handle owns). */
int  sfmba_set_stream(sfmba_handle* h, void* hip_stream);

/* Storage precision of the per-observation streams (uv, r, Jacobian): 64 (default) or 32.  Arithmetic
 * and every accumulation are fp64 in both modes; 32 halves the bytes of the sweeps (BASELINE.json
 * config 5).  Takes effect at the next sfmba_set_problem. */
int  sfmba_set_precision(sfmba_handle* h, int32_t storage_bits);

/* ---- problem (the args= tuple of sfm.py:268) ---------------------------------------------- */
/* camera_indices, point_indices: (N) int64; points_2d: (N,2) float64 (caller converts the
 * reference's int64 pixels, bundle_adjustment.py:41 promotes them the same way); K: 3x3 row-major.
 * Indices are range-checked here (the reference's fancy indexing would raise IndexError,
 * bundle_adjustment.py:40).  Any observation order is accepted; point-major (what
 * Graph.pt3ds_pt2ds produces, graph.py:186-191) is the fast path.
 * A new problem returns the handle to single-process operation: a registered exchange callback, RCCL
 * communicator or direct link is dropped and has to be set up again after this call.  The drop is not silent: when
 * a transport was active, every compute call on the handle fails with -1 until one is set up again
 * (sfmba_set_exchange / sfmba_comm_init / sfmba_p2p_attach) or single-rank use of the shard is acknowledged
 * (sfmba_set_exchange(h, NULL, 0, NULL, NULL, 0), sfmba_comm_destroy, sfmba_p2p_detach). */
int  sfmba_set_problem(sfmba_handle* h, int64_t n_cameras, int64_t n_points, int64_t n_obs,
                       const int64_t* camera_indices, const int64_t* point_indices,
                       const double* points_2d, const double* K);
/* Incremental re-use: the reference calls BA once per fused edge on a growing reconstruction
 * (/root/reference/sfm_lite/sfm.py:59-71); once all cameras are registered a new edge only appends points and
 * observations, so the arrays of one call start with those of the previous call.  Every sfmba_set_problem compares the
 * arrays with the previous problem of the handle (kept converted in pinned memory and in HBM), finds the first
 * observation that differs and uploads from there on only; structure tables are always rebuilt from the complete
 * arrays, so results are bitwise those of a fresh handle.  sfmba_problem_reuse reports what the last call re-used. */
int  sfmba_problem_reuse(const sfmba_handle* h, int64_t* obs_reused, int64_t* obs_uploaded);
/* Same with the pixels as the reference holds them, (N,2) int64 (graph.py:112-113): saves the caller a
 * converted copy. */
int  sfmba_set_problem_i64(sfmba_handle* h, int64_t n_cameras, int64_t n_points, int64_t n_obs,
                           const int64_t* camera_indices, const int64_t* point_indices,
                           const int64_t* points_2d, const double* K);

/* Cameras held still: the `fixed_camera_indices` of create_sparsity_matrix (bundle_adjustment.py:6,13-14), whose six
 * Jacobian columns the pattern leaves empty -- scipy's finite differences then never fill them, so the gradient, the
 * step and hence the parameters of those cameras stay as they are, and x_scale='jac' gives them scale 1
 * (SCIPY/optimize/_lsq/common.py:598-610).  The list is read at the NEXT sfmba_set_problem and stays in force until
 * it is replaced (n_fixed = 0 clears it); indices are range-checked there.  Their observations still count in the
 * residual, the cost and the point blocks. */
int  sfmba_set_fixed_cameras(sfmba_handle* h, const int64_t* camera_indices, int64_t n_fixed);

/* Observation sharding: this handle holds the local shard (its own points + their observations,
 * all cameras replicated); n_obs_total counts all shards.  `arena` is device memory of at least
 * sfmba_exchange_doubles(n_cameras) doubles that `fn` can all-reduce (e.g. a torch tensor).
 * Pass fn = NULL to return to single-process operation. */
int64_t sfmba_exchange_doubles(int64_t n_cameras);
int  sfmba_set_exchange(sfmba_handle* h, void* arena, int64_t arena_doubles,
                        sfmba_allreduce_fn fn, void* ctx, int64_t n_obs_total);

/* Native collective path: the library all-reduces its exchange arena itself with RCCL over xGMI
 * (librccl.so.1 is opened at run time; ncclAllReduce is enqueued on the handle's stream, so there is
 * no host synchronisation and no interpreter on the data path).  Rank 0 obtains the 128-byte id,
 * the host shim distributes it to all ranks (torch.distributed broadcast in sfmba.dist), every rank
 * calls sfmba_comm_init.  world == 1 is valid.  sfmba_comm_destroy returns to single-process mode. */
int  sfmba_comm_get_unique_id(void* id128_out);
int  sfmba_comm_init(sfmba_handle* h, const void* id128, int32_t rank, int32_t world,
                     int64_t n_obs_total);
int  sfmba_comm_destroy(sfmba_handle* h);

/* Direct all-reduce over peer-mapped device memory (xGMI inside a node), used in preference to RCCL or
 * the callback for every exchanged vector once attached: the solver reduces a dozen small vectors (a few
 * scalars to 27*n_cameras doubles) per iteration, which is latency, not bandwidth.  Collective set-up,
 * after sfmba_set_problem and sfmba_comm_init / sfmba_set_exchange on every rank:
 *   sfmba_p2p_export  allocates this rank's staging buffer and returns its 64-byte hipIpcMemHandle_t;
 *   (the caller all-gathers the handles over any channel, rank order)
 *   sfmba_p2p_attach  maps the peers' buffers and runs a 24-round self-test (the three message sizes of
 *                     the solver, chains of back-to-back collectives); returns -5 and detaches when
 *                     mapping or the self-test fails (the previous transport stays).  Its last collective settles
 *                     what the ranks must agree on for the per-camera sums to be exchanged INSIDE the kernels that
 *                     form them (pass B of the Schur product, the camera blocks, the reduced right-hand side): that
 *                     no rank's shard has a camera cut into several chunks, and how many ranks sit on one physical
 *                     GPU (a rehearsal: waiting workgroups of one rank must not fill the card the other needs).
 *                     Otherwise those sums keep collective launches of their own -- on every rank alike.
 * A wait gives up after 30 s (60 s for the first collective of a solve, the rendezvous) and fails the solve with -5;
 * the text of sfmba_last_error names the exchange and the camera whose peer value did not arrive.
 * All ranks must attach or none: agree on the minimum of the return codes and call sfmba_p2p_detach on
 * every rank if any failed.  world <= 16.  Results are summed in rank order: bitwise equal on all ranks. */
int  sfmba_p2p_export(sfmba_handle* h, int32_t world, void* handle64_out);
int  sfmba_p2p_attach(sfmba_handle* h, const void* handles_world_x_64, int32_t rank, int32_t world);
int  sfmba_p2p_detach(sfmba_handle* h);
int64_t sfmba_p2p_calls(const sfmba_handle* h);      /* collectives served by the direct path so far */
/* Running totals since sfmba_create: kernel launches enqueued by the library and collectives performed (any
 * transport).  Differences around a solve give launches / collectives per outer iteration (bench.py). */
int  sfmba_get_counters(const sfmba_handle* h, int64_t* kernel_launches, int64_t* collectives);
/* Which kernel form the current problem runs (the problem stage of the forms table): value = 0 / 1 for name =
 * "lds_tab", "lds_vec", "sweep_rc", "sweep_rc_g", "pcg_fused", "mixed", "mixed_b" (pass B reads the fp32 point records
 * too), "jfree", "rc_cons", "dense", "cam_multi" (some
 * camera has several chunks: k_cam_combine runs), "xcd_b" (pass B over the XCD-aware table), "rhsrec" (the rhs pass
 * gathers the 128-byte records), "round_blocks"; and of the solve stage, as the next compute call decides it from the
 * transport and the options of that moment: "xcd_cam" (K3 and the rhs pass one wave per chunk), "own_inverse" (the rhs
 * pass inverts its camera's preconditioner block itself), "one_rank", "precond" (Schur-diagonal preconditioner),
 * "dense_solve", "pcg_local" / "pcg_local2" (per-camera bookkeeping of the PCG in pass B or its tail: fused form /
 * k_pcg_update_local), "pcg_split" (k_pcg_tail), "skip_last" (0, 1, 2: what of the last speculative launch pair is left
 * out), "quick_start", "spec_scale", "cost_rider".  "match_form" belongs to the descriptor set, not to the
 * problem (sfmba_set_descriptors): 1 = form A, 2 = form B. */
int  sfmba_get_form(sfmba_handle* h, const char* name, int32_t* value);
/* PCG iterations of every outer iteration of the last completed sfmba_solve on this handle (the record the next
 * solve's speculative launches are sized from); returns the number of outer iterations, writes min(that, cap)
 * entries.  What the full-size parity tests compare with the recorded oracle runs (tests/golden/oracle_cfg*.json). */
int32_t sfmba_get_pcg_history(const sfmba_handle* h, int32_t* out, int32_t cap);

/* ---- compute_residuals (bundle_adjustment.py:35-42) ----------------------------------------- */
/* x: (6C+3P) float64 -> r_out: (2N) float64, interleaved x,y in the caller's observation order. */
int  sfmba_residuals(sfmba_handle* h, const double* x, double* r_out);

/* Residual and analytic Jacobian blocks (replaces scipy's sparse 2-point finite differences,
 * SCIPY/optimize/_numdiff.py:628-705).  Jc: (N,2,6) d r/d(rotvec,T); Jp: (N,2,3) d r/d X. */
int  sfmba_residual_jacobian(sfmba_handle* h, const double* x, double* r_out, double* Jc_out,
                             double* Jp_out);

/* ---- reprojection statistics and track filtering ----------------------------------------------- */
/* What the reference evaluates around its BA call in Python loops or not at all: the mean reprojection error it prints
 * after every fused edge (one calc_reproj_error call per observation, sfm.py:234-241), the depth test behind a camera
 * (sfm.py:221-223), the angle between the rays to a point (sfm.py:146-157) -- and the masks that turn thresholds on
 * them into a smaller problem (the reference never drops an observation).  One sweep per observation, one reduction
 * per point, one per camera, at the parameter vector x (6C+3P) of the current problem.
 *
 * Per observation (N, the caller's observation order):
 *   obs_err    sqrt(rx^2 + ry^2) in pixels, (rx, ry) the residual of sfmba_residuals at the same x, bit for bit
 *   obs_depth  z of R(w_c) (X_p - T_c), the camera-frame coordinate the projection divides by
 *   obs_keep   1 iff the observation passes its own test (err <= max_error_px, err finite, depth > min_depth) AND its
 *              point is kept: the final mask.  "Kept observations" of a POINT below are those that pass their own test.
 * Per point (P), over its observations in stored (point-major, else caller's) order:
 *   pt_views          kept observations
 *   pt_max_err        largest err among them (0 if none)
 *   pt_sum_err2       sum of err^2 over them
 *   pt_min_depth      smallest depth over ALL its observations, kept or not (+inf if it has none)
 *   pt_max_angle_deg  widest angle between the rays X_p - T_a, X_p - T_b over all pairs of kept observations, as
 *                     atan2(|a x b|, a . b) in degrees; 0 with fewer than two
 *   pt_keep           1 iff pt_views >= min_views and pt_max_angle_deg >= min_angle_deg
 * Per camera (C), over its finally kept observations (obs_keep = 1), cameras held still included:
 *   cam_views, cam_sum_err, cam_max_err;  cam_behind counts ALL its observations with depth <= 0
 * summary: observations in the problem, finally kept, points kept, observations with depth <= 0; sum of err, sum of
 *   err^2 and largest err over the finally kept observations.
 * With the default options (max_error_px = +inf, min_depth = -inf, min_angle_deg = 0, min_views = 0) everything with a
 * finite err is kept: a pure statistics pass.
 *
 * Any output pointer may be NULL; an array that is not asked for is not downloaded, and the per-camera pass and its
 * camera-major order (built at the first call of a problem that asks, at most 40448 cameras) run only when a per-camera
 * array is asked for.  opt = NULL: the defaults.  Returns -1 when no problem is set, x is NULL, a threshold is NaN, or
 * the handle waits for its transport (see sfmba_set_problem).  A non-finite x is no error: the observations it reaches
 * report a non-finite err and are never kept.  The call works on buffers of its own: fun and grad of the last solve and
 * the record the next solve starts from are as they were.  Same input, same bits: no atomics; sums run in a fixed order.
 * On a sharded handle the call describes the LOCAL shard only: its observations and points; per-camera figures and the
 * summary count this shard's observations (the caller adds or maximises over the ranks). */
typedef struct sfmba_filter_options {
    double  max_error_px;  /* an observation is kept when err <= this ...                          */
    double  min_depth;     /* ... and depth > this                                                 */
    double  min_angle_deg; /* a point is kept when its widest ray angle is >= this ...             */
    int32_t min_views;     /* ... and it has at least this many kept observations                  */
    int32_t reserved;
} sfmba_filter_options;
typedef struct sfmba_stats_summary {
    int64_t n_obs, n_obs_kept, n_points_kept, n_behind;
    double  sum_err, sum_err2, max_err;
} sfmba_stats_summary;
void sfmba_default_filter_options(sfmba_filter_options* opt);
int  sfmba_reprojection_stats(sfmba_handle* h, const double* x, const sfmba_filter_options* opt,
                              double* obs_err, double* obs_depth, uint8_t* obs_keep,
                              int32_t* pt_views, double* pt_max_err, double* pt_sum_err2, double* pt_min_depth,
                              double* pt_max_angle_deg, uint8_t* pt_keep,
                              int32_t* cam_views, double* cam_sum_err, double* cam_max_err, int32_t* cam_behind,
                              sfmba_stats_summary* summary);

/* ---- triangulation: N-view DLT plus point refinement ------------------------------------------- */
/* What creates the points bundle adjustment is given.  The reference calls cv2.triangulatePoints (sfm.py:140, 218), a
 * two-view DLT over the first two views of a track, once; this call triangulates every selected point of the current
 * problem from ALL its used observations, with the cameras of x[:6C], in one kernel (k_triangulate).  The points of x
 * are read only to fill X_out where no new point is returned.
 *
 * Per selected point, over its used observations in stored (point-major) order:
 *   linear stage  cv2.triangulatePoints extended to n views: rows u M3 - M1 and v M3 - M2 with M = K R [I | -T] in
 *                 pixel units, A^T A accumulated as ten doubles, its smallest eigenvector v by cyclic Jacobi rotations,
 *                 X = v[:3] / v[3].  The unknowns are neither translated nor rescaled (the homogeneous minimiser is
 *                 not invariant to that): for two views the result is the reference's.
 *   refinement    (max_iter > 0) Gauss-Newton on 1/2 sum |r|^2 over the three coordinates, r the residual of
 *                 sfmba_residuals and its 2x3 block.  The damping (H + lambda diag H) starts at zero; a trial point that
 *                 raises the cost is rejected and the damping raised (1e-3, then x10; x0.1 after an accepted step), so
 *                 the refined point never has a higher cost than the linear one.  It stops when an accepted step has
 *                 |d| <= xtol (|X| + xtol), when the step on offer is that small already (it is not taken: at rounding
 *                 level a trial point no longer lowers the cost), when a trial is rejected whose predicted reduction
 *                 was below 1e-12 of the cost (the rounding of the cost's own evaluation decides such trials), or after
 *                 max_iter trial points.  The run is walked once for the linear
 *                 stage, once at the linear point and once per trial point (pt_iters counts the trial points).
 *   verdict       at the result, first match wins (pt_status):
 *                   1 FEW_VIEWS    fewer used observations than max(2, min_views)
 *                   2 AT_INFINITY  |v[3]| <= 1e-12 |v|, or anything non-finite
 *                   3 BEHIND       a used observation has depth <= min_depth
 *                   4 LOW_ANGLE    the widest ray angle over the used observations (as pt_max_angle_deg of
 *                                  sfmba_reprojection_stats) is below min_angle_deg
 *                   5 HIGH_ERROR   a used observation has err above max_error_px
 *                   0 OK           otherwise;            -1: the point was not selected
 * X_out (P,3): the new point for status 0, the point of x for every other status.  pt_views: used observations, for
 * every selected point (else 0).  pt_iters, pt_rms_err = sqrt(sum err^2 / pt_views) in pixels and pt_angle_deg are
 * those of the result for every point that got past AT_INFINITY; else 0, NaN, NaN.  n_ok: points with status 0.
 *
 * pt_select (P) and obs_use (N, the caller's observation order): nonzero = take part; NULL = all.  Any output pointer may
 * be NULL; an array that is not asked for is not downloaded.  opt = NULL: the defaults.  Returns -1 when no problem is
 * set, x is NULL, an option is NaN, or the handle waits for its transport.  As sfmba_reprojection_stats: on a sharded
 * handle the call describes the LOCAL shard only; pixels are read as stored (fp64 or fp32); every buffer is the call's
 * own (shared with the statistics call), so fun, grad, the PCG record and a following solve are exactly what a fresh
 * handle gives; no atomics, sums in a fixed order: same input, same bits. */
typedef struct sfmba_triangulate_options {
    int32_t max_iter;      /* refinement iterations after the linear solution; 0 = linear only (default 10) */
    int32_t min_views;     /* used observations a point needs; values < 2 count as 2 (default 2)            */
    double  xtol;          /* refinement stops when an accepted step has |d| <= xtol (|X| + xtol) (1e-10)    */
    double  min_angle_deg; /* widest ray angle over the used observations at the result (default 1.0)        */
    double  min_depth;     /* every used observation must have depth > this at the result (default 0.0)      */
    double  max_error_px;  /* ... and err <= this (default +inf)                                             */
} sfmba_triangulate_options;
void sfmba_default_triangulate_options(sfmba_triangulate_options* opt);
int  sfmba_triangulate(sfmba_handle* h, const double* x, const uint8_t* pt_select /* P or NULL = all */,
                       const uint8_t* obs_use /* N, caller's order, or NULL = all */,
                       const sfmba_triangulate_options* opt,
                       double* X_out /* (P,3) */, int32_t* pt_status /* P */, int32_t* pt_views /* P */,
                       int32_t* pt_iters /* P */, double* pt_rms_err /* P */, double* pt_angle_deg /* P */,
                       int64_t* n_ok);

/* ---- resection: n-point DLT plus pose refinement ------------------------------------------------ */
/* What registers a camera: its pose from its observations of known points.  The reference calls cv2.solvePnP per new
 * camera (sfm.py:207-208; its teaching restatement is cv2_lite/solve_pnp.py); this call resects every selected camera
 * of the current problem from ALL its used observations and the points of x[6C:], in one kernel (k_resect), one
 * workgroup per camera.  The cameras of x are read only for start = 1 and to fill cam_out where no new pose is returned.
 *
 * Per selected camera, over its used observations in camera-major stored order:
 *   linear stage  (start = 0) _solve_pnp_linear (solve_pnp.py:18-43): pixels normalised by K^-1, rows [P, 0, -u P] and
 *                 [0, P, -v P] with P = (X, Y, Z, 1), nothing translated or rescaled; A^T A from forty sums, its smallest
 *                 eigenvector h by cyclic Jacobi rotations on the 12x12 matrix (pairs (0,1), (0,2), .., (10,11), until
 *                 the off-diagonal part is 1e-40 of the diagonal, at most 30 sweeps); h = [M | m], R = M (M^T M)^(-1/2)
 *                 (the reference's U V^T), R and m negated when det M < 0.  Unlike the reference, which takes t = m of the
 *                 unit-norm h, t = m / s with s the mean singular value of M: the reference's unscaled t is only a poor
 *                 start.  T = -R^T t, omega from R through a quaternion.
 *   refinement    (max_iter > 0) Gauss-Newton on 1/2 sum |r|^2 over the six parameters (omega, T), r the residual of
 *                 sfmba_residuals and its 2x6 block.  Damping (H + lambda diag H, from zero; 1e-3, then x10 after a
 *                 rejected trial, x0.1 after an accepted one), the rejection of a trial pose that raises the cost (a
 *                 non-finite cost counts as raised) and the stops are those of sfmba_triangulate, with |p| the norm of
 *                 the six parameters: the result never costs more than the start pose.  cam_iters counts trial poses.
 *   verdict       at the result, first match wins (cam_status):
 *                   1 FEW_VIEWS   fewer used observations than max(min_views, 6) (start = 0) / max(min_views, 3) (start = 1)
 *                   2 DEGENERATE  anything non-finite, or (start = 0) the second-smallest eigenvalue of A^T A is at most
 *                                 1e-12 of the largest (coplanar points: the null space has more than one dimension)
 *                   3 BEHIND      a used observation has depth <= min_depth
 *                   4 HIGH_ERROR  sqrt(sum |r|^2 / views) over the used observations is above max_rms_px
 *                   0 OK          otherwise;            -1: the camera was not selected
 * cam_out (C,6): the new pose for status 0, the camera of x for every other status.  cam_views: used observations, for
 * every selected camera (else 0).  cam_iters and cam_rms_err are those of the result for every camera that got past
 * DEGENERATE; else 0, NaN.  n_ok: cameras with status 0.
 *
 * cam_select (C) and obs_use (N, the caller's observation order): nonzero = take part; NULL = all.  Any output pointer may
 * be NULL; an array that is not asked for is not downloaded.  opt = NULL: the defaults.  Returns -1 when no problem is
 * set, x is NULL, an option is NaN, the handle waits for its transport, or the handle holds a shard (a camera's
 * observations are spread over the ranks).  Pixels are read as stored (fp64 or fp32); every buffer is the call's own or
 * the statistics call's, so fun, grad, the PCG record and a following solve are exactly what a fresh handle gives; no
 * atomics, sums in a fixed order: same input, same bits. */
typedef struct sfmba_resect_options {
    int32_t max_iter;    /* refinement trials after the start pose; 0 = start pose only (default 20) */
    int32_t min_views;   /* used observations a camera needs; below 6 counts as 6 when start = 0, below 3 as 3 when start = 1 (default 6) */
    int32_t start;       /* 0 = linear stage (DLT), 1 = the camera's pose in x (pose-only refinement) */
    double  xtol;        /* stop when a step has |d| <= xtol (|p| + xtol), p the six parameters (1e-10) */
    double  min_depth;   /* every used observation must have depth > this at the result (0.0) */
    double  max_rms_px;  /* rms reprojection error over the used observations at the result (default +inf) */
} sfmba_resect_options;
void sfmba_default_resect_options(sfmba_resect_options* opt);
int  sfmba_resect(sfmba_handle* h, const double* x, const uint8_t* cam_select /* C or NULL = all */,
                  const uint8_t* obs_use /* N, caller's order, or NULL = all */, const sfmba_resect_options* opt,
                  double* cam_out /* (C,6): omega, centre T, the BA model's parameters */, int32_t* cam_status,
                  int32_t* cam_views, int32_t* cam_iters, double* cam_rms_err, int64_t* n_ok);

/* ---- robust resection: P3P inside RANSAC, then pose refinement over the inliers --------------------------------------- */
/* sfmba_resect takes every used observation of a camera, so one wrong 2-D--3-D correspondence moves its DLT pose
 * arbitrarily far.  This call is cv2.solvePnPRansac for every selected camera of the current problem at once: H = max_iters
 * hypotheses per camera from three observations each (a minimal P3P solver), scored over all used observations, then
 * sfmba_resect's refinement (start = 1) over the inliers of the best one.  No local optimisation inside the loop, no
 * adaptive exit, and the mask is not recomputed after the refinement.
 *
 * A camera's "used observations" are numbered 0 .. n-1 in camera-major stored order (as in sfmba_resect); a masked call
 * gives bit for bit what the problem without those observations gives.
 *   samples     given: (C, H, 3) int32 positions among a camera's used observations; a position outside 0 .. n-1 (of a
 *               selected camera with enough views) makes the call return -1, a sample with a repeated position is invalid:
 *               its count is -1.  NULL: drawn by the counter-based rule of sfmba_fundamental_ransac with three draws,
 *                 key = mix(seed ^ mix(c << 32 | h)), c the camera's index in the problem (not its rank among the selected)
 *                 draw j = 0, 1, 2: k = mix(key + (j + 1) 0x9e3779b97f4a7c15) mod (n - j); then, for every earlier choice
 *                 in ascending order, if (k >= choice) ++k
 *   hypothesis  Grunert's P3P.  Unit rays j_i = K^-1 (u_i, v_i, 1) normalised; ca = j2.j3, cb = j1.j3, cg = j1.j2;
 *               a2 = |P2 - P3|^2, b2 = |P1 - P3|^2, c2 = |P1 - P2|^2, p = (a2 - c2) / b2, q = (a2 + c2) / b2.  The quartic
 *               in v = s3 / s1 (s_i the depth along ray i):
 *                 A4 = (p - 1)^2 - 4 (c2 / b2) ca^2
 *                 A3 = 4 [p (1 - p) cb - (1 - q) ca cg + 2 (c2 / b2) ca^2 cb]
 *                 A2 = 2 [p^2 - 1 + 2 p^2 cb^2 + 2 ((b2 - c2) / b2) ca^2 - 4 q ca cb cg + 2 ((b2 - a2) / b2) cg^2]
 *                 A1 = 4 [-p (1 + p) cb + 2 (a2 / b2) cg^2 cb - (1 - q) ca cg]
 *                 A0 = (1 + p)^2 - 4 (a2 / b2) cg^2
 *               Real roots in closed form: divided by A4 and depressed (v = y - b / 4), the largest real root z of the
 *               resolvent cubic z^3 + 2 p' z^2 + (p'^2 - 4 r') z - q'^2 (Cardano for one real root, the trigonometric form
 *               for three), the quadratics y^2 + s y + (p' + z - q' / s) / 2 and y^2 - s y + (p' + z + q' / s) / 2 with
 *               s = sqrt z, then two Newton steps on the quartic; the roots in ascending order of v.
 *               u = [(p - 1) v^2 - 2 p cb v + 1 + p] / (2 (cg - v ca)); a root counts when v > 0, u > 0 and everything is
 *               finite.  s1 = sqrt(b2 / (1 + v^2 - 2 v cb)), s2 = u s1, s3 = v s1, Q_i = s_i j_i.  The pose aligns the two
 *               triangles: frames e1 = (A2 - A1) / |.|, e3 = e1 x (A3 - A1) normalised, e2 = e3 x e1 for A = Q and A = P,
 *               R = E_Q E_P^T, T = P1 - R^T Q1 -- the bundle-adjustment model x_cam = R (X - T).  At most four solutions,
 *               numbered in ascending v; a repeated 3-D point, or a triple with |e1 x (P3 - P1)| <= 1e-9 |P3 - P1| (collinear),
 *               has none.
 *   score       of a solution: the used observations with |pi(K R (X - T)) - uv|^2 STRICTLY below threshold^2 and depth
 *               > min_depth; a non-finite value is no inlier.  Of a hypothesis: the largest over its solutions, the lowest
 *               solution among equals; 0 when it has no solution, -1 for an invalid sample.
 *   best        the largest count, the lowest h among equals.  The mask is that of the best solution, evaluated once more,
 *               and cam_inliers is counted FROM that mask: mask, count and the refinement's input agree by construction.
 *   refinement  sfmba_resect's (k_resect, start = 1) from the best pose over the inliers, for every camera whose best
 *               hypothesis has a finite solution and at least max(min_views, 4) inliers; max_iter, xtol, max_rms_px as
 *               there.  refine = 0: no trial pose (k_resect gives the verdict and the rms error at the best pose itself).
 *   verdict     first match wins (cam_status):
 *                  -1 the camera was not selected
 *                   1 FEW_VIEWS   fewer used observations than max(min_views, 4)
 *                   2 DEGENERATE  no hypothesis with a finite solution and at least max(min_views, 4) inliers
 *                   3 BEHIND / 4 HIGH_ERROR  k_resect's verdict over the inliers (also 2 for anything non-finite there)
 *                   0 OK          otherwise
 * cam_out (C,6): the refined pose (refine = 0: the best hypothesis' pose) for status 0, the camera of x otherwise.
 * cam_hyp (C,6): the best hypothesis' pose (rotation vector, centre), unrefined, wherever it has a finite solution --
 * DEGENERATE for want of inliers still reports it, with the count, h, solution and mask --, else the camera of x.
 * inlier_mask (N, the caller's order): 0 for observations that took no part.  cam_views: used observations of a selected
 * camera (else 0).  cam_best: h of the best hypothesis, -1 when no sample was valid (or there was no hypothesis);
 * cam_best_sol: its solution, -1 when it has none.  cam_success: inliers / n >= confidence.  cam_iters, cam_rms_err:
 * k_resect's, over the inliers, for every camera that reached it; else 0, NaN.  hyp_inliers (C,H): the count of every
 * hypothesis (-1: invalid sample, not selected or FEW_VIEWS).  n_ok: cameras with status 0.  kernel_us: with profile = 1
 * the HIP-event time of the call's launches, else 0.
 *
 * cam_select, obs_use, NULL outputs, opt = NULL and the return value -1 as for sfmba_resect, and also -1 for max_iters < 1.
 * Pixels are read as stored (fp64 or fp32).  Every buffer is the call's own, sfmba_resect's or the statistics call's, so
 * fun, grad, the PCG record and a following solve are exactly what a fresh handle gives; no atomics, sums in a fixed order:
 * same input, same bits. */
typedef struct sfmba_pnp_ransac_options {
    double   threshold;   /* pixels (default 8.0, cv2.solvePnPRansac's) */
    double   confidence;  /* cam_success = inliers / n >= confidence (0.99); there is no adaptive exit */
    double   min_depth;   /* an inlier has depth above this (0.0) */
    uint64_t seed;        /* of the drawn samples (0) */
    int32_t  max_iters;   /* hypotheses per camera, H, at least 1 (256) */
    int32_t  min_views;   /* used observations a camera needs, and inliers its best hypothesis needs; below 4 counts as 4 (6) */
    int32_t  refine;      /* 1 = Gauss-Newton over the inliers from the best hypothesis' pose (1) */
    int32_t  profile;     /* 1 = kernel_us is measured (0) */
    int32_t  max_iter;    /* the refinement's trial poses, as sfmba_resect's max_iter (default 20) */
    int32_t  reserved;
    double   xtol;        /* as sfmba_resect's xtol (default 1e-10) */
    double   max_rms_px;  /* as sfmba_resect's max_rms_px, over the inliers (default +inf) */
} sfmba_pnp_ransac_options;
void sfmba_default_pnp_ransac_options(sfmba_pnp_ransac_options* opt);
int  sfmba_resect_ransac(sfmba_handle* h, const double* x, const uint8_t* cam_select /* C or NULL = all */,
                         const uint8_t* obs_use /* N, caller's order, or NULL = all */,
                         const int32_t* samples /* (C,H,3) or NULL = drawn */, const sfmba_pnp_ransac_options* opt,
                         double* cam_out /* (C,6) */, double* cam_hyp /* (C,6) best hypothesis, unrefined */,
                         uint8_t* inlier_mask /* N, caller's order */, int32_t* cam_status, int32_t* cam_views,
                         int32_t* cam_inliers, int32_t* cam_best /* h */, int32_t* cam_best_sol, uint8_t* cam_success,
                         int32_t* cam_iters, double* cam_rms_err /* over the inliers */, int32_t* hyp_inliers /* (C,H) */,
                         int64_t* n_ok, double* kernel_us);

/* ---- robust triangulation: view-pair RANSAC over each track, then sfmba_triangulate over the inliers ---------------- */
/* sfmba_triangulate takes every used observation of a point, so one wrong match in a track -- tracks are the transitive
 * closure of the matches -- bends its DLT point or fails its verdict, and all the good observations of the track are lost
 * with it.  This call triangulates every selected point of the current problem from PAIRS of its used observations, scores
 * each pair's point over all of them, and hands the inliers of the best to sfmba_triangulate's kernel: the caller gets a
 * per-observation mask, drops one observation and keeps the point.  No local optimisation inside the loop, no adaptive
 * exit, no caller-supplied pairs, and the mask is not recomputed after the refinement.
 *
 * A point's "used observations" are numbered 0 .. n-1 in stored (point-major) order among the used; the hypotheses, their
 * counts, the best, the mask and X_hyp of a masked call are bit for bit what the problem without those observations gives.
 * (So are the outputs of the refinement -- X_out, pt_iters, pt_rms_err, pt_angle_deg -- for every point with fewer than 32
 * STORED observations: k_triangulate adds such a run in stored order, a longer one lane by lane of a wave from its stored
 * positions, which a mask shifts; there the two agree as two refinements that stop on xtol do.)
 *   hypotheses  M = n (n - 1) / 2, H = max_pairs.  M <= H: every pair (i < j) in lexicographic order -- (0,1), (0,2), ..,
 *               (0,n-1), (1,2), .., (n-2,n-1) --, h = 0 .. M-1; a hypothesis h >= M does not exist (hyp_inliers: -1).
 *               M > H: H hypotheses, hypothesis h the pair (first draw, second draw) of the counter-based rule of
 *               sfmba_fundamental_ransac with two draws:
 *                 key = mix(seed ^ mix(p << 32 | h)), p the point's index in the problem (not its rank among the selected)
 *                 draw j = 0, 1: k = mix(key + (j + 1) 0x9e3779b97f4a7c15) mod (n - j); second draw: if (k >= first) ++k
 *               Two hypotheses may name the same pair.
 *   point       of a pair (a, b), in this order: the two-view case of sfmba_triangulate's linear stage -- rows u M3 - M1,
 *               v M3 - M2 of a, then of b, with M = K R [I | -T] in pixel units, A^T A as ten sums, its smallest eigenvector
 *               w by the same cyclic Jacobi rotations, X = w[:3] / w[3]: cv2.triangulatePoints of the two views.  It is
 *               VALID when X is finite, |w[3]| > 1e-12 |w|, the depth of X (third component of R (X - T)) is above
 *               min_depth in a and in b, and the angle between the rays X - T_a and X - T_b, atan2(|r_a x r_b|, r_a . r_b)
 *               in degrees, is at least min_pair_angle_deg.
 *   score       the used observations with |pi(K R (X - T)) - uv|^2 STRICTLY below threshold^2 and depth above min_depth;
 *               a non-finite value is no inlier; the pair's own two views are scored like any other.  A pair whose point
 *               is not valid scores 0.
 *   best        the largest count, the lowest h among equals (all counts 0: h = 0).  The mask is that of the best
 *               hypothesis, evaluated once more -- all zero when its point is not valid --, and pt_inliers is counted
 *               FROM that mask: mask, count and the refinement's input agree by construction.
 *   refinement  sfmba_triangulate's kernel (k_triangulate, unchanged) with the inlier mask as its obs_use and, as its
 *               pt_select, the points whose best hypothesis is valid with at least max(2, min_views) inliers: the n-view
 *               DLT over the inliers, Gauss-Newton and the verdict with max_iter, xtol, min_angle_deg, min_depth and
 *               max_error_px as there.  refine = 0: max_iter = 0 (the n-view DLT over the inliers and its verdict).
 *   verdict     first match wins (pt_status):
 *                  -1 the point was not selected
 *                   1 FEW_VIEWS     fewer used observations than max(2, min_views)
 *                   6 NO_CONSENSUS  no valid best hypothesis with at least max(2, min_views) inliers
 *                   2 AT_INFINITY / 3 BEHIND / 4 LOW_ANGLE / 5 HIGH_ERROR  k_triangulate's verdict over the inliers
 *                   0 OK            otherwise
 * X_out (P,3): the refined point for status 0, the point of x otherwise.  X_hyp (P,3): the best hypothesis' point wherever
 * it is valid -- NO_CONSENSUS for want of inliers still reports it, with the count, h and mask --, else the point of x.
 * inlier_mask (N, the caller's order): 0 for observations that took no part.  pt_views: used observations of a selected
 * point (else 0).  pt_inliers: the count of the mask.  pt_best: h of the best hypothesis; -1: not selected or FEW_VIEWS.
 * pt_iters, pt_rms_err, pt_angle_deg: k_triangulate's, over the inliers, for every point that reached it and got past
 * AT_INFINITY; else 0, NaN, NaN.  hyp_inliers (P,H): the count of every hypothesis (-1: it does not exist, or the point is
 * not selected or FEW_VIEWS).  n_ok: points with status 0.  kernel_us: with profile = 1 the HIP-event time of the call's
 * launches, else 0.
 *
 * pt_select, obs_use, NULL outputs and opt = NULL as for sfmba_triangulate.  Returns -1 when no problem is set, x is NULL,
 * an option is NaN, max_pairs < 1, hyp_inliers is asked for with P * H >= 2^31, or the handle waits for its transport.  As
 * sfmba_triangulate: on a sharded handle the call describes the LOCAL shard only (p is the local index); pixels are read
 * as stored (fp64 or fp32); every buffer is the call's own, sfmba_triangulate's or the statistics call's, so fun, grad, the
 * PCG record and a following solve are exactly what a fresh handle gives; no atomics, sums in a fixed order, a point's
 * results depend on nothing but its own inputs: same input, same bits. */
typedef struct sfmba_tri_ransac_options {
    double   threshold;          /* pixels (default 4.0) */
    double   min_depth;          /* an inlier, and a pair's point in its two views, has depth above this; the verdict's too (0.0) */
    double   min_pair_angle_deg; /* smallest angle between the two rays of a hypothesis (1.0) */
    uint64_t seed;               /* of the drawn pairs (0) */
    int32_t  max_pairs;          /* hypotheses per point, H, at least 1; a point with at most H pairs takes them all (64) */
    int32_t  min_views;          /* used observations a point needs, and inliers its best hypothesis needs; below 2 counts as 2 (2) */
    int32_t  refine;             /* 1 = Gauss-Newton over the inliers after their n-view DLT (1) */
    int32_t  profile;            /* 1 = kernel_us is measured (0) */
    int32_t  max_iter;           /* the refinement's trial points, as sfmba_triangulate's max_iter (default 10) */
    int32_t  reserved;
    double   xtol;               /* as sfmba_triangulate's xtol (default 1e-10) */
    double   min_angle_deg;      /* as sfmba_triangulate's min_angle_deg, over the inliers (default 1.0) */
    double   max_error_px;       /* as sfmba_triangulate's max_error_px, over the inliers (default +inf) */
} sfmba_tri_ransac_options;
void sfmba_default_tri_ransac_options(sfmba_tri_ransac_options* opt);
int  sfmba_triangulate_ransac(sfmba_handle* h, const double* x, const uint8_t* pt_select /* P or NULL = all */,
                              const uint8_t* obs_use /* N, caller's order, or NULL = all */,
                              const sfmba_tri_ransac_options* opt,
                              double* X_out /* (P,3) */, double* X_hyp /* (P,3) best hypothesis, unrefined */,
                              uint8_t* inlier_mask /* N, caller's order */, int32_t* pt_status, int32_t* pt_views,
                              int32_t* pt_inliers, int32_t* pt_best /* h */, int32_t* pt_iters,
                              double* pt_rms_err /* over the inliers */, double* pt_angle_deg, int32_t* hyp_inliers /* (P,H) */,
                              int64_t* n_ok, double* kernel_us);

/* ---- two-view geometry: F by RANSAC and pose recovery for a batch of edges (sfm.py:88-107, 120-180) -------------- */
/* A batch of edges (image pairs) that is independent of the bundle-adjustment problem: neither call needs
 * sfmba_set_problem, both ignore sfmba_set_precision (pairs are always fp64) and any transport, and both use buffers of
 * their own, so fun, grad, the PCG record and a following solve are exactly what a fresh handle gives.  No atomics, sums
 * in a fixed order: same input, same bits.
 *   n_edges, edge_ptr (n_edges + 1, ascending, edge_ptr[0] = 0), pts1, pts2 ((M,2) with M = edge_ptr[n_edges]: the pixels
 *   of pair k in image 1 and image 2), pair_use (M bytes, nonzero = take part; NULL = all).
 * An edge's "used pairs" are its pairs with pair_use != 0 in stored order, numbered 0 .. n-1; a batch with a mask gives
 * bit for bit what the batch with those pairs removed gives.
 *
 * sfmba_fundamental_ransac: the reference's estimate_fundamental_matrix_ransac (cv2_lite/fundamental_matrix_estimation.py)
 * for every edge, H = max_iters hypotheses each, without early exit (the reference has none).
 *   hypothesis  estimate_fundamental_matrix on eight used pairs: each image's eight points minus their column means, over
 *               ONE scale, the standard deviation of all 16 coordinates together (np.std(pts) as the reference writes it;
 *               neither per axis nor Hartley's sqrt 2); rows of construct_matrix_A; f = the eigenvector of the smallest
 *               eigenvalue of A^T A (cyclic Jacobi on the 9x9 matrix, pairs (0,1), (0,2), .., (7,8), until the off-diagonal
 *               part is 1e-40 of the diagonal, at most 30 sweeps); rank 2 by removing the smallest singular direction,
 *               F <- F - (F v3) v3^T with v3 the smallest eigenvector of F^T F; then T2^T F T1.
 *   score       THE REFERENCE'S RULE, NOT OpenCV's: the one-sided distance in image 2, |x2^T F x1| / sqrt(l0^2 + l1^2) with
 *               l = F x1, is STRICTLY below threshold; a non-finite distance is no inlier.  (cv2.findFundamentalMat takes
 *               the larger of the distances in both images.)
 *   best        the largest inlier count, the lowest h among equals (Python's max keeps the first)
 *   samples     given: (n_edges, H, 8) int32 positions among the used pairs; a position outside 0 .. n-1 makes the call
 *               return -1, a sample with a repeated position is invalid: its count is -1.  NULL: drawn by a counter-based
 *               rule, so that a result depends neither on the grid nor on the order of execution:
 *                 mix(z): z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31
 *                 key = mix(seed ^ mix(e << 32 | h)), e the edge's position in the batch
 *                 draw j = 0..7: k = mix(key + (j + 1) 0x9e3779b97f4a7c15) mod (n - j); then, for every earlier choice c
 *                 in ascending order of c, if (k >= c) ++k
 *   refit = 1   F_refit: the same estimate_fundamental_matrix over ALL inliers of the best hypothesis (45 sums of A^T A
 *               in a fixed order, the same Jacobi, rank 2, denormalised).  refit = 0: F_refit is a copy of F.
 * F and F_refit (n_edges,9) have unit Frobenius norm and their entry of largest magnitude positive.  inlier_mask (M):
 * the mask of the best hypothesis, 0 for pairs that took no part.  edge_inliers, edge_best: count and h of the best
 * hypothesis.  edge_success: inliers / n >= confidence (the reference's `success`).  edge_status: 0 OK; 1 FEW_PAIRS
 * (n < 8); 2 DEGENERATE (no hypothesis with a finite F and at least 8 inliers).  For a status other than 0, F and F_refit
 * are zero; DEGENERATE still reports the count, h and mask of its best hypothesis (the reference returns that hypothesis
 * whatever its count), FEW_PAIRS reports 0, -1 and an empty mask.  hyp_inliers (n_edges,H): the count of every hypothesis (-1:
 * invalid sample, or FEW_PAIRS).  n_ok: edges with status 0.  kernel_us: with profile = 1 the HIP-event time of the call's
 * launches, else 0.
 *
 * sfmba_recover_pose: the reference's recover_pose (cv2_lite/recover_pose.py) for every edge, E (n_edges,9) row-major, K (9).
 *   decomposition  eigenvectors v1 v2 v3 of E^T E by a 3x3 Jacobi, by descending eigenvalue, v1 and v2 with their
 *                  component of largest magnitude positive (the sign decides which rotation is R1), v3 flipped so that det V = +1;
 *                  s_i = |E v_i|, u1 = E v1 / s1, u2 = E v2 / s2 made orthogonal to u1 and of unit length, u3 = u1 x u2; R1 = U W V^T,
 *                  R2 = U W^T V^T with the W of decompose_essential_matrix (both determinants +1 by construction), t = u3;
 *                  candidates in the order (R1,t), (R1,-t), (R2,t), (R2,-t)
 *   choice         every used pair is triangulated against every candidate by the two-view DLT (the rows of
 *                  triangulate_points_linear2 with M1 = K [I | 0], M2 = K [R | t]; smallest eigenvector of the 4x4 A^T A,
 *                  unknowns neither translated nor rescaled).  A pair is in front when both depths are finite and
 *                  > min_depth.  Most pairs in front wins, the earliest candidate among equals.  The reference refines the
 *                  points before it counts; this call does not (sfmba_triangulate refines points).
 * R (n_edges,9), t (n_edges,3): x2 = R x1 + t, |t| = 1.  front_mask (M), X (M,3; NaN for pairs that took no part),
 * angle_deg (M): the angle between the rays X - O1 and X - O2 (O1 = 0, O2 = -R^T t) as atan2(|a x b|, a . b), NaN where
 * the pair is not in front.  edge_front: the winner's count; edge_front_all (n_edges,4): every candidate's.
 * edge_sum_err: the reference's reproj_err total (both images) over the used pairs.  edge_status, first match wins: 0 OK;
 * 1 FEW_PAIRS (no used pair); 2 DEGENERATE (anything non-finite in E, or s2 <= 1e-12 s1; outputs zero / NaN); 3 TIE (the
 * winner's count is not above the runner-up's; the winner is still returned).  n_ok, kernel_us as above.
 *
 * Every output pointer may be NULL, and an array that is not asked for is not downloaded.  opt = NULL: the defaults.
 * Both return -1 for a malformed batch (edge_ptr not ascending from 0, NULL pixels), a NaN option or max_iters < 1. */
typedef struct sfmba_ransac_options {
    double   threshold;   /* pixels (default 1.0, the reference's; sfm.py passes 0.1) */
    double   confidence;  /* edge_success = inliers / n >= confidence (0.99) */
    uint64_t seed;        /* of the drawn samples (0) */
    int32_t  max_iters;   /* hypotheses per edge, H, the same for all edges, at least 1 (1000) */
    int32_t  refit;       /* 1 = F_refit over all inliers of the best hypothesis (0) */
    int32_t  profile;     /* 1 = kernel_us is measured (0) */
    int32_t  reserved;
} sfmba_ransac_options;
void sfmba_default_ransac_options(sfmba_ransac_options* opt);
int  sfmba_fundamental_ransac(sfmba_handle* h, int64_t n_edges, const int64_t* edge_ptr, const double* pts1, const double* pts2,
                              const uint8_t* pair_use /* M or NULL = all */, const int32_t* samples /* (n_edges,H,8) or NULL = drawn */,
                              const sfmba_ransac_options* opt, double* F, double* F_refit, uint8_t* inlier_mask,
                              int32_t* edge_inliers, int32_t* edge_best, uint8_t* edge_success, int32_t* edge_status,
                              int32_t* hyp_inliers, int64_t* n_ok, double* kernel_us);
/* sfmba_homography_ransac: a homography x2 ~ H x1 by RANSAC for every edge, H = max_iters hypotheses each, without early
 * exit: the sibling of sfmba_fundamental_ransac (what cv2.findHomography(.., cv2.RANSAC) estimates before its refinement).
 * The batch (n_edges, edge_ptr, pts1, pts2, pair_use, "used pairs") and sfmba_ransac_options are those of the F call;
 * a batch with a mask gives bit for bit what the batch with those pairs removed gives.  No atomics, sums in a fixed
 * order: same input, same bits.  Buffers are shared with the F call and grow only; neither call changes what the other,
 * or a following solve, computes.
 *   hypothesis  four used pairs: each image's four points minus their column means, over ONE scale, the standard
 *               deviation of all 8 coordinates together (np.std(pts), the normalisation of the F call); T1 and T2 are the
 *               matrices that do this, T = [[1/s, 0, -mx/s], [0, 1/s, -my/s], [0, 0, 1]].  A normalised pair (x, y) -> (u, v)
 *               gives the two rows
 *                 [-x, -y, -1,  0,  0,  0, u x, u y, u]
 *                 [ 0,  0,  0, -x, -y, -1, v x, v y, v]
 *               of the 8 x 9 matrix A, the four first rows before the four second rows; h = the eigenvector of the
 *               smallest eigenvalue of A^T A (the cyclic Jacobi of the F call: pairs (0,1), (0,2), .., (7,8), until the
 *               off-diagonal part is 1e-40 of the diagonal, at most 30 sweeps), Hn = h as 3 x 3 row-major; then
 *               H = T2^-1 Hn T1 with T2^-1 = [[s2, 0, m2x], [0, s2, m2y], [0, 0, 1]] in closed form.
 *   score       q = H (x1, y1, 1); d2 = (q0/q2 - x2)^2 + (q1/q2 - y2)^2; the pair is an inlier when d2 is finite and
 *               STRICTLY below threshold^2.  One-sided in image 2, as cv2.findHomography's and as the F call's.
 *   best        the largest inlier count, the lowest h among equals
 *   samples     given: (n_edges, H, 4) int32 positions among the used pairs; a position outside 0 .. n-1 makes the call
 *               return -1, a sample with a repeated position is invalid: its count is -1.  NULL: drawn by the counter-based
 *               rule of the F call with four draws: key = mix(seed ^ mix(e << 32 | h)); draw j = 0..3:
 *               k = mix(key + (j + 1) 0x9e3779b97f4a7c15) mod (n - j); then, for every earlier choice c in ascending
 *               order of c, if (k >= c) ++k
 *   finish      inlier_mask and edge_inliers are evaluated once more from the best H (one place decides count, success,
 *               status and the refit's pairs).
 *   refit = 1   H_refit: the same estimate over ALL inliers of the best hypothesis: means and scale over the inliers,
 *               both rows of every inlier, the 45 sums of A^T A in a fixed order, the same Jacobi, denormalised.  When the
 *               result is not finite, H_refit is a copy of H.  refit_mask and edge_refit_inliers: the used pairs scored
 *               against H_refit AS RETURNED (unit norm) with the expression of the score.
 *               refit = 0, or a status other than 0: H_refit, refit_mask and edge_refit_inliers are copies of H,
 *               inlier_mask and edge_inliers.
 * Hm and H_refit (n_edges,9) have unit Frobenius norm and their entry of largest magnitude (the first of equals)
 * positive.  inlier_mask, refit_mask (M): 0 for pairs that took no part.  edge_inliers, edge_best: count and h of the best
 * hypothesis.  edge_success: inliers / n >= confidence.  edge_status: 0 OK; 1 FEW_PAIRS (n < 4): count 0, best -1, empty
 * masks, every hyp_inliers entry -1; 2 DEGENERATE (no hypothesis with a finite H and at least 4 inliers): both H are zero,
 * the count, h and mask of the best hypothesis are still reported (best -1 and an empty mask when no sample was valid).
 * hyp_inliers (n_edges,H): the count of every hypothesis (-1: invalid sample, or FEW_PAIRS).  n_ok: edges with status 0.
 * kernel_us: with profile = 1 the HIP-event time of the call's launches, else 0.  Every output pointer may be NULL.
 * Returns -1 for a malformed batch, a NaN option, max_iters < 1 or a sample position outside 0 .. n-1.
 * Not done here: the LM refinement cv2 runs after its RANSAC, a symmetric transfer error, the orientation / collinearity
 * pre-test of a sample, the decomposition of H into poses, adaptive exit. */
int  sfmba_homography_ransac(sfmba_handle* h, int64_t n_edges, const int64_t* edge_ptr, const double* pts1, const double* pts2,
                             const uint8_t* pair_use /* M or NULL = all */, const int32_t* samples /* (n_edges,H,4) or NULL = drawn */,
                             const sfmba_ransac_options* opt, double* Hm, double* H_refit, uint8_t* inlier_mask,
                             uint8_t* refit_mask, int32_t* edge_inliers, int32_t* edge_refit_inliers, int32_t* edge_best,
                             uint8_t* edge_success, int32_t* edge_status, int32_t* hyp_inliers, int64_t* n_ok, double* kernel_us);
/* sfmba_similarity_ransac: a similarity dst ~ s R src + t between two sets of 3-D points by RANSAC, H = max_iters hypotheses
 * per set, without early exit: what relates two reconstructions (each lives in its own 7-dof gauge), or a reconstruction to
 * positions known from outside.  A batch of n_sets SETS plays the part of the edges: set_ptr (n_sets + 1) ascending from 0 to
 * M, src and dst (M,3) row-major, pair_use (M) or NULL = all; "used pairs" are those of the mask in stored order, n of them in
 * a set.  sfmba_ransac_options are those of the F call; threshold is a DISTANCE IN THE UNITS OF dst (the default 1.0 means
 * nothing here: pass one).  A batch with a mask gives bit for bit what the batch with those pairs removed gives; set e of a
 * batch is a one-set batch given that set's samples.  No atomics, sums in a fixed order: same input, same bits.  Buffers are
 * shared with the two-view calls and grow only; no call changes what another, or a following solve, computes.
 *   hypothesis  three used pairs a_k -> b_k (k = 0, 1, 2 in the sample's order), Horn's closed form (J. Opt. Soc. Am. A 4,
 *               1987): the means am, bm (sum / 3); the centred a'_k = a_k - am, b'_k = b_k - bm; the nine sums
 *               S_ij = sum_k a'_k,i b'_k,j and saa = sum_k |a'_k|^2, accumulated in the order k = 0, 1, 2; the symmetric
 *                 N = [ Sxx+Syy+Szz  Syz-Szy       Szx-Sxz       Sxy-Syx     ]
 *                     [ .            Sxx-Syy-Szz   Sxy+Syx       Szx+Sxz     ]
 *                     [ .            .            -Sxx+Syy-Szz   Syz+Szy     ]
 *                     [ .            .             .            -Sxx-Syy+Szz ];
 *               q = (w, x, y, z) the eigenvector of N's largest eigenvalue l1 (cyclic Jacobi on -N in registers, pairs
 *               (0,1), (0,2), .., (2,3), until the off-diagonal part is 1e-40 of the diagonal, at most 12 sweeps), divided
 *               by its norm; R the rotation of q,
 *                 [ w2+x2-y2-z2  2(xy-wz)     2(xz+wy)    ]
 *                 [ 2(xy+wz)     w2-x2+y2-z2  2(yz-wx)    ]
 *                 [ 2(xz-wy)     2(yz+wx)     w2-x2-y2+z2 ], always proper: there is no reflection case;
 *               s = sum_k b'_k . (R a'_k) / saa, evaluated as sum_ij R_ji S_ij / saa; t = bm - s R am.  With this s it is
 *               Umeyama's least-squares estimate whenever that has det > 0.
 *               NO SOLUTION (the sample is valid, its count is 0): l1 - l2 is not above 1e-9 (l1 - l4), l1 >= l2 >= l3 >= l4
 *               the eigenvalues of N -- a collinear or repeated triple, the rotation about the line is free --, or saa or s
 *               is not positive, or anything of (s, R, t) is not finite.
 *   score       d2 = |s R a + t - b|^2 of a used pair; an inlier when d2 is finite and STRICTLY below threshold^2.
 *               One-sided, in the frame and units of dst.
 *   best        the largest inlier count, the lowest h among equals
 *   samples     given: (n_sets, H, 3) int32 positions among the used pairs; a position outside 0 .. n-1 makes the call
 *               return -1, a sample with a repeated position is invalid: its count is -1.  NULL: drawn by the counter-based
 *               rule of the F call with three draws: key = mix(seed ^ mix(e << 32 | h)), e the set's position in the batch;
 *               draw j = 0..2: k = mix(key + (j + 1) 0x9e3779b97f4a7c15) mod (n - j); then, for every earlier choice c in
 *               ascending order of c, if (k >= c) ++k
 *   finish      inlier_mask and set_inliers are evaluated once more from the best (s, R, t) (one place decides count,
 *               success, status and the refit's pairs).
 *   refit = 1   sim_refit: the same estimate over ALL inliers of the best hypothesis: the means over the inliers first,
 *               then S_ij and saa about them, each a sum in a fixed order; the same N, Jacobi, R, s, t.  When that has no
 *               solution, sim_refit is a copy of sim.  refit_mask and set_refit_inliers: the used pairs scored against
 *               sim_refit AS RETURNED with the expression of the score.
 *               refit = 0, or a status other than 0: sim_refit, refit_mask and set_refit_inliers are copies of sim,
 *               inlier_mask and set_inliers.
 * sim and sim_refit (n_sets,13): s, R (9, row-major), t (3).  inlier_mask, refit_mask (M): 0 for pairs that took no part.
 * set_inliers, set_best: count and h of the best hypothesis.  set_success: inliers / n >= confidence.  set_status: 0 OK;
 * 1 FEW_PAIRS (n < 3): count 0, best -1, empty masks, every hyp_inliers entry -1; 2 DEGENERATE (no hypothesis with a
 * solution and at least 3 inliers): both similarities are zero, the count, h and mask of the best hypothesis are still
 * reported (count 0 and an empty mask when the best sample had no solution; best -1 when no sample was valid).  A
 * triple whose two triangles are similar fits its own similarity exactly, so a set without a common one can still be OK
 * with a count of a handful (a mirrored copy: every triangle is congruent to its image, and a mirror image of a plane is a
 * rotation of it): the caller decides how many inliers are enough.  hyp_inliers (n_sets,H): the count of every hypothesis (-1: invalid
 * sample, or FEW_PAIRS).  n_ok: sets with status 0.  kernel_us: with profile = 1 the HIP-event time of the call's launches,
 * else 0.  Every output pointer may be NULL, and an array that is not asked for is not downloaded.
 * Returns -1 for a malformed batch, a NaN option, max_iters < 1 or a sample position outside 0 .. n-1.
 * Not done here: adaptive exit, local optimisation of the best hypothesis, a reflection model, a robust weight in the refit. */
int  sfmba_similarity_ransac(sfmba_handle* h, int64_t n_sets, const int64_t* set_ptr, const double* src, const double* dst,
                             const uint8_t* pair_use /* M or NULL = all */, const int32_t* samples /* (n_sets,H,3) or NULL = drawn */,
                             const sfmba_ransac_options* opt, double* sim /* (n_sets,13) */, double* sim_refit, uint8_t* inlier_mask,
                             uint8_t* refit_mask, int32_t* set_inliers, int32_t* set_refit_inliers, int32_t* set_best,
                             uint8_t* set_success, int32_t* set_status, int32_t* hyp_inliers, int64_t* n_ok, double* kernel_us);
/* sfmba_essential_ransac: the essential matrix x2^T E x1 = 0 (x in camera coordinates) by five-point RANSAC for every edge,
 * H = max_iters hypotheses each, without early exit: the calibrated sibling of sfmba_fundamental_ransac (what
 * cv2.findEssentialMat(pts1, pts2, K, cv2.RANSAC) estimates).  The batch (n_edges, edge_ptr, pts1, pts2, pair_use, "used
 * pairs") and sfmba_ransac_options are those of the F call; K (9, row-major) is ONE camera matrix for the whole batch and
 * both images.  A batch with a mask gives bit for bit what the batch with those pairs removed gives; edge e of a batch
 * gives what the one-edge batch gives.  No atomics, sums in a fixed order: same input, same bits.  Buffers are shared
 * with the F and H calls and grow only; no call changes what another, or a following solve, computes.
 *   hypothesis  five used pairs.  A pixel (x, y) goes to camera coordinates by q = K^-1 (x, y, 1), (q0/q2, q1/q2) (K^-1 in
 *               closed form by cofactors); nothing else is normalised.  A pair gives the row of construct_matrix_A of the
 *               F call, [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1], of the 5 x 9 matrix A.  The eigenvectors of the
 *               four smallest eigenvalues of A^T A (the cyclic Jacobi of the F call, the same order of pairs and the same
 *               caps), by ascending eigenvalue, the lower column first among equals, are X, Y, Z, W (3 x 3 row-major), and
 *               E = x X + y Y + z Z + W.  A sample whose rows have no rank 5 -- the fifth-smallest eigenvalue is not above
 *               1e-12 times the largest, as for five collinear points -- has no candidate: 0 roots, count 0.
 *   constraints det E = 0 and the nine entries (row-major) of 2 E E^T E - tr(E E^T) E = 0: ten cubics in x, y, z, written
 *               as a 10 x 20 matrix over the monomials in Nister's order
 *                 x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
 *               Gauss-Jordan elimination with partial pivoting (the first row of equal magnitudes) makes the left 10 x 10
 *               block the identity.  With <m> the reduced row of monomial m, the three differences <x^2z> - z <x^2>,
 *               <y^2z> - z <y^2>, <xyz> - z <xy> hold only x, y and 1 times polynomials in z: B(z) (x, y, 1)^T = 0, B 3 x 3
 *               with columns of degree 3, 3, 4.  det B(z) has degree 10.
 *   roots       EVERY real root z of det B(z): a zero leading coefficient lowers the degree; the roots of the derivatives
 *               of every order, found from the highest down, cut the interval of the Cauchy bound 1 + max |c_k / c_n| into
 *               stretches on which the next polynomial is monotonic; a sign change over a stretch is one root, found by
 *               Newton steps inside a bracket that is bisected when a step leaves it or shrinks by less than half (at most
 *               100 steps).  A simple real root is never missed.  A non-finite coefficient: no root.
 *   candidates  one per root, by ascending z (0 to 10): (x, y, 1) is the null vector of B(z), the cross product of the two
 *               rows of B(z) whose product is the longest (rows 0 1, then 0 2, then 1 2 among equals) divided by its last
 *               entry; E = x X + y Y + z Z + W; F_pix = K^-T E K^-1.
 *   score       the F call's, applied to F_pix: |x2^T F x1| / sqrt(l0^2 + l1^2) with l = F x1, in pixels, one-sided in image
 *               2, STRICTLY below threshold; a non-finite distance is no inlier.  Counts are comparable with the F and H
 *               calls'.  The count of a hypothesis is its best candidate's, the lower z among equals; a hypothesis with no
 *               real root or no finite candidate counts 0.
 *   best        the largest count, the lowest h among equals
 *   samples     given: (n_edges, H, 5) int32 positions among the used pairs; a position outside 0 .. n-1 makes the call
 *               return -1, a sample with a repeated position is invalid: its count is -1.  NULL: drawn by the counter-based
 *               rule of the F call with five draws.
 *   polish      the best candidate of the best hypothesis once more, in homogeneous coordinates: v = its parts along X, Y, Z,
 *               W at unit length; two Gauss-Newton steps on the ten cubics c(v) = 0 with the step kept orthogonal to v,
 *               (J^T J + v v^T) d = -J^T c, v <- (v + d) / |v + d|; E = v0 X + v1 Y + v2 Z + v3 W and its F_pix.  (The four
 *               null vectors share one eigenvalue, so their basis is whatever the eigensolver returns, and the chart W = 1
 *               loses digits when the solution has a small W part in it.)  A step that is not finite leaves the candidate.
 *   finish      inlier_mask and edge_inliers are evaluated once more from the bits of the polished F_pix; hyp_inliers
 *               holds the counts before the polish.
 * E (n_edges,9): the best candidate's E with unit Frobenius norm and its entry of largest magnitude (the first of equals)
 * positive -- [t]x R has two largest entries of nearly equal magnitude, so compare E up to sign.  inlier_mask (M): 0 for pairs
 * that took no part.  edge_inliers, edge_best, edge_best_root: count, h and candidate number (by ascending z) of the best
 * hypothesis.  edge_success: inliers / n >= confidence.  edge_status: 0 OK; 1 FEW_PAIRS (n < 5): count 0, best -1, root -1, empty
 * mask; 2 DEGENERATE (no hypothesis with a finite E and at least 5 inliers): E is zero, the count, h, root and mask of the best
 * hypothesis are still reported (-1, -1 and an empty mask when no sample was valid; root -1 when it had no real root).
 * hyp_inliers, hyp_roots (n_edges,H): the count and the number of real roots of every hypothesis (-1: invalid sample, or
 * FEW_PAIRS).  n_ok: edges with status 0.  kernel_us: with profile = 1 the HIP-event time of the call's launches, else 0.
 * Every output pointer may be NULL.
 * Returns -1 for a malformed batch, a NaN option, max_iters < 1, a sample position outside 0 .. n-1, a NULL, non-finite or
 * singular K, and opt->refit != 0.
 * Not done here: a refit or local optimisation over the inliers (a linear eight-point refit would bring the planar
 * degeneracy back), adaptive exit, different intrinsics for the two images, cv2's Sampson score, making a planar first
 * pair usable (all points in one plane leave a two-fold ambiguity). */
int  sfmba_essential_ransac(sfmba_handle* h, int64_t n_edges, const int64_t* edge_ptr, const double* pts1, const double* pts2,
                            const uint8_t* pair_use /* M or NULL = all */, const int32_t* samples /* (n_edges,H,5) or NULL = drawn */,
                            const double* K, const sfmba_ransac_options* opt, double* E, uint8_t* inlier_mask,
                            int32_t* edge_inliers, int32_t* edge_best, int32_t* edge_best_root, uint8_t* edge_success,
                            int32_t* edge_status, int32_t* hyp_inliers, int32_t* hyp_roots, int64_t* n_ok, double* kernel_us);
typedef struct sfmba_pose_options {
    double  min_depth;   /* a pair is in front when both depths are above this (0.0) */
    int32_t profile;     /* 1 = kernel_us is measured (0) */
    int32_t reserved;
} sfmba_pose_options;
void sfmba_default_pose_options(sfmba_pose_options* opt);
int  sfmba_recover_pose(sfmba_handle* h, int64_t n_edges, const int64_t* edge_ptr, const double* pts1, const double* pts2,
                        const uint8_t* pair_use /* M or NULL = all */, const double* E, const double* K,
                        const sfmba_pose_options* opt, double* R, double* t, uint8_t* front_mask, double* X, double* angle_deg,
                        int32_t* edge_front, int32_t* edge_front_all, double* edge_sum_err, int32_t* edge_status,
                        int64_t* n_ok, double* kernel_us);

/* ---- descriptor matching: 2 nearest neighbours and the ratio test for a batch of image pairs (sfm.py:94-96) -------- */
/* What produces the pixel pairs of the two-view calls: for every ordered pair of images the reference runs
 * BFMatcher(NORM_L2).knnMatch(desc_u, desc_v, k=2) and Lowe's test m.distance < 0.5 * n.distance.  Here a set of images'
 * descriptors is put on the device once (sfmba_set_descriptors) and any number of batches of (query image, train image)
 * edges are matched against it (sfmba_match_descriptors, one launch of k_match per batch).  Neither call needs
 * sfmba_set_problem; both use buffers of their own, so fun, grad, the PCG record and a following solve are exactly what
 * a fresh handle gives.  No atomics: same input, same bits.
 *
 * sfmba_set_descriptors: n_images images; image i owns rows img_ptr[i] .. img_ptr[i+1] - 1 of desc, (N, dim) row-major,
 * uint8 (dtype 0) or float32 (dtype 1), 1 <= dim <= 512.  The set takes one of two forms, reported in form_out and by
 * sfmba_get_form(h, "match_form", ..):
 *   1, form A  every value is an integer in 0..255 and dim <= 256 (what cv2.SIFT emits): uint8 input of that width
 *              always, float32 input when a pass over it on the device finds it so.  Stored as fp16; the dot products
 *              are fp16 MFMAs with fp32 accumulation, in which every product and partial sum is an integer below 2^24;
 *              d^2 = |a|^2 + |b|^2 - 2 a.b is formed in integers.  Distances are the exact integers.
 *   2, form B  anything else.  Stored as fp32; dot products are fp32 MFMAs (an fp32 fma chain over k), norms and
 *              |a|^2 + |b|^2 - 2 a.b are fp64, the top two are kept by that value; the two winners' distances are then
 *              recomputed as sum (a - b)^2 in fp64 over the fp32 values, and these decide their order, the ratio test and
 *              dist_sq.  A pair of candidates whose true distances differ by less than 4 dim 2^-24 |a| max|b| may come
 *              out in the other order or lose the second place to the third.
 * The buffers of a set are freed by the next sfmba_set_descriptors and by sfmba_destroy.
 *
 * sfmba_match_descriptors: edges (n_edges, 2) int32: query image u, train image v (u == v is allowed: every row's
 * nearest neighbour is then itself at distance 0).  The outputs are per query row, the edges' query images one after
 * another: query_ptr (n_edges + 1) with Q = query_ptr[n_edges] = the sum of the rows of the edges' query images.
 *   order       the candidates of a query are ordered by (d^2, train index) lexicographically: the lower index wins an
 *               exact tie.  A result depends neither on the tiles, the grid, nor the batch its edge is part of.
 *   idx (Q,2)   the nearest and the second nearest train row (index within the train image); dist_sq (Q,2) their d^2
 *   good (Q)    d1^2 < ratio^2 d2^2, strictly, in fp64, ratio^2 = ratio * ratio in fp64 (default ratio 0.5, sfm.py's).
 *               For integer descriptors this is cv2's test on the float32 roots as long as correctly rounded float32
 *               roots of distinct integers stay distinct (d^2 < 2^22 by our derivation; not verified against OpenCV).
 *   too few     a train image with fewer than 2 rows or a query image with none: edge_status 1 (FEW), every idx -1,
 *               dist_sq +inf, good 0 (the reference's `for m, n in matches` raises there); else edge_status 0
 *   non-finite  a train row whose distance to the query is not finite is never a neighbour; a query left with fewer than
 *               two neighbours gets idx -1 and dist_sq +inf for the missing ones and good 0
 *   edge_good   the number of good queries of the edge;  n_ok: edges with status 0;  kernel_us: with profile = 1 the
 *               HIP-event time of the launch, else 0.
 * form: 0 the set's own form; 1 form A, -1 when the set does not qualify; 2 form B whatever the values (built from the
 * set at the first such call); on integer data both forms give the same idx, dist_sq and good.
 * Every output pointer may be NULL, and an array that is not asked for is not downloaded.  opt = NULL: the defaults.
 * Returns -1 for a malformed img_ptr (not ascending from 0), an image id out of range, dim outside 1..512, a NaN or
 * non-positive ratio, or a call made before sfmba_set_descriptors. */
int  sfmba_set_descriptors(sfmba_handle* h, int64_t n_images, const int64_t* img_ptr /* n_images + 1, ascending from 0 */,
                           const void* desc /* (N, dim) row-major */, int32_t dtype /* 0 uint8, 1 float32 */,
                           int32_t dim /* 1..512 */, int32_t* form_out);
typedef struct sfmba_match_options {
    double  ratio;       /* Lowe's ratio (0.5) */
    int32_t form;        /* 0 = the set's form, 1 = A, 2 = B (0) */
    int32_t profile;     /* 1 = kernel_us is measured (0) */
} sfmba_match_options;
void sfmba_default_match_options(sfmba_match_options* opt);
int  sfmba_match_descriptors(sfmba_handle* h, int64_t n_edges, const int32_t* edges /* (n_edges,2): query image, train image */,
                             const sfmba_match_options* opt, int64_t* query_ptr /* n_edges + 1 */, int32_t* idx /* (Q,2) */,
                             double* dist_sq /* (Q,2) */, uint8_t* good /* Q */, int32_t* edge_good, int32_t* edge_status,
                             int64_t* n_ok, double* kernel_us);

/* ---- feature tracks: the connected components of the matches (sfm.py:109-117, graph.py:101-119) ------------------- */
/* What turns the pair lists of the matched edges into the index arrays of a problem: which features of which images are
 * the same 3-D point.  The vertices are the features that occur in a used pair, the edges are the used pairs, and a
 * track is a connected component (the transitive closure of the matches, not the reference's one-hop sets, and
 * independent of the order of edges and pairs).  Neither call needs sfmba_set_problem or sfmba_set_descriptors; both use
 * buffers of their own, freed by the next sfmba_build_tracks and by sfmba_destroy, so fun, grad, the PCG record and a
 * following solve are exactly what a fresh handle gives.
 *
 * Input: n_images images; image i owns the global feature ids img_ptr[i] .. img_ptr[i+1] - 1 (the convention of
 * sfmba_set_descriptors), N = img_ptr[n_images] < 2^31.  edges (n_edges, 2) int32 of images (u, v), u != v, in either
 * orientation and possibly repeated; edge e owns the pairs pair_ptr[e] .. pair_ptr[e+1] - 1 of pairs (M, 2) int32: row in
 * u, row in v; a pair may be repeated.  pair_use (M) uint8 or NULL: a pair with 0 takes no part (it is still checked).
 *
 * A component becomes a track when it has at least min_length features and, with max_length > 0, at most max_length,
 * and when it holds no two features of one image or conflicts = 1.  (A component has two features or more, so
 * min_length 1 and 2 ask for the same.)  Tracks are numbered by ascending smallest global feature id; within a track the
 * observations ascend by global feature id, that is by image and then by row.
 *   feat_track (N)   the feature's track, or -1: in no used pair; -2: its component was dropped for its length; -3: its
 *                    component was dropped for a conflict (also when the length fails as well)
 *   counts (6)       components, tracks kept, dropped as too short, dropped as too long, dropped for a conflict (a
 *                    component that also fails a length test counts here only), T = observations of the kept tracks
 *   kernel_us        with profile = 1 the HIP-event time over all launches of the call, else 0
 * sfmba_get_tracks returns the CSR of the last build: track_ptr (n_tracks + 1) int64, track_feat (T) global feature ids,
 * track_image (T), n_tracks = counts[1]; any of them may be NULL.
 * The result is a pure function of the input: the same bits whatever the grid, the schedule, or the order of edges and
 * pairs.  Zero edges, zero pairs and a pair_use of zeros are valid: no track, feat_track all -1.
 * Returns -1, before any kernel reads a pair, for img_ptr or pair_ptr not ascending from 0, an image id out of range,
 * u == v, a row outside its image, N >= 2^31, min_length < 1, a non-zero max_length below min_length, conflicts other
 * than 0 or 1, and for sfmba_get_tracks before a successful build. */
typedef struct sfmba_track_options {
    int32_t min_length;  /* fewest features of a track (2) */
    int32_t max_length;  /* most features of a track, 0 = no limit (0) */
    int32_t conflicts;   /* 0 = drop a component with two features of one image, 1 = keep it (0) */
    int32_t profile;     /* 1 = kernel_us is measured (0) */
} sfmba_track_options;
void sfmba_default_track_options(sfmba_track_options* opt);
int  sfmba_build_tracks(sfmba_handle* h, int64_t n_images, const int64_t* img_ptr /* n_images + 1, ascending from 0 */,
                        int64_t n_edges, const int32_t* edges /* (n_edges,2) */, const int64_t* pair_ptr /* n_edges + 1 */,
                        const int32_t* pairs /* (M,2) */, const uint8_t* pair_use /* M or NULL */,
                        const sfmba_track_options* opt, int32_t* feat_track /* N or NULL */, int64_t* counts /* 6 or NULL */,
                        double* kernel_us);
int  sfmba_get_tracks(sfmba_handle* h, int64_t* track_ptr, int32_t* track_feat, int32_t* track_image);

/* ---- view planning and problem assembly: the bookkeeping of an incremental reconstruction (sfm.py:59-71, 182-241) ---- */
/* Every round of the loop of SFM.construct asks which unregistered images see enough triangulated points (_select_edge,
 * over Node.pts3d_pts2d, graph.py:46-54) and what the index arrays of the problem over a given set of cameras and
 * tracks are (Graph.pt3ds_pt2ds, graph.py:186-191).  Both are sweeps over what the last successful sfmba_build_tracks
 * left on the device; n_images and n_tracks below are that build's (n_tracks = counts[1]) and are compared with it.
 * The calls read the tracks' tables and write buffers of their own: the tracks, the descriptor set, the problem, fun,
 * grad and a following solve are exactly what they are without these calls.  A mask entry is set when it is not 0.
 * The results are pure functions of the tracks and the masks: the same bits from call to call.
 *
 * sfmba_plan_views: cam_reg (n_images) uint8, the image is registered; trk_known (n_tracks) uint8, the track has a 3-D
 * point.  Outputs, each may be NULL:
 *   trk_reg_views (n_tracks) int32  the registered images among the views of track t
 *   img_tracks (n_images) int32     the features of image i that lie in a kept track
 *   img_known (n_images) int32      of those, the ones whose track is known: len(feat2point_index) of graph.py:46-54,
 *                                   the quantity _select_edge scores with
 *   img_gain (n_images) int32       the features of i whose track is not known and has trk_reg_views[t] - cam_reg[i] >= 1:
 *                                   the tracks that become (or already are) two-view once i is registered
 *   totals (3) int64                registered images, known tracks, tracks with trk_known == 0 and trk_reg_views >= 2
 *   kernel_us                       with profile = 1 the HIP-event time over the launches of the call, else 0
 *
 * sfmba_assemble_problem: cam_use (n_images), trk_use (n_tracks).  Observation k of track t is used when trk_use[t] and
 * cam_use[track_image[k]]; a track is in the sub-problem when it has at least min_views used observations; an image is
 * in it when cam_use is set and it has at least one used observation of such a track.  counts (3): cameras, points,
 * observations of the sub-problem.  sfmba_get_assembled then returns it (two calls because the sizes are not known
 * before the first); any pointer may be NULL:
 *   cam_of (cameras) int32          image id per sub-camera, ascending
 *   pt_of (points) int32            track id per sub-point, ascending
 *   camera_indices, point_indices   (observations) int64, renumbered through cam_of and pt_of: what sfmba_set_problem takes
 *   obs_feat (observations) int32   global feature id
 *   points_2d (observations, 2)     the pixels of obs_feat, gathered on the device from the table of sfmba_set_keypoints
 * in point-major order, ascending by feature id within a point, as the tracks' CSR is.
 *
 * sfmba_set_keypoints: the pixel positions pts (N, 2) fp64 of all features, once, with the img_ptr convention of
 * sfmba_set_descriptors.  Needs no tracks.  The table is compared with the tracks' img_ptr where points_2d is asked for,
 * and a sfmba_build_tracks with another img_ptr drops it.
 *
 * Return -1, with a message that starts with the function's name: sfmba_plan_views, sfmba_assemble_problem and
 * sfmba_get_assembled before a successful sfmba_build_tracks ("... sfmba_build_tracks first"); a mask of another length
 * than the build's or NULL; min_views < 1; sfmba_get_assembled before sfmba_assemble_problem on the current tracks, or
 * with points_2d and no (or another img_ptr's) keypoint table; img_ptr not ascending from 0, N >= 2^31 or a pixel that
 * is not finite for sfmba_set_keypoints. */
typedef struct sfmba_plan_options {
    int32_t min_views;   /* fewest used observations of a track of the sub-problem (2); sfmba_plan_views ignores it */
    int32_t profile;     /* 1 = kernel_us is measured (0) */
} sfmba_plan_options;
void sfmba_default_plan_options(sfmba_plan_options* opt);
int  sfmba_set_keypoints(sfmba_handle* h, int64_t n_images, const int64_t* img_ptr /* n_images + 1, ascending from 0 */,
                         const double* pts /* (N,2) */);
int  sfmba_plan_views(sfmba_handle* h, int64_t n_images, const uint8_t* cam_reg, int64_t n_tracks, const uint8_t* trk_known,
                      const sfmba_plan_options* opt, int32_t* trk_reg_views, int32_t* img_tracks, int32_t* img_known,
                      int32_t* img_gain, int64_t* totals /* 3 or NULL */, double* kernel_us);
int  sfmba_assemble_problem(sfmba_handle* h, int64_t n_images, const uint8_t* cam_use, int64_t n_tracks, const uint8_t* trk_use,
                            const sfmba_plan_options* opt, int64_t* counts /* 3 or NULL */, double* kernel_us);
int  sfmba_get_assembled(sfmba_handle* h, int32_t* cam_of, int32_t* pt_of, int64_t* camera_indices, int64_t* point_indices,
                         int32_t* obs_feat, double* points_2d);

/* ---- least_squares(method='trf', x_scale='jac') (sfm.py:266-268) ---------------------------- */
/* x_inout: x0 on entry, result.x on success (untouched on failure). */
int  sfmba_solve(sfmba_handle* h, double* x_inout, const sfmba_options* opt, sfmba_result* out);
/* The same with the start and the result in separate arrays (x_out may be x0): a caller that keeps x0 -- scipy's
   least_squares does not modify its argument -- saves the copy it would otherwise make for the in/out form. */
int  sfmba_solve_from(sfmba_handle* h, const double* x0, double* x_out, const sfmba_options* opt, sfmba_result* out);
/* After a successful sfmba_solve: result.fun (2N) and result.grad (6C+3P); either may be NULL. */
int  sfmba_get_fun_grad(sfmba_handle* h, double* fun_out, double* grad_out);

/* ---- covariance of a solution: camera and point blocks ------------------------------------------ */
/* How well the solution x is determined.  With r(x) the 2N residuals of sfmba_residuals, J = d r/d x from the analytic
 * blocks of the solver, D the set of HELD camera parameters and F its complement (every point parameter is free):
 *   U = J_F^T J_F,  V_p = sum Jp^T Jp (3x3 per point),  W_p = J_F^T Jp,  S = U - sum_p W_p V_p^-1 W_p^T.
 * kind = 0 (marginal):    Sigma_cc = sigma^2 S^-1 on F (rows and columns in D are zero),
 *                         Sigma_pp(p) = sigma^2 (V_p^-1 + V_p^-1 W_p^T S^-1 W_p V_p^-1).
 * kind = 1 (conditional): sigma^2 (U_cc|F)^-1 per camera with the points held, sigma^2 V_p^-1 per point with the cameras
 *                         held: cheap, available at every size, and optimistic.
 * sigma^2 = opt.sigma2 if > 0, else sum r^2 / dof with dof = 2N - (free parameters of observed cameras) - 3 (observed
 * points); dof <= 0: sigma^2 = 1 (info.dof says so).  No damping and no x_scale: the undamped J^T J at the caller's x.
 *
 * The held set D is the union of (1) all six parameters of every camera the problem holds (sfmba_set_fixed_cameras),
 * (2) the call's `hold` list: n_hold indices in [0, 6C), each one camera parameter (6 c + k: k = 0..2 the rotation vector,
 * 3..5 T), (3) with opt.gauge = 1 (default), ONLY when n_hold == 0 and the problem holds fewer than two cameras, the
 * usual "first camera plus one baseline coordinate": g0 = the held camera if there is one, else camera 0; g1 = the
 * observed camera with the largest |T - T_g0| at x (ties: lowest index); all six parameters of g0 and the one T
 * coordinate of g1 with the largest |T_g1 - T_g0| component (ties: lowest axis).  opt.gauge = 0 adds nothing: with nothing
 * held S has seven null directions and the call reports RANK_DEFICIENT.  A camera without observations is treated as held
 * and its blocks are NaN; a point without observations is skipped (pt_status = 3, NaN blocks).  held_out (6C bytes): 0 free,
 * 1 held, 2 unobserved.
 *
 * Rank is decided in the factorisations.  Cameras: a Cholesky pivot d_k <= opt.rank_tol S_kk (default 1e-10) ends the call
 * with info.status = 1 and info.bad_param = k.  Points: a point whose 3x3 Cholesky has a pivot <= opt.point_tol max diag V_p
 * (default 1e-12) gets pt_status = 1 (a single-view or otherwise undetermined point); any such point ends the call with
 * info.status = 2, info.n_bad_points and info.bad_point (the first).  After either, every matrix is NaN while pt_status and
 * held_out are valid, so the caller can trim the problem and call again.  A rank failure returns 0.
 *
 * Outputs (any may be NULL; an array that is not asked for is not downloaded, and the point sweep runs only when pt_cov or
 * pt_sigma is asked for): cam_cov (C,6,6) the diagonal blocks; cam_full (6C,6C) (kind = 1: block diagonal); cam_sigma
 * (C,2) sqrt of the largest eigenvalue of the rotation and of the T block; pt_cov (P,3,3); pt_sigma (P) sqrt of the largest
 * eigenvalue; pt_status (P) 0 fine, 1 undetermined, 3 no observation.  info.cost = 0.5 sum r^2; info.min_pivot_rel the
 * smallest d_k / S_kk met; info.kernel_us the device time of the call's kernels with opt.profile = 1.
 *
 * Returns -1 when no problem is set or x is NULL, an option is NaN or negative, a hold index is out of range or repeated,
 * the handle is sharded (a shard's covariance is not the problem's), the storage is fp32, or kind = 0 and the problem is
 * not on the dense form (6 C > 128, or its pair lists were not built); kind = 1 is limited only as the per-camera pass of
 * sfmba_reprojection_stats is.  The call works on buffers of its own: fun and grad of the last solve and the record the
 * next solve starts from are as they were.  Same input, same bits: no atomics; every sum runs in a fixed order. */
typedef struct sfmba_covariance_options {
    int32_t kind, gauge;
    double  sigma2, rank_tol, point_tol;
    int32_t profile, reserved;
} sfmba_covariance_options;
typedef struct sfmba_covariance_info {
    int32_t status, g0, g1, g1_axis, n_free, n_held, bad_param, reserved;
    int64_t dof, n_bad_points, bad_point;
    double  sigma2, cost, min_pivot_rel, kernel_us;
} sfmba_covariance_info;
void sfmba_default_covariance_options(sfmba_covariance_options* opt);
int  sfmba_covariance(sfmba_handle* h, const double* x, const int32_t* hold, int32_t n_hold,
                      const sfmba_covariance_options* opt, double* cam_cov /*(C,6,6)*/, double* cam_full /*(6C,6C) or NULL*/,
                      double* cam_sigma /*(C,2)*/, double* pt_cov /*(P,3,3)*/, double* pt_sigma /*P*/,
                      int32_t* pt_status /*P*/, uint8_t* held_out /*6C*/, sfmba_covariance_info* info);

/* ---- measurement / test entry points -------------------------------------------------------- */
/* `reps` back-to-back launches of one kernel at x, bracketed by HIP events on the handle's stream.
 * which: 0 residual+Jacobian sweep (with the point blocks V_p, g_p it leaves behind), 1 residual-only sweep,
 *        2 the camera pass of the normal equations (U_c, g_c, and the point rows the sweep's tiles cut),
 *        3 one implicit Schur product (pass A + pass B), 4 pass A alone, 5 pass B alone, 6 the reduced
 *        right-hand-side pass, 7 the residual+Jacobian sweep with its point-block sums switched off,
 *        10 a streaming-store fill of the Jacobian buffer (ceiling probe),
 *        11 k_jdot and 12 k_backsub (without its PCG prologue) in the form the problem has selected ("rc_consumers"),
 *        13 the per-observation sweep and 14 the per-point reduction of sfmba_reprojection_stats (default options),
 *        15 k_triangulate of sfmba_triangulate over every point and observation (default options),
 *        16 k_resect of sfmba_resect over every camera and observation (default options).
 *        17 k_pnp_ransac + k_pnp_finish of sfmba_resect_ransac over every camera and observation (default options).
 *        18 the kernels of sfmba_covariance with the default options, point sweep included (kind = 1 above 21 cameras).
 *        19 the kernels of sfmba_triangulate_ransac (k_tri_ransac, then k_triangulate over its mask) at the default
 *           options over every point and observation.
 * avg_us: average duration of one repetition. */
int  sfmba_time_kernel(sfmba_handle* h, const double* x, int32_t which, int32_t reps, double* avg_us);
/* Normal-equation blocks at x: U (C,21 upper triangle row-major), V (P,6 upper), gc (C,6), gp (P,3). */
int  sfmba_normal_blocks(sfmba_handle* h, const double* x, double* U, double* V, double* gc,
                         double* gp);
/* y = S v with S = U + diag(dc) - W (V + diag(dp))^-1 W^T at x (v, dc, y: 6C; dp: 3P). */
int  sfmba_schur_matvec(sfmba_handle* h, const double* x, const double* dc, const double* dp,
                        const double* v, double* y);

/* The two products of an outer iteration with the whole Jacobian, by the kernels the solver itself runs in the form the
 * problem has selected ("rc_consumers"): k_jdot, t1 = J sg with sum |t1|^2, and k_backsub for the camera step dc:
 * dp = (V + diag(dp_diag))^-1 (-g_p - sum Jp^T Jc dc) per point, t2 = J [dc; dp], and its ten sums
 * (t1.t2, t2.t2; g.p, |p / scale|^2, (D^2 g).p, |p|^2 of the point slice; the same four of the camera slice), where g and
 * the column scale are those of x, D^2 g of the cameras is sg, and D^2 g of the points is g_p * scale_p^2 as the solver has it.
 * x, sg: 6C+3P; dc: 6C; dp_diag: 3P.  t1_out: 2N in the caller's observation order; dp_out: 3P; sums_out: 10;
 * g_out, si_out (6C+3P, either may be NULL): the gradient and the inverse column scale the sums were formed with.
 * Single rank; 64-bit or 32-bit storage.  In 32-bit storage the fp32 OPERANDS of the two kernels are the stored Jacobian
 * blocks Jc, Jp (the float32 values sfmba_residual_jacobian returns; with the J-free iteration, debug option jfree, the
 * blocks are recomputed in fp64 and nothing of J is rounded) and the stored t1; everything formed from them is fp64:
 *   t1_out holds the stored float32 values of t1 exactly (each widened to a double);
 *   *g11_out is the sum of the squares of the UNROUNDED fp64 t1, which k_jdot sums before it stores;
 *   the sum t1.t2 of sums_out is formed by k_backsub with the STORED (rounded) t1 it reads back.
 * Leaves the handle as the other entries of this group do: a solve afterwards is the solve without the call. */
int  sfmba_step_products(sfmba_handle* h, const double* x, const double* sg, const double* dc, const double* dp_diag,
                         double* t1_out, double* g11_out, double* dp_out, double* sums_out, double* g_out, double* si_out);

/* The reduced right-hand-side + preconditioner pass of an outer iteration, by the kernels the solver itself runs in the
 * form the handle has decided (one workgroup per camera chunk with its own 6x6 inverse, or chunk sums combined and
 * inverted by a launch behind it; point data from the point records and the inverse blocks, or from the 128-byte
 * records; the wave-per-chunk form over the XCD-aware table).  At x, with J = [Jc | Jp] the Jacobian blocks of the
 * observations, W_i = Jc_i^T Jp_i (6x3), V_p = sum_{i in p} Jp_i^T Jp_i, g_p = sum_{i in p} Jp_i^T r_i,
 * U_c = sum_{i in c} Jc_i^T Jc_i, and the caller's diagonals dc (6C) and dp (3P):
 *     Vinv_p = (V_p + diag(dp_p))^-1,      e_p = +Vinv_p g_p   (the gradient of the point, not its negative),
 *     rhs_c  = -sum_{i in c} W_i e_p(i)    (6 per camera: the solver's reduced right-hand side is -g_c - rhs_c),
 *     sd_c   = +sum_{i in c} W_i Vinv_p(i) W_i^T   (21 per camera: upper triangle, row-major),
 *     minv_c = (U_c + diag(dc_c) - sd_c)^-1        (21 per camera: upper triangle, row-major; the values the PCG reads).
 * x: 6C+3P.  rhs_out: 6C, sd_out and minv_out: 21C, camera by camera.  A camera without observations has rhs = sd = 0.
 * Single rank, Schur-diagonal preconditioner (the default); 64-bit storage, or 32-bit storage with a recomputing pass A
 * (form "round_blocks" 0: the pass then reads nothing rounded but the pixels, as float32 values, behind g_p; with the
 * stored fp32 Jacobian it rounds its blocks and the call returns -1).  Leaves the handle as the other entries
 * of this group do: a solve afterwards is the solve without the call. */
int  sfmba_rhs_precond(sfmba_handle* h, const double* x, const double* dc, const double* dp, double* rhs_out,
                       double* sd_out, double* minv_out);

/* The fp32 operands of the mixed-precision Schur product (debug option "pcg_mixed"; the default with 32-bit storage) as
 * they stand after the last sfmba_schur_matvec: origin (3) the point the coordinates are rounded relative to,
 * rt32 (12 C floats: R row-major | T - origin per camera), rec32 (8 P floats per point: X - origin | z of the last
 * pass A | two unused floats; the z slots of a point without observations are never written), rtd (12 C doubles: the
 * values of rt32 as pass B reads them).  Any output may be NULL.  Returns -1 when the problem does not run the mixed
 * form (sfmba_get_form(h, "mixed")).  Copies only: launches nothing and changes nothing on the handle. */
int  sfmba_get_mixed_operands(sfmba_handle* h, double* origin, float* rt32, float* rec32, double* rtd);

/* What the LAST outer iteration of the last sfmba_solve left on the handle, valid until the next operation that computes
 * on it.  A solve with max_nfev = 1 runs the linear phase and the device-decided trial of iteration 0 and returns x0, so
 * the state is that of one outer iteration at x0; max_nfev = 2 leaves iteration 1 (at the point the solve returns) when
 * the first step was accepted.  n = 6C + 3P.  Every output may be NULL; all are in the caller's layout:
 *   scalars (32)   the exchange scalars on the device: 0 sum r^2 of the last evaluated point, 1 G11, 2 G12, 3 G22,
 *                  4..7 q5..q8 and 8..11 q1..q4 of the point slice, 12 max|g_p|, 13 reg, 14 |g_h|^2 (the next forcing
 *                  term's memory), 15 eta, 16..24 q0..q8 of the camera slice, 25..29 c1, c2, predicted reduction, |step_h|,
 *                  |step| as the device decided them, 30 the skip flag, 31 the radius the device used
 *   ctrl (8)       the PCG control block the solve ended on: rz, rz0, tol2, rz_prev, alpha_prev, iters, max_iters, done
 *   si, g, sg      (n each) column scale, gradient and D^2 g of the point the solve returns
 *   si2, g2, sg2   (n each) the other buffer set: with "spec_scale", those of the last trial point
 *   Dc (6C), Minv (21C: upper triangles, the values the PCG read), Vinv (6P: upper triangles), e (3P)
 *   pcg_x, pcg_r   (6C each) iterate and residual the PCG ended on, from the vector set the control block names
 *   p (n)          the step [dc | dp];   x_new (n) the last trial point
 * An output the solve's form does not keep is refused: the call returns -1 and the message names the output.  Minv:
 * not on the dense path (its inverses live in LDS).  e: only on the dense path or with the 128-byte records ("rhsrec");
 * elsewhere pass A has overwritten it with its z.  pcg_r: not on the dense path and not in the local forms (their r
 * lags one update behind).  pcg_x: not when k_backsub's prologue did the last update (the final x is dc of p only).
 * Returns -1 without a completed solve.  Waits for the stream and copies: launches nothing and changes nothing on the
 * handle. */
int  sfmba_get_iteration_state(sfmba_handle* h, double* scalars, double* ctrl, double* si, double* g, double* sg,
                               double* si2, double* g2, double* sg2, double* Dc, double* Minv, double* Vinv, double* e,
                               double* pcg_x, double* pcg_r, double* p, double* x_new);

/* Few-camera path (6 n_cameras <= 128, the reference's own problem sizes): at x, with the diagonals dc (6C) and dp
 * (3P), form S = U + diag(dc) - W (V + diag(dp))^-1 W^T (S_out: (6C)^2 row-major, may be NULL) and solve S y = rhs
 * with the in-LDS PCG run to the end (relative tolerance 1e-14; sol_out: 6C). */
int  sfmba_dense_schur(sfmba_handle* h, const double* x, const double* dc, const double* dp, const double* rhs,
                       double* S_out, double* sol_out);

/* Host-only helper for the CPU test-suite (no GPU needed): the 2-D trust-region subproblem of
 * SCIPY/optimize/_lsq/common.py:171-219.  B3 = (B00, B01, B11), g2, Delta -> p2; returns 1 when the Newton step
 * lies inside the region, 0 for a boundary solution. */
int  sfmba_tr2d_solve(const double* B3, const double* g2, double Delta, double* p2);
/* Test / diagnostic hooks (nothing in the library reads the environment).  -1 (or 0 where noted) = the library's own
 * choice.  Placement options (P) take effect at the next sfmba_set_problem, the others at the next solve.
 *   "dense"          P  0: implicit Schur product + launched PCG although the reduced camera matrix would be formed
 *                       and solved inside one workgroup (6 n_cameras <= 128)
 *   "sweep_rc"       P  0: pass A of the Schur product reads the stored Jacobian instead of recomputing the blocks from
 *                       the camera table; 2: recomputes them from a table in GLOBAL memory (the form of > 1100 cameras)
 *                       whatever the camera count
 *   "tab_lds", "vec_lds" P  0: camera table / camera vector read from L2 although they would fit the LDS
 *   "pcg_fused"      P  0: the PCG update as a kernel of its own instead of the prologue of pass A
 *   "pcg_local"         0: the fused PCG keeps its whole update in pass A's prologue (no per-camera tail in pass B)
 *   "pcg_split"         1: the per-camera tail of the local form in a kernel of its own (k_pcg_tail) on one rank too;
 *                       0: sharded / multi-chunk solves keep the general prologue or k_pcg_update
 *   "precond"           0: block-Jacobi preconditioner from U + D instead of the Schur-diagonal blocks
 *   "cov_lds"           0: the point sweep of sfmba_covariance reads Sigma_cc from L2 instead of staging it in LDS
 *   "cam_chunk"      P  > 0: chunk length of the camera-major kernels (forces multi-chunk cameras + k_cam_combine)
 *   "xcd_chunks"     P  1 / 0: pass B's camera lists cut at the eight point-range boundaries (one piece per XCD) whatever
 *                       the problem size (default: from 250k points on)
 *   "rhsrec"         P  1 / 0: the rhs + preconditioner pass gathers dedicated 128-byte point records whatever the size
 *   "cost_rider"        0: the trial cost is summed and posted by a k_finish launch of its own instead of riding with
 *                       the normal-block launch
 *   "spec_scale"        0: k_update_scale (column scale, gradient, D^2 g and the partial sums of an accepted point) is
 *                       launched after the host has accepted the trial point (default on one rank: enqueued behind the
 *                       trial point's normal blocks before the verdict, into a second set of the three vectors which
 *                       is swapped in on acceptance; with several ranks always the 0 form)
 *   "start_handoff"     0: a solve starts with a blocking read-back of the cost and the scale sums, the camera table
 *                       and the point records as two launches (default on one rank: the cost is posted by the
 *                       normal-block launch and picked up behind the first k_jdot, the first radius is derived on the
 *                       device by k_prep / k_tr_step and read at the first hand-off; needs "cost_rider")
 *   "early_download"    0: the result is copied to the host behind the last launch of the solve (default: when a
 *                       solve ends on an accepted step, x leaves on the copy stream as soon as the host has accepted
 *                       it, beside the last kernels)
 *   "pcg_mixed"      P  1 / 0: fp32 operands with fp64 accumulation in the implicit Schur product (default: with fp32
 *                       storage, sfmba_set_precision); "pcg_mixed_b" 0: pass B keeps its fp64 point records
 *   "pcg_inline"        0: sharded solves over the direct link keep the all-reduces of the per-camera sums as launches
 *                       of their own (default: exchanged by the producing workgroups; ranks that SHARE one device --
 *                       rehearsals -- get 0 by themselves once their camera workgroups together exceed the device's
 *                       resident slots: settled at sfmba_p2p_attach)
 *   "xcd_cam"        P  0: K3 and the rhs + preconditioner pass keep one workgroup per camera where pass B takes the
 *                       XCD-aware chunk table ("xcd_chunks"; default from 250k points on: all three one wave per chunk)
 *   "pcg_skip_last"     0: the launches that a replayed record says find the PCG solve finished are enqueued all the
 *                       same; 2: only the pass B is left out (default: neither the last pass A -- k_backsub's prologue
 *                       does its update -- nor the pass B behind it is enqueued; both are owed if the record turns out
 *                       too short)
 *   "cm_device"      P  1 / 0: camera-major order sorted on the device / on the host (default: device from 64k
 *                       observations on); "packed_upload" P 1 / 0: observation arrays uploaded packed (same default)
 *   "jfree"          P  1: the J-free iteration (measurement): K1 does not write the Jacobian, k_jdot / k_backsub
 *                       recompute its blocks (needs the camera table in LDS)
 *   "rc_consumers"   P  0: k_jdot and k_backsub read the stored Jacobian; 1: their row form wherever it is legal, whatever the
 *                       size (default, -1: by the forms table -- the row form, which takes J (D^2 g) and J p from pass A's LDS
 *                       camera rows and the point instead of the stored blocks, from 65536 observations on, with 64-bit
 *                       storage, whenever pass A runs in its LDS row form)
 *   "pcg_guess_bias"    added to the number of speculatively enqueued PCG iterations (negative: force misses)
 *   "wait_deadline_s"   a hand-off not posted within this many seconds fails the solve with -3 (default 120)
 *   "p2p_delay_ms"      sleep before the first collective of a solve (late-peer test)
 *   "p2p_timeout_ms"    > 0: overrides both time-outs of the direct all-reduce (test)
 *   "trace_pcg", "trace_stalls", "trace_timing"   stderr diagnostics */
int  sfmba_debug_option(sfmba_handle* h, const char* name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* SFMBA_H */
