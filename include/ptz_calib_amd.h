/*
 * ptz_calib_amd.h -- C-ABI of libptzcalib_hip.so: the MI355X (gfx950) implementation of the PTZ-Calib
 * optimisation hot path (per-observation PTZ reprojection residual/Jacobian evaluation, Levenberg-
 * Marquardt normal-equation assembly, Schur elimination, dense reduced-camera solve, LM control) and of the match table's
 * per-pair RANSAC homographies.
 *
 * The reference (gjgjh/PTZ-Calib) has no FFI layer; its seam is the pair of C++ classes that each own
 * a ceres::Problem.  Every entry point below names the reference interface it replaces
 * (file:line relative to the reference tree).  Plain pointers and sizes only; no C++ or torch types.
 * All functions return 0 on success or a negative PTZ_E* code; no exceptions cross the boundary and
 * there is no CPU fallback: without a HIP device every compute entry point returns PTZ_ENODEVICE.
 *
 * Conventions
 *  - Camera = 15 doubles, layout of Camera::ToVector (src/core/types.cc:32-57):
 *      [fx, fy, cx, cy, r1, r2, r3, t1, t2, t3, k1, k2, k3, p1, p2]
 *  - pixels are float32 pairs (cv::Point2f; src/core/data_io.cc:40), everything else float64
 *  - observations are sorted (track id ascending, image id ascending), the order in which
 *    PTZRayOptimizer::AddConstraints2d2d adds residual blocks (src/core/ptzray_optimizer.cc:801-850)
 *  - "host" pointers are ordinary process memory; "dev" pointers are HIP device memory
 */
#ifndef PTZ_CALIB_AMD_H
#define PTZ_CALIB_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTZ_CAM_DIM 15

/* error codes */
#define PTZ_OK 0
#define PTZ_EINVAL (-1)     /* malformed problem (CheckValid, ptzray_optimizer.cc:515-535) */
#define PTZ_ENODEVICE (-2)  /* no usable HIP device / HIP runtime error */
#define PTZ_ENOMEM (-3)
#define PTZ_EUNSUPPORTED (-4) /* factor type not implemented on the device path */
#define PTZ_ELIMIT (-5)     /* a problem dimension beyond what the device path handles: more than 65535 observations in ONE view
                               (16-bit positions in the camera-pair records), more than 2^31 - 1 observations or pair entries in
                               one batch.  The number of views and tracks is bounded by device memory only (the reduced camera
                               system is stored as dense tiles: 8 (NC n_views + 64)^2 bytes per scene).  Never a silent failure:
                               the C++ classes report it on stderr and return false. */
#define PTZ_ENOOBS (-6)     /* ptz_ba_batch_create_views: a view none of whose tracks has a candidate observation -- no residual block, not a problem
                               (the reference's Solve returns false there, ptzray_optimizer.cc:517); every other malformed view is PTZ_EINVAL */
#define PTZ_EINTERNAL (-7)  /* a bounded device loop reached its step cap (ptz_tracks_*): a bug in the library, reported and never waited for */

/* enum FACTOR_TYPE { PTZRay, PTZRayDist, PTZRayFxfyDist, PTZRayDistDisp }  (ptzray_optimizer.h:110) */
#define PTZ_BA_PTZRay 0
#define PTZ_BA_PTZRayDist 1
#define PTZ_BA_PTZRayFxfyDist 2 /* fx, fy, k1 free (ptzray_optimizer.cc:136-191); camera block of 6 columns */
#define PTZ_BA_PTZRayDistDisp 3 /* fx, k1 free + ONE 3-parameter displacement block shared by every residual of the problem
                                 * (ptzray_optimizer.cc:195-265, disp_param_ :655; with annotations Reproj2d3dDispFactor :334-396);
                                 * CLOSED-FORM JACOBIANS ONLY, a documented deviation (type 3 is dead from the reference's tools): the
                                 * reference differentiates the d2 column numerically with delta = 1.49e-8 against f^2 ~ 6e6, so ITS
                                 * column is a per cent off and its trajectory follows that through the flat valley of (f, k1, disp);
                                 * this library converges to the closed-form oracle's point (1e-6) and may stop up to 8 % in f from the
                                 * numeric-differentiation reference at equal cost (tests/test_gpu_disp.py holds the number) */
/* KRTOptimizer::FACTOR_TYPE { F, FDist, Fxfy, FxfyDist }  (krt_optimizer.h:110) */
#define PTZ_KRT_F 0
#define PTZ_KRT_FDist 1
#define PTZ_KRT_Fxfy 2      /* fy free as well: Factor2d2dFxfy (krt_optimizer.cc:52-71), dead from the reference's tools */
#define PTZ_KRT_FxfyDist 3  /* Factor2d2dFxfyDist (krt_optimizer.cc:141-192) */
/* ceres::TerminationType as read by the reference (ptzray_optimizer.cc:482, krt_optimizer.cc:513) */
#define PTZ_CONVERGENCE 0
#define PTZ_NO_CONVERGENCE 1
#define PTZ_FAILURE 2

/* Solver options.  The reference sets max_num_iterations, linear_solver_type, num_threads only
 * (ptzray_optimizer.cc:469-473, krt_optimizer.cc:387-391); every other field is the Ceres 1.14
 * default and is exposed so that the defaults are data, not code. */
typedef struct ptz_lm_options {
  int32_t max_num_iterations;                /* 200 (run_ptz_ba.cc:52) / 100 (ptz_incremental_optimizer.cc:396) */
  int32_t device_id;                         /* HIP device ordinal */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  int32_t jacobi_scaling;                    /* 1 */
  double initial_trust_region_radius;        /* 1e4 */
  double max_trust_region_radius;            /* 1e16 */
  double min_trust_region_radius;            /* 1e-32 */
  double min_relative_decrease;              /* 1e-3 */
  double min_lm_diagonal;                    /* 1e-6 */
  double max_lm_diagonal;                    /* 1e32 */
  double function_tolerance;                 /* 1e-6 */
  double gradient_tolerance;                 /* 1e-10 */
  double parameter_tolerance;                /* 1e-8 */
  /* ptz_krt_solve_batch*: lanes of a wavefront that work on one query.  64 = a wave per query (lowest latency: registration
   * attempts, a handful of queries); 16 = four queries per wave (highest throughput once the launch fills the GPU); 0 = the
   * library picks from the launch size (16 from 16384 queries on).  The two forms add the matches up in different orders: a
   * query's bits depend on the form, never on its neighbours in the launch -- callers that compare runs bit by bit pin it. */
  int32_t krt_lanes_per_query;               /* 0 */
  int32_t reserved_;                         /* 0 */
} ptz_lm_options;

/* The ceres::Solver::Summary fields the reference reads (ptzray_optimizer.cc:962-963,482;
 * krt_optimizer.cc:396,506-513) plus iteration bookkeeping. */
typedef struct ptz_lm_summary {
  int32_t termination_type;     /* PTZ_CONVERGENCE / PTZ_NO_CONVERGENCE / PTZ_FAILURE */
  int32_t num_iterations;       /* summary.iterations.size() - 1 */
  int32_t num_lm_steps;         /* trust-region loop passes executed (includes the terminating pass) */
  int32_t num_successful_steps; /* iteration 0 counts as successful (Ceres 2.x convention; whether 1.14 did is unverified here --
                                   the reference only stores the value in KRTOptimizer::num_iter_, krt_optimizer.cc:396, and never reads it) */
  int32_t num_unsuccessful_steps;
  int32_t num_residuals;        /* scalar residuals */
  int32_t num_linear_solves;
  int32_t num_jacobian_evals;
  double initial_cost;
  double final_cost;
  double final_radius;
  double final_gradient_max_norm;
} ptz_lm_summary;

void ptz_lm_options_default(ptz_lm_options* o);

/* Library / device probe.  ptz_device_count() never initialises a GPU context beyond counting. */
const char* ptz_version(void);
int32_t ptz_device_count(void);
/* The reference builds a new optimizer object per solve; so do callers of this library.  Device blocks, pinned blocks,
 * streams and events released by finished solves are parked in a process-wide cache (budget PTZ_CACHE_MAX_MB of device
 * memory per GPU, default 32768) and reused by later ones.  ptz_trim_cache() hands everything parked back to the driver. */
void ptz_trim_cache(void);

/* ------------------------------------------------------------------------------------------------
 * PTZ-IBA global bundle adjustment
 *   replaces PTZRayOptimizer::Solve (ptzray_optimizer.cc:454-489) from AddConstraints2d2d onwards:
 *   residual blocks, SubsetParameterization masks, ScaledLoss weights, ceres::Solve(SPARSE_SCHUR).
 * One problem = one scene's candidate cameras + tracks, in packed form.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ptz_ba_problem {
  int32_t n_cam;             /* candidate cameras (compact ids 0..n_cam-1) */
  int32_t n_ray;             /* tracks with >= 1 candidate observation */
  int64_t n_obs;             /* 2D-2D observations */
  const float* obs_uv;       /* host [2*n_obs] */
  const int32_t* obs_cam;    /* host [n_obs] */
  const int32_t* obs_ray;    /* host [n_obs] non-decreasing */
  const double* ray_weight;  /* host [n_ray]: ScaledLoss weight = full track length (ptzray_optimizer.cc:805) */
  int32_t n_obs3d;           /* 2D-3D annotation observations (ptzray_optimizer.cc:887-923); 0 = none */
  const float* obs3d_uv;     /* host [2*n_obs3d] */
  const double* obs3d_xyz;   /* host [3*n_obs3d] */
  const int32_t* obs3d_cam;  /* host [n_obs3d] */
  int32_t factor_type;       /* PTZ_BA_* */
  /* PTZRayOptimizer::SetSharedIntrinsics (ptzray_optimizer.cc:497-505): cameras with equal ids share ONE intrinsics block
   * (fx, fy, cx, cy, k1..p2); its initial value is the first such camera's (:645-650).  NULL = every camera its own block,
   * the reference's default (:427-428). */
  const int32_t* ic_of_cam;  /* host [n_cam] or NULL */
} ptz_ba_problem;

typedef struct ptz_ba_batch ptz_ba_batch; /* opaque: device-resident problems + workspaces */

/* Build a device-resident batch of n independent problems (all with the same factor_type).  Uploads
 * the observation records, builds the structural indices (per-camera observation lists, camera-pair
 * lists for the Schur complement) and allocates every workspace, so that ptz_ba_batch_solve performs
 * no allocation.  The problem arrays may be released after this call returns. */
int32_t ptz_ba_batch_create(int32_t n, const ptz_ba_problem* problems, const ptz_lm_options* opt, ptz_ba_batch** out);
void ptz_ba_batch_destroy(ptz_ba_batch* b);

/* Initial point.  cam: host [15 * sum(n_cam)], ray: host [3 * sum(n_ray)], tlw: host [6 * n] (may be
 * NULL = zeros), each concatenated over the problems in order
 * (SetUpInitialCameraParams, ptzray_optimizer.cc:635-670). */
int32_t ptz_ba_batch_set_state(ptz_ba_batch* b, const double* cam, const double* ray, const double* tlw);
/* Run LM on every problem of the batch from the state last set (the state set by
 * ptz_ba_batch_set_state is kept, so repeated calls re-solve from the same initial point).
 * Device work is enqueued on the batch's stream; the call returns after the stream has drained.
 * summaries: host [n]. */
int32_t ptz_ba_batch_solve(ptz_ba_batch* b, ptz_lm_summary* summaries);
/* Solution = parameters at the minimum-cost point, as Ceres writes back (any termination type). */
int32_t ptz_ba_batch_get_state(ptz_ba_batch* b, double* cam, double* ray, double* tlw);
/* PTZRayDistDisp only (else PTZ_EUNSUPPORTED): the displacement block of every problem, disp [3 * n]: (d0, d1, d2) of
 * delta_z = d0 + d1 fx + d2 fx^2.  The initial value is zero (disp_param_ = {0, 0, 0}, ptzray_optimizer.cc:655) unless set;
 * get returns the block at the minimum-cost point like ptz_ba_batch_get_state (the reference adds it to t_z, :693, :714). */
int32_t ptz_ba_batch_set_disp(ptz_ba_batch* b, const double* disp);
int32_t ptz_ba_batch_get_disp(ptz_ba_batch* b, double* disp);
/* Device time of the last ptz_ba_batch_solve in milliseconds (HIP events on the batch's stream),
 * and, per kernel family, the accumulated device time and launch count when profiling was enabled
 * with ptz_ba_batch_set_profiling(b, 1) (serialises the stream between kernels and runs the batch as ONE scene group,
 * so that no other group's kernels share the device while a family is being timed). */
int32_t ptz_ba_batch_last_solve_ms(const ptz_ba_batch* b, double* ms);
int32_t ptz_ba_batch_set_profiling(ptz_ba_batch* b, int32_t enable);
#define PTZ_PROF_SLOTS 16
int32_t ptz_ba_batch_get_profile(const ptz_ba_batch* b, double* ms_per_slot, int64_t* launches_per_slot,
                                 const char** slot_names);

/* One-shot convenience: create + set_state + solve + get_state + destroy for a single problem.
 * cam/ray/tlw are updated in place. */
int32_t ptz_ba_solve(const ptz_ba_problem* p, double* cam, double* ray, double* tlw, const ptz_lm_options* opt,
                     ptz_lm_summary* summary);
/* The same for PTZRayDistDisp: disp [3] initial value in (NULL: zeros), refined value out.  cam[9] (t_z) is returned as the
 * parameter block holds it; the reference's read-back also adds d0 + d1 fx + d2 fx^2 to it (ptzray_optimizer.cc:693, 714):
 * that last step is the caller's (the C++ class PTZRayOptimizer and api.fold_displacement do it). */
int32_t ptz_ba_solve_disp(const ptz_ba_problem* p, double* cam, double* ray, double* tlw, double* disp,
                          const ptz_lm_options* opt, ptz_lm_summary* summary);

/* Kernel-level entry points used by the parity tests (one linearisation at the current state of
 * problem `index`; weighted by sqrt(track length), not Jacobi-scaled).  Host outputs, any may be NULL:
 *   cost; g_c [nc*n_cam], U [nc*nc*n_cam]; g_r [3*n_ray], V [9*n_ray]; W [nw*3*n_obs]
 * where nw = ptz_ba_cam_block_dim(factor_type), nc = ptz_ba_batch_cam_block_dim(batch): the free camera parameters carried on the device
 * ([fx, r1, r2, r3] for PTZRay, [fx, k1, r1, r2, r3] for PTZRayDist, [fx, fy, k1, r1, r2, r3] for PTZRayFxfyDist,
 * [fx, k1, r1, r2, r3, d0, d1, d2] for PTZRayDistDisp -- every camera carries its copy of the displacement block, the
 * copies are one parameter; the reference's always-zero fy column (ptzray_optimizer.cc:24-25) is not materialised). */
int32_t ptz_ba_cam_block_dim(int32_t factor_type);
/* ... and of a batch: one more (fy, live through Reproj2d3dFactor, ptzray_optimizer.cc:273) when any problem of the
 * batch carries 2D-3D annotation observations: [fx, fy, (k1), r1, r2, r3]; the reduced system then also holds the
 * 6-dof T_l_w block (ptzray_optimizer.cc:909-910). */
int32_t ptz_ba_batch_cam_block_dim(const ptz_ba_batch* b);
int32_t ptz_ba_batch_linearize(ptz_ba_batch* b, int32_t index, double* cost, double* g_c, double* U, double* g_r,
                               double* V, double* W);
/* Pix2Ray ray initialisation (ptzray_optimizer.cc:768-797) on the device for the whole batch:
 * overwrites the ray part of the stored initial state from the stored cameras. */
int32_t ptz_ba_batch_pix2ray(ptz_ba_batch* b);

/* n independent problems over the devices device_ids[0 .. n_devices) of one node, from one process: scenes are dealt
 * longest-first to the least loaded device, one host thread per device creates / solves / reads back its own batch
 * (replaces the sequential scene loops of the reference's scripts, run_ptzba_synthetic.sh:4-13, run_ptzba_worldcup14.sh).
 * cam [15 * sum n_cam], ray [3 * sum n_ray], tlw [6 * n] or NULL: in = initial values, out = solutions, all in problem
 * order; summaries [n] or NULL.  opt->device_id is ignored.  No collective is involved: the scenes never interact. */
int32_t ptz_ba_solve_sharded(int32_t n, const ptz_ba_problem* problems, double* cam, double* ray, double* tlw,
                             const int32_t* device_ids, int32_t n_devices, const ptz_lm_options* opt, ptz_lm_summary* summaries);

/* ------------------------------------------------------------------------------------------------
 * Rig-resident tracks: bundle adjustments over candidate SUBSETS of one rig without rebuilding the problem on the host
 *   PTZ-IBA adjusts a growing subset of one rig's images ~2N times (AdjustGlobalBundle after every ~10 % of new registrations,
 *   src/core/ptz_incremental_optimizer.cc:91, 420-440), and the reference re-walks the match table into a fresh
 *   PTZRayOptimizer each time (ptzray_optimizer.cc:537-552, 799-850).  Here the rig's tracks (TracksBuilder output after
 *   Filter(4), tracks.cc:19-113) are uploaded ONCE; a bundle adjustment is then a VIEW of them -- the ascending list of candidate
 *   images -- and the packed problem AddConstraints2d2d would produce for that candidate set (observations in (track, image)
 *   order, full-track weights :805, the library's internal ray order, camera-major lists, camera pairs) is built ON THE DEVICE,
 *   word for word the arrays ptz_ba_batch_create builds from the host-packed problem: same batch, same bits.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ptz_rig ptz_rig; /* opaque: one rig's tracks, resident in HBM */
/* trk_ptr [n_track + 1] offsets into the view arrays; per view of a track (image ids ascending inside a track, the order of
 * the reference's map of maps): trk_img [n_view] image id in [0, n_img), trk_uv [2 * n_view] the keypoint's pixel (cv::Point2f). */
int32_t ptz_rig_create(int32_t n_img, int32_t n_track, const int64_t* trk_ptr, const int32_t* trk_img, const float* trk_uv,
                       int32_t device_id, ptz_rig** out);
void ptz_rig_destroy(ptz_rig* rig);
typedef struct ptz_rig_view {
  const ptz_rig* rig;
  int32_t n_cam;             /* candidate images */
  const int32_t* cam_image;  /* host [n_cam] image ids, ascending: compact camera c is image cam_image[c] (SetUpInitialCameraParams' order) */
} ptz_rig_view;
/* The batch ptz_ba_batch_create would build from the n packed problems of these views (2D-2D residuals only, no shared
 * intrinsics): tracks without a candidate view are not rays of the problem; a view without any candidate observation is
 * PTZ_EINVAL.  Ray i of problem k, for set/get_state, is the i-th track of the rig (ascending) that has a candidate view. */
int32_t ptz_ba_batch_create_views(int32_t n, const ptz_rig_view* views, int32_t factor_type, const ptz_lm_options* opt,
                                  ptz_ba_batch** out);
/* Initial state of a batch: cameras cam [15 * sum n_cam] and, computed ON THE DEVICE, the rays by Pix2Ray
 * (ptzray_optimizer.cc:768-797): ray = normalise(mean over the candidate views of normalise(R^-1 K^-1 [u, v, 1])), with the
 * per-camera matrices rkinv [9 * sum n_cam] = R^-1 K^-1 as the caller's (reference's) matrix code evaluates them -- the same
 * operations in the same order as a host loop over the track's views, without contraction: the same bits.  T_l_w = 0. */
int32_t ptz_ba_batch_set_state_pix2ray(ptz_ba_batch* b, const double* cam, const double* rkinv);
/* Diagnostic for the tests: FNV-1a hash over the batch's structure arrays (observations in the library's order, ray and
 * camera lists, camera pairs, entries, runs, weights, ray order), real extents only -- two batches that hash alike solve alike. */
int32_t ptz_debug_batch_structure_hash(ptz_ba_batch* b, uint64_t* hash);
/* ... and the stored initial rays of the batch in the caller's ray numbering, ray [3 * sum n_ray] (at the extents the batch was
 * created with), e.g. what ptz_ba_batch_set_state_pix2ray computed. */
int32_t ptz_debug_batch_initial_rays(ptz_ba_batch* b, double* ray);

/* Dense SPD solve used for the reduced camera system, exposed for parity tests and micro-benchmarks:
 * solves A x = rhs for `count` independent n x n systems (host, row-major, lower triangle read).
 * Returns per-system status in fail[count] (1 = not positive definite). */
int32_t ptz_chol_solve_batch(int32_t count, int32_t n, const double* A, const double* rhs, double* x, int32_t* fail,
                             int32_t device_id, double* device_ms);
/* Diagnostic for the tests of the factorisation kernels: the same solve with the launch path chosen by the caller and one
 * order per system.  A [count][ld][ld] and rhs / x [count][ld] hold system i in their leading n[i] rows and columns
 * (ld >= max n; only the lower triangle of A is read).  path: 0 what ptz_chol_solve_batch would take, 1 the one-launch
 * chain (count <= 32), 2 one launch per step, 3 right-looking panel + trailing update, 4 left-looking column update +
 * panel (the path of a large bundle-adjustment batch).  flags bit 0: the device buffers the kernels write before they read
 * (factored diagonal tiles, block and tile inverses, the solution) start as 0xFF bytes instead of whatever the allocation
 * held.  active (may be NULL): systems with active[i] == 0 are skipped, x[i] and fail[i] stay as passed.  fail[i]: 1 = not
 * positive definite.  PTZ_EINVAL, with nothing launched: count <= 0, an n[i] <= 0, ld < max n, path outside 0..4, path 1 with
 * more than 32 systems. */
int32_t ptz_debug_chol_solve(int32_t count, const int32_t* n, int32_t ld, const double* A, const double* rhs, double* x,
                             int32_t* fail, const int32_t* active, int32_t path, int32_t flags, int32_t device_id);

/* Diagnostic for the tests of the Schur kernels (k_ray_prep, k_schur_f / k_schur / k_schur_w): the damped reduced camera system
 * S y = b of the FIRST LM step of problem `index`, as the solver's own launches leave it.  The call runs the solver's prologue
 * (state and LM reset, linearisation, control words, the step opened) and its first pass up to and including the system's
 * construction, through the code the solver runs, in the full-size launch shape -- with the caller's Jacobi scales in place of the
 * column norms: scale_c [n_cam][NC], scale_r [n_ray][3] in the caller's ray order, of problem `index` (NULL: 1.0; the other
 * problems of the batch always get 1.0).  flags bit 0: the problem's block of the padded system starts as 0xFF bytes, so a tile
 * that is read without having been cleared shows as NaN.  Outputs, in the cameras' numbering (camera i: rows i NC ..), the
 * elimination order undone, tiles outside the structure reported as zero, the lower triangle mirrored: S [n][n], n = NC n_cam;
 * rhs [n] = g_c - sum W E g_r; diag_c [n_cam][NC] (may be NULL) the clamped diagonal the LM term is made of; info [8] (may be NULL):
 * kernel (0 k_schur_w, 1 k_schur, 2 k_schur_f), table in global memory, order np of the padded system, its 64-column tiles,
 * 1 if the problem's elimination order is not the identity, the batch's largest observation count and run count of one camera,
 * threads of the Schur workgroup.  The batch's state is left mid-step: a later solve starts over from the stored initial state.
 * PTZ_EUNSUPPORTED: PTZRayDistDisp, annotations, shared intrinsics.  PTZ_EINVAL: no state, index out of range, NULL S / rhs, or
 * a problem that ends at iteration zero (no step is opened). */
int32_t ptz_debug_batch_reduced_system(ptz_ba_batch* b, int32_t index, const double* scale_c, const double* scale_r, int32_t flags,
                                       double* S, double* rhs, double* diag_c, int32_t* info);

/* Measured FP64 matrix-core rate of the device (v_mfma_f64_16x16x4_f64 from registers, every wave slot busy): the
 * number the reduced-camera solve is priced against in the roofline reports. */
int32_t ptz_mfma_f64_peak(int32_t device_id, double* tflops);
/* Host logic only (no device needed; used by the CPU tests): the elimination order ptz_ba_batch_create would give a reduced
 * camera system of nt 64-column tiles whose lower-triangular tile adjacency is mask[nt*nt] (row-major, non-zero = coupled),
 * tiles >= first_dense kept last.  perm[t] = position of tile t; lanes[0], lanes[1] = tiles of the two lanes that are
 * factored side by side (positions [0, lanes[0]) and [lanes[0], lanes[0] + lanes[1])).  sched (may be NULL): [nt * 4] the
 * block columns (positions, -1 = none) each step of the factorisation handles, n_steps[0] their number -- read off the filled
 * structure for a dissected order, one column per step otherwise.  Returns 1 if a dissection was chosen, 0 for the natural
 * order (perm = identity). */
int32_t ptz_ba_plan_tile_order(int32_t nt, int32_t first_dense, const uint8_t* mask, int32_t* perm, int32_t* lanes,
                               int32_t* sched, int32_t* n_steps);

/* Measured HBM rates of the device in GB/s: streaming read of 4 GB, and copy of 4 GB counted as read + write. */
int32_t ptz_hbm_bandwidth(int32_t device_id, double* read_gbps, double* copy_gbps);

/* ------------------------------------------------------------------------------------------------
 * Single-view LM, batched over queries
 *   replaces KRTOptimizer::Add2d2dConstraints + Solve (krt_optimizer.cc:265-348, 385-404), the loop
 *   body of run_ptz_reloc.cc:68-118 and RegisterNextImage (ptz_incremental_optimizer.cc:377-418).
 * Query q owns matches [match_ptr[q], match_ptr[q+1]).  cam_ref: reference camera (world frame),
 * cam_cur: in = initial current camera in world frame (SetInitParams), out = refined camera in world
 * frame (ObtainRefinedCameraParams, krt_optimizer.cc:535-567), written only when accepted[q] = 1
 * (CheckResults, krt_optimizer.cc:504-533, with max_reproj_error).
 * ------------------------------------------------------------------------------------------------ */
int32_t ptz_krt_solve_batch(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                            const double* cam_ref, double* cam_cur, int32_t factor_type, double max_reproj_error,
                            const ptz_lm_options* opt, ptz_lm_summary* summaries, int32_t* accepted,
                            double* device_ms);

/* The same solve with 2D-3D constraints added to every query:
 *   replaces KRTOptimizer::Add2d3dConstraints (krt_optimizer.cc:350-383; Factor2d3dDist / Factor2d3dFxfyDist,
 *   :200-249) on top of Add2d2dConstraints -- never called by the reference's tools.
 * Query q owns points [point_ptr[q], point_ptr[q+1]): pts2d = pixels (2 x f32), pts3d = WORLD points (3 x f64); the
 * library moves them into the local frame of the query's reference camera as the reference does (:357-362) and
 * projects them as cv::projectPoints does, including its (k1,k2,p1,p2,k3) reading of the stored distortion.
 * num_residuals counts both kinds.  point_ptr = NULL is ptz_krt_solve_batch. */
int32_t ptz_krt_solve_batch_2d3d(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                 const int64_t* point_ptr, const float* pts2d, const double* pts3d, const double* cam_ref,
                                 double* cam_cur, int32_t factor_type, double max_reproj_error, const ptz_lm_options* opt,
                                 ptz_lm_summary* summaries, int32_t* accepted, double* device_ms);

/* The same launch on queries that are already resident in HBM (matches produced on the device, a serving loop that keeps its
 * buffers): every d_* argument is a DEVICE pointer with the layout of its host counterpart above, d_point_ptr = NULL for no
 * 2D-3D constraints.  The kernel is enqueued on `hip_stream` (a hipStream_t; NULL = the default stream) of the device that
 * OWNS d_cam_cur (hipPointerGetAttributes) and the call returns without synchronising: results (d_cam_cur, d_summaries,
 * d_accepted) are valid once the stream has passed this point.  PTZ_EINVAL if the stream belongs to another device than the
 * buffers, or if opt->device_id names a different device explicitly (a non-zero value; 0 is the untouched default and is
 * not taken as a request for device 0).  The CSR offsets are not validated (they live on the device).
 * Like every entry point of this library the call leaves the calling thread's current HIP device as it found it. */
int32_t ptz_krt_solve_batch_device(int32_t n_query, const int64_t* d_match_ptr, const float* d_uv_ref, const float* d_uv_cur,
                                   const int64_t* d_point_ptr, const float* d_pts2d, const double* d_pts3d,
                                   const double* d_cam_ref, double* d_cam_cur, int32_t factor_type, double max_reproj_error,
                                   const ptz_lm_options* opt, ptz_lm_summary* d_summaries, int32_t* d_accepted, void* hip_stream);

/* Registration attempts over match tables that stay on the device:
 *   replaces the loop body of PtzIncrementalOptimizer::RegisterNextImage (ptz_incremental_optimizer.cc:377-418) -- one
 *   KRTOptimizer per table entry (registered image i -> image j) -- for callers that try many entries of the SAME tables again
 *   and again while only the cameras change (the incremental pipeline: ~5 000 attempts per 200-view rig over ~8 500 entries).
 * ptz_krt_table_create copies a table's matches to device `device_id` once: entry e owns matches [match_ptr[e], match_ptr[e+1])
 * (match_ptr[0] = 0), uv_ref / uv_cur as in ptz_krt_solve_batch.  ptz_krt_solve_attempts then solves query q = entry
 * attempts[q].entry of attempts[q].table with the cameras cam_ref / cam_cur [15 n_query] (in / out as in ptz_krt_solve_batch); the
 * tables of one call may differ (several rigs in one launch) but live on one device, where the launch runs (opt->device_id, if
 * non-zero, must name it).  Results are bit-identical to ptz_krt_solve_batch on the same matches. */
typedef struct ptz_krt_table ptz_krt_table;
typedef struct ptz_krt_attempt { const ptz_krt_table* table; int32_t entry; } ptz_krt_attempt;
int32_t ptz_krt_table_create(int32_t n_entry, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur, int32_t device_id,
                             ptz_krt_table** out);
void ptz_krt_table_destroy(ptz_krt_table* table);
int32_t ptz_krt_solve_attempts(int32_t n_query, const ptz_krt_attempt* attempts, const double* cam_ref, double* cam_cur,
                               int32_t factor_type, double max_reproj_error, const ptz_lm_options* opt, ptz_lm_summary* summaries,
                               int32_t* accepted, double* device_ms);

/* The queries over the devices device_ids[0 .. n_devices) of one node, from one process: contiguous chunks of about equal
 * total match count, one host thread per device, results written into the caller's arrays in query order.  Host pointers
 * as in ptz_krt_solve_batch_2d3d (point_ptr = NULL: no 2D-3D constraints); opt->device_id is ignored. */
int32_t ptz_krt_solve_batch_sharded(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                    const int64_t* point_ptr, const float* pts2d, const double* pts3d, const double* cam_ref,
                                    double* cam_cur, int32_t factor_type, double max_reproj_error, const int32_t* device_ids,
                                    int32_t n_devices, const ptz_lm_options* opt, ptz_lm_summary* summaries, int32_t* accepted);

/* ------------------------------------------------------------------------------------------------
 * Pair homographies of a match table (RANSAC, batched over pairs)
 * ------------------------------------------------------------------------------------------------ */
/* replaces cv::findHomography(pts_i, pts_j, RANSAC, thresh) per pair of LoadMatchesInfo (data_io.cc:340-355, 384-385);
 * pair p owns [match_ptr[p], match_ptr[p+1]), dst ~ H src; bit-identical to the host estimator (host/homography.cc).
 * src_uv / dst_uv: float pairs [2 match_ptr[n_pair]].  found[p] = 1: H[9p .. 9p+9) row-major with h33 = 1 and, if inlier_mask
 * is non-NULL, one byte per match of the pair; found[p] = 0 (fewer than 4 matches, no model with 4 inliers): that pair's H and
 * mask bytes are left untouched.  PTZ_EINVAL (checked before any device work): n_pair < 0, match_ptr[0] != 0, decreasing
 * offsets, NULL arrays with non-zero extents, a threshold that is not finite and positive; PTZ_ELIMIT: a pair of more than
 * 2^31 - 1 matches.  n_pair = 0 is PTZ_OK.  Pairs of any size run on the device; no CPU fallback. */
int32_t ptz_homography_ransac_batch(int32_t n_pair, const int64_t* match_ptr, const float* src_uv, const float* dst_uv,
                                    double ransac_thresh, int32_t device_id, double* H /* [9 n_pair] */,
                                    int32_t* found /* [n_pair] */, uint8_t* inlier_mask /* [match_ptr[n_pair]] or NULL */,
                                    double* device_ms);
/* Host logic only (no device): the estimator's adaptive iteration bound for cnt = 0 .. n inliers of n matches, bound[n + 1] --
 * static_cast<int>(ceil(need)) of the host's libm, INT32_MIN where need exceeds the int range.  The kernel reads this table. */
int32_t ptz_debug_homography_bounds(int32_t n, int32_t* bound);

/* ------------------------------------------------------------------------------------------------
 * RANSAC inlier gating of matches
 * ------------------------------------------------------------------------------------------------ */
/* puts to use what the reference drops: the mask cv::findHomography returns in LoadMatchesInfo (`matches_msk`,
 * data_io.cc:351-352, never read) -- every listed match, wrong ones included, goes into a squared-loss LM there.
 * GATING a CSR match set (match_ptr, uv_a, uv_b) with a threshold and min_inliers: the pair estimator of
 * ptz_homography_ransac_batch runs with src = uv_a, dst = uv_b; pair p PASSES when found[p] = 1 and its mask has at least
 * max(min_inliers, 4) ones; a passing pair keeps exactly its matches with mask byte 1, in their order; every other pair keeps
 * none.  Integers and copies only: H, found and mask are the estimator's bits, the compacted CSR is what
 * keep = mask & passes[pair_of_match] selects.
 *
 * ptz_match_gate owns what a launch on DEVICE-RESIDENT offsets needs: the adaptive-bound table of every pair size
 * 5 .. max_pair_matches (about max^2 / 2 int32, computed once by host code with the host's libm; PTZ_ELIMIT above 4096, and
 * for max_matches beyond 2^31 - 1) and the estimator's workspace for max_matches matches.  PTZ_EINVAL: out = NULL,
 * max_pairs <= 0, a negative extent or device_id -- all checked before any device work.
 * ptz_match_gate_run_device: every d_* is a DEVICE pointer on the gate's device; d_match_ptr [n_pair + 1], d_uv_a / d_uv_b float
 * pairs; outputs d_found [n_pair], d_H [9 n_pair] or NULL, d_mask [n_match] or NULL, d_out_ptr [n_pair + 1], d_out_uv_a /
 * d_out_uv_b with room for n_match float pairs, d_out_index (the kept match's index in the input arrays) likewise or NULL.
 * Five kernels are enqueued on `hip_stream` (NULL = the default stream; it must belong to the gate's device) and the call
 * returns without synchronising; the outputs feed ptz_krt_solve_batch_device on the same stream as they are.  A pair with more
 * than max_pair_matches matches, or with a range outside [0, max_matches], is not served: found[p] = -1, an empty output
 * range, nothing else written for it, and the estimator does not run on it.  d_H and the d_mask bytes of a pair whose found
 * is not 1 are left as they were.  A pair's bits do not depend on the other pairs of the launch.  Runs on one gate are ordered
 * by the caller (one stream, or events): they share its workspace.  PTZ_EINVAL: NULL gate / required arrays, n_pair < 0, a
 * threshold that is not finite and positive, min_inliers < 0, a stream of another device; PTZ_ELIMIT: n_pair > max_pairs. */
typedef struct ptz_match_gate ptz_match_gate;
int32_t ptz_match_gate_create(int32_t max_pairs, int64_t max_matches, int32_t max_pair_matches, int32_t device_id,
                              ptz_match_gate** out);
void ptz_match_gate_destroy(ptz_match_gate* g);
int32_t ptz_match_gate_run_device(ptz_match_gate* g, int32_t n_pair, const int64_t* d_match_ptr, const float* d_uv_a,
                                  const float* d_uv_b, double ransac_thresh, int32_t min_inliers, double* d_H, int32_t* d_found,
                                  uint8_t* d_mask, int64_t* d_out_ptr, float* d_out_uv_a, float* d_out_uv_b, int32_t* d_out_index,
                                  void* hip_stream);
/* The same run on HOST arrays (callers without device buffers of their own): upload, ptz_match_gate_run_device, download.
 * out_uv_a / out_uv_b / out_index need room for match_ptr[n_pair] entries; H and mask of a pair whose found is not 1 are left
 * untouched.  The argument list of ptz_homography_ransac_batch applies, plus min_inliers < 0 (PTZ_EINVAL) and a set larger
 * than the gate (PTZ_ELIMIT). */
int32_t ptz_match_gate_run(ptz_match_gate* g, int32_t n_pair, const int64_t* match_ptr, const float* uv_a, const float* uv_b,
                           double ransac_thresh, int32_t min_inliers, double* H /* or NULL */, int32_t* found,
                           uint8_t* mask /* or NULL */, int64_t* out_ptr, float* out_uv_a, float* out_uv_b,
                           int32_t* out_index /* or NULL */, double* device_ms);

/* The rotation-and-focal gate: the same gating for ASSEMBLED relocalization queries, under the model such a query obeys.  uv_a of
 * query p is a pixel of the pinhole cam_ref[15 p] = [fx, fy, cx, cy, ..] at the rig's centre (the anchor, or the virtual anchor of
 * ptz_reloc_assemble / ptz_landmark_assemble; only these four entries are read), uv_b a pixel of the query, whose centre is
 * (cam_cur[15 p + 2], cam_cur[15 p + 3]); the two are related by K_q R K_a^-1 with unknown f and R, which two matches fix in closed
 * form.  `iters` two-match samples (1 .. 4096, 128 is the default of every caller here) give up to 2 iters hypotheses; the one with
 * the most inliers at `thresh` pixels wins, ties to the lowest number.  The contract -- sampling, the closed form, the order of every
 * operation -- is csrc/ptz_rotfocal.h, and the outputs are its bits whatever the batch and the launch shape.  No adaptive bound, no
 * table, no per-query size limit (2^31 - 1 matches), no refinement: the solve consumes the mask.  The query's distortion and
 * fx != fy do not enter the model; the threshold absorbs them.
 * Outputs: d_found [n_pair] (1: a model with at least 3 inliers; 0: none; -1: a range outside [0, max_matches], nothing else is
 * written for it), d_model [10 n_pair] or NULL (f, R row-major), d_H [9 n_pair] or NULL (K_q R K_a^-1 divided by its last entry;
 * nine NaN where that entry's magnitude is not above 1e-300 -- what the guided matcher takes for "no admissible candidate"),
 * d_mask [n_match] or NULL; model, H and mask bytes of a query whose found is not 1 are left as they were.  The compacted CSR
 * (d_out_ptr, d_out_uv_a, d_out_uv_b, d_out_index or NULL) is ptz_match_gate_run_device's, by the same rule: a query passes with
 * found = 1 and at least max(min_inliers, 4) mask ones.  Four kernels on `hip_stream`, no synchronisation.  The gate holds workspace
 * only.  PTZ_EINVAL, before any device work: NULL gate / required arrays, negative extents, max_pairs <= 0, a threshold that is not
 * finite and positive, min_inliers < 0, iters outside 1 .. 4096, a stream of another device; PTZ_ELIMIT: n_pair > max_pairs,
 * max_matches beyond 2^31 - 1; n_pair = 0 is PTZ_OK. */
typedef struct ptz_rotfocal_gate ptz_rotfocal_gate;
int32_t ptz_rotfocal_gate_create(int32_t max_pairs, int64_t max_matches, int32_t device_id, ptz_rotfocal_gate** out);
void ptz_rotfocal_gate_destroy(ptz_rotfocal_gate* g);
int32_t ptz_rotfocal_gate_run_device(ptz_rotfocal_gate* g, int32_t n_pair, const int64_t* d_match_ptr, const float* d_uv_a,
                                     const float* d_uv_b, const double* d_cam_ref, const double* d_cam_cur, double thresh,
                                     int32_t min_inliers, int32_t iters, double* d_model /* or NULL */, double* d_H /* or NULL */,
                                     int32_t* d_found, uint8_t* d_mask /* or NULL */, int64_t* d_out_ptr, float* d_out_uv_a,
                                     float* d_out_uv_b, int32_t* d_out_index /* or NULL */, void* hip_stream);
/* The same run on HOST arrays: upload, ptz_rotfocal_gate_run_device, download.  Also PTZ_EINVAL: match_ptr[0] != 0 or decreasing
 * offsets; PTZ_ELIMIT: more matches than the gate's max_matches.  device_ms (or NULL): the four kernels, between events. */
int32_t ptz_rotfocal_gate_run(ptz_rotfocal_gate* g, int32_t n_pair, const int64_t* match_ptr, const float* uv_a, const float* uv_b,
                              const double* cam_ref, const double* cam_cur, double thresh, int32_t min_inliers, int32_t iters,
                              double* model /* or NULL */, double* H /* or NULL */, int32_t* found, uint8_t* mask /* or NULL */,
                              int64_t* out_ptr, float* out_uv_a, float* out_uv_b, int32_t* out_index /* or NULL */, double* device_ms);

/* Gate, then solve, in one call:
 *   replaces the loop body of run_ptz_reloc.cc:68-118 for callers whose matches hold outliers -- upload, gate with
 *   src = uv_ref, dst = uv_cur, the LM of ptz_krt_solve_batch on the compacted CSR (ptz_krt_solve_batch_device's launch, same
 *   stream, no host round trip in between), download.
 * Arguments as ptz_krt_solve_batch.  A query that does not pass is solved on no matches, i.e. gets exactly what
 * ptz_krt_solve_batch returns for a query whose range is empty, and n_inliers = 0.  n_inliers [n_query]: kept matches;
 * inlier_mask [n_match] or NULL: 1 for every kept match, 0 for every other (all of a query that does not pass);
 * H [9 n_query] or NULL: the estimator's H, untouched where it found none; device_ms [2] or NULL: gate, LM.
 * The offsets are read on the host, so the bound tables are built per distinct size and no pair size limit applies.
 * PTZ_EINVAL, before any device work: the list of ptz_homography_ransac_batch, min_inliers < 0, NULL cameras / summaries /
 * accepted / n_inliers with n_query > 0; PTZ_EUNSUPPORTED: factor_type.  n_query = 0 is PTZ_OK. */
int32_t ptz_krt_solve_batch_gated(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                  const double* cam_ref, double* cam_cur, int32_t factor_type, double max_reproj_error,
                                  double ransac_thresh, int32_t min_inliers, const ptz_lm_options* opt, ptz_lm_summary* summaries,
                                  int32_t* accepted, int32_t* n_inliers /* [n_query] */,
                                  uint8_t* inlier_mask /* [n_match] or NULL */, double* H /* [9 n_query] or NULL */,
                                  double* device_ms /* [2]: gate, LM; or NULL */);
/* Host logic only (no device): the bound table a gate of max_pair_matches holds.  *table_len = its length, offsets
 * [max_pair_matches + 1] (or NULL) = where size n's n + 1 entries begin (sizes below 5 have none), table (or NULL) = the
 * entries: ptz_debug_homography_bounds size after size. */
int32_t ptz_debug_match_gate_table(int32_t max_pair_matches, int32_t* table, int64_t* table_len, int64_t* offsets);

/* ------------------------------------------------------------------------------------------------
 * Covariance of relocalized cameras (per query)
 * ------------------------------------------------------------------------------------------------ */
/* what calibration tools report beside a camera (cv::calibrateCamera's stdDeviations, ceres::Covariance) and the reference
 * does not: its only quality signal is the mean reprojection error against max_reproj_error (CheckResults,
 * krt_optimizer.cc:504-533), which a well and an ill constrained camera pass alike.
 * For query q: the refined camera cam_cur (world frame, as ptz_krt_solve_batch returns it) is moved into the local frame of
 * cam_ref as the solve does (krt_optimizer.cc:269-284).  Free parameters p = [fx, (fy), d1, d2, d3, (k1)], NF =
 * ptz_krt_free_dim(factor_type) of them; d is a LEFT perturbation of the current rotation, R <- Exp(d) R, in radians about the
 * current camera's own x (right), y (down), z (forward) axes -- it perturbs the world rotation R_local R_ref in the same way,
 * so the result does not depend on the reference view.  F / FDist: fy := fx as in the solve.  Residual blocks that count:
 * every match whose match_mask byte is non-zero (all, if match_mask = NULL) and that the border guard of the distortion
 * variants does not skip (krt_optimizer.cc:97-101), and every 2D-3D point; B blocks, m = 2 B residuals.  N = J^T J and
 * cost = 1/2 sum r^2 over them, sigma0^2 = 2 cost / (m - NF);  cov = sigma0^2 N^-1 if pixel_sigma = 0 (a-posteriori),
 * pixel_sigma^2 N^-1 if pixel_sigma > 0 (a-priori); sigma0 is returned either way.  N is scaled to unit diagonal, factored by
 * Cholesky and inverted in registers.  status[q]:
 *   PTZ_COV_OK        covariance computed: cov [NF * NF] row-major and sigma0 written;
 *   PTZ_COV_DOF       m <= NF (B = 0 included);
 *   PTZ_COV_SINGULAR  a diagonal entry of N not positive and finite, a pivot of the scaled matrix <= 1e-10, or a non-finite cost
 *                     or covariance;
 *   PTZ_COV_SKIPPED   `accepted` given and accepted[q] = 0 (the solve never wrote that query's cam_cur);
 * with every status but PTZ_COV_OK the query's cov and sigma0 are left untouched.  One reduction order whatever the launch: sixteen
 * lanes per query, lane l sums matches l, l + 16, .. and then points l, l + 16, .., the lanes are added by the butterfly
 * l ^ 8, l ^ 4, l ^ 2, l ^ 1 -- a query's bits depend on its own data only, not on its neighbours or their number.
 * match_mask takes the inlier_mask of ptz_krt_solve_batch_gated as it is; point_ptr = pts2d = pts3d = NULL: no 2D-3D blocks.
 * PTZ_EINVAL, before any device work: n_query < 0, match_ptr[0] != 0 or decreasing offsets, NULL required arrays with non-zero
 * extents, pixel_sigma negative or not finite, point_ptr without pts2d / pts3d; PTZ_EUNSUPPORTED: factor_type;
 * n_query = 0 is PTZ_OK; PTZ_ENODEVICE without a device (no CPU fallback). */
#define PTZ_COV_OK 0
#define PTZ_COV_DOF 1
#define PTZ_COV_SINGULAR 2
#define PTZ_COV_SKIPPED 3
/* Host logic only: free parameters of a factor type -- 4, 5, 5, 6 for F, FDist, Fxfy, FxfyDist; PTZ_EUNSUPPORTED otherwise. */
int32_t ptz_krt_free_dim(int32_t factor_type);
int32_t ptz_krt_covariance_batch(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                 const int64_t* point_ptr, const float* pts2d, const double* pts3d, const double* cam_ref,
                                 const double* cam_cur /* refined, world frame */, int32_t factor_type,
                                 const uint8_t* match_mask /* [n_match] or NULL */, const int32_t* accepted /* [n_query] or NULL */,
                                 double pixel_sigma, int32_t device_id, double* cov /* [NF * NF * n_query] row-major */,
                                 double* sigma0 /* [n_query] */, int32_t* status /* [n_query] */, double* device_ms /* or NULL */);
/* The same launch on DEVICE pointers: enqueued on `hip_stream` (NULL = the default stream) of the device that owns d_cam_cur,
 * returns without synchronising.  Behind ptz_krt_solve_batch_device on the same stream it takes the d_cam_cur and d_accepted that
 * call wrote, with no host round trip.  The CSR offsets are not validated (they live on the device); PTZ_EINVAL also for a
 * stream of another device than the buffers. */
int32_t ptz_krt_covariance_batch_device(int32_t n_query, const int64_t* d_match_ptr, const float* d_uv_ref, const float* d_uv_cur,
                                        const int64_t* d_point_ptr, const float* d_pts2d, const double* d_pts3d,
                                        const double* d_cam_ref, const double* d_cam_cur, int32_t factor_type,
                                        const uint8_t* d_match_mask, const int32_t* d_accepted, double pixel_sigma, double* d_cov,
                                        double* d_sigma0, int32_t* d_status, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Covariance of bundle-adjusted cameras (per view)
 * ------------------------------------------------------------------------------------------------ */
/* what cv::calibrateCamera and ceres::Covariance report and the reference does not: PTZRayOptimizer hands back N cameras and one
 * scalar, the mean reprojection error of the whole rig (ptzray_optimizer.cc:960-968), with no sign of which views are weak.
 * Scope: a batch of 2D-2D problems of type PTZRay, PTZRayDist or PTZRayFxfyDist (ptz_ba_batch_create or
 * ptz_ba_batch_create_views), evaluated at exactly the state ptz_ba_batch_get_state would return at the moment of the call: after a
 * solve the minimum-cost point, before any solve the state last set.
 * Parameters: per camera p = [fx, (fy), d1, d2, d3, (k1)], NF = ptz_ba_cov_dim(factor_type) = 4 / 5 / 6 of them, order and meaning
 * those of ptz_krt_covariance_batch: d is a LEFT perturbation R <- Exp(d) R in radians about the camera's own x, y, z axes (the
 * kernels differentiate with respect to the additive Rodrigues vector and convert each camera's block with the left Jacobian of
 * SO(3), C_d = A C_r A^T).
 * Per ray r over its candidate observations o (closed-form Jacobians, no Jacobi scaling; A_o 2 x NF, B_o 2 x 3, w_r the track
 * weight): V_r = w_r sum B_o^T B_o, E_o = w_r A_o^T B_o, P_r = (V_r + 1/2 tr(V_r) x^ x^T)^-1 -- every 2D-2D functor is invariant to
 * the scale of the ray, so V_r has rank 2 with null vector x^ and, since E_o x^ = 0, E_o P_r E_o'^T = E_o V_r^+ E_o'^T exactly.
 * Reduced matrices: S[c_o, c_o'] = sum_r ([o = o'] w_r A_o^T A_o - E_o P_r E_o'^T), T the same sum with every term multiplied once
 * more by w_r; a ray with a single candidate observation contributes exactly zero.  The track weights are not inverse variances:
 * under iid pixel noise the estimator's covariance is the sandwich s^2 H^-1 (J^T W^2 J) H^-1, whose camera part is s^2 S^-1 T S^-1
 * (sigma0^2 (J^T W J)^-1 would understate the standard deviations about twofold for track lengths 2..6).
 * Gauge: rotation-only bundle adjustment leaves the global rotation free.  gauge_cam[k] names the anchor of problem k (NULL: camera
 * 0): its three rotation rows and columns are identity in S and zero in T, and zero in the result, which describes every view's
 * rotation RELATIVE TO THE ANCHOR; the anchor's fx / fy / k1 entries are ordinary.
 * Solve: S is scaled to unit diagonal and factored by the batch Cholesky (FP64 matrix cores), S^-1 is formed by 64 x 64 tiles;
 * C = s^2 S^-1 T S^-1, of which the per-camera diagonal blocks are returned: cov [NF * NF per camera, concatenated over the
 * problems in order], row-major, symmetric bit for bit.  s = pixel_sigma if pixel_sigma > 0, else s = sigma0 with
 * sigma0^2 = sum_o |e_o|^2 / (m - p), the residuals UNWEIGHTED, m = 2 n_obs, p = NF n_cam - 3 + 2 n_ray; sigma0 [n problems] is
 * returned either way.  It is an ESTIMATE of the pixel noise: exact in expectation for equal weights, within a per cent for track
 * weights 2..6.
 * status [n problems]: PTZ_COV_OK; PTZ_COV_DOF: m <= p; PTZ_COV_SINGULAR: the Cholesky's fail flag, a diagonal entry of S that is
 * not positive and finite, a non-finite result, or an observation in the behind-the-camera penalty branch of PTZRayDist (no
 * linearisation there).  With any status but PTZ_COV_OK the problem's cov and sigma0 are left untouched.
 * PTZ_EUNSUPPORTED: PTZRayDistDisp, a batch with 2D-3D annotations, shared intrinsics.  PTZ_EINVAL, before any device work: NULL
 * batch or outputs, no state, gauge_cam out of range, pixel_sigma negative or not finite.
 * The call does not disturb the batch: a ptz_ba_batch_solve after it returns the bits it returns without it.  Large batches are
 * processed in groups under a workspace budget (PTZ_BA_COV_MAX_MB, default 2048); a problem's bits depend neither on its position
 * in the batch nor on the grouping nor on the run.  device_ms (may be NULL): device time of the covariance kernels. */
/* Host logic only: 4, 5, 6 for PTZRay, PTZRayDist, PTZRayFxfyDist; PTZ_EUNSUPPORTED otherwise. */
int32_t ptz_ba_cov_dim(int32_t factor_type);
int32_t ptz_ba_batch_covariance(ptz_ba_batch* b, const int32_t* gauge_cam /* [n] or NULL */, double pixel_sigma,
                                double* cov /* [NF * NF * sum n_cam] */, double* sigma0 /* [n] */, int32_t* status /* [n] */,
                                double* device_ms /* or NULL */);
/* One-shot: create + set_state + covariance + destroy for a single problem at the state (cam, ray) given, with no solve.
 * cov [NF * NF * n_cam], sigma0 [1], status [1]. */
int32_t ptz_ba_covariance(const ptz_ba_problem* p, const double* cam, const double* ray, int32_t gauge_cam, double pixel_sigma,
                          const ptz_lm_options* opt, double* cov, double* sigma0, int32_t* status);

/* ------------------------------------------------------------------------------------------------
 * Covariance of georeferenced cameras and of the rig's projection centre
 * ------------------------------------------------------------------------------------------------ */
/* The uncertainty of what the georeferencing bundle adjustment outputs -- the world cameras R_i R_lw -- and of where the rig
 * stands, which ptz_ba_batch_covariance (2D-2D problems only, rotations relative to an anchor view) stops one stage short of.
 * Scope: a batch of type PTZRay or PTZRayDist (the two types the georeferencing stage uses), evaluated at exactly the state
 * ptz_ba_batch_get_state would return, T_l_w included.  A problem takes part if it has n_obs3d > 0.
 * Parameters of the linearisation (closed-form Jacobians, no Jacobi scaling): per camera the NC = ptz_ba_batch_cam_block_dim
 * columns [fx, fy, (k1), r1, r2, r3], per problem the T_l_w block L = [rho1..3, t1..3], per ray its rank-2 block, eliminated as
 * in ptz_ba_batch_covariance (rays do not enter 2D-3D residuals).  fy is read only by the 2D-3D functor: the fy column of a camera
 * WITHOUT annotations is identically zero and is treated like a gauge row (identity in S, zero in M).
 * Reduced system, order NC n_cam + 6: S = the 2D-2D part of ptz_ba_batch_covariance plus, per annotation a of camera c (weight 1;
 * A_a 2 x NC, G_a 2 x 6): A_a^T A_a into block (c, c), A_a^T G_a into the border (c, L), G_a^T G_a into (L, L).
 * Noise: clicked annotations and matched key points do not share one level.  M = s_f^2 T_f + s_a^2 T_a with T_f the T of
 * ptz_ba_batch_covariance and T_a the annotation terms of S; the full covariance is C = S^-1 M S^-1.  s_f = pixel_sigma and
 * s_a = annotation_sigma where positive; a zero is estimated from the UNWEIGHTED residuals:
 * s_f^2 = SSE_2d2d / (2 n_obs - p_f), p_f = NF2 n_cam - 3 + 2 n_ray with NF2 = 4 / 5 (the rule of ptz_ba_batch_covariance), and
 * s_a^2 = SSE_2d3d / (2 n_obs3d - p_a), p_a = 6 + (number of annotated cameras); p_f + p_a is the parameter count.  Both estimates
 * are returned either way, sigma0[2k] and sigma0[2k + 1].  They are ESTIMATES, not exact: the split of the degrees of freedom
 * between the two kinds of residual is a heuristic, and s_a comes out a few per cent low (about 0.96 of the truth on a 6-view rig
 * with 24 annotations).
 * Gauge: gauge_cam[k] (NULL: camera 0) names the camera whose three rotation columns are anchored, as in
 * ptz_ba_batch_covariance.  The outputs are WORLD-frame quantities: they do not depend on the anchor beyond round-off, and the
 * anchor's rows are NOT zero.
 * Outputs per problem: cov [NF * NF per camera, concatenated over the problems in order], NF = ptz_ba_geo_cov_dim = 4 / 5, order
 * [fx, d1, d2, d3, (k1)] -- the slots of ptz_ba_batch_covariance, but d is now a LEFT perturbation of the WORLD rotation
 * R_w = R_i R_lw about the camera's own axes: to first order d_w = d_i + R_i d_lw, so the block is
 * C_ii + R_i C_ll R_i^T + C_il R_i^T + R_i C_li over the left-perturbation forms of both rotations (the additive Rodrigues columns
 * convert with the left Jacobian of SO(3), for the cameras and likewise for rho); fy is marginalised.  cov_centre [9 per problem]:
 * covariance of the projection centre C_w = -R_lw^T t_lw in world units, dC_w = -R_lw^T ([t_lw]_x d_lw + tau); the extrinsic
 * translation t_i is not part of the 2D-3D model and not part of this.  Both row-major, symmetric bit for bit.
 * status [n problems]: PTZ_COV_OK; PTZ_COV_DOF: 2 n_obs <= p_f or 2 n_obs3d <= p_a (a problem without annotations lands here);
 * PTZ_COV_SINGULAR: the Cholesky's fail flag, a diagonal entry of S that is not positive and finite, a non-finite result, a 2D-2D
 * observation in the penalty branch of PTZRayDist, or a 2D-3D point with camera-frame z <= 0.  With any status but PTZ_COV_OK the
 * problem's cov, cov_centre and sigma0 are left untouched.
 * PTZ_EUNSUPPORTED: PTZRayFxfyDist, PTZRayDistDisp, shared intrinsics.  PTZ_EINVAL, before any device work: NULL batch or
 * outputs, no state, gauge_cam out of range, a sigma negative or not finite.
 * No floating-point atomics: a camera's annotation terms are summed over its annotations in stored order, (L, L) in stored
 * order; a problem's bits depend neither on its position in the batch nor on the grouping under PTZ_BA_COV_MAX_MB nor on the
 * run.  The call does not disturb the batch: a ptz_ba_batch_solve after it returns the bits it returns without it.
 * device_ms (may be NULL): device time of the covariance kernels. */
/* Host logic only: 4, 5 for PTZRay, PTZRayDist; PTZ_EUNSUPPORTED otherwise. */
int32_t ptz_ba_geo_cov_dim(int32_t factor_type);
int32_t ptz_ba_batch_covariance_georef(ptz_ba_batch* b, const int32_t* gauge_cam /* [n] or NULL */, double pixel_sigma,
                                       double annotation_sigma, double* cov /* [NF * NF * sum n_cam] */,
                                       double* cov_centre /* [9 n] */, double* sigma0 /* [2 n] */, int32_t* status /* [n] */,
                                       double* device_ms /* or NULL */);
/* One-shot: create + set_state + covariance_georef + destroy for a single problem at the state (cam, ray, tlw) given, with no
 * solve.  cov [NF * NF * n_cam], cov_centre [9], sigma0 [2], status [1]. */
int32_t ptz_ba_covariance_georef(const ptz_ba_problem* p, const double* cam, const double* ray, const double* tlw, int32_t gauge_cam,
                                 double pixel_sigma, double annotation_sigma, const ptz_lm_options* opt, double* cov,
                                 double* cov_centre, double* sigma0, int32_t* status);

/* ------------------------------------------------------------------------------------------------
 * Residual report and outlier trimming of the bundle adjustment
 * ------------------------------------------------------------------------------------------------ */
/* what incremental SfM tools do between solves and the reference does not: every observation of every track goes into its
 * squared-loss LM (ptzray_optimizer.cc:799-850) and the only figure that comes back is the rig's mean reprojection error (:960-968).
 *
 * ptz_ba_batch_residuals -- the report, on the device, at exactly the state ptz_ba_batch_get_state would return.  Scope: a batch
 * of ptz_ba_batch_create or ptz_ba_batch_create_views, type PTZRay, PTZRayDist or PTZRayFxfyDist, annotations allowed;
 * PTZ_EUNSUPPORTED: PTZRayDistDisp, shared intrinsics.  Host outputs, concatenated over the problems at their real extents, any
 * may be NULL (all NULL: PTZ_EINVAL, like a NULL batch or a batch without state -- checked before any device work):
 *   err_px [sum n_obs]      |e_o|, the norm of the UNWEIGHTED 2-vector residual (the functors of the LM, the 1e6 penalty branch of
 *                           PTZRayDist as it stands), in the caller's observation order; for a view batch that is the order of
 *                           the packed problem of the same view
 *   ray_max, ray_worst [sum n_ray]   the largest err_px of the track and the problem-local index of that observation (the lowest
 *                           index on a tie), in the caller's ray numbering
 *   view_rms, view_max, view_count [sum n_cam]   over the camera's observations: sqrt(mean |e_o|^2), max |e_o|, their number
 *   rms, median [n]         sqrt(mean |e_o|^2) of the problem (PTZRayOptimizer's final_reproj_error_2d2d); the exact LOWER median,
 *                           element (n_obs - 1) / 2 of the sorted err_px (not computed when NULL)
 *   err3d_px [sum n_obs3d], rms3d [n]   the same for the 2D-3D annotations; rms3d is NaN for a problem without annotations
 * No floating-point atomics, one reduction shape per figure: a problem's bits depend neither on its position in the batch nor on
 * the run.  The call does not disturb the batch: a ptz_ba_batch_solve after it returns the bits it returns without it.
 * device_ms (may be NULL): device time of the report's kernels. */
int32_t ptz_ba_batch_residuals(ptz_ba_batch* b, double* err_px, double* ray_max, int32_t* ray_worst, double* view_rms, double* view_max,
                               int32_t* view_count, double* rms, double* median, double* err3d_px, double* rms3d, double* device_ms);
/* The selection rule on that report: threshold[k] = max(trim_px, k_sigma * median / 1.1774) (1.1774: the median of a Rayleigh
 * variable with unit per-axis sigma; k_sigma = 0: trim_px, no median taken); every ray rejects AT MOST ONE observation, its
 * ray_worst, if ray_max > threshold -- one wrong observation drags its whole ray, so the others are judged after the next solve.
 * reject [sum n_obs] (1 = rejected, caller's order), threshold [n], n_reject [n]; any may be NULL, not all.  PTZ_EINVAL also for
 * trim_px not positive and finite, k_sigma negative or not finite. */
int32_t ptz_ba_batch_trim_select(ptz_ba_batch* b, double trim_px, double k_sigma, uint8_t* reject, double* threshold, int32_t* n_reject,
                                 double* device_ms);
/* Host logic only (no device): the problem `in` without the observations whose reject byte is non-zero and without every ray
 * left with fewer than 2 observations (with what it still had: a single-observation ray adds exactly zero to the reduced system).
 * Surviving rays are renumbered ascending, the order inside a ray is kept; ray_weight_out = ray_weight_in - (observations of
 * that ray removed); ray_map [n_ray_in] = new index or -1.  The out arrays need room for the input's extents; annotations and
 * ic_of_cam are not touched (the caller copies `in` and swaps the five fields).  PTZ_ENOOBS: a camera would be left without any
 * observation -- nothing is written, trimming never drops a view.  PTZ_EINVAL: NULL arguments, empty extents, indices out of
 * range, obs_ray decreasing. */
int32_t ptz_ba_problem_trim(const ptz_ba_problem* in, const uint8_t* reject, float* obs_uv_out, int32_t* obs_cam_out, int32_t* obs_ray_out,
                            double* ray_weight_out, int32_t* ray_map, int32_t* n_ray_out, int64_t* n_obs_out);

typedef struct ptz_trim_options {
  double trim_px;      /* 4.0 */
  double k_sigma;      /* 3.0 */
  int32_t max_rounds;  /* 8: solves per problem at most */
  int32_t reserved_;   /* 0 */
} ptz_trim_options;
void ptz_trim_options_default(ptz_trim_options* o);
#define PTZ_TRIM_ENOOBS 1     /* re-packing would have emptied a view: finished at the result it had */
#define PTZ_TRIM_MAX_ROUNDS 2 /* observations above the threshold remain after max_rounds solves */
typedef struct ptz_trim_report {
  int32_t rounds;         /* solves of this problem */
  int32_t flags;          /* PTZ_TRIM_* */
  int64_t n_obs_removed;  /* rejected observations and those that left with their ray */
  int32_t n_ray_removed;
  int32_t reserved_;
  double threshold;       /* of the last selection */
  double rms_first;       /* 2D-2D rms after the first solve, all observations */
  double rms_last;        /* ... after the last solve, over the observations kept */
} ptz_trim_report;
/* The trimmed solve.  Round 0: the n problems as given, one batch, from (cam, ray, tlw).  After every round: the report and the
 * selection on the round's batch; a problem with n_reject = 0, or one that has run max_rounds solves, is finished; the others
 * are re-packed (ptz_ba_problem_trim; PTZ_ENOOBS finishes the problem at the result it has, flagged) and solved together in one
 * new batch, cameras from the previous round's solution, rays through ray_map, nothing re-initialised.  The existing batch API is
 * used as it is: a problem's result is the bits of the manual loop over ptz_ba_solve, ptz_ba_batch_trim_select and
 * ptz_ba_problem_trim, whatever the other problems of the call do.
 * Out: cam / tlw and summaries [n] (or NULL) of each problem's last solve; ray in the INPUT numbering, removed rays left as given;
 * kept [sum n_obs] (or NULL): 1 for every observation of the last solve; report [n] (or NULL).  trim = NULL: the defaults.
 * PTZ_EUNSUPPORTED: PTZRayDistDisp, shared intrinsics.  PTZ_EINVAL: malformed problems or options.  Annotations pass through
 * untrimmed. */
int32_t ptz_ba_solve_trimmed_batch(int32_t n, const ptz_ba_problem* problems, double* cam, double* ray, double* tlw,
                                   const ptz_trim_options* trim, const ptz_lm_options* opt, ptz_lm_summary* summaries,
                                   uint8_t* kept /* [sum n_obs] */, ptz_trim_report* report /* [n] */);
int32_t ptz_ba_solve_trimmed(const ptz_ba_problem* p, double* cam, double* ray, double* tlw, const ptz_trim_options* trim,
                             const ptz_lm_options* opt, ptz_lm_summary* summary, uint8_t* kept, ptz_trim_report* report);

/* ------------------------------------------------------------------------------------------------
 * Residual report and outlier trimming of relocalized cameras (per query)
 * ------------------------------------------------------------------------------------------------ */
/* the online counterpart of the section above.  A relocalized camera comes back with one scalar, the mean reprojection error that
 * CheckResults compares with max_reproj_error (krt_optimizer.cc:504-533); nobody sees which matches the fit rests on, and a match
 * inside the homography gate's threshold is never judged again by the functors the LM fits.
 *
 * ptz_krt_residuals_batch -- the report.  Arguments as ptz_krt_covariance_batch: CSR matches, optional 2D-3D points, cam_ref, the
 * refined cam_cur (world frame), match_mask, accepted.  The LM's own functors, evaluated once at the refined camera in the form the
 * solve takes its final cost with (IEEE quotients), the camera moved into the local frame of cam_ref as the solve does.  Outputs,
 * any may be NULL (all NULL: PTZ_EINVAL):
 *   err_px [n_match]     |e_m|, the norm of the UNWEIGHTED 2-vector residual, in the caller's order, for EVERY match of the query,
 *                        masked or not; -1.0 for a match the border guard of the distortion variants skips (krt_optimizer.cc:97-101)
 *   err3d_px [n_point]   the same for the 2D-3D points
 *   rms, max, median, count [n_query]   over the COUNTED matches: mask byte non-zero (all, if match_mask = NULL) and not skipped;
 *                        sqrt(mean |e_m|^2), max |e_m|, the exact LOWER median -- element (count - 1) / 2 of the sorted errors --,
 *                        their number.  rms, max and median are NaN with count = 0
 *   rms3d [n_query]      over the query's points; NaN without points
 * For a query with accepted[q] = 0 every output is left untouched and its cam_cur is not read.
 * lanes_per_query: 16 or 64 lanes of a wave per query, anything else: by the launch size as ptz_krt_solve_batch
 * (ptz_lm_options::krt_lanes_per_query).  A speed matter only: one reduction order per figure whatever the group (64 partial sums,
 * partial v takes matches v, v + 64, ..; added by the butterfly v ^ 32, v ^ 16, .. v ^ 1), the median a selection by counting over
 * the bit patterns, no floating-point atomics -- a query's bits depend on its own data only, not on its neighbours, their number,
 * the group size or the run.
 * PTZ_EINVAL, before any device work: n_query < 0, match_ptr[0] != 0 or decreasing offsets, NULL required arrays with non-zero
 * extents, point_ptr without pts2d / pts3d; PTZ_EUNSUPPORTED: factor_type; n_query = 0 is PTZ_OK; PTZ_ENODEVICE without a device. */
int32_t ptz_krt_residuals_batch(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                const int64_t* point_ptr, const float* pts2d, const double* pts3d, const double* cam_ref,
                                const double* cam_cur /* refined, world frame */, int32_t factor_type,
                                const uint8_t* match_mask /* [n_match] or NULL */, const int32_t* accepted /* [n_query] or NULL */,
                                int32_t lanes_per_query, int32_t device_id, double* err_px, double* err3d_px, double* rms, double* max,
                                double* median, int32_t* count, double* rms3d, double* device_ms /* or NULL */);
/* The same launch on DEVICE pointers: enqueued on `hip_stream` (NULL = the default stream) of the device that owns d_cam_cur,
 * returns without synchronising; behind ptz_krt_solve_batch_device on the same stream it takes the d_cam_cur and d_accepted that call
 * wrote.  The CSR offsets are not validated (they live on the device).  The call keeps no scratch of its own: d_median needs
 * d_err_px (the selection reads the errors of a query of more than 8 x lanes matches back from it), PTZ_EINVAL otherwise, as for a
 * stream of another device than the buffers. */
int32_t ptz_krt_residuals_batch_device(int32_t n_query, const int64_t* d_match_ptr, const float* d_uv_ref, const float* d_uv_cur,
                                       const int64_t* d_point_ptr, const float* d_pts2d, const double* d_pts3d, const double* d_cam_ref,
                                       const double* d_cam_cur, int32_t factor_type, const uint8_t* d_match_mask,
                                       const int32_t* d_accepted, int32_t lanes_per_query, double* d_err_px, double* d_err3d_px,
                                       double* d_rms, double* d_max, double* d_median, int32_t* d_count, double* d_rms3d, void* hip_stream);

typedef struct ptz_krt_trim_options {
  double trim_px;      /* 4.0 */
  double k_sigma;      /* 3.0 */
  int32_t max_rounds;  /* 8: solves per query at most (1 .. 64) */
  int32_t min_keep;    /* 8: counted matches a kept set needs */
} ptz_krt_trim_options;
void ptz_krt_trim_options_default(ptz_krt_trim_options* o);
/* flags of ptz_krt_trim_report, beside PTZ_TRIM_MAX_ROUNDS: matches changed sides in the round of the last solve allowed */
#define PTZ_KRT_TRIM_MIN_KEEP 4 /* the next kept set would have counted fewer than min_keep matches: finished on the set it had */
#define PTZ_KRT_TRIM_REJECTED 8 /* a solve of the query was not accepted under the open bound: cam_cur is left untouched */
typedef struct ptz_krt_trim_report {
  int32_t rounds;      /* solves of this query */
  int32_t flags;       /* PTZ_TRIM_MAX_ROUNDS, PTZ_KRT_TRIM_* */
  int32_t n_removed;   /* matches of the universe that the last solve's set lacks */
  int32_t n_kept;      /* matches of the last solve's set (skipped ones included) */
  double threshold;    /* of the last round judged; NaN if none was */
  double rms_first;    /* rms of the report after the first solve, over the universe */
  double rms_last;     /* ... after the last solve, over its set */
  double median_last;
} ptz_krt_trim_report;
/* The trimmed solve: sigma clipping with the LM's own functors, all rounds on the device, on one stream, no host round trip.
 * The rule (csrc/ptz_krt_trim.h).  Universe U: the query's matches whose match_mask byte is non-zero (all, if NULL; the inlier_mask
 * of ptz_krt_solve_batch_gated as it is).  Round 0 solves on K = U from cam_cur like ptz_krt_solve_batch, with an OPEN error bound
 * (max_reproj_error = 1e300: CheckResults' convergence and field-of-view tests apply).  After every round, for the queries still
 * active: the report above at the round's camera, over the counted matches of K (a match the border guard skips stays in K, counts
 * for nothing and is never rejected); t = max(trim_px, k_sigma * median / 1.1774) (k_sigma = 0: trim_px); the new set
 * K' = { m in U : skipped, or |e_m| <= t } -- EVERY match of U is judged again, a good match that a dragged early fit pushed out
 * comes back.  The query is finished if K' == K; if K' would count fewer than min_keep matches (PTZ_KRT_TRIM_MIN_KEEP, keeps K); if it
 * has run max_rounds solves (PTZ_TRIM_MAX_ROUNDS, keeps K); if its solve was not accepted (PTZ_KRT_TRIM_REJECTED).  Otherwise K'
 * is packed from the ORIGINAL arrays, order kept, and solved from the camera the previous round ended at.  A finished query is not
 * solved again: camera and summary are those of its last solve.  2D-3D points are in every round's solve and are not trimmed.
 * Every round runs with the lanes per query ptz_krt_solve_batch takes for the call's n_query (krt_lanes_per_query honoured).
 * At the end accepted[q] = (last solve accepted under the open bound) && sqrt(2) * sqrt(2 * final_cost / num_residuals) <
 * max_reproj_error; cam_cur is written only for accepted queries.  summaries [n]: of each query's last solve; kept [n_match] (or
 * NULL): 1 for every match of the last solve's set; report [n] (or NULL); trim = NULL: the defaults.
 * Contract: a query's result is the bits of the manual loop over ptz_krt_solve_batch[_2d3d] with the open bound,
 * ptz_krt_residuals_batch, the rule and a compaction of the caller's arrays -- whatever the other queries of the call do.
 * PTZ_EINVAL, before any device work: as ptz_krt_residuals_batch, NULL summaries / accepted, trim_px not positive and finite, k_sigma
 * negative or not finite, max_rounds outside 1 .. 64, min_keep negative. */
int32_t ptz_krt_solve_batch_trimmed(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                    const int64_t* point_ptr, const float* pts2d, const double* pts3d, const double* cam_ref,
                                    double* cam_cur, int32_t factor_type, double max_reproj_error,
                                    const uint8_t* match_mask /* [n_match] or NULL */, const ptz_krt_trim_options* trim,
                                    const ptz_lm_options* opt, ptz_lm_summary* summaries, int32_t* accepted, uint8_t* kept,
                                    ptz_krt_trim_report* report, double* device_ms /* or NULL */);
/* The same on DEVICE pointers: max_rounds rounds are enqueued on `hip_stream` and the call returns without synchronising; a round
 * in which no query is active costs its launches' early returns.  n_match: the extent of the match arrays (the offsets live on the
 * device and are not validated).  d_workspace: 256-byte aligned device memory of at least
 * ptz_krt_trim_workspace_bytes(n_query, n_match) bytes, the caller's until the stream has run the call. */
int64_t ptz_krt_trim_workspace_bytes(int32_t n_query, int64_t n_match);
int32_t ptz_krt_solve_batch_trimmed_device(int32_t n_query, int64_t n_match, const int64_t* d_match_ptr, const float* d_uv_ref,
                                           const float* d_uv_cur, const int64_t* d_point_ptr, const float* d_pts2d, const double* d_pts3d,
                                           const double* d_cam_ref, double* d_cam_cur, int32_t factor_type, double max_reproj_error,
                                           const uint8_t* d_match_mask, const ptz_krt_trim_options* trim, const ptz_lm_options* opt,
                                           ptz_lm_summary* d_summaries, int32_t* d_accepted, uint8_t* d_kept,
                                           ptz_krt_trim_report* d_report, void* d_workspace, int64_t workspace_bytes, void* hip_stream);

/* ---- descriptor matching: the match table from features ------------------------------------------------------------------------
 * What ReadColmapMatches (src/core/data_io.cc) reads from pairs_matches.txt, computed: mutual nearest neighbours of uint8
 * descriptors under Lowe's ratio test, for a batch of image pairs.  The contract is csrc/ptz_desc_match.h, all integer:
 * d2(i, j) = sum_k (a_ik - b_jk)^2 in int32; best(i) = the j of smallest d2, lowest j on a tie; second(i) = the smallest d2 over
 * j != best(i), INT32_MAX if there is none.  (i, j) is a match when j = best_A(i); with cross_check, i = best_B(j); with ratio > 0,
 * (double)d2 < ratio^2 * (double)second on A's side and, with cross_check, on B's side as well (so the matches of (B, A) are the
 * transposed matches of (A, B)); and max_dist2 == 0 or d2 <= max_dist2.  A pair with fewer than min_matches matches has none.
 * Matches of a pair are in ascending i, pairs in the caller's order; a pair's result depends on its two images only. */
typedef struct ptz_desc_options {
  double ratio;            /* 0.8; 0: no ratio test */
  int32_t max_dist2;       /* 0: no bound */
  int32_t cross_check;     /* 1 */
  int32_t min_matches;     /* 0 */
  int32_t device_id;       /* 0; must be the sets' device */
  int64_t workspace_bytes; /* 256 MiB: bound on the top-2 state (12 bytes per feature and side) and keep bytes of the pairs in
                              flight; the pair list is processed in chunks that stay below it (one pair at least, 2^20 pairs at most) */
} ptz_desc_options;
void ptz_desc_options_default(ptz_desc_options* o);

/* The descriptors (and key points) of a set of images, packed and resident on the device.  Image m owns features
 * [feat_ptr[m], feat_ptr[m + 1]) of desc [n_feat, D] (uint8, host) and of kp_xy [n_feat, 2] (float32 pixels, host, or NULL: the
 * matches of this set then carry no pixels).
 * PTZ_EINVAL: n_img < 0, feat_ptr[0] != 0 or decreasing, D outside 1 .. 512, NULL desc with features, device_id < 0;
 * PTZ_ELIMIT: more than 2^31 - 1 features in one image. */
typedef struct ptz_desc_set ptz_desc_set;
int32_t ptz_desc_set_create(int32_t n_img, const int64_t* feat_ptr, const uint8_t* desc, int32_t D, const float* kp_xy,
                            int32_t device_id, ptz_desc_set** out);
void ptz_desc_set_destroy(ptz_desc_set* s);

/* Matches of pair p = (image img_a[p] of set_a, image img_b[p] of set_b).  set_a == set_b and img_a[p] == img_b[p] are allowed.
 * opt = NULL: the defaults.  PTZ_EINVAL, before any device work: NULL sets / out, n_pair < 0, different D or devices of the sets,
 * opt->device_id not the sets' device, an image index out of range, ratio negative or not finite, max_dist2 / min_matches
 * negative, workspace_bytes not positive.  n_pair = 0 and images without features are PTZ_OK. */
typedef struct ptz_desc_matches ptz_desc_matches;
int32_t ptz_desc_match_pairs(const ptz_desc_set* set_a, const ptz_desc_set* set_b, int32_t n_pair, const int32_t* img_a,
                             const int32_t* img_b, const ptz_desc_options* opt, ptz_desc_matches** out);
int64_t ptz_desc_matches_n_matches(const ptz_desc_matches* m);
int32_t ptz_desc_matches_n_pairs(const ptz_desc_matches* m);
double ptz_desc_matches_device_ms(const ptz_desc_matches* m); /* kernels of all chunks, between events on the call's stream */
int32_t ptz_desc_matches_n_chunks(const ptz_desc_matches* m);
/* every pointer nullable: match_ptr [n_pair + 1], idx_a / idx_b / dist2 [n_matches] int32, uv_a / uv_b [n_matches, 2] float32
 * (PTZ_EINVAL if asked of a set created without key points) */
int32_t ptz_desc_matches_download(const ptz_desc_matches* m, int64_t* match_ptr, int32_t* idx_a, int32_t* idx_b, int32_t* dist2,
                                  float* uv_a, float* uv_b);
/* the same arrays on the device, the result's until it is destroyed, in the layout ptz_match_gate_run_device and
 * ptz_krt_solve_batch_device take (d_uv_* NULL without key points); every out pointer nullable */
int32_t ptz_desc_matches_device_ptrs(const ptz_desc_matches* m, const int64_t** d_match_ptr, const int32_t** d_idx_a,
                                     const int32_t** d_idx_b, const int32_t** d_dist2, const float** d_uv_a, const float** d_uv_b);
void ptz_desc_matches_destroy(ptz_desc_matches* m);

/* Homography-guided matching: the rule of ptz_desc_match_pairs over the candidates pair p's homography admits (the second pass of
 * COLMAP's guided_matching and of OpenCV's stitching matcher, for texture that repeats).  H [9 n_pair] row-major, b ~ H a, as
 * ptz_homography_ransac_batch returns it for src = A's pixels, dst = B's.  Contract (csrc/ptz_desc_match.h): feature i of A is
 * warped in double, X = H0 x + H1 y + H2 and Y, Z likewise, left to right without fma; ok(i) = Z > 0 and X, Y, Z finite; the pair
 * (i, j) is ADMISSIBLE iff ok(i) and, in float without fma, (wx - bx)^2 + (wy - by)^2 <= (float)(radius_px^2), inclusive, with
 * (wx, wy) = ((float)(X / Z), (float)(Y / Z)) and (bx, by) the pixel of B's feature j.  B's features ask A over the SAME admissible
 * set (the error is measured in B's image in both directions), so best, second (INT32_MAX with fewer than two admissible
 * candidates), ties, the ratio test, cross_check, max_dist2 and min_matches are ptz_desc_match_pairs's over the admissible
 * candidates only, and:
 *   - the matches of (B, A) under the same H and roles are the transposed matches of (A, B); a call with the sets swapped and
 *     H^-1 measures the error in the other image, is another predicate and need not return the transpose;
 *   - a pair's result depends on its two images and its H only (not on the batch, its order or the chunking);
 *   - a radius that admits every candidate returns ptz_desc_match_pairs's arrays.
 * found [n_pair] or NULL (= all 1): a pair with found[p] != 1 has no matches and its H is not read.  A non-finite H is not an
 * error: that pair has no admissible candidate.  The result is an ordinary ptz_desc_matches.
 * PTZ_EINVAL, before any device work: the list of ptz_desc_match_pairs, a set with features but without key points, NULL H with
 * n_pair > 0, a radius that is not finite and positive.
 * ptz_desc_match_pairs_guided_device: d_H and d_found are DEVICE pointers on the sets' device, as ptz_match_gate_run_device leaves
 * them; the call runs on a stream of its own, so the work that writes them must have completed (synchronise its stream first). */
int32_t ptz_desc_match_pairs_guided(const ptz_desc_set* set_a, const ptz_desc_set* set_b, int32_t n_pair, const int32_t* img_a,
                                    const int32_t* img_b, const double* H /* [9 n_pair], b ~ H a */,
                                    const int32_t* found /* [n_pair] or NULL = all 1 */, double radius_px,
                                    const ptz_desc_options* opt, ptz_desc_matches** out);
int32_t ptz_desc_match_pairs_guided_device(const ptz_desc_set* set_a, const ptz_desc_set* set_b, int32_t n_pair, const int32_t* img_a,
                                           const int32_t* img_b, const double* d_H, const int32_t* d_found /* or NULL */,
                                           double radius_px, const ptz_desc_options* opt, ptz_desc_matches** out);
/* The grid-binned guided matcher: a second implementation of the contract above (csrc/ptz_desc_grid.h), the signatures, the error
 * lists and the output arrays of its namesakes, bit for bit.  Per (pair, direction) the searched positions are sorted into the cells
 * of a 32 x 32 grid over their bounding box (cell size at least radius_px (1 + 2^-10)), a query tests the candidates of the cells its
 * reach touches -- a superset of the admissible ones, by the monotonicity of the one cell function -- with the predicate above, and
 * a wave computes the descriptor distance of each hit together.  Off by default everywhere: ptz_reloc_options.guided_grid,
 * DescMatchOptions::guided_grid and --guided_grid select it. */
int32_t ptz_desc_match_pairs_guided_grid(const ptz_desc_set* set_a, const ptz_desc_set* set_b, int32_t n_pair, const int32_t* img_a,
                                         const int32_t* img_b, const double* H, const int32_t* found, double radius_px,
                                         const ptz_desc_options* opt, ptz_desc_matches** out);
int32_t ptz_desc_match_pairs_guided_grid_device(const ptz_desc_set* set_a, const ptz_desc_set* set_b, int32_t n_pair,
                                                const int32_t* img_a, const int32_t* img_b, const double* d_H, const int32_t* d_found,
                                                double radius_px, const ptz_desc_options* opt, ptz_desc_matches** out);
/* tests only: the full matrix d2 [n_a, n_b] (host) of one pair, from the matcher's own matrix-core tile code */
int32_t ptz_debug_desc_dist2(const ptz_desc_set* set_a, int32_t img_a, const ptz_desc_set* set_b, int32_t img_b, int32_t* out);

/* ---- relocalization assembly: from the match table of every (reference, query) pair to the solve's inputs ----------------------
 * What run_ptz_reloc.cc does on the host between the matcher and the solve -- FindBestMatch, the initial camera, the query's CSR --
 * on the device, and for the K = max_refs best references of a query instead of one.  The contract is csrc/ptz_reloc_assemble.h:
 * a query's pairs are ranked by (match count descending, position in its list ascending), pairs without matches never rank; slots
 * 0 .. n_sel - 1 (n_sel <= K) take the first K, slot 0 is the anchor.  cam_cur = [f, f, 0.5 w, 0.5 h, rvec, t, dist] of the anchor.
 * K = 1: the output CSR is a copy of the anchor pair's matches and cam_ref the anchor's camera -- the arrays the tool builds, so every
 * downstream call returns the bits it returns today.  K > 1: cam_ref is the virtual anchor [fa, fa, S, S, rvec_a, t_a, 0 x 5],
 * S = 8192, and every match of every selected pair is re-expressed as a pixel of it (undistorted in its own view for factor_type & 1
 * and dropped where that view's border guard would skip it; rotated R_a R_r^T; dropped behind the anchor or outside [0, 2S)^2).  All
 * references are assumed to share one projection centre (the library's rotation-only model).
 * Inputs: the match CSR over n_pair pairs in the layout of ptz_desc_matches_device_ptrs; pair_ref [n_pair] the reference image of
 * each pair; query_ptr [n_query + 1] the contiguous pair list of each query (query_ptr[0] = 0, query_ptr[n_query] = n_pair);
 * ref_cams [15 n_ref]; ref_R [9 n_ref] row-major, from ptz_reloc_ref_rotations (host logic only: Rodrigues of every reference, once);
 * query_wh [2 n_query] the queries' image sizes.
 * Outputs: sel_pair [K n_query] (pair index, -1 for an unused slot), n_sel [n_query] (0: unusable query, empty range, finite cameras:
 * those of the first reference of its list, reference 0 for an empty list), out_ptr [n_query + 1], out_uv_ref / out_uv_cur
 * [n_match, 2] and out_src [n_match] (index of each kept match in the input arrays) of which the first out_ptr[n_query] entries are
 * written, kept matches slot after slot in each pair's order; cam_ref / cam_cur [15 n_query].
 * A query's output depends on its own pairs only: not on the batch, the order of the queries or the launch.
 * ptz_reloc_assemble (host arrays: upload, run, download).  PTZ_EINVAL, before any device work: negative extents, max_refs < 1,
 * offsets that do not start at 0, decrease or do not cover the pairs, pair_ref outside [0, n_ref), missing arrays, an image size
 * that is not positive, device_id < 0; PTZ_EUNSUPPORTED: an unknown factor_type; PTZ_ELIMIT: more than 2^31 - 1 matches or slots;
 * n_query = 0 is PTZ_OK.
 * ptz_reloc_assemble_device: the same on DEVICE pointers of the device that owns d_cam_cur, enqueued on `hip_stream`, returns without
 * synchronising.  Nothing on the device is validated (a malformed list is an empty one, a pair whose reference is out of range never
 * ranks).  d_workspace: 256-byte aligned device memory of at least ptz_reloc_assemble_workspace_bytes(n_query, n_match) bytes, the
 * caller's until the stream has run the call. */
int32_t ptz_reloc_ref_rotations(int32_t n_ref, const double* ref_cams, double* ref_R);
int64_t ptz_reloc_assemble_workspace_bytes(int32_t n_query, int64_t n_match);
int32_t ptz_reloc_assemble_device(int32_t n_query, int32_t n_pair, int64_t n_match, int32_t n_ref, const int64_t* d_match_ptr,
                                  const float* d_uv_ref, const float* d_uv_cur, const int32_t* d_pair_ref, const int64_t* d_query_ptr,
                                  const double* d_ref_cams, const double* d_ref_R, const int32_t* d_query_wh, int32_t factor_type,
                                  int32_t max_refs, int32_t* d_sel_pair, int32_t* d_n_sel, int64_t* d_out_ptr, float* d_out_uv_ref,
                                  float* d_out_uv_cur, int32_t* d_out_src, double* d_cam_ref, double* d_cam_cur, void* d_workspace,
                                  int64_t workspace_bytes, void* hip_stream);
int32_t ptz_reloc_assemble(int32_t n_query, int32_t n_pair, int32_t n_ref, const int64_t* match_ptr, const float* uv_ref,
                           const float* uv_cur, const int32_t* pair_ref, const int64_t* query_ptr, const double* ref_cams,
                           const double* ref_R, const int32_t* query_wh, int32_t factor_type, int32_t max_refs, int32_t device_id,
                           int32_t* sel_pair, int32_t* n_sel, int64_t* out_ptr, float* out_uv_ref, float* out_uv_cur, int32_t* out_src,
                           double* cam_ref, double* cam_cur, double* device_ms /* or NULL */);

/* ---- the resident serving loop of relocalization ---------------------------------------------------------------------------------
 * What joins the device entry points above.  The references stay on the device: their descriptor set (the caller's, with key
 * points, alive as long as the relocalizer) and their cameras ref_cams [15 n_ref] (image m of the set is camera m).  A run takes the
 * n_query images of query_set (with key points; query_wh [2 n_query] their sizes) through, in this order, every array in between on
 * the device:
 *   1. ptz_desc_match_pairs over all (reference, query) pairs, test image by test image, the references in their order;
 *   2. guided_radius > 0: ptz_match_gate_run_device on all pairs (ransac_thresh, min_inliers) and ptz_desc_match_pairs_guided_device
 *      with the H it leaves and found = (the gate kept matches of the pair), exactly as MatchDescriptors composes the host forms;
 *   3. ptz_reloc_assemble_device (max_refs, factor_type);
 *   4. inlier_matches: ptz_match_gate_run_device on the assembled queries;
 *   5. trim = 0: ptz_krt_solve_batch_device, on the gate's compacted CSR if inlier_matches; trim != 0:
 *      ptz_krt_solve_batch_trimmed_device over the assembled arrays, the gate's kept set as its universe if inlier_matches;
 *   6. uncertainty: ptz_krt_covariance_batch_device over the matches a query kept (the trimming loop's set, else the gate's, else all).
 * The composition is run_ptz_reloc's, so with max_refs = 1 every per-query output is the bits of the path through
 * ptz_krt_solve_batch / _gated / _trimmed and ptz_krt_covariance_batch on the host-selected arrays.  The host reads one word in
 * between (the extent of the assembled arrays) and, at the end, per-query results only -- any pointer of the result may be NULL:
 * cam [15 n_query] (the solve's cam_cur: the initial camera where the query was not accepted), accepted, summaries, sel_ref
 * [max_refs n_query] (reference image of each slot, -1 unused), n_sel, n_matches (assembled), n_inliers (kept by the gate;
 * n_matches without it), trim_report (trim != 0), cov [NF NF n_query] / sigma0 / cov_status (uncertainty), and stage_ms [6]: device
 * time of the stages above (2: the gate's launches plus the guided matcher's).  A query with n_sel = 0 is solved on no matches.
 * guided_grid = 1 runs every guided pass (stage 2, and the matcher of ptz_relocalizer_run_tracked) through
 * ptz_desc_match_pairs_guided_grid_device: the same matches, hence the same outputs; any value but 0 and 1 is PTZ_EINVAL.
 * gate_max_pair_matches (2048, at most 4096): the pair size the gates' bound tables are built for; a pair (stage 2) or a query
 * (stage 4) with more matches does not pass.  The gate object is kept and grows with the runs.
 * ptz_relocalizer_set_gate_model(r, gate_model, gate_iters): the model of stage 4 in every run on r that follows (a relocalizer
 * starts with 0, 128; ptz_reloc_options keeps its layout).  gate_model 0: the homography gate.  1: the rotation-and-focal gate,
 * ptz_rotfocal_gate_run_device with gate_iters samples on the assembled arrays and cam_ref / cam_cur as stage 3 (and the prior) left
 * them on the device -- in all six runs; gate_max_pair_matches does not apply to it, and stage 2 stays the homography gate (a
 * general pair model between two distorted images).  That a query the gate kept nothing of is not accepted in a tracked run is
 * unchanged.  With gate_model = 0 every output is what it was before the call existed.  PTZ_EINVAL, nothing changed: a NULL
 * relocalizer, a gate_model other than 0 and 1, gate_iters outside 1 .. 4096.
 * ptz_relocalizer_gate_models downloads the last run's models of stage 4 (gate_model = 1 and a gated run, PTZ_EINVAL otherwise):
 * model [10 n_query] (f, R row-major; zeros where found is not 1), found [n_query] (the estimator's flag), either may be NULL.
 * ptz_relocalizer_matches downloads the last run's assembled matches (tests): match_ptr [n_query + 1], uv_ref / uv_cur
 * [ptz_relocalizer_n_matches, 2], src (index in the matcher's table), any may be NULL.
 * ptz_relocalizer_table: the last run's match table of all pairs (the guided pass's, if it ran), the relocalizer's until its next run
 * or its end: one ptz_desc_matches_download of it is what --save_matches writes.
 * PTZ_EINVAL, before any device work: NULL relocalizer / sets / result, n_ref < 1, n_query < 0, an image size that is not positive,
 * max_refs < 1, min_inliers < 0, a radius or threshold that is negative or not finite, a device_id in the options that is not the
 * relocalizer's; PTZ_EUNSUPPORTED: factor_type; the stages' own codes otherwise.  Runs on one relocalizer are the caller's to order. */
typedef struct ptz_reloc_options {
  ptz_desc_options match;        /* stage 1 (and 2) */
  double guided_radius;          /* 0: no guided pass */
  double ransac_thresh;          /* 4.0 */
  int32_t min_inliers;           /* 6 */
  int32_t inlier_matches;        /* 0 */
  int32_t trim;                  /* 0 */
  int32_t uncertainty;           /* 0 */
  ptz_krt_trim_options trim_options;
  int32_t max_refs;              /* 1 */
  int32_t factor_type;           /* PTZ_KRT_F */
  double max_reproj_error;       /* 100 */
  int32_t gate_max_pair_matches; /* 2048 */
  int32_t guided_grid;           /* 0: the guided matcher's scan kernel; 1: its grid kernel (the same matches); else PTZ_EINVAL */
  ptz_lm_options lm;
} ptz_reloc_options;
void ptz_reloc_options_default(ptz_reloc_options* o);
typedef struct ptz_reloc_result {
  double* cam;
  int32_t* accepted;
  ptz_lm_summary* summaries;
  int32_t* sel_ref;
  int32_t* n_sel;
  int32_t* n_matches;
  int32_t* n_inliers;
  ptz_krt_trim_report* trim_report;
  double* cov;
  double* sigma0;
  int32_t* cov_status;
  double stage_ms[6];
} ptz_reloc_result;
typedef struct ptz_relocalizer ptz_relocalizer;
int32_t ptz_relocalizer_create(const ptz_desc_set* ref_set, const double* ref_cams, int32_t n_ref, int32_t device_id, ptz_relocalizer** out);
void ptz_relocalizer_destroy(ptz_relocalizer* r);
int32_t ptz_relocalizer_run(ptz_relocalizer* r, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_wh,
                            const ptz_reloc_options* options, ptz_reloc_result* result);
const ptz_desc_matches* ptz_relocalizer_table(const ptz_relocalizer* r);
int64_t ptz_relocalizer_n_matches(const ptz_relocalizer* r);
int32_t ptz_relocalizer_matches(const ptz_relocalizer* r, int64_t* match_ptr, float* uv_ref, float* uv_cur, int32_t* src);
int32_t ptz_relocalizer_set_gate_model(ptz_relocalizer* r, int32_t gate_model, int32_t gate_iters);
int32_t ptz_relocalizer_gate_models(const ptz_relocalizer* r, double* model /* or NULL */, int32_t* found /* or NULL */);

/* ---- reference shortlist: which references a query is worth matching against ----------------------------------------------------
 * A retrieval step in front of the matcher.  The contract is csrc/ptz_desc_shortlist.h, all integer but desc_ratio_ok's multiply:
 *   probes     a query image with n features has m = min(n, n_probes) probes: feature k if n <= n_probes, else feature
 *              floor(k n / n_probes) in int64 -- strictly increasing, in file order;
 *   vote       a probe votes for reference r when its top-2 over ALL features of r (ptz_desc_match_pairs's: lowest j on a tie,
 *              second = INT32_MAX with one candidate) has a feature, passes the ratio test of desc_opt->ratio and, with
 *              desc_opt->max_dist2 != 0, has d2 <= max_dist2.  One direction: cross_check and min_matches do not enter;
 *   shortlist  the references are ranked by (votes descending, reference index ascending), one with fewer than max(min_votes, 1)
 *              votes never ranks, the first min(max_refs, ranked) are taken and written in ASCENDING reference index.
 * Every image of ref_set is a reference.  Query q is image query_img[q] of query_set.  Outputs: shortlist [max_refs n_query]
 * (query q owns entries max_refs q .., -1 in unused slots), n_short [n_query], votes [n_query n_ref].  A query's output depends on
 * its own image, the reference set and the options only: not on the batch, its order or the launch.  An empty query or reference
 * has no votes.  Whenever a query's shortlist contains the references ptz_relocalizer_run would select, matching the shortlisted
 * pairs alone gives that run's per-query bits (a pair's matches depend on its two images only).
 * ptz_desc_shortlist (host arrays: run, download).  PTZ_EINVAL, before any device work: the list of ptz_desc_match_pairs (NULL sets,
 * n_query < 0, different D or devices, desc_opt->device_id not the sets' device, ratio negative or not finite, max_dist2 /
 * min_matches negative, workspace_bytes not positive), max_refs < 1, n_probes < 1, min_votes < 0, an image index out of range, a
 * missing output; PTZ_ELIMIT: more than 2^31 - 1 shortlist slots or vote cells; n_query = 0 is PTZ_OK.  desc_opt / sl_opt = NULL: defaults.
 * ptz_desc_shortlist_device: outputs (and d_query_img, or NULL: query q is image q) are DEVICE pointers on the sets' device; the
 * call is enqueued on `hip_stream` and returns without synchronising.  An image index the device reads out of range is an empty
 * query.  d_workspace: 256-byte aligned device memory of at least ptz_desc_shortlist_workspace_bytes(...) bytes, the caller's until
 * the stream has run the call; whatever it holds before is never read. */
typedef struct ptz_shortlist_options {
  int32_t max_refs;  /* 8: R, the most references a query keeps */
  int32_t n_probes;  /* 256: M, the most features of a query that vote */
  int32_t min_votes; /* 1 */
  int32_t reserved_;
} ptz_shortlist_options;
void ptz_shortlist_options_default(ptz_shortlist_options* o);
int32_t ptz_desc_shortlist(const ptz_desc_set* ref_set, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_img,
                           const ptz_desc_options* desc_opt, const ptz_shortlist_options* sl_opt, int32_t* shortlist, int32_t* n_short,
                           int32_t* votes /* or NULL */, double* device_ms /* or NULL */);
int64_t ptz_desc_shortlist_workspace_bytes(const ptz_desc_set* ref_set, const ptz_desc_set* query_set, int32_t n_query,
                                           const ptz_shortlist_options* sl_opt);
int32_t ptz_desc_shortlist_device(const ptz_desc_set* ref_set, const ptz_desc_set* query_set, int32_t n_query,
                                  const int32_t* d_query_img /* or NULL */, const ptz_desc_options* desc_opt,
                                  const ptz_shortlist_options* sl_opt, int32_t* d_shortlist, int32_t* d_n_short,
                                  int32_t* d_votes /* or NULL */, void* d_workspace, int64_t workspace_bytes, void* hip_stream);

/* ptz_relocalizer_run with the shortlist in front: stage 0 is ptz_desc_shortlist_device of the query images against the resident
 * references (options->match's ratio and max_dist2, sl_opt); the host downloads shortlist and n_short and builds the pair list,
 * query-major, a query's references ascending; stages 1-6 are ptz_relocalizer_run's on that list.  The reference set must hold
 * exactly the relocalizer's n_ref images.  result is ptz_relocalizer_run's (sel_ref stays a reference image index); sl_result (or
 * NULL), every pointer nullable: shortlist [sl_opt->max_refs n_query], n_short [n_query], votes [n_query n_ref], shortlist_ms the
 * device time of stage 0.  A query with n_short = 0 has no pairs and goes on as a query with n_sel = 0.  ptz_relocalizer_table is
 * then the table of the shortlisted pairs.
 * ptz_relocalizer_pairs: the pair list of the last run of either kind, *n_pair pairs, pair_ref [n_pair] the reference image of
 * each, query_ptr [n_query + 1] each query's range; every pointer nullable (ask for n_pair first). */
typedef struct ptz_shortlist_result {
  int32_t* shortlist;
  int32_t* n_short;
  int32_t* votes;
  double shortlist_ms;
} ptz_shortlist_result;
int32_t ptz_relocalizer_run_shortlisted(ptz_relocalizer* r, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_wh,
                                        const ptz_reloc_options* options, const ptz_shortlist_options* sl_opt, ptz_reloc_result* result,
                                        ptz_shortlist_result* sl_result);
int32_t ptz_relocalizer_pairs(const ptz_relocalizer* r, int32_t* n_pair, int32_t* pair_ref, int64_t* query_ptr);

/* ---- relocalization from a prior camera: overlap shortlist and pair homographies ------------------------------------------------
 * For a query whose camera is roughly known (the last frame's, or pan / tilt / zoom telemetry) both expensive questions of the
 * online half have answers before a feature is matched.  The contract is csrc/ptz_reloc_prior.h, doubles with + - * / only:
 *   H          of pair (reference r, query q): K_q R_q R_r^T K_r^-1, with K^-1 written out; the query contributes its image centre
 *              (0.5 w, 0.5 h), the prior's fx, and fy = fx for PTZ_KRT_F / PTZ_KRT_FDist, the prior's fy otherwise.  Distortion
 *              does not enter: the matcher's radius absorbs it.  This is the H ptz_desc_match_pairs_guided takes (A = reference).
 *   overlap    0 .. 128: of an 8 x 8 lattice of cell centres of the reference frame [0, 2cx) x [0, 2cy), the points H puts inside
 *              the query frame, plus the same count of the query's lattice in the reference frame.
 *   shortlist  references ranked by (overlap descending, index ascending), one below max(min_overlap, 1) never ranks, the first
 *              min(max_refs, ranked) taken and written in ASCENDING index.
 * ref_cams [15 n_ref], ref_R [9 n_ref] and prior_cams [15 n_query], prior_R [9 n_query]: the rotations are ptz_reloc_ref_rotations
 * of the respective cameras (one host function for both).  query_wh [2 n_query].  Outputs: shortlist [max_refs n_query] (-1 in unused
 * slots), n_short [n_query], overlap [n_query n_ref], H_slot [9 max_refs n_query] (H of each listed slot, zeros in unused ones).
 * A query's output depends on its own prior, its image size, the references and the options only.
 * ptz_reloc_prior_pairs (host arrays: upload, run, download; overlap, H_slot, device_ms may be NULL).  PTZ_EINVAL, before any device
 * work: negative extents, n_ref < 1 with queries, a missing array, an image size that is not positive, a prior camera with a
 * non-finite entry or a focal that is not positive, a radius that is not finite and positive, max_refs < 1, min_overlap outside
 * 0 .. 128; PTZ_EUNSUPPORTED: factor_type; PTZ_ELIMIT: more than 2^31 - 1 slots or scores; n_query = 0 is PTZ_OK.  opt = NULL: defaults.
 * ptz_reloc_prior_pairs_device: every array a DEVICE pointer on the device that owns d_shortlist, all of them required; enqueued
 * on `hip_stream`, returns without synchronising.  The cameras are not validated there (they live on the device). */
typedef struct ptz_prior_options {
  double radius_px;    /* 40: the guided matcher's radius under the predicted H (ptz_relocalizer_run_tracked) */
  int32_t max_refs;    /* 8: R, the most references a query keeps */
  int32_t min_overlap; /* 8, of 128 */
  int32_t reserved_;
} ptz_prior_options;
void ptz_prior_options_default(ptz_prior_options* o);
int32_t ptz_reloc_prior_pairs(int32_t n_ref, const double* ref_cams, const double* ref_R, int32_t n_query, const double* prior_cams,
                              const double* prior_R, const int32_t* query_wh, int32_t factor_type, const ptz_prior_options* opt,
                              int32_t device_id, int32_t* shortlist, int32_t* n_short, int32_t* overlap /* or NULL */,
                              double* H_slot /* or NULL */, double* device_ms /* or NULL */);
int32_t ptz_reloc_prior_pairs_device(int32_t n_ref, const double* d_ref_cams, const double* d_ref_R, int32_t n_query,
                                     const double* d_prior_cams, const double* d_prior_R, const int32_t* d_query_wh, int32_t factor_type,
                                     const ptz_prior_options* opt, int32_t* d_shortlist, int32_t* d_n_short, int32_t* d_overlap,
                                     double* d_H_slot, void* hip_stream);

/* ptz_relocalizer_run with a prior camera per query, prior_cams [15 n_query] on the host: no dense pass, no vote pass and no
 * per-pair RANSAC.  Stage 0 is ptz_reloc_prior_pairs_device of the priors against the resident references (the prior rotations
 * computed on the host); the host downloads the lists and builds the pair list as the shortlisted run does, query-major, a query's
 * references ascending; the H of each pair is gathered on the device and ptz_desc_match_pairs_guided_device runs with it, found =
 * NULL and prior_opt->radius_px IN PLACE of stages 1 and 2 (options->guided_radius is ignored); stage 3 is the assembly; then the
 * solve's initial camera takes the prior's focal, rotation and distortion (reloc_prior_camera); stages 4 - 6 are unchanged.
 * THE GATE ON THE ASSEMBLED QUERY (stage 4) IS FORCED ON, whatever options->inlier_matches says: within a radius of tens of pixels a
 * feature whose true partner is absent often has exactly one admissible candidate, which passes the ratio test (second = INT32_MAX)
 * and the cross check.  options->match.max_dist2, if set, comes on top.  stage_ms[0] is 0, stage_ms[1] the guided matcher's time.
 * prior_result (or NULL), every pointer nullable: shortlist [prior_opt->max_refs n_query], n_short, overlap [n_query n_ref], prior_ms
 * the device time of stage 0.  A query with n_short = 0 goes on as one with n_sel = 0; a lost query is one that is not accepted --
 * the caller's signal to fall back to ptz_relocalizer_run / _run_shortlisted.  To make it one signal, accepted[q] is also 0 for a query
 * the gate kept nothing of (the solve on no matches converges where it stands and would say 1).  With a radius of tens of pixels
 * min_inliers = 6 is weak evidence: a wrong prior's lone candidates agree with SOME homography in a dozen matches by chance; callers
 * that rely on the signal raise options->min_inliers to a fraction of what a true overlap yields (tens).  ptz_relocalizer_pairs / _table / _matches work as after
 * any run.  Known limits: gate_max_pair_matches (at most 4096) bounds an assembled query (gate_model = 0); H ignores distortion; an overlap list is
 * only as good as the prior. */
typedef struct ptz_prior_result {
  int32_t* shortlist;
  int32_t* n_short;
  int32_t* overlap;
  double prior_ms;
} ptz_prior_result;
int32_t ptz_relocalizer_run_tracked(ptz_relocalizer* r, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_wh,
                                    const double* prior_cams, const ptz_reloc_options* options, const ptz_prior_options* prior_opt,
                                    ptz_reloc_result* result, ptz_prior_result* prior_result);

/* ---- landmark map: relocalize against one ray and one descriptor per track --------------------------------------------------------
 * The references overlap, so a world point sits in the resident set once per view that saw it.  A landmark map holds it ONCE: per
 * track of the reference images a unit ray from the shared projection centre and an aggregated descriptor.  The contract is
 * csrc/ptz_landmark.h (integers, and + - * / sqrt in double rounded one by one; the references' rotations from
 * ptz_reloc_ref_rotations).
 * Map build.  ref_set: the references' resident set WITH key points, image m = camera m of ref_cams [15 n_ref]; tracks as CSR:
 * trk_ptr [n_track + 1], trk_img / trk_feat [trk_ptr[n_track]] (the feature's index inside its image); min_views >= 1.  Per track,
 * over its views in CSR order: a view is valid iff image and feature are in range and, for factor_type & 1, its undistorted pixel
 * lies inside its view's frame; ray_v = R_r^T n / |R_r^T n|; L = s / |s| with s the left-to-right sum of ray_v over the valid views;
 * the track is a landmark iff it has at least min_views valid views and L is finite; descriptor byte k = (2 S_k + n) / (2 n), S_k
 * the int32 sum of byte k over the n valid views; home = the reference of the valid view with the largest (R_r L)_z, the first in
 * CSR order on a tie.  Landmarks are compacted in ascending track order.
 * ptz_landmark_map_download, every pointer nullable: lm_track / lm_home / lm_views [n_lm], lm_ray [3 n_lm], lm_desc [n_lm D].
 * ptz_landmark_map_desc_set: the map's descriptors as a ptz_desc_set of ONE image of n_lm features (placeholder key points), the
 * map's until it is destroyed: what ptz_desc_match_pairs takes as set_a with img_a = 0.
 * PTZ_EINVAL, before any device work: NULL set / cameras / trk_ptr / out, n_ref < 1 or not the set's image count, n_track < 0,
 * offsets that do not start at 0 or decrease, views without trk_img / trk_feat, min_views < 1, a set with features but without key
 * points, device_id not the set's; PTZ_EUNSUPPORTED: factor_type; PTZ_ELIMIT: more than 8192 references (the anchor vote's LDS
 * counters).  Out-of-range images and features are not errors: such a view is not valid.
 * Assembly.  Pair q is (map, query q): match_ptr [n_query + 1], idx_a (landmark index) and uv_b (query pixel) in the layout of
 * ptz_desc_matches_device_ptrs.  A match votes for lm_home[idx_a]; the anchor of a query is the reference with the most votes, the
 * lowest index on a tie; without a vote anchor_ref = -1, the range is empty and the cameras are those of reference 0.  cam_ref is
 * the virtual anchor [fa, fa, S, S, rvec_a, t_a, 0 x 5] of ptz_reloc_assemble (K > 1), cam_cur its cam_cur.  Each match is
 * transferred as m = R_a L, kept iff m_z > 0, m finite and the pixel (float)(fa m_x / m_z + S), .. lies in [0, 2S)^2.  Outputs in
 * the layout of ptz_reloc_assemble: anchor_ref [n_query], out_ptr [n_query + 1], out_uv_ref / out_uv_cur [n_match, 2], out_src
 * [n_match] of which the first out_ptr[n_query] entries are written, cam_ref / cam_cur [15 n_query].  A query's output depends on
 * its own matches and the map only.  ref_cams / ref_R: those the map was built with (ref_R from ptz_reloc_ref_rotations).
 * ptz_landmark_assemble (host arrays).  PTZ_EINVAL, before any device work: NULL map, n_query < 0, offsets that do not start at 0
 * or decrease, idx_a outside [0, n_lm), missing arrays, an image size that is not positive; PTZ_EUNSUPPORTED: factor_type;
 * PTZ_ELIMIT: more than 2^31 - 1 matches; n_query = 0 is PTZ_OK.
 * ptz_landmark_assemble_device: DEVICE pointers on the map's device, enqueued on `hip_stream`, no synchronisation inside.  Nothing
 * on the device is validated: a malformed range is an empty one, a match whose landmark is out of range neither votes nor is
 * kept.  d_workspace: 256-byte aligned, at least ptz_landmark_assemble_workspace_bytes(n_query, n_match) bytes, the caller's until
 * the stream has run the call; whatever it holds before is never read.
 * ptz_relocalizer_run_landmarks: stage 1 is ptz_desc_match_pairs over the n_query (map, query) pairs, stage 3 the landmark
 * assembly, stages 4 - 6 exactly ptz_relocalizer_run's; options->max_refs is ignored: sel_ref is [n_query], sel_ref[q] the anchor
 * (-1 without one), n_sel 0 or 1.  The map must come from the relocalizer's references, device and D: the count of references, the
 * device and D are checked (PTZ_EINVAL); that the map was built from the SAME cameras is not -- the assembly reads the
 * relocalizer's cameras, and a map built from others with the same count gives wrong pixels silently.  guided_radius > 0 is
 * PTZ_EUNSUPPORTED: there is no pair homography between a map and an image.  ptz_relocalizer_table / _matches / _pairs work as
 * after any run (pair_ref is the map's image, 0). */
typedef struct ptz_landmark_map ptz_landmark_map;
int32_t ptz_landmark_map_create(const ptz_desc_set* ref_set, const double* ref_cams, int32_t n_ref, int32_t n_track, const int64_t* trk_ptr,
                                const int32_t* trk_img, const int32_t* trk_feat, int32_t factor_type, int32_t min_views, int32_t device_id,
                                ptz_landmark_map** out);
void ptz_landmark_map_destroy(ptz_landmark_map* m);
int32_t ptz_landmark_map_n_landmarks(const ptz_landmark_map* m);
double ptz_landmark_map_build_ms(const ptz_landmark_map* m); /* the build's launches, between events on the call's stream */
int32_t ptz_landmark_map_download(const ptz_landmark_map* m, int32_t* lm_track, double* lm_ray, int32_t* lm_home, int32_t* lm_views,
                                  uint8_t* lm_desc);
const ptz_desc_set* ptz_landmark_map_desc_set(const ptz_landmark_map* m);
int64_t ptz_landmark_assemble_workspace_bytes(int32_t n_query, int64_t n_match);
int32_t ptz_landmark_assemble(const ptz_landmark_map* map, int32_t n_query, const int64_t* match_ptr, const int32_t* idx_a, const float* uv_b,
                              const double* ref_cams, const double* ref_R, const int32_t* query_wh, int32_t factor_type, int32_t* anchor_ref,
                              int64_t* out_ptr, float* out_uv_ref, float* out_uv_cur, int32_t* out_src, double* cam_ref, double* cam_cur,
                              double* device_ms /* or NULL */);
int32_t ptz_landmark_assemble_device(const ptz_landmark_map* map, int32_t n_query, int64_t n_match, const int64_t* d_match_ptr,
                                     const int32_t* d_idx_a, const float* d_uv_b, const double* d_ref_cams, const double* d_ref_R,
                                     const int32_t* d_query_wh, int32_t factor_type, int32_t* d_anchor_ref, int64_t* d_out_ptr,
                                     float* d_out_uv_ref, float* d_out_uv_cur, int32_t* d_out_src, double* d_cam_ref, double* d_cam_cur,
                                     void* d_workspace, int64_t workspace_bytes, void* hip_stream);
int32_t ptz_relocalizer_run_landmarks(ptz_relocalizer* r, const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query,
                                      const int32_t* query_wh, const ptz_reloc_options* options, ptz_reloc_result* result);

/* ---- landmark view: relocalize against the map from a prior camera -----------------------------------------------------------------
 * A landmark is a unit ray L from the shared centre, so under a prior (K_q, R_q) its pixel in the query is K_q R_q L: no homography,
 * no reference image, no reference-side distortion.  The contract is csrc/ptz_landmark_prior.h (+ - * / in double rounded one by
 * one; prior_R [9 n_query] is ptz_reloc_ref_rotations of prior_cams [15 n_query]).
 * Prediction: m = R_q L, rows summed left to right; ok = m_z > 0 and m finite; px = fx (m_x / m_z) + 0.5 w, py = fy (m_y / m_z) +
 * 0.5 h, fx the prior's and fy = fx for F / FDist, the prior's fy otherwise.  The prior's distortion does not enter.
 * Visibility: ok, -radius_px <= px < w + radius_px and -radius_px <= py < h + radius_px, on the doubles; position ((float)px,
 * (float)py).  The VIEW of query q is its visible landmarks in ascending landmark index: vis_ptr [n_query + 1], vis_lm [n_vis],
 * vis_uv [n_vis, 2].  It depends on the query's own prior, its image size and the map only.
 * ptz_landmark_visible (host arrays) builds the view and gathers the packed descriptor rows of the visible landmarks into a
 * ptz_desc_set of n_query images whose key points are vis_uv (ptz_landmark_view_desc_set, the view's until it is destroyed): the
 * guided matcher over the pairs (view image q, query image q) under H = identity and radius_px gives the matches of (map, q), idx_a
 * view-local (the landmark is vis_lm[vis_ptr[q] + idx_a]).  The host reads vis_ptr once, to size the set.
 * PTZ_EINVAL, before any device work: NULL map / out, n_query < 0, missing arrays, an image size that is not positive, a prior
 * with a non-finite entry or a focal that is not positive, a radius that is not finite and positive, max_view_bytes < 1;
 * PTZ_EUNSUPPORTED: factor_type; PTZ_ELIMIT: a view whose set needs more than max_view_bytes or 2^31 - 1 rows -- the caller splits
 * the batch; n_query = 0 is PTZ_OK with an empty view.  opt = NULL: defaults.
 * ptz_landmark_view_download / _device_ptrs: every pointer nullable.  ptz_landmark_view_device_ms: the launches of both passes.
 * ptz_landmark_visible_device: raw DEVICE pointers on the device that owns d_vis_ptr, enqueued on `hip_stream`, no synchronisation;
 * d_ray [3 n_lm] are arbitrary rays, nothing is validated.  d_vis_ptr [n_query + 1] is always complete; of d_vis_lm / d_vis_uv at
 * most `capacity` entries are written.  d_workspace: 256-byte aligned, at least ptz_landmark_visible_workspace_bytes(n_lm, n_query)
 * bytes; whatever it holds before is never read.  PTZ_ELIMIT: n_query x ceil(n_lm / 1024) above 2^31 - 1.
 * ptz_relocalizer_run_landmarks_tracked is ptz_relocalizer_run_landmarks with three differences: stage 0 builds the view from
 * prior_cams (lp_opt->radius_px; the prior rotations computed on the host); stage 1 is the guided matcher
 * (options->guided_grid selects the kernel) over the pairs (view image q, query q) under identity H, and its idx_a is lifted to
 * landmark indices by a small kernel before ptz_landmark_assemble_device; the solve starts from reloc_prior_camera.  As in
 * ptz_relocalizer_run_tracked THE GATE ON THE ASSEMBLED QUERY IS FORCED ON and accepted[q] is 0 for a query the gate kept nothing
 * of.  options->guided_radius is ignored.  stage_ms[0] is the view's device time, stage_ms[1] the matcher's.  view_result (or
 * NULL), pointers nullable: n_visible [n_query], view_ms.  ptz_relocalizer_table returns the matcher's table: idx_a is view-local,
 * uv_a the predicted pixel.  ptz_relocalizer_view downloads the last such run's view (every pointer nullable; PTZ_EINVAL when the
 * last run was neither a tracked nor a shortlisted landmark run).  Validation is that of the two runs it combines.  Known limits: the prior's distortion is
 * ignored in the prediction; max_view_bytes; gate_max_pair_matches still bounds an assembled query (gate_model = 0); a view is only as good as the
 * prior. */
typedef struct ptz_landmark_prior_options {
  double radius_px;       /* 40: the margin of the visibility rule and the guided matcher's radius */
  int64_t max_view_bytes; /* 2 GiB: the most a view's gathered set may take on the device */
} ptz_landmark_prior_options;
void ptz_landmark_prior_options_default(ptz_landmark_prior_options* o);
typedef struct ptz_landmark_view ptz_landmark_view;
int32_t ptz_landmark_visible(const ptz_landmark_map* map, int32_t n_query, const double* prior_cams, const double* prior_R,
                             const int32_t* query_wh, int32_t factor_type, const ptz_landmark_prior_options* opt, ptz_landmark_view** out);
void ptz_landmark_view_destroy(ptz_landmark_view* v);
int64_t ptz_landmark_view_n_visible(const ptz_landmark_view* v);
int32_t ptz_landmark_view_download(const ptz_landmark_view* v, int64_t* vis_ptr, int32_t* vis_lm, float* vis_uv);
const ptz_desc_set* ptz_landmark_view_desc_set(const ptz_landmark_view* v);
int32_t ptz_landmark_view_device_ptrs(const ptz_landmark_view* v, const int64_t** d_vis_ptr, const int32_t** d_vis_lm, const float** d_vis_uv);
double ptz_landmark_view_device_ms(const ptz_landmark_view* v);
int64_t ptz_landmark_visible_workspace_bytes(int32_t n_lm, int32_t n_query);
int32_t ptz_landmark_visible_device(int32_t n_lm, const double* d_ray, int32_t n_query, const double* d_prior_cams, const double* d_prior_R,
                                    const int32_t* d_query_wh, int32_t factor_type, double radius_px, int64_t* d_vis_ptr, int32_t* d_vis_lm,
                                    float* d_vis_uv, int64_t capacity, void* d_workspace, int64_t workspace_bytes, void* hip_stream);
typedef struct ptz_landmark_view_result {
  int32_t* n_visible;
  double view_ms;
} ptz_landmark_view_result;
int32_t ptz_relocalizer_run_landmarks_tracked(ptz_relocalizer* r, const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query,
                                              const int32_t* query_wh, const double* prior_cams, const ptz_reloc_options* options,
                                              const ptz_landmark_prior_options* lp_opt, ptz_reloc_result* result,
                                              ptz_landmark_view_result* view_result);
int32_t ptz_relocalizer_view(const ptz_relocalizer* r, int64_t* n_visible, int64_t* vis_ptr, int32_t* vis_lm, float* vis_uv);

/* ---- landmark shortlist: relocalize against the map through probe votes for its cells ----------------------------------------------
 * Without a prior the landmark run matches every query feature against every landmark.  The map already holds a partition to vote
 * over: a landmark's HOME is the reference whose optical axis is nearest its ray, a cell of the view sphere.  The contract is
 * csrc/ptz_landmark_shortlist.h, all integer, on top of csrc/ptz_desc_shortlist.h:
 *   home set   the landmarks grouped by home: image r of a ptz_desc_set of n_ref images holds the landmarks with home == r in
 *              ascending landmark index (home_ptr [n_ref + 1], home_lm [n_lm]); a reference that is home of nothing is an empty
 *              image.  ptz_landmark_map_home_set builds it from the map's host copies on the first request (NULL if that fails);
 *              the map owns it.  ptz_landmark_map_home_groups downloads the grouping (pointers nullable).
 *   votes      ptz_landmark_shortlist / _device / _workspace_bytes ARE ptz_desc_shortlist / _device / _workspace_bytes with the home
 *              set as the reference set: the same kernels, arguments, errors and outputs (shortlist [max_refs n_query] of home
 *              indices in ascending order, -1 in unused slots; n_short; votes [n_query n_ref]).
 *   view       the view of query q is every landmark whose home is on q's list, in ascending landmark index (a tie in the matcher
 *              resolves to the lowest landmark, as in the dense run); a home listed twice counts once.
 *              ptz_landmark_view_from_homes (host lists [R n_query]; an entry outside [0, n_ref) other than -1 is PTZ_EINVAL) and
 *              ptz_landmark_view_from_homes_device (a DEVICE list on the map's device, written on `hip_stream` or already complete;
 *              such an entry is ignored) return a ptz_landmark_view of kind PTZ_LANDMARK_VIEW_HOMES: vis_ptr and vis_lm as for the
 *              prior's view, a gathered set of n_query images whose key points -- and vis_uv -- are zeros, as the map's own set's.
 *              Both wait for the stream: the host reads vis_ptr once, to size the set.  PTZ_ELIMIT: a set beyond max_view_bytes or
 *              2^31 - 1 rows, more than 2^31 - 1 list slots or (query, tile) cells.  R >= 1; n_query = 0 is an empty view.
 *   matches    ptz_desc_match_pairs over the pairs (view image q, query image q); idx_a is view-local, the landmark is
 *              vis_lm[vis_ptr[q] + idx_a].  A list that names every non-empty home makes the view the whole map in order, and the
 *              matches are those of the pairs (map, query q), array for array.
 * ptz_relocalizer_run_landmarks_shortlisted is ptz_relocalizer_run_landmarks with a stage 0 in front: 0a the vote pass on the
 * device (options->match's ratio and max_dist2, sl_opt; the lists are not downloaded for the run's own use), 0b the view from the
 * device lists (at most the default max_view_bytes of ptz_landmark_prior_options); stage 1 is the DENSE matcher over (view q,
 * query q) with its ratio test and cross check, its idx_a lifted to landmark indices in front of ptz_landmark_assemble_device; the
 * rest is the landmark run's.  The gate is NOT forced on.  guided_radius > 0 is PTZ_EUNSUPPORTED.  A query with n_short = 0 has an
 * empty view and no anchor (n_sel = 0).  stage_ms[0] is the matcher's; sl_result (or NULL, pointers nullable): shortlist
 * [sl_opt->max_refs n_query], n_short, votes [n_query n_ref], shortlist_ms the vote pass; view_result (or NULL): n_visible, view_ms.
 * ptz_relocalizer_view downloads the run's view, ptz_relocalizer_table its view-local table.  Validation is that of
 * ptz_relocalizer_run_landmarks and ptz_desc_shortlist_device. */
#define PTZ_LANDMARK_VIEW_PRIOR 0
#define PTZ_LANDMARK_VIEW_HOMES 1
const ptz_desc_set* ptz_landmark_map_home_set(const ptz_landmark_map* map);
int32_t ptz_landmark_map_home_groups(const ptz_landmark_map* map, int64_t* home_ptr, int32_t* home_lm);
int32_t ptz_landmark_shortlist(const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_img,
                               const ptz_desc_options* desc_opt, const ptz_shortlist_options* sl_opt, int32_t* shortlist, int32_t* n_short,
                               int32_t* votes /* or NULL */, double* device_ms /* or NULL */);
int64_t ptz_landmark_shortlist_workspace_bytes(const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query,
                                               const ptz_shortlist_options* sl_opt);
int32_t ptz_landmark_shortlist_device(const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query,
                                      const int32_t* d_query_img /* or NULL */, const ptz_desc_options* desc_opt,
                                      const ptz_shortlist_options* sl_opt, int32_t* d_shortlist, int32_t* d_n_short,
                                      int32_t* d_votes /* or NULL */, void* d_workspace, int64_t workspace_bytes, void* hip_stream);
int32_t ptz_landmark_view_from_homes(const ptz_landmark_map* map, int32_t n_query, int32_t max_refs, const int32_t* shortlist,
                                     int64_t max_view_bytes, ptz_landmark_view** out);
int32_t ptz_landmark_view_from_homes_device(const ptz_landmark_map* map, int32_t n_query, int32_t max_refs, const int32_t* d_shortlist,
                                            int64_t max_view_bytes, void* hip_stream, ptz_landmark_view** out);
int32_t ptz_landmark_view_kind(const ptz_landmark_view* v);
int32_t ptz_relocalizer_run_landmarks_shortlisted(ptz_relocalizer* r, const ptz_landmark_map* map, const ptz_desc_set* query_set,
                                                  int32_t n_query, const int32_t* query_wh, const ptz_reloc_options* options,
                                                  const ptz_shortlist_options* sl_opt, ptz_reloc_result* result,
                                                  ptz_shortlist_result* sl_result, ptz_landmark_view_result* view_result);

/* ---- feature tracks on the device: connected components of the match table ---------------------------------------------------------
 * The tracks the landmark map is built from, without the host: the matches of a set of images among themselves are the edges of a
 * graph over the features, a track is a connected component that holds no image twice.  The contract is csrc/ptz_tracks.h, all
 * integer:
 *   node       feature `feat` of image `img` is node feat_ptr[img] + feat (image-major); fewer than 2^31 features in all (PTZ_ELIMIT)
 *   edge       match m of pair p, match_ptr[p] <= m < match_ptr[p + 1]: (img_a[p], idx_a[m]) - (img_b[p], idx_b[m]), the layout of
 *              ptz_desc_matches.  Duplicate edges, a pair listed twice or reversed, img_a == img_b and an edge from a node to itself
 *              are all allowed.
 *   label      of a matched node: the smallest node of its connected component.  Unmatched features belong to nothing.
 *   track      a component in which no image occurs twice and that has at least min_len nodes (min_len >= 2, else PTZ_EINVAL):
 *              what Build + Filter(min_len) + ExportFlat of host/tracks.cc keep
 *   order      tracks in ascending label, the views of a track in ascending node, which is ascending image
 *   outputs    trk_ptr [n_track + 1]; per view trk_img, trk_feat, trk_node, trk_uv (the set's key point of the node; zeros where
 *              there are none); counts [4]: matched nodes, components, components dropped for a repeated image, components dropped
 *              as short (a component with both defects counts as repeated)
 * The result depends on the SET of edges only: not on the order of pairs or matches, on which side of a pair is a, on the launch
 * shape or on the run.  As arrays it equals the host builder's tracks sorted by the node of their first view.
 * ptz_tracks_build (host arrays: upload, run).  PTZ_EINVAL, before any device work: NULL out / feat_ptr, n_img < 0, feat_ptr that
 * does not start at 0 or decreases, n_pair < 0, match_ptr that does not start at 0 or decreases, missing arrays, an image or a
 * feature index out of range, min_len < 2, device_id < 0; PTZ_ELIMIT: 2^31 features or matches and above.
 * ptz_tracks_from_matches: the resident form, for the table of ptz_desc_match_pairs(set, set, ...) over the pairs (img_a[p],
 * img_b[p]) -- HOST arrays of the table's n_pair, uploaded; everything else is read where it lies (the table's device arrays, the
 * set's offsets and key points) and nothing is downloaded but the sizes, the counts and the error word.  PTZ_EINVAL: NULL
 * arguments, a table of another device, an image out of range, min_len < 2.
 * ptz_tracks_build_device: raw DEVICE pointers on the device that owns d_trk_ptr, enqueued on `hip_stream`, no synchronisation
 * inside.  d_feat_ptr [n_img + 1] and n_feat = its last entry (the host's copy); d_kp [n_feat] float2 or NULL.  Nothing on the
 * device is validated: an edge with an image or a feature out of range is ignored.  Outputs: d_trk_ptr with room for n_feat / 2 +
 * 2 entries; d_trk_img / d_trk_feat / d_trk_node with room for n_feat entries and d_trk_uv for 2 n_feat (or NULL); d_sizes [8]
 * int64: n_track, n_view, the four counts, the error word (non-zero: PTZ_EINTERNAL for the caller to report), 0.  d_workspace:
 * 256-byte aligned, at least ptz_tracks_workspace_bytes(n_feat) bytes; whatever it holds before is never read.
 * PTZ_EINTERNAL: a walk up a parent chain or a retry loop reached its cap of n_feat steps.  Every loop of every kernel is
 * bounded and no kernel waits for another workgroup, so a bug ends as this code.
 * ptz_tracks_download / _device_ptrs: every pointer nullable.  ptz_tracks_device_ms: the launches, between events.
 * ptz_landmark_map_create_from_tracks is ptz_landmark_map_create on the tracks' device (the set's), the three track arrays copied
 * device to device instead of uploaded: the same launches, the same map.  lm_track indexes the device's track order.
 * Known limits: tracks are rebuilt from the whole table every time; the bundle adjustment is not fed from device tracks (its
 * observation order follows the track order). */
typedef struct ptz_tracks ptz_tracks;
int32_t ptz_tracks_build(int32_t n_img, const int64_t* feat_ptr, int32_t n_pair, const int32_t* img_a, const int32_t* img_b,
                         const int64_t* match_ptr, const int32_t* idx_a, const int32_t* idx_b, int32_t min_len, int32_t device_id,
                         ptz_tracks** out);
int32_t ptz_tracks_from_matches(const ptz_desc_set* set, const ptz_desc_matches* matches, const int32_t* img_a, const int32_t* img_b,
                                int32_t min_len, ptz_tracks** out);
int64_t ptz_tracks_workspace_bytes(int64_t n_feat);
int32_t ptz_tracks_build_device(int32_t n_img, const int64_t* d_feat_ptr, int64_t n_feat, const float* d_kp /* or NULL */, int32_t n_pair,
                                const int32_t* d_img_a, const int32_t* d_img_b, const int64_t* d_match_ptr, int64_t n_match,
                                const int32_t* d_idx_a, const int32_t* d_idx_b, int32_t min_len, int64_t* d_trk_ptr, int32_t* d_trk_img,
                                int32_t* d_trk_feat, int32_t* d_trk_node, float* d_trk_uv /* or NULL */, int64_t* d_sizes,
                                void* d_workspace, int64_t workspace_bytes, void* hip_stream);
void ptz_tracks_destroy(ptz_tracks* t);
int32_t ptz_tracks_n_tracks(const ptz_tracks* t);
int64_t ptz_tracks_n_views(const ptz_tracks* t);
int32_t ptz_tracks_counts(const ptz_tracks* t, int64_t* counts /* [4] */);
int32_t ptz_tracks_download(const ptz_tracks* t, int64_t* trk_ptr, int32_t* trk_img, int32_t* trk_feat, int32_t* trk_node, float* trk_uv);
int32_t ptz_tracks_device_ptrs(const ptz_tracks* t, const int64_t** d_trk_ptr, const int32_t** d_trk_img, const int32_t** d_trk_feat,
                               const int32_t** d_trk_node, const float** d_trk_uv);
double ptz_tracks_device_ms(const ptz_tracks* t);
int32_t ptz_landmark_map_create_from_tracks(const ptz_desc_set* ref_set, const double* ref_cams, int32_t n_ref, const ptz_tracks* tracks,
                                            int32_t factor_type, int32_t min_views, ptz_landmark_map** out);

#ifdef __cplusplus
}
#endif
#endif /* PTZ_CALIB_AMD_H */
