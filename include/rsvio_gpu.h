/*
 * rsvio_gpu.h -- C ABI of the MI355X (gfx950) implementation of RS-VIO's two hot paths.
 *
 * The reference (EthanD11/RS-VIO) is a pure-Rust crate with no FFI layer; its drop-in
 * boundary is the Rust API the estimator calls.  Every entry point below names the
 * reference item it replaces (file:line under the reference root).  INTEGRATION.md
 * shows the `extern "C"` block and safe wrapper a Rust maintainer binds to it.
 *
 * Conventions
 *  - Every function returns int: RSVIO_OK (0) or a negative RSVIO_ERR_* code;
 *    rsvio_last_error() returns a thread-local message.  Nothing aborts or unwinds.
 *  - Per-feature failure is valid = 0 (the reference's Option::None / false).
 *  - Host buffers are borrowed for the duration of the call only.  Device memory is
 *    owned by the handle and released by *_destroy.
 *  - A handle is single-threaded (mirrors `&mut self`); distinct handles may run
 *    concurrently on distinct HIP streams.
 *  - Affine2<f32> state is float[6] = {m11, m12, m21, m22, m13, m23}.
 *  - Pyramids are packed: level i is (w >> i) x (h >> i) u8, levels back to back.
 *  - SE3 poses are 7-vectors {tx, ty, tz, qw, qx, qy, qz} of T_B_W
 *    (src/estimator/sliding_window.rs:222-224).
 */
#ifndef RSVIO_GPU_H
#define RSVIO_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    RSVIO_OK = 0,
    RSVIO_ERR_INVALID_ARG = -1,
    RSVIO_ERR_HIP = -2,
    RSVIO_ERR_NOMEM = -3,
    RSVIO_ERR_CAPACITY = -4,
    RSVIO_ERR_NO_DEVICE = -5,
    RSVIO_ERR_INTERNAL = -6,
    RSVIO_ERR_RCCL = -7
};

/* Thread-local message for the last failing call on this thread. */
const char* rsvio_last_error(void);
/* Library / device identification; returns RSVIO_ERR_NO_DEVICE if no gfx950 is visible. */
int rsvio_device_info(int device, char* name_out, size_t cap, int* n_cus);

/* HIP stream (hipStream_t) for the device-pointer entry points and rsvio_ba_set_stream.
 * cu_mask (mask_words x 32 bits, bit i = CU i; NULL = all CUs) restricts the stream's kernels
 * to a CU subset, so the tracker and the BA of one process can run side by side on disjoint
 * CUs (hipExtStreamCreateWithCUMask).  No reference counterpart (the reference is CPU-only). */
int rsvio_stream_create(int32_t device, const uint32_t* cu_mask, uint32_t mask_words, void** out);
int rsvio_stream_destroy(void* stream);
/* Host-to-device copy of page-locked host memory (hipHostMalloc / hipHostRegister) by a kernel on
 * `stream` instead of a copy engine: the next kernel on the stream starts without the copy-engine ->
 * compute-queue hand-off (how bench.py's protocol step uploads the frame's images).  A pageable or
 * non-16-byte-aligned source or destination takes hipMemcpyAsync.  As with hipMemcpyAsync, the source
 * must stay valid and unchanged until the stream has passed the copy.  No reference counterpart. */
int rsvio_upload_async(void* d_dst, const void* h_src, size_t bytes, void* stream);

/* =============================== HP-T: patch tracker =============================== */

typedef struct {
    int32_t width, height;
    int32_t levels;                 /* StereoPatchTracker<LEVELS> (estimator.rs:27 uses 6) */
    int32_t grid_size;              /* config/euroc_vio.yaml:42 */
    int32_t max_iterations;         /* optical_flow_max_iterations (:44) */
    float convergence_threshold;    /* optical_flow_convergence_threshold (:45), f64->f32 (feature_tracker.rs:112) */
    int32_t device;
    int32_t max_features;           /* per-camera capacity of the track maps (0 -> 4096) */
} rsvio_tracker_params;

/* One tracked point: id + Affine2 state (pixel position = m13, m23). */
typedef struct {
    uint64_t id;
    float x, y;       /* m13, m23 */
    float r[4];       /* m11, m12, m21, m22 */
} rsvio_feature;

typedef struct rsvio_tracker rsvio_tracker;

/* StereoPatchTracker::<N>::new(grid_size, max_iters, thresh)  (src/feature_tracker/feature_tracker.rs:103-114) */
int rsvio_tracker_create(const rsvio_tracker_params* params, rsvio_tracker** out);
void rsvio_tracker_destroy(rsvio_tracker* t);

/* StereoPatchTracker::process_frame(&mut self, &GrayImage, &GrayImage, &mut Frame) (:116-187)
 * followed by get_track_points (:188-200).  Images are u8, row stride `stride` bytes.
 * Outputs are sorted by ascending id (canonical order; the reference iterates HashMaps).
 * New ids are assigned in detection scan order (image_utilities.rs:141-142).
 * RSVIO_ERR_CAPACITY (lists still consistent and returned) when the frame's new points exceed
 * max_features -- both cameras then admit the same leading new points and the rest are dropped
 * -- or when cap_l / cap_r truncated a list. */
int rsvio_tracker_process_frame(rsvio_tracker* t, const uint8_t* left, const uint8_t* right,
                                size_t stride, rsvio_feature* out_l, size_t cap_l, size_t* n_l,
                                rsvio_feature* out_r, size_t cap_r, size_t* n_r);
/* Same, with both images already in device memory (tightly packed w x h). */
int rsvio_tracker_process_frame_device(rsvio_tracker* t, const uint8_t* d_left,
                                       const uint8_t* d_right, rsvio_feature* out_l,
                                       size_t cap_l, size_t* n_l, rsvio_feature* out_r,
                                       size_t cap_r, size_t* n_r);
/* process_frame in two halves, for a caller that runs one frame ahead (the Estimator's look-ahead:
 * estimator.rs:190 passes the tracker only the two images, so frame t+1 can be tracked while frame
 * t's motion tracking and BA run).  submit enqueues the frame (pyramids, LK, FAST, packing and the
 * read-back of its lists) and returns at once; collect waits for it and fills the lists exactly as
 * process_frame does.  One frame in flight per handle: process_frame*, submit*, remove_ids and
 * set_cameras refuse (RSVIO_ERR_INVALID_ARG) while one is, collect refuses when none is.  Host
 * images (rsvio_tracker_submit) are borrowed until collect returns.  Consumers of the last
 * collected frame (rsvio_tracker_undistorted, rsvio_track_motion_tracker) keep reading THAT frame
 * after a later submit: frames alternate between two device output slots. */
int rsvio_tracker_submit(rsvio_tracker* t, const uint8_t* left, const uint8_t* right, size_t stride);
int rsvio_tracker_submit_device(rsvio_tracker* t, const uint8_t* d_left, const uint8_t* d_right);
int rsvio_tracker_collect(rsvio_tracker* t, rsvio_feature* out_l, size_t cap_l, size_t* n_l,
                          rsvio_feature* out_r, size_t cap_r, size_t* n_r);
/* StereoPatchTracker::remove_id (:201-206) */
int rsvio_tracker_remove_ids(rsvio_tracker* t, const uint64_t* ids, size_t n);
/* HIP stream the tracker enqueues on (hipStream_t) */
void* rsvio_tracker_stream(rsvio_tracker* t);

/* ---- parity-level entry points (host buffers in/out) ---- */

size_t rsvio_pyramid_bytes(int32_t w, int32_t h, int32_t levels);
/* build_image_pyramid (feature_tracker.rs:209-220): imageops::resize Triangle per level */
int rsvio_build_pyramid(const uint8_t* img, int32_t w, int32_t h, int32_t levels, uint8_t* out);
/* track_points (feature_tracker.rs:252-291): forward, backward and ||dt||^2 < 0.4 per feature.
 * aff_out receives the forward result for valid features (aff_in copied otherwise). */
int rsvio_track_points(const uint8_t* pyr0, const uint8_t* pyr1, int32_t w, int32_t h,
                       int32_t levels, const float* aff_in, int32_t n, int32_t max_iterations,
                       float thresh, float* aff_out, uint8_t* valid_out);
/* rsvio_track_points with the search of feature i started at seeds[i] (n x 2 f32 pixels of the second
 * image) instead of its own position -- motion-predicted tracking, see rsvio_tracker_set_prediction
 * for the rule.  A non-finite seed is replaced by the feature's own position; with every seed equal
 * to its feature's position the results are rsvio_track_points' bit for bit.  Same contract
 * otherwise (host buffers; n = 0 is allowed). */
int rsvio_track_points_seeded(const uint8_t* pyr0, const uint8_t* pyr1, int32_t w, int32_t h,
                              int32_t levels, const float* aff_in, const float* seeds, int32_t n,
                              int32_t max_iterations, float thresh, float* aff_out, uint8_t* valid_out);
/* detect_key_points(img, grid, current, 1) (image_utilities.rs:108-175) with the existing
 * tracks' positions (rounded as feature_tracker.rs:232-233).  out_xy: u32 (x, y) pairs. */
int rsvio_detect_keypoints(const uint8_t* img, int32_t w, int32_t h, int32_t grid,
                           const float* existing_xy, int32_t n_existing, uint32_t* out_xy,
                           float* out_score, int32_t cap, int32_t* n_out);

/* ---- device-pointer entry points (enqueue on `stream`, no synchronisation) ---- */
typedef struct rsvio_track_ctx rsvio_track_ctx;
/* Holds the per-(w,h,levels) resampling tables on device. */
int rsvio_track_ctx_create(int32_t w, int32_t h, int32_t levels, int32_t device, rsvio_track_ctx** out);
void rsvio_track_ctx_destroy(rsvio_track_ctx* c);
/* n_img images (each w x h, packed) -> n_img pyramids (each rsvio_pyramid_bytes, packed) */
int rsvio_build_pyramids_d(rsvio_track_ctx* c, const uint8_t* d_imgs, int32_t n_img,
                           uint8_t* d_pyrs, void* stream);
/* Up to 4 independent track_points batches in one launch. */
typedef struct {
    const uint8_t* d_pyr0;
    const uint8_t* d_pyr1;
    const float* d_aff_in;
    float* d_aff_out;
    uint8_t* d_valid;
    int32_t n;
} rsvio_track_batch;
int rsvio_track_points_d(rsvio_track_ctx* c, const rsvio_track_batch* batches, int32_t n_batches,
                         int32_t max_iterations, float thresh, void* stream);
/* Batched serving mode: any number of independent track_points batches (e.g. 3 per stereo
 * stream for many streams) in one launch.  d_table: n_batches descriptors in DEVICE memory;
 * d_start: n_batches + 1 int32 prefix sums of their sizes in device memory (d_start[0] = 0);
 * total = d_start[n_batches], given on the host for the grid size.  Same per-feature results as
 * rsvio_track_points_d (feature_tracker.rs:252-291). */
int rsvio_track_points_table_d(rsvio_track_ctx* c, const rsvio_track_batch* d_table, const int32_t* d_start,
                               int32_t n_batches, int32_t total, int32_t max_iterations, float thresh,
                               void* stream);

/* ====== T-sec: the feature_tracker/ crate (FeatureTracker, bicubic LK + Shi-Tomasi) ====== */

/* FeatureTrackingConfig (feature_tracker/src/feature_tracker.rs:25-38; defaults
 * feature_tracker/config/config.yaml) + image size, matching cost, device and capacity. */
enum { RSVIO_FT_SSD = 0, RSVIO_FT_LSSD = 1 };   /* MatchingCost (patch.rs:6-9) */
typedef struct {
    int32_t width, height;
    int32_t nlevels;                  /* 5 */
    int32_t preprocessing_blur;       /* 1 */
    double ratio;                     /* 2.0 */
    float preprocessing_blur_sigma;   /* 2.0 */
    float detection_threshold;        /* 2.5 */
    uint32_t detection_min_dist;      /* 15 */
    float detection_blur;             /* 6.0 */
    int32_t optical_flow_max_iter;    /* 25 */
    float optical_flow_lm_lambda;     /* 0.1 */
    int32_t matching_cost;            /* RSVIO_FT_SSD: what process_frame uses (feature_tracker.rs:125) */
    int32_t device;
    int32_t max_features;             /* capacity of the frame's feature list (0 -> 8192) */
    int32_t reserved;
} rsvio_ft_config;                    /* 64 bytes */

/* Feature (feature_tracker.rs:41-48): id + central point */
typedef struct {
    uint64_t feature_id;
    float x, y;
} rsvio_ft_feature;                   /* 16 bytes */

typedef struct rsvio_ft rsvio_ft;

/* FeatureTracker::new(config, None) (feature_tracker.rs:59-69) */
int rsvio_ft_create(const rsvio_ft_config* cfg, rsvio_ft** out);
void rsvio_ft_destroy(rsvio_ft* t);
/* FeatureTracker::process_frame(&FloatGrayImage, Frame) (:77-185): img is f32 luma in [0, 1]
 * (to_luma32f), row stride in floats (0 = width).  out receives frame.features: the previous
 * frame's features that track (previous order, positions transform * centre), then the new
 * Shi-Tomasi corners in (y, x) order with consecutive ids.  RSVIO_ERR_CAPACITY when the list
 * exceeds max_features (the list is truncated). */
int rsvio_ft_process_frame(rsvio_ft* t, const float* img, size_t stride, rsvio_ft_feature* out, size_t cap,
                           size_t* n);
/* Same with the image already in device memory (tightly packed). */
int rsvio_ft_process_frame_device(rsvio_ft* t, const float* d_img, rsvio_ft_feature* out, size_t cap, size_t* n);
/* FeatureTracker::get_pyramid (:190-193): the last frame's packed pyramid (rsvio_ft_pyramid_floats) */
int rsvio_ft_get_pyramid(rsvio_ft* t, float* out, size_t cap_floats);
void* rsvio_ft_stream(rsvio_ft* t);

/* ---- parity-level entry points (host buffers in/out, current device) ---- */
/* packed size of build_image_pyramid's output: level l = round(w / ratio^l) x round(h / ratio^l) */
size_t rsvio_ft_pyramid_floats(int32_t w, int32_t h, int32_t nlevels, double ratio);
/* build_image_pyramid (image_operations.rs:47-78) */
int rsvio_ft_build_pyramid(const float* img, int32_t w, int32_t h, int32_t nlevels, double ratio, int32_t blur,
                           float sigma, float* out);
/* feature_tracking::track_points (feature_tracking.rs:16-61) on packed pyramids: per feature the
 * forward transform {cos, sin, tx, ty} (identity when lost) and the keep flag. */
int rsvio_ft_track_points(const float* pyr0, const float* pyr1, int32_t w, int32_t h, int32_t nlevels,
                          double ratio, const float* xy, int32_t n, int32_t max_iter, float lm_lambda,
                          int32_t matching_cost, float* iso_out, uint8_t* valid_out);
/* shi_tomasi_score (feature_detection.rs:82-164) */
int rsvio_ft_shi_tomasi_score(const float* img, int32_t w, int32_t h, float detection_blur, float* score);
/* feature_detection::add_points (feature_detection.rs:47-80) on the fine level with the tracked
 * features' centres: new corners (u32 x, y) in (y, x) order. */
int rsvio_ft_add_points(const float* fine, int32_t w, int32_t h, const float* tracked_xy, int32_t n_tracked,
                        float threshold, int32_t min_dist, float detection_blur, uint32_t* out_xy, int32_t cap,
                        int32_t* n_out);

/* ============ T11: the trackers' f32 sin/cos (glibc sinf/cosf restated, trig.hpp) ============ */

/* Rust's f32::sin/cos as se2_exp_matrix reaches them through nalgebra's Rotation2::new
 * (src/feature_tracker/image_utilities.rs:84,93-94) and the crate's exp_se2
 * (feature_tracker/src/feature_tracker/feature_tracking.rs:199-203): glibc sinf/cosf on x86-64
 * Linux.  Parity entry points for the device restatement the LK kernels use:
 * rsvio_sincosf evaluates it on n host values; rsvio_sincosf_digest evaluates it on the f32 bit
 * patterns [first, first + count) and returns one 64-bit digest per 2^chunk_log2 inputs (the sum
 * mod 2^64 of splitmix64(((sin bits << 32) | cos bits) + u * 0x9E3779B97F4A7C15) over inputs u,
 * NaNs as 0x7fc00000), so all 2^32 inputs can be compared with the host's libm.  first must be
 * chunk-aligned, first + count <= 2^32, 16 <= chunk_log2 <= 32. */
int rsvio_sincosf(const float* x, size_t n, float* sin_out, float* cos_out);
int rsvio_sincosf_digest(uint64_t first, uint64_t count, uint32_t chunk_log2, uint64_t* digests_out);

/* ================= T12: camera unprojection (Frame::add_*_feature) ================= */

/* Camera models of src/datasets/mod.rs:93-163 (camera-intrinsic-model 0.7.2):
 *   RSVIO_CAM_OPENCV5  OpenCVModel5, params {fx, fy, cx, cy, k1, k2, p1, p2, k3} (pinhole-radtan)
 *   RSVIO_CAM_EUCM     EUCM,         params {fx, fy, cx, cy, alpha, beta}
 * unproject_one's return convention is not verifiable offline, so it is
 * a parameter: RSVIO_UNPROJ_PLANE gives (x/z, y/z), RSVIO_UNPROJ_RAY the first two components
 * of the unit ray.  frame.rs:118-119,131-132 keep components [0..2] as f32. */
enum { RSVIO_CAM_OPENCV5 = 0, RSVIO_CAM_EUCM = 1 };
enum { RSVIO_UNPROJ_PLANE = 0, RSVIO_UNPROJ_RAY = 1 };

typedef struct {
    int32_t model;           /* RSVIO_CAM_* */
    int32_t convention;      /* RSVIO_UNPROJ_* */
    int32_t max_iterations;  /* radtan Newton cap; <= 0 means 20 */
    int32_t reserved;
    double params[9];
} rsvio_camera;              /* 88 bytes */

/* Batched unproject_one (frame.rs:107-134): pixels (n x 2 f32, cast to f64 as frame.rs:118)
 * -> undistorted (n x 2 f32).  Failure of one point (EUCM outside its valid cone, radtan
 * Newton not converging, non-finite) gives NaN coordinates and valid_out = 0 (valid_out may be
 * NULL).  Host buffers, current device. */
int rsvio_unproject(const rsvio_camera* cam, const float* px, size_t n, float* out_xy,
                    uint8_t* valid_out);
/* Same on device pointers, enqueued on `stream` (hipStream_t; NULL = legacy stream). */
int rsvio_unproject_d(const rsvio_camera* cam, const float* d_px, size_t n, float* d_out_xy,
                      uint8_t* d_valid_out, void* stream);
/* The forward projection of the same models: camera-frame points (n x 3 f64) -> pixels (n x 2 f64),
 * with distortion, in f64 without contraction.
 *   EUCM    den = alpha sqrt(beta (X*X + Y*Y) + Z*Z) + (1 - alpha) Z, valid iff den > 0
 *   radtan  valid iff Z > 0; k3 included
 * An invalid point gives NaN coordinates and valid_out = 0 (valid_out may be NULL); n = 0 is a no-op
 * that returns RSVIO_OK.  Host buffers, current device; _d: device pointers, enqueued on `stream`. */
int rsvio_project(const rsvio_camera* cam, const double* pts, size_t n, double* out_uv, uint8_t* valid_out);
int rsvio_project_d(const rsvio_camera* cam, const double* d_pts, size_t n, double* d_out_uv,
                    uint8_t* d_valid_out, void* stream);
/* Frame::add_left_feature / add_right_feature on the tracker's output: after this call every
 * process_frame also unprojects both cameras' features on device (fused into the output
 * packing) and rsvio_tracker_undistorted returns them in feature order.  NULL, NULL turns it
 * off. */
int rsvio_tracker_set_cameras(rsvio_tracker* t, const rsvio_camera* left, const rsvio_camera* right);
int rsvio_tracker_undistorted(rsvio_tracker* t, float* out_l, size_t cap_l, float* out_r, size_t cap_r);

/* =========================== HP-B: sliding-window BA =========================== */

enum {
    RSVIO_LM_COST_TOLERANCE = 1,      /* OptimizationStatus::CostToleranceReached */
    RSVIO_LM_PARAMETER_TOLERANCE = 2, /* ::ParameterToleranceReached */
    RSVIO_LM_MAX_ITERATIONS = 3,      /* ::MaxIterationsReached (counts as success, sliding_window.rs:393) */
    RSVIO_LM_TRUST_REGION = 4,        /* ::TrustRegionRadiusTooSmall */
    RSVIO_LM_NUMERICAL_FAILURE = -1,  /* ::NumericalFailure -> caller reverts (:354-359) */
    RSVIO_LM_SKIPPED = -2,            /* too few residuals (:309-319) -> Ok(false) */
    RSVIO_LM_LINEAR_SOLVE_FAILED = -3 /* Err(LinearSolveFailed / "Singular matrix"): the caller retries
                                       * with RSVIO_SOLVER_CHOLESKY, then reverts (:326-353) */
};

enum {
    RSVIO_SOLVER_SCHUR = 0,     /* LinearSolverType::SparseSchurComplement (sliding_window.rs:126-135) */
    RSVIO_SOLVER_CHOLESKY = 1   /* LinearSolverType::SparseCholesky, the fallback (:334-341): the full
                                 * damped system, landmarks eliminated first (3x3 LL^T blocks) */
};

typedef struct {
    int32_t max_iterations;       /* 20  (sliding_window.rs:131) */
    double cost_tolerance;        /* 1e-6 (:132) */
    double parameter_tolerance;   /* 1e-9 (:133) */
    double huber_delta;           /* 2.0 (:295) */
    double lambda_init;           /* 1e-4 (build's LM) */
    int32_t linear_solver;        /* RSVIO_SOLVER_* (BA only; PnP always solves its 6x6 by Cholesky) */
} rsvio_lm_cfg;

typedef struct {
    int32_t status;               /* RSVIO_LM_* ; success iff > 0 (is_optimization_successful :384-395) */
    int32_t iterations;
    double initial_cost;
    double final_cost;
    double solve_ms;              /* device time of the solve (HIP events) */
} rsvio_ba_result;

typedef struct {
    int32_t max_keyframes;        /* window size (config/euroc_vio.yaml:35) */
    int32_t max_landmarks;
    int32_t max_observations;
    int32_t device;
} rsvio_ba_params;

typedef struct rsvio_ba rsvio_ba;

int rsvio_ba_create(const rsvio_ba_params* params, rsvio_ba** out);
void rsvio_ba_destroy(rsvio_ba* ba);

/* SlidingWindow::optimize's solver call (sliding_window.rs:325): LM with Schur elimination of
 * the landmarks on BundleAdjustmentFactor residuals (factors.rs:350-447) + Huber.
 * Observations: landmark index, keyframe index, camera (0 = left, 1 = right), normalised
 * undistorted coordinates (frame.rs:118-119).  T_C_B2: two row-major 4x4 (T_Cl_B, T_Cr_B).
 * pose7 and p_W are updated in place on success (status > 0). */
int rsvio_ba_solve(rsvio_ba* ba, int32_t n_kf, double* pose7, const uint8_t* kf_fixed,
                   int32_t n_lm, double* p_W, int32_t n_obs, const int32_t* obs_lm,
                   const int32_t* obs_kf, const uint8_t* obs_cam, const double* obs_uv,
                   const double* T_C_B2, const rsvio_lm_cfg* cfg, rsvio_ba_result* res);

/* Split form: upload a window, solve it (possibly many times from the uploaded initial state;
 * nothing crosses PCIe inside rsvio_ba_run except the status).  Observations may come in any
 * order; one per (landmark, keyframe, camera) -- a second is RSVIO_ERR_INVALID_ARG, as is an
 * index out of range.  The host validates the observations and packs per-landmark (keyframe,
 * camera) masks into pinned staging; the slot layout and Schur pair lists are built on the
 * device after one H2D copy.  Does not wait for the previous solve's stream tail.  The window's
 * geometry and buffer addresses also go up as a device descriptor: the first solve of a window
 * replays a launch graph keyed only by the window's shape (free keyframes, LM configuration, wave
 * count within a band), so a new keyframe window costs one graph launch, no capture. */
int rsvio_ba_set_problem(rsvio_ba* ba, int32_t n_kf, const double* pose7, const uint8_t* kf_fixed,
                         int32_t n_lm, const double* p_W, int32_t n_obs, const int32_t* obs_lm,
                         const int32_t* obs_kf, const uint8_t* obs_cam, const double* obs_uv,
                         const double* T_C_B2);
int rsvio_ba_run(rsvio_ba* ba, const rsvio_lm_cfg* cfg, rsvio_ba_result* res);
/* rsvio_ba_run split in two so the host can overlap other work (e.g. the next frame's
 * tracking) with the solve: _run_async enqueues the first chunk of LM iterations and returns;
 * _wait completes the solve and fills res.  One solve in flight per handle.  Single rank, _wait
 * returns when the final LM state has landed in host memory (a ticket the last decision kernel
 * publishes); the stream may still be draining that kernel's exit, and the handle synchronises
 * it before any later call copies to or from its buffers.  res->solve_ms: device wall clock
 * from the solve's first kernel to its last decision. */
int rsvio_ba_run_async(rsvio_ba* ba, const rsvio_lm_cfg* cfg);
/* Enqueue the handle's work on a caller-owned stream (NULL: back to the handle's own stream). */
int rsvio_ba_set_stream(rsvio_ba* ba, void* stream);
int rsvio_ba_wait(rsvio_ba* ba, rsvio_ba_result* res);
/* The current state (n_kf x 7 poses, n_lm x 3 points).  After the first call on a handle, each
 * later solve's final decision kernel also publishes the optimised state to pinned host memory
 * (one slice per workgroup, each with its own flag), and get_state copies it from there without
 * a stream synchronisation; otherwise (or after rsvio_ba_build_system, a skipped solve, a batch
 * run) it is copied from the device buffers. */
int rsvio_ba_get_state(rsvio_ba* ba, double* pose7, double* p_W);
/* Landmark triangulation and the depth / reprojection gate, on the device.  The reference creates a
 * landmark that is not in the map at depth 2.0 along its first observation's ray and leaves two
 * TODOs (sliding_window.rs:257 "Triangulate instead of assigning depth", :472 "check if points are
 * estimated at obviously wrong locations"); its configs' `depth: {min_depth: 0.1, max_depth: 100.0}`
 * section is read by nothing.  Per observation o (keyframe k, camera c, normalised (u, v)):
 * [R | t] = T_C_B[c] T_B_W(k), centre c_o = -R^T t, unit ray d_o = R^T (u, v, 1)^T / |.|,
 * M_o = I - d_o d_o^T; per landmark p = (sum M_o)^-1 sum M_o c_o over the observations used:
 *   RSVIO_TRI_ALL_VIEWS     every observation of the landmark
 *   RSVIO_TRI_FIRST_STEREO  the two observations of its first keyframe (ascending) that holds both
 *                           cameras: depends on the extrinsics and ONE pose only, so it is safe while
 *                           the poses are poor (the bootstrap, every keyframe at identity)
 * The gate then takes, over the same observations, the depths (R p + t)_z and the squared normalised
 * reprojection errors.  Flags per landmark (rsvio_landmark_info.flags):
 *   OK            the point was accepted
 *   TOO_FEW       fewer than 2 observations used (no stereo keyframe in mode 1); terminal
 *   DEGENERATE    !(det A > 1e-12 n^3) or not finite, n = observations used (two rays: det A =
 *                 2 sin^2 of their angle, i.e. parallax below ~2 microradians); terminal
 *   DEPTH         some depth below min_depth or above max_depth       } both evaluated whenever a
 *   ERROR         max_sq_error > 0 and the largest squared error > it } point exists; may combine
 *   NOT_SELECTED  the mask byte is 0 (n_obs and the figures are 0)
 * n_obs: the observations used; min_depth, max_depth, max_sq_error: over them (0 without a point).
 * Every sum runs in a fixed order: two calls give identical bits. */
enum { RSVIO_TRI_ALL_VIEWS = 0, RSVIO_TRI_FIRST_STEREO = 1 };
enum {
    RSVIO_LM_OK = 1,
    RSVIO_LM_TOO_FEW = 2,
    RSVIO_LM_DEGENERATE = 4,
    RSVIO_LM_DEPTH = 8,
    RSVIO_LM_ERROR = 16,
    RSVIO_LM_NOT_SELECTED = 32
};
typedef struct {
    int32_t mode;                 /* RSVIO_TRI_* */
    int32_t reserved;
    double min_depth, max_depth;  /* metres along the optical axis (the reference configs: 0.1, 100.0) */
    double max_sq_error;          /* squared normalised reprojection error; <= 0: off */
} rsvio_landmark_gate;            /* 32 bytes */
typedef struct {
    int32_t n_obs, flags;
    double min_depth, max_depth, max_sq_error;
} rsvio_landmark_info;            /* 32 bytes */
/* Triangulate the landmarks of the uploaded problem that lm_mask selects (n_lm bytes, NULL = all;
 * n_lm must be the problem's landmark count) from its INITIAL poses, and write the accepted points
 * into the device's initial point array, which every later rsvio_ba_run / _run_async / batch run of
 * this problem starts from (rsvio_ba_solve, the one-shot path, uploads its own).  A rejected or
 * unselected landmark keeps its uploaded value bit for bit.  Reads poses and observations, never
 * the points: idempotent.  With all three outputs NULL the call only enqueues on the handle's
 * stream (set_problem -> triangulate -> run_async has no host wait); otherwise it waits, p_W_out
 * (n_lm x 3) receives the whole initial point array as the next run will see it, info_out (n_lm)
 * the report and n_accepted the number of OK landmarks.  Refused while a solve is in flight.  On a
 * sharded handle it is local (every rank holds all poses and its own landmarks). */
int rsvio_ba_triangulate(rsvio_ba* ba, const uint8_t* lm_mask, int32_t n_lm, const rsvio_landmark_gate* gate,
                         double* p_W_out, rsvio_landmark_info* info_out, int32_t* n_accepted);
/* The gate's report on the state rsvio_ba_get_state would return (the solved state after a solve,
 * the initial state before one) over ALL observations of every landmark (gate->mode is ignored);
 * a landmark with no observation reports TOO_FEW.  Writes nothing but info_out (n_lm) and n_ok. */
int rsvio_ba_check_landmarks(rsvio_ba* ba, int32_t n_lm, const rsvio_landmark_gate* gate,
                             rsvio_landmark_info* info_out, int32_t* n_ok);
/* Pose and landmark covariance from the reduced camera system, on the device.  x is the state
 * rsvio_ba_get_state would return (the solved state after a solve or a batch run, the initial
 * state before one).  H = sum_obs w J^T J is the Gauss-Newton Hessian of the BA cost at x with no
 * damping (lambda = 0): J is BundleAdjustmentFactor::linearize's 2x9 [dp_W | dt | dw]
 * (factors.rs:350-447, zero on its cheirality branch), w the Huber IRLS weight at huber_delta, the
 * pose columns those of the free keyframes in ascending order, in the tangent the LM's (+) uses
 * (se3_plus: [dt; dw] of T_B_W).
 *   pose covariance      Sigma_cc    = S^-1,  S = U - W V^-1 W^T at lambda = 0,  n = 6 n_free <= 120
 *   landmark covariance  Sigma_pp(l) = V_l^-1 + sum_{a,b} Y_a^T Sigma_cc[a,b] Y_b,  Y_k = W_k V_l^-1,
 *                        over the landmark's slots in free keyframes (only fixed ones: V_l^-1)
 * Units: normalised-image-coordinate^2 per unit measurement variance -- the caller multiplies by
 * its sigma^2; no sigma is assumed here.
 * info->status:
 *   RSVIO_COV_OK                 the outputs are written
 *   RSVIO_COV_LANDMARK_SINGULAR  n_singular landmarks with observations have a V that fails the
 *                                solve's det > 0 test (the rule of RSVIO_LM_LINEAR_SOLVE_FAILED)
 *   RSVIO_COV_CAMERA_SINGULAR    a pivot of S was not positive and finite (e.g. no fixed keyframe)
 * On a negative status no covariance output is written; the function still returns RSVIO_OK.
 * cov_cc (n x n row-major, exactly symmetric), cov_pose (n_kf x 36: each keyframe's 6x6 diagonal
 * block of cov_cc, zeros for a fixed keyframe) may be NULL.  lm_idx selects n_sel landmarks (repeats
 * allowed; NULL with n_sel == n_lm: every landmark; n_sel 0: none, cov_lm and lm_flags may be NULL);
 * cov_lm is n_sel x 9, lm_flags n_sel: LM_OK, or LM_NOT_OBSERVED (no observation: zeros).
 * info->cost is the cost at x, device_ms the call's own kernels by HIP events.  The state, and what
 * any later run computes, is untouched; every sum runs in a fixed order (two calls: the same bits).
 * Refused while a solve is in flight and on a sharded handle; an lm_idx entry out of range is
 * RSVIO_ERR_INVALID_ARG. */
enum { RSVIO_COV_OK = 1, RSVIO_COV_CAMERA_SINGULAR = -1, RSVIO_COV_LANDMARK_SINGULAR = -2 };
enum { RSVIO_COV_LM_OK = 1, RSVIO_COV_LM_NOT_OBSERVED = 2 };
typedef struct { int32_t status, n_free, n_singular, reserved; double cost, device_ms; } rsvio_cov_info;
int rsvio_ba_covariance(rsvio_ba* ba, double huber_delta,
                        double* cov_cc,     /* n x n row-major, or NULL */
                        double* cov_pose,   /* n_kf x 36: each keyframe's 6x6 diagonal block, zeros for a fixed one, or NULL */
                        const int32_t* lm_idx, int32_t n_sel,  /* NULL + n_sel == n_lm: every landmark; n_sel 0: none */
                        double* cov_lm,     /* n_sel x 9 */
                        uint8_t* lm_flags,  /* n_sel */
                        rsvio_cov_info* info);
/* Reduced camera system at `lambda` for the uploaded state (parity tests):
 * S is n x n row-major (n = 6 * free keyframes, ascending keyframe order), b is n. */
int rsvio_ba_build_system(rsvio_ba* ba, double lambda, double huber_delta, double* S, double* b,
                          double* cost);

/* Batched mode: n independent windows -- each a handle whose problem was
 * uploaded by rsvio_ba_set_problem -- solved by ONE launch chain (the window is a grid dimension
 * of every LM kernel; one camera-solve workgroup per window), each window exactly as its own
 * rsvio_ba_run would solve it (SlidingWindow::optimize, sliding_window.rs:159-381, per window).
 * Windows may differ in keyframes (<= 10 free each), landmarks and observations; a window the
 * guards of sliding_window.rs:303-319 skip reports RSVIO_LM_SKIPPED.  results[i] is window i's;
 * solve_ms is the whole batch's.  rsvio_ba_get_state on a window handle reads its solution.  The
 * batch borrows the handles (they must outlive it) and runs on its own stream. */
typedef struct rsvio_ba_batch rsvio_ba_batch;
int rsvio_ba_batch_create(rsvio_ba* const* windows, int32_t n, rsvio_ba_batch** out);
int rsvio_ba_batch_run(rsvio_ba_batch* batch, const rsvio_lm_cfg* cfg, rsvio_ba_result* results);
void rsvio_ba_batch_destroy(rsvio_ba_batch* batch);

/* The batched keyframe step: what a window calls around its solve -- rsvio_ba_triangulate,
 * rsvio_ba_check_landmarks, rsvio_ba_covariance -- for all windows of a batch by one launch (chain)
 * each, and the solve of a subset.  `active` is n bytes, one per window of the batch (NULL: every
 * window).  A window that is not active is not read, written or required to hold a problem, and its
 * slot / result is left untouched.  Slot i is window i's; per slot the semantics are exactly the
 * single call's (the same kernels' code on the window as a grid dimension: the same bits).
 * Everything is checked before anything is launched or written: RSVIO_ERR_INVALID_ARG, with
 * rsvio_last_error naming the slot, for an active window without a problem, with a solve in flight
 * (rsvio_ba_run_async not waited), an n_lm that differs from the problem's, a bad landmark
 * selection, or huber_delta <= 0 / NaN.  The calls run on the batch's stream after, on the device,
 * what each active window's own stream has enqueued; where a call returns without a host wait
 * (the enqueue-only triangulate) each active window's stream is made to wait for the batch's kernel
 * by an event, so a later single-handle call on the window sees the batch's writes.  *device_ms
 * (may be NULL): the call's kernels by HIP events; 0 when the call only enqueued. */
/* rsvio_ba_batch_run over the active windows only (rsvio_ba_batch_run is the NULL case). */
int rsvio_ba_batch_run_active(rsvio_ba_batch* batch, const uint8_t* active, const rsvio_lm_cfg* cfg,
                              rsvio_ba_result* results);
typedef struct {
    const uint8_t* lm_mask;           /* triangulate: n_lm bytes, NULL = all landmarks; check: ignored */
    const rsvio_landmark_gate* gate;  /* NULL: the call's gate */
    double* p_W_out;                  /* triangulate: n_lm x 3, the initial points as the next run sees them; or NULL */
    rsvio_landmark_info* info_out;    /* n_lm, or NULL */
    int32_t n_lm;                     /* must be the window's landmark count */
    int32_t n_ok;                     /* out: landmarks reported OK; -1 when the call only enqueued */
    int32_t status;                   /* out: RSVIO_OK */
    int32_t reserved;
} rsvio_ba_landmark_slot;             /* 48 bytes */
/* rsvio_ba_triangulate per active window.  `gate` may be NULL only if every active slot has its own.
 * With p_W_out and info_out NULL in every active slot the call only enqueues (set_problem x n ->
 * batch_triangulate -> batch_run_active has no host wait); otherwise one host wait for the call. */
int rsvio_ba_batch_triangulate(rsvio_ba_batch* batch, const uint8_t* active, const rsvio_landmark_gate* gate,
                               rsvio_ba_landmark_slot* slots, double* device_ms);
/* rsvio_ba_check_landmarks per active window (reads only; one host wait). */
int rsvio_ba_batch_check_landmarks(rsvio_ba_batch* batch, const uint8_t* active, const rsvio_landmark_gate* gate,
                                   rsvio_ba_landmark_slot* slots, double* device_ms);
typedef struct {
    double* cov_cc;                   /* as rsvio_ba_covariance's arguments of the same names */
    double* cov_pose;
    const int32_t* lm_idx;
    double* cov_lm;
    uint8_t* lm_flags;
    int32_t n_sel;
    int32_t reserved;
    rsvio_cov_info info;              /* out; device_ms is the whole call's */
} rsvio_ba_cov_slot;                  /* 80 bytes */
/* rsvio_ba_covariance per active window by one launch chain (K4, K4c, the camera covariance once
 * per distinct solver template among the windows, the landmark covariance) and at most two host
 * waits whatever n is.  A singular window is a normal slot result (info.status < 0, nothing else
 * written for it).  The state, and what any later run computes, is untouched. */
int rsvio_ba_batch_covariance(rsvio_ba_batch* batch, const uint8_t* active, double huber_delta,
                              rsvio_ba_cov_slot* slots, double* device_ms);

/* Landmark sharding over ranks: each rank uploads only its own
 * landmarks/observations; the reduced system and costs are summed with RCCL over xGMI. */
int rsvio_rccl_unique_id(uint8_t* out, size_t cap);   /* cap >= 128 */
int rsvio_ba_attach_comm(rsvio_ba* ba, int32_t nranks, int32_t rank, const uint8_t* unique_id);
/* Peer-to-peer one-shot all-reduce for the same exchanges (latency-bound small messages over
 * xGMI): each rank exports its exchange buffer (64-byte IPC handle), the handles of all ranks
 * are exchanged by the caller, then every rank attaches; attach runs a self-test and fails
 * (the handle keeps RCCL / its previous collective) if any peer is unreachable.  All ranks
 * must end in the same mode: on any rank's failure every rank calls rsvio_ba_detach_p2p. */
int rsvio_ba_p2p_export(rsvio_ba* ba, int32_t nranks, uint8_t* handle_out, size_t cap);
int rsvio_ba_attach_p2p(rsvio_ba* ba, int32_t nranks, int32_t rank, const uint8_t* handles);
int rsvio_ba_detach_p2p(rsvio_ba* ba);
/* Diagnostics (no reference counterpart): average device microseconds of one P2P exchange of n
 * doubles (1 <= n <= 8192) over reps back-to-back exchanges after one warm-up; collective --
 * every attached rank makes the same call.  Reported by bench.py at N > 1. */
int rsvio_ba_p2p_latency(rsvio_ba* ba, int32_t reps, int32_t n, double* us_out);
/* Diagnostics (no reference counterpart): the exchange form the current problem's LM iterations
 * take -- -1 not P2P-sharded; 0 five launches (X1, X2); 1 four (K5 exchanges the system, X2 the
 * trial scalars); 2, 3, 4 three (the trial exchange folded into K6 / the next decision).  Level 3
 * (the default) needs K6's whole grid resident on the stream's CUs at once (its reducer workgroup
 * waits inside the grid); a problem past that capacity takes level 1, bit-identically. */
int rsvio_ba_p2p_level(rsvio_ba* ba, int32_t* level_out);

/* ===== B8: motion tracking (PnP) + keyframe rule (SlidingWindow::track_motion) ===== */

/* One SE3 pose (T_B_W) against the fixed map: PnPFactor (src/optimization/factors.rs:455-583,
 * no cheirality guard, J = [dt | dw]) with Huber(2.0), the build's LM with
 * max 10 iterations (sliding_window.rs:494-501), initialised from the last keyframe
 * (:506-517); then the keyframe rule of estimator.rs:195-226.  The whole sequence -- map join,
 * LM, T_W_B = inverse(SE3), T_rel, euler angles, thresholds -- is one single-workgroup kernel. */
typedef struct rsvio_pnp rsvio_pnp;

typedef struct {
    double translation_threshold;  /* keyframe_management.translation_threshold (euroc 0.05) */
    double rotation_threshold;     /* keyframe_management.rotation_threshold    (euroc 0.05) */
} rsvio_keyframe_rule;

typedef struct {
    int32_t status;            /* RSVIO_LM_*; > 0 or TRUST_REGION is success (:384-395) */
    int32_t iterations;
    int32_t is_keyframe;       /* estimator.rs:216-225; 1 on failure (frame keeps is_keyframe) */
    int32_t n_observations;    /* features with a map point (:521-547) */
    double initial_cost;
    double final_cost;
    double translation_norm;   /* ||t_rel|| (estimator.rs:206) */
    double rotation_norm;      /* ||euler(R_rel)|| (:207-212) */
    double T_W_B[16];          /* row-major; identity on failure (frame.rs:95, state.rs:26) */
    double kernel_ms;          /* device time of the launch: its first wave's entry to the result
                                  write (the device wall clock; no host or copy time) */
} rsvio_motion_result;        /* 184 bytes */

int rsvio_pnp_create(int32_t device, rsvio_pnp** out);
void rsvio_pnp_destroy(rsvio_pnp* p);
/* UnitQuaternion::from_matrix (sliding_window.rs:221,511; estimator.rs:209-211): nalgebra's
 * iterative Rotation3::from_matrix_eps(m, f64::EPSILON, 0, identity) then from_rotation_matrix,
 * for n row-major 3x3 matrices -> n quaternions (w, i, j, k).  Host only (no device needed). */
int rsvio_quat_from_matrix(const double* R, size_t n, double* q);
/* ---- the Estimator's per-keyframe host logic (host only, no device needed) ---- */

/* SlidingWindow::optimize's problem assembly (sliding_window.rs:174-300) for a window of n_kf
 * keyframes: T_W_B (n_kf row-major 4x4), T_B_C2 (the FRONT keyframe's T_B_Cl, T_B_Cr; :180-181),
 * per keyframe k and camera c (list 2k + c, the 2 n_kf lists back to back in ids / uv, n_feat[i]
 * entries each) the features' ids and undistorted coordinates (frame.rs:107-134, f32), the map (ids strictly ascending, p_W as f32; :466-475).  Out: pose7
 * (T_B_W as [t; w, i, j, k], :214-226), kf_fixed (KF_0), T_C_B2 (T_Cl_B, T_Cr_B), the landmarks
 * -- features seen at least once in each camera across the window (:183-209, :238-240), indexed
 * by first appearance -- with their ids and initial values (map point, else depth 2.0 along the
 * first observation's ray, :241-262), and one observation per factor in window order (keyframe,
 * left then right, feature order).  RSVIO_ERR_CAPACITY when cap_lm / cap_obs are too small. */
int rsvio_window_problem(int32_t n_kf, const double* T_W_B, const double* T_B_C2, const uint64_t* ids,
                         const float* uv, const int32_t* n_feat, const uint64_t* map_ids,
                         const float* map_pw, int32_t n_map, double* pose7, uint8_t* kf_fixed, double* T_C_B2,
                         int32_t cap_lm, uint64_t* lm_ids, double* p_init, int32_t* n_lm, int32_t cap_obs,
                         int32_t* obs_lm, int32_t* obs_kf, uint8_t* obs_cam, double* obs_uv, int32_t* n_obs);
/* process_optimization_result (sliding_window.rs:418-486): keyframe T_W_B = inverse(SE3(pose7))
 * (n_kf row-major 4x4) and the map = the optimised landmarks as f32, by ascending id. */
int rsvio_window_apply(int32_t n_kf, const double* pose7, int32_t n_lm, const uint64_t* lm_ids, const double* p_W,
                       double* T_W_B, uint64_t* map_ids, float* map_pw);

/* Launch rsvio_track_motion on a caller-owned stream (hipStream_t; NULL: the handle's own). */
int rsvio_pnp_set_stream(rsvio_pnp* p, void* stream);
/* SlidingWindow::map_points after optimize (sliding_window.rs:466-475): feature ids strictly
 * ascending, p_W as f32 triples. */
int rsvio_pnp_set_map(rsvio_pnp* p, const uint64_t* ids, const float* p_W, int32_t n);
/* track_motion(&Frame) + keyframe rule for a frame given as host arrays (feature ids and
 * undistorted coordinates per camera, frame.rs:107-134).  T_W_B_last_kf: keyframes.back()
 * (:506); T_C_B2: T_Cl_B, T_Cr_B of keyframes.front() (:520-521), row-major 4x4 each. */
int rsvio_track_motion(rsvio_pnp* p, const uint64_t* ids_l, const float* uv_l, size_t n_l,
                       const uint64_t* ids_r, const float* uv_r, size_t n_r,
                       const double* T_W_B_last_kf, const double* T_C_B2, const rsvio_lm_cfg* cfg,
                       const rsvio_keyframe_rule* rule, rsvio_motion_result* res);
/* Same for the tracker's last COLLECTED frame, read in place on the device (ids and the fused
 * undistorted coordinates; needs rsvio_tracker_set_cameras): no host round trip between
 * tracking and motion tracking.  Runs on the pnp handle's stream, so it may run while the next
 * frame (rsvio_tracker_submit*) is being tracked: that frame writes the other output slot. */
int rsvio_track_motion_tracker(rsvio_pnp* p, rsvio_tracker* t, const double* T_W_B_last_kf,
                               const double* T_C_B2, const rsvio_lm_cfg* cfg,
                               const rsvio_keyframe_rule* rule, rsvio_motion_result* res);

/* Outlier-robust motion tracking: a stereo 3-point RANSAC in front of the same LM (no reference
 * counterpart: the reference's only defence is Huber(2.0) in normalised units, inactive for real
 * residuals).  Three launches on the handle's stream, no host wait between them and no workgroup
 * waiting on another; every cross-workgroup reduction is done by the next launch.
 *   R1  the joined observations (a feature whose id is in the map; left list then right list, each
 *       in list order -- the order of rsvio_track_motion's factors) and the PAIRS: ids present in
 *       both lists with a map point, by ascending position in the left list (equal ids inside the
 *       right list: the first).  Each pair's point q in the BODY frame is the least-squares
 *       intersection of its two rays ([R | t] = T_C_B[c], c_o = -R^T t, d_o = R^T (u, v, 1)^T / |.|,
 *       M_o = I - d_o d_o^T, q = (sum M_o)^-1 sum M_o c_o); the pair is valid iff
 *       det(sum M_o) > 1e-12 2^3 (rsvio_ba_triangulate's rule at two rays), q is finite and both
 *       depths (T_C_B[c] q)_z >= min_depth.
 *   R2  hypotheses 0 <= h < n_hyp <= 1024, one wave each.  h = 0 is the prior: the pose
 *       rsvio_track_motion starts from.  h >= 1 takes pair indices i_k, k = 0..2, from
 *       samples[3 h + k] (row 0 is ignored) or, with samples NULL, i_k = z mod n_pairs in 64-bit
 *       unsigned arithmetic with  z = seed + 0x9E3779B97F4A7C15 (3 h + k + 1),
 *       z = (z ^ z >> 30) 0xBF58476D1CE4E5B9,  z = (z ^ z >> 27) 0x94D049BB133111EB,  z ^= z >> 31.
 *       With a = w2 - w1, b = w3 - w1, e1 = a / |a|, e3 = a x b / |a x b|, e2 = e3 x e1 and
 *       F_w = [e1 e2 e3] of the three map points, F_q likewise of the three q:  R = F_q F_w^T,
 *       t = mean(q) - R mean(w)  (T_B_W).  The hypothesis is invalid (count -1) when n_pairs < 3, an
 *       index is out of range (not an error), two indices are equal, a chosen pair is invalid,
 *       |a x b|^2 <= 1e-12 |a|^2 |b|^2 in either frame, or anything is not finite.  A joined
 *       observation is an inlier iff p_C = T_C_B[c] (R w + t) has z >= min_depth and
 *       |p_C.xy / z - uv|^2 <= inlier_sq_error; hyp_count[h] is the number of inliers.
 *   R3  the winner is the largest count, the lowest h on a tie.  Below max(min_inliers, 1):
 *       ransac_status = NO_CONSENSUS and `motion` is what rsvio_track_motion returns when no
 *       feature has a map point (RSVIO_LM_SKIPPED, identity, is_keyframe = 1); every joined
 *       observation is marked an outlier.  Otherwise rsvio_track_motion's LM (the caller's cfg) runs
 *       on the winner's inliers only, in the same factor order, from the winner's pose, and the
 *       keyframe rule is applied against T_W_B_last_kf; motion.n_observations is the number of
 *       factors.  Then every joined observation is classified by the same test at the refined pose
 *       (at the winner's pose if the LM failed): mask_l[n_l], mask_r[n_r] hold 0 = no map point,
 *       1 = inlier, 2 = outlier, n_inliers the number of 1s.
 * n_hyp = 1 with an all-accepting inlier_sq_error (e.g. 1e300) and min_inliers <= the joined
 * observations gives rsvio_track_motion's result bit for bit.  TOO_FEW_PAIRS (n_pairs < 3: only
 * h = 0 could be valid) is a success status.  device_ms: the three launches by HIP events.  Two calls
 * give identical bits (the counts are integers, every floating-point sum runs in a fixed order).
 * n_hyp outside [1, 1024], inlier_sq_error <= 0 or NaN, or a NULL cfg: RSVIO_ERR_INVALID_ARG. */
enum { RSVIO_RANSAC_OK = 1, RSVIO_RANSAC_TOO_FEW_PAIRS = 2, RSVIO_RANSAC_NO_CONSENSUS = -1 };
typedef struct {
    int32_t n_hyp, min_inliers;
    uint64_t seed;
    double inlier_sq_error;  /* squared normalised reprojection error (1e-4: ~4.6 px at EuRoC's fx) */
    double min_depth;        /* metres along the optical axis (the reference configs: 0.1) */
} rsvio_ransac_cfg;          /* 32 bytes */
typedef struct {
    rsvio_motion_result motion;
    int32_t ransac_status;   /* RSVIO_RANSAC_* */
    int32_t n_pairs, n_valid_pairs, n_valid_hyp, best_hyp, best_count, n_inliers, reserved;
    double device_ms;
} rsvio_robust_motion_result;  /* 224 bytes */
int rsvio_track_motion_robust(rsvio_pnp* p, const uint64_t* ids_l, const float* uv_l, size_t n_l,
                              const uint64_t* ids_r, const float* uv_r, size_t n_r,
                              const double* T_W_B_last_kf, const double* T_C_B2, const rsvio_lm_cfg* cfg,
                              const rsvio_keyframe_rule* rule, const rsvio_ransac_cfg* ransac,
                              const int32_t* samples,  /* n_hyp x 3 pair indices, or NULL: the seeded sampler */
                              uint8_t* mask_l, uint8_t* mask_r,  /* n_l, n_r, or NULL */
                              int32_t* hyp_count,      /* n_hyp, or NULL */
                              rsvio_robust_motion_result* res);
/* Same for the tracker's last collected frame, read in place on the device (as
 * rsvio_track_motion_tracker); mask_l / mask_r are indexed like the collected feature lists. */
int rsvio_track_motion_robust_tracker(rsvio_pnp* p, rsvio_tracker* t, const double* T_W_B_last_kf,
                                      const double* T_C_B2, const rsvio_lm_cfg* cfg,
                                      const rsvio_keyframe_rule* rule, const rsvio_ransac_cfg* ransac,
                                      const int32_t* samples, uint8_t* mask_l, uint8_t* mask_r,
                                      int32_t* hyp_count, rsvio_robust_motion_result* res);

/* Batched motion tracking (the serving mode's third leg beside rsvio_track_points_table_d and
 * rsvio_ba_batch_*): n handles, each with its own map, and ONE frame per handle tracked by one
 * launch (plain; workgroup i is stream i) or three (robust: join on a grid of n, score on
 * (n_hyp, n), refit on n) with one upload and one host wait.  results[i] is exactly -- bit for
 * bit, keyframe rule included -- what rsvio_track_motion / rsvio_track_motion_robust returns for
 * frame i on handle i; kernel_ms is that workgroup's own device time, *device_ms (may be NULL)
 * and, on the robust path, every results[i].device_ms the whole batch's launches by HIP events.
 * A frame whose LM fails or is skipped is a normal result.
 *   The batch borrows the handles (they must outlive it; all on one device; the same handle may
 * sit in several slots) and runs on a stream of its own.  Every run reads each handle's CURRENT
 * map, so an rsvio_pnp_set_map between two runs is picked up; the map is read-only during a run.
 *   A frame's lists are host arrays (on_device = 0: staged into the batch's one upload) or DEVICE
 * pointers read in place (on_device = 1: ids `id_stride` bytes apart, 0 meaning 8 -- e.g.
 * sizeof(rsvio_feature) for the tracker's output -- and uv as float pairs), complete on the
 * device before the call.  frames[i].cfg overrides the call's cfg for slot i; `samples`, `mask_l`,
 * `mask_r` and `hyp_count` are as in rsvio_track_motion_robust (ignored by the plain call).
 *   Everything is checked before anything is launched or written: 1 <= n <= 4096; a NULL
 * argument, a bad `ransac`, an id_stride in 1..7 or no cfg at all for a frame is
 * RSVIO_ERR_INVALID_ARG; a frame with n_l + n_r > 4096 is RSVIO_ERR_CAPACITY and
 * rsvio_last_error names the slot.  The kernels hold a frame's features in LDS entries for 1024
 * features when the batch's largest frame has at most 1024 (several workgroups per CU), for 4096
 * otherwise; RSVIO_PNP_BATCH_CAP=4096 in the environment forces the large form.  The choice
 * changes no bit of any result. */
typedef struct rsvio_pnp_batch rsvio_pnp_batch;
typedef struct {
    const uint64_t* ids_l;  const float* uv_l;  size_t n_l;   /* as rsvio_track_motion */
    const uint64_t* ids_r;  const float* uv_r;  size_t n_r;
    const double* T_W_B_last_kf;   /* 16 */
    const double* T_C_B2;          /* 32 */
    const rsvio_lm_cfg* cfg;       /* NULL: the call's cfg */
    const int32_t* samples;        /* robust only: n_hyp x 3, or NULL: the seeded sampler */
    uint8_t* mask_l; uint8_t* mask_r; int32_t* hyp_count;  /* robust only; each may be NULL */
    int32_t on_device;   /* 0: ids/uv are host arrays.  1: DEVICE pointers, read in place */
    int32_t id_stride;   /* bytes between ids (0 means 8); e.g. sizeof(rsvio_feature) for tracker output */
} rsvio_motion_frame;
int rsvio_pnp_batch_create(rsvio_pnp* const* handles, int32_t n, rsvio_pnp_batch** out);
int rsvio_pnp_batch_track_motion(rsvio_pnp_batch* b, const rsvio_motion_frame* frames,
                                 const rsvio_lm_cfg* cfg, const rsvio_keyframe_rule* rule,
                                 rsvio_motion_result* results, double* device_ms);
int rsvio_pnp_batch_track_motion_robust(rsvio_pnp_batch* b, const rsvio_motion_frame* frames,
                                        const rsvio_lm_cfg* cfg, const rsvio_keyframe_rule* rule,
                                        const rsvio_ransac_cfg* ransac,
                                        rsvio_robust_motion_result* results, double* device_ms);
void rsvio_pnp_batch_destroy(rsvio_pnp_batch* b);

/* Motion covariance: the 6x6 covariance of a frame's pose from the PnP Hessian (no reference
 * counterpart; the per-frame companion of rsvio_ba_covariance).  One single-workgroup launch per
 * frame, one pass over the features: no LM runs, no existing call changes.
 *   Pose.  x is T_B_W = inverse(T_W_B) of the T_W_B the caller passes (a rigid inverse in f64 on
 * the host) -- the pose the caller was given back, not the LM's internal 7-vector.  It need not be
 * a minimum of the cost.
 *   Factors.  A feature of the left list, then of the right list, in list order, is a factor iff
 * its id has a map point (rsvio_track_motion's lookup) and its mask byte is 1, or no mask was given
 * for that list.  A mask byte of 1 on a feature without a map point is ignored: the masks are
 * exactly what rsvio_track_motion_robust writes (1 = inlier).
 *   H = sum_factors w J^T J with no damping: J is the PnP factor's 2x6 [dt | dw], w the Huber IRLS
 * weight at huber_delta, in the tangent the LM's (+) uses (T_B_W <- T_B_W Exp([dt; dw])) -- the
 * convention of rsvio_ba_covariance's pose blocks, so a frame's covariance and a keyframe's are
 * comparable.
 *   cov36 = H^-1, 6x6 row-major, symmetric bit for bit, per unit measurement variance in
 * normalised-image-coordinate^2: the caller multiplies by its sigma^2.  Because
 * T_W_B' = Exp(-d) T_W_B, it is also the covariance of T_W_B under a LEFT (world-side) perturbation.
 * info->status:
 *   RSVIO_MCOV_OK        cov36 is H^-1
 *   RSVIO_MCOV_TOO_FEW   fewer than 3 factors (six rows for six unknowns); also no factor at all,
 *                        an empty map or a handle without a map
 *   RSVIO_MCOV_SINGULAR  an LDL^T pivot of H is not positive and finite (the solver's and the BA
 *                        covariance's rule), e.g. a non-finite T_W_B or a point on a camera's z = 0
 * On a status other than OK the 36 outputs are NaN; the function still returns RSVIO_OK.  A
 * geometry degenerate only up to rounding may report OK with a huge covariance or SINGULAR.
 * info: n_observations the factors used, n_downweighted those with w < 1, cost = sum rho / 2 over
 * the factors (rsvio_motion_result.final_cost's definition), min_pivot the smallest pivot (the
 * first one that failed on SINGULAR, 0 when nothing was factorised), kernel_ms as in
 * rsvio_motion_result.  Every sum runs in a fixed order: two calls give the same bits, and slot i
 * of the batched call gives the single call's on handle i.
 *   The calls run on the handle's active stream (the batch call on the batch's: one upload, one
 * launch, one host wait) and neither read nor change the map or anything a tracking call left.
 * Everything is checked before anything is launched or written: a NULL required pointer, or
 * huber_delta <= 0 or NaN, is RSVIO_ERR_INVALID_ARG; n_l + n_r > 4096 is RSVIO_ERR_CAPACITY (the
 * batch names the slot in rsvio_last_error). */
enum { RSVIO_MCOV_OK = 1, RSVIO_MCOV_TOO_FEW = -1, RSVIO_MCOV_SINGULAR = -2 };
typedef struct {
    int32_t status;           /* RSVIO_MCOV_* */
    int32_t n_observations;   /* factors used */
    int32_t n_downweighted;   /* ... with a Huber weight below 1 */
    int32_t reserved;
    double cost;              /* sum rho / 2 over the factors */
    double min_pivot;         /* smallest LDL^T pivot; 0 if not factorised */
    double kernel_ms;         /* device wall clock, as rsvio_motion_result.kernel_ms */
} rsvio_motion_cov_info;      /* 40 bytes */
int rsvio_motion_covariance(rsvio_pnp* p, const uint64_t* ids_l, const float* uv_l, size_t n_l,
                            const uint64_t* ids_r, const float* uv_r, size_t n_r,
                            const uint8_t* mask_l, const uint8_t* mask_r,  /* n_l, n_r bytes, or NULL: every joined feature */
                            const double* T_W_B, const double* T_C_B2, double huber_delta,
                            double* cov36, rsvio_motion_cov_info* info);
/* Same for the tracker's last collected frame, read in place on the device (as
 * rsvio_track_motion_tracker, with its preconditions); mask_l / mask_r are host arrays indexed
 * like the collected feature lists. */
int rsvio_motion_covariance_tracker(rsvio_pnp* p, rsvio_tracker* t, const uint8_t* mask_l, const uint8_t* mask_r,
                                    const double* T_W_B, const double* T_C_B2, double huber_delta,
                                    double* cov36, rsvio_motion_cov_info* info);
/* Batched: the frame table of rsvio_pnp_batch_track_motion*, one launch on a grid of n.  Read per
 * slot: the lists (on_device 0 or 1, id_stride), T_C_B2, and mask_l / mask_r as INPUTS when
 * non-NULL (host arrays: the ones the robust batch call filled); cfg, samples, hyp_count and
 * T_W_B_last_kf are ignored.  T_W_B holds slot i's pose at 16 i, cov its covariance at 36 i. */
int rsvio_pnp_batch_covariance(rsvio_pnp_batch* b, const rsvio_motion_frame* frames, const double* T_W_B /* n x 16 */,
                               double huber_delta, double* cov /* n x 36 */, rsvio_motion_cov_info* info /* n */,
                               double* device_ms /* may be NULL */);

/* Batched tracker (the serving mode's first leg): n StereoPatchTracker handles and ONE stereo frame
 * per handle tracked by one call -- one upload (the staged host images and the descriptor tables),
 * three launches whatever n is (pyramids + FAST-9 of all 2n images; one LK launch of up to 3n
 * batches: cam0 and cam1 temporal of the streams with history, every stream's stereo cell jobs;
 * append / pack with workgroup i = stream i), one read-back and one host wait.  frames[i]'s lists,
 * n_l, n_r and status are exactly -- byte for byte, ids included -- what
 * rsvio_tracker_process_frame[_device] returns for that frame on handle i, and the handle is left in
 * the state that call leaves (pyramid ping-pong, track maps, counts, output slot), so batch calls and
 * single calls may alternate on a handle, and rsvio_tracker_undistorted, rsvio_tracker_remove_ids,
 * rsvio_track_motion_tracker and rsvio_tracker_device_lists see the batch's frame as the last
 * collected one.  Streams on their first frame and streams with history mix in one call.  A slot's
 * RSVIO_ERR_CAPACITY (lists still consistent) is reported in its status and does not fail the call.
 *   The batch borrows the handles (they must outlive it): 1 <= n <= 1024, all on one device with
 * equal rsvio_tracker_params, each handle in ONE slot only (the call writes its state); it runs on a
 * stream of its own.  Host images (on_device = 0; `stride` bytes per row, 0 meaning width) are
 * staged into the batch's one upload; device images (on_device = 1) are tightly packed, complete on
 * the device before the call, and read in place.  out_l / out_r NULL with capacity 0: that list is
 * not copied to the host (not an error) and n_l / n_r report the device list's length.
 *   Everything is checked before anything is launched or written: a NULL argument, n out of range,
 * a NULL or repeated handle, unequal parameters or devices, a handle with a submitted frame not yet
 * collected, a NULL image, a host stride below the width (a device stride other than 0 or the
 * width) are RSVIO_ERR_INVALID_ARG and rsvio_last_error names the slot.  *device_ms (may be NULL):
 * the call's launches by HIP events. */
typedef struct rsvio_tracker_batch rsvio_tracker_batch;
typedef struct {
    const uint8_t* left;  const uint8_t* right;  /* w x h u8 each */
    size_t stride;                /* host images: bytes per row (>= width); device images: 0 or width */
    rsvio_feature* out_l; size_t cap_l;          /* host lists; NULL with cap 0: not copied, not an error */
    rsvio_feature* out_r; size_t cap_r;
    size_t n_l, n_r;              /* out: as process_frame's *n_l, *n_r (device list length when not copied) */
    int32_t on_device;            /* 0: host images (staged into the batch's one upload); 1: device pointers */
    int32_t status;               /* out: what rsvio_tracker_process_frame would have returned for this slot */
} rsvio_stereo_frame;
int rsvio_tracker_batch_create(rsvio_tracker* const* handles, int32_t n, rsvio_tracker_batch** out);
int rsvio_tracker_batch_process_frames(rsvio_tracker_batch* b, rsvio_stereo_frame* frames, double* device_ms);
void rsvio_tracker_batch_destroy(rsvio_tracker_batch* b);
/* The last collected frame's lists in place on the device (valid until the handle's next-but-one
 * frame, which writes the same output slot): AoS rsvio_feature lists and, with cameras attached
 * (rsvio_tracker_set_cameras), the fused undistorted coordinates as float pairs (NULL without) --
 * e.g. an rsvio_motion_frame with on_device = 1 and id_stride = sizeof(rsvio_feature).  d_uv_l and
 * d_uv_r may be NULL. */
int rsvio_tracker_device_lists(rsvio_tracker* t, const rsvio_feature** d_l, size_t* n_l,
                               const rsvio_feature** d_r, size_t* n_r,
                               const float** d_uv_l, const float** d_uv_r);

/* Stereo gate: an epipolar check on the pairs of every frame, at the frame's end on the device.
 * StereoPatchTracker::process_frame (feature_tracker.rs:116-187) admits a point when the left ->
 * right LK track converges and then tracks cam0 and cam1 of that id independently; nothing checks
 * that the two pixels of an id are views of one 3-D point.  The gate is state of a handle
 * {mode, max_error, T_Cl_Cr}, off by default; a handle without one behaves exactly as before.
 *   T_Cl_Cr: row-major 4 x 4, the right camera's pose in the left camera's frame (x_l = R x_r + t).
 * The host computes E = [t / |t|]x R once in f64 (|t| = sqrt(tx*tx + ty*ty + tz*tz), every entry
 * of E a left-to-right sum over k = 0, 1, 2).
 *   At the end of every frame, after the new points were appended and the ids assigned and before
 * the lists are packed and read back, for every PAIR (an id present in both cameras' maps):
 *   bearing d from the fused unprojection's stored f32 coordinates (x, y) (what
 *     rsvio_tracker_undistorted returns) promoted to f64, per camera convention:
 *       RSVIO_UNPROJ_PLANE  d = (x, y, 1) / sqrt((x*x + y*y) + 1)
 *       RSVIO_UNPROJ_RAY    s = (1 - x*x) - y*y, d = (x, y, sqrt(s)); s < 0: the pair is invalid
 *   error   e = |d_l . (E d_r)|, both products left-to-right sums in f64 without contraction
 *   rejected when a coordinate of either side is NaN (the unprojection failed: invalid, e = NaN),
 *     s < 0 (invalid), or !(e <= max_error).
 *   RSVIO_GATE_DROP_RIGHT  a rejected id leaves cam1's map; cam0 keeps tracking it as a mono point
 *   RSVIO_GATE_DROP_BOTH   it leaves both maps, exactly as rsvio_tracker_remove_ids of that id right
 *                          after the frame would (its grid cell is free for the next detection)
 * Ids present in one camera only are never touched; rejected new points still consume their ids;
 * the overflow flag / RSVIO_ERR_CAPACITY are decided before the gate.  The maps keep ascending ids,
 * and the affines, the packed lists and the undistorted arrays stay aligned; the counts read back
 * are the gated ones.  The gate rides in the frame's last launch (single, look-ahead and batched
 * calls; the handles of a batch may carry different gates): no extra launch, no extra host wait.
 *   rsvio_tracker_set_stereo_gate: gate NULL or mode RSVIO_GATE_OFF turns it off.
 * RSVIO_ERR_INVALID_ARG (rsvio_last_error names the reason): no cameras attached, a mode outside
 * 0..2, max_error not finite or <= 0, a non-finite T, |t| = 0, max |R^T R - I| > 1e-6, a frame in
 * flight.  rsvio_tracker_set_cameras(t, NULL, NULL) is refused while a gate is set.
 *   rsvio_tracker_gate_report: the last collected frame (a batch's frame counts as collected):
 * n_pairs before the gate, n_rejected, n_invalid (a subset of the rejected); the rejected ids
 * ascending, each with its e (NaN for an invalid pair); *n = n_rejected.  cap < *n truncates and
 * returns RSVIO_ERR_CAPACITY -- except ids_out = err_out = NULL with cap = 0, which asks for the
 * counts alone.  Zeros with the gate off.  The counters travel with the frame's counts read-back;
 * the list is fetched by this call (the collected frame's own buffer: a frame submitted since
 * writes another).  counts, ids_out, err_out and n may each be NULL.
 *   rsvio_stereo_gate_lists: the same device function on two arbitrary lists with ascending ids
 * (host buffers, current device; uv: n x 2 f32 stored coordinates; any lengths): keep_l / keep_r
 * 0 or 1 per entry (keep_l all 1 under DROP_RIGHT), err_r[j] = e of right entry j (NaN: unpaired or
 * invalid).  mode must be DROP_RIGHT or DROP_BOTH; ids not strictly ascending within a list, a
 * convention other than RSVIO_UNPROJ_*, or a gate set_stereo_gate would refuse:
 * RSVIO_ERR_INVALID_ARG, checked before any device call.  counts may be NULL. */
enum { RSVIO_GATE_OFF = 0, RSVIO_GATE_DROP_RIGHT = 1, RSVIO_GATE_DROP_BOTH = 2 };
typedef struct { int32_t mode, reserved; double max_error; double T_Cl_Cr[16]; } rsvio_stereo_gate;   /* 144 bytes */
typedef struct { int32_t n_pairs, n_rejected, n_invalid, reserved; } rsvio_gate_counts;               /* 16 bytes */
int rsvio_tracker_set_stereo_gate(rsvio_tracker* t, const rsvio_stereo_gate* gate);
int rsvio_tracker_gate_report(rsvio_tracker* t, rsvio_gate_counts* counts,
                              uint64_t* ids_out, double* err_out, size_t cap, size_t* n);
int rsvio_stereo_gate_lists(const rsvio_stereo_gate* gate, int32_t convention_l, int32_t convention_r,
                            const uint64_t* ids_l, const float* uv_l, size_t n_l,
                            const uint64_t* ids_r, const float* uv_r, size_t n_r,
                            uint8_t* keep_l, uint8_t* keep_r, double* err_r, rsvio_gate_counts* counts);

/* Motion-predicted tracking: the LK search of a feature started where a rotation hint says it went.
 * track_one_point (feature_tracker.rs:292-342) starts the search in the new image at the feature's
 * position in the old one; with a few pyramid levels the capture range is a few pixels at the
 * coarsest level, so a camera that yaws a few degrees between frames loses almost every track.  A
 * rotation hint R = R_cur_prev (a bearing in the current camera frame is R times the bearing in the
 * previous one: an integrated gyro, or the last inter-frame rotation) moves each feature's start.
 *   Seed of a feature at pixel (u, v) of a camera:
 *     (x, y, ok) = the fused unprojection of (u, v) (the stored f32 values)
 *     b = (x, y, 1) (RSVIO_UNPROJ_PLANE) or (x, y, sqrt(max(0, (1 - x*x) - y*y))) (RSVIO_UNPROJ_RAY), f64
 *     q = R b, row-major, each row summed left to right
 *     (u', v') = rsvio_project's projection of q, narrowed to f32
 *   seeded iff ok, the projection is valid, both values are finite, 0 <= u' <= w - 1 and
 *   0 <= v' <= h - 1; otherwise the seed is (u, v) itself and the feature counts as unseeded.
 *   Seeded LK (rsvio_track_points_seeded, and the handle's frame): the forward pass builds its
 * templates at the feature's position as before and starts its search at the seed; the backward pass
 * (images swapped, templates at the forward result fwd) starts at fwd.t - (seed - t0), the inverse
 * prediction; the result is accepted by the same test |t0 - bwd.t|^2 < 0.4.
 *   rsvio_predict_seeds: the seeds of n pixels (host buffers, current device; _d: device pointers,
 * enqueued on `stream`); seeded_out: 1 / 0 per entry.  RSVIO_ERR_INVALID_ARG when
 * max |R^T R - I| > 1e-6 or det R < 0.
 *   rsvio_tracker_set_prediction: the hint of both cameras for EXACTLY the next frame enqueued on the
 * handle (process_frame*, or submit* with collect); that enqueue clears it.  NULL clears a pending
 * one.  Off by default: a handle without a pending prediction launches exactly what it launched
 * before.  It needs rsvio_tracker_set_cameras (RSVIO_ERR_INVALID_ARG without; detaching the cameras
 * clears a pending prediction) and validates both rotations as rsvio_predict_seeds does.  It is host
 * state: it may be set while a frame is in flight and then applies to the next submit.  On a
 * handle's first frame it is consumed without effect.  The predicted frame costs one extra launch
 * (the seeds of both maps) and no extra host wait; the new corners' stereo jobs, the append / pack
 * and the stereo gate are unchanged.
 *   rsvio_tracker_prediction_report: the last collected frame: per camera how many entries of the
 * previous frame's lists were seeded / unseeded (all 0 when that frame had no prediction) and, when
 * seeds_l / seeds_r are given (n x 2 f32, capacities in entries), the seeds in the order of the
 * previous frame's lists; a capacity below the list's length truncates and returns
 * RSVIO_ERR_CAPACITY.  An on-demand read-back with its own wait, from the collected frame's own
 * buffer (a frame submitted since writes another).  counts may be NULL.
 *   rsvio_tracker_batch_process_frames does not seed: a batch holding a handle with a pending
 * prediction is refused (RSVIO_ERR_INVALID_ARG, nothing enqueued, the prediction stays pending). */
typedef struct { double R_l[9]; double R_r[9]; } rsvio_track_prediction;          /* 144 bytes; row-major R_cur_prev */
typedef struct { int32_t n_seeded[2]; int32_t n_unseeded[2]; } rsvio_prediction_counts;   /* 16 bytes; [left, right] */
int rsvio_predict_seeds(const rsvio_camera* cam, const double* R, const float* px, size_t n,
                        int32_t w, int32_t h, float* seeds_out, uint8_t* seeded_out);
int rsvio_predict_seeds_d(const rsvio_camera* cam, const double* R, const float* d_px, size_t n,
                          int32_t w, int32_t h, float* d_seeds_out, uint8_t* d_seeded_out, void* stream);
int rsvio_tracker_set_prediction(rsvio_tracker* t, const rsvio_track_prediction* pred);
int rsvio_tracker_prediction_report(rsvio_tracker* t, rsvio_prediction_counts* counts,
                                    float* seeds_l, size_t cap_l, float* seeds_r, size_t cap_r);

#ifdef __cplusplus
}
#endif
#endif
