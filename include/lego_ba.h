/*
 * lego_ba.h — C ABI of the MI355X sliding-window bundle-adjustment solver.
 *
 * Drop-in boundary for LEGO-SLAM's backend optimisation.
 * The reference builds a `lego::Problem` inside `Backend::Optimize`
 * (src/backend_lego.cpp:57-158), calls `problem.solve(10)` (:161) and then reads
 * each edge's robust chi2 and the vertex estimates back (:163-217).  This ABI
 * replaces exactly that block with one call:
 *
 *     reference                                   this ABI
 *     ---------------------------------------     ----------------------------
 *     lego::Problem problem(SLAM)  problem.h:53   lh_create
 *     addVertex / addEdge          problem.h:65,69 lh_window (flat arrays)
 *     setInitialLambda             problem.h:99   lh_options.lambda_init
 *     setVerbose                   problem.h:104  lh_options.verbose
 *     setStrategyType              problem.h:62   lh_options.strategy
 *     solve(iterations)            problem.cpp:156 lh_solve
 *     edge->getRobustChi2()        base_edge.cpp:33 lh_result.edge_robust_chi2
 *     vertex->getEstimate()        base_vertex.h:34 lh_result.pose_Tcw / lm_xyz
 *     outlier threshold loop       backend_lego.cpp:163-194 lh_result.is_outlier (on the device, ABI 5)
 *                                                                  or lh_classify_outliers (host, on edge_robust_chi2)
 *     Frontend::EstimateCurrentPose frontend_lego.cpp:157-250 lh_estimate_pose (batched)
 *     LKOpticalFlow4Layer / 1Layer  algorithm.cpp:11-206      lh_lk_track
 *     cv::calcOpticalFlowPyrLK      frontend_lego.cpp:383-463 lh_klt_track, lh_klt_stereo_landmarks (the live trackers)
 *     Frontend::Track               frontend_lego.cpp:48-75   lh_track_frame (guesses, KLT, selection, pose: one call per frame)
 *     Frontend::InsertKeyframe      frontend_lego.cpp:77-102  lh_insert_keyframe (DetectFeatures, the right-image KLT and
 *     Frontend::StereoInit          frontend_lego.cpp:323-362                     TriangulateNewPoints: one call per keyframe)
 *     triangulation                 algorithm.h:11-34         lh_triangulate (batched)
 *     Frontend::TriangulateNewPoints frontend_lego.cpp:111-155 lh_stereo_landmarks (LK left -> right + triangulation,
 *     Frontend::BuildInitMap        frontend_lego.cpp:323-362                       one call per stereo frame)
 *     ~Problem                     problem.cpp:32 lh_destroy
 *
 * Plain C types only (no torch, Eigen or Sophus in any signature).  No C++
 * exception crosses the ABI; every entry point returns an lh_status.
 * A handle is single-threaded; use one handle per calling thread (the
 * reference runs one Problem on the backend thread and one on the frontend
 * thread).  Handles share no global state (the reference's global_vertex_id /
 * global_edge_id counters, base_vertex.cpp:5 / base_edge.cpp:6, have no analogue).
 */
#ifndef LEGO_BA_H
#define LEGO_BA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LH_ABI_VERSION 5   /* lh_create accepts 4 and 5; the lh_result fields marked ABI 5 are read only at 5 */

typedef enum lh_status {
    LH_OK = 0,
    LH_E_EMPTY = 1,       /* no vertices or no edges: Problem::solve returns false (problem.cpp:157-161) */
    LH_E_BADARG = 2,      /* null pointer, index out of range, bad option                              */
    LH_E_HIP = 3,         /* HIP runtime error (device missing, OOM, launch failure)                    */
    LH_E_RCCL = 4,        /* RCCL communicator / collective error                                       */
    LH_E_UNSUPPORTED = 5, /* window outside the supported envelope (see DESIGN.md "Limits")            */
    LH_E_STATE = 6,       /* call out of order (e.g. lh_solve_resident before lh_upload)               */
    LH_E_SINGULAR = 7     /* lh_covariance: no free pose, a non-positive pivot, rank-deficient landmarks */
} lh_status;

/* Problem::StrategyType (problem.h:45-50) */
typedef enum lh_strategy { LH_STRATEGY_DEFAULT = 0, LH_STRATEGY_1 = 1 } lh_strategy;

/* Reduced pose-system solver: the reference uses Eigen LDLT (problem.cpp:420);
   PCG is the reference's Jacobi-PCG (Problem::PCGSolver, :584-614), which it left commented out
   (:422), with its first-step bug fixed (:595-596 never add alpha*p to x). */
typedef enum lh_linear_solver { LH_SOLVER_LDLT = 0, LH_SOLVER_PCG = 1 } lh_linear_solver;

/* Arithmetic of the per-edge path.  FP64: double throughout, the residual a bitwise
   mirror of the reference's (lego_types.h:200-216).  FP32_RESID: BASELINE config 3's "fp32 residuals
   + fp64 accumulate" as far as it can be taken without changing the LM decisions: each edge's
   Jacobians (the projection derivative and its chain through the extrinsic and the pose rotation,
   lego_types.h:218-254) in float, widened to double before any product that is summed; the camera
   point, the residual, the Huber weight, rho0, chi2, b's residual factor and the gain ratio stay the
   fp64 mirror, and every sum over edges (H blocks, b, chi2, the Schur complement) is double.  Parity
   to tolerance, not to the bit. */
typedef enum lh_precision { LH_PREC_FP64 = 0, LH_PREC_FP32_RESID = 1 } lh_precision;

/* The per-trial exchange of a landmark-sharded solve (world_size > 1): RCCL on the handle's stream
   (one process per GPU), or a caller-supplied all-reduce over host buffers (any transport: MPI, gloo,
   sockets), called once per LM trial from inside lh_solve on the calling thread, or (LH_COMM_P2P) a one-shot
   exchange on the device: every rank writes its partial reduced system into every rank's IPC-mapped buffer
   (xGMI between GPUs) and sums the ranks' slots in rank order; the caller's all-reduce (as LH_COMM_HOST) then
   only carries the upload-time agreement and the IPC handles.  At most 16 ranks; every rank's device must be
   able to map the others' memory. */
typedef enum lh_comm_mode { LH_COMM_RCCL = 0, LH_COMM_HOST = 1, LH_COMM_P2P = 2 } lh_comm_mode;
/* in-place all-reduce of count doubles over the ranks; op 0 = sum, 1 = max; returns 0 on success */
typedef int (*lh_allreduce_fn)(void *user, double *buf, int64_t count, int32_t op);

typedef struct lh_options {
    int32_t abi_version;      /* LH_ABI_VERSION (4 is still accepted: no ABI-5 lh_result fields)   */
    int32_t max_iters;        /* outer LM iterations, solve(10)          backend_lego.cpp:161 */
    int32_t max_trials;       /* false_cnt_threshold = 10                problem.cpp:178      */
    int32_t strategy;         /* lh_strategy                             problem.h:45         */
    double huber_delta;       /* HuberCost(5.991); <= 0: no robust kernel backend_lego.cpp:92-94 */
    double stop_dchi2;        /* diffChiThreshold_ = 1e-5 (absolute)     problem.h:165        */
    double tau;               /* 1e-5                                    problem.cpp:495      */
    double lambda_cap;        /* 5e10                                    problem.cpp:494      */
    double lambda_init;       /* < 0: computed; >= 0: setInitialLambda   problem.h:99-102     */
    int32_t linear_solver;    /* lh_linear_solver                                             */
    int32_t verbose;          /* print the reference's per-iteration line problem.cpp:180-184 */
    int32_t device;           /* HIP device ordinal, -1 = current device                      */
    int32_t world_size;       /* landmark shards (one process per GPU); 1 = single GPU.  Every rank
                                 must pass the same solver options (iteration caps, strategy, Huber
                                 delta, tolerances, solver, gate, depth): lh_create compares them
                                 across the ranks with one MAX all-reduce and returns LH_E_BADARG on
                                 every rank when they differ (the collective count per solve is a
                                 function of them)                                               */
    int32_t rank;             /* this process's shard                                         */
    int32_t degenerate_guard; /* 0: reference semantics: a landmark with one edge (rank-2 H_ll) or a
                                 non-positive-definite H_ll poisons the step, as the LU inverse's
                                 inf does (problem.cpp:396-400; the solve then rejects every trial);
                                 1: such landmarks are held fixed (no Schur term, no update)   */
    int32_t trials_per_sync;  /* LM trials kept enqueued past the last one the device has decided (0: auto = 2; one while the next completed iteration reaches max_iters) */
    int32_t profile;          /* 1: time every kernel with HIP events (lh_kernel_stats)       */
    int32_t pcg_max_iters;    /* PCG: iteration cap; <= 0: 2 * rows (problem.cpp:422)          */
    double pcg_tol;           /* PCG: stop when ||r|| <= pcg_tol * ||b|| (1e-6, problem.cpp:597) */
    uint8_t comm_id[128];     /* ncclUniqueId from lh_comm_unique_id on rank 0 (world_size>1) */
    /* ---- ABI 3 ---- */
    int32_t gate_mode;        /* 0: the reference's Huber gate rho1 + 2 rho2 e2 > 0 (base_edge.cpp:55);
                                 1: diagnostic, its analytically-zero residue on outlier edges taken
                                 as 0 (the oracle's gate_mode 1; parity tests only)            */
    int32_t chunk_landmarks;  /* landmarks per k_lin chunk; 0 = auto (~2 workgroups per CU)     */
    int32_t comm_mode;        /* lh_comm_mode (world_size > 1)                                  */
    int32_t host_threads;     /* window-preprocessing threads; 0 = auto (the CPUs this process may
                                 use: affinity mask capped by the cgroup CPU quota, <= 8)        */
    lh_allreduce_fn allreduce;  /* LH_COMM_HOST: the exchange                                    */
    void *allreduce_user;       /* its first argument                                            */
    /* ---- ABI 4 ---- */
    int32_t precision;        /* lh_precision (default LH_PREC_FP64)                             */
} lh_options;

/*
 * One sliding window.  Caller-owned, read-only during the call.
 * Order contract: poses in ascending keyframe id and landmarks in ascending
 * landmark id, i.e. the reference's ordering (Problem::setOrdering,
 * problem.cpp:234-255: std::map by vertex id, poses first).  Observation order
 * is free (the reference's is unordered_map hash order).
 */
typedef struct lh_window {
    int32_t n_poses;
    const double *pose_Tcw;    /* [n_poses][12] row-major [R | t], T_cw (VertexPose estimate, lego_types.h:37,57) */
    const uint8_t *pose_fixed; /* [n_poses] or NULL; nonzero = BaseVertex::setFixed (base_vertex.h:50)              */
    int32_t n_landmarks;
    const double *lm_xyz;      /* [n_landmarks][3] world position (VertexXYZ, lego_types.h:97-115) */
    int64_t n_obs;
    const uint32_t *obs_pose;  /* [n_obs] pose index                                                */
    const uint32_t *obs_lm;    /* [n_obs] landmark index                                            */
    const uint8_t *obs_cam;    /* [n_obs] camera index or NULL (all camera 0)                       */
    const double *obs_uv;      /* [n_obs][2] pixel measurement: toVec2 of cv::KeyPoint::pt (algorithm.h:37),
                                  i.e. float values widened; a value no float holds exactly (or a NaN) is
                                  LH_E_BADARG (the device keeps the pixels as floats)                 */
    double K[4];               /* fx, fy, cx, cy (Camera::K, camera.h:36-41)                         */
    int32_t n_cams;            /* number of extrinsics in cam_ext (0 with cam_ext NULL = identity)   */
    const double *cam_ext;     /* [n_cams][12] row-major [R | t] camera extrinsic (Camera::pose_)    */
} lh_window;

typedef struct lh_result {
    /* caller-owned outputs; any pointer may be NULL */
    double *pose_Tcw;          /* [n_poses][12]                                                   */
    double *lm_xyz;            /* [n_landmarks][3]                                                */
    double *edge_robust_chi2;  /* [n_obs] rho0 of the residuals as last evaluated, window order
                                  (stale after an all-rejected exit, as backend_lego.cpp:171 sees) */
    double *trace_chi2;        /* [trace_cap] currentChi_ at the top of each outer iteration       */
    double *trace_lambda;      /* [trace_cap] currentLambda_ at the same point                     */
    int32_t trace_cap;
    /* scalar outputs */
    int32_t trace_len;
    int32_t iterations;        /* outer LM iterations completed (problem.cpp:207)                  */
    int32_t trials;            /* solveLinearEquation calls                                        */
    int32_t accepted;          /* accepted trials                                                  */
    double chi2_initial;       /* 0.5 * sum rho0 at the input state (problem.cpp:475-479)          */
    double chi2_final;         /* currentChi_ at exit                                              */
    double lambda_final;
    double time_ms;            /* wall time of the LM solve on the device (excludes upload); host
                                  clock from the first launch to the stop when no array is requested */
    int32_t pcg_iterations;    /* PCG iterations summed over all trials (0 with LH_SOLVER_LDLT)    */
    int32_t degenerate;        /* landmarks with a rank-deficient H_ll at the initial linearisation */
    double time_prep_ms;       /* lh_solve / lh_upload: host preprocessing of the window           */
    double time_upload_ms;     /* lh_solve / lh_upload: preprocessing + host-to-device copies      */
    double time_download_ms;   /* device-to-host copies of the requested outputs                   */
    /* ---- ABI 5 (read only when lh_options.abi_version >= 5) ---- */
    uint8_t *is_outlier;       /* [n_obs] window order, or NULL.  Backend::Optimize's outlier pass
                                  (backend_lego.cpp:163-194) on the device over rho0 as last evaluated:
                                  starting from outlier_chi2_th, the threshold doubles (at most 5 times)
                                  while the inlier ratio is <= 0.5, then is_outlier = rho0 > threshold.
                                  Only the flags cross the link (edge_robust_chi2 may stay NULL); the
                                  same result as lh_classify_outliers on edge_robust_chi2          */
    double outlier_chi2_th;    /* in: the pass's starting threshold (the reference's 5.991, :92)  */
    double outlier_th;         /* out: the threshold after the doubling loop                       */
    int64_t n_inlier;          /* out: the loop's last counts (the reference's LOG line, :196)     */
    int64_t n_outlier;
} lh_result;

typedef struct lh_kernel_stats {
    int64_t launches[8];       /* per kernel class, see lh_kernel_name                             */
    double total_ms[8];
} lh_kernel_stats;

typedef struct lh_handle lh_handle;

const char *lh_strerror(int status);
/* The defaults for a caller built against ABI `abi` (its LH_ABI_VERSION at compile time): abi_version = abi, so the
   library reads exactly the lh_result fields that caller's struct has.  Callers write lh_default_options(&opt),
   which this header maps to lh_default_options_v(&opt, LH_ABI_VERSION).  The plain symbol lh_default_options,
   which binaries built against the ABI-4 header call, fills abi_version = 4 (no ABI-5 fields read). */
void lh_default_options_v(lh_options *opt, int abi);
void lh_default_options(lh_options *opt);
#define lh_default_options(opt) lh_default_options_v((opt), LH_ABI_VERSION)
const char *lh_kernel_name(int kernel_class);

/* RCCL: rank 0 creates the id and ships it to the other ranks (any transport). */
int lh_comm_unique_id(uint8_t out[128]);

int lh_create(lh_handle **h, const lh_options *opt);
void lh_destroy(lh_handle *h);

/* Host-buffer path: upload, solve, download.  The drop-in for problem.solve(). */
int lh_solve(lh_handle *h, const lh_window *in, lh_result *out);

/* Device-resident path (bench): lh_upload preprocesses and copies the window
   once; every lh_solve_resident restarts from the uploaded initial state.
   A solve that requests no array (pose_Tcw, lm_xyz, edge_robust_chi2 all NULL) returns as soon as
   the device has stopped the LM loop: its scalars and trace come with the stop flag in mapped
   host memory, and the kernels still draining are stream-ordered before any later call on the
   handle (lh_destroy synchronises). */
int lh_upload(lh_handle *h, const lh_window *in);
int lh_solve_resident(lh_handle *h, lh_result *out);

int lh_kernel_stats_get(lh_handle *h, lh_kernel_stats *out);
int lh_set_profiling(lh_handle *h, int on);   /* toggle lh_options.profile on a live handle */
void lh_kernel_stats_reset(lh_handle *h);

/*
 * Backend::Optimize outlier pass (backend_lego.cpp:163-194): starting from
 * chi2_th, double the threshold (at most 5 times) while the inlier ratio is
 * <= 0.5, then flag edges with robust chi2 > threshold.  is_outlier may be NULL.
 */
int lh_classify_outliers(const double *edge_robust_chi2, int64_t n_obs, double chi2_th,
                         uint8_t *is_outlier, double *th_out, int64_t *n_inlier, int64_t *n_outlier);

/*
 * Frontend pose-only LM: Frontend::EstimateCurrentPose
 * (src/frontend_lego.cpp:157-250) for a batch of independent frames.  Per frame:
 * one VertexPose, one EdgeProjectionPoseOnly per observation (lego_types.h:116-180),
 * four rounds of problem.solve(max_iters) each restarting from the frame's pose,
 * the outlier flags refreshed after each round (robust chi2 > 5.991, :205-226;
 * flagged features recomputed at the final estimate first), Huber(huber_delta) on
 * rounds one to three and none on round four (:223-225).  Flags never remove an
 * edge (the reference's setLevel is commented out).  Uses the handle's options
 * (max_iters, max_trials, strategy, huber_delta, stop_dchi2, tau, lambda_cap,
 * lambda_init); one workgroup per frame, the whole batch in one launch.
 */
typedef struct lh_frames {
    int32_t n_frames;
    const int64_t *obs_ptr;     /* [n_frames + 1] CSR: frame f owns observations [obs_ptr[f], obs_ptr[f+1]) */
    const double *pose_Tcw;     /* [n_frames][12] row-major [R | t]: current_frame_->Pose()           */
    const double *pts_w;        /* [n_obs][3] map-point world positions (mp->pos_)                     */
    const double *obs_uv;       /* [n_obs][2] feature pixels (toVec2(feat->position_.pt))              */
    const uint8_t *is_outlier;  /* [n_obs] the features' is_outlier_ on entry, or NULL (all false)     */
    double K[4];                /* fx, fy, cx, cy (camera_left_->K())                                   */
} lh_frames;

typedef struct lh_frames_result {
    double *pose_Tcw;           /* [n_frames][12] SE3(vertex_pose->getEstimate()) after round four     */
    uint8_t *is_outlier;        /* [n_obs] flags after round four, or NULL                             */
    double *edge_chi2;          /* [n_obs] chi2 the last classification compared with 5.991, or NULL  */
    int32_t *n_inliers;         /* [n_frames] EstimateCurrentPose's return value, or NULL               */
    int32_t *iterations;        /* [n_frames] LM iterations summed over the four rounds, or NULL       */
    double time_ms;             /* device time of the batch (upload and download excluded)             */
} lh_frames_result;

int lh_estimate_pose(lh_handle *h, const lh_frames *in, lh_frames_result *out);

/*
 * Gauss-Newton pyramidal LK optical flow, replacing
 *   void LKOpticalFlow4Layer(const cv::Mat &img1, const cv::Mat &img2,
 *                            const std::vector<cv::KeyPoint> &kp1, std::vector<cv::KeyPoint> &kp2,
 *                            std::vector<bool> &success, bool inverse, bool has_initial)
 *                                                                      (src/algorithm.cpp:128-206)
 * (levels = 4) and LKOpticalFlow1Layer (algorithm.cpp:11-31, levels = 1), as the frontend's
 * *LKOpticalFlow4LayerSelf trackers call them (frontend_lego.cpp:466-556).  Images are 8-bit gray
 * (CV_8UC1 layout: rows of `step` bytes); keypoints are cv::KeyPoint::pt.  The pyramid is built as
 * cv::resize(INTER_LINEAR, 0.5) does (exactly for even-sized levels; see oracle/lk_oracle.c).
 * Semantics as written, including inverse mode's single J variable (from iteration 1 on every
 * patch pixel uses the last pixel's J, algorithm.cpp:73-78).  kp2 and success are overwritten;
 * with has_initial, kp2 holds the initial guess on entry.
 */
typedef struct lh_lk_input {
    int32_t cols, rows;         /* level-0 image size                                                */
    int64_t step;               /* bytes per image row (>= cols)                                      */
    const uint8_t *img1;        /* [rows][step] previous / left image                                 */
    const uint8_t *img2;        /* [rows][step] current / right image                                 */
    int32_t n_points;
    const float *kp1;           /* [n_points][2] keypoints in img1                                    */
    int32_t inverse;            /* 0: forward (the frontend's mode), 1: inverse                       */
    int32_t has_initial;        /* kp2 on entry is the initial guess                                  */
    int32_t levels;             /* 4 (LKOpticalFlow4Layer) or 1 (LKOpticalFlow1Layer)                  */
} lh_lk_input;

typedef struct lh_lk_result {
    float *kp2;                 /* [n_points][2] in: initial guess (has_initial); out: tracked points */
    uint8_t *success;           /* [n_points] out                                                     */
    double time_ms;             /* device time: pyramid + tracking (copies excluded)                  */
} lh_lk_result;

int lh_lk_track(lh_handle *h, const lh_lk_input *in, lh_lk_result *out);

/*
 * Batched SVD triangulation, replacing
 *   bool triangulation(const std::vector<SE3> &poses, const VecVec3 &points, Vec3 &pt_world,
 *                      double singRatioThr = 1e-3)                  (include/legoslam/algorithm.h:11-34)
 * as Frontend::TriangulateNewPoints (src/frontend_lego.cpp:111-155) and Frontend::BuildInitMap (:323-362) call it
 * once per stereo feature.  Per point: two rows of A per view, x m.row(2) - m.row(0) and y m.row(2) - m.row(1)
 * (:18-22), with (x, y) the view's normalised camera coordinates (Camera::pixel2camera at depth 1,
 * src/camera.cpp:21-25, when cam_K is given); the right singular vector v of A's smallest singular value;
 * pt = v[0..2] / v[3] (:24).  One lane per point in fp64; a point's result depends on nothing but its own views
 * (the same bits at any batch position and batch size).  Any number (>= 2) of views per point.
 *
 * flags, 0 = accepted:
 *   bit 0  a component of pt is NaN or infinite                       algorithm.h:26-28
 *   bit 1  !(sigma3 / sigma2 < sing_ratio_thr)                        algorithm.h:30-33
 *          (a NaN ratio fails, as in the reference; the ratio is NaN when sigma2 <= 4 eps sigma0, i.e. A has two
 *          null directions to working precision, as with two identical views: the reference's quotient of two
 *          rounding-noise values is replaced by a definite rejection)
 *   bit 2  gate: !(pt[1] <= y_max)                                    frontend_lego.cpp:134
 *   bit 3  gate: !(pt[2] > z_min && pt[2] <= z_max)                   frontend_lego.cpp:135
 *   bit 4  lh_stereo_landmarks: the LK track failed; the point is not triangulated (pt = 0)
 *   bit 5  lh_insert_keyframe (LH_TRI_F_HAS_POINT): the feature already has a map point; not triangulated (pt = 0)
 * Every test is evaluated (the reference stops at its first failure, so a rejected point may carry several bits),
 * the gate on pt before T_out.  With T_out and flags == 0, pt <- T_out * pt (current_pose_Twc * pworld, :138);
 * a rejected point keeps its untransformed value.
 *
 * LH_E_BADARG: a null required pointer, a point with fewer than 2 views (the reference would read V.col(3) of a
 * 2x4 system), a pose index out of range, a view_ptr that does not start at >= 0 or decreases.  n_points == 0: LH_OK.
 */
typedef struct lh_tri_input {
    int32_t n_points;
    int32_t n_poses;
    const double *pose_Tcw;     /* [n_poses][12] row-major [R|t]: Camera::pose() of each view's camera (or any SE3) */
    const double *cam_K;        /* [n_poses][4] fx,fy,cx,cy: view_xy holds pixels; NULL: already normalised */
    const int64_t *view_ptr;    /* [n_points+1] CSR over views; NULL: every point has n_poses views, view v uses pose v */
    const uint32_t *view_pose;  /* [n_views] pose index (ignored when view_ptr is NULL) */
    const double *view_xy;      /* [n_views][2] */
    double sing_ratio_thr;      /* singRatioThr = 1e-3, algorithm.h:14 */
    int32_t gate;               /* 1: apply y_max / z_min / z_max (frontend_lego.cpp:133-136) */
    double y_max, z_min, z_max;
    const double *T_out;        /* [12] or NULL */
} lh_tri_input;
typedef struct lh_tri_result {
    double *pt;                 /* [n_points][3] */
    uint8_t *flags;             /* [n_points] 0 = accepted; bits as above */
    double *sing_ratio;         /* [n_points] sigma3/sigma2, or NULL */
    int32_t n_accepted;
    double time_ms;             /* device time, copies excluded */
} lh_tri_result;
int lh_triangulate(lh_handle *h, const lh_tri_input *in, lh_tri_result *out);

/*
 * One stereo frame's new landmarks without a host round trip: lh_lk_track from the left image (lk.img1, lk.kp1)
 * to the right (lk.img2), then lh_triangulate on every tracked pair, reading kp1 and kp2 on the device (floats
 * widened to double, as toVec2 does, algorithm.h:37).  View 0 is the left camera (pose_Tcw[0], cam_K[0]), view 1
 * the right.  kp2 and success are bitwise lh_lk_track's; pt and flags are bitwise lh_triangulate's on them; a point
 * whose track failed carries flag bit 4 alone.  out->kp2 holds the initial guess when lk.has_initial.
 */
typedef struct lh_stereo_input {
    lh_lk_input lk;             /* img1 = left, img2 = right */
    const double *pose_Tcw;     /* [2][12] camera_left_->pose(), camera_right_->pose() */
    const double *cam_K;        /* [2][4] fx,fy,cx,cy of the two cameras; NULL: the keypoints are already normalised */
    double sing_ratio_thr;
    int32_t gate;
    double y_max, z_min, z_max;
    const double *T_out;        /* [12] or NULL */
} lh_stereo_input;
typedef struct lh_stereo_result {
    float *kp2;                 /* [n_points][2] */
    uint8_t *success;           /* [n_points] */
    double *pt;                 /* [n_points][3] */
    uint8_t *flags;             /* [n_points] */
    int32_t n_accepted;
    double time_ms;             /* device time: pyramid + tracking + triangulation (copies excluded) */
} lh_stereo_result;
int lh_stereo_landmarks(lh_handle *h, const lh_stereo_input *in, lh_stereo_result *out);

/*
 * Pyramidal KLT tracking, replacing the call the live frontend makes twice per frame
 * (Frontend::TrackLastFrameLKOpticalFlowOpenCV and FindFeaturesInRightLKOpticalFlowOpenCV, src/frontend_lego.cpp:383-463):
 *   cv::calcOpticalFlowPyrLK(img1, img2, kps1, kps2, status, err, cv::Size(11, 11), 3,
 *                            TermCriteria(COUNT + EPS, 30, 0.01), OPTFLOW_USE_INITIAL_FLOW)
 * The window is 11 x 11, the images 8-bit gray.  The tracker is defined here, after OpenCV 4's scalar path
 * (lkpyramid.cpp), in arithmetic that leaves nothing to a compiler or a SIMD width: "float" is IEEE binary32, every
 * float operation below is one correctly rounded operation, and no product and sum is contracted into an FMA.
 * OpenCV's own float sums run in SIMD order, so parity with OpenCV itself is not specified to the bit and is
 * unverified (DESIGN.md 2.5c lists where the two can differ).
 *
 *   pyramid      level 0 is the image; level l+1 has size ((cols+1)/2, (rows+1)/2) and
 *                  dst(x, y) = (sum_{i,j=-2..2} w_i w_j src(r(2x+i), r(2y+j)) + 128) >> 8,  w = (1, 4, 6, 4, 1),
 *                r = BORDER_REFLECT_101.  Level l+1 is built while l < max_level and both its sizes are > 11
 *                (buildOpticalFlowPyramid); L is the last level.  Both images get the same pyramid.
 *   reads        I (img1) and J (img2) outside the image return the REFLECT_101 pixel (offsets reach 11 past an edge).
 *   derivatives  of I, Scharr, REFLECT_101 neighbours at the edge:
 *                  t0(x,y) = 3 (I(x,y-1) + I(x,y+1)) + 10 I(x,y),  Ix(x,y) = t0(x+1,y) - t0(x-1,y)
 *                  t1(x,y) = I(x,y+1) - I(x,y-1),                  Iy(x,y) = 3 (t1(x-1,y) + t1(x+1,y)) + 10 t1(x,y)
 *                A derivative read at a position outside the image is 0 (the BORDER_CONSTANT border of the buffer).
 *   per point    status = 1, kp2 = the guess (kp1 without has_initial).  For l = L down to 0, sc = (float)(1 / 2^l):
 *                p = kp1 sc;  q = kp2 sc if l = L, else 2 kp2;  kp2 = q.  "fail": status = 0 if l = 0; next level.
 *     1  p -= 5;  ip = floor(p);  !(ip.x >= -11 && ip.x < cols_l && ip.y >= -11 && ip.y < rows_l), in float: fail
 *     2  weights of (p, ip):  a = p.x - ip.x, b = p.y - ip.y,  w00 = rint(((1-a)(1-b)) 16384),  w01 = rint((a (1-b)) 16384),
 *        w10 = rint(((1-a) b) 16384) (half to even),  w11 = 16384 - w00 - w01 - w10
 *     3  for the 121 window pixels (x, y = 0..10), bil(F) = F(ip+(x,y)) w00 + F(ip+(x+1,y)) w01 + F(ip+(x,y+1)) w10 +
 *        F(ip+(x+1,y+1)) w11:  Iw = (bil(I) + 256) >> 9,  ix = (bil(Ix) + 8192) >> 14,  iy = (bil(Iy) + 8192) >> 14
 *     4  S11 = sum ix ix, S12 = sum ix iy, S22 = sum iy iy (exact);  A11 = (float)(double)S11 2^-20, A12, A22 likewise;
 *        D = A11 A22 - A12 A12;  d = A11 - A22;  minEig = ((A22 + A11) - sqrt(d d + (4 A12) A12)) / 242;
 *        (double)minEig < min_eig_threshold or D < FLT_EPSILON: fail.  D = 1 / D
 *     5  q -= 5;  prev = 0.  For j = 0 .. max_iters - 1:
 *        1  iq = floor(q);  the range test of 1: if it fails, status = 0 if l = 0, and the loop ends
 *        2  weights of (q, iq);  Jw = (bil(J) + 256) >> 9;  diff = Jw - Iw
 *        3  B1 = sum diff ix, B2 = sum diff iy (exact, in 64 bits);  b1 = (float)(double)B1 2^-20, b2 likewise
 *        4  delta = ((A12 b2 - A22 b1) D, (A12 b1 - A11 b2) D)
 *        5  q += delta;  kp2 = q + 5
 *        6  in double, delta.x^2 + delta.y^2 <= epsilon^2: the loop ends
 *        7  j > 0 and (double)|delta.x + prev.x| < 0.01 and (double)|delta.y + prev.y| < 0.01 (the sums in float):
 *           kp2 -= 0.5 delta, and the loop ends
 *        8  prev = delta
 * The err output of OpenCV is not computed (the reference discards it).  status is cleared at level 0 only, and a
 * tracked point may lie outside the image with status 1, both as in OpenCV.  A NaN or infinite keypoint or guess gives
 * success 0 and is no error.  out->kp2 holds the guess on entry with has_initial; kp2, success and time_ms are
 * lh_lk_track's.
 *
 * LH_E_BADARG: cols < 12 or rows < 12, step < cols, max_level outside 0..3, max_iters < 1, an epsilon that is not > 0,
 * a min_eig_threshold that is not >= 0 (NaN included), n_points < 0, a null pointer with n_points > 0.
 * n_points == 0: LH_OK.
 */
typedef struct lh_klt_input {
    int32_t cols, rows;         /* level-0 image size (>= 12)                                         */
    int64_t step;               /* bytes per image row (>= cols)                                      */
    const uint8_t *img1;        /* [rows][step] previous / left image                                 */
    const uint8_t *img2;        /* [rows][step] current / right image                                 */
    int32_t n_points;
    const float *kp1;           /* [n_points][2] keypoints in img1                                    */
    int32_t has_initial;        /* kp2 on entry is the guess (OPTFLOW_USE_INITIAL_FLOW)               */
    int32_t max_level;          /* 0..3; the reference: 3                                             */
    int32_t max_iters;          /* >= 1; the reference: 30                                            */
    double epsilon;             /* > 0; the reference: 0.01                                           */
    double min_eig_threshold;   /* >= 0; the reference: 1e-4 (OpenCV's default)                       */
} lh_klt_input;
int lh_klt_track(lh_handle *h, const lh_klt_input *in, lh_lk_result *out);

/*
 * lh_stereo_landmarks with this tracker: lh_klt_track from the left image (klt.img1, klt.kp1) to the right (klt.img2),
 * then lh_triangulate on every tracked pair where the tracker left them on the device.  kp2 and success are bitwise
 * lh_klt_track's; pt and flags are bitwise lh_triangulate's on them; a failed track carries flag bit 4 alone.
 */
typedef struct lh_klt_stereo_input {
    lh_klt_input klt;           /* img1 = left, img2 = right */
    const double *pose_Tcw;     /* as lh_stereo_input's, from here on */
    const double *cam_K;
    double sing_ratio_thr;
    int32_t gate;
    double y_max, z_min, z_max;
    const double *T_out;
} lh_klt_stereo_input;
int lh_klt_stereo_landmarks(lh_handle *h, const lh_klt_stereo_input *in, lh_stereo_result *out);

/*
 * Shi-Tomasi corner detection, replacing Frontend::DetectFeatures (src/frontend_lego.cpp:292-310): a mask with a
 * box of +-10 pixels cleared around every feature the frame already has (:294-297), then
 *   gftt_ = cv::GFTTDetector::create(num_features, 0.01, 20);  gftt_->detect(left_img, keypoints, mask)  (:16, :300)
 * i.e. cv::goodFeaturesToTrack with blockSize 3, the Sobel aperture 3 and no Harris detector.  The quantities are
 * OpenCV's, defined in exact arithmetic (OpenCV's own float32 path is not specified to the bit):
 *   gx, gy     integer Sobel 3x3 gradients of the 8-bit image, BORDER_REFLECT_101
 *   A, B, C    the sums of gx gx, gx gy, gy gy over the 3x3 block, the product images extended by REFLECT_101
 *   lambda     (double)(A + C) - sqrt((double)((A - C)^2 + 4 B^2)): 2 * 3060^2 times cornerMinEigenVal's value
 *   allowed    the mask byte is nonzero and the pixel lies in no box [rint(p - half), rint(p + half)] of an
 *              exclusion point p (float32 arithmetic, round half to even, both ends inclusive, clipped to the image)
 *   lambda_max the largest lambda over allowed pixels, border pixels included; none, or lambda_max <= 0: no corners
 *   candidates allowed pixels with 1 <= x <= cols - 2, 1 <= y <= rows - 2, lambda > quality_level * lambda_max and
 *              lambda >= each of the 8 neighbours' (whatever their mask; equal neighbours both stay)
 *   selection  in descending lambda, ties to the larger y * cols + x first (OpenCV 4): a candidate is accepted unless
 *              an accepted one lies at a squared distance < min_distance^2; min_distance < 1: all are accepted
 * kp holds the first max_corners accepted points in that order as (x, y), usable as lh_lk_input.kp1
 * (cv::KeyPoint::size, 3, is not returned).  With max_corners <= 0 there is no limit: at most kp_capacity corners
 * are written and n_corners is the true count.
 *
 * LH_E_BADARG: a null required pointer, cols < 3 or rows < 3, rows * cols > INT32_MAX, step < cols (mask_step
 * likewise), a negative count, kp_capacity < max_corners when max_corners > 0, a negative or NaN quality_level or
 * min_distance.
 */
typedef struct lh_detect_input {
    int32_t cols, rows;
    int64_t step;               /* bytes per image row (>= cols) */
    const uint8_t *img;         /* [rows][step] 8-bit gray */
    const uint8_t *mask;        /* [rows][mask_step] nonzero: allowed; NULL: all allowed */
    int64_t mask_step;
    int32_t n_exclude;
    const float *exclude_pt;    /* [n_exclude][2] position_.pt of the frame's existing features */
    float exclude_half;         /* 10 (frontend_lego.cpp:295-296) */
    int32_t max_corners;        /* num_features = 150; <= 0: no limit */
    double quality_level;       /* 0.01 */
    double min_distance;        /* 20 */
} lh_detect_input;
typedef struct lh_detect_result {
    float *kp;                  /* [kp_capacity][2] */
    int32_t kp_capacity;
    double *response;           /* [kp_capacity] lambda of each corner, or NULL */
    double *eig;                /* [rows][cols] the whole lambda image, or NULL (tests) */
    int32_t n_corners;
    int32_t n_candidates;
    double lambda_max;          /* 0 when no pixel is allowed */
    double time_ms;             /* device time, first kernel to last (the host's checks between selection rounds
                                   included; copies of the inputs and outputs excluded) */
} lh_detect_result;
int lh_detect_features(lh_handle *h, const lh_detect_input *in, lh_detect_result *out);

/*
 * One frame of Frontend::Track (src/frontend_lego.cpp:48-75) without a host step in between: the tracker's guesses
 * (TrackLastFrameLKOpticalFlowOpenCV, :383-398), lh_klt_track last-left -> current-left (:402-406), the tracked features
 * that carry a map point (:408-417), and lh_estimate_pose on them (EstimateCurrentPose, :157-258).  One upload besides
 * the image(s), one download, one synchronise.
 *
 *   guess    feature i with has_point, X = pts_w[i], T = pose_Tcw, E = cam_ext, every operation one correctly rounded
 *            binary64 operation and none contracted into an FMA:
 *              Pb_r = ((T[r][0] X0 + T[r][1] X1) + T[r][2] X2) + T[r][3]          r = 0..2
 *              Pc_r = ((E[r][0] Pb0 + E[r][1] Pb1) + E[r][2] Pb2) + E[r][3]       (world2camera, src/camera.cpp:8-14)
 *              u = (fx Pc0) / Pc2 + cx,  v = (fy Pc1) / Pc2 + cy                    (camera2pixel, camera.cpp:16-19)
 *            and the guess is ((float)u, (float)v), round to nearest even, a value past FLT_MAX +-inf.  Without
 *            has_point the guess is kp1[i] (:395-396).  A NaN or infinite guess is no special case: lh_klt_track gives
 *            it success 0.  The reference forms pose_ * T_c_w first, as a Sophus quaternion product; the two orders
 *            agree to rounding before the conversion to float.  Parity with Sophus to the bit is unverified, like every
 *            other Sophus / OpenCV statement in this header.
 *   track    lh_klt_track on (img1, img2, kp1) with those guesses (has_initial) and klt's parameters: kp2 and success
 *            are bitwise the values it would return.
 *   select   the edges are the features with success[i] && has_point[i], in ascending i: the order features_left_ gets
 *            (:409-416) and EstimateCurrentPose walks it in (:179-197).  An edge has the point pts_w[i], the measurement
 *            ((double)kp2[i].x, (double)kp2[i].y) (toVec2) and the entry flag 0.
 *   pose     lh_estimate_pose on that one frame from pose_Tcw, with K and the handle's options: pose_Tcw, the edges'
 *            flags and chi2, n_inliers and iterations are bitwise its outputs.  With no edge Problem::solve returns
 *            false: out->pose_Tcw is the input bit for bit and n_inliers = iterations = 0.
 *
 * The resident image.  The call keeps img2 and its pyramid in buffers of its own, which no other entry point reads or
 * writes.  klt.img1 == NULL means the img2 of the previous successful lh_track_frame on this handle: LH_E_STATE if
 * there is none, or if its cols / rows differ from this call's.  An argument error leaves the resident image as it
 * was; a call that fails after it began to enqueue invalidates it.  n_points == 0 is LH_OK with pose_Tcw copied
 * through and the counts 0; img1 is then not looked at, and a non-NULL img2 still becomes resident (uploaded, its
 * pyramid built): the priming call after StereoInit.
 *
 * LH_E_BADARG: lh_klt_track's argument errors (on img2, and on img1 when given), a null pts_w when some feature can
 * have a point, a null kp2 or success with n_points > 0.
 */
typedef struct lh_track_input {
    lh_klt_input klt;         /* img1 = last_frame_->left_img_ (NULL: the resident image), img2 = current_frame_->left_img_,
                                 kp1 = the last frame's features_left_; klt.has_initial is not read (the guesses are made
                                 here); klt.step describes img2, and img1 when given */
    const double *pts_w;      /* [n_points][3] mp->pos_ of each feature; read only where has_point */
    const uint8_t *has_point; /* [n_points] nonzero: kp->map_point_.lock(); NULL: every feature has one */
    double pose_Tcw[12];      /* current_frame_->Pose() on entry: relative_motion_ * last_frame_->Pose() (:50) */
    double cam_ext[12];       /* camera_left_->pose(), row-major [R|t] */
    double K[4];              /* fx, fy, cx, cy */
} lh_track_input;
typedef struct lh_track_result {
    float *kp2;               /* [n_points][2] tracked positions (required when n_points > 0) */
    uint8_t *success;         /* [n_points]     (required when n_points > 0) */
    double pose_Tcw[12];      /* the pose after EstimateCurrentPose's round four */
    uint8_t *is_outlier;      /* [n_points] or NULL: the feature's flag after round four; 0 for a feature that was no edge */
    double *edge_chi2;        /* [n_points] or NULL: lh_frames_result.edge_chi2 of the feature's edge; 0.0 for no edge */
    int32_t n_tracked;        /* num_good_pts (:408-417) */
    int32_t n_edges;          /* features.size() in EstimateCurrentPose */
    int32_t n_inliers;        /* its return value (tracking_inliers_) */
    int32_t iterations;       /* LM iterations over the four rounds */
    double time_ms;           /* HIP-event bracket, first kernel to last, copies excluded */
} lh_track_result;
int lh_track_frame(lh_handle *h, const lh_track_input *in, lh_track_result *out);

/*
 * A keyframe's half of the frame without a host step in between: Frontend::InsertKeyframe (src/frontend_lego.cpp:77-102)
 * and StereoInit / BuildInitMap (:323-362) run DetectFeatures (:292-310), the right-image guesses and
 * cv::calcOpticalFlowPyrLK left -> right (FindFeaturesInRightLKOpticalFlowOpenCV, :423-463) and TriangulateNewPoints
 * (:111-155).  One upload besides the image(s), one download; the host waits only where lh_detect_features already does
 * (between batches of selection rounds) and at the end.  The call is defined by the composition it equals bit for bit:
 *
 *   detect       corners c_0 .. c_{m-1}: lh_detect_features on the left image with mask = NULL, exclude_pt = have_kp
 *                (n_exclude = n_have) and this call's exclude_half, max_corners, quality_level and min_distance; m is its
 *                n_corners (at most max_corners), the order is its order.  n_candidates and lambda_max are its outputs.
 *   features     n = n_have + m; kl = have_kp followed by the corners, the order features_left_ has after DetectFeatures.
 *                Feature i < n_have has a point when have_point[i] != 0 (have_point NULL: always); a corner has none.
 *   guess        with a point: lh_track_frame's guess arithmetic on X = have_pts_w[i], T = pose_Tcw, E = cam_pose[1],
 *                K = cam_K[1] (camera_right_->world2pixel, :432).  Without: kl[i] (:436).
 *   track        lh_klt_track(img_left, img_right, kl, the guesses, has_initial = 1) with this call's tracker parameters:
 *                kp_right and success are bitwise its kp2 and success.  n_right counts success (num_good_pts).
 *   triangulate  a feature with success and no point (:116-117): pt and flags are bitwise lh_triangulate's on the two
 *                views ((double)kl[i], (double)kp_right[i]) with cam_pose, cam_K, sing_ratio_thr, the gate and T_out,
 *                as lh_klt_stereo_landmarks returns them.  A failed track without a point carries flag bit 4 alone; a
 *                feature that has a point carries bit 5 (LH_TRI_F_HAS_POINT) alone, tracked or not.  Both have pt = 0.
 *                n_accepted counts flags == 0.
 *
 * The resident image is lh_track_frame's.  img_left == NULL reads it: LH_E_STATE if there is none or its cols / rows
 * differ; the image stays resident and unchanged (the next lh_track_frame with klt.img1 == NULL still finds it), and
 * the pyramid levels this call's max_level needs beyond those already built are built and remembered.  A non-NULL
 * img_left is uploaded and becomes the resident image: StereoInit's call (n_have = 0, T_out = NULL) replaces the priming
 * call.  An argument error or LH_E_STATE leaves the resident image as it was, and so does a failure to
 * allocate the call's own buffers; a call that fails after it began to enqueue, or while it makes room for a given
 * img_left, invalidates it.  n_have == 0 with no corner found is LH_OK with every count 0.
 *
 * The per-feature outputs have room for n_have + max_corners entries; the first n_have + n_new are written.
 *
 * LH_E_BADARG: lh_detect_features' and lh_klt_track's argument errors (cols < 12 or rows < 12, rows * cols > INT32_MAX,
 * step < cols, a negative or NaN quality_level or min_distance, max_level outside 0..3, max_iters < 1, an epsilon that
 * is not > 0, a min_eig_threshold that is not >= 0), max_corners <= 0, n_have < 0, a null img_right, a null have_kp with
 * n_have > 0, a null have_pts_w when some feature can have a point, a null output array, n_have + max_corners > 2^24.
 */
typedef struct lh_keyframe_input {
    int32_t cols, rows;
    int64_t step;               /* bytes per row of img_right, and of img_left when given (>= cols) */
    const uint8_t *img_left;    /* [rows][step] current_frame_->left_img_; NULL: the resident image */
    const uint8_t *img_right;   /* [rows][step] current_frame_->right_img_ */
    int32_t n_have;
    const float *have_kp;       /* [n_have][2] current_frame_->features_left_ positions */
    const double *have_pts_w;   /* [n_have][3] mp->pos_ of each; read only where have_point */
    const uint8_t *have_point;  /* [n_have] nonzero: the feature has a map point; NULL: every one has */
    float exclude_half;         /* the detector's, as lh_detect_input's: 10 */
    int32_t max_corners;        /* > 0: num_features_ (gftt_'s limit, :16), however many features the frame has */
    double quality_level;       /* 0.01 */
    double min_distance;        /* 20 */
    int32_t max_level;          /* the tracker's, as lh_klt_input's: 3 */
    int32_t max_iters;          /* 30 */
    double epsilon;             /* 0.01 */
    double min_eig_threshold;   /* 1e-4 */
    double pose_Tcw[12];        /* current_frame_->Pose() */
    double cam_pose[2][12];     /* camera_left_->pose(), camera_right_->pose() */
    double cam_K[2][4];         /* fx, fy, cx, cy of the two cameras */
    double sing_ratio_thr;      /* the triangulation's, as lh_stereo_input's */
    int32_t gate;
    double y_max, z_min, z_max;
    const double *T_out;        /* [12] or NULL */
} lh_keyframe_input;
typedef struct lh_keyframe_result {
    float *kp_new;              /* [max_corners][2] the detected corners (required) */
    float *kp_right;            /* [n_have + max_corners][2] (required, as the three below) */
    uint8_t *success;           /* [n_have + max_corners] */
    double *pt;                 /* [n_have + max_corners][3] */
    uint8_t *flags;             /* [n_have + max_corners] */
    int32_t n_new;              /* m */
    int32_t n_candidates;
    double lambda_max;
    int32_t n_right;            /* num_good_pts (:454-461) */
    int32_t n_accepted;         /* cnt_triangulated_pts (:146) */
    double time_ms;             /* HIP-event bracket, first kernel to last: the detector's host checks included, copies excluded */
} lh_keyframe_result;
int lh_insert_keyframe(lh_handle *h, const lh_keyframe_input *in, lh_keyframe_result *out);

/* ---- marginal covariances of a solved window (g2o's computeMarginals, Ceres' Covariance) ----
 *
 * lh_covariance works on the state the last lh_solve / lh_solve_resident on the handle returned (lh_result's poses and
 * landmarks), with the handle's weights and gate: Huber(huber_delta), gate_mode, precision; the information of an
 * observation is the identity in pixels, as the reference sets it.  With H the Gauss-Newton Hessian at that state
 * (H_pp, H_pl, H_ll as the solver forms them; no lambda) and S = H_pp - H_pl H_ll^-1 H_lp:
 *
 *   held poses   the window's fixed poses, and pose `anchor` when anchor >= 0; f: the six rows of every other pose;
 *   Sigma_pp     [f, f] = (S[f, f])^-1; every row and column of a held pose is +0.0.  The covariance of the left
 *                perturbation d in T_cw <- exp(d) T_cw, translation part first (VertexPose::add's convention);
 *   Sigma_l      = H_ll^-1 + H_ll^-1 (sum over the landmark's edges e, e' of H_lp,e Sigma_pp[p(e), p(e')] H_pl,e') H_ll^-1,
 *                H_lp,e = J_l,e^T W_e J_p,e: symmetric 3x3, in window landmark order.  A landmark no edge observes is
 *                no vertex: nine NaNs.  So is, under degenerate_guard = 1, a rank-deficient landmark (held fixed by
 *                the solver, it adds nothing to S).
 *
 * Deleting the anchor's rows and columns conditions on that pose.  A window without a fixed pose has a gauge freedom:
 * its S is numerically singular, and anchor (the oldest keyframe, say) is there for it.
 * The outputs are exactly symmetric, two calls return the same bits, and the call changes nothing a later solve
 * returns (it reads the solver's state and writes buffers of its own).
 *
 * LH_E_STATE: no completed solve of the uploaded window on the handle.  LH_E_BADARG: a null in or out, anchor outside
 * [-1, n_poses).  LH_E_UNSUPPORTED: n_poses > 64 (the inverse of a banded S is dense), world_size > 1.
 * LH_E_SINGULAR: no free pose (bad_row 0); a pivot of the Cholesky factor of S[f, f] that is not > 0 (bad_row: its row
 * of the 6 n_poses), which is what a free gauge gives; degenerate_guard = 0 on a window with rank-deficient landmarks.
 * On LH_E_SINGULAR no output array is written. */
typedef struct lh_cov_input {
    int32_t anchor;        /* pose held in addition to pose_fixed; -1: none */
} lh_cov_input;
typedef struct lh_cov_result {
    double *pose_cov;      /* [n_poses][36] diagonal blocks Sigma_pp[p, p], row-major, or NULL               */
    double *pose_cov_full; /* [6 n_poses][6 n_poses] row-major, or NULL                                        */
    double *lm_cov;        /* [n_landmarks][9] window order, or NULL (then no landmark kernel runs)            */
    int32_t n_free;        /* rows factored (6 x free poses)                                                   */
    int32_t bad_row;       /* first row whose pivot was not > 0 (LH_E_SINGULAR), else -1                       */
    double min_pivot, max_pivot;  /* of the factor's L_ii^2: a cheap conditioning signal                       */
    double time_ms;        /* device time (HIP events), linearisation included, the download excluded          */
} lh_cov_result;
int lh_covariance(lh_handle *h, const lh_cov_input *in, lh_cov_result *out);

/* ---- a keyframe of a solved window marginalised into a prior on the poses that stay ----
 *
 * lh_marginalize works on the state the last lh_solve / lh_solve_resident on the handle returned, with the handle's
 * weights and gate (Huber(huber_delta), gate_mode, precision) and identity information in pixels, as lh_covariance
 * does.  With m = marg_pose:
 *
 *   M            the landmarks with a valid edge to pose m, whether or not m is fixed;
 *   the system   of the edges of M's landmarks alone, to every pose they reach:
 *                A_M = H_pp - H_pl H_ll^-1 H_lp, b_M = b_p - H_pl H_ll^-1 b_l, exactly what the solver's linearisation
 *                forms for a window holding just those edges: no lambda, a fixed pose's rows and columns zero, the
 *                solver's sign of b (the step solves A dx = b);
 *   the earlier prior   prior_H / prior_b, when given, are added to A_M and b_M with the rows and columns of the
 *                fixed poses zeroed first.  They are used as given: the caller has expressed them at this state.
 *                Only prior_H's lower triangle (row >= col) is read;
 *   the elimination   with r the rows of the other poses, H_prior = A[r, r] - A[r, m] A[m, m]^-1 A[m, r] and
 *                b_prior = b[r] - A[r, m] A[m, m]^-1 b[m], by an unpivoted Cholesky A[m, m] = C C^T,
 *                Y = C^-1 A[m, r], y = C^-1 b[m], H = A[r, r] - Y^T Y, g = b[r] - Y^T y.  No eigenvalue is thresholded:
 *                a pivot that is not > 0 gives LH_E_SINGULAR with bad_row, and no output array is written;
 *   a fixed m    nothing is eliminated: conditioning on it gives H_prior = A[r, r], b_prior = b[r]
 *                (min_pivot = max_pivot = 0);
 *   the layout   H_prior [6P][6P] and b_prior [6P] cover all P window poses in window order, so that the caller only
 *                drops m's six rows and columns when the window slides, and the prior adds to the next window's system
 *                as Hessian.topLeftCorner += H_prior, b.head += b_prior.  The rows and columns of m and of every fixed
 *                pose are exact +0.0, and so are, without an earlier prior, those of every pose that shares no
 *                landmark with m (an earlier prior's entries there pass through unchanged);
 *   rank-deficient landmarks of M (fewer than two valid edges, or an H_ll that is not positive definite) are treated
 *                as the solver treats them under degenerate_guard = 1: held fixed.  Their Schur terms
 *                H_pl H_ll^-1 H_lp and H_pl H_ll^-1 b_l are dropped; their edges' H_pp and b_p stay.  They are counted
 *                in n_degenerate.  On a handle with degenerate_guard = 0 and n_degenerate > 0 the call answers
 *                LH_E_SINGULAR (bad_row 0), as lh_covariance does.
 *
 * H_prior equals its transpose by bits, two calls return the same bits, and the call changes nothing that a later
 * solve, lh_covariance or lh_debug_reduced_system returns (it reads the solver's state and writes buffers of its own).
 * A solve does not consume a prior yet: adding H_prior and b_prior to the system inside the LM loop is not part of
 * this interface.
 *
 * LH_E_STATE: no completed solve of the uploaded window on the handle.  LH_E_BADARG: a null h, in, out, H_prior or
 * b_prior, marg_pose outside [0, n_poses), one of prior_H / prior_b without the other.  LH_E_UNSUPPORTED: n_poses > 64,
 * world_size > 1 (lh_covariance's envelope).  LH_E_SINGULAR: above; the counts and pivots are still reported. */
typedef struct lh_marg_input {
    int32_t marg_pose;            /* the pose to marginalise, 0 <= m < n_poses */
    const double *prior_H;        /* [6P][6P] row-major or NULL: an earlier prior, added before the elimination; only the lower triangle (row >= col) is read */
    const double *prior_b;        /* [6P] or NULL (both given or both NULL) */
} lh_marg_input;
typedef struct lh_marg_result {
    double *H_prior;              /* [6P][6P] row-major (required) */
    double *b_prior;              /* [6P] (required) */
    uint8_t *lm_marginalised;     /* [n_landmarks] window order, or NULL: 1 = eliminated with the pose (the caller drops it from the map) */
    int32_t n_landmarks, n_edges; /* landmarks eliminated; valid edges of those landmarks (all of them, to any pose) */
    int32_t n_degenerate;         /* rank-deficient landmarks among them */
    int32_t bad_row;              /* first row (0..5) of the eliminated block whose pivot was not > 0, else -1 */
    double min_pivot, max_pivot;  /* L_ii^2 of the 6x6 factor */
    double time_ms;               /* HIP-event bracket, linearisation included, download excluded */
} lh_marg_result;
int lh_marginalize(lh_handle *h, const lh_marg_input *in, lh_marg_result *out);

/* ---- test hooks (not part of the reference interface) ---- */
/* f64 MFMA accumulator-layout probe: D(16x16) = A(16x4) * B(4x16), device pointers, row-major */
int lh_debug_mfma_probe(const double *A, const double *B, double *D);
/* k_ctrl's reduced-system solve (natural order, blocked LDL^T over a dense envelope, back
   substitution) on a dense symmetric n x n S (row-major), n <= 384: x = S^-1 b.  Device pointers.
   n > 128 runs k_ctrl_g's global-memory solve (Eigen-LDLT pivot order: dense windows of 22..64
   keyframes). */
int lh_debug_ldlt_probe(const double* S, const double* b, int n, double* x);
/* k_ctrl's PCG solve (same LDS layout and pivot order) on a dense symmetric n x n S, n <= 128:
   x ~= S^-1 b to ||r|| <= tol ||b|| within max_iters (<= 0: 2n).  Device pointers; *iters host. */
int lh_debug_pcg_probe(const double* S, const double* b, int n, double tol, int max_iters, double* x, int* iters);
/* mean HIP-event bracket (ms) of an empty kernel on the handle's stream: the launch floor of the
   per-kernel times lh_set_profiling reports (bench.py subtracts it for the roofline) */
int lh_debug_event_floor(lh_handle *h, double *ms);
/* per-phase wave-cycle totals of a -DLH_STAMPS diagnostic build (all zero in the product build) */
int lh_debug_stamps(unsigned long long *out, int n, int reset);
/* k_lin's waves in a -DLH_STAMPS diagnostic build (all zero in the product build): 8 words per (workgroup, wave) of
   the last full trial launch, workgroup-major: [0] HW_ID | XCC_ID << 32 | 1 << 40, [1] the clock at the wave's entry
   to its sub-batch loop, [2 + r] at the end of its r-th sub-batch.  Up to 16384 words; cleared by the read. */
int lh_debug_lin_stamps(unsigned long long *out, int n);
/* k_lin's duration per LM trial, measured after a solve: the trial-mode k_lin launch(es) replayed
   reps times back to back between two HIP events on the handle's stream (ms per replay).  The
   replay rewrites the candidate buffers and the per-edge chi2: read the solve's outputs first. */
int lh_debug_time_lin(lh_handle *h, int reps, double *ms);
/* reduced-system all-reduces (data-path collectives) the last solve issued on this rank */
int lh_debug_comm_count(lh_handle *h, int64_t *n);
/* the controller the uploaded window's trials run: 0 k_ctrl (LDS, <= 21 poses), 1 k_ctrl_g (dense
   LDL^T in global memory), 2 k_ctrl_p (PCG on the block-sparse system), 3 k_ctrl_b (banded LDL^T);
   bit 8: k_ctrl_b's back substitution holds one row per lane (every row's envelope within 56 rows);
   bit 9: some k_ctrl_b step needs more than 11 unit waves, so its stream loaders take units too */
int lh_debug_controller(lh_handle *h, int *which);
/* k_lin's shape on the uploaded window: waves per workgroup (4, or 8: one workgroup per compute unit, the planner's
   choice for a window that fills the GPU; LH_NO_LIN_WG8=1 keeps 4), the window's chunks, and the landmarks-per-chunk
   bound they were cut with */
int lh_debug_lin_shape(lh_handle *h, int *waves, int *chunks, int *chunk_landmarks);
/* the LM chains (k_lin, k_reduce, exchange, controller) the last solve decided past the initial
   linearisation: its trials, plus one re-linearisation per evaluate-only trial accepted outside the
   final iteration (a trial after a rejection only evaluates).  Solves that return arrays only. */
int lh_debug_chains(lh_handle *h, int *chains);
/* the lambda ladder: the rungs a factoring controller of the uploaded window builds (1: off),
   and the rejections of the last solve whose step a rung had already solved, so that no controller factored
   for them.  Solves that return arrays only (else skipped = -1). */
int lh_debug_ladder(lh_handle *h, int *rungs, int *skipped);

/* batched evaluation of rejection runs: the most rungs one chain of the uploaded window evaluates
   (1: off -- LH_NO_BATCH=1, or a ladder of one rung), the batches the last solve decided, and (retrials, two ints,
   may be NULL) the acceptances among them: [0] re-run by the next chain as a full trial, [1] re-run and stopping
   the loop.  Solves that return arrays only (else -1). */
int lh_debug_batch(lh_handle *h, int *batch_max, int *batches, int *retrials);
/* the reduced pose system as the last chain left it, copied to out[cap] behind the handle's stream.  which: 0 the
   staged packed system (k_reduce's output: npairs 6x6 blocks of S, b_s, b_p, diag H_pp, the chunk scalars), 1 the
   committed one, 2 the pending pose step (6 n_poses doubles), 3 the staged half of k_reduce's image of S where the
   controller reads S from one (k_ctrl's LDS layout, k_ctrl_b's band; *n_out 0 otherwise).  *n_out: the doubles the
   buffer holds; *npairs_out: the blocks of S.  LH_E_BADARG without an uploaded window or with cap < *n_out. */
int lh_debug_reduced_system(lh_handle *h, int which, double *out, int64_t cap, int64_t *n_out, int32_t *npairs_out);
/* every step of the lambda ladder the last factoring controller of the last solve built, copied behind
   the handle's stream; nothing on the device is written, so every later solve returns what it would have.  *lad_n_out:
   the rungs built (1: the step alone; 0: no controller factored, max_iters = 0); dxp_out[cap]: the lad_n pose steps,
   rung-major (rung r at r 6 n_poses), *n_out = lad_n 6 n_poses; *lad_out: the rung of the pending step (row lad of
   dxp_out is lh_debug_reduced_system's which = 2); spose_out[r], its_out[r], r < lad_n (room for 16 each): the pose
   half of rung r's gain denominator and the PCG iterations of its solve (0 under LDL^T).  LH_E_BADARG without an
   uploaded window or with cap < *n_out: *n_out and *lad_n_out are reported and nothing else is written. */
int lh_debug_ladder_steps(lh_handle *h, double *dxp_out, int64_t cap, int64_t *n_out, int32_t *lad_n_out,
                          int32_t *lad_out, double *spose_out, int32_t *its_out);

#ifdef __cplusplus
}
#endif
#endif
