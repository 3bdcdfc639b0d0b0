/*
 * plba.h — C ABI of the MI355X local-bundle-adjustment backend.
 *
 * Drop-in boundary for the g2o solve inside
 *   void PLSLAM::MapHandler::localBundleAdjustmentForPlukerWithG2O()
 *   (reference: include/mapHandler.h:134, src/mapHandler.cpp:5851-6323)
 *
 * The reference builds a g2o::SparseOptimizer on the stack (src/mapHandler.cpp:5923-5929),
 * adds VertexLMPose / VertexLMPointXYZ / VertexLMLineOrth vertices and EdgePosePoint /
 * EdgePoseLine edges (g2o_types/g2o_types.h:28-502), then runs
 *   initializeOptimization(); optimize(5);  ... classify ...;
 *   initializeOptimization(0); optimize(10);                     (src/mapHandler.cpp:6119-6152)
 * Each entry point below replaces one of those g2o calls:
 *
 *   plba_create / plba_destroy        ~ g2o::SparseOptimizer ctor + setAlgorithm(Levenberg(BlockSolverX(
 *                                       LinearSolverEigen)))  / dtor          (src/mapHandler.cpp:5923-5929)
 *   plba_upload                       ~ addVertex / addEdge / setRobustKernel / SetParams loop
 *                                                                              (src/mapHandler.cpp:5931-6117)
 *   plba_set_edge_levels              ~ Edge::setLevel                        (src/mapHandler.cpp:6130,6143)
 *   plba_set_robust                   ~ Edge::setRobustKernel(0 | Huber)      (src/mapHandler.cpp:6133,6146)
 *   plba_initialize_optimization      ~ SparseOptimizer::initializeOptimization(int level)
 *                                                                              (src/mapHandler.cpp:6121,6151)
 *   plba_optimize                     ~ SparseOptimizer::optimize(int iterations)
 *                                                                              (src/mapHandler.cpp:6122,6152)
 *   plba_refresh_edge_errors          ~ Edge::computeError() on level-1 edges (src/mapHandler.cpp:6158-6160,6226-6228)
 *   plba_get_edge_chi2                ~ Edge::chi2() / EdgePosePoint::isDepthPositive()
 *                                                                              (src/mapHandler.cpp:6129,6142,6161,6230)
 *   plba_download                     ~ Vertex::estimate()                    (src/mapHandler.cpp:6297-6319)
 *   plba_lba_plucker                  the whole two-stage schedule of src/mapHandler.cpp:6119-6160 on device,
 *                                     with no host round trip between the stages.
 *
 * Conventions: all arrays are host pointers owned by the caller and copied by the call;
 * FP64 everywhere; indices are int32; every function returns PLBA_OK (0) or a negative
 * PLBA_E* status and never throws or exits (the reference exit(0)s on index errors,
 * src/mapHandler.cpp:5894,5910,5998,6062). A context is single-threaded (one LBA at a time,
 * as handlerThread guarantees, src/mapHandler.cpp:1186-1188).
 */
#ifndef PLBA_H
#define PLBA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLBA_OK              0
#define PLBA_E_INVALID     (-1)   /* bad argument / index out of range                 */
#define PLBA_E_DEVICE      (-2)   /* HIP runtime error                                 */
#define PLBA_E_STATE       (-3)   /* call out of order (e.g. optimize before upload)   */
#define PLBA_E_NOMEM       (-4)
#define PLBA_E_COMM        (-5)   /* RCCL error (sharded windows)                      */

/* One LBA window in g2o vertex/edge form (structure-of-arrays).
 * Vertex ids follow src/mapHandler.cpp:5941 (pose id = kf_idx), :5983 (point id =
 * idx+max_kf_id+1), :6047 (line id = idx+maxPointId+1). Ids order the Hessian exactly as
 * g2o's buildIndexMapping does (free poses by id, then landmarks by id). Edge arrays are in
 * g2o insertion order (all point edges, then all line edges). */
typedef struct plba_graph {
    int32_t n_kf, n_pt, n_ln, n_ept, n_eln;
    double fx, fy, cx, cy;            /* EdgePosePoint/EdgePoseLine::SetParams (g2o_types.h:217,313) */
    const double  *kf_Tcw;            /* [n_kf][12]  row-major 3x4 [R | t] of Tcw = T_kf_w^-1     */
    const uint8_t *kf_fixed;          /* [n_kf]      VertexLMPose::setFixed                        */
    const int32_t *kf_id;             /* [n_kf]      vertex id                                     */
    const double  *pt_xyz;            /* [n_pt][3]   VertexLMPointXYZ estimate                     */
    const int32_t *pt_id;             /* [n_pt]                                                    */
    const double  *ln_orth;           /* [n_ln][4]   VertexLMLineOrth estimate (θ1,θ2,θ3,φ)        */
    const int32_t *ln_id;             /* [n_ln]                                                    */
    const int32_t *ept_lm, *ept_kf;   /* [n_ept]     vertex 0 (point index) / vertex 1 (kf index)  */
    const double  *ept_obs;           /* [n_ept][2]  pixel measurement                             */
    const double  *ept_info;          /* [n_ept]     Ω = info·I2 (info already float-rounded)      */
    const int32_t *eln_lm, *eln_kf;   /* [n_eln]                                                   */
    const double  *eln_obs;           /* [n_eln][4]  (spl.x, spl.y, epl.x, epl.y)                  */
    const double  *eln_info;          /* [n_eln]     Ω = info·I4                                   */
    double huber_pt, huber_ln;        /* RobustKernelHuber::setDelta ((float)sqrt(5.991))          */
} plba_graph;

/* Per outer-LM-iteration trace (OptimizationAlgorithmLevenberg::solve). */
typedef struct plba_iter_trace {
    int32_t stage;        /* 0 or 1 (optimize(5) / optimize(10))                    */
    int32_t iter;         /* iteration index inside optimize()                      */
    int32_t trials;       /* damped trials run (1..10)                              */
    int32_t result;       /* 0 OK, 1 Terminate, 2 Fail                              */
    double  chi2_start;   /* activeRobustChi2 at linearisation                     */
    double  chi2_end;     /* currentChi after the trial loop                        */
    double  lambda_start; /* λ used by the first trial                              */
    double  lambda_end;   /* λ after the trial loop                                 */
} plba_iter_trace;

/* Output of plba_lba_plucker (all optional; NULL = not wanted). */
typedef struct plba_result {
    double  *kf_Tcw;        /* [n_kf][12] final Tcw (fixed poses unchanged)                   */
    double  *pt_xyz;        /* [n_pt][3]                                                       */
    double  *ln_orth;       /* [n_ln][4]                                                       */
    double  *ept_chi2;      /* [n_ept] chi2 as the post-solve outlier pass sees it (A13 rules) */
    uint8_t *ept_depth_ok;  /* [n_ept] isDepthPositive() at the final state                    */
    uint8_t *ept_level;     /* [n_ept] level after the stage-1 classification                  */
    double  *eln_chi2;      /* [n_eln]                                                         */
    uint8_t *eln_level;     /* [n_eln]                                                         */
    int32_t  iters[2];      /* outer iterations executed by optimize(5) and optimize(10)      */
    double   chi2[2];       /* final activeRobustChi2 of each stage                            */
    double   solve_ms;      /* wall time inside the two optimize() calls                       */
} plba_result;

typedef struct plba_opts {
    int32_t device;                  /* HIP device ordinal                                         */
    int32_t corrected_line_jacobian; /* 0 = reproduce g2o_types.h:429-430 (orth used as Plücker)   */
    int32_t verbose;                 /* print a per-iteration log to stderr                        */
    int32_t max_trials;              /* g2o maxTrialsAfterFailure (10)                             */
    double  tau;                     /* g2o Levenberg τ (1e-5)                                     */
} plba_opts;

typedef struct plba_ctx plba_ctx;

void        plba_default_opts(plba_opts *o);
int         plba_create(plba_ctx **ctx, const plba_opts *opts);
int         plba_destroy(plba_ctx *ctx);
const char *plba_last_error(const plba_ctx *ctx);

int plba_upload(plba_ctx *ctx, const plba_graph *g);
int plba_reset_estimates(plba_ctx *ctx);                       /* back to the uploaded estimates */
int plba_set_edge_levels(plba_ctx *ctx, const uint8_t *ept_level, const uint8_t *eln_level);
int plba_set_robust(plba_ctx *ctx, int32_t robust);            /* 1 = Huber on every edge, 0 = none */
int plba_initialize_optimization(plba_ctx *ctx, int32_t level);
int plba_optimize(plba_ctx *ctx, int32_t iterations, int32_t *iters_done, double *final_chi2);
int plba_refresh_edge_errors(plba_ctx *ctx, int32_t level);    /* computeError() on edges of `level` */
int plba_get_edge_chi2(plba_ctx *ctx, double *ept_chi2, uint8_t *ept_depth_ok, double *eln_chi2);
int plba_download(plba_ctx *ctx, double *kf_Tcw, double *pt_xyz, double *ln_orth);
int plba_lba_plucker(plba_ctx *ctx, plba_result *res);         /* full two-stage schedule          */
int plba_get_trace(plba_ctx *ctx, plba_iter_trace *out, int32_t cap, int32_t *n);
int plba_synchronize(plba_ctx *ctx);

/* Per-kernel timing of the last plba_lba_plucker call (HIP events on the solver stream).
 * names[i] points to a static string; ms[i] is the summed time of that kernel. */
int plba_enable_kernel_timing(plba_ctx *ctx, int32_t on);   /* HIP-event timing of each launch */
/* Structure of the uploaded window: out[0]=free poses, [1]=envelope bandwidth (pose blocks),
 * [2]=reduced-camera blocks, [3]=Schur triples, [4]=edges, [5]=landmarks, [6]=banded (1/0),
 * [7]=assembly chunks, [8]=edges with a free pose, [9]=point edges, [10]=step hipGraph in use,
 * [11]=sharded code path, [12]=two-sided (twisted) band factorisation, [13]=column-lane
 * band factorisation (bandwidth <= 9), [14]=super-rows of the block-cyclic-reduction
 * factorisation (0 = not used), [15]=dense RCS on the multi-workgroup MFMA path,
 * [16]=times a block-cyclic-reduction hand-off timed out and the schedule was re-solved with
 * the column-lane factorisation (the context then keeps that factorisation), [17]=trial slots
 * a step evaluates at most (speculative damped trials, 1 = off), [18]=their policy
 * (0 off, 1 always, 2 after a rejection in the iteration, 3 after the first rejection of the
 * optimize() call), [19]=device steps the last schedule took, [20]=block cyclic reduction runs its back
 * substitution inside the forward launch (1; 0 with PLBA_BCR_SPLIT=1 or without BCR), [21]=window structure built on the
 * device (1) or on the host (0).
 * Counts are this rank's when the window is sharded. */
int plba_structure_stats(plba_ctx *ctx, int64_t *out, int32_t cap);
int plba_kernel_times(plba_ctx *ctx, const char **names, double *ms, int32_t *launches,
                      int32_t cap, int32_t *n);
/* The factorisation plba_upload would choose, under the current environment switches, for a
 * window of nf free poses whose envelope is bw pose blocks wide, on a device that holds
 * `resident` block-cyclic-reduction workgroups at once. Needs no context and touches no device.
 * flags: 1 = block cyclic reduction ruled out (the context fell back before), 2 = sharded window,
 * 4 = the window has Schur triples (trial slots are possible).
 * out[0]=mode (0 dense scalar, 1 dense MFMA, 2 band, 3 band two-sided, 4 column-lane,
 * 5 column-lane two-sided, 6 block cyclic reduction), [1]=BCR super-rows, [2]=BCR back
 * substitution fused, [3]=two-sided split row, [4]=band kernels' ring slots, [5]=trial slots,
 * [6]=their policy, [7]=mode a BCR window falls back to after a hand-off timeout (-1: none),
 * [8]=its split row. Entries past cap are not written. */
int plba_factor_plan(int32_t bw, int32_t nf, int32_t resident, int32_t flags, int32_t *out, int32_t cap);

/* ---- Hand-rolled Levenberg–Marquardt local BA:
 *   int MapHandler::levMarquardtOptimizationLBAForPluker(X_aux, kf_list, pt_list, ls_list,
 *                                                         pt_obs_list, ls_obs_list)
 *   (src/mapHandler.cpp:1618-2332; window lists built by localBundleAdjustmentForPluker, :1505-1615)
 * One scalar residual r = ‖e‖ per observation with a Cauchy weight w = 1/(1+r²)
 * (src2/auxiliar.cpp:556-559), H += w·JᵀJ, g += w·J·r, Marquardt damping H(i,i) += λ·H(i,i),
 * DX = H⁻¹g, poses X_i ← log(exp(X_i)·exp(DX_i)⁻¹), points X += DX, lines updateOrthCoord.
 * The window is the plba_graph of plba_upload, read as the reference's lists:
 *   kf_fixed[k] == 0  <=>  KF k is in kf_list (local && kf_idx != 0, :1516)
 *   kf_Tcw  = inverse_se3(T_kf_w), the MAP pose (:1657-1659): fixed KFs and every line
 *             observation use it on every iteration (:2010-2012), free KFs on the first one
 *   pt_xyz  = point3D (:1536), ln_orth = orthNDw = changePlukerToOrth(NDw) (:1577)
 *   edges   = pt_obs_list / ls_obs_list (obs_list[i] / NDw_obs_list[i]); the info, Huber and
 *             level fields are not used by this solver. */
typedef struct plba_hlm_state {
    const double *kf_x;        /* [n_kf][6] KeyFrame::x_kf_w = X_aux pose blocks [t; ω] (:1518)   */
    const double *ln_pluker;   /* [n_ln][6] MapLine::NDw of the map (first linearisation, :1744)  */
    const double *ln_line3d;   /* GBA / LBA_ENDPOINTS: [n_ln][6] MapLine::line3D endpoints [P; Q]
                                  (:3089, :1464)                                                  */
} plba_hlm_state;

typedef struct plba_hlm_params {
    double  lambda0;           /* SlamConfig::lambdaLbaLM()  1e-5 (src/slamConfig.cpp:65)         */
    double  lambda_k;          /* SlamConfig::lambdaLbaK()   10   (src/slamConfig.cpp:66)         */
    double  homog_th;          /* Config::homogTh()          1e-7 (src2/config.cpp:80)            */
    double  min_error;         /* Config::minError()         1e-7 (src2/config.cpp:84)            */
    double  min_error_change;  /* Config::minErrorChange()   1e-7 (src2/config.cpp:85)            */
    int32_t max_iters;         /* SlamConfig::maxItersLba()  15   (src/slamConfig.cpp:67)         */
    int32_t err_per_obs;       /* 0 = the reference: err /= (Npt_obs + Nls_obs), both counters stay
                                  0 (:1642,1731,1849) so err becomes +inf and every step after the
                                  first is accepted; 1 = divide by the observation count instead */
    int32_t variant;           /* PLBA_HLM_LBA_PLUCKER, PLBA_HLM_GBA or PLBA_HLM_LBA_ENDPOINTS    */
    int32_t pad;
} plba_hlm_params;

/* plba_hlm_params.variant
 * PLBA_HLM_GBA = MapHandler::levMarquardtOptimizationGBA (src/mapHandler.cpp:3128-3726, window of
 * globalBundleAdjustment :3022-3126): every KF but kf_idx 0 free; lines are 6-dim landmarks, the
 * endpoints line3D = [P; Q] (state_ln_line3d), observed as image line equations (a, b, c) in
 * eln_obs[.][0..2]; residual e = (l·π(P), l·π(Q)); from the second linearisation on both
 * endpoints are read from X at the aliased offset 6Nkf+3Npt+3·j (:3547-3548); Hmax is an int
 * (:3386, truncation); the stop tests use numeric_limits<double>::epsilon() (pass it as
 * min_error / min_error_change).
 * PLBA_HLM_LBA_ENDPOINTS = MapHandler::levMarquardtOptimizationLBA (src/mapHandler.cpp:2334-3016,
 * window of localBundleAdjustment :1392-1502), the local BA of a build without USE_LINE_PLUKER:
 * a KF is free iff local && kf_idx != 0 (:1403, kf_fixed[k] == 0), every other observing KF is
 * fixed and its observations add to the landmark block and g only (:2417-2423, :2530-2536); lines
 * and observations as in GBA (state_ln_line3d, eln_obs[.][0..2] = (a, b, c)), with the same aliased
 * reads of both endpoints from the second linearisation on (:2697-2698) and the map pose T_kf_w for
 * every line observation (:2700); Hmax is a double (:2555); err is divided by Npt_obs + Nls_obs == 0
 * on the first linearisation (:2551, +inf) and by the landmark counts Npt + Nls afterwards (:2796,
 * finite; err_per_obs = 1 divides both by the observation count); the later line linearisations
 * hard-code the homogeneous threshold 1e-7 (:2717-2760) where the first one and the points read
 * homog_th; the stop tests use min_error_change / min_error (:2798, :2834). Unsharded windows only,
 * as GBA. ln_pluker is not read. */
#define PLBA_HLM_LBA_PLUCKER   0
#define PLBA_HLM_GBA           1
#define PLBA_HLM_LBA_ENDPOINTS 2

typedef struct plba_hlm_result {
    double  *kf_x;             /* [n_kf][6] X pose blocks at exit (KFs not in kf_list: input x)   */
    double  *kf_Tcw;           /* [n_kf][12] inverse_se3(expmap_se3(x)) of each free KF, map pose
                                  of the others                                                   */
    double  *pt_xyz;           /* [n_pt][3]                                                       */
    double  *ln_orth;          /* [n_ln][4]                                                       */
    int32_t  linearizations;   /* H/g builds executed (1 .. max_iters)                            */
    int32_t  solves;           /* SimplicialLDLT solves executed                                  */
    int32_t  accepted;         /* solves whose DX was applied                                     */
    int32_t  pad;
    double   err;              /* last err (after the division)                                   */
    double   lambda;           /* λ at exit                                                       */
    double   dx_norm;          /* ‖DX‖ of the last solve                                          */
    double   solve_ms;         /* wall time of the loop                                           */
    double  *ln_line3d;        /* GBA / LBA_ENDPOINTS: [n_ln][6] line3D at exit                   */
} plba_hlm_result;

void plba_hlm_default_params(plba_hlm_params *p);
/* The whole loop on the uploaded window, on the device (one captured step per iteration).
 * Per-iteration records (plba_get_trace): stage 0, iter, trials 1, result 0 = DX applied,
 * 1 = DX rejected (err > err_prev), 3 = stopped before the solve; chi2_start = chi2_end = err,
 * lambda_start / lambda_end around the iteration.
 * Deliberate divergence (INTEGRATION.md B'): a free keyframe with no active observation gets 1.0
 * on its diagonal (DX = 0) and a zero pivot elsewhere keeps X unchanged, where the reference's
 * Eigen SimplicialLDLT would solve on a partial factor and produce inf / NaN. */
int plba_hlm_lba(plba_ctx *ctx, const plba_hlm_state *st, const plba_hlm_params *p, plba_hlm_result *res);

/* ---- Loop-closure pose graph:
 *   bool MapHandler::loopClosureOptimizationEssGraphG2O()  (src/mapHandler.cpp:5070-5299)
 *   bool MapHandler::loopClosureOptimizationCovGraphG2O()  (src/mapHandler.cpp:5301-5531)
 * g2o::SparseOptimizer with g2o::VertexSE3 vertices and g2o::EdgeSE3 edges,
 * OptimizationAlgorithmLevenberg over BlockSolver_6_3 + LinearSolverCholmod,
 * setUserLambdaInit(1e-10) (:5085), then initializeOptimization(); computeInitialGuess();
 * computeActiveErrors(); optimize(maxItersPGO) (:5182-5185).
 *   VertexSE3::oplusImpl:  X <- X · fromVectorMQT(δ),  δ = [Δt; qx qy qz]
 *   EdgeSE3::computeError: e = toVectorMQT(Z⁻¹ · X_from⁻¹ · X_to), χ² = eᵀΩe
 * Poses are Isometry3 (row-major 3x4 [R | t]). The reference replaces Cholmod's supernodal
 * Cholesky here by a dense LDLᵀ on the device: same solution; the solve fails when a pivot is
 * not positive (CHOLMOD_NOT_POSDEF), which g2o treats as a rejected trial. */
typedef struct plba_pgo_graph {
    int32_t        n_v;     /* vertices                                                         */
    int32_t        n_e;     /* edges                                                            */
    const int32_t *v_id;    /* [n_v] g2o vertex ids (the reference: KF indices), unique         */
    const double  *v_T;     /* [n_v][12] VertexSE3 estimates                                    */
    const uint8_t *v_fixed; /* [n_v] setFixed                                                   */
    const int32_t *e_v;     /* [n_e][2] vertex positions (0..n_v-1) of vertex(0), vertex(1)     */
    const double  *e_Z;     /* [n_e][12] setMeasurement                                         */
    const double  *e_info;  /* [n_e][36] information, row-major; NULL = identity (the reference) */
} plba_pgo_graph;

typedef struct plba_pgo_params {
    double  user_lambda_init; /* setUserLambdaInit: 1e-10 (:5085); <= 0: τ·max|H_ii|, τ = 1e-5
                                 always (g2o's default; plba_opts::tau is the window solver's)   */
    int32_t max_iters;        /* optimize(SlamConfig::maxItersPGO()) — 100 (src/slamConfig.cpp:79) */
    int32_t initial_guess;    /* 1: computeInitialGuess() (the reference calls it)              */
    int32_t max_trials;       /* OptimizationAlgorithmLevenberg maxTrialsAfterFailure: 10        */
    int32_t pad;
} plba_pgo_params;

typedef struct plba_pgo_result {
    double          *v_T;        /* [n_v][12] final estimates (NULL = not wanted)                */
    plba_iter_trace *trace;      /* [trace_cap] per-iteration records (stage 0), may be NULL     */
    int32_t          trace_cap;
    int32_t          n_trace;
    int32_t          iterations; /* outer iterations run by optimize()                          */
    int32_t          trials;     /* damped trials run                                           */
    int32_t          solve_fails;/* trials whose factorisation met a non-positive pivot         */
    int32_t          n_free;     /* vertices in the Hessian (active, not fixed)                 */
    double           chi2_initial; /* activeChi2 after computeInitialGuess                      */
    double           chi2_final;
    double           lambda_final;
    double           solve_ms;   /* wall time of optimize()                                     */
} plba_pgo_result;

void plba_pgo_default_params(plba_pgo_params *p);
/* computeInitialGuess (host: g2o's EstimatePropagator, Dijkstra from the fixed vertices over the
 * active edges, unit edge cost) and optimize() on the device (per-edge linearisation, dense
 * assembly, multi-workgroup LDLᵀ with MFMA trailing updates, one host decision per trial). */
int plba_pgo_optimize(plba_ctx *ctx, const plba_pgo_graph *g, const plba_pgo_params *p, plba_pgo_result *res);

/* ---- Loop-closure relative pose, the verification step between place recognition and the pose graph:
 *   bool MapHandler::computeRelativePoseRobustGN(lc_points, lc_lines, lc_pt_idx, lc_ls_idx, pose_inc)
 *                                                           (src/mapHandler.cpp:4677-5068)
 *   bool MapHandler::computeRelativePoseGN(...)             (src/mapHandler.cpp:4413-4675)
 * called by isLoopClosure (:4303-4411) with the descriptor matches of the two keyframes. A robust
 * pose-only Gauss–Newton: the 3-D points P and line endpoints sP, eP of the old keyframe kf0 are
 * moved by T_inc and projected into the new keyframe kf1, against its pixel pl and its normalised
 * image line le. One scalar residual r = ‖e‖ per match with the Cauchy weight w = 1/(1+r²),
 * H += w·JJᵀ, g += w·J·r, e += w·r², e /= active matches; x = H⁻¹g by ColPivHouseholderQR;
 * T_inc ← T_inc·inverse_se3(expmap_se3(x)). At most max_iters_first passes, then every active
 * match with ‖e‖ > sqrt(7.815) becomes an outlier, then (RobustGN) at most max_iters refinement
 * passes on the inliers, err_prev carried over. Stop tests: |e − err_prev| < ε, e < ε (before the
 * solve), ‖x‖ < ε (after the update), ε = numeric_limits<double>::epsilon().
 * The accept test: e < lc_res, the largest eigenvalue of H⁻¹ < lc_unc, inliers / matches > lc_inl
 * (forced true in RobustGN, :5014), ‖x_inc[0:3]‖ < lc_trs, ‖x_inc[3:6]‖·180/π < lc_rot, with
 * x_inc = logmap_se3(T_inc). pose_inc is what loopClosure() pushes onto lc_pose_list (:4080-4081).
 * Kept from the reference: the Jacobian rows use fx for both image directions (:4719); the step of
 * this left-perturbation Jacobian is applied on the right (:4815).
 * Defined where the reference is not: a candidate with no active match (none given, or none left by
 * the outlier pass; the reference divides by zero) has accepted = 0, its T_inc is left as it was
 * and its other numbers are unspecified; a singular H has unc = +inf and accepted = 0 (the
 * reference's H.inverse() is inf / NaN there). Neither disturbs the rest of the batch.
 * A call verifies a batch of candidate pairs in one kernel launch, one workgroup per candidate. */
typedef struct plba_lcpose_batch {      /* K candidate pairs, concatenated */
    int32_t n;                          /* candidates                                        */
    const int32_t *pt_off, *ln_off;     /* [n+1] feature ranges                              */
    const double *pt_P;                 /* [pt_off[n]][3] stereo_pt[i1]->P of kf0 (:4341)    */
    const double *pt_obs;               /* [pt_off[n]][2] stereo_pt[i2]->pl of kf1 (:4342)   */
    const double *ln_sP, *ln_eP;        /* [ln_off[n]][3] (:4367-4368)                       */
    const double *ln_le;                /* [ln_off[n]][3] le of kf1 (:4369)                  */
    double fx, fy, cx, cy;
} plba_lcpose_batch;

/* plba_lcpose_params.variant */
#define PLBA_LCPOSE_ROBUST_GN 0         /* computeRelativePoseRobustGN (what isLoopClosure calls)   */
#define PLBA_LCPOSE_GN        1         /* computeRelativePoseGN: no refinement, lc_inl tested,
                                           pose_inc = logmap(inverse(T_inc)) (:4669)                */

typedef struct plba_lcpose_params {
    double  homog_th;          /* Config::homogTh()      1e-7 (src2/config.cpp:80)                  */
    double  lc_res;            /* SlamConfig::lcRes()    1.0  (src/slamConfig.cpp:73-77)            */
    double  lc_unc;            /* SlamConfig::lcUnc()    0.01                                       */
    double  lc_inl;            /* SlamConfig::lcInl()    0.3                                        */
    double  lc_trs;            /* SlamConfig::lcTrs()    1.5                                        */
    double  lc_rot;            /* SlamConfig::lcRot()    35                                         */
    int32_t max_iters_first;   /* SlamConfig::maxIters()    5 (src2/config.cpp:82-83)               */
    int32_t max_iters;         /* SlamConfig::maxItersRef() 10                                      */
    int32_t variant;           /* PLBA_LCPOSE_ROBUST_GN or PLBA_LCPOSE_GN                           */
    int32_t pad;
} plba_lcpose_params;

typedef struct plba_lcpose_out {
    int32_t accepted;          /* the reference's return value                                      */
    int32_t conditions;        /* bit 0 res, 1 unc, 2 inl, 3 trs, 4 rot                             */
    int32_t iters_first;       /* passes (H / g builds) of the first loop                           */
    int32_t iters_ref;         /* passes of the refinement loop (0 in PLBA_LCPOSE_GN)               */
    int32_t n_inl_pt, n_inl_ln;/* matches still active after the outlier pass                       */
    double  e, unc, t, r_deg;  /* the four tested figures (e: last pass)                            */
    double  x_inc[6];          /* logmap_se3(T_inc), [t; ω]                                         */
    double  pose_inc[6];       /* RobustGN: logmap(inverse(expmap(x_inc))) (:5062)                  */
    double  T_inc[12];         /* row-major 3x4                                                     */
    double  H[36];             /* last pass, row-major                                              */
} plba_lcpose_out;

void plba_lcpose_default_params(plba_lcpose_params *p);
/* Runs on the context's stream; needs no uploaded window and leaves one intact; its device buffers
 * are kept and reused across calls. out: [n]. pt_inlier [pt_off[n]] / ln_inlier [ln_off[n]] receive
 * the inlier flags (each may be NULL). p == NULL: the defaults. PLBA_E_INVALID for a NULL batch /
 * out / array, n < 0, decreasing (or negative) offsets, negative iteration caps or an unknown
 * variant; n == 0 does nothing and returns PLBA_OK. */
int plba_lc_relative_pose(plba_ctx *ctx, const plba_lcpose_batch *b, const plba_lcpose_params *p,
                          plba_lcpose_out *out, uint8_t *pt_inlier, uint8_t *ln_inlier);

/* ---- Frame-to-frame pose, the numerical routine of the per-frame loop:
 *   void StereoFrameHandler::optimizePose()                 (src2/stereoFrameHandler.cpp:307-405)
 * with gaussNewtonOptimizationRobust / optimizeFunctionsRobust (:446-494, :1010-1277; the endpoint
 * line model), gaussNewtonOptimizationforPluker / optimizeFunctionsUsingPluker (:803-853, :564-801;
 * a USE_LINE_PLUKER build), removeOutliers (:1303-1396), isGoodSolution (:292-305), the MAD scales
 * of src2/auxiliar.cpp:387-460 and StereoFrame::lineSegmentOverlap (src2/stereoFrame.cpp:547-653).
 * The matches of the previous frame's features with the current frame (what matchF2FPoints / Lines
 * leave, :131-180) go in; DT, DT_cov, err_norm and the eigenvalues of DT_cov come out.
 *   DT = the previous frame's DT if use_motion_model and isGoodSolution(prev) else I (:317-326);
 *   fewer than min_features matches: DT = I (:377-381);
 *   else a first loop of at most max_iters passes on a copy DT_; if isGoodSolution(DT_, cov, err):
 *   removeOutliers(DT_) over ALL matches with r·sqrt(sigma2), mean and 1.4826·MAD by
 *   vector_mean_stdv_mad, |r − mean| > inlier_k·stdv is an outlier (points only with has_points,
 *   lines only with has_lines); then, with at least min_features inliers, a second loop of at most
 *   max_iters_ref passes that starts again from the INITIAL DT (:352/:356), else DT = I. If the first
 *   solution is not good, the endpoint model runs one loop of max_iters_ref passes on all matches
 *   from the initial DT (:371) and the Plücker model does nothing (:369).
 *   The end (:385-404): isGoodSolution(DT, cov, err) and DT != I (exactly) gives
 *   DT = expmap(logmap(inverse(DT))), DT_cov, err_norm and the eigenvalues; anything else gives
 *   DT = I, DT_cov = 0, err_norm = -1, eigenvalues 0.
 * A pass: the residual lists of the active matches; s_p, s_l = vector_stdv_mad of each (element n/2
 * of the sorted list, the deviations rounded through float by fabsf, an empty list gives 0), clamped
 * to [1e-4, sqrt(7.815)]; w = 1/(1 + (r/s)²), for a line times lineSegmentOverlap of the previous
 * frame's segment and the projected endpoints; H += w·JJᵀ, g += w·J·r, e += w·r², e /= N_l + N_p.
 * Stop if |e − e_prev| < min_error_change or e < min_error; x = H⁻¹g by ColPivHouseholderQR; if its
 * logAbsDeterminant() < 0 the loop's DT is restored, err = −1 and cov = I; DT ← inverse(expmap(x))·DT
 * (on the left); stop if ‖x‖ < min_error_change. After the loop cov = H⁻¹, err = e.
 * Line residuals. PLBA_TRACK_ENDPOINTS: (l·π(sP'), l·π(eP')) with the current frame's line l = le.
 * PLBA_TRACK_PLUCKER: the line n' = R·N + t×(R·D) (TransformForPluker, include2/stereoFrameHandler.h
 * :114-122) in pixels, l = K_pl·n' with K_pl = [fy 0 0; 0 fx 0; −fy·cx −fx·cy fx·fy]
 * (src2/pinholeStereoCamera.cpp:123-125), and the distances of the current frame's two endpoints to
 * it; g (only) is built with r = ‖e‖·sqrt(sigma2), e and the weight with ‖e‖ (:757-781).
 * isGoodSolution here is: smallest eigenvalue >= 0, largest <= 1, 0 <= err <= 1, DT finite, each
 * comparison as written, so that a NaN anywhere is "not good" (the reference's negated comparisons
 * let a NaN covariance or error pass).
 * Defined where the reference is not: a pass with no active match divides 0 by 0: err is NaN, the
 * solution is not good and the identity is returned; a non-finite H or g (a match with z = 0) gives
 * a NaN step and takes the same route, after its iteration caps; a singular last H (H.inverse() is
 * inf / NaN in the reference) gives a NaN covariance, which is not good. None of them disturbs the
 * rest of the batch. Modes 0 and 2 of the endpoint build (gaussNewtonOptimization,
 * levenbergMarquardtOptimization) are dead in the reference (mode = 1) and are not here. */
#define PLBA_TRACK_MAX_N 2048           /* matches of one kind in one problem: the residual list of a
                                           kind sits in a workgroup's LDS whole for the rank selection */
#define PLBA_TRACK_PLUCKER   0          /* plba_track_params.line_model */
#define PLBA_TRACK_ENDPOINTS 1
/* plba_track_out.branch: the path optimizePose took */
#define PLBA_TRACK_OK              0    /* refined, final test passed: DT is the estimate            */
#define PLBA_TRACK_FEW_BEFORE      1    /* fewer than min_features matches (:377-381)                */
#define PLBA_TRACK_FIRST_NOT_GOOD  2    /* the first solution failed isGoodSolution (:366-375); in the
                                           endpoint model err_norm >= 0 tells that the loop on all
                                           matches still passed the final test                       */
#define PLBA_TRACK_FEW_AFTER       3    /* fewer than min_features inliers after removal (:360-364)  */
#define PLBA_TRACK_FINAL_NOT_GOOD  4    /* refined, but the final test failed (:395-404)             */

typedef struct plba_track_batch {       /* K frame pairs, concatenated */
    int32_t n;                          /* problems                                                  */
    const int32_t *pt_off, *ln_off;     /* [n+1] match ranges                                        */
    const double *pt_P;                 /* [.][3] stereo_pt[i1]->P of the previous frame             */
    const double *pt_obs;               /* [.][2] pl_obs: the current frame's pixel (:148)           */
    const double *pt_sigma2;            /* [.]                                                       */
    const double *ln_sP, *ln_eP;        /* [.][3] endpoints in the previous frame's camera           */
    const double *ln_NDc;               /* [.][6] Plücker line (N, D) there; PLBA_TRACK_PLUCKER only */
    const double *ln_le;                /* [.][3] le_obs (:175); PLBA_TRACK_ENDPOINTS only           */
    const double *ln_obs;               /* [.][4] spl_obs, epl_obs (:173-174); PLBA_TRACK_PLUCKER only */
    const double *ln_seg;               /* [.][4] spl, epl: the previous frame's own segment         */
    const double *ln_sigma2;            /* [.]                                                       */
    const double *prev;                 /* [n][53] the previous frame's DT (row-major 4x4), DT_cov
                                           (6x6) and err_norm; read only with use_motion_model       */
    double fx, fy, cx, cy;
} plba_track_batch;

typedef struct plba_track_params {
    double  homog_th;          /* Config::homogTh()        1e-7 (src2/config.cpp:80)                 */
    double  min_error;         /* Config::minError()       1e-7 (:84)                                */
    double  min_error_change;  /* Config::minErrorChange() 1e-7 (:85)                                */
    double  inlier_k;          /* Config::inlierK()        4.0  (:86)                                */
    int32_t min_features;      /* Config::minFeatures()    10   (:81)                                */
    int32_t max_iters;         /* Config::maxIters()       5    (:82)                                */
    int32_t max_iters_ref;     /* Config::maxItersRef()    10   (:83)                                */
    int32_t has_points;        /* Config::hasPoints()      1    (:46)                                */
    int32_t has_lines;         /* Config::hasLines()       1    (:47)                                */
    int32_t use_motion_model;  /* Config::useMotionModel() 0    (:53)                                */
    int32_t line_model;        /* PLBA_TRACK_PLUCKER (the default) or PLBA_TRACK_ENDPOINTS           */
    int32_t pad;
} plba_track_params;

typedef struct plba_track_out {
    int32_t branch;            /* PLBA_TRACK_OK ...                                                  */
    int32_t iters_first;       /* passes (H / g builds) of the first loop                            */
    int32_t iters_ref;         /* passes of the second loop                                          */
    int32_t n_inl_pt, n_inl_ln;/* matches still active at the end                                    */
    int32_t pad;
    double  err_norm;          /* curr_frame->err_norm                                               */
    double  s_p, s_l;          /* the scales of the last pass (0 if there was none)                  */
    double  DT[16];            /* curr_frame->DT, row-major 4x4                                      */
    double  DT_cov[36];        /* curr_frame->DT_cov                                                 */
    double  DT_cov_eig[6];     /* ascending                                                          */
    double  DT_solver[16];     /* the solver's own DT, before the inversion                          */
    double  H[36];             /* last pass, row-major (0 if there was none)                         */
} plba_track_out;

void plba_track_default_params(plba_track_params *p);
/* Runs on the context's stream; needs no uploaded window and leaves one intact; its device buffers
 * are kept and reused across calls. One workgroup per problem, the whole of optimizePose in one
 * launch; the same problem gives bitwise the same result alone or anywhere in a batch. out: [n].
 * pt_inlier [pt_off[n]] / ln_inlier [ln_off[n]] receive the inlier flags (each may be NULL).
 * p == NULL: the defaults. PLBA_E_INVALID for a NULL batch / out / array that the line model reads,
 * n < 0, decreasing (or negative) offsets, an iteration cap below 1, an unknown line model, a NULL
 * prev with use_motion_model, or more than PLBA_TRACK_MAX_N matches of one kind in one problem;
 * n == 0 does nothing and returns PLBA_OK. */
int plba_track_pose(plba_ctx *ctx, const plba_track_batch *b, const plba_track_params *p,
                    plba_track_out *out, uint8_t *pt_inlier, uint8_t *ln_inlier);

/* ---- Frame-to-frame tracking: f2fTracking() followed by optimizePose() in one call
 *   void StereoFrameHandler::f2fTracking()   (src2/stereoFrameHandler.cpp:106-180)
 *   void StereoFrameHandler::optimizePose()  (:307-405)
 * for a batch of K frame pairs, from the features that plba_stereo_associate leaves for a frame to
 * the pose. Per pair and kind: matches_12 = match(prev desc, curr desc, nnr) as plba_desc_match
 * defines it (:141, :164); the previous rows with a match, in increasing i1, are matched_pt /
 * matched_ls (:150, :177), each with the current row's pl (:148), spl / epl (:173-174) and le
 * (:175) as its observation; n_pt / n_ls are their counts (:126-127) and the pose problem of the
 * pair is exactly these rows in this order, solved as plba_track_pose solves it: the result is
 * bitwise what plba_track_pose returns for the same rows. has_points = 0 or an empty side gives
 * no point matches (:137), the same for lines (:160). cur_from_prev is the previous row whose idx
 * the reference copies into a current row (:151, :178): the loop runs in increasing i1 and the
 * last write wins, so it is the largest i1 with matches_12[i1] == i2 (without best_lr several
 * previous rows can share a current row, and all of them enter the pose problem); the caller does
 * curr.idx[i2] = prev.idx[cur_from_prev[i2]]. Nothing is kept between calls.
 * On the device: one upload, k_desc_nn and k_desc_cross over 2K problems, k_f2f_gather (an
 * in-order compaction, one workgroup per pair and kind), k_trackpose, k_f2f_scatter (the inlier
 * flags back to previous-row order), one read-back; no host synchronisation in between. */
typedef struct plba_frames_batch {      /* K frame pairs, concatenated per kind and side */
    int32_t n;                          /* pairs                                                     */
    int32_t pad;
    const int32_t *pt_off1, *pt_off2;   /* [n+1] point rows of the previous / current frame; each of
                                           the four arrays starts at 0                               */
    const int32_t *ln_off1, *ln_off2;   /* [n+1] line rows                                           */
    /* previous frame */
    const uint8_t *prev_pdesc;          /* [pt_off1[n]][desc_bytes]                                  */
    const double *prev_pt_P;            /* [.][3]                                                    */
    const double *prev_pt_sigma2;       /* [.]                                                       */
    const uint8_t *prev_ldesc;          /* [ln_off1[n]][desc_bytes]                                  */
    const double *prev_ln_sP, *prev_ln_eP;  /* [.][3]                                                */
    const double *prev_ln_NDc;          /* [.][6]; PLBA_TRACK_PLUCKER only                           */
    const double *prev_ln_seg;          /* [.][4] spl, epl                                           */
    const double *prev_ln_sigma2;       /* [.]                                                       */
    /* current frame */
    const uint8_t *cur_pdesc;           /* [pt_off2[n]][desc_bytes]                                  */
    const double *cur_pt_pl;            /* [.][2]                                                    */
    const uint8_t *cur_ldesc;           /* [ln_off2[n]][desc_bytes]                                  */
    const double *cur_ln_seg;           /* [.][4] spl, epl; PLBA_TRACK_PLUCKER only                  */
    const double *cur_ln_le;            /* [.][3]; PLBA_TRACK_ENDPOINTS only                         */
    const double *prev;                 /* [n][53] as in plba_track_batch; use_motion_model only     */
    double fx, fy, cx, cy;
} plba_frames_batch;

typedef struct plba_frames_params {
    plba_track_params track;
    float   nnr_pt, nnr_ln;    /* Config::minRatio12P() / minRatio12L() as floats                    */
    int32_t best_lr;           /* Config::bestLRMatches(): 1 = cross-check                           */
    int32_t desc_bytes;        /* as in plba_match_batch                                             */
} plba_frames_params;

typedef struct plba_frames_out {
    plba_track_out *out;                /* [n]                                                       */
    int32_t *pt_m12, *ln_m12;           /* [pt_off1[n]], [ln_off1[n]] matches_12 per previous row,
                                           local to the pair, or -1                                  */
    int32_t *n_pt, *n_ln;               /* [n] n_inliers_pt / n_inliers_ls (:126-127)                */
    uint8_t *pt_inlier, *ln_inlier;     /* per PREVIOUS row, 0 for an unmatched row; may be NULL     */
    int32_t *pt_cur_from_prev, *ln_cur_from_prev;  /* [pt_off2[n]], [ln_off2[n]] or -1               */
} plba_frames_out;

/* track: plba_track_default_params; nnr_pt = nnr_ln = 0.9f (src2/config.cpp:60, :68), best_lr = 1 (:51),
 * desc_bytes = 32 */
void plba_frames_default_params(plba_frames_params *p);
/* Runs on the context's stream; needs no uploaded window and leaves one intact; shares
 * plba_desc_match's device block and pinned host image. p == NULL: the defaults. PLBA_E_INVALID,
 * checked on the host before any launch, for everything plba_desc_match and plba_track_pose refuse
 * (a NULL batch / out / array that is read, n < 0, decreasing offsets, a bad desc_bytes, an
 * iteration cap below 1, an unknown line model, a NULL prev with use_motion_model), for an offset
 * array that does not start at 0, and for a pair whose PREVIOUS frame has more than
 * PLBA_TRACK_MAX_N rows of one kind (matches cannot exceed previous rows; nothing is ever
 * truncated). n == 0 does nothing and returns PLBA_OK. */
int plba_track_frames(plba_ctx *ctx, const plba_frames_batch *b, const plba_frames_params *p,
                      const plba_frames_out *out);

/* ---- Descriptor matching, what feeds the relative pose above and every other matching step of
 * the back end:
 *   int StVO::match(desc1, desc2, nnr, matches_12)          (src2/matching.cpp:63-91)
 *   int StVO::matchNNR(desc1, desc2, nnr, matches_12)       (src2/matching.cpp:41-61)
 * called by isLoopClosure (src/mapHandler.cpp:4334, :4360), matchKF2KFPoints / Lines (:280, :427),
 * matchMap2KFPoints / Lines (:762, :877) and the VO's tracking (src2/stereoFrameHandler.cpp:141,
 * :164). BFMatcher(NORM_HAMMING).knnMatch(k = 2) in both directions, a nearest-neighbour-ratio test
 * and a left/right cross-check. Integer work: the results are exact.
 * Nearest neighbours, per pair and direction: for each query row the smallest and second-smallest
 * Hamming distance over the train rows, scanned in increasing train index; a distance replaces the
 * best only if strictly smaller, otherwise the second only if strictly smaller, so ties go to the
 * lowest train index (OpenCV's batch distance; matchGrid's own loop, matching.cpp:152-157).
 * Ratio test: a row is matched if (float)d0 < (float)d1 * nnr, a single-precision product and
 * compare (matching.cpp:54: DMatch::distance and nnr are floats). In double it would differ, e.g.
 * for nnr = 0.6f, d0 = 6, d1 = 10.
 * Cross-check: with best_lr a match i1 -> i2 survives only if the reverse pass, with the same
 * ratio, matched i2 -> i1 (:80-86). matches_12 is local to the pair: the row index within the
 * pair's own desc2 slice, or -1. n_matches[k] is the surviving count, the function's return value.
 * Defined where the reference is not: a pair with fewer than 2 train rows in a direction has no
 * match in that direction (the reference reads matches_[idx][1] out of range); a pair with 0 rows
 * on either side has 0 matches. Neither disturbs the rest of the batch.
 * A call matches a batch of descriptor-set pairs, both directions, in two kernel launches. */
typedef struct plba_match_batch {       /* B descriptor-set pairs, concatenated */
    int32_t n;                          /* pairs                                              */
    int32_t desc_bytes;                 /* bytes per descriptor: a multiple of 4 in [4, 64];
                                           ORB and LBD are 32                                 */
    const int32_t *off1, *off2;         /* [n+1] row ranges into desc1 / desc2                */
    const uint8_t *desc1, *desc2;       /* [off1[n]][desc_bytes], [off2[n]][desc_bytes]       */
    const float   *nnr;                 /* [n] ratio per pair (minRatio12P / minRatio12L as float) */
    int32_t best_lr;                    /* Config::bestLRMatches(): 1 = cross-check (default) */
    int32_t pad;
} plba_match_batch;
/* Runs on the context's stream; needs no uploaded window and leaves one intact; its device block
 * and pinned host image are kept and reused across calls. matches_12: [off1[n]], n_matches: [n].
 * PLBA_E_INVALID for a NULL batch or array (desc1 / matches_12 may be NULL when off1[n] == 0,
 * desc2 when off2[n] == 0), n < 0, decreasing or negative offsets or a bad desc_bytes; n == 0 does
 * nothing and returns PLBA_OK. */
int plba_desc_match(plba_ctx *ctx, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches);

/* ---- Median descriptor of a batch of descriptor lists: the descriptor half of
 *   void MapPoint::updateAverageDescDir() / MapLine::updateAverageDescDir()  (src/mapFeatures.cpp:52-86, :140-174)
 * which loopClosureFuseLandmarks (src/mapHandler.cpp:5636, :5784) runs after every observation it
 * appends. For a list of n descriptors, row i of the symmetric n x n Hamming table (zero diagonal)
 * has a k-th smallest value, k = min(int(1 + 0.5 (n - 1)), n - 1); medoid[.] is the first i whose
 * value is strictly smaller than that of every earlier row (the start value 99999 is above any
 * distance), as a position within the list. Integer work: the result is exact. The k-th smallest
 * value is found by counting, not by sorting.
 * Defined where the reference is not: an empty list gives -1; a list of one gives 0 (the reference
 * reads one past the row's end, k is clamped here as the host mirror clamps it).
 * One kernel launch per call: a wave per list of at most 64 descriptors, a workgroup of four waves
 * per longer list. The largest list is 1024 descriptors: a list sits in the workgroup's LDS whole
 * (1024 x 64 bytes = 64 KiB). A longer one is refused, never truncated. */
typedef struct plba_medoid_batch {      /* B descriptor lists, concatenated */
    int32_t n;                          /* lists                                              */
    int32_t desc_bytes;                 /* bytes per descriptor: a multiple of 4 in [4, 64]   */
    const int32_t *list_ptr;            /* [n+1] row ranges into desc                         */
    const uint8_t *desc;                /* [list_ptr[n]][desc_bytes]                          */
} plba_medoid_batch;
#define PLBA_MEDOID_MAX_N 1024
/* Runs on the context's stream; needs no uploaded window and leaves one intact; shares
 * plba_desc_match's device block and pinned host image. medoid: [n]. PLBA_E_INVALID for a NULL
 * batch or array (desc may be NULL when list_ptr[n] == 0), n < 0, decreasing or negative offsets, a
 * bad desc_bytes or a list of more than PLBA_MEDOID_MAX_N descriptors; n == 0 does nothing and
 * returns PLBA_OK. */
int plba_desc_medoid(plba_ctx *ctx, const plba_medoid_batch *b, int32_t *medoid);

/* ---- Grid-guided descriptor matching, what the local-mapping associations try first:
 *   int StVO::matchGrid(points1, desc1, grid, desc2, w, matches_12)               (src2/matching.cpp:111-177)
 *   int StVO::matchGrid(lines1, desc1, grid, desc2, directions2, w, matches_12)   (:179-258)
 * called by matchKF2KFPoints / Lines (src/mapHandler.cpp:273, :421) and matchMap2KFPoints / Lines
 * (:756, :871) when SlamConfig::fastMatching() is set. The train rows (side 2) sit in a cols x rows
 * grid of cells (GridStructure, 64 x 48 in the reference): a point in one cell, a rasterised line in
 * several. A query row (side 1) has an integer cell, a line query two (start and end point), already
 * truncated by the caller (point_2d is pair<int, int>); they may lie outside the grid. A problem has
 * a kind (0 points, 1 lines), a window half-width ws, a ratio nnr and, for lines, a direction
 * threshold. Integer work but for two double comparisons: the results are exact.
 * Candidates: cand(i1, i2) if some cell (cx, cy) of i2 inside [0, cols) x [0, rows) has
 * max(0, x - ws) <= cx < min(cols, x + ws + 1) and the same in y for the query cell (GridStructure::
 * get, src2/gridStructure.cpp:65-76); a listed cell outside the grid is ignored (GridStructure::at).
 * A line query takes the test for either of its two cells and also needs |dot(v1, dir2[i2])| >=
 * line_sim_th (:221), v1 = the integer difference of its cells divided by its norm, in double. For
 * two equal cells v1 is NaN, the comparison of :221 is false and the row is kept: the direction
 * test passes. A train row counts once however many of its cells are in the window.
 * Cross-check with best_lr: the query rows are taken in increasing i1, and (i1, i2) is seen by row
 * i1 only if its Hamming distance is strictly below that of every earlier candidate of column i2
 * (:145-150); matches_21[i2] is the last such i1. Without best_lr every candidate is seen.
 * Best and second best of a row over its seen pairs in increasing i2: a distance replaces the best
 * only if strictly smaller, else the second only if strictly smaller (:152-157), so the lowest i2
 * wins a tie. (The reference iterates an unordered_set there: its order is unspecified.)
 * Ratio test: (double)best_d < (double)best_d2 * nnr (:160; Config::minRatio12P() is a double), with
 * INT_MAX for a missing second. Then, with best_lr, matches_12[i1] = i2 survives only if
 * matches_21[i2] == i1 (:166-174). n_matches[p] is the surviving count, the function's return value.
 * Defined where the reference is not: a row with candidates but no seen pair has best_d = INT_MAX;
 * above nnr = 1 the reference counts a match with index -1 there. Here it is -1 and not counted.
 * A problem has at most 65535 train rows. */
typedef struct plba_gridmatch_batch {   /* B problems, concatenated */
    int32_t n;                          /* problems                                             */
    int32_t desc_bytes;                 /* as in plba_match_batch                               */
    int32_t cols, rows;                 /* the grid, > 0 (GRID_COLS 64, GRID_ROWS 48)           */
    int32_t best_lr;                    /* Config::bestLRMatches()                              */
    int32_t pad;
    const int32_t *off1, *off2;         /* [n+1] row ranges of problem p: [off[p], off[p+1])    */
    const uint8_t *desc1, *desc2;       /* [off1[n]][desc_bytes] queries, [off2[n]][desc_bytes] */
    const int32_t *cell1;               /* [off1[n]][2] (x, y) of a point query, of a line's start */
    const int32_t *cell1_end;           /* [off1[n]][2] of a line query's end; rows of point
                                           problems are not read; NULL with no line query       */
    const int32_t *cell_off2;           /* [off2[n]+1] CSR: cells of train row r are
                                           cells2[cell_off2[r] .. cell_off2[r+1])               */
    const int32_t *cells2;              /* [cell_off2[off2[n]]][2] (x, y)                       */
    const double  *dir2;                /* [off2[n]][2] unit direction of a train line; rows of
                                           point problems are not read; NULL with no train line */
    const int32_t *kind;                /* [n] 0 points, 1 lines                                */
    const int32_t *ws;                  /* [n] window half-width, >= 0 (matchingF2FWs, 3)       */
    const double  *nnr;                 /* [n] Config::minRatio12P(), for lines too (:241)      */
    const double  *line_sim_th;         /* [n] Config::lineSimTh(), 0.75; read for lines        */
} plba_gridmatch_batch;
/* Runs on the context's stream in a fixed number of launches with one upload and one read-back;
 * needs no uploaded window and leaves one intact; shares plba_desc_match's device block and pinned
 * host image. matches_12: [off1[n]], local to the problem; n_matches: [n].
 * PLBA_E_INVALID for a NULL batch or array where rows exist, n < 0, decreasing or negative offsets
 * (rows or cells), ws < 0, cols or rows <= 0, a bad desc_bytes, a kind outside {0, 1} or more than
 * 65535 train rows in a problem; n == 0 does nothing; an empty side gives no match. */
int plba_grid_match(plba_ctx *ctx, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches);

/* ---- Stereo association of a frame's features, what makes stereo_pt / stereo_ls of every frame:
 *   StereoFrame::matchStereoPoints(points_l, points_r, pdesc_l, pdesc_r, initial)   (src2/stereoFrame.cpp:121-174)
 *   StereoFrame::matchStereoLines(lines_l, lines_r, ldesc_l, ldesc_r, initial)      (:310-435)
 * from the detector output of the left and the right image (cv::KeyPoint::pt; KeyLine::startPointX,
 * startPointY, endPointX, endPointY: all float). A call takes a batch of frames, each with its point
 * and its line problem. Detection, octave, angle and the idx that `initial` assigns stay the caller's:
 * pt_src / ls_src give the left row of every survivor.
 * Cells. inv_width = cols / (double)width, inv_height = rows / (double)height (:47-48). A left
 * feature's query cell is ((int)(x * inv_width), (int)(y * inv_height)): the float promoted to double,
 * one double product, truncated toward zero (:133, :322-323: point_2d is pair<int, int>); a line has
 * the cell of its start and of its end. A right point is entered in its one cell (:139). A right line
 * is entered in the cells of getLineCoords over its endpoints in grid units (:336; the walk of
 * plslam_line_cells), and its direction is normalize(((ex - sx) * inv_width, (ey - sy) * inv_height))
 * with the differences taken in float first (:333).
 * Window. w.width = (matching_s_ws, 0), w.height = (0, 0) (:142-144): the candidates of a query cell
 * (x, y) are the right rows with an in-grid cell (cx, cy), max(0, x - matching_s_ws) <= cx <
 * min(cols, x + 1) and max(0, y) <= cy < min(rows, y + 1) (GridStructure::get, src2/gridStructure.cpp:
 * 65-76). Everything else is matchGrid exactly as plba_grid_match defines it above: candidate order,
 * the prefix-minimum cross-check with best_lr, the direction test against line_sim_th, the ratio test
 * in double with min_ratio_12_p for points and lines alike.
 * Point gates, for a match i1 -> i2 (:158-161): (double)|yl - yr| <= max_dist_epip with the
 * difference and its absolute value in float; disp = (double)(xl - xr), the difference in float;
 * disp >= min_disp. Then pl = (xl, yl) and P = backProjection(xl, yl, disp) (src2/pinholeStereoCamera.
 * cpp:225-233): bd = b / disp, P = (bd * (u - cx), bd * (v - cy), bd * fx).
 * Line part (:357-397), every float promoted first. sp_l = (sx, sy, 1), ep_l = (ex, ey, 1), le = sp_l x
 * ep_l divided, component by component, by sqrt(le0 * le0 + le1 * le1). overlap =
 * lineSegmentOverlapStereo(sy_l, ey_l, sy_r, ey_r) (:510-545) on the right line's own endpoints: 1 if
 * |ey_l - sy_l| <= line_horiz_th; else with sln / eln the smaller / larger left y and spn / epn of the
 * right, length = eln - spn; 0 if epn < sln or spn > eln, eln - sln if epn > eln and spn < sln, else
 * min(eln, epn) - max(sln, spn); divided by length if length > (double)0.01f, else 0; at most 1.
 * Then :367 overwrites sp_r and :368 reads what it wrote:
 *   X  = (sx_r * (sy_l - ey_r) + ex_r * (sy_r - sy_l)) / (sy_r - ey_r),     sp_r = (X, sy_l)
 *   Xe = (X * (ey_l - ey_r) + ex_r * (sy_l - ey_l)) / (sy_l - ey_r),        ep_r = (Xe, ey_l)
 * sdisp = sx_l - X, edisp = ex_l - Xe; if min(sdisp, edisp) / max(sdisp, edisp) < ls_min_disp_ratio
 * both become -1 (:442-452; std::min(a, b) = b < a ? b : a, std::max(a, b) = a < b ? b : a). The five
 * gates (:372-375): sdisp >= min_disp, edisp >= min_disp, |sy_l - ey_l| > line_horiz_th, |sp_r(1) -
 * ep_r(1)| > line_horiz_th, which after the overwrite is the same |sy_l - ey_l| again, and overlap >
 * stereo_overlap_th. sP = backProjection(sx_l, sy_l, sdisp), eP = backProjection(ex_l, ey_l, edisp).
 * With pluker (a USE_LINE_PLUKER build, :383-397, :870-883): unit(u, v) = ((u - cx) / fx, (v - cy) / fy,
 * 1); a = unit(sp_l), c = unit(ep_l), a2 = unit(sp_r) + (b, 0, 0), c2 = unit(ep_r) + (b, 0, 0) with the
 * overwritten sp_r / ep_r, o1 = 0, o2 = (b, 0, 0); pi_from_ppp(x1, x2, x3) = ((x1 - x3) x (x2 - x3),
 * -(x3 . (x1 x x2))), the dot product summed as t0 + (t1 + t2) (Eigen's unrolled reduction of three);
 * pi1 = pi_from_ppp(a, c, o1), pi2 = pi_from_ppp(a2, c2, o2); dp(i, j) = pi1[i] * pi2[j] - pi2[i] *
 * pi1[j]; NDc = (dp03, dp13, dp23, -dp12, dp02, -dp01). A cross product is (a1 b2 - a2 b1, a2 b0 -
 * a0 b2, a0 b1 - a1 b0).
 * Arithmetic: every double operation is rounded once (no fused multiply-add); only + - * / sqrt occur,
 * so the doubles are bit for bit those of a host evaluation in this order.
 * Defined where the reference is not: a frame side with no rows gives no survivor and does not
 * disturb the batch; NaN (0 / 0 in X for sy_r == ey_r, say) compares false in every gate, as in C++.
 * A coordinate must be finite and at most one image size outside the image: -width <= x <= 2 * width,
 * -height <= y <= 2 * height. That bounds the walk of a right line: it advances one cell per step along
 * the axis of larger extent from (int)first to (int)last (src2/lineIterator.cpp:53-76), and both lie in
 * [-size, 2 * size] grid units, so a line has at most 3 * max(cols, rows) + 1 cells. Their coordinates
 * along that axis are distinct, so at most max(cols, rows) of them lie inside the grid. */
typedef struct plba_stereo_params {
    int32_t cols, rows;                 /* GRID_COLS 64, GRID_ROWS 48 (include2/stereoFrame.h)   */
    int32_t width, height;              /* the image size, > 0                                   */
    int32_t matching_s_ws;              /* Config::matchingSWs()        10 (src2/config.cpp:91)  */
    int32_t best_lr;                    /* Config::bestLRMatches()       1 (:51)                 */
    int32_t pluker;                     /* 1: a USE_LINE_PLUKER build, NDc is computed           */
    int32_t pad;
    double  min_ratio_12_p;             /* Config::minRatio12P()       0.9 (:60)                 */
    double  line_sim_th;                /* Config::lineSimTh()        0.75 (:63)                 */
    double  max_dist_epip;              /* Config::maxDistEpip()       1.0 (:58)                 */
    double  min_disp;                   /* Config::minDisp()           1.0 (:59)                 */
    double  ls_min_disp_ratio;          /* Config::lsMinDispRatio()    0.7 (:69)                 */
    double  line_horiz_th;              /* Config::lineHorizTh()       0.1 (:67)                 */
    double  stereo_overlap_th;          /* Config::stereoOverlapTh()  0.75 (:64)                 */
    double  fx, fy, cx, cy, b;          /* PinholeStereoCamera                                   */
} plba_stereo_params;
typedef struct plba_stereo_batch {      /* n frames, concatenated */
    int32_t n;                          /* frames                                                */
    int32_t desc_bytes;                 /* as in plba_match_batch                                */
    const int32_t *pt_off_l, *pt_off_r; /* [n+1] point rows of frame f: [off[f], off[f+1])       */
    const int32_t *ls_off_l, *ls_off_r; /* [n+1] line rows                                       */
    const float   *pt_l, *pt_r;         /* [.][2] (x, y) of the left / right keypoints           */
    const uint8_t *pdesc_l, *pdesc_r;   /* [.][desc_bytes]                                       */
    const float   *ls_l, *ls_r;         /* [.][4] (sx, sy, ex, ey) of the left / right segments  */
    const uint8_t *ldesc_l, *ldesc_r;   /* [.][desc_bytes]                                       */
} plba_stereo_batch;
/* The survivors of frame f, compacted in increasing left index (the order the reference pushes
 * them): n_pt[f] rows from row pt_off_l[f] of every point array, n_ls[f] rows from row ls_off_l[f] of
 * every line array. Rows past the count are not written. n_pt and n_ls are required; any other array
 * may be NULL and is then skipped. ls_NDc is written only with params.pluker. */
typedef struct plba_stereo_out {
    int32_t *n_pt, *n_ls;               /* [n]                                                   */
    int32_t *pt_src;                    /* [pt_off_l[n]] the left row i1, local to the frame     */
    double  *pt_pl, *pt_disp, *pt_P;    /* [.][2], [.], [.][3]                                   */
    uint8_t *pdesc;                     /* [.][desc_bytes] the filtered pdesc_l                  */
    int32_t *ls_src;                    /* [ls_off_l[n]]                                         */
    double  *ls_spl, *ls_epl;           /* [.][2]                                                */
    double  *ls_sdisp, *ls_edisp;       /* [.]                                                   */
    double  *ls_sP, *ls_eP, *ls_le;     /* [.][3]                                                */
    double  *ls_NDc;                    /* [.][6]                                                */
    uint8_t *ldesc;                     /* [.][desc_bytes] the filtered ldesc_l                  */
} plba_stereo_out;
/* The defaults of src2/config.cpp:51-91 with the grid of include2/stereoFrame.h; width, height, the
 * camera and pluker are zero and must be set. */
void plba_stereo_default_params(plba_stereo_params *p);
/* Runs on the context's stream in a fixed number of launches (the cells, the matcher's three, the
 * gates) with one upload and one read-back; needs no uploaded window and leaves one intact; shares
 * plba_desc_match's device block and pinned host image. PLBA_E_INVALID, checked on the host before
 * anything is launched, for a NULL batch, params, out, n_pt, n_ls or offset array, a NULL input array
 * where rows exist, n < 0, decreasing or negative offsets, a bad desc_bytes, cols, rows, width or
 * height <= 0, matching_s_ws < 0, more than 65535 right rows in a problem, or a coordinate that is not
 * finite or outside the bound above; n == 0 does nothing and returns PLBA_OK. */
int plba_stereo_associate(plba_ctx *ctx, const plba_stereo_batch *b, const plba_stereo_params *p,
                          const plba_stereo_out *out);

/* ---- Keyframe-to-keyframe association, the first half of lookForCommonMatches and the only place
 * where map landmarks are created:
 *   MapHandler::matchKF2KFPoints(prev_kf, curr_kf)    (src/mapHandler.cpp:237-366)
 *   MapHandler::matchKF2KFLines(prev_kf, curr_kf)     (:368-695, the USE_LINE_PLUKER branch :433-590)
 * up to, and without, the sequential part that builds the landmarks: the matches of every previous row
 * and the geometry a new or extended landmark needs, indexed by previous row. A call takes a batch of
 * keyframe pairs; pair f is the matcher's problems 2 f (points) and 2 f + 1 (lines). The previous
 * keyframe's rows are the query side (1), the current keyframe's the train side (2).
 * Sums. A sum of three terms t0, t1, t2 is t0 + (t1 + t2) (Eigen's unrolled reduction of three, as in the
 * stereo block). R x + t for a pose T = (R, t) is (R_i0 x0 + (R_i1 x1 + R_i2 x2)) + t_i, and the norm of
 * x is sqrt(x0 x0 + (x1 x1 + x2 x2)). A cross product is (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
 * Query cells. inv_width = cols / (double)width, inv_height = rows / (double)height. A previous point
 * projects as Q = DT.R P + DT.t, u = cx + fx * Q0 / Q2 (the product first, then the quotient), v = cy +
 * fy * Q1 / Q2 (src2/pinholeStereoCamera.cpp:235-241); there is no depth check (:258). Its cell is
 * ((int)(u * inv_width), (int)(v * inv_height)) (:259). A previous line's two cells are the truncated
 * pixel coordinates ((int)u, (int)v) of its projected sP and eP: :395-396 does not scale them, unlike
 * :823-824. With line_query_in_grid_units they are scaled like a point's. Converting a double that is
 * not finite or out of range to int is undefined in the reference; here, if a cell's coordinate g (after
 * the scaling, if any) has !(fabs(g) < 2^30) in x or in y, the cell is (-2^30, -2^30): its clipped window
 * is empty, so the grid stage has no match for that row.
 * Train side. A current point is entered in the cell ((int)(pl0 * inv_width), (int)(pl1 * inv_height))
 * (:266). A current line is entered in the cells of getLineCoords over (spl * inv, epl * inv) (:410-411,
 * the walk of plslam_line_cells), with the direction normalize(((epl0 - spl0) * inv_width, (epl1 - spl1)
 * * inv_height)) (:407-408): mag = sqrt(x x + y y), then two divisions. A current coordinate must be
 * finite and at most one image size outside the image, as in the stereo block: that bounds the walk.
 * Matching. With fast_matching, matchGrid as plba_grid_match defines it, window (ws, ws, ws, ws), ratio
 * min_ratio_12_p for points and lines alike (matching.cpp:160, :241). Without it the grid count is 0.
 * The brute-force fallback (:277-281, :424-429) replaces a problem's matches when n2 > min and n1 > min
 * and grid count < min, min = min_pt_matches or min_ls_matches; it is match() as plba_desc_match defines
 * it with the ratio (float)min_ratio_12_p or (float)min_ratio_12_l. The fallback's result stands alone:
 * the reference's match() resizes matches_12 without clearing it, so a grid match that the brute-force
 * ratio test does not replace can survive there; here it does not. The decision is taken on the device.
 * Point record [9], for a row with a match i1 -> i2 (:299-318, :339-341): P3d = T_prev.R P1 + T_prev.t;
 * dir_prev = P3d / |P3d|; dir_curr = Pc / |Pc| with Pc = T_curr.R P2 + T_curr.t, each component divided.
 * Line record [8] (:450-494, :546-562). TransformForPluker(T, (N, D)) (include/mapHandler.h:232-240) is
 * head = (R_i . N) + (M_i . D), tail = R_i . D, with column j of M the cross product t x R_col_j and the
 * structural zeros of the 6 x 6 skipped. For a row with ls_new (the feature's idx is -1): L =
 * TransformForPluker(T_prev, NDc), d = |L.head| / |L.tail|, new_pluker_lw = ((L.head_i / |L.head|) * d,
 * L.tail_i / |L.tail|). The error of a world line W seen from Tcw against the image segment (s, e):
 * h = head of TransformForPluker(Tcw, W); lx = fy * h0, ly = fx * h1, lz = (-fy * cx) h0 + ((-fx * cy) h1
 * + (fx * fy) h2) (getPlukerK, src2/pinholeStereoCamera.cpp:123-125); f = sqrt(lx lx + ly ly); e0 = ((s0 lx
 * + s1 ly) + lz) / f, e1 the same with e; the norm sqrt(e0 e0 + e1 e1). err_prev (new rows only) is that
 * of new_pluker_lw from Tcw_prev against the previous row's (spl, epl); err_curr against the current
 * row's, of new_pluker_lw from Tcw_curr for a new row, of ls_lm_NDw for a row that carries a landmark.
 * ls_rejected = err_curr > sqrt(5.991) (:489, :557); NaN compares false. The record is new_pluker_lw[6],
 * err_prev, err_curr; what a row does not compute is 0, and a row without a match has a zero record.
 * Tcw_prev / Tcw_curr are the caller's T.inverse() (Eigen's general inverse): the device does not invert.
 * Arithmetic: doubles, only + - * / sqrt, one rounding per operation, as in the stereo block. */
typedef struct plba_kfassoc_params {
    int32_t cols, rows;                 /* GRID_COLS 64, GRID_ROWS 48                            */
    int32_t width, height;              /* the image size, > 0                                   */
    int32_t fast_matching;              /* SlamConfig::fastMatching(): 1 as the shipped yaml has */
    int32_t ws;                         /* Config::matchingF2FWs()     3 (src2/config.cpp:92)  */
    int32_t best_lr;                    /* Config::bestLRMatches()       1 (src2/config.cpp:51)  */
    int32_t min_pt_matches;             /* SlamConfig::minPointMatches() 10                      */
    int32_t min_ls_matches;             /* SlamConfig::minLineMatches()   6                      */
    int32_t line_query_in_grid_units;   /* 0: the reference's pixel-unit line query (:395-396)   */
    double  min_ratio_12_p;             /* Config::minRatio12P()       0.9 (:60)                 */
    double  min_ratio_12_l;             /* Config::minRatio12L()       0.9 (:68)                 */
    double  line_sim_th;                /* Config::lineSimTh()        0.75 (:63)                 */
    double  fx, fy, cx, cy;             /* PinholeStereoCamera                                   */
} plba_kfassoc_params;
typedef struct plba_kfassoc_batch {     /* n keyframe pairs, concatenated; _p previous, _c current */
    int32_t n;
    int32_t desc_bytes;                 /* as in plba_match_batch                                */
    const int32_t *pt_off_p, *pt_off_c; /* [n+1] point rows of pair f: [off[f], off[f+1])        */
    const int32_t *ls_off_p, *ls_off_c; /* [n+1] line rows                                       */
    const double  *DT;                  /* [n][12] 3 x 4, row-major                              */
    const double  *T_prev, *T_curr;     /* [n][16] T_kf_w of the two keyframes, row-major        */
    const double  *Tcw_prev, *Tcw_curr; /* [n][16] their inverses                                */
    const double  *pt_P_p;              /* [.][3]                                                */
    const uint8_t *pdesc_p;             /* [.][desc_bytes]                                       */
    const double  *ls_sP_p, *ls_eP_p;   /* [.][3]                                                */
    const double  *ls_NDc_p;            /* [.][6]                                                */
    const double  *ls_spl_p, *ls_epl_p; /* [.][2]                                                */
    const uint8_t *ldesc_p;
    const double  *ls_lm_NDw;           /* [.][6] the map line's NDw where ls_new is 0, else 0   */
    const uint8_t *ls_new;              /* [.] 1 where the feature's idx is -1                   */
    const double  *pt_pl_c;             /* [.][2]                                                */
    const double  *pt_P_c;              /* [.][3]                                                */
    const uint8_t *pdesc_c;
    const double  *ls_spl_c, *ls_epl_c; /* [.][2]                                                */
    const uint8_t *ldesc_c;
} plba_kfassoc_batch;
/* Indexed by previous row, not compacted: the sequential part needs them in row order. n_grid,
 * n_matches and fallback are required; any other array may be NULL and is then skipped. */
typedef struct plba_kfassoc_out {
    int32_t *n_grid, *n_matches, *fallback; /* [2n] per problem: 2 f points, 2 f + 1 lines       */
    int32_t *pt_m12;                    /* [pt_off_p[n]] the current row, local to the pair, or -1 */
    int32_t *ls_m12;                    /* [ls_off_p[n]]                                         */
    double  *pt_rec;                    /* [.][9] P3d, dir_prev, dir_curr                        */
    double  *ls_rec;                    /* [.][8] new_pluker_lw, |err_prev|, |err_curr|          */
    uint8_t *ls_rejected;               /* [.]                                                   */
} plba_kfassoc_out;
/* src/slamConfig.cpp and src2/config.cpp, fast_matching as the shipped configuration files have it;
 * width, height and the camera are zero and must be set. */
void plba_kfassoc_default_params(plba_kfassoc_params *p);
/* Runs on the context's stream in a fixed number of launches (the cells, the matcher's three, the
 * brute-force matcher's two, which return at once where a problem does not fall back, and the geometry)
 * with one upload and one read-back; needs no uploaded window and leaves one intact; shares
 * plba_desc_match's device block and pinned host image. PLBA_E_INVALID, checked on the host before
 * anything is launched, for a NULL batch, params, out, n_grid, n_matches, fallback or offset array, a
 * NULL input array where rows exist, n < 0, decreasing or negative offsets, a bad desc_bytes, cols, rows,
 * width or height <= 0, ws < 0 or ws >= 2^30, more than 65535 current rows in a problem, a DT, T or Tcw
 * that is not finite, or a current coordinate that is not finite or outside the bound above; n == 0 does
 * nothing and returns PLBA_OK. */
int plba_kf_associate(plba_ctx *ctx, const plba_kfassoc_batch *b, const plba_kfassoc_params *p,
                      const plba_kfassoc_out *out);

/* ---- Map-to-keyframe association, the second half of lookForCommonMatches, run for every new keyframe:
 *   MapHandler::matchMap2KFPoints()    (src/mapHandler.cpp:697-797)
 *   MapHandler::matchMap2KFLines()     (:799-921, the endpoint-line arithmetic of :885-907)
 * up to, and without, the sequential part that changes the map (idx, addMapPointObservation /
 * addMapLineObservation, full_graph): the match of every candidate landmark, the epipolar test and the
 * geometry an accepted observation needs, indexed by candidate row. A call takes a batch of keyframes;
 * keyframe f is the matcher's problems 2 f (points) and 2 f + 1 (lines). The candidate landmarks are the
 * query side (1), the keyframe's unmatched features the train side (2). The caller passes as candidates
 * the landmarks with local && kf_obs_list.back() != kf_idx (:712, :813) and as features those with idx ==
 * -1 (:730, :835), in the reference's order: filters on map state, which stay the caller's.
 * Sums and products are those of the keyframe-to-keyframe block above: a sum of three is t0 + (t1 + t2),
 * R x + t is (R_i0 x0 + (R_i1 x1 + R_i2 x2)) + t_i, the norm of x is sqrt(x0 x0 + (x1 x1 + x2 x2)).
 * Visibility (:714-716, :815-820). Q = Twf.R X + Twf.t; u = cx + fx * Q0 / Q2, v = cy + fy * Q1 / Q2 (the
 * product first, then the quotient). A row is visible iff u > 0 && u < width && v > 0 && v < height && Q2 >
 * 0.0; a line iff both endpoints of ls_X (line3D: start, then end) pass. NaN compares false: a landmark
 * that is not finite is invisible, not refused.
 * Query cells. inv_width = cols / (double)width, inv_height = rows / (double)height. A visible point has
 * the cell ((int)(u * inv_width), (int)(v * inv_height)) (:719). A visible line has the cells of both
 * projected endpoints in grid units (:823-824), unlike matchKF2KFLines, which leaves them in pixels.
 * Train side. Exactly that of plba_kf_associate for its current keyframe: a point feature is entered in
 * the cell ((int)(pl0 * inv_width), (int)(pl1 * inv_height)) (:748), a line feature in the cells of
 * getLineCoords over (spl * inv, epl * inv) with the direction normalize(((epl0 - spl0) * inv_width, (epl1
 * - spl1) * inv_height)) (:857-863). A feature coordinate must be finite and at most one image size
 * outside the image, which bounds the walk.
 * Invisible rows. The reference compacts the visible rows in map order and matches the compacted list
 * (:718-720, :822-825). Here every output is indexed by candidate row and equals what the reference
 * computes on the compacted list with the indices mapped back: an invisible row is inert in both
 * matchers. In the grid stage it has the cell (-2^30, -2^30), whose clipped window is empty, so it is seen
 * by no column and touches neither `distances` nor matches_21; in the brute-force stage it has no
 * nearest feature and is no feature's nearest row (the fallback runs only where at least two rows are
 * visible: grid count < min < n_visible). matchGrid's order-dependent left/right check
 * and match()'s lowest-index ties depend only on the relative order of the visible rows, which is kept.
 * Matching. With fast_matching, matchGrid as plba_grid_match defines it, window (ws, ws, ws, ws), ratio
 * min_ratio_12_p for points and lines alike (matching.cpp:160, :241). Without it the grid count is 0.
 * Fallback (:759-764, :874-879). It runs iff n_visible > min && grid count < min, min = min_pt_matches or
 * min_ls_matches: both size tests of the reference read the number of visible landmarks, and, unlike
 * matchKF2KF*, the feature side's size is not tested. It is match() as plba_desc_match defines it with the
 * ratio (float)min_ratio_12_p or (float)min_ratio_12_l, and its result stands alone, as in
 * plba_kf_associate. n_visible is known only on the device: the decision is taken there.
 * Point test and record [6], for a row with a match i1 -> i2 (:770-784): err = sqrt(du du + dv dv), du =
 * u - pl0, dv = v - pl1; accepted iff err < max_kf_epip_p. dir = T_kf_w.R (P / |P|) + T_kf_w.t, each
 * component of P divided by the norm: the translation is added to a direction, kept from the reference.
 * The record is u, v, err, dir[3].
 * Line test and record [9] (:885-907), (su, sv) and (eu, ev) the projections of the two endpoints: err0 =
 * (le0 * su + le1 * sv) + le2, err1 = (le0 * eu + le1 * ev) + le2; accepted iff err0 < max_kf_epip_l && err1
 * < max_kf_epip_l. The test is signed, kept from the reference: a large negative error passes. mid =
 * y / |y| with y = T_kf_w.R m + T_kf_w.t, m_i = 0.5 * (sP_i + eP_i): the observation direction of an
 * endpoint-line build (:899-901), always computed. The record is su, sv, eu, ev, err0, err1, mid[3].
 * An invisible or unmatched row has a zero record and is not accepted; NaN compares false in both tests.
 * Defined where the reference is not: an empty side gives no match and does not disturb the batch (the
 * reference returns before matching, :736, :841; the fallback flag is still n_visible > min && grid count
 * < min). Arithmetic: doubles, only + - * / sqrt, one rounding per operation, as in the stereo block. */
typedef struct plba_mapassoc_params {
    int32_t cols, rows;                 /* GRID_COLS 64, GRID_ROWS 48                            */
    int32_t width, height;              /* the image size, > 0                                   */
    int32_t fast_matching;              /* SlamConfig::fastMatching(): 1 as the shipped yaml has */
    int32_t ws;                         /* Config::matchingF2FWs()       3 (src2/config.cpp:92)  */
    int32_t best_lr;                    /* Config::bestLRMatches()       1 (src2/config.cpp:51)  */
    int32_t min_pt_matches;             /* SlamConfig::minPointMatches() 10                      */
    int32_t min_ls_matches;             /* SlamConfig::minLineMatches()   6                      */
    int32_t pad;
    double  min_ratio_12_p;             /* Config::minRatio12P()       0.9 (:60)                 */
    double  min_ratio_12_l;             /* Config::minRatio12L()       0.9 (:68)                 */
    double  line_sim_th;                /* Config::lineSimTh()        0.75 (:63)                 */
    double  max_kf_epip_p;              /* SlamConfig::maxKFEpipP()    1.0 (src/slamConfig.cpp:51) */
    double  max_kf_epip_l;              /* SlamConfig::maxKFEpipL()    1.0 (:52)                 */
    double  fx, fy, cx, cy;             /* PinholeStereoCamera                                   */
} plba_mapassoc_params;
typedef struct plba_mapassoc_batch {    /* n keyframes, concatenated; _m map candidates, _f features */
    int32_t n;
    int32_t desc_bytes;                 /* as in plba_match_batch                                */
    const int32_t *pt_off_m, *pt_off_f; /* [n+1] point rows of keyframe f: [off[f], off[f+1])    */
    const int32_t *ls_off_m, *ls_off_f; /* [n+1] line rows                                       */
    const double  *Twf;                 /* [n][12] 3 x 4, row-major: world -> keyframe           */
    const double  *T_kf_w;              /* [n][16] the keyframe's pose, row-major                */
    const double  *pt_X;                /* [.][3] MapPoint::point3D                              */
    const uint8_t *pdesc_m;             /* [.][desc_bytes] med_desc                              */
    const double  *ls_X;                /* [.][6] MapLine::line3D: start, then end               */
    const uint8_t *ldesc_m;
    const double  *pt_pl;               /* [.][2]                                                */
    const double  *pt_P;                /* [.][3]                                                */
    const uint8_t *pdesc_f;
    const double  *ls_spl, *ls_epl;     /* [.][2]                                                */
    const double  *ls_le;               /* [.][3]                                                */
    const double  *ls_sP, *ls_eP;       /* [.][3]                                                */
    const uint8_t *ldesc_f;
} plba_mapassoc_batch;
/* Indexed by candidate row, not compacted. The five per-problem arrays are required; any other array
 * may be NULL and is then skipped. n_matches is the reference's return value, counted after the epipolar
 * test; n_accepted counts the accepted flags and so equals it (the matcher's own count is the number of
 * rows with m12 >= 0). */
typedef struct plba_mapassoc_out {
    int32_t *n_visible, *n_grid, *n_matches, *fallback, *n_accepted; /* [2n]: 2 f points, 2 f + 1 lines */
    uint8_t *pt_visible;                /* [pt_off_m[n]]                                         */
    int32_t *pt_m12;                    /* [.] the feature row, local to the keyframe, or -1     */
    uint8_t *pt_accepted;               /* [.]                                                   */
    double  *pt_rec;                    /* [.][6] u, v, err, dir                                 */
    uint8_t *ls_visible;                /* [ls_off_m[n]]                                         */
    int32_t *ls_m12;
    uint8_t *ls_accepted;
    double  *ls_rec;                    /* [.][9] su, sv, eu, ev, err0, err1, mid                */
} plba_mapassoc_out;
/* src/slamConfig.cpp and src2/config.cpp as plba_kfassoc_default_params takes them; width, height and the
 * camera are zero and must be set. */
void plba_mapassoc_default_params(plba_mapassoc_params *p);
/* Runs on the context's stream in a fixed number of launches (the cells, the matcher's three, the
 * fallback's bound, the brute-force matcher's two, which return at once where a problem does not fall
 * back, and the geometry) with one upload and one read-back; needs no uploaded window and leaves one
 * intact; shares plba_desc_match's device block and pinned host image. PLBA_E_INVALID, checked on the host
 * before anything is launched, for a NULL batch, params, out, per-problem output or offset array, a NULL
 * input array where rows exist, n < 0, decreasing or negative offsets, a bad desc_bytes, cols, rows, width
 * or height <= 0, ws < 0 or ws >= 2^30, more than 65535 feature rows or more than 65535 * 256 candidate
 * rows in a problem, a Twf or T_kf_w that is not finite, or a feature coordinate (pt_pl, ls_spl, ls_epl)
 * that is not finite or outside the bound above. A landmark that is not finite is invisible, not refused.
 * n == 0 does nothing and returns PLBA_OK. */
int plba_map_associate(plba_ctx *ctx, const plba_mapassoc_batch *b, const plba_mapassoc_params *p,
                       const plba_mapassoc_out *out);

/* ---- Place recognition, the step of loopClosure() that decides whether to look for a loop at all:
 *   DBoW2 TemplatedVocabulary<FORB>::transform(features, v)   (TemplatedVocabulary.h:1046-1084, :1198-1239)
 *   BowVector::addWeight / normalize(L1)                       (BowVector.cpp:34-84)
 *   L1Scoring::score(v1, v2)                                   (ScoringObject.cpp:23-68)
 * as insertKFBowVectorP / L / PL call them for every keyframe (src/mapHandler.cpp:4118-4239) on
 * dbow_voc_p and dbow_voc_l. Only TF-IDF weighting with L1 scoring is supported: the only combination
 * the reference's vocabularies use. A slot (0 points, 1 lines) holds one vocabulary and one database
 * of BoW vectors, both resident on the device; the slots are independent.
 * The vocabulary is a flat tree. Node 0 is the root; its descriptor and weight are not read. The
 * children of node i are children[child_off[i] .. child_off[i+1]), in the order of the vocabulary
 * file (TemplatedVocabulary.h:1458-1471). A node without children is a leaf (a word).
 * Arithmetic, equal to the reference's bit for bit:
 * Descent: from the root, the child with the smallest Hamming distance over desc_bytes
 * (FORB.cpp:78-100); a child replaces the best only if strictly nearer, so the first child wins a
 * tie; until a node has no children. Leaves may sit at different depths.
 * Accumulation: a descriptor whose leaf weight is not > 0 is dropped; otherwise v[word] += weight,
 * once per descriptor: the repeated sum, not count * weight.
 * Normalisation: norm = sum |v_i| added in increasing word id; if norm > 0 every value is divided by
 * it (a division, not a product with the reciprocal).
 * Score: over the words common to both vectors in increasing word id, s += |a - b| - |a| - |b| with a
 * of the first argument (the new vector); the score is -s / 2.0, which is -0.0 with no common word. */
typedef struct plba_bow_vocab {
    int32_t n_nodes;                    /* nodes, the root included: >= 2                        */
    int32_t n_words;                    /* words: word ids are 0 .. n_words-1                    */
    int32_t desc_bytes;                 /* as in plba_match_batch                                */
    int32_t pad;
    const int32_t *child_off;           /* [n_nodes+1]                                           */
    const int32_t *children;            /* [child_off[n_nodes]] node indices in 1 .. n_nodes-1   */
    const uint8_t *node_desc;           /* [n_nodes][desc_bytes]                                 */
    const int32_t *word_id;             /* [n_nodes] the word of a leaf, -1 on inner nodes       */
    const double  *weight;              /* [n_nodes] the idf of a leaf (Node::weight)            */
} plba_bow_vocab;
/* Uploads the vocabulary of a slot, once; it stays resident. Clears the slot's database.
 * PLBA_E_INVALID, with the slot left as it was, for a slot outside {0, 1}, a NULL array, n_nodes < 2,
 * a root without children, offsets that do not start at 0 or decrease, a child index out of range or
 * not greater than 0, a node reached twice (which covers cycles) or never, a leaf without a word_id in
 * [0, n_words) or with one that another leaf has, an inner node with a word_id >= 0, a weight that is
 * not finite, or a bad desc_bytes. The validated depth bounds the descent loop on the device. */
int plba_bow_set_vocab(plba_ctx *ctx, int32_t slot, const plba_bow_vocab *v);
/* Transforms desc [n_desc][desc_bytes] into a BoW vector, stores it under kf_id, and scores it against
 * every live stored vector of the slot and, last, against itself: *n = live vectors + 1 entries,
 * ids[j] in increasing kf_id (the last is kf_id itself), scores[j] = score(new, ids[j]). At most cap
 * entries are written; the vector is stored whatever cap is. A fixed number of launches (three), one
 * upload and one read-back; runs on the context's stream, needs no uploaded window and leaves one
 * intact. PLBA_E_INVALID, with nothing stored, for a bad slot, no vocabulary in the slot, kf_id < 0 or
 * already used in the slot (a removed vector keeps its id), n_desc < 0 or above 65535, desc == NULL
 * with n_desc > 0, scores or ids == NULL with cap > 0, cap < 0 or n == NULL. */
int plba_bow_insert(plba_ctx *ctx, int32_t slot, int32_t kf_id, const uint8_t *desc, int32_t n_desc,
                    double *scores, int32_t *ids, int32_t cap, int32_t *n);
/* Marks the vector of kf_id dead (the reference skips map_keyframes[i] == NULL): it is never scored
 * again. PLBA_E_INVALID if the slot has no live vector of that id. */
int plba_bow_remove(plba_ctx *ctx, int32_t slot, int32_t kf_id);
/* Reads the live vector of kf_id back (KeyFrame::descDBoW_P / _L): *n = its length, word_ids and
 * values in increasing word id, at most cap entries written (both may be NULL with cap == 0). */
int plba_bow_get(plba_ctx *ctx, int32_t slot, int32_t kf_id, int32_t *word_ids, double *values, int32_t cap,
                 int32_t *n);

/* ---- Sharded windows: one context per GPU, one window split over nranks.
 * Landmarks (with all their edges) are partitioned by the keyframe range of their first
 * observation (kf_obs_list[0], the base KF of map_points_kf_idx); poses are replicated.
 * Per LM trial each rank assembles its partial reduced camera system and the ranks exchange it
 * with one all-gather of each rank's block-row runs, summed in rank order (PLBA_SHARD_XCHG=allreduce:
 * one all-reduce of the whole system), plus a 13·nf-double all-reduce per outer iteration and a
 * 3-double one per trial (trial χ², scale, failed solves); every rank then factorises the identical
 * system redundantly, so accept/reject
 * decisions agree bit for bit across ranks. plba_download / plba_get_edge_chi2 /
 * plba_lba_plucker return the FULL window on every rank (one final gather all-reduce).
 * Call exactly one plba_comm_init_* before plba_upload; every rank uploads the same full
 * graph and then makes the same sequence of calls. */

/* In-place sum over ranks of n doubles in host memory (caller's transport, e.g. gloo). */
typedef int (*plba_host_allreduce_fn)(void *user, double *buf, int64_t n);

/* Landmark -> rank assignment used by sharded uploads (pure host code, no device needed). */
int plba_shard_plan(const plba_graph *g, int32_t nranks, int32_t *pt_owner, int32_t *ln_owner);
/* RCCL transport over xGMI: rank 0 creates the id, the caller broadcasts its 128 bytes. */
int plba_comm_unique_id(uint8_t id[128]);
int plba_comm_init_rccl(plba_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t id[128]);
/* Host transport (tests / hosts without RCCL): device buffers are staged through pinned memory. */
int plba_comm_init_host(plba_ctx *ctx, int32_t nranks, int32_t rank, plba_host_allreduce_fn fn, void *user);
/* What the transport itself reports, so that a multi-GPU record proves N ranks on N distinct GPUs:
 * out[0] transport (0 none, 1 RCCL, 2 host), [1] ranks (RCCL: ncclCommCount), [2] this rank
 * (RCCL: ncclCommUserRank), [3] the communicator's device (RCCL: ncclCommCuDevice; else the
 * context's), [4] the HIP device ordinal the context runs on (hipGetDevice), [5] its PCI domain,
 * [6] PCI bus, [7] PCI device. Entries past cap are not written. */
int plba_comm_info(plba_ctx *ctx, int32_t *out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PLBA_H */
