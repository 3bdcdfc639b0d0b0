/*
 * plslam_host.h — C ABI of the host-side mirror of the reference's map objects and of
 *   void PLSLAM::MapHandler::localBundleAdjustmentForPlukerWithG2O()
 *   (reference: include/mapHandler.h:134, src/mapHandler.cpp:5851-6323)
 *
 * The C++ classes behind it (pl-slam-plucker_amd/host/plslam_map.hpp) restate the state the
 * reference LBA reads and mutates — KeyFrame (include/keyFrame.h:50-71), MapPoint / MapLine
 * (include/mapFeatures.h:39-107), MapHandler::{map_keyframes, map_points, map_lines,
 * map_points_kf_idx, full_graph} (include/mapHandler.h:141-151) — and run the reference's
 * host logic around the solve: window gather (A1, src/mapHandler.cpp:5868-5921), graph
 * marshalling (A1b, :5923-6117), post-solve outlier bookkeeping (A1d, :6154-6293) and
 * write-back (A1e, :6296-6319). The solve itself (A1c) goes through plba.h on the GPU.
 *
 * These entry points exist for bindings and tests; a C++ caller (the reference's own
 * MapHandler) uses the classes directly — see INTEGRATION.md.
 *
 * Status codes are plba.h's (PLBA_OK / PLBA_E_*); nothing throws or exits.
 */
#ifndef PLSLAM_HOST_H
#define PLSLAM_HOST_H

#include <stdint.h>

#include "plba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plslam_map plslam_map;

/* Solver hook: solves one marshalled window (plba_graph) into plba_result.
 * NULL (the default) = the MI355X backend of plba.h (one plba context per map, reused across
 * LBA calls). Tests install a stub here to drive the host bookkeeping without a GPU. */
typedef int (*plslam_solve_fn)(void *user, const plba_graph *g, plba_result *r);

/* Statistics of one LBA call (the counters the reference prints, src/mapHandler.cpp:6147,6216,6290). */
typedef struct plslam_lba_stats {
    int32_t n_free_kf, n_fixed_kf;         /* idx_nofix_kfs / idx_fix_kfs sizes                      */
    int32_t n_pt, n_ln, n_ept, n_eln;      /* local landmarks and edges in the window                */
    int32_t bad_line_stage1;               /* "Bad Obs" after optimize(5) (:6147)                     */
    int32_t bad_point_obs, actually_bad_point_obs;   /* (:6216)                                     */
    int32_t bad_line_obs, actually_bad_line_obs;     /* (:6290)                                     */
    int32_t iters[2];
    double  chi2[2];
    double  gather_ms, solve_ms, bookkeeping_ms;
    double  upload_ms;                     /* plba_upload, part of solve_ms (0 with a solver hook)   */
    int32_t dirty_landmarks;               /* landmarks the incremental gather re-read from the map  */
} plslam_lba_stats;

int         plslam_map_create(plslam_map **m, double fx, double fy, double cx, double cy, const plba_opts *opts);
int         plslam_map_destroy(plslam_map *m);
const char *plslam_map_last_error(plslam_map *m);
int         plslam_set_solver(plslam_map *m, plslam_solve_fn fn, void *user);

/* KeyFrame(sf, kf_idx) placed at map_keyframes[kf_idx]; T_kf_w is row-major 4x4 (camera->world).
 * pt_idx / ls_idx are the idx fields of the KF's stereo_frame->stereo_pt / stereo_ls features. */
int plslam_add_keyframe(plslam_map *m, int32_t kf_idx, const double T_kf_w[16], int32_t n_pt_feat,
                        const int32_t *pt_idx, int32_t n_ls_feat, const int32_t *ls_idx);
/* MapPoint(idx, point3D, desc, kf_obs, obs, dir, sigma2) at map_points[idx] (src/mapFeatures.cpp:38-50). */
int plslam_add_point(plslam_map *m, int32_t idx, const double xyz[3], const uint8_t *desc, int32_t desc_bytes,
                     int32_t kf, const double obs[2], const double dir[3], double sigma2);
/* MapPoint::addMapPointObservation (src/mapFeatures.cpp:52-60). */
int plslam_point_add_observation(plslam_map *m, int32_t idx, const uint8_t *desc, int32_t kf, const double obs[2],
                                 const double dir[3], double sigma2);
/* Plücker MapLine(idx, NDw, desc, kf_obs, obs, sigma2) at map_lines[idx] (src/mapFeatures.cpp:114-122). */
int plslam_add_line(plslam_map *m, int32_t idx, const double NDw[6], const uint8_t *desc, int32_t desc_bytes,
                    int32_t kf, const double obs[4], double sigma2);
/* MapLine::addMapLineObservation(desc, kf_obs, obs4, sigma2) (src/mapFeatures.cpp:132-138). */
int plslam_line_add_observation(plslam_map *m, int32_t idx, const uint8_t *desc, int32_t kf, const double obs[4],
                                double sigma2);
/* the `local` flag of a keyframe (kind 0), point (1) or line (2). */
int plslam_set_local(plslam_map *m, int32_t kind, int32_t idx, int32_t local);
/* the `inlier` flag of a point (kind 1) or line (2). */
int plslam_set_inlier(plslam_map *m, int32_t kind, int32_t idx, int32_t inlier);
/* full_graph (n x n, row-major); map_points_kf_idx[kf] = lm[0..n) (creates the key, even empty) */
int plslam_set_full_graph(plslam_map *m, int32_t n, const uint32_t *g);
int plslam_get_full_graph(plslam_map *m, int32_t n, uint32_t *g);
int plslam_kf_idx_set(plslam_map *m, int32_t kf, const int32_t *lm, int32_t n);
int plslam_kf_idx_get(plslam_map *m, int32_t kf, int32_t *out, int32_t cap, int32_t *n);

/* MapHandler::localBundleAdjustmentForPlukerWithG2O() */
int plslam_local_ba_plucker_g2o(plslam_map *m, plslam_lba_stats *stats);

/* Incremental window (default on): the handler keeps every landmark's observations flattened and
 * the local landmarks in a registry, so the LBA gather and formLocalMap cost O(window + changes)
 * instead of scanning the map (the reference's :5877-5886, :1076-1091). Landmarks placed and
 * changed through this ABI are tracked; a caller that writes a landmark's observations or position
 * behind the handler's back reports it with plslam_mark_landmark_changed. on = 0: the scan gather.
 * plslam_check_incremental_gather compares the landmark pass of both gathers (tests). */
int plslam_set_incremental(plslam_map *m, int32_t on);
int plslam_mark_landmark_changed(plslam_map *m, int32_t kind, int32_t idx);
int plslam_check_incremental_gather(plslam_map *m, int32_t *equal);

/* ---- MapHandler::localBundleAdjustmentForPluker() (src/mapHandler.cpp:1505-1615), the hand-rolled
 * LM of levMarquardtOptimizationLBAForPluker (:1618-2332) on the GPU (plba_hlm_lba), and its
 * write-back (:2160-2330: T_kf_w = expmap_se3(X_i); point3D = X with inlier = false when it moved
 * more than 0.01; NDw = changeOrthToPluker(X − orthNDw) — the reference converts the difference).
 * x_kf_w: KeyFrame::x_kf_w; plslam_add_keyframe initialises it to logmap_se3(T_kf_w). */
int plslam_set_keyframe_x(plslam_map *m, int32_t kf_idx, const double x[6]);
int plslam_get_keyframe_x(plslam_map *m, int32_t kf_idx, double x[6]);
typedef int (*plslam_hlm_solve_fn)(void *user, const plba_graph *g, const plba_hlm_state *st,
                                   const plba_hlm_params *p, plba_hlm_result *r);
int plslam_set_hlm_solver(plslam_map *m, plslam_hlm_solve_fn fn, void *user);   /* NULL = plba_hlm_lba */
/* SlamConfig / Config values (NULL = plba_hlm_default_params) and vo_status == VO_INSERTING_KF */
int plslam_set_hlm_params(plslam_map *m, const plba_hlm_params *p, int32_t vo_inserting_kf);
typedef struct plslam_hlm_stats {
    int32_t ret;                            /* the reference's return value: 0 or -1                */
    int32_t n_kf_list, n_fixed_kf, n_pt, n_ln, n_pt_obs, n_ls_obs;
    int32_t linearizations, solves, accepted;
    int32_t pt_outliers, ln_outliers;       /* inlier = false set by the write-back                 */
    double  err, lambda, gather_ms, solve_ms, writeback_ms;
} plslam_hlm_stats;
int plslam_local_ba_plucker(plslam_map *m, plslam_hlm_stats *stats);
/* ---- MapHandler::localBundleAdjustment() (src/mapHandler.cpp:1392-1502), the local BA of a build
 * without USE_LINE_PLUKER: levMarquardtOptimizationLBA (:2334-3016) on the GPU (plba_hlm_lba,
 * variant PLBA_HLM_LBA_ENDPOINTS whatever plslam_set_hlm_params set) through the same solver hook,
 * and its write-back (:2841-2882: T_kf_w = expmap_se3(X_i); point3D / line3D = X with inlier = false
 * when the landmark moved more than 0.01; nothing when vo_status == VO_INSERTING_KF). Lines are
 * their endpoints line3D (plslam_set_line_geometry) and each line observation is the image line
 * equation (a, b, c) in obs[0..2] of plslam_add_line / plslam_line_add_observation. stats->ret is
 * the reference's return value: -1 with no observation or while VO inserts a KF, else 0. The
 * observation-removal loop of :2884-3006 acts on a flag that nothing in :2334-2840 sets: no-op. */
int plslam_local_ba(plslam_map *m, plslam_hlm_stats *stats);

/* ---- the rest of the Plücker local-mapping step around the LBA ---- */
/* SlamConfig::minLMObs / minLMCovGraph / minKFLocalMap (src/slamConfig.cpp:48,61-62; defaults
 * 5 / 75 / 3) and MapHandler::max_kf_idx (include/mapHandler.h, src/mapHandler.cpp:135,173). */
int plslam_set_params(plslam_map *m, int32_t min_lm_obs, int32_t min_lm_cov_graph, int32_t min_kf_local_map);
int plslam_set_max_kf_idx(plslam_map *m, int32_t max_kf_idx);
/* map_lines_kf_idx[kf] (include/mapHandler.h:149) */
int plslam_kf_lines_idx_set(plslam_map *m, int32_t kf, const int32_t *lm, int32_t n);
int plslam_kf_lines_idx_get(plslam_map *m, int32_t kf, int32_t *out, int32_t cap, int32_t *n);
/* MapHandler::formLocalMap(KeyFrame*) (src/mapHandler.cpp:1073-1137) */
int plslam_form_local_map(plslam_map *m, int32_t kf_idx);
/* MapHandler::removeBadMapLandmarksForPluker() (src/mapHandler.cpp:3816-3897); counts may be NULL */
int plslam_remove_bad_landmarks_pluker(plslam_map *m, int32_t *n_pt_removed, int32_t *n_ln_removed);
/* localMappingThread's USE_LINE_PLUKER body (src/mapHandler.cpp:1274-1279) after
 * lookForCommonMatches (front-end matching, the caller's): formLocalMap(kf) -> LBA -> culling */
int plslam_local_mapping_step(plslam_map *m, int32_t kf_idx, plslam_lba_stats *stats, int32_t *n_pt_removed,
                              int32_t *n_ln_removed);
/* 1 if map_points[idx] (kind 1) / map_lines[idx] (kind 2) / map_keyframes[idx] (kind 0) is
 * non-NULL, else 0 */
int plslam_exists(plslam_map *m, int32_t kind, int32_t idx, int32_t *exists);

/* State readers (any pointer may be NULL). n_obs receives the observation count; the list
 * outputs are written up to `cap` entries. */
int plslam_get_keyframe(plslam_map *m, int32_t kf_idx, double T_kf_w[16], int32_t *local, int32_t *pt_idx,
                        int32_t pt_cap, int32_t *ls_idx, int32_t ls_cap);
int plslam_get_point(plslam_map *m, int32_t idx, double xyz[3], int32_t *inlier, int32_t *local, int32_t *n_obs,
                     int32_t *kf_obs, double *obs, double *dir, double *sigma, int32_t cap, uint8_t *med_desc,
                     double med_dir[3]);
int plslam_get_line(plslam_map *m, int32_t idx, double NDw[6], int32_t *inlier, int32_t *local, int32_t *n_obs,
                    int32_t *kf_obs, double *obs, double *sigma, int32_t cap, uint8_t *med_desc);

/* ---- loop-closure pose graph ----
 * MapHandler::loopClosureOptimizationEssGraphG2O (src/mapHandler.cpp:5070-5299, ess = 1) and
 * ::loopClosureOptimizationCovGraphG2O (:5301-5531, ess = 0): the g2o VertexSE3 / EdgeSE3 graph of
 * the loop's KFs solved by plba_pgo_optimize (or the hook), then T_kf_w / x_kf_w of those KFs,
 * their landmarks (point3D, med_obs_dir, dir_list; line3D, med_obs_dir, dir_list) and every
 * later KF corrected, lc_idx_list[.][2] = 0, lc_state = LC_IDLE. This entry point leaves out
 * loopClosureFuseLandmarks() (:5294, :5526); plslam_loop_closure_optimization_fuse below runs it
 * too. lc_idxs / lc_idx_list: [n][3] int, lc_pose_list:
 * [n][6] ([t; ω], include/mapHandler.h:186-187). The lists are filled by plslam_loop_closure_step
 * below (the relative pose of each accepted loop comes from plba_lc_relative_pose);
 * plslam_set_loop_closure sets them directly, for a caller that keeps its own verification. */
int plslam_set_loop_closure(plslam_map *m, int32_t n_lc_idxs, const int32_t *lc_idxs, int32_t n_lc_idx_list,
                            const int32_t *lc_idx_list, int32_t n_lc_pose_list, const double *lc_pose_list);
int plslam_get_lc_idx_list(plslam_map *m, int32_t *out, int32_t cap, int32_t *n);
/* SlamConfig::minLMEssGraph (150) and maxItersPGO (100) (src/slamConfig.cpp:60,79) */
int plslam_set_pgo_params(plslam_map *m, int32_t min_lm_ess_graph, int32_t max_iters_pgo);
typedef int (*plslam_pgo_solve_fn)(void *user, const plba_pgo_graph *g, const plba_pgo_params *p,
                                   plba_pgo_result *r);
int plslam_set_pgo_solver(plslam_map *m, plslam_pgo_solve_fn fn, void *user);  /* NULL = plba_pgo_optimize */
typedef struct plslam_pgo_stats {
    int32_t kf_prev_idx, kf_curr_idx, n_vertices, n_fixed, n_edges, n_loop_edges, iterations, trials;
    double  chi2_initial, chi2_final, solve_ms;
} plslam_pgo_stats;
int plslam_loop_closure_optimization(plslam_map *m, int32_t ess, plslam_pgo_stats *stats);
/* ---- MapHandler::loopClosureFuseLandmarks() (src/mapHandler.cpp:5533-5808): for every loop whose
 * lc_idx_list flag is 1, the rows (lm_idx0, lm_ldx0, lm_idx1, lm_ldx1) of lc_pt_idxs and then of
 * lc_ls_idxs (plslam_get_lc_feature_idxs), in order. Per row one of four cases: the observation of the
 * previous keyframe's feature added to landmark lm_idx1 (case 0, :5552), that of the current
 * keyframe's feature added to lm_idx0 (case 1, :5567), a new landmark from both features (case 2, :5585),
 * or lm_idx1's lists appended to lm_idx0 and lm_idx1 erased (case 3, :5612), with the reference's
 * full_graph increments (case 0 names kf_curr_idx although the observation comes from kf_prev_idx,
 * :5562; case 1 the other way round, :5579), the erase from map_points_kf_idx / map_lines_kf_idx of
 * the erased landmark's first observer, the feature idx rewrites and the new index
 * max_pt_idx / max_ls_idx (the size of the map, as in plslam_match_kf_to_kf). The changed landmarks are
 * registered with the incremental window. The reference recomputes med_desc (and a point's
 * med_obs_dir) after every appended observation; only the last recomputation of a landmark can be
 * observed, so they are computed once per changed landmark when the rows are done: one
 * plba_desc_medoid batch on the map's context (or the hook below), and the mean direction on the host.
 * The keyframes need plslam_set_keyframe_features, for lines plslam_set_keyframe_line_endpoints too.
 * Defined where the reference is not (pl-slam-plucker_amd/host/fuse_landmarks.cpp lists every case):
 * a row with lm_idx0 == lm_idx1 != -1 is left untouched and counted; a feature index past a
 * keyframe's arrays (for a new line also lm_ldx1 past the previous keyframe's lines, which :5747
 * reads), a landmark index outside the map or an observer outside full_graph returns PLBA_E_INVALID
 * with the map unchanged; a feature cannot be NULL here, a landmark can (erased by an earlier row, or
 * culled): the row is skipped and counted; sigma_list is fused with the other lists. Lines: the
 * reference uses the endpoint constructor and observation in a Plücker build too, which leave NDw,
 * orthNDw and NDw_obs_list unset. Here the observation list of a line (NDw_obs_list, parallel to
 * kf_obs_list) takes pts = (spl, epl), the image endpoints, with sigma2 = 1; a new line stores
 * line3D = (sP, eP) in the world, med_obs_dir, and NDw = (sP x eP, eP - sP); le is not stored. */
typedef struct plslam_fuse_stats {
    int32_t loops, loops_skipped;           /* loops with flag 1 / with another flag                   */
    int32_t rows[2][4];                     /* [points, lines][case]: rows that passed their guard     */
    int32_t null_skipped[2][4];             /* rows whose landmark was NULL                            */
    int32_t same_landmark[2];               /* rows with lm_idx0 == lm_idx1 != -1                      */
    int32_t erased[2];                      /* landmarks deleted by case 3                             */
    int32_t medoid_lists, pad;              /* lists of the medoid batch                               */
    double  medoid_ms, total_ms;
} plslam_fuse_stats;
int plslam_fuse_landmarks(plslam_map *m, plslam_fuse_stats *stats);
/* Medoid hook, in the style of plslam_set_match_fn: NULL = plba_desc_medoid. */
typedef int (*plslam_medoid_fn)(void *user, const plba_medoid_batch *b, int32_t *medoid);
int plslam_set_medoid_fn(plslam_map *m, plslam_medoid_fn fn, void *user);
/* tools/fuse_bench.py and the tests only, not a product path: a single-threaded restatement of
 * plba_desc_medoid's semantics on the CPU (the table and a sort of every row, as the reference), with
 * the signature of the medoid hook. */
int plslam_desc_medoid_cpu(void *user, const plba_medoid_batch *b, int32_t *medoid);
/* plslam_loop_closure_optimization with the fuse: the pose graph and the map correction, then
 * plslam_fuse_landmarks, then the flags cleared and lc_state = LC_IDLE. The reference clears the
 * flags (:5290-5292, :5522-5523) before it calls loopClosureFuseLandmarks (:5294, :5526), whose
 * test for flag 1 then fails for every loop: as written it fuses nothing. Here the fuse runs while the
 * flags still name the loops that were just optimised. If the fuse is refused, the error is returned
 * with the map corrected, not fused, the flags set and lc_state unchanged. */
int plslam_loop_closure_optimization_fuse(plslam_map *m, int32_t ess, plslam_pgo_stats *pgo_stats,
                                          plslam_fuse_stats *fuse_stats);
/* ---- MapHandler::loopClosure() (src/mapHandler.cpp:4053-4116) after lookForLoopCandidates (which
 * plslam_loop_closure_kf below runs first; these entry points take its candidate from the caller):
 * the descriptor matching of isLoopClosure (:4327-4380, through
 * plba_desc_match or the hook, in plslam_loop_closure_step_kf below; plslam_loop_closure_step takes
 * the matched candidate from a caller that keeps its own matcher), the
 * inlier-ratio gate (:4384-4409; a zero feature count makes the ratio NaN or 0, so false),
 * computeRelativePoseRobustGN (:4677-5068) through plba_lc_relative_pose or the hook, and the state
 * machine. An accepted loop extends lc_poses, lc_pose_list (pose_inc), lc_idxs, lc_idx_list
 * ((kf_prev_idx, kf_curr_idx, 1)) and lc_pt_idxs / lc_ls_idxs (the index rows of the inliers, which
 * the landmark fusion needs) and turns LC_IDLE into LC_ACTIVE; anything else turns LC_ACTIVE into
 * LC_READY. On LC_READY loopClosureOptimizationCovGraphG2O runs (as plslam_loop_closure_optimization
 * with ess = 0) and the state returns to LC_IDLE (:4109-4115). */
typedef struct plslam_lc_candidate {
    int32_t kf_prev_idx, kf_curr_idx;
    int32_t n_pt_0, n_pt_1, n_ls_0, n_ls_1; /* stereo_pt / stereo_ls sizes of kf0 and kf1 (:4313-4316) */
    int32_t has_points, has_lines;          /* SlamConfig::hasPoints() / hasLines()                    */
    int32_t n_pt, n_ln;                     /* matches; then as in plba_lcpose_batch for one candidate */
    const double *pt_P, *pt_obs, *ln_sP, *ln_eP, *ln_le;
    const int32_t *pt_idx, *ls_idx;         /* [n][4] lc_pt_idx / lc_ls_idx rows (:4346-4351); may be NULL */
} plslam_lc_candidate;
typedef struct plslam_lc_stats {
    int32_t is_candidate, ratio_ok;         /* a candidate was given / it passed the inlier-ratio gate */
    int32_t accepted, conditions;           /* plba_lcpose_out of the candidate (0 when not solved)    */
    int32_t n_inl_pt, n_inl_ln;
    int32_t state_before, state_after;      /* lc_state: 0 LC_IDLE, 1 LC_ACTIVE, 2 LC_READY            */
    int32_t pgo_ran, pad;
    double  inl_ratio_pt, inl_ratio_ls, e, unc, t, r_deg, pose_ms;
    plslam_pgo_stats pgo;                   /* of the pose graph, when it ran                          */
} plslam_lc_stats;
typedef int (*plslam_lcpose_solve_fn)(void *user, const plba_lcpose_batch *b, const plba_lcpose_params *p,
                                      plba_lcpose_out *out, uint8_t *pt_inlier, uint8_t *ln_inlier);
int plslam_set_lcpose_solver(plslam_map *m, plslam_lcpose_solve_fn fn, void *user); /* NULL = plba_lc_relative_pose */
int plslam_set_lcpose_params(plslam_map *m, const plba_lcpose_params *p);           /* NULL = the defaults          */
/* c == NULL: lookForLoopCandidates found none. lc_inlier_ratio: SlamConfig::lcInlierRatio(), 30
 * (src/slamConfig.cpp:83). */
int plslam_loop_closure_step(plslam_map *m, const plslam_lc_candidate *c, double lc_inlier_ratio,
                             plslam_lc_stats *st);
/* ---- isLoopClosure from two keyframe indices (src/mapHandler.cpp:4303-4411).
 * What it reads of a keyframe's stereo_frame: pdesc_l / ldesc_l (one descriptor row per feature) and,
 * per point feature, P (3-D, camera frame) and pl (pixel); per line feature sP, eP (3-D endpoints) and
 * le (normalised image line). The counts are those given to plslam_add_keyframe; an array of a kind
 * with no feature may be NULL. desc_bytes as in plba_match_batch. */
int plslam_set_keyframe_features(plslam_map *m, int32_t kf_idx, int32_t desc_bytes, const uint8_t *pdesc,
                                 const double *pt_P, const double *pt_pl, const uint8_t *ldesc, const double *ls_sP,
                                 const double *ls_eP, const double *ls_le);
/* Matcher hook, in the style of plslam_set_lcpose_solver: NULL = plba_desc_match. */
typedef int (*plslam_match_fn)(void *user, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches);
int plslam_set_match_fn(plslam_map *m, plslam_match_fn fn, void *user);
typedef struct plslam_match_params {
    float   min_ratio_12_p, min_ratio_12_l; /* SlamConfig::minRatio12P() / minRatio12L(), 0.9 (src2/config.cpp:60,68) */
    int32_t best_lr;                        /* Config::bestLRMatches(), 1 (src2/config.cpp:51)         */
    int32_t has_points, has_lines;          /* SlamConfig::hasPoints() / hasLines(), 1                 */
    int32_t pad;
} plslam_match_params;
/* loopClosure() with isLoopClosure(kf_prev, kf_curr) whole: one match call with two pairs (points,
 * lines; a kind that is disabled or empty on either side, :4331 / :4357, is an empty pair), lc_points /
 * lc_lines / lc_pt_idx / lc_ls_idx built in i1 order (:4336-4379), then as plslam_loop_closure_step.
 * mp == NULL: the defaults. A bad keyframe index, or a keyframe whose features were not set, returns
 * PLBA_E_INVALID and leaves the map untouched. */
int plslam_loop_closure_step_kf(plslam_map *m, int32_t kf_prev_idx, int32_t kf_curr_idx, const plslam_match_params *mp,
                                double lc_inlier_ratio, plslam_lc_stats *st);
/* K candidates kf_prev_idx[0..n) for one new keyframe: one match call with 2n pairs, then one
 * plba_lc_relative_pose call with the candidates that pass the gate. accepted [n], pose_inc [n][6]
 * (zero where not accepted), n_matches [n][2] (points, lines); each may be NULL. No map state is
 * changed. A bad keyframe index returns PLBA_E_INVALID. */
int plslam_verify_loop_candidates(plslam_map *m, int32_t kf_curr_idx, int32_t n, const int32_t *kf_prev_idx,
                                  const plslam_match_params *mp, double lc_inlier_ratio, int32_t *accepted,
                                  double *pose_inc, int32_t *n_matches);
/* ---- place recognition: insertKFBowVectorP / L / PL (src/mapHandler.cpp:4118-4239), lookForLoopCandidates
 * (:4241-4301) and with them loopClosure() (:4053-4116) whole, from a keyframe's descriptors. The BoW
 * vectors (KeyFrame::descDBoW_P / _L) live in the place-recognition database of plba.h, slot 0 for
 * points and slot 1 for lines; the map keeps conf_matrix.
 * The hook, in the style of plslam_set_match_fn: every database operation goes through one call
 * record. NULL = the device path (plba_bow_set_vocab / _insert / _remove / _get). */
#define PLSLAM_BOW_SET_VOCAB 0          /* slot, vocab                                             */
#define PLSLAM_BOW_INSERT    1          /* slot, kf_id, desc, n_desc, scores, ids, cap -> n        */
#define PLSLAM_BOW_REMOVE    2          /* slot, kf_id                                             */
#define PLSLAM_BOW_GET       3          /* slot, kf_id, word_ids, values, cap -> n                 */
typedef struct plslam_bow_call {
    int32_t op, slot, kf_id, n_desc, cap;
    int32_t n;                          /* out, as *n of plba_bow_insert / plba_bow_get            */
    const plba_bow_vocab *vocab;
    const uint8_t *desc;
    double  *scores;
    int32_t *ids;
    int32_t *word_ids;
    double  *values;
} plslam_bow_call;
typedef int (*plslam_bow_fn)(void *user, plslam_bow_call *c);
int plslam_set_bow_fn(plslam_map *m, plslam_bow_fn fn, void *user);
/* The tests and tools/bow_bench.py only, not a product path: a single-threaded C++ restatement of
 * plba_bow_*'s semantics (sorted arrays, popcounts) with the hook's signature. user: a database made
 * by plslam_bow_cpu_new, which holds both slots. */
void *plslam_bow_cpu_new(void);
void  plslam_bow_cpu_free(void *db);
int   plslam_bow_cpu(void *user, plslam_bow_call *c);
/* dbow_voc_p (slot 0) / dbow_voc_l (slot 1): forwards to the hook or the device; clears the slot. */
int plslam_set_vocabulary(plslam_map *m, int32_t slot, const plba_bow_vocab *v);
/* map_keyframes[kf_idx] = NULL (a culled keyframe). Its BoW vectors leave the database at the next
 * plslam_insert_kf_bow; its row and column of conf_matrix stay as they are. */
int plslam_remove_keyframe(plslam_map *m, int32_t kf_idx);
/* insertKFBowVectorPL (both kinds), ...P or ...L (one kind); PLBA_E_INVALID with neither. Reads the
 * descriptors given by plslam_set_keyframe_features and, for PL, the point pixels pl and the line
 * midpoints (spl + epl) * 0.5 (plslam_set_keyframe_line_endpoints) for vector_stdv
 * (src2/auxiliar.cpp:504-513: mean and squared sum sequential, sqrt(1.0 / n * e)). The PL score is
 * :4226-4228 in that order in double, without contraction; n_pl == 0 or std_pl == 0 divides by zero as
 * the reference does and the NaN is stored. conf_matrix is vector<vector<float>>
 * (include/mapHandler.h:153): every score is rounded to float when stored, for row and column alike,
 * and the matrix grows with zeros to kf_idx + 1 (expandGraphs, :1000-1002). Keyframes that are NULL
 * are skipped. PLBA_E_INVALID, with the map and the database untouched, for a keyframe that does not
 * exist, has no features (or, for PL with line features, no endpoints), was inserted before, a slot
 * without vocabulary, or for PL when the two slots do not hold the same keyframes. */
int plslam_insert_kf_bow(plslam_map *m, int32_t kf_idx, int32_t has_points, int32_t has_lines);
/* conf_matrix: row kf_idx, *n = its length, at most cap floats written; the whole n x n matrix set */
int plslam_get_conf_matrix_row(plslam_map *m, int32_t kf_idx, float *out, int32_t cap, int32_t *n);
int plslam_set_conf_matrix(plslam_map *m, int32_t n, const float *c);
typedef struct plslam_lc_search_params {
    int32_t lc_kf_dist;                 /* SlamConfig::lcKFDist()      50 (src/slamConfig.cpp:80)  */
    int32_t lc_kf_max_dist;             /* SlamConfig::lcKFMaxDist()   50 (:81)                    */
    int32_t lc_nkf_closest;             /* SlamConfig::lcNKFClosest()   4 (:82)                    */
    int32_t min_lm_cov_graph;           /* SlamConfig::minLMCovGraph() 75 (:61)                    */
    int32_t min_kf_local_map;           /* SlamConfig::minKFLocalMap()  3 (:62)                    */
    int32_t pad;
} plslam_lc_search_params;
void plslam_lc_search_default_params(plslam_lc_search_params *p);
/* lookForLoopCandidates (:4241-4301): the live keyframes i < kf_curr_idx - lc_kf_dist with
 * conf_matrix[i][kf_curr_idx]; more than lc_kf_max_dist of them, else no candidate; sorted by score,
 * descending, ties by increasing index, NaN last (the reference's std::sort leaves ties open);
 * lc_min_score, from 1.0, the smallest score > 0.001 over the keyframes i < kf_curr_idx with
 * full_graph[i][kf_curr_idx] >= min_lm_cov_graph or kf_curr_idx - i <= min_kf_local_map + 3; the best
 * must be >= lc_min_score; then the ranks >= 1 with |idx - idx_max| <= lc_kf_max_dist and score >=
 * lc_min_score * 0.8 are counted, and lc_nkf_closest of them make idx_max the candidate.
 * *kf_prev_idx is -1 without one. p == NULL: the defaults. PLBA_E_INVALID for a negative parameter (the
 * reference compares a size_t with it), or a kf_curr_idx outside conf_matrix or full_graph. */
int plslam_look_for_loop_candidates(plslam_map *m, int32_t kf_curr_idx, const plslam_lc_search_params *p,
                                    int32_t *is_candidate, int32_t *kf_prev_idx);
/* loopClosure() whole: the search above, then plslam_loop_closure_step_kf with the candidate, or the
 * c == NULL branch of plslam_loop_closure_step without one. */
int plslam_loop_closure_kf(plslam_map *m, int32_t kf_curr_idx, const plslam_lc_search_params *sp,
                           const plslam_match_params *mp, double lc_inlier_ratio, plslam_lc_stats *st);
/* tools/descmatch_bench.py only, not a product path: a single-threaded popcount restatement of
 * plba_desc_match's semantics on the CPU, with the signature of the matcher hook. */
int plslam_desc_match_cpu(void *user, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches);
/* ---- around the grid-guided matcher (plba_grid_match; StVO::matchGrid, src2/matching.cpp:111-258).
 * getLineCoords / LineIterator (src2/gridStructure.cpp:33-41, src2/lineIterator.cpp): the cells under
 * which matchKF2KFLines / matchMap2KFLines (src/mapHandler.cpp:410-413, :860-863) enter a line from
 * (x1, y1) to (x2, y2), given in grid units (spl * inv_width, ...), in the reference's order: the
 * cells2 list of that train row. cells [cap][2] is written up to cap entries, *n is their number.
 * PLBA_E_INVALID for a coordinate that is not finite or beyond 1e6 cells in magnitude. */
int plslam_line_cells(double x1, double y1, double x2, double y2, int32_t *cells, int32_t cap, int32_t *n);
/* tools/gridmatch_bench.py and the tests only, not a product path: a single-threaded restatement of
 * plba_grid_match's semantics on the CPU, the query rows walked in order as the reference does. */
int plslam_grid_match_cpu(void *user, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches);
/* ---- MapHandler::matchMap2KFPoints + matchMap2KFLines (src/mapHandler.cpp:697-921), the map-to-keyframe
 * association that opens a local-mapping step (lookForCommonMatches, :923), for keyframe kf_idx.
 * It needs the keyframe's features (plslam_set_keyframe_features), the image endpoints spl / epl of its
 * line features ([n_ls][2], :857-861, :903) and the camera with the image size (cam->getWidth() /
 * getHeight(), :716); plslam_set_camera also replaces the intrinsics given to plslam_map_create. */
int plslam_set_keyframe_line_endpoints(plslam_map *m, int32_t kf_idx, const double *spl, const double *epl);
int plslam_set_camera(plslam_map *m, double fx, double fy, double cx, double cy, int32_t width, int32_t height);
/* Grid-matcher hook, in the style of plslam_set_match_fn: NULL = plba_grid_match. */
typedef int (*plslam_grid_match_fn)(void *user, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches);
int plslam_set_grid_match_fn(plslam_map *m, plslam_grid_match_fn fn, void *user);
typedef struct plslam_mapmatch_params {
    int32_t fast_matching;                  /* SlamConfig::fastMatching(): false in src/slamConfig.cpp:43, true in
                                               the shipped config/config/config.yaml:5; the default here is 1    */
    int32_t ws;                             /* Config::matchingF2FWs(), 3 (src2/config.cpp:92)                  */
    int32_t min_pt_matches, min_ls_matches; /* SlamConfig::minPointMatches() / minLineMatches(), 10 / 6 (:85-86) */
    int32_t best_lr;                        /* Config::bestLRMatches(), 1                                       */
    int32_t has_points, has_lines;          /* SlamConfig::hasPoints() / hasLines(), 1                          */
    int32_t pad;
    double  max_kf_epip_p, max_kf_epip_l;   /* SlamConfig::maxKFEpipP() / maxKFEpipL(), 1.0 (:51-52)            */
    double  line_sim_th;                    /* Config::lineSimTh(), 0.75 (src2/config.cpp:63)                   */
    double  min_ratio_12_p, min_ratio_12_l; /* Config::minRatio12P() / minRatio12L(), 0.9. matchGrid uses _p for
                                               lines too (matching.cpp:241); the fallback uses both, as floats  */
} plslam_mapmatch_params;
void plslam_mapmatch_default_params(plslam_mapmatch_params *p);
typedef struct plslam_mapmatch_stats {      /* [0] points, [1] lines */
    int32_t visible[2];                     /* local landmarks not yet seen by the keyframe, inside the image   */
    int32_t unmatched[2];                   /* features of the keyframe with idx -1                             */
    int32_t grid_matches[2];                /* what matchGrid returned                                          */
    int32_t fallback[2];                    /* 1 if match() ran for the kind (:759-764, :874-879)               */
    int32_t accepted[2], rejected[2];       /* by the epipolar test (:778, :894)                                */
    double  match_ms;                       /* the matcher calls                                                */
} plslam_mapmatch_stats;
/* The local-landmark scan (pt->local, kf_obs_list.back() != kf, :712 / :813), the projection by Twf
 * (row-major 4x4, world -> keyframe; NULL = the inverse of the keyframe's T_kf_w) with the strict
 * in-image test, the cells, the keyframe's features with idx -1 gridded or rasterised; ONE
 * plba_grid_match call with the point and the line problem; where a kind has more than min_*_matches
 * visible landmarks and fewer grid matches, one plba_desc_match call through plslam_set_match_fn's
 * hook (min_ratio_12_p / _l); then per match, in i1 order, points before lines: the epipolar test
 * (points: the pixel distance < max_kf_epip_p; lines: both signed distances of the projected endpoints
 * to the feature's line < max_kf_epip_l, signed as the reference has it), the feature's idx,
 * addMapPointObservation(desc, kf, pl, T_kf_w * normalized(P)) / addMapLineObservation(desc, kf,
 * (spl, epl)) with the default sigma2 = 1 (include/mapFeatures.h:51,81), and full_graph[kf][obs]++,
 * full_graph[obs][kf]++ for every earlier observer. The incremental window is told of each landmark.
 * Lines are projected from line3D, which a Plücker build never sets: the line half is meaningful for
 * endpoint-line maps or where the caller keeps line3D (plslam_set_line_geometry).
 * Where the reference's fallback keeps grid matches that match() does not overwrite (match() resizes
 * matches_12 without clearing it), the fallback's result stands alone here.
 * params == NULL: the defaults; stats may be NULL. A bad index, a keyframe without features (or without
 * line endpoints when it has line features), no image size, a keyframe outside full_graph or ws < 0
 * return PLBA_E_INVALID with the map untouched. */
int plslam_match_map_to_kf(plslam_map *m, int32_t kf_idx, const double *Twf, const plslam_mapmatch_params *params,
                           plslam_mapmatch_stats *stats);
/* lookForCommonMatches' map half, then formLocalMap -> LBA -> culling: plslam_match_map_to_kf(kf_idx,
 * NULL, params), then plslam_local_mapping_step. */
int plslam_local_mapping_step_kf(plslam_map *m, int32_t kf_idx, const plslam_mapmatch_params *params,
                                 plslam_mapmatch_stats *match_stats, plslam_lba_stats *stats, int32_t *n_pt_removed,
                                 int32_t *n_ln_removed);
/* The same association around ONE plba_map_associate call (or the hook): matchMap2KFPoints +
 * matchMap2KFLines with the projection, the in-image test, the cells, both matchers, the fallback's decision
 * and the epipolar tests on the device. The candidates (local, kf_obs_list.back() != kf_idx) and the
 * keyframe's features with idx -1 are gathered in the reference's order, the call is made, and the rows are
 * walked in i1 order, points before lines: the feature's idx, addMapPointObservation with the record's dir /
 * addMapLineObservation, full_graph. It fills the statistics of plslam_match_map_to_kf (fallback is 0 where a
 * kind has no unmatched feature, as there) and leaves the map as that call leaves it, up to the order of a
 * three-term sum in the stored direction. A kind takes part when the keyframe has features of it. Every
 * candidate's descriptor size and observers are checked, not only the visible ones'. params NULL = the
 * defaults; params->width == 0 and height == 0: the image size and the camera of plslam_set_camera; the grid
 * is params->cols x rows. plslam_match_map_to_kf stays the yardstick and is unchanged. */
int plslam_match_map_to_kf_assoc(plslam_map *m, int32_t kf_idx, const double *Twf, const plba_mapassoc_params *params,
                                 plslam_mapmatch_stats *stats);
/* plslam_match_map_to_kf_assoc(kf_idx, NULL, params), then plslam_local_mapping_step. */
int plslam_local_mapping_step_kf_assoc(plslam_map *m, int32_t kf_idx, const plba_mapassoc_params *params,
                                       plslam_mapmatch_stats *match_stats, plslam_lba_stats *stats, int32_t *n_pt_removed,
                                       int32_t *n_ln_removed);
/* Association hook, in the style of plslam_set_kfassoc_fn: NULL = plba_map_associate. */
typedef int (*plslam_mapassoc_fn)(void *user, const plba_mapassoc_batch *b, const plba_mapassoc_params *p,
                                  const plba_mapassoc_out *out);
int plslam_set_mapassoc_fn(plslam_map *m, plslam_mapassoc_fn fn, void *user);
/* tools/mapassoc_bench.py and the tests only, not a product path: a single-threaded restatement of
 * plba_map_associate's semantics on the CPU, which compacts the visible landmarks as the reference does. */
int plslam_map_assoc_cpu(void *user, const plba_mapassoc_batch *b, const plba_mapassoc_params *p, const plba_mapassoc_out *out);
/* ---- StereoFrame::matchStereoPoints + matchStereoLines (src2/stereoFrame.cpp:121-174, :310-435): the
 * features of keyframe kf_idx from the detector output of its two images, with no StVO on the caller's
 * side. One plba_stereo_associate call (or the hook) with the one frame; the survivors are stored as
 * plslam_set_keyframe_features + plslam_set_keyframe_line_endpoints would store them (pdesc, P, pl,
 * ldesc, sP, eP, le, spl, epl). plslam_add_keyframe fixes a kind's feature count when it is given that
 * kind's idx list: the count must then equal the survivors'. A keyframe added without the list (NULL
 * or n = 0) is sized here with every idx -1, the reference's frames after the first (:168, :411).
 * pt_src [n_pt_l] / ls_src [n_ls_l] (may be NULL) receive the left row of each stored feature, for the
 * octave and whatever else the caller keeps per detection; stats (may be NULL) the counts. params is
 * required (the baseline b and the image size are in it). Anything invalid returns PLBA_E_INVALID with
 * the keyframe untouched. */
typedef struct plslam_stereo_frame {
    int32_t desc_bytes;                     /* as in plba_match_batch                                           */
    int32_t n_pt_l, n_pt_r, n_ls_l, n_ls_r; /* detections of the left / right image                             */
    int32_t pad;
    const float   *pt_l, *pt_r;             /* [n][2] cv::KeyPoint::pt                                          */
    const uint8_t *pdesc_l, *pdesc_r;       /* [n][desc_bytes]                                                  */
    const float   *ls_l, *ls_r;             /* [n][4] KeyLine startPointX, startPointY, endPointX, endPointY    */
    const uint8_t *ldesc_l, *ldesc_r;       /* [n][desc_bytes]                                                  */
} plslam_stereo_frame;
typedef struct plslam_stereo_stats {
    int32_t n_pt, n_ls;                     /* stereo_pt.size(), stereo_ls.size()                               */
    double  ms;                             /* the association call                                             */
} plslam_stereo_stats;
int plslam_set_keyframe_stereo(plslam_map *m, int32_t kf_idx, const plslam_stereo_frame *frame,
                               const plba_stereo_params *params, int32_t *pt_src, int32_t *ls_src,
                               plslam_stereo_stats *stats);
/* Stereo hook, in the style of plslam_set_grid_match_fn: NULL = plba_stereo_associate. */
typedef int (*plslam_stereo_fn)(void *user, const plba_stereo_batch *b, const plba_stereo_params *p,
                                const plba_stereo_out *out);
int plslam_set_stereo_fn(plslam_map *m, plslam_stereo_fn fn, void *user);
/* tools/stereo_bench.py and the tests only, not a product path: a single-threaded restatement of
 * plba_stereo_associate's semantics on the CPU, with the hook's signature. */
int plslam_stereo_cpu(void *user, const plba_stereo_batch *b, const plba_stereo_params *p, const plba_stereo_out *out);
/* tools/trackpose_bench.py and the tests only, not a product path: a single-threaded restatement of
 * plba_track_pose's semantics (StereoFrameHandler::optimizePose) on the CPU, with that call's
 * signature behind a user pointer. H, g and e are summed in match order. */
int plslam_track_pose_cpu(void *user, const plba_track_batch *b, const plba_track_params *p, plba_track_out *out,
                          uint8_t *pt_inlier, uint8_t *ln_inlier);
/* tools/trackframes_bench.py and the tests only, not a product path: a single-threaded restatement of
 * plba_track_frames' semantics (f2fTracking + optimizePose) on the CPU, composed of plslam_desc_match_cpu,
 * the scatter loops of src2/stereoFrameHandler.cpp:144-152 / :167-179 and plslam_track_pose_cpu, with that
 * call's signature behind a user pointer. */
int plslam_track_frames_cpu(void *user, const plba_frames_batch *b, const plba_frames_params *p, const plba_frames_out *out);
/* ---- MapHandler::matchKF2KFPoints + matchKF2KFLines (src/mapHandler.cpp:237-366, :368-590, the
 * USE_LINE_PLUKER branch), the only place where map landmarks are created, between two keyframes that have
 * their features (plslam_set_keyframe_stereo with params.pluker, or plslam_set_keyframe_features +
 * plslam_set_keyframe_line_endpoints + plslam_set_keyframe_line_pluker). One plba_kf_associate call (or the
 * hook) with the one pair, then the rows of the previous keyframe in order as :283-363 and :434-589 walk them.
 * New landmark (the previous feature's idx is -1): its index is the size of the map's point / line list (the
 * reference's max_pt_idx / max_ls_idx always equal it); both features get it; the landmark is built from the
 * previous keyframe's observation, listed under that keyframe in map_points_kf_idx / map_lines_kf_idx, given
 * the current keyframe's observation (sigma2 1), and full_graph is bumped both ways. Existing landmark: a
 * deleted (NULL) one skips the row; otherwise the current feature takes the idx, the landmark the observation,
 * and full_graph is bumped against every earlier observer. Rejected line (|error2| > sqrt(5.991)): both idx
 * become -1 for a new landmark, the current one for an existing. Two previous rows matching one current row
 * (without best_lr) both go through, and the later one overwrites the idx, as in the reference.
 * DT: 4 x 4 row-major, NULL = expmap(logmap(inverse(T_curr) * T_prev)) (:143-145). params NULL = the defaults;
 * params->width == 0 and height == 0: the image size and the camera of plslam_set_camera. The pose refinement
 * of :937-977 (has_refinement, default false) is not part of it: the accepted pairs are returned for a caller
 * that runs its own. Anything invalid returns PLBA_E_INVALID before the map is touched. */
typedef struct plslam_kfmatch_stats {
    int32_t grid_matches[2], fallback[2], matches[2];   /* [points, lines]                                  */
    int32_t created[2], extended[2], rejected[2];
    int32_t n_pairs[2];                     /* accepted rows: created + extended                            */
    int32_t pt_cap, ls_cap;                 /* in: the pairs that pt_pairs / ls_pairs hold                  */
    int32_t *pt_pairs, *ls_pairs;           /* in: [cap][2] or NULL; out: the first min(n, cap) accepted
                                               (i1, i2) in row order (matched_pt / matched_ls)              */
    double  match_ms;
} plslam_kfmatch_stats;
int plslam_match_kf_to_kf(plslam_map *m, int32_t kf_prev_idx, int32_t kf_curr_idx, const double *DT,
                          const plba_kfassoc_params *params, plslam_kfmatch_stats *stats);
/* lookForCommonMatches (:923-990) without the refinement block: plslam_match_kf_to_kf with DT NULL, then
 * plslam_match_map_to_kf of the current keyframe with Twf NULL. */
int plslam_look_for_common_matches(plslam_map *m, int32_t kf_prev_idx, int32_t kf_curr_idx,
                                   const plba_kfassoc_params *kf_params, const plslam_mapmatch_params *map_params,
                                   plslam_kfmatch_stats *kf_stats, plslam_mapmatch_stats *map_stats);
/* NDc [n_ls][6] of keyframe kf_idx's line features, for callers on the plslam_set_keyframe_features route
 * (plslam_set_keyframe_stereo stores it with params.pluker). */
int plslam_set_keyframe_line_pluker(plslam_map *m, int32_t kf_idx, const double *NDc);
/* Association hook, in the style of plslam_set_stereo_fn: NULL = plba_kf_associate. */
typedef int (*plslam_kfassoc_fn)(void *user, const plba_kfassoc_batch *b, const plba_kfassoc_params *p,
                                 const plba_kfassoc_out *out);
int plslam_set_kfassoc_fn(plslam_map *m, plslam_kfassoc_fn fn, void *user);
/* tools/kfassoc_bench.py and the tests only, not a product path: a single-threaded restatement of
 * plba_kf_associate's semantics (matchKF2KFPoints / Lines up to the sequential part) on the CPU. */
int plslam_kf_assoc_cpu(void *user, const plba_kfassoc_batch *b, const plba_kfassoc_params *p, const plba_kfassoc_out *out);
int plslam_get_lc_state(plslam_map *m, int32_t *state);
/* lc_pose_list [n][6]; the kept index rows of loop `loop` (kind 1 points, 2 lines), [n][4] */
int plslam_get_lc_pose_list(plslam_map *m, double *out, int32_t cap, int32_t *n);
int plslam_get_lc_feature_idxs(plslam_map *m, int32_t kind, int32_t loop, int32_t *out, int32_t cap, int32_t *n);
/* Sets the index rows of loop `loop` (kind 1 points, 2 lines), rows [n][4], for a caller that keeps its
 * own verification, in the style of plslam_set_loop_closure; both lists grow to hold the loop. */
int plslam_set_lc_feature_idxs(plslam_map *m, int32_t kind, int32_t loop, const int32_t *rows, int32_t n);

/* MapLine::line3D / med_obs_dir (include/mapFeatures.h:93-94; never set in Plücker mode) */
int plslam_set_line_geometry(plslam_map *m, int32_t idx, const double line3D[6], const double med_obs_dir[3]);
int plslam_get_line_geometry(plslam_map *m, int32_t idx, double line3D[6], double med_obs_dir[3]);

/* MapLine::changePlukerToOrth / changeOrthToPluker (src/mapFeatures.cpp:186-221) */
void plslam_pluker_to_orth(const double NDw[6], double orth[4]);
void plslam_orth_to_pluker(const double orth[4], double NDw[6]);

#ifdef __cplusplus
}
#endif

#endif /* PLSLAM_HOST_H */
