// Host-side mirror of the map state the Plücker LBA reads and mutates, and of
// MapHandler::localBundleAdjustmentForPlukerWithG2O (src/mapHandler.cpp:5851-6323).
//
// The classes keep the reference's field names and list semantics (parallel per-observation
// vectors, pointer vectors indexed by id, std::map<int, vector<int>> map_points_kf_idx,
// vector<vector<unsigned>> full_graph) so the bookkeeping reads line-for-line against the
// reference; Eigen/OpenCV types become fixed-size arrays (Matrix4d -> row-major double[16],
// cv::Mat binary descriptor -> byte vector, NORM_HAMMING -> popcount).
#pragma once

#include <array>
#include <cstdint>
#include <map>
#include <memory>
#include <new>
#include <utility>
#include <string>
#include <vector>

#include "plba.h"

namespace plslam {

// Incremental window state of a MapHandler (map_handler.cpp): landmarks report changes to it.
struct LandmarkStore;
void landmark_changed(LandmarkStore *s, int kind, int idx);  // kind 1 = point, 2 = line

// The marshalled window's arrays: resize() default-initialises (no zero fill) — every element
// is written by the gather. (Page-locked memory for them was measured and did not shorten
// plba_upload: 0.97 vs 0.92-0.96 ms at C3.)
template <class T>
struct DefaultInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = DefaultInitAlloc<U>;
    };
    DefaultInitAlloc() = default;
    template <class U>
    DefaultInitAlloc(const DefaultInitAlloc<U> &) {}
    template <class U, class... Args>
    void construct(U *p, Args &&...args) {
        if constexpr (sizeof...(Args) == 0) ::new ((void *)p) U;
        else ::new ((void *)p) U(std::forward<Args>(args)...);
    }
};
template <class T>
using wvector = std::vector<T, DefaultInitAlloc<T>>;

using Vec2 = std::array<double, 2>;
using Vec3 = std::array<double, 3>;
using Vec4 = std::array<double, 4>;
using Vec6 = std::array<double, 6>;
using Mat4 = std::array<double, 16>;  // row-major
using Vec3i = std::array<int, 3>;
using Desc = std::vector<uint8_t>;

// StVO::StereoFrame, reduced to what the LBA touches: the idx of each point / line feature
// (src/mapHandler.cpp:6189-6198, 6262-6271).
struct StereoFrame {
    std::vector<int> stereo_pt_idx;
    std::vector<int> stereo_ls_idx;
    // what isLoopClosure reads (src/mapHandler.cpp:4334-4378): the descriptor matrices pdesc_l /
    // ldesc_l, one row of desc_bytes per feature, and per point feature P and pl, per line feature
    // sP, eP and le, as flat rows in feature order
    bool has_features = false;
    int desc_bytes = 32;
    std::vector<uint8_t> pdesc_l, ldesc_l;
    std::vector<double> pt_P, pt_pl;          // [n_pt][3], [n_pt][2]
    std::vector<double> ls_sP, ls_eP, ls_le;  // [n_ls][3]
    // what matchMap2KFLines reads besides (src/mapHandler.cpp:857-861, :903): the image endpoints
    bool has_endpoints = false;
    std::vector<double> ls_spl, ls_epl;       // [n_ls][2]
    // what matchKF2KFLines reads besides (src/mapHandler.cpp:451): the Plücker line in the camera frame
    bool has_pluker = false;
    std::vector<double> ls_NDc;               // [n_ls][6]
};

// include/keyFrame.h:50-71
struct KeyFrame {
    bool local = false;
    int kf_idx = -1;
    Mat4 T_kf_w{};  // camera -> world
    Vec6 x_kf_w{};  // logmap_se3 of T_kf_w at insertion (src/mapHandler.cpp:140,179); the g2o LBA
                    // writes T_kf_w only, so this can be stale — the hand-rolled LBA reads it
    StereoFrame stereo_frame;
};

// include/mapFeatures.h:39-66 and src/mapFeatures.cpp:38-94
struct MapPoint {
    int idx = -1;
    bool inlier = true;
    bool local = false;
    Vec3 point3D{};
    Vec3 med_obs_dir{};
    Desc med_desc;
    std::vector<Desc> desc_list;
    std::vector<Vec2> obs_list;
    std::vector<Vec3> dir_list;
    std::vector<int> kf_obs_list;
    std::vector<double> sigma_list;
    LandmarkStore *store = nullptr;  // the owning MapHandler's incremental window (set when placed)

    MapPoint(int idx_, const Vec3 &p, const Desc &desc, int kf_obs, const Vec2 &obs, const Vec3 &dir, double sigma2);
    void addMapPointObservation(const Desc &desc, int kf_obs, const Vec2 &obs, const Vec3 &dir, double sigma2);
    void updateAverageDescDir();
    void updateAverageDir();  // the direction half of updateAverageDescDir (src/mapFeatures.cpp:88-92)
};

// include/mapFeatures.h:68-107 (Plücker constructor, src/mapFeatures.cpp:114-138, 140-184
// with USE_LINE_PLUKER: no direction average)
struct MapLine {
    int idx = -1;
    bool inlier = true;
    bool local = false;
    Vec6 NDw{};
    Vec4 orthNDw{};  // set by localBundleAdjustmentForPluker (src/mapHandler.cpp:1577)
    Desc med_desc;
    std::vector<Desc> desc_list;
    std::vector<Vec4> NDw_obs_list;
    std::vector<int> kf_obs_list;
    std::vector<double> sigma_list;
    // endpoint geometry (include/mapFeatures.h:93-100): not set by the Plücker constructor
    // (src/mapFeatures.cpp:110-118, left uninitialised there, zero here); the loop-closure
    // write-back transforms it (src/mapHandler.cpp:5224-5238)
    Vec6 line3D{};
    Vec3 med_obs_dir{};
    std::vector<Vec3> dir_list;
    LandmarkStore *store = nullptr;

    MapLine(int idx_, const Vec6 &NDw_, const Desc &desc, int kf_obs, const Vec4 &obs, double sigma2);
    void addMapLineObservation(const Desc &desc, int kf_obs, const Vec4 &obs, double sigma2);
    void updateAverageDescDir();

    static Vec4 changePlukerToOrth(const Vec6 &L);
    static Vec6 changeOrthToPluker(const Vec4 &o);
};

// Marshalled window: the plba_graph SoA arrays plus the back-references the outlier pass and
// the write-back need (vpEdgeKFMono / vpMapPointEdgeMono / vpLmObsIdx, ...).
struct Window {
    std::vector<KeyFrame *> nofix_kfs, fix_kfs;  // idx_nofix_kfs / idx_fix_kfs in id order
    std::vector<MapPoint *> local_pt;
    std::vector<MapLine *> local_ls;
    int max_kf_id = 0, maxPointId = 0;
    // plba_graph arrays
    wvector<double> kf_Tcw, pt_xyz, ln_orth, ept_obs, ept_info, eln_obs, eln_info;
    wvector<uint8_t> kf_fixed;
    wvector<int32_t> kf_id, pt_id, ln_id, ept_lm, ept_kf, eln_lm, eln_kf;
    // per-edge back references
    std::vector<KeyFrame *> ept_kfp, eln_kfp;
    std::vector<int> ept_obs_idx, eln_obs_idx;
    plba_graph graph(double fx, double fy, double cx, double cy) const;
    // empty, keeping every array's capacity (a MapHandler reuses one Window across calls: the
    // arrays of a C3 window are ~6 MB, and fresh pages cost more than filling them)
    void clear();
};

struct LbaStats {
    int n_free_kf = 0, n_fixed_kf = 0, n_pt = 0, n_ln = 0, n_ept = 0, n_eln = 0;
    int bad_line_stage1 = 0, bad_point_obs = 0, actually_bad_point_obs = 0, bad_line_obs = 0,
        actually_bad_line_obs = 0;
    int iters[2] = {0, 0};
    double chi2[2] = {0, 0};
    double gather_ms = 0, solve_ms = 0, bookkeeping_ms = 0;
    double upload_ms = 0;      // plba_upload, part of solve_ms
    int dirty_landmarks = 0;   // landmarks re-read from their objects by the gather (incremental mode)
};

using SolveFn = int (*)(void *user, const plba_graph *g, plba_result *r);
using HlmSolveFn = int (*)(void *user, const plba_graph *g, const plba_hlm_state *st, const plba_hlm_params *p,
                           plba_hlm_result *r);

// One localBundleAdjustmentForPluker call (hand-rolled LM).
struct HlmStats {
    int ret = 0;  // the reference's return value: 0, or -1 (no observations / VO inserting a KF)
    int n_kf_list = 0, n_fixed_kf = 0, n_pt = 0, n_ln = 0, n_pt_obs = 0, n_ls_obs = 0;
    int linearizations = 0, solves = 0, accepted = 0;
    int pt_outliers = 0, ln_outliers = 0;  // inlier = false set by the write-back (|DX| > 0.01)
    double err = 0, lambda = 0, gather_ms = 0, solve_ms = 0, writeback_ms = 0;
};

// The SlamConfig values the local-mapping step reads (src/slamConfig.cpp:48,61-62 defaults).
struct SlamParams {
    int min_lm_obs = 5;         // SlamConfig::minLMObs()
    int min_lm_cov_graph = 75;  // SlamConfig::minLMCovGraph()
    int min_kf_local_map = 3;   // SlamConfig::minKFLocalMap()
    int min_lm_ess_graph = 150; // SlamConfig::minLMEssGraph()  (src/slamConfig.cpp:60)
    int max_iters_pgo = 100;    // SlamConfig::maxItersPGO()    (src/slamConfig.cpp:79)
};

using PgoSolveFn = int (*)(void *user, const plba_pgo_graph *g, const plba_pgo_params *p, plba_pgo_result *r);

// One loopClosureOptimization{EssGraph,CovGraph}G2O call.
struct PgoStats {
    int kf_prev_idx = 0, kf_curr_idx = -1;
    int n_vertices = 0, n_fixed = 0, n_edges = 0, n_loop_edges = 0;
    int iterations = 0, trials = 0;
    double chi2_initial = 0, chi2_final = 0, solve_ms = 0;
};

using LcposeSolveFn = int (*)(void *user, const plba_lcpose_batch *b, const plba_lcpose_params *p, plba_lcpose_out *out,
                              uint8_t *pt_inlier, uint8_t *ln_inlier);
using Vec4i = std::array<int, 4>;
using MatchFn = int (*)(void *user, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches);

// The configuration values isLoopClosure's matching reads (src2/config.cpp:46-47,51,60,68).
struct MatchParams {
    float min_ratio_12_p = 0.9f, min_ratio_12_l = 0.9f;
    bool best_lr = true, has_points = true, has_lines = true;
};

// What isLoopClosure (src/mapHandler.cpp:4303-4411) has after its descriptor matching: the feature
// counts of both keyframes and the matched features with their lc_pt_idx / lc_ls_idx rows.
struct LcCandidate {
    int kf_prev_idx = 0, kf_curr_idx = 0;
    int n_pt_0 = 0, n_pt_1 = 0, n_ls_0 = 0, n_ls_1 = 0;  // stereo_pt / stereo_ls sizes of kf0, kf1
    bool has_points = true, has_lines = true;            // SlamConfig::hasPoints() / hasLines()
    int n_pt = 0, n_ln = 0;                              // matches
    const double *pt_P = nullptr, *pt_obs = nullptr, *ln_sP = nullptr, *ln_eP = nullptr, *ln_le = nullptr;
    const int32_t *pt_idx = nullptr, *ls_idx = nullptr;  // [n][4]
};

// One loopClosure() step (src/mapHandler.cpp:4053-4116) after lookForLoopCandidates.
struct LcStats {
    int is_candidate = 0, ratio_ok = 0, accepted = 0, conditions = 0;
    int n_inl_pt = 0, n_inl_ln = 0, state_before = 0, state_after = 0, pgo_ran = 0;
    double inl_ratio_pt = 0, inl_ratio_ls = 0, e = 0, unc = 0, t = 0, r_deg = 0, pose_ms = 0;
    PgoStats pgo;
};

using GridMatchFn = int (*)(void *user, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches);

// One place-recognition database operation (plslam_bow_call of plslam_host.h, the same layout) and
// the hook that takes it.
struct BowCall {
    int32_t op, slot, kf_id, n_desc, cap, n;
    const plba_bow_vocab *vocab;
    const uint8_t *desc;
    double *scores;
    int32_t *ids;
    int32_t *word_ids;
    double *values;
};
enum { BOW_SET_VOCAB = 0, BOW_INSERT = 1, BOW_REMOVE = 2, BOW_GET = 3 };
using BowFn = int (*)(void *user, BowCall *c);
// the tests and tools/bow_bench.py only: plba_bow_*'s semantics, single-threaded, on the CPU
struct BowCpuDb;
BowCpuDb *bowCpuNew();
void bowCpuFree(BowCpuDb *db);
int bowCpu(BowCpuDb *db, BowCall *c);

// SlamConfig values of lookForLoopCandidates (src/slamConfig.cpp:61-62,80-82)
struct LcSearchParams {
    int lc_kf_dist = 50, lc_kf_max_dist = 50, lc_nkf_closest = 4, min_lm_cov_graph = 75, min_kf_local_map = 3;
};

// What matchMap2KFPoints / Lines read of SlamConfig and Config (src/slamConfig.cpp:43,51-52,85-86;
// src2/config.cpp:51,60,63,68,92). fast_matching is false in slamConfig.cpp and true in the
// configuration files the reference ships (config/config/config.yaml:5): true here.
struct MapMatchParams {
    bool fast_matching = true, best_lr = true, has_points = true, has_lines = true;
    int ws = 3, min_pt_matches = 10, min_ls_matches = 6;
    double max_kf_epip_p = 1.0, max_kf_epip_l = 1.0, line_sim_th = 0.75, min_ratio_12_p = 0.9, min_ratio_12_l = 0.9;
};

struct MapMatchStats {
    int visible[2] = {0, 0}, unmatched[2] = {0, 0};  // [points, lines]: landmarks projected into the image, features with idx -1
    int grid_matches[2] = {0, 0}, fallback[2] = {0, 0}, accepted[2] = {0, 0}, rejected[2] = {0, 0};
    double match_ms = 0;
};

// The detector output of one stereo frame (plslam_stereo_frame of plslam_host.h, the same layout), what
// setKeyframeStereo reports, and the hook that takes the association.
struct StereoInput {
    int32_t desc_bytes, n_pt_l, n_pt_r, n_ls_l, n_ls_r, pad;
    const float *pt_l, *pt_r;
    const uint8_t *pdesc_l, *pdesc_r;
    const float *ls_l, *ls_r;
    const uint8_t *ldesc_l, *ldesc_r;
};
struct StereoStats {
    int n_pt = 0, n_ls = 0;
    double ms = 0;
};
using StereoFn = int (*)(void *user, const plba_stereo_batch *b, const plba_stereo_params *p, const plba_stereo_out *out);

// What matchKfToKf reports, per kind [points, lines]; pt_pairs / ls_pairs are the accepted (i1, i2) in row
// order, the reference's matched_pt / matched_ls for a caller that runs its own refinement.
struct KfMatchStats {
    int grid_matches[2] = {0, 0}, fallback[2] = {0, 0}, matches[2] = {0, 0};
    int created[2] = {0, 0}, extended[2] = {0, 0}, rejected[2] = {0, 0};
    double match_ms = 0;
    std::vector<std::array<int, 2>> pt_pairs, ls_pairs;
};
using KfAssocFn = int (*)(void *user, const plba_kfassoc_batch *b, const plba_kfassoc_params *p, const plba_kfassoc_out *out);
using MapAssocFn = int (*)(void *user, const plba_mapassoc_batch *b, const plba_mapassoc_params *p, const plba_mapassoc_out *out);

// One loopClosureFuseLandmarks call (fuse_landmarks.cpp), per kind [points, lines]. The four cases in the
// reference's order: observation added to the later landmark (:5552), to the earlier one (:5567), a new
// landmark from both features (:5585), two landmarks fused and the second erased (:5612).
struct FuseStats {
    int loops = 0, loops_skipped = 0;            // loops with flag 1 / with another flag
    int rows[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // rows that passed their guard, per case
    int null_skipped[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // rows whose NULL guard failed, per case
    int same_landmark[2] = {0, 0};               // rows with lm_idx0 == lm_idx1 != -1, left untouched
    int erased[2] = {0, 0};                      // landmarks deleted by the fourth case
    int medoid_lists = 0;                        // lists of the one medoid batch
    double medoid_ms = 0, total_ms = 0;
};
using MedoidFn = int (*)(void *user, const plba_medoid_batch *b, int32_t *medoid);

struct CullStats {
    int points_removed = 0, lines_removed = 0;
};

// A caller's replacement for one device call (the CPU tests, the benchmarks' baselines); unset: the MI355X backend.
template <class Fn>
struct Hook {
    Fn fn = nullptr;
    void *user = nullptr;
};

// include/mapHandler.h:141-151 (the members the LBA uses)
class MapHandler {
  public:
    MapHandler(double fx, double fy, double cx, double cy, const plba_opts *opts = nullptr);
    ~MapHandler();
    MapHandler(const MapHandler &) = delete;
    MapHandler &operator=(const MapHandler &) = delete;

    std::vector<KeyFrame *> map_keyframes;
    std::vector<MapPoint *> map_points;
    std::vector<MapLine *> map_lines;
    std::map<int, std::vector<int>> map_points_kf_idx;
    std::map<int, std::vector<int>> map_lines_kf_idx;
    std::vector<std::vector<unsigned int>> full_graph;
    int max_kf_idx = 0;
    SlamParams params;

    // src/mapHandler.cpp:1073-1137: the local window around `kf` (covisibility >= min_lm_cov_graph
    // landmarks or within min_kf_local_map keyframes of the newest), by the `local` flags.
    int formLocalMap(int kf_idx);
    // src/mapHandler.cpp:3816-3897: delete old non-local landmarks that are outliers or have
    // fewer than min_lm_obs observations (slots become NULL).
    int removeBadMapLandmarksForPluker(CullStats *cs = nullptr);
    // The USE_LINE_PLUKER body of localMappingThread (src/mapHandler.cpp:1264-1280) after
    // lookForCommonMatches (front-end descriptor matching, not part of this library):
    // formLocalMap(kf) -> localBundleAdjustmentForPlukerWithG2O() -> removeBadMapLandmarksForPluker().
    int localMappingStep(int kf_idx, LbaStats *stats = nullptr, CullStats *cs = nullptr);

    // src/mapHandler.cpp:5851. Returns PLBA_OK or a PLBA_E_* status (the reference exit(0)s
    // on an inconsistent map, :5894,5910,5998,6062; here the map is left untouched then).
    int localBundleAdjustmentForPlukerWithG2O(LbaStats *stats = nullptr);

    // src/mapHandler.cpp:1505-1615 + levMarquardtOptimizationLBAForPluker (:1618-2332): the
    // hand-rolled LM LBA of the Plücker map (dead code in the reference's localMappingThread,
    // :1277, kept callable). Returns PLBA_OK (stats->ret carries the reference's 0 / -1).
    int localBundleAdjustmentForPluker(HlmStats *stats = nullptr);
    // src/mapHandler.cpp:1392-1502 + levMarquardtOptimizationLBA (:2334-3016): the local BA of a
    // build without USE_LINE_PLUKER — lines are their endpoints line3D, observed as image line
    // equations (the first three entries of NDw_obs_list[i]); write-back :2841-2882 (T_kf_w =
    // expmap_se3(X_i), point3D / line3D = X with inlier = false when they moved more than 0.01).
    // hlm_params with the variant forced to PLBA_HLM_LBA_ENDPOINTS; stats->ret as above.
    int localBundleAdjustment(HlmStats *stats = nullptr);
    plba_hlm_params hlm_params{1e-5, 10.0, 1e-7, 1e-7, 1e-7, 15, 0, PLBA_HLM_LBA_PLUCKER, 0};
    bool vo_inserting_kf = false;  // vo_status == VO_INSERTING_KF (:2160): nothing is written back

    // src/mapHandler.cpp:5070-5299 / :5301-5531: the loop-closure pose graph (VertexSE3 per KF from
    // the loop's first to its last KF, EdgeSE3 for covisible / consecutive pairs and for each
    // loop), optimised on the GPU (plba_pgo_optimize), then the KF poses, their landmarks and
    // every later KF corrected, lc_idx_list marked optimised, lc_state = LC_IDLE.
    // These two leave out loopClosureFuseLandmarks() (:5294, :5526); loopClosureOptimizationFuse runs
    // the same body with the fuse below before the flags are cleared.
    int loopClosureOptimizationEssGraphG2O(PgoStats *stats = nullptr);
    int loopClosureOptimizationCovGraphG2O(PgoStats *stats = nullptr);
    int loopClosureOptimizationFuse(bool ess, PgoStats *stats = nullptr, FuseStats *fs = nullptr);
    // fuse_landmarks.cpp. loopClosureFuseLandmarks() (src/mapHandler.cpp:5533-5808) over lc_pt_idxs /
    // lc_ls_idxs of the loops whose lc_idx_list flag is 1, points then lines, row by row; the median
    // descriptors of the landmarks whose lists changed come from one medoid batch at the end
    // (plba_desc_medoid, or the hook). What the reference leaves undefined is listed in the file's header.
    // Anything invalid returns PLBA_E_INVALID before the map is touched.
    int fuseLandmarks(FuseStats *stats = nullptr);
    void setMedoidFn(MedoidFn fn, void *user) { medoid_ = {fn, user}; }
    // include/mapHandler.h:186-200
    std::vector<Vec3i> lc_idxs, lc_idx_list;
    std::vector<Vec6> lc_poses, lc_pose_list;
    int lc_state = 0;  // LC_IDLE = 0
    enum { LC_IDLE = 0, LC_ACTIVE = 1, LC_READY = 2 };  // include/mapHandler.h:195-197

    // src/mapHandler.cpp:4053-4116, loopClosure() after lookForLoopCandidates (DBoW2, the caller's)
    // from a matched candidate: the inlier-ratio gate (:4384-4409), computeRelativePoseRobustGN on
    // the GPU (plba_lc_relative_pose), the lists and the LC_IDLE / LC_ACTIVE / LC_READY state
    // machine, and on LC_READY the pose graph above. c == nullptr: no candidate was found.
    int loopClosureStep(const LcCandidate *c, double lc_inlier_ratio, LcStats *stats = nullptr);
    // The same with isLoopClosure (:4303-4411) whole, from two keyframe indices: the descriptor
    // matching of :4334 / :4360 in one plba_desc_match call with two pairs (points, lines), then
    // lc_points / lc_lines / lc_pt_idx / lc_ls_idx in i1 order (:4336-4379) into loopClosureStep.
    int isLoopClosure(int kf0_idx, int kf1_idx, const MatchParams &mp, double lc_inlier_ratio, LcStats *stats = nullptr);
    // K candidates for one new keyframe: one match call with 2K pairs, one relative-pose call with
    // those that pass the gate. No map state is changed. accepted [n], pose_inc [n][6],
    // n_matches [n][2]; each may be nullptr.
    int verifyLoopCandidates(int kf_curr_idx, int n, const int32_t *kf_prev_idx, const MatchParams &mp,
                             double lc_inlier_ratio, int32_t *accepted, double *pose_inc, int32_t *n_matches);
    void setMatchFn(MatchFn fn, void *user) { match_ = {fn, user}; }
    // bow.cpp. Place recognition: insertKFBowVectorP / L / PL (src/mapHandler.cpp:4118-4239) over the
    // database of plba_bow_* (or the hook), the float conf_matrix (include/mapHandler.h:153),
    // lookForLoopCandidates (:4241-4301) and loopClosure() whole (:4053-4116).
    std::vector<std::vector<float>> conf_matrix;
    void setBowFn(BowFn fn, void *user) { bow_ = {fn, user}; }
    int setVocabulary(int slot, const plba_bow_vocab *v);
    int removeKeyframe(int kf_idx);
    int insertKfBow(int kf_idx, bool has_points, bool has_lines);
    int lookForLoopCandidates(int kf_curr_idx, const LcSearchParams &p, bool &is_candidate, int &kf_prev_idx);
    int loopClosureKf(int kf_curr_idx, const LcSearchParams &sp, const MatchParams &mp, double lc_inlier_ratio,
                      LcStats *stats = nullptr);
    // map_match.cpp. matchMap2KFPoints + matchMap2KFLines (src/mapHandler.cpp:697-921) for keyframe
    // kf_idx: the local landmarks not yet seen by it that project into the image against its features
    // with idx -1, by one plba_grid_match call (points and lines) and, where the reference falls back
    // to match() (:759-764, :874-879), one plba_desc_match call; then the epipolar tests, the feature
    // idx, addMapPointObservation / addMapLineObservation and full_graph. Twf == nullptr: the inverse
    // of the keyframe's T_kf_w. Anything invalid returns PLBA_E_INVALID before the map is touched.
    int matchMapToKf(int kf_idx, const Mat4 *Twf, const MapMatchParams &p, MapMatchStats *stats = nullptr);
    // matchMapToKf, then localMappingStep
    int localMappingStepKf(int kf_idx, const MapMatchParams &p, MapMatchStats *ms = nullptr, LbaStats *stats = nullptr,
                           CullStats *cs = nullptr);
    void setGridMatchFn(GridMatchFn fn, void *user) { grid_ = {fn, user}; }
    // map_assoc.cpp. The same association around ONE plba_map_associate call (or the hook): the candidates
    // (local, not yet seen by the keyframe) and the features with idx -1 are gathered, the call projects,
    // tests, matches and gates them, and the rows are walked in i1 order, points before lines, as
    // matchMapToKf walks them. It refuses what matchMapToKf refuses and fills the same statistics.
    int matchMapToKfAssoc(int kf_idx, const Mat4 *Twf, const plba_mapassoc_params &p, MapMatchStats *stats = nullptr);
    // matchMapToKfAssoc, then localMappingStep
    int localMappingStepKfAssoc(int kf_idx, const plba_mapassoc_params &p, MapMatchStats *ms = nullptr, LbaStats *stats = nullptr,
                                CullStats *cs = nullptr);
    void setMapAssocFn(MapAssocFn fn, void *user) { mapassoc_ = {fn, user}; }
    // stereo.cpp. StereoFrame::matchStereoPoints + matchStereoLines (src2/stereoFrame.cpp:121-174, :310-435)
    // for keyframe kf_idx from the detector output of its two images: one plba_stereo_associate call (or the
    // hook), stored as plslam_set_keyframe_features + plslam_set_keyframe_line_endpoints would store it.
    // A keyframe added with idx lists must have been added with the surviving counts; one added without
    // is sized here, every idx -1. pt_src / ls_src (may be nullptr) receive the left row of each feature.
    // Anything invalid returns before the keyframe is touched.
    int setKeyframeStereo(int kf_idx, const StereoInput &in, const plba_stereo_params &prm, int32_t *pt_src, int32_t *ls_src,
                          StereoStats *stats = nullptr);
    void setStereoFn(StereoFn fn, void *user) { stereo_ = {fn, user}; }
    // kf_match.cpp. matchKF2KFPoints + matchKF2KFLines (src/mapHandler.cpp:237-366, :368-590, the
    // USE_LINE_PLUKER branch) between two keyframes with features: one plba_kf_associate call (or the hook),
    // then the rows in order as :283-363 and :434-589 walk them: a new landmark takes the index
    // map_points.size() / map_lines.size() (the reference's max_pt_idx / max_ls_idx always equal it, :67-68,
    // :320-321, :519-520), is built by the constructors and adopted by the registry, pushed to
    // map_*_kf_idx of the previous keyframe, and full_graph is bumped both ways; an existing landmark gets
    // the observation and full_graph against every earlier observer (a NULL landmark skips the row); a
    // rejected line resets the idx (both for a new landmark, the current one for an existing). DT == nullptr:
    // expmap(logmap(inverse(T_curr) * T_prev)) (:143-145). p.width == 0: the image size and the camera of
    // setCamera. Anything invalid returns PLBA_E_INVALID before the map is touched. The pose refinement of
    // :937-977 (has_refinement) is not part of it.
    int matchKfToKf(int kf_prev_idx, int kf_curr_idx, const Mat4 *DT, const plba_kfassoc_params &p, KfMatchStats *stats = nullptr);
    // matchKfToKf, then matchMapToKf of the current keyframe: lookForCommonMatches (:923-990) without the refinement
    int lookForCommonMatches(int kf_prev_idx, int kf_curr_idx, const plba_kfassoc_params &kp, const MapMatchParams &mp,
                             KfMatchStats *ks = nullptr, MapMatchStats *ms = nullptr);
    void setKfAssocFn(KfAssocFn fn, void *user) { kfassoc_ = {fn, user}; }
    void setCamera(double fx, double fy, double cx, double cy, int width, int height) {
        fx_ = fx; fy_ = fy; cx_ = cx; cy_ = cy; width_ = width; height_ = height;
    }
    std::vector<std::vector<Vec4i>> lc_pt_idxs, lc_ls_idxs;  // inlier-filtered rows, one list per loop (:4078-4079)
    plba_lcpose_params lcpose_params{1e-7, 1.0, 0.01, 0.3, 1.5, 35.0, 5, 10, PLBA_LCPOSE_ROBUST_GN, 0};
    void setLcposeSolver(LcposeSolveFn fn, void *user) { lcpose_ = {fn, user}; }

    void setSolver(SolveFn fn, void *user) { solve_ = {fn, user}; }
    void setPgoSolver(PgoSolveFn fn, void *user) { pgo_ = {fn, user}; }
    void setHlmSolver(HlmSolveFn fn, void *user) { hlm_ = {fn, user}; }
    const std::string &lastError() const { return err_; }
    void setError(const char *fmt, ...);

    // window gather + marshalling (A1, A1b) — public for tests
    int gatherWindow(Window &w);

    // ---- incremental window (round 6). The handler keeps every landmark's
    // observations flattened into arenas and the set of local landmarks as a registry, so that the
    // gather and formLocalMap cost O(window + changes), not O(map): the reference scans every map
    // landmark (src/mapHandler.cpp:5877-5886, :1076-1091). Landmarks report changes through
    // landmark_changed: placed / replaced (adoptLandmark), observations added (their methods),
    // erased by the outlier pass, deleted by the culling, moved by the loop closure or the hand-rolled
    // LBA. A caller that writes a landmark's fields directly calls markLandmarkChanged, or
    // rebuildLocalRegistry after writing `local` flags, or sets incremental = false (the scan gather).
    bool incremental = true;
    void adoptLandmark(int kind, int idx);
    void markLandmarkChanged(int kind, int idx);
    int setLandmarkLocal(int kind, int idx, bool local);
    void rebuildLocalRegistry();
    // tests: the landmark pass of both gathers on the current map, compared (0 = equal); no mutation
    int checkIncrementalGather(std::string *why = nullptr);

  private:
    // the body of both hand-rolled local BAs: Plücker lines (orthNDw / NDw) or endpoint lines (line3D)
    int handRolledLocalBa(HlmStats *stats, bool endpoints);
    int gatherScan(Window &w, std::vector<uint8_t> &observer);
    int gatherIncremental(Window &w, std::vector<uint8_t> &observer, int *dirty);
    int finishGather(Window &w, const std::vector<uint8_t> &observer);
    std::unique_ptr<LandmarkStore> store_;
    int last_dirty_ = 0;
    double last_upload_ms_ = 0;
    void storePosition(int kind, int idx, const double *pos);  // write-back: the cached position
    int solve(const plba_graph &g, plba_result &r);
    int ensureCtx();
    int outlierPass(Window &w, const std::vector<double> &ept_chi2, const std::vector<uint8_t> &ept_depth_ok,
                    const std::vector<uint8_t> &ept_level, const std::vector<double> &eln_chi2,
                    const std::vector<uint8_t> &eln_level, LbaStats &st);
    double fx_, fy_, cx_, cy_;
    plba_opts opts_{};
    bool have_opts_ = false;
    plba_ctx *ctx_ = nullptr;  // reused across LBA calls
    Hook<SolveFn> solve_;
    Hook<HlmSolveFn> hlm_;
    Hook<PgoSolveFn> pgo_;
    Hook<LcposeSolveFn> lcpose_;
    Hook<MatchFn> match_;
    Hook<GridMatchFn> grid_;
    Hook<StereoFn> stereo_;
    Hook<KfAssocFn> kfassoc_;
    Hook<MapAssocFn> mapassoc_;
    Hook<MedoidFn> medoid_;
    Hook<BowFn> bow_;
    // One backend call: the hook with args when it is set, otherwise device(ctx_) on the map's context.
    // A failure's message is "<what> hook returned <rc>", ensureCtx's own, or plba's last error.
    template <class Fn, class Device, class... Args>
    int backend(const Hook<Fn> &h, const char *what, Device &&device, Args &&...args) {
        if (h.fn) {
            const int rc = h.fn(h.user, std::forward<Args>(args)...);
            if (rc) setError("%s hook returned %d", what, rc);
            return rc;
        }
        int rc = ensureCtx();
        if (rc) return rc;
        rc = device(ctx_);
        if (rc) setError("plba: %s", plba_last_error(ctx_));
        return rc;
    }
    int bowCall(BowCall &c);                 // the hook, or plba_bow_* on the map's context
    bool bow_vocab_[2] = {false, false};
    std::vector<uint8_t> bow_in_db_[2];      // [kf_idx] the keyframe has a live vector in the slot
    std::vector<uint8_t> bow_inserted_;      // [kf_idx] insertKfBow ran for it
    int width_ = 0, height_ = 0;  // the image size (cam->getWidth() / getHeight()); 0: not set
    // the matched features of kf_prev_idx[0..n) against kf_curr_idx, by one match call
    struct LcBuilt;
    int buildLoopCandidates(int kf_curr_idx, int n, const int32_t *kf_prev_idx, const MatchParams &mp,
                            std::vector<LcBuilt> &out);
    static bool inlierRatioGate(const LcCandidate &c, double lc_inlier_ratio, int &common_pt, int &common_ls,
                                double &ratio_pt, double &ratio_ls);
    int lcRelativePose(const plba_lcpose_batch &b, plba_lcpose_out *out, uint8_t *pin, uint8_t *lin);
    int loopClosurePGO(bool ess, PgoStats *stats, bool fuse = false, FuseStats *fs = nullptr);
    std::string err_;
    // per-call scratch reused across LBA calls (capacity kept; see Window::clear)
    Window win_;
    std::vector<double> out_Tcw_, out_xyz_, out_orth_, out_ept_chi2_, out_eln_chi2_;
    std::vector<uint8_t> out_ept_depth_, out_ept_level_, out_eln_level_;
};

// helpers (host restatements)
Mat4 inverse4(const Mat4 &T);  // Eigen Matrix4d::inverse (general cofactor inverse)
// src2/auxiliar.cpp:113-173 (row-major 4x4, x = [t; ω])
Mat4 inverse_se3(const Mat4 &T);
Mat4 mul4(const Mat4 &A, const Mat4 &B);  // Matrix4d * Matrix4d
Mat4 expmap_se3(const Vec6 &x);
Vec6 logmap_se3(const Mat4 &T);
int hamming(const Desc &a, const Desc &b);
// tools/descmatch_bench.py only: plba_desc_match's semantics, single-threaded, on the CPU
int descMatchCpu(const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches);
// map_match.cpp. getLineCoords / LineIterator (src2/gridStructure.cpp:33-41, src2/lineIterator.cpp): the
// cells a line from (x1, y1) to (x2, y2), in grid units, is entered under in the matching grid
// Returns the number of cells and writes at most max_out of them; -1 for coordinates that are not
// finite or beyond +-1e6 cells.
long lineCells(double x1, double y1, double x2, double y2, std::vector<std::array<int, 2>> &out, size_t max_out);
// tools/gridmatch_bench.py and the tests only: plba_grid_match's semantics, single-threaded, on the CPU
int gridMatchCpu(const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches);
// the same with a window of four half-widths per problem (win [n][4]: left, right, up, down; b->ws is not read)
int gridMatchCpuWin(const plba_gridmatch_batch *b, const int32_t *win, int32_t *matches_12, int32_t *n_matches);
// fuse_landmarks.cpp. tools/fuse_bench.py and the tests only: plba_desc_medoid's semantics, single-threaded, on the CPU
int descMedoidCpu(const plba_medoid_batch *b, int32_t *medoid);
// stereo.cpp. tools/stereo_bench.py and the tests only: plba_stereo_associate's semantics, single-threaded, on the CPU
int stereoCpu(const plba_stereo_batch *b, const plba_stereo_params *p, const plba_stereo_out *out);
// host/track_pose.cpp: plba_track_pose's semantics on the CPU, single-threaded, sums in match order
int trackPoseCpu(const plba_track_batch *b, const plba_track_params *p, plba_track_out *out, uint8_t *pt_inlier,
                 uint8_t *ln_inlier);
// host/track_frames.cpp: plba_track_frames' semantics on the CPU, composed of descMatchCpu and trackPoseCpu
int trackFramesCpu(const plba_frames_batch *b, const plba_frames_params *p, const plba_frames_out *out);
// kf_match.cpp. tools/kfassoc_bench.py and the tests only: plba_kf_associate's semantics, single-threaded, on the CPU
int kfAssocCpu(const plba_kfassoc_batch *b, const plba_kfassoc_params *p, const plba_kfassoc_out *out);
// map_assoc.cpp. tools/mapassoc_bench.py and the tests only: plba_map_associate's semantics, single-threaded, on the CPU
int mapAssocCpu(const plba_mapassoc_batch *b, const plba_mapassoc_params *p, const plba_mapassoc_out *out);

}  // namespace plslam
