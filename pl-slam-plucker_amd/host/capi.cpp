// C ABI of the host mirror (include/plslam_host.h) over plslam::MapHandler.
#include "plslam_host.h"

#include <cstring>
#include <string>
#include <new>

#include "plslam_map.hpp"

using namespace plslam;

struct plslam_map {
    MapHandler mh;
    int desc_bytes = 32;
    plslam_map(double fx, double fy, double cx, double cy, const plba_opts *o) : mh(fx, fy, cx, cy, o) {}
};

namespace {
Desc make_desc(const uint8_t *d, int n) { return d ? Desc(d, d + n) : Desc((size_t)n, 0); }

template <typename T>
bool slot_ok(std::vector<T *> &v, int idx) {
    return idx >= 0 && idx < (int)v.size() && v[idx] != nullptr;
}
template <typename T>
void place(std::vector<T *> &v, int idx, T *p) {
    if ((int)v.size() <= idx) v.resize(idx + 1, nullptr);
    delete v[idx];
    v[idx] = p;
}
// every plslam_set_*_fn / plslam_set_*_solver: the hook (or nullptr) to the MapHandler's setter
template <class Fn>
int set_hook(plslam_map *m, void (MapHandler::*set)(Fn, void *), Fn fn, void *user) {
    if (!m) return PLBA_E_INVALID;
    (m->mh.*set)(fn, user);
    return PLBA_OK;
}
}  // namespace

extern "C" {

int plslam_map_create(plslam_map **m, double fx, double fy, double cx, double cy, const plba_opts *opts) {
    if (!m) return PLBA_E_INVALID;
    *m = new (std::nothrow) plslam_map(fx, fy, cx, cy, opts);
    return *m ? PLBA_OK : PLBA_E_NOMEM;
}

int plslam_map_destroy(plslam_map *m) {
    delete m;
    return PLBA_OK;
}

const char *plslam_map_last_error(plslam_map *m) { return m ? m->mh.lastError().c_str() : "null map"; }

int plslam_set_solver(plslam_map *m, plslam_solve_fn fn, void *user) { return set_hook(m, &MapHandler::setSolver, fn, user); }

int plslam_add_keyframe(plslam_map *m, int32_t kf_idx, const double T_kf_w[16], int32_t n_pt_feat,
                        const int32_t *pt_idx, int32_t n_ls_feat, const int32_t *ls_idx) {
    if (!m || kf_idx < 0 || !T_kf_w || n_pt_feat < 0 || n_ls_feat < 0) return PLBA_E_INVALID;
    auto *k = new KeyFrame();
    k->kf_idx = kf_idx;
    std::memcpy(k->T_kf_w.data(), T_kf_w, sizeof(double) * 16);
    k->x_kf_w = logmap_se3(k->T_kf_w);  // x_kf_w = logmap_se3(T) at insertion (src/mapHandler.cpp:140,179)
    if (pt_idx) k->stereo_frame.stereo_pt_idx.assign(pt_idx, pt_idx + n_pt_feat);
    if (ls_idx) k->stereo_frame.stereo_ls_idx.assign(ls_idx, ls_idx + n_ls_feat);
    place(m->mh.map_keyframes, kf_idx, k);
    return PLBA_OK;
}

int plslam_add_point(plslam_map *m, int32_t idx, const double xyz[3], const uint8_t *desc, int32_t desc_bytes,
                     int32_t kf, const double obs[2], const double dir[3], double sigma2) {
    if (!m || idx < 0 || !xyz || !obs || desc_bytes <= 0) return PLBA_E_INVALID;
    m->desc_bytes = desc_bytes;
    Vec3 d = dir ? Vec3{dir[0], dir[1], dir[2]} : Vec3{0, 0, 0};
    place(m->mh.map_points, idx,
          new MapPoint(idx, Vec3{xyz[0], xyz[1], xyz[2]}, make_desc(desc, desc_bytes), kf, Vec2{obs[0], obs[1]}, d,
                       sigma2));
    m->mh.adoptLandmark(1, idx);
    return PLBA_OK;
}

int plslam_point_add_observation(plslam_map *m, int32_t idx, const uint8_t *desc, int32_t kf, const double obs[2],
                                 const double dir[3], double sigma2) {
    if (!m || !obs || !slot_ok(m->mh.map_points, idx)) return PLBA_E_INVALID;
    Vec3 d = dir ? Vec3{dir[0], dir[1], dir[2]} : Vec3{0, 0, 0};
    m->mh.map_points[idx]->addMapPointObservation(make_desc(desc, m->desc_bytes), kf, Vec2{obs[0], obs[1]}, d, sigma2);
    return PLBA_OK;
}

int plslam_add_line(plslam_map *m, int32_t idx, const double NDw[6], const uint8_t *desc, int32_t desc_bytes,
                    int32_t kf, const double obs[4], double sigma2) {
    if (!m || idx < 0 || !NDw || !obs || desc_bytes <= 0) return PLBA_E_INVALID;
    m->desc_bytes = desc_bytes;
    Vec6 L;
    std::memcpy(L.data(), NDw, sizeof(double) * 6);
    place(m->mh.map_lines, idx,
          new MapLine(idx, L, make_desc(desc, desc_bytes), kf, Vec4{obs[0], obs[1], obs[2], obs[3]}, sigma2));
    m->mh.adoptLandmark(2, idx);
    return PLBA_OK;
}

int plslam_line_add_observation(plslam_map *m, int32_t idx, const uint8_t *desc, int32_t kf, const double obs[4],
                                double sigma2) {
    if (!m || !obs || !slot_ok(m->mh.map_lines, idx)) return PLBA_E_INVALID;
    m->mh.map_lines[idx]->addMapLineObservation(make_desc(desc, m->desc_bytes), kf,
                                                Vec4{obs[0], obs[1], obs[2], obs[3]}, sigma2);
    return PLBA_OK;
}

int plslam_set_local(plslam_map *m, int32_t kind, int32_t idx, int32_t local) {
    if (!m) return PLBA_E_INVALID;
    switch (kind) {
        case 0:
            if (!slot_ok(m->mh.map_keyframes, idx)) return PLBA_E_INVALID;
            m->mh.map_keyframes[idx]->local = local != 0;
            return PLBA_OK;
        case 1:
        case 2:
            return m->mh.setLandmarkLocal(kind, idx, local != 0);
        default:
            return PLBA_E_INVALID;
    }
}

int plslam_set_inlier(plslam_map *m, int32_t kind, int32_t idx, int32_t inlier) {
    if (!m) return PLBA_E_INVALID;
    if (kind == 1 && slot_ok(m->mh.map_points, idx)) {
        m->mh.map_points[idx]->inlier = inlier != 0;
        return PLBA_OK;
    }
    if (kind == 2 && slot_ok(m->mh.map_lines, idx)) {
        m->mh.map_lines[idx]->inlier = inlier != 0;
        return PLBA_OK;
    }
    return PLBA_E_INVALID;
}

int plslam_set_full_graph(plslam_map *m, int32_t n, const uint32_t *g) {
    if (!m || n < 0 || (n && !g)) return PLBA_E_INVALID;
    m->mh.full_graph.assign(n, std::vector<unsigned int>(n, 0));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) m->mh.full_graph[i][j] = g[(size_t)i * n + j];
    return PLBA_OK;
}

int plslam_get_full_graph(plslam_map *m, int32_t n, uint32_t *g) {
    if (!m || !g || n != (int)m->mh.full_graph.size()) return PLBA_E_INVALID;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) g[(size_t)i * n + j] = m->mh.full_graph[i][j];
    return PLBA_OK;
}

int plslam_kf_idx_set(plslam_map *m, int32_t kf, const int32_t *lm, int32_t n) {
    if (!m || n < 0 || (n && !lm)) return PLBA_E_INVALID;
    m->mh.map_points_kf_idx[kf].assign(lm, lm + n);
    return PLBA_OK;
}

int plslam_kf_idx_get(plslam_map *m, int32_t kf, int32_t *out, int32_t cap, int32_t *n) {
    if (!m || !n) return PLBA_E_INVALID;
    auto it = m->mh.map_points_kf_idx.find(kf);
    if (it == m->mh.map_points_kf_idx.end()) {
        *n = -1;
        return PLBA_OK;
    }
    *n = (int32_t)it->second.size();
    for (int i = 0; out && i < *n && i < cap; ++i) out[i] = it->second[i];
    return PLBA_OK;
}

static void copy_stats(const LbaStats &st, plslam_lba_stats *stats) {
    if (stats) {
        stats->n_free_kf = st.n_free_kf; stats->n_fixed_kf = st.n_fixed_kf;
        stats->n_pt = st.n_pt; stats->n_ln = st.n_ln; stats->n_ept = st.n_ept; stats->n_eln = st.n_eln;
        stats->bad_line_stage1 = st.bad_line_stage1;
        stats->bad_point_obs = st.bad_point_obs; stats->actually_bad_point_obs = st.actually_bad_point_obs;
        stats->bad_line_obs = st.bad_line_obs; stats->actually_bad_line_obs = st.actually_bad_line_obs;
        stats->iters[0] = st.iters[0]; stats->iters[1] = st.iters[1];
        stats->chi2[0] = st.chi2[0]; stats->chi2[1] = st.chi2[1];
        stats->gather_ms = st.gather_ms; stats->solve_ms = st.solve_ms; stats->bookkeeping_ms = st.bookkeeping_ms;
        stats->upload_ms = st.upload_ms;
        stats->dirty_landmarks = st.dirty_landmarks;
    }
}

int plslam_set_incremental(plslam_map *m, int32_t on) {
    if (!m) return PLBA_E_INVALID;
    m->mh.incremental = on != 0;
    m->mh.rebuildLocalRegistry();
    return PLBA_OK;
}

int plslam_mark_landmark_changed(plslam_map *m, int32_t kind, int32_t idx) {
    if (!m || (kind != 1 && kind != 2) || idx < 0) return PLBA_E_INVALID;
    m->mh.markLandmarkChanged(kind, idx);
    return PLBA_OK;
}

int plslam_check_incremental_gather(plslam_map *m, int32_t *equal) {
    if (!m || !equal) return PLBA_E_INVALID;
    std::string why;
    const int rc = m->mh.checkIncrementalGather(&why);
    *equal = rc == 0 ? 1 : 0;
    if (rc) m->mh.setError("incremental gather differs from the scan gather: %s", why.c_str());
    return PLBA_OK;
}

int plslam_local_ba_plucker_g2o(plslam_map *m, plslam_lba_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    LbaStats st;
    const int rc = m->mh.localBundleAdjustmentForPlukerWithG2O(&st);
    if (rc) return rc;
    copy_stats(st, stats);
    return PLBA_OK;
}

int plslam_set_keyframe_x(plslam_map *m, int32_t kf_idx, const double x[6]) {
    if (!m || !x || !slot_ok(m->mh.map_keyframes, kf_idx)) return PLBA_E_INVALID;
    std::memcpy(m->mh.map_keyframes[kf_idx]->x_kf_w.data(), x, sizeof(double) * 6);
    return PLBA_OK;
}

int plslam_get_keyframe_x(plslam_map *m, int32_t kf_idx, double x[6]) {
    if (!m || !x || !slot_ok(m->mh.map_keyframes, kf_idx)) return PLBA_E_INVALID;
    std::memcpy(x, m->mh.map_keyframes[kf_idx]->x_kf_w.data(), sizeof(double) * 6);
    return PLBA_OK;
}

int plslam_set_hlm_solver(plslam_map *m, plslam_hlm_solve_fn fn, void *user) { return set_hook(m, &MapHandler::setHlmSolver, fn, user); }

static int hand_rolled_local_ba(plslam_map *m, plslam_hlm_stats *stats, bool endpoints);

int plslam_set_hlm_params(plslam_map *m, const plba_hlm_params *p, int32_t vo_inserting_kf) {
    if (!m) return PLBA_E_INVALID;
    if (p) m->mh.hlm_params = *p;
    else plba_hlm_default_params(&m->mh.hlm_params);
    m->mh.vo_inserting_kf = vo_inserting_kf != 0;
    return PLBA_OK;
}

int plslam_local_ba_plucker(plslam_map *m, plslam_hlm_stats *stats) { return hand_rolled_local_ba(m, stats, false); }
int plslam_local_ba(plslam_map *m, plslam_hlm_stats *stats) { return hand_rolled_local_ba(m, stats, true); }

static int hand_rolled_local_ba(plslam_map *m, plslam_hlm_stats *stats, bool endpoints) {
    if (!m) return PLBA_E_INVALID;
    HlmStats st;
    const int rc = endpoints ? m->mh.localBundleAdjustment(&st) : m->mh.localBundleAdjustmentForPluker(&st);
    if (rc) return rc;
    if (stats) {
        stats->ret = st.ret;
        stats->n_kf_list = st.n_kf_list; stats->n_fixed_kf = st.n_fixed_kf;
        stats->n_pt = st.n_pt; stats->n_ln = st.n_ln; stats->n_pt_obs = st.n_pt_obs; stats->n_ls_obs = st.n_ls_obs;
        stats->linearizations = st.linearizations; stats->solves = st.solves; stats->accepted = st.accepted;
        stats->pt_outliers = st.pt_outliers; stats->ln_outliers = st.ln_outliers;
        stats->err = st.err; stats->lambda = st.lambda;
        stats->gather_ms = st.gather_ms; stats->solve_ms = st.solve_ms; stats->writeback_ms = st.writeback_ms;
    }
    return PLBA_OK;
}

int plslam_set_loop_closure(plslam_map *m, int32_t n_lc_idxs, const int32_t *lc_idxs, int32_t n_lc_idx_list,
                            const int32_t *lc_idx_list, int32_t n_lc_pose_list, const double *lc_pose_list) {
    if (!m || n_lc_idxs < 0 || n_lc_idx_list < 0 || n_lc_pose_list < 0 || (n_lc_idxs && !lc_idxs) ||
        (n_lc_idx_list && !lc_idx_list) || (n_lc_pose_list && !lc_pose_list))
        return PLBA_E_INVALID;
    MapHandler &mh = m->mh;
    mh.lc_idxs.assign((size_t)n_lc_idxs, Vec3i{});
    for (int i = 0; i < n_lc_idxs; ++i) mh.lc_idxs[i] = Vec3i{lc_idxs[3 * i], lc_idxs[3 * i + 1], lc_idxs[3 * i + 2]};
    mh.lc_idx_list.assign((size_t)n_lc_idx_list, Vec3i{});
    for (int i = 0; i < n_lc_idx_list; ++i)
        mh.lc_idx_list[i] = Vec3i{lc_idx_list[3 * i], lc_idx_list[3 * i + 1], lc_idx_list[3 * i + 2]};
    mh.lc_pose_list.assign((size_t)n_lc_pose_list, Vec6{});
    for (int i = 0; i < n_lc_pose_list; ++i)
        for (int k = 0; k < 6; ++k) mh.lc_pose_list[i][k] = lc_pose_list[6 * i + k];
    return PLBA_OK;
}

int plslam_get_lc_idx_list(plslam_map *m, int32_t *out, int32_t cap, int32_t *n) {
    if (!m) return PLBA_E_INVALID;
    const auto &l = m->mh.lc_idx_list;
    if (n) *n = (int32_t)l.size();
    for (int i = 0; i < (int)l.size() && i < cap && out; ++i)
        for (int k = 0; k < 3; ++k) out[3 * i + k] = l[i][k];
    return PLBA_OK;
}

int plslam_set_pgo_params(plslam_map *m, int32_t min_lm_ess_graph, int32_t max_iters_pgo) {
    if (!m || max_iters_pgo < 0) return PLBA_E_INVALID;
    m->mh.params.min_lm_ess_graph = min_lm_ess_graph;
    m->mh.params.max_iters_pgo = max_iters_pgo;
    return PLBA_OK;
}

int plslam_set_pgo_solver(plslam_map *m, plslam_pgo_solve_fn fn, void *user) { return set_hook(m, &MapHandler::setPgoSolver, fn, user); }

namespace {
void export_pgo_stats(const PgoStats &st, plslam_pgo_stats *stats) {
    stats->kf_prev_idx = st.kf_prev_idx; stats->kf_curr_idx = st.kf_curr_idx;
    stats->n_vertices = st.n_vertices; stats->n_fixed = st.n_fixed; stats->n_edges = st.n_edges;
    stats->n_loop_edges = st.n_loop_edges; stats->iterations = st.iterations; stats->trials = st.trials;
    stats->chi2_initial = st.chi2_initial; stats->chi2_final = st.chi2_final; stats->solve_ms = st.solve_ms;
}
void export_fuse_stats(const FuseStats &st, plslam_fuse_stats *stats) {
    stats->loops = st.loops; stats->loops_skipped = st.loops_skipped;
    for (int k = 0; k < 2; ++k) {
        for (int c = 0; c < 4; ++c) {
            stats->rows[k][c] = st.rows[k][c];
            stats->null_skipped[k][c] = st.null_skipped[k][c];
        }
        stats->same_landmark[k] = st.same_landmark[k];
        stats->erased[k] = st.erased[k];
    }
    stats->medoid_lists = st.medoid_lists; stats->pad = 0;
    stats->medoid_ms = st.medoid_ms; stats->total_ms = st.total_ms;
}
}  // namespace

int plslam_loop_closure_optimization(plslam_map *m, int32_t ess, plslam_pgo_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    PgoStats st;
    const int rc = ess ? m->mh.loopClosureOptimizationEssGraphG2O(&st) : m->mh.loopClosureOptimizationCovGraphG2O(&st);
    if (rc) return rc;
    if (stats) export_pgo_stats(st, stats);
    return PLBA_OK;
}

int plslam_loop_closure_optimization_fuse(plslam_map *m, int32_t ess, plslam_pgo_stats *pgo_stats,
                                          plslam_fuse_stats *fuse_stats) {
    if (!m) return PLBA_E_INVALID;
    PgoStats st;
    FuseStats fs;
    const int rc = m->mh.loopClosureOptimizationFuse(ess != 0, &st, &fs);
    if (rc) return rc;
    if (pgo_stats) export_pgo_stats(st, pgo_stats);
    if (fuse_stats) export_fuse_stats(fs, fuse_stats);
    return PLBA_OK;
}

int plslam_fuse_landmarks(plslam_map *m, plslam_fuse_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    FuseStats fs;
    const int rc = m->mh.fuseLandmarks(&fs);
    if (rc) return rc;
    if (stats) export_fuse_stats(fs, stats);
    return PLBA_OK;
}

int plslam_set_medoid_fn(plslam_map *m, plslam_medoid_fn fn, void *user) { return set_hook(m, &MapHandler::setMedoidFn, fn, user); }

int plslam_desc_medoid_cpu(void *user, const plba_medoid_batch *b, int32_t *medoid) {
    (void)user;
    return descMedoidCpu(b, medoid);
}

int plslam_set_lcpose_solver(plslam_map *m, plslam_lcpose_solve_fn fn, void *user) { return set_hook(m, &MapHandler::setLcposeSolver, fn, user); }

int plslam_set_lcpose_params(plslam_map *m, const plba_lcpose_params *p) {
    if (!m) return PLBA_E_INVALID;
    if (p) m->mh.lcpose_params = *p;
    else plba_lcpose_default_params(&m->mh.lcpose_params);
    return PLBA_OK;
}

namespace {
void export_lc_stats(const LcStats &st, plslam_lc_stats *stats) {
    stats->is_candidate = st.is_candidate; stats->ratio_ok = st.ratio_ok;
    stats->accepted = st.accepted; stats->conditions = st.conditions;
    stats->n_inl_pt = st.n_inl_pt; stats->n_inl_ln = st.n_inl_ln;
    stats->state_before = st.state_before; stats->state_after = st.state_after;
    stats->pgo_ran = st.pgo_ran; stats->pad = 0;
    stats->inl_ratio_pt = st.inl_ratio_pt; stats->inl_ratio_ls = st.inl_ratio_ls;
    stats->e = st.e; stats->unc = st.unc; stats->t = st.t; stats->r_deg = st.r_deg; stats->pose_ms = st.pose_ms;
    const PgoStats &g = st.pgo;
    stats->pgo.kf_prev_idx = g.kf_prev_idx; stats->pgo.kf_curr_idx = g.kf_curr_idx;
    stats->pgo.n_vertices = g.n_vertices; stats->pgo.n_fixed = g.n_fixed; stats->pgo.n_edges = g.n_edges;
    stats->pgo.n_loop_edges = g.n_loop_edges; stats->pgo.iterations = g.iterations; stats->pgo.trials = g.trials;
    stats->pgo.chi2_initial = g.chi2_initial; stats->pgo.chi2_final = g.chi2_final; stats->pgo.solve_ms = g.solve_ms;
}
}  // namespace

int plslam_loop_closure_step(plslam_map *m, const plslam_lc_candidate *c, double lc_inlier_ratio, plslam_lc_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    LcCandidate cc;
    if (c) {
        cc.kf_prev_idx = c->kf_prev_idx; cc.kf_curr_idx = c->kf_curr_idx;
        cc.n_pt_0 = c->n_pt_0; cc.n_pt_1 = c->n_pt_1; cc.n_ls_0 = c->n_ls_0; cc.n_ls_1 = c->n_ls_1;
        cc.has_points = c->has_points != 0; cc.has_lines = c->has_lines != 0;
        cc.n_pt = c->n_pt; cc.n_ln = c->n_ln;
        cc.pt_P = c->pt_P; cc.pt_obs = c->pt_obs; cc.ln_sP = c->ln_sP; cc.ln_eP = c->ln_eP; cc.ln_le = c->ln_le;
        cc.pt_idx = c->pt_idx; cc.ls_idx = c->ls_idx;
    }
    LcStats st;
    const int rc = m->mh.loopClosureStep(c ? &cc : nullptr, lc_inlier_ratio, &st);
    if (rc) return rc;
    if (stats) export_lc_stats(st, stats);
    return PLBA_OK;
}

int plslam_set_keyframe_features(plslam_map *m, int32_t kf_idx, int32_t desc_bytes, const uint8_t *pdesc,
                                 const double *pt_P, const double *pt_pl, const uint8_t *ldesc, const double *ls_sP,
                                 const double *ls_eP, const double *ls_le) {
    if (!m || !slot_ok(m->mh.map_keyframes, kf_idx) || desc_bytes < 4 || desc_bytes > 64 || desc_bytes % 4)
        return PLBA_E_INVALID;
    StereoFrame &f = m->mh.map_keyframes[kf_idx]->stereo_frame;
    const size_t np = f.stereo_pt_idx.size(), nl = f.stereo_ls_idx.size(), db = (size_t)desc_bytes;
    if ((np && (!pdesc || !pt_P || !pt_pl)) || (nl && (!ldesc || !ls_sP || !ls_eP || !ls_le))) return PLBA_E_INVALID;
    f.desc_bytes = desc_bytes;
    f.pdesc_l.assign(pdesc, pdesc + (np ? np * db : 0));
    f.pt_P.assign(pt_P, pt_P + (np ? 3 * np : 0));
    f.pt_pl.assign(pt_pl, pt_pl + (np ? 2 * np : 0));
    f.ldesc_l.assign(ldesc, ldesc + (nl ? nl * db : 0));
    f.ls_sP.assign(ls_sP, ls_sP + (nl ? 3 * nl : 0));
    f.ls_eP.assign(ls_eP, ls_eP + (nl ? 3 * nl : 0));
    f.ls_le.assign(ls_le, ls_le + (nl ? 3 * nl : 0));
    f.has_features = true;
    return PLBA_OK;
}

int plslam_set_match_fn(plslam_map *m, plslam_match_fn fn, void *user) { return set_hook(m, &MapHandler::setMatchFn, fn, user); }

namespace {
MatchParams match_params(const plslam_match_params *mp) {
    MatchParams p;
    if (mp) {
        p.min_ratio_12_p = mp->min_ratio_12_p; p.min_ratio_12_l = mp->min_ratio_12_l;
        p.best_lr = mp->best_lr != 0; p.has_points = mp->has_points != 0; p.has_lines = mp->has_lines != 0;
    }
    return p;
}

}  // namespace

int plslam_loop_closure_step_kf(plslam_map *m, int32_t kf_prev_idx, int32_t kf_curr_idx, const plslam_match_params *mp,
                                double lc_inlier_ratio, plslam_lc_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    LcStats st;
    const int rc = m->mh.isLoopClosure(kf_prev_idx, kf_curr_idx, match_params(mp), lc_inlier_ratio, &st);
    if (rc) return rc;
    if (stats) export_lc_stats(st, stats);
    return PLBA_OK;
}

int plslam_verify_loop_candidates(plslam_map *m, int32_t kf_curr_idx, int32_t n, const int32_t *kf_prev_idx,
                                  const plslam_match_params *mp, double lc_inlier_ratio, int32_t *accepted,
                                  double *pose_inc, int32_t *n_matches) {
    if (!m) return PLBA_E_INVALID;
    return m->mh.verifyLoopCandidates(kf_curr_idx, n, kf_prev_idx, match_params(mp), lc_inlier_ratio, accepted, pose_inc,
                                      n_matches);
}

// ---- place recognition (bow.cpp)
static_assert(sizeof(plslam_bow_call) == sizeof(BowCall), "plslam_bow_call and BowCall share one layout");

int plslam_set_bow_fn(plslam_map *m, plslam_bow_fn fn, void *user) { return set_hook(m, &MapHandler::setBowFn, reinterpret_cast<BowFn>(fn), user); }

void *plslam_bow_cpu_new(void) { return bowCpuNew(); }
void plslam_bow_cpu_free(void *db) { bowCpuFree(static_cast<BowCpuDb *>(db)); }
int plslam_bow_cpu(void *user, plslam_bow_call *c) {
    return bowCpu(static_cast<BowCpuDb *>(user), reinterpret_cast<BowCall *>(c));
}

int plslam_set_vocabulary(plslam_map *m, int32_t slot, const plba_bow_vocab *v) {
    return m ? m->mh.setVocabulary(slot, v) : PLBA_E_INVALID;
}

int plslam_remove_keyframe(plslam_map *m, int32_t kf_idx) { return m ? m->mh.removeKeyframe(kf_idx) : PLBA_E_INVALID; }

int plslam_insert_kf_bow(plslam_map *m, int32_t kf_idx, int32_t has_points, int32_t has_lines) {
    return m ? m->mh.insertKfBow(kf_idx, has_points != 0, has_lines != 0) : PLBA_E_INVALID;
}

int plslam_get_conf_matrix_row(plslam_map *m, int32_t kf_idx, float *out, int32_t cap, int32_t *n) {
    if (!m || !n || cap < 0 || (cap && !out) || kf_idx < 0 || kf_idx >= (int)m->mh.conf_matrix.size()) return PLBA_E_INVALID;
    const std::vector<float> &row = m->mh.conf_matrix[kf_idx];
    *n = (int32_t)row.size();
    for (int i = 0; i < std::min<int>(cap, *n); ++i) out[i] = row[i];
    return PLBA_OK;
}

int plslam_set_conf_matrix(plslam_map *m, int32_t n, const float *c) {
    if (!m || n < 0 || (n && !c)) return PLBA_E_INVALID;
    m->mh.conf_matrix.assign((size_t)n, std::vector<float>((size_t)n, 0.0f));
    for (int i = 0; i < n; ++i) std::memcpy(m->mh.conf_matrix[i].data(), c + (size_t)i * n, sizeof(float) * (size_t)n);
    return PLBA_OK;
}

void plslam_lc_search_default_params(plslam_lc_search_params *p) {
    if (!p) return;
    const LcSearchParams d;
    p->lc_kf_dist = d.lc_kf_dist; p->lc_kf_max_dist = d.lc_kf_max_dist; p->lc_nkf_closest = d.lc_nkf_closest;
    p->min_lm_cov_graph = d.min_lm_cov_graph; p->min_kf_local_map = d.min_kf_local_map; p->pad = 0;
}

namespace {
LcSearchParams search_params(const plslam_lc_search_params *sp) {
    LcSearchParams p;
    if (sp) {
        p.lc_kf_dist = sp->lc_kf_dist; p.lc_kf_max_dist = sp->lc_kf_max_dist; p.lc_nkf_closest = sp->lc_nkf_closest;
        p.min_lm_cov_graph = sp->min_lm_cov_graph; p.min_kf_local_map = sp->min_kf_local_map;
    }
    return p;
}
}  // namespace

int plslam_look_for_loop_candidates(plslam_map *m, int32_t kf_curr_idx, const plslam_lc_search_params *p,
                                    int32_t *is_candidate, int32_t *kf_prev_idx) {
    if (!m || !is_candidate || !kf_prev_idx) return PLBA_E_INVALID;
    bool cand = false;
    int prev = -1;
    const int rc = m->mh.lookForLoopCandidates(kf_curr_idx, search_params(p), cand, prev);
    if (rc) return rc;
    *is_candidate = cand ? 1 : 0;
    *kf_prev_idx = prev;
    return PLBA_OK;
}

int plslam_loop_closure_kf(plslam_map *m, int32_t kf_curr_idx, const plslam_lc_search_params *sp,
                           const plslam_match_params *mp, double lc_inlier_ratio, plslam_lc_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    LcStats st;
    const int rc = m->mh.loopClosureKf(kf_curr_idx, search_params(sp), match_params(mp), lc_inlier_ratio, &st);
    if (rc) return rc;
    if (stats) export_lc_stats(st, stats);
    return PLBA_OK;
}

int plslam_desc_match_cpu(void *user, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches) {
    (void)user;
    return descMatchCpu(b, matches_12, n_matches);
}

int plslam_line_cells(double x1, double y1, double x2, double y2, int32_t *cells, int32_t cap, int32_t *n) {
    if (!n || cap < 0 || (cap > 0 && !cells)) return PLBA_E_INVALID;
    std::vector<std::array<int, 2>> out;
    const long count = lineCells(x1, y1, x2, y2, out, (size_t)cap);
    if (count < 0) return PLBA_E_INVALID;
    *n = (int32_t)count;
    for (size_t i = 0; i < out.size(); ++i) {
        cells[2 * i] = out[i][0];
        cells[2 * i + 1] = out[i][1];
    }
    return PLBA_OK;
}

int plslam_set_keyframe_line_endpoints(plslam_map *m, int32_t kf_idx, const double *spl, const double *epl) {
    if (!m || !slot_ok(m->mh.map_keyframes, kf_idx)) return PLBA_E_INVALID;
    StereoFrame &f = m->mh.map_keyframes[kf_idx]->stereo_frame;
    const size_t nl = f.stereo_ls_idx.size();
    if (nl && (!spl || !epl)) return PLBA_E_INVALID;
    f.ls_spl.assign(spl, spl + (nl ? 2 * nl : 0));
    f.ls_epl.assign(epl, epl + (nl ? 2 * nl : 0));
    f.has_endpoints = true;
    return PLBA_OK;
}

int plslam_set_camera(plslam_map *m, double fx, double fy, double cx, double cy, int32_t width, int32_t height) {
    if (!m || width <= 0 || height <= 0) return PLBA_E_INVALID;
    m->mh.setCamera(fx, fy, cx, cy, width, height);
    return PLBA_OK;
}

int plslam_set_grid_match_fn(plslam_map *m, plslam_grid_match_fn fn, void *user) { return set_hook(m, &MapHandler::setGridMatchFn, fn, user); }

void plslam_mapmatch_default_params(plslam_mapmatch_params *p) {
    if (!p) return;
    const MapMatchParams d;
    *p = plslam_mapmatch_params{d.fast_matching, d.ws, d.min_pt_matches, d.min_ls_matches, d.best_lr, d.has_points,
                                d.has_lines, 0, d.max_kf_epip_p, d.max_kf_epip_l, d.line_sim_th, d.min_ratio_12_p,
                                d.min_ratio_12_l};
}

namespace {
MapMatchParams mapmatch_params(const plslam_mapmatch_params *mp) {
    MapMatchParams p;
    if (mp) {
        p.fast_matching = mp->fast_matching != 0; p.best_lr = mp->best_lr != 0;
        p.has_points = mp->has_points != 0; p.has_lines = mp->has_lines != 0;
        p.ws = mp->ws; p.min_pt_matches = mp->min_pt_matches; p.min_ls_matches = mp->min_ls_matches;
        p.max_kf_epip_p = mp->max_kf_epip_p; p.max_kf_epip_l = mp->max_kf_epip_l; p.line_sim_th = mp->line_sim_th;
        p.min_ratio_12_p = mp->min_ratio_12_p; p.min_ratio_12_l = mp->min_ratio_12_l;
    }
    return p;
}
void export_mapmatch_stats(const MapMatchStats &s, plslam_mapmatch_stats *o) {
    if (!o) return;
    for (int k = 0; k < 2; ++k) {
        o->visible[k] = s.visible[k]; o->unmatched[k] = s.unmatched[k]; o->grid_matches[k] = s.grid_matches[k];
        o->fallback[k] = s.fallback[k]; o->accepted[k] = s.accepted[k]; o->rejected[k] = s.rejected[k];
    }
    o->match_ms = s.match_ms;
}
}  // namespace

int plslam_match_map_to_kf(plslam_map *m, int32_t kf_idx, const double *Twf, const plslam_mapmatch_params *params,
                           plslam_mapmatch_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    Mat4 T;
    if (Twf) std::memcpy(T.data(), Twf, sizeof(double) * 16);
    MapMatchStats st;
    const int rc = m->mh.matchMapToKf(kf_idx, Twf ? &T : nullptr, mapmatch_params(params), &st);
    if (rc) return rc;
    export_mapmatch_stats(st, stats);
    return PLBA_OK;
}

int plslam_local_mapping_step_kf(plslam_map *m, int32_t kf_idx, const plslam_mapmatch_params *params,
                                 plslam_mapmatch_stats *match_stats, plslam_lba_stats *stats, int32_t *n_pt_removed,
                                 int32_t *n_ln_removed) {
    if (!m) return PLBA_E_INVALID;
    MapMatchStats ms;
    LbaStats st;
    CullStats cs;
    const int rc = m->mh.localMappingStepKf(kf_idx, mapmatch_params(params), &ms, &st, &cs);
    if (rc) return rc;
    export_mapmatch_stats(ms, match_stats);
    copy_stats(st, stats);
    if (n_pt_removed) *n_pt_removed = cs.points_removed;
    if (n_ln_removed) *n_ln_removed = cs.lines_removed;
    return PLBA_OK;
}

namespace {
plba_mapassoc_params mapassoc_params(const plba_mapassoc_params *p) {
    plba_mapassoc_params d;
    plba_mapassoc_default_params(&d);
    return p ? *p : d;
}
}  // namespace

int plslam_match_map_to_kf_assoc(plslam_map *m, int32_t kf_idx, const double *Twf, const plba_mapassoc_params *params,
                                 plslam_mapmatch_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    Mat4 T;
    if (Twf) std::memcpy(T.data(), Twf, sizeof(double) * 16);
    MapMatchStats st;
    const int rc = m->mh.matchMapToKfAssoc(kf_idx, Twf ? &T : nullptr, mapassoc_params(params), &st);
    if (rc) return rc;
    export_mapmatch_stats(st, stats);
    return PLBA_OK;
}

int plslam_local_mapping_step_kf_assoc(plslam_map *m, int32_t kf_idx, const plba_mapassoc_params *params,
                                       plslam_mapmatch_stats *match_stats, plslam_lba_stats *stats, int32_t *n_pt_removed,
                                       int32_t *n_ln_removed) {
    if (!m) return PLBA_E_INVALID;
    MapMatchStats ms;
    LbaStats st;
    CullStats cs;
    const int rc = m->mh.localMappingStepKfAssoc(kf_idx, mapassoc_params(params), &ms, &st, &cs);
    if (rc) return rc;
    export_mapmatch_stats(ms, match_stats);
    copy_stats(st, stats);
    if (n_pt_removed) *n_pt_removed = cs.points_removed;
    if (n_ln_removed) *n_ln_removed = cs.lines_removed;
    return PLBA_OK;
}

int plslam_set_mapassoc_fn(plslam_map *m, plslam_mapassoc_fn fn, void *user) { return set_hook(m, &MapHandler::setMapAssocFn, fn, user); }

int plslam_map_assoc_cpu(void *user, const plba_mapassoc_batch *b, const plba_mapassoc_params *p, const plba_mapassoc_out *out) {
    (void)user;
    return mapAssocCpu(b, p, out);
}

int plslam_grid_match_cpu(void *user, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches) {
    (void)user;
    return gridMatchCpu(b, matches_12, n_matches);
}

int plslam_set_keyframe_stereo(plslam_map *m, int32_t kf_idx, const plslam_stereo_frame *frame,
                               const plba_stereo_params *params, int32_t *pt_src, int32_t *ls_src,
                               plslam_stereo_stats *stats) {
    if (!m || !frame || !params) return PLBA_E_INVALID;
    const StereoInput in{frame->desc_bytes, frame->n_pt_l, frame->n_pt_r, frame->n_ls_l, frame->n_ls_r, 0,
                         frame->pt_l, frame->pt_r, frame->pdesc_l, frame->pdesc_r,
                         frame->ls_l, frame->ls_r, frame->ldesc_l, frame->ldesc_r};
    StereoStats st;
    const int rc = m->mh.setKeyframeStereo(kf_idx, in, *params, pt_src, ls_src, &st);
    if (rc) return rc;
    if (stats) *stats = plslam_stereo_stats{st.n_pt, st.n_ls, st.ms};
    return PLBA_OK;
}

int plslam_set_stereo_fn(plslam_map *m, plslam_stereo_fn fn, void *user) { return set_hook(m, &MapHandler::setStereoFn, fn, user); }

int plslam_stereo_cpu(void *user, const plba_stereo_batch *b, const plba_stereo_params *p, const plba_stereo_out *out) {
    (void)user;
    return stereoCpu(b, p, out);
}

int plslam_track_pose_cpu(void *user, const plba_track_batch *b, const plba_track_params *p, plba_track_out *out,
                          uint8_t *pt_inlier, uint8_t *ln_inlier) {
    (void)user;
    return trackPoseCpu(b, p, out, pt_inlier, ln_inlier);
}

int plslam_track_frames_cpu(void *user, const plba_frames_batch *b, const plba_frames_params *p, const plba_frames_out *out) {
    (void)user;
    return trackFramesCpu(b, p, out);
}

int plslam_set_keyframe_line_pluker(plslam_map *m, int32_t kf_idx, const double *NDc) {
    if (!m || !slot_ok(m->mh.map_keyframes, kf_idx)) return PLBA_E_INVALID;
    StereoFrame &f = m->mh.map_keyframes[kf_idx]->stereo_frame;
    const size_t nl = f.stereo_ls_idx.size();
    if (nl && !NDc) return PLBA_E_INVALID;
    f.ls_NDc.assign(NDc, NDc + (nl ? 6 * nl : 0));
    f.has_pluker = true;
    return PLBA_OK;
}

namespace {
void export_kfmatch_stats(const KfMatchStats &s, plslam_kfmatch_stats *o) {
    if (!o) return;
    for (int k = 0; k < 2; ++k) {
        o->grid_matches[k] = s.grid_matches[k]; o->fallback[k] = s.fallback[k]; o->matches[k] = s.matches[k];
        o->created[k] = s.created[k]; o->extended[k] = s.extended[k]; o->rejected[k] = s.rejected[k];
    }
    o->n_pairs[0] = (int32_t)s.pt_pairs.size();
    o->n_pairs[1] = (int32_t)s.ls_pairs.size();
    for (int i = 0; o->pt_pairs && i < o->pt_cap && i < o->n_pairs[0]; ++i) {
        o->pt_pairs[2 * i] = s.pt_pairs[i][0];
        o->pt_pairs[2 * i + 1] = s.pt_pairs[i][1];
    }
    for (int i = 0; o->ls_pairs && i < o->ls_cap && i < o->n_pairs[1]; ++i) {
        o->ls_pairs[2 * i] = s.ls_pairs[i][0];
        o->ls_pairs[2 * i + 1] = s.ls_pairs[i][1];
    }
    o->match_ms = s.match_ms;
}
plba_kfassoc_params kfassoc_params(const plba_kfassoc_params *p) {
    plba_kfassoc_params d;
    plba_kfassoc_default_params(&d);
    return p ? *p : d;
}
}  // namespace

int plslam_match_kf_to_kf(plslam_map *m, int32_t kf_prev_idx, int32_t kf_curr_idx, const double *DT,
                          const plba_kfassoc_params *params, plslam_kfmatch_stats *stats) {
    if (!m) return PLBA_E_INVALID;
    Mat4 T;
    if (DT) std::memcpy(T.data(), DT, sizeof(double) * 16);
    KfMatchStats st;
    const int rc = m->mh.matchKfToKf(kf_prev_idx, kf_curr_idx, DT ? &T : nullptr, kfassoc_params(params), &st);
    if (rc) return rc;
    export_kfmatch_stats(st, stats);
    return PLBA_OK;
}

int plslam_look_for_common_matches(plslam_map *m, int32_t kf_prev_idx, int32_t kf_curr_idx,
                                   const plba_kfassoc_params *kf_params, const plslam_mapmatch_params *map_params,
                                   plslam_kfmatch_stats *kf_stats, plslam_mapmatch_stats *map_stats) {
    if (!m) return PLBA_E_INVALID;
    KfMatchStats ks;
    MapMatchStats ms;
    const int rc = m->mh.lookForCommonMatches(kf_prev_idx, kf_curr_idx, kfassoc_params(kf_params), mapmatch_params(map_params), &ks, &ms);
    if (rc) return rc;
    export_kfmatch_stats(ks, kf_stats);
    export_mapmatch_stats(ms, map_stats);
    return PLBA_OK;
}

int plslam_set_kfassoc_fn(plslam_map *m, plslam_kfassoc_fn fn, void *user) { return set_hook(m, &MapHandler::setKfAssocFn, fn, user); }

int plslam_kf_assoc_cpu(void *user, const plba_kfassoc_batch *b, const plba_kfassoc_params *p, const plba_kfassoc_out *out) {
    (void)user;
    return kfAssocCpu(b, p, out);
}

int plslam_get_lc_state(plslam_map *m, int32_t *state) {
    if (!m || !state) return PLBA_E_INVALID;
    *state = m->mh.lc_state;
    return PLBA_OK;
}

int plslam_get_lc_pose_list(plslam_map *m, double *out, int32_t cap, int32_t *n) {
    if (!m) return PLBA_E_INVALID;
    const auto &l = m->mh.lc_pose_list;
    if (n) *n = (int32_t)l.size();
    for (int i = 0; i < (int)l.size() && i < cap && out; ++i)
        for (int k = 0; k < 6; ++k) out[6 * i + k] = l[i][k];
    return PLBA_OK;
}

int plslam_get_lc_feature_idxs(plslam_map *m, int32_t kind, int32_t loop, int32_t *out, int32_t cap, int32_t *n) {
    if (!m || (kind != 1 && kind != 2)) return PLBA_E_INVALID;
    const auto &ll = kind == 1 ? m->mh.lc_pt_idxs : m->mh.lc_ls_idxs;
    if (loop < 0 || loop >= (int)ll.size()) return PLBA_E_INVALID;
    const auto &l = ll[loop];
    if (n) *n = (int32_t)l.size();
    for (int i = 0; i < (int)l.size() && i < cap && out; ++i)
        for (int k = 0; k < 4; ++k) out[4 * i + k] = l[i][k];
    return PLBA_OK;
}

int plslam_set_lc_feature_idxs(plslam_map *m, int32_t kind, int32_t loop, const int32_t *rows, int32_t n) {
    if (!m || (kind != 1 && kind != 2) || loop < 0 || n < 0 || (n && !rows)) return PLBA_E_INVALID;
    if ((int)m->mh.lc_pt_idxs.size() <= loop) m->mh.lc_pt_idxs.resize((size_t)loop + 1);
    if ((int)m->mh.lc_ls_idxs.size() <= loop) m->mh.lc_ls_idxs.resize((size_t)loop + 1);
    auto &l = (kind == 1 ? m->mh.lc_pt_idxs : m->mh.lc_ls_idxs)[loop];
    l.resize((size_t)n);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 4; ++k) l[i][k] = rows[4 * i + k];
    return PLBA_OK;
}

int plslam_set_line_geometry(plslam_map *m, int32_t idx, const double line3D[6], const double med_obs_dir[3]) {
    if (!m || idx < 0 || idx >= (int)m->mh.map_lines.size() || !m->mh.map_lines[idx]) return PLBA_E_INVALID;
    MapLine *ml = m->mh.map_lines[idx];
    if (line3D) for (int k = 0; k < 6; ++k) ml->line3D[k] = line3D[k];
    if (med_obs_dir) for (int k = 0; k < 3; ++k) ml->med_obs_dir[k] = med_obs_dir[k];
    return PLBA_OK;
}

int plslam_get_line_geometry(plslam_map *m, int32_t idx, double line3D[6], double med_obs_dir[3]) {
    if (!m || idx < 0 || idx >= (int)m->mh.map_lines.size() || !m->mh.map_lines[idx]) return PLBA_E_INVALID;
    const MapLine *ml = m->mh.map_lines[idx];
    if (line3D) for (int k = 0; k < 6; ++k) line3D[k] = ml->line3D[k];
    if (med_obs_dir) for (int k = 0; k < 3; ++k) med_obs_dir[k] = ml->med_obs_dir[k];
    return PLBA_OK;
}

int plslam_set_params(plslam_map *m, int32_t min_lm_obs, int32_t min_lm_cov_graph, int32_t min_kf_local_map) {
    if (!m) return PLBA_E_INVALID;
    m->mh.params.min_lm_obs = min_lm_obs;
    m->mh.params.min_lm_cov_graph = min_lm_cov_graph;
    m->mh.params.min_kf_local_map = min_kf_local_map;
    return PLBA_OK;
}

int plslam_set_max_kf_idx(plslam_map *m, int32_t max_kf_idx) {
    if (!m) return PLBA_E_INVALID;
    m->mh.max_kf_idx = max_kf_idx;
    return PLBA_OK;
}

int plslam_kf_lines_idx_set(plslam_map *m, int32_t kf, const int32_t *lm, int32_t n) {
    if (!m || n < 0 || (n && !lm)) return PLBA_E_INVALID;
    m->mh.map_lines_kf_idx[kf].assign(lm, lm + n);
    return PLBA_OK;
}

int plslam_kf_lines_idx_get(plslam_map *m, int32_t kf, int32_t *out, int32_t cap, int32_t *n) {
    if (!m || !n) return PLBA_E_INVALID;
    auto it = m->mh.map_lines_kf_idx.find(kf);
    if (it == m->mh.map_lines_kf_idx.end()) {
        *n = -1;
        return PLBA_OK;
    }
    *n = (int32_t)it->second.size();
    for (int i = 0; out && i < *n && i < cap; ++i) out[i] = it->second[i];
    return PLBA_OK;
}

int plslam_form_local_map(plslam_map *m, int32_t kf_idx) {
    if (!m) return PLBA_E_INVALID;
    return m->mh.formLocalMap(kf_idx);
}

int plslam_remove_bad_landmarks_pluker(plslam_map *m, int32_t *n_pt_removed, int32_t *n_ln_removed) {
    if (!m) return PLBA_E_INVALID;
    CullStats cs;
    const int rc = m->mh.removeBadMapLandmarksForPluker(&cs);
    if (rc) return rc;
    if (n_pt_removed) *n_pt_removed = cs.points_removed;
    if (n_ln_removed) *n_ln_removed = cs.lines_removed;
    return PLBA_OK;
}

int plslam_local_mapping_step(plslam_map *m, int32_t kf_idx, plslam_lba_stats *stats, int32_t *n_pt_removed,
                              int32_t *n_ln_removed) {
    if (!m) return PLBA_E_INVALID;
    LbaStats st;
    CullStats cs;
    const int rc = m->mh.localMappingStep(kf_idx, &st, &cs);
    if (rc) return rc;
    copy_stats(st, stats);
    if (n_pt_removed) *n_pt_removed = cs.points_removed;
    if (n_ln_removed) *n_ln_removed = cs.lines_removed;
    return PLBA_OK;
}

int plslam_exists(plslam_map *m, int32_t kind, int32_t idx, int32_t *exists) {
    if (!m || !exists) return PLBA_E_INVALID;
    switch (kind) {
        case 0: *exists = slot_ok(m->mh.map_keyframes, idx); return PLBA_OK;
        case 1: *exists = slot_ok(m->mh.map_points, idx); return PLBA_OK;
        case 2: *exists = slot_ok(m->mh.map_lines, idx); return PLBA_OK;
        default: return PLBA_E_INVALID;
    }
}

int plslam_get_keyframe(plslam_map *m, int32_t kf_idx, double T_kf_w[16], int32_t *local, int32_t *pt_idx,
                        int32_t pt_cap, int32_t *ls_idx, int32_t ls_cap) {
    if (!m || !slot_ok(m->mh.map_keyframes, kf_idx)) return PLBA_E_INVALID;
    const KeyFrame *k = m->mh.map_keyframes[kf_idx];
    if (T_kf_w) std::memcpy(T_kf_w, k->T_kf_w.data(), sizeof(double) * 16);
    if (local) *local = k->local;
    for (int i = 0; pt_idx && i < pt_cap && i < (int)k->stereo_frame.stereo_pt_idx.size(); ++i)
        pt_idx[i] = k->stereo_frame.stereo_pt_idx[i];
    for (int i = 0; ls_idx && i < ls_cap && i < (int)k->stereo_frame.stereo_ls_idx.size(); ++i)
        ls_idx[i] = k->stereo_frame.stereo_ls_idx[i];
    return PLBA_OK;
}

int plslam_get_point(plslam_map *m, int32_t idx, double xyz[3], int32_t *inlier, int32_t *local, int32_t *n_obs,
                     int32_t *kf_obs, double *obs, double *dir, double *sigma, int32_t cap, uint8_t *med_desc,
                     double med_dir[3]) {
    if (!m || !slot_ok(m->mh.map_points, idx)) return PLBA_E_INVALID;
    const MapPoint *p = m->mh.map_points[idx];
    if (xyz) std::memcpy(xyz, p->point3D.data(), sizeof(double) * 3);
    if (inlier) *inlier = p->inlier;
    if (local) *local = p->local;
    if (n_obs) *n_obs = (int32_t)p->kf_obs_list.size();
    for (int i = 0; i < cap && i < (int)p->kf_obs_list.size(); ++i) {
        if (kf_obs) kf_obs[i] = p->kf_obs_list[i];
        if (obs) { obs[2 * i] = p->obs_list[i][0]; obs[2 * i + 1] = p->obs_list[i][1]; }
        if (dir) for (int k = 0; k < 3; ++k) dir[3 * i + k] = p->dir_list[i][k];
    }
    for (int i = 0; sigma && i < cap && i < (int)p->sigma_list.size(); ++i) sigma[i] = p->sigma_list[i];
    if (med_desc) std::memcpy(med_desc, p->med_desc.data(), p->med_desc.size());
    if (med_dir) std::memcpy(med_dir, p->med_obs_dir.data(), sizeof(double) * 3);
    return PLBA_OK;
}

int plslam_get_line(plslam_map *m, int32_t idx, double NDw[6], int32_t *inlier, int32_t *local, int32_t *n_obs,
                    int32_t *kf_obs, double *obs, double *sigma, int32_t cap, uint8_t *med_desc) {
    if (!m || !slot_ok(m->mh.map_lines, idx)) return PLBA_E_INVALID;
    const MapLine *l = m->mh.map_lines[idx];
    if (NDw) std::memcpy(NDw, l->NDw.data(), sizeof(double) * 6);
    if (inlier) *inlier = l->inlier;
    if (local) *local = l->local;
    if (n_obs) *n_obs = (int32_t)l->kf_obs_list.size();
    for (int i = 0; i < cap && i < (int)l->kf_obs_list.size(); ++i) {
        if (kf_obs) kf_obs[i] = l->kf_obs_list[i];
        if (obs) for (int k = 0; k < 4; ++k) obs[4 * i + k] = l->NDw_obs_list[i][k];
    }
    for (int i = 0; sigma && i < cap && i < (int)l->sigma_list.size(); ++i) sigma[i] = l->sigma_list[i];
    if (med_desc) std::memcpy(med_desc, l->med_desc.data(), l->med_desc.size());
    return PLBA_OK;
}

void plslam_pluker_to_orth(const double NDw[6], double orth[4]) {
    Vec6 L;
    std::memcpy(L.data(), NDw, sizeof(double) * 6);
    const Vec4 o = MapLine::changePlukerToOrth(L);
    std::memcpy(orth, o.data(), sizeof(double) * 4);
}

void plslam_orth_to_pluker(const double orth[4], double NDw[6]) {
    const Vec4 o{orth[0], orth[1], orth[2], orth[3]};
    const Vec6 L = MapLine::changeOrthToPluker(o);
    std::memcpy(NDw, L.data(), sizeof(double) * 6);
}

}  // extern "C"
