// The keyframe-to-keyframe association of the local-mapping loop, MapHandler::matchKF2KFPoints / Lines
// (src/mapHandler.cpp:237-366, :368-590, the USE_LINE_PLUKER branch): MapHandler::matchKfToKf, which runs
// plba_kf_associate (or the hook) on a keyframe pair and then walks the rows in order, creating and
// extending the map's landmarks; lookForCommonMatches (:923-990 without the refinement); and kfAssocCpu, a
// single-threaded restatement of plba_kf_associate's semantics (include/plba.h) with the hook's signature,
// for the tests and tools/kfassoc_bench.py (not a product path). The arithmetic is that of
// csrc/plba_kfassoc_geom.hpp; this file is compiled without contraction.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/plba_kfassoc_geom.hpp"
#include "plslam_map.hpp"

namespace plslam {

int kfAssocCpu(const plba_kfassoc_batch *b, const plba_kfassoc_params *pp, const plba_kfassoc_out *out) {
    using namespace plba;
    if (!b || b->n < 0) return PLBA_E_INVALID;
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    // what plba_kf_associate refuses is refused here
    if (n > (INT32_MAX - 1) / 2) return PLBA_E_INVALID;
    if (b->desc_bytes < 4 || b->desc_bytes > 64 || b->desc_bytes % 4) return PLBA_E_INVALID;
    if (!pp || !out || !out->n_grid || !out->n_matches || !out->fallback || !b->pt_off_p || !b->pt_off_c || !b->ls_off_p ||
        !b->ls_off_c || !b->DT || !b->T_prev || !b->T_curr || !b->Tcw_prev || !b->Tcw_curr)
        return PLBA_E_INVALID;
    const plba_kfassoc_params &prm = *pp;
    if (prm.cols <= 0 || prm.rows <= 0 || prm.width <= 0 || prm.height <= 0 || prm.ws < 0 || prm.ws >= (1 << 30))
        return PLBA_E_INVALID;
    const int32_t *const offs[2][2] = {{b->pt_off_p, b->pt_off_c}, {b->ls_off_p, b->ls_off_c}};
    for (int kd = 0; kd < 2; ++kd)
        for (int sd = 0; sd < 2; ++sd) {
            const int32_t *off = offs[kd][sd];
            if (off[0] < 0) return PLBA_E_INVALID;
            for (int f = 0; f < n; ++f)
                if (off[f + 1] < off[f] || (sd && off[f + 1] - off[f] > 65535)) return PLBA_E_INVALID;
        }
    const bool have[2][2] = {{offs[0][0][n] > offs[0][0][0], offs[0][1][n] > offs[0][1][0]},
                             {offs[1][0][n] > offs[1][0][0], offs[1][1][n] > offs[1][1][0]}};
    if ((have[0][0] && (!b->pt_P_p || !b->pdesc_p)) || (have[0][1] && (!b->pt_pl_c || !b->pt_P_c || !b->pdesc_c)) ||
        (have[1][0] && (!b->ls_sP_p || !b->ls_eP_p || !b->ls_NDc_p || !b->ls_spl_p || !b->ls_epl_p || !b->ldesc_p ||
                        !b->ls_lm_NDw || !b->ls_new)) ||
        (have[1][1] && (!b->ls_spl_c || !b->ls_epl_c || !b->ldesc_c)))
        return PLBA_E_INVALID;
    const double *const poses[5] = {b->DT, b->T_prev, b->T_curr, b->Tcw_prev, b->Tcw_curr};
    for (int k = 0; k < 5; ++k)
        for (size_t e = 0; e < (size_t)n * (k ? 16 : 12); ++e)
            if (!std::isfinite(poses[k][e])) return PLBA_E_INVALID;
    const double *const ccoords[3] = {b->pt_pl_c, b->ls_spl_c, b->ls_epl_c};
    for (int k = 0; k < 3; ++k) {
        const int kd = k ? 1 : 0;
        for (size_t e = 2 * (size_t)offs[kd][1][0]; e < 2 * (size_t)offs[kd][1][n]; ++e) {
            const double v = ccoords[k][e], size = (e & 1) ? prm.height : prm.width;
            if (!(v >= -size && v <= 2.0 * size)) return PLBA_E_INVALID;
        }
    }
    const int db = b->desc_bytes, stride = std::max(prm.cols, prm.rows), max_steps = st_max_steps(prm.cols, prm.rows);
    const double inv_w = prm.cols / (double)prm.width, inv_h = prm.rows / (double)prm.height;
    std::vector<int32_t> cell1, cell1e, cell_off2, cells2, m12, fm, line(2 * (size_t)stride);
    std::vector<double> dir2;
    for (int f = 0; f < n; ++f)
        for (int kd = 0; kd < 2; ++kd) {
            const int p = 2 * f + kd;
            const int a1 = offs[kd][0][f], n1 = offs[kd][0][f + 1] - a1, a2 = offs[kd][1][f], n2 = offs[kd][1][f + 1] - a2;
            const double *DT = b->DT + 12 * (size_t)f, *T_prev = b->T_prev + 16 * (size_t)f, *T_curr = b->T_curr + 16 * (size_t)f,
                         *Tcw_prev = b->Tcw_prev + 16 * (size_t)f, *Tcw_curr = b->Tcw_curr + 16 * (size_t)f;
            const uint8_t *d1 = kd ? b->ldesc_p : b->pdesc_p, *d2 = kd ? b->ldesc_c : b->pdesc_c;
            d1 = n1 ? d1 + (size_t)db * a1 : nullptr;
            d2 = n2 ? d2 + (size_t)db * a2 : nullptr;
            m12.assign((size_t)n1 + 1, -1);
            int32_t grid_matches = 0;
            const int32_t off1[2] = {0, n1}, off2[2] = {0, n2}, kind = kd;
            if (prm.fast_matching && n1 && n2) {  // :253-275, :384-422
                cell1.assign(2 * (size_t)n1, 0);
                cell1e.assign(2 * (size_t)n1, 0);
                for (int i = 0; i < n1; ++i) {
                    const size_t r = (size_t)a1 + i;
                    if (kd) {
                        kf_line_cell(prm, DT, b->ls_sP_p + 3 * r, inv_w, inv_h, &cell1[2 * i]);
                        kf_line_cell(prm, DT, b->ls_eP_p + 3 * r, inv_w, inv_h, &cell1e[2 * i]);
                    } else {
                        kf_point_cell(prm, DT, b->pt_P_p + 3 * r, inv_w, inv_h, &cell1[2 * i]);
                    }
                }
                cell_off2.assign(1, 0);
                cells2.clear();
                dir2.assign(2 * (size_t)n2, 0.0);
                for (int i = 0; i < n2; ++i) {
                    const size_t r = (size_t)a2 + i;
                    if (kd) {
                        const double *s = b->ls_spl_c + 2 * r, *e = b->ls_epl_c + 2 * r;
                        kf_line_dir(s, e, inv_w, inv_h, &dir2[2 * (size_t)i]);
                        const int k = st_line_cells(s[0] * inv_w, s[1] * inv_h, e[0] * inv_w, e[1] * inv_h, prm.cols, prm.rows,
                                                    max_steps, line.data(), stride);
                        cells2.insert(cells2.end(), line.begin(), line.begin() + 2 * k);
                    } else {
                        const double gx = b->pt_pl_c[2 * r] * inv_w, gy = b->pt_pl_c[2 * r + 1] * inv_h;
                        cells2.insert(cells2.end(), {(int32_t)gx, (int32_t)gy});
                    }
                    cell_off2.push_back((int32_t)(cells2.size() / 2));
                }
                plba_gridmatch_batch g{};
                g.n = 1; g.desc_bytes = db; g.cols = prm.cols; g.rows = prm.rows; g.best_lr = prm.best_lr ? 1 : 0;
                g.off1 = off1; g.off2 = off2; g.desc1 = d1; g.desc2 = d2;
                g.cell1 = cell1.data(); g.cell1_end = cell1e.data(); g.cell_off2 = cell_off2.data(); g.cells2 = cells2.data();
                g.dir2 = dir2.data(); g.kind = &kind; g.ws = &prm.ws; g.nnr = &prm.min_ratio_12_p; g.line_sim_th = &prm.line_sim_th;
                if (const int rc = gridMatchCpu(&g, m12.data(), &grid_matches)) return rc;
            }
            int32_t matches = grid_matches;
            const int min_matches = kd ? prm.min_ls_matches : prm.min_pt_matches;
            const bool fallback = n2 > min_matches && n1 > min_matches && grid_matches < min_matches;  // :277-279, :424-426
            if (fallback) {  // its result stands alone
                const float nnr = (float)(kd ? prm.min_ratio_12_l : prm.min_ratio_12_p);
                const plba_match_batch mb{1, db, off1, off2, d1, d2, &nnr, prm.best_lr ? 1 : 0, 0};
                fm.assign((size_t)n1 + 1, -1);
                if (const int rc = descMatchCpu(&mb, fm.data(), &matches)) return rc;
                m12.swap(fm);
            }
            out->n_grid[p] = grid_matches;
            out->n_matches[p] = matches;
            out->fallback[p] = fallback ? 1 : 0;
            for (int i1 = 0; i1 < n1; ++i1) {
                const size_t r1 = (size_t)a1 + i1;
                const int i2 = m12[i1];
                double rec[kKfPtDoubles] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                int bit = 0;
                if (i2 >= 0) {
                    const size_t r2 = (size_t)a2 + i2;
                    if (kd) {
                        double q[kKfQLsDoubles];
                        std::copy(b->ls_sP_p + 3 * r1, b->ls_sP_p + 3 * r1 + 3, q);
                        std::copy(b->ls_eP_p + 3 * r1, b->ls_eP_p + 3 * r1 + 3, q + 3);
                        std::copy(b->ls_NDc_p + 6 * r1, b->ls_NDc_p + 6 * r1 + 6, q + 6);
                        std::copy(b->ls_spl_p + 2 * r1, b->ls_spl_p + 2 * r1 + 2, q + 12);
                        std::copy(b->ls_epl_p + 2 * r1, b->ls_epl_p + 2 * r1 + 2, q + 14);
                        std::copy(b->ls_lm_NDw + 6 * r1, b->ls_lm_NDw + 6 * r1 + 6, q + 16);
                        const double c[4] = {b->ls_spl_c[2 * r2], b->ls_spl_c[2 * r2 + 1], b->ls_epl_c[2 * r2], b->ls_epl_c[2 * r2 + 1]};
                        bit = kf_line(prm, T_prev, Tcw_prev, Tcw_curr, q, b->ls_new[r1] != 0, c, rec);
                    } else {
                        kf_point(T_prev, T_curr, b->pt_P_p + 3 * r1, b->pt_P_c + 3 * r2, rec);
                    }
                }
                if (kd) {
                    if (out->ls_m12) out->ls_m12[r1] = i2;
                    if (out->ls_rec) std::copy(rec, rec + kKfLsDoubles, out->ls_rec + kKfLsDoubles * r1);
                    if (out->ls_rejected) out->ls_rejected[r1] = (uint8_t)bit;
                } else {
                    if (out->pt_m12) out->pt_m12[r1] = i2;
                    if (out->pt_rec) std::copy(rec, rec + kKfPtDoubles, out->pt_rec + kKfPtDoubles * r1);
                }
            }
        }
    return PLBA_OK;
}

int MapHandler::matchKfToKf(int kf_prev_idx, int kf_curr_idx, const Mat4 *DT_in, const plba_kfassoc_params &p_in,
                            KfMatchStats *stats) {
    KfMatchStats st;
    const int nkf = (int)map_keyframes.size();
    if (kf_prev_idx < 0 || kf_prev_idx >= nkf || !map_keyframes[kf_prev_idx] || kf_curr_idx < 0 || kf_curr_idx >= nkf ||
        !map_keyframes[kf_curr_idx] || kf_prev_idx == kf_curr_idx) {
        setError("matchKfToKf: no keyframe %d or %d, or the same twice", kf_prev_idx, kf_curr_idx);
        return PLBA_E_INVALID;
    }
    KeyFrame *kp = map_keyframes[kf_prev_idx], *kc = map_keyframes[kf_curr_idx];
    StereoFrame &fp = kp->stereo_frame, &fc = kc->stereo_frame;
    const int np1 = (int)fp.stereo_pt_idx.size(), nl1 = (int)fp.stereo_ls_idx.size(), np2 = (int)fc.stereo_pt_idx.size(),
              nl2 = (int)fc.stereo_ls_idx.size();
    if (!fp.has_features || !fc.has_features || fp.desc_bytes != fc.desc_bytes || (nl1 && (!fp.has_endpoints || !fp.has_pluker)) ||
        (nl2 && !fc.has_endpoints)) {
        setError("matchKfToKf: keyframe %d or %d has no features, line endpoints or Pluecker lines, or another descriptor size",
                 kf_prev_idx, kf_curr_idx);
        return PLBA_E_INVALID;
    }
    plba_kfassoc_params p = p_in;
    if (p.width == 0 && p.height == 0) {  // the camera of setCamera
        p.width = width_; p.height = height_; p.fx = fx_; p.fy = fy_; p.cx = cx_; p.cy = cy_;
    }
    if (p.width <= 0 || p.height <= 0) {
        setError("matchKfToKf: the image size is not set");
        return PLBA_E_INVALID;
    }
    const int ng = (int)full_graph.size();
    if (kf_prev_idx >= ng || kf_curr_idx >= ng || (int)full_graph[kf_prev_idx].size() < ng || (int)full_graph[kf_curr_idx].size() < ng) {
        setError("matchKfToKf: keyframe %d or %d outside full_graph", kf_prev_idx, kf_curr_idx);
        return PLBA_E_INVALID;
    }
    // the landmarks the previous features carry: in range, their observers inside full_graph
    auto obs_ok = [&](const std::vector<int> &kfs) {
        for (int o : kfs)
            if (o < 0 || o >= ng || (int)full_graph[o].size() < ng) return false;
        return true;
    };
    for (int i = 0; i < np1; ++i) {
        const int idx = fp.stereo_pt_idx[i];
        if (idx < -1 || idx >= (int)map_points.size() || (idx >= 0 && map_points[idx] && !obs_ok(map_points[idx]->kf_obs_list))) {
            setError("matchKfToKf: point feature %d of keyframe %d has idx %d outside the map, or an observer outside full_graph", i,
                     kf_prev_idx, idx);
            return PLBA_E_INVALID;
        }
    }
    const size_t db = (size_t)fp.desc_bytes;
    std::vector<double> lm_NDw(6 * (size_t)nl1 + 1, 0.0);
    std::vector<uint8_t> ls_new((size_t)nl1 + 1, 0);
    for (int i = 0; i < nl1; ++i) {
        const int idx = fp.stereo_ls_idx[i];
        if (idx < -1 || idx >= (int)map_lines.size() || (idx >= 0 && map_lines[idx] && !obs_ok(map_lines[idx]->kf_obs_list))) {
            setError("matchKfToKf: line feature %d of keyframe %d has idx %d outside the map, or an observer outside full_graph", i,
                     kf_prev_idx, idx);
            return PLBA_E_INVALID;
        }
        ls_new[i] = idx == -1;
        if (idx >= 0 && map_lines[idx]) std::copy(map_lines[idx]->NDw.begin(), map_lines[idx]->NDw.end(), &lm_NDw[6 * (size_t)i]);
    }
    const Mat4 Tcw_prev = inverse4(kp->T_kf_w), Tcw_curr = inverse4(kc->T_kf_w);
    const Mat4 DT = DT_in ? *DT_in : expmap_se3(logmap_se3(mul4(Tcw_curr, kp->T_kf_w)));  // :143-145

    const int32_t po_p[2] = {0, np1}, po_c[2] = {0, np2}, lo_p[2] = {0, nl1}, lo_c[2] = {0, nl2};
    plba_kfassoc_batch b{};
    b.n = 1; b.desc_bytes = fp.desc_bytes;
    b.pt_off_p = po_p; b.pt_off_c = po_c; b.ls_off_p = lo_p; b.ls_off_c = lo_c;
    b.DT = DT.data(); b.T_prev = kp->T_kf_w.data(); b.T_curr = kc->T_kf_w.data(); b.Tcw_prev = Tcw_prev.data(); b.Tcw_curr = Tcw_curr.data();
    b.pt_P_p = fp.pt_P.data(); b.pdesc_p = fp.pdesc_l.data();
    b.ls_sP_p = fp.ls_sP.data(); b.ls_eP_p = fp.ls_eP.data(); b.ls_NDc_p = fp.ls_NDc.data(); b.ls_spl_p = fp.ls_spl.data();
    b.ls_epl_p = fp.ls_epl.data(); b.ldesc_p = fp.ldesc_l.data(); b.ls_lm_NDw = lm_NDw.data(); b.ls_new = ls_new.data();
    b.pt_pl_c = fc.pt_pl.data(); b.pt_P_c = fc.pt_P.data(); b.pdesc_c = fc.pdesc_l.data();
    b.ls_spl_c = fc.ls_spl.data(); b.ls_epl_c = fc.ls_epl.data(); b.ldesc_c = fc.ldesc_l.data();
    int32_t n_grid[2] = {0, 0}, n_matches[2] = {0, 0}, fallback[2] = {0, 0};
    std::vector<int32_t> pt_m12((size_t)np1 + 1, -1), ls_m12((size_t)nl1 + 1, -1);
    std::vector<double> pt_rec(plba::kKfPtDoubles * (size_t)np1 + 1), ls_rec(plba::kKfLsDoubles * (size_t)nl1 + 1);
    std::vector<uint8_t> rej((size_t)nl1 + 1, 0);
    plba_kfassoc_out o{n_grid, n_matches, fallback, pt_m12.data(), ls_m12.data(), pt_rec.data(), ls_rec.data(), rej.data()};
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = backend(kfassoc_, "keyframe association", [&](plba_ctx *ctx) { return plba_kf_associate(ctx, &b, &p, &o); },
                           &b, &p, &o);
    if (rc) return rc;
    st.match_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int i1 = 0; i1 < np1 + nl1; ++i1) {  // what a hook returns is checked before the map changes
        const int v = i1 < np1 ? pt_m12[i1] : ls_m12[i1 - np1], lim = i1 < np1 ? np2 : nl2;
        if (v < -1 || v >= lim) {
            setError("matchKfToKf: match %d of row %d is outside its %d features", v, i1, lim);
            return PLBA_E_INVALID;
        }
    }
    for (int k = 0; k < 2; ++k) {
        st.grid_matches[k] = n_grid[k]; st.fallback[k] = fallback[k]; st.matches[k] = n_matches[k];
    }

    auto bump_graph = [&](const std::vector<int> &kfs) {  // :347-352, :569-574
        for (int obs : kfs)
            if (obs != kf_curr_idx) {
                full_graph[kf_curr_idx][obs]++;
                full_graph[obs][kf_curr_idx]++;
            }
    };
    auto desc_row = [&](const std::vector<uint8_t> &d, int i) { return Desc(d.begin() + db * (size_t)i, d.begin() + db * (size_t)(i + 1)); };
    for (int i1 = 0; i1 < np1; ++i1) {  // :283-363
        const int i2 = pt_m12[i1];
        if (i2 < 0) continue;
        const double *r = &pt_rec[plba::kKfPtDoubles * (size_t)i1];
        const Vec2 pl2{fc.pt_pl[2 * i2], fc.pt_pl[2 * i2 + 1]};
        const Vec3 dir2{r[6], r[7], r[8]};
        if (fp.stereo_pt_idx[i1] == -1) {
            const int idx = (int)map_points.size();  // max_pt_idx
            fp.stereo_pt_idx[i1] = idx;
            fc.stereo_pt_idx[i2] = idx;
            auto *pt = new MapPoint(idx, Vec3{r[0], r[1], r[2]}, desc_row(fp.pdesc_l, i1), kf_prev_idx,
                                    Vec2{fp.pt_pl[2 * i1], fp.pt_pl[2 * i1 + 1]}, Vec3{r[3], r[4], r[5]}, 1.0);
            map_points.push_back(pt);
            adoptLandmark(1, idx);
            map_points_kf_idx[kf_prev_idx].push_back(idx);
            pt->addMapPointObservation(desc_row(fc.pdesc_l, i2), kf_curr_idx, pl2, dir2, 1.0);
            full_graph[kf_curr_idx][kf_prev_idx]++;
            full_graph[kf_prev_idx][kf_curr_idx]++;
            ++st.created[0];
        } else {
            MapPoint *pt = map_points[fp.stereo_pt_idx[i1]];
            if (!pt) continue;  // :336
            fc.stereo_pt_idx[i2] = pt->idx;
            pt->addMapPointObservation(desc_row(fc.pdesc_l, i2), kf_curr_idx, pl2, dir2, 1.0);
            bump_graph(pt->kf_obs_list);
            ++st.extended[0];
        }
        st.pt_pairs.push_back({i1, i2});
    }
    for (int i1 = 0; i1 < nl1; ++i1) {  // :434-589
        const int i2 = ls_m12[i1];
        if (i2 < 0) continue;
        const double *r = &ls_rec[plba::kKfLsDoubles * (size_t)i1];
        const Vec4 obs2{fc.ls_spl[2 * i2], fc.ls_spl[2 * i2 + 1], fc.ls_epl[2 * i2], fc.ls_epl[2 * i2 + 1]};
        if (fp.stereo_ls_idx[i1] == -1) {
            if (rej[i1]) {  // :489-494
                fc.stereo_ls_idx[i2] = -1;
                fp.stereo_ls_idx[i1] = -1;
                ++st.rejected[1];
                continue;
            }
            const int idx = (int)map_lines.size();  // max_ls_idx
            fp.stereo_ls_idx[i1] = idx;
            fc.stereo_ls_idx[i2] = idx;
            auto *ls = new MapLine(idx, Vec6{r[0], r[1], r[2], r[3], r[4], r[5]}, desc_row(fp.ldesc_l, i1), kf_prev_idx,
                                   Vec4{fp.ls_spl[2 * i1], fp.ls_spl[2 * i1 + 1], fp.ls_epl[2 * i1], fp.ls_epl[2 * i1 + 1]}, 1.0);
            map_lines.push_back(ls);
            adoptLandmark(2, idx);
            map_lines_kf_idx[kf_prev_idx].push_back(idx);
            ls->addMapLineObservation(desc_row(fc.ldesc_l, i2), kf_curr_idx, obs2, 1.0);
            full_graph[kf_curr_idx][kf_prev_idx]++;
            full_graph[kf_prev_idx][kf_curr_idx]++;
            ++st.created[1];
        } else {
            MapLine *ls = map_lines[fp.stereo_ls_idx[i1]];
            if (!ls) continue;  // :539
            if (rej[i1]) {  // :557-562
                fc.stereo_ls_idx[i2] = -1;
                ++st.rejected[1];
                continue;
            }
            fc.stereo_ls_idx[i2] = ls->idx;
            ls->addMapLineObservation(desc_row(fc.ldesc_l, i2), kf_curr_idx, obs2, 1.0);
            bump_graph(ls->kf_obs_list);
            ++st.extended[1];
        }
        st.ls_pairs.push_back({i1, i2});
    }
    if (stats) *stats = std::move(st);
    return PLBA_OK;
}

int MapHandler::lookForCommonMatches(int kf_prev_idx, int kf_curr_idx, const plba_kfassoc_params &kp, const MapMatchParams &mp,
                                     KfMatchStats *ks, MapMatchStats *ms) {
    // what matchMapToKf refuses of its own arguments is refused before the first half changes the map; the
    // keyframe, its features and full_graph are checked by matchKfToKf
    if (mp.ws < 0 || width_ <= 0 || height_ <= 0) {
        setError("lookForCommonMatches: window %d, or the image size is not set", mp.ws);
        return PLBA_E_INVALID;
    }
    const int rc = matchKfToKf(kf_prev_idx, kf_curr_idx, nullptr, kp, ks);
    if (rc) return rc;
    return matchMapToKf(kf_curr_idx, nullptr, mp, ms);  // :982-989
}

}  // namespace plslam
