// The map-to-keyframe association of the local-mapping loop around one association call:
// MapHandler::matchMapToKfAssoc, which gathers the candidate landmarks and the keyframe's unmatched
// features, runs plba_map_associate (or the hook) and then walks the rows in order as
// MapHandler::matchMap2KFPoints / Lines (src/mapHandler.cpp:766-794, :881-918) walk them; and mapAssocCpu, a
// single-threaded restatement of plba_map_associate's semantics (include/plba.h) with the hook's
// signature, for the tests and tools/mapassoc_bench.py (not a product path). The restatement does what the
// reference does: it compacts the visible landmarks, matches the compacted list and maps the indices back.
// The arithmetic is that of csrc/plba_mapassoc_geom.hpp; this file is compiled without contraction.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../csrc/plba_mapassoc_geom.hpp"
#include "plslam_map.hpp"

namespace plslam {

int mapAssocCpu(const plba_mapassoc_batch *b, const plba_mapassoc_params *pp, const plba_mapassoc_out *out) {
    using namespace plba;
    if (!b || b->n < 0) return PLBA_E_INVALID;
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    // what plba_map_associate refuses is refused here
    if (n > (INT32_MAX - 1) / 2) return PLBA_E_INVALID;
    if (b->desc_bytes < 4 || b->desc_bytes > 64 || b->desc_bytes % 4) return PLBA_E_INVALID;
    if (!pp || !out || !out->n_visible || !out->n_grid || !out->n_matches || !out->fallback || !out->n_accepted ||
        !b->pt_off_m || !b->pt_off_f || !b->ls_off_m || !b->ls_off_f || !b->Twf || !b->T_kf_w)
        return PLBA_E_INVALID;
    const plba_mapassoc_params &prm = *pp;
    if (prm.cols <= 0 || prm.rows <= 0 || prm.width <= 0 || prm.height <= 0 || prm.ws < 0 || prm.ws >= (1 << 30))
        return PLBA_E_INVALID;
    const int32_t *const offs[2][2] = {{b->pt_off_m, b->pt_off_f}, {b->ls_off_m, b->ls_off_f}};
    for (int kd = 0; kd < 2; ++kd)
        for (int sd = 0; sd < 2; ++sd) {
            const int32_t *off = offs[kd][sd];
            if (off[0] < 0) return PLBA_E_INVALID;
            for (int f = 0; f < n; ++f)
                if (off[f + 1] < off[f] || off[f + 1] - off[f] > (sd ? 65535 : 65535 * kDmNT)) return PLBA_E_INVALID;
        }
    const bool have[2][2] = {{offs[0][0][n] > offs[0][0][0], offs[0][1][n] > offs[0][1][0]},
                             {offs[1][0][n] > offs[1][0][0], offs[1][1][n] > offs[1][1][0]}};
    if ((have[0][0] && (!b->pt_X || !b->pdesc_m)) || (have[0][1] && (!b->pt_pl || !b->pt_P || !b->pdesc_f)) ||
        (have[1][0] && (!b->ls_X || !b->ldesc_m)) ||
        (have[1][1] && (!b->ls_spl || !b->ls_epl || !b->ls_le || !b->ls_sP || !b->ls_eP || !b->ldesc_f)))
        return PLBA_E_INVALID;
    for (size_t e = 0; e < 12 * (size_t)n; ++e)
        if (!std::isfinite(b->Twf[e])) return PLBA_E_INVALID;
    for (size_t e = 0; e < 16 * (size_t)n; ++e)
        if (!std::isfinite(b->T_kf_w[e])) return PLBA_E_INVALID;
    const double *const fcoords[3] = {b->pt_pl, b->ls_spl, b->ls_epl};
    for (int k = 0; k < 3; ++k) {
        const int kd = k ? 1 : 0;
        for (size_t e = 2 * (size_t)offs[kd][1][0]; e < 2 * (size_t)offs[kd][1][n]; ++e) {
            const double v = fcoords[k][e], size = (e & 1) ? prm.height : prm.width;
            if (!(v >= -size && v <= 2.0 * size)) return PLBA_E_INVALID;
        }
    }
    const int db = b->desc_bytes, stride = std::max(prm.cols, prm.rows), max_steps = st_max_steps(prm.cols, prm.rows);
    const double inv_w = prm.cols / (double)prm.width, inv_h = prm.rows / (double)prm.height;
    std::vector<int32_t> row, cell1, cell1e, cell_off2, cells2, m12, fm, line(2 * (size_t)stride);
    std::vector<uint8_t> desc1;
    std::vector<double> dir2;
    for (int f = 0; f < n; ++f)
        for (int kd = 0; kd < 2; ++kd) {
            const int p = 2 * f + kd;
            const int a1 = offs[kd][0][f], n1 = offs[kd][0][f + 1] - a1, a2 = offs[kd][1][f], n2 = offs[kd][1][f + 1] - a2;
            const double *Twf = b->Twf + 12 * (size_t)f, *T_kf_w = b->T_kf_w + 16 * (size_t)f;
            const uint8_t *d1 = kd ? b->ldesc_m : b->pdesc_m, *d2 = kd ? b->ldesc_f : b->pdesc_f;
            d2 = n2 ? d2 + (size_t)db * a2 : nullptr;
            // :710-723, :812-828: the visible landmarks, compacted in map order
            row.clear(); cell1.clear(); cell1e.clear(); desc1.clear();
            for (int i = 0; i < n1; ++i) {
                const size_t r = (size_t)a1 + i;
                double uv[2], uve[2] = {0, 0};
                bool vis;
                int32_t c[2], ce[2] = {0, 0};
                if (kd) {
                    const bool vs = ma_project(prm, Twf, b->ls_X + 6 * r, uv), ve = ma_project(prm, Twf, b->ls_X + 6 * r + 3, uve);
                    vis = vs && ve;
                    ma_cell(vis, uve, inv_w, inv_h, ce);
                } else {
                    vis = ma_project(prm, Twf, b->pt_X + 3 * r, uv);
                }
                ma_cell(vis, uv, inv_w, inv_h, c);
                if (uint8_t *ov = kd ? out->ls_visible : out->pt_visible) ov[r] = vis;
                if (!vis) continue;
                row.push_back(i);
                cell1.insert(cell1.end(), {c[0], c[1]});
                cell1e.insert(cell1e.end(), {ce[0], ce[1]});
                desc1.insert(desc1.end(), d1 + (size_t)db * r, d1 + (size_t)db * (r + 1));
            }
            const int nv = (int)row.size();
            m12.assign((size_t)nv + 1, -1);
            int32_t grid_matches = 0;
            const int32_t off1[2] = {0, nv}, off2[2] = {0, n2}, kind = kd;
            if (prm.fast_matching && nv && n2) {  // :743-757, :848-872
                cell_off2.assign(1, 0);
                cells2.clear();
                dir2.assign(2 * (size_t)n2, 0.0);
                for (int i = 0; i < n2; ++i) {
                    const size_t r = (size_t)a2 + i;
                    if (kd) {
                        const double *s = b->ls_spl + 2 * r, *e = b->ls_epl + 2 * r;
                        kf_line_dir(s, e, inv_w, inv_h, &dir2[2 * (size_t)i]);
                        const int k = st_line_cells(s[0] * inv_w, s[1] * inv_h, e[0] * inv_w, e[1] * inv_h, prm.cols, prm.rows,
                                                    max_steps, line.data(), stride);
                        cells2.insert(cells2.end(), line.begin(), line.begin() + 2 * k);
                    } else {
                        const double gx = b->pt_pl[2 * r] * inv_w, gy = b->pt_pl[2 * r + 1] * inv_h;
                        cells2.insert(cells2.end(), {(int32_t)gx, (int32_t)gy});
                    }
                    cell_off2.push_back((int32_t)(cells2.size() / 2));
                }
                plba_gridmatch_batch g{};
                g.n = 1; g.desc_bytes = db; g.cols = prm.cols; g.rows = prm.rows; g.best_lr = prm.best_lr ? 1 : 0;
                g.off1 = off1; g.off2 = off2; g.desc1 = desc1.data(); g.desc2 = d2;
                g.cell1 = cell1.data(); g.cell1_end = cell1e.data(); g.cell_off2 = cell_off2.data(); g.cells2 = cells2.data();
                g.dir2 = dir2.data(); g.kind = &kind; g.ws = &prm.ws; g.nnr = &prm.min_ratio_12_p; g.line_sim_th = &prm.line_sim_th;
                if (const int rc = gridMatchCpu(&g, m12.data(), &grid_matches)) return rc;
            }
            const int min_matches = kd ? prm.min_ls_matches : prm.min_pt_matches;
            const bool fallback = nv > min_matches && grid_matches < min_matches;  // :759-761, :874-876
            if (fallback) {  // its result stands alone
                const float nnr = (float)(kd ? prm.min_ratio_12_l : prm.min_ratio_12_p);
                const plba_match_batch mb{1, db, off1, off2, desc1.data(), d2, &nnr, prm.best_lr ? 1 : 0, 0};
                fm.assign((size_t)nv + 1, -1);
                int32_t cnt = 0;
                if (const int rc = descMatchCpu(&mb, fm.data(), &cnt)) return rc;
                m12.swap(fm);
            }
            // the rows back at their own index: the epipolar test and the record of each match
            int accepted = 0;
            for (int i1 = 0, v = 0; i1 < n1; ++i1) {
                const size_t r1 = (size_t)a1 + i1;
                const bool vis = v < nv && row[v] == i1;
                const int i2 = vis ? m12[v] : -1;
                v += vis;
                double rec[kMaLsDoubles] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                bool ok = false;
                if (i2 >= 0) {
                    const size_t r2 = (size_t)a2 + i2;
                    if (kd) {
                        double t[kMaTLsDoubles];
                        std::copy(b->ls_spl + 2 * r2, b->ls_spl + 2 * r2 + 2, t);
                        std::copy(b->ls_epl + 2 * r2, b->ls_epl + 2 * r2 + 2, t + 2);
                        std::copy(b->ls_le + 3 * r2, b->ls_le + 3 * r2 + 3, t + 4);
                        std::copy(b->ls_sP + 3 * r2, b->ls_sP + 3 * r2 + 3, t + 7);
                        std::copy(b->ls_eP + 3 * r2, b->ls_eP + 3 * r2 + 3, t + 10);
                        ok = ma_line(prm, Twf, T_kf_w, b->ls_X + 6 * r1, t, rec);
                    } else {
                        const double t[kMaTPtDoubles] = {b->pt_pl[2 * r2], b->pt_pl[2 * r2 + 1], b->pt_P[3 * r2], b->pt_P[3 * r2 + 1],
                                                         b->pt_P[3 * r2 + 2]};
                        ok = ma_point(prm, Twf, T_kf_w, b->pt_X + 3 * r1, t, rec);
                    }
                }
                accepted += ok;
                if (kd) {
                    if (out->ls_m12) out->ls_m12[r1] = i2;
                    if (out->ls_accepted) out->ls_accepted[r1] = ok;
                    if (out->ls_rec) std::copy(rec, rec + kMaLsDoubles, out->ls_rec + kMaLsDoubles * r1);
                } else {
                    if (out->pt_m12) out->pt_m12[r1] = i2;
                    if (out->pt_accepted) out->pt_accepted[r1] = ok;
                    if (out->pt_rec) std::copy(rec, rec + kMaPtDoubles, out->pt_rec + kMaPtDoubles * r1);
                }
            }
            out->n_visible[p] = nv;
            out->n_grid[p] = grid_matches;
            out->fallback[p] = fallback ? 1 : 0;
            out->n_matches[p] = out->n_accepted[p] = accepted;  // :793, :917
        }
    return PLBA_OK;
}

int MapHandler::matchMapToKfAssoc(int kf_idx, const Mat4 *Twf_in, const plba_mapassoc_params &p_in, MapMatchStats *stats) {
    MapMatchStats st;
    if (kf_idx < 0 || kf_idx >= (int)map_keyframes.size() || !map_keyframes[kf_idx]) {
        setError("matchMapToKfAssoc: no keyframe %d", kf_idx);
        return PLBA_E_INVALID;
    }
    KeyFrame *kf = map_keyframes[kf_idx];
    StereoFrame &f = kf->stereo_frame;
    const int np = (int)f.stereo_pt_idx.size(), nl = (int)f.stereo_ls_idx.size();
    if (!f.has_features || (nl && !f.has_endpoints)) {
        setError("matchMapToKfAssoc: keyframe %d has no features (or no line endpoints)", kf_idx);
        return PLBA_E_INVALID;
    }
    plba_mapassoc_params p = p_in;
    if (p.width == 0 && p.height == 0) {  // the camera of setCamera
        p.width = width_; p.height = height_; p.fx = fx_; p.fy = fy_; p.cx = cx_; p.cy = cy_;
    }
    if (p.width <= 0 || p.height <= 0) {
        setError("matchMapToKfAssoc: the image size is not set");
        return PLBA_E_INVALID;
    }
    if (p.ws < 0 || kf_idx >= (int)full_graph.size()) {
        setError("matchMapToKfAssoc: window %d, or keyframe %d outside full_graph", p.ws, kf_idx);
        return PLBA_E_INVALID;
    }
    const Mat4 Twf = Twf_in ? *Twf_in : inverse4(kf->T_kf_w);
    const int db = f.desc_bytes, ng = (int)full_graph.size();
    auto obs_ok = [&](const std::vector<int> &kfs) {
        for (int o : kfs)
            if (o < 0 || o >= ng || (int)full_graph[o].size() < ng) return false;
        return true;
    };

    // the candidates (:712, :813) and the unmatched features (:728-734, :833-839), in the reference's order
    std::vector<MapPoint *> cand_pt;
    std::vector<MapLine *> cand_ls;
    std::vector<int> um_pt, um_ls;
    std::vector<double> pt_X, ls_X, pt_pl, pt_P, ls_spl, ls_epl, ls_le, ls_sP, ls_eP;
    std::vector<uint8_t> pdesc_m, ldesc_m, pdesc_f, ldesc_f;
    if (np) {
        for (MapPoint *pt : map_points) {
            if (!pt || !pt->local || pt->kf_obs_list.empty() || pt->kf_obs_list.back() == kf_idx) continue;
            if ((int)pt->med_desc.size() != db || !obs_ok(pt->kf_obs_list)) {
                setError("matchMapToKfAssoc: point %d has a descriptor of %zu bytes or an observer outside full_graph", pt->idx,
                         pt->med_desc.size());
                return PLBA_E_INVALID;
            }
            cand_pt.push_back(pt);
            pt_X.insert(pt_X.end(), pt->point3D.begin(), pt->point3D.end());
            pdesc_m.insert(pdesc_m.end(), pt->med_desc.begin(), pt->med_desc.end());
        }
        for (int i = 0; i < np; ++i)
            if (f.stereo_pt_idx[i] == -1) {
                um_pt.push_back(i);
                pt_pl.insert(pt_pl.end(), &f.pt_pl[2 * i], &f.pt_pl[2 * i] + 2);
                pt_P.insert(pt_P.end(), &f.pt_P[3 * i], &f.pt_P[3 * i] + 3);
                pdesc_f.insert(pdesc_f.end(), &f.pdesc_l[(size_t)i * db], &f.pdesc_l[(size_t)i * db] + db);
            }
    }
    if (nl) {
        for (MapLine *ls : map_lines) {
            if (!ls || !ls->local || ls->kf_obs_list.empty() || ls->kf_obs_list.back() == kf_idx) continue;
            if ((int)ls->med_desc.size() != db || !obs_ok(ls->kf_obs_list)) {
                setError("matchMapToKfAssoc: line %d has a descriptor of %zu bytes or an observer outside full_graph", ls->idx,
                         ls->med_desc.size());
                return PLBA_E_INVALID;
            }
            cand_ls.push_back(ls);
            ls_X.insert(ls_X.end(), ls->line3D.begin(), ls->line3D.end());
            ldesc_m.insert(ldesc_m.end(), ls->med_desc.begin(), ls->med_desc.end());
        }
        for (int i = 0; i < nl; ++i)
            if (f.stereo_ls_idx[i] == -1) {
                um_ls.push_back(i);
                ls_spl.insert(ls_spl.end(), &f.ls_spl[2 * i], &f.ls_spl[2 * i] + 2);
                ls_epl.insert(ls_epl.end(), &f.ls_epl[2 * i], &f.ls_epl[2 * i] + 2);
                ls_le.insert(ls_le.end(), &f.ls_le[3 * i], &f.ls_le[3 * i] + 3);
                ls_sP.insert(ls_sP.end(), &f.ls_sP[3 * i], &f.ls_sP[3 * i] + 3);
                ls_eP.insert(ls_eP.end(), &f.ls_eP[3 * i], &f.ls_eP[3 * i] + 3);
                ldesc_f.insert(ldesc_f.end(), &f.ldesc_l[(size_t)i * db], &f.ldesc_l[(size_t)i * db] + db);
            }
    }
    const int n1p = (int)cand_pt.size(), n1l = (int)cand_ls.size(), n2p = (int)um_pt.size(), n2l = (int)um_ls.size();
    st.unmatched[0] = n2p;
    st.unmatched[1] = n2l;

    const int32_t po_m[2] = {0, n1p}, po_f[2] = {0, n2p}, lo_m[2] = {0, n1l}, lo_f[2] = {0, n2l};
    plba_mapassoc_batch b{};
    b.n = 1; b.desc_bytes = db;
    b.pt_off_m = po_m; b.pt_off_f = po_f; b.ls_off_m = lo_m; b.ls_off_f = lo_f;
    b.Twf = Twf.data(); b.T_kf_w = kf->T_kf_w.data();
    b.pt_X = pt_X.data(); b.pdesc_m = pdesc_m.data(); b.ls_X = ls_X.data(); b.ldesc_m = ldesc_m.data();
    b.pt_pl = pt_pl.data(); b.pt_P = pt_P.data(); b.pdesc_f = pdesc_f.data();
    b.ls_spl = ls_spl.data(); b.ls_epl = ls_epl.data(); b.ls_le = ls_le.data(); b.ls_sP = ls_sP.data(); b.ls_eP = ls_eP.data();
    b.ldesc_f = ldesc_f.data();
    int32_t n_visible[2] = {0, 0}, n_grid[2] = {0, 0}, n_matches[2] = {0, 0}, fallback[2] = {0, 0}, n_accepted[2] = {0, 0};
    std::vector<int32_t> pt_m12((size_t)n1p + 1, -1), ls_m12((size_t)n1l + 1, -1);
    std::vector<uint8_t> pt_vis((size_t)n1p + 1, 0), ls_vis((size_t)n1l + 1, 0), pt_acc((size_t)n1p + 1, 0), ls_acc((size_t)n1l + 1, 0);
    std::vector<double> pt_rec(plba::kMaPtDoubles * (size_t)n1p + 1), ls_rec(plba::kMaLsDoubles * (size_t)n1l + 1);
    plba_mapassoc_out o{n_visible, n_grid, n_matches, fallback, n_accepted, pt_vis.data(), pt_m12.data(), pt_acc.data(),
                        pt_rec.data(), ls_vis.data(), ls_m12.data(), ls_acc.data(), ls_rec.data()};
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = backend(mapassoc_, "map association", [&](plba_ctx *ctx) { return plba_map_associate(ctx, &b, &p, &o); },
                           &b, &p, &o);
    if (rc) return rc;
    st.match_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int i1 = 0; i1 < n1p + n1l; ++i1) {  // what a hook returns is checked before the map changes
        const bool pt = i1 < n1p;
        const int r = pt ? i1 : i1 - n1p, v = pt ? pt_m12[r] : ls_m12[r], lim = pt ? n2p : n2l;
        if (v < -1 || v >= lim || (v < 0 && (pt ? pt_acc[r] : ls_acc[r]))) {
            setError("matchMapToKfAssoc: match %d of row %d is outside its %d features, or accepted without a match", v, i1, lim);
            return PLBA_E_INVALID;
        }
    }
    for (int k = 0; k < 2; ++k) {
        const int n2 = k ? n2l : n2p;
        st.visible[k] = n_visible[k];
        st.grid_matches[k] = n_grid[k];
        st.fallback[k] = (fallback[k] && n2 > 0) ? 1 : 0;  // :736, :841: the reference returns before it matches
    }

    auto bump_graph = [&](const std::vector<int> &kfs) {  // :786-791, :910-915
        for (int obs : kfs)
            if (obs != kf_idx) {
                full_graph[kf_idx][obs]++;
                full_graph[obs][kf_idx]++;
            }
    };
    for (int i1 = 0; i1 < n1p; ++i1) {  // :766-794
        const int i2 = pt_m12[i1];
        if (i2 < 0) continue;
        if (!pt_acc[i1]) {
            ++st.rejected[0];
            continue;
        }
        MapPoint *pt = cand_pt[i1];
        const int fi = um_pt[i2];
        const double *r = &pt_rec[plba::kMaPtDoubles * (size_t)i1];
        f.stereo_pt_idx[fi] = pt->idx;
        pt->addMapPointObservation(Desc(&f.pdesc_l[(size_t)fi * db], &f.pdesc_l[(size_t)fi * db] + db), kf_idx,
                                   Vec2{f.pt_pl[2 * fi], f.pt_pl[2 * fi + 1]}, Vec3{r[3], r[4], r[5]}, 1.0);
        bump_graph(pt->kf_obs_list);
        ++st.accepted[0];
    }
    for (int i1 = 0; i1 < n1l; ++i1) {  // :881-918
        const int i2 = ls_m12[i1];
        if (i2 < 0) continue;
        if (!ls_acc[i1]) {
            ++st.rejected[1];
            continue;
        }
        MapLine *ls = cand_ls[i1];
        const int fi = um_ls[i2];
        f.stereo_ls_idx[fi] = ls->idx;
        ls->addMapLineObservation(Desc(&f.ldesc_l[(size_t)fi * db], &f.ldesc_l[(size_t)fi * db] + db), kf_idx,
                                  Vec4{f.ls_spl[2 * fi], f.ls_spl[2 * fi + 1], f.ls_epl[2 * fi], f.ls_epl[2 * fi + 1]}, 1.0);
        bump_graph(ls->kf_obs_list);
        ++st.accepted[1];
    }
    if (stats) *stats = st;
    return PLBA_OK;
}

int MapHandler::localMappingStepKfAssoc(int kf_idx, const plba_mapassoc_params &p, MapMatchStats *ms, LbaStats *stats, CullStats *cs) {
    const int rc = matchMapToKfAssoc(kf_idx, nullptr, p, ms);
    if (rc) return rc;
    return localMappingStep(kf_idx, stats, cs);
}

}  // namespace plslam
