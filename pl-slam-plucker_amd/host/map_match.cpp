// The map-to-keyframe association of the local-mapping loop, MapHandler::matchMap2KFPoints / Lines
// (src/mapHandler.cpp:697-921), around the grid-guided matcher (StVO::matchGrid, src2/matching.cpp:111-258,
// on the GPU as plba_grid_match); the line rasteriser that fills the grid (getLineCoords,
// src2/gridStructure.cpp:33-41); and a single-threaded matcher with the signature of the grid-matcher
// hook, for the benchmark tool and the tests (not a product path).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>

#include "plslam_map.hpp"

namespace plslam {

// Bresenham's line algorithm (IBM Systems Journal 4(1), 1965) over grid cells, as the reference's
// matching grid uses it: the axis with the larger extent is the one that advances a cell per step,
// from its smaller coordinate to its larger; the first and last cell and the start of the other axis
// are the coordinates truncated toward zero; the slack before the other axis moves is a double that
// starts at half the extent.
long lineCells(double ax, double ay, double bx, double by, std::vector<std::array<int, 2>> &out, size_t max_out) {
    out.clear();
    constexpr double kMaxCoord = 1e6;
    for (double v : {ax, ay, bx, by})
        if (!std::isfinite(v) || std::abs(v) > kMaxCoord) return -1;
    const bool by_rows = std::abs(by - ay) > std::abs(bx - ax);  // y is the stepping axis
    double u0 = by_rows ? ay : ax, v0 = by_rows ? ax : ay, u1 = by_rows ? by : bx, v1 = by_rows ? bx : by;
    if (u0 > u1) {
        std::swap(u0, u1);
        std::swap(v0, v1);
    }
    const double extent = u1 - u0, rise = std::abs(v1 - v0);
    const int first = static_cast<int>(u0), last = static_cast<int>(u1), dir = v0 < v1 ? 1 : -1;
    int v = static_cast<int>(v0);
    double slack = extent / 2.0;
    const long count = (long)last - first + 1;
    for (long k = 0; k < count && (size_t)k < max_out; ++k) {
        const int u = first + (int)k;
        out.push_back(by_rows ? std::array<int, 2>{v, u} : std::array<int, 2>{u, v});
        slack -= rise;
        if (slack < 0) {
            v += dir;
            slack += extent;
        }
    }
    return count;
}

// plba_grid_match's semantics (include/plba.h) restated as the reference runs them: the query rows
// in order, the running `distances` / `matches_21` of the columns, the candidates of a row in
// increasing train index. win: [n][4] half-widths of the window to the left, right, up and down (the stereo
// association's w.width / w.height pairs); nullptr: b->ws on all four sides.
int gridMatchCpuWin(const plba_gridmatch_batch *b, const int32_t *win, int32_t *matches_12, int32_t *n_matches) {
    if (!b || b->n < 0) return PLBA_E_INVALID;
    if (b->n == 0) return PLBA_OK;
    // what plba_grid_match refuses is refused here
    if (b->desc_bytes < 4 || b->desc_bytes > 64 || b->desc_bytes % 4 || b->cols <= 0 || b->rows <= 0) return PLBA_E_INVALID;
    if (!b->off1 || !b->off2 || !b->kind || (!win && !b->ws) || !b->nnr || !b->line_sim_th || !n_matches) return PLBA_E_INVALID;
    if (b->off1[0] < 0 || b->off2[0] < 0) return PLBA_E_INVALID;
    bool line_q = false, line_t = false;
    for (int k = 0; k < b->n; ++k) {
        if (b->off1[k + 1] < b->off1[k] || b->off2[k + 1] < b->off2[k] || (!win && b->ws[k] < 0) || (b->kind[k] != 0 && b->kind[k] != 1) ||
            b->off2[k + 1] - b->off2[k] > 65535)
            return PLBA_E_INVALID;
        line_q = line_q || (b->kind[k] == 1 && b->off1[k + 1] > b->off1[k]);
        line_t = line_t || (b->kind[k] == 1 && b->off2[k + 1] > b->off2[k]);
    }
    const size_t tn1 = (size_t)b->off1[b->n], tn2 = (size_t)b->off2[b->n];
    if ((tn1 && (!b->desc1 || !b->cell1 || !matches_12)) || (tn2 && (!b->desc2 || !b->cell_off2)) ||
        (line_q && !b->cell1_end) || (line_t && !b->dir2))
        return PLBA_E_INVALID;
    if (tn2) {
        if (b->cell_off2[0] < 0) return PLBA_E_INVALID;
        for (size_t r = 0; r < tn2; ++r)
            if (b->cell_off2[r + 1] < b->cell_off2[r]) return PLBA_E_INVALID;
        if (b->cell_off2[tn2] && !b->cells2) return PLBA_E_INVALID;
    }
    const int dw = b->desc_bytes / 4;
    std::vector<int> distances, matches_21, bx0, bx1, by0, by1;
    for (int k = 0; k < b->n; ++k) {
        const int o1 = b->off1[k], n1 = b->off1[k + 1] - o1, o2 = b->off2[k], n2 = b->off2[k + 1] - o2;
        const bool line = b->kind[k] == 1;
        int wl, wr, wu, wd;
        if (win) { wl = win[4 * k]; wr = win[4 * k + 1]; wu = win[4 * k + 2]; wd = win[4 * k + 3]; }
        else wl = wr = wu = wd = b->ws[k];
        if (wl < 0 || wr < 0 || wu < 0 || wd < 0) return PLBA_E_INVALID;
        distances.assign((size_t)n2, INT_MAX);
        matches_21.assign((size_t)n2, -1);
        // the bounding box of each train row's in-grid cells, to skip most rows without reading their cells
        bx0.assign((size_t)n2, INT_MAX); bx1.assign((size_t)n2, INT_MIN);
        by0.assign((size_t)n2, INT_MAX); by1.assign((size_t)n2, INT_MIN);
        for (int i2 = 0; i2 < n2; ++i2)
            for (int c = b->cell_off2[o2 + i2]; c < b->cell_off2[o2 + i2 + 1]; ++c) {
                const int cx = b->cells2[2 * c], cy = b->cells2[2 * c + 1];
                if (cx < 0 || cx >= b->cols || cy < 0 || cy >= b->rows) continue;
                bx0[i2] = std::min(bx0[i2], cx); bx1[i2] = std::max(bx1[i2], cx);
                by0[i2] = std::min(by0[i2], cy); by1[i2] = std::max(by1[i2], cy);
            }
        int matches = 0;
        for (int i1 = 0; i1 < n1; ++i1) {
            const int32_t *q = b->cell1 + 2 * (size_t)(o1 + i1);
            long long w[2][4];
            int nw = 1;
            auto window = [&](const int32_t *c, long long *o) {
                o[0] = std::max(0LL, (long long)c[0] - wl); o[1] = std::min((long long)b->cols, (long long)c[0] + wr + 1);
                o[2] = std::max(0LL, (long long)c[1] - wu); o[3] = std::min((long long)b->rows, (long long)c[1] + wd + 1);
            };
            window(q, w[0]);
            double vx = 0, vy = 0;
            if (line) {
                const int32_t *e = b->cell1_end + 2 * (size_t)(o1 + i1);
                window(e, w[1]);
                nw = 2;
                vx = (double)((long long)e[0] - q[0]);
                vy = (double)((long long)e[1] - q[1]);
                const double mag = std::sqrt(vx * vx + vy * vy);
                vx /= mag;
                vy /= mag;
            }
            int best_d = INT_MAX, best_d2 = INT_MAX, best_idx = -1;
            const uint8_t *d1 = b->desc1 + (size_t)(o1 + i1) * b->desc_bytes;
            for (int i2 = 0; i2 < n2; ++i2) {
                bool cand = false;
                for (int v = 0; v < nw && !cand; ++v) {
                    if (bx1[i2] < w[v][0] || bx0[i2] >= w[v][1] || by1[i2] < w[v][2] || by0[i2] >= w[v][3]) continue;
                    for (int c = b->cell_off2[o2 + i2]; c < b->cell_off2[o2 + i2 + 1] && !cand; ++c) {
                        const int cx = b->cells2[2 * c], cy = b->cells2[2 * c + 1];
                        cand = cx >= w[v][0] && cx < w[v][1] && cy >= w[v][2] && cy < w[v][3];
                    }
                }
                if (!cand) continue;
                if (line) {
                    const double *dd = b->dir2 + 2 * (size_t)(o2 + i2);
                    const double px = vx * dd[0], py = vy * dd[1];
                    const double dot = px + py;
                    if (std::abs(dot) < b->line_sim_th[k]) continue;
                }
                const uint8_t *d2 = b->desc2 + (size_t)(o2 + i2) * b->desc_bytes;
                int d = 0;
                for (int c = 0; c < dw; ++c) {
                    uint32_t x, y;
                    std::memcpy(&x, d1 + 4 * c, 4);
                    std::memcpy(&y, d2 + 4 * c, 4);
                    d += __builtin_popcount(x ^ y);
                }
                if (b->best_lr) {
                    if (d < distances[i2]) {
                        distances[i2] = d;
                        matches_21[i2] = i1;
                    } else {
                        continue;
                    }
                }
                if (d < best_d) {
                    best_d2 = best_d;
                    best_d = d;
                    best_idx = i2;
                } else if (d < best_d2) {
                    best_d2 = d;
                }
            }
            const bool ok = best_idx >= 0 && (double)best_d < (double)best_d2 * b->nnr[k];
            matches_12[o1 + i1] = ok ? best_idx : -1;
            matches += ok;
        }
        if (b->best_lr)
            for (int i1 = 0; i1 < n1; ++i1) {
                int32_t &i2 = matches_12[o1 + i1];
                if (i2 >= 0 && matches_21[i2] != i1) {
                    i2 = -1;
                    --matches;
                }
            }
        n_matches[k] = matches;
    }
    return PLBA_OK;
}

int gridMatchCpu(const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches) {
    return gridMatchCpuWin(b, nullptr, matches_12, n_matches);
}

namespace {
constexpr int kGridCols = 64, kGridRows = 48;  // GRID_COLS / GRID_ROWS (include2/stereoFrame.h:51-52)

struct Projected {
    double u, v, z;
};
// Twf * X, then cam->projection (src2/pinholeStereoCamera.cpp:235-241)
Projected project(const Mat4 &T, const double *X, double fx, double fy, double cx, double cy) {
    const double x = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3], y = T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7],
                 z = T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11];
    return {cx + fx * x / z, cy + fy * y / z, z};
}
}  // namespace

int MapHandler::matchMapToKf(int kf_idx, const Mat4 *Twf_in, const MapMatchParams &p, MapMatchStats *stats) {
    MapMatchStats st;
    if (kf_idx < 0 || kf_idx >= (int)map_keyframes.size() || !map_keyframes[kf_idx]) {
        setError("matchMapToKf: no keyframe %d", kf_idx);
        return PLBA_E_INVALID;
    }
    KeyFrame *kf = map_keyframes[kf_idx];
    StereoFrame &f = kf->stereo_frame;
    const int np = (int)f.stereo_pt_idx.size(), nl = (int)f.stereo_ls_idx.size();
    if (!f.has_features || (nl && !f.has_endpoints)) {
        setError("matchMapToKf: keyframe %d has no features (or no line endpoints)", kf_idx);
        return PLBA_E_INVALID;
    }
    if (width_ <= 0 || height_ <= 0) {
        setError("matchMapToKf: the image size is not set");
        return PLBA_E_INVALID;
    }
    if (p.ws < 0 || kf_idx >= (int)full_graph.size()) {
        setError("matchMapToKf: window %d, or keyframe %d outside full_graph", p.ws, kf_idx);
        return PLBA_E_INVALID;
    }
    const Mat4 Twf = Twf_in ? *Twf_in : inverse4(kf->T_kf_w);
    const int db = f.desc_bytes, ng = (int)full_graph.size();
    const double inv_width = kGridCols / (double)width_, inv_height = kGridRows / (double)height_;
    auto in_image = [&](const Projected &q) { return q.u > 0 && q.u < width_ && q.v > 0 && q.v < height_ && q.z > 0.0; };
    auto obs_ok = [&](const std::vector<int> &kfs) {
        for (int o : kfs)
            if (o < 0 || o >= ng || (int)full_graph[o].size() < ng) return false;
        return true;
    };

    // the local map seen from the keyframe (:710-723, :812-828) and its unmatched features (:728-734, :833-839)
    std::vector<MapPoint *> map_local_points;
    std::vector<MapLine *> map_local_lines;
    std::vector<int> um_pt, um_ls;
    std::vector<int32_t> cell1, cell1_end;
    std::vector<uint8_t> desc1;
    if (p.has_points && np) {
        for (MapPoint *pt : map_points) {
            if (!pt || !pt->local || pt->kf_obs_list.empty() || pt->kf_obs_list.back() == kf_idx) continue;
            const Projected q = project(Twf, pt->point3D.data(), fx_, fy_, cx_, cy_);
            if (!in_image(q)) continue;
            if ((int)pt->med_desc.size() != db || !obs_ok(pt->kf_obs_list)) {
                setError("matchMapToKf: point %d has a descriptor of %zu bytes or an observer outside full_graph", pt->idx,
                         pt->med_desc.size());
                return PLBA_E_INVALID;
            }
            map_local_points.push_back(pt);
            cell1.insert(cell1.end(), {(int32_t)(q.u * inv_width), (int32_t)(q.v * inv_height)});
            cell1_end.insert(cell1_end.end(), {0, 0});
            desc1.insert(desc1.end(), pt->med_desc.begin(), pt->med_desc.end());
        }
        for (int i = 0; i < np; ++i)
            if (f.stereo_pt_idx[i] == -1) um_pt.push_back(i);
        st.visible[0] = (int)map_local_points.size();
        st.unmatched[0] = (int)um_pt.size();
        if (map_local_points.empty() || um_pt.empty()) {  // :736
            map_local_points.clear(); um_pt.clear(); cell1.clear(); cell1_end.clear(); desc1.clear();
        }
    }
    const int n1p = (int)map_local_points.size(), n2p = (int)um_pt.size();
    if (p.has_lines && nl) {
        const size_t keep = cell1.size(), keep_d = desc1.size();
        for (MapLine *ls : map_lines) {
            if (!ls || !ls->local || ls->kf_obs_list.empty() || ls->kf_obs_list.back() == kf_idx) continue;
            const Projected s = project(Twf, ls->line3D.data(), fx_, fy_, cx_, cy_),
                            e = project(Twf, ls->line3D.data() + 3, fx_, fy_, cx_, cy_);
            if (!in_image(s) || !in_image(e)) continue;
            if ((int)ls->med_desc.size() != db || !obs_ok(ls->kf_obs_list)) {
                setError("matchMapToKf: line %d has a descriptor of %zu bytes or an observer outside full_graph", ls->idx,
                         ls->med_desc.size());
                return PLBA_E_INVALID;
            }
            map_local_lines.push_back(ls);
            cell1.insert(cell1.end(), {(int32_t)(s.u * inv_width), (int32_t)(s.v * inv_height)});
            cell1_end.insert(cell1_end.end(), {(int32_t)(e.u * inv_width), (int32_t)(e.v * inv_height)});
            desc1.insert(desc1.end(), ls->med_desc.begin(), ls->med_desc.end());
        }
        for (int i = 0; i < nl; ++i)
            if (f.stereo_ls_idx[i] == -1) um_ls.push_back(i);
        st.visible[1] = (int)map_local_lines.size();
        st.unmatched[1] = (int)um_ls.size();
        if (map_local_lines.empty() || um_ls.empty()) {  // :841
            map_local_lines.clear(); um_ls.clear(); cell1.resize(keep); cell1_end.resize(keep); desc1.resize(keep_d);
        }
    }
    const int n1l = (int)map_local_lines.size(), n2l = (int)um_ls.size();
    if (n2p > 65535 || n2l > 65535) {
        setError("matchMapToKf: more than 65535 unmatched features of a kind");
        return PLBA_E_INVALID;
    }

    // the train side: descriptors, the grid's content as a cell list per feature, the line directions
    std::vector<uint8_t> desc2((size_t)(n2p + n2l) * db);
    std::vector<int32_t> cell_off2{0}, cells2;
    std::vector<double> dir2(2 * (size_t)(n2p + n2l), 0.0);
    std::vector<std::array<int, 2>> line_coords;
    for (int k = 0; k < n2p; ++k) {
        const int i = um_pt[k];
        std::memcpy(&desc2[(size_t)k * db], &f.pdesc_l[(size_t)i * db], db);
        cells2.insert(cells2.end(), {(int32_t)(f.pt_pl[2 * i] * inv_width), (int32_t)(f.pt_pl[2 * i + 1] * inv_height)});  // :748
        cell_off2.push_back((int32_t)(cells2.size() / 2));
    }
    for (int k = 0; k < n2l; ++k) {
        const int i = um_ls[k];
        std::memcpy(&desc2[(size_t)(n2p + k) * db], &f.ldesc_l[(size_t)i * db], db);
        const double *sp = &f.ls_spl[2 * i], *ep = &f.ls_epl[2 * i];
        double vx = (ep[0] - sp[0]) * inv_width, vy = (ep[1] - sp[1]) * inv_height;  // :857-858
        const double mag = std::sqrt(vx * vx + vy * vy);
        dir2[2 * (size_t)(n2p + k)] = vx / mag;
        dir2[2 * (size_t)(n2p + k) + 1] = vy / mag;
        if (lineCells(sp[0] * inv_width, sp[1] * inv_height, ep[0] * inv_width, ep[1] * inv_height, line_coords, 1u << 20) < 0) {
            setError("matchMapToKf: line feature %d of keyframe %d has endpoints that are not finite", i, kf_idx);
            return PLBA_E_INVALID;
        }
        for (const auto &c : line_coords) cells2.insert(cells2.end(), {c[0], c[1]});
        cell_off2.push_back((int32_t)(cells2.size() / 2));
    }

    std::vector<int32_t> m12((size_t)(n1p + n1l) + 1, -1);
    int32_t matches[2] = {0, 0};
    const int32_t off1[3] = {0, n1p, n1p + n1l}, off2[3] = {0, n2p, n2p + n2l};
    const auto t0 = std::chrono::steady_clock::now();
    if (p.fast_matching && n1p + n1l > 0) {  // :743-757, :848-872 in one call
        const int32_t kind[2] = {0, 1}, ws[2] = {p.ws, p.ws};
        const double nnr[2] = {p.min_ratio_12_p, p.min_ratio_12_p}, th[2] = {p.line_sim_th, p.line_sim_th};  // :160, :241
        plba_gridmatch_batch b{};
        b.n = 2; b.desc_bytes = db; b.cols = kGridCols; b.rows = kGridRows; b.best_lr = p.best_lr ? 1 : 0;
        b.off1 = off1; b.off2 = off2; b.desc1 = desc1.data(); b.desc2 = desc2.data();
        b.cell1 = cell1.data(); b.cell1_end = cell1_end.data(); b.cell_off2 = cell_off2.data(); b.cells2 = cells2.data();
        b.dir2 = dir2.data(); b.kind = kind; b.ws = ws; b.nnr = nnr; b.line_sim_th = th;
        const int rc = backend(grid_, "grid matcher", [&](plba_ctx *ctx) { return plba_grid_match(ctx, &b, m12.data(), matches); },
                               &b, m12.data(), matches);
        if (rc) return rc;
    }
    st.grid_matches[0] = matches[0];
    st.grid_matches[1] = matches[1];
    // :759-764, :874-879: too few grid matches on a map side above the minimum: brute force. (The reference's
    // match() resizes matches_12 without clearing it, so a grid match that the brute-force ratio test does not
    // replace can survive there; here the fallback's result stands alone.)
    st.fallback[0] = n1p > p.min_pt_matches && matches[0] < p.min_pt_matches;
    st.fallback[1] = n1l > p.min_ls_matches && matches[1] < p.min_ls_matches;
    if (st.fallback[0] || st.fallback[1]) {
        const int a1 = st.fallback[0] ? n1p : 0, a2 = st.fallback[0] ? n2p : 0, b1 = st.fallback[1] ? n1l : 0,
                  b2 = st.fallback[1] ? n2l : 0;
        std::vector<uint8_t> d1((size_t)(a1 + b1) * db), d2((size_t)(a2 + b2) * db);
        if (a1) std::memcpy(d1.data(), desc1.data(), (size_t)a1 * db);
        if (a2) std::memcpy(d2.data(), desc2.data(), (size_t)a2 * db);
        if (b1) std::memcpy(d1.data() + (size_t)a1 * db, desc1.data() + (size_t)n1p * db, (size_t)b1 * db);
        if (b2) std::memcpy(d2.data() + (size_t)a2 * db, desc2.data() + (size_t)n2p * db, (size_t)b2 * db);
        const int32_t o1[3] = {0, a1, a1 + b1}, o2[3] = {0, a2, a2 + b2};
        const float nnr[2] = {(float)p.min_ratio_12_p, (float)p.min_ratio_12_l};
        plba_match_batch mb{2, db, o1, o2, d1.data(), d2.data(), nnr, p.best_lr ? 1 : 0, 0};
        std::vector<int32_t> fm((size_t)(a1 + b1) + 1, -1);
        int32_t cnt[2] = {0, 0};
        const int rc = backend(match_, "matcher", [&](plba_ctx *ctx) { return plba_desc_match(ctx, &mb, fm.data(), cnt); },
                               &mb, fm.data(), cnt);
        if (rc) return rc;
        if (st.fallback[0]) std::copy(fm.begin(), fm.begin() + a1, m12.begin());
        if (st.fallback[1]) std::copy(fm.begin() + a1, fm.begin() + a1 + b1, m12.begin() + n1p);
    }
    st.match_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int i1 = 0; i1 < n1p + n1l; ++i1) {  // what a matcher hook returns is checked before the map changes
        const int lim = i1 < n1p ? n2p : n2l;
        if (m12[i1] < -1 || m12[i1] >= lim) {
            setError("matchMapToKf: match %d of row %d is outside its %d features", m12[i1], i1, lim);
            return PLBA_E_INVALID;
        }
    }

    auto bump_graph = [&](const std::vector<int> &kfs) {  // :786-791, :910-915
        for (int obs : kfs)
            if (obs != kf_idx) {
                full_graph[kf_idx][obs]++;
                full_graph[obs][kf_idx]++;
            }
    };
    const Mat4 &Tk = kf->T_kf_w;
    for (int i1 = 0; i1 < n1p; ++i1) {  // :766-794
        const int i2 = m12[i1];
        if (i2 < 0) continue;
        MapPoint *pt = map_local_points[i1];
        const int fi = um_pt[i2];
        const Projected q = project(Twf, pt->point3D.data(), fx_, fy_, cx_, cy_);
        const double du = q.u - f.pt_pl[2 * fi], dv = q.v - f.pt_pl[2 * fi + 1];
        if (std::sqrt(du * du + dv * dv) < p.max_kf_epip_p) {
            f.stereo_pt_idx[fi] = pt->idx;
            const double *P = &f.pt_P[3 * fi];
            const double n = std::sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]);
            const double d[3] = {P[0] / n, P[1] / n, P[2] / n};
            // :783 as the reference has it: the rotation and the translation of T_kf_w
            const Vec3 dir{Tk[0] * d[0] + Tk[1] * d[1] + Tk[2] * d[2] + Tk[3], Tk[4] * d[0] + Tk[5] * d[1] + Tk[6] * d[2] + Tk[7],
                           Tk[8] * d[0] + Tk[9] * d[1] + Tk[10] * d[2] + Tk[11]};
            pt->addMapPointObservation(Desc(&f.pdesc_l[(size_t)fi * db], &f.pdesc_l[(size_t)fi * db] + db), kf_idx,
                                       Vec2{f.pt_pl[2 * fi], f.pt_pl[2 * fi + 1]}, dir, 1.0);
            bump_graph(pt->kf_obs_list);
            ++st.accepted[0];
        } else {
            ++st.rejected[0];
        }
    }
    for (int i1 = 0; i1 < n1l; ++i1) {  // :881-918
        const int i2 = m12[n1p + i1];
        if (i2 < 0) continue;
        MapLine *ls = map_local_lines[i1];
        const int fi = um_ls[i2];
        const Projected s = project(Twf, ls->line3D.data(), fx_, fy_, cx_, cy_),
                        e = project(Twf, ls->line3D.data() + 3, fx_, fy_, cx_, cy_);
        const double *le = &f.ls_le[3 * fi];
        const double err0 = le[0] * s.u + le[1] * s.v + le[2], err1 = le[0] * e.u + le[1] * e.v + le[2];
        if (err0 < p.max_kf_epip_l && err1 < p.max_kf_epip_l) {  // signed, as the reference has it (:894)
            f.stereo_ls_idx[fi] = ls->idx;
            ls->addMapLineObservation(Desc(&f.ldesc_l[(size_t)fi * db], &f.ldesc_l[(size_t)fi * db] + db), kf_idx,
                                      Vec4{f.ls_spl[2 * fi], f.ls_spl[2 * fi + 1], f.ls_epl[2 * fi], f.ls_epl[2 * fi + 1]}, 1.0);
            bump_graph(ls->kf_obs_list);
            ++st.accepted[1];
        } else {
            ++st.rejected[1];
        }
    }
    if (stats) *stats = st;
    return PLBA_OK;
}

int MapHandler::localMappingStepKf(int kf_idx, const MapMatchParams &p, MapMatchStats *ms, LbaStats *stats, CullStats *cs) {
    const int rc = matchMapToKf(kf_idx, nullptr, p, ms);
    if (rc) return rc;
    return localMappingStep(kf_idx, stats, cs);
}

}  // namespace plslam
