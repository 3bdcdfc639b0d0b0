// fuse_landmarks.cpp — MapHandler::loopClosureFuseLandmarks() (src/mapHandler.cpp:5533-5808) on the
// host mirror: for every loop whose lc_idx_list flag is 1, the rows (lm_idx0, lm_ldx0, lm_idx1, lm_ldx1)
// that isLoopClosure stored in lc_pt_idxs / lc_ls_idxs, points first and then lines, statement for
// statement: an observation added to the later landmark (:5552), to the earlier one (:5567), a new
// landmark from both features (:5585), or two landmarks fused and the second erased (:5612), with the
// reference's full_graph increments (the first case names kf_curr_idx although the observation comes
// from kf_prev_idx, :5562, and the second the other way round, :5579), its map_*_kf_idx erase, its
// feature idx rewrites and max_pt_idx / max_ls_idx (map_points.size() / map_lines.size() here, as in
// kf_match.cpp).
//
// The reference runs updateAverageDescDir() after every observation it appends (:5636, :5784 and inside
// addMap*Observation). That function assigns med_desc (and for points med_obs_dir) wholesale from the
// lists as they are and keeps no state, and nothing between two appends reads either field, so only the
// last call on a landmark is observable. The walk below therefore only edits the lists and notes which
// landmarks changed; afterwards one medoid batch (plba_desc_medoid on the map's context, or the hook)
// gives every changed landmark that is still alive its med_desc, and updateAverageDir() its direction.
//
// Defined here where the reference is not:
//  - a row with lm_idx0 == lm_idx1 != -1 would append to the list it iterates: left untouched, counted
//    in same_landmark;
//  - a feature index past a keyframe's arrays, a landmark index outside [-1, size of the map), a loop
//    without keyframes or an observer outside full_graph: PLBA_E_INVALID before the map is touched. The
//    new-line branch reads stereo_ls[lm_ldx1]->epl of the *previous* keyframe (:5747): lm_ldx1 must
//    be inside that keyframe's lines too;
//  - a feature of the mirror is a row of its keyframe's arrays and cannot be NULL: of the NULL guards
//    the landmark halves remain. A landmark erased by one row is NULL for every later row;
//  - the fourth case does not copy sigma_list (the local BA would read past it): copied here. An erased
//    landmark without observations has no kf_obs_list[0]: nothing is removed from map_*_kf_idx then, and a
//    first observer without a map_*_kf_idx entry (.at() throws) removes nothing either;
//  - lines. The reference calls the endpoint constructor and the endpoint addMapLineObservation in a
//    Plücker build too (src/mapFeatures.cpp:98-109, :121-130): they fill obs_list (le), dir_list and
//    pts_list and leave NDw, orthNDw and NDw_obs_list unset, so the next Plücker BA would read an
//    uninitialised NDw and index NDw_obs_list past its end. The mirror keeps one observation list per
//    line, NDw_obs_list, parallel to kf_obs_list: it takes pts (what the Plücker observations hold: the
//    two image endpoints) with sigma2 = 1; dir goes to dir_list; le is not stored. A new line stores
//    line3D = (sP, eP) in the world, med_obs_dir = dir, and NDw = (sP x eP, eP - sP), the Plücker
//    coordinates of that segment; orthNDw stays zero until a BA sets it. The fourth case copies dir_list
//    entries as far as the erased line has them (a line made by Plücker observations has none). The
//    mirror has one spl / epl per line feature, which serves as spl_obs / epl_obs too.
#include "plslam_map.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <set>

namespace plslam {

namespace {

Vec3 rot_trans(const Mat4 &T, const double *p) {  // T.block(0,0,3,3) * p + T.col(3).head(3)
    Vec3 o;
    for (int i = 0; i < 3; ++i) o[i] = T[4 * i] * p[0] + T[4 * i + 1] * p[1] + T[4 * i + 2] * p[2] + T[4 * i + 3];
    return o;
}
Vec3 unit(const Vec3 &v) {  // v / v.norm()
    const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    return Vec3{v[0] / n, v[1] / n, v[2] / n};
}
Desc desc_row(const std::vector<uint8_t> &d, size_t db, int i) {
    return Desc(d.begin() + db * (size_t)i, d.begin() + db * (size_t)(i + 1));
}

}  // namespace

// plba_desc_medoid's semantics as the reference computes them: the table, a sort of every row.
int descMedoidCpu(const plba_medoid_batch *b, int32_t *medoid) {
    if (!b || b->n < 0) return PLBA_E_INVALID;
    if (b->n == 0) return PLBA_OK;
    if (!b->list_ptr || !medoid || b->desc_bytes < 4 || b->desc_bytes > 64 || b->desc_bytes % 4 || b->list_ptr[0] < 0)
        return PLBA_E_INVALID;
    for (int l = 0; l < b->n; ++l)
        if (b->list_ptr[l + 1] < b->list_ptr[l] || b->list_ptr[l + 1] - b->list_ptr[l] > PLBA_MEDOID_MAX_N) return PLBA_E_INVALID;
    if (b->list_ptr[b->n] && !b->desc) return PLBA_E_INVALID;
    const size_t db = (size_t)b->desc_bytes;
    std::vector<int> conf, row;
    for (int l = 0; l < b->n; ++l) {
        const int n = b->list_ptr[l + 1] - b->list_ptr[l];
        const uint8_t *d = b->desc + db * (size_t)b->list_ptr[l];
        if (n == 0) {
            medoid[l] = -1;
            continue;
        }
        conf.assign((size_t)n * n, 0);
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) {
                int h = 0;
                for (size_t c = 0; c < db; ++c) h += __builtin_popcount((unsigned)(d[db * i + c] ^ d[db * j + c]));
                conf[(size_t)i * n + j] = h;
                conf[(size_t)j * n + i] = h;
            }
        int max_dist = 99999, max_idx = 0;
        row.resize(n);
        const int k = std::min(int(1 + 0.5 * (n - 1)), n - 1);
        for (int i = 0; i < n; ++i) {
            std::copy(conf.begin() + (size_t)i * n, conf.begin() + (size_t)(i + 1) * n, row.begin());
            std::sort(row.begin(), row.end());
            if (row[k] < max_dist) {
                max_dist = row[k];
                max_idx = i;
            }
        }
        medoid[l] = max_idx;
    }
    return PLBA_OK;
}

int MapHandler::fuseLandmarks(FuseStats *stats) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    FuseStats st;
    const int nkf = (int)map_keyframes.size();
    size_t db = 0;  // the descriptor size of every list the batch will hold

    // ---- everything that could fail is checked before the map changes; the lists' lengths are followed
    // through the rows so that a list the device would refuse is refused here
    for (int kind = 0; kind < 2; ++kind) {
        const auto &loops = kind ? lc_ls_idxs : lc_pt_idxs;
        const char *const what = kind ? "line" : "point";
        const int nlm = kind ? (int)map_lines.size() : (int)map_points.size();
        std::map<int, long> len;
        std::set<int> dead, kfs;
        auto alive = [&](int idx) { return (kind ? (void *)map_lines[idx] : (void *)map_points[idx]) != nullptr && !dead.count(idx); };
        auto length = [&](int idx) -> long & {
            auto it = len.find(idx);
            if (it == len.end())
                it = len.emplace(idx, (long)(kind ? map_lines[idx]->desc_list.size() : map_points[idx]->desc_list.size())).first;
            return it->second;
        };
        for (int lc = 0; lc < (int)loops.size(); ++lc) {
            if (lc >= (int)lc_idx_list.size()) {
                setError("fuseLandmarks: %s loop %d has no lc_idx_list entry", what, lc);
                return PLBA_E_INVALID;
            }
            if (lc_idx_list[lc][2] != 1) continue;
            const int kf0 = lc_idx_list[lc][0], kf1 = lc_idx_list[lc][1];
            if (kf0 < 0 || kf0 >= nkf || kf1 < 0 || kf1 >= nkf || !map_keyframes[kf0] || !map_keyframes[kf1]) {
                setError("fuseLandmarks: loop %d names keyframes %d and %d, which the map does not have", lc, kf0, kf1);
                return PLBA_E_INVALID;
            }
            if (loops[lc].empty()) continue;
            const StereoFrame &f0 = map_keyframes[kf0]->stereo_frame, &f1 = map_keyframes[kf1]->stereo_frame;
            if (!f0.has_features || !f1.has_features || f0.desc_bytes != f1.desc_bytes || (kind && (!f0.has_endpoints || !f1.has_endpoints))) {
                setError("fuseLandmarks: keyframe %d or %d has no features%s, or their descriptor sizes differ", kf0, kf1,
                         kind ? " or line endpoints" : "");
                return PLBA_E_INVALID;
            }
            if (db == 0) db = (size_t)f0.desc_bytes;
            if (db != (size_t)f0.desc_bytes) {
                setError("fuseLandmarks: the loops' keyframes have descriptors of %zu and %d bytes", db, f0.desc_bytes);
                return PLBA_E_INVALID;
            }
            const int n0 = (int)(kind ? f0.stereo_ls_idx.size() : f0.stereo_pt_idx.size());
            const int n1 = (int)(kind ? f1.stereo_ls_idx.size() : f1.stereo_pt_idx.size());
            kfs.insert(kf0);
            kfs.insert(kf1);
            for (size_t r = 0; r < loops[lc].size(); ++r) {
                const Vec4i &row = loops[lc][r];
                const int i0 = row[0], l0 = row[1], i1 = row[2], l1 = row[3];
                if (i0 < -1 || i0 >= nlm || i1 < -1 || i1 >= nlm) {
                    setError("fuseLandmarks: row %zu of %s loop %d names landmarks %d and %d outside the map (%d slots)", r, what,
                             lc, i0, i1, nlm);
                    return PLBA_E_INVALID;
                }
                if (l0 < 0 || l0 >= n0 || l1 < 0 || l1 >= n1 || (kind && i0 == -1 && i1 == -1 && l1 >= n0)) {
                    setError("fuseLandmarks: row %zu of %s loop %d names features %d and %d past the keyframes' %d and %d", r,
                             what, lc, l0, l1, n0, n1);
                    return PLBA_E_INVALID;
                }
                for (int idx : {i0, i1}) {
                    if (idx < 0 || !alive(idx) || len.count(idx)) continue;
                    const std::vector<Desc> &dl = kind ? map_lines[idx]->desc_list : map_points[idx]->desc_list;
                    const std::vector<int> &ko = kind ? map_lines[idx]->kf_obs_list : map_points[idx]->kf_obs_list;
                    bool ok = dl.size() == ko.size();
                    if (kind) ok = ok && map_lines[idx]->NDw_obs_list.size() == dl.size() && map_lines[idx]->sigma_list.size() == dl.size();
                    else ok = ok && map_points[idx]->obs_list.size() == dl.size() && map_points[idx]->dir_list.size() == dl.size() &&
                              map_points[idx]->sigma_list.size() == dl.size();
                    for (const Desc &d : dl) ok = ok && d.size() == db;
                    for (int k : ko) {
                        ok = ok && k >= 0;
                        kfs.insert(k);
                    }
                    if (!ok) {
                        setError("fuseLandmarks: %s landmark %d has lists of different lengths, a descriptor of another size or a negative observer",
                                 what, idx);
                        return PLBA_E_INVALID;
                    }
                    length(idx);
                }
                if (i0 == -1 && i1 != -1 && alive(i1)) length(i1)++;
                if (i0 != -1 && i1 == -1 && alive(i0)) length(i0)++;
                if (i0 != -1 && i1 != -1 && i0 != i1 && alive(i0) && alive(i1)) {
                    length(i0) += length(i1);
                    dead.insert(i1);
                }
            }
        }
        if (!kfs.empty()) {
            const int top = *kfs.rbegin();
            for (int k : kfs)
                if (k >= (int)full_graph.size() || top >= (int)full_graph[k].size()) {
                    setError("fuseLandmarks: full_graph has no entry for keyframes %d and %d", k, top);
                    return PLBA_E_INVALID;
                }
        }
        if (!medoid_.fn)
            for (const auto &e : len)
                if (e.second > PLBA_MEDOID_MAX_N) {
                    setError("fuseLandmarks: %s landmark %d would have %ld descriptors, more than %d", what, e.first, e.second,
                             PLBA_MEDOID_MAX_N);
                    return PLBA_E_INVALID;
                }
    }

    std::vector<std::pair<int, int>> changed;  // (kind, idx) in the order of the first change
    std::set<std::pair<int, int>> seen;
    auto touch = [&](int kind, int idx) {
        landmark_changed(store_.get(), kind, idx);
        if (seen.insert({kind, idx}).second) changed.push_back({kind, idx});
    };
    auto bump = [&](int a, int b) {
        full_graph[a][b]++;
        full_graph[b][a]++;
    };

    // ---- point matches (:5536-5658)
    for (int lc = 0; lc < (int)lc_pt_idxs.size(); ++lc) {
        if (lc_idx_list[lc][2] != 1) {  // already optimised
            ++st.loops_skipped;
            continue;
        }
        ++st.loops;
        const int kf_prev_idx = lc_idx_list[lc][0], kf_curr_idx = lc_idx_list[lc][1];
        KeyFrame *kp = map_keyframes[kf_prev_idx], *kc = map_keyframes[kf_curr_idx];
        StereoFrame &fp = kp->stereo_frame, &fc = kc->stereo_frame;
        for (const Vec4i &row : lc_pt_idxs[lc]) {
            const int lm_idx0 = row[0], lm_ldx0 = row[1], lm_idx1 = row[2], lm_ldx1 = row[3];
            auto add_obs = [&](MapPoint *mp, KeyFrame *k, int ldx) {  // addMapPointObservation without the average
                const StereoFrame &f = k->stereo_frame;
                mp->desc_list.push_back(desc_row(f.pdesc_l, db, ldx));
                mp->obs_list.push_back(Vec2{f.pt_pl[2 * ldx], f.pt_pl[2 * ldx + 1]});
                mp->kf_obs_list.push_back(k->kf_idx);
                mp->dir_list.push_back(unit(Vec3{f.pt_P[3 * ldx], f.pt_P[3 * ldx + 1], f.pt_P[3 * ldx + 2]}));
                mp->sigma_list.push_back(1.0);
                touch(1, mp->idx);
            };
            if (lm_idx0 == -1 && lm_idx1 != -1) {  // the landmark exists once: add the observation
                if (MapPoint *mp = map_points[lm_idx1]) {
                    fp.stereo_pt_idx[lm_ldx0] = lm_idx1;
                    add_obs(mp, kp, lm_ldx0);
                    for (int kf : mp->kf_obs_list) bump(kf, kf_curr_idx);  // :5560-5564
                    ++st.rows[0][0];
                } else ++st.null_skipped[0][0];
            }
            if (lm_idx0 != -1 && lm_idx1 == -1) {
                if (MapPoint *mp = map_points[lm_idx0]) {
                    fc.stereo_pt_idx[lm_ldx1] = lm_idx0;
                    add_obs(mp, kc, lm_ldx1);
                    for (int kf : mp->kf_obs_list) bump(kf, kf_prev_idx);  // :5577-5581
                    ++st.rows[0][1];
                } else ++st.null_skipped[0][1];
            }
            if (lm_idx0 == -1 && lm_idx1 == -1) {  // a new landmark with both observations
                const int max_pt_idx = (int)map_points.size();
                fp.stereo_pt_idx[lm_ldx0] = max_pt_idx;
                fc.stereo_pt_idx[lm_ldx1] = max_pt_idx;
                Vec3 P3d = rot_trans(kp->T_kf_w, &fp.pt_P[3 * lm_ldx0]);
                auto *mp = new MapPoint(max_pt_idx, P3d, desc_row(fp.pdesc_l, db, lm_ldx0), kp->kf_idx,
                                        Vec2{fp.pt_pl[2 * lm_ldx0], fp.pt_pl[2 * lm_ldx0 + 1]}, unit(P3d), 1.0);
                map_points_kf_idx[kf_prev_idx].push_back(max_pt_idx);
                P3d = rot_trans(kc->T_kf_w, &fc.pt_P[3 * lm_ldx1]);
                mp->desc_list.push_back(desc_row(fc.pdesc_l, db, lm_ldx1));
                mp->obs_list.push_back(Vec2{fc.pt_pl[2 * lm_ldx1], fc.pt_pl[2 * lm_ldx1 + 1]});
                mp->kf_obs_list.push_back(kc->kf_idx);
                mp->dir_list.push_back(unit(P3d));
                mp->sigma_list.push_back(1.0);
                map_points.push_back(mp);
                adoptLandmark(1, max_pt_idx);
                touch(1, max_pt_idx);
                bump(kf_prev_idx, kf_curr_idx);
                ++st.rows[0][2];
            }
            if (lm_idx0 != -1 && lm_idx1 != -1) {  // two landmarks: fuse them and erase the second
                if (lm_idx0 == lm_idx1) {
                    ++st.same_landmark[0];
                    continue;
                }
                MapPoint *m0 = map_points[lm_idx0], *m1 = map_points[lm_idx1];
                if (!m0 || !m1) {
                    ++st.null_skipped[0][3];
                    continue;
                }
                const int Nobs_lm_prev = (int)m0->kf_obs_list.size();
                for (size_t iter = 0; iter < m1->desc_list.size(); ++iter) {
                    m0->desc_list.push_back(m1->desc_list[iter]);
                    m0->obs_list.push_back(m1->obs_list[iter]);
                    m0->dir_list.push_back(m1->dir_list[iter]);
                    m0->kf_obs_list.push_back(m1->kf_obs_list[iter]);
                    m0->sigma_list.push_back(m1->sigma_list[iter]);
                    const int jdx = m1->kf_obs_list[iter];
                    for (int i = 0; i < Nobs_lm_prev; ++i) bump(m0->kf_obs_list[i], jdx);
                    fc.stereo_pt_idx[lm_ldx1] = lm_idx0;
                    touch(1, lm_idx0);
                }
                if (!m1->kf_obs_list.empty()) {  // :5640-5650
                    auto it = map_points_kf_idx.find(m1->kf_obs_list[0]);
                    if (it != map_points_kf_idx.end()) {
                        auto pos = std::find(it->second.begin(), it->second.end(), lm_idx1);
                        if (pos != it->second.end()) it->second.erase(pos);
                    }
                }
                delete m1;
                map_points[lm_idx1] = nullptr;
                markLandmarkChanged(1, lm_idx1);
                ++st.erased[0];
                ++st.rows[0][3];
            }
        }
    }

    // ---- line segment matches (:5660-5806)
    for (int lc = 0; lc < (int)lc_ls_idxs.size(); ++lc) {
        if (lc_idx_list[lc][2] != 1) {
            if (lc >= (int)lc_pt_idxs.size()) ++st.loops_skipped;
            continue;
        }
        if (lc >= (int)lc_pt_idxs.size()) ++st.loops;
        const int kf_prev_idx = lc_idx_list[lc][0], kf_curr_idx = lc_idx_list[lc][1];
        KeyFrame *kp = map_keyframes[kf_prev_idx], *kc = map_keyframes[kf_curr_idx];
        StereoFrame &fp = kp->stereo_frame, &fc = kc->stereo_frame;
        for (const Vec4i &row : lc_ls_idxs[lc]) {
            const int lm_idx0 = row[0], lm_ldx0 = row[1], lm_idx1 = row[2], lm_ldx1 = row[3];
            auto add_obs = [&](MapLine *ml, KeyFrame *k, int ldx) {  // the endpoint addMapLineObservation, see the header
                const StereoFrame &f = k->stereo_frame;
                const Vec3 mid{f.ls_sP[3 * ldx] + f.ls_eP[3 * ldx], f.ls_sP[3 * ldx + 1] + f.ls_eP[3 * ldx + 1],
                               f.ls_sP[3 * ldx + 2] + f.ls_eP[3 * ldx + 2]};
                ml->desc_list.push_back(desc_row(f.ldesc_l, db, ldx));
                ml->NDw_obs_list.push_back(Vec4{f.ls_spl[2 * ldx], f.ls_spl[2 * ldx + 1], f.ls_epl[2 * ldx], f.ls_epl[2 * ldx + 1]});
                ml->kf_obs_list.push_back(k->kf_idx);
                ml->dir_list.push_back(unit(mid));
                ml->sigma_list.push_back(1.0);
                touch(2, ml->idx);
            };
            if (lm_idx0 == -1 && lm_idx1 != -1) {
                if (MapLine *ml = map_lines[lm_idx1]) {
                    fp.stereo_ls_idx[lm_ldx0] = lm_idx1;
                    add_obs(ml, kp, lm_ldx0);
                    for (int kf : ml->kf_obs_list) bump(kf, kf_curr_idx);  // :5691-5695
                    ++st.rows[1][0];
                } else ++st.null_skipped[1][0];
            }
            if (lm_idx0 != -1 && lm_idx1 == -1) {
                if (MapLine *ml = map_lines[lm_idx0]) {
                    fc.stereo_ls_idx[lm_ldx1] = lm_idx0;
                    add_obs(ml, kc, lm_ldx1);
                    for (int kf : ml->kf_obs_list) bump(kf, kf_prev_idx);  // :5712-5716
                    ++st.rows[1][1];
                } else ++st.null_skipped[1][1];
            }
            if (lm_idx0 == -1 && lm_idx1 == -1) {
                const int max_ls_idx = (int)map_lines.size();
                fp.stereo_ls_idx[lm_ldx0] = max_ls_idx;
                fc.stereo_ls_idx[lm_ldx1] = max_ls_idx;
                Vec3 sP3d = rot_trans(kp->T_kf_w, &fp.ls_sP[3 * lm_ldx0]), eP3d = rot_trans(kp->T_kf_w, &fp.ls_eP[3 * lm_ldx0]);
                Vec3 mP3d{0.5 * (sP3d[0] + eP3d[0]), 0.5 * (sP3d[1] + eP3d[1]), 0.5 * (sP3d[2] + eP3d[2])};
                Vec3 dir = unit(mP3d);
                const Vec6 NDw{sP3d[1] * eP3d[2] - sP3d[2] * eP3d[1], sP3d[2] * eP3d[0] - sP3d[0] * eP3d[2],
                               sP3d[0] * eP3d[1] - sP3d[1] * eP3d[0], eP3d[0] - sP3d[0], eP3d[1] - sP3d[1], eP3d[2] - sP3d[2]};
                auto *ml = new MapLine(max_ls_idx, NDw, desc_row(fp.ldesc_l, db, lm_ldx0), kp->kf_idx,
                                       Vec4{fp.ls_spl[2 * lm_ldx0], fp.ls_spl[2 * lm_ldx0 + 1], fp.ls_epl[2 * lm_ldx0], fp.ls_epl[2 * lm_ldx0 + 1]}, 1.0);
                ml->line3D = Vec6{sP3d[0], sP3d[1], sP3d[2], eP3d[0], eP3d[1], eP3d[2]};
                ml->med_obs_dir = dir;
                ml->dir_list.push_back(dir);
                map_lines_kf_idx[kf_prev_idx].push_back(max_ls_idx);
                sP3d = rot_trans(kc->T_kf_w, &fc.ls_sP[3 * lm_ldx1]);
                eP3d = rot_trans(kc->T_kf_w, &fc.ls_eP[3 * lm_ldx1]);
                mP3d = Vec3{0.5 * (sP3d[0] + eP3d[0]), 0.5 * (sP3d[1] + eP3d[1]), 0.5 * (sP3d[2] + eP3d[2])};
                dir = unit(mP3d);
                ml->desc_list.push_back(desc_row(fc.ldesc_l, db, lm_ldx1));
                // pts.head(2) is the current keyframe's spl, pts.tail(2) the previous keyframe's epl at lm_ldx1 (:5746-5747)
                ml->NDw_obs_list.push_back(Vec4{fc.ls_spl[2 * lm_ldx1], fc.ls_spl[2 * lm_ldx1 + 1], fp.ls_epl[2 * lm_ldx1], fp.ls_epl[2 * lm_ldx1 + 1]});
                ml->kf_obs_list.push_back(kc->kf_idx);
                ml->dir_list.push_back(dir);
                ml->sigma_list.push_back(1.0);
                map_lines.push_back(ml);
                adoptLandmark(2, max_ls_idx);
                touch(2, max_ls_idx);
                bump(kf_prev_idx, kf_curr_idx);
                ++st.rows[1][2];
            }
            if (lm_idx0 != -1 && lm_idx1 != -1) {
                if (lm_idx0 == lm_idx1) {
                    ++st.same_landmark[1];
                    continue;
                }
                MapLine *m0 = map_lines[lm_idx0], *m1 = map_lines[lm_idx1];
                if (!m0 || !m1) {
                    ++st.null_skipped[1][3];
                    continue;
                }
                const int Nobs_lm_prev = (int)m0->kf_obs_list.size();
                for (size_t iter = 0; iter < m1->desc_list.size(); ++iter) {
                    m0->desc_list.push_back(m1->desc_list[iter]);
                    m0->NDw_obs_list.push_back(m1->NDw_obs_list[iter]);
                    if (iter < m1->dir_list.size()) m0->dir_list.push_back(m1->dir_list[iter]);
                    m0->kf_obs_list.push_back(m1->kf_obs_list[iter]);
                    m0->sigma_list.push_back(m1->sigma_list[iter]);
                    const int jdx = m1->kf_obs_list[iter];
                    for (int i = 0; i < Nobs_lm_prev; ++i) bump(m0->kf_obs_list[i], jdx);
                    fc.stereo_ls_idx[lm_ldx1] = lm_idx0;
                    touch(2, lm_idx0);
                }
                if (!m1->kf_obs_list.empty()) {  // :5788-5798
                    auto it = map_lines_kf_idx.find(m1->kf_obs_list[0]);
                    if (it != map_lines_kf_idx.end()) {
                        auto pos = std::find(it->second.begin(), it->second.end(), lm_idx1);
                        if (pos != it->second.end()) it->second.erase(pos);
                    }
                }
                delete m1;
                map_lines[lm_idx1] = nullptr;
                markLandmarkChanged(2, lm_idx1);
                ++st.erased[1];
                ++st.rows[1][3];
            }
        }
    }

    // ---- the last updateAverageDescDir() of every changed landmark that is still there: one medoid batch
    std::vector<int32_t> list_ptr{0};
    std::vector<uint8_t> desc;
    std::vector<std::pair<int, int>> live;
    for (const auto &c : changed) {
        const std::vector<Desc> *dl = nullptr;
        if (c.first == 1 && map_points[c.second]) dl = &map_points[c.second]->desc_list;
        if (c.first == 2 && map_lines[c.second]) dl = &map_lines[c.second]->desc_list;
        if (!dl || dl->empty()) continue;
        for (const Desc &d : *dl) desc.insert(desc.end(), d.begin(), d.end());
        list_ptr.push_back((int32_t)(desc.size() / db));
        live.push_back(c);
    }
    st.medoid_lists = (int)live.size();
    if (!live.empty()) {
        std::vector<int32_t> medoid(live.size(), -1);
        plba_medoid_batch b{};
        b.n = (int32_t)live.size();
        b.desc_bytes = (int32_t)db;
        b.list_ptr = list_ptr.data();
        b.desc = desc.data();
        const auto tm = clk::now();
        int rc = backend(medoid_, "medoid", [&](plba_ctx *ctx) { return plba_desc_medoid(ctx, &b, medoid.data()); }, &b, medoid.data());
        st.medoid_ms = std::chrono::duration<double, std::milli>(clk::now() - tm).count();
        for (size_t k = 0; !rc && k < live.size(); ++k)
            if (medoid[k] < 0 || medoid[k] >= list_ptr[k + 1] - list_ptr[k]) {
                setError("fuseLandmarks: medoid %d of a list of %d descriptors", medoid[k], list_ptr[k + 1] - list_ptr[k]);
                rc = PLBA_E_INVALID;
            }
        if (rc) {  // the lists are fused; med_desc comes from the host so that the map stays consistent
            for (const auto &c : live) {
                if (c.first == 1) map_points[c.second]->updateAverageDescDir();
                else map_lines[c.second]->updateAverageDescDir();
            }
            return rc;
        }
        for (size_t k = 0; k < live.size(); ++k) {
            if (live[k].first == 1) {
                MapPoint *mp = map_points[live[k].second];
                mp->med_desc = mp->desc_list[medoid[k]];
                mp->updateAverageDir();
            } else {
                MapLine *ml = map_lines[live[k].second];
                ml->med_desc = ml->desc_list[medoid[k]];  // USE_LINE_PLUKER: no direction average (:175-183)
            }
        }
    }
    st.total_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    if (stats) *stats = st;
    return PLBA_OK;
}

}  // namespace plslam
