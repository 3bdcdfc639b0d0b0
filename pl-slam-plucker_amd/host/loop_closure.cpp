// Host mirror of MapHandler::loopClosureOptimizationEssGraphG2O (src/mapHandler.cpp:5070-5299)
// and MapHandler::loopClosureOptimizationCovGraphG2O (:5301-5531) around the GPU pose-graph
// solve (plba_pgo_optimize), with the g2o SE3Quat conversions the reference goes through
// (SE3Quat::exp / log, SE3Quat <-> Isometry3 via Eigen's quaternion); and of MapHandler::loopClosure()
// (:4053-4116) from the candidate on: the inlier-ratio gate of isLoopClosure, the relative pose on
// the GPU (plba_lc_relative_pose), the loop lists and the LC_IDLE / LC_ACTIVE / LC_READY states;
// and of isLoopClosure (:4303-4411) from two keyframe indices, its descriptor matching
// (StVO::match, src2/matching.cpp:63-91) on the GPU (plba_desc_match).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>

#include "plslam_map.hpp"

namespace plslam {

Mat4 mul4(const Mat4 &A, const Mat4 &B) {
    Mat4 C{};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * B[k * 4 + j];
            C[i * 4 + j] = s;
        }
    return C;
}

namespace {

struct Quat {  // Eigen coefficient order is (x, y, z, w)
    double x, y, z, w;
};
// Eigen Quaternion(const Matrix3&)
Quat quat_from_R(const double *m) {
    Quat q;
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (m[7] - m[5]) * t;
        q.y = (m[2] - m[6]) * t;
        q.z = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        double v[3];
        v[i] = 0.5 * t;
        t = 0.5 / t;
        q.w = (m[3 * k + j] - m[3 * j + k]) * t;
        v[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        v[k] = (m[3 * k + i] + m[3 * i + k]) * t;
        q.x = v[0]; q.y = v[1]; q.z = v[2];
    }
    return q;
}
void R_from_quat(const Quat &q, double *R) {  // QuaternionBase::toRotationMatrix
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}
// g2o::SE3Quat: unit quaternion (w >= 0 after normalizeRotation) + translation
struct SE3Quat {
    Quat r;
    double t[3];
};
SE3Quat make_se3quat(Quat q, const double *t) {  // SE3Quat(q, t): normalizeRotation()
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    q.x /= n; q.y /= n; q.z /= n; q.w /= n;
    SE3Quat s;
    s.r = q;
    s.t[0] = t[0]; s.t[1] = t[1]; s.t[2] = t[2];
    return s;
}
void skew(const double *v, double *S) {
    S[0] = 0.0;   S[1] = -v[2]; S[2] = v[1];
    S[3] = v[2];  S[4] = 0.0;   S[5] = -v[0];
    S[6] = -v[1]; S[7] = v[0];  S[8] = 0.0;
}
void m3mul(const double *A, const double *B, double *C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += A[3 * i + k] * B[3 * k + j];
            C[3 * i + j] = s;
        }
}
// SE3Quat::exp(update), update = [ω; υ]
SE3Quat se3quat_exp(const double *u) {
    const double omega[3] = {u[0], u[1], u[2]}, upsilon[3] = {u[3], u[4], u[5]};
    const double theta = std::sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
    double Om[9], Om2[9], R[9], V[9];
    skew(omega, Om);
    m3mul(Om, Om, Om2);
    if (theta < 0.00001) {
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + Om[k] + Om2[k];
        for (int k = 0; k < 9; ++k) V[k] = R[k];
    } else {
        const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta);
        const double c = (theta - std::sin(theta)) / std::pow(theta, 3);
        for (int k = 0; k < 9; ++k) {
            const double I = (k % 4 == 0) ? 1.0 : 0.0;
            R[k] = I + a * Om[k] + b * Om2[k];
            V[k] = I + b * Om[k] + c * Om2[k];
        }
    }
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = V[3 * i] * upsilon[0] + V[3 * i + 1] * upsilon[1] + V[3 * i + 2] * upsilon[2];
    return make_se3quat(quat_from_R(R), t);
}
// SE3Quat::log() -> [ω; υ]
Vec6 se3quat_log(const SE3Quat &s) {
    double R[9];
    R_from_quat(s.r, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};  // deltaR
    double omega[3], Om[9], Om2[9], Vinv[9];
    if (std::fabs(d) > 0.99999) {
        for (int i = 0; i < 3; ++i) omega[i] = 0.5 * dR[i];
        skew(omega, Om);
        m3mul(Om, Om, Om2);
        for (int k = 0; k < 9; ++k) Vinv[k] = ((k % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[k] + (1. / 12.) * Om2[k];
    } else {
        const double theta = std::acos(d);
        for (int i = 0; i < 3; ++i) omega[i] = theta / (2 * std::sqrt(1 - d * d)) * dR[i];
        skew(omega, Om);
        m3mul(Om, Om, Om2);
        const double c = (1 - theta / (2 * std::tan(theta / 2))) / (theta * theta);
        for (int k = 0; k < 9; ++k) Vinv[k] = ((k % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[k] + c * Om2[k];
    }
    Vec6 res;
    for (int i = 0; i < 3; ++i) res[i] = omega[i];
    for (int i = 0; i < 3; ++i) res[3 + i] = Vinv[3 * i] * s.t[0] + Vinv[3 * i + 1] * s.t[1] + Vinv[3 * i + 2] * s.t[2];
    return res;
}
// (Isometry3) SE3Quat: R = rotation().toRotationMatrix(), t
void se3quat_to_iso(const SE3Quat &s, double *T12) {
    double R[9];
    R_from_quat(s.r, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T12[4 * r + c] = R[3 * r + c];
        T12[4 * r + 3] = s.t[r];
    }
}
// internal::toSE3Quat(Isometry3): SE3Quat(Quaternion(R), t)
SE3Quat iso_to_se3quat(const double *T12) {
    const double R[9] = {T12[0], T12[1], T12[2], T12[4], T12[5], T12[6], T12[8], T12[9], T12[10]};
    const double t[3] = {T12[3], T12[7], T12[11]};
    return make_se3quat(quat_from_R(R), t);
}
Vec6 reverse_se3(const Vec6 &x) {  // src2/auxiliar.cpp:199-204
    return Vec6{x[3], x[4], x[5], x[0], x[1], x[2]};
}
Vec3 xform(const Mat4 &T, const Vec3 &p) {  // T.block(0,0,3,3)·p + T.block(0,3,3,1)
    Vec3 o;
    for (int i = 0; i < 3; ++i) o[i] = T[4 * i] * p[0] + T[4 * i + 1] * p[1] + T[4 * i + 2] * p[2] + T[4 * i + 3];
    return o;
}

}  // namespace

int MapHandler::loopClosureOptimizationEssGraphG2O(PgoStats *stats) { return loopClosurePGO(true, stats); }
int MapHandler::loopClosureOptimizationCovGraphG2O(PgoStats *stats) { return loopClosurePGO(false, stats); }

int MapHandler::loopClosureOptimizationFuse(bool ess, PgoStats *stats, FuseStats *fs) {
    return loopClosurePGO(ess, stats, true, fs);
}

int MapHandler::loopClosurePGO(bool ess, PgoStats *stats, bool fuse, FuseStats *fs) {
    using clk = std::chrono::steady_clock;
    PgoStats st;
    // ---- the KF range (:5087-5097 / :5319-5330; the CovGraph variant then starts at KF 0)
    const std::vector<Vec3i> &range_list = ess ? lc_idxs : lc_idx_list;
    int kf_prev_idx = 2 * max_kf_idx, kf_curr_idx = -1;
    for (const Vec3i &l : range_list) {
        if (l[0] < kf_prev_idx) kf_prev_idx = l[0];
        if (l[1] > kf_curr_idx) kf_curr_idx = l[1];
    }
    if (!ess) kf_prev_idx = 0;
    st.kf_prev_idx = kf_prev_idx;
    st.kf_curr_idx = kf_curr_idx;
    const int nkf = (int)map_keyframes.size();
    if (kf_curr_idx >= nkf || (kf_curr_idx >= 0 && kf_prev_idx < 0)) {
        setError("loop closure: KF range [%d, %d] outside the map (%d KFs)", kf_prev_idx, kf_curr_idx, nkf);
        return PLBA_E_INVALID;
    }
    // ---- vertices (:5099-5141 / :5332-5370); the is_lc test walks the list the range came from
    std::vector<int> kf_list;
    std::vector<double> v_T;
    std::vector<uint8_t> v_fixed;
    std::map<int, int> vpos;
    for (int i = kf_prev_idx; i <= kf_curr_idx; ++i) {
        if (map_keyframes[i] == nullptr) continue;
        bool is_lc_i = false, is_lc_j = false;
        int id = 0;
        for (auto it = range_list.begin(); it != range_list.end(); ++it, ++id) {
            if ((*it)[0] == i) { is_lc_i = true; break; }
            if ((*it)[1] == i) { is_lc_j = true; break; }
        }
        kf_list.push_back(i);
        Vec6 x;
        bool fixed;
        if (is_lc_j) {
            // setFixed(ess); estimate = exp(reverse(log(expmap(lc_pose_list[id]) · T_{kf lc(0)})))
            const int src = range_list[id][0];
            if (id >= (int)lc_pose_list.size() || src < 0 || src >= nkf || map_keyframes[src] == nullptr) {
                setError("loop closure: lc_pose_list / source KF missing for loop %d", id);
                return PLBA_E_INVALID;
            }
            x = reverse_se3(logmap_se3(mul4(expmap_se3(lc_pose_list[id]), map_keyframes[src]->T_kf_w)));
            fixed = ess;
        } else {
            x = reverse_se3(map_keyframes[i]->x_kf_w);
            fixed = ess ? (is_lc_i || i == 0) : (i == 0);
        }
        double T12[12];
        se3quat_to_iso(se3quat_exp(x.data()), T12);
        vpos[i] = (int)v_fixed.size();
        v_T.insert(v_T.end(), T12, T12 + 12);
        v_fixed.push_back(fixed ? 1 : 0);
        st.n_fixed += fixed ? 1 : 0;
    }
    // ---- KF-to-KF edges (:5144-5164 / :5376-5396), then the loop edges (:5166-5179 / :5398-5411)
    std::vector<int32_t> e_v;
    std::vector<double> e_Z;
    auto add_edge = [&](int i, int j, const Vec6 &x) {
        double Z12[12];
        se3quat_to_iso(se3quat_exp(x.data()), Z12);
        e_v.push_back(vpos[i]);
        e_v.push_back(vpos[j]);
        e_Z.insert(e_Z.end(), Z12, Z12 + 12);
    };
    for (int i = kf_prev_idx; i <= kf_curr_idx; ++i)
        for (int j = i + 1; j <= kf_curr_idx; ++j) {
            if (map_keyframes[i] == nullptr || map_keyframes[j] == nullptr) continue;
            const unsigned fg = (size_t)i < full_graph.size() && (size_t)j < full_graph[i].size() ? full_graph[i][j] : 0u;
            const bool conn = ess ? (fg >= (unsigned)params.min_lm_ess_graph || std::abs(i - j) == 1)
                                  : (fg >= (unsigned)params.min_lm_ess_graph || fg >= (unsigned)params.min_lm_cov_graph ||
                                     std::abs(i - j) == 1);
            if (!conn) continue;
            const Mat4 T_ji = mul4(inverse_se3(map_keyframes[i]->T_kf_w), map_keyframes[j]->T_kf_w);
            add_edge(i, j, reverse_se3(logmap_se3(T_ji)));
        }
    st.n_edges = (int)e_v.size() / 2;
    {
        int id = 0;
        for (auto it = lc_idx_list.begin(); it != lc_idx_list.end(); ++it, ++id) {
            // optimizer.vertex() of a KF outside the graph is NULL: g2o refuses the edge
            if (!vpos.count((*it)[0]) || !vpos.count((*it)[1]) || id >= (int)lc_pose_list.size()) continue;
            add_edge((*it)[0], (*it)[1], reverse_se3(lc_pose_list[id]));
            ++st.n_loop_edges;
        }
    }
    st.n_vertices = (int)kf_list.size();
    // ---- initializeOptimization(); computeInitialGuess(); computeActiveErrors(); optimize(maxItersPGO)
    plba_pgo_graph g{};
    std::vector<int32_t> v_id(kf_list.begin(), kf_list.end());
    g.n_v = (int32_t)kf_list.size();
    g.n_e = (int32_t)e_v.size() / 2;
    g.v_id = v_id.data();
    g.v_T = v_T.data();
    g.v_fixed = v_fixed.data();
    g.e_v = e_v.data();
    g.e_Z = e_Z.data();
    g.e_info = nullptr;  // setInformation(Matrix6d::Identity())
    plba_pgo_params p;
    plba_pgo_default_params(&p);
    p.max_iters = params.max_iters_pgo;
    std::vector<double> v_out(v_T.size());
    plba_pgo_result r{};
    r.v_T = v_out.data();
    const auto t0 = clk::now();
    const int rc = backend(pgo_, "pose-graph solver", [&](plba_ctx *ctx) { return plba_pgo_optimize(ctx, &g, &p, &r); },
                           &g, &p, &r);
    if (rc) return rc;
    st.solve_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    st.iterations = r.iterations;
    st.trials = r.trials;
    st.chi2_initial = r.chi2_initial;
    st.chi2_final = r.chi2_final;
    // ---- recover poses and correct the map (:5187-5240)
    Mat4 Tkfw_corr{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // (uninitialised in the reference if no KF)
    auto correct_landmarks = [&](int kf) {
        auto pit = map_points_kf_idx.find(kf);  // .at() in the reference (throws when absent)
        if (pit != map_points_kf_idx.end())
            for (int idx : pit->second) {
                if (idx < 0 || idx >= (int)map_points.size() || map_points[idx] == nullptr) continue;
                MapPoint *mp = map_points[idx];
                mp->point3D = xform(Tkfw_corr, mp->point3D);
                markLandmarkChanged(1, idx);
                mp->med_obs_dir = xform(Tkfw_corr, mp->med_obs_dir);  // directions get the translation too
                for (Vec3 &d : mp->dir_list) d = xform(Tkfw_corr, d);
            }
        auto lit = map_lines_kf_idx.find(kf);
        if (lit != map_lines_kf_idx.end())
            for (int idx : lit->second) {
                if (idx < 0 || idx >= (int)map_lines.size() || map_lines[idx] == nullptr) continue;
                MapLine *ml = map_lines[idx];
                const Vec3 sP{ml->line3D[0], ml->line3D[1], ml->line3D[2]}, eP{ml->line3D[3], ml->line3D[4], ml->line3D[5]};
                const Vec3 sN = xform(Tkfw_corr, sP), eN = xform(Tkfw_corr, eP);
                for (int k = 0; k < 3; ++k) { ml->line3D[k] = sN[k]; ml->line3D[3 + k] = eN[k]; }
                ml->med_obs_dir = xform(Tkfw_corr, ml->med_obs_dir);
                for (Vec3 &d : ml->dir_list) d = xform(Tkfw_corr, d);
            }
    };
    for (size_t q = 0; q < kf_list.size(); ++q) {
        const int kf = kf_list[q];
        const SE3Quat Tiw_corr = iso_to_se3quat(&v_out[12 * q]);  // estimateAsSE3Quat()
        const Mat4 Tkfw = expmap_se3(reverse_se3(se3quat_log(Tiw_corr)));
        const Mat4 Tkfw_prev = map_keyframes[kf]->T_kf_w;
        map_keyframes[kf]->T_kf_w = Tkfw;
        map_keyframes[kf]->x_kf_w = logmap_se3(Tkfw);
        Tkfw_corr = mul4(Tkfw, inverse_se3(Tkfw_prev));
        correct_landmarks(kf);
    }
    // ---- the KFs after the loop (:5243-5287) take the last correction
    for (int i = kf_curr_idx + 1; i < nkf; ++i) {
        if (map_keyframes[i] == nullptr) continue;  // (dereferenced unchecked in the reference)
        map_keyframes[i]->T_kf_w = mul4(Tkfw_corr, map_keyframes[i]->T_kf_w);
        map_keyframes[i]->x_kf_w = logmap_se3(map_keyframes[i]->T_kf_w);
        correct_landmarks(i);
    }
    // loopClosureFuseLandmarks() (:5294 / :5526), for loopClosureOptimizationFuse. The reference calls it
    // after it has cleared the flags, so its own call finds no loop with flag 1; here it runs while the
    // flags still name the loops of this optimisation (fuse_landmarks.cpp). A refused fuse leaves the
    // flags and lc_state as they are: the map is corrected and not fused.
    if (fuse) {
        if (stats) *stats = st;
        if (const int frc = fuseLandmarks(fs)) return frc;
    }
    for (Vec3i &l : lc_idx_list) l[2] = 0;  // mark as optimised (:5290-5292)
    lc_state = 0;                            // LC_IDLE (:5296)
    if (stats) *stats = st;
    return PLBA_OK;
}

// MapHandler::loopClosure() (src/mapHandler.cpp:4053-4116) from the candidate on, with the tail of
// isLoopClosure (:4382-4409) and computeRelativePoseRobustGN (:4677-5068, on the GPU) inside.
int MapHandler::loopClosureStep(const LcCandidate *c, double lc_inlier_ratio, LcStats *stats) {
    using clk = std::chrono::steady_clock;
    LcStats st;
    st.state_before = lc_state;
    bool isLC = false;
    if (c) {
        st.is_candidate = 1;
        if (c->n_pt < 0 || c->n_ln < 0 || (c->n_pt && (!c->pt_P || !c->pt_obs)) ||
            (c->n_ln && (!c->ln_sP || !c->ln_eP || !c->ln_le))) {
            setError("loop closure: candidate with negative counts or NULL feature arrays");
            return PLBA_E_INVALID;
        }
        int common_pt, common_ls;
        const bool cond = inlierRatioGate(*c, lc_inlier_ratio, common_pt, common_ls, st.inl_ratio_pt, st.inl_ratio_ls);
        st.ratio_ok = cond ? 1 : 0;
        if (cond) {
            const int32_t pt_off[2] = {0, common_pt}, ln_off[2] = {0, common_ls};
            plba_lcpose_batch b{};
            b.n = 1;
            b.pt_off = pt_off;
            b.ln_off = ln_off;
            b.pt_P = c->pt_P; b.pt_obs = c->pt_obs;
            b.ln_sP = c->ln_sP; b.ln_eP = c->ln_eP; b.ln_le = c->ln_le;
            b.fx = fx_; b.fy = fy_; b.cx = cx_; b.cy = cy_;
            plba_lcpose_out o{};
            std::vector<uint8_t> pin((size_t)std::max(common_pt, 1), 0), lin((size_t)std::max(common_ls, 1), 0);
            const auto t0 = clk::now();
            const int rc = lcRelativePose(b, &o, pin.data(), lin.data());
            if (rc) return rc;
            st.pose_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
            st.accepted = o.accepted;
            st.conditions = o.conditions;
            st.n_inl_pt = o.n_inl_pt; st.n_inl_ln = o.n_inl_ln;
            st.e = o.e; st.unc = o.unc; st.t = o.t; st.r_deg = o.r_deg;
            isLC = o.accepted != 0;
            if (isLC) {
                // the outliers leave lc_pt_idx / lc_ls_idx (:5025-5056); the rows are kept for the
                // landmark fusion (:4078-4079)
                std::vector<Vec4i> pt_rows, ls_rows;
                for (int i = 0; i < common_pt && c->pt_idx; ++i)
                    if (pin[i]) pt_rows.push_back(Vec4i{c->pt_idx[4 * i], c->pt_idx[4 * i + 1], c->pt_idx[4 * i + 2], c->pt_idx[4 * i + 3]});
                for (int i = 0; i < common_ls && c->ls_idx; ++i)
                    if (lin[i]) ls_rows.push_back(Vec4i{c->ls_idx[4 * i], c->ls_idx[4 * i + 1], c->ls_idx[4 * i + 2], c->ls_idx[4 * i + 3]});
                lc_pt_idxs.push_back(std::move(pt_rows));
                lc_ls_idxs.push_back(std::move(ls_rows));
                Vec6 pose_inc;
                for (int k = 0; k < 6; ++k) pose_inc[k] = o.pose_inc[k];
                lc_poses.push_back(pose_inc);
                lc_pose_list.push_back(pose_inc);
                const Vec3i lc_idx{c->kf_prev_idx, c->kf_curr_idx, 1};
                lc_idxs.push_back(lc_idx);
                lc_idx_list.push_back(lc_idx);
            }
        }
    }
    if (isLC) {
        if (lc_state == LC_IDLE) lc_state = LC_ACTIVE;
    } else {
        if (lc_state == LC_ACTIVE) lc_state = LC_READY;
    }
    if (lc_state == LC_READY) {  // (:4109-4115)
        const int rc = loopClosureOptimizationCovGraphG2O(&st.pgo);
        if (rc) return rc;
        st.pgo_ran = 1;
        lc_state = LC_IDLE;
    }
    st.state_after = lc_state;
    if (stats) *stats = st;
    return PLBA_OK;
}

// The tail of isLoopClosure before the relative pose (:4384-4402).
bool MapHandler::inlierRatioGate(const LcCandidate &c, double lc_inlier_ratio, int &common_pt, int &common_ls,
                                 double &ratio_pt, double &ratio_ls) {
    // the matching runs only for an enabled kind with features in both keyframes (:4331, :4357)
    const bool use_pt = c.has_points && c.n_pt_0 > 0 && c.n_pt_1 > 0;
    const bool use_ls = c.has_lines && c.n_ls_0 > 0 && c.n_ls_1 > 0;
    common_pt = use_pt ? c.n_pt : 0;
    common_ls = use_ls ? c.n_ln : 0;
    // :4384-4385 — a zero count gives NaN or 0 here, and the comparisons below are then false
    ratio_pt = std::max(100.0 * common_pt / c.n_pt_0, 100.0 * common_pt / c.n_pt_1);
    ratio_ls = std::max(100.0 * common_ls / c.n_ls_0, 100.0 * common_ls / c.n_ls_1);
    if (c.has_points && c.has_lines) return ratio_pt > lc_inlier_ratio && ratio_ls > lc_inlier_ratio;
    if (c.has_points) return ratio_pt > lc_inlier_ratio;
    if (c.has_lines) return ratio_ls > lc_inlier_ratio;
    return false;
}

int MapHandler::lcRelativePose(const plba_lcpose_batch &b, plba_lcpose_out *out, uint8_t *pin, uint8_t *lin) {
    return backend(lcpose_, "relative-pose solver",
                   [&](plba_ctx *ctx) { return plba_lc_relative_pose(ctx, &b, &lcpose_params, out, pin, lin); },
                   &b, &lcpose_params, out, pin, lin);
}

// What isLoopClosure holds after its matching (:4327-4380) for one pair of keyframes.
struct MapHandler::LcBuilt {
    std::vector<double> pt_P, pt_obs, ln_sP, ln_eP, ln_le;
    std::vector<int32_t> pt_idx, ls_idx;
    int n_pt_0 = 0, n_pt_1 = 0, n_ls_0 = 0, n_ls_1 = 0, common_pt = 0, common_ls = 0;
    LcCandidate candidate(int kf0, int kf1, const MatchParams &mp) const {
        LcCandidate c;
        c.kf_prev_idx = kf0; c.kf_curr_idx = kf1;
        c.n_pt_0 = n_pt_0; c.n_pt_1 = n_pt_1; c.n_ls_0 = n_ls_0; c.n_ls_1 = n_ls_1;
        c.has_points = mp.has_points; c.has_lines = mp.has_lines;
        c.n_pt = common_pt; c.n_ln = common_ls;
        c.pt_P = pt_P.data(); c.pt_obs = pt_obs.data();
        c.ln_sP = ln_sP.data(); c.ln_eP = ln_eP.data(); c.ln_le = ln_le.data();
        c.pt_idx = pt_idx.data(); c.ls_idx = ls_idx.data();
        return c;
    }
};

int MapHandler::buildLoopCandidates(int kf1_idx, int n, const int32_t *kf_prev_idx, const MatchParams &mp,
                                    std::vector<LcBuilt> &out) {
    auto frame = [&](int idx) -> const StereoFrame * {
        if (idx < 0 || idx >= (int)map_keyframes.size() || !map_keyframes[idx]) return nullptr;
        const StereoFrame &f = map_keyframes[idx]->stereo_frame;
        return f.has_features ? &f : nullptr;
    };
    const StereoFrame *f1 = frame(kf1_idx);
    if (n < 0 || (n && !kf_prev_idx) || !f1) {
        setError("loop closure: keyframe %d does not exist or has no features set", kf1_idx);
        return PLBA_E_INVALID;
    }
    for (int k = 0; k < n; ++k) {
        const StereoFrame *f0 = frame(kf_prev_idx[k]);
        if (!f0 || f0->desc_bytes != f1->desc_bytes) {
            setError("loop closure: keyframe %d does not exist, has no features set or has descriptors of another size",
                     kf_prev_idx[k]);
            return PLBA_E_INVALID;
        }
    }
    out.assign((size_t)n, LcBuilt{});
    if (n == 0) return PLBA_OK;
    // pairs 2k (points) and 2k + 1 (lines) of candidate k; desc1 = kf0 (:4334, :4360). A kind that
    // is disabled or empty on either side is not matched (:4331, :4357): an empty pair.
    const size_t db = (size_t)f1->desc_bytes;
    const int n_pt_1 = (int)f1->stereo_pt_idx.size(), n_ls_1 = (int)f1->stereo_ls_idx.size();
    std::vector<int32_t> off1(2 * (size_t)n + 1, 0), off2(2 * (size_t)n + 1, 0), cnt(2 * (size_t)n, 0);
    std::vector<float> nnr(2 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        const StereoFrame &f0 = *frame(kf_prev_idx[k]);
        const int n_pt_0 = (int)f0.stereo_pt_idx.size(), n_ls_0 = (int)f0.stereo_ls_idx.size();
        const bool use_pt = mp.has_points && n_pt_0 > 0 && n_pt_1 > 0, use_ls = mp.has_lines && n_ls_0 > 0 && n_ls_1 > 0;
        off1[2 * k + 1] = off1[2 * k] + (use_pt ? n_pt_0 : 0);
        off2[2 * k + 1] = off2[2 * k] + (use_pt ? n_pt_1 : 0);
        off1[2 * k + 2] = off1[2 * k + 1] + (use_ls ? n_ls_0 : 0);
        off2[2 * k + 2] = off2[2 * k + 1] + (use_ls ? n_ls_1 : 0);
        nnr[2 * k] = mp.min_ratio_12_p;
        nnr[2 * k + 1] = mp.min_ratio_12_l;
    }
    std::vector<uint8_t> d1((size_t)off1[2 * n] * db + 1), d2((size_t)off2[2 * n] * db + 1);
    for (int k = 0; k < n; ++k) {
        const StereoFrame &f0 = *frame(kf_prev_idx[k]);
        if (off1[2 * k + 1] > off1[2 * k]) {
            std::memcpy(&d1[(size_t)off1[2 * k] * db], f0.pdesc_l.data(), f0.pdesc_l.size());
            std::memcpy(&d2[(size_t)off2[2 * k] * db], f1->pdesc_l.data(), f1->pdesc_l.size());
        }
        if (off1[2 * k + 2] > off1[2 * k + 1]) {
            std::memcpy(&d1[(size_t)off1[2 * k + 1] * db], f0.ldesc_l.data(), f0.ldesc_l.size());
            std::memcpy(&d2[(size_t)off2[2 * k + 1] * db], f1->ldesc_l.data(), f1->ldesc_l.size());
        }
    }
    std::vector<int32_t> m12((size_t)off1[2 * n] + 1, -1);
    plba_match_batch b{};
    b.n = 2 * n;
    b.desc_bytes = (int32_t)db;
    b.off1 = off1.data(); b.off2 = off2.data();
    b.desc1 = d1.data(); b.desc2 = d2.data();
    b.nnr = nnr.data();
    b.best_lr = mp.best_lr ? 1 : 0;
    const int rc = backend(match_, "matcher", [&](plba_ctx *ctx) { return plba_desc_match(ctx, &b, m12.data(), cnt.data()); },
                           &b, m12.data(), cnt.data());
    if (rc) return rc;
    for (int k = 0; k < n; ++k) {
        const StereoFrame &f0 = *frame(kf_prev_idx[k]);
        LcBuilt &o = out[k];
        o.n_pt_0 = (int)f0.stereo_pt_idx.size(); o.n_pt_1 = n_pt_1;
        o.n_ls_0 = (int)f0.stereo_ls_idx.size(); o.n_ls_1 = n_ls_1;
        o.common_pt = cnt[2 * k];      // match()'s return value (:4334)
        o.common_ls = cnt[2 * k + 1];  // (:4360)
        for (int i1 = 0; i1 < off1[2 * k + 1] - off1[2 * k]; ++i1) {  // (:4336-4352)
            const int i2 = m12[off1[2 * k] + i1];
            if (i2 < 0) continue;
            o.pt_P.insert(o.pt_P.end(), &f0.pt_P[3 * i1], &f0.pt_P[3 * i1] + 3);
            o.pt_obs.insert(o.pt_obs.end(), &f1->pt_pl[2 * i2], &f1->pt_pl[2 * i2] + 2);
            const int32_t row[4] = {f0.stereo_pt_idx[i1], i1, f1->stereo_pt_idx[i2], i2};
            o.pt_idx.insert(o.pt_idx.end(), row, row + 4);
        }
        for (int i1 = 0; i1 < off1[2 * k + 2] - off1[2 * k + 1]; ++i1) {  // (:4362-4379)
            const int i2 = m12[off1[2 * k + 1] + i1];
            if (i2 < 0) continue;
            o.ln_sP.insert(o.ln_sP.end(), &f0.ls_sP[3 * i1], &f0.ls_sP[3 * i1] + 3);
            o.ln_eP.insert(o.ln_eP.end(), &f0.ls_eP[3 * i1], &f0.ls_eP[3 * i1] + 3);
            o.ln_le.insert(o.ln_le.end(), &f1->ls_le[3 * i2], &f1->ls_le[3 * i2] + 3);
            const int32_t row[4] = {f0.stereo_ls_idx[i1], i1, f1->stereo_ls_idx[i2], i2};
            o.ls_idx.insert(o.ls_idx.end(), row, row + 4);
        }
        if ((int)o.pt_idx.size() != 4 * o.common_pt || (int)o.ls_idx.size() != 4 * o.common_ls) {
            setError("matcher: the counts of candidate %d do not equal its matches", k);
            return PLBA_E_INVALID;
        }
    }
    return PLBA_OK;
}

int MapHandler::isLoopClosure(int kf0_idx, int kf1_idx, const MatchParams &mp, double lc_inlier_ratio, LcStats *stats) {
    std::vector<LcBuilt> built;
    const int32_t prev = kf0_idx;
    const int rc = buildLoopCandidates(kf1_idx, 1, &prev, mp, built);
    if (rc) return rc;
    const LcCandidate c = built[0].candidate(kf0_idx, kf1_idx, mp);
    return loopClosureStep(&c, lc_inlier_ratio, stats);
}

int MapHandler::verifyLoopCandidates(int kf_curr_idx, int n, const int32_t *kf_prev_idx, const MatchParams &mp,
                                     double lc_inlier_ratio, int32_t *accepted, double *pose_inc, int32_t *n_matches) {
    std::vector<LcBuilt> built;
    int rc = buildLoopCandidates(kf_curr_idx, n, kf_prev_idx, mp, built);
    if (rc) return rc;
    for (int k = 0; k < n; ++k) {
        if (accepted) accepted[k] = 0;
        for (int j = 0; j < 6 && pose_inc; ++j) pose_inc[6 * k + j] = 0.0;
        if (n_matches) {
            n_matches[2 * k] = built[k].common_pt;
            n_matches[2 * k + 1] = built[k].common_ls;
        }
    }
    // the candidates that pass the gate, concatenated for one relative-pose call
    std::vector<int> passed;
    std::vector<int32_t> pt_off{0}, ln_off{0};
    std::vector<double> P, obs, sP, eP, le;
    for (int k = 0; k < n; ++k) {
        const LcBuilt &o = built[k];
        const LcCandidate c = o.candidate(kf_prev_idx[k], kf_curr_idx, mp);
        int common_pt, common_ls;
        double rp, rl;
        if (!inlierRatioGate(c, lc_inlier_ratio, common_pt, common_ls, rp, rl)) continue;
        passed.push_back(k);
        P.insert(P.end(), o.pt_P.begin(), o.pt_P.begin() + 3 * common_pt);
        obs.insert(obs.end(), o.pt_obs.begin(), o.pt_obs.begin() + 2 * common_pt);
        sP.insert(sP.end(), o.ln_sP.begin(), o.ln_sP.begin() + 3 * common_ls);
        eP.insert(eP.end(), o.ln_eP.begin(), o.ln_eP.begin() + 3 * common_ls);
        le.insert(le.end(), o.ln_le.begin(), o.ln_le.begin() + 3 * common_ls);
        pt_off.push_back(pt_off.back() + common_pt);
        ln_off.push_back(ln_off.back() + common_ls);
    }
    if (passed.empty()) return PLBA_OK;
    plba_lcpose_batch b{};
    b.n = (int32_t)passed.size();
    b.pt_off = pt_off.data(); b.ln_off = ln_off.data();
    b.pt_P = P.data(); b.pt_obs = obs.data();
    b.ln_sP = sP.data(); b.ln_eP = eP.data(); b.ln_le = le.data();
    b.fx = fx_; b.fy = fy_; b.cx = cx_; b.cy = cy_;
    std::vector<plba_lcpose_out> o(passed.size());
    std::vector<uint8_t> pin((size_t)pt_off.back() + 1, 0), lin((size_t)ln_off.back() + 1, 0);
    rc = lcRelativePose(b, o.data(), pin.data(), lin.data());
    if (rc) return rc;
    for (size_t j = 0; j < passed.size(); ++j) {
        if (!o[j].accepted) continue;
        if (accepted) accepted[passed[j]] = 1;
        for (int i = 0; i < 6 && pose_inc; ++i) pose_inc[6 * passed[j] + i] = o[j].pose_inc[i];
    }
    return PLBA_OK;
}

// tools/descmatch_bench.py only: the semantics of plba_desc_match (include/plba.h) restated with
// popcounts, single-threaded. Not a product path.
int descMatchCpu(const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches) {
    if (!b || b->n < 0 || b->desc_bytes < 4 || b->desc_bytes > 64 || b->desc_bytes % 4) return PLBA_E_INVALID;
    const int dw = b->desc_bytes / 4;
    auto nearest = [&](const uint8_t *q, int nq, const uint8_t *t, int nt, float nnr, std::vector<int32_t> &m) {
        m.assign((size_t)nq, -1);
        for (int i = 0; i < nq && nt >= 2; ++i) {
            int d0 = INT_MAX, d1 = INT_MAX, i0 = -1;
            for (int j = 0; j < nt; ++j) {
                int d = 0;
                for (int c = 0; c < dw; ++c) {
                    uint32_t x, y;
                    std::memcpy(&x, q + (size_t)i * b->desc_bytes + 4 * c, 4);
                    std::memcpy(&y, t + (size_t)j * b->desc_bytes + 4 * c, 4);
                    d += __builtin_popcount(x ^ y);
                }
                if (d < d0) { d1 = d0; d0 = d; i0 = j; }
                else if (d < d1) d1 = d;
            }
            const float lhs = (float)d0, rhs = (float)d1 * nnr;
            if (lhs < rhs) m[i] = i0;
        }
    };
    std::vector<int32_t> m12, m21;
    for (int k = 0; k < b->n; ++k) {
        const int o1 = b->off1[k], n1 = b->off1[k + 1] - o1, o2 = b->off2[k], n2 = b->off2[k + 1] - o2;
        const uint8_t *a = b->desc1 + (size_t)o1 * b->desc_bytes, *c = b->desc2 + (size_t)o2 * b->desc_bytes;
        nearest(a, n1, c, n2, b->nnr[k], m12);
        if (b->best_lr) nearest(c, n2, a, n1, b->nnr[k], m21);
        int cnt = 0;
        for (int i1 = 0; i1 < n1; ++i1) {
            int i2 = m12[i1];
            if (b->best_lr && i2 >= 0 && m21[i2] != i1) i2 = -1;
            matches_12[o1 + i1] = i2;
            cnt += i2 >= 0;
        }
        n_matches[k] = cnt;
    }
    return PLBA_OK;
}

}  // namespace plslam
