// trackPoseCpu: a single-threaded restatement of plba_track_pose's semantics (include/plba.h;
// StereoFrameHandler::optimizePose, src2/stereoFrameHandler.cpp:307-405) with its signature, for the
// tests and tools/trackpose_bench.py (not a product path). The arithmetic of a match and the small
// dense routines are those of the kernel (csrc/plba_trackpose_geom.hpp, csrc/plba_posegn.hpp); H, g
// and e are summed in match order, points then lines, and the medians come from sorted lists. This
// file is compiled without contraction.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../csrc/plba_trackpose_geom.hpp"
#include "plslam_map.hpp"

namespace plslam {

namespace {

using namespace plba;

struct TpCam {
    double fx, fy, cx, cy;
};

// vector_stdv_mad without its factor (src2/auxiliar.cpp:444-460): an empty list gives 0
double mad_of(std::vector<double> v, double *median = nullptr) {
    if (v.empty()) return 0.0;
    const size_t n = v.size();
    std::sort(v.begin(), v.end());
    const double med = v[n / 2];
    for (double &r : v) r = tpg::mad_dev(r, med);
    std::sort(v.begin(), v.end());
    if (median) *median = med;
    return v[n / 2];
}

const Mat4 kIdentity{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

struct Problem {
    const plba_track_batch *b;
    const plba_track_params *prm;
    TpCam cam;
    int p0, np, l0, nl;
    uint8_t *pin, *lin;
    bool pluker;
    // the state of optimizePose
    Mat4 T, T0;
    double H[36], cov[36], err, s_p, s_l;
    int iters[2];
    pgn::Work w;

    double point(const double *T_, int i, double *G, double &dx, double &dy) const {
        const size_t q = (size_t)(p0 + i);
        return tpg::point_res(cam, T_, b->pt_P + 3 * q, b->pt_obs + 2 * q, G, dx, dy);
    }
    // the line residual of the model; the projected endpoints and (Plücker) L for the row
    double line(const double *T_, int i, double *Gs, double *Ge, double *ps, double *pe, tpg::PlLine &L, double &ds,
                double &de) const {
        const size_t q = (size_t)(l0 + i);
        tpg::line_proj(cam, T_, b->ln_sP + 3 * q, b->ln_eP + 3 * q, Gs, Ge, ps, pe);
        if (pluker) return tpg::line_res_pl(cam, T_, b->ln_NDc + 6 * q, b->ln_obs + 4 * q, L);
        return tpg::line_res_ep(b->ln_le + 3 * q, ps, pe, ds, de);
    }

    void loop(int cap, int phase) {  // :446-494 / :803-853
        double err_prev = 999999999.9, e_last = 0.0;
        bool bad = false;
        const double hth = prm->homog_th;
        for (int it = 0; it < cap; ++it) {
            const double *T_ = T.data();
            std::vector<double> rp, rl;
            double G[3], Gs[3], Ge[3], ps[2], pe[2], dx, dy, ds, de, J[6];
            tpg::PlLine L;
            for (int i = 0; i < np; ++i)
                if (pin[i]) rp.push_back(point(T_, i, G, dx, dy));
            for (int i = 0; i < nl; ++i)
                if (lin[i]) rl.push_back(line(T_, i, Gs, Ge, ps, pe, L, ds, de));
            s_p = tpg::clamp_scale(mad_of(rp));
            s_l = tpg::clamp_scale(mad_of(rl));
            double acc[tpg::kAcc] = {0};
            for (int i = 0; i < np; ++i) {
                if (!pin[i]) continue;
                const double r = point(T_, i, G, dx, dy);
                tpg::point_row(cam, hth, G, dx, dy, r, J);
                tpg::accumulate(acc, J, r, r, tpg::cauchy(r, s_p));
            }
            for (int i = 0; i < nl; ++i) {
                if (!lin[i]) continue;
                const size_t q = (size_t)(l0 + i);
                const double r = line(T_, i, Gs, Ge, ps, pe, L, ds, de);
                double rg = r;
                if (pluker) {
                    tpg::line_row_pl(cam, hth, T_, b->ln_obs + 4 * q, L, r, J);
                    rg = r * sqrt(b->ln_sigma2[q]);
                } else {
                    tpg::line_row_ep(cam, hth, Gs, Ge, b->ln_le + 3 * q, ds, de, r, J);
                }
                const double wgt = tpg::cauchy(r, s_l) * st_overlap2d(b->ln_seg + 4 * q, b->ln_seg + 4 * q + 2, ps, pe);
                tpg::accumulate(acc, J, rg, r, wgt);
            }
            ++iters[phase];
            double g[6];
            for (int i = 0, q = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j, ++q) H[6 * i + j] = H[6 * j + i] = acc[q];
            for (int i = 0; i < 6; ++i) g[i] = acc[21 + i];
            const double e = acc[27] / acc[28];
            e_last = e;
            if (acc[28] == 0.0 || fabs(e - err_prev) < prm->min_error_change || e < prm->min_error) break;
            double x[6], logdet;
            pgn::qr_solve(H, g, x, w, &logdet);
            if (logdet < 0.0) {
                bad = true;
                break;
            }
            T = mul4(inverse_se3(expmap_se3(Vec6{x[0], x[1], x[2], x[3], x[4], x[5]})), T);
            double n2 = 0.0;
            for (int k = 0; k < 6; ++k) n2 += x[k] * x[k];
            if (sqrt(n2) < prm->min_error_change) break;
            err_prev = e;
        }
        if (!bad) {
            pgn::inverse6(H, cov, w);
            err = e_last;
        } else {
            T = T0;
            for (int k = 0; k < 36; ++k) cov[k] = (k % 7 == 0) ? 1.0 : 0.0;
            err = -1.0;
        }
    }

    bool good(const double *DT, double e) {
        double ev[6];
        pgn::eig6_sorted(cov, ev, w);
        return tpg::is_good(ev, e, DT);
    }

    void remove_outliers() {  // :1303-1396
        const double *T_ = T.data();
        for (int kind = 0; kind < 2; ++kind) {
            if (!(kind ? prm->has_lines : prm->has_points)) continue;
            const int n = kind ? nl : np;
            uint8_t *in = kind ? lin : pin;
            std::vector<double> res(n);
            double G[3], Gs[3], Ge[3], ps[2], pe[2], dx, dy, ds, de;
            tpg::PlLine L;
            for (int i = 0; i < n; ++i)
                res[i] = kind ? line(T_, i, Gs, Ge, ps, pe, L, ds, de) * sqrt(b->ln_sigma2[l0 + i])
                              : point(T_, i, G, dx, dy) * sqrt(b->pt_sigma2[p0 + i]);
            // vector_mean_stdv_mad (src2/auxiliar.cpp:387-430)
            const double stdv = 1.4826 * mad_of(res);
            double mean = 0.0, all = 0.0;
            int k = 0;
            for (int i = 0; i < n; ++i) {
                if (res[i] < 2.0 * stdv) {
                    mean += res[i];
                    ++k;
                }
                all += res[i];
            }
            if (n) mean = (k >= (int)(0.2 * (double)n)) ? mean / (double)k : all / (double)n;
            const double th = prm->inlier_k * stdv;
            for (int i = 0; i < n; ++i)
                if (in[i] && fabs(res[i] - mean) > th) in[i] = 0;
        }
    }

    void solve(plba_track_out &o, int prob) {
        T0 = kIdentity;
        for (int k = 0; k < 36; ++k) H[k] = cov[k] = 0.0;
        err = -1.0, s_p = s_l = 0.0, iters[0] = iters[1] = 0;
        if (prm->use_motion_model) {  // :317-324
            const double *pv = b->prev + (size_t)53 * prob;
            for (int k = 0; k < 36; ++k) cov[k] = pv[16 + k];
            if (good(pv, pv[52]))
                for (int k = 0; k < 16; ++k) T0[k] = pv[k];
        }
        T = T0;
        for (int i = 0; i < np; ++i) pin[i] = 1;
        for (int i = 0; i < nl; ++i) lin[i] = 1;
        int branch = PLBA_TRACK_OK;
        auto inliers = [&] { return (int)(std::count(pin, pin + np, 1) + std::count(lin, lin + nl, 1)); };
        if (np + nl < prm->min_features) {
            branch = PLBA_TRACK_FEW_BEFORE;
            T = kIdentity;
        } else {
            loop(prm->max_iters, 0);
            if (good(T.data(), err)) {
                remove_outliers();
                T = T0;
                if (inliers() >= prm->min_features) {
                    loop(prm->max_iters_ref, 1);
                } else {
                    branch = PLBA_TRACK_FEW_AFTER;
                    T = kIdentity;
                }
            } else {
                branch = PLBA_TRACK_FIRST_NOT_GOOD;
                T = T0;
                if (!pluker) loop(prm->max_iters_ref, 1);
            }
        }
        double ev[6];
        pgn::eig6_sorted(cov, ev, w);
        if (tpg::is_good(ev, err, T.data()) && T != kIdentity) {
            const Mat4 DT = expmap_se3(logmap_se3(inverse_se3(T)));
            for (int k = 0; k < 16; ++k) o.DT[k] = DT[k];
            for (int k = 0; k < 36; ++k) o.DT_cov[k] = cov[k];
            for (int k = 0; k < 6; ++k) o.DT_cov_eig[k] = ev[k];
            o.err_norm = err;
        } else {
            for (int k = 0; k < 16; ++k) o.DT[k] = kIdentity[k];
            for (int k = 0; k < 36; ++k) o.DT_cov[k] = 0.0;
            for (int k = 0; k < 6; ++k) o.DT_cov_eig[k] = 0.0;
            o.err_norm = -1.0;
            if (branch == PLBA_TRACK_OK) branch = PLBA_TRACK_FINAL_NOT_GOOD;
        }
        o.branch = branch;
        o.iters_first = iters[0];
        o.iters_ref = iters[1];
        o.n_inl_pt = (int)std::count(pin, pin + np, 1);
        o.n_inl_ln = (int)std::count(lin, lin + nl, 1);
        o.pad = 0;
        o.s_p = s_p;
        o.s_l = s_l;
        for (int k = 0; k < 16; ++k) o.DT_solver[k] = T[k];
        for (int k = 0; k < 36; ++k) o.H[k] = H[k];
    }
};

}  // namespace

int trackPoseCpu(const plba_track_batch *b, const plba_track_params *pp, plba_track_out *out, uint8_t *pt_inlier,
                 uint8_t *ln_inlier) {
    if (!b || b->n < 0) return PLBA_E_INVALID;
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    plba_track_params prm;
    if (pp) prm = *pp;
    else plba_track_default_params(&prm);
    // what plba_track_pose refuses is refused here
    if (!out || !b->pt_off || !b->ln_off) return PLBA_E_INVALID;
    if ((prm.line_model != PLBA_TRACK_PLUCKER && prm.line_model != PLBA_TRACK_ENDPOINTS) || prm.max_iters < 1 ||
        prm.max_iters_ref < 1)
        return PLBA_E_INVALID;
    const bool pluker = prm.line_model == PLBA_TRACK_PLUCKER;
    for (const int32_t *off : {b->pt_off, b->ln_off}) {
        if (off[0] < 0) return PLBA_E_INVALID;
        for (int k = 0; k < n; ++k)
            if (off[k + 1] < off[k] || off[k + 1] - off[k] > PLBA_TRACK_MAX_N) return PLBA_E_INVALID;
    }
    const size_t np = (size_t)b->pt_off[n], nl = (size_t)b->ln_off[n];
    if ((np && (!b->pt_P || !b->pt_obs || !b->pt_sigma2)) ||
        (nl && (!b->ln_sP || !b->ln_eP || !b->ln_seg || !b->ln_sigma2 || (pluker ? (!b->ln_NDc || !b->ln_obs) : !b->ln_le))))
        return PLBA_E_INVALID;
    if (prm.use_motion_model && !b->prev) return PLBA_E_INVALID;
    std::vector<uint8_t> pin(np + 1), lin(nl + 1);
    for (int k = 0; k < n; ++k) {
        Problem P{};
        P.b = b, P.prm = &prm, P.cam = TpCam{b->fx, b->fy, b->cx, b->cy}, P.pluker = pluker;
        P.p0 = b->pt_off[k], P.np = b->pt_off[k + 1] - P.p0, P.l0 = b->ln_off[k], P.nl = b->ln_off[k + 1] - P.l0;
        P.pin = pin.data() + P.p0, P.lin = lin.data() + P.l0;
        P.solve(out[k], k);
    }
    if (pt_inlier && np) std::copy(pin.begin(), pin.begin() + np, pt_inlier);
    if (ln_inlier && nl) std::copy(lin.begin(), lin.begin() + nl, ln_inlier);
    return PLBA_OK;
}

}  // namespace plslam
