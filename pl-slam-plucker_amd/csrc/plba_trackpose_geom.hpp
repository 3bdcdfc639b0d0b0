// plba_trackpose_geom.hpp — the per-match arithmetic of plba_track_pose (include/plba.h), restated
// from src2/stereoFrameHandler.cpp: the residuals and Jacobian rows of optimizeFunctionsRobust
// (:1010-1277, the endpoint line model) and optimizeFunctionsUsingPluker (:564-801), the pieces of the
// MAD scale (src2/auxiliar.cpp:444-460) and isGoodSolution (:292-305). Plain C++ with no HIP type,
// compiled for the device by csrc/plba_trackpose.hpp and for the host by host/track_pose.cpp
// (plslam_track_pose_cpu), so that both evaluate the same expressions; every function switches
// contraction off.
#pragma once

#include "plba_posegn.hpp"
#include "plba_stereo_geom.hpp"  // st_overlap2d

namespace plba {
namespace tpg {

constexpr int kAcc = 29;  // 21 upper entries of H | 6 of g | e | active count

// point residual (dx, dy), ‖·‖ and the moved point (:1103-1107)
template <typename CamT>
PLBA_PGN_FN double point_res(const CamT &c, const double *T, const double *P, const double *obs, double *G, double &dx,
                             double &dy) {
    PLBA_PGN_EXACT
    pgn::xform(T, P, G);
    double u, v;
    pgn::project(c, G, u, v);
    dx = u - obs[0];
    dy = v - obs[1];
    return sqrt(dx * dx + dy * dy);
}

// J_aux of a point (:1117-1124)
template <typename CamT>
PLBA_PGN_FN void point_row(const CamT &c, double hth, const double *G, double dx, double dy, double r, double *J) {
    PLBA_PGN_EXACT
    pgn::jrow(c, hth, G, dx, dy, J);
    const double m = fmax(hth, r);
    for (int k = 0; k < 6; ++k) J[k] = J[k] / m;
}

// The projected endpoints of a line (:1192-1195): both models need them for the overlap
template <typename CamT>
PLBA_PGN_FN void line_proj(const CamT &c, const double *T, const double *sP, const double *eP, double *Gs, double *Ge,
                           double *ps, double *pe) {
    PLBA_PGN_EXACT
    pgn::xform(T, sP, Gs);
    pgn::xform(T, eP, Ge);
    pgn::project(c, Gs, ps[0], ps[1]);
    pgn::project(c, Ge, pe[0], pe[1]);
}

// endpoint model: the distances of the projected endpoints to the observed line (:1198-1201)
PLBA_PGN_FN double line_res_ep(const double *le, const double *ps, const double *pe, double &ds, double &de) {
    PLBA_PGN_EXACT
    ds = le[0] * ps[0] + le[1] * ps[1] + le[2];
    de = le[0] * pe[0] + le[1] * pe[1] + le[2];
    return sqrt(ds * ds + de * de);
}

// endpoint model: J_aux (:1204-1234)
template <typename CamT>
PLBA_PGN_FN void line_row_ep(const CamT &c, double hth, const double *Gs, const double *Ge, const double *le, double ds,
                             double de, double r, double *J) {
    PLBA_PGN_EXACT
    double Js[6], Je[6];
    pgn::jrow(c, hth, Gs, le[0], le[1], Js);
    pgn::jrow(c, hth, Ge, le[0], le[1], Je);
    const double m = fmax(hth, r);
    for (int k = 0; k < 6; ++k) J[k] = (Js[k] * ds + Je[k] * de) / m;
}

// What the Plücker model keeps of a line between its residual and its row
struct PlLine {
    double RN[3], RD[3];  // R·N, R·D
    double l[3];          // the line in pixels, K_pl·n'
    double e0, e1;        // the signed distances of spl_obs and epl_obs to it
};

// Plücker model: n' = R·N + (t^ R)·D (TransformForPluker), l = K_pl·n', the two distances (:712-720)
template <typename CamT>
PLBA_PGN_FN double line_res_pl(const CamT &c, const double *T, const double *ND, const double *obs, PlLine &L) {
    PLBA_PGN_EXACT
    const double t[3] = {T[3], T[7], T[11]};
    double n[3];
    for (int i = 0; i < 3; ++i) {
        L.RN[i] = (T[4 * i] * ND[0] + T[4 * i + 1] * ND[1]) + T[4 * i + 2] * ND[2];
        L.RD[i] = (T[4 * i] * ND[3] + T[4 * i + 1] * ND[4]) + T[4 * i + 2] * ND[5];
    }
    // row i of (t^ R)·D, its three products summed after the three of R·N
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        double s = L.RN[i];
        for (int j = 0; j < 3; ++j) s += (t[i1] * T[4 * i2 + j] - t[i2] * T[4 * i1 + j]) * ND[3 + j];
        n[i] = s;
    }
    L.l[0] = c.fy * n[0];
    L.l[1] = c.fx * n[1];
    L.l[2] = ((-c.fy * c.cx) * n[0] + (-c.fx * c.cy) * n[1]) + (c.fx * c.fy) * n[2];
    const double d = sqrt(L.l[0] * L.l[0] + L.l[1] * L.l[1]);
    L.e0 = (obs[0] * L.l[0] + obs[1] * L.l[1] + L.l[2]) / d;
    L.e1 = (obs[2] * L.l[0] + obs[3] * L.l[1] + L.l[2]) / d;
    return sqrt(L.e0 * L.e0 + L.e1 * L.e1);
}

// Plücker model: J_aux = (jac0ᵀ·err0 + jac1ᵀ·err1) / max(homog_th, ‖e‖) with
// jac = ∂e/∂l · [K_pl 0] · ∂(n', d')/∂(t, ω) (:722-753); only the first three rows of the last factor
// meet a non-zero column: [−(R·D)^ | −(R·N)^ − t^·(R·D)^].
template <typename CamT>
PLBA_PGN_FN void line_row_pl(const CamT &c, double hth, const double *T, const double *obs, const PlLine &L, double r,
                             double *J) {
    PLBA_PGN_EXACT
    const double lx = L.l[0], ly = L.l[1];
    const double fm = 1.0 / sqrt(lx * lx + ly * ly);
    const double t[3] = {T[3], T[7], T[11]};
    // B = [−(R·D)^ | −(R·N)^ − t^·(R·D)^], 3x6
    double B[18], hd[9], hn[9], ht[9];
    const double *v3[3] = {L.RD, L.RN, t};
    double *h3[3] = {hd, hn, ht};
    for (int m = 0; m < 3; ++m) {
        const double *v = v3[m];
        double *h = h3[m];
        h[0] = 0.0, h[1] = -v[2], h[2] = v[1];
        h[3] = v[2], h[4] = 0.0, h[5] = -v[0];
        h[6] = -v[1], h[7] = v[0], h[8] = 0.0;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += ht[3 * i + k] * hd[3 * k + j];
            B[6 * i + j] = -hd[3 * i + j];
            B[6 * i + 3 + j] = -hn[3 * i + j] - s;
        }
    const double e[2] = {L.e0, L.e1};
    double jac[2][6];
    for (int m = 0; m < 2; ++m) {
        const double a = obs[2 * m], b = obs[2 * m + 1];
        const double f0 = a * fm - lx * e[m] * fm * fm, f1 = b * fm - ly * e[m] * fm * fm, f2 = fm;
        // (∂e/∂l)·K_pl
        const double k0 = f0 * c.fy + f2 * (-c.fy * c.cx), k1 = f1 * c.fx + f2 * (-c.fx * c.cy), k2 = f2 * (c.fx * c.fy);
        for (int j = 0; j < 6; ++j) jac[m][j] = (k0 * B[j] + k1 * B[6 + j]) + k2 * B[12 + j];
    }
    const double mx = fmax(hth, r);
    for (int j = 0; j < 6; ++j) J[j] = (jac[0][j] * e[0] + jac[1][j] * e[1]) / mx;
}

// H += J·Jᵀ·w, g += J·rg·w, e += re·re·w, N += 1 (rg = re but in the Plücker lines, :779-781)
PLBA_PGN_FN void accumulate(double *acc, const double *J, double rg, double re, double w) {
    PLBA_PGN_EXACT
    int q = 0;
    PLBA_PGN_UNROLL
    for (int i = 0; i < 6; ++i)
        PLBA_PGN_UNROLL
        for (int j = i; j < 6; ++j) acc[q++] += J[i] * J[j] * w;
    PLBA_PGN_UNROLL
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * rg * w;
    acc[27] += re * re * w;
    acc[28] += 1.0;
}

// robustWeightCauchy(r / s) (src2/auxiliar.cpp:556-559)
PLBA_PGN_FN double cauchy(double r, double s) {
    PLBA_PGN_EXACT
    const double x = r / s;
    return 1.0 / (1.0 + x * x);
}

// fabsf(r − median): the deviation rounded to float (src2/auxiliar.cpp:401, :453)
PLBA_PGN_FN double mad_dev(double r, double median) {
    PLBA_PGN_EXACT
    return (double)fabsf((float)(r - median));
}

// 1.4826·MAD clamped to [1e-4, sqrt(7.815)] (:1085-1093)
PLBA_PGN_FN double clamp_scale(double mad) {
    PLBA_PGN_EXACT
    double s = 1.4826 * mad;
    if (s < 0.0001) s = 0.0001;
    if (s > sqrt(7.815)) s = sqrt(7.815);
    return s;
}

// isGoodSolution (:292-305) on the ascending eigenvalues of the covariance; a NaN is not good
PLBA_PGN_FN bool is_good(const double *ev, double err, const double *DT) {
    bool fin = true;
    for (int k = 0; k < 16; ++k) fin = fin && __builtin_isfinite(DT[k]);
    return ev[0] >= 0.0 && ev[5] <= 1.0 && err >= 0.0 && err <= 1.0 && fin;
}

}  // namespace tpg
}  // namespace plba
