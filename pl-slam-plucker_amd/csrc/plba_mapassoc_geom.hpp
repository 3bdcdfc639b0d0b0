// plba_mapassoc_geom.hpp — the arithmetic of plba_map_associate (include/plba.h), one statement per
// rounded operation: the projection of a candidate landmark with its visibility test and query cell, and
// the epipolar tests and records of MapHandler::matchMap2KFPoints / Lines (src/mapHandler.cpp:714-719,
// :770-784, :815-824, :885-901). Plain C++ with no HIP type, compiled for the device by
// csrc/plba_mapassoc.hpp and for the host by host/map_assoc.cpp (plslam_map_assoc_cpu), so that both
// evaluate the same expressions; every function switches contraction off, and the host object is built
// with -ffp-contract=off besides. The sums, the pose products and the macros are those of
// plba_kfassoc_geom.hpp.
#pragma once

#include "plba_kfassoc_geom.hpp"

namespace plba {

// kMa*Doubles, the widths of its rows and records, are in csrc/plba_assoc_args.hpp

// :714-716: cam->projection(Twf.R X + Twf.t) into uv, and the strict in-image and depth test (false for NaN)
PLBA_ST_FN bool ma_project(const plba_mapassoc_params &p, const double *Twf, const double *X, double *uv) {
    PLBA_ST_EXACT
    double Q[3];
    kf_transform(Twf, X, Q);
    const double a = p.fx * Q[0], b = p.fy * Q[1];
    const double qa = a / Q[2], qb = b / Q[2];
    uv[0] = p.cx + qa;
    uv[1] = p.cy + qb;
    return uv[0] > 0 && uv[0] < p.width && uv[1] > 0 && uv[1] < p.height && Q[2] > 0.0;
}

// :719, :823-824: the query cell of a projection that passed the test (so both products have an int
// value); an invisible row takes (kKfNoCell, kKfNoCell), whose window is empty
PLBA_ST_FN void ma_cell(bool visible, const double *uv, double inv_w, double inv_h, int32_t *cell) {
    PLBA_ST_EXACT
    const double gx = uv[0] * inv_w, gy = uv[1] * inv_h;
    cell[0] = visible ? (int)gx : kKfNoCell;
    cell[1] = visible ? (int)gy : kKfNoCell;
}

// :770-784. X: the landmark; t: the kMaTPtDoubles of the feature row (pl[2], P[3]); o: the kMaPtDoubles
// of a point record. Returns the epipolar test.
PLBA_ST_FN bool ma_point(const plba_mapassoc_params &p, const double *Twf, const double *T_kf_w, const double *X,
                         const double *t, double *o) {
    PLBA_ST_EXACT
    ma_project(p, Twf, X, o);
    const double du = o[0] - t[0], dv = o[1] - t[1];
    const double uu = du * du, vv = dv * dv;
    o[2] = sqrt(uu + vv);
    const double n = kf_norm3(t + 2);
    const double d[3] = {t[2] / n, t[3] / n, t[4] / n};
    kf_transform(T_kf_w, d, o + 3);  // :783: the translation too
    return o[2] < p.max_kf_epip_p;
}

// :885-901. X: line3D; t: the kMaTLsDoubles of the feature row (spl[2], epl[2], le[3], sP[3], eP[3]); o: the
// kMaLsDoubles of a line record. Returns the epipolar test, signed as the reference has it.
PLBA_ST_FN bool ma_line(const plba_mapassoc_params &p, const double *Twf, const double *T_kf_w, const double *X,
                        const double *t, double *o) {
    PLBA_ST_EXACT
    ma_project(p, Twf, X, o);
    ma_project(p, Twf, X + 3, o + 2);
    const double *le = t + 4, *sP = t + 7, *eP = t + 10;
    const double a0 = le[0] * o[0], a1 = le[1] * o[1], b0 = le[0] * o[2], b1 = le[1] * o[3];
    const double a01 = a0 + a1, b01 = b0 + b1;
    o[4] = a01 + le[2];
    o[5] = b01 + le[2];
    double m[3], y[3];
    for (int i = 0; i < 3; ++i) {
        const double s = sP[i] + eP[i];
        m[i] = 0.5 * s;
    }
    kf_transform(T_kf_w, m, y);
    const double n = kf_norm3(y);
    for (int i = 0; i < 3; ++i) o[6 + i] = y[i] / n;
    return o[4] < p.max_kf_epip_l && o[5] < p.max_kf_epip_l;
}

}  // namespace plba
