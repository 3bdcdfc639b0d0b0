// plba_kfassoc_geom.hpp — the arithmetic of plba_kf_associate (include/plba.h), one statement per
// rounded operation: the projected query cells of the previous keyframe's features, the train side's
// direction, and the landmark geometry of MapHandler::matchKF2KFPoints / Lines (src/mapHandler.cpp:
// 299-318, :450-494, :546-562). Plain C++ with no HIP type, compiled for the device by
// csrc/plba_kfassoc.hpp and for the host by host/kf_match.cpp (plslam_kf_assoc_cpu), so that both
// evaluate the same expressions; every function switches contraction off, and the host object is built
// with -ffp-contract=off besides. The rasterised line and the macros are those of plba_stereo_geom.hpp.
#pragma once

#include "plba_stereo_geom.hpp"

namespace plba {

// kKf*Doubles, the widths of its rows and records, are in csrc/plba_assoc_args.hpp
constexpr int kKfNoCell = -(1 << 30);  // both coordinates of a cell that has no int value

// t0 + (t1 + t2)
PLBA_ST_FN double kf_sum3(double t0, double t1, double t2) {
    PLBA_ST_EXACT
    const double t12 = t1 + t2;
    return t0 + t12;
}

PLBA_ST_FN double kf_dot3(const double *a, const double *b) {
    PLBA_ST_EXACT
    const double t0 = a[0] * b[0], t1 = a[1] * b[1], t2 = a[2] * b[2];
    return kf_sum3(t0, t1, t2);
}

PLBA_ST_FN double kf_norm3(const double *a) { return sqrt(kf_dot3(a, a)); }

// R x of the pose T (row-major, four doubles per row: the 3 x 4 DT and a 4 x 4 alike)
PLBA_ST_FN void kf_rot(const double *T, const double *x, double *y) {
    for (int i = 0; i < 3; ++i) y[i] = kf_dot3(T + 4 * i, x);
}

// R x + t
PLBA_ST_FN void kf_transform(const double *T, const double *x, double *y) {
    PLBA_ST_EXACT
    kf_rot(T, x, y);
    for (int i = 0; i < 3; ++i) y[i] = y[i] + T[4 * i + 3];
}

// cam->projection(DT.R P + DT.t) (src2/pinholeStereoCamera.cpp:235-241)
PLBA_ST_FN void kf_project(const plba_kfassoc_params &p, const double *DT, const double *P, double *uv) {
    PLBA_ST_EXACT
    double Q[3];
    kf_transform(DT, P, Q);
    const double a = p.fx * Q[0], b = p.fy * Q[1];
    const double qa = a / Q[2], qb = b / Q[2];
    uv[0] = p.cx + qa;
    uv[1] = p.cy + qb;
}

// the cell of (gx, gy), or (kKfNoCell, kKfNoCell) where either has no int value
PLBA_ST_FN void kf_cell(double gx, double gy, int32_t *cell) {
    const double lim = 1073741824.0;
    const bool ok = fabs(gx) < lim && fabs(gy) < lim;  // false for NaN
    cell[0] = ok ? (int)gx : kKfNoCell;
    cell[1] = ok ? (int)gy : kKfNoCell;
}

// :258-259: a previous point's query cell
PLBA_ST_FN void kf_point_cell(const plba_kfassoc_params &p, const double *DT, const double *P, double inv_w, double inv_h,
                              int32_t *cell) {
    PLBA_ST_EXACT
    double uv[2];
    kf_project(p, DT, P, uv);
    const double gx = uv[0] * inv_w, gy = uv[1] * inv_h;
    kf_cell(gx, gy, cell);
}

// :389-396: one of a previous line's two query cells, in pixels unless line_query_in_grid_units
PLBA_ST_FN void kf_line_cell(const plba_kfassoc_params &p, const double *DT, const double *P, double inv_w, double inv_h,
                             int32_t *cell) {
    PLBA_ST_EXACT
    double uv[2];
    kf_project(p, DT, P, uv);
    if (p.line_query_in_grid_units) {
        const double gx = uv[0] * inv_w, gy = uv[1] * inv_h;
        kf_cell(gx, gy, cell);
    } else {
        kf_cell(uv[0], uv[1], cell);
    }
}

// :407-408: the direction of a current line
PLBA_ST_FN void kf_line_dir(const double *spl, const double *epl, double inv_w, double inv_h, double *dir) {
    PLBA_ST_EXACT
    const double dx = epl[0] - spl[0], dy = epl[1] - spl[1];
    const double vx = dx * inv_w, vy = dy * inv_h;
    const double xx = vx * vx, yy = vy * vy;
    const double mag = sqrt(xx + yy);
    dir[0] = vx / mag;
    dir[1] = vy / mag;
}

// :299-318, :339-341. T_prev, T_curr: 4 x 4; o: the kKfPtDoubles of a point record
PLBA_ST_FN void kf_point(const double *T_prev, const double *T_curr, const double *P1, const double *P2, double *o) {
    PLBA_ST_EXACT
    double Pc[3];
    kf_transform(T_prev, P1, o);
    const double n1 = kf_norm3(o);
    for (int i = 0; i < 3; ++i) o[3 + i] = o[i] / n1;
    kf_transform(T_curr, P2, Pc);
    const double n2 = kf_norm3(Pc);
    for (int i = 0; i < 3; ++i) o[6 + i] = Pc[i] / n2;
}

// TransformForPluker (include/mapHandler.h:232-240): head = R N + (t^ R) D, tail = R D (tail may be null)
PLBA_ST_FN void kf_pluker(const double *T, const double *ND, double *head, double *tail) {
    PLBA_ST_EXACT
    const double t[3] = {T[3], T[7], T[11]};
    double M[9];  // t^ R, column by column
    for (int j = 0; j < 3; ++j) {
        const double c[3] = {T[j], T[4 + j], T[8 + j]};
        double m[3];
        st_cross(t, c, m);
        M[j] = m[0];
        M[3 + j] = m[1];
        M[6 + j] = m[2];
    }
    for (int i = 0; i < 3; ++i) {
        const double a = kf_dot3(T + 4 * i, ND), b = kf_dot3(M + 3 * i, ND + 3);
        head[i] = a + b;
    }
    if (tail) kf_rot(T, ND + 3, tail);
}

// the norm of the two-row point-to-line error of the world line W seen from Tcw against (s, e) (:463-471)
PLBA_ST_FN double kf_line_err(const plba_kfassoc_params &p, const double *Tcw, const double *W, const double *s,
                              const double *e) {
    PLBA_ST_EXACT
    double h[3];
    kf_pluker(Tcw, W, h, nullptr);
    const double k20 = (-p.fy) * p.cx, k21 = (-p.fx) * p.cy, k22 = p.fx * p.fy;
    const double lx = p.fy * h[0], ly = p.fx * h[1];
    const double z0 = k20 * h[0], z1 = k21 * h[1], z2 = k22 * h[2];
    const double lz = kf_sum3(z0, z1, z2);
    const double xx = lx * lx, yy = ly * ly;
    const double f = sqrt(xx + yy);
    const double a0 = s[0] * lx, a1 = s[1] * ly, b0 = e[0] * lx, b1 = e[1] * ly;
    const double a01 = a0 + a1, b01 = b0 + b1;
    const double e0 = (a01 + lz) / f, e1 = (b01 + lz) / f;
    const double q0 = e0 * e0, q1 = e1 * e1;
    return sqrt(q0 + q1);
}

// :450-494 (is_new) / :546-562. q: the kKfQLsDoubles of the previous row; c: the current row's spl, epl;
// o: the kKfLsDoubles of a line record. Returns the gate bit.
PLBA_ST_FN int kf_line(const plba_kfassoc_params &p, const double *T_prev, const double *Tcw_prev, const double *Tcw_curr,
                       const double *q, bool is_new, const double *c, double *o) {
    PLBA_ST_EXACT
    const double th = sqrt(5.991);
    if (is_new) {
        double head[3], tail[3];
        kf_pluker(T_prev, q + 6, head, tail);
        const double nh = kf_norm3(head), nt = kf_norm3(tail);
        const double d = nh / nt;
        for (int i = 0; i < 3; ++i) {
            const double u = head[i] / nh;
            o[i] = u * d;
            o[3 + i] = tail[i] / nt;
        }
        o[6] = kf_line_err(p, Tcw_prev, o, q + 12, q + 14);
        o[7] = kf_line_err(p, Tcw_curr, o, c, c + 2);
    } else {
        for (int i = 0; i < 7; ++i) o[i] = 0.0;
        o[7] = kf_line_err(p, Tcw_curr, q + 16, c, c + 2);
    }
    return o[7] > th ? 1 : 0;
}

}  // namespace plba
