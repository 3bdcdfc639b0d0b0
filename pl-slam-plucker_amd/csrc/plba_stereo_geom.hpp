// plba_stereo_geom.hpp — the arithmetic of plba_stereo_associate (include/plba.h), one statement per
// rounded operation: the cells, the rasterised right line, the point gates, the line part of
// StereoFrame::matchStereoLines (src2/stereoFrame.cpp:357-397) and the Plücker line from the two
// viewing planes. Plain C++ with no HIP type, compiled for the device by csrc/plba_stereo.hpp and for
// the host by host/stereo.cpp (plslam_stereo_cpu), so that both evaluate the same expressions; every
// function switches contraction off, and the host object is built with -ffp-contract=off besides.
#pragma once

#include <math.h>

#include "plba_assoc_args.hpp"  // kStPtDoubles, kStLsDoubles

#if defined(__HIPCC__)
#define PLBA_ST_FN __host__ __device__ inline
#else
#define PLBA_ST_FN inline
#endif
#if defined(__clang__)
#define PLBA_ST_EXACT _Pragma("clang fp contract(off)")
#else
#define PLBA_ST_EXACT
#endif

namespace plba {

// gate bits, 0 = the row survives. Points: epipolar, disparity. Lines: the five of :372-375 in order.
enum { kStPtEpip = 1, kStPtDisp = 2 };
enum { kStLsDispS = 1, kStLsDispE = 2, kStLsHorizL = 4, kStLsHorizR = 8, kStLsOverlap = 16 };

// (int)(v * inv): the float promoted, one double product, truncated toward zero (:133, :139, :322-323)
PLBA_ST_FN int st_cell(float v, double inv) {
    PLBA_ST_EXACT
    const double g = (double)v * inv;
    return (int)g;
}

// the steps of the walk of a line whose coordinates are at most one image size outside the image: its
// first and last cell along the stepping axis are truncations toward zero of values in [-size, 2 * size]
// grid units (a rounding beyond either end truncates back onto it), so last - first + 1 <= 3 * size + 1
PLBA_ST_FN int st_max_steps(int cols, int rows) { return 3 * (cols > rows ? cols : rows) + 1; }

// getLineCoords / LineIterator (src2/lineIterator.cpp) over (x1, y1) -> (x2, y2) in grid units: the
// cells inside the grid (GridStructure::at drops the others) in the walk's order, at most cap of them;
// the walk itself takes at most max_steps steps whatever the coordinates are. Returns their number.
PLBA_ST_FN int st_line_cells(double x1, double y1, double x2, double y2, int cols, int rows, int max_steps,
                             int32_t *cells, int cap) {
    PLBA_ST_EXACT
    const bool steep = fabs(y2 - y1) > fabs(x2 - x1);
    double u0 = steep ? y1 : x1, v0 = steep ? x1 : y1, u1 = steep ? y2 : x2, v1 = steep ? x2 : y2;
    if (u0 > u1) {
        double t = u0; u0 = u1; u1 = t;
        t = v0; v0 = v1; v1 = t;
    }
    const double dx = u1 - u0, dy = fabs(v1 - v0);
    double error = dx / 2.0;
    const int ystep = v0 < v1 ? 1 : -1;
    const int first = (int)u0, last = (int)u1;
    int v = (int)v0, n = 0;
    long long steps = (long long)last - first + 1;
    if (steps > max_steps) steps = max_steps;
    for (long long k = 0; k < steps; ++k) {
        const int u = first + (int)k;
        const int cx = steep ? v : u, cy = steep ? u : v;
        if (cx >= 0 && cx < cols && cy >= 0 && cy < rows && n < cap) {
            cells[2 * n] = cx;
            cells[2 * n + 1] = cy;
            ++n;
        }
        error -= dy;
        if (error < 0) {
            v += ystep;
            error += dx;
        }
    }
    return n;
}

// the direction of a right line (:333-334): the differences in float, scaled, normalised
PLBA_ST_FN void st_line_dir(const float *r, double inv_w, double inv_h, double *dir) {
    PLBA_ST_EXACT
    const float fx = r[2] - r[0], fy = r[3] - r[1];
    const double vx = (double)fx * inv_w, vy = (double)fy * inv_h;
    const double xx = vx * vx, yy = vy * vy;
    const double mag = sqrt(xx + yy);
    dir[0] = vx / mag;
    dir[1] = vy / mag;
}

// PinholeStereoCamera::backProjection (src2/pinholeStereoCamera.cpp:225-233)
PLBA_ST_FN void st_back_projection(const plba_stereo_params &p, double u, double v, double disp, double *P) {
    PLBA_ST_EXACT
    const double bd = p.b / disp;
    P[0] = bd * (u - p.cx);
    P[1] = bd * (v - p.cy);
    P[2] = bd * p.fx;
}

// :158-164 for the match l -> r of two keypoints (x, y); o: pl[2], disp, P[3]
PLBA_ST_FN int st_point(const plba_stereo_params &p, const float *l, const float *r, double *o) {
    PLBA_ST_EXACT
    const float dy = fabsf(l[1] - r[1]), dx = l[0] - r[0];
    const double disp = (double)dx;
    int bits = 0;
    if (!((double)dy <= p.max_dist_epip)) bits |= kStPtEpip;
    if (!(disp >= p.min_disp)) bits |= kStPtDisp;
    o[0] = (double)l[0];
    o[1] = (double)l[1];
    o[2] = disp;
    st_back_projection(p, o[0], o[1], disp, o + 3);
    return bits;
}

PLBA_ST_FN void st_cross(const double *a, const double *b, double *c) {
    PLBA_ST_EXACT
    const double p0 = a[1] * b[2], q0 = a[2] * b[1], p1 = a[2] * b[0], q1 = a[0] * b[2];
    const double p2 = a[0] * b[1], q2 = a[1] * b[0];
    c[0] = p0 - q0;
    c[1] = p1 - q1;
    c[2] = p2 - q2;
}

// StereoFrame::pi_from_ppp (:870-875): the plane through x1, x2, x3
PLBA_ST_FN void st_pi_from_ppp(const double *x1, const double *x2, const double *x3, double *pi) {
    PLBA_ST_EXACT
    const double a[3] = {x1[0] - x3[0], x1[1] - x3[1], x1[2] - x3[2]};
    const double b[3] = {x2[0] - x3[0], x2[1] - x3[1], x2[2] - x3[2]};
    st_cross(a, b, pi);
    double c[3];
    st_cross(x1, x2, c);
    const double t0 = x3[0] * c[0], t1 = x3[1] * c[1], t2 = x3[2] * c[2];
    const double t12 = t1 + t2;
    pi[3] = -(t0 + t12);
}

// lineSegmentOverlapStereo (:510-545)
PLBA_ST_FN double st_overlap(double spl_obs, double epl_obs, double spl_proj, double epl_proj, double line_horiz_th) {
    PLBA_ST_EXACT
    double overlap = 1.0;
    if (fabs(epl_obs - spl_obs) > line_horiz_th) {
        const double sln = epl_obs < spl_obs ? epl_obs : spl_obs, eln = spl_obs < epl_obs ? epl_obs : spl_obs;
        const double spn = epl_proj < spl_proj ? epl_proj : spl_proj, epn = spl_proj < epl_proj ? epl_proj : spl_proj;
        const double length = eln - spn;
        if (epn < sln || spn > eln) overlap = 0.0;
        else if (epn > eln && spn < sln) overlap = eln - sln;
        else overlap = (epn < eln ? epn : eln) - (sln < spn ? spn : sln);
        if (length > (double)0.01f) overlap = overlap / length;
        else overlap = 0.0;
        if (overlap > 1.0) overlap = 1.0;
    }
    return overlap;
}

// lineSegmentOverlap (:547-653), the 2-D one of the frame-to-frame pose: the share of the observed
// segment (so, eo) that the projected one (sp, ep) covers. A vertical segment (|Δx| < 1) compares the
// y coordinates, a horizontal one (|Δy| < 1) the x coordinates, any other the x coordinates of the
// feet of the perpendiculars on the observed line.
PLBA_ST_FN double st_overlap2d(const double *so, const double *eo, const double *sp, const double *ep) {
    PLBA_ST_EXACT
    double ls, le;
    if (fabs(so[0] - eo[0]) < 1.0) {
        const double l1 = eo[1] - so[1];
        ls = (sp[1] - so[1]) / l1;
        le = (ep[1] - so[1]) / l1;
    } else if (fabs(so[1] - eo[1]) < 1.0) {
        const double l0 = eo[0] - so[0];
        ls = (sp[0] - so[0]) / l0;
        le = (ep[0] - so[0]) / l0;
    } else {
        const double l0 = eo[0] - so[0];
        const double a = so[1] - eo[1], b = eo[0] - so[0], c = so[0] * eo[1] - eo[0] * so[1];
        const double lxy = 1.0 / (a * a + b * b);
        const double xs = (b * (b * sp[0] - a * sp[1]) - a * c) * lxy;
        const double xe = (b * (b * ep[0] - a * ep[1]) - a * c) * lxy;
        ls = (xs - so[0]) / l0;
        le = (xe - so[0]) / l0;
    }
    const double lmin = le < ls ? le : ls, lmax = ls < le ? le : ls;  // std::min / std::max
    if (lmin < 0.0 && lmax > 1.0) return 1.0;
    if (lmax < 0.0 || lmin > 1.0) return 0.0;
    if (lmin < 0.0) return lmax;
    if (lmax > 1.0) return 1.0 - lmin;
    return lmax - lmin;
}

// :357-397 for the match l -> r of two segments (sx, sy, ex, ey); o: the kStLsDoubles of a line record
// (NDc only with p.pluker)
PLBA_ST_FN int st_line(const plba_stereo_params &p, const float *l, const float *r, double *o) {
    PLBA_ST_EXACT
    const double slx = (double)l[0], sly = (double)l[1], elx = (double)l[2], ely = (double)l[3];
    const double srx = (double)r[0], sry = (double)r[1], erx = (double)r[2], ery = (double)r[3];
    const double sp_l[3] = {slx, sly, 1.0}, ep_l[3] = {elx, ely, 1.0};
    double le[3];
    st_cross(sp_l, ep_l, le);
    const double l00 = le[0] * le[0], l11 = le[1] * le[1];
    const double ln = sqrt(l00 + l11);
    const double overlap = st_overlap(sly, ely, sry, ery, p.line_horiz_th);
    // :367 writes sp_r = (X, sy_l); :368 reads it
    const double a0 = sly - ery, a1 = sry - sly, a2 = sry - ery;
    const double n0 = srx * a0, n1 = erx * a1;
    const double X = (n0 + n1) / a2;
    const double b0 = ely - ery, b1 = sly - ely, b2 = sly - ery;
    const double m0 = X * b0, m1 = erx * b1;
    const double Xe = (m0 + m1) / b2;
    double ds = slx - X, de = elx - Xe;  // filterLineSegmentDisparity (:442-452)
    const double dmin = de < ds ? de : ds, dmax = ds < de ? de : ds;
    if (dmin / dmax < p.ls_min_disp_ratio) {
        ds = -1.0;
        de = -1.0;
    }
    int bits = 0;
    if (!(ds >= p.min_disp)) bits |= kStLsDispS;
    if (!(de >= p.min_disp)) bits |= kStLsDispE;
    if (!(fabs(sly - ely) > p.line_horiz_th)) bits |= kStLsHorizL;
    if (!(fabs(sly - ely) > p.line_horiz_th)) bits |= kStLsHorizR;  // sp_r(1) - ep_r(1) after the overwrite
    if (!(overlap > p.stereo_overlap_th)) bits |= kStLsOverlap;
    o[0] = slx; o[1] = sly; o[2] = elx; o[3] = ely;
    o[4] = ds; o[5] = de;
    st_back_projection(p, slx, sly, ds, o + 6);
    st_back_projection(p, elx, ely, de, o + 9);
    o[12] = le[0] / ln; o[13] = le[1] / ln; o[14] = le[2] / ln;
    if (p.pluker) {
        const double a[3] = {(slx - p.cx) / p.fx, (sly - p.cy) / p.fy, 1.0};
        const double c[3] = {(elx - p.cx) / p.fx, (ely - p.cy) / p.fy, 1.0};
        const double ux = (X - p.cx) / p.fx, wx = (Xe - p.cx) / p.fx;
        const double a2v[3] = {ux + p.b, (sly - p.cy) / p.fy, 1.0}, c2v[3] = {wx + p.b, (ely - p.cy) / p.fy, 1.0};
        const double o1[3] = {0.0, 0.0, 0.0}, o2[3] = {p.b, 0.0, 0.0};
        double pi1[4], pi2[4];
        st_pi_from_ppp(a, c, o1, pi1);
        st_pi_from_ppp(a2v, c2v, o2, pi2);
        // pipi_plk (:877-883)
        const int I[6] = {0, 1, 2, 1, 0, 0}, J[6] = {3, 3, 3, 2, 2, 1};
        for (int k = 0; k < 6; ++k) {
            const double s = pi1[I[k]] * pi2[J[k]], t = pi2[I[k]] * pi1[J[k]];
            const double d = s - t;
            o[15 + k] = (k == 3 || k == 5) ? -d : d;
        }
    }
    return bits;
}

}  // namespace plba
