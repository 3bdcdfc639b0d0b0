// Keyframe-to-keyframe association on the device (plba_kf_associate): MapHandler::matchKF2KFPoints /
// matchKF2KFLines (src/mapHandler.cpp:237-366, :368-590) without the sequential part that builds the
// landmarks. A keyframe pair is two matcher problems, 2 f its points and 2 f + 1 its lines; the previous
// keyframe's rows are the query side, the current keyframe's the train side; rows are indexed over the
// whole batch as the matcher indexes them (csrc/plba_gridmatch.hpp). The arithmetic is in
// csrc/plba_kfassoc_geom.hpp, shared with the host restatement.
//
//   k_kf_cells   grid (problem, block of 256 rows); a thread takes the previous row and the current row
//                of its index. Previous: the projection through DT and the query cell(s). Current: the CSR
//                entry, and for a point its one cell, for a line its direction and its rasterised cells
//                in a fixed stride of max(cols, rows), as k_stereo_cells lays them out and for its reasons.
//   k_grid_cols x 2, k_grid_rows   the matcher, with the window (ws, ws, ws, ws); not launched without
//                fast_matching.
//   k_desc_nn, k_desc_cross        the brute-force matcher over every problem. A workgroup reads its
//                problem's grid count and returns at once unless count < gate_min[p]; the host sets
//                gate_min[p] to the minimum where both sides have more rows than it, else to INT_MIN. So
//                the fallback costs no read-back and the number of launches is fixed.
//   k_kf_geom    grid (problem, block of 256 previous rows), one thread per row, no ordering atomics: the
//                row's match (the fallback's where the problem fell back, else the grid's), its record
//                and its gate bit, written at the row's own index. Thread 0 of a problem's first block
//                writes the problem's grid count, match count and fallback flag.
#pragma once

#include <limits.h>

#include "plba_kfassoc_geom.hpp"  // and with it plba_assoc_args.hpp: KfDev, kKfNT

namespace plba {

// The train side of problem p, row i of its n2: the CSR entry, and for a point (c: pl[2]) its one cell,
// for a line (c: spl[2], epl[2]) its direction and its rasterised cells. Dev is the struct that owns the
// cells, a KfDev or plba_map_associate's MaDev (csrc/plba_mapassoc.hpp), which enters a keyframe's
// unmatched features exactly as the current keyframe's features are entered here.
template <typename Dev>
__device__ inline void kf_train_row(const Dev &D, int p, int i, int n2, const double *c) {
    const bool line = D.kind[p] != 0;
    const int cols = D.prm.cols, rows = D.prm.rows;
    const size_t g = (size_t)(D.off2[p] + i);
    const int per = line ? D.stride : 1;
    const int first = D.cbase[p] + i * per;
    D.cell_off2[g] = first;
    // = cbase[p + 1]: the next problem's first train row writes the same value to the same entry, on purpose
    if (i == n2 - 1) D.cell_off2[g + 1] = first + per;
    int32_t *dst = D.cells2 + 2 * (size_t)first;
    if (line) {
        kf_line_dir(c, c + 2, D.inv_w, D.inv_h, D.dir2 + 2 * g);
        const double x1 = c[0] * D.inv_w, y1 = c[1] * D.inv_h, x2 = c[2] * D.inv_w, y2 = c[3] * D.inv_h;
        const int m = st_line_cells(x1, y1, x2, y2, cols, rows, st_max_steps(cols, rows), dst, per);
        for (int e = m; e < per; ++e) {
            dst[2 * e] = -1;
            dst[2 * e + 1] = -1;
        }
    } else {
        const double gx = c[0] * D.inv_w, gy = c[1] * D.inv_h;
        dst[0] = (int)gx;
        dst[1] = (int)gy;
    }
}

__global__ __launch_bounds__(kKfNT) void k_kf_cells(KfDev D) {
    const int p = blockIdx.x, i = blockIdx.y * kKfNT + threadIdx.x;
    const int o1 = D.off1[p], n1 = D.off1[p + 1] - o1;
    const int n2 = D.off2[p + 1] - D.off2[p];
    const bool line = D.kind[p] != 0;
    const double *DT = D.pose + (size_t)(p >> 1) * kKfPoseDoubles;
    if (i < n1) {
        const size_t g = (size_t)(o1 + i), k = (size_t)(D.kbase1[p] + i);
        if (line) {
            const double *q = D.q_ls + k * kKfQLsDoubles;
            kf_line_cell(D.prm, DT, q, D.inv_w, D.inv_h, D.cell1 + 2 * g);
            kf_line_cell(D.prm, DT, q + 3, D.inv_w, D.inv_h, D.cell1e + 2 * g);
        } else {
            kf_point_cell(D.prm, DT, D.q_pt + 3 * k, D.inv_w, D.inv_h, D.cell1 + 2 * g);
        }
    }
    if (i < n2) {
        const size_t k = (size_t)(D.kbase2[p] + i);
        kf_train_row(D, p, i, n2, line ? D.t_ls + k * kKfTLsDoubles : D.t_pt + k * kKfTPtDoubles);
    }
}

__global__ __launch_bounds__(kKfNT) void k_kf_geom(KfDev D) {
    const int p = blockIdx.x, i1 = blockIdx.y * kKfNT + threadIdx.x;
    const int o1 = D.off1[p], n1 = D.off1[p + 1] - o1, n2 = D.off2[p + 1] - D.off2[p];
    const bool line = D.kind[p] != 0;
    const int gc = D.prm.fast_matching ? D.gcount[p] : 0;
    const bool fb = gc < D.gate_min[p];
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        D.res[3 * p] = gc;
        D.res[3 * p + 1] = fb ? D.fcount[p] : gc;
        D.res[3 * p + 2] = fb ? 1 : 0;
    }
    if (i1 >= n1) return;
    const size_t g = (size_t)(o1 + i1), k1 = (size_t)(D.kbase1[p] + i1);
    int i2 = fb ? D.fm12[g] : (D.prm.fast_matching ? D.gm12[g] : -1);
    if (i2 >= n2) i2 = -1;  // never, from the matchers above
    D.m12[g] = i2;
    double rec[kKfPtDoubles];
    const int nd = line ? kKfLsDoubles : kKfPtDoubles;
    for (int e = 0; e < nd; ++e) rec[e] = 0.0;
    int bit = 0;
    if (i2 >= 0) {
        const double *pose = D.pose + (size_t)(p >> 1) * kKfPoseDoubles;
        const size_t k2 = (size_t)(D.kbase2[p] + i2);
        if (line)
            bit = kf_line(D.prm, pose + 12, pose + 44, pose + 60, D.q_ls + k1 * kKfQLsDoubles, D.ls_new[k1] != 0,
                          D.t_ls + k2 * kKfTLsDoubles, rec);
        else
            kf_point(pose + 12, pose + 28, D.q_pt + 3 * k1, D.t_pt + k2 * kKfTPtDoubles + 2, rec);
    }
    double *o = (line ? D.lsd : D.ptd) + k1 * nd;
    for (int e = 0; e < nd; ++e) o[e] = rec[e];
    if (line) D.rej[k1] = (uint8_t)bit;
}

}  // namespace plba
