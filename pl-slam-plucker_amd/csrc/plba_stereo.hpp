// Stereo association of a frame's features on the device (plba_stereo_associate):
// StereoFrame::matchStereoPoints / matchStereoLines (src2/stereoFrame.cpp:121-174, :310-435). A frame
// is two matcher problems, 2 f its points and 2 f + 1 its lines; rows are indexed over the whole
// batch as the matcher indexes them (csrc/plba_gridmatch.hpp). The arithmetic is in
// csrc/plba_stereo_geom.hpp, shared with the host restatement.
//
//   k_stereo_cells  grid (problem, block of 256 rows); a thread takes the left row and the right row of
//                   its index. Left: the query cell(s). Right: the CSR entry, and for a point its one
//                   cell, for a line its direction and its rasterised cells. A right line owns a fixed
//                   stride of max(cols, rows) cells: the walk is sequential in a double error term, so a
//                   line is one thread's work whatever the layout is, and a count / scan / fill would
//                   walk every line twice and add a scan over the batch for the sake of a list that is
//                   at most 64 cells long. The cells of a walk have distinct coordinates along its
//                   stepping axis, so at most max(cols, rows) lie inside the grid; only those are
//                   stored, and the rest of the stride is (-1, -1), which the matcher ignores as
//                   GridStructure::at does. The walk is bounded by st_max_steps whatever the input is.
//   k_grid_cols x 2, k_grid_rows   the matcher, with the window (matching_s_ws, 0, 0, 0).
//   k_stereo_gate   one workgroup per problem, its left rows in blocks of 256 in index order: the gates
//                   and the geometry of a matched row in its thread, then an inclusive scan of the
//                   survivor flags (shuffles within a wave, the four wave totals added in wave order, a
//                   running base across blocks), so a survivor's output row is its rank in index order
//                   with no atomic in the ordering. The thread writes its record, its left index and
//                   its descriptor row.
#pragma once

#include "plba_stereo_geom.hpp"  // and with it plba_assoc_args.hpp: StDev, kStNT

namespace plba {

__global__ __launch_bounds__(kStNT) void k_stereo_cells(StDev D) {
    const int p = blockIdx.x, i = blockIdx.y * kStNT + threadIdx.x;
    const int o1 = D.off1[p], n1 = D.off1[p + 1] - o1;
    const int o2 = D.off2[p], n2 = D.off2[p + 1] - o2;
    const bool line = D.kind[p] != 0;
    const int cols = D.prm.cols, rows = D.prm.rows;
    if (i < n1) {
        const size_t g = (size_t)(o1 + i);
        const float *c = D.co1 + 4 * g;
        D.cell1[2 * g] = st_cell(c[0], D.inv_w);
        D.cell1[2 * g + 1] = st_cell(c[1], D.inv_h);
        if (line) {
            D.cell1e[2 * g] = st_cell(c[2], D.inv_w);
            D.cell1e[2 * g + 1] = st_cell(c[3], D.inv_h);
        }
    }
    if (i < n2) {
        const size_t g = (size_t)(o2 + i);
        const float *c = D.co2 + 4 * g;
        const int per = line ? D.stride : 1;
        const int first = D.cbase[p] + i * per;
        D.cell_off2[g] = first;
        if (i == n2 - 1) D.cell_off2[g + 1] = first + per;  // = cbase[p + 1]
        int32_t *dst = D.cells2 + 2 * (size_t)first;
        if (line) {
            st_line_dir(c, D.inv_w, D.inv_h, D.dir2 + 2 * g);
            const double x1 = (double)c[0] * D.inv_w, y1 = (double)c[1] * D.inv_h, x2 = (double)c[2] * D.inv_w,
                         y2 = (double)c[3] * D.inv_h;
            const int k = st_line_cells(x1, y1, x2, y2, cols, rows, st_max_steps(cols, rows), dst, per);
            for (int e = k; e < per; ++e) {
                dst[2 * e] = -1;
                dst[2 * e + 1] = -1;
            }
        } else {
            dst[0] = st_cell(c[0], D.inv_w);
            dst[1] = st_cell(c[1], D.inv_h);
        }
    }
}

__global__ __launch_bounds__(kStNT) void k_stereo_gate(StDev D) {
    __shared__ int wtot[kStNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o1 = D.off1[p], n1 = D.off1[p + 1] - o1, o2 = D.off2[p];
    const bool line = D.kind[p] != 0;
    const int nd = line ? kStLsDoubles : kStPtDoubles;
    const int nw = line ? (D.prm.pluker ? kStLsDoubles : kStLsDoubles - 6) : kStPtDoubles;  // NDc only with pluker
    double *const recs = (line ? D.lsd : D.ptd) + (size_t)D.kbase[p] * nd;
    int base = 0;
    // the loop's bounds depend on the problem alone: every thread reaches every barrier
    for (int b0 = 0; b0 < n1; b0 += kStNT) {
        const int i1 = b0 + tid;
        double rec[kStLsDoubles];
        bool keep = false;
        if (i1 < n1) {
            const int i2 = D.m12[o1 + i1];
            if (i2 >= 0) {
                const float *l = D.co1 + 4 * (size_t)(o1 + i1), *r = D.co2 + 4 * (size_t)(o2 + i2);
                keep = (line ? st_line(D.prm, l, r, rec) : st_point(D.prm, l, r, rec)) == 0;
            }
        }
        int incl = keep ? 1 : 0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int v = __shfl_up(incl, m, 64);
            if (lane >= m) incl += v;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < kStNT / 64; ++w) {
            if (w < wave) before += wtot[w];
            total += wtot[w];
        }
        if (keep) {
            const int rank = before + incl - 1;  // < n1
            double *o = recs + (size_t)rank * nd;
            for (int k = 0; k < nw; ++k) o[k] = rec[k];
            D.src[o1 + rank] = i1;
            const uint32_t *ds = D.desc1 + (size_t)(o1 + i1) * D.dwords;
            uint32_t *dd = D.odesc + (size_t)(o1 + rank) * D.dwords;
            for (int c = 0; c < D.dwords; ++c) dd[c] = ds[c];
        }
        base += total;
        __syncthreads();  // wtot is written again
    }
    if (tid == 0) D.count[p] = base;
}

}  // namespace plba
