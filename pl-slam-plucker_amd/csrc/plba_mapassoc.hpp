// Map-to-keyframe association on the device (plba_map_associate): MapHandler::matchMap2KFPoints /
// matchMap2KFLines (src/mapHandler.cpp:697-797, :799-921) without the sequential part that changes the
// map. A keyframe is two matcher problems, 2 f its points and 2 f + 1 its lines; the candidate landmarks
// are the query side, the keyframe's unmatched features the train side; rows are indexed over the whole
// batch as the matcher indexes them (csrc/plba_gridmatch.hpp). The arithmetic is in
// csrc/plba_mapassoc_geom.hpp, shared with the host restatement. The reference matches the visible
// candidates only, compacted; here nothing is compacted and an invisible row is inert instead.
//
//   k_map_cells  grid (problem, block of 256 rows); a thread takes the candidate row and the feature row
//                of its index. Candidate: the projection through Twf, the visibility flag, the query
//                cell(s), or the empty-window cell of an invisible row, and the skip flag the brute-force
//                matcher reads; a workgroup adds its visible rows to the problem's count with one integer
//                atomic. Feature: the train side, by kf_train_row of csrc/plba_kfassoc.hpp.
//   k_grid_cols x 2, k_grid_rows   the matcher, with the window (ws, ws, ws, ws); not launched without
//                fast_matching.
//   k_map_gate   one thread per problem: gate_min[p] = the minimum where more candidates than it are
//                visible, else INT_MIN. The count is complete only when k_map_cells has ended, so this
//                is a launch of its own; it costs no read-back and the number of launches stays fixed.
//   k_desc_nn<W, MASK>, k_desc_cross   the brute-force matcher over every problem, gated by the grid count
//                against gate_min as in plba_kf_associate, with the skip flags (csrc/plba_match.hpp).
//   k_map_geom   grid (problem, block of 256 candidate rows), one thread per row: the row's match (the
//                fallback's where the problem fell back, else the grid's), the epipolar test, the record
//                and the flags, written at the row's own index; a workgroup adds its accepted rows to the
//                problem's count with one integer atomic. Thread 0 of a problem's first block writes the
//                problem's grid count and fallback flag.
// The two counts are integer sums, so they do not depend on the order of arrival.
#pragma once

#include <limits.h>

#include "plba_kfassoc.hpp"        // kf_train_row
#include "plba_mapassoc_geom.hpp"  // and with it plba_assoc_args.hpp: MaDev, kMaNT

namespace plba {

__global__ __launch_bounds__(kMaNT) void k_map_cells(MaDev D) {
    const int p = blockIdx.x, i = blockIdx.y * kMaNT + threadIdx.x;
    const int o1 = D.off1[p], n1 = D.off1[p + 1] - o1;
    const int n2 = D.off2[p + 1] - D.off2[p];
    const bool line = D.kind[p] != 0;
    const double *Twf = D.pose + (size_t)(p >> 1) * kMaPoseDoubles;
    bool vis = false;
    if (i < n1) {
        const size_t g = (size_t)(o1 + i), k = (size_t)(D.kbase1[p] + i);
        double uv[2];
        if (line) {
            const double *q = D.q_ls + k * kMaQLsDoubles;
            double uve[2];
            const bool vs = ma_project(D.prm, Twf, q, uv), ve = ma_project(D.prm, Twf, q + 3, uve);
            vis = vs && ve;
            ma_cell(vis, uve, D.inv_w, D.inv_h, D.cell1e + 2 * g);
        } else {
            vis = ma_project(D.prm, Twf, D.q_pt + 3 * k, uv);
        }
        ma_cell(vis, uv, D.inv_w, D.inv_h, D.cell1 + 2 * g);
        D.vis[g] = vis ? 1 : 0;
        D.skip[g] = vis ? 0 : 1;
    }
    if (i < n2) {
        const size_t k = (size_t)(D.kbase2[p] + i);
        kf_train_row(D, p, i, n2, line ? D.t_ls + k * kMaTLsDoubles : D.t_pt + k * kMaTPtDoubles);
    }
    const int c = __syncthreads_count(vis);  // every thread of the workgroup is here
    if (threadIdx.x == 0 && c) atomicAdd(&D.cnt[2 * p], c);
}

__global__ __launch_bounds__(kMaNT) void k_map_gate(MaDev D, int np) {
    const int p = blockIdx.x * kMaNT + threadIdx.x;
    if (p >= np) return;
    const int lim = D.min_matches[p];
    D.gate_min[p] = D.cnt[2 * p] > lim ? lim : INT_MIN;  // :759-760, :874-875: both read the visible count
}

__global__ __launch_bounds__(kMaNT) void k_map_geom(MaDev D) {
    const int p = blockIdx.x, i1 = blockIdx.y * kMaNT + threadIdx.x;
    const int o1 = D.off1[p], n1 = D.off1[p + 1] - o1, n2 = D.off2[p + 1] - D.off2[p];
    const bool line = D.kind[p] != 0;
    const int gc = D.prm.fast_matching ? D.gcount[p] : 0;
    const bool fb = gc < D.gate_min[p];
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        D.res[2 * p] = gc;
        D.res[2 * p + 1] = fb ? 1 : 0;
    }
    bool ok = false;
    if (i1 < n1) {
        const size_t g = (size_t)(o1 + i1), k1 = (size_t)(D.kbase1[p] + i1);
        int i2 = fb ? D.fm12[g] : (D.prm.fast_matching ? D.gm12[g] : -1);
        if (i2 >= n2 || D.skip[g]) i2 = -1;  // never, from the matchers above
        D.m12[g] = i2;
        double rec[kMaLsDoubles];
        const int nd = line ? kMaLsDoubles : kMaPtDoubles;
        for (int e = 0; e < nd; ++e) rec[e] = 0.0;
        if (i2 >= 0) {
            const double *pose = D.pose + (size_t)(p >> 1) * kMaPoseDoubles;
            const size_t k2 = (size_t)(D.kbase2[p] + i2);
            if (line) ok = ma_line(D.prm, pose, pose + 12, D.q_ls + k1 * kMaQLsDoubles, D.t_ls + k2 * kMaTLsDoubles, rec);
            else ok = ma_point(D.prm, pose, pose + 12, D.q_pt + 3 * k1, D.t_pt + k2 * kMaTPtDoubles, rec);
        }
        double *o = (line ? D.lsd : D.ptd) + k1 * nd;
        for (int e = 0; e < nd; ++e) o[e] = rec[e];
        D.acc[g] = ok ? 1 : 0;
    }
    const int c = __syncthreads_count(ok);  // every thread of the workgroup is here
    if (threadIdx.x == 0 && c) atomicAdd(&D.cnt[2 * p + 1], c);
}

}  // namespace plba
