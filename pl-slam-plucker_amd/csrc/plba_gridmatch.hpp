// Grid-guided descriptor matching on the device (plba_grid_match): both StVO::matchGrid overloads
// (src2/matching.cpp:111-258), the window-restricted Hamming matcher that matchKF2KFPoints / Lines
// and matchMap2KFPoints / Lines (src/mapHandler.cpp:253-273, :384-421, :743-757, :848-872) try first.
// A call handles a batch of independent problems, points and lines mixed, in a fixed number of launches.
//
// The reference walks the query rows in order and keeps, per train row (a column), the running
// minimum distance: with the left/right check a pair (i1, i2) is seen by row i1 only if its distance
// is strictly below that of every earlier candidate of column i2, a strict prefix-minimum record.
// Distances lie in [0, 8 * desc_bytes], so a column has at most 8 * desc_bytes + 1 records. The
// columns are independent of each other, and what a row keeps of its seen pairs (the smallest and
// the second-smallest distance, ties to the lowest i2) is the two smallest of the packed keys
// (d << 16) | i2, which are distinct within a row. So:
//
//   k_grid_cols<W, 0>  grid (problem, block of 64 train rows), 64 threads. A thread owns one train
//                 row: its descriptor (W dwords), its direction and the bounding box of its in-grid
//                 cells in registers, its cell list (one cell for a point) in LDS when the lists of
//                 the block's rows fit in 4096 cells, else in global memory. The
//                 query rows go through LDS in tiles of 256: descriptor, the clipped window of each
//                 query cell ([lo, hi) in x and y, inside the grid, so a cell outside the grid is in
//                 no window) and, for a line, the normalised direction. Every thread reads the same
//                 LDS address at the same time (a broadcast). The thread walks the tile in index
//                 order, tests the window first (bounding box, then the cells), then the direction,
//                 and takes the Hamming distance only for candidates; it keeps the column minimum
//                 and matches_21 and, for every seen pair, takes an integer atomicMin of the key
//                 into the tile's LDS row-best. After a tile, one global atomicMin per row that was
//                 touched. Pass 0 ends with the plain store of matches_21.
//   k_grid_cols<W, 1>  the same walk; the tile also stages the final best key of each row, and every
//                 seen key other than it goes into the row's second-best.
//   k_grid_rows   one workgroup per problem: the ratio test in double, the final cross-check and the
//                 count, summed per thread, then over the wave and the four waves in a fixed order.
//
// Integer minima over distinct keys do not depend on the order of arrival, so the result does not
// depend on the launch geometry. The tile loop's bounds depend on the problem alone and threads
// past the last train row only skip the walk, so every thread reaches every barrier.
#pragma once

#include <limits.h>

#include "plba_assoc_args.hpp"  // GmDev, kGmNT, kGmMaxTrain

namespace plba {

constexpr int kGmTile = 256;    // query rows staged through LDS at a time
constexpr int kGmCells = 4096;   // in-grid cells of a block's train rows kept in LDS (64 rasterised lines fit)
constexpr int kGmRowsNT = 256;  // threads of k_grid_rows
constexpr uint32_t kGmNone = 0xFFFFFFFFu;  // no key: above every (d << 16) | i2

// GridStructure::get's bounds (src2/gridStructure.cpp:67-71) for one axis with the two half-widths of
// a GridWindow pair (w.width or w.height: below, above), [lo, hi) kept inside [0, size] so that an
// empty range stays empty whatever the query cell is
__device__ inline int2 gm_window(int x, int ws_lo, int ws_hi, int size) {
    const long long lo = max(0LL, (long long)x - ws_lo), hi = min((long long)size, (long long)x + ws_hi + 1);
    return make_int2((int)min(lo, (long long)size), (int)max(hi, 0LL));
}

__device__ inline bool gm_in(const int4 w, int cx, int cy) { return cx >= w.x && cx < w.y && cy >= w.z && cy < w.w; }

// include2/matching.h:39-48, dot and normalize, as a host compiler without fused multiply-add
// evaluates them: two rounded products and a rounded sum
__device__ inline double gm_dot(const double2 a, const double2 b) {
#pragma clang fp contract(off)
    const double x = a.x * b.x, y = a.y * b.y;
    return x + y;
}

__device__ inline double2 gm_normalize(double x, double y) {
    const double mag = sqrt(gm_dot(make_double2(x, y), make_double2(x, y)));
    return make_double2(x / mag, y / mag);
}

// W: dwords of a row in registers and in LDS (8 or 16), dwords <= W. PASS 0: best key, matches_21.
// PASS 1: second-best key.
template <int W, int PASS>
__global__ __launch_bounds__(kGmNT) void k_grid_cols(GmDev D) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[kGmTile * W];
    __shared__ int4 win0[kGmTile], win1[kGmTile];
    __shared__ double2 qdir[kGmTile];
    __shared__ uint32_t lkey[kGmTile];    // PASS 0: the tile's row-best; PASS 1: the row-second
    __shared__ uint32_t lbest[kGmTile];   // PASS 1: the final best key of each row
    __shared__ int2 lcell[kGmCells];      // the in-grid cells of the block's train rows, row after row
    const int p = blockIdx.x, tid = threadIdx.x;
    const int o1 = D.off1[p], n1 = D.off1[p + 1] - o1;
    const int o2 = D.off2[p], n2 = D.off2[p + 1] - o2;
    if ((int)blockIdx.y * kGmNT >= n2) return;  // the whole workgroup, before any barrier
    const int i2 = blockIdx.y * kGmNT + tid;
    const bool owner = i2 < n2;
    const int dw = D.dwords, cols = D.cols, rows = D.rows;
    const int wl = D.ws[4 * p], wr = D.ws[4 * p + 1], wu = D.ws[4 * p + 2], wd = D.ws[4 * p + 3];
    const bool line = D.kind[p] != 0;
    const double th = D.sim_th[p];

    uint32_t t[W];
#pragma unroll
    for (int c = 0; c < W; ++c) t[c] = 0u;
    int c0 = 0, c1 = 0, bx0 = INT_MAX, bx1 = INT_MIN, by0 = INT_MAX, by1 = INT_MIN, ncell = 0, onex = 0, oney = 0;
    double2 d2 = make_double2(0.0, 0.0);
    if (owner) {
        const uint32_t *src = D.desc2 + (size_t)(o2 + i2) * dw;
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c < dw) t[c] = src[c];
        c0 = D.cell_off2[o2 + i2];
        c1 = D.cell_off2[o2 + i2 + 1];
        for (int c = c0; c < c1; ++c) {
            const int cx = D.cells2[2 * c], cy = D.cells2[2 * c + 1];
            if (cx >= 0 && cx < cols && cy >= 0 && cy < rows) {  // GridStructure::at: the others are dropped
                bx0 = min(bx0, cx); bx1 = max(bx1, cx);
                by0 = min(by0, cy); by1 = max(by1, cy);
                onex = cx; oney = cy;
                ++ncell;
            }
        }
        if (line) d2 = make_double2(D.dir2[2 * (size_t)(o2 + i2)], D.dir2[2 * (size_t)(o2 + i2) + 1]);
    }
    if (dw != W)  // the padding columns, never written again
        for (int e = tid; e < kGmTile * W; e += kGmNT) tile[e] = 0u;
    // Rows of several cells (lines) keep their in-grid cells in LDS when those of the whole block
    // fit; otherwise every row of the block reads its list from global memory. One wave: a shuffle scan.
    int coff = ncell;
#pragma unroll
    for (int m = 1; m < kGmNT; m <<= 1) {
        const int v = __shfl_up(coff, m, kGmNT);
        if (tid >= m) coff += v;
    }
    const bool in_lds = __shfl(coff, kGmNT - 1, kGmNT) <= kGmCells;
    coff -= ncell;
    if (in_lds && ncell > 1) {
        int w = coff;
        for (int c = c0; c < c1; ++c) {
            const int cx = D.cells2[2 * c], cy = D.cells2[2 * c + 1];
            if (cx >= 0 && cx < cols && cy >= 0 && cy < rows) lcell[w++] = make_int2(cx, cy);
        }
    }

    int colmin = INT_MAX, m21 = -1;
    for (int base = 0; base < n1; base += kGmTile) {
        const int nrow = min(kGmTile, n1 - base);
        __syncthreads();  // the previous tile has been read and flushed (and the padding is in place)
        const uint32_t *src = D.desc1 + (size_t)(o1 + base) * dw;
        if (dw == W) {    // one contiguous, 16-byte aligned run
            const uint4 *s4 = (const uint4 *)src;
            uint4 *t4 = (uint4 *)tile;
            for (int e = tid; e < nrow * (W / 4); e += kGmNT) t4[e] = s4[e];
        } else {
            for (int e = tid; e < nrow * dw; e += kGmNT) tile[(e / dw) * W + (e % dw)] = src[e];
        }
        for (int r = tid; r < nrow; r += kGmNT) {
            const size_t g = (size_t)(o1 + base + r);
            const int sx = D.cell1[2 * g], sy = D.cell1[2 * g + 1];
            const int2 wx = gm_window(sx, wl, wr, cols), wy = gm_window(sy, wu, wd, rows);
            win0[r] = make_int4(wx.x, wx.y, wy.x, wy.y);
            if (line) {
                const int ex = D.cell1e[2 * g], ey = D.cell1e[2 * g + 1];
                const int2 vx = gm_window(ex, wl, wr, cols), vy = gm_window(ey, wu, wd, rows);
                win1[r] = make_int4(vx.x, vx.y, vy.x, vy.y);
                // matching.cpp:210-211: the integer difference, normalised; a zero vector gives NaN
                const double ux = (double)((long long)ex - sx), uy = (double)((long long)ey - sy);
                qdir[r] = gm_normalize(ux, uy);
            }
            lkey[r] = kGmNone;
            if (PASS == 1) lbest[r] = D.best[g];
        }
        __syncthreads();
        if (owner && ncell > 0) {
            for (int j = 0; j < nrow; ++j) {
                const int4 w0 = win0[j];
                bool cand = !(bx1 < w0.x || bx0 >= w0.y || by1 < w0.z || by0 >= w0.w);
                int4 w1 = w0;
                if (line) {
                    w1 = win1[j];
                    cand = cand || !(bx1 < w1.x || bx0 >= w1.y || by1 < w1.z || by0 >= w1.w);
                }
                if (!cand) continue;
                if (ncell > 1) {  // the bounding box overlaps a window: the cells decide
                    cand = false;
                    if (in_lds) {
                        for (int c = coff; c < coff + ncell && !cand; ++c) {
                            const int2 v = lcell[c];
                            cand = gm_in(w0, v.x, v.y) || gm_in(w1, v.x, v.y);
                        }
                    } else {
                        for (int c = c0; c < c1 && !cand; ++c) {
                            const int cx = D.cells2[2 * c], cy = D.cells2[2 * c + 1];
                            cand = gm_in(w0, cx, cy) || gm_in(w1, cx, cy);
                        }
                    }
                    if (!cand) continue;
                } else if (!(gm_in(w0, onex, oney) || gm_in(w1, onex, oney))) {
                    continue;
                }
                if (line) {  // matching.cpp:221: a product sum without contraction, as the host compiles it
                    if (fabs(gm_dot(qdir[j], d2)) < th) continue;  // false for NaN: a degenerate query direction passes
                }
                const uint4 *q4 = (const uint4 *)(tile + j * W);
                int d = 0;
#pragma unroll
                for (int c = 0; c < W / 4; ++c) {
                    const uint4 v = q4[c];
                    d += __popc(t[4 * c] ^ v.x) + __popc(t[4 * c + 1] ^ v.y) + __popc(t[4 * c + 2] ^ v.z) +
                         __popc(t[4 * c + 3] ^ v.w);
                }
                if (D.best_lr) {  // matching.cpp:145-150
                    if (d < colmin) {
                        colmin = d;
                        m21 = base + j;
                    } else {
                        continue;
                    }
                }
                const uint32_t key = ((uint32_t)d << 16) | (uint32_t)i2;
                if (PASS == 0) atomicMin(&lkey[j], key);
                else if (key != lbest[j]) atomicMin(&lkey[j], key);
            }
        }
        __syncthreads();
        uint32_t *dst = PASS == 0 ? D.best : D.second;
        for (int r = tid; r < nrow; r += kGmNT)
            if (lkey[r] != kGmNone) atomicMin(&dst[o1 + base + r], lkey[r]);
    }
    if (PASS == 0 && owner) D.m21[o2 + i2] = m21;
}

__global__ __launch_bounds__(kGmRowsNT) void k_grid_rows(GmDev D) {
    __shared__ int wsum[kGmRowsNT / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int o1 = D.off1[p], n1 = D.off1[p + 1] - o1, o2 = D.off2[p];
    const double nnr = D.nnr[p];
    int cnt = 0;
    for (int i1 = tid; i1 < n1; i1 += kGmRowsNT) {
        const uint32_t k0 = D.best[o1 + i1], k1 = D.second[o1 + i1];
        const int best_d = k0 == kGmNone ? INT_MAX : (int)(k0 >> 16);
        const int best_d2 = k1 == kGmNone ? INT_MAX : (int)(k1 >> 16);
        int i2 = -1;
        // matching.cpp:160; a row with no seen pair (INT_MAX < INT_MAX * nnr above nnr = 1) stays unmatched
        if (k0 != kGmNone && (double)best_d < (double)best_d2 * nnr) i2 = (int)(k0 & 0xFFFFu);
        if (D.best_lr && i2 >= 0 && D.m21[o2 + i2] != i1) i2 = -1;  // matching.cpp:166-174
        D.m12[o1 + i1] = i2;
        cnt += i2 >= 0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < kGmRowsNT / 64; ++w) s += wsum[w];
        D.count[p] = s;
    }
}

}  // namespace plba
