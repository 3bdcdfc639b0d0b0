// Descriptor matching on the device (plba_desc_match): StVO::match / StVO::matchNNR
// (src2/matching.cpp:41-91), the brute-force Hamming matcher behind isLoopClosure
// (src/mapHandler.cpp:4334, :4360) and every other matching step of the back end: the two nearest
// train rows of every query row, the nearest-neighbour-ratio test in single precision (:54) and the
// left/right cross-check (:80-86). A call handles a batch of descriptor-set pairs in two launches.
//
//   k_desc_nn     grid (pair, row tile, direction), 256 threads. Direction 0 matches desc1 -> desc2,
//                 direction 1 desc2 -> desc1, in the same launch. A thread owns one query row, held
//                 as W dwords in registers (desc_bytes zero-padded to 32 or 64 bytes: the padding
//                 xors to zero). The train rows go through LDS in tiles of 256 rows; every thread
//                 reads the same LDS address at the same time (a broadcast, no bank conflict) and
//                 keeps d0, i0, d1 in registers. The tile loop's bounds depend on the pair alone, so
//                 every thread reaches every barrier; the tail rows of the query side compute on a
//                 zero row and write nothing, the tail of the train side is outside the row loop.
//                 Train rows are scanned in increasing index; a distance replaces the best only if
//                 strictly smaller, else the second only if strictly smaller: ties go to the lowest
//                 train index (OpenCV's batch distance; matchGrid's own loop, :152-157).
//   k_desc_cross  one workgroup per pair: the cross-check and the count of the survivors, summed
//                 per thread, then over the wave and over the four waves in a fixed order.
// Every element is written by the one thread that owns its index, with ordinary vector stores, so
// the result does not depend on the launch geometry.
// plba_kf_associate launches both kernels over every problem with a gate (DmDev::gate_count): a
// workgroup of a problem that does not fall back returns at once and writes nothing.
// plba_map_associate launches the MASK instantiation of k_desc_nn with DmDev::skip1, a flag per side-1
// row: a flagged row is what a row removed from the list would be. As a query (direction 0) it gets -1;
// as a train row (direction 1) the scan passes over it, and the scan keeps the order of the others, so
// ties still go to the lowest index among them. Without the flags the kernel is the one it was.
// Defined where the reference is not: fewer than 2 train rows give no match in that direction (the
// reference reads matches_[idx][1] out of range); with MASK, fewer than 2 unflagged ones.
#pragma once

#include <limits.h>

#include "plba_assoc_args.hpp"  // DmDev, kDmNT

namespace plba {

constexpr int kDmTile = 256;  // train rows staged through LDS at a time

// uniform over the workgroup: the pair is switched off by its gate
__device__ inline bool dm_gated_off(const DmDev &D, int pair) {
    return D.gate_count && !(D.gate_count[pair] < D.gate_min[pair]);
}

// W: dwords of a row in registers and in LDS (8 or 16), dwords <= W. MASK: D.skip1 is read
template <int W, bool MASK = false>
__global__ __launch_bounds__(kDmNT) void k_desc_nn(DmDev D) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[kDmTile * W];
    __shared__ uint8_t tskip[MASK ? kDmTile : 1];  // direction 1: the flags of the tile's side-1 rows
    const int pair = blockIdx.x, dir = blockIdx.z, tid = threadIdx.x;
    const int32_t *qoff = dir ? D.off2 : D.off1, *toff = dir ? D.off1 : D.off2;
    const int q0 = qoff[pair], nq = qoff[pair + 1] - q0;
    const int t0 = toff[pair], nt = toff[pair + 1] - t0;
    const int row = blockIdx.y * kDmNT + tid;
    if ((int)blockIdx.y * kDmNT >= nq || dm_gated_off(D, pair)) return;  // the whole workgroup, before any barrier
    const int dw = D.dwords;
    const uint32_t *qd = dir ? D.desc2 : D.desc1, *td = dir ? D.desc1 : D.desc2;
    const bool owner = row < nq;

    uint32_t q[W];
#pragma unroll
    for (int c = 0; c < W; ++c) q[c] = 0u;
    if (owner) {
        const uint32_t *src = qd + (size_t)(q0 + row) * dw;
        if (dw == W) {  // rows of 32 or 64 bytes start on 16 bytes
            const uint4 *s4 = (const uint4 *)src;
#pragma unroll
            for (int c = 0; c < W / 4; ++c) {
                const uint4 v = s4[c];
                q[4 * c] = v.x; q[4 * c + 1] = v.y; q[4 * c + 2] = v.z; q[4 * c + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c < dw) q[c] = src[c];
        }
    }
    if (dw != W)  // the padding columns, never written again
        for (int e = tid; e < kDmTile * W; e += kDmNT) tile[e] = 0u;

    int d0 = INT_MAX, d1 = INT_MAX, i0 = -1;
    for (int base = 0; base < nt; base += kDmTile) {
        const int rows = min(kDmTile, nt - base);
        __syncthreads();  // the previous tile has been read (and the padding is in place)
        const uint32_t *src = td + (size_t)(t0 + base) * dw;
        if (dw == W) {    // the tile is one contiguous, 16-byte aligned run: coalesced 16-byte loads
            const uint4 *s4 = (const uint4 *)src;
            uint4 *t4 = (uint4 *)tile;
            for (int e = tid; e < rows * (W / 4); e += kDmNT) t4[e] = s4[e];
        } else {
            for (int e = tid; e < rows * dw; e += kDmNT) tile[(e / dw) * W + (e % dw)] = src[e];
        }
        if (MASK && dir)
            for (int e = tid; e < rows; e += kDmNT) tskip[e] = D.skip1[t0 + base + e];
        __syncthreads();
        for (int j = 0; j < rows; ++j) {
            if (MASK && dir && tskip[j]) continue;  // uniform over the workgroup
            const uint4 *t4 = (const uint4 *)(tile + j * W);
            int d = 0;
#pragma unroll
            for (int c = 0; c < W / 4; ++c) {
                const uint4 v = t4[c];
                d += __popc(q[4 * c] ^ v.x) + __popc(q[4 * c + 1] ^ v.y) + __popc(q[4 * c + 2] ^ v.z) +
                     __popc(q[4 * c + 3] ^ v.w);
            }
            if (d < d0) {
                d1 = d0;
                d0 = d;
                i0 = base + j;
            } else if (d < d1) {
                d1 = d;
            }
        }
    }
    if (owner) {
        // matching.cpp:54 — a float product and a float compare
        const float lhs = (float)d0, rhs = (float)d1 * D.nnr[pair];
        // two rows were scanned: nt >= 2, or with MASK a second distance was kept
        const bool two = MASK ? d1 != INT_MAX : nt >= 2;
        const bool skipped = MASK && !dir && D.skip1[q0 + row] != 0;
        (dir ? D.nn21 : D.nn12)[q0 + row] = (two && !skipped && lhs < rhs) ? i0 : -1;
    }
}

__global__ __launch_bounds__(kDmNT) void k_desc_cross(DmDev D) {
    __shared__ int wsum[kDmNT / 64];
    const int pair = blockIdx.x, tid = threadIdx.x;
    if (dm_gated_off(D, pair)) return;  // the whole workgroup, before the barrier
    const int o1 = D.off1[pair], n1 = D.off1[pair + 1] - o1, o2 = D.off2[pair];
    int cnt = 0;
    for (int i1 = tid; i1 < n1; i1 += kDmNT) {
        int i2 = D.nn12[o1 + i1];
        if (D.best_lr && i2 >= 0 && D.nn21[o2 + i2] != i1) i2 = -1;  // matching.cpp:80-86
        D.m12[o1 + i1] = i2;
        cnt += i2 >= 0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < kDmNT / 64; ++w) s += wsum[w];
        D.count[pair] = s;
    }
}

}  // namespace plba
