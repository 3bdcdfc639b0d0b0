// Batched median descriptor on the device (plba_desc_medoid): the descriptor half of
// MapPoint::updateAverageDescDir / MapLine::updateAverageDescDir (src/mapFeatures.cpp:52-86, :140-174)
// for a batch of descriptor lists, as loopClosureFuseLandmarks needs it once per changed landmark.
// For a list of n descriptors, row i of the symmetric Hamming table (zero diagonal) has a k-th
// smallest value, k = min(int(1 + 0.5 (n - 1)), n - 1); the answer is the first row whose value is
// strictly smaller than that of every earlier row (the reference starts at 99999, above any
// distance), which is the lowest index among the rows with the smallest value.
//
//   k_desc_medoid  one launch, 256 threads (four waves). The host sorts the lists into short ones
//                  (n <= 64) and long ones. A workgroup below n_short_wg takes four short lists, one
//                  per wave, a lane per row; every other workgroup takes one long list and its
//                  threads take the rows tid, tid + 256, ... The descriptors of the list go to LDS
//                  once, zero-padded to W dwords (8 or 16, the padding xors to zero); a thread
//                  keeps its own row in registers and reads row j from LDS, the same address in
//                  every lane (a broadcast). Nothing of the n x n table is stored.
//                  The k-th smallest value of a row is an integer in [0, 32 W], found by counting:
//                  the smallest v with #{j : d(i, j) <= v} >= k + 1, by bisection on v, each
//                  probe one pass over the row (at most 10 passes for 512 bits). No sort.
//                  The rows' (value, index) pairs are packed as value * 65536 + index and reduced
//                  with min: over a thread's rows, the wave (shuffles), and for a long list the
//                  four waves through LDS. Integers only, so the result does not depend on the
//                  geometry.
// The largest list is kMedMaxN = 1024 rows: the list sits in LDS whole, and 1024 rows of 64
// bytes are the 64 KiB a workgroup may have without asking for more; the index also has to fit the
// 16 low bits of the packed pair. A longer list is refused on the host, never truncated.
// n = 0 gives -1, n = 1 gives 0 (k is clamped to n - 1, as median_descriptor() of the host mirror
// clamps it: the reference reads one past the row's end there).
#pragma once

#include <limits.h>

#include "plba_assoc_args.hpp"  // MedDev

namespace plba {

constexpr int kMedNT = 256;       // threads of a workgroup
constexpr int kMedWaves = kMedNT / 64;
constexpr int kMedShort = 64;     // rows of a list that one wave takes, a lane per row
constexpr int kMedMaxN = PLBA_MEDOID_MAX_N;  // rows of the longest list (1024)

// The k-th smallest (0-based) of d(q, row j), j < n, rows of W dwords at `rows`: rank selection by
// bisection on the value, each probe one counting pass.
template <int W>
__device__ inline int med_kth(const uint32_t (&q)[W], const uint32_t *rows, int n, int k) {
    int lo = 0, hi = 32 * W;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
        for (int j = 0; j < n; ++j) {
            const uint4 *t4 = (const uint4 *)(rows + j * W);
            int d = 0;
#pragma unroll
            for (int c = 0; c < W / 4; ++c) {
                const uint4 v = t4[c];
                d += __popc(q[4 * c] ^ v.x) + __popc(q[4 * c + 1] ^ v.y) + __popc(q[4 * c + 2] ^ v.z) +
                     __popc(q[4 * c + 3] ^ v.w);
            }
            cnt += d <= mid;
        }
        if (cnt >= k + 1) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// W: dwords of a row in registers and in LDS (8 or 16), dwords <= W. Dynamic LDS: W dwords for
// each of max(4 * kMedShort, the longest list) rows; the waves' minima of a long list reuse its start.
template <int W>
__global__ __launch_bounds__(kMedNT) void k_desc_medoid(MedDev D) {
    extern __shared__ __attribute__((aligned(16))) uint32_t med_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, dw = D.dwords;
    const bool is_long = (int)blockIdx.x >= D.n_short_wg;  // uniform over the workgroup
    // the list of this wave (short) or of this workgroup (long); -1: a wave past the last short list
    int list = -1;
    if (is_long) list = D.order[D.n_short + ((int)blockIdx.x - D.n_short_wg)];
    else if (4 * (int)blockIdx.x + wave < D.n_short) list = D.order[4 * (int)blockIdx.x + wave];
    const int r0 = list >= 0 ? D.list_ptr[list] : 0;
    const int n = list >= 0 ? D.list_ptr[list + 1] - r0 : 0;
    uint32_t *rows = is_long ? med_lds : med_lds + wave * kMedShort * W;
    // the list to LDS, the padding columns zero
    {
        const uint32_t *src = D.desc + (size_t)r0 * dw;
        const int t = is_long ? tid : lane, nt = is_long ? kMedNT : 64;
        for (int e = t; e < n * W; e += nt) {
            const int r = e / W, c = e % W;
            rows[e] = c < dw ? src[(size_t)r * dw + c] : 0u;
        }
    }
    __syncthreads();  // every thread of every workgroup arrives: nothing above returns
    const int k = min((int)(1 + 0.5 * (n - 1)), n - 1);
    int best = INT_MAX;
    for (int i = is_long ? tid : lane; i < n; i += is_long ? kMedNT : 64) {
        uint32_t q[W];
#pragma unroll
        for (int c = 0; c < W; ++c) q[c] = rows[i * W + c];
        best = min(best, med_kth<W>(q, rows, n, k) * 65536 + i);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) best = min(best, __shfl_xor(best, m, 64));
    if (!is_long) {
        if (lane == 0 && list >= 0) D.medoid[list] = n > 0 ? (best & 0xFFFF) : -1;
        return;  // no barrier below for a workgroup of short lists
    }
    int *wmin = (int *)med_lds;
    __syncthreads();  // every row has been read
    if (lane == 0) wmin[wave] = best;
    __syncthreads();
    if (tid == 0) {
        int b = wmin[0];
        for (int w = 1; w < kMedWaves; ++w) b = min(b, wmin[w]);
        D.medoid[list] = b & 0xFFFF;  // a long list has rows
    }
}

}  // namespace plba
