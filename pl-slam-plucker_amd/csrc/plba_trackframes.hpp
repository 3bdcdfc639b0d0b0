// Frame-to-frame tracking on the device (plba_track_frames): what lies between the matcher and the pose
// in StereoFrameHandler::f2fTracking + optimizePose (src2/stereoFrameHandler.cpp:106-180, :307-405).
// The matcher is k_desc_nn / k_desc_cross (csrc/plba_match.hpp) over the problems 2 k (the points of
// pair k) and 2 k + 1 (its lines); the pose is k_trackpose (csrc/plba_trackpose.hpp). Both are launched
// as they are. The two kernels here turn the one's output into the other's input and back:
//
//   k_f2f_gather   one workgroup per problem, its previous rows in blocks of 256 in index order. A row
//                  with a match is kept; its rank is the matches of the same kind in the pairs before
//                  (the matcher's counts, summed), plus the matches of the blocks before, plus a ballot
//                  and a popcount below its lane, plus the totals of the waves before it: the rows of
//                  matched_pt / matched_ls in push_back order (:150, :177), pairs back to back, so the
//                  pose kernel reads ranges as plba_track_pose's caller would have written them. The
//                  thread copies the previous row and the current row's observation to that rank, and
//                  its i1 for the way back. cur_from_prev starts at -1 in the workgroup that owns the
//                  current rows and takes the maximum i1 of the rows that name it: the last writer of
//                  :151 / :178. Integer atomics on a maximum: the result does not depend on their order.
//   k_f2f_scatter  after the pose: the inlier flag of every match row to its previous row.
// Every other element is written by the one thread that owns its index, with ordinary vector stores.
#pragma once

#include "plba_assoc_args.hpp"  // TfDev, kTfNT

namespace plba {

__global__ __launch_bounds__(kTfNT) void k_f2f_gather(TfDev F) {
    __shared__ int wtot[kTfNT / 64];
    const int p = blockIdx.x, pair = p >> 1, kind = p & 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o1 = F.off1[p], n1 = F.off1[p + 1] - o1, n2 = F.off2[p + 1] - F.off2[p];
    const int kb1 = F.kb1[p], kb2 = F.kb2[p];
    const bool on = F.on[kind] != 0;  // :137 / :160: a kind that is switched off has no match
    int32_t *const cfp = F.cfp[kind] + kb2;

    // the first match row of the pair: the counts of its kind in the pairs before (all 0 if switched off)
    int first = 0;
    if (on)
        for (int j = tid; j < pair; j += kTfNT) first += F.count[2 * j + kind];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) first += __shfl_xor(first, m, 64);
    if (lane == 0) wtot[wave] = first;
    for (int i2 = tid; i2 < n2; i2 += kTfNT) cfp[i2] = -1;
    __syncthreads();  // wtot; and every -1 is in place before the first maximum
    first = 0;
    for (int w = 0; w < kTfNT / 64; ++w) first += wtot[w];
    __syncthreads();  // wtot is written again

    int base = first;
    // the loop's bounds depend on the problem alone: every thread reaches every barrier
    for (int b0 = 0; b0 < n1; b0 += kTfNT) {
        const int i1 = b0 + tid;
        int i2 = -1;
        if (i1 < n1) {
            if (on) i2 = F.m12[o1 + i1];
            F.om12[kind][kb1 + i1] = i2;
            F.inl[kind][kb1 + i1] = 0;
        }
        const bool keep = i2 >= 0;
        const unsigned long long mask = __ballot(keep);
        const int incl = __popcll(mask & ((2ull << lane) - 1ull));  // lane 63: 2 << 63 wraps to 0, the mask is all ones
        if (lane == 0) wtot[wave] = __popcll(mask);
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < kTfNT / 64; ++w) {
            if (w < wave) before += wtot[w];
            total += wtot[w];
        }
        const int r = before + incl - 1;
        if (keep && r < F.cap[kind]) {  // (it always is: matches cannot exceed previous rows)
            const size_t q = (size_t)r, a = (size_t)(kb1 + i1), c = (size_t)(kb2 + i2);
            if (kind == 0) {
                for (int k = 0; k < 3; ++k) F.g_pt_P[3 * q + k] = F.p_P[3 * a + k];
                for (int k = 0; k < 2; ++k) F.g_pt_obs[2 * q + k] = F.c_pl[2 * c + k];
                F.g_pt_s2[q] = F.p_s2[a];
            } else {
                for (int k = 0; k < 3; ++k) F.g_ln_sP[3 * q + k] = F.l_sP[3 * a + k];
                for (int k = 0; k < 3; ++k) F.g_ln_eP[3 * q + k] = F.l_eP[3 * a + k];
                for (int k = 0; k < 4; ++k) F.g_ln_seg[4 * q + k] = F.l_seg[4 * a + k];
                F.g_ln_s2[q] = F.l_s2[a];
                if (F.pluker) {
                    for (int k = 0; k < 6; ++k) F.g_ln_ND[6 * q + k] = F.l_ND[6 * a + k];
                    for (int k = 0; k < 4; ++k) F.g_ln_obs[4 * q + k] = F.c_seg[4 * c + k];
                } else {
                    for (int k = 0; k < 3; ++k) F.g_ln_le[3 * q + k] = F.c_le[3 * c + k];
                }
            }
            F.src[kind][q] = i1;
            atomicMax(&cfp[i2], i1);
        }
        base += total;
        __syncthreads();  // wtot is written again
    }
    if (tid == 0) {
        F.g_off[kind][pair] = first;
        if (pair == F.n - 1) F.g_off[kind][F.n] = base;
        F.nm[kind][pair] = base - first;
    }
}

__global__ __launch_bounds__(kTfNT) void k_f2f_scatter(TfDev F) {
    const int p = blockIdx.x, pair = p >> 1, kind = p & 1;
    const int r0 = F.g_off[kind][pair], n = F.g_off[kind][pair + 1] - r0, kb1 = F.kb1[p];
    for (int i = threadIdx.x; i < n; i += kTfNT) F.inl[kind][kb1 + F.src[kind][r0 + i]] = F.tin[kind][r0 + i];
}

}  // namespace plba
