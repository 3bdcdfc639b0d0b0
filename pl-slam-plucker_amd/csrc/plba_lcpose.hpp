// Loop-closure relative pose on the device (plba_lc_relative_pose):
// MapHandler::computeRelativePoseRobustGN (src/mapHandler.cpp:4677-5068, what isLoopClosure calls)
// and MapHandler::computeRelativePoseGN (:4413-4675). A robust pose-only Gauss–Newton over the 3-D
// points and line endpoints of the old keyframe reprojected into the new one: a first loop, an
// outlier pass, (RobustGN) a refinement loop and a five-way accept test.
//
//   k_lcpose   one workgroup of 256 threads per candidate pair, the whole function in one launch.
//              Threads stride over the candidate's active points, then its active lines, with the 21
//              upper entries of H, g, e and the active count in registers; the sums are reduced by
//              an xor butterfly inside each wave and over the four waves through LDS in wave order
//              (the same input gives bitwise the same output). Thread 0 then runs the serial part:
//              the stop tests, x = H⁻¹g by column-pivoted Householder QR, T_inc ← T_inc·exp(x)⁻¹.
//              The continue / stop decision goes through LDS and is read by every thread after a
//              barrier, so every thread of the workgroup reaches every barrier.
// Kept from the reference: fx in both Jacobian rows, the left-perturbation step applied on the
// right, err_prev carried from the first loop into the refinement, lc_inl forced true in RobustGN.
// Defined where the reference is not: a candidate with no active feature (empty, or emptied by the
// outlier pass) is rejected with T_inc left as it was; a singular H is rejected (unc = +inf); a
// non-finite H or g (a match with z = 0) gives a NaN step, every later comparison is false and
// the candidate is rejected at the caps.
// No FMA contraction, like the checker (tests/ref_lcpose.py) and the se(3) maps of plba_math.hpp.
#pragma once

#include <float.h>

#include "../../include/plba.h"
#include "plba_math.hpp"
#include "plba_posegn.hpp"

namespace plba {

constexpr int kLcNT = 256;                // threads of a candidate's workgroup
constexpr int kLcWaves = kLcNT / 64;
constexpr int kLcAcc = 29;                // 21 upper entries of H | 6 of g | e | active count

struct LcDev {
    const int32_t *pt_off, *ln_off;       // [n+1] feature ranges of each candidate
    const double *pt_P, *pt_obs;          // [.][3] P of kf0, [.][2] pl of kf1
    const double *ln_sP, *ln_eP, *ln_le;  // [.][3] endpoints of kf0, [.][3] image line of kf1
    uint8_t *pt_in, *ln_in;               // [.] inlier flags
    plba_lcpose_out *out;                 // [n]
    Cam cam;
    plba_lcpose_params prm;
};

namespace lcp {
#pragma clang fp contract(off)
using namespace pgn;  // xform, project, jrow, Work, qr_solve, min_eig, the reduction (csrc/plba_posegn.hpp)

// point residual (dx, dy) and the projected point
__device__ __forceinline__ double point_res(const Cam &c, const double *T, const double *P, const double *obs, double *G,
                                            double &dx, double &dy) {
#pragma clang fp contract(off)
    xform(T, P, G);
    double u, v;
    project(c, G, u, v);
    dx = u - obs[0];
    dy = v - obs[1];
    return sqrt(dx * dx + dy * dy);
}

// line residual (ds, de): the distances of both projected endpoints to the observed image line
__device__ __forceinline__ double line_res(const Cam &c, const double *T, const double *sP, const double *eP,
                                           const double *le, double *Gs, double *Ge, double &ds, double &de) {
#pragma clang fp contract(off)
    xform(T, sP, Gs);
    xform(T, eP, Ge);
    double us, vs, ue, ve;
    project(c, Gs, us, vs);
    project(c, Ge, ue, ve);
    ds = le[0] * us + le[1] * vs + le[2];
    de = le[0] * ue + le[1] * ve + le[2];
    return sqrt(ds * ds + de * de);
}

// H += J·Jᵀ·w, g += J·r·w, e += r·r·w, N += 1 (Cauchy weight w = 1/(1+r²), src2/auxiliar.cpp:556-559)
__device__ __forceinline__ void accumulate(double *acc, const double *J, double r) {
#pragma clang fp contract(off)
    const double w = 1.0 / (1.0 + r * r);
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[q++] += J[i] * J[j] * w;
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * r * w;
    acc[27] += r * r * w;
    acc[28] += 1.0;
}

}  // namespace lcp

__global__ __launch_bounds__(kLcNT) void k_lcpose(LcDev d) {
#pragma clang fp contract(off)
    __shared__ double s_part[kLcWaves][kLcAcc];
    __shared__ int s_cnt[kLcWaves][2];
    __shared__ double s_T[16];   // T_inc, row-major 4x4
    __shared__ double s_H[36], s_g[6];
    __shared__ lcp::Work s_w;
    __shared__ int s_stop;       // the pass's continue / stop decision, read by every thread
    const int cand = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = d.pt_off[cand], p1 = d.pt_off[cand + 1], l0 = d.ln_off[cand], l1 = d.ln_off[cand + 1];
    const Cam cam = d.cam;
    const double hth = d.prm.homog_th;
    const double out_th = sqrt(7.815);
    // every feature starts as an inlier. A flag is only ever touched by the thread that owns its
    // index (the same stride in every phase), so the flags need no barrier of their own.
    for (int i = p0 + tid; i < p1; i += kLcNT) d.pt_in[i] = 1;
    for (int i = l0 + tid; i < l1; i += kLcNT) d.ln_in[i] = 1;
    if (tid == 0) {
        for (int k = 0; k < 16; ++k) s_T[k] = (k % 5 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 36; ++k) s_H[k] = 0.0;
        s_stop = 0;
    }
    __syncthreads();
    // thread 0's scalars (data only; no branch of another thread depends on them)
    double err_prev = 999999999.9, e_last = 0.0;
    int iters[2] = {0, 0}, empty = 0;
    const int nphase = d.prm.variant == PLBA_LCPOSE_ROBUST_GN ? 2 : 1;
    for (int phase = 0; phase < nphase; ++phase) {
        const int cap = phase == 0 ? d.prm.max_iters_first : d.prm.max_iters;
        for (int it = 0; it < cap; ++it) {
            double T[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = s_T[k];
            double acc[kLcAcc];
#pragma unroll
            for (int k = 0; k < kLcAcc; ++k) acc[k] = 0.0;
            for (int i = p0 + tid; i < p1; i += kLcNT) {
                if (!d.pt_in[i]) continue;
                double G[3], dx, dy, J[6];
                const double r = lcp::point_res(cam, T, d.pt_P + 3 * (size_t)i, d.pt_obs + 2 * (size_t)i, G, dx, dy);
                lcp::jrow(cam, hth, G, dx, dy, J);
                const double m = fmax(hth, r);
#pragma unroll
                for (int k = 0; k < 6; ++k) J[k] = J[k] / m;
                lcp::accumulate(acc, J, r);
            }
            for (int i = l0 + tid; i < l1; i += kLcNT) {
                if (!d.ln_in[i]) continue;
                const double *le = d.ln_le + 3 * (size_t)i;
                double Gs[3], Ge[3], ds, de, Js[6], Je[6], J[6];
                const double r = lcp::line_res(cam, T, d.ln_sP + 3 * (size_t)i, d.ln_eP + 3 * (size_t)i, le, Gs, Ge, ds, de);
                lcp::jrow(cam, hth, Gs, le[0], le[1], Js);
                lcp::jrow(cam, hth, Ge, le[0], le[1], Je);
                const double m = fmax(hth, r);
#pragma unroll
                for (int k = 0; k < 6; ++k) J[k] = (Js[k] * ds + Je[k] * de) / m;
                lcp::accumulate(acc, J, r);
            }
            // fixed-order reduction: butterfly inside the wave, the four waves in index order
            pgn::wave_reduce<kLcAcc, kLcWaves>(acc, s_part, lane, wave);
            __syncthreads();
            if (tid == 0) {
                double S[kLcAcc];
                pgn::block_sum<kLcAcc, kLcWaves>(s_part, S);
                int stop = 0;
                ++iters[phase];
                if (S[28] == 0.0) {  // no active feature: rejected, T_inc stays
                    empty = 1;
                    stop = 1;
                } else {
                    int q = 0;
#pragma unroll
                    for (int i = 0; i < 6; ++i)
#pragma unroll
                        for (int j = i; j < 6; ++j) {
                            s_H[6 * i + j] = S[q];
                            s_H[6 * j + i] = S[q];
                            ++q;
                        }
#pragma unroll
                    for (int i = 0; i < 6; ++i) s_g[i] = S[21 + i];
                    const double e = S[27] / S[28];
                    e_last = e;
                    if (fabs(e - err_prev) < DBL_EPSILON || e < DBL_EPSILON) {
                        stop = 1;
                    } else {
                        double x[6], E[16], Ei[12], Tn[12];
                        lcp::qr_solve(s_H, s_g, x, s_w);
                        se3_exp(x, E);
                        se3_inv34(E, Ei);
                        // T_inc ← T_inc · inverse_se3(expmap_se3(x)): the step on the right
                        for (int i = 0; i < 3; ++i)
                            for (int j = 0; j < 4; ++j) {
                                double s = 0.0;
                                for (int k = 0; k < 3; ++k) s += s_T[4 * i + k] * Ei[4 * k + j];
                                s += s_T[4 * i + 3] * (j == 3 ? 1.0 : 0.0);
                                Tn[4 * i + j] = s;
                            }
                        for (int k = 0; k < 12; ++k) s_T[k] = Tn[k];
                        double n2 = 0.0;
                        for (int k = 0; k < 6; ++k) n2 += x[k] * x[k];
                        if (sqrt(n2) < DBL_EPSILON) stop = 1;
                        else err_prev = e;
                    }
                }
                s_stop = stop;
            }
            __syncthreads();
            if (s_stop) break;  // an LDS value: the same for every thread of the workgroup
        }
        if (phase == 0) {  // the outlier pass at the pose of the first loop (:4829-4860)
            double T[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = s_T[k];
            for (int i = p0 + tid; i < p1; i += kLcNT) {
                if (!d.pt_in[i]) continue;
                double G[3], dx, dy;
                if (lcp::point_res(cam, T, d.pt_P + 3 * (size_t)i, d.pt_obs + 2 * (size_t)i, G, dx, dy) > out_th)
                    d.pt_in[i] = 0;
            }
            for (int i = l0 + tid; i < l1; i += kLcNT) {
                if (!d.ln_in[i]) continue;
                double Gs[3], Ge[3], ds, de;
                if (lcp::line_res(cam, T, d.ln_sP + 3 * (size_t)i, d.ln_eP + 3 * (size_t)i, d.ln_le + 3 * (size_t)i, Gs, Ge, ds,
                                  de) > out_th)
                    d.ln_in[i] = 0;
            }
        }
    }
    // inlier counts, then the tail on thread 0
    int npi = 0, nli = 0;
    for (int i = p0 + tid; i < p1; i += kLcNT) npi += d.pt_in[i] ? 1 : 0;
    for (int i = l0 + tid; i < l1; i += kLcNT) nli += d.ln_in[i] ? 1 : 0;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        npi += __shfl_xor(npi, m, 64);
        nli += __shfl_xor(nli, m, 64);
    }
    if (lane == 0) {
        s_cnt[wave][0] = npi;
        s_cnt[wave][1] = nli;
    }
    __syncthreads();
    if (tid != 0) return;  // (no barrier below)
    npi = nli = 0;
    for (int wv = 0; wv < kLcWaves; ++wv) {
        npi += s_cnt[wv][0];
        nli += s_cnt[wv][1];
    }
    plba_lcpose_out &o = d.out[cand];
    double x_inc[6], pose[6], Ti[12];
    se3_log(s_T, x_inc);
    const double t = sqrt(x_inc[0] * x_inc[0] + x_inc[1] * x_inc[1] + x_inc[2] * x_inc[2]);
    const double r_deg = sqrt(x_inc[3] * x_inc[3] + x_inc[4] * x_inc[4] + x_inc[5] * x_inc[5]) * 180.0 / 3.14159265358979323846;
    const double lmin = lcp::min_eig(s_H, s_w);
    const double unc = lmin > 0.0 ? 1.0 / lmin : INFINITY;  // the largest eigenvalue of H⁻¹
    if (d.prm.variant == PLBA_LCPOSE_ROBUST_GN) {  // logmap(inverse(expmap(x_inc))) (:5062)
        double E[16];
        se3_exp(x_inc, E);
        se3_inv34(E, Ti);
    } else {                                       // logmap(inverse(T_inc)) (:4669)
        se3_inv34(s_T, Ti);
    }
    se3_log(Ti, pose);
    const int n_all = (p1 - p0) + (l1 - l0);
    int cond = 0;
    if (e_last < d.prm.lc_res) cond |= 1;
    if (unc < d.prm.lc_unc) cond |= 2;
    if (d.prm.variant == PLBA_LCPOSE_ROBUST_GN || (double)(npi + nli) / (double)n_all > d.prm.lc_inl) cond |= 4;
    if (t < d.prm.lc_trs) cond |= 8;
    if (r_deg < d.prm.lc_rot) cond |= 16;
    o.accepted = (cond == 31 && !empty) ? 1 : 0;
    o.conditions = cond;
    o.iters_first = iters[0];
    o.iters_ref = iters[1];
    o.n_inl_pt = npi;
    o.n_inl_ln = nli;
    o.e = e_last;
    o.unc = unc;
    o.t = t;
    o.r_deg = r_deg;
    for (int k = 0; k < 6; ++k) {
        o.x_inc[k] = x_inc[k];
        o.pose_inc[k] = pose[k];
    }
    for (int k = 0; k < 12; ++k) o.T_inc[k] = s_T[k];
    for (int k = 0; k < 36; ++k) o.H[k] = s_H[k];
}

}  // namespace plba
