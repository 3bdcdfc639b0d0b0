// Frame-to-frame pose on the device (plba_track_pose): StereoFrameHandler::optimizePose
// (src2/stereoFrameHandler.cpp:307-405) with its two Gauss–Newton loops, removeOutliers (:1303-1396)
// and isGoodSolution (:292-305); the semantics are spelt out in include/plba.h.
//
//   k_trackpose<MODEL>  one workgroup of 256 threads per frame pair, the whole function in one launch;
//              MODEL is the line model (PLBA_TRACK_PLUCKER / PLBA_TRACK_ENDPOINTS), which changes the
//              line residual, its Jacobian row and the line half of the outlier pass, nothing else.
//              A pass has two sweeps, like the reference's build. The first leaves the residual of
//              every active match in the problem's scratch block; the scales s_p and s_l are then
//              the MAD of each list. The medians are exact order statistics, found by rank selection:
//              the list of a kind sits in LDS (at most PLBA_TRACK_MAX_N doubles), a thread counts for
//              each of its own entries how many entries are smaller (ties by index) and the entry of
//              rank n/2 writes itself to an LDS slot. No sort, no sum: the scales do not depend on the
//              geometry. The second sweep strides over the matches with the 21 upper entries of H,
//              g, e and the count in registers, reduced in the fixed tree of csrc/plba_posegn.hpp
//              (the same input gives bitwise the same output, alone or anywhere in a batch).
//              Thread 0 runs the serial part (stop tests, QR solve, logAbsDeterminant, the update on
//              the left, the inverse and the eigenvalues); every decision goes through LDS and is
//              read by every thread after a barrier, so every thread reaches every barrier, also
//              with a NaN anywhere.
// The arithmetic of a match is csrc/plba_trackpose_geom.hpp, which host/track_pose.cpp compiles too.
// No FMA contraction, like k_lcpose and the checker (tests/ref_trackpose.py).
#pragma once

#include "../../include/plba.h"
#include "plba_assoc_args.hpp"
#include "plba_math.hpp"
#include "plba_trackpose_geom.hpp"

namespace plba {

constexpr int kTpWaves = kTpNT / 64;     // TpDev, kTpNT, kTpMaxN, kTpPrev: csrc/plba_assoc_args.hpp

namespace tpk {

// What the workgroup shares
struct Shared {
    double part[kTpWaves][tpg::kAcc];
    double small[kTpWaves][4];
    double val[kTpMaxN];                 // the list of the running rank selection
    double sel[4];                       // median and MAD of the points, of the lines
    double T[16], T0[16];                // the loop's DT and the initial DT, row-major 4x4
    double H[36], g[6], cov[36];
    pgn::Work w;
    int flow;                            // a decision of thread 0, read by every thread after a barrier
};

// The entry of rank k (ties by index) of val[0..n): it writes itself to *slot, which holds NaN
// beforehand. The caller has a barrier before (val and *slot written) and after (the slot read).
__device__ __forceinline__ void select_rank(const double *val, int n, int k, double *slot, int tid) {
    for (int i = tid; i < n; i += kTpNT) {
        const double v = val[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double u = val[j];  // the same address in every lane: a broadcast
            rank += (u < v || (u == v && j < i)) ? 1 : 0;
        }
        if (rank == k) *slot = v;
    }
}

// The MAD of the na entries of res[base .. base + n) whose flag is set (in == nullptr: all of them):
// element na/2 of the sorted list, then element na/2 of the sorted float deviations from it
// (src2/auxiliar.cpp:444-460). slot[0] receives the median, slot[1] the MAD; both hold NaN beforehand.
// n and na are the same in every thread; a barrier comes first, so the caller needs none after writing res.
__device__ __forceinline__ double mad(Shared &s, const double *res, const uint8_t *in, int base, int n, int na,
                                      double *slot, int tid) {
    if (na == 0) return 0.0;
    for (int i = tid; i < n; i += kTpNT) s.val[i] = (!in || in[base + i]) ? res[base + i] : INFINITY;
    __syncthreads();
    select_rank(s.val, n, na / 2, &slot[0], tid);
    __syncthreads();
    const double med = slot[0];
    for (int i = tid; i < n; i += kTpNT) s.val[i] = (!in || in[base + i]) ? tpg::mad_dev(res[base + i], med) : INFINITY;
    __syncthreads();
    select_rank(s.val, n, na / 2, &slot[1], tid);
    __syncthreads();
    return slot[1];
}

// The sums of four per-thread values over the workgroup, in every thread (fixed tree)
__device__ __forceinline__ void sum4(Shared &s, const double *v, double *S, int lane, int wave) {
    pgn::wave_reduce<4, kTpWaves>(v, s.small, lane, wave);
    __syncthreads();
    pgn::block_sum<4, kTpWaves>(s.small, S);
    __syncthreads();  // s.small may be written again
}

// rows 0-2 of inverse_se3(expmap_se3(x))·T, row 3 of T kept (:474, :831)
__device__ void step_left(const double *x, double *T) {
#pragma clang fp contract(off)
    double E[16], Ei[12], Tn[12];
    se3_exp(x, E);
    se3_inv34(E, Ei);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double a = 0.0;
            for (int k = 0; k < 4; ++k) a += Ei[4 * i + k] * T[4 * k + j];
            Tn[4 * i + j] = a;
        }
    for (int k = 0; k < 12; ++k) T[k] = Tn[k];
}

}  // namespace tpk

template <int MODEL>
__global__ __launch_bounds__(kTpNT) void k_trackpose(TpDev d) {
#pragma clang fp contract(off)
    __shared__ tpk::Shared s;
    const int prob = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = d.pt_off[prob], np = d.pt_off[prob + 1] - p0, l0 = d.ln_off[prob], nl = d.ln_off[prob + 1] - l0;
    const Cam cam{d.fx, d.fy, d.cx, d.cy};
    const plba_track_params prm = d.prm;
    const double hth = prm.homog_th;
    // every match starts as an inlier. A flag and a residual are only ever touched by the thread that
    // owns the index (the same stride in every phase), so they need no barrier of their own.
    for (int i = tid; i < np; i += kTpNT) d.pt_in[p0 + i] = 1;
    for (int i = tid; i < nl; i += kTpNT) d.ln_in[l0 + i] = 1;
    // thread 0's scalars (data only; every branch that holds a barrier is decided through s.flow)
    double err = -1.0, s_p = 0.0, s_l = 0.0;
    int iters[2] = {0, 0}, branch = PLBA_TRACK_OK;
    int na_p = np, na_l = nl;  // active matches of each kind: the same in every thread
    if (tid == 0) {
        for (int k = 0; k < 16; ++k) s.T0[k] = (k % 5 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 36; ++k) s.H[k] = s.cov[k] = 0.0;
        if (prm.use_motion_model) {  // :317-324
            const double *pv = d.prev + (size_t)kTpPrev * prob;
            double ev[6];
            for (int k = 0; k < 36; ++k) s.cov[k] = pv[16 + k];
            pgn::eig6_sorted(s.cov, ev, s.w);
            if (tpg::is_good(ev, pv[52], pv))
                for (int k = 0; k < 16; ++k) s.T0[k] = pv[k];
        }
        for (int k = 0; k < 16; ++k) s.T[k] = s.T0[k];
    }
    __syncthreads();

    // One Gauss–Newton loop on s.T over the active matches (:446-494 / :803-853)
    auto run_loop = [&](int cap, int phase) {
        double err_prev = 999999999.9, e_last = 0.0;  // thread 0's
        int bad = 0;
        for (int it = 0; it < cap; ++it) {
            double T[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = s.T[k];
            if (tid < 4) s.sel[tid] = NAN;
            // first sweep: the residual lists
            for (int i = tid; i < np; i += kTpNT) {
                if (!d.pt_in[p0 + i]) continue;
                double G[3], dx, dy;
                d.pt_res[p0 + i] = tpg::point_res(cam, T, d.pt_P + 3 * (size_t)(p0 + i), d.pt_obs + 2 * (size_t)(p0 + i), G, dx, dy);
            }
            for (int i = tid; i < nl; i += kTpNT) {
                if (!d.ln_in[l0 + i]) continue;
                const size_t q = (size_t)(l0 + i);
                if (MODEL == PLBA_TRACK_PLUCKER) {
                    tpg::PlLine L;
                    d.ln_res[q] = tpg::line_res_pl(cam, T, d.ln_ND + 6 * q, d.ln_obs + 4 * q, L);
                } else {
                    double Gs[3], Ge[3], ps[2], pe[2], ds, de;
                    tpg::line_proj(cam, T, d.ln_sP + 3 * q, d.ln_eP + 3 * q, Gs, Ge, ps, pe);
                    d.ln_res[q] = tpg::line_res_ep(d.ln_le + 3 * q, ps, pe, ds, de);
                }
            }
            s_p = tpg::clamp_scale(tpk::mad(s, d.pt_res, d.pt_in, p0, np, na_p, &s.sel[0], tid));
            s_l = tpg::clamp_scale(tpk::mad(s, d.ln_res, d.ln_in, l0, nl, na_l, &s.sel[2], tid));
            // second sweep: H, g, e
            double acc[tpg::kAcc];
#pragma unroll
            for (int k = 0; k < tpg::kAcc; ++k) acc[k] = 0.0;
            for (int i = tid; i < np; i += kTpNT) {
                if (!d.pt_in[p0 + i]) continue;
                double G[3], dx, dy, J[6];
                const double r = tpg::point_res(cam, T, d.pt_P + 3 * (size_t)(p0 + i), d.pt_obs + 2 * (size_t)(p0 + i), G, dx, dy);
                tpg::point_row(cam, hth, G, dx, dy, r, J);
                tpg::accumulate(acc, J, r, r, tpg::cauchy(r, s_p));
            }
            for (int i = tid; i < nl; i += kTpNT) {
                if (!d.ln_in[l0 + i]) continue;
                const size_t q = (size_t)(l0 + i);
                double Gs[3], Ge[3], ps[2], pe[2], J[6], r, rg;
                tpg::line_proj(cam, T, d.ln_sP + 3 * q, d.ln_eP + 3 * q, Gs, Ge, ps, pe);
                if (MODEL == PLBA_TRACK_PLUCKER) {
                    tpg::PlLine L;
                    r = tpg::line_res_pl(cam, T, d.ln_ND + 6 * q, d.ln_obs + 4 * q, L);
                    tpg::line_row_pl(cam, hth, T, d.ln_obs + 4 * q, L, r, J);
                    rg = r * sqrt(d.ln_s2[q]);
                } else {
                    double ds, de;
                    r = tpg::line_res_ep(d.ln_le + 3 * q, ps, pe, ds, de);
                    tpg::line_row_ep(cam, hth, Gs, Ge, d.ln_le + 3 * q, ds, de, r, J);
                    rg = r;
                }
                const double w = tpg::cauchy(r, s_l) * st_overlap2d(d.ln_seg + 4 * q, d.ln_seg + 4 * q + 2, ps, pe);
                tpg::accumulate(acc, J, rg, r, w);
            }
            pgn::wave_reduce<tpg::kAcc, kTpWaves>(acc, s.part, lane, wave);
            __syncthreads();
            if (tid == 0) {
                double S[tpg::kAcc];
                pgn::block_sum<tpg::kAcc, kTpWaves>(s.part, S);
                int stop = 0, q = 0;
                ++iters[phase];
                for (int i = 0; i < 6; ++i)
                    for (int j = i; j < 6; ++j) {
                        s.H[6 * i + j] = S[q];
                        s.H[6 * j + i] = S[q];
                        ++q;
                    }
                for (int i = 0; i < 6; ++i) s.g[i] = S[21 + i];
                const double e = S[27] / S[28];  // no active match: 0 / 0
                e_last = e;
                if (S[28] == 0.0 || fabs(e - err_prev) < prm.min_error_change || e < prm.min_error) {
                    stop = 1;
                } else {
                    double x[6], logdet;
                    pgn::qr_solve(s.H, s.g, x, s.w, &logdet);
                    if (logdet < 0.0) {  // solution_is_good = false
                        bad = 1;
                        stop = 1;
                    } else {
                        tpk::step_left(x, s.T);
                        double n2 = 0.0;
                        for (int k = 0; k < 6; ++k) n2 += x[k] * x[k];
                        if (sqrt(n2) < prm.min_error_change) stop = 1;
                        else err_prev = e;
                    }
                }
                s.flow = stop;
            }
            __syncthreads();
            if (s.flow) break;  // an LDS value: the same for every thread of the workgroup
        }
        if (tid == 0) {
            if (!bad) {
                pgn::inverse6(s.H, s.cov, s.w);
                err = e_last;
            } else {
                for (int k = 0; k < 16; ++k) s.T[k] = s.T0[k];
                for (int k = 0; k < 36; ++k) s.cov[k] = (k % 7 == 0) ? 1.0 : 0.0;
                err = -1.0;
            }
        }
        __syncthreads();
    };

    if (np + nl < prm.min_features) {  // :377-381 (the same in every thread)
        branch = PLBA_TRACK_FEW_BEFORE;
        if (tid == 0)
            for (int k = 0; k < 16; ++k) s.T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    } else {
        run_loop(prm.max_iters, 0);
        if (tid == 0) {
            double ev[6];
            pgn::eig6_sorted(s.cov, ev, s.w);
            s.flow = tpg::is_good(ev, err, s.T) ? 1 : 0;
        }
        __syncthreads();
        const int good = s.flow;
        __syncthreads();  // s.flow is written again in the second loop
        if (good) {
            // removeOutliers at the first loop's DT_, over all matches (:1303-1396)
            double T[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = s.T[k];
            if (tid < 4) s.sel[tid] = NAN;
            for (int kind = 0; kind < 2; ++kind) {
                if (!(kind ? prm.has_lines : prm.has_points)) continue;
                const int base = kind ? l0 : p0, n = kind ? nl : np;
                double *res = kind ? d.ln_res : d.pt_res;
                uint8_t *in = kind ? d.ln_in : d.pt_in;
                for (int i = tid; i < n; i += kTpNT) {
                    const size_t q = (size_t)(base + i);
                    double r;
                    if (kind == 0) {
                        double G[3], dx, dy;
                        r = tpg::point_res(cam, T, d.pt_P + 3 * q, d.pt_obs + 2 * q, G, dx, dy) * sqrt(d.pt_s2[q]);
                    } else if (MODEL == PLBA_TRACK_PLUCKER) {
                        tpg::PlLine L;
                        r = tpg::line_res_pl(cam, T, d.ln_ND + 6 * q, d.ln_obs + 4 * q, L) * sqrt(d.ln_s2[q]);
                    } else {
                        double Gs[3], Ge[3], ps[2], pe[2], ds, de;
                        tpg::line_proj(cam, T, d.ln_sP + 3 * q, d.ln_eP + 3 * q, Gs, Ge, ps, pe);
                        r = tpg::line_res_ep(d.ln_le + 3 * q, ps, pe, ds, de) * sqrt(d.ln_s2[q]);
                    }
                    res[q] = r;
                }
                // vector_mean_stdv_mad (src2/auxiliar.cpp:387-430)
                const double stdv = 1.4826 * tpk::mad(s, res, nullptr, base, n, n, &s.sel[2 * kind], tid);
                double v[4] = {0.0, 0.0, 0.0, 0.0}, S[4];
                for (int i = tid; i < n; i += kTpNT) {
                    const double r = res[base + i];
                    if (r < 2.0 * stdv) {
                        v[0] += r;
                        v[1] += 1.0;
                    }
                    v[2] += r;
                }
                tpk::sum4(s, v, S, lane, wave);
                double mean = 0.0;
                if (n) mean = ((int)S[1] >= (int)(0.2 * (double)n)) ? S[0] / S[1] : S[2] / (double)n;
                const double th = prm.inlier_k * stdv;
                v[0] = 0.0;
                for (int i = tid; i < n; i += kTpNT) {
                    if (in[base + i] && fabs(res[base + i] - mean) > th) in[base + i] = 0;
                    v[0] += in[base + i] ? 1.0 : 0.0;
                }
                tpk::sum4(s, v, S, lane, wave);
                if (kind) na_l = (int)S[0];
                else na_p = (int)S[0];
            }
            if (tid == 0)
                for (int k = 0; k < 16; ++k) s.T[k] = s.T0[k];  // the refinement starts from the initial DT (:352)
            __syncthreads();
            if (na_p + na_l >= prm.min_features) {
                run_loop(prm.max_iters_ref, 1);
            } else {  // :360-364
                branch = PLBA_TRACK_FEW_AFTER;
                if (tid == 0)
                    for (int k = 0; k < 16; ++k) s.T[k] = (k % 5 == 0) ? 1.0 : 0.0;
            }
        } else {
            branch = PLBA_TRACK_FIRST_NOT_GOOD;
            if (tid == 0)
                for (int k = 0; k < 16; ++k) s.T[k] = s.T0[k];
            __syncthreads();
            if (MODEL == PLBA_TRACK_ENDPOINTS) run_loop(prm.max_iters_ref, 1);  // :371; the Plücker build does nothing
        }
    }
    __syncthreads();
    if (tid != 0) return;  // (no barrier below)
    // :385-404
    plba_track_out &o = d.out[prob];
    double ev[6];
    pgn::eig6_sorted(s.cov, ev, s.w);
    bool ident = true;
    for (int k = 0; k < 16; ++k) ident = ident && s.T[k] == ((k % 5 == 0) ? 1.0 : 0.0);
    const bool ok = tpg::is_good(ev, err, s.T) && !ident;
    if (ok) {
        double Ti[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, x[6];
        se3_inv34(s.T, Ti);
        se3_log(Ti, x);
        se3_exp(x, o.DT);
        for (int k = 0; k < 36; ++k) o.DT_cov[k] = s.cov[k];
        for (int k = 0; k < 6; ++k) o.DT_cov_eig[k] = ev[k];
        o.err_norm = err;
    } else {
        for (int k = 0; k < 16; ++k) o.DT[k] = (k % 5 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 36; ++k) o.DT_cov[k] = 0.0;
        for (int k = 0; k < 6; ++k) o.DT_cov_eig[k] = 0.0;
        o.err_norm = -1.0;
        if (branch == PLBA_TRACK_OK) branch = PLBA_TRACK_FINAL_NOT_GOOD;
    }
    o.branch = branch;
    o.iters_first = iters[0];
    o.iters_ref = iters[1];
    o.n_inl_pt = na_p;
    o.n_inl_ln = na_l;
    o.pad = 0;
    o.s_p = s_p;
    o.s_l = s_l;
    for (int k = 0; k < 16; ++k) o.DT_solver[k] = s.T[k];
    for (int k = 0; k < 36; ++k) o.H[k] = s.H[k];
}

}  // namespace plba
