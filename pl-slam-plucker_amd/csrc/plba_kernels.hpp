// plba_kernels.hpp — HIP kernels of the LM solve (gfx950, FP64, wave64).
//
// Per LM outer iteration (OptimizationAlgorithmLevenberg::solve):
//   k_linearize        edge-parallel: error, χ², Huber weight, weighted Jacobians
//                      (computeActiveErrors + linearizeOplus + constructQuadraticForm, A5/A6/A9/A10)
//   k_iter_reduce      one launch, two roles: pose-parallel partial sums of Hpp, b_p
//                      (kPoseParts workgroups per pose) and landmark-parallel Hll, b_l,
//                      max|diag| partials
//   k_iter_init        Hpp, b_p from the pose parts, χ²_cur, λ init (τ·max|H_jj|, iteration 0)
// Stage switch (initializeOptimization): folded into the iteration kernels of the first step
// of a stage — k_linearize classifies and activates edges, k_iter_reduce activates
// landmarks, k_iter_init advances the stage (or skips it when nothing is active).
// Per damped trial (TRIAL_GUARD):
//   k_edge_schur       edge-parallel: (Hll+λI) = LLᵀ of its landmark, Z_e = B_e L⁻ᵀ, q_e = Z_e L⁻¹b_l
//   k_rcs_chunk        one wave per chunk of <=128 (e1,e2) triples of one RCS block:
//                      Σ A₁ᵀ(Z₁Z₂ᵀ)A₂ (and Σ A_eᵀq_e on diagonal blocks)
//   k_rcs_finalize     per block entry: Hpp+λI − Σ chunks into the band (or dense) matrix, b_s
//   k_rcs_factor_twisted<BW>  two workgroups: two-sided block-banded LDLᵀ meeting at a
//                      bw-block separator, forward/backward solve (LinearSolverEigen);
//                      k_rcs_factor_band<BW> (one sweep) and the dense k_rcs_factor (bw>20)
//                      are the fallbacks
//                      ... each ending with the pose oplus of the free poses (pose_update_wg)
//   k_lm_solve         landmark-parallel: x_l = L⁻ᵀL⁻¹(b_l − Σ_e B_eᵀA_e x_p), oplus, Σx(λx+b)
//                      partials, then the landmark's edges' χ² at the trial state (robust partials)
//   k_decide           ρ, accept/reject, λ/ν update, optimize() loop control (g2o Levenberg)
//                      (accepting flips Ctrl::cur: the trial buffer becomes the current state)
// After the schedule: k_refresh (level-1 computeError) and k_depth (isDepthPositive).
// All reductions are fixed-order trees: results are bitwise reproducible run to run.
#pragma once

#include "plba_dev.hpp"      // constants, Ctrl, Dev, LmKind, slot views, reductions, hand-offs, guards

namespace plba {

// ---------------------------------------------------------------- linearisation
__global__ __launch_bounds__(kBlock) void k_linearize(Dev d) {
    ITER_GUARD
    __shared__ double sh[kBlock / 64];
    const int e = blockIdx.x * kBlock + threadIdx.x;
    double rc = 0.0;
    const Ctrl *cc = d.ctrl;
    const bool sw = cc->switch_pending;
    const int nxt = cc->stage + 1;
    const int robust = sw ? cc->stage_robust[nxt] : cc->robust;
    double *chi2e = chi2cur(d);  // this iteration's χ² go where the last consumed trial's are
    // A/c/B rows are staged in LDS and written out as contiguous 1-KB pieces per store instruction:
    // written per lane (96/16/64-B rows at a lane stride) every store instruction of a wave touched
    // ~48 cache lines, and the stores of the long line-edge waves were the kernel's tail
    __shared__ __attribute__((aligned(16))) double stA[kBlock * 12], stc[kBlock * 2], stB[kBlock * 8];
    if (e < d.E) {
        double *A = stA + threadIdx.x * 12, *c = stc + threadIdx.x * 2, *B = stB + threadIdx.x * 8;
        if (sw) {
            const double stale = chi2e[e];
            // every χ² buffer starts the stage with the stale values: an edge the new stage leaves
            // inactive keeps its χ² whichever buffer the stage's last trial writes
            for (int b = 0; b < d.nbx; ++b)
                if (d.chi2b[b] != chi2e) d.chi2b[b][e] = stale;
            // stage switch: classify on the stale χ² and the current depth (src/mapHandler.cpp:
            // 6125-6147), then activate the edges of the optimised level
            if (cc->stage_classify[nxt]) {
                bool bad = stale > kChi2Thr;
                if (e < d.Ep) {
                    double Pc[3];
                    point_pc(Tcur(d) + (size_t)d.e_kf[e] * 12, Xcur(d) + (size_t)d.e_lm[e] * 4, Pc);
                    bad = bad || !(Pc[2] > 0.0);
                }
                if (bad) d.e_level[e] = 1;
            }
            d.e_active[e] = d.e_level[e] == cc->stage_level[nxt] ? 1 : 0;
        }
        if (d.e_active[e] && lm_hand_rolled(cc->hlm)) {
            // hand-rolled LM (src/mapHandler.cpp:1909-2103): one scalar residual r = ‖e‖ with
            // Cauchy weight w; row 0 of A/B holds √w·J, c = (√w·r, 0), so Σ AᵀA = Σ w JᵀJ and
            // Σ Aᵀc = Σ w J r = g. Point observations read the current pose (the map pose of
            // fixed KFs and, before the first update, of every KF); line observations always
            // read the map pose T_init (:2010-2012) and the current NDw (the map's on the first
            // linearisation, uploaded into Lpb by plba_hlm_lba).
            const int lm = d.e_lm[e], kf = d.e_kf[e];
            const double *obs = d.e_obs + (size_t)e * 4;
            double r, w, Jp[6], Jl[4];
            double Jl6[6] = {0, 0, 0, 0, 0, 0};
            if (e < d.Ep) {
                hlm_point(Tcur(d) + (size_t)kf * 12, Xcur(d) + (size_t)lm * 4, obs, d.cam, cc->hlm_homog, r, w, Jp, Jl);
            } else if (lm_endpoint_lines(cc->hlm)) {
                // GBA: map pose, endpoints line3D on the first linearisation, then both read from
                // the aliased X.block(6Nkf+3Npt+3·j) (src/mapHandler.cpp:3547-3548)
                // endpoint-line LBA (kLmLbaEndpoints): the same reads (:2453-2456, :2697-2700); its later
                // linearisations hard-code the homogeneous threshold 1e-7 (:2717-2760)
                const int j = d.ln_gidx[lm - d.n_pt];
                const double *XLc = d.XL[cc->cur];
                const bool first = cc->iter == 0;
                const double *P = XLc + (first ? (size_t)j * 6 : (size_t)j * 3);
                const double *Q = XLc + (first ? (size_t)j * 6 + 3 : (size_t)j * 3);
                const double hth = cc->hlm == kLmLbaEndpoints && !first ? 0.0000001 : cc->hlm_homog;
                gba_line(d.T_init + (size_t)kf * 12, P, Q, obs, d.cam, hth, r, w, Jp, Jl6);
            } else {
                const double *Lc = d.Lpb[cc->cur] + (size_t)(lm - d.n_pt) * 8;
                double L[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) L[k] = Lc[k];
                hlm_line(d.T_init + (size_t)kf * 12, L, obs, d.cam, cc->hlm_homog, r, w, Jp, Jl);
            }
            chi2e[e] = r * r;
            rc = r * r * w;
            const double sw = sqrt(w);
            const bool pose_free = d.e_hidx[e] >= 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                A[k] = pose_free ? sw * Jp[k] : 0.0;
                A[6 + k] = 0.0;
            }
            c[0] = sw * r;
            c[1] = 0.0;
            if (e >= d.Ep && lm_endpoint_lines(cc->hlm)) {  // 6-dim landmark row, flat in B
#pragma unroll
                for (int k = 0; k < 6; ++k) B[k] = sw * Jl6[k];
                B[6] = B[7] = 0.0;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    B[k] = sw * Jl[k];
                    B[4 + k] = 0.0;
                }
            }
        } else if (d.e_active[e]) {
            const int lm = d.e_lm[e], kf = d.e_kf[e];
            const double *T = Tcur(d) + (size_t)kf * 12;
            const double *X = Xcur(d) + (size_t)lm * 4;
            const double *obs = d.e_obs + (size_t)e * 4;
            double err[2], Jl[8], Jp[12];
            double delta;
            if (e < d.Ep) {
                double z;
                point_error(T, X, obs, d.cam, err, z);
                point_jac(T, X, d.cam, Jl, Jp);
                // widen 2x3 -> 2x4
                Jl[7] = 0; Jl[6] = Jl[5]; Jl[5] = Jl[4]; Jl[4] = Jl[3]; Jl[3] = 0;
                delta = d.huber_pt;
            } else {
                // changeOrthToPluker of the current state, evaluated once per line (Lpb)
                const double *Lc = d.Lpb[cc->cur] + (size_t)(lm - d.n_pt) * 8;
                double L[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) L[k] = Lc[k];
                line_jac(T, X, L, obs, d.cam, d.corrected, err, Jl, Jp);
                delta = d.huber_ln;
            }
            const double info = d.e_info[e];
            const double chi = err[0] * (info * err[0]) + err[1] * (info * err[1]);
            chi2e[e] = chi;
            double rho0 = chi, rho1 = 1.0;
            if (robust) huber(chi, delta, rho0, rho1);
            rc = rho0;
            const double s = sqrt(rho1 * info);
            const bool pose_free = d.e_hidx[e] >= 0;
#pragma unroll
            for (int k = 0; k < 12; ++k) A[k] = pose_free ? s * Jp[k] : 0.0;
            c[0] = -s * err[0];
            c[1] = -s * err[1];
#pragma unroll
            for (int k = 0; k < 8; ++k) B[k] = s * Jl[k];
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) A[k] = 0.0;
            c[0] = c[1] = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) B[k] = 0.0;
        }
    }
    __syncthreads();
    {
        const int e0 = blockIdx.x * kBlock, n = min(kBlock, d.E - e0);
        auto copy_out = [&](const double *src, double *dst, int cnt) {  // cnt doubles, even
            const double2 *s2 = reinterpret_cast<const double2 *>(src);
            double2 *d2 = reinterpret_cast<double2 *>(dst);
            for (int t = threadIdx.x; t < cnt / 2; t += kBlock) d2[t] = s2[t];
        };
        copy_out(stA, d.A + (size_t)e0 * 12, n * 12);
        copy_out(stc, d.cvec + (size_t)e0 * 2, n * 2);
        copy_out(stB, d.B + (size_t)e0 * 8, n * 8);
    }
    double s = block_sum<kBlock>(rc, sh);
    if (threadIdx.x == 0) d.part_chi2[blockIdx.x] = s;
}

// The iteration's two reductions in ONE launch of 64-thread workgroups (they are independent
// and each alone leaves most of the chip idle):
//   workgroups [0, kPoseParts·nf): pose h, part j sums A_eᵀA_e and A_eᵀc_e over the pose's
//     edges p ≡ 64j + lane (mod 64·kPoseParts) into pose_part[h][j][kPP]; the parts are added in
//     j order by pose_combine (k_iter_init / k_iter_pack) — the same per-lane sets and order
//     as one 256-thread workgroup per pose, so the sums are deterministic;
//   workgroups [kPoseParts·nf, ...): 64 landmarks each, Hll = Σ B_eᵀB_e, b_l = Σ B_eᵀc_e
//     (and, on a stage switch, the landmark activation).
constexpr int kPoseParts = 4;
constexpr int kPoseKU = 4;     // pose-part edges with loads in flight per pass
constexpr int kPP = 28;        // per pose part: 21 (upper Σ AᵀA) + 6 (Σ Aᵀc) + active-edge count
constexpr int kInitNT = 1024;  // k_iter_init / k_iter_pack: one wide workgroup (the pose combine)

// packed lower-triangular index for 4x4 symmetric
__device__ __forceinline__ constexpr int pk(int r, int c) { return r * (r + 1) / 2 + c; }

// returns max|Hpp_jj| of pose h in the workgroup that combined it (folded init), else 0
__device__ __forceinline__ double pose_partial(const Dev &d, int h, int part) {
    double acc[kPP];
#pragma unroll
    for (int k = 0; k < kPP; ++k) acc[k] = 0.0;
    // kU edges per pass with all their loads issued before the arithmetic (the per-thread
    // chains are edge-index -> A/c misses; one edge at a time leaves them serialised)
    constexpr int S = kPoseParts * 64, kU = kPoseKU;
    const int pend = d.pe_off[h + 1];
    for (int p0 = d.pe_off[h] + part * 64 + threadIdx.x; p0 < pend; p0 += kU * S) {
        int ei[kU];
#pragma unroll
        for (int j = 0; j < kU; ++j) ei[j] = p0 + j * S < pend ? d.pe_list[p0 + j * S] : -1;
        double a[kU][12], cv[kU][2];
#pragma unroll
        for (int j = 0; j < kU; ++j) {
            const int e = ei[j] < 0 ? ei[0] : ei[j];  // in-range address; masked below
            const double *A = d.A + (size_t)e * 12;
#pragma unroll
            for (int k = 0; k < 12; ++k) a[j][k] = A[k];
            cv[j][0] = d.cvec[(size_t)e * 2];
            cv[j][1] = d.cvec[(size_t)e * 2 + 1];
        }
#pragma unroll
        for (int j = 0; j < kU; ++j) {
            if (ei[j] < 0) break;
            acc[27] += d.e_active[ei[j]] ? 1.0 : 0.0;
            const double *a0 = a[j], *a1 = a[j] + 6;
            int idx = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int cc = r; cc < 6; ++cc) acc[idx++] += a0[r] * a0[cc] + a1[r] * a1[cc];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[21 + r] += a0[r] * cv[j][0] + a1[r] * cv[j][1];
        }
    }
    {
        // the 28 sums as a reduce-scatter: each butterfly step halves the values a lane carries
        // (~220 instead of ~500 instructions); value k ends in lane 2k. The same pairwise
        // additions as wave_sum (a + b in the same butterfly order), so bitwise the same sums.
        const int lane = threadIdx.x;
        double v[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) v[k] = k < kPP ? acc[k] : 0.0;
#pragma unroll
        for (int n = 16; n >= 1; n >>= 1) {
            const int m = 2 * n;  // lane bit of this step: 32, 16, 8, 4, 2
            const bool hi = (lane & m) != 0;
#pragma unroll
            for (int i = 0; i < n; ++i) {
                const double keep = hi ? v[n + i] : v[i], send = hi ? v[i] : v[n + i];
                v[i] = keep + __shfl_xor(send, m, 64);
            }
        }
        v[0] += __shfl_xor(v[0], 1, 64);
        if ((lane & 1) == 0 && lane / 2 < kPP)
            st_sc1(d.pose_part + ((size_t)h * kPoseParts + part) * kPP + lane / 2, v[0]);  // read by the combine below
    }
    // folded iteration init: the last of the pose's kPoseParts workgroups adds the parts (in part
    // order, as pose_combine does) into Hpp / b_p / active count and publishes max|Hpp_jj|
    // (sharded windows too: the combine then writes this rank's partial Hpp / b_p into the
    // all-reduce source, and k_iter_pack only packs χ² and the landmark maxima)
    if ((d.fold_init || d.sharded) && arrive_last(d.cnt + 2 + d.nblk + h, kPoseParts)) {
        const int k = threadIdx.x;
        double v = 0.0;
        if (k < kPP) {
            const double *src = d.pose_part + (size_t)h * kPoseParts * kPP + k;
            double p[kPoseParts];
#pragma unroll
            for (int j = 0; j < kPoseParts; ++j) p[j] = ld_sc1(src + j * kPP);
            v = p[0];
#pragma unroll
            for (int j = 1; j < kPoseParts; ++j) v += p[j];
            if (k < 21) {
                int r = 0, rem = k;
                while (rem >= 6 - r) { rem -= 6 - r; ++r; }
                const int cc = r + rem;
                d.Hpp_w[(size_t)h * 36 + r * 6 + cc] = v;
                d.Hpp_w[(size_t)h * 36 + cc * 6 + r] = v;
                if (r == cc && d.Hdg_w) d.Hdg_w[(size_t)h * 6 + r] = v;
                if (r != cc) v = 0.0;
            } else if (k < 27) {
                d.bp_w[(size_t)h * 6 + (k - 21)] = v;
                v = 0.0;
            } else {
                d.pact_w[h] = v;
                v = 0.0;
            }
        }
        const double m = wave_max(fabs(v));  // kLmBlock = one wave
        if (threadIdx.x == 0) st_sc1(d.part_max + h, m);
        return m;
    }
    return 0.0;
}

// returns (block max|H_ll diag|, block has an active landmark) through mx_out / any_out
__device__ __forceinline__ void landmark_reduce(const Dev &d, int lb, double &mx_out, int &any_out) {
    __shared__ double sh[kLmBlock / 64];
    const int l = lb * kLmBlock + threadIdx.x;
    const bool sw = d.ctrl->switch_pending;
    double mx = 0.0;
    bool any = false;
    if (l < d.n_lm) {
        if (sw) {  // a landmark is active iff it has an active edge
            bool act = false;
            for (int e = d.lm_off[l]; e < d.lm_off[l + 1]; ++e) act = act || d.e_active[e];
            d.lm_active[l] = act ? 1 : 0;
        }
        any = d.lm_active[l] != 0;
        if (l >= d.n_pt && lm_endpoint_lines(d.ctrl->hlm)) {  // GBA / LBA endpoint line: 6x6 block (flat 6-vector rows in B)
            double H6[21], b6[6];
#pragma unroll
            for (int k = 0; k < 21; ++k) H6[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) b6[k] = 0.0;
            for (int e = d.lm_off[l]; e < d.lm_off[l + 1]; ++e) {
                double bb[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) bb[k] = d.B[(size_t)e * 8 + k];
                const double c0 = d.cvec[(size_t)e * 2];
#pragma unroll
                for (int r = 0; r < 6; ++r) {
#pragma unroll
                    for (int cc = 0; cc <= r; ++cc) H6[pk(r, cc)] += bb[r] * bb[cc];
                    b6[r] += bb[r] * c0;
                }
            }
            const int li = l - d.n_pt;
#pragma unroll
            for (int k = 0; k < 21; ++k) d.Hl6[(size_t)li * 21 + k] = H6[k];
#pragma unroll
            for (int k = 0; k < 6; ++k) d.bl6[(size_t)li * 6 + k] = b6[k];
#pragma unroll
            for (int k = 0; k < 6; ++k) mx = fmax(mx, fabs(H6[pk(k, k)]));
        } else {
        double H[10], b[4];
#pragma unroll
        for (int k = 0; k < 10; ++k) H[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = 0.0;
        const int e1 = d.lm_off[l + 1];
        for (int e0 = d.lm_off[l]; e0 < e1; e0 += 2) {  // two edges' loads in flight per pass
            double bb[2][8], cc2[2][2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int e = e0 + j < e1 ? e0 + j : e0;
#pragma unroll
                for (int k = 0; k < 8; ++k) bb[j][k] = d.B[(size_t)e * 8 + k];
                cc2[j][0] = d.cvec[(size_t)e * 2];
                cc2[j][1] = d.cvec[(size_t)e * 2 + 1];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (e0 + j >= e1) break;
                const double *b0 = bb[j], *b1 = bb[j] + 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int cc = 0; cc <= r; ++cc) H[pk(r, cc)] += b0[r] * b0[cc] + b1[r] * b1[cc];
                    b[r] += b0[r] * cc2[j][0] + b1[r] * cc2[j][1];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) d.Hll[(size_t)l * 10 + k] = H[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) d.bl[(size_t)l * 4 + k] = b[k];
        mx = fmax(fmax(fabs(H[pk(0, 0)]), fabs(H[pk(1, 1)])), fmax(fabs(H[pk(2, 2)]), fabs(H[pk(3, 3)])));
        }
    }
    double m = block_max<kLmBlock>(mx, sh);
    const int anyb = __syncthreads_or(any ? 1 : 0);
    if (threadIdx.x == 0) {
        st_sc1(d.part_max + d.nf + lb, m);
        __hip_atomic_store(d.part_any + lb, anyb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    mx_out = m;
    any_out = anyb;
}


// Hpp, b_p from the pose parts (added in part order); returns this thread's max |Hpp_jj|
template <int NT, bool SC1 = false>
__device__ __forceinline__ double pose_combine(const Dev &d, double *H, double *bp) {
    double m = 0.0;
    for (int i = threadIdx.x; i < d.nf * kPP; i += NT) {
        const int h = i / kPP, k = i % kPP;
        const double *src = d.pose_part + (size_t)h * kPoseParts * kPP + k;
        double v = SC1 ? ld_sc1(src) : src[0];
#pragma unroll
        for (int j = 1; j < kPoseParts; ++j) v += SC1 ? ld_sc1(src + j * kPP) : src[j * kPP];
        if (k < 21) {
            int r = 0, rem = k;
            while (rem >= 6 - r) { rem -= 6 - r; ++r; }
            const int cc = r + rem;
            H[(size_t)h * 36 + r * 6 + cc] = v;
            H[(size_t)h * 36 + cc * 6 + r] = v;
            if (r == cc) m = fmax(m, fabs(v));
        } else if (k < 27) {
            bp[(size_t)h * 6 + (k - 21)] = v;
        } else {
            d.pact_w[h] = v;
        }
    }
    return m;
}

// sharded windows: this rank's χ² and landmark max|diag| into the all-reduced iteration array
// (Hpp and b_p already sit in it). The rank's max goes to its own slot: the sum over ranks of
// one-hot slots is the list of maxima, reduced with max by k_iter_init.
__global__ __launch_bounds__(kInitNT) void k_iter_pack(Dev d) {
    ITER_GUARD
    __shared__ double sh[kInitNT / 64];
    // (Hpp / b_p / active counts: combined per pose by the last of its k_iter_reduce parts)
    double s = 0.0;
    for (int i = threadIdx.x; i < d.n_lin_blocks; i += kInitNT) s += d.part_chi2[i];
    const double chi = block_sum<kInitNT>(s, sh);
    double m = 0.0;
    for (int i = threadIdx.x; i < d.n_lm_blocks; i += kInitNT) m = fmax(m, d.part_max[d.nf + i]);
    const double mx = block_max<kInitNT>(m, sh);
    int any = 0;
    for (int i = threadIdx.x; i < d.n_lm_blocks; i += kInitNT) any |= d.part_any[i];
    any = __syncthreads_or(any);
    double *o = d.red_iter_loc + (size_t)d.nf * 13;  // (sharded layout: diag | b_p | active | scalars)
    if (threadIdx.x == 0) {
        o[0] = chi;
        o[1] = any ? 1.0 : 0.0;
    }
    for (int r = threadIdx.x; r < d.nranks; r += kInitNT) o[2 + r] = r == d.rank ? mx : 0.0;
}

// the iteration init (k_iter_init's work): run as its own launch (sharded windows, windows with
// nothing to reduce) or as the tail of the last-arriving k_iter_reduce workgroup (SC1: the
// partials of that launch are read write-through)
__device__ __forceinline__ void iter_init_ctrl(const Dev &d, double chi, double mx, bool any);
template <int NT>
__device__ __forceinline__ void iter_init_body(const Dev &d, double *sh) {
    double chi, mx;
    bool any;
    if (d.sharded) {  // totals from the all-reduced iteration array
        const double *o = d.red_iter + (size_t)d.nf * 13;
        double m = 0.0;
        for (int i = threadIdx.x; i < d.nf * 6; i += NT) m = fmax(m, fabs(d.Hdg[i]));
        for (int r = threadIdx.x; r < d.nranks; r += NT) m = fmax(m, o[2 + r]);
        mx = block_max<NT>(m, sh);
        chi = o[0];
        any = o[1] != 0.0;
    } else {
        double m = pose_combine<NT>(d, d.Hpp_w, d.bp_w);
        double s = 0.0;
        for (int i = threadIdx.x; i < d.n_lin_blocks; i += NT) s += d.part_chi2[i];
        chi = block_sum<NT>(s, sh);
        for (int i = threadIdx.x; i < d.n_lm_blocks; i += NT) m = fmax(m, d.part_max[d.nf + i]);
        mx = block_max<NT>(m, sh);
        int a = 0;
        for (int i = threadIdx.x; i < d.n_lm_blocks; i += NT) a |= d.part_any[i];
        any = __syncthreads_or(a) != 0;
    }
    if (threadIdx.x == 0) iter_init_ctrl(d, chi, mx, any);
}
// the control part of the iteration init (one thread): stage switch, λ init / hand-rolled stops
__device__ __forceinline__ void iter_init_ctrl(const Dev &d, double chi, double mx, bool any) {
    {
        Ctrl *c = d.ctrl;
        if (c->switch_pending) {  // initializeOptimization(level) of the next stage
            c->switch_pending = 0;
            c->stage += 1;
            c->iter = 0;
            c->robust = c->stage_robust[c->stage];
            c->level = c->stage_level[c->stage];
            if (!any) {  // _ivMap empty: optimize() returns -1 without iterating
                c->iters_done[c->stage] = -1;
                c->chi2_final[c->stage] = 0.0;
                c->need_iter = 0;
                if (c->stage + 1 < c->n_stages) c->switch_pending = 1;
                else c->all_done = 1;
                return;
            }
        }
        if (lm_hand_rolled(c->hlm)) {  // src/mapHandler.cpp:1849-1858 (first linearisation), :2108-2112 (later)
            // reference: / (Npt_obs + Nls_obs) == / 0; the endpoint-line LBA divides its later
            // linearisations by the landmark counts Npt + Nls instead (src/mapHandler.cpp:2796)
            const double err = chi / (c->hlm == kLmLbaEndpoints && c->iter > 0 ? c->hlm_nobs2 : c->hlm_nobs);
            c->hlm_lin += 1;
            if (c->iter == 0) {
                c->maxdiag = mx;
                // GBA keeps Hmax in an int (src/mapHandler.cpp:3386): truncated toward zero; the
                // endpoint-line LBA in a double (:2555)
                c->lambda = c->hlm_lambda0 * (c->hlm == kLmGba ? (double)(long long)mx : mx);
            } else if (fabs(err - c->err_prev) < c->hlm_minchg || err < c->hlm_minerr) {
                if (c->ntrace < kTraceCap)
                    d.trace[c->ntrace++] = plba_iter_trace{c->stage, c->iter, 0, 3, err, err, c->lambda, c->lambda};
                c->currentChi = err;
                c->chi2_final[c->stage] = err;
                c->need_iter = 0;
                c->all_done = 1;
                return;
            }
            c->currentChi = err;
            c->chi2_start = err;
            c->lambda_start = c->lambda;
            c->accept = 0;
            c->need_iter = 0;
            return;
        }
        // currentChi: at iteration 0 the χ² of the linearisation; later iterations start at the
        // state of the trial just accepted, whose χ² (the same edges at the same state, summed in
        // another order) is already currentChi — kept, so the folded init can skip its global
        // reduction after the first iteration (k_iter_reduce) and every mode agrees
        if (c->iter == 0) {  // computeLambdaInit: τ·max|H_jj|, ν = 2
            c->currentChi = chi;
            c->maxdiag = mx;
            c->lambda = d.tau * mx;
            c->ni = 2.0;
        }
        c->chi2_start = c->currentChi;
        c->lambda_start = c->lambda;
        c->qmax = 0;
        c->accept = 0;
        c->rho = 0.0;
        c->broke = 0;
        c->need_iter = 0;
    }
}
__global__ __launch_bounds__(kInitNT) void k_iter_init(Dev d) {
    ITER_GUARD
    __shared__ double sh[kInitNT / 64];
    iter_init_body<kInitNT>(d, sh);
}

constexpr int kRedGrp = 256;  // k_iter_reduce workgroups per first-level group of the folded init
// an iteration after the first of its stage (g2o Levenberg, not the hand-rolled LM, unsharded,
// folded init): k_decide has already done the iteration init (decide_body), so k_iter_reduce only
// forms Hpp / b_p / Hll / b_l. Uniform: read before any workgroup can change the control block.
__device__ __forceinline__ bool iter_init_fast(const Dev &d) {
    const Ctrl *c = d.ctrl;
    return d.fold_init && !d.sharded && !lm_hand_rolled(c->hlm) && !c->switch_pending && c->iter > 0;
}
__global__ __launch_bounds__(kLmBlock) void k_iter_reduce(Dev d) {
    ITER_GUARD
    __shared__ double sh_init[kLmBlock / 64];
    const int b = blockIdx.x, np = kPoseParts * d.nf;
    const int G = (int)gridDim.x, lane = threadIdx.x;
    // folded init: this workgroup's slice of k_linearize's χ² partials, loaded before the main
    // work so the round trip overlaps it
    double sc = 0.0;
    if (d.fold_init && !iter_init_fast(d)) {
        const int lo = (int)((long long)b * d.n_lin_blocks / G), hi = (int)((long long)(b + 1) * d.n_lin_blocks / G);
        for (int i = lo + lane; i < hi; i += kLmBlock) sc += d.part_chi2[i];
    }
    double wmax = 0.0;
    int wany = 0;
    if (b < np) wmax = pose_partial(d, b / kPoseParts, b % kPoseParts);  // workgroup-uniform branch
    else landmark_reduce(d, b - np, wmax, wany);
    if (!d.fold_init) return;
    // after the first iteration of a stage the init needs none of the global terms (λ is set, the
    // χ² is the accepted trial's, no activity change): k_decide already started the iteration
    if (iter_init_fast(d)) return;
    // folded iteration init (k_iter_init's work; the pose combine already ran per pose), reduced
    // in two levels so no single workgroup reads every partial: each workgroup adds a slice of
    // k_linearize's χ² partials to its own (max, any), the last of each group of kRedGrp
    // workgroups combines the group, the last group runs the control step. Fixed order.
    {
        sc = wave_sum(sc);  // kLmBlock = one wave
        if (lane == 0) {
            st_sc1(d.wg_red + 3 * (size_t)b, sc);
            st_sc1(d.wg_red + 3 * (size_t)b + 1, wmax);
            st_sc1(d.wg_red + 3 * (size_t)b + 2, wany ? 1.0 : 0.0);
        }
    }
    constexpr int U = kRedGrp / kLmBlock;
    const int g = b / kRedGrp, gn = min(kRedGrp, G - kRedGrp * g), ng = (G + kRedGrp - 1) / kRedGrp;
    if (!arrive_last(d.cnt + 2 + d.nblk + d.nf + g, gn)) return;
    {
        double cv[U], mv[U], av[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {  // lane holds members lane·U .. lane·U+U-1, all loads in flight
            const int k = lane * U + u;
            const double *w = d.wg_red + 3 * (size_t)(kRedGrp * g + min(k, gn - 1));
            cv[u] = ld_sc1(w);
            mv[u] = ld_sc1(w + 1);
            av[u] = ld_sc1(w + 2);
        }
        double c = 0.0, m = 0.0, a = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (lane * U + u < gn) {
                c += cv[u];
                m = fmax(m, mv[u]);
                a = fmax(a, av[u]);
            }
        c = wave_sum(c);
        m = wave_max(m);
        a = wave_max(a);
        if (lane == 0) {
            st_sc1(d.grp_red + 3 * (size_t)g, c);
            st_sc1(d.grp_red + 3 * (size_t)g + 1, m);
            st_sc1(d.grp_red + 3 * (size_t)g + 2, a);
        }
    }
    if (!arrive_last(d.cnt + 1, ng)) return;
    double c = 0.0, m = 0.0, a = 0.0;
    for (int g0 = 0; g0 < ng; g0 += 64) {  // groups in index order, 64 at a time
        double cg = 0.0, mg = 0.0, ag = 0.0;
        if (g0 + lane < ng) {
            const double *w = d.grp_red + 3 * (size_t)(g0 + lane);
            cg = ld_sc1(w);
            mg = ld_sc1(w + 1);
            ag = ld_sc1(w + 2);
        }
        c += wave_sum(cg);
        m = fmax(m, wave_max(mg));
        a = fmax(a, wave_max(ag));
    }
    (void)sh_init;
    if (lane == 0) iter_init_ctrl(d, c, m, a != 0.0);
}

}  // namespace plba

#include "plba_rcs.hpp"      // k_rcs_chunk(_h), k_rcs_finalize, pose_update_wg
#include "plba_dense.hpp"    // factorisations: scalar dense (k_rcs_factor) and MFMA dense,
#include "plba_band.hpp"     //   LDS-window band (k_rcs_factor_band / _twisted),
#include "plba_band_cl.hpp"  //   column lane,
#include "plba_bcr.hpp"      //   block cyclic reduction,
#include "plba_pgo.hpp"      //   and the pose graph on the dense path

namespace plba {

// ---------------------------------------------------------------- update + trial evaluation
// stand-alone pose update (windows without free poses: no factorisation kernel to fuse into)
__global__ __launch_bounds__(kBlock) void k_pose_update(Dev d0) {
    TRIAL_SLOT(0)
    if (blockIdx.x == 0) pose_update_wg<kBlock>(d, false);
}

// ---------------------------------------------------------------- edge-parallel trial path
// per landmark: (Hll + λI) = L Lᵀ, g = L⁻¹ b_l (packed lower; recomputed where needed — 4x4,
// cheaper than a kernel boundary)
// Signed form (the hand-rolled LM, `sgn`): (Hll + λ·diag) = M S Mᵀ with S = diag(±1), as an
// unpivoted LDLᵀ tolerates a non-positive pivot (the reference solves the whole system with
// SimplicialLDLT, src/mapHandler.cpp:1861-1865; a rank-deficient landmark block under λ·diag ≈
// 1e-24·H meets one). Every sign is exactly 1 for a positive definite block, and the products
// are grouped so that the result is then bitwise the plain Cholesky's.
__device__ __forceinline__ void lm_chol(const Dev &d, int l, double lam, bool mul, double (&L)[10], double (&g)[4],
                                        double (&S)[4], bool sgn = false) {
    const int DIM = is_point_lm(d, l) ? 3 : 4;
    double H[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) { H[k] = d.Hll[(size_t)l * 10 + k]; L[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { g[k] = 0.0; S[k] = 1.0; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < DIM) {
            double sj = H[pk(j, j)] + (mul ? lam * H[pk(j, j)] : lam);
#pragma unroll
            for (int p = 0; p < j; ++p) sj -= (L[pk(j, p)] * S[p]) * L[pk(j, p)];
            const double sg = (sgn && sj < 0.0) ? -1.0 : 1.0;
            S[j] = sg;
            const double djj = 1.0 / sqrt(sg * sj);  // reciprocal diagonal: every use divides by it
            L[pk(j, j)] = djj;
#pragma unroll
            for (int i = j + 1; i < 4; ++i) {
                if (i < DIM) {
                    double t = H[pk(i, j)];
#pragma unroll
                    for (int p = 0; p < j; ++p) t -= L[pk(i, p)] * (L[pk(j, p)] * S[p]);
                    L[pk(i, j)] = (t * djj) * sg;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < DIM) {
            double t = d.bl[(size_t)l * 4 + i];
#pragma unroll
            for (int p = 0; p < i; ++p) t -= L[pk(i, p)] * g[p];
            g[i] = t * L[pk(i, i)];
        }
    }
}
// per edge: Z_e = B_e L⁻ᵀ (rows solved with L), q_e = Z_e g. The Z / q rows are staged in LDS and
// written out as contiguous pieces (per-lane 64-B / 16-B rows made every store instruction touch
// ~32 cache lines; see k_linearize)
__device__ __forceinline__ void edge_schur_body(const Dev &d, int e, double *Z, double *qe) {
    const int l = d.e_lm[e];
    if (e >= d.Ep && lm_endpoint_lines(d.ctrl->hlm)) {  // GBA / LBA endpoint line: 6x6 (Hl6 + λ·diag) = L Lᵀ, Z_e = L⁻¹ b_e, q_e = Z_e·L⁻¹ b_l
        const double lam = d.lam;
        const int li = l - d.n_pt;
        double H[21], L6[21], g6[6], bb[6], z[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) { H[k] = d.Hl6[(size_t)li * 21 + k]; L6[k] = 0.0; }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double sj = H[pk(j, j)] + lam * H[pk(j, j)];
#pragma unroll
            for (int p = 0; p < j; ++p) sj -= L6[pk(j, p)] * L6[pk(j, p)];
            const double djj = sqrt(sj);
            L6[pk(j, j)] = djj;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double t = H[pk(i, j)];
#pragma unroll
                for (int p = 0; p < j; ++p) t -= L6[pk(i, p)] * L6[pk(j, p)];
                L6[pk(i, j)] = t / djj;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) bb[k] = d.B[(size_t)e * 8 + k];
        double q0 = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double t = bb[i], tg = d.bl6[(size_t)li * 6 + i];
#pragma unroll
            for (int p = 0; p < i; ++p) {
                t -= L6[pk(i, p)] * z[p];
                tg -= L6[pk(i, p)] * g6[p];
            }
            z[i] = t / L6[pk(i, i)];
            g6[i] = tg / L6[pk(i, i)];
            q0 += z[i] * g6[i];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) Z[k] = z[k];
        Z[6] = Z[7] = 0.0;
        qe[0] = q0;
        qe[1] = 0.0;
        return;
    }
    const int DIM = e < d.Ep ? 3 : 4;
    const bool sgn = lm_signed_ldlt(d.ctrl->hlm);
    double L[10], g[4], B[8], S[4];
    lm_chol(d, l, d.lam, lm_hand_rolled(d.ctrl->hlm), L, g, S, sgn);
#pragma unroll
    for (int k = 0; k < 8; ++k) B[k] = d.B[(size_t)e * 8 + k];
    double z[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < DIM) {
                double t = B[r * 4 + i];
#pragma unroll
                for (int p = 0; p < i; ++p) t -= L[pk(i, p)] * z[r][p];
                z[r][i] = t * L[pk(i, i)];
            }
        }
    double q0 = 0, q1 = 0;
    if (sgn) {  // hand-rolled LM (one live row): row 1 carries S·z_0, the assembly takes z_1·(S z_2)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Z[i] = z[0][i];
            Z[4 + i] = z[0][i] * S[i];
            q0 += (z[0][i] * S[i]) * g[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Z[i] = z[0][i];
            Z[4 + i] = z[1][i];
            q0 += z[0][i] * g[i];
            q1 += z[1][i] * g[i];
        }
    }
    qe[0] = q0;
    qe[1] = q1;
}
__global__ __launch_bounds__(kBlock) void k_edge_schur(Dev d0) {
    TRIAL_SLOT(blockIdx.y)
    const int e = blockIdx.x * kBlock + threadIdx.x;
    __shared__ __attribute__((aligned(16))) double stZ[kBlock * 8], stq[kBlock * 2];
    if (e < d.E) edge_schur_body(d, e, stZ + threadIdx.x * 8, stq + threadIdx.x * 2);
    __syncthreads();
    const int e0 = blockIdx.x * kBlock, n = min(kBlock, d.E - e0);
    {
        const double2 *s2 = reinterpret_cast<const double2 *>(stZ);
        double2 *d2 = reinterpret_cast<double2 *>(d.Z + (size_t)e0 * 8);
        for (int t = threadIdx.x; t < n * 4; t += kBlock) d2[t] = s2[t];
    }
    {
        const double2 *s2 = reinterpret_cast<const double2 *>(stq);
        double2 *d2 = reinterpret_cast<double2 *>(d.q + (size_t)e0 * 2);
        for (int t = threadIdx.x; t < n; t += kBlock) d2[t] = s2[t];
    }
}
// per landmark: x_l = L⁻ᵀ L⁻¹ (b_l - Σ u_e), oplus into the trial state, scale partial
// quad (4-lane) DPP exchanges: xor 1 = quad_perm [1,0,3,2], xor 2 = quad_perm [2,3,0,1]
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// sum over the 4 lanes of a quad, identical in all four (a+b == b+a bitwise)
__device__ __forceinline__ double quad_sum(double v) {
    v += dpp_f64<0xB1>(v);
    return v + dpp_f64<0x4E>(v);
}

// v[q] for a lane-dependent q without dynamic register indexing (which spills the array to
// scratch)
__device__ __forceinline__ double sel4(const double (&v)[4], int q) {
    // a select chain is turned back into an indexed scratch load by the compiler: blend instead
    const double m0 = q == 0 ? 1.0 : 0.0, m1 = q == 1 ? 1.0 : 0.0, m2 = q == 2 ? 1.0 : 0.0, m3 = q == 3 ? 1.0 : 0.0;
    return fma(v[3], m3, fma(v[2], m2, fma(v[1], m1, v[0] * m0)));
}

// value of quad lane Q in every lane of the quad (DPP quad_perm [Q,Q,Q,Q])
template <int Q>
__device__ __forceinline__ double quad_bcast(double v) {
    return dpp_f64<Q | (Q << 2) | (Q << 4) | (Q << 6)>(v);
}

// VertexLMLineOrth::oplusImpl (g2o_types/g2o_types.h:72-130) followed by changeOrthToPluker
// (g2o_types.h:367-387) for one line, with the transcendentals spread over the landmark's quad:
// lane q evaluates sincos of θ_q and δθ_q (θ_3 = φ), the quad exchanges them by DPP, every lane
// forms U' = R_xyz(θ)·Rx(δθ1)·Ry(δθ2)·Rz(δθ3) and W10 redundantly, lane q takes angle q of the
// result with the reference's own function (atan2 / asin / atan2 / asin) and its sincos, and the
// quad exchanges those to rebuild the Plücker vector from the new angles exactly as the
// reference does: 3 sincos + 1 inverse per lane instead of 28 calls, same formulas.
// Returns angle q of the new state. All four lanes of the quad must be active.
__device__ __forceinline__ double orth_oplus_quad(const double (&D)[4], const double (&dD)[4], int q, double (&Lp)[6]) {
    const double a = sel4(D, q), b = sel4(dD, q);
    double sa, ca, sb, cb;
    sincos(a, &sa, &ca);
    sincos(b, &sb, &cb);
    const double s1 = quad_bcast<0>(sa), c1 = quad_bcast<0>(ca), s2 = quad_bcast<1>(sa), c2 = quad_bcast<1>(ca);
    const double s3 = quad_bcast<2>(sa), c3 = quad_bcast<2>(ca), w2 = quad_bcast<3>(sa), w1 = quad_bcast<3>(ca);
    const double sx = quad_bcast<0>(sb), cx = quad_bcast<0>(cb), sy = quad_bcast<1>(sb), cy = quad_bcast<1>(cb);
    const double sz = quad_bcast<2>(sb), cz = quad_bcast<2>(cb), sp = quad_bcast<3>(sb), cp = quad_bcast<3>(cb);
    const double R[9] = {c2 * c3, s1 * s2 * c3 - c1 * s3, c1 * s2 * c3 + s1 * s3,
                         c2 * s3, s1 * s2 * s3 + c1 * c3, c1 * s2 * s3 - s1 * c3,
                         -s2,     s1 * c2,                c1 * c2};
    const double Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx};
    const double Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy};
    const double Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
    double T1[9], T2[9], Rn[9];
    mat3mul(R, Rx, T1);
    mat3mul(T1, Ry, T2);
    mat3mul(T2, Rz, Rn);
    const double W10 = w2 * cp + w1 * sp;
    double o;
    if (q & 1) o = asin(q == 1 ? -Rn[6] : W10);
    else o = q == 0 ? atan2(Rn[7], Rn[8]) : atan2(Rn[3], Rn[0]);
    double so, co;
    sincos(o, &so, &co);
    const double t1 = quad_bcast<0>(so), u1 = quad_bcast<0>(co), t2 = quad_bcast<1>(so), u2 = quad_bcast<1>(co);
    const double t3 = quad_bcast<2>(so), u3 = quad_bcast<2>(co), v2 = quad_bcast<3>(so), v1 = quad_bcast<3>(co);
    // rot_xyz(new angles), columns 0 and 1 (plba_math.hpp), scaled by cos φ' / sin φ'
    Lp[0] = v1 * (u2 * u3); Lp[1] = v1 * (u2 * t3); Lp[2] = v1 * (-t2);
    Lp[3] = v2 * (t1 * t2 * u3 - u1 * t3); Lp[4] = v2 * (t1 * t2 * t3 + u1 * u3); Lp[5] = v2 * (t1 * u2);
    return o;
}

// kLmLanes lanes per landmark: lane q walks edges q, q+4, ... of the landmark's CSR range for
// the back-substitution sum, the quad adds the partials (DPP, fixed order), and every lane of
// the quad then solves the 3x3/4x4 system redundantly; lane q writes component q.
constexpr int kLmLanes = 4;
constexpr int kLmsNT = 256;  // k_lm_solve workgroup: 64 landmarks
// Edge slots held in registers per lane (lane q: edges q, q+4, ... up to kLmSlots of them);
// longer tracks fall back to a loop for the remainder. Every load of the kernel that does not
// depend on another load is issued up front, so a landmark costs two dependent global round
// trips (CSR offsets -> edge records, then x_p / trial poses) instead of one per phase.
// (one slot: 2 → 1 cut the kernel's registers enough for 3 waves per SIMD; C5 94.7 → 89 µs,
// C3 unchanged; the edges of a lane are visited in the same order either way)
constexpr int kLmSlots = 1;  // (the slot arrays stay: written out for one slot the kernel allocates registers differently)
struct LmEdge {
    int e, h, kf;
    bool act;
    double info, obs[4], A[12], B[8];
};
__device__ __forceinline__ void lm_load_edge(const Dev &d, int e, LmEdge &s) {
    s.e = e;
    s.h = d.e_hidx[e];
    s.kf = d.e_kf[e];
    s.act = d.e_active[e] != 0;
    s.info = d.e_info[e];
#pragma unroll
    for (int k = 0; k < 4; ++k) s.obs[k] = d.e_obs[(size_t)e * 4 + k];
#pragma unroll
    for (int k = 0; k < 12; ++k) s.A[k] = d.A[(size_t)e * 12 + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) s.B[k] = d.B[(size_t)e * 8 + k];
}
// u += B_eᵀ (A_e x_p) for an edge of a free pose; a GBA line's 6-entry row (flat in B, A's second
// row zero) also feeds u45 (components 4, 5)
template <bool GBA = false>
__device__ __forceinline__ void lm_hpl_x(const LmEdge &s, const double (&x)[6], double (&u)[4], double (&u45)[2]) {
    double ax0 = 0, ax1 = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        ax0 += s.A[k] * x[k];
        ax1 += s.A[6 + k] * x[k];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] += s.B[i] * ax0 + s.B[4 + i] * ax1;
    if (GBA) {
        u45[0] += s.B[4] * ax0;
        u45[1] += s.B[5] * ax0;
    }
}
// robust χ² of one active edge at the trial state (computeActiveErrors)
__device__ __forceinline__ double lm_eval(const Dev &d, const LmEdge &s, const double *T, bool pt, const double (&X)[4],
                                          const double (&Lp)[6], bool robust, double delta) {
    double err[2];
    if (pt) {
        double z;
        point_error(T, X, s.obs, d.cam, err, z);
    } else {
        line_error(T, Lp, s.obs, d.cam, err);
    }
    const double c2 = err[0] * (s.info * err[0]) + err[1] * (s.info * err[1]);
    d.chi2_last[s.e] = c2;
    double rho0 = c2, rho1;
    if (robust) huber(c2, delta, rho0, rho1);
    return rho0;
}

// OptimizationAlgorithmLevenberg trial decision + optimize() loop control.
// Runs as its own launch (sharded windows, windows without landmarks) or as the tail of the last
// k_lm_solve workgroup; the landmark partials are read with sc1 loads in both cases.
// Speculative steps: the W = Ctrl::spec_w trial slots evaluated λ_0 = λ, λ_1 = λ·ν, ... of the
// same linearisation from the same state; they are consumed in slot order exactly as g2o's loop
// would have met them (slot s is only reached when slot s-1 was rejected and the loop goes on,
// and then λ, ν here equal the λ_s, ν_s slot s used, bit for bit), and the slots after an
// accepted or iteration-ending trial are discarded. A failed solve (zero pivot) uses the last
// successful solve's x; a slot whose solve failed after an earlier slot of the same step had
// succeeded saw the wrong "last" x, so it is not consumed: the next step evaluates it again,
// alone (one slot: no concurrent writer of the buffers it reads).
constexpr int kSpecOff = 0, kSpecAlways = 1, kSpecAfterReject = 2, kSpecSticky = 3;
template <int NT>
__device__ __forceinline__ void decide_body(const Dev &d, double *sh) {
    const int W = d.ctrl->spec_w;  // trial slots this step evaluated (uniform)
    double tch[kMaxSpec], scl[kMaxSpec];
#pragma unroll
    for (int s = 0; s < kMaxSpec; ++s) {
        tch[s] = scl[s] = 0.0;
        if (s >= W) continue;
        const double *plm = d.part_lm + (size_t)s * sl_lms(d), *plms = d.part_lms + (size_t)s * sl_lms(d);
        const double *pps = d.part_ps + (size_t)s * d.n_ps;
        double a = 0.0, b = 0.0;
        if (!d.sharded) {  // 8 loads of each array in flight per thread; summed in index order
            constexpr int U = 8;
            for (int i0 = threadIdx.x; i0 < d.n_lms_blocks; i0 += NT * U) {
                double va[U], vb[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = i0 + u * NT;
                    const bool ok = i < d.n_lms_blocks;
                    va[u] = ok ? ld_sc1(plm + i) : 0.0;
                    vb[u] = ok ? ld_sc1(plms + i) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    a += va[u];
                    b += vb[u];
                }
            }
        }
        for (int i = threadIdx.x; i < d.n_ps; i += NT) b += pps[i];  // poses: replicated
        tch[s] = block_sum<NT>(a, sh);
        scl[s] = block_sum<NT>(b, sh);
    }
    if (d.sharded) {  // landmark terms summed over ranks (one slot)
        tch[0] = d.red_dec[0];
        scl[0] += d.red_dec[1];
    }
    if (threadIdx.x != 0) return;
    Ctrl *c = d.ctrl;
    c->steps += 1;
    if (lm_hand_rolled(c->hlm)) {  // src/mapHandler.cpp:1867-1895 (first step), :2121-2156 — one slot
        const double lam0 = c->lambda;
        const bool first = c->iter == 0;
        int result = 0;
        c->hlm_solves += 1;
        // sharded: the landmark pivots are checked on the rank that owns the landmark, so the
        // decision uses the failures summed over the ranks (k_decide_pack), the same on every rank
        const bool ok = d.sharded ? d.red_dec[2] == 0.0
                                  : __hip_atomic_load(&c->solve_ok[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        const double dx2 = ok ? scl[0] : 0.0;  // a failed solve leaves DX = 0 (|DX| < minchg stops)
        c->dx2 = dx2;
        bool apply;
        if (first) {
            apply = true;
        } else if (c->currentChi > c->err_prev) {
            c->lambda /= c->hlm_k;
            apply = false;
            result = 1;
        } else {
            c->lambda *= c->hlm_k;
            apply = true;
        }
        if (ok) c->last_ok = (c->last_ok + 1) % d.nbx;
        apply = apply && ok;  // (an LDLᵀ breakdown leaves X unchanged)
        if (apply) {
            c->cur = (c->cur + 1) % d.nbs;
            c->hlm_acc += 1;
        }
        if (c->ntrace < kTraceCap)
            d.trace[c->ntrace++] = plba_iter_trace{c->stage, c->iter, 1, result, c->currentChi, c->currentChi, lam0,
                                                   c->lambda};
        c->iters_done[c->stage] += 1;
        c->iter += 1;
        const bool small = !first && sqrt(dx2) < c->hlm_minchg;
        c->err_prev = c->currentChi;
        if (small || c->iter >= c->max_iters[c->stage]) {
            c->chi2_final[c->stage] = c->currentChi;
            c->all_done = 1;
        } else {
            c->need_iter = 1;
        }
        c->spec_w = 1;
        return;
    }
    const int cur0 = c->cur, lo0 = c->last_ok, ch0 = c->chi_src;
    bool any_ok = false, hold = false, trials_go_on = false, done = false;
    c->need_iter = 0;  // (iter_init_ctrl's reset when k_iter_reduce took the fast path)
#pragma unroll
    for (int s = 0; s < kMaxSpec; ++s) {
        if (done || s >= W) continue;
        const bool ok = c->solve_ok[s] != 0;
        if (!ok && any_ok) {  // evaluated with the wrong "last successful" x: evaluate again alone
            hold = true;
            done = true;
            continue;
        }
        c->chi_src = (ch0 + 1 + s) % d.nbx;  // the edges now hold this trial's χ² (stale if rejected)
        if (ok) {
            c->last_ok = (lo0 + 1 + s) % d.nbx;
            any_ok = true;
        }
        double tempChi = tch[s];
        if (!ok) tempChi = 1.7976931348623157e308;
        const double scale = scl[s] + 1e-3;
        const double rho = (c->currentChi - tempChi) / scale;
        c->tempChi = tempChi;
        c->scale = scale;
        c->rho = rho;
        if (rho > 0 && isfinite(tempChi)) {
            double alpha = 1. - pow((2 * rho - 1), 3);
            alpha = fmin(alpha, 2. / 3.);
            const double sf = fmax(1. / 3., alpha);
            c->lambda *= sf;
            c->ni = 2;
            c->currentChi = tempChi;
            c->accept = 1;
            c->qmax += 1;
            c->cur = (cur0 + 1 + s) % d.nbs;  // the trial becomes the current estimate
        } else {
            c->lambda *= c->ni;
            c->ni *= 2;
            c->accept = 0;
            c->spec_sticky = 1;
            if (!isfinite(c->lambda)) c->broke = 1;
            else c->qmax += 1;
        }
        const bool again = !c->broke && rho < 0 && c->qmax < c->max_trials;
        if (again) {  // another damped trial of this iteration: the next slot, or the next step
            trials_go_on = true;
            continue;
        }
        trials_go_on = false;
        done = true;
        // end of OptimizationAlgorithmLevenberg::solve(iter)
        const int terminate = (c->qmax == c->max_trials || rho == 0 || !isfinite(c->lambda)) ? 1 : 0;
        if (c->ntrace < kTraceCap)
            d.trace[c->ntrace++] = plba_iter_trace{c->stage, c->iter, c->qmax, terminate, c->chi2_start, c->currentChi,
                                                   c->lambda_start, c->lambda};
        c->iters_done[c->stage] += 1;
        c->iter += 1;
        if (terminate || c->iter >= c->max_iters[c->stage]) {  // optimize() returns
            c->chi2_final[c->stage] = c->currentChi;
            c->spec_sticky = 0;
            if (c->stage + 1 < c->n_stages) c->switch_pending = 1;
            else c->all_done = 1;
        } else {
            // the next iteration's init (iter_init_ctrl with iter > 0), done here so that
            // k_iter_reduce can skip its global reduction (iter_init_fast)
            c->need_iter = 1;
            c->chi2_start = c->currentChi;
            c->lambda_start = c->lambda;
            c->qmax = 0;
            c->accept = 0;
            c->rho = 0.0;
            c->broke = 0;
        }
    }
    // the next step's trial slots (Dev::spec_policy)
    int w = 1;
    if (d.spec_max > 1 && !hold) {
        const int pol = d.spec_policy;
        if (pol == kSpecAlways) w = d.spec_max;
        else if (pol == kSpecAfterReject) w = trials_go_on ? d.spec_max : 1;
        else if (pol == kSpecSticky) w = c->spec_sticky ? d.spec_max : 1;
    }
    c->spec_w = w;
}
__global__ __launch_bounds__(kBlock) void k_decide(Dev d) {
    TRIAL_GUARD
    __shared__ double sh[kBlock / 64];
    decide_body<kBlock>(d, sh);
}

__global__ __launch_bounds__(kLmsNT) void k_lm_solve(Dev d0) {
    // Not TRIAL_SLOT: the folded decision (last arriver) rewrites Ctrl::spec_w inside this launch,
    // so a workgroup dispatched after it would read the NEXT step's width. Every workgroup of the
    // grid (gridDim.y = spec_max) therefore arrives, idle slots included, and all of them read
    // spec_w before arriving: the arrival total does not depend on spec_w and no workgroup can
    // observe the decision's writes.
    TRIAL_GUARD_OF(d0)
    __shared__ double sh[kLmsNT / 64];
    const int nslots = d0.ctrl->spec_w;
    if ((int)blockIdx.y >= nslots) {
        if (d0.fold && arrive_last(d0.cnt, (int32_t)(gridDim.x * gridDim.y))) decide_body<kLmsNT>(d0, sh);
        return;
    }
    const Dev d = slot_view(d0, (int)blockIdx.y);
    const int gt = blockIdx.x * kLmsNT + threadIdx.x;
    const int l = gt / kLmLanes, q = gt % kLmLanes;   // a quad never straddles a wave
    const bool live = l < d.n_lm;
    const int lc = live ? l : 0;
    const Ctrl *cg = d.ctrl;
    const bool solve = *d.solve_okp != 0;
    const bool robust = cg->robust != 0;
    const double lam = d.lam;
    const bool hlm = cg->hlm != kLmG2o;
    // ---- round 1: landmark record + this lane's edge slots
    const bool act = live && d.lm_active[lc] != 0;
    const int off0 = d.lm_off[lc], off1 = d.lm_off[lc + 1];
    double Xc[4], bl[4], H[10];
#pragma unroll
    for (int k = 0; k < 4; ++k) Xc[k] = d.Xc[(size_t)lc * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) bl[k] = d.bl[(size_t)lc * 4 + k];
#pragma unroll
    for (int k = 0; k < 10; ++k) H[k] = d.Hll[(size_t)lc * 10 + k];
    LmEdge sl[kLmSlots];
    bool sv[kLmSlots];
#pragma unroll
    for (int j = 0; j < kLmSlots; ++j) {
        const int e = off0 + q + kLmLanes * j;
        sv[j] = act && e < off1;
        lm_load_edge(d, sv[j] ? e : 0, sl[j]);
    }
    // ---- round 2: x_p of each slot's free pose, the slot's trial pose
    const double *Tt0 = d.Tt;
    double xs[kLmSlots][6], Ts[kLmSlots][12];
#pragma unroll
    for (int j = 0; j < kLmSlots; ++j) {
        const int h = max(sl[j].h, 0);
#pragma unroll
        for (int k = 0; k < 6; ++k) xs[j][k] = d.xp[6 * h + k];
#pragma unroll
        for (int k = 0; k < 12; ++k) Ts[j][k] = Tt0[(size_t)sl[j].kf * 12 + k];
    }
    double chi = 0.0, sc = 0.0;
    // r = b_l − Σ_e Hpl_eᵀ x_p,  Hpl_eᵀ x_p = B_eᵀ (A_e x_p)  (edges of a fixed pose: 0)
    double u[4] = {0, 0, 0, 0}, u45[2] = {0, 0};
    const bool gba_ln = cg->hlm >= kLmGba && live && !is_point_lm(d, l);  // uniform across the quad
    if (act && solve) {
        if (gba_ln) {
#pragma unroll
            for (int j = 0; j < kLmSlots; ++j)
                if (sv[j] && sl[j].h >= 0) lm_hpl_x<true>(sl[j], xs[j], u, u45);
        } else {
#pragma unroll
            for (int j = 0; j < kLmSlots; ++j)
                if (sv[j] && sl[j].h >= 0) lm_hpl_x(sl[j], xs[j], u, u45);
        }
        for (int e = off0 + q + kLmLanes * kLmSlots; e < off1; e += kLmLanes) {  // long tracks
            LmEdge s;
            lm_load_edge(d, e, s);
            if (s.h < 0) continue;
            double x[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = d.xp[6 * s.h + k];
            if (gba_ln) lm_hpl_x<true>(s, x, u, u45);
            else lm_hpl_x(s, x, u, u45);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = quad_sum(u[i]);  // all lanes: DPP reads the whole quad
    if (cg->hlm >= kLmGba) {
        u45[0] = quad_sum(u45[0]);
        u45[1] = quad_sum(u45[1]);
    }
    if (live && gba_ln) {
        // GBA line (src/mapHandler.cpp:3673-3691): x = (Hl6 + λ·diag)⁻¹ (b_l − Σ_e b_e a_e·x_p),
        // X += DX on the 6 endpoint coordinates, ‖DX‖² partial; lane q == 0 writes
        const int li = l - d.n_pt, j = d.ln_gidx[li];
        const double *XLc = d.XLc + (size_t)j * 6;
        double *XLt = d.XLt + (size_t)j * 6;
        double *Xt = d.Xt + (size_t)l * 4;
        if (act && solve) {
            double H[21], L6[21], y[6], x[6];
#pragma unroll
            for (int k = 0; k < 21; ++k) { H[k] = d.Hl6[(size_t)li * 21 + k]; L6[k] = 0.0; }
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) {
                double sj = H[pk(jj, jj)] + lam * H[pk(jj, jj)];
#pragma unroll
                for (int p = 0; p < jj; ++p) sj -= L6[pk(jj, p)] * L6[pk(jj, p)];
                if (!(sj > 0.0))  // a non-positive pivot fails the solve (X unchanged, DX = 0)
                    __hip_atomic_store(d.solve_okp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const double djj = sqrt(sj);
                L6[pk(jj, jj)] = djj;
#pragma unroll
                for (int i = jj + 1; i < 6; ++i) {
                    double t = H[pk(i, jj)];
#pragma unroll
                    for (int p = 0; p < jj; ++p) t -= L6[pk(i, p)] * L6[pk(jj, p)];
                    L6[pk(i, jj)] = t / djj;
                }
            }
            const double uu[6] = {u[0], u[1], u[2], u[3], u45[0], u45[1]};
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double t = d.bl6[(size_t)li * 6 + i] - uu[i];
#pragma unroll
                for (int p = 0; p < i; ++p) t -= L6[pk(i, p)] * y[p];
                y[i] = t / L6[pk(i, i)];
            }
#pragma unroll
            for (int i = 5; i >= 0; --i) {
                double t = y[i];
#pragma unroll
                for (int p = i + 1; p < 6; ++p) t -= L6[pk(p, i)] * x[p];
                x[i] = t / L6[pk(i, i)];
            }
            if (q == 0) {
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    sc += x[i] * x[i];
                    XLt[i] = XLc[i] + x[i];
                }
            }
        } else if (q == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) XLt[i] = XLc[i];
        }
        if (q == 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) Xt[i] = Xc[i];
    } else if (live) {
        double *Xt = d.Xt + (size_t)l * 4;
        if (act) {
            const bool pt = is_point_lm(d, l);
            const int DIM = pt ? 3 : 4;
            double x[4] = {0, 0, 0, 0};
            if (solve) {
                // (Hll + λI) = L Lᵀ (packed lower), x = L⁻ᵀ L⁻¹ (b_l − u); the hand-rolled LM in
                // the signed form of lm_chol, x = L⁻ᵀ S L⁻¹ (b_l − u)
                const bool sgn = cg->hlm == kLmLbaPlucker;
                double L[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, S[4] = {1.0, 1.0, 1.0, 1.0};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < DIM) {
                        double sj = H[pk(j, j)] + (hlm ? lam * H[pk(j, j)] : lam);
#pragma unroll
                        for (int p = 0; p < j; ++p) sj -= (L[pk(j, p)] * S[p]) * L[pk(j, p)];
                        const double sg = (sgn && sj < 0.0) ? -1.0 : 1.0;
                        S[j] = sg;
                        // a zero pivot fails the hand-rolled LM's solve (the oracle's unpivoted
                        // LDLᵀ; the step is then not applied, k_decide's hlm branch); GBA keeps
                        // the Cholesky form and fails on any non-positive pivot
                        if (hlm && (sgn ? sj == 0.0 : !(sj > 0.0)))
                            __hip_atomic_store(d.solve_okp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const double djj = 1.0 / sqrt(sg * sj);  // reciprocal diagonal (as lm_chol)
                        L[pk(j, j)] = djj;
#pragma unroll
                        for (int i = j + 1; i < 4; ++i) {
                            if (i < DIM) {
                                double t = H[pk(i, j)];
#pragma unroll
                                for (int p = 0; p < j; ++p) t -= L[pk(i, p)] * (L[pk(j, p)] * S[p]);
                                L[pk(i, j)] = (t * djj) * sg;
                            }
                        }
                    }
                }
                double y[4] = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < DIM) {
                        double t = bl[i] - u[i];
#pragma unroll
                        for (int p = 0; p < i; ++p) t -= L[pk(i, p)] * y[p];
                        y[i] = t * L[pk(i, i)];
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] *= S[i];
#pragma unroll
                for (int i = 3; i >= 0; --i)
                    if (i < DIM) {
                        double t = y[i];
#pragma unroll
                        for (int p = i + 1; p < 4; ++p)
                            if (p < DIM) t -= L[pk(p, i)] * x[p];
                        x[i] = t * L[pk(i, i)];
                    }
                if (q == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) d.xl[(size_t)l * 4 + i] = x[i];
                }
            } else {  // failed solve: the last successful solve's x (A13)
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = d.xl_prev[(size_t)l * 4 + i];
            }
            if (q == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < DIM) sc += hlm ? x[i] * x[i] : x[i] * (lam * x[i] + bl[i]);
            }
            double X[4] = {0, 0, 0, 0}, Lp[6] = {0, 0, 0, 0, 0, 0};
            if (pt) {
                X[0] = Xc[0] + x[0]; X[1] = Xc[1] + x[1]; X[2] = Xc[2] + x[2]; X[3] = 0.0;
                if (q == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) Xt[i] = X[i];
                }
            } else {
                Xt[q] = orth_oplus_quad(Xc, x, q, Lp);
                if (q == 0) {
                    double *Lt = d.Lpt + (size_t)(l - d.n_pt) * 8;
#pragma unroll
                    for (int k = 0; k < 6; ++k) Lt[k] = Lp[k];
                }
            }
            // the landmark's edges at the trial state (computeActiveErrors of the trial); the
            // trial poses were written by the factorisation kernel
            const double delta = pt ? d.huber_pt : d.huber_ln;
            if (!hlm)  // (the hand-rolled LM scores a step at the next linearisation)
#pragma unroll
            for (int j = 0; j < kLmSlots; ++j)
                if (sv[j] && sl[j].act) chi += lm_eval(d, sl[j], Ts[j], pt, X, Lp, robust, delta);
            for (int e = off0 + q + kLmLanes * kLmSlots; e < off1 && !hlm; e += kLmLanes) {  // long tracks
                if (!d.e_active[e]) continue;
                LmEdge s;
                lm_load_edge(d, e, s);
                chi += lm_eval(d, s, Tt0 + (size_t)s.kf * 12, pt, X, Lp, robust, delta);
            }
        } else {
            if (q == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) Xt[i] = Xc[i];
                if (!is_point_lm(d, l)) {  // an inactive line keeps its Plücker vector too
                    const double *Lc = d.Lpc + (size_t)(l - d.n_pt) * 8;
                    double *Lt = d.Lpt + (size_t)(l - d.n_pt) * 8;
#pragma unroll
                    for (int k = 0; k < 6; ++k) Lt[k] = Lc[k];
                }
            }
        }
    }
    const double s2 = block_sum<kLmsNT>(sc, sh);
    const double s1 = block_sum<kLmsNT>(chi, sh);
    if (threadIdx.x == 0) {
        st_sc1(d.part_lms + blockIdx.x, s2);
        st_sc1(d.part_lm + blockIdx.x, s1);
    }
    // the last workgroup to finish takes the trial decision (k_decide's work)
    if (d.fold && arrive_last(d.cnt, (int32_t)(gridDim.x * gridDim.y))) decide_body<kLmsNT>(d0, sh);
}
// sharded: this rank's trial χ² and landmark scale terms into the all-reduced decision array
__global__ __launch_bounds__(kBlock) void k_decide_pack(Dev d) {
    TRIAL_GUARD
    __shared__ double sh[kBlock / 64];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < d.n_lms_blocks; i += kBlock) a += d.part_lm[i];
    for (int i = threadIdx.x; i < d.n_lms_blocks; i += kBlock) b += d.part_lms[i];
    const double ta = block_sum<kBlock>(a, sh);
    const double tb = block_sum<kBlock>(b, sh);
    if (threadIdx.x == 0) {
        d.red_dec_loc[0] = ta;
        d.red_dec_loc[1] = tb;
        // a failed solve on this rank (the hand-rolled LM's landmark pivots are rank-local): the
        // ranks sum the failures so that every rank takes the same decision (decide_body)
        d.red_dec_loc[2] = d.ctrl->solve_ok[0] != 0 ? 0.0 : 1.0;
    }
}

// changeOrthToPluker (g2o_types.h:367-387) of every line at the current state into Lpb[cur];
// launched once per schedule (estimates may have been reset or uploaded in between)
__global__ void k_line_pluker(Dev d) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= d.n_ln) return;
    const int cur = d.ctrl->cur;
    double L[6];
    orth_to_pluker(d.Xb[cur] + (size_t)(d.n_pt + l) * 4, L);
    double *o = d.Lpb[cur] + (size_t)l * 8;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = L[k];
}

// plba_reset_estimates in one launch: the initial estimates into state buffer 0, zeros into every
// solve / χ² buffer and the edge levels, and the three buffer indices of the control block back to
// 0. One grid-stride loop per range; the extents are the ones the arrays are allocated with
// (an empty array still owns one record, plba_layout.hpp).
__global__ __launch_bounds__(kBlock) void k_reset_estimates(Dev d) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x, nt = (size_t)gridDim.x * kBlock;
    auto copy = [&](double *dst, const double *src, size_t n) {
        for (size_t i = t; i < n; i += nt) dst[i] = src[i];
    };
    auto zero = [&](double *dst, size_t n) {
        for (size_t i = t; i < (n > 0 ? n : 1); i += nt) dst[i] = 0.0;
    };
    copy(d.Tb[0], d.T_init, (size_t)d.n_kf * 12);
    copy(d.Xb[0], d.X_init, (size_t)d.n_lm * 4);
    for (int b = 0; b < d.nbx; ++b) {
        zero(d.xpb[b], (size_t)d.n);
        zero(d.xlb[b], (size_t)d.n_lm * 4);
        zero(d.chi2b[b], (size_t)d.E);
    }
    // levels are bytes: whole words first (the array is 256-byte aligned), then the tail
    const size_t lb = d.E > 0 ? (size_t)d.E : 1, lw = lb / 4;
    uint32_t *lv = reinterpret_cast<uint32_t *>(d.e_level);
    for (size_t i = t; i < lw; i += nt) lv[i] = 0u;
    for (size_t i = lw * 4 + t; i < lb; i += nt) d.e_level[i] = 0;
    if (t == 0) {
        d.ctrl->cur = 0;
        d.ctrl->last_ok = 0;
        d.ctrl->chi_src = 0;
    }
}

// ---------------------------------------------------------------- outlier pass helpers
// computeError() at the current state for edges of `level`. The current state buffer and the χ²
// buffer are the control block's, so the launch may be queued behind the steps that decide them.
// when_done: the epilogue of a schedule, queued before the host has polled the control block —
// nothing happens unless the schedule finished (and no hand-off wait timed out).
__global__ void k_refresh(Dev d, int level, int when_done) {
    if (when_done && (!d.ctrl->all_done || d.ctrl->dev_error)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= d.E || d.e_level[e] != level) return;
    const double *T = Tcur(d) + (size_t)d.e_kf[e] * 12;
    const double *X = Xcur(d) + (size_t)d.e_lm[e] * 4;
    const double *obs = d.e_obs + (size_t)e * 4;
    double err[2];
    if (e < d.Ep) {
        double z;
        point_error(T, X, obs, d.cam, err, z);
    } else {
        double L[6];
        orth_to_pluker(X, L);
        line_error(T, L, obs, d.cam, err);
    }
    const double info = d.e_info[e];
    chi2cur(d)[e] = err[0] * (info * err[0]) + err[1] * (info * err[1]);
}
// isDepthPositive() at the current state
__global__ void k_depth(Dev d, uint8_t *out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= d.Ep) return;
    double Pc[3];
    point_pc(Tcur(d) + (size_t)d.e_kf[e] * 12, Xcur(d) + (size_t)d.e_lm[e] * 4, Pc);
    out[e] = Pc[2] > 0.0 ? 1 : 0;
}

// unsharded download: poses, landmark states and per-edge outputs in the caller's order, one
// staging block (Tcw | pt_xyz | ln_orth | χ² by e_gpos, points then lines | bytes:
// isDepthPositive [Ep] | levels by e_gpos)
__global__ void k_out_scatter(Dev d, double *od, int want_depth, int cur, int chi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double *T = d.Tb[cur], *X = d.Xb[cur];  // the host's current state / χ² buffer index
    const size_t nk = d.n_kf, np = d.n_pt, nl = d.n_ln, E = d.E;
    if (i < d.n_kf)
#pragma unroll
        for (int k = 0; k < 12; ++k) od[(size_t)i * 12 + k] = T[(size_t)i * 12 + k];
    double *opt = od + nk * 12;
    if (i < d.n_lm) {
        const int gp = d.lm_gpos[i];
        const double *x = X + (size_t)i * 4;
        if (gp < d.n_pt) {
#pragma unroll
            for (int k = 0; k < 3; ++k) opt[(size_t)gp * 3 + k] = x[k];
        } else {
            double *o = opt + np * 3 + (size_t)(gp - d.n_pt) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = x[k];
        }
    }
    if (i < d.E) {
        const int g = d.e_gpos[i];
        opt[np * 3 + nl * 4 + g] = d.chi2b[chi][i];
        uint8_t *ob = reinterpret_cast<uint8_t *>(opt + np * 3 + nl * 4 + E);
        ob[(size_t)d.Ep + g] = d.e_level[i];
        if (want_depth && i < d.Ep) {
            double Pc[3];
            point_pc(T + (size_t)d.e_kf[i] * 12, X + (size_t)d.e_lm[i] * 4, Pc);
            ob[g] = Pc[2] > 0.0 ? 1 : 0;
        }
    }
}

// sharded: scatter this rank's landmark states and per-edge outputs to their whole-window
// positions (the buffer is zeroed first and summed over ranks afterwards)
__global__ void k_gather(Dev d, const uint8_t *depth) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.n_lm)
#pragma unroll
        for (int k = 0; k < 4; ++k) d.gat[(size_t)d.lm_gpos[i] * 4 + k] = Xcur(d)[(size_t)i * 4 + k];
    if (i < d.E) {
        double *o = d.gat + (size_t)d.n_lm_g * 4;
        const int g = d.e_gpos[i];
        o[g] = chi2cur(d)[i];
        o[(size_t)d.E_g + g] = i < d.Ep ? (double)depth[i] : 0.0;
        o[2 * (size_t)d.E_g + g] = (double)d.e_level[i];
    }
}

}  // namespace plba
