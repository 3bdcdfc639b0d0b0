// plba_band.hpp — LDS-window (register-resident) banded factorisation of the reduced camera
// system: one sweep (k_rcs_factor_band) or from both ends (k_rcs_factor_twisted).
#pragma once

#include "plba_rcs.hpp"

namespace plba {

// Block-banded LDLᵀ of the reduced camera system (A = L_B D_B L_Bᵀ, 6x6 pose blocks) with an
// LDS sliding window of bw+1 block rows, forward substitution folded in (augmented column b),
// then a one-wave backward pass. One workgroup; 3 barriers per pose block.
// Failure semantics of SimplicialLDLT: a zero pivot (Gauss–Jordan pivots of S_k are the LDLᵀ
// pivots) fails the solve and x_p keeps its previous value.
// fast IEEE-accurate reciprocal: v_rcp_f64 + two Newton steps
__device__ __forceinline__ double rcp_nr(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
// v_rcp_f64 + one Newton step (the estimate is good to ~2^-26, one step squares the error)
__device__ __forceinline__ double rcp_nr1(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    return fma(fma(-x, r, 1.0), r, r);
}

// Lane-local LDLᵀ of a 6x6 symmetric block held as its packed lower triangle (row-major,
// ltri(i, j) for j <= i): on return s holds the unit lower factor below the diagonal and dv the
// reciprocal pivots. zp is set if a pivot is exactly zero (SimplicialLDLT's failure condition).
__host__ __device__ constexpr int ltri(int i, int j) { return i * (i + 1) / 2 + j; }
__device__ __forceinline__ void ldl6_inplace(double (&s)[21], double (&dv)[6], bool &zp) {
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const double dp = s[ltri(p, p)];
        zp = zp || dp == 0.0;
        const double rp = rcp_nr1(dp);
        dv[p] = rp;
        double col[6];
#pragma unroll
        for (int i = p + 1; i < 6; ++i) col[i] = s[ltri(i, p)];
#pragma unroll
        for (int i = p + 1; i < 6; ++i) s[ltri(i, p)] = col[i] * rp;
#pragma unroll
        for (int i = p + 1; i < 6; ++i)
#pragma unroll
            for (int j = p + 1; j <= i; ++j) s[ltri(i, j)] = fma(-s[ltri(i, p)], col[j], s[ltri(i, j)]);
    }
}
// x <- (L D Lᵀ)⁻¹ x with the factors of ldl6_inplace
__device__ __forceinline__ void ldl6_solve(const double (&s)[21], const double (&dv)[6], double (&x)[6]) {
#pragma unroll
    for (int i = 1; i < 6; ++i)
#pragma unroll
        for (int m = 0; m < i; ++m) x[i] = fma(-s[ltri(i, m)], x[m], x[i]);
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] *= dv[i];
#pragma unroll
    for (int i = 4; i >= 0; --i)
#pragma unroll
        for (int m = 5; m > i; --m) x[i] = fma(-s[ltri(m, i)], x[m], x[i]);
}

// Lane-local inverse of a 6x6 pivot block just published to LDS (entry (r, c) at S[r * 6 + c]; its
// lower triangle is read): every lane factors S LDLᵀ in its own registers, then lanes r*6+c
// (0..35) return (S⁻¹)[r][c] (column c of S⁻¹ solved from e_c) and lanes 36+r return (S⁻¹y)[r].
// No cross-lane traffic: replaces gj_inverse6's 6 pivot broadcasts + 18 LDS permutes, which on
// the register-window band kernel contend with the worker waves' trailing-update LDS reads.
// The LDLᵀ pivots are the system's, so a zero pivot fails the solve as SimplicialLDLT does.
// (LDS operations of one wave complete in order: the caller's stores of S and y need no wait.)
__device__ __forceinline__ double ldl_inverse6(const double *S, const double *y, int lane, bool &fail) {
    double s[21], dv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) s[ltri(i, j)] = S[i * 6 + j];
    bool zp = false;
    ldl6_inplace(s, dv, zp);
    if (zp) fail = true;
    const bool mat = lane < 36;
    const int r = mat ? lane / 6 : min(lane - 36, 5), c = lane % 6;
    double x[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) x[m] = mat ? (m == c ? 1.0 : 0.0) : y[m];
    ldl6_solve(s, dv, x);
    double out = x[0];
#pragma unroll
    for (int m = 1; m < 6; ++m) out = r == m ? x[m] : out;
    return out;
}
// Gauss–Jordan on [S | y] (6x7, one entry per lane): lanes r*6+c (0..35) hold S and return
// S^{-1}; lanes 36+r hold y and return z = S^{-1} y. No pivoting: the pivots are the LDLᵀ
// pivots, so a zero pivot reports failure exactly as SimplicialLDLT's NumericalIssue does.
__device__ __forceinline__ double gj_inverse6(double M, int lane, bool &fail) {
    const bool mat = lane < 36, rhs = lane >= 36 && lane < 42;
    const int r = mat ? lane / 6 : (rhs ? lane - 36 : 0);
    const int c = mat ? lane % 6 : 0;
    double I = (mat && r == c) ? 1.0 : (rhs ? M : 0.0);  // rhs lanes carry y in I
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        // the pivot comes from a compile-time lane: v_readlane (SGPR broadcast) instead of an
        // LDS-crossbar round trip, so its reciprocal overlaps the three row/column permutes
        const double piv = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(M), 7 * p),
                                            __builtin_amdgcn_readlane(__double2loint(M), 7 * p));
        const double f = __shfl(M, r * 6 + p, 64);
        double ip = __shfl(I, rhs ? 36 + p : p * 6 + c, 64);
        double mp = __shfl(M, p * 6 + c, 64);
        if (piv == 0.0) fail = true;
        const double rp = rcp_nr(piv);
        mp = mp * rp;
        ip = ip * rp;
        if (r == p) { M = mp; I = ip; }
        else { M = fma(-f, mp, M); I = fma(-f, ip, I); }
    }
    return I;
}

// Block-banded LDLᵀ with lookahead, templated on the envelope bandwidth BW (pose blocks).
// Wave 0 carries the critical chain
//   S_k^{-1} -> L_{k+1,k} -> S_{k+1} = A_{k+1,k+1} - L_{k+1,k} A_{k+1,k}ᵀ -> S_{k+1}^{-1}
// while waves 1..15 compute the other L blocks and the trailing updates of step k
// (2 LDS-only barriers per step). Each worker's entries and LDS offsets are compile-time /
// hoisted; window slots advance incrementally (no runtime modulo in the loop).
//
// band_forward eliminates the first `nsteps` block rows of an `nrows`-row band (forward
// substitution folded in) and, when `sep` is given, stores the updated rows
// nsteps..nsteps+BW-1 — the separator a second segment meets (k_rcs_factor_twisted).
struct BandSeg {
    const double *Bd, *bs;     // [nrows][BW+1][36] block (i, i-w) row-major, [nrows][6]
    double *Lband, *Kinv, *zb; // outputs, indexed by this segment's row numbering
    int nrows, nsteps;
    double *sep;               // nullable: [BW][BW+1][36] + [BW][6]
};

// Register-resident band window. Block (i, i-w) of a live row is owned by a pair of worker
// threads (3 rows each; whole blocks on one thread for bw 25..27) for its whole life in the
// window and updated in registers; it is written to LDS once, when it becomes part of the next
// pivot column (the step's operand A_jk and the source of L), or, on the diagonal, when it becomes
// the next pivot block. Ownership follows diagonal-major rings: diagonal w has C_w = W-w+1 slots,
// row i in slot i mod C_w; at step k the slot's offset o = (slot - k - w) mod C_w says which row
// it holds (i = k+w+o): o = 0 the pivot column, 1 <= o <= BW-w a trailing block (pair wi = w+o,
// wj = o), o = C_w-1 the spare slot whose row k+W enters (staged, below). W(W+3) half blocks
// (bw 23: 648 of the 704 worker threads of a 768-thread workgroup); LDS keeps only two pivot
// columns, the pivot blocks, the staged rows and the L / S^-1 / z staging rings, so no
// read-modify-write of the trailing blocks goes through LDS.
__host__ __device__ constexpr int bd_cap(int W, int w) { return W - w + 1; }
__host__ __device__ constexpr int bd_base(int W, int w) { return w * (W + 1) - w * (w - 1) / 2; }
__host__ __device__ constexpr int bd_blocks(int W) { return W * (W + 3) / 2; }

template <int BW>
__device__ __forceinline__ void band_lds(double *lds, int R, double *&col, double *&piv, double *&bwin, double *&Lcol,
                                         double *&Kv, double *&xr, double *&part, double *&ys, double *&ringL,
                                         double *&ringK, double *&ringZ) {
    constexpr int W = BW + 1;
    col = lds;                                   // [2][W][36] pivot columns k, k+1: block (c+w, c) at [c&1][w]
    piv = col + (size_t)2 * W * 36;              // [2][36]  pivot block (c, c) at [c&1]
    bwin = piv + 72;                             // [W][6]  right-hand sides, row slot ring
    // (the entering rows are staged in band_forward's static LDS: band_static_bytes)
    Lcol = bwin + (size_t)W * 6;                 // [W][36]  (index w = 1..BW)
    Kv = Lcol + (size_t)W * 36;                  // [2][36]  S_k^{-1} double buffer
    xr = Kv + 72;                                // [W][6]  ring of solved x blocks
    part = xr + (size_t)W * 6;                   // [W][6]
    ys = part + (size_t)W * 6;                   // [2][6]  y_k snapshots
    ringL = ys + 12;                             // [R][BW][36]
    ringK = ringL + (size_t)R * BW * 36;         // [R+1][36]
    ringZ = ringK + (size_t)(R + 1) * 36;        // [R+1][6]
}
// doubles of the band layout above
__host__ __device__ constexpr size_t band_lds_doubles(int bw, int R) {
    return (size_t)(bw + 1) * 72 + 72 + (size_t)(bw + 1) * (6 + 36 + 6 + 6) + 72 + 12 + (size_t)R * bw * 36 +
           (size_t)(R + 1) * 42;
}
// static LDS of band_forward: the entering rows' staging buffers [2][W*36 + 6] (blocks, right-hand
// side) plus a few flags. A separate LDS object from the dynamic window, so that the compiler can
// tell the direct global->LDS loads into it from the window's reads (with one LDS object every
// ds_read after such a load waits for it)
// entering-row staging buffers of band_forward: a row is issued at the start of a step's second
// phase and retired before its last barrier (round 6: a third buffer with the row in flight
// across the barrier, retired one step later with vmcnt(1), measured 294 -> 303 µs at C3R)
constexpr int kBandStage = 2;
__host__ __device__ constexpr size_t band_static_bytes(int bw) { return 8 * kBandStage * ((size_t)(bw + 1) * 36 + 6) + 64; }
// The twisted kernel's merge, after both segments have exported their separator windows, reuses
// the LDS from 0: the separator's L blocks [bw(bw-1)/2][36], pivot inverses [bw][36], the
// current pivot column [2][bw][36] (step parity), the pivot blocks [bw][36], its right-hand side and
// two solution copies [3][6bw]; behind the x_p staging [nf][6] at offset 0 (twisted_lds_bytes:
// the back substitution's streamed chunks reuse the region, band_backward_stream).
__host__ __device__ constexpr size_t twisted_merge_doubles(int bw) {
    return (size_t)bw * (bw - 1) / 2 * 36 + 144 * (size_t)bw + 3 * (size_t)(6 * bw);
}

template <int BW>
__device__ __forceinline__ bool band_forward(const BandSeg &g, double *lds, int ring) {
    constexpr int NT = band_nt(BW), W = BW + 1, NW = NT - 64;
    constexpr int UR = band_ur(BW), UPB = 6 / UR, UE = UR * 6;  // rows per owner, owners per block, entries
    static_assert(UPB * bd_blocks(W) <= NW, "one owned (part) block per worker thread");
    constexpr int LPT = ((BW > 1 ? BW - 1 : 0) * 36 + NW - 1) / NW;  // L entries per worker (w >= 2)
    const int nrows = g.nrows, nsteps = g.nsteps;
    double *col, *piv, *bwin, *Lcol, *Kv, *xr, *part, *ys, *ringL, *ringK, *ringZ;
    band_lds<BW>(lds, ring, col, piv, bwin, Lcol, Kv, xr, part, ys, ringL, ringK, ringZ);
    const int R = ring;
    const int RK = R + 1;                         // S^-1 / z of step k+1 are written during step k
    __shared__ int s_fail;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // wave index in an SGPR: the loop's wave-0 tests and the staging-row split need no per-lane
    // register (a VGPR tid carried through the step loop was spilled and reloaded every step)
    const int wv_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool crit = wv_s == 0;                  // wave 0
    const int wt = tid - 64;                      // worker thread index
    if (tid == 0) s_fail = 0;
    // ---- the (part) block this worker owns: slot p of diagonal w, rows oh/6 .. oh/6+UR-1
    const bool own = !crit && wt < UPB * bd_blocks(W);
    int ow = 0, op = 0;
    if (own) {
        const int b = wt / UPB;
        while (bd_base(W, ow + 1) <= b) ++ow;
        op = b - bd_base(W, ow);
    }
    const int oC = bd_cap(W, ow), oh = (max(wt, 0) % UPB) * UE;
    int oo = ((op - ow) % oC + oC) % oC;          // offset at step 0
    double t[UE];
    {   // rows 0..BW (the spare slot's row W arrives during step 0)
        const int i = ow + oo;
        const bool ld = own && oo != oC - 1 && i < nrows;
        const double *src = g.Bd + ((size_t)(ld ? i : 0) * W + ow) * 36 + oh;
#pragma unroll
        for (int j = 0; j < UE; ++j) t[j] = ld ? src[j] : 0.0;
        if (own) {
            double *dst = nullptr;
            if (ow >= 1 && oo == 0) dst = col + (size_t)ow * 36;   // column 0
            else if (ow == 0 && oo <= 1) dst = piv + oo * 36;      // pivots (0,0), (1,1)
            if (dst)
#pragma unroll
                for (int j = 0; j < UE; ++j) dst[oh + j] = t[j];
        }
    }
    for (int t2 = tid; t2 < W * 6; t2 += NT) bwin[t2] = (t2 / 6 < nrows) ? g.bs[t2] : 0.0;
    // Entering rows (W blocks + the right-hand side) come in by direct global->LDS loads
    // (global_load_lds_dwordx4, no VGPR destination): row r to staging buffer r & 1, issued by the
    // worker waves at the start of step r-W-1's second phase and retired before its last barrier;
    // the diagonal-BW block goes into the pivot column during step r-W, the rest into the owners'
    // registers at the top of step r-BW. No owner register and no spill reload waits on a global
    // load. Past the band's end the last row is loaded again (never read: readers stop at wmax).
    constexpr int RW = W * 36 + 6, NPC = RW / 2;  // doubles per staged row, 16-byte pieces
    __shared__ __attribute__((aligned(16))) double stgb[kBandStage * RW];
    // staging buffer of a row (r mod kBandStage): incremental, no runtime modulo in the loop
    auto stg = [&](int slot) { return stgb + (size_t)slot * RW; };
    auto stage_row = [&](int row, int slot, int wv, int lnv) {  // wv: worker wave index (uniform)
      for (int pb = wv * 64; pb < NPC; pb += NW) {  // (more pieces than worker lanes at bw >= 24)
        const int p = pb + lnv;
        if (p < NPC) {
            const int rr = min(row, nrows - 1);
            const double *src = p < W * 18 ? g.Bd + (size_t)rr * W * 36 + 2 * p : g.bs + (size_t)rr * 6 + 2 * (p - W * 18);
            // inline asm rather than the builtin: with the builtin the compiler waits for the load
            // before every later ds_read of the window (it cannot tell the LDS objects apart);
            // this load is retired by the explicit vmcnt(0) before the step's last barrier
            const unsigned dst = __builtin_amdgcn_readfirstlane(
                (unsigned)(size_t)(__attribute__((address_space(3))) double *)(stg(slot) + pb * 2));
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(src), "s"(dst)
                         : "memory");
        }
      }
    };
    if (!crit) {
        stage_row(W, W % kBandStage, wv_s - 1, lane);
        // retired here like every later row's (the compiler does not track the inline-asm load,
        // and step 0's phase 2 already copies its diagonal-BW block out of the staging buffer)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(tid) < 64) __builtin_amdgcn_s_setprio(3);
    // S_0^{-1}, y_0, z_0
    if (crit) {
        bool fail = false;
        if (lane >= 36 && lane < 42) ys[lane - 36] = bwin[lane - 36];
        const double I = ldl_inverse6(piv, bwin, lane, fail);
        if (lane < 36) { Kv[lane] = I; ringK[lane] = I; }
        else if (lane < 42) ringZ[lane - 36] = I;
        if (fail && lane == 0) s_fail = 1;
    }
    lds_barrier();
    int sk = 0, kR = 0, kRK = 1;                  // k % W (rhs row slots), k % R, (k+1) % RK
    int sB = BW % kBandStage, sW = W % kBandStage; // staging slots of rows k+BW, k+W
    int fr0 = 0;                                  // (first step of the current flush batch) % RK
    // a zero pivot sets s_fail and the sweep runs on (inf/NaN blocks are never used: the
    // caller drops the solve); no per-step LDS read of the flag on the critical chain
    for (int k = 0; k < nsteps; ++k) {
        // per-lane indices made opaque each step: everything derived from them is recomputed in
        // the step (a few integer ops) instead of being hoisted out of the loop as dozens of
        // loop-invariant registers that then spill to scratch (a scratch reload waits for every
        // outstanding global load, the spare-slot loads included)
        // (the lane index is re-derived from v_mbcnt each step: carried, it was spilled and its
        // scratch reload at the step top stalled the critical wave on vmcnt)
        int wtl = wt, owl = ow, ohl = oh, oCl = oC;
        asm volatile("" : "+v"(wtl), "+v"(owl), "+v"(ohl), "+v"(oCl));
        const int lnl = (int)__lane_id();
        const int kb = k & 1;
        const int wmax = min(BW, nrows - 1 - k);
        const double *Kk = Kv + kb * 36;
        const double *yk = ys + kb * 6;
        const double *colk = col + (size_t)kb * W * 36;
        auto slot = [&](int w) { const int x = sk + w; return x >= W ? x - W : x; };
        if (!crit && k > 0) {
            // row k+BW (last step's spare slot) from its staging buffer into the owners' registers
            // (bw 1: its block (k+1, k+1) is also this step's next pivot); its right-hand side into
            // its row slot. (Its diagonal-BW block, this step's pivot-column entry, was copied in
            // the previous step: phase 1 reads it before any barrier of this step.)
            const double *sr = stg(sB);  // row k+BW
            if (own && oo == oCl - 2) {
                const double2 *src = (const double2 *)(sr + owl * 36 + ohl);
                double2 *D = (BW == 1 && owl == 0) ? (double2 *)(piv + (kb ^ 1) * 36 + ohl) : nullptr;
#pragma unroll
                for (int v = 0; v < UE / 2; ++v) {
                    const double2 x = src[v];
                    t[2 * v] = x.x;
                    t[2 * v + 1] = x.y;
                    if (D) D[v] = x;
                }
            }
            if (wtl < 6) bwin[slot(BW) * 6 + wtl] = k + BW < nrows ? sr[W * 36 + wtl] : 0.0;
        }
        // ---- phase 1: L_{k+w,k} = A_{k+w,k} S_k^{-1}   (w = 1 on wave 0, w >= 2 on the workers)
        if (crit) {
            if (lnl < 36 && wmax >= 1) {
                const int c = lnl % 6;
                const double *Aik = colk + 36 + (lnl / 6) * 6;
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < 6; ++m) v = fma(Aik[m], Kk[m * 6 + c], v);
                Lcol[36 + lnl] = v;
                ringL[((size_t)kR * BW + 0) * 36 + lnl] = v;
            }
        } else {
#pragma unroll
            for (int q = 0; q < LPT; ++q) {
                const int t2 = wtl + 36 + q * NW;
                const int w = 1 + t2 / 36, e = t2 % 36;
                if (t2 < BW * 36 && w <= wmax) {
                    const double *Aik = colk + (size_t)w * 36 + (e / 6) * 6;
                    const int c = e % 6;
                    double v = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) v = fma(Aik[m], Kk[m * 6 + c], v);
                    Lcol[w * 36 + e] = v;
                    ringL[((size_t)kR * BW + (w - 1)) * 36 + e] = v;
                }
            }
        }
        lds_barrier();
        // ---- phase 2 (the worker waves first put row k+W+1 in flight)
        if (!crit) stage_row(k + W + 1, sB, wv_s - 1, lnl);  // (row k+BW's buffer: consumed at the top)
        if (crit) {
            if (k + 1 < nrows) {
                const int s1 = slot(1), k1b = kb ^ 1;
                // lanes 0..35: S_{k+1} = A_{k+1,k+1} - L_{k+1,k} A_{k+1,k}ᵀ
                // lanes 36..41: y_{k+1} = b_{k+1} - L_{k+1,k} y_k
                double M = 0.0;
                if (lnl < 42) {
                    const bool mat = lnl < 36;
                    const int r = mat ? lnl / 6 : lnl - 36, c = mat ? lnl % 6 : 0;
                    double sacc = 0.0;
                    if constexpr (BW >= 1) {
                        const double *L1 = Lcol + 36 + r * 6;
                        const double *A1 = mat ? colk + 36 + c * 6 : yk;
#pragma unroll
                        for (int m = 0; m < 6; ++m) sacc = fma(L1[m], A1[m], sacc);
                    }
                    double *dst = mat ? piv + k1b * 36 + lnl : bwin + s1 * 6 + r;
                    M = *dst - sacc;
                    *dst = M;
                    if (!mat) ys[k1b * 6 + r] = M;
                }
                bool fail = false;
                const double I = ldl_inverse6(piv + k1b * 36, ys + k1b * 6, lnl, fail);
                if (lnl < 36) { Kv[k1b * 36 + lnl] = I; ringK[kRK * 36 + lnl] = I; }
                else if (lnl < 42) ringZ[kRK * 6 + lnl - 36] = I;
                // the look-ahead inverse past the last eliminated row (a separator row) is not a pivot
                if (fail && lnl == 0 && k + 1 < nsteps) s_fail = 1;
            }
        } else {
            // trailing update of the owned (part) block (k+wi, k+wj), wi = w+o, wj = o:
            // A_ij -= L_ik A_jkᵀ (same fma order per entry as one entry at a time); (1,1) is wave 0's
            const int wi = owl + oo;
            if (own && oo >= 1 && oo != oCl - 1 && wi <= wmax && !(owl == 0 && oo == 1)) {
                const double2 *Li = (const double2 *)(Lcol + wi * 36 + ohl);
                const double2 *Aj = (const double2 *)(colk + (size_t)oo * 36);
                double l[UE];
#pragma unroll
                for (int v = 0; v < UE / 2; ++v) { const double2 x = Li[v]; l[2 * v] = x.x; l[2 * v + 1] = x.y; }
#pragma unroll
                for (int c = 0; c < 6; ++c) {  // column c of the target = row c of A_jk
                    double a[6];
#pragma unroll
                    for (int v = 0; v < 3; ++v) { const double2 x = Aj[c * 3 + v]; a[2 * v] = x.x; a[2 * v + 1] = x.y; }
#pragma unroll
                    for (int r = 0; r < UR; ++r) {
                        double sacc = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; ++m) sacc = fma(l[r * 6 + m], a[m], sacc);
                        t[r * 6 + c] -= sacc;
                    }
                }
                // next step's pivot column (k+1+w, k+1) / the pivot block after next (k+2, k+2)
                double *dst = (owl >= 1 && oo == 1) ? col + ((size_t)(kb ^ 1) * W + owl) * 36
                            : (owl == 0 && oo == 2) ? piv + kb * 36 : nullptr;
                if (dst) {
                    double2 *D = (double2 *)(dst + ohl);
#pragma unroll
                    for (int v = 0; v < UE / 2; ++v) D[v] = make_double2(t[2 * v], t[2 * v + 1]);
                }
            }
            // the next pivot column's diagonal-BW entry (k+W, k+1), from row k+W's staging buffer
            if (wtl < 18) {
                const double *cs = stg(sW) + BW * 36;  // row k+W
                ((double2 *)(col + ((size_t)(kb ^ 1) * W + BW) * 36))[wtl] = ((const double2 *)cs)[wtl];
            }
            // b_i -= L_ik y_k for w >= 2 (last worker wave)
            {
                const int t2 = NW - 1 - wtl;  // 0.. on the last wave
                if (t2 < (wmax - 1) * 6) {
                    const int wr = 2 + t2 / 6, r = t2 % 6;
                    double sacc = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) sacc = fma(Lcol[wr * 36 + r * 6 + m], yk[m], sacc);
                    bwin[slot(wr) * 6 + r] -= sacc;
                }
            }
            if (kR == R - 1 || k == nsteps - 1) {  // flush the staged steps k0..k to global
                const int k0 = k - kR;
                const int cnt = kR + 1;
                if constexpr (BW >= 1)
                    for (int t2 = wtl; t2 < cnt * BW * 36; t2 += NW) {
                        const int st = t2 / (BW * 36), rem = t2 % (BW * 36), w = 1 + rem / 36, e = rem % 36;
                        const int i = k0 + st + w;
                        if (i < nrows) g.Lband[((size_t)i * W + w) * 36 + e] = ringL[(size_t)st * BW * 36 + rem];
                    }
                const int r0 = fr0;      // k0 mod RK, kept incrementally (a per-lane division by the
                fr0 = fr0 + R >= RK ? fr0 + R - RK : fr0 + R;  // runtime ring size spilled its magic number)
                for (int t2 = wtl; t2 < cnt * 36; t2 += NW) {
                    const int sl = r0 + t2 / 36;
                    g.Kinv[(size_t)k0 * 36 + t2] = ringK[(sl >= RK ? sl - RK : sl) * 36 + t2 % 36];
                }
                for (int t2 = wtl; t2 < cnt * 6; t2 += NW) {
                    const int sl = r0 + t2 / 6;
                    g.zb[(size_t)k0 * 6 + t2] = ringZ[(sl >= RK ? sl - RK : sl) * 6 + t2 % 6];
                }
            }
            // the staged row lands before the barrier (issued at the start of this phase; read at
            // the top of step k+2)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        lds_barrier();
        sk = (sk + 1 == W) ? 0 : sk + 1;
        sB = (sB + 1 == kBandStage) ? 0 : sB + 1;
        sW = (sW + 1 == kBandStage) ? 0 : sW + 1;
        kR = (kR + 1 == R) ? 0 : kR + 1;
        kRK = (kRK + 1 == RK) ? 0 : kRK + 1;
        oo = (oo == 0) ? oCl - 1 : oo - 1;
    }
    __syncthreads();  // drains every wave's flush stores: the backward pass reads them
    const bool failed = s_fail != 0;
    if (g.sep && !failed) {  // rows nsteps..nsteps+BW-1, blocks w <= row (later columns) and their right-hand sides
        const int i = ow + oo;  // separator row of the owned block (k = nsteps)
        if (own && oo <= BW - ow && i < BW) {
            double *dst = g.sep + ((size_t)i * W + ow) * 36 + oh;
            const double *pv = piv + (nsteps & 1) * 36 + oh;  // (nsteps, nsteps) carries wave 0's last update
#pragma unroll
            for (int j = 0; j < UE; ++j) dst[j] = (ow == 0 && oo == 0) ? pv[j] : t[j];
        }
        for (int t2 = tid; t2 < BW * 6; t2 += NT) g.sep[(size_t)BW * W * 36 + t2] = bwin[((sk + t2 / 6) % W) * 6 + t2 % 6];
    }
    return failed;
}

// Backward substitution x_k = z_k - Σ_w L_{k+w,k}ᵀ x_{k+w} for k = nsteps-1..0, by ONE wave (no
// barriers; L prefetched one step ahead). Rows nsteps..nsteps+BW-1 take x from `xsep` (a
// separator solved elsewhere) or do not exist (xsep == nullptr, nsteps == nrows). Row k is
// written to xp[k] (or xp[nf-1-k] for a reversed segment).
// Right-looking variant for bw <= 10 (one lane per (row, component) of the BW-row window, all
// in registers): once x_i is final, its 6 values are read from the owning lanes with
// v_readlane and every window row j = i-w applies z_j -= L_{i,j}ᵀ x_i at once. The chain per
// step is one readlane batch + one 6-term dot product; no LDS round trips.
// LX: x rows go to LDS (the caller copies them out) — a global store in the loop would make
// the compiler's vmcnt waits (loads and stores share the counter) drain the L prefetches.
template <int BW, bool LX = false>
__device__ __forceinline__ void band_backward_rl(const double *Lband, const double *zb, int nsteps, int nrows,
                                                 const double *xsep, double *xp, bool reversed, int nf, int lane) {
    constexpr int W = BW + 1, kPipe = 4;
    if (nsteps <= 0) return;
    const int G = lane / 6, r = lane % 6;      // lane group G holds the window row j ≡ G (mod BW)
    const bool act = lane < BW * 6;
    const int top = xsep ? min(nrows - 1, nsteps - 1 + BW) : nsteps - 1;
    // window rows top-BW+1..top: separator x (known) or z to be completed
    double zv = 0.0;
    if (act) {
        int j = top - ((top - G) % BW + BW) % BW;  // the row of this group in [top-BW+1, top]
        if (j >= 0) zv = j >= nsteps ? (xsep ? xsep[(j - nsteps) * 6 + r] : 0.0) : zb[(size_t)j * 6 + r];
    }
    // Load cursor: row li's L block for this lane's window row li - wl, wl = ((li-G-1) mod BW)+1,
    // stepped incrementally (wl cycles BW..1 as li decreases). Loads are unconditional from
    // clamped in-range addresses and masked afterwards, so the loop carries no branches.
    int li = top, wl = ((top - G - 1) % BW + BW) % BW + 1;
    double Lr[kPipe][6], zr[kPipe];
    bool lok[kPipe], zok[kPipe];               // masks applied when the values are consumed, so
    auto load_step = [&](double (&dst)[6], double &z, bool &okL, bool &okZ) {  // no load is waited on early
        const int jl = li - wl;
        okL = act && li >= 0 && jl >= 0 && jl < nsteps;
        const int base = (max(li, 0) * W + wl) * 36 + r;
#pragma unroll
        for (int m = 0; m < 6; ++m) dst[m] = Lband[base + m * 6];
        const int iz = li - BW;
        z = zb[min(max(iz, 0), nsteps - 1) * 6 + r];
        okZ = act && iz >= 0 && iz < nsteps;
        --li;
        wl = wl == 1 ? BW : wl - 1;
    };
#pragma unroll
    for (int u = 0; u < kPipe; ++u) load_step(Lr[u], zr[u], lok[u], zok[u]);
    int gi = top % BW;                          // group holding row i (final), uniform
    // whole kPipe batches (trailing steps with i < 0 are masked no-ops): no exits inside the
    // unrolled body, so the compiler can count the prefetches in flight exactly
    for (int ib = top; ib >= 0; ib -= kPipe) {
#pragma unroll
        for (int u = 0; u < kPipe; ++u) {
            const int i = ib - u;
            double x[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                const int src = gi * 6 + m;
                const int lo = __builtin_amdgcn_readlane(__double2loint(zv), src);
                const int hi = __builtin_amdgcn_readlane(__double2hiint(zv), src);
                x[m] = __hiloint2double(hi, lo);
            }
            const bool mine = act && G == gi && i >= 0;  // this group holds the final row i
            if (mine && i < nsteps) {
                const int row = reversed ? nf - 1 - i : i;
                if constexpr (LX) ((__attribute__((address_space(3))) double *)xp)[row * 6 + r] = zv;
                else xp[(size_t)row * 6 + r] = zv;
            }
            // z_j -= L_{i,j}ᵀ x_i for the window rows j < nsteps (masked to zero elsewhere);
            // the group that held row i takes row i-BW
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m) acc = fma(Lr[u][m], x[m], acc);
            const double znew = zok[u] ? zr[u] : 0.0;
            zv = (mine ? znew : zv) - (lok[u] ? acc : 0.0);
            load_step(Lr[u], zr[u], lok[u], zok[u]);
            gi = gi == 0 ? BW - 1 : gi - 1;
        }
    }
}

template <int BW>
__device__ __forceinline__ void band_backward(const double *Lband, const double *zb, int nsteps, int nrows, const double *xsep,
                              double *xp, bool reversed, int nf, double *xr, double *part, int lane) {
    constexpr int W = BW + 1;
    const int last = min(nrows - 1, nsteps - 1 + BW);  // highest row coupled to the segment
    if (xsep && lane < 6)
        for (int i = 0; i < BW && nsteps + i < nrows; ++i) xr[((nsteps + i) % W) * 6 + lane] = xsep[i * 6 + lane];
    wave_lds_sync();
    // L_{k+w,k} and z_k are loaded kPipe steps ahead into a register ring (static slots: the
    // step loop is unrolled by kPipe), so their L2 latency hides behind kPipe steps of work
    constexpr int kMaxB = (BW * 6 + 63) / 64 > 0 ? (BW * 6 + 63) / 64 : 1;
    constexpr int kPipe = kMaxB == 1 ? 6 : 2;  // register budget: 12 f64 per slot per lane at bw <= 10
    double Lr[kPipe][kMaxB][6], zr[kPipe];
    auto load_step = [&](int k, double (&dst)[kMaxB][6], double &z) {
        const int wmax = (k >= 0) ? min(BW, last - k) : 0;
#pragma unroll
        for (int q = 0; q < kMaxB; ++q) {
            const int t = q * 64 + lane;
            const int w = 1 + t / 6, r = t % 6;
            const bool ok = t < wmax * 6;
            const double *L = Lband + ((size_t)(k + w) * W + w) * 36;
#pragma unroll
            for (int m = 0; m < 6; ++m) dst[q][m] = ok ? L[m * 6 + r] : 0.0;
        }
        z = (lane < 6 && k >= 0) ? zb[(size_t)k * 6 + lane] : 0.0;
    };
#pragma unroll
    for (int u = 0; u < kPipe; ++u) load_step(nsteps - 1 - u, Lr[u], zr[u]);
    for (int kb = nsteps - 1; kb >= 0; kb -= kPipe) {
#pragma unroll
        for (int u = 0; u < kPipe; ++u) {
            const int k = kb - u;
            if (k < 0) break;
            const int wmax = min(BW, last - k);
#pragma unroll
            for (int q = 0; q < kMaxB; ++q) {
                const int t = q * 64 + lane;
                if (t < wmax * 6) {
                    const int w = 1 + t / 6, r = t % 6, i = k + w;
                    const double *x = xr + (i % W) * 6;
                    double s = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) s += Lr[u][q][m] * x[m];
                    part[w * 6 + r] = s;
                }
            }
            wave_lds_sync();
            if (lane < 6) {
                double v = zr[u];
                for (int w = 1; w <= wmax; ++w) v -= part[w * 6 + lane];
                xr[(k % W) * 6 + lane] = v;
                xp[(size_t)(reversed ? nf - 1 - k : k) * 6 + lane] = v;
            }
            wave_lds_sync();
            load_step(k - kPipe, Lr[u], zr[u]);  // refill this slot kPipe steps ahead
        }
    }
}

// Streamed back substitution of the two-sided register-window band kernel (bw >= 11), both
// segments at once: wave 0 runs segment 0, wave 1 segment 1, and the other waves stream the rows
// of L they are about to need into LDS, CH rows a chunk, double-buffered with one workgroup
// barrier per chunk (the one-wave band_backward waited on its L2 prefetches, two steps ahead at
// ≈ 2.2 k cycles a step). Right-looking: the wave keeps the z values of the BW rows below the
// current row i in registers (lane entry t = q·64 + lane: ring slot t/6 = row mod BW, component
// t%6); once row i is final, x_i is broadcast by v_readlane and every lane removes
// L_{i,j}ᵀ x_i from its row j = i − w in one 6-term product, reading row i of L (contiguous in
// Lband: blocks (i, i−1) .. (i, i−BW)) from the staged chunk; row i's slot then takes row i−BW
// (z_{i−BW} staged with the row). Rows nsteps.. of a segment are the separator (x given).
struct BackSeg {
    const double *Lband, *zb, *xsep;  // segment's L rows and z, its separator x [BW][6]
    int nsteps;                       // eliminated rows (x written for rows < nsteps)
    int nrows;                        // rows of the segment's band (separator included)
    bool reversed;                    // row i is pose nf-1-i
};
__host__ __device__ constexpr int bstream_ch(int bw) { return bw <= 24 ? 4 : 3; }
__host__ __device__ constexpr size_t bstream_doubles(int bw) {
    return (size_t)4 * bstream_ch(bw) * ((size_t)bw * 36 + 6);  // [2 buffers][2 segments][CH][RS]
}
template <int BW, int NT, int CH>
__device__ __forceinline__ void band_backward_stream(const BackSeg (&sg)[2], int nf, double *xl, double *buf) {
    constexpr int RS = BW * 36 + 6, NQ = (BW * 6 + 63) / 64;  // buf: [2][2][CH][RS]
    constexpr int SEG = CH * RS;                       // doubles of one segment's chunk
    constexpr int PN = NT - 128, NP2 = SEG;            // producer threads; double2 pieces of a chunk
    constexpr int PER = (NP2 + PN - 1) / PN;           // pieces per producer thread
    static_assert(RS % 2 == 0 && PN > 0, "staged rows are double2 pieces");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int last0 = min(sg[0].nrows - 1, sg[0].nsteps - 1 + BW), last1 = min(sg[1].nrows - 1, sg[1].nsteps - 1 + BW);
    const double *L0 = sg[0].Lband, *L1 = sg[1].Lband, *z0 = sg[0].zb, *z1 = sg[1].zb;
    const int nchunk = (max(last0, last1) + CH) / CH;  // chunk c: rows last - c·CH .. last - c·CH - CH + 1
    // producers: both segments' rows of chunk c, loaded into registers one chunk period before
    // they are stored (the loads stay in flight across the LDS-only barrier)
    const int pt = tid - 128;
    double2 v[PER];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int e = pt + j * PN;                 // piece: segment e / (SEG/2), offset 2·(e % (SEG/2))
            v[j] = make_double2(0.0, 0.0);
            if (e < NP2) {
                const int s = e / (SEG / 2), o2 = 2 * (e % (SEG / 2)), u = o2 / RS, o = o2 % RS;
                const int i = (s ? last1 : last0) - (c * CH + u);
                if (i >= 0) {
                    const double *Lb = s ? L1 : L0, *zb = s ? z1 : z0;  // (no runtime index into sg: stack)
                    if (o < BW * 36) v[j] = *(const double2 *)(Lb + ((size_t)i * (BW + 1) + 1) * 36 + o);
                    else if (i - BW >= 0) v[j] = *(const double2 *)(zb + (size_t)(i - BW) * 6 + (o - BW * 36));
                }
            }
        }
    };
    auto store_chunk = [&](int c) {
        double2 *dst = (double2 *)(buf + (size_t)(c & 1) * 2 * SEG);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int e = pt + j * PN;
            if (e < NP2) dst[e] = v[j];
        }
    };
    // ---- consumer state: the ring of the segment's z (rows last-BW+1 .. last at the start)
    const bool cons = wv < 2, s1 = wv == 1;
    const double *gz = s1 ? z1 : z0, *gx = s1 ? sg[1].xsep : sg[0].xsep;
    const bool grev = s1 ? sg[1].reversed : sg[0].reversed;
    const int last = s1 ? last1 : last0, ns = s1 ? sg[1].nsteps : sg[0].nsteps;
    const int lastu = __builtin_amdgcn_readfirstlane(last);  // (per wave)
    double z[NQ];
    int ws[NQ];                                        // w = i - j of the entry's row j at step i
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int t = q * 64 + lane, sl = t / 6, r = t % 6;
        z[q] = 0.0;
        ws[q] = 0;
        if (cons && t < BW * 6) {
            const int j = last - (((last - sl) % BW) + BW) % BW;
            ws[q] = last - j;
            if (j >= ns) z[q] = gx[(j - ns) * 6 + r];
            else if (j >= 0) z[q] = gz[(size_t)j * 6 + r];
        }
    }
    if (wv >= 2) load_chunk(0);
    __syncthreads();  // (the separator x sits in the region the chunks overwrite)
    if (wv >= 2) {
        store_chunk(0);
        if (1 < nchunk) load_chunk(1);
    }
    lds_barrier();
    for (int c = 0; c < nchunk; ++c) {
        if (wv >= 2) {
            if (c + 1 < nchunk) store_chunk(c + 1);
            if (c + 2 < nchunk) load_chunk(c + 2);
        } else if (cons) {
            const double *B = buf + ((size_t)(c & 1) * 2 + wv) * SEG;
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int i = lastu - (c * CH + u);  // (uniform: scalar slot arithmetic below)
                if (i < 0) break;
                const double *Lr = B + u * RS;
                // the step's L reads first: they do not depend on x_i (a slot whose row is final
                // this step reads block BW, row i-BW's, and the staged z_{i-BW})
                double Lv[NQ][6], zr[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int r = (q * 64 + lane) % 6, w = ws[q] == 0 ? BW : ws[q];
#pragma unroll
                    for (int m = 0; m < 6; ++m) Lv[q][m] = Lr[(w - 1) * 36 + m * 6 + r];
                    zr[q] = Lr[BW * 36 + r];
                }
                const int si = i % BW;
                double x[6];
#pragma unroll
                for (int r = 0; r < 6; ++r) {  // x_i from the lanes of row i's slot
                    const int t = si * 6 + r, q = t >> 6, ln = t & 63;
                    double v = z[0];
#pragma unroll
                    for (int qq = 1; qq < NQ; ++qq) v = q == qq ? z[qq] : v;
                    x[r] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), ln),
                                            __builtin_amdgcn_readlane(__double2loint(v), ln));
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int t = q * 64 + lane, r = t % 6;
                    const bool fin = ws[q] == 0;   // row i: final; the slot takes row i - BW
                    const int w = fin ? BW : ws[q], j = i - w;
                    if (fin && t < BW * 6 && i < ns) xl[(size_t)(grev ? nf - 1 - i : i) * 6 + r] = z[q];
                    double acc = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) acc = fma(Lv[q][m], x[m], acc);
                    const double zz = fin ? zr[q] : z[q];
                    z[q] = (j >= 0 && j < ns) ? zz - acc : zz;
                    ws[q] = w - 1;
                }
            }
        }
        lds_barrier();
    }
}

template <int BW>
__global__ __launch_bounds__(band_nt(BW)) void k_rcs_factor_band(Dev d0) {
    TRIAL_SLOT(blockIdx.y)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const BandSeg g{d.Bd, d.bs, d.Lband, d.Kinv, d.zb, d.nf, d.nf, nullptr};
    const bool fail = band_forward<BW>(g, lds, d.ring) || diag_fail(d);
    if (threadIdx.x == 0) *d.solve_okp = fail ? 0 : 1;
    if (!fail && threadIdx.x < 64) {
        double *col, *piv, *bwin, *Lcol, *Kv, *xr, *part, *ys, *ringL, *ringK, *ringZ;
        band_lds<BW>(lds, d.ring, col, piv, bwin, Lcol, Kv, xr, part, ys, ringL, ringK, ringZ);
        if constexpr (BW >= 1 && BW * 6 <= 64) band_backward_rl<BW>(d.Lband, d.zb, d.nf, d.nf, nullptr, d.xp, false, d.nf, threadIdx.x);
        else band_backward<BW>(d.Lband, d.zb, d.nf, d.nf, nullptr, d.xp, false, d.nf, xr, part, threadIdx.x);
    }
    __syncthreads();
    pose_update_wg<band_nt(BW)>(d, fail);  // applied even after a failed solve, with the previous x_p (A13)
}

// Two-sided ("twisted") banded LDLᵀ: workgroup 0 eliminates block rows 0..m-1 top-down,
// workgroup 1 eliminates rows nf-1..m+BW bottom-up (as the top-down elimination of the
// block-reversed matrix Bd2), concurrently on two CUs. The two eliminated sets do not couple
// (they are > BW blocks apart), so their Schur updates of the BW-block separator m..m+BW-1
// add: S_sep = W0 + W1 − A_sep. The workgroup that finishes second solves the separator
// (block LDLᵀ on its packed lower triangle, no pivoting: a zero pivot fails the solve as
// SimplicialLDLT does) and runs both back substitutions on two waves. Half the serial chain.
template <int BW>
__device__ __forceinline__ void k_rcs_factor_twisted_body(const Dev &d) {
    constexpr int W = BW + 1, NT = band_nt(BW), NS = 6 * BW;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int s_last, s_sfail;
    const int seg = blockIdx.x, tid = threadIdx.x;
    const size_t sep_stride = (size_t)BW * W * 36 + (size_t)BW * 6;
    const int m = d.tw_m, n1 = d.nf - BW - d.tw_m;
    const BandSeg g = seg == 0 ? BandSeg{d.Bd, d.bs, d.Lband, d.Kinv, d.zb, d.nf, m, d.tw_sep}
                               : BandSeg{d.Bd2, d.bs2, d.Lband2, d.Kinv2, d.zb2, d.nf, n1, d.tw_sep + sep_stride};
    const bool fail = band_forward<BW>(g, lds, d.ring) || diag_fail(d);
    // hand-off (MI355X_MICROARCH.md §Workgroup dispatch…, counter form): every wave drains its
    // L / z / separator stores, one agent release by lane 0, then the arrival counter; the
    // workgroup whose add returns 1 is last and acquires once before reading the other's data
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_store(&d.tw_fail[seg], fail ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = __hip_atomic_fetch_add(d.tw_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == 1 ? 1 : 0;
        if (old == 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(d.tw_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
            s_sfail = (__hip_atomic_load(&d.tw_fail[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
                       __hip_atomic_load(&d.tw_fail[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 1 : 0;
        }
    }
    __syncthreads();
    if (!s_last) return;
    if (!s_sfail) {
    // merge layout (twisted_merge_doubles) from LDS offset 0: the band windows are dead, both
    // separators having been exported to global memory before the arrival
    double *xl = lds;                                  // [nf][6] x_p staging
    double *Ls = lds + (size_t)d.nf * 6;               // [BW(BW-1)/2][36] L_IP, I > P (block I(I-1)/2 + P)
    double *Kp = Ls + (size_t)BW * (BW - 1) / 2 * 36;  // [BW][36] pivot inverses S_PP⁻¹ (after the sweep)
    double *colA = Kp + (size_t)BW * 36;               // [2][BW][36] pivot column A_IP (step parity)
    double *Sp = colA + (size_t)2 * BW * 36;           // [BW][36] pivot blocks S_PP
    double *rhs = Sp + (size_t)BW * 36, *xs0 = rhs + NS, *xsr = xs0 + NS;  // [NS] each
    // Separator system S_sep (lower block (I, J), I >= J, w = I - J < BW) by right-looking block
    // LDLᵀ with the blocks held in registers: block (I, J) is owned by UPB threads (UR rows each,
    // the band kernel's split) for the whole elimination, so a trailing update reads only its
    // L_IP rows and A_JP from LDS (54 reads for 108 FMA at UR = 3) and writes nothing back. Per
    // pivot P two barriers: the owners of column P factor S_PP LDLᵀ in their own registers and
    // solve their rows of L_IP = A_IP S_PP⁻¹; the owners of the trailing blocks apply
    // A_IJ -= L_IP A_JPᵀ and publish column P + 1 into the other parity buffer (the right-hand
    // side y_R -= L_RP y_P on the side). The pivot inverses the back substitution needs are formed
    // after the sweep, all at once (a wave-0 inverse per step was one more barrier and ≈ 1 k cycles
    // on the chain). No pivoting: a zero LDLᵀ pivot fails the solve as SimplicialLDLT does. (Round 5 held the system as a packed scalar triangle in LDS and
    // swept it with one thread per entry: runtime divisions + 12 LDS reads per FMA-6 entry;
    // ≈ 28 % of the C3R factorisation.)
    const double *W0 = d.tw_sep, *W1 = d.tw_sep + sep_stride;
    constexpr int UR = band_ur(BW), UPB = 6 / UR, UE = UR * 6, NB = BW * (BW + 1) / 2;
    static_assert(UPB * NB <= NT, "one owned separator (part) block per thread");
    const bool own = tid < UPB * NB;
    int oI = 0, oJ = 0;
    if (own) {
        const int b = tid / UPB;
        while ((oI + 1) * (oI + 2) / 2 <= b) ++oI;
        oJ = b - oI * (oI + 1) / 2;
    }
    const int oh = (tid % UPB) * UR;  // first row of the owned part
    double t[UE];
    if (own) {
        const int w = oI - oJ;
#pragma unroll
        for (int r = 0; r < UR; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const int a = oh + r;
                const double w0 = W0[((size_t)oI * W + w) * 36 + a * 6 + c];
                t[r * 6 + c] = w0 + W1[((size_t)(BW - 1 - oJ) * W + w) * 36 + c * 6 + a] -
                               d.Bd[((size_t)(m + oI) * W + w) * 36 + a * 6 + c];
            }
        // column 0: the first pivot block / pivot column
        if (oJ == 0) {
            double *dst = oI == 0 ? Sp : colA + (size_t)oI * 36;
#pragma unroll
            for (int j = 0; j < UE; ++j) dst[oh * 6 + j] = t[j];
        }
    }
    for (int q = tid; q < NS; q += NT) {
        const int i = q / 6, a = q % 6;
        rhs[q] = W0[(size_t)BW * W * 36 + i * 6 + a] + W1[(size_t)BW * W * 36 + (BW - 1 - i) * 6 + a] -
                 d.bs[(size_t)(m + i) * 6 + a];
    }
    if (tid == 0) s_sfail = 0;
    __syncthreads();
    for (int P = 0; P < BW; ++P) {
        const double *colP = colA + (size_t)(P & 1) * BW * 36;
        if (own && oJ == P && oI > P) {  // rows oh..oh+UR-1 of L_IP = A_IP S_PP⁻¹ (S symmetric: S⁻¹ a_r)
            const double *S = Sp + P * 36;
            double s[21], dv[6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) s[ltri(i, j)] = S[i * 6 + j];
            bool zp = false;  // (a zero pivot is reported by the inverses below)
            ldl6_inplace(s, dv, zp);
            double *L = Ls + ((size_t)oI * (oI - 1) / 2 + P) * 36 + oh * 6;
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                double x[6];
#pragma unroll
                for (int c = 0; c < 6; ++c) x[c] = t[r * 6 + c];
                ldl6_solve(s, dv, x);
#pragma unroll
                for (int c = 0; c < 6; ++c) L[r * 6 + c] = x[c];
            }
        }
        __syncthreads();
        if (own && oJ > P) {  // A_IJ -= L_IP A_JPᵀ, then column P + 1 published
            const double *L = Ls + ((size_t)oI * (oI - 1) / 2 + P) * 36 + oh * 6;
            const double *Aj = colP + (size_t)oJ * 36;
            double l[UE];
#pragma unroll
            for (int j = 0; j < UE; ++j) l[j] = L[j];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double a[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) a[q] = Aj[c * 6 + q];
#pragma unroll
                for (int r = 0; r < UR; ++r) {
                    double acc = 0.0;
#pragma unroll
                    for (int q = 0; q < 6; ++q) acc = fma(l[r * 6 + q], a[q], acc);
                    t[r * 6 + c] -= acc;
                }
            }
        }
        {   // y_R -= L_RP y_P for the trailing rows (threads past the owners first)
            const int q = NT - 1 - tid, R = (P + 1) * 6 + q;
            if (q >= 0 && R < NS) {
                const double *L = Ls + ((size_t)(R / 6) * (R / 6 - 1) / 2 + P) * 36 + (R % 6) * 6;
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c < 6; ++c) acc = fma(L[c], rhs[P * 6 + c], acc);
                rhs[R] -= acc;
            }
        }
        if (own && oJ == P + 1) {
            double *dst = oI == P + 1 ? Sp + (P + 1) * 36 : colA + ((size_t)((P + 1) & 1) * BW + oI) * 36;
#pragma unroll
            for (int j = 0; j < UE; ++j) dst[oh * 6 + j] = t[j];
        }
        __syncthreads();
    }
    for (int P = tid >> 6; P < BW; P += NT / 64) {  // S_PP⁻¹, one pivot block per wave
        bool f = false;
        const double I = ldl_inverse6(Sp + P * 36, rhs, tid & 63, f);
        if ((tid & 63) < 36) Kp[P * 36 + (tid & 63)] = I;
        if (f && (tid & 63) == 0) s_sfail = 1;
    }
    __syncthreads();
    if (!s_sfail) {
    // back substitution x_P = S_PP⁻¹ y_P − Σ_{I>P} L_IPᵀ x_I, right-looking: x_I is final once the
    // blocks below it are done, and its contribution is removed from every P < I in one pass.
    // x_sep in both segment orders: rows m+i for segment 0, reversed rows n1+i = original
    // m+BW-1-i for segment 1
    for (int q = tid; q < NS; q += NT) {
        const int P = q / 6, c = q % 6;
        double x = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) x = fma(Kp[P * 36 + c * 6 + r], rhs[P * 6 + r], x);
        xs0[q] = x;
    }
    __syncthreads();
    for (int I = BW - 1; I >= 1; --I) {
        if (tid < I * 6) {
            const int P = tid / 6, c = tid % 6;
            const double *L = Ls + ((size_t)I * (I - 1) / 2 + P) * 36 + c;
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) acc = fma(L[r * 6], xs0[I * 6 + r], acc);
            xs0[tid] -= acc;
        }
        __syncthreads();
    }
    for (int q = tid; q < NS; q += NT) {
        xl[(size_t)m * 6 + q] = xs0[q];
        xsr[q] = xs0[(BW - 1 - q / 6) * 6 + q % 6];
    }
    __syncthreads();
    if constexpr (BW * 6 <= 64) {
        if (tid < 64) band_backward_rl<BW, true>(d.Lband, d.zb, m, d.nf, xs0, xl, false, d.nf, tid);
        else if (tid < 128) band_backward_rl<BW, true>(d.Lband2, d.zb2, n1, d.nf, xsr, xl, true, d.nf, tid - 64);
    } else {
        const BackSeg sg[2] = {{d.Lband, d.zb, xs0, m, d.nf, false}, {d.Lband2, d.zb2, xsr, n1, d.nf, true}};
        band_backward_stream<BW, NT, bstream_ch(BW)>(sg, d.nf, xl, Ls);
    }
    __syncthreads();
    for (int t = tid; t < d.nf * 6; t += NT) d.xp[t] = xl[t];
    }  // separator solved
    }  // both segments eliminated
    __syncthreads();
    if (tid == 0) *d.solve_okp = s_sfail ? 0 : 1;
    pose_update_wg<NT>(d, s_sfail != 0);  // applied even after a failed solve, with the previous x_p (A13)
}

template <int BW>
__global__ __launch_bounds__(band_nt(BW)) void k_rcs_factor_twisted(Dev d0) {
    if constexpr (BW >= 1) {  // (the host never selects bw 0)
        TRIAL_SLOT(blockIdx.y)
        k_rcs_factor_twisted_body<BW>(d);
    }
}

}  // namespace plba
