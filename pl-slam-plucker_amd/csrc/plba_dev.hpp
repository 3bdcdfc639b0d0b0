// plba_dev.hpp — what every kernel of the LM step shares: constants, the device control block
// (Ctrl), the window (Dev) and its per-slot views, block reductions, in-launch hand-offs, the
// kernel guards.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plba.h"
#include "plba_math.hpp"

namespace plba {

constexpr int kBlock = 256;
constexpr int kLmBlock = 64;  // landmark-parallel kernels: 24k landmarks at C3 -> 375 workgroups, not 94
constexpr int kChunk = 256;  // Schur triples per assembly wave (4 per lane)
constexpr int kTraceCap = 64;
constexpr int kTile = 32;   // RCS factorisation tile (dense fallback)
constexpr int kBandMax = 27; // widest envelope (in pose blocks) the register-window factorisation holds
constexpr int kBandNT = 768; // threads of the banded factorisation workgroup (bw <= 24)
// rows of a band block one worker owns in registers (plba_band.hpp band_forward): whole 6x6
// blocks at 512 threads (256 VGPRs), half blocks when more, smaller waves are configured
// Bandwidths 25..27 need more owned blocks than 704 worker threads hold at three rows each: they
// run 512-thread workgroups owning whole blocks (256 VGPRs, no scratch; at bw 23 that form was 6 %
// slower than 768 threads at half blocks)
__host__ __device__ constexpr int band_nt(int bw) { return bw <= 24 ? kBandNT : 512; }
__host__ __device__ constexpr int band_ur(int bw) { return band_nt(bw) <= 512 ? 6 : 3; }
// Speculative trials (DESIGN §2 "Speculative trials"): a step may evaluate up to kMaxSpec damped
// trials of one linearisation at once — λ, λ·ν, λ·ν·2ν, ... (exactly the λ sequence g2o's
// Levenberg loop walks after rejections) — in trial slots 0..W-1 (blockIdx.y of the trial
// kernels); k_decide consumes them in order, as the sequential loop would have evaluated them.
// State-like arrays rotate through kNB buffers so that no slot overwrites the current state,
// the last consumed χ² or the last successful solve.
constexpr int kMaxSpec = 4;
constexpr int kNB = kMaxSpec + 1;

// The LM loop a step graph runs (Ctrl::hlm, held there as a plain int32_t). The values are part of
// Ctrl's layout; plba_hlm_lba (plba.hip) maps the public PLBA_HLM_* constants onto them.
enum LmKind : int32_t {
    kLmG2o = 0,           // g2o Levenberg
    kLmLbaPlucker = 1,    // levMarquardtOptimizationLBAForPluker
    kLmGba = 2,           // levMarquardtOptimizationGBA
    kLmLbaEndpoints = 3   // levMarquardtOptimizationLBA
};
// The questions the kernels ask of it. k_rcs_chunk, k_rcs_chunk_h, pose_update_wg and k_lm_solve
// compare with the enumerators instead: with the predicates there, the instruction streams of those
// kernels (and of every factorisation kernel that ends in pose_update_wg) differed from the
// bare-integer form's (another register allocation and VGPR count).
// the hand-rolled LM (scalar residuals, Marquardt damping, se(3) pose update, its own decision)
__host__ __device__ constexpr bool lm_hand_rolled(int32_t k) { return k != kLmG2o; }
// lines are 6-dim endpoint blocks (line3D), not 4-dim orthonormal ones
__host__ __device__ constexpr bool lm_endpoint_lines(int32_t k) { return k >= kLmGba; }
// the landmark factor is the signed LDLᵀ (lm_chol's `sgn`)
__host__ __device__ constexpr bool lm_signed_ldlt(int32_t k) { return k == kLmLbaPlucker; }

// Device-resident LM control block: the g2o optimize()/solve() loop runs as a state machine
// advanced by k_decide, so the host only replays a captured "step" graph and polls this block.
struct Ctrl {
    double lambda, ni, currentChi, tempChi, rho, scale, maxdiag;
    double chi2_start, lambda_start;
    double chi2_final[2];
    int32_t qmax, accept, broke;
    int32_t solve_ok[kMaxSpec];                        // per trial slot: the factorisation succeeded
    int32_t last_ok, chi_src;                          // xp/xl buffer of the last successful consumed solve,
                                                       // χ² buffer of the last consumed trial (or linearisation)
    int32_t spec_w, spec_sticky;                       // trial slots of the next step; a rejection seen in
                                                       // this optimize() call
    int32_t stage, n_stages, iter, need_iter;        // schedule position
    int32_t all_done, switch_pending, robust, level;
    int32_t max_iters[2], iters_done[2];
    int32_t stage_robust[2], stage_level[2], stage_classify[2];
    int32_t max_trials, ntrace, any_active, cur;      // cur: which state buffer is current
    int32_t steps;                                     // step graphs that did work (diagnostic)
    int32_t dev_error;                                 // a bounded in-kernel wait timed out
    // hand-rolled LM (plba_hlm_lba, src/mapHandler.cpp:1618-2332): the same step graph with the
    // scalar-residual linearisation, Marquardt damping, se(3) pose update and its own decision
    int32_t hlm;                                       // LmKind: which LM loop the step graph runs
    int32_t hlm_lin, hlm_solves, hlm_acc;              // linearisations, solves, applied updates
    int32_t pad[2];
    double hlm_lambda0, hlm_k, hlm_homog, hlm_minerr, hlm_minchg;
    double hlm_nobs;                                   // err divisor (0 = the reference's Npt_obs+Nls_obs)
    double hlm_nobs2;                                  // kLmLbaEndpoints: err divisor of the later linearisations
                                                       // (Npt+Nls, src/mapHandler.cpp:2796); others: not read
    double err_prev, dx2;                              // err of the previous linearisation, ‖DX‖² of the last solve
};

// All device pointers of one window (passed by value to every kernel).
struct Dev {
    int32_t n_kf, n_pt, n_ln, n_lm, Ep, El, E, nf, n;
    int32_t corrected, n_lin_blocks, n_lm_blocks, n_kf_blocks, nblk, ntiles;
    int32_t solve_lds_n;                // dense solve: y in LDS up to this n (kSolveLdsN; tests lower it)
    int32_t n_lms_blocks;               // k_lm_solve workgroups (kLmLanes lanes per landmark)
    Cam cam;
    double huber_pt, huber_ln, tau;
    // state
    // state buffers: Tb[ctrl->cur] is the current estimate; trial slot s writes Tb[(cur+1+s) % nbs];
    // accepting slot s moves ctrl->cur there (g2o's push/pop/discardTop without a copy)
    double *Tb[kNB], *T_init;           // [n_kf][12]
    double *Xb[kNB], *X_init;           // [n_lm][4]
    double *xk[kNB];                    // [n_kf][6] se(3) pose vectors X_i of the hand-rolled LM
    double *XL[kNB];                    // [n_ln_g][6] GBA line3D endpoints, reference (global) line order
    double *Hl6, *bl6;                  // [n_ln][21], [n_ln][6] GBA line blocks (packed lower 6x6)
    int32_t *ln_gidx;                   // [n_ln] device line -> reference (global) line index
    double *Lpb[kNB];                   // [n_ln][8]: Plücker vector (6) of each line at Xb[i]
                                        //   (k_line_pluker at schedule start, then k_lm_solve)
    // solve / χ² buffers: slot s writes xpb/xlb[(last_ok+1+s) % nbx] and chi2b[(chi_src+1+s) % nbx]
    // (nbx = 1 without speculation: one buffer, as g2o's _x and the edges' _error)
    double *xpb[kNB], *xlb[kNB], *chi2b[kNB];
    int32_t nbs, nbx;                   // state buffers (spec_max + 1), solve / χ² buffers
    int32_t spec_max, spec_policy;      // trial slots captured per step; when to use them (kSpec*)
    // ---- resolved per trial slot by slot_view() (trial kernels) / cur_view() (others)
    int32_t slot;
    double lam;                         // λ of this slot
    double *Tc, *Tt, *Xc, *Xt, *Lpc, *Lpt, *xkc, *xkt, *XLc, *XLt;  // current / trial state of the slot
    double *xp_prev, *xl_prev;          // solution of the last successful solve (used when this one fails)
    int32_t *solve_okp;                 // &ctrl->solve_ok[slot]
    int32_t *cnt_rcs;                   // [spec_max][nblk] arrival counters of the RCS blocks
    int32_t *kf_hidx;                   // [n_kf]
    // edges, landmark-major CSR order (points first, then lines)
    int32_t *e_lm, *e_kf, *e_hidx;      // [E]
    double *e_obs;                      // [E][4]
    double *e_info;                     // [E]
    uint8_t *e_level, *e_active;        // [E]
    int32_t *lm_off;                    // [n_lm+1]
    uint8_t *lm_active;                 // [n_lm]
    int32_t *pe_off, *pe_list;          // free-pose-major edge lists [nf+1], [..]
    // linearisation
    double *A, *cvec, *B, *chi2_last;   // [E][12], [E][2], [E][8], [E] (chi2_last: this slot's χ² buffer)
    double *Hpp, *bp;                   // [nf][36], [nf][6]
    double *Hll, *bl;                   // [n_lm][10], [n_lm][4]
    // Schur
    double *Z, *q, *xl;                 // [E][8], [E][2], [n_lm][4]
    // reduced camera system
    int32_t *blk_i1, *blk_i2, *blk_off; // [nblk], [nblk], [nblk+1]
    int32_t *trip;                      // [T][2]
    int32_t nch;                        // triple chunks (<= kChunk triples, one block each)
    int32_t *ch_blk, *ch_off;           // [nch], [nch+1] (triple range)
    int32_t *blk_ch;                    // [nblk+1] chunk range of each block
    double *ch_part;                    // [nch][42]  partial block sums (36) + b_s sums (6)
    double *Ad, *bs, *xp, *Wbuf;        // [n*n], [n], [n], [n*(kTile+1)] (W, then y of the dense path)
    int32_t *tile_first;                // [ntiles] first nonzero column tile of each row tile
    int32_t *tile_last;                 // [ntiles] last row tile whose envelope reaches column tile K
    // block-band storage (used when the envelope bandwidth bw <= kBandMax)
    int32_t bw, band_mode;              // bandwidth in pose blocks; 1 = banded factorisation
    int32_t dense_mfma;                 // dense RCS on many workgroups + MFMA (plba_dense.hpp)
    int32_t ring;                       // steps of L / S^-1 / z staged in LDS between global flushes
    int32_t *first_blk;                 // [nf] first block column of each block row (lower)
    double *Bd;                         // [nf][bw+1][36]  block (i, i-w), row-major 6x6
    double *Lband;                      // [nf][bw+1][36]  L_{i,i-w} (w >= 1)
    double *Kinv;                       // [nf][36]        S_k^{-1}
    double *zb;                         // [nf][6]         z = D_B^{-1} y
    // reductions
    double *part_chi2;                  // [n_lin_blocks]
    double *wg_red, *grp_red;           // folded init: [nred][3], [ceil(nred/64)][3] (χ², max, any)
    int32_t *part_any;                  // [n_lm_blocks] block has an active landmark
    double *part_max;                   // [nf + n_lm_blocks] (landmark part from nf on)
    double *part_lm, *part_lms;         // [n_lms_blocks] trial χ² partials, scale partials (k_lm_solve)
    double *part_ps;                    // [n_ps] pose part of Σx(λx+b) (one slot per factorisation workgroup)
    int32_t n_ps;                       // max(n_kf_blocks, bcr_N)
    int32_t fold;                       // 1: k_rcs_finalize / k_decide run as the tails of the
                                        //    preceding launch (last arriver); 0 when sharded
    int32_t fold_init;                  // 1: k_iter_init runs as the tail of k_iter_reduce
    int32_t *cnt;                       // [2 + nblk + nf] arrival counters: lm_solve, iter_reduce, per RCS block, per pose
    int32_t *h_kf;                      // [nf] keyframe of each free-pose Hessian index
    Ctrl *ctrl;
    plba_iter_trace *trace;             // [kTraceCap] per-iteration records written by k_decide
    // sharded windows: the arrays the ranks sum with one all-reduce each
    int32_t sharded, nranks, rank;
    int32_t n_lm_g, E_g;                // whole-window landmark / edge counts
    // Out-of-place (send *_loc -> receive) so that replaying a step whose kernels were guarded
    // off re-reduces unchanged partials and leaves the totals intact.
    double *red_iter, *red_iter_loc;    // [nf*43 + 2 + nranks] (sharded [nf*13 + ...], see Hdg): Hpp | b_p | #active edges | χ² | active | lm max per rank
    double *red_rcs, *red_rcs_loc;      // [nblk*36 + nf*6]: Σ A₁ᵀZ₁Z₂ᵀA₂ per block | Σ A_eᵀq_e per pose
    // sharded, all-gather exchange (xg_P > 0): each rank's partial RCS is nonzero only on the
    // block rows of its keyframe range; xg_rng[4r..4r+3] = rank r's two runs of red_rcs
    // (block run start, length | right-hand-side run start, length, in doubles), xg_send = this
    // rank's runs packed (P doubles; host transport: its slot of an R x P array), xg_recv = R x P
    double *xg_send, *xg_recv;
    int64_t *xg_rng;
    int64_t xg_P;
    int32_t xg_host;
    double *red_dec, *red_dec_loc;      // [3]: trial χ² | landmark part of Σx(λx+b) | failed solves (sharded)
    double *Hpp_w, *bp_w;               // where pose_combine writes (== Hpp, bp unless sharded)
    // sharded: the iteration all-reduce carries only diag(Hpp) | b_p | active counts | scalars
    // (nf·13 + 2 + R); this rank's full partial Hpp (Hpp_w, local) rides in the RCS exchange inside
    // its diagonal blocks (k_rcs_blockpart), so Hpp is nullptr and Hdg holds the summed diagonals
    double *Hdg, *Hdg_w;                // [nf][6] (sharded only)
    double *pose_part;                  // [nf][kPoseParts][kPP] partial Σ AᵀA (upper), Σ Aᵀc, #active edges
    double *pact, *pact_w;              // [nf] active edges of each free pose (0 = vertex inactive in g2o)
    int32_t *lm_gpos, *e_gpos;          // local landmark / edge -> whole-window position
    double *gat;                        // [n_lm_g*4 + 3*E_g] final gather buffer
    // two-sided banded factorisation (k_rcs_factor_twisted)
    int32_t cl;                         // column-lane factorisation (plba_band_cl.hpp)
    int32_t diag;                       // PLBA_DIAG test bits (0 in every real run): 64 times out every
                                        // BCR hand-off (bcr_poll), 128 fails factorisations by λ (diag_fail)
    int32_t twisted, tw_m;              // enabled; rows 0..tw_m-1 top-down, separator tw_m..tw_m+bw-1
    double *Bd2, *bs2;                  // block-reversed band / rhs (row r' = nf-1-i)
    double *Lband2, *Kinv2, *zb2;       // factors of the bottom segment (reversed numbering)
    double *tw_sep;                     // [2][bw][bw+1][36] + [2][bw][6] separator windows
    int32_t *tw_fail, *tw_count;        // [2] per-segment failure, arrival counter
    // block cyclic reduction over super-rows of bw pose blocks (plba_bcr.hpp)
    int32_t bcr, bcr_N;                 // enabled; super-rows (= workgroups of the launch)
    int32_t bcr_fused;                  // back substitution + pose update in the forward launch (1) or
                                        // a second launch, k_rcs_bcr_back (0: PLBA_BCR_SPLIT=1)
    double *bcr_pub;                    // [N][bcr_pub_doubles(bw)] Schur contributions + coupling
    double *bcr_x;                      // [N][6 bw] solution of each super-row
    double *bcr_X;                      // [N][6 bw][12 bw + 1] X = D_m⁻¹[U | V | b] (forward -> backward)
    uint32_t *bcr_flag;                 // [N][2] forward / backward hand-off flags (epoch)
    uint32_t *bcr_ctl;                  // [kBcrCtl] epoch, forward arrivals / tickets, backward arrivals / tickets
    unsigned long long *bcr_stamps;     // never allocated: target of the retired phase marks kept in plba_dense.hpp
    int64_t bcr_sl[5];                  // per trial slot strides of bcr_pub, _x, _X, _flag, _ctl
};


// current state, read straight from the kernel arguments (kernels outside the trial: the index is
// dynamic, so these must not be applied to a local copy of Dev)
__device__ __forceinline__ double *Tcur(const Dev &d) { return d.Tb[d.ctrl->cur]; }
__device__ __forceinline__ double *Xcur(const Dev &d) { return d.Xb[d.ctrl->cur]; }
// per-edge χ² as g2o's edges hold it (the last consumed trial's, or the last linearisation's)
__device__ __forceinline__ double *chi2cur(const Dev &d) { return d.chi2b[d.ctrl->chi_src]; }

// element counts of the per-slot arrays (each allocated spec_max times back to back; the host
// allocation in plba.hip uses the same functions)
__host__ __device__ __forceinline__ size_t sl_band(const Dev &d) { return d.band_mode ? (size_t)d.nf * (d.bw + 1) * 36 : 1; }
__host__ __device__ __forceinline__ size_t sl_tw(const Dev &d) { return (size_t)d.nf * (d.bw + 1) * 36; }
__host__ __device__ __forceinline__ size_t sl_sep(const Dev &d) {
    return 2 * ((size_t)d.bw * (d.bw + 1) * 36 + (size_t)d.bw * 6);
}
__host__ __device__ __forceinline__ size_t sl_chp(const Dev &d) { return (size_t)(d.nch > 1 ? d.nch : 1) * 42; }
__host__ __device__ __forceinline__ size_t sl_lms(const Dev &d) { return (size_t)(d.n_lms_blocks > 1 ? d.n_lms_blocks : 1); }

// The window as trial slot s sees it: λ_s (g2o's λ after s rejections: λ *= ν, ν *= 2 — the same
// operations in the same order, so bitwise the λ the sequential loop would use), the state it
// starts from and the buffers it writes, and its own copies of every λ-dependent array.
// Returns a copy of Dev whose rotating-buffer arrays (Tb, Xb, ...) must not be indexed: only the
// resolved pointers are valid in it.
__device__ __forceinline__ Dev slot_view(const Dev &d0, int s) {
    Dev d = d0;
    const Ctrl *c = d0.ctrl;
    double lam = c->lambda, ni = c->ni;
    for (int k = 0; k < s; ++k) {
        lam *= ni;
        ni *= 2.0;
    }
    d.slot = s;
    d.lam = lam;
    const int cur = c->cur, ts = (cur + 1 + s) % d0.nbs;
    d.Tc = d0.Tb[cur]; d.Tt = d0.Tb[ts];
    d.Xc = d0.Xb[cur]; d.Xt = d0.Xb[ts];
    d.Lpc = d0.Lpb[cur]; d.Lpt = d0.Lpb[ts];
    d.xkc = d0.xk[cur]; d.xkt = d0.xk[ts];
    d.XLc = d0.XL[cur]; d.XLt = d0.XL[ts];
    const int lo = c->last_ok, xw = (lo + 1 + s) % d0.nbx;
    d.xp = d0.xpb[xw]; d.xl = d0.xlb[xw];
    d.xp_prev = d0.xpb[lo]; d.xl_prev = d0.xlb[lo];
    d.chi2_last = d0.chi2b[(c->chi_src + 1 + s) % d0.nbx];
    d.solve_okp = const_cast<int32_t *>(c->solve_ok) + s;
    if (s) {
        const size_t E = (size_t)d0.E, nf = (size_t)d0.nf, ss = (size_t)s;
        d.Z += ss * E * 8;
        d.q += ss * E * 2;
        d.ch_part += ss * sl_chp(d0);
        d.Bd += ss * sl_band(d0);
        d.Lband += ss * sl_band(d0);
        d.bs += ss * (size_t)d0.n;
        d.Kinv += ss * nf * 36;
        d.zb += ss * nf * 6;
        if (d0.twisted) {
            d.Bd2 += ss * sl_tw(d0);
            d.Lband2 += ss * sl_tw(d0);
            d.bs2 += ss * nf * 6;
            d.Kinv2 += ss * nf * 36;
            d.zb2 += ss * nf * 6;
            d.tw_sep += ss * sl_sep(d0);
            d.tw_fail += 2 * ss;
            d.tw_count += ss;
        }
        if (d0.bcr) {
            d.bcr_pub += ss * d0.bcr_sl[0];
            d.bcr_x += ss * d0.bcr_sl[1];
            d.bcr_X += ss * d0.bcr_sl[2];
            d.bcr_flag += ss * d0.bcr_sl[3];
            d.bcr_ctl += ss * d0.bcr_sl[4];
        }
        d.part_lm += ss * sl_lms(d0);
        d.part_lms += ss * sl_lms(d0);
        d.part_ps += ss * (size_t)d0.n_ps;
        d.cnt_rcs += ss * (size_t)d0.nblk;
    }
    return d;
}

// ---------------------------------------------------------------- block reductions
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}
// deterministic block sum: xor-butterfly inside each wave, then waves in index order.
// `sh` needs NT/64 doubles. Every thread receives the result.
template <int NT>
__device__ __forceinline__ double block_sum(double v, double *sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r += sh[w];
    __syncthreads();
    return r;
}
template <int NT>
__device__ __forceinline__ double block_max(double v, double *sh) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = fmax(r, sh[w]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ bool is_point_lm(const Dev &d, int lm) { return lm < d.n_pt; }

// ---------------------------------------------------------------- in-launch hand-offs
// Write-through (sc1) stores / loads: MI355X_MICROARCH.md "Valid forms" row 1 — data stored sc1,
// every storing wave drained, one lane per workgroup adds to an agent-scope counter, the
// workgroup whose add returns total-1 is last and reads the others' data with sc1 loads.
__device__ __forceinline__ double ld_sc1(const double *p) {
    return __hip_atomic_load(const_cast<double *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Every thread calls it after its sc1 stores; true in the last of `total` arriving workgroups,
// which resets the counter for the next launch (exactly `total` arrivals per launch).
__device__ __forceinline__ bool arrive_last(int32_t *counter, int32_t total) {
    __shared__ int s_last_arrival;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int32_t old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last_arrival = old == total - 1 ? 1 : 0;
        if (s_last_arrival) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return s_last_arrival != 0;
}

// Wave-level LDS ordering: this wave's LDS writes are complete and visible to its other lanes.
// Unlike a wavefront fence it does not wait for global loads/stores (vmcnt), so prefetches and
// result stores stay in flight across it.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Workgroup barrier that orders LDS only: global stores/prefetch loads stay in flight across it
// (__syncthreads() would drain vmcnt and put an L2 round trip on every step of a serial chain).
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---------------------------------------------------------------- kernel guards
// iteration kernels run for a new outer iteration and for the first one of a stage (the stage
// switch — SparseOptimizer::initializeOptimization — is folded into them)
// (a bounded in-kernel wait that timed out — Ctrl::dev_error — stops every later kernel of the
// batch; the host then re-solves the window with another factorisation)
#define ITER_GUARD                                                                             \
    {                                                                                          \
        const Ctrl *cg = d.ctrl;                                                               \
        if (cg->all_done || cg->dev_error || !(cg->need_iter || cg->switch_pending)) return;   \
    }
constexpr double kChi2Thr = 5.991;  // src/mapHandler.cpp:6129,6142
// a stage skipped by k_iter_init (no active edge) leaves switch_pending set: no trial
// PLBA_DIAG bit 128 (tests only): the column-lane factorisation reports a failed solve whenever
// bits 20.. of λ's representation are ≡ 0 (mod 3) — a deterministic function of the trial's λ, so
// runs with and without speculative slots fail the same trials (exercises A13's failure path).
__device__ __forceinline__ bool diag_fail(const Dev &d) {
    return (d.diag & 128) && ((unsigned long long)__double_as_longlong(d.lam) >> 20) % 3 == 0;
}
#define TRIAL_GUARD_OF(dd)                                                   \
    {                                                                        \
        const Ctrl *cg = (dd).ctrl;                                          \
        if (cg->all_done || cg->switch_pending || cg->dev_error) return;     \
    }
#define TRIAL_GUARD TRIAL_GUARD_OF(d)
// Trial kernels take the window as d0 and work on slot_view(d0, S): slots at or above this
// step's width (Ctrl::spec_w) exit at once.
#define TRIAL_SLOT(S)                                   \
    TRIAL_GUARD_OF(d0)                                  \
    if ((int)(S) >= d0.ctrl->spec_w) return;            \
    const Dev d = slot_view(d0, (int)(S));

}  // namespace plba
