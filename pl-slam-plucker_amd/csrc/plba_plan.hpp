// plba_plan.hpp — host-side decisions of an upload that need no device: the environment switches
// (Tuning) and the factorisation of the reduced camera system (FactorPlan). Pure functions of
// their arguments, so plba_factor_plan can pin the choice on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <string>

#include "plba_kernels.hpp"

namespace plba {

constexpr int kGraphLevelsMax = 4;  // multi-step graphs of 2, 4, 8, 16 steps

// Every environment switch of the solver, sampled ONCE at the start of each upload
// (read_tuning) and kept in the context: a switch changed later takes effect at the next upload.
// plba_pgo_optimize samples its own copy per call. Flags are on when the value starts with '1'
// unless noted. "bitwise": results are bit-for-bit the default's; "parity": same solution up
// to rounding (another summation or elimination order). Only PLBA_POISON, PLBA_PREWARM_MB and
// PLBA_NO_PREWARM are read elsewhere (when a context is created / an arena is filled).
struct Tuning {
    // PLBA_FACTOR=bcr|band|cl: force the banded factorisation (any other non-empty value acts
    // as cl: no BCR). parity
    enum Factor { kAuto, kForceBcr, kForceBand, kForceCl } factor = kAuto;
    bool no_cl = false;         // PLBA_NO_CL: LDS-window band kernels instead of column-lane. parity
    bool no_twist = false;      // PLBA_NO_TWIST: one-sided elimination only. parity
    bool no_rcm = false;        // PLBA_NO_RCM: keep the id order of a wide envelope. parity
    bool force_dense = false;   // PLBA_FORCE_DENSE: dense path for a banded window. parity
    bool dense_scalar = false;  // PLBA_DENSE_SCALAR: single-workgroup dense LDLᵀ, no MFMA. parity
    bool bcr_split = false;     // PLBA_BCR_SPLIT: BCR back substitution as a second launch. parity
    bool bcr_resident_set = false;  // PLBA_BCR_RESIDENT=<n> (non-empty): resident BCR workgroups
    int bcr_resident = 0;           //   assumed instead of the occupancy query (changes the choice)
    int spec = 0;               // PLBA_SPEC=<slots> (non-empty), 1..kMaxSpec; 0: default. bitwise
    int spec_policy = -1;       // PLBA_SPEC_POLICY=<0..3> (non-empty); -1: default. bitwise
    bool spec_bcr_off = false;  // PLBA_SPEC_BCR=0: one trial slot on BCR windows. bitwise
    int solve_lds_n = kSolveLdsN;   // PLBA_SOLVE_LDS_N=<n> (non-empty): y of the dense solve in LDS up to n. bitwise
    int chunk_triples = 0;      // PLBA_CHUNK_TRIPLES=<n> (set at all), 1..kChunk; 0: default. parity
    long long chunk_half_min = 1792;  // PLBA_CHUNK_HALF_MIN=<n> (set at all): two-lane assembly above n chunks. parity
    bool chunk_direct = false;  // PLBA_CHUNK_DIRECT (set at all): per-lane row loads in the assembly. bitwise
    bool no_fold_init = false;  // PLBA_NO_FOLD_INIT (set at all): k_iter_init as its own launch. parity
    int graph_levels = kGraphLevelsMax;  // PLBA_GRAPH_LEVELS=<n> (set at all), 0..4 multi-step graphs. bitwise
    bool shard_gather = true;   // PLBA_SHARD_XCHG=allreduce clears it: all-reduce the whole partial system. parity
    bool host_build = false;    // PLBA_HOST_BUILD: window structure built on the host. bitwise
    bool timing = false;        // PLBA_TIMING: upload / schedule phase log on stderr. bitwise
    bool timing_any = false;    //   (set at all: the device build's stage log too)
    int diag = 0;               // PLBA_DIAG=<mask> (set at all), tests only: 64 times out every BCR hand-off,
                                //   128 fails factorisations as a function of λ; other bits are ignored
};

inline Tuning read_tuning() {
    auto flag = [](const char *name) { const char *v = getenv(name); return v && v[0] == '1'; };
    auto filled = [](const char *name) { const char *v = getenv(name); return v && v[0] ? v : nullptr; };
    Tuning t;
    if (const char *f = filled("PLBA_FACTOR")) {
        const std::string s(f);
        t.factor = s == "bcr" ? Tuning::kForceBcr : s == "band" ? Tuning::kForceBand : Tuning::kForceCl;
    }
    t.no_cl = flag("PLBA_NO_CL");
    t.no_twist = flag("PLBA_NO_TWIST");
    t.no_rcm = flag("PLBA_NO_RCM");
    t.force_dense = flag("PLBA_FORCE_DENSE");
    t.dense_scalar = flag("PLBA_DENSE_SCALAR");
    t.bcr_split = flag("PLBA_BCR_SPLIT");
    if (const char *e = filled("PLBA_BCR_RESIDENT")) { t.bcr_resident_set = true; t.bcr_resident = atoi(e); }
    if (const char *e = filled("PLBA_SPEC")) t.spec = std::max(1, std::min(atoi(e), kMaxSpec));
    if (const char *e = filled("PLBA_SPEC_POLICY")) t.spec_policy = std::max(0, std::min(atoi(e), 3));
    if (const char *e = getenv("PLBA_SPEC_BCR")) t.spec_bcr_off = e[0] == '0';
    if (const char *e = filled("PLBA_SOLVE_LDS_N")) t.solve_lds_n = std::min(atoi(e), kSolveLdsN);
    if (const char *e = getenv("PLBA_CHUNK_TRIPLES")) t.chunk_triples = std::max(1, std::min(atoi(e), kChunk));
    if (const char *e = getenv("PLBA_CHUNK_HALF_MIN")) t.chunk_half_min = atoll(e);
    t.chunk_direct = getenv("PLBA_CHUNK_DIRECT") != nullptr;
    t.no_fold_init = getenv("PLBA_NO_FOLD_INIT") != nullptr;
    if (const char *e = getenv("PLBA_GRAPH_LEVELS")) t.graph_levels = std::max(0, std::min(atoi(e), kGraphLevelsMax));
    if (const char *e = getenv("PLBA_SHARD_XCHG")) t.shard_gather = std::string(e) != "allreduce";
    t.host_build = flag("PLBA_HOST_BUILD");
    t.timing = flag("PLBA_TIMING");
    t.timing_any = getenv("PLBA_TIMING") != nullptr;
    if (const char *e = getenv("PLBA_DIAG")) t.diag = atoi(e) & (64 | 128);
    return t;
}

// ---- dynamic LDS of the banded factorisation kernels (the element counts: plba_band.hpp,
// plba_band_cl.hpp, plba_bcr.hpp)
inline int band_ring(int bw, int nf) {
    const size_t budget = 158 * 1024 - band_static_bytes(bw), base = sizeof(double) * band_lds_doubles(bw, 0);
    const size_t per = sizeof(double) * ((size_t)bw * 36 + 36 + 6);
    int R = base + per < budget ? (int)((budget - base - per) / per) : 1;
    return std::max(1, std::min(R, 16));
}
static_assert(band_lds_doubles(kBandMax, 1) * sizeof(double) + band_static_bytes(kBandMax) <= 158 * 1024,
              "kBandMax window must fit LDS");
inline size_t band_lds_bytes(int bw, int nf) { return sizeof(double) * band_lds_doubles(bw, band_ring(bw, nf)); }
inline size_t twisted_lds_bytes(int bw, int nf) {
    // x_p staging [nf][6], then the separator merge or (bw >= 11) the streamed back substitution
    const size_t tail = std::max(twisted_merge_doubles(bw), bw * 6 > 64 ? bstream_doubles(bw) : (size_t)0);
    return std::max(band_lds_bytes(bw, nf), sizeof(double) * ((size_t)nf * 6 + tail));
}
inline size_t cl_lds_bytes(int bw, int nf, bool twisted) {
    return sizeof(double) * (cl_lds_doubles(bw) + (twisted ? (size_t)nf * 6 : 0));
}
inline size_t bcr_lds_bytes(int bw) { return sizeof(double) * bcr_lds_doubles(bw); }
inline size_t bcr_back_lds_bytes(int bw) { return sizeof(double) * bcr_back_lds_doubles(bw); }
constexpr size_t kLdsLimit = 159 * 1024;

// ---- the factorisation of one window
enum FactorMode : int {
    kDenseScalar,  // single-workgroup scalar LDLᵀ (k_rcs_factor, plba_dense.hpp)
    kDenseMfma,    // blocked LDLᵀ with MFMA trailing updates (plba_dense.hpp)
    kBand,         // LDS-window band kernel (plba_band.hpp), one sweep
    kBandTw,       // the same from both ends
    kCl,           // column-lane (plba_band_cl.hpp), bw <= kClMaxBW
    kClTw,         // column-lane from both ends
    kBcr,          // block cyclic reduction (plba_bcr.hpp), bw <= kBcrMaxBW
    kBcrBack       // (kernel lookup only: the split back substitution of kBcr)
};
struct FactorChoice {
    int mode = kBand;
    int tw_m = 0;  // two-sided modes: rows 0..tw_m-1 go top-down
};
struct FactorPlan : FactorChoice {
    int bcr_N = 0;      // BCR super-rows (= workgroups)
    int bcr_fused = 0;  // BCR back substitution inside the forward launch
    int ring = 1;       // band kernels: entering-row ring slots
    int slots = 1, policy = kSpecOff;  // speculative trial slots per step
    FactorChoice fallback{-1, 0};      // BCR: what the window drops to after a hand-off timeout
};

inline bool band_mode(int bw, const Tuning &t) { return bw <= kBandMax && !t.force_dense; }
// Two-sided split: rows 0..m-1 top-down, nf-1..m+bw bottom-up. An odd remainder goes to the top
// segment, so workgroup 0 usually arrives last and merges with the separator window already in
// its LDS (workgroup 1 as the last arriver must first reload segment 0's window from global
// memory): C3 hand-off + merge 10.9 k -> 8.1 k cycles, factorisation 74.8 -> 73.3 µs.
inline int tw_split(int nf, int bw) { return (nf - bw + 1) / 2; }
// column-lane factorisation for bandwidths up to kClMaxBW
inline bool use_cl(int bw, const Tuning &t) {
    return t.factor != Tuning::kForceBand && bw >= 1 && bw <= kClMaxBW && !t.no_cl;
}
// The non-BCR banded choice: column-lane when `cl`, else the LDS-window kernel; two-sided when the
// chain is long enough to halve and the separator's dense system fits next to the band window in LDS.
inline FactorChoice band_choice(int bw, int nf, bool cl, const Tuning &t) {
    const bool twisted = bw >= 1 && nf >= 2 * bw + 16 && !t.no_twist &&
                         (cl ? cl_lds_bytes(bw, nf, true) : twisted_lds_bytes(bw, nf) + band_static_bytes(bw)) <= kLdsLimit;
    if (cl && cl_lds_bytes(bw, nf, twisted) <= kLdsLimit) return {twisted ? kClTw : kCl, twisted ? tw_split(nf, bw) : 0};
    return {twisted ? kBandTw : kBand, twisted ? tw_split(nf, bw) : 0};
}
// BCR once the window has enough super-rows for its log-depth chain to beat the two-sided
// column-lane chain of (nf+bw)/2 pivot steps, and only when its N workgroups fit the device at
// once (`resident`): a launch that cannot hold them all still completes (ticket order,
// plba_bcr.hpp) but serialises the levels it exists to overlap.
inline bool want_bcr(int bw, int nf, int resident, const Tuning &t) {
    if (bw < 1 || bw > kBcrMaxBW) return false;
    const int N = (nf + bw - 1) / bw;
    if (N < 2 || N > resident || bcr_lds_bytes(bw) > kLdsLimit) return false;
    if (t.factor != Tuning::kAuto) return t.factor == Tuning::kForceBcr;
    // latency model calibrated on C3/C4/C5 (profiles/r02): the two-sided column-lane
    // chain costs ~1.3 µs per pivot block, (nf + bw)/2 of them; BCR ~(2.6·bw + 4.8) µs per level,
    // ceil(log2 N) + 1 levels. C3 (N = 13): 76 vs 116 µs -> column lane; C4 (N = 52): 230 vs
    // 157 µs and C5 (N = 129): 539 vs 198 µs -> BCR.
    int levels = 1;
    while ((1 << (levels - 1)) < N) ++levels;
    const double t_cl = 1.3 * (nf + bw) / 2.0, t_bcr = levels * (2.6 * bw + 4.8);
    return t_bcr < t_cl;
}
// Speculative trials: worth it where the step is bound by the serial factorisation
// chain and the rest of the chip idles during it — the banded one- or two-workgroup kernels and BCR
// windows whose slots' super-rows all fit the device at once (bcr_fit = resident workgroups /
// super-rows; else the second slot's super-rows would wait for the first's to retire. A/B at C4:
// 1,551 -> 1,817 LM it/s, 31 -> 22 steps per LBA). Not for the dense path or sharded windows
// (collectives per slot). Results are identical in every setting.
inline void plan_trials(FactorPlan &p, int bcr_fit, bool sharded, bool has_trials, const Tuning &t) {
    const bool bcr = p.mode == kBcr, wide = p.mode == kBand || p.mode == kBandTw;
    p.slots = 1;
    p.policy = kSpecOff;
    if (sharded || !has_trials || p.mode < kBand) return;
    int cap = kMaxSpec;
    if (bcr) {
        if (t.spec_bcr_off || bcr_fit < 2) return;
        cap = std::min(cap, bcr_fit);
    }
    // wide bands (bw > 9: the register-window kernel, ≈0.5 ms a factorisation at C3R) take every
    // slot: C3R 21 -> 17 steps per LBA, 1,000 -> 1,194 LM it/s (2 / 3 / 4 slots); so do
    // BCR windows, as far as the device holds the slots' super-rows (C4: 4 fit, 22 -> 17 steps,
    // 1,822 -> 1,851 LM it/s); the column-lane windows keep two (C3: 3 slots 5,248 vs 5,304)
    p.slots = std::min(t.spec ? t.spec : (wide || bcr) ? kMaxSpec : 2, cap);
    p.policy = t.spec_policy >= 0 ? t.spec_policy : kSpecSticky;
    if (p.policy == kSpecOff) p.slots = 1;
    if (p.slots == 1) p.policy = kSpecOff;
}
// The whole choice. `resident`: BCR forward workgroups the device holds at once (the occupancy
// query of the caller; PLBA_BCR_RESIDENT overrides it). `no_bcr`: this context fell back before.
inline FactorPlan plan_factor(int bw, int nf, int resident, bool no_bcr, bool sharded, bool has_trials, const Tuning &t) {
    static_assert(kBcrMaxBW <= kClMaxBW, "a BCR window must be able to fall back to the column-lane kernel");
    FactorPlan p;
    p.ring = band_ring(bw, nf);
    if (!band_mode(bw, t)) {
        p.mode = t.dense_scalar ? kDenseScalar : kDenseMfma;
        return p;
    }
    if (t.bcr_resident_set) resident = t.bcr_resident;
    const bool cl = use_cl(bw, t);
    if (!no_bcr && want_bcr(bw, nf, resident, t)) {
        p.mode = kBcr;
        p.bcr_N = (nf + bw - 1) / bw;
        p.bcr_fused = t.bcr_split ? 0 : 1;
        // the same rule as a window that never chose BCR, except that without the column-lane
        // kernel (PLBA_NO_CL) it is the one-sweep band kernel, never the two-sided one
        p.fallback = cl ? band_choice(bw, nf, true, t) : FactorChoice{kBand, 0};
    } else {
        static_cast<FactorChoice &>(p) = band_choice(bw, nf, cl, t);
    }
    plan_trials(p, p.mode == kBcr ? resident / std::max(p.bcr_N, 1) : 0, sharded, has_trials, t);
    return p;
}

}  // namespace plba
