// plba.hip — host side of the MI355X LBA backend: context, structure preparation, the
// Levenberg–Marquardt driver and the C ABI of include/plba.h.
//
// Control flow mirrors g2o exactly:
//   SparseOptimizer::initializeOptimization(level)   -> plba_initialize_optimization
//   SparseOptimizer::optimize(n)                     -> plba_optimize
//     OptimizationAlgorithmLevenberg::solve(it)      -> one iteration launch + trial launches
// The numerical work is all on the device (plba_kernels.hpp and the headers it includes); the host only reads back the
// 80-byte control block after each trial to decide whether another trial runs.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/plba.h"
#include "plba_build.hpp"
#include "plba_kernels.hpp"
#include "plba_plan.hpp"
#include "plba_scratch.hpp"

namespace plba {

enum KernelId {
    K_LINEARIZE, K_REDUCE, K_ITER_INIT, K_ESCHUR, K_MEMSET, K_ASSEMBLE, K_FINALIZE, K_FACTOR,
    K_POSE_UPDATE, K_LM_UPDATE, K_EVAL, K_DECIDE, K_DENSE_PANEL, K_DENSE_UPDATE,
    K_PACK,  // sharded: this rank's partials packed for an exchange (per-rank work)
    K_COMM,  // sharded: the collectives themselves (RCCL, or the host transport's round trip)
    K_COUNT
};
static const char *kKernelNames[K_COUNT] = {
    "k_linearize", "k_iter_reduce", "k_iter_init", "k_edge_schur", "memset_rcs",
    "k_rcs_chunk", "k_rcs_finalize", "k_rcs_factor", "k_pose_update", "k_lm_solve", "k_edge_eval", "k_decide",
    "k_dense_panel", "k_dense_update", "k_shard_pack", "collectives"};

// the pinned host copy of Ctrl, rounded up so that the trace copy behind it starts aligned
constexpr size_t kCtrlBlock = (sizeof(Ctrl) + 255) & ~(size_t)255;

}  // namespace plba

using namespace plba;

struct plba_ctx : plba::CtxBase {  // (opts, err / set_error, stream and the scratch blocks)
    bool uploaded = false, initialized = false;
    int level = 0;
    int robust = 1;
    Dev d{};
    // sharded windows: transport of the three per-step all-reduces
    struct Comm {
        enum Kind { NONE, RCCL, HOST } kind = NONE;
        int nranks = 1, rank = 0;
        ncclComm_t nccl = nullptr;
        plba_host_allreduce_fn fn = nullptr;
        void *user = nullptr;
        double *hbuf = nullptr;  // pinned staging (HOST)
        size_t hcap = 0;
    } comm;
    // device arena: ONE grow-only allocation carved per window (no hipMalloc / hipFree per
    // upload), filled by one memset and one host->device copy from pinned staging
    struct Item {
        void **field;
        size_t bytes, src_bytes;
        const void *src;
        bool zero;
        size_t off;
        const void *dsrc = nullptr;  // device source (copied D2D after the arena is carved)
    };
    std::vector<Item> arena_plan;  // the window's arrays in carving order (alloc .. commit_plan)
    BuildMem bmemA, bmemB;   // device window build scratch (plba_build.hip), grow-only
    char *arena = nullptr, *staging = nullptr;
    size_t arena_cap = 0, staging_cap = 0;
    Ctrl *h_ctrl = nullptr;  // pinned, one block with h_trace
    plba_iter_trace *h_trace = nullptr;  // [kTraceCap] pinned copy of Dev::trace, read with h_ctrl
    uint8_t *d_depth = nullptr;  // [Ep] isDepthPositive flags
    double *d_outd = nullptr;    // download staging, caller order: Tcw | pt_xyz | ln_orth | χ² (points,
                                 // lines) | bytes: depth flags [Ep] | levels (points, lines)
    char *h_out = nullptr;       // pinned host copy of it (grow-only)
    size_t h_out_cap = 0;
    // host-side bookkeeping
    int32_t n_kf = 0, n_pt = 0, n_ln = 0, Ep = 0, El = 0;
    std::vector<int32_t> e_orig;        // CSR edge -> original index within its type
    std::vector<int32_t> h_tile_last;   // dense path: last row tile of each column tile's envelope
    std::vector<int32_t> lm_gpos;       // local landmark -> whole-window landmark (points, then lines)
    std::vector<uint8_t> h_level;       // [E] CSR order
    std::vector<plba_iter_trace> trace;
    int stage = 0;
    size_t n_triples = 0;
    int64_t n_free_edges = 0;  // edges whose pose vertex is free
    // captured step graph (one LM trial + guarded iteration / stage-switch work)
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_exec = nullptr;
    bool graphs_stale = false;  // captured for a previous window (update before use)
    std::vector<int64_t> graph_sig;  // launch signature the executable graphs were built for
    // the same step captured 2, 4, 8, 16 times back to back: a batch of N steps is launched as
    // its binary decomposition (a graph-to-graph transition costs ~8 us on the device)
    static constexpr int kMultiLevels = kGraphLevelsMax;
    hipGraph_t multi_graph[kMultiLevels] = {};
    hipGraphExec_t multi_exec[kMultiLevels] = {};
    int last_steps = 16;     // steps the previous schedule needed (first batch size)
    int cur = 0;             // which state buffer holds the current estimate (mirror of Ctrl::cur)
    int last_ok = 0, chi_src = 0;  // x_p / x_l and χ² buffer indices (mirrors of Ctrl::last_ok / chi_src)
    bool no_graph = false;   // set when the step cannot be captured (RCCL without capture support)
    // block cyclic reduction safety net: a BCR hand-off wait that timed out (Ctrl::dev_error)
    // makes run_schedule restore the schedule's starting state from these copies, switch this
    // context to the column-lane factorisation for good (no_bcr) and solve the window again
    bool no_bcr = false;
    int bcr_fallbacks = 0;
    bool pool_hold = false;  // this context keeps the device pool's release threshold raised (prewarm)
    int dev_build = 0;  // the last upload's window structure was built on the device
    Tuning tuning;      // environment switches as sampled by the last upload
    FactorPlan plan;    // the factorisation chosen by the last upload (its fallback included)
    double *bk_T = nullptr, *bk_X = nullptr, *bk_xp = nullptr, *bk_xk = nullptr, *bk_Lpb = nullptr, *bk_XL = nullptr,
           *bk_xl = nullptr;
    uint8_t *bk_level = nullptr;
    int steps_launched = 0;
    // kernel timing (optional)
    bool timing = false;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_used;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;
    double k_ms[K_COUNT] = {0};
    int32_t k_n[K_COUNT] = {0};

    // A new window keeps the instantiated step graphs: the next capture updates them in place
    // (hipGraphExecUpdate, same topology, new kernel arguments and grids) instead of destroying
    // and re-instantiating five executable graphs (capture_step).
    void free_all() {
        graphs_stale = true;
        arena_plan.clear();
        d = Dev{};
        bk_T = bk_X = bk_xp = bk_xk = bk_Lpb = bk_XL = bk_xl = nullptr;
        bk_level = nullptr;
        uploaded = initialized = false;
    }
    // Records a device array of `count` T (at least 128 bytes: kernels issue unconditional
    // loads of one record for dead lanes, which must stay inside the array). `src` (host, kept
    // alive until commit_plan) is uploaded; everything else starts zeroed (`zero`: must stay
    // zero even under PLBA_POISON).
    template <typename T>
    void alloc(T *&p, size_t count, const void *src = nullptr, bool zero = false) {
        p = nullptr;
        const size_t sb = count * sizeof(T);
        arena_plan.push_back(Item{(void **)&p, std::max(sb, (size_t)128), src ? sb : 0, src, zero, 0});
    }
    // a device array filled from device memory (the device window build's outputs)
    template <typename T>
    void alloc_dev(T *&p, size_t count, const void *dsrc) {
        p = nullptr;
        const size_t sb = count * sizeof(T);
        arena_plan.push_back(Item{(void **)&p, std::max(sb, (size_t)128), sb, nullptr, false, 0, dsrc});
    }
    int commit_plan() {
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        size_t up = 0, tot = 0;
        for (auto &it : arena_plan)
            if (it.src) { it.off = up; up = al(up + it.bytes); }
        size_t dv = up;  // device-sourced arrays after the host-sourced ones, outside the memset
        for (auto &it : arena_plan)
            if (it.dsrc) { it.off = dv; dv = al(dv + it.bytes); }
        tot = dv;
        for (auto &it : arena_plan)
            if (!it.src && !it.dsrc) { it.off = tot; tot = al(tot + it.bytes); }
        if (tot > arena_cap) {
            // stream-ordered: hipFree / hipMalloc would synchronise the whole device, which fails
            // (and invalidates the capture) while another context of the process captures its
            // step graphs
            if (arena) (void)hipFreeAsync(arena, stream);
            arena = nullptr;
            arena_cap = 0;
            const size_t cap = tot + tot / 4;
            if (hipMallocAsync((void **)&arena, cap, stream) != hipSuccess) {
                (void)hipGetLastError();
                set_error("hipMalloc(%zu bytes) of the window arena failed", cap);
                return PLBA_E_NOMEM;
            }
            arena_cap = cap;
        }
        if (up > staging_cap) {
            (void)hipStreamSynchronize(stream);
            retire_pinned(staging);
            staging = nullptr;
            staging_cap = 0;
            const size_t cap = up + up / 4;
            if (hipHostMalloc((void **)&staging, cap, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                set_error("hipHostMalloc(%zu bytes) of the upload staging failed", cap);
                return PLBA_E_NOMEM;
            }
            staging_cap = cap;
        }
        for (auto &it : arena_plan) {
            *it.field = arena + it.off;
            if (it.src) {
                if (it.src_bytes) std::memcpy(staging + it.off, it.src, it.src_bytes);
                if (it.bytes > it.src_bytes) std::memset(staging + it.off + it.src_bytes, 0, it.bytes - it.src_bytes);
            }
        }
        // PLBA_POISON=1 (diagnostics only): non-uploaded arrays start as NaN (0xFF bytes) to expose
        // reads of memory no kernel wrote; arrays whose zero start is part of the contract stay 0
        const char *poison = getenv("PLBA_POISON");
        const bool pz = poison && poison[0] == '1';
        // device-sourced arrays [up, dv) are zeroed too before their payload is copied in, so the
        // padding past their payload reads as zero like a host array's (the 128-byte over-read
        // contract of alloc) — one memset of [up, tot) unless the rest is poisoned
        hipError_t e = pz ? hipMemsetAsync(arena + up, 0, dv - up, stream) : hipSuccess;
        if (e == hipSuccess) e = pz ? hipMemsetAsync(arena + dv, 0xFF, tot - dv, stream) : hipMemsetAsync(arena + up, 0, tot - up, stream);
        for (auto &it : arena_plan)
            if (it.dsrc && it.src_bytes && e == hipSuccess)
                e = hipMemcpyAsync(arena + it.off, it.dsrc, it.src_bytes, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess && pz)
            for (auto &it : arena_plan)
                if (it.zero && e == hipSuccess) e = hipMemsetAsync(arena + it.off, 0, it.bytes, stream);
        if (e == hipSuccess && up) e = hipMemcpyAsync(arena, staging, up, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("window arena fill failed: %s", hipGetErrorString(e));
            return PLBA_E_DEVICE;
        }
        return PLBA_OK;
    }
    // Pinned host blocks outgrown by a bigger window are freed only when the context is destroyed:
    // hipHostFree synchronises the device (see commit_plan). Growth is geometric, so few retire.
    std::vector<void *> retired;
    void retire_pinned(void *p) {
        if (p) retired.push_back(p);
    }
    hipEvent_t next_event() {
        if (ev_next == ev_pool.size()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            ev_pool.push_back(e);
        }
        return ev_pool[ev_next++];
    }
};

namespace {

inline int blocks_for(int n, int b = kBlock) { return (n + b - 1) / b; }

// Landmark -> rank: landmarks ordered by the id rank of the keyframe of their
// first observation (kf_obs_list[0]), cut into nranks contiguous runs of ~equal edge count.
void shard_plan(const plba_graph *g, int R, int32_t *pt_owner, int32_t *ln_owner) {
    std::vector<int32_t> korder(g->n_kf), kpos(g->n_kf);
    std::iota(korder.begin(), korder.end(), 0);
    std::stable_sort(korder.begin(), korder.end(), [&](int a, int b) { return g->kf_id[a] < g->kf_id[b]; });
    for (int i = 0; i < g->n_kf; ++i) kpos[korder[i]] = i;
    const int np = g->n_pt, nl = g->n_ln;
    std::vector<int32_t> key(np + nl, INT32_MAX), cnt(np + nl, 0);
    for (int e = 0; e < g->n_ept; ++e) {
        const int l = g->ept_lm[e];
        if (cnt[l]++ == 0) key[l] = kpos[g->ept_kf[e]];
    }
    for (int e = 0; e < g->n_eln; ++e) {
        const int l = np + g->eln_lm[e];
        if (cnt[l]++ == 0) key[l] = kpos[g->eln_kf[e]];
    }
    std::vector<int32_t> ord(np + nl);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return key[a] < key[b]; });
    int64_t total = 0, acc = 0;
    for (int c : cnt) total += c;
    for (int l : ord) {
        // rank of this landmark's edge-count midpoint
        const int64_t mid2 = 2 * acc + cnt[l];
        int r = total > 0 ? (int)((mid2 * R) / (2 * total)) : 0;
        r = std::min(std::max(r, 0), R - 1);
        acc += cnt[l];
        if (l < np) pt_owner[l] = r;
        else ln_owner[l - np] = r;
    }
}

// the instance K<bw> of a kernel template for bw in 0..Max (nullptr outside)
template <typename F, int... B>
const void *kernel_for(int bw, F pick, std::integer_sequence<int, B...>) {
    const void *k = nullptr;
    ((bw == B ? (k = pick(std::integral_constant<int, B>{}), 0) : 0), ...);
    return k;
}
#define PLBA_KERNEL(name, max, bw) \
    kernel_for(bw, [](auto b) { return (const void *)name<decltype(b)::value>; }, std::make_integer_sequence<int, (max) + 1>{})
// the kernel of a banded factorisation mode and its launch geometry (grid y = trial slots)
struct KernelLaunch {
    const void *fn;
    int grid_x, block;
    size_t lds_bytes;
};
KernelLaunch factor_kernel(int mode, int bw, int nf) {
    const int N = bw > 0 ? (nf + bw - 1) / bw : 0;  // BCR super-rows
    switch (mode) {
    case kBand: return {PLBA_KERNEL(k_rcs_factor_band, kBandMax, bw), 1, band_nt(bw), band_lds_bytes(bw, nf)};
    case kBandTw: return {PLBA_KERNEL(k_rcs_factor_twisted, kBandMax, bw), 2, band_nt(bw), twisted_lds_bytes(bw, nf)};
    case kCl: return {PLBA_KERNEL(k_rcs_factor_band_cl, kClMaxBW, bw), 1, kClNT, cl_lds_bytes(bw, nf, false)};
    case kClTw: return {PLBA_KERNEL(k_rcs_factor_twisted_cl, kClMaxBW, bw), 2, kClNT, cl_lds_bytes(bw, nf, true)};
    case kBcr: return {PLBA_KERNEL(k_rcs_factor_bcr, kBcrMaxBW, bw), N, kBcrNT, bcr_lds_bytes(bw)};
    case kBcrBack: return {PLBA_KERNEL(k_rcs_bcr_back, kBcrMaxBW, bw), N, kBcrBackNT, bcr_back_lds_bytes(bw)};
    default: return {nullptr, 0, 0, 0};  // the dense modes launch from launch_step
    }
}
// Workgroups of the BCR forward kernel the device holds at once: CUs x occupancy (LDS-bound, one
// per CU above 80 KB).
int bcr_resident(int device, int bw, int nf) {
    if (bw < 1 || bw > kBcrMaxBW) return 0;
    const KernelLaunch k = factor_kernel(kBcr, bw, nf);
    int cus = 0, occ = 0;
    if (k.lds_bytes > kLdsLimit ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds_bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k.fn, k.block, k.lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return cus * occ;
}
// The Dev fields the kernels read the factorisation from. A FactorChoice alone is what a BCR
// window's fallback rewrites (run_schedule): bcr_fused and the trial slots stay as uploaded.
void apply_plan(Dev &d, const FactorChoice &c) {
    d.bcr = c.mode == kBcr;
    if (!d.bcr) d.bcr_N = 0;
    d.cl = c.mode == kCl || c.mode == kClTw;
    d.twisted = c.mode == kBandTw || c.mode == kClTw;
    d.tw_m = c.tw_m;
}
void apply_plan(Dev &d, const FactorPlan &p) {
    d.band_mode = p.mode >= kBand;
    d.dense_mfma = p.mode == kDenseMfma;
    d.bcr_N = p.bcr_N;
    d.bcr_fused = p.bcr_fused;
    d.ring = p.ring;
    d.spec_max = p.slots;
    d.spec_policy = p.policy;
    d.nbs = d.spec_max + 1;
    d.nbx = d.spec_max > 1 ? d.spec_max + 1 : 1;
    apply_plan(d, static_cast<const FactorChoice &>(p));
}
inline int factor_mode(const Dev &d) {  // (inverse of apply_plan on a banded window)
    return d.bcr ? kBcr : d.cl ? (d.twisted ? kClTw : kCl) : (d.twisted ? kBandTw : kBand);
}
// the banded factorisation's launch(es); the first failing launch's status is returned
inline hipError_t launch_band(Dev &d, hipStream_t s) {
    void *args[] = {&d};
    const int mode = factor_mode(d);
    const KernelLaunch k = factor_kernel(mode, d.bw, d.nf);
    const hipError_t e = hipLaunchKernel(k.fn, dim3(k.grid_x, d.spec_max), dim3(k.block), args, k.lds_bytes, s);
    if (e != hipSuccess || mode != kBcr || d.bcr_fused) return e;
    const KernelLaunch b = factor_kernel(kBcrBack, d.bw, d.nf);  // back substitution + pose update
    return hipLaunchKernel(b.fn, dim3(b.grid_x, d.spec_max), dim3(b.block), args, b.lds_bytes, s);
}

// time a launch when kernel timing is enabled
template <typename F>
int timed(plba_ctx *ctx, int kid, F &&launch) {
    hipEvent_t a = nullptr, b = nullptr;
    if (ctx->timing) {
        a = ctx->next_event();
        b = ctx->next_event();
        (void)hipEventRecord(a, ctx->stream);
    }
    (void)hipGetLastError();  // launch errors below belong to this launch only
    launch();
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ctx->set_error("kernel %s launch failed: %s", kKernelNames[kid], hipGetErrorString(e));
        return PLBA_E_DEVICE;
    }
    if (ctx->timing) {
        (void)hipEventRecord(b, ctx->stream);
        ctx->ev_used.push_back({kid, {a, b}});
    }
    return PLBA_OK;
}

#define LAUNCH(kid, ...)                                   \
    do {                                                   \
        int _rc = timed(ctx, kid, [&] { __VA_ARGS__; });   \
        if (_rc) return _rc;                               \
    } while (0)

int collect_timing(plba_ctx *ctx) {
    if (!ctx->timing) return PLBA_OK;
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    for (auto &u : ctx->ev_used) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, u.second.first, u.second.second);
        ctx->k_ms[u.first] += ms;
        ctx->k_n[u.first] += 1;
    }
    ctx->ev_used.clear();
    ctx->ev_next = 0;
    return PLBA_OK;
}


// ------------------------------------------------------------------ upload / structure prep
// Reverse Cuthill–McKee order of the free poses (hidx 0..nf-1) on the graph "two free poses
// observe a common landmark": BFS from a pseudo-peripheral vertex of each component, neighbours
// by increasing degree, then reversed. Returns rcm[i] = the hidx placed at position i.
std::vector<int32_t> rcm_from_adj(std::vector<std::vector<int32_t>> &adj);
// doubles of the download staging block before its byte outputs
inline size_t out_doubles(size_t n_kf, size_t n_pt, size_t n_ln, size_t E) { return n_kf * 12 + n_pt * 3 + n_ln * 4 + E; }
std::vector<int32_t> rcm_order(const plba_graph *g, const std::vector<int32_t> &kf_hidx, int nf) {
    // landmark -> free poses as a CSR (counting sort of the edges by landmark), then the coupling
    // graph as an nf x nf bit matrix: its rows are the sorted, duplicate-free adjacency lists
    const int np_ = g->n_pt, nl = np_ + g->n_ln;
    std::vector<int32_t> off(nl + 1, 0);
    for (int e = 0; e < g->n_ept; ++e) off[g->ept_lm[e] + 1] += kf_hidx[g->ept_kf[e]] >= 0;
    for (int e = 0; e < g->n_eln; ++e) off[np_ + g->eln_lm[e] + 1] += kf_hidx[g->eln_kf[e]] >= 0;
    for (int l = 0; l < nl; ++l) off[l + 1] += off[l];
    std::vector<int32_t> fill(off.begin(), off.end() - 1), hs(off[nl]);
    for (int e = 0; e < g->n_ept; ++e) {
        const int h = kf_hidx[g->ept_kf[e]];
        if (h >= 0) hs[fill[g->ept_lm[e]]++] = h;
    }
    for (int e = 0; e < g->n_eln; ++e) {
        const int h = kf_hidx[g->eln_kf[e]];
        if (h >= 0) hs[fill[np_ + g->eln_lm[e]]++] = h;
    }
    const size_t W = ((size_t)nf + 63) / 64;
    std::vector<uint64_t> bits((size_t)nf * W, 0);
    for (int l = 0; l < nl; ++l)
        for (int i = off[l]; i < off[l + 1]; ++i)
            for (int j = i + 1; j < off[l + 1]; ++j) {
                const int a = hs[i], b = hs[j];
                if (a == b) continue;
                bits[(size_t)a * W + b / 64] |= 1ull << (b % 64);
                bits[(size_t)b * W + a / 64] |= 1ull << (a % 64);
            }
    std::vector<std::vector<int32_t>> adj(nf);
    for (int h = 0; h < nf; ++h) {
        const uint64_t *row = bits.data() + (size_t)h * W;
        int cnt = 0;
        for (size_t w = 0; w < W; ++w) cnt += __builtin_popcountll(row[w]);
        adj[h].reserve(cnt);
        for (size_t w = 0; w < W; ++w)
            for (uint64_t m = row[w]; m; m &= m - 1) adj[h].push_back((int32_t)(w * 64 + __builtin_ctzll(m)));
    }
    return rcm_from_adj(adj);
}
// RCM of an undirected graph given as adjacency lists (duplicates allowed; sorted in place)
std::vector<int32_t> rcm_from_adj(std::vector<std::vector<int32_t>> &adj) {
    const int nf = (int)adj.size();
    std::vector<int32_t> deg(nf);
    for (int h = 0; h < nf; ++h) {
        auto &a = adj[h];
        std::sort(a.begin(), a.end());
        a.erase(std::unique(a.begin(), a.end()), a.end());
        deg[h] = (int32_t)a.size();
    }
    for (int h = 0; h < nf; ++h)
        std::stable_sort(adj[h].begin(), adj[h].end(), [&](int x, int y) { return deg[x] < deg[y]; });
    std::vector<int32_t> order;
    order.reserve(nf);
    std::vector<char> seen(nf, 0);
    auto bfs = [&](int root, std::vector<int32_t> &out) {  // returns the last level's min-degree vertex
        std::vector<int32_t> lev(nf, -1);
        out.clear();
        out.push_back(root);
        lev[root] = 0;
        for (size_t q = 0; q < out.size(); ++q)
            for (int v : adj[out[q]])
                if (lev[v] < 0) {
                    lev[v] = lev[out[q]] + 1;
                    out.push_back(v);
                }
        const int last = lev[out.back()];
        int best = out.back();
        for (int v : out)
            if (lev[v] == last && deg[v] < deg[best]) best = v;
        return std::make_pair(best, last);
    };
    std::vector<int32_t> comp;
    for (int s0 = 0; s0 < nf; ++s0) {
        if (seen[s0]) continue;
        // pseudo-peripheral start: repeat BFS from the far end while the depth grows
        int root = s0;
        auto r = bfs(root, comp);
        for (int it = 0; it < 8; ++it) {
            auto r2 = bfs(r.first, comp);
            if (r2.second <= r.second) break;
            root = r.first;
            r = r2;
        }
        bfs(root, comp);  // Cuthill–McKee order of this component (neighbours by degree)
        for (int v : comp) {
            seen[v] = 1;
            order.push_back(v);
        }
    }
    std::reverse(order.begin(), order.end());
    // refinement: a few passes of "sort by the mean position of self and neighbours" (a discrete
    // smoothing that straightens thick paths, where level-by-level orders give ~2x the band);
    // the narrowest order seen wins
    auto bandwidth = [&](const std::vector<int32_t> &ord) {
        std::vector<int32_t> p(nf);
        for (int i = 0; i < nf; ++i) p[ord[i]] = i;
        int w = 0;
        for (int h = 0; h < nf; ++h)
            for (int v : adj[h]) w = std::max(w, std::abs(p[h] - p[v]));
        return w;
    };
    std::vector<int32_t> best = order, cur = order, p(nf);
    int bw_best = bandwidth(best);
    for (int it = 0; it < 24 && bw_best > 0; ++it) {
        for (int i = 0; i < nf; ++i) p[cur[i]] = i;
        std::vector<double> key(nf);
        for (int h = 0; h < nf; ++h) {
            double s = p[h];
            for (int v : adj[h]) s += p[v];
            key[h] = s / (double)(adj[h].size() + 1);
        }
        std::stable_sort(cur.begin(), cur.end(), [&](int a, int b) { return key[a] < key[b]; });
        const int w = bandwidth(cur);
        if (w < bw_best) {
            bw_best = w;
            best = cur;
        }
    }
    return best;
}

int allreduce(plba_ctx *ctx, const double *send, double *recv, size_t n);
// ---- upload, phase by phase (do_upload, at the end, is the sequence)
int validate_graph(plba_ctx *ctx, const plba_graph *g, bool host_build) {
    if (!g || g->n_kf < 0 || g->n_pt < 0 || g->n_ln < 0 || g->n_ept < 0 || g->n_eln < 0) {
        ctx->set_error("invalid graph sizes");
        return PLBA_E_INVALID;
    }
    if ((g->n_kf && (!g->kf_Tcw || !g->kf_fixed || !g->kf_id)) || (g->n_pt && (!g->pt_xyz || !g->pt_id)) ||
        (g->n_ln && (!g->ln_orth || !g->ln_id)) ||
        (g->n_ept && (!g->ept_lm || !g->ept_kf || !g->ept_obs || !g->ept_info)) ||
        (g->n_eln && (!g->eln_lm || !g->eln_kf || !g->eln_obs || !g->eln_info))) {
        ctx->set_error("null array in graph");
        return PLBA_E_INVALID;
    }
    if (g->n_kf > 0 && !host_build) return PLBA_OK;  // (the device build validates the edges itself)
    for (int e = 0; e < g->n_ept; ++e)
        if (g->ept_lm[e] < 0 || g->ept_lm[e] >= g->n_pt || g->ept_kf[e] < 0 || g->ept_kf[e] >= g->n_kf) {
            ctx->set_error("point edge %d references a missing vertex", e);
            return PLBA_E_INVALID;
        }
    for (int e = 0; e < g->n_eln; ++e)
        if (g->eln_lm[e] < 0 || g->eln_lm[e] >= g->n_ln || g->eln_kf[e] < 0 || g->eln_kf[e] >= g->n_kf) {
            ctx->set_error("line edge %d references a missing vertex", e);
            return PLBA_E_INVALID;
        }
    return PLBA_OK;
}
// the "[plba upload]" phase log of PLBA_TIMING (tools/upload_timing.py and DESIGN quote the labels)
struct PhaseLog {
    bool on;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        const auto t = std::chrono::steady_clock::now();
        if (on) fprintf(stderr, "[plba upload] %-24s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - last).count());
        last = t;
    }
};
// What the window build hands on, from the host or from the device (plba_build.hip; bit for bit
// the same arrays): free poses, envelope, this rank's counts and the landmark-major edge arrays
// — host vectors, or (devb) wb's device arrays. The output maps (lm_gpos, e_orig), the free-edge
// count and the level mirror go to the context directly.
struct WindowStructure {
    bool devb = false;
    int nf = 0, bw = 0, n_pt = 0, n_ln = 0, Ep = 0, El = 0;
    std::vector<int32_t> kf_hidx, first_blk;
    std::vector<int32_t> e_lm, e_kf, e_hidx, e_gpos, lm_off, pe_off, pe_list, trip;
    std::vector<double> e_obs, e_info;
    WindowBuild wb;
};
// keyframes in vertex-id order (buildIndexMapping)
std::vector<int32_t> kf_id_order(const plba_graph *g) {
    std::vector<int32_t> korder(g->n_kf);
    std::iota(korder.begin(), korder.end(), 0);
    std::stable_sort(korder.begin(), korder.end(), [&](int a, int b) { return g->kf_id[a] < g->kf_id[b]; });
    return korder;
}
// Hessian indices after the free poses are reordered: rcm[i] = the old index placed at position i
std::vector<int32_t> permute_hidx(const std::vector<int32_t> &hidx, const std::vector<int32_t> &rcm) {
    std::vector<int32_t> pos(rcm.size()), h2(hidx.size(), -1);
    for (size_t i = 0; i < rcm.size(); ++i) pos[rcm[i]] = (int32_t)i;
    for (size_t k = 0; k < hidx.size(); ++k) h2[k] = hidx[k] >= 0 ? pos[hidx[k]] : -1;
    return h2;
}
// Window structure on the device (sorts / scans / scatters on the solver stream).
int build_structure_device(plba_ctx *ctx, const plba_graph *g, PhaseLog &mark, WindowStructure &ws) {
    const int n_kf = g->n_kf;
    WindowBuild &wb = ws.wb;
    // free poses by vertex id and the id rank of every keyframe
    const std::vector<int32_t> korder = kf_id_order(g);
    std::vector<int32_t> kpos(n_kf);
    ws.kf_hidx.assign(n_kf, -1);
    for (int i = 0; i < n_kf; ++i) {
        kpos[korder[i]] = i;
        if (!g->kf_fixed[korder[i]]) ws.kf_hidx[korder[i]] = ws.nf++;
    }
    const int nf = ws.nf;
    wb.g = g;
    wb.nranks = ctx->comm.nranks;
    wb.rank = ctx->comm.rank;
    wb.nf = nf;
    wb.kpos = kpos.data();
    wb.stream = ctx->stream;
    wb.timing = ctx->tuning.timing_any;
    auto stage1 = [&](const std::vector<int32_t> &hidx, int &bw) {  // the build and its envelope width
        char msg[256] = {0};
        wb.kf_hidx = hidx.data();
        const int rc = build_stage1(ctx->bmemA, wb, msg, sizeof msg);
        if (rc) ctx->set_error("%s", msg);
        bw = 0;
        for (int h = 0; h < nf && !rc; ++h) bw = std::max(bw, h - wb.first_blk[h]);
        return rc;
    };
    int rc = stage1(ws.kf_hidx, ws.bw);
    if (rc) return rc;
    // an envelope the banded kernels cannot take may narrow under the RCM order (the host
    // build's rule, same permutation: rcm_order over the whole graph): build again with the
    // reordered free poses, kept when the envelope narrows, else built once more in id order
    if (ws.bw > kClMaxBW && nf > 2 && !ctx->tuning.no_rcm) {
        const std::vector<int32_t> h2 = permute_hidx(ws.kf_hidx, rcm_order(g, ws.kf_hidx, nf));
        int bw2 = 0;
        if ((rc = stage1(h2, bw2))) return rc;
        if (bw2 < ws.bw) {
            ws.kf_hidx = h2;
            ws.bw = bw2;
        } else if ((rc = stage1(ws.kf_hidx, bw2))) {
            return rc;
        }
        wb.kf_hidx = ws.kf_hidx.data();  // (h2 dies with this block)
        mark("device build (RCM order)");
    }
    ws.first_blk = wb.first_blk;
    ws.devb = true;
    mark("device build (stage 1 proper)");
    ws.n_pt = wb.n_pt; ws.n_ln = wb.n_ln; ws.Ep = wb.Ep; ws.El = wb.El;
    ctx->n_free_edges = wb.n_free_edges;
    // host mirrors of the output maps (plba_download / plba_get_edge_chi2)
    ctx->lm_gpos.resize(wb.n_lm);
    ctx->e_orig.resize(wb.E);
    if (wb.n_lm)
        PLBA_CHECK(hipMemcpyAsync(ctx->lm_gpos.data(), wb.lm_gpos, sizeof(int32_t) * wb.n_lm, hipMemcpyDeviceToHost, ctx->stream));
    if (wb.E)
        PLBA_CHECK(hipMemcpyAsync(ctx->e_orig.data(), wb.e_orig, sizeof(int32_t) * wb.E, hipMemcpyDeviceToHost, ctx->stream));
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->h_level.assign(wb.E, 0);
    mark("device build (stage 1)");
    return PLBA_OK;
}
// first_blk[h] = the lowest free pose sharing a landmark with free pose h (over the WHOLE window);
// returns the envelope width in pose blocks
int envelope(const plba_graph *g, const std::vector<int32_t> &hidx, std::vector<int32_t> &fb) {
    const int nf = (int)fb.size(), np_ = g->n_pt;
    for (int h = 0; h < nf; ++h) fb[h] = h;
    std::vector<int32_t> lmin(np_ + g->n_ln, INT32_MAX);
    for (int e = 0; e < g->n_ept; ++e) {
        const int h = hidx[g->ept_kf[e]];
        if (h >= 0) lmin[g->ept_lm[e]] = std::min(lmin[g->ept_lm[e]], h);
    }
    for (int e = 0; e < g->n_eln; ++e) {
        const int h = hidx[g->eln_kf[e]];
        if (h >= 0) lmin[np_ + g->eln_lm[e]] = std::min(lmin[np_ + g->eln_lm[e]], h);
    }
    for (int e = 0; e < g->n_ept; ++e) {
        const int h = hidx[g->ept_kf[e]];
        if (h >= 0) fb[h] = std::min(fb[h], lmin[g->ept_lm[e]]);
    }
    for (int e = 0; e < g->n_eln; ++e) {
        const int h = hidx[g->eln_kf[e]];
        if (h >= 0) fb[h] = std::min(fb[h], lmin[np_ + g->eln_lm[e]]);
    }
    int w = 0;
    for (int h = 0; h < nf; ++h) w = std::max(w, h - fb[h]);
    return w;
}
// Window structure on the host (PLBA_HOST_BUILD=1, or a window without keyframes): the reference
// the device build is tested against bit for bit.
int build_structure_host(plba_ctx *ctx, const plba_graph *g, PhaseLog &mark, WindowStructure &ws) {
    const int n_kf = g->n_kf, n_pt_g = g->n_pt, n_ln_g = g->n_ln, Ep_g = g->n_ept, El_g = g->n_eln;
    const int R = ctx->comm.nranks, rank = ctx->comm.rank;
    int &n_pt = ws.n_pt, &n_ln = ws.n_ln, &nf = ws.nf;
    const std::vector<int32_t> korder = kf_id_order(g);
    // landmarks owned by this rank (all of them unless the window is sharded)
    std::vector<int32_t> pt_owner(n_pt_g, 0), ln_owner(n_ln_g, 0);
    if (R > 1) shard_plan(g, R, pt_owner.data(), ln_owner.data());
    // Local landmark order: points then lines, each sorted (stably) by the id rank of the
    // keyframe of their first observation, so the edges of one pose — and the landmarks one RCS
    // block couples — sit in a narrow range of the landmark-major edge array (cache locality of
    // the pose reduction and the Schur assembly; any order gives the same solution).
    std::vector<int32_t> pt_loc(n_pt_g, -1), ln_loc(n_ln_g, -1), &lm_gpos = ctx->lm_gpos;
    lm_gpos.clear();
    {
        std::vector<int32_t> kpos(n_kf);
        for (int i = 0; i < n_kf; ++i) kpos[korder[i]] = i;
        std::vector<int32_t> key_pt(n_pt_g, INT32_MAX), key_ln(n_ln_g, INT32_MAX);
        for (int e = Ep_g - 1; e >= 0; --e) key_pt[g->ept_lm[e]] = kpos[g->ept_kf[e]];
        for (int e = El_g - 1; e >= 0; --e) key_ln[g->eln_lm[e]] = kpos[g->eln_kf[e]];
        // stable counting sort by key (key in [0, n_kf], n_kf = never observed)
        auto order = [&](int n, const std::vector<int32_t> &own, const std::vector<int32_t> &key,
                         std::vector<int32_t> &loc, int &cnt, int gbase) {
            std::vector<int32_t> c(n_kf + 2, 0);
            for (int i = 0; i < n; ++i)
                if (own[i] == rank) c[std::min(key[i], n_kf) + 1]++;
            for (int k = 0; k <= n_kf; ++k) c[k + 1] += c[k];
            const int base = (int)lm_gpos.size();
            lm_gpos.resize(base + c[n_kf + 1]);
            for (int i = 0; i < n; ++i)
                if (own[i] == rank) {
                    const int pos = c[std::min(key[i], n_kf)]++;
                    loc[i] = pos;
                    lm_gpos[base + pos] = gbase + i;
                }
            cnt = (int)lm_gpos.size() - base;
        };
        order(n_pt_g, pt_owner, key_pt, pt_loc, n_pt, 0);
        order(n_ln_g, ln_owner, key_ln, ln_loc, n_ln, n_pt_g);
    }
    for (int e = 0; e < Ep_g; ++e) ws.Ep += pt_loc[g->ept_lm[e]] >= 0;
    for (int e = 0; e < El_g; ++e) ws.El += ln_loc[g->eln_lm[e]] >= 0;
    const int n_lm = n_pt + n_ln, E = ws.Ep + ws.El;

    // free poses ordered by vertex id (buildIndexMapping)
    ws.kf_hidx.assign(n_kf, -1);
    for (int k : korder)
        if (!g->kf_fixed[k]) ws.kf_hidx[k] = nf++;
    ws.first_blk.assign(nf, 0);
    ws.bw = envelope(g, ws.kf_hidx, ws.first_blk);
    // Reverse Cuthill–McKee on the free-pose coupling graph when the natural (id) order leaves an
    // envelope wider than the column-lane / BCR kernels take: windows that revisit old keyframes
    // couple poses a loop apart. LinearSolverEigen orders the same matrix by AMD; any symmetric
    // permutation gives the same exact LDLᵀ solution (rounding aside). PLBA_NO_RCM=1 disables.
    if (ws.bw > kClMaxBW && nf > 2 && !ctx->tuning.no_rcm) {
        const std::vector<int32_t> h2 = permute_hidx(ws.kf_hidx, rcm_order(g, ws.kf_hidx, nf));
        std::vector<int32_t> fb2(nf);
        const int bw2 = envelope(g, h2, fb2);
        if (bw2 < ws.bw) {
            ws.kf_hidx = h2;
            ws.first_blk = fb2;
            ws.bw = bw2;
        }
    }
    mark("envelope (+ RCM)");

    // landmark-major CSR of the local landmarks (stable within a landmark = g2o insertion order)
    std::vector<int32_t> &e_lm = ws.e_lm, &e_kf = ws.e_kf, &e_hidx = ws.e_hidx, &e_gpos = ws.e_gpos, &e_orig = ctx->e_orig;
    ws.lm_off.assign(n_lm + 1, 0);
    for (int e = 0; e < Ep_g; ++e)
        if (pt_loc[g->ept_lm[e]] >= 0) ws.lm_off[pt_loc[g->ept_lm[e]] + 1]++;
    for (int e = 0; e < El_g; ++e)
        if (ln_loc[g->eln_lm[e]] >= 0) ws.lm_off[n_pt + ln_loc[g->eln_lm[e]] + 1]++;
    for (int l = 0; l < n_lm; ++l) ws.lm_off[l + 1] += ws.lm_off[l];
    std::vector<int32_t> fill(ws.lm_off.begin(), ws.lm_off.end() - 1);
    e_lm.assign(E, 0); e_kf.assign(E, 0); e_hidx.assign(E, 0); e_orig.assign(E, 0); e_gpos.assign(E, 0);
    ws.e_obs.assign((size_t)E * 4, 0.0); ws.e_info.assign(E, 0.0);
    for (int e = 0; e < Ep_g; ++e) {
        const int l = pt_loc[g->ept_lm[e]];
        if (l < 0) continue;
        const int pos = fill[l]++;
        e_lm[pos] = l;
        e_kf[pos] = g->ept_kf[e];
        e_orig[pos] = e;
        e_gpos[pos] = e;
        ws.e_obs[(size_t)pos * 4] = g->ept_obs[2 * e];
        ws.e_obs[(size_t)pos * 4 + 1] = g->ept_obs[2 * e + 1];
        ws.e_info[pos] = g->ept_info[e];
    }
    for (int e = 0; e < El_g; ++e) {
        if (ln_loc[g->eln_lm[e]] < 0) continue;
        const int l = n_pt + ln_loc[g->eln_lm[e]], pos = fill[l]++;
        e_lm[pos] = l;
        e_kf[pos] = g->eln_kf[e];
        e_orig[pos] = e;
        e_gpos[pos] = Ep_g + e;
        for (int k = 0; k < 4; ++k) ws.e_obs[(size_t)pos * 4 + k] = g->eln_obs[4 * e + k];
        ws.e_info[pos] = g->eln_info[e];
    }
    for (int e = 0; e < E; ++e) e_hidx[e] = ws.kf_hidx[e_kf[e]];
    ctx->n_free_edges = std::count_if(e_hidx.begin(), e_hidx.end(), [](int32_t h) { return h >= 0; });
    ctx->h_level.assign(E, 0);
    mark("landmark order + CSR");
    // free-pose-major edge lists (ascending CSR edge index)
    ws.pe_off.assign(nf + 1, 0);
    for (int e = 0; e < E; ++e)
        if (e_hidx[e] >= 0) ws.pe_off[e_hidx[e] + 1]++;
    for (int h = 0; h < nf; ++h) ws.pe_off[h + 1] += ws.pe_off[h];
    ws.pe_list.assign(ws.pe_off[nf], 0);
    std::vector<int32_t> f(ws.pe_off.begin(), ws.pe_off.end() - 1);
    for (int e = 0; e < E; ++e)
        if (e_hidx[e] >= 0) ws.pe_list[f[e_hidx[e]]++] = e;
    return PLBA_OK;
}

// Reduced-camera block pattern: the envelope of the lower triangle. Blocks are indexed densely
// within the envelope in (i2, i1) order (one layout on every rank: the all-reduced value array);
// Schur triples (e1 at pose i1 <= e2 at pose i2, same landmark, local landmarks only) are
// counting-sorted by block, landmark order inside a block, and cut into assembly chunks.
struct BlockPattern {
    int nblk = 0, nch = 0, n = 0, ntiles = 0;
    std::vector<int64_t> blk_base;
    std::vector<int32_t> blk_i1, blk_i2, blk_off, ch_blk, ch_off, blk_ch, tile_first, tile_last;
};
int build_block_pattern(plba_ctx *ctx, WindowStructure &ws, PhaseLog &mark, BlockPattern &bp) {
    const int nf = ws.nf;
    const std::vector<int32_t> &first_blk = ws.first_blk;
    std::vector<int64_t> &blk_base = bp.blk_base;
    blk_base.assign(nf + 1, 0);
    for (int h = 0; h < nf; ++h) blk_base[h + 1] = blk_base[h] + (h - first_blk[h] + 1);
    if (blk_base[nf] > INT32_MAX / 64) {
        ctx->set_error("reduced camera envelope too large (%lld blocks)", (long long)blk_base[nf]);
        return PLBA_E_INVALID;
    }
    const int nblk = bp.nblk = (int)blk_base[nf];
    std::vector<int32_t> &blk_off = bp.blk_off;
    bp.blk_i1.resize(nblk);
    bp.blk_i2.resize(nblk);
    blk_off.assign(nblk + 1, 0);
    for (int h = 0; h < nf; ++h)
        for (int i1 = first_blk[h]; i1 <= h; ++i1) {
            const int b = (int)(blk_base[h] + (i1 - first_blk[h]));
            bp.blk_i1[b] = i1;
            bp.blk_i2[b] = h;
        }
    if (ws.devb) {  // device build, stage 2: Schur triples sorted by block on the device
        char msg[256] = {0};
        const int brc = build_stage2(ctx->bmemA, ctx->bmemB, ws.wb, blk_base, nblk, msg, sizeof msg);
        if (brc) {
            ctx->set_error("%s", msg);
            return brc;
        }
        blk_off = ws.wb.h_blk_off;
        ctx->n_triples = (size_t)ws.wb.n_triples;
    } else {
        auto for_pairs = [&](auto &&f) {
            for (int l = 0; l < ws.n_pt + ws.n_ln; ++l)
                for (int a = ws.lm_off[l]; a < ws.lm_off[l + 1]; ++a) {
                    const int i1 = ws.e_hidx[a];
                    if (i1 < 0) continue;
                    for (int b = ws.lm_off[l]; b < ws.lm_off[l + 1]; ++b) {
                        const int i2 = ws.e_hidx[b];
                        if (i2 < i1) continue;
                        f(a, b, (int)(blk_base[i2] + (i1 - first_blk[i2])));
                    }
                }
        };
        for_pairs([&](int, int, int blk) { blk_off[blk + 1]++; });
        for (int k = 0; k < nblk; ++k) blk_off[k + 1] += blk_off[k];
        ws.trip.resize(2 * (size_t)blk_off[nblk]);
        std::vector<int32_t> pos(blk_off.begin(), blk_off.end() - 1);
        for_pairs([&](int a, int b, int blk) {
            const size_t t = (size_t)pos[blk]++;
            ws.trip[2 * t] = a;
            ws.trip[2 * t + 1] = b;
        });
        ctx->n_triples = (size_t)blk_off[nblk];
    }
    mark("blocks + triples");
    // chunks of <= chunk triples, never spanning two blocks
    // (at least one chunk per block, possibly empty: the last chunk of a block to finish
    // assembles it, so every envelope block — zero ones included — is written each trial).
    // Windows up to 600 k triples take half-size chunks: twice the waves, each half as long, the
    // assembly being one round of waves there (C3: 25.5 -> 23.9 µs; C5 keeps 256: 115.3 vs 117.9);
    // PLBA_CHUNK_TRIPLES overrides (<= kChunk)
    int chunk = ctx->n_triples <= 600000 ? kChunk / 2 : kChunk;
    if (ctx->tuning.chunk_triples) chunk = ctx->tuning.chunk_triples;
    bp.blk_ch.assign(nblk + 1, 0);
    for (int k = 0; k < nblk; ++k) {
        bp.blk_ch[k] = (int32_t)bp.ch_blk.size();
        int t = blk_off[k];
        do {
            bp.ch_blk.push_back(k);
            bp.ch_off.push_back(t);
            t += chunk;
        } while (t < blk_off[k + 1]);
    }
    bp.blk_ch[nblk] = (int32_t)bp.ch_blk.size();
    bp.ch_off.push_back(blk_off[nblk]);
    bp.nch = (int)bp.ch_blk.size();
    // envelope of the lower triangle (per 6-row pose block: first pose block column)
    bp.n = 6 * nf;
    bp.ntiles = (bp.n + kTile - 1) / kTile;
    TileEnvelope te = tile_envelope(first_blk, bp.n, kTile);
    bp.tile_first = std::move(te.tile_first);
    bp.tile_last = std::move(te.tile_last);
    ctx->h_tile_last = bp.tile_last;
    mark("chunks + envelope");
    return PLBA_OK;
}

// sizes, options and launch grids of the window (everything in Dev that is not a pointer or part
// of the factorisation plan)
void describe_window(plba_ctx *ctx, const plba_graph *g, const WindowStructure &ws, const BlockPattern &bp) {
    Dev &d = ctx->d;
    d.n_kf = g->n_kf; d.n_pt = ws.n_pt; d.n_ln = ws.n_ln; d.n_lm = ws.n_pt + ws.n_ln;
    d.Ep = ws.Ep; d.El = ws.El; d.E = ws.Ep + ws.El;
    d.nf = ws.nf; d.n = bp.n; d.nblk = bp.nblk; d.ntiles = bp.ntiles; d.nch = bp.nch;
    // any transport selects the sharded code path (a 1-rank RCCL window exercises it on one GPU)
    d.sharded = ctx->comm.kind != plba_ctx::Comm::NONE ? 1 : 0;
    d.nranks = ctx->comm.nranks;
    d.rank = ctx->comm.rank;
    d.n_lm_g = g->n_pt + g->n_ln;
    d.E_g = g->n_ept + g->n_eln;
    d.bw = ws.bw;
    d.corrected = ctx->opts.corrected_line_jacobian;
    d.diag = ctx->tuning.diag;
    d.solve_lds_n = ctx->tuning.solve_lds_n;
    d.cam = Cam{g->fx, g->fy, g->cx, g->cy};
    d.huber_pt = g->huber_pt;
    d.huber_ln = g->huber_ln;
    d.tau = ctx->opts.tau;
    d.n_lin_blocks = blocks_for(d.E);
    d.n_lm_blocks = blocks_for(d.n_lm, kLmBlock);
    d.n_lms_blocks = blocks_for(d.n_lm * kLmLanes, kLmsNT);
    d.n_kf_blocks = blocks_for(d.n_kf);
    d.fold = d.sharded ? 0 : 1;
    d.fold_init = d.fold && !ctx->tuning.no_fold_init;
    d.xg_host = ctx->comm.kind == plba_ctx::Comm::HOST ? 1 : 0;
}

int allreduce(plba_ctx *ctx, const double *send, double *recv, size_t n);
// Sharded windows, all-gather exchange of the RCS (the default; PLBA_SHARD_XCHG=allreduce restores
// the all-reduce of the whole partial system): this rank's block-row range [lo, hi]
// (rows of the blocks that hold one of its Schur triples — every local edge of a free pose has its
// diagonal triple), as two runs of red_rcs; every rank's runs are exchanged here, so all ranks
// size the same record (P doubles per rank)
struct ShardRanges {
    std::vector<int64_t> rng;
    int64_t P = 0;
};
int exchange_shard_ranges(plba_ctx *ctx, int nf, const BlockPattern &bp, ShardRanges &xg) {
    if (!ctx->d.sharded || bp.nblk <= 0 || !ctx->tuning.shard_gather) return PLBA_OK;
    const int R = ctx->comm.nranks, rank = ctx->comm.rank;
    int lo = nf, hi = -1;
    for (int b = 0; b < bp.nblk; ++b)
        if (bp.blk_off[b + 1] > bp.blk_off[b]) {
            lo = std::min(lo, bp.blk_i2[b]);
            hi = std::max(hi, bp.blk_i2[b]);
        }
    std::vector<double> mine(4 * (size_t)R, 0.0);
    if (hi >= lo) {
        mine[4 * rank + 0] = (double)(bp.blk_base[lo] * 36);
        mine[4 * rank + 1] = (double)((bp.blk_base[hi + 1] - bp.blk_base[lo]) * 36);
        mine[4 * rank + 2] = (double)((int64_t)bp.nblk * 36 + 6 * (int64_t)lo);
        mine[4 * rank + 3] = (double)(6 * (int64_t)(hi - lo + 1));
    }
    double *tmp = nullptr;
    PLBA_CHECK(hipMallocAsync((void **)&tmp, mine.size() * sizeof(double), ctx->stream));
    PLBA_CHECK(hipMemcpyAsync(tmp, mine.data(), mine.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    int xrc = allreduce(ctx, tmp, tmp, mine.size());
    if (!xrc) {
        xrc = hipMemcpyAsync(mine.data(), tmp, mine.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) ==
                      hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess
                  ? PLBA_OK : PLBA_E_DEVICE;
    }
    (void)hipFreeAsync(tmp, ctx->stream);
    if (xrc) {
        if (xrc == PLBA_E_DEVICE) ctx->set_error("shard range exchange: device copy failed");
        return xrc;
    }
    xg.rng.resize(4 * (size_t)R);
    for (int r = 0; r < R; ++r) {
        for (int k = 0; k < 4; ++k) xg.rng[4 * r + k] = (int64_t)mine[4 * r + k];
        xg.P = std::max(xg.P, xg.rng[4 * r + 1] + xg.rng[4 * r + 3]);
    }
    xg.P = std::max<int64_t>(xg.P, 2);
    return PLBA_OK;
}

// Every device array of the window, carved from the arena: commit_plan assigns the pointers IN
// CALL ORDER, so the order of the lines below is the arena layout (addresses, PLBA_POISON
// coverage) and must not change. Host sources must live until commit_plan (stage_arrays).
#define ALLOC(p, n_) ctx->alloc(p, (size_t)(n_))
#define ZALLOC(p, n_) ctx->alloc(p, (size_t)(n_), nullptr, true)
#define UPLOAD(p, v) ctx->alloc(p, (v).size(), (v).data())
// host vector (host build) or the device build's array of n_ elements
#define UPLOAD_D(p, v, dptr, n_)                             \
    do {                                                     \
        if (ws.devb) ctx->alloc_dev(p, (size_t)(n_), (dptr)); \
        else UPLOAD(p, v);                                   \
    } while (0)
struct StagedHost {  // host sources built for the staging only
    std::vector<double> T, X;
    std::vector<int32_t> ln_gidx, h_kf;
};
// first part: states, edges, per-iteration and per-slot arrays
void stage_state_arrays(plba_ctx *ctx, const plba_graph *g, const WindowStructure &ws, StagedHost &h) {
    Dev &d = ctx->d;
    const WindowBuild &wb = ws.wb;
    const int n_kf = d.n_kf, n_pt = d.n_pt, n_ln = d.n_ln, n_lm = d.n_lm, E = d.E, nf = d.nf, n_pt_g = g->n_pt, n_ln_g = g->n_ln;
    const std::vector<int32_t> &lm_gpos = ctx->lm_gpos;
    h.T.assign(g->kf_Tcw, g->kf_Tcw + (size_t)n_kf * 12);
    if (!ws.devb) {
        h.X.assign((size_t)n_lm * 4, 0.0);
        for (int p = 0; p < n_pt; ++p)
            for (int k = 0; k < 3; ++k) h.X[(size_t)p * 4 + k] = g->pt_xyz[3 * (size_t)lm_gpos[p] + k];
        for (int l = 0; l < n_ln; ++l)
            for (int k = 0; k < 4; ++k)
                h.X[(size_t)(n_pt + l) * 4 + k] = g->ln_orth[4 * (size_t)(lm_gpos[n_pt + l] - n_pt_g) + k];
    }
    const int nbs = d.nbs, nbx = d.nbx, W = d.spec_max;
    UPLOAD(d.T_init, h.T);
    UPLOAD(d.Tb[0], h.T);
    for (int b = 1; b < nbs; ++b) ALLOC(d.Tb[b], h.T.size());
    UPLOAD_D(d.X_init, h.X, wb.X, (size_t)n_lm * 4);
    UPLOAD_D(d.Xb[0], h.X, wb.X, (size_t)n_lm * 4);
    for (int b = 1; b < nbs; ++b) ALLOC(d.Xb[b], (size_t)n_lm * 4);
    for (int b = 0; b < nbs; ++b) ALLOC(d.xk[b], (size_t)n_kf * 6);
    // hand-rolled GBA: endpoint lines in the reference's (global) order, their 6x6 blocks
    for (int b = 0; b < nbs; ++b) ALLOC(d.XL[b], (size_t)std::max(n_ln_g, 1) * 6);
    ALLOC(d.Hl6, (size_t)std::max(n_ln, 1) * 21);
    ALLOC(d.bl6, (size_t)std::max(n_ln, 1) * 6);
    h.ln_gidx.assign(std::max(n_ln, 1), 0);
    for (int i = 0; i < n_ln; ++i) h.ln_gidx[i] = lm_gpos[n_pt + i] - n_pt_g;
    UPLOAD(d.ln_gidx, h.ln_gidx);
    for (int b = 0; b < nbs; ++b) ALLOC(d.Lpb[b], (size_t)std::max(n_ln, 1) * 8);
    UPLOAD(d.kf_hidx, ws.kf_hidx);
    UPLOAD_D(d.e_lm, ws.e_lm, wb.e_lm, E);
    UPLOAD_D(d.e_kf, ws.e_kf, wb.e_kf, E);
    UPLOAD_D(d.e_hidx, ws.e_hidx, wb.e_hidx, E);
    UPLOAD_D(d.e_obs, ws.e_obs, wb.e_obs, (size_t)E * 4);
    UPLOAD_D(d.e_info, ws.e_info, wb.e_info, E);
    ZALLOC(d.e_level, E);
    ALLOC(d.e_active, E);
    UPLOAD_D(d.lm_off, ws.lm_off, wb.lm_off, n_lm + 1);
    ALLOC(d.lm_active, n_lm);
    UPLOAD_D(d.pe_off, ws.pe_off, wb.pe_off, nf + 1);
    UPLOAD_D(d.pe_list, ws.pe_list, wb.pe_list, ctx->n_free_edges);
    ALLOC(d.A, (size_t)E * 12);
    ALLOC(d.cvec, (size_t)E * 2);
    ALLOC(d.B, (size_t)E * 8);
    for (int b = 0; b < nbx; ++b) ZALLOC(d.chi2b[b], E);
    // unsharded: Hpp | b_p | active | χ² | any | max; sharded: diag(Hpp) | b_p | active | χ² | any |
    // per-rank maxima, all-reduced (the full partial Hpp stays local: Hpp_w)
    ALLOC(d.red_iter, (size_t)nf * (d.sharded ? 13 : 43) + 2 + d.nranks);
    if (d.sharded) {
        ALLOC(d.red_iter_loc, (size_t)nf * 13 + 2 + d.nranks);
        ALLOC(d.Hpp_w, (size_t)nf * 36);
    }
    ALLOC(d.Hll, (size_t)n_lm * 10);
    ALLOC(d.bl, (size_t)n_lm * 4);
    // λ-dependent arrays: one copy per trial slot, back to back (slot_view, sl_* in plba_dev.hpp)
    ALLOC(d.Z, (size_t)W * E * 8);
    ALLOC(d.q, (size_t)W * E * 2);
    for (int b = 0; b < nbx; ++b) ZALLOC(d.xlb[b], (size_t)n_lm * 4);
}
// second part: the reduced camera system, its factorisation scratch, reductions, outputs
void stage_system_arrays(plba_ctx *ctx, const plba_graph *g, const WindowStructure &ws, const BlockPattern &bp,
                         const ShardRanges &xg, StagedHost &h) {
    Dev &d = ctx->d;
    const WindowBuild &wb = ws.wb;
    const FactorPlan &plan = ctx->plan;
    const int n_kf = d.n_kf, n_pt = d.n_pt, n_ln = d.n_ln, n_lm = d.n_lm, Ep = d.Ep, E = d.E, nf = d.nf, n = d.n, nblk = d.nblk,
              bw = d.bw, R = d.nranks, n_ln_g = g->n_ln, nbx = d.nbx, W = d.spec_max;
    const bool two_sided = d.twisted || plan.fallback.mode == kClTw;
    UPLOAD(d.blk_i1, bp.blk_i1);
    UPLOAD(d.blk_i2, bp.blk_i2);
    UPLOAD(d.blk_off, bp.blk_off);
    UPLOAD_D(d.trip, ws.trip, wb.trip, 2 * (size_t)ctx->n_triples);
    UPLOAD(d.ch_blk, bp.ch_blk);
    UPLOAD(d.ch_off, bp.ch_off);
    UPLOAD(d.blk_ch, bp.blk_ch);
    ALLOC(d.ch_part, (size_t)W * sl_chp(d));
    ALLOC(d.Ad, d.band_mode ? 1 : (size_t)n * n);
    UPLOAD(d.first_blk, ws.first_blk);
    // band blocks outside the envelope (w > i - first_blk[i]) are never assembled and must
    // read as zero: the band kernels sweep all BW block columns of every row
    ZALLOC(d.Bd, (size_t)W * sl_band(d));
    ALLOC(d.Lband, (size_t)W * sl_band(d));
    ALLOC(d.Kinv, (size_t)W * nf * 36);
    ALLOC(d.zb, (size_t)W * nf * 6);
    if (two_sided) {  // (of the plan or of the fallback a BCR window may switch to)
        ZALLOC(d.Bd2, (size_t)W * sl_tw(d));
        ALLOC(d.bs2, (size_t)W * nf * 6);
        ALLOC(d.Lband2, (size_t)W * sl_tw(d));
        ALLOC(d.Kinv2, (size_t)W * nf * 36);
        ALLOC(d.zb2, (size_t)W * nf * 6);
        ALLOC(d.tw_sep, (size_t)W * sl_sep(d));
        ZALLOC(d.tw_fail, 2 * (size_t)W);
        ZALLOC(d.tw_count, (size_t)W);
    }
    if (d.bcr) {  // flags carry epochs from bcr_ctl[0]: start from a clean slate (one set per trial slot)
        const int64_t N = d.bcr_N;
        d.bcr_sl[0] = N * (int64_t)bcr_pub_doubles(bw);
        d.bcr_sl[1] = N * (int64_t)bcr_xrec(bw);
        d.bcr_sl[2] = N * (int64_t)bcr_X_doubles(bw);
        d.bcr_sl[3] = 2 * N;
        d.bcr_sl[4] = kBcrCtl;
        ALLOC(d.bcr_pub, (size_t)W * d.bcr_sl[0]);
        ALLOC(d.bcr_x, (size_t)W * d.bcr_sl[1]);
        ALLOC(d.bcr_X, (size_t)W * d.bcr_sl[2]);
        h.h_kf.assign(nf, 0);
        for (int k = 0; k < n_kf; ++k)
            if (ws.kf_hidx[k] >= 0) h.h_kf[ws.kf_hidx[k]] = k;
        UPLOAD(d.h_kf, h.h_kf);
        ZALLOC(d.bcr_flag, (size_t)W * d.bcr_sl[3]);
        ZALLOC(d.bcr_ctl, (size_t)W * kBcrCtl);
        // the schedule's starting state, restored if a hand-off wait times out (run_schedule)
        ALLOC(ctx->bk_T, (size_t)n_kf * 12);
        ALLOC(ctx->bk_X, (size_t)std::max(n_lm, 1) * 4);
        ALLOC(ctx->bk_xp, (size_t)std::max(n, 6));
        ALLOC(ctx->bk_xk, (size_t)n_kf * 6);
        ALLOC(ctx->bk_Lpb, (size_t)std::max(n_ln, 1) * 8);
        ALLOC(ctx->bk_XL, (size_t)std::max(n_ln_g, 1) * 6);
        ALLOC(ctx->bk_level, (size_t)std::max(E, 1));
        ALLOC(ctx->bk_xl, (size_t)std::max(n_lm, 1) * 4);
    }
    ALLOC(d.bs, (size_t)W * n);
    // k_lm_solve reads x_p[6·max(h, 0) ..] for fixed-pose slots too
    for (int b = 0; b < nbx; ++b) ZALLOC(d.xpb[b], std::max(n, 6));
    ALLOC(d.Wbuf, (size_t)std::max(n, 1) * (kTile + 1));  // W panel + y of the dense path
    UPLOAD(d.tile_first, bp.tile_first);
    UPLOAD(d.tile_last, bp.tile_last);
    ALLOC(d.part_chi2, d.n_lin_blocks);
    ALLOC(d.part_any, d.n_lm_blocks);
    ALLOC(d.part_max, nf + d.n_lm_blocks);
    ALLOC(d.pose_part, (size_t)std::max(nf, 1) * kPoseParts * kPP);
    ALLOC(d.part_lm, (size_t)W * sl_lms(d));
    ALLOC(d.part_lms, (size_t)W * sl_lms(d));
    // arrival counters: lm_solve, iter_reduce (top), RCS blocks, poses, iter_reduce groups
    const int nred = kPoseParts * nf + (d.n_lm > 0 ? d.n_lm_blocks : 0), ngrp = (nred + kRedGrp - 1) / kRedGrp;
    ZALLOC(d.cnt, 2 + (size_t)nblk + nf + ngrp);
    ZALLOC(d.cnt_rcs, (size_t)W * nblk);  // per trial slot: arrivals per RCS block
    ALLOC(d.wg_red, 3 * (size_t)std::max(nred, 1));
    ALLOC(d.grp_red, 3 * (size_t)std::max(ngrp, 1));
    d.n_ps = std::max(d.n_kf_blocks, d.bcr_N);
    ZALLOC(d.part_ps, (size_t)W * d.n_ps);
    ZALLOC(d.ctrl, 1);
    ALLOC(d.trace, kTraceCap);
    ALLOC(ctx->d_depth, Ep);
    ALLOC(d.red_rcs, (size_t)nblk * 36 + (size_t)nf * 6);
    ALLOC(d.red_dec, 3);
    if (d.sharded) {
        ALLOC(d.red_rcs_loc, (size_t)nblk * 36 + (size_t)nf * 6);
        ALLOC(d.red_dec_loc, 4);  // + the hand-off error agreement slot (agree_dev_error)
    }
    d.xg_P = 0;
    if (d.sharded && xg.rng.size()) {
        d.xg_P = xg.P;
        UPLOAD(d.xg_rng, xg.rng);
        // zeroed once: blockpart rewrites the same in-run positions every step, the padding (and,
        // host transport, the other ranks' slots) stays zero
        ZALLOC(d.xg_send, (size_t)(d.xg_host ? R : 1) * xg.P);
        ALLOC(d.xg_recv, (size_t)R * xg.P);
    }
    // output maps (local landmark / edge -> whole-window position): the download scatter
    // (k_out_scatter) or, sharded, the final gather of the full window X | χ² | depth | level
    UPLOAD_D(d.lm_gpos, ctx->lm_gpos, wb.lm_gpos, n_lm);
    UPLOAD_D(d.e_gpos, ws.e_gpos, wb.e_gpos, E);
    if (d.sharded) {
        ALLOC(d.gat, (size_t)d.n_lm_g * 4 + 3 * (size_t)d.E_g);
    } else {
        // one staging block: Tcw | pt_xyz | ln_orth | χ² (doubles), then the byte outputs
        ALLOC(ctx->d_outd, out_doubles(n_kf, n_pt, n_ln, E) + ((size_t)Ep + E + 7) / 8);
    }
}
#undef ALLOC
#undef ZALLOC
#undef UPLOAD
#undef UPLOAD_D
// stages every array and fills the arena while the host sources are alive
int stage_arrays(plba_ctx *ctx, const plba_graph *g, const WindowStructure &ws, const BlockPattern &bp,
                 const ShardRanges &xg, PhaseLog &mark) {
    StagedHost h;
    stage_state_arrays(ctx, g, ws, h);
    stage_system_arrays(ctx, g, ws, bp, xg, h);
    mark("host arrays staged");
    return ctx->commit_plan();
}
// views into the arena's arrays: slot 0's buffers for the kernels that never run speculatively
// (one χ² / solve buffer then) and the sections of the per-iteration reduction record
void bind_views(Dev &d) {
    const size_t nf = (size_t)d.nf;
    d.xp = d.xpb[0];
    d.xl = d.xlb[0];
    d.chi2_last = d.chi2b[0];
    if (d.sharded) {
        d.Hpp = nullptr;
        d.Hdg = d.red_iter;
        d.bp = d.red_iter + nf * 6;
        d.pact = d.red_iter + nf * 12;
        d.Hdg_w = d.red_iter_loc;
        d.bp_w = d.red_iter_loc + nf * 6;
        d.pact_w = d.red_iter_loc + nf * 12;
    } else {
        d.Hpp = d.red_iter;
        d.bp = d.red_iter + nf * 36;
        d.pact = d.red_iter + nf * 42;
        d.red_iter_loc = d.red_iter;
        d.Hpp_w = d.red_iter_loc;
        d.bp_w = d.red_iter_loc + nf * 36;
        d.pact_w = d.red_iter_loc + nf * 42;
        d.Hdg = d.Hdg_w = nullptr;
    }
}
// dynamic LDS above the default limit: every kernel the plan or its fallback may launch
int raise_lds_limits(plba_ctx *ctx) {
    const FactorPlan &p = ctx->plan;
    const int modes[] = {p.mode, p.mode == kBcr && !p.bcr_fused ? kBcrBack : -1, p.fallback.mode};
    for (int m : modes) {
        const KernelLaunch k = factor_kernel(m, ctx->d.bw, ctx->d.nf);
        if (k.fn) PLBA_CHECK(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds_bytes));
    }
    return PLBA_OK;
}

int do_upload(plba_ctx *ctx, const plba_graph *g) {
    const Tuning &t = ctx->tuning = read_tuning();
    int rc = validate_graph(ctx, g, t.host_build);
    if (rc) return rc;
    PhaseLog mark{t.timing};
    ctx->free_all();
    mark("free");
    ctx->n_kf = g->n_kf; ctx->n_pt = g->n_pt; ctx->n_ln = g->n_ln; ctx->Ep = g->n_ept; ctx->El = g->n_eln;
    // Window structure on the device unless PLBA_HOST_BUILD=1 (or there is no keyframe)
    WindowStructure ws;
    rc = g->n_kf > 0 && !t.host_build ? build_structure_device(ctx, g, mark, ws) : build_structure_host(ctx, g, mark, ws);
    if (rc) return rc;
    ctx->dev_build = ws.devb ? 1 : 0;
    BlockPattern bp;
    if ((rc = build_block_pattern(ctx, ws, mark, bp))) return rc;
    Dev &d = ctx->d;
    describe_window(ctx, g, ws, bp);
    const int resident =
        band_mode(ws.bw, t) && !ctx->no_bcr && !t.bcr_resident_set ? bcr_resident(ctx->opts.device, ws.bw, ws.nf) : 0;
    ctx->plan = plan_factor(ws.bw, ws.nf, resident, ctx->no_bcr, d.sharded != 0, d.n_lm > 0 && bp.nch > 0, t);
    apply_plan(d, ctx->plan);
    ShardRanges xg;
    if ((rc = exchange_shard_ranges(ctx, ws.nf, bp, xg))) return rc;
    if ((rc = stage_arrays(ctx, g, ws, bp, xg, mark))) return rc;
    bind_views(d);
    if ((rc = raise_lds_limits(ctx))) return rc;
    mark("alloc + copy + memset");
    ctx->uploaded = true;
    ctx->initialized = false;
    ctx->cur = ctx->last_ok = ctx->chi_src = 0;
    return PLBA_OK;
}

// One "step": [stage switch] -> [iteration: linearise + reductions + λ init] -> one damped
// trial -> decide -> commit. Every kernel is guarded by the device control block, so a fixed
// sequence can be captured once and replayed; steps after the schedule finished are no-ops.
// Sum of n doubles over the ranks of a sharded window: send (this rank's partials) -> recv.
// Device -> host read on the context's own stream. Never the legacy stream (plain hipMemcpy):
// while another context of the process captures its step graphs (first batch of a new window),
// a legacy-stream copy is refused and invalidates that capture.
hipError_t d2h(plba_ctx *ctx, void *dst, const void *src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    return e == hipSuccess ? hipStreamSynchronize(ctx->stream) : e;
}
int allreduce(plba_ctx *ctx, const double *send, double *recv, size_t n) {
    auto &c = ctx->comm;
    if (n == 0) return PLBA_OK;
    if (c.kind == plba_ctx::Comm::RCCL) {
        const ncclResult_t r = ncclAllReduce(send, recv, n, ncclDouble, ncclSum, c.nccl, ctx->stream);
        if (r != ncclSuccess) {
            ctx->set_error("ncclAllReduce(%zu doubles): %s", n, ncclGetErrorString(r));
            return PLBA_E_COMM;
        }
        return PLBA_OK;
    }
    if (c.kind == plba_ctx::Comm::HOST) {
        if (c.hcap < n) {
            PLBA_CHECK(hipStreamSynchronize(ctx->stream));
            ctx->retire_pinned(c.hbuf);
            c.hbuf = nullptr;
            PLBA_CHECK(hipHostMalloc((void **)&c.hbuf, n * sizeof(double), hipHostMallocDefault));
            c.hcap = n;
        }
        PLBA_CHECK(hipMemcpyAsync(c.hbuf, send, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PLBA_CHECK(hipStreamSynchronize(ctx->stream));
        const int rc = c.fn(c.user, c.hbuf, (int64_t)n);
        if (rc) {
            ctx->set_error("host all-reduce callback returned %d", rc);
            return PLBA_E_COMM;
        }
        PLBA_CHECK(hipMemcpyAsync(recv, c.hbuf, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        return PLBA_OK;
    }
    ctx->set_error("sharded window without a transport");
    return PLBA_E_COMM;
}
// All-gather of P doubles per rank: recv = [rank 0's P | rank 1's P | ...]. The host transport
// only sums, so there each rank's send is its own slot of an R x P array, zero elsewhere.
int allgather(plba_ctx *ctx, const double *send, double *recv, size_t P) {
    auto &c = ctx->comm;
    if (P == 0) return PLBA_OK;
    if (c.kind == plba_ctx::Comm::RCCL) {
        const ncclResult_t r = ncclAllGather(send, recv, P, ncclDouble, c.nccl, ctx->stream);
        if (r != ncclSuccess) {
            ctx->set_error("ncclAllGather(%zu doubles): %s", P, ncclGetErrorString(r));
            return PLBA_E_COMM;
        }
        return PLBA_OK;
    }
    return allreduce(ctx, send, recv, (size_t)c.nranks * P);
}
#define COMM(send, recv, n)                                                        \
    do {                                                                           \
        int _crc = 0;                                                              \
        LAUNCH(K_COMM, _crc = allreduce(ctx, (send), (recv), (size_t)(n)));        \
        if (_crc) return _crc;                                                     \
    } while (0)

// Schur assembly with two lanes per triple (k_rcs_chunk_h) once a slot's chunk waves exceed what
// k_rcs_chunk keeps resident (1.75 waves per SIMD x 1024 SIMDs) — per slot, so that the choice
// (and the rounding) does not depend on the trial-slot count; PLBA_CHUNK_HALF_MIN overrides the
// threshold (0: always, a huge value: never)
bool chunk_half(const plba_ctx *ctx) { return (long long)ctx->d.nch > ctx->tuning.chunk_half_min; }
int launch_step(plba_ctx *ctx) {
    Dev &d = ctx->d;
    hipStream_t s = ctx->stream;
    // PLBA_CHUNK_DIRECT=1: per-lane A/Z row loads in the Schur assembly (A/B of the staged copy)
    const bool chunk_direct = ctx->tuning.chunk_direct;

    if (d.E > 0) LAUNCH(K_LINEARIZE, hipLaunchKernelGGL(k_linearize, dim3(d.n_lin_blocks), dim3(kBlock), 0, s, d));
    if (d.nf > 0 || d.n_lm > 0) {
        const int nred = kPoseParts * d.nf + (d.n_lm > 0 ? d.n_lm_blocks : 0);
        LAUNCH(K_REDUCE, hipLaunchKernelGGL(k_iter_reduce, dim3(nred), dim3(kLmBlock), 0, s, d));
    }
    if (d.sharded) {
        LAUNCH(K_PACK, hipLaunchKernelGGL(k_iter_pack, dim3(1), dim3(kInitNT), 0, s, d));
        COMM(d.red_iter_loc, d.red_iter, (size_t)d.nf * 13 + 2 + d.nranks);
    }
    const bool reduced = d.nf > 0 || d.n_lm > 0;
    if (!(d.fold_init && reduced))  // (folded into the last k_iter_reduce workgroup otherwise)
        LAUNCH(K_ITER_INIT, hipLaunchKernelGGL(k_iter_init, dim3(1), dim3(kInitNT), 0, s, d));
    if (d.n_lm > 0) {
        LAUNCH(K_ESCHUR, hipLaunchKernelGGL(k_edge_schur, dim3(d.n_lin_blocks, d.spec_max), dim3(kBlock), 0, s, d));
    }
    if (d.n > 0) {
        if (!d.band_mode) LAUNCH(K_MEMSET, (void)hipMemsetAsync(d.Ad, 0, sizeof(double) * (size_t)d.n * d.n, s));
        if (d.nch > 0) LAUNCH(K_ASSEMBLE, hipLaunchKernelGGL(chunk_direct ? k_rcs_chunk<false> : chunk_half(ctx) ? k_rcs_chunk_h : k_rcs_chunk<true>, dim3(8 * ((d.nch + 7) / 8), d.spec_max), dim3(64), 0, s, d));
        if (d.sharded) {
            LAUNCH(K_PACK, hipLaunchKernelGGL(k_rcs_blockpart, dim3(blocks_for(d.nblk * 42)), dim3(kBlock), 0, s, d));
            if (d.xg_P > 0) {  // all-gather of every rank's nonzero runs, summed in rank order
                int grc = 0;
                LAUNCH(K_COMM, grc = allgather(ctx, d.xg_send, d.xg_recv, (size_t)d.xg_P));
                if (grc) return grc;
                LAUNCH(K_FINALIZE, hipLaunchKernelGGL(k_rcs_xunpack, dim3(blocks_for(d.nblk * 36 + d.nf * 6)), dim3(kBlock), 0, s, d));
            } else {
                COMM(d.red_rcs_loc, d.red_rcs, (size_t)d.nblk * 36 + (size_t)d.nf * 6);
            }
        }
        if (!(d.fold && d.nch > 0))  // (folded into the last chunk of each block otherwise)
            LAUNCH(K_FINALIZE, hipLaunchKernelGGL(k_rcs_finalize, dim3(blocks_for(d.nblk * 42)), dim3(kBlock), 0, s, d));
        const size_t solve_lds = d.n <= d.solve_lds_n ? sizeof(double) * (size_t)d.n : 0;  // y of dense_solve_wg
        if (d.band_mode) {
            hipError_t fe = hipSuccess;
            LAUNCH(K_FACTOR, fe = launch_band(d, s));
            if (fe != hipSuccess) {
                (void)hipGetLastError();
                ctx->set_error("factorisation launch failed: %s", hipGetErrorString(fe));
                return PLBA_E_DEVICE;
            }
        } else if (d.dense_mfma) {  // blocked LDLᵀ, MFMA trailing updates (plba_dense.hpp)
            for (int K = 0; K < d.ntiles; ++K) {  // the envelope's row tiles K..tile_last[K] only
                const int m = ctx->h_tile_last[K] - K;
                LAUNCH(K_DENSE_PANEL, hipLaunchKernelGGL(k_dense_panel, dim3((m + 2) / 2), dim3(kDensePanelNT), 0, s, d, K));
                if (m > 0)
                    LAUNCH(K_DENSE_UPDATE, hipLaunchKernelGGL(k_dense_update, dim3(m * (m + 1) / 2), dim3(64), 0, s, d, K));
            }
            LAUNCH(K_FACTOR, hipLaunchKernelGGL(k_dense_solve, dim3(1), dim3(kFacThreads), solve_lds, s, d));
        } else {
            LAUNCH(K_FACTOR, hipLaunchKernelGGL(k_rcs_factor, dim3(1), dim3(kFacThreads), solve_lds, s, d));
        }
    }
    // the factorisation kernels end with the pose update; without free poses it runs alone
    if (d.n == 0 && d.n_kf > 0) LAUNCH(K_POSE_UPDATE, hipLaunchKernelGGL(k_pose_update, dim3(1), dim3(kBlock), 0, s, d));
    if (d.n_lm > 0) {
        LAUNCH(K_LM_UPDATE, hipLaunchKernelGGL(k_lm_solve, dim3(d.n_lms_blocks, d.spec_max), dim3(kLmsNT), 0, s, d));
    }
    if (d.sharded) {
        LAUNCH(K_PACK, hipLaunchKernelGGL(k_decide_pack, dim3(1), dim3(kBlock), 0, s, d));
        COMM(d.red_dec_loc, d.red_dec, 3);
    }
    if (!(d.fold && d.n_lm > 0))  // (folded into the last k_lm_solve workgroup otherwise)
        LAUNCH(K_DECIDE, hipLaunchKernelGGL(k_decide, dim3(1), dim3(kBlock), 0, s, d));
    return PLBA_OK;
}

void destroy_graphs(plba_ctx *ctx) {
    if (ctx->step_exec) (void)hipGraphExecDestroy(ctx->step_exec);
    if (ctx->step_graph) (void)hipGraphDestroy(ctx->step_graph);
    ctx->step_exec = nullptr;
    ctx->step_graph = nullptr;
    for (int i = 0; i < plba_ctx::kMultiLevels; ++i) {
        if (ctx->multi_exec[i]) (void)hipGraphExecDestroy(ctx->multi_exec[i]);
        if (ctx->multi_graph[i]) (void)hipGraphDestroy(ctx->multi_graph[i]);
        ctx->multi_exec[i] = nullptr;
        ctx->multi_graph[i] = nullptr;
    }
}

int capture_steps(plba_ctx *ctx, int nsteps, hipGraph_t &graph, hipGraphExec_t &exec) {
    const bool t = ctx->timing;
    ctx->timing = false;
    PLBA_CHECK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    for (int i = 0; i < nsteps && !rc; ++i) rc = launch_step(ctx);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    ctx->timing = t;
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess) {
        ctx->set_error("graph capture failed: %s", hipGetErrorString(e));
        return PLBA_E_DEVICE;
    }
    if (exec) {  // a previous window's executable graph: update it in place when the topology matches
        hipGraphNode_t bad = nullptr;
        hipGraphExecUpdateResult res = hipGraphExecUpdateSuccess;
        if (hipGraphExecUpdate(exec, g, &bad, &res) == hipSuccess && res == hipGraphExecUpdateSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            graph = g;
            return PLBA_OK;
        }
        (void)hipGetLastError();
        (void)hipGraphExecDestroy(exec);
        exec = nullptr;
    }
    if (graph) (void)hipGraphDestroy(graph);
    graph = g;
    PLBA_CHECK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
    return PLBA_OK;
}
// Which kernels (template instances) a step launches, in which order: an executable graph is
// updated in place only for a window with the same signature (hipGraphExecUpdate changes kernel
// arguments and grids, never the kernel a node runs).
std::vector<int64_t> launch_signature(const plba_ctx *ctx) {
    const Dev &d = ctx->d;
    return {d.E > 0, d.nf > 0, d.n_lm > 0, d.n > 0, d.nch > 0, d.band_mode, d.dense_mfma, d.dense_mfma ? d.ntiles : 0,
            d.bw, d.bcr, d.bcr_fused, d.cl, d.twisted, d.sharded, d.xg_P, d.fold, d.fold_init, d.n_kf > 0, d.spec_max,
            (int64_t)ctx->tuning.chunk_direct, (int64_t)chunk_half(ctx), (int64_t)ctx->comm.kind};
}
int capture_step(plba_ctx *ctx) {
    if (ctx->step_exec && !ctx->graphs_stale) return PLBA_OK;
    ctx->graphs_stale = false;
    const std::vector<int64_t> sig = launch_signature(ctx);
    if (ctx->step_exec && sig != ctx->graph_sig) destroy_graphs(ctx);  // different kernels: rebuild
    ctx->graph_sig = sig;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = capture_steps(ctx, 1, ctx->step_graph, ctx->step_exec);
    for (int i = 0; i < ctx->tuning.graph_levels && !rc; ++i)  // 2, 4, .. 2^L steps
        rc = capture_steps(ctx, 2 << i, ctx->multi_graph[i], ctx->multi_exec[i]);
    if (ctx->tuning.timing)
        fprintf(stderr, "[plba upload] %-24s %8.3f ms\n", "graph capture",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}
// launch n replays of the step as the binary decomposition of n over the captured graphs
int launch_steps_graph(plba_ctx *ctx, int n) {
    const int L = ctx->tuning.graph_levels;
    if (L == 0) {
        for (int i = 0; i < n; ++i) PLBA_CHECK(hipGraphLaunch(ctx->step_exec, ctx->stream));
        return PLBA_OK;
    }
    while (n >= (2 << (L - 1))) {
        PLBA_CHECK(hipGraphLaunch(ctx->multi_exec[L - 1], ctx->stream));
        n -= 2 << (L - 1);
    }
    for (int i = L - 1; i >= 0; --i)
        if (n & (2 << i)) PLBA_CHECK(hipGraphLaunch(ctx->multi_exec[i], ctx->stream));
    if (n & 1) PLBA_CHECK(hipGraphLaunch(ctx->step_exec, ctx->stream));
    return PLBA_OK;
}

// One poll of a schedule: the control block and the per-iteration trace (all kTraceCap records:
// how many are valid is in the control block the same poll reads) into the pinned block, one wait.
int read_ctrl(plba_ctx *ctx) {
    PLBA_CHECK(hipMemcpyAsync(ctx->h_ctrl, ctx->d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, ctx->stream));
    PLBA_CHECK(hipMemcpyAsync(ctx->h_trace, ctx->d.trace, sizeof(plba_iter_trace) * kTraceCap, hipMemcpyDeviceToHost, ctx->stream));
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    return PLBA_OK;
}


// Copies of the state a schedule starts from (BCR windows only): save = true before the first
// batch, save = false to put it back after a hand-off timeout.
int bcr_state_copy(plba_ctx *ctx, bool save) {
    Dev &d = ctx->d;
    const int c = ctx->cur;
    hipStream_t s = ctx->stream;
    auto cp = [&](void *bk, void *live, size_t bytes) -> hipError_t {
        if (!bytes) return hipSuccess;
        return save ? hipMemcpyAsync(bk, live, bytes, hipMemcpyDeviceToDevice, s)
                    : hipMemcpyAsync(live, bk, bytes, hipMemcpyDeviceToDevice, s);
    };
    PLBA_CHECK(cp(ctx->bk_T, d.Tb[c], sizeof(double) * (size_t)d.n_kf * 12));
    PLBA_CHECK(cp(ctx->bk_X, d.Xb[c], sizeof(double) * (size_t)d.n_lm * 4));
    PLBA_CHECK(cp(ctx->bk_xp, d.xp, sizeof(double) * (size_t)d.n));
    PLBA_CHECK(cp(ctx->bk_xk, d.xk[c], sizeof(double) * (size_t)d.n_kf * 6));
    PLBA_CHECK(cp(ctx->bk_Lpb, d.Lpb[c], sizeof(double) * (size_t)d.n_ln * 8));
    PLBA_CHECK(cp(ctx->bk_XL, d.XL[c], sizeof(double) * (size_t)ctx->n_ln * 6));
    PLBA_CHECK(cp(ctx->bk_level, d.e_level, (size_t)d.E));
    PLBA_CHECK(cp(ctx->bk_xl, d.xl, sizeof(double) * (size_t)d.n_lm * 4));
    return PLBA_OK;
}

// Sharded windows: every rank learns whether any rank hit a hand-off timeout in this batch, so
// that all of them fall back together (a collective cannot be re-run by one rank alone).
int agree_dev_error(plba_ctx *ctx, int mine, int *any) {
    *any = mine;
    if (!ctx->d.sharded) return PLBA_OK;
    double *buf = ctx->d.red_dec_loc + 3;  // spare slot after the three decision terms
    const double v = mine ? 1.0 : 0.0;
    PLBA_CHECK(hipMemcpyAsync(buf, &v, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    int rc = allreduce(ctx, buf, buf, 1);
    if (rc) return rc;
    double out = 0.0;
    PLBA_CHECK(hipMemcpyAsync(&out, buf, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    *any = out != 0.0 ? 1 : 0;
    return PLBA_OK;
}

// computeError() on the edges of `level` at the device's current state. when_done: queued as a
// schedule's epilogue before the control block is polled (k_refresh does nothing then unless the
// schedule has finished).
int launch_refresh(plba_ctx *ctx, int level, bool when_done) {
    if (ctx->d.E > 0) hipLaunchKernelGGL(k_refresh, dim3(blocks_for(ctx->d.E)), dim3(kBlock), 0, ctx->stream, ctx->d, level, when_done ? 1 : 0); PLBA_LAUNCHED(ctx, "k_refresh");
    PLBA_CHECK(hipGetLastError());
    return PLBA_OK;
}

// Run a schedule of 1 or 2 optimize() calls entirely on the device: replay the step graph in
// batches, polling the control block once per batch.
// refresh_level >= 0: the caller's epilogue, computeError() on that level's edges at the final
// state. It is queued behind every batch, before the poll (k_refresh's when_done: it reads the
// current buffers from the device control block and does nothing until the schedule has finished),
// so the batch that finishes the schedule needs no wait of its own for it: one host wait per solve
// when the first batch was long enough.
// every launch outside the step graphs is checked where it is issued (PLBA_LAUNCHED; the graph
// launches are checked by LAUNCH / launch_band)
int run_schedule_once(plba_ctx *ctx, const Ctrl &init, int refresh_level, bool &dev_error) {
    dev_error = false;
    Dev &d = ctx->d;
    *ctx->h_ctrl = init;
    PLBA_CHECK(hipMemcpyAsync(d.ctrl, ctx->h_ctrl, sizeof(Ctrl), hipMemcpyHostToDevice, ctx->stream));
    if (d.n_ln > 0 && !lm_hand_rolled(init.hlm)) {  // Plücker vectors of the current line states (read by k_linearize;
                                     // the hand-rolled LM starts from the map's NDw, uploaded instead)
        hipLaunchKernelGGL(k_line_pluker, dim3(blocks_for(d.n_ln)), dim3(kBlock), 0, ctx->stream, d); PLBA_LAUNCHED(ctx, "k_line_pluker");
        PLBA_CHECK(hipGetLastError());
    }
    // the host transport synchronises inside the step: no graph then
    bool use_graph = !ctx->timing && ctx->comm.kind != plba_ctx::Comm::HOST && !ctx->no_graph;
    // A new window's step graphs are captured (or updated) on the host while the device runs the
    // first batch, launched directly: the capture leaves the end-to-end call's critical path.
    bool capture_pending = use_graph && (!ctx->step_exec || ctx->graphs_stale);
    auto capture_now = [&]() -> int {
        capture_pending = false;
        int rc = capture_step(ctx);
        if (rc) {
            // a step that cannot be captured (collectives that refuse stream capture, graph
            // instantiation failing for lack of memory): the first batch is already running as
            // direct launches, so keep launching that way for the rest of this context's life
            (void)hipGetLastError();
            destroy_graphs(ctx);
            ctx->no_graph = true;
            use_graph = false;
            if (ctx->opts.verbose) fprintf(stderr, "[plba] step capture failed (%s); direct launches\n", ctx->err.c_str());
            ctx->err.clear();
        }
        return PLBA_OK;
    };
    int launched = 0;
    int batch = std::max(4, ctx->last_steps);
    const bool tlog = ctx->tuning.timing;
    auto tb0 = std::chrono::steady_clock::now();
    const int max_steps = init.n_stages * 10 * (init.max_iters[0] + init.max_iters[1] + 2) + 8;
    for (;;) {
        if (use_graph && !capture_pending) {
            int rc = launch_steps_graph(ctx, batch);
            if (rc) return rc;
        } else {
            for (int b = 0; b < batch; ++b) {
                int rc = launch_step(ctx);
                if (rc) return rc;
            }
            if (capture_pending)
                if (int rc = capture_now()) return rc;
        }
        launched += batch;
        int rc = refresh_level >= 0 ? launch_refresh(ctx, refresh_level, true) : PLBA_OK;
        if (rc) return rc;
        if ((rc = read_ctrl(ctx))) return rc;
        if (tlog) {
            const auto tb1 = std::chrono::steady_clock::now();
            fprintf(stderr, "[plba schedule] batch of %3d steps (%3d so far, device step %3d) %8.3f ms\n", batch, launched,
                    ctx->h_ctrl->steps, std::chrono::duration<double, std::milli>(tb1 - tb0).count());
            tb0 = tb1;
        }
        int any_error = ctx->h_ctrl->dev_error;
        if (d.sharded && d.bcr && (rc = agree_dev_error(ctx, any_error, &any_error))) return rc;
        if (any_error) {
            dev_error = true;
            ctx->set_error("a bounded in-kernel hand-off wait timed out");
            return PLBA_E_DEVICE;
        }
        if (ctx->h_ctrl->all_done) break;
        if (launched >= max_steps) {
            ctx->set_error("LM schedule did not terminate after %d steps", launched);
            return PLBA_E_STATE;
        }
        // steps still needed: at least one per remaining trial; keep batches small near the end
        batch = 4;
    }
    ctx->steps_launched = launched;
    ctx->last_steps = std::max(4, ctx->h_ctrl->steps + 1);
    ctx->cur = ctx->h_ctrl->cur;
    ctx->last_ok = ctx->h_ctrl->last_ok;
    ctx->chi_src = ctx->h_ctrl->chi_src;
    // per-iteration trace written by k_decide (read by the poll that saw the schedule finish)
    const int nt = std::min(ctx->h_ctrl->ntrace, kTraceCap);
    ctx->trace.insert(ctx->trace.end(), ctx->h_trace, ctx->h_trace + nt);
    return PLBA_OK;
}

// run_schedule_once with the BCR safety net: the starting state is copied first; if a hand-off
// wait times out (Ctrl::dev_error — every later kernel of that batch is a no-op), the state is put
// back, the window is switched to the column-lane factorisation for the rest of this context's
// life (its arrays were allocated with the BCR ones) and the same schedule runs again, in this
// process. Sharded windows agree on the error first, so every rank falls back together.
int run_schedule(plba_ctx *ctx, const Ctrl &init, int refresh_level = -1) {
    Dev &d = ctx->d;
    int rc;
    if (d.bcr && (rc = bcr_state_copy(ctx, true))) return rc;
    bool dev_error = false;
    rc = run_schedule_once(ctx, init, refresh_level, dev_error);
    if (!rc || !dev_error || !d.bcr) return rc;
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    if ((rc = bcr_state_copy(ctx, false))) return rc;
    if (ctx->opts.verbose)
        fprintf(stderr, "[plba] BCR hand-off timed out; re-solving with the column-lane factorisation\n");
    destroy_graphs(ctx);
    apply_plan(d, ctx->plan.fallback);
    ctx->no_bcr = true;
    ++ctx->bcr_fallbacks;
    ctx->err.clear();
    rc = run_schedule_once(ctx, init, refresh_level, dev_error);
    return rc;
}

Ctrl schedule_init(plba_ctx *ctx, int n_stages) {
    Ctrl c{};
    c.stage = -1;
    c.n_stages = n_stages;
    c.switch_pending = 1;
    c.solve_ok[0] = 1;
    c.max_trials = ctx->opts.max_trials;
    c.cur = ctx->cur;
    c.last_ok = ctx->last_ok;
    c.chi_src = ctx->chi_src;
    c.spec_w = 1;
    return c;
}

int do_optimize(plba_ctx *ctx, int iterations, int32_t *iters_done, double *final_chi2) {
    Ctrl c = schedule_init(ctx, 1);
    c.max_iters[0] = iterations;
    c.stage_robust[0] = ctx->robust;
    c.stage_level[0] = ctx->level;
    c.stage_classify[0] = 0;
    if (iterations <= 0) {
        if (iters_done) *iters_done = 0;
        if (final_chi2) *final_chi2 = 0.0;
        return PLBA_OK;
    }
    int rc = run_schedule(ctx, c);
    if (rc) return rc;
    if (iters_done) *iters_done = ctx->h_ctrl->iters_done[0];
    if (final_chi2) *final_chi2 = ctx->h_ctrl->chi2_final[0];
    return PLBA_OK;
}

// Sharded windows: whole-window landmark states and per-edge outputs on every rank
// (one all-reduce of a zero-filled, scattered buffer). Collective: all ranks call it.
int gather_outputs(plba_ctx *ctx, std::vector<double> &out) {
    Dev &d = ctx->d;
    const size_t n = (size_t)d.n_lm_g * 4 + 3 * (size_t)d.E_g;
    PLBA_CHECK(hipMemsetAsync(d.gat, 0, n * sizeof(double), ctx->stream));
    if (d.Ep) hipLaunchKernelGGL(k_depth, dim3(blocks_for(d.Ep)), dim3(kBlock), 0, ctx->stream, d, ctx->d_depth); PLBA_LAUNCHED(ctx, "k_depth");
    const int m = std::max(d.n_lm, d.E);
    if (m) hipLaunchKernelGGL(k_gather, dim3(blocks_for(m)), dim3(kBlock), 0, ctx->stream, d, ctx->d_depth); PLBA_LAUNCHED(ctx, "k_gather");
    PLBA_CHECK(hipGetLastError());
    int rc = allreduce(ctx, d.gat, d.gat, n);
    if (rc) return rc;
    out.resize(n);
    PLBA_CHECK(hipMemcpyAsync(out.data(), d.gat, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    return PLBA_OK;
}

// Unsharded windows: every requested output in the caller's order, scattered on the device
// (k_out_scatter) into one staging block, one copy into pinned memory, one synchronisation, then
// host copies into the caller's arrays.
int download_outputs(plba_ctx *ctx, double *kf_Tcw, double *pt_xyz, double *ln_orth, double *ept_chi2,
                     uint8_t *ept_depth_ok, double *eln_chi2, uint8_t *ept_level, uint8_t *eln_level) {
    Dev &d = ctx->d;
    hipStream_t s = ctx->stream;
    const size_t nk = (size_t)d.n_kf, np = (size_t)d.n_pt, nl = (size_t)d.n_ln, Ep = (size_t)d.Ep, El = (size_t)d.El;
    const size_t nd = out_doubles(nk, np, nl, Ep + El), bytes = nd * sizeof(double) + Ep + (Ep + El);
    const int m = std::max({d.n_lm, d.E, d.n_kf});
    const bool any = kf_Tcw || pt_xyz || ln_orth || ept_chi2 || ept_depth_ok || eln_chi2 || ept_level || eln_level;
    if (!m || !any) return PLBA_OK;
    if (bytes > ctx->h_out_cap) {  // grow-only, with slack: the next windows of a session are similar
        PLBA_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->retire_pinned(ctx->h_out);
        ctx->h_out = nullptr;
        ctx->h_out_cap = 0;
        const size_t cap = bytes + bytes / 2;
        PLBA_CHECK(hipHostMalloc((void **)&ctx->h_out, cap));
        ctx->h_out_cap = cap;
    }
    hipLaunchKernelGGL(k_out_scatter, dim3(blocks_for(m)), dim3(kBlock), 0, s, d, ctx->d_outd, ept_depth_ok ? 1 : 0,
                       ctx->cur, ctx->chi_src); PLBA_LAUNCHED(ctx, "k_out_scatter");
    PLBA_CHECK(hipGetLastError());
    PLBA_CHECK(hipMemcpyAsync(ctx->h_out, ctx->d_outd, bytes, hipMemcpyDeviceToHost, s));
    PLBA_CHECK(hipStreamSynchronize(s));
    const double *od = reinterpret_cast<const double *>(ctx->h_out);
    const uint8_t *ob = reinterpret_cast<const uint8_t *>(od + nd);
    auto put = [](void *dst, const void *src, size_t b) {
        if (dst && b) std::memcpy(dst, src, b);
    };
    put(kf_Tcw, od, sizeof(double) * nk * 12);
    put(pt_xyz, od + nk * 12, sizeof(double) * np * 3);
    put(ln_orth, od + nk * 12 + np * 3, sizeof(double) * nl * 4);
    put(ept_chi2, od + nk * 12 + np * 3 + nl * 4, sizeof(double) * Ep);
    put(eln_chi2, od + nk * 12 + np * 3 + nl * 4 + Ep, sizeof(double) * El);
    put(ept_depth_ok, ob, Ep);
    put(ept_level, ob + Ep, Ep);
    put(eln_level, ob + 2 * Ep, El);
    return PLBA_OK;
}

}  // namespace

#include "plba_pgo_driver.hpp"

// ==================================================================================== C ABI
extern "C" {

void plba_default_opts(plba_opts *o) {
    if (!o) return;
    o->device = 0;
    o->corrected_line_jacobian = 0;
    o->verbose = 0;
    o->max_trials = 10;
    o->tau = 1e-5;
}

// The device's default memory pool is process-wide: its release threshold is raised while at
// least one context of the device lives and the value found before the first one is put back when
// the last one is destroyed (other users of the pool in the process see their own setting again).
void pool_hold(plba_ctx *ctx, bool on) {
    static std::mutex mu;
    static std::map<int, std::pair<int, uint64_t>> held;  // device -> (contexts holding, previous threshold)
    if (ctx->pool_hold == on) return;
    std::lock_guard<std::mutex> lk(mu);
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, ctx->opts.device) != hipSuccess || !pool) {
        (void)hipGetLastError();
        return;
    }
    auto &h = held[ctx->opts.device];
    if (on) {
        if (h.first++ == 0) {
            uint64_t prev = 0;
            if (hipMemPoolGetAttribute(pool, hipMemPoolAttrReleaseThreshold, &prev) != hipSuccess) prev = 0;
            h.second = prev;
            uint64_t thr = UINT64_MAX;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
        }
    } else if (--h.first == 0) {
        uint64_t prev = h.second;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &prev);
    }
    (void)hipGetLastError();
    ctx->pool_hold = on;
}

// A three-keyframe window with points and a line solved once through the whole path (device
// build, step graphs, every kernel of a step, output scatter); the context is left without a
// window, as plba_create returns it.
int prewarm(plba_ctx *ctx) {
    // Device memory: windows are carved from stream-ordered allocations (hipMallocAsync); keep what
    // they free in the device's default pool (release threshold: never) and grow the pool once
    // here (PLBA_PREWARM_MB, default 256 MB of the 288 GB), so that a first window does not pay
    // the pool's growth; the first pinned upload staging likewise.
    {
        pool_hold(ctx, true);
        const char *mb = getenv("PLBA_PREWARM_MB");
        const size_t bytes = (size_t)(mb && mb[0] ? std::max(0, atoi(mb)) : 256) << 20;
        void *p = nullptr;
        if (bytes && hipMallocAsync(&p, bytes, ctx->stream) == hipSuccess) (void)hipFreeAsync(p, ctx->stream);
        (void)hipGetLastError();
        constexpr size_t kStage = 8u << 20;
        if (!ctx->staging && hipHostMalloc((void **)&ctx->staging, kStage, hipHostMallocDefault) == hipSuccess)
            ctx->staging_cap = kStage;
        (void)hipGetLastError();
        PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    }
    // a window of nk poses, np points and nl lines, each landmark seen by two consecutive poses:
    // large enough that the device build takes its full-size sort paths (first-call costs of a
    // small window differ from a real one's)
    const int nk = 8, np = 4096, nl = 256, nep = 2 * np, nel = 2 * nl;
    std::vector<double> T((size_t)nk * 12, 0.0), P((size_t)np * 3), L((size_t)nl * 4), eobs((size_t)nep * 2),
        einfo(nep, 1.0), lobs((size_t)nel * 4), linfo(nel, 1.0);
    std::vector<uint8_t> fixed(nk, 0);
    std::vector<int32_t> kf_id(nk), pt_id(np), ln_id(nl), elm(nep), ekf(nep), llm(nel), lkf(nel);
    fixed[0] = 1;
    for (int k = 0; k < nk; ++k) {
        T[(size_t)k * 12 + 0] = T[(size_t)k * 12 + 5] = T[(size_t)k * 12 + 10] = 1.0;
        T[(size_t)k * 12 + 3] = -0.1 * k;  // t_x
        kf_id[k] = k;
    }
    const double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375;
    for (int l = 0; l < np; ++l) {
        pt_id[l] = nk + l;
        P[(size_t)l * 3] = -1.0 + 2.0 * ((l * 37) % 101) / 101.0;
        P[(size_t)l * 3 + 1] = -0.8 + 1.6 * ((l * 53) % 97) / 97.0;
        P[(size_t)l * 3 + 2] = 4.0 + 3.0 * ((l * 29) % 89) / 89.0;
        for (int o = 0; o < 2; ++o) {
            const int e = 2 * l + o, k = (l + o) % nk;
            elm[e] = l;
            ekf[e] = k;
            const double x = P[(size_t)l * 3] + T[(size_t)k * 12 + 3], y = P[(size_t)l * 3 + 1], z = P[(size_t)l * 3 + 2];
            eobs[(size_t)e * 2] = fx * x / z + cx + 0.3;
            eobs[(size_t)e * 2 + 1] = fy * y / z + cy - 0.2;
        }
    }
    for (int l = 0; l < nl; ++l) {
        ln_id[l] = nk + np + 1 + l;
        L[(size_t)l * 4] = 0.3 + 0.001 * l;
        L[(size_t)l * 4 + 1] = -0.2;
        L[(size_t)l * 4 + 2] = 0.4;
        L[(size_t)l * 4 + 3] = 0.5;
        for (int o = 0; o < 2; ++o) {
            const int e = 2 * l + o;
            llm[e] = l;
            lkf[e] = (l + o) % nk;
            const double q[4] = {300.0 + l % 7, 200.0 + o, 420.0, 260.0 + l % 5};
            for (int c = 0; c < 4; ++c) lobs[(size_t)e * 4 + c] = q[c];
        }
    }
    plba_graph g{};
    g.n_kf = nk; g.n_pt = np; g.n_ln = nl; g.n_ept = nep; g.n_eln = nel;
    g.fx = fx; g.fy = fy; g.cx = cx; g.cy = cy;
    g.kf_Tcw = T.data(); g.kf_fixed = fixed.data(); g.kf_id = kf_id.data();
    g.pt_xyz = P.data(); g.pt_id = pt_id.data(); g.ln_orth = L.data(); g.ln_id = ln_id.data();
    g.ept_lm = elm.data(); g.ept_kf = ekf.data(); g.ept_obs = eobs.data(); g.ept_info = einfo.data();
    g.eln_lm = llm.data(); g.eln_kf = lkf.data(); g.eln_obs = lobs.data(); g.eln_info = linfo.data();
    g.huber_pt = g.huber_ln = (double)(float)2.4476519360399;
    int rc = plba_upload(ctx, &g);
    if (rc) return rc;
    std::vector<double> Tout((size_t)nk * 12);
    plba_result res{};
    res.kf_Tcw = Tout.data();
    rc = plba_lba_plucker(ctx, &res);
    ctx->uploaded = false;  // no window: calls before the caller's own upload stay PLBA_E_STATE
    ctx->initialized = false;
    ctx->no_bcr = false;    // (a diagnostic forcing BCR timeouts must not carry over to real windows)
    ctx->bcr_fallbacks = 0;
    return rc;
}

int plba_create(plba_ctx **out, const plba_opts *opts) {
    if (!out) return PLBA_E_INVALID;
    *out = nullptr;
    plba_ctx *ctx = new (std::nothrow) plba_ctx();
    if (!ctx) return PLBA_E_NOMEM;
    if (opts) ctx->opts = *opts;
    else plba_default_opts(&ctx->opts);
    if (ctx->opts.max_trials <= 0) ctx->opts.max_trials = 10;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        delete ctx;
        return PLBA_E_DEVICE;
    }
    if (ctx->opts.device < 0 || ctx->opts.device >= ndev || hipSetDevice(ctx->opts.device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&ctx->h_ctrl, kCtrlBlock + sizeof(plba_iter_trace) * kTraceCap, hipHostMallocDefault) != hipSuccess) {
        delete ctx;
        return PLBA_E_DEVICE;
    }
    std::memset(ctx->h_ctrl, 0, kCtrlBlock + sizeof(plba_iter_trace) * kTraceCap);
    ctx->h_trace = reinterpret_cast<plba_iter_trace *>(reinterpret_cast<char *>(ctx->h_ctrl) + kCtrlBlock);
    *out = ctx;
    // Pre-warm (PLBA_NO_PREWARM=1 skips it): the first window of a process otherwise pays the
    // code-object load, the first rocPRIM sorts of the device window build and the first pinned
    // staging (C3: first upload 38 ms against 1.2 ms warm) on the LBA thread's first keyframe.
    const char *npw = getenv("PLBA_NO_PREWARM");
    // A failed pre-warm (a diagnostic switch in the caller's environment, say) is not fatal: the
    // context is returned without a window, as it would be without the pre-warm, and the reason is
    // kept in plba_last_error and printed once. A device that cannot run a kernel fails the caller's
    // own first upload or solve instead.
    if (!(npw && npw[0] == '1')) {
        const int rc = prewarm(ctx);
        if (rc) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(ctx->stream);
            ctx->uploaded = false;
            ctx->initialized = false;
            ctx->no_bcr = false;
            ctx->bcr_fallbacks = 0;
            ctx->set_error("pre-warm failed (%d): %s (continuing without it)", rc, ctx->err.c_str());
            fprintf(stderr, "[plba] %s\n", ctx->err.c_str());
        }
    }
    return PLBA_OK;
}

int plba_destroy(plba_ctx *ctx) {
    if (!ctx) return PLBA_OK;
    (void)hipSetDevice(ctx->opts.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ctx->free_all();
    destroy_graphs(ctx);
    if (ctx->arena) (void)hipFreeAsync(ctx->arena, ctx->stream);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->staging) (void)hipHostFree(ctx->staging);
    for (void *p : ctx->retired) (void)hipHostFree(p);
    for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->h_ctrl) (void)hipHostFree(ctx->h_ctrl);
    ctx->bmemA.release(ctx->stream);
    ctx->bmemB.release(ctx->stream);
    std::vector<ScratchBlock *> blocks{&ctx->pgo, &ctx->lc, &ctx->track, &ctx->match, &ctx->bow_io};
    for (BowSlot &b : ctx->bow) blocks.insert(blocks.end(), {&b.voc, &b.db_word, &b.db_val});
    for (ScratchBlock *sb : blocks) sb->release(ctx->stream);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (ScratchBlock *sb : blocks) sb->release_host();
    if (ctx->h_out) (void)hipHostFree(ctx->h_out);
    if (ctx->comm.hbuf) (void)hipHostFree(ctx->comm.hbuf);
    if (ctx->comm.nccl) (void)ncclCommDestroy(ctx->comm.nccl);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    pool_hold(ctx, false);
    delete ctx;
    return PLBA_OK;
}

const char *plba_last_error(const plba_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int plba_upload(plba_ctx *ctx, const plba_graph *g) {
    if (!ctx) return PLBA_E_INVALID;
    (void)hipSetDevice(ctx->opts.device);
    ctx->robust = 1;
    ctx->trace.clear();
    return do_upload(ctx, g);
}

int plba_reset_estimates(plba_ctx *ctx) {
    if (!ctx || !ctx->uploaded) return ctx ? PLBA_E_STATE : PLBA_E_INVALID;
    Dev &d = ctx->d;
    ctx->cur = ctx->last_ok = ctx->chi_src = 0;
    // one launch for every array (k_reset_estimates): sized by the longest range, capped — the
    // kernel strides
    const size_t longest = std::max({(size_t)d.n_kf * 12, (size_t)d.n_lm * 4, (size_t)d.E, (size_t)d.n, (size_t)1});
    const int blocks = (int)std::min((longest + kBlock - 1) / kBlock, (size_t)2048);
    hipLaunchKernelGGL(k_reset_estimates, dim3(blocks), dim3(kBlock), 0, ctx->stream, d); PLBA_LAUNCHED(ctx, "k_reset_estimates");
    PLBA_CHECK(hipGetLastError());
    std::fill(ctx->h_level.begin(), ctx->h_level.end(), 0);
    ctx->robust = 1;
    ctx->initialized = false;
    ctx->trace.clear();
    return PLBA_OK;
}

int plba_set_edge_levels(plba_ctx *ctx, const uint8_t *ept_level, const uint8_t *eln_level) {
    if (!ctx) return PLBA_E_INVALID;
    if (!ctx->uploaded) return PLBA_E_STATE;
    const int E = ctx->d.E;
    std::vector<uint8_t> lv(E, 0);
    for (int e = 0; e < E; ++e) {
        int o = ctx->e_orig[e];
        bool is_pt = e < ctx->d.Ep;
        lv[e] = is_pt ? (ept_level ? ept_level[o] : 0) : (eln_level ? eln_level[o] : 0);
    }
    ctx->h_level = lv;
    // on the solver stream (ordered after a pending plba_reset_estimates launch), then wait:
    // lv is a local buffer
    if (E) {
        PLBA_CHECK(hipMemcpyAsync(ctx->d.e_level, lv.data(), E, hipMemcpyHostToDevice, ctx->stream));
        PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    }
    ctx->initialized = false;
    return PLBA_OK;
}

int plba_set_robust(plba_ctx *ctx, int32_t robust) {
    if (!ctx) return PLBA_E_INVALID;
    ctx->robust = robust ? 1 : 0;
    return PLBA_OK;
}

int plba_initialize_optimization(plba_ctx *ctx, int32_t level) {
    if (!ctx) return PLBA_E_INVALID;
    if (!ctx->uploaded) return PLBA_E_STATE;
    ctx->level = level;  // activation runs on the device at the start of the next optimize()
    ctx->initialized = true;
    return PLBA_OK;
}

int plba_optimize(plba_ctx *ctx, int32_t iterations, int32_t *iters_done, double *final_chi2) {
    if (!ctx) return PLBA_E_INVALID;
    if (!ctx->uploaded || !ctx->initialized) return PLBA_E_STATE;
    (void)hipSetDevice(ctx->opts.device);
    ctx->trace.clear();
    return do_optimize(ctx, iterations, iters_done, final_chi2);
}

int plba_refresh_edge_errors(plba_ctx *ctx, int32_t level) {
    if (!ctx) return PLBA_E_INVALID;
    if (!ctx->uploaded) return PLBA_E_STATE;
    return launch_refresh(ctx, level, false);
}

int plba_get_edge_chi2(plba_ctx *ctx, double *ept_chi2, uint8_t *ept_depth_ok, double *eln_chi2) {
    if (!ctx) return PLBA_E_INVALID;
    if (!ctx->uploaded) return PLBA_E_STATE;
    Dev &d = ctx->d;
    if (d.sharded) {
        std::vector<double> gv;
        int rc = gather_outputs(ctx, gv);
        if (rc) return rc;
        const double *o = gv.data() + (size_t)d.n_lm_g * 4;
        for (int e = 0; e < ctx->Ep; ++e) {
            if (ept_chi2) ept_chi2[e] = o[e];
            if (ept_depth_ok) ept_depth_ok[e] = (uint8_t)o[(size_t)d.E_g + e];
        }
        for (int e = 0; e < ctx->El && eln_chi2; ++e) eln_chi2[e] = o[ctx->Ep + e];
        return PLBA_OK;
    }
    return download_outputs(ctx, nullptr, nullptr, nullptr, ept_chi2, ept_depth_ok, eln_chi2, nullptr, nullptr);
}

int plba_download(plba_ctx *ctx, double *kf_Tcw, double *pt_xyz, double *ln_orth) {
    if (!ctx) return PLBA_E_INVALID;
    if (!ctx->uploaded) return PLBA_E_STATE;
    Dev &d = ctx->d;
    if (d.sharded) {  // poses are replicated; landmarks come from the gather
        std::vector<double> gv;
        int rc = gather_outputs(ctx, gv);
        if (rc) return rc;
        if (kf_Tcw && d.n_kf)
            PLBA_CHECK(d2h(ctx, kf_Tcw, d.Tb[ctx->cur], sizeof(double) * (size_t)d.n_kf * 12));
        for (int p = 0; p < ctx->n_pt && pt_xyz; ++p)
            for (int k = 0; k < 3; ++k) pt_xyz[3 * p + k] = gv[(size_t)p * 4 + k];
        for (int l = 0; l < ctx->n_ln && ln_orth; ++l)
            for (int k = 0; k < 4; ++k) ln_orth[4 * l + k] = gv[(size_t)(ctx->n_pt + l) * 4 + k];
        return PLBA_OK;
    }
    return download_outputs(ctx, kf_Tcw, pt_xyz, ln_orth, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// The whole schedule of src/mapHandler.cpp:6119-6160 (stage 1, classification, stage 2,
// level-1 refresh) with no host round trip except the per-trial control read.
int plba_lba_plucker(plba_ctx *ctx, plba_result *res) {
    if (!ctx) return PLBA_E_INVALID;
    if (!ctx->uploaded) return PLBA_E_STATE;
    (void)hipSetDevice(ctx->opts.device);
    Dev &d = ctx->d;
    ctx->trace.clear();
    for (int k = 0; k < K_COUNT; ++k) { ctx->k_ms[k] = 0; ctx->k_n[k] = 0; }
    auto t0 = std::chrono::steady_clock::now();
    int rc;
    // stage 1: level 0, Huber; classification; stage 2: level 0, no kernel
    Ctrl c = schedule_init(ctx, 2);
    c.max_iters[0] = 5;
    c.max_iters[1] = 10;
    c.stage_robust[0] = 1;
    c.stage_robust[1] = 0;
    c.stage_level[0] = 0;
    c.stage_level[1] = 0;
    c.stage_classify[0] = 0;
    c.stage_classify[1] = 1;
    // the schedule, with computeError() on the level-1 edges at the final state as its epilogue
    // (done when the schedule's last poll returns)
    if ((rc = run_schedule(ctx, c, 1))) return rc;
    auto t1 = std::chrono::steady_clock::now();
    if ((rc = collect_timing(ctx))) return rc;
    ctx->robust = 0;
    ctx->level = 0;
    if (res) {
        res->iters[0] = ctx->h_ctrl->iters_done[0];
        res->iters[1] = ctx->h_ctrl->iters_done[1];
        res->chi2[0] = ctx->h_ctrl->chi2_final[0];
        res->chi2[1] = ctx->h_ctrl->chi2_final[1];
        res->solve_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        if (d.sharded) {  // one gather for every output
            std::vector<double> gv;
            if ((rc = gather_outputs(ctx, gv))) return rc;
            if (res->kf_Tcw && d.n_kf)
                PLBA_CHECK(d2h(ctx, res->kf_Tcw, d.Tb[ctx->cur], sizeof(double) * (size_t)d.n_kf * 12));
            for (int p = 0; p < ctx->n_pt && res->pt_xyz; ++p)
                for (int k = 0; k < 3; ++k) res->pt_xyz[3 * p + k] = gv[(size_t)p * 4 + k];
            for (int l = 0; l < ctx->n_ln && res->ln_orth; ++l)
                for (int k = 0; k < 4; ++k) res->ln_orth[4 * l + k] = gv[(size_t)(ctx->n_pt + l) * 4 + k];
            const double *o = gv.data() + (size_t)d.n_lm_g * 4;
            const size_t Eg = d.E_g;
            for (int e = 0; e < ctx->Ep; ++e) {
                if (res->ept_chi2) res->ept_chi2[e] = o[e];
                if (res->ept_depth_ok) res->ept_depth_ok[e] = (uint8_t)o[Eg + e];
                if (res->ept_level) res->ept_level[e] = (uint8_t)o[2 * Eg + e];
            }
            for (int e = 0; e < ctx->El; ++e) {
                if (res->eln_chi2) res->eln_chi2[e] = o[ctx->Ep + e];
                if (res->eln_level) res->eln_level[e] = (uint8_t)o[2 * Eg + ctx->Ep + e];
            }
            return PLBA_OK;
        }
        if ((rc = download_outputs(ctx, res->kf_Tcw, res->pt_xyz, res->ln_orth, res->ept_chi2, res->ept_depth_ok,
                                   res->eln_chi2, res->ept_level, res->eln_level)))
            return rc;
    }
    return PLBA_OK;
}

void plba_hlm_default_params(plba_hlm_params *p) {
    if (!p) return;
    p->lambda0 = 1e-5;          // src/slamConfig.cpp:65
    p->lambda_k = 10.0;         // :66
    p->homog_th = 1e-7;         // src2/config.cpp:80
    p->min_error = 1e-7;        // :84
    p->min_error_change = 1e-7; // :85
    p->max_iters = 15;          // src/slamConfig.cpp:67
    p->err_per_obs = 0;
    p->variant = PLBA_HLM_LBA_PLUCKER;
    p->pad = 0;
}

// MapHandler::levMarquardtOptimizationLBAForPluker (src/mapHandler.cpp:1618-2332) on the uploaded
// window: the captured step graph with the Ctrl::hlm variants of each kernel, one step per
// iteration (linearise -> [stop] -> Schur solve -> decide), no host round trip inside a batch.
int plba_hlm_lba(plba_ctx *ctx, const plba_hlm_state *st, const plba_hlm_params *p, plba_hlm_result *res) {
    if (!ctx || !st || (ctx->n_kf && !st->kf_x)) return PLBA_E_INVALID;
    if (!ctx->uploaded) return PLBA_E_STATE;
    (void)hipSetDevice(ctx->opts.device);
    plba_hlm_params prm;
    if (p) prm = *p;
    else plba_hlm_default_params(&prm);
    if (prm.max_iters < 1 || (prm.variant != PLBA_HLM_LBA_PLUCKER && prm.variant != PLBA_HLM_GBA &&
                              prm.variant != PLBA_HLM_LBA_ENDPOINTS)) {
        ctx->set_error("max_iters must be >= 1 and variant PLBA_HLM_LBA_PLUCKER, PLBA_HLM_GBA or PLBA_HLM_LBA_ENDPOINTS");
        return PLBA_E_INVALID;
    }
    // endpoint lines (6-dim landmarks line3D): GBA and levMarquardtOptimizationLBA (:2334-3016)
    const bool lba_ep = prm.variant == PLBA_HLM_LBA_ENDPOINTS;
    const bool gba = prm.variant == PLBA_HLM_GBA || lba_ep;
    if (!lba_ep && ctx->n_ln && !st->ln_pluker) return PLBA_E_INVALID;  // (the new variant never reads NDw)
    if (gba && ctx->n_ln && !st->ln_line3d) {
        ctx->set_error("the endpoint-line variants need state ln_line3d");
        return PLBA_E_INVALID;
    }
    if (gba && ctx->d.sharded) {
        ctx->set_error("the endpoint-line variants run on unsharded windows only");
        return PLBA_E_STATE;
    }
    int rc = plba_reset_estimates(ctx);
    if (rc) return rc;
    Dev &d = ctx->d;
    ctx->trace.clear();
    // X_aux pose blocks and the map's NDw (in this rank's device landmark order)
    std::vector<double> Lm((size_t)std::max(d.n_ln, 1) * 8, 0.0);
    for (int i = 0; i < d.n_ln && !gba; ++i) {
        const int gl = ctx->lm_gpos[d.n_pt + i] - ctx->n_pt;
        for (int k = 0; k < 6; ++k) Lm[(size_t)i * 8 + k] = st->ln_pluker[(size_t)gl * 6 + k];
    }
    if (d.n_kf) PLBA_CHECK(hipMemcpyAsync(d.xk[0], st->kf_x, sizeof(double) * (size_t)d.n_kf * 6, hipMemcpyHostToDevice, ctx->stream));
    if (d.n_ln && !gba)
        PLBA_CHECK(hipMemcpyAsync(d.Lpb[0], Lm.data(), sizeof(double) * Lm.size(), hipMemcpyHostToDevice, ctx->stream));
    if (ctx->n_ln && gba)
        PLBA_CHECK(hipMemcpyAsync(d.XL[0], st->ln_line3d, sizeof(double) * (size_t)ctx->n_ln * 6, hipMemcpyHostToDevice,
                                  ctx->stream));
    auto t0 = std::chrono::steady_clock::now();
    Ctrl c = schedule_init(ctx, 1);
    c.max_iters[0] = prm.max_iters;
    c.stage_robust[0] = 0;
    c.stage_level[0] = 0;
    c.hlm = lba_ep ? kLmLbaEndpoints : gba ? kLmGba : kLmLbaPlucker;
    c.hlm_lambda0 = prm.lambda0;
    c.hlm_k = prm.lambda_k;
    c.hlm_homog = prm.homog_th;
    c.hlm_minerr = prm.min_error;
    c.hlm_minchg = prm.min_error_change;
    c.hlm_nobs = prm.err_per_obs ? (double)(ctx->Ep + ctx->El) : 0.0;
    // :2796 divides by the landmark counts Npt + Nls from the second linearisation on
    c.hlm_nobs2 = prm.err_per_obs ? c.hlm_nobs : (double)(ctx->n_pt + ctx->n_ln);
    c.err_prev = 999999999.9;  // :1634
    rc = run_schedule(ctx, c);
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    auto t1 = std::chrono::steady_clock::now();
    if (rc) return rc;
    if ((rc = collect_timing(ctx))) return rc;
    ctx->robust = 1;
    ctx->level = 0;
    ctx->initialized = false;
    if (!res) return PLBA_OK;
    const Ctrl &h = *ctx->h_ctrl;
    res->linearizations = h.hlm_lin;
    res->solves = h.hlm_solves;
    res->accepted = h.hlm_acc;
    res->pad = 0;
    res->err = h.currentChi;
    res->lambda = h.lambda;
    res->dx_norm = std::sqrt(h.dx2);
    res->solve_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (res->kf_x && d.n_kf) {
        PLBA_CHECK(d2h(ctx, res->kf_x, d.xk[ctx->cur], sizeof(double) * (size_t)d.n_kf * 6));
        // KFs outside kf_list keep the caller's x (the device copy carries them through unchanged)
    }
    if (gba && res->ln_line3d && ctx->n_ln)
        PLBA_CHECK(d2h(ctx, res->ln_line3d, d.XL[ctx->cur], sizeof(double) * (size_t)ctx->n_ln * 6));
    return plba_download(ctx, res->kf_Tcw, res->pt_xyz, gba ? nullptr : res->ln_orth);
}

int plba_get_trace(plba_ctx *ctx, plba_iter_trace *out, int32_t cap, int32_t *n) {
    if (!ctx) return PLBA_E_INVALID;
    if (n) *n = (int32_t)ctx->trace.size();
    if (out)
        for (int i = 0; i < (int)ctx->trace.size() && i < cap; ++i) out[i] = ctx->trace[i];
    return PLBA_OK;
}

int plba_synchronize(plba_ctx *ctx) {
    if (!ctx) return PLBA_E_INVALID;
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    return PLBA_OK;
}

int plba_kernel_times(plba_ctx *ctx, const char **names, double *ms, int32_t *launches, int32_t cap, int32_t *n) {
    if (!ctx) return PLBA_E_INVALID;
    if (n) *n = K_COUNT;
    for (int k = 0; k < K_COUNT && k < cap; ++k) {
        if (names) names[k] = kKernelNames[k];
        if (ms) ms[k] = ctx->k_ms[k];
        if (launches) launches[k] = ctx->k_n[k];
    }
    return PLBA_OK;
}

int plba_structure_stats(plba_ctx *ctx, int64_t *out, int32_t cap) {
    if (!ctx || !out) return PLBA_E_INVALID;
    if (!ctx->uploaded) return PLBA_E_STATE;
    const int64_t v[22] = {ctx->d.nf, ctx->d.bw, ctx->d.nblk, (int64_t)ctx->n_triples, ctx->d.E, ctx->d.n_lm,
                           ctx->d.band_mode, ctx->d.nch, ctx->n_free_edges, ctx->d.Ep,
                           ctx->step_exec != nullptr, ctx->d.sharded, ctx->d.twisted, ctx->d.cl, ctx->d.bcr_N,
                           ctx->d.dense_mfma, ctx->bcr_fallbacks, ctx->d.spec_max, ctx->d.spec_policy,
                           ctx->h_ctrl ? ctx->h_ctrl->steps : 0, ctx->d.bcr_fused, ctx->dev_build};
    for (int i = 0; i < cap && i < 22; ++i) out[i] = v[i];
    return PLBA_OK;
}

// The factorisation an upload would choose for a window of nf free poses and envelope width bw
// (plan_factor under the current environment): no context, no device. flags: 1 no_bcr (the
// context fell back before), 2 sharded, 4 the window has Schur triples to assemble.
int plba_factor_plan(int32_t bw, int32_t nf, int32_t resident, int32_t flags, int32_t *out, int32_t cap) {
    if (!out || bw < 0 || nf < 0) return PLBA_E_INVALID;
    const FactorPlan p = plan_factor(bw, nf, resident, flags & 1, flags & 2, flags & 4, read_tuning());
    const int32_t v[9] = {p.mode, p.bcr_N, p.bcr_fused, p.tw_m, p.ring, p.slots, p.policy, p.fallback.mode, p.fallback.tw_m};
    for (int i = 0; i < cap && i < 9; ++i) out[i] = v[i];
    return PLBA_OK;
}

int plba_shard_plan(const plba_graph *g, int32_t nranks, int32_t *pt_owner, int32_t *ln_owner) {
    if (!g || nranks < 1 || (g->n_pt && !pt_owner) || (g->n_ln && !ln_owner)) return PLBA_E_INVALID;
    if ((g->n_ept && (!g->ept_lm || !g->ept_kf)) || (g->n_eln && (!g->eln_lm || !g->eln_kf)) ||
        (g->n_kf && !g->kf_id))
        return PLBA_E_INVALID;
    for (int e = 0; e < g->n_ept; ++e)
        if (g->ept_lm[e] < 0 || g->ept_lm[e] >= g->n_pt || g->ept_kf[e] < 0 || g->ept_kf[e] >= g->n_kf)
            return PLBA_E_INVALID;
    for (int e = 0; e < g->n_eln; ++e)
        if (g->eln_lm[e] < 0 || g->eln_lm[e] >= g->n_ln || g->eln_kf[e] < 0 || g->eln_kf[e] >= g->n_kf)
            return PLBA_E_INVALID;
    shard_plan(g, nranks, pt_owner, ln_owner);
    return PLBA_OK;
}

int plba_comm_unique_id(uint8_t id[128]) {
    if (!id) return PLBA_E_INVALID;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return PLBA_E_COMM;
    std::memcpy(id, &u, sizeof(u));
    return PLBA_OK;
}

int plba_comm_init_rccl(plba_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t id[128]) {
    if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return PLBA_E_INVALID;
    if (ctx->comm.kind != plba_ctx::Comm::NONE || ctx->uploaded) return PLBA_E_STATE;
    (void)hipSetDevice(ctx->opts.device);
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    const ncclResult_t r = ncclCommInitRank(&ctx->comm.nccl, nranks, u, rank);
    if (r != ncclSuccess) {
        ctx->set_error("ncclCommInitRank(%d ranks, rank %d): %s", nranks, rank, ncclGetErrorString(r));
        ctx->comm.nccl = nullptr;
        return PLBA_E_COMM;
    }
    ctx->comm.kind = plba_ctx::Comm::RCCL;
    ctx->comm.nranks = nranks;
    ctx->comm.rank = rank;
    return PLBA_OK;
}

int plba_comm_init_host(plba_ctx *ctx, int32_t nranks, int32_t rank, plba_host_allreduce_fn fn, void *user) {
    if (!ctx || !fn || nranks < 1 || rank < 0 || rank >= nranks) return PLBA_E_INVALID;
    if (ctx->comm.kind != plba_ctx::Comm::NONE || ctx->uploaded) return PLBA_E_STATE;
    ctx->comm.kind = plba_ctx::Comm::HOST;
    ctx->comm.nranks = nranks;
    ctx->comm.rank = rank;
    ctx->comm.fn = fn;
    ctx->comm.user = user;
    return PLBA_OK;
}

int plba_comm_info(plba_ctx *ctx, int32_t *out, int32_t cap) {
    if (!ctx || (cap > 0 && !out)) return PLBA_E_INVALID;
    (void)hipSetDevice(ctx->opts.device);
    const auto &c = ctx->comm;
    int32_t v[8] = {c.kind == plba_ctx::Comm::RCCL ? 1 : c.kind == plba_ctx::Comm::HOST ? 2 : 0,
                    c.kind == plba_ctx::Comm::NONE ? 1 : c.nranks, c.rank, ctx->opts.device, -1, -1, -1, -1};
    if (c.kind == plba_ctx::Comm::RCCL && c.nccl) {
        int n = 0, r = 0, dv = 0;
        if (ncclCommCount(c.nccl, &n) != ncclSuccess || ncclCommUserRank(c.nccl, &r) != ncclSuccess ||
            ncclCommCuDevice(c.nccl, &dv) != ncclSuccess) {
            ctx->set_error("RCCL communicator query failed");
            return PLBA_E_COMM;
        }
        v[1] = n;
        v[2] = r;
        v[3] = dv;
    }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        ctx->set_error("hipGetDevice failed");
        return PLBA_E_DEVICE;
    }
    v[4] = dev;
    int a = 0;
    if (hipDeviceGetAttribute(&a, hipDeviceAttributePciDomainID, dev) == hipSuccess) v[5] = a;
    if (hipDeviceGetAttribute(&a, hipDeviceAttributePciBusId, dev) == hipSuccess) v[6] = a;
    if (hipDeviceGetAttribute(&a, hipDeviceAttributePciDeviceId, dev) == hipSuccess) v[7] = a;
    (void)hipGetLastError();
    for (int i = 0; i < cap && i < 8; ++i) out[i] = v[i];
    return PLBA_OK;
}

// Extension: enable per-kernel HIP-event timing for subsequent plba_lba_plucker calls.
int plba_enable_kernel_timing(plba_ctx *ctx, int32_t on) {
    if (!ctx) return PLBA_E_INVALID;
    ctx->timing = on != 0;
    return PLBA_OK;
}

// ---------------------------------------------------------------- loop-closure pose graph
// defaults and the forwarder here; the driver is csrc/plba_pgo_driver.hpp
void plba_pgo_default_params(plba_pgo_params *p) {
    if (!p) return;
    p->user_lambda_init = 1e-10;  // src/mapHandler.cpp:5085
    p->max_iters = 100;           // SlamConfig::maxItersPGO(), src/slamConfig.cpp:79
    p->initial_guess = 1;         // optimizer.computeInitialGuess(), :5183
    p->max_trials = 10;           // g2o maxTrialsAfterFailure
    p->pad = 0;
}

int plba_pgo_optimize(plba_ctx *ctx, const plba_pgo_graph *g, const plba_pgo_params *pp, plba_pgo_result *res) {
    return ctx ? pgo_optimize(ctx, g, pp, res) : PLBA_E_INVALID;
}

// ---------------------------------------------------------------- loop-closure relative pose
// defaults here; the call itself is plba::lc_relative_pose (csrc/plba_assoc.hip)
void plba_lcpose_default_params(plba_lcpose_params *p) {
    if (!p) return;
    p->homog_th = 1e-7;       // src2/config.cpp:80
    p->lc_res = 1.0;          // src/slamConfig.cpp:73-77
    p->lc_unc = 0.01;
    p->lc_inl = 0.3;
    p->lc_trs = 1.5;
    p->lc_rot = 35.0;
    p->max_iters_first = 5;   // src2/config.cpp:82
    p->max_iters = 10;        // src2/config.cpp:83
    p->variant = PLBA_LCPOSE_ROBUST_GN;
    p->pad = 0;
}

int plba_lc_relative_pose(plba_ctx *ctx, const plba_lcpose_batch *b, const plba_lcpose_params *pp, plba_lcpose_out *out,
                          uint8_t *pt_inlier, uint8_t *ln_inlier) {
    return ctx ? lc_relative_pose(ctx, b, pp, out, pt_inlier, ln_inlier) : PLBA_E_INVALID;
}

// ---------------------------------------------------------------- frame-to-frame pose
// defaults here (src2/config.cpp:46-53, :80-86); the call itself is plba::track_pose (csrc/plba_assoc.hip)
void plba_track_default_params(plba_track_params *p) {
    if (!p) return;
    p->homog_th = 1e-7;
    p->min_error = 1e-7;
    p->min_error_change = 1e-7;
    p->inlier_k = 4.0;
    p->min_features = 10;
    p->max_iters = 5;
    p->max_iters_ref = 10;
    p->has_points = 1;
    p->has_lines = 1;
    p->use_motion_model = 0;
    p->line_model = PLBA_TRACK_PLUCKER;
    p->pad = 0;
}

int plba_track_pose(plba_ctx *ctx, const plba_track_batch *b, const plba_track_params *pp, plba_track_out *out,
                    uint8_t *pt_inlier, uint8_t *ln_inlier) {
    return ctx ? track_pose(ctx, b, pp, out, pt_inlier, ln_inlier) : PLBA_E_INVALID;
}

// frame-to-frame tracking: the matcher's defaults (src2/config.cpp:51, :60, :68) on top of the pose's; the
// call itself is plba::track_frames (csrc/plba_assoc.hip, csrc/plba_trackframes.hpp)
void plba_frames_default_params(plba_frames_params *p) {
    if (!p) return;
    plba_track_default_params(&p->track);
    p->nnr_pt = 0.9f;
    p->nnr_ln = 0.9f;
    p->best_lr = 1;
    p->desc_bytes = 32;
}

int plba_track_frames(plba_ctx *ctx, const plba_frames_batch *b, const plba_frames_params *pp, const plba_frames_out *out) {
    return ctx ? track_frames(ctx, b, pp, out) : PLBA_E_INVALID;
}

// descriptor matching and grid-guided matching (csrc/plba_assoc.hip)
int plba_desc_match(plba_ctx *ctx, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches) {
    return ctx ? desc_match(ctx, b, matches_12, n_matches) : PLBA_E_INVALID;
}

int plba_grid_match(plba_ctx *ctx, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches) {
    return ctx ? grid_match(ctx, b, matches_12, n_matches) : PLBA_E_INVALID;
}

// stereo association (csrc/plba_assoc.hip, csrc/plba_stereo.hpp)
void plba_stereo_default_params(plba_stereo_params *p) {
    if (!p) return;
    *p = plba_stereo_params{};
    p->cols = 64;                  // GRID_COLS / GRID_ROWS (include2/stereoFrame.h:51-52)
    p->rows = 48;
    p->matching_s_ws = 10;         // src2/config.cpp:91
    p->best_lr = 1;                // :51
    p->min_ratio_12_p = 0.9;       // :60
    p->line_sim_th = 0.75;         // :63
    p->max_dist_epip = 1.0;        // :58
    p->min_disp = 1.0;             // :59
    p->ls_min_disp_ratio = 0.7;    // :69
    p->line_horiz_th = 0.1;        // :67
    p->stereo_overlap_th = 0.75;   // :64
}

int plba_stereo_associate(plba_ctx *ctx, const plba_stereo_batch *b, const plba_stereo_params *p,
                          const plba_stereo_out *out) {
    return ctx ? stereo_associate(ctx, b, p, out) : PLBA_E_INVALID;
}

// keyframe-to-keyframe association (csrc/plba_assoc.hip, csrc/plba_kfassoc.hpp)
void plba_kfassoc_default_params(plba_kfassoc_params *p) {
    if (!p) return;
    *p = plba_kfassoc_params{};
    p->cols = 64;                  // GRID_COLS / GRID_ROWS (include2/stereoFrame.h:51-52)
    p->rows = 48;
    p->fast_matching = 1;          // config/config/config.yaml:5 (src/slamConfig.cpp:43 has false)
    p->ws = 3;                     // src2/config.cpp:92
    p->best_lr = 1;                // :51
    p->min_pt_matches = 10;        // src/slamConfig.cpp:51-52
    p->min_ls_matches = 6;
    p->min_ratio_12_p = 0.9;       // src2/config.cpp:60
    p->min_ratio_12_l = 0.9;       // :68
    p->line_sim_th = 0.75;         // :63
}

int plba_kf_associate(plba_ctx *ctx, const plba_kfassoc_batch *b, const plba_kfassoc_params *p,
                      const plba_kfassoc_out *out) {
    return ctx ? kf_associate(ctx, b, p, out) : PLBA_E_INVALID;
}

// map-to-keyframe association (csrc/plba_assoc.hip, csrc/plba_mapassoc.hpp)
void plba_mapassoc_default_params(plba_mapassoc_params *p) {
    if (!p) return;
    *p = plba_mapassoc_params{};
    p->cols = 64;                  // GRID_COLS / GRID_ROWS (include2/stereoFrame.h:51-52)
    p->rows = 48;
    p->fast_matching = 1;          // config/config/config.yaml:5 (src/slamConfig.cpp:43 has false)
    p->ws = 3;                     // src2/config.cpp:92
    p->best_lr = 1;                // :51
    p->min_pt_matches = 10;        // src/slamConfig.cpp:85-86
    p->min_ls_matches = 6;
    p->min_ratio_12_p = 0.9;       // src2/config.cpp:60
    p->min_ratio_12_l = 0.9;       // :68
    p->line_sim_th = 0.75;         // :63
    p->max_kf_epip_p = 1.0;        // src/slamConfig.cpp:51-52
    p->max_kf_epip_l = 1.0;
}

int plba_map_associate(plba_ctx *ctx, const plba_mapassoc_batch *b, const plba_mapassoc_params *p,
                       const plba_mapassoc_out *out) {
    return ctx ? map_associate(ctx, b, p, out) : PLBA_E_INVALID;
}

// median descriptor (csrc/plba_assoc.hip, csrc/plba_medoid.hpp)
int plba_desc_medoid(plba_ctx *ctx, const plba_medoid_batch *b, int32_t *medoid) {
    if (!ctx) return PLBA_E_INVALID;
    if (!b) {
        ctx->set_error("median descriptor: NULL batch");
        return PLBA_E_INVALID;
    }
    return desc_medoid(ctx, b->n, b->list_ptr, b->desc, b->desc_bytes, medoid);
}

// place recognition (csrc/plba_assoc.hip, csrc/plba_bow.hpp)
int plba_bow_set_vocab(plba_ctx *ctx, int32_t slot, const plba_bow_vocab *v) {
    return ctx ? bow_set_vocab(ctx, slot, v) : PLBA_E_INVALID;
}

int plba_bow_insert(plba_ctx *ctx, int32_t slot, int32_t kf_id, const uint8_t *desc, int32_t n_desc, double *scores,
                    int32_t *ids, int32_t cap, int32_t *n) {
    return ctx ? bow_insert(ctx, slot, kf_id, desc, n_desc, scores, ids, cap, n) : PLBA_E_INVALID;
}

int plba_bow_remove(plba_ctx *ctx, int32_t slot, int32_t kf_id) {
    return ctx ? bow_remove(ctx, slot, kf_id) : PLBA_E_INVALID;
}

int plba_bow_get(plba_ctx *ctx, int32_t slot, int32_t kf_id, int32_t *word_ids, double *values, int32_t cap,
                 int32_t *n) {
    return ctx ? bow_get(ctx, slot, kf_id, word_ids, values, cap, n) : PLBA_E_INVALID;
}

}  // extern "C"
