// plba_pgo_driver.hpp — host driver of the loop-closure pose graph (plba_pgo_optimize), phase by
// phase; pgo_optimize, at the end, is the sequence.
// MapHandler::loopClosureOptimization{EssGraph,CovGraph}G2O (src/mapHandler.cpp:5070-5531):
// g2o SparseOptimizer::initializeOptimization / computeInitialGuess / optimize over VertexSE3 +
// EdgeSE3 with OptimizationAlgorithmLevenberg (setUserLambdaInit) — device kernels in
// csrc/plba_pgo.hpp, Levenberg decisions here.
// Included by plba.hip only (the pose graph shares k_dense_panel / k_dense_update with the step
// graph, so it stays in the solver's translation unit), after its rcm_from_adj / permute_hidx.
// Host arithmetic that g2o does in plain doubles (HIso products, the Levenberg bookkeeping) is
// compiled under fp contract(off), function by function.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <map>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "plba_kernels.hpp"
#include "plba_plan.hpp"
#include "plba_scratch.hpp"

namespace {

struct HIso {
    double R[9], t[3];
};
HIso hiso_load(const double *T) {
    HIso a;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a.R[3 * r + c] = T[4 * r + c];
        a.t[r] = T[4 * r + 3];
    }
    return a;
}
void hiso_store(const HIso &a, double *T) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = a.R[3 * r + c];
        T[4 * r + 3] = a.t[r];
    }
}
HIso hiso_mul(const HIso &a, const HIso &b) {
#pragma clang fp contract(off)
    HIso o;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s = s + a.R[3 * r + k] * b.R[3 * k + c];
            o.R[3 * r + c] = s;
        }
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s = s + a.R[3 * r + k] * b.t[k];
        o.t[r] = s + a.t[r];
    }
    return o;
}
HIso hiso_inv(const HIso &a) {
#pragma clang fp contract(off)
    HIso o;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o.R[3 * r + c] = a.R[3 * c + r];
    for (int r = 0; r < 3; ++r) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s = s + o.R[3 * r + k] * a.t[k];
        o.t[r] = -s;
    }
    return o;
}

// everything the host derives from one pose graph, filled phase by phase
struct PgoProblem {
    const plba_pgo_graph *g = nullptr;
    plba_pgo_params prm;
    Tuning tuning;  // (PLBA_NO_RCM, PLBA_SOLVE_LDS_N: sampled per call)
    int nv = 0, ne = 0;
    std::vector<HIso> X, Z, Zinv;  // estimates, measurements and their inverses
    std::vector<int32_t> act;      // active edges in creation order
    std::vector<uint8_t> is_act;
    std::vector<int32_t> hidx;     // vertex -> Hessian block index, -1: fixed or inactive
    int nfree = 0;
    std::vector<int32_t> first_h;  // first block column of each block row of H's envelope
    std::vector<int32_t> blk_r, blk_c, blk_off, blk_con;  // lower-triangle blocks, CSR of contributions
    int n = 0, nblk = 0, ntiles = 0;
    TileEnvelope env;
};

int pgo_validate(const plba_pgo_graph *g, const plba_pgo_params *pp, const plba_pgo_result *res, PgoProblem &pb,
                 std::string &why) {
    if (!g || !res || g->n_v < 0 || g->n_e < 0) return PLBA_E_INVALID;
    if ((g->n_v && (!g->v_id || !g->v_T || !g->v_fixed)) || (g->n_e && (!g->e_v || !g->e_Z))) return PLBA_E_INVALID;
    if (pp) pb.prm = *pp;
    else plba_pgo_default_params(&pb.prm);
    if (pb.prm.max_iters < 0 || pb.prm.max_trials < 1) {
        why = "max_iters must be >= 0 and max_trials >= 1";
        return PLBA_E_INVALID;
    }
    pb.g = g;
    const int nv = pb.nv = g->n_v, ne = pb.ne = g->n_e;
    for (int e = 0; e < 2 * ne; ++e)
        if (g->e_v[e] < 0 || g->e_v[e] >= nv) {
            why = "pose-graph edge " + std::to_string(e / 2) + " references vertex " + std::to_string(g->e_v[e]) +
                  " (n_v " + std::to_string(nv) + ")";
            return PLBA_E_INVALID;
        }
    std::vector<int32_t> ids(g->v_id, g->v_id + nv);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) {
        why = "duplicate pose-graph vertex id";
        return PLBA_E_INVALID;
    }
    return PLBA_OK;
}

// SparseOptimizer::initializeOptimization(): active edges (not all vertices fixed) in creation
// order; Hessian index of the active free vertices in id order
void pgo_active_set(PgoProblem &pb) {
    const plba_pgo_graph *g = pb.g;
    const int nv = pb.nv, ne = pb.ne;
    pb.X.resize(nv);
    pb.Z.resize(ne);
    pb.Zinv.resize(ne);
    for (int v = 0; v < nv; ++v) pb.X[v] = hiso_load(g->v_T + 12 * (size_t)v);
    for (int e = 0; e < ne; ++e) {
        pb.Z[e] = hiso_load(g->e_Z + 12 * (size_t)e);
        pb.Zinv[e] = hiso_inv(pb.Z[e]);  // EdgeSE3::setMeasurement keeps the inverse
    }
    pb.is_act.assign(ne, 0);
    std::vector<int> nact_v(nv, 0);
    for (int e = 0; e < ne; ++e) {
        const int a = g->e_v[2 * e], b = g->e_v[2 * e + 1];
        if (g->v_fixed[a] && g->v_fixed[b]) continue;
        pb.act.push_back(e);
        pb.is_act[e] = 1;
        ++nact_v[a];
        ++nact_v[b];
    }
    std::vector<int> order(nv);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return g->v_id[a] < g->v_id[b]; });
    pb.hidx.assign(nv, -1);
    for (int v : order)
        if (nact_v[v] > 0 && !g->v_fixed[v]) pb.hidx[v] = pb.nfree++;
}

// computeInitialGuess(): EstimatePropagator from the fixed vertices of the active edges
// (std::set<Vertex*>: creation order), unit edge cost, multimap frontier (smallest distance first,
// FIFO among equals), EdgeSE3::initialEstimate on each first reach
void pgo_initial_guess(PgoProblem &pb) {
    const plba_pgo_graph *g = pb.g;
    const int nv = pb.nv, ne = pb.ne;
    std::vector<HIso> &X = pb.X;
    std::vector<std::vector<int>> vedges(nv);
    for (int e = 0; e < ne; ++e) {
        vedges[g->e_v[2 * e]].push_back(e);
        vedges[g->e_v[2 * e + 1]].push_back(e);
    }
    std::vector<int> roots;
    std::vector<uint8_t> isroot(nv, 0);
    for (int e : pb.act)
        for (int sd = 0; sd < 2; ++sd) {
            const int v = g->e_v[2 * e + sd];
            if (g->v_fixed[v] && !isroot[v]) { isroot[v] = 1; roots.push_back(v); }
        }
    std::sort(roots.begin(), roots.end());
    const double inf = std::numeric_limits<double>::max();
    std::vector<double> dist(nv, inf);
    std::vector<int> level(nv, 0), pedge(nv, -1), parent(nv, -1);
    std::multimap<double, int> frontier;
    std::vector<std::multimap<double, int>::iterator> qit(nv);
    std::vector<uint8_t> inq(nv, 0);
    auto push = [&](int v) {
        if (inq[v]) frontier.erase(qit[v]);
        qit[v] = frontier.insert(frontier.upper_bound(dist[v]), {dist[v], v});
        inq[v] = 1;
    };
    for (int r : roots) { dist[r] = 0.0; push(r); }
    while (!frontier.empty()) {
        const auto it = frontier.begin();
        const int u = it->second;
        frontier.erase(it);
        inq[u] = 0;
        if (level[u] > 0 && !g->v_fixed[u]) {
            const int e = pedge[u];
            if (parent[u] == g->e_v[2 * e]) X[u] = hiso_mul(X[g->e_v[2 * e]], pb.Z[e]);
            else X[u] = hiso_mul(X[g->e_v[2 * e + 1]], hiso_inv(pb.Z[e]));
        }
        for (int e : vedges[u]) {
            if (!pb.is_act[e]) continue;
            int maxf = -1;
            for (int sd = 0; sd < 2; ++sd) {
                const int z = g->e_v[2 * e + sd];
                if (dist[z] != inf) maxf = std::max(maxf, level[z]);
            }
            for (int sd = 0; sd < 2; ++sd) {
                const int z = g->e_v[2 * e + sd];
                if (z == u) continue;
                const double zd = dist[u] + 1.0;
                if (zd < dist[z]) {
                    dist[z] = zd;
                    parent[z] = u;
                    pedge[z] = e;
                    level[z] = maxf + 1;
                    push(z);
                }
            }
        }
    }
}

// Hessian order: Cholmod orders H by AMD before its supernodal factorisation; here the free
// vertices are reordered by reverse Cuthill–McKee when that narrows the band (loop edges couple
// vertices far apart in id order), and the dense factorisation runs over the envelope only
// (tile_first / tile_last). Any symmetric order gives the same exact solve.
void pgo_order(PgoProblem &pb) {
    const plba_pgo_graph *g = pb.g;
    const int nfree = pb.nfree;
    auto envelope_of = [&](const std::vector<int32_t> &hx, std::vector<int32_t> &fh) {
        for (int h = 0; h < nfree; ++h) fh[h] = h;
        for (int e : pb.act) {
            const int a = hx[g->e_v[2 * e]], b = hx[g->e_v[2 * e + 1]];
            if (a < 0 || b < 0) continue;
            fh[std::max(a, b)] = std::min(fh[std::max(a, b)], std::min(a, b));
        }
        int w = 0;
        for (int h = 0; h < nfree; ++h) w = std::max(w, h - fh[h]);
        return w;
    };
    pb.first_h.resize(nfree);
    const int bwp = envelope_of(pb.hidx, pb.first_h);
    if (bwp > 1 && nfree > 2 && !pb.tuning.no_rcm) {
        std::vector<std::vector<int32_t>> adj(nfree);
        for (int e : pb.act) {
            const int a = pb.hidx[g->e_v[2 * e]], b = pb.hidx[g->e_v[2 * e + 1]];
            if (a < 0 || b < 0 || a == b) continue;
            adj[a].push_back(b);
            adj[b].push_back(a);
        }
        const std::vector<int32_t> h2 = permute_hidx(pb.hidx, rcm_from_adj(adj));
        std::vector<int32_t> fh2(nfree);
        if (envelope_of(h2, fh2) < bwp) {
            pb.hidx = h2;
            pb.first_h = fh2;
        }
    }
}

// blocks of H (lower triangle) and their contributions in edge order; the map's (col, row) order
// is the order of blk_* and so the summation order on the device
void pgo_block_pattern(PgoProblem &pb) {
    const plba_pgo_graph *g = pb.g;
    std::map<std::pair<int, int>, std::vector<int32_t>> blocks;  // (col, row) -> contributions
    for (int h = 0; h < pb.nfree; ++h) blocks[{h, h}];
    for (int e : pb.act) {
        const int hi = pb.hidx[g->e_v[2 * e]], hj = pb.hidx[g->e_v[2 * e + 1]];
        if (hi >= 0) blocks[{hi, hi}].push_back(e << 2 | 0);
        if (hj >= 0) blocks[{hj, hj}].push_back(e << 2 | 1);
        if (hi >= 0 && hj >= 0 && hi != hj) {
            if (hi > hj) blocks[{hj, hi}].push_back(e << 2 | 2);  // row block = vertex i
            else blocks[{hi, hj}].push_back(e << 2 | 3);          // row block = vertex j
        }
    }
    pb.blk_off.assign(1, 0);
    for (auto &kv : blocks) {
        pb.blk_c.push_back(kv.first.first);
        pb.blk_r.push_back(kv.first.second);
        for (int32_t c : kv.second) pb.blk_con.push_back(c);
        pb.blk_off.push_back((int32_t)pb.blk_con.size());
    }
    pb.n = 6 * pb.nfree;
    pb.nblk = (int)pb.blk_r.size();
    pb.ntiles = (pb.n + kTile - 1) / kTile;
    pb.env = tile_envelope(pb.first_h, pb.n, kTile);
}

// the device block (grow-only), its uploads and the kernels' views of it
int pgo_stage(CtxBase *ctx, const PgoProblem &pb, PgoDev &P_out, Dev &dd_out) {
    const plba_pgo_graph *g = pb.g;
    const size_t nv = pb.nv, ne = pb.ne, n = pb.n, nblk = pb.nblk, nt = pb.ntiles;
    PgoDev P{};  // the caller's are written once everything is issued
    Dev dd{};
    Staged B;  // device only: the uploads below are copies from pageable memory, array by array
    B.dev(P.e_v, 2 * ne); B.dev(P.act, pb.act.size()); B.dev(P.hidx, nv);
    B.dev(P.blk_r, nblk); B.dev(P.blk_c, nblk); B.dev(P.blk_off, nblk + 1); B.dev(P.blk_con, pb.blk_con.size());
    B.dev(dd.tile_first, nt); B.dev(dd.tile_last, nt);
    B.dev(P.Zinv, 12 * ne); B.dev(P.info, 36 * ne); B.dev(P.T[0], 12 * nv); B.dev(P.T[1], 12 * nv);
    B.dev(P.eH, 144 * ne); B.dev(P.eg, 12 * ne); B.dev(P.echi, ne);
    B.dev(P.Hd, n * n); B.dev(dd.Ad, n * n); B.dev(P.b, n); B.dev(P.x, n);
    B.dev(dd.Wbuf, std::max(n, (size_t)1) * (kTile + 1)); B.dev(P.out, 4); B.dev(dd.ctrl, 1);
    if (const int rc = ctx->pgo.reserve(*ctx, B.total(), sizeof(double) * 4, "pose graph")) return rc;
    B.stage(nullptr, ctx->pgo.dev);
    hipStream_t s = ctx->stream;
    std::vector<double> Tv(12 * nv), Zi(12 * ne), Om(36 * ne);
    for (size_t v = 0; v < nv; ++v) hiso_store(pb.X[v], &Tv[12 * v]);
    for (size_t e = 0; e < ne; ++e) {
        hiso_store(pb.Zinv[e], &Zi[12 * e]);
        for (int k = 0; k < 36; ++k) Om[36 * e + k] = g->e_info ? g->e_info[36 * e + k] : (k % 7 == 0 ? 1.0 : 0.0);
    }
    auto up = [&](const void *dst, const void *src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(const_cast<void *>(dst), src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    auto upv = [&](const void *dst, const auto &v) { return up(dst, v.data(), sizeof(v[0]) * v.size()); };
    PLBA_CHECK(up(P.e_v, g->e_v, sizeof(int32_t) * 2 * ne));
    PLBA_CHECK(upv(P.act, pb.act));
    PLBA_CHECK(upv(P.hidx, pb.hidx));
    PLBA_CHECK(upv(P.blk_r, pb.blk_r));
    PLBA_CHECK(upv(P.blk_c, pb.blk_c));
    PLBA_CHECK(upv(P.blk_off, pb.blk_off));
    PLBA_CHECK(upv(P.blk_con, pb.blk_con));
    PLBA_CHECK(upv(dd.tile_first, pb.env.tile_first));
    PLBA_CHECK(upv(dd.tile_last, pb.env.tile_last));
    PLBA_CHECK(upv(P.Zinv, Zi));
    PLBA_CHECK(upv(P.info, Om));
    PLBA_CHECK(upv(P.T[0], Tv));
    PLBA_CHECK(hipMemsetAsync(P.x, 0, sizeof(double) * std::max(n, (size_t)1), s));  // g2o's _x starts at zero
    PLBA_CHECK(hipMemsetAsync(dd.ctrl, 0, sizeof(Ctrl), s));
    P.nv = pb.nv; P.ne = pb.ne; P.nact = (int)pb.act.size(); P.nfree = pb.nfree; P.n = pb.n; P.nblk = pb.nblk;
    dd.n = pb.n; dd.ntiles = pb.ntiles; dd.bs = P.b; dd.xp = P.x;
    dd.solve_lds_n = pb.tuning.solve_lds_n;
    P_out = P;
    dd_out = dd;
    return PLBA_OK;
}

// the four doubles of P.out, on the host once the stream has drained
int pgo_fetch(CtxBase *ctx, const PgoDev &P) {
    PLBA_CHECK(hipMemcpyAsync(ctx->pgo.host, P.out, sizeof(double) * 4, hipMemcpyDeviceToHost, ctx->stream));
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    return PLBA_OK;
}

// g2o's default τ: the reference makes a fresh OptimizationAlgorithmLevenberg for every pose graph,
// so plba_opts::tau (the window solver's) does not reach it
constexpr double kPgoTau = 1e-5;

// computeActiveErrors() after the initial guess, then OptimizationAlgorithmLevenberg::solve per
// iteration: three read-backs per trial decide the next launch
int pgo_levenberg(CtxBase *ctx, const PgoProblem &pb, PgoDev &P, Dev &dd, plba_pgo_result *res) {
#pragma clang fp contract(off)
    const plba_pgo_params &prm = pb.prm;
    const int nv = pb.nv, nfree = pb.nfree, n = pb.n, nblk = pb.nblk, ntiles = pb.ntiles, nact = P.nact;
    const std::vector<int32_t> &tl = pb.env.tile_last;
    const Ctrl *ctrl_d = dd.ctrl;
    double *Ad = dd.Ad;
    const double *hout = (const double *)ctx->pgo.host;
    hipStream_t s = ctx->stream;
    const int eb = std::max((nact + kPgoNT - 1) / kPgoNT, 1);
    int cur = 0;
    hipLaunchKernelGGL(k_pgo_linearize<false>, dim3(eb), dim3(kPgoNT), 0, s, P, cur); PLBA_LAUNCHED(ctx, "k_pgo_linearize");
    hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(64), 0, s, P, ctrl_d, 0, 0.0); PLBA_LAUNCHED(ctx, "k_pgo_sum");
    PLBA_CHECK(hipGetLastError());
    if (int rc = pgo_fetch(ctx, P)) return rc;
    res->chi2_initial = hout[0];
    res->n_free = nfree;
    res->iterations = res->trials = res->solve_fails = 0;
    res->n_trace = 0;
    double lambda = 0.0, ni = 2.0, currentChi = hout[0];
    for (int it = 0; it < prm.max_iters && nfree > 0; ++it) {
        // OptimizationAlgorithmLevenberg::solve: computeActiveErrors, buildSystem
        hipLaunchKernelGGL(k_pgo_linearize<true>, dim3(eb), dim3(kPgoNT), 0, s, P, cur); PLBA_LAUNCHED(ctx, "k_pgo_linearize");
        hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(64), 0, s, P, ctrl_d, 0, 0.0); PLBA_LAUNCHED(ctx, "k_pgo_sum");
        PLBA_CHECK(hipMemsetAsync(P.Hd, 0, sizeof(double) * (size_t)n * n, s));
        hipLaunchKernelGGL(k_pgo_assemble, dim3((nblk * 42 + kPgoNT - 1) / kPgoNT), dim3(kPgoNT), 0, s, P); PLBA_LAUNCHED(ctx, "k_pgo_assemble");
        if (it == 0 && prm.user_lambda_init <= 0.0) hipLaunchKernelGGL(k_pgo_maxdiag, dim3(1), dim3(64), 0, s, P); PLBA_LAUNCHED(ctx, "k_pgo_maxdiag");
        PLBA_CHECK(hipGetLastError());
        if (int rc = pgo_fetch(ctx, P)) return rc;
        currentChi = hout[0];
        const double chiStart = currentChi;
        if (it == 0) {  // computeLambdaInit: the pose graph's own OptimizationAlgorithmLevenberg, τ = 1e-5
            lambda = prm.user_lambda_init > 0.0 ? prm.user_lambda_init : kPgoTau * hout[2];
            ni = 2.0;
        }
        const double lambdaStart = lambda;
        double rho = 0.0;
        int qmax = 0;
        do {
            // setLambda + solve (dense LDLᵀ, Cholmod's positive-definite test) + update
            hipLaunchKernelGGL(k_pgo_damp, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, s, P, Ad, lambda); PLBA_LAUNCHED(ctx, "k_pgo_damp");
            for (int K = 0; K < ntiles; ++K) {  // the envelope's row tiles K..tl[K] only
                const int m = tl[K] - K;
                hipLaunchKernelGGL(k_dense_panel, dim3((m + 2) / 2), dim3(kDensePanelNT), 0, s, dd, K); PLBA_LAUNCHED(ctx, "k_dense_panel");
                if (m > 0) hipLaunchKernelGGL(k_dense_update, dim3(m * (m + 1) / 2), dim3(64), 0, s, dd, K); PLBA_LAUNCHED(ctx, "k_dense_update");
            }
            hipLaunchKernelGGL(k_pgo_check, dim3(1), dim3(256), 0, s, dd); PLBA_LAUNCHED(ctx, "k_pgo_check");
            hipLaunchKernelGGL(k_pgo_solve, dim3(1), dim3(kFacThreads),
                               n <= dd.solve_lds_n ? sizeof(double) * (size_t)n : 0, s, dd); PLBA_LAUNCHED(ctx, "k_pgo_solve");
            hipLaunchKernelGGL(k_pgo_update, dim3((nv + kPgoNT - 1) / kPgoNT), dim3(kPgoNT), 0, s, P, cur); PLBA_LAUNCHED(ctx, "k_pgo_update");
            // restoreDiagonal (Hd is untouched), computeActiveErrors at the trial state
            hipLaunchKernelGGL(k_pgo_linearize<false>, dim3(eb), dim3(kPgoNT), 0, s, P, cur ^ 1); PLBA_LAUNCHED(ctx, "k_pgo_linearize");
            hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(64), 0, s, P, ctrl_d, 1, lambda); PLBA_LAUNCHED(ctx, "k_pgo_sum");
            PLBA_CHECK(hipGetLastError());
            if (int rc = pgo_fetch(ctx, P)) return rc;
            const bool ok = hout[3] != 0.0;
            double tempChi = hout[1];
            if (!ok) {
                tempChi = std::numeric_limits<double>::max();
                ++res->solve_fails;
            }
            const double scale = hout[2] + 1e-3;
            rho = (currentChi - tempChi) / scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                lambda *= std::max(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                cur ^= 1;  // discardTop: the trial state becomes current
            } else {
                lambda *= ni;
                ni *= 2;
                if (!std::isfinite(lambda)) break;  // (pop: the current state is untouched)
            }
            ++qmax;
            ++res->trials;
        } while (rho < 0 && qmax < prm.max_trials);
        const int result = (qmax == prm.max_trials || rho == 0 || !std::isfinite(lambda)) ? 1 : 0;
        if (res->trace && res->n_trace < res->trace_cap)
            res->trace[res->n_trace++] = plba_iter_trace{0, it, qmax, result, chiStart, currentChi, lambdaStart, lambda};
        ++res->iterations;
        if (result != 0) break;
    }
    res->chi2_final = currentChi;
    res->lambda_final = lambda;
    if (res->v_T) {
        PLBA_CHECK(hipMemcpyAsync(res->v_T, P.T[cur], sizeof(double) * 12 * (size_t)nv, hipMemcpyDeviceToHost, s));
        PLBA_CHECK(hipStreamSynchronize(s));
    }
    return PLBA_OK;
}

int pgo_optimize(CtxBase *ctx, const plba_pgo_graph *g, const plba_pgo_params *pp, plba_pgo_result *res) {
    PgoProblem pb;
    std::string why;
    if (const int rc = pgo_validate(g, pp, res, pb, why)) {
        if (!why.empty()) ctx->set_error("%s", why.c_str());
        return rc;
    }
    (void)hipSetDevice(ctx->opts.device);
    pb.tuning = read_tuning();
    const auto t0 = std::chrono::steady_clock::now();
    pgo_active_set(pb);
    if (pb.prm.initial_guess) pgo_initial_guess(pb);
    pgo_order(pb);
    pgo_block_pattern(pb);
    PgoDev P;
    Dev dd;
    if (const int rc = pgo_stage(ctx, pb, P, dd)) return rc;
    if (const int rc = pgo_levenberg(ctx, pb, P, dd, res)) return rc;
    res->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PLBA_OK;
}

}  // namespace
