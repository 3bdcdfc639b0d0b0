// plba_assoc.hip — host side of the data-association entry points: the loop-closure relative pose
// and the two descriptor matchers. They share nothing with the solver (no Dev, no step graph, no
// window arena), so they are a translation unit of their own: an edit to a matcher does not
// rebuild the factorisation kernels. Each call is one upload, its kernels and one read-back through
// a ScratchBlock laid out by a Layout; the extern "C" symbols are forwarders in plba.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "plba_lcpose.hpp"
#include "plba_match.hpp"
#include "plba_gridmatch.hpp"
#include "plba_scratch.hpp"

namespace plba {

namespace {

// "<op>: desc_bytes N is no multiple of 4 in [4, 64]"
int check_desc_bytes(CtxBase *ctx, const char *op, int desc_bytes) {
    if (desc_bytes < 4 || desc_bytes > 64 || desc_bytes % 4) {
        ctx->set_error("%s: desc_bytes %d is no multiple of 4 in [4, 64]", op, desc_bytes);
        return PLBA_E_INVALID;
    }
    return PLBA_OK;
}

// off[0..n] starts at >= 0 and never decreases; *max_span (if given) is raised to the widest span.
// "<op>: negative <kind> offset" / "<op>: <kind> offsets decrease at <unit> K"
int check_offsets(CtxBase *ctx, const char *op, const char *kind, const char *unit, const int32_t *off, int n,
                  int *max_span = nullptr) {
    if (off[0] < 0) {
        ctx->set_error("%s: negative %s offset", op, kind);
        return PLBA_E_INVALID;
    }
    for (int k = 0; k < n; ++k) {
        if (off[k + 1] < off[k]) {
            ctx->set_error("%s: %s offsets decrease at %s %d", op, kind, unit, k);
            return PLBA_E_INVALID;
        }
        if (max_span) *max_span = std::max(*max_span, off[k + 1] - off[k]);
    }
    return PLBA_OK;
}

// copies count T into the host image at `off` (nothing for an absent or empty array)
template <typename T>
void put(char *h, size_t off, const T *src, size_t count) {
    if (src && count) memcpy(h + off, src, sizeof(T) * count);
}

}  // namespace

// ---------------------------------------------------------------- loop-closure relative pose
// MapHandler::computeRelativePoseRobustGN / computeRelativePoseGN (src/mapHandler.cpp:4677-5068,
// :4413-4675) for a batch of candidate pairs: one upload, one launch of k_lcpose
// (csrc/plba_lcpose.hpp, one workgroup per candidate), one read-back.
int lc_relative_pose(CtxBase &cb, const plba_lcpose_batch *b, const plba_lcpose_params *pp, plba_lcpose_out *out,
                     uint8_t *pt_inlier, uint8_t *ln_inlier) {
    CtxBase *const ctx = &cb;
    const char *const op = "relative pose";
    if (!b || b->n < 0) {
        ctx->set_error("relative pose: NULL batch or n < 0");
        return PLBA_E_INVALID;
    }
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    plba_lcpose_params prm;
    if (pp) prm = *pp;
    else plba_lcpose_default_params(&prm);
    if (!out || !b->pt_off || !b->ln_off) {
        ctx->set_error("relative pose: NULL out / pt_off / ln_off");
        return PLBA_E_INVALID;
    }
    if ((prm.variant != PLBA_LCPOSE_ROBUST_GN && prm.variant != PLBA_LCPOSE_GN) || prm.max_iters_first < 0 ||
        prm.max_iters < 0) {
        ctx->set_error("relative pose: unknown variant %d or a negative iteration cap", prm.variant);
        return PLBA_E_INVALID;
    }
    for (const int32_t *off : {b->pt_off, b->ln_off})
        if (const int rc = check_offsets(ctx, op, "feature", "candidate", off, n)) return rc;
    const size_t np = (size_t)b->pt_off[n], nl = (size_t)b->ln_off[n];
    if ((np && (!b->pt_P || !b->pt_obs)) || (nl && (!b->ln_sP || !b->ln_eP || !b->ln_le))) {
        ctx->set_error("relative pose: NULL feature array");
        return PLBA_E_INVALID;
    }
    (void)hipSetDevice(ctx->opts.device);
    // one block, the same layout on the device and in pinned host memory
    Layout L;
    const size_t o_ptoff = L.add<int32_t>(n + 1), o_lnoff = L.add<int32_t>(n + 1), o_P = L.add<double>(3 * np),
                 o_obs = L.add<double>(2 * np), o_sP = L.add<double>(3 * nl), o_eP = L.add<double>(3 * nl),
                 o_le = L.add<double>(3 * nl);
    const size_t inputs_end = L.mark();  // host -> device
    const size_t o_out = L.add<plba_lcpose_out>(n), o_pin = L.add(np), o_lin = L.add(nl);
    const size_t outputs_end = L.mark();  // device -> host
    if (const int rc = ctx->lc.reserve(cb, outputs_end, outputs_end, op)) return rc;
    char *h = ctx->lc.host, *dv = ctx->lc.dev;
    put(h, o_ptoff, b->pt_off, n + 1);
    put(h, o_lnoff, b->ln_off, n + 1);
    put(h, o_P, b->pt_P, 3 * np);
    put(h, o_obs, b->pt_obs, 2 * np);
    put(h, o_sP, b->ln_sP, 3 * nl);
    put(h, o_eP, b->ln_eP, 3 * nl);
    put(h, o_le, b->ln_le, 3 * nl);
    hipStream_t s = ctx->stream;
    PLBA_CHECK(hipMemcpyAsync(dv, h, inputs_end, hipMemcpyHostToDevice, s));
    LcDev D{};
    D.pt_off = at<const int32_t>(dv, o_ptoff);
    D.ln_off = at<const int32_t>(dv, o_lnoff);
    D.pt_P = at<const double>(dv, o_P);
    D.pt_obs = at<const double>(dv, o_obs);
    D.ln_sP = at<const double>(dv, o_sP);
    D.ln_eP = at<const double>(dv, o_eP);
    D.ln_le = at<const double>(dv, o_le);
    D.out = at<plba_lcpose_out>(dv, o_out);
    D.pt_in = at<uint8_t>(dv, o_pin);
    D.ln_in = at<uint8_t>(dv, o_lin);
    D.cam = Cam{b->fx, b->fy, b->cx, b->cy};
    D.prm = prm;
    hipLaunchKernelGGL(k_lcpose, dim3(n), dim3(kLcNT), 0, s, D); PLBA_LAUNCHED(ctx, "k_lcpose");
    PLBA_CHECK(hipMemcpyAsync(h + inputs_end, dv + inputs_end, outputs_end - inputs_end, hipMemcpyDeviceToHost, s));
    PLBA_CHECK(hipStreamSynchronize(s));
    memcpy(out, h + o_out, sizeof(plba_lcpose_out) * (size_t)n);
    if (pt_inlier && np) memcpy(pt_inlier, h + o_pin, np);
    if (ln_inlier && nl) memcpy(ln_inlier, h + o_lin, nl);
    return PLBA_OK;
}

// ---------------------------------------------------------------- descriptor matching
// StVO::match / matchNNR (src2/matching.cpp:41-91) for a batch of descriptor-set pairs: one upload,
// k_desc_nn (both directions of every pair) and k_desc_cross (csrc/plba_match.hpp), one read-back.
int desc_match(CtxBase &cb, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches) {
    CtxBase *const ctx = &cb;
    const char *const op = "descriptor matching";
    if (!b || b->n < 0) {
        ctx->set_error("descriptor matching: NULL batch or n < 0");
        return PLBA_E_INVALID;
    }
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    if (const int rc = check_desc_bytes(ctx, op, b->desc_bytes)) return rc;
    if (!b->off1 || !b->off2 || !b->nnr || !n_matches) {
        ctx->set_error("descriptor matching: NULL off1 / off2 / nnr / n_matches");
        return PLBA_E_INVALID;
    }
    int max_rows = 0;
    for (const int32_t *off : {b->off1, b->off2})
        if (const int rc = check_offsets(ctx, op, "row", "pair", off, n, &max_rows)) return rc;
    if ((max_rows + kDmNT - 1) / kDmNT > 65535) {  // the row tiles are the grid's second dimension
        ctx->set_error("descriptor matching: a set of %d rows is more than %d", max_rows, 65535 * kDmNT);
        return PLBA_E_INVALID;
    }
    const size_t n1 = (size_t)b->off1[n], n2 = (size_t)b->off2[n], db = (size_t)b->desc_bytes;
    if ((n1 && (!b->desc1 || !matches_12)) || (n2 && !b->desc2)) {
        ctx->set_error("descriptor matching: NULL desc1 / desc2 / matches_12");
        return PLBA_E_INVALID;
    }
    (void)hipSetDevice(ctx->opts.device);
    // one block; the pinned host image holds its inputs and outputs
    Layout L;
    const size_t o_off1 = L.add<int32_t>(n + 1), o_off2 = L.add<int32_t>(n + 1), o_nnr = L.add<float>(n),
                 o_d1 = L.add(db * n1), o_d2 = L.add(db * n2);
    const size_t inputs_end = L.mark();  // host -> device
    const size_t o_m12 = L.add<int32_t>(n1), o_cnt = L.add<int32_t>(n);
    const size_t outputs_end = L.mark();  // device -> host
    const size_t o_nn12 = L.add<int32_t>(n1), o_nn21 = L.add<int32_t>(n2);  // device only
    if (const int rc = ctx->match.reserve(cb, L.total, outputs_end, op)) return rc;
    char *h = ctx->match.host, *dv = ctx->match.dev;
    put(h, o_off1, b->off1, n + 1);
    put(h, o_off2, b->off2, n + 1);
    put(h, o_nnr, b->nnr, n);
    put(h, o_d1, b->desc1, db * n1);
    put(h, o_d2, b->desc2, db * n2);
    hipStream_t s = ctx->stream;
    PLBA_CHECK(hipMemcpyAsync(dv, h, inputs_end, hipMemcpyHostToDevice, s));
    DmDev D{};
    D.off1 = at<const int32_t>(dv, o_off1);
    D.off2 = at<const int32_t>(dv, o_off2);
    D.nnr = at<const float>(dv, o_nnr);
    D.desc1 = at<const uint32_t>(dv, o_d1);
    D.desc2 = at<const uint32_t>(dv, o_d2);
    D.m12 = at<int32_t>(dv, o_m12);
    D.count = at<int32_t>(dv, o_cnt);
    D.nn12 = at<int32_t>(dv, o_nn12);
    D.nn21 = at<int32_t>(dv, o_nn21);
    D.n = n;
    D.dwords = b->desc_bytes / 4;
    D.best_lr = b->best_lr != 0;
    if (max_rows > 0) {  // a workgroup past its pair's rows in its direction returns at once
        const dim3 grid(n, (max_rows + kDmNT - 1) / kDmNT, 2);
        if (D.dwords <= 8) hipLaunchKernelGGL(k_desc_nn<8>, grid, dim3(kDmNT), 0, s, D);
        else hipLaunchKernelGGL(k_desc_nn<16>, grid, dim3(kDmNT), 0, s, D);
        PLBA_LAUNCHED(ctx, "k_desc_nn");
    }
    hipLaunchKernelGGL(k_desc_cross, dim3(n), dim3(kDmNT), 0, s, D); PLBA_LAUNCHED(ctx, "k_desc_cross");
    PLBA_CHECK(hipMemcpyAsync(h + inputs_end, dv + inputs_end, outputs_end - inputs_end, hipMemcpyDeviceToHost, s));
    PLBA_CHECK(hipStreamSynchronize(s));
    if (n1) memcpy(matches_12, h + o_m12, sizeof(int32_t) * n1);
    memcpy(n_matches, h + o_cnt, sizeof(int32_t) * n);
    return PLBA_OK;
}

// ---------------------------------------------------------------- grid-guided matching
// StVO::matchGrid (src2/matching.cpp:111-258) for a batch of point and line problems: one upload, a
// fill of the key arrays, k_grid_cols twice (best, then second best) and k_grid_rows
// (csrc/plba_gridmatch.hpp), one read-back.
int grid_match(CtxBase &cb, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches) {
    CtxBase *const ctx = &cb;
    const char *const op = "grid matching";
    if (!b || b->n < 0) {
        ctx->set_error("grid matching: NULL batch or n < 0");
        return PLBA_E_INVALID;
    }
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    if (const int rc = check_desc_bytes(ctx, op, b->desc_bytes)) return rc;
    if (b->cols <= 0 || b->rows <= 0) {
        ctx->set_error("grid matching: a grid of %d x %d cells", b->cols, b->rows);
        return PLBA_E_INVALID;
    }
    if (!b->off1 || !b->off2 || !b->kind || !b->ws || !b->nnr || !b->line_sim_th || !n_matches) {
        ctx->set_error("grid matching: NULL off1 / off2 / kind / ws / nnr / line_sim_th / n_matches");
        return PLBA_E_INVALID;
    }
    for (const int32_t *off : {b->off1, b->off2})
        if (const int rc = check_offsets(ctx, op, "row", "problem", off, n)) return rc;
    int max_train = 0;
    bool line_q = false, line_t = false;  // a line problem with query rows / with train rows
    for (int k = 0; k < n; ++k) {
        if (b->kind[k] != 0 && b->kind[k] != 1) {
            ctx->set_error("grid matching: kind %d of problem %d", b->kind[k], k);
            return PLBA_E_INVALID;
        }
        if (b->ws[k] < 0) {
            ctx->set_error("grid matching: window half-width %d of problem %d", b->ws[k], k);
            return PLBA_E_INVALID;
        }
        max_train = std::max(max_train, b->off2[k + 1] - b->off2[k]);
        line_q = line_q || (b->kind[k] == 1 && b->off1[k + 1] > b->off1[k]);
        line_t = line_t || (b->kind[k] == 1 && b->off2[k + 1] > b->off2[k]);
    }
    if (max_train > kGmMaxTrain) {  // the low 16 bits of a key
        ctx->set_error("grid matching: %d train rows in a problem are more than %d", max_train, kGmMaxTrain);
        return PLBA_E_INVALID;
    }
    const size_t n1 = (size_t)b->off1[n], n2 = (size_t)b->off2[n], db = (size_t)b->desc_bytes;
    if ((n1 && (!b->desc1 || !b->cell1 || !matches_12)) || (n2 && (!b->desc2 || !b->cell_off2)) ||
        (line_q && !b->cell1_end) || (line_t && !b->dir2)) {
        ctx->set_error("grid matching: NULL desc1 / cell1 / cell1_end / matches_12 / desc2 / cell_off2 / dir2");
        return PLBA_E_INVALID;
    }
    size_t nc = 0;  // the kernels index cells2 through cell_off2: every entry is checked here
    if (n2) {
        if (const int rc = check_offsets(ctx, op, "cell", "train row", b->cell_off2, (int)n2)) return rc;
        nc = (size_t)b->cell_off2[n2];
        if (nc && !b->cells2) {
            ctx->set_error("grid matching: NULL cells2");
            return PLBA_E_INVALID;
        }
    }
    (void)hipSetDevice(ctx->opts.device);
    // one block; the pinned host image holds its inputs and outputs
    Layout L;
    const size_t o_off1 = L.add<int32_t>(n + 1), o_off2 = L.add<int32_t>(n + 1), o_kind = L.add<int32_t>(n),
                 o_ws = L.add<int32_t>(n), o_nnr = L.add<double>(n), o_th = L.add<double>(n), o_d1 = L.add(db * n1),
                 o_d2 = L.add(db * n2), o_c1 = L.add<int32_t>(2 * n1), o_c1e = L.add<int32_t>(2 * n1),
                 o_co2 = L.add<int32_t>(n2 + 1), o_cl2 = L.add<int32_t>(2 * nc), o_dir = L.add<double>(2 * n2);
    const size_t inputs_end = L.mark();  // host -> device
    const size_t o_m12 = L.add<int32_t>(n1), o_cnt = L.add<int32_t>(n);
    const size_t outputs_end = L.mark();  // device -> host
    const size_t o_best = L.add<uint32_t>(n1), o_sec = L.add<uint32_t>(n1);
    const size_t keys_end = L.mark();  // the key arrays start as kGmNone
    const size_t o_m21 = L.add<int32_t>(n2);  // device only, as the keys
    if (const int rc = ctx->match.reserve(cb, L.total, outputs_end, op)) return rc;
    char *h = ctx->match.host, *dv = ctx->match.dev;
    put(h, o_off1, b->off1, n + 1);
    put(h, o_off2, b->off2, n + 1);
    put(h, o_kind, b->kind, n);
    put(h, o_ws, b->ws, n);
    put(h, o_nnr, b->nnr, n);
    put(h, o_th, b->line_sim_th, n);
    put(h, o_d1, b->desc1, db * n1);
    put(h, o_d2, b->desc2, db * n2);
    put(h, o_c1, b->cell1, 2 * n1);
    put(h, o_c1e, b->cell1_end, 2 * n1);
    if (n2) put(h, o_co2, b->cell_off2, n2 + 1);
    else memset(h + o_co2, 0, sizeof(int32_t));
    put(h, o_cl2, b->cells2, 2 * nc);
    put(h, o_dir, b->dir2, 2 * n2);
    hipStream_t s = ctx->stream;
    PLBA_CHECK(hipMemcpyAsync(dv, h, inputs_end, hipMemcpyHostToDevice, s));
    PLBA_CHECK(hipMemsetAsync(dv + o_best, 0xFF, keys_end - o_best, s));  // kGmNone in every key
    GmDev D{};
    D.off1 = at<const int32_t>(dv, o_off1);
    D.off2 = at<const int32_t>(dv, o_off2);
    D.kind = at<const int32_t>(dv, o_kind);
    D.ws = at<const int32_t>(dv, o_ws);
    D.nnr = at<const double>(dv, o_nnr);
    D.sim_th = at<const double>(dv, o_th);
    D.desc1 = at<const uint32_t>(dv, o_d1);
    D.desc2 = at<const uint32_t>(dv, o_d2);
    D.cell1 = at<const int32_t>(dv, o_c1);
    D.cell1e = at<const int32_t>(dv, o_c1e);
    D.cell_off2 = at<const int32_t>(dv, o_co2);
    D.cells2 = at<const int32_t>(dv, o_cl2);
    D.dir2 = at<const double>(dv, o_dir);
    D.m12 = at<int32_t>(dv, o_m12);
    D.count = at<int32_t>(dv, o_cnt);
    D.best = at<uint32_t>(dv, o_best);
    D.second = at<uint32_t>(dv, o_sec);
    D.m21 = at<int32_t>(dv, o_m21);
    D.n = n;
    D.dwords = b->desc_bytes / 4;
    D.cols = b->cols;
    D.rows = b->rows;
    D.best_lr = b->best_lr != 0;
    if (max_train > 0) {  // a workgroup past its problem's train rows returns at once
        const dim3 grid(n, (max_train + kGmNT - 1) / kGmNT);
        if (D.dwords <= 8) {
            hipLaunchKernelGGL((k_grid_cols<8, 0>), grid, dim3(kGmNT), 0, s, D);
            hipLaunchKernelGGL((k_grid_cols<8, 1>), grid, dim3(kGmNT), 0, s, D);
        } else {
            hipLaunchKernelGGL((k_grid_cols<16, 0>), grid, dim3(kGmNT), 0, s, D);
            hipLaunchKernelGGL((k_grid_cols<16, 1>), grid, dim3(kGmNT), 0, s, D);
        }
        PLBA_LAUNCHED(ctx, "k_grid_cols");
    }
    hipLaunchKernelGGL(k_grid_rows, dim3(n), dim3(kGmRowsNT), 0, s, D); PLBA_LAUNCHED(ctx, "k_grid_rows");
    PLBA_CHECK(hipMemcpyAsync(h + inputs_end, dv + inputs_end, outputs_end - inputs_end, hipMemcpyDeviceToHost, s));
    PLBA_CHECK(hipStreamSynchronize(s));
    if (n1) memcpy(matches_12, h + o_m12, sizeof(int32_t) * n1);
    memcpy(n_matches, h + o_cnt, sizeof(int32_t) * n);
    return PLBA_OK;
}

}  // namespace plba
