// plba_assoc.hip — host side of the data-association entry points: the loop-closure relative pose,
// the frame-to-frame pose and tracking, the two descriptor matchers, the stereo, the keyframe and the map association, the median descriptor and
// place recognition. They share nothing with the solver (no Dev, no step graph, no window arena), so
// they are a translation unit of their own: an edit to a matcher does not rebuild the factorisation
// kernels. Each call is one upload, its kernels and one read-back through a ScratchBlock. A Staged
// (csrc/plba_layout.hpp) lays the block out: the call declares each array once, by its kernel-struct
// field, role, count and host source or destination; stage() then fills the pinned image and the
// fields, fetch() delivers the outputs. The three association calls run in phases (validate, plan,
// fill, launch, scatter) over a plan of csrc/plba_assoc_plan.hpp, which needs no device.
// The extern "C" symbols are forwarders in plba.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "plba_lcpose.hpp"
#include "plba_trackpose.hpp"
#include "plba_trackframes.hpp"
#include "plba_match.hpp"
#include "plba_gridmatch.hpp"
#include "plba_stereo.hpp"
#include "plba_kfassoc.hpp"
#include "plba_mapassoc.hpp"
#include "plba_bow.hpp"
#include "plba_medoid.hpp"
#include "plba_assoc_plan.hpp"
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

// Every coordinate of `rows` rows of PER values (x, y[, x, y]) lies at most one image size outside the
// image, which bounds the walk of a rasterised line.
// "<op>: coordinate V of <side> <kind> row K is not finite or outside [A, B]"
template <typename T, int PER>
int check_coords(CtxBase *ctx, const char *op, const char *side, const char *kind, const T *c, size_t rows, double width,
                 double height) {
    for (size_t e = 0; e < rows * PER; ++e) {
        const double v = c[e], size = (e & 1) ? height : width;
        if (!(v >= -size && v <= 2.0 * size)) {  // false for NaN
            ctx->set_error("%s: coordinate %g of %s %s row %zu is not finite or outside [%g, %g]", op, v, side, kind, e / PER,
                           -size, 2.0 * size);
            return PLBA_E_INVALID;
        }
    }
    return PLBA_OK;
}

// the one upload of a call: the inputs of the pinned image to the device
int upload(CtxBase *ctx, const ScratchBlock &k, const Staged &B) {
    PLBA_CHECK(hipMemcpyAsync(k.dev, k.host, B.inputs_end(), hipMemcpyHostToDevice, ctx->stream));
    return PLBA_OK;
}

// the one read-back of a call: the outputs into the pinned image, and the wait for them
int read_back(CtxBase *ctx, const ScratchBlock &k, const Staged &B) {
    const size_t from = B.inputs_end();
    PLBA_CHECK(hipMemcpyAsync(k.host + from, k.dev + from, B.outputs_end() - from, hipMemcpyDeviceToHost, ctx->stream));
    PLBA_CHECK(hipStreamSynchronize(ctx->stream));
    return PLBA_OK;
}

// The grid matcher's device side on a GmDev whose arrays are bound, in two steps so that the stereo
// path can launch k_stereo_cells between them. First its scalars and kGmNone in every key (best
// and second are one range of key_bytes):
int grid_prepare(CtxBase *ctx, GmDev &D, int n, int desc_bytes, int cols, int rows, int best_lr, size_t key_bytes) {
    PLBA_CHECK(hipMemsetAsync(D.best, 0xFF, key_bytes, ctx->stream));
    D.n = n;
    D.dwords = desc_bytes / 4;
    D.cols = cols;
    D.rows = rows;
    D.best_lr = best_lr != 0;
    return PLBA_OK;
}

// then k_grid_cols for the best and for the second-best key, and k_grid_rows
int grid_launch(CtxBase *ctx, const GmDev &D, int max_train) {
    hipStream_t s = ctx->stream;
    const int n = D.n;
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
    return PLBA_OK;
}

// the arrays of a GmDev that the struct O owns (an StDev, a KfDev or a MaDev, whose kernels make the cells)
template <typename Owner>
void grid_bind(GmDev &D, const Owner &O) {
    D.off1 = O.off1; D.off2 = O.off2; D.kind = O.kind;
    D.cell1 = O.cell1; D.cell1e = O.cell1e; D.cell_off2 = O.cell_off2; D.cells2 = O.cells2; D.dir2 = O.dir2;
}

// The brute-force matcher's device side on a DmDev that is bound and has its scalars: k_desc_nn over
// both directions of every pair, then k_desc_cross
int desc_launch(CtxBase *ctx, const DmDev &M, int max_rows) {
    hipStream_t s = ctx->stream;
    if (max_rows > 0) {  // a workgroup past its pair's rows in its direction, or of a pair that its gate switches off, returns at once
        const dim3 grid(M.n, (max_rows + kDmNT - 1) / kDmNT, 2);
        if (M.skip1) {  // plba_map_associate: the side-1 rows with a flag take no part
            if (M.dwords <= 8) hipLaunchKernelGGL((k_desc_nn<8, true>), grid, dim3(kDmNT), 0, s, M);
            else hipLaunchKernelGGL((k_desc_nn<16, true>), grid, dim3(kDmNT), 0, s, M);
        } else {
            if (M.dwords <= 8) hipLaunchKernelGGL(k_desc_nn<8>, grid, dim3(kDmNT), 0, s, M);
            else hipLaunchKernelGGL(k_desc_nn<16>, grid, dim3(kDmNT), 0, s, M);
        }
        PLBA_LAUNCHED(ctx, "k_desc_nn");
    }
    hipLaunchKernelGGL(k_desc_cross, dim3(M.n), dim3(kDmNT), 0, s, M); PLBA_LAUNCHED(ctx, "k_desc_cross");
    return PLBA_OK;
}

}  // namespace

// ---------------------------------------------------------------- loop-closure relative pose
// MapHandler::computeRelativePoseRobustGN / computeRelativePoseGN (src/mapHandler.cpp:4677-5068,
// :4413-4675) for a batch of candidate pairs: one upload, one launch of k_lcpose
// (csrc/plba_lcpose.hpp, one workgroup per candidate), one read-back.
int lc_relative_pose(CtxBase *ctx, const plba_lcpose_batch *b, const plba_lcpose_params *pp, plba_lcpose_out *out,
                     uint8_t *pt_inlier, uint8_t *ln_inlier) {
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
    LcDev D{};
    Staged B;
    B.in(D.pt_off, n + 1, b->pt_off);
    B.in(D.ln_off, n + 1, b->ln_off);
    B.in(D.pt_P, 3 * np, b->pt_P);
    B.in(D.pt_obs, 2 * np, b->pt_obs);
    B.in(D.ln_sP, 3 * nl, b->ln_sP);
    B.in(D.ln_eP, 3 * nl, b->ln_eP);
    B.in(D.ln_le, 3 * nl, b->ln_le);
    B.out(D.out, n, out);
    B.out(D.pt_in, np, pt_inlier);
    B.out(D.ln_in, nl, ln_inlier);
    if (const int rc = ctx->lc.reserve(*ctx, B.outputs_end(), B.outputs_end(), op)) return rc;
    B.stage(ctx->lc.host, ctx->lc.dev);
    if (const int rc = upload(ctx, ctx->lc, B)) return rc;
    D.cam = Cam{b->fx, b->fy, b->cx, b->cy};
    D.prm = prm;
    hipLaunchKernelGGL(k_lcpose, dim3(n), dim3(kLcNT), 0, ctx->stream, D); PLBA_LAUNCHED(ctx, "k_lcpose");
    if (const int rc = read_back(ctx, ctx->lc, B)) return rc;
    B.fetch();
    return PLBA_OK;
}

// ---------------------------------------------------------------- frame-to-frame pose
// StereoFrameHandler::optimizePose (src2/stereoFrameHandler.cpp:307-405) for a batch of frame pairs:
// one upload, one launch of k_trackpose (csrc/plba_trackpose.hpp, one workgroup per problem), one
// read-back. The block is laid out by trackpose_plan (csrc/plba_assoc_plan.hpp).
int track_pose(CtxBase *ctx, const plba_track_batch *b, const plba_track_params *pp, plba_track_out *out,
               uint8_t *pt_inlier, uint8_t *ln_inlier) {
    const char *const op = "track pose";
    if (!b || b->n < 0) {
        ctx->set_error("track pose: NULL batch or n < 0");
        return PLBA_E_INVALID;
    }
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    plba_track_params prm;
    if (pp) prm = *pp;
    else plba_track_default_params(&prm);
    if (!out || !b->pt_off || !b->ln_off) {
        ctx->set_error("track pose: NULL out / pt_off / ln_off");
        return PLBA_E_INVALID;
    }
    if ((prm.line_model != PLBA_TRACK_PLUCKER && prm.line_model != PLBA_TRACK_ENDPOINTS) || prm.max_iters < 1 ||
        prm.max_iters_ref < 1) {
        ctx->set_error("track pose: unknown line model %d or an iteration cap below 1", prm.line_model);
        return PLBA_E_INVALID;
    }
    const bool pluker = prm.line_model == PLBA_TRACK_PLUCKER, motion = prm.use_motion_model != 0;
    int widest = 0;
    for (const int32_t *off : {b->pt_off, b->ln_off})
        if (const int rc = check_offsets(ctx, op, "match", "problem", off, n, &widest)) return rc;
    if (widest > kTpMaxN) {
        ctx->set_error("track pose: %d matches of one kind in one problem, PLBA_TRACK_MAX_N is %d", widest, kTpMaxN);
        return PLBA_E_INVALID;
    }
    const size_t np = (size_t)b->pt_off[n], nl = (size_t)b->ln_off[n];
    if ((np && (!b->pt_P || !b->pt_obs || !b->pt_sigma2)) ||
        (nl && (!b->ln_sP || !b->ln_eP || !b->ln_seg || !b->ln_sigma2 || (pluker ? (!b->ln_NDc || !b->ln_obs) : !b->ln_le)))) {
        ctx->set_error("track pose: NULL match array");
        return PLBA_E_INVALID;
    }
    if (motion && !b->prev) {
        ctx->set_error("track pose: use_motion_model without prev");
        return PLBA_E_INVALID;
    }
    (void)hipSetDevice(ctx->opts.device);
    TpDev D{};
    Staged B;
    trackpose_plan(B, D, b, pluker, motion, out, pt_inlier, ln_inlier);
    if (const int rc = ctx->track.reserve(*ctx, B.total(), B.outputs_end(), op)) return rc;
    B.stage(ctx->track.host, ctx->track.dev);
    if (const int rc = upload(ctx, ctx->track, B)) return rc;
    D.fx = b->fx, D.fy = b->fy, D.cx = b->cx, D.cy = b->cy;
    D.prm = prm;
    if (pluker) hipLaunchKernelGGL(k_trackpose<PLBA_TRACK_PLUCKER>, dim3(n), dim3(kTpNT), 0, ctx->stream, D);
    else hipLaunchKernelGGL(k_trackpose<PLBA_TRACK_ENDPOINTS>, dim3(n), dim3(kTpNT), 0, ctx->stream, D);
    PLBA_LAUNCHED(ctx, "k_trackpose");
    if (const int rc = read_back(ctx, ctx->track, B)) return rc;
    B.fetch();
    return PLBA_OK;
}

// ---------------------------------------------------------------- descriptor matching
// StVO::match / matchNNR (src2/matching.cpp:41-91) for a batch of descriptor-set pairs: one upload,
// k_desc_nn (both directions of every pair) and k_desc_cross (csrc/plba_match.hpp), one read-back.
int desc_match(CtxBase *ctx, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches) {
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
    const size_t n1 = (size_t)b->off1[n], n2 = (size_t)b->off2[n], dw = (size_t)b->desc_bytes / 4;
    if ((n1 && (!b->desc1 || !matches_12)) || (n2 && !b->desc2)) {
        ctx->set_error("descriptor matching: NULL desc1 / desc2 / matches_12");
        return PLBA_E_INVALID;
    }
    (void)hipSetDevice(ctx->opts.device);
    DmDev D{};
    Staged B;
    B.in(D.off1, n + 1, b->off1);
    B.in(D.off2, n + 1, b->off2);
    B.in(D.nnr, n, b->nnr);
    B.in(D.desc1, dw * n1, b->desc1);
    B.in(D.desc2, dw * n2, b->desc2);
    B.out(D.m12, n1, matches_12);
    B.out(D.count, n, n_matches);
    B.dev(D.nn12, n1);
    B.dev(D.nn21, n2);
    if (const int rc = ctx->match.reserve(*ctx, B.total(), B.outputs_end(), op)) return rc;
    B.stage(ctx->match.host, ctx->match.dev);
    if (const int rc = upload(ctx, ctx->match, B)) return rc;
    D.n = n;
    D.dwords = b->desc_bytes / 4;
    D.best_lr = b->best_lr != 0;
    if (const int rc = desc_launch(ctx, D, max_rows)) return rc;
    if (const int rc = read_back(ctx, ctx->match, B)) return rc;
    B.fetch();
    return PLBA_OK;
}

// ---------------------------------------------------------------- frame-to-frame tracking
// StereoFrameHandler::f2fTracking + optimizePose (src2/stereoFrameHandler.cpp:106-180, :307-405) for a
// batch of frame pairs: one upload, the matcher's two launches over the points and the lines of every
// pair, k_f2f_gather, k_trackpose, k_f2f_scatter (csrc/plba_trackframes.hpp), one read-back. The block
// is laid out by TfPlan (csrc/plba_assoc_plan.hpp).
namespace {

// everything that is refused, before any device call; T is initialised on the way
int frames_validate(CtxBase *ctx, const plba_frames_batch *b, const plba_frames_params &prm, const plba_frames_out *out,
                    ProblemTable &T) {
    const char *const op = "track frames";
    const int n = b->n;
    const plba_track_params &tp = prm.track;
    if (const int rc = check_desc_bytes(ctx, op, prm.desc_bytes)) return rc;
    if (!out || !out->out || !out->n_pt || !out->n_ln || !b->pt_off1 || !b->pt_off2 || !b->ln_off1 || !b->ln_off2) {
        ctx->set_error("track frames: NULL out / n_pt / n_ln / offsets");
        return PLBA_E_INVALID;
    }
    if ((tp.line_model != PLBA_TRACK_PLUCKER && tp.line_model != PLBA_TRACK_ENDPOINTS) || tp.max_iters < 1 ||
        tp.max_iters_ref < 1) {
        ctx->set_error("track frames: unknown line model %d or an iteration cap below 1", tp.line_model);
        return PLBA_E_INVALID;
    }
    if (n > (INT32_MAX - 1) / 2) {
        ctx->set_error("track frames: %d pairs are more than %d", n, (INT32_MAX - 1) / 2);
        return PLBA_E_INVALID;
    }
    const bool pluker = tp.line_model == PLBA_TRACK_PLUCKER;
    int widest_prev = 0, widest = 0;
    const int32_t *const offs[4] = {b->pt_off1, b->ln_off1, b->pt_off2, b->ln_off2};
    for (int a = 0; a < 4; ++a) {
        if (const int rc = check_offsets(ctx, op, a % 2 ? "line" : "point", "pair", offs[a], n, a < 2 ? &widest_prev : &widest))
            return rc;
        if (offs[a][0] != 0) {
            ctx->set_error("track frames: %s offsets start at %d, not at 0", a % 2 ? "line" : "point", offs[a][0]);
            return PLBA_E_INVALID;
        }
    }
    if (widest_prev > kTpMaxN) {
        ctx->set_error("track frames: a previous frame has %d rows of one kind, PLBA_TRACK_MAX_N is %d", widest_prev, kTpMaxN);
        return PLBA_E_INVALID;
    }
    widest = std::max(widest, widest_prev);
    if ((widest + kDmNT - 1) / kDmNT > 65535) {  // the matcher's row tiles are its grid's second dimension
        ctx->set_error("track frames: a set of %d rows is more than %d", widest, 65535 * kDmNT);
        return PLBA_E_INVALID;
    }
    if (T.init(b->pt_off1, b->pt_off2, b->ln_off1, b->ln_off2, n, 0, 0) == ProblemTable::kTooMany) {
        ctx->set_error("track frames: more than %d rows on one side of the batch", INT32_MAX);
        return PLBA_E_INVALID;
    }
    const size_t p1 = T.cnt[0][0], p2 = T.cnt[0][1], l1 = T.cnt[1][0], l2 = T.cnt[1][1];
    if ((p1 && (!b->prev_pdesc || !b->prev_pt_P || !b->prev_pt_sigma2 || !out->pt_m12)) ||
        (p2 && (!b->cur_pdesc || !b->cur_pt_pl || !out->pt_cur_from_prev)) ||
        (l1 && (!b->prev_ldesc || !b->prev_ln_sP || !b->prev_ln_eP || !b->prev_ln_seg || !b->prev_ln_sigma2 || !out->ln_m12 ||
                (pluker && !b->prev_ln_NDc))) ||
        (l2 && (!b->cur_ldesc || !out->ln_cur_from_prev || (pluker ? !b->cur_ln_seg : !b->cur_ln_le)))) {
        ctx->set_error("track frames: NULL feature or output array");
        return PLBA_E_INVALID;
    }
    if (tp.use_motion_model && !b->prev) {
        ctx->set_error("track frames: use_motion_model without prev");
        return PLBA_E_INVALID;
    }
    return PLBA_OK;
}

// the scalars of the three structs, the arrays they share, and the launches
int frames_launch(CtxBase *ctx, TfPlan &Q, const plba_frames_batch *b, const plba_frames_params &prm) {
    TfDev &F = Q.F;
    DmDev &M = Q.M;
    TpDev &P = Q.P;
    const int n = Q.T.n;
    hipStream_t s = ctx->stream;
    M.off1 = F.off1; M.off2 = F.off2;
    M.n = 2 * n;
    M.dwords = prm.desc_bytes / 4;
    M.best_lr = prm.best_lr != 0;
    F.m12 = M.m12; F.count = M.count;
    F.tin[0] = P.pt_in; F.tin[1] = P.ln_in;
    for (int kd = 0; kd < 2; ++kd) F.cap[kd] = (int32_t)Q.T.cnt[kd][0];
    F.on[0] = prm.track.has_points != 0; F.on[1] = prm.track.has_lines != 0;
    F.n = n;
    F.pluker = prm.track.line_model == PLBA_TRACK_PLUCKER;
    P.pt_off = F.g_off[0]; P.ln_off = F.g_off[1];
    P.pt_P = F.g_pt_P; P.pt_obs = F.g_pt_obs; P.pt_s2 = F.g_pt_s2;
    P.ln_sP = F.g_ln_sP; P.ln_eP = F.g_ln_eP; P.ln_ND = F.g_ln_ND; P.ln_le = F.g_ln_le;
    P.ln_obs = F.g_ln_obs; P.ln_seg = F.g_ln_seg; P.ln_s2 = F.g_ln_s2;
    P.fx = b->fx, P.fy = b->fy, P.cx = b->cx, P.cy = b->cy;
    P.prm = prm.track;
    if (const int rc = desc_launch(ctx, M, Q.T.max_rows)) return rc;
    hipLaunchKernelGGL(k_f2f_gather, dim3(2 * n), dim3(kTfNT), 0, s, F); PLBA_LAUNCHED(ctx, "k_f2f_gather");
    if (F.pluker) hipLaunchKernelGGL(k_trackpose<PLBA_TRACK_PLUCKER>, dim3(n), dim3(kTpNT), 0, s, P);
    else hipLaunchKernelGGL(k_trackpose<PLBA_TRACK_ENDPOINTS>, dim3(n), dim3(kTpNT), 0, s, P);
    PLBA_LAUNCHED(ctx, "k_trackpose");
    hipLaunchKernelGGL(k_f2f_scatter, dim3(2 * n), dim3(kTfNT), 0, s, F); PLBA_LAUNCHED(ctx, "k_f2f_scatter");
    return PLBA_OK;
}

}  // namespace

int track_frames(CtxBase *ctx, const plba_frames_batch *b, const plba_frames_params *pp, const plba_frames_out *out) {
    if (!b || b->n < 0) {
        ctx->set_error("track frames: NULL batch or n < 0");
        return PLBA_E_INVALID;
    }
    if (b->n == 0) return PLBA_OK;
    plba_frames_params prm;
    if (pp) prm = *pp;
    else plba_frames_default_params(&prm);
    TfPlan Q;
    if (const int rc = frames_validate(ctx, b, prm, out, Q.T)) return rc;
    (void)hipSetDevice(ctx->opts.device);
    Q.declare((size_t)prm.desc_bytes / 4, b, prm.track.line_model == PLBA_TRACK_PLUCKER, prm.track.use_motion_model != 0, out);
    if (const int rc = ctx->match.reserve(*ctx, Q.B.total(), Q.B.outputs_end(), "track frames")) return rc;
    Q.B.stage(ctx->match.host, ctx->match.dev);
    const uint8_t *const descs[2][2] = {{b->prev_pdesc, b->cur_pdesc}, {b->prev_ldesc, b->cur_ldesc}};
    std::vector<int32_t> kind(2 * (size_t)b->n), cbase(2 * (size_t)b->n + 1);  // the table's, not read on the device
    Q.T.fill(Q.B.host(Q.F.off1), Q.B.host(Q.F.off2), kind.data(), Q.B.host(Q.F.kb1), Q.B.host(Q.F.kb2), cbase.data(), descs,
             (size_t)prm.desc_bytes, (uint8_t *)Q.B.host(Q.M.desc1), (uint8_t *)Q.B.host(Q.M.desc2));
    float *nnr = Q.B.host(Q.M.nnr);
    for (int k = 0; k < b->n; ++k) nnr[2 * k] = prm.nnr_pt, nnr[2 * k + 1] = prm.nnr_ln;
    if (const int rc = upload(ctx, ctx->match, Q.B)) return rc;
    if (const int rc = frames_launch(ctx, Q, b, prm)) return rc;
    if (const int rc = read_back(ctx, ctx->match, Q.B)) return rc;
    Q.B.fetch();
    return PLBA_OK;
}

// ---------------------------------------------------------------- grid-guided matching
// StVO::matchGrid (src2/matching.cpp:111-258) for a batch of point and line problems: one upload, a
// fill of the key arrays, k_grid_cols twice (best, then second best) and k_grid_rows
// (csrc/plba_gridmatch.hpp), one read-back.
int grid_match(CtxBase *ctx, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches) {
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
    const size_t n1 = (size_t)b->off1[n], n2 = (size_t)b->off2[n], dw = (size_t)b->desc_bytes / 4;
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
    GmDev D{};
    Staged B;
    B.in(D.off1, n + 1, b->off1);
    B.in(D.off2, n + 1, b->off2);
    B.in(D.kind, n, b->kind);
    B.in(D.ws, 4 * (size_t)n);  // filled below
    B.in(D.nnr, n, b->nnr);
    B.in(D.sim_th, n, b->line_sim_th);
    B.in(D.desc1, dw * n1, b->desc1);
    B.in(D.desc2, dw * n2, b->desc2);
    B.in(D.cell1, 2 * n1, b->cell1);
    B.in(D.cell1e, 2 * n1, b->cell1_end);
    B.in(D.cell_off2, n2 + 1, n2 ? b->cell_off2 : nullptr);  // without train rows: one zero, below
    B.in(D.cells2, 2 * nc, b->cells2);
    B.in(D.dir2, 2 * n2, b->dir2);
    B.out(D.m12, n1, matches_12);
    B.out(D.count, n, n_matches);
    const size_t o_best = B.dev(D.best, n1);
    B.dev(D.second, n1);
    const size_t key_bytes = B.mark() - o_best;  // the two key arrays start as kGmNone
    B.dev(D.m21, n2);
    if (const int rc = ctx->match.reserve(*ctx, B.total(), B.outputs_end(), op)) return rc;
    B.stage(ctx->match.host, ctx->match.dev);
    int32_t *const ws = B.host(D.ws);
    for (int k = 0; k < n; ++k)  // the symmetric window of matchGrid's callers: ws to the left, right, up and down
        for (int e = 0; e < 4; ++e) ws[4 * k + e] = b->ws[k];
    if (!n2) B.host(D.cell_off2)[0] = 0;
    if (const int rc = upload(ctx, ctx->match, B)) return rc;
    if (const int rc = grid_prepare(ctx, D, n, b->desc_bytes, b->cols, b->rows, b->best_lr, key_bytes)) return rc;
    if (const int rc = grid_launch(ctx, D, max_train)) return rc;
    if (const int rc = read_back(ctx, ctx->match, B)) return rc;
    B.fetch();
    return PLBA_OK;
}

// ---------------------------------------------------------------- stereo association
// StereoFrame::matchStereoPoints / matchStereoLines (src2/stereoFrame.cpp:121-174, :310-435) for a batch
// of frames: one upload, k_stereo_cells, the matcher's three launches with the window
// (matching_s_ws, 0, 0, 0), k_stereo_gate (csrc/plba_stereo.hpp), one read-back. Frame f is the
// matcher's problems 2 f (points) and 2 f + 1 (lines).
namespace {

// everything that refuses the call, and the table; no device call
int stereo_validate(CtxBase *ctx, const plba_stereo_batch *b, const plba_stereo_params *pp, const plba_stereo_out *out,
                    ProblemTable &T) {
    const char *const op = "stereo association";
    const int n = b->n;
    if (n > (INT32_MAX - 1) / 2) {
        ctx->set_error("stereo association: %d frames", n);
        return PLBA_E_INVALID;
    }
    if (const int rc = check_desc_bytes(ctx, op, b->desc_bytes)) return rc;
    if (!pp || !out || !out->n_pt || !out->n_ls || !b->pt_off_l || !b->pt_off_r || !b->ls_off_l || !b->ls_off_r) {
        ctx->set_error("stereo association: NULL params / out / n_pt / n_ls / offsets");
        return PLBA_E_INVALID;
    }
    const plba_stereo_params &prm = *pp;
    if (prm.cols <= 0 || prm.rows <= 0 || prm.width <= 0 || prm.height <= 0 || prm.matching_s_ws < 0) {
        ctx->set_error("stereo association: a grid of %d x %d cells, an image of %d x %d or a window of %d", prm.cols,
                       prm.rows, prm.width, prm.height, prm.matching_s_ws);
        return PLBA_E_INVALID;
    }
    for (const int32_t *off : {b->pt_off_l, b->pt_off_r, b->ls_off_l, b->ls_off_r})
        if (const int rc = check_offsets(ctx, op, "row", "frame", off, n)) return rc;
    const int bad = T.init(b->pt_off_l, b->pt_off_r, b->ls_off_l, b->ls_off_r, n, prm.cols, prm.rows);
    if (bad == T.kTooMany) {
        ctx->set_error("stereo association: %zu left rows, %zu right rows or %zu cells are more than %d", T.N1, T.N2, T.nc, INT32_MAX);
        return PLBA_E_INVALID;
    }
    if ((T.cnt[0][0] && (!b->pt_l || !b->pdesc_l)) || (T.cnt[0][1] && (!b->pt_r || !b->pdesc_r)) ||
        (T.cnt[1][0] && (!b->ls_l || !b->ldesc_l)) || (T.cnt[1][1] && (!b->ls_r || !b->ldesc_r))) {
        ctx->set_error("stereo association: NULL coordinate or descriptor array");
        return PLBA_E_INVALID;
    }
    if (bad == T.kTooWide) {
        ctx->set_error("stereo association: %d right rows in a problem are more than %d", T.max_train, kGmMaxTrain);
        return PLBA_E_INVALID;
    }
    // the bound of a right line's walk
    const float *const coords[2][2] = {{b->pt_l, b->pt_r}, {b->ls_l, b->ls_r}};
    for (int kd = 0; kd < 2; ++kd)
        for (int sd = 0; sd < 2; ++sd) {
            const size_t rows = T.cnt[kd][sd];
            if (!rows) continue;
            const float *c = coords[kd][sd] + (size_t)(kd ? 4 : 2) * T.offs[kd][sd][0];
            const char *const side = sd ? "right" : "left";
            if (const int rc = kd ? check_coords<float, 4>(ctx, op, side, "line", c, rows, prm.width, prm.height)
                                  : check_coords<float, 2>(ctx, op, side, "point", c, rows, prm.width, prm.height))
                return rc;
        }
    return PLBA_OK;
}

// the inputs into the staged image, problem by problem
void stereo_fill(const StereoPlan &P, const plba_stereo_batch *b, const plba_stereo_params &prm) {
    const ProblemTable &T = P.T;
    const Staged &B = P.B;
    const uint8_t *const descs[2][2] = {{b->pdesc_l, b->pdesc_r}, {b->ldesc_l, b->ldesc_r}};
    const float *const coords[2][2] = {{b->pt_l, b->pt_r}, {b->ls_l, b->ls_r}};
    int32_t *off1 = B.host(P.S.off1), *off2 = B.host(P.S.off2), *ws = B.host(P.D.ws);
    T.fill(off1, off2, B.host(P.S.kind), B.host(P.S.kbase), nullptr, B.host(P.S.cbase), descs, (size_t)b->desc_bytes,
           (uint8_t *)B.host(P.S.desc1), (uint8_t *)B.host(P.D.desc2));
    double *nnr = B.host(P.D.nnr), *sim_th = B.host(P.D.sim_th);
    float *const co_h[2] = {B.host(P.S.co1), B.host(P.S.co2)};
    for (int p = 0; p < 2 * T.n; ++p) {
        const ProblemTable::Problem q = T.at(p);
        const int per = q.kind ? 4 : 2;
        ws[4 * p] = prm.matching_s_ws;  // w.width = (matchingSWs, 0), w.height = (0, 0) (:142-144)
        ws[4 * p + 1] = ws[4 * p + 2] = ws[4 * p + 3] = 0;
        nnr[p] = prm.min_ratio_12_p;  // matching.cpp:160, :241: for lines too
        sim_th[p] = prm.line_sim_th;
        for (int sd = 0; sd < 2; ++sd) {
            const int a = sd ? q.a2 : q.a1, r = sd ? q.r2 : q.r1;
            float *dst = co_h[sd] + 4 * (size_t)(sd ? off2[p] : off1[p]);
            const float *src = coords[q.kind][sd];
            for (int i = 0; i < r; ++i)
                for (int e = 0; e < 4; ++e) dst[4 * i + e] = e < per ? src[(size_t)per * (a + i) + e] : 0.0f;
        }
    }
}

// the scalars of both structs, the matcher's arrays handed over from S, and the five launches
int stereo_launch(CtxBase *ctx, StereoPlan &P, int desc_bytes, const plba_stereo_params &prm) {
    StDev &S = P.S;
    GmDev &D = P.D;
    const int np = 2 * P.T.n, max_rows = P.T.max_rows;
    hipStream_t s = ctx->stream;
    S.m12 = D.m12;
    S.inv_w = prm.cols / (double)prm.width;   // :47-48
    S.inv_h = prm.rows / (double)prm.height;
    S.dwords = desc_bytes / 4;
    S.stride = P.T.stride;
    S.prm = prm;
    grid_bind(D, S);
    D.desc1 = S.desc1;
    if (const int rc = grid_prepare(ctx, D, np, desc_bytes, prm.cols, prm.rows, prm.best_lr, P.key_bytes)) return rc;
    if (max_rows > 0) {  // a thread past its problem's rows does nothing
        hipLaunchKernelGGL(k_stereo_cells, dim3(np, (max_rows + kStNT - 1) / kStNT), dim3(kStNT), 0, s, S);
        PLBA_LAUNCHED(ctx, "k_stereo_cells");
    }
    if (const int rc = grid_launch(ctx, D, P.T.max_train)) return rc;
    hipLaunchKernelGGL(k_stereo_gate, dim3(np), dim3(kStNT), 0, s, S); PLBA_LAUNCHED(ctx, "k_stereo_gate");
    return PLBA_OK;
}

// the first count[p] rows of each problem, to the frame's left offset in the caller's arrays
int stereo_scatter(CtxBase *ctx, const StereoPlan &P, size_t db, int pluker, const plba_stereo_out *out) {
    const Staged &B = P.B;
    const int32_t *count = B.host(P.S.count), *src = B.host(P.S.src), *off1 = B.host(P.S.off1), *kbase = B.host(P.S.kbase);
    const double *ptd = B.host(P.S.ptd), *lsd = B.host(P.S.lsd);
    const uint8_t *odesc_h = (const uint8_t *)B.host(P.S.odesc);
    for (int p = 0; p < 2 * P.T.n; ++p) {
        const ProblemTable::Problem q = P.T.at(p);
        const int f = q.f, kd = q.kind, k = count[p], a1 = q.a1;
        if (k < 0 || k > q.r1) {
            ctx->set_error("stereo association: the device returned %d survivors for %d rows", k, q.r1);
            return PLBA_E_DEVICE;
        }
        (kd ? out->n_ls : out->n_pt)[f] = k;
        int32_t *osrc = kd ? out->ls_src : out->pt_src;
        uint8_t *odesc = kd ? out->ldesc : out->pdesc;
        if (osrc && k) memcpy(osrc + a1, src + off1[p], sizeof(int32_t) * k);
        if (odesc && k) memcpy(odesc + db * a1, odesc_h + db * off1[p], db * k);
        auto cols_out = [&](double *dst, const double *rec, int nd, int first, int width) {
            if (!dst) return;
            for (int i = 0; i < k; ++i)
                for (int e = 0; e < width; ++e) dst[(size_t)width * (a1 + i) + e] = rec[(size_t)nd * (kbase[p] + i) + first + e];
        };
        if (!kd) {
            cols_out(out->pt_pl, ptd, kStPtDoubles, 0, 2);
            cols_out(out->pt_disp, ptd, kStPtDoubles, 2, 1);
            cols_out(out->pt_P, ptd, kStPtDoubles, 3, 3);
        } else {
            cols_out(out->ls_spl, lsd, kStLsDoubles, 0, 2);
            cols_out(out->ls_epl, lsd, kStLsDoubles, 2, 2);
            cols_out(out->ls_sdisp, lsd, kStLsDoubles, 4, 1);
            cols_out(out->ls_edisp, lsd, kStLsDoubles, 5, 1);
            cols_out(out->ls_sP, lsd, kStLsDoubles, 6, 3);
            cols_out(out->ls_eP, lsd, kStLsDoubles, 9, 3);
            cols_out(out->ls_le, lsd, kStLsDoubles, 12, 3);
            if (pluker) cols_out(out->ls_NDc, lsd, kStLsDoubles, 15, 6);
        }
    }
    return PLBA_OK;
}

}  // namespace

int stereo_associate(CtxBase *ctx, const plba_stereo_batch *b, const plba_stereo_params *pp, const plba_stereo_out *out) {
    if (!b || b->n < 0) {
        ctx->set_error("stereo association: NULL batch or n < 0");
        return PLBA_E_INVALID;
    }
    if (b->n == 0) return PLBA_OK;
    StereoPlan P;
    if (const int rc = stereo_validate(ctx, b, pp, out, P.T)) return rc;
    (void)hipSetDevice(ctx->opts.device);
    P.declare((size_t)b->desc_bytes / 4);
    if (const int rc = ctx->match.reserve(*ctx, P.B.total(), P.B.outputs_end(), "stereo association")) return rc;
    P.B.stage(ctx->match.host, ctx->match.dev);
    stereo_fill(P, b, *pp);
    if (const int rc = upload(ctx, ctx->match, P.B)) return rc;
    if (const int rc = stereo_launch(ctx, P, b->desc_bytes, *pp)) return rc;
    if (const int rc = read_back(ctx, ctx->match, P.B)) return rc;
    return stereo_scatter(ctx, P, (size_t)b->desc_bytes, pp->pluker, out);
}

// ---------------------------------------------------------------- keyframe-to-keyframe association
// MapHandler::matchKF2KFPoints / matchKF2KFLines (src/mapHandler.cpp:237-366, :368-590) up to the
// sequential part, for a batch of keyframe pairs: one upload, k_kf_cells, the grid matcher's three
// launches with the window (ws, ws, ws, ws), the brute-force matcher's two, gated per problem on the
// device by the grid count, k_kf_geom (csrc/plba_kfassoc.hpp), one read-back. Pair f is the matcher's
// problems 2 f (points) and 2 f + 1 (lines).
namespace {

// everything that refuses the call, and the table; no device call
int kf_validate(CtxBase *ctx, const plba_kfassoc_batch *b, const plba_kfassoc_params *pp, const plba_kfassoc_out *out,
                ProblemTable &T) {
    const char *const op = "keyframe association";
    const int n = b->n;
    if (n > (INT32_MAX - 1) / 2) {
        ctx->set_error("keyframe association: %d pairs", n);
        return PLBA_E_INVALID;
    }
    if (const int rc = check_desc_bytes(ctx, op, b->desc_bytes)) return rc;
    if (!pp || !out || !out->n_grid || !out->n_matches || !out->fallback || !b->pt_off_p || !b->pt_off_c || !b->ls_off_p ||
        !b->ls_off_c || !b->DT || !b->T_prev || !b->T_curr || !b->Tcw_prev || !b->Tcw_curr) {
        ctx->set_error("keyframe association: NULL params / out / n_grid / n_matches / fallback / offsets / poses");
        return PLBA_E_INVALID;
    }
    const plba_kfassoc_params &prm = *pp;
    if (prm.cols <= 0 || prm.rows <= 0 || prm.width <= 0 || prm.height <= 0 || prm.ws < 0 || prm.ws >= (1 << 30)) {
        ctx->set_error("keyframe association: a grid of %d x %d cells, an image of %d x %d or a window of %d", prm.cols,
                       prm.rows, prm.width, prm.height, prm.ws);
        return PLBA_E_INVALID;
    }
    for (const int32_t *off : {b->pt_off_p, b->pt_off_c, b->ls_off_p, b->ls_off_c})
        if (const int rc = check_offsets(ctx, op, "row", "pair", off, n)) return rc;
    const int bad = T.init(b->pt_off_p, b->pt_off_c, b->ls_off_p, b->ls_off_c, n, prm.cols, prm.rows);
    if (bad == T.kTooMany) {
        ctx->set_error("keyframe association: %zu previous rows, %zu current rows or %zu cells are more than %d", T.N1, T.N2,
                       T.nc, INT32_MAX);
        return PLBA_E_INVALID;
    }
    if ((T.cnt[0][0] && (!b->pt_P_p || !b->pdesc_p)) || (T.cnt[0][1] && (!b->pt_pl_c || !b->pt_P_c || !b->pdesc_c)) ||
        (T.cnt[1][0] && (!b->ls_sP_p || !b->ls_eP_p || !b->ls_NDc_p || !b->ls_spl_p || !b->ls_epl_p || !b->ldesc_p ||
                         !b->ls_lm_NDw || !b->ls_new)) ||
        (T.cnt[1][1] && (!b->ls_spl_c || !b->ls_epl_c || !b->ldesc_c))) {
        ctx->set_error("keyframe association: NULL feature or descriptor array");
        return PLBA_E_INVALID;
    }
    if (bad == T.kTooWide) {
        ctx->set_error("keyframe association: %d current rows in a problem are more than %d", T.max_train, kGmMaxTrain);
        return PLBA_E_INVALID;
    }
    const double *const poses[5] = {b->DT, b->T_prev, b->T_curr, b->Tcw_prev, b->Tcw_curr};
    for (int k = 0; k < 5; ++k)
        for (size_t e = 0; e < (size_t)n * (k ? 16 : 12); ++e)
            if (!std::isfinite(poses[k][e])) {
                ctx->set_error("keyframe association: %s of pair %zu is not finite",
                               k == 0 ? "DT" : k == 1 ? "T_prev" : k == 2 ? "T_curr" : k == 3 ? "Tcw_prev" : "Tcw_curr",
                               e / (k ? 16 : 12));
                return PLBA_E_INVALID;
            }
    // the bound of a current line's walk
    const double *const ccoords[3] = {b->pt_pl_c, b->ls_spl_c, b->ls_epl_c};
    for (int k = 0; k < 3; ++k) {
        const int kd = k ? 1 : 0;
        if (!T.cnt[kd][1]) continue;
        const double *c = ccoords[k] + 2 * (size_t)T.offs[kd][1][0];
        if (const int rc = check_coords<double, 2>(ctx, op, "current", kd ? "line" : "point", c, T.cnt[kd][1], prm.width, prm.height))
            return rc;
    }
    return PLBA_OK;
}

// the inputs into the staged image: the poses pair by pair, the matchers' inputs problem by problem, the rows
void kf_fill(const KfPlan &P, const plba_kfassoc_batch *b, const plba_kfassoc_params &prm) {
    const ProblemTable &T = P.T;
    const Staged &B = P.B;
    const double *const poses[5] = {b->DT, b->T_prev, b->T_curr, b->Tcw_prev, b->Tcw_curr};
    const uint8_t *const descs[2][2] = {{b->pdesc_p, b->pdesc_c}, {b->ldesc_p, b->ldesc_c}};
    double *pose = B.host(P.K.pose);
    for (int f = 0; f < T.n; ++f) {
        double *q = pose + (size_t)kKfPoseDoubles * f;
        memcpy(q, b->DT + 12 * (size_t)f, 12 * sizeof(double));
        for (int k = 1; k < 5; ++k) memcpy(q + 12 + 16 * (k - 1), poses[k] + 16 * (size_t)f, 16 * sizeof(double));
    }
    T.fill(B.host(P.K.off1), B.host(P.K.off2), B.host(P.K.kind), B.host(P.K.kbase1), B.host(P.K.kbase2), B.host(P.K.cbase),
           descs, (size_t)b->desc_bytes, (uint8_t *)B.host(P.D.desc1), (uint8_t *)B.host(P.D.desc2));
    int32_t *gate_min = B.host(P.K.gate_min), *ws = B.host(P.D.ws);
    double *nnr = B.host(P.D.nnr), *sim_th = B.host(P.D.sim_th);
    float *fnnr = B.host(P.M.nnr);
    for (int p = 0; p < 2 * T.n; ++p) {
        const ProblemTable::Problem q = T.at(p);
        const int min_matches = q.kind ? prm.min_ls_matches : prm.min_pt_matches;
        gate_min[p] = (q.r2 > min_matches && q.r1 > min_matches) ? min_matches : INT32_MIN;  // :277-279, :424-426
        for (int e = 0; e < 4; ++e) ws[4 * p + e] = prm.ws;  // :269-272, :416-419
        nnr[p] = prm.min_ratio_12_p;  // matching.cpp:160, :241: for lines too
        sim_th[p] = prm.line_sim_th;
        fnnr[p] = (float)(q.kind ? prm.min_ratio_12_l : prm.min_ratio_12_p);  // :280, :427
    }
    // the rows of each kind keep the caller's order from the first pair's offset
    const size_t ap = (size_t)T.offs[0][0][0], al = (size_t)T.offs[1][0][0], cp = (size_t)T.offs[0][1][0], cl = (size_t)T.offs[1][1][0];
    if (T.cnt[0][0]) memcpy(B.host(P.K.q_pt), b->pt_P_p + 3 * ap, 3 * T.cnt[0][0] * sizeof(double));
    double *q = B.host(P.K.q_ls);
    for (size_t i = 0; i < T.cnt[1][0]; ++i, q += kKfQLsDoubles) {
        const size_t r = al + i;
        memcpy(q, b->ls_sP_p + 3 * r, 3 * sizeof(double));
        memcpy(q + 3, b->ls_eP_p + 3 * r, 3 * sizeof(double));
        memcpy(q + 6, b->ls_NDc_p + 6 * r, 6 * sizeof(double));
        memcpy(q + 12, b->ls_spl_p + 2 * r, 2 * sizeof(double));
        memcpy(q + 14, b->ls_epl_p + 2 * r, 2 * sizeof(double));
        memcpy(q + 16, b->ls_lm_NDw + 6 * r, 6 * sizeof(double));
    }
    if (T.cnt[1][0]) memcpy(B.host(P.K.ls_new), b->ls_new + al, T.cnt[1][0]);
    double *t = B.host(P.K.t_pt);
    for (size_t i = 0; i < T.cnt[0][1]; ++i, t += kKfTPtDoubles) {
        memcpy(t, b->pt_pl_c + 2 * (cp + i), 2 * sizeof(double));
        memcpy(t + 2, b->pt_P_c + 3 * (cp + i), 3 * sizeof(double));
    }
    t = B.host(P.K.t_ls);
    for (size_t i = 0; i < T.cnt[1][1]; ++i, t += kKfTLsDoubles) {
        memcpy(t, b->ls_spl_c + 2 * (cl + i), 2 * sizeof(double));
        memcpy(t + 2, b->ls_epl_c + 2 * (cl + i), 2 * sizeof(double));
    }
}

// the scalars of the three structs, the matchers' arrays handed over from K, and the launches
int kf_launch(CtxBase *ctx, KfPlan &P, int desc_bytes, const plba_kfassoc_params &prm) {
    KfDev &K = P.K;
    GmDev &D = P.D;
    DmDev &M = P.M;
    const int np = 2 * P.T.n, max_rows = P.T.max_rows;
    hipStream_t s = ctx->stream;
    K.gm12 = D.m12; K.gcount = D.count; K.fm12 = M.m12; K.fcount = M.count;
    K.inv_w = prm.cols / (double)prm.width;
    K.inv_h = prm.rows / (double)prm.height;
    K.stride = P.T.stride;
    K.prm = prm;
    grid_bind(D, K);
    M.off1 = K.off1; M.off2 = K.off2; M.desc1 = D.desc1; M.desc2 = D.desc2;
    M.n = np;
    M.dwords = desc_bytes / 4;
    M.best_lr = prm.best_lr != 0;
    M.gate_count = D.count;
    M.gate_min = K.gate_min;
    if (prm.fast_matching) {
        if (const int rc = grid_prepare(ctx, D, np, desc_bytes, prm.cols, prm.rows, prm.best_lr, P.key_bytes)) return rc;
        if (max_rows > 0) {  // a thread past its problem's rows does nothing
            hipLaunchKernelGGL(k_kf_cells, dim3(np, (max_rows + kKfNT - 1) / kKfNT), dim3(kKfNT), 0, s, K);
            PLBA_LAUNCHED(ctx, "k_kf_cells");
        }
        if (const int rc = grid_launch(ctx, D, P.T.max_train)) return rc;
    } else {  // the grid count is 0 (:249)
        PLBA_CHECK(hipMemsetAsync(D.count, 0, sizeof(int32_t) * np, s));
    }
    if (const int rc = desc_launch(ctx, M, max_rows)) return rc;  // a problem that keeps its grid matches is gated off
    hipLaunchKernelGGL(k_kf_geom, dim3(np, std::max(1, (P.T.max_prev + kKfNT - 1) / kKfNT)), dim3(kKfNT), 0, s, K);
    PLBA_LAUNCHED(ctx, "k_kf_geom");
    return PLBA_OK;
}

// every previous row's match and record, to the pair's previous offset in the caller's arrays
int kf_scatter(CtxBase *ctx, const KfPlan &P, const plba_kfassoc_out *out) {
    const Staged &B = P.B;
    const int32_t *res = B.host(P.K.res), *m12 = B.host(P.K.m12), *off1 = B.host(P.K.off1), *kbase1 = B.host(P.K.kbase1);
    const double *ptd = B.host(P.K.ptd), *lsd = B.host(P.K.lsd);
    const uint8_t *rej = B.host(P.K.rej);
    for (int p = 0; p < 2 * P.T.n; ++p) {
        const ProblemTable::Problem q = P.T.at(p);
        const int kd = q.kind, a1 = q.a1, r1 = q.r1;
        if (res[3 * p + 1] < 0 || res[3 * p + 1] > r1) {
            ctx->set_error("keyframe association: the device returned %d matches for %d rows", res[3 * p + 1], r1);
            return PLBA_E_DEVICE;
        }
        out->n_grid[p] = res[3 * p];
        out->n_matches[p] = res[3 * p + 1];
        out->fallback[p] = res[3 * p + 2];
        if (!r1) continue;
        int32_t *om = kd ? out->ls_m12 : out->pt_m12;
        if (om) memcpy(om + a1, m12 + off1[p], sizeof(int32_t) * r1);
        if (!kd) {
            if (out->pt_rec) memcpy(out->pt_rec + (size_t)kKfPtDoubles * a1, ptd + (size_t)kKfPtDoubles * kbase1[p], sizeof(double) * kKfPtDoubles * r1);
        } else {
            if (out->ls_rec) memcpy(out->ls_rec + (size_t)kKfLsDoubles * a1, lsd + (size_t)kKfLsDoubles * kbase1[p], sizeof(double) * kKfLsDoubles * r1);
            if (out->ls_rejected) memcpy(out->ls_rejected + a1, rej + kbase1[p], r1);
        }
    }
    return PLBA_OK;
}

}  // namespace

int kf_associate(CtxBase *ctx, const plba_kfassoc_batch *b, const plba_kfassoc_params *pp, const plba_kfassoc_out *out) {
    if (!b || b->n < 0) {
        ctx->set_error("keyframe association: NULL batch or n < 0");
        return PLBA_E_INVALID;
    }
    if (b->n == 0) return PLBA_OK;
    KfPlan P;
    if (const int rc = kf_validate(ctx, b, pp, out, P.T)) return rc;
    (void)hipSetDevice(ctx->opts.device);
    P.declare((size_t)b->desc_bytes / 4);
    if (const int rc = ctx->match.reserve(*ctx, P.B.total(), P.B.outputs_end(), "keyframe association")) return rc;
    P.B.stage(ctx->match.host, ctx->match.dev);
    kf_fill(P, b, *pp);
    if (const int rc = upload(ctx, ctx->match, P.B)) return rc;
    if (const int rc = kf_launch(ctx, P, b->desc_bytes, *pp)) return rc;
    if (const int rc = read_back(ctx, ctx->match, P.B)) return rc;
    return kf_scatter(ctx, P, out);
}

// ---------------------------------------------------------------- map-to-keyframe association
// MapHandler::matchMap2KFPoints / matchMap2KFLines (src/mapHandler.cpp:697-797, :799-921) up to the
// sequential part, for a batch of keyframes: one upload, k_map_cells, the grid matcher's three launches
// with the window (ws, ws, ws, ws), k_map_gate, the brute-force matcher's two, gated per problem on the
// device and blind to the invisible landmarks, k_map_geom (csrc/plba_mapassoc.hpp), one read-back.
// Keyframe f is the matcher's problems 2 f (points) and 2 f + 1 (lines).
namespace {

// everything that refuses the call, and the table; no device call
int map_validate(CtxBase *ctx, const plba_mapassoc_batch *b, const plba_mapassoc_params *pp, const plba_mapassoc_out *out,
                 ProblemTable &T) {
    const char *const op = "map association";
    const int n = b->n;
    if (n > (INT32_MAX - 1) / 2) {
        ctx->set_error("map association: %d keyframes", n);
        return PLBA_E_INVALID;
    }
    if (const int rc = check_desc_bytes(ctx, op, b->desc_bytes)) return rc;
    if (!pp || !out || !out->n_visible || !out->n_grid || !out->n_matches || !out->fallback || !out->n_accepted ||
        !b->pt_off_m || !b->pt_off_f || !b->ls_off_m || !b->ls_off_f || !b->Twf || !b->T_kf_w) {
        ctx->set_error("map association: NULL params / out / n_visible / n_grid / n_matches / fallback / n_accepted / offsets / poses");
        return PLBA_E_INVALID;
    }
    const plba_mapassoc_params &prm = *pp;
    if (prm.cols <= 0 || prm.rows <= 0 || prm.width <= 0 || prm.height <= 0 || prm.ws < 0 || prm.ws >= (1 << 30)) {
        ctx->set_error("map association: a grid of %d x %d cells, an image of %d x %d or a window of %d", prm.cols, prm.rows,
                       prm.width, prm.height, prm.ws);
        return PLBA_E_INVALID;
    }
    for (const int32_t *off : {b->pt_off_m, b->pt_off_f, b->ls_off_m, b->ls_off_f})
        if (const int rc = check_offsets(ctx, op, "row", "keyframe", off, n)) return rc;
    const int bad = T.init(b->pt_off_m, b->pt_off_f, b->ls_off_m, b->ls_off_f, n, prm.cols, prm.rows);
    if (bad == T.kTooMany) {
        ctx->set_error("map association: %zu candidate rows, %zu feature rows or %zu cells are more than %d", T.N1, T.N2, T.nc,
                       INT32_MAX);
        return PLBA_E_INVALID;
    }
    if ((T.cnt[0][0] && (!b->pt_X || !b->pdesc_m)) || (T.cnt[0][1] && (!b->pt_pl || !b->pt_P || !b->pdesc_f)) ||
        (T.cnt[1][0] && (!b->ls_X || !b->ldesc_m)) ||
        (T.cnt[1][1] && (!b->ls_spl || !b->ls_epl || !b->ls_le || !b->ls_sP || !b->ls_eP || !b->ldesc_f))) {
        ctx->set_error("map association: NULL landmark, feature or descriptor array");
        return PLBA_E_INVALID;
    }
    if (bad == T.kTooWide) {
        ctx->set_error("map association: %d feature rows in a problem are more than %d", T.max_train, kGmMaxTrain);
        return PLBA_E_INVALID;
    }
    if ((T.max_prev + kDmNT - 1) / kDmNT > 65535) {  // the row tiles are a grid's second dimension
        ctx->set_error("map association: %d candidate rows in a problem are more than %d", T.max_prev, 65535 * kDmNT);
        return PLBA_E_INVALID;
    }
    for (int k = 0; k < 2; ++k)
        for (size_t e = 0; e < (size_t)n * (k ? 16 : 12); ++e)
            if (!std::isfinite((k ? b->T_kf_w : b->Twf)[e])) {
                ctx->set_error("map association: %s of keyframe %zu is not finite", k ? "T_kf_w" : "Twf", e / (k ? 16 : 12));
                return PLBA_E_INVALID;
            }
    // the bound of a line feature's walk
    const double *const fcoords[3] = {b->pt_pl, b->ls_spl, b->ls_epl};
    for (int k = 0; k < 3; ++k) {
        const int kd = k ? 1 : 0;
        if (!T.cnt[kd][1]) continue;
        const double *c = fcoords[k] + 2 * (size_t)T.offs[kd][1][0];
        if (const int rc = check_coords<double, 2>(ctx, op, "feature", kd ? "line" : "point", c, T.cnt[kd][1], prm.width, prm.height))
            return rc;
    }
    return PLBA_OK;
}

// the inputs into the staged image: the poses keyframe by keyframe, the matchers' inputs problem by problem, the rows
void map_fill(const MaPlan &P, const plba_mapassoc_batch *b, const plba_mapassoc_params &prm) {
    const ProblemTable &T = P.T;
    const Staged &B = P.B;
    const uint8_t *const descs[2][2] = {{b->pdesc_m, b->pdesc_f}, {b->ldesc_m, b->ldesc_f}};
    double *pose = B.host(P.A.pose);
    for (int f = 0; f < T.n; ++f) {
        memcpy(pose + (size_t)kMaPoseDoubles * f, b->Twf + 12 * (size_t)f, 12 * sizeof(double));
        memcpy(pose + (size_t)kMaPoseDoubles * f + 12, b->T_kf_w + 16 * (size_t)f, 16 * sizeof(double));
    }
    T.fill(B.host(P.A.off1), B.host(P.A.off2), B.host(P.A.kind), B.host(P.A.kbase1), B.host(P.A.kbase2), B.host(P.A.cbase),
           descs, (size_t)b->desc_bytes, (uint8_t *)B.host(P.D.desc1), (uint8_t *)B.host(P.D.desc2));
    int32_t *min_matches = B.host(P.A.min_matches), *ws = B.host(P.D.ws);
    double *nnr = B.host(P.D.nnr), *sim_th = B.host(P.D.sim_th);
    float *fnnr = B.host(P.M.nnr);
    for (int p = 0; p < 2 * T.n; ++p) {
        const int kd = p % 2;
        min_matches[p] = kd ? prm.min_ls_matches : prm.min_pt_matches;
        for (int e = 0; e < 4; ++e) ws[4 * p + e] = prm.ws;  // :751-754, :866-869
        nnr[p] = prm.min_ratio_12_p;  // matching.cpp:160, :241: for lines too
        sim_th[p] = prm.line_sim_th;
        fnnr[p] = (float)(kd ? prm.min_ratio_12_l : prm.min_ratio_12_p);  // :762, :877
    }
    // the rows of each kind keep the caller's order from the first keyframe's offset
    const size_t mp = (size_t)T.offs[0][0][0], ml = (size_t)T.offs[1][0][0], fp = (size_t)T.offs[0][1][0], fl = (size_t)T.offs[1][1][0];
    if (T.cnt[0][0]) memcpy(B.host(P.A.q_pt), b->pt_X + 3 * mp, 3 * T.cnt[0][0] * sizeof(double));
    if (T.cnt[1][0]) memcpy(B.host(P.A.q_ls), b->ls_X + 6 * ml, 6 * T.cnt[1][0] * sizeof(double));
    double *t = B.host(P.A.t_pt);
    for (size_t i = 0; i < T.cnt[0][1]; ++i, t += kMaTPtDoubles) {
        memcpy(t, b->pt_pl + 2 * (fp + i), 2 * sizeof(double));
        memcpy(t + 2, b->pt_P + 3 * (fp + i), 3 * sizeof(double));
    }
    t = B.host(P.A.t_ls);
    for (size_t i = 0; i < T.cnt[1][1]; ++i, t += kMaTLsDoubles) {
        memcpy(t, b->ls_spl + 2 * (fl + i), 2 * sizeof(double));
        memcpy(t + 2, b->ls_epl + 2 * (fl + i), 2 * sizeof(double));
        memcpy(t + 4, b->ls_le + 3 * (fl + i), 3 * sizeof(double));
        memcpy(t + 7, b->ls_sP + 3 * (fl + i), 3 * sizeof(double));
        memcpy(t + 10, b->ls_eP + 3 * (fl + i), 3 * sizeof(double));
    }
}

// the scalars of the three structs, the matchers' arrays handed over from A, and the launches
int map_launch(CtxBase *ctx, MaPlan &P, int desc_bytes, const plba_mapassoc_params &prm) {
    MaDev &A = P.A;
    GmDev &D = P.D;
    DmDev &M = P.M;
    const int np = 2 * P.T.n, max_rows = P.T.max_rows;
    hipStream_t s = ctx->stream;
    A.gm12 = D.m12; A.gcount = D.count; A.fm12 = M.m12;
    A.inv_w = prm.cols / (double)prm.width;
    A.inv_h = prm.rows / (double)prm.height;
    A.stride = P.T.stride;
    A.prm = prm;
    grid_bind(D, A);
    M.off1 = A.off1; M.off2 = A.off2; M.desc1 = D.desc1; M.desc2 = D.desc2;
    M.n = np;
    M.dwords = desc_bytes / 4;
    M.best_lr = prm.best_lr != 0;
    M.gate_count = D.count;
    M.gate_min = A.gate_min;
    M.skip1 = A.skip;
    PLBA_CHECK(hipMemsetAsync(A.cnt, 0, sizeof(int32_t) * 2 * np, s));  // the two sums start at 0
    if (prm.fast_matching) {
        if (const int rc = grid_prepare(ctx, D, np, desc_bytes, prm.cols, prm.rows, prm.best_lr, P.key_bytes)) return rc;
    } else {  // the grid count is 0 (:739)
        PLBA_CHECK(hipMemsetAsync(D.count, 0, sizeof(int32_t) * np, s));
    }
    // a thread past its problem's rows only takes part in the count; with no row at all every count stays 0
    hipLaunchKernelGGL(k_map_cells, dim3(np, std::max(1, (max_rows + kMaNT - 1) / kMaNT)), dim3(kMaNT), 0, s, A);
    PLBA_LAUNCHED(ctx, "k_map_cells");
    if (prm.fast_matching)
        if (const int rc = grid_launch(ctx, D, P.T.max_train)) return rc;
    hipLaunchKernelGGL(k_map_gate, dim3((np + kMaNT - 1) / kMaNT), dim3(kMaNT), 0, s, A, np); PLBA_LAUNCHED(ctx, "k_map_gate");
    if (const int rc = desc_launch(ctx, M, max_rows)) return rc;  // a problem that keeps its grid matches is gated off
    hipLaunchKernelGGL(k_map_geom, dim3(np, std::max(1, (P.T.max_prev + kMaNT - 1) / kMaNT)), dim3(kMaNT), 0, s, A);
    PLBA_LAUNCHED(ctx, "k_map_geom");
    return PLBA_OK;
}

// every candidate row's flags, match and record, to the keyframe's candidate offset in the caller's arrays
int map_scatter(CtxBase *ctx, const MaPlan &P, const plba_mapassoc_out *out) {
    const Staged &B = P.B;
    const int32_t *cnt = B.host(P.A.cnt), *res = B.host(P.A.res), *m12 = B.host(P.A.m12), *off1 = B.host(P.A.off1),
                  *kbase1 = B.host(P.A.kbase1);
    const uint8_t *vis = B.host(P.A.vis), *acc = B.host(P.A.acc);
    const double *ptd = B.host(P.A.ptd), *lsd = B.host(P.A.lsd);
    for (int p = 0; p < 2 * P.T.n; ++p) {
        const ProblemTable::Problem q = P.T.at(p);
        const int kd = q.kind, a1 = q.a1, r1 = q.r1;
        if (cnt[2 * p] < 0 || cnt[2 * p] > r1 || cnt[2 * p + 1] < 0 || cnt[2 * p + 1] > cnt[2 * p]) {
            ctx->set_error("map association: the device returned %d visible and %d accepted rows for %d rows", cnt[2 * p],
                           cnt[2 * p + 1], r1);
            return PLBA_E_DEVICE;
        }
        out->n_visible[p] = cnt[2 * p];
        out->n_grid[p] = res[2 * p];
        out->fallback[p] = res[2 * p + 1];
        out->n_matches[p] = out->n_accepted[p] = cnt[2 * p + 1];  // :793, :917: the count after the epipolar test
        if (!r1) continue;
        int32_t *om = kd ? out->ls_m12 : out->pt_m12;
        uint8_t *ov = kd ? out->ls_visible : out->pt_visible, *oa = kd ? out->ls_accepted : out->pt_accepted;
        if (om) memcpy(om + a1, m12 + off1[p], sizeof(int32_t) * r1);
        if (ov) memcpy(ov + a1, vis + off1[p], r1);
        if (oa) memcpy(oa + a1, acc + off1[p], r1);
        if (!kd) {
            if (out->pt_rec) memcpy(out->pt_rec + (size_t)kMaPtDoubles * a1, ptd + (size_t)kMaPtDoubles * kbase1[p], sizeof(double) * kMaPtDoubles * r1);
        } else {
            if (out->ls_rec) memcpy(out->ls_rec + (size_t)kMaLsDoubles * a1, lsd + (size_t)kMaLsDoubles * kbase1[p], sizeof(double) * kMaLsDoubles * r1);
        }
    }
    return PLBA_OK;
}

}  // namespace

int map_associate(CtxBase *ctx, const plba_mapassoc_batch *b, const plba_mapassoc_params *pp, const plba_mapassoc_out *out) {
    if (!b || b->n < 0) {
        ctx->set_error("map association: NULL batch or n < 0");
        return PLBA_E_INVALID;
    }
    if (b->n == 0) return PLBA_OK;
    MaPlan P;
    if (const int rc = map_validate(ctx, b, pp, out, P.T)) return rc;
    (void)hipSetDevice(ctx->opts.device);
    P.declare((size_t)b->desc_bytes / 4);
    if (const int rc = ctx->match.reserve(*ctx, P.B.total(), P.B.outputs_end(), "map association")) return rc;
    P.B.stage(ctx->match.host, ctx->match.dev);
    map_fill(P, b, *pp);
    if (const int rc = upload(ctx, ctx->match, P.B)) return rc;
    if (const int rc = map_launch(ctx, P, b->desc_bytes, *pp)) return rc;
    if (const int rc = read_back(ctx, ctx->match, P.B)) return rc;
    return map_scatter(ctx, P, out);
}

// ---------------------------------------------------------------- median descriptor
// The descriptor half of updateAverageDescDir (src/mapFeatures.cpp:57-86) for a batch of descriptor
// lists: one upload, one launch of k_desc_medoid (csrc/plba_medoid.hpp), one read-back. The lists
// of at most kMedShort rows are packed four to a workgroup, every longer one has its own.
int desc_medoid(CtxBase *ctx, int n, const int32_t *list_ptr, const uint8_t *desc, int desc_bytes, int32_t *medoid) {
    const char *const op = "median descriptor";
    if (n < 0) {
        ctx->set_error("median descriptor: n < 0");
        return PLBA_E_INVALID;
    }
    if (n == 0) return PLBA_OK;
    if (const int rc = check_desc_bytes(ctx, op, desc_bytes)) return rc;
    if (!list_ptr || !medoid) {
        ctx->set_error("median descriptor: NULL list_ptr / medoid");
        return PLBA_E_INVALID;
    }
    int max_n = 0;
    if (const int rc = check_offsets(ctx, op, "row", "list", list_ptr, n, &max_n)) return rc;
    if (max_n > kMedMaxN) {  // the list sits in LDS whole
        ctx->set_error("median descriptor: a list of %d descriptors is more than %d", max_n, kMedMaxN);
        return PLBA_E_INVALID;
    }
    const size_t total = (size_t)list_ptr[n], dw = (size_t)desc_bytes / 4;
    if (total && !desc) {
        ctx->set_error("median descriptor: NULL desc");
        return PLBA_E_INVALID;
    }
    (void)hipSetDevice(ctx->opts.device);
    MedDev D{};
    Staged B;
    medoid_plan(B, D, (size_t)n, total, dw, list_ptr, desc, medoid);
    if (const int rc = ctx->match.reserve(*ctx, B.total(), B.outputs_end(), op)) return rc;
    B.stage(ctx->match.host, ctx->match.dev);
    int32_t *order = B.host(D.order);
    int n_short = 0;
    for (int k = 0; k < n; ++k)
        if (list_ptr[k + 1] - list_ptr[k] <= kMedShort) order[n_short++] = k;
    int n_long = 0;
    for (int k = 0; k < n; ++k)
        if (list_ptr[k + 1] - list_ptr[k] > kMedShort) order[n_short + n_long++] = k;
    if (const int rc = upload(ctx, ctx->match, B)) return rc;
    D.n = n;
    D.dwords = desc_bytes / 4;
    D.n_short = n_short;
    D.n_short_wg = (n_short + kMedWaves - 1) / kMedWaves;
    const dim3 grid(D.n_short_wg + n_long);
    const int W = D.dwords <= 8 ? 8 : 16;
    const size_t lds = sizeof(uint32_t) * W * (size_t)std::max(kMedWaves * kMedShort, max_n);  // at most 64 KiB
    if (W == 8) hipLaunchKernelGGL(k_desc_medoid<8>, grid, dim3(kMedNT), lds, ctx->stream, D);
    else hipLaunchKernelGGL(k_desc_medoid<16>, grid, dim3(kMedNT), lds, ctx->stream, D);
    PLBA_LAUNCHED(ctx, "k_desc_medoid");
    if (const int rc = read_back(ctx, ctx->match, B)) return rc;
    B.fetch();
    return PLBA_OK;
}

// ---------------------------------------------------------------- place recognition
// DBoW2's transform and L1 score as insertKFBowVectorP / L / PL use them (src/mapHandler.cpp:
// 4118-4239); the kernels and the arithmetic are in csrc/plba_bow.hpp.
namespace {

BowSlot *bow_slot(CtxBase *ctx, const char *op, int slot, bool need_vocab) {
    if (slot != 0 && slot != 1) {
        ctx->set_error("%s: slot %d is neither 0 (points) nor 1 (lines)", op, slot);
        return nullptr;
    }
    if (need_vocab && ctx->bow[slot].n_nodes == 0) {
        ctx->set_error("%s: slot %d has no vocabulary", op, slot);
        return nullptr;
    }
    return &ctx->bow[slot];
}

// A database array that keeps its contents when it grows (ScratchBlock::reserve does not): at
// least doubled, the used part copied on the stream.
int bow_grow(CtxBase *ctx, ScratchBlock &b, size_t need, size_t used) {
    if (need <= b.dev_cap) return PLBA_OK;
    const size_t cap = std::max(need, 2 * b.dev_cap);
    char *nd = nullptr;
    if (hipMallocAsync((void **)&nd, cap, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        ctx->set_error("place recognition: cannot allocate %zu bytes for the database", cap);
        return PLBA_E_NOMEM;
    }
    if (used) {
        const hipError_t e = hipMemcpyAsync(nd, b.dev, used, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFreeAsync(nd, ctx->stream);  // the old array stays
            ctx->set_error("place recognition: HIP error %s while the database grew", hipGetErrorString(e));
            return PLBA_E_DEVICE;
        }
    }
    b.release(ctx->stream);
    b.dev = nd;
    b.dev_cap = cap;
    return PLBA_OK;
}

std::vector<BowSlot::Row>::iterator bow_find(BowSlot &S, int kf_id) {
    return std::lower_bound(S.rows.begin(), S.rows.end(), kf_id,
                            [](const BowSlot::Row &r, int id) { return r.kf_id < id; });
}

}  // namespace

int bow_set_vocab(CtxBase *ctx, int slot, const plba_bow_vocab *v) {
    const char *const op = "vocabulary";
    BowSlot *S = bow_slot(ctx, op, slot, false);
    if (!S) return PLBA_E_INVALID;
    if (!v || !v->child_off || !v->children || !v->node_desc || !v->word_id || !v->weight) {
        ctx->set_error("vocabulary: NULL vocabulary or array");
        return PLBA_E_INVALID;
    }
    if (const int rc = check_desc_bytes(ctx, op, v->desc_bytes)) return rc;
    const int nn = v->n_nodes;
    if (nn < 2 || v->n_words < 1 || v->n_words > nn) {
        ctx->set_error("vocabulary: %d nodes and %d words", nn, v->n_words);
        return PLBA_E_INVALID;
    }
    if (v->child_off[0] != 0) {
        ctx->set_error("vocabulary: the child offsets do not start at 0");
        return PLBA_E_INVALID;
    }
    int max_children = 0;
    if (const int rc = check_offsets(ctx, op, "child", "node", v->child_off, nn, &max_children)) return rc;
    if (v->child_off[nn] != nn - 1 || v->child_off[1] == 0) {
        // a tree in which every node but the root is reached once has n_nodes - 1 child entries
        ctx->set_error("vocabulary: %d child entries for %d nodes, or a root without children", v->child_off[nn], nn);
        return PLBA_E_INVALID;
    }
    // breadth first from the root: every child index in range, every node reached exactly once
    std::vector<int32_t> level(nn, -1), queue{0};
    queue.reserve(nn);
    level[0] = 0;
    int depth = 0;
    for (size_t head = 0; head < queue.size(); ++head) {
        const int node = queue[head];
        for (int e = v->child_off[node]; e < v->child_off[node + 1]; ++e) {
            const int c = v->children[e];
            if (c <= 0 || c >= nn) {
                ctx->set_error("vocabulary: child %d of node %d is outside 1 .. %d", c, node, nn - 1);
                return PLBA_E_INVALID;
            }
            if (level[c] >= 0) {
                ctx->set_error("vocabulary: node %d is reached twice", c);
                return PLBA_E_INVALID;
            }
            level[c] = level[node] + 1;
            depth = std::max(depth, level[c]);
            queue.push_back(c);
        }
    }
    if ((int)queue.size() != nn) {
        ctx->set_error("vocabulary: %d of %d nodes are not reached from the root", nn - (int)queue.size(), nn);
        return PLBA_E_INVALID;
    }
    std::vector<double> word_weight(v->n_words, 0.0);
    std::vector<uint8_t> word_seen(v->n_words, 0);
    for (int i = 0; i < nn; ++i) {
        if (!std::isfinite(v->weight[i])) {
            ctx->set_error("vocabulary: the weight of node %d is not finite", i);
            return PLBA_E_INVALID;
        }
        const int w = v->word_id[i];
        if (v->child_off[i + 1] > v->child_off[i]) {
            if (w >= 0) {
                ctx->set_error("vocabulary: inner node %d has word id %d", i, w);
                return PLBA_E_INVALID;
            }
            continue;
        }
        if (w < 0 || w >= v->n_words || word_seen[w]) {
            ctx->set_error("vocabulary: leaf %d has word id %d, outside 0 .. %d or used twice", i, w, v->n_words - 1);
            return PLBA_E_INVALID;
        }
        word_seen[w] = 1;
        word_weight[w] = v->weight[i];
    }
    (void)hipSetDevice(ctx->opts.device);
    const size_t db = (size_t)v->desc_bytes;
    S->n_nodes = 0;  // the slot is empty until the upload is through
    S->rows.clear();
    S->used = 0;
    int32_t *child_off, *children, *word_id;
    uint32_t *node_desc;
    double *weight;
    Staged B;  // for the offsets alone: no host image, five copies from the caller's arrays
    B.dev(child_off, nn + 1);
    B.dev(children, nn - 1);
    B.dev(node_desc, db / 4 * nn);
    B.dev(word_id, nn);
    B.dev(weight, v->n_words);
    if (const int rc = S->voc.reserve(*ctx, B.total(), 0, op)) return rc;
    B.stage(nullptr, S->voc.dev);
    hipStream_t s = ctx->stream;
    PLBA_CHECK(hipMemcpyAsync(child_off, v->child_off, sizeof(int32_t) * (nn + 1), hipMemcpyHostToDevice, s));
    PLBA_CHECK(hipMemcpyAsync(children, v->children, sizeof(int32_t) * (nn - 1), hipMemcpyHostToDevice, s));
    PLBA_CHECK(hipMemcpyAsync(node_desc, v->node_desc, db * nn, hipMemcpyHostToDevice, s));
    PLBA_CHECK(hipMemcpyAsync(word_id, v->word_id, sizeof(int32_t) * nn, hipMemcpyHostToDevice, s));
    PLBA_CHECK(hipMemcpyAsync(weight, word_weight.data(), sizeof(double) * v->n_words, hipMemcpyHostToDevice, s));
    PLBA_CHECK(hipStreamSynchronize(s));  // the caller's arrays and word_weight are free again
    S->child_off = child_off; S->children = children; S->node_desc = node_desc; S->word_id = word_id; S->word_weight = weight;
    S->n_words = v->n_words;
    S->dwords = v->desc_bytes / 4;
    S->depth = depth;
    S->max_children = max_children;
    S->n_nodes = nn;
    return PLBA_OK;
}

int bow_insert(CtxBase *ctx, int slot, int kf_id, const uint8_t *desc, int n_desc, double *scores, int32_t *ids, int cap,
               int32_t *n_out) {
    const char *const op = "place recognition";
    BowSlot *S = bow_slot(ctx, op, slot, true);
    if (!S) return PLBA_E_INVALID;
    if (kf_id < 0 || n_desc < 0 || n_desc > kBowMaxDesc || cap < 0 || !n_out) {
        ctx->set_error("place recognition: kf_id %d, %d descriptors (at most %d), cap %d or n == NULL", kf_id, n_desc,
                       kBowMaxDesc, cap);
        return PLBA_E_INVALID;
    }
    if ((n_desc && !desc) || (cap && (!scores || !ids))) {
        ctx->set_error("place recognition: NULL desc / scores / ids");
        return PLBA_E_INVALID;
    }
    auto pos = bow_find(*S, kf_id);
    if (pos != S->rows.end() && pos->kf_id == kf_id) {
        ctx->set_error("place recognition: keyframe %d is already in slot %d", kf_id, slot);
        return PLBA_E_INVALID;
    }
    if (S->used + (size_t)n_desc > (size_t)INT32_MAX) {
        ctx->set_error("place recognition: the database of slot %d is full", slot);
        return PLBA_E_NOMEM;
    }
    (void)hipSetDevice(ctx->opts.device);
    int n_live = 0;
    for (const BowSlot::Row &r : S->rows) n_live += r.live;
    int npad = 1;
    while (npad < n_desc) npad <<= 1;
    BowDev D{};
    Staged B;
    B.in(D.desc, (size_t)S->dwords * n_desc, desc);
    B.in(D.ent, 2 * (size_t)n_live);  // filled below
    B.out(D.scores, (size_t)n_live + 1);  // delivered below, up to the caller's cap
    B.out(D.n_new, 1);
    B.dev(D.keys, n_desc);
    B.dev(D.sortbuf, npad > kBowLdsKeys ? npad : 0);
    B.dev(D.run_start, n_desc);
    if (const int rc = ctx->bow_io.reserve(*ctx, B.total(), B.outputs_end(), op)) return rc;
    // the new row has at most n_desc words
    if (const int rc = bow_grow(ctx, S->db_word, sizeof(int32_t) * (S->used + n_desc + 32), sizeof(int32_t) * S->used))
        return rc;
    if (const int rc = bow_grow(ctx, S->db_val, sizeof(double) * (S->used + n_desc + 32), sizeof(double) * S->used))
        return rc;
    B.stage(ctx->bow_io.host, ctx->bow_io.dev);
    int32_t *ent = B.host(D.ent);
    int j = 0;
    for (const BowSlot::Row &r : S->rows) {
        if (!r.live) continue;
        ent[2 * j] = r.off;
        ent[2 * j + 1] = r.len;
        if (j < cap) ids[j] = r.kf_id;
        ++j;
    }
    if (const int rc = upload(ctx, ctx->bow_io, B)) return rc;
    hipStream_t s = ctx->stream;
    D.child_off = S->child_off;
    D.children = S->children;
    D.node_desc = S->node_desc;
    D.word_id = S->word_id;
    D.word_weight = S->word_weight;
    D.dwords = S->dwords;
    D.depth = S->depth;
    D.max_children = S->max_children;
    D.n_desc = n_desc;
    D.npad = npad;
    D.db_word = reinterpret_cast<int32_t *>(S->db_word.dev);
    D.db_val = reinterpret_cast<double *>(S->db_val.dev);
    D.new_off = (int32_t)S->used;
    D.n_live = n_live;
    constexpr int per_wg = kBowDescNT / kBowGroup, waves_per_wg = kBowScoreNT / 64;
    hipLaunchKernelGGL(k_bow_descend, dim3(std::max(1, (n_desc + per_wg - 1) / per_wg)), dim3(kBowDescNT), 0, s, D);
    PLBA_LAUNCHED(ctx, "k_bow_descend");
    hipLaunchKernelGGL(k_bow_vector, dim3(1), dim3(kBowVecNT), 0, s, D); PLBA_LAUNCHED(ctx, "k_bow_vector");
    hipLaunchKernelGGL(k_bow_score, dim3((n_live + 1 + waves_per_wg - 1) / waves_per_wg), dim3(kBowScoreNT), 0, s, D);
    PLBA_LAUNCHED(ctx, "k_bow_score");
    if (const int rc = read_back(ctx, ctx->bow_io, B)) return rc;
    const int32_t len = *B.host(D.n_new);
    if (len < 0 || len > n_desc) {
        ctx->set_error("place recognition: the device returned a vector of %d words for %d descriptors", len, n_desc);
        return PLBA_E_DEVICE;
    }
    S->rows.insert(bow_find(*S, kf_id), BowSlot::Row{kf_id, (int32_t)S->used, len, true});
    S->used += (size_t)len;
    const double *sc = B.host(D.scores);
    for (int k = 0; k < std::min(cap, n_live); ++k) scores[k] = sc[k];
    if (n_live < cap) {
        scores[n_live] = sc[n_live];
        ids[n_live] = kf_id;
    }
    *n_out = n_live + 1;
    return PLBA_OK;
}

int bow_remove(CtxBase *ctx, int slot, int kf_id) {
    BowSlot *S = bow_slot(ctx, "place recognition", slot, false);
    if (!S) return PLBA_E_INVALID;
    auto pos = bow_find(*S, kf_id);
    if (pos == S->rows.end() || pos->kf_id != kf_id || !pos->live) {
        ctx->set_error("place recognition: slot %d has no live vector of keyframe %d", slot, kf_id);
        return PLBA_E_INVALID;
    }
    pos->live = false;
    return PLBA_OK;
}

int bow_get(CtxBase *ctx, int slot, int kf_id, int32_t *word_ids, double *values, int cap, int32_t *n_out) {
    BowSlot *S = bow_slot(ctx, "place recognition", slot, false);
    if (!S) return PLBA_E_INVALID;
    auto pos = bow_find(*S, kf_id);
    if (pos == S->rows.end() || pos->kf_id != kf_id || !pos->live) {
        ctx->set_error("place recognition: slot %d has no live vector of keyframe %d", slot, kf_id);
        return PLBA_E_INVALID;
    }
    if (cap < 0 || !n_out || (cap && (!word_ids || !values))) {
        ctx->set_error("place recognition: cap %d, NULL word_ids / values / n", cap);
        return PLBA_E_INVALID;
    }
    *n_out = pos->len;
    const size_t cnt = (size_t)std::min(cap, pos->len);
    if (cnt) {
        (void)hipSetDevice(ctx->opts.device);
        hipStream_t s = ctx->stream;
        PLBA_CHECK(hipMemcpyAsync(word_ids, S->db_word.dev + sizeof(int32_t) * (size_t)pos->off, sizeof(int32_t) * cnt,
                                  hipMemcpyDeviceToHost, s));
        PLBA_CHECK(hipMemcpyAsync(values, S->db_val.dev + sizeof(double) * (size_t)pos->off, sizeof(double) * cnt,
                                  hipMemcpyDeviceToHost, s));
        PLBA_CHECK(hipStreamSynchronize(s));
    }
    return PLBA_OK;
}

}  // namespace plba
