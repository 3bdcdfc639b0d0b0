// trackFramesCpu: a single-threaded restatement of plba_track_frames' semantics (include/plba.h;
// StereoFrameHandler::f2fTracking + optimizePose, src2/stereoFrameHandler.cpp:106-180, :307-405) with its
// signature, for the tests and tools/trackframes_bench.py (not a product path). It is composed of the two
// restatements it stands between: descMatchCpu per pair and kind, the scatter loop of :144-152 / :167-179
// as it is written there, and trackPoseCpu on the rows it pushed. No arithmetic of its own.
#include <vector>

#include "plslam_map.hpp"

namespace plslam {

int trackFramesCpu(const plba_frames_batch *b, const plba_frames_params *pp, const plba_frames_out *out) {
    if (!b || b->n < 0) return PLBA_E_INVALID;
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    plba_frames_params prm;
    if (pp) prm = *pp;
    else plba_frames_default_params(&prm);
    const plba_track_params &tp = prm.track;
    // what plba_track_frames refuses is refused here
    if (prm.desc_bytes < 4 || prm.desc_bytes > 64 || prm.desc_bytes % 4) return PLBA_E_INVALID;
    if (!out || !out->out || !out->n_pt || !out->n_ln || !b->pt_off1 || !b->pt_off2 || !b->ln_off1 || !b->ln_off2)
        return PLBA_E_INVALID;
    if ((tp.line_model != PLBA_TRACK_PLUCKER && tp.line_model != PLBA_TRACK_ENDPOINTS) || tp.max_iters < 1 || tp.max_iters_ref < 1)
        return PLBA_E_INVALID;
    const bool pluker = tp.line_model == PLBA_TRACK_PLUCKER;
    const int32_t *const offs[4] = {b->pt_off1, b->ln_off1, b->pt_off2, b->ln_off2};
    for (int a = 0; a < 4; ++a) {
        if (offs[a][0] != 0) return PLBA_E_INVALID;
        for (int k = 0; k < n; ++k)
            if (offs[a][k + 1] < offs[a][k] || (a < 2 && offs[a][k + 1] - offs[a][k] > PLBA_TRACK_MAX_N)) return PLBA_E_INVALID;
    }
    const size_t p1 = (size_t)b->pt_off1[n], p2 = (size_t)b->pt_off2[n], l1 = (size_t)b->ln_off1[n], l2 = (size_t)b->ln_off2[n];
    if ((p1 && (!b->prev_pdesc || !b->prev_pt_P || !b->prev_pt_sigma2 || !out->pt_m12)) ||
        (p2 && (!b->cur_pdesc || !b->cur_pt_pl || !out->pt_cur_from_prev)) ||
        (l1 && (!b->prev_ldesc || !b->prev_ln_sP || !b->prev_ln_eP || !b->prev_ln_seg || !b->prev_ln_sigma2 || !out->ln_m12 ||
                (pluker && !b->prev_ln_NDc))) ||
        (l2 && (!b->cur_ldesc || !out->ln_cur_from_prev || (pluker ? !b->cur_ln_seg : !b->cur_ln_le))))
        return PLBA_E_INVALID;
    if (tp.use_motion_model && !b->prev) return PLBA_E_INVALID;

    // match(prev desc, curr desc) of every pair, points then lines (:141, :164); a kind that is switched off
    // has no match (:137, :160)
    auto match = [&](const int32_t *off1, const int32_t *off2, const uint8_t *d1, const uint8_t *d2, float nnr, bool on,
                     int32_t *m12) {
        std::vector<int32_t> cnt((size_t)n);
        std::vector<float> ratio((size_t)n, nnr);
        plba_match_batch mb{};
        mb.n = n, mb.desc_bytes = prm.desc_bytes, mb.off1 = off1, mb.off2 = off2, mb.desc1 = d1, mb.desc2 = d2;
        mb.nnr = ratio.data(), mb.best_lr = prm.best_lr;
        if (on && off1[n]) return descMatchCpu(&mb, m12, cnt.data());
        for (int i = 0; i < off1[n]; ++i) m12[i] = -1;
        return (int)PLBA_OK;
    };
    if (const int rc = match(b->pt_off1, b->pt_off2, b->prev_pdesc, b->cur_pdesc, prm.nnr_pt, tp.has_points != 0, out->pt_m12)) return rc;
    if (const int rc = match(b->ln_off1, b->ln_off2, b->prev_ldesc, b->cur_ldesc, prm.nnr_ln, tp.has_lines != 0, out->ln_m12)) return rc;

    // the loops around matches_12 (:144-152, :167-179): push_back in increasing i1, the last writer of idx
    std::vector<int32_t> pt_off((size_t)n + 1, 0), ln_off((size_t)n + 1, 0), pt_src, ln_src;
    std::vector<double> pt_P, pt_obs, pt_s2, ln_sP, ln_eP, ln_ND, ln_le, ln_obs, ln_seg, ln_s2;
    auto push = [](std::vector<double> &v, const double *src, size_t row, int w) { v.insert(v.end(), src + w * row, src + w * (row + 1)); };
    for (size_t i = 0; i < p2; ++i) out->pt_cur_from_prev[i] = -1;
    for (size_t i = 0; i < l2; ++i) out->ln_cur_from_prev[i] = -1;
    for (int k = 0; k < n; ++k) {
        for (int i1 = 0; i1 < b->pt_off1[k + 1] - b->pt_off1[k]; ++i1) {
            const size_t a = (size_t)(b->pt_off1[k] + i1);
            const int i2 = out->pt_m12[a];
            if (i2 < 0) continue;
            const size_t c = (size_t)(b->pt_off2[k] + i2);
            push(pt_P, b->prev_pt_P, a, 3), push(pt_obs, b->cur_pt_pl, c, 2), push(pt_s2, b->prev_pt_sigma2, a, 1);
            pt_src.push_back((int32_t)a);
            out->pt_cur_from_prev[c] = i1;
        }
        for (int i1 = 0; i1 < b->ln_off1[k + 1] - b->ln_off1[k]; ++i1) {
            const size_t a = (size_t)(b->ln_off1[k] + i1);
            const int i2 = out->ln_m12[a];
            if (i2 < 0) continue;
            const size_t c = (size_t)(b->ln_off2[k] + i2);
            push(ln_sP, b->prev_ln_sP, a, 3), push(ln_eP, b->prev_ln_eP, a, 3), push(ln_seg, b->prev_ln_seg, a, 4);
            push(ln_s2, b->prev_ln_sigma2, a, 1);
            if (pluker) push(ln_ND, b->prev_ln_NDc, a, 6), push(ln_obs, b->cur_ln_seg, c, 4);
            else push(ln_le, b->cur_ln_le, c, 3);
            ln_src.push_back((int32_t)a);
            out->ln_cur_from_prev[c] = i1;
        }
        pt_off[k + 1] = (int32_t)pt_src.size(), ln_off[k + 1] = (int32_t)ln_src.size();
        out->n_pt[k] = pt_off[k + 1] - pt_off[k], out->n_ln[k] = ln_off[k + 1] - ln_off[k];
    }

    // optimizePose on the rows pushed, and its inlier flags back to the previous rows
    plba_track_batch tb{};
    tb.n = n, tb.pt_off = pt_off.data(), tb.ln_off = ln_off.data();
    tb.pt_P = pt_P.data(), tb.pt_obs = pt_obs.data(), tb.pt_sigma2 = pt_s2.data();
    tb.ln_sP = ln_sP.data(), tb.ln_eP = ln_eP.data(), tb.ln_NDc = ln_ND.data(), tb.ln_le = ln_le.data();
    tb.ln_obs = ln_obs.data(), tb.ln_seg = ln_seg.data(), tb.ln_sigma2 = ln_s2.data();
    tb.prev = b->prev, tb.fx = b->fx, tb.fy = b->fy, tb.cx = b->cx, tb.cy = b->cy;
    // (an empty vector's data() may be NULL, which trackPoseCpu refuses only for a kind that has rows)
    std::vector<uint8_t> pin(pt_src.size() + 1), lin(ln_src.size() + 1);
    if (const int rc = trackPoseCpu(&tb, &tp, out->out, pin.data(), lin.data())) return rc;
    if (out->pt_inlier) {
        for (size_t i = 0; i < p1; ++i) out->pt_inlier[i] = 0;
        for (size_t r = 0; r < pt_src.size(); ++r) out->pt_inlier[pt_src[r]] = pin[r];
    }
    if (out->ln_inlier) {
        for (size_t i = 0; i < l1; ++i) out->ln_inlier[i] = 0;
        for (size_t r = 0; r < ln_src.size(); ++r) out->ln_inlier[ln_src[r]] = lin[r];
    }
    return PLBA_OK;
}

}  // namespace plslam
