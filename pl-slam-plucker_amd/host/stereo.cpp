// The stereo front end that makes a keyframe's features, StereoFrame::matchStereoPoints / matchStereoLines
// (src2/stereoFrame.cpp:121-174, :310-435): MapHandler::setKeyframeStereo, which runs plba_stereo_associate
// (or the hook) on one frame's detector output and stores the result as the keyframe's features; and
// stereoCpu, a single-threaded restatement of that call's semantics (include/plba.h) with the hook's
// signature, for the tests and tools/stereo_bench.py (not a product path). The arithmetic is that of
// csrc/plba_stereo_geom.hpp; this file is compiled without contraction.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "../csrc/plba_stereo_geom.hpp"
#include "plslam_map.hpp"

namespace plslam {

int stereoCpu(const plba_stereo_batch *b, const plba_stereo_params *pp, const plba_stereo_out *out) {
    using namespace plba;
    if (!b || b->n < 0) return PLBA_E_INVALID;
    const int n = b->n;
    if (n == 0) return PLBA_OK;
    // what plba_stereo_associate refuses is refused here
    if (b->desc_bytes < 4 || b->desc_bytes > 64 || b->desc_bytes % 4) return PLBA_E_INVALID;
    if (!pp || !out || !out->n_pt || !out->n_ls || !b->pt_off_l || !b->pt_off_r || !b->ls_off_l || !b->ls_off_r)
        return PLBA_E_INVALID;
    const plba_stereo_params &prm = *pp;
    if (prm.cols <= 0 || prm.rows <= 0 || prm.width <= 0 || prm.height <= 0 || prm.matching_s_ws < 0) return PLBA_E_INVALID;
    const int32_t *const offs[2][2] = {{b->pt_off_l, b->pt_off_r}, {b->ls_off_l, b->ls_off_r}};
    const float *const coords[2][2] = {{b->pt_l, b->pt_r}, {b->ls_l, b->ls_r}};
    const uint8_t *const descs[2][2] = {{b->pdesc_l, b->pdesc_r}, {b->ldesc_l, b->ldesc_r}};
    for (int kd = 0; kd < 2; ++kd)
        for (int sd = 0; sd < 2; ++sd) {
            const int32_t *off = offs[kd][sd];
            if (off[0] < 0) return PLBA_E_INVALID;
            for (int f = 0; f < n; ++f)
                if (off[f + 1] < off[f] || (sd && off[f + 1] - off[f] > 65535)) return PLBA_E_INVALID;
            const size_t rows = (size_t)(off[n] - off[0]), per = kd ? 4 : 2;
            if (!rows) continue;
            if (!coords[kd][sd] || !descs[kd][sd]) return PLBA_E_INVALID;
            const float *c = coords[kd][sd] + per * off[0];
            for (size_t e = 0; e < rows * per; ++e) {
                const double v = c[e], size = (e & 1) ? prm.height : prm.width;
                if (!(v >= -size && v <= 2.0 * size)) return PLBA_E_INVALID;
            }
        }
    const int db = b->desc_bytes, stride = std::max(prm.cols, prm.rows), max_steps = st_max_steps(prm.cols, prm.rows);
    const double inv_w = prm.cols / (double)prm.width, inv_h = prm.rows / (double)prm.height;  // :47-48
    std::vector<int32_t> cell1, cell1e, cell_off2, cells2, m12, line(2 * (size_t)stride);
    std::vector<double> dir2;
    for (int f = 0; f < n; ++f)
        for (int kd = 0; kd < 2; ++kd) {
            const int per = kd ? 4 : 2;
            const int a1 = offs[kd][0][f], n1 = offs[kd][0][f + 1] - a1, a2 = offs[kd][1][f], n2 = offs[kd][1][f + 1] - a2;
            const float *cl = coords[kd][0] ? coords[kd][0] + (size_t)per * a1 : nullptr,
                        *cr = coords[kd][1] ? coords[kd][1] + (size_t)per * a2 : nullptr;
            cell1.assign(2 * (size_t)n1, 0);
            cell1e.assign(2 * (size_t)n1, 0);
            for (int i = 0; i < n1; ++i) {  // :130-133, :319-323
                cell1[2 * i] = st_cell(cl[per * i], inv_w);
                cell1[2 * i + 1] = st_cell(cl[per * i + 1], inv_h);
                if (kd) {
                    cell1e[2 * i] = st_cell(cl[4 * i + 2], inv_w);
                    cell1e[2 * i + 1] = st_cell(cl[4 * i + 3], inv_h);
                }
            }
            cell_off2.assign(1, 0);
            cells2.clear();
            dir2.assign(2 * (size_t)n2, 0.0);
            for (int i = 0; i < n2; ++i) {  // :137-140, :329-339
                const float *c = cr + per * i;
                if (kd) {
                    st_line_dir(c, inv_w, inv_h, &dir2[2 * (size_t)i]);
                    const int k = st_line_cells((double)c[0] * inv_w, (double)c[1] * inv_h, (double)c[2] * inv_w,
                                                (double)c[3] * inv_h, prm.cols, prm.rows, max_steps, line.data(), stride);
                    cells2.insert(cells2.end(), line.begin(), line.begin() + 2 * k);
                } else {
                    cells2.insert(cells2.end(), {st_cell(c[0], inv_w), st_cell(c[1], inv_h)});
                }
                cell_off2.push_back((int32_t)(cells2.size() / 2));
            }
            m12.assign((size_t)n1 + 1, -1);
            int32_t matches = 0;
            const int32_t off1[2] = {0, n1}, off2[2] = {0, n2}, kind = kd;
            const int32_t win[4] = {prm.matching_s_ws, 0, 0, 0};  // :142-144
            plba_gridmatch_batch g{};
            g.n = 1; g.desc_bytes = db; g.cols = prm.cols; g.rows = prm.rows; g.best_lr = prm.best_lr ? 1 : 0;
            g.off1 = off1; g.off2 = off2;
            g.desc1 = descs[kd][0] ? descs[kd][0] + (size_t)db * a1 : nullptr;
            g.desc2 = descs[kd][1] ? descs[kd][1] + (size_t)db * a2 : nullptr;
            g.cell1 = cell1.data(); g.cell1_end = cell1e.data(); g.cell_off2 = cell_off2.data(); g.cells2 = cells2.data();
            g.dir2 = dir2.data(); g.kind = &kind; g.nnr = &prm.min_ratio_12_p; g.line_sim_th = &prm.line_sim_th;
            if (n1 && n2)  // :127, :316
                if (const int rc = gridMatchCpuWin(&g, win, m12.data(), &matches)) return rc;
            int k = 0;
            for (int i1 = 0; i1 < n1; ++i1) {  // :153-171, :352-432
                const int i2 = m12[i1];
                if (i2 < 0) continue;
                double rec[kStLsDoubles];
                const size_t o = (size_t)a1 + k;
                if (!kd) {
                    if (st_point(prm, cl + 2 * i1, cr + 2 * i2, rec)) continue;
                    if (out->pt_pl) std::copy(rec, rec + 2, out->pt_pl + 2 * o);
                    if (out->pt_disp) out->pt_disp[o] = rec[2];
                    if (out->pt_P) std::copy(rec + 3, rec + 6, out->pt_P + 3 * o);
                    if (out->pt_src) out->pt_src[o] = i1;
                    if (out->pdesc) std::memcpy(out->pdesc + (size_t)db * o, g.desc1 + (size_t)db * i1, db);
                } else {
                    if (st_line(prm, cl + 4 * i1, cr + 4 * i2, rec)) continue;
                    if (out->ls_spl) std::copy(rec, rec + 2, out->ls_spl + 2 * o);
                    if (out->ls_epl) std::copy(rec + 2, rec + 4, out->ls_epl + 2 * o);
                    if (out->ls_sdisp) out->ls_sdisp[o] = rec[4];
                    if (out->ls_edisp) out->ls_edisp[o] = rec[5];
                    if (out->ls_sP) std::copy(rec + 6, rec + 9, out->ls_sP + 3 * o);
                    if (out->ls_eP) std::copy(rec + 9, rec + 12, out->ls_eP + 3 * o);
                    if (out->ls_le) std::copy(rec + 12, rec + 15, out->ls_le + 3 * o);
                    if (out->ls_NDc && prm.pluker) std::copy(rec + 15, rec + 21, out->ls_NDc + 6 * o);
                    if (out->ls_src) out->ls_src[o] = i1;
                    if (out->ldesc) std::memcpy(out->ldesc + (size_t)db * o, g.desc1 + (size_t)db * i1, db);
                }
                ++k;
            }
            (kd ? out->n_ls : out->n_pt)[f] = k;
        }
    return PLBA_OK;
}

int MapHandler::setKeyframeStereo(int kf_idx, const StereoInput &in, const plba_stereo_params &prm, int32_t *pt_src,
                                  int32_t *ls_src, StereoStats *stats) {
    if (kf_idx < 0 || kf_idx >= (int)map_keyframes.size() || !map_keyframes[kf_idx]) {
        setError("setKeyframeStereo: no keyframe %d", kf_idx);
        return PLBA_E_INVALID;
    }
    if (in.n_pt_l < 0 || in.n_pt_r < 0 || in.n_ls_l < 0 || in.n_ls_r < 0 || in.desc_bytes < 4 || in.desc_bytes > 64 ||
        in.desc_bytes % 4) {
        setError("setKeyframeStereo: a negative row count or desc_bytes %d", in.desc_bytes);
        return PLBA_E_INVALID;
    }
    const size_t npl = (size_t)in.n_pt_l, nll = (size_t)in.n_ls_l, db = (size_t)in.desc_bytes;
    const int32_t po_l[2] = {0, in.n_pt_l}, po_r[2] = {0, in.n_pt_r}, lo_l[2] = {0, in.n_ls_l}, lo_r[2] = {0, in.n_ls_r};
    plba_stereo_batch b{};
    b.n = 1; b.desc_bytes = in.desc_bytes;
    b.pt_off_l = po_l; b.pt_off_r = po_r; b.ls_off_l = lo_l; b.ls_off_r = lo_r;
    b.pt_l = in.pt_l; b.pt_r = in.pt_r; b.pdesc_l = in.pdesc_l; b.pdesc_r = in.pdesc_r;
    b.ls_l = in.ls_l; b.ls_r = in.ls_r; b.ldesc_l = in.ldesc_l; b.ldesc_r = in.ldesc_r;
    int32_t n_pt = 0, n_ls = 0;
    std::vector<int32_t> psrc(npl + 1), lsrc(nll + 1);
    std::vector<uint8_t> pdesc(npl * db + 1), ldesc(nll * db + 1);
    std::vector<double> pl(2 * npl + 1), pdisp(npl + 1), P(3 * npl + 1), spl(2 * nll + 1), epl(2 * nll + 1), sdisp(nll + 1),
        edisp(nll + 1), sP(3 * nll + 1), eP(3 * nll + 1), le(3 * nll + 1), NDc(6 * nll + 1);
    plba_stereo_out o{};
    o.n_pt = &n_pt; o.n_ls = &n_ls;
    o.pt_src = psrc.data(); o.pt_pl = pl.data(); o.pt_disp = pdisp.data(); o.pt_P = P.data(); o.pdesc = pdesc.data();
    o.ls_src = lsrc.data(); o.ls_spl = spl.data(); o.ls_epl = epl.data(); o.ls_sdisp = sdisp.data(); o.ls_edisp = edisp.data();
    o.ls_sP = sP.data(); o.ls_eP = eP.data(); o.ls_le = le.data(); o.ls_NDc = NDc.data(); o.ldesc = ldesc.data();
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = backend(stereo_, "stereo", [&](plba_ctx *ctx) { return plba_stereo_associate(ctx, &b, &prm, &o); }, &b, &prm, &o);
    if (rc) return rc;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (n_pt < 0 || n_pt > in.n_pt_l || n_ls < 0 || n_ls > in.n_ls_l) {
        setError("setKeyframeStereo: %d / %d survivors of %d / %d rows", n_pt, n_ls, in.n_pt_l, in.n_ls_l);
        return PLBA_E_DEVICE;
    }
    // plslam_add_keyframe fixes the feature counts when it is given idx lists: they must agree then; a
    // keyframe added without a list of a kind is sized here, every idx -1 (`initial` false, :168, :411)
    StereoFrame &f = map_keyframes[kf_idx]->stereo_frame;
    if ((!f.stereo_pt_idx.empty() && (int)f.stereo_pt_idx.size() != n_pt) ||
        (!f.stereo_ls_idx.empty() && (int)f.stereo_ls_idx.size() != n_ls)) {
        setError("setKeyframeStereo: keyframe %d was added with %zu / %zu features, the frame has %d / %d", kf_idx,
                 f.stereo_pt_idx.size(), f.stereo_ls_idx.size(), n_pt, n_ls);
        return PLBA_E_INVALID;
    }
    if (f.stereo_pt_idx.empty()) f.stereo_pt_idx.assign((size_t)n_pt, -1);
    if (f.stereo_ls_idx.empty()) f.stereo_ls_idx.assign((size_t)n_ls, -1);
    const size_t kp = (size_t)n_pt, kl = (size_t)n_ls;
    f.desc_bytes = in.desc_bytes;
    f.pdesc_l.assign(pdesc.begin(), pdesc.begin() + kp * db);
    f.pt_P.assign(P.begin(), P.begin() + 3 * kp);
    f.pt_pl.assign(pl.begin(), pl.begin() + 2 * kp);
    f.ldesc_l.assign(ldesc.begin(), ldesc.begin() + kl * db);
    f.ls_sP.assign(sP.begin(), sP.begin() + 3 * kl);
    f.ls_eP.assign(eP.begin(), eP.begin() + 3 * kl);
    f.ls_le.assign(le.begin(), le.begin() + 3 * kl);
    f.ls_spl.assign(spl.begin(), spl.begin() + 2 * kl);
    f.ls_epl.assign(epl.begin(), epl.begin() + 2 * kl);
    f.has_features = true;
    f.has_endpoints = true;
    f.has_pluker = prm.pluker != 0;
    if (f.has_pluker) f.ls_NDc.assign(NDc.begin(), NDc.begin() + 6 * kl);
    else f.ls_NDc.clear();
    if (pt_src) std::copy(psrc.begin(), psrc.begin() + kp, pt_src);
    if (ls_src) std::copy(lsrc.begin(), lsrc.begin() + kl, ls_src);
    if (stats) *stats = StereoStats{n_pt, n_ls, ms};
    return PLBA_OK;
}

}  // namespace plslam
