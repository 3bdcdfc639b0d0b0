"""TEST INFRASTRUCTURE: checker of plba_track_frames (include/plba.h), that is of
StereoFrameHandler::f2fTracking followed by optimizePose (src2/stereoFrameHandler.cpp:106-180, :307-405).
The matcher is tests/ref_descmatch.py and the pose is tests/ref_trackpose.py, both as they are; what is
added here is only what lies between them: the loops around matches_12 (:144-152, :167-179), which push
the matched previous rows in increasing i1 with the current row's observation, and write the previous
row's idx into the current row, so that the last i1 that names a current row stays."""
from __future__ import annotations

import numpy as np

import ref_descmatch as rd
import ref_trackpose as rt
from plba.trackpose import TrackProblem


def _match(desc1, desc2, nnr, best_lr, on):
    """matches_12 of one kind and the matcher's detail; a kind that is switched off or has an empty side has
    no match (:137, :160)."""
    desc1, desc2 = np.asarray(desc1, np.uint8), np.asarray(desc2, np.uint8)
    if not on or len(desc1) == 0 or len(desc2) == 0:
        return np.full(len(desc1), -1, np.int32), None
    d = rd.match_detail(desc1, desc2, np.float32(nnr), bool(best_lr))
    return d["matches_12"], d


def scatter_loop(m12, n2):
    """The loop of :144-152 / :167-179 as it is written: (rows, cur_from_prev). rows are the (i1, i2) pushed,
    in push_back order; cur_from_prev[i2] is the i1 whose idx the current row holds when the loop ends."""
    rows, cfp = [], np.full(n2, -1, np.int32)
    for i1 in range(len(m12)):
        i2 = int(m12[i1])
        if i2 < 0:
            continue
        rows.append((i1, i2))
        cfp[i2] = i1
    return np.asarray(rows, np.int64).reshape(-1, 2), cfp


def track_frames(pair, params) -> dict:
    """The fields of Solver.track_frames for one pair (params: a capi.PlbaFramesParams), plus `problem` (the
    pose problem that was gathered), `pt_rows` / `ln_rows` (its (i1, i2) in order), `pt_detail` / `ln_detail`
    (the matcher's figures) and everything tests/ref_trackpose.py adds."""
    tp = params.track
    f = lambda a, w: np.asarray(a, np.float64).reshape(-1, w)
    pt_m12, pt_detail = _match(pair.prev_pdesc, pair.cur_pdesc, params.nnr_pt, params.best_lr, tp.has_points)
    ln_m12, ln_detail = _match(pair.prev_ldesc, pair.cur_ldesc, params.nnr_ln, params.best_lr, tp.has_lines)
    pt_rows, pt_cfp = scatter_loop(pt_m12, len(np.asarray(pair.cur_pdesc)))
    ln_rows, ln_cfp = scatter_loop(ln_m12, len(np.asarray(pair.cur_ldesc)))
    i1, i2, j1, j2 = pt_rows[:, 0], pt_rows[:, 1], ln_rows[:, 0], ln_rows[:, 1]
    prob = TrackProblem(pt_P=f(pair.prev_pt_P, 3)[i1], pt_obs=f(pair.cur_pt_pl, 2)[i2], pt_sigma2=f(pair.prev_pt_sigma2, 1)[i1, 0],
                        ln_sP=f(pair.prev_ln_sP, 3)[j1], ln_eP=f(pair.prev_ln_eP, 3)[j1], ln_NDc=f(pair.prev_ln_NDc, 6)[j1],
                        ln_le=f(pair.cur_ln_le, 3)[j2], ln_obs=f(pair.cur_ln_seg, 4)[j2], ln_seg=f(pair.prev_ln_seg, 4)[j1],
                        ln_sigma2=f(pair.prev_ln_sigma2, 1)[j1, 0], prev=np.asarray(pair.prev, np.float64), cam=tuple(pair.cam))
    out = rt.track_pose(prob, tp)
    pin, lin = np.zeros(len(pt_m12), np.uint8), np.zeros(len(ln_m12), np.uint8)
    pin[i1], lin[j1] = out["pt_inlier"], out["ln_inlier"]
    out.update(pt_inlier=pin, ln_inlier=lin, pt_m12=pt_m12.astype(np.int32), ln_m12=ln_m12.astype(np.int32),
               n_pt=len(pt_rows), n_ln=len(ln_rows), pt_cur_from_prev=pt_cfp, ln_cur_from_prev=ln_cfp, problem=prob,
               pt_rows=pt_rows, ln_rows=ln_rows, pt_detail=pt_detail, ln_detail=ln_detail)
    return out
