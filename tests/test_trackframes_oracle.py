"""The checker of the frame-to-frame tracking (tests/ref_trackframes.py) pinned on two hand-built descriptor
sets whose results are written out here, and the margins of every case the GPU tests use
(tests/trackframes_cases.py): the ratio test in float, the branch tests and min_features of the pose. A case
that fails a margin gets another seed in trackframes_cases.py; it is never skipped on the GPU."""
import numpy as np
import pytest

import ref_trackframes as rf
import trackframes_cases as cases
import trackpose_cases as pcases
from plba import capi, trackframes as tf

model_param = pytest.mark.parametrize("model", cases.MODELS, ids=cases.MODEL_IDS)


# ---- the loop around matches_12 (:144-152, :167-179)
def test_scatter_loop_pushes_in_row_order_and_the_last_writer_stays():
    rows, cfp = rf.scatter_loop([2, -1, 0, 2, -1, 2], 4)
    assert rows.tolist() == [[0, 2], [2, 0], [3, 2], [5, 2]]
    assert cfp.tolist() == [2, -1, 5, -1]
    rows, cfp = rf.scatter_loop([], 3)
    assert rows.shape == (0, 2) and cfp.tolist() == [-1, -1, -1]
    assert np.array_equal(tf.cur_from_prev([2, -1, 0, 2, -1, 2], 4), [2, -1, 5, -1])   # the package's helper agrees


def test_d_by_hand_three_previous_rows_share_a_current_row():
    """best_lr = 0: rows 1, 2 and 3 are 1, 2 and 0 bits from current row 0 and 31, 30, 32 from the next."""
    ref = cases.D_SMALL.reference(capi.TRACK_PLUCKER)[0]
    assert ref["pt_detail"]["fwd"]["d0"].tolist() == [0, 1, 2, 0, 0]
    assert ref["pt_detail"]["fwd"]["d1"].tolist() == [32, 31, 30, 32, 32]
    assert ref["pt_m12"].tolist() == [1, 0, 0, 0, 2]
    assert ref["pt_rows"].tolist() == [[0, 1], [1, 0], [2, 0], [3, 0], [4, 2]]       # all three enter the pose problem
    assert ref["pt_cur_from_prev"].tolist() == [3, 0, 4]                             # the largest i1
    assert ref["n_pt"] == 5 and ref["n_ln"] == 0 and ref["branch"] == capi.TRACK_FEW_BEFORE
    q = cases.D_SMALL.pairs()[0]
    assert np.array_equal(ref["problem"].pt_P, q.prev_pt_P)
    assert np.array_equal(ref["problem"].pt_obs, q.cur_pt_pl[[1, 0, 0, 0, 2]])
    # with the cross-check only the row that current row 0 names back survives
    assert rf.track_frames(q, capi.frames_params(best_lr=True, desc_bytes=8))["pt_m12"].tolist() == [1, -1, -1, 0, 2]


def test_e_by_hand_ties_go_to_the_lowest_current_row():
    """Current rows (0, 2) and (1, 3) are equal descriptors; previous rows 1 and 0 are one bit from them."""
    ref = cases.E_SMALL.reference(capi.TRACK_PLUCKER)[0]
    fwd = ref["pt_detail"]["fwd"]
    assert fwd["d0"].tolist() == [1, 1, 0] and fwd["d1"].tolist() == [1, 1, 32] and fwd["tie"].tolist() == [True, True, False]
    assert ref["pt_m12"].tolist() == [1, 0, 4]
    assert ref["pt_rows"].tolist() == [[0, 1], [1, 0], [2, 4]]
    assert ref["pt_cur_from_prev"].tolist() == [1, 0, -1, -1, 2]
    q = cases.E_SMALL.pairs()[0]
    assert np.array_equal(ref["problem"].pt_obs, q.cur_pt_pl[[1, 0, 4]])              # through to the gathered obs
    # a ratio below 1 rejects a tie
    assert rf.track_frames(q, capi.frames_params(nnr_pt=0.9, desc_bytes=8))["pt_m12"].tolist() == [-1, -1, 4]


def test_a_kind_that_is_switched_off_or_has_an_empty_side_has_no_match():
    q = cases.A.pairs()[0]
    ref = rf.track_frames(q, cases.A.params(capi.TRACK_PLUCKER, has_points=0))
    assert (ref["pt_m12"] == -1).all() and ref["n_pt"] == 0 and ref["n_ln"] == 12 and (ref["pt_cur_from_prev"] == -1).all()
    lines, empty_prev = (cases.B.reference(capi.TRACK_PLUCKER)[k] for k in (2, 3))
    assert len(lines["pt_m12"]) == 5 and (lines["pt_m12"] == -1).all() and len(lines["pt_cur_from_prev"]) == 0
    assert len(empty_prev["pt_m12"]) == 0 and empty_prev["pt_cur_from_prev"].tolist() == [-1] * 6
    assert empty_prev["ln_cur_from_prev"].tolist() == [-1] * 4 and empty_prev["branch"] == capi.TRACK_FEW_BEFORE


# ---- the cases are what their names say
@model_param
def test_the_cases_reach_what_they_are_for(model):
    a = cases.A.reference(model)[0]
    assert a["branch"] == capi.TRACK_OK and a["n_pt"] == 12 and a["n_ln"] == 12
    b = cases.B.reference(model)
    assert b[1]["n_pt"] + b[1]["n_ln"] == 9 and b[1]["branch"] == capi.TRACK_FEW_BEFORE
    assert (b[2]["n_pt"], b[2]["n_ln"]) == (0, 12) and (b[3]["n_pt"], b[3]["n_ln"]) == (0, 0)
    c = cases.C.reference(model)
    assert np.array_equal(np.flatnonzero(c[0]["pt_m12"] >= 0), np.arange(0, 65, 2))
    assert np.array_equal(np.flatnonzero(c[1]["ln_m12"] >= 0), np.arange(0, 257, 2)) and len(c[1]["pt_m12"]) == 257
    assert np.flatnonzero(c[2]["pt_m12"] >= 0).tolist() == [63, 127, 191, 255] and len(c[2]["pt_m12"]) == 256
    d = cases.D.reference(model)[0]
    j = int(cases.D.pairs()[0].true_pt[4, 1])
    assert np.flatnonzero(d["pt_m12"] == j).tolist() == [4, 12, 13] and d["pt_cur_from_prev"][j] == 13 and d["n_pt"] == 14
    e, q = cases.E.reference(model)[0], cases.E.pairs()[0]
    i1, j = (int(v) for v in q.true_pt[5])
    assert e["pt_detail"]["fwd"]["tie"][i1] and e["pt_m12"][i1] == j and np.array_equal(q.cur_pdesc[j], q.cur_pdesc[12])
    assert np.array_equal(e["problem"].pt_obs[i1], q.cur_pt_pl[j]) and not np.array_equal(q.cur_pt_pl[j], q.cur_pt_pl[12])
    f = cases.F.reference(model)[0]
    assert f["n_pt"] == capi.TRACK_MAX_N and (f["pt_m12"] >= 0).all() and f["branch"] == capi.TRACK_OK
    g = cases.G.reference(model)
    plain = rf.track_frames(cases.G.pairs()[1], cases.G.params(model, use_motion_model=0))
    assert g[0]["branch"] == capi.TRACK_OK and np.array_equal(g[1]["DT_solver"], plain["DT_solver"])
    assert not np.array_equal(g[0]["DT_solver"], rf.track_frames(cases.G.pairs()[0], cases.G.params(model, use_motion_model=0))["DT_solver"])
    h, q = cases.H.reference(model)[0], cases.H.pairs()[0]
    assert h["branch"] == capi.TRACK_OK and 0 < h["n_inl_pt"] < h["n_pt"] == 60 and 0 < h["n_inl_ln"] < h["n_ln"] == 20
    src = pcases.BRANCH[capi.TRACK_OK].problem()    # the same synthetic problem: its outlier rows are known
    assert np.array_equal(np.flatnonzero(h["pt_m12"] >= 0), q.true_pt[:, 0])
    assert np.array_equal(h["pt_inlier"][q.true_pt[:, 0]] == 0, src.pt_outlier) and h["pt_inlier"].sum() == h["n_inl_pt"]
    assert np.array_equal(h["ln_inlier"][q.true_ln[:, 0]] == 0, src.ln_outlier) and h["ln_inlier"].sum() == h["n_inl_ln"]


@pytest.mark.parametrize("case", cases.GPU_CASES, ids=[c.name for c in cases.GPU_CASES])
def test_the_planted_matches_are_found_and_nothing_else(case):
    for q, ref in zip(case.pairs(), case.reference(capi.TRACK_PLUCKER)):
        if len(q.true_pt) + len(q.true_ln) == 0:
            continue
        for m12, true in ((ref["pt_m12"], q.true_pt), (ref["ln_m12"], q.true_ln)):
            assert np.array_equal(m12[true[:, 0]], true[:, 1])
            if case not in (cases.D, cases.E):   # (these two add rows to a pair after it was planted)
                assert (m12 >= 0).sum() == len(true)


# ---- the margins of every case used on the GPU
@model_param
@pytest.mark.parametrize("case", cases.GPU_CASES, ids=[c.name for c in cases.GPU_CASES])
def test_every_decision_keeps_its_margin(case, model):
    r = cases.ratio_margin(case, model)
    print(case.name, "ratio", r)
    assert r > cases.MARGIN_RATIO, r
    for k in range(len(case.pairs())):
        view = cases.PoseView(case, k)
        m = pcases.margins(view, model)
        print(view.name, m)
        assert m["inlier"] > pcases.MARGIN_PX, m
        assert m["stop"] > pcases.MARGIN_REL, m
        assert m["good"] > pcases.MARGIN_REL, m
        assert m["features"] >= 0.5, m   # integers on both sides of min_features
