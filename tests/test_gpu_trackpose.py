"""Frame-to-frame pose on the GPU (plba_track_pose: StereoFrameHandler::optimizePose,
src2/stereoFrameHandler.cpp:307-405, both line models) against the numpy checker
(tests/ref_trackpose.py). The device sums H, g and e per thread and reduces them in a fixed tree, the
checker sums them in match order, so the two agree to rounding, not bitwise; the medians behind the
scales s_p and s_l are exact order statistics and are compared bitwise. The decisions (inlier flags,
stop tests, isGoodSolution, min_features) are kept away from their thresholds by the generator
(tests/test_trackpose_oracle.py checks the margins of exactly these cases)."""
import numpy as np
import pytest

import parity
import trackpose_cases as cases
from plba import capi, trackpose as tp

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
INT_KEYS = ("branch", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln")
BITWISE_KEYS = INT_KEYS + ("err_norm", "s_p", "s_l", "DT", "DT_cov", "DT_cov_eig", "DT_solver", "H", "pt_inlier",
                           "ln_inlier")
model_param = pytest.mark.parametrize("model", cases.MODELS, ids=cases.MODEL_IDS)


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _bitwise_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in BITWISE_KEYS)


def _assert_parity(out, ref):
    for k in INT_KEYS:
        assert out[k] == ref[k], (k, out[k], ref[k])
    assert np.array_equal(out["pt_inlier"], ref["pt_inlier"]) and np.array_equal(out["ln_inlier"], ref["ln_inlier"])
    for k in ("DT", "DT_solver", "err_norm", "s_p", "s_l"):
        v = parity.elem_violation(out[k], ref[k])
        print(k, "violation", v)
        assert v <= 1.0, (k, v, out[k], ref[k])
    if np.abs(ref["H"]).max() > 0:
        dH = float(np.abs(out["H"] - ref["H"]).max() / np.abs(ref["H"]).max())
        print("H rel", dH)
        assert dH <= 1e-8, dH
    if ref["err_norm"] != -1.0:
        tol = 1e-8 + 100.0 * EPS * np.linalg.cond(ref["H"])
        for k in ("DT_cov", "DT_cov_eig"):
            d = float(np.abs(out[k] - ref[k]).max() / np.abs(ref[k]).max())
            print(k, "rel", d, "tol", tol)
            assert d <= tol, (k, d, tol)
    else:
        assert not out["DT_cov"].any() and not out["DT_cov_eig"].any()
        assert out["DT"].tobytes() == np.eye(4).tobytes()


def _ids(cs):
    return [c.name for c in cs]


@model_param
@pytest.mark.parametrize("case", cases.PARITY, ids=_ids(cases.PARITY))
def test_parity_with_the_checker(solver, case, model):
    out = solver.track_pose([case.problem()], case.params(model))[0]
    ref = case.reference(model)
    if case.n_pt + case.n_ln >= 100:
        assert ref["branch"] == capi.TRACK_OK and ref["n_inl_pt"] < case.n_pt + (case.n_pt == 0)
    _assert_parity(out, ref)


@model_param
@pytest.mark.parametrize("case", cases.PROBES, ids=_ids(cases.PROBES))
def test_the_scales_of_one_pass_are_bitwise_the_checkers(solver, case, model):
    """max_iters = 1 at the identity on all matches: the residuals are the same operations on both sides,
    the medians are exact, so s_p and s_l are equal to the last bit (the float rounding of fabsf and the
    n/2 index). 63 / 64 / 65 matches of a kind, and a list whose median lies in a run of equal values."""
    out = solver.track_pose([case.problem()], case.params(model))[0]
    ref = case.reference(model)
    assert ref["iters_first"] == 1 and out["iters_first"] == 1
    assert np.float64(out["s_p"]).tobytes() == np.float64(ref["s_p"]).tobytes(), (out["s_p"], ref["s_p"])
    assert np.float64(out["s_l"]).tobytes() == np.float64(ref["s_l"]).tobytes(), (out["s_l"], ref["s_l"])
    assert rt_min() < out["s_p"] < rt_max() and rt_min() < out["s_l"] < rt_max()   # neither clamp hides a median
    _assert_parity(out, ref)


def rt_min():
    return 0.0001


def rt_max():
    return float(np.sqrt(7.815))


@model_param
@pytest.mark.parametrize("branch", sorted(cases.BRANCH), ids=[cases.BRANCH[b].name for b in sorted(cases.BRANCH)])
def test_each_branch_of_optimize_pose(solver, branch, model):
    case = cases.BRANCH[branch]
    out = solver.track_pose([case.problem()], case.params(model))[0]
    ref = case.reference(model)
    assert ref["branch"] == branch and out["branch"] == branch, (ref["branch"], out["branch"])
    assert (out["err_norm"] != -1.0) == (branch == capi.TRACK_OK)
    _assert_parity(out, ref)


@model_param
def test_a_rank_deficient_problem_has_a_negative_log_determinant(solver, model):
    """All matches the same point: the QR's R has four tiny pivots, logAbsDeterminant() < 0, the loop
    restores DT, err = -1 and cov = I, which isGoodSolution rejects."""
    case = cases.BRANCH[capi.TRACK_FIRST_NOT_GOOD]
    out = solver.track_pose([case.problem()], case.params(model))[0]
    ref = case.reference(model)
    assert [t["logdet"] for t in ref["trace"] if t["logdet"] is not None][0] < -10.0
    assert out["iters_first"] == 1 and out["err_norm"] == -1.0
    assert out["DT_solver"].tobytes() == np.eye(4).tobytes() and out["DT"].tobytes() == np.eye(4).tobytes()
    _assert_parity(out, ref)


@model_param
def test_motion_model_input_that_is_good_solution_rejects(solver, model):
    """err_norm = 2 of the previous frame: DT starts at the identity, and the result is bitwise that of a run
    without the motion model; with err_norm = 0.5 it starts at the previous DT and differs."""
    rej, acc = cases.MOTION_REJECTED, cases.MOTION_ACCEPTED
    out = solver.track_pose([rej.problem()], rej.params(model))[0]
    plain = solver.track_pose([rej.problem()], rej.params(model, use_motion_model=0))[0]
    assert _bitwise_equal(out, plain)
    _assert_parity(out, rej.reference(model))
    out_acc = solver.track_pose([acc.problem()], acc.params(model))[0]
    assert out_acc["branch"] == capi.TRACK_OK and not _bitwise_equal(out_acc, plain)
    _assert_parity(out_acc, acc.reference(model))


@model_param
def test_a_match_with_z_zero_returns_rejected_and_leaves_its_neighbours_alone(solver, model):
    ok = cases.BRANCH[capi.TRACK_OK]
    p = ok.params(model)
    alone = solver.track_pose([ok.problem()], p)[0]
    batch = solver.track_pose([ok.problem(), cases.Z0.problem(), ok.problem()], p)
    assert batch[1]["branch"] != capi.TRACK_OK and batch[1]["err_norm"] == -1.0
    assert batch[1]["DT"].tobytes() == np.eye(4).tobytes() and not batch[1]["DT_cov"].any()
    assert not np.isfinite(batch[1]["H"]).all()
    assert _bitwise_equal(batch[0], alone) and _bitwise_equal(batch[2], alone)
    assert cases.Z0.reference(model)["branch"] == batch[1]["branch"]


def _mixed_batch(model):
    ok, other = cases.BRANCH[capi.TRACK_OK], cases.PARITY[3]
    fill = [other.problem(), tp.empty(), cases.BRANCH[capi.TRACK_FEW_BEFORE].problem(), cases.PARITY[4].problem()]
    batch = [ok.problem()] + [fill[i % 4] for i in range(38)] + [ok.problem()]
    return ok, batch


@model_param
def test_batch_is_deterministic_and_position_independent(solver, model):
    """The same batch twice is bitwise equal; a problem alone and at positions 0 and 39 of a mixed batch of
    40 (with empty problems in it) is bitwise equal. The single call after the batch also shrinks the
    request on a context whose scratch block has grown."""
    ok, batch = _mixed_batch(model)
    p = ok.params(model)
    small = solver.track_pose([ok.problem()], p)[0]          # a small block first
    a = solver.track_pose(batch, p)                          # the block grows
    b = solver.track_pose(batch, p)
    assert len(a) == 40 and all(_bitwise_equal(x, y) for x, y in zip(a, b))
    alone = solver.track_pose([ok.problem()], p)[0]
    assert _bitwise_equal(a[0], alone) and _bitwise_equal(a[39], alone) and _bitwise_equal(small, alone)
    assert a[2]["branch"] == capi.TRACK_FEW_BEFORE and a[2]["n_inl_pt"] == 0   # the empty problem
    _assert_parity(alone, ok.reference(model))


def test_an_uploaded_window_survives_the_call(solver):
    import golden_io
    g, _ = golden_io.load("C1L")
    solver.upload(g)
    before = solver.lba_plucker()
    solver.upload(g)
    ok = cases.BRANCH[capi.TRACK_OK]
    solver.track_pose([ok.problem()] * 3, ok.params(capi.TRACK_PLUCKER))
    after = solver.lba_plucker()
    assert np.array_equal(before["chi2"], after["chi2"])


def _wide(n):
    pr = tp.synth(n, 0, seed=1, outlier_frac=0.1)
    return pr


def test_the_cap_on_matches_and_one_above(solver):
    from plba.lib import PlbaError
    p = capi.track_params(max_iters=2, max_iters_ref=2)
    out = solver.track_pose([_wide(capi.TRACK_MAX_N)], p)[0]
    assert out["branch"] == capi.TRACK_OK and 0 < out["n_inl_pt"] < capi.TRACK_MAX_N
    with pytest.raises(PlbaError) as e:
        solver.track_pose([_wide(capi.TRACK_MAX_N + 1)], p)
    assert str(capi.TRACK_MAX_N + 1) in str(e.value) and str(capi.TRACK_MAX_N) in str(e.value)
    ok = cases.BRANCH[capi.TRACK_OK]
    _assert_parity(solver.track_pose([ok.problem()], ok.params(0))[0], ok.reference(0))   # the context is usable


def test_invalid_arguments(solver):
    import ctypes as C
    from plba.lib import PlbaError
    ok = cases.BRANCH[capi.TRACK_OK]
    assert solver.track_pose([]) == []                                   # n == 0: PLBA_OK
    for kw in (dict(line_model=2), dict(max_iters=0), dict(max_iters_ref=0)):
        with pytest.raises(PlbaError):
            solver.track_pose([ok.problem()], capi.track_params(**kw))
    bv = capi.TrackBatchView([ok.problem()])
    out = (capi.PlbaTrackOut * 1)()
    prm = capi.track_params()
    L = solver.L

    def call(**kw):
        for k, v in kw.items():
            setattr(bv.struct, k, v)
        return L.plba_track_pose(solver.ctx, C.byref(bv.struct), C.byref(prm), out, None, None)

    assert call() == 0                                                   # the inlier arrays are optional
    assert call(n=-1) != 0
    assert call(n=1, ln_NDc=None) != 0                                   # the Plücker model reads NDc
    bad = np.array([5, 0], np.int32)
    assert call(pt_off=bad.ctypes.data_as(C.POINTER(C.c_int32))) != 0    # decreasing offsets
    assert L.plba_track_pose(solver.ctx, None, C.byref(prm), out, None, None) != 0
    _assert_parity(solver.track_pose([ok.problem()], ok.params(0))[0], ok.reference(0))   # the context is usable
