"""Loop-closure relative pose on the GPU (plba_lc_relative_pose: computeRelativePoseRobustGN /
computeRelativePoseGN, src/mapHandler.cpp:4677-5068 / :4413-4675) against the numpy checker
(tests/ref_lcpose.py). The device sums H, g and e per thread and reduces them in a fixed tree, the
checker sums them in feature order, so the two agree to rounding, not bitwise; the decisions
(outlier flags, accept conditions) are kept away from their thresholds by the generator
(tests/test_lcpose_oracle.py checks the margins of exactly these candidates)."""
import numpy as np
import pytest

import lcpose_cases as cases
import parity
from plba import capi

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
BITWISE_KEYS = ("accepted", "conditions", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln", "e", "unc", "t", "r_deg",
                "x_inc", "pose_inc", "T_inc", "H", "pt_inlier", "ln_inlier")


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _bitwise_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in BITWISE_KEYS)


def _assert_parity(out, ref):
    for k in ("x_inc", "pose_inc", "T_inc", "e", "t", "r_deg"):
        v = parity.elem_violation(out[k], ref[k])
        print(k, "violation", v)
        assert v <= 1.0, (k, v, out[k], ref[k])
    dH = float(np.abs(out["H"] - ref["H"]).max() / np.abs(ref["H"]).max())
    print("H rel", dH)
    assert dH <= 1e-8, dH
    tol = 1e-8 + 100.0 * EPS * np.linalg.cond(ref["H"])
    du = abs(out["unc"] - ref["unc"]) / abs(ref["unc"])
    print("unc rel", du, "tol", tol)
    assert du <= tol, (out["unc"], ref["unc"], tol)
    assert np.array_equal(out["pt_inlier"], ref["pt_inlier"]) and np.array_equal(out["ln_inlier"], ref["ln_inlier"])
    for k in ("n_inl_pt", "n_inl_ln", "conditions", "accepted"):
        assert out[k] == ref[k], (k, out[k], ref[k])


@pytest.mark.parametrize("n_pt,n_ln,frac,variant", cases.parity_cases())
def test_parity_with_the_checker(solver, n_pt, n_ln, frac, variant):
    out = solver.lc_relative_pose([cases.problem(n_pt, n_ln, frac)], cases.params(variant))[0]
    ref = cases.reference(n_pt, n_ln, frac, variant)
    assert ref["accepted"] == 1  # a loop closure the function accepts
    _assert_parity(out, ref)


@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("n_pt,n_ln,frac", cases.CAPPED_CASES)
def test_iteration_counts_where_the_caps_end_both_loops(solver, n_pt, n_ln, frac, variant):
    p = cases.params(variant, max_iters_first=3, max_iters=2)
    out = solver.lc_relative_pose([cases.problem(n_pt, n_ln, frac)], p)[0]
    ref = cases.reference(n_pt, n_ln, frac, variant, 3, 2)
    assert ref["iters_first"] == 3 and ref["iters_ref"] == (2 if variant == capi.LCPOSE_ROBUST_GN else 0)
    assert (out["iters_first"], out["iters_ref"]) == (ref["iters_first"], ref["iters_ref"])
    _assert_parity(out, ref)


def _ids(cs):
    return [c.name for c in cs]


@pytest.mark.parametrize("case", cases.ONE_PASS_CASES, ids=_ids(cases.ONE_PASS_CASES))
def test_one_pass_from_the_identity(solver, case):
    """Variant GN with max_iters_first = 1: H and e as summed at T_inc = I, T_inc after exactly one step,
    the outlier flags at that pose. Nothing here depends on convergence, so the bar is not the 1e-8 of
    the full runs: H and e within 1.22e-13 relative, a hundred times the 1.218e-15 by which the checker
    differs from itself when the features are reordered (measured on these candidates by
    tests/test_lcpose_oracle.py; the device's tree matches no serial order), and T_inc within that bar
    times cond₂(H). Shapes: 6-8 features, 63/64/65 and 255/256/257 of one kind, both kinds, both sides of
    both clamps (homog_th = 0.5 and 0.25) and fy = 300."""
    p = case.params(capi.LCPOSE_GN, **cases.ONE_PASS)
    out = solver.lc_relative_pose([case.problem()], p)[0]
    ref = case.reference(capi.LCPOSE_GN, **cases.ONE_PASS)
    assert (out["iters_first"], out["iters_ref"]) == (1, 0) == (ref["iters_first"], ref["iters_ref"])
    fig = cases.one_pass_figures(out, ref)
    print(case.name, fig, "cond", np.linalg.cond(ref["H"]))
    for k, v in fig.items():
        assert v <= cases.ONE_PASS_BAR, (k, v)
    assert np.array_equal(out["H"], out["H"].T)
    assert np.array_equal(out["pt_inlier"], ref["pt_inlier"]) and np.array_equal(out["ln_inlier"], ref["ln_inlier"])
    for k in ("n_inl_pt", "n_inl_ln", "conditions", "accepted"):
        assert out[k] == ref[k], (k, out[k], ref[k])


@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("case,robust,gn", cases.REJECTED, ids=_ids([c for c, _, _ in cases.REJECTED]))
def test_each_accept_condition_fails_alone(solver, case, robust, gn, variant):
    """A rotation of 40 degrees (r_deg), a translation of 2 m (t), lc_res = 0.05 (e), lc_unc = 1e-6 (unc)
    and, in GN only, lc_inl = 0.9 over 75 % inliers: the one bit clear, the others set."""
    mask = robust if variant == capi.LCPOSE_ROBUST_GN else gn
    out = solver.lc_relative_pose([case.problem()], case.params(variant))[0]
    ref = case.reference(variant)
    assert ref["conditions"] == mask and out["conditions"] == mask, (ref["conditions"], out["conditions"], mask)
    assert out["accepted"] == ref["accepted"] == int(mask == 31)
    _assert_parity(out, ref)


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_stagnation_ends_both_loops_below_their_caps(solver, variant):
    """Noise-free data, caps 30 and 10: the first loop ends on |e − err_prev| < ε at pass 14, and the
    refinement on its first pass, which it could not with err_prev reset (e ~ 8e-8 is not below ε).
    The deciding differences are ε/3 and 26 ε with e rounded to ~1e-22, and the checker gives the same
    counts in five feature orders (tests/test_lcpose_oracle.py), so the count is not the summation order's.
    The third stop, ‖x‖ < ε, is reached by no finite candidate of the suite: it needs g = 0 to sixteen
    digits at a pose where e is neither below ε nor unchanged, and none is contrived."""
    case = cases.STAGNATION
    p = case.params(variant)
    out = solver.lc_relative_pose([case.problem()], p)[0]
    ref = case.reference(variant)
    assert (out["iters_first"], out["iters_ref"]) == (ref["iters_first"], ref["iters_ref"])
    assert out["iters_first"] == 14 < p.max_iters_first
    assert out["iters_ref"] == (1 if variant == capi.LCPOSE_ROBUST_GN else 0)
    _assert_parity(out, ref)


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_exact_observations_at_the_identity_stop_on_the_first_pass(solver, variant):
    """e < ε on the first pass: no step, and logmap_se3's arm for θ <= 1e-6."""
    out = solver.lc_relative_pose([cases.AT_IDENTITY.problem()], cases.AT_IDENTITY.params(variant))[0]
    ref = cases.AT_IDENTITY.reference(variant)
    assert out["iters_first"] == 1 and out["iters_ref"] == ref["iters_ref"]
    assert out["e"] < EPS
    assert out["T_inc"].tobytes() == np.eye(4)[:3].tobytes()
    assert not out["x_inc"].any() and not out["pose_inc"].any()
    assert out["t"] == 0.0 and out["r_deg"] == 0.0
    assert (out["n_inl_pt"], out["n_inl_ln"], out["conditions"]) == (40, 12, ref["conditions"])


FULL_RUN = cases.CLAMPS + cases.FULL_RUN


@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("case", FULL_RUN, ids=_ids(FULL_RUN))
def test_full_run_away_from_the_defaults(solver, case, variant):
    """The full function at the bars of the full runs: both sides of fmax(homog_th, r) and of
    fmax(homog_th, gz²) (all three clamp candidates are admitted: margins above 1e-6 and cond₂(H) <= 1e3),
    fy = 300 against fx = 458.654, a point behind the camera, and the smallest full-rank candidates
    (cond₂(H) up to 7e4; unc's bar scales with it)."""
    out = solver.lc_relative_pose([case.problem()], case.params(variant))[0]
    ref = case.reference(variant)
    _assert_parity(out, ref)
    if case.mirror >= 0:
        assert not out["pt_inlier"][case.mirror] and not ref["pt_inlier"][case.mirror] and out["n_inl_pt"] == case.n_pt - 1


def _decisions_equal(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
               for k in ("accepted", "conditions", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln", "pt_inlier", "ln_inlier"))


def _bitwise_equal_nan(a, b):
    """_bitwise_equal where a NaN equals a NaN of any payload."""
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in BITWISE_KEYS)


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_rank_deficient_candidates_are_rejected_on_the_uncertainty(solver, variant):
    """2 and 5 points, 3 lines (cond₂(H) >= 1e17): the decisions only. x of a truncated QR is not
    compared: its rank decision sits at rounding level on both sides."""
    p = cases.params(variant)
    good = cases.problem(40, 12, 0.25)
    probs = [c.problem() for c in cases.RANK_DEFICIENT]
    batch = solver.lc_relative_pose([probs[0], good, probs[1], probs[2]], p)
    assert _bitwise_equal(batch[1], solver.lc_relative_pose([good], p)[0]) and batch[1]["accepted"] == 1
    for o, q in zip((batch[0], batch[2], batch[3]), probs):
        assert o["accepted"] == 0 and not (o["conditions"] & 2)
        assert o["n_inl_pt"] == int(o["pt_inlier"].sum()) <= q.n_pt and o["n_inl_ln"] == int(o["ln_inlier"].sum()) <= q.n_ln
        assert _bitwise_equal_nan(o, solver.lc_relative_pose([q], p)[0])


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_a_point_with_zero_depth_is_rejected_and_leaves_its_neighbours_alone(solver, variant):
    """z = 0 in kf0 makes the first pass non-finite. Defined as in the checker: a non-finite H or g gives
    a NaN step, after which no comparison holds: both loops run to their caps, no match is flagged, e, unc
    and t fail their tests. The call itself succeeds (PLBA_OK: no exception)."""
    p = cases.ZERO_DEPTH.params(variant)
    ref = cases.ZERO_DEPTH.reference(variant)
    a, b = cases.problem(40, 12, 0.25), cases.problem(64, 0, 0.0)
    out = solver.lc_relative_pose([a, cases.ZERO_DEPTH.problem(), b], p)
    assert out[1]["accepted"] == 0 and ref["accepted"] == 0
    assert _decisions_equal(out[1], ref), (out[1], ref)
    assert np.isnan(out[1]["T_inc"]).all() and np.isnan(out[1]["e"]) and out[1]["unc"] == np.inf
    assert _bitwise_equal(out[0], solver.lc_relative_pose([a], p)[0]) and out[0]["accepted"] == 1
    assert _bitwise_equal(out[2], solver.lc_relative_pose([b], p)[0]) and out[2]["accepted"] == 1


def test_singular_and_empty_candidates_are_rejected_and_leave_their_neighbours_alone(solver):
    good_a, good_b = cases.problem(40, 12, 0.25), cases.problem(64, 0, 0.0)
    singular, empty = cases.problem(*cases.SINGULAR_SHAPE), cases.problem(*cases.EMPTY_SHAPE)
    alone = solver.lc_relative_pose([good_a])[0], solver.lc_relative_pose([good_b])[0]
    for variant in cases.VARIANTS:
        p = cases.params(variant)
        a1, b1 = solver.lc_relative_pose([good_a], p)[0], solver.lc_relative_pose([good_b], p)[0]
        out = solver.lc_relative_pose([singular, good_a, empty, good_b, empty], p)   # PLBA_OK: no exception
        assert [o["accepted"] for o in out] == [0, 1, 0, 1, 0]
        assert _bitwise_equal(out[1], a1) and _bitwise_equal(out[3], b1)
        assert np.array_equal(out[2]["T_inc"], np.eye(4)[:3])   # left as it was
        assert out[0]["unc"] > p.lc_unc and not (out[0]["conditions"] & 2)
        for o in (solver.lc_relative_pose([singular], p)[0], solver.lc_relative_pose([empty], p)[0]):
            assert o["accepted"] == 0
    assert alone[0]["accepted"] == 1 and alone[1]["accepted"] == 1


def test_a_candidate_emptied_by_the_outlier_pass_is_rejected(solver):
    # a first loop of zero passes leaves T_inc = I, where every observation, moved by 500 px, is an outlier
    import dataclasses
    import ref_lcpose
    base = cases.problem(40, 12, 0.0)
    le = base.ln_le.copy()
    le[:, 2] += 500.0
    pr = dataclasses.replace(base, pt_obs=base.pt_obs + 500.0, ln_le=le)
    p = cases.params(max_iters_first=0)
    ref = ref_lcpose.relative_pose(pr, p)
    assert ref["empty"] and ref["n_inl_pt"] == 0 and ref["n_inl_ln"] == 0
    neighbour = cases.problem(64, 0, 0.0)
    out = solver.lc_relative_pose([pr, neighbour], p)
    assert out[0]["accepted"] == 0 and out[0]["n_inl_pt"] == 0 and out[0]["n_inl_ln"] == 0
    assert np.array_equal(out[0]["T_inc"], np.eye(4)[:3])
    assert not out[0]["pt_inlier"].any() and not out[0]["ln_inlier"].any()
    assert _bitwise_equal(out[1], solver.lc_relative_pose([neighbour], p)[0])


def test_a_batch_equals_its_single_calls_bitwise_and_repeats_bitwise(solver):
    probs = [cases.problem(300, 100, 0.25), cases.problem(0, 64, 0.0), cases.problem(*cases.SINGULAR_SHAPE),
             cases.problem(40, 12, 0.25), cases.problem(64, 0, 0.25)]
    batch = solver.lc_relative_pose(probs)
    again = solver.lc_relative_pose(probs)
    for q, o, o2 in zip(probs, batch, again):
        assert _bitwise_equal(o, solver.lc_relative_pose([q])[0])
        assert _bitwise_equal(o, o2)


def test_relative_pose_leaves_an_uploaded_window_intact(solver):
    from plba import synth
    g = synth.generate("C1L")
    solver.upload(g)
    before = solver.lba_plucker()
    out = solver.lc_relative_pose([cases.problem(40, 12, 0.25)])[0]
    assert out["accepted"] == 1
    solver.reset()
    after = solver.lba_plucker()
    for k in ("kf_Tcw", "pt_xyz", "ln_orth"):
        assert np.array_equal(before[k], after[k]), k


def test_bad_arguments_are_refused(solver):
    import ctypes as C
    from plba.lib import PLBA_ERRORS, PlbaError
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        solver.lc_relative_pose([cases.problem(40, 12, 0.0)], cases.params(9))
    bv = capi.LcposeBatchView([cases.problem(40, 12, 0.0), cases.problem(64, 0, 0.0)])
    bv.pt_off[:] = [0, 104, 40]   # decreasing
    out = (capi.PlbaLcposeOut * 2)()
    p = cases.params()
    rc = solver.L.plba_lc_relative_pose(solver.ctx, C.byref(bv.struct), C.byref(p), out, None, None)
    assert PLBA_ERRORS.get(rc) == "PLBA_E_INVALID"
    bv.pt_off[:] = [0, 40, 104]
    bv.struct.n = -1
    assert PLBA_ERRORS.get(solver.L.plba_lc_relative_pose(solver.ctx, C.byref(bv.struct), C.byref(p), out, None, None)) \
        == "PLBA_E_INVALID"
    bv.struct.n = 2
    assert PLBA_ERRORS.get(solver.L.plba_lc_relative_pose(solver.ctx, C.byref(bv.struct), C.byref(p), None, None, None)) \
        == "PLBA_E_INVALID"
    bv.struct.n = 0   # nothing to do
    assert solver.L.plba_lc_relative_pose(solver.ctx, C.byref(bv.struct), C.byref(p), out, None, None) == 0
    bv.struct.n = 2   # and the same view, intact, is accepted
    assert solver.L.plba_lc_relative_pose(solver.ctx, C.byref(bv.struct), C.byref(p), out, None, None) == 0
    assert out[0].accepted == 1 and out[1].accepted == 1
