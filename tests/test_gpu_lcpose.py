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
