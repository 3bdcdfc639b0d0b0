"""What tests/test_gpu_depth.py takes for granted, shown on the CPU checker alone: the windows of
tests/depth_cases.py really put points behind cameras (both outcomes of isDepthPositive, edges the
stage switch classifies by depth alone, depths far from zero so that the flag's sign test is exact
on any arithmetic), and the large-τ windows really end the damped trial loop through ρ == 0 and
through a non-finite λ, with finite estimates throughout."""
import numpy as np
import pytest

import depth_cases as dc
import graph_mut as gm
import oracle_api as oa
from plba import synth

EST = ("kf_Tcw", "pt_xyz", "ln_orth")
MARGIN = 1e-6


def _finite(ref):
    return all(np.isfinite(ref[k]).all() for k in EST + ("ept_chi2", "eln_chi2", "chi2"))


def test_mutation_reflects_through_the_camera_centre():
    g0 = synth.generate("C1L")
    g = gm.points_behind_cameras(g0)
    sel = g._behind
    np.testing.assert_array_equal(sel, np.arange(g0.n_pt)[::7][:20])
    C = gm.camera_centres(g0)
    for k in range(g0.n_kf):  # C_k = −Rᵀt: the point the pose maps to the origin
        assert np.abs(g0.kf_Tcw[k, :, :3] @ C[k] + g0.kf_Tcw[k, :, 3]).max() < 1e-12
    rest = np.setdiff1d(np.arange(g0.n_pt), sel)
    np.testing.assert_array_equal(g.pt_xyz[rest], g0.pt_xyz[rest])
    d0 = gm.point_depths(g0.kf_Tcw, g0.pt_xyz, g0.ept_kf, g0.ept_lm)
    d = gm.point_depths(g.kf_Tcw, g.pt_xyz, g.ept_kf, g.ept_lm)
    for j in sel:
        e = np.nonzero(g0.ept_lm == j)[0]
        first = g0.ept_kf[e[0]]
        np.testing.assert_allclose(g.pt_xyz[j] + g0.pt_xyz[j], 2.0 * C[first], rtol=0, atol=1e-12)
        assert abs(d[e[0]] + d0[e[0]]) < 1e-12 and d[e[0]] < 0  # the same ray, behind the camera
    # "mean" reflects through the mean centre, "short" only landmarks with at most 3 observations
    gmn = gm.points_behind_cameras(g0, through="mean")
    j = sel[3]
    kfs = g0.ept_kf[g0.ept_lm == j]
    np.testing.assert_allclose(gmn.pt_xyz[j] + g0.pt_xyz[j], 2.0 * C[kfs].mean(axis=0), rtol=0, atol=1e-12)
    gs = gm.points_behind_cameras(g0, through="short")
    assert len(gs._behind) and np.bincount(g0.ept_lm, minlength=g0.n_pt)[gs._behind].max() <= 3


@pytest.mark.parametrize("name", list(dc.VARIANTS))
def test_checker_sees_both_depth_outcomes(name):
    g = dc.window(name)
    assert (g.n_kf, g.n_pt, g.n_ln) == (10, 200, 40)
    ref, ref1 = dc.oracle(name), dc.oracle_stage1(name)
    assert _finite(ref) and _finite(ref1)
    for r in (ref, ref1):
        assert int((r["ept_depth_ok"] == 0).sum()) >= 20 and int((r["ept_depth_ok"] == 1).sum()) >= 20
    # classified by depth alone: level 1, behind the camera, stage-1 χ² at or below the threshold
    assert dc.stage1_ends_on_accept(ref1), ref1["trace"][-1]
    only = dc.depth_only(ref, ref1)
    assert int(only.sum()) >= 2, int(only.sum())
    # the classification is the reference's rule on the stage-1 values
    np.testing.assert_array_equal(ref["ept_level"], (ref1["ept_chi2"] > dc.CHI2_THR) | (ref1["ept_depth_ok"] == 0))
    # no depth near zero at the start, at the stage switch or at the end
    for est, flags in ((None, None), (ref1, ref1["ept_depth_ok"]), (ref, ref["ept_depth_ok"])):
        d = dc.depths(g, est)
        assert np.abs(d).min() >= MARGIN, np.abs(d).min()
        if flags is not None:
            np.testing.assert_array_equal(flags, (d > 0).astype(np.uint8))
    assert any(t["trials"] > 1 for t in ref["trace"]), ref["trace"]
    np.testing.assert_array_equal(ref["iters"], [5, 10])


@pytest.mark.parametrize("order", dc.ORDERS)
@pytest.mark.parametrize("shuffled", [0, 1])
def test_checker_on_the_caller_order_windows(order, shuffled):
    g = dc.order_windows(order)[shuffled]
    assert (g.n_eln == 0) == (order == "points")
    ref, ref1 = dc.order_oracle(order, shuffled), dc.order_oracle(order, shuffled, stage1=True)
    assert _finite(ref) and _finite(ref1)
    for r, est in ((ref1, ref1), (ref, ref)):
        assert int((r["ept_depth_ok"] == 0).sum()) >= 20 and int((r["ept_depth_ok"] == 1).sum()) >= 20
        assert np.abs(dc.depths(g, est)).min() >= MARGIN
    assert np.abs(dc.depths(g, None)).min() >= MARGIN
    if shuffled:  # the same problem: the flags are the unshuffled ones in the recorded edge order
        pe = g._perm["pe"]
        for s1 in (False, True):
            base = dc.order_oracle(order, 0, stage1=s1)
            np.testing.assert_array_equal(dc.order_oracle(order, 1, stage1=s1)["ept_depth_ok"],
                                          base["ept_depth_ok"][pe])
        assert not np.array_equal(ref["ept_depth_ok"], dc.order_oracle(order, 0)["ept_depth_ok"])


def test_checker_on_the_no_solve_window():
    g = dc.no_solve_window()
    ref, chi2 = dc.no_solve_oracle()
    # exact depths: Z + 4 in the first keyframe, Z itself in the second
    d = gm.point_depths(g.kf_Tcw, g.pt_xyz, g.ept_kf, g.ept_lm)
    assert tuple(d[1::2]) == dc.NO_SOLVE_DEPTHS
    # the -0.0 case: every term of 0·X + 0·Y + 1·Z + t_z is -0.0 (the flag must not depend on it)
    assert np.signbit(g.pt_xyz[1]).all() and np.signbit(g.kf_Tcw[1, 2, 3]) and not np.signbit(g.pt_xyz[0, 2])
    assert tuple(d[0::2]) == (4.0, 4.0, 4.0, 4.0, 7.0, 9.0)
    np.testing.assert_array_equal(ref["ept_depth_ok"][1::2], dc.NO_SOLVE_FLAGS_KF1)
    np.testing.assert_array_equal(ref["ept_depth_ok"][0::2], 1)
    np.testing.assert_array_equal(ref["iters"], [0, 0])
    for k in ("kf_Tcw", "pt_xyz"):
        np.testing.assert_array_equal(ref[k], getattr(g, k))
    # χ²: finite in the first keyframe and for the two ordinary points, non-finite at the four depths
    fin = np.isfinite(chi2)
    np.testing.assert_array_equal(fin[0::2], True)
    np.testing.assert_array_equal(fin[1::2], [False, False, False, False, True, True])
    # the schedule's own χ² (level-1 edges refreshed, the others never evaluated) agrees where it evaluates
    lv = ref["ept_level"] == 1
    np.testing.assert_array_equal(lv, ref["ept_depth_ok"] == 0)
    np.testing.assert_array_equal(np.isfinite(ref["ept_chi2"][lv]), False)


@pytest.mark.parametrize("name", list(dc.TERMINATION))
def test_checker_ends_the_trial_loop_early(name):
    g = dc.termination_window()
    ref = dc.termination_oracle(name)
    assert _finite(ref)
    tr = ref["trace"]
    assert len(tr) == int(ref["iters"].sum())
    assert np.isfinite(tr["lambda_start"]).all()  # every factorised system is finite
    rho0 = [t for t in tr if t["result"] == 1 and 0 < t["trials"] < 10]
    assert rho0, tr
    for t in rho0:  # ρ == 0: χ² unchanged, the rejected trial multiplied λ by ν = 2
        assert t["chi2_end"] == t["chi2_start"] and t["lambda_end"] == 2.0 * t["lambda_start"], t
    if name == "lambda_inf":
        t = tr[0]
        assert t["stage"] == 0 and t["trials"] == 0 and t["result"] == 1, t
        assert np.isinf(t["lambda_end"]) and t["chi2_end"] == t["chi2_start"], t
    else:
        assert np.isfinite(tr["lambda_end"]).all()
    # steps that far below one ulp move nothing: every trial state is bitwise the current one, so
    # ρ == 0 is exact and does not hang on the rounding of an update
    for k in EST:
        np.testing.assert_array_equal(ref[k], getattr(g, k), err_msg=k)
    np.testing.assert_array_equal(ref["iters"], [1, 1])

