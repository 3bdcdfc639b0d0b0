"""The numpy checker of the loop-closure relative pose (tests/ref_lcpose.py) against what the function
is described to do (computeRelativePoseRobustGN / computeRelativePoseGN, src/mapHandler.cpp:4677-5068
/ :4413-4675), the generator's margins for the candidates the GPU tests use, and the C ABI's
presence and layout. No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import lcpose_cases as cases
import oracle_api as oa
import ref_lcpose as R
from plba import capi, lcpose

HTH = 1e-7
H_FD = 1e-5   # expmap_se3 drops rotations below 1e-6 rad: the difference step stays above it


def _left_perturbed(T, k, h):
    d = np.zeros(6)
    d[k] = h
    return R.mat4mul(oa.hlm_expmap(d), T)


def _fd_rows(res_fn, T):
    """Central difference of r under a left perturbation exp(δ)·T, δ = [t; ω]."""
    cols = [(res_fn(_left_perturbed(T, k, H_FD)) - res_fn(_left_perturbed(T, k, -H_FD))) / (2 * H_FD) for k in range(6)]
    return np.stack(cols, 1)


def _candidate(fy=None):
    pr = lcpose.synth(30, 10, seed=4, rot_deg=4.0, trans=0.15, noise_px=1.0)
    cam = pr.cam if fy is None else (pr.cam[0], fy, pr.cam[2], pr.cam[3])
    T = oa.hlm_expmap(np.array([0.05, -0.02, 0.03, 0.01, 0.02, -0.015]))   # some pose away from the optimum
    return pr, cam, T


def test_jacobian_row_is_the_left_perturbation_derivative_when_fx_equals_fy():
    pr, cam, T = _candidate()
    cam = (cam[0], cam[0], cam[2], cam[3])
    r, J = R.point_rows(T, pr.pt_P, pr.pt_obs, cam, HTH)
    fd = _fd_rows(lambda Tp: R.point_res(Tp, pr.pt_P, pr.pt_obs, cam)[0], T)
    # central difference: O(h²) truncation, ~1e-10 relative, plus rounding ε·r/h ~ 1e-10
    np.testing.assert_allclose(J, fd, rtol=1e-6, atol=1e-6 * np.abs(J).max())
    r, J = R.line_rows(T, pr.ln_sP, pr.ln_eP, pr.ln_le, cam, HTH)
    fd = _fd_rows(lambda Tp: R.line_res(Tp, pr.ln_sP, pr.ln_eP, pr.ln_le, cam)[0], T)
    np.testing.assert_allclose(J, fd, rtol=1e-6, atol=1e-6 * np.abs(J).max())


def test_jacobian_row_uses_fx_in_both_image_directions():
    pr, cam, T = _candidate(fy=300.0)
    fx = cam[0]
    r, dx, dy, G = R.point_res(T, pr.pt_P, pr.pt_obs, cam)
    _, J = R.point_rows(T, pr.pt_P, pr.pt_obs, cam, HTH)
    # the formula of :4719-4730 written out per match, fx throughout
    for k in range(len(r)):
        gx, gy, gz = G[k]
        f = fx / max(HTH, gz * gz)
        lit = np.array([f * dx[k] * gz, f * dy[k] * gz, -f * (gx * dx[k] + gy * dy[k]),
                        -f * (gx * gy * dx[k] + gy * gy * dy[k] + gz * gz * dy[k]),
                        f * (gx * gx * dx[k] + gz * gz * dx[k] + gx * gy * dy[k]),
                        f * (gx * gz * dy[k] - gy * gz * dx[k])]) / max(HTH, r[k])
        np.testing.assert_allclose(J[k], lit, rtol=1e-14, atol=0)
    fd = _fd_rows(lambda Tp: R.point_res(Tp, pr.pt_P, pr.pt_obs, cam)[0], T)
    # ... which is not the derivative once fy differs: the y translation column is off by fx/fy
    ratio = J[:, 1] / fd[:, 1]
    big = np.abs(dy) > 1.0
    assert big.sum() > 5
    np.testing.assert_allclose(ratio[big], fx / 300.0, rtol=1e-5)
    assert np.abs(J - fd).max() > 1e-2 * np.abs(fd).max()
    # lines: the same rows with the image line's normal in place of the error
    _, Jl = R.line_rows(T, pr.ln_sP, pr.ln_eP, pr.ln_le, cam, HTH)
    fdl = _fd_rows(lambda Tp: R.line_res(Tp, pr.ln_sP, pr.ln_eP, pr.ln_le, cam)[0], T)
    assert np.abs(Jl - fdl).max() > 1e-3 * np.abs(fdl).max()


def test_the_step_is_applied_on_the_right():
    pr = cases.problem(40, 12, 0.0)
    p1 = cases.params(capi.LCPOSE_GN, max_iters_first=1)
    p2 = cases.params(capi.LCPOSE_GN, max_iters_first=2)
    T1 = np.vstack([R.relative_pose(pr, p1)["T_inc"], [0, 0, 0, 1]])
    T2 = R.relative_pose(pr, p2)["T_inc"]
    rp, Jp = R.point_rows(T1, pr.pt_P, pr.pt_obs, pr.cam, HTH)
    rl, Jl = R.line_rows(T1, pr.ln_sP, pr.ln_eP, pr.ln_le, pr.cam, HTH)
    r, J = np.r_[rp, rl], np.r_[Jp, Jl]
    w = 1.0 / (1.0 + r * r)
    x = np.linalg.solve((J * w[:, None]).T @ J, J.T @ (w * r))
    E = R.inverse_se3(oa.hlm_expmap(x))
    right, left = R.mat4mul(T1, E)[:3], R.mat4mul(E, T1)[:3]
    np.testing.assert_allclose(T2, right, rtol=0, atol=1e-12)
    assert np.abs(T2 - left).max() > 1e-5


def test_converges_to_the_true_pose_on_noise_free_data():
    pr = lcpose.synth(40, 12, seed=1, rot_deg=5.0, trans=0.2, noise_px=0.0)
    out = R.relative_pose(pr, cases.params(max_iters_first=20, max_iters=20))
    # expmap_se3 applies no rotation below 1e-6 rad, so the rotation stalls within 1e-6 of the truth
    # and the translation within 1e-6 rad times the depth of the scene (10 m)
    assert np.abs(out["T_inc"][:, :3] - pr.T_true[:3, :3]).max() <= 1e-6
    assert np.abs(out["T_inc"][:, 3] - pr.T_true[:3, 3]).max() <= 1e-5
    assert out["accepted"] == 1 and out["n_inl_pt"] == 40 and out["n_inl_ln"] == 12
    assert out["e"] < 1e-6
    # pose_inc is the inverse motion
    np.testing.assert_allclose(R.mat4mul(oa.hlm_expmap(out["pose_inc"]), np.vstack([out["T_inc"], [0, 0, 0, 1]])),
                               np.eye(4), atol=1e-9)


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_outlier_flags_on_a_generated_set(variant):
    pr = cases.problem(300, 100, 0.25)
    ref = cases.reference(300, 100, 0.25, variant)
    assert pr.pt_outlier.sum() == 75 and pr.ln_outlier.sum() == 25
    assert np.array_equal(ref["pt_inlier"].astype(bool), ~pr.pt_outlier)
    assert np.array_equal(ref["ln_inlier"].astype(bool), ~pr.ln_outlier)
    assert (ref["n_inl_pt"], ref["n_inl_ln"]) == (225, 75)


def test_variant_gn_differs_from_robust_gn_as_listed():
    pr = cases.problem(40, 12, 0.25)
    rob, gn = cases.reference(40, 12, 0.25, capi.LCPOSE_ROBUST_GN), cases.reference(40, 12, 0.25, capi.LCPOSE_GN)
    # no refinement loop: GN ends where RobustGN's first loop ends
    assert gn["iters_ref"] == 0 and rob["iters_ref"] > 0
    rob0 = R.relative_pose(pr, cases.params(capi.LCPOSE_ROBUST_GN, max_iters=0))
    for k in ("T_inc", "H", "x_inc", "pt_inlier", "ln_inlier"):
        assert np.array_equal(rob0[k], gn[k]), k
    assert rob0["e"] == gn["e"] and not np.array_equal(rob["T_inc"], gn["T_inc"])
    # pose_inc: logmap(inverse(expmap(x_inc))) against logmap(inverse(T_inc))
    T4 = np.vstack([gn["T_inc"], [0, 0, 0, 1]])
    assert np.array_equal(gn["pose_inc"], oa.hlm_logmap(R.inverse_se3(T4)))
    assert np.array_equal(rob["pose_inc"], oa.hlm_logmap(R.inverse_se3(oa.hlm_expmap(rob["x_inc"]))))
    # lc_inl: tested by GN, forced true by RobustGN (39 of 52 matches are inliers)
    strict = dict(lc_inl=0.9)
    a = R.relative_pose(pr, cases.params(capi.LCPOSE_ROBUST_GN, **strict))
    b = R.relative_pose(pr, cases.params(capi.LCPOSE_GN, **strict))
    assert a["conditions"] & 4 and a["accepted"] == 1
    assert not (b["conditions"] & 4) and b["conditions"] | 4 == 31 and b["accepted"] == 0


def test_err_prev_is_carried_into_the_refinement():
    # with err_prev reset, the refinement's first pass could never stop on |e − err_prev| < ε; carried
    # over from a converged first loop on outlier-free data (the inlier set does not change) it does
    pr = lcpose.synth(40, 12, seed=1, rot_deg=5.0, trans=0.2, noise_px=0.0)
    out = R.relative_pose(pr, cases.params(max_iters_first=30, max_iters=10))
    assert out["iters_first"] < 30 and out["iters_ref"] == 1


def test_singular_and_empty_candidates_are_rejected():
    for shape in (cases.SINGULAR_SHAPE, cases.EMPTY_SHAPE):
        for v in cases.VARIANTS:
            out = R.relative_pose(cases.problem(*shape), cases.params(v))
            assert out["accepted"] == 0
    assert np.array_equal(R.relative_pose(cases.problem(0, 0), cases.params())["T_inc"], np.eye(4)[:3])


@pytest.mark.parametrize("n_pt,n_ln,frac,variant", cases.parity_cases())
def test_generator_margins_of_the_gpu_fixtures(n_pt, n_ln, frac, variant):
    """Every decision of the candidates the GPU tests compare is far from its threshold: a rounding
    difference between two summation orders cannot flip it."""
    for caps in ((5, 10), (3, 2)):
        p = cases.params(variant, max_iters_first=caps[0], max_iters=caps[1])
        m = R.margins(cases.problem(n_pt, n_ln, frac), p)
        assert m["outlier"] > 1e-6, m
        for k in ("e", "unc", "t", "r_deg"):
            assert m[k] > 1e-6, (k, m)


def _ids(cs):
    return [c.name for c in cs]


def _margins_ok(pr, p):
    m = R.margins(pr, p)
    return all(m[k] > 1e-6 for k in ("outlier", "e", "unc", "t", "r_deg")), m


@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("case", cases.MARGIN_CASES, ids=_ids(cases.MARGIN_CASES))
def test_generator_margins_of_the_candidates_away_from_the_defaults(case, variant):
    ok, m = _margins_ok(case.problem(), case.params(variant))
    assert ok, m
    ref = case.reference(variant)
    if case.prm and dict(case.prm).get("lc_inl"):   # the inlier share is a decision of GN too
        share = (ref["n_inl_pt"] + ref["n_inl_ln"]) / (case.n_pt + case.n_ln)
        assert abs(share - dict(case.prm)["lc_inl"]) > 1e-6
    # the full runs of the clamp cases are compared only because they are well conditioned
    assert np.linalg.cond(ref["H"]) <= 1e6


@pytest.mark.parametrize("case", cases.ONE_PASS_CASES, ids=_ids(cases.ONE_PASS_CASES))
def test_generator_margins_of_one_pass_from_the_identity(case):
    ok, m = _margins_ok(case.problem(), case.params(capi.LCPOSE_GN, **cases.ONE_PASS))
    assert ok, m


@pytest.mark.parametrize("case,robust,gn", cases.REJECTED, ids=_ids([c for c, _, _ in cases.REJECTED]))
def test_each_accept_condition_fails_alone(case, robust, gn):
    """conditions: 1 e < lc_res | 2 unc < lc_unc | 4 inlier share > lc_inl (GN; forced in RobustGN) |
    8 t < lc_trs | 16 r_deg < lc_rot."""
    a, b = case.reference(capi.LCPOSE_ROBUST_GN), case.reference(capi.LCPOSE_GN)
    assert (a["conditions"], b["conditions"]) == (robust, gn)
    assert a["accepted"] == int(robust == 31) and b["accepted"] == int(gn == 31)
    for ref in (a, b):   # a pose was reached: the rejection is the threshold's, not a failed run's
        assert ref["n_inl_pt"] + ref["n_inl_ln"] >= 39 and np.isfinite(ref["unc"])


def _unpermuted(o, ip, il):
    o = dict(o)
    for k, idx in (("pt_inlier", ip), ("ln_inlier", il)):
        a = np.zeros_like(o[k])
        a[idx] = o[k]
        o[k] = a
    return o


def test_one_pass_bar_is_a_hundred_times_the_checkers_own_reordering_noise():
    """The largest relative difference of H and e between the checker's one pass and its pass over the
    same features in three other orders, over every one-pass candidate: 1.218e-15 measured (plain
    elementwise arithmetic, the same on every machine); the device's tree over 256 partial sums matches no serial order, hence the factor 100."""
    worst = 0.0
    for case in cases.ONE_PASS_CASES:
        ref = case.reference(capi.LCPOSE_GN, **cases.ONE_PASS)
        for seed in (1, 2, 3):
            q, ip, il = cases.permuted(case.problem(), seed)
            o = _unpermuted(R.relative_pose(q, case.params(capi.LCPOSE_GN, **cases.ONE_PASS)), ip, il)
            assert np.array_equal(o["pt_inlier"], ref["pt_inlier"]) and np.array_equal(o["ln_inlier"], ref["ln_inlier"])
            fig = cases.one_pass_figures(o, ref)
            worst = max(worst, fig["H"], fig["e"])
            assert fig["T_inc"] <= cases.ONE_PASS_BAR, (case.name, fig)   # the bar times cond₂(H) holds for the step
    print("one pass, reordering noise", worst)
    assert 100.0 * worst <= cases.ONE_PASS_BAR <= 101.0 * worst, worst


@pytest.mark.parametrize("variant", cases.VARIANTS)
def test_noise_free_run_stagnates_at_the_same_pass_in_any_feature_order(variant):
    """|e − err_prev| < ε ends both loops below their caps, and the count does not depend on the
    summation order."""
    case = cases.STAGNATION
    ref = case.reference(variant)
    n_ref = 1 if variant == capi.LCPOSE_ROBUST_GN else 0
    assert 5 < ref["iters_first"] < 30 and ref["iters_ref"] == n_ref and ref["e"] > 100 * R.EPS
    for seed in range(1, 6):
        q, _, _ = cases.permuted(case.problem(), seed)
        o = R.relative_pose(q, case.params(variant))
        assert (o["iters_first"], o["iters_ref"]) == (ref["iters_first"], ref["iters_ref"]), seed
    # the deciding differences are far from ε on the scale of e's own rounding (e ~ 8e-8, so ~1e-22):
    # |e14 − e13| = 7.3e-17 = ε/3 stops the loop, |e13 − e12| = 5.7e-15 = 26 ε did not
    n = ref["iters_first"]
    e = [R.relative_pose(case.problem(), case.params(capi.LCPOSE_GN, max_iters_first=k))["e"] for k in (n - 2, n - 1, n)]
    assert abs(e[2] - e[1]) < 0.5 * R.EPS and abs(e[1] - e[0]) > 10.0 * R.EPS, e


def test_exact_observations_at_the_identity_stop_on_the_first_pass():
    for variant in cases.VARIANTS:
        ref = cases.AT_IDENTITY.reference(variant)
        assert ref["iters_first"] == 1 and ref["e"] < R.EPS
        assert np.array_equal(ref["T_inc"], np.eye(4)[:3])
        assert not ref["x_inc"].any() and not ref["pose_inc"].any()   # logmap_se3's arm for θ <= 1e-6


def test_both_sides_of_both_clamps_occur():
    def first_pass(case):
        pr = case.problem()
        r_pt, _, _, G = R.point_res(np.eye(4), pr.pt_P, pr.pt_obs, pr.cam)
        r_ln, _, _, Gs, Ge = R.line_res(np.eye(4), pr.ln_sP, pr.ln_eP, pr.ln_le, pr.cam)
        return np.r_[r_pt, r_ln], np.r_[G[:, 2], Gs[:, 2], Ge[:, 2]] ** 2, dict(case.prm)["homog_th"]
    # fmax(homog_th, r) on the first pass of the small motion: (below, above)
    r, z2, hth = first_pass(cases.CLAMP_R_SMALL)
    assert ((r < hth).sum(), (r > hth).sum()) == (12, 40) and (z2 > hth).all()
    # ... and on the last pass of the ordinary scene, whose first pass is all above
    r, z2, hth = first_pass(cases.CLAMP_R)
    assert (r > hth).all() and (z2 > hth).all()
    for v in cases.VARIANTS:
        ref = cases.CLAMP_R.reference(v)
        res = np.r_[ref["out_res_pt"], ref["out_res_ln"]]
        assert (res < hth).sum() >= 5 and (res > hth).sum() >= 5
    # fmax(homog_th, gz²) on the first pass of the scene at a tenth of its size
    r, z2, hth = first_pass(cases.CLAMP_Z)
    assert ((z2 < hth).sum(), (z2 > hth).sum()) == (24, 40)


@pytest.mark.parametrize("case", cases.FEW, ids=_ids(cases.FEW))
def test_few_feature_candidates_agree_with_their_reordered_runs_within_a_tenth_of_each_bar(case):
    for variant in cases.VARIANTS:
        ref = case.reference(variant)
        assert 1e3 <= np.linalg.cond(ref["H"]) <= 1e6
        for seed in (0, 1, 2):
            q, ip, il = cases.permuted(case.problem(), seed)
            o = _unpermuted(R.relative_pose(q, case.params(variant)), ip, il)
            assert np.array_equal(o["pt_inlier"], ref["pt_inlier"]) and np.array_equal(o["ln_inlier"], ref["ln_inlier"])
            fig = cases.parity_figures(o, ref)
            assert max(fig.values()) <= 0.1, (variant, seed, fig)


@pytest.mark.parametrize("case", cases.RANK_DEFICIENT, ids=_ids(cases.RANK_DEFICIENT))
def test_rank_deficient_candidates_are_rejected_on_the_uncertainty(case):
    for variant in cases.VARIANTS:
        ref = case.reference(variant)
        assert ref["accepted"] == 0 and not (ref["conditions"] & 2)
        assert np.linalg.cond(ref["H"]) > 1e15


def test_a_point_behind_the_camera_is_an_ordinary_outlier():
    pr, k = cases.BEHIND.problem(), cases.BEHIND.mirror
    assert (pr.T_true[:3, :3] @ pr.pt_P[k] + pr.T_true[:3, 3])[2] < -1.0
    for variant in cases.VARIANTS:
        ref = cases.BEHIND.reference(variant)
        assert ref["accepted"] == 1 and np.isfinite(ref["out_res_pt"]).all()
        assert not ref["pt_inlier"][k] and ref["n_inl_pt"] == 39 and ref["n_inl_ln"] == 12


def test_a_point_with_zero_depth_gives_a_nan_step_and_a_rejection():
    """Defined here, where the reference is not: a non-finite H or g gives a NaN x and no exception.
    Every comparison with NaN is then false: no stop test holds, both loops run to their caps, no match
    is an outlier (‖e‖ > sqrt(7.815) is false), e and t fail their tests and r_deg = 0 passes."""
    pr = cases.ZERO_DEPTH.problem()
    assert pr.pt_P[cases.ZERO_DEPTH.zero_z, 2] == 0.0
    assert np.isnan(R.qr_solve(np.full((6, 6), np.nan), np.ones(6))).all()
    assert np.isnan(R.qr_solve(np.eye(6), np.r_[np.inf, np.zeros(5)])).all()
    for variant in cases.VARIANTS:
        ref = cases.ZERO_DEPTH.reference(variant)
        assert ref["accepted"] == 0 and ref["conditions"] == 4 | 16
        assert (ref["iters_first"], ref["iters_ref"]) == (5, 10 if variant == capi.LCPOSE_ROBUST_GN else 0)
        assert ref["pt_inlier"].all() and ref["ln_inlier"].all() and np.isnan(ref["T_inc"]).all()
        assert ref["unc"] == np.inf and np.isnan(ref["e"])


def test_generator_outliers_are_gross_and_noise_is_bounded():
    pr = cases.problem(300, 100, 0.25)
    T = pr.T_true
    r_pt = R.point_res(T, pr.pt_P, pr.pt_obs, pr.cam)[0]
    assert r_pt[~pr.pt_outlier].max() <= 1.0 + 1e-9 and r_pt[pr.pt_outlier].min() >= lcpose.OUTLIER_MIN_PX
    r_ln, ds, de, _, _ = R.line_res(T, pr.ln_sP, pr.ln_eP, pr.ln_le, pr.cam)
    assert np.abs(np.r_[ds, de][np.r_[~pr.ln_outlier, ~pr.ln_outlier]]).max() <= 1.0 + 1e-9
    assert np.minimum(np.abs(ds), np.abs(de))[pr.ln_outlier].min() >= lcpose.OUTLIER_MIN_PX
    np.testing.assert_allclose(pr.ln_le[:, 0] ** 2 + pr.ln_le[:, 1] ** 2, 1.0, rtol=1e-14)


def test_library_exports_and_struct_layout():
    from plba import lib
    L = C.CDLL(lib.LIB_PATH)
    assert hasattr(L, "plba_lc_relative_pose") and hasattr(L, "plba_lcpose_default_params")
    assert {"plba_lc_relative_pose", "plba_lcpose_default_params"} <= set(lib.EXPORTED)
    # include/plba.h: int32 + pad, 7 pointers, 4 doubles | 6 doubles, 4 int32 | 6 int32, 4 + 60 doubles
    assert C.sizeof(capi.PlbaLcposeBatch) == 8 + 7 * 8 + 4 * 8
    assert C.sizeof(capi.PlbaLcposeParams) == 6 * 8 + 4 * 4
    assert C.sizeof(capi.PlbaLcposeOut) == 6 * 4 + 64 * 8
    assert capi.PlbaLcposeOut.e.offset == 24 and capi.PlbaLcposeOut.H.offset == 24 + (4 + 6 + 6 + 12) * 8
    p = capi.PlbaLcposeParams()
    L.plba_lcpose_default_params.argtypes = [C.POINTER(capi.PlbaLcposeParams)]
    L.plba_lcpose_default_params.restype = None
    L.plba_lcpose_default_params(C.byref(p))
    d = capi.lcpose_params()
    for name, _ in capi.PlbaLcposeParams._fields_:
        assert getattr(p, name) == getattr(d, name), name
    assert (p.homog_th, p.max_iters_first, p.max_iters, p.lc_res, p.lc_unc, p.lc_inl, p.lc_trs, p.lc_rot, p.variant) == \
        (1e-7, 5, 10, 1.0, 0.01, 0.3, 1.5, 35.0, 0)
