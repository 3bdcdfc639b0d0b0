"""The numpy checker of the frame-to-frame pose (tests/ref_trackpose.py) pinned by hand-computed values,
finite differences and named cases, and the margins of every case the GPU tests use
(tests/trackpose_cases.py): each decision has to stay further from its threshold than the rounding by
which a tree sum and a match-order sum differ. A case that fails its margin gets another seed in
trackpose_cases.py; it is never skipped on the GPU."""
import numpy as np
import pytest

import ref_trackpose as rt
import trackpose_cases as cases
from plba import capi

model_param = pytest.mark.parametrize("model", cases.MODELS, ids=cases.MODEL_IDS)
F32 = np.float32


# ---- vector_stdv_mad / vector_mean_stdv_mad (src2/auxiliar.cpp:387-460)
def test_stdv_mad_known_values():
    assert rt.vector_stdv_mad([]) == 0.0                                   # n = 0
    assert rt.vector_stdv_mad([3.5]) == 0.0                                # n = 1: the deviation of the median from itself
    # n = 2: element 1 is the median (the upper one), deviations {1, 0}, element 1 of the sorted {0, 1}
    assert rt.vector_stdv_mad([1.0, 2.0]) == 1.4826 * 1.0
    # odd n: median 3, deviations {2, 1, 0, 1, 6} -> sorted {0, 1, 1, 2, 6}, element 2
    assert rt.vector_stdv_mad([1.0, 2.0, 3.0, 4.0, 9.0]) == 1.4826 * 1.0
    # even n: element 2 of {1, 2, 4, 8} is 4 (not the mean 3), deviations {3, 2, 0, 4} -> {0, 2, 3, 4}, element 2
    assert rt.vector_stdv_mad([8.0, 1.0, 4.0, 2.0]) == 1.4826 * 3.0
    # ties: the median lies in a run of equal values and so does the MAD
    assert rt.vector_stdv_mad([2.0, 2.0, 2.0, 5.0, 5.0, 1.0, 1.0]) == 1.4826 * 1.0


def test_stdv_mad_rounds_the_deviation_through_float():
    # 0.1 is not a float: fabsf(1.1 - 1.0) is float(0.1) = 0.100000001490116..., not the double 0.1
    d = rt.vector_stdv_mad([1.0, 1.0, 1.1])          # median 1.0, deviations {0, 0, f32(0.1)} -> element 1 = 0
    assert d == 0.0
    d = rt.vector_stdv_mad([0.9, 1.0, 1.1, 1.2])     # median 1.1: {f(0.2), f(0.1), 0, f(0.1)} -> element 2
    assert d == 1.4826 * float(F32(1.1 - 1.0)) and d != 1.4826 * (1.1 - 1.0)
    # a pair that differs only below float precision (as floats both are 1.0f): the DIFFERENCE is taken in
    # double and then rounded, so it is float(b - a), neither 0 nor the double b - a
    a, b = 1.0, 1.00000005
    assert F32(a) == F32(b) and float(F32(b - a)) != b - a
    # n = 2: the median is b (element 1), deviations {f(b - a), 0} -> element 1 of the sorted pair
    assert rt.vector_stdv_mad([a, b]) == 1.4826 * float(F32(b - a))
    assert rt.vector_stdv_mad([a, a, b, b]) == 1.4826 * float(F32(b - a))
    big = 1.0e8
    assert rt.vector_stdv_mad([big, big, big + 1.0, big + 3.0]) == 1.4826 * 1.0   # the DIFFERENCE is rounded, not the terms


def test_mean_stdv_mad_both_mean_branches():
    mean, stdv = rt.vector_mean_stdv_mad([])
    assert (mean, stdv) == (0.0, 0.0)
    # stdv = 1.4826, best samples r < 2.9652: {1, 2}; k = 2 >= int(0.2 * 5) = 1 -> their mean
    mean, stdv = rt.vector_mean_stdv_mad([1.0, 2.0, 3.0, 4.0, 9.0])
    assert stdv == 1.4826 and mean == 1.5
    # MAD = 0 (more than half equal): no sample is below 2 * 0, k = 0 < int(0.2 * 10) = 2 -> the mean of all
    res = [5.0] * 8 + [1.0, 9.0]
    mean, stdv = rt.vector_mean_stdv_mad(res)
    assert stdv == 0.0 and mean == 5.0
    # n = 2: median 2, deviations {1, 0} -> MAD 1; both below 2.9652
    mean, stdv = rt.vector_mean_stdv_mad([1.0, 2.0])
    assert stdv == 1.4826 and mean == 1.5
    # n = 1: MAD 0, k = 0 >= int(0.2) = 0 -> 0 / 0
    mean, stdv = rt.vector_mean_stdv_mad([4.0])
    assert stdv == 0.0 and np.isnan(mean)


# ---- lineSegmentOverlap (src2/stereoFrame.cpp:547-653)
@pytest.mark.parametrize("so,eo,axis", [((10.0, 0.0), (10.5, 100.0), 1),     # vertical: |dx| < 1, y compared
                                        ((0.0, 20.0), (100.0, 20.5), 0)])    # horizontal: |dy| < 1, x compared
def test_overlap_degenerate_branches_and_their_five_cases(so, eo, axis):
    def seg(a, b):
        s, e = [3.0, 3.0], [4.0, 4.0]
        s[axis], e[axis] = a, b
        return s, e
    assert rt.line_segment_overlap(so, eo, *seg(-10.0, 110.0)) == 1.0        # covers it
    assert rt.line_segment_overlap(so, eo, *seg(-30.0, -10.0)) == 0.0        # before it
    assert rt.line_segment_overlap(so, eo, *seg(120.0, 150.0)) == 0.0        # after it
    assert rt.line_segment_overlap(so, eo, *seg(-20.0, 25.0)) == 0.25        # starts before
    assert rt.line_segment_overlap(so, eo, *seg(75.0, 130.0)) == 0.25        # ends after
    assert rt.line_segment_overlap(so, eo, *seg(25.0, 75.0)) == 0.5          # inside
    assert rt.line_segment_overlap(so, eo, *seg(75.0, 25.0)) == 0.5          # the order of the endpoints does not matter


def test_overlap_general_branch_projects_onto_the_line():
    so, eo = (0.0, 0.0), (100.0, 100.0)
    # the foot of (30, 10) on y = x is (20, 20), of (70, 90) it is (80, 80): lambdas 0.2 and 0.8
    assert abs(rt.line_segment_overlap(so, eo, (30.0, 10.0), (70.0, 90.0)) - 0.6) < 1e-15
    assert rt.line_segment_overlap(so, eo, (-50.0, -50.0), (150.0, 150.0)) == 1.0
    assert rt.line_segment_overlap(so, eo, (-50.0, -50.0), (-10.0, -10.0)) == 0.0
    assert abs(rt.line_segment_overlap(so, eo, (-50.0, -50.0), (25.0, 25.0)) - 0.25) < 1e-15
    assert abs(rt.line_segment_overlap(so, eo, (75.0, 75.0), (150.0, 150.0)) - 0.25) < 1e-15


# ---- TransformForPluker and the projected-line residual
def test_transform_for_pluker_moves_the_line_of_two_points():
    rng = np.random.default_rng(0)
    p, q = rng.normal(size=3) + (0, 0, 5), rng.normal(size=3) + (0, 0, 5)
    ND = np.concatenate([np.cross(p, q), q - p])
    T = np.eye(4)
    T[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])   # 90 degrees about z
    T[:3, 3] = (0.5, -0.25, 2.0)
    p2, q2 = T[:3, :3] @ p + T[:3, 3], T[:3, :3] @ q + T[:3, 3]
    exp = np.concatenate([np.cross(p2, q2), q2 - p2])
    assert np.allclose(rt.transform_for_pluker(T, ND), exp, rtol=0, atol=1e-12)
    # a hand value: the x axis through (0, 1, 0) has N = (0,1,0) x (1,0,0) = (0, 0, -1); moved by t = (0, 0, 3)
    # with R = I it passes through (0, 1, 3): N' = (0,1,3) x (1,0,0) = (0, 3, -1)
    T = np.eye(4)
    T[2, 3] = 3.0
    assert np.array_equal(rt.transform_for_pluker(T, np.array([0, 0, -1.0, 1, 0, 0])), np.array([0, 3.0, -1.0, 1, 0, 0]))


def test_pluker_residual_is_the_distance_of_the_pixels_to_the_projected_line():
    cam = (400.0, 300.0, 320.0, 240.0)
    p, q = np.array([-1.0, 0.5, 4.0]), np.array([2.0, 1.0, 5.0])
    ND = np.concatenate([np.cross(p, q), q - p])
    proj = lambda P: np.array([cam[2] + cam[0] * P[0] / P[2], cam[3] + cam[1] * P[1] / P[2]])
    a, b = proj(p), proj(q)
    r, e0, e1, l, _, _ = rt.pluker_res(np.eye(4), ND, np.concatenate([a, b]), cam)
    assert abs(e0) < 1e-9 and abs(e1) < 1e-9                        # its own projections lie on it
    n = np.array([-(b - a)[1], (b - a)[0]]) / np.linalg.norm(b - a)
    r, e0, e1, l, _, _ = rt.pluker_res(np.eye(4), ND, np.concatenate([a + 3.0 * n, b - 4.0 * n]), cam)
    assert abs(abs(e0) - 3.0) < 1e-9 and abs(abs(e1) - 4.0) < 1e-9 and e0 * e1 < 0 and abs(r - 5.0) < 1e-9


@model_param
def test_the_rows_are_the_gradient_of_the_residual(model):
    """J_aux is d‖e‖/dξ for the left perturbation DT <- expmap(ξ)·DT (what the update on the left inverts),
    up to fx standing in for fy in the endpoint rows: central differences with fx = fy. The Plücker row's
    rotation block is the reference's −(R·N)^ − t^·(R·D)^ (:744-746), which is the derivative only where
    t = 0 (it should be −(R·N + t×R·D)^): kept as it is, so that model is differentiated at t = 0."""
    import oracle_api as oa
    import ref_lcpose as rl
    cam = (400.0, 400.0, 320.0, 240.0)
    pr = cases.tp.synth(0, 6, seed=9, cam=cam, noise_px=3.0)
    T = np.eye(4)
    if model == rt.ENDPOINTS:
        T[:3, 3] = (0.02, -0.01, 0.03)
    h = 1e-6
    for k in range(6):
        if model == rt.PLUCKER:
            r, e0, e1, l, RN, RD = rt.pluker_res(T, pr.ln_NDc[k], pr.ln_obs[k], cam)
            J = rt.pluker_row(T, pr.ln_obs[k], cam, 1e-7, r, e0, e1, l, RN, RD)
            f = lambda Tx: rt.pluker_res(Tx, pr.ln_NDc[k], pr.ln_obs[k], cam)[0]
        else:
            r, J = (a[0] for a in rl.line_rows(T, pr.ln_sP[k:k + 1], pr.ln_eP[k:k + 1], pr.ln_le[k:k + 1], cam, 1e-7))
            f = lambda Tx: rl.line_res(Tx, pr.ln_sP[k:k + 1], pr.ln_eP[k:k + 1], pr.ln_le[k:k + 1], cam)[0][0]
        num = np.zeros(6)
        for i in range(6):
            x = np.zeros(6)
            x[i] = h
            num[i] = (f(rl.mat4mul(oa.hlm_expmap(x), T)) - f(rl.mat4mul(oa.hlm_expmap(-x), T))) / (2 * h)
        assert np.allclose(J, num, rtol=1e-5, atol=1e-5 * np.abs(num).max()), (k, J, num)


# ---- the branches, by named cases
@model_param
@pytest.mark.parametrize("branch", sorted(cases.BRANCH), ids=[cases.BRANCH[b].name for b in sorted(cases.BRANCH)])
def test_each_branch_is_reached(branch, model):
    ref = cases.BRANCH[branch].reference(model)
    assert ref["branch"] == branch
    if branch == capi.TRACK_OK:
        pr = cases.BRANCH[branch].problem()
        assert np.abs(np.linalg.inv(ref["DT"]) - pr.T_true).max() < 5e-3        # it estimates the motion
        assert np.array_equal(ref["pt_inlier"] == 0, pr.pt_outlier) and np.array_equal(ref["ln_inlier"] == 0, pr.ln_outlier)
        assert np.allclose(ref["DT_solver"] @ ref["DT"], np.eye(4), atol=1e-9)  # DT is the inverse of the solver's
        assert np.array_equal(ref["DT_cov_eig"], np.sort(ref["DT_cov_eig"]))
    else:
        assert ref["err_norm"] == -1.0 and np.array_equal(ref["DT"], np.eye(4)) and not ref["DT_cov"].any()
    if branch == capi.TRACK_FINAL_NOT_GOOD:
        assert ref["iters_ref"] == 1 and np.array_equal(ref["DT_solver"], np.eye(4))
    if branch == capi.TRACK_FIRST_NOT_GOOD:
        assert (ref["iters_first"], ref["iters_ref"]) == (1, 1 if model == rt.ENDPOINTS else 0)


@model_param
def test_the_refinement_starts_from_the_initial_pose(model):
    """With one refinement pass the solver's DT is one step from the identity, not from the first loop's DT_."""
    case = cases.BRANCH[capi.TRACK_OK]
    one = rt.track_pose(case.problem(), case.params(model, max_iters_ref=1))
    first = rt.track_pose(case.problem(), case.params(model, max_iters=1, max_iters_ref=1, has_points=0, has_lines=0))
    assert one["iters_ref"] == 1 and one["iters_first"] > 1
    # without removal both loops see the same matches at the same pose: one step each, the same DT
    assert np.array_equal(first["DT_solver"], rt.track_pose(case.problem(), case.params(
        model, max_iters=1, max_iters_ref=1, has_points=0, has_lines=0, min_features=1))["DT_solver"])
    assert np.abs(one["DT_solver"] - np.eye(4)).max() > 1e-4


@model_param
def test_motion_model(model):
    acc, rej = cases.MOTION_ACCEPTED.reference(model), cases.MOTION_REJECTED.reference(model)
    plain = rt.track_pose(cases.MOTION_REJECTED.problem(), cases.MOTION_REJECTED.params(model, use_motion_model=0))
    assert all(np.array_equal(rej[k], plain[k]) for k in ("DT", "DT_solver", "H", "DT_cov", "pt_inlier", "ln_inlier"))
    assert acc["branch"] == capi.TRACK_OK and not np.array_equal(acc["DT_solver"], plain["DT_solver"])


@model_param
def test_z_zero_is_not_good(model):
    ref = cases.Z0.reference(model)
    assert ref["branch"] != capi.TRACK_OK and ref["err_norm"] == -1.0 and not np.isfinite(ref["H"]).all()


@model_param
@pytest.mark.parametrize("case", cases.PROBES, ids=[c.name for c in cases.PROBES])
def test_the_probes_see_one_pass_and_no_clamp(case, model):
    ref = case.reference(model)
    assert ref["iters_first"] == 1 and ref["iters_ref"] <= 1
    assert rt.TH_MIN < ref["s_p"] < rt.TH_MAX and rt.TH_MIN < ref["s_l"] < rt.TH_MAX


# ---- the margins of every case used on the GPU
@model_param
@pytest.mark.parametrize("case", cases.GPU_CASES, ids=[c.name for c in cases.GPU_CASES])
def test_every_decision_keeps_its_margin(case, model):
    m = cases.margins(case, model)
    print(case.name, m)
    assert m["inlier"] > cases.MARGIN_PX, m
    assert m["stop"] > cases.MARGIN_REL, m
    assert m["good"] > cases.MARGIN_REL, m
