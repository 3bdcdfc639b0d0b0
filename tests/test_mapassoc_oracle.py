"""The checker of plba_map_associate (tests/ref_mapassoc.py) pinned: hand-computed rows with their numbers
written out, the visibility boundary, every branch reached, the epipolar tests on either side, the margins of
every gate of every GPU case, and the two cases that make the masking of invisible rows observable. Runs
without a GPU."""
import numpy as np
import pytest

import kfassoc_cases as KC
import mapassoc_cases as MC
import ref_mapassoc as RM


def prm(**kw):
    return RM.params(**{**KC.CAMERA, **kw})


# the parameter sets of the parity runs
MODES = {
    "default": dict(),
    "no_best_lr": dict(best_lr=0),
    "brute_force": dict(fast_matching=0),
    "brute_force_no_best_lr": dict(fast_matching=0, best_lr=0),
}
_want, _margin = {}, {}


def want(name, mode):
    """The checker's result, computed once per (case, mode) and never changed."""
    if (name, mode) not in _want:
        _margin[name, mode] = RM.Margin()
        _want[name, mode] = RM.associate(MC.case(name), prm(**MODES[mode]), _margin[name, mode])
    return _want[name, mode]


def matched(w):
    return int((w["pt_m12"] >= 0).sum()), int((w["ls_m12"] >= 0).sum())


def test_hand_point_row():
    """u = 320 + 500 * 3 / 12 = 445, v = 240 + 480 * 4 / 12 = 400, cell (44, 40); err = sqrt(0.375^2 + 0.5^2) = 0.625;
    dir = P / 26 + t, the translation (1, 2, 3) added to a direction as the reference adds it."""
    p = MC.hand_point()
    u, v, z = RM.project(prm(), RM.RK.f64(p["Twf"]), RM.RK.f64(p["pt_X"][0]))
    assert (u, v, z) == (445.0, 400.0, 12.0) and (int(u * 0.1), int(v * 0.1)) == (44, 40)
    w = RM.associate(p, prm())
    assert w["pt_visible"].tolist() == [1] and w["pt_m12"].tolist() == [0] and w["pt_accepted"].tolist() == [1]
    assert w["n_visible"] == (1, 0) and w["n_grid"] == (1, 0) and w["fallback"] == (0, 0) and w["n_matches"] == (1, 0) == w["n_accepted"]
    assert w["pt_rec"][0].tolist() == [445.0, 400.0, 0.625, 6.0 / 26.0 + 1.0, 8.0 / 26.0 + 2.0, 24.0 / 26.0 + 3.0]


@pytest.mark.parametrize("le, errs, accepted", [
    ([0.0, 1.0, -400.25], (-0.25, -0.25), 1),     # below the bound
    ([0.0, -1.0, 400.25], (0.25, 0.25), 1),
    ([0.0, -1.0, 401.5], (1.5, 1.5), 0),          # above max_kf_epip_l = 1
    ([0.0, 1.0, -1400.0], (-1000.0, -1000.0), 1),  # a large negative error passes: the test is signed
    ([0.004, -1.0, 399.72], (1.5, 0.5), 0),       # one endpoint above is enough
])
def test_hand_line_row(le, errs, accepted):
    """The endpoints project to (445, 400) and (195, 400), cells (44, 40) and (19, 40) in grid units; err = le . (u, v, 1);
    mid = (3, 0, 4) / 5."""
    p = MC.hand_line(le)
    w = RM.associate(p, prm())
    assert w["ls_visible"].tolist() == [1] and w["ls_m12"].tolist() == [0] and w["ls_accepted"].tolist() == [accepted]
    assert w["ls_rec"][0, :4].tolist() == [445.0, 400.0, 195.0, 400.0]
    np.testing.assert_allclose(w["ls_rec"][0, 4:6], errs, rtol=0, atol=1e-12)
    assert w["ls_rec"][0, 6:].tolist() == [0.6, 0.0, 0.8]
    assert w["n_matches"] == (0, accepted) and w["n_grid"] == (0, 1)
    # the query cells are in grid units: in pixels, (445, 400) and (195, 400) lie outside the 64 x 48 grid and find nothing
    assert RM.associate(p, prm(ws=0))["ls_m12"].tolist() == [0]


def test_point_acceptance_either_side():
    p = MC.hand_point()
    for bound, ok in ((0.7, 1), (0.6, 0), (0.625, 0)):   # err = 0.625 exactly: the test is strict
        w = RM.associate(p, prm(max_kf_epip_p=bound))
        assert w["pt_m12"].tolist() == [0] and w["pt_accepted"].tolist() == [ok] and w["n_matches"] == (ok, 0)
        assert w["pt_rec"][0, 2] == 0.625   # a rejected row keeps its record


def test_visibility_boundary():
    p, flags = MC.boundary_points()
    w = RM.associate(p, prm())
    assert w["pt_visible"].tolist() == flags and w["n_visible"] == (sum(flags), 0)
    u, _, _ = RM.project(prm(), RM.RK.f64(p["Twf"]), RM.RK.f64(p["pt_X"][0]))
    assert u == 0.0 and RM.project(prm(), RM.RK.f64(p["Twf"]), RM.RK.f64(p["pt_X"][1]))[0] == 640.0
    u, v, z = RM.project(prm(), RM.RK.f64(p["Twf"]), RM.RK.f64(p["pt_X"][5]))
    assert 0 < u < 640 and 0 < v < 480 and z < 0   # only the depth test keeps it out
    p, flags = MC.boundary_lines()
    w = RM.associate(p, prm())
    assert w["ls_visible"].tolist() == flags and w["n_visible"] == (0, 1)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(MC.CASES))
def test_every_gate_has_a_margin(name, mode):
    """No compared quantity of a GPU case lies within 1e-9 (relative) of its threshold, so that rounding cannot
    flip a case; and the invisible rows are really there."""
    w = want(name, mode)
    m = _margin[name, mode]
    assert m.value > 1e-9, (m.value, m.where)
    for k in ("pt", "ls"):
        n = len(w[k + "_visible"])
        if n:
            assert w[k + "_visible"].sum() == n - (n + 1) // MC.INVISIBLE_EVERY
            assert (w[k + "_m12"][w[k + "_visible"] == 0] == -1).all()
            assert not w[k + "_rec"][w[k + "_m12"] < 0].any() and not w[k + "_accepted"][w[k + "_m12"] < 0].any()


def test_branches_are_reached(result=None):
    """The facts hold of the checker's result, and of ``result(name, mode)``."""
    for get in (want, result) if result else (want,):
        w = get("mixed", "default")   # the grid stands
        assert w["fallback"] == (0, 0) and w["n_grid"][0] >= 10 and w["n_grid"][1] >= 6 and matched(w) == w["n_grid"]
        assert 0 < w["n_matches"][0] < w["n_grid"][0] and 0 < w["n_matches"][1] < w["n_grid"][1]   # accepted and rejected rows
        w = get("pts_far", "default")   # only the points fall back
        assert w["fallback"] == (1, 0) and w["n_grid"][0] < 10 < w["n_visible"][0] and matched(w)[0] > w["n_grid"][0]
        w = get("lines_far", "default")   # only the lines
        assert w["fallback"] == (0, 1) and w["n_grid"][1] < 6 < w["n_visible"][1] and matched(w)[1] > w["n_grid"][1]
        w = get("mixed", "brute_force")   # fast_matching = 0
        assert w["fallback"] == (1, 1) and w["n_grid"] == (0, 0) and min(matched(w)) > 0
        # the fallback's condition is strict and reads the visible rows: 15 and 9 candidates, 10 and 6 visible
        w = get("at_min", "brute_force")
        assert w["n_visible"] == (10, 6) and w["fallback"] == (0, 0) and matched(w) == (0, 0)
        w = get("above_min", "brute_force")
        assert w["n_visible"] == (11, 7) and w["fallback"] == (1, 1) and min(matched(w)) > 0
        # more than 64 features (a second train block) and more than 256 candidates (a second tile)
        assert matched(get("pts_300x130", "default"))[0] > 64 and matched(get("pts_300x130", "brute_force"))[0] > 64
        w = get("empty_sides", "default")
        assert w["n_visible"][0] > 10 and w["fallback"] == (1, 0) and matched(w) == (0, 0)


def test_line_errors_of_the_cases_cover_the_signed_test():
    w = want("mixed", "default")
    e = w["ls_rec"][w["ls_m12"] >= 0][:, 4:6]
    acc = w["ls_accepted"][w["ls_m12"] >= 0]
    assert ((e.max(axis=1) > 2.0) & (acc == 0)).any()    # about +3: rejected
    assert ((e.min(axis=1) < -2.0) & (acc == 1)).any()   # about -3: accepted
    assert ((np.abs(e).max(axis=1) < 1.0) & (acc == 1)).any()


@pytest.mark.parametrize("stage", ["grid", "fallback"])
def test_an_invisible_nearest_row_is_inert(stage):
    """With the invisible row inert, the visible runner-up gets the match under best_lr = 1; a matcher that
    saw the invisible row would give the match to it and nothing to the runner-up."""
    p = MC.masking_keyframe()
    q = prm() if stage == "grid" else prm(fast_matching=0, min_pt_matches=1)
    w = RM.associate(p, q)
    assert w["pt_visible"].tolist() == [0, 1, 1] and w["pt_m12"].tolist() == [-1, 0, -1]
    assert w["fallback"] == ((0, 0) if stage == "grid" else (1, 0)) and w["pt_accepted"].tolist() == [0, 1, 0]
    naive = RM.associate(p, q, see_invisible=True)
    assert naive["pt_m12"].tolist() == [0, -1, -1]
    assert RM.same(w, naive) is not None


def test_two_visible_rows_on_one_feature():
    p = MC.two_on_one_keyframe()
    w = RM.associate(p, prm(best_lr=0))
    assert w["pt_visible"].tolist() == [1, 0, 1] and w["pt_m12"].tolist() == [0, -1, 0] and w["n_matches"] == (2, 0)
    w = RM.associate(p, prm(best_lr=1))   # the cross-check keeps the first only (equal distance: no new record)
    assert w["pt_m12"].tolist() == [0, -1, -1]
