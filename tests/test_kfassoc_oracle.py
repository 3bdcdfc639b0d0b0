"""plslam_kf_assoc_cpu (the restatement of plba_kf_associate) against the checker tests/ref_kfassoc.py, bit
for bit, and the hand cases with their numbers written out. Runs without a GPU."""
import numpy as np
import pytest

import kfassoc_cases as KC
import ref_kfassoc as RK
from plba import capi, slam_map
from plba.slam_map import PlbaError


def prm(**kw):
    return RK.params(**{**KC.CAMERA, **kw})


# the parameter sets of the parity run: the grid with either line query, brute force alone, no cross-check
MODES = {
    "default": dict(),
    "grid_units": dict(line_query_in_grid_units=1),
    "no_best_lr": dict(best_lr=0, line_query_in_grid_units=1),
    "brute_force": dict(fast_matching=0),
    "brute_force_no_best_lr": dict(fast_matching=0, best_lr=0),
}
_want = {}
# 10 rows a side without the grid: the fallback's strict condition leaves the problem without a match
NO_MATCH = {("pts_at_min", "brute_force"), ("pts_at_min", "brute_force_no_best_lr")}


def want(name, mode):
    """The checker's result, computed once per (case, mode) and never changed."""
    if (name, mode) not in _want:
        _want[name, mode] = RK.associate(KC.case(name), prm(**MODES[mode]))
    return _want[name, mode]


def assert_not_vacuous(name, w):
    p = KC.case(name)
    for kd, (a, b) in enumerate((("pdesc_p", "pdesc_c"), ("ldesc_p", "ldesc_c"))):
        if len(p.get(a, ())) and len(p.get(b, ())):
            assert w["n_matches"][kd] >= 1, (name, kd)


def line_classes(w, pair):
    """(created, extended, rejected) rows of a line result, as the sequential part will class them."""
    m, new, rej = w["ls_m12"] >= 0, np.asarray(pair["ls_new"]).reshape(-1) != 0, w["ls_rejected"] != 0
    return int((m & new & ~rej).sum()), int((m & ~new & ~rej).sum()), int((m & rej).sum())


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(KC.CASES))
def test_cpu_equals_checker(name, mode):
    w = want(name, mode)
    if (name, mode) not in NO_MATCH:
        assert_not_vacuous(name, w)
    got = slam_map.kf_assoc_cpu([KC.case(name)], prm(**MODES[mode]))[0]
    assert RK.same(w, got) is None


def cpu(name, mode):
    return slam_map.kf_assoc_cpu([KC.case(name)], prm(**MODES[mode]))[0]


def test_line_cases_create_extend_and_reject():
    tot, got = np.zeros(3, int), np.zeros(3, int)
    for name in ("lines_40x40", "mixed"):
        for mode in ("default", "grid_units"):
            tot += line_classes(want(name, mode), KC.case(name))
            got += line_classes(cpu(name, mode), KC.case(name))
    assert (tot > 0).all() and (got == tot).all(), (tot, got)


def test_branches_are_reached(result=None):
    """The facts hold of the checker's result, and of ``result(name, mode)``: the restatement's here."""
    for want in (globals()["want"], result or cpu):
        _branches(want)


def _branches(want):
    assert want("mixed", "grid_units")["fallback"] == (0, 0) and min(want("mixed", "grid_units")["n_grid"]) >= 10
    w = want("mixed", "default")   # the pixel-unit line query finds nothing: only the line problem falls back
    assert w["fallback"] == (0, 1) and w["n_grid"][1] == 0 and w["n_matches"][1] > 0
    assert want("mixed", "brute_force")["fallback"] == (1, 1) and want("mixed", "brute_force")["n_grid"] == (0, 0)
    # the fallback's condition is strict: 10 rows against min_pt_matches = 10 never fall back, 11 do
    assert want("pts_at_min", "brute_force")["fallback"] == (0, 0) and want("pts_at_min", "brute_force")["n_matches"] == (0, 0)
    assert want("pts_above_min", "brute_force")["fallback"] == (1, 0) and want("pts_above_min", "brute_force")["n_matches"][0] > 0


def test_point_record_by_hand():
    """Identity poses: P3d = P1, dir_prev = P1 / |P1|, dir_curr = P2 / |P2|. (3, 4, 12) has norm 13."""
    p = KC.identity_poses()
    d = np.full((1, KC.DB), 0x33, np.uint8)
    u, v = 320.0 + 500.0 * 3.0 / 12.0, 240.0 + 480.0 * 4.0 / 12.0
    p.update(pt_P_p=[[3.0, 4.0, 12.0]], pdesc_p=d, pt_pl_c=[[u, v], [10.0, 10.0]], pt_P_c=[[6.0, 8.0, 24.0], [0, 0, 1.0]],
             pdesc_c=np.vstack([d, ~d]))
    for got in (RK.associate(p, prm()), slam_map.kf_assoc_cpu([p], prm())[0]):
        assert got["pt_m12"].tolist() == [0] and got["n_grid"] == (1, 0) and got["fallback"] == (0, 0)
        assert got["pt_rec"][0].tolist() == [3.0, 4.0, 12.0] + [3.0 / 13.0, 4.0 / 13.0, 12.0 / 13.0] + \
            [6.0 / 26.0, 8.0 / 26.0, 24.0 / 26.0]


def test_pixel_unit_line_query():
    """The line through pixels (100, 100) - (140, 100) has no grid candidate as the reference queries it (pixel
    coordinates as cells) and its partner with line_query_in_grid_units; one row is below min_ls_matches, so
    there is no fallback either way. An implementation that scales fails the default."""
    p = KC.pixel_unit_pair()
    for fn in (RK.associate, lambda q, r: slam_map.kf_assoc_cpu([q], r)[0]):
        got = fn(p, prm())
        assert got["ls_m12"].tolist() == [-1] and got["n_grid"] == (0, 0) and got["fallback"] == (0, 0)
        assert not got["ls_rec"].any() and got["ls_rejected"].tolist() == [0]
        got = fn(p, prm(line_query_in_grid_units=1))
        assert got["ls_m12"].tolist() == [0] and got["n_grid"] == (0, 1) and got["ls_rejected"].tolist() == [0]
        # the 3-D line runs along x: the unit direction is exact; both errors vanish up to rounding (the
        # segments are the line's own projections: 40 px long, coordinates of a few hundred, 2^-52 relative)
        assert got["ls_rec"][0, 3:6].tolist() == [1.0, 0.0, 0.0] and got["ls_rec"][0, 0] == 0.0
        assert 0.0 <= got["ls_rec"][0, 6] < 1e-9 and 0.0 <= got["ls_rec"][0, 7] < 1e-9


@pytest.mark.parametrize("is_new", [1, 0])
@pytest.mark.parametrize("norm, rejected", [(2.0, 0), (3.0, 1)])
def test_line_gate_either_side(is_new, norm, rejected):
    """|err_curr| about 2.0 px and 3.0 px around sqrt(5.991) = 2.4477, for a new row and for one that takes ls_lm_NDw."""
    p = KC.gate_pair(is_new, norm)
    w = RK.associate(p, prm(line_query_in_grid_units=1))
    got = slam_map.kf_assoc_cpu([p], prm(line_query_in_grid_units=1))[0]
    assert RK.same(w, got) is None
    assert w["ls_m12"].tolist() == [0] and w["ls_rejected"].tolist() == [rejected]
    assert abs(w["ls_rec"][0, 7] - norm) < 0.05
    if is_new:
        assert w["ls_rec"][0, 6] < 1e-6 and abs(np.linalg.norm(w["ls_rec"][0, 3:6]) - 1.0) < 1e-12
    else:
        assert not w["ls_rec"][0, :7].any()


def test_behind_camera_rows_take_the_sentinel_cell_and_the_fallback():
    p, a, b = KC.behind_camera_pair()
    w = RK.associate(p, prm())
    assert w["fallback"][0] == 1 and w["pt_m12"][a] >= 0 and w["pt_m12"][b] >= 0   # matched by the fallback
    DT = RK.f64(p["DT"])
    u, v = RK.project(prm(), DT, RK.f64(p["pt_P_p"][b]))
    assert RK.cell(u * 0.1, v * 0.1) == (RK.NO_CELL, RK.NO_CELL)   # z = 0: not finite
    assert RK.same(w, slam_map.kf_assoc_cpu([p], prm())[0]) is None
    # with a minimum that the grid alone reaches, the two rows stay unmatched: their window is empty
    g = RK.associate(p, prm(min_pt_matches=3))
    assert g["fallback"][0] == 0 and g["pt_m12"][b] == -1 and g["n_grid"][0] >= 3
    assert RK.same(g, slam_map.kf_assoc_cpu([p], prm(min_pt_matches=3))[0]) is None


def test_two_previous_rows_on_one_current_row():
    p = KC.two_on_one_pair()
    w = RK.associate(p, prm(best_lr=0))
    assert w["pt_m12"].tolist() == [0, 0]
    assert RK.same(w, slam_map.kf_assoc_cpu([p], prm(best_lr=0))[0]) is None
    w = RK.associate(p, prm(best_lr=1))   # the cross-check keeps the first only (equal distance: no new record)
    assert w["pt_m12"].tolist() == [0, -1]
    assert RK.same(w, slam_map.kf_assoc_cpu([p], prm(best_lr=1))[0]) is None


def test_batch_equals_single_calls():
    names = ["mixed", "pts_70x70", "empty_side"]
    got = slam_map.kf_assoc_cpu([KC.case(n) for n in names], prm())
    for n, g in zip(names, got):
        assert RK.same(want(n, "default"), g) is None, n


def test_c_defaults_are_those_of_the_checker():
    p = capi.kfassoc_params()
    for k, v in RK.DEFAULTS.items():
        assert getattr(p, k) == v, k
    for k in ("width", "height", "fx", "fy", "cx", "cy"):
        assert getattr(p, k) == 0


def refusals():
    """(name, pairs -> (view patch or None), params overrides, desc_bytes)"""
    f = KC.case("mixed")

    def with_value(key, idx, value):
        g = {k: np.array(v) for k, v in f.items()}
        g[key][idx] = value
        return g
    big = dict(KC.identity_poses(), pt_P_p=np.ones((1, 3)), pdesc_p=np.zeros((1, 32), np.uint8),
               pt_pl_c=np.ones((65536, 2)), pt_P_c=np.ones((65536, 3)), pdesc_c=np.zeros((65536, 32), np.uint8))

    def negative_offset(bv):
        bv.off["pt_c"][0] = -1

    def decreasing_offset(bv):
        bv.off["ls_p"][1] = -2

    def null_array(bv):
        bv.struct.ls_NDc_p = None
    d6 = {k: (np.zeros((len(v), 6), np.uint8) if "desc" in k else v) for k, v in f.items()}
    return [
        ("nan current point", [with_value("pt_pl_c", (3, 1), np.nan)], None, {}, None),
        ("inf current line", [with_value("ls_epl_c", (2, 0), np.inf)], None, {}, None),
        ("current point beyond one image size", [with_value("pt_pl_c", (0, 1), 2.0 * KC.HEIGHT + 1.0)], None, {}, None),
        ("current line beyond one image size", [with_value("ls_spl_c", (0, 0), -KC.WIDTH - 1.0)], None, {}, None),
        ("DT not finite", [with_value("DT", (1, 3), np.nan)], None, {}, None),
        ("T_prev not finite", [with_value("T_prev", (0, 0), np.inf)], None, {}, None),
        ("Tcw_curr not finite", [with_value("Tcw_curr", (2, 2), np.nan)], None, {}, None),
        ("negative offset", [f], negative_offset, {}, None),
        ("decreasing offset", [f], decreasing_offset, {}, None),
        ("NULL array with rows", [f], null_array, {}, None),
        ("desc_bytes 6", [d6], None, {}, 6),
        ("65536 current rows", [big], None, {}, None),
        ("ws < 0", [f], None, dict(ws=-1), None),
        ("no image size", [f], None, dict(width=0), None),
        ("no grid", [f], None, dict(cols=0), None),
    ]


@pytest.mark.parametrize("name, pairs, patch, over, db", refusals(), ids=[r[0] for r in refusals()])
def test_kf_assoc_cpu_refusals(name, pairs, patch, over, db):
    bv = capi.KfassocBatchView(pairs, db)
    if patch:
        patch(bv)
    with pytest.raises(PlbaError):
        slam_map.kf_assoc_cpu(bv, prm(**over))


def test_empty_batch_is_ok():
    assert slam_map.kf_assoc_cpu([], prm()) == []
