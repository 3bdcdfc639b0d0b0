"""plba_kf_associate on the device against the checker tests/ref_kfassoc.py: every count, index, flag and
double, bit for bit."""
import numpy as np
import pytest

import kfassoc_cases as KC
import ref_kfassoc as RK
import test_host_kfmatch as TH
import test_kfassoc_oracle as TO
from plba import capi
from plba.lib import PlbaError, Solver

pytestmark = pytest.mark.gpu

prm, want, MODES = TO.prm, TO.want, TO.MODES


@pytest.fixture(scope="module")
def solver():
    with Solver(device=0) as s:
        yield s


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(KC.CASES))
def test_parity_with_checker(solver, name, mode):
    """best_lr 0 and 1, the grid with either line query, brute force alone; the sizes at min_pt_matches and
    one above; a pair with an empty side."""
    w = want(name, mode)
    if (name, mode) not in TO.NO_MATCH:
        TO.assert_not_vacuous(name, w)
    assert RK.same(w, solver.kf_associate([KC.case(name)], prm(**MODES[mode]))[0]) is None


def test_branches_on_the_device(solver):
    """No fallback with enough grid matches; only the line problem falls back; brute force alone."""
    TO.test_branches_are_reached(lambda name, mode: solver.kf_associate([KC.case(name)], prm(**MODES[mode]))[0])
    tot = np.zeros(3, int)
    for name in ("lines_40x40", "mixed"):
        for mode in ("default", "grid_units"):
            tot += TO.line_classes(solver.kf_associate([KC.case(name)], prm(**MODES[mode]))[0], KC.case(name))
    assert (tot > 0).all(), tot   # created, extended and rejected line rows


@pytest.mark.parametrize("is_new", [1, 0])
@pytest.mark.parametrize("norm, rejected", [(2.0, 0), (3.0, 1)])
def test_line_gate_either_side_on_the_device(solver, is_new, norm, rejected):
    """|err_curr| about 2.0 px and 3.0 px around sqrt(5.991), for a new row and for one that takes ls_lm_NDw."""
    p = KC.gate_pair(is_new, norm)
    got = solver.kf_associate([p], prm(line_query_in_grid_units=1))[0]
    assert RK.same(RK.associate(p, prm(line_query_in_grid_units=1)), got) is None
    assert got["ls_m12"].tolist() == [0] and got["ls_rejected"].tolist() == [rejected] and abs(got["ls_rec"][0, 7] - norm) < 0.05
    assert bool(got["ls_rec"][0, :7].any()) == bool(is_new)


def test_behind_camera_rows(solver):
    p, _, b = KC.behind_camera_pair()
    for over in (dict(), dict(min_pt_matches=3)):
        w = RK.associate(p, prm(**over))
        assert RK.same(w, solver.kf_associate([p], prm(**over))[0]) is None
    assert w["pt_m12"][b] == -1   # min 3: the grid stands, and the row in the plane z = 0 has an empty window


def test_pixel_unit_line_query_on_the_device(solver):
    p = KC.pixel_unit_pair()
    got = solver.kf_associate([p], prm())[0]
    assert got["ls_m12"].tolist() == [-1] and got["n_grid"] == (0, 0) and got["fallback"] == (0, 0)
    got = solver.kf_associate([p], prm(line_query_in_grid_units=1))[0]
    assert got["ls_m12"].tolist() == [0] and got["n_grid"] == (0, 1)
    assert RK.same(RK.associate(p, prm(line_query_in_grid_units=1)), got) is None


def test_two_previous_rows_on_one_current_row(solver):
    p = KC.two_on_one_pair()
    got = solver.kf_associate([p], prm(best_lr=0))[0]
    assert got["pt_m12"].tolist() == [0, 0] and RK.same(RK.associate(p, prm(best_lr=0)), got) is None


def test_batch_equals_single_calls(solver):
    names = ["mixed", "pts_70x70", "lines_40x40"]   # three unequal pairs
    got = solver.kf_associate([KC.case(n) for n in names], prm())
    for n, g in zip(names, got):
        assert RK.same(want(n, "default"), g) is None, n
        assert RK.same(solver.kf_associate([KC.case(n)], prm())[0], g) is None, n


def test_smaller_batch_after_larger_reuses_scratch():
    with Solver(device=0) as s:
        s.kf_associate([KC.case(n) for n in ("pts_300x130", "lines_40x40", "mixed")], prm())
        after = s.kf_associate([KC.case("mixed")], prm())[0]
    assert RK.same(want("mixed", "default"), after) is None


def test_leaves_uploaded_window_intact(solver):
    from plba import synth
    g = synth.generate("C1L")
    solver.upload(g)
    first = solver.lba_plucker()
    solver.upload(g)
    assert RK.same(want("mixed", "default"), solver.kf_associate([KC.case("mixed")], prm())[0]) is None
    second = solver.lba_plucker()
    for k in ("kf_Tcw", "pt_xyz", "ln_orth"):
        assert np.array_equal(first[k], second[k]), k


def test_desc_match_unchanged_by_the_gate(solver):
    """plba_desc_match runs the gated kernels without a gate: the brute-force result of the checker."""
    p = KC.case("pts_70x70")
    m12, cnt = solver.desc_match([(p["pdesc_p"], p["pdesc_c"])], [0.9], True)[0]
    w = RK.brute_force(np.asarray(p["pdesc_p"]), np.asarray(p["pdesc_c"]), 0.9, True)
    assert m12.tolist() == w and cnt == sum(i >= 0 for i in w) and cnt > 0


@pytest.mark.parametrize("name, pairs, patch, over, db", TO.refusals(), ids=[r[0] for r in TO.refusals()])
def test_refusals(solver, name, pairs, patch, over, db):
    bv = capi.KfassocBatchView(pairs, db)
    if patch:
        patch(bv)
    with pytest.raises(PlbaError):
        solver.kf_associate(bv, prm(**over))


def test_context_usable_after_refusals(solver):
    with pytest.raises(PlbaError):
        solver.kf_associate([KC.case("mixed")], prm(ws=-1))
    assert solver.kf_associate([], prm()) == []
    assert RK.same(want("mixed", "default"), solver.kf_associate([KC.case("mixed")], prm())[0]) is None


def test_mirror_device_route_equals_cpu_hook():
    built = TH.build()
    got = []
    for hooks in (True, False):
        h = TH.hostmap(built, hooks=hooks)
        if not hooks:   # the association on the device; the map half of look_for_common_matches keeps its cpu hooks
            h.set_grid_match_fn("cpu")
            h.set_match_fn(lambda b, m12, cnt: h.L.plslam_desc_match_cpu(None, TH.C.byref(b), m12, cnt))
        st = h.look_for_common_matches(TH.PREV, TH.CURR)
        st["map"].pop("match_ms")
        got.append((st, TH.state(h)))
        h.close()
    assert got[0] == got[1] and min(got[0][0]["kf"]["created"]) >= 3 and got[0][0]["kf"]["rejected"][1] >= 1


def test_a_map_grows_from_detector_output_and_the_lba_runs():
    """Three keyframes set up with set_keyframe_stereo, linked by two look_for_common_matches calls, everything on
    the device; then local_mapping_step. The map equals the one the cpu hooks build."""
    h, res = TH.three_keyframes(hooks=False)
    hc, res_c = TH.three_keyframes(hooks=True)
    for r in res + res_c:
        r["map"].pop("match_ms")
    assert res == res_c and TH.state(h) == TH.state(hc)
    assert res[0]["kf"]["created"][0] >= 10 and res[1]["kf"]["extended"][0] >= 10
    st = h.local_mapping_step(2)
    assert st["n_pt"] >= 10 and st["n_ept"] >= 2 * st["n_pt"] and st["n_free_kf"] + st["n_fixed_kf"] == 3
    h.close(), hc.close()
