"""plba_map_associate on the device against the checker tests/ref_mapassoc.py: every count, index, flag and
double, bit for bit; and the host mirror's one-call route on the device against the same with the CPU hook."""
import numpy as np
import pytest

import mapassoc_cases as MC
import mapmatch_cases as mc
import ref_mapassoc as RM
import test_host_mapassoc as TH
import test_host_mapmatch as TM
import test_mapassoc_oracle as TO
from plba import capi, synth
from plba.lib import PlbaError, Solver
from plba.slam_map import HostMap, SlamParams, make_map, mapassoc_params

pytestmark = pytest.mark.gpu

prm, want, MODES = TO.prm, TO.want, TO.MODES


@pytest.fixture(scope="module")
def solver():
    with Solver(device=0) as s:
        yield s


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(MC.CASES))
def test_parity_with_checker(solver, name, mode):
    """best_lr 0 and 1, the grid and brute force alone; 10 / 11 visible points and 6 / 7 visible lines; more than 64
    features, more than 256 candidates; empty sides; invisible rows interleaved throughout."""
    assert RM.same(want(name, mode), solver.map_associate([MC.case(name)], prm(**MODES[mode]))[0]) is None


def test_branches_on_the_device(solver):
    TO.test_branches_are_reached(lambda name, mode: solver.map_associate([MC.case(name)], prm(**MODES[mode]))[0])


@pytest.mark.parametrize("name, kf, over", TH.hand_cases(), ids=[c[0] for c in TH.hand_cases()])
def test_hand_cases_on_the_device(solver, name, kf, over):
    """The hand rows, the visibility boundary, both acceptance tests on either side, and the masking cases in
    the grid stage and in the fallback."""
    assert RM.same(RM.associate(kf, prm(**over)), solver.map_associate([kf], prm(**over))[0]) is None


def test_an_invisible_nearest_row_is_inert_on_the_device(solver):
    p = MC.masking_keyframe()
    for q in (prm(), prm(fast_matching=0, min_pt_matches=1)):
        got = solver.map_associate([p], q)[0]
        assert got["pt_m12"].tolist() == [-1, 0, -1] and got["pt_accepted"].tolist() == [0, 1, 0]
        assert RM.same(RM.associate(p, q, see_invisible=True), got) is not None


def test_batch_equals_single_calls(solver):
    names = ["mixed", "pts_300x130", "lines_40x70"]   # three unequal keyframes
    got = solver.map_associate([MC.case(n) for n in names], prm())
    for n, g in zip(names, got):
        assert RM.same(want(n, "default"), g) is None, n
        assert RM.same(solver.map_associate([MC.case(n)], prm())[0], g) is None, n


def test_empty_sides_inside_a_batch(solver):
    """A keyframe with candidates and no features, and with features and no candidates, between two others."""
    names = ["mixed", "empty_sides", "pts_far"]
    for mode in ("default", "brute_force"):
        got = solver.map_associate([MC.case(n) for n in names], prm(**MODES[mode]))
        for n, g in zip(names, got):
            assert RM.same(want(n, mode), g) is None, (n, mode)


def test_smaller_batch_after_larger_reuses_scratch():
    with Solver(device=0) as s:
        s.map_associate([MC.case(n) for n in ("pts_300x130", "lines_40x70", "mixed")], prm())
        after = s.map_associate([MC.case("pts_far")], prm())[0]
    assert RM.same(want("pts_far", "default"), after) is None


def test_leaves_uploaded_window_intact(solver):
    g = synth.generate("C1L")
    solver.upload(g)
    first = solver.lba_plucker()
    solver.upload(g)
    assert RM.same(want("mixed", "default"), solver.map_associate([MC.case("mixed")], prm())[0]) is None
    second = solver.lba_plucker()
    for k in ("kf_Tcw", "pt_xyz", "ln_orth"):
        assert np.array_equal(first[k], second[k]), k


@pytest.mark.parametrize("name, kfs, patch, over, db", TH.refusals(), ids=[r[0] for r in TH.refusals()])
def test_refusals(solver, name, kfs, patch, over, db):
    bv = capi.MapassocBatchView(kfs, db)
    if patch:
        patch(bv)
    with pytest.raises(PlbaError):
        solver.map_associate(bv, prm(**over))


def test_context_usable_after_refusals(solver):
    with pytest.raises(PlbaError):
        solver.map_associate([MC.case("mixed")], prm(ws=-1))
    assert solver.map_associate([], prm()) == []
    assert RM.same(want("mixed", "default"), solver.map_associate([MC.case("mixed")], prm())[0]) is None


@pytest.mark.parametrize("kw", [dict(), dict(ws=0, min_pt_matches=40, min_ls_matches=22), dict(fast_matching=0)])
def test_mirror_device_route_equals_cpu_hook(kw):
    built = mc.build()
    dev, cpu = TH.assoc_hostmap(built, hook=None), TH.assoc_hostmap(built)
    a = dev.match_map_to_kf_assoc(mc.KF_NEW, built[3], mapassoc_params(**kw))
    b = cpu.match_map_to_kf_assoc(mc.KF_NEW, built[3], mapassoc_params(**kw))
    a.pop("match_ms"), b.pop("match_ms")
    assert a == b and a["accepted"][0] >= 15 and a["accepted"][1] >= 5
    assert TM.state(dev, built[0]) == TM.state(cpu, built[0])
    assert dev.check_incremental_gather()


def test_local_mapping_step_from_the_keyframes_features():
    m = make_map(synth.generate("C1L", fixed_frac=0.3), seed=25)
    m.max_kf_idx = len(m.keyframes) - 1 + 5
    kf = len(m.keyframes) - 1
    row = m.full_graph[-1, :-1].astype(np.int64)
    h = HostMap(m, params=SlamParams(min_lm_obs=4, min_lm_cov_graph=int(np.median(row)) + 1, min_kf_local_map=2))
    rng = np.random.default_rng(3)
    n_pt, n_ls = len(m.keyframes[kf].pt_idx), len(m.keyframes[kf].ls_idx)
    spl = rng.uniform([0, 0], [640, 480], (n_ls, 2))
    h.set_keyframe_features(kf, rng.integers(0, 256, (n_pt, 32), dtype=np.uint8), rng.normal(size=(n_pt, 3)) + [0, 0, 5],
                            rng.uniform([0, 0], [640, 480], (n_pt, 2)), rng.integers(0, 256, (n_ls, 32), dtype=np.uint8),
                            rng.normal(size=(n_ls, 3)) + [0, 0, 5], rng.normal(size=(n_ls, 3)) + [0, 0, 5],
                            rng.normal(size=(n_ls, 3)))
    h.set_keyframe_line_endpoints(kf, spl, spl + rng.uniform(-60, 60, (n_ls, 2)))
    h.set_camera(m.fx, m.fy, m.cx, m.cy, 640, 480)
    st = h.local_mapping_step_kf_assoc(kf, mapassoc_params())
    assert st["n_free_kf"] > 0 and st["n_ept"] > 0 and st["iters"][0] > 0
    assert st["match"]["unmatched"][0] >= 1
    assert h.check_incremental_gather()
