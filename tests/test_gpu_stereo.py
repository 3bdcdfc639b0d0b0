"""plba_stereo_associate on the device against its checker (tests/ref_stereo.py), bit for bit: counts, source
indices, descriptor rows and every double; batch against single calls; the matcher's unchanged results with
the four-half-width window; the workspace; the refusals; and the host mirror's device route."""
import ctypes as C

import numpy as np
import pytest

import gridmatch_cases as gcases
import mapmatch_cases as mc
import ref_stereo as RS
import stereo_cases as SC
import test_host_mapmatch as thm
from plba import capi
from plba.lib import PlbaError, Solver
from plba.slam_map import HostMap

pytestmark = pytest.mark.gpu

_want = {}


def want(name, best_lr, pluker):
    """The checker's result, computed once per (case, flags) and never changed."""
    key = (name, best_lr, pluker)
    if key not in _want:
        _want[key] = RS.associate(SC.case(name), prm(best_lr, pluker))
    return _want[key]


def prm(best_lr=1, pluker=1, **kw):
    return RS.params(**SC.CAMERA, best_lr=best_lr, pluker=pluker, **kw)


@pytest.fixture(scope="module")
def solver():
    with Solver(device=0) as s:
        yield s


@pytest.mark.parametrize("pluker", [0, 1])
@pytest.mark.parametrize("best_lr", [0, 1])
@pytest.mark.parametrize("name", list(SC.CASES))
def test_parity_with_checker(solver, name, best_lr, pluker):
    got = solver.stereo_associate([SC.case(name)], prm(best_lr, pluker))[0]
    assert RS.same(want(name, best_lr, pluker), got) is None


def test_window_is_asymmetric_on_the_device(solver):
    """The hand case: a decoy at Hamming distance 0 one cell to the right / one row below the query cell must
    not be chosen over the partner at distance 1 in the window. Any reuse of a symmetric ws fails here."""
    frames = SC.asymmetric_window_frames()
    p = RS.params(**SC.HAND_CAMERA)
    for got in [solver.stereo_associate([f], p)[0] for f in frames] + solver.stereo_associate(frames, p):
        assert got["n_pt"] == 1 and got["pt_src"].tolist() == [0] and got["pt_disp"].tolist() == [10.0]
        assert got["pt_P"].tolist() == [[0.125 / 10.0 * 8.0, 0.125 / 10.0 * 8.0, 0.125 / 10.0 * 512.0]]


def test_batch_equals_single_calls(solver):
    names = ["mixed", "pts_70x70", "lines_40x40"]   # three unequal frames
    got = solver.stereo_associate([SC.case(n) for n in names], prm())
    for n, g in zip(names, got):
        assert RS.same(want(n, 1, 1), g) is None, n
        assert RS.same(solver.stereo_associate([SC.case(n)], prm())[0], g) is None, n


def test_grid_match_unchanged(solver):
    """plba_grid_match passes ws for all four half-widths: its cases still equal ref_gridmatch."""
    cases = gcases.parity_cases() + gcases.boundary_cases()
    for best_lr in (True, False):
        for c in cases:   # one call per case: the cases differ in desc_bytes
            m12, cnt = solver.grid_match([gcases.problem(*c)], gcases.COLS, gcases.ROWS, best_lr)[0]
            w12, wcnt = gcases.reference(*c, best_lr)
            assert np.array_equal(m12, w12) and cnt == wcnt, c


def test_leaves_uploaded_window_intact(solver):
    from plba import synth
    g = synth.generate("C1L")
    solver.upload(g)
    first = solver.lba_plucker()
    solver.upload(g)
    assert RS.same(want("mixed", 1, 1), solver.stereo_associate([SC.case("mixed")], prm())[0]) is None
    second = solver.lba_plucker()
    for k in ("kf_Tcw", "pt_xyz", "ln_orth"):
        assert np.array_equal(first[k], second[k]), k


def test_smaller_batch_after_larger_reuses_scratch():
    with Solver(device=0) as s:
        s.stereo_associate([SC.case(n) for n in ("pts_300x130", "lines_40x40", "mixed")], prm())
        after = s.stereo_associate([SC.case("mixed")], prm())[0]
    with Solver(device=0) as fresh:
        alone = fresh.stereo_associate([SC.case("mixed")], prm())[0]
    assert RS.same(alone, after) is None and RS.same(want("mixed", 1, 1), after) is None


def _refused(solver, frames, params=None, desc_bytes=None, patch=None):
    bv = capi.StereoBatchView(frames, desc_bytes)
    if patch:
        patch(bv)
    with pytest.raises(PlbaError):
        solver.stereo_associate(bv, params or prm())


def test_refusals_leave_the_context_usable(solver):
    f = SC.case("mixed")

    def with_coord(key, value):
        g = {k: np.array(v) for k, v in f.items()}
        g[key][3, 1] = value
        return g
    _refused(solver, [with_coord("pt_l", np.nan)])
    _refused(solver, [with_coord("ls_r", np.inf)])
    _refused(solver, [with_coord("pt_r", 2.0 * SC.HEIGHT + 1.0)])     # beyond one image size outside
    _refused(solver, [with_coord("ls_l", -SC.HEIGHT - 1.0)])

    def negative_offset(bv):
        bv.off["pt_r"][0] = -1
    _refused(solver, [f], patch=negative_offset)
    d6 = {k: (np.zeros((len(v), 6), np.uint8) if "desc" in k else v) for k, v in f.items()}
    _refused(solver, [d6], desc_bytes=6)
    big = dict(pt_l=np.ones((1, 2), np.float32), pdesc_l=np.zeros((1, 32), np.uint8),
               pt_r=np.ones((65536, 2), np.float32), pdesc_r=np.zeros((65536, 32), np.uint8))
    _refused(solver, [big])
    assert RS.same(want("mixed", 1, 1), solver.stereo_associate([f], prm())[0]) is None


def test_mirror_device_route_equals_cpu_hook():
    built = mc.build(seed=3)
    f, p = SC.case("mixed"), prm()
    w = want("mixed", 1, 1)
    kf = built[0].keyframes[mc.KF_NEW]
    kf.pt_idx, kf.ls_idx = [-1] * w["n_pt"], [-1] * w["n_ls"]
    got = []
    for hook in ("cpu", None):
        h = HostMap(built[0])
        h.set_stereo_fn(hook)
        r = h.set_keyframe_stereo(mc.KF_NEW, f, p)
        assert np.array_equal(r["pt_src"], w["pt_src"]) and np.array_equal(r["ls_src"], w["ls_src"])
        for i, L in enumerate(built[1]):
            h.set_line_geometry(i, L, np.zeros(3))
        h.set_camera(*mc.CAM, mc.WIDTH, mc.HEIGHT)
        h.set_grid_match_fn("cpu")
        h.set_match_fn(lambda b, m12, cnt: h.L.plslam_desc_match_cpu(None, C.byref(b), m12, cnt))
        st = h.match_map_to_kf(mc.KF_NEW, built[3])
        st.pop("match_ms", None)
        got.append((st, thm.state(h, built[0])))
        h.close()
    assert got[0] == got[1]
