"""C++ host mirror of MapHandler::localBundleAdjustment() (src/mapHandler.cpp:1392-1502) and the
write-back of levMarquardtOptimizationLBA (:2841-2882): plslam_local_ba / HostMap.local_ba_endpoints.

The CPU tests drive it through the solver hook with a prescribed X; the GPU test runs the default
solver (plba_hlm_lba, variant PLBA_HLM_LBA_ENDPOINTS) and compares with Solver.hlm_lba on the
window the mirror gathered."""
import numpy as np
import pytest

from plba import capi, synth
from plba import geometry as geo
from plba.hlm import HlmWindow, lba_window
from plba.slam_map import HostMap, make_map

from test_host_mirror import graph_from_struct


def _arr(p, n):
    return np.ctypeslib.as_array(p, shape=(n,)).copy() if n and p else np.zeros(0)   # (NULL: not handed over)


def _put(p, a):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if a.size:
        np.ctypeslib.as_array(p, shape=(a.size,))[:] = a


def endpoint_map(cfg="C1L", **kw):
    """A SlamMap in endpoint-line form: image-line observations (a, b, c, 0), line3D per line."""
    win = lba_window(synth.generate(cfg, **kw))
    m = make_map(win.graph)
    hmap = HostMap(m)
    for l in m.lines:
        hmap.set_line_geometry(l.idx, win.ln_line3d[l.idx], np.zeros(3))
    return win, m, hmap


def hook(record, answer=None, rc=0):
    """Solver hook: records the window; answers with answer(win) -> dict(kf_x, pt_xyz, ln_line3d)."""
    def fn(gs, ss, ps, rs):
        g = graph_from_struct(gs)
        win = HlmWindow(g, _arr(ss.kf_x, 6 * g.n_kf).reshape(-1, 6), _arr(ss.ln_pluker, 6 * g.n_ln).reshape(-1, 6),
                        _arr(ss.ln_line3d, 6 * g.n_ln).reshape(-1, 6))
        record["win"], record["variant"], record["max_iters"] = win, ps.variant, ps.max_iters
        if rc or answer is None:
            return rc or -7
        out = record["out"] = answer(win)
        assert bool(rs.ln_line3d) or g.n_ln == 0
        _put(rs.kf_x, out["kf_x"])
        _put(rs.pt_xyz, out["pt_xyz"])
        _put(rs.ln_line3d, out["ln_line3d"])
        rs.linearizations, rs.solves, rs.accepted = 3, 3, 2
        rs.err, rs.lambda_ = 1.5, 2.5
        return 0
    return fn


def prescribed(win):
    """X with every other landmark moved by just under / just over the 0.01 threshold."""
    g = win.graph
    x = win.kf_x.copy()
    x[g.kf_fixed == 0] += 0.01 * np.arange(1, 7)
    d3 = np.array([2.0, -1.0, 2.0]) / 3.0                         # unit vectors
    d6 = np.array([1.0, -1.0, 1.0, 1.0, -1.0, 1.0]) / np.sqrt(6.0)
    sp = np.where(np.arange(g.n_pt) % 2 == 0, 0.0099, 0.0101)
    sl = np.where(np.arange(g.n_ln) % 2 == 0, 0.0101, 0.0099)
    return dict(kf_x=x, pt_xyz=g.pt_xyz + sp[:, None] * d3, ln_line3d=win.ln_line3d + sl[:, None] * d6)


def test_window_and_writeback_with_a_prescribed_x():
    win0, m, hmap = endpoint_map()
    hmap.set_hlm_params(capi.hlm_params(max_iters=9))             # the variant is forced, the rest kept
    rec = {}
    hmap.set_hlm_solver(hook(rec, prescribed))
    xs = {k.kf_idx: hmap.keyframe_x(k.kf_idx) for k in m.keyframes if k is not None}
    st = hmap.local_ba_endpoints()
    assert st["ret"] == 0 and rec["variant"] == capi.HLM_LBA_ENDPOINTS and rec["max_iters"] == 9
    assert (st["linearizations"], st["solves"], st["accepted"], st["err"], st["lambda_"]) == (3, 3, 2, 1.5, 2.5)
    win, g, out = rec["win"], rec["win"].graph, rec["out"]
    # the gather (:1395-1493): free = local && kf_idx != 0, every other observer fixed
    kf_list = [k for k in m.keyframes if k is not None and k.local and k.kf_idx != 0]
    pts = [p for p in m.points if p is not None and p.local]
    lns = [l for l in m.lines if l is not None and l.local]
    free = g.kf_fixed == 0
    assert list(g.kf_id[free]) == [k.kf_idx for k in kf_list] and 0 in list(g.kf_id[~free])
    for i, kid in enumerate(g.kf_id):
        np.testing.assert_allclose(g.kf_Tcw[i], geo.inverse_se3(m.keyframes[kid].T_kf_w)[:3, :], rtol=0, atol=1e-14)
        np.testing.assert_array_equal(win.kf_x[i], xs[kid])
    np.testing.assert_array_equal(g.pt_xyz, np.array([p.pos for p in pts]))
    np.testing.assert_array_equal(win.ln_line3d, win0.ln_line3d[[l.idx for l in lns]])
    assert g.n_ept == sum(len(p.kf_obs_list) for p in pts) == st["n_pt_obs"]
    assert g.n_eln == sum(len(l.kf_obs_list) for l in lns) == st["n_ls_obs"]
    np.testing.assert_array_equal(g.eln_obs, np.concatenate([np.array(l.obs_list) for l in lns]))
    assert np.all(g.eln_obs[:, 3] == 0)
    # the write-back (:2841-2882)
    after = hmap.read(m)
    for i, k in enumerate(kf_list):
        np.testing.assert_allclose(after.keyframes[k.kf_idx].T_kf_w, geo.expmap_se3(out["kf_x"][i]), rtol=0, atol=1e-14)
    free_ids = {k.kf_idx for k in kf_list}
    for k in m.keyframes:
        if k is not None and k.kf_idx not in free_ids:
            np.testing.assert_array_equal(after.keyframes[k.kf_idx].T_kf_w, k.T_kf_w)
        if k is not None:
            np.testing.assert_array_equal(hmap.keyframe_x(k.kf_idx), xs[k.kf_idx])   # x_kf_w is never written
    for i, p in enumerate(pts):
        q = after.points[p.idx]
        np.testing.assert_array_equal(q.pos, out["pt_xyz"][i])
        assert q.inlier == (i % 2 == 0)                     # 0.0099 stays an inlier, 0.0101 does not
    for i, l in enumerate(lns):
        l3d, _ = hmap.line_geometry(l.idx)
        np.testing.assert_array_equal(l3d, out["ln_line3d"][i])
        assert after.lines[l.idx].inlier == (i % 2 == 1)
        np.testing.assert_array_equal(after.lines[l.idx].pos, l.pos)      # NDw is not this function's
    assert st["pt_outliers"] == len(pts) // 2 and st["ln_outliers"] == (len(lns) + 1) // 2
    # nothing else moved: non-local landmarks, observations (the removal loop of :2884-3006 is a no-op)
    for lms_b, lms_a in ((m.points, after.points), (m.lines, after.lines)):
        for b, a in zip(lms_b, lms_a):
            if b is None:
                continue
            assert a.kf_obs_list == b.kf_obs_list and len(a.obs_list) == len(b.obs_list)
            if not b.local:
                np.testing.assert_array_equal(a.pos, b.pos)
                assert a.inlier == b.inlier
    np.testing.assert_array_equal(after.full_graph, m.full_graph)
    hmap.close()


def test_vo_inserting_kf_returns_minus_one_and_writes_nothing():
    win0, m, hmap = endpoint_map()
    hmap.set_hlm_params(None, vo_inserting_kf=True)
    rec = {}
    hmap.set_hlm_solver(hook(rec, prescribed))
    st = hmap.local_ba_endpoints()
    assert st["ret"] == -1 and "out" in rec                 # the optimiser ran (:2841 is after the loop)
    after = hmap.read(m)
    for b, a in zip(m.keyframes, after.keyframes):
        np.testing.assert_array_equal(a.T_kf_w, b.T_kf_w)
    for b, a in zip(m.points, after.points):
        if b is not None:
            np.testing.assert_array_equal(a.pos, b.pos)
            assert a.inlier == b.inlier
    for l in m.lines:
        np.testing.assert_array_equal(hmap.line_geometry(l.idx)[0], win0.ln_line3d[l.idx])
        assert after.lines[l.idx].inlier == l.inlier
    hmap.close()


def test_no_observations_returns_minus_one_without_a_solve():
    win0, m, hmap = endpoint_map("C1")
    hmap.close()
    for lm in m.points + m.lines:
        if lm is not None:
            lm.local = False
    hmap = HostMap(m)
    rec = {}
    hmap.set_hlm_solver(hook(rec, prescribed))
    st = hmap.local_ba_endpoints()
    assert st["ret"] == -1 and "win" not in rec
    after = hmap.read(m)
    for b, a in zip(m.keyframes, after.keyframes):
        np.testing.assert_array_equal(a.T_kf_w, b.T_kf_w)
    hmap.close()


def test_the_plucker_function_is_untouched_by_the_shared_body():
    """localBundleAdjustmentForPluker still hands the optimiser orthNDw / NDw and its own variant."""
    m = make_map(synth.generate("C1L"))
    hmap = HostMap(m)
    rec = {}
    hmap.set_hlm_solver(hook(rec, None))
    with pytest.raises(Exception):
        hmap.local_ba_hlm()
    g = rec["win"].graph
    assert rec["variant"] == capi.HLM_LBA_PLUCKER
    lns = [l for l in m.lines if l is not None and l.local]
    np.testing.assert_array_equal(rec["win"].ln_pluker, np.array([l.pos for l in lns]))
    np.testing.assert_allclose(g.ln_orth, geo.pluker_to_orth(np.array([l.pos for l in lns])), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(g.eln_obs, np.concatenate([np.array(l.obs_list) for l in lns]))
    hmap.close()


@pytest.mark.gpu
def test_gpu_default_solver_equals_solver_hlm_lba_on_the_gathered_window():
    from plba.lib import Solver
    win0, m, probe = endpoint_map()
    rec = {}
    probe.set_hlm_solver(hook(rec, None))                   # capture the window; the hook fails
    with pytest.raises(Exception):
        probe.local_ba_endpoints()
    probe.close()
    win = rec["win"]
    p = capi.lba_params()
    with Solver() as s:
        s.upload(win.graph)
        out = s.hlm_lba(win, p)
    _, _, hmap = endpoint_map()
    st = hmap.local_ba_endpoints()                          # plba_hlm_lba through the mirror
    assert st["ret"] == 0
    assert (st["linearizations"], st["solves"], st["accepted"]) == (out["linearizations"], out["solves"], out["accepted"])
    assert (st["err"], st["lambda_"]) == (out["err"], out["lam"])
    assert out["accepted"] >= 2
    after = hmap.read(m)
    g = win.graph
    for i, pid in enumerate(g.pt_id):
        np.testing.assert_array_equal(after.points[pid].pos, out["pt_xyz"][i])
    for i, lid in enumerate(g.ln_id):
        np.testing.assert_array_equal(hmap.line_geometry(lid)[0], out["ln_line3d"][i])
    for i, kid in enumerate(g.kf_id):
        if not g.kf_fixed[i]:
            np.testing.assert_allclose(after.keyframes[kid].T_kf_w, geo.expmap_se3(out["kf_x"][i]), rtol=0, atol=1e-14)
    hmap.close()
