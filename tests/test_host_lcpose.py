"""Host mirror of MapHandler::loopClosure() from the candidate on (src/mapHandler.cpp:4053-4116):
the inlier-ratio gate of isLoopClosure (:4384-4409), the relative pose, the loop lists and the
LC_IDLE / LC_ACTIVE / LC_READY state machine with the pose graph on LC_READY. CPU tests drive it
through the relative-pose solver hook (the numpy checker) and the pose-graph oracle hook of
tests/test_host_pgo.py; the GPU test runs the same sequence with no hooks and compares."""
import ctypes as C
import types

import numpy as np
import pytest

import lcpose_cases as cases
import parity
import ref_lcpose
from plba import capi, pgo
from plba.slam_map import LC_ACTIVE, LC_IDLE, LC_READY, HostMap
from test_host_pgo import _kf, _oracle_hook

N_LOOP, N_KF = 24, 27


def _hostmap(hooks=True, seed=3):
    m, _, _, _, line3d = pgo.loop_map(n_loop=N_LOOP, n_after=N_KF - N_LOOP, seed=seed)
    h = HostMap(m)
    for i, L in enumerate(line3d):
        h.set_line_geometry(i, L, L[:3] * 0.5)
    calls = []
    if hooks:
        h.set_lcpose_solver(_checker_hook(calls))
        h.set_pgo_solver(_oracle_hook({}))
    return h, calls


def _checker_hook(calls):
    """plba_lc_relative_pose for one candidate, by tests/ref_lcpose.py."""
    def fn(b, p, out, pin, lin):
        assert b.n == 1
        n_pt, n_ln = b.pt_off[1], b.ln_off[1]

        def arr(ptr, n, w):
            return np.ctypeslib.as_array(ptr, (n * w,)).reshape(n, w).copy() if n else np.zeros((0, w))
        prob = types.SimpleNamespace(pt_P=arr(b.pt_P, n_pt, 3), pt_obs=arr(b.pt_obs, n_pt, 2), ln_sP=arr(b.ln_sP, n_ln, 3),
                                     ln_eP=arr(b.ln_eP, n_ln, 3), ln_le=arr(b.ln_le, n_ln, 3), cam=(b.fx, b.fy, b.cx, b.cy))
        ref = ref_lcpose.relative_pose(prob, p)
        calls.append(dict(n_pt=n_pt, n_ln=n_ln, ref=ref))
        o = out[0]
        for k in ("accepted", "conditions", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln", "e", "unc", "t", "r_deg"):
            setattr(o, k, ref[k])
        for k in ("x_inc", "pose_inc", "T_inc", "H"):
            getattr(o, k)[:] = list(np.asarray(ref[k]).ravel())
        for i in range(n_pt):
            pin[i] = int(ref["pt_inlier"][i])
        for i in range(n_ln):
            lin[i] = int(ref["ln_inlier"][i])
        return 0
    return fn


def _rows(n, base):
    """lc_pt_idx / lc_ls_idx rows (idx of kf0's feature, i1, idx of kf1's feature, i2)."""
    i = np.arange(n, dtype=np.int32)
    return np.stack([base + i, i, base + 1000 + i, 2 * i], 1)


def _step(h, pr, n_feat=(100, 100, 30, 30), **kw):
    return h.loop_closure_step(pr, kf_prev_idx=0, kf_curr_idx=N_LOOP - 1, n_feat=n_feat,
                               pt_idx=_rows(pr.n_pt, 5000), ls_idx=_rows(pr.n_ln, 7000), **kw)


def test_inlier_ratio_gate():
    h, calls = _hostmap()
    pr = cases.problem(40, 12, 0.25)
    # 40 of (200, 100) points: max(20, 40) > 30; 12 of (30, 100) lines: max(40, 12) > 30
    st = _step(h, pr, n_feat=(200, 100, 30, 100))
    assert st["ratio_ok"] == 1 and len(calls) == 1 and st["inl_ratio_pt"] == 40.0 and st["inl_ratio_ls"] == 40.0
    # below the ratio in one kind: rejected without a solve (and ACTIVE -> READY -> pose graph -> IDLE)
    for nf in ((200, 200, 30, 100), (200, 100, 100, 100), (200, 100, 30, 100)):
        h2, calls2 = _hostmap()
        st = _step(h2, pr, n_feat=nf, lc_inlier_ratio=30.0 if nf != (200, 100, 30, 100) else 40.0)
        assert st["ratio_ok"] == 0 and st["accepted"] == 0 and not calls2 and st["state_after"] == LC_IDLE
        h2.close()
    # a zero feature count: NaN or 0, never above the ratio
    for nf in ((0, 100, 30, 30), (100, 0, 30, 30), (100, 100, 0, 30), (0, 0, 0, 0)):
        h2, calls2 = _hostmap()
        st = _step(h2, pr, n_feat=nf)
        assert st["ratio_ok"] == 0 and not calls2, nf
        h2.close()
    h.close()


def test_gate_with_one_kind_disabled():
    pr = cases.problem(40, 12, 0.25)
    # lines off: their counts do not matter, and no line reaches the solver
    h, calls = _hostmap()
    st = _step(h, pr, n_feat=(100, 100, 0, 0), has_lines=False)
    assert st["ratio_ok"] == 1 and calls[0]["n_pt"] == 40 and calls[0]["n_ln"] == 0
    h.close()
    h, calls = _hostmap()
    st = _step(h, pr, n_feat=(0, 0, 30, 30), has_points=False)
    assert st["ratio_ok"] == 1 and calls[0]["n_pt"] == 0 and calls[0]["n_ln"] == 12
    h.close()
    h, calls = _hostmap()
    st = _step(h, pr, n_feat=(100, 100, 30, 30), has_points=False, has_lines=False)
    assert st["ratio_ok"] == 0 and not calls
    h.close()


def _sequence(h):
    """accept -> (NULL candidate) -> READY: pose graph -> IDLE. Returns what the tests compare."""
    pr = cases.problem(40, 12, 0.25)
    T0 = [_kf(h, k) for k in range(N_KF)]
    assert h.lc_state() == LC_IDLE
    st1 = _step(h, pr)
    state1 = h.lc_state()
    poses, idxs = h.lc_pose_list().copy(), h.lc_idx_list().copy()
    pt_rows, ls_rows = h.lc_feature_idxs(1, 0), h.lc_feature_idxs(2, 0)
    st2 = h.loop_closure_step(None)
    T1 = [_kf(h, k) for k in range(N_KF)]
    return dict(pr=pr, st1=st1, st2=st2, state1=state1, state2=h.lc_state(), poses=poses, idxs=idxs, pt_rows=pt_rows,
                ls_rows=ls_rows, T0=np.array(T0), T1=np.array(T1), idxs_after=h.lc_idx_list().copy())


def test_accept_then_reject_runs_the_pose_graph():
    h, calls = _hostmap()
    s = _sequence(h)
    ref = calls[0]["ref"]
    # accepted: lists extended, IDLE -> ACTIVE
    assert s["st1"]["accepted"] == 1 and s["st1"]["state_before"] == LC_IDLE and s["st1"]["state_after"] == LC_ACTIVE
    assert s["state1"] == LC_ACTIVE and s["st1"]["pgo_ran"] == 0
    np.testing.assert_array_equal(s["idxs"], [[0, N_LOOP - 1, 1]])
    np.testing.assert_array_equal(s["poses"], [ref["pose_inc"]])
    # the index rows of the inliers only
    np.testing.assert_array_equal(s["pt_rows"], _rows(40, 5000)[ref["pt_inlier"].astype(bool)])
    np.testing.assert_array_equal(s["ls_rows"], _rows(12, 7000)[ref["ln_inlier"].astype(bool)])
    assert len(s["pt_rows"]) == 30 and len(s["ls_rows"]) == 9
    # no candidate while ACTIVE: READY, the pose graph ran, the poses moved, IDLE
    assert s["st2"]["is_candidate"] == 0 and s["st2"]["state_before"] == LC_ACTIVE and s["st2"]["pgo_ran"] == 1
    assert s["st2"]["state_after"] == LC_IDLE and s["state2"] == LC_IDLE
    pg = s["st2"]["pgo"]
    assert pg["n_vertices"] == N_LOOP and pg["n_loop_edges"] == 1 and pg["chi2_final"] < pg["chi2_initial"]
    assert np.abs(s["T1"] - s["T0"]).max() > 1e-3
    np.testing.assert_array_equal(s["idxs_after"], [[0, N_LOOP - 1, 0]])   # marked optimised
    # idle and nothing to do: stays idle, no pose graph
    st3 = h.loop_closure_step(None)
    assert st3["state_after"] == LC_IDLE and st3["pgo_ran"] == 0
    h.close()


def test_rejected_candidate_while_active_and_while_idle():
    h, calls = _hostmap()
    bad = cases.problem(*cases.SINGULAR_SHAPE)
    st = _step(h, bad, n_feat=(1, 1, 0, 0), has_lines=False)   # passes the gate, fails the accept test
    assert st["ratio_ok"] == 1 and st["accepted"] == 0 and st["state_after"] == LC_IDLE and st["pgo_ran"] == 0
    assert len(h.lc_pose_list()) == 0 and len(h.lc_idx_list()) == 0
    assert _step(h, cases.problem(40, 12, 0.25))["state_after"] == LC_ACTIVE
    # a second accepted loop while ACTIVE stays ACTIVE and extends the lists
    assert _step(h, cases.problem(64, 0, 0.0), has_lines=False)["state_after"] == LC_ACTIVE
    assert len(h.lc_pose_list()) == 2 and len(h.lc_feature_idxs(2, 1)) == 0 and len(h.lc_feature_idxs(1, 1)) == 64
    st = _step(h, bad, n_feat=(1, 1, 0, 0), has_lines=False)
    assert st["accepted"] == 0 and st["state_before"] == LC_ACTIVE and st["pgo_ran"] == 1 and st["state_after"] == LC_IDLE
    assert st["pgo"]["n_loop_edges"] == 2
    h.close()


def test_lcpose_params_reach_the_solver():
    h, calls = _hostmap()
    h.set_lcpose_params(capi.lcpose_params(variant=capi.LCPOSE_GN, lc_inl=0.9))
    st = _step(h, cases.problem(40, 12, 0.25))
    assert st["accepted"] == 0 and not (st["conditions"] & 4) and calls[0]["ref"]["iters_ref"] == 0
    h.set_lcpose_params(None)
    assert _step(h, cases.problem(40, 12, 0.25))["accepted"] == 1
    h.close()


@pytest.mark.gpu
def test_gpu_sequence_matches_the_hooked_run():
    ref_h, _ = _hostmap()
    ref = _sequence(ref_h)
    gpu_h, _ = _hostmap(hooks=False)
    out = _sequence(gpu_h)   # plba_lc_relative_pose and plba_pgo_optimize on the GPU
    for k in ("state1", "state2"):
        assert out[k] == ref[k]
    for k in ("idxs", "pt_rows", "ls_rows", "idxs_after"):
        np.testing.assert_array_equal(out[k], ref[k])
    assert parity.elem_violation(out["poses"], ref["poses"]) <= 1.0
    for k in ("accepted", "conditions", "n_inl_pt", "n_inl_ln", "state_after"):
        assert out["st1"][k] == ref["st1"][k]
    assert out["st2"]["pgo_ran"] == 1 and out["st2"]["pgo"]["n_edges"] == ref["st2"]["pgo"]["n_edges"]
    np.testing.assert_allclose(out["T1"], ref["T1"], atol=1e-7)
    ref_h.close()
    gpu_h.close()
