"""Host mirror of MapHandler::isLoopClosure from two keyframe indices (src/mapHandler.cpp:4303-4411):
the descriptor matching of :4334 / :4360, the candidate built in i1 order (:4336-4379), the gate and
what follows (tests/test_host_lcpose.py). CPU tests drive it with the matcher hook set to the numpy
checker (tests/ref_descmatch.py) and the relative-pose hook set to tests/ref_lcpose.py; the GPU test
(tests/test_gpu_isloopclosure.py) runs the same without hooks."""
import types

import numpy as np
import pytest

import descmatch_cases as dcases
import ref_descmatch
import ref_lcpose
from plba import pgo
from plba.lib import PlbaError
from plba.slam_map import LC_ACTIVE, LC_IDLE, HostMap, match_params
from test_host_pgo import _oracle_hook

N_LOOP, N_KF = 24, 27
KF_CURR = N_LOOP - 1
PLANTED = (0, 3)            # keyframes that see the place of KF_CURR
CANDIDATES = list(range(8))


def _idx(kf, n, kind):
    """The idx fields of a keyframe's features (distinct per keyframe and kind)."""
    return [10000 * kf + 1000 * kind + i for i in range(n)]


def frames():
    """kf_idx -> feature dict: the planted keyframes share kf0's features, the rest are unrelated."""
    kf0, kf1, _ = dcases.keyframe_pair()
    f = {k: (kf0 if k in PLANTED else dcases.unrelated_keyframe(seed=k)) for k in CANDIDATES}
    f[KF_CURR] = kf1
    return f


def match_hook(calls):
    """plba_desc_match by tests/ref_descmatch.py."""
    def fn(b, m12, cnt):
        db = b.desc_bytes
        off1, off2 = [b.off1[i] for i in range(b.n + 1)], [b.off2[i] for i in range(b.n + 1)]

        def rows(ptr, n):
            return np.ctypeslib.as_array(ptr, (n * db,)).reshape(n, db).copy() if n else np.zeros((0, db), np.uint8)
        d1, d2 = rows(b.desc1, off1[-1]), rows(b.desc2, off2[-1])
        calls.append(dict(n=b.n, off1=off1, off2=off2, nnr=[b.nnr[i] for i in range(b.n)], best_lr=b.best_lr))
        for k in range(b.n):
            m, c = ref_descmatch.match(d1[off1[k]:off1[k + 1]], d2[off2[k]:off2[k + 1]], np.float32(b.nnr[k]), bool(b.best_lr))
            for i, v in enumerate(m):
                m12[off1[k] + i] = int(v)
            cnt[k] = c
        return 0
    return fn


def lcpose_hook(calls, accept_all=False):
    """plba_lc_relative_pose for a batch, by tests/ref_lcpose.py. ``accept_all``: every match an
    inlier and the candidate accepted, so that the whole index rows reach the lists."""
    def fn(b, p, out, pin, lin):
        def arr(ptr, lo, hi, w):
            return np.ctypeslib.as_array(ptr, (hi * w,)).reshape(hi, w)[lo:].copy() if hi > lo else np.zeros((0, w))
        for k in range(b.n):
            p0, p1, l0, l1 = b.pt_off[k], b.pt_off[k + 1], b.ln_off[k], b.ln_off[k + 1]
            prob = types.SimpleNamespace(pt_P=arr(b.pt_P, p0, p1, 3), pt_obs=arr(b.pt_obs, p0, p1, 2),
                                         ln_sP=arr(b.ln_sP, l0, l1, 3), ln_eP=arr(b.ln_eP, l0, l1, 3),
                                         ln_le=arr(b.ln_le, l0, l1, 3), cam=(b.fx, b.fy, b.cx, b.cy))
            ref = ref_lcpose.relative_pose(prob, p)
            calls.append(dict(prob=prob, ref=ref, batch=b.n))
            o = out[k]
            for name in ("accepted", "conditions", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln", "e", "unc", "t", "r_deg"):
                setattr(o, name, ref[name])
            for name in ("x_inc", "pose_inc", "T_inc", "H"):
                getattr(o, name)[:] = list(np.asarray(ref[name]).ravel())
            if accept_all:
                o.accepted = 1
            for i in range(p1 - p0):
                pin[p0 + i] = 1 if accept_all else int(ref["pt_inlier"][i])
            for i in range(l1 - l0):
                lin[l0 + i] = 1 if accept_all else int(ref["ln_inlier"][i])
        return 0
    return fn


def hostmap(hooks=True, accept_all=False, feats=None, skip=()):
    """A loop map whose keyframes CANDIDATES and KF_CURR carry features. Returns (HostMap, calls)."""
    feats = frames() if feats is None else feats
    m, _, _, _, line3d = pgo.loop_map(n_loop=N_LOOP, n_after=N_KF - N_LOOP, seed=3)
    for k, f in feats.items():
        m.keyframes[k].pt_idx, m.keyframes[k].ls_idx = _idx(k, len(f["pdesc"]), 1), _idx(k, len(f["ldesc"]), 2)
    h = HostMap(m)
    for i, L in enumerate(line3d):
        h.set_line_geometry(i, L, L[:3] * 0.5)
    for k, f in feats.items():
        if k not in skip:
            h.set_keyframe_features(k, f["pdesc"], f["P"], f["pl"], f["ldesc"], f["sP"], f["eP"], f["le"])
    calls = dict(match=[], pose=[])
    if hooks:
        h.set_match_fn(match_hook(calls["match"]))
        h.set_lcpose_solver(lcpose_hook(calls["pose"], accept_all))
        h.set_pgo_solver(_oracle_hook({}))
    return h, calls


def model(kf0_idx, kf1_idx, f0, f1, mp):
    """src/mapHandler.cpp:4327-4402 in Python: the candidate and the gate's figures."""
    out = dict(P=[], obs=[], sP=[], eP=[], le=[], pt_idx=[], ls_idx=[], common_pt=0, common_ls=0)
    n_pt_0, n_pt_1, n_ls_0, n_ls_1 = len(f0["pdesc"]), len(f1["pdesc"]), len(f0["ldesc"]), len(f1["ldesc"])
    if mp.has_points and n_pt_1 and n_pt_0:
        m12, out["common_pt"] = ref_descmatch.match(f0["pdesc"], f1["pdesc"], np.float32(mp.min_ratio_12_p), bool(mp.best_lr))
        for i1, i2 in enumerate(m12):
            if i2 < 0:
                continue
            out["P"].append(f0["P"][i1])
            out["obs"].append(f1["pl"][i2])
            out["pt_idx"].append([_idx(kf0_idx, n_pt_0, 1)[i1], i1, _idx(kf1_idx, n_pt_1, 1)[i2], i2])
    if mp.has_lines and n_ls_1 and n_ls_0:
        m12, out["common_ls"] = ref_descmatch.match(f0["ldesc"], f1["ldesc"], np.float32(mp.min_ratio_12_l), bool(mp.best_lr))
        for i1, i2 in enumerate(m12):
            if i2 < 0:
                continue
            out["sP"].append(f0["sP"][i1])
            out["eP"].append(f0["eP"][i1])
            out["le"].append(f1["le"][i2])
            out["ls_idx"].append([_idx(kf0_idx, n_ls_0, 2)[i1], i1, _idx(kf1_idx, n_ls_1, 2)[i2], i2])
    with np.errstate(divide="ignore", invalid="ignore"):
        cp, cl = np.float64(out["common_pt"]), np.float64(out["common_ls"])
        out["ratio_pt"] = max(100.0 * cp / n_pt_0, 100.0 * cp / n_pt_1)   # C++ max(a, b): a < b ? b : a
        out["ratio_ls"] = max(100.0 * cl / n_ls_0, 100.0 * cl / n_ls_1)
    for k, w in (("P", 3), ("obs", 2), ("sP", 3), ("eP", 3), ("le", 3)):
        out[k] = np.array(out[k], np.float64).reshape(-1, w)
    for k in ("pt_idx", "ls_idx"):
        out[k] = np.array(out[k], np.int32).reshape(-1, 4)
    return out


def _same_ratios(st, mod):
    """Equal, a NaN (0 / 0 features) being equal to a NaN."""
    return all((np.isnan(a) and np.isnan(b)) or a == b
               for a, b in ((st["inl_ratio_pt"], mod["ratio_pt"]), (st["inl_ratio_ls"], mod["ratio_ls"])))


def _assert_candidate(call, st, h, mod, loop=0):
    prob = call["prob"]
    for a, b in ((prob.pt_P, mod["P"]), (prob.pt_obs, mod["obs"]), (prob.ln_sP, mod["sP"]), (prob.ln_eP, mod["eP"]),
                 (prob.ln_le, mod["le"])):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(h.lc_feature_idxs(1, loop), mod["pt_idx"])   # accept_all: every row is kept
    np.testing.assert_array_equal(h.lc_feature_idxs(2, loop), mod["ls_idx"])
    assert _same_ratios(st, mod)


def test_candidate_equals_the_python_model():
    h, calls = hostmap(accept_all=True)
    f = frames()
    mp = match_params()
    st = h.loop_closure_step_kf(0, KF_CURR, mp)
    mod = model(0, KF_CURR, f[0], f[KF_CURR], mp)
    _, _, true = dcases.keyframe_pair()
    # the planted matches are what the matcher finds, in i1 order
    np.testing.assert_array_equal(mod["pt_idx"][:, [1, 3]], true["pt"])
    np.testing.assert_array_equal(mod["ls_idx"][:, [1, 3]], true["ln"])
    assert len(calls["match"]) == 1 and calls["match"][0]["n"] == 2 and calls["match"][0]["best_lr"] == 1
    assert calls["match"][0]["nnr"] == [np.float32(0.9), np.float32(0.9)]
    assert calls["match"][0]["off1"] == [0, 70, 90] and calls["match"][0]["off2"] == [0, 60, 77]
    assert st["ratio_ok"] == 1 and st["accepted"] == 1 and st["state_after"] == LC_ACTIVE and len(calls["pose"]) == 1
    _assert_candidate(calls["pose"][0], st, h, mod)
    np.testing.assert_array_equal(h.lc_idx_list(), [[0, KF_CURR, 1]])
    # other parameters reach the matcher: no cross-check, a ratio per kind
    mp2 = match_params(min_ratio_12_p=0.6, min_ratio_12_l=1.0, best_lr=False)
    st = h.loop_closure_step_kf(3, KF_CURR, mp2)
    assert calls["match"][1]["nnr"] == [np.float32(0.6), np.float32(1.0)] and calls["match"][1]["best_lr"] == 0
    _assert_candidate(calls["pose"][1], st, h, model(3, KF_CURR, f[3], f[KF_CURR], mp2), loop=1)
    h.close()


def test_real_verification_accepts_the_planted_pair_and_keeps_the_inlier_rows():
    h, calls = hostmap()
    st = h.loop_closure_step_kf(0, KF_CURR)
    ref = calls["pose"][0]["ref"]
    mod = model(0, KF_CURR, frames()[0], frames()[KF_CURR], match_params())
    assert st["accepted"] == 1 and ref["accepted"] == 1 and st["n_inl_pt"] == 30 and st["n_inl_ln"] == 9
    np.testing.assert_array_equal(h.lc_feature_idxs(1, 0), mod["pt_idx"][ref["pt_inlier"].astype(bool)])
    np.testing.assert_array_equal(h.lc_feature_idxs(2, 0), mod["ls_idx"][ref["ln_inlier"].astype(bool)])
    np.testing.assert_array_equal(h.lc_pose_list(), [ref["pose_inc"]])
    # an unrelated keyframe: nothing matches, the gate fails, ACTIVE -> READY -> pose graph -> IDLE
    st = h.loop_closure_step_kf(1, KF_CURR)
    assert st["ratio_ok"] == 0 and st["accepted"] == 0 and len(calls["pose"]) == 1
    assert st["state_before"] == LC_ACTIVE and st["pgo_ran"] == 1 and st["state_after"] == LC_IDLE
    h.close()


@pytest.mark.parametrize("has_points,has_lines", [(True, False), (False, True), (False, False)])
def test_has_points_has_lines(has_points, has_lines):
    h, calls = hostmap(accept_all=True)
    f = frames()
    mp = match_params(has_points=has_points, has_lines=has_lines)
    st = h.loop_closure_step_kf(0, KF_CURR, mp)
    mod = model(0, KF_CURR, f[0], f[KF_CURR], mp)
    c = calls["match"][0]
    # a disabled kind is an empty pair: its descriptors do not reach the matcher
    assert c["off1"] == [0, 70 if has_points else 0, (70 if has_points else 0) + (20 if has_lines else 0)]
    assert _same_ratios(st, mod)
    if not (has_points or has_lines):
        assert st["ratio_ok"] == 0 and not calls["pose"] and st["state_after"] == LC_IDLE
    else:
        assert st["ratio_ok"] == 1 and len(mod["P"]) == (40 if has_points else 0) and len(mod["sP"]) == (12 if has_lines else 0)
        _assert_candidate(calls["pose"][0], st, h, mod)
    h.close()


@pytest.mark.parametrize("empty", ["pt0", "pt1", "ls0", "ls1"])
def test_empty_side_guards(empty):
    """:4331 / :4357 — a kind with no feature in either keyframe is not matched; its ratio is NaN or
    0 / 0 = NaN or 0, never above the threshold, so with both kinds on the gate fails."""
    f = dict(frames())
    kf, kind = (0 if empty.endswith("0") else KF_CURR), empty[:2]
    g = dict(f[kf])
    for k in (("pdesc", "P", "pl") if kind == "pt" else ("ldesc", "sP", "eP", "le")):
        g[k] = g[k][:0]
    f[kf] = g
    h, calls = hostmap(accept_all=True, feats=f)
    st = h.loop_closure_step_kf(0, KF_CURR)
    mod = model(0, KF_CURR, f[0], f[KF_CURR], match_params())
    c = calls["match"][0]
    widths = [c["off1"][1] - c["off1"][0], c["off2"][1] - c["off2"][0], c["off1"][2] - c["off1"][1], c["off2"][2] - c["off2"][1]]
    assert widths == ([0, 0, 20, 17] if kind == "pt" else [70, 60, 0, 0])
    assert st["ratio_ok"] == 0 and not calls["pose"]
    assert _same_ratios(st, mod)
    # with the empty kind switched off the other kind decides
    mp = match_params(has_points=kind != "pt", has_lines=kind != "ls")
    st = h.loop_closure_step_kf(0, KF_CURR, mp)
    assert st["ratio_ok"] == 1 and st["accepted"] == 1
    _assert_candidate(calls["pose"][0], st, h, model(0, KF_CURR, f[0], f[KF_CURR], mp))
    h.close()


def _state(h):
    return (h.lc_state(), h.lc_pose_list().tobytes(), h.lc_idx_list().tobytes())


def test_bad_indices_leave_the_map_untouched():
    h, calls = hostmap(skip=(5,))
    assert h.loop_closure_step_kf(0, KF_CURR)["state_after"] == LC_ACTIVE   # so that a stray step would show
    before = _state(h)
    n_match = len(calls["match"])
    for a, b in ((-1, KF_CURR), (0, N_KF + 5), (N_KF, KF_CURR), (5, KF_CURR), (0, 5), (0, 9)):   # 5, 9: no features set
        with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
            h.loop_closure_step_kf(a, b)
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.verify_loop_candidates(KF_CURR, [0, 1, 99])
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.verify_loop_candidates(-2, [0, 1])
    assert _state(h) == before and len(calls["match"]) == n_match and len(calls["pose"]) == 1
    with pytest.raises(ValueError):
        h.set_keyframe_features(0, np.zeros((3, 32), np.uint8), np.zeros((3, 3)), np.zeros((3, 2)), np.zeros((0, 32), np.uint8),
                                np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    h.close()


def test_verify_loop_candidates_equals_single_steps_and_changes_no_state():
    h, calls = hostmap()
    before = _state(h)
    out = h.verify_loop_candidates(KF_CURR, CANDIDATES)
    assert _state(h) == before
    # one match call with 2K pairs, one relative-pose call with the candidates that pass the gate
    assert len(calls["match"]) == 1 and calls["match"][0]["n"] == 2 * len(CANDIDATES)
    assert len(calls["pose"]) == len(PLANTED) and all(c["batch"] == len(PLANTED) for c in calls["pose"])
    assert out["accepted"].tolist() == [int(k in PLANTED) for k in CANDIDATES]
    f = frames()
    for k in CANDIDATES:
        mod = model(k, KF_CURR, f[k], f[KF_CURR], match_params())
        assert out["n_matches"][k].tolist() == [mod["common_pt"], mod["common_ls"]]
        h1, c1 = hostmap()
        st = h1.loop_closure_step_kf(k, KF_CURR)
        assert st["accepted"] == out["accepted"][k]
        if st["accepted"]:
            np.testing.assert_array_equal(h1.lc_pose_list()[0], out["pose_inc"][k])
        else:
            assert not out["pose_inc"][k].any()
        h1.close()
    assert h.verify_loop_candidates(KF_CURR, [])["accepted"].tolist() == []
    assert _state(h) == before
    h.close()


def test_cpu_restatement_of_the_bench_equals_the_checker():
    """plslam_desc_match_cpu (the timing yardstick of tools/descmatch_bench.py) on a mixed batch."""
    import ctypes as C
    from plba import capi
    from plba.slam_map import load_host
    L = load_host()
    shapes = [(257, 255, 32), (5, 0, 32), (1, 2, 32), (300, 1000, 32)]
    for nnr, best_lr in ((0.9, True), (0.6, False), (1.5, True)):
        bv = capi.MatchBatchView([dcases.pair(*s) for s in shapes], nnr, best_lr)
        m12, cnt = np.full(int(bv.off1[-1]), -7, np.int32), np.zeros(len(shapes), np.int32)
        ip = C.POINTER(C.c_int32)
        assert L.plslam_desc_match_cpu(None, C.byref(bv.struct), m12.ctypes.data_as(ip), cnt.ctypes.data_as(ip)) == 0
        for k, s in enumerate(shapes):
            rm, rc = ref_descmatch.match(*dcases.pair(*s), np.float32(nnr), best_lr)
            np.testing.assert_array_equal(m12[bv.off1[k]:bv.off1[k + 1]], rm)
            assert cnt[k] == rc
