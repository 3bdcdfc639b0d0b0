"""Host mirror of MapHandler::matchMap2KFPoints / Lines (plslam_match_map_to_kf, src/mapHandler.cpp:697-921)
with the CPU hooks (plslam_grid_match_cpu, plslam_desc_match_cpu) against the Python model of
tests/mapmatch_cases.py on a small synthetic map. No GPU."""
import ctypes as C

import numpy as np
import pytest

import mapmatch_cases as mc
from plba import slam_map
from plba.lib import PlbaError
from plba.slam_map import HostMap, mapmatch_params

IP, DP, BP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def hostmap(built, hooks=True, camera=True, features=True, endpoints=True):
    m, line3d, feat, _ = built
    h = HostMap(m)
    for i, L in enumerate(line3d):
        h.set_line_geometry(i, L, np.zeros(3))
    if features:
        h.set_keyframe_features(mc.KF_NEW, feat["pdesc"], feat["P"], feat["pl"], feat["ldesc"], feat["sP"], feat["eP"],
                                feat["le"])
    if endpoints:
        h.set_keyframe_line_endpoints(mc.KF_NEW, feat["spl"], feat["epl"])
    if camera:
        h.set_camera(*mc.CAM, mc.WIDTH, mc.HEIGHT)
    calls = []
    if hooks:
        h.set_grid_match_fn("cpu")

        def match(b, m12, cnt):
            calls.append([b.off1[i] for i in range(b.n + 1)])
            return h.L.plslam_desc_match_cpu(None, C.byref(b), m12, cnt)
        h.set_match_fn(match)
    return h, calls


def state(h, m):
    """Everything the association may change, through the getters."""
    out = dict(kf={}, pt={}, ln={})
    for kf in m.keyframes:
        pi, li = np.zeros(len(kf.pt_idx) + 1, np.int32), np.zeros(len(kf.ls_idx) + 1, np.int32)
        h._check(h.L.plslam_get_keyframe(h.h, kf.kf_idx, None, None, pi.ctypes.data_as(IP), len(kf.pt_idx),
                                         li.ctypes.data_as(IP), len(kf.ls_idx)), "get_keyframe")
        out["kf"][kf.kf_idx] = (pi[:-1].tolist(), li[:-1].tolist())
    cap = 8
    for lm in m.points:
        n, kfo, obs, dirs, sig = C.c_int32(), np.zeros(cap, np.int32), np.zeros((cap, 2)), np.zeros((cap, 3)), np.zeros(cap)
        md = np.zeros(32, np.uint8)
        h._check(h.L.plslam_get_point(h.h, lm.idx, None, None, None, C.byref(n), kfo.ctypes.data_as(IP), obs.ctypes.data_as(DP),
                                      dirs.ctypes.data_as(DP), sig.ctypes.data_as(DP), cap, md.ctypes.data_as(BP), None),
                 "get_point")
        k = n.value
        out["pt"][lm.idx] = (kfo[:k].tolist(), obs[:k].tolist(), dirs[:k].tolist(), sig[:k].tolist(), md.tolist())
    for lm in m.lines:
        n, kfo, obs, sig = C.c_int32(), np.zeros(cap, np.int32), np.zeros((cap, 4)), np.zeros(cap)
        md = np.zeros(32, np.uint8)
        h._check(h.L.plslam_get_line(h.h, lm.idx, None, None, None, C.byref(n), kfo.ctypes.data_as(IP), obs.ctypes.data_as(DP),
                                     sig.ctypes.data_as(DP), cap, md.ctypes.data_as(BP)), "get_line")
        k = n.value
        out["ln"][lm.idx] = (kfo[:k].tolist(), obs[:k].tolist(), sig[:k].tolist(), md.tolist())
    fg = np.zeros((4, 4), np.uint32)
    h._check(h.L.plslam_get_full_graph(h.h, 4, fg.ctypes.data_as(C.POINTER(C.c_uint32))), "full_graph")
    out["full_graph"] = fg.tolist()
    return out


def check_against_model(built, h, st, p, before):
    m, line3d, feat, Twf = built
    want = mc.model(m, line3d, feat, Twf, p)
    for k, v in want["stats"].items():
        assert st[k] == v, (k, st[k], v)
    after = state(h, m)
    assert after["kf"][mc.KF_NEW] == (want["pt_idx"], want["ls_idx"])
    assert after["full_graph"] == want["full_graph"].tolist()
    assert (np.array(after["full_graph"]) == np.array(after["full_graph"]).T).all()
    for k in range(3):
        assert after["kf"][k] == before["kf"][k]
    T = m.keyframes[mc.KF_NEW].T_kf_w
    for kind, key, lms in ((1, "pt", m.points), (2, "ln", m.lines)):
        for lm in lms:
            a, b = after[key][lm.idx], before[key][lm.idx]
            if lm.idx not in want["new_obs"][kind]:
                assert a == b, (key, lm.idx)
                continue
            assert a[0] == b[0] + [mc.KF_NEW] and a[1][:-1] == b[1] and a[-2] == b[-2] + [1.0]   # sigma2 = 1
            assert a[1][-1] == want["new_obs"][kind][lm.idx].tolist()
            if kind == 1:   # dir = T_kf_w * normalized(P), translation included as the reference has it
                fi = want["pt_idx"].index(lm.idx)
                d = feat["P"][fi] / np.linalg.norm(feat["P"][fi])
                np.testing.assert_allclose(a[2][-1], T[:3, :3] @ d + T[:3, 3], rtol=0, atol=1e-15)
    return want


@pytest.fixture(scope="module")
def built():
    return mc.build()


def test_observations_idx_graph_and_counts_match_the_model(built):
    h, calls = hostmap(built)
    before = state(h, built[0])
    p = mapmatch_params()
    st = h.match_map_to_kf(mc.KF_NEW, built[3], p)
    want = check_against_model(built, h, st, p, before)
    assert st["fallback"] == [0, 0] and calls == []
    assert st["accepted"][0] >= 15 and st["accepted"][1] >= 5 and st["visible"][0] > st["accepted"][0]
    assert st["rejected"][0] >= 1 and st["rejected"][1] >= 1       # the displaced features: the count goes down
    assert sum(v == -1 for v in want["pt_idx"]) >= 12
    assert h.check_incremental_gather()
    # a second call finds the matched landmarks already observed by the keyframe
    st2 = h.match_map_to_kf(mc.KF_NEW, built[3], p)
    assert st2["visible"][0] == st["visible"][0] - st["accepted"][0] and st2["accepted"] == [0, 0]


def test_twf_defaults_to_the_inverse_of_the_keyframe_pose(built):
    h, _ = hostmap(built)
    h2, _ = hostmap(built)
    a, b = h.match_map_to_kf(mc.KF_NEW, None), h2.match_map_to_kf(mc.KF_NEW, built[3])
    a.pop("match_ms"), b.pop("match_ms")
    assert a == b and state(h, built[0]) == state(h2, built[0])


def test_fallback_runs_when_the_grid_finds_too_few(built):
    # a window of one cell finds fewer than the minimum, and the map side is above the minimum
    p = mapmatch_params(ws=0, min_pt_matches=40, min_ls_matches=22)
    h, calls = hostmap(built)
    before = state(h, built[0])
    st = h.match_map_to_kf(mc.KF_NEW, built[3], p)
    assert st["fallback"] == [1, 1] and len(calls) == 1   # one call, both kinds
    assert 0 < st["grid_matches"][0] < 40 < st["visible"][0] and 0 < st["grid_matches"][1] < 22 < st["visible"][1]
    assert calls[0][1] == st["visible"][0] and calls[0][2] - calls[0][1] == st["visible"][1]
    check_against_model(built, h, st, p, before)
    assert st["accepted"][1] >= 5
    # a minimum above the visible landmarks: no fallback although nothing was matched
    p = mapmatch_params(ws=0, min_pt_matches=1000, min_ls_matches=1000)
    h, calls = hostmap(built)
    before = state(h, built[0])
    st = h.match_map_to_kf(mc.KF_NEW, built[3], p)
    assert st["fallback"] == [0, 0] and calls == []
    check_against_model(built, h, st, p, before)
    # only one kind falls back: the other is an empty pair of the same call
    p = mapmatch_params(ws=0, min_pt_matches=40)
    h, calls = hostmap(built)
    before = state(h, built[0])
    st = h.match_map_to_kf(mc.KF_NEW, built[3], p)
    assert st["fallback"] == [1, 0] and calls == [[0, st["visible"][0], st["visible"][0]]]
    check_against_model(built, h, st, p, before)
    # fast matching off: the brute-force matcher alone
    p = mapmatch_params(fast_matching=0)
    h, calls = hostmap(built)
    before = state(h, built[0])
    st = h.match_map_to_kf(mc.KF_NEW, built[3], p)
    assert st["fallback"] == [1, 1] and len(calls) == 1
    check_against_model(built, h, st, p, before)


def test_a_kind_switched_off_is_left_alone(built):
    p = mapmatch_params(has_lines=0)
    h, _ = hostmap(built)
    before = state(h, built[0])
    st = h.match_map_to_kf(mc.KF_NEW, built[3], p)
    check_against_model(built, h, st, p, before)
    assert st["visible"][1] == 0 and state(h, built[0])["ln"] == before["ln"]


def test_invalid_arguments_leave_the_map_unchanged(built):
    for kw, kf in ((dict(), 7), (dict(), -1), (dict(features=False, endpoints=False), mc.KF_NEW),
                   (dict(endpoints=False), mc.KF_NEW), (dict(camera=False), mc.KF_NEW), (dict(), 1)):
        h, _ = hostmap(built, **kw)
        before = state(h, built[0])
        with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
            h.match_map_to_kf(kf, built[3])
        assert state(h, built[0]) == before
    h, _ = hostmap(built)
    before = state(h, built[0])
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.match_map_to_kf(mc.KF_NEW, built[3], mapmatch_params(ws=-1))
    h.set_grid_match_fn(lambda b, m12, cnt: -1)          # a failing matcher
    with pytest.raises(PlbaError):
        h.match_map_to_kf(mc.KF_NEW, built[3])

    def wild(b, m12, cnt):                                # a matcher that answers outside the features
        m12[0], cnt[0], cnt[1] = 10 ** 6, 100, 100       # (enough matches: no fallback replaces them)
        return 0
    h.set_grid_match_fn(wild)
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.match_map_to_kf(mc.KF_NEW, built[3])
    assert state(h, built[0]) == before and h.check_incremental_gather()


def test_struct_layout_and_defaults():
    p = mapmatch_params()
    assert C.sizeof(p) == 8 * 4 + 5 * 8 and C.sizeof(slam_map.PlslamMapMatchStats) == 12 * 4 + 8
    assert (p.fast_matching, p.ws, p.min_pt_matches, p.min_ls_matches, p.best_lr, p.has_points, p.has_lines) == \
        (1, 3, 10, 6, 1, 1, 1)
    assert (p.max_kf_epip_p, p.max_kf_epip_l, p.line_sim_th, p.min_ratio_12_p, p.min_ratio_12_l) == (1.0, 1.0, 0.75, 0.9, 0.9)
    n = C.c_int32()
    L = slam_map.load_host()
    for bad in (float("nan"), float("inf"), 1e300, -2e6):
        assert L.plslam_line_cells(bad, 0.0, 1.0, 1.0, None, 0, C.byref(n)) != 0
    buf = np.full((3, 2), -9, np.int32)
    assert L.plslam_line_cells(0.5, 0.5, 9.5, 0.5, buf.ctypes.data_as(IP), 2, C.byref(n)) == 0
    assert n.value == 10 and buf.tolist() == [[0, 0], [1, 0], [-9, -9]]
    bv = slam_map.capi.GridMatchBatchView([])
    assert L.plslam_grid_match_cpu(None, None, None, None) != 0
    bv.struct.n = 1
    bv.struct.off1 = None
    assert L.plslam_grid_match_cpu(None, C.byref(bv.struct), None, None) != 0
