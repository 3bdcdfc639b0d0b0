"""Host mirror of MapHandler::matchKF2KFPoints / Lines (plslam_match_kf_to_kf, src/mapHandler.cpp:237-590) and
of lookForCommonMatches (:923-990 without the refinement) with the CPU hooks, against a Python model of the
row loop over the checker's association (tests/ref_kfassoc.py). No GPU."""
import copy
import ctypes as C

import numpy as np
import pytest

import kfassoc_cases as KC
import ref_kfassoc as RK
import stereo_cases as SC
import ref_stereo as RS
from plba import slam_map
from plba.lib import PlbaError
from plba.slam_map import KF, HostMap, Landmark, SlamMap, mapmatch_params, median_descriptor

IP, DP, BP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
PREV, CURR, OLD = 1, 2, 0   # keyframe 0 is an earlier observer of the existing landmarks
CAM = (KC.CAMERA["fx"], KC.CAMERA["fy"], KC.CAMERA["cx"], KC.CAMERA["cy"])


def build(seed=4, n_pt=(50, 45), n_ls=(20, 22)):
    """(SlamMap, pair): the previous keyframe's features of a generated pair; every fourth point row and the
    line rows with ls_new 0 carry a landmark seen by keyframes OLD and PREV; landmark 1 of each kind is
    deleted (NULL) although a feature still names it."""
    rng = np.random.default_rng(seed)
    p = KC.pair(seed, n_pt, n_ls)
    p["pt_pl_p"] = np.array([KC.proj(P) for P in p["pt_P_p"]])
    kfs = [KF(OLD, np.eye(4), True, [], []), KF(PREV, p["T_prev"], True, [], []), KF(CURR, p["T_curr"], True, [], [])]

    def lm(idx, pos, desc, obs, width):
        return Landmark(idx=idx, local=True, inlier=True, pos=np.array(pos, np.float64),
                        desc_list=[rng.integers(0, 256, KC.DB, dtype=np.uint8), np.array(desc)],
                        obs_list=[rng.uniform(0, 400, width), np.array(obs, np.float64)], kf_obs_list=[OLD, PREV],
                        sigma_list=[1.0, 1.0], dir_list=[np.array([0.0, 0.0, 1.0])] * 2 if width == 2 else None)
    points, lines, pt_idx, ls_idx = [], [], [], []
    for i in range(n_pt[0]):
        if i % 4 == 0:
            pt_idx.append(len(points))
            points.append(lm(len(points), p["T_prev"][:3, :3] @ p["pt_P_p"][i] + p["T_prev"][:3, 3], p["pdesc_p"][i],
                             p["pt_pl_p"][i], 2))
        else:
            pt_idx.append(-1)
    for i in range(n_ls[0]):
        if p["ls_new"][i] == 0:
            ls_idx.append(len(lines))
            lines.append(lm(len(lines), p["ls_lm_NDw"][i], p["ldesc_p"][i], np.concatenate([p["ls_spl_p"][i], p["ls_epl_p"][i]]), 4))
        else:
            ls_idx.append(-1)
    points[1], lines[1] = None, None
    kfs[PREV].pt_idx, kfs[PREV].ls_idx = pt_idx, ls_idx
    kfs[CURR].pt_idx, kfs[CURR].ls_idx = [-1] * n_pt[1], [-1] * n_ls[1]
    fg = rng.integers(0, 20, (3, 3)).astype(np.uint32)
    m = SlamMap(*CAM, keyframes=kfs, points=points, lines=lines, map_points_kf_idx={OLD: [x.idx for x in points if x]},
                full_graph=fg + fg.T, map_lines_kf_idx={OLD: [x.idx for x in lines if x]}, max_kf_idx=CURR)
    for lms in (points, lines):
        for x in lms:
            if x is not None:
                x.med_desc = x.desc_list[median_descriptor(x.desc_list)]
    return m, p


def hostmap(built, hooks=True, camera=True, pluker=True, curr_features=True):
    m, p = built
    h = HostMap(m)
    z = np.zeros
    h.set_keyframe_features(PREV, p["pdesc_p"], p["pt_P_p"], p["pt_pl_p"], p["ldesc_p"], p["ls_sP_p"], p["ls_eP_p"],
                            z((len(p["ldesc_p"]), 3)))
    h.set_keyframe_line_endpoints(PREV, p["ls_spl_p"], p["ls_epl_p"])
    if pluker:
        h.set_keyframe_line_pluker(PREV, p["ls_NDc_p"])
    if curr_features:
        n = len(p["ldesc_c"])
        h.set_keyframe_features(CURR, p["pdesc_c"], p["pt_P_c"], p["pt_pl_c"], p["ldesc_c"], z((n, 3)), z((n, 3)), z((n, 3)))
        h.set_keyframe_line_endpoints(CURR, p["ls_spl_c"], p["ls_epl_c"])
    if camera:
        h.set_camera(*CAM, KC.WIDTH, KC.HEIGHT)
    if hooks:
        h.set_kfassoc_fn("cpu")
        h.set_grid_match_fn("cpu")
        h.set_match_fn(lambda b, m12, cnt: h.L.plslam_desc_match_cpu(None, C.byref(b), m12, cnt))
    return h


def state(h, n_kf=3):
    """The whole map through the getters: keyframe idx arrays, every landmark with its lists and med_desc,
    full_graph, map_points_kf_idx / map_lines_kf_idx."""
    out = dict(kf={}, pt={}, ln={}, kf_pts={}, kf_lns={})
    cap = 512
    for k in range(n_kf):
        pi, li = np.full(cap, -9, np.int32), np.full(cap, -9, np.int32)
        h._check(h.L.plslam_get_keyframe(h.h, k, None, None, pi.ctypes.data_as(IP), cap, li.ctypes.data_as(IP), cap), "get_keyframe")
        out["kf"][k] = (pi[pi != -9].tolist(), li[li != -9].tolist())
        for key, fn in (("kf_pts", h.L.plslam_kf_idx_get), ("kf_lns", h.L.plslam_kf_lines_idx_get)):
            buf, n = np.zeros(cap, np.int32), C.c_int32()
            h._check(fn(h.h, k, buf.ctypes.data_as(IP), cap, C.byref(n)), key)
            out[key][k] = buf[:max(n.value, 0)].tolist()   # -1: the keyframe has no list yet
    for key, kind, width, getter in (("pt", 1, 2, h.L.plslam_get_point), ("ln", 2, 4, h.L.plslam_get_line)):
        idx = 0
        while True:
            if not h.exists(kind, idx):
                if idx > 200:
                    break
                idx += 1
                continue
            n, kfo, obs, dirs, sig = C.c_int32(), np.zeros(8, np.int32), np.zeros((8, width)), np.zeros((8, 3)), np.zeros(8)
            md, pos = np.zeros(32, np.uint8), np.zeros(3 if kind == 1 else 6)
            if kind == 1:
                rc = getter(h.h, idx, pos.ctypes.data_as(DP), None, None, C.byref(n), kfo.ctypes.data_as(IP), obs.ctypes.data_as(DP),
                            dirs.ctypes.data_as(DP), sig.ctypes.data_as(DP), 8, md.ctypes.data_as(BP), None)
            else:
                rc = getter(h.h, idx, pos.ctypes.data_as(DP), None, None, C.byref(n), kfo.ctypes.data_as(IP), obs.ctypes.data_as(DP),
                            sig.ctypes.data_as(DP), 8, md.ctypes.data_as(BP))
            h._check(rc, "get landmark")
            k = n.value
            out[key][idx] = dict(pos=pos.tolist(), kf=kfo[:k].tolist(), obs=obs[:k].tolist(), sig=sig[:k].tolist(), md=md.tolist())
            if kind == 1:
                out[key][idx]["dirs"] = dirs[:k].tolist()
            idx += 1
    fg = np.zeros((n_kf, n_kf), np.uint32)
    h._check(h.L.plslam_get_full_graph(h.h, n_kf, fg.ctypes.data_as(C.POINTER(C.c_uint32))), "full_graph")
    out["full_graph"] = fg.tolist()
    return out


def model(built, before, prm):
    """:237-590 in Python over the checker's association: the state the mirror must leave behind, and the stats."""
    m, p = built
    q = dict(p)
    q["ls_new"] = np.array([v == -1 for v in m.keyframes[PREV].ls_idx], np.uint8)
    r = RK.associate(q, prm)
    s = copy.deepcopy(before)
    fg = np.array(before["full_graph"], np.int64)
    st = dict(grid_matches=list(r["n_grid"]), fallback=list(r["fallback"]), matches=list(r["n_matches"]), created=[0, 0],
              extended=[0, 0], rejected=[0, 0], pt_pairs=[], ls_pairs=[])
    descs = {}   # landmark -> its desc_list, to find med_desc

    def bump(obs_kfs):
        for o in obs_kfs:
            if o != CURR:
                fg[CURR, o] += 1
                fg[o, CURR] += 1
    for kind, key, lms, m12 in ((0, "pt", m.points, r["pt_m12"]), (1, "ln", m.lines, r["ls_m12"])):
        pidx, cidx = s["kf"][PREV][kind], s["kf"][CURR][kind]
        n_total = len(lms)
        d_p, d_c = (p["ldesc_p"], p["ldesc_c"]) if kind else (p["pdesc_p"], p["pdesc_c"])
        for i1, i2 in enumerate(m12):
            if i2 < 0:
                continue
            if kind:
                obs_p = np.concatenate([p["ls_spl_p"][i1], p["ls_epl_p"][i1]]).tolist()
                obs_c = np.concatenate([p["ls_spl_c"][i2], p["ls_epl_c"][i2]]).tolist()
            else:
                obs_p, obs_c = p["pt_pl_p"][i1].tolist(), p["pt_pl_c"][i2].tolist()
            rec = (r["ls_rec"] if kind else r["pt_rec"])[i1]
            if pidx[i1] == -1:
                if kind and r["ls_rejected"][i1]:
                    cidx[i2] = -1
                    st["rejected"][1] += 1
                    continue
                idx = n_total
                n_total += 1
                pidx[i1] = cidx[i2] = idx
                dl = [d_p[i1], d_c[i2]]
                s[key][idx] = dict(pos=rec[:6 if kind else 3].tolist(), kf=[PREV, CURR], obs=[obs_p, obs_c], sig=[1.0, 1.0],
                                   md=dl[median_descriptor(dl)].tolist())
                if not kind:
                    s[key][idx]["dirs"] = [rec[3:6].tolist(), rec[6:9].tolist()]
                s["kf_lns" if kind else "kf_pts"][PREV].append(idx)
                fg[CURR, PREV] += 1
                fg[PREV, CURR] += 1
                st["created"][kind] += 1
            else:
                lmk = lms[pidx[i1]]
                if lmk is None:
                    continue
                if kind and r["ls_rejected"][i1]:
                    cidx[i2] = -1
                    st["rejected"][1] += 1
                    continue
                cidx[i2] = lmk.idx
                e = s[key][lmk.idx]
                dl = descs.setdefault((kind, lmk.idx), list(lmk.desc_list))
                dl.append(d_c[i2])
                e["kf"].append(CURR), e["obs"].append(obs_c), e["sig"].append(1.0)
                e["md"] = dl[median_descriptor(dl)].tolist()
                if not kind:
                    e["dirs"].append(rec[6:9].tolist())
                bump(e["kf"])
                st["extended"][kind] += 1
            st["ls_pairs" if kind else "pt_pairs"].append([i1, int(i2)])
    s["full_graph"] = fg.tolist()
    return s, st


def DT4(p):
    return np.vstack([p["DT"], [0, 0, 0, 1]])


@pytest.fixture(scope="module")
def built():
    return build()


@pytest.mark.parametrize("over", [dict(), dict(line_query_in_grid_units=1), dict(best_lr=0, fast_matching=0)],
                         ids=["default", "grid_units", "brute_force_no_best_lr"])
def test_map_state_equals_the_model(built, over):
    h = hostmap(built)
    before = state(h)
    want, wst = model(built, before, RK.params(**{**KC.CAMERA, **over}))
    got = h.match_kf_to_kf(PREV, CURR, DT4(built[1]), over)
    assert got == wst
    after = state(h)
    for k in want:
        assert after[k] == want[k], k
    # not vacuous: landmarks of both kinds were created and extended, lines rejected, a NULL landmark skipped
    assert min(wst["created"]) >= 3 and min(wst["extended"]) >= 1 and wst["rejected"][1] >= 1
    assert len(wst["pt_pairs"]) == wst["created"][0] + wst["extended"][0] < wst["matches"][0]
    assert (np.array(after["full_graph"]) == np.array(after["full_graph"]).T).all()
    assert after["kf_pts"][PREV] and after["kf_lns"][PREV] and after["kf"][OLD] == before["kf"][OLD]
    assert h.check_incremental_gather()


def test_two_previous_rows_on_one_current_row_both_go_through():
    p = KC.two_on_one_pair()
    p["pt_pl_p"] = np.array([KC.proj(P) for P in p["pt_P_p"]])
    kfs = [KF(OLD, np.eye(4), True, [], []), KF(PREV, np.eye(4), True, [-1, -1], []), KF(CURR, np.eye(4), True, [-1, -1], [])]
    m = SlamMap(*CAM, keyframes=kfs, points=[], lines=[], map_points_kf_idx={}, full_graph=np.zeros((3, 3), np.uint32), max_kf_idx=CURR)
    h = HostMap(m)
    e = np.zeros((0, 3))
    h.set_keyframe_features(PREV, p["pdesc_p"], p["pt_P_p"], p["pt_pl_p"], np.zeros((0, 32), np.uint8), e, e, e)
    h.set_keyframe_features(CURR, p["pdesc_c"], p["pt_P_c"], p["pt_pl_c"], np.zeros((0, 32), np.uint8), e, e, e)
    h.set_camera(*CAM, KC.WIDTH, KC.HEIGHT)
    h.set_kfassoc_fn("cpu")
    st = h.match_kf_to_kf(PREV, CURR, np.eye(4), dict(best_lr=0))
    assert st["created"] == [2, 0] and st["pt_pairs"] == [[0, 0], [1, 0]]
    s = state(h)
    assert s["kf"][PREV][0] == [0, 1] and s["kf"][CURR][0] == [1, -1]   # the later row overwrites the idx
    assert s["full_graph"][CURR][PREV] == 2 and s["kf_pts"][PREV] == [0, 1]


def test_dt_defaults_to_the_relative_pose(built):
    a, b = hostmap(built), hostmap(built)
    sa, sb = a.match_kf_to_kf(PREV, CURR, None), b.match_kf_to_kf(PREV, CURR, DT4(built[1]))
    assert sa == sb and state(a) == state(b)   # the two DT differ in the last bits only: no cell changes here


def test_look_for_common_matches_equals_the_two_calls(built):
    a, b = hostmap(built), hostmap(built)
    both = a.look_for_common_matches(PREV, CURR)
    first = b.match_kf_to_kf(PREV, CURR, None)
    second = b.match_map_to_kf(CURR, None)
    both["map"].pop("match_ms"), second.pop("match_ms")
    assert both == dict(kf=first, map=second) and state(a) == state(b)


def test_refusals_leave_the_map_untouched(built):
    for kw, args in ((dict(), (7, CURR)), (dict(), (PREV, -1)), (dict(), (PREV, PREV)), (dict(pluker=False), (PREV, CURR)),
                     (dict(curr_features=False), (PREV, CURR)), (dict(camera=False), (PREV, CURR))):
        h = hostmap(built, **kw)
        before = state(h)
        with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
            h.match_kf_to_kf(*args)
        with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
            h.look_for_common_matches(*args)
        assert state(h) == before
    h = hostmap(built)
    before = state(h)
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.match_kf_to_kf(PREV, CURR, None, dict(ws=-1))
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.look_for_common_matches(PREV, CURR, None, mapmatch_params(ws=-1))
    h.set_kfassoc_fn(lambda b, p, o: -1)   # a failing hook
    with pytest.raises(PlbaError):
        h.match_kf_to_kf(PREV, CURR)

    def wild(b, p, o):   # a hook that answers outside the features
        o.pt_m12[0] = 10 ** 6
        o.n_grid[0] = o.n_matches[0] = 1
        return 0
    h.set_kfassoc_fn(wild)
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.match_kf_to_kf(PREV, CURR)
    assert state(h) == before and h.check_incremental_gather()


def three_keyframes(hooks):
    """From an empty map: three keyframes a few centimetres apart, each set up with set_keyframe_stereo from the
    same detector output, linked by two look_for_common_matches calls. Returns (HostMap, the two results)."""
    T = [KC.se3(0, 0, 0, [0.02 * k, 0.0, 0.01 * k]) for k in range(3)]
    m = SlamMap(*CAM, keyframes=[KF(k, T[k], True, [], []) for k in range(3)], points=[], lines=[], map_points_kf_idx={},
                full_graph=np.zeros((3, 3), np.uint32), max_kf_idx=2)
    h = HostMap(m)
    if hooks:
        h.set_stereo_fn("cpu"), h.set_kfassoc_fn("cpu"), h.set_grid_match_fn("cpu")
        h.set_match_fn(lambda b, m12, cnt: h.L.plslam_desc_match_cpu(None, C.byref(b), m12, cnt))
    sp = RS.params(**SC.CAMERA, pluker=1)
    h.set_camera(sp["fx"], sp["fy"], sp["cx"], sp["cy"], SC.WIDTH, SC.HEIGHT)
    for k in range(3):
        h.set_keyframe_stereo(k, SC.case("mixed"), sp)
    res = [h.look_for_common_matches(k - 1, k, dict(line_query_in_grid_units=1)) for k in (1, 2)]
    return h, res


def test_a_map_grows_from_detector_output_alone():
    h, (r1, r2) = three_keyframes(hooks=True)
    assert r1["kf"]["created"][0] >= 10 and r1["kf"]["created"][1] >= 1 and r1["kf"]["extended"] == [0, 0]
    assert r2["kf"]["extended"][0] >= 10 and r2["kf"]["extended"][1] >= 1   # the second link extends what the first made
    s = state(h)
    n_pt, n_ln = len(s["pt"]), len(s["ln"])
    assert n_pt == r1["kf"]["created"][0] + r2["kf"]["created"][0] and n_ln == r1["kf"]["created"][1] + r2["kf"]["created"][1]
    assert any(v["kf"] == [0, 1, 2] for v in s["pt"].values()) and any(v["kf"] == [0, 1, 2] for v in s["ln"].values())
    assert s["full_graph"][2][0] >= 10 and s["kf_pts"][0] and s["kf_pts"][1] is not None
    h.form_local_map(2)   # up to the LBA, which needs the device
    assert h.check_incremental_gather()
