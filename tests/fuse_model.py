"""Python model of MapHandler::loopClosureFuseLandmarks (src/mapHandler.cpp:5533-5808) on a SlamMap, with
the decisions of pl-slam-plucker_amd/host/fuse_landmarks.cpp where the reference is undefined, and the
small scenario the fuse tests share. The model recomputes the median descriptor and the mean direction
after every appended observation, as the reference does; the mirror computes them once per landmark at
the end, and the tests show that the maps are equal. Doubles are computed with Python floats in the
mirror's order of operations, so they are compared for equality."""
import math

import numpy as np

import ref_medoid as RM
from plba.slam_map import KF, Landmark, SlamMap

DB = 32


def rot_trans(T, p):
    return np.array([T[i, 0] * p[0] + T[i, 1] * p[1] + T[i, 2] * p[2] + T[i, 3] for i in range(3)])


def unit(v):
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return np.array([v[0] / n, v[1] / n, v[2] / n])


def update_average(lm, is_point):
    """updateAverageDescDir (src/mapFeatures.cpp:52-94, :140-184 with USE_LINE_PLUKER)."""
    if not lm.desc_list:
        return
    lm.med_desc = lm.desc_list[RM.medoid(np.array(lm.desc_list))].copy()
    if is_point:
        s = [0.0, 0.0, 0.0]
        for d in lm.dir_list:
            for k in range(3):
                s[k] += d[k]
        lm.med_dir = np.array([s[k] / len(lm.desc_list) for k in range(3)])


def fuse(m: SlamMap, feats, lc_idx_list, lc_pt_idxs, lc_ls_idxs):
    """Returns (the fused copy of m, line_geom {idx: (line3D, med_obs_dir)} of the new lines, stats)."""
    m = m.copy()
    for lm in m.lines:      # a line of the package's maps carries no directions
        if lm is not None and lm.dir_list is None:
            lm.dir_list = []
    fg = m.full_graph
    st = dict(rows=[[0] * 4, [0] * 4], null_skipped=[[0] * 4, [0] * 4], same_landmark=[0, 0], erased=[0, 0])
    line_geom = {}

    def bump(a, b):
        fg[a, b] += 1
        fg[b, a] += 1

    for kind, (loops, lms, kf_lists) in enumerate(((lc_pt_idxs, m.points, m.map_points_kf_idx),
                                                    (lc_ls_idxs, m.lines, m.map_lines_kf_idx))):
        is_point = kind == 0
        for lc, rows in enumerate(loops):
            if lc_idx_list[lc][2] != 1:
                continue
            kfp, kfc = lc_idx_list[lc][0], lc_idx_list[lc][1]
            fp, fc = feats[kfp], feats[kfc]
            idx_p = m.keyframes[kfp].pt_idx if is_point else m.keyframes[kfp].ls_idx
            idx_c = m.keyframes[kfc].pt_idx if is_point else m.keyframes[kfc].ls_idx

            def observation(kf, f, ldx):
                if is_point:
                    return f["pdesc"][ldx].copy(), np.array(f["pl"][ldx]), unit(f["P"][ldx])
                mid = [f["sP"][ldx][k] + f["eP"][ldx][k] for k in range(3)]
                return f["ldesc"][ldx].copy(), np.array(list(f["spl"][ldx]) + list(f["epl"][ldx])), unit(mid)

            def add_obs(lm, kf, f, ldx):
                desc, obs, d = observation(kf, f, ldx)
                lm.desc_list.append(desc)
                lm.obs_list.append(obs)
                lm.kf_obs_list.append(kf)
                lm.dir_list.append(d)
                lm.sigma_list.append(1.0)
                update_average(lm, is_point)

            for i0, l0, i1, l1 in rows:
                if i0 == -1 and i1 != -1:
                    if lms[i1] is not None:
                        idx_p[l0] = i1
                        add_obs(lms[i1], kfp, fp, l0)
                        for kf in lms[i1].kf_obs_list:
                            bump(kf, kfc)          # :5562 names kf_curr_idx
                        st["rows"][kind][0] += 1
                    else:
                        st["null_skipped"][kind][0] += 1
                if i0 != -1 and i1 == -1:
                    if lms[i0] is not None:
                        idx_c[l1] = i0
                        add_obs(lms[i0], kfc, fc, l1)
                        for kf in lms[i0].kf_obs_list:
                            bump(kf, kfp)          # :5579
                        st["rows"][kind][1] += 1
                    else:
                        st["null_skipped"][kind][1] += 1
                if i0 == -1 and i1 == -1:
                    new = len(lms)
                    idx_p[l0] = new
                    idx_c[l1] = new
                    Tp, Tc = m.keyframes[kfp].T_kf_w, m.keyframes[kfc].T_kf_w
                    if is_point:
                        P = rot_trans(Tp, fp["P"][l0])
                        lm = Landmark(idx=new, local=False, inlier=True, pos=P, desc_list=[fp["pdesc"][l0].copy()],
                                      obs_list=[np.array(fp["pl"][l0])], kf_obs_list=[kfp], sigma_list=[1.0], dir_list=[unit(P)])
                        lm.med_desc, lm.med_dir = lm.desc_list[0].copy(), lm.dir_list[0].copy()
                        kf_lists.setdefault(kfp, []).append(new)
                        P = rot_trans(Tc, fc["P"][l1])
                        lm.desc_list.append(fc["pdesc"][l1].copy())
                        lm.obs_list.append(np.array(fc["pl"][l1]))
                        lm.kf_obs_list.append(kfc)
                        lm.dir_list.append(unit(P))
                        lm.sigma_list.append(1.0)
                    else:
                        s, e = rot_trans(Tp, fp["sP"][l0]), rot_trans(Tp, fp["eP"][l0])
                        d = unit([0.5 * (s[k] + e[k]) for k in range(3)])
                        ndw = np.array([s[1] * e[2] - s[2] * e[1], s[2] * e[0] - s[0] * e[2], s[0] * e[1] - s[1] * e[0],
                                        e[0] - s[0], e[1] - s[1], e[2] - s[2]])
                        lm = Landmark(idx=new, local=False, inlier=True, pos=ndw, desc_list=[fp["ldesc"][l0].copy()],
                                      obs_list=[np.array(list(fp["spl"][l0]) + list(fp["epl"][l0]))], kf_obs_list=[kfp],
                                      sigma_list=[1.0], dir_list=[d])
                        lm.med_desc = lm.desc_list[0].copy()
                        line_geom[new] = (np.concatenate([s, e]), d.copy())
                        kf_lists.setdefault(kfp, []).append(new)
                        s, e = rot_trans(Tc, fc["sP"][l1]), rot_trans(Tc, fc["eP"][l1])
                        lm.desc_list.append(fc["ldesc"][l1].copy())
                        # :5746-5747: the current keyframe's spl, the previous keyframe's epl at lm_ldx1
                        lm.obs_list.append(np.array(list(fc["spl"][l1]) + list(fp["epl"][l1])))
                        lm.kf_obs_list.append(kfc)
                        lm.dir_list.append(unit([0.5 * (s[k] + e[k]) for k in range(3)]))
                        lm.sigma_list.append(1.0)
                    update_average(lm, is_point)
                    lms.append(lm)
                    bump(kfp, kfc)
                    st["rows"][kind][2] += 1
                if i0 != -1 and i1 != -1:
                    if i0 == i1:
                        st["same_landmark"][kind] += 1
                        continue
                    a, b = lms[i0], lms[i1]
                    if a is None or b is None:
                        st["null_skipped"][kind][3] += 1
                        continue
                    n_prev = len(a.kf_obs_list)
                    for it in range(len(b.desc_list)):
                        a.desc_list.append(b.desc_list[it])
                        a.obs_list.append(b.obs_list[it])
                        if it < len(b.dir_list):
                            a.dir_list.append(b.dir_list[it])
                        a.kf_obs_list.append(b.kf_obs_list[it])
                        a.sigma_list.append(b.sigma_list[it])
                        for i in range(n_prev):
                            bump(a.kf_obs_list[i], b.kf_obs_list[it])
                        update_average(a, is_point)
                        idx_c[l1] = i0
                    if b.kf_obs_list and b.kf_obs_list[0] in kf_lists and i1 in kf_lists[b.kf_obs_list[0]]:
                        kf_lists[b.kf_obs_list[0]].remove(i1)
                    lms[i1] = None
                    st["erased"][kind] += 1
                    st["rows"][kind][3] += 1
    return m, line_geom, st


# ---------------------------------------------------------------- the scenario
N_KF = 6
N_FEAT = 12            # features of each kind in every keyframe
LOOPS = [(0, 5, 1), (1, 4, 0), (1, 5, 1)]      # lc_idx_list: the second loop is already optimised


def _pose(rng):
    w = rng.normal(size=3) * 0.3
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.normal(size=3) * 2
    return T


def scenario(seed=11):
    """(SlamMap, feats, lc_idx_list, lc_pt_idxs, lc_ls_idxs). Landmark slots of each kind:
    3, 4: take one observation; 5 <- 6 <- fused, then 5 <- 9; 7, 8: guards; 10: NULL from the start;
    11 .. : background. Landmark 9 is missing from its first observer's kf-idx list."""
    rng = np.random.default_rng(seed)
    kfs = [KF(kf_idx=k, T_kf_w=_pose(rng), local=True, pt_idx=[-1] * N_FEAT, ls_idx=[-1] * N_FEAT) for k in range(N_KF)]
    observers = {0: [0, 1], 1: [1, 2, 3], 2: [2], 3: [2, 3, 4], 4: [0, 1, 2], 5: [0, 1, 2], 6: [3, 4, 5], 7: [1, 2],
                 8: [0, 5], 9: [4, 3, 2, 1], 11: [2, 3], 12: [0, 1, 2, 3, 4, 5], 13: [5], 14: [1, 4]}
    n_lm = 15

    def landmarks(is_point):
        out = []
        for idx in range(n_lm):
            if idx not in observers:
                out.append(None)
                continue
            n = len(observers[idx])
            base = rng.integers(0, 256, DB, dtype=np.uint8)
            descs = []
            for _ in range(n):
                d = base.copy()
                for p in rng.choice(8 * DB, size=int(rng.integers(0, 20)), replace=False):
                    d[p // 8] ^= np.uint8(1 << (p % 8))
                descs.append(d)
            lm = Landmark(idx=idx, local=True, inlier=True, pos=rng.normal(size=3 if is_point else 6) * 3,
                          desc_list=descs, obs_list=[rng.uniform(0, 600, 2 if is_point else 4) for _ in range(n)],
                          kf_obs_list=list(observers[idx]), sigma_list=[1.0] * n,
                          dir_list=[unit(rng.normal(size=3)) for _ in range(n)] if is_point else [])
            update_average(lm, is_point)
            out.append(lm)
        return out

    points, lines = landmarks(True), landmarks(False)
    kf_pt, kf_ln = {k: [] for k in range(N_KF)}, {k: [] for k in range(N_KF)}
    for lms, lists in ((points, kf_pt), (lines, kf_ln)):
        for lm in lms:
            if lm is not None and lm.idx != 9:
                lists[lm.kf_obs_list[0]].append(lm.idx)
    feats = {}
    for k in (0, 1, 4, 5):
        feats[k] = dict(pdesc=rng.integers(0, 256, (N_FEAT, DB), dtype=np.uint8), P=rng.normal(size=(N_FEAT, 3)) + [0, 0, 5],
                        pl=rng.uniform(0, 600, (N_FEAT, 2)), ldesc=rng.integers(0, 256, (N_FEAT, DB), dtype=np.uint8),
                        sP=rng.normal(size=(N_FEAT, 3)) + [0, 0, 5], eP=rng.normal(size=(N_FEAT, 3)) + [0, 0, 5],
                        le=rng.normal(size=(N_FEAT, 3)), spl=rng.uniform(0, 600, (N_FEAT, 2)), epl=rng.uniform(0, 600, (N_FEAT, 2)))
    rows0 = [(-1, 0, 3, 0),      # case 0: observation of kf_prev's feature added to landmark 3
             (4, 1, -1, 1),      # case 1: observation of kf_curr's feature added to landmark 4
             (-1, 2, -1, 2),     # case 2: a new landmark
             (5, 3, 6, 3),       # case 3: 6 fused into 5 and erased
             (6, 4, -1, 4),      # case 1 on the erased landmark: NULL guard
             (-1, 5, 6, 5),      # case 0 on it
             (7, 6, 6, 6),       # case 3, second landmark NULL
             (6, 7, 7, 7),       # case 3, first landmark NULL
             (8, 8, 8, 8),       # lm_idx0 == lm_idx1
             (5, 9, 9, 9),       # case 3 again into the fused landmark; 9 is in no kf-idx list
             (-1, 10, 5, 10),    # case 0 on the fused landmark
             (10, 11, -1, 11),   # case 1 on a landmark that was NULL from the start
             (-1, 3, -1, 0)]     # a second new landmark
    rows1 = [(-1, 0, -1, 0), (0, 1, 1, 1)]        # flag 0: left alone
    rows2 = [(-1, 0, 3, 10), (12, 1, 13, 11)]     # a later loop: landmark 3 again, and another fuse
    lc_rows = [rows0, rows1, rows2]
    for (kp, kc, _), rows in zip(LOOPS, lc_rows):    # the idx fields as isLoopClosure read them
        for i0, l0, i1, l1 in rows:
            kfs[kp].pt_idx[l0] = kfs[kp].ls_idx[l0] = i0
            kfs[kc].pt_idx[l1] = kfs[kc].ls_idx[l1] = i1
    m = SlamMap(fx=500.0, fy=500.0, cx=320.0, cy=240.0, keyframes=kfs, points=points, lines=lines,
                map_points_kf_idx=kf_pt, full_graph=rng.integers(0, 9, (N_KF, N_KF)).astype(np.uint32),
                map_lines_kf_idx=kf_ln, max_kf_idx=N_KF - 1)
    m.full_graph = np.triu(m.full_graph) + np.triu(m.full_graph, 1).T
    return m, feats, [list(l) for l in LOOPS], [list(r) for r in lc_rows], [list(r) for r in lc_rows]


def host_map(m, feats, lc_idx_list, lc_pt_idxs, lc_ls_idxs, medoid="cpu"):
    """A HostMap of the scenario with its features, loops and rows; ``medoid``: "cpu", None (device) or a hook."""
    from plba.slam_map import HostMap
    h = HostMap(m)
    for k, f in feats.items():
        h.set_keyframe_features(k, f["pdesc"], f["P"], f["pl"], f["ldesc"], f["sP"], f["eP"], f["le"])
        h.set_keyframe_line_endpoints(k, f["spl"], f["epl"])
    h.set_loop_closure(lc_idx_list, lc_idx_list, np.zeros((len(lc_idx_list), 6)))
    for lc in range(len(lc_idx_list)):
        h.set_lc_feature_idxs(1, lc, lc_pt_idxs[lc])
        h.set_lc_feature_idxs(2, lc, lc_ls_idxs[lc])
    h.set_medoid_fn(medoid)
    return h


def assert_maps_equal(h, want: SlamMap, line_geom=None):
    """The host map's state against the model's, entry by entry."""
    got = h.read(want)
    for kg, kw in zip(got.keyframes, want.keyframes):
        assert kg.pt_idx == list(kw.pt_idx) and kg.ls_idx == list(kw.ls_idx), kw.kf_idx
    for kind, (lg, lw) in enumerate(((got.points, want.points), (got.lines, want.lines))):
        assert not h.exists(kind + 1, len(lw))            # max_pt_idx / max_ls_idx: no slot past the model's
        for a, b in zip(lg, lw):
            assert (a is None) == (b is None), (kind, getattr(b, "idx", None))
            if b is None:
                continue
            assert a.kf_obs_list == list(b.kf_obs_list), (kind, b.idx)
            assert np.array_equal(np.array(a.obs_list), np.array(b.obs_list)), (kind, b.idx)
            assert a.sigma_list == list(b.sigma_list), (kind, b.idx)
            assert np.array_equal(a.med_desc, b.med_desc), (kind, b.idx)
            assert np.array_equal(a.pos, b.pos), (kind, b.idx)
            if kind == 0:
                assert np.array_equal(np.array(a.dir_list), np.array(b.dir_list)), b.idx
                assert np.array_equal(a.med_dir, b.med_dir), b.idx
    assert np.array_equal(got.full_graph, want.full_graph)
    assert got.map_points_kf_idx == want.map_points_kf_idx
    assert got.map_lines_kf_idx == want.map_lines_kf_idx
    for idx, (l3d, d) in (line_geom or {}).items():
        g3d, gd = h.line_geometry(idx)
        assert np.array_equal(g3d, l3d) and np.array_equal(gd, d), idx
