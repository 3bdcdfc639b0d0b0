"""A small synthetic map for MapHandler::matchMap2KFPoints / Lines (src/mapHandler.cpp:697-921) and a
Python model of both functions over it (grid matching by tests/ref_gridmatch.py, the fallback by
tests/ref_descmatch.py). Keyframes 0..3 look down +z; keyframe 3 is the new one. Its first features are
re-observations of map landmarks (a pixel of noise at most, a few flipped descriptor bits), some of
them displaced by several pixels (the epipolar test rejects those), the rest are random."""
import numpy as np

import gridmatch_cases as gcases
import ref_descmatch
import ref_gridmatch as R
from plba.slam_map import KF, Landmark, SlamMap

CAM = (400.0, 400.0, 320.0, 240.0)
WIDTH, HEIGHT, KF_NEW = 640, 480, 3
INV_W, INV_H = 64 / float(WIDTH), 48 / float(HEIGHT)


def transform(T, X):
    """Twf * X with the mirror's operation order."""
    return np.array([T[r, 0] * X[0] + T[r, 1] * X[1] + T[r, 2] * X[2] + T[r, 3] for r in range(3)])


def project(T, X):
    P = transform(T, X)
    fx, fy, cx, cy = CAM
    return np.array([cx + fx * P[0] / P[2], cy + fy * P[1] / P[2]]), P


def in_image(uv, P):
    return 0 < uv[0] < WIDTH and 0 < uv[1] < HEIGHT and P[2] > 0.0


def build(seed=0, n_pt=60, n_ln=30):
    """(SlamMap, line3D [n_ln][6], features of keyframe 3, Twf)."""
    rng = np.random.default_rng(seed)
    kfs = []
    for k in range(4):
        T = np.eye(4)
        T[0, 3] = 0.1 * k
        kfs.append(KF(k, T, True, [], []))
    Twf = np.eye(4)
    Twf[0, 3] = -0.1 * KF_NEW

    def lm(idx, pos, width, kf_list, local):
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        n = len(kf_list)
        return Landmark(idx=idx, local=local, inlier=True, pos=np.array(pos, np.float64), desc_list=[d.copy() for _ in range(n)],
                        obs_list=[rng.uniform(0, 400, width) for _ in range(n)], kf_obs_list=list(kf_list),
                        sigma_list=[1.0] * n, dir_list=[np.array([0.0, 0.0, 1.0])] * n if width == 2 else None)

    def xyz():
        return np.array([rng.uniform(-2.5, 2.5), rng.uniform(-1.8, 1.8), rng.uniform(4, 8)])
    points, lines, line3d = [], [], []
    for i in range(n_pt):
        X = xyz()
        if i % 15 == 14:
            X[2] = -3.0                                     # behind the camera
        seen_by_new = i % 10 == 9
        points.append(lm(i, X, 2, [0, 1, KF_NEW] if seen_by_new else ([0, 1] if i % 2 else [1]), i % 12 != 11))
    for i in range(n_ln):
        a = xyz()
        b = a + rng.uniform(-1.2, 1.2, 3) * np.array([1, 1, 0.3])
        seen_by_new = i % 10 == 9
        lines.append(lm(i, rng.normal(size=6), 4, [0, 2, KF_NEW] if seen_by_new else [0, 2], i % 12 != 11))
        line3d.append(np.concatenate([a, b]))
    feat = dict(pdesc=[], P=[], pl=[], ldesc=[], sP=[], eP=[], le=[], spl=[], epl=[])
    pt_idx, ls_idx = [], []
    for i, p in enumerate(points):
        uv, P = project(Twf, p.pos)
        if i % 4 == 3 and i % 10 != 9:
            continue                                        # no feature for this landmark
        noise = rng.uniform(-0.3, 0.3, 2) + (np.array([4.0, -3.0]) if i % 7 == 6 else 0)
        feat["pdesc"].append(gcases.flip(rng, p.desc_list[0], int(rng.integers(0, 7))))
        feat["P"].append(P)
        feat["pl"].append(uv + noise)
        pt_idx.append(i if i % 10 == 9 else -1)
    for _ in range(12):                                     # features of nothing in the map
        feat["pdesc"].append(rng.integers(0, 256, 32, dtype=np.uint8))
        feat["P"].append(xyz())
        feat["pl"].append(rng.uniform([0, 0], [WIDTH, HEIGHT]))
        pt_idx.append(-1)
    for i, l in enumerate(lines):
        (s, sP), (e, eP) = project(Twf, line3d[i][:3]), project(Twf, line3d[i][3:])
        if i % 4 == 3 and i % 10 != 9:
            continue
        shift = np.array([0.0, 5.0]) if i % 7 == 6 else 0
        s, e = s + rng.uniform(-0.3, 0.3, 2) + shift, e + rng.uniform(-0.3, 0.3, 2) + shift
        le = np.cross(np.append(s, 1.0), np.append(e, 1.0))   # the feature's own line
        le = le / np.hypot(le[0], le[1]) * (1 if i % 2 else -1)
        feat["ldesc"].append(gcases.flip(rng, l.desc_list[0], int(rng.integers(0, 7))))
        for k, v in (("sP", sP), ("eP", eP), ("le", le), ("spl", s), ("epl", e)):
            feat[k].append(v)
        ls_idx.append(i if i % 10 == 9 else -1)
    feat = {k: np.array(v) for k, v in feat.items()}
    kfs[KF_NEW].pt_idx, kfs[KF_NEW].ls_idx = pt_idx, ls_idx
    fg = rng.integers(0, 20, (4, 4)).astype(np.uint32)
    fg = fg + fg.T
    for lms in (points, lines):
        for x in lms:
            x.med_desc = x.desc_list[0]
    m = SlamMap(*CAM, keyframes=kfs, points=points, lines=lines, map_points_kf_idx={}, full_graph=fg, max_kf_idx=KF_NEW)
    return m, np.array(line3d), feat, Twf


def model(m, line3d, feat, Twf, p):
    """matchMap2KFPoints + matchMap2KFLines on (a copy of) the map: what the mirror must leave behind."""
    kf = m.keyframes[KF_NEW]
    out = dict(pt_idx=list(kf.pt_idx), ls_idx=list(kf.ls_idx), full_graph=m.full_graph.astype(np.int64).copy(),
               new_obs={1: {}, 2: {}}, stats=dict(visible=[0, 0], unmatched=[0, 0], grid_matches=[0, 0], fallback=[0, 0],
                                                   accepted=[0, 0], rejected=[0, 0]))
    st = out["stats"]
    for kind, lms, idx_list, mn, nnr_l in ((0, m.points, out["pt_idx"], p.min_pt_matches, p.min_ratio_12_p),
                                           (1, m.lines, out["ls_idx"], p.min_ls_matches, p.min_ratio_12_l)):
        if not (p.has_lines if kind else p.has_points) or not idx_list:
            continue
        local, cell1, cell1_end = [], [], []
        for lmk in lms:
            if lmk is None or not lmk.local or lmk.kf_obs_list[-1] == KF_NEW:
                continue
            if kind == 0:
                uv, P = project(Twf, lmk.pos)
                if not in_image(uv, P):
                    continue
                cell1.append((int(uv[0] * INV_W), int(uv[1] * INV_H)))
            else:
                (s, sP), (e, eP) = project(Twf, line3d[lmk.idx][:3]), project(Twf, line3d[lmk.idx][3:])
                if not (in_image(s, sP) and in_image(e, eP)):
                    continue
                cell1.append((int(s[0] * INV_W), int(s[1] * INV_H)))
                cell1_end.append((int(e[0] * INV_W), int(e[1] * INV_H)))
            local.append(lmk)
        um = [i for i, v in enumerate(idx_list) if v == -1]
        st["visible"][kind], st["unmatched"][kind] = len(local), len(um)
        if not local or not um:
            continue
        desc1 = np.array([x.med_desc for x in local], np.uint8)
        desc2 = (feat["ldesc"] if kind else feat["pdesc"])[um]
        m12, matches = np.full(len(local), -1), 0
        if p.fast_matching:
            if kind == 0:
                cells2 = [np.array([[int(feat["pl"][i][0] * INV_W), int(feat["pl"][i][1] * INV_H)]]) for i in um]
                dir2 = None
            else:
                cells2 = [np.array(R.line_cells(feat["spl"][i][0] * INV_W, feat["spl"][i][1] * INV_H, feat["epl"][i][0] * INV_W,
                                                feat["epl"][i][1] * INV_H)) for i in um]
                dir2 = np.array([R.normalize((feat["epl"][i][0] - feat["spl"][i][0]) * INV_W,
                                             (feat["epl"][i][1] - feat["spl"][i][1]) * INV_H) for i in um])
            pb = dict(kind=kind, ws=p.ws, nnr=p.min_ratio_12_p, line_sim_th=p.line_sim_th, desc1=desc1,
                      cell1=np.array(cell1), cell1_end=np.array(cell1_end) if kind else None, desc2=desc2, cells2=cells2,
                      dir2=dir2)
            m12, matches = R.match_grid(pb, 64, 48, bool(p.best_lr))
        st["grid_matches"][kind] = matches
        if len(local) > mn and matches < mn:
            st["fallback"][kind] = 1
            m12, matches = ref_descmatch.match(desc1, desc2, np.float32(nnr_l), bool(p.best_lr))
        for i1, i2 in enumerate(m12):
            if i2 < 0:
                continue
            lmk, fi = local[i1], um[i2]
            if kind == 0:
                uv, _ = project(Twf, lmk.pos)
                ok = np.sqrt((uv[0] - feat["pl"][fi][0]) ** 2 + (uv[1] - feat["pl"][fi][1]) ** 2) < p.max_kf_epip_p
                obs = feat["pl"][fi]
            else:
                (s, _), (e, _) = project(Twf, line3d[lmk.idx][:3]), project(Twf, line3d[lmk.idx][3:])
                le = feat["le"][fi]
                ok = (le[0] * s[0] + le[1] * s[1] + le[2] < p.max_kf_epip_l) and (le[0] * e[0] + le[1] * e[1] + le[2] < p.max_kf_epip_l)
                obs = np.concatenate([feat["spl"][fi], feat["epl"][fi]])
            if not ok:
                st["rejected"][kind] += 1
                continue
            st["accepted"][kind] += 1
            idx_list[fi] = lmk.idx
            out["new_obs"][kind + 1][lmk.idx] = obs
            for o in lmk.kf_obs_list:
                if o != KF_NEW:
                    out["full_graph"][KF_NEW, o] += 1
                    out["full_graph"][o, KF_NEW] += 1
    return out
