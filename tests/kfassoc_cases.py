"""Cases of the keyframe-to-keyframe association (plba_kf_associate): generated keyframe pairs and the
hand cases. A pair is a dict with the keys of capi.KfassocBatchView."""
import numpy as np

WIDTH, HEIGHT = 640, 480
CAMERA = dict(width=WIDTH, height=HEIGHT, fx=500.0, fy=480.0, cx=320.0, cy=240.0)
DB = 32
# |err_curr| of a generated line pair, in turn: well inside, about 2.0 px (kept), about 3.0 px (rejected);
# the gate is sqrt(5.991) = 2.4477
ERR_NORMS = (0.4, 2.0, 3.0)


def se3(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def poses(T_prev=None, T_rel=None):
    """T_curr = T_prev T_rel (camera -> world), DT = inverse(T_curr) T_prev, the inverses as the caller's."""
    T_prev = se3(0.02, -0.03, 0.01, [0.4, -0.2, 1.5]) if T_prev is None else T_prev
    T_rel = se3(0.004, 0.01, -0.003, [0.05, 0.01, 0.12]) if T_rel is None else T_rel
    T_curr = T_prev @ T_rel
    DT = np.linalg.inv(T_curr) @ T_prev
    return dict(DT=DT[:3].copy(), T_prev=T_prev, T_curr=T_curr, Tcw_prev=np.linalg.inv(T_prev),
                Tcw_curr=np.linalg.inv(T_curr))


def back(u, v, z):
    return np.array([(u - CAMERA["cx"]) / CAMERA["fx"] * z, (v - CAMERA["cy"]) / CAMERA["fy"] * z, z])


def proj(P):
    return np.array([CAMERA["cx"] + CAMERA["fx"] * P[0] / P[2], CAMERA["cy"] + CAMERA["fy"] * P[1] / P[2]])


def _desc(rng, n):
    return rng.integers(0, 256, (n, DB), dtype=np.uint8)


def _partner(rng, d, flips=6):
    out = d.copy()
    for row in out:
        for bit in rng.choice(8 * DB, flips, replace=False):
            row[bit // 8] ^= np.uint8(1 << (bit % 8))
    return out


def _to_prev(ps, P_c):
    """a point of the current camera frame in the previous one: inverse(DT)"""
    DT = np.vstack([ps["DT"], [0, 0, 0, 1]])
    return (np.linalg.inv(DT) @ np.append(P_c, 1.0))[:3]


def points(rng, ps, n_p, n_c, share=0.85):
    """n_c current points; the first k = share * min previous rows are their partners, shuffled."""
    k = int(share * min(n_p, n_c))
    pl_c = np.column_stack([rng.uniform(20, WIDTH - 20, n_c), rng.uniform(20, HEIGHT - 20, n_c)])
    P_c = np.array([back(u, v, z) for (u, v), z in zip(pl_c, rng.uniform(2.0, 12.0, n_c))]).reshape(-1, 3)
    d_c = _desc(rng, n_c)
    P_p = np.array([back(rng.uniform(20, WIDTH - 20), rng.uniform(20, HEIGHT - 20), rng.uniform(2, 12))
                    for _ in range(n_p)]).reshape(-1, 3)
    d_p = _desc(rng, n_p)
    rows = rng.permutation(n_p)[:k]
    for j, r in enumerate(rows):
        P_p[r] = _to_prev(ps, P_c[j]) + rng.normal(0, 0.002, 3)
        d_p[r] = _partner(rng, d_c[j:j + 1])[0]
    return dict(pt_P_p=P_p, pdesc_p=d_p, pt_pl_c=pl_c, pt_P_c=P_c, pdesc_c=d_c, pt_partner_rows=np.asarray(rows))


def line_pair(ps, s_px, e_px, zs, ze, err_norm):
    """The previous row of a current segment: the same 3-D line in the previous camera, its Plücker
    coordinates there and its projection; the current segment is then shifted along its normal so that
    |err_curr| is about err_norm."""
    sP_c, eP_c = back(*s_px, zs), back(*e_px, ze)
    sP, eP = _to_prev(ps, sP_c), _to_prev(ps, eP_c)
    NDc = np.concatenate([np.cross(sP, eP), eP - sP])
    d = np.asarray(e_px, float) - np.asarray(s_px, float)
    nrm = np.array([-d[1], d[0]]) / np.hypot(*d) * err_norm / np.sqrt(2.0)
    return dict(sP=sP, eP=eP, NDc=NDc, spl=proj(sP), epl=proj(eP), spl_c=np.asarray(s_px, float) + nrm,
                epl_c=np.asarray(e_px, float) + nrm)


def world_pluker(T, ND):
    R, t = T[:3, :3], T[:3, 3]
    return np.concatenate([R @ ND[:3] + np.cross(t, R @ ND[3:]), R @ ND[3:]])


def lines(rng, ps, n_p, n_c, share=0.85):
    """As points(); every third partner row carries a landmark (ls_new 0, ls_lm_NDw its world line)."""
    k = int(share * min(n_p, n_c))
    out = dict(ls_sP_p=np.zeros((n_p, 3)), ls_eP_p=np.zeros((n_p, 3)), ls_NDc_p=np.zeros((n_p, 6)),
               ls_spl_p=np.zeros((n_p, 2)), ls_epl_p=np.zeros((n_p, 2)), ldesc_p=_desc(rng, n_p),
               ls_lm_NDw=np.zeros((n_p, 6)), ls_new=np.ones(n_p, np.uint8), ls_spl_c=np.zeros((n_c, 2)),
               ls_epl_c=np.zeros((n_c, 2)), ldesc_c=_desc(rng, n_c))

    def segment():
        s = np.array([rng.uniform(40, WIDTH - 40), rng.uniform(40, HEIGHT - 40)])
        a, ln = rng.uniform(0, 2 * np.pi), rng.uniform(30, 120)
        e = np.clip(s + ln * np.array([np.cos(a), np.sin(a)]), 5, [WIDTH - 5, HEIGHT - 5])
        return s, e, rng.uniform(2, 10), rng.uniform(2, 10)
    rows = list(rng.permutation(n_p)[:k])
    for r in range(n_p):   # a previous row without a partner: a line of its own
        lp = line_pair(ps, *segment(), 0.0)
        out["ls_sP_p"][r], out["ls_eP_p"][r], out["ls_NDc_p"][r] = lp["sP"], lp["eP"], lp["NDc"]
        out["ls_spl_p"][r], out["ls_epl_p"][r] = lp["spl"], lp["epl"]
    for j in range(n_c):
        lp = line_pair(ps, *segment(), ERR_NORMS[j % 3] if j < k else 0.0)
        out["ls_spl_c"][j], out["ls_epl_c"][j] = lp["spl_c"], lp["epl_c"]
        if j < k:
            r = rows[j]
            out["ls_sP_p"][r], out["ls_eP_p"][r], out["ls_NDc_p"][r] = lp["sP"], lp["eP"], lp["NDc"]
            out["ls_spl_p"][r], out["ls_epl_p"][r] = lp["spl"], lp["epl"]
            out["ldesc_p"][r] = _partner(rng, out["ldesc_c"][j:j + 1])[0]
            if (j // 3) % 2 == 0:   # an existing landmark, over all three error classes
                out["ls_new"][r] = 0
                out["ls_lm_NDw"][r] = world_pluker(ps["T_prev"], lp["NDc"])
    return out


def pair(seed, n_pt=(0, 0), n_ls=(0, 0)):
    rng = np.random.default_rng(seed)
    p = poses()
    if n_pt[0] or n_pt[1]:
        p.update(points(rng, p, *n_pt))
    if n_ls[0] or n_ls[1]:
        p.update(lines(rng, p, *n_ls))
    return p


# name: (seed, previous x current points, previous x current lines)
CASES = {
    "pts_70x70": (1, (70, 70), (0, 0)),        # crosses a wave
    "pts_300x130": (2, (300, 130), (0, 0)),    # crosses a 256 block
    "lines_40x40": (3, (0, 0), (40, 40)),
    "mixed": (4, (50, 45), (20, 22)),
    "empty_side": (5, (30, 0), (0, 12)),
    "pts_at_min": (6, (10, 10), (0, 0)),       # n == min_pt_matches: no fallback whatever the grid finds
    "pts_above_min": (7, (11, 11), (0, 0)),    # one above
}
_cache = {}


def case(name):
    if name not in _cache:
        seed, n_pt, n_ls = CASES[name]
        _cache[name] = pair(seed, n_pt, n_ls)
    return _cache[name]


def behind_camera_pair():
    """(pair, a, b): 'pts_above_min' with the previous row a behind the current camera and the row b in its
    plane z = 0; both are rows with a partner, and their descriptors still match it."""
    p = {k: np.array(v) for k, v in case("pts_above_min").items()}
    a, b = (int(r) for r in p["pt_partner_rows"][:2])
    DTi = np.linalg.inv(np.vstack([p["DT"], [0, 0, 0, 1]]))
    p["pt_P_p"][a] = (DTi @ [0.3, -0.2, -4.0, 1.0])[:3]
    p["pt_P_p"][b] = (DTi @ [0.5, 0.25, 0.0, 1.0])[:3]
    return p, a, b


def gate_pair(is_new, err_norm):
    """The hand case of the line gate: one line pair whose |err_curr| is about err_norm, the previous row new
    or carrying a landmark whose NDw is the same world line."""
    ps = poses()
    lp = line_pair(ps, (200.0, 120.0), (330.0, 260.0), 5.0, 7.0, err_norm)
    d = np.arange(DB, dtype=np.uint8).reshape(1, DB)
    return dict(ps, ls_sP_p=lp["sP"].reshape(1, 3), ls_eP_p=lp["eP"].reshape(1, 3), ls_NDc_p=lp["NDc"].reshape(1, 6),
                ls_spl_p=lp["spl"].reshape(1, 2), ls_epl_p=lp["epl"].reshape(1, 2), ldesc_p=d,
                ls_lm_NDw=(np.zeros((1, 6)) if is_new else world_pluker(ps["T_prev"], lp["NDc"]).reshape(1, 6)),
                ls_new=np.array([is_new], np.uint8), ls_spl_c=lp["spl_c"].reshape(1, 2), ls_epl_c=lp["epl_c"].reshape(1, 2),
                ldesc_c=d.copy())


def identity_poses():
    eye = np.eye(4)
    return dict(DT=eye[:3].copy(), T_prev=eye.copy(), T_curr=eye.copy(), Tcw_prev=eye.copy(), Tcw_curr=eye.copy())


def pixel_unit_pair():
    """The hand case of the pixel-unit line query: identity poses, one line through pixels (100, 100) -
    (140, 100) at depth 4 in both keyframes, equal descriptors. Its grid cells are (10, 10) and (14, 10); the
    reference queries (100, 100) and (140, 100), outside the 64 x 48 grid."""
    p = identity_poses()
    lp = line_pair(p, (100.0, 100.0), (140.0, 100.0), 4.0, 4.0, 0.0)
    d = np.arange(DB, dtype=np.uint8).reshape(1, DB)
    p.update(ls_sP_p=lp["sP"].reshape(1, 3), ls_eP_p=lp["eP"].reshape(1, 3), ls_NDc_p=lp["NDc"].reshape(1, 6),
             ls_spl_p=lp["spl"].reshape(1, 2), ls_epl_p=lp["epl"].reshape(1, 2), ldesc_p=d, ls_lm_NDw=np.zeros((1, 6)),
             ls_new=np.ones(1, np.uint8), ls_spl_c=lp["spl_c"].reshape(1, 2), ls_epl_c=lp["epl_c"].reshape(1, 2),
             ldesc_c=d.copy())
    return p


def two_on_one_pair():
    """Two previous points with one descriptor, at the same place, and one current point: without best_lr
    both match it."""
    p = identity_poses()
    P = back(200.0, 150.0, 5.0)
    d = np.full((1, DB), 0x5A, np.uint8)
    far = back(500.0, 400.0, 5.0)   # a second current row far away: the ratio test needs no second candidate
    p.update(pt_P_p=np.array([P, P]), pdesc_p=np.repeat(d, 2, 0), pt_pl_c=np.array([[200.0, 150.0], [500.0, 400.0]]),
             pt_P_c=np.array([P, far]), pdesc_c=np.vstack([d, ~d]))
    return p
