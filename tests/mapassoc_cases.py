"""Cases of the map-to-keyframe association (plba_map_associate): generated keyframes and the hand cases.
A keyframe is a dict with the keys of capi.MapassocBatchView: the candidate landmarks (pt_X, ls_X in the
world, with descriptors) and the keyframe's unmatched features. Among the candidates sit invisible rows, one
in every INVISIBLE_EVERY, of every way to be invisible in turn."""
import numpy as np

import kfassoc_cases as KC

WIDTH, HEIGHT, CAMERA, DB = KC.WIDTH, KC.HEIGHT, KC.CAMERA, KC.DB
back, proj = KC.back, KC.proj
INVISIBLE_EVERY = 3


def poses(T_kf_w=None):
    """T_kf_w (camera -> world) and Twf, its inverse, as the caller's."""
    T = KC.se3(0.03, -0.02, 0.015, [0.3, -0.1, 0.8]) if T_kf_w is None else T_kf_w
    return dict(T_kf_w=T, Twf=np.linalg.inv(T)[:3].copy())


def to_world(ps, P_cam):
    return (ps["T_kf_w"] @ np.append(P_cam, 1.0))[:3]


# an invisible point, in the camera frame: behind the camera (it projects inside the image), right of the
# image, below it, in the camera's plane, and one that is not finite
def _invisible(rng, k):
    u, v, z = rng.uniform(40, WIDTH - 40), rng.uniform(40, HEIGHT - 40), rng.uniform(2, 10)
    return (back(u, v, -z), back(WIDTH + 50.0, v, z), back(u, HEIGHT + 30.0, z), np.array([0.4, 0.2, 0.0]),
            np.array([np.nan, 0.0, 1.0]))[k % 5]


def points(rng, ps, n_m, n_f, far=0.0):
    """n_m candidate points, every INVISIBLE_EVERY-th invisible; the first features are partners of visible
    candidates, shuffled: three in four within the epipolar bound (under 0.6 px), one displaced by about 3.9 px;
    a share `far` of the partners sits 100 px away instead, out of the grid window but still a brute-force match."""
    X, vis = np.zeros((n_m, 3)), []
    for i in range(n_m):
        if i % INVISIBLE_EVERY == 1:
            X[i] = to_world(ps, _invisible(rng, i // INVISIBLE_EVERY))
        else:
            X[i] = to_world(ps, back(rng.uniform(30, WIDTH - 30), rng.uniform(30, HEIGHT - 30), rng.uniform(2, 10)))
            vis.append(i)
    d_m, d_f = KC._desc(rng, n_m), KC._desc(rng, n_f)
    pl = np.column_stack([rng.uniform(20, WIDTH - 20, n_f), rng.uniform(20, HEIGHT - 20, n_f)])
    rows = rng.permutation(vis)[:min(n_f, len(vis))]
    Twf4 = np.vstack([ps["Twf"], [0, 0, 0, 1]])
    for j, r in enumerate(rows):
        uv = proj((Twf4 @ np.append(X[r], 1.0))[:3])
        noise = rng.uniform(-0.4, 0.4, 2) if j % 4 != 3 else np.array([3.0, -2.5])
        if j < far * len(rows):
            noise = noise + np.array([100.0 if uv[0] < WIDTH / 2 else -100.0, 0.0])
        pl[j] = uv + noise
        d_f[j] = KC._partner(rng, d_m[r:r + 1])[0]
    P = np.array([back(u, v, z) for (u, v), z in zip(pl, rng.uniform(2, 10, n_f))]).reshape(-1, 3)
    return dict(pt_X=X, pdesc_m=d_m, pt_pl=pl, pt_P=P, pdesc_f=d_f, pt_partner_rows=np.asarray(rows))


def lines(rng, ps, n_m, n_f, far=0.0):
    """As points(). A partner feature is the candidate's projection shifted along its normal by 0.3 px, or by
    3 px for every third; le is the feature's own line with either sign, so the 3 px rows have an error of
    about +3 (rejected) or -3 (accepted: the test is signed)."""
    X, vis, seg = np.zeros((n_m, 6)), [], {}

    def segment():
        s = np.array([rng.uniform(40, WIDTH - 40), rng.uniform(40, HEIGHT - 40)])
        a, ln = rng.uniform(0, 2 * np.pi), rng.uniform(40, 120)
        e = np.clip(s + ln * np.array([np.cos(a), np.sin(a)]), 10, [WIDTH - 10, HEIGHT - 10])
        return s, e
    for i in range(n_m):
        s, e = segment()
        sP, eP = back(*s, rng.uniform(2, 10)), back(*e, rng.uniform(2, 10))
        if i % INVISIBLE_EVERY == 1:   # one endpoint out, the other, or both
            k = i // INVISIBLE_EVERY
            if k % 3 != 1:
                sP = _invisible(rng, k)
            if k % 3 != 0:
                eP = _invisible(rng, k + 1)
        else:
            vis.append(i)
            seg[i] = (s, e)
        X[i] = np.concatenate([to_world(ps, sP), to_world(ps, eP)])
    out = dict(ls_X=X, ldesc_m=KC._desc(rng, n_m), ls_spl=np.zeros((n_f, 2)), ls_epl=np.zeros((n_f, 2)), ls_le=np.zeros((n_f, 3)),
               ls_sP=np.zeros((n_f, 3)), ls_eP=np.zeros((n_f, 3)), ldesc_f=KC._desc(rng, n_f))
    rows = rng.permutation(vis)[:min(n_f, len(vis))]
    for j in range(n_f):
        if j < len(rows):
            s, e = seg[rows[j]]
            d = e - s
            nrm = np.array([-d[1], d[0]]) / np.hypot(*d)
            shift = (3.0 if j % 3 == 2 else 0.3) * nrm
            if j < far * len(rows):
                shift = shift + np.array([100.0 if min(s[0], e[0]) < WIDTH / 2 else -100.0, 0.0])
            s, e = s + shift, e + shift
            out["ldesc_f"][j] = KC._partner(rng, out["ldesc_m"][rows[j]:rows[j] + 1])[0]
        else:
            s, e = segment()
        le = np.cross(np.append(s, 1.0), np.append(e, 1.0))
        out["ls_spl"][j], out["ls_epl"][j] = s, e
        out["ls_le"][j] = le / np.hypot(le[0], le[1]) * (1 if (j // 3) % 2 else -1)
        out["ls_sP"][j], out["ls_eP"][j] = back(*s, rng.uniform(2, 10)), back(*e, rng.uniform(2, 10))
    out["ls_partner_rows"] = np.asarray(rows)
    return out


def keyframe(seed, n_pt=(0, 0), n_ls=(0, 0), far=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    p = poses()
    if n_pt[0] or n_pt[1]:
        p.update(points(rng, p, *n_pt, far=far[0]))
    if n_ls[0] or n_ls[1]:
        p.update(lines(rng, p, *n_ls, far=far[1]))
    return p


# name: (seed, candidates x features of the points, of the lines, the far share of either kind)
# n candidates hold n - (n + 1) // 3 visible rows
CASES = {
    "mixed": (11, (45, 30), (27, 18), (0.0, 0.0)),          # the grid stands for both kinds
    "pts_far": (12, (45, 30), (27, 18), (0.8, 0.0)),        # the grid finds too few points: only they fall back
    "lines_far": (13, (45, 30), (27, 18), (0.0, 0.9)),      # only the lines fall back
    "pts_300x130": (14, (300, 130), (0, 0), (0.0, 0.0)),    # a second block of 64 features, a second tile of 256 candidates
    "lines_40x70": (15, (0, 0), (40, 70), (0.0, 0.0)),      # a second block of line features
    "at_min": (16, (15, 12), (9, 8), (0.0, 0.0)),           # 10 visible points and 6 visible lines: never a fallback
    "above_min": (17, (16, 12), (10, 8), (0.0, 0.0)),       # 11 and 7 visible: 11 + 7 candidates take part
    "empty_sides": (18, (20, 0), (0, 9), (0.0, 0.0)),       # candidates without features, features without candidates
}
_cache = {}


def case(name):
    if name not in _cache:
        seed, n_pt, n_ls, far = CASES[name]
        _cache[name] = keyframe(seed, n_pt, n_ls, far)
    return _cache[name]


def identity_poses(t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, 3] = t
    return dict(Twf=np.eye(4)[:3].copy(), T_kf_w=T)


def hand_point():
    """Identity Twf, T_kf_w a translation by (1, 2, 3). The landmark (3, 4, 12) projects to (445, 400), cell
    (44, 40); the feature sits at (445.375, 400.5): err = 0.625 exactly; P = (6, 8, 24) has norm 26. A second
    feature far away gives the ratio test its second distance."""
    d = np.full((1, DB), 0x33, np.uint8)
    p = identity_poses((1.0, 2.0, 3.0))
    p.update(pt_X=[[3.0, 4.0, 12.0]], pdesc_m=d, pt_pl=[[445.375, 400.5], [10.0, 10.0]], pt_P=[[6.0, 8.0, 24.0], [0, 0, 1.0]],
             pdesc_f=np.vstack([d, ~d]))
    return p


def hand_line(le):
    """Identity poses. line3D (3, 4, 12) - (-3, 4, 12) projects to (445, 400) - (195, 400), cells (44, 40) and
    (19, 40); the feature is the segment (445, 400.25) - (195, 400.25) with the line le; sP = (0, 0, 4), eP =
    (6, 0, 4): the midpoint (3, 0, 4) has norm 5."""
    d = np.full((1, DB), 0x5A, np.uint8)
    p = identity_poses()
    p.update(ls_X=[[3.0, 4.0, 12.0, -3.0, 4.0, 12.0]], ldesc_m=d, ls_spl=[[445.0, 400.25]], ls_epl=[[195.0, 400.25]], ls_le=[le],
             ls_sP=[[0.0, 0.0, 4.0]], ls_eP=[[6.0, 0.0, 4.0]], ldesc_f=d.copy())
    return p


def boundary_points():
    """(keyframe, expected flags): identity poses, landmarks whose projection is exact. u = 320 + 500 x / z."""
    X = [[-3.2, 0.0, 5.0],    # u = 0: out
         [3.2, 0.0, 5.0],     # u = 640 = width: out
         [0.0, -2.5, 5.0],    # v = 0: out
         [0.0, 2.5, 5.0],     # v = 480 = height: out
         [0.1, 0.1, 0.0],     # z = 0: out
         [0.1, 0.1, -5.0],    # z < 0 (it projects inside the image): out
         [np.nan, 0.0, 5.0],  # NaN: out
         [0.0, 0.0, 5.0],     # the principal point: in
         [-3.125, 0.0, 5.0]]  # u = 7.5: in
    p = identity_poses()
    p.update(pt_X=X, pdesc_m=np.zeros((len(X), DB), np.uint8))
    return p, [0, 0, 0, 0, 0, 0, 0, 1, 1]


def boundary_lines():
    """A line with one endpoint out is invisible, whichever; one with both in is visible."""
    a, b, out = [0.0, 0.0, 5.0], [1.0, 1.0, 5.0], [3.2, 0.0, 5.0]
    p = identity_poses()
    p.update(ls_X=[a + b, a + out, out + b, out + out], ldesc_m=np.zeros((4, DB), np.uint8))
    return p, [1, 0, 0, 0]


def masking_keyframe():
    """Candidate 0 lies behind the camera and projects onto the very pixel of feature 0, whose descriptor it
    has exactly: the nearest candidate of feature 0, and invisible. Candidate 1 is visible, projects there
    too and differs from the feature by 5 bits: the runner-up. Candidate 2 is visible, far away and unlike
    anything, the second row that the feature side's ratio test needs; feature 1 is far away with the
    complement descriptor, the second row of the candidate side's. A matcher that sees candidate 0 gives it
    feature 0 and, with the left/right check, leaves candidate 1 without a match."""
    p = identity_poses()
    d = np.full((1, DB), 0xC3, np.uint8)
    d5 = d.copy()
    d5[0, 0] ^= 0x1F
    rng = np.random.default_rng(5)
    P = back(200.0, 150.0, 5.0)
    p.update(pt_X=np.array([-P, P, back(500.0, 400.0, 6.0)]), pdesc_m=np.vstack([d, d5, KC._desc(rng, 1)]),
             pt_pl=np.array([[200.25, 150.25], [60.0, 420.0]]), pt_P=np.array([P, back(60.0, 420.0, 4.0)]),
             pdesc_f=np.vstack([d, ~d]))
    return p


def two_on_one_keyframe():
    """Two visible candidates with one descriptor at the same place (an invisible row between them) and one
    feature there: without best_lr both match it."""
    p = identity_poses()
    P = back(200.0, 150.0, 5.0)
    d = np.full((1, DB), 0x5A, np.uint8)
    p.update(pt_X=np.array([P, -P, P]), pdesc_m=np.repeat(d, 3, 0), pt_pl=np.array([[200.0, 150.0], [500.0, 400.0]]),
             pt_P=np.array([P, back(500.0, 400.0, 5.0)]), pdesc_f=np.vstack([d, ~d]))
    return p
