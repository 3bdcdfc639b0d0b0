"""Synthetic stereo frames for plba_stereo_associate: detector output of a left and a right image (float32
keypoints and segments, 32-byte descriptors) in which a known share of the left rows has a true partner
on the right. The partners are built so that every gate and the window's asymmetry both reject and pass
rows (tests/test_stereo_oracle.py asserts it on the checker's output), and the right rows are shuffled so
that indices do not line up."""
import numpy as np

import gridmatch_cases as gcases

WIDTH, HEIGHT = 640, 480
CAMERA = dict(width=WIDTH, height=HEIGHT, fx=400.0, fy=410.0, cx=318.5, cy=241.25, b=0.12)
DB = 32


def _desc(rng, n):
    return rng.integers(0, 256, (n, DB), dtype=np.uint8)


def points(rng, n_l, n_r, share=0.9):
    """pt_l [n_l][2], pdesc_l, pt_r [n_r][2], pdesc_r."""
    pl = np.stack([rng.uniform(30, WIDTH - 30, n_l), rng.uniform(20, HEIGHT - 20, n_l)], axis=1).astype(np.float32)
    dl = _desc(rng, n_l)
    pr = np.stack([rng.uniform(0, WIDTH, n_r), rng.uniform(0, HEIGHT, n_r)], axis=1).astype(np.float32)
    dr = _desc(rng, n_r)
    k = int(np.ceil(min(n_l, n_r) * share))
    left = rng.permutation(n_l)[:k]
    for j, i in enumerate(left):
        kind = j % 10
        disp = rng.uniform(2.0, 60.0)
        dy = rng.uniform(-0.7, 0.7)
        if kind == 7:
            disp = rng.uniform(-1.5, 0.9)                 # the disparity gate
        elif kind == 8:
            dy = rng.choice([-1, 1]) * rng.uniform(1.2, 3.0)   # the epipolar gate
        if kind == 9 and j + 1 < k:
            # a decoy with the left row's own descriptor one cell to the right or one row below: inside a
            # symmetric window, outside the stereo window; the true partner has a few bits flipped
            j2 = j + 1 if j + 1 < n_r else j
            off = (12.0, 0.0) if (j // 10) % 2 else (0.0, 12.0)
            pr[j2] = (pl[i, 0] + off[0], pl[i, 1] + off[1])
            dr[j2] = dl[i]
        if kind == 0 and j > 0 and (j - 1) % 10 == 9:
            continue                                       # this right row is the decoy above
        pr[j] = (pl[i, 0] - disp, pl[i, 1] + dy)
        dr[j] = gcases.flip(rng, dl[i], int(rng.integers(1, 6)))
    perm = rng.permutation(n_r)
    return dict(pt_l=pl, pdesc_l=dl, pt_r=np.ascontiguousarray(pr[perm]), pdesc_r=np.ascontiguousarray(dr[perm]))


def lines(rng, n_l, n_r, share=0.9, outside=False):
    """ls_l [n_l][4], ldesc_l, ls_r [n_r][4], ldesc_r: long diagonals, many cells per line."""
    lo, hi = (-0.6, 1.6) if outside else (0.05, 0.95)

    def segs(n):
        s = np.stack([rng.uniform(lo * WIDTH, hi * WIDTH, n), rng.uniform(lo * HEIGHT, hi * HEIGHT, n)], axis=1)
        ang = rng.uniform(0.25, np.pi - 0.25, n) * rng.choice([-1, 1], n)
        length = rng.uniform(60, 320, n)
        e = s + length[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        e[:, 0] = np.clip(e[:, 0], -0.9 * WIDTH, 1.9 * WIDTH)
        e[:, 1] = np.clip(e[:, 1], -0.9 * HEIGHT, 1.9 * HEIGHT)
        return np.concatenate([s, e], axis=1)
    ll = segs(n_l)
    dl = _desc(rng, n_l)
    lr = segs(n_r)
    dr = _desc(rng, n_r)
    k = int(np.ceil(min(n_l, n_r) * share))
    left = rng.permutation(n_l)[:k]
    for j, i in enumerate(left):
        kind = j % 10
        sx, sy, ex, ey = ll[i]
        if kind == 4:                                      # a horizontal left line: the third and fourth gate
            ey = sy + rng.uniform(-0.08, 0.08)
            ll[i] = (sx, sy, ex, ey)
        ds = rng.uniform(3.0, 50.0)
        de = ds * rng.uniform(0.8, 1.25)
        if kind == 5:
            de = ds * rng.uniform(0.3, 0.6)                # the disparity ratio: both disparities become -1
        elif kind == 6:
            ds, de = rng.uniform(0.75, 0.95), rng.uniform(1.0, 1.05)   # only the start's disparity is too small
        elif kind == 7:
            ds, de = rng.uniform(1.0, 1.05), rng.uniform(0.75, 0.95)   # only the end's
        u0, u1 = rng.uniform(-0.05, 0.1), rng.uniform(0.9, 1.05)
        if kind == 8:
            u0, u1 = rng.uniform(0.0, 0.1), rng.uniform(0.35, 0.6)     # the right segment covers half: overlap
        if kind == 9:
            u0, u1 = u1, u0                                            # the right segment runs the other way

        def right(u):                                       # the point of the right line at the height u of the left
            return sx + u * (ex - sx) - (ds + u * (de - ds)), sy + u * (ey - sy)
        lr[j] = right(u0) + right(u1)
        dr[j] = gcases.flip(rng, dl[i], int(rng.integers(1, 6)))
    perm = rng.permutation(n_r)
    return dict(ls_l=ll.astype(np.float32), ldesc_l=dl, ls_r=np.ascontiguousarray(lr[perm]).astype(np.float32),
                ldesc_r=np.ascontiguousarray(dr[perm]))


def frame(seed, n_pt=(0, 0), n_ls=(0, 0), outside=False):
    rng = np.random.default_rng(seed)
    f = {}
    if max(n_pt):
        f.update(points(rng, *n_pt))
    if max(n_ls):
        f.update(lines(rng, *n_ls, outside=outside))
    return f


# the smallest shapes that reach every path: name -> (seed, points left x right, lines left x right, outside)
CASES = {
    "left_empty": (1, (0, 5), (0, 5), False),
    "right_empty": (2, (5, 0), (5, 0), False),
    "one": (3, (1, 1), (1, 1), False),
    "pts_70x70": (4, (70, 70), (0, 0), False),            # two 64-row train blocks
    "pts_300x130": (5, (300, 130), (0, 0), False),        # two 256-row query tiles
    "lines_40x40": (6, (0, 0), (40, 40), False),          # long diagonals, many cells per line
    "lines_outside": (7, (0, 0), (30, 34), True),         # endpoints outside the image: cells outside the grid
    "mixed": (8, (50, 45), (20, 22), False),
}
LARGEST = "pts_300x130"


def case(name):
    seed, n_pt, n_ls, outside = CASES[name]
    return frame(seed, n_pt, n_ls, outside)


# ---- the hand case of the window's asymmetry, shared by the checker's, the CPU restatement's and the
# device's test. A camera with exactly representable values; 10 px a cell.
HAND_CAMERA = dict(width=640, height=480, fx=512.0, fy=256.0, cx=320.0, cy=240.0, b=0.125)


def bits_desc(*bits):
    """A 32-byte descriptor with the given bits set."""
    d = np.zeros(256, np.uint8)
    d[list(bits)] = 1
    return np.packbits(d)


def asymmetric_window_frames():
    """Two frames with one left point at (328, 248), query cell (32, 24). Its true partner, 10 px to the left
    in cell 31, is at Hamming distance 1; a decoy at distance 0 sits one cell to the right (cell 33) in the
    first frame and one row below (row 25) in the second. A symmetric window takes the decoy; the stereo
    window [x - 10, x] x [y, y] must give the partner: one survivor with disparity 10, right row 1."""
    frames = []
    for decoy in ((338.0, 248.0), (328.0, 258.0)):
        frames.append(dict(pt_l=np.array([(328.0, 248.0)], np.float32), pdesc_l=np.array([bits_desc(0, 1, 2, 3)]),
                           pt_r=np.array([decoy, (318.0, 248.0)], np.float32),
                           pdesc_r=np.array([bits_desc(0, 1, 2, 3), bits_desc(0, 1, 2)])))
    return frames
