"""Seeded problems for plba_grid_match and their checker results (computed once per process).

A 640 x 480 image over the reference's 64 x 48 grid (10 pixels per cell). Train features sit at pixel
positions; the first min(n1, n2) queries are the same features displaced by up to 2 pixels, with up
to 8 descriptor bits flipped; further queries observe a train feature a second time (they compete for
its column), are rotated copies of a line (the direction test) or are random. Every eighth train row
is a distractor: a near copy, or an exact copy, of its neighbour a few pixels away (second-best
distances, ties). Some features lie outside the image, so some cells lie outside the grid."""
import functools

import numpy as np

import ref_gridmatch as R

COLS, ROWS, WIDTH, HEIGHT = 64, 48, 640.0, 480.0
INV_W, INV_H = COLS / WIDTH, ROWS / HEIGHT


def flip(rng, row, k):
    bits = np.unpackbits(np.asarray(row, np.uint8))
    bits[rng.permutation(bits.size)[:k]] ^= 1
    return np.packbits(bits)


def _cell(x, y):   # pair<int, int>(x * inv_width, y * inv_height): toward zero
    return int(x * INV_W), int(y * INV_H)


def _segment(mid, ang, length):
    h = 0.5 * length * np.array([np.cos(ang), np.sin(ang)])
    return mid - h, mid + h


def make(kind, n1, n2, desc_bytes=32, ws=3, nnr=0.9, seed=0, line_sim_th=0.75):
    rng = np.random.default_rng(1000 * seed + 7 * n1 + 31 * n2 + kind)
    desc2 = rng.integers(0, 256, (n2, desc_bytes), dtype=np.uint8)
    pos2 = rng.uniform([0, 0], [WIDTH, HEIGHT], (n2, 2))
    ang2 = rng.uniform(0, np.pi, n2)
    len2 = rng.uniform(4, 250, n2)
    if kind == 1 and n2 >= 2:
        pos2[0], len2[0] = (325.0, 245.0), 2.0             # one cell
        pos2[1], ang2[1], len2[1] = (320.0, 200.0), 0.02, 450.0  # 46 cells
    for j in range(7, n2, 8):   # distractors next to their neighbour
        pos2[j] = pos2[j - 1] + rng.uniform(-3, 3, 2)
        ang2[j] = ang2[j - 1] + rng.uniform(-0.05, 0.05)
        len2[j] = len2[j - 1]
        desc2[j] = flip(rng, desc2[j - 1], int(rng.integers(0, 4)) * (j % 16 == 7))   # exact copies too
    if n2 >= 12:
        pos2[9] = (-15.0, 100.0)                            # outside the image
    cells2, dir2 = [], np.zeros((n2, 2))
    for j in range(n2):
        if kind == 0:
            cells2.append(np.array([_cell(*pos2[j])], np.int32))
        else:
            s, e = _segment(pos2[j], ang2[j], len2[j])
            cells2.append(np.array(R.line_cells(s[0] * INV_W, s[1] * INV_H, e[0] * INV_W, e[1] * INV_H), np.int32))
            dir2[j] = R.normalize((e[0] - s[0]) * INV_W, (e[1] - s[1]) * INV_H)
    desc1 = rng.integers(0, 256, (n1, desc_bytes), dtype=np.uint8)
    cell1 = np.zeros((n1, 2), np.int32)
    cell1_end = np.zeros((n1, 2), np.int32)
    src = np.full(n1, -1, np.int64)
    n_disp = min(n1, n2)
    perm = rng.permutation(n2) if n2 else np.zeros(0, np.int64)
    for i in range(n1):
        how = 0 if i < n_disp else int(rng.integers(1, 4)) if n2 else 3
        if how == 0:
            j, nflip = int(perm[i]), int(rng.integers(0, 9))
        elif how in (1, 2):
            j, nflip = int(rng.integers(0, n2)), int(rng.integers(0, 13))
        if how == 3:
            p, a, ln = rng.uniform([-30, -30], [WIDTH + 30, HEIGHT + 30]), rng.uniform(0, np.pi), rng.uniform(4, 250)
        else:
            desc1[i] = flip(rng, desc2[j], nflip)
            p, a, ln = pos2[j] + rng.uniform(-2, 2, 2), ang2[j], len2[j]
            if how == 2 and kind == 1:
                a += np.pi / 3                               # fails the direction test
            if how == 0:
                src[i] = j
        if kind == 0:
            cell1[i] = _cell(*p)
        else:
            s, e = _segment(p, a, ln)
            if i % 5 == 0:
                s, e = e, s                                  # |dot|: the sense of a line does not matter
            cell1[i], cell1_end[i] = _cell(*s), _cell(*e)
    return dict(kind=kind, ws=ws, nnr=nnr, line_sim_th=line_sim_th, desc1=desc1, cell1=cell1,
                cell1_end=cell1_end if kind == 1 else None, desc2=desc2, cells2=cells2,
                dir2=dir2 if kind == 1 else None, src=src)


def record_chain(n_extra=43):
    """One train row and 257 + n_extra queries in its cell whose distances fall from 256 to 0 and then
    rise again: 257 records in one column; with best_lr only the query at distance 0 is matched."""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    order = rng.permutation(256)
    bits = np.unpackbits(t[0])
    rows = []
    for i in range(257 + n_extra):
        k = 256 - i if i <= 256 else i - 256
        b = bits.copy()
        b[order[:k]] ^= 1
        rows.append(np.packbits(b))
    n1 = len(rows)
    return dict(kind=0, ws=1, nnr=0.9, line_sim_th=0.75, desc1=np.array(rows, np.uint8),
                cell1=np.tile(np.array([[20, 20]], np.int32), (n1, 1)), cell1_end=None, desc2=t,
                cells2=[np.array([[21, 19]], np.int32)], dir2=None, src=np.zeros(n1, np.int64))


# (kind, n1, n2, desc_bytes, ws, nnr, seed)
def parity_cases():
    out = []
    for kind in (0, 1):
        for ws in (0, 1, 3):
            for nnr in (0.9, 1.5):
                out.append((kind, 300, 200, 32, ws, nnr, 0))
        out.append((kind, 280, 150, 64, 3, 0.9, 1))
        out.append((kind, 280, 150, 8, 1, 1.5, 1))
    return out


def boundary_cases():
    """Query rows around the LDS tile of 256, train rows around the wave of 64 and past 256."""
    out = [(0, n1, 130, 32, 3, 0.9, 2) for n1 in (1, 255, 256, 257, 513)]
    out += [(1, n1, 70, 32, 3, 0.9, 2) for n1 in (1, 256, 257)]
    out += [(0, 140, n2, 32, 3, 0.9, 3) for n2 in (1, 63, 64, 65, 257)]
    out += [(1, 90, n2, 32, 3, 1.5, 3) for n2 in (1, 63, 64, 65, 257)]
    return out


@functools.lru_cache(maxsize=None)
def problem(kind, n1, n2, desc_bytes, ws, nnr, seed):
    return make(kind, n1, n2, desc_bytes, ws, nnr, seed)


@functools.lru_cache(maxsize=None)
def reference(kind, n1, n2, desc_bytes, ws, nnr, seed, best_lr):
    m12, n = R.match_grid(problem(kind, n1, n2, desc_bytes, ws, nnr, seed), COLS, ROWS, best_lr)
    m12.setflags(write=False)
    return m12, n
