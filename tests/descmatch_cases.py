"""TEST INFRASTRUCTURE: seeded descriptor sets shared by tests/test_gpu_descmatch.py (device against
the checker) and tests/test_descmatch_oracle.py (the conditions on exactly these cases), and the
checker's results computed once for both.

Random 256-bit descriptors sit about 128 bits apart, so a 0.9 ratio almost never passes on them.
The generator plants what a matcher has to tell apart (disjoint rows for each kind):
  matches        desc1[a] = desc2[j] with a few flipped bits                (mutual, accepted)
  ratio rejects  desc2[j'] = desc2[j] and desc1[a] near both: d0 == d1       (a tie in d0, rejected
                 by the ratio test for every nnr <= 1; the index rule shows at nnr > 1)
  cross rejects  desc1[a'] = desc2[j] exactly and desc1[a] = desc2[j] with more flips: a -> j passes
                 the ratio test, but j -> a' in the reverse pass
"""
from __future__ import annotations

import functools

import numpy as np

import ref_descmatch

# (n1, n2): one and two rows, an empty side, around one tile of 256 rows, several tiles on one side
SHAPES = [(1, 2), (2, 1), (5, 0), (0, 5), (255, 257), (256, 256), (257, 255), (300, 1000)]
NNRS = [0.9, 0.6, 1.0]
DESC_BYTES = [8, 32, 64]
# the shapes large enough to hold every planted kind: the conditions of test_descmatch_oracle hold here
PLANTED_MIN_ROWS = 64
N_RATIO, N_CROSS = 3, 3


def _flip(rng, row: np.ndarray, k: int) -> np.ndarray:
    bits = np.unpackbits(row)
    pos = rng.choice(len(bits), k, replace=False)
    bits[pos] ^= 1
    return np.packbits(bits)


@functools.lru_cache(maxsize=None)
def pair(n1: int, n2: int, desc_bytes: int = 32, seed: int = 0):
    """(desc1 [n1][desc_bytes], desc2 [n2][desc_bytes]) uint8, read-only."""
    rng = np.random.default_rng(10007 * seed + 131 * n1 + 17 * n2 + desc_bytes)
    d1 = rng.integers(0, 256, (n1, desc_bytes), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, desc_bytes), dtype=np.uint8)
    bits = 8 * desc_bytes
    m = min(n1, n2)
    p1, p2 = rng.permutation(n1), rng.permutation(n2)
    u1 = u2 = 0
    if m >= PLANTED_MIN_ROWS:
        for _ in range(N_RATIO):
            a, j, j2 = p1[u1], p2[u2], p2[u2 + 1]
            u1, u2 = u1 + 1, u2 + 2
            d2[j2] = d2[j]
            d1[a] = _flip(rng, d2[j], 1)
        for _ in range(N_CROSS):
            a, a2, j = p1[u1], p1[u1 + 1], p2[u2]
            u1, u2 = u1 + 2, u2 + 1
            d1[a2] = d2[j]
            d1[a] = _flip(rng, d2[j], bits // 16)
    for _ in range(m // 2 if m >= 4 else 0):   # half of the smaller side is a true match
        a, j = p1[u1], p2[u2]
        u1, u2 = u1 + 1, u2 + 1
        d1[a] = _flip(rng, d2[j], int(rng.integers(0, bits // 64 + 1)))
    d1.setflags(write=False)
    d2.setflags(write=False)
    return d1, d2


@functools.lru_cache(maxsize=None)
def reference(n1: int, n2: int, desc_bytes: int, nnr: float, best_lr: bool, seed: int = 0):
    """The checker's result of pair(...) (read-only: shared by the tests)."""
    d1, d2 = pair(n1, n2, desc_bytes, seed)
    return ref_descmatch.match_detail(d1, d2, np.float32(nnr), best_lr)


def parity_cases():
    """(n1, n2, desc_bytes, nnr): every shape at 32 bytes, the other widths around the tile size."""
    out = [(s[0], s[1], 32, r) for s in SHAPES for r in NNRS]
    out += [(257, 255, db, r) for db in DESC_BYTES if db != 32 for r in NNRS]
    return out


# ---- two keyframes for isLoopClosure: lcpose_cases geometry with planted descriptors
@functools.lru_cache(maxsize=None)
def keyframe_pair(n_match_pt: int = 40, n_match_ln: int = 12, extra=(30, 20, 8, 5), seed: int = 0, outlier_frac: float = 0.25):
    """Features of an old keyframe kf0 and a new one kf1 that see the same place: the matched
    features are an lcpose_cases problem (P / sP / eP of kf0, pl / le of kf1), shuffled among
    ``extra`` = (kf0 points, kf1 points, kf0 lines, kf1 lines) unmatched features with random
    descriptors. Returns (kf0, kf1, true): dicts of pdesc, P, pl, ldesc, sP, eP, le, and the
    planted (i1, i2) rows of points and lines in i1 order."""
    import lcpose_cases
    pr = lcpose_cases.problem(n_match_pt, n_match_ln, outlier_frac)
    rng = np.random.default_rng(777 + seed)

    def kind(n_match, x0, x1):
        n0, n1 = n_match + x0, n_match + x1
        s0, s1 = rng.permutation(n0)[:n_match], rng.permutation(n1)[:n_match]
        desc0 = rng.integers(0, 256, (n0, 32), dtype=np.uint8)
        desc1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
        for a, j in zip(s0, s1):
            desc1[j] = _flip(rng, desc0[a], int(rng.integers(0, 5)))
        return n0, n1, s0, s1, desc0, desc1

    n0, n1, s0, s1, pd0, pd1 = kind(n_match_pt, extra[0], extra[1])
    P0, pl0 = rng.normal(0, 1, (n0, 3)) + [0, 0, 5], rng.uniform(50, 400, (n0, 2))
    P1, pl1 = rng.normal(0, 1, (n1, 3)) + [0, 0, 5], rng.uniform(50, 400, (n1, 2))
    P0[s0], pl1[s1] = pr.pt_P, pr.pt_obs
    m0, m1, t0, t1, ld0, ld1 = kind(n_match_ln, extra[2], extra[3])
    sP0, eP0, le0 = (rng.normal(0, 1, (m0, 3)) + [0, 0, 5] for _ in range(3))
    sP1, eP1, le1 = (rng.normal(0, 1, (m1, 3)) + [0, 0, 5] for _ in range(3))
    sP0[t0], eP0[t0], le1[t1] = pr.ln_sP, pr.ln_eP, pr.ln_le
    kf0 = dict(pdesc=pd0, P=P0, pl=pl0, ldesc=ld0, sP=sP0, eP=eP0, le=le0)
    kf1 = dict(pdesc=pd1, P=P1, pl=pl1, ldesc=ld1, sP=sP1, eP=eP1, le=le1)
    o, q = np.argsort(s0), np.argsort(t0)
    true = dict(pt=np.stack([s0[o], s1[o]], 1), ln=np.stack([t0[q], t1[q]], 1))
    return kf0, kf1, true


def unrelated_keyframe(n_pt: int = 70, n_ls: int = 20, seed: int = 1):
    """A keyframe of another place: random descriptors, no match with anything."""
    rng = np.random.default_rng(4242 + seed)
    return dict(pdesc=rng.integers(0, 256, (n_pt, 32), dtype=np.uint8), P=rng.normal(0, 1, (n_pt, 3)) + [0, 0, 5],
                pl=rng.uniform(50, 400, (n_pt, 2)), ldesc=rng.integers(0, 256, (n_ls, 32), dtype=np.uint8),
                sP=rng.normal(0, 1, (n_ls, 3)) + [0, 0, 5], eP=rng.normal(0, 1, (n_ls, 3)) + [0, 0, 5],
                le=rng.normal(0, 1, (n_ls, 3)))
