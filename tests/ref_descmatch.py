"""TEST INFRASTRUCTURE: numpy checker of plba_desc_match (include/plba.h), that is of StVO::match /
StVO::matchNNR (src2/matching.cpp:41-91): Hamming distances by np.unpackbits, a stable argsort for
the tie rule (the lowest train index among equal distances comes first, which is what a scan in
increasing index with strict comparisons keeps), np.float32 arithmetic for the ratio test."""
from __future__ import annotations

import numpy as np


def hamming(desc1: np.ndarray, desc2: np.ndarray) -> np.ndarray:
    """[n1][n2] Hamming distances of uint8 rows (exact: counts up to 512 in float32 products)."""
    a = np.unpackbits(np.asarray(desc1, np.uint8), axis=1).astype(np.float32)
    b = np.unpackbits(np.asarray(desc2, np.uint8), axis=1).astype(np.float32)
    return np.rint(a @ (1.0 - b).T + (1.0 - a) @ b.T).astype(np.int64)


def nearest(desc1: np.ndarray, desc2: np.ndarray, nnr) -> dict:
    """matchNNR for one direction. ``matches``: the train row or -1; ``d0`` / ``d1`` / ``i0``: the two
    smallest distances and the best row before the ratio test; ``tie``: the best distance is shared."""
    n1, n2 = len(desc1), len(desc2)
    none = np.full(n1, -1, np.int64)
    if n2 < 2 or n1 == 0:   # defined here: fewer than 2 train rows give no match
        return dict(matches=none, d0=none.copy(), d1=none.copy(), i0=none.copy(), tie=np.zeros(n1, bool))
    D = hamming(desc1, desc2)
    order = np.argsort(D, axis=1, kind="stable")
    rows = np.arange(n1)
    i0 = order[:, 0]
    d0, d1 = D[rows, i0], D[rows, order[:, 1]]
    ok = d0.astype(np.float32) < d1.astype(np.float32) * np.float32(nnr)   # matching.cpp:54, in float
    return dict(matches=np.where(ok, i0, -1), d0=d0, d1=d1, i0=i0, tie=d0 == d1)


def match_detail(desc1, desc2, nnr, best_lr: bool = True) -> dict:
    fwd, rev = nearest(desc1, desc2, nnr), nearest(desc2, desc1, nnr)
    m12 = fwd["matches"].copy()
    if best_lr:   # matching.cpp:80-86
        has = m12 >= 0
        back = np.full(len(m12), -2, np.int64)
        back[has] = rev["matches"][m12[has]]
        m12[has & (back != np.arange(len(m12)))] = -1
    return dict(matches_12=m12.astype(np.int32), n_matches=int((m12 >= 0).sum()), fwd=fwd, rev=rev)


def match(desc1, desc2, nnr, best_lr: bool = True):
    """(matches_12 int32 [n1], n_matches) of StVO::match."""
    d = match_detail(desc1, desc2, nnr, best_lr)
    return d["matches_12"], d["n_matches"]
