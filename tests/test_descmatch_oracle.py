"""The numpy checker of plba_desc_match (tests/ref_descmatch.py) against a literal restatement of
StVO::matchNNR + StVO::match (src2/matching.cpp:41-91), the pinned semantics one by one, the ABI
layout, and the conditions on the generated parity cases that make a GPU pass mean something. No GPU."""
import ctypes as C

import numpy as np
import pytest

import descmatch_cases as cases
import ref_descmatch as R
from plba import capi


def _literal_nnr(desc1, desc2, nnr):
    """matchNNR, row by row: knnMatch(k = 2) as a scan in increasing train index with strict
    comparisons, then `distance[0] < distance[1] * nnr` on floats. No match below 2 train rows."""
    matches_12 = [-1] * len(desc1)
    if len(desc2) < 2:
        return matches_12
    for idx in range(len(desc1)):
        best, second, best_i = None, None, -1
        for j in range(len(desc2)):
            d = 0
            for c in range(desc1.shape[1]):
                d += bin(int(desc1[idx, c]) ^ int(desc2[j, c])).count("1")
            if best is None or d < best:
                best, second, best_i = d, best, j
            elif second is None or d < second:
                second = d
        if np.float32(best) < np.float32(second) * np.float32(nnr):
            matches_12[idx] = best_i
    return matches_12


def _literal_match(desc1, desc2, nnr, best_lr):
    matches_12 = _literal_nnr(desc1, desc2, nnr)
    matches = sum(i2 >= 0 for i2 in matches_12)
    if best_lr:
        matches_21 = _literal_nnr(desc2, desc1, nnr)
        for i1 in range(len(matches_12)):
            i2 = matches_12[i1]
            if i2 >= 0 and matches_21[i2] != i1:
                matches_12[i1] = -1
                matches -= 1
    return matches_12, matches


def _small(n1, n2, desc_bytes, seed):
    """Small sets with planted matches, exact duplicates and near-duplicates on both sides."""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n1, desc_bytes), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, desc_bytes), dtype=np.uint8)
    for k in range(min(n1, n2) // 2):
        d1[k] = cases._flip(rng, d2[(3 * k) % n2], int(rng.integers(0, 3)))
    if n2 >= 4:
        d2[n2 - 1] = d2[0]
    if n1 >= 4:
        d1[n1 - 1] = cases._flip(rng, d1[1], 1)
    return d1, d2


@pytest.mark.parametrize("best_lr", [False, True])
@pytest.mark.parametrize("nnr", [0.9, 0.6, 1.0, 1.5])
@pytest.mark.parametrize("n1,n2,desc_bytes", [(9, 7, 4), (12, 20, 8), (20, 12, 32), (1, 2, 32), (2, 1, 32), (3, 0, 32),
                                              (0, 3, 32), (2, 2, 64)])
def test_checker_equals_the_literal_restatement(n1, n2, desc_bytes, nnr, best_lr):
    d1, d2 = _small(n1, n2, desc_bytes, 5 + n1 + 31 * n2)
    m12, n = R.match(d1, d2, nnr, best_lr)
    lit, nl = _literal_match(d1, d2, nnr, best_lr)
    assert m12.tolist() == lit and n == nl


def test_ties_go_to_the_lowest_train_index():
    q = np.zeros((1, 32), np.uint8)
    t = np.zeros((5, 32), np.uint8)
    t[0, 0], t[1, 0], t[2, 0], t[3, 0], t[4, 0] = 0x0F, 0x03, 0x30, 0x07, 0x03   # distances 4, 2, 2, 3, 2
    r = R.nearest(q, t, 2.0)
    assert (r["d0"][0], r["d1"][0], r["i0"][0], bool(r["tie"][0])) == (2, 2, 1, True)
    assert r["matches"][0] == 1                      # 2 < 2 * 2: visible only above nnr = 1
    assert R.nearest(q, t, 1.0)["matches"][0] == -1  # a tie in d0 never passes nnr <= 1
    assert _literal_nnr(q, t, 2.0) == [1]
    # the second-best is a value, not a row: a later equal distance does not displace the best
    assert R.nearest(q, t[::-1].copy(), 2.0)["i0"][0] == 0


def test_fewer_than_two_train_rows_give_no_match():
    d1, d2 = _small(6, 1, 32, 3)
    d1[2] = d2[0]   # even an exact copy
    for best_lr in (False, True):
        m12, n = R.match(d1, d2, 0.9, best_lr)
        assert n == 0 and (m12 == -1).all() and len(m12) == 6
    # the forward pass has its two rows, the reverse pass has one: without the cross-check the
    # forward matches stand, with it none survives
    m12, n = R.match(d2, d1, 0.9, False)
    assert n == 1 and m12.tolist() == [2]
    m12, n = R.match(d2, d1, 0.9, True)
    assert n == 0
    for a, b in (((0, 32), (4, 32)), ((4, 32), (0, 32)), ((0, 32), (0, 32))):
        m12, n = R.match(np.zeros(a, np.uint8), np.zeros(b, np.uint8), 0.9, True)
        assert n == 0 and len(m12) == a[0]


def test_ratio_test_is_single_precision():
    # nnr = 0.6f, d0 = 6, d1 = 10: 10 * 0.6f = 6.0000002384 in double, so double says 6 < 6.0000002;
    # the float product rounds to 6.0f and float says 6 < 6 is false (matching.cpp:54 is float)
    nnr = np.float32(0.6)
    assert 6.0 < 10.0 * float(nnr) and not (np.float32(6) < np.float32(10) * nnr)
    q = np.zeros((1, 32), np.uint8)
    t = np.zeros((2, 32), np.uint8)
    t[0, 0], t[1, :2] = 0x3F, (0xFF, 0x03)   # distances 6 and 10
    r = R.nearest(q, t, nnr)
    assert (r["d0"][0], r["d1"][0]) == (6, 10) and r["matches"][0] == -1
    t[0, 0] = 0x1F                           # 5 < 6: matched
    assert R.nearest(q, t, nnr)["matches"][0] == 0


def test_library_exports_and_struct_layout():
    from plba import lib
    L = C.CDLL(lib.LIB_PATH)
    assert hasattr(L, "plba_desc_match") and "plba_desc_match" in lib.EXPORTED
    # include/plba.h: 2 int32, 5 pointers, 2 int32
    assert C.sizeof(capi.PlbaMatchBatch) == 8 + 5 * 8 + 8
    assert capi.PlbaMatchBatch.off1.offset == 8 and capi.PlbaMatchBatch.nnr.offset == 40
    assert capi.PlbaMatchBatch.best_lr.offset == 48
    from plba import slam_map
    assert C.sizeof(slam_map.PlslamMatchParams) == 24
    bv = capi.MatchBatchView([cases.pair(5, 0), cases.pair(1, 2)], [0.9, 0.6])
    assert bv.off1.tolist() == [0, 5, 6] and bv.off2.tolist() == [0, 0, 2] and bv.struct.desc_bytes == 32
    assert bv.nnr.dtype == np.float32 and bv.struct.best_lr == 1


@pytest.mark.parametrize("n1,n2,desc_bytes,nnr", [c for c in cases.parity_cases()
                                                 if min(c[0], c[1]) >= cases.PLANTED_MIN_ROWS])
def test_parity_cases_exercise_every_branch(n1, n2, desc_bytes, nnr):
    """On the checker alone: a device that answers -1 everywhere, skips the ratio test, skips the
    cross-check or breaks ties the other way cannot pass these cases. (The shapes below 64 rows are
    the empty, one-row and two-row pairs; what they must give is pinned in the tests above.)"""
    ref = cases.reference(n1, n2, desc_bytes, nnr, True)
    fwd = ref["fwd"]
    assert ref["n_matches"] >= 0.25 * n1, (ref["n_matches"], n1)
    ratio_rejected = (fwd["matches"] < 0) & (fwd["i0"] >= 0)
    assert ratio_rejected.any()
    cross_only = (fwd["matches"] >= 0) & (ref["matches_12"] < 0)
    assert cross_only.any()
    tied = np.flatnonzero(fwd["tie"])
    assert len(tied) >= 1
    D = R.hamming(*cases.pair(n1, n2, desc_bytes))
    for i in tied:   # resolved by index: the best row is the first of the rows at d0
        assert fwd["i0"][i] == np.flatnonzero(D[i] == fwd["d0"][i])[0]
        assert (D[i] == fwd["d0"][i]).sum() >= 2
    # without the cross-check the cross-only rows are matches
    assert cases.reference(n1, n2, desc_bytes, nnr, False)["n_matches"] == ref["n_matches"] + int(cross_only.sum())
