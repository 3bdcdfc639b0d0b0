"""Descriptor matching on the GPU (plba_desc_match: StVO::match / matchNNR, src2/matching.cpp:41-91)
against the numpy checker (tests/ref_descmatch.py). Integer distances, a float product and a float
compare: the parity is bitwise, with no tolerance. tests/test_descmatch_oracle.py shows on the
checker alone that these cases hold matches, ratio rejects, cross-check rejects and ties."""
import ctypes as C

import numpy as np
import pytest

import descmatch_cases as cases
import ref_descmatch as R
from plba import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _assert_equal(out, ref_m12, ref_n):
    m12, n = out
    assert m12.dtype == np.int32 and m12.tobytes() == np.asarray(ref_m12, np.int32).tobytes(), \
        np.flatnonzero(m12 != ref_m12)[:10]
    assert n == ref_n


@pytest.mark.parametrize("best_lr", [False, True])
@pytest.mark.parametrize("n1,n2,desc_bytes,nnr", cases.parity_cases())
def test_parity_with_the_checker(solver, n1, n2, desc_bytes, nnr, best_lr):
    ref = cases.reference(n1, n2, desc_bytes, nnr, best_lr)
    out = solver.desc_match([cases.pair(n1, n2, desc_bytes)], nnr, best_lr, desc_bytes=desc_bytes)[0]
    print("matches", out[1], "of", n1)
    _assert_equal(out, ref["matches_12"], ref["n_matches"])


@pytest.mark.parametrize("n1,n2,desc_bytes", [(257, 255, 32), (300, 1000, 32), (257, 255, 8), (257, 255, 64)])
def test_ties_go_to_the_lowest_train_index(solver, n1, n2, desc_bytes):
    # above nnr = 1 a row whose two nearest train rows tie is matched, to the first of them
    ref = cases.reference(n1, n2, desc_bytes, 1.5, False)
    tied = ref["fwd"]["tie"] & (ref["matches_12"] >= 0)
    assert tied.any()
    out = solver.desc_match([cases.pair(n1, n2, desc_bytes)], 1.5, False)[0]
    _assert_equal(out, ref["matches_12"], ref["n_matches"])
    # and with the train rows reversed the same rows go to the other member of the tie
    d1, d2 = cases.pair(n1, n2, desc_bytes)
    d2r = np.ascontiguousarray(d2[::-1])
    rm, rn = R.match(d1, d2r, np.float32(1.5), False)
    assert (rm[tied] != n2 - 1 - ref["matches_12"][tied]).any()
    _assert_equal(solver.desc_match([(d1, d2r)], 1.5, False)[0], rm, rn)


def test_float_ratio_at_six_of_ten(solver):
    # nnr = 0.6f, d0 = 6, d1 = 10: no match in float (6 < 6.0f is false), a match in double
    q = np.zeros((1, 32), np.uint8)
    t = np.zeros((2, 32), np.uint8)
    t[0, 0], t[1, :2] = 0x3F, (0xFF, 0x03)
    assert solver.desc_match([(q, t)], 0.6, False)[0][1] == 0
    t[0, 0] = 0x1F
    out = solver.desc_match([(q, t)], 0.6, False)[0]
    assert out[1] == 1 and out[0].tolist() == [0]


@pytest.mark.parametrize("best_at,second_at,n2", [(255, 511, 600), (511, 255, 600), (599, 256, 600), (0, 767, 768),
                                                  (767, 0, 768)])
def test_best_and_second_best_in_different_train_tiles(solver, best_at, second_at, n2):
    """The two nearest rows sit in different tiles of 256 train rows, on a tile's last or first row
    and on the last row of a partial tile: d0, i0 and d1 are carried across the tiles."""
    rng = np.random.default_rng(best_at + 7 * second_at)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    d1 = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    d1[1] = cases._flip(rng, d2[best_at], 2)
    d2[second_at] = cases._flip(rng, d2[best_at], 20)
    ref = R.nearest(d1, d2, np.float32(0.9))
    assert ref["i0"][1] == best_at and ref["d0"][1] == 2 and 18 <= ref["d1"][1] <= 22
    for nnr in (0.9, 0.1, 0.12):   # matched; d0 = 2 against 0.1 * d1 <= 2.2 and 0.12 * d1 up to 2.64: the second-best decides
        rm, rn = R.match(d1, d2, np.float32(nnr), False)
        _assert_equal(solver.desc_match([(d1, d2)], nnr, False)[0], rm, rn)
    assert R.match(d1, d2, np.float32(0.9), False)[0][1] == best_at
    assert R.match(d1, d2, np.float32(0.05), False)[0][1] == -1


def test_a_mixed_batch_equals_its_single_calls_bitwise(solver):
    shapes = [(300, 1000), (5, 0), (1, 2), (257, 255), (0, 5), (2, 1), (0, 0), (256, 256), (1, 1)]
    pairs = [cases.pair(a, b, 32, seed=1) for a, b in shapes]
    nnr = [0.9, 0.9, 0.6, 1.0, 0.9, 0.6, 0.9, 0.6, 0.9]
    for best_lr in (True, False):
        batch = solver.desc_match(pairs, nnr, best_lr)
        again = solver.desc_match(pairs, nnr, best_lr)
        for p, r, o, o2 in zip(pairs, nnr, batch, again):
            single = solver.desc_match([p], r, best_lr)[0]
            rm, rn = R.match(p[0], p[1], np.float32(r), best_lr)
            _assert_equal(o, rm, rn)
            _assert_equal(single, rm, rn)
            _assert_equal(o2, rm, rn)
    assert batch[1][1] == 0 and batch[2][1] == 0 and batch[8][1] == 0 and len(batch[4][0]) == 0


def test_matching_leaves_an_uploaded_window_intact(solver):
    from plba import synth
    g = synth.generate("C1L")
    solver.upload(g)
    before = solver.lba_plucker()
    out = solver.desc_match([cases.pair(257, 255, 32)], 0.9)[0]
    assert out[1] == cases.reference(257, 255, 32, 0.9, True)["n_matches"]
    solver.reset()
    after = solver.lba_plucker()
    for k in ("kf_Tcw", "pt_xyz", "ln_orth"):
        assert np.array_equal(before[k], after[k]), k


def test_bad_arguments_are_refused(solver):
    from plba.lib import PLBA_ERRORS
    ip = C.POINTER(C.c_int32)
    bv = capi.MatchBatchView([cases.pair(5, 0), cases.pair(257, 255)], 0.9)
    m12, cnt = np.zeros(262, np.int32), np.zeros(2, np.int32)

    def call(m=m12, c=cnt):
        rc = solver.L.plba_desc_match(solver.ctx, C.byref(bv.struct), m.ctypes.data_as(ip) if m is not None else None,
                                      c.ctypes.data_as(ip) if c is not None else None)
        return PLBA_ERRORS.get(rc, rc)
    assert call() == 0
    for db in (0, 2, 30, 68, -4):
        bv.struct.desc_bytes = db
        assert call() == "PLBA_E_INVALID", db
    bv.struct.desc_bytes = 32
    bv.struct.n = -1
    assert call() == "PLBA_E_INVALID"
    bv.struct.n = 2
    bv.off1[:] = [0, 262, 5]      # decreasing
    assert call() == "PLBA_E_INVALID"
    bv.off1[:] = [-1, 5, 262]     # negative
    assert call() == "PLBA_E_INVALID"
    bv.off1[:] = [0, 5, 262]
    assert call(m=None) == "PLBA_E_INVALID" and call(c=None) == "PLBA_E_INVALID"
    for name, typ in capi.PlbaMatchBatch._fields_:
        if name in ("off1", "off2", "desc1", "desc2", "nnr"):
            addr = C.cast(getattr(bv.struct, name), C.c_void_p).value   # the field object aliases the struct
            setattr(bv.struct, name, None)
            assert call() == "PLBA_E_INVALID", name
            setattr(bv.struct, name, C.cast(addr, typ))
    assert solver.L.plba_desc_match(solver.ctx, None, m12.ctypes.data_as(ip), cnt.ctypes.data_as(ip)) != 0
    bv.struct.n = 0               # nothing to do
    assert call() == 0
    bv.struct.n = 2               # and the same view, intact, is accepted and right
    m12[:] = -7
    assert call() == 0
    ref = cases.reference(257, 255, 32, 0.9, True)
    assert m12[5:].tolist() == ref["matches_12"].tolist() and cnt.tolist() == [0, ref["n_matches"]] and (m12[:5] == -1).all()
