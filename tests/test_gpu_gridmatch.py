"""Grid-guided descriptor matching on the GPU (plba_grid_match: both StVO::matchGrid overloads,
src2/matching.cpp:111-258) against the checker (tests/ref_gridmatch.py). Integer work and two double
comparisons: the parity is bitwise, with no tolerance. tests/test_gridmatch_oracle.py shows on the
checker alone that the generated cases hold matches, cross-check losses, order dependence and ties."""
import ctypes as C

import numpy as np
import pytest

import gridmatch_cases as cases
import ref_gridmatch as R
from plba import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _assert_equal(out, ref):
    m12, n = out
    ref_m12, ref_n = ref
    assert m12.dtype == np.int32 and m12.tobytes() == np.asarray(ref_m12, np.int32).tobytes(), \
        np.flatnonzero(m12 != ref_m12)[:10]
    assert n == ref_n


@pytest.mark.parametrize("best_lr", [False, True])
@pytest.mark.parametrize("case", cases.parity_cases() + cases.boundary_cases())
def test_parity_with_the_checker(solver, case, best_lr):
    out = solver.grid_match([cases.problem(*case)], cases.COLS, cases.ROWS, best_lr, desc_bytes=case[3])[0]
    print("matches", out[1], "of", case[1])
    _assert_equal(out, cases.reference(*case, best_lr))


def test_an_empty_side_gives_no_match(solver):
    full = cases.problem(1, 90, 63, 32, 3, 1.5, 3)
    no_train = dict(full, desc2=np.zeros((0, 32), np.uint8), cells2=[], dir2=np.zeros((0, 2)))
    no_query = dict(full, desc1=np.zeros((0, 32), np.uint8), cell1=np.zeros((0, 2), np.int32),
                    cell1_end=np.zeros((0, 2), np.int32))
    out = solver.grid_match([no_train, no_query, full], cases.COLS, cases.ROWS, True)
    assert out[0][1] == 0 and (out[0][0] == -1).all() and len(out[0][0]) == 90
    assert out[1][1] == 0 and len(out[1][0]) == 0
    _assert_equal(out[2], cases.reference(1, 90, 63, 32, 3, 1.5, 3, True))
    assert solver.grid_match([no_train], cases.COLS, cases.ROWS, True)[0][1] == 0


def test_a_long_record_chain_in_one_column(solver):
    pb = cases.record_chain()
    for best_lr in (True, False):
        _assert_equal(solver.grid_match([pb], cases.COLS, cases.ROWS, best_lr)[0],
                      R.match_grid(pb, cases.COLS, cases.ROWS, best_lr))
    assert solver.grid_match([pb], cases.COLS, cases.ROWS, True)[0][0][256] == 0


def test_cell_lists_too_long_for_lds_are_read_from_global_memory(solver):
    """A block of 64 train rows keeps up to 4096 in-grid cells in LDS; past that it reads the lists from
    global memory. Listing every cell eight times changes no candidate, only the path."""
    case = (1, 90, 65, 32, 3, 1.5, 3)
    pb = cases.problem(*case)
    assert sum(len(c) for c in pb["cells2"][:64]) <= 4096
    long = dict(pb, cells2=[np.tile(c, (8, 1)) if len(c) >= 2 else c for c in pb["cells2"]])
    assert sum(len(c) for c in long["cells2"][:64]) > 4096
    for best_lr in (False, True):
        _assert_equal(solver.grid_match([long], cases.COLS, cases.ROWS, best_lr)[0], cases.reference(*case, best_lr))


def test_hand_cases_on_the_device(solver):
    q = np.zeros((2, 32), np.uint8)
    t = np.zeros((1, 32), np.uint8)
    t[0, 0] = 0x07
    pb = dict(kind=0, ws=1, nnr=1.5, line_sim_th=0.75, desc1=q, cell1=np.array([[5, 5], [5, 5]], np.int32),
              cell1_end=None, desc2=t, cells2=[np.array([[5, 5]], np.int32)], dir2=None)
    out = solver.grid_match([pb], 64, 48, True)[0]     # the second row has candidates and no seen pair
    assert out[0].tolist() == [0, -1] and out[1] == 1
    # cells outside the grid on both sides, a degenerate query line (NaN direction) and |dot| == th
    ln = dict(kind=1, ws=1, nnr=0.9, line_sim_th=0.6, desc1=np.zeros((4, 32), np.uint8),
              cell1=np.array([[10, 10], [10, 10], [-2 ** 31, 5], [64, 47]], np.int32),
              cell1_end=np.array([[13, 14], [10, 10], [2 ** 31 - 1, 5], [70, 47]], np.int32),
              desc2=t, cells2=[np.array([[-1, 10], [10, 10], [64, 47], [63, 47]], np.int32)],
              dir2=np.array([[1.0, 0.0]]))
    for best_lr in (False, True):
        _assert_equal(solver.grid_match([ln], 64, 48, best_lr)[0], R.match_grid(ln, 64, 48, best_lr))
    assert solver.grid_match([ln], 64, 48, False)[0][0].tolist() == [0, 0, -1, 0]
    ln["line_sim_th"] = float(np.nextafter(0.6, 1.0))
    assert solver.grid_match([ln], 64, 48, False)[0][0].tolist() == [-1, 0, -1, 0]


def test_a_batch_equals_its_single_calls_bitwise(solver):
    pool = [cases.problem(*c) for c in (cases.parity_cases()[4], cases.parity_cases()[12], cases.boundary_cases()[3],
                                        cases.boundary_cases()[7], cases.boundary_cases()[12],
                                        cases.boundary_cases()[17], cases.parity_cases()[0], cases.parity_cases()[9])]
    assert {p["kind"] for p in pool} == {0, 1} and len({(p["ws"], p["nnr"]) for p in pool}) >= 3
    single = {True: [solver.grid_match([p], cases.COLS, cases.ROWS, True)[0] for p in pool],
              False: [solver.grid_match([p], cases.COLS, cases.ROWS, False)[0] for p in pool]}
    for best_lr in (True, False):
        for k in (1, 2, 8):
            batch = solver.grid_match(pool[:k], cases.COLS, cases.ROWS, best_lr)
            again = solver.grid_match(pool[:k], cases.COLS, cases.ROWS, best_lr)
            for p, o, o2, s in zip(pool, batch, again, single[best_lr]):
                _assert_equal(o, s)
                _assert_equal(o2, s)
                _assert_equal(o, R.match_grid(p, cases.COLS, cases.ROWS, best_lr))


def test_matching_leaves_an_uploaded_window_intact(solver):
    from plba import synth
    g = synth.generate("C1L")
    solver.upload(g)
    before = solver.lba_plucker()
    solver.upload(g)
    case = cases.parity_cases()[4]
    _assert_equal(solver.grid_match([cases.problem(*case)], cases.COLS, cases.ROWS, True)[0], cases.reference(*case, True))
    after = solver.lba_plucker()
    for k in ("kf_Tcw", "pt_xyz", "ln_orth"):
        assert np.array_equal(before[k], after[k]), k


def test_bad_arguments_are_refused(solver):
    from plba.lib import PLBA_ERRORS
    ip = C.POINTER(C.c_int32)
    c0, c1 = cases.boundary_cases()[3], cases.boundary_cases()[7]
    bv = capi.GridMatchBatchView([cases.problem(*c0), cases.problem(*c1)], cases.COLS, cases.ROWS, True)
    n1 = int(bv.off1[-1])
    m12, cnt = np.zeros(n1, np.int32), np.zeros(2, np.int32)

    def call(m=m12, c=cnt):
        rc = solver.L.plba_grid_match(solver.ctx, C.byref(bv.struct), m.ctypes.data_as(ip) if m is not None else None,
                                      c.ctypes.data_as(ip) if c is not None else None)
        return PLBA_ERRORS.get(rc, rc)
    assert call() == 0
    for name, bad in (("desc_bytes", (0, 2, 30, 68, -4)), ("cols", (0, -1)), ("rows", (0, -64)), ("n", (-1,))):
        keep = getattr(bv.struct, name)
        for v in bad:
            setattr(bv.struct, name, v)
            assert call() == "PLBA_E_INVALID", (name, v)
        setattr(bv.struct, name, keep)
    for arr, bad in ((bv.off1, [0, n1, 5]), (bv.off1, [-1, 5, n1]), (bv.off2, [0, 200, 100]), (bv.ws, [3, -1]),
                     (bv.kind, [0, 2]), (bv.kind, [-1, 1])):
        keep = arr.copy()
        arr[:] = bad
        assert call() == "PLBA_E_INVALID", bad
        arr[:] = keep
    keep = bv.cell_off2.copy()
    bv.cell_off2[5] = bv.cell_off2[4] - 1                 # decreasing cell offsets
    assert call() == "PLBA_E_INVALID"
    bv.cell_off2[:] = keep
    bv.cell_off2[0] = -1
    assert call() == "PLBA_E_INVALID"
    bv.cell_off2[:] = keep
    assert call(m=None) == "PLBA_E_INVALID" and call(c=None) == "PLBA_E_INVALID"
    for name, typ in capi.PlbaGridMatchBatch._fields_:
        if name in ("off1", "off2", "desc1", "desc2", "cell1", "cell1_end", "cell_off2", "cells2", "dir2", "kind", "ws",
                    "nnr", "line_sim_th"):
            addr = C.cast(getattr(bv.struct, name), C.c_void_p).value
            setattr(bv.struct, name, None)
            assert call() == "PLBA_E_INVALID", name
            setattr(bv.struct, name, C.cast(addr, typ))
    assert solver.L.plba_grid_match(solver.ctx, None, m12.ctypes.data_as(ip), cnt.ctypes.data_as(ip)) != 0
    # more train rows in a problem than a key's 16 bits index
    big = capi.GridMatchBatchView([dict(kind=0, ws=0, nnr=0.9, desc1=np.zeros((1, 32), np.uint8),
                                        cell1=np.zeros((1, 2), np.int32), desc2=np.zeros((65536, 32), np.uint8),
                                        cells2=[np.zeros((1, 2), np.int32)] * 65536)])
    assert PLBA_ERRORS.get(solver.L.plba_grid_match(solver.ctx, C.byref(big.struct), m12.ctypes.data_as(ip),
                                                    cnt.ctypes.data_as(ip))) == "PLBA_E_INVALID"
    bv.struct.n = 0               # nothing to do
    assert call() == 0
    bv.struct.n = 2               # and the same view, intact, is accepted and right
    m12[:] = -7
    assert call() == 0
    r0, r1 = cases.reference(*c0, True), cases.reference(*c1, True)
    assert m12.tolist() == r0[0].tolist() + r1[0].tolist() and cnt.tolist() == [r0[1], r1[1]]
