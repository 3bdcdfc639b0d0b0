"""The checker of plba_grid_match (tests/ref_gridmatch.py, a literal restatement of StVO::matchGrid,
src2/matching.cpp:111-258) on hand-worked cases; the parallel formulation the kernels rely on and the
host mirror's CPU matcher and rasteriser against it; the ABI layout; and the conditions on the generated
parity cases that make a GPU pass mean something. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gridmatch_cases as cases
import ref_gridmatch as R
from plba import capi, slam_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = cases.parity_cases() + cases.boundary_cases()


def _desc(*dists):
    """Rows at the given Hamming distances from the zero row (32 bytes)."""
    out = np.zeros((len(dists), 32), np.uint8)
    for r, d in enumerate(dists):
        bits = np.zeros(256, np.uint8)
        bits[:d] = 1
        out[r] = np.packbits(bits)
    return out


def _points(qcells, tcells, qd, td, ws=1, nnr=0.9):
    return dict(kind=0, ws=ws, nnr=nnr, line_sim_th=0.75, desc1=qd, cell1=np.array(qcells, np.int32).reshape(-1, 2),
                cell1_end=None, desc2=td, cells2=[np.array(c, np.int32).reshape(-1, 2) for c in tcells], dir2=None)


def _both(pb, best_lr=True, cols=64, rows=48):
    """Checker, parallel formulation and the host mirror's CPU matcher agree; returns the checker's."""
    m, n = R.match_grid(pb, cols, rows, best_lr)
    pm, pn = R.match_grid_parallel(pb, cols, rows, best_lr)
    assert pm.tolist() == m.tolist() and pn == n
    cm, cn = slam_map.grid_match_cpu([pb], cols, rows, best_lr, desc_bytes=32)[0]
    assert cm.tolist() == m.tolist() and cn == n
    return m.tolist(), n


def test_a_tie_goes_to_the_lowest_train_index():
    q = _desc(0)
    pb = _points([(5, 5)], [[(5, 5)], [(5, 5)], [(5, 5)], [(6, 5)]], q, _desc(4, 2, 2, 3), nnr=1.5)
    assert _both(pb, False) == ([1], 1)            # 2 < 2 * 1.5
    pb["nnr"] = 1.0
    assert _both(pb, False) == ([-1], 0)           # a tie never passes nnr <= 1
    pb["nnr"], pb["desc2"] = 1.5, _desc(2, 2, 4, 3)
    assert _both(pb, False) == ([0], 1)


def test_a_single_candidate_passes_against_int_max():
    pb = _points([(5, 5)], [[(5, 5)], [(40, 40)]], _desc(0), _desc(200, 0))
    assert _both(pb, True) == ([0], 1)             # 200 < INT_MAX * 0.9
    assert _both(pb, False) == ([0], 1)


def test_no_seen_pair_is_no_match_above_nnr_one():
    # both queries see train 0; the second is not below the first's distance, so it has candidates
    # and no seen pair: best_d = INT_MAX. The reference counts index -1 there when nnr > 1.
    pb = _points([(5, 5), (5, 5)], [[(5, 5)]], _desc(3, 3), _desc(0), nnr=1.5)
    assert _both(pb, True) == ([0, -1], 1)
    assert _both(pb, False) == ([0, 0], 2)


def test_the_running_minimum_is_order_dependent():
    # train 0 is seen by query 0 (d = 9) and taken back by query 1 (d = 2): query 0 loses it in the
    # final cross-check although its own ratio test passed; the records are prefix minima
    pb = _points([(5, 5), (5, 5), (5, 5)], [[(5, 5)]], _desc(9, 2, 5), _desc(0))
    assert _both(pb, True) == ([-1, 0, -1], 1)
    pb["desc1"] = _desc(2, 9, 1)
    assert _both(pb, True) == ([-1, -1, 0], 1)
    assert R.match_grid_parallel(pb, 64, 48, True, records="column")[0].tolist() == [-1, -1, 0]


def _line(qs, qe, tcells, tdir, th=0.75, ws=1, qd=None, td=None):
    return dict(kind=1, ws=ws, nnr=0.9, line_sim_th=th, desc1=_desc(0) if qd is None else qd,
                cell1=np.array([qs], np.int32), cell1_end=np.array([qe], np.int32),
                desc2=_desc(1) if td is None else td, cells2=[np.array(tcells, np.int32).reshape(-1, 2)],
                dir2=np.array([tdir], np.float64))


def test_a_line_in_both_windows_counts_once():
    # the train line has cells in the start and in the end window: one candidate, second = INT_MAX
    pb = _line((10, 10), (14, 10), [(10, 10), (11, 10), (12, 10), (13, 10), (14, 10)], (1.0, 0.0))
    assert _both(pb) == ([0], 1)
    two = dict(pb, desc2=_desc(1, 1), cells2=pb["cells2"] * 2, dir2=np.array([(1.0, 0.0)] * 2))
    assert _both(two) == ([-1], 0)                 # counted twice it would look like this tie


def test_window_clipping_and_cells_outside_the_grid():
    q, t = _desc(0), _desc(1)
    for qc, tc, hit in (((0, 0), (1, 1), True), ((63, 47), (62, 46), True), ((0, 47), (1, 46), True),
                        ((63, 0), (62, 1), True), ((-1, 5), (0, 5), True), ((-2, 5), (0, 5), False),
                        ((64, 5), (63, 5), True), ((65, 5), (63, 5), False), ((5, 48), (5, 47), True),
                        ((5, -2), (5, 0), False), ((2 ** 31 - 1, 5), (63, 5), False), ((-2 ** 31, 5), (0, 5), False),
                        ((0, 0), (-1, 0), False), ((63, 47), (64, 47), False), ((5, 47), (5, 48), False)):
        assert _both(_points([qc], [[tc]], q, t)) == (([0], 1) if hit else ([-1], 0)), (qc, tc)
    # a row with an in-grid and an out-of-grid cell is found through the in-grid one only
    assert _both(_points([(0, 0)], [[(-1, 0), (1, 0)]], q, t)) == ([0], 1)
    assert _both(_points([(0, 0)], [[(-1, 0), (2, 0)]], q, t)) == ([-1], 0)
    assert _both(_points([(0, 0)], [[]], q, t)) == ([-1], 0)
    # a smaller grid clips earlier
    assert _both(_points([(9, 3)], [[(8, 3)]], q, t), cols=8, rows=6) == ([-1], 0)
    assert _both(_points([(8, 3)], [[(7, 3)]], q, t), cols=8, rows=6) == ([0], 1)


def test_a_zero_window_is_the_query_cell_alone():
    q, t = _desc(0), _desc(1)
    assert _both(_points([(7, 9)], [[(7, 9)]], q, t, ws=0)) == ([0], 1)
    for tc in ((8, 9), (7, 8), (6, 9), (7, 10)):
        assert _both(_points([(7, 9)], [[tc]], q, t, ws=0)) == ([-1], 0)


def test_the_direction_threshold_at_equality():
    # v1 = (3, 4) / 5 = (0.6, 0.8) exactly as doubles; with dir2 = (1, 0) the product is 0.6
    c = 0.6
    assert R.normalize(3, 4)[0] == c
    cells = [(10, 10)]
    assert _both(_line((10, 10), (13, 14), cells, (1.0, 0.0), th=c)) == ([0], 1)       # |dot| == th is kept
    assert _both(_line((10, 10), (13, 14), cells, (1.0, 0.0), th=np.nextafter(c, 1.0))) == ([-1], 0)
    assert _both(_line((13, 14), (10, 10), cells, (1.0, 0.0), th=c)) == ([0], 1)       # |.|: the sense is free
    assert _both(_line((10, 10), (13, 14), cells, (0.0, 1.0), th=0.81)) == ([-1], 0)
    # a query with equal cells: normalize() gives NaN, `abs(dot) < th` is false, the candidate is kept
    assert np.isnan(R.normalize(0, 0)[0])
    assert _both(_line((10, 10), (10, 10), cells, (1.0, 0.0), th=0.99)) == ([0], 1)


@pytest.mark.parametrize("best_lr", [False, True])
@pytest.mark.parametrize("case", ALL_CASES)
def test_parallel_formulation_and_cpu_matcher_equal_the_checker(case, best_lr):
    pb = cases.problem(*case)
    m, n = cases.reference(*case, best_lr)
    pm, pn = R.match_grid_parallel(pb, cases.COLS, cases.ROWS, best_lr)
    assert pm.tobytes() == m.tobytes() and pn == n
    cm, cn = slam_map.grid_match_cpu([pb], cases.COLS, cases.ROWS, best_lr, desc_bytes=case[3])[0]
    assert cm.tobytes() == m.tobytes() and cn == n


def test_record_chain_has_257_records_and_one_match():
    pb = cases.record_chain()
    cand, D = R.candidates_and_distances(pb)
    assert cand.all() and D[:257, 0].tolist() == list(range(256, -1, -1))
    m, n = _both(pb, True)
    assert n == 1 and m[256] == 0 and m.count(-1) == len(m) - 1


def test_library_exports_and_struct_layout():
    from plba import lib
    L = C.CDLL(lib.LIB_PATH)
    assert hasattr(L, "plba_grid_match") and "plba_grid_match" in lib.EXPORTED
    # the field list of include/plba.h, in order
    text = open(os.path.join(ROOT, "include", "plba.h")).read()
    body = re.search(r"typedef struct plba_gridmatch_batch \{(.*?)\} plba_gridmatch_batch;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        for name in decl.split(","):
            fields.append((re.sub(r"[^A-Za-z0-9_]", " ", name).split()[-1], pointer))
    assert [f for f, _ in fields] == [f for f, _ in capi.PlbaGridMatchBatch._fields_]
    off = 0
    for (name, pointer), (_, typ) in zip(fields, capi.PlbaGridMatchBatch._fields_):
        size = 8 if pointer else 4
        off = (off + size - 1) // size * size
        assert getattr(capi.PlbaGridMatchBatch, name).offset == off and C.sizeof(typ) == size, name
        off += size
    assert C.sizeof(capi.PlbaGridMatchBatch) == (off + 7) // 8 * 8 == 128
    assert C.sizeof(capi.PlbaMatchBatch) == 56     # untouched
    bv = capi.GridMatchBatchView([cases.problem(0, 1, 130, 32, 3, 0.9, 2), cases.problem(1, 1, 70, 32, 3, 0.9, 2)])
    assert bv.off1.tolist() == [0, 1, 2] and bv.off2.tolist() == [0, 130, 200] and bv.kind.tolist() == [0, 1]
    assert bv.cell_off2[130] == 130 and bv.cell_off2[-1] == len(bv.cells2) and bv.nnr.dtype == np.float64


def test_rasteriser_equals_its_model():
    rng = np.random.default_rng(11)
    segs = [(0.5, 0.5, 0.5, 0.5), (3.2, 4.9, 3.9, 4.1), (0, 0, 10, 10), (10, 10, 0, 0), (2.5, 7.5, 40.25, 9.75),
            (5.5, 40.0, 5.5, 2.0), (-3.7, 5.2, 4.1, -2.9), (63.9, 47.9, 60.1, 0.2), (1.0, 2.0, 1.0, 9.0),
            (7.999, 3.0, 8.001, 30.0), (-0.9, -0.9, 0.9, 0.9)]
    segs += [tuple(rng.uniform(-5, 70, 4)) for _ in range(200)]
    segs += [tuple(np.round(rng.uniform(0, 64, 4))) for _ in range(50)]   # on cell borders
    for s in segs:
        model = R.line_cells(*s)
        assert slam_map.line_cells(*s).tolist() == [list(c) for c in model], s
    assert len(R.line_cells(3.2, 4.9, 3.9, 4.1)) == 1 and len(R.line_cells(0.5, 20.0, 45.3, 21.0)) == 46
    # the line problems' train rows: one cell, and 40 or more
    pb = cases.problem(1, 300, 200, 32, 3, 0.9, 0)
    assert len(pb["cells2"][0]) == 1 and len(pb["cells2"][1]) >= 40


def test_generated_cases_are_not_vacuous():
    """On the checker alone: a device that answers -1, skips the final cross-check or the running
    minimum, takes column minima for records or breaks ties the other way cannot pass these cases."""
    lost_to_cross = lr_differs = column_differs = tie_by_index = 0
    for case in cases.parity_cases():
        pb = cases.problem(*case)
        m, n = cases.reference(*case, True)
        m0, n0 = cases.reference(*case, False)
        disp = pb["src"] >= 0
        assert (m[disp] == pb["src"][disp]).sum() >= 0.5 * disp.sum(), case
        lr_differs += int((m != m0).any())
        column_differs += int((R.match_grid_parallel(pb, cases.COLS, cases.ROWS, True, "column")[0] != m).any())
        # rows whose ratio test passed and whose match the final cross-check removed; ties at the best
        cand, D = R.candidates_and_distances(pb, cases.COLS, cases.ROWS)
        big = np.where(cand, D, R.INT_MAX)
        before = np.vstack([np.full((1, big.shape[1]), R.INT_MAX), np.minimum.accumulate(big, axis=0)[:-1]])
        seen = cand & (D < before)
        for i1 in range(len(m)):
            ds = np.sort(D[i1][seen[i1]])
            if len(ds) and m[i1] < 0 and (len(ds) == 1 or float(ds[0]) < float(ds[1]) * pb["nnr"]):
                lost_to_cross += 1
            if len(ds) >= 2 and ds[0] == ds[1] and m[i1] >= 0:
                assert m[i1] == np.flatnonzero(seen[i1] & (D[i1] == ds[0]))[0]
                tie_by_index += 1
    for case in cases.boundary_cases():
        assert cases.reference(*case, True)[1] >= 1, case
    assert lost_to_cross >= 1 and lr_differs >= 1 and column_differs >= 1 and tie_by_index >= 1, \
        (lost_to_cross, lr_differs, column_differs, tie_by_index)
