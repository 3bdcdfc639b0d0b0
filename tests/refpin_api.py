"""TEST INFRASTRUCTURE: ctypes binding of oracle/_ref/libref_stvo.so, the pieces of the reference that
compile with the standard library alone behind the shim of oracle/refpin/ (getLineCoords, GridStructure,
both matchGrid overloads, distance, normalize, BowVector). `make -C oracle` builds it where the reference
tree is present; tests/golden/refpin.npz holds its recorded outputs for everywhere else.

require() is the one rule for a test's live half: the library if it is there; a failure if the reference tree
is there and the library is not (the build is broken); a skip only when both are absent."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_stvo.so")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")   # oracle/Makefile's variable and default

IP, DP, BP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
_lib = None


def available() -> bool:
    return os.path.exists(REF_SO)


def tree_present() -> bool:
    return os.path.exists(os.path.join(REFERENCE, "src2", "matching.cpp"))


def require():
    import pytest
    if available():
        return lib()
    if tree_present():
        pytest.fail("the reference tree is present but oracle/_ref/libref_stvo.so is not: `make -C oracle` failed")
    pytest.skip("neither the reference tree nor oracle/_ref/libref_stvo.so is here: only the recorded half runs")


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(REF_SO)
        vp, i32, dbl = C.c_void_p, C.c_int32, C.c_double
        L.refpin_line_coords.argtypes = [dbl, dbl, dbl, dbl, IP, i32, IP]
        L.refpin_grid_new.argtypes, L.refpin_grid_new.restype = [i32, i32], vp
        L.refpin_grid_free.argtypes, L.refpin_grid_free.restype = [vp], None
        L.refpin_grid_fill.argtypes = [vp, i32, IP, IP]
        L.refpin_grid_get.argtypes = [vp, i32, i32, IP, IP, i32, IP]
        L.refpin_distance.argtypes = [BP, BP]
        L.refpin_normalize.argtypes = [DP]
        L.refpin_match_grid_points.argtypes = [vp, i32, IP, BP, i32, BP, IP, i32, dbl, IP, IP]
        L.refpin_match_grid_lines.argtypes = [vp, i32, IP, IP, BP, i32, BP, DP, IP, i32, dbl, dbl, IP, IP]
        L.refpin_bow_new.argtypes, L.refpin_bow_new.restype = [], vp
        L.refpin_bow_free.argtypes, L.refpin_bow_free.restype = [vp], None
        L.refpin_bow_add_weight.argtypes = [vp, C.c_uint32, dbl]
        L.refpin_bow_add_if_not_exist.argtypes = [vp, C.c_uint32, dbl]
        L.refpin_bow_normalize_l1.argtypes = [vp]
        L.refpin_bow_entries.argtypes = [vp, C.POINTER(C.c_uint32), DP, i32, IP]
        _lib = L
    return _lib


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {rc}")


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def line_coords(x1, y1, x2, y2) -> np.ndarray:
    """getLineCoords(x1, y1, x2, y2): [n][2] int32 (x, y) in the walk's order."""
    n = C.c_int32(0)
    _ok(lib().refpin_line_coords(x1, y1, x2, y2, None, 0, C.byref(n)), "refpin_line_coords")
    out = np.zeros((n.value, 2), np.int32)
    _ok(lib().refpin_line_coords(x1, y1, x2, y2, out.ctypes.data_as(IP), n.value, C.byref(n)), "refpin_line_coords")
    return out


class Grid:
    """A GridStructure(rows, cols) filled with grid.at(x, y).push_back(idx) over cells2, a list of [k][2]
    arrays, one per train row."""

    def __init__(self, cells2, cols=64, rows=48):
        self.h = lib().refpin_grid_new(rows, cols)
        if not self.h:
            raise RuntimeError("refpin_grid_new failed")
        off = np.zeros(len(cells2) + 1, np.int32)
        off[1:] = np.cumsum([len(np.asarray(c).reshape(-1, 2)) for c in cells2])
        flat = _i32(np.concatenate([np.asarray(c, np.int32).reshape(-1, 2) for c in cells2])) if len(cells2) else \
            np.zeros((0, 2), np.int32)
        _ok(lib().refpin_grid_fill(self.h, len(cells2), off.ctypes.data_as(IP), flat.ctypes.data_as(IP)), "refpin_grid_fill")

    def get(self, x, y, w) -> list:
        """GridStructure::get(x, y, w) with w = (left, right, up, down): the indices, sorted."""
        w = _i32(w)
        n = C.c_int32(0)
        _ok(lib().refpin_grid_get(self.h, x, y, w.ctypes.data_as(IP), None, 0, C.byref(n)), "refpin_grid_get")
        out = np.zeros(max(n.value, 1), np.int32)
        _ok(lib().refpin_grid_get(self.h, x, y, w.ctypes.data_as(IP), out.ctypes.data_as(IP), n.value, C.byref(n)),
            "refpin_grid_get")
        return out[:n.value].tolist()

    def close(self):
        if self.h:
            lib().refpin_grid_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def distance(a, b) -> int:
    a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
    assert a.size == 32 and b.size == 32, "StVO::distance reads exactly eight 32-bit words"
    return int(lib().refpin_distance(a.ctypes.data_as(BP), b.ctypes.data_as(BP)))


def normalize(vx, vy):
    v = np.array([vx, vy], np.float64)
    _ok(lib().refpin_normalize(v.ctypes.data_as(DP)), "refpin_normalize")
    return float(v[0]), float(v[1])


def match_grid(pb, cols=64, rows=48, best_lr=True, w=None):
    """(matches_12 int32 [n1], the returned count) of the reference's matchGrid on a problem of
    Solver.grid_match (tests/ref_gridmatch.py); w = (left, right, up, down), default ws on every side.
    Descriptors are 32 bytes: the reference's distance reads nothing else."""
    desc1, desc2 = np.ascontiguousarray(pb["desc1"], np.uint8), np.ascontiguousarray(pb["desc2"], np.uint8)
    n1, n2 = len(desc1), len(desc2)
    assert (n1 == 0 or desc1.shape[1] == 32) and (n2 == 0 or desc2.shape[1] == 32)
    w = _i32([pb["ws"]] * 4 if w is None else w)
    cell1 = _i32(np.asarray(pb["cell1"]).reshape(-1, 2))
    m12, cnt = np.full(max(n1, 1), -1, np.int32), C.c_int32(0)
    with Grid(pb["cells2"], cols, rows) as g:
        if pb["kind"] == 0:
            _ok(lib().refpin_match_grid_points(g.h, n1, cell1.ctypes.data_as(IP), desc1.ctypes.data_as(BP), n2,
                                               desc2.ctypes.data_as(BP), w.ctypes.data_as(IP), int(best_lr),
                                               float(pb["nnr"]), m12.ctypes.data_as(IP), C.byref(cnt)), "matchGrid (points)")
        else:
            end = _i32(np.asarray(pb["cell1_end"]).reshape(-1, 2))
            dir2 = np.ascontiguousarray(np.asarray(pb["dir2"], np.float64).reshape(-1, 2))
            _ok(lib().refpin_match_grid_lines(g.h, n1, cell1.ctypes.data_as(IP), end.ctypes.data_as(IP),
                                              desc1.ctypes.data_as(BP), n2, desc2.ctypes.data_as(BP), dir2.ctypes.data_as(DP),
                                              w.ctypes.data_as(IP), int(best_lr), float(pb["nnr"]), float(pb["line_sim_th"]),
                                              m12.ctypes.data_as(IP), C.byref(cnt)), "matchGrid (lines)")
    return m12[:n1].copy(), int(cnt.value)


def bow(ids, values, normalize_l1=True, if_not_exist=None):
    """A BowVector after addWeight(ids[k], values[k]) in order (addIfNotExist where if_not_exist[k]) and
    normalize(L1): (ids uint32, values float64) in map order."""
    h = lib().refpin_bow_new()
    try:
        for k, (i, v) in enumerate(zip(ids, values)):
            f = lib().refpin_bow_add_if_not_exist if if_not_exist is not None and if_not_exist[k] else lib().refpin_bow_add_weight
            _ok(f(h, int(i), float(v)), "BowVector add")
        if normalize_l1:
            _ok(lib().refpin_bow_normalize_l1(h), "BowVector::normalize")
        n = C.c_int32(0)
        _ok(lib().refpin_bow_entries(h, None, None, 0, C.byref(n)), "refpin_bow_entries")
        oi, ov = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.float64)
        _ok(lib().refpin_bow_entries(h, oi.ctypes.data_as(C.POINTER(C.c_uint32)), ov.ctypes.data_as(DP), n.value, C.byref(n)),
            "refpin_bow_entries")
        return oi[:n.value].copy(), ov[:n.value].copy()
    finally:
        lib().refpin_bow_free(h)
