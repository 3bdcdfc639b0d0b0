"""TEST INFRASTRUCTURE: the zero-pivot matrix shared by tests/test_gpu_zero_pivot.py (every
factorisation of the reduced camera system against the checker) and tests/test_zero_pivot_oracle.py
(the checker's own preconditions for exactly these cases, and the planner's mode for each), and
the checker results computed once for both.

A case is a window, the environment switches that select a factorisation, the structure an upload
must report for it (nf free poses, envelope width bw, the mode of plba_factor_plan) and the rows
of the reduced camera system that receive the special keyframe. Row r is the r-th free pose in
increasing kf_id; it is the factorisation's row r because no case lets the reordering run
(bw <= kClMaxBW = 9, or PLBA_NO_RCM=1).

Windows are those of tests/test_gpu_edge_cases.py and tests/test_gpu_dense.py at their smallest
sizes, with track_min = 3: a landmark that loses the zero-information keyframe's observation still
has two, so its own block stays regular at lambda = 0 and the only singular pivots are the
keyframe's.

Not in the table: a one-sweep band window with 24 < bw <= 27 (512-thread workgroups). Consecutive
keyframes of plba.synth see a common landmark over at most 22 free poses (3000 points with tracks
of 20..n_kf keyframes, n_kf = 30..58: bw 22 every time), and its revisit observations need a loop
of 126 keyframes."""
from __future__ import annotations

import collections
import functools

import numpy as np

import graph_mut as gm
import oracle_api as oa
from plba import synth

# plba_factor_plan's out[0] (FactorMode, csrc/plba_plan.hpp)
DENSE_SCALAR, DENSE_MFMA, BAND, BAND_TW, CL, CL_TW, BCR = range(7)
# every factorisation: the seven modes, block cyclic reduction fused and split
ALL_MODES = {(DENSE_SCALAR, 0), (DENSE_MFMA, 0), (BAND, 0), (BAND_TW, 0), (CL, 0), (CL_TW, 0), (BCR, 1), (BCR, 0)}

WINDOWS = {
    # column-lane sweeps of test_column_lane_factorisation_bandwidths
    "cl14-3": ("C1L", dict(n_kf=14, n_pt=420, n_ln=84, seed=317, track_min=3, track_max=3, fixed_frac=0.1)),
    "cl14-10": ("C1L", dict(n_kf=14, n_pt=420, n_ln=84, seed=324, track_min=3, track_max=10, fixed_frac=0.1)),
    # (seed 353, the sweep's own, is its ill-conditioned window: the checker against itself with the
    # edges in another order already differs by up to 110 element bars; with seed 356 by 0.01)
    "cl48-5": ("C1L", dict(n_kf=48, n_pt=1440, n_ln=288, seed=356, track_min=3, track_max=5, fixed_frac=0.1)),
    # test_wide_bands_and_dense_fallback / test_twisted_factorisation_matches_single_sweep
    "b16-16": ("C1", dict(n_kf=16, n_pt=400, seed=21, track_min=3, track_max=16, fixed_frac=0.1)),
    "b24-12": ("C1", dict(n_kf=24, n_pt=400, seed=17, track_min=3, track_max=12, fixed_frac=0.1)),
    # (also the dense window of test_dense_mfma_factorisation. Seed 35 with track_min = 3 leaves the
    # last keyframe one observation, a rank-2 block: at lambda = 0 the checker then fails every solve
    # of the unmodified window too. With seed 38 every free keyframe has 15 or more.)
    "b30-30": ("C1", dict(n_kf=30, n_pt=400, seed=38, track_min=3, track_max=30, fixed_frac=0.1)),
    "b60-12": ("C1", dict(n_kf=60, n_pt=1500, seed=77, track_min=3, track_max=12)),
    # test_block_cyclic_reduction_matches_oracle
    "bcr30-3": ("C1L", dict(n_kf=30, n_pt=750, n_ln=150, seed=533, track_min=3, track_max=3, fixed_frac=0.1)),
    "bcr40-5": ("C1L", dict(n_kf=40, n_pt=1000, n_ln=200, seed=545, track_min=3, track_max=5, fixed_frac=0.1)),
    "bcr64-8": ("C1L", dict(n_kf=64, n_pt=1600, n_ln=320, seed=572, track_min=3, track_max=8, fixed_frac=0.1)),
}

Case = collections.namedtuple("Case", "id window env mode fused nf bw stats rows")


def tw_split(nf, bw):
    """Two-sided kernels: rows 0..m-1 go top-down, m..m+bw-1 are the separator (csrc/plba_plan.hpp)."""
    return (nf - bw + 1) // 2


def _uniq(rows):
    return tuple(dict.fromkeys(rows))


def _rows_cl(nf, bw):
    return _uniq((0, 1, bw, nf - 1 - bw, nf - 1))


def _rows_band(nf, bw):
    return _uniq((0, 1, nf - 1 - bw, nf - 2, nf - 1))


def _rows_tw(nf, bw):
    # first; last top-down; first and last separator; last bottom-up; last
    m = tw_split(nf, bw)
    return _uniq((0, m - 1, m, m + bw - 1, m + bw, nf - 1))


def _rows_bcr(nf, bw):
    # super-row 0; super-row 1 (odd: eliminated at the first level); super-rows 2 and 4 (even and
    # interior: they survive one and two levels); the first row of the last super-row; last
    N = -(-nf // bw)
    assert N >= 6
    return _uniq((bw // 2, bw, 3 * bw - 1, 5 * bw - 1, (N - 1) * bw, nf - 1))


def _rows_dense(nf, bw):
    # pose 5 is scalar rows 30..35 (tiles 0 and 1 of kTile = 32); poses 10 and 11 lie around scalar 64
    return (0, 5, 10, 11, nf - 1)


def _banded(**kw):
    st = dict(banded=1, column_lane=0, twisted=0, bcr_rows=0, dense_mfma=0)
    st.update(kw)
    return st


def _case(cid, window, env, mode, nf, bw, rows, fused=0, **flags):
    env, stats = dict(env), dict(nf=nf, bw=bw, **flags)
    if bw > 9:  # the reordering runs iff bw > kClMaxBW and PLBA_NO_RCM is unset
        env["PLBA_NO_RCM"] = "1"
    return Case(cid, window, env, mode, fused, nf, bw, stats, rows(nf, bw))


_CL, _BAND, _BCR = {"PLBA_FACTOR": "cl"}, {"PLBA_FACTOR": "band"}, {"PLBA_FACTOR": "bcr", "PLBA_SPEC_BCR": "0"}
_DENSE = {"PLBA_FORCE_DENSE": "1", "PLBA_NO_RCM": "1"}

CASES = [
    # column-lane, one sweep
    _case("cl-bw2", "cl14-3", _CL, CL, 13, 2, _rows_cl, **_banded(column_lane=1)),
    _case("cl-bw9", "cl14-10", _CL, CL, 13, 9, _rows_cl, **_banded(column_lane=1)),
    # column-lane, two-sided
    _case("cltw-bw4", "cl48-5", _CL, CL_TW, 43, 4, _rows_tw, **_banded(column_lane=1, twisted=1)),
    # register-window band kernel, one sweep (bw <= 24: 768 threads)
    _case("band-bw2", "cl14-3", _BAND, BAND, 13, 2, _rows_band, **_banded()),
    _case("band-bw9", "cl14-10", _BAND, BAND, 13, 9, _rows_band, **_banded()),
    _case("band-full", "b16-16", {}, BAND, 14, 13, _rows_band, **_banded()),  # bw = nf-1: the window starts full
    _case("band-bw11", "b24-12", {}, BAND, 22, 11, _rows_band, **_banded()),
    _case("band-bw21", "b30-30", {}, BAND, 27, 21, _rows_band, **_banded()),
    # band kernel, two-sided with its separator solve (bw 11: the multi-wave Gauss-Jordan)
    _case("bandtw-bw4", "cl48-5", _BAND, BAND_TW, 43, 4, _rows_tw, **_banded(twisted=1)),
    _case("bandtw-bw11", "b60-12", {}, BAND_TW, 54, 11, _rows_tw, **_banded(twisted=1)),
    # block cyclic reduction, fused and split (27 = 13*2 + 1 and 58 = 8*7 + 2: a partial last super-row)
    _case("bcr-bw2", "bcr30-3", _BCR, BCR, 27, 2, _rows_bcr, fused=1, **_banded(bcr_rows=14, bcr_fused=1)),
    _case("bcr-bw4", "bcr40-5", _BCR, BCR, 36, 4, _rows_bcr, fused=1, **_banded(bcr_rows=9, bcr_fused=1)),
    _case("bcr-bw7", "bcr64-8", _BCR, BCR, 58, 7, _rows_bcr, fused=1, **_banded(bcr_rows=9, bcr_fused=1)),
    _case("bcr-bw2-split", "bcr30-3", dict(_BCR, PLBA_BCR_SPLIT="1"), BCR, 27, 2, _rows_bcr, fused=0,
          **_banded(bcr_rows=14, bcr_fused=0)),
    # dense, scalar and MFMA panels, the latter also with the substitution vector in global memory
    _case("dense-scalar", "b30-30", dict(_DENSE, PLBA_DENSE_SCALAR="1"), DENSE_SCALAR, 27, 21, _rows_dense,
          banded=0, dense_mfma=0),
    _case("dense-mfma", "b30-30", _DENSE, DENSE_MFMA, 27, 21, _rows_dense, banded=0, dense_mfma=1),
    _case("dense-mfma-yglobal", "b30-30", dict(_DENSE, PLBA_SOLVE_LDS_N="0"), DENSE_MFMA, 27, 21, _rows_dense,
          banded=0, dense_mfma=1),
]
BY_ID = {c.id: c for c in CASES}


def case_rows():
    """(case id, row) of the whole matrix."""
    return [(c.id, r) for c in CASES for r in c.rows]


def window_rows():
    """(window, row) pairs of the matrix: what the checker has to agree to, once per pair."""
    return sorted({(c.window, r) for c in CASES for r in c.rows})


def structure(g):
    """(nf, bw) of a window in id order, as the upload computes them (envelope(), csrc/plba.hip):
    the largest distance in free-pose rows between a keyframe and the first keyframe of a
    landmark it observes."""
    rows = gm.free_rows(g)
    hid = np.full(g.n_kf, -1, np.int64)
    hid[rows] = np.arange(len(rows))
    lm = np.concatenate([g.ept_lm, g.n_pt + g.eln_lm])
    h = hid[np.concatenate([g.ept_kf, g.eln_kf])]
    lo = np.full(g.n_pt + g.n_ln, len(rows), np.int64)
    np.minimum.at(lo, lm[h >= 0], h[h >= 0])
    return len(rows), int((h - lo[lm])[h >= 0].max(initial=0))


@functools.lru_cache(maxsize=None)
def window(name):
    """(read-only: shared by the tests)"""
    cfg, kw = WINDOWS[name]
    return synth.generate(cfg, **kw)


@functools.lru_cache(maxsize=None)
def zero_window(name, row):
    return gm.zero_information_keyframe(window(name), row=row)


@functools.lru_cache(maxsize=None)
def zero_oracle_gn(name, row):
    """The checker's Huber stage at tau = 0 (lambda = 0) on the zero-information window."""
    return oa.lba_plucker(zero_window(name, row), tau=0.0, stage_iters=(5, 0))


@functools.lru_cache(maxsize=None)
def zero_oracle(name, row):
    """The checker's full schedule at the default tau on the zero-information window."""
    return oa.lba_plucker(zero_window(name, row))


# ---- the idle free pose (no edge): one window per factorisation; first row, the row at which the
# factorisation changes hands, last row. The idle pose widens the envelope of what it sits inside,
# so the boundary row is found on the window that contains it.
IdleCase = collections.namedtuple("IdleCase", "id window env stats boundary")

IDLE_CASES = [
    IdleCase("cl", "cl14-3", _CL, dict(banded=1, column_lane=1, twisted=0), lambda r, nf, bw: r == bw),
    IdleCase("cltw", "cl48-5", _CL, dict(banded=1, column_lane=1, twisted=1), lambda r, nf, bw: r == tw_split(nf, bw)),
    IdleCase("band", "cl14-3", _BAND, dict(banded=1, column_lane=0, twisted=0, bcr_rows=0),
             lambda r, nf, bw: r == nf - 1 - bw),
    IdleCase("band-bw11", "b24-12", {"PLBA_NO_RCM": "1"}, dict(banded=1, column_lane=0, twisted=0, bcr_rows=0),
             lambda r, nf, bw: r == nf - 1 - bw),
    IdleCase("bandtw", "cl48-5", _BAND, dict(banded=1, column_lane=0, twisted=1),
             lambda r, nf, bw: r == tw_split(nf, bw)),
    IdleCase("bandtw-bw11", "b60-12", {"PLBA_NO_RCM": "1"}, dict(banded=1, column_lane=0, twisted=1),
             lambda r, nf, bw: r == tw_split(nf, bw)),
    IdleCase("bcr", "bcr40-5", _BCR, dict(banded=1, bcr_fused=1), lambda r, nf, bw: r == (-(-nf // bw) - 1) * bw),
    # (boundary rows: the first row of the last super-row, and the first row of super-row 1)
    IdleCase("bcr-split", "bcr30-3", dict(_BCR, PLBA_BCR_SPLIT="1"), dict(banded=1, bcr_fused=0),
             lambda r, nf, bw: r == bw),
    IdleCase("dense-scalar", "b30-30", dict(_DENSE, PLBA_DENSE_SCALAR="1"), dict(banded=0, dense_mfma=0),
             lambda r, nf, bw: r == 5),
    IdleCase("dense-mfma", "b30-30", _DENSE, dict(banded=0, dense_mfma=1), lambda r, nf, bw: r == 5),
]
IDLE_BY_ID = {c.id: c for c in IDLE_CASES}
IDLE_KINDS = ("first", "boundary", "last")


@functools.lru_cache(maxsize=None)
def idle_window(name, row):
    return gm.add_idle_free_pose(window(name), row=row)


@functools.lru_cache(maxsize=None)
def idle_row(cid, kind):
    """The row of the idle pose, and (nf, bw) of the window that holds it there."""
    c = IDLE_BY_ID[cid]
    nf0 = structure(window(c.window))[0]
    if kind == "first":
        return (0,) + structure(idle_window(c.window, 0))
    if kind == "last":
        return (nf0,) + structure(idle_window(c.window, nf0))
    for r in range(1, nf0):
        nf, bw = structure(idle_window(c.window, r))
        if c.boundary(r, nf, bw):
            return r, nf, bw
    raise AssertionError(f"{cid}: no row of the window is the boundary row once the idle pose sits there")


def idle_cases():
    return [(c.id, k) for c in IDLE_CASES for k in IDLE_KINDS]


@functools.lru_cache(maxsize=None)
def idle_oracle_gn(name, row):
    return oa.lba_plucker(idle_window(name, row), tau=0.0, stage_iters=(5, 0))
