"""Growth and reuse of the scratch blocks behind plba_desc_match / plba_grid_match / plba_stereo_associate
(one shared block), plba_lc_relative_pose, plba_pgo_optimize and plba_bow_insert: a call on a block that an
earlier, larger call left full of stale bytes, or that has just grown, must give bit for bit what the same call
gives on a fresh context. Every array of a block owns at least 256 bytes, empty ones included, so one pair has
an empty side and one relative-pose candidate has no lines (and one nothing at all)."""
import struct

import numpy as np
import pytest

import bow_cases as bcases
import descmatch_cases as dcases
import gridmatch_cases as gcases
import lcpose_cases as lcases
import ref_bow
import ref_stereo
import stereo_cases as scases
from plba import pgo

pytestmark = pytest.mark.gpu

GRID = min(gcases.parity_cases() + gcases.boundary_cases(), key=lambda c: (c[1] + c[2]) * c[3])
LC_BATCH = [(40, 12), lcases.EMPTY_SHAPE, (64, 0)]
BOW_VOCAB = min(bcases.VOCABS, key=lambda name: len(bcases.vocab(name)["word_id"]))
BOW_SMALL, BOW_LARGE = 5, max(bcases.N_DESC)


def _bits(x):
    """A result as nested tuples of bytes: equality is bitwise (NaN and -0.0 included)."""
    if isinstance(x, dict):
        return tuple((k, _bits(v)) for k, v in sorted(x.items()) if k != "solve_ms")
    if isinstance(x, (list, tuple)):
        return tuple(_bits(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, float):
        return struct.pack("d", x)
    return x


def _calls():
    small = [dcases.pair(3, 2), dcases.pair(5, 0)]           # the second pair has an empty side
    large = [dcases.pair(300, 257)]
    grid = [gcases.problem(*GRID)]
    lc3 = [lcases.problem(*s) for s in LC_BATCH]
    graphs = {n: pgo.loop_graph(n_kf=n, seed=11) for n in (6, 40)}
    one_point = [scases.frame(9, n_pt=(1, 1))]               # one left and one right point, no lines
    stereo_large = [scases.case(scases.LARGEST)]
    sprm = ref_stereo.params(**scases.CAMERA)
    return dict(desc_small=lambda s: s.desc_match(small, 0.9),
                grid=lambda s: s.grid_match(grid, gcases.COLS, gcases.ROWS, True, desc_bytes=GRID[3]),
                desc_large=lambda s: s.desc_match(large, 0.9),
                stereo_one=lambda s: s.stereo_associate(one_point, sprm),
                stereo_large=lambda s: s.stereo_associate(stereo_large, sprm),
                lc3=lambda s: s.lc_relative_pose(lc3),
                lc1=lambda s: s.lc_relative_pose(lc3[:1]),
                pgo6=lambda s: s.pgo_optimize(graphs[6]),
                pgo40=lambda s: s.pgo_optimize(graphs[40]))


def test_a_reused_or_grown_block_gives_the_fresh_context_result_bitwise():
    from plba.lib import Solver
    calls = _calls()
    assert GRID[1] == 1 and LC_BATCH[1] == (0, 0)
    # the witness: a fresh context on which no call finds a block that held a larger problem
    with Solver() as w:
        fresh = {k: _bits(calls[k](w)) for k in ("stereo_one", "grid", "desc_small", "desc_large", "stereo_large",
                                                 "lc1", "lc3", "pgo6", "pgo40")}
    order = ["desc_small", "grid", "desc_large", "stereo_one", "grid", "stereo_large", "stereo_one", "lc3", "lc1",
             "pgo6", "pgo40", "pgo6"]
    with Solver() as s:
        for step, k in enumerate(order):
            assert _bits(calls[k](s)) == fresh[k], (step, k)
    # the calls did something: matches found, a candidate accepted, the pose graph converged
    assert fresh["desc_large"][0][1] > 0 and dict(fresh["lc3"][0])["accepted"] == 1
    assert dict(fresh["pgo40"])["iterations"] > 0 and dict(fresh["stereo_large"][0])["n_pt"] > 0


def _bow_small_insert(s, after_a_larger_keyframe):
    """The small keyframe's score list and stored vector; first, if asked, a larger keyframe comes and goes."""
    s.bow_set_vocab(0, bcases.vocab(BOW_VOCAB))
    if after_a_larger_keyframe:
        s.bow_insert(0, 0, bcases.descriptors(BOW_VOCAB, BOW_LARGE))
        s.bow_remove(0, 0)
    return _bits((s.bow_insert(0, 1, bcases.descriptors(BOW_VOCAB, BOW_SMALL)), s.bow_get(0, 1)))


def test_a_small_insert_on_a_grown_stale_bow_block_gives_the_fresh_context_result_bitwise():
    from plba.lib import Solver
    with Solver() as w:
        fresh = _bow_small_insert(w, False)
    with Solver() as s:
        assert _bow_small_insert(s, True) == fresh
    # the checker's answer for either history: no live row but the new one, which scores against itself
    vec = ref_bow.transform(bcases.vocab(BOW_VOCAB), bcases.descriptors(BOW_VOCAB, BOW_SMALL))
    assert len(vec) > 0
    assert fresh == _bits(((np.array([1], np.int32), np.array([ref_bow.score(vec, vec)])), bcases.as_arrays(vec)))
