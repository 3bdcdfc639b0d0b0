"""TEST INFRASTRUCTURE: the frame pairs that the frame-to-frame tracking tests share (plba_track_frames).

A case is a named batch of frame pairs with its parameters; the checker's result (tests/ref_trackframes.py)
is computed once per case and line model and cached. The pairs are synthetic and seeded: a pose problem of
plba.trackpose.synth is spread over a previous and a current frame by plba.trackframes.from_problem, its
matches carry descriptors a few bits apart (d0 <= 4 against a second distance of about 100: the ratio test
passes by far), every other row a random descriptor (d0 / d1 above 0.9 by a margin that
tests/test_trackframes_oracle.py asserts, with every other decision's margin). A case that does not hold a
margin there gets another seed HERE; it is never loosened or skipped.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import numpy as np

import ref_trackframes as rf
import trackpose_cases as pcases
from plba import capi, trackframes as tf, trackpose as tp

MODELS, MODEL_IDS = pcases.MODELS, pcases.MODEL_IDS
# |d0 - nnr·d1| of every row of every matching direction stays above this: the float product of :54 is
# exact to 512 · 2^-24 = 3e-5, so the float and the double decision agree
MARGIN_RATIO = 1e-3


@dataclass(frozen=True)
class Case:
    name: str
    build: object            # () -> tuple of FramePair
    track_kw: tuple = ()     # over capi.track_params
    match_kw: tuple = ()     # nnr_pt, nnr_ln, best_lr, desc_bytes over capi.frames_params

    def pairs(self):
        return _pairs(self)

    def params(self, model, **kw):
        d = dict(self.track_kw)
        d.update(kw)
        return capi.frames_params(capi.track_params(line_model=model, **d), **dict(self.match_kw))

    def reference(self, model):
        return _reference(self, model)


@functools.lru_cache(maxsize=None)
def _pairs(case):
    return tuple(case.build())


@functools.lru_cache(maxsize=None)
def _reference(case, model):
    """One checker result per pair (read-only: shared by the tests)."""
    return tuple(rf.track_frames(q, case.params(model)) for q in case.pairs())


def _synth(n_pt, n_ln, seed, **kw):
    kw.setdefault("outlier_frac", 0.0)
    return tp.synth(n_pt, n_ln, seed=seed, **kw)


def _second(n):
    """Every second of n rows: 0, 2, ..."""
    return np.arange(0, n, 2)


def _geometry(rng, n1p, n2p, n1l, n2l):
    """Feature arrays of the given row counts for a hand-built descriptor set: any finite values."""
    cam = tp.empty().cam
    P, sP, eP = tf._in_front(rng, n1p, cam), tf._in_front(rng, n1l, cam), tf._in_front(rng, n1l, cam)
    le = rng.normal(size=(n2l, 3))
    return dict(prev_pt_P=P, prev_pt_sigma2=np.ones(n1p), prev_ln_sP=sP, prev_ln_eP=eP,
                prev_ln_NDc=np.concatenate([np.cross(sP, eP).reshape(n1l, 3), eP - sP], 1),
                prev_ln_seg=rng.uniform(20, 400, (n1l, 4)), prev_ln_sigma2=np.ones(n1l),
                cur_pt_pl=rng.uniform(20, 400, (n2p, 2)), cur_ln_seg=rng.uniform(20, 400, (n2l, 4)), cur_ln_le=le)


def _rows(*hexes):
    """Descriptors of 8 bytes from 16 hex digits each."""
    return np.array([list(bytes.fromhex(h)) for h in hexes], np.uint8).reshape(-1, 8)


# ---- D and E by hand, 8-byte descriptors; tests/test_trackframes_oracle.py writes their results out
C0, C1, C2 = "0000000000000000", "ffffffffffffffff", "0f0f0f0f0f0f0f0f"
# previous rows: c1 itself; c0 with one, with two and with no bit set; c2 itself. Without the cross-check
# rows 1, 2 and 3 all have c0 (current row 0) as their nearest: distances 1, 2, 0 against 31, 30, 32 to c2.
D_SMALL_PREV = _rows(C1, "0000000000000001", "0000000000000003", C0, C2)
D_SMALL_CUR = _rows(C0, C1, C2)
# current rows 1 and 3 are the same descriptor, rows 0 and 2 too; previous row 0 is one bit from the first
# pair, row 1 one bit from the second: d0 == d1 == 1, which only a ratio above 1 accepts, and the lower
# index of each pair wins (rows 1 and 0). Previous row 2 equals c1 exactly: d0 = 0 < 1.5 · d1.
E_SMALL_PREV = _rows("0f0f0f0f0f0f0f0e", "0000000000000080", C1)
E_SMALL_CUR = _rows(C0, C2, C0, C2, C1)


def _hand(prev_d, cur_d, seed):
    rng = np.random.default_rng(seed)
    z = np.zeros((0, 8), np.uint8)
    return tf.FramePair(prev_pdesc=prev_d, cur_pdesc=cur_d, prev_ldesc=z, cur_ldesc=z,
                        **_geometry(rng, len(prev_d), len(cur_d), 0, 0))


def _case_a():
    return (tf.from_problem(_synth(12, 12, seed=2), seed=1),)


def _case_b():
    nine = tf.from_problem(_synth(5, 4, seed=3), seed=2, extra=(3, 2, 2, 3))
    lines = tf.from_problem(_synth(0, 12, seed=4), seed=3, extra=(5, 0, 1, 2))   # 5 previous points, no current point
    empty_prev = tf.from_problem(_synth(0, 0, seed=5), seed=4, extra=(0, 6, 0, 4))
    return _case_a() + (nine, lines, empty_prev)


def _case_c():
    """The third pair has four point matches by construction. A MAD over four residuals is a step function of
    the pose, and with a dozen lines the re-weighted iteration does not settle in its ten passes: a rounding
    error grows from pass to pass (seen between the checker and the match-order C++ restatement, two CPU sums
    in the same order). Forty lines carry the pose, and the two agree to a thousandth of the tolerance."""
    waves = np.array([63, 127, 191, 255])
    return (tf.from_problem(_synth(33, 33, seed=6), seed=5, extra=(32, 7, 32, 3), pt_rows=_second(65), ln_rows=_second(65)),
            tf.from_problem(_synth(129, 129, seed=7), seed=6, extra=(128, 5, 128, 9), pt_rows=_second(257), ln_rows=_second(257)),
            tf.from_problem(_synth(4, 40, seed=8), seed=7, extra=(252, 3, 0, 2), pt_rows=waves))


def _case_d():
    """Two more previous point rows, one and two bits from the current row that previous row 4 matches."""
    q = tf.from_problem(_synth(12, 12, seed=9), seed=8, extra=(0, 3, 0, 0))
    rng = np.random.default_rng(81)
    j = int(q.true_pt[4, 1])
    more = np.stack([tf.flip(rng, q.cur_pdesc[j], 1), tf.flip(rng, q.cur_pdesc[j], 2)])
    P = tf._in_front(rng, 2, q.cam)
    big = replace(q, prev_pdesc=np.concatenate([q.prev_pdesc, more]), prev_pt_P=np.concatenate([q.prev_pt_P, P]),
                  prev_pt_sigma2=np.concatenate([q.prev_pt_sigma2, np.ones(2)]))
    return (big,)


def _case_e():
    """Current point row 5's descriptor once more, as a new last row with another pixel; the previous row that
    matches it is at least one bit away, so the two distances are equal and not zero."""
    q = tf.from_problem(_synth(12, 12, seed=10), seed=9)
    rng = np.random.default_rng(91)
    i1, j = (int(v) for v in q.true_pt[5])
    prev_d = q.prev_pdesc.copy()
    prev_d[i1] = tf.flip(rng, q.cur_pdesc[j], 1)
    big = replace(q, prev_pdesc=prev_d, cur_pdesc=np.concatenate([q.cur_pdesc, q.cur_pdesc[j:j + 1]]),
                  cur_pt_pl=np.concatenate([q.cur_pt_pl, q.cur_pt_pl[j:j + 1] + 25.0]))
    return (big,)


def _case_f():
    return (tf.from_problem(_synth(capi.TRACK_MAX_N, 0, seed=1, outlier_frac=0.1), seed=10),)


def too_wide():
    """A previous frame of PLBA_TRACK_MAX_N + 1 point rows: refused before any launch."""
    return tf.from_problem(_synth(capi.TRACK_MAX_N + 1, 0, seed=1), seed=11)


def _case_g():
    return (tf.from_problem(pcases.MOTION_ACCEPTED.problem(), seed=12, extra=(9, 4, 3, 5)),
            tf.from_problem(pcases.MOTION_REJECTED.problem(), seed=13, extra=(9, 4, 3, 5)))


def _case_h():
    return (tf.from_problem(_synth(60, 20, seed=2, outlier_frac=0.2), seed=14, extra=(17, 9, 6, 8)),)


A = Case("A_all_matched", _case_a)
B = Case("B_batch_few_empty", _case_b)
C = Case("C_scan_carries", _case_c)
D = Case("D_no_cross_check", _case_d, match_kw=(("best_lr", False),))
E = Case("E_ties", _case_e, match_kw=(("nnr_pt", 1.5),))
F = Case("F_max_n", _case_f, track_kw=(("max_iters", 2), ("max_iters_ref", 2)))
G = Case("G_motion_model", _case_g, track_kw=(("use_motion_model", 1),))
H = Case("H_outliers", _case_h)
D_SMALL = Case("D_small", lambda: (_hand(D_SMALL_PREV, D_SMALL_CUR, 82),), match_kw=(("best_lr", False), ("desc_bytes", 8)))
E_SMALL = Case("E_small", lambda: (_hand(E_SMALL_PREV, E_SMALL_CUR, 92),), match_kw=(("nnr_pt", 1.5), ("desc_bytes", 8)))

GPU_CASES = (A, B, C, D, E, F, G, H, D_SMALL, E_SMALL)


class PoseView:
    """The pose problem that pair k of a case gathers, with the interface trackpose_cases.margins reads."""

    def __init__(self, case, k):
        self.case, self.k, self.name = case, k, f"{case.name}[{k}]"

    def problem(self):
        return self.case.reference(MODELS[0])[self.k]["problem"]

    def params(self, model):
        return self.case.params(model).track

    def reference(self, model):
        return self.case.reference(model)[self.k]


def ratio_margin(case, model) -> float:
    """The smallest |d0 - nnr·d1| over every row of both matching directions of every pair and kind."""
    p, m = case.params(model), np.inf
    for ref in case.reference(model):
        for det, nnr in ((ref["pt_detail"], p.nnr_pt), (ref["ln_detail"], p.nnr_ln)):
            for side in ((det["fwd"], det["rev"]) if det else ()):
                if len(side["d0"]) and (side["d1"] >= 0).all():
                    m = min(m, float(np.abs(side["d0"] - float(np.float32(nnr)) * side["d1"]).min()))
    return m
