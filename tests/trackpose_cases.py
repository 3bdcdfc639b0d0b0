"""TEST INFRASTRUCTURE: the frame pairs that the frame-to-frame pose tests share (plba_track_pose).

Every case is a named problem with its parameters; the numpy checker's result (tests/ref_trackpose.py)
is computed once per case and line model and cached. tests/test_trackpose_oracle.py checks that every
decision of every case used on the GPU stays away from its threshold (margins()); a case that does
not is given another seed HERE, never skipped there.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field, replace

import numpy as np

import ref_trackpose as rt
from plba import capi, trackpose as tp

MODELS = (capi.TRACK_PLUCKER, capi.TRACK_ENDPOINTS)
MODEL_IDS = ("plucker", "endpoints")

# The rounding the two sides may differ by: the device sums H, g and e in a tree, the checker in match
# order. Measured between the checker and the match-order C++ restatement: below 1e-12 relative on every
# figure. Each decision has to stay at least this far (relative, or absolute for a residual in pixels)
# from its threshold.
MARGIN_REL = 1e-6
MARGIN_PX = 1e-6


@dataclass(frozen=True)
class Case:
    name: str
    n_pt: int
    n_ln: int
    seed: int = 0
    synth_kw: tuple = ()
    param_kw: tuple = ()
    edit: object = None     # a function TrackProblem -> TrackProblem applied after synth

    def problem(self):
        return _problem(self)

    def params(self, model, **kw):
        d = dict(self.param_kw)
        d.update(kw)
        for k, v in list(d.items()):
            if callable(v):
                d[k] = v(self, model)
        return capi.track_params(line_model=model, **d)

    def reference(self, model):
        return _reference(self, model)


@functools.lru_cache(maxsize=None)
def _problem(case):
    kw = dict(outlier_frac=0.2)
    kw.update(dict(case.synth_kw))
    pr = tp.synth(case.n_pt, case.n_ln, seed=case.seed, **kw)
    return case.edit(pr) if case.edit else pr


@functools.lru_cache(maxsize=None)
def _reference(case, model):
    return rt.track_pose(case.problem(), case.params(model))


# ---- parity: the sizes of the issue, 20 % gross outliers. Below ten matches min_features is 1, so that
# the loops run there too (they end in FIRST_NOT_GOOD: six unknowns from one to five rows).
SIZES = ((0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (255, 0), (256, 257), (300, 100))
PARITY = tuple(Case(f"parity_{a}_{b}", a, b, seed=3, param_kw=(("min_features", 1 if a + b < 10 else 10),))
               for a, b in SIZES)


# ---- pass-0 probes: one pass at the identity on all matches, then too few inliers (min_features = all),
# so s_p and s_l are those of that pass. 63 / 64 / 65 active matches of each kind, and medians inside ties.
def _tied(pr):
    """Every match three times: the median and the MAD fall inside a run of equal values."""
    rep = lambda a: np.ascontiguousarray(np.repeat(a, 3, axis=0))
    return replace(pr, **{k: rep(getattr(pr, k)) for k, _ in capi.TrackBatchView.FIELDS},
                   pt_outlier=rep(pr.pt_outlier), ln_outlier=rep(pr.ln_outlier))


_all = lambda case, model: len(case.problem().pt_P) + len(case.problem().ln_sP)
PROBE_KW = (("max_iters", 1), ("max_iters_ref", 1), ("min_features", _all))
PROBE_MOTION = (("rot_deg", 0.05), ("trans", 0.002))   # residuals of a pixel at the identity: no scale is clamped
PROBES = tuple(Case(f"probe_{a}_{b}", a, b, seed=5, synth_kw=PROBE_MOTION, param_kw=PROBE_KW)
               for a, b in ((63, 65), (64, 64), (65, 63))) + (
    Case("probe_ties", 21, 22, seed=6, synth_kw=PROBE_MOTION, param_kw=PROBE_KW, edit=_tied),)


# ---- the five branches, and the inputs the reference leaves undefined
def _same_point(pr):
    """Every point match is the same 3-D point seen at scattered pixels, no lines: H has rank two."""
    n = len(pr.pt_P)
    rng = np.random.default_rng(11)
    P = np.tile(pr.pt_P[:1], (n, 1))
    obs = tp._project(P, pr.cam) + tp._disc(rng, n, 2.0)
    return replace(pr, pt_P=np.ascontiguousarray(P), pt_obs=np.ascontiguousarray(obs))


def _z0(pr):
    P = pr.pt_P.copy()
    P[7] = (0.3, 0.2, 0.0)
    return replace(pr, pt_P=P)


def _min_error_between(case, model):
    """Between e of the refinement's first pass (inliers at the identity) and e of the first loop's."""
    ref = rt.track_pose(case.problem(), capi.track_params(line_model=model))
    e0 = [t["e"] for t in ref["trace"] if t["phase"] == 0][0]
    e1 = [t["e"] for t in ref["trace"] if t["phase"] == 1][0]
    assert e1 < e0
    return float(np.sqrt(e0 * e1))


BRANCH = {
    capi.TRACK_OK: Case("ok", 60, 20, seed=2),
    capi.TRACK_FEW_BEFORE: Case("few_before", 4, 3, seed=2),
    capi.TRACK_FIRST_NOT_GOOD: Case("first_not_good_rank_deficient", 24, 0, seed=2, edit=_same_point),
    capi.TRACK_FEW_AFTER: Case("few_after", 60, 20, seed=2, param_kw=(("min_features", 80),)),
    # no motion, so the refinement starts at the identity with e already below min_error: it stops on its
    # first pass, DT == Identity exactly, and the final test fails on that comparison
    capi.TRACK_FINAL_NOT_GOOD: Case("final_not_good_identity", 60, 20, seed=2,
                                    synth_kw=(("rot_deg", 0.0), ("trans", 0.0)),
                                    param_kw=(("min_error", _min_error_between),)),
}
Z0 = Case("z0_match", 40, 12, seed=4, edit=_z0)


def _prev(DT, cov_scale, err):
    return np.concatenate([np.asarray(DT, np.float64).ravel(), (cov_scale * np.eye(6)).ravel(), [err]])


def _motion(err):
    def edit(pr):
        DT = np.eye(4)
        DT[:3, 3] = (0.01, -0.02, 0.015)
        return replace(pr, prev=_prev(DT, 1e-4, err))
    return edit


MOTION_ACCEPTED = Case("motion_accepted", 60, 20, seed=2, param_kw=(("use_motion_model", 1),), edit=_motion(0.5))
MOTION_REJECTED = Case("motion_rejected", 60, 20, seed=2, param_kw=(("use_motion_model", 1),), edit=_motion(2.0))

GPU_CASES = PARITY + PROBES + tuple(BRANCH.values()) + (MOTION_ACCEPTED, MOTION_REJECTED)


def margins(case, model) -> dict:
    """The smallest distance of each kind of decision to its threshold, over the whole run of the checker."""
    ref, p = case.reference(model), case.params(model)
    m = dict(inlier=np.inf, stop=np.inf, good=np.inf, features=np.inf)
    for rem in ref["removal"].values():
        if len(rem["res"]):
            m["inlier"] = min(m["inlier"], float(np.abs(np.abs(rem["res"] - rem["mean"]) - rem["th"]).min()))
    for t in ref["trace"]:
        if t["N"] == 0:
            continue
        m["stop"] = min(m["stop"], abs(t["de"] - p.min_error_change) / p.min_error_change,
                        abs(t["e"] - p.min_error) / p.min_error)
        if t["x_norm"] is not None:
            m["stop"] = min(m["stop"], abs(t["x_norm"] - p.min_error_change) / p.min_error_change)
        if t["logdet"] is not None:
            m["good"] = min(m["good"], abs(t["logdet"]))
    for g in (ref["good_first"], ref["good_final"]):
        if g is None or not np.isfinite(g["ev"]).all():
            continue
        if g["err"] != -1.0:   # (err >= 0 is a sum of non-negative terms: no rounding makes it negative)
            m["good"] = min(m["good"], abs(g["err"] - 1.0), abs(g["ev"][5] - 1.0))
            # the smallest eigenvalue against 0, relative to the largest
            m["good"] = min(m["good"], abs(g["ev"][0]) / abs(g["ev"][5]))
    n_all = case.problem().n_pt + case.problem().n_ln
    m["features"] = min(abs(n_all - (p.min_features - 0.5)),
                        abs(ref["n_inl_pt"] + ref["n_inl_ln"] - (p.min_features - 0.5)))
    return m
