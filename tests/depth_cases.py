"""TEST INFRASTRUCTURE: windows whose points lie behind cameras, and windows that end the damped
trial loop early, shared by tests/test_depth_oracle.py (what the checker alone must show for them)
and tests/test_gpu_depth.py (the device on them), with the checker results computed once for both.

Behind cameras: graph_mut.points_behind_cameras on C1L. "first" and "mean" are the mutation's
defaults. "short" (landmarks with at most 3 observations) uses every third candidate: with every
seventh the checker leaves 25 edges behind a camera and classifies none of them by depth alone
(every one also has a stage-1 χ² above the threshold); with every third it leaves 49 and
classifies 6 by depth alone.

Early termination (OptimizationAlgorithmLevenberg::solve, the checker's solveIteration), on the
points of C1L alone: with τ = 1e20 the first damping is 1e20 times the largest diagonal entry, the
step is far below one ulp of every estimate, the trial state is bitwise the current one and χ² is
exactly what it was: ρ == 0, the iteration ends after one trial with Terminate. With τ = 2e300 the
first damping of the Huber stage is within a factor two of the largest double: the same ρ == 0
rejection multiplies it by ν = 2 to +inf and the trial loop breaks before it counts the trial (0
trials, Terminate); stage 2 starts lower and ends through ρ == 0. The window has no lines because
the checker's own line update is not idempotent: with the 40 lines of C1L a zero step moves two
orth entries by one ulp, χ² of stage 2 then falls by 4 ulp and the checker accepts that trial, so
its trace there is decided by the rounding of its own sin / cos / atan2, which no other
implementation can be asked to repeat. Points and poses come back bitwise. Every system that is
factorised is finite in both."""
from __future__ import annotations

import functools

import numpy as np

import graph_mut as gm
import oracle_api as oa
from plba import synth

CHI2_THR = 5.991
VARIANTS = {
    "first": dict(through="first"),
    "mean": dict(through="mean"),
    "short": dict(through="short", every=3),
}
# derived windows of the caller-order tests: the mixed window (Ep < E) and its points alone (Ep == E)
ORDERS = ("mixed", "points")
SHUFFLE_SEED = 3


@functools.lru_cache(maxsize=None)
def window(name):
    return gm.points_behind_cameras(synth.generate("C1L"), **VARIANTS[name])


@functools.lru_cache(maxsize=None)
def order_windows(order):
    """(window, shuffled window) of the caller-order tests, from the "first" variant."""
    g = window("first") if order == "mixed" else gm.drop_lines(window("first"))
    return g, gm.shuffled(g, seed=SHUFFLE_SEED)


@functools.lru_cache(maxsize=None)
def _oracle(key, stage1):
    kind, name = key
    g = window(name) if kind == "v" else order_windows(name[0])[name[1]]
    return oa.lba_plucker(g, **({"stage_iters": (5, 0)} if stage1 else {}))


def oracle(name):
    """Full schedule of the checker on a variant (shared: do not modify)."""
    return _oracle(("v", name), False)


def oracle_stage1(name):
    """The checker after optimize(5) of the Huber stage: the g2o-style call sequence's state at the
    classification (stage 2 runs no iteration)."""
    return _oracle(("v", name), True)


def order_oracle(order, shuffled, stage1=False):
    return _oracle(("o", (order, int(shuffled))), stage1)


def depth_only(ref, ref1):
    """Edges the stage switch puts on level 1 for their depth alone: behind the camera with a
    stage-1 χ² at or below the threshold. ref1's χ² is the one the classification read when the
    Huber stage ended on an accepted trial (stage1_ends_on_accept): the level-1 refresh then
    evaluates the same edges at the same state."""
    return (ref["ept_level"] == 1) & (ref1["ept_depth_ok"] == 0) & (ref1["ept_chi2"] <= CHI2_THR)


def stage1_ends_on_accept(ref1):
    t = ref1["trace"][-1]
    return t["stage"] == 0 and t["result"] == 0 and t["trials"] < 10 and t["chi2_end"] < t["chi2_start"]


def depths(g, est):
    """|Pc[2]| margins are taken at the start (est = None), at the stage switch and at the end."""
    if est is None:
        return gm.point_depths(g.kf_Tcw, g.pt_xyz, g.ept_kf, g.ept_lm)
    return gm.point_depths(est["kf_Tcw"], est["pt_xyz"], g.ept_kf, g.ept_lm)


# ---- the no-solve window: depths of exactly 0.0, -0.0, 5e-324, -5e-324 in the second keyframe
TINY = 5e-324
NO_SOLVE_DEPTHS = (0.0, -0.0, TINY, -TINY, 3.0, 5.0)
NO_SOLVE_FLAGS_KF1 = (0, 0, 1, 0, 1, 1)


@functools.lru_cache(maxsize=None)
def no_solve_window():
    """2 keyframes (identity rotations; t = (0, 0, 4) fixed and t = (0.5, 0, -0.0) free) and 6
    points, each seen by both. Pc[2] = 0·X + 0·Y + 1·Z + t_z is exact: Z + 4 in the first keyframe
    (4, 7 or 9) and Z itself in the second; the point at depth -0.0 has X, Y < 0 so that every
    term of the sum is -0.0. Edges are landmark-major: 2j is point j in the first keyframe, 2j + 1
    in the second."""
    T = np.zeros((2, 3, 4))
    T[:, :, :3] = np.eye(3)
    T[0, :, 3] = (0.0, 0.0, 4.0)
    T[1, :, 3] = (0.5, 0.0, -0.0)
    P = np.array([[0.0, 0.0, 0.0], [-0.25, -0.5, -0.0], [0.25, 0.5, TINY], [0.5, -0.25, -TINY],
                  [0.25, 0.125, 3.0], [-0.5, 0.25, 5.0]])
    assert tuple(P[:, 2]) == NO_SOLVE_DEPTHS
    c = synth.CAMERA
    n = len(P)
    lm = np.repeat(np.arange(n, dtype=np.int32), 2)
    kf = np.tile(np.arange(2, dtype=np.int32), n)
    obs = np.tile(np.array([c["cx"] + 3.0, c["cy"] - 2.0]), (2 * n, 1))
    return synth.Graph(
        fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"],
        kf_Tcw=T, kf_fixed=np.array([1, 0], np.uint8), kf_id=np.arange(2, dtype=np.int32),
        pt_xyz=P, pt_id=(np.arange(n) + 3).astype(np.int32),
        ln_orth=np.zeros((0, 4)), ln_id=np.zeros(0, np.int32),
        ept_lm=lm, ept_kf=kf, ept_obs=obs, ept_info=np.ones(2 * n),
        eln_lm=np.zeros(0, np.int32), eln_kf=np.zeros(0, np.int32), eln_obs=np.zeros((0, 4)),
        eln_info=np.zeros(0))


@functools.lru_cache(maxsize=None)
def no_solve_oracle():
    """The checker without an iteration: depth flags of every edge, and computeError() + chi2() of
    every edge through its own edge function."""
    g = no_solve_window()
    ref = oa.lba_plucker(g, stage_iters=(0, 0))
    cam = (g.fx, g.fy, g.cx, g.cy)
    chi2 = np.zeros(g.n_ept)
    with np.errstate(all="ignore"):
        for e in range(g.n_ept):
            err, _, _ = oa.point_edge(g.kf_Tcw[g.ept_kf[e]], g.pt_xyz[g.ept_lm[e]], g.ept_obs[e], cam)
            chi2[e] = err[0] * (g.ept_info[e] * err[0]) + err[1] * (g.ept_info[e] * err[1])
    return ref, chi2


# ---- windows that end the trial loop early (τ through Solver(tau=...) / the checker's opts)
TERMINATION = {
    "rho0": dict(tau=1e20),     # ρ == 0 after one trial
    "lambda_inf": dict(tau=2e300),  # λ·ν overflows in the first trial of the Huber stage
}


@functools.lru_cache(maxsize=None)
def termination_window():
    return gm.drop_lines(synth.generate("C1L"))


@functools.lru_cache(maxsize=None)
def termination_oracle(name):
    return oa.lba_plucker(termination_window(), **TERMINATION[name])
