"""TEST INFRASTRUCTURE: the loop-closure relative-pose candidates shared by tests/test_gpu_lcpose.py
(device against the checker) and tests/test_lcpose_oracle.py (the generator's margins of exactly
these candidates), and the checker results computed once for both."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from plba import capi, lcpose

import ref_lcpose

# (n_pt, n_ln): small; more than one stride of 256 and no multiple of 64; one kind only
PARITY_SHAPES = [(40, 12), (300, 100), (64, 0), (0, 64)]
# (n_pt, n_ln, outlier_frac) compared under the caps 3 and 2. Three passes from the identity do not
# reach the pose: with 25 % outliers the outlier pass then keeps three of the (40, 12) matches and four
# of the (64, 0) ones, H is singular (cond₂ ~ 1e17) and no pose is defined to compare; these keep theirs
CAPPED_CASES = [(40, 12, 0.0), (300, 100, 0.25)]
SINGULAR_SHAPE = (1, 0)
EMPTY_SHAPE = (0, 0)
OUTLIER_FRACS = [0.0, 0.25]
VARIANTS = [capi.LCPOSE_ROBUST_GN, capi.LCPOSE_GN]


@functools.lru_cache(maxsize=None)
def problem(n_pt: int, n_ln: int, outlier_frac: float = 0.0):
    """True pose of 5 degrees / 0.2 m, noise <= 1 px."""
    return lcpose.synth(n_pt, n_ln, seed=1000 + 7 * n_pt + n_ln, rot_deg=5.0, trans=0.2, noise_px=1.0,
                        outlier_frac=outlier_frac)


def params(variant: int = capi.LCPOSE_ROBUST_GN, **kw):
    return capi.lcpose_params(variant=variant, **kw)


@functools.lru_cache(maxsize=None)
def reference(n_pt: int, n_ln: int, outlier_frac: float, variant: int, max_iters_first: int = 5, max_iters: int = 10):
    """The checker's result (read-only: shared by the tests)."""
    return ref_lcpose.relative_pose(problem(n_pt, n_ln, outlier_frac),
                                    params(variant, max_iters_first=max_iters_first, max_iters=max_iters))


def parity_cases():
    return [(s[0], s[1], f, v) for s in PARITY_SHAPES for f in OUTLIER_FRACS for v in VARIANTS]


# ---- the candidates away from 5 degrees / 0.2 m / 1 px / EuRoC / homog_th = 1e-7 ----------------------------------

CAM_FY300 = (lcpose.CAMERA["fx"], 300.0, lcpose.CAMERA["cx"], lcpose.CAMERA["cy"])


def scaled(pr, s: float):
    """The scene, its points, endpoints and true translation, times s: the pixels do not change."""
    T = pr.T_true.copy()
    T[:3, 3] *= s
    return dataclasses.replace(pr, pt_P=pr.pt_P * s, ln_sP=pr.ln_sP * s, ln_eP=pr.ln_eP * s, T_true=T)


def mirrored(pr, k: int):
    """Point k mirrored in kf1's image plane to the same distance behind that camera: it still projects
    to a finite pixel, the one opposite the principal point."""
    T, P = pr.T_true, pr.pt_P.copy()
    P1 = (T[:3, :3] @ P[k] + T[:3, 3]) * np.array([1.0, 1.0, -1.0])
    P[k] = T[:3, :3].T @ (P1 - T[:3, 3])
    return dataclasses.replace(pr, pt_P=P)


def zero_depth(pr, k: int):
    """Point k with z = 0 in kf0's frame: the first pass, at T_inc = I, divides by it."""
    P = pr.pt_P.copy()
    P[k, 2] = 0.0
    return dataclasses.replace(pr, pt_P=P)


def permuted(pr, seed: int):
    """The same candidate with its points and its lines reordered; also returns the two orders."""
    rng = np.random.default_rng(seed)
    ip, il = rng.permutation(pr.n_pt), rng.permutation(pr.n_ln)
    q = dataclasses.replace(pr, pt_P=pr.pt_P[ip], pt_obs=pr.pt_obs[ip], ln_sP=pr.ln_sP[il], ln_eP=pr.ln_eP[il],
                            ln_le=pr.ln_le[il], pt_outlier=pr.pt_outlier[ip], ln_outlier=pr.ln_outlier[il])
    return q, ip, il


@dataclasses.dataclass(frozen=True)
class Case:
    """A named candidate: lcpose.synth's arguments, what is done to the scene afterwards, and the
    parameters that differ from the defaults (the variant is chosen by the test)."""
    name: str
    n_pt: int = 40
    n_ln: int = 12
    seed: int | None = None          # None: the seed of problem()
    rot_deg: float = 5.0
    trans: float = 0.2
    noise_px: float = 1.0
    outlier_frac: float = 0.0
    cam: tuple | None = None
    scale: float = 1.0
    mirror: int = -1                 # index of the point put behind the camera
    zero_z: int = -1                 # index of the point with z = 0 in kf0
    prm: tuple = ()                  # ((name, value), ...) of PlbaLcposeParams

    def problem(self):
        return _case_problem(self)

    def params(self, variant: int = capi.LCPOSE_ROBUST_GN, **kw):
        return params(variant, **{**dict(self.prm), **kw})

    def reference(self, variant: int, **kw):
        return _case_reference(self, variant, tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def _case_problem(c: Case):
    seed = 1000 + 7 * c.n_pt + c.n_ln if c.seed is None else c.seed
    pr = lcpose.synth(c.n_pt, c.n_ln, seed=seed, rot_deg=c.rot_deg, trans=c.trans, noise_px=c.noise_px,
                      outlier_frac=c.outlier_frac, cam=c.cam)
    if c.scale != 1.0:
        pr = scaled(pr, c.scale)
    if c.mirror >= 0:
        pr = mirrored(pr, c.mirror)
    if c.zero_z >= 0:
        pr = zero_depth(pr, c.zero_z)
    return pr


@functools.lru_cache(maxsize=None)
def _case_reference(c: Case, variant: int, kw: tuple):
    """The checker's result (read-only: shared by the tests)."""
    return ref_lcpose.relative_pose(c.problem(), c.params(variant, **dict(kw)))


def parity_figures(out, ref) -> dict:
    """Every figure test_gpu_lcpose._assert_parity bounds, divided by its bar (<= 1 passes), for two
    results with equal flags: what the admission checks of test_lcpose_oracle.py measure between the
    checker and its own run on a reordered candidate."""
    import parity
    fig = {k: parity.elem_violation(out[k], ref[k]) for k in ("x_inc", "pose_inc", "T_inc", "e", "t", "r_deg")}
    fig["H"] = float(np.abs(out["H"] - ref["H"]).max() / np.abs(ref["H"]).max()) / 1e-8
    tol = 1e-8 + 100.0 * float(np.finfo(np.float64).eps) * np.linalg.cond(ref["H"])
    fig["unc"] = float(abs(out["unc"] - ref["unc"]) / abs(ref["unc"]) / tol)
    return fig


def one_pass_figures(out, ref) -> dict:
    """The relative differences of one pass from the identity: H and e as summed there, and T_inc
    after the step divided by cond₂(H), the factor by which the solve may amplify them."""
    T = np.abs(out["T_inc"] - ref["T_inc"]).max() / max(1.0, np.abs(ref["T_inc"]).max())
    return dict(H=float(np.abs(out["H"] - ref["H"]).max() / np.abs(ref["H"]).max()),
                e=float(abs(out["e"] - ref["e"]) / abs(ref["e"])), T_inc=float(T / np.linalg.cond(ref["H"])))


# one pass from the identity (variant GN, max_iters_first = 1): 6-8 features, either side of a wave and
# of the stride in one kind, both kinds across a wave, and the four shapes of the full runs
ONE_PASS_SHAPES = [(7, 0), (0, 6), (3, 3), (63, 0), (64, 0), (65, 0), (0, 63), (0, 64), (0, 65), (255, 0), (256, 0),
                   (257, 0), (0, 257), (63, 65), (40, 12), (300, 100)]
ONE_PASS = dict(max_iters_first=1)
# H and e of one pass, relative: 100 times the largest difference the checker shows against itself on
# reordered features (1.218e-15, measured by test_lcpose_oracle.py over three orders of every candidate)
ONE_PASS_BAR = 1.22e-13

# (case, the conditions mask RobustGN must give, the one GN must give): one accept bit clear at a time.
# bit 0: e < lc_res, 1: unc < lc_unc, 2: inlier share > lc_inl (GN only), 3: t < lc_trs, 4: r_deg < lc_rot
REJECTED = [
    (Case("rotation of 40 degrees", rot_deg=40.0, prm=(("max_iters_first", 20), ("max_iters", 20))), 15, 15),
    (Case("translation of 2 m", trans=2.0, prm=(("max_iters_first", 10),)), 23, 23),
    (Case("lc_res = 0.05", prm=(("lc_res", 0.05),)), 30, 30),
    (Case("lc_unc = 1e-6", prm=(("lc_unc", 1e-6),)), 29, 29),
    (Case("lc_inl = 0.9, a quarter outliers", outlier_frac=0.25, prm=(("lc_inl", 0.9),)), 31, 27),
]

# noise-free: both loops end on |e − err_prev| < ε, below their caps
STAGNATION = Case("noise-free", seed=1, noise_px=0.0, prm=(("max_iters_first", 30), ("max_iters", 10)))
# the identity pose with exact observations: e < ε on the first pass
AT_IDENTITY = Case("exact at the identity", seed=1, rot_deg=0.0, trans=0.0, noise_px=0.0)

# fmax(homog_th, r): a motion of a fraction of a pixel, so that the residuals of the first pass, at the
# identity, are the noise (<= 1 px) on either side of 0.5; and the ordinary scene, whose later passes are
CLAMP_R_SMALL = Case("homog_th = 0.5, small motion", rot_deg=0.02, trans=0.002, prm=(("homog_th", 0.5),))
CLAMP_R = Case("homog_th = 0.5", prm=(("homog_th", 0.5),))
# fmax(homog_th, gz²): the scene at a tenth of its size, depths of 0.2-1.0 m on either side of 0.5 m
CLAMP_Z = Case("homog_th = 0.25, scene times 0.1", scale=0.1, prm=(("homog_th", 0.25),))
CLAMPS = [CLAMP_R_SMALL, CLAMP_R, CLAMP_Z]

FY300 = Case("fy = 300", cam=CAM_FY300)

# the smallest full-rank candidates (cond₂(H) of 1e4-1e6) and rank-deficient ones (cond₂(H) >= 1e17)
# (the seeds: the first of each shape whose checker run agrees with its reordered runs within a tenth of
# every bar, test_lcpose_oracle.py; "7 points, all rejected" ends with no inlier left)
FEW = [Case("7 points", 7, 0, seed=38), Case("7 points, all rejected", 7, 0, seed=11), Case("6 lines", 0, 6, seed=5),
       Case("8 lines", 0, 8, seed=0), Case("3 points, 3 lines", 3, 3, seed=35)]
RANK_DEFICIENT = [Case("2 points", 2, 0), Case("5 points", 5, 0), Case("3 lines", 0, 3)]

BEHIND = Case("a point behind the camera", mirror=3)
ZERO_DEPTH = Case("a point with z = 0", zero_z=3)

FULL_RUN = [FY300, BEHIND] + FEW   # + the clamp cases that test_lcpose_oracle.py admits
ONE_PASS_CASES = [Case(f"{a} points, {b} lines", a, b) for a, b in ONE_PASS_SHAPES] + CLAMPS + [FY300]
# every candidate whose full run is compared at the bars of the full runs
MARGIN_CASES = [c for c, _, _ in REJECTED] + [STAGNATION] + CLAMPS + FULL_RUN
