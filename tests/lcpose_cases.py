"""TEST INFRASTRUCTURE: the loop-closure relative-pose candidates shared by tests/test_gpu_lcpose.py
(device against the checker) and tests/test_lcpose_oracle.py (the generator's margins of exactly
these candidates), and the checker results computed once for both."""
from __future__ import annotations

import functools

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
