"""Synthetic loop-closure candidates for plba_lc_relative_pose (Solver.lc_relative_pose).

A candidate pair is what MapHandler::isLoopClosure (src/mapHandler.cpp:4303-4411) hands to
computeRelativePoseRobustGN: the 3-D points and line endpoints of the old keyframe kf0, in its
camera frame, matched to the pixels and the normalised image lines of the new keyframe kf1.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .synth import CAMERA

OUTLIER_MIN_PX = 10.0   # gross outliers are displaced by at least this much
OUTLIER_MAX_PX = 40.0


@dataclass
class LcProblem:
    pt_P: np.ndarray        # [n_pt][3] stereo_pt[i1]->P of kf0
    pt_obs: np.ndarray      # [n_pt][2] stereo_pt[i2]->pl of kf1
    ln_sP: np.ndarray       # [n_ln][3]
    ln_eP: np.ndarray       # [n_ln][3]
    ln_le: np.ndarray       # [n_ln][3] normalised image line (a, b, c), a² + b² = 1
    cam: tuple = (CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"])
    T_true: np.ndarray = field(default_factory=lambda: np.eye(4))   # P_kf1 = T_true · P_kf0
    pt_outlier: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))
    ln_outlier: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))

    @property
    def n_pt(self) -> int:
        return len(self.pt_P)

    @property
    def n_ln(self) -> int:
        return len(self.ln_sP)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _in_front(rng, n, cam, margin=60.0):
    """n points seen inside the image (with a margin) at 2-10 m."""
    fx, fy, cx, cy = cam
    u = rng.uniform(margin, CAMERA["width"] - margin, n)
    v = rng.uniform(margin, CAMERA["height"] - margin, n)
    z = rng.uniform(2.0, 10.0, n)
    return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)


def _project(P, cam):
    fx, fy, cx, cy = cam
    return np.stack([cx + fx * P[:, 0] / P[:, 2], cy + fy * P[:, 1] / P[:, 2]], 1)


def _disc(rng, n, rmax):
    """n offsets with ‖·‖ <= rmax."""
    a = rng.uniform(0, 2 * np.pi, n)
    r = rmax * np.sqrt(rng.uniform(0, 1, n))
    return np.stack([r * np.cos(a), r * np.sin(a)], 1)


def synth(n_pt: int = 40, n_ln: int = 12, seed: int = 0, rot_deg: float = 3.0, trans: float = 0.1,
          noise_px: float = 0.5, outlier_frac: float = 0.0, cam=None) -> LcProblem:
    """A kf0 feature set in front of an EuRoC-like camera, a true relative pose of ``rot_deg`` degrees
    about a random axis and ``trans`` metres, and the kf1 observations with pixel noise bounded by
    ``noise_px``. A fraction ``outlier_frac`` of each kind are gross outliers: points moved by
    10-40 px, lines shifted by 10-40 px along their normal."""
    rng = np.random.default_rng(seed)
    cam = tuple(cam) if cam is not None else (CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"])
    T = np.eye(4)
    T[:3, :3] = _rodrigues(_unit(rng) * np.deg2rad(rot_deg))
    T[:3, 3] = _unit(rng) * trans
    Tinv = np.linalg.inv(T)

    def to_kf0(P1):   # features are drawn in kf1's view, so that they project inside its image
        return P1 @ Tinv[:3, :3].T + Tinv[:3, 3]

    def to_kf1(P0):
        return P0 @ T[:3, :3].T + T[:3, 3]

    # points
    P0 = to_kf0(_in_front(rng, n_pt, cam))
    obs = _project(to_kf1(P0), cam) + _disc(rng, n_pt, noise_px)
    pt_out = np.zeros(n_pt, bool)
    k = int(round(outlier_frac * n_pt))
    if k:
        pt_out[rng.choice(n_pt, k, replace=False)] = True
        a = rng.uniform(0, 2 * np.pi, k)
        r = rng.uniform(OUTLIER_MIN_PX + 2.0 * noise_px, OUTLIER_MAX_PX, k)
        obs[pt_out] += np.stack([r * np.cos(a), r * np.sin(a)], 1)
    # lines: two endpoints 0.3-1.5 m apart, observed as the normalised line through their noisy pixels
    s1 = _in_front(rng, n_ln, cam)
    dirs = rng.normal(size=(n_ln, 3))
    e1 = s1 + dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(0.3, 1.5, (n_ln, 1))
    e1[:, 2] = np.maximum(e1[:, 2], 1.5)
    sP, eP = to_kf0(s1), to_kf0(e1)
    ps = np.concatenate([_project(to_kf1(sP), cam) + _disc(rng, n_ln, noise_px), np.ones((n_ln, 1))], 1)
    pe = np.concatenate([_project(to_kf1(eP), cam) + _disc(rng, n_ln, noise_px), np.ones((n_ln, 1))], 1)
    le = np.cross(ps, pe)
    le = le / np.sqrt(le[:, 0:1] ** 2 + le[:, 1:2] ** 2)
    ln_out = np.zeros(n_ln, bool)
    k = int(round(outlier_frac * n_ln))
    if k:
        ln_out[rng.choice(n_ln, k, replace=False)] = True
        le[ln_out, 2] += rng.choice([-1.0, 1.0], k) * rng.uniform(OUTLIER_MIN_PX + 2.0 * noise_px, OUTLIER_MAX_PX, k)
    return LcProblem(pt_P=np.ascontiguousarray(P0), pt_obs=np.ascontiguousarray(obs), ln_sP=np.ascontiguousarray(sP),
                     ln_eP=np.ascontiguousarray(eP), ln_le=np.ascontiguousarray(le), cam=cam, T_true=T,
                     pt_outlier=pt_out, ln_outlier=ln_out)
