"""Synthetic frame pairs for plba_track_pose (Solver.track_pose) and the CPU restatement's call.

A problem is what StereoFrameHandler::matchF2FPoints / matchF2FLines (src2/stereoFrameHandler.cpp
:131-180) leave for optimizePose: the 3-D points, line endpoints and Plücker lines of the previous
frame, in its camera, matched to the pixels, the segment endpoints and the normalised image lines of
the current frame, plus the previous frame's own image segments (for the overlap weight).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi
from .lcpose import OUTLIER_MAX_PX, OUTLIER_MIN_PX, _disc, _in_front, _project, _rodrigues, _unit
from .synth import CAMERA


def _prev_default():
    """A previous frame whose estimate isGoodSolution accepts: DT = I, DT_cov = 1e-4·I, err_norm = 0.5."""
    return np.concatenate([np.eye(4).ravel(), (1e-4 * np.eye(6)).ravel(), [0.5]])


@dataclass
class TrackProblem:
    pt_P: np.ndarray        # [n_pt][3] P of the previous frame
    pt_obs: np.ndarray      # [n_pt][2] pl of the current frame
    pt_sigma2: np.ndarray   # [n_pt]
    ln_sP: np.ndarray       # [n_ln][3]
    ln_eP: np.ndarray       # [n_ln][3]
    ln_NDc: np.ndarray      # [n_ln][6] Plücker line (moment N, direction D) in the previous camera
    ln_le: np.ndarray       # [n_ln][3] normalised image line of the current frame
    ln_obs: np.ndarray      # [n_ln][4] its endpoints (spl_obs, epl_obs)
    ln_seg: np.ndarray      # [n_ln][4] the previous frame's own segment (spl, epl)
    ln_sigma2: np.ndarray   # [n_ln]
    prev: np.ndarray = field(default_factory=_prev_default)   # [53] DT, DT_cov, err_norm of the previous frame
    cam: tuple = (CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"])
    T_true: np.ndarray = field(default_factory=lambda: np.eye(4))   # P_curr = T_true · P_prev
    pt_outlier: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))
    ln_outlier: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))

    @property
    def n_pt(self) -> int:
        return len(self.pt_P)

    @property
    def n_ln(self) -> int:
        return len(self.ln_sP)


def empty(cam=None) -> TrackProblem:
    z = np.zeros
    cam = tuple(cam) if cam is not None else (CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"])
    return TrackProblem(z((0, 3)), z((0, 2)), z(0), z((0, 3)), z((0, 3)), z((0, 6)), z((0, 3)), z((0, 4)), z((0, 4)), z(0),
                        cam=cam)


def synth(n_pt: int = 300, n_ln: int = 100, seed: int = 0, rot_deg: float = 1.0, trans: float = 0.05,
          noise_px: float = 0.5, outlier_frac: float = 0.0, cam=None) -> TrackProblem:
    """A feature set in front of an EuRoC-like camera, a true frame-to-frame motion of ``rot_deg``
    degrees about a random axis and ``trans`` metres, and the current frame's observations with pixel
    noise bounded by ``noise_px``. A fraction ``outlier_frac`` of each kind are gross outliers: points
    moved by 10-40 px, lines (both observed endpoints, hence the image line) shifted by 10-40 px along
    their normal. sigma2 takes the values of three pyramid levels."""
    rng = np.random.default_rng(seed)
    cam = tuple(cam) if cam is not None else (CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"])
    T = np.eye(4)
    T[:3, :3] = _rodrigues(_unit(rng) * np.deg2rad(rot_deg))
    T[:3, 3] = _unit(rng) * trans
    Tinv = np.linalg.inv(T)

    def to_prev(P1):   # features are drawn in the current view, so that they project inside its image
        return P1 @ Tinv[:3, :3].T + Tinv[:3, 3]

    def to_curr(P0):
        return P0 @ T[:3, :3].T + T[:3, 3]

    levels = np.array([1.0, 1.44, 2.0736])
    # points
    P0 = to_prev(_in_front(rng, n_pt, cam))
    obs = _project(to_curr(P0), cam) + _disc(rng, n_pt, noise_px)
    pt_out = np.zeros(n_pt, bool)
    k = int(round(outlier_frac * n_pt))
    if k:
        pt_out[rng.choice(n_pt, k, replace=False)] = True
        a = rng.uniform(0, 2 * np.pi, k)
        r = rng.uniform(OUTLIER_MIN_PX + 2.0 * noise_px, OUTLIER_MAX_PX, k)
        obs[pt_out] += np.stack([r * np.cos(a), r * np.sin(a)], 1)
    # lines: two endpoints 0.3-1.5 m apart
    s1 = _in_front(rng, n_ln, cam)
    dirs = rng.normal(size=(n_ln, 3))
    e1 = s1 + dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(0.3, 1.5, (n_ln, 1))
    e1[:, 2] = np.maximum(e1[:, 2], 1.5)
    sP, eP = to_prev(s1), to_prev(e1)
    ps = _project(to_curr(sP), cam) + _disc(rng, n_ln, noise_px)
    pe = _project(to_curr(eP), cam) + _disc(rng, n_ln, noise_px)
    ln_out = np.zeros(n_ln, bool)
    k = int(round(outlier_frac * n_ln))
    if k:
        ln_out[rng.choice(n_ln, k, replace=False)] = True
        d = pe[ln_out] - ps[ln_out]
        nrm = np.stack([-d[:, 1], d[:, 0]], 1) / np.linalg.norm(d, axis=1, keepdims=True)
        sh = (rng.choice([-1.0, 1.0], k) * rng.uniform(OUTLIER_MIN_PX + 2.0 * noise_px, OUTLIER_MAX_PX, k))[:, None] * nrm
        ps[ln_out] += sh
        pe[ln_out] += sh
    one = np.ones((n_ln, 1))
    le = np.cross(np.concatenate([ps, one], 1), np.concatenate([pe, one], 1)).reshape(n_ln, 3)
    le = le / np.sqrt(le[:, 0:1] ** 2 + le[:, 1:2] ** 2) if n_ln else le
    ND = np.concatenate([np.cross(sP, eP).reshape(n_ln, 3), eP - sP], 1)
    seg = np.concatenate([_project(sP, cam), _project(eP, cam)], 1)
    c = np.ascontiguousarray
    return TrackProblem(pt_P=c(P0), pt_obs=c(obs), pt_sigma2=c(levels[rng.integers(0, 3, n_pt)]),
                        ln_sP=c(sP), ln_eP=c(eP), ln_NDc=c(ND), ln_le=c(le), ln_obs=c(np.concatenate([ps, pe], 1)),
                        ln_seg=c(seg), ln_sigma2=c(levels[rng.integers(0, 3, n_ln)]), cam=cam, T_true=T,
                        pt_outlier=pt_out, ln_outlier=ln_out)


def track_pose_cpu(problems, params=None) -> list:
    """plslam_track_pose_cpu (host/track_pose.cpp): the call's semantics restated on the CPU,
    single-threaded, H / g / e summed in match order. The same dicts as Solver.track_pose."""
    from .slam_map import load_host
    H = load_host()
    bp = C.POINTER(C.c_uint8)
    if params is None:
        params = capi.track_params()
    bv = capi.TrackBatchView(list(problems))
    n = bv.struct.n
    out = (capi.PlbaTrackOut * max(n, 1))()
    pin = np.zeros(max(int(bv.pt_off[-1]), 1), np.uint8)
    lin = np.zeros(max(int(bv.ln_off[-1]), 1), np.uint8)
    rc = H.plslam_track_pose_cpu(None, C.byref(bv.struct), C.byref(params), out, pin.ctypes.data_as(bp),
                                 lin.ctypes.data_as(bp))
    if rc != 0:
        raise RuntimeError(f"plslam_track_pose_cpu failed with {rc}")
    return [capi.track_out_to_dict(out[i], pin[bv.pt_off[i]:bv.pt_off[i + 1]], lin[bv.ln_off[i]:bv.ln_off[i + 1]])
            for i in range(n)]
