"""Synthetic frame pairs for plba_track_frames (Solver.track_frames), the host gather of the two-call
path and the CPU restatement's call.

A pair is what plba_stereo_associate leaves for two consecutive frames: descriptors, 3-D points, line
endpoints, Plücker lines, image segments and sigma2 of the previous frame's features, descriptors,
pixels, segments and normalised image lines of the current frame's. StereoFrameHandler::f2fTracking
(src2/stereoFrameHandler.cpp:106-180) matches the descriptors and pushes the matched previous rows, in
increasing row order, with the current row's observation; optimizePose (:307-405) takes those.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi
from .lcpose import _in_front, _project
from .synth import CAMERA
from .trackpose import TrackProblem, _prev_default


@dataclass
class FramePair:
    prev_pdesc: np.ndarray       # [n1p][desc_bytes] uint8
    prev_pt_P: np.ndarray        # [n1p][3]
    prev_pt_sigma2: np.ndarray   # [n1p]
    prev_ldesc: np.ndarray       # [n1l][desc_bytes]
    prev_ln_sP: np.ndarray       # [n1l][3]
    prev_ln_eP: np.ndarray       # [n1l][3]
    prev_ln_NDc: np.ndarray      # [n1l][6]
    prev_ln_seg: np.ndarray      # [n1l][4] spl, epl
    prev_ln_sigma2: np.ndarray   # [n1l]
    cur_pdesc: np.ndarray        # [n2p][desc_bytes]
    cur_pt_pl: np.ndarray        # [n2p][2]
    cur_ldesc: np.ndarray        # [n2l][desc_bytes]
    cur_ln_seg: np.ndarray       # [n2l][4] spl, epl
    cur_ln_le: np.ndarray        # [n2l][3]
    prev: np.ndarray = field(default_factory=_prev_default)   # [53] DT, DT_cov, err_norm of the previous frame
    cam: tuple = (CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"])
    true_pt: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int64))   # planted (i1, i2), in i1 order
    true_ln: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int64))


def flip(rng, row: np.ndarray, k: int) -> np.ndarray:
    """``row`` with k of its bits flipped."""
    bits = np.unpackbits(row)
    bits[rng.choice(len(bits), k, replace=False)] ^= 1
    return np.packbits(bits)


def _place(n_all: int, n: int, rows, rng):
    if rows is None:
        return np.sort(rng.permutation(n_all)[:n])
    rows = np.asarray(rows, np.int64)
    assert len(rows) == n and (np.diff(rows) > 0).all() and (n == 0 or rows[-1] < n_all)
    return rows


def from_problem(pr: TrackProblem, seed: int = 0, extra=(0, 0, 0, 0), pt_rows=None, ln_rows=None, max_flips: int = 4,
                 desc_bytes: int = 32) -> FramePair:
    """The frame pair whose matching gives back the pose problem ``pr``: match k of a kind sits in previous
    row pt_rows[k] / ln_rows[k] (increasing; None: drawn) and in a drawn current row, its current descriptor
    is the previous one with at most ``max_flips`` bits flipped. ``extra`` = (previous points, current points,
    previous lines, current lines) rows with random descriptors and features lie in between: random rows of
    256 bits sit about 128 bits apart, which no ratio test below 1 accepts."""
    rng = np.random.default_rng(90001 + seed)
    cam = tuple(pr.cam)

    def kind(n, x1, x2, rows):
        n1, n2 = n + x1, n + x2
        s1, s2 = _place(n1, n, rows, rng), rng.permutation(n2)[:n]
        d1 = rng.integers(0, 256, (n1, desc_bytes), dtype=np.uint8)
        d2 = rng.integers(0, 256, (n2, desc_bytes), dtype=np.uint8)
        for a, j in zip(s1, s2):
            d2[j] = flip(rng, d1[a], int(rng.integers(0, max_flips + 1)))
        return n1, n2, s1, s2, d1, d2

    n1, n2, s1, s2, pd1, pd2 = kind(pr.n_pt, extra[0], extra[1], pt_rows)
    P = _in_front(rng, n1, cam)
    s2p = np.ones(n1)
    pl = rng.uniform(20.0, 400.0, (n2, 2))
    P[s1], s2p[s1], pl[s2] = pr.pt_P, pr.pt_sigma2, pr.pt_obs

    m1, m2, t1, t2, ld1, ld2 = kind(pr.n_ln, extra[2], extra[3], ln_rows)
    sP, eP = _in_front(rng, m1, cam), _in_front(rng, m1, cam)
    s2l = np.ones(m1)
    cseg = rng.uniform(20.0, 400.0, (m2, 4))
    sP[t1], eP[t1], s2l[t1] = pr.ln_sP, pr.ln_eP, pr.ln_sigma2
    ND = np.concatenate([np.cross(sP, eP).reshape(m1, 3), eP - sP], 1)
    seg = np.concatenate([_project(sP, cam), _project(eP, cam)], 1).reshape(m1, 4)
    ND[t1], seg[t1], cseg[t2] = pr.ln_NDc, pr.ln_seg, pr.ln_obs
    one = np.ones((m2, 1))
    le = np.cross(np.concatenate([cseg[:, 0:2], one], 1), np.concatenate([cseg[:, 2:4], one], 1)).reshape(m2, 3)
    le = le / np.sqrt(le[:, 0:1] ** 2 + le[:, 1:2] ** 2) if m2 else le
    le[t2] = pr.ln_le
    c = np.ascontiguousarray
    return FramePair(prev_pdesc=pd1, prev_pt_P=c(P), prev_pt_sigma2=c(s2p), prev_ldesc=ld1, prev_ln_sP=c(sP), prev_ln_eP=c(eP),
                     prev_ln_NDc=c(ND), prev_ln_seg=c(seg), prev_ln_sigma2=c(s2l), cur_pdesc=pd2, cur_pt_pl=c(pl),
                     cur_ldesc=ld2, cur_ln_seg=c(cseg), cur_ln_le=c(le), prev=np.asarray(pr.prev, np.float64).copy(), cam=cam,
                     true_pt=np.stack([s1, s2], 1).astype(np.int64).reshape(-1, 2),
                     true_ln=np.stack([t1, t2], 1).astype(np.int64).reshape(-1, 2))


def gather(pair: FramePair, pt_m12, ln_m12) -> TrackProblem:
    """The loops around matches_12 (:144-152, :167-179) on the host: the pose problem of the matched
    previous rows in increasing i1, each with the observation of its current row. This is the middle of the
    two-call path (plba_desc_match, this, plba_track_pose)."""
    pt_m12, ln_m12 = np.asarray(pt_m12, np.int64), np.asarray(ln_m12, np.int64)
    i1, j1 = np.flatnonzero(pt_m12 >= 0), np.flatnonzero(ln_m12 >= 0)
    i2, j2 = pt_m12[i1], ln_m12[j1]
    f, c = lambda a, w: np.asarray(a, np.float64).reshape(-1, w), np.ascontiguousarray
    return TrackProblem(pt_P=c(f(pair.prev_pt_P, 3)[i1]), pt_obs=c(f(pair.cur_pt_pl, 2)[i2]),
                        pt_sigma2=c(f(pair.prev_pt_sigma2, 1)[i1, 0]), ln_sP=c(f(pair.prev_ln_sP, 3)[j1]),
                        ln_eP=c(f(pair.prev_ln_eP, 3)[j1]), ln_NDc=c(f(pair.prev_ln_NDc, 6)[j1]), ln_le=c(f(pair.cur_ln_le, 3)[j2]),
                        ln_obs=c(f(pair.cur_ln_seg, 4)[j2]), ln_seg=c(f(pair.prev_ln_seg, 4)[j1]),
                        ln_sigma2=c(f(pair.prev_ln_sigma2, 1)[j1, 0]), prev=np.asarray(pair.prev, np.float64), cam=tuple(pair.cam))


def cur_from_prev(m12, n2: int) -> np.ndarray:
    """For each current row the previous row whose idx it inherits (:151, :178): the last writer of the loop
    in increasing i1, or -1."""
    out = np.full(n2, -1, np.int32)
    for i1, i2 in enumerate(np.asarray(m12, np.int64)):
        if i2 >= 0:
            out[i2] = i1
    return out


def track_frames_cpu(pairs, params=None) -> list:
    """plslam_track_frames_cpu (host/track_frames.cpp): the call's semantics restated on the CPU,
    single-threaded. The same dicts as Solver.track_frames."""
    from .slam_map import load_host
    H = load_host()
    if params is None:
        params = capi.frames_params()
    bv = capi.FramesBatchView(pairs, params.desc_bytes)
    rc = H.plslam_track_frames_cpu(None, C.byref(bv.struct), C.byref(params), C.byref(bv.out_struct))
    if rc != 0:
        raise RuntimeError(f"plslam_track_frames_cpu failed with {rc}")
    return bv.results()
