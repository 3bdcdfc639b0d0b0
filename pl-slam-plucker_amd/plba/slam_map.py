"""Map-level view of an LBA window: the KeyFrame / MapPoint / MapLine state that
``MapHandler::localBundleAdjustmentForPlukerWithG2O`` reads and mutates
(include/keyFrame.h:50-71, include/mapFeatures.h:39-107, include/mapHandler.h:141-151),
and the ctypes binding of the C++ host mirror (include/plslam_host.h, libplslam_host.so).

``make_map`` turns a synthetic window (synth.Graph) into such a map: free keyframes are
``local``, KF 0 is local (and therefore fixed by id, src/mapHandler.cpp:5943-5945), the other
fixed keyframes are non-local observers that the gather step pulls in as fixed
(:5888-5919); non-local landmarks and keyframes outside the window are added so the gather
has something to skip.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Callable, Dict, List, Optional

import numpy as np

from . import capi
from . import geometry as geo
from .lib import PKG_DIR, PLBA_ERRORS, PlbaError
from .synth import Graph

HOST_LIB_PATH = os.path.join(PKG_DIR, "libplslam_host.so")
DESC_BYTES = 32


@dataclasses.dataclass
class KF:
    kf_idx: int
    T_kf_w: np.ndarray            # (4,4) camera -> world
    local: bool
    pt_idx: List[int]
    ls_idx: List[int]


@dataclasses.dataclass
class Landmark:
    idx: int
    local: bool
    inlier: bool
    pos: np.ndarray               # point3D (3,) or NDw (6,)
    desc_list: List[np.ndarray]
    obs_list: List[np.ndarray]    # (2,) for points, (4,) for lines
    kf_obs_list: List[int]
    sigma_list: List[float]
    dir_list: Optional[List[np.ndarray]] = None   # points only
    med_desc: Optional[np.ndarray] = None
    med_dir: Optional[np.ndarray] = None


@dataclasses.dataclass
class SlamMap:
    fx: float
    fy: float
    cx: float
    cy: float
    keyframes: List[Optional[KF]]
    points: List[Optional[Landmark]]
    lines: List[Optional[Landmark]]
    map_points_kf_idx: Dict[int, List[int]]
    full_graph: np.ndarray        # (n_kf, n_kf) uint32
    map_lines_kf_idx: Dict[int, List[int]] = dataclasses.field(default_factory=dict)
    max_kf_idx: int = 0           # MapHandler::max_kf_idx (the newest KF)

    def copy(self) -> "SlamMap":
        import copy
        return copy.deepcopy(self)


def median_descriptor(desc_list) -> int:
    """Index of the descriptor with the least median Hamming distance to the others
    (MapPoint::updateAverageDescDir, src/mapFeatures.cpp:57-86; the n == 1 read past the end
    of dist_idx is clamped to the only entry)."""
    n = len(desc_list)
    D = np.array([[int(np.unpackbits(np.bitwise_xor(a, b)).sum()) for b in desc_list] for a in desc_list])
    best, best_i = 99999, 0
    k = min(int(1 + 0.5 * (n - 1)), n - 1)
    for i in range(n):
        med = int(np.sort(D[i])[k])
        if med < best:
            best, best_i = med, i
    return best_i


def make_map(g: Graph, seed: int = 0, n_extra_kf: int = 2, n_extra_pt: int = 5, sigma2: float = 1.0) -> SlamMap:
    rng = np.random.default_rng(seed)
    kf_ids = [int(i) for i in g.kf_id]
    n_kf = max(kf_ids) + 1 + n_extra_kf
    kfs: List[Optional[KF]] = [None] * n_kf
    for k in range(g.n_kf):
        Twc = np.eye(4)
        Twc[:3, :] = geo.invert_rigid(g.kf_Tcw[k])
        kid = kf_ids[k]
        local = (not g.kf_fixed[k]) or kid == 0
        kfs[kid] = KF(kid, Twc, bool(local), [], [])
    for kid in range(n_kf):   # keyframes outside the window (not observed by local landmarks)
        if kfs[kid] is None:
            T = np.eye(4)
            T[:3, 3] = rng.normal(size=3)
            kfs[kid] = KF(kid, T, False, [], [])

    def new_lm(idx, pos, obs_rows, kf_rows, is_point):
        lm = Landmark(idx=idx, local=True, inlier=True, pos=np.array(pos, np.float64), desc_list=[], obs_list=[],
                      kf_obs_list=[], sigma_list=[], dir_list=[] if is_point else None)
        for o, k in zip(obs_rows, kf_rows):
            lm.desc_list.append(rng.integers(0, 256, DESC_BYTES, dtype=np.uint8))
            lm.obs_list.append(np.array(o, np.float64))
            lm.kf_obs_list.append(int(k))
            lm.sigma_list.append(float(sigma2 if rng.random() > 0.1 else 1.7))
            if is_point:
                d = rng.normal(size=3)
                lm.dir_list.append(d / np.linalg.norm(d))
        return lm

    points: List[Optional[Landmark]] = []
    for p in range(g.n_pt):
        sel = np.nonzero(g.ept_lm == p)[0]
        points.append(new_lm(p, g.pt_xyz[p], g.ept_obs[sel], g.kf_id[g.ept_kf[sel]], True))
    lines: List[Optional[Landmark]] = []
    for l in range(g.n_ln):
        sel = np.nonzero(g.eln_lm == l)[0]
        lines.append(new_lm(l, geo.orth_to_pluker(g.ln_orth[l]), g.eln_obs[sel], g.kf_id[g.eln_kf[sel]], False))
    # non-local landmarks (skipped by the gather) and a hole in the vectors (NULL pointer)
    for j in range(n_extra_pt):
        k1, k2 = rng.integers(0, n_kf, 2)
        lm = new_lm(len(points), rng.normal(size=3) * 3, [rng.uniform(0, 700, 2)] * 2, [k1, k2], True)
        lm.local = False
        points.append(lm)
    points.append(None)
    for lms in (points, lines):   # state after the constructor + addObservation replay
        for lm in lms:
            if lm is None:
                continue
            lm.med_desc = lm.desc_list[median_descriptor(lm.desc_list)]
            if lm.dir_list is not None:
                lm.med_dir = np.sum(lm.dir_list, axis=0) / len(lm.dir_list)
    # keyframe stereo features: every landmark seen, plus an untracked feature (-1)
    for lm in points:
        if lm is not None:
            for k in lm.kf_obs_list:
                kfs[k].pt_idx.append(lm.idx)
    for lm in lines:
        if lm is not None:
            for k in lm.kf_obs_list:
                kfs[k].ls_idx.append(lm.idx)
    for kf in kfs:
        kf.pt_idx.append(-1)
        rng.shuffle(kf.pt_idx)
    # map_points_kf_idx / map_lines_kf_idx: base KF -> its points / lines (the LBA's outlier
    # pass looks lines up in map_points_kf_idx, src/mapHandler.cpp:6239-6251)
    kidx: Dict[int, List[int]] = {k: [] for k in range(n_kf)}
    lidx: Dict[int, List[int]] = {k: [] for k in range(n_kf)}
    for lm in points:
        if lm is not None:
            kidx[lm.kf_obs_list[0]].append(lm.idx)
    for lm in lines:
        lidx[lm.kf_obs_list[0]].append(lm.idx)
    fg = np.zeros((n_kf, n_kf), np.uint32)
    for lm in points + lines:
        if lm is not None:
            for a in lm.kf_obs_list:
                for b in lm.kf_obs_list:
                    if a != b:
                        fg[a, b] += 1
    fg += 3   # so a few decrements never wrap
    return SlamMap(g.fx, g.fy, g.cx, g.cy, kfs, points, lines, kidx, fg, lidx, n_kf - 1)


# ------------------------------------------------------------------------------------ binding
class PlslamLbaStats(C.Structure):
    _fields_ = [("n_free_kf", C.c_int32), ("n_fixed_kf", C.c_int32), ("n_pt", C.c_int32), ("n_ln", C.c_int32),
                ("n_ept", C.c_int32), ("n_eln", C.c_int32), ("bad_line_stage1", C.c_int32),
                ("bad_point_obs", C.c_int32), ("actually_bad_point_obs", C.c_int32),
                ("bad_line_obs", C.c_int32), ("actually_bad_line_obs", C.c_int32),
                ("iters", C.c_int32 * 2), ("chi2", C.c_double * 2),
                ("gather_ms", C.c_double), ("solve_ms", C.c_double), ("bookkeeping_ms", C.c_double),
                ("upload_ms", C.c_double), ("dirty_landmarks", C.c_int32)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["iters"] = list(self.iters)
        d["chi2"] = list(self.chi2)
        return d


SOLVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaGraph), C.POINTER(capi.PlbaResult))
HLM_SOLVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaGraph), C.POINTER(capi.PlbaHlmState),
                           C.POINTER(capi.PlbaHlmParams), C.POINTER(capi.PlbaHlmResult))


PGO_SOLVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaPgoGraph), C.POINTER(capi.PlbaPgoParams),
                           C.POINTER(capi.PlbaPgoResult))


class PlslamPgoStats(C.Structure):
    _fields_ = [("kf_prev_idx", C.c_int32), ("kf_curr_idx", C.c_int32), ("n_vertices", C.c_int32),
                ("n_fixed", C.c_int32), ("n_edges", C.c_int32), ("n_loop_edges", C.c_int32),
                ("iterations", C.c_int32), ("trials", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("solve_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class PlslamFuseStats(C.Structure):
    _fields_ = [("loops", C.c_int32), ("loops_skipped", C.c_int32), ("rows", (C.c_int32 * 4) * 2),
                ("null_skipped", (C.c_int32 * 4) * 2), ("same_landmark", C.c_int32 * 2), ("erased", C.c_int32 * 2),
                ("medoid_lists", C.c_int32), ("pad", C.c_int32), ("medoid_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        d = {f: getattr(self, f) for f in ("loops", "loops_skipped", "medoid_lists", "medoid_ms", "total_ms")}
        d["rows"] = [list(r) for r in self.rows]
        d["null_skipped"] = [list(r) for r in self.null_skipped]
        d["same_landmark"] = list(self.same_landmark)
        d["erased"] = list(self.erased)
        return d


MEDOID_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaMedoidBatch), C.POINTER(C.c_int32))


class PlslamHlmStats(C.Structure):
    _fields_ = [("ret", C.c_int32), ("n_kf_list", C.c_int32), ("n_fixed_kf", C.c_int32), ("n_pt", C.c_int32),
                ("n_ln", C.c_int32), ("n_pt_obs", C.c_int32), ("n_ls_obs", C.c_int32),
                ("linearizations", C.c_int32), ("solves", C.c_int32), ("accepted", C.c_int32),
                ("pt_outliers", C.c_int32), ("ln_outliers", C.c_int32),
                ("err", C.c_double), ("lambda_", C.c_double), ("gather_ms", C.c_double), ("solve_ms", C.c_double),
                ("writeback_ms", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}

LCPOSE_SOLVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaLcposeBatch), C.POINTER(capi.PlbaLcposeParams),
                              C.POINTER(capi.PlbaLcposeOut), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))
LC_IDLE, LC_ACTIVE, LC_READY = 0, 1, 2   # include/mapHandler.h:195-197
MATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaMatchBatch), C.POINTER(C.c_int32), C.POINTER(C.c_int32))


class PlslamMatchParams(C.Structure):
    _fields_ = [("min_ratio_12_p", C.c_float), ("min_ratio_12_l", C.c_float), ("best_lr", C.c_int32),
                ("has_points", C.c_int32), ("has_lines", C.c_int32), ("pad", C.c_int32)]


def match_params(min_ratio_12_p: float = 0.9, min_ratio_12_l: float = 0.9, best_lr: bool = True,
                 has_points: bool = True, has_lines: bool = True) -> PlslamMatchParams:
    """src2/config.cpp:46-47,51,60,68."""
    return PlslamMatchParams(min_ratio_12_p=min_ratio_12_p, min_ratio_12_l=min_ratio_12_l, best_lr=int(best_lr),
                             has_points=int(has_points), has_lines=int(has_lines), pad=0)


STEREO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaStereoBatch), C.POINTER(capi.PlbaStereoParams),
                        C.POINTER(capi.PlbaStereoOut))


class PlslamStereoFrame(C.Structure):
    _fields_ = [("desc_bytes", C.c_int32), ("n_pt_l", C.c_int32), ("n_pt_r", C.c_int32), ("n_ls_l", C.c_int32),
                ("n_ls_r", C.c_int32), ("pad", C.c_int32), ("pt_l", C.POINTER(C.c_float)), ("pt_r", C.POINTER(C.c_float)),
                ("pdesc_l", C.POINTER(C.c_uint8)), ("pdesc_r", C.POINTER(C.c_uint8)), ("ls_l", C.POINTER(C.c_float)),
                ("ls_r", C.POINTER(C.c_float)), ("ldesc_l", C.POINTER(C.c_uint8)), ("ldesc_r", C.POINTER(C.c_uint8))]


class PlslamStereoStats(C.Structure):
    _fields_ = [("n_pt", C.c_int32), ("n_ls", C.c_int32), ("ms", C.c_double)]


GRID_MATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaGridMatchBatch), C.POINTER(C.c_int32),
                            C.POINTER(C.c_int32))


class PlslamKfMatchStats(C.Structure):
    _fields_ = [("grid_matches", C.c_int32 * 2), ("fallback", C.c_int32 * 2), ("matches", C.c_int32 * 2),
                ("created", C.c_int32 * 2), ("extended", C.c_int32 * 2), ("rejected", C.c_int32 * 2),
                ("n_pairs", C.c_int32 * 2), ("pt_cap", C.c_int32), ("ls_cap", C.c_int32),
                ("pt_pairs", C.POINTER(C.c_int32)), ("ls_pairs", C.POINTER(C.c_int32)), ("match_ms", C.c_double)]

    def as_dict(self):
        return {k: list(getattr(self, k)) for k in ("grid_matches", "fallback", "matches", "created", "extended", "rejected")}


KFASSOC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaKfassocBatch), C.POINTER(capi.PlbaKfassocParams),
                         C.POINTER(capi.PlbaKfassocOut))


MAPASSOC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(capi.PlbaMapassocBatch), C.POINTER(capi.PlbaMapassocParams),
                          C.POINTER(capi.PlbaMapassocOut))


def mapassoc_params(**kw) -> capi.PlbaMapassocParams:
    """The reference's defaults (plba_mapassoc_default_params) with ``kw`` over them."""
    return capi.mapassoc_params(None, **kw)


class PlslamMapMatchParams(C.Structure):
    _fields_ = [("fast_matching", C.c_int32), ("ws", C.c_int32), ("min_pt_matches", C.c_int32),
                ("min_ls_matches", C.c_int32), ("best_lr", C.c_int32), ("has_points", C.c_int32),
                ("has_lines", C.c_int32), ("pad", C.c_int32), ("max_kf_epip_p", C.c_double),
                ("max_kf_epip_l", C.c_double), ("line_sim_th", C.c_double), ("min_ratio_12_p", C.c_double),
                ("min_ratio_12_l", C.c_double)]


class PlslamMapMatchStats(C.Structure):
    _fields_ = [("visible", C.c_int32 * 2), ("unmatched", C.c_int32 * 2), ("grid_matches", C.c_int32 * 2),
                ("fallback", C.c_int32 * 2), ("accepted", C.c_int32 * 2), ("rejected", C.c_int32 * 2),
                ("match_ms", C.c_double)]

    def as_dict(self):
        return {f: (list(getattr(self, f)) if f != "match_ms" else self.match_ms) for f, _ in self._fields_}


def mapmatch_params(**kw) -> PlslamMapMatchParams:
    """The reference's defaults (plslam_mapmatch_default_params) with ``kw`` over them."""
    p = PlslamMapMatchParams()
    load_host().plslam_mapmatch_default_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(p._fields_):
            raise TypeError(k)
        setattr(p, k, v)
    return p


class PlslamLcCandidate(C.Structure):
    _fields_ = [("kf_prev_idx", C.c_int32), ("kf_curr_idx", C.c_int32), ("n_pt_0", C.c_int32), ("n_pt_1", C.c_int32),
                ("n_ls_0", C.c_int32), ("n_ls_1", C.c_int32), ("has_points", C.c_int32), ("has_lines", C.c_int32),
                ("n_pt", C.c_int32), ("n_ln", C.c_int32),
                ("pt_P", C.POINTER(C.c_double)), ("pt_obs", C.POINTER(C.c_double)), ("ln_sP", C.POINTER(C.c_double)),
                ("ln_eP", C.POINTER(C.c_double)), ("ln_le", C.POINTER(C.c_double)),
                ("pt_idx", C.POINTER(C.c_int32)), ("ls_idx", C.POINTER(C.c_int32))]


class PlslamLcStats(C.Structure):
    _fields_ = [("is_candidate", C.c_int32), ("ratio_ok", C.c_int32), ("accepted", C.c_int32),
                ("conditions", C.c_int32), ("n_inl_pt", C.c_int32), ("n_inl_ln", C.c_int32),
                ("state_before", C.c_int32), ("state_after", C.c_int32), ("pgo_ran", C.c_int32), ("pad", C.c_int32),
                ("inl_ratio_pt", C.c_double), ("inl_ratio_ls", C.c_double), ("e", C.c_double), ("unc", C.c_double),
                ("t", C.c_double), ("r_deg", C.c_double), ("pose_ms", C.c_double), ("pgo", PlslamPgoStats)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_ if f not in ("pad", "pgo")}
        d["pgo"] = self.pgo.as_dict()
        return d


# ---- place recognition (plslam_bow_call / plslam_set_bow_fn / plslam_lc_search_params)
BOW_SET_VOCAB, BOW_INSERT, BOW_REMOVE, BOW_GET = 0, 1, 2, 3


class PlslamBowCall(C.Structure):
    _fields_ = [("op", C.c_int32), ("slot", C.c_int32), ("kf_id", C.c_int32), ("n_desc", C.c_int32), ("cap", C.c_int32),
                ("n", C.c_int32), ("vocab", C.POINTER(capi.PlbaBowVocab)), ("desc", C.POINTER(C.c_uint8)),
                ("scores", C.POINTER(C.c_double)), ("ids", C.POINTER(C.c_int32)), ("word_ids", C.POINTER(C.c_int32)),
                ("values", C.POINTER(C.c_double))]


BOW_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(PlslamBowCall))


class PlslamLcSearchParams(C.Structure):
    _fields_ = [("lc_kf_dist", C.c_int32), ("lc_kf_max_dist", C.c_int32), ("lc_nkf_closest", C.c_int32),
                ("min_lm_cov_graph", C.c_int32), ("min_kf_local_map", C.c_int32), ("pad", C.c_int32)]


def lc_search_params(lc_kf_dist: int = 50, lc_kf_max_dist: int = 50, lc_nkf_closest: int = 4,
                     min_lm_cov_graph: int = 75, min_kf_local_map: int = 3) -> PlslamLcSearchParams:
    """src/slamConfig.cpp:61-62,80-82."""
    return PlslamLcSearchParams(lc_kf_dist, lc_kf_max_dist, lc_nkf_closest, min_lm_cov_graph, min_kf_local_map, 0)


class BowCpu:
    """The single-threaded CPU restatement of plba_bow_* (plslam_bow_cpu) with a database of its own:
    the hook of the CPU tests and the baseline of tools/bow_bench.py. Not a product path."""

    def __init__(self):
        self.L = load_host()
        self.db = C.c_void_p(self.L.plslam_bow_cpu_new())

    def close(self):
        if self.db:
            self.L.plslam_bow_cpu_free(self.db)
            self.db = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, c: PlslamBowCall):
        rc = self.L.plslam_bow_cpu(self.db, C.byref(c))
        if rc != 0:
            raise PlbaError(f"plslam_bow_cpu op {c.op} failed: {PLBA_ERRORS.get(rc, rc)}")

    def set_vocab(self, slot: int, voc):
        vv = voc if isinstance(voc, capi.BowVocabView) else capi.BowVocabView(voc)
        self._call(PlslamBowCall(op=BOW_SET_VOCAB, slot=slot, vocab=C.pointer(vv.struct)))
        self._live = getattr(self, "_live", {})
        self._live[slot] = 0

    def insert(self, slot: int, kf_id: int, desc):
        desc = np.ascontiguousarray(desc, dtype=np.uint8)
        n_desc = int(desc.shape[0]) if desc.ndim == 2 else 0
        cap = self._live[slot] + 1
        scores, ids = np.zeros(cap), np.zeros(cap, np.int32)
        c = PlslamBowCall(op=BOW_INSERT, slot=slot, kf_id=kf_id, n_desc=n_desc, cap=cap,
                          desc=desc.ctypes.data_as(C.POINTER(C.c_uint8)) if n_desc else None,
                          scores=scores.ctypes.data_as(C.POINTER(C.c_double)), ids=ids.ctypes.data_as(C.POINTER(C.c_int32)))
        self._call(c)
        assert c.n == cap
        self._live[slot] = cap
        return ids, scores

    def remove(self, slot: int, kf_id: int):
        self._call(PlslamBowCall(op=BOW_REMOVE, slot=slot, kf_id=kf_id))
        self._live[slot] -= 1

    def get(self, slot: int, kf_id: int):
        c = PlslamBowCall(op=BOW_GET, slot=slot, kf_id=kf_id)
        self._call(c)
        w, v = np.zeros(max(c.n, 1), np.int32), np.zeros(max(c.n, 1))
        c.cap, c.word_ids, c.values = c.n, w.ctypes.data_as(C.POINTER(C.c_int32)), v.ctypes.data_as(C.POINTER(C.c_double))
        self._call(c)
        return w[:c.n].copy(), v[:c.n].copy()


@dataclasses.dataclass
class SlamParams:
    """SlamConfig values of the local-mapping step (src/slamConfig.cpp:48,61-62 defaults)."""
    min_lm_obs: int = 5
    min_lm_cov_graph: int = 75
    min_kf_local_map: int = 3


# every function load_host() binds, with its argtypes; the return type is an int but for HOST_RESTYPES
_P, _vp, _i32, _f64 = C.POINTER, C.c_void_p, C.c_int32, C.c_double
_dp, _ip, _bp, _fp, _u32p = _P(C.c_double), _P(C.c_int32), _P(C.c_uint8), _P(C.c_float), _P(C.c_uint32)


def _batch3(batch, params, out):   # a *_cpu restatement: user, batch, params, out
    return [_vp, _P(batch), _P(params), _P(out)]


HOST_ARGTYPES = {
    "plslam_map_create": [_P(_vp), _f64, _f64, _f64, _f64, _P(capi.PlbaOpts)],
    "plslam_map_destroy": [_vp],
    "plslam_map_last_error": [_vp],
    "plslam_set_solver": [_vp, SOLVE_FN, _vp],
    "plslam_add_keyframe": [_vp, _i32, _dp, _i32, _ip, _i32, _ip],
    "plslam_add_point": [_vp, _i32, _dp, _bp, _i32, _i32, _dp, _dp, _f64],
    "plslam_point_add_observation": [_vp, _i32, _bp, _i32, _dp, _dp, _f64],
    "plslam_add_line": [_vp, _i32, _dp, _bp, _i32, _i32, _dp, _f64],
    "plslam_line_add_observation": [_vp, _i32, _bp, _i32, _dp, _f64],
    "plslam_set_local": [_vp, _i32, _i32, _i32],
    "plslam_set_full_graph": [_vp, _i32, _u32p],
    "plslam_get_full_graph": [_vp, _i32, _u32p],
    "plslam_kf_idx_set": [_vp, _i32, _ip, _i32],
    "plslam_kf_idx_get": [_vp, _i32, _ip, _i32, _ip],
    "plslam_local_ba_plucker_g2o": [_vp, _P(PlslamLbaStats)],
    "plslam_get_keyframe": [_vp, _i32, _dp, _ip, _ip, _i32, _ip, _i32],
    "plslam_get_point": [_vp, _i32, _dp, _ip, _ip, _ip, _ip, _dp, _dp, _dp, _i32, _bp, _dp],
    "plslam_get_line": [_vp, _i32, _dp, _ip, _ip, _ip, _ip, _dp, _dp, _i32, _bp],
    "plslam_pluker_to_orth": [_dp, _dp],
    "plslam_orth_to_pluker": [_dp, _dp],
    "plslam_set_inlier": [_vp, _i32, _i32, _i32],
    "plslam_set_params": [_vp, _i32, _i32, _i32],
    "plslam_set_max_kf_idx": [_vp, _i32],
    "plslam_kf_lines_idx_set": [_vp, _i32, _ip, _i32],
    "plslam_kf_lines_idx_get": [_vp, _i32, _ip, _i32, _ip],
    "plslam_form_local_map": [_vp, _i32],
    "plslam_remove_bad_landmarks_pluker": [_vp, _ip, _ip],
    "plslam_local_mapping_step": [_vp, _i32, _P(PlslamLbaStats), _ip, _ip],
    "plslam_exists": [_vp, _i32, _i32, _ip],
    "plslam_set_keyframe_x": [_vp, _i32, _dp],
    "plslam_get_keyframe_x": [_vp, _i32, _dp],
    "plslam_set_hlm_solver": [_vp, HLM_SOLVE_FN, _vp],
    "plslam_set_hlm_params": [_vp, _P(capi.PlbaHlmParams), _i32],
    "plslam_local_ba_plucker": [_vp, _P(PlslamHlmStats)],
    "plslam_local_ba": [_vp, _P(PlslamHlmStats)],
    "plslam_set_loop_closure": [_vp, _i32, _ip, _i32, _ip, _i32, _dp],
    "plslam_get_lc_idx_list": [_vp, _ip, _i32, _ip],
    "plslam_set_pgo_params": [_vp, _i32, _i32],
    "plslam_set_pgo_solver": [_vp, PGO_SOLVE_FN, _vp],
    "plslam_loop_closure_optimization": [_vp, _i32, _P(PlslamPgoStats)],
    "plslam_set_line_geometry": [_vp, _i32, _dp, _dp],
    "plslam_get_line_geometry": [_vp, _i32, _dp, _dp],
    "plslam_set_incremental": [_vp, _i32],
    "plslam_mark_landmark_changed": [_vp, _i32, _i32],
    "plslam_check_incremental_gather": [_vp, _ip],
    "plslam_set_lcpose_solver": [_vp, LCPOSE_SOLVE_FN, _vp],
    "plslam_set_lcpose_params": [_vp, _P(capi.PlbaLcposeParams)],
    "plslam_loop_closure_step": [_vp, _P(PlslamLcCandidate), _f64, _P(PlslamLcStats)],
    "plslam_get_lc_state": [_vp, _ip],
    "plslam_get_lc_pose_list": [_vp, _dp, _i32, _ip],
    "plslam_get_lc_feature_idxs": [_vp, _i32, _i32, _ip, _i32, _ip],
    "plslam_set_lc_feature_idxs": [_vp, _i32, _i32, _ip, _i32],
    "plslam_set_keyframe_features": [_vp, _i32, _i32, _bp, _dp, _dp, _bp, _dp, _dp, _dp],
    "plslam_set_match_fn": [_vp, MATCH_FN, _vp],
    "plslam_loop_closure_step_kf": [_vp, _i32, _i32, _P(PlslamMatchParams), _f64, _P(PlslamLcStats)],
    "plslam_verify_loop_candidates": [_vp, _i32, _i32, _ip, _P(PlslamMatchParams), _f64, _ip, _dp, _ip],
    "plslam_desc_match_cpu": [_vp, _P(capi.PlbaMatchBatch), _ip, _ip],
    "plslam_line_cells": [_f64, _f64, _f64, _f64, _ip, _i32, _ip],
    "plslam_grid_match_cpu": [_vp, _P(capi.PlbaGridMatchBatch), _ip, _ip],
    "plslam_set_keyframe_stereo": [_vp, _i32, _P(PlslamStereoFrame), _P(capi.PlbaStereoParams), _ip, _ip,
                                   _P(PlslamStereoStats)],
    "plslam_set_stereo_fn": [_vp, STEREO_FN, _vp],
    "plslam_stereo_cpu": _batch3(capi.PlbaStereoBatch, capi.PlbaStereoParams, capi.PlbaStereoOut),
    "plslam_kf_assoc_cpu": _batch3(capi.PlbaKfassocBatch, capi.PlbaKfassocParams, capi.PlbaKfassocOut),
    "plslam_track_pose_cpu": _batch3(capi.PlbaTrackBatch, capi.PlbaTrackParams, capi.PlbaTrackOut) + [_bp, _bp],
    "plslam_track_frames_cpu": _batch3(capi.PlbaFramesBatch, capi.PlbaFramesParams, capi.PlbaFramesOut),
    "plslam_match_kf_to_kf": [_vp, _i32, _i32, _dp, _P(capi.PlbaKfassocParams), _P(PlslamKfMatchStats)],
    "plslam_look_for_common_matches": [_vp, _i32, _i32, _P(capi.PlbaKfassocParams), _P(PlslamMapMatchParams),
                                       _P(PlslamKfMatchStats), _P(PlslamMapMatchStats)],
    "plslam_set_keyframe_line_pluker": [_vp, _i32, _dp],
    "plslam_set_kfassoc_fn": [_vp, KFASSOC_FN, _vp],
    "plslam_set_keyframe_line_endpoints": [_vp, _i32, _dp, _dp],
    "plslam_set_camera": [_vp, _f64, _f64, _f64, _f64, _i32, _i32],
    "plslam_set_grid_match_fn": [_vp, GRID_MATCH_FN, _vp],
    "plslam_mapmatch_default_params": [_P(PlslamMapMatchParams)],
    "plslam_match_map_to_kf": [_vp, _i32, _dp, _P(PlslamMapMatchParams), _P(PlslamMapMatchStats)],
    "plslam_local_mapping_step_kf": [_vp, _i32, _P(PlslamMapMatchParams), _P(PlslamMapMatchStats), _P(PlslamLbaStats),
                                     _ip, _ip],
    "plslam_match_map_to_kf_assoc": [_vp, _i32, _dp, _P(capi.PlbaMapassocParams), _P(PlslamMapMatchStats)],
    "plslam_local_mapping_step_kf_assoc": [_vp, _i32, _P(capi.PlbaMapassocParams), _P(PlslamMapMatchStats),
                                           _P(PlslamLbaStats), _ip, _ip],
    "plslam_set_mapassoc_fn": [_vp, MAPASSOC_FN, _vp],
    "plslam_map_assoc_cpu": _batch3(capi.PlbaMapassocBatch, capi.PlbaMapassocParams, capi.PlbaMapassocOut),
    "plslam_set_bow_fn": [_vp, _vp, _vp],    # the hook as an address: plslam_bow_cpu itself can be passed
    "plslam_bow_cpu_new": [],
    "plslam_bow_cpu_free": [_vp],
    "plslam_bow_cpu": [_vp, _P(PlslamBowCall)],
    "plslam_set_vocabulary": [_vp, _i32, _P(capi.PlbaBowVocab)],
    "plslam_remove_keyframe": [_vp, _i32],
    "plslam_insert_kf_bow": [_vp, _i32, _i32, _i32],
    "plslam_get_conf_matrix_row": [_vp, _i32, _fp, _i32, _ip],
    "plslam_set_conf_matrix": [_vp, _i32, _fp],
    "plslam_look_for_loop_candidates": [_vp, _i32, _P(PlslamLcSearchParams), _ip, _ip],
    "plslam_loop_closure_kf": [_vp, _i32, _P(PlslamLcSearchParams), _P(PlslamMatchParams), _f64, _P(PlslamLcStats)],
    "plslam_lc_search_default_params": [_P(PlslamLcSearchParams)],
    "plslam_fuse_landmarks": [_vp, _P(PlslamFuseStats)],
    "plslam_set_medoid_fn": [_vp, MEDOID_FN, _vp],
    "plslam_desc_medoid_cpu": [_vp, _P(capi.PlbaMedoidBatch), _ip],
    "plslam_loop_closure_optimization_fuse": [_vp, _i32, _P(PlslamPgoStats), _P(PlslamFuseStats)],
}
HOST_RESTYPES = {"plslam_map_last_error": C.c_char_p, "plslam_bow_cpu_new": _vp, "plslam_pluker_to_orth": None,
                 "plslam_orth_to_pluker": None, "plslam_mapmatch_default_params": None, "plslam_bow_cpu_free": None,
                 "plslam_lc_search_default_params": None}
HOST_EXPORTED = list(HOST_ARGTYPES)

# The hooks of a MapHandler: the setter, the hook's type, which of its arguments (after ``user``) the Python
# callable gets as .contents, and the C function that "cpu" stands for where the library has one.
HOOKS = {
    "solver": ("plslam_set_solver", SOLVE_FN, (0, 1), None),
    "hlm": ("plslam_set_hlm_solver", HLM_SOLVE_FN, (0, 1, 2, 3), None),
    "pgo": ("plslam_set_pgo_solver", PGO_SOLVE_FN, (0, 1, 2), None),
    "lcpose": ("plslam_set_lcpose_solver", LCPOSE_SOLVE_FN, (0, 1), None),
    "match": ("plslam_set_match_fn", MATCH_FN, (0,), None),
    "medoid": ("plslam_set_medoid_fn", MEDOID_FN, (0,), "plslam_desc_medoid_cpu"),
    "stereo": ("plslam_set_stereo_fn", STEREO_FN, (0, 1, 2), "plslam_stereo_cpu"),
    "kfassoc": ("plslam_set_kfassoc_fn", KFASSOC_FN, (0, 1, 2), "plslam_kf_assoc_cpu"),
    "grid": ("plslam_set_grid_match_fn", GRID_MATCH_FN, (0,), "plslam_grid_match_cpu"),
    "mapassoc": ("plslam_set_mapassoc_fn", MAPASSOC_FN, (0, 1, 2), "plslam_map_assoc_cpu"),
    "bow": ("plslam_set_bow_fn", BOW_FN, (0,), None),
}

_hl = None


def load_host(path: Optional[str] = None):
    global _hl
    if _hl is not None:
        return _hl
    path = path or HOST_LIB_PATH
    if not os.path.exists(path):
        raise PlbaError(f"libplslam_host.so not found at {path}: run `make -C pl-slam-plucker_amd/host`")
    L = C.CDLL(path)
    for name, argtypes in HOST_ARGTYPES.items():
        f = getattr(L, name)
        f.argtypes = argtypes
        f.restype = HOST_RESTYPES.get(name, C.c_int)
    _hl = L
    return L


def line_cells(x1: float, y1: float, x2: float, y2: float) -> np.ndarray:
    """getLineCoords (src2/gridStructure.cpp:33-41): the grid cells [k][2] of a line given in grid units."""
    L = load_host()
    n = C.c_int32(0)
    ip = C.POINTER(C.c_int32)
    L.plslam_line_cells(x1, y1, x2, y2, None, 0, C.byref(n))
    out = np.zeros((max(n.value, 1), 2), np.int32)
    rc = L.plslam_line_cells(x1, y1, x2, y2, out.ctypes.data_as(ip), n.value, C.byref(n))
    if rc != 0:
        raise PlbaError(f"plslam_line_cells failed: {rc}")
    return out[:n.value]


def _cpu_call(name: str, *args):
    """One of the library's *_cpu restatements (user pointer NULL); raises on a non-zero status."""
    rc = getattr(load_host(), name)(None, *args)
    if rc != 0:
        raise PlbaError(f"{name} failed: {rc}")


def _assoc_cpu(name: str, view_cls, params_fn, problems, params, desc_bytes):
    """The restatements over a view that holds its own outputs: (the view, the params struct) after the call."""
    bv = problems if isinstance(problems, view_cls) else view_cls(problems, desc_bytes)
    prm = params_fn(params)
    _cpu_call(name, C.byref(bv.struct), C.byref(prm), C.byref(bv.out))
    return bv, prm


def grid_match_cpu(problems, cols: int = 64, rows: int = 48, best_lr: bool = True, desc_bytes=None) -> list:
    """plslam_grid_match_cpu on the problems of Solver.grid_match (tests and tools/gridmatch_bench.py)."""
    bv = capi.GridMatchBatchView(problems, cols, rows, best_lr, desc_bytes)
    n = bv.struct.n
    m12 = np.full(max(int(bv.off1[-1]), 1), -1, np.int32)
    cnt = np.zeros(max(n, 1), np.int32)
    _cpu_call("plslam_grid_match_cpu", C.byref(bv.struct), m12.ctypes.data_as(_ip), cnt.ctypes.data_as(_ip))
    return [(m12[bv.off1[i]:bv.off1[i + 1]].copy(), int(cnt[i])) for i in range(n)]


def desc_medoid_cpu(list_ptr, desc, desc_bytes=None) -> np.ndarray:
    """plslam_desc_medoid_cpu on the lists of Solver.desc_medoid (tests and tools/fuse_bench.py)."""
    bv = capi.MedoidBatchView(list_ptr, desc, desc_bytes)
    out = np.full(max(bv.struct.n, 1), -1, np.int32)
    _cpu_call("plslam_desc_medoid_cpu", C.byref(bv.struct), out.ctypes.data_as(_ip))
    return out[:bv.struct.n].copy()


def kf_assoc_cpu(pairs, params, desc_bytes=None) -> list:
    """plslam_kf_assoc_cpu on the pairs of Solver.kf_associate (tests and tools/kfassoc_bench.py)."""
    return _assoc_cpu("plslam_kf_assoc_cpu", capi.KfassocBatchView, capi.kfassoc_params, pairs, params, desc_bytes)[0].results()


def map_assoc_cpu(problems, params, desc_bytes=None) -> list:
    """plslam_map_assoc_cpu on the keyframes of Solver.map_associate (tests and tools/mapassoc_bench.py)."""
    return _assoc_cpu("plslam_map_assoc_cpu", capi.MapassocBatchView, capi.mapassoc_params, problems, params,
                      desc_bytes)[0].results()


def stereo_cpu(frames, params, desc_bytes=None) -> list:
    """plslam_stereo_cpu on the frames of Solver.stereo_associate (tests and tools/stereo_bench.py)."""
    bv, prm = _assoc_cpu("plslam_stereo_cpu", capi.StereoBatchView, capi.stereo_params, frames, params, desc_bytes)
    return bv.results(bool(prm.pluker))


def _d(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(_dp)


def _mat4(T):
    """An optional (4, 4) matrix, row-major: (the array to keep alive, its pointer), or (None, None)."""
    return (None, None) if T is None else _d(np.asarray(T, np.float64).reshape(16))


def _ref(params):
    """An optional params struct: byref, or NULL for the library's defaults."""
    return C.byref(params) if params is not None else None


class HostMap:
    """A MapHandler (C++ host mirror) holding a SlamMap."""

    def __init__(self, m: SlamMap, corrected_line_jacobian: bool = False, device: int = 0,
                 params: Optional[SlamParams] = None):
        self.L = load_host()
        o = capi.PlbaOpts()
        from .lib import load
        load().plba_default_opts(C.byref(o))
        o.device = device
        o.corrected_line_jacobian = int(corrected_line_jacobian)
        self.h = C.c_void_p()
        self._check(self.L.plslam_map_create(C.byref(self.h), m.fx, m.fy, m.cx, m.cy, C.byref(o)), "create")
        self._hooks = {}     # hook name -> the callback object the C side holds, kept alive until replaced
        self._kf_feat = {}   # kf_idx -> (point features, line features), as given to plslam_add_keyframe
        self.n_kf = len(m.keyframes)
        self.n_pt = len(m.points)
        self.n_ln = len(m.lines)
        self._push(m)
        p = params or SlamParams()
        self._check(self.L.plslam_set_params(self.h, p.min_lm_obs, p.min_lm_cov_graph, p.min_kf_local_map), "params")

    def _check(self, rc, what):
        if rc != 0:
            msg = self.L.plslam_map_last_error(self.h).decode(errors="replace") if self.h else ""
            raise PlbaError(f"plslam {what} failed: {PLBA_ERRORS.get(rc, rc)}: {msg}")

    def close(self):
        if self.h:
            self.L.plslam_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _push(self, m: SlamMap):
        L, h = self.L, self.h
        ip = C.POINTER(C.c_int32)
        for kf in m.keyframes:
            if kf is None:
                continue
            T, Tp = _d(kf.T_kf_w.reshape(16))
            pi = np.asarray(kf.pt_idx, np.int32)
            li = np.asarray(kf.ls_idx, np.int32)
            self._check(L.plslam_add_keyframe(h, kf.kf_idx, Tp, len(pi), pi.ctypes.data_as(ip), len(li),
                                              li.ctypes.data_as(ip)), "add_keyframe")
            self._kf_feat[kf.kf_idx] = (len(pi), len(li))
            self._check(L.plslam_set_local(h, 0, kf.kf_idx, int(kf.local)), "set_local")
        bp = C.POINTER(C.c_uint8)
        for kind, lms in ((1, m.points), (2, m.lines)):
            for lm in lms:
                if lm is None:
                    continue
                for i in range(len(lm.kf_obs_list)):
                    desc = np.ascontiguousarray(lm.desc_list[i], np.uint8)
                    o, op = _d(lm.obs_list[i])
                    s = lm.sigma_list[i]
                    if kind == 1:
                        dvec, dpp = _d(lm.dir_list[i])
                        if i == 0:
                            x, xp = _d(lm.pos)
                            rc = L.plslam_add_point(h, lm.idx, xp, desc.ctypes.data_as(bp), len(desc),
                                                    lm.kf_obs_list[i], op, dpp, s)
                        else:
                            rc = L.plslam_point_add_observation(h, lm.idx, desc.ctypes.data_as(bp),
                                                                lm.kf_obs_list[i], op, dpp, s)
                    else:
                        if i == 0:
                            x, xp = _d(lm.pos)
                            rc = L.plslam_add_line(h, lm.idx, xp, desc.ctypes.data_as(bp), len(desc),
                                                   lm.kf_obs_list[i], op, s)
                        else:
                            rc = L.plslam_line_add_observation(h, lm.idx, desc.ctypes.data_as(bp),
                                                               lm.kf_obs_list[i], op, s)
                    self._check(rc, "add landmark")
                self._check(L.plslam_set_local(h, kind, lm.idx, int(lm.local)), "set_local")
                self._check(L.plslam_set_inlier(h, kind, lm.idx, int(lm.inlier)), "set_inlier")
        fg = np.ascontiguousarray(m.full_graph, np.uint32)
        self._check(L.plslam_set_full_graph(h, fg.shape[0], fg.ctypes.data_as(C.POINTER(C.c_uint32))), "full_graph")
        for k, lst in m.map_points_kf_idx.items():
            a = np.asarray(lst, np.int32)
            self._check(L.plslam_kf_idx_set(h, k, a.ctypes.data_as(ip), len(a)), "kf_idx_set")
        for k, lst in m.map_lines_kf_idx.items():
            a = np.asarray(lst, np.int32)
            self._check(L.plslam_kf_lines_idx_set(h, k, a.ctypes.data_as(ip), len(a)), "kf_lines_idx_set")
        self._check(L.plslam_set_max_kf_idx(h, int(m.max_kf_idx)), "max_kf_idx")

    def add_background(self, n_kf: int, n_pt: int, n_ln: int, seed: int = 0, obs_per_lm=(2, 5)):
        """Non-local keyframes and landmarks around the window (appended after the existing slots):
        e.g. a C5-sized map (BASELINE.json configs[4]: 1000 KF / 200k points / 40k lines) holding a
        C3 window, so that the per-call cost of the LBA is measured on a map of real size. Each
        background landmark is observed by 2-4 of the new keyframes; none is local."""
        L, h = self.L, self.h
        rng = np.random.default_rng(seed)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        k0 = self.n_kf
        for k in range(n_kf):
            T = np.eye(4)
            T[:3, 3] = rng.normal(size=3) * 10
            Tc = np.ascontiguousarray(T.reshape(16))
            self._check(L.plslam_add_keyframe(h, k0 + k, Tc.ctypes.data_as(dp), 0, None, 0, None), "add_keyframe")
        self.n_kf += n_kf
        for kind, n, width in ((1, n_pt, 2), (2, n_ln, 4)):
            base = self.n_pt if kind == 1 else self.n_ln
            nobs = rng.integers(obs_per_lm[0], obs_per_lm[1], size=n)
            kfs = (k0 + rng.integers(0, max(n_kf, 1), size=int(nobs.sum()))).astype(np.int32)
            obs = np.ascontiguousarray(rng.uniform(0, 700, size=(int(nobs.sum()), width)))
            pos = np.ascontiguousarray(rng.normal(size=(n, 3 if kind == 1 else 6)) * 5)
            d3 = np.ascontiguousarray(np.array([0.0, 0.0, 1.0]))
            po, oo, dd = pos.ctypes.data, obs.ctypes.data, d3.ctypes.data_as(dp)
            e = 0
            for i in range(n):
                idx = base + i
                xp = C.cast(po + i * pos.shape[1] * 8, dp)
                for j in range(int(nobs[i])):
                    op = C.cast(oo + e * width * 8, dp)
                    if j == 0:
                        rc = (L.plslam_add_point(h, idx, xp, None, DESC_BYTES, int(kfs[e]), op, dd, 1.0) if kind == 1
                              else L.plslam_add_line(h, idx, xp, None, DESC_BYTES, int(kfs[e]), op, 1.0))
                    else:
                        rc = (L.plslam_point_add_observation(h, idx, None, int(kfs[e]), op, dd, 1.0) if kind == 1
                              else L.plslam_line_add_observation(h, idx, None, int(kfs[e]), op, 1.0))
                    if rc:
                        self._check(rc, "add background landmark")
                    e += 1
            if kind == 1:
                self.n_pt += n
            else:
                self.n_ln += n

    def _set_hook(self, name: str, fn):
        """Installs ``fn`` as hook ``name`` of HOOKS: None clears it (the MI355X backend), "cpu" is the library's
        own CPU restatement, passed straight through, and a callable runs behind a trampoline that never lets
        an exception unwind through C: the traceback is printed and the hook returns -1."""
        setter, ftype, deref, cpu = HOOKS[name]
        if fn is None:
            cb = C.cast(None, ftype)
        elif isinstance(fn, str):
            if fn != "cpu" or cpu is None:
                raise ValueError(f"{setter}: {fn!r} is neither a callable nor a CPU restatement of this hook")
            cb = C.cast(getattr(self.L, cpu), ftype)
        else:
            def tramp(user, *args):
                try:
                    return int(fn(*(a.contents if i in deref else a for i, a in enumerate(args))))
                except Exception:  # never unwind through C
                    import traceback
                    traceback.print_exc()
                    return -1
            cb = ftype(tramp)
        set_fn = getattr(self.L, setter)
        self._check(set_fn(self.h, cb if set_fn.argtypes[1] is ftype else C.cast(cb, C.c_void_p), None), setter[7:])
        self._hooks[name] = cb

    @property
    def _cb(self):
        return self._hooks.get("solver")

    def set_solver(self, fn: Optional[Callable]):
        """fn(graph: PlbaGraph, result: PlbaResult) -> int, or None for the MI355X backend."""
        self._set_hook("solver", fn)

    def set_incremental(self, on: bool):
        self._check(self.L.plslam_set_incremental(self.h, int(on)), "set_incremental")

    def mark_landmark_changed(self, kind: int, idx: int):
        self._check(self.L.plslam_mark_landmark_changed(self.h, kind, idx), "mark_landmark_changed")

    def check_incremental_gather(self) -> bool:
        e = C.c_int32()
        self._check(self.L.plslam_check_incremental_gather(self.h, C.byref(e)), "check_incremental_gather")
        if not e.value:
            self._why = self.L.plslam_map_last_error(self.h).decode(errors="replace")
        return bool(e.value)

    def local_ba(self) -> dict:
        st = PlslamLbaStats()
        self._check(self.L.plslam_local_ba_plucker_g2o(self.h, C.byref(st)), "local_ba_plucker_g2o")
        return st.as_dict()

    # -- hand-rolled LM LBA (MapHandler::localBundleAdjustmentForPluker)
    def set_hlm_solver(self, fn: Optional[Callable]):
        """fn(graph, state, params, result) -> int, or None for the MI355X backend (plba_hlm_lba)."""
        self._set_hook("hlm", fn)

    def set_hlm_params(self, params=None, vo_inserting_kf: bool = False):
        self._check(self.L.plslam_set_hlm_params(self.h, _ref(params),
                                                 int(vo_inserting_kf)), "set_hlm_params")

    def local_ba_hlm(self) -> dict:
        st = PlslamHlmStats()
        self._check(self.L.plslam_local_ba_plucker(self.h, C.byref(st)), "local_ba_plucker")
        return st.as_dict()

    def local_ba_endpoints(self) -> dict:
        """MapHandler::localBundleAdjustment() (src/mapHandler.cpp:1392-1502): the endpoint-line
        hand-rolled LM (plslam_local_ba). Lines need ``set_line_geometry`` and image-line
        observations (a, b, c, 0); ``ret`` is the reference's 0 / -1."""
        st = PlslamHlmStats()
        self._check(self.L.plslam_local_ba(self.h, C.byref(st)), "local_ba")
        return st.as_dict()

    # ---- loop-closure pose graph (src/mapHandler.cpp:5070-5531)
    def set_loop_closure(self, lc_idxs, lc_idx_list, lc_pose_list):
        a = np.ascontiguousarray(np.asarray(lc_idxs, np.int32).reshape(-1, 3))
        b = np.ascontiguousarray(np.asarray(lc_idx_list, np.int32).reshape(-1, 3))
        c = np.ascontiguousarray(np.asarray(lc_pose_list, np.float64).reshape(-1, 6))
        ip = C.POINTER(C.c_int32)
        self._check(self.L.plslam_set_loop_closure(self.h, len(a), a.ctypes.data_as(ip), len(b), b.ctypes.data_as(ip),
                                                   len(c), c.ctypes.data_as(C.POINTER(C.c_double))), "set_loop_closure")

    def _sized(self, fn, what: str, width: int, ctype, *args) -> np.ndarray:
        """The getters fn(h, *args, out, cap, n) that report their row count: asked for it, then for the rows."""
        n = C.c_int32(0)
        self._check(fn(self.h, *args, None, 0, C.byref(n)), what)
        out = np.zeros((max(n.value, 1), width), ctype)
        self._check(fn(self.h, *args, out.ctypes.data_as(C.POINTER(ctype)), n.value, C.byref(n)), what)
        return out[:max(n.value, 0)]

    def lc_idx_list(self) -> np.ndarray:
        return self._sized(self.L.plslam_get_lc_idx_list, "get_lc_idx_list", 3, C.c_int32)

    def set_pgo_params(self, min_lm_ess_graph: int = 150, max_iters_pgo: int = 100):
        self._check(self.L.plslam_set_pgo_params(self.h, min_lm_ess_graph, max_iters_pgo), "set_pgo_params")

    def set_pgo_solver(self, fn: Optional[Callable]):
        """fn(graph, params, result) -> int, or None for the MI355X backend (plba_pgo_optimize)."""
        self._set_hook("pgo", fn)

    def loop_closure(self, ess: bool = True) -> dict:
        st = PlslamPgoStats()
        self._check(self.L.plslam_loop_closure_optimization(self.h, int(ess), C.byref(st)), "loop_closure")
        return st.as_dict()

    # ---- loopClosureFuseLandmarks (src/mapHandler.cpp:5533-5808)
    def set_lc_feature_idxs(self, kind: int, loop: int, rows):
        """The rows (lm_idx0, lm_ldx0, lm_idx1, lm_ldx1) of loop ``loop`` (kind 1 points, 2 lines)."""
        a = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 4))
        self._check(self.L.plslam_set_lc_feature_idxs(self.h, kind, loop, a.ctypes.data_as(C.POINTER(C.c_int32)), len(a)),
                    "set_lc_feature_idxs")

    def set_medoid_fn(self, fn):
        """fn(batch, medoid) -> int; "cpu" for plslam_desc_medoid_cpu (no trampoline: the C function
        itself); None for the MI355X backend (plba_desc_medoid)."""
        self._set_hook("medoid", fn)

    def fuse_landmarks(self) -> dict:
        st = PlslamFuseStats()
        self._check(self.L.plslam_fuse_landmarks(self.h, C.byref(st)), "fuse_landmarks")
        return st.as_dict()

    def loop_closure_fuse(self, ess: bool = True):
        """plslam_loop_closure_optimization_fuse: (pose-graph stats, fuse stats)."""
        st, fs = PlslamPgoStats(), PlslamFuseStats()
        self._check(self.L.plslam_loop_closure_optimization_fuse(self.h, int(ess), C.byref(st), C.byref(fs)),
                    "loop_closure_fuse")
        return st.as_dict(), fs.as_dict()

    # ---- loopClosure() from the candidate on (src/mapHandler.cpp:4053-4116)
    def set_lcpose_solver(self, fn: Optional[Callable]):
        """fn(batch, params, out, pt_inlier, ln_inlier) -> int, or None for the MI355X backend
        (plba_lc_relative_pose)."""
        self._set_hook("lcpose", fn)

    def set_lcpose_params(self, params=None):
        self._check(self.L.plslam_set_lcpose_params(self.h, _ref(params)),
                    "set_lcpose_params")

    def loop_closure_step(self, candidate=None, kf_prev_idx: int = 0, kf_curr_idx: int = 0, n_feat=None,
                          pt_idx=None, ls_idx=None, has_points: bool = True, has_lines: bool = True,
                          lc_inlier_ratio: float = 30.0) -> dict:
        """loopClosure() after lookForLoopCandidates and the descriptor matching. ``candidate``: the
        matched features (plba.lcpose.LcProblem) or None when there is no candidate; ``n_feat`` =
        (n_pt_0, n_pt_1, n_ls_0, n_ls_1), the feature counts of both keyframes; ``pt_idx`` /
        ``ls_idx``: [n][4] lc_pt_idx / lc_ls_idx rows."""
        st = PlslamLcStats()
        if candidate is None:
            self._check(self.L.plslam_loop_closure_step(self.h, None, lc_inlier_ratio, C.byref(st)), "loop_closure_step")
            return st.as_dict()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        keep = [np.ascontiguousarray(np.asarray(getattr(candidate, k), np.float64).reshape(-1, w))
                for k, w in (("pt_P", 3), ("pt_obs", 2), ("ln_sP", 3), ("ln_eP", 3), ("ln_le", 3))]
        n_pt, n_ln = len(keep[0]), len(keep[2])
        idx = [None if a is None else np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1, 4)) for a in (pt_idx, ls_idx)]
        if (idx[0] is not None and len(idx[0]) != n_pt) or (idx[1] is not None and len(idx[1]) != n_ln):
            raise ValueError("one index row per match")
        nf = n_feat if n_feat is not None else (n_pt, n_pt, n_ln, n_ln)
        c = PlslamLcCandidate(kf_prev_idx=kf_prev_idx, kf_curr_idx=kf_curr_idx, n_pt_0=nf[0], n_pt_1=nf[1],
                              n_ls_0=nf[2], n_ls_1=nf[3], has_points=int(has_points), has_lines=int(has_lines),
                              n_pt=n_pt, n_ln=n_ln, pt_P=keep[0].ctypes.data_as(dp), pt_obs=keep[1].ctypes.data_as(dp),
                              ln_sP=keep[2].ctypes.data_as(dp), ln_eP=keep[3].ctypes.data_as(dp),
                              ln_le=keep[4].ctypes.data_as(dp),
                              pt_idx=idx[0].ctypes.data_as(ip) if idx[0] is not None else None,
                              ls_idx=idx[1].ctypes.data_as(ip) if idx[1] is not None else None)
        self._check(self.L.plslam_loop_closure_step(self.h, C.byref(c), lc_inlier_ratio, C.byref(st)), "loop_closure_step")
        return st.as_dict()

    # ---- isLoopClosure from two keyframe indices (src/mapHandler.cpp:4303-4411)
    def set_keyframe_features(self, kf_idx: int, pdesc, pt_P, pt_pl, ldesc, ls_sP, ls_eP, ls_le, desc_bytes: int = 32):
        """What isLoopClosure reads of keyframe ``kf_idx``: pdesc_l [n_pt][desc_bytes] uint8 with P
        [n_pt][3] and pl [n_pt][2]; ldesc_l [n_ls][desc_bytes] with sP, eP and le [n_ls][3]. The
        counts are those of the keyframe's pt_idx / ls_idx."""
        bp, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        d = [np.ascontiguousarray(np.asarray(a, np.uint8).reshape(-1, desc_bytes)) for a in (pdesc, ldesc)]
        f = [np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, w))
             for a, w in ((pt_P, 3), (pt_pl, 2), (ls_sP, 3), (ls_eP, 3), (ls_le, 3))]
        if not (len(d[0]) == len(f[0]) == len(f[1]) and len(d[1]) == len(f[2]) == len(f[3]) == len(f[4])):
            raise ValueError("one row per feature in every array of a kind")
        if self._kf_feat.get(kf_idx, (0, 0)) != (len(d[0]), len(d[1])):
            raise ValueError(f"keyframe {kf_idx} has {self._kf_feat.get(kf_idx, (0, 0))} features, "
                             f"not ({len(d[0])}, {len(d[1])})")
        self._check(self.L.plslam_set_keyframe_features(
            self.h, kf_idx, desc_bytes, d[0].ctypes.data_as(bp), f[0].ctypes.data_as(dp), f[1].ctypes.data_as(dp),
            d[1].ctypes.data_as(bp), f[2].ctypes.data_as(dp), f[3].ctypes.data_as(dp), f[4].ctypes.data_as(dp)),
            "set_keyframe_features")

    def set_match_fn(self, fn: Optional[Callable]):
        """fn(batch, matches_12, n_matches) -> int, or None for the MI355X backend (plba_desc_match)."""
        self._set_hook("match", fn)

    # ---- place recognition: insertKFBowVector*, lookForLoopCandidates, loopClosure() whole
    def set_bow_cpu(self, bow_cpu: Optional["BowCpu"]):
        """Routes the place-recognition database through plslam_bow_cpu with ``bow_cpu``'s database (CPU
        tests), or, with None, back to the MI355X backend (plba_bow_*)."""
        self._bow_cpu = bow_cpu
        if bow_cpu is None:
            return self._set_hook("bow", None)
        fn = C.cast(self.L.plslam_bow_cpu, C.c_void_p)
        self._check(self.L.plslam_set_bow_fn(self.h, fn, bow_cpu.db), "set_bow_fn")

    def set_bow_fn(self, fn: Optional[Callable]):
        """fn(call: PlslamBowCall) -> int, or None for the MI355X backend."""
        self._set_hook("bow", fn)

    def set_vocabulary(self, slot: int, voc):
        vv = voc if isinstance(voc, capi.BowVocabView) else capi.BowVocabView(voc)
        self._check(self.L.plslam_set_vocabulary(self.h, slot, C.byref(vv.struct)), "set_vocabulary")

    def remove_keyframe(self, kf_idx: int):
        self._check(self.L.plslam_remove_keyframe(self.h, kf_idx), "remove_keyframe")

    def insert_kf_bow(self, kf_idx: int, has_points: bool = True, has_lines: bool = True):
        """insertKFBowVectorPL / P / L for keyframe ``kf_idx`` (its features given before)."""
        self._check(self.L.plslam_insert_kf_bow(self.h, kf_idx, int(has_points), int(has_lines)), "insert_kf_bow")

    def conf_matrix(self) -> np.ndarray:
        n = C.c_int32(0)
        fp = C.POINTER(C.c_float)
        if self.L.plslam_get_conf_matrix_row(self.h, 0, None, 0, C.byref(n)) != 0:
            return np.zeros((0, 0), np.float32)
        out = np.zeros((n.value, n.value), np.float32)
        for i in range(n.value):
            self._check(self.L.plslam_get_conf_matrix_row(self.h, i, out[i].ctypes.data_as(fp), n.value, C.byref(n)),
                        "get_conf_matrix_row")
        return out

    def set_conf_matrix(self, c):
        c = np.ascontiguousarray(c, np.float32)
        self._check(self.L.plslam_set_conf_matrix(self.h, len(c), c.ctypes.data_as(C.POINTER(C.c_float))), "set_conf_matrix")

    def look_for_loop_candidates(self, kf_curr_idx: int, params: Optional[PlslamLcSearchParams] = None):
        """lookForLoopCandidates: (is_candidate, kf_prev_idx)."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(self.L.plslam_look_for_loop_candidates(self.h, kf_curr_idx, _ref(params),
                                                           C.byref(a), C.byref(b)), "look_for_loop_candidates")
        return bool(a.value), b.value

    def loop_closure_kf(self, kf_curr_idx: int, search: Optional[PlslamLcSearchParams] = None,
                        params: Optional[PlslamMatchParams] = None, lc_inlier_ratio: float = 30.0) -> dict:
        """loopClosure() whole: the candidate search, then isLoopClosure and the state machine."""
        st = PlslamLcStats()
        self._check(self.L.plslam_loop_closure_kf(self.h, kf_curr_idx, _ref(search),
                                                  _ref(params), lc_inlier_ratio,
                                                  C.byref(st)), "loop_closure_kf")
        return st.as_dict()

    def loop_closure_step_kf(self, kf_prev_idx: int, kf_curr_idx: int, params: Optional[PlslamMatchParams] = None,
                             lc_inlier_ratio: float = 30.0) -> dict:
        """loopClosure() with isLoopClosure(kf_prev, kf_curr) whole: descriptor matching, gate,
        relative pose, lists and state machine."""
        st = PlslamLcStats()
        self._check(self.L.plslam_loop_closure_step_kf(self.h, kf_prev_idx, kf_curr_idx,
                                                       _ref(params),
                                                       lc_inlier_ratio, C.byref(st)), "loop_closure_step_kf")
        return st.as_dict()

    def verify_loop_candidates(self, kf_curr_idx: int, kf_prev_idxs, params: Optional[PlslamMatchParams] = None,
                               lc_inlier_ratio: float = 30.0) -> dict:
        """K candidates for one new keyframe in one match call and one relative-pose call; no map
        state is changed. accepted [K], pose_inc [K][6], n_matches [K][2] (points, lines)."""
        prev = np.ascontiguousarray(np.asarray(kf_prev_idxs, np.int32).reshape(-1))
        k = len(prev)
        acc, pose, cnt = np.zeros(max(k, 1), np.int32), np.zeros((max(k, 1), 6)), np.zeros((max(k, 1), 2), np.int32)
        ip = C.POINTER(C.c_int32)
        self._check(self.L.plslam_verify_loop_candidates(
            self.h, kf_curr_idx, k, prev.ctypes.data_as(ip), _ref(params),
            lc_inlier_ratio, acc.ctypes.data_as(ip), pose.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(ip)),
            "verify_loop_candidates")
        return dict(accepted=acc[:k], pose_inc=pose[:k], n_matches=cnt[:k])

    # ---- matchMap2KFPoints / Lines (src/mapHandler.cpp:697-921)
    def set_keyframe_line_endpoints(self, kf_idx: int, spl, epl):
        """The image endpoints spl / epl [n_ls][2] of keyframe ``kf_idx``'s line features."""
        a, b = (np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 2)) for x in (spl, epl))
        if not len(a) == len(b) == self._kf_feat.get(kf_idx, (0, 0))[1]:
            raise ValueError("one row per line feature")
        dp = C.POINTER(C.c_double)
        self._check(self.L.plslam_set_keyframe_line_endpoints(self.h, kf_idx, a.ctypes.data_as(dp), b.ctypes.data_as(dp)),
                    "set_keyframe_line_endpoints")

    def set_stereo_fn(self, fn):
        """fn(batch, params, out) -> int; "cpu" for plslam_stereo_cpu; None for the MI355X backend
        (plba_stereo_associate)."""
        self._set_hook("stereo", fn)

    def set_keyframe_stereo(self, kf_idx: int, frame: dict, params, desc_bytes=None) -> dict:
        """The features of keyframe ``kf_idx`` from the detector output of its two images (``frame``: a
        dict as in capi.StereoBatchView): matchStereoPoints + matchStereoLines through
        plba_stereo_associate or the hook, stored as set_keyframe_features + set_keyframe_line_endpoints
        would store them. Returns n_pt, n_ls, pt_src, ls_src (the left row of each feature) and ms."""
        bv = capi.StereoBatchView([frame], desc_bytes)
        fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        n = {k: len(bv.co[k]) for k in bv.co}
        fr = PlslamStereoFrame(
            desc_bytes=bv.desc_bytes, n_pt_l=n["pt_l"], n_pt_r=n["pt_r"], n_ls_l=n["ls_l"], n_ls_r=n["ls_r"], pad=0,
            pt_l=bv.co["pt_l"].ctypes.data_as(fp), pt_r=bv.co["pt_r"].ctypes.data_as(fp),
            pdesc_l=bv.desc["pt_l"].ctypes.data_as(bp), pdesc_r=bv.desc["pt_r"].ctypes.data_as(bp),
            ls_l=bv.co["ls_l"].ctypes.data_as(fp), ls_r=bv.co["ls_r"].ctypes.data_as(fp),
            ldesc_l=bv.desc["ls_l"].ctypes.data_as(bp), ldesc_r=bv.desc["ls_r"].ctypes.data_as(bp))
        prm = capi.stereo_params(params)
        ip = C.POINTER(C.c_int32)
        psrc, lsrc = np.full(n["pt_l"] + 1, -1, np.int32), np.full(n["ls_l"] + 1, -1, np.int32)
        st = PlslamStereoStats()
        self._check(self.L.plslam_set_keyframe_stereo(self.h, kf_idx, C.byref(fr), C.byref(prm), psrc.ctypes.data_as(ip),
                                                      lsrc.ctypes.data_as(ip), C.byref(st)), "set_keyframe_stereo")
        self._kf_feat[kf_idx] = (st.n_pt, st.n_ls)
        return dict(n_pt=st.n_pt, n_ls=st.n_ls, pt_src=psrc[:st.n_pt].copy(), ls_src=lsrc[:st.n_ls].copy(), ms=st.ms)

    def set_keyframe_line_pluker(self, kf_idx: int, NDc):
        """The Plücker lines NDc [n_ls][6] (camera frame) of keyframe ``kf_idx``'s line features."""
        a = np.ascontiguousarray(np.asarray(NDc, np.float64).reshape(-1, 6))
        if len(a) != self._kf_feat.get(kf_idx, (0, 0))[1]:
            raise ValueError("one row per line feature")
        self._check(self.L.plslam_set_keyframe_line_pluker(self.h, kf_idx, a.ctypes.data_as(C.POINTER(C.c_double))),
                    "set_keyframe_line_pluker")

    def set_kfassoc_fn(self, fn):
        """fn(batch, params, out) -> int; "cpu" for plslam_kf_assoc_cpu; None for the MI355X backend
        (plba_kf_associate)."""
        self._set_hook("kfassoc", fn)

    def _kfmatch_stats(self, kf_prev_idx: int):
        n = self._kf_feat.get(kf_prev_idx, (0, 0))
        pp, lp = np.full((n[0] + 1, 2), -1, np.int32), np.full((n[1] + 1, 2), -1, np.int32)
        ip = C.POINTER(C.c_int32)
        return PlslamKfMatchStats(pt_cap=n[0], ls_cap=n[1], pt_pairs=pp.ctypes.data_as(ip), ls_pairs=lp.ctypes.data_as(ip)), pp, lp

    @staticmethod
    def _kfmatch_dict(st, pp, lp):
        d = st.as_dict()
        d["pt_pairs"], d["ls_pairs"] = pp[:st.n_pairs[0]].tolist(), lp[:st.n_pairs[1]].tolist()
        return d

    def match_kf_to_kf(self, kf_prev_idx: int, kf_curr_idx: int, DT=None, params=None) -> dict:
        """matchKF2KFPoints + matchKF2KFLines between two keyframes with features: new landmarks are created,
        existing ones extended, rejected lines reset. ``DT`` (4, 4), None for expmap(logmap(inverse(T_curr) *
        T_prev)); ``params``: a dict over plba_kfassoc_default_params (or a capi.PlbaKfassocParams); without
        width / height the camera of set_camera is used. Returns the statistics with the accepted pairs."""
        st, pp, lp = self._kfmatch_stats(kf_prev_idx)
        T, Tp = _mat4(DT)
        prm = capi.kfassoc_params(params)
        self._check(self.L.plslam_match_kf_to_kf(
            self.h, kf_prev_idx, kf_curr_idx, Tp,
            C.byref(prm), C.byref(st)), "match_kf_to_kf")
        return self._kfmatch_dict(st, pp, lp)

    def look_for_common_matches(self, kf_prev_idx: int, kf_curr_idx: int, kf_params=None,
                                map_params: Optional[PlslamMapMatchParams] = None) -> dict:
        """match_kf_to_kf (DT None), then match_map_to_kf of the current keyframe: lookForCommonMatches without
        the pose refinement. Returns dict(kf=..., map=...) of both statistics."""
        st, pp, lp = self._kfmatch_stats(kf_prev_idx)
        ms = PlslamMapMatchStats()
        prm = capi.kfassoc_params(kf_params)
        self._check(self.L.plslam_look_for_common_matches(
            self.h, kf_prev_idx, kf_curr_idx, C.byref(prm), _ref(map_params),
            C.byref(st), C.byref(ms)), "look_for_common_matches")
        return dict(kf=self._kfmatch_dict(st, pp, lp), map=ms.as_dict())

    def set_camera(self, fx: float, fy: float, cx: float, cy: float, width: int, height: int):
        self._check(self.L.plslam_set_camera(self.h, fx, fy, cx, cy, width, height), "set_camera")

    def set_grid_match_fn(self, fn):
        """fn(batch, matches_12, n_matches) -> int; "cpu" for plslam_grid_match_cpu; None for the
        MI355X backend (plba_grid_match)."""
        self._set_hook("grid", fn)

    def match_map_to_kf(self, kf_idx: int, Twf=None, params: Optional[PlslamMapMatchParams] = None) -> dict:
        """matchMap2KFPoints + matchMap2KFLines for keyframe ``kf_idx``; ``Twf`` (4, 4) world ->
        keyframe, None for the inverse of its T_kf_w. Returns the statistics."""
        st = PlslamMapMatchStats()
        T, Tp = _mat4(Twf)
        self._check(self.L.plslam_match_map_to_kf(
            self.h, kf_idx, Tp,
            _ref(params), C.byref(st)), "match_map_to_kf")
        return st.as_dict()

    def set_mapassoc_fn(self, fn):
        """fn(batch, params, out) -> int; "cpu" for plslam_map_assoc_cpu; None for the MI355X backend
        (plba_map_associate)."""
        self._set_hook("mapassoc", fn)

    def match_map_to_kf_assoc(self, kf_idx: int, Twf=None, params=None) -> dict:
        """match_map_to_kf around one plba_map_associate call (or the hook of set_mapassoc_fn). ``params``: a
        dict over plba_mapassoc_default_params (or a capi.PlbaMapassocParams); without width / height the
        camera of set_camera is used. Returns the statistics of match_map_to_kf."""
        st = PlslamMapMatchStats()
        T, Tp = _mat4(Twf)
        prm = capi.mapassoc_params(params)
        self._check(self.L.plslam_match_map_to_kf_assoc(
            self.h, kf_idx, Tp, C.byref(prm), C.byref(st)),
            "match_map_to_kf_assoc")
        return st.as_dict()

    def local_mapping_step_kf_assoc(self, kf_idx: int, params=None) -> dict:
        """match_map_to_kf_assoc, then local_mapping_step."""
        ms, st = PlslamMapMatchStats(), PlslamLbaStats()
        a, b = C.c_int32(), C.c_int32()
        prm = capi.mapassoc_params(params)
        self._check(self.L.plslam_local_mapping_step_kf_assoc(self.h, kf_idx, C.byref(prm), C.byref(ms), C.byref(st),
                                                              C.byref(a), C.byref(b)), "local_mapping_step_kf_assoc")
        return self._step_dict(st, a, b, ms)

    def local_mapping_step_kf(self, kf_idx: int, params: Optional[PlslamMapMatchParams] = None) -> dict:
        """match_map_to_kf, then local_mapping_step."""
        ms, st = PlslamMapMatchStats(), PlslamLbaStats()
        a, b = C.c_int32(), C.c_int32()
        self._check(self.L.plslam_local_mapping_step_kf(self.h, kf_idx, _ref(params),
                                                        C.byref(ms), C.byref(st), C.byref(a), C.byref(b)),
                    "local_mapping_step_kf")
        return self._step_dict(st, a, b, ms)

    def lc_state(self) -> int:
        v = C.c_int32(0)
        self._check(self.L.plslam_get_lc_state(self.h, C.byref(v)), "get_lc_state")
        return v.value

    def lc_pose_list(self) -> np.ndarray:
        return self._sized(self.L.plslam_get_lc_pose_list, "get_lc_pose_list", 6, C.c_double)

    def lc_feature_idxs(self, kind: int, loop: int) -> np.ndarray:
        """The kept lc_pt_idx (kind 1) / lc_ls_idx (kind 2) rows of accepted loop ``loop``."""
        return self._sized(self.L.plslam_get_lc_feature_idxs, "get_lc_feature_idxs", 4, C.c_int32, kind, loop)

    def set_line_geometry(self, idx: int, line3d, med_obs_dir):
        a, pa = _d(line3d)
        b, pb = _d(med_obs_dir)
        self._check(self.L.plslam_set_line_geometry(self.h, idx, pa, pb), "set_line_geometry")

    def line_geometry(self, idx: int):
        a, b = np.zeros(6), np.zeros(3)
        self._check(self.L.plslam_get_line_geometry(self.h, idx, a.ctypes.data_as(C.POINTER(C.c_double)),
                                                    b.ctypes.data_as(C.POINTER(C.c_double))), "get_line_geometry")
        return a, b

    def keyframe_x(self, kf_idx: int) -> np.ndarray:
        x = np.zeros(6)
        self._check(self.L.plslam_get_keyframe_x(self.h, kf_idx, x.ctypes.data_as(C.POINTER(C.c_double))), "get_x")
        return x

    def set_keyframe_x(self, kf_idx: int, x):
        a, ap = _d(x)
        self._check(self.L.plslam_set_keyframe_x(self.h, kf_idx, ap), "set_x")

    def form_local_map(self, kf_idx: int):
        self._check(self.L.plslam_form_local_map(self.h, kf_idx), "form_local_map")

    def remove_bad_landmarks(self):
        a, b = C.c_int32(), C.c_int32()
        self._check(self.L.plslam_remove_bad_landmarks_pluker(self.h, C.byref(a), C.byref(b)), "remove_bad")
        return a.value, b.value

    def local_mapping_step(self, kf_idx: int) -> dict:
        st = PlslamLbaStats()
        a, b = C.c_int32(), C.c_int32()
        self._check(self.L.plslam_local_mapping_step(self.h, kf_idx, C.byref(st), C.byref(a), C.byref(b)),
                    "local_mapping_step")
        return self._step_dict(st, a, b)

    @staticmethod
    def _step_dict(st, n_pt_removed, n_ln_removed, ms=None) -> dict:
        """What the local-mapping steps return: the LBA statistics, the culled counts and the match statistics."""
        d = st.as_dict()
        d["points_removed"], d["lines_removed"] = n_pt_removed.value, n_ln_removed.value
        if ms is not None:
            d["match"] = ms.as_dict()
        return d

    def exists(self, kind: int, idx: int) -> bool:
        e = C.c_int32()
        self._check(self.L.plslam_exists(self.h, kind, idx, C.byref(e)), "exists")
        return bool(e.value)

    def read(self, like: SlamMap) -> SlamMap:
        """Read the map state back (same object layout as `like`)."""
        L, h = self.L, self.h
        out = like.copy()
        ip = C.POINTER(C.c_int32)
        for kf in out.keyframes:
            if kf is None:
                continue
            T = np.zeros(16)
            loc = C.c_int32()
            pi = np.zeros(len(kf.pt_idx), np.int32)
            li = np.zeros(len(kf.ls_idx), np.int32)
            self._check(L.plslam_get_keyframe(h, kf.kf_idx, T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(loc),
                                              pi.ctypes.data_as(ip), len(pi), li.ctypes.data_as(ip), len(li)),
                        "get_keyframe")
            kf.T_kf_w = T.reshape(4, 4)
            kf.local = bool(loc.value)
            kf.pt_idx = [int(v) for v in pi]
            kf.ls_idx = [int(v) for v in li]
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        for kind, lms in ((1, out.points), (2, out.lines)):
            for j, lm in enumerate(lms):
                if lm is None:
                    continue
                if not self.exists(kind, lm.idx):   # deleted by removeBadMapLandmarksForPluker
                    lms[j] = None
                    continue
                cap = len(lm.kf_obs_list) + len(lm.sigma_list) + 4
                inl, loc, nobs = C.c_int32(), C.c_int32(), C.c_int32()
                kfo = np.zeros(cap, np.int32)
                sig = np.zeros(cap)
                md = np.zeros(DESC_BYTES, np.uint8)
                if kind == 1:
                    pos = np.zeros(3)
                    obs = np.zeros((cap, 2))
                    dirs = np.zeros((cap, 3))
                    mdir = np.zeros(3)
                    self._check(L.plslam_get_point(h, lm.idx, pos.ctypes.data_as(dp), C.byref(inl), C.byref(loc),
                                                   C.byref(nobs), kfo.ctypes.data_as(ip), obs.ctypes.data_as(dp),
                                                   dirs.ctypes.data_as(dp), sig.ctypes.data_as(dp), cap,
                                                   md.ctypes.data_as(bp), mdir.ctypes.data_as(dp)), "get_point")
                    n = nobs.value
                    lm.dir_list = [dirs[i].copy() for i in range(n)]
                    lm.med_dir = mdir
                else:
                    pos = np.zeros(6)
                    obs = np.zeros((cap, 4))
                    self._check(L.plslam_get_line(h, lm.idx, pos.ctypes.data_as(dp), C.byref(inl), C.byref(loc),
                                                  C.byref(nobs), kfo.ctypes.data_as(ip), obs.ctypes.data_as(dp),
                                                  sig.ctypes.data_as(dp), cap, md.ctypes.data_as(bp)), "get_line")
                    n = nobs.value
                lm.pos = pos
                lm.inlier = bool(inl.value)
                lm.local = bool(loc.value)
                lm.kf_obs_list = [int(v) for v in kfo[:n]]
                lm.obs_list = [obs[i].copy() for i in range(n)]
                lm.sigma_list = [float(v) for v in sig[:len(lm.sigma_list)]]
                lm.med_desc = md
                lm.desc_list = None   # not exposed; med_desc covers the descriptor logic
        fg = np.zeros_like(out.full_graph)
        self._check(L.plslam_get_full_graph(h, fg.shape[0], fg.ctypes.data_as(C.POINTER(C.c_uint32))), "full_graph")
        out.full_graph = fg
        for k in list(out.map_points_kf_idx.keys()):
            out.map_points_kf_idx[k] = self._sized(L.plslam_kf_idx_get, "kf_idx_get", 1, C.c_int32, k)[:, 0].tolist()
        for k in list(out.map_lines_kf_idx.keys()):
            out.map_lines_kf_idx[k] = self._sized(L.plslam_kf_lines_idx_get, "kf_lines_idx_get", 1, C.c_int32,
                                                  k)[:, 0].tolist()
        return out
