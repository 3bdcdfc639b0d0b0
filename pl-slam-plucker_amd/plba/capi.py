"""ctypes mirror of include/plba.h (structs only; no library is loaded here)."""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from .synth import Graph

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_bp = C.POINTER(C.c_uint8)


class PlbaGraph(C.Structure):
    _fields_ = [
        ("n_kf", C.c_int32), ("n_pt", C.c_int32), ("n_ln", C.c_int32), ("n_ept", C.c_int32), ("n_eln", C.c_int32),
        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
        ("kf_Tcw", _dp), ("kf_fixed", _bp), ("kf_id", _ip),
        ("pt_xyz", _dp), ("pt_id", _ip),
        ("ln_orth", _dp), ("ln_id", _ip),
        ("ept_lm", _ip), ("ept_kf", _ip), ("ept_obs", _dp), ("ept_info", _dp),
        ("eln_lm", _ip), ("eln_kf", _ip), ("eln_obs", _dp), ("eln_info", _dp),
        ("huber_pt", C.c_double), ("huber_ln", C.c_double),
    ]


class PlbaIterTrace(C.Structure):
    _fields_ = [("stage", C.c_int32), ("iter", C.c_int32), ("trials", C.c_int32), ("result", C.c_int32),
                ("chi2_start", C.c_double), ("chi2_end", C.c_double),
                ("lambda_start", C.c_double), ("lambda_end", C.c_double)]


class PlbaResult(C.Structure):
    _fields_ = [("kf_Tcw", _dp), ("pt_xyz", _dp), ("ln_orth", _dp),
                ("ept_chi2", _dp), ("ept_depth_ok", _bp), ("ept_level", _bp),
                ("eln_chi2", _dp), ("eln_level", _bp),
                ("iters", C.c_int32 * 2), ("chi2", C.c_double * 2), ("solve_ms", C.c_double)]


class PlbaOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("corrected_line_jacobian", C.c_int32), ("verbose", C.c_int32),
                ("max_trials", C.c_int32), ("tau", C.c_double)]


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(t)


class GraphView:
    """Keeps contiguous copies of a Graph's arrays alive and exposes a PlbaGraph."""

    def __init__(self, g: Graph):
        self.keep: List[np.ndarray] = []

        def f64(a, shape_last=None):
            a = np.ascontiguousarray(a, dtype=np.float64)
            self.keep.append(a)
            return _ptr(a, _dp)

        def i32(a):
            a = np.ascontiguousarray(a, dtype=np.int32)
            self.keep.append(a)
            return _ptr(a, _ip)

        def u8(a):
            a = np.ascontiguousarray(a, dtype=np.uint8)
            self.keep.append(a)
            return _ptr(a, _bp)

        s = PlbaGraph()
        s.n_kf, s.n_pt, s.n_ln, s.n_ept, s.n_eln = g.n_kf, g.n_pt, g.n_ln, g.n_ept, g.n_eln
        s.fx, s.fy, s.cx, s.cy = g.fx, g.fy, g.cx, g.cy
        s.kf_Tcw = f64(g.kf_Tcw.reshape(-1, 12))
        s.kf_fixed = u8(g.kf_fixed)
        s.kf_id = i32(g.kf_id)
        s.pt_xyz = f64(g.pt_xyz.reshape(-1, 3))
        s.pt_id = i32(g.pt_id)
        s.ln_orth = f64(g.ln_orth.reshape(-1, 4))
        s.ln_id = i32(g.ln_id)
        s.ept_lm, s.ept_kf = i32(g.ept_lm), i32(g.ept_kf)
        s.ept_obs, s.ept_info = f64(g.ept_obs.reshape(-1, 2)), f64(g.ept_info)
        s.eln_lm, s.eln_kf = i32(g.eln_lm), i32(g.eln_kf)
        s.eln_obs, s.eln_info = f64(g.eln_obs.reshape(-1, 4)), f64(g.eln_info)
        s.huber_pt, s.huber_ln = g.huber_pt, g.huber_ln
        self.struct = s


class ResultBuffers:
    """Host output arrays for plba_result."""

    def __init__(self, g: Graph):
        self.kf_Tcw = np.zeros((g.n_kf, 3, 4))
        self.pt_xyz = np.zeros((g.n_pt, 3))
        self.ln_orth = np.zeros((g.n_ln, 4))
        self.ept_chi2 = np.zeros(g.n_ept)
        self.ept_depth_ok = np.zeros(g.n_ept, np.uint8)
        self.ept_level = np.zeros(g.n_ept, np.uint8)
        self.eln_chi2 = np.zeros(g.n_eln)
        self.eln_level = np.zeros(g.n_eln, np.uint8)
        r = PlbaResult()
        r.kf_Tcw = _ptr(self.kf_Tcw, _dp)
        r.pt_xyz = _ptr(self.pt_xyz, _dp)
        r.ln_orth = _ptr(self.ln_orth, _dp)
        r.ept_chi2 = _ptr(self.ept_chi2, _dp)
        r.ept_depth_ok = _ptr(self.ept_depth_ok, _bp)
        r.ept_level = _ptr(self.ept_level, _bp)
        r.eln_chi2 = _ptr(self.eln_chi2, _dp)
        r.eln_level = _ptr(self.eln_level, _bp)
        self.struct = r

    def as_dict(self) -> dict:
        s = self.struct
        return dict(kf_Tcw=self.kf_Tcw, pt_xyz=self.pt_xyz, ln_orth=self.ln_orth,
                    ept_chi2=self.ept_chi2, ept_depth_ok=self.ept_depth_ok, ept_level=self.ept_level,
                    eln_chi2=self.eln_chi2, eln_level=self.eln_level,
                    iters=np.array([s.iters[0], s.iters[1]], np.int32),
                    chi2=np.array([s.chi2[0], s.chi2[1]]), solve_ms=float(s.solve_ms))


def trace_to_array(tr, n: int) -> np.ndarray:
    """Structured numpy array from a PlbaIterTrace buffer."""
    dt = np.dtype([("stage", np.int32), ("iter", np.int32), ("trials", np.int32), ("result", np.int32),
                   ("chi2_start", np.float64), ("chi2_end", np.float64),
                   ("lambda_start", np.float64), ("lambda_end", np.float64)])
    out = np.zeros(n, dt)
    for i in range(n):
        t = tr[i]
        out[i] = (t.stage, t.iter, t.trials, t.result, t.chi2_start, t.chi2_end, t.lambda_start, t.lambda_end)
    return out


# ---- hand-rolled LM (plba_hlm_*)
class PlbaHlmState(C.Structure):
    _fields_ = [("kf_x", _dp), ("ln_pluker", _dp), ("ln_line3d", _dp)]


class PlbaHlmParams(C.Structure):
    _fields_ = [("lambda0", C.c_double), ("lambda_k", C.c_double), ("homog_th", C.c_double),
                ("min_error", C.c_double), ("min_error_change", C.c_double),
                ("max_iters", C.c_int32), ("err_per_obs", C.c_int32), ("variant", C.c_int32), ("pad", C.c_int32)]


HLM_LBA_PLUCKER = 0
HLM_GBA = 1
HLM_LBA_ENDPOINTS = 2
DBL_EPSILON = float(np.finfo(np.float64).eps)


class PlbaHlmResult(C.Structure):
    _fields_ = [("kf_x", _dp), ("kf_Tcw", _dp), ("pt_xyz", _dp), ("ln_orth", _dp),
                ("linearizations", C.c_int32), ("solves", C.c_int32), ("accepted", C.c_int32), ("pad", C.c_int32),
                ("err", C.c_double), ("lambda_", C.c_double), ("dx_norm", C.c_double), ("solve_ms", C.c_double),
                ("ln_line3d", _dp)]


def gba_params(**kw) -> "PlbaHlmParams":
    """levMarquardtOptimizationGBA: the LBA defaults with ε stop tests (src/mapHandler.cpp:3664,3694)."""
    p = hlm_params(min_error=DBL_EPSILON, min_error_change=DBL_EPSILON, variant=HLM_GBA)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def lba_params(**kw) -> "PlbaHlmParams":
    """levMarquardtOptimizationLBA (src/mapHandler.cpp:2350-2352): lambdaLbaLM, lambdaLbaK and maxItersLba
    with the Config stop tests, the same defaults as the Plücker hand-rolled LM, on endpoint lines."""
    p = hlm_params(variant=HLM_LBA_ENDPOINTS)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def hlm_params(**kw) -> PlbaHlmParams:
    """Defaults of src/slamConfig.cpp:65-67 and src2/config.cpp:80-85 (plba_hlm_default_params)."""
    p = PlbaHlmParams(lambda0=1e-5, lambda_k=10.0, homog_th=1e-7, min_error=1e-7, min_error_change=1e-7,
                      max_iters=15, err_per_obs=0, variant=HLM_LBA_PLUCKER)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class HlmStateView:
    def __init__(self, kf_x: np.ndarray, ln_pluker: np.ndarray, ln_line3d=None):
        self.kf_x = np.ascontiguousarray(kf_x, np.float64).reshape(-1, 6)
        self.ln_pluker = np.ascontiguousarray(ln_pluker, np.float64).reshape(-1, 6)
        self.ln_line3d = np.ascontiguousarray(ln_line3d if ln_line3d is not None else np.zeros((0, 6)),
                                              np.float64).reshape(-1, 6)
        self.struct = PlbaHlmState(kf_x=_ptr(self.kf_x, _dp), ln_pluker=_ptr(self.ln_pluker, _dp),
                                   ln_line3d=_ptr(self.ln_line3d, _dp) if self.ln_line3d.size else None)


class HlmResultBuffers:
    def __init__(self, g: Graph):
        self.kf_x = np.zeros((g.n_kf, 6))
        self.kf_Tcw = np.zeros((g.n_kf, 3, 4))
        self.pt_xyz = np.zeros((g.n_pt, 3))
        self.ln_orth = np.zeros((g.n_ln, 4))
        self.ln_line3d = np.zeros((g.n_ln, 6))
        self.struct = PlbaHlmResult(kf_x=_ptr(self.kf_x, _dp), kf_Tcw=_ptr(self.kf_Tcw, _dp),
                                    pt_xyz=_ptr(self.pt_xyz, _dp), ln_orth=_ptr(self.ln_orth, _dp),
                                    ln_line3d=_ptr(self.ln_line3d, _dp))

    def as_dict(self) -> dict:
        s = self.struct
        return dict(kf_x=self.kf_x, kf_Tcw=self.kf_Tcw, pt_xyz=self.pt_xyz, ln_orth=self.ln_orth,
                    ln_line3d=self.ln_line3d,
                    linearizations=int(s.linearizations), solves=int(s.solves), accepted=int(s.accepted),
                    err=float(s.err), lam=float(s.lambda_), dx_norm=float(s.dx_norm), solve_ms=float(s.solve_ms))


# ---- loop-closure pose graph (plba_pgo_*)
class PlbaPgoGraph(C.Structure):
    _fields_ = [("n_v", C.c_int32), ("n_e", C.c_int32), ("v_id", _ip), ("v_T", _dp), ("v_fixed", _bp),
                ("e_v", _ip), ("e_Z", _dp), ("e_info", _dp)]


class PlbaPgoParams(C.Structure):
    _fields_ = [("user_lambda_init", C.c_double), ("max_iters", C.c_int32), ("initial_guess", C.c_int32),
                ("max_trials", C.c_int32), ("pad", C.c_int32)]


class PlbaPgoResult(C.Structure):
    _fields_ = [("v_T", _dp), ("trace", C.POINTER(PlbaIterTrace)), ("trace_cap", C.c_int32), ("n_trace", C.c_int32),
                ("iterations", C.c_int32), ("trials", C.c_int32), ("solve_fails", C.c_int32), ("n_free", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double),
                ("solve_ms", C.c_double)]


def pgo_params(**kw) -> PlbaPgoParams:
    """plba_pgo_default_params: the reference's values (setUserLambdaInit(1e-10), maxItersPGO 100)."""
    p = PlbaPgoParams(user_lambda_init=1e-10, max_iters=100, initial_guess=1, max_trials=10, pad=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class PgoGraphView:
    """Contiguous copies of a plba.pgo.PoseGraph's arrays and the PlbaPgoGraph over them."""

    def __init__(self, pg):
        self.v_id = np.ascontiguousarray(pg.v_id, dtype=np.int32)
        self.v_T = np.ascontiguousarray(pg.v_T, dtype=np.float64).reshape(-1, 12)
        self.v_fixed = np.ascontiguousarray(pg.v_fixed, dtype=np.uint8)
        self.e_v = np.ascontiguousarray(pg.e_v, dtype=np.int32).reshape(-1, 2)
        self.e_Z = np.ascontiguousarray(pg.e_Z, dtype=np.float64).reshape(-1, 12)
        self.e_info = None if pg.e_info is None else np.ascontiguousarray(pg.e_info, dtype=np.float64).reshape(-1, 36)
        self.struct = PlbaPgoGraph(
            n_v=len(self.v_id), n_e=len(self.e_v), v_id=_ptr(self.v_id, _ip), v_T=_ptr(self.v_T, _dp),
            v_fixed=_ptr(self.v_fixed, _bp), e_v=_ptr(self.e_v, _ip), e_Z=_ptr(self.e_Z, _dp),
            e_info=_ptr(self.e_info, _dp) if self.e_info is not None else C.cast(None, _dp))


class PgoResultBuffers:
    def __init__(self, n_v: int, trace_cap: int = 256):
        self.v_T = np.zeros((n_v, 12))
        self.trace = (PlbaIterTrace * trace_cap)()
        self.struct = PlbaPgoResult(v_T=_ptr(self.v_T, _dp), trace=self.trace, trace_cap=trace_cap)

    def as_dict(self) -> dict:
        s = self.struct
        return dict(v_T=self.v_T.copy(), iterations=s.iterations, trials=s.trials, solve_fails=s.solve_fails,
                    n_free=s.n_free, chi2_initial=s.chi2_initial, chi2_final=s.chi2_final,
                    lambda_final=s.lambda_final, solve_ms=s.solve_ms, trace=trace_to_array(self.trace, s.n_trace))


# ---- loop-closure relative pose (plba_lcpose_* / plba_lc_relative_pose)
LCPOSE_ROBUST_GN = 0
LCPOSE_GN = 1


class PlbaLcposeBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("pt_off", _ip), ("ln_off", _ip), ("pt_P", _dp), ("pt_obs", _dp),
                ("ln_sP", _dp), ("ln_eP", _dp), ("ln_le", _dp),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class PlbaLcposeParams(C.Structure):
    _fields_ = [("homog_th", C.c_double), ("lc_res", C.c_double), ("lc_unc", C.c_double), ("lc_inl", C.c_double),
                ("lc_trs", C.c_double), ("lc_rot", C.c_double),
                ("max_iters_first", C.c_int32), ("max_iters", C.c_int32), ("variant", C.c_int32), ("pad", C.c_int32)]


class PlbaLcposeOut(C.Structure):
    _fields_ = [("accepted", C.c_int32), ("conditions", C.c_int32), ("iters_first", C.c_int32),
                ("iters_ref", C.c_int32), ("n_inl_pt", C.c_int32), ("n_inl_ln", C.c_int32),
                ("e", C.c_double), ("unc", C.c_double), ("t", C.c_double), ("r_deg", C.c_double),
                ("x_inc", C.c_double * 6), ("pose_inc", C.c_double * 6), ("T_inc", C.c_double * 12),
                ("H", C.c_double * 36)]


def lcpose_params(**kw) -> PlbaLcposeParams:
    """plba_lcpose_default_params: src2/config.cpp:80-83 and src/slamConfig.cpp:73-77."""
    p = PlbaLcposeParams(homog_th=1e-7, lc_res=1.0, lc_unc=0.01, lc_inl=0.3, lc_trs=1.5, lc_rot=35.0,
                         max_iters_first=5, max_iters=10, variant=LCPOSE_ROBUST_GN, pad=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class LcposeBatchView:
    """Concatenates candidate pairs (objects with pt_P, pt_obs, ln_sP, ln_eP, ln_le and cam, e.g.
    plba.lcpose.LcProblem) into contiguous arrays and the PlbaLcposeBatch over them."""

    def __init__(self, problems):
        def cat(name, w):
            rows = [np.asarray(getattr(q, name), np.float64).reshape(-1, w) for q in problems]
            return np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, w)))

        self.pt_P, self.pt_obs = cat("pt_P", 3), cat("pt_obs", 2)
        self.ln_sP, self.ln_eP, self.ln_le = cat("ln_sP", 3), cat("ln_eP", 3), cat("ln_le", 3)
        self.pt_off = np.zeros(len(problems) + 1, np.int32)
        self.ln_off = np.zeros(len(problems) + 1, np.int32)
        for i, q in enumerate(problems):
            self.pt_off[i + 1] = self.pt_off[i] + len(np.asarray(q.pt_P).reshape(-1, 3))
            self.ln_off[i + 1] = self.ln_off[i] + len(np.asarray(q.ln_sP).reshape(-1, 3))
        cam = problems[0].cam if problems else (1.0, 1.0, 0.0, 0.0)
        if any(tuple(q.cam) != tuple(cam) for q in problems):
            raise ValueError("the candidates of one batch share one camera")
        self.struct = PlbaLcposeBatch(
            n=len(problems), pt_off=_ptr(self.pt_off, _ip), ln_off=_ptr(self.ln_off, _ip),
            pt_P=_ptr(self.pt_P, _dp), pt_obs=_ptr(self.pt_obs, _dp), ln_sP=_ptr(self.ln_sP, _dp),
            ln_eP=_ptr(self.ln_eP, _dp), ln_le=_ptr(self.ln_le, _dp), fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3])


def lcpose_out_to_dict(o: PlbaLcposeOut, pt_inlier, ln_inlier) -> dict:
    return dict(accepted=int(o.accepted), conditions=int(o.conditions), iters_first=int(o.iters_first),
                iters_ref=int(o.iters_ref), n_inl_pt=int(o.n_inl_pt), n_inl_ln=int(o.n_inl_ln),
                e=float(o.e), unc=float(o.unc), t=float(o.t), r_deg=float(o.r_deg),
                x_inc=np.array(o.x_inc[:]), pose_inc=np.array(o.pose_inc[:]),
                T_inc=np.array(o.T_inc[:]).reshape(3, 4), H=np.array(o.H[:]).reshape(6, 6),
                pt_inlier=np.array(pt_inlier, np.uint8), ln_inlier=np.array(ln_inlier, np.uint8))


# ---- frame-to-frame pose (plba_track_* / plba_track_pose)
TRACK_MAX_N = 2048       # PLBA_TRACK_MAX_N: matches of one kind in one problem
TRACK_PLUCKER = 0
TRACK_ENDPOINTS = 1
TRACK_OK, TRACK_FEW_BEFORE, TRACK_FIRST_NOT_GOOD, TRACK_FEW_AFTER, TRACK_FINAL_NOT_GOOD = range(5)
TRACK_PREV = 53          # doubles of a problem's motion-model input: DT, DT_cov, err_norm


class PlbaTrackBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("pt_off", _ip), ("ln_off", _ip), ("pt_P", _dp), ("pt_obs", _dp), ("pt_sigma2", _dp),
                ("ln_sP", _dp), ("ln_eP", _dp), ("ln_NDc", _dp), ("ln_le", _dp), ("ln_obs", _dp), ("ln_seg", _dp),
                ("ln_sigma2", _dp), ("prev", _dp),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class PlbaTrackParams(C.Structure):
    _fields_ = [("homog_th", C.c_double), ("min_error", C.c_double), ("min_error_change", C.c_double),
                ("inlier_k", C.c_double), ("min_features", C.c_int32), ("max_iters", C.c_int32),
                ("max_iters_ref", C.c_int32), ("has_points", C.c_int32), ("has_lines", C.c_int32),
                ("use_motion_model", C.c_int32), ("line_model", C.c_int32), ("pad", C.c_int32)]


class PlbaTrackOut(C.Structure):
    _fields_ = [("branch", C.c_int32), ("iters_first", C.c_int32), ("iters_ref", C.c_int32),
                ("n_inl_pt", C.c_int32), ("n_inl_ln", C.c_int32), ("pad", C.c_int32),
                ("err_norm", C.c_double), ("s_p", C.c_double), ("s_l", C.c_double),
                ("DT", C.c_double * 16), ("DT_cov", C.c_double * 36), ("DT_cov_eig", C.c_double * 6),
                ("DT_solver", C.c_double * 16), ("H", C.c_double * 36)]


def track_params(**kw) -> PlbaTrackParams:
    """plba_track_default_params: src2/config.cpp:46-53, :80-86."""
    p = PlbaTrackParams(homog_th=1e-7, min_error=1e-7, min_error_change=1e-7, inlier_k=4.0, min_features=10,
                        max_iters=5, max_iters_ref=10, has_points=1, has_lines=1, use_motion_model=0,
                        line_model=TRACK_PLUCKER, pad=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class TrackBatchView:
    """Concatenates frame pairs (objects with the arrays of plba.trackpose.TrackProblem) into
    contiguous arrays and the PlbaTrackBatch over them."""
    FIELDS = (("pt_P", 3), ("pt_obs", 2), ("pt_sigma2", 1), ("ln_sP", 3), ("ln_eP", 3), ("ln_NDc", 6), ("ln_le", 3),
              ("ln_obs", 4), ("ln_seg", 4), ("ln_sigma2", 1))

    def __init__(self, problems):
        def cat(name, w):
            rows = [np.asarray(getattr(q, name), np.float64).reshape(-1, w) for q in problems]
            return np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, w)))

        self.arrays = {name: cat(name, w) for name, w in self.FIELDS}
        self.pt_off = np.zeros(len(problems) + 1, np.int32)
        self.ln_off = np.zeros(len(problems) + 1, np.int32)
        for i, q in enumerate(problems):
            self.pt_off[i + 1] = self.pt_off[i] + len(np.asarray(q.pt_P).reshape(-1, 3))
            self.ln_off[i + 1] = self.ln_off[i] + len(np.asarray(q.ln_sP).reshape(-1, 3))
        self.prev = np.ascontiguousarray(np.stack([np.asarray(q.prev, np.float64).reshape(TRACK_PREV) for q in problems])
                                         if problems else np.zeros((0, TRACK_PREV)))
        cam = problems[0].cam if problems else (1.0, 1.0, 0.0, 0.0)
        if any(tuple(q.cam) != tuple(cam) for q in problems):
            raise ValueError("the problems of one batch share one camera")
        self.struct = PlbaTrackBatch(n=len(problems), pt_off=_ptr(self.pt_off, _ip), ln_off=_ptr(self.ln_off, _ip),
                                     prev=_ptr(self.prev, _dp), fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3],
                                     **{name: _ptr(a, _dp) for name, a in self.arrays.items()})


def track_out_to_dict(o: PlbaTrackOut, pt_inlier, ln_inlier) -> dict:
    return dict(branch=int(o.branch), iters_first=int(o.iters_first), iters_ref=int(o.iters_ref),
                n_inl_pt=int(o.n_inl_pt), n_inl_ln=int(o.n_inl_ln), err_norm=float(o.err_norm),
                s_p=float(o.s_p), s_l=float(o.s_l), DT=np.array(o.DT[:]).reshape(4, 4),
                DT_cov=np.array(o.DT_cov[:]).reshape(6, 6), DT_cov_eig=np.array(o.DT_cov_eig[:]),
                DT_solver=np.array(o.DT_solver[:]).reshape(4, 4), H=np.array(o.H[:]).reshape(6, 6),
                pt_inlier=np.array(pt_inlier, np.uint8), ln_inlier=np.array(ln_inlier, np.uint8))


# ---- descriptor matching (plba_match_batch / plba_desc_match)
_fp = C.POINTER(C.c_float)


class PlbaMatchBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc_bytes", C.c_int32), ("off1", _ip), ("off2", _ip), ("desc1", _bp),
                ("desc2", _bp), ("nnr", _fp), ("best_lr", C.c_int32), ("pad", C.c_int32)]


class MatchBatchView:
    """Concatenates descriptor-set pairs [(desc1 [n1][desc_bytes] uint8, desc2 [n2][desc_bytes]), ...]
    into contiguous arrays and the PlbaMatchBatch over them. ``nnr``: one ratio, or one per pair."""

    def __init__(self, pairs, nnr, best_lr: bool = True, desc_bytes=None):
        pairs = [(np.asarray(a, np.uint8), np.asarray(b, np.uint8)) for a, b in pairs]
        if desc_bytes is None:
            desc_bytes = next((x.shape[1] for p in pairs for x in p if x.ndim == 2 and x.shape[1]), 32)
        pairs = [(a.reshape(-1, desc_bytes), b.reshape(-1, desc_bytes)) for a, b in pairs]
        self.desc_bytes = int(desc_bytes)
        empty = np.zeros((0, desc_bytes), np.uint8)
        self.desc1 = np.ascontiguousarray(np.concatenate([a for a, _ in pairs] + [empty]))
        self.desc2 = np.ascontiguousarray(np.concatenate([b for _, b in pairs] + [empty]))
        self.off1 = np.zeros(len(pairs) + 1, np.int32)
        self.off2 = np.zeros(len(pairs) + 1, np.int32)
        self.off1[1:] = np.cumsum([len(a) for a, _ in pairs], dtype=np.int64)
        self.off2[1:] = np.cumsum([len(b) for _, b in pairs], dtype=np.int64)
        self.nnr = np.ascontiguousarray(np.broadcast_to(np.asarray(nnr, np.float32), (len(pairs),)))
        self.struct = PlbaMatchBatch(
            n=len(pairs), desc_bytes=self.desc_bytes, off1=_ptr(self.off1, _ip), off2=_ptr(self.off2, _ip),
            desc1=_ptr(self.desc1, _bp), desc2=_ptr(self.desc2, _bp), nnr=_ptr(self.nnr, _fp),
            best_lr=int(bool(best_lr)), pad=0)


# ---- frame-to-frame tracking (plba_frames_* / plba_track_frames)
class PlbaFramesBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("pt_off1", _ip), ("pt_off2", _ip), ("ln_off1", _ip), ("ln_off2", _ip),
                ("prev_pdesc", _bp), ("prev_pt_P", _dp), ("prev_pt_sigma2", _dp),
                ("prev_ldesc", _bp), ("prev_ln_sP", _dp), ("prev_ln_eP", _dp), ("prev_ln_NDc", _dp), ("prev_ln_seg", _dp),
                ("prev_ln_sigma2", _dp),
                ("cur_pdesc", _bp), ("cur_pt_pl", _dp), ("cur_ldesc", _bp), ("cur_ln_seg", _dp), ("cur_ln_le", _dp),
                ("prev", _dp), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class PlbaFramesParams(C.Structure):
    _fields_ = [("track", PlbaTrackParams), ("nnr_pt", C.c_float), ("nnr_ln", C.c_float), ("best_lr", C.c_int32),
                ("desc_bytes", C.c_int32)]


class PlbaFramesOut(C.Structure):
    _fields_ = [("out", C.POINTER(PlbaTrackOut)), ("pt_m12", _ip), ("ln_m12", _ip), ("n_pt", _ip), ("n_ln", _ip),
                ("pt_inlier", _bp), ("ln_inlier", _bp), ("pt_cur_from_prev", _ip), ("ln_cur_from_prev", _ip)]


def frames_params(track=None, nnr_pt=0.9, nnr_ln=0.9, best_lr=True, desc_bytes=32) -> PlbaFramesParams:
    """plba_frames_default_params (src2/config.cpp:51, :60, :68) over ``track`` (a PlbaTrackParams; None: its defaults)."""
    p = PlbaFramesParams(nnr_pt=nnr_pt, nnr_ln=nnr_ln, best_lr=int(bool(best_lr)), desc_bytes=int(desc_bytes))
    C.memmove(C.byref(p.track), C.byref(track if track is not None else track_params()), C.sizeof(PlbaTrackParams))
    return p


class FramesBatchView:
    """Concatenates frame pairs (objects with the arrays of plba.trackframes.FramePair) into contiguous
    arrays per kind and side, the PlbaFramesBatch over them, and the output arrays with their PlbaFramesOut."""
    F64 = (("prev_pt_P", 3, "pt1"), ("prev_pt_sigma2", 1, "pt1"), ("prev_ln_sP", 3, "ln1"), ("prev_ln_eP", 3, "ln1"),
           ("prev_ln_NDc", 6, "ln1"), ("prev_ln_seg", 4, "ln1"), ("prev_ln_sigma2", 1, "ln1"), ("cur_pt_pl", 2, "pt2"),
           ("cur_ln_seg", 4, "ln2"), ("cur_ln_le", 3, "ln2"))
    DESC = (("prev_pdesc", "pt1"), ("prev_ldesc", "ln1"), ("cur_pdesc", "pt2"), ("cur_ldesc", "ln2"))

    def __init__(self, pairs, desc_bytes=32):
        pairs = list(pairs)
        db = int(desc_bytes)
        self.off = {}
        for name, key in self.DESC:
            rows = [np.asarray(getattr(q, name), np.uint8) for q in pairs]
            rows = [r if r.ndim == 2 else r.reshape(-1, db) for r in rows]   # (rows of their own width are the caller's claim)
            off = np.zeros(len(pairs) + 1, np.int32)
            off[1:] = np.cumsum([len(r) for r in rows], dtype=np.int64)
            self.off[key] = off
            setattr(self, name, np.ascontiguousarray(np.concatenate([r.reshape(-1) for r in rows] + [np.zeros(1, np.uint8)])))
        self.arrays = {}
        for name, w, key in self.F64:
            rows = [np.asarray(getattr(q, name), np.float64).reshape(-1, w) for q in pairs]
            a = np.ascontiguousarray(np.concatenate(rows + [np.zeros((0, w))]))
            if len(a) != self.off[key][-1]:
                raise ValueError(f"{name} has {len(a)} rows, the descriptors have {self.off[key][-1]}")
            self.arrays[name] = a
        self.prev = np.ascontiguousarray(np.stack([np.asarray(q.prev, np.float64).reshape(TRACK_PREV) for q in pairs])
                                         if pairs else np.zeros((0, TRACK_PREV)))
        cam = pairs[0].cam if pairs else (1.0, 1.0, 0.0, 0.0)
        if any(tuple(q.cam) != tuple(cam) for q in pairs):
            raise ValueError("the pairs of one batch share one camera")
        n = len(pairs)
        self.struct = PlbaFramesBatch(
            n=n, pad=0, pt_off1=_ptr(self.off["pt1"], _ip), pt_off2=_ptr(self.off["pt2"], _ip),
            ln_off1=_ptr(self.off["ln1"], _ip), ln_off2=_ptr(self.off["ln2"], _ip),
            prev=_ptr(self.prev, _dp), fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3],
            **{name: _ptr(getattr(self, name), _bp) for name, _ in self.DESC},
            **{name: _ptr(a, _dp) for name, a in self.arrays.items()})
        # the outputs (an array of no rows still has an address)
        i32 = lambda k, fill: np.full(max(int(self.off[k][-1]), 1), fill, np.int32)
        self.out = (PlbaTrackOut * max(n, 1))()
        self.pt_m12, self.ln_m12 = i32("pt1", -1), i32("ln1", -1)
        self.pt_cfp, self.ln_cfp = i32("pt2", -1), i32("ln2", -1)
        self.n_pt, self.n_ln = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        self.pt_inl = np.zeros(max(int(self.off["pt1"][-1]), 1), np.uint8)
        self.ln_inl = np.zeros(max(int(self.off["ln1"][-1]), 1), np.uint8)
        self.out_struct = PlbaFramesOut(
            out=self.out, pt_m12=_ptr(self.pt_m12, _ip), ln_m12=_ptr(self.ln_m12, _ip), n_pt=_ptr(self.n_pt, _ip),
            n_ln=_ptr(self.n_ln, _ip), pt_inlier=_ptr(self.pt_inl, _bp), ln_inlier=_ptr(self.ln_inl, _bp),
            pt_cur_from_prev=_ptr(self.pt_cfp, _ip), ln_cur_from_prev=_ptr(self.ln_cfp, _ip))

    def results(self) -> list:
        """One dict per pair: the fields of track_out_to_dict (the inlier flags per PREVIOUS row) and pt_m12,
        ln_m12, n_pt, n_ln, pt_cur_from_prev, ln_cur_from_prev."""
        o = self.off
        res = []
        for k in range(self.struct.n):
            s = lambda a, key: a[o[key][k]:o[key][k + 1]].copy()
            d = track_out_to_dict(self.out[k], s(self.pt_inl, "pt1"), s(self.ln_inl, "ln1"))
            d.update(pt_m12=s(self.pt_m12, "pt1"), ln_m12=s(self.ln_m12, "ln1"), n_pt=int(self.n_pt[k]), n_ln=int(self.n_ln[k]),
                     pt_cur_from_prev=s(self.pt_cfp, "pt2"), ln_cur_from_prev=s(self.ln_cfp, "ln2"))
            res.append(d)
        return res


# ---- median descriptor (plba_medoid_batch / plba_desc_medoid)
class PlbaMedoidBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc_bytes", C.c_int32), ("list_ptr", _ip), ("desc", _bp)]


MEDOID_MAX_N = 1024  # PLBA_MEDOID_MAX_N


class MedoidBatchView:
    """Contiguous copies of the CSR offsets list_ptr [B+1] and the descriptors desc [total][desc_bytes]
    uint8 of a batch of descriptor lists, and the PlbaMedoidBatch over them."""

    def __init__(self, list_ptr, desc, desc_bytes=None):
        self.list_ptr = np.ascontiguousarray(list_ptr, dtype=np.int32).reshape(-1)
        desc = np.asarray(desc, np.uint8)
        if desc_bytes is None:
            desc_bytes = desc.shape[1] if desc.ndim == 2 and desc.shape[1] else 32
        self.desc_bytes = int(desc_bytes)
        self.desc = np.ascontiguousarray(desc).reshape(-1)
        n = len(self.list_ptr) - 1
        if n < 0 or (n > 0 and int(self.list_ptr[-1]) * self.desc_bytes > self.desc.size):
            raise ValueError("list_ptr is empty or reaches past the descriptors")
        if self.desc.size == 0:
            self.desc = np.zeros(1, np.uint8)
        self.struct = PlbaMedoidBatch(n=n, desc_bytes=self.desc_bytes, list_ptr=_ptr(self.list_ptr, _ip),
                                      desc=_ptr(self.desc, _bp))


# ---- place recognition (plba_bow_vocab / plba_bow_*)
class PlbaBowVocab(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_words", C.c_int32), ("desc_bytes", C.c_int32), ("pad", C.c_int32),
                ("child_off", _ip), ("children", _ip), ("node_desc", _bp), ("word_id", _ip), ("weight", _dp)]


class BowVocabView:
    """Contiguous copies of a flat vocabulary tree and the PlbaBowVocab over them. ``voc``: a dict (or
    an object) with child_off [n_nodes+1], children, node_desc [n_nodes][desc_bytes] uint8, word_id
    [n_nodes] (-1 on inner nodes), weight [n_nodes] and n_words."""

    def __init__(self, voc):
        get = voc.__getitem__ if isinstance(voc, dict) else (lambda k: getattr(voc, k))
        self.child_off = np.ascontiguousarray(get("child_off"), dtype=np.int32)
        self.children = np.ascontiguousarray(get("children"), dtype=np.int32)
        self.node_desc = np.ascontiguousarray(get("node_desc"), dtype=np.uint8)
        self.word_id = np.ascontiguousarray(get("word_id"), dtype=np.int32)
        self.weight = np.ascontiguousarray(get("weight"), dtype=np.float64)
        n_nodes = len(self.word_id)
        try:
            self.desc_bytes = int(get("desc_bytes"))
        except (KeyError, AttributeError):
            self.desc_bytes = int(self.node_desc.shape[1])
        self.struct = PlbaBowVocab(
            n_nodes=n_nodes, n_words=int(get("n_words")), desc_bytes=self.desc_bytes, pad=0,
            child_off=_ptr(self.child_off, _ip), children=_ptr(self.children, _ip),
            node_desc=_ptr(self.node_desc, _bp), word_id=_ptr(self.word_id, _ip), weight=_ptr(self.weight, _dp))


# ---- grid-guided matching (plba_gridmatch_batch / plba_grid_match)
class PlbaGridMatchBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc_bytes", C.c_int32), ("cols", C.c_int32), ("rows", C.c_int32),
                ("best_lr", C.c_int32), ("pad", C.c_int32), ("off1", _ip), ("off2", _ip), ("desc1", _bp),
                ("desc2", _bp), ("cell1", _ip), ("cell1_end", _ip), ("cell_off2", _ip), ("cells2", _ip),
                ("dir2", _dp), ("kind", _ip), ("ws", _ip), ("nnr", _dp), ("line_sim_th", _dp)]


class GridMatchBatchView:
    """Concatenates matchGrid problems into contiguous arrays and the PlbaGridMatchBatch over them.
    A problem is a dict: kind (0 points, 1 lines), ws, nnr, line_sim_th (lines), desc1 [n1][desc_bytes]
    uint8, cell1 [n1][2] int, cell1_end [n1][2] (lines), desc2 [n2][desc_bytes], cells2 (one [k][2] int
    array per train row) and dir2 [n2][2] (lines)."""

    def __init__(self, problems, cols: int = 64, rows: int = 48, best_lr: bool = True, desc_bytes=None):
        problems = list(problems)
        if desc_bytes is None:
            desc_bytes = next((np.asarray(p[k]).shape[1] for p in problems for k in ("desc1", "desc2")
                               if np.asarray(p[k]).ndim == 2 and np.asarray(p[k]).shape[1]), 32)
        self.desc_bytes = db = int(desc_bytes)
        n = len(problems)
        d1 = [np.asarray(p["desc1"], np.uint8).reshape(-1, db) for p in problems]
        d2 = [np.asarray(p["desc2"], np.uint8).reshape(-1, db) for p in problems]
        self.off1 = np.zeros(n + 1, np.int32)
        self.off2 = np.zeros(n + 1, np.int32)
        self.off1[1:] = np.cumsum([len(a) for a in d1], dtype=np.int64)
        self.off2[1:] = np.cumsum([len(a) for a in d2], dtype=np.int64)
        self.desc1 = np.ascontiguousarray(np.concatenate(d1 + [np.zeros((0, db), np.uint8)]))
        self.desc2 = np.ascontiguousarray(np.concatenate(d2 + [np.zeros((0, db), np.uint8)]))
        n1, n2 = int(self.off1[-1]), int(self.off2[-1])
        self.cell1 = np.zeros((n1, 2), np.int32)
        self.cell1_end = np.zeros((n1, 2), np.int32)
        self.dir2 = np.zeros((n2, 2), np.float64)
        counts, cells = [], [np.zeros((0, 2), np.int32)]
        for k, p in enumerate(problems):
            a, b = self.off1[k], self.off1[k + 1]
            self.cell1[a:b] = np.asarray(p["cell1"], np.int32).reshape(-1, 2)
            if p["kind"] == 1:
                self.cell1_end[a:b] = np.asarray(p["cell1_end"], np.int32).reshape(-1, 2)
                self.dir2[self.off2[k]:self.off2[k + 1]] = np.asarray(p["dir2"], np.float64).reshape(-1, 2)
            if len(p["cells2"]) != len(d2[k]):
                raise ValueError("one cell list per train row")
            for c in p["cells2"]:
                c = np.asarray(c, np.int32).reshape(-1, 2)
                counts.append(len(c))
                cells.append(c)
        self.cell_off2 = np.zeros(n2 + 1, np.int32)
        self.cell_off2[1:] = np.cumsum(counts, dtype=np.int64)
        self.cells2 = np.ascontiguousarray(np.concatenate(cells))
        self.kind = np.array([int(p["kind"]) for p in problems], np.int32).reshape(n)
        self.ws = np.array([int(p["ws"]) for p in problems], np.int32).reshape(n)
        self.nnr = np.array([float(p["nnr"]) for p in problems], np.float64).reshape(n)
        self.line_sim_th = np.array([float(p.get("line_sim_th", 0.75)) for p in problems], np.float64).reshape(n)
        self.struct = PlbaGridMatchBatch(
            n=n, desc_bytes=db, cols=int(cols), rows=int(rows), best_lr=int(bool(best_lr)), pad=0,
            off1=_ptr(self.off1, _ip), off2=_ptr(self.off2, _ip), desc1=_ptr(self.desc1, _bp),
            desc2=_ptr(self.desc2, _bp), cell1=_ptr(self.cell1, _ip), cell1_end=_ptr(self.cell1_end, _ip),
            cell_off2=_ptr(self.cell_off2, _ip), cells2=_ptr(self.cells2, _ip), dir2=_ptr(self.dir2, _dp),
            kind=_ptr(self.kind, _ip), ws=_ptr(self.ws, _ip), nnr=_ptr(self.nnr, _dp),
            line_sim_th=_ptr(self.line_sim_th, _dp))


# ---- stereo association (plba_stereo_params / plba_stereo_batch / plba_stereo_out / plba_stereo_associate)
class PlbaStereoParams(C.Structure):
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("matching_s_ws", C.c_int32), ("best_lr", C.c_int32), ("pluker", C.c_int32), ("pad", C.c_int32),
                ("min_ratio_12_p", C.c_double), ("line_sim_th", C.c_double), ("max_dist_epip", C.c_double),
                ("min_disp", C.c_double), ("ls_min_disp_ratio", C.c_double), ("line_horiz_th", C.c_double),
                ("stereo_overlap_th", C.c_double), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("b", C.c_double)]


class PlbaStereoBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc_bytes", C.c_int32), ("pt_off_l", _ip), ("pt_off_r", _ip), ("ls_off_l", _ip),
                ("ls_off_r", _ip), ("pt_l", _fp), ("pt_r", _fp), ("pdesc_l", _bp), ("pdesc_r", _bp), ("ls_l", _fp),
                ("ls_r", _fp), ("ldesc_l", _bp), ("ldesc_r", _bp)]


class PlbaStereoOut(C.Structure):
    _fields_ = [("n_pt", _ip), ("n_ls", _ip), ("pt_src", _ip), ("pt_pl", _dp), ("pt_disp", _dp), ("pt_P", _dp),
                ("pdesc", _bp), ("ls_src", _ip), ("ls_spl", _dp), ("ls_epl", _dp), ("ls_sdisp", _dp), ("ls_edisp", _dp),
                ("ls_sP", _dp), ("ls_eP", _dp), ("ls_le", _dp), ("ls_NDc", _dp), ("ldesc", _bp)]


def stereo_params(params=None) -> PlbaStereoParams:
    """PlbaStereoParams from a dict: plba_stereo_default_params, then the dict's entries (width, height,
    fx, fy, cx, cy and b have no default)."""
    if isinstance(params, PlbaStereoParams):
        return params
    from . import lib   # lib imports this module
    p = PlbaStereoParams()
    lib.load().plba_stereo_default_params(C.byref(p))
    for k, v in dict(params or {}).items():
        if k not in dict(PlbaStereoParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class StereoBatchView:
    """Concatenates stereo frames into contiguous arrays, the PlbaStereoBatch over them and the output
    arrays of a call. A frame is a dict: pt_l [n][2] / pt_r float32, pdesc_l / pdesc_r [n][desc_bytes] uint8,
    ls_l / ls_r [n][4] float32 (sx, sy, ex, ey), ldesc_l / ldesc_r; a missing key is an empty side."""

    KEYS = (("pt_l", 2), ("pt_r", 2), ("ls_l", 4), ("ls_r", 4))
    DESC = {"pt_l": "pdesc_l", "pt_r": "pdesc_r", "ls_l": "ldesc_l", "ls_r": "ldesc_r"}

    def __init__(self, frames, desc_bytes=None):
        frames = list(frames)
        if desc_bytes is None:
            desc_bytes = next((np.asarray(f[k]).shape[1] for f in frames for k in self.DESC.values()
                               if k in f and np.asarray(f[k]).ndim == 2 and np.asarray(f[k]).shape[1]), 32)
        self.desc_bytes = db = int(desc_bytes)
        self.n = n = len(frames)
        self.off, self.co, self.desc = {}, {}, {}
        for key, per in self.KEYS:
            co = [np.asarray(f.get(key, np.zeros((0, per))), np.float32).reshape(-1, per) for f in frames]
            de = [np.asarray(f.get(self.DESC[key], np.zeros((0, db))), np.uint8).reshape(-1, db) for f in frames]
            if any(len(a) != len(d) for a, d in zip(co, de)):
                raise ValueError("one descriptor row per feature")
            off = np.zeros(n + 1, np.int32)
            off[1:] = np.cumsum([len(a) for a in co], dtype=np.int64)
            self.off[key] = off
            self.co[key] = np.ascontiguousarray(np.concatenate(co + [np.zeros((0, per), np.float32)]))
            self.desc[key] = np.ascontiguousarray(np.concatenate(de + [np.zeros((0, db), np.uint8)]))
        self.struct = PlbaStereoBatch(
            n=n, desc_bytes=db, pt_off_l=_ptr(self.off["pt_l"], _ip), pt_off_r=_ptr(self.off["pt_r"], _ip),
            ls_off_l=_ptr(self.off["ls_l"], _ip), ls_off_r=_ptr(self.off["ls_r"], _ip),
            pt_l=_ptr(self.co["pt_l"], _fp), pt_r=_ptr(self.co["pt_r"], _fp), pdesc_l=_ptr(self.desc["pt_l"], _bp),
            pdesc_r=_ptr(self.desc["pt_r"], _bp), ls_l=_ptr(self.co["ls_l"], _fp), ls_r=_ptr(self.co["ls_r"], _fp),
            ldesc_l=_ptr(self.desc["ls_l"], _bp), ldesc_r=_ptr(self.desc["ls_r"], _bp))
        npt, nls = max(int(self.off["pt_l"][-1]), 1), max(int(self.off["ls_l"][-1]), 1)
        # rows past a frame's count are never written: a fill that no result can equal shows it
        self.o = dict(
            n_pt=np.zeros(max(n, 1), np.int32), n_ls=np.zeros(max(n, 1), np.int32),
            pt_src=np.full(npt, -7, np.int32), pt_pl=np.full((npt, 2), np.nan), pt_disp=np.full(npt, np.nan),
            pt_P=np.full((npt, 3), np.nan), pdesc=np.zeros((npt, db), np.uint8),
            ls_src=np.full(nls, -7, np.int32), ls_spl=np.full((nls, 2), np.nan), ls_epl=np.full((nls, 2), np.nan),
            ls_sdisp=np.full(nls, np.nan), ls_edisp=np.full(nls, np.nan), ls_sP=np.full((nls, 3), np.nan),
            ls_eP=np.full((nls, 3), np.nan), ls_le=np.full((nls, 3), np.nan), ls_NDc=np.full((nls, 6), np.nan),
            ldesc=np.zeros((nls, db), np.uint8))
        kinds = {np.dtype(np.int32): _ip, np.dtype(np.float64): _dp, np.dtype(np.uint8): _bp}
        self.out = PlbaStereoOut(**{k: v.ctypes.data_as(kinds[v.dtype]) for k, v in self.o.items()})

    PT = ("pt_src", "pt_pl", "pt_disp", "pt_P", "pdesc")
    LS = ("ls_src", "ls_spl", "ls_epl", "ls_sdisp", "ls_edisp", "ls_sP", "ls_eP", "ls_le", "ls_NDc", "ldesc")

    def results(self, pluker: bool) -> list:
        """One dict per frame: n_pt, n_ls and the first n_pt / n_ls rows of every output array (ls_NDc only
        with pluker), copied."""
        res = []
        for f in range(self.n):
            kp, kl = int(self.o["n_pt"][f]), int(self.o["n_ls"][f])
            a, b = int(self.off["pt_l"][f]), int(self.off["ls_l"][f])
            r = dict(n_pt=kp, n_ls=kl)
            r.update({k: self.o[k][a:a + kp].copy() for k in self.PT})
            r.update({k: self.o[k][b:b + kl].copy() for k in self.LS if pluker or k != "ls_NDc"})
            res.append(r)
        return res


# ---- keyframe-to-keyframe association (plba_kfassoc_params / _batch / _out / plba_kf_associate)
class PlbaKfassocParams(C.Structure):
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("fast_matching", C.c_int32), ("ws", C.c_int32), ("best_lr", C.c_int32), ("min_pt_matches", C.c_int32),
                ("min_ls_matches", C.c_int32), ("line_query_in_grid_units", C.c_int32),
                ("min_ratio_12_p", C.c_double), ("min_ratio_12_l", C.c_double), ("line_sim_th", C.c_double),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class PlbaKfassocBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc_bytes", C.c_int32), ("pt_off_p", _ip), ("pt_off_c", _ip), ("ls_off_p", _ip),
                ("ls_off_c", _ip), ("DT", _dp), ("T_prev", _dp), ("T_curr", _dp), ("Tcw_prev", _dp), ("Tcw_curr", _dp),
                ("pt_P_p", _dp), ("pdesc_p", _bp), ("ls_sP_p", _dp), ("ls_eP_p", _dp), ("ls_NDc_p", _dp),
                ("ls_spl_p", _dp), ("ls_epl_p", _dp), ("ldesc_p", _bp), ("ls_lm_NDw", _dp), ("ls_new", _bp),
                ("pt_pl_c", _dp), ("pt_P_c", _dp), ("pdesc_c", _bp), ("ls_spl_c", _dp), ("ls_epl_c", _dp),
                ("ldesc_c", _bp)]


class PlbaKfassocOut(C.Structure):
    _fields_ = [("n_grid", _ip), ("n_matches", _ip), ("fallback", _ip), ("pt_m12", _ip), ("ls_m12", _ip),
                ("pt_rec", _dp), ("ls_rec", _dp), ("ls_rejected", _bp)]


def kfassoc_params(params=None) -> PlbaKfassocParams:
    """PlbaKfassocParams from a dict: plba_kfassoc_default_params, then the dict's entries (width, height,
    fx, fy, cx and cy have no default)."""
    if isinstance(params, PlbaKfassocParams):
        return params
    from . import lib   # lib imports this module
    p = PlbaKfassocParams()
    lib.load().plba_kfassoc_default_params(C.byref(p))
    for k, v in dict(params or {}).items():
        if k not in dict(PlbaKfassocParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class KfassocBatchView:
    """Concatenates keyframe pairs into contiguous arrays, the PlbaKfassocBatch over them and the output
    arrays of a call. A pair is a dict: DT [3][4], T_prev / T_curr / Tcw_prev / Tcw_curr [4][4]; of the previous
    keyframe pt_P_p [n][3], pdesc_p, ls_sP_p, ls_eP_p [n][3], ls_NDc_p [n][6], ls_spl_p, ls_epl_p [n][2], ldesc_p,
    ls_lm_NDw [n][6], ls_new [n] uint8; of the current one pt_pl_c [n][2], pt_P_c [n][3], pdesc_c, ls_spl_c,
    ls_epl_c [n][2], ldesc_c. A missing feature key is an empty side."""

    # key: (columns, dtype, the side's row-count key)
    ROWS = (("pt_P_p", 3, "pt_p"), ("ls_sP_p", 3, "ls_p"), ("ls_eP_p", 3, "ls_p"), ("ls_NDc_p", 6, "ls_p"),
            ("ls_spl_p", 2, "ls_p"), ("ls_epl_p", 2, "ls_p"), ("ls_lm_NDw", 6, "ls_p"), ("pt_pl_c", 2, "pt_c"),
            ("pt_P_c", 3, "pt_c"), ("ls_spl_c", 2, "ls_c"), ("ls_epl_c", 2, "ls_c"))
    DESC = (("pdesc_p", "pt_p"), ("ldesc_p", "ls_p"), ("pdesc_c", "pt_c"), ("ldesc_c", "ls_c"))
    LEAD = {"pt_p": "pt_P_p", "ls_p": "ls_sP_p", "pt_c": "pt_pl_c", "ls_c": "ls_spl_c"}
    POSES = (("DT", 12), ("T_prev", 16), ("T_curr", 16), ("Tcw_prev", 16), ("Tcw_curr", 16))

    def __init__(self, pairs, desc_bytes=None):
        pairs = list(pairs)
        if desc_bytes is None:
            desc_bytes = next((np.asarray(f[k]).shape[1] for f in pairs for k, _ in self.DESC
                               if k in f and np.asarray(f[k]).ndim == 2 and np.asarray(f[k]).shape[1]), 32)
        self.desc_bytes = db = int(desc_bytes)
        self.n = n = len(pairs)
        cnt = {s: [len(np.asarray(f.get(k, np.zeros((0, 1))))) for f in pairs] for s, k in self.LEAD.items()}
        self.off = {}
        for s, c in cnt.items():
            self.off[s] = np.zeros(n + 1, np.int32)
            self.off[s][1:] = np.cumsum(c, dtype=np.int64)
        self.a = {}

        def cat(key, per, dtype, side):
            parts = [np.asarray(f.get(key, np.zeros((0, per))), dtype).reshape(-1, per) for f in pairs]
            if [len(p) for p in parts] != cnt[side]:
                raise ValueError(f"{key}: one row per feature")
            return np.ascontiguousarray(np.concatenate(parts + [np.zeros((0, per), dtype)]))

        for key, per, side in self.ROWS:
            self.a[key] = cat(key, per, np.float64, side)
        for key, side in self.DESC:
            self.a[key] = cat(key, db, np.uint8, side)
        self.a["ls_new"] = cat("ls_new", 1, np.uint8, "ls_p")
        for key, per in self.POSES:
            self.a[key] = np.ascontiguousarray(
                np.concatenate([np.asarray(f[key], np.float64).reshape(1, per) for f in pairs] + [np.zeros((0, per))]))
        kinds = {np.dtype(np.int32): _ip, np.dtype(np.float64): _dp, np.dtype(np.uint8): _bp}
        self.struct = PlbaKfassocBatch(
            n=n, desc_bytes=db, pt_off_p=_ptr(self.off["pt_p"], _ip), pt_off_c=_ptr(self.off["pt_c"], _ip),
            ls_off_p=_ptr(self.off["ls_p"], _ip), ls_off_c=_ptr(self.off["ls_c"], _ip),
            **{k: _ptr(v, kinds[v.dtype]) for k, v in self.a.items()})
        npt, nls, P = max(int(self.off["pt_p"][-1]), 1), max(int(self.off["ls_p"][-1]), 1), max(2 * n, 1)
        # every row is written: a fill that no result can equal shows one that was not
        self.o = dict(n_grid=np.full(P, -7, np.int32), n_matches=np.full(P, -7, np.int32), fallback=np.full(P, -7, np.int32),
                      pt_m12=np.full(npt, -7, np.int32), ls_m12=np.full(nls, -7, np.int32),
                      pt_rec=np.full((npt, 9), np.nan), ls_rec=np.full((nls, 8), np.nan),
                      ls_rejected=np.full(nls, 7, np.uint8))
        self.out = PlbaKfassocOut(**{k: v.ctypes.data_as(kinds[v.dtype]) for k, v in self.o.items()})

    def results(self) -> list:
        """One dict per pair: n_grid, n_matches, fallback as (points, lines), and the previous rows' pt_m12,
        pt_rec, ls_m12, ls_rec, ls_rejected, copied."""
        res = []
        for f in range(self.n):
            a, b = self.off["pt_p"][f:f + 2]
            c, d = self.off["ls_p"][f:f + 2]
            r = {k: (int(self.o[k][2 * f]), int(self.o[k][2 * f + 1])) for k in ("n_grid", "n_matches", "fallback")}
            r.update(pt_m12=self.o["pt_m12"][a:b].copy(), pt_rec=self.o["pt_rec"][a:b].copy(),
                     ls_m12=self.o["ls_m12"][c:d].copy(), ls_rec=self.o["ls_rec"][c:d].copy(),
                     ls_rejected=self.o["ls_rejected"][c:d].copy())
            res.append(r)
        return res


# ---- map-to-keyframe association (plba_mapassoc_params / _batch / _out / plba_map_associate)
class PlbaMapassocParams(C.Structure):
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("fast_matching", C.c_int32), ("ws", C.c_int32), ("best_lr", C.c_int32), ("min_pt_matches", C.c_int32),
                ("min_ls_matches", C.c_int32), ("pad", C.c_int32),
                ("min_ratio_12_p", C.c_double), ("min_ratio_12_l", C.c_double), ("line_sim_th", C.c_double),
                ("max_kf_epip_p", C.c_double), ("max_kf_epip_l", C.c_double),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class PlbaMapassocBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc_bytes", C.c_int32), ("pt_off_m", _ip), ("pt_off_f", _ip), ("ls_off_m", _ip),
                ("ls_off_f", _ip), ("Twf", _dp), ("T_kf_w", _dp), ("pt_X", _dp), ("pdesc_m", _bp), ("ls_X", _dp),
                ("ldesc_m", _bp), ("pt_pl", _dp), ("pt_P", _dp), ("pdesc_f", _bp), ("ls_spl", _dp), ("ls_epl", _dp),
                ("ls_le", _dp), ("ls_sP", _dp), ("ls_eP", _dp), ("ldesc_f", _bp)]


class PlbaMapassocOut(C.Structure):
    _fields_ = [("n_visible", _ip), ("n_grid", _ip), ("n_matches", _ip), ("fallback", _ip), ("n_accepted", _ip),
                ("pt_visible", _bp), ("pt_m12", _ip), ("pt_accepted", _bp), ("pt_rec", _dp),
                ("ls_visible", _bp), ("ls_m12", _ip), ("ls_accepted", _bp), ("ls_rec", _dp)]


def mapassoc_params(params=None, **kw) -> PlbaMapassocParams:
    """PlbaMapassocParams from a dict and / or keywords: plba_mapassoc_default_params, then the entries
    (width, height, fx, fy, cx and cy have no default)."""
    if isinstance(params, PlbaMapassocParams) and not kw:
        return params
    from . import lib   # lib imports this module
    p = PlbaMapassocParams()
    lib.load().plba_mapassoc_default_params(C.byref(p))
    for k, v in {**dict(params or {}), **kw}.items():
        if k not in dict(PlbaMapassocParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class MapassocBatchView:
    """Concatenates keyframes into contiguous arrays, the PlbaMapassocBatch over them and the output arrays
    of a call. A keyframe is a dict: Twf [3][4], T_kf_w [4][4]; of the candidate landmarks pt_X [n][3], pdesc_m,
    ls_X [n][6] (line3D), ldesc_m; of the unmatched features pt_pl [n][2], pt_P [n][3], pdesc_f, ls_spl, ls_epl
    [n][2], ls_le, ls_sP, ls_eP [n][3], ldesc_f. A missing row key is an empty side."""

    # key: (columns, the side's row-count key)
    ROWS = (("pt_X", 3, "pt_m"), ("ls_X", 6, "ls_m"), ("pt_pl", 2, "pt_f"), ("pt_P", 3, "pt_f"), ("ls_spl", 2, "ls_f"),
            ("ls_epl", 2, "ls_f"), ("ls_le", 3, "ls_f"), ("ls_sP", 3, "ls_f"), ("ls_eP", 3, "ls_f"))
    DESC = (("pdesc_m", "pt_m"), ("ldesc_m", "ls_m"), ("pdesc_f", "pt_f"), ("ldesc_f", "ls_f"))
    LEAD = {"pt_m": "pt_X", "ls_m": "ls_X", "pt_f": "pt_pl", "ls_f": "ls_spl"}
    POSES = (("Twf", 12), ("T_kf_w", 16))

    def __init__(self, problems, desc_bytes=None):
        problems = list(problems)
        if desc_bytes is None:
            desc_bytes = next((np.asarray(f[k]).shape[1] for f in problems for k, _ in self.DESC
                               if k in f and np.asarray(f[k]).ndim == 2 and np.asarray(f[k]).shape[1]), 32)
        self.desc_bytes = db = int(desc_bytes)
        self.n = n = len(problems)
        cnt = {s: [len(np.asarray(f.get(k, np.zeros((0, 1))))) for f in problems] for s, k in self.LEAD.items()}
        self.off = {}
        for s, c in cnt.items():
            self.off[s] = np.zeros(n + 1, np.int32)
            self.off[s][1:] = np.cumsum(c, dtype=np.int64)
        self.a = {}

        def cat(key, per, dtype, side):
            parts = [np.asarray(f.get(key, np.zeros((0, per))), dtype).reshape(-1, per) for f in problems]
            if [len(p) for p in parts] != cnt[side]:
                raise ValueError(f"{key}: one row per landmark or feature")
            return np.ascontiguousarray(np.concatenate(parts + [np.zeros((0, per), dtype)]))

        for key, per, side in self.ROWS:
            self.a[key] = cat(key, per, np.float64, side)
        for key, side in self.DESC:
            self.a[key] = cat(key, db, np.uint8, side)
        for key, per in self.POSES:
            self.a[key] = np.ascontiguousarray(
                np.concatenate([np.asarray(f[key], np.float64).reshape(-1)[:per].reshape(1, per) for f in problems] +
                               [np.zeros((0, per))]))
        kinds = {np.dtype(np.int32): _ip, np.dtype(np.float64): _dp, np.dtype(np.uint8): _bp}
        self.struct = PlbaMapassocBatch(
            n=n, desc_bytes=db, pt_off_m=_ptr(self.off["pt_m"], _ip), pt_off_f=_ptr(self.off["pt_f"], _ip),
            ls_off_m=_ptr(self.off["ls_m"], _ip), ls_off_f=_ptr(self.off["ls_f"], _ip),
            **{k: _ptr(v, kinds[v.dtype]) for k, v in self.a.items()})
        npt, nls, P = max(int(self.off["pt_m"][-1]), 1), max(int(self.off["ls_m"][-1]), 1), max(2 * n, 1)
        # every row is written: a fill that no result can equal shows one that was not
        self.o = {k: np.full(P, -7, np.int32) for k in self.COUNTS}
        self.o.update(pt_visible=np.full(npt, 7, np.uint8), pt_m12=np.full(npt, -7, np.int32),
                      pt_accepted=np.full(npt, 7, np.uint8), pt_rec=np.full((npt, 6), np.nan),
                      ls_visible=np.full(nls, 7, np.uint8), ls_m12=np.full(nls, -7, np.int32),
                      ls_accepted=np.full(nls, 7, np.uint8), ls_rec=np.full((nls, 9), np.nan))
        self.out = PlbaMapassocOut(**{k: v.ctypes.data_as(kinds[v.dtype]) for k, v in self.o.items()})

    COUNTS = ("n_visible", "n_grid", "n_matches", "fallback", "n_accepted")
    PT = ("pt_visible", "pt_m12", "pt_accepted", "pt_rec")
    LS = ("ls_visible", "ls_m12", "ls_accepted", "ls_rec")

    def results(self) -> list:
        """One dict per keyframe: n_visible, n_grid, n_matches, fallback, n_accepted as (points, lines), and the
        candidate rows' pt_visible, pt_m12, pt_accepted, pt_rec, ls_visible, ls_m12, ls_accepted, ls_rec, copied."""
        res = []
        for f in range(self.n):
            a, b = self.off["pt_m"][f:f + 2]
            c, d = self.off["ls_m"][f:f + 2]
            r = {k: (int(self.o[k][2 * f]), int(self.o[k][2 * f + 1])) for k in self.COUNTS}
            r.update({k: self.o[k][a:b].copy() for k in self.PT})
            r.update({k: self.o[k][c:d].copy() for k in self.LS})
            res.append(r)
        return res
