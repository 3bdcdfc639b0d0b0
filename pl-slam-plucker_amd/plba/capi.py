"""ctypes mirror of include/plba.h (structs only; no library is loaded here)."""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from .synth import Graph

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_bp = C.POINTER(C.c_uint8)
_fp = C.POINTER(C.c_float)


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


# ---- the batched calls: one base for their views, one constructor for their params
_KINDS = {np.dtype(np.int32): _ip, np.dtype(np.float32): _fp, np.dtype(np.float64): _dp, np.dtype(np.uint8): _bp}
_F8, _F4, _U1, _I4 = np.float64, np.float32, np.uint8, np.int32
DESC = None                     # in a table, a column count of desc_bytes
_LEFT_OUT = np.zeros((0, 0))    # the rows of a key that a dict-style problem leaves out


def _field(q, key, default=None):
    """An array of a problem: the entry of a dict (``default`` where the key is left out) or the attribute of an object."""
    if not isinstance(q, dict):
        return getattr(q, key)
    return q[key] if default is None else q.get(key, default)


def _params_from(struct_cls, default_fn_name, params=None, **kw):
    """``params`` itself if it is a struct_cls already; else the library's defaults, then the entries of the
    dict ``params`` and the keywords (KeyError for a name that is no field)."""
    if isinstance(params, struct_cls) and not kw:
        return params
    from . import lib   # lib imports this module
    p = struct_cls()
    getattr(lib.load(), default_fn_name)(C.byref(p))
    for k, v in {**dict(params or {}), **kw}.items():
        if k not in dict(struct_cls._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class _BatchView:
    """Concatenates the problems of a batch into contiguous arrays, fills the batch struct over them and
    allocates the output arrays of a call. A view class declares the tables, with the struct's field names:

    SIDES  (key, the field of its [n+1] int32 offsets): the kinds of rows that a problem has.
    ROWS   (field, columns, dtype, side): one row per feature, the problems' rows one after the other. The
           first array of a side leads: every other one has its row count in every problem.
    PER    (field, width): float64, one row per problem.
    OUT    (field of OUT_STRUCT, side or "n" or "2n", trailing shape, dtype, fill): one row per row of the
           side, per problem or per half problem (points, lines), holding ``fill`` until a call writes it.

    A problem is a dict, where a row key left out is an empty side, or an object. Every array that a struct
    points to stays referenced: off[side], a[field] and o[field], each also an attribute under its field's name."""
    STRUCT = OUT_STRUCT = None
    SIDES = ROWS = PER = OUT = ()
    SHORT = "{key}: one row per feature"
    CAMERA = None   # what the message calls the problems ("pairs") if each has a .cam that one batch shares

    def _build(self, problems, desc_bytes=None, **scalars):
        problems = list(problems)
        self.n = n = len(problems)
        if desc_bytes is None:
            desc_bytes = self._desc_width(problems, 32)
        self.desc_bytes = db = int(desc_bytes)
        self.a, self.off, self.o, cnt = {}, {}, {}, {}
        for key, per, dtype, side in self.ROWS:
            per = db if per is DESC else per
            parts = [np.asarray(_field(q, key, _LEFT_OUT), dtype).reshape(-1, per) for q in problems]
            rows = [len(p) for p in parts]
            if rows != cnt.setdefault(side, rows):
                raise ValueError(self.SHORT.format(key=key, rows=sum(rows), lead=sum(cnt[side])))
            # (the row of no length: an empty batch still has an address)
            self.a[key] = np.ascontiguousarray(np.concatenate(parts + [np.zeros((0, per), dtype)]))
        for side, _ in self.SIDES:
            self.off[side] = np.zeros(n + 1, np.int32)
            self.off[side][1:] = np.cumsum(cnt[side], dtype=np.int64)
        for key, per in self.PER:
            parts = [np.asarray(_field(q, key), np.float64).reshape(-1, per) for q in problems]
            self.a[key] = np.ascontiguousarray(np.concatenate(parts + [np.zeros((0, per))]))
            if len(self.a[key]) != n:
                raise ValueError(f"{key}: {per} values per problem")
        if self.CAMERA:
            cam = problems[0].cam if problems else (1.0, 1.0, 0.0, 0.0)
            if any(tuple(q.cam) != tuple(cam) for q in problems):
                raise ValueError(f"the {self.CAMERA} of one batch share one camera")
            scalars.update(zip(("fx", "fy", "cx", "cy"), cam))
        if hasattr(self.STRUCT, "desc_bytes"):
            scalars["desc_bytes"] = db
        named = {**{f: self.off[s] for s, f in self.SIDES}, **self.a}
        self.struct = self.STRUCT(n=n, **scalars, **{k: _ptr(v, _KINDS[v.dtype]) for k, v in named.items()})
        for key, side, shape, dtype, fill in self.OUT:
            rows = n if side == "n" else 2 * n if side == "2n" else int(self.off[side][-1])
            self.o[key] = np.full((max(rows, 1),) + tuple(db if s is DESC else s for s in shape), fill, dtype)
        if self.OUT_STRUCT is not None:
            self.out = self.out_struct = self.OUT_STRUCT(**{k: _ptr(v, _KINDS[v.dtype]) for k, v in self.o.items()})

    def _desc_width(self, problems, default):
        """The width of the first 2-D descriptor array that has one."""
        found = (np.asarray(_field(q, key, _LEFT_OUT)) for q in problems for key, per, _, _ in self.ROWS if per is DESC)
        return next((d.shape[1] for d in found if d.ndim == 2 and d.shape[1]), default)

    def __getattr__(self, name):
        d = self.__dict__
        for side, field in self.SIDES:
            if field == name and side in d.get("off", ()):
                return d["off"][side]
        for table in ("a", "o"):
            if name in d.get(table, ()):
                return d[table][name]
        raise AttributeError(name)

    def results(self) -> list:
        """One dict per problem, every output under its field's name: the rows of the problem's side, copied;
        the int of a per-problem output; the (points, lines) ints of a per-half-problem one."""
        res = []
        for f in range(self.n):
            r = {}
            for key, side, *_ in self.OUT:
                if side == "n":
                    r[key] = int(self.o[key][f])
                elif side == "2n":
                    r[key] = (int(self.o[key][2 * f]), int(self.o[key][2 * f + 1]))
                else:
                    r[key] = self.o[key][self.off[side][f]:self.off[side][f + 1]].copy()
            res.append(r)
        return res


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


class LcposeBatchView(_BatchView):
    """The PlbaLcposeBatch over candidate pairs (objects with pt_P, pt_obs, ln_sP, ln_eP, ln_le and cam, e.g.
    plba.lcpose.LcProblem)."""
    STRUCT = PlbaLcposeBatch
    SIDES = (("pt", "pt_off"), ("ln", "ln_off"))
    ROWS = (("pt_P", 3, _F8, "pt"), ("pt_obs", 2, _F8, "pt"), ("ln_sP", 3, _F8, "ln"), ("ln_eP", 3, _F8, "ln"),
            ("ln_le", 3, _F8, "ln"))
    SHORT = "{key}: one row per match"
    CAMERA = "candidates"

    def __init__(self, problems):
        self._build(problems)


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


class TrackBatchView(_BatchView):
    """The PlbaTrackBatch over frame pairs (objects with the arrays of plba.trackpose.TrackProblem)."""
    FIELDS = (("pt_P", 3), ("pt_obs", 2), ("pt_sigma2", 1), ("ln_sP", 3), ("ln_eP", 3), ("ln_NDc", 6), ("ln_le", 3),
              ("ln_obs", 4), ("ln_seg", 4), ("ln_sigma2", 1))
    STRUCT = PlbaTrackBatch
    SIDES = LcposeBatchView.SIDES
    ROWS = tuple((name, w, _F8, name[:2]) for name, w in FIELDS)
    PER = (("prev", TRACK_PREV),)
    SHORT = LcposeBatchView.SHORT
    CAMERA = "problems"

    def __init__(self, problems):
        self._build(problems)


def track_out_to_dict(o: PlbaTrackOut, pt_inlier, ln_inlier) -> dict:
    return dict(branch=int(o.branch), iters_first=int(o.iters_first), iters_ref=int(o.iters_ref),
                n_inl_pt=int(o.n_inl_pt), n_inl_ln=int(o.n_inl_ln), err_norm=float(o.err_norm),
                s_p=float(o.s_p), s_l=float(o.s_l), DT=np.array(o.DT[:]).reshape(4, 4),
                DT_cov=np.array(o.DT_cov[:]).reshape(6, 6), DT_cov_eig=np.array(o.DT_cov_eig[:]),
                DT_solver=np.array(o.DT_solver[:]).reshape(4, 4), H=np.array(o.H[:]).reshape(6, 6),
                pt_inlier=np.array(pt_inlier, np.uint8), ln_inlier=np.array(ln_inlier, np.uint8))


# ---- descriptor matching (plba_match_batch / plba_desc_match)
class PlbaMatchBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc_bytes", C.c_int32), ("off1", _ip), ("off2", _ip), ("desc1", _bp),
                ("desc2", _bp), ("nnr", _fp), ("best_lr", C.c_int32), ("pad", C.c_int32)]


class MatchBatchView(_BatchView):
    """The PlbaMatchBatch over descriptor-set pairs [(desc1 [n1][desc_bytes] uint8, desc2 [n2][desc_bytes]), ...].
    ``nnr``: one ratio, or one per pair."""
    STRUCT = PlbaMatchBatch
    SIDES = (("1", "off1"), ("2", "off2"))
    ROWS = (("desc1", DESC, _U1, "1"), ("desc2", DESC, _U1, "2"))

    def __init__(self, pairs, nnr, best_lr: bool = True, desc_bytes=None):
        self._build([dict(desc1=a, desc2=b) for a, b in pairs], desc_bytes, best_lr=int(bool(best_lr)))
        self.nnr = np.ascontiguousarray(np.broadcast_to(np.asarray(nnr, np.float32), (self.n,)))
        self.struct.nnr = _ptr(self.nnr, _fp)


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


class FramesBatchView(_BatchView):
    """The PlbaFramesBatch over frame pairs (objects with the arrays of plba.trackframes.FramePair), and the
    output arrays with their PlbaFramesOut. The descriptors lead: every other array of a kind and side has
    their row count."""
    STRUCT, OUT_STRUCT = PlbaFramesBatch, PlbaFramesOut
    SIDES = (("pt1", "pt_off1"), ("pt2", "pt_off2"), ("ln1", "ln_off1"), ("ln2", "ln_off2"))
    ROWS = (("prev_pdesc", DESC, _U1, "pt1"), ("prev_ldesc", DESC, _U1, "ln1"), ("cur_pdesc", DESC, _U1, "pt2"),
            ("cur_ldesc", DESC, _U1, "ln2"), ("prev_pt_P", 3, _F8, "pt1"), ("prev_pt_sigma2", 1, _F8, "pt1"),
            ("prev_ln_sP", 3, _F8, "ln1"), ("prev_ln_eP", 3, _F8, "ln1"), ("prev_ln_NDc", 6, _F8, "ln1"),
            ("prev_ln_seg", 4, _F8, "ln1"), ("prev_ln_sigma2", 1, _F8, "ln1"), ("cur_pt_pl", 2, _F8, "pt2"),
            ("cur_ln_seg", 4, _F8, "ln2"), ("cur_ln_le", 3, _F8, "ln2"))
    PER = (("prev", TRACK_PREV),)
    OUT = (("pt_m12", "pt1", (), _I4, -1), ("ln_m12", "ln1", (), _I4, -1), ("n_pt", "n", (), _I4, 0),
           ("n_ln", "n", (), _I4, 0), ("pt_inlier", "pt1", (), _U1, 0), ("ln_inlier", "ln1", (), _U1, 0),
           ("pt_cur_from_prev", "pt2", (), _I4, -1), ("ln_cur_from_prev", "ln2", (), _I4, -1))
    SHORT = "{key} has {rows} rows, the descriptors have {lead}"
    CAMERA = "pairs"

    def __init__(self, pairs, desc_bytes=32):
        pairs = list(pairs)
        # (2-D descriptors keep their rows: their own width is the caller's claim, desc_bytes cuts the flat ones)
        self._build(pairs, self._desc_width(pairs, desc_bytes))
        self.out = self.out_struct.out = (PlbaTrackOut * max(self.n, 1))()   # (here .out is not the out struct)

    def results(self) -> list:
        """One dict per pair: the fields of track_out_to_dict (the inlier flags per PREVIOUS row) and pt_m12,
        ln_m12, n_pt, n_ln, pt_cur_from_prev, ln_cur_from_prev."""
        res = super().results()
        for k, r in enumerate(res):
            r.update(track_out_to_dict(self.out[k], r.pop("pt_inlier"), r.pop("ln_inlier")))
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


class GridMatchBatchView(_BatchView):
    """The PlbaGridMatchBatch over matchGrid problems.
    A problem is a dict: kind (0 points, 1 lines), ws, nnr, line_sim_th (lines), desc1 [n1][desc_bytes]
    uint8, cell1 [n1][2] int, cell1_end [n1][2] (lines), desc2 [n2][desc_bytes], cells2 (one [k][2] int
    array per train row) and dir2 [n2][2] (lines)."""
    STRUCT, SIDES, ROWS = PlbaGridMatchBatch, MatchBatchView.SIDES, MatchBatchView.ROWS

    def __init__(self, problems, cols: int = 64, rows: int = 48, best_lr: bool = True, desc_bytes=None):
        problems = list(problems)
        self._build(problems, desc_bytes, cols=int(cols), rows=int(rows), best_lr=int(bool(best_lr)))
        n, n1, n2 = self.n, int(self.off1[-1]), int(self.off2[-1])
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
            if len(p["cells2"]) != self.off2[k + 1] - self.off2[k]:
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
        for k in ("cell1", "cell1_end", "cell_off2", "cells2", "dir2", "kind", "ws", "nnr", "line_sim_th"):
            v = getattr(self, k)
            setattr(self.struct, k, _ptr(v, _KINDS[v.dtype]))


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
    return _params_from(PlbaStereoParams, "plba_stereo_default_params", params)


class StereoBatchView(_BatchView):
    """The PlbaStereoBatch over stereo frames and the output arrays of a call (.o, .out). A frame is a dict:
    pt_l [n][2] / pt_r float32, pdesc_l / pdesc_r [n][desc_bytes] uint8, ls_l / ls_r [n][4] float32 (sx, sy, ex, ey),
    ldesc_l / ldesc_r; a missing key is an empty side. .co[side] and .desc[side] are a side's coordinates and
    descriptors."""
    STRUCT, OUT_STRUCT = PlbaStereoBatch, PlbaStereoOut
    SIDES = (("pt_l", "pt_off_l"), ("pt_r", "pt_off_r"), ("ls_l", "ls_off_l"), ("ls_r", "ls_off_r"))
    ROWS = (("pt_l", 2, _F4, "pt_l"), ("pdesc_l", DESC, _U1, "pt_l"), ("pt_r", 2, _F4, "pt_r"), ("pdesc_r", DESC, _U1, "pt_r"),
            ("ls_l", 4, _F4, "ls_l"), ("ldesc_l", DESC, _U1, "ls_l"), ("ls_r", 4, _F4, "ls_r"), ("ldesc_r", DESC, _U1, "ls_r"))
    # rows past a frame's count are never written: a fill that no result can equal shows it
    OUT = (("n_pt", "n", (), _I4, 0), ("n_ls", "n", (), _I4, 0),
           ("pt_src", "pt_l", (), _I4, -7), ("pt_pl", "pt_l", (2,), _F8, np.nan), ("pt_disp", "pt_l", (), _F8, np.nan),
           ("pt_P", "pt_l", (3,), _F8, np.nan), ("pdesc", "pt_l", (DESC,), _U1, 0),
           ("ls_src", "ls_l", (), _I4, -7), ("ls_spl", "ls_l", (2,), _F8, np.nan), ("ls_epl", "ls_l", (2,), _F8, np.nan),
           ("ls_sdisp", "ls_l", (), _F8, np.nan), ("ls_edisp", "ls_l", (), _F8, np.nan), ("ls_sP", "ls_l", (3,), _F8, np.nan),
           ("ls_eP", "ls_l", (3,), _F8, np.nan), ("ls_le", "ls_l", (3,), _F8, np.nan), ("ls_NDc", "ls_l", (6,), _F8, np.nan),
           ("ldesc", "ls_l", (DESC,), _U1, 0))
    SHORT = "one descriptor row per feature"

    def __init__(self, frames, desc_bytes=None):
        self._build(frames, desc_bytes)
        self.co = {side: self.a[side] for side, _ in self.SIDES}
        self.desc = {side: self.a[key] for key, per, _, side in self.ROWS if per is DESC}

    def results(self, pluker: bool) -> list:
        """One dict per frame: n_pt, n_ls and the first n_pt / n_ls rows of every output array (ls_NDc only
        with pluker), copied."""
        res = super().results()
        for r in res:
            for key, side, *_ in self.OUT[2:]:
                r[key] = r[key][:r["n_pt" if side == "pt_l" else "n_ls"]]
            if not pluker:
                del r["ls_NDc"]
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
    return _params_from(PlbaKfassocParams, "plba_kfassoc_default_params", params)


class KfassocBatchView(_BatchView):
    """The PlbaKfassocBatch over keyframe pairs and the output arrays of a call (.o, .out). A pair is a dict:
    DT [3][4], T_prev / T_curr / Tcw_prev / Tcw_curr [4][4]; of the previous
    keyframe pt_P_p [n][3], pdesc_p, ls_sP_p, ls_eP_p [n][3], ls_NDc_p [n][6], ls_spl_p, ls_epl_p [n][2], ldesc_p,
    ls_lm_NDw [n][6], ls_new [n] uint8; of the current one pt_pl_c [n][2], pt_P_c [n][3], pdesc_c, ls_spl_c,
    ls_epl_c [n][2], ldesc_c. A missing feature key is an empty side. results(): one dict per pair with n_grid,
    n_matches, fallback as (points, lines), and the previous rows' pt_m12, pt_rec, ls_m12, ls_rec, ls_rejected."""
    STRUCT, OUT_STRUCT = PlbaKfassocBatch, PlbaKfassocOut
    SIDES = (("pt_p", "pt_off_p"), ("pt_c", "pt_off_c"), ("ls_p", "ls_off_p"), ("ls_c", "ls_off_c"))
    ROWS = (("pt_P_p", 3, _F8, "pt_p"), ("ls_sP_p", 3, _F8, "ls_p"), ("ls_eP_p", 3, _F8, "ls_p"), ("ls_NDc_p", 6, _F8, "ls_p"),
            ("ls_spl_p", 2, _F8, "ls_p"), ("ls_epl_p", 2, _F8, "ls_p"), ("ls_lm_NDw", 6, _F8, "ls_p"),
            ("pt_pl_c", 2, _F8, "pt_c"), ("pt_P_c", 3, _F8, "pt_c"), ("ls_spl_c", 2, _F8, "ls_c"), ("ls_epl_c", 2, _F8, "ls_c"),
            ("pdesc_p", DESC, _U1, "pt_p"), ("ldesc_p", DESC, _U1, "ls_p"), ("pdesc_c", DESC, _U1, "pt_c"),
            ("ldesc_c", DESC, _U1, "ls_c"), ("ls_new", 1, _U1, "ls_p"))
    PER = (("DT", 12), ("T_prev", 16), ("T_curr", 16), ("Tcw_prev", 16), ("Tcw_curr", 16))
    # every row is written: a fill that no result can equal shows one that was not
    OUT = (("n_grid", "2n", (), _I4, -7), ("n_matches", "2n", (), _I4, -7), ("fallback", "2n", (), _I4, -7),
           ("pt_m12", "pt_p", (), _I4, -7), ("pt_rec", "pt_p", (9,), _F8, np.nan), ("ls_m12", "ls_p", (), _I4, -7),
           ("ls_rec", "ls_p", (8,), _F8, np.nan), ("ls_rejected", "ls_p", (), _U1, 7))

    def __init__(self, pairs, desc_bytes=None):
        self._build(pairs, desc_bytes)


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
    return _params_from(PlbaMapassocParams, "plba_mapassoc_default_params", params, **kw)


class MapassocBatchView(_BatchView):
    """The PlbaMapassocBatch over keyframes and the output arrays of a call (.o, .out). A keyframe is a dict:
    Twf [3][4] (or [4][4]: its first three rows), T_kf_w [4][4]; of the candidate landmarks pt_X [n][3], pdesc_m,
    ls_X [n][6] (line3D), ldesc_m; of the unmatched features pt_pl [n][2], pt_P [n][3], pdesc_f, ls_spl, ls_epl
    [n][2], ls_le, ls_sP, ls_eP [n][3], ldesc_f. A missing row key is an empty side. results(): one dict per
    keyframe with n_visible, n_grid, n_matches, fallback, n_accepted as (points, lines), and the candidate rows'
    pt_visible, pt_m12, pt_accepted, pt_rec, ls_visible, ls_m12, ls_accepted, ls_rec."""
    STRUCT, OUT_STRUCT = PlbaMapassocBatch, PlbaMapassocOut
    SIDES = (("pt_m", "pt_off_m"), ("pt_f", "pt_off_f"), ("ls_m", "ls_off_m"), ("ls_f", "ls_off_f"))
    ROWS = (("pt_X", 3, _F8, "pt_m"), ("ls_X", 6, _F8, "ls_m"), ("pt_pl", 2, _F8, "pt_f"), ("pt_P", 3, _F8, "pt_f"),
            ("ls_spl", 2, _F8, "ls_f"), ("ls_epl", 2, _F8, "ls_f"), ("ls_le", 3, _F8, "ls_f"), ("ls_sP", 3, _F8, "ls_f"),
            ("ls_eP", 3, _F8, "ls_f"), ("pdesc_m", DESC, _U1, "pt_m"), ("ldesc_m", DESC, _U1, "ls_m"),
            ("pdesc_f", DESC, _U1, "pt_f"), ("ldesc_f", DESC, _U1, "ls_f"))
    PER = (("Twf", 12), ("T_kf_w", 16))
    # every row is written: a fill that no result can equal shows one that was not
    OUT = tuple((k, "2n", (), _I4, -7) for k in ("n_visible", "n_grid", "n_matches", "fallback", "n_accepted")) + (
        ("pt_visible", "pt_m", (), _U1, 7), ("pt_m12", "pt_m", (), _I4, -7), ("pt_accepted", "pt_m", (), _U1, 7),
        ("pt_rec", "pt_m", (6,), _F8, np.nan), ("ls_visible", "ls_m", (), _U1, 7), ("ls_m12", "ls_m", (), _I4, -7),
        ("ls_accepted", "ls_m", (), _U1, 7), ("ls_rec", "ls_m", (9,), _F8, np.nan))
    SHORT = "{key}: one row per landmark or feature"

    def __init__(self, problems, desc_bytes=None):
        self._build([{**f, "Twf": np.asarray(f["Twf"], np.float64).reshape(-1)[:12]} for f in problems], desc_bytes)
