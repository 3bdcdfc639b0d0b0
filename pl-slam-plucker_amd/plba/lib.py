"""ctypes binding of libplba.so (the HIP backend, C ABI of include/plba.h).

This is the product path: it fails loudly when the HIP library is missing or no GPU is
visible — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import capi
from .synth import Graph

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "libplba.so")

_lib = None

PLBA_ERRORS = {-1: "PLBA_E_INVALID", -2: "PLBA_E_DEVICE", -3: "PLBA_E_STATE", -4: "PLBA_E_NOMEM", -5: "PLBA_E_COMM"}

# int (*plba_host_allreduce_fn)(void *user, double *buf, int64_t n)
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)

# every function load() binds, with its argtypes. plba_default_opts and every *_default_params return void,
# plba_last_error a string, the others an int
_P, _vp, _i32 = C.POINTER, C.c_void_p, C.c_int32
_dp, _bp, _ip = _P(C.c_double), _P(C.c_uint8), _P(C.c_int32)
ARGTYPES = {
    "plba_default_opts": [_P(capi.PlbaOpts)],
    "plba_create": [_P(_vp), _P(capi.PlbaOpts)],
    "plba_destroy": [_vp],
    "plba_last_error": [_vp],
    "plba_upload": [_vp, _P(capi.PlbaGraph)],
    "plba_reset_estimates": [_vp],
    "plba_set_edge_levels": [_vp, _bp, _bp],
    "plba_set_robust": [_vp, _i32],
    "plba_initialize_optimization": [_vp, _i32],
    "plba_optimize": [_vp, _i32, _ip, _dp],
    "plba_refresh_edge_errors": [_vp, _i32],
    "plba_get_edge_chi2": [_vp, _dp, _bp, _dp],
    "plba_download": [_vp, _dp, _dp, _dp],
    "plba_lba_plucker": [_vp, _P(capi.PlbaResult)],
    "plba_get_trace": [_vp, _P(capi.PlbaIterTrace), _i32, _ip],
    "plba_synchronize": [_vp],
    "plba_enable_kernel_timing": [_vp, _i32],
    "plba_kernel_times": [_vp, _P(C.c_char_p), _dp, _ip, _i32, _ip],
    "plba_structure_stats": [_vp, _P(C.c_int64), _i32],
    "plba_shard_plan": [_P(capi.PlbaGraph), _i32, _ip, _ip],
    "plba_comm_unique_id": [_bp],
    "plba_comm_init_rccl": [_vp, _i32, _i32, _bp],
    "plba_comm_init_host": [_vp, _i32, _i32, HOST_ALLREDUCE_FN, _vp],
    "plba_comm_info": [_vp, _ip, _i32],
    "plba_factor_plan": [_i32, _i32, _i32, _i32, _ip, _i32],
    "plba_hlm_default_params": [_P(capi.PlbaHlmParams)],
    "plba_hlm_lba": [_vp, _P(capi.PlbaHlmState), _P(capi.PlbaHlmParams), _P(capi.PlbaHlmResult)],
    "plba_pgo_default_params": [_P(capi.PlbaPgoParams)],
    "plba_pgo_optimize": [_vp, _P(capi.PlbaPgoGraph), _P(capi.PlbaPgoParams), _P(capi.PlbaPgoResult)],
    "plba_lcpose_default_params": [_P(capi.PlbaLcposeParams)],
    "plba_lc_relative_pose": [_vp, _P(capi.PlbaLcposeBatch), _P(capi.PlbaLcposeParams), _P(capi.PlbaLcposeOut), _bp, _bp],
    "plba_track_default_params": [_P(capi.PlbaTrackParams)],
    "plba_track_pose": [_vp, _P(capi.PlbaTrackBatch), _P(capi.PlbaTrackParams), _P(capi.PlbaTrackOut), _bp, _bp],
    "plba_frames_default_params": [_P(capi.PlbaFramesParams)],
    "plba_track_frames": [_vp, _P(capi.PlbaFramesBatch), _P(capi.PlbaFramesParams), _P(capi.PlbaFramesOut)],
    "plba_desc_match": [_vp, _P(capi.PlbaMatchBatch), _ip, _ip],
    "plba_grid_match": [_vp, _P(capi.PlbaGridMatchBatch), _ip, _ip],
    "plba_stereo_default_params": [_P(capi.PlbaStereoParams)],
    "plba_stereo_associate": [_vp, _P(capi.PlbaStereoBatch), _P(capi.PlbaStereoParams), _P(capi.PlbaStereoOut)],
    "plba_kfassoc_default_params": [_P(capi.PlbaKfassocParams)],
    "plba_kf_associate": [_vp, _P(capi.PlbaKfassocBatch), _P(capi.PlbaKfassocParams), _P(capi.PlbaKfassocOut)],
    "plba_mapassoc_default_params": [_P(capi.PlbaMapassocParams)],
    "plba_map_associate": [_vp, _P(capi.PlbaMapassocBatch), _P(capi.PlbaMapassocParams), _P(capi.PlbaMapassocOut)],
    "plba_desc_medoid": [_vp, _P(capi.PlbaMedoidBatch), _ip],
    "plba_bow_set_vocab": [_vp, _i32, _P(capi.PlbaBowVocab)],
    "plba_bow_insert": [_vp, _i32, _i32, _bp, _i32, _dp, _ip, _i32, _ip],
    "plba_bow_remove": [_vp, _i32, _i32],
    "plba_bow_get": [_vp, _i32, _i32, _ip, _dp, _i32, _ip],
}
EXPORTED = list(ARGTYPES)


class PlbaError(RuntimeError):
    pass


def load(path: Optional[str] = None):
    """Load libplba.so (raises if it is missing — no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("PLBA_LIB") or LIB_PATH  # (PLBA_LIB: A/B builds of the same library)
    if not os.path.exists(path):
        raise PlbaError(f"libplba.so not found at {path}: run `make -C pl-slam-plucker_amd` "
                        "(or __graft_entry__.build()) first")
    L = C.CDLL(path)
    for name, argtypes in ARGTYPES.items():
        f = getattr(L, name)
        f.argtypes = argtypes
        void = name == "plba_default_opts" or name.endswith("_default_params")
        f.restype = None if void else C.c_char_p if name == "plba_last_error" else C.c_int
    _lib = L
    return L


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def shard_plan(g: Graph, nranks: int):
    """Landmark -> rank assignment of a sharded window (pure host code; no GPU needed)."""
    L = load()
    gv = capi.GraphView(g)
    po = np.zeros(max(g.n_pt, 1), np.int32)
    lo = np.zeros(max(g.n_ln, 1), np.int32)
    rc = L.plba_shard_plan(C.byref(gv.struct), nranks, _p(po, C.c_int32), _p(lo, C.c_int32))
    if rc != 0:
        raise PlbaError(f"plba_shard_plan failed: {PLBA_ERRORS.get(rc, rc)}")
    return po[:g.n_pt], lo[:g.n_ln]


def comm_unique_id() -> bytes:
    """RCCL unique id (create on rank 0, broadcast the 128 bytes)."""
    buf = (C.c_uint8 * 128)()
    rc = load().plba_comm_unique_id(buf)
    if rc != 0:
        raise PlbaError(f"plba_comm_unique_id failed: {PLBA_ERRORS.get(rc, rc)}")
    return bytes(buf)


class Solver:
    """One plba context bound to a device (g2o::SparseOptimizer equivalent)."""

    def __init__(self, device: int = 0, corrected_line_jacobian: bool = False, verbose: bool = False,
                 kernel_timing: bool = False, tau: Optional[float] = None, max_trials: Optional[int] = None):
        self.L = load()
        o = capi.PlbaOpts()
        self.L.plba_default_opts(C.byref(o))
        o.device = device
        o.corrected_line_jacobian = int(corrected_line_jacobian)
        o.verbose = int(verbose)
        if tau is not None:
            o.tau = float(tau)          # OptimizationAlgorithmLevenberg τ (λ init = τ·max|H_jj|)
        if max_trials is not None:
            o.max_trials = int(max_trials)
        self.ctx = C.c_void_p()
        rc = self.L.plba_create(C.byref(self.ctx), C.byref(o))
        if rc != 0:
            raise PlbaError(f"plba_create failed: {PLBA_ERRORS.get(rc, rc)} (no usable HIP device?)")
        self.graph: Optional[Graph] = None
        self._bow_live = {0: 0, 1: 0}   # live vectors per place-recognition slot: sizes bow_insert's outputs
        if kernel_timing:
            self._check(self.L.plba_enable_kernel_timing(self.ctx, 1), "plba_enable_kernel_timing")

    def _check(self, rc, what):
        if rc != 0:
            msg = self.L.plba_last_error(self.ctx).decode(errors="replace")
            raise PlbaError(f"{what} failed: {PLBA_ERRORS.get(rc, rc)}: {msg}")

    def close(self):
        if self.ctx:
            self.L.plba_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- sharded windows (call one of these before upload)
    def comm_init_rccl(self, nranks: int, rank: int, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.L.plba_comm_init_rccl(self.ctx, nranks, rank, buf), "plba_comm_init_rccl")

    def comm_init_host(self, nranks: int, rank: int, allreduce):
        """allreduce(np.ndarray[float64]) sums the array over ranks in place."""
        def tramp(user, buf, n):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(n,)))
                return 0
            except Exception:  # never unwind through C
                import traceback
                traceback.print_exc()
                return -1
        self._host_cb = HOST_ALLREDUCE_FN(tramp)
        self._check(self.L.plba_comm_init_host(self.ctx, nranks, rank, self._host_cb, None), "plba_comm_init_host")

    def comm_info(self) -> dict:
        """What the transport reports (plba_comm_info): RCCL's own rank count, rank and device, and
        the HIP device / PCI location this context runs on."""
        v = np.zeros(8, np.int32)
        self._check(self.L.plba_comm_info(self.ctx, _p(v, C.c_int32), 8), "plba_comm_info")
        return dict(transport={0: "none", 1: "rccl", 2: "host"}.get(int(v[0]), str(int(v[0]))),
                    ranks=int(v[1]), rank=int(v[2]), comm_device=int(v[3]), hip_device=int(v[4]),
                    pci=f"{int(v[5]):04x}:{int(v[6]):02x}:{int(v[7]):02x}" if v[5] >= 0 else None)

    # -- g2o-style calls
    def upload(self, g: Graph):
        self.graph = g
        gv = capi.GraphView(g)
        self._check(self.L.plba_upload(self.ctx, C.byref(gv.struct)), "plba_upload")

    def reset(self):
        self._check(self.L.plba_reset_estimates(self.ctx), "plba_reset_estimates")

    def set_edge_levels(self, ept_level, eln_level):
        a = np.ascontiguousarray(ept_level, np.uint8)
        b = np.ascontiguousarray(eln_level, np.uint8)
        self._check(self.L.plba_set_edge_levels(self.ctx, _p(a, C.c_uint8), _p(b, C.c_uint8)), "plba_set_edge_levels")

    def set_robust(self, on: bool):
        self._check(self.L.plba_set_robust(self.ctx, int(on)), "plba_set_robust")

    def initialize_optimization(self, level: int = 0):
        self._check(self.L.plba_initialize_optimization(self.ctx, level), "plba_initialize_optimization")

    def optimize(self, iterations: int):
        it = C.c_int32(0)
        chi = C.c_double(0)
        self._check(self.L.plba_optimize(self.ctx, iterations, C.byref(it), C.byref(chi)), "plba_optimize")
        return it.value, chi.value

    def refresh_edge_errors(self, level: int):
        self._check(self.L.plba_refresh_edge_errors(self.ctx, level), "plba_refresh_edge_errors")

    def edge_chi2(self):
        g = self.graph
        pc, pd, lc = np.zeros(g.n_ept), np.zeros(g.n_ept, np.uint8), np.zeros(g.n_eln)
        self._check(self.L.plba_get_edge_chi2(self.ctx, _p(pc), _p(pd, C.c_uint8), _p(lc)), "plba_get_edge_chi2")
        return pc, pd, lc

    def download(self):
        g = self.graph
        T, P, O = np.zeros((g.n_kf, 3, 4)), np.zeros((g.n_pt, 3)), np.zeros((g.n_ln, 4))
        self._check(self.L.plba_download(self.ctx, _p(T), _p(P), _p(O)), "plba_download")
        return T, P, O

    def lba_plucker(self, want_outputs: bool = True, with_trace: bool = True) -> dict:
        """Full two-stage schedule (src/mapHandler.cpp:6119-6160) on the uploaded window."""
        g = self.graph
        if want_outputs:
            rb = capi.ResultBuffers(g)
            self._check(self.L.plba_lba_plucker(self.ctx, C.byref(rb.struct)), "plba_lba_plucker")
            out = rb.as_dict()
        else:
            r = capi.PlbaResult()
            self._check(self.L.plba_lba_plucker(self.ctx, C.byref(r)), "plba_lba_plucker")
            out = dict(iters=np.array([r.iters[0], r.iters[1]]), chi2=np.array([r.chi2[0], r.chi2[1]]),
                       solve_ms=r.solve_ms)
        if with_trace:
            out["trace"] = self.trace()
        return out

    def hlm_lba(self, win, params=None, with_trace: bool = True) -> dict:
        """levMarquardtOptimizationLBAForPluker (src/mapHandler.cpp:1618-2332) on the uploaded window;
        ``params.variant`` selects levMarquardtOptimizationGBA (capi.gba_params) or the endpoint-line
        levMarquardtOptimizationLBA (capi.lba_params), whose lines come back as ``ln_line3d``.

        ``win`` is a plba.hlm.HlmWindow whose ``graph`` was uploaded with :meth:`upload`."""
        g = self.graph
        if params is None:
            params = capi.PlbaHlmParams()
            self.L.plba_hlm_default_params(C.byref(params))
        sv = capi.HlmStateView(win.kf_x, win.ln_pluker, getattr(win, "ln_line3d", None))
        rb = capi.HlmResultBuffers(g)
        self._check(self.L.plba_hlm_lba(self.ctx, C.byref(sv.struct), C.byref(params), C.byref(rb.struct)),
                    "plba_hlm_lba")
        out = rb.as_dict()
        if with_trace:
            out["trace"] = self.trace()
        return out

    def pgo_optimize(self, pg, params=None) -> dict:
        """Loop-closure pose graph (plba_pgo_optimize; src/mapHandler.cpp:5070-5531) of a
        plba.pgo.PoseGraph: computeInitialGuess + optimize on this context's device. Needs no
        uploaded window and leaves one intact."""
        if params is None:
            params = capi.PlbaPgoParams()
            self.L.plba_pgo_default_params(C.byref(params))
        gv = capi.PgoGraphView(pg)
        rb = capi.PgoResultBuffers(len(gv.v_id))
        self._check(self.L.plba_pgo_optimize(self.ctx, C.byref(gv.struct), C.byref(params), C.byref(rb.struct)),
                    "plba_pgo_optimize")
        return rb.as_dict()

    def _pose_batch(self, name, defaults, bv, params, params_cls, out_cls, to_dict) -> list:
        """The calls that give one ``out_cls`` per problem and an inlier flag per point and line row."""
        if params is None:
            params = params_cls()
            getattr(self.L, defaults)(C.byref(params))
        n = bv.struct.n
        out = (out_cls * max(n, 1))()
        pin = np.zeros(max(int(bv.pt_off[-1]), 1), np.uint8)
        lin = np.zeros(max(int(bv.ln_off[-1]), 1), np.uint8)
        self._check(getattr(self.L, name)(self.ctx, C.byref(bv.struct), C.byref(params), out, _p(pin, C.c_uint8),
                                          _p(lin, C.c_uint8)), name)
        return [to_dict(out[i], pin[bv.pt_off[i]:bv.pt_off[i + 1]], lin[bv.ln_off[i]:bv.ln_off[i + 1]]) for i in range(n)]

    def _match(self, name, bv) -> list:
        """The calls that give matches_12 per query row and a count per problem."""
        n = bv.struct.n
        m12 = np.full(max(int(bv.off1[-1]), 1), -1, np.int32)
        cnt = np.zeros(max(n, 1), np.int32)
        self._check(getattr(self.L, name)(self.ctx, C.byref(bv.struct), _p(m12, C.c_int32), _p(cnt, C.c_int32)), name)
        return [(m12[bv.off1[i]:bv.off1[i + 1]].copy(), int(cnt[i])) for i in range(n)]

    def _associate(self, name, view_cls, params_fn, problems, params, desc_bytes):
        """The calls over a view that holds its own outputs: (the view, the params struct) after the call."""
        bv = problems if isinstance(problems, view_cls) else view_cls(problems, desc_bytes)
        prm = params_fn(params)
        self._check(getattr(self.L, name)(self.ctx, C.byref(bv.struct), C.byref(prm), C.byref(bv.out)), name)
        return bv, prm

    def lc_relative_pose(self, problems, params=None) -> list:
        """Loop-closure relative pose (plba_lc_relative_pose; computeRelativePoseRobustGN /
        computeRelativePoseGN, src/mapHandler.cpp:4677-5068 / :4413-4675) of a batch of candidate
        pairs (plba.lcpose.LcProblem), verified in one launch. One dict per candidate, with its
        inlier flags. Needs no uploaded window and leaves one intact."""
        return self._pose_batch("plba_lc_relative_pose", "plba_lcpose_default_params", capi.LcposeBatchView(problems),
                                params, capi.PlbaLcposeParams, capi.PlbaLcposeOut, capi.lcpose_out_to_dict)

    def track_pose(self, problems, params=None) -> list:
        """Frame-to-frame pose (plba_track_pose; StereoFrameHandler::optimizePose,
        src2/stereoFrameHandler.cpp:307-405) of a batch of frame pairs (plba.trackpose.TrackProblem),
        each solved by one workgroup of one launch. One dict per problem, with its inlier flags.
        Needs no uploaded window and leaves one intact."""
        return self._pose_batch("plba_track_pose", "plba_track_default_params", capi.TrackBatchView(problems),
                                params, capi.PlbaTrackParams, capi.PlbaTrackOut, capi.track_out_to_dict)

    def track_frames(self, pairs, params=None) -> list:
        """Frame-to-frame tracking (plba_track_frames; StereoFrameHandler::f2fTracking + optimizePose,
        src2/stereoFrameHandler.cpp:106-180, :307-405) of a batch of frame pairs (plba.trackframes.FramePair):
        the descriptors and features of the previous and of the current frame go in, and the matching, the
        gather of the matched rows and the pose run on the device in one call. ``params``: a
        capi.PlbaFramesParams (capi.frames_params), None for the defaults. One dict per pair: the fields of
        track_pose with the inlier flags per PREVIOUS row (0 where it has no match), pt_m12 / ln_m12
        (matches_12), n_pt / n_ln, and pt_cur_from_prev / ln_cur_from_prev, the previous row whose idx a
        current row inherits or -1. Needs no uploaded window and leaves one intact."""
        if params is None:
            params = capi.PlbaFramesParams()
            self.L.plba_frames_default_params(C.byref(params))
        bv = capi.FramesBatchView(pairs, params.desc_bytes)
        self._check(self.L.plba_track_frames(self.ctx, C.byref(bv.struct), C.byref(params), C.byref(bv.out_struct)),
                    "plba_track_frames")
        return bv.results()

    def desc_match(self, pairs, nnr, best_lr: bool = True, desc_bytes=None) -> list:
        """Descriptor matching (plba_desc_match; StVO::match / matchNNR, src2/matching.cpp:41-91) of a
        batch of descriptor-set pairs [(desc1, desc2), ...] of uint8 rows, both directions of every
        pair in one launch. ``nnr``: one ratio or one per pair (taken as float32). One
        (matches_12, n_matches) per pair: the desc2 row of each desc1 row or -1, and their count.
        Needs no uploaded window and leaves one intact."""
        return self._match("plba_desc_match", capi.MatchBatchView(pairs, nnr, best_lr, desc_bytes))

    def grid_match(self, problems, cols: int = 64, rows: int = 48, best_lr: bool = True, desc_bytes=None) -> list:
        """Grid-guided descriptor matching (plba_grid_match; both StVO::matchGrid overloads,
        src2/matching.cpp:111-258) of a batch of problems (capi.GridMatchBatchView: point and line
        problems mixed) over a cols x rows grid, in one call. One (matches_12, n_matches) per problem:
        the train row of each query row or -1, and their count. Needs no uploaded window and leaves
        one intact."""
        return self._match("plba_grid_match", capi.GridMatchBatchView(problems, cols, rows, best_lr, desc_bytes))

    def stereo_associate(self, frames, params, desc_bytes=None) -> list:
        """Stereo association (plba_stereo_associate; StereoFrame::matchStereoPoints / matchStereoLines,
        src2/stereoFrame.cpp:121-174, :310-435) of a batch of frames (capi.StereoBatchView) in one call.
        params: a dict over plba_stereo_default_params with width, height, fx, fy, cx, cy, b (or a
        capi.PlbaStereoParams). One dict per frame: n_pt, n_ls and the survivors' rows in increasing left
        index (pt_src, pt_pl, pt_disp, pt_P, pdesc; ls_src, ls_spl, ls_epl, ls_sdisp, ls_edisp, ls_sP, ls_eP,
        ls_le, ls_NDc with pluker, ldesc). Needs no uploaded window and leaves one intact."""
        bv, prm = self._associate("plba_stereo_associate", capi.StereoBatchView, capi.stereo_params, frames, params,
                                  desc_bytes)
        return bv.results(bool(prm.pluker))

    def kf_associate(self, pairs, params, desc_bytes=None) -> list:
        """Keyframe-to-keyframe association (plba_kf_associate; MapHandler::matchKF2KFPoints / Lines,
        src/mapHandler.cpp:237-590, up to the sequential part) of a batch of keyframe pairs
        (capi.KfassocBatchView) in one call. params: a dict over plba_kfassoc_default_params with width,
        height, fx, fy, cx, cy (or a capi.PlbaKfassocParams). One dict per pair, indexed by previous row:
        n_grid, n_matches, fallback as (points, lines); pt_m12, pt_rec [.][9]; ls_m12, ls_rec [.][8],
        ls_rejected. Needs no uploaded window and leaves one intact."""
        return self._associate("plba_kf_associate", capi.KfassocBatchView, capi.kfassoc_params, pairs, params,
                               desc_bytes)[0].results()

    def map_associate(self, problems, params, desc_bytes=None) -> list:
        """Map-to-keyframe association (plba_map_associate; MapHandler::matchMap2KFPoints / Lines,
        src/mapHandler.cpp:697-921, up to the sequential part) of a batch of keyframes
        (capi.MapassocBatchView) in one call. params: a dict over plba_mapassoc_default_params with width,
        height, fx, fy, cx, cy (or a capi.PlbaMapassocParams). One dict per keyframe, indexed by candidate
        row: n_visible, n_grid, n_matches, fallback, n_accepted as (points, lines); pt_visible, pt_m12,
        pt_accepted, pt_rec [.][6]; ls_visible, ls_m12, ls_accepted, ls_rec [.][9]. Needs no uploaded window
        and leaves one intact."""
        return self._associate("plba_map_associate", capi.MapassocBatchView, capi.mapassoc_params, problems, params,
                               desc_bytes)[0].results()

    def desc_medoid(self, list_ptr, desc, desc_bytes=None) -> np.ndarray:
        """Median descriptor (plba_desc_medoid; the descriptor half of updateAverageDescDir,
        src/mapFeatures.cpp:57-86) of a batch of descriptor lists in one launch: CSR offsets list_ptr
        [B+1] into desc [total][desc_bytes] uint8. Returns int32 [B]: the position within each list of
        the first descriptor with the smallest median Hamming distance to the list, -1 for an empty
        list. A list of more than capi.MEDOID_MAX_N descriptors is refused. Needs no uploaded window and
        leaves one intact."""
        bv = capi.MedoidBatchView(list_ptr, desc, desc_bytes)
        out = np.full(max(bv.struct.n, 1), -1, np.int32)
        self._check(self.L.plba_desc_medoid(self.ctx, C.byref(bv.struct), _p(out, C.c_int32)), "plba_desc_medoid")
        return out[:bv.struct.n].copy()

    def bow_set_vocab(self, slot: int, voc):
        """Uploads the vocabulary of a place-recognition slot (plba_bow_set_vocab; 0 points, 1 lines)
        from a flat tree (capi.BowVocabView) and clears the slot's database."""
        vv = voc if isinstance(voc, capi.BowVocabView) else capi.BowVocabView(voc)
        self._check(self.L.plba_bow_set_vocab(self.ctx, slot, C.byref(vv.struct)), "plba_bow_set_vocab")
        self._bow_live[slot] = 0

    def bow_insert(self, slot: int, kf_id: int, desc):
        """plba_bow_insert: the BoW vector of the uint8 rows ``desc`` (DBoW2 transform, TF-IDF / L1) is
        stored under kf_id and scored against every live stored vector and, last, itself.
        Returns (ids int32, scores float64) in increasing kf_id. Needs no uploaded window and leaves
        one intact."""
        desc = np.ascontiguousarray(desc, dtype=np.uint8)
        n_desc = int(desc.shape[0]) if desc.ndim == 2 else 0
        cap = self._bow_live.get(slot, 0) + 1
        scores, ids, n = np.zeros(cap), np.zeros(cap, np.int32), C.c_int32(0)
        self._check(self.L.plba_bow_insert(self.ctx, slot, kf_id, _p(desc, C.c_uint8) if n_desc else None, n_desc,
                                           _p(scores), _p(ids, C.c_int32), cap, C.byref(n)), "plba_bow_insert")
        if n.value != cap:
            raise PlbaError(f"plba_bow_insert returned {n.value} scores for {cap} live vectors")
        self._bow_live[slot] = cap
        return ids, scores

    def bow_remove(self, slot: int, kf_id: int):
        """plba_bow_remove: the vector of kf_id is never scored again."""
        self._check(self.L.plba_bow_remove(self.ctx, slot, kf_id), "plba_bow_remove")
        self._bow_live[slot] -= 1

    def bow_get(self, slot: int, kf_id: int):
        """plba_bow_get: (word_ids int32, values float64) of a stored vector, in increasing word id."""
        n = C.c_int32(0)
        self._check(self.L.plba_bow_get(self.ctx, slot, kf_id, None, None, 0, C.byref(n)), "plba_bow_get")
        w, v = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1))
        self._check(self.L.plba_bow_get(self.ctx, slot, kf_id, _p(w, C.c_int32), _p(v), n.value, C.byref(n)),
                    "plba_bow_get")
        return w[:n.value].copy(), v[:n.value].copy()

    def trace(self) -> np.ndarray:
        n = C.c_int32(0)
        self._check(self.L.plba_get_trace(self.ctx, None, 0, C.byref(n)), "plba_get_trace")
        buf = (capi.PlbaIterTrace * max(n.value, 1))()
        self._check(self.L.plba_get_trace(self.ctx, buf, n.value, C.byref(n)), "plba_get_trace")
        return capi.trace_to_array(buf, n.value)

    def kernel_times(self) -> dict:
        cap = 32
        names = (C.c_char_p * cap)()
        ms = np.zeros(cap)
        nl = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        self._check(self.L.plba_kernel_times(self.ctx, names, _p(ms), _p(nl, C.c_int32), cap, C.byref(n)),
                    "plba_kernel_times")
        return {names[i].decode(): (float(ms[i]), int(nl[i])) for i in range(n.value)}

    def structure_stats(self) -> dict:
        st = (C.c_int64 * 22)()
        self._check(self.L.plba_structure_stats(self.ctx, st, 22), "plba_structure_stats")
        return dict(nf=st[0], bw=st[1], nblk=st[2], triples=st[3], edges=st[4], landmarks=st[5], banded=st[6],
                    chunks=st[7], free_edges=st[8], point_edges=st[9], graph=st[10], sharded=st[11],
                    twisted=st[12], column_lane=st[13], bcr_rows=st[14], dense_mfma=st[15],
                    bcr_fallbacks=st[16], spec_slots=st[17], spec_policy=st[18], device_steps=st[19],
                    bcr_fused=st[20], device_build=st[21])

    def synchronize(self):
        self._check(self.L.plba_synchronize(self.ctx), "plba_synchronize")
