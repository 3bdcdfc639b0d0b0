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

EXPORTED = [
    "plba_default_opts", "plba_create", "plba_destroy", "plba_last_error", "plba_upload", "plba_reset_estimates",
    "plba_set_edge_levels", "plba_set_robust", "plba_initialize_optimization", "plba_optimize",
    "plba_refresh_edge_errors", "plba_get_edge_chi2", "plba_download", "plba_lba_plucker", "plba_get_trace",
    "plba_synchronize", "plba_enable_kernel_timing", "plba_kernel_times", "plba_structure_stats",
    "plba_shard_plan", "plba_comm_unique_id", "plba_comm_init_rccl", "plba_comm_init_host",
    "plba_comm_info", "plba_factor_plan",
    "plba_hlm_default_params", "plba_hlm_lba",
    "plba_pgo_default_params", "plba_pgo_optimize",
    "plba_lcpose_default_params", "plba_lc_relative_pose",
    "plba_track_default_params", "plba_track_pose", "plba_frames_default_params", "plba_track_frames",
    "plba_desc_match", "plba_grid_match", "plba_stereo_default_params", "plba_stereo_associate",
    "plba_kfassoc_default_params", "plba_kf_associate", "plba_mapassoc_default_params", "plba_map_associate",
    "plba_desc_medoid",
    "plba_bow_set_vocab", "plba_bow_insert", "plba_bow_remove", "plba_bow_get",
]

# int (*plba_host_allreduce_fn)(void *user, double *buf, int64_t n)
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)


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
    vp = C.c_void_p
    dp = C.POINTER(C.c_double)
    bp = C.POINTER(C.c_uint8)
    ip = C.POINTER(C.c_int32)
    L.plba_default_opts.argtypes = [C.POINTER(capi.PlbaOpts)]
    L.plba_default_opts.restype = None
    L.plba_create.argtypes = [C.POINTER(vp), C.POINTER(capi.PlbaOpts)]
    L.plba_destroy.argtypes = [vp]
    L.plba_last_error.argtypes = [vp]
    L.plba_last_error.restype = C.c_char_p
    L.plba_upload.argtypes = [vp, C.POINTER(capi.PlbaGraph)]
    L.plba_reset_estimates.argtypes = [vp]
    L.plba_set_edge_levels.argtypes = [vp, bp, bp]
    L.plba_set_robust.argtypes = [vp, C.c_int32]
    L.plba_initialize_optimization.argtypes = [vp, C.c_int32]
    L.plba_optimize.argtypes = [vp, C.c_int32, ip, dp]
    L.plba_refresh_edge_errors.argtypes = [vp, C.c_int32]
    L.plba_get_edge_chi2.argtypes = [vp, dp, bp, dp]
    L.plba_download.argtypes = [vp, dp, dp, dp]
    L.plba_lba_plucker.argtypes = [vp, C.POINTER(capi.PlbaResult)]
    L.plba_get_trace.argtypes = [vp, C.POINTER(capi.PlbaIterTrace), C.c_int32, ip]
    L.plba_synchronize.argtypes = [vp]
    L.plba_enable_kernel_timing.argtypes = [vp, C.c_int32]
    L.plba_kernel_times.argtypes = [vp, C.POINTER(C.c_char_p), dp, ip, C.c_int32, ip]
    L.plba_structure_stats.argtypes = [vp, C.POINTER(C.c_int64), C.c_int32]
    L.plba_shard_plan.argtypes = [C.POINTER(capi.PlbaGraph), C.c_int32, ip, ip]
    L.plba_comm_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    L.plba_comm_init_rccl.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]
    L.plba_comm_init_host.argtypes = [vp, C.c_int32, C.c_int32, HOST_ALLREDUCE_FN, vp]
    L.plba_comm_info.argtypes = [vp, ip, C.c_int32]
    L.plba_factor_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, C.c_int32]
    L.plba_hlm_default_params.argtypes = [C.POINTER(capi.PlbaHlmParams)]
    L.plba_hlm_default_params.restype = None
    L.plba_hlm_lba.argtypes = [vp, C.POINTER(capi.PlbaHlmState), C.POINTER(capi.PlbaHlmParams),
                               C.POINTER(capi.PlbaHlmResult)]
    L.plba_pgo_default_params.argtypes = [C.POINTER(capi.PlbaPgoParams)]
    L.plba_pgo_default_params.restype = None
    L.plba_pgo_optimize.argtypes = [vp, C.POINTER(capi.PlbaPgoGraph), C.POINTER(capi.PlbaPgoParams),
                                    C.POINTER(capi.PlbaPgoResult)]
    L.plba_lcpose_default_params.argtypes = [C.POINTER(capi.PlbaLcposeParams)]
    L.plba_lcpose_default_params.restype = None
    L.plba_lc_relative_pose.argtypes = [vp, C.POINTER(capi.PlbaLcposeBatch), C.POINTER(capi.PlbaLcposeParams),
                                        C.POINTER(capi.PlbaLcposeOut), bp, bp]
    L.plba_track_default_params.argtypes = [C.POINTER(capi.PlbaTrackParams)]
    L.plba_track_default_params.restype = None
    L.plba_track_pose.argtypes = [vp, C.POINTER(capi.PlbaTrackBatch), C.POINTER(capi.PlbaTrackParams),
                                  C.POINTER(capi.PlbaTrackOut), bp, bp]
    L.plba_frames_default_params.argtypes = [C.POINTER(capi.PlbaFramesParams)]
    L.plba_frames_default_params.restype = None
    L.plba_track_frames.argtypes = [vp, C.POINTER(capi.PlbaFramesBatch), C.POINTER(capi.PlbaFramesParams),
                                    C.POINTER(capi.PlbaFramesOut)]
    L.plba_desc_match.argtypes = [vp, C.POINTER(capi.PlbaMatchBatch), ip, ip]
    L.plba_grid_match.argtypes = [vp, C.POINTER(capi.PlbaGridMatchBatch), ip, ip]
    L.plba_stereo_default_params.argtypes = [C.POINTER(capi.PlbaStereoParams)]
    L.plba_stereo_default_params.restype = None
    L.plba_stereo_associate.argtypes = [vp, C.POINTER(capi.PlbaStereoBatch), C.POINTER(capi.PlbaStereoParams),
                                        C.POINTER(capi.PlbaStereoOut)]
    L.plba_kfassoc_default_params.argtypes = [C.POINTER(capi.PlbaKfassocParams)]
    L.plba_kfassoc_default_params.restype = None
    L.plba_kf_associate.argtypes = [vp, C.POINTER(capi.PlbaKfassocBatch), C.POINTER(capi.PlbaKfassocParams),
                                    C.POINTER(capi.PlbaKfassocOut)]
    L.plba_mapassoc_default_params.argtypes = [C.POINTER(capi.PlbaMapassocParams)]
    L.plba_mapassoc_default_params.restype = None
    L.plba_map_associate.argtypes = [vp, C.POINTER(capi.PlbaMapassocBatch), C.POINTER(capi.PlbaMapassocParams),
                                     C.POINTER(capi.PlbaMapassocOut)]
    L.plba_desc_medoid.argtypes = [vp, C.POINTER(capi.PlbaMedoidBatch), ip]
    L.plba_bow_set_vocab.argtypes = [vp, C.c_int32, C.POINTER(capi.PlbaBowVocab)]
    L.plba_bow_insert.argtypes = [vp, C.c_int32, C.c_int32, bp, C.c_int32, dp, ip, C.c_int32, ip]
    L.plba_bow_remove.argtypes = [vp, C.c_int32, C.c_int32]
    L.plba_bow_get.argtypes = [vp, C.c_int32, C.c_int32, ip, dp, C.c_int32, ip]
    for name in EXPORTED:
        f = getattr(L, name)
        if name not in ("plba_default_opts", "plba_last_error", "plba_hlm_default_params", "plba_pgo_default_params",
                        "plba_lcpose_default_params", "plba_stereo_default_params", "plba_kfassoc_default_params",
                        "plba_track_default_params", "plba_mapassoc_default_params", "plba_frames_default_params"):
            f.restype = C.c_int
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

    def lc_relative_pose(self, problems, params=None) -> list:
        """Loop-closure relative pose (plba_lc_relative_pose; computeRelativePoseRobustGN /
        computeRelativePoseGN, src/mapHandler.cpp:4677-5068 / :4413-4675) of a batch of candidate
        pairs (plba.lcpose.LcProblem), verified in one launch. One dict per candidate, with its
        inlier flags. Needs no uploaded window and leaves one intact."""
        if params is None:
            params = capi.PlbaLcposeParams()
            self.L.plba_lcpose_default_params(C.byref(params))
        bv = capi.LcposeBatchView(list(problems))
        n = bv.struct.n
        out = (capi.PlbaLcposeOut * max(n, 1))()
        pin = np.zeros(max(int(bv.pt_off[-1]), 1), np.uint8)
        lin = np.zeros(max(int(bv.ln_off[-1]), 1), np.uint8)
        self._check(self.L.plba_lc_relative_pose(self.ctx, C.byref(bv.struct), C.byref(params), out,
                                                 _p(pin, C.c_uint8), _p(lin, C.c_uint8)), "plba_lc_relative_pose")
        return [capi.lcpose_out_to_dict(out[i], pin[bv.pt_off[i]:bv.pt_off[i + 1]], lin[bv.ln_off[i]:bv.ln_off[i + 1]])
                for i in range(n)]

    def track_pose(self, problems, params=None) -> list:
        """Frame-to-frame pose (plba_track_pose; StereoFrameHandler::optimizePose,
        src2/stereoFrameHandler.cpp:307-405) of a batch of frame pairs (plba.trackpose.TrackProblem),
        each solved by one workgroup of one launch. One dict per problem, with its inlier flags.
        Needs no uploaded window and leaves one intact."""
        if params is None:
            params = capi.PlbaTrackParams()
            self.L.plba_track_default_params(C.byref(params))
        bv = capi.TrackBatchView(list(problems))
        n = bv.struct.n
        out = (capi.PlbaTrackOut * max(n, 1))()
        pin = np.zeros(max(int(bv.pt_off[-1]), 1), np.uint8)
        lin = np.zeros(max(int(bv.ln_off[-1]), 1), np.uint8)
        self._check(self.L.plba_track_pose(self.ctx, C.byref(bv.struct), C.byref(params), out,
                                           _p(pin, C.c_uint8), _p(lin, C.c_uint8)), "plba_track_pose")
        return [capi.track_out_to_dict(out[i], pin[bv.pt_off[i]:bv.pt_off[i + 1]], lin[bv.ln_off[i]:bv.ln_off[i + 1]])
                for i in range(n)]

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
        bv = capi.MatchBatchView(pairs, nnr, best_lr, desc_bytes)
        n = bv.struct.n
        m12 = np.full(max(int(bv.off1[-1]), 1), -1, np.int32)
        cnt = np.zeros(max(n, 1), np.int32)
        self._check(self.L.plba_desc_match(self.ctx, C.byref(bv.struct), _p(m12, C.c_int32), _p(cnt, C.c_int32)),
                    "plba_desc_match")
        return [(m12[bv.off1[i]:bv.off1[i + 1]].copy(), int(cnt[i])) for i in range(n)]

    def grid_match(self, problems, cols: int = 64, rows: int = 48, best_lr: bool = True, desc_bytes=None) -> list:
        """Grid-guided descriptor matching (plba_grid_match; both StVO::matchGrid overloads,
        src2/matching.cpp:111-258) of a batch of problems (capi.GridMatchBatchView: point and line
        problems mixed) over a cols x rows grid, in one call. One (matches_12, n_matches) per problem:
        the train row of each query row or -1, and their count. Needs no uploaded window and leaves
        one intact."""
        bv = capi.GridMatchBatchView(problems, cols, rows, best_lr, desc_bytes)
        n = bv.struct.n
        m12 = np.full(max(int(bv.off1[-1]), 1), -1, np.int32)
        cnt = np.zeros(max(n, 1), np.int32)
        self._check(self.L.plba_grid_match(self.ctx, C.byref(bv.struct), _p(m12, C.c_int32), _p(cnt, C.c_int32)),
                    "plba_grid_match")
        return [(m12[bv.off1[i]:bv.off1[i + 1]].copy(), int(cnt[i])) for i in range(n)]

    def stereo_associate(self, frames, params, desc_bytes=None) -> list:
        """Stereo association (plba_stereo_associate; StereoFrame::matchStereoPoints / matchStereoLines,
        src2/stereoFrame.cpp:121-174, :310-435) of a batch of frames (capi.StereoBatchView) in one call.
        params: a dict over plba_stereo_default_params with width, height, fx, fy, cx, cy, b (or a
        capi.PlbaStereoParams). One dict per frame: n_pt, n_ls and the survivors' rows in increasing left
        index (pt_src, pt_pl, pt_disp, pt_P, pdesc; ls_src, ls_spl, ls_epl, ls_sdisp, ls_edisp, ls_sP, ls_eP,
        ls_le, ls_NDc with pluker, ldesc). Needs no uploaded window and leaves one intact."""
        bv = frames if isinstance(frames, capi.StereoBatchView) else capi.StereoBatchView(frames, desc_bytes)
        prm = capi.stereo_params(params)
        self._check(self.L.plba_stereo_associate(self.ctx, C.byref(bv.struct), C.byref(prm), C.byref(bv.out)),
                    "plba_stereo_associate")
        return bv.results(bool(prm.pluker))

    def kf_associate(self, pairs, params, desc_bytes=None) -> list:
        """Keyframe-to-keyframe association (plba_kf_associate; MapHandler::matchKF2KFPoints / Lines,
        src/mapHandler.cpp:237-590, up to the sequential part) of a batch of keyframe pairs
        (capi.KfassocBatchView) in one call. params: a dict over plba_kfassoc_default_params with width,
        height, fx, fy, cx, cy (or a capi.PlbaKfassocParams). One dict per pair, indexed by previous row:
        n_grid, n_matches, fallback as (points, lines); pt_m12, pt_rec [.][9]; ls_m12, ls_rec [.][8],
        ls_rejected. Needs no uploaded window and leaves one intact."""
        bv = pairs if isinstance(pairs, capi.KfassocBatchView) else capi.KfassocBatchView(pairs, desc_bytes)
        prm = capi.kfassoc_params(params)
        self._check(self.L.plba_kf_associate(self.ctx, C.byref(bv.struct), C.byref(prm), C.byref(bv.out)),
                    "plba_kf_associate")
        return bv.results()

    def map_associate(self, problems, params, desc_bytes=None) -> list:
        """Map-to-keyframe association (plba_map_associate; MapHandler::matchMap2KFPoints / Lines,
        src/mapHandler.cpp:697-921, up to the sequential part) of a batch of keyframes
        (capi.MapassocBatchView) in one call. params: a dict over plba_mapassoc_default_params with width,
        height, fx, fy, cx, cy (or a capi.PlbaMapassocParams). One dict per keyframe, indexed by candidate
        row: n_visible, n_grid, n_matches, fallback, n_accepted as (points, lines); pt_visible, pt_m12,
        pt_accepted, pt_rec [.][6]; ls_visible, ls_m12, ls_accepted, ls_rec [.][9]. Needs no uploaded window
        and leaves one intact."""
        bv = problems if isinstance(problems, capi.MapassocBatchView) else capi.MapassocBatchView(problems, desc_bytes)
        prm = capi.mapassoc_params(params)
        self._check(self.L.plba_map_associate(self.ctx, C.byref(bv.struct), C.byref(prm), C.byref(bv.out)),
                    "plba_map_associate")
        return bv.results()

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
