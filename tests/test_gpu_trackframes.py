"""Frame-to-frame tracking on the GPU (plba_track_frames: StereoFrameHandler::f2fTracking + optimizePose,
src2/stereoFrameHandler.cpp:106-180, :307-405, both line models) over the cases of
tests/trackframes_cases.py. Three bars:
  - every integer output equals the checker's (tests/ref_trackframes.py) exactly;
  - plba_track_out and the inlier flags are bitwise what plba_track_pose returns on the same context for the
    batch gathered on the host from plba_desc_match's output: the same kernel on the same rows in the same
    order, so no tolerance;
  - against the checker the doubles keep tests/test_gpu_trackpose.py's tolerances, copied.
tests/test_trackframes_oracle.py checks that every decision of these cases stays away from its threshold."""
import struct

import numpy as np
import pytest

import parity
import trackframes_cases as cases
from plba import capi, trackframes as tf

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
INT_KEYS = ("branch", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln", "n_pt", "n_ln")
ARRAY_KEYS = ("pt_m12", "ln_m12", "pt_cur_from_prev", "ln_cur_from_prev", "pt_inlier", "ln_inlier")
OUT_KEYS = ("branch", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln", "err_norm", "s_p", "s_l", "DT", "DT_cov",
            "DT_cov_eig", "DT_solver", "H")
model_param = pytest.mark.parametrize("model", cases.MODELS, ids=cases.MODEL_IDS)
case_param = pytest.mark.parametrize("case", cases.GPU_CASES, ids=[c.name for c in cases.GPU_CASES])


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _bits(x):
    """A result as nested tuples of bytes: equality is bitwise (NaN and -0.0 included)."""
    if isinstance(x, dict):
        return tuple((k, _bits(v)) for k, v in sorted(x.items()) if k != "solve_ms")
    if isinstance(x, (list, tuple)):
        return tuple(_bits(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, float):
        return struct.pack("d", x)
    return x


def _assert_integers(out, ref):
    for k in INT_KEYS:
        assert out[k] == ref[k], (k, out[k], ref[k])
    for k in ARRAY_KEYS:
        assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]), (k, out[k], ref[k])


def _assert_parity(out, ref):
    """tests/test_gpu_trackpose.py's tolerances"""
    for k in ("DT", "DT_solver", "err_norm", "s_p", "s_l"):
        v = parity.elem_violation(out[k], ref[k])
        print(k, "violation", v)
        assert v <= 1.0, (k, v, out[k], ref[k])
    if np.abs(ref["H"]).max() > 0:
        dH = float(np.abs(out["H"] - ref["H"]).max() / np.abs(ref["H"]).max())
        print("H rel", dH)
        assert dH <= 1e-8, dH
    if ref["err_norm"] != -1.0:
        tol = 1e-8 + 100.0 * EPS * np.linalg.cond(ref["H"])
        for k in ("DT_cov", "DT_cov_eig"):
            d = float(np.abs(out[k] - ref[k]).max() / np.abs(ref[k]).max())
            print(k, "rel", d, "tol", tol)
            assert d <= tol, (k, d, tol)
    else:
        assert not out["DT_cov"].any() and not out["DT_cov_eig"].any()
        assert out["DT"].tobytes() == np.eye(4).tobytes()


def _two_calls(solver, pairs, p):
    """plba_desc_match, the gather on the host, plba_track_pose: one dict per pair with the inlier flags
    scattered to the previous rows."""
    sets = [s for q in pairs for s in ((q.prev_pdesc, q.cur_pdesc), (q.prev_ldesc, q.cur_ldesc))]
    m = solver.desc_match(sets, [p.nnr_pt, p.nnr_ln] * len(pairs), bool(p.best_lr), p.desc_bytes)
    none = lambda a: np.full(len(a), -1, np.int32)
    pt = [m[2 * k][0] if p.track.has_points else none(q.prev_pdesc) for k, q in enumerate(pairs)]
    ln = [m[2 * k + 1][0] if p.track.has_lines else none(q.prev_ldesc) for k, q in enumerate(pairs)]
    out = solver.track_pose([tf.gather(q, a, b) for q, a, b in zip(pairs, pt, ln)], p.track)
    for o, a, b in zip(out, pt, ln):
        for key, m12 in (("pt_inlier", a), ("ln_inlier", b)):
            flags = np.zeros(len(m12), np.uint8)
            flags[m12 >= 0] = o[key]
            o[key] = flags
        o.update(pt_m12=a, ln_m12=b)
    return out


@model_param
@case_param
def test_integers_equal_the_checker_and_doubles_keep_the_pose_tolerances(solver, case, model):
    out = solver.track_frames(case.pairs(), case.params(model))
    assert len(out) == len(case.pairs())
    for o, ref in zip(out, case.reference(model)):
        _assert_integers(o, ref)
        _assert_parity(o, ref)


@model_param
@case_param
def test_the_pose_is_bitwise_that_of_the_two_call_path(solver, case, model):
    p = case.params(model)
    one = solver.track_frames(case.pairs(), p)
    two = _two_calls(solver, case.pairs(), p)
    for a, b in zip(one, two):
        for k in OUT_KEYS + ("pt_inlier", "ln_inlier", "pt_m12", "ln_m12"):
            assert _bits(a[k]) == _bits(b[k]), k


@model_param
def test_a_pair_alone_is_the_pair_in_the_batch_and_a_batch_twice_is_the_same(solver, model):
    p = cases.B.params(model)
    first, second = solver.track_frames(cases.B.pairs(), p), solver.track_frames(cases.B.pairs(), p)
    assert _bits(first) == _bits(second)
    for q, o in zip(cases.B.pairs(), first):
        assert _bits(solver.track_frames([q], p)[0]) == _bits(o)
    # every output of the pair whose previous frame is empty is defined
    e = first[3]
    assert e["branch"] == capi.TRACK_FEW_BEFORE and (e["n_pt"], e["n_ln"], e["n_inl_pt"], e["n_inl_ln"]) == (0, 0, 0, 0)
    assert e["pt_cur_from_prev"].tolist() == [-1] * 6 and e["ln_cur_from_prev"].tolist() == [-1] * 4
    assert e["DT"].tobytes() == np.eye(4).tobytes() and e["err_norm"] == -1.0 and len(e["pt_m12"]) == 0


@model_param
def test_a_kind_that_is_switched_off_has_no_match(solver, model):
    q = cases.A.pairs()
    for kw, keep in ((dict(has_points=0), "ln"), (dict(has_lines=0), "pt")):
        p = cases.A.params(model, **kw)
        out, ref = solver.track_frames(q, p)[0], tf.track_frames_cpu(q, p)[0]
        off = "pt" if keep == "ln" else "ln"
        assert (out[off + "_m12"] == -1).all() and out["n_" + off] == 0 and (out[off + "_cur_from_prev"] == -1).all()
        assert out["n_" + keep] == 12
        _assert_integers(out, ref)
        assert _bits([out[k] for k in OUT_KEYS]) == _bits([_two_calls(solver, q, p)[0][k] for k in OUT_KEYS])


def test_the_cap_on_previous_rows_and_one_above(solver):
    """2048 previous rows are accepted (case F, above); 2049 are refused before any launch, the context stays
    usable and case A gives bitwise what it gave before."""
    from plba.lib import PlbaError
    p = cases.A.params(capi.TRACK_PLUCKER)
    before = solver.track_frames(cases.A.pairs(), p)
    with pytest.raises(PlbaError) as e:
        solver.track_frames([cases.too_wide()], cases.F.params(capi.TRACK_PLUCKER))
    assert "PLBA_E_INVALID" in str(e.value) and str(capi.TRACK_MAX_N + 1) in str(e.value)
    assert _bits(solver.track_frames(cases.A.pairs(), p)) == _bits(before)
    _assert_integers(before[0], cases.A.reference(capi.TRACK_PLUCKER)[0])


def test_invalid_arguments(solver):
    import ctypes as C
    from plba.lib import PlbaError
    q = cases.A.pairs()
    assert solver.track_frames([]) == []                                   # n == 0: PLBA_OK
    for p in (capi.frames_params(capi.track_params(line_model=2)), capi.frames_params(capi.track_params(max_iters=0)),
              capi.frames_params(capi.track_params(max_iters_ref=0)), capi.frames_params(desc_bytes=30),
              capi.frames_params(desc_bytes=68)):
        with pytest.raises(PlbaError):
            solver.track_frames(q, p)
    bv = capi.FramesBatchView(q)
    prm = capi.frames_params()
    L = solver.L

    def call(**kw):
        for k, v in kw.items():
            setattr(bv.out_struct if hasattr(bv.out_struct, k) else bv.struct, k, v)
        return L.plba_track_frames(solver.ctx, C.byref(bv.struct), C.byref(prm), C.byref(bv.out_struct))

    assert call(pt_inlier=None, ln_inlier=None) == 0                      # the inlier arrays are optional
    assert call(n=-1) != 0
    assert call(n=1, prev_ln_NDc=None) != 0                               # the Plücker model reads NDc
    bv = capi.FramesBatchView(q)
    assert call(pt_m12=None) != 0
    bv = capi.FramesBatchView(q)
    ip = C.POINTER(C.c_int32)
    bad, shifted = np.array([5, 0], np.int32), np.array([1, 12], np.int32)
    assert call(pt_off1=bad.ctypes.data_as(ip)) != 0                      # decreasing offsets
    assert call(pt_off1=shifted.ctypes.data_as(ip)) != 0                  # offsets start at 0
    assert L.plba_track_frames(solver.ctx, None, C.byref(prm), C.byref(bv.out_struct)) != 0
    assert L.plba_track_frames(solver.ctx, C.byref(capi.FramesBatchView(q).struct), C.byref(prm), None) != 0
    prm.track.use_motion_model = 1
    bv = capi.FramesBatchView(q)
    assert call(prev=None) != 0                                           # the motion model reads prev
    out = solver.track_frames(q, cases.A.params(0))[0]                    # the context is usable
    _assert_integers(out, cases.A.reference(0)[0])


def test_an_uploaded_window_and_a_grown_block_survive_the_call():
    """A window uploaded before the call solves to what a fresh context gives; a small call after a large one,
    on the block the large one grew and left full, gives what a fresh context gives."""
    import golden_io
    from plba.lib import Solver
    g, _ = golden_io.load("C1L")
    pa, pc = cases.A.params(capi.TRACK_PLUCKER), cases.C.params(capi.TRACK_PLUCKER)
    with Solver() as w:
        w.upload(g)
        fresh_lba = _bits(w.lba_plucker())
        fresh_a = _bits(w.track_frames(cases.A.pairs(), pa))
    with Solver() as s:
        s.upload(g)
        large = s.track_frames(cases.C.pairs(), pc)
        assert _bits(s.track_frames(cases.A.pairs(), pa)) == fresh_a
        assert _bits(s.lba_plucker()) == fresh_lba
        assert _bits(s.track_frames(cases.C.pairs(), pc)) == _bits(large)
