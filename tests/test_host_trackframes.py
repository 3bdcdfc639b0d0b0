"""plslam_track_frames_cpu (host/track_frames.cpp, the single-threaded C++ restatement of plba_track_frames)
against the checker (tests/ref_trackframes.py) on the cases the GPU tests use: every integer is equal, and
the doubles agree as plslam_track_pose_cpu's do in tests/test_host_trackpose.py (parity.elem_violation <= 1:
both sides sum H, g and e in match order)."""
import numpy as np
import pytest

import parity
import trackframes_cases as cases
from plba import capi, trackframes as tf

INT_KEYS = ("branch", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln", "n_pt", "n_ln")
ARRAY_KEYS = ("pt_m12", "ln_m12", "pt_cur_from_prev", "ln_cur_from_prev", "pt_inlier", "ln_inlier")
FLOAT_KEYS = ("DT", "DT_solver", "err_norm", "s_p", "s_l", "H", "DT_cov", "DT_cov_eig")
model_param = pytest.mark.parametrize("model", cases.MODELS, ids=cases.MODEL_IDS)


def _assert_equal(out, ref):
    for k in INT_KEYS:
        assert out[k] == ref[k], (k, out[k], ref[k])
    for k in ARRAY_KEYS:
        assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]), (k, out[k], ref[k])
    for k in FLOAT_KEYS:
        v = parity.elem_violation(out[k], ref[k])
        assert v <= 1.0, (k, v)


@model_param
@pytest.mark.parametrize("case", cases.GPU_CASES, ids=[c.name for c in cases.GPU_CASES])
def test_restatement_matches_the_checker(case, model):
    out = tf.track_frames_cpu(case.pairs(), case.params(model))
    assert len(out) == len(case.pairs())
    for o, ref in zip(out, case.reference(model)):
        _assert_equal(o, ref)


@model_param
def test_a_batch_is_its_pairs_one_by_one(model):
    p = cases.B.params(model)
    batch = tf.track_frames_cpu(cases.B.pairs(), p)
    for q, o in zip(cases.B.pairs(), batch):
        alone = tf.track_frames_cpu([q], p)[0]
        assert all(np.asarray(o[k]).tobytes() == np.asarray(alone[k]).tobytes() for k in INT_KEYS + ARRAY_KEYS + FLOAT_KEYS)


def test_a_kind_that_is_switched_off_has_no_match():
    q = cases.A.pairs()[0]
    out = tf.track_frames_cpu([q], cases.A.params(capi.TRACK_PLUCKER, has_lines=0))[0]
    assert (out["ln_m12"] == -1).all() and out["n_ln"] == 0 and out["n_pt"] == 12 and (out["ln_cur_from_prev"] == -1).all()


def test_refusals():
    q = cases.A.pairs()[0]
    assert tf.track_frames_cpu([]) == []
    for p in (capi.frames_params(capi.track_params(line_model=2)), capi.frames_params(capi.track_params(max_iters=0)),
              capi.frames_params(desc_bytes=30)):
        with pytest.raises(RuntimeError):
            tf.track_frames_cpu([q], p)
    with pytest.raises(RuntimeError):
        tf.track_frames_cpu([cases.too_wide()])
