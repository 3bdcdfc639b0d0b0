"""plslam_track_pose_cpu (host/track_pose.cpp, the single-threaded C++ restatement of plba_track_pose)
against the numpy checker (tests/ref_trackpose.py) on the cases the GPU tests use. Both sum H, g and e
in match order, so integers and flags are equal and every float agrees within parity.elem_violation <= 1."""
import numpy as np
import pytest

import parity
import trackpose_cases as cases
from plba import capi, trackpose as tp

INT_KEYS = ("branch", "iters_first", "iters_ref", "n_inl_pt", "n_inl_ln")
FLOAT_KEYS = ("DT", "DT_solver", "err_norm", "s_p", "s_l", "H", "DT_cov", "DT_cov_eig")
model_param = pytest.mark.parametrize("model", cases.MODELS, ids=cases.MODEL_IDS)


def _assert_equal(out, ref):
    for k in INT_KEYS:
        assert out[k] == ref[k], (k, out[k], ref[k])
    assert np.array_equal(out["pt_inlier"], ref["pt_inlier"]) and np.array_equal(out["ln_inlier"], ref["ln_inlier"])
    for k in FLOAT_KEYS:
        v = parity.elem_violation(out[k], ref[k])
        assert v <= 1.0, (k, v)


@model_param
@pytest.mark.parametrize("case", cases.GPU_CASES, ids=[c.name for c in cases.GPU_CASES])
def test_restatement_matches_the_checker(case, model):
    out = tp.track_pose_cpu([case.problem()], case.params(model))[0]
    _assert_equal(out, case.reference(model))


@model_param
def test_a_batch_is_its_problems_one_by_one(model):
    cs = [cases.BRANCH[capi.TRACK_OK], cases.PARITY[3], cases.BRANCH[capi.TRACK_FEW_BEFORE]]
    p = cs[0].params(model)
    batch = tp.track_pose_cpu([c.problem() for c in cs] + [tp.empty()], p)
    for c, o in zip(cs, batch):
        alone = tp.track_pose_cpu([c.problem()], p)[0]
        assert all(np.asarray(o[k]).tobytes() == np.asarray(alone[k]).tobytes() for k in INT_KEYS + FLOAT_KEYS)
    assert batch[3]["branch"] == capi.TRACK_FEW_BEFORE


@model_param
def test_z_zero_is_rejected_without_a_fault(model):
    out = tp.track_pose_cpu([cases.Z0.problem()], cases.Z0.params(model))[0]
    ref = cases.Z0.reference(model)
    assert out["branch"] == ref["branch"] != capi.TRACK_OK and out["err_norm"] == -1.0
    assert out["DT"].tobytes() == np.eye(4).tobytes()


def test_refusals():
    ok = cases.BRANCH[capi.TRACK_OK]
    assert tp.track_pose_cpu([]) == []
    for kw in (dict(line_model=2), dict(max_iters=0)):
        with pytest.raises(RuntimeError):
            tp.track_pose_cpu([ok.problem()], capi.track_params(**kw))
    with pytest.raises(RuntimeError):
        tp.track_pose_cpu([tp.synth(capi.TRACK_MAX_N + 1, 0, seed=1)])
