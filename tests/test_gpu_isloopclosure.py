"""isLoopClosure from two keyframe indices with no hooks: the descriptor matching (plba_desc_match)
and the relative pose (plba_lc_relative_pose) on the GPU, against the hooked CPU run of
tests/test_host_isloopclosure.py (numpy checkers). The matching is exact, so the candidate, the
counts, the gate and the state transitions are equal; pose_inc is held to the tolerance
tests/test_gpu_lcpose.py uses (parity.elem_violation <= 1)."""
import numpy as np
import pytest

import parity
from plba.slam_map import LC_ACTIVE, LC_IDLE
from test_host_isloopclosure import CANDIDATES, KF_CURR, PLANTED, hostmap

pytestmark = pytest.mark.gpu


def _sequence(h):
    """accept (planted) -> accept (planted) -> reject (unrelated): pose graph -> IDLE."""
    out = dict(steps=[], states=[])
    for kf_prev in (PLANTED[0], PLANTED[1], 1):
        out["steps"].append(h.loop_closure_step_kf(kf_prev, KF_CURR))
        out["states"].append(h.lc_state())
        if kf_prev == PLANTED[1]:
            out["poses"], out["idxs"] = h.lc_pose_list().copy(), h.lc_idx_list().copy()
            out["rows"] = [h.lc_feature_idxs(kind, loop) for loop in (0, 1) for kind in (1, 2)]
    return out


def test_device_run_equals_the_hooked_run():
    ref_h, _ = hostmap()
    ref = _sequence(ref_h)
    gpu_h, _ = hostmap(hooks=False)
    out = _sequence(gpu_h)
    assert ref["states"] == [LC_ACTIVE, LC_ACTIVE, LC_IDLE] and out["states"] == ref["states"]
    for a, b in zip(out["steps"], ref["steps"]):
        for k in ("is_candidate", "ratio_ok", "accepted", "conditions", "n_inl_pt", "n_inl_ln", "state_before",
                  "state_after", "pgo_ran", "inl_ratio_pt", "inl_ratio_ls"):   # the ratios: exact counts
            assert a[k] == b[k], (k, a[k], b[k])
    assert [s["accepted"] for s in ref["steps"]] == [1, 1, 0] and ref["steps"][2]["ratio_ok"] == 0
    # the same candidate: the kept index rows are the matched rows the relative pose calls inliers
    for a, b in zip(out["rows"], ref["rows"]):
        np.testing.assert_array_equal(a, b)
    assert len(ref["rows"][0]) == 30 and len(ref["rows"][1]) == 9
    np.testing.assert_array_equal(out["idxs"], ref["idxs"])
    v = parity.elem_violation(out["poses"], ref["poses"])
    print("pose_inc violation", v)
    assert v <= 1.0
    ref_h.close()
    gpu_h.close()


def test_verify_loop_candidates_accepts_exactly_the_planted():
    ref_h, _ = hostmap()
    ref = ref_h.verify_loop_candidates(KF_CURR, CANDIDATES)
    gpu_h, _ = hostmap(hooks=False)
    before = (gpu_h.lc_state(), gpu_h.lc_pose_list().tobytes(), gpu_h.lc_idx_list().tobytes())
    out = gpu_h.verify_loop_candidates(KF_CURR, CANDIDATES)
    assert out["accepted"].tolist() == [int(k in PLANTED) for k in CANDIDATES] == ref["accepted"].tolist()
    np.testing.assert_array_equal(out["n_matches"], ref["n_matches"])
    assert out["n_matches"][PLANTED[0]].tolist() == [40, 12]
    v = parity.elem_violation(out["pose_inc"][list(PLANTED)], ref["pose_inc"][list(PLANTED)])
    print("pose_inc violation", v)
    assert v <= 1.0
    assert not out["pose_inc"][[k for k in CANDIDATES if k not in PLANTED]].any()
    assert (gpu_h.lc_state(), gpu_h.lc_pose_list().tobytes(), gpu_h.lc_idx_list().tobytes()) == before
    # the batch equals the single steps on the device
    st = gpu_h.loop_closure_step_kf(PLANTED[1], KF_CURR)
    assert st["accepted"] == 1
    np.testing.assert_array_equal(gpu_h.lc_pose_list()[0], out["pose_inc"][PLANTED[1]])
    ref_h.close()
    gpu_h.close()
