"""The map-to-keyframe association of the host mirror (plslam_match_map_to_kf) with the device matchers
(plba_grid_match, plba_desc_match) against the same call with the CPU hooks, and the local-mapping step
that starts from it."""
import numpy as np
import pytest

import mapmatch_cases as mc
from plba import synth
from plba.slam_map import HostMap, SlamParams, make_map, mapmatch_params
from test_host_mapmatch import hostmap, state

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", [dict(), dict(ws=0, min_pt_matches=40, min_ls_matches=22), dict(fast_matching=0)])
def test_device_matchers_equal_the_cpu_hooks(kw):
    built = mc.build()
    p = mapmatch_params(**kw)
    dev, _ = hostmap(built, hooks=False)
    cpu, _ = hostmap(built, hooks=True)
    a, b = dev.match_map_to_kf(mc.KF_NEW, built[3], p), cpu.match_map_to_kf(mc.KF_NEW, built[3], p)
    a.pop("match_ms"), b.pop("match_ms")
    assert a == b and a["accepted"][0] >= 15 and a["accepted"][1] >= 5
    assert state(dev, built[0]) == state(cpu, built[0])
    assert dev.check_incremental_gather()


def test_local_mapping_step_from_the_keyframes_features():
    m = make_map(synth.generate("C1L", fixed_frac=0.3), seed=25)
    m.max_kf_idx = len(m.keyframes) - 1 + 5
    kf = len(m.keyframes) - 1
    row = m.full_graph[-1, :-1].astype(np.int64)
    h = HostMap(m, params=SlamParams(min_lm_obs=4, min_lm_cov_graph=int(np.median(row)) + 1, min_kf_local_map=2))
    rng = np.random.default_rng(3)
    n_pt, n_ls = len(m.keyframes[kf].pt_idx), len(m.keyframes[kf].ls_idx)
    spl = rng.uniform([0, 0], [640, 480], (n_ls, 2))
    h.set_keyframe_features(kf, rng.integers(0, 256, (n_pt, 32), dtype=np.uint8), rng.normal(size=(n_pt, 3)) + [0, 0, 5],
                            rng.uniform([0, 0], [640, 480], (n_pt, 2)), rng.integers(0, 256, (n_ls, 32), dtype=np.uint8),
                            rng.normal(size=(n_ls, 3)) + [0, 0, 5], rng.normal(size=(n_ls, 3)) + [0, 0, 5],
                            rng.normal(size=(n_ls, 3)))
    h.set_keyframe_line_endpoints(kf, spl, spl + rng.uniform(-60, 60, (n_ls, 2)))
    h.set_camera(m.fx, m.fy, m.cx, m.cy, 640, 480)
    st = h.local_mapping_step_kf(kf, mapmatch_params())
    assert st["n_free_kf"] > 0 and st["n_ept"] > 0 and st["iters"][0] > 0
    assert st["match"]["unmatched"][0] >= 1
    assert h.check_incremental_gather()
