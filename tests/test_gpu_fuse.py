"""plslam_fuse_landmarks with the default medoid (plba_desc_medoid on the map's context) against the same
with plslam_desc_medoid_cpu: on the scenario of tests/test_host_fuse.py, and inside
plslam_loop_closure_optimization_fuse on the loop map of tests/test_host_pgo.py with the pose graph on the
device too. Integers and copied doubles: equality."""
import numpy as np
import pytest

import fuse_model as FM
from plba.slam_map import LC_IDLE
from test_host_fuse import _loop_map

pytestmark = pytest.mark.gpu


def test_device_medoid_gives_the_model_s_map():
    sc = FM.scenario()
    want, geom, _ = FM.fuse(*sc)
    h = FM.host_map(*sc, medoid=None)
    st = h.fuse_landmarks()
    assert st["medoid_lists"] == 12 and st["erased"] == [3, 3]
    FM.assert_maps_equal(h, want, geom)
    assert h.check_incremental_gather()
    # and the CPU medoid on the same scenario in this process
    h2 = FM.host_map(*sc, medoid="cpu")
    h2.fuse_landmarks()
    FM.assert_maps_equal(h2, want, geom)


def test_long_tracks_take_the_workgroup_path():
    """Two landmarks of 70 observations each fused: a list of 140 descriptors, beyond one wave."""
    m, feats, loops, pt_rows, ls_rows = FM.scenario()
    rng = np.random.default_rng(5)
    for lms in (m.points, m.lines):
        for idx in (5, 6):
            lm = lms[idx]
            n = 70
            base = lm.desc_list[0]
            lm.desc_list = [base ^ np.packbits(rng.random(8 * FM.DB) < 0.05) for _ in range(n)]
            lm.obs_list = [rng.uniform(0, 600, len(lm.obs_list[0])) for _ in range(n)]
            lm.kf_obs_list = [int(v) for v in rng.integers(0, FM.N_KF, n)]
            lm.sigma_list = [1.0] * n
            if lm.dir_list:
                lm.dir_list = [FM.unit(rng.normal(size=3)) for _ in range(n)]
            FM.update_average(lm, bool(lm.dir_list))
    m.map_points_kf_idx = {k: [] for k in range(FM.N_KF)}
    m.map_lines_kf_idx = {k: [] for k in range(FM.N_KF)}
    want, geom, _ = FM.fuse(m, feats, loops, pt_rows, ls_rows)
    assert len(want.points[5].desc_list) == 70 + 70 + 4 + 1
    h = FM.host_map(m, feats, loops, pt_rows, ls_rows, medoid=None)
    h.fuse_landmarks()
    FM.assert_maps_equal(h, want, geom)


def test_optimization_fuse_on_the_device_equals_the_cpu_medoid():
    maps = []
    for medoid in (None, "cpu"):
        h, m, feats, loops, rows = _loop_map()      # the pose graph runs on the device in both
        h.set_medoid_fn(medoid)
        pst, fst = h.loop_closure_fuse(ess=True)
        assert fst["rows"] == [[1, 1, 1, 1], [1, 1, 1, 1]] and fst["medoid_lists"] == 8
        assert h.lc_state() == LC_IDLE and all(int(l[2]) == 0 for l in h.lc_idx_list())
        # a map of the fused shape to read into: the model on the uncorrected map has the same lists
        like, _, _ = FM.fuse(m, feats, loops, [rows], [rows])
        maps.append((h, h.read(like)))
    (h0, a), (h1, b) = maps
    for la, lb in ((a.points, b.points), (a.lines, b.lines)):
        for x, y in zip(la, lb):
            assert (x is None) == (y is None)
            if x is not None:
                assert x.kf_obs_list == y.kf_obs_list and np.array_equal(x.med_desc, y.med_desc)
                assert np.array_equal(np.array(x.obs_list), np.array(y.obs_list))
    assert np.array_equal(a.full_graph, b.full_graph)
    assert a.map_points_kf_idx == b.map_points_kf_idx and a.map_lines_kf_idx == b.map_lines_kf_idx
    assert [k.pt_idx for k in a.keyframes] == [k.pt_idx for k in b.keyframes]
    assert h0.check_incremental_gather()
