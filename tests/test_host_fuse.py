"""Host mirror of MapHandler::loopClosureFuseLandmarks (plslam_fuse_landmarks) with the CPU medoid
(plslam_desc_medoid_cpu) against the Python model tests/fuse_model.py on a map of 6 keyframes and 13
landmarks of each kind: the four cases for points and lines, a loop with flag 0, the NULL guards, a
landmark erased by one row and named by later ones, the lm_idx0 == lm_idx1 row, full_graph, the kf-idx
lists, the new indices, the feature indices, med_desc / med_obs_dir and the incremental gather. Integers
and doubles computed in the same order: equality. Runs without a GPU."""
import numpy as np
import pytest

import fuse_model as FM
import ref_medoid as RM
from plba import pgo
from plba.lib import PlbaError
from plba.slam_map import LC_IDLE, HostMap
from test_host_pgo import _oracle_hook


@pytest.fixture(scope="module")
def fused():
    """The scenario, the model's result (computed once) and the host map after plslam_fuse_landmarks."""
    sc = FM.scenario()
    want, geom, st = FM.fuse(*sc)
    h = FM.host_map(*sc)
    return dict(sc=sc, want=want, geom=geom, model_stats=st, h=h, stats=h.fuse_landmarks())


def test_map_equals_the_model(fused):
    FM.assert_maps_equal(fused["h"], fused["want"], fused["geom"])


def test_stats_count_every_case_and_guard(fused):
    st, ms = fused["stats"], fused["model_stats"]
    for k in ("rows", "null_skipped", "same_landmark", "erased"):
        assert st[k] == ms[k], k
    # the scenario reaches each case, each guard and the equal-index row, for points and for lines
    assert st["rows"] == [[3, 1, 2, 3], [3, 1, 2, 3]]
    assert st["null_skipped"] == [[1, 2, 0, 2], [1, 2, 0, 2]]
    assert st["same_landmark"] == [1, 1] and st["erased"] == [3, 3]
    assert st["loops"] == 2 and st["loops_skipped"] == 1
    # landmarks 3, 4, 5, 12 and the two new ones of each kind: one list each in the one medoid batch
    assert st["medoid_lists"] == 12


def test_scenario_holds_what_it_is_meant_to(fused):
    m0, feats = fused["sc"][0], fused["sc"][1]
    want = fused["want"]
    for before, after in ((m0.points, want.points), (m0.lines, want.lines)):
        assert after[6] is None and after[9] is None and after[13] is None and after[10] is None
        assert len(after) == len(before) + 2
        assert len(after[5].kf_obs_list) == 3 + 3 + 4 + 1       # 5 <- 6, 5 <- 9, one observation
        assert after[7].kf_obs_list == before[7].kf_obs_list    # guarded rows changed nothing
        assert after[8].kf_obs_list == before[8].kf_obs_list    # lm_idx0 == lm_idx1
        assert after[3].kf_obs_list == before[3].kf_obs_list + [0, 1]   # loops 0 and 2
    assert 6 not in want.map_points_kf_idx[3] and 6 in m0.map_points_kf_idx[3]
    assert want.map_points_kf_idx[0][-2:] == [15, 16] and want.map_lines_kf_idx[0][-2:] == [15, 16]
    # the flag-0 loop (1, 4): its rows would have made a landmark and fused 1 into 0
    assert want.points[1] is not None and want.keyframes[4].pt_idx[0] == m0.keyframes[4].pt_idx[0]
    # case 0 increments full_graph against kf_curr_idx although the observation is kf_prev_idx's (:5562)
    assert want.keyframes[0].pt_idx[0] == 3 and want.points[3].kf_obs_list[-2] == 0
    # the new line's second observation: the current keyframe's spl and the previous keyframe's epl (:5747)
    obs = want.lines[15].obs_list[1]
    assert np.array_equal(obs[:2], feats[5]["spl"][2]) and np.array_equal(obs[2:], feats[0]["epl"][2])
    assert not np.array_equal(obs[2:], feats[5]["epl"][2])


def test_only_the_last_average_is_observable(fused):
    """The model updates after every append; the same lists averaged once give the same fields."""
    for lm in (fused["want"].points[5], fused["want"].lines[5], fused["want"].points[15]):
        assert np.array_equal(lm.med_desc, lm.desc_list[RM.medoid(np.array(lm.desc_list))])


def test_incremental_gather_equals_the_scan_afterwards(fused):
    assert fused["h"].check_incremental_gather()


def test_fuse_twice_with_cleared_flags_changes_nothing(fused):
    sc = FM.scenario()
    h = FM.host_map(*sc)
    h.fuse_landmarks()
    h.set_loop_closure([[a, b, 0] for a, b, _ in sc[2]], [[a, b, 0] for a, b, _ in sc[2]], np.zeros((3, 6)))
    st = h.fuse_landmarks()
    assert st["loops"] == 0 and st["loops_skipped"] == 3 and st["medoid_lists"] == 0
    FM.assert_maps_equal(h, fused["want"], fused["geom"])


def test_python_medoid_hook_sees_one_batch(fused):
    sc = FM.scenario()
    calls = []

    def hook(b, med):
        ptr = [b.list_ptr[i] for i in range(b.n + 1)]
        desc = np.ctypeslib.as_array(b.desc, (ptr[-1] * b.desc_bytes,)).reshape(-1, b.desc_bytes)
        calls.append(ptr)
        for i, v in enumerate(RM.medoids(ptr, desc, b.desc_bytes)):
            med[i] = int(v)
        return 0
    h = FM.host_map(*sc, medoid=hook)
    h.fuse_landmarks()
    assert len(calls) == 1 and len(calls[0]) == 13
    FM.assert_maps_equal(h, fused["want"], fused["geom"])


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("row, what", [((-1, FM.N_FEAT, 3, 0), "features"), ((4, 0, -1, FM.N_FEAT), "features"),
                                       ((-1, -1, 3, 0), "features"), ((99, 0, -1, 0), "outside the map"),
                                       ((-2, 0, 3, 0), "outside the map")])
def test_an_index_out_of_range_is_refused_and_the_map_unchanged(kind, row, what):
    m, feats, loops, pt_rows, ls_rows = FM.scenario()
    rows = [list(r) for r in (pt_rows if kind == 1 else ls_rows)]
    rows[2] = rows[2] + [row]           # after rows that would have changed the map
    h = FM.host_map(m, feats, loops, rows if kind == 1 else pt_rows, rows if kind == 2 else ls_rows)
    with pytest.raises(PlbaError, match=what):
        h.fuse_landmarks()
    FM.assert_maps_equal(h, m)


def test_new_line_reads_the_previous_keyframe_at_lm_ldx1():
    """stereo_ls[lm_ldx1] of the previous keyframe (:5747) must exist: a previous keyframe with fewer lines."""
    m, feats, loops, pt_rows, ls_rows = FM.scenario()
    m.keyframes[1].ls_idx = m.keyframes[1].ls_idx[:4]
    feats[1] = {k: (v[:4] if k in ("ldesc", "sP", "eP", "le", "spl", "epl") else v) for k, v in feats[1].items()}
    ls_rows[2] = [(-1, 0, -1, 6)]       # loop (1, 5): feature 6 of kf 5 exists, line 6 of kf 1 does not
    h = FM.host_map(m, feats, loops, pt_rows, ls_rows)
    with pytest.raises(PlbaError, match="features"):
        h.fuse_landmarks()
    FM.assert_maps_equal(h, m)


# ---- with the pose graph: plslam_loop_closure_optimization_fuse against plslam_loop_closure_optimization
def _loop_map():
    """The loop map of tests/test_host_pgo.py with features on both keyframes of its loop and rows of
    every case. Returns (HostMap, SlamMap, feats, loops, rows)."""
    m, lc_idxs, lc_idx_list, lc_pose_list, line3d = pgo.loop_map(n_loop=12, n_after=2, seed=3)
    kp, kc = int(lc_idx_list[0][0]), int(lc_idx_list[0][1])
    sc = FM.scenario()
    feats = {kp: sc[1][0], kc: sc[1][5]}
    n_pt, n_ln = len(m.points), len(m.lines)
    rows = [(-1, 0, 1, 0), (2, 1, -1, 1), (-1, 2, -1, 2), (3, 3, 4, 3), (4, 4, -1, 4), (5, 5, 5, 5)]
    assert n_pt > 5 and n_ln > 5
    for k in (kp, kc):
        m.keyframes[k].pt_idx = [-1] * FM.N_FEAT
        m.keyframes[k].ls_idx = [-1] * FM.N_FEAT
    h = HostMap(m)
    for i, L in enumerate(line3d):
        h.set_line_geometry(i, L, L[:3] * 0.5)
    for k, f in feats.items():
        h.set_keyframe_features(k, f["pdesc"], f["P"], f["pl"], f["ldesc"], f["sP"], f["eP"], f["le"])
        h.set_keyframe_line_endpoints(k, f["spl"], f["epl"])
    h.set_loop_closure(lc_idxs, lc_idx_list, lc_pose_list)
    h.set_lc_feature_idxs(1, 0, rows)
    h.set_lc_feature_idxs(2, 0, rows)
    return h, m, feats, [[int(v) for v in l] for l in lc_idx_list], rows


def test_optimization_fuse_ends_idle_with_flags_cleared_and_the_map_fused():
    h, m, feats, loops, rows = _loop_map()
    h.set_pgo_solver(_oracle_hook({}))
    h.set_medoid_fn("cpu")
    pst, fst = h.loop_closure_fuse(ess=True)
    assert pst["n_loop_edges"] == len(loops) and fst["loops"] == 1
    assert fst["rows"] == [[1, 1, 1, 1], [1, 1, 1, 1]] and fst["erased"] == [1, 1] and fst["same_landmark"] == [1, 1]
    assert fst["null_skipped"][0][1] == 1                    # row (4, 4, -1, 4) after 4 was erased
    assert h.lc_state() == LC_IDLE and all(int(l[2]) == 0 for l in h.lc_idx_list())
    assert not h.exists(1, 4) and not h.exists(2, 4) and h.exists(1, len(m.points)) and h.exists(2, len(m.lines))
    # the fuse ran on the corrected map: the model on the map that the optimisation alone leaves
    h2, m2, feats2, loops2, rows2 = _loop_map()
    h2.set_pgo_solver(_oracle_hook({}))
    h2.loop_closure(ess=True)
    corrected = h2.read(m2)
    for kind, (lw, l0) in enumerate(((corrected.points, m2.points), (corrected.lines, m2.lines))):
        for a, b in zip(lw, l0):       # read() returns no descriptors or line directions: the originals
            if a is not None:
                a.desc_list = [d.copy() for d in b.desc_list]
                if kind == 1:
                    a.dir_list = []
    want, geom, _ = FM.fuse(corrected, feats2, loops2, [rows2], [rows2])
    FM.assert_maps_equal(h, want, geom)
    assert h.check_incremental_gather()


def test_optimization_alone_leaves_the_landmarks_unfused():
    h, m, feats, loops, rows = _loop_map()
    h.set_pgo_solver(_oracle_hook({}))
    fg0 = h.read(m).full_graph.copy()
    h.loop_closure(ess=True)
    after = h.read(m)
    assert h.lc_state() == LC_IDLE and all(int(l[2]) == 0 for l in h.lc_idx_list())
    assert h.exists(1, 4) and h.exists(2, 4) and not h.exists(1, len(m.points)) and not h.exists(2, len(m.lines))
    assert np.array_equal(after.full_graph, fg0)
    for a, b in zip(after.points + after.lines, m.points + m.lines):
        if b is not None:
            assert a.kf_obs_list == list(b.kf_obs_list)
    # and a fuse afterwards finds every flag cleared
    h.set_medoid_fn("cpu")
    assert h.fuse_landmarks()["loops"] == 0
