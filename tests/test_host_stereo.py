"""Host mirror of the stereo front end (plslam_set_keyframe_stereo) with the CPU hook (plslam_stereo_cpu):
the keyframe ends up with exactly the features that set_keyframe_features + set_keyframe_line_endpoints
would hold given the checker's output, shown by the map-to-keyframe association giving the same result by
either route. No GPU."""
import ctypes as C

import numpy as np
import pytest

import mapmatch_cases as mc
import ref_stereo as RS
import stereo_cases as SC
import test_host_mapmatch as thm
from plba.lib import PlbaError
from plba.slam_map import HostMap

PRM = RS.params(**SC.CAMERA, pluker=1)


@pytest.fixture(scope="module")
def checker():
    f = SC.case("mixed")
    w = RS.associate(f, PRM)
    assert w["n_pt"] > 0 and w["n_ls"] > 0
    return f, w


def _map(w, sized):
    """The map of mapmatch_cases with the new keyframe added for w's feature counts (every idx -1), or, not
    sized, added without idx lists."""
    built = mc.build(seed=3)
    kf = built[0].keyframes[mc.KF_NEW]
    kf.pt_idx, kf.ls_idx = ([-1] * w["n_pt"], [-1] * w["n_ls"]) if sized else ([], [])
    return built


def _associate(h, built):
    for i, L in enumerate(built[1]):
        h.set_line_geometry(i, L, np.zeros(3))
    h.set_camera(*mc.CAM, mc.WIDTH, mc.HEIGHT)
    h.set_grid_match_fn("cpu")
    h.set_match_fn(lambda b, m12, cnt: h.L.plslam_desc_match_cpu(None, C.byref(b), m12, cnt))
    st = h.match_map_to_kf(mc.KF_NEW, built[3])
    st.pop("match_ms", None)
    return st, thm.state(h, built[0])


def test_stereo_route_equals_feature_route(checker):
    f, w = checker
    built = _map(w, True)
    a = HostMap(built[0])
    a.set_stereo_fn("cpu")
    r = a.set_keyframe_stereo(mc.KF_NEW, f, PRM)
    assert (r["n_pt"], r["n_ls"]) == (w["n_pt"], w["n_ls"])
    assert np.array_equal(r["pt_src"], w["pt_src"]) and np.array_equal(r["ls_src"], w["ls_src"])
    b = HostMap(built[0])
    b.set_keyframe_features(mc.KF_NEW, w["pdesc"], w["pt_P"], w["pt_pl"], w["ldesc"], w["ls_sP"], w["ls_eP"], w["ls_le"])
    b.set_keyframe_line_endpoints(mc.KF_NEW, w["ls_spl"], w["ls_epl"])
    ra, rb = _associate(a, built), _associate(b, built)
    assert ra == rb
    assert ra[0]["unmatched"] == [w["n_pt"], w["n_ls"]]
    a.close()
    b.close()


def test_keyframe_added_without_idx_lists_is_sized(checker):
    f, w = checker
    built = _map(w, False)
    h = HostMap(built[0])
    h.set_stereo_fn("cpu")
    r = h.set_keyframe_stereo(mc.KF_NEW, f, PRM)
    assert (r["n_pt"], r["n_ls"]) == (w["n_pt"], w["n_ls"])
    pi, li = np.zeros(w["n_pt"] + 1, np.int32), np.zeros(w["n_ls"] + 1, np.int32)
    ip = C.POINTER(C.c_int32)
    h._check(h.L.plslam_get_keyframe(h.h, mc.KF_NEW, None, None, pi.ctypes.data_as(ip), w["n_pt"], li.ctypes.data_as(ip),
                                     w["n_ls"]), "get_keyframe")
    assert pi[:-1].tolist() == [-1] * w["n_pt"] and li[:-1].tolist() == [-1] * w["n_ls"]
    h.close()


def test_refusals_leave_the_keyframe_untouched(checker):
    f, w = checker
    built = _map(w, True)
    built[0].keyframes[mc.KF_NEW].pt_idx = [-1] * (w["n_pt"] + 1)    # added with another count
    h = HostMap(built[0])
    h.set_stereo_fn("cpu")
    with pytest.raises(PlbaError):
        h.set_keyframe_stereo(mc.KF_NEW, f, PRM)
    with pytest.raises(PlbaError):
        h.set_keyframe_stereo(17, f, PRM)                            # no such keyframe
    bad = {k: np.array(v) for k, v in f.items()}
    bad["pt_l"][0, 0] = np.nan
    with pytest.raises(PlbaError):
        h.set_keyframe_stereo(mc.KF_NEW, bad, PRM)
    with pytest.raises(PlbaError):                                   # still without features
        h.set_camera(*mc.CAM, mc.WIDTH, mc.HEIGHT)
        h.match_map_to_kf(mc.KF_NEW, built[3])
    h.close()


def test_python_hook_sees_the_one_frame(checker):
    f, w = checker
    built = _map(w, True)
    h = HostMap(built[0])
    seen = []

    def hook(b, p, o):
        seen.append((b.n, b.pt_off_l[1], b.pt_off_r[1], b.ls_off_l[1], b.ls_off_r[1], p.matching_s_ws, p.pluker))
        return h.L.plslam_stereo_cpu(None, C.byref(b), C.byref(p), C.byref(o))
    h.set_stereo_fn(hook)
    r = h.set_keyframe_stereo(mc.KF_NEW, f, PRM)
    assert seen == [(1, len(f["pt_l"]), len(f["pt_r"]), len(f["ls_l"]), len(f["ls_r"]), 10, 1)]
    assert (r["n_pt"], r["n_ls"]) == (w["n_pt"], w["n_ls"])
    h.close()
