"""plslam_map_assoc_cpu (the restatement of plba_map_associate) against the checker tests/ref_mapassoc.py, bit
for bit; plslam_match_map_to_kf_assoc with the CPU hook against plslam_match_map_to_kf with its CPU hooks on the
map of tests/mapmatch_cases.py; and the refusals. Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import mapassoc_cases as MC
import mapmatch_cases as mc
import ref_mapassoc as RM
import test_host_mapmatch as TM
import test_mapassoc_oracle as TO
from plba import capi, slam_map
from plba.slam_map import PlbaError, mapassoc_params, mapmatch_params

prm, want, MODES = TO.prm, TO.want, TO.MODES


def cpu(name, mode):
    return slam_map.map_assoc_cpu([MC.case(name)], prm(**MODES[mode]))[0]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(MC.CASES))
def test_cpu_equals_checker(name, mode):
    assert RM.same(want(name, mode), cpu(name, mode)) is None


def test_branches_are_reached_by_the_restatement():
    TO.test_branches_are_reached(cpu)


def hand_cases():
    """(name, keyframe, parameter overrides) of the hand cases of the oracle file"""
    out = [("point", MC.hand_point(), {}), ("point rejected", MC.hand_point(), dict(max_kf_epip_p=0.625)),
           ("boundary points", MC.boundary_points()[0], {}), ("boundary lines", MC.boundary_lines()[0], {}),
           ("masking, grid", MC.masking_keyframe(), {}),
           ("masking, fallback", MC.masking_keyframe(), dict(fast_matching=0, min_pt_matches=1)),
           ("two on one", MC.two_on_one_keyframe(), dict(best_lr=0)), ("two on one, best_lr", MC.two_on_one_keyframe(), {})]
    for le in ([0.0, 1.0, -400.25], [0.0, -1.0, 401.5], [0.0, 1.0, -1400.0], [0.004, -1.0, 399.72]):
        out.append((f"line {le}", MC.hand_line(le), {}))
    return out


@pytest.mark.parametrize("name, kf, over", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_cases_equal_the_checker(name, kf, over):
    assert RM.same(RM.associate(kf, prm(**over)), slam_map.map_assoc_cpu([kf], prm(**over))[0]) is None


def test_batch_equals_single_calls():
    names = ["mixed", "pts_far", "empty_sides", "lines_40x70"]
    got = slam_map.map_assoc_cpu([MC.case(n) for n in names], prm())
    for n, g in zip(names, got):
        assert RM.same(want(n, "default"), g) is None, n


def test_c_defaults_are_those_of_the_checker():
    p = capi.mapassoc_params()
    for k, v in RM.DEFAULTS.items():
        assert getattr(p, k) == v, k
    for k in ("width", "height", "fx", "fy", "cx", "cy"):
        assert getattr(p, k) == 0
    assert C.sizeof(p) == 10 * 4 + 9 * 8 and C.sizeof(capi.PlbaMapassocBatch) == 8 + 19 * 8 and C.sizeof(capi.PlbaMapassocOut) == 13 * 8


def refusals():
    """(name, keyframes, view patch or None, params overrides, desc_bytes)"""
    f = MC.case("mixed")

    def with_value(key, idx, value):
        g = {k: np.array(v) for k, v in f.items()}
        g[key][idx] = value
        return g
    big = dict(MC.identity_poses(), pt_X=np.ones((1, 3)), pdesc_m=np.zeros((1, 32), np.uint8), pt_pl=np.ones((65536, 2)),
               pt_P=np.ones((65536, 3)), pdesc_f=np.zeros((65536, 32), np.uint8))

    def patch(fn):
        return fn
    d6 = {k: (np.zeros((len(v), 6), np.uint8) if "desc" in k else v) for k, v in f.items()}
    return [
        ("nan point feature", [with_value("pt_pl", (3, 1), np.nan)], None, {}, None),
        ("inf line feature", [with_value("ls_epl", (2, 0), np.inf)], None, {}, None),
        ("point feature beyond one image size", [with_value("pt_pl", (0, 1), 2.0 * MC.HEIGHT + 1.0)], None, {}, None),
        ("line feature beyond one image size", [with_value("ls_spl", (0, 0), -MC.WIDTH - 1.0)], None, {}, None),
        ("Twf not finite", [with_value("Twf", (1, 3), np.nan)], None, {}, None),
        ("T_kf_w not finite", [with_value("T_kf_w", (0, 0), np.inf)], None, {}, None),
        ("negative offset", [f], patch(lambda bv: bv.off["pt_f"].__setitem__(0, -1)), {}, None),
        ("decreasing offset", [f], patch(lambda bv: bv.off["ls_m"].__setitem__(1, -2)), {}, None),
        ("NULL input array with rows", [f], patch(lambda bv: setattr(bv.struct, "ls_le", None)), {}, None),
        ("NULL offset array", [f], patch(lambda bv: setattr(bv.struct, "pt_off_m", None)), {}, None),
        ("NULL required output", [f], patch(lambda bv: setattr(bv.out, "n_visible", None)), {}, None),
        ("NULL poses", [f], patch(lambda bv: setattr(bv.struct, "Twf", None)), {}, None),
        ("n < 0", [f], patch(lambda bv: setattr(bv.struct, "n", -1)), {}, None),
        ("desc_bytes 6", [d6], None, {}, 6),
        ("65536 feature rows", [big], None, {}, None),
        ("ws < 0", [f], None, dict(ws=-1), None),
        ("ws 2^30", [f], None, dict(ws=1 << 30), None),
        ("no image width", [f], None, dict(width=0), None),
        ("no image height", [f], None, dict(height=-1), None),
        ("no grid columns", [f], None, dict(cols=0), None),
        ("no grid rows", [f], None, dict(rows=0), None),
    ]


@pytest.mark.parametrize("name, kfs, patch, over, db", refusals(), ids=[r[0] for r in refusals()])
def test_map_assoc_cpu_refusals(name, kfs, patch, over, db):
    bv = capi.MapassocBatchView(kfs, db)
    if patch:
        patch(bv)
    with pytest.raises(PlbaError):
        slam_map.map_assoc_cpu(bv, prm(**over))


def test_null_batch_params_out_and_the_empty_batch():
    L = slam_map.load_host()
    bv = capi.MapassocBatchView([MC.case("mixed")])
    p = capi.mapassoc_params(prm())
    assert L.plslam_map_assoc_cpu(None, None, C.byref(p), C.byref(bv.out)) != 0
    assert L.plslam_map_assoc_cpu(None, C.byref(bv.struct), None, C.byref(bv.out)) != 0
    assert L.plslam_map_assoc_cpu(None, C.byref(bv.struct), C.byref(p), None) != 0
    assert slam_map.map_assoc_cpu([], prm()) == []


def test_a_landmark_that_is_not_finite_is_invisible_not_refused():
    f = {k: np.array(v) for k, v in MC.case("mixed").items()}
    f["pt_X"][0] = [np.inf, 0.0, 1.0]
    f["ls_X"][0, 4] = np.nan
    got = slam_map.map_assoc_cpu([f], prm())[0]
    assert got["pt_visible"][0] == 0 and got["ls_visible"][0] == 0 and RM.same(RM.associate(f, prm()), got) is None


# ---- the host mirror: one association call against the two matcher calls of match_map_to_kf
def assoc_hostmap(built, hook="cpu"):
    h, _ = TM.hostmap(built, hooks=False)
    if hook:
        h.set_mapassoc_fn(hook)
    return h


def assert_same_state(a, b):
    """Indices, flags, lists and full_graph exactly; the stored directions to rtol 1e-14: the two paths may order
    the three-term sum of T_kf_w.R d differently, a few roundings on unit-scale values."""
    assert a["kf"] == b["kf"] and a["ln"] == b["ln"] and a["full_graph"] == b["full_graph"] and a["pt"].keys() == b["pt"].keys()
    for idx, x in a["pt"].items():
        y = b["pt"][idx]
        assert x[0] == y[0] and x[1] == y[1] and x[3] == y[3] and x[4] == y[4], idx
        assert np.shape(x[2]) == np.shape(y[2])
        np.testing.assert_allclose(x[2], y[2], rtol=1e-14, atol=0)


@pytest.mark.parametrize("kw", [dict(), dict(ws=0, min_pt_matches=40, min_ls_matches=22), dict(fast_matching=0)])
def test_one_call_leaves_the_map_of_the_two_matcher_calls(kw):
    built = mc.build()
    legacy, _ = TM.hostmap(built, hooks=True)
    new = assoc_hostmap(built)
    a = legacy.match_map_to_kf(mc.KF_NEW, built[3], mapmatch_params(**kw))
    b = new.match_map_to_kf_assoc(mc.KF_NEW, built[3], mapassoc_params(**kw))
    a.pop("match_ms"), b.pop("match_ms")
    assert a == b and a["accepted"][0] >= 15 and a["accepted"][1] >= 5 and a["rejected"][0] >= 1
    if kw:
        assert a["fallback"] == [1, 1]
    assert_same_state(TM.state(new, built[0]), TM.state(legacy, built[0]))
    assert new.check_incremental_gather()
    # a second call finds the matched landmarks already observed by the keyframe
    b2 = new.match_map_to_kf_assoc(mc.KF_NEW, built[3], mapassoc_params(**kw))
    assert b2["accepted"] == [0, 0] and b2["unmatched"][0] == b["unmatched"][0] - b["accepted"][0]


def test_twf_defaults_to_the_inverse_of_the_keyframe_pose():
    built = mc.build()
    h, h2 = assoc_hostmap(built), assoc_hostmap(built)
    a, b = h.match_map_to_kf_assoc(mc.KF_NEW, None), h2.match_map_to_kf_assoc(mc.KF_NEW, built[3])
    a.pop("match_ms"), b.pop("match_ms")
    assert a == b and TM.state(h, built[0]) == TM.state(h2, built[0])


def test_invalid_arguments_and_hook_answers_leave_the_map_unchanged():
    built = mc.build()
    for kw, kf in ((dict(), 7), (dict(), -1), (dict(features=False, endpoints=False), mc.KF_NEW), (dict(endpoints=False), mc.KF_NEW),
                   (dict(camera=False), mc.KF_NEW), (dict(), 1)):
        h, _ = TM.hostmap(built, hooks=False, **kw)
        h.set_mapassoc_fn("cpu")
        before = TM.state(h, built[0])
        with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
            h.match_map_to_kf_assoc(kf, built[3])
        assert TM.state(h, built[0]) == before
    h = assoc_hostmap(built)
    before = TM.state(h, built[0])
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.match_map_to_kf_assoc(mc.KF_NEW, built[3], mapassoc_params(ws=-1))
    h.set_mapassoc_fn(lambda b, p, o: -1)   # a failing hook
    with pytest.raises(PlbaError):
        h.match_map_to_kf_assoc(mc.KF_NEW, built[3])

    def wild(b, p, o):   # a hook that answers outside the features
        for k in range(2):
            o.n_visible[k], o.n_grid[k], o.n_matches[k], o.fallback[k], o.n_accepted[k] = 1, 1, 1, 0, 1
        o.pt_m12[0] = 10 ** 6
        return 0
    h.set_mapassoc_fn(wild)
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        h.match_map_to_kf_assoc(mc.KF_NEW, built[3])
    assert TM.state(h, built[0]) == before and h.check_incremental_gather()
