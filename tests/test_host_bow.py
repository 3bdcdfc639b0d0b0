"""Host mirror of place recognition (insertKFBowVectorP / L / PL, lookForLoopCandidates, loopClosure()
whole; src/mapHandler.cpp:4053-4301) on the CPU: the place-recognition hook is plslam_bow_cpu, the
matcher and relative-pose hooks are the checkers of tests/test_host_isloopclosure.py. Everything is
compared with the plain-Python checker (tests/ref_bow.py) as bytes. tests/test_gpu_bow.py runs the
same end to end on the device."""
import ctypes as C

import numpy as np
import pytest

import bow_cases as cases
import descmatch_cases as dcases
import ref_bow as R
from plba import pgo
from plba.lib import PlbaError
from plba.slam_map import LC_ACTIVE, LC_IDLE, BowCpu, HostMap, lc_search_params, match_params
from test_host_isloopclosure import _idx, lcpose_hook, match_hook
from test_host_pgo import _oracle_hook

N_KF, KF_CURR, KF_PREV = 14, 13, 2
SMALL = lc_search_params(**cases.SMALL)


def _vec_bytes(vec):
    w, v = cases.as_arrays(vec)
    return w.tobytes(), v.tobytes()


@pytest.mark.parametrize("name", cases.VOCABS)
def test_the_cpu_restatement_equals_the_checker(name):
    b = BowCpu()
    b.set_vocab(0, cases.vocab(name))
    stored = []
    for kf, n in enumerate(cases.N_DESC):
        vec = cases.reference_vector(name, n)
        ids, scores = b.insert(0, kf, cases.descriptors(name, n))
        assert ids.tolist() == list(range(kf + 1))
        assert scores.tobytes() == np.array([R.score(vec, o) for o in stored] + [R.score(vec, vec)]).tobytes()
        got = b.get(0, kf)
        assert (got[0].tobytes(), got[1].tobytes()) == _vec_bytes(vec)
        stored.append(vec)
    b.remove(0, 3)
    ids, scores = b.insert(0, 50, cases.descriptors(name, 65))
    assert ids.tolist() == [0, 1, 2, 4, 5, 6, 50]
    with pytest.raises(PlbaError):
        b.get(0, 3)
    b.close()


def test_the_cpu_restatement_on_the_constructed_cases_and_bad_vocabularies():
    b = BowCpu()
    voc, q, first, _ = cases.tie_case()
    b.set_vocab(0, voc)
    b.insert(0, 0, q)
    assert b.get(0, 0)[0].tolist() == [int(voc["word_id"][first])]
    for count in (6, 10):
        voc, q = cases.sum_case(count)
        b.set_vocab(0, voc)
        b.insert(0, 0, q)
        got = b.get(0, 0)
        assert (got[0].tobytes(), got[1].tobytes()) == _vec_bytes(R.transform(voc, q))
    voc, a, d = cases.disjoint_case()
    b.set_vocab(1, voc)
    b.insert(1, 0, a)
    s = b.insert(1, 1, d)[1]
    assert s[0] == 0.0 and np.signbit(s[0])
    for why, bad in cases.malformed().items():
        with pytest.raises(PlbaError):
            b.set_vocab(1, bad)
    assert b.get(1, 1)[0].size        # the refused vocabularies left the slot as it was
    b.close()


def bow_hostmap(n_kf, feats, bow=True):
    """A loop map of n_kf keyframes with the features of ``feats`` (kf_idx -> dict with pdesc, ldesc,
    pl, spl, epl and optionally P, sP, eP, le), the vocabularies set and every hook on the CPU."""
    m, _, _, _, line3d = pgo.loop_map(n_loop=n_kf, n_after=0, seed=3)
    for k, f in feats.items():
        m.keyframes[k].pt_idx, m.keyframes[k].ls_idx = _idx(k, len(f["pdesc"]), 1), _idx(k, len(f["ldesc"]), 2)
    h = HostMap(m)
    for i, L in enumerate(line3d):
        h.set_line_geometry(i, L, L[:3] * 0.5)
    for k, f in feats.items():
        n_pt, n_ls = len(f["pdesc"]), len(f["ldesc"])
        z = lambda key, n, w: f[key] if key in f else np.zeros((n, w))
        h.set_keyframe_features(k, f["pdesc"], z("P", n_pt, 3), f["pl"], f["ldesc"], z("sP", n_ls, 3), z("eP", n_ls, 3),
                                z("le", n_ls, 3))
        h.set_keyframe_line_endpoints(k, f["spl"], f["epl"])
    calls = dict(match=[], pose=[])
    h.set_match_fn(match_hook(calls["match"]))
    h.set_lcpose_solver(lcpose_hook(calls["pose"], accept_all=True))
    h.set_pgo_solver(_oracle_hook({}))
    cpu = None
    if bow:
        cpu = BowCpu()
        h.set_bow_cpu(cpu)
        h.set_vocabulary(0, cases.vocab("k10L3"))
        h.set_vocabulary(1, cases.vocab("lines"))
    return h, cpu, calls


@pytest.mark.parametrize("mode,empty_kf", [("P", -1), ("L", -1), ("PL", -1), ("PL", 9)])
def test_the_float_conf_matrix_after_12_inserts_with_a_culled_keyframe(mode, empty_kf):
    ref = cases.reference_map(mode, empty_kf=empty_kf)
    feats = {i: (cases.keyframe(i, 0, 0) if i == empty_kf else cases.keyframe(i)) for i in range(12)}
    h, cpu, _ = bow_hostmap(12, feats)
    for i in range(12):
        h.insert_kf_bow(i, "P" in mode, "L" in mode)
        if i == 6:
            h.remove_keyframe(4)
    conf = h.conf_matrix()
    assert conf.dtype == np.float32 and conf.tobytes() == ref.conf.tobytes(), np.argwhere(conf != ref.conf)[:5]
    if empty_kf >= 0:
        assert np.isnan(conf[9, 0]) and np.isnan(conf[0, 9])
    # the vectors are KeyFrame::descDBoW_P / _L; the culled keyframe left the database
    for slot, on in ((0, "P" in mode), (1, "L" in mode)):
        if on:
            got = cpu.get(slot, 7)
            assert (got[0].tobytes(), got[1].tobytes()) == _vec_bytes(ref.vec[7][slot])
            with pytest.raises(PlbaError):
                cpu.get(slot, 4)
    h.close()


def _set_search_inputs(h, conf, fg, live):
    n = len(conf)
    h.set_conf_matrix(conf)
    g = np.ascontiguousarray(fg, np.uint32)
    assert h.L.plslam_set_full_graph(h.h, n, g.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    for i, on in enumerate(live):
        if not on:
            h.remove_keyframe(i)


@pytest.mark.parametrize("kind", cases.SEARCH_KINDS)
def test_the_candidate_search_takes_every_exit(kind):
    conf, fg, live, cur, p, expected = cases.search_case(kind)
    h, _, _ = bow_hostmap(N_KF, {}, bow=False)
    _set_search_inputs(h, conf, fg, live)
    ref = R.look_for_loop_candidates(conf, fg, live, cur, **p)
    assert ref[2] == expected
    assert h.look_for_loop_candidates(cur, lc_search_params(**p)) == ref[:2]
    if kind == "accepted":      # a covisible old keyframe lowers lc_min_score
        conf, fg = conf.copy(), fg.copy()
        conf[5, cur] = conf[cur, 5] = 0.02
        fg[5, cur] = fg[cur, 5] = 75
        _set_search_inputs(h, conf, fg, live)
        assert h.look_for_loop_candidates(cur, lc_search_params(**p)) == R.look_for_loop_candidates(conf, fg, live, cur, **p)[:2]
    h.close()


def test_the_candidate_search_with_the_default_parameters():
    h, _, _ = bow_hostmap(120, {}, bow=False)
    for kind in ("accepted", "too_few_neighbours"):
        conf, fg, live, cur, p, expected = cases.search_case(kind, n=120, params=R.DEFAULT_SEARCH)
        _set_search_inputs(h, conf, fg, live)
        ref = R.look_for_loop_candidates(conf, fg, live, cur)
        assert ref[2] == expected and h.look_for_loop_candidates(cur) == ref[:2]
    h.close()


def loop_features():
    """14 keyframes: 13 sees the place of 2 again (descmatch_cases.keyframe_pair), the others are
    unrelated; pixels and line endpoints for the PL dispersion."""
    kf0, kf1, _ = dcases.keyframe_pair()
    feats = {}
    for k in range(N_KF):
        f = dict(kf0 if k == KF_PREV else kf1 if k == KF_CURR else dcases.unrelated_keyframe(seed=k))
        rng = np.random.default_rng(900 + k)
        f["spl"], f["epl"] = rng.uniform(0, 640, (len(f["ldesc"]), 2)), rng.uniform(0, 640, (len(f["ldesc"]), 2))
        feats[k] = f
    return feats


def reference_loop_conf(feats):
    m = R.Map(cases.vocab("k10L3"), cases.vocab("lines"))
    for k in range(N_KF):
        f = feats[k]
        m.insert(k, f["pdesc"], f["ldesc"], True, True, f["pl"], f["spl"], f["epl"])
    return m.conf


def test_loop_closure_whole_from_descriptors_and_its_state_machine():
    feats = loop_features()
    h, _, calls = bow_hostmap(N_KF, feats)
    for k in range(N_KF):
        h.insert_kf_bow(k)
    conf = h.conf_matrix()
    ref_conf = reference_loop_conf(feats)
    assert conf.tobytes() == ref_conf.tobytes()
    fg = np.zeros((N_KF, N_KF), np.uint32)
    assert h.L.plslam_get_full_graph(h.h, N_KF, fg.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    ref = R.look_for_loop_candidates(ref_conf, fg, [True] * N_KF, KF_CURR, **cases.SMALL)
    assert ref[:2] == (True, KF_PREV), ref
    assert h.look_for_loop_candidates(KF_CURR, SMALL) == (True, KF_PREV)
    assert h.lc_state() == LC_IDLE
    n_loops = len(h.lc_idx_list())
    st = h.loop_closure_kf(KF_CURR, SMALL, match_params())
    assert st["is_candidate"] == 1 and st["accepted"] == 1 and (st["state_before"], st["state_after"]) == (LC_IDLE, LC_ACTIVE)
    assert h.lc_idx_list()[-1].tolist() == [KF_PREV, KF_CURR, 1] and len(h.lc_idx_list()) == n_loops + 1
    assert len(calls["match"]) == 1 and len(calls["pose"]) == 1
    # no candidate (more neighbours asked for than there are): ACTIVE -> READY, the pose graph runs, -> IDLE
    none = lc_search_params(**dict(cases.SMALL, lc_nkf_closest=100))
    assert h.look_for_loop_candidates(KF_CURR, none) == (False, -1)
    st = h.loop_closure_kf(KF_CURR, none, match_params())
    assert st["is_candidate"] == 0 and st["pgo_ran"] == 1 and (st["state_before"], st["state_after"]) == (LC_ACTIVE, LC_IDLE)
    assert len(calls["match"]) == 1      # the c == NULL branch matches nothing
    h.close()


def test_bad_arguments_leave_the_map_untouched():
    feats = {i: cases.keyframe(i) for i in range(4)}
    h, cpu, _ = bow_hostmap(12, feats)
    h.insert_kf_bow(0)
    h.insert_kf_bow(1)
    before = h.conf_matrix().tobytes()
    for args in ((2, False, False), (-1, True, True), (12, True, True), (5, True, True), (1, True, True)):
        with pytest.raises(PlbaError):          # neither kind; no such keyframe; no features; inserted before
            h.insert_kf_bow(*args)
    with pytest.raises(PlbaError):
        h.set_vocabulary(2, cases.vocab("lines"))
    with pytest.raises(PlbaError):
        h.set_vocabulary(1, cases.malformed()["cycle"])
    for kw in ("lc_kf_dist", "lc_kf_max_dist", "lc_nkf_closest", "min_lm_cov_graph", "min_kf_local_map"):
        with pytest.raises(PlbaError):
            h.look_for_loop_candidates(1, lc_search_params(**{kw: -1}))
    for cur in (-1, 2, 99):                     # outside conf_matrix
        with pytest.raises(PlbaError):
            h.look_for_loop_candidates(cur, SMALL)
    with pytest.raises(PlbaError):
        h.loop_closure_kf(99, SMALL, match_params())
    assert h.conf_matrix().tobytes() == before and h.lc_state() == LC_IDLE
    h.insert_kf_bow(2)                          # and the next valid call is right
    assert h.conf_matrix().tobytes() == cases.reference_map("PL", n_kf=3, culled=99).conf.tobytes()
    # a slot without vocabulary
    h2, _, _ = bow_hostmap(12, feats, bow=False)
    h2.set_bow_cpu(BowCpu())
    with pytest.raises(PlbaError):
        h2.insert_kf_bow(0)
    h2.close()
    h.close()
