"""Place recognition on the GPU (plba_bow_*: DBoW2 transform, L1 normalisation and L1 score) against
the plain-Python checker (tests/ref_bow.py). The results are doubles compared as bytes: -0.0 and every
last bit count. tests/test_bow_oracle.py shows on the checker alone that the constructed cases hold
what they are meant to."""
import ctypes as C

import numpy as np
import pytest

import bow_cases as cases
import ref_bow as R
from plba import capi
from plba.lib import PlbaError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _assert_vector(got, vec):
    w, v = got
    assert w.dtype == np.int32 and v.dtype == np.float64
    rw, rv = cases.as_arrays(vec)
    assert w.tobytes() == rw.tobytes(), (w[:10], rw[:10])
    assert v.tobytes() == rv.tobytes(), np.flatnonzero(v != rv)[:10]


def _assert_scores(scores, ref):
    ref = np.array(ref, np.float64)
    assert scores.tobytes() == ref.tobytes(), (scores[:8], ref[:8])


@pytest.mark.parametrize("name", cases.VOCABS)
def test_vectors_and_scores_equal_the_checker(solver, name):
    solver.bow_set_vocab(0, cases.vocab(name))
    stored = []
    for kf, n in enumerate(cases.N_DESC):
        vec = cases.reference_vector(name, n)
        ids, scores = solver.bow_insert(0, kf, cases.descriptors(name, n))
        assert ids.tolist() == list(range(kf + 1))
        _assert_scores(scores, [R.score(vec, o) for o in stored] + [R.score(vec, vec)])
        _assert_vector(solver.bow_get(0, kf), vec)
        stored.append(vec)
    print(name, "words per vector", [len(v) for v in stored])


def test_more_keys_than_the_lds_sort_holds(solver):
    # 9000 descriptors: the word ids are sorted in global memory (above 8192 keys)
    name, n = "k10L3", 9000
    solver.bow_set_vocab(0, cases.vocab(name))
    vec = cases.reference_vector(name, n)
    small = cases.reference_vector(name, 257)
    solver.bow_insert(0, 0, cases.descriptors(name, 257))
    ids, scores = solver.bow_insert(0, 1, cases.descriptors(name, n))
    _assert_vector(solver.bow_get(0, 1), vec)
    _assert_scores(scores, [R.score(vec, small), R.score(vec, vec)])


def test_the_first_child_wins_a_tie(solver):
    voc, q, first, second = cases.tie_case()
    solver.bow_set_vocab(0, voc)
    solver.bow_insert(0, 0, q)
    w, v = solver.bow_get(0, 0)
    assert w.tolist() == [int(voc["word_id"][first])] and v.tolist() == [1.0]


@pytest.mark.parametrize("count", [6, 10])
def test_a_word_is_the_repeated_sum_not_the_product(solver, count):
    voc, q = cases.sum_case(count)
    solver.bow_set_vocab(0, voc)
    ids, scores = solver.bow_insert(0, 0, q)
    vec = R.transform(voc, q)
    _assert_vector(solver.bow_get(0, 0), vec)
    _assert_scores(scores, [R.score(vec, vec)])
    # and a permutation of the rows gives the same bytes
    solver.bow_insert(0, 1, np.ascontiguousarray(q[::-1]))
    _assert_vector(solver.bow_get(0, 1), vec)


def test_an_empty_vector_and_no_common_word(solver):
    voc, q = cases.stopped_case()
    solver.bow_set_vocab(0, voc)
    ids, scores = solver.bow_insert(0, 0, q)
    assert len(solver.bow_get(0, 0)[0]) == 0
    _assert_scores(scores, [-0.0])
    voc, a, b = cases.disjoint_case()
    solver.bow_set_vocab(0, voc)
    solver.bow_insert(0, 3, a)
    ids, scores = solver.bow_insert(0, 5, b)
    va, vb = R.transform(voc, a), R.transform(voc, b)
    _assert_scores(scores, [R.score(vb, va), R.score(vb, vb)])
    assert np.signbit(scores[0]) and scores[0] == 0.0


@pytest.mark.parametrize("n_db", [0, 1, 65, 300])
def test_a_database_with_removed_vectors(solver, n_db):
    """n_db stored vectors, every fifth removed, ids with gaps; the new vector is scored against the
    live ones in increasing kf_id, then against itself. Twice, and in a fresh database holding only the live ones."""
    name = "k10L3"
    voc = cases.vocab(name)
    sizes = [0, 1, 2, 63, 65]
    vecs = {3 * i + 1: cases.reference_vector(name, sizes[i % 5], seed=i // 5) for i in range(n_db)}
    new = cases.reference_vector(name, 257)
    runs = []
    for fresh in (False, False, True):
        solver.bow_set_vocab(0, voc)
        for i in range(n_db):
            if not fresh or i % 5 != 2:
                solver.bow_insert(0, 3 * i + 1, cases.descriptors(name, sizes[i % 5], seed=i // 5))
        if not fresh:
            for i in range(2, n_db, 5):
                solver.bow_remove(0, 3 * i + 1)
        if not fresh and n_db > 2:     # a removed vector is gone, its neighbour is not
            with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
                solver.bow_get(0, 7)
            _assert_vector(solver.bow_get(0, 10), vecs[10])
        ids, scores = solver.bow_insert(0, 2, cases.descriptors(name, 257))   # an id between the stored ones
        runs.append((ids.tobytes(), scores.tobytes()))
        live = sorted(k for k in vecs if (k - 1) // 3 % 5 != 2) + [2]    # the new vector itself comes last
        assert ids.tolist() == live
        _assert_scores(scores, [R.score(new, new if k == 2 else vecs[k]) for k in live])
    assert runs[0] == runs[1] == runs[2]
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        solver.bow_get(0, 99)          # an id that was never stored


def test_the_slots_are_independent(solver):
    solver.bow_set_vocab(0, cases.vocab("k10L3"))
    solver.bow_set_vocab(1, cases.vocab("lines"))
    vp = [cases.reference_vector("k10L3", n) for n in (63, 65)]
    vl = [cases.reference_vector("lines", n) for n in (65, 63, 257)]
    solver.bow_insert(0, 0, cases.descriptors("k10L3", 63))
    solver.bow_insert(1, 0, cases.descriptors("lines", 65))
    solver.bow_insert(1, 1, cases.descriptors("lines", 63))
    ids, scores = solver.bow_insert(0, 1, cases.descriptors("k10L3", 65))
    assert ids.tolist() == [0, 1]
    _assert_scores(scores, [R.score(vp[1], vp[0]), R.score(vp[1], vp[1])])
    solver.bow_set_vocab(0, cases.vocab("k3L2"))      # clears slot 0 only
    ids, scores = solver.bow_insert(1, 2, cases.descriptors("lines", 257))
    _assert_scores(scores, [R.score(vl[2], vl[0]), R.score(vl[2], vl[1]), R.score(vl[2], vl[2])])
    _assert_vector(solver.bow_get(1, 1), vl[1])
    assert solver.bow_insert(0, 0, cases.descriptors("k3L2", 2))[0].tolist() == [0]


def test_inserting_leaves_an_uploaded_window_intact(solver):
    from plba import synth
    g = synth.generate("C1L")
    solver.upload(g)
    before = solver.lba_plucker()
    solver.bow_set_vocab(0, cases.vocab("k3L2"))
    solver.bow_insert(0, 0, cases.descriptors("k3L2", 65))
    _assert_vector(solver.bow_get(0, 0), cases.reference_vector("k3L2", 65))
    solver.reset()
    after = solver.lba_plucker()
    for k in ("kf_Tcw", "pt_xyz", "ln_orth"):
        assert np.array_equal(before[k], after[k]), k


@pytest.fixture()
def fresh_solver():
    from plba.lib import Solver
    s = Solver()     # slot 1 of the shared one may hold a vocabulary
    yield s
    s.close()


def test_malformed_vocabularies_and_bad_arguments_are_refused(fresh_solver):
    from plba.lib import PLBA_ERRORS
    solver = fresh_solver
    good = cases.vocab("k3L2")
    solver.bow_set_vocab(0, good)
    solver.bow_insert(0, 0, cases.descriptors("k3L2", 63))
    for why, voc in cases.malformed().items():
        vv = capi.BowVocabView(voc)
        rc = solver.L.plba_bow_set_vocab(solver.ctx, 0, C.byref(vv.struct))
        assert PLBA_ERRORS.get(rc, rc) == "PLBA_E_INVALID", why
    vv = capi.BowVocabView(good)
    assert solver.L.plba_bow_set_vocab(solver.ctx, 2, C.byref(vv.struct)) == -1
    assert solver.L.plba_bow_set_vocab(solver.ctx, 0, None) == -1
    d = np.ascontiguousarray(cases.descriptors("k3L2", 65))
    sc, ids, n = np.zeros(4), np.zeros(4, np.int32), C.c_int32(-5)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)

    def insert(slot=0, kf=1, desc=d.ctypes.data_as(bp), nd=65, s=sc.ctypes.data_as(dp), i=ids.ctypes.data_as(ip), cap=4,
               nn=C.byref(n)):
        return solver.L.plba_bow_insert(solver.ctx, slot, kf, desc, nd, s, i, cap, nn)
    for kw in (dict(slot=1), dict(slot=-1), dict(kf=-1), dict(kf=0), dict(desc=None), dict(nd=-1), dict(nd=65536),
               dict(s=None), dict(i=None), dict(cap=-1), dict(nn=None)):
        assert insert(**kw) == -1, kw          # slot 1 has no vocabulary; kf 0 is already stored
    assert n.value == -5
    assert solver.L.plba_bow_remove(solver.ctx, 0, 1) == -1 and solver.L.plba_bow_get(solver.ctx, 0, 1, None, None, 0, C.byref(n)) == -1
    # the refused calls left the slot as it was: the next valid insert is right
    ids2, scores = solver.bow_insert(0, 1, d)
    a, b = cases.reference_vector("k3L2", 65), cases.reference_vector("k3L2", 63)
    assert ids2.tolist() == [0, 1]
    _assert_scores(scores, [R.score(a, b), R.score(a, a)])


def test_loop_closure_whole_on_the_device_equals_the_cpu_hooks():
    """The 14-keyframe map of tests/test_host_bow.py, where keyframe 13 revisits keyframe 2: every
    keyframe inserted (PL) and plslam_loop_closure_kf run with no hook at all (place recognition,
    matcher, relative pose and pose graph on the device), against the same calls with every hook on
    the CPU (plslam_bow_cpu and the checkers of the matcher, the relative pose and the pose graph).
    The float conf_matrix is compared as bytes; of the statistics the counts, gates and states, as
    tests/test_gpu_isloopclosure.py does."""
    import test_host_bow as T
    from plba.slam_map import LC_ACTIVE, LC_IDLE, match_params
    from test_host_isloopclosure import lcpose_hook
    feats = T.loop_features()

    def run(device):
        h, _, calls = T.bow_hostmap(T.N_KF, feats, bow=not device)
        if device:
            for setter in (h.set_match_fn, h.set_lcpose_solver, h.set_pgo_solver):
                setter(None)
            h.set_vocabulary(0, cases.vocab("k10L3"))
            h.set_vocabulary(1, cases.vocab("lines"))
        else:
            h.set_lcpose_solver(lcpose_hook(calls["pose"]))      # the checker's own verdict, not accept-all
        for k in range(T.N_KF):
            h.insert_kf_bow(k)
        out = dict(conf=h.conf_matrix().tobytes(), cand=h.look_for_loop_candidates(T.KF_CURR, T.SMALL))
        out["step"] = h.loop_closure_kf(T.KF_CURR, T.SMALL, match_params())
        out["idxs"], out["state"] = h.lc_idx_list().tolist(), h.lc_state()
        none = T.lc_search_params(**dict(cases.SMALL, lc_nkf_closest=100))
        out["step2"] = h.loop_closure_kf(T.KF_CURR, none, match_params())
        out["state2"] = h.lc_state()
        h.close()
        return out
    dev, cpu = run(True), run(False)
    assert dev["conf"] == cpu["conf"] == T.reference_loop_conf(feats).tobytes()
    assert dev["cand"] == cpu["cand"] == (True, T.KF_PREV)
    for step in ("step", "step2"):
        for k in ("is_candidate", "ratio_ok", "accepted", "conditions", "n_inl_pt", "n_inl_ln", "state_before",
                  "state_after", "pgo_ran", "inl_ratio_pt", "inl_ratio_ls"):
            assert dev[step][k] == cpu[step][k], (step, k, dev[step][k], cpu[step][k])
    assert dev["step"]["accepted"] == 1 and dev["state"] == cpu["state"] == LC_ACTIVE and dev["idxs"] == cpu["idxs"]
    assert dev["idxs"][-1] == [T.KF_PREV, T.KF_CURR, 1]
    assert dev["step2"]["pgo_ran"] == 1 and dev["state2"] == cpu["state2"] == LC_IDLE
