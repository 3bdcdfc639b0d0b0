"""The place-recognition checker (tests/ref_bow.py) on its own, no GPU and no library: the constructed
cases of tests/bow_cases.py hold the property each was built for, and the loop-candidate search inputs
take every exit of lookForLoopCandidates. What the device tests compare against is therefore not
vacuous."""
import math

import numpy as np
import pytest

import bow_cases as cases
import ref_bow as R


def test_the_tie_exists_and_the_first_child_wins():
    voc, q, first, second = cases.tie_case()
    kids = voc["children"][voc["child_off"][0]:voc["child_off"][1]].tolist()
    assert kids.index(first) < kids.index(second) and first > second     # listed first, not lowest index
    for d in q:
        d1, d2 = R.hamming(d, voc["node_desc"][first]), R.hamming(d, voc["node_desc"][second])
        assert d1 == d2 and all(R.hamming(d, voc["node_desc"][k]) > d1 for k in kids if k not in (first, second))
        assert R.descend(voc, d)[0] == first
    assert R.transform(voc, q) == [(int(voc["word_id"][first]), 1.0)]


@pytest.mark.parametrize("count", [6, 10])
def test_the_repeated_sum_is_not_the_product(count):
    voc, q = cases.sum_case(count)
    acc = 0.0
    for _ in range(count):
        acc += 0.1
    assert acc != count * 0.1
    vec = R.transform(voc, q)
    assert [w for w, _ in vec] == [0, 1]
    assert vec[0][1] == acc / (acc + 0.3) and vec[0][1] != (count * 0.1) / (count * 0.1 + 0.3)
    assert R.transform(voc, q[::-1]) == vec          # the order of the descriptors does not matter


def test_stopped_words_and_the_empty_vector():
    voc, q = cases.stopped_case()
    assert R.transform(voc, q) == []
    s = R.score([], [])
    assert s == 0.0 and math.copysign(1.0, s) == -1.0
    voc = cases.vocab("zeros")
    leaves = np.flatnonzero(voc["word_id"] >= 0)
    assert (voc["weight"][leaves] == 0).sum() == len(leaves[::3])
    hit = {R.descend(voc, d)[0] for d in cases.descriptors("zeros", 257)}
    stopped = {int(n) for n in hit if voc["weight"][n] == 0}
    assert stopped and hit - stopped        # both kinds of leaf are reached
    words = {w for w, _ in cases.reference_vector("zeros", 257)}
    assert words == {int(voc["word_id"][n]) for n in hit - stopped}


def test_no_common_word_gives_minus_zero():
    voc, a, b = cases.disjoint_case()
    va, vb = R.transform(voc, a), R.transform(voc, b)
    assert va and vb and not {w for w, _ in va} & {w for w, _ in vb}
    s = R.score(vb, va)
    assert s == 0.0 and math.copysign(1.0, s) == -1.0
    assert R.score(va, va) == 1.0 or abs(R.score(va, va) - 1.0) < 1e-15


def test_the_ragged_leaves_are_reached():
    voc = cases.vocab("ragged")
    depth = {}
    for n in (1, 2, 63, 65, 257, 600):
        for d in cases.descriptors("ragged", n):
            leaf, path = R.descend(voc, d)
            depth.setdefault(len(path), set()).add(leaf)
    assert 1 in depth and 3 in depth and 2 in depth, depth
    assert 3 in [p for n in (257,) for d in cases.descriptors("ragged", n) for p in R.descend(voc, d)[1]]  # through the single child
    assert max(len(v) for v in depth.values()) >= 2


def test_vectors_are_normalised_and_sorted():
    for name in cases.VOCABS:
        for n in cases.N_DESC:
            vec = cases.reference_vector(name, n)
            words = [w for w, _ in vec]
            assert words == sorted(set(words))
            if vec:
                assert abs(sum(v for _, v in vec) - 1.0) < 1e-12
                assert abs(R.score(vec, vec) - 1.0) < 1e-12
    a, b = cases.reference_vector("k10L3", 257), cases.reference_vector("k10L3", 600)
    assert 0.0 < R.score(a, b) < 1.0


def test_every_malformed_vocabulary_differs_from_the_valid_one():
    base = cases.vocab("k3L2")
    bad = cases.malformed()
    assert len(bad) == 13
    for why, voc in bad.items():
        assert any(not np.array_equal(voc[k], base[k], equal_nan=False) if isinstance(base[k], np.ndarray)
                   else voc[k] != base[k] for k in base), why


def test_vector_stdv_and_the_combined_score():
    assert R.vector_stdv([1.0, 2.0, 3.0, 4.0]) == math.sqrt(1.0 / 4 * 5.0)
    assert math.isnan(R.vector_stdv([]))
    assert R.vector_stdv([7.5]) == 0.0
    assert math.isnan(R.combined(0.5, 0.25, 0, 0, math.nan, math.nan))
    assert math.isnan(R.combined(0.5, 0.25, 1, 1, 0.0, 0.0))          # std_pl == 0: 0 / 0
    s = R.combined(0.5, 0.25, 70, 20, 300.0, 280.0)
    assert s == (0.5 * 70 + 0.25 * 20) / 90 + (0.5 * 300.0 + 0.25 * 280.0) / 580.0
    assert R.f32(0.1) == float(np.float32(0.1)) and R.f32(0.1) != 0.1


@pytest.mark.parametrize("mode", ["P", "L", "PL"])
def test_the_map_keeps_a_symmetric_float_matrix(mode):
    m = cases.reference_map(mode)
    c = m.conf
    assert c.dtype == np.float32 and c.shape == (12, 12)
    assert np.array_equal(c, c.T)
    # keyframe 4 was culled after insert 6: its row keeps what it had, later keyframes never scored it
    assert (c[4, :7] != 0).all() and (c[4, 7:] == 0).all()
    lo, hi = (0.999, 1.001) if mode != "PL" else (1.999, 2.001)
    assert all(lo < c[i, i] < hi for i in range(12))


def test_a_keyframe_without_features_stores_nan():
    m = cases.reference_map("PL", empty_kf=9)
    live = [i for i in range(10) if i != 4]
    assert np.isnan(m.conf[9, live]).all() and np.isnan(m.conf[live, 9]).all()
    assert m.conf[9, 4] == 0 and m.conf[4, 9] == 0           # the culled keyframe was skipped
    assert not np.isnan(m.conf[10, :9]).any()


@pytest.mark.parametrize("kind", cases.SEARCH_KINDS)
def test_the_search_takes_every_exit(kind):
    conf, fg, live, cur, p, expected = cases.search_case(kind)
    ok, prev, exit_ = R.look_for_loop_candidates(conf, fg, live, cur, **p)
    assert exit_ == expected
    assert (ok, prev) == ((True, 2) if expected == "accepted" else (False, -1))


def test_the_search_with_the_default_parameters():
    for kind in ("accepted", "too_few_neighbours", "best_too_low"):
        conf, fg, live, cur, p, expected = cases.search_case(kind, n=120, params=R.DEFAULT_SEARCH)
        ok, prev, exit_ = R.look_for_loop_candidates(conf, fg, live, cur)
        assert exit_ == expected and (ok, prev) == ((True, 2) if kind == "accepted" else (False, -1))
    conf, fg, live, cur, p, _ = cases.search_case("accepted", n=101, params=R.DEFAULT_SEARCH)
    assert R.look_for_loop_candidates(conf, fg, live, cur)[2] == "too_few"     # 50 candidates are not more than 50


def test_covisible_keyframes_lower_the_minimum_score():
    conf, fg, live, cur, p, _ = cases.search_case("best_too_low")
    fg = fg.copy()
    conf = conf.copy()
    conf[5, cur] = conf[cur, 5] = 0.2       # an old keyframe that shares 75 landmarks: lc_min_score 0.2
    fg[5, cur] = 75
    ok, prev, exit_ = R.look_for_loop_candidates(conf, fg, live, cur, **p)
    assert exit_ == "too_few_neighbours" and not ok     # the best (0.29) passes now; its neighbours do not
