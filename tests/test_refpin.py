"""The association front end pinned to the reference's own code: the recorded outputs of the compiled
reference (tests/golden/refpin.npz; oracle/refpin, tests/refpin_cases.py) against the checkers
(tests/ref_gridmatch.py, ref_stereo.py, ref_bow.py) and the host mirror (plslam_line_cells,
plslam_grid_match_cpu, plslam_stereo_cpu), and, where oracle/_ref/libref_stvo.so is present, the library
itself against the recording. Everything is compared for equality; there is no tolerance. No GPU.

The equality rules of matchGrid. Below nnr = 1 every row and the count are equal: a tie at a row's minimum
fails the ratio test in any order, and the records of `distances[i2]` are independent per train row, so the
order in which the reference walks its unordered_set cannot show. Above nnr = 1 two things can differ, and
both are computed from the cell lists and the checker's distance matrix, never from an output:
  * a row where two seen candidates tie at the minimum is matched to whichever the set yields first: such
    rows (refpin_cases.tie_rows) are left out of the comparison, and only them;
  * a row whose window holds train rows of which none is seen (refpin_cases.phantom_rows) passes the
    reference's ratio test INT_MAX < INT_MAX * nnr: the reference counts it and leaves its index at -1, the
    checker, the host mirror and the device do not count it. The reference's count less those rows must be
    the number of its indices >= 0."""
import numpy as np
import pytest

import bow_cases
import gridmatch_cases as G
import ref_bow
import ref_gridmatch as R
import ref_stereo as RS
import refpin_api as api
import refpin_cases as P
import stereo_cases as SC
from plba import capi, slam_map

GOLD = P.golden()
WINDOW = tuple(int(v) for v in GOLD["stereo_window"])


def assert_same_matches(got, name, pb, best_lr, w=None):
    """got = (matches_12, count) of a checker or twin against the recording of case `name`."""
    P.assert_same_matches(got, P.recorded(name, best_lr), pb, best_lr, w)


def all_match_cases():
    """name -> (problem, window) of every recorded matchGrid case."""
    out = {P.base_name(c): (G.problem(*c), None) for c in P.base_cases()}
    for name in P.stored_problems():
        out[name] = (P.stored_problem(name), None)
    for name in ("stereo_pts", "stereo_lns"):
        out[name] = (P.stored_problem(name), WINDOW)
    return out


# ---- the live half
def test_the_library_reproduces_the_recording():
    api.require()
    fresh = P.compute(api, WINDOW)
    assert sorted(fresh) == sorted(GOLD)
    cases = all_match_cases()
    for k in sorted(fresh):
        a, b = np.asarray(fresh[k]), GOLD[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        name = k[3:-4] if k.startswith("mg_") and not k.endswith("_digest") else None
        if name is not None and cases[name][0]["nnr"] > 1.0:
            free = np.append(P.tie_rows(cases[name][0], k.endswith("lr1"), cases[name][1]), False)
            assert np.array_equal(a[~free], b[~free]), k
        else:
            assert a.tobytes() == b.tobytes(), k


def test_stored_inputs_are_the_cases_of_this_tree():
    for name, pb in P.stored_problems().items():
        assert P.digest(pb).tobytes() == P.digest(P.stored_problem(name)).tobytes(), name
    assert GOLD["seg"].tobytes() == P.segments().tobytes()
    assert GOLD["stereo_lines"].tobytes() == P.stereo_case_lines().tobytes()
    for k, v in P.stereo_frame().items():
        assert GOLD[f"stereo_frame_{k}"].tobytes() == np.ascontiguousarray(v).tobytes(), k
    for name, (ids, vals) in P.bow_sequences().items():
        rec = P.recorded_bow(name)
        assert np.array_equal(rec[0], ids) and rec[1].tobytes() == vals.tobytes(), name


# ---- the rasteriser
def _cells(prefix, i):
    a, b = GOLD[prefix + "_off"][i:i + 2]
    return GOLD[prefix + "_cells"][a:b].astype(np.int64).tolist()


def test_line_walk_of_the_checkers_and_the_host_mirror():
    seg = GOLD["seg"]
    assert len(seg) >= 2000
    kinds = dict(zero=0, flat=0, upright=0, diagonal=0, reversed=0, negative=0, outside=0)
    for i, s in enumerate(seg):
        want = _cells("seg", i)
        assert [list(c) for c in R.line_cells(*s)] == want, s
        assert [list(c) for c in RS.R.line_cells(*s)] == want, s          # the walk ref_stereo.associate calls
        assert slam_map.line_cells(*s).tolist() == want, s
        kinds["zero"] += s[0] == s[2] and s[1] == s[3]
        kinds["flat"] += s[1] == s[3] and s[0] != s[2]
        kinds["upright"] += s[0] == s[2] and s[1] != s[3]
        kinds["diagonal"] += abs(s[3] - s[1]) == abs(s[2] - s[0]) and s[0] != s[2]
        kinds["reversed"] += s[0] > s[2]
        kinds["negative"] += bool(((s > -1) & (s < 0)).any())
        kinds["outside"] += any(not (0 <= c[0] < P.COLS and 0 <= c[1] < P.ROWS) for c in want)
    assert all(v >= 4 for v in kinds.values()), kinds


def test_line_walk_stays_within_the_documented_cap():
    """include/plba.h: coordinates at most one image size outside the image give at most 3 * max(cols, rows)
    + 1 cells; k_stereo_cells and its CPU twin stop there. The reference reaches the cap and does not pass it."""
    n_edge = len(P.EDGE_SEGMENTS)
    lengths = np.diff(GOLD["seg_off"])
    contract = lengths[n_edge - P.N_CONTRACT_EDGES:n_edge]
    print("longest walk: contract edges", int(contract.max()), "all segments", int(lengths.max()), "cap", P.MAX_STEPS)
    assert contract.max() == P.MAX_STEPS == 193
    assert lengths.max() <= P.MAX_STEPS
    assert np.diff(GOLD["stereo_lines_off"]).max() <= P.MAX_STEPS


def test_right_lines_of_the_stereo_cases():
    """Every right-image line of tests/stereo_cases.py: the reference's cells are ref_stereo's. With
    tests/test_gpu_stereo.py (device == ref_stereo, bit for bit) that is the chain reference -> checker -> device."""
    lines = P.stereo_case_lines()
    assert len(lines) >= 100 and GOLD["stereo_lines"].tobytes() == lines.tobytes()
    outside = 0
    for i, s in enumerate(lines):
        want = _cells("stereo_lines", i)
        assert [list(c) for c in RS.R.line_cells(*s)] == want, s
        assert slam_map.line_cells(*s).tolist() == want, s
        outside += any(not (0 <= c[0] < P.COLS and 0 <= c[1] < P.ROWS) for c in want)
    assert outside >= 10


# ---- GridStructure::get
def test_grid_windows():
    fill = P.uncsr(GOLD["get_fill_off"], GOLD["get_fill_cells"])
    assert all(np.array_equal(a, b) for a, b in zip(fill, P.get_fill())) and len(fill) == 200
    grid = RS.WindowGrid(P.ROWS, P.COLS)
    for idx, cells in enumerate(fill):
        for x, y in cells:
            grid.add(int(x), int(y), idx)
    windows = P.get_windows(WINDOW)
    assert windows[3] == (RS.DEFAULTS["matching_s_ws"], 0, 0, 0)
    sizes = []
    for wi, w in enumerate(windows):
        sym = w[0] == w[1] == w[2] == w[3]
        if sym:
            q = dict(kind=0, ws=w[0], nnr=0.9, line_sim_th=0.75, desc1=np.zeros((len(P.GET_QUERIES), 32), np.uint8),
                     cell1=np.array(P.GET_QUERIES, np.int32), cell1_end=None, desc2=np.zeros((len(fill), 32), np.uint8),
                     cells2=fill, dir2=None)
            cand, _ = R.candidates_and_distances(q, P.COLS, P.ROWS)
        for qi, (x, y) in enumerate(P.GET_QUERIES):
            k = wi * len(P.GET_QUERIES) + qi
            want = GOLD["get_idx"][GOLD["get_off"][k]:GOLD["get_off"][k + 1], 0].tolist()
            got = set()
            grid.get4(x, y, w, got)
            assert sorted(got) == want, (w, x, y)
            if sym:
                got = set()
                grid.get(x, y, w[0], got)
                assert sorted(got) == want, (w, x, y)
                assert np.flatnonzero(cand[qi]).tolist() == want, (w, x, y)
            sizes.append(len(want))
    assert min(sizes) == 0 and max(sizes) > 50


# ---- matchGrid
@pytest.mark.parametrize("best_lr", [False, True])
@pytest.mark.parametrize("case", P.base_cases())
def test_match_grid_base_cases(case, best_lr):
    pb, name = G.problem(*case), P.base_name(case)
    assert GOLD[f"mg_{name}_digest"].tobytes() == P.digest(pb).tobytes(), "the generator changed: record the fixture again"
    assert_same_matches(G.reference(*case, best_lr), name, pb, best_lr)
    assert_same_matches(slam_map.grid_match_cpu([pb], P.COLS, P.ROWS, best_lr, desc_bytes=32)[0], name, pb, best_lr)


def _checker_and_twin(pb, best_lr):
    out = R.match_grid(pb, P.COLS, P.ROWS, best_lr)
    twin = slam_map.grid_match_cpu([pb], P.COLS, P.ROWS, best_lr, desc_bytes=32)[0]
    assert np.array_equal(out[0], twin[0]) and out[1] == twin[1]
    return out


@pytest.mark.parametrize("best_lr", [False, True])
def test_ratio_test_on_the_double_boundary(best_lr):
    """d0 = 6, d1 = 10: 10 * 0.6 rounds to 6.0 and 6 < 6.0 fails; 0.6f widened is above 0.6 and passes."""
    assert 10 * 0.6 == 6.0 and 10 * P.NNR_06F > 6.0
    for name, want in (("ratio_06", [-1]), ("ratio_06f", [0])):
        pb = P.stored_problem(name)
        assert P.recorded(name, best_lr)[0].tolist() == want
        assert_same_matches(_checker_and_twin(pb, best_lr), name, pb, best_lr)


@pytest.mark.parametrize("best_lr", [False, True])
def test_line_similarity_one_ulp_either_side(best_lr):
    for name, want in (("sim_below", [0]), ("sim_equal", [0]), ("sim_above", [-1])):
        pb = P.stored_problem(name)
        assert abs(pb["line_sim_th"] - P.V0) <= np.spacing(P.V0)
        assert P.recorded(name, best_lr)[0].tolist() == want, name
        assert_same_matches(_checker_and_twin(pb, best_lr), name, pb, best_lr)


@pytest.mark.parametrize("best_lr", [False, True])
@pytest.mark.parametrize("name", [f"device{k}" for k in range(len(P.DEVICE_PROBLEMS))])
def test_match_grid_device_problems_on_the_host(name, best_lr):
    pb = P.stored_problem(name)
    assert_same_matches(_checker_and_twin(pb, best_lr), name, pb, best_lr)


@pytest.mark.parametrize("best_lr", [False, True])
def test_match_grid_above_nnr_one(best_lr):
    pb = P.stored_problem("nnr12")
    assert pb["nnr"] == 1.2
    free = P.tie_rows(pb, best_lr)
    print("tie rows", int(free.sum()), "of", len(free), "phantom rows", int(P.phantom_rows(pb, best_lr).sum()))
    assert 0 < free.sum() <= 0.1 * len(free)
    assert_same_matches(_checker_and_twin(pb, best_lr), "nnr12", pb, best_lr)


# ---- the three places where the checker pins what the reference leaves open
def test_divergence_candidate_order():
    """Two candidates tie at the minimum above nnr = 1. The reference takes whichever its unordered_set yields
    first (recorded: either); the checker, the twin and the kernels take the lowest i2."""
    pb = P.stored_problem("order_tie")
    for best_lr in (False, True):
        m12, cnt = P.recorded("order_tie", best_lr)
        assert P.tie_rows(pb, best_lr).tolist() == [True]
        assert m12[0] in (0, 1) and cnt == 1
        assert _checker_and_twin(pb, best_lr)[0].tolist() == [0]


def test_divergence_nan_direction():
    """A query line whose two cells are equal: normalize gives NaN, |NaN| < th is false and the candidate is
    kept, in the reference as in the checker. Row 1 is a real rejection by the same test."""
    pb = P.stored_problem("nan_direction")
    assert all(np.isnan(v) for v in R.normalize(0, 0))
    for best_lr in (False, True):
        m12, cnt = P.recorded("nan_direction", best_lr)
        assert m12.tolist() == [0, -1] and cnt == 1
        assert_same_matches(_checker_and_twin(pb, best_lr), "nan_direction", pb, best_lr)


def test_divergence_no_seen_pair_above_nnr_one():
    """Two equal queries, one train row, best_lr, nnr = 1.5: the second query sees no pair. The reference
    counts it (INT_MAX < INT_MAX * 1.5) with index -1: it returns 2 for one index; the checker and the twin
    return 1 (include/plba.h, "Defined where the reference is not")."""
    pb = P.stored_problem("no_seen_pair")
    m12, cnt = P.recorded("no_seen_pair", True)
    assert m12.tolist() == [0, -1] and cnt == 2
    assert P.phantom_rows(pb, True).tolist() == [False, True]
    got = _checker_and_twin(pb, True)
    assert got[0].tolist() == [0, -1] and got[1] == 1
    assert_same_matches(got, "no_seen_pair", pb, True)
    m12, cnt = P.recorded("no_seen_pair", False)           # without the cross-check both see the pair
    assert m12.tolist() == [0, 0] and cnt == 2
    assert_same_matches(_checker_and_twin(pb, False), "no_seen_pair", pb, False)


# ---- the stereo window
OPEN = dict(P.OPEN_GATES, matching_s_ws=WINDOW[0])


def test_stereo_window_is_the_reference_s():
    """(matching_s_ws, 0, 0, 0), read from src2/stereoFrame.cpp and src2/config.cpp when the fixture was made."""
    assert WINDOW == (10, 0, 0, 0)
    assert capi.stereo_params(dict(SC.CAMERA)).matching_s_ws == WINDOW[0] == RS.DEFAULTS["matching_s_ws"]


@pytest.mark.parametrize("best_lr", [0, 1])
def test_stereo_window_match_grid(best_lr):
    frame = {k[len("stereo_frame_"):]: v for k, v in GOLD.items() if k.startswith("stereo_frame_")}
    prm = RS.params(**SC.CAMERA, best_lr=best_lr, **OPEN)
    got, twin = RS.associate(frame, prm), slam_map.stereo_cpu([frame], prm)[0]
    assert RS.same(got, twin) is None
    for kind, name in enumerate(("stereo_pts", "stereo_lns")):
        pb = P.stored_problem(name)
        grid = RS.WindowGrid(P.ROWS, P.COLS)
        for idx, cells in enumerate(pb["cells2"]):
            for x, y in cells:
                grid.add(int(x), int(y), idx)
        m12 = RS.match_grid(kind, pb["cell1"].tolist(), pb["cell1_end"].tolist() if kind else None, pb["desc1"], grid,
                            pb["desc2"], pb["dir2"], WINDOW, dict(best_lr=best_lr, min_ratio_12_p=pb["nnr"],
                                                                  line_sim_th=pb["line_sim_th"]))
        ref_m12, ref_cnt = P.recorded(name, best_lr)
        assert m12 == ref_m12.tolist() and ref_cnt == int((ref_m12 >= 0).sum())
        assert 10 <= ref_cnt < len(m12)
        # with every gate open the survivors of the whole front end are the matched rows
        assert got["ls_src" if kind else "pt_src"].tolist() == np.flatnonzero(ref_m12 >= 0).tolist()
    ref_m12 = P.recorded("stereo_pts", best_lr)[0]
    rows = np.flatnonzero(ref_m12 >= 0)
    disp = (frame["pt_l"][rows, 0] - frame["pt_r"][ref_m12[rows], 0]).astype(np.float64)
    assert got["pt_disp"].tobytes() == disp.tobytes()      # and they are matched to the reference's right rows


def test_distance():
    want = [R.hamming_row(a, b) for a, b in zip(GOLD["dist_a"], GOLD["dist_b"])]
    assert GOLD["dist"].tolist() == want and want[0] == 256 and want[1] == 1


# ---- BowVector
@pytest.mark.parametrize("count", [6, 10])
def test_bow_repeated_add_weight_is_the_repeated_sum(count):
    voc, q = bow_cases.sum_case(count)
    in_ids, in_vals, ids, raw, vals = P.recorded_bow(f"sum{count}")
    assert in_ids.tolist() == [0] * count + [1] and in_vals.tolist() == [0.1] * count + [0.3]
    acc = 0.0
    for _ in range(count):
        acc += 0.1
    assert acc != count * 0.1 and ids.tolist() == [0, 1] and raw.tolist() == [acc, 0.3]
    want = ref_bow.transform(voc, q)
    assert [w for w, _ in want] == ids.tolist()
    assert np.array([v for _, v in want]).tobytes() == vals.tobytes()


def test_bow_l1_normalisation_on_the_bow_cases():
    seen = 0
    for name in bow_cases.VOCABS:
        for n in P.BOW_N_DESC + ([600] if name == "k10L3" else []):
            _, _, ids, raw, vals = P.recorded_bow(f"{name}_{n}")
            w_ids, w_vals = bow_cases.as_arrays(bow_cases.reference_vector(name, n))
            assert ids.tolist() == w_ids.tolist(), (name, n)
            assert vals.tobytes() == w_vals.tobytes(), (name, n)
            seen += len(ids)
    assert seen > 500


def test_bow_add_if_not_exist():
    ids, vals, flags = P.IF_NOT_EXIST
    want = {}
    for i, v, f in zip(ids.tolist(), vals.tolist(), flags.tolist()):
        if f:
            want.setdefault(i, v)
        else:
            want[i] = want.get(i, 0.0) + v
    assert GOLD["bow_ifne_ids"].tolist() == sorted(want)
    assert GOLD["bow_ifne_vals"].tolist() == [want[i] for i in sorted(want)]
