"""The grid matcher and the stereo front end on the device against the reference's own code, with no checker
in between: Solver.grid_match and Solver.stereo_associate against the outputs of the compiled reference
(oracle/refpin): the library itself where oracle/_ref/libref_stvo.so is present, its recording
tests/golden/refpin.npz otherwise (tests/test_refpin.py shows that the two agree). Equality throughout, by the
rules stated in tests/test_refpin.py: every row and the count below nnr = 1; above it every row but those
where two seen candidates tie at the minimum, and the count less the rows that the reference counts at
index -1."""
import numpy as np
import pytest

import ref_stereo as RS
import refpin_api as api
import refpin_cases as P
import stereo_cases as SC

pytestmark = pytest.mark.gpu

GOLD = P.golden()
WINDOW = tuple(int(v) for v in GOLD["stereo_window"])
HAND = ["ratio_06", "ratio_06f", "sim_below", "sim_equal", "sim_above", "order_tie", "nan_direction", "no_seen_pair",
        "nnr12"]
DEVICE = [f"device{k}" for k in range(len(P.DEVICE_PROBLEMS))]


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    with Solver(device=0) as s:
        yield s


def reference(name, best_lr, w=None):
    if api.available():
        return api.match_grid(P.stored_problem(name), P.COLS, P.ROWS, best_lr, w)
    return P.recorded(name, best_lr)


@pytest.mark.parametrize("best_lr", [False, True])
@pytest.mark.parametrize("name", DEVICE)
def test_grid_match_single_problems(solver, name, best_lr):
    pb = P.stored_problem(name)
    assert len(pb["desc1"]) <= 300 and len(pb["desc2"]) <= 300
    out = solver.grid_match([pb], P.COLS, P.ROWS, best_lr, desc_bytes=32)[0]
    print(name, "matches", out[1], "of", len(pb["desc1"]))
    P.assert_same_matches(out, reference(name, best_lr), pb, best_lr)


@pytest.mark.parametrize("best_lr", [False, True])
def test_grid_match_one_batch_of_both_kinds_and_every_window(solver, best_lr):
    names = DEVICE + HAND
    pbs = [P.stored_problem(n) for n in names]
    assert {p["kind"] for p in pbs} == {0, 1} and {p["ws"] for p in pbs[:len(DEVICE)]} == {0, 1, 12}
    assert {(p["kind"], p["ws"]) for p in pbs[:len(DEVICE)]} == {(k, w) for k in (0, 1) for w in (0, 1, 12)}
    for name, pb, out in zip(names, pbs, solver.grid_match(pbs, P.COLS, P.ROWS, best_lr, desc_bytes=32)):
        P.assert_same_matches(out, reference(name, best_lr), pb, best_lr)


def test_the_documented_divergences_on_the_device(solver):
    """What the reference does is recorded; the device does what include/plba.h defines."""
    tie, nan, none = (P.stored_problem(n) for n in ("order_tie", "nan_direction", "no_seen_pair"))
    got = solver.grid_match([tie, nan, none], P.COLS, P.ROWS, True, desc_bytes=32)
    assert reference("order_tie", True)[0][0] in (0, 1) and got[0][0].tolist() == [0] and got[0][1] == 1
    assert reference("nan_direction", True)[0].tolist() == got[1][0].tolist() == [0, -1] and got[1][1] == 1
    ref = reference("no_seen_pair", True)
    assert ref[0].tolist() == got[2][0].tolist() == [0, -1] and ref[1] == 2 and got[2][1] == 1


@pytest.mark.parametrize("best_lr", [0, 1])
def test_stereo_window_against_the_reference(solver, best_lr):
    """The window (matching_s_ws, 0, 0, 0) of src2/stereoFrame.cpp: with every gate open the survivors of
    stereo_associate are the rows that the reference's matchGrid matches under that window, and the
    disparities name the same right rows."""
    frame = {k[len("stereo_frame_"):]: v for k, v in GOLD.items() if k.startswith("stereo_frame_")}
    got = solver.stereo_associate([frame], RS.params(**SC.CAMERA, best_lr=best_lr, matching_s_ws=WINDOW[0], **P.OPEN_GATES))[0]
    pts, lns = reference("stereo_pts", best_lr, WINDOW), reference("stereo_lns", best_lr, WINDOW)
    assert got["pt_src"].tolist() == np.flatnonzero(pts[0] >= 0).tolist() and got["n_pt"] == pts[1]
    assert got["ls_src"].tolist() == np.flatnonzero(lns[0] >= 0).tolist() and got["n_ls"] == lns[1]
    rows = np.flatnonzero(pts[0] >= 0)
    disp = (frame["pt_l"][rows, 0] - frame["pt_r"][pts[0][rows], 0]).astype(np.float64)
    assert got["pt_disp"].tobytes() == disp.tobytes()


def test_stereo_cases_close_the_chain(solver):
    """tests/test_refpin.py::test_right_lines_of_the_stereo_cases: the reference's getLineCoords gives ref_stereo's
    cells for every right line of these cases; here the device gives ref_stereo's results on them, bit for bit."""
    names = list(SC.CASES)
    prm = RS.params(**SC.CAMERA, best_lr=1, pluker=1)
    for name, got in zip(names, solver.stereo_associate([SC.case(n) for n in names], prm)):
        assert RS.same(RS.associate(SC.case(name), prm), got) is None, name
