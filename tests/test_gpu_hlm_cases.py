"""The hand-rolled LM loops on the device (plba_hlm_lba variants 0, 1, 2) where they reject a step, stop
on each of their tests, or clamp a residual row: the candidates of tests/hlm_cases.py, admitted by
tests/test_hlm_cases_oracle.py, through the bar of test_gpu_hlm._compare (identical counters and trace,
λ and err to 1e-9, states within 1e-4 of the checker's total change), plus what the bar alone would
not pin: the result sequence literally, λ on the rejected row, and the state after a rejection."""
import ctypes as C

import numpy as np
import pytest

import hlm_cases as cases
from test_gpu_hlm import _compare

pytestmark = pytest.mark.gpu

STATE = ("kf_x", "kf_Tcw", "pt_xyz", "ln_orth", "ln_line3d")


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _check_family(solver, case):
    """The uploaded window takes the factorisation family the case is there for."""
    st = solver.structure_stats()
    if case.family == "band":
        assert st["banded"] == 1 and st["column_lane"] == 0 and st["bcr_rows"] == 0 and st["bw"] >= 10, st
    elif case.family == "column_lane":
        assert st["column_lane"] == 1 and st["twisted"] == 1 and st["bcr_rows"] == 0 and st["nf"] == 54, st
    elif case.family == "bcr":   # the smallest plan that goes to block cyclic reduction at this band width
        plan = (C.c_int32 * 9)()
        assert st["nf"] == cases.BCR_NF and st["bcr_rows"] > 0, st
        assert solver.L.plba_factor_plan(st["bw"], st["nf"], 256, 4, plan, 9) == 0 and plan[0] == 6
        assert solver.L.plba_factor_plan(st["bw"], st["nf"] - 1, 256, 4, plan, 9) == 0 and plan[0] != 6
    else:
        assert not case.family


def _run(solver, case, **kw):
    win = case.window()
    solver.upload(win.graph)
    _check_family(solver, case)
    out = solver.hlm_lba(win, case.params(**kw))
    if case.family == "bcr":
        assert solver.structure_stats()["bcr_fallbacks"] == 0
    return out


@pytest.mark.parametrize("case", cases.ALL, ids=[c.id for c in cases.ALL])
def test_case_matches_the_checker_and_its_named_flow(solver, case):
    out, ref, p = _run(solver, case), case.reference(), case.params()
    tr = out["trace"]
    print(case.id, list(tr["result"]), out["linearizations"], out["solves"], out["accepted"], out["err"], ref["err"],
          out["dx_norm"], ref["dx_norm"])
    assert tuple(int(r) for r in tr["result"]) == case.results
    assert (out["linearizations"], out["solves"], out["accepted"]) == case.counters
    assert cases.stop_of(out, p) == case.stop
    _compare(out, ref, case.window())
    for row in case.rejected_rows():
        assert tr["lambda_end"][row] == tr["lambda_start"][row] / p.lambda_k
        assert tr["chi2_start"][row] > tr["chi2_start"][row - 1]
    for row in range(1, len(tr)):
        if case.results[row] == 0:
            assert tr["lambda_end"][row] == tr["lambda_start"][row] * p.lambda_k


@pytest.mark.parametrize("case", cases.REJECTS, ids=[c.id for c in cases.REJECTS])
def test_rejected_step_is_not_applied(solver, case):
    """The state returned is the one after the last applied step: bitwise the run capped before the
    rejected iteration (the rejected DX is 0.03 or more in norm, tests/test_hlm_cases_oracle.py)."""
    row = case.rejected_rows()[0]
    full = _run(solver, case)
    before = _run(solver, case, max_iters=row)
    assert before["accepted"] == full["accepted"] and len(before["trace"]) == row
    for k in STATE:
        assert np.array_equal(full[k], before[k]), k


@pytest.mark.parametrize("reject,descend", [(cases.REJECT[0], cases.DERR[0]), (cases.REJECT[4], cases.DERR[1]),
                                            (cases.REJECT[8], cases.DERR[2])],
                         ids=[cases.VARIANT_NAME[v] for v in (cases.PLUCKER, cases.GBA, cases.ENDPOINTS)])
def test_reject_descend_reject_on_one_context(solver, reject, descend):
    """A rejection leaves last_ok ahead of cur; nine applied steps of another window follow, then the
    rejection again: no ring offset leaks from one solve into the next."""
    assert reject.variant == descend.variant
    a = _run(solver, reject)
    b = _run(solver, descend)
    c = _run(solver, reject)
    assert tuple(b["trace"]["result"]) == descend.results and b["accepted"] == 9
    for k in STATE:
        assert np.array_equal(a[k], c[k]), k
    assert np.array_equal(a["trace"], c["trace"])
    assert (a["err"], a["lam"], a["dx_norm"], a["accepted"]) == (c["err"], c["lam"], c["dx_norm"], c["accepted"])


@pytest.mark.parametrize("case", cases.MIN_ERROR_EXACT, ids=[c.id for c in cases.MIN_ERROR_EXACT])
def test_exact_data_stops_on_min_error_alone(solver, case):
    """The Config value min_error = 1e-7 with min_error_change = 0 on exact observations of the true map:
    one step, then err = 6e-12 < min_error stops. The step is rounding noise (g is, ‖DX‖ = 7e-7), so the
    states are not compared, nor is λ = λ0·max|H_ii| (H is built from residuals of 1e-13 px, rounding
    noise as well): the flow, the counters and the deciding err are."""
    out, ref, p = _run(solver, case), case.reference(), case.params()
    tr = out["trace"]
    print(case.id, list(tr["result"]), out["err"], ref["err"], out["dx_norm"], ref["dx_norm"])
    assert tuple(int(r) for r in tr["result"]) == case.results
    assert (out["linearizations"], out["solves"], out["accepted"]) == case.counters
    assert cases.stop_of(out, p) == "min_error" and p.min_error_change == 0.0
    assert out["err"] < p.min_error / 1e3 and tr["chi2_start"][0] < p.min_error / 1e3
    np.testing.assert_array_equal(tr["lambda_end"], tr["lambda_start"])   # no λ·k on the first step, none on a stop
