"""Admission checks of the candidates of tests/hlm_cases.py, on the CPU checkers alone (oracle/refhlm.cpp,
tests/ref_lba_endpoints.py): each reaches the flow it is named for, every decision the loop makes on
the way is at least 1e3 times the checker's own reordering noise from its threshold, the checker's
reordered runs stay within a tenth of every bar of test_gpu_hlm._compare, and the raised-homog_th
cases have the stated rows on either side of the clamp. Prints the figures per case. No GPU needed."""
import numpy as np
import pytest

import hlm_cases as cases
import ref_lba_endpoints

MARGIN_FACTOR = 1e3


def _ids(cs):
    return [c.id for c in cs]


@pytest.mark.parametrize("case", cases.ALL, ids=_ids(cases.ALL))
def test_case_reaches_its_flow_with_a_margin_on_every_decision(case):
    ref, p = case.reference(), case.params()
    assert cases.flow_of(ref) == (case.results, case.counters)
    assert cases.stop_of(ref, p) == case.stop
    adm = cases.admission(case)
    assert len(adm["flows"]) >= 3
    for label, flow in adm["flows"]:
        assert flow == (case.results, case.counters), label
    worst = None
    for i, r in enumerate(adm["rows"]):
        after_reject = r["name"] == "derr" and case.results[r["it"] - 1] == 1
        if after_reject:
            # X did not move: err repeats. A property of the loop, not a margin (exempt)
            assert r["value"] < p.min_error_change / 1e3, r
            continue
        assert r["margin"] >= MARGIN_FACTOR * r["noise"], r
        if worst is None or r["margin"] / max(r["noise"], 1e-300) < worst["margin"] / max(worst["noise"], 1e-300):
            worst = r
    # the comparison is meaningful: the checker against itself in another order is well inside the bars
    assert adm["bar"] <= 0.1, adm["bar"]
    print(f"{case.id}: flow {case.results} {case.counters}, stop {case.stop}; smallest margin {worst['margin']:.3g} "
          f"({worst['name']} at iteration {worst['it']}: {worst['value']:.6g} against {worst['threshold']:.3g}), its "
          f"reordering noise {worst['noise']:.3g}; reordered runs at {adm['bar']:.3g} of the bars")


@pytest.mark.parametrize("case", cases.MIN_ERROR_EXACT, ids=_ids(cases.MIN_ERROR_EXACT))
def test_exact_data_stops_on_min_error_alone(case):
    ref, p = case.reference(), case.params()
    assert cases.flow_of(ref) == (case.results, case.counters) and cases.stop_of(ref, p) == "min_error"
    assert p.min_error_change == 0.0 and ref["err"] < p.min_error / 1e3
    for label, run in cases.reorderings(case):
        assert cases.flow_of(run(p.max_iters)) == (case.results, case.counters), label


@pytest.mark.parametrize("case", cases.REJECTS, ids=_ids(cases.REJECTS))
def test_rejected_step_is_far_above_the_bar(case):
    """The state returned is the one after the last applied step: the run capped before the rejected
    iteration ends bitwise there, and the rejected DX is at least 0.03 in norm."""
    ref = case.reference()
    row = case.rejected_rows()[0]
    before = case.prefix(row)
    for k in ("kf_x", "kf_Tcw", "pt_xyz", "ln_orth", "ln_line3d"):
        assert np.array_equal(ref[k], before[k]), k
    assert cases.history(case.prefix, len(ref["trace"]))[row]["dx"] >= (0.03 if "failed" not in case.name else 0.0)
    tr = ref["trace"]
    assert tr["lambda_end"][row] == tr["lambda_start"][row] / case.params().lambda_k
    if "failed" in case.name:
        assert ref["accepted"] == 0 and ref["dx_norm"] == 0.0


@pytest.mark.parametrize("clamp", cases.CLAMPS, ids=_ids([c.case for c in cases.CLAMPS]))
def test_rows_on_either_side_of_homog_th(clamp):
    case = clamp.case
    hth = case.params().homog_th
    fp = cases.first_pass(case.variant, case.window())
    others = [cases.first_pass(case.variant, cases.permuted(case.variant, case.window(), seed)[0]) for seed in (1, 2, 3)]
    worst = {}
    for key in ("r_pt", "r_ln", "z2_pt", "z2_ln"):
        a = fp[key]
        assert (int((a < hth).sum()), len(a)) == getattr(clamp, key), key
        if len(a):
            # the same rows of the reordered windows (matched by rank: the values are distinct)
            noise = max(np.abs(np.sort(o[key]) - np.sort(a)).max() for o in others)
            gap = np.abs(a - hth).min()
            assert gap > 0.0 and gap >= MARGIN_FACTOR * noise, (key, gap, noise)
            worst[key] = (float(gap), float(noise))
    print(f"{case.id}: below homog_th = {hth:g} on the first linearisation: r {clamp.r_pt} of the point rows, "
          f"{clamp.r_ln} of the line rows; gz² {clamp.z2_pt} of the points, {clamp.z2_ln} of the endpoints; "
          f"(nearest to homog_th, reordering noise) {worst}")


def test_endpoint_lba_uses_homog_th_on_the_first_linearisation_only(monkeypatch):
    case = cases.LATER_PASSES
    ref, hth = case.reference(), case.params().homog_th
    assert case.variant == cases.ENDPOINTS and ref["linearizations"] >= 3 and ref["accepted"] >= 3
    later = cases.first_pass(case.variant, case.window(), case.prefix(1))["r_ln"]
    between = int(((later > 1e-7) & (later < hth)).sum())
    noise = 0.0
    for _, run in cases.reorderings(case):
        noise = max(noise, np.abs(cases.first_pass(case.variant, case.window(), run(1))["r_ln"] - later).max())
    # (few: read at the aliased offset, most line residuals of a later linearisation are tens of pixels)
    assert between == 5 and np.abs(later - hth).min() >= MARGIN_FACTOR * noise
    assert np.minimum(later, np.abs(later - 1e-7)).min() >= MARGIN_FACTOR * noise
    # the checker with homog_th kept on the later linearisations: far beyond the bar
    monkeypatch.setattr(ref_lba_endpoints, "LINE_TH_LATER", hth)
    mut = ref_lba_endpoints.lba(case.window(), case.params())
    fig = cases.bar_figures(mut, ref, case.window()) if cases.flow_of(mut) == cases.flow_of(ref) else {"flow": np.inf}
    print(f"{case.id}: {between} of {len(later)} line rows of the second linearisation between 1e-7 and {hth:g} "
          f"(noise {noise:.3g}); homog_th kept on later passes: {max(fig.values()):.3g} times the bar")
    assert max(fig.values()) >= 100.0


@pytest.mark.parametrize("case", [c for c in cases.ALL if c.variant == cases.GBA and dict(c.prm).get("homog_th", 1e-7) == 1e-7
                                  and dict(c.prm).get("err_per_obs")],
                         ids=lambda c: c.id)
def test_both_checkers_agree_on_the_flow_of_gba(case):
    """tests/ref_lba_endpoints.py on a GBA window with err_per_obs = 1 and homog_th = 1e-7 differs from
    oracle/refhlm.cpp's GBA by the int Hmax alone (λ0·Hmax truncated: a relative 1e-9 here)."""
    other = ref_lba_endpoints.lba(case.window(), case.params())
    assert cases.flow_of(other) == (case.results, case.counters)
