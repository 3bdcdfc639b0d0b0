"""The device on windows whose points lie behind cameras, and on windows that end the damped trial
loop early (tests/depth_cases.py; the checker's side of each is tests/test_depth_oracle.py).

On the synthetic windows every camera-frame depth is positive and every iteration ends on an
accepted trial or after maxTrials, so the depth term of the stage-switch classification (k_linearize),
the depth bytes of the downloads (k_out_scatter; k_depth + k_gather when sharded) and the ρ == 0 and
non-finite-λ ends of k_decide only ever showed one outcome. Here both outcomes occur, no depth is
within 1e-6 of zero (so the flags must equal the checker's exactly), and at least two edges per
window reach level 1 through the depth term alone."""
import numpy as np
import pytest

import depth_cases as dc
from parity import assert_trace_parity
from test_gpu_build import KEYS, STRUCT
from test_gpu_build import _solve as _build_solve
from test_gpu_edge_cases import _amax, _check
from test_gpu_spec import _assert_same
from test_gpu_spec import _solve as _spec_solve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


@pytest.fixture(scope="module")
def device_first(solver):
    """The device's full schedule on the "first" variant, and on its points alone."""
    res = {}
    for order in dc.ORDERS:
        solver.upload(dc.order_windows(order)[0])
        res[order] = solver.lba_plucker()
    return res


@pytest.mark.parametrize("name", list(dc.VARIANTS))
def test_full_schedule_matches_oracle(solver, name):
    ref, ref1 = dc.oracle(name), dc.oracle_stage1(name)
    solver.upload(dc.window(name))
    out = solver.lba_plucker()
    np.testing.assert_array_equal(out["ept_depth_ok"], ref["ept_depth_ok"])
    np.testing.assert_array_equal(out["ept_level"], ref["ept_level"])
    np.testing.assert_array_equal(out["eln_level"], ref["eln_level"])
    only = dc.depth_only(ref, ref1)
    assert only.sum() >= 2 and (out["ept_level"][only] == 1).all(), out["ept_level"][only]
    _check(out, ref)
    assert_trace_parity(out, ref)


@pytest.mark.parametrize("name", list(dc.VARIANTS))
def test_g2o_style_call_sequence_reads_depth_after_stage_one(solver, name):
    """plba_get_edge_chi2 after optimize(5): the flags at the classification, where they decide
    levels, and again after stage 2 and the level-1 refresh."""
    g = dc.window(name)
    ref, ref1 = dc.oracle(name), dc.oracle_stage1(name)
    solver.upload(g)
    solver.set_robust(True)
    solver.initialize_optimization(0)
    it, _ = solver.optimize(5)
    assert it == ref1["iters"][0]
    pc, pd, lc = solver.edge_chi2()
    np.testing.assert_array_equal(pd, ref1["ept_depth_ok"])
    np.testing.assert_allclose(pc, ref1["ept_chi2"], rtol=1e-6, atol=1e-9)
    pl = ((pc > dc.CHI2_THR) | (pd == 0)).astype(np.uint8)
    ll = (lc > dc.CHI2_THR).astype(np.uint8)
    np.testing.assert_array_equal(pl, ref["ept_level"])
    np.testing.assert_array_equal(ll, ref["eln_level"])
    only = dc.depth_only(ref, ref1)
    assert (pc[only] <= dc.CHI2_THR).all() and (pd[only] == 0).all() and (pl[only] == 1).all()
    solver.set_edge_levels(pl, ll)
    solver.set_robust(False)
    solver.initialize_optimization(0)
    it2, _ = solver.optimize(10)
    assert it2 == ref["iters"][1]
    solver.refresh_edge_errors(1)
    pc2, pd2, lc2 = solver.edge_chi2()
    np.testing.assert_array_equal(pd2, ref["ept_depth_ok"])
    np.testing.assert_allclose(pc2, ref["ept_chi2"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(lc2, ref["eln_chi2"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("order", dc.ORDERS)
def test_flags_come_back_in_the_callers_order(solver, device_first, order):
    """Shuffled keyframes, landmarks, ids and edges: the flags are the checker's for the shuffled
    window and the unshuffled device flags in the recorded edge order, with lines after the points
    (Ep < E) and without (Ep == E). Both through plba_lba_plucker and through plba_get_edge_chi2."""
    g, h = dc.order_windows(order)
    base = device_first[order]
    _check(base, dc.order_oracle(order, 0))
    ref = dc.order_oracle(order, 1)
    solver.upload(h)
    out = solver.lba_plucker()
    _, pd, _ = solver.edge_chi2()
    pe = h._perm["pe"]
    for flags in (out["ept_depth_ok"], pd):
        np.testing.assert_array_equal(flags, ref["ept_depth_ok"])
        np.testing.assert_array_equal(flags, base["ept_depth_ok"][pe])
    np.testing.assert_array_equal(out["ept_level"], ref["ept_level"])
    np.testing.assert_array_equal(out["ept_level"], base["ept_level"][pe])
    _check(out, ref)
    # after stage 1 as well (the other download path's flags at the classification)
    ref1 = dc.order_oracle(order, 1, stage1=True)
    solver.upload(h)
    solver.set_robust(True)
    solver.initialize_optimization(0)
    solver.optimize(5)
    _, pd1, _ = solver.edge_chi2()
    np.testing.assert_array_equal(pd1, ref1["ept_depth_ok"])


@pytest.mark.parametrize("case", ["first", "first_shuffled"])
def test_device_build_equals_host_build(monkeypatch, case):
    g = dc.window("first") if case == "first" else dc.order_windows("mixed")[1]
    st_d, out_d = _build_solve(monkeypatch, g, host=False)
    st_h, out_h = _build_solve(monkeypatch, g, host=True)
    assert st_d["device_build"] == 1 and st_h["device_build"] == 0, (st_d, st_h)
    for k in STRUCT:
        assert st_d[k] == st_h[k], (k, st_d, st_h)
    for k in KEYS:
        assert np.array_equal(out_d[k], out_h[k]), k
    assert 20 <= int((out_d["ept_depth_ok"] == 0).sum()) <= g.n_ept - 20


def test_no_solve_depth_signs(solver):
    """Depths of exactly 0.0, -0.0, 5e-324 and -5e-324: isDepthPositive is Pc[2] > 0, so only the
    smallest positive double passes. No optimize(): the edges at those depths have non-finite
    errors, which must not reach a factorisation."""
    g = dc.no_solve_window()
    ref, chi2 = dc.no_solve_oracle()
    solver.upload(g)
    solver.refresh_edge_errors(0)       # computeError() of every edge (all on level 0)
    pc, pd, lc = solver.edge_chi2()
    np.testing.assert_array_equal(pd[1::2], dc.NO_SOLVE_FLAGS_KF1)
    np.testing.assert_array_equal(pd[0::2], 1)
    np.testing.assert_array_equal(pd, ref["ept_depth_ok"])
    fin = np.isfinite(chi2)
    np.testing.assert_array_equal(np.isfinite(pc), fin)
    np.testing.assert_allclose(pc[fin], chi2[fin], rtol=1e-6, atol=1e-9)
    assert lc.size == 0
    T, P, _ = solver.download()
    np.testing.assert_array_equal(T, g.kf_Tcw)
    np.testing.assert_array_equal(P, g.pt_xyz)
    assert np.signbit(P[1]).all() and np.signbit(T[1, 2, 3])
    # the schedule's view: the checker's levels, computeError() of the level-1 edges only
    solver.upload(g)
    solver.set_edge_levels(ref["ept_level"], np.zeros(0, np.uint8))
    solver.refresh_edge_errors(1)
    pc1, pd1, _ = solver.edge_chi2()
    np.testing.assert_array_equal(pd1, ref["ept_depth_ok"])
    np.testing.assert_array_equal(np.isfinite(pc1), np.isfinite(ref["ept_chi2"]))
    lv0 = ref["ept_level"] == 0
    np.testing.assert_array_equal(pc1[lv0], ref["ept_chi2"][lv0])


@pytest.mark.parametrize("name", list(dc.TERMINATION))
def test_trial_loop_ends_early_like_the_oracle(name):
    """ρ == 0 (Terminate after one trial) and, with τ = 2e300, λ·ν = +inf in the first trial of the
    Huber stage (Terminate with no trial counted), on the points of C1L: iteration counts, the whole
    trace and the estimates against the checker, with one trial slot. Every trial state is bitwise
    the current one (depth_cases), so ρ == 0 must be exact on the device as well: a trial χ² that
    differed from currentChi by rounding would retry (ρ < 0, ten trials) or accept (ρ > 0)."""
    g = dc.termination_window()
    ref = dc.termination_oracle(name)
    tau = dc.TERMINATION[name]["tau"]
    out, _, st = _spec_solve(g, 1, 0, tau=tau)
    assert st["spec_slots"] == 1
    tg, tr = out["trace"], ref["trace"]
    print(name, "device", [(int(t["stage"]), int(t["iter"]), int(t["trials"]), int(t["result"]), float(t["chi2_start"]),
                            float(t["chi2_end"]), float(t["lambda_start"]), float(t["lambda_end"])) for t in tg])
    print(name, "oracle", [(int(t["stage"]), int(t["iter"]), int(t["trials"]), int(t["result"]), float(t["chi2_start"]),
                            float(t["chi2_end"]), float(t["lambda_start"]), float(t["lambda_end"])) for t in tr])
    np.testing.assert_array_equal(out["iters"], ref["iters"])
    assert len(tg) == len(tr)
    for k in ("stage", "iter", "trials", "result"):
        np.testing.assert_array_equal(tg[k], tr[k], err_msg=k)
    for k in ("lambda_start", "lambda_end"):
        np.testing.assert_allclose(tg[k], tr[k], rtol=1e-12, err_msg=k)
    assert_trace_parity(out, ref)
    _check(out, ref)


@pytest.mark.parametrize("name", list(dc.TERMINATION))
def test_trial_loop_end_is_bitwise_with_speculative_slots(name):
    """The same windows with PLBA_SPEC=3, PLBA_SPEC_POLICY=1: whichever way the loop ends, three
    trial slots must be bitwise the one-slot run (estimates, χ², flags, iteration counts and the
    whole trace), on a second schedule too, and nothing may move or turn non-finite."""
    g = dc.termination_window()
    tau = dc.TERMINATION[name]["tau"]
    out, out2, st = _spec_solve(g, 1, 0, tau=tau)
    assert st["spec_slots"] == 1
    for k in ("kf_Tcw", "pt_xyz", "ln_orth"):
        assert np.isfinite(out[k]).all() and _amax(out[k] - getattr(g, k)) <= 1e-12, k
    _assert_same(out, out2, "second schedule")
    spec, spec2, st3 = _spec_solve(g, 3, 1, tau=tau)
    assert st3["spec_slots"] == 3 and st3["spec_policy"] == 1, st3
    _assert_same(out, spec, "three slots")
    _assert_same(out, spec2, "three slots, second schedule")
