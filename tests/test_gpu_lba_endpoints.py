"""Endpoint-line local BA on the GPU (plba_hlm_lba, variant PLBA_HLM_LBA_ENDPOINTS, Ctrl::hlm = 3)
against the numpy checker tests/ref_lba_endpoints.py.

MapHandler::levMarquardtOptimizationLBA (src/mapHandler.cpp:2334-3016). The acceptance bar is
test_gpu_hlm._compare: identical control flow and trace, λ to 1e-9, err to 1e-9, ‖DX‖ to 1e-4 and
each estimate within 1e-4 of the checker's total change."""
import ctypes as C

import numpy as np
import pytest

import ref_lba_endpoints as ref
from plba import capi, synth
from plba.hlm import gba_window, hlm_window, lba_window
from test_gpu_hlm import _compare

pytestmark = pytest.mark.gpu

STATE = ("kf_x", "kf_Tcw", "pt_xyz", "ln_line3d")


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _run(solver, win, p):
    solver.upload(win.graph)
    return solver.hlm_lba(win, p)


def test_variant_2_runs_and_an_unknown_variant_is_refused(solver):
    from plba.lib import PlbaError
    win = lba_window(synth.generate("C1L"))
    out = _run(solver, win, capi.lba_params())
    assert capi.HLM_LBA_ENDPOINTS == 2 and out["linearizations"] >= 2 and out["accepted"] >= 2
    assert np.abs(out["ln_line3d"] - win.ln_line3d).max() > 0        # ln_line3d is filled at exit
    with pytest.raises(PlbaError, match="PLBA_E_INVALID"):
        solver.hlm_lba(win, capi.lba_params(variant=7))


CASES = [("C1L", {}), ("C1", {}), ("C2", {}), ("C1L", {"lambda0": 1e-24}), ("C2", {"max_iters": 4})]


@pytest.mark.parametrize("cfg,params", CASES, ids=[f"{c}-{'-'.join(f'{k}={v}' for k, v in p.items()) or 'ref'}"
                                                  for c, p in CASES])
def test_lba_endpoints_matches_checker(solver, cfg, params):
    win = lba_window(synth.generate(cfg))
    p = capi.lba_params(**params)
    _compare(_run(solver, win, p), ref.lba(win, p), win)


def test_fixed_observers_and_an_idle_free_keyframe(solver):
    """Half the keyframes fixed: observations with kf_idx_loc == -1 add to the landmark block and g
    only (:2417-2423, :2530-2536); a point and a line seen by fixed KFs alone take the
    landmark-only branch for every observation; a free KF without observations gets the unit
    diagonal (INTEGRATION.md B')."""
    g = synth.generate("C1L", n_kf=6, n_pt=60, n_ln=12, seed=5, fixed_frac=0.5)
    fixed = g.kf_fixed != 0
    assert fixed.sum() == 3

    def only_fixed(lm, kf, n):
        return [l for l in range(n) if (lm == l).any() and fixed[kf[lm == l]].all()]
    idle = int(np.nonzero(~fixed)[0][-1])                 # drop every observation of one free KF
    kp, kl = g.ept_kf != idle, g.eln_kf != idle
    g.ept_lm, g.ept_kf, g.ept_obs, g.ept_info = g.ept_lm[kp], g.ept_kf[kp], g.ept_obs[kp], g.ept_info[kp]
    g.eln_lm, g.eln_kf, g.eln_obs, g.eln_info = g.eln_lm[kl], g.eln_kf[kl], g.eln_obs[kl], g.eln_info[kl]
    assert only_fixed(g.ept_lm, g.ept_kf, g.n_pt) and only_fixed(g.eln_lm, g.eln_kf, g.n_ln)
    assert not (g.ept_kf == idle).any() and not (g.eln_kf == idle).any()
    for lm, n in ((g.ept_lm, g.n_pt), (g.eln_lm, g.n_ln)):
        assert len(np.unique(lm)) == n                    # every landmark keeps an observation
    win = lba_window(g)
    p = capi.lba_params()
    out, exp = _run(solver, win, p), ref.lba(win, p)
    _compare(out, exp, win)
    # DX_i = 0 exactly: X_i only goes through log(exp(X_i)·I) once per applied step, a round trip
    # that costs a few ulp of |X_i| <= 2.5 each (at most 15 steps: well under 1e-13)
    np.testing.assert_allclose(out["kf_x"][idle], win.kf_x[idle], rtol=0, atol=1e-13)
    assert np.abs(exp["kf_x"][idle] - win.kf_x[idle]).max() <= 1e-13
    assert out["accepted"] >= 2


def test_wide_band_family(solver):
    g = synth.generate("C1", n_kf=30, n_pt=400, n_ln=60, seed=35, track_min=2, track_max=30, fixed_frac=0.1)
    win = lba_window(g)
    p = capi.lba_params()
    solver.upload(win.graph)
    st = solver.structure_stats()
    assert st["banded"] == 1 and st["column_lane"] == 0 and st["bcr_rows"] == 0 and st["bw"] >= 10, st
    _compare(solver.hlm_lba(win, p), ref.lba(win, p), win)


def test_two_sided_column_lane_family_short_trajectory(solver):
    """The same family on a 60-KF window whose keyframe rotations stay away from π (largest angle
    2.09 rad), so the comparison does not lean on the operation order of the se(3) maps: a 1-ulp
    change of the input x_kf_w moves the checker's poses by 7e-15 there, against a bound of 2.4e-9."""
    win = lba_window(synth.generate("C3", n_kf=60, n_pt=6000, n_ln=1200))
    p = capi.lba_params(max_iters=4)
    solver.upload(win.graph)
    st = solver.structure_stats()
    assert st["column_lane"] == 1 and st["twisted"] == 1 and st["bcr_rows"] == 0 and st["nf"] == 54, st
    _compare(solver.hlm_lba(win, p), ref.lba(win, p), win)


def test_two_sided_column_lane_family(solver):
    """C3, max_iters = 4. KF 94 of the C3 trajectory is free in this window and its rotation angle is
    3.14017 rad, 1.4e-3 short of π, where logmap_se3 (src2/auxiliar.cpp:143-173: sine = sqrt(1 −
    cosine²), ω = θ·(R − Rᵀ)/(2·sine)) amplifies a 1-ulp difference in T by ~1/sin²θ ≈ 5e5; the bound
    on kf_Tcw is 1.7e-9 because this variant's λ = 1e-5·Hmax ≈ 590 barely moves the window. The
    device keeps the reference's operation order in its se(3) maps, so the checker has to as well
    (ref_lba_endpoints.pose_update): with numpy maps in another order it sat 2.3e-9 from the device;
    with the reference's order the two agree to 3.8e-14 (err to 8e-16, ‖DX‖ to 6e-14 relative)."""
    win = lba_window(synth.generate("C3"))
    p = capi.lba_params(max_iters=4)
    solver.upload(win.graph)
    st = solver.structure_stats()
    assert st["column_lane"] == 1 and st["twisted"] == 1 and st["bcr_rows"] == 0, st
    _compare(solver.hlm_lba(win, p), ref.lba(win, p), win)


def test_block_cyclic_reduction_family(solver):
    """The smallest window plba_factor_plan sends to block cyclic reduction (each factor kernel
    embeds the pose update, so each family runs the new variant once)."""
    L = solver.L
    kw = dict(n_pt=3000, n_ln=300, seed=77, fixed_frac=0.0)
    solver.upload(lba_window(synth.generate("C1", n_kf=40, **kw)).graph)
    bw = solver.structure_stats()["bw"]                    # set by the track length, not by n_kf
    plan = (C.c_int32 * 9)()
    nf = next(n for n in range(2, 2000)
              if L.plba_factor_plan(bw, n, 256, 4, plan, 9) == 0 and plan[0] == 6)
    assert L.plba_factor_plan(bw, nf - 1, 256, 4, plan, 9) == 0 and plan[0] != 6
    g = synth.generate("C1", n_kf=nf + 1, **kw)            # fixed_frac 0: one fixed KF
    assert (g.kf_fixed == 0).sum() == nf
    win = lba_window(g)
    p = capi.lba_params(max_iters=3)
    solver.upload(win.graph)
    st = solver.structure_stats()
    assert st["nf"] == nf and st["bw"] == bw and st["bcr_rows"] > 0, (st, nf, bw)
    _compare(solver.hlm_lba(win, p), ref.lba(win, p), win)
    assert solver.structure_stats()["bcr_fallbacks"] == 0


def test_reruns_are_bitwise_equal(solver):
    win = lba_window(synth.generate("C2"))
    p = capi.lba_params(max_iters=5)
    solver.upload(win.graph)
    a = solver.hlm_lba(win, p)
    b = solver.hlm_lba(win, p)
    for k in STATE:
        assert np.array_equal(a[k], b[k]), k
    assert (a["err"], a["lam"], a["dx_norm"]) == (b["err"], b["lam"], b["dx_norm"])


def test_mixed_use_of_one_context(solver):
    """Variant 2, the g2o schedule, GBA (variant 1) and variant 2 again on one context: the first
    and the last result are bitwise equal (no state of another variant leaks into the step graph)."""
    g = synth.generate("C1L")
    win, gwin, hwin = lba_window(g), gba_window(g), hlm_window(g)
    p = capi.lba_params()
    a = _run(solver, win, p)
    solver.upload(hwin.graph)
    b = solver.lba_plucker()
    c = _run(solver, gwin, capi.gba_params())
    d = _run(solver, win, p)
    assert b["iters"][0] > 0 and c["linearizations"] >= 2
    for k in STATE:
        assert np.array_equal(a[k], d[k]), k
    assert (a["linearizations"], a["accepted"], a["err"], a["lam"]) == (d["linearizations"], d["accepted"], d["err"], d["lam"])
