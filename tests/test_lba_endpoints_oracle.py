"""The numpy checker of the endpoint-line local BA (tests/ref_lba_endpoints.py) pinned on the CPU:
its per-observation kernels against oracle/refhlm.cpp, its landmark rows against central
differences, its block-Schur solve against the literal dense H, and the two quirks of
MapHandler::levMarquardtOptimizationLBA (src/mapHandler.cpp:2334-2840) that no other variant has
in this combination: the aliased endpoint reads and the infinite first err."""
import numpy as np
import pytest

import oracle_api as oa
import ref_lba_endpoints as ref
from plba import capi, synth
from plba.hlm import lba_window


@pytest.fixture(scope="module")
def c1l():
    return lba_window(synth.generate("C1L"))


def _close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1.0), (np.abs(a - b).max(), np.abs(b).max())


def test_lba_window_keeps_the_windows_fixed_keyframes():
    g = synth.generate("C1", n_kf=12, n_pt=80, fixed_frac=0.5)
    w = lba_window(g)
    np.testing.assert_array_equal(w.graph.kf_fixed, g.kf_fixed)
    assert w.graph.kf_fixed.sum() == 6
    p = capi.lba_params()
    assert (p.variant, p.lambda0, p.lambda_k, p.max_iters) == (capi.HLM_LBA_ENDPOINTS, 1e-5, 10.0, 15)
    assert (p.min_error, p.min_error_change, p.homog_th, p.err_per_obs) == (1e-7, 1e-7, 1e-7, 0)


def test_observation_kernels_match_refhlm(c1l):
    g = c1l.graph
    pb = ref.Problem(c1l, capi.lba_params())
    T = pb.Tmap
    for hth in (1e-7, 1e-3):
        r, w, Jp, Jl = ref.point_obs(T[pb.ept_kf], pb.Xp[pb.ept_lm], pb.ept_obs, pb.cam, hth)
        for e in range(0, g.n_ept, 7):
            o = oa.hlm_point_obs(T[pb.ept_kf[e]], pb.Xp[pb.ept_lm[e]], pb.ept_obs[e], pb.cam, hth)
            for a, b in zip((r[e], w[e], Jp[e], Jl[e]), o):
                _close(a, b, 1e-13)
        P, Q = pb.Xl[pb.eln_lm, :3], pb.Xl[pb.eln_lm, 3:]
        r, w, Jp, Jl = ref.line_obs(T[pb.eln_kf], P, Q, pb.eln_obs, pb.cam, hth)
        for e in range(0, g.n_eln, 3):
            o = oa.gba_line_obs(T[pb.eln_kf[e]], P[e], Q[e], pb.eln_obs[e], pb.cam, hth)
            for a, b in zip((r[e], w[e], Jp[e], Jl[e]), o):
                _close(a, b, 1e-13)
            o = oa.gba_line_obs(T[pb.eln_kf[e]], P[e], P[e], pb.eln_obs[e], pb.cam, hth)   # the aliased read
            q = ref.line_obs(T[pb.eln_kf[e:e + 1]], P[e:e + 1], P[e:e + 1], pb.eln_obs[e:e + 1], pb.cam, hth)
            for a, b in zip((q[0][0], q[1][0], q[2][0], q[3][0]), o):
                _close(a, b, 1e-13)


def _cdiff(f, x, h=1e-6):
    out = []
    for i in range(len(x)):
        d = np.zeros(len(x))
        d[i] = h
        out.append((f(x + d) - f(x - d)) / (2 * h))
    return np.array(out)


def test_landmark_rows_against_central_differences(c1l):
    """Point row: J = −∂r/∂X (the reference writes the descent direction, X += DX). Line row: the
    reference builds it with (fx·e0, fy·e1) where ∂r/∂P has (fx·a, fy·b) — it is not a gradient;
    what it is, Jl_P = (e0/m)·(∂π(P)/∂P)ᵀ·(e0, e1) and the same for Q with e1, is checked with
    ∂π/∂P from central differences of the projection."""
    pb = ref.Problem(c1l, capi.lba_params())
    T, cam = pb.Tmap, pb.cam
    fx, fy, cx, cy = cam
    for e in range(0, len(pb.ept_kf), 29):
        Te, ob = T[pb.ept_kf[e]][None], pb.ept_obs[e][None]
        X = pb.Xp[pb.ept_lm[e]]
        _, _, _, Jl = ref.point_obs(Te, X[None], ob, cam, 1e-7)
        gr = _cdiff(lambda x: ref.point_obs(Te, x[None], ob, cam, 1e-7)[0][0], X)
        _close(Jl[0], -gr, 1e-6)

    def proj(Te, x):
        G = Te[:, :3] @ x + Te[:, 3]
        return np.array([cx + fx * G[0] / G[2], cy + fy * G[1] / G[2]])
    for e in range(0, len(pb.eln_kf), 11):
        Te, lo = T[pb.eln_kf[e]], pb.eln_obs[e]
        P, Q = pb.Xl[pb.eln_lm[e], :3], pb.Xl[pb.eln_lm[e], 3:]
        r, _, _, Jl = ref.line_obs(Te[None], P[None], Q[None], lo[None], cam, 1e-7)
        e0 = lo[:2] @ proj(Te, P) + lo[2]
        e1 = lo[:2] @ proj(Te, Q) + lo[2]
        assert r[0] == pytest.approx(np.hypot(e0, e1), rel=1e-12)
        for V, ek, row in ((P, e0, Jl[0, :3]), (Q, e1, Jl[0, 3:])):
            dpi = _cdiff(lambda x: proj(Te, x), V)          # (3, 2): ∂π/∂V transposed
            _close(row, (ek / max(1e-7, r[0])) * (dpi @ np.array([e0, e1])), 1e-6)


def test_schur_solve_equals_dense_solve(c1l):
    p = capi.lba_params()
    pb = ref.Problem(c1l, p)
    for first in (True, False):
        lin = pb.linearize(first)
        for lam in (p.lambda0 * pb.hmax(lin), 1e-3):
            ok_s, xs = pb.solve(lin, lam, dense=False)
            ok_d, xd = pb.solve(lin, lam, dense=True)
            assert ok_s and ok_d
            _close(xs, xd, 1e-9)
    a = ref.lba(c1l, capi.lba_params(max_iters=4))
    b = ref.lba(c1l, capi.lba_params(max_iters=4), dense=True)
    assert (a["linearizations"], a["solves"], a["accepted"]) == (b["linearizations"], b["solves"], b["accepted"])
    for k in ("kf_x", "pt_xyz", "ln_line3d"):
        _close(a[k], b[k], 1e-9)


def test_later_linearisations_read_both_endpoints_from_the_aliased_offset(c1l):
    pb = ref.Problem(c1l, capi.lba_params())
    j = pb.n_ln - 1                       # its own Q slot, 6j+3.., is no line's aliased slot (3k = 6j+3 -> k >= n_ln)
    mine = pb.eln_lm == j
    assert mine.any()
    base = pb.linearize(False)
    # positive: X[6Nkf+3Npt+3j .. +3) — inside line (3j)//6's block — moves line j's residuals and rows
    keep = pb.Xl.copy()
    pb.Xl.reshape(-1)[3 * j:3 * j + 3] += 0.05
    assert (3 * j) // 6 != j
    moved = pb.linearize(False)
    assert np.all(moved["rl"][mine] != base["rl"][mine])
    assert np.any(moved["Hln"][j] != base["Hln"][j])
    pb.Xl[:] = keep
    # negative: line j's own Q slot is read by nothing after the first linearisation
    pb.Xl[j, 3:] += 0.05
    same = pb.linearize(False)
    for k in ("rl", "Jll", "Jpl", "Hln", "gln", "Hpp", "gp"):
        np.testing.assert_array_equal(same[k], base[k])
    first = pb.linearize(True)            # ... while the first linearisation does read it
    pb.Xl[:] = keep
    assert np.all(first["rl"][mine] != pb.linearize(True)["rl"][mine])
    # and P == Q there: the two halves of every line row coincide
    np.testing.assert_array_equal(base["Jll"][:, :3], base["Jll"][:, 3:])


@pytest.mark.parametrize("cfg", ["C1L", "C1"])
def test_first_err_is_infinite_and_the_second_step_is_always_applied(cfg):
    win = lba_window(synth.generate(cfg))
    out = ref.lba(win, capi.lba_params(max_iters=3))
    tr = out["trace"]
    assert np.isposinf(tr["chi2_start"][0])          # err / (Npt_obs + Nls_obs) == err / 0
    assert np.isfinite(tr["chi2_start"][1])          # err / (Npt + Nls)
    assert list(tr["result"][:2]) == [0, 0] and out["accepted"] >= 2
    assert tr["lambda_end"][1] == pytest.approx(tr["lambda_start"][1] * 10.0)
    # even from a state whose err grows: start the points far off, the second step is still applied
    far = lba_window(synth.generate(cfg))
    far.graph.pt_xyz = far.graph.pt_xyz + 0.5
    o2 = ref.lba(far, capi.lba_params(max_iters=2, lambda0=1e-12))
    assert list(o2["trace"]["result"]) == [0, 0] and o2["accepted"] == 2
    # err_per_obs = 1 divides both by the observation count: finite from the start
    o3 = ref.lba(win, capi.lba_params(max_iters=2, err_per_obs=1))
    assert np.isfinite(o3["trace"]["chi2_start"][0])
