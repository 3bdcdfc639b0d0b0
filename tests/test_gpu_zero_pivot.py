"""Real zero pivots in every factorisation of the reduced camera system (column-lane, band window,
block cyclic reduction, dense; one sweep and two-sided, fused and split, scalar and MFMA) and at
every row position where one of them changes hands: first and last row, the first full window,
the separator rows of the two-sided kernels, super-row boundaries, rows that straddle two panels.

LinearSolverEigen fails iff an LDLᵀ pivot is exactly 0; the trial is then
rejected, x keeps its previous value and the update is still applied. Each factorisation carries
its own copy of that rule. The matrix (tests/zero_pivot_cases.py; its preconditions are checked on
the CPU by tests/test_zero_pivot_oracle.py) puts a keyframe whose edges all carry Ω = 0 on a chosen
row: its block row of the system is exactly zero, so at λ = 0 the pivot there is exactly zero in
any elimination order (a), and at the default τ it is exactly λ, decoupled, with a zero right-hand
side (b). A free keyframe without edges (c) is not in g2o's system at all: its row is the
identity and must not fail anything.

The environment switches are sampled at upload, so one context per τ serves every case."""
import numpy as np
import pytest

import graph_mut as gm
import zero_pivot_cases as zc
from parity import ELEM_ATOL, compare
from test_gpu_edge_cases import _amax, _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gn_solver():
    """τ = 0: λ = 0 in every trial."""
    from plba.lib import Solver
    s = Solver(tau=0.0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _upload(s, g, want):
    s.upload(g)
    st = s.structure_stats()
    assert {k: st[k] for k in want} == want, (want, st)
    return st


def _huber_stage(s):
    s.set_robust(True)
    s.initialize_optimization(0)
    it, chi = s.optimize(5)
    tr = s.trace()
    return it, chi, tr, s.download()


# ---- (a) an exact zero pivot
KEYS = ("kf_Tcw", "pt_xyz", "ln_orth", "ept_chi2", "eln_chi2", "ept_level", "eln_level", "ept_depth_ok", "iters",
        "chi2", "trace")
_clean = {}


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x))
    return x.shape, x.dtype, x.tobytes()  # bitwise: the NaN χ² of a diverged λ = 0 schedule included


def _clean_solve(c):
    """The full schedule of the case's unmodified window at τ = 0 in a context of its own, which
    never saw a failed solve (the case's switches are set by the caller)."""
    if c.id not in _clean:
        from plba.lib import Solver
        with Solver(tau=0.0) as s:
            _upload(s, zc.window(c.window), c.stats)
            _clean[c.id] = s.lba_plucker()
    return _clean[c.id]


@pytest.mark.parametrize("cid,row", zc.case_rows())
def test_exact_zero_pivot_rejects_every_trial(gn_solver, monkeypatch, cid, row):
    """The solve fails in all ten trials of the only iteration and nothing moves. The context then
    solves the unmodified window bit for bit as a context that never failed does: no failure
    word, hand-off record or epoch is left behind.

    (That last comparison is device against device. At λ = 0 the full schedule of an unmodified
    window is undamped Gauss-Newton, and the checker gives no result to hold it to: on the 14-KF
    column-lane window its first iteration rejects all ten trials on ρ and its second stage ends
    with χ² = NaN; the device agrees with it to 1.7 element bars on the lines there and to 4e7 and
    1e7 bars on the 16- and 24-KF band windows, which is the conditioning of that schedule, the
    same with every factorisation. Parity with the checker on these windows and paths is (b).)"""
    c, s = zc.BY_ID[cid], gn_solver
    _setenv(monkeypatch, c.env)
    clean = _clean_solve(c)
    g, ref = zc.zero_window(c.window, row), zc.zero_oracle_gn(c.window, row)
    _upload(s, g, c.stats)
    it, chi, tr, (T, P, O) = _huber_stage(s)
    print(cid, row, "iters", it, "trace", tr, "chi2 rel", abs(chi - ref["chi2"][0]) / ref["chi2"][0],
          "finite", bool(np.isfinite(T).all() and np.isfinite(P).all() and np.isfinite(O).all()))
    assert it == ref["iters"][0] == 1
    assert len(tr) == 1 and tr[0]["trials"] == 10 and tr[0]["result"] == 1, tr
    assert tr[0]["lambda_start"] == 0.0 and tr[0]["lambda_end"] == 0.0
    assert abs(chi - ref["chi2"][0]) <= 1e-9 * ref["chi2"][0]
    np.testing.assert_array_equal(T, g.kf_Tcw)
    np.testing.assert_array_equal(P, g.pt_xyz)
    np.testing.assert_array_equal(O, g.ln_orth)
    if c.mode == zc.BCR:  # a failed solve, not a hand-off timeout
        st = s.structure_stats()
        assert st["bcr_fallbacks"] == 0 and st["bcr_rows"] == c.stats["bcr_rows"] > 0, st
    _upload(s, zc.window(c.window), c.stats)
    after = s.lba_plucker()
    for k in KEYS:
        assert _bits(after[k]) == _bits(clean[k]), (cid, row, k)
    if c.mode == zc.BCR:
        assert s.structure_stats()["bcr_fallbacks"] == 0


# ---- (b) a tiny decoupled pivot
@pytest.mark.parametrize("cid,row", zc.case_rows())
def test_zero_information_row_with_damping(solver, monkeypatch, cid, row):
    """Default τ: the zero-information row has pivots of exactly λ and right-hand side 0. The full
    schedule matches the checker's and the keyframe stays where the checker leaves it."""
    c, s = zc.BY_ID[cid], solver
    _setenv(monkeypatch, c.env)
    g, ref = zc.zero_window(c.window, row), zc.zero_oracle(c.window, row)
    _upload(s, g, c.stats)
    out = s.lba_plucker()
    k = gm.free_rows(g)[row]
    d = _amax(out["kf_Tcw"][k] - ref["kf_Tcw"][k])
    print(cid, row, compare(out, ref), "iters", out["iters"], ref["iters"], "keyframe", d)
    _check(out, ref)  # every case meets the element bar of 1: no exception taken
    assert d <= ELEM_ATOL, d
    if c.mode == zc.BCR:
        assert s.structure_stats()["bcr_fallbacks"] == 0


# ---- (c) an idle free pose at λ = 0
@pytest.mark.parametrize("cid,kind", zc.idle_cases())
def test_idle_free_pose_is_inactive_on_every_path(gn_solver, monkeypatch, cid, kind):
    """A free keyframe without edges is no vertex of g2o's system: on whatever row it lands, the
    solve at λ = 0 must not fail and must be the solve of the window without it, by the same
    factorisation (GPU against GPU, as in test_idle_free_pose_is_inactive_at_zero_lambda; the
    checker agrees on the iteration and trial counts and on the pose staying put)."""
    c, s = zc.IDLE_BY_ID[cid], gn_solver
    _setenv(monkeypatch, c.env)
    r, nf, bw = zc.idle_row(cid, kind)
    base, g, ref = zc.window(c.window), zc.idle_window(c.window, r), zc.idle_oracle_gn(c.window, r)
    assert gm.free_rows(g)[r] == g.n_kf - 1
    _upload(s, g, dict(c.stats, nf=nf, bw=bw))
    it, chi, tr, (T, P, O) = _huber_stage(s)
    _upload(s, base, dict(c.stats, nf=nf - 1))
    it0, chi0, tr0, (T0, P0, O0) = _huber_stage(s)
    print(cid, kind, (r, nf, bw), "iters", it, it0, ref["iters"][0], "trials", [int(t["trials"]) for t in tr],
          [int(t["trials"]) for t in tr0], [int(t["trials"]) for t in ref["trace"]],
          "chi2 rel", abs(chi - chi0) / chi0, "T", _amax(T[:-1] - T0), "P rel", _amax(P - P0) / _amax(P0),
          "O", _amax(O - O0))
    assert it == it0 == ref["iters"][0]
    assert [int(t["trials"]) for t in tr] == [int(t["trials"]) for t in tr0] == [int(t["trials"]) for t in ref["trace"]]
    assert abs(chi - chi0) <= 1e-9 * chi0
    assert _amax(T[:-1] - T0) <= 1e-9 and _amax(P - P0) <= 1e-9 * _amax(P0)
    assert _amax(O - O0) <= 1e-9 * max(_amax(O0), 1.0)
    np.testing.assert_array_equal(T[-1], g.kf_Tcw[-1])
    np.testing.assert_array_equal(ref["kf_Tcw"][-1], g.kf_Tcw[-1])
    if "bcr_fused" in c.stats:
        st = s.structure_stats()
        assert st["bcr_fallbacks"] == 0 and st["bcr_rows"] > 0, st
