"""The pose-graph kernels (csrc/plba_pgo.hpp) and their host-built structure
(csrc/plba_pgo_driver.hpp) on the graphs of tests/pgo_cases.py against the CPU oracle
(oracle/refpgo.cpp): large relative and error rotations in every arm of the matrix -> quaternion
conversion, ids that are not positions, reversed / duplicate / antiparallel edges, isolated and
inner fixed vertices, a star, no free vertex at all, a graph at rest, and n = 6·nfree around the
32-wide tile. tests/test_pgo_cases_oracle.py shows on the CPU that the cases reach what they are
named for and that the oracle's Jacobians are right there. Each case is compared at three depths:
χ² at the uploaded state (k_pgo_linearize<false> alone), one iteration of one trial (the
linearisation at exactly that state, through assembly, solve and update), and the full run.
The bars are the project's (tests/test_gpu_pgo.py), see pgo_cases.py."""
import numpy as np
import pytest

import oracle_api as oa
import pgo_cases as pc
from test_gpu_pgo import _compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from plba.lib import Solver
    s = Solver()
    yield s
    s.close()


def _untouched(pg):
    """Vertices no step may move: fixed ones and free ones without an active edge."""
    moved = np.zeros(len(pg.v_id), bool)
    for i, j in pg.e_v:
        if not (pg.v_fixed[i] and pg.v_fixed[j]):
            moved[[i, j]] = True
    return ~moved | pg.v_fixed.astype(bool)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_initial_chi2(solver, name):
    ref = pc.oracle(name, "chi2")
    out = solver.pgo_optimize(pc.graph(name), pc.params(name, max_iters=0))
    assert out["n_free"] == ref["n_free"] and out["iterations"] == 0
    assert abs(out["chi2_initial"] - ref["chi2_initial"]) <= pc.CHI2_INITIAL_RTOL * ref["chi2_initial"]


@pytest.mark.parametrize("lam", pc.ONE_ITER_LAMBDAS)
@pytest.mark.parametrize("name", pc.ONE_ITER)
def test_one_iteration(solver, name, lam):
    pg = pc.graph(name)
    out = solver.pgo_optimize(pg, pc.params(name, max_iters=1, max_trials=1, user_lambda_init=lam))
    ref = pc.oracle(name, "one", lam)
    pc.compare_one_iteration(out, ref)
    keep = _untouched(pg)
    np.testing.assert_array_equal(out["v_T"][keep], pg.v_T[keep])
    # pgo::from_mqt's |v| > 1 arm: the same vertices keep their rotation bitwise as in the oracle
    assert pc.rotation_kept_translation_moved(pg, out["v_T"]) == pc.rotation_kept_translation_moved(pg, ref["v_T"])


@pytest.mark.parametrize("name", pc.FULL_RUN)
def test_full_run(solver, name):
    pg = pc.graph(name)
    out = solver.pgo_optimize(pg, pc.params(name))
    _compare(out, pc.oracle(name, "full"), pose_tol=pc.POSE_TOL)
    keep = _untouched(pg)
    assert keep.any()
    np.testing.assert_array_equal(out["v_T"][keep], pg.v_T[keep])


def test_isolated_vertices_come_back_bitwise(solver):
    pg = pc.graph("isolated")
    out = solver.pgo_optimize(pg, pc.params("isolated"))
    for v in (pc.ISOLATED_FREE, pc.ISOLATED_FIXED) + pc.FIXED_PAIR:
        np.testing.assert_array_equal(out["v_T"][v], pg.v_T[v])
    assert out["n_free"] == 8


@pytest.mark.parametrize("name", pc.NONE_FREE)
def test_none_free_returns_the_input(solver, name):
    pg = pc.graph(name)
    out = solver.pgo_optimize(pg, pc.params(name))
    assert out["n_free"] == 0 and out["iterations"] == 0 and out["trials"] == 0 and len(out["trace"]) == 0
    assert out["chi2_final"] == out["chi2_initial"] == 0.0
    np.testing.assert_array_equal(out["v_T"], pg.v_T.reshape(-1, 12))
    # the context is left clean: the next graph on it runs and matches
    nxt = solver.pgo_optimize(pc.graph("sized_5"), pc.params("sized_5"))
    _compare(nxt, pc.oracle("sized_5", "full"))


def test_at_rest_ends_after_one_trial(solver):
    pg = pc.graph("at_rest")
    out = solver.pgo_optimize(pg, pc.params("at_rest"))
    assert (out["iterations"], out["trials"], out["solve_fails"]) == (1, 1, 0)
    assert out["trace"]["result"][0] == 1 and out["chi2_initial"] == 0.0 and out["chi2_final"] == 0.0
    np.testing.assert_array_equal(out["v_T"], pg.v_T)


@pytest.mark.parametrize("name", pc.PATH_SWITCH)
def test_id_order_and_global_memory_solve(solver, monkeypatch, name):
    """PLBA_NO_RCM=1 keeps g2o's id order (another envelope, same oracle agreement);
    PLBA_SOLVE_LDS_N=0 substitutes with y in global memory, bitwise the default path."""
    ref = pc.oracle(name, "full")
    default = solver.pgo_optimize(pc.graph(name), pc.params(name))
    monkeypatch.setenv("PLBA_SOLVE_LDS_N", "0")
    gmem = solver.pgo_optimize(pc.graph(name), pc.params(name))
    np.testing.assert_array_equal(gmem["v_T"], default["v_T"])
    assert gmem["trials"] == default["trials"] and gmem["chi2_final"] == default["chi2_final"]
    monkeypatch.delenv("PLBA_SOLVE_LDS_N")
    monkeypatch.setenv("PLBA_NO_RCM", "1")
    _compare(solver.pgo_optimize(pc.graph(name), pc.params(name)), ref)
    for lam in pc.ONE_ITER_LAMBDAS:
        one = solver.pgo_optimize(pc.graph(name), pc.params(name, max_iters=1, max_trials=1, user_lambda_init=lam))
        pc.compare_one_iteration(one, pc.oracle(name, "one", lam))


def test_position_order_does_not_matter(solver):
    """The same vertices (ids, estimates) and edge list stored in another position order: the
    Hessian index follows the ids and the sums follow the edge list, so every pose comes back
    bitwise the same, id by id (the oracle has the same property: test_pgo_cases_oracle.py)."""
    a, b = pc.scrambled_ids(order_seed=1), pc.scrambled_ids(order_seed=2)
    assert not np.array_equal(a.v_id, b.v_id) and sorted(a.v_id) == sorted(b.v_id)
    p = pc.params("scrambled_ids")
    ra, rb = solver.pgo_optimize(a, p), solver.pgo_optimize(b, p)
    np.testing.assert_array_equal(ra["v_T"][np.argsort(a.v_id)], rb["v_T"][np.argsort(b.v_id)])
    assert ra["trials"] == rb["trials"] and ra["chi2_final"] == rb["chi2_final"]


def test_lambda_init_ignores_the_window_solvers_tau():
    """λ₀ = τ·max|H_ii| with g2o's default τ = 1e-5 (the reference makes a fresh
    OptimizationAlgorithmLevenberg per pose graph; include/plba.h), whatever plba_opts::tau the
    context was created with for its window solves."""
    from plba.lib import Solver
    with Solver(tau=1e-3) as s:
        one = s.pgo_optimize(pc.graph("sized_5"), pc.params("sized_5", max_iters=1, max_trials=1, user_lambda_init=0.0))
        pc.compare_one_iteration(one, pc.oracle("sized_5", "one", 0.0))
        p = pc.params("fixed_inside", user_lambda_init=0.0)
        _compare(s.pgo_optimize(pc.graph("fixed_inside"), p), oa.pgo_optimize(pc.graph("fixed_inside"), p))
