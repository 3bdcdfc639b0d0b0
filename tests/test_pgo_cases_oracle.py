"""What the pose graphs of tests/pgo_cases.py reach, shown on the CPU: the branch counts of the
rotation cases with their margins, the structural property each shape case is named for, and that
the oracle (oracle/refpgo.cpp) is right on these inputs — its EdgeSE3 Jacobians against central
differences on every edge of the rotation cases (tests/test_pgo_oracle.py's method and bars, which
stops at about 150° and aims at no particular arm). tests/test_gpu_pgo_cases.py then compares the
device with the oracle on the same graphs."""
import collections

import numpy as np
import pytest

import oracle_api as oa
import pgo_cases as pc
from plba.pgo import inv4, to4, to12


def _structure(pg):
    """The host-side structure plba_pgo_optimize derives (pgo_active_set / pgo_block_pattern):
    active edges, Hessian index in id order, contributions (edge, kind) of every lower block."""
    act = [e for e, (i, j) in enumerate(pg.e_v) if not (pg.v_fixed[i] and pg.v_fixed[j])]
    used = np.zeros(len(pg.v_id), bool)
    for e in act:
        used[pg.e_v[e]] = True
    hidx = np.full(len(pg.v_id), -1)
    k = 0
    for v in np.argsort(pg.v_id, kind="stable"):
        if used[v] and not pg.v_fixed[v]:
            hidx[v] = k
            k += 1
    blocks = collections.defaultdict(list)
    for e in act:
        hi, hj = hidx[pg.e_v[e]]
        if hi >= 0:
            blocks[hi, hi].append((e, 0))
        if hj >= 0:
            blocks[hj, hj].append((e, 1))
        if hi >= 0 and hj >= 0:
            blocks[(hi, hj) if hi > hj else (hj, hi)].append((e, 2 if hi > hj else 3))
    return act, hidx, blocks


# ---- rotation cases: branch coverage with margins
@pytest.mark.parametrize("name", pc.ROTATION)
def test_rotation_case_reaches_every_arm(name):
    br = pc.edge_branches(pc.graph(name))
    hard = name in pc.ROTATION_HARD
    for key, least in (("Zinv", 3), ("B", 3)) + ((("D", 2),) if hard else ()):
        count = collections.Counter(b[key][0] for b in br)
        assert all(count[a] >= least for a in range(4)), (key, count)
    for b in br:
        assert min(b["Zinv"][1], b["B"][1], b["D"][1]) >= pc.BRANCH_MARGIN, b
        assert abs(b["w"]) >= pc.BRANCH_MARGIN and abs(b["sgn"]) >= pc.BRANCH_MARGIN, b
    assert sum(b["sgn"] < 0 for b in br) >= 3 and sum(b["sgn"] > 0 for b in br) >= 3
    if hard:  # qnormalize's flip through D, and error rotations above 120° outside the trace arm
        assert sum(b["w"] < 0 for b in br) >= 2
    else:
        assert all(b["D"][0] == 0 for b in br)
    print(name, {k: [collections.Counter(b[k][0] for b in br)[a] for a in range(4)] for k in ("Zinv", "B", "D")},
          "w<0", sum(b["w"] < 0 for b in br), "sgn-", sum(b["sgn"] < 0 for b in br))


def test_rotation_case_information():
    assert pc.graph("rot_hard_id").e_info is None
    for name in ("rot_hard_info", "rot_mild_info"):
        for O in pc.graph(name).e_info.reshape(-1, 6, 6):
            assert np.allclose(O, O.T) and np.linalg.eigvalsh(O).min() > 0.5
            assert np.abs(O - np.diag(np.diag(O))).max() > 0.05


@pytest.mark.parametrize("name", pc.ROTATION)
def test_rotation_case_jacobians_central_differences(name):
    pg = pc.graph(name)
    h = 1e-6
    for e, (i, j) in enumerate(pg.e_v):
        Z, X = pg.e_Z[e], [pg.v_T[i], pg.v_T[j]]
        for J, which in zip(oa.se3_edge_jacobians(Z, *X), (0, 1)):
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                Xp, Xm = list(X), list(X)
                Xp[which] = oa.se3_oplus(X[which], d)
                Xm[which] = oa.se3_oplus(X[which], -d)
                num = (oa.se3_edge_error(Z, *Xp) - oa.se3_edge_error(Z, *Xm)) / (2 * h)
                np.testing.assert_allclose(J[:, k], num, atol=2e-8, rtol=1e-6, err_msg=f"edge {e} side {which}")


@pytest.mark.parametrize("name", pc.ONE_ITER)
def test_first_trial_is_accepted(name):
    """The one-iteration comparison sees the step: the oracle accepts the single trial (at_rest:
    ρ == 0, nothing moves)."""
    for lam in pc.ONE_ITER_LAMBDAS:
        r = pc.oracle(name, "one", lam)
        t = r["trace"][0]
        assert r["solve_fails"] == 0 and t["trials"] == 1
        if name == "at_rest":
            assert t["chi2_start"] == 0.0 and t["chi2_end"] == 0.0 and t["result"] == 1
        else:
            assert t["chi2_end"] < t["chi2_start"]
            assert np.abs(r["v_T"] - pc.graph(name).v_T).max() > 1e-4


@pytest.mark.parametrize("name", pc.ROTATION_HARD)
def test_hard_rotation_step_takes_the_identity_arm_of_from_mqt(name):
    pg = pc.graph(name)
    for lam in pc.ONE_ITER_LAMBDAS:
        hit = pc.rotation_kept_translation_moved(pg, pc.oracle(name, "one", lam)["v_T"])
        assert len(hit) >= 1 and not pg.v_fixed[hit].any()


# ---- shape cases: each has the property it is named for
def test_scrambled_ids_are_not_positions():
    for seed in (1, 2):
        pg = pc.scrambled_ids(seed)
        _, hidx, _ = _structure(pg)
        free = hidx >= 0
        assert set(pg.v_id) == {3 * k + 5 for k in range(12)}
        assert np.any(np.diff(pg.v_id) < 0) and np.any(np.diff(pg.v_id) > 0)
        assert not np.array_equal(hidx[free], np.arange(free.sum()))          # Hessian order != position order
        assert np.any(pg.e_v[:, 0] > pg.e_v[:, 1]) and np.any(pg.e_v[:, 0] < pg.e_v[:, 1])


def test_position_order_does_not_matter_to_the_oracle():
    a, b = pc.scrambled_ids(1), pc.scrambled_ids(2)
    p = pc.params("scrambled_ids")
    ra, rb = oa.pgo_optimize(a, p), oa.pgo_optimize(b, p)
    np.testing.assert_array_equal(ra["v_T"][np.argsort(a.v_id)], rb["v_T"][np.argsort(b.v_id)])
    assert ra["chi2_final"] == rb["chi2_final"] and ra["trials"] == rb["trials"]


def test_reversed_edges_use_both_kinds_and_both_propagation_arms():
    pg = pc.graph("reversed_edges")
    _, hidx, blocks = _structure(pg)
    kinds = collections.Counter(k for (r, c), con in blocks.items() if r != c for _, k in con)
    assert kinds[2] >= 4 and kinds[3] >= 4, kinds
    assert np.sum(pg.e_v[:, 0] > pg.e_v[:, 1]) >= len(pg.e_v) // 2 - 1
    # computeInitialGuess reaches vertices through vertex(0) of some edges and vertex(1) of others:
    # with exact measurements the chain comes back whichever way the edges point
    exact = pc.graph("reversed_edges")
    T = [to4(t) for t in exact.T_true]
    exact.e_Z = np.array([to12(inv4(T[i]) @ T[j]) for i, j in exact.e_v])
    exact.v_T[0] = exact.T_true[0]
    np.testing.assert_allclose(oa.pgo_initial_guess(exact), exact.T_true, atol=1e-10)
    moved = oa.pgo_initial_guess(pg)
    assert np.abs(moved - pg.v_T).max() > 1e-3


def test_multi_edges_stack_on_one_block():
    pg = pc.graph("multi_edges")
    _, hidx, blocks = _structure(pg)
    for i, j in pc.MULTI_PAIRS:
        con = blocks[max(hidx[i], hidx[j]), min(hidx[i], hidx[j])]
        assert len(con) >= 3 and {k for _, k in con} == {2, 3}, con
        zs = [pg.e_Z[e] for e, _ in con]
        assert all(not np.allclose(zs[0], z) for z in zs[1:])


def test_isolated_vertices_and_the_inactive_edge():
    pg = pc.graph("isolated")
    act, hidx, _ = _structure(pg)
    assert hidx[pc.ISOLATED_FREE] == -1 and not pg.v_fixed[pc.ISOLATED_FREE]
    assert hidx[pc.ISOLATED_FIXED] == -1 and pg.v_fixed[pc.ISOLATED_FIXED]
    assert not np.any(pg.e_v == pc.ISOLATED_FREE) and not np.any(pg.e_v == pc.ISOLATED_FIXED)
    dead = [e for e in range(len(pg.e_v)) if e not in act]
    assert len(dead) == 1 and tuple(pg.e_v[dead[0]]) == pc.FIXED_PAIR and 0 < dead[0] < len(pg.e_v) - 1
    assert act != list(range(len(act)))  # the active list skips an index
    assert pc.oracle("isolated", "chi2")["n_free"] == 8


def test_fixed_inside_sits_on_both_sides_of_edges():
    pg = pc.graph("fixed_inside")
    fx = np.where(pg.v_fixed)[0]
    assert not pg.v_fixed[0] and not pg.v_fixed[-1] and len(fx) == 2
    for v in fx:
        assert np.any(pg.e_v[:, 0] == v) and np.any(pg.e_v[:, 1] == v)
    _, hidx, _ = _structure(pg)
    assert hidx[fx[0] - 1] + 1 == hidx[fx[0] + 1]  # the Hessian index skips the fixed vertex


def test_star_hub_collects_every_spoke():
    pg = pc.graph("star")
    _, hidx, blocks = _structure(pg)
    hub = blocks[hidx[0], hidx[0]]
    assert len(hub) == 15 and {k for _, k in hub} == {0, 1}
    assert len(pg.e_v) == 19 and hidx[0] == 0 and pc.oracle("star", "chi2")["n_free"] == 15


def test_none_free_graphs():
    for name in pc.NONE_FREE:
        pg = pc.graph(name)
        r = pc.oracle(name, "full")
        assert r["n_free"] == 0 and r["iterations"] == 0 and r["chi2_initial"] == 0.0 == r["chi2_final"]
        np.testing.assert_array_equal(r["v_T"], pg.v_T.reshape(-1, 12))
    assert len(pc.graph("no_vertices").v_id) == 0
    assert len(pc.graph("no_edges").e_v) == 0 and not pc.graph("no_edges").v_fixed.all()
    assert pc.graph("all_fixed").v_fixed.all() and len(pc.graph("all_fixed").e_v) > 0


def test_at_rest_is_a_rho_zero_termination():
    r = pc.oracle("at_rest", "full")
    assert (r["iterations"], r["trials"], r["chi2_initial"], r["chi2_final"]) == (1, 1, 0.0, 0.0)
    assert r["trace"]["result"][0] == 1
    np.testing.assert_array_equal(r["v_T"], pc.graph("at_rest").v_T)


@pytest.mark.parametrize("nfree", pc.SIZED)
def test_sized_cases_straddle_the_tile(nfree):
    pg = pc.graph(f"sized_{nfree}")
    _, hidx, blocks = _structure(pg)
    assert pc.oracle(f"sized_{nfree}", "chi2")["n_free"] == nfree == hidx.max() + 1
    n = 6 * nfree  # (tiles of 32, rows in the last tile)
    assert ((n + 31) // 32, n - 32 * ((n - 1) // 32)) == {1: (1, 6), 5: (1, 30), 6: (2, 4), 16: (3, 32), 17: (4, 6)}[nfree]
    if nfree > 2:  # the loop edge: a block far from the diagonal
        assert max(r - c for r, c in blocks) == nfree - 1
    else:
        assert len(blocks[0, 0]) == 2


def test_full_runs_converge_or_are_listed():
    for name in pc.FULL_RUN:
        r = pc.oracle(name, "full")
        assert r["solve_fails"] == 0 and r["chi2_final"] < r["chi2_initial"]
        if name not in pc.ROTATION_HARD:
            assert r["iterations"] < 20 and r["trace"]["result"][-1] == 1
