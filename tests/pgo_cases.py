"""TEST INFRASTRUCTURE: small deterministic pose graphs that reach the branches of the pose-graph
kernels (csrc/plba_pgo.hpp) and of its host-built structure (csrc/plba_pgo_driver.hpp) that
plba.pgo.loop_graph cannot, shared by tests/test_pgo_cases_oracle.py (what the cases cover, and
that the CPU oracle is right on them) and tests/test_gpu_pgo_cases.py (the device on them), with
the oracle's results computed once for both.

Rotation cases ("rot_*"): 16 vertices, a chain plus skip edges, vertex 0 fixed, run with
initial_guess = 0 so the estimates written here are the linearisation point. Every edge is built
for a branch of Eigen's matrix -> quaternion (pgo::quat_from_R) in each of the three matrices the
kernel converts: Zinv.R, B.R = (Xi⁻¹Xj).R and the error rotation D.R = (Zinv·Xi⁻¹·Xj).R. The arms
other than trace > 0 come from rotations of 130°-175° about an axis near x, y or z, or near the
diagonal leaning to one of them, of either sign (the sign of the axis decides the sign of the raw
quaternion's w). The "hard" graphs put such a rotation into D itself, so estimate and measurement
disagree by more than 120° on most edges, and their first accepted step is so long that one vertex
gets a compact quaternion with |v| > 1 (fromVectorMQT's identity arm: rotation_kept_translation_moved);
the "mild" graphs keep Zinv and B but make D a rotation of about a degree, so their full trajectory
converges. Every branch decision keeps a margin of BRANCH_MARGIN; the generator asks for ten
times that.

Shape cases: chains with loop edges (unless named otherwise) of moderate relative rotations whose
estimates are the truth perturbed, so Levenberg converges in a few iterations.

One-iteration runs: max_iters = 1, max_trials = 1 at user_lambda_init 1e-10 and 0.0 (the τ path).
The oracle accepts that one trial on every case but at_rest (tests/test_pgo_cases_oracle.py asserts
it), so the step computed from the Jacobians of these branches reaches v_T; a rejected trial would
leave only λ·2 to compare.

Tolerances are the project's (tests/test_gpu_pgo.py): χ² initial 1e-12 relative, χ² of an iteration
1e-9, poses 1e-7 of the largest entry. Measured on the CPU, oracle against oracle with the free
vertices' ids permuted (another summation order of H and another elimination order), the largest
differences over all cases here were: one iteration χ²_end 5.1e-14 relative (sized_6), λ_end 2.8e-14
relative (sized_6), v_T 3.0e-14 of the largest entry (rot_hard_id); full run v_T 6.6e-10 of the
largest entry (isolated), and on the hard rotation graphs 1.3e-14 over all 100 iterations with the
same trials throughout: their trajectory does not converge but is not chaotic either, so it is
compared in full like the others. The project's bars are at least 150 times these figures and none
was widened."""
from __future__ import annotations

import functools

import numpy as np

import oracle_api as oa
from plba import capi, pgo
from plba.pgo import inv4, rot, to4, to12

ARMS = ("trace>0", "i=0", "i=1", "i=2")
BRANCH_MARGIN = 1e-3
CHI2_INITIAL_RTOL = 1e-12
CHI2_END_RTOL = 1e-9
POSE_TOL = 1e-7
LAMBDA_RTOL = 1e-9  # λ_end = λ·max(1/3, 1 - (2ρ - 1)³): ρ inherits χ²_end's 1e-9 (measured: 2.8e-14)


def _T(R, t):
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = t
    return M


def _unit(v):
    return np.asarray(v, float) / np.linalg.norm(v)


def arm(R):
    """(arm of quat_from_R, margin of the comparisons that chose it): 0 trace > 0, 1 + i otherwise."""
    R = np.asarray(R, float).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        return 0, tr
    i, m = 0, abs(R[1, 1] - R[0, 0])
    if R[1, 1] > R[0, 0]:
        i = 1
    m = min(m, abs(R[2, 2] - R[i, i]))
    if R[2, 2] > R[i, i]:
        i = 2
    return 1 + i, min(-tr, m)


def edge_branches(pg):
    """Per active edge, at the stored estimates: arm and margin of Zinv.R, B.R and D.R, the raw
    (un-normalised) quaternion's w of D, and the Ji rotation block's sign expression qa·qb."""
    out = []
    for e, (i, j) in enumerate(pg.e_v):
        if pg.v_fixed[i] and pg.v_fixed[j]:
            continue
        Zinv = inv4(to4(pg.e_Z[e]))
        Xii = inv4(to4(pg.v_T[i]))
        B = Xii @ to4(pg.v_T[j])
        D = (Zinv @ Xii) @ to4(pg.v_T[j])
        qa, qb = oa.quat_from_R(Zinv[:3, :3]), oa.quat_from_R(B[:3, :3])  # x y z w
        out.append(dict(edge=e, Zinv=arm(Zinv[:3, :3]), B=arm(B[:3, :3]), D=arm(D[:3, :3]),
                        w=oa.quat_from_R(D[:3, :3])[3], sgn=qa[3] * qb[3] - qa[:3] @ qb[:3]))
    return out


def _sample_R(rng, a):
    """A rotation that quat_from_R converts in arm a."""
    if a == 0:
        return rot(_unit(rng.normal(size=3)) * np.deg2rad(rng.uniform(20, 100)))
    ax = np.zeros(3)
    ax[a - 1] = 1.0
    if rng.random() < 0.5:
        ax = ax + rng.normal(0, 0.15, 3)                         # near x, y or z
    else:
        ax = np.ones(3) + 0.4 * ax + rng.normal(0, 0.04, 3)       # near the diagonal
    return rot(_unit(ax) * rng.choice([-1.0, 1.0]) * np.deg2rad(rng.uniform(130, 175)))


def _spd_info(rng, m):
    info = np.zeros((m, 36))
    for e in range(m):
        A = rng.normal(0, 0.3, (6, 6))
        info[e] = (np.eye(6) + A @ A.T).reshape(36)
    return info


@functools.lru_cache(maxsize=None)
def _rotation_graph(seed, info, mild):
    rng = np.random.default_rng(seed)
    n = 16
    pairs = [(k, k + 1) for k in range(n - 1)] + [(k, k + 2) for k in range(0, n - 2, 2)] + \
            [(k, k + 5) for k in range(0, n - 5, 3)]
    gm = 10 * BRANCH_MARGIN
    while True:  # the chain edges' B by construction; the skip edges' B as they come, with the margin
        X = [_T(rot(rng.normal(0, 1.5, 3)), rng.normal(0, 2, 3))]
        for k in range(n - 1):
            X.append(X[-1] @ _T(_sample_R(rng, k % 4), rng.normal(0, 1, 3)))
        if all(arm((inv4(X[i]) @ X[j])[:3, :3])[1] >= gm for i, j in pairs):
            break
    ez = []
    for e, (i, j) in enumerate(pairs):
        B = inv4(X[i]) @ X[j]
        aZ, aD = (e + e // 4) % 4, (e // 2) % 4
        for attempt in range(4000):
            if mild:
                DR = rot(rng.normal(0, 0.02, 3))
            else:
                DR = _sample_R(rng, aD)
            Zinv = _T(DR, rng.normal(0, 0.05 if mild else 0.3, 3)) @ inv4(B)
            D = Zinv @ B
            az, mz = arm(Zinv[:3, :3])
            ad, md = arm(D[:3, :3])
            qa, qb = oa.quat_from_R(Zinv[:3, :3]), oa.quat_from_R(B[:3, :3])
            ok = mz >= gm and md >= gm and arm(B[:3, :3])[1] >= gm
            ok = ok and abs(oa.quat_from_R(D[:3, :3])[3]) >= gm and abs(qa[3] * qb[3] - qa[:3] @ qb[:3]) >= gm
            if ok and (mild or az == aZ or attempt >= 2000):
                break
        else:
            raise AssertionError(f"no measurement for edge {e}")
        ez.append(to12(inv4(Zinv)))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return pgo.PoseGraph(np.arange(n, dtype=np.int32), np.array([to12(M) for M in X]), fixed,
                         np.array(pairs, np.int32), np.array(ez), _spd_info(rng, len(pairs)) if info else None)


def _chain(n, seed, loops=(), fixed=(0,), info=False, step_rot=0.3):
    """n vertices on a random walk (the truth), edges k -> k+1 and `loops`, measurements the true
    relative poses with a little noise, estimates the truth perturbed."""
    rng = np.random.default_rng(seed)
    Tt = [_T(rot(rng.normal(0, 0.5, 3)), rng.normal(0, 2, 3))]
    for _ in range(n - 1):
        Tt.append(Tt[-1] @ _T(rot(rng.normal(0, step_rot, 3)), rng.normal(0, 0.5, 3)))
    Te = [M @ _T(rot(rng.normal(0, 0.03, 3)), rng.normal(0, 0.05, 3)) for M in Tt]
    pairs = [(k, k + 1) for k in range(n - 1)] + list(loops)
    ez = [to12(inv4(Tt[i]) @ Tt[j] @ _T(rot(rng.normal(0, 0.01, 3)), rng.normal(0, 0.02, 3))) for i, j in pairs]
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    return pgo.PoseGraph(np.arange(n, dtype=np.int32), np.array([to12(M) for M in Te]), fx,
                         np.array(pairs, np.int32).reshape(-1, 2), np.array(ez).reshape(-1, 12),
                         _spd_info(rng, len(pairs)) if info else None, np.array([to12(M) for M in Tt]))


def reposition(pg, perm):
    """The same vertices (ids, estimates, fixed flags) and edge list, vertex perm[p] stored at
    position p."""
    perm = np.asarray(perm)
    where = np.empty(len(perm), np.int32)
    where[perm] = np.arange(len(perm), dtype=np.int32)
    return pgo.PoseGraph(pg.v_id[perm].copy(), pg.v_T[perm].copy(), pg.v_fixed[perm].copy(),
                         where[pg.e_v].astype(np.int32), pg.e_Z.copy(),
                         None if pg.e_info is None else pg.e_info.copy())


def reverse_edge(pg, e):
    pg.e_v[e] = pg.e_v[e][::-1].copy()
    pg.e_Z[e] = to12(inv4(to4(pg.e_Z[e])))


def scrambled_ids(order_seed=1):
    """12 vertices whose ids 3k + 5 are dealt out by one permutation and whose arrays are stored in
    another (order_seed): neither ids nor Hessian indices are monotone in position."""
    pg = _chain(12, seed=31, loops=[(0, 11), (2, 8)], fixed=(3,))
    pg.v_id = (3 * np.random.default_rng(7).permutation(12) + 5).astype(np.int32)
    return reposition(pg, np.random.default_rng(order_seed).permutation(12))


def reversed_edges():
    pg = _chain(12, seed=32, loops=[(11, 0), (3, 9)], fixed=(0,))
    for e in range(0, len(pg.e_v), 2):
        reverse_edge(pg, e)
    return pg


MULTI_PAIRS = ((1, 2), (4, 5), (2, 7))


def multi_edges():
    """For each pair of MULTI_PAIRS two more parallel edges and one antiparallel edge, each with its
    own measurement and information, appended to a chain with a loop."""
    pg = _chain(10, seed=33, loops=[(0, 9), (2, 7)], fixed=(0,), info=True)
    rng = np.random.default_rng(34)
    T = [to4(t) for t in pg.T_true]
    ev, ez = list(map(tuple, pg.e_v)), list(pg.e_Z)
    for i, j in MULTI_PAIRS:
        for a, b in ((i, j), (i, j), (j, i)):
            ev.append((a, b))
            ez.append(to12(inv4(T[a]) @ T[b] @ _T(rot(rng.normal(0, 0.02, 3)), rng.normal(0, 0.03, 3))))
    pg.e_v, pg.e_Z = np.array(ev, np.int32), np.array(ez)
    pg.e_info = _spd_info(rng, len(ev))
    return pg


ISOLATED_FREE, ISOLATED_FIXED, FIXED_PAIR = 10, 11, (0, 5)


def isolated():
    """Vertex 10 free without an edge, vertex 11 fixed without an edge, and the edge 0 - 5 between
    two fixed vertices in the middle of the edge list."""
    pg = _chain(10, seed=35, loops=[(1, 8)], fixed=FIXED_PAIR)
    rng = np.random.default_rng(36)
    extra = np.array([to12(_T(rot(rng.normal(0, 1, 3)), rng.normal(0, 2, 3))) for _ in range(2)])
    pg.v_id = np.arange(12, dtype=np.int32)
    pg.v_T = np.vstack([pg.v_T, extra])
    pg.v_fixed = np.concatenate([pg.v_fixed, np.array([0, 1], np.uint8)])
    T = [to4(t) for t in pg.T_true]
    mid = len(pg.e_v) // 2
    pg.e_v = np.insert(pg.e_v, mid, FIXED_PAIR, axis=0).astype(np.int32)
    pg.e_Z = np.insert(pg.e_Z, mid, to12(inv4(T[0]) @ T[5] @ _T(rot([0.2, 0, 0]), [0.5, 0, 0])), axis=0)
    pg.T_true = None
    return pg


def fixed_inside():
    """Vertices 4 and 7 of 12 fixed, vertex 0 free: each is vertex(1) of the chain edge that reaches
    it and vertex(0) of the one that leaves it."""
    return _chain(12, seed=37, loops=[(0, 11), (7, 2)], fixed=(4, 7))


def star():
    """Hub 0 (free) with 15 spokes, alternately hub -> rim and rim -> hub, four rim edges, rim
    vertex 9 fixed."""
    rng = np.random.default_rng(38)
    n = 16
    Tt = [_T(rot(rng.normal(0, 0.6, 3)), rng.normal(0, 2, 3)) for _ in range(n)]
    Te = [M @ _T(rot(rng.normal(0, 0.03, 3)), rng.normal(0, 0.05, 3)) for M in Tt]
    pairs = [(0, k) if k % 2 else (k, 0) for k in range(1, n)] + [(1, 2), (5, 12), (14, 3), (8, 9)]
    ez = [to12(inv4(Tt[i]) @ Tt[j] @ _T(rot(rng.normal(0, 0.01, 3)), rng.normal(0, 0.02, 3))) for i, j in pairs]
    fx = np.zeros(n, np.uint8)
    fx[9] = 1
    return pgo.PoseGraph(np.arange(n, dtype=np.int32), np.array([to12(M) for M in Te]), fx,
                         np.array(pairs, np.int32), np.array(ez))


def none_free(which):
    if which == "no_vertices":
        return pgo.PoseGraph(np.zeros(0, np.int32), np.zeros((0, 12)), np.zeros(0, np.uint8),
                             np.zeros((0, 2), np.int32), np.zeros((0, 12)))
    pg = _chain(5, seed=39, loops=[(0, 4)])
    if which == "no_edges":
        pg.e_v, pg.e_Z = np.zeros((0, 2), np.int32), np.zeros((0, 12))
    else:
        assert which == "all_fixed"
        pg.v_fixed[:] = 1
    return pg


def at_rest():
    n = 6
    I = to12(np.eye(4))
    fx = np.zeros(n, np.uint8)
    fx[2] = 1
    pairs = [(k, k + 1) for k in range(n - 1)] + [(0, 5)]
    return pgo.PoseGraph(np.arange(n, dtype=np.int32), np.tile(I, (n, 1)), fx, np.array(pairs, np.int32),
                         np.tile(I, (len(pairs), 1)))


SIZED = (1, 5, 6, 16, 17)  # n = 6·nfree = 6, 30, 36, 96, 102 against the 32-wide tile


def sized(nfree):
    """Vertex 0 fixed and nfree free ones on a chain, one loop edge from vertex 1 to the last (for
    one free vertex: a second, different edge 0 -> 1)."""
    return _chain(nfree + 1, seed=40 + nfree, loops=[(1, nfree)] if nfree > 1 else [(0, 1)])


# name -> (graph, keyword arguments of capi.pgo_params)
CASES = {
    "rot_hard_id": (lambda: _rotation_graph(51, False, False), dict(initial_guess=0)),
    "rot_hard_info": (lambda: _rotation_graph(52, True, False), dict(initial_guess=0)),
    "rot_mild_id": (lambda: _rotation_graph(51, False, True), dict(initial_guess=0)),
    "rot_mild_info": (lambda: _rotation_graph(52, True, True), dict(initial_guess=0)),
    "scrambled_ids": (scrambled_ids, dict(initial_guess=0)),
    "scrambled_ids_guess": (scrambled_ids, dict()),
    "reversed_edges": (reversed_edges, dict(initial_guess=0)),
    "reversed_edges_guess": (reversed_edges, dict()),
    "multi_edges": (multi_edges, dict()),
    "isolated": (isolated, dict()),
    "fixed_inside": (fixed_inside, dict()),
    "star": (star, dict()),
    "no_vertices": (lambda: none_free("no_vertices"), dict()),
    "no_edges": (lambda: none_free("no_edges"), dict()),
    "all_fixed": (lambda: none_free("all_fixed"), dict()),
    "at_rest": (at_rest, dict()),
    **{f"sized_{k}": (functools.partial(sized, k), dict()) for k in SIZED},
}
ROTATION_HARD = ("rot_hard_id", "rot_hard_info")
ROTATION = ROTATION_HARD + ("rot_mild_id", "rot_mild_info")
NONE_FREE = ("no_vertices", "no_edges", "all_fixed")
PATH_SWITCH = ("star",) + tuple(f"sized_{k}" for k in SIZED)
# The full trajectory through tests/test_gpu_pgo.py's comparison: every case with a free vertex
# except at_rest (exact expectations instead)
FULL_RUN = tuple(k for k in CASES if k not in NONE_FREE + ("at_rest",))
ONE_ITER = tuple(k for k in CASES if k not in NONE_FREE)
ONE_ITER_LAMBDAS = (1e-10, 0.0)  # setUserLambdaInit, and the τ path


def graph(name):
    """A fresh copy of the case's graph (callers may modify it)."""
    return CASES[name][0]().copy()


def params(name, **kw):
    return capi.pgo_params(**{**CASES[name][1], **kw})


@functools.lru_cache(maxsize=None)
def oracle(name, depth, lam=None):
    """The CPU oracle on a case (shared: do not modify). depth: "chi2" (max_iters = 0), "one"
    (max_iters = 1, max_trials = 1, user_lambda_init = lam) or "full"."""
    kw = {"chi2": dict(max_iters=0), "one": dict(max_iters=1, max_trials=1, user_lambda_init=lam), "full": {}}[depth]
    return oa.pgo_optimize(graph(name), params(name, **kw))


def rotation_kept_translation_moved(pg, v_T):
    """Vertices whose rotation block came back bitwise while the translation moved: an accepted
    step whose compact quaternion had |v| > 1, fromVectorMQT's identity arm (the one-iteration
    step of the hard rotation graphs has one such vertex)."""
    a, b = np.asarray(v_T).reshape(-1, 3, 4), pg.v_T.reshape(-1, 3, 4)
    return [v for v in range(len(a)) if np.array_equal(a[v, :, :3], b[v, :, :3]) and not np.array_equal(a[v, :, 3], b[v, :, 3])]


def compare_one_iteration(out, ref):
    """Device against oracle after max_iters = 1, max_trials = 1."""
    assert out["n_free"] == ref["n_free"] and out["solve_fails"] == ref["solve_fails"]
    assert out["iterations"] == ref["iterations"] == 1 and out["trials"] == ref["trials"]
    t, r = out["trace"][0], ref["trace"][0]
    assert (t["trials"], t["result"]) == (r["trials"], r["result"]), (t, r)
    np.testing.assert_allclose(t["chi2_start"], r["chi2_start"], rtol=CHI2_INITIAL_RTOL)
    np.testing.assert_allclose(t["chi2_end"], r["chi2_end"], rtol=CHI2_END_RTOL)
    np.testing.assert_allclose(t["lambda_start"], r["lambda_start"], rtol=CHI2_INITIAL_RTOL)
    np.testing.assert_allclose(t["lambda_end"], r["lambda_end"], rtol=LAMBDA_RTOL)
    scale = max(np.abs(ref["v_T"]).max(), 1.0)
    assert np.abs(out["v_T"] - ref["v_T"]).max() <= POSE_TOL * scale
