"""TEST INFRASTRUCTURE: the seeded candidates on which the three hand-rolled LM loops (plba_hlm_lba
variants 0, 1, 2) reject a step, stop on each of their tests, or clamp a residual row, shared by
tests/test_hlm_cases_oracle.py (the admission checks: flow, decision margins, clamp counts, all on
the CPU checkers) and tests/test_gpu_hlm_cases.py (the device on them), with the checker results
computed once for both.

The checkers: oracle/refhlm.cpp for variants 0 and 1, tests/ref_lba_endpoints.py for variant 2.
Every finite-error case sets err_per_obs = 1: the reference's own err is +inf (variants 0, 1) and
`inf > inf` never rejects.

A flow is written (trace results; linearisations, solves, applied steps). Result 0: solved, λ·k;
1: err > err_prev, λ/k, step not applied; 3: stopped on |err − err_prev| < min_error_change or
err < min_error before a solve."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import oracle_api as oa
import ref_lba_endpoints
from plba import capi, synth
from plba.hlm import HlmWindow, gba_window, hlm_window, lba_window

PLUCKER, GBA, ENDPOINTS = capi.HLM_LBA_PLUCKER, capi.HLM_GBA, capi.HLM_LBA_ENDPOINTS
_WINDOW = {PLUCKER: hlm_window, GBA: gba_window, ENDPOINTS: lba_window}
_PARAMS = {PLUCKER: capi.hlm_params, GBA: capi.gba_params, ENDPOINTS: capi.lba_params}
VARIANT_NAME = {PLUCKER: "plucker", GBA: "gba", ENDPOINTS: "endpoints"}


@functools.lru_cache(maxsize=None)
def _window(variant: int, cfg: str, gen: tuple) -> HlmWindow:
    return _WINDOW[variant](synth.generate(cfg, **dict(gen)))


def run_checker(variant: int, win: HlmWindow, p, dense: bool = False) -> dict:
    if variant == ENDPOINTS:
        return ref_lba_endpoints.lba(win, p, dense)
    return oa.hlm_lba(win, p, dense)


@dataclasses.dataclass(frozen=True)
class Case:
    """A named candidate: the variant, synth.generate's arguments, the parameters that differ from
    the variant's defaults, and the flow it is admitted for."""
    name: str
    variant: int
    cfg: str
    gen: tuple = ()                  # ((name, value), ...) of synth.generate
    prm: tuple = ()                  # ((name, value), ...) of PlbaHlmParams
    results: tuple = ()              # the trace's result column
    counters: tuple = ()             # (linearizations, solves, accepted)
    stop: str = ""                   # which test ended the run: "derr", "min_error", "dx", "max_iters"
    dense: bool = True               # the checker's dense solve counts as a reordering (small windows)
    family: str = ""                 # the factorisation family the window must take: "band", "column_lane", "bcr"

    @property
    def id(self) -> str:
        return f"{VARIANT_NAME[self.variant]}-{self.name}"

    def window(self) -> HlmWindow:
        return _window(self.variant, self.cfg, self.gen)

    def params(self, **kw):
        return _PARAMS[self.variant](**{**dict(self.prm), **kw})

    def reference(self) -> dict:
        """The checker's result (read-only: shared by the tests)."""
        return _reference(self, None)

    def prefix(self, n_iters: int) -> dict:
        """The checker stopped after n_iters iterations (max_iters = n_iters)."""
        return _reference(self, n_iters)

    def rejected_rows(self):
        return [i for i, r in enumerate(self.results) if r == 1]


@functools.lru_cache(maxsize=None)
def _reference(c: Case, n_iters):
    p = c.params() if n_iters is None else c.params(max_iters=n_iters)
    return run_checker(c.variant, c.window(), p)


# ---- the loop's decisions and their distance from the thresholds -------------------------------------

def history(run, n: int) -> list:
    """Per iteration 0..n-1: err of its linearisation and ‖DX‖ of its solve (None when the iteration
    stopped before solving). run(k) is the checker's result with max_iters = k: the loop's first k
    iterations are the same whatever the cap, and dx_norm is that of the last solve."""
    full = run(n)
    tr = full["trace"]
    out = []
    for it in range(len(tr)):
        solved = tr["result"][it] != 3
        o = full if it + 1 == len(tr) else run(it + 1)
        out.append(dict(err=float(tr["chi2_start"][it]), dx=float(o["dx_norm"]) if solved else None,
                        result=int(tr["result"][it])))
    return out


def decisions(hist: list, p) -> list:
    """Every comparison the loop made, as (iteration, name, decided quantity, threshold, outcome), in
    the loop's order. Comparisons on a non-finite err are left out: |inf − inf| < x and inf > inf are
    false whatever the rounding."""
    out = []
    for it in range(1, len(hist)):
        err, prev, dx = hist[it]["err"], hist[it - 1]["err"], hist[it]["dx"]
        if np.isfinite(err) and np.isfinite(prev):
            d = abs(err - prev)
            out.append((it, "derr", d, p.min_error_change, d < p.min_error_change))
        if np.isfinite(err):
            out.append((it, "min_error", err, p.min_error, err < p.min_error))
        if dx is None:
            break
        if np.isfinite(err) and np.isfinite(prev):
            out.append((it, "reject", err - prev, 0.0, err > prev))
        out.append((it, "dx", dx, p.min_error_change, dx < p.min_error_change))
    return out


def stop_of(ref: dict, p) -> str:
    """Which test ended a run, from the counters and the trace alone."""
    tr = ref["trace"]
    if tr["result"][-1] == 3:
        prev, err = tr["chi2_start"][-2], tr["chi2_start"][-1]
        small = abs(err - prev) < p.min_error_change
        low = err < p.min_error
        return "derr+min_error" if small and low else "derr" if small else "min_error"
    assert ref["linearizations"] == ref["solves"]
    if ref["dx_norm"] < p.min_error_change:
        return "dx+max_iters" if len(tr) == p.max_iters else "dx"
    assert len(tr) == p.max_iters
    return "max_iters"


# ---- the same problem in another order ----------------------------------------------------------------

def permuted(variant: int, win: HlmWindow, seed: int):
    """The window with its point landmarks and its edges reordered (and, for the Plücker variant, its
    lines); keyframes keep their places, and so do endpoint lines: variants 1 and 2 read line j's
    endpoints at the aliased offset 3·j, so their order is part of the problem. Also returns the point
    and line orders."""
    rng = np.random.default_rng(seed)
    g = win.graph
    h = g.copy()
    pp = rng.permutation(g.n_pt)
    h.pt_xyz, h.pt_id = np.ascontiguousarray(g.pt_xyz[pp]), g.pt_id[pp]
    pe = rng.permutation(g.n_ept)
    h.ept_lm = np.argsort(pp)[g.ept_lm][pe].astype(np.int32)
    h.ept_kf, h.ept_obs, h.ept_info = g.ept_kf[pe], np.ascontiguousarray(g.ept_obs[pe]), g.ept_info[pe]
    pl = rng.permutation(g.n_ln) if variant == PLUCKER else np.arange(g.n_ln)
    h.ln_orth, h.ln_id = np.ascontiguousarray(g.ln_orth[pl]), g.ln_id[pl]
    pq = rng.permutation(g.n_eln)
    h.eln_lm = np.argsort(pl)[g.eln_lm][pq].astype(np.int32)
    h.eln_kf, h.eln_obs, h.eln_info = g.eln_kf[pq], np.ascontiguousarray(g.eln_obs[pq]), g.eln_info[pq]
    line3d = None if win.ln_line3d is None else np.ascontiguousarray(win.ln_line3d[pl])
    return HlmWindow(h, win.kf_x, np.ascontiguousarray(win.ln_pluker[pl]), line3d), pp, pl


DENSE_MAX_N = 1000   # unknowns up to which the checkers' literal N×N solve is also run (C1L: 894)


def n_unknowns(c: Case) -> int:
    g = c.window().graph
    return 6 * int((g.kf_fixed == 0).sum()) + 3 * g.n_pt + (4 if c.variant == PLUCKER else 6) * g.n_ln


def reorderings(c: Case) -> list:
    """[(label, run)]: the checker on the case in three other orders and, on a small window, through
    its dense solve; run(k) is the result with max_iters = k, its landmarks back in the case's order."""
    def back(o, pp, pl):
        o = dict(o)
        for key, perm in (("pt_xyz", pp), ("ln_orth", pl), ("ln_line3d", pl)):
            a = np.asarray(o[key])
            if len(a) == len(perm):
                b = np.empty_like(a)
                b[perm] = a
                o[key] = b
        return o

    out = []
    for seed in (1, 2, 3):
        q, pp, pl = permuted(c.variant, c.window(), seed)
        out.append((f"order {seed}", functools.lru_cache(maxsize=None)(
            lambda k, q=q, pp=pp, pl=pl: back(run_checker(c.variant, q, c.params(max_iters=k)), pp, pl))))
    if c.dense and n_unknowns(c) <= DENSE_MAX_N:
        out.append(("dense", functools.lru_cache(maxsize=None)(
            lambda k: run_checker(c.variant, c.window(), c.params(max_iters=k), dense=True))))
    return out


def bar_figures(out: dict, ref: dict, win: HlmWindow) -> dict:
    """Every figure test_gpu_hlm._compare bounds, divided by its bar (<= 1 passes), for two results
    with the same flow: what the admission checks measure between the checker and its reordered runs."""
    g = win.graph
    fig = {}
    for key, x0 in (("kf_Tcw", g.kf_Tcw), ("pt_xyz", g.pt_xyz),
                    ("ln_line3d", win.ln_line3d) if win.ln_line3d is not None else ("ln_orth", g.ln_orth)):
        a, b = np.asarray(out[key], np.float64), np.asarray(ref[key], np.float64)
        if b.size:
            x0 = np.asarray(x0, np.float64).reshape(b.shape)
            fig[key] = float(np.abs(a - b).max() / (1e-4 * np.abs(b - x0).max() + 1e-12 * max(np.abs(b).max(), 1.0)))
    fig["kf_x"] = float(np.abs(out["kf_x"] - ref["kf_x"]).max() / 1e-6)
    for key in ("lambda_start", "lambda_end"):
        a, b = out["trace"][key], ref["trace"][key]
        fig[key] = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) / 1e-9)
    if np.isfinite(ref["err"]):
        fig["err"] = abs(out["err"] - ref["err"]) / abs(ref["err"]) / 1e-9
    fig["dx_norm"] = abs(out["dx_norm"] - ref["dx_norm"]) / (1e-4 * abs(ref["dx_norm"]) + 1e-30)
    return fig


def flow_of(o: dict) -> tuple:
    return tuple(int(r) for r in o["trace"]["result"]), (o["linearizations"], o["solves"], o["accepted"])


@functools.lru_cache(maxsize=None)
def admission(c: Case) -> dict:
    """What the admission checks assert of a case, measured once: its decisions with, for each, the
    margin |quantity − threshold| and the reordering noise, the largest difference of that quantity
    between the checker and its reordered runs; and the worst bar figure of a reordered run."""
    p = c.params()
    n = len(c.reference()["trace"])
    dec = decisions(history(c.prefix, n), p)
    noise = [0.0] * len(dec)
    worst, flows = 0.0, []
    for label, run in reorderings(c):
        flows.append((label, flow_of(run(p.max_iters))))
        # a reordered run with another flow: some decision has no margin, the candidate is not admitted
        assert flows[-1][1] == flow_of(c.reference()), (c.id, label, flows[-1][1], flow_of(c.reference()))
        other = decisions(history(run, n), p)
        for i, (d, o) in enumerate(zip(dec, other)):
            noise[i] = max(noise[i], abs(d[2] - o[2]))
        worst = max(worst, max(bar_figures(run(p.max_iters), c.reference(), c.window()).values()))
    rows = [dict(it=d[0], name=d[1], value=d[2], threshold=d[3], outcome=bool(d[4]), margin=abs(d[2] - d[3]), noise=nz)
            for d, nz in zip(dec, noise)]
    return dict(rows=rows, flows=flows, bar=worst)


# ---- first-pass residuals and depths² of a window, for the clamp cases ------------------------------

def first_pass(variant: int, win: HlmWindow, state: dict | None = None) -> dict:
    """r of every point row and line row and gz² of every projected point / endpoint, at the map state
    (the first linearisation) or, for variant 2 with `state` a checker result, as a later linearisation
    reads it (aliased endpoints, map poses for lines, poses from X for points)."""
    g = win.graph
    cam = (g.fx, g.fy, g.cx, g.cy)
    T = np.asarray(g.kf_Tcw, np.float64).reshape(-1, 3, 4)
    Xp = np.asarray(g.pt_xyz, np.float64).reshape(-1, 3)
    Tp = T
    if state is not None:
        Tp, Xp = np.asarray(state["kf_Tcw"]).reshape(-1, 3, 4), np.asarray(state["pt_xyz"]).reshape(-1, 3)
    Te = Tp[g.ept_kf]
    G = np.einsum("eij,ej->ei", Te[:, :, :3], Xp[g.ept_lm]) + Te[:, :, 3]
    out = dict(r_pt=ref_lba_endpoints.point_obs(Te, Xp[g.ept_lm], g.ept_obs.reshape(-1, 2), cam, 1e-7)[0],
               z2_pt=G[:, 2] ** 2)
    if not g.n_eln:
        out.update(r_ln=np.zeros(0), z2_ln=np.zeros(0))
    elif variant == PLUCKER:
        out["r_ln"] = np.array([oa.hlm_line_obs(T[g.eln_kf[e]], win.ln_pluker[g.eln_lm[e]], g.eln_obs[e], cam)[0]
                                for e in range(g.n_eln)])
        out["z2_ln"] = np.zeros(0)   # the Plücker line row has no depth
    else:
        Xl = np.asarray(win.ln_line3d if state is None else state["ln_line3d"], np.float64).reshape(-1, 6)
        if state is None:
            P, Q = Xl[g.eln_lm, :3], Xl[g.eln_lm, 3:]
        else:
            P = Q = Xl.reshape(-1)[3 * g.eln_lm[:, None] + np.arange(3)[None, :]]
        Tl = T[g.eln_kf]
        out["r_ln"] = ref_lba_endpoints.line_obs(Tl, P, Q, g.eln_obs.reshape(-1, 4)[:, :3], cam, 1e-7)[0]
        out["z2_ln"] = np.concatenate([(np.einsum("ej,ej->e", Tl[:, 2, :3], V) + Tl[:, 2, 3]) ** 2 for V in (P, Q)])
    return out


# ---- the candidates ------------------------------------------------------------------------------------

def _t(**kw):
    return tuple(kw.items())


NOISY = _t(noise_px=20, outlier_frac=0)              # C1 with 20 px noise: the second err is higher
OUTLIERS = _t(noise_px=5, outlier_frac=0.3)          # C1, 5 px and 30 % outliers: the third err is
EXACT = _t(noise_px=0, outlier_frac=0, perturb=False)   # exact observations of the true map
FINITE = _t(err_per_obs=1)
CONFIG_STOPS = _t(min_error=1e-7, min_error_change=1e-7)   # GBA with the Config stop tests in place of ε

# err > err_prev after one, two and three applied steps; X does not move, so the next err repeats and
# the run ends with result 3. The small λ0 let the first steps be long enough to overshoot; smaller
# ones still (1e-12) reject as well, but there the checker's own reordered runs differ by a third of
# the states' bar
NOISY_OUTLIERS = _t(noise_px=10, outlier_frac=0.3)
REJECT = [
    Case("reject after 1 step", PLUCKER, "C1", NOISY, FINITE + _t(lambda0=1e-10), (0, 1, 3), (3, 2, 1), "derr"),
    Case("reject after 2 steps", PLUCKER, "C1", _t(noise_px=10, outlier_frac=0.1), FINITE + _t(lambda0=1e-9), (0, 0, 1, 3),
         (4, 3, 2), "derr"),
    Case("reject after 1 step, C1L", GBA, "C1L", (), FINITE, (0, 1, 3), (3, 2, 1), "derr"),
    Case("reject after 1 step, C2", GBA, "C2", (), FINITE, (0, 1, 3), (3, 2, 1), "derr"),
    Case("reject after 2 steps", GBA, "C1L", NOISY_OUTLIERS, FINITE + _t(lambda0=1e-9), (0, 0, 1, 3), (4, 3, 2), "derr"),
    Case("reject after 3 steps", GBA, "C1L", NOISY, FINITE + _t(lambda0=1e-9), (0, 0, 0, 1, 3), (5, 4, 3), "derr"),
    Case("reject after 1 step, C1L", ENDPOINTS, "C1L", (), FINITE, (0, 1, 3), (3, 2, 1), "derr"),
    Case("reject after 1 step, C2", ENDPOINTS, "C2", (), FINITE, (0, 1, 3), (3, 2, 1), "derr"),
    Case("reject after 2 steps", ENDPOINTS, "C1L", NOISY_OUTLIERS, FINITE + _t(lambda0=1e-9), (0, 0, 1, 3), (4, 3, 2), "derr"),
]
# λ0 = 1e-24: both solves fail on a zero landmark pivot (DX = 0, nothing applied), err still rises (the
# later linearisation reads the endpoints at the aliased offset), so λ /= k runs with ok == false, and
# ‖DX‖ = 0 < min_error_change ends the run. The pivot is exactly zero when the landmark blocks are
# eliminated first, in any order of the edges (tests/test_gpu_zero_pivot.py); the checkers'
# dense solve eliminates the poses first and meets no zero, so it is no reordering of these cases
REJECT_FAILED = [Case(f"reject with failed solves, {cfg}", v, cfg, (), FINITE + _t(lambda0=1e-24), (0, 1), (2, 2, 0), "dx",
                      dense=False)
                 for v in (GBA, ENDPOINTS) for cfg in ("C1L", "C2")]
# min_error_change = 0: |err − err_prev| < 0 and ‖DX‖ < 0 never hold, err < min_error alone stops: at
# min_error = 0.6, which the descent from λ0 = 1e-7 passes between 0.6126 and 0.5854
MIN_ERROR = [Case("err < min_error alone", v, "C1", (), FINITE + _t(min_error_change=0.0, min_error=0.6, lambda0=1e-7),
                  (0, 0, 0, 3), (4, 3, 3), "min_error") for v in (PLUCKER, GBA, ENDPOINTS)]
# ... and at the Config value 1e-7 on exact observations of the true map: err = 6e-12 after one step.
# Checked on the checkers only: g is rounding noise there, and so is the step (‖DX‖ = 7e-7), so no two
# implementations agree on the state. GBA's int Hmax leaves its first solve a zero pivot, nothing applied
MIN_ERROR_EXACT = [Case("err < min_error alone, exact data", v, "C1", EXACT, FINITE + _t(min_error_change=0.0, min_error=1e-7),
                        (0, 3), (2, 1, 1), "min_error") for v in (PLUCKER, ENDPOINTS)]
# nine applied steps from λ0 = 1e-7, then |err − err_prev| = 2.4e-8 against err = 0.58 and ‖DX‖ = 1.06e-6
DERR = [Case("|derr| alone", v, "C1", (), FINITE + _t(lambda0=1e-7) + (CONFIG_STOPS if v == GBA else ()),
             (0,) * 9 + (3,), (10, 9, 9), "derr") for v in (PLUCKER, GBA, ENDPOINTS)]
# the reference's parameters on C1. Variants 0 and 1 (err = +inf, no test on err can hold): ‖DX‖ falls by
# ten per step, 1.36e-7 then 1.36e-8. Variant 2 (a finite err from the second linearisation on):
# min_error_change = 1.5e-7 lies between |derr| = 1.67e-7 and ‖DX‖ = 1.36e-7 of its eighth iteration
DX = [
    Case("|DX| alone", PLUCKER, "C1", (), (), (0,) * 9, (9, 9, 9), "dx"),
    Case("|DX| alone", GBA, "C1", (), CONFIG_STOPS, (0,) * 9, (9, 9, 9), "dx"),
    Case("|DX| alone", ENDPOINTS, "C1", (), _t(min_error_change=1.5e-7), (0,) * 8, (8, 8, 8), "dx"),
]
# the cap, while every test still fails by a margin (GBA: its own ε tests)
MAX_ITERS = [
    Case("max_iters", PLUCKER, "C1", (), FINITE + _t(lambda0=1e-7, max_iters=5), (0,) * 5, (5, 5, 5), "max_iters"),
    Case("max_iters", GBA, "C1", (), FINITE + _t(max_iters=6), (0,) * 6, (6, 6, 6), "max_iters"),
    Case("max_iters", ENDPOINTS, "C1", (), FINITE + _t(lambda0=1e-7, max_iters=5), (0,) * 5, (5, 5, 5), "max_iters"),
]
STOPS = MIN_ERROR + DERR + DX + MAX_ITERS


@dataclasses.dataclass(frozen=True)
class Clamp:
    """A raised-homog_th case and the rows of its first linearisation below homog_th: (below, of) per
    kind, r of the point rows and of the line rows, gz² of the points and of the line endpoints."""
    case: Case
    r_pt: tuple
    r_ln: tuple
    z2_pt: tuple
    z2_ln: tuple


def _c(name, v, cfg, hth, prm, results, counters, stop):
    return Case(name, v, cfg, (), FINITE + _t(homog_th=hth) + prm, results, counters, stop)


# homog_th = 3: max(homog_th, r) clamps the rows with r < 3 px, no depth² (>= 3.9 m²) is below it.
# homog_th = 16: 1/max(homog_th, gz²) clamps the points nearer than 4 m, and nearly every r as well.
CLAMPS = [
    Clamp(_c("homog_th = 3, point rows", PLUCKER, "C1", 3.0, (), (0,) * 7 + (3,), (8, 7, 7), "derr"),
          (326, 2384), (0, 0), (0, 2384), (0, 0)),
    Clamp(_c("homog_th = 3, Pluecker line rows", PLUCKER, "C1L", 3.0, _t(lambda0=1e-24), (0, 0, 0, 0, 3), (5, 4, 4), "derr"),
          (256, 936), (63, 199), (0, 936), (0, 0)),
    Clamp(_c("homog_th = 16, depths", PLUCKER, "C1", 16.0, (), (0, 0, 1, 3), (4, 3, 2), "derr"),
          (2283, 2384), (0, 0), (757, 2384), (0, 0)),
    Clamp(_c("homog_th = 3, line rows", GBA, "C1L", 3.0, _t(lambda0=1e-7, max_iters=6), (0,) * 6, (6, 6, 6), "max_iters"),
          (256, 936), (56, 199), (0, 936), (0, 398)),
    Clamp(_c("homog_th = 16, depths", GBA, "C1L", 16.0, _t(max_iters=6), (0,) * 6, (6, 6, 6), "max_iters"),
          (901, 936), (196, 199), (332, 936), (88, 398)),
    Clamp(_c("homog_th = 3, line rows", ENDPOINTS, "C1L", 3.0, _t(lambda0=1e-7), (0,) * 9 + (3,), (10, 9, 9), "derr"),
          (256, 936), (56, 199), (0, 936), (0, 398)),
    Clamp(_c("homog_th = 16, depths", ENDPOINTS, "C1L", 16.0, (), (0,) * 8 + (3,), (9, 8, 8), "derr"),
          (901, 936), (196, 199), (332, 936), (88, 398)),
]
# the endpoint-line LBA uses homog_th for its line rows on the first linearisation only and the literal
# 1e-7 afterwards: this case applies eight later steps whose line rows lie between the two
LATER_PASSES = CLAMPS[5].case

# one reject and one raised-homog_th case through each factorisation family the hand-rolled step graphs
# embed their pose update in, on the small windows of test_gpu_hlm.py and test_gpu_lba_endpoints.py, so
# that each kernel's pose update sees a step that is not applied:
# the register-window band kernel (a band ~20 pose blocks wide) ...
WIDE = _t(n_kf=30, n_pt=400, seed=35, track_min=2, track_max=30, fixed_frac=0.1)
WIDE_BAND = [
    Case("wide band, reject after 1 step", PLUCKER, "C1", WIDE + NOISY, FINITE + _t(lambda0=1e-9), (0, 1, 3), (3, 2, 1), "derr",
         family="band"),
    Case("wide band, homog_th = 3", PLUCKER, "C1", WIDE, FINITE + _t(homog_th=3.0, max_iters=4), (0,) * 4, (4, 4, 4), "max_iters",
         family="band"),
    Case("wide band, reject after 1 step", ENDPOINTS, "C1", WIDE + _t(n_ln=60), FINITE, (0, 1, 3), (3, 2, 1), "derr",
         family="band"),
    Case("wide band, homog_th = 16", ENDPOINTS, "C1", WIDE + _t(n_ln=60), FINITE + _t(homog_th=16.0, max_iters=4), (0,) * 4,
         (4, 4, 4), "max_iters", family="band"),
]
# ... the two-sided column-lane kernel: the 60-KF short trajectory (54 free keyframes), max_iters = 4 ...
KF60 = _t(n_kf=60, n_pt=6000, n_ln=1200)
COLUMN_LANE = [
    Case("column lane, reject after 1 step", ENDPOINTS, "C3", KF60, FINITE + _t(max_iters=4), (0, 1, 3), (3, 2, 1), "derr",
         family="column_lane"),
    Case("column lane, homog_th = 3", ENDPOINTS, "C3", KF60, FINITE + _t(max_iters=4, homog_th=3.0), (0, 1, 3), (3, 2, 1), "derr",
         family="column_lane"),
]
# ... and block cyclic reduction: the smallest window plba_factor_plan sends there at the band width of
# these tracks (bw 7: 206 free keyframes and one fixed; the GPU test checks that 205 would not)
BCR_NF = 206
BCR_WINDOW = _t(n_kf=BCR_NF + 1, n_pt=3000, n_ln=300, seed=77, fixed_frac=0.0)
BCR = [
    Case("bcr, reject after 1 step", GBA, "C1", BCR_WINDOW, FINITE + _t(max_iters=3), (0, 1, 3), (3, 2, 1), "derr", family="bcr"),
    Case("bcr, homog_th = 16", GBA, "C1", BCR_WINDOW, FINITE + _t(max_iters=3, homog_th=16.0), (0, 0, 0), (3, 3, 3), "max_iters",
         family="bcr"),
]
FAMILIES = WIDE_BAND + COLUMN_LANE + BCR

ALL = REJECT + REJECT_FAILED + STOPS + [c.case for c in CLAMPS] + FAMILIES
REJECTS = [c for c in ALL if 1 in c.results]

