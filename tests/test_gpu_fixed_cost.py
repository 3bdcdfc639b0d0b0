"""What a solve does outside its step graphs (DESIGN §2 "Fixed per-solve cost"): the one-launch
reset of the estimates (k_reset_estimates) and the schedule's single poll, with the level-1 χ²
refresh queued behind the steps as a device-gated epilogue. None of it changes any arithmetic, so
every comparison here is bitwise."""
import os

import numpy as np
import pytest

import graph_mut as gm
from plba import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2o_sequence_C1L.npz")
KEYS = ("iters", "chi2", "kf_Tcw", "pt_xyz", "ln_orth", "ept_chi2", "ept_depth_ok", "eln_chi2")


class _Env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bits(x):
    x = np.ascontiguousarray(np.asarray(x))
    return x.shape, x.dtype, x.tobytes()


def _assert_same(a, b, what, keys=KEYS):
    for k in keys:
        assert _bits(a[k]) == _bits(b[k]), (what, k)
    assert _bits(a["trace"]) == _bits(b["trace"]), (what, a["trace"], b["trace"])


def _state(s):
    T, P, O = s.download()
    pc, pd, lc = s.edge_chi2()
    return dict(kf_Tcw=T, pt_xyz=P, ln_orth=O, ept_chi2=pc, ept_depth_ok=pd, eln_chi2=lc)


@pytest.mark.parametrize("slots", [1, 2, 4])
@pytest.mark.parametrize("cfg", ["C1L", "C2"])
def test_reset_equals_a_fresh_upload(cfg, slots):
    """Estimates, per-edge χ² and the next solve after reset are those of a fresh upload, for every
    count of solve / χ² buffers the reset kernel loops over."""
    from plba.lib import Solver
    g = synth.generate(cfg)
    with _Env(PLBA_SPEC=slots):
        with Solver() as s:
            s.upload(g)
            assert s.structure_stats()["spec_slots"] == slots
            fresh = _state(s)
            fresh_solve = s.lba_plucker()
        with Solver() as s:
            s.upload(g)
            s.lba_plucker()
            s.reset()
            again = _state(s)
            again_solve = s.lba_plucker()
    for k in fresh:
        assert _bits(fresh[k]) == _bits(again[k]), k
    _assert_same(fresh_solve, again_solve, (cfg, slots))


def _degenerate(name):
    if name == "no_lines":
        return gm.drop_lines(synth.generate("C1L"))
    if name == "all_fixed":
        return gm.all_fixed(synth.generate("C1L"))
    return synth.generate("C1L", n_kf=6, n_pt=60, n_ln=12, seed=5, fixed_frac=0.5)  # the suite's smallest


@pytest.mark.parametrize("name", ["no_lines", "all_fixed", "smallest"])
def test_reset_of_degenerate_windows(name):
    """Windows whose arrays are empty (no lines; no free pose) and the smallest one: reset then
    solve, twice, gives the same bits and no error status (a non-zero status raises)."""
    from plba.lib import Solver
    g = _degenerate(name)
    if name == "no_lines":
        assert g.n_ln == 0
    if name == "all_fixed":
        assert bool(np.all(g.kf_fixed))
    with Solver() as s:
        s.upload(g)
        s.reset()
        a = s.lba_plucker()
        s.reset()
        b = s.lba_plucker()
    _assert_same(a, b, name)


def test_too_short_first_batch():
    """A context whose previous schedule was short predicts too few steps for C2: the epilogue queued
    behind the first batch finds the schedule unfinished and does nothing, later batches finish it
    and the epilogue behind the last one lands. Bitwise C2 solved in a fresh context."""
    from plba.lib import Solver
    g = synth.generate("C2")
    with Solver() as s:
        s.upload(g)
        ref = s.lba_plucker()
        ref_steps = s.structure_stats()["device_steps"]
    with Solver() as s:
        # a short schedule on a small window: one iteration of the g2o call sequence
        s.upload(synth.generate("C1L", n_kf=6, n_pt=60, n_ln=12, seed=5, fixed_frac=0.5))
        s.initialize_optimization(0)
        s.optimize(1)
        small_steps = s.structure_stats()["device_steps"]
        # the first batch of the next schedule is max(4, small_steps + 1) steps: too few for C2
        assert max(4, small_steps + 1) < ref_steps, (small_steps, ref_steps)
        s.upload(g)
        out = s.lba_plucker()
        assert s.structure_stats()["device_steps"] == ref_steps
    _assert_same(ref, out, "C2 after a short schedule")


def test_level1_refresh_still_lands():
    """lba_plucker leaves the level-1 edges' χ² at the final state: an explicit refresh of level 1
    afterwards changes nothing."""
    from plba.lib import Solver
    g = synth.generate("C2")
    with Solver() as s:
        s.upload(g)
        out = s.lba_plucker()
        n1 = int((out["ept_level"] == 1).sum() + (out["eln_level"] == 1).sum())
        assert n1 > 0, "stage 1 classified no edge as an outlier: the test would pass vacuously"
        pc, _, lc = s.edge_chi2()
        s.refresh_edge_errors(1)
        pc2, _, lc2 = s.edge_chi2()
    assert _bits(pc) == _bits(pc2) and _bits(lc) == _bits(lc2)
    assert _bits(out["ept_chi2"]) == _bits(pc) and _bits(out["eln_chi2"]) == _bits(lc)


def g2o_sequence(s, g):
    """initializeOptimization / optimize(5) / levels from the χ² test / optimize(10), as the g2o
    facade drives it; every output of it by name."""
    s.upload(g)
    s.set_robust(True)
    s.initialize_optimization(0)
    it1, chi1 = s.optimize(5)
    tr1 = s.trace()
    pc, pd, lc = s.edge_chi2()
    s.set_edge_levels((pc > 5.991).astype(np.uint8), (lc > 7.815).astype(np.uint8))
    s.set_robust(False)
    s.initialize_optimization(0)
    it2, chi2 = s.optimize(10)
    tr2 = s.trace()
    T, P, O = s.download()
    pc2, pd2, lc2 = s.edge_chi2()
    return dict(iters=np.array([it1, it2]), chi2=np.array([chi1, chi2]), kf_Tcw=T, pt_xyz=P, ln_orth=O,
                ept_chi2_stage1=pc, ept_depth_ok_stage1=pd, eln_chi2_stage1=lc,
                ept_chi2=pc2, ept_depth_ok=pd2, eln_chi2=lc2,
                trace1=np.frombuffer(np.ascontiguousarray(tr1).tobytes(), np.uint8),
                trace2=np.frombuffer(np.ascontiguousarray(tr2).tobytes(), np.uint8))


def test_g2o_call_sequence_is_unchanged():
    """The sequence's outputs, bitwise those recorded on an MI355X from the commit before the
    single-poll schedule (tests/golden/g2o_sequence_C1L.npz: this project's own outputs)."""
    from plba.lib import Solver
    with Solver() as s:
        out = g2o_sequence(s, synth.generate("C1L"))
    exp = np.load(GOLDEN)
    assert sorted(exp.files) == sorted(out)
    for k in exp.files:
        assert _bits(out[k]) == _bits(exp[k]), k
