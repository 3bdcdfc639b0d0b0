"""The ctypes binding of the host mirror (plba/slam_map.py) against include/plslam_host.h, and the one hook
dispatch of MapHandler behind every entry point that has a device backend: what a failing or raising hook
reports, what "cpu" stands for, and what a map without a usable device reports with no hook set. Every map is
built by the case builders of the tests/test_host_*.py of its entry point, on a device index that plba_create
refuses before it touches a device, so nothing here reaches a GPU. No GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import bow_cases
import fuse_model as FM
import lcpose_cases
import mapmatch_cases as mc
import stereo_cases as SC
import test_host_bow as TB
import test_host_isloopclosure as IL
import test_host_kfmatch as KM
import test_host_lcpose as LP
import test_host_mapassoc as MA
import test_host_mapmatch as TM
import test_host_mirror_lba_endpoints as EP
import test_host_pgo as PG
import test_host_stereo as TS
from plba import slam_map, synth
from plba.lib import PlbaError
from plba.slam_map import HOOKS, HOST_ARGTYPES, HOST_LIB_PATH, HostMap, make_map, match_params

pytestmark = pytest.mark.skipif(not os.path.exists(HOST_LIB_PATH), reason="libplslam_host.so not built")

NO_DEVICE = 2 ** 20   # plba_create refuses an index out of range before it touches a device


class NoDeviceMap(HostMap):
    def __init__(self, m, **kw):
        super().__init__(m, device=NO_DEVICE, **kw)


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Every HostMap the case builders make sits on NO_DEVICE."""
    for mod in (slam_map, TB, IL, KM, LP, TM, EP, PG, TS):
        monkeypatch.setattr(mod, "HostMap", NoDeviceMap)


# ---- include/plslam_host.h against HOST_ARGTYPES
def _declarations():
    """name -> parameter count of every function the header declares. The hooks are passed by typedef name, so a
    parameter list holds no parenthesis and its parameters are its commas plus one."""
    txt = open(os.path.join(os.path.dirname(__file__), "..", "include", "plslam_host.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(plslam_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params == "void" else params.count(",") + 1
    assert set(out) == set(re.findall(r"\b(plslam_[a-z0-9_]+)\s*\(", txt))   # no declaration spells a hook inline
    return out


def test_the_table_binds_exactly_what_the_header_declares():
    decl = _declarations()
    assert set(decl) == set(HOST_ARGTYPES), set(decl) ^ set(HOST_ARGTYPES)
    L = slam_map.load_host()
    for name, argtypes in HOST_ARGTYPES.items():
        assert hasattr(L, name), name
        assert len(argtypes) == decl[name], name
        assert getattr(L, name).argtypes == argtypes
    assert slam_map.HOST_EXPORTED == list(HOST_ARGTYPES)


# ---- one scene per entry point with a device backend: (hook of HOOKS, the prefix of its failure, builder);
# a builder gives the map and the call that reaches the backend
@functools.lru_cache(maxsize=None)
def _window():
    return synth.generate("C1L", fixed_frac=0.3)


@functools.lru_cache(maxsize=None)
def _built(which):
    return dict(mapmatch=mc.build, kfmatch=KM.build, stereo=lambda: TS._map(None, False), fuse=FM.scenario,
                stereo_frame=lambda: SC.case("mixed"))[which]()


def _lba():
    h = NoDeviceMap(make_map(_window(), seed=6))
    return h, h.local_ba


def _hlm():
    h = NoDeviceMap(make_map(_window(), seed=6))
    return h, h.local_ba_hlm


def _endpoints():
    h = EP.endpoint_map()[2]
    return h, h.local_ba_endpoints


def _pgo():
    h = PG._hostmap()[1]
    return h, h.loop_closure


def _lcpose():
    h = LP._hostmap(hooks=False)[0]
    return h, lambda: LP._step(h, lcpose_cases.problem(40, 12, 0.25), n_feat=(200, 100, 30, 100))


def _match():
    h = IL.hostmap(hooks=False)[0]
    return h, lambda: h.loop_closure_step_kf(IL.PLANTED[0], IL.KF_CURR, match_params())


def _grid():
    built = _built("mapmatch")
    h = TM.hostmap(built, hooks=False)[0]
    return h, lambda: _timeless(h.match_map_to_kf(mc.KF_NEW, built[3])), lambda: TM.state(h, built[0])


def _mapassoc():
    built = _built("mapmatch")
    h = MA.assoc_hostmap(built, hook=None)
    return h, lambda: _timeless(h.match_map_to_kf_assoc(mc.KF_NEW, built[3])), lambda: TM.state(h, built[0])


def _stereo():
    built = _built("stereo")
    h = NoDeviceMap(built[0])
    return h, lambda: _timeless(h.set_keyframe_stereo(mc.KF_NEW, _built("stereo_frame"), TS.PRM))


def _kfassoc():
    built = _built("kfmatch")
    h = KM.hostmap(built, hooks=False)
    return h, lambda: _timeless(h.match_kf_to_kf(KM.PREV, KM.CURR, KM.DT4(built[1]))), lambda: KM.state(h)


def _medoid():
    sc = _built("fuse")
    h = FM.host_map(*sc, medoid=None)

    def med_descs():   # of every landmark, the ones the fuse created (past the map's own) included
        out, md = [], np.zeros(slam_map.DESC_BYTES, np.uint8)
        p = md.ctypes.data_as(C.POINTER(C.c_uint8))
        for kind, n in ((1, h.n_pt), (2, h.n_ln)):
            for idx in range(n + 16):
                if h.exists(kind, idx):
                    rc = (h.L.plslam_get_point(h.h, idx, None, None, None, None, None, None, None, None, 0, p, None) if kind == 1
                          else h.L.plslam_get_line(h.h, idx, None, None, None, None, None, None, None, 0, p))
                    assert rc == 0
                    out.append((kind, idx, md.tobytes()))
        return out
    return h, lambda: _timeless(h.fuse_landmarks()), med_descs


def _bow():
    h = TB.bow_hostmap(3, {i: bow_cases.keyframe(i) for i in range(3)}, bow=False)[0]
    return h, lambda: h.set_vocabulary(0, bow_cases.vocab("k10L3"))


def _timeless(d):
    """A result without its wall times, comparable between two runs."""
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items() if k != "ms" and not k.endswith("_ms")}


SCENES = {
    "local_ba": ("solver", "solver", _lba),
    "local_ba_hlm": ("hlm", "hand-rolled LM solver", _hlm),
    "local_ba_endpoints": ("hlm", "hand-rolled LM solver", _endpoints),
    "loop_closure": ("pgo", "pose-graph solver", _pgo),
    "loop_closure_step": ("lcpose", "relative-pose solver", _lcpose),
    "loop_closure_step_kf": ("match", "matcher", _match),
    "match_map_to_kf": ("grid", "grid matcher", _grid),
    "set_keyframe_stereo": ("stereo", "stereo", _stereo),
    "match_kf_to_kf": ("kfassoc", "keyframe association", _kfassoc),
    "match_map_to_kf_assoc": ("mapassoc", "map association", _mapassoc),
    "fuse_landmarks": ("medoid", "medoid", _medoid),
    "set_vocabulary": ("bow", "place-recognition", _bow),
}
scenes = pytest.mark.parametrize("scene", list(SCENES))
SETTERS = dict(solver="set_solver", hlm="set_hlm_solver", pgo="set_pgo_solver", lcpose="set_lcpose_solver",
               match="set_match_fn", medoid="set_medoid_fn", stereo="set_stereo_fn", kfassoc="set_kfassoc_fn",
               grid="set_grid_match_fn", mapassoc="set_mapassoc_fn", bow="set_bow_fn")


def set_hook(h, hook, fn):
    getattr(h, SETTERS[hook])(fn)


def test_the_scenes_cover_every_hook():
    assert {s[0] for s in SCENES.values()} == set(HOOKS) == set(SETTERS)


@scenes
def test_a_failing_hook_is_reported_under_its_prefix(scene):
    hook, prefix, build = SCENES[scene]
    h, call = build()[:2]
    seen = []
    set_hook(h, hook, lambda *a: seen.append(len(a)) or 7)
    with pytest.raises(PlbaError, match=re.escape(prefix + " hook returned 7")):
        call()
    assert seen == [len(HOOKS[hook][1]._argtypes_) - 1]   # called once, with everything but the user pointer
    h.close()


@scenes
def test_a_raising_hook_returns_minus_one_and_does_not_unwind(scene, capfd):
    hook, prefix, build = SCENES[scene]
    h, call = build()[:2]

    def boom(*a):
        raise KeyError("raised inside the hook")
    set_hook(h, hook, boom)
    with pytest.raises(PlbaError, match=re.escape(prefix + " hook returned -1")):
        call()
    assert "KeyError: 'raised inside the hook'" in capfd.readouterr().err   # the traceback is printed instead
    h.close()


@scenes
def test_without_a_usable_device_every_backend_says_so(scene):
    """No hook, and after a hook was set and cleared: plba_create's refusal, never a message about a null context."""
    hook, _, build = SCENES[scene]
    for clear_first in (False, True):
        h, call = build()[:2]
        if clear_first:
            set_hook(h, hook, lambda *a: 7)
            set_hook(h, hook, None)
        with pytest.raises(PlbaError) as e:
            call()
        assert "plba_create failed" in str(e.value) and "null context" not in str(e.value)
        h.close()


CPU_HOOKS = {hook: cpu for hook, (_, _, _, cpu) in HOOKS.items() if cpu}


def test_five_hooks_have_a_cpu_restatement():
    assert set(CPU_HOOKS) == {"medoid", "stereo", "kfassoc", "mapassoc", "grid"}


@pytest.mark.parametrize("scene", [s for s, v in SCENES.items() if v[0] in CPU_HOOKS])
def test_cpu_is_the_restatement_passed_straight_through(scene):
    """ "cpu" and a Python hook that forwards to the same plslam_*_cpu leave the same result and the same map."""
    hook, _, build = SCENES[scene]
    results = []
    for direct in (True, False):
        h, call, *state = build()
        cpu = getattr(h.L, CPU_HOOKS[hook])
        calls = []

        def forward(*a):
            calls.append(1)
            return cpu(None, *(C.byref(x) if isinstance(x, C.Structure) else x for x in a))
        set_hook(h, hook, "cpu" if direct else forward)
        results.append((call(), state[0]() if state else None))
        assert len(calls) == (0 if direct else 1)
        h.close()
    assert results[0] == results[1]


@pytest.mark.parametrize("hook", sorted(set(HOOKS) - set(CPU_HOOKS)))
def test_cpu_is_refused_where_the_library_has_no_restatement(hook):
    h = _lba()[0]
    with pytest.raises(ValueError):
        set_hook(h, hook, "cpu")
    assert hook not in h._hooks
    h.close()


def test_the_callback_is_kept_alive_until_it_is_replaced():
    h = _lba()[0]
    for hook in HOOKS:
        set_hook(h, hook, lambda *a: 0)
        assert isinstance(h._hooks[hook], HOOKS[hook][1]) and h._hooks[hook]
        set_hook(h, hook, None)
        assert not h._hooks[hook]     # a NULL function pointer
    h.close()


# ---- the getters that report their row count
@pytest.mark.parametrize("n", [0, 3])
def test_sized_getters(n):
    h = _lba()[0]
    rng = np.random.default_rng(n)
    idx = rng.integers(0, 100, (n, 3)).astype(np.int32)
    pose = rng.normal(size=(n, 6))
    rows = rng.integers(-1, 100, (n, 4)).astype(np.int32)
    h.set_loop_closure(idx, idx, pose)
    for kind in (1, 2):
        h.set_lc_feature_idxs(kind, 0, rows + kind)
    got = h.lc_idx_list()
    assert got.shape == (n, 3) and got.dtype == np.int32 and np.array_equal(got, idx)
    got = h.lc_pose_list()
    assert got.shape == (n, 6) and got.dtype == np.float64 and np.array_equal(got, pose)
    for kind in (1, 2):
        got = h.lc_feature_idxs(kind, 0)
        assert got.shape == (n, 4) and got.dtype == np.int32 and np.array_equal(got, rows + kind)
    h.close()
