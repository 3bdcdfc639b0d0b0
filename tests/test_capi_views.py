"""The batch views of plba.capi at the smallest shapes where their shared base can go wrong: no library, no GPU.

Each view is described here a second time, by hand (its sides with their offset field and row arrays, its
per-problem arrays, its outputs with their fills), and built from problems whose every array has contents of
its own. What the struct's pointers name is then read back through them."""
import ctypes as C
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "pl-slam-plucker_amd"))
from plba import capi  # noqa: E402

DB = 16                   # not the default of 32, so that an inferred width shows; no other column count
F8, F4, U1, I4 = np.float64, np.float32, np.uint8, np.int32
NAN = np.nan
CAM = (400.0, 410.0, 320.0, 240.0)


def _object(p, **more):
    return SimpleNamespace(**p, **more)


def _grid_problem(p):
    n1, n2 = len(p.get("desc1", ())), len(p.get("desc2", ()))
    return dict(p, kind=0, ws=1, nnr=0.9, cell1=np.zeros((n1, 2), I4), cells2=[np.zeros((1, 2), I4)] * n2)


# name: the class, how a list of plain dicts becomes its constructor's arguments, sides {key: (offset field,
# [(row array, columns, dtype), ...] with the leading array first)}, per-problem arrays, outputs (field,
# side | "n" | "2n", trailing shape, dtype, fill), the text of a short row array, and whether a problem is a dict
VIEWS = dict(
    match=dict(
        cls=capi.MatchBatchView, args=lambda ps: ([(p["desc1"], p["desc2"]) for p in ps], 0.9),
        sides={"1": ("off1", [("desc1", DB, U1)]), "2": ("off2", [("desc2", DB, U1)])}, per=[], out=[], short=None,
        dicts=False),
    grid=dict(
        cls=capi.GridMatchBatchView, args=lambda ps: ([_grid_problem(p) for p in ps],),
        sides={"1": ("off1", [("desc1", DB, U1)]), "2": ("off2", [("desc2", DB, U1)])}, per=[], out=[], short=None,
        dicts=True),
    lcpose=dict(
        cls=capi.LcposeBatchView, args=lambda ps: ([_object(p, cam=CAM) for p in ps],),
        sides={"pt": ("pt_off", [("pt_P", 3, F8), ("pt_obs", 2, F8)]),
               "ln": ("ln_off", [("ln_sP", 3, F8), ("ln_eP", 3, F8), ("ln_le", 3, F8)])},
        per=[], out=[], short="{key}: one row per match", dicts=False),
    track=dict(
        cls=capi.TrackBatchView, args=lambda ps: ([_object(p, cam=CAM) for p in ps],),
        sides={"pt": ("pt_off", [("pt_P", 3, F8), ("pt_obs", 2, F8), ("pt_sigma2", 1, F8)]),
               "ln": ("ln_off", [("ln_sP", 3, F8), ("ln_eP", 3, F8), ("ln_NDc", 6, F8), ("ln_le", 3, F8), ("ln_obs", 4, F8),
                                 ("ln_seg", 4, F8), ("ln_sigma2", 1, F8)])},
        per=[("prev", capi.TRACK_PREV)], out=[], short="{key}: one row per match", dicts=False),
    frames=dict(
        cls=capi.FramesBatchView, args=lambda ps: ([_object(p, cam=CAM) for p in ps], DB),
        sides={"pt1": ("pt_off1", [("prev_pdesc", DB, U1), ("prev_pt_P", 3, F8), ("prev_pt_sigma2", 1, F8)]),
               "pt2": ("pt_off2", [("cur_pdesc", DB, U1), ("cur_pt_pl", 2, F8)]),
               "ln1": ("ln_off1", [("prev_ldesc", DB, U1), ("prev_ln_sP", 3, F8), ("prev_ln_eP", 3, F8), ("prev_ln_NDc", 6, F8),
                                   ("prev_ln_seg", 4, F8), ("prev_ln_sigma2", 1, F8)]),
               "ln2": ("ln_off2", [("cur_ldesc", DB, U1), ("cur_ln_seg", 4, F8), ("cur_ln_le", 3, F8)])},
        per=[("prev", capi.TRACK_PREV)],
        out=[("pt_m12", "pt1", (), I4, -1), ("ln_m12", "ln1", (), I4, -1), ("n_pt", "n", (), I4, 0), ("n_ln", "n", (), I4, 0),
             ("pt_inlier", "pt1", (), U1, 0), ("ln_inlier", "ln1", (), U1, 0), ("pt_cur_from_prev", "pt2", (), I4, -1),
             ("ln_cur_from_prev", "ln2", (), I4, -1)],
        short="{key} has {rows} rows, the descriptors have {lead}", dicts=False),
    stereo=dict(
        cls=capi.StereoBatchView, args=lambda ps: (ps,),
        sides={"pt_l": ("pt_off_l", [("pt_l", 2, F4), ("pdesc_l", DB, U1)]), "pt_r": ("pt_off_r", [("pt_r", 2, F4), ("pdesc_r", DB, U1)]),
               "ls_l": ("ls_off_l", [("ls_l", 4, F4), ("ldesc_l", DB, U1)]), "ls_r": ("ls_off_r", [("ls_r", 4, F4), ("ldesc_r", DB, U1)])},
        per=[],
        out=[("n_pt", "n", (), I4, 0), ("n_ls", "n", (), I4, 0), ("pt_src", "pt_l", (), I4, -7), ("pt_pl", "pt_l", (2,), F8, NAN),
             ("pt_disp", "pt_l", (), F8, NAN), ("pt_P", "pt_l", (3,), F8, NAN), ("pdesc", "pt_l", (DB,), U1, 0),
             ("ls_src", "ls_l", (), I4, -7), ("ls_spl", "ls_l", (2,), F8, NAN), ("ls_epl", "ls_l", (2,), F8, NAN),
             ("ls_sdisp", "ls_l", (), F8, NAN), ("ls_edisp", "ls_l", (), F8, NAN), ("ls_sP", "ls_l", (3,), F8, NAN),
             ("ls_eP", "ls_l", (3,), F8, NAN), ("ls_le", "ls_l", (3,), F8, NAN), ("ls_NDc", "ls_l", (6,), F8, NAN),
             ("ldesc", "ls_l", (DB,), U1, 0)],
        short="one descriptor row per feature", dicts=True),
    kfassoc=dict(
        cls=capi.KfassocBatchView, args=lambda ps: (ps,),
        sides={"pt_p": ("pt_off_p", [("pt_P_p", 3, F8), ("pdesc_p", DB, U1)]),
               "pt_c": ("pt_off_c", [("pt_pl_c", 2, F8), ("pt_P_c", 3, F8), ("pdesc_c", DB, U1)]),
               "ls_p": ("ls_off_p", [("ls_sP_p", 3, F8), ("ls_eP_p", 3, F8), ("ls_NDc_p", 6, F8), ("ls_spl_p", 2, F8), ("ls_epl_p", 2, F8),
                                     ("ldesc_p", DB, U1), ("ls_lm_NDw", 6, F8), ("ls_new", 1, U1)]),
               "ls_c": ("ls_off_c", [("ls_spl_c", 2, F8), ("ls_epl_c", 2, F8), ("ldesc_c", DB, U1)])},
        per=[("DT", 12), ("T_prev", 16), ("T_curr", 16), ("Tcw_prev", 16), ("Tcw_curr", 16)],
        out=[("n_grid", "2n", (), I4, -7), ("n_matches", "2n", (), I4, -7), ("fallback", "2n", (), I4, -7),
             ("pt_m12", "pt_p", (), I4, -7), ("ls_m12", "ls_p", (), I4, -7), ("pt_rec", "pt_p", (9,), F8, NAN),
             ("ls_rec", "ls_p", (8,), F8, NAN), ("ls_rejected", "ls_p", (), U1, 7)],
        short="{key}: one row per feature", dicts=True),
    mapassoc=dict(
        cls=capi.MapassocBatchView, args=lambda ps: (ps,),
        sides={"pt_m": ("pt_off_m", [("pt_X", 3, F8), ("pdesc_m", DB, U1)]), "ls_m": ("ls_off_m", [("ls_X", 6, F8), ("ldesc_m", DB, U1)]),
               "pt_f": ("pt_off_f", [("pt_pl", 2, F8), ("pt_P", 3, F8), ("pdesc_f", DB, U1)]),
               "ls_f": ("ls_off_f", [("ls_spl", 2, F8), ("ls_epl", 2, F8), ("ls_le", 3, F8), ("ls_sP", 3, F8), ("ls_eP", 3, F8),
                                     ("ldesc_f", DB, U1)])},
        per=[("Twf", 12), ("T_kf_w", 16)],
        out=[(k, "2n", (), I4, -7) for k in ("n_visible", "n_grid", "n_matches", "fallback", "n_accepted")] +
            [("pt_visible", "pt_m", (), U1, 7), ("pt_m12", "pt_m", (), I4, -7), ("pt_accepted", "pt_m", (), U1, 7),
             ("pt_rec", "pt_m", (6,), F8, NAN), ("ls_visible", "ls_m", (), U1, 7), ("ls_m12", "ls_m", (), I4, -7),
             ("ls_accepted", "ls_m", (), U1, 7), ("ls_rec", "ls_m", (9,), F8, NAN)],
        short="{key}: one row per landmark or feature", dicts=True),
)
NAMES = sorted(VIEWS)
WITH_ROWS_TO_CUT = [n for n in NAMES if VIEWS[n]["short"]]
WITH_OUTPUTS = [n for n in NAMES if VIEWS[n]["out"]]
DICT_STYLE = [n for n in NAMES if VIEWS[n]["dicts"]]


def problem(name, rows, seed=0):
    """A plain dict with every array of the view: ``rows`` of each side (an int, or {side: rows}), contents of its own."""
    v, rng, p = VIEWS[name], np.random.default_rng(seed), {}
    for side, (_, arrays) in v["sides"].items():
        n = rows if isinstance(rows, int) else rows.get(side, 0)
        for key, cols, dtype in arrays:
            p[key] = rng.integers(1, 255, (n, cols)).astype(dtype) if dtype is U1 else rng.random((n, cols)).astype(dtype)
    for key, width in v["per"]:
        p[key] = rng.random(width)
    return p


def build(name, problems):
    v = VIEWS[name]
    return v["cls"](*v["args"](problems))


def desc_width(name, problems):
    """No problem, no descriptor to read a width from: the default (FramesBatchView is given its own)."""
    return DB if problems or name == "frames" else 32


def through(ptr, like):
    """The memory a struct's pointer names, read as an array like ``like``."""
    assert {C.c_double: F8, C.c_float: F4, C.c_uint8: U1, C.c_int32: I4}[ptr._type_] == like.dtype
    raw = (C.c_char * like.nbytes).from_address(C.cast(ptr, C.c_void_p).value)
    return np.frombuffer(raw, like.dtype).reshape(like.shape)


def check_inputs(name, problems, bv):
    """Offsets, row arrays and per-problem arrays, through the struct's own pointers and under the view's names."""
    v, n, db = VIEWS[name], len(problems), desc_width(name, problems)
    assert bv.struct.n == n
    if hasattr(bv.struct, "desc_bytes"):
        assert bv.struct.desc_bytes == bv.desc_bytes == db
    for side, (off_field, arrays) in v["sides"].items():
        counts = [len(p.get(arrays[0][0], ())) for p in problems]
        want = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        off = getattr(bv, off_field)
        assert off.dtype == np.int32 and np.array_equal(off, want), (side, off, want)
        assert C.cast(getattr(bv.struct, off_field), C.c_void_p).value == off.ctypes.data
        if hasattr(bv, "off") and isinstance(getattr(bv, "off"), dict):
            assert bv.off[side] is off
        for key, cols, dtype in arrays:
            cols = db if cols == DB else cols
            rows = np.concatenate([np.asarray(p.get(key, np.zeros((0, cols))), dtype).reshape(-1, cols) for p in problems] +
                                  [np.zeros((0, cols), dtype)])
            held = getattr(bv, key)
            assert held.dtype == dtype and held.flags.c_contiguous and held.shape == rows.shape, key
            addr = C.cast(getattr(bv.struct, key), C.c_void_p).value
            assert addr is not None and addr == held.ctypes.data, key      # an empty batch still has an address
            assert np.array_equal(through(getattr(bv.struct, key), rows), rows), key
    for key, width in v["per"]:
        rows = np.stack([np.asarray(p[key], F8).reshape(-1)[:width] for p in problems]) if n else np.zeros((0, width))
        held = getattr(bv, key)
        assert held.dtype == F8 and held.shape == (n, width) and C.cast(getattr(bv.struct, key), C.c_void_p).value == held.ctypes.data
        assert np.array_equal(through(getattr(bv.struct, key), rows), rows), key
    if name in ("lcpose", "track", "frames"):
        assert (bv.struct.fx, bv.struct.fy, bv.struct.cx, bv.struct.cy) == (CAM if n else (1.0, 1.0, 0.0, 0.0))


def out_struct(name, bv):
    return bv.out_struct if name == "frames" else bv.out


def check_outputs(name, problems, bv):
    """Every output: its dtype, its shape with at least one row, its fill, and the out struct's pointer to it."""
    v, n = VIEWS[name], len(problems)
    total = {side: sum(len(p.get(arrays[0][0], ())) for p in problems) for side, (_, arrays) in v["sides"].items()}
    for key, side, trail, dtype, fill in v["out"]:
        rows = n if side == "n" else 2 * n if side == "2n" else total[side]
        a = bv.o[key] if hasattr(bv, "o") and key in bv.o else getattr(bv, key)
        trail = (desc_width(name, problems),) if trail == (DB,) else trail
        assert a.dtype == dtype and a.shape == (max(rows, 1),) + trail, key
        assert np.isnan(a).all() if fill is NAN else (a == fill).all(), key
        assert C.cast(getattr(out_struct(name, bv), key), C.c_void_p).value == a.ctypes.data, key


@pytest.mark.parametrize("name", NAMES)
def test_a_batch_of_no_problems(name):
    bv = build(name, [])
    check_inputs(name, [], bv)
    check_outputs(name, [], bv)
    if VIEWS[name]["out"]:
        assert (bv.results(True) if name == "stereo" else bv.results()) == []


@pytest.mark.parametrize("name", NAMES)
def test_one_problem_with_every_side_empty(name):
    ps = [problem(name, 0)]
    bv = build(name, ps)
    check_inputs(name, ps, bv)
    check_outputs(name, ps, bv)


@pytest.mark.parametrize("name", NAMES)
def test_an_empty_side_repeats_an_offset_and_every_pointer_names_its_own_array(name):
    sides = list(VIEWS[name]["sides"])
    first = {s: (0 if i % 2 == 0 else 2 + i) for i, s in enumerate(sides)}       # every other side empty
    second = {s: 3 + i for i, s in enumerate(sides)}
    ps = [problem(name, first, 1), problem(name, second, 2)]
    bv = build(name, ps)
    check_inputs(name, ps, bv)
    check_outputs(name, ps, bv)
    for s in sides[::2]:
        off = getattr(bv, VIEWS[name]["sides"][s][0])
        assert off[0] == off[1] == 0 and off[2] == second[s]
    pointers = [C.cast(getattr(bv.struct, f), C.c_void_p).value for f, t in bv.struct._fields_ if issubclass(t, C._Pointer)]
    assert None not in pointers and len(set(pointers)) == len(pointers)          # no two fields share an array


@pytest.mark.parametrize("name", DICT_STYLE)
def test_a_key_left_out_of_a_dict_is_an_empty_side(name):
    for side, (_, arrays) in VIEWS[name]["sides"].items():
        full = problem(name, 3, 4)
        cut = {k: a for k, a in full.items() if k not in [key for key, _, _ in arrays]}
        ps = [cut, full]
        bv = build(name, ps)
        check_inputs(name, ps, bv)
        check_outputs(name, ps, bv)


@pytest.mark.parametrize("name", WITH_ROWS_TO_CUT)
def test_a_row_array_one_row_short_is_refused(name):
    import re
    v = VIEWS[name]
    for side, (_, arrays) in v["sides"].items():
        for key, _, _ in arrays[1:]:
            ps = [problem(name, 2, 5), problem(name, 3, 6)]
            ps[1][key] = ps[1][key][:-1]
            with pytest.raises(ValueError, match=re.escape(v["short"].format(key=key, rows=4, lead=5))):
                build(name, ps)


def test_a_cell_list_short_of_the_train_rows_is_refused():
    p = _grid_problem(problem("grid", 3))
    p["cells2"] = p["cells2"][:-1]
    with pytest.raises(ValueError, match="one cell list per train row"):
        capi.GridMatchBatchView([p])


def _descriptors(name):
    return [key for _, arrays in VIEWS[name]["sides"].values() for key, cols, dtype in arrays if cols == DB and dtype is U1]


@pytest.mark.parametrize("name", [n for n in NAMES if _descriptors(n)])
def test_desc_bytes_comes_from_a_later_problem_when_the_first_has_no_rows(name):
    v, descs = VIEWS[name], _descriptors(name)
    ps = [problem(name, 0), problem(name, 2, 7)]
    args = v["args"](ps)
    bv = v["cls"](*(args[:1] if name == "frames" else args))      # (FramesBatchView: without its desc_bytes of 8)
    assert bv.desc_bytes == DB
    check_inputs(name, ps, bv)
    ps = [problem(name, 0)]
    for p in ps:
        for key in descs:
            p[key] = np.zeros(0, U1)                              # flat and empty: no width to read
    args = v["args"](ps)
    assert v["cls"](*(args[:1] if name == "frames" else args)).desc_bytes == 32


@pytest.mark.parametrize("name", WITH_OUTPUTS)
def test_results_of_untouched_outputs_are_the_fills_cut_by_the_offsets(name):
    v = VIEWS[name]
    sides = list(v["sides"])
    ps = [problem(name, {s: i % 2 * 2 for i, s in enumerate(sides)}, 8), problem(name, {s: 3 + i for i, s in enumerate(sides)}, 9)]
    bv = build(name, ps)
    res = bv.results(True) if name == "stereo" else bv.results()
    assert len(res) == 2
    for k, (p, r) in enumerate(zip(ps, res)):
        for key, side, trail, dtype, fill in v["out"]:
            if side == "n":
                assert r[key] == fill and isinstance(r[key], int)
            elif side == "2n":
                assert r[key] == (fill, fill)
            else:
                rows = len(p[v["sides"][side][1][0][0]])
                if name == "stereo":
                    rows = 0                                     # n_pt = n_ls = 0: the first none of the side's rows
                got = np.asarray(r[key])
                assert got.dtype == dtype and got.shape == (rows,) + trail, (key, got.shape)
                assert np.isnan(got).all() if fill is NAN else (got == fill).all()
    if name == "stereo":                                         # counts set as a call would: the side's first rows
        bv.o["n_pt"][1], bv.o["n_ls"][1] = 2, 1
        bv.o["pt_src"][int(bv.off["pt_l"][1]):] = np.arange(len(ps[1]["pt_l"]))
        r = bv.results(False)[1]
        assert "ls_NDc" not in r and r["pt_src"].tolist() == [0, 1] and r["ls_src"].tolist() == [-7]
        assert r["pt_P"].shape == (2, 3) and r["ldesc"].shape == (1, DB)
    if name == "frames":
        assert all(r["branch"] == 0 and r["DT"].shape == (4, 4) for r in res)


def test_what_only_some_views_do():
    """float32 stereo coordinates; the broadcast float32 ratio against the grid's float64; a 4x4 Twf; one camera
    per batch; the aliases that callers read."""
    bv = build("stereo", [problem("stereo", 2)])
    assert bv.co["pt_l"].dtype == np.float32 and bv.co["ls_r"].shape == (2, 4) and set(bv.co) == set(bv.desc) == set(bv.off)
    assert bv.desc["ls_l"] is bv.a["ldesc_l"] and bv.co["pt_r"] is bv.a["pt_r"] and bv.n == 1
    m = capi.MatchBatchView([(np.zeros((1, DB), U1), np.zeros((2, DB), U1))] * 3, 0.9)
    assert m.nnr.dtype == np.float32 and m.nnr.tolist() == [np.float32(0.9)] * 3 and m.struct.best_lr == 1
    assert C.cast(m.struct.nnr, C.c_void_p).value == m.nnr.ctypes.data
    m = capi.MatchBatchView([(np.zeros((1, DB), U1), np.zeros((2, DB), U1))] * 2, [0.9, 0.6], False)
    assert m.nnr.tolist() == [np.float32(0.9), np.float32(0.6)] and m.struct.best_lr == 0
    g = build("grid", [problem("grid", 2)])
    assert g.nnr.dtype == np.float64 and g.kind.dtype == g.ws.dtype == np.int32 and (g.struct.cols, g.struct.rows) == (64, 48)
    assert g.cell_off2.tolist() == [0, 1, 2] and C.cast(g.struct.cells2, C.c_void_p).value == g.cells2.ctypes.data
    p = problem("mapassoc", 1)
    T = np.arange(16.0).reshape(4, 4)
    assert capi.MapassocBatchView([dict(p, Twf=T)]).a["Twf"].tolist() == [list(range(12))]
    for name in ("lcpose", "track", "frames"):
        two = VIEWS[name]["args"]([problem(name, 1), problem(name, 1)])[0]
        two[1].cam = (1.0, 2.0, 3.0, 4.0)
        with pytest.raises(ValueError, match="of one batch share one camera"):
            VIEWS[name]["cls"](two)
    f = build("frames", [problem("frames", 2)])
    assert isinstance(f.out_struct, capi.PlbaFramesOut) and isinstance(f.out[0], capi.PlbaTrackOut) and len(f.out) == 1
    assert C.cast(f.out_struct.out, C.c_void_p).value == C.addressof(f.out)
    k = build("kfassoc", [problem("kfassoc", 2)])
    assert isinstance(k.out, capi.PlbaKfassocOut) and set(k.o) == {key for key, *_ in VIEWS["kfassoc"]["out"]}
    with pytest.raises(KeyError):
        capi.KfassocBatchView([{key: a for key, a in problem("kfassoc", 1).items() if key != "DT"}])
