"""The zero-pivot matrix of tests/zero_pivot_cases.py on the CPU: what the GPU tests take for
granted. The checker alone must show, for every (window, row), that a zero-information keyframe at
lambda = 0 fails every solve of the Huber stage (one iteration, maxTrials = 10 rejected trials,
Terminate, nothing moved); the structure written in the table must be the window's; and the
planner must pick, for that structure and those switches, the factorisation the case is there
for, so that the matrix keeps one entry for each of the eight."""
import ctypes
import os

import numpy as np
import pytest

import graph_mut as gm
import zero_pivot_cases as zc
from plba import lib, synth


@pytest.mark.parametrize("name,row", zc.window_rows(), ids=lambda v: str(v))
def test_checker_rejects_every_trial(name, row):
    g = zc.zero_window(name, row)
    ref = zc.zero_oracle_gn(name, row)
    tr = ref["trace"]
    assert len(tr) == 1 and tr[0]["trials"] == 10 and tr[0]["result"] == 1, tr
    assert ref["iters"][0] == 1
    assert tr[0]["lambda_start"] == 0.0 and tr[0]["lambda_end"] == 0.0
    np.testing.assert_array_equal(ref["kf_Tcw"], g.kf_Tcw)
    np.testing.assert_array_equal(ref["pt_xyz"], g.pt_xyz)
    np.testing.assert_array_equal(ref["ln_orth"], g.ln_orth)


def test_no_entry_is_left_out():
    # every row of every case is a row of its window, and each has its checker run above
    assert len(zc.CASES) == len(zc.BY_ID) == 17
    for c in zc.CASES:
        assert c.rows and all(0 <= r < c.nf for r in c.rows), c
    assert {(c.window, r) for c in zc.CASES for r in c.rows} == set(zc.window_rows())


@pytest.mark.parametrize("cid", [c.id for c in zc.CASES])
def test_table_structure_is_the_windows(cid):
    c = zc.BY_ID[cid]
    assert zc.structure(zc.window(c.window)) == (c.nf, c.bw)
    # Ω = 0 changes no structure
    assert zc.structure(zc.zero_window(c.window, c.rows[-1])) == (c.nf, c.bw)
    # no reordering: row r of the table is row r of the factorisation
    assert c.bw <= 9 or c.env.get("PLBA_NO_RCM") == "1", c


def test_rows_are_the_intended_ones():
    by = zc.BY_ID
    assert by["cl-bw9"].rows == (0, 1, 9, 3, 12)
    # 43 free poses, bw 4: m = 20 rows top-down, separator rows 20..23, rows 42..24 bottom-up
    assert by["cltw-bw4"].rows == by["bandtw-bw4"].rows == (0, 19, 20, 23, 24, 42)
    assert by["bandtw-bw11"].rows == (0, 21, 22, 32, 33, 53)
    assert by["band-full"].rows == (0, 1, 12, 13)          # bw = nf-1: nf-1-bw is row 0
    assert by["band-bw21"].rows == (0, 1, 5, 25, 26)
    # super-rows of bw rows: 0, 1, 2, 4, the last one (partial at nf 27 / bw 2 and nf 58 / bw 7)
    assert by["bcr-bw2"].rows == by["bcr-bw2-split"].rows == (1, 2, 5, 9, 26)
    assert by["bcr-bw4"].rows == (2, 4, 11, 19, 32, 35)
    assert by["bcr-bw7"].rows == (3, 7, 20, 34, 56, 57)
    assert 27 % 2 and 58 % 7
    assert by["dense-mfma"].rows == (0, 5, 10, 11, 26)


def _plan(monkeypatch, bw, nf, env):
    for k in [k for k in os.environ if k.startswith("PLBA_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = (ctypes.c_int32 * 9)(*([-99] * 9))
    # 256 resident workgroups (more than any window's super-rows), a window with Schur triples
    assert lib.load().plba_factor_plan(bw, nf, 256, 4, out, 9) == 0
    return tuple(out)


def test_planner_covers_every_factorisation(monkeypatch):
    seen = set()
    for c in zc.CASES:
        p = _plan(monkeypatch, c.bw, c.nf, c.env)
        assert p[0] == c.mode, (c.id, p)
        if c.mode == zc.BCR:
            assert p[1] == c.stats["bcr_rows"] and p[2] == c.fused, (c.id, p)
        if c.mode in (zc.BAND_TW, zc.CL_TW):
            assert p[3] == zc.tw_split(c.nf, c.bw), (c.id, p)
        seen.add((p[0], p[2]))
    assert seen == zc.ALL_MODES, seen ^ zc.ALL_MODES


def test_planner_keeps_the_idle_windows_on_their_path(monkeypatch):
    """The idle pose widens the envelope it sits in; each idle window must still be planned onto
    the factorisation of its entry, and its boundary row must exist."""
    for cid, kind in zc.idle_cases():
        c = zc.IDLE_BY_ID[cid]
        r, nf, bw = zc.idle_row(cid, kind)
        assert bw <= 9 or c.env.get("PLBA_NO_RCM") == "1", (cid, kind, bw)
        p = _plan(monkeypatch, bw, nf, c.env)
        st = c.stats
        assert (p[0] >= zc.BAND) == bool(st["banded"]), (cid, kind, p)
        if "column_lane" in st:
            assert (p[0] in (zc.CL, zc.CL_TW)) == bool(st["column_lane"]), (cid, kind, p)
        if "twisted" in st:
            assert (p[0] in (zc.BAND_TW, zc.CL_TW)) == bool(st["twisted"]), (cid, kind, p)
        if "bcr_fused" in st:
            assert p[0] == zc.BCR and p[2] == st["bcr_fused"], (cid, kind, p)
        if "dense_mfma" in st:
            assert (p[0] == zc.DENSE_MFMA) == bool(st["dense_mfma"]), (cid, kind, p)


# ---- the row argument of the two mutations
def test_row_argument_places_the_keyframe():
    g = synth.generate("C1L", track_min=3, seed=41)
    rows = gm.free_rows(g)
    for r in (0, 3, len(rows) - 1, -1, -len(rows)):
        z = gm.zero_information_keyframe(g, row=r)
        k = rows[r]
        assert (z.ept_info[g.ept_kf == k] == 0).all() and (z.eln_info[g.eln_kf == k] == 0).all()
        np.testing.assert_array_equal(z.ept_info[g.ept_kf != k], g.ept_info[g.ept_kf != k])
        np.testing.assert_array_equal(z.eln_info[g.eln_kf != k], g.eln_info[g.eln_kf != k])
    # scrambled ids: rows follow kf_id, not array order
    h = gm.shuffled(g, seed=3)
    hr = gm.free_rows(h)
    assert (np.diff(h.kf_id[hr]) > 0).all() and (h.kf_fixed[hr] == 0).all()
    z = gm.zero_information_keyframe(h, row=2)
    assert set(h.ept_kf[z.ept_info == 0]) == {hr[2]}


def test_defaults_are_unchanged():
    g = synth.generate("C1L", track_min=3, seed=41)
    z = gm.zero_information_keyframe(g)
    free = np.nonzero(g.kf_fixed == 0)[0]
    k = free[len(free) // 2]
    np.testing.assert_array_equal(z.ept_info, np.where(g.ept_kf == k, 0.0, g.ept_info))
    np.testing.assert_array_equal(z.eln_info, np.where(g.eln_kf == k, 0.0, g.eln_info))
    h = gm.add_idle_free_pose(g)
    assert h.kf_id[-1] == g.kf_id.max() + 1 and h.kf_fixed[-1] == 0
    np.testing.assert_array_equal(h.kf_id[:-1], g.kf_id)
    np.testing.assert_array_equal(h.pt_id, g.pt_id)
    np.testing.assert_array_equal(h.ln_id, g.ln_id)
    np.testing.assert_array_equal(h.kf_Tcw[-1], g.kf_Tcw[-1])


def test_idle_pose_row_shifts_the_ids_above_it():
    g = synth.generate("C1L", track_min=3, seed=41)
    nf = len(gm.free_rows(g))
    for r in (0, 4, nf, -1, -(nf + 1)):
        h = gm.add_idle_free_pose(g, row=r)
        hr = gm.free_rows(h)
        want = r + nf + 1 if r < 0 else r
        assert len(hr) == nf + 1 and hr[want] == h.n_kf - 1, (r, hr)
        # the other free poses keep their order, every vertex id stays unique, no edge moved
        np.testing.assert_array_equal(np.delete(hr, want), gm.free_rows(g))
        ids = np.concatenate([h.kf_id, h.pt_id, h.ln_id])
        assert len(np.unique(ids)) == len(ids)
        assert (np.diff(h.pt_id) > 0).all() and (np.diff(h.ln_id) > 0).all() and h.pt_id.max() < h.ln_id.min()
        np.testing.assert_array_equal(h.ept_kf, g.ept_kf)
        assert h.kf_id.dtype == g.kf_id.dtype and h.pt_id.dtype == g.pt_id.dtype
        assert not (h.ept_kf == h.n_kf - 1).any() and not (h.eln_kf == h.n_kf - 1).any()
