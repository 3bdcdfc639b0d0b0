"""TEST INFRASTRUCTURE: the cases that pin the association front end to the reference's own code, and their
recorded results. compute(api) runs every case through the compiled reference (tests/refpin_api.py) and
returns a flat dict of arrays; tools/make_refpin_golden.py saves that dict as tests/golden/refpin.npz and
golden() loads it. The tests compare the checkers, the host mirror and the device with the recorded arrays,
and, where the library is present, a fresh compute() with the recorded arrays.

Inputs. The cases this module defines (segments, grid queries, hand cases, the nnr = 1.2 case, the device's
problems, the stereo-window frames, the BoW sequences) are stored whole. The parity and boundary cases of
tests/gridmatch_cases.py are regenerated from their seeds instead, and the fixture holds a SHA-256 of their
packed inputs: 30 problems of up to 513 + 130 random 32-byte descriptors are 340 KiB that do not compress,
which with the rest would pass the size of the largest committed fixture. A digest that no longer matches
means the generator changed under the fixture: the test fails and the fixture is to be recorded again.

Only 32-byte descriptors can be pinned: the reference's distance reads exactly eight 32-bit words."""
from __future__ import annotations

import functools
import hashlib
import os

import numpy as np

import bow_cases
import gridmatch_cases as G
import ref_bow
import ref_gridmatch as R
import stereo_cases as SC

COLS, ROWS = G.COLS, G.ROWS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin.npz")
F32, F64 = np.float32, np.float64


# ---- segments for getLineCoords
EDGE_SEGMENTS = [
    # zero length
    (5.5, 5.5, 5.5, 5.5), (0.0, 0.0, 0.0, 0.0), (-0.5, -0.5, -0.5, -0.5), (63.2, 47.9, 63.2, 47.9),
    # horizontal and vertical, both directions of travel
    (2.3, 7.7, 40.1, 7.7), (40.1, 7.7, 2.3, 7.7), (9.2, 3.1, 9.2, 44.6), (9.2, 44.6, 9.2, 3.1),
    # |dy| == |dx| exactly: steep is false
    (1.0, 1.0, 11.0, 11.0), (11.0, 11.0, 1.0, 1.0), (1.0, 11.0, 11.0, 1.0), (11.0, 1.0, 1.0, 11.0),
    (0.25, 3.5, 20.25, 23.5), (20.25, 3.5, 0.25, 23.5), (2.5, 2.5, 2.5 + 7.0, 2.5 - 7.0),
    # half-integer endpoints: error lands on 0 and is not below it
    (0.5, 0.5, 7.5, 3.5), (7.5, 3.5, 0.5, 0.5), (0.5, 0.5, 4.5, 2.5), (1.5, 6.5, 9.5, 2.5), (3.5, 0.5, 5.5, 8.5),
    (0.5, 10.5, 8.5, 12.5), (8.5, 12.5, 0.5, 10.5), (2.5, 1.5, 3.5, 9.5),
    # coordinates in (-1, 0): static_cast<int> truncates toward zero
    (-0.7, -0.3, 5.2, 3.9), (5.2, 3.9, -0.7, -0.3), (-0.9, -0.9, -0.1, -0.1), (-0.2, 5.5, 4.4, -0.6),
    (3.3, -0.99, 3.9, 6.0), (-0.5, -0.5, 0.5, 0.5), (-1.5, -0.25, 2.5, -0.75),
    # endpoints outside the 64 x 48 grid on each side
    (-3.0, 10.2, 10.0, 12.9), (60.1, 10.0, 70.0, 12.0), (10.0, -3.0, 12.5, 10.0), (10.0, 40.0, 12.0, 52.0),
    (-2.5, -2.5, 66.0, 50.0), (66.0, -2.0, -2.0, 50.5),
    # the full diagonals
    (0.0, 0.0, 63.99, 47.99), (63.99, 47.99, 0.0, 0.0), (0.0, 47.99, 63.99, 0.0), (63.99, 0.0, 0.0, 47.99),
    # the contract of plba_stereo_associate, one image size outside the image: the longest walks there are
    (-64.0, -48.0, 128.0, 96.0), (128.0, 96.0, -64.0, -48.0), (-64.0, 96.0, 128.0, -48.0), (-64.0, 10.0, 128.0, 10.5),
    (10.0, -48.0, 10.5, 96.0), (30.0, 96.0, 31.0, -48.0), (-63.99, 5.0, 127.99, 40.0),
]
N_RANDOM = 2400


def segments() -> np.ndarray:
    """[n][4] float64 (x1, y1, x2, y2): the edges, then seeded random segments with endpoints in [-3, 70]:
    a third on half-integers, a third on multiples of 2^-10 (every operation of the walk is exact), a third
    any double; every sixteenth zero-length, horizontal or vertical."""
    rng = np.random.default_rng(20240)
    s = rng.uniform(-3.0, 70.0, (N_RANDOM, 4))
    third = N_RANDOM // 3
    s[:third] = np.floor(s[:third]) + 0.5
    s[third:2 * third] = np.round(s[third:2 * third] * 1024.0) / 1024.0
    for i in range(0, N_RANDOM, 16):
        how = (i // 16) % 3
        if how == 0:
            s[i, 2:] = s[i, :2]
        elif how == 1:
            s[i, 3] = s[i, 1]
        else:
            s[i, 2] = s[i, 0]
    return np.concatenate([np.array(EDGE_SEGMENTS, F64), s])


N_CONTRACT_EDGES = 7            # the last edges: inside plba_stereo_associate's coordinate contract
MAX_STEPS = 3 * max(COLS, ROWS) + 1


def csr(lists, width):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in lists])
    flat = np.concatenate([np.asarray(c, np.int32).reshape(-1, width) for c in lists]) if len(lists) else \
        np.zeros((0, width), np.int32)
    return off, flat.astype(np.int32)


def uncsr(off, flat):
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


# ---- problems of matchGrid, packed into arrays and back
def pack(pb) -> dict:
    n1, n2 = len(pb["desc1"]), len(pb["desc2"])
    off, flat = csr([np.asarray(c, np.int32).reshape(-1, 2) for c in pb["cells2"]], 2)
    line = pb["kind"] == 1
    return dict(scal=np.array([pb["kind"], pb["ws"], pb["nnr"], pb["line_sim_th"]], F64),
                desc1=np.ascontiguousarray(pb["desc1"], np.uint8).reshape(n1, 32),
                desc2=np.ascontiguousarray(pb["desc2"], np.uint8).reshape(n2, 32),
                cell1=np.asarray(pb["cell1"], np.int32).reshape(n1, 2),
                cell1_end=np.asarray(pb["cell1_end"], np.int32).reshape(n1, 2) if line else np.zeros((0, 2), np.int32),
                cell_off2=off, cells2=flat,
                dir2=np.asarray(pb["dir2"], F64).reshape(n2, 2) if line else np.zeros((0, 2), F64))


def unpack(a) -> dict:
    kind, ws, nnr, th = a["scal"]
    line = int(kind) == 1
    return dict(kind=int(kind), ws=int(ws), nnr=float(nnr), line_sim_th=float(th), desc1=a["desc1"], desc2=a["desc2"],
                cell1=a["cell1"], cell1_end=a["cell1_end"] if line else None, cells2=uncsr(a["cell_off2"], a["cells2"]),
                dir2=a["dir2"] if line else None)


def digest(pb) -> np.ndarray:
    h = hashlib.sha256()
    for k, v in sorted(pack(pb).items()):
        h.update(k.encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def base_cases():
    """tests/gridmatch_cases.py's parity and boundary cases at desc_bytes = 32."""
    return [c for c in G.parity_cases() + G.boundary_cases() if c[3] == 32]


def base_name(c):
    return "base_" + "_".join(str(v) for v in c)


def _two_in_a_cell(d_first, d_second, nnr, n_query=1):
    """Point queries in cell (5, 5) and two train rows there at Hamming distances d_first and d_second."""
    return dict(kind=0, ws=1, nnr=nnr, line_sim_th=0.75, desc1=np.zeros((n_query, 32), np.uint8),
                cell1=np.tile(np.array([[5, 5]], np.int32), (n_query, 1)), cell1_end=None,
                desc2=np.array([SC.bits_desc(*range(d_first)), SC.bits_desc(*range(100, 100 + d_second))]),
                cells2=[np.array([[5, 5]], np.int32), np.array([[6, 4]], np.int32)], dir2=None)


NNR_06F = float(F32(0.6))       # 0.6f widened: 0.60000002384185791015625


def _line_sim(th):
    """One query line from cell (10, 10) to (13, 14), v = (3, 4) / 5, and a train line of direction (1, 0) in
    its window: dot = v[0], the double nearest 0.6."""
    t = SC.bits_desc(0, 1, 2)
    return dict(kind=1, ws=1, nnr=0.9, line_sim_th=th, desc1=np.zeros((1, 32), np.uint8),
                cell1=np.array([[10, 10]], np.int32), cell1_end=np.array([[13, 14]], np.int32), desc2=t[None, :],
                cells2=[np.array([[10, 10], [11, 10]], np.int32)], dir2=np.array([[1.0, 0.0]]))


V0 = float(F64(3.0) / np.sqrt(F64(25.0)))   # what normalize gives for (3, 4)


def hand_cases() -> dict:
    q2 = _two_in_a_cell(3, 100, 1.5, n_query=2)
    q2 = dict(q2, desc2=q2["desc2"][:1], cells2=q2["cells2"][:1])
    nan_line = dict(kind=1, ws=1, nnr=0.9, line_sim_th=0.75, desc1=np.zeros((2, 32), np.uint8),
                    cell1=np.array([[10, 10], [30, 30]], np.int32), cell1_end=np.array([[10, 10], [30, 33]], np.int32),
                    desc2=np.array([SC.bits_desc(0, 1, 2), SC.bits_desc(5)]),
                    cells2=[np.array([[10, 10]], np.int32), np.array([[30, 30], [31, 30]], np.int32)],
                    dir2=np.array([[1.0, 0.0], [1.0, 0.0]]))
    return {
        # the ratio test on the double-precision boundary: 6 < 10 * 0.6 is false in double (the product
        # rounds to 6.0), 6 < 10 * (double)0.6f is true
        "ratio_06": _two_in_a_cell(6, 10, 0.6),
        "ratio_06f": _two_in_a_cell(6, 10, NNR_06F),
        # |dot| one ulp either side of line_sim_th: rejected only when strictly below
        "sim_below": _line_sim(float(np.nextafter(V0, 0.0))),
        "sim_equal": _line_sim(V0),
        "sim_above": _line_sim(float(np.nextafter(V0, 1.0))),
        # the three places where the checker pins what the reference leaves open
        "order_tie": _two_in_a_cell(4, 4, 1.5),        # two candidates tie at the minimum above nnr = 1
        "nan_direction": nan_line,                     # row 0: a zero-length query line; row 1: a real rejection
        "no_seen_pair": q2,                            # two equal queries, one train row, nnr = 1.5
    }


def nnr12_case():
    """nnr = 1.2 over the generator's problem. Its exact-copy distractors tie at the minimum of every query that
    sees both; two thirds of them get one bit flipped, which leaves ties on fewer than a tenth of the rows."""
    pb = G.make(0, 220, 140, 32, 3, 1.2, seed=11)
    desc2 = pb["desc2"].copy()
    for j in range(15, len(desc2), 16):
        if (j // 16) % 3:
            desc2[j, 0] ^= 1
    return dict(pb, desc2=desc2)


# (kind, n1, n2, ws, nnr, seed): n1, n2 <= 300, every ws of {0, 1, 12} for both kinds
DEVICE_PROBLEMS = [(0, 300, 200, 0, 0.9, 21), (0, 257, 130, 1, 0.75, 22), (0, 150, 65, 12, 0.9, 23),
                   (1, 300, 200, 12, 0.9, 24), (1, 90, 65, 0, 0.75, 25), (1, 130, 257, 1, 0.9, 26)]


def device_problem(k):
    kind, n1, n2, ws, nnr, seed = DEVICE_PROBLEMS[k]
    return G.make(kind, n1, n2, 32, ws, nnr, seed)


def stored_problems() -> dict:
    out = dict(hand_cases())
    out["nnr12"] = nnr12_case()
    for k in range(len(DEVICE_PROBLEMS)):
        out[f"device{k}"] = device_problem(k)
    return out


# ---- the stereo window: frames in pixels, as plba_stereo_associate takes them
def stereo_frame():
    rng = np.random.default_rng(77)
    f = SC.points(rng, 120, 100)
    f.update(SC.lines(rng, 60, 64, outside=True))
    return f


OPEN_GATES = dict(max_dist_epip=1e300, min_disp=-1e300, ls_min_disp_ratio=-1e300, line_horiz_th=-1.0,
                  stereo_overlap_th=-1.0)


def stereo_cell(v, inv):
    return int(F64(v) * inv)    # kp.pt.x * inv_width into a pair<int, int>: float times double, truncated


def stereo_problems(frame, api, window):
    """The two matchGrid problems of a frame as src2/stereoFrame.cpp:131-147 and :318-346 set them up: the
    right lines rasterised by the reference's getLineCoords and their directions by its normalize."""
    inv_w, inv_h = COLS / F64(SC.WIDTH), ROWS / F64(SC.HEIGHT)
    pl, pr, ll, lr = frame["pt_l"], frame["pt_r"], frame["ls_l"], frame["ls_r"]
    pts = dict(kind=0, ws=window[0], nnr=0.9, line_sim_th=0.75, desc1=frame["pdesc_l"], desc2=frame["pdesc_r"],
               cell1=np.array([(stereo_cell(p[0], inv_w), stereo_cell(p[1], inv_h)) for p in pl], np.int32),
               cell1_end=None, dir2=None,
               cells2=[np.array([(stereo_cell(p[0], inv_w), stereo_cell(p[1], inv_h))], np.int32) for p in pr])
    lns = dict(kind=1, ws=window[0], nnr=0.9, line_sim_th=0.75, desc1=frame["ldesc_l"], desc2=frame["ldesc_r"],
               cell1=np.array([(stereo_cell(s[0], inv_w), stereo_cell(s[1], inv_h)) for s in ll], np.int32),
               cell1_end=np.array([(stereo_cell(s[2], inv_w), stereo_cell(s[3], inv_h)) for s in ll], np.int32),
               cells2=[api.line_coords(F64(s[0]) * inv_w, F64(s[1]) * inv_h, F64(s[2]) * inv_w, F64(s[3]) * inv_h) for s in lr],
               dir2=np.array([api.normalize(F64(s[2] - s[0]) * inv_w, F64(s[3] - s[1]) * inv_h) for s in lr]))
    return pts, lns


def stereo_case_lines():
    """(case name, row) and the grid coordinates of every right-image line of tests/stereo_cases.py."""
    inv_w, inv_h = COLS / F64(SC.WIDTH), ROWS / F64(SC.HEIGHT)
    out = []
    for name in SC.CASES:
        for s in np.asarray(SC.case(name).get("ls_r", np.zeros((0, 4))), F32).reshape(-1, 4):
            out.append((F64(s[0]) * inv_w, F64(s[1]) * inv_h, F64(s[2]) * inv_w, F64(s[3]) * inv_h))
    return np.array(out, F64).reshape(-1, 4)


# ---- GridStructure::get
GET_QUERIES = [(0, 0), (63, 0), (0, 47), (63, 47), (-1, -1), (64, 48), (-5, 20), (70, 20), (20, -13), (20, 60),
               (-12, 10), (75, 47), (32, 24), (1, 46), (62, 1)]


def get_windows(stereo_window):
    return [(0, 0, 0, 0), (1, 1, 1, 1), (12, 12, 12, 12), tuple(int(v) for v in stereo_window)]


def get_fill():
    """The cell lists of a line problem: rows in several cells, cells outside the grid, a cell listed twice."""
    cells2 = [np.array(c, np.int32) for c in G.problem(1, 300, 200, 32, 3, 0.9, 0)["cells2"]]
    cells2[3] = np.concatenate([cells2[3], cells2[3][:1], np.array([[-1, 5], [64, 47], [0, 48]], np.int32)])
    for i, (x, y) in enumerate([(0, 0), (63, 0), (0, 47), (63, 47)]):
        cells2[10 + i] = np.array([[x, y]], np.int32)
    return cells2


# ---- BowVector
BOW_N_DESC = [1, 2, 63, 65, 257]


def bow_sequence(voc, desc):
    """The addWeight calls of the transform (TemplatedVocabulary.h:1046-1084) for these descriptors: the
    checker's descent picks the words; a word of weight 0 is not added."""
    ids, vals = [], []
    for d in np.asarray(desc, np.uint8).reshape(-1, voc["node_desc"].shape[1]):
        leaf, _ = ref_bow.descend(voc, d)
        w = float(voc["weight"][leaf])
        if w > 0:
            ids.append(int(voc["word_id"][leaf]))
            vals.append(w)
    return np.array(ids, np.uint32), np.array(vals, F64)


def bow_sequences() -> dict:
    out = {}
    for count in (6, 10):
        out[f"sum{count}"] = bow_sequence(*bow_cases.sum_case(count))
    for name in bow_cases.VOCABS:
        for n in BOW_N_DESC + ([600] if name == "k10L3" else []):
            out[f"{name}_{n}"] = bow_sequence(bow_cases.vocab(name), bow_cases.descriptors(name, n))
    return out


IF_NOT_EXIST = (np.array([7, 3, 7, 9, 3, 1, 9], np.uint32), np.array([0.5, 0.25, 4.0, 1.0, 8.0, 2.0, 0.125]),
                np.array([0, 1, 1, 0, 0, 1, 0], np.uint8))   # 1: addIfNotExist, 0: addWeight


# ---- everything through the reference
def compute(api, stereo_window) -> dict:
    out = {"stereo_window": np.asarray(stereo_window, np.int32)}
    seg = segments()
    out["seg"] = seg
    out["seg_off"], cells = csr([api.line_coords(*s) for s in seg], 2)
    out["seg_cells"] = cells.astype(np.int16)            # |coordinate| <= 128
    assert np.array_equal(out["seg_cells"], cells)
    sl = stereo_case_lines()
    out["stereo_lines"] = sl
    out["stereo_lines_off"], out["stereo_lines_cells"] = csr([api.line_coords(*s) for s in sl], 2)

    fill = get_fill()
    out["get_fill_off"], out["get_fill_cells"] = csr(fill, 2)
    with api.Grid(fill, COLS, ROWS) as g:
        got = [g.get(x, y, w) for w in get_windows(stereo_window) for (x, y) in GET_QUERIES]
    out["get_off"], out["get_idx"] = csr([np.array(v, np.int32).reshape(-1, 1) for v in got], 1)

    def run(name, pb, w=None):
        for lr in (0, 1):
            m12, cnt = api.match_grid(pb, COLS, ROWS, bool(lr), w)
            out[f"mg_{name}_lr{lr}"] = np.append(m12, np.int32(cnt)).astype(np.int32)   # matches_12, then the count
    for c in base_cases():
        pb = G.problem(*c)
        out[f"mg_{base_name(c)}_digest"] = digest(pb)
        run(base_name(c), pb)
    for name, pb in stored_problems().items():
        for k, v in pack(pb).items():
            out[f"pb_{name}_{k}"] = v
        run(name, pb)
    frame = stereo_frame()
    for k, v in frame.items():
        out[f"stereo_frame_{k}"] = v
    for name, pb in zip(("stereo_pts", "stereo_lns"), stereo_problems(frame, api, stereo_window)):
        for k, v in pack(pb).items():
            out[f"pb_{name}_{k}"] = v
        run(name, pb, stereo_window)

    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 256, (64, 32), dtype=np.uint8), rng.integers(0, 256, (64, 32), dtype=np.uint8)
    a[0], b[0], a[1], b[1] = 0, 255, 0, 0
    a[1, 3] = 0x80                                 # row 0: all bits; row 1: the sign bit of a word
    out["dist_a"], out["dist_b"] = a, b
    out["dist"] = np.array([api.distance(x, y) for x, y in zip(a, b)], np.int32)

    seqs = bow_sequences()
    raw, fin = [api.bow(i, v, normalize_l1=False) for i, v in seqs.values()], [api.bow(i, v) for i, v in seqs.values()]
    assert all(np.array_equal(r[0], f[0]) for r, f in zip(raw, fin))
    out["bow_in_off"], out["bow_in_ids"] = csr([i.astype(np.int64).reshape(-1, 1) for i, _ in seqs.values()], 1)
    out["bow_in_vals"] = np.concatenate([v for _, v in seqs.values()])
    out["bow_off"], out["bow_ids"] = csr([r[0].astype(np.int64).reshape(-1, 1) for r in raw], 1)
    out["bow_raw_vals"], out["bow_vals"] = np.concatenate([r[1] for r in raw]), np.concatenate([f[1] for f in fin])
    out["bow_ifne_ids"], out["bow_ifne_vals"] = api.bow(*IF_NOT_EXIST[:2], normalize_l1=False, if_not_exist=IF_NOT_EXIST[2])
    return out


@functools.lru_cache(maxsize=None)
def golden() -> dict:
    with np.load(GOLDEN) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def stored_problem(name) -> dict:
    g = golden()
    return unpack({k: g[f"pb_{name}_{k}"] for k in ("scal", "desc1", "desc2", "cell1", "cell1_end", "cell_off2", "cells2", "dir2")})


def recorded(name, best_lr):
    a = golden()[f"mg_{name}_lr{int(best_lr)}"]
    return a[:-1], int(a[-1])


# ---- what the equality rules need from the checker's distance matrix
def seen_pairs(pb, best_lr, w=None):
    """(window [n1][n2]: i2 is in the set that GridStructure::get returns for row i1; seen [n1][n2]: the pair
    reaches the best / second-best update; D): from the cell lists and the checker's Hamming distances alone."""
    import ref_stereo as RS
    n1, n2 = len(pb["desc1"]), len(pb["desc2"])
    w = tuple([int(pb["ws"])] * 4 if w is None else w)
    grid = RS.WindowGrid(ROWS, COLS)
    for idx, cells in enumerate(pb["cells2"]):
        for x, y in np.asarray(cells, np.int64).reshape(-1, 2):
            grid.add(int(x), int(y), idx)
    window = np.zeros((n1, n2), bool)
    for i1 in range(n1):
        s = set()
        grid.get4(int(pb["cell1"][i1][0]), int(pb["cell1"][i1][1]), w, s)
        if pb["kind"] == 1:
            grid.get4(int(pb["cell1_end"][i1][0]), int(pb["cell1_end"][i1][1]), w, s)
        window[i1, sorted(s)] = True
    cand = window.copy()
    if pb["kind"] == 1 and n1 and n2:
        d2 = np.asarray(pb["dir2"], F64).reshape(n2, 2)
        for i1 in range(n1):
            v = R.normalize(int(pb["cell1_end"][i1][0]) - int(pb["cell1"][i1][0]),
                            int(pb["cell1_end"][i1][1]) - int(pb["cell1"][i1][1]))
            with np.errstate(invalid="ignore"):
                cand[i1] &= ~(np.abs(v[0] * d2[:, 0] + v[1] * d2[:, 1]) < pb["line_sim_th"])
    d1, d2 = np.asarray(pb["desc1"], np.uint8), np.asarray(pb["desc2"], np.uint8)
    D = np.unpackbits(d1[:, None, :] ^ d2[None, :, :], axis=2).sum(axis=2).astype(np.int64) if n1 and n2 else \
        np.zeros((n1, n2), np.int64)
    seen = cand
    if best_lr and n1 and n2:
        big = np.where(cand, D, R.INT_MAX)
        before = np.vstack([np.full((1, n2), R.INT_MAX, np.int64), np.minimum.accumulate(big, axis=0)[:-1]])
        seen = cand & (D < before)
    return window, seen, D


def tie_rows(pb, best_lr, w=None) -> np.ndarray:
    """bool [n1]: two seen candidates tie at the row's minimum seen distance. Above nnr = 1 such a row is
    matched to whichever the reference's unordered_set yields first; every other row is order-free."""
    _, seen, D = seen_pairs(pb, best_lr, w)
    if seen.shape[1] == 0:
        return np.zeros(seen.shape[0], bool)
    big = np.where(seen, D, R.INT_MAX)
    mn = big.min(axis=1)
    return (mn < R.INT_MAX) & ((big == mn[:, None]).sum(axis=1) >= 2)


def phantom_rows(pb, best_lr, w=None) -> np.ndarray:
    """bool [n1]: the window holds a train row and no pair is seen. Above nnr = 1 the reference's ratio test
    INT_MAX < INT_MAX * nnr passes there: it counts a match and leaves the index at -1."""
    window, seen, _ = seen_pairs(pb, best_lr, w)
    return window.any(axis=1) & ~seen.any(axis=1)


def recorded_bow(name):
    """(input ids, input values, ids in map order, accumulated values, normalised values) of a sequence."""
    g, k = golden(), list(bow_sequences()).index(name)
    a, b = g["bow_in_off"][k:k + 2]
    c, d = g["bow_off"][k:k + 2]
    return g["bow_in_ids"][a:b, 0], g["bow_in_vals"][a:b], g["bow_ids"][c:d, 0], g["bow_raw_vals"][c:d], g["bow_vals"][c:d]


def assert_same_matches(got, ref, pb, best_lr, w=None):
    """got = (matches_12, count) of a checker, the host mirror or the device; ref = the reference's. Below
    nnr = 1 everything is equal. Above it the rows of tie_rows are free (with best_lr the cross-check may
    then keep one choice and drop the other), and the reference's count includes the phantom rows."""
    m12, cnt = np.asarray(got[0]), int(got[1])
    ref_m12, ref_cnt = np.asarray(ref[0]), int(ref[1])
    assert m12.shape == ref_m12.shape and m12.dtype == np.int32
    if pb["nnr"] < 1.0:
        assert np.array_equal(m12, ref_m12), np.flatnonzero(m12 != ref_m12)[:10]
        assert cnt == ref_cnt
        return
    free, phantom = tie_rows(pb, best_lr, w), int(phantom_rows(pb, best_lr, w).sum())
    assert np.array_equal(m12[~free], ref_m12[~free]), np.flatnonzero((m12 != ref_m12) & ~free)[:10]
    assert ref_cnt - phantom == int((ref_m12 >= 0).sum())
    assert cnt == int((m12 >= 0).sum())
    if not free.any():
        assert cnt == ref_cnt - phantom
