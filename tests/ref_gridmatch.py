"""Checker of plba_grid_match: a literal restatement of both StVO::matchGrid overloads
(src2/matching.cpp:111-258) with GridStructure (src2/gridStructure.cpp:43-76) as a real grid of lists,
a set of candidates per query and the sequential `distances` / `matches_21` arrays; of getLineCoords /
LineIterator (src2/lineIterator.cpp); and the parallel formulation the kernels rely on.

Pinned where the reference leaves it open or undefined:
  * the candidates of a query are iterated in increasing i2 (the reference iterates an unordered_set);
  * normalize() of a zero vector gives NaN, `abs(dot) < th` is then false and the candidate is kept;
  * a row with candidates but no seen pair (best_d = INT_MAX) is unmatched whatever nnr is (above
    nnr = 1 the reference counts a match with index -1).
Each of the three is confirmed on the compiled reference (tests/test_refpin.py, test_divergence_*): the set's
order shows only where two seen candidates tie at a row's minimum above nnr = 1; the reference keeps the
NaN candidate too; and it does return a count that includes rows left at -1.

Pinned to the reference's own code (oracle/refpin compiles src2/lineIterator.cpp, gridStructure.cpp and
matching.cpp in place; tests/golden/refpin.npz records their outputs; tests/test_refpin.py compares, for
equality): line_cells against getLineCoords; Grid.get and candidates_and_distances against
GridStructure::get under symmetric windows and, through ref_stereo.WindowGrid, the stereo window;
hamming_row against distance; match_grid against both matchGrid overloads at 32-byte descriptors (distance
reads eight 32-bit words whatever the width, so no other width can be pinned). Still a restatement with
no reference run behind it: match / matchNNR (tests/ref_descmatch.py; they need OpenCV's BFMatcher).

A problem is a dict: kind (0 points, 1 lines), ws, nnr, line_sim_th, desc1 [n1][B] uint8, cell1 [n1][2],
cell1_end [n1][2] (lines), desc2 [n2][B], cells2 (a list of [k][2] int arrays, one per train row),
dir2 [n2][2] (lines)."""
import numpy as np

INT_MAX = 2 ** 31 - 1
NONE_KEY = 0xFFFFFFFF


def line_cells(x1, y1, x2, y2):
    """getLineCoords(x1, y1, x2, y2): LineIterator's cells in its order."""
    x1, y1, x2, y2 = float(x1), float(y1), float(x2), float(y2)
    steep = abs(y2 - y1) > abs(x2 - x1)
    if steep:
        x1, y1 = y1, x1
        x2, y2 = y2, x2
    if x1 > x2:
        x1, x2 = x2, x1
        y1, y2 = y2, y1
    dx = x2 - x1
    dy = abs(y2 - y1)
    error = dx / 2.0
    ystep = 1 if y1 < y2 else -1
    x, y, max_x = int(x1), int(y1), int(x2)   # static_cast<int>: toward zero
    out = []
    while x <= max_x:
        out.append((y, x) if steep else (x, y))
        error -= dy
        if error < 0:
            y += ystep
            error += dx
        x += 1
    return out


def hamming_row(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def normalize(vx, vy):
    """include2/matching.h:43-48 in double; (0, 0) gives (NaN, NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        vx, vy = np.float64(vx), np.float64(vy)
        mag = np.sqrt(vx * vx + vy * vy)
        return vx / mag, vy / mag


class Grid:
    def __init__(self, rows, cols):
        self.rows, self.cols = rows, cols
        self.grid = [[[] for _ in range(rows)] for _ in range(cols)]

    def add(self, x, y, idx):   # grid.at(x, y).push_back(idx); out of bounds goes nowhere
        if 0 <= x < self.cols and 0 <= y < self.rows:
            self.grid[x][y].append(idx)

    def get(self, x, y, ws, indices):
        for x_ in range(max(0, x - ws), min(self.cols, x + ws + 1)):
            for y_ in range(max(0, y - ws), min(self.rows, y + ws + 1)):
                indices.update(self.grid[x_][y_])


def fill_grid(pb, cols, rows):
    grid = Grid(rows, cols)
    for idx, cells in enumerate(pb["cells2"]):
        for x, y in np.asarray(cells, np.int64).reshape(-1, 2):
            grid.add(int(x), int(y), idx)
    return grid


def match_grid(pb, cols=64, rows=48, best_lr=True):
    """(matches_12 int32 [n1], matches): matchGrid, points or lines by pb['kind']."""
    desc1, desc2 = pb["desc1"], pb["desc2"]
    n1, n2 = len(desc1), len(desc2)
    line, ws, nnr = pb["kind"] == 1, int(pb["ws"]), float(pb["nnr"])
    grid = fill_grid(pb, cols, rows)
    matches = 0
    matches_12 = [-1] * n1
    matches_21 = [-1] * n2
    distances = [INT_MAX] * n2
    for i1 in range(n1):
        best_d, best_d2, best_idx = INT_MAX, INT_MAX, -1
        sx, sy = (int(v) for v in pb["cell1"][i1])
        candidates = set()
        grid.get(sx, sy, ws, candidates)
        if line:
            ex, ey = (int(v) for v in pb["cell1_end"][i1])
            v = normalize(ex - sx, ey - sy)
            grid.get(ex, ey, ws, candidates)
        if not candidates:
            continue
        for i2 in sorted(candidates):
            if line:
                with np.errstate(invalid="ignore"):
                    dot = v[0] * np.float64(pb["dir2"][i2][0]) + v[1] * np.float64(pb["dir2"][i2][1])
                    if abs(dot) < pb["line_sim_th"]:
                        continue
            d = hamming_row(desc1[i1], desc2[i2])
            if best_lr:
                if d < distances[i2]:
                    distances[i2] = d
                    matches_21[i2] = i1
                else:
                    continue
            if d < best_d:
                best_d2, best_d, best_idx = best_d, d, i2
            elif d < best_d2:
                best_d2 = d
        if best_idx >= 0 and float(best_d) < float(best_d2) * nnr:
            matches_12[i1] = best_idx
            matches += 1
    if best_lr:
        for i1 in range(n1):
            i2 = matches_12[i1]
            if i2 >= 0 and matches_21[i2] != i1:
                matches_12[i1] = -1
                matches -= 1
    return np.asarray(matches_12, np.int32).reshape(n1), matches


def candidates_and_distances(pb, cols=64, rows=48):
    """cand [n1][n2] bool and the Hamming distances [n1][n2], from the cell lists alone."""
    desc1, desc2 = np.asarray(pb["desc1"], np.uint8), np.asarray(pb["desc2"], np.uint8)
    n1, n2 = len(desc1), len(desc2)
    ws, line = int(pb["ws"]), pb["kind"] == 1
    occ = np.zeros((n2, cols, rows), bool)
    for i2, cells in enumerate(pb["cells2"]):
        c = np.asarray(cells, np.int64).reshape(-1, 2)
        c = c[(c[:, 0] >= 0) & (c[:, 0] < cols) & (c[:, 1] >= 0) & (c[:, 1] < rows)]
        occ[i2, c[:, 0], c[:, 1]] = True
    cand = np.zeros((n1, n2), bool)
    for i1 in range(n1):
        qs = [pb["cell1"][i1]] + ([pb["cell1_end"][i1]] if line else [])
        for x, y in qs:
            x, y = int(x), int(y)
            w = occ[:, max(0, x - ws):max(0, min(cols, x + ws + 1)), max(0, y - ws):max(0, min(rows, y + ws + 1))]
            cand[i1] |= w.reshape(n2, -1).any(axis=1)
        if line and n2:
            sx, sy = (int(v) for v in pb["cell1"][i1])
            ex, ey = (int(v) for v in pb["cell1_end"][i1])
            v = normalize(ex - sx, ey - sy)
            d2 = np.asarray(pb["dir2"], np.float64).reshape(n2, 2)
            with np.errstate(invalid="ignore"):
                dot = v[0] * d2[:, 0] + v[1] * d2[:, 1]
                cand[i1] &= ~(np.abs(dot) < pb["line_sim_th"])
    D = np.unpackbits(desc1[:, None, :] ^ desc2[None, :, :], axis=2).sum(axis=2).astype(np.int64) if n1 and n2 else \
        np.zeros((n1, n2), np.int64)
    return cand, D


def match_grid_parallel(pb, cols=64, rows=48, best_lr=True, records="prefix"):
    """The formulation of the kernels: per column the strict prefix-minimum records over the
    candidates, per row the two smallest packed keys (d << 16) | i2 of its seen pairs.
    records="column" is the wrong formulation in which only a column's final minimum is seen."""
    cand, D = candidates_and_distances(pb, cols, rows)
    n1, n2 = cand.shape
    nnr = float(pb["nnr"])
    big = np.where(cand, D, INT_MAX)
    m21 = np.full(n2, -1, np.int64)
    if best_lr and n1 and n2:
        if records == "prefix":
            before = np.vstack([np.full((1, n2), INT_MAX, np.int64), np.minimum.accumulate(big, axis=0)[:-1]])
            seen = cand & (D < before)
        else:
            first = np.argmax(big == big.min(axis=0, keepdims=True), axis=0)
            seen = cand & (np.arange(n1)[:, None] == first[None, :])
        has = seen.any(axis=0)
        m21[has] = (n1 - 1 - np.argmax(seen[::-1], axis=0))[has]
    else:
        seen = cand
    keys = np.where(seen, (D << 16) | np.arange(n2, dtype=np.int64)[None, :], NONE_KEY)
    m12 = np.full(n1, -1, np.int32)
    for i1 in range(n1 if n2 else 0):
        k = np.sort(keys[i1])
        k0, k1 = int(k[0]), int(k[1]) if n2 > 1 else NONE_KEY
        if k0 == NONE_KEY:
            continue
        d0, d1 = k0 >> 16, (k1 >> 16 if k1 != NONE_KEY else INT_MAX)
        if float(d0) < float(d1) * nnr:
            i2 = k0 & 0xFFFF
            if not best_lr or m21[i2] == i1:
                m12[i1] = i2
    return m12, int((m12 >= 0).sum())
