"""Checker of plba_stereo_associate: a plain numpy / Python restatement of the semantics in include/plba.h
(StereoFrame::matchStereoPoints / matchStereoLines, src2/stereoFrame.cpp:121-174, :310-435). float32 where
the reference has float, float64 elsewhere, one rounding per operation (numpy scalars never fuse).

The matcher is matchGrid as tests/ref_gridmatch.py states it (its grid of lists, its line rasteriser, its
Hamming distance and normalize are imported); that module's match_grid takes one symmetric half-width, so
the query loop is restated here over a grid whose get() takes the four half-widths of a GridWindow.

A frame is a dict: pt_l / pt_r [n][2] float32, pdesc_l / pdesc_r [n][B] uint8, ls_l / ls_r [n][4] float32
(sx, sy, ex, ey), ldesc_l / ldesc_r. prm is a dict with the fields of plba_stereo_params."""
import numpy as np

import ref_gridmatch as R

F32, F64 = np.float32, np.float64
INT_MAX = R.INT_MAX
DEFAULTS = dict(cols=64, rows=48, matching_s_ws=10, best_lr=1, pluker=0, min_ratio_12_p=0.9, line_sim_th=0.75,
                max_dist_epip=1.0, min_disp=1.0, ls_min_disp_ratio=0.7, line_horiz_th=0.1, stereo_overlap_th=0.75)
PT_GATES = ("epip", "disp")
LS_GATES = ("disp_s", "disp_e", "horiz_l", "horiz_r", "overlap")


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


class WindowGrid(R.Grid):
    def get4(self, x, y, w, indices):
        """GridStructure::get with w = (left, right, up, down)."""
        for x_ in range(max(0, x - w[0]), min(self.cols, x + w[1] + 1)):
            for y_ in range(max(0, y - w[2]), min(self.rows, y + w[3] + 1)):
                indices.update(self.grid[x_][y_])


def cell(v, inv):
    return int(F64(v) * inv)   # the float promoted, one product, truncated toward zero


def match_grid(kind, cells1, cells1e, desc1, grid, desc2, dir2, w, prm, stats=None):
    """matchGrid (src2/matching.cpp:111-258) over a filled grid with the window w."""
    n1, n2 = len(desc1), len(desc2)
    best_lr, nnr, th = bool(prm["best_lr"]), float(prm["min_ratio_12_p"]), prm["line_sim_th"]
    m12, m21, dist = [-1] * n1, [-1] * n2, [INT_MAX] * n2
    ws = w[0]
    for i1 in range(n1):
        best_d, best_d2, best_idx = INT_MAX, INT_MAX, -1
        cand, sym = set(), set()
        grid.get4(*cells1[i1], w, cand)
        grid.get4(*cells1[i1], (ws, ws, ws, ws), sym)
        if kind:
            v = R.normalize(cells1e[i1][0] - cells1[i1][0], cells1e[i1][1] - cells1[i1][1])
            grid.get4(*cells1e[i1], w, cand)
            grid.get4(*cells1e[i1], (ws, ws, ws, ws), sym)
        if stats is not None:
            stats["window_pass"] += len(cand)
            stats["window_reject"] += len(sym - cand)
        for i2 in sorted(cand):
            if kind:
                with np.errstate(invalid="ignore"):
                    dot = v[0] * F64(dir2[i2][0]) + v[1] * F64(dir2[i2][1])
                    if abs(dot) < th:
                        continue
            d = R.hamming_row(desc1[i1], desc2[i2])
            if best_lr:
                if d < dist[i2]:
                    dist[i2], m21[i2] = d, i1
                else:
                    continue
            if d < best_d:
                best_d2, best_d, best_idx = best_d, d, i2
            elif d < best_d2:
                best_d2 = d
        if best_idx >= 0 and float(best_d) < float(best_d2) * nnr:
            m12[i1] = best_idx
    if best_lr:
        for i1 in range(n1):
            if m12[i1] >= 0 and m21[m12[i1]] != i1:
                m12[i1] = -1
    return m12


def back_projection(prm, u, v, disp):
    with np.errstate(all="ignore"):
        bd = F64(prm["b"]) / disp
        return np.array([bd * (u - F64(prm["cx"])), bd * (v - F64(prm["cy"])), bd * F64(prm["fx"])], F64)


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F64)


def pi_from_ppp(x1, x2, x3):
    n = cross(x1 - x3, x2 - x3)
    c = cross(x1, x2)
    return np.array([n[0], n[1], n[2], -(x3[0] * c[0] + (x3[1] * c[1] + x3[2] * c[2]))], F64)


def overlap_stereo(spl_obs, epl_obs, spl_proj, epl_proj, horiz_th):
    overlap = F64(1.0)
    if abs(epl_obs - spl_obs) > horiz_th:
        sln, eln = min(spl_obs, epl_obs), max(spl_obs, epl_obs)
        spn, epn = min(spl_proj, epl_proj), max(spl_proj, epl_proj)
        length = eln - spn
        if epn < sln or spn > eln:
            overlap = F64(0.0)
        elif epn > eln and spn < sln:
            overlap = eln - sln
        else:
            overlap = min(eln, epn) - max(sln, spn)
        overlap = overlap / length if length > F64(F32(0.01)) else F64(0.0)
        if overlap > 1.0:
            overlap = F64(1.0)
    return overlap


def point_row(prm, l, r):
    """(gate bits, pl, disp, P) of the match of two keypoints (float32 [2])."""
    dy, dx = abs(F32(l[1]) - F32(r[1])), F32(l[0]) - F32(r[0])   # in float
    disp = F64(dx)
    bits = (0 if F64(dy) <= prm["max_dist_epip"] else 1) | (0 if disp >= prm["min_disp"] else 2)
    pl = np.array([F64(l[0]), F64(l[1])])
    return bits, pl, disp, back_projection(prm, pl[0], pl[1], disp)


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def line_row(prm, l, r):
    """(gate bits, dict of the line outputs) of the match of two segments (float32 [4])."""
    with np.errstate(all="ignore"):
        slx, sly, elx, ely = (F64(v) for v in l)
        srx, sry, erx, ery = (F64(v) for v in r)
        one = F64(1.0)
        le = cross(np.array([slx, sly, one]), np.array([elx, ely, one]))
        le = le / np.sqrt(le[0] * le[0] + le[1] * le[1])
        overlap = overlap_stereo(sly, ely, sry, ery, prm["line_horiz_th"])
        X = (srx * (sly - ery) + erx * (sry - sly)) / (sry - ery)          # :367; sp_r = (X, sly)
        Xe = (X * (ely - ery) + erx * (sly - ely)) / (sly - ery)           # :368 reads the new sp_r
        ds, de = slx - X, elx - Xe
        if std_min(ds, de) / std_max(ds, de) < prm["ls_min_disp_ratio"]:
            ds, de = F64(-1.0), F64(-1.0)
        horiz_l = abs(sly - ely) > prm["line_horiz_th"]
        horiz_r = abs(sly - ely) > prm["line_horiz_th"]                    # sp_r(1) - ep_r(1) after the overwrite
        bits = ((0 if ds >= prm["min_disp"] else 1) | (0 if de >= prm["min_disp"] else 2) | (0 if horiz_l else 4) |
                (0 if horiz_r else 8) | (0 if overlap > prm["stereo_overlap_th"] else 16))
        o = dict(spl=np.array([slx, sly]), epl=np.array([elx, ely]), sdisp=ds, edisp=de,
                 sP=back_projection(prm, slx, sly, ds), eP=back_projection(prm, elx, ely, de), le=le)
        if prm["pluker"]:
            fx, fy, cx, cy, b = (F64(prm[k]) for k in ("fx", "fy", "cx", "cy", "b"))

            def unit(u, v):
                return np.array([(u - cx) / fx, (v - cy) / fy, one])
            a, c = unit(slx, sly), unit(elx, ely)
            a2, c2 = unit(X, sly), unit(Xe, ely)
            a2[0], c2[0] = a2[0] + b, c2[0] + b                            # :388-389: only x is shifted
            pi1 = pi_from_ppp(a, c, np.zeros(3))
            pi2 = pi_from_ppp(a2, c2, np.array([b, 0.0, 0.0]))

            def dp(i, j):
                return pi1[i] * pi2[j] - pi2[i] * pi1[j]
            o["NDc"] = np.array([dp(0, 3), dp(1, 3), dp(2, 3), -dp(1, 2), dp(0, 2), -dp(0, 1)], F64)
    return bits, o


def associate(frame, prm, stats=None):
    """One frame: the dict that Solver.stereo_associate returns for it. stats (optional) is a dict that
    collects, over calls, how often every gate and the window's asymmetry rejected and passed."""
    db = next((np.asarray(frame[k]).shape[1] for k in ("pdesc_l", "pdesc_r", "ldesc_l", "ldesc_r")
               if k in frame and np.asarray(frame[k]).ndim == 2 and np.asarray(frame[k]).shape[1]), 32)
    cols, rows = prm["cols"], prm["rows"]
    inv_w, inv_h = cols / F64(prm["width"]), rows / F64(prm["height"])
    w = (int(prm["matching_s_ws"]), 0, 0, 0)
    if stats is not None and not stats:
        stats.update(window_pass=0, window_reject=0, **{f"{g}_{k}": 0 for g in PT_GATES + LS_GATES for k in ("pass", "reject")})
    res = {}
    for kind, (lk, rk, dl, dr) in enumerate((("pt_l", "pt_r", "pdesc_l", "pdesc_r"), ("ls_l", "ls_r", "ldesc_l", "ldesc_r"))):
        per = 4 if kind else 2
        cl = np.asarray(frame.get(lk, np.zeros((0, per))), F32).reshape(-1, per)
        cr = np.asarray(frame.get(rk, np.zeros((0, per))), F32).reshape(-1, per)
        d1 = np.asarray(frame.get(dl, np.zeros((0, db))), np.uint8).reshape(-1, db)
        d2 = np.asarray(frame.get(dr, np.zeros((0, db))), np.uint8).reshape(-1, db)
        grid = WindowGrid(rows, cols)
        dir2 = []
        for idx, c in enumerate(cr):
            if kind:
                dir2.append(R.normalize(F64(c[2] - c[0]) * inv_w, F64(c[3] - c[1]) * inv_h))   # float differences
                for x, y in R.line_cells(F64(c[0]) * inv_w, F64(c[1]) * inv_h, F64(c[2]) * inv_w, F64(c[3]) * inv_h):
                    grid.add(x, y, idx)
            else:
                grid.add(cell(c[0], inv_w), cell(c[1], inv_h), idx)
        cells1 = [(cell(c[0], inv_w), cell(c[1], inv_h)) for c in cl]
        cells1e = [(cell(c[2], inv_w), cell(c[3], inv_h)) for c in cl] if kind else None
        m12 = match_grid(kind, cells1, cells1e, d1, grid, d2, dir2, w, prm, stats) if len(cl) and len(cr) else [-1] * len(cl)
        names = ("spl", "epl", "sdisp", "edisp", "sP", "eP", "le") + (("NDc",) if prm["pluker"] else ()) if kind else ()
        src, desc, rows_out = [], [], {k: [] for k in (names if kind else ("pl", "disp", "P"))}
        for i1, i2 in enumerate(m12):
            if i2 < 0:
                continue
            if kind:
                bits, o = line_row(prm, cl[i1], cr[i2])
            else:
                bits, pl, disp, P = point_row(prm, cl[i1], cr[i2])
                o = dict(pl=pl, disp=disp, P=P)
            if stats is not None:
                for k, g in enumerate(LS_GATES if kind else PT_GATES):
                    stats[f"{g}_{'reject' if bits >> k & 1 else 'pass'}"] += 1
            if bits:
                continue
            src.append(i1)
            desc.append(d1[i1])
            for k in rows_out:
                rows_out[k].append(o[k])
        pre = "ls_" if kind else "pt_"
        shapes = dict(pl=(0, 2), disp=(0,), P=(0, 3), spl=(0, 2), epl=(0, 2), sdisp=(0,), edisp=(0,), sP=(0, 3), eP=(0, 3),
                      le=(0, 3), NDc=(0, 6))
        res["n_ls" if kind else "n_pt"] = len(src)
        res[pre + "src"] = np.asarray(src, np.int32).reshape(-1)
        res["ldesc" if kind else "pdesc"] = np.asarray(desc, np.uint8).reshape(-1, db)
        for k, v in rows_out.items():
            res[pre + k] = np.asarray(v, F64).reshape((-1,) + shapes[k][1:])
    return res


def same(a, b):
    """Bitwise equality of two result dicts; returns the first key that differs, or None."""
    if set(a) != set(b):
        return "keys %s" % sorted(set(a) ^ set(b))
    for k in sorted(a):
        x, y = a[k], b[k]
        if isinstance(x, (int, np.integer)):
            if int(x) != int(y):
                return k
        elif x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return k
    return None
