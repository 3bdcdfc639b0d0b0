"""Checker of plba_kf_associate: a plain numpy / Python restatement of the semantics in include/plba.h
(MapHandler::matchKF2KFPoints / matchKF2KFLines, src/mapHandler.cpp:237-590, up to the sequential part).
Scalar float64 throughout, one rounding per operation (numpy scalars never fuse), every sum of three as
t0 + (t1 + t2).

The grid matcher is ref_stereo.match_grid over ref_stereo.WindowGrid with the window (ws, ws, ws, ws); the
brute-force matcher is match() as plba_desc_match defines it (float ratio test, ties to the lowest index).

A pair is a dict with the keys of capi.KfassocBatchView; prm is a dict with the fields of plba_kfassoc_params."""
import numpy as np

import ref_gridmatch as R
import ref_stereo as RS

F32, F64 = np.float32, np.float64
NO_CELL = -(1 << 30)
DEFAULTS = dict(cols=64, rows=48, fast_matching=1, ws=3, best_lr=1, min_pt_matches=10, min_ls_matches=6,
                line_query_in_grid_units=0, min_ratio_12_p=0.9, min_ratio_12_l=0.9, line_sim_th=0.75)
GATE = np.sqrt(F64(5.991))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def sum3(t0, t1, t2):
    return t0 + (t1 + t2)


def dot3(a, b):
    return sum3(a[0] * b[0], a[1] * b[1], a[2] * b[2])


def norm3(a):
    return np.sqrt(dot3(a, a))


def f64(a):
    return [F64(v) for v in np.asarray(a, F64).ravel()]


def rot(T, x):
    """T: 12 or 16 doubles, row-major with four per row."""
    return [dot3(T[4 * i:4 * i + 3], x) for i in range(3)]


def transform(T, x):
    return [y + T[4 * i + 3] for i, y in enumerate(rot(T, x))]


def project(prm, DT, P):
    Q = transform(DT, P)
    with np.errstate(all="ignore"):
        return F64(prm["cx"]) + F64(prm["fx"]) * Q[0] / Q[2], F64(prm["cy"]) + F64(prm["fy"]) * Q[1] / Q[2]


def cell(gx, gy):
    if abs(gx) < 2.0 ** 30 and abs(gy) < 2.0 ** 30:   # false for NaN
        return int(gx), int(gy)
    return NO_CELL, NO_CELL


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def pluker(T, ND):
    """TransformForPluker: (head, tail)."""
    t = [T[3], T[7], T[11]]
    cols = [cross(t, [T[j], T[4 + j], T[8 + j]]) for j in range(3)]
    M = [[cols[j][i] for j in range(3)] for i in range(3)]
    head = [dot3(T[4 * i:4 * i + 3], ND[:3]) + dot3(M[i], ND[3:]) for i in range(3)]
    return head, rot(T, ND[3:])


def line_err(prm, Tcw, W, s, e):
    fx, fy, cx, cy = (F64(prm[k]) for k in ("fx", "fy", "cx", "cy"))
    h, _ = pluker(Tcw, W)
    lx, ly = fy * h[0], fx * h[1]
    lz = sum3(((-fy) * cx) * h[0], ((-fx) * cy) * h[1], (fx * fy) * h[2])
    with np.errstate(all="ignore"):
        f = np.sqrt(lx * lx + ly * ly)
        e0 = ((s[0] * lx + s[1] * ly) + lz) / f
        e1 = ((e[0] * lx + e[1] * ly) + lz) / f
        return np.sqrt(e0 * e0 + e1 * e1)


def point_row(T_prev, T_curr, P1, P2):
    with np.errstate(all="ignore"):
        P3d = transform(T_prev, P1)
        n1 = norm3(P3d)
        Pc = transform(T_curr, P2)
        n2 = norm3(Pc)
        return P3d + [v / n1 for v in P3d] + [v / n2 for v in Pc]


def line_row(prm, T_prev, Tcw_prev, Tcw_curr, NDc, spl, epl, lm_NDw, is_new, spl_c, epl_c):
    """(record [8], rejected)"""
    with np.errstate(all="ignore"):
        if is_new:
            head, tail = pluker(T_prev, NDc)
            nh, nt = norm3(head), norm3(tail)
            d = nh / nt
            W = [(v / nh) * d for v in head] + [v / nt for v in tail]
            rec = W + [line_err(prm, Tcw_prev, W, spl, epl), line_err(prm, Tcw_curr, W, spl_c, epl_c)]
        else:
            rec = [F64(0.0)] * 7 + [line_err(prm, Tcw_curr, lm_NDw, spl_c, epl_c)]
        return rec, int(rec[7] > GATE)


def brute_force(desc1, desc2, nnr, best_lr):
    """match() (src2/matching.cpp:63-91) as plba_desc_match defines it."""
    n1, n2 = len(desc1), len(desc2)
    bits1, bits2 = np.unpackbits(desc1, axis=1).astype(np.int32), np.unpackbits(desc2, axis=1).astype(np.int32)
    dist = bits1 @ (1 - bits2).T + (1 - bits1) @ bits2.T

    def nn(d):
        out = []
        for row in d:
            if len(row) < 2:
                out.append(-1)
                continue
            i0 = int(np.argmin(row))   # the first of equal minima
            d1 = int(np.delete(row, i0).min())
            out.append(i0 if F32(row[i0]) < F32(d1) * F32(nnr) else -1)
        return out
    m12, m21 = nn(dist), nn(dist.T)
    if best_lr:
        m12 = [i2 if i2 >= 0 and m21[i2] == i1 else -1 for i1, i2 in enumerate(m12)]
    assert len(m12) == n1 and len(m21) == n2
    return m12


def associate(pair, prm):
    """The result dict of Solver.kf_associate for one pair."""
    cols, rows, ws = prm["cols"], prm["rows"], prm["ws"]
    inv_w, inv_h = F64(cols) / F64(prm["width"]), F64(rows) / F64(prm["height"])
    DT, T_prev, T_curr, Tcw_prev, Tcw_curr = (f64(pair[k]) for k in ("DT", "T_prev", "T_curr", "Tcw_prev", "Tcw_curr"))
    res = dict(n_grid=[0, 0], n_matches=[0, 0], fallback=[0, 0])
    db = next((np.asarray(pair[k]).shape[1] for k in ("pdesc_p", "ldesc_p", "pdesc_c", "ldesc_c") if k in pair), 32)

    def get(key, per, dtype=F64):
        return np.asarray(pair.get(key, np.zeros((0, per))), dtype).reshape(-1, per)
    for kd in (0, 1):
        d1, d2 = get("ldesc_p" if kd else "pdesc_p", db, np.uint8), get("ldesc_c" if kd else "pdesc_c", db, np.uint8)
        n1, n2 = len(d1), len(d2)
        m12, n_grid = [-1] * n1, 0
        if prm["fast_matching"] and n1 and n2:
            grid = RS.WindowGrid(rows, cols)
            cells1, cells1e, dir2 = [], [], []
            if kd:
                for sP, eP in zip(get("ls_sP_p", 3), get("ls_eP_p", 3)):
                    for P, dst in ((sP, cells1), (eP, cells1e)):
                        u, v = project(prm, DT, f64(P))
                        dst.append(cell(u * inv_w, v * inv_h) if prm["line_query_in_grid_units"] else cell(u, v))
                for idx, (s, e) in enumerate(zip(get("ls_spl_c", 2), get("ls_epl_c", 2))):
                    dir2.append(R.normalize((e[0] - s[0]) * inv_w, (e[1] - s[1]) * inv_h))
                    for x, y in R.line_cells(s[0] * inv_w, s[1] * inv_h, e[0] * inv_w, e[1] * inv_h):
                        grid.add(x, y, idx)
            else:
                for P in get("pt_P_p", 3):
                    u, v = project(prm, DT, f64(P))
                    cells1.append(cell(u * inv_w, v * inv_h))
                for idx, pl in enumerate(get("pt_pl_c", 2)):
                    grid.add(int(pl[0] * inv_w), int(pl[1] * inv_h), idx)
            m12 = RS.match_grid(kd, cells1, cells1e, d1, grid, d2, dir2, (ws, ws, ws, ws), prm)
            n_grid = sum(i2 >= 0 for i2 in m12)
        lim = prm["min_ls_matches"] if kd else prm["min_pt_matches"]
        fallback = n2 > lim and n1 > lim and n_grid < lim
        if fallback:
            m12 = brute_force(d1, d2, prm["min_ratio_12_l"] if kd else prm["min_ratio_12_p"], bool(prm["best_lr"]))
        res["n_grid"][kd], res["n_matches"][kd], res["fallback"][kd] = n_grid, sum(i2 >= 0 for i2 in m12), int(fallback)
        if kd:
            rec, rej = np.zeros((n1, 8)), np.zeros(n1, np.uint8)
            NDc, spl, epl, NDw, new = get("ls_NDc_p", 6), get("ls_spl_p", 2), get("ls_epl_p", 2), get("ls_lm_NDw", 6), \
                get("ls_new", 1, np.uint8)
            spl_c, epl_c = get("ls_spl_c", 2), get("ls_epl_c", 2)
            for i1, i2 in enumerate(m12):
                if i2 >= 0:
                    rec[i1], rej[i1] = line_row(prm, T_prev, Tcw_prev, Tcw_curr, f64(NDc[i1]), f64(spl[i1]), f64(epl[i1]),
                                                f64(NDw[i1]), bool(new[i1, 0]), f64(spl_c[i2]), f64(epl_c[i2]))
            res.update(ls_m12=np.asarray(m12, np.int32).reshape(-1), ls_rec=rec, ls_rejected=rej)
        else:
            rec = np.zeros((n1, 9))
            P1, P2 = get("pt_P_p", 3), get("pt_P_c", 3)
            for i1, i2 in enumerate(m12):
                if i2 >= 0:
                    rec[i1] = point_row(T_prev, T_curr, f64(P1[i1]), f64(P2[i2]))
            res.update(pt_m12=np.asarray(m12, np.int32).reshape(-1), pt_rec=rec)
    for k in ("n_grid", "n_matches", "fallback"):
        res[k] = tuple(int(v) for v in res[k])
    return res


def same(a, b):
    """None if the two results are equal bit for bit (NaN equal to NaN), else the first difference."""
    for k in ("n_grid", "n_matches", "fallback"):
        if tuple(a[k]) != tuple(b[k]):
            return f"{k}: {a[k]} != {b[k]}"
    for k in ("pt_m12", "ls_m12", "ls_rejected", "pt_rec", "ls_rec"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            return f"{k}: shape {x.shape} != {y.shape}"
        if x.dtype.kind == "f":
            x, y = np.ascontiguousarray(x, F64).view(np.uint64), np.ascontiguousarray(y, F64).view(np.uint64)
        if not np.array_equal(x, y):
            i = np.argwhere(x != y)[0]
            return f"{k}{tuple(i)}: {np.asarray(a[k])[tuple(i)]!r} != {np.asarray(b[k])[tuple(i)]!r}"
    return None
