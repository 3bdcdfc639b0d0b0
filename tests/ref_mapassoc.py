"""Checker of plba_map_associate: a plain numpy / Python restatement of the semantics in include/plba.h
(MapHandler::matchMap2KFPoints / matchMap2KFLines, src/mapHandler.cpp:697-921, up to the sequential part).
Scalar float64 throughout, one rounding per operation, every sum of three as t0 + (t1 + t2).

It does what the reference does: the visible landmarks are compacted in map order, the compacted list is
matched (ref_stereo.match_grid with the window (ws, ws, ws, ws); ref_kfassoc.brute_force for the fallback) and
the indices are mapped back to the candidate rows. So it knows nothing of how an implementation keeps an
invisible row out of its matchers.

A keyframe is a dict with the keys of capi.MapassocBatchView; prm is a dict with the fields of
plba_mapassoc_params."""
import numpy as np

import ref_gridmatch as R
import ref_kfassoc as RK
import ref_stereo as RS

F32, F64 = np.float32, np.float64
DEFAULTS = dict(cols=64, rows=48, fast_matching=1, ws=3, best_lr=1, min_pt_matches=10, min_ls_matches=6,
                min_ratio_12_p=0.9, min_ratio_12_l=0.9, line_sim_th=0.75, max_kf_epip_p=1.0, max_kf_epip_l=1.0)
COUNTS = ("n_visible", "n_grid", "n_matches", "fallback", "n_accepted")


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


class Margin:
    """The smallest relative distance of a compared quantity to its threshold."""

    def __init__(self):
        self.value, self.where = np.inf, None

    def see(self, x, th, scale, where):
        if np.isfinite(x):
            m = abs(float(x) - float(th)) / float(scale)
            if m < self.value:
                self.value, self.where = m, where


def project(prm, Twf, X):
    """(u, v, Q2): cam->projection(Twf.R X + Twf.t) and the depth."""
    Q = RK.transform(Twf, X)
    with np.errstate(all="ignore"):
        return F64(prm["cx"]) + F64(prm["fx"]) * Q[0] / Q[2], F64(prm["cy"]) + F64(prm["fy"]) * Q[1] / Q[2], Q[2]


def visible(prm, u, v, z, margin=None, where=None):
    """:716, :819-820. NaN compares false."""
    w, h = F64(prm["width"]), F64(prm["height"])
    tests = ((u > 0, u, 0.0, w), (u < w, u, w, w), (v > 0, v, 0.0, h), (v < h, v, h, h), (z > 0.0, z, 0.0, 1.0))
    ok = all(bool(t[0]) for t in tests)
    if margin is not None and all(np.isfinite(t[1]) for t in tests):   # a NaN fails whatever the rounding
        # a conjunction: every test of a visible row must hold by the margin, one failed test of an invisible row
        # suffices (the depth against 0 is measured in metres, the pixels against the image size)
        dist = [abs(float(x) - th) / float(sc) for passed, x, th, sc in tests if bool(passed) == ok]
        margin.see(min(dist) if ok else max(dist), 0.0, 1.0, where)
    return ok


def point_row(prm, Twf, T_kf_w, X, pl, P):
    """(record [6], accepted) of a point match (:770-784)."""
    with np.errstate(all="ignore"):
        u, v, _ = project(prm, Twf, X)
        du, dv = u - pl[0], v - pl[1]
        err = np.sqrt(du * du + dv * dv)
        n = RK.norm3(P)
        d = RK.transform(T_kf_w, [c / n for c in P])
        return [u, v, err] + d, bool(err < F64(prm["max_kf_epip_p"]))


def line_row(prm, Twf, T_kf_w, X, le, sP, eP):
    """(record [9], accepted) of a line match (:885-901)."""
    with np.errstate(all="ignore"):
        su, sv, _ = project(prm, Twf, X[:3])
        eu, ev, _ = project(prm, Twf, X[3:])
        e0 = (le[0] * su + le[1] * sv) + le[2]
        e1 = (le[0] * eu + le[1] * ev) + le[2]
        y = RK.transform(T_kf_w, [F64(0.5) * (a + b) for a, b in zip(sP, eP)])
        n = RK.norm3(y)
        th = F64(prm["max_kf_epip_l"])
        return [su, sv, eu, ev, e0, e1] + [c / n for c in y], bool(e0 < th and e1 < th)


def associate(kf, prm, margin=None, see_invisible=False):
    """The result dict of Solver.map_associate for one keyframe. margin: a Margin that collects the distances
    of the visibility tests, the direction test of every visible line against every line feature, and the
    epipolar tests. see_invisible: the WRONG matcher that leaves the invisible rows in both matchers (their
    flag stays 0), for the tests that show that masking matters."""
    cols, rows, ws = prm["cols"], prm["rows"], prm["ws"]
    inv_w, inv_h = F64(cols) / F64(prm["width"]), F64(rows) / F64(prm["height"])
    Twf, T_kf_w = RK.f64(kf["Twf"])[:12], RK.f64(kf["T_kf_w"])
    res = {k: [0, 0] for k in COUNTS}
    db = next((np.asarray(kf[k]).shape[1] for k in ("pdesc_m", "ldesc_m", "pdesc_f", "ldesc_f") if k in kf), 32)

    def get(key, per, dtype=F64):
        return np.asarray(kf.get(key, np.zeros((0, per))), dtype).reshape(-1, per)
    for kd in (0, 1):
        d1, d2 = get("ldesc_m" if kd else "pdesc_m", db, np.uint8), get("ldesc_f" if kd else "pdesc_f", db, np.uint8)
        X = get("ls_X", 6) if kd else get("pt_X", 3)
        n1, n2 = len(d1), len(d2)
        vis, cells1, cells1e = np.zeros(n1, np.uint8), [], []
        with np.errstate(all="ignore"):
            for i in range(n1):
                x = RK.f64(X[i])
                u, v, z = project(prm, Twf, x[:3])
                ok = visible(prm, u, v, z, margin, ("visible", kd, i))
                c, ce = (u * inv_w, v * inv_h), None
                if kd:
                    u, v, z = project(prm, Twf, x[3:])
                    ok = visible(prm, u, v, z, margin, ("visible end", kd, i)) and ok
                    ce = (u * inv_w, v * inv_h)
                vis[i] = ok
                if ok or see_invisible:   # :719, :823-824: grid units for a line's endpoints too
                    cells1.append(RK.cell(*c) if see_invisible else (int(c[0]), int(c[1])))
                    if kd:
                        cells1e.append(RK.cell(*ce) if see_invisible else (int(ce[0]), int(ce[1])))
        keep = np.arange(n1) if see_invisible else np.flatnonzero(vis)   # the compacted list, in map order
        nv, d1c = int(vis.sum()), d1[keep]
        m12c, n_grid = [-1] * len(keep), 0
        if prm["fast_matching"] and len(keep) and n2:
            grid = RS.WindowGrid(rows, cols)
            dir2 = []
            if kd:
                for idx, (s, e) in enumerate(zip(get("ls_spl", 2), get("ls_epl", 2))):
                    dir2.append(R.normalize((e[0] - s[0]) * inv_w, (e[1] - s[1]) * inv_h))
                    for x, y in R.line_cells(s[0] * inv_w, s[1] * inv_h, e[0] * inv_w, e[1] * inv_h):
                        grid.add(x, y, idx)
                if margin is not None:
                    for j, (c, ce) in enumerate(zip(cells1, cells1e)):
                        q = R.normalize(ce[0] - c[0], ce[1] - c[1])
                        for i2, t in enumerate(dir2):
                            with np.errstate(invalid="ignore"):
                                margin.see(abs(q[0] * t[0] + q[1] * t[1]), prm["line_sim_th"], 1.0, ("direction", j, i2))
            else:
                for idx, pl in enumerate(get("pt_pl", 2)):
                    grid.add(int(pl[0] * inv_w), int(pl[1] * inv_h), idx)
            m12c = RS.match_grid(kd, cells1, cells1e, d1c, grid, d2, dir2, (ws, ws, ws, ws), prm)
            n_grid = sum(i2 >= 0 for i2 in m12c)
        lim = prm["min_ls_matches"] if kd else prm["min_pt_matches"]
        fallback = nv > lim and n_grid < lim   # :759-761, :874-876: both size tests read the visible landmarks
        if fallback:
            m12c = RK.brute_force(d1c, d2, prm["min_ratio_12_l"] if kd else prm["min_ratio_12_p"], bool(prm["best_lr"]))
        m12 = np.full(n1, -1, np.int32)
        m12[keep] = m12c   # the indices mapped back
        nd = 9 if kd else 6
        rec, acc = np.zeros((n1, nd)), np.zeros(n1, np.uint8)
        for i1, i2 in enumerate(m12):
            if i2 < 0:
                continue
            if kd:
                rec[i1], acc[i1] = line_row(prm, Twf, T_kf_w, RK.f64(X[i1]), RK.f64(get("ls_le", 3)[i2]), RK.f64(get("ls_sP", 3)[i2]),
                                            RK.f64(get("ls_eP", 3)[i2]))
                if margin is not None:
                    for e in (4, 5):
                        margin.see(rec[i1, e], prm["max_kf_epip_l"], prm["max_kf_epip_l"], ("line error", i1, e))
            else:
                rec[i1], acc[i1] = point_row(prm, Twf, T_kf_w, RK.f64(X[i1]), RK.f64(get("pt_pl", 2)[i2]), RK.f64(get("pt_P", 3)[i2]))
                if margin is not None:
                    margin.see(rec[i1, 2], prm["max_kf_epip_p"], prm["max_kf_epip_p"], ("point error", i1))
        res["n_visible"][kd], res["n_grid"][kd], res["fallback"][kd] = nv, n_grid, int(fallback)
        res["n_matches"][kd] = res["n_accepted"][kd] = int(acc.sum())   # :793, :917: counted after the test
        k = "ls" if kd else "pt"
        res.update({k + "_visible": vis, k + "_m12": m12, k + "_accepted": acc, k + "_rec": rec})
    for k in COUNTS:
        res[k] = tuple(int(v) for v in res[k])
    return res


ARRAYS = ("pt_visible", "pt_m12", "pt_accepted", "pt_rec", "ls_visible", "ls_m12", "ls_accepted", "ls_rec")


def same(a, b):
    """None if the two results are equal bit for bit (NaN equal to NaN), else the first difference."""
    for k in COUNTS:
        if tuple(a[k]) != tuple(b[k]):
            return f"{k}: {a[k]} != {b[k]}"
    for k in ARRAYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            return f"{k}: shape {x.shape} != {y.shape}"
        if x.dtype.kind == "f":
            x, y = np.ascontiguousarray(x, F64).view(np.uint64), np.ascontiguousarray(y, F64).view(np.uint64)
        if not np.array_equal(x, y):
            i = np.argwhere(x != y)[0]
            return f"{k}{tuple(i)}: {np.asarray(a[k])[tuple(i)]!r} != {np.asarray(b[k])[tuple(i)]!r}"
    return None
