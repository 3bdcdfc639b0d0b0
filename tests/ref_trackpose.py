"""TEST INFRASTRUCTURE: numpy checker of the frame-to-frame pose (plba_track_pose).

StereoFrameHandler::optimizePose (src2/stereoFrameHandler.cpp:307-405) with
gaussNewtonOptimizationRobust / optimizeFunctionsRobust (:446-494, :1010-1277; line model 1, the
endpoints) and gaussNewtonOptimizationforPluker / optimizeFunctionsUsingPluker (:803-853, :564-801;
line model 0), removeOutliers (:1303-1396), isGoodSolution (:292-305), vector_stdv_mad /
vector_mean_stdv_mad (src2/auxiliar.cpp:444-460, :387-430) and StereoFrame::lineSegmentOverlap
(src2/stereoFrame.cpp:547-653), restated from their lines in float64. PARITY UNPINNED against the
reference itself (it cannot be built here); pinned by tests/test_trackpose_oracle.py (hand-computed
values, finite differences, every branch).

Sums are in match order, points then lines. The deviations of the MAD go through np.float32, as
fabsf does. Defined where the reference is not, as include/plba.h says: isGoodSolution's comparisons
are written so that a NaN is not good; no active match gives err = NaN; a non-finite H or g gives a
NaN step; a singular last H gives a NaN covariance.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

import oracle_api as oa
import ref_lcpose as rl

PLUCKER, ENDPOINTS = 0, 1
OK, FEW_BEFORE, FIRST_NOT_GOOD, FEW_AFTER, FINAL_NOT_GOOD = range(5)
TH_MIN, TH_MAX = 0.0001, float(np.sqrt(7.815))
ERR_PREV0 = 999999999.9


# ---- src2/auxiliar.cpp
def _mad(res):
    """(median, MAD): element n/2 of the sorted list, then of the sorted float deviations."""
    r = np.sort(np.asarray(res, np.float64))
    n = len(r)
    med = r[n // 2]
    with np.errstate(all="ignore"):
        dev = np.sort(np.abs((r - med).astype(np.float32)).astype(np.float64))
    return float(med), float(dev[n // 2])


def vector_stdv_mad(res) -> float:
    """:444-460."""
    if len(res) == 0:
        return 0.0
    return 1.4826 * _mad(res)[1]


def vector_mean_stdv_mad(res):
    """:387-430 -> (mean, stdv)."""
    res = np.asarray(res, np.float64)
    n = len(res)
    if n == 0:
        return 0.0, 0.0
    stdv = 1.4826 * _mad(res)[1]
    mean, k = 0.0, 0
    for v in res:
        if v < 2.0 * stdv:
            mean += v
            k += 1
    if k >= int(0.2 * n):
        with np.errstate(all="ignore"):
            mean = np.float64(mean) / np.float64(k)
    else:
        mean = 0.0
        for v in res:
            mean += v
        mean /= float(n)
    return float(mean), float(stdv)


def clamp_scale(s: float) -> float:
    return min(max(s, TH_MIN), TH_MAX) if s == s else s


# ---- src2/stereoFrame.cpp:547-653
def line_segment_overlap(so, eo, sp, ep) -> float:
    with np.errstate(all="ignore"):
        if abs(so[0] - eo[0]) < 1.0:
            l1 = eo[1] - so[1]
            ls, le = (sp[1] - so[1]) / l1, (ep[1] - so[1]) / l1
        elif abs(so[1] - eo[1]) < 1.0:
            l0 = eo[0] - so[0]
            ls, le = (sp[0] - so[0]) / l0, (ep[0] - so[0]) / l0
        else:
            l0 = eo[0] - so[0]
            a, b, c = so[1] - eo[1], eo[0] - so[0], so[0] * eo[1] - eo[0] * so[1]
            lxy = 1.0 / (a * a + b * b)
            xs = (b * (b * sp[0] - a * sp[1]) - a * c) * lxy
            xe = (b * (b * ep[0] - a * ep[1]) - a * c) * lxy
            ls, le = (xs - so[0]) / l0, (xe - so[0]) / l0
    lmin = le if le < ls else ls
    lmax = le if ls < le else ls
    if lmin < 0.0 and lmax > 1.0:
        return 1.0
    if lmax < 0.0 or lmin > 1.0:
        return 0.0
    if lmin < 0.0:
        return float(lmax)
    if lmax > 1.0:
        return float(1.0 - lmin)
    return float(lmax - lmin)


# ---- the Plücker line (include2/stereoFrameHandler.h:106-122, src2/pinholeStereoCamera.cpp:123-125)
def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def pluker_k(cam):
    fx, fy, cx, cy = cam
    return np.array([[fy, 0.0, 0.0], [0.0, fx, 0.0], [-fy * cx, -fx * cy, fx * fy]])


def transform_for_pluker(T, ND):
    """The six entries of TransformForPluker(T, ND)."""
    R, t = T[:3, :3], T[:3, 3]
    M = np.zeros((6, 6))
    M[:3, :3] = R
    M[:3, 3:] = hat(t) @ R
    M[3:, 3:] = R
    return M @ ND


def pluker_res(T, ND, obs, cam):
    """(‖e‖, err0, err1, l, R·N, R·D) of one line (:712-720), products summed left to right."""
    R, t = T[:3, :3], T[:3, 3]
    RN = np.array([(R[i, 0] * ND[0] + R[i, 1] * ND[1]) + R[i, 2] * ND[2] for i in range(3)])
    RD = np.array([(R[i, 0] * ND[3] + R[i, 1] * ND[4]) + R[i, 2] * ND[5] for i in range(3)])
    n = np.zeros(3)
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        s = RN[i]
        for j in range(3):
            s += (t[i1] * R[i2, j] - t[i2] * R[i1, j]) * ND[3 + j]
        n[i] = s
    fx, fy, cx, cy = cam
    l = np.array([fy * n[0], fx * n[1], ((-fy * cx) * n[0] + (-fx * cy) * n[1]) + (fx * fy) * n[2]])
    d = np.sqrt(l[0] * l[0] + l[1] * l[1])
    e0 = (obs[0] * l[0] + obs[1] * l[1] + l[2]) / d
    e1 = (obs[2] * l[0] + obs[3] * l[1] + l[2]) / d
    return float(np.sqrt(e0 * e0 + e1 * e1)), e0, e1, l, RN, RD


def pluker_row(T, obs, cam, hth, r, e0, e1, l, RN, RD):
    """J_aux of :722-753."""
    fx, fy, cx, cy = cam
    t = T[:3, 3]
    lx, ly = l[0], l[1]
    fm = 1.0 / np.sqrt(lx * lx + ly * ly)
    hd, hn, ht = hat(RD), hat(RN), hat(t)
    B = np.zeros((3, 6))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += ht[i, k] * hd[k, j]
            B[i, j] = -hd[i, j]
            B[i, 3 + j] = -hn[i, j] - s
    jac = []
    for (a, b, e) in ((obs[0], obs[1], e0), (obs[2], obs[3], e1)):
        f0, f1, f2 = a * fm - lx * e * fm * fm, b * fm - ly * e * fm * fm, fm
        k0, k1, k2 = f0 * fy + f2 * (-fy * cx), f1 * fx + f2 * (-fx * cy), f2 * (fx * fy)
        jac.append((k0 * B[0] + k1 * B[1]) + k2 * B[2])
    return (jac[0] * e0 + jac[1] * e1) / max(hth, r)


# ---- the dense pieces
def qr_solve_logdet(H, g):
    """(x, logAbsDeterminant) of ColPivHouseholderQR(H); NaN for a non-finite system."""
    if not (np.isfinite(H).all() and np.isfinite(g).all()):
        return np.full(6, np.nan), float("nan")
    R = scipy.linalg.qr(H, pivoting=True)[1]
    with np.errstate(all="ignore"):
        logdet = float(np.log(np.abs(np.diag(R))).sum())
    return rl.qr_solve(H, g), logdet


def inverse6(H):
    """H⁻¹, all NaN for a singular or non-finite H."""
    try:
        with np.errstate(all="ignore"):
            C = np.linalg.inv(H)
        if np.isfinite(C).all():
            return C
    except np.linalg.LinAlgError:
        pass
    return np.full((6, 6), np.nan)


def eigenvalues(C):
    if not np.isfinite(C).all():
        return np.full(6, np.nan)
    return np.linalg.eigvalsh(C)


def is_good(DT, C, err) -> bool:
    """:292-305, a NaN is not good."""
    ev = eigenvalues(C)
    return bool(ev[0] >= 0.0 and ev[5] <= 1.0 and err >= 0.0 and err <= 1.0 and np.isfinite(DT).all())


def step_left(T, x):
    """inverse_se3(expmap_se3(x)) · T  (:474, :831)."""
    return rl.mat4mul(rl.inverse_se3(oa.hlm_expmap(x)), T)


class _Problem:
    def __init__(self, prob, params):
        f = lambda a, w: np.asarray(a, np.float64).reshape(-1, w)
        self.p = params
        self.cam = tuple(float(v) for v in prob.cam)
        self.hth = float(params.homog_th)
        self.pluker = int(params.line_model) == PLUCKER
        self.P, self.obs, self.ps2 = f(prob.pt_P, 3), f(prob.pt_obs, 2), f(prob.pt_sigma2, 1)[:, 0]
        self.sP, self.eP, self.ND, self.le = f(prob.ln_sP, 3), f(prob.ln_eP, 3), f(prob.ln_NDc, 6), f(prob.ln_le, 3)
        self.lobs, self.seg, self.ls2 = f(prob.ln_obs, 4), f(prob.ln_seg, 4), f(prob.ln_sigma2, 1)[:, 0]
        self.n_pt, self.n_ln = len(self.P), len(self.sP)
        self.pin, self.lin = np.ones(self.n_pt, bool), np.ones(self.n_ln, bool)
        self.prev = np.asarray(prob.prev, np.float64).reshape(53)
        self.H, self.cov, self.err = np.zeros((6, 6)), np.zeros((6, 6)), -1.0
        self.s_p = self.s_l = 0.0
        self.iters = [0, 0]
        self.trace = []   # per pass: dict(e, de, x_norm, logdet) for the margins

    # residuals of all points / lines at T
    def point_all(self, T):
        if self.n_pt == 0:
            z = np.zeros(0)
            return z, z, z, np.zeros((0, 3))
        return rl.point_res(T, self.P, self.obs, self.cam)

    def line_proj(self, T):
        Gs, Ge = rl.xform(T, self.sP), rl.xform(T, self.eP)
        us, vs = rl.project(Gs, self.cam)
        ue, ve = rl.project(Ge, self.cam)
        return Gs, Ge, np.stack([us, vs], 1), np.stack([ue, ve], 1)

    def line_all(self, T):
        """r (n,) and what the rows need."""
        if self.n_ln == 0:
            return np.zeros(0), None
        if self.pluker:
            out = [pluker_res(T, self.ND[i], self.lobs[i], self.cam) for i in range(self.n_ln)]
            return np.array([o[0] for o in out]), out
        r, ds, de, Gs, Ge = rl.line_res(T, self.sP, self.eP, self.le, self.cam)
        return r, (ds, de, Gs, Ge)

    def loop(self, T, cap, phase):
        """One Gauss–Newton loop from T; returns the loop's DT."""
        p, cam, hth = self.p, self.cam, self.hth
        T_start, err_prev, bad, e = T.copy(), ERR_PREV0, False, 0.0
        for _ in range(int(cap)):
            self.iters[phase] += 1
            rp, dx, dy, G = self.point_all(T)
            rln, aux = self.line_all(T)
            self.s_p = clamp_scale(vector_stdv_mad(rp[self.pin]))
            self.s_l = clamp_scale(vector_stdv_mad(rln[self.lin]))
            H, g, en, N = np.zeros((6, 6)), np.zeros(6), 0.0, 0
            if self.n_pt:
                Jp = rl.jrow(G, dx, dy, cam, hth) / np.maximum(hth, rp)[:, None]
                for k in np.flatnonzero(self.pin):
                    x = rp[k] / self.s_p
                    w = 1.0 / (1.0 + x * x)
                    H += Jp[k][:, None] * Jp[k][None, :] * w
                    g += Jp[k] * rp[k] * w
                    en += rp[k] * rp[k] * w
                    N += 1
            if self.n_ln:
                Gs, Ge, ps, pe = self.line_proj(T)
                if not self.pluker:
                    ds, de, _, _ = aux
                    Js = rl.jrow(Gs, self.le[:, 0], self.le[:, 1], cam, hth)
                    Je = rl.jrow(Ge, self.le[:, 0], self.le[:, 1], cam, hth)
                    Jl = (Js * ds[:, None] + Je * de[:, None]) / np.maximum(hth, rln)[:, None]
                for k in np.flatnonzero(self.lin):
                    r = rln[k]
                    if self.pluker:
                        _, e0, e1, l, RN, RD = aux[k]
                        J = pluker_row(T, self.lobs[k], cam, hth, r, e0, e1, l, RN, RD)
                        rg = r * np.sqrt(self.ls2[k])
                    else:
                        J, rg = Jl[k], r
                    x = r / self.s_l
                    w = 1.0 / (1.0 + x * x)
                    w = w * line_segment_overlap(self.seg[k, 0:2], self.seg[k, 2:4], ps[k], pe[k])
                    H += J[:, None] * J[None, :] * w
                    g += J * rg * w
                    en += r * r * w
                    N += 1
            e = np.float64(en) / np.float64(N)
            self.H = H
            rec = dict(phase=phase, e=float(e), de=abs(float(e) - err_prev), N=N, x_norm=None, logdet=None)
            self.trace.append(rec)
            if N == 0 or abs(e - err_prev) < p.min_error_change or e < p.min_error:
                break
            x, logdet = qr_solve_logdet(H, g)
            rec["logdet"] = logdet
            if logdet < 0.0:
                bad = True
                break
            T = step_left(T, x)
            rec["x_norm"] = float(np.sqrt((x * x).sum()))
            if rec["x_norm"] < p.min_error_change:
                break
            err_prev = e
        if not bad:
            self.cov, self.err = inverse6(self.H), float(e)
        else:
            T, self.cov, self.err = T_start, np.eye(6), -1.0
        return T

    def remove_outliers(self, T):
        """:1303-1396; the residuals, mean and threshold of each kind are kept for the margins."""
        self.removal = {}
        for kind in (0, 1):
            if not (self.p.has_lines if kind else self.p.has_points):
                continue
            if kind == 0:
                res = self.point_all(T)[0] * np.sqrt(self.ps2)
                flags = self.pin
            else:
                res = self.line_all(T)[0] * np.sqrt(self.ls2)
                flags = self.lin
            mean, stdv = vector_mean_stdv_mad(res)
            th = self.p.inlier_k * stdv
            self.removal[kind] = dict(res=res, mean=mean, th=th)
            flags &= ~(np.abs(res - mean) > th)


def track_pose(prob, params) -> dict:
    """The fields of Solver.track_pose for one problem, plus `trace`, `removal`, `good_first`, `good_final`
    (the figures every decision was taken on)."""
    with np.errstate(all="ignore"):   # a match with z = 0 divides by it, as the function does
        return _track_pose(prob, params)


def _track_pose(prob, params) -> dict:
    q = _Problem(prob, params)
    p = params
    T0 = np.eye(4)
    if p.use_motion_model:
        q.cov = q.prev[16:52].reshape(6, 6).copy()
        if is_good(q.prev[:16], q.cov, q.prev[52]):
            T0 = q.prev[:16].reshape(4, 4).copy()
    T, branch = T0.copy(), OK
    good_first = None
    q.removal = {}
    if q.n_pt + q.n_ln < p.min_features:
        branch, T = FEW_BEFORE, np.eye(4)
    else:
        T1 = q.loop(T0.copy(), p.max_iters, 0)
        good_first = dict(ev=eigenvalues(q.cov), err=q.err)
        if is_good(T1, q.cov, q.err):
            q.remove_outliers(T1)
            if int(q.pin.sum() + q.lin.sum()) >= p.min_features:
                T = q.loop(T0.copy(), p.max_iters_ref, 1)
            else:
                branch, T = FEW_AFTER, np.eye(4)
        else:
            branch, T = FIRST_NOT_GOOD, T0.copy()
            if not q.pluker:
                T = q.loop(T0.copy(), p.max_iters_ref, 1)
    ev = eigenvalues(q.cov)
    good_final = dict(ev=ev, err=q.err)
    if is_good(T, q.cov, q.err) and not np.array_equal(T, np.eye(4)):
        DT = oa.hlm_expmap(oa.hlm_logmap(rl.inverse_se3(T)))
        cov, err_norm, eig = q.cov.copy(), q.err, ev
    else:
        DT, cov, err_norm, eig = np.eye(4), np.zeros((6, 6)), -1.0, np.zeros(6)
        if branch == OK:
            branch = FINAL_NOT_GOOD
    return dict(branch=branch, iters_first=q.iters[0], iters_ref=q.iters[1], n_inl_pt=int(q.pin.sum()),
                n_inl_ln=int(q.lin.sum()), err_norm=float(err_norm), s_p=float(q.s_p), s_l=float(q.s_l),
                DT=np.asarray(DT, np.float64).reshape(4, 4), DT_cov=cov, DT_cov_eig=np.asarray(eig, np.float64),
                DT_solver=T, H=q.H.copy(), pt_inlier=q.pin.astype(np.uint8), ln_inlier=q.lin.astype(np.uint8),
                trace=q.trace, removal=q.removal, good_first=good_first, good_final=good_final)
