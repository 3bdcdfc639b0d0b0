"""TEST INFRASTRUCTURE: numpy checker of the loop-closure relative pose.

MapHandler::computeRelativePoseRobustGN (src/mapHandler.cpp:4677-5068; variant 0, what
isLoopClosure calls) and MapHandler::computeRelativePoseGN (:4413-4675; variant 1), restated from
their description. PARITY UNPINNED against the reference itself (it cannot be built here); pinned
by tests/test_lcpose_oracle.py (finite differences, convergence, the kept quirks).

What the functions do, as restated here:
  * T_inc = I, err_prev = 999999999.9;
  * a pass over the active matches: P_ = R·P + t, projected with cx + fx·X/Z, cy + fy·Y/Z; points
    e = proj − obs, lines e = (l·π(sP_), l·π(eP_)); r = ‖e‖; the row J built with fx in BOTH image
    directions and max(homog_th, z²), divided by max(homog_th, r) (lines: (Js·ds + Je·de)/max(..));
    w = 1/(1+r²); H += J·Jᵀ·w, g += J·r·w, e += r·r·w; points then lines, in feature order;
  * e /= N_p + N_l; stop if |e − err_prev| < ε or e < ε; x = H⁻¹g (column-pivoted Householder QR);
    T_inc ← T_inc · inverse_se3(expmap_se3(x)) — on the right; stop if ‖x‖ < ε; err_prev = e;
  * at most max_iters_first passes; then every active match with ‖e‖ > sqrt(7.815) is deactivated;
    variant 0 then runs at most max_iters more passes (err_prev carried over, not reset);
  * x_inc = logmap_se3(T_inc), t = ‖x_inc[0:3]‖, r = ‖x_inc[3:6]‖·180/π, unc = the largest
    eigenvalue of H⁻¹; accepted iff e < lc_res, unc < lc_unc, inliers/matches > lc_inl (variant 0:
    forced true), t < lc_trs, r < lc_rot;
  * pose_inc = logmap(inverse(expmap(x_inc))) (variant 0) / logmap(inverse(T_inc)) (variant 1).
Defined where the reference is not, as the device does: no active match -> accepted = 0 and T_inc
stays; a singular H (inv fails or is not finite) -> unc = +inf; a non-finite H or g (a match with
z = 0) -> x = NaN and no exception, after which every comparison is false.
The se(3) maps are the reference-ordered restatements of oracle/refhlm.cpp.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

import oracle_api as oa

EPS = float(np.finfo(np.float64).eps)
OUTLIER_TH = float(np.sqrt(7.815))
ERR_PREV0 = 999999999.9


def inverse_se3(T):
    Ti = np.zeros(16)
    oa._hlm_lib().refhlm_inverse_se3(oa._p(np.ascontiguousarray(T, np.float64).reshape(16)), oa._p(Ti))
    return Ti.reshape(4, 4)


def mat4mul(A, B):
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += A[i, k] * B[k, j]
            C[i, j] = s
    return C


def step_right(T, x):
    """T · inverse_se3(expmap_se3(x))  (:4815)."""
    return mat4mul(T, inverse_se3(oa.hlm_expmap(x)))


def xform(T, P):
    """T.block(0,0,3,3)·P + T.col(3).head(3), rows summed left to right; P (N,3)."""
    return np.stack([((T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]) + T[i, 2] * P[:, 2]) + T[i, 3] for i in range(3)], 1)


def project(G, cam):
    fx, fy, cx, cy = cam
    return cx + fx * G[:, 0] / G[:, 2], cy + fy * G[:, 1] / G[:, 2]


def jrow(G, a, b, cam, hth):
    """The six entries of :4724-4729 / :4769-4774 for the projected points G and the image direction (a, b)."""
    gx, gy, gz = G[:, 0], G[:, 1], G[:, 2]
    gz2 = gz * gz
    fgz2 = cam[0] / np.maximum(hth, gz2)
    return np.stack([+fgz2 * a * gz,
                     +fgz2 * b * gz,
                     -fgz2 * (gx * a + gy * b),
                     -fgz2 * (gx * gy * a + gy * gy * b + gz * gz * b),
                     +fgz2 * (gx * gx * a + gz * gz * a + gx * gy * b),
                     +fgz2 * (gx * gz * b - gy * gz * a)], 1)


def point_res(T, P, obs, cam):
    G = xform(T, P)
    u, v = project(G, cam)
    dx, dy = u - obs[:, 0], v - obs[:, 1]
    return np.sqrt(dx * dx + dy * dy), dx, dy, G


def line_res(T, sP, eP, le, cam):
    Gs, Ge = xform(T, sP), xform(T, eP)
    us, vs = project(Gs, cam)
    ue, ve = project(Ge, cam)
    ds = le[:, 0] * us + le[:, 1] * vs + le[:, 2]
    de = le[:, 0] * ue + le[:, 1] * ve + le[:, 2]
    return np.sqrt(ds * ds + de * de), ds, de, Gs, Ge


def point_rows(T, P, obs, cam, hth):
    """r (N,), J (N,6) of the point matches."""
    r, dx, dy, G = point_res(T, P, obs, cam)
    return r, jrow(G, dx, dy, cam, hth) / np.maximum(hth, r)[:, None]


def line_rows(T, sP, eP, le, cam, hth):
    r, ds, de, Gs, Ge = line_res(T, sP, eP, le, cam)
    Js, Je = jrow(Gs, le[:, 0], le[:, 1], cam, hth), jrow(Ge, le[:, 0], le[:, 1], cam, hth)
    return r, (Js * ds[:, None] + Je * de[:, None]) / np.maximum(hth, r)[:, None]


def qr_solve(H, g):
    """x = ColPivHouseholderQR(H).solve(g): rank by Eigen's pivot threshold, the rest of x zero.
    A non-finite H or g (a match with z = 0) gives a NaN x: no comparison with a NaN norm holds, so
    no rank is dropped, and the reflections spread the NaN over every entry."""
    if not (np.isfinite(H).all() and np.isfinite(g).all()):
        return np.full(6, np.nan)
    Q, R, P = scipy.linalg.qr(H, pivoting=True)
    thr = (np.sqrt((H * H).sum(axis=0).max()) * EPS / 6.0) ** 2
    nz = 6
    for k in range(6):
        if R[k, k] * R[k, k] < thr * (6 - k):
            nz = k
            break
    x = np.zeros(6)
    if nz:
        y = scipy.linalg.solve_triangular(R[:nz, :nz], (Q.T @ g)[:nz])
        x[P[:nz]] = y
    return x


def uncertainty(H):
    """The largest eigenvalue of H⁻¹ (:4993-4997); +inf for a singular H."""
    try:
        with np.errstate(all="ignore"):
            C = np.linalg.inv(H)
        if not np.isfinite(C).all():
            return float("inf")
        return float(np.linalg.eigvalsh(C)[-1])
    except np.linalg.LinAlgError:
        return float("inf")


def relative_pose(prob, params) -> dict:
    """The fields of Solver.lc_relative_pose for one candidate, plus the residuals of the outlier pass
    (`out_res_pt`, `out_res_ln`: ‖e‖ of the matches it tested, NaN for the others)."""
    with np.errstate(all="ignore"):   # a match with z = 0 divides by it, as the function does
        return _relative_pose(prob, params)


def _relative_pose(prob, params) -> dict:
    p = params
    cam = tuple(float(v) for v in prob.cam)
    hth = float(p.homog_th)
    P, obs = np.asarray(prob.pt_P, np.float64).reshape(-1, 3), np.asarray(prob.pt_obs, np.float64).reshape(-1, 2)
    sP, eP = np.asarray(prob.ln_sP, np.float64).reshape(-1, 3), np.asarray(prob.ln_eP, np.float64).reshape(-1, 3)
    le = np.asarray(prob.ln_le, np.float64).reshape(-1, 3)
    n_pt, n_ln = len(P), len(sP)
    pin, lin = np.ones(n_pt, bool), np.ones(n_ln, bool)
    T = np.eye(4)
    H, e, err_prev, empty = np.zeros((6, 6)), 0.0, ERR_PREV0, False
    iters = [0, 0]

    def loop(cap, phase):
        nonlocal T, H, e, err_prev, empty
        for _ in range(int(cap)):
            iters[phase] += 1
            rp, Jp = point_rows(T, P[pin], obs[pin], cam, hth)
            rl, Jl = line_rows(T, sP[lin], eP[lin], le[lin], cam, hth)
            N = len(rp) + len(rl)
            if N == 0:
                empty = True
                return
            Hn, g, en = np.zeros((6, 6)), np.zeros(6), 0.0
            for r, J in ((rp, Jp), (rl, Jl)):            # points, then lines, in feature order
                w = 1.0 / (1.0 + r * r)
                for k in range(len(r)):
                    Hn += J[k][:, None] * J[k][None, :] * w[k]
                    g += J[k] * r[k] * w[k]
                    en += r[k] * r[k] * w[k]
            H, e = Hn, en / N
            if abs(e - err_prev) < EPS or e < EPS:
                return
            x = qr_solve(H, g)
            T = step_right(T, x)
            if np.sqrt((x * x).sum()) < EPS:
                return
            err_prev = e

    loop(p.max_iters_first, 0)
    # outlier pass (:4829-4860)
    out_res_pt, out_res_ln = np.full(n_pt, np.nan), np.full(n_ln, np.nan)
    if pin.any():
        out_res_pt[pin] = point_res(T, P[pin], obs[pin], cam)[0]
    if lin.any():
        out_res_ln[lin] = line_res(T, sP[lin], eP[lin], le[lin], cam)[0]
    pin &= ~(out_res_pt > OUTLIER_TH)
    lin &= ~(out_res_ln > OUTLIER_TH)
    if int(p.variant) == 0:
        loop(p.max_iters, 1)
    x_inc = oa.hlm_logmap(T)
    t = float(np.sqrt(x_inc[0] * x_inc[0] + x_inc[1] * x_inc[1] + x_inc[2] * x_inc[2]))
    r_deg = float(np.sqrt(x_inc[3] * x_inc[3] + x_inc[4] * x_inc[4] + x_inc[5] * x_inc[5]) * 180.0 / np.pi)
    unc = uncertainty(H)
    n_inl, n_all = int(pin.sum() + lin.sum()), n_pt + n_ln
    with np.errstate(all="ignore"):
        ratio = np.float64(n_inl) / np.float64(n_all)
    cond = 0
    cond |= 1 if e < p.lc_res else 0
    cond |= 2 if unc < p.lc_unc else 0
    cond |= 4 if (int(p.variant) == 0 or ratio > p.lc_inl) else 0
    cond |= 8 if t < p.lc_trs else 0
    cond |= 16 if r_deg < p.lc_rot else 0
    if int(p.variant) == 0:
        pose_inc = oa.hlm_logmap(inverse_se3(oa.hlm_expmap(x_inc)))
    else:
        pose_inc = oa.hlm_logmap(inverse_se3(T))
    return dict(accepted=int(cond == 31 and not empty), conditions=cond, iters_first=iters[0], iters_ref=iters[1],
                n_inl_pt=int(pin.sum()), n_inl_ln=int(lin.sum()), e=float(e), unc=unc, t=t, r_deg=r_deg,
                x_inc=x_inc, pose_inc=pose_inc, T_inc=T[:3, :].copy(), H=H.copy(),
                pt_inlier=pin.astype(np.uint8), ln_inlier=lin.astype(np.uint8),
                out_res_pt=out_res_pt, out_res_ln=out_res_ln, empty=empty)


def margins(prob, params) -> dict:
    """How far the candidate is from every decision of the function: the smallest |‖e‖ − sqrt(7.815)| of
    the outlier pass and the relative distance of e, unc, t, r_deg to their thresholds."""
    ref = relative_pose(prob, params)
    res = np.concatenate([ref["out_res_pt"], ref["out_res_ln"]])
    res = res[np.isfinite(res)]
    p = params
    rel = {k: abs(ref[k] - th) / abs(th) for k, th in (("e", p.lc_res), ("unc", p.lc_unc), ("t", p.lc_trs),
                                                      ("r_deg", p.lc_rot))}
    return dict(outlier=float(np.abs(res - OUTLIER_TH).min()) if len(res) else float("inf"), **rel)
