"""TEST INFRASTRUCTURE: numpy checker of the endpoint-line hand-rolled LM local BA.

MapHandler::levMarquardtOptimizationLBA (src/mapHandler.cpp:2334-2840; window of
localBundleAdjustment, :1392-1502), restated from its description, vectorised over the
observations. PARITY UNPINNED against the reference itself (it cannot be built here); pinned by
tests/test_lba_endpoints_oracle.py against the per-observation kernels of oracle/refhlm.cpp.

What the function does, as restated here:
  * one scalar residual r = ‖e‖ per observation, Cauchy weight w = 1/(1+r²); H += w·JᵀJ,
    g += w·J·r, err += w·r²; an observation of a fixed keyframe (kf_idx_loc == -1) adds to its
    landmark block and g only;
  * lines are 6-dim landmarks [P; Q], observed as image lines (a, b, c): e = (l·π(P), l·π(Q));
  * first linearisation: map values (point3D, line3D, T_kf_w), err /= (Npt_obs + Nls_obs) == 0
    (+inf), λ = λ0·max|H_ii| (a double), H_ii += λ·H_ii, DX = H⁻¹g applied unconditionally;
  * later linearisations: points and free poses from X; every line observation reads BOTH
    endpoints from X at the aliased offset 6Nkf+3Npt+3·j (P == Q) and always the map pose; the
    line thresholds are the literal 1e-7; err /= (Npt + Nls), the landmark counts;
  * stop if |err − err_prev| < minErrorChange or err < minError; solve; err > err_prev: λ /= k and
    no update, else λ *= k and update; stop if ‖DX‖ < minErrorChange;
  * poses X_i ← logmap(expmap(X_i)·expmap(DX_i)⁻¹), landmarks X += DX; the se(3) maps are the
    reference-ordered restatements of oracle/refhlm.cpp (see pose_update below).
DX comes from an exact block elimination (3×3 / 6×6 landmark blocks by unpivoted LDLᵀ, then the
reduced pose system) or, with ``dense=True``, from the literal N×N H. Pivot policy of
oracle/refhlm.cpp: a zero pivot fails the solve (DX = 0, X unchanged); a free keyframe without
any observation gets 1.0 on its diagonal (DX_i = 0), as the device does (INTEGRATION.md B').
"""
from __future__ import annotations

import numpy as np

import oracle_api as oa

LINE_TH_LATER = 0.0000001   # src/mapHandler.cpp:2717,2737,2743,2757,2760


# se(3) maps: the restatements of src2/auxiliar.cpp:113-173 in oracle/refhlm.cpp, in the reference's
# own operation order. logmap_se3 divides by sin θ (sine = sqrt(1 − cosine²)), so for a keyframe whose
# rotation is close to π any other order of the same formulas moves X_i by ~1e-10 per step.
def _inverse_se3(T):
    Ti = np.zeros(16)
    oa._hlm_lib().refhlm_inverse_se3(oa._p(np.ascontiguousarray(T, np.float64).reshape(16)), oa._p(Ti))
    return Ti.reshape(4, 4)


def _mat4mul(A, B):
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += A[i, k] * B[k, j]
            C[i, j] = s
    return C


def pose_update(x, dx):
    """X_i ← logmap_se3(expmap_se3(X_i)·inverse_se3(expmap_se3(DX_i)))  (:2573-2577, :2818-2822)."""
    return oa.hlm_logmap(_mat4mul(oa.hlm_expmap(x), _inverse_se3(oa.hlm_expmap(dx))))


def tcw_of(x):
    """Tiw = inverse_se3(expmap_se3(X_i)) as a 3x4 (:2617-2621)."""
    return _inverse_se3(oa.hlm_expmap(x))[:3, :]


def _rot(R, X):
    """R·X row by row, summed left to right (the operation order of oracle/refhlm.cpp's mat3vec)."""
    return R[:, :, 0] * X[:, 0:1] + R[:, :, 1] * X[:, 1:2] + R[:, :, 2] * X[:, 2:3]


def _rot_t(j, R):
    """jᵀ·R, summed left to right."""
    return j[:, 0:1] * R[:, 0, :] + j[:, 1:2] * R[:, 1, :] + j[:, 2:3] * R[:, 2, :]


def point_obs(Tcw, X, obs, cam, hth):
    """Batched point observation: Tcw (E,3,4), X (E,3), obs (E,2) -> r, w, Jp (E,6), Jl (E,3)."""
    fx, fy, cx, cy = cam
    R, t = Tcw[:, :, :3], Tcw[:, :, 3]
    G = _rot(R, X) + t
    gx, gy, gz = G[:, 0], G[:, 1], G[:, 2]
    dx = obs[:, 0] - (cx + fx * gx / gz)
    dy = obs[:, 1] - (cy + fy * gy / gz)
    r = np.sqrt(dx * dx + dy * dy)
    gz2 = 1.0 / np.maximum(hth, gz * gz)
    a, b = fx * dx, fy * dy
    m = np.maximum(hth, r)
    j3 = np.stack([gz2 * a * gz, gz2 * b * gz, -gz2 * (a * gx + b * gy)], 1)
    Jp = np.concatenate([j3, np.stack([-gz2 * (a * gx * gy + b * gy * gy + b * gz * gz),
                                       gz2 * (a * gx * gx + a * gz * gz + b * gx * gy),
                                       gz2 * (b * gx * gz - a * gy * gz)], 1)], 1) / m[:, None]
    Jl = _rot_t(j3, R) / m[:, None]
    return r, 1.0 / (1.0 + r * r), Jp, Jl


def line_obs(Tcw, P, Q, lo, cam, hth):
    """Batched endpoint-line observation: image line lo (E,3) -> r, w, Jp (E,6), Jl (E,6)."""
    fx, fy, cx, cy = cam
    R, t = Tcw[:, :, :3], Tcw[:, :, 3]
    G = [_rot(R, V) + t for V in (P, Q)]
    e = [lo[:, 0] * (cx + fx * g[:, 0] / g[:, 2]) + lo[:, 1] * (cy + fy * g[:, 1] / g[:, 2]) + lo[:, 2] for g in G]
    r = np.sqrt(e[0] * e[0] + e[1] * e[1])
    a, b = fx * e[0], fy * e[1]        # fxlx = fx·l_err(0), fyly = fy·l_err(1)
    m = np.maximum(hth, r)
    Jp = np.zeros((len(r), 6))
    Jl = np.zeros((len(r), 6))
    for s, g in enumerate(G):
        gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
        gz2 = 1.0 / np.maximum(hth, gz * gz)
        j3 = np.stack([gz2 * a * gz, gz2 * b * gz, -gz2 * (a * gx + b * gy)], 1)
        j6 = np.concatenate([j3, np.stack([-gz2 * (a * gx * gy + b * gy * gy + b * gz * gz),
                                           gz2 * (a * gx * gx + a * gz * gz + b * gx * gy),
                                           gz2 * (b * gx * gz - a * gy * gz)], 1)], 1)
        Jp += j6 * e[s][:, None]
        Jl[:, 3 * s:3 * s + 3] = _rot_t(j3, R) * e[s][:, None] / m[:, None]
    return r, 1.0 / (1.0 + r * r), Jp / m[:, None], Jl


def ldlt(A):
    """Unpivoted LDLᵀ of a batch of small symmetric matrices (B,D,D) -> L (unit lower), d, ok (B,)."""
    A = A.copy()
    B, D, _ = A.shape
    L = np.zeros_like(A)
    d = np.zeros((B, D))
    ok = np.ones(B, bool)
    for j in range(D):
        dj = A[:, j, j] - np.einsum("bk,bk,bk->b", L[:, j, :j], L[:, j, :j], d[:, :j])
        ok &= dj != 0.0
        d[:, j] = dj
        L[:, j, j] = 1.0
        with np.errstate(all="ignore"):
            for i in range(j + 1, D):
                L[:, i, j] = (A[:, i, j] - np.einsum("bk,bk,bk->b", L[:, i, :j], L[:, j, :j], d[:, :j])) / dj
    return L, d, ok


def ldlt_solve(L, d, Bm):
    """Solve with the factors of :func:`ldlt`; Bm (B,D,K)."""
    D = L.shape[1]
    Y = Bm.copy()
    for i in range(D):
        Y[:, i] -= np.einsum("bk,bkc->bc", L[:, i, :i], Y[:, :i])
    with np.errstate(all="ignore"):
        Y /= d[:, :, None]
    for i in range(D - 1, -1, -1):
        Y[:, i] -= np.einsum("bk,bkc->bc", L[:, i + 1:, i], Y[:, i + 1:])
    return Y


class Problem:
    """The window as the reference's lists: free KFs in id order, then points, then lines."""

    def __init__(self, win, params):
        g = self.g = win.graph
        self.p = params
        self.cam = (g.fx, g.fy, g.cx, g.cy)
        order = np.argsort(g.kf_id, kind="stable")
        self.hidx = np.full(g.n_kf, -1)
        free = [k for k in order if not g.kf_fixed[k]]
        self.hidx[free] = np.arange(len(free))
        self.free = np.asarray(free, int)
        self.nf, self.n_pt, self.n_ln = len(free), g.n_pt, g.n_ln
        self.N = 6 * self.nf + 3 * self.n_pt + 6 * self.n_ln
        self.Tmap = np.asarray(g.kf_Tcw, np.float64).reshape(-1, 3, 4)
        self.ept_obs = np.asarray(g.ept_obs, np.float64).reshape(-1, 2)
        self.eln_obs = np.asarray(g.eln_obs, np.float64).reshape(-1, 4)[:, :3]
        self.ept_kf, self.ept_lm = np.asarray(g.ept_kf, int), np.asarray(g.ept_lm, int)
        self.eln_kf, self.eln_lm = np.asarray(g.eln_kf, int), np.asarray(g.eln_lm, int)
        # state
        self.xk = np.asarray(win.kf_x, np.float64).reshape(-1, 6).copy()
        self.Xp = np.asarray(g.pt_xyz, np.float64).reshape(-1, 3).copy()
        self.Xl = np.asarray(win.ln_line3d, np.float64).reshape(-1, 6).copy() if g.n_ln else np.zeros((0, 6))

    def tcw_from_x(self):
        T = self.Tmap.copy()
        for k in self.free:
            T[k] = tcw_of(self.xk[k])
        return T

    def linearize(self, first):
        p = self.p
        Tp = self.Tmap if first else self.tcw_from_x()
        rp, wp, Jpp, Jlp = point_obs(Tp[self.ept_kf], self.Xp[self.ept_lm], self.ept_obs, self.cam, p.homog_th)
        if first:
            P, Q = self.Xl[self.eln_lm, :3], self.Xl[self.eln_lm, 3:]
            hth = p.homog_th
        else:  # both endpoints from the 6-dim blocks read at a stride of 3 (:2697-2698)
            flat = self.Xl.reshape(-1)
            P = Q = flat[3 * self.eln_lm[:, None] + np.arange(3)[None, :]].reshape(-1, 3)
            hth = LINE_TH_LATER
        rl, wl, Jpl, Jll = line_obs(self.Tmap[self.eln_kf], P, Q, self.eln_obs, self.cam, hth)
        lin = dict(rp=rp, wp=wp, Jpp=Jpp, Jlp=Jlp, rl=rl, wl=wl, Jpl=Jpl, Jll=Jll,
                   hp=self.hidx[self.ept_kf], hl=self.hidx[self.eln_kf])
        nf = self.nf
        Hpp, gp = np.zeros((nf, 6, 6)), np.zeros((nf, 6))
        for h, J, w, r in ((lin["hp"], Jpp, wp, rp), (lin["hl"], Jpl, wl, rl)):
            f = h >= 0
            np.add.at(Hpp, h[f], (w[f, None, None] * J[f, :, None]) * J[f, None, :])
            np.add.at(gp, h[f], J[f] * (w[f] * r[f])[:, None])
        Hpt, gpt = np.zeros((self.n_pt, 3, 3)), np.zeros((self.n_pt, 3))
        np.add.at(Hpt, self.ept_lm, (wp[:, None, None] * Jlp[:, :, None]) * Jlp[:, None, :])
        np.add.at(gpt, self.ept_lm, Jlp * (wp * rp)[:, None])
        Hln, gln = np.zeros((self.n_ln, 6, 6)), np.zeros((self.n_ln, 6))
        np.add.at(Hln, self.eln_lm, (wl[:, None, None] * Jll[:, :, None]) * Jll[:, None, :])
        np.add.at(gln, self.eln_lm, Jll * (wl * rl)[:, None])
        lin.update(Hpp=Hpp, gp=gp, Hpt=Hpt, gpt=gpt, Hln=Hln, gln=gln)
        chi = float(np.sum(wp * rp * rp) + np.sum(wl * rl * rl))
        nobs = len(rp) + len(rl)
        if p.err_per_obs:
            div = float(nobs)
        else:
            div = 0.0 if first else float(self.n_pt + self.n_ln)   # :2551 / :2796
        with np.errstate(all="ignore"):
            lin["err"] = float(np.float64(chi) / np.float64(div))
        # free keyframes with at least one observation (the others get the unit diagonal)
        act = np.zeros(nf, bool)
        act[lin["hp"][lin["hp"] >= 0]] = True
        act[lin["hl"][lin["hl"] >= 0]] = True
        lin["pose_active"] = act
        return lin

    @staticmethod
    def hmax(lin):
        m = 0.0
        for H in (lin["Hpp"], lin["Hpt"], lin["Hln"]):
            if H.size:
                m = max(m, float(np.abs(np.diagonal(H, axis1=1, axis2=2)).max()))
        return m

    # ---- DX = (H + λ·diag H)⁻¹ g
    def solve(self, lin, lam, dense=False):
        return self._solve_dense(lin, lam) if dense else self._solve_schur(lin, lam)

    def _damped_pose_blocks(self, lin, lam):
        A = lin["Hpp"].copy()
        i6 = np.arange(6)
        A[:, i6, i6] += lam * A[:, i6, i6]
        for k in np.nonzero(~lin["pose_active"])[0]:
            A[k, i6, i6] = 1.0
        return A

    def _solve_dense(self, lin, lam):
        nf, n_pt, N = self.nf, self.n_pt, self.N
        H, gv = np.zeros((N, N)), np.zeros(N)
        for h in range(nf):
            H[6 * h:6 * h + 6, 6 * h:6 * h + 6] = lin["Hpp"][h]
            gv[6 * h:6 * h + 6] = lin["gp"][h]
        o = 6 * nf
        for l in range(n_pt):
            H[o + 3 * l:o + 3 * l + 3, o + 3 * l:o + 3 * l + 3] = lin["Hpt"][l]
            gv[o + 3 * l:o + 3 * l + 3] = lin["gpt"][l]
        o2 = o + 3 * n_pt
        for l in range(self.n_ln):
            H[o2 + 6 * l:o2 + 6 * l + 6, o2 + 6 * l:o2 + 6 * l + 6] = lin["Hln"][l]
            gv[o2 + 6 * l:o2 + 6 * l + 6] = lin["gln"][l]
        for h, lm, Jp, Jl, w, base, D in ((lin["hp"], self.ept_lm, lin["Jpp"], lin["Jlp"], lin["wp"], o, 3),
                                          (lin["hl"], self.eln_lm, lin["Jpl"], lin["Jll"], lin["wl"], o2, 6)):
            for e in np.nonzero(h >= 0)[0]:
                blk = w[e] * np.outer(Jl[e], Jp[e])
                c0, r0 = base + D * lm[e], 6 * h[e]
                H[c0:c0 + D, r0:r0 + 6] += blk
                H[r0:r0 + 6, c0:c0 + D] += blk.T
        dg = np.arange(N)
        H[dg, dg] += lam * H[dg, dg]
        for k in np.nonzero(~lin["pose_active"])[0]:
            H[6 * k + np.arange(6), 6 * k + np.arange(6)] = 1.0
        if np.any(H[dg, dg] == 0.0):
            return False, np.zeros(N)
        try:
            return True, np.linalg.solve(H, gv)
        except np.linalg.LinAlgError:
            return False, np.zeros(N)

    def _solve_schur(self, lin, lam):
        nf, n_pt, n_ln, N = self.nf, self.n_pt, self.n_ln, self.N
        zero = np.zeros(N)
        n = 6 * nf
        S4 = np.zeros((nf, nf, 6, 6))
        hh = np.arange(nf)
        S4[hh, hh] = self._damped_pose_blocks(lin, lam)
        bs = lin["gp"].copy()
        fac = []
        for H, gl, h, lm, Jp, Jl, w, D, nl in ((lin["Hpt"], lin["gpt"], lin["hp"], self.ept_lm, lin["Jpp"], lin["Jlp"],
                                                lin["wp"], 3, n_pt),
                                               (lin["Hln"], lin["gln"], lin["hl"], self.eln_lm, lin["Jpl"], lin["Jll"],
                                                lin["wl"], 6, n_ln)):
            if nl == 0:
                fac.append(None)
                continue
            A = H.copy()
            iD = np.arange(D)
            A[:, iD, iD] += lam * A[:, iD, iD]
            L, d, ok = ldlt(A)
            if not ok.all():
                return False, zero
            y = ldlt_solve(L, d, gl[:, :, None])[:, :, 0]          # D⁻¹ g_l
            f = np.nonzero(h >= 0)[0]
            # per free observation: v_e = D_l⁻¹ Jl_e
            V = np.zeros((len(h), D))
            # solve per landmark with all its observations' rows at once: group by landmark
            V[f] = self._solve_rows(L, d, lm[f], Jl[f])
            fac.append((L, d, f, V))
            # b_s -= W_e y = Jp_e w_e (Jl_e · y_l)
            np.add.at(bs, h[f], -Jp[f] * (w[f] * np.einsum("ei,ei->e", Jl[f], y[lm[f]]))[:, None])
            # S -= Σ_{a,b of one landmark} w_a w_b (Jl_a · v_b) Jp_a Jp_bᵀ
            order = f[np.argsort(lm[f], kind="stable")]
            lms = lm[order]
            start = np.r_[0, np.nonzero(np.diff(lms))[0] + 1] if len(lms) else np.zeros(0, int)
            cnt = np.diff(np.r_[start, len(lms)]) if len(lms) else np.zeros(0, int)
            for k in np.unique(cnt):
                grp = start[cnt == k][:, None] + np.arange(k)[None, :]        # (G,k) positions in `order`
                ee = order[grp]                                              # (G,k) observation indices
                s = np.einsum("gai,gbi->gab", Jl[ee], V[ee]) * w[ee][:, :, None] * w[ee][:, None, :]
                blocks = s[:, :, :, None, None] * Jp[ee][:, :, None, :, None] * Jp[ee][:, None, :, None, :]
                key = (h[ee][:, :, None] * nf + h[ee][:, None, :]).reshape(-1)
                blocks = blocks.reshape(-1, 36)
                Sf = S4.reshape(nf * nf, 36)
                for c in range(36):
                    Sf[:, c] -= np.bincount(key, weights=blocks[:, c], minlength=nf * nf)
        S = S4.transpose(0, 2, 1, 3).reshape(n, n)
        DX = np.zeros(N)
        if n:
            if np.any(np.diagonal(S) == 0.0):
                return False, zero
            try:
                xp = np.linalg.solve(S, bs.reshape(-1))
            except np.linalg.LinAlgError:
                return False, zero
            DX[:n] = xp
        xp6 = DX[:n].reshape(nf, 6)
        off = n
        for fc, gl, h, lm, Jp, Jl, w, D, nl in ((fac[0], lin["gpt"], lin["hp"], self.ept_lm, lin["Jpp"], lin["Jlp"],
                                                 lin["wp"], 3, n_pt),
                                                (fac[1], lin["gln"], lin["hl"], self.eln_lm, lin["Jpl"], lin["Jll"],
                                                 lin["wl"], 6, n_ln)):
            if nl == 0:
                continue
            L, d, f, _ = fc
            rr = gl.copy()                                           # x_l = D⁻¹ (g_l − Σ W_eᵀ x_p)
            np.add.at(rr, lm[f], -Jl[f] * (w[f] * np.einsum("ei,ei->e", Jp[f], xp6[h[f]]))[:, None])
            DX[off:off + D * nl] = ldlt_solve(L, d, rr[:, :, None])[:, :, 0].reshape(-1)
            off += D * nl
        return True, DX

    @staticmethod
    def _solve_rows(L, d, lm, rows):
        """D_l⁻¹ row for each (landmark, row) pair: gathers the landmark's factors per row."""
        return ldlt_solve(L[lm], d[lm], rows[:, :, None])[:, :, 0]

    def apply(self, DX):
        nf, n_pt = self.nf, self.n_pt
        for h, k in enumerate(self.free):
            self.xk[k] = pose_update(self.xk[k], DX[6 * h:6 * h + 6])
        o = 6 * nf
        self.Xp += DX[o:o + 3 * n_pt].reshape(-1, 3)
        self.Xl += DX[o + 3 * n_pt:].reshape(-1, 6)


TRACE_DT = np.dtype([("stage", np.int32), ("iter", np.int32), ("trials", np.int32), ("result", np.int32),
                     ("chi2_start", np.float64), ("chi2_end", np.float64),
                     ("lambda_start", np.float64), ("lambda_end", np.float64)])


def lba(win, params, dense: bool = False) -> dict:
    """The whole loop; returns the fields of Solver.hlm_lba (plba.capi.HlmResultBuffers.as_dict)."""
    pb = Problem(win, params)
    p = params
    lam, err, err_prev, dxn = float(p.lambda0), 0.0, 999999999.9, 0.0
    lins = solves = acc = 0
    trace = []
    n_obs = pb.g.n_ept + pb.g.n_eln
    if pb.N > 0 and n_obs > 0:
        lin = pb.linearize(True)
        lins += 1
        err = lin["err"]
        lam *= pb.hmax(lin)                      # Hmax is a double here (:2555-2561)
        l0 = lam
        solves += 1
        ok, DX = pb.solve(lin, lam, dense)
        if ok:
            pb.apply(DX)
            acc += 1
        dxn = float(np.linalg.norm(DX))
        trace.append((0, 0, 1, 0, err, err, l0, lam))
        err_prev = err
        for it in range(1, int(p.max_iters)):
            lin = pb.linearize(False)
            lins += 1
            err = lin["err"]
            l0 = lam
            if abs(err - err_prev) < p.min_error_change or err < p.min_error:
                trace.append((0, it, 1, 3, err, err, l0, lam))
                break
            solves += 1
            ok, DX = pb.solve(lin, lam, dense)
            dxn = float(np.linalg.norm(DX))
            if err > err_prev:
                lam /= p.lambda_k
                trace.append((0, it, 1, 1, err, err, l0, lam))
            else:
                lam *= p.lambda_k
                if ok:
                    pb.apply(DX)
                    acc += 1
                trace.append((0, it, 1, 0, err, err, l0, lam))
            if dxn < p.min_error_change:
                break
            err_prev = err
    return dict(kf_x=pb.xk, kf_Tcw=pb.tcw_from_x(), pt_xyz=pb.Xp, ln_line3d=pb.Xl,
                ln_orth=np.zeros((pb.n_ln, 4)), linearizations=lins, solves=solves, accepted=acc,
                err=err, lam=lam, dx_norm=dxn, trace=np.array(trace, TRACE_DT))
