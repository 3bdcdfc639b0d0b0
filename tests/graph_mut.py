"""Graph mutations for edge-case parity tests (shuffles, duplicates, fixed/idle vertices)."""
import numpy as np

from plba.synth import Graph


def shuffled(g: Graph, seed=0) -> Graph:
    """Permute edge order, vertex array order and vertex ids (keeps the same optimisation
    problem up to g2o's id-based ordering)."""
    rng = np.random.default_rng(seed)
    h = g.copy()
    # permute keyframe array order, keep ids attached
    pk = rng.permutation(g.n_kf)
    inv_k = np.argsort(pk)
    h.kf_Tcw, h.kf_fixed, h.kf_id = g.kf_Tcw[pk], g.kf_fixed[pk], g.kf_id[pk]
    h.ept_kf = inv_k[g.ept_kf].astype(np.int32)
    h.eln_kf = inv_k[g.eln_kf].astype(np.int32)
    pp = rng.permutation(g.n_pt)
    inv_p = np.argsort(pp)
    h.pt_xyz, h.pt_id = g.pt_xyz[pp], g.pt_id[pp]
    h.ept_lm = inv_p[g.ept_lm].astype(np.int32)
    # edges in random order
    pe = rng.permutation(g.n_ept)
    h.ept_lm, h.ept_kf, h.ept_obs, h.ept_info = h.ept_lm[pe], h.ept_kf[pe], g.ept_obs[pe], g.ept_info[pe]
    pl = rng.permutation(g.n_eln)
    h.eln_lm, h.eln_kf, h.eln_obs, h.eln_info = g.eln_lm[pl], h.eln_kf[pl], g.eln_obs[pl], g.eln_info[pl]
    h._perm = dict(pk=pk, pp=pp, pe=pe, pl=pl)
    return h


def with_duplicate_observations(g: Graph, every=7) -> Graph:
    """Append a second, slightly different observation of some landmarks by the same KF."""
    h = g.copy()
    sel = np.arange(0, g.n_ept, every)
    h.ept_lm = np.concatenate([g.ept_lm, g.ept_lm[sel]]).astype(np.int32)
    h.ept_kf = np.concatenate([g.ept_kf, g.ept_kf[sel]]).astype(np.int32)
    h.ept_obs = np.concatenate([g.ept_obs, g.ept_obs[sel] + 0.3])
    h.ept_info = np.concatenate([g.ept_info, g.ept_info[sel]])
    return h


def drop_lines(g: Graph) -> Graph:
    h = g.copy()
    h.ln_orth, h.ln_id = g.ln_orth[:0], g.ln_id[:0]
    h.eln_lm, h.eln_kf, h.eln_obs, h.eln_info = g.eln_lm[:0], g.eln_kf[:0], g.eln_obs[:0], g.eln_info[:0]
    return h


def drop_points(g: Graph) -> Graph:
    h = g.copy()
    h.pt_xyz, h.pt_id = g.pt_xyz[:0], g.pt_id[:0]
    h.ept_lm, h.ept_kf, h.ept_obs, h.ept_info = g.ept_lm[:0], g.ept_kf[:0], g.ept_obs[:0], g.ept_info[:0]
    return h


def all_fixed(g: Graph) -> Graph:
    h = g.copy()
    h.kf_fixed = np.ones_like(g.kf_fixed)
    return h


def free_rows(g: Graph) -> np.ndarray:
    """Array indices of the free keyframes in increasing kf_id: entry r is row r of the reduced
    camera system as g2o builds it (and as the solver factorises it when no reordering runs)."""
    free = np.nonzero(g.kf_fixed == 0)[0]
    return free[np.argsort(g.kf_id[free], kind="stable")]


def add_idle_free_pose(g: Graph, row=None) -> Graph:
    """A free keyframe that no edge observes (inactive in g2o, must stay untouched). It is the
    last array entry. row: its position among the free poses of the new window in increasing
    kf_id (negative: from the end); every vertex id at or above the one it takes moves up by one.
    Default: the id after the largest keyframe id."""
    h = g.copy()
    h.kf_Tcw = np.concatenate([g.kf_Tcw, g.kf_Tcw[-1:]])
    h.kf_fixed = np.concatenate([g.kf_fixed, np.zeros(1, np.uint8)])
    if row is None:
        h.kf_id = np.concatenate([g.kf_id, np.array([g.kf_id.max() + 1], np.int32)])
        return h
    ids = g.kf_id[free_rows(g)]
    r = row + len(ids) + 1 if row < 0 else row
    assert 0 <= r <= len(ids), (row, len(ids))
    new = int(ids[r]) if r < len(ids) else int(ids[-1]) + 1 if len(ids) else int(g.kf_id.max(initial=-1)) + 1
    h.kf_id = np.concatenate([g.kf_id + (g.kf_id >= new), np.array([new])]).astype(np.int32)
    h.pt_id = (g.pt_id + (g.pt_id >= new)).astype(np.int32)
    h.ln_id = (g.ln_id + (g.ln_id >= new)).astype(np.int32)
    return h


def fixed_only_landmarks(g: Graph) -> Graph:
    """Re-point the edges of the first landmarks to fixed keyframes only."""
    h = g.copy()
    fixed = np.nonzero(g.kf_fixed)[0]
    sel = g.ept_lm < 20
    h.ept_kf = np.where(sel, fixed[np.arange(g.n_ept) % len(fixed)], g.ept_kf).astype(np.int32)
    return h


def camera_centres(g: Graph) -> np.ndarray:
    """C_k = −Rᵀt of every keyframe estimate, (n_kf, 3)."""
    return -np.einsum("kji,kj->ki", g.kf_Tcw[:, :, :3], g.kf_Tcw[:, :, 3])


def point_depths(kf_Tcw, pt_xyz, ept_kf, ept_lm) -> np.ndarray:
    """Camera-frame depth Pc[2] = R₂·P + t₂ of every point edge at the given estimates."""
    T = np.asarray(kf_Tcw)[ept_kf]
    return np.einsum("ej,ej->e", T[:, 2, :3], np.asarray(pt_xyz)[ept_lm]) + T[:, 2, 3]


def points_behind_cameras(g: Graph, every=7, count=20, through="first") -> Graph:
    """Reflect some point landmarks through a camera centre: P_j <- 2·C − P_j. The landmarks are
    every `every`-th one, `count` at the most; C is the centre of the first keyframe (in edge
    order) that observes the landmark ("first"), or the mean of its observing centres ("mean").
    "short" takes its landmarks among those with at most 3 observations only, and reflects through
    the first observer. A reflection through a camera's centre keeps that camera's projection and
    makes its depth negative: the window stays finite, with a small χ² in that view and large ones
    in the others. The chosen landmarks are left in `_behind`."""
    assert through in ("first", "mean", "short"), through
    h = g.copy()
    nobs = np.bincount(g.ept_lm, minlength=g.n_pt)
    cand = np.nonzero(nobs > 0)[0]
    if through == "short":
        cand = cand[nobs[cand] <= 3]
    sel = cand[::every][:count]
    C = camera_centres(g)
    for j in sel:
        kfs = g.ept_kf[g.ept_lm == j]
        c = C[kfs].mean(axis=0) if through == "mean" else C[kfs[0]]
        h.pt_xyz[j] = 2.0 * c - g.pt_xyz[j]
    h._behind = sel
    return h


def zero_information_keyframe(g: Graph, row=None) -> Graph:
    """Ω = 0 on every edge of one free keyframe: the vertex stays active (it has edges) but its
    reduced-camera block row is exactly zero, so with λ = 0 the LDLᵀ meets an exact zero pivot
    in any elimination order (g2o's LinearSolverEigen fails there too). row: the keyframe's
    position among the free poses in increasing kf_id (negative: from the end). Default: the
    middle free keyframe in array order."""
    h = g.copy()
    free = np.nonzero(g.kf_fixed == 0)[0]
    k = free[len(free) // 2] if row is None else free_rows(g)[row]
    h.ept_info = np.where(g.ept_kf == k, 0.0, g.ept_info)
    h.eln_info = np.where(g.eln_kf == k, 0.0, g.eln_info)
    return h
