// plba_assoc_plan.hpp — the host decisions of the stereo, the keyframe and the map association (and the median
// descriptor) that need no device: the problem table of a batch and the block layout of a call, array
// by array in block order. Standard C++ only, like csrc/plba_layout.hpp, so that
// tests/cpp/layout_check.cpp runs what csrc/plba_assoc.hip runs.
#pragma once

#include "plba_assoc_args.hpp"
#include "plba_layout.hpp"

namespace plba {

// The points / lines by side-1 / side-2 table of a batch of n units (frames, keyframe pairs). Unit f is
// the matcher's problems 2 f (its points) and 2 f + 1 (its lines); side 1 holds a problem's query rows,
// side 2 its train rows. Each of the four offset arrays has n + 1 entries that start at >= 0 and never
// decrease (the caller has checked that, and n <= (INT32_MAX - 1) / 2); rows count from the first
// unit's offset. A train row owns one cell if it is a point and max(cols, rows) cells if it is a line.
struct ProblemTable {
    enum { kOk = 0, kTooMany, kTooWide };  // what init() returns
    struct Problem {
        int f, kind, a1, r1, a2, r2;  // unit, 0 points / 1 lines, first row and rows of side 1, of side 2
    };
    const int32_t *offs[2][2];  // [kind][side]
    int n, stride;
    size_t cnt[2][2], N1, N2, nc;      // rows of a kind and side, rows of a side, cells of side 2
    int max_rows, max_prev, max_train;  // of one problem: its longer side, side 1, side 2

    // kTooMany: N1, N2 or nc is above INT32_MAX; kTooWide: max_train is above kGmMaxTrain, the low 16 bits of a key
    int init(const int32_t *pt1, const int32_t *pt2, const int32_t *ls1, const int32_t *ls2, int n_, int cols, int rows) {
        offs[0][0] = pt1, offs[0][1] = pt2, offs[1][0] = ls1, offs[1][1] = ls2;
        n = n_, stride = std::max(cols, rows);  // a walk's cells differ along its stepping axis
        for (int kd = 0; kd < 2; ++kd)
            for (int sd = 0; sd < 2; ++sd) cnt[kd][sd] = (size_t)(offs[kd][sd][n] - offs[kd][sd][0]);
        N1 = cnt[0][0] + cnt[1][0], N2 = cnt[0][1] + cnt[1][1], nc = cnt[0][1] + cnt[1][1] * (size_t)stride;
        max_prev = max_train = 0;
        for (int p = 0; p < 2 * n; ++p) {
            max_prev = std::max(max_prev, at(p).r1);
            max_train = std::max(max_train, at(p).r2);
        }
        max_rows = std::max(max_prev, max_train);
        if (N1 > (size_t)INT32_MAX || N2 > (size_t)INT32_MAX || nc > (size_t)INT32_MAX) return kTooMany;
        return max_train > kGmMaxTrain ? kTooWide : kOk;
    }
    Problem at(int p) const {
        const int f = p / 2, kd = p % 2, a1 = offs[kd][0][f], a2 = offs[kd][1][f];
        return {f, kd, a1, offs[kd][0][f + 1] - a1, a2, offs[kd][1][f + 1] - a2};
    }
    // The inputs every problem has: its row ranges over the batch and the first cell of its side 2
    // (off1, off2, cbase: 2 n + 1 entries), its kind and the first row of each side within its kind
    // (kind, kbase1, kbase2: 2 n entries; kbase2 may be absent), and its descriptor rows of db bytes,
    // gathered from descs[kind][side] into desc1 / desc2 in problem order.
    void fill(int32_t *off1, int32_t *off2, int32_t *kind, int32_t *kbase1, int32_t *kbase2, int32_t *cbase,
              const uint8_t *const descs[2][2], size_t db, uint8_t *desc1, uint8_t *desc2) const {
        off1[0] = off2[0] = cbase[0] = 0;
        for (int p = 0; p < 2 * n; ++p) {
            const Problem q = at(p);
            kind[p] = q.kind;
            kbase1[p] = q.a1 - offs[q.kind][0][0];
            if (kbase2) kbase2[p] = q.a2 - offs[q.kind][1][0];
            off1[p + 1] = off1[p] + q.r1;
            off2[p + 1] = off2[p] + q.r2;
            cbase[p + 1] = cbase[p] + q.r2 * (q.kind ? stride : 1);
            if (q.r1) memcpy(desc1 + db * off1[p], descs[q.kind][0] + db * q.a1, db * q.r1);
            if (q.r2) memcpy(desc2 + db * off2[p], descs[q.kind][1] + db * q.a2, db * q.r2);
        }
    }
};

// The grid matcher's working set where the cells are made on the device, in O (an StDev or a KfDev):
// the two key arrays, one range that starts as kGmNone, then the matcher's results and the cells of
// both sides. Returns the keys' size in bytes.
template <typename Owner>
size_t grid_workset(Staged &B, GmDev &D, Owner &O, const ProblemTable &T) {
    const size_t o_best = B.dev(D.best, T.N1);
    B.dev(D.second, T.N1);
    const size_t key_bytes = B.mark() - o_best;
    B.dev(D.m12, T.N1), B.dev(D.m21, T.N2), B.dev(D.count, 2 * (size_t)T.n);
    B.dev(O.cell1, 2 * T.N1), B.dev(O.cell1e, 2 * T.N1);
    B.dev(O.cell_off2, T.N2 + 1), B.dev(O.cells2, 2 * T.nc), B.dev(O.dir2, 2 * T.N2);
    return key_bytes;
}

// A call's plan: the table, the kernel structs and the block that binds them. B keeps the addresses of
// the structs' fields, so a plan stays where it was declared. T is set first (init); declare() then
// lays the block out for descriptors of dw dwords. The call fills every input and scatters every
// output itself, so no array has a source or a destination here.
struct StereoPlan {
    ProblemTable T;
    StDev S{};  // owns the arrays that the stereo kernels use too; the matcher's struct is bound from it
    GmDev D{};
    Staged B;
    size_t key_bytes = 0;

    void declare(size_t dw) {
        const size_t P = 2 * (size_t)T.n, N1 = T.N1, N2 = T.N2;
        B.in(S.off1, P + 1), B.in(S.off2, P + 1), B.in(S.kind, P), B.in(S.kbase, P), B.in(S.cbase, P + 1);
        B.in(D.ws, 4 * P), B.in(D.nnr, P), B.in(D.sim_th, P);
        B.in(S.desc1, dw * N1), B.in(D.desc2, dw * N2), B.in(S.co1, 4 * N1), B.in(S.co2, 4 * N2);
        B.out(S.count, P), B.out(S.src, N1), B.out(S.odesc, dw * N1);
        B.out(S.ptd, kStPtDoubles * T.cnt[0][0]), B.out(S.lsd, kStLsDoubles * T.cnt[1][0]);
        key_bytes = grid_workset(B, D, S, T);
    }
};

struct KfPlan {
    ProblemTable T;
    KfDev K{};  // owns the arrays that several kernels use; the matchers' structs are bound from it
    GmDev D{};
    DmDev M{};
    Staged B;
    size_t key_bytes = 0;

    void declare(size_t dw) {
        const size_t P = 2 * (size_t)T.n, N1 = T.N1, N2 = T.N2;
        B.in(K.off1, P + 1), B.in(K.off2, P + 1), B.in(K.kind, P), B.in(K.kbase1, P), B.in(K.kbase2, P), B.in(K.cbase, P + 1);
        B.in(K.gate_min, P), B.in(D.ws, 4 * P), B.in(D.nnr, P), B.in(D.sim_th, P), B.in(M.nnr, P);
        B.in(K.pose, (size_t)kKfPoseDoubles * T.n), B.in(D.desc1, dw * N1), B.in(D.desc2, dw * N2);
        B.in(K.q_pt, 3 * T.cnt[0][0]), B.in(K.q_ls, kKfQLsDoubles * T.cnt[1][0]), B.in(K.ls_new, T.cnt[1][0]);
        B.in(K.t_pt, kKfTPtDoubles * T.cnt[0][1]), B.in(K.t_ls, kKfTLsDoubles * T.cnt[1][1]);
        B.out(K.res, 3 * P), B.out(K.m12, N1);
        B.out(K.ptd, kKfPtDoubles * T.cnt[0][0]), B.out(K.lsd, kKfLsDoubles * T.cnt[1][0]), B.out(K.rej, T.cnt[1][0]);
        key_bytes = grid_workset(B, D, K, T);
        B.dev(M.nn12, N1), B.dev(M.nn21, N2), B.dev(M.m12, N1), B.dev(M.count, P);
    }
};

struct MaPlan {
    ProblemTable T;  // side 1: the candidate landmarks, side 2: the keyframe's unmatched features
    MaDev A{};  // owns the arrays that several kernels use; the matchers' structs are bound from it
    GmDev D{};
    DmDev M{};
    Staged B;
    size_t key_bytes = 0;

    void declare(size_t dw) {
        const size_t P = 2 * (size_t)T.n, N1 = T.N1, N2 = T.N2;
        B.in(A.off1, P + 1), B.in(A.off2, P + 1), B.in(A.kind, P), B.in(A.kbase1, P), B.in(A.kbase2, P), B.in(A.cbase, P + 1);
        B.in(A.min_matches, P), B.in(D.ws, 4 * P), B.in(D.nnr, P), B.in(D.sim_th, P), B.in(M.nnr, P);
        B.in(A.pose, (size_t)kMaPoseDoubles * T.n), B.in(D.desc1, dw * N1), B.in(D.desc2, dw * N2);
        B.in(A.q_pt, 3 * T.cnt[0][0]), B.in(A.q_ls, kMaQLsDoubles * T.cnt[1][0]);
        B.in(A.t_pt, kMaTPtDoubles * T.cnt[0][1]), B.in(A.t_ls, kMaTLsDoubles * T.cnt[1][1]);
        B.out(A.cnt, 2 * P), B.out(A.res, 2 * P), B.out(A.m12, N1), B.out(A.vis, N1), B.out(A.acc, N1);
        B.out(A.ptd, kMaPtDoubles * T.cnt[0][0]), B.out(A.lsd, kMaLsDoubles * T.cnt[1][0]);
        key_bytes = grid_workset(B, D, A, T);
        B.dev(M.nn12, N1), B.dev(M.nn21, N2), B.dev(M.m12, N1), B.dev(M.count, P);
        B.dev(A.skip, N1), B.dev(A.gate_min, P);
    }
};

// The median descriptor's block: n lists of `total` descriptors of dw dwords; the call fills `order`
inline void medoid_plan(Staged &B, MedDev &D, size_t n, size_t total, size_t dw, const int32_t *list_ptr,
                        const uint8_t *desc, int32_t *medoid) {
    B.in(D.list_ptr, n + 1, list_ptr), B.in(D.order, n), B.in(D.desc, dw * total, desc);
    B.out(D.medoid, n, medoid);
}

// The frame-to-frame pose's block: n problems over np point and nl line matches. An array that the
// line model or the motion model does not read has no source and no rows.
inline void trackpose_plan(Staged &B, TpDev &D, const plba_track_batch *b, bool pluker, bool motion, plba_track_out *out,
                           uint8_t *pt_inlier, uint8_t *ln_inlier) {
    const size_t n = (size_t)b->n, np = (size_t)b->pt_off[n], nl = (size_t)b->ln_off[n];
    B.in(D.pt_off, n + 1, b->pt_off), B.in(D.ln_off, n + 1, b->ln_off);
    B.in(D.pt_P, 3 * np, b->pt_P), B.in(D.pt_obs, 2 * np, b->pt_obs), B.in(D.pt_s2, np, b->pt_sigma2);
    B.in(D.ln_sP, 3 * nl, b->ln_sP), B.in(D.ln_eP, 3 * nl, b->ln_eP);
    B.in(D.ln_ND, pluker ? 6 * nl : 0, b->ln_NDc), B.in(D.ln_le, pluker ? 0 : 3 * nl, b->ln_le);
    B.in(D.ln_obs, pluker ? 4 * nl : 0, b->ln_obs), B.in(D.ln_seg, 4 * nl, b->ln_seg), B.in(D.ln_s2, nl, b->ln_sigma2);
    B.in(D.prev, motion ? (size_t)kTpPrev * n : 0, b->prev);
    B.out(D.out, n, out), B.out(D.pt_in, np, pt_inlier), B.out(D.ln_in, nl, ln_inlier);
    B.dev(D.pt_res, np), B.dev(D.ln_res, nl);
}

// Frame-to-frame tracking: the matcher's problems (side 1: a pair's previous rows, side 2: its current
// rows), the feature rows as the caller holds them (per kind, pairs back to back: a problem's kbase), and
// the pose's inputs, which k_f2f_gather writes on the device. A pair has at most as many matches of a
// kind as previous rows, so the pose's arrays are as long as the previous rows of the kind over the
// batch. An array that the line model or the motion model does not read has no source and no rows.
struct TfPlan {
    ProblemTable T;
    TfDev F{};
    DmDev M{};
    TpDev P{};
    Staged B;

    void declare(size_t dw, const plba_frames_batch *b, bool pluker, bool motion, const plba_frames_out *o) {
        const size_t np = 2 * (size_t)T.n, n = (size_t)T.n, N1 = T.N1, N2 = T.N2;
        const size_t p1 = T.cnt[0][0], p2 = T.cnt[0][1], l1 = T.cnt[1][0], l2 = T.cnt[1][1];
        B.in(F.off1, np + 1), B.in(F.off2, np + 1), B.in(F.kb1, np), B.in(F.kb2, np), B.in(M.nnr, np);
        B.in(M.desc1, dw * N1), B.in(M.desc2, dw * N2);
        B.in(F.p_P, 3 * p1, b->prev_pt_P), B.in(F.p_s2, p1, b->prev_pt_sigma2);
        B.in(F.l_sP, 3 * l1, b->prev_ln_sP), B.in(F.l_eP, 3 * l1, b->prev_ln_eP);
        B.in(F.l_ND, pluker ? 6 * l1 : 0, b->prev_ln_NDc), B.in(F.l_seg, 4 * l1, b->prev_ln_seg), B.in(F.l_s2, l1, b->prev_ln_sigma2);
        B.in(F.c_pl, 2 * p2, b->cur_pt_pl);
        B.in(F.c_seg, pluker ? 4 * l2 : 0, b->cur_ln_seg), B.in(F.c_le, pluker ? 0 : 3 * l2, b->cur_ln_le);
        B.in(P.prev, motion ? (size_t)kTpPrev * n : 0, b->prev);
        B.out(P.out, n, o->out);
        B.out(F.om12[0], p1, o->pt_m12), B.out(F.om12[1], l1, o->ln_m12);
        B.out(F.nm[0], n, o->n_pt), B.out(F.nm[1], n, o->n_ln);
        B.out(F.inl[0], p1, o->pt_inlier), B.out(F.inl[1], l1, o->ln_inlier);
        B.out(F.cfp[0], p2, o->pt_cur_from_prev), B.out(F.cfp[1], l2, o->ln_cur_from_prev);
        B.dev(M.nn12, N1), B.dev(M.nn21, N2), B.dev(M.m12, N1), B.dev(M.count, np);
        B.dev(F.g_off[0], n + 1), B.dev(F.g_off[1], n + 1), B.dev(F.src[0], p1), B.dev(F.src[1], l1);
        B.dev(F.g_pt_P, 3 * p1), B.dev(F.g_pt_obs, 2 * p1), B.dev(F.g_pt_s2, p1);
        B.dev(F.g_ln_sP, 3 * l1), B.dev(F.g_ln_eP, 3 * l1);
        B.dev(F.g_ln_ND, pluker ? 6 * l1 : 0), B.dev(F.g_ln_le, pluker ? 0 : 3 * l1);
        B.dev(F.g_ln_obs, pluker ? 4 * l1 : 0), B.dev(F.g_ln_seg, 4 * l1), B.dev(F.g_ln_s2, l1);
        B.dev(P.pt_in, p1), B.dev(P.ln_in, l1), B.dev(P.pt_res, p1), B.dev(P.ln_res, l1);
    }
};

}  // namespace plba
