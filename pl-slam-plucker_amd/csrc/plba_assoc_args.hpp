// plba_assoc_args.hpp — the kernel-argument structs of the matchers, the three association calls and the
// median descriptor, with the constants their host side sizes blocks and grids by. Standard C++ only:
// no HIP type, no kernel, so the host-only plans (csrc/plba_assoc_plan.hpp) and the layout test
// (tests/cpp/layout_check.cpp) read what the kernels read. Each kernel header includes this one and
// documents its fields' use.
#pragma once

#include <stdint.h>

#include "../../include/plba.h"

namespace plba {

// ---------------------------------------------------------------- csrc/plba_match.hpp
constexpr int kDmNT = 256;    // threads of a workgroup = query rows of a tile

struct DmDev {
    const int32_t *off1, *off2;   // [n+1] row ranges of each pair
    const uint32_t *desc1, *desc2;  // [.][desc_bytes / 4]
    const float *nnr;             // [n]
    int32_t *nn12, *nn21;         // [off1[n]], [off2[n]] nearest row after the ratio test, or -1
    int32_t *m12;                 // [off1[n]] matches_12
    int32_t *count;               // [n]
    int32_t n, dwords, best_lr;
    // plba_kf_associate's fallback: a pair runs only if gate_count[pair] < gate_min[pair]; NULL: every pair
    const int32_t *gate_count, *gate_min;
    // plba_map_associate's invisible landmarks: [off1[n]], nonzero where the side-1 row takes no part (it gets
    // nn12 = -1 and is never a side-2 row's nearest); NULL: every row takes part
    const uint8_t *skip1;
};

// ---------------------------------------------------------------- csrc/plba_gridmatch.hpp
constexpr int kGmNT = 64;       // threads of a workgroup = train rows of a block (one wave)
constexpr int kGmMaxTrain = 65535;         // i2 takes the key's low 16 bits

struct GmDev {
    const int32_t *off1, *off2;      // [n+1] row ranges of each problem
    const uint32_t *desc1, *desc2;   // [.][desc_bytes / 4]
    const int32_t *cell1, *cell1e;   // [off1[n]][2] query cell; second cell of a line query
    const int32_t *cell_off2;        // [off2[n]+1] CSR over the train rows
    const int32_t *cells2;           // [.][2]
    const double *dir2;              // [off2[n]][2]
    const int32_t *kind;             // [n]
    const int32_t *ws;               // [n][4] window half-widths: left, right (x), up, down (y)
    const double *nnr, *sim_th;      // [n]
    uint32_t *best, *second;         // [off1[n]] smallest and second-smallest seen key of a row
    int32_t *m21;                    // [off2[n]] matches_21 (best_lr)
    int32_t *m12;                    // [off1[n]] matches_12
    int32_t *count;                  // [n]
    int32_t n, dwords, cols, rows, best_lr;
};

// ---------------------------------------------------------------- csrc/plba_stereo.hpp
constexpr int kStNT = 256;  // threads of both kernels
constexpr int kStPtDoubles = 6;    // a point record: pl[2], disp, P[3]
constexpr int kStLsDoubles = 21;   // a line record: spl[2], epl[2], sdisp, edisp, sP[3], eP[3], le[3], NDc[6]

struct StDev {
    const int32_t *off1, *off2;    // [2n+1] left / right row ranges of each problem
    const int32_t *kind;           // [2n] 0 points, 1 lines
    const int32_t *kbase;          // [2n] first output record of the problem within its kind
    const int32_t *cbase;          // [2n+1] first cell of the problem's right rows
    const float *co1, *co2;        // [.][4] (x, y, -, -) of a point, (sx, sy, ex, ey) of a line
    const uint32_t *desc1;         // [off1[2n]][dwords]
    int32_t *cell1, *cell1e;       // [off1[2n]][2]
    int32_t *cell_off2;            // [off2[2n]+1]
    int32_t *cells2;               // [cbase[2n]][2]
    double *dir2;                  // [off2[2n]][2]
    const int32_t *m12;            // [off1[2n]] the matcher's result
    int32_t *count;                // [2n] survivors
    int32_t *src;                  // [off1[2n]] left index of each survivor, from off1[p]
    uint32_t *odesc;               // [off1[2n]][dwords]
    double *ptd, *lsd;             // point records [.][kStPtDoubles], line records [.][kStLsDoubles]
    double inv_w, inv_h;           // cols / (double)width, rows / (double)height
    int32_t dwords, stride;        // stride: cells of a right line, max(cols, rows)
    plba_stereo_params prm;
};

// ---------------------------------------------------------------- csrc/plba_kfassoc.hpp
constexpr int kKfNT = 256;  // threads of both kernels
constexpr int kKfPtDoubles = 9;   // a point record: P3d[3], dir_prev[3], dir_curr[3]
constexpr int kKfLsDoubles = 8;   // a line record: new_pluker_lw[6], |err_prev|, |err_curr|
constexpr int kKfPoseDoubles = 76;  // a pair's poses: DT[12], T_prev, T_curr, Tcw_prev, Tcw_curr [16] each
constexpr int kKfQLsDoubles = 22;   // a previous line row: sP[3], eP[3], NDc[6], spl[2], epl[2], lm_NDw[6]
constexpr int kKfTPtDoubles = 5;    // a current point row: pl[2], P[3]
constexpr int kKfTLsDoubles = 4;    // a current line row: spl[2], epl[2]

struct KfDev {
    const int32_t *off1, *off2;    // [2n+1] previous / current row ranges of each problem
    const int32_t *kind;           // [2n] 0 points, 1 lines
    const int32_t *kbase1, *kbase2;  // [2n] first previous / current row of the problem within its kind
    const int32_t *cbase;          // [2n+1] first cell of the problem's current rows
    const int32_t *gate_min;       // [2n] the fallback's bound on the grid count, or INT_MIN
    const double *pose;            // [n][kKfPoseDoubles]
    const double *q_pt, *q_ls;     // previous rows: [.][3], [.][kKfQLsDoubles]
    const uint8_t *ls_new;         // [.] per previous line row
    const double *t_pt, *t_ls;     // current rows: [.][kKfTPtDoubles], [.][kKfTLsDoubles]
    int32_t *cell1, *cell1e;       // [off1[2n]][2]
    int32_t *cell_off2;            // [off2[2n]+1]
    int32_t *cells2;               // [cbase[2n]][2]
    double *dir2;                  // [off2[2n]][2]
    const int32_t *gm12, *gcount;  // the grid matcher's result
    const int32_t *fm12, *fcount;  // the brute-force matcher's, where it ran
    int32_t *res;                  // [2n][3] grid count, match count, fallback
    int32_t *m12;                  // [off1[2n]]
    double *ptd, *lsd;             // point records [.][kKfPtDoubles], line records [.][kKfLsDoubles]
    uint8_t *rej;                  // [.] per previous line row
    double inv_w, inv_h;           // cols / (double)width, rows / (double)height
    int32_t stride, pad;           // stride: cells of a current line, max(cols, rows)
    plba_kfassoc_params prm;
};

// ---------------------------------------------------------------- csrc/plba_mapassoc.hpp
constexpr int kMaNT = 256;  // threads of the three kernels
constexpr int kMaPtDoubles = 6;    // a point record: u, v, err, dir[3]
constexpr int kMaLsDoubles = 9;    // a line record: su, sv, eu, ev, err0, err1, mid[3]
constexpr int kMaPoseDoubles = 28;  // a keyframe's poses: Twf[12], T_kf_w[16]
constexpr int kMaQLsDoubles = 6;    // a candidate line row: line3D
constexpr int kMaTPtDoubles = 5;    // a point feature row: pl[2], P[3]
constexpr int kMaTLsDoubles = 13;   // a line feature row: spl[2], epl[2], le[3], sP[3], eP[3]

struct MaDev {
    const int32_t *off1, *off2;    // [2n+1] candidate / feature row ranges of each problem
    const int32_t *kind;           // [2n] 0 points, 1 lines
    const int32_t *kbase1, *kbase2;  // [2n] first candidate / feature row of the problem within its kind
    const int32_t *cbase;          // [2n+1] first cell of the problem's feature rows
    const int32_t *min_matches;    // [2n] min_pt_matches or min_ls_matches
    const double *pose;            // [n][kMaPoseDoubles]
    const double *q_pt, *q_ls;     // candidate rows: [.][3], [.][kMaQLsDoubles]
    const double *t_pt, *t_ls;     // feature rows: [.][kMaTPtDoubles], [.][kMaTLsDoubles]
    int32_t *cell1, *cell1e;       // [off1[2n]][2]
    int32_t *cell_off2;            // [off2[2n]+1]
    int32_t *cells2;               // [cbase[2n]][2]
    double *dir2;                  // [off2[2n]][2]
    uint8_t *skip;                 // [off1[2n]] 1 where the candidate is invisible: DmDev::skip1
    int32_t *gate_min;             // [2n] the fallback's bound on the grid count, or INT_MIN: DmDev::gate_min
    const int32_t *gm12, *gcount;  // the grid matcher's result
    const int32_t *fm12;           // the brute-force matcher's, where it ran
    int32_t *cnt;                  // [2n][2] visible candidates, accepted rows: summed with integer atomics from 0
    int32_t *res;                  // [2n][2] grid count, fallback
    int32_t *m12;                  // [off1[2n]]
    uint8_t *vis, *acc;            // [off1[2n]] visible, accepted
    double *ptd, *lsd;             // point records [.][kMaPtDoubles], line records [.][kMaLsDoubles]
    double inv_w, inv_h;           // cols / (double)width, rows / (double)height
    int32_t stride, pad;           // stride: cells of a line feature, max(cols, rows)
    plba_mapassoc_params prm;
};
// the kernels read the struct as an argument: 29 pointers, two doubles, two ints and the parameters, no padding
static_assert(sizeof(plba_mapassoc_params) == 10 * 4 + 9 * 8, "plba_mapassoc_params has no padding");
static_assert(sizeof(MaDev) == 29 * sizeof(void *) + 2 * 8 + 2 * 4 + sizeof(plba_mapassoc_params), "MaDev has no padding");

// ---------------------------------------------------------------- csrc/plba_medoid.hpp
struct MedDev {
    const int32_t *list_ptr;   // [n+1]
    const uint32_t *desc;      // [list_ptr[n]][dwords]
    const int32_t *order;      // [n] the short lists, then the long ones
    int32_t *medoid;           // [n]
    int32_t n, dwords, n_short, n_short_wg;
};

// ---------------------------------------------------------------- csrc/plba_trackpose.hpp
constexpr int kTpNT = 256;               // threads of a problem's workgroup
constexpr int kTpMaxN = PLBA_TRACK_MAX_N;  // matches of one kind in one problem
constexpr int kTpPrev = 53;              // doubles of a problem's motion-model input: DT, DT_cov, err_norm

struct TpDev {
    const int32_t *pt_off, *ln_off;      // [n+1] match ranges of each problem
    const double *pt_P, *pt_obs, *pt_s2; // [.][3], [.][2], [.]
    const double *ln_sP, *ln_eP;         // [.][3]
    const double *ln_ND, *ln_le;         // [.][6] (Plücker model), [.][3] (endpoint model)
    const double *ln_obs, *ln_seg;       // [.][4] spl_obs, epl_obs (Plücker model); [.][4] spl, epl
    const double *ln_s2;                 // [.]
    const double *prev;                  // [n][kTpPrev] (motion model)
    plba_track_out *out;                 // [n]
    uint8_t *pt_in, *ln_in;              // [.] inlier flags
    double *pt_res, *ln_res;             // [.] the residual lists (device only)
    double fx, fy, cx, cy;
    plba_track_params prm;
};

// ---------------------------------------------------------------- csrc/plba_trackframes.hpp
constexpr int kTfNT = 256;  // threads of both kernels

// A pair is the matcher's problems 2 k (its points) and 2 k + 1 (its lines). Arrays of two are [kind].
struct TfDev {
    const int32_t *off1, *off2;    // [2n+1] previous / current row ranges of each problem, as the matcher reads them
    const int32_t *kb1, *kb2;      // [2n] first previous / current row of the problem within its kind
    const int32_t *m12, *count;    // the matcher's result: [off1[2n]], [2n]
    const double *p_P, *p_s2;      // previous point rows: [.][3], [.]
    const double *l_sP, *l_eP;     // previous line rows: [.][3]
    const double *l_ND, *l_seg, *l_s2;  // [.][6] (Plücker model), [.][4], [.]
    const double *c_pl;            // current point rows: [.][2]
    const double *c_seg, *c_le;    // current line rows: [.][4] (Plücker model), [.][3] (endpoint model)
    int32_t *om12[2];              // per previous row of the kind: matches_12
    uint8_t *inl[2];               // per previous row of the kind: the inlier flag, 0 where there is no match
    int32_t *cfp[2];               // per current row of the kind: cur_from_prev
    int32_t *nm[2];                // [n] matches of the pair
    int32_t *src[2];               // per match row: its i1 within the pair
    // k_trackpose's inputs, which k_f2f_gather writes (the TpDev of the call points to the same arrays)
    int32_t *g_off[2];             // [n+1] match ranges of each pair
    double *g_pt_P, *g_pt_obs, *g_pt_s2;
    double *g_ln_sP, *g_ln_eP, *g_ln_ND, *g_ln_le, *g_ln_obs, *g_ln_seg, *g_ln_s2;
    const uint8_t *tin[2];         // k_trackpose's inlier flags, per match row
    int32_t cap[2];                // previous rows of the kind over the batch: no match row lies beyond
    int32_t on[2];                 // has_points, has_lines
    int32_t n, pluker;
};

}  // namespace plba
