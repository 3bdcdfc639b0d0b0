// TEST INFRASTRUCTURE ONLY — extern "C" entry points over the pieces of the reference that compile with the
// standard library alone, so that tests can compare the checkers (tests/ref_gridmatch.py, ref_stereo.py,
// ref_bow.py), the host mirror and the kernels with the reference's own code:
//   src2/lineIterator.cpp, src2/gridStructure.cpp   getLineCoords, GridStructure::at / get
//   src2/matching.cpp                               both matchGrid overloads, distance; normalize (matching.h)
//   3rdparty/DBoW2/src/DBoW2/BowVector.cpp          addWeight, addIfNotExist, normalize(L1)
// oracle/Makefile compiles those files in place from the reference tree together with this file, the two
// stand-in headers under opencv2/ and refpin_config.cpp into oracle/_ref/libref_stvo.so. Nothing of the
// reference is copied here.
// Left out: matchNNR / match (they need OpenCV's real BFMatcher and its tie order; the stand-in's knnMatch
// throws) and L1Scoring::score (behind TemplatedVocabulary.h, which needs OpenCV and DUtils).
// Every function returns 0, or -1 for an exception or a NULL argument. Arrays are the caller's.
#include <algorithm>
#include <cstdint>
#include <list>
#include <unordered_set>
#include <utility>
#include <vector>

#include <opencv2/core.hpp>

#include "BowVector.h"
#include "config.h"
#include "gridStructure.h"
#include "matching.h"

namespace {
StVO::GridWindow window(const int32_t *w) {   // w: left, right, up, down
    StVO::GridWindow gw;
    gw.width = std::make_pair((int)w[0], (int)w[1]);
    gw.height = std::make_pair((int)w[2], (int)w[3]);
    return gw;
}
void set_config(int best_lr, double nnr, double line_sim_th) {
    Config::bestLRMatches() = best_lr != 0;
    Config::minRatio12P() = nnr;
    Config::lineSimTh() = line_sim_th;
}
}  // namespace

extern "C" {

// getLineCoords: *n is the number of cells; the first min(*n, cap) are written as (x, y) in the walk's order.
int refpin_line_coords(double x1, double y1, double x2, double y2, int32_t *cells, int32_t cap, int32_t *n) {
    if (!n || (cap > 0 && !cells)) return -1;
    try {
        std::list<std::pair<int, int>> coords;
        StVO::getLineCoords(x1, y1, x2, y2, coords);
        *n = (int32_t)coords.size();
        int32_t k = 0;
        for (const std::pair<int, int> &p : coords) {
            if (k >= cap) break;
            cells[2 * k] = p.first;
            cells[2 * k + 1] = p.second;
            ++k;
        }
    } catch (...) { return -1; }
    return 0;
}

void *refpin_grid_new(int32_t rows, int32_t cols) {
    try { return new StVO::GridStructure(rows, cols); } catch (...) { return nullptr; }
}
void refpin_grid_free(void *g) { delete static_cast<StVO::GridStructure *>(g); }

// grid.at(x, y).push_back(idx) for the cells of train row idx = 0 .. n2 - 1, rows in order, a row's cells in
// order: cells[cell_off[idx] .. cell_off[idx + 1]) as (x, y). The fill of src2/stereoFrame.cpp:137-140, :329-339.
int refpin_grid_fill(void *g, int32_t n2, const int32_t *cell_off, const int32_t *cells) {
    if (!g || (n2 > 0 && (!cell_off || !cells))) return -1;
    try {
        StVO::GridStructure &grid = *static_cast<StVO::GridStructure *>(g);
        for (int32_t idx = 0; idx < n2; ++idx)
            for (int32_t c = cell_off[idx]; c < cell_off[idx + 1]; ++c) grid.at(cells[2 * c], cells[2 * c + 1]).push_back(idx);
    } catch (...) { return -1; }
    return 0;
}

// GridStructure::get: *n indices, the first min(*n, cap) written in increasing order (the set has none).
int refpin_grid_get(void *g, int32_t x, int32_t y, const int32_t *w, int32_t *out, int32_t cap, int32_t *n) {
    if (!g || !w || !n || (cap > 0 && !out)) return -1;
    try {
        std::unordered_set<int> indices;
        static_cast<const StVO::GridStructure *>(g)->get(x, y, window(w), indices);
        std::vector<int> sorted(indices.begin(), indices.end());
        std::sort(sorted.begin(), sorted.end());
        *n = (int32_t)sorted.size();
        for (int32_t k = 0; k < *n && k < cap; ++k) out[k] = sorted[k];
    } catch (...) { return -1; }
    return 0;
}

// StVO::distance over two rows of at least 32 bytes (it reads eight 32-bit words whatever the width).
int refpin_distance(const uint8_t *a, const uint8_t *b) {
    return StVO::distance(cv::Mat(1, 32, a, 32), cv::Mat(1, 32, b, 32));
}

// matching.h's normalize on v[2]
int refpin_normalize(double *v) {
    if (!v) return -1;
    std::pair<double, double> p(v[0], v[1]);
    StVO::normalize(p);
    v[0] = p.first;
    v[1] = p.second;
    return 0;
}

// matchGrid for points: cell1 [n1][2], desc1 [n1][32], desc2 [n2][32]; matches_12 [n1]; *count is what the
// reference returns (it may count rows whose index stays -1).
int refpin_match_grid_points(void *g, int32_t n1, const int32_t *cell1, const uint8_t *desc1, int32_t n2,
                             const uint8_t *desc2, const int32_t *w, int32_t best_lr, double nnr, int32_t *matches_12,
                             int32_t *count) {
    if (!g || !w || !count || (n1 > 0 && (!cell1 || !desc1 || !matches_12))) return -1;
    try {
        set_config(best_lr, nnr, 0.0);
        std::vector<StVO::point_2d> points1(n1);
        for (int32_t i = 0; i < n1; ++i) points1[i] = std::make_pair((int)cell1[2 * i], (int)cell1[2 * i + 1]);
        std::vector<int> m12;
        *count = StVO::matchGrid(points1, cv::Mat(n1, 32, desc1, 32), *static_cast<const StVO::GridStructure *>(g),
                                 cv::Mat(n2, 32, desc2, 32), window(w), m12);
        for (int32_t i = 0; i < n1; ++i) matches_12[i] = m12[i];
    } catch (...) { return -1; }
    return 0;
}

// matchGrid for lines: cell1 / cell1_end [n1][2] the start and end cells, dir2 [n2][2]
int refpin_match_grid_lines(void *g, int32_t n1, const int32_t *cell1, const int32_t *cell1_end, const uint8_t *desc1,
                            int32_t n2, const uint8_t *desc2, const double *dir2, const int32_t *w, int32_t best_lr,
                            double nnr, double line_sim_th, int32_t *matches_12, int32_t *count) {
    if (!g || !w || !count || (n1 > 0 && (!cell1 || !cell1_end || !desc1 || !matches_12)) || (n2 > 0 && !dir2)) return -1;
    try {
        set_config(best_lr, nnr, line_sim_th);
        std::vector<StVO::line_2d> lines1(n1);
        for (int32_t i = 0; i < n1; ++i)
            lines1[i] = std::make_pair(std::make_pair((int)cell1[2 * i], (int)cell1[2 * i + 1]),
                                       std::make_pair((int)cell1_end[2 * i], (int)cell1_end[2 * i + 1]));
        std::vector<std::pair<double, double>> directions2(n2);
        for (int32_t i = 0; i < n2; ++i) directions2[i] = std::make_pair(dir2[2 * i], dir2[2 * i + 1]);
        std::vector<int> m12;
        *count = StVO::matchGrid(lines1, cv::Mat(n1, 32, desc1, 32), *static_cast<const StVO::GridStructure *>(g),
                                 cv::Mat(n2, 32, desc2, 32), directions2, window(w), m12);
        for (int32_t i = 0; i < n1; ++i) matches_12[i] = m12[i];
    } catch (...) { return -1; }
    return 0;
}

// BowVector: the calls in the caller's order, then the entries back in map order.
void *refpin_bow_new() { try { return new DBoW2::BowVector(); } catch (...) { return nullptr; } }
void refpin_bow_free(void *v) { delete static_cast<DBoW2::BowVector *>(v); }
int refpin_bow_add_weight(void *v, uint32_t id, double value) {
    if (!v) return -1;
    try { static_cast<DBoW2::BowVector *>(v)->addWeight(id, value); } catch (...) { return -1; }
    return 0;
}
int refpin_bow_add_if_not_exist(void *v, uint32_t id, double value) {
    if (!v) return -1;
    try { static_cast<DBoW2::BowVector *>(v)->addIfNotExist(id, value); } catch (...) { return -1; }
    return 0;
}
int refpin_bow_normalize_l1(void *v) {
    if (!v) return -1;
    try { static_cast<DBoW2::BowVector *>(v)->normalize(DBoW2::L1); } catch (...) { return -1; }
    return 0;
}
int refpin_bow_entries(void *v, uint32_t *ids, double *values, int32_t cap, int32_t *n) {
    if (!v || !n || (cap > 0 && (!ids || !values))) return -1;
    const DBoW2::BowVector &bv = *static_cast<const DBoW2::BowVector *>(v);
    *n = (int32_t)bv.size();
    int32_t k = 0;
    for (DBoW2::BowVector::const_iterator it = bv.begin(); it != bv.end() && k < cap; ++it, ++k) {
        ids[k] = it->first;
        values[k] = it->second;
    }
    return 0;
}

}  // extern "C"
