// Place recognition in the host mirror: insertKFBowVectorP / L / PL (src/mapHandler.cpp:4118-4239),
// lookForLoopCandidates (:4241-4301) and loopClosure() whole (:4053-4116). The BoW vectors live in the
// database of plba_bow_* (include/plba.h) or behind the hook; the map keeps conf_matrix. This file is
// compiled with -ffp-contract=off: the combined score of :4226-4228 and vector_stdv are the
// reference's double arithmetic, one rounding per operation. Also here: the single-threaded CPU
// restatement of plba_bow_* (bowCpu), for the tests and tools/bow_bench.py only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "plslam_map.hpp"

namespace plslam {

int MapHandler::bowCall(BowCall &c) {
    const int rc = backend(bow_, "place-recognition", [&](plba_ctx *ctx) -> int {
        switch (c.op) {
        case BOW_SET_VOCAB: return plba_bow_set_vocab(ctx, c.slot, c.vocab);
        case BOW_INSERT: return plba_bow_insert(ctx, c.slot, c.kf_id, c.desc, c.n_desc, c.scores, c.ids, c.cap, &c.n);
        case BOW_REMOVE: return plba_bow_remove(ctx, c.slot, c.kf_id);
        case BOW_GET: return plba_bow_get(ctx, c.slot, c.kf_id, c.word_ids, c.values, c.cap, &c.n);
        default: return PLBA_E_INVALID;
        }
    }, &c);
    if (rc && bow_.fn) setError("%s (op %d, slot %d)", std::string(err_).c_str(), c.op, c.slot);
    return rc;
}

int MapHandler::setVocabulary(int slot, const plba_bow_vocab *v) {
    if (slot != 0 && slot != 1) {
        setError("vocabulary: slot %d is neither 0 (points) nor 1 (lines)", slot);
        return PLBA_E_INVALID;
    }
    BowCall c{};
    c.op = BOW_SET_VOCAB;
    c.slot = slot;
    c.vocab = v;
    const int rc = bowCall(c);
    if (rc) return rc;
    bow_vocab_[slot] = true;
    bow_in_db_[slot].clear();
    return PLBA_OK;
}

int MapHandler::removeKeyframe(int kf_idx) {
    if (kf_idx < 0 || kf_idx >= (int)map_keyframes.size() || !map_keyframes[kf_idx]) {
        setError("keyframe %d does not exist", kf_idx);
        return PLBA_E_INVALID;
    }
    delete map_keyframes[kf_idx];
    map_keyframes[kf_idx] = nullptr;
    return PLBA_OK;
}

namespace {

// src2/auxiliar.cpp:504-513; n == 0 gives NaN as there (0 / 0, then inf * 0)
double vector_stdv(const std::vector<double> &v) {
    double mean = 0.0, e = 0.0;
    for (size_t i = 0; i < v.size(); ++i) mean += v[i];
    mean /= (double)v.size();
    for (size_t i = 0; i < v.size(); ++i) e += (v[i] - mean) * (v[i] - mean);
    return std::sqrt(1.0 / (double)v.size() * e);
}

// src/mapHandler.cpp:4226-4228, in that order
double combined_score(double score_p, double score_l, int n_pt, int n_ls, double std_pt, double std_ls) {
    const int n_pl = n_pt + n_ls;
    const double std_pl = std_ls + std_pt;
    double score = 0.0;
    score += (score_p * n_pt + score_l * n_ls) / n_pl;
    score += (score_p * std_pt + score_l * std_ls) / std_pl;
    return score;
}

}  // namespace

int MapHandler::insertKfBow(int kf_idx, bool has_points, bool has_lines) {
    const bool use[2] = {has_points, has_lines};
    if (!has_points && !has_lines) {
        setError("place recognition: neither points nor lines");
        return PLBA_E_INVALID;
    }
    if (kf_idx < 0 || kf_idx >= (int)map_keyframes.size() || !map_keyframes[kf_idx] ||
        !map_keyframes[kf_idx]->stereo_frame.has_features) {
        setError("place recognition: keyframe %d does not exist or has no features set", kf_idx);
        return PLBA_E_INVALID;
    }
    if (kf_idx < (int)bow_inserted_.size() && bow_inserted_[kf_idx]) {
        setError("place recognition: keyframe %d was inserted before", kf_idx);
        return PLBA_E_INVALID;
    }
    const StereoFrame &f = map_keyframes[kf_idx]->stereo_frame;
    const int n_pt = (int)f.stereo_pt_idx.size(), n_ls = (int)f.stereo_ls_idx.size();
    for (int s = 0; s < 2; ++s)
        if (use[s] && !bow_vocab_[s]) {
            setError("place recognition: slot %d has no vocabulary", s);
            return PLBA_E_INVALID;
        }
    if (has_points && has_lines && n_ls > 0 && !f.has_endpoints) {
        setError("place recognition: keyframe %d has line features without image endpoints", kf_idx);
        return PLBA_E_INVALID;
    }
    const size_t nkf = map_keyframes.size();
    for (int s = 0; s < 2; ++s) bow_in_db_[s].resize(std::max(bow_in_db_[s].size(), nkf), 0);
    // the keyframes culled since the last insert leave the database (the reference skips NULL ones)
    std::vector<uint8_t> live[2];
    for (int s = 0; s < 2; ++s) {
        live[s] = bow_in_db_[s];
        for (size_t i = 0; i < live[s].size(); ++i)
            if (live[s][i] && (i >= nkf || !map_keyframes[i])) live[s][i] = 0;
    }
    if (has_points && has_lines && live[0] != live[1]) {
        setError("place recognition: the point and the line database do not hold the same keyframes");
        return PLBA_E_INVALID;
    }
    for (int s = 0; s < 2; ++s)
        for (size_t i = 0; i < live[s].size(); ++i)
            if (bow_in_db_[s][i] && !live[s][i]) {
                BowCall c{};
                c.op = BOW_REMOVE;
                c.slot = s;
                c.kf_id = (int32_t)i;
                if (const int rc = bowCall(c)) return rc;
                bow_in_db_[s][i] = 0;
            }
    // transform and score (dbow_voc.transform / .score): one insert per kind
    std::vector<double> scores[2];
    std::vector<int32_t> ids[2];
    for (int s = 0; s < 2; ++s) {
        if (!use[s]) continue;
        const int cap = 1 + (int)std::count(live[s].begin(), live[s].end(), (uint8_t)1);
        scores[s].assign(cap, 0.0);
        ids[s].assign(cap, -1);
        BowCall c{};
        c.op = BOW_INSERT;
        c.slot = s;
        c.kf_id = kf_idx;
        const std::vector<uint8_t> &d = s == 0 ? f.pdesc_l : f.ldesc_l;
        c.n_desc = s == 0 ? n_pt : n_ls;
        c.desc = c.n_desc ? d.data() : nullptr;
        c.scores = scores[s].data();
        c.ids = ids[s].data();
        c.cap = cap;
        if (const int rc = bowCall(c)) return rc;
        bow_in_db_[s][kf_idx] = 1;
        if (c.n != cap || ids[s].back() != kf_idx) {
            setError("place recognition: %d scores for %d live keyframes in slot %d", c.n, cap, s);
            return PLBA_E_INVALID;
        }
    }
    const int lead = has_points ? 0 : 1;
    if (has_points && has_lines && ids[0] != ids[1]) {
        setError("place recognition: the slots answered for different keyframes");
        return PLBA_E_INVALID;
    }
    double std_pt = 0.0, std_ls = 0.0;
    if (has_points && has_lines) {  // the dispersion of the features (:4181-4213)
        std::vector<double> x(n_pt), y(n_pt);
        for (int i = 0; i < n_pt; ++i) {
            x[i] = f.pt_pl[2 * i];
            y[i] = f.pt_pl[2 * i + 1];
        }
        std_pt = vector_stdv(x) + vector_stdv(y);
        x.resize(n_ls);
        y.resize(n_ls);
        for (int i = 0; i < n_ls; ++i) {
            x[i] = (f.ls_spl[2 * i] + f.ls_epl[2 * i]) * 0.5;
            y[i] = (f.ls_spl[2 * i + 1] + f.ls_epl[2 * i + 1]) * 0.5;
        }
        std_ls = vector_stdv(x) + vector_stdv(y);
    }
    // expandGraphs (:1000-1002): conf_matrix grows with zeros
    const size_t need = std::max(conf_matrix.size(), (size_t)kf_idx + 1);
    conf_matrix.resize(need);
    for (auto &row : conf_matrix) row.resize(need, 0.0f);
    for (size_t j = 0; j < ids[lead].size(); ++j) {
        const int i = ids[lead][j];
        double score = scores[lead][j];
        if (has_points && has_lines) score = combined_score(scores[0][j], scores[1][j], n_pt, n_ls, std_pt, std_ls);
        if (i > kf_idx) continue;  // the reference scores against earlier keyframes only (:4131)
        conf_matrix[kf_idx][i] = (float)score;
        conf_matrix[i][kf_idx] = (float)score;
    }
    bow_inserted_.resize(std::max(bow_inserted_.size(), (size_t)kf_idx + 1), 0);
    bow_inserted_[kf_idx] = 1;
    return PLBA_OK;
}

int MapHandler::lookForLoopCandidates(int kf_curr_idx, const LcSearchParams &p, bool &is_candidate, int &kf_prev_idx) {
    is_candidate = false;
    kf_prev_idx = -1;
    if (p.lc_kf_dist < 0 || p.lc_kf_max_dist < 0 || p.lc_nkf_closest < 0 || p.min_lm_cov_graph < 0 || p.min_kf_local_map < 0) {
        setError("loop candidates: a negative parameter");
        return PLBA_E_INVALID;
    }
    if (kf_curr_idx < 0 || kf_curr_idx >= (int)conf_matrix.size() || kf_curr_idx >= (int)full_graph.size() ||
        kf_curr_idx >= (int)map_keyframes.size()) {
        setError("loop candidates: keyframe %d is outside conf_matrix, full_graph or the map", kf_curr_idx);
        return PLBA_E_INVALID;
    }
    struct Cand {
        int idx;
        double score;
    };
    std::vector<Cand> max_confmat;
    for (int i = 0; i < kf_curr_idx - p.lc_kf_dist; ++i)
        if (map_keyframes[i] != nullptr) max_confmat.push_back(Cand{i, (double)conf_matrix[i][kf_curr_idx]});
    if (!(max_confmat.size() > (size_t)p.lc_kf_max_dist)) return PLBA_OK;
    // descending by score, ties by increasing index, NaN last
    std::sort(max_confmat.begin(), max_confmat.end(), [](const Cand &a, const Cand &b) {
        const bool an = std::isnan(a.score), bn = std::isnan(b.score);
        if (an != bn) return bn;
        if (!an && a.score != b.score) return a.score > b.score;
        return a.idx < b.idx;
    });
    double lc_min_score = 1.0;
    for (int i = 0; i < kf_curr_idx; ++i)
        if (full_graph[i][kf_curr_idx] >= (unsigned)p.min_lm_cov_graph || kf_curr_idx - i <= p.min_kf_local_map + 3) {
            const double score_i = conf_matrix[i][kf_curr_idx];
            if (score_i < lc_min_score && score_i > 0.001) lc_min_score = score_i;
        }
    const int idx_max = max_confmat[0].idx;
    int n_closest = 0;
    if (max_confmat[0].score >= lc_min_score) {
        for (size_t i = 1; i < max_confmat.size(); ++i)
            if (std::abs(max_confmat[i].idx - idx_max) <= p.lc_kf_max_dist && max_confmat[i].score >= lc_min_score * 0.8)
                n_closest++;
        if (n_closest >= p.lc_nkf_closest) {
            is_candidate = true;
            kf_prev_idx = idx_max;
        }
    }
    return PLBA_OK;
}

int MapHandler::loopClosureKf(int kf_curr_idx, const LcSearchParams &sp, const MatchParams &mp, double lc_inlier_ratio,
                              LcStats *stats) {
    bool is_candidate = false;
    int kf_prev_idx = -1;
    if (const int rc = lookForLoopCandidates(kf_curr_idx, sp, is_candidate, kf_prev_idx)) return rc;
    if (is_candidate) return isLoopClosure(kf_prev_idx, kf_curr_idx, mp, lc_inlier_ratio, stats);
    return loopClosureStep(nullptr, lc_inlier_ratio, stats);
}

// ---------------------------------------------------------------- the CPU restatement
// plba_bow_*'s semantics (include/plba.h) on sorted arrays, single-threaded. Not a product path.
struct BowCpuDb {
    struct Slot {
        bool has_vocab = false;
        int n_nodes = 0, n_words = 0, desc_bytes = 0;
        std::vector<int32_t> child_off, children, word_id;
        std::vector<uint8_t> node_desc;
        std::vector<double> weight;
        struct Vec {
            std::vector<int32_t> words;
            std::vector<double> values;
            bool live = true;
        };
        std::map<int, Vec> rows;  // by kf_id; a removed row keeps its id
    } slot[2];
};

BowCpuDb *bowCpuNew() { return new BowCpuDb(); }
void bowCpuFree(BowCpuDb *db) { delete db; }

namespace {

int cpu_set_vocab(BowCpuDb::Slot &S, const plba_bow_vocab *v) {
    if (!v || !v->child_off || !v->children || !v->node_desc || !v->word_id || !v->weight) return PLBA_E_INVALID;
    const int nn = v->n_nodes, db = v->desc_bytes;
    if (db < 4 || db > 64 || db % 4 || nn < 2 || v->n_words < 1 || v->n_words > nn) return PLBA_E_INVALID;
    if (v->child_off[0] != 0) return PLBA_E_INVALID;
    for (int i = 0; i < nn; ++i)
        if (v->child_off[i + 1] < v->child_off[i]) return PLBA_E_INVALID;
    if (v->child_off[nn] != nn - 1 || v->child_off[1] == 0) return PLBA_E_INVALID;
    std::vector<uint8_t> seen(nn, 0), word_seen(v->n_words, 0);
    std::vector<int> stack{0};
    seen[0] = 1;
    int reached = 1;
    while (!stack.empty()) {
        const int node = stack.back();
        stack.pop_back();
        for (int e = v->child_off[node]; e < v->child_off[node + 1]; ++e) {
            const int c = v->children[e];
            if (c <= 0 || c >= nn || seen[c]) return PLBA_E_INVALID;
            seen[c] = 1;
            ++reached;
            stack.push_back(c);
        }
    }
    if (reached != nn) return PLBA_E_INVALID;
    for (int i = 0; i < nn; ++i) {
        if (!std::isfinite(v->weight[i])) return PLBA_E_INVALID;
        const int w = v->word_id[i];
        if (v->child_off[i + 1] > v->child_off[i]) {
            if (w >= 0) return PLBA_E_INVALID;
        } else {
            if (w < 0 || w >= v->n_words || word_seen[w]) return PLBA_E_INVALID;
            word_seen[w] = 1;
        }
    }
    S.n_nodes = nn;
    S.n_words = v->n_words;
    S.desc_bytes = db;
    S.child_off.assign(v->child_off, v->child_off + nn + 1);
    S.children.assign(v->children, v->children + nn - 1);
    S.word_id.assign(v->word_id, v->word_id + nn);
    S.node_desc.assign(v->node_desc, v->node_desc + (size_t)nn * db);
    S.weight.assign(v->weight, v->weight + nn);
    S.rows.clear();
    S.has_vocab = true;
    return PLBA_OK;
}

int cpu_distance(const uint8_t *a, const uint8_t *b, int bytes) {
    int d = 0;
    for (int c = 0; c < bytes; c += 4) {
        uint32_t x, y;
        std::memcpy(&x, a + c, 4);
        std::memcpy(&y, b + c, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

void cpu_transform(const BowCpuDb::Slot &S, const uint8_t *desc, int n_desc, BowCpuDb::Slot::Vec &out) {
    std::vector<int32_t> words;
    for (int r = 0; r < n_desc; ++r) {
        const uint8_t *q = desc + (size_t)r * S.desc_bytes;
        int node = 0;
        while (S.child_off[node + 1] > S.child_off[node]) {
            int best = -1, best_d = 0;
            for (int e = S.child_off[node]; e < S.child_off[node + 1]; ++e) {
                const int c = S.children[e];
                const int d = cpu_distance(q, &S.node_desc[(size_t)c * S.desc_bytes], S.desc_bytes);
                if (best < 0 || d < best_d) {
                    best = c;
                    best_d = d;
                }
            }
            node = best;
        }
        if (S.weight[node] > 0) words.push_back(node);  // the leaf; its word below
    }
    std::sort(words.begin(), words.end(), [&](int a, int b) { return S.word_id[a] < S.word_id[b]; });
    for (size_t i = 0; i < words.size();) {
        const double w = S.weight[words[i]];
        double v = w;
        size_t j = i + 1;
        for (; j < words.size() && words[j] == words[i]; ++j) v += w;
        out.words.push_back(S.word_id[words[i]]);
        out.values.push_back(v);
        i = j;
    }
    double norm = 0.0;
    for (double v : out.values) norm += std::fabs(v);
    if (norm > 0.0)
        for (double &v : out.values) v /= norm;
}

double cpu_score(const BowCpuDb::Slot::Vec &a, const BowCpuDb::Slot::Vec &b) {
    double s = 0.0;
    size_t i = 0, j = 0;
    while (i < a.words.size() && j < b.words.size()) {
        if (a.words[i] == b.words[j]) {
            const double vi = a.values[i], wi = b.values[j];
            s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            ++i;
            ++j;
        } else if (a.words[i] < b.words[j]) {
            ++i;
        } else {
            ++j;
        }
    }
    return -s / 2.0;
}

}  // namespace

int bowCpu(BowCpuDb *db, BowCall *c) {
    if (!db || !c || (c->slot != 0 && c->slot != 1)) return PLBA_E_INVALID;
    BowCpuDb::Slot &S = db->slot[c->slot];
    if (c->op == BOW_SET_VOCAB) return cpu_set_vocab(S, c->vocab);
    if (c->op == BOW_INSERT) {
        if (!S.has_vocab || c->kf_id < 0 || c->n_desc < 0 || c->n_desc > 65535 || c->cap < 0 || (c->n_desc && !c->desc) ||
            (c->cap && (!c->scores || !c->ids)) || S.rows.count(c->kf_id))
            return PLBA_E_INVALID;
        BowCpuDb::Slot::Vec v;
        cpu_transform(S, c->desc, c->n_desc, v);
        int j = 0;
        for (const auto &kv : S.rows) {
            if (!kv.second.live) continue;
            if (j < c->cap) {
                c->ids[j] = kv.first;
                c->scores[j] = cpu_score(v, kv.second);
            }
            ++j;
        }
        if (j < c->cap) {
            c->ids[j] = c->kf_id;
            c->scores[j] = cpu_score(v, v);
        }
        c->n = j + 1;
        S.rows.emplace(c->kf_id, std::move(v));
        return PLBA_OK;
    }
    auto it = S.rows.find(c->kf_id);
    if (it == S.rows.end() || !it->second.live) return PLBA_E_INVALID;
    if (c->op == BOW_REMOVE) {
        it->second.live = false;
        return PLBA_OK;
    }
    if (c->op == BOW_GET) {
        if (c->cap < 0 || (c->cap && (!c->word_ids || !c->values))) return PLBA_E_INVALID;
        c->n = (int32_t)it->second.words.size();
        for (int k = 0; k < std::min(c->cap, c->n); ++k) {
            c->word_ids[k] = it->second.words[k];
            c->values[k] = it->second.values[k];
        }
        return PLBA_OK;
    }
    return PLBA_E_INVALID;
}

}  // namespace plslam
