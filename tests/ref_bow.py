"""TEST INFRASTRUCTURE: the checker of place recognition, in plain Python floats (IEEE doubles, one
rounding per operation, no contraction) and sorted dicts. Written from the rules of include/plba.h
(DBoW2 transform with TF-IDF weights, L1 normalisation and L1 score; vector_stdv; the three
insertKFBowVector variants with their float confusion matrix; lookForLoopCandidates) and independent
of the C++ restatement plslam_bow_cpu.

A vocabulary is a dict: child_off [n_nodes+1], children, node_desc [n_nodes][desc_bytes] uint8,
word_id [n_nodes] (-1 on inner nodes), weight [n_nodes], n_words. A BoW vector is a list of
(word, value) in increasing word id."""
from __future__ import annotations

import math
import struct

import numpy as np


def hamming(a: np.ndarray, b: np.ndarray) -> int:
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def descend(voc, d: np.ndarray):
    """The leaf a descriptor reaches, and the nodes on the way: at every node the child with the
    smallest distance, the first of equals."""
    node, path = 0, []
    co, ch, nd = voc["child_off"], voc["children"], voc["node_desc"]
    while co[node + 1] > co[node]:
        kids = ch[co[node]:co[node + 1]]
        # one vectorised distance per level; argmin returns the first minimum
        dist = np.unpackbits(np.bitwise_xor(nd[kids], d[None, :]), axis=1).sum(axis=1)
        best, best_d = int(kids[0]), int(dist[0])
        for k, dk in zip(kids[1:], dist[1:]):
            if int(dk) < best_d:
                best, best_d = int(k), int(dk)
        node = best
        path.append(node)
    return node, path


def transform(voc, desc: np.ndarray):
    v = {}
    for d in np.asarray(desc, np.uint8).reshape(-1, voc["node_desc"].shape[1]):
        leaf, _ = descend(voc, d)
        w = float(voc["weight"][leaf])
        if w > 0:
            word = int(voc["word_id"][leaf])
            v[word] = v[word] + w if word in v else w
    norm = 0.0
    for word in sorted(v):
        norm += math.fabs(v[word])
    if norm > 0.0:
        for word in v:
            v[word] = v[word] / norm
    return sorted(v.items())


def score(a, b) -> float:
    """L1Scoring::score(a, b): a is the first argument (the new keyframe's vector)."""
    db = dict(b)
    s = 0.0
    for word, vi in a:
        if word in db:
            wi = db[word]
            s += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
    return -s / 2.0


def vector_stdv(v) -> float:
    n = len(v)
    mean = e = 0.0
    for x in v:
        mean += x
    mean = mean / n if n else math.nan
    for x in v:
        e += (x - mean) * (x - mean)
    return math.sqrt((1.0 / n if n else math.inf) * e)


def f32(x: float) -> float:
    """A double stored in a float and read back (conf_matrix is vector<vector<float>>)."""
    return struct.unpack("f", struct.pack("f", x))[0] if math.isfinite(x) and abs(x) < 3e38 else \
        float(np.float32(x))


def combined(score_p: float, score_l: float, n_pt: int, n_ls: int, std_pt: float, std_ls: float) -> float:
    """src/mapHandler.cpp:4226-4228, in that order. A zero n_pl or std_pl divides by zero as the
    reference does: NaN (0 / 0) or an infinity."""
    def div(a, b):
        if b == 0:
            return math.nan if (a == 0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
        return a / b
    n_pl, std_pl = n_pt + n_ls, std_ls + std_pt
    s = 0.0
    s += div(score_p * n_pt + score_l * n_ls, n_pl)
    s += div(score_p * std_pt + score_l * std_ls, std_pl)
    return s


class Map:
    """insertKFBowVectorP / L / PL over a growing map: the vectors, the live flags and the float
    conf_matrix, grown with zeros."""

    def __init__(self, voc_p, voc_l):
        self.voc = (voc_p, voc_l)
        self.vec = {}       # kf_idx -> (vector_p, vector_l)
        self.live = {}
        self.conf = np.zeros((0, 0), np.float32)

    def _grow(self, n):
        if n > len(self.conf):
            c = np.zeros((n, n), np.float32)
            c[:len(self.conf), :len(self.conf)] = self.conf
            self.conf = c

    def cull(self, kf_idx):
        self.live[kf_idx] = False

    def insert(self, kf_idx, pdesc, ldesc, has_points=True, has_lines=True, pl=None, spl=None, epl=None):
        vp = transform(self.voc[0], pdesc) if has_points else []
        vl = transform(self.voc[1], ldesc) if has_lines else []
        self._grow(kf_idx + 1)
        if has_points and has_lines:
            pl = np.asarray(pl, np.float64).reshape(-1, 2)
            mid = [((float(s[0]) + float(e[0])) * 0.5, (float(s[1]) + float(e[1])) * 0.5)
                   for s, e in zip(np.asarray(spl, np.float64).reshape(-1, 2), np.asarray(epl, np.float64).reshape(-1, 2))]
            std_pt = vector_stdv([float(x) for x in pl[:, 0]]) + vector_stdv([float(x) for x in pl[:, 1]])
            std_ls = vector_stdv([m[0] for m in mid]) + vector_stdv([m[1] for m in mid])
            n_pt, n_ls = len(pl), len(mid)

        def sc(other_p, other_l):
            if has_points and has_lines:
                return combined(score(vp, other_p), score(vl, other_l), n_pt, n_ls, std_pt, std_ls)
            return score(vp, other_p) if has_points else score(vl, other_l)
        for i in range(kf_idx):
            if self.live.get(i):
                s = np.float32(sc(*self.vec[i]))
                self.conf[kf_idx, i] = s
                self.conf[i, kf_idx] = s
        self.conf[kf_idx, kf_idx] = np.float32(sc(vp, vl))
        self.vec[kf_idx] = (vp, vl)
        self.live[kf_idx] = True


DEFAULT_SEARCH = dict(lc_kf_dist=50, lc_kf_max_dist=50, lc_nkf_closest=4, min_lm_cov_graph=75, min_kf_local_map=3)


def look_for_loop_candidates(conf, full_graph, live, kf_curr_idx, lc_kf_dist=50, lc_kf_max_dist=50, lc_nkf_closest=4,
                             min_lm_cov_graph=75, min_kf_local_map=3):
    """src/mapHandler.cpp:4241-4301. Returns (is_candidate, kf_prev_idx, exit) where exit names the
    gate that decided: 'too_few', 'best_too_low', 'too_few_neighbours' or 'accepted'. The sort is
    descending by score, ties by increasing index, NaN last."""
    cand = [(i, float(conf[i][kf_curr_idx])) for i in range(max(kf_curr_idx - lc_kf_dist, 0)) if live[i]]
    if not len(cand) > lc_kf_max_dist:
        return False, -1, "too_few"
    cand.sort(key=lambda t: (1, 0.0, t[0]) if t[1] != t[1] else (0, -t[1], t[0]))
    lc_min_score = 1.0
    for i in range(kf_curr_idx):
        if full_graph[i][kf_curr_idx] >= min_lm_cov_graph or kf_curr_idx - i <= min_kf_local_map + 3:
            s = float(conf[i][kf_curr_idx])
            if s < lc_min_score and s > 0.001:
                lc_min_score = s
    idx_max = cand[0][0]
    if not cand[0][1] >= lc_min_score:
        return False, -1, "best_too_low"
    n_closest = 0
    for idx, s in cand[1:]:
        if abs(idx - idx_max) <= lc_kf_max_dist and s >= lc_min_score * 0.8:
            n_closest += 1
    if n_closest >= lc_nkf_closest:
        return True, idx_max, "accepted"
    return False, -1, "too_few_neighbours"
