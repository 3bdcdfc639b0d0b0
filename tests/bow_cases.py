"""TEST INFRASTRUCTURE: seeded synthetic vocabularies and descriptor sets shared by
tests/test_gpu_bow.py (device against the checker), tests/test_host_bow.py (host mirror against the
checker) and tests/test_bow_oracle.py (the properties of exactly these cases), with the checker's
results computed once. The reference ships no vocabulary: these are built here.

A descriptor set draws half of its rows near random leaves (a few flipped bits) and half uniformly, so
that words repeat within a keyframe and recur between keyframes."""
from __future__ import annotations

import functools

import numpy as np

import ref_bow

N_DESC = [0, 1, 2, 63, 65, 257, 600]


def _freeze(voc):
    for v in voc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return voc


def from_children(kids: list, desc_bytes: int, rng, zero_third: bool = False, weights=None):
    """A vocabulary from a list of child lists (node 0 the root). Words are numbered over the leaves
    in node order; idf-like weights in (0.5, 8)."""
    n = len(kids)
    child_off = np.zeros(n + 1, np.int32)
    child_off[1:] = np.cumsum([len(k) for k in kids])
    children = np.array([c for k in kids for c in k], np.int32)
    word_id = np.full(n, -1, np.int32)
    leaves = [i for i in range(n) if not kids[i]]
    word_id[leaves] = np.arange(len(leaves), dtype=np.int32)
    weight = np.zeros(n)
    weight[leaves] = rng.uniform(0.5, 8.0, len(leaves)) if weights is None else weights
    if zero_third:
        weight[leaves[::3]] = 0.0
    node_desc = rng.integers(0, 256, (n, desc_bytes), dtype=np.uint8)
    return _freeze(dict(child_off=child_off, children=children, node_desc=node_desc, word_id=word_id, weight=weight,
                        n_words=len(leaves), desc_bytes=desc_bytes))


def full_tree(k: int, levels: int) -> list:
    """Child lists of the full k-ary tree with `levels` levels below the root, breadth first."""
    kids, frontier = [[]], [0]
    for _ in range(levels):
        nxt = []
        for node in frontier:
            for _ in range(k):
                kids.append([])
                kids[node].append(len(kids) - 1)
                nxt.append(len(kids) - 1)
        frontier = nxt
    return kids


# node 0 root -> 1 (leaf, depth 1), 2 (single child 3), 4; 3 -> 5, 6 (leaves, depth 3);
# 4 -> 7, 8, 9; 9 -> 10, 11 (depth 3); children listed out of node order on purpose
RAGGED = [[1, 4, 2], [], [3], [6, 5], [9, 7, 8], [], [], [], [], [11, 10], [], []]


@functools.lru_cache(maxsize=None)
def vocab(name: str):
    rng = np.random.default_rng(abs(hash_name(name)))
    if name == "k10L3":
        return from_children(full_tree(10, 3), 32, rng)
    if name == "k3L2":
        return from_children(full_tree(3, 2), 32, rng)
    if name == "ragged":
        return from_children(RAGGED, 32, rng)
    if name == "zeros":
        return from_children(full_tree(6, 2), 32, rng, zero_third=True)
    if name == "wide":     # 40 children of one node: more than one chunk of 16 lanes
        return from_children([list(range(1, 41))] + [[] for _ in range(40)], 32, rng)
    if name == "db8":
        return from_children(full_tree(5, 2), 8, rng)
    if name == "db64":
        return from_children(full_tree(5, 2), 64, rng)
    if name == "lines":    # the second slot of the map tests
        return from_children(full_tree(4, 3), 32, rng)
    raise KeyError(name)


VOCABS = ["k10L3", "k3L2", "ragged", "zeros", "wide", "db8", "db64"]


def hash_name(name: str) -> int:
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) + 90001


def flip(rng, row: np.ndarray, k: int) -> np.ndarray:
    bits = np.unpackbits(row)
    bits[rng.choice(len(bits), k, replace=False)] ^= 1
    return np.packbits(bits)


@functools.lru_cache(maxsize=None)
def descriptors(name: str, n: int, seed: int = 0, pool: int = 40):
    """[n][desc_bytes] uint8, read-only: half near one of `pool` leaves fixed per vocabulary (so that
    keyframes share words), half uniform."""
    voc = vocab(name)
    db = voc["desc_bytes"]
    leaves = np.flatnonzero(voc["word_id"] >= 0)
    fixed = np.random.default_rng(hash_name(name) + 5).choice(leaves, min(pool, len(leaves)), replace=False)
    rng = np.random.default_rng(7919 * seed + 31 * n + hash_name(name))
    d = rng.integers(0, 256, (n, db), dtype=np.uint8)
    for i in range(0, n, 2):
        d[i] = flip(rng, voc["node_desc"][rng.choice(fixed)], int(rng.integers(0, db // 8 + 1)))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference_vector(name: str, n: int, seed: int = 0):
    return ref_bow.transform(vocab(name), descriptors(name, n, seed))


def as_arrays(vec):
    return (np.array([w for w, _ in vec], np.int32), np.array([v for _, v in vec], np.float64))


# ---- constructed cases
@functools.lru_cache(maxsize=None)
def tie_case():
    """Two children of the root with the same descriptor, and a query at equal distance of both (and
    nearer to them than to the third): the first listed child wins. Returns (vocabulary, query rows,
    first child, second child)."""
    rng = np.random.default_rng(11)
    voc = dict(from_children([[3, 1, 2], [], [], []], 32, rng))
    nd = voc["node_desc"].copy()
    nd[1] = nd[3]
    nd[2] = ~nd[3]
    voc["node_desc"] = nd
    q = np.stack([flip(rng, nd[3], 5), nd[3].copy()])
    return _freeze(voc), q, 3, 1


@functools.lru_cache(maxsize=None)
def sum_case(count: int):
    """A word of weight 0.1 hit `count` times (6 or 10), and another word of weight 0.3 hit once:
    the repeated sum of 0.1 is not count * 0.1."""
    rng = np.random.default_rng(12 + count)
    voc = from_children([[1, 2], [], []], 32, rng, weights=np.array([0.1, 0.3]))
    nd = voc["node_desc"]
    q = np.stack([flip(rng, nd[1], 3) for _ in range(count)] + [flip(rng, nd[2], 3)])
    return voc, q


@functools.lru_cache(maxsize=None)
def stopped_case():
    """Every leaf has weight 0: every descriptor is dropped and the vector is empty."""
    rng = np.random.default_rng(13)
    voc = from_children(full_tree(3, 2), 32, rng, weights=np.zeros(9))
    return voc, rng.integers(0, 256, (20, 32), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def disjoint_case():
    """Two descriptor sets that reach different leaves: no common word, the score is -0.0."""
    rng = np.random.default_rng(14)
    voc = vocab("k3L2")
    leaves = np.flatnonzero(voc["word_id"] >= 0)
    a = np.stack([flip(rng, voc["node_desc"][leaves[i % 4]], 2) for i in range(9)])
    b = np.stack([flip(rng, voc["node_desc"][leaves[4 + i % 5]], 2) for i in range(7)])
    return voc, a, b


# ---- malformed vocabularies: every rule of plba_bow_set_vocab, from a valid small tree
def malformed():
    base = vocab("k3L2")

    def edit(**kw):
        v = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in base.items()}
        for k, f in kw.items():
            v[k] = f(v[k]) if callable(f) else f
        return v

    def put(i, x):
        def f(a):
            a[i] = x
            return a
        return f
    n = len(base["word_id"])
    out = {
        "child out of range": edit(children=put(0, n)),
        "child negative": edit(children=put(0, -2)),
        "child is the root": edit(children=put(5, 0)),
        "node reached twice": edit(children=put(1, 1)),          # node 2 unreached, node 1 twice
        "cycle": edit(children=put(3, 1)),                       # node 1 lists itself
        "leaf without word": edit(word_id=put(n - 1, -1)),
        "leaf word out of range": edit(word_id=put(n - 1, base["n_words"])),
        "inner node with word": edit(word_id=put(1, 0)),
        "weight nan": edit(weight=put(n - 2, np.nan)),
        "weight inf": edit(weight=put(n - 2, np.inf)),
    }
    for db in (0, 30, 68):
        out[f"desc_bytes {db}"] = edit(desc_bytes=db)
    return out


# ---- a map: keyframes with point and line descriptors, pixels and line endpoints
@functools.lru_cache(maxsize=None)
def keyframe(kf_idx: int, n_pt: int = 70, n_ls: int = 20):
    rng = np.random.default_rng(500 + kf_idx)
    return dict(pdesc=descriptors("k10L3", n_pt, seed=100 + kf_idx), ldesc=descriptors("lines", n_ls, seed=200 + kf_idx),
                pl=rng.uniform(0, 640, (n_pt, 2)), spl=rng.uniform(0, 640, (n_ls, 2)), epl=rng.uniform(0, 640, (n_ls, 2)))


@functools.lru_cache(maxsize=None)
def reference_map(mode: str, n_kf: int = 12, culled: int = 4, empty_kf: int = -1):
    """The checker's map after n_kf inserts (mode 'P', 'L' or 'PL'), keyframe `culled` removed after
    insert culled + 2; keyframe empty_kf (if any) has no feature at all: its PL scores are NaN."""
    m = ref_bow.Map(vocab("k10L3"), vocab("lines"))
    for i in range(n_kf):
        kf = keyframe(i, 0, 0) if i == empty_kf else keyframe(i)
        m.insert(i, kf["pdesc"], kf["ldesc"], "P" in mode, "L" in mode, kf["pl"], kf["spl"], kf["epl"])
        if i == culled + 2:
            m.cull(culled)
    m.conf.setflags(write=False)
    return m


# ---- lookForLoopCandidates: confusion matrices that take every exit
# min_kf_local_map 1: the recent keyframes (kf_curr_idx - i <= 4) stay clear of the candidates (i < kf_curr_idx - 5)
SMALL = dict(lc_kf_dist=5, lc_kf_max_dist=3, lc_nkf_closest=2, min_lm_cov_graph=75, min_kf_local_map=1)


def search_case(kind: str, n: int = 14, params=None):
    """(conf float32 [n][n], full_graph, live, kf_curr_idx, params, expected exit). The current keyframe
    is n - 1; the recent keyframes score 0.3 (lc_min_score), the old ones 0.05 but for what `kind`
    plants around keyframe 2."""
    p = dict(params or SMALL)
    cur = n - 1
    conf = np.full((n, n), 0.05, np.float32)
    for i in range(cur - p["min_kf_local_map"] - 3, cur):
        conf[i, cur] = conf[cur, i] = 0.3
    conf[cur, cur] = 1.0
    live = [True] * n
    fg = np.zeros((n, n), np.uint32)
    first_old = max(cur - p["lc_kf_dist"], 0)
    lo = 2
    if kind == "too_few":
        for i in range(first_old):
            live[i] = i < p["lc_kf_max_dist"]     # exactly lc_kf_max_dist live: not more than it
    elif kind == "best_too_low":
        conf[lo, cur] = conf[cur, lo] = 0.29
    elif kind == "too_few_neighbours":
        conf[lo, cur] = conf[cur, lo] = 0.5
        conf[lo + 1, cur] = conf[cur, lo + 1] = 0.25
    elif kind == "accepted":
        conf[lo, cur] = conf[cur, lo] = 0.5
        for i in range(lo + 1, lo + 1 + p["lc_nkf_closest"]):
            conf[i, cur] = conf[cur, i] = 0.25
    elif kind == "tie":       # two equal best scores: the lower index is the candidate
        conf[lo, cur] = conf[cur, lo] = 0.5
        conf[lo + 1, cur] = conf[cur, lo + 1] = 0.5
        for i in range(lo + 2, lo + 1 + p["lc_nkf_closest"]):
            conf[i, cur] = conf[cur, i] = 0.25
        conf[0, cur] = conf[cur, 0] = np.nan      # and a NaN sorts last
    else:
        raise KeyError(kind)
    return conf, fg, live, cur, p, ("accepted" if kind == "tie" else kind)


SEARCH_KINDS = ["too_few", "best_too_low", "too_few_neighbours", "accepted", "tie"]
