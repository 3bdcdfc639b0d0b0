// Place recognition on the device (plba_bow_*): DBoW2's TemplatedVocabulary<FORB>::transform
// (TemplatedVocabulary.h:1046-1084, :1198-1239), BowVector::addWeight / normalize (BowVector.cpp:34-84)
// and L1Scoring::score (ScoringObject.cpp:23-68), as insertKFBowVectorP / L / PL use them
// (src/mapHandler.cpp:4118-4239): a keyframe's descriptors become a BoW vector, which is scored
// against every stored one. TF-IDF weighting with L1 scoring only. The results are doubles that
// equal the reference's bit for bit, so every sum below runs in the reference's order; only the
// search for what to add is parallel. Three launches per insert:
//
//   k_bow_descend  16 lanes per descriptor, 16 descriptors per workgroup. From the root, a lane takes
//                  the children at positions lane, lane + 16, ... of the current node, computes the
//                  Hamming distance and keeps the smallest key (distance << 32 | position); a 16-lane
//                  xor-shuffle minimum then gives the smallest distance and, among equals, the first
//                  child (TemplatedVocabulary.h:1224: a child replaces the best only if strictly
//                  nearer). The level loop runs `depth` times and the chunk loop ceil(max_children /
//                  16) times for every lane, both validated by plba_bow_set_vocab: no input can make
//                  it spin, and every shuffle is executed by whole waves. A descriptor whose leaf
//                  weight is not > 0 gets the key kBowNoWord (:1073).
//   k_bow_vector   one workgroup: bitonic sort of the word ids (in LDS up to kBowLdsKeys, else in a
//                  global buffer), run heads compacted by a ballot scan into the new CSR row, the
//                  value of a word as the repeated sum w + w + ... (count addends, not count * w),
//                  norm = sum |v| by one thread in increasing word id, then v / norm (IEEE division)
//                  by all.
//   k_bow_score    one wave per stored live vector, and one for the new vector against itself: a lane
//                  takes one element of the stored vector and looks its word up in the new vector by
//                  binary search; the hits of the 64 lanes are then added in lane order, which is
//                  increasing word id: s += (|a - b| - |a|) - |b|, a of the new vector; the score is
//                  -s / 2 (so -0.0 with no common word).
// No floating-point atomics; every element is written by the one thread that owns it.
#pragma once

#include "../../include/plba.h"

namespace plba {

constexpr int kBowGroup = 16;        // lanes of a descriptor in the descent
constexpr int kBowDescNT = 256;
constexpr int kBowVecNT = 1024;
constexpr int kBowLdsKeys = 8192;    // keys sorted in LDS (32 KB); more are sorted in global memory
constexpr int kBowNormTile = 2048;   // values staged through LDS for the sequential norm
constexpr int kBowScoreNT = 256;     // 4 waves: 4 stored vectors per workgroup
constexpr int kBowMaxDesc = 65535;
constexpr uint32_t kBowNoWord = 0xFFFFFFFFu;

struct BowDev {
    // the vocabulary (resident)
    const int32_t *child_off, *children;  // [n_nodes+1], [child_off[n_nodes]]
    const uint32_t *node_desc;            // [n_nodes][dwords]
    const int32_t *word_id;               // [n_nodes], -1 on inner nodes
    const double *word_weight;            // [n_words] the leaf's weight, by word id
    int32_t dwords, depth, max_children;
    // the call
    const uint32_t *desc;                 // [n_desc][dwords]
    uint32_t *keys;                       // [n_desc] word id or kBowNoWord
    uint32_t *sortbuf;                    // [npad] when npad > kBowLdsKeys
    int32_t *run_start;                   // [n_desc] first sorted position of each distinct word
    int32_t n_desc, npad;                 // npad: the power of two >= max(n_desc, 1)
    // the database (CSR rows) and the live rows to score against
    int32_t *db_word;
    double *db_val;
    const int32_t *ent;                   // [n_live][2] (offset, length), in increasing kf_id
    int32_t new_off, n_live;
    int32_t *n_new;                       // length of the new row
    double *scores;                       // [n_live + 1]
};

__global__ __launch_bounds__(kBowDescNT) void k_bow_descend(BowDev D) {
    const int tid = threadIdx.x, lane = tid & (kBowGroup - 1);
    const int row = blockIdx.x * (kBowDescNT / kBowGroup) + tid / kBowGroup;
    const bool owner = row < D.n_desc;
    const int dw = D.dwords;
    uint32_t q[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) q[c] = (owner && c < dw) ? D.desc[(size_t)row * dw + c] : 0u;
    const int chunks = (D.max_children + kBowGroup - 1) / kBowGroup;
    int node = 0;
    bool at_leaf = !owner;
    for (int level = 0; level < D.depth; ++level) {
        int c0 = 0, nc = 0;
        if (!at_leaf) {
            c0 = D.child_off[node];
            nc = D.child_off[node + 1] - c0;
        }
        if (nc == 0) at_leaf = true;
        unsigned long long best = ~0ull;
        for (int ch = 0; ch < chunks; ++ch) {
            const int pos = ch * kBowGroup + lane;
            if (pos < nc) {
                const uint32_t *nd = D.node_desc + (size_t)D.children[c0 + pos] * dw;
                int d = 0;
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < dw) d += __popc(q[c] ^ nd[c]);
                const unsigned long long key = ((unsigned long long)(uint32_t)d << 32) | (uint32_t)pos;
                best = key < best ? key : best;
            }
        }
#pragma unroll
        for (int m = kBowGroup / 2; m >= 1; m >>= 1) {
            const unsigned long long o = __shfl_xor(best, m, kBowGroup);
            best = o < best ? o : best;
        }
        if (!at_leaf) node = D.children[c0 + (int)(uint32_t)best];
    }
    if (owner && lane == 0) {
        uint32_t key = kBowNoWord;
        if (D.child_off[node + 1] == D.child_off[node]) {
            const int w = D.word_id[node];
            if (w >= 0 && D.word_weight[w] > 0.0) key = (uint32_t)w;  // :1073 "not stopped"
        }
        D.keys[row] = key;
    }
}

__global__ __launch_bounds__(kBowVecNT) void k_bow_vector(BowDev D) {
#pragma clang fp contract(off)
    __shared__ uint32_t lds_keys[kBowLdsKeys];
    __shared__ double lds_val[kBowNormTile];
    __shared__ int wave_cnt[kBowVecNT / 64];
    __shared__ int s_nvalid;
    __shared__ double s_norm;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = D.n_desc, npad = D.npad;
    uint32_t *k = npad <= kBowLdsKeys ? lds_keys : D.sortbuf;
    for (int i = tid; i < npad; i += kBowVecNT) k[i] = i < n ? D.keys[i] : kBowNoWord;
    if (tid == 0) s_nvalid = 0;
    __syncthreads();
    // bitonic sort, ascending: kBowNoWord (dropped descriptors and the padding) goes last
    for (int size = 2; size <= npad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < npad / 2; t += kBowVecNT) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint32_t a = k[i], b = k[j];
                if ((a > b) == ((i & size) == 0)) {
                    k[i] = b;
                    k[j] = a;
                }
            }
            __syncthreads();
        }
    }
    // the distinct words, in order, into the new row; run_start[r] is the first position of word r
    int32_t *qw = D.db_word + D.new_off;
    double *qv = D.db_val + D.new_off;
    int nq = 0;
    for (int base = 0; base < npad; base += kBowVecNT) {  // npad is 1 .. 512 or a multiple of 1024
        const int i = base + tid;
        const uint32_t key = i < npad ? k[i] : kBowNoWord;
        const bool valid = key != kBowNoWord;
        const bool head = valid && (i == 0 || k[i - 1] != key);
        if (valid && (i == npad - 1 || k[i + 1] == kBowNoWord)) s_nvalid = i + 1;  // one thread at the most
        const unsigned long long m = __ballot(head);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kBowVecNT / 64; ++w) {
            before += w < wv ? wave_cnt[w] : 0;
            total += wave_cnt[w];
        }
        if (head) {
            const int r = nq + before + __popcll(m & ((1ull << lane) - 1ull));
            qw[r] = (int32_t)key;
            D.run_start[r] = i;
        }
        nq += total;
        __syncthreads();
    }
    // BowVector::addWeight once per descriptor: count equal addends, added one by one
    const int nvalid = s_nvalid;
    for (int r = tid; r < nq; r += kBowVecNT) {
        const int cnt = (r + 1 < nq ? D.run_start[r + 1] : nvalid) - D.run_start[r];
        const double w = D.word_weight[qw[r]];
        double v = w;
        for (int c = 1; c < cnt; ++c) v = __dadd_rn(v, w);
        qv[r] = v;
    }
    __syncthreads();
    // BowVector::normalize(L1): the norm is one sequential sum in increasing word id
    double norm = 0.0;
    for (int base = 0; base < nq; base += kBowNormTile) {
        const int cnt = min(kBowNormTile, nq - base);
        for (int i = tid; i < cnt; i += kBowVecNT) lds_val[i] = fabs(qv[base + i]);
        __syncthreads();
        if (tid == 0) {
#pragma unroll 8
            for (int i = 0; i < cnt; ++i) norm = __dadd_rn(norm, lds_val[i]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        s_norm = norm;
        *D.n_new = nq;
    }
    __syncthreads();
    norm = s_norm;
    if (norm > 0.0)
        for (int r = tid; r < nq; r += kBowVecNT) qv[r] = __ddiv_rn(qv[r], norm);
}

__global__ __launch_bounds__(kBowScoreNT) void k_bow_score(BowDev D) {
#pragma clang fp contract(off)
    const int wave = (int)((blockIdx.x * kBowScoreNT + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (wave > D.n_live) return;  // a whole wave
    const int nq = *D.n_new;
    const int32_t *qw = D.db_word + D.new_off;
    const double *qv = D.db_val + D.new_off;
    int off = D.new_off, len = nq;  // the last wave: the new vector against itself
    if (wave < D.n_live) {
        off = D.ent[2 * wave];
        len = D.ent[2 * wave + 1];
    }
    double s = 0.0;
    for (int base = 0; base < len; base += 64) {
        const int i = base + lane;
        bool hit = false;
        double t = 0.0;
        if (i < len) {
            const int32_t w = D.db_word[off + i];
            int lo = 0, hi = nq;  // the first position with qw[pos] >= w
            for (int it = 0; it < 32 && lo < hi; ++it) {
                const int mid = (lo + hi) >> 1;
                if (qw[mid] < w) lo = mid + 1;
                else hi = mid;
            }
            if (lo < nq && qw[lo] == w) {
                const double a = qv[lo], b = D.db_val[off + i];
                t = __dsub_rn(__dsub_rn(fabs(__dsub_rn(a, b)), fabs(a)), fabs(b));  // ScoringObject.cpp:41
                hit = true;
            }
        }
        unsigned long long m = __ballot(hit);
        for (int bit = 0; bit < 64 && m; ++bit) {  // the hits in lane order = increasing word id
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            s = __dadd_rn(s, __shfl(t, l, 64));
        }
    }
    if (lane == 0) D.scores[wave] = -s / 2.0;
}

}  // namespace plba
