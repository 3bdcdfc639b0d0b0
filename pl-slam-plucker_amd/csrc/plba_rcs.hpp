// plba_rcs.hpp — assembly of the reduced camera system (Schur triples -> band / dense matrix)
// and the pose update every factorisation kernel ends with.
#pragma once

#include "plba_dev.hpp"

namespace plba {

// ---------------------------------------------------------------- reduced camera system
// one entry of block b: e < 36 the 6x6 value (Hpp + λI on the diagonal minus Σ chunks), 36..41
// the right-hand side b_s = b_p - Σ A_eᵀq_e (diagonal blocks only)
__device__ __forceinline__ void rcs_finalize_entry(const Dev &d, int b, int e, double sacc) {
    const int i1 = d.blk_i1[b], i2 = d.blk_i2[b];
    const bool diag = i1 == i2;
    if (e >= 36 && !diag) return;
    const int n = d.n;
    if (e >= 36) {
        const double v = d.bp[(size_t)i1 * 6 + (e - 36)] - sacc;
        d.bs[6 * i1 + (e - 36)] = v;
        if (d.twisted) d.bs2[6 * (d.nf - 1 - i1) + (e - 36)] = v;
        return;
    }
    const int r = e / 6, c = e % 6;
    if (diag) {
        // (sharded: the exchanged sum already holds −Hpp, k_rcs_blockpart)
        double h = (d.Hpp ? d.Hpp[(size_t)i1 * 36 + e] : 0.0) - sacc;
        // a free pose with no active edge is not in g2o's system (SparseOptimizer activation,
        // SURVEY.md §8 A13); its all-zero block row becomes I (x = 0 exactly) instead of λI,
        // which would be a zero pivot at λ = 0
        // (hand-rolled LM: Marquardt damping H(i,i) += λ·H(i,i), src/mapHandler.cpp:2114-2115)
        if (r == c)
            h += d.pact[i1] == 0.0 ? 1.0
                 : lm_hand_rolled(d.ctrl->hlm) ? d.lam * (d.Hpp ? d.Hpp[(size_t)i1 * 36 + e] : d.Hdg[(size_t)i1 * 6 + r])
                                 : d.lam;
        if (d.band_mode) d.Bd[((size_t)i1 * (d.bw + 1)) * 36 + e] = h;
        else d.Ad[(size_t)(6 * i1 + r) + (size_t)(6 * i1 + c) * n] = h;
        if (d.twisted) d.Bd2[((size_t)(d.nf - 1 - i1) * (d.bw + 1)) * 36 + e] = h;
    } else {
        if (d.band_mode) d.Bd[((size_t)i2 * (d.bw + 1) + (i2 - i1)) * 36 + c * 6 + r] = -sacc;
        else d.Ad[(size_t)(6 * i2 + c) + (size_t)(6 * i1 + r) * n] = -sacc;
        // reversed row nf-1-i1 holds block (i1, i2) = (i1, i1 + w) in its natural orientation
        if (d.twisted) d.Bd2[((size_t)(d.nf - 1 - i1) * (d.bw + 1) + (i2 - i1)) * 36 + r * 6 + c] = -sacc;
    }
}

// Chunked reduced-camera assembly, pass 1: one wave per chunk of <= kChunk triples of one
// block; each lane accumulates A₁ᵀ(Z₁Z₂ᵀ)A₂ (36) and, for self-triples of a diagonal block,
// A_eᵀ q_e (6); the wave reduces through LDS in fixed lane order (deterministic).
// STAGED (default): the 64 triples of a batch fetch their A/Z rows cooperatively — load j of
// the wave covers rows (64j + lane)/6 of the batch's A₁ (16 B per lane, consecutive lanes on
// consecutive pieces of one 96-B row), so one load instruction touches ~8-16 cache lines
// instead of 64 (one per lane and piece); the rows land in LDS and every lane then reads its
// own row. The arithmetic per lane is unchanged (bitwise-identical sums).
typedef double dbl2 __attribute__((ext_vector_type(2)));  // register-promotable 16-B pair
template <bool STAGED>
__global__ __launch_bounds__(64) void k_rcs_chunk(Dev d0) {
    TRIAL_SLOT(blockIdx.y)
    __shared__ double smem[64 * 43];  // staging: A₁ | A₂ (64x12) | Z₁ | Z₂ (64x8); then red[64][43]
    double(*red)[43] = reinterpret_cast<double(*)[43]>(smem);
    // XCD-aware remap (blocks are dealt round-robin over the 8 XCDs): each XCD gets a contiguous
    // run of chunks = a contiguous range of RCS block rows, so the A/Z rows of the landmarks
    // they couple are re-read from that XCD's L2 instead of the fabric (speed only). The grid's x
    // extent is padded to a multiple of 8 so that every trial slot (blockIdx.y) sees the same
    // block -> XCD assignment; the padding blocks exit.
    const int nb = d.nch, per = (nb + 7) / 8, xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
    const int full = nb - 8 * (per - 1);  // XCDs that get `per` chunks (the rest get per-1)
    if (xcd >= full && slot >= per - 1) return;  // padding
    const int ch = xcd < full ? xcd * per + slot : full * per + (xcd - full) * (per - 1) + slot;
    const int lane = threadIdx.x;
    const int hlm = d.ctrl->hlm;
    const int b = d.ch_blk[ch];
    const bool diag = d.blk_i1[b] == d.blk_i2[b];
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; ++k) acc[k] = 0.0;
    const int t0 = d.ch_off[ch], t1 = d.ch_off[ch + 1];
    // the next batch's triple indices are loaded one batch ahead, so their latency hides behind
    // this batch's row loads instead of preceding them (rows past the chunk re-read a valid triple)
    int2 nx = make_int2(0, 0);
    if (t0 < t1) nx = reinterpret_cast<const int2 *>(d.trip)[min(t0 + lane, t1 - 1)];
#pragma unroll 1
    for (int q = 0; q < kChunk / 64; ++q) {
        const int tb = t0 + 64 * q;
        if (tb >= t1) break;  // wave-uniform
        const int t = tb + lane;
        const int e1 = nx.x, e2 = nx.y;
        if (tb + 64 < t1) nx = reinterpret_cast<const int2 *>(d.trip)[min(tb + 64 + lane, t1 - 1)];
        double z1[8], z2[8], a1[12], a2[12];
        if (STAGED) {
            dbl2 *sA1 = reinterpret_cast<dbl2 *>(smem), *sA2 = sA1 + 384;
            dbl2 *sZ1 = sA2 + 384, *sZ2 = sZ1 + 256;
            dbl2 v1[6], v2[6], w1[4], w2[4];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int pc = 64 * j + lane, r = pc / 6, k = pc - 6 * r;
                const int f1 = __shfl(e1, r, 64), f2 = __shfl(e2, r, 64);
                v1[j] = reinterpret_cast<const dbl2 *>(d.A + (size_t)f1 * 12)[k];
                v2[j] = reinterpret_cast<const dbl2 *>(d.A + (size_t)f2 * 12)[k];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 16 * j + (lane >> 2), k = lane & 3;
                const int f1 = __shfl(e1, r, 64), f2 = __shfl(e2, r, 64);
                w1[j] = reinterpret_cast<const dbl2 *>(d.Z + (size_t)f1 * 8)[k];
                w2[j] = reinterpret_cast<const dbl2 *>(d.Z + (size_t)f2 * 8)[k];
            }
            __syncthreads();  // the previous batch's rows are read (one wave: a cheap barrier)
            // Bank-conflict-free row reads (ds_read_b128: 16-lane groups, bank (a/4) mod 64):
            //  Z rows (4 pieces, 64-B stride: lanes l, l+4, l+8, l+12 share a bank window) are
            //  stored rotated by ρ(r) = (r >> 2) & 3 pieces, so the lane reading its row at step k
            //  fetches piece k from position (k + ρ) mod 4; stores stay conflict-free.
            //  A rows (6 pieces, 96-B stride: lanes l and l+8 collide) are stored linearly and read
            //  rotated by ρ = (lane >> 3) & 1, the pieces put back in order with selects (rotating
            //  the stores instead would move the conflicts to the stores).
#pragma unroll
            for (int j = 0; j < 6; ++j) { sA1[64 * j + lane] = v1[j]; sA2[64 * j + lane] = v2[j]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 16 * j + (lane >> 2), k = lane & 3, pos = 4 * r + ((k + ((r >> 2) & 3)) & 3);
                sZ1[pos] = w1[j];
                sZ2[pos] = w2[j];
            }
            __syncthreads();
            const int ra = (lane >> 3) & 1, rz = (lane >> 2) & 3;
            dbl2 tA1[6], tA2[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int pk = k + ra < 6 ? k + ra : k + ra - 6;
                tA1[k] = sA1[6 * lane + pk];
                tA2[k] = sA2[6 * lane + pk];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {  // piece k sits in tA[k] (ra = 0) or tA[k - 1] (ra = 1)
                const dbl2 x = ra ? tA1[(k + 5) % 6] : tA1[k], y = ra ? tA2[(k + 5) % 6] : tA2[k];
                a1[2 * k] = x.x; a1[2 * k + 1] = x.y; a2[2 * k] = y.x; a2[2 * k + 1] = y.y;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int pos = 4 * lane + ((k + rz) & 3);
                const dbl2 x = sZ1[pos], y = sZ2[pos];
                z1[2 * k] = x.x; z1[2 * k + 1] = x.y; z2[2 * k] = y.x; z2[2 * k + 1] = y.y;
            }
        } else {
            const double *Z1 = d.Z + (size_t)e1 * 8, *Z2 = d.Z + (size_t)e2 * 8;
            const double *A1 = d.A + (size_t)e1 * 12, *A2 = d.A + (size_t)e2 * 12;
#pragma unroll
            for (int k = 0; k < 8; ++k) { z1[k] = Z1[k]; z2[k] = Z2[k]; }
#pragma unroll
            for (int k = 0; k < 12; ++k) { a1[k] = A1[k]; a2[k] = A2[k]; }
        }
        if (t < t1) {
            double m00 = 0, m01 = 0, m10 = 0, m11 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m00 = fma(z1[k], z2[k], m00);
                m01 = fma(z1[k], z2[4 + k], m01);
                m10 = fma(z1[4 + k], z2[k], m10);
                m11 = fma(z1[4 + k], z2[4 + k], m11);
            }
            // hand-rolled LM: A has one live row, so only m00 is used — and a GBA line's Z_e
            // (6 entries) spills into Z's second row: the full 8-entry product
            if (hlm == kLmLbaPlucker) m00 = m01;  // z_1 · (S z_2): row 1 of Z carries S z_0 (edge_schur_body)
            else if (hlm != kLmG2o) m00 += m11;
            double Q[12];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                Q[k] = m00 * a2[k] + m01 * a2[6 + k];
                Q[6 + k] = m10 * a2[k] + m11 * a2[6 + k];
            }
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) acc[r * 6 + c] += a1[r] * Q[c] + a1[6 + r] * Q[6 + c];
            if (diag && e1 == e2) {
                const double q0 = d.q[(size_t)e1 * 2], q1 = d.q[(size_t)e1 * 2 + 1];
#pragma unroll
                for (int r = 0; r < 6; ++r) acc[36 + r] += a1[r] * q0 + a1[6 + r] * q1;
            }
        }
    }
    if (STAGED) __syncthreads();  // the staging rows are read before red overwrites them
#pragma unroll
    for (int k = 0; k < 42; ++k) red[lane][k] = acc[k];
    __syncthreads();
    if (lane < 42) {
        double sacc = 0.0;
        for (int l = 0; l < 64; ++l) sacc += red[l][lane];
        st_sc1(d.ch_part + (size_t)ch * 42 + lane, sacc);
    }
    // the last chunk of block b to arrive assembles the block (the k_rcs_finalize entry work)
    if (d.fold && arrive_last(d.cnt_rcs + b, d.blk_ch[b + 1] - d.blk_ch[b]) && lane < 42) {
        double sacc = 0.0;
        const int c1 = d.blk_ch[b + 1];
        for (int c0 = d.blk_ch[b]; c0 < c1; c0 += 4) {  // 4 partials in flight, summed in chunk order
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = c0 + u < c1 ? ld_sc1(d.ch_part + (size_t)(c0 + u) * 42 + lane) : 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) sacc += v[u];
        }
        rcs_finalize_entry(d, b, lane, sacc);
    }
}

// Chunked reduced-camera assembly with two lanes per triple, for windows with more chunks than
// k_rcs_chunk's waves can hold at once (chunk_half_min, plba.hip): lane h·32 + p takes triple p
// of a 32-triple batch and accumulates block rows 3h .. 3h+2 of A₁ᵀ(Z₁Z₂ᵀ)A₂ (18) and of A_eᵀq_e
// (3). Half the accumulators and half the staging per wave: 216 → 146 VGPRs and 22 → 11 KB of LDS,
// 3 waves per SIMD instead of 1.75 to hide the row loads, at twice the batches per wave (so a
// window whose chunks all fit at once keeps k_rcs_chunk: C3 24.9 vs 25.3 µs; C5 121.7 → 114.7 µs).
// The per-element sums run over the same triples in another lane partition (deterministic, not
// bitwise equal to k_rcs_chunk's).
constexpr int kChhMinB = 3;  // waves per SIMD the register budget is sized for (4 spills: 115 -> 226 us at C5)
__global__ __launch_bounds__(64, kChhMinB) void k_rcs_chunk_h(Dev d0) {
    TRIAL_SLOT(blockIdx.y)
    constexpr int NB = 32, NA = 22;  // triples per batch; accumulators per lane (21) padded
    __shared__ double smem[64 * NA];  // staging: A₁ | A₂ (32x12) | Z₁ | Z₂ (32x8); then red[64][NA]
    double(*red)[NA] = reinterpret_cast<double(*)[NA]>(smem);
    // XCD-aware chunk order (as k_rcs_chunk)
    const int nb = d.nch, per = (nb + 7) / 8, xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
    const int full = nb - 8 * (per - 1);
    if (xcd >= full && slot >= per - 1) return;  // padding
    const int ch = xcd < full ? xcd * per + slot : full * per + (xcd - full) * (per - 1) + slot;
    const int lane = threadIdx.x, p = lane & (NB - 1), h = lane >> 5;
    const int hlm = d.ctrl->hlm;
    const int b = d.ch_blk[ch];
    const bool diag = d.blk_i1[b] == d.blk_i2[b];
    double acc[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) acc[k] = 0.0;
    const int t0 = d.ch_off[ch], t1 = d.ch_off[ch + 1];
    int2 nx = make_int2(0, 0);
    if (t0 < t1) nx = reinterpret_cast<const int2 *>(d.trip)[min(t0 + p, t1 - 1)];
    dbl2 *sA1 = reinterpret_cast<dbl2 *>(smem), *sA2 = sA1 + NB * 6;
    dbl2 *sZ1 = sA2 + NB * 6, *sZ2 = sZ1 + NB * 4;
#pragma unroll 1
    for (int q = 0; q < kChunk / NB; ++q) {
        const int tb = t0 + NB * q;
        if (tb >= t1) break;  // wave-uniform
        const int t = tb + p;
        const int e1 = nx.x, e2 = nx.y;
        if (tb + NB < t1) nx = reinterpret_cast<const int2 *>(d.trip)[min(tb + NB + p, t1 - 1)];
        // cooperative row loads: A pieces 64j + lane of the batch's 32 x 6, Z pieces of 32 x 4
        dbl2 v1[3], v2[3], w1[2], w2[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int pc = 64 * j + lane, r = pc / 6, k = pc - 6 * r;
            const int f1 = __shfl(e1, r, 64), f2 = __shfl(e2, r, 64);
            v1[j] = reinterpret_cast<const dbl2 *>(d.A + (size_t)f1 * 12)[k];
            v2[j] = reinterpret_cast<const dbl2 *>(d.A + (size_t)f2 * 12)[k];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 16 * j + (lane >> 2), k = lane & 3;
            const int f1 = __shfl(e1, r, 64), f2 = __shfl(e2, r, 64);
            w1[j] = reinterpret_cast<const dbl2 *>(d.Z + (size_t)f1 * 8)[k];
            w2[j] = reinterpret_cast<const dbl2 *>(d.Z + (size_t)f2 * 8)[k];
        }
        __syncthreads();  // the previous batch's rows are read
        // bank-conflict-free reads as k_rcs_chunk (rotated Z stores, rotated A reads)
#pragma unroll
        for (int j = 0; j < 3; ++j) { sA1[64 * j + lane] = v1[j]; sA2[64 * j + lane] = v2[j]; }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 16 * j + (lane >> 2), k = lane & 3, pos = 4 * r + ((k + ((r >> 2) & 3)) & 3);
            sZ1[pos] = w1[j];
            sZ2[pos] = w2[j];
        }
        __syncthreads();
        double m00 = 0, m01 = 0, m10 = 0, m11 = 0;
        {
            const int rz = (p >> 2) & 3;
            double z1[8], z2[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int pos = 4 * p + ((k + rz) & 3);
                const dbl2 x = sZ1[pos], y = sZ2[pos];
                z1[2 * k] = x.x; z1[2 * k + 1] = x.y; z2[2 * k] = y.x; z2[2 * k + 1] = y.y;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m00 = fma(z1[k], z2[k], m00);
                m01 = fma(z1[k], z2[4 + k], m01);
                m10 = fma(z1[4 + k], z2[k], m10);
                m11 = fma(z1[4 + k], z2[4 + k], m11);
            }
        }
        if (hlm == kLmLbaPlucker) m00 = m01;  // (as k_rcs_chunk)
        else if (hlm != kLmG2o) m00 += m11;
        // Q = (Z₁Z₂ᵀ) A₂ from the A₂ row (read rotated as k_rcs_chunk), then this lane's A₁
        // entries 3h .. 3h+2 of both residual rows (pieces 3h/2, 3h/2 + 1 and 3 + the same)
        const int ra = (p >> 3) & 1;
        double Q[12];
        {
            dbl2 tA2[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) tA2[k] = sA2[6 * p + (k + ra < 6 ? k + ra : k + ra - 6)];
            double a2[12];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const dbl2 y = ra ? tA2[(k + 5) % 6] : tA2[k];
                a2[2 * k] = y.x; a2[2 * k + 1] = y.y;
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                Q[k] = m00 * a2[k] + m01 * a2[6 + k];
                Q[6 + k] = m10 * a2[k] + m11 * a2[6 + k];
            }
        }
        double a1[6];
        {
            const int k0 = h;  // pieces h, h+1 hold entries 2h .. 2h+3 ⊇ 3h .. 3h+2
            const dbl2 x0 = sA1[6 * p + k0], x1 = sA1[6 * p + k0 + 1];
            const dbl2 y0 = sA1[6 * p + 3 + k0], y1 = sA1[6 * p + 4 + k0];
            // h = 0: (x0.x, x0.y, x1.x); h = 1: (x0.y, x1.x, x1.y) — entries 3h + rr = 2h + (h + rr)
            a1[0] = h ? x0.y : x0.x;
            a1[1] = h ? x1.x : x0.y;
            a1[2] = h ? x1.y : x1.x;
            a1[3] = h ? y0.y : y0.x;
            a1[4] = h ? y1.x : y0.y;
            a1[5] = h ? y1.y : y1.x;
        }
        if (t < t1) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) acc[r * 6 + c] += a1[r] * Q[c] + a1[3 + r] * Q[6 + c];
            if (diag && e1 == e2) {
                const double q0 = d.q[(size_t)e1 * 2], q1 = d.q[(size_t)e1 * 2 + 1];
#pragma unroll
                for (int r = 0; r < 3; ++r) acc[18 + r] += a1[r] * q0 + a1[3 + r] * q1;
            }
        }
    }
    __syncthreads();  // the staging rows are read before red overwrites them
#pragma unroll
    for (int k = 0; k < 21; ++k) red[lane][k] = acc[k];
    __syncthreads();
    if (lane < 42) {
        // entry (r, c) of the block (lane < 36) or row r of the right-hand side (36..41): the 32
        // lanes of half r / 3, in lane order
        const int r = lane < 36 ? lane / 6 : lane - 36, hh = r / 3;
        const int k = lane < 36 ? (r % 3) * 6 + lane % 6 : 18 + r % 3;
        double sacc = 0.0;
        for (int l = 0; l < NB; ++l) sacc += red[hh * NB + l][k];
        st_sc1(d.ch_part + (size_t)ch * 42 + lane, sacc);
    }
    if (d.fold && arrive_last(d.cnt_rcs + b, d.blk_ch[b + 1] - d.blk_ch[b]) && lane < 42) {
        double sacc = 0.0;
        const int c1 = d.blk_ch[b + 1];
        for (int c0 = d.blk_ch[b]; c0 < c1; c0 += 4) {  // 4 partials in flight, summed in chunk order
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = c0 + u < c1 ? ld_sc1(d.ch_part + (size_t)(c0 + u) * 42 + lane) : 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) sacc += v[u];
        }
        rcs_finalize_entry(d, b, lane, sacc);
    }
}

// sharded pass 2a: this rank's per-block sums (chunks in order) into the all-reduced array
__global__ __launch_bounds__(kBlock) void k_rcs_blockpart(Dev d0) {
    TRIAL_SLOT(0)
    const int gid = blockIdx.x * kBlock + threadIdx.x;
    const int b = gid / 42, e = gid % 42;
    if (b >= d.nblk) return;
    const int i1 = d.blk_i1[b];
    if (e >= 36 && i1 != d.blk_i2[b]) return;
    double sacc = 0.0;
    for (int c = d.blk_ch[b]; c < d.blk_ch[b + 1]; ++c) sacc += d.ch_part[(size_t)c * 42 + e];
    // this rank's partial Hpp into its diagonal blocks (the sum is S − Hpp: rcs_finalize_entry)
    if (e < 36 && i1 == d.blk_i2[b]) sacc -= d.Hpp_w[(size_t)i1 * 36 + e];
    const int64_t x = e < 36 ? (int64_t)b * 36 + e : (int64_t)d.nblk * 36 + 6 * i1 + (e - 36);
    if (d.xg_P > 0) {  // packed into this rank's all-gather record (outside its runs: zero by construction)
        const int64_t *rg = d.xg_rng + 4 * (size_t)d.rank;
        int64_t o;
        if (x >= rg[0] && x < rg[0] + rg[1]) o = x - rg[0];
        else if (x >= rg[2] && x < rg[2] + rg[3]) o = rg[1] + (x - rg[2]);
        else return;
        d.xg_send[(d.xg_host ? (size_t)d.rank * d.xg_P : 0) + o] = sacc;
    } else {
        d.red_rcs_loc[x] = sacc;
    }
}

// sharded pass 2b (all-gather exchange): the full red_rcs as the sum, in rank order, of every
// rank's runs — the same additions on every rank, so every rank factorises the same matrix
__global__ __launch_bounds__(kBlock) void k_rcs_xunpack(Dev d0) {
    TRIAL_SLOT(0)
    const int64_t x = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (x >= (int64_t)d.nblk * 36 + (int64_t)d.nf * 6) return;
    double s = 0.0;
    for (int r = 0; r < d.nranks; ++r) {
        const int64_t *rg = d.xg_rng + 4 * (size_t)r;
        const double *rv = d.xg_recv + (size_t)r * d.xg_P;
        if (x >= rg[0] && x < rg[0] + rg[1]) s += rv[x - rg[0]];
        else if (x >= rg[2] && x < rg[2] + rg[3]) s += rv[rg[1] + (x - rg[2])];
    }
    d.red_rcs[x] = s;
}

// pass 2: per block entry, sum its chunks in order, add Hpp + λI (diagonal), write the band /
// dense matrix and b_s = b_p - Σ A_eᵀ q_e.
__global__ __launch_bounds__(kBlock) void k_rcs_finalize(Dev d0) {
    TRIAL_SLOT(0)
    const int gid = blockIdx.x * kBlock + threadIdx.x;
    const int b = gid / 42, e = gid % 42;
    if (b >= d.nblk) return;
    const int i1 = d.blk_i1[b];
    if (e >= 36 && i1 != d.blk_i2[b]) return;
    double sacc = 0.0;
    if (d.sharded) sacc = e < 36 ? d.red_rcs[(size_t)b * 36 + e] : d.red_rcs[(size_t)d.nblk * 36 + 6 * i1 + (e - 36)];
    else
        for (int c = d.blk_ch[b]; c < d.blk_ch[b + 1]; ++c) sacc += d.ch_part[(size_t)c * 42 + e];
    rcs_finalize_entry(d, b, e, sacc);
}

// oplus of every free pose with x_p (trial state; fixed poses copied), and the pose part of
// Σx(λx+b), reduced over the NT threads of one workgroup into part_ps[0] (other slots zeroed).
// `d` is a slot view; `failed`: the solve failed, x_p is the last successful solve's (A13).
template <int NT>
__device__ __forceinline__ void pose_update_wg(const Dev &d, bool failed) {
    __shared__ double sh_pu[NT / 64];
    double sc = 0.0;
    const double lam = d.lam;
    const int hlm = d.ctrl->hlm;
    const double *Tc0 = d.Tc, *xp = failed ? d.xp_prev : d.xp;
    double *Tt0 = d.Tt;
    for (int k = threadIdx.x; k < d.n_kf; k += NT) {
        const double *Tc = Tc0 + (size_t)k * 12;
        double *Tt = Tt0 + (size_t)k * 12;
        const int h = d.kf_hidx[k];
        // a free pose with no active edge has a zero RCS row: x = 0 exactly and the oplus is an
        // exact identity, so every free pose is updated
        if (h >= 0 && hlm != kLmG2o) {  // X_i <- log(exp(X_i)·exp(DX_i)⁻¹); sc = ‖DX‖² part
            double x[6], xn[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                x[i] = xp[6 * h + i];
                sc += x[i] * x[i];
            }
            hlm_pose_update(d.xkc + (size_t)k * 6, x, xn, Tt);
#pragma unroll
            for (int i = 0; i < 6; ++i) d.xkt[(size_t)k * 6 + i] = xn[i];
        } else if (h >= 0) {
            double x[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                x[i] = xp[6 * h + i];
                sc += x[i] * (lam * x[i] + d.bp[(size_t)h * 6 + i]);
            }
            pose_oplus(Tc, x, Tt);
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) Tt[i] = Tc[i];
            if (hlm != kLmG2o)
#pragma unroll
                for (int i = 0; i < 6; ++i) d.xkt[(size_t)k * 6 + i] = d.xkc[(size_t)k * 6 + i];
        }
    }
    const double s = block_sum<NT>(sc, sh_pu);
    for (int i = threadIdx.x; i < d.n_ps; i += NT) d.part_ps[i] = i == 0 ? s : 0.0;
}

}  // namespace plba
