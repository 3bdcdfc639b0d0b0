// plba_layout.hpp — host-only layout arithmetic shared by the entry points: the carving of one
// block into arrays (Layout, at) and the tile envelope of a block-banded lower triangle
// (tile_envelope). Standard C++ only: no HIP types, no kernel headers, so a host compiler can
// build it on its own (tests/cpp/layout_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace plba {

// Hands out offsets into one block in call order. Every array takes max(bytes, 128) rounded up to
// 256: kernels issue unconditional loads of one record for dead lanes, which must stay inside the
// array (see plba_ctx::alloc), so an empty array still owns 256 bytes. mark() is the offset the
// next array will get, i.e. the extent of everything added so far: an entry point adds its inputs,
// takes a mark, adds its outputs, takes a mark, adds its scratch, and then uploads [0, inputs_end)
// and reads back [inputs_end, outputs_end).
struct Layout {
    size_t total = 0;
    size_t add(size_t bytes) {
        const size_t off = total;
        total += (std::max(bytes, (size_t)128) + 255) & ~(size_t)255;
        return off;
    }
    template <typename T>
    size_t add(size_t count) { return add(sizeof(T) * count); }
    size_t mark() const { return total; }
};

// the array at `off` of the block at `base`, typed
template <typename T>
inline T *at(char *base, size_t off) { return reinterpret_cast<T *>(base + off); }

// Envelope of the lower triangle of an n x n matrix (n = 6 * poses) in tiles of `tile` rows:
// first[h] is the first pose-block column of pose-block row h. tile_first[I] is the first column
// tile any row of row tile I reaches, tile_last[K] the last row tile whose envelope reaches
// column tile K. Both have max(ntiles, 1) entries (n = 0: one zeroed tile).
struct TileEnvelope {
    std::vector<int32_t> tile_first, tile_last;
};
inline TileEnvelope tile_envelope(const std::vector<int32_t> &first, int n, int tile) {
    const int ntiles = (n + tile - 1) / tile;
    TileEnvelope te;
    te.tile_first.assign(std::max(ntiles, 1), 0);
    te.tile_last.assign(std::max(ntiles, 1), 0);
    for (int I = 0; I < ntiles; ++I) {
        int f = I;
        for (int r = I * tile; r < std::min(n, (I + 1) * tile); ++r) f = std::min(f, (6 * first[r / 6]) / tile);
        te.tile_first[I] = f;
    }
    for (int K = 0; K < ntiles; ++K) {
        int last = K;
        for (int I = K; I < ntiles; ++I)
            if (te.tile_first[I] <= K) last = I;
        te.tile_last[K] = last;
    }
    return te;
}

}  // namespace plba
