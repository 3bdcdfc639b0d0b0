// TEST PROGRAM: the block layout builder and the tile envelope (csrc/plba_layout.hpp) on the host
// alone, built with the address and undefined-behaviour sanitizers. Prints "layout_check ok" and
// exits 0, or names the first check that failed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plba_layout.hpp"

using plba::Layout;
using plba::TileEnvelope;
using plba::tile_envelope;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

// tile_first / tile_last from the dense pattern: entry (r, c) of the lower triangle is inside the
// envelope when c >= 6 * first[r / 6]
static TileEnvelope brute_force(const std::vector<int32_t> &first, int n, int tile) {
    const int nt = (n + tile - 1) / tile;
    std::vector<char> dense((size_t)n * n, 0);
    for (int r = 0; r < n; ++r)
        for (int c = 6 * first[r / 6]; c <= r; ++c) dense[(size_t)r * n + c] = 1;
    TileEnvelope te;
    te.tile_first.assign(nt > 0 ? nt : 1, 0);
    te.tile_last.assign(nt > 0 ? nt : 1, 0);
    for (int I = 0; I < nt; ++I) {
        int f = I;
        for (int r = I * tile; r < n && r < (I + 1) * tile; ++r)
            for (int c = 0; c <= r; ++c)
                if (dense[(size_t)r * n + c] && c / tile < f) f = c / tile;
        te.tile_first[I] = f;
    }
    for (int K = 0; K < nt; ++K) {
        int last = K;
        for (int r = 0; r < n; ++r)
            for (int c = K * tile; c < n && c < (K + 1) * tile && c <= r; ++c)
                if (dense[(size_t)r * n + c] && r / tile > last) last = r / tile;
        te.tile_last[K] = last;
    }
    return te;
}

int main() {
    {  // every array takes max(bytes, 128) rounded up to 256
        Layout L;
        CHECK(L.add(0) == 0);
        CHECK(L.add(1) == 256);
        const size_t inputs_end = L.mark();
        CHECK(L.add(128) == 512);
        const size_t outputs_end = L.mark();
        CHECK(L.add(257) == 768);
        CHECK(L.total == 1280 && L.mark() == 1280);
        CHECK(inputs_end == 512 && outputs_end == 768);  // upload [0, 512), read back [512, 768)
        Layout T;
        CHECK(T.add<double>(0) == 0 && T.add<int32_t>(65) == 256 && T.total == 768);
        alignas(8) char block[1280] = {0};
        *plba::at<int32_t>(block, 512) = 7;
        CHECK(block[512] == 7 && plba::at<const double>(block, 768) == (const double *)(block + 768));
    }
    const int tile = 16;
    {  // no free pose: one zeroed tile
        const TileEnvelope te = tile_envelope({}, 0, tile);
        CHECK(te.tile_first == std::vector<int32_t>{0} && te.tile_last == std::vector<int32_t>{0});
    }
    const int nf = 7, n = 6 * nf, nt = (n + tile - 1) / tile;  // 42 rows: 3 tiles, the last one partial
    CHECK(nt == 3);
    {  // block diagonal: a 6-row block that straddles a tile boundary couples the two tiles
        std::vector<int32_t> first(nf);
        for (int h = 0; h < nf; ++h) first[h] = h;
        const TileEnvelope te = tile_envelope(first, n, tile), bf = brute_force(first, n, tile);
        CHECK(te.tile_first == bf.tile_first && te.tile_last == bf.tile_last);
        // rows 12..17 straddle tiles 0 | 1, rows 30..35 tiles 1 | 2
        CHECK((te.tile_first == std::vector<int32_t>{0, 0, 1}) && (te.tile_last == std::vector<int32_t>{1, 2, 2}));
    }
    {  // arrow: the last pose is coupled to pose 0
        std::vector<int32_t> first(nf);
        for (int h = 0; h < nf; ++h) first[h] = h;
        first[nf - 1] = 0;
        const TileEnvelope te = tile_envelope(first, n, tile), bf = brute_force(first, n, tile);
        CHECK(te.tile_first == bf.tile_first && te.tile_last == bf.tile_last);
        CHECK(te.tile_first[nt - 1] == 0 && te.tile_last[0] == nt - 1);
    }
    {  // a multiple of the tile where no block straddles: 8 poses = 48 rows, tile 24
        std::vector<int32_t> first(8);
        for (int h = 0; h < 8; ++h) first[h] = h;
        const TileEnvelope te = tile_envelope(first, 48, 24);
        CHECK((te.tile_last == std::vector<int32_t>{0, 1}) && (te.tile_first == std::vector<int32_t>{0, 1}));
    }
    std::puts("layout_check ok");
    return 0;
}
