// TEST PROGRAM: the staged-block builder and the tile envelope (csrc/plba_layout.hpp) on the host
// alone, on plain heap memory, built with the address and undefined-behaviour sanitizers. Prints
// "layout_check ok" and exits 0, or names the first check that failed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/plba.h"
#include "plba_layout.hpp"

using plba::Staged;
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

// The offsets before the builder: every array took max(bytes, 128) rounded up to 256, in call order.
// The entry points' former sequences are written out with it below.
struct Ref {
    size_t total = 0;
    size_t add(size_t bytes) {
        const size_t off = total;
        total += ((bytes < 128 ? 128 : bytes) + 255) / 256 * 256;
        return off;
    }
    template <typename T>
    size_t add(size_t count) { return add(sizeof(T) * count); }
};

static void check_builder() {
    // an empty input, a 1-byte input, a 128-byte output, a 257-byte device-only array in a marked range
    struct {
        const double *empty;
        const uint8_t *one;
        int32_t *out;
        uint8_t *scratch;
    } D{};
    const uint8_t one = 0x5A;
    std::vector<int32_t> dst(32, -1);  // exactly the output: the sanitizer sees a copy past it
    Staged B;
    CHECK(B.in(D.empty, 0, (const double *)nullptr) == 0);
    CHECK(B.in(D.one, 1, &one) == 256);
    CHECK(B.out(D.out, 32, dst.data()) == 512);
    const size_t from = B.mark();
    CHECK(B.dev(D.scratch, 257) == 768);
    CHECK(from == 768 && B.mark() == 1280);
    CHECK(B.inputs_end() == 512 && B.outputs_end() == 768 && B.total() == 1280);  // upload [0, 512), read back [512, 768)
    std::vector<char> host(B.outputs_end(), 0x11), device(B.total());
    B.stage(host.data(), device.data());
    CHECK((const char *)D.empty == device.data() && D.one == (const uint8_t *)device.data() + 256);
    CHECK(D.out == (int32_t *)(device.data() + 512) && D.scratch == (uint8_t *)device.data() + 768);
    // the one source byte arrived; the absent source, the padding and the outputs are untouched
    for (size_t i = 0; i < host.size(); ++i) CHECK(host[i] == (i == 256 ? 0x5A : 0x11));
    CHECK(B.host(D.one) == (uint8_t *)host.data() + 256 && B.host(D.out) == (int32_t *)(host.data() + 512));
    for (int i = 0; i < 32; ++i) B.host(D.out)[i] = 100 + i;
    B.fetch();
    for (int i = 0; i < 32; ++i) CHECK(dst[i] == 100 + i);

    // a block without a host image binds only; a source of bytes for a field of dwords; an absent destination
    struct {
        const uint32_t *desc;
        const int32_t *fill;
        double *res;
    } E{};
    const uint8_t rows[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    Staged C;
    CHECK(C.in(E.desc, 2, rows) == 0 && C.in(E.fill, 3) == 256 && C.out(E.res, 65) == 512 && C.total() == 1280);
    std::vector<char> dev2(C.total());
    C.stage(nullptr, dev2.data());
    CHECK((const char *)E.desc == dev2.data() && (char *)E.res == dev2.data() + 512);
    std::vector<char> host2(C.outputs_end(), 0x22);
    C.stage(host2.data(), dev2.data());
    for (size_t i = 0; i < host2.size(); ++i) CHECK(host2[i] == (i < 8 ? (char)rows[i] : 0x22));  // fill is the caller's
    C.fetch();  // nothing to deliver
}

// One shape of each entry point's case file (tests/*_cases.py), declared as the entry point declares
// it, against the sequence of offsets the entry point computed before the builder.
static void check_entry_point_offsets() {
    {  // relative pose, lcpose_cases (300, 100): one candidate
        const size_t n = 1, np = 300, nl = 100;
        Ref L;
        const size_t ref[] = {L.add<int32_t>(n + 1), L.add<int32_t>(n + 1), L.add<double>(3 * np), L.add<double>(2 * np),
                              L.add<double>(3 * nl), L.add<double>(3 * nl), L.add<double>(3 * nl)};
        const size_t inputs_end = L.total;
        const size_t ref_out[] = {L.add<plba_lcpose_out>(n), L.add(np), L.add(nl)};
        struct {
            const int32_t *pt_off, *ln_off;
            const double *pt_P, *pt_obs, *ln_sP, *ln_eP, *ln_le;
            plba_lcpose_out *out;
            uint8_t *pt_in, *ln_in;
        } D{};
        Staged B;
        const size_t got[] = {B.in(D.pt_off, n + 1), B.in(D.ln_off, n + 1), B.in(D.pt_P, 3 * np), B.in(D.pt_obs, 2 * np),
                              B.in(D.ln_sP, 3 * nl), B.in(D.ln_eP, 3 * nl), B.in(D.ln_le, 3 * nl)};
        const size_t got_out[] = {B.out(D.out, n), B.out(D.pt_in, np), B.out(D.ln_in, nl)};
        for (int i = 0; i < 7; ++i) CHECK(got[i] == ref[i]);
        for (int i = 0; i < 3; ++i) CHECK(got_out[i] == ref_out[i]);
        CHECK(B.inputs_end() == inputs_end && B.outputs_end() == L.total && B.total() == L.total);
    }
    {  // descriptor matching, descmatch_cases (255, 257) at 32 bytes: one pair
        const size_t n = 1, n1 = 255, n2 = 257, db = 32;
        Ref L;
        const size_t ref[] = {L.add<int32_t>(n + 1), L.add<int32_t>(n + 1), L.add<float>(n), L.add(db * n1), L.add(db * n2)};
        const size_t inputs_end = L.total;
        const size_t ref_out[] = {L.add<int32_t>(n1), L.add<int32_t>(n)};
        const size_t outputs_end = L.total;
        const size_t ref_dev[] = {L.add<int32_t>(n1), L.add<int32_t>(n2)};
        struct {
            const int32_t *off1, *off2;
            const float *nnr;
            const uint32_t *desc1, *desc2;
            int32_t *m12, *count, *nn12, *nn21;
        } D{};
        Staged B;
        const size_t got[] = {B.in(D.off1, n + 1), B.in(D.off2, n + 1), B.in(D.nnr, n), B.in(D.desc1, db / 4 * n1),
                              B.in(D.desc2, db / 4 * n2)};
        const size_t got_out[] = {B.out(D.m12, n1), B.out(D.count, n)};
        const size_t got_dev[] = {B.dev(D.nn12, n1), B.dev(D.nn21, n2)};
        for (int i = 0; i < 5; ++i) CHECK(got[i] == ref[i]);
        for (int i = 0; i < 2; ++i) CHECK(got_out[i] == ref_out[i] && got_dev[i] == ref_dev[i]);
        CHECK(B.inputs_end() == inputs_end && B.outputs_end() == outputs_end && B.total() == L.total);
    }
    {  // grid matching, gridmatch_cases (1, 257, 70, 32, ...): one line problem, 431 train cells
        const size_t n = 1, n1 = 257, n2 = 70, db = 32, nc = 431;
        Ref L;
        const size_t ref[] = {L.add<int32_t>(n + 1), L.add<int32_t>(n + 1), L.add<int32_t>(n), L.add<int32_t>(4 * n),
                              L.add<double>(n), L.add<double>(n), L.add(db * n1), L.add(db * n2), L.add<int32_t>(2 * n1),
                              L.add<int32_t>(2 * n1), L.add<int32_t>(n2 + 1), L.add<int32_t>(2 * nc), L.add<double>(2 * n2)};
        const size_t inputs_end = L.total;
        const size_t ref_out[] = {L.add<int32_t>(n1), L.add<int32_t>(n)};
        const size_t outputs_end = L.total;
        const size_t ref_keys[] = {L.add<uint32_t>(n1), L.add<uint32_t>(n1)};
        const size_t keys_end = L.total;
        const size_t ref_m21 = L.add<int32_t>(n2);
        struct {
            const int32_t *off1, *off2, *kind, *ws, *cell1, *cell1e, *cell_off2, *cells2;
            const double *nnr, *sim_th, *dir2;
            const uint32_t *desc1, *desc2;
            int32_t *m12, *count, *m21;
            uint32_t *best, *second;
        } D{};
        Staged B;
        const size_t got[] = {B.in(D.off1, n + 1), B.in(D.off2, n + 1), B.in(D.kind, n), B.in(D.ws, 4 * n), B.in(D.nnr, n),
                              B.in(D.sim_th, n), B.in(D.desc1, db / 4 * n1), B.in(D.desc2, db / 4 * n2), B.in(D.cell1, 2 * n1),
                              B.in(D.cell1e, 2 * n1), B.in(D.cell_off2, n2 + 1), B.in(D.cells2, 2 * nc), B.in(D.dir2, 2 * n2)};
        const size_t got_out[] = {B.out(D.m12, n1), B.out(D.count, n)};
        const size_t got_keys[] = {B.dev(D.best, n1), B.dev(D.second, n1)};
        const size_t got_keys_end = B.mark();
        const size_t got_m21 = B.dev(D.m21, n2);
        for (int i = 0; i < 13; ++i) CHECK(got[i] == ref[i]);
        for (int i = 0; i < 2; ++i) CHECK(got_out[i] == ref_out[i] && got_keys[i] == ref_keys[i]);
        CHECK(got_keys_end == keys_end && got_m21 == ref_m21);
        CHECK(B.inputs_end() == inputs_end && B.outputs_end() == outputs_end && B.total() == L.total);
    }
    {  // stereo association, stereo_cases "mixed": one frame of 50 x 45 points and 20 x 22 lines, a 64 x 48 grid
        const size_t P = 2, N1 = 70, N2 = 67, db = 32, npl = 50, nll = 20, nc = 45 + 22 * 64;
        Ref L;
        const size_t ref[] = {L.add<int32_t>(P + 1), L.add<int32_t>(P + 1), L.add<int32_t>(P), L.add<int32_t>(P),
                              L.add<int32_t>(P + 1), L.add<int32_t>(4 * P), L.add<double>(P), L.add<double>(P),
                              L.add(db * N1), L.add(db * N2), L.add<float>(4 * N1), L.add<float>(4 * N2)};
        const size_t inputs_end = L.total;
        const size_t ref_out[] = {L.add<int32_t>(P), L.add<int32_t>(N1), L.add(db * N1), L.add<double>(6 * npl),
                                  L.add<double>(21 * nll)};
        const size_t outputs_end = L.total;
        const size_t ref_keys[] = {L.add<uint32_t>(N1), L.add<uint32_t>(N1)};
        const size_t keys_end = L.total;
        const size_t ref_dev[] = {L.add<int32_t>(N1), L.add<int32_t>(N2), L.add<int32_t>(P), L.add<int32_t>(2 * N1),
                                  L.add<int32_t>(2 * N1), L.add<int32_t>(N2 + 1), L.add<int32_t>(2 * nc), L.add<double>(2 * N2)};
        struct {
            const int32_t *off1, *off2, *kind, *kbase, *cbase, *ws;
            const double *nnr, *sim_th;
            const uint32_t *desc1, *desc2;
            const float *co1, *co2;
            int32_t *count, *src, *m12, *m21, *gcount, *cell1, *cell1e, *cell_off2, *cells2;
            uint32_t *odesc, *best, *second;
            double *ptd, *lsd, *dir2;
        } S{};
        Staged B;
        const size_t got[] = {B.in(S.off1, P + 1), B.in(S.off2, P + 1), B.in(S.kind, P), B.in(S.kbase, P), B.in(S.cbase, P + 1),
                              B.in(S.ws, 4 * P), B.in(S.nnr, P), B.in(S.sim_th, P), B.in(S.desc1, db / 4 * N1),
                              B.in(S.desc2, db / 4 * N2), B.in(S.co1, 4 * N1), B.in(S.co2, 4 * N2)};
        const size_t got_out[] = {B.out(S.count, P), B.out(S.src, N1), B.out(S.odesc, db / 4 * N1), B.out(S.ptd, 6 * npl),
                                  B.out(S.lsd, 21 * nll)};
        const size_t got_keys[] = {B.dev(S.best, N1), B.dev(S.second, N1)};
        const size_t got_keys_end = B.mark();
        const size_t got_dev[] = {B.dev(S.m12, N1), B.dev(S.m21, N2), B.dev(S.gcount, P), B.dev(S.cell1, 2 * N1),
                                  B.dev(S.cell1e, 2 * N1), B.dev(S.cell_off2, N2 + 1), B.dev(S.cells2, 2 * nc),
                                  B.dev(S.dir2, 2 * N2)};
        for (int i = 0; i < 12; ++i) CHECK(got[i] == ref[i]);
        for (int i = 0; i < 5; ++i) CHECK(got_out[i] == ref_out[i]);
        for (int i = 0; i < 2; ++i) CHECK(got_keys[i] == ref_keys[i]);
        for (int i = 0; i < 8; ++i) CHECK(got_dev[i] == ref_dev[i]);
        CHECK(got_keys_end == keys_end);
        CHECK(B.inputs_end() == inputs_end && B.outputs_end() == outputs_end && B.total() == L.total);
    }
    {  // place recognition, bow_cases: 257 descriptors of 32 bytes against 3 live rows; then 8193, sorted out of LDS
        for (const size_t n_desc : {(size_t)257, (size_t)8193}) {
            const size_t db = 32, n_live = 3, npad = n_desc == 257 ? 512 : 16384, lds_keys = 8192;
            Ref L;
            const size_t ref[] = {L.add(db * n_desc), L.add<int32_t>(2 * n_live)};
            const size_t inputs_end = L.total;
            const size_t ref_out[] = {L.add<double>(n_live + 1), L.add<int32_t>(1)};
            const size_t outputs_end = L.total;
            const size_t ref_dev[] = {L.add<uint32_t>(n_desc), L.add<uint32_t>(npad > lds_keys ? npad : 0), L.add<int32_t>(n_desc)};
            struct {
                const uint32_t *desc;
                const int32_t *ent;
                double *scores;
                int32_t *n_new, *run_start;
                uint32_t *keys, *sortbuf;
            } D{};
            Staged B;
            const size_t got[] = {B.in(D.desc, db / 4 * n_desc), B.in(D.ent, 2 * n_live)};
            const size_t got_out[] = {B.out(D.scores, n_live + 1), B.out(D.n_new, 1)};
            const size_t got_dev[] = {B.dev(D.keys, n_desc), B.dev(D.sortbuf, npad > lds_keys ? npad : 0), B.dev(D.run_start, n_desc)};
            for (int i = 0; i < 2; ++i) CHECK(got[i] == ref[i] && got_out[i] == ref_out[i]);
            for (int i = 0; i < 3; ++i) CHECK(got_dev[i] == ref_dev[i]);
            CHECK(B.inputs_end() == inputs_end && B.outputs_end() == outputs_end && B.total() == L.total);
        }
    }
}

int main() {
    check_builder();
    check_entry_point_offsets();
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
