// TEST PROGRAM: the staged-block builder and the tile envelope (csrc/plba_layout.hpp), and the problem
// table and the plans of the association calls (csrc/plba_assoc_plan.hpp), on the host alone, on plain
// heap memory, built with the address and undefined-behaviour sanitizers. Prints "layout_check ok" and
// exits 0, or names the first check that failed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/plba.h"
#include "plba_assoc_plan.hpp"
#include "plba_layout.hpp"

using plba::ProblemTable;
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

// the fields that a plan's stage() bound into `base` lie at the offsets ref, one by one
template <size_t N>
static void check_bound(const std::vector<char> &base, const void *const (&field)[N], const size_t (&ref)[N]) {
    for (size_t i = 0; i < N; ++i) CHECK((size_t)((const char *)field[i] - base.data()) == ref[i]);
}

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

// One shape of each entry point's case file (tests/*_cases.py) against the sequence of offsets the
// entry point computed before the builder. The stereo and the keyframe association and the median
// descriptor run the entry point's own plan (csrc/plba_assoc_plan.hpp); the others, whose declarations
// are in csrc/plba_assoc.hip, are declared here as the entry point declares them.
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
        const int32_t pt_l[] = {0, 50}, pt_r[] = {0, 45}, ls_l[] = {0, 20}, ls_r[] = {0, 22};
        plba::StereoPlan Q;
        CHECK(Q.T.init(pt_l, pt_r, ls_l, ls_r, 1, 64, 48) == ProblemTable::kOk);
        CHECK(Q.T.N1 == N1 && Q.T.N2 == N2 && Q.T.nc == nc && Q.T.cnt[0][0] == npl && Q.T.cnt[1][0] == nll);
        Q.declare(db / 4);
        std::vector<char> dev(Q.B.total());
        Q.B.stage(nullptr, dev.data());
        const plba::StDev &S = Q.S;
        const plba::GmDev &D = Q.D;
        check_bound(dev, {S.off1, S.off2, S.kind, S.kbase, S.cbase, D.ws, D.nnr, D.sim_th, S.desc1, D.desc2, S.co1, S.co2}, ref);
        check_bound(dev, {S.count, S.src, S.odesc, S.ptd, S.lsd}, ref_out);
        check_bound(dev, {D.best, D.second}, ref_keys);
        check_bound(dev, {D.m12, D.m21, D.count, S.cell1, S.cell1e, S.cell_off2, S.cells2, S.dir2}, ref_dev);
        CHECK(Q.key_bytes == keys_end - ref_keys[0]);
        CHECK(Q.B.inputs_end() == inputs_end && Q.B.outputs_end() == outputs_end && Q.B.total() == L.total);
    }
    // keyframe association, kfassoc_cases "empty_side" (30 x 0 points, 0 x 12 lines) and "mixed" (50 x 45 points,
    // 20 x 22 lines): one pair, a 64 x 48 grid
    for (const bool mixed : {false, true}) {
        const int32_t pt_p[] = {0, mixed ? 50 : 30}, pt_c[] = {0, mixed ? 45 : 0}, ls_p[] = {0, mixed ? 20 : 0},
                      ls_c[] = {0, mixed ? 22 : 12};
        const size_t P = 2, db = 32, c00 = pt_p[1], c01 = pt_c[1], c10 = ls_p[1], c11 = ls_c[1], N1 = c00 + c10, N2 = c01 + c11,
                     nc = c01 + c11 * 64;
        Ref L;
        const size_t ref[] = {L.add<int32_t>(P + 1), L.add<int32_t>(P + 1), L.add<int32_t>(P), L.add<int32_t>(P),
                              L.add<int32_t>(P), L.add<int32_t>(P + 1), L.add<int32_t>(P), L.add<int32_t>(4 * P),
                              L.add<double>(P), L.add<double>(P), L.add<float>(P), L.add<double>(76 * P / 2), L.add(db * N1),
                              L.add(db * N2), L.add<double>(3 * c00), L.add<double>(22 * c10), L.add(c10), L.add<double>(5 * c01),
                              L.add<double>(4 * c11)};
        const size_t inputs_end = L.total;
        const size_t ref_out[] = {L.add<int32_t>(3 * P), L.add<int32_t>(N1), L.add<double>(9 * c00), L.add<double>(8 * c10),
                                  L.add(c10)};
        const size_t outputs_end = L.total;
        const size_t ref_keys[] = {L.add<uint32_t>(N1), L.add<uint32_t>(N1)};
        const size_t keys_end = L.total;
        const size_t ref_dev[] = {L.add<int32_t>(N1), L.add<int32_t>(N2), L.add<int32_t>(P), L.add<int32_t>(2 * N1),
                                  L.add<int32_t>(2 * N1), L.add<int32_t>(N2 + 1), L.add<int32_t>(2 * nc), L.add<double>(2 * N2),
                                  L.add<int32_t>(N1), L.add<int32_t>(N2), L.add<int32_t>(N1), L.add<int32_t>(P)};
        plba::KfPlan Q;
        CHECK(Q.T.init(pt_p, pt_c, ls_p, ls_c, 1, 64, 48) == ProblemTable::kOk);
        Q.declare(db / 4);
        std::vector<char> dev(Q.B.total());
        Q.B.stage(nullptr, dev.data());
        const plba::KfDev &K = Q.K;
        const plba::GmDev &D = Q.D;
        const plba::DmDev &M = Q.M;
        check_bound(dev, {K.off1, K.off2, K.kind, K.kbase1, K.kbase2, K.cbase, K.gate_min, D.ws, D.nnr, D.sim_th, M.nnr, K.pose,
                          D.desc1, D.desc2, K.q_pt, K.q_ls, K.ls_new, K.t_pt, K.t_ls}, ref);
        check_bound(dev, {K.res, K.m12, K.ptd, K.lsd, K.rej}, ref_out);
        check_bound(dev, {D.best, D.second}, ref_keys);
        check_bound(dev, {D.m12, D.m21, D.count, K.cell1, K.cell1e, K.cell_off2, K.cells2, K.dir2, M.nn12, M.nn21, M.m12, M.count},
                    ref_dev);
        CHECK(Q.key_bytes == keys_end - ref_keys[0]);
        CHECK(Q.B.inputs_end() == inputs_end && Q.B.outputs_end() == outputs_end && Q.B.total() == L.total);
    }
    {  // median descriptor, medoid_cases wave_lists: lists of 63, 64 and 65 descriptors of 32 bytes
        const size_t n = 3, total = 192, db = 32;
        Ref L;
        const size_t ref[] = {L.add<int32_t>(n + 1), L.add<int32_t>(n), L.add(db * total)};
        const size_t inputs_end = L.total;
        const size_t ref_out[] = {L.add<int32_t>(n)};
        plba::MedDev D{};
        Staged B;
        plba::medoid_plan(B, D, n, total, db / 4, nullptr, nullptr, nullptr);
        std::vector<char> dev(B.total());
        B.stage(nullptr, dev.data());
        check_bound(dev, {D.list_ptr, D.order, D.desc}, ref);
        check_bound(dev, {D.medoid}, ref_out);
        CHECK(B.inputs_end() == inputs_end && B.outputs_end() == L.total && B.total() == L.total);
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

// what ProblemTable::fill writes for a table, into arrays of exactly the sizes the plans declare (the
// sanitizer sees a write past one), the descriptor rows of db bytes gathered from descs
struct Filled {
    std::vector<int32_t> off1, off2, kind, kbase1, kbase2, cbase;
    std::vector<uint8_t> desc1, desc2;
    Filled(const ProblemTable &T, const uint8_t *const descs[2][2], size_t db)
        : off1(2 * T.n + 1, -7), off2(off1), kind(2 * T.n, -7), kbase1(kind), kbase2(kind), cbase(off1),
          desc1(db * T.N1), desc2(db * T.N2) {
        T.fill(off1.data(), off2.data(), kind.data(), kbase1.data(), kbase2.data(), cbase.data(), descs, db, desc1.data(),
               desc2.data());
    }
};
using I32 = std::vector<int32_t>;

static void check_problem_table() {
    const uint8_t *const none[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    ProblemTable T;
    {  // one unit without a row
        const int32_t z[] = {0, 0};
        CHECK(T.init(z, z, z, z, 1, 64, 48) == ProblemTable::kOk);
        CHECK(T.N1 == 0 && T.N2 == 0 && T.nc == 0 && T.max_rows == 0 && T.max_prev == 0 && T.max_train == 0);
        const Filled F(T, none, 32);
        CHECK(F.off1 == (I32{0, 0, 0}) && F.off2 == F.off1 && F.cbase == F.off1);
        CHECK(F.kind == (I32{0, 1}) && F.kbase1 == (I32{0, 0}) && F.kbase2 == F.kbase1);
    }
    {  // points only, then lines only: 3 x 2 rows of one byte
        const int32_t z[] = {0, 0}, a[] = {0, 3}, b[] = {0, 2};
        const uint8_t d1[] = {9, 8, 7}, d2[] = {6, 5};
        const uint8_t *const descs[2][2] = {{d1, d2}, {d1, d2}};
        CHECK(T.init(a, b, z, z, 1, 64, 48) == ProblemTable::kOk);
        CHECK(T.N1 == 3 && T.N2 == 2 && T.nc == 2 && T.cnt[0][0] == 3 && T.cnt[1][1] == 0 && T.max_rows == 3);
        const Filled Fp(T, descs, 1);
        CHECK(Fp.off1 == (I32{0, 3, 3}) && Fp.off2 == (I32{0, 2, 2}) && Fp.cbase == (I32{0, 2, 2}));
        CHECK(Fp.desc1 == (std::vector<uint8_t>{9, 8, 7}) && Fp.desc2 == (std::vector<uint8_t>{6, 5}));
        CHECK(T.init(z, z, a, b, 1, 64, 48) == ProblemTable::kOk);
        CHECK(T.N1 == 3 && T.N2 == 2 && T.nc == 2 * 64 && T.cnt[0][0] == 0 && T.cnt[1][1] == 2 && T.max_train == 2);
        const Filled Fl(T, descs, 1);
        CHECK(Fl.off1 == (I32{0, 0, 3}) && Fl.off2 == (I32{0, 0, 2}) && Fl.cbase == (I32{0, 0, 128}));
        CHECK(Fl.desc1 == Fp.desc1 && Fl.desc2 == Fp.desc2);
    }
    // Two units whose first offsets are not zero, with a problem without side-1 rows (the lines of unit 0) and one
    // without side-2 rows (the points of unit 1) between others; descriptor rows of 4 bytes, row r of an array
    // tagged (array, r), each array exactly as long as its last offset. cols < rows, then cols > rows.
    for (const int cols : {3, 7}) {
        const int rows = 5, stride = cols > rows ? cols : rows;
        const int32_t pt1[] = {5, 7, 10}, pt2[] = {2, 3, 3}, ls1[] = {1, 1, 4}, ls2[] = {4, 6, 7};
        CHECK(T.init(pt1, pt2, ls1, ls2, 2, cols, rows) == ProblemTable::kOk);
        CHECK(T.stride == stride && T.cnt[0][0] == 5 && T.cnt[0][1] == 1 && T.cnt[1][0] == 3 && T.cnt[1][1] == 3);
        CHECK(T.N1 == 8 && T.N2 == 4 && T.nc == 1 + 3 * (size_t)stride);
        CHECK(T.max_prev == 3 && T.max_train == 2 && T.max_rows == 3);
        const ProblemTable::Problem q = T.at(3);
        CHECK(q.f == 1 && q.kind == 1 && q.a1 == 1 && q.r1 == 3 && q.a2 == 6 && q.r2 == 1);
        std::vector<uint8_t> src[2][2];
        const int last[2][2] = {{10, 3}, {4, 7}};
        for (int kd = 0; kd < 2; ++kd)
            for (int sd = 0; sd < 2; ++sd)
                for (int r = 0; r < last[kd][sd]; ++r)
                    for (int e = 0; e < 4; ++e) src[kd][sd].push_back((uint8_t)(64 * (2 * kd + sd) + 4 * r + e));
        const uint8_t *const descs[2][2] = {{src[0][0].data(), src[0][1].data()}, {src[1][0].data(), src[1][1].data()}};
        const Filled F(T, descs, 4);
        CHECK(F.off1 == (I32{0, 2, 2, 5, 8}) && F.off2 == (I32{0, 1, 3, 3, 4}));
        CHECK(F.cbase == (I32{0, 1, 1 + 2 * stride, 1 + 2 * stride, 1 + 3 * stride}));
        CHECK(F.kind == (I32{0, 1, 0, 1}) && F.kbase1 == (I32{0, 0, 2, 0}) && F.kbase2 == (I32{0, 0, 1, 2}));
        // side 1: point rows 5, 6 | - | point rows 7, 8, 9 | line rows 1, 2, 3; side 2: point row 2 | line rows 4, 5 | - | line row 6
        const int want1[8][2] = {{0, 5}, {0, 6}, {0, 7}, {0, 8}, {0, 9}, {1, 1}, {1, 2}, {1, 3}};
        const int want2[4][2] = {{0, 2}, {1, 4}, {1, 5}, {1, 6}};
        for (int i = 0; i < 8; ++i)
            for (int e = 0; e < 4; ++e) CHECK(F.desc1[4 * i + e] == src[want1[i][0]][0][4 * want1[i][1] + e]);
        for (int i = 0; i < 4; ++i)
            for (int e = 0; e < 4; ++e) CHECK(F.desc2[4 * i + e] == src[want2[i][0]][1][4 * want2[i][1] + e]);
    }
    {  // a side-2 span of kGmMaxTrain is accepted, one more is refused: offsets only
        const int32_t z[] = {0, 0, 0}, at[] = {3, 3, 3 + plba::kGmMaxTrain}, over[] = {3, 3, 4 + plba::kGmMaxTrain};
        CHECK(T.init(z, at, z, z, 2, 64, 48) == ProblemTable::kOk && T.max_train == plba::kGmMaxTrain);
        CHECK(T.init(z, z, z, over, 2, 64, 48) == ProblemTable::kTooWide && T.max_train == plba::kGmMaxTrain + 1);
        CHECK(T.init(over, z, over, z, 2, 64, 48) == ProblemTable::kOk && T.max_prev == plba::kGmMaxTrain + 1);  // side 1 may
    }
    {  // lines whose cells pass INT32_MAX are refused, every problem within kGmMaxTrain; the sum is a size_t
        const int n = 513;  // 513 * 65535 * 64 = 2151645120
        I32 z(n + 1, 0), ls2(n + 1);
        for (int f = 0; f <= n; ++f) ls2[f] = f * plba::kGmMaxTrain;
        CHECK(T.init(z.data(), z.data(), z.data(), ls2.data(), n, 64, 48) == ProblemTable::kTooMany);
        CHECK(T.nc == (size_t)513 * 65535 * 64 && T.N2 == (size_t)513 * 65535 && T.max_train == plba::kGmMaxTrain);
        CHECK(T.init(z.data(), z.data(), z.data(), ls2.data(), n - 1, 64, 48) == ProblemTable::kOk);  // 2147450880
        // the widest grid: one line owns INT32_MAX cells, two lines are too many
        const int32_t one[] = {0, 1}, two[] = {0, 2};
        CHECK(T.init(one, one, one, one, 1, INT32_MAX, 1) == ProblemTable::kTooMany && T.nc == (size_t)INT32_MAX + 1);
        CHECK(T.init(z.data(), z.data(), one, one, 1, 1, INT32_MAX) == ProblemTable::kOk && T.nc == (size_t)INT32_MAX);
        CHECK(T.init(z.data(), z.data(), two, two, 1, 1, INT32_MAX) == ProblemTable::kTooMany);
    }
}

int main() {
    check_builder();
    check_entry_point_offsets();
    check_problem_table();
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
