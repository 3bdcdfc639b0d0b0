// plba_layout.hpp — host-only layout arithmetic shared by the entry points: the carving of one
// block into arrays (Staged) and the tile envelope of a block-banded lower triangle
// (tile_envelope). Standard C++ only: no HIP types, no kernel headers, so a host compiler can
// build it on its own (tests/cpp/layout_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace plba {

// One block of device memory with an optional pinned host image, declared array by array. Each
// array is named once, by the kernel-struct field that will point to it:
//     B.in(D.off1, n + 1, b->off1);      uploaded; the source is copied into the host image by stage()
//     B.in(D.ws, 4 * n);                 uploaded; the caller fills host(D.ws) itself
//     B.out(D.m12, n1, matches_12);      read back; fetch() copies n1 elements to matches_12
//     B.dev(D.best, n1);                 device only
// in that order of roles, which is the order in the block: the entry point uploads
// [0, inputs_end()) and reads back [inputs_end(), outputs_end()). Every declaration returns the
// array's offset, and mark() the offset the next one will get, for a range of the block that is
// filled as one. Every array takes max(bytes, 128) rounded up to 256: kernels issue unconditional
// loads of one record for dead lanes, which must stay inside the array (see plba_ctx::alloc), so
// an empty array still owns 256 bytes. An absent source or destination, or an empty array, copies
// nothing. The builder issues no device call and allocates nothing.
class Staged {
public:
    template <typename T, typename S = T>
    size_t in(T *&field, size_t count, const S *src = nullptr) {
        static_assert(sizeof(S) == sizeof(T) || sizeof(S) == 1, "the source holds the field's elements, or bytes");
        return add(0, field, count, src, nullptr);
    }
    template <typename T, typename S = T>
    size_t out(T *&field, size_t count, S *dst = nullptr) {
        static_assert(sizeof(S) == sizeof(T) || sizeof(S) == 1, "the destination holds the field's elements, or bytes");
        return add(1, field, count, nullptr, dst);
    }
    template <typename T>
    size_t dev(T *&field, size_t count) { return add(2, field, count, nullptr, nullptr); }

    size_t mark() const { return end_[2]; }
    size_t inputs_end() const { return end_[0]; }
    size_t outputs_end() const { return end_[1]; }
    size_t total() const { return end_[2]; }

    // once the block is reserved: the sources into the host image, base + offset into every field
    // (host may be null for a block without an image: there is nothing to copy then)
    void stage(char *host, char *device) {
        host_ = host;
        for (int i = 0; i < n_; ++i) {
            const Array &a = arr_[i];
            if (host && a.src && a.bytes) memcpy(host + a.off, a.src, a.bytes);
            a.bind(a.field, device + a.off);
        }
    }
    // after the read-back: the outputs to their destinations
    void fetch() const {
        for (int i = 0; i < n_; ++i)
            if (arr_[i].dst && arr_[i].bytes) memcpy(arr_[i].dst, host_ + arr_[i].off, arr_[i].bytes);
    }
    // the array of `field` in the host image
    template <typename T>
    typename std::remove_const<T>::type *host(T *const &field) const {
        for (int i = 0; i < n_; ++i)
            if (arr_[i].field == (const void *)&field)
                return reinterpret_cast<typename std::remove_const<T>::type *>(host_ + arr_[i].off);
        abort();  // not declared here
    }

private:
    struct Array {
        void *field;
        void (*bind)(void *field, char *p);
        size_t off, bytes;
        const void *src;
        void *dst;
    };
    // The most arrays of one call. track_frames declares 49, the most today: raise this with the
    // entry point that needs more. One too many, a role out of order or a host() of an undeclared field
    // is a mistake in the entry point's own text, so it aborts at that entry point's first call.
    static constexpr int kMax = 56;
    Array arr_[kMax];
    int n_ = 0, role_ = 0;
    size_t end_[3] = {0, 0, 0};  // of the inputs, the outputs, everything
    char *host_ = nullptr;

    template <typename T>
    size_t add(int role, T *&field, size_t count, const void *src, void *dst) {
        if (n_ == kMax || role < role_) abort();  // inputs, then outputs, then device only
        role_ = role;
        const size_t off = end_[2], bytes = sizeof(T) * count;
        arr_[n_++] = Array{(void *)&field, [](void *f, char *p) { *static_cast<T **>(f) = reinterpret_cast<T *>(p); },
                           off, bytes, src, dst};
        for (int r = role; r < 3; ++r) end_[r] = off + ((std::max(bytes, (size_t)128) + 255) & ~(size_t)255);
        return off;
    }
};

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
