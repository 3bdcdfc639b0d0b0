// plba_scratch.hpp — what every entry point needs from a context, and nothing of the solver: the
// options, the error string, the stream and the grow-only scratch blocks (CtxBase), the error
// macros, and the entry points that live outside the solver's translation unit (plba_assoc.hip).
// No kernel header is included here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/plba.h"
#include "plba_layout.hpp"

namespace plba {

struct CtxBase;

// A grow-only device allocation on the context's stream with an optional pinned host image, kept
// across calls. A block that is too small is freed and allocated again at exactly the size asked
// for; the contents do not survive that.
struct ScratchBlock {
    char *dev = nullptr, *host = nullptr;
    size_t dev_cap = 0, host_cap = 0;
    // PLBA_OK, or PLBA_E_NOMEM with "<what>: cannot allocate N bytes[ of pinned memory]"
    inline int reserve(CtxBase &ctx, size_t dev_bytes, size_t host_bytes, const char *what);
    // the device part, stream-ordered; the pinned part only after that stream was synchronised
    void release(hipStream_t stream) {
        if (dev) (void)hipFreeAsync(dev, stream);
        dev = nullptr;
        dev_cap = 0;
    }
    void release_host() {
        if (host) (void)hipHostFree(host);
        host = nullptr;
        host_cap = 0;
    }
};

// One place-recognition slot (plba_bow_*; 0 points, 1 lines): the resident vocabulary and the
// database of BoW vectors as CSR rows. The rows' bookkeeping stays on the host.
struct BowSlot {
    ScratchBlock voc;              // child_off, children, node_desc, word_id, word_weight
    ScratchBlock db_word, db_val;  // int32 word ids and double values of every row, appended
    int32_t *child_off = nullptr, *children = nullptr, *word_id = nullptr;  // the arrays of voc (BowDev's names)
    uint32_t *node_desc = nullptr;
    double *word_weight = nullptr;
    int n_nodes = 0, n_words = 0, dwords = 0, depth = 0, max_children = 0;  // n_nodes == 0: no vocabulary
    struct Row {
        int32_t kf_id, off, len;
        bool live;
    };
    std::vector<Row> rows;         // in increasing kf_id; a removed row keeps its id and its space
    size_t used = 0;               // elements of db_word / db_val in use
};

struct CtxBase {
    plba_opts opts;
    std::string err;
    hipStream_t stream = nullptr;
    // Blocks independent of the window arena (these calls leave an uploaded window intact):
    ScratchBlock pgo;    // pose graph (plba_pgo_optimize); host image: the four doubles read back per trial
    ScratchBlock lc;     // relative pose (plba_lc_relative_pose): inputs up, results and inlier flags down
    ScratchBlock track;  // frame-to-frame pose (plba_track_pose): the same, and the residual lists
    ScratchBlock match;  // descriptor matching, grid-guided matching and stereo association share one
    BowSlot bow[2];      // place recognition: the vocabulary and the database of each slot
    ScratchBlock bow_io; // descriptors and the live rows up, scores down, the sort's scratch

    void set_error(const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        if (opts.verbose) fprintf(stderr, "[plba] %s\n", buf);
    }
};

inline int ScratchBlock::reserve(CtxBase &ctx, size_t dev_bytes, size_t host_bytes, const char *what) {
    if (dev_bytes > dev_cap) {
        // stream-ordered: hipFree / hipMalloc would synchronise the whole device (see commit_plan)
        release(ctx.stream);
        if (hipMallocAsync((void **)&dev, dev_bytes, ctx.stream) != hipSuccess) {
            (void)hipGetLastError();
            dev = nullptr;
            ctx.set_error("%s: cannot allocate %zu bytes", what, dev_bytes);
            return PLBA_E_NOMEM;
        }
        dev_cap = dev_bytes;
    }
    if (host_bytes > host_cap) {
        release_host();
        if (hipHostMalloc((void **)&host, host_bytes) != hipSuccess) {
            (void)hipGetLastError();
            host = nullptr;
            ctx.set_error("%s: cannot allocate %zu bytes of pinned memory", what, host_bytes);
            return PLBA_E_NOMEM;
        }
        host_cap = host_bytes;
    }
    return PLBA_OK;
}

// Both macros return from the calling function and expect its context in a pointer named `ctx`.
#define PLBA_CHECK(expr)                                                                       \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            (void)hipGetLastError(); /* do not leak into the next launch check */              \
            ctx->set_error("HIP error %s at %s:%d: %s", hipGetErrorString(_e), __FILE__,       \
                           __LINE__, #expr);                                                   \
            return PLBA_E_DEVICE;                                                              \
        }                                                                                      \
    } while (0)

// every launch outside the step graphs is checked where it is issued
#define PLBA_LAUNCHED(ctx_, name_)                                                        \
    do {                                                                                  \
        const hipError_t le_ = hipGetLastError();                                         \
        if (le_ != hipSuccess) {                                                          \
            (ctx_)->set_error("kernel %s launch failed: %s", name_, hipGetErrorString(le_)); \
            return PLBA_E_DEVICE;                                                         \
        }                                                                                 \
    } while (0)

// plba_assoc.hip: the bodies of plba_lc_relative_pose, plba_desc_match, plba_grid_match and
// plba_stereo_associate,
int lc_relative_pose(CtxBase *ctx, const plba_lcpose_batch *b, const plba_lcpose_params *pp, plba_lcpose_out *out,
                     uint8_t *pt_inlier, uint8_t *ln_inlier);
int track_pose(CtxBase *ctx, const plba_track_batch *b, const plba_track_params *pp, plba_track_out *out,
               uint8_t *pt_inlier, uint8_t *ln_inlier);
int desc_match(CtxBase *ctx, const plba_match_batch *b, int32_t *matches_12, int32_t *n_matches);
int track_frames(CtxBase *ctx, const plba_frames_batch *b, const plba_frames_params *pp, const plba_frames_out *out);
int grid_match(CtxBase *ctx, const plba_gridmatch_batch *b, int32_t *matches_12, int32_t *n_matches);
int stereo_associate(CtxBase *ctx, const plba_stereo_batch *b, const plba_stereo_params *pp,
                     const plba_stereo_out *out);
int kf_associate(CtxBase *ctx, const plba_kfassoc_batch *b, const plba_kfassoc_params *pp, const plba_kfassoc_out *out);
int map_associate(CtxBase *ctx, const plba_mapassoc_batch *b, const plba_mapassoc_params *pp, const plba_mapassoc_out *out);
int desc_medoid(CtxBase *ctx, int n, const int32_t *list_ptr, const uint8_t *desc, int desc_bytes, int32_t *medoid);
// and of plba_bow_set_vocab / _insert / _remove / _get
int bow_set_vocab(CtxBase *ctx, int slot, const plba_bow_vocab *v);
int bow_insert(CtxBase *ctx, int slot, int kf_id, const uint8_t *desc, int n_desc, double *scores, int32_t *ids, int cap,
               int32_t *n);
int bow_remove(CtxBase *ctx, int slot, int kf_id);
int bow_get(CtxBase *ctx, int slot, int kf_id, int32_t *word_ids, double *values, int cap, int32_t *n);

}  // namespace plba
