// draw_ring.h -- the host side of what bdf_scores (k_recommend.hip) and bdf_acquire (k_acquire.hip) share: a ring of posterior draws
// that are not in the object's planes yet, the scored rows, and planes of n_rows x M doubles with a guard behind them.  The functions
// live in k_recommend.hip beside the kernels they launch; `who` names the exported function, or the object, in the messages.
#pragma once
#include "bdf_common.h"
#include "recommend.h"

struct bdf_draw_ring {
    bdf_ctx *ctx = nullptr;        // borrowed
    int64_t n_rows = 0, M = 0;
    int D = 0, nblk = 0;           // nblk: blocks of four d, ceil(D / 4)
    int batch = 0, held = 0;       // the ring's slots, and how many hold a draw that is not in the planes yet
    double draws = 0.0;            // draws pushed
    int64_t slot = 0;              // doubles per slot: (n_rows + M) x 4 nblk of factors, then the owner's tail
    DevBuf<double> ring_dev;       // batch slots
    DevBuf<int32_t> rows_dev;      // nullable: 0-based row of U per scored row
    std::vector<int32_t> rows_host;
    int (*flush)(void *owner) = nullptr;   // folds the held draws into the owner's planes (bdf_scores_flush, bdf_acquire_flush)
    void *owner = nullptr;         // the object the ring is a member of
    // the object's destructor: waits for the work that may still read the ring and the planes (a ring whose checks failed has no context)
    void drain() const { if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); } }
};

inline double *bdf_ring_slot(const bdf_draw_ring *r) { return r->ring_dev + (int64_t)r->held * r->slot; }      // where the next draw goes
// create: the argument checks (after the NULL check) and the fields; a plane filled with the byte `fill`, then
// BDF_REC_GUARD doubles of NaN that nothing writes; the ring's slots and the scored rows (checked on the host), then a wait for ctx's stream
int bdf_ring_init(bdf_draw_ring *r, const char *who, bdf_ctx *ctx, int64_t n_rows, int64_t M, int D, int batch, int tail, int (*flush)(void *), void *owner);
int bdf_ring_plane(const bdf_draw_ring *r, const char *who, const char *what, int fill, DevBuf<double> &plane);
int bdf_ring_alloc(bdf_draw_ring *r, const char *who, const int32_t *rows_dev);
// k_scores_push of one draw's factors into the next slot, which then holds a draw; a full ring is flushed
int bdf_ring_push(bdf_draw_ring *r, const double *U, const double *V);
// `count` doubles from cell `first` of a plane and its guard to or from buf_dev, flushed first; `what`: "sum" or "plane"
int bdf_ring_copy(bdf_draw_ring *r, const char *who, const char *what, double *plane, double *buf_dev, int64_t first, int64_t count, int write);
int bdf_ring_set_draws(bdf_draw_ring *r, const char *who, double draws);
// k_topk_rows on a plane scored as plane / draws + mean_value, after the checks of `rel` against the scored rows
int bdf_topk_plane(const bdf_draw_ring *r, const char *who, const double *plane, const bdf_rel *rel, int K, double draws, double mean_value,
                   int32_t *items_out, double *scores_out);
