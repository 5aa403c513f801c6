// rows_plan.hip -- the latent-row sampler's host side: which of the four row kernels takes which row of a launch, the cached
// plan that records it, and the launches.
//
// bdf_launch_sample_rows (the end of this file) is the one entry: prior pack, routing key, plan (built once per key and kept
// in the context), dispatch counts, then up to four launches in a fixed order
//     K1-lr  k_rows_lr.hip      rows of few observations at D > 16          (route_key: key.lr / key.lr32, collect_rows: enough of them)
//     K1s    k_rows_small.hip   short rows at D <= 16                       (route_key: key.small)
//     K1c    k_rows_col.hip     every other row at 16 < D <= 32             (route_key: key.col)
//     K1     k_sample_rows.hip  what is left
// An eligibility rule lives in route_key and nowhere else; which kernel ONE row goes to is classify().  No kernel here.
#include "rows.h"
#include "c_layout_chol.h"
#include <cstdlib>
#include <mutex>

namespace {

// ---- the plan (items, split rows, slab) for a (terms, row list) combination, cached per context -----------------------
struct PlanKey {
    uint64_t rel[BDF_MAX_TERMS];      // relation serials
    int mode[BDF_MAX_TERMS];
    int n_terms, DP, T, Tp;
    int shard, n_shards;
    int small;                        // > 0: rows of at most this many observations go to k_rows_small (four rows per wave)
    int lr;                           // > 0: rows of at most this many observations go to k_rows_lr (the low-rank sampler, k_rows_lr.hip)
    int lr32;                         // > lr: rows of lr + 1 .. lr32 observations too (k_rows_lr32: two observations per lane, D > 32)
    int64_t lr_min, lr_other;         // ... if the launch has at least lr_min of them, and at least half as many as the opposite entity has rows
    int col;                          // > 0: the rows of k_rows go to k_rows_col instead (four rows per wave, column layout), cut into pieces of at most this size
    int col_slots;                    // ... dealt to at most this many waves
    int64_t k0, k1;                   // k1 > 0 (a system dump of bdf_sample_rows_nonneg): positions k0 .. k1 - 1 of the shard's row list only, system k at index k - k0
    bool operator<(const PlanKey &o) const { return memcmp(this, &o, sizeof(PlanKey)) < 0; }
};

struct Plan {
    PlanDev dev{};                    // K1's items, split rows and slab: the kernels' view of the seven buffers below
    DevBuf<Item> direct_dev, split_dev;
    DevBuf<SplitRow> rows_dev;
    DevBuf<int32_t> order_dev, arrived_dev;
    DevBuf<double> partials_dev;
    DevBuf<RowItem> small_dev;
    int64_t n_small = 0;              // entries of small_dev (a multiple of 4)
    DevBuf<RowItem> lr_dev;           // the rows of the low-rank sampler, and their positions for the back-transform
    DevBuf<int32_t> lr_rows_dev;
    int64_t n_lr = 0, n_lr_padded = 0;   // rows of the low-rank sampler in all; records of the rows of at most key.lr observations (a multiple of 4)
    int64_t n_lr32_padded = 0;           // ... and of the rows of key.lr + 1 .. key.lr32 observations, behind them in lr_dev
    bdf_col_plan col;                 // the rows of k_rows_col (K1c)
    int64_t rows_lr = 0, rows_small = 0, rows_col = 0, rows_k1 = 0;      // how the plan's rows are shared out (bdf_ctx_rows_dispatch)
};

// what lr_T / lr_vt of the context were computed from: a later chunk of the same entity launch reuses them
struct LrKey {
    const void *fac, *Lambda, *mu; uint32_t sweep, tag; int D; int64_t M;
    bool operator==(const LrKey &o) const { return fac == o.fac && Lambda == o.Lambda && mu == o.mu && sweep == o.sweep && tag == o.tag && D == o.D && M == o.M; }
};

std::mutex g_plans_mutex;             // around every context's plan cache

// K1c's gather image of the sample at one address (k_gather_image.hip).  `valid`: the image is that of the sample as the library last
// saw it written -- left by the K1c launch that sampled it, or packed from it since; every row launch clears it for its `out`, and
// so does whoever else writes a sample (bdf_gather_image_invalidate).  A launch believes it only when its caller vouches that nothing
// outside the library writes the sample either (bdf_ctx::gimg_trust: bdf_gibbs_sweep, whose buffers are its own); every other launch
// packs the image anew.
struct GatherImage { DevBuf<double> dev; int64_t rows = 0; int tier = 0; bool valid = false; };

}  // namespace

// the row launcher's state of one context (bdf_ctx::rows)
struct bdf_rows_state {
    std::map<PlanKey, Plan> plans;
    std::map<uint32_t, std::array<int64_t, 7>> dispatch;      // bdf_ctx_rows_dispatch: per entity tag, see bdf_rows_dispatch_counts
    LrKey lr_key{nullptr, nullptr, nullptr, 0, 0, 0, 0};
    std::map<const double *, GatherImage> images;             // by the sample's address: an image follows its sample through the rotation
    int64_t image_stats[3] = {0, 0, 0};                       // bdf_ctx_gather_image_stats
};

namespace {

constexpr int64_t MAX_PIECES = 64;

// one row of the launch as the plan sees it: where its sample goes, its original id, and per term its observations in
// that term's device arrays
struct RowRef {
    int32_t out, orig;
    int64_t qb[BDF_MAX_TERMS];
    int64_t cnt[BDF_MAX_TERMS];
};

enum class Route { LowRank, LowRank32, Small, Column, K1Direct, K1Split };

// The kernel that takes row rr; n_items: the items K1 cuts it into (set for K1Direct / K1Split).  The three whole-row kernels
// come first: they take rows with observations in at most one relation, and no more of them than the item size
// (route_key: key.small, key.lr, key.lr32 <= key.T), so such a row would be ONE item of K1.
Route classify(const PlanKey &key, const RowRef &rr, bool lr_on, int &n_items)
{
    int nz = 0;
    int64_t n = 0;
    for (int r = 0; r < key.n_terms; r++) { nz += rr.cnt[r] > 0; n += rr.cnt[r]; }
    if (nz <= 1 && key.small > 0 && n <= key.small) return Route::Small;
    if (nz <= 1 && lr_on && n <= key.lr) return Route::LowRank;
    if (nz <= 1 && lr_on && n <= key.lr32) return Route::LowRank32;
    if (key.col > 0) return Route::Column;
    const int T = key.T;
    n_items = 0;
    for (int r = 0; r < key.n_terms; r++) n_items += (int)std::min<int64_t>((rr.cnt[r] + T - 1) / T, MAX_PIECES);
    // (at most MAX_PIECES per relation: the row's finisher adds the partial sums one slot after the other, ~0.5 us each
    // -- a 78,000-observation row of config C5 in 128-observation pieces would keep it busy for 0.3 ms)
    // a row that is split anyway is cut into smaller pieces than the longest whole row: the launch ends with the split
    // rows (their pieces gather at a sixth of the matrix pipe each, then one wave sums and finishes the row)
    if (n_items > 1 && key.Tp != T) {
        n_items = 0;
        for (int r = 0; r < key.n_terms; r++) n_items += (int)std::min<int64_t>((rr.cnt[r] + key.Tp - 1) / key.Tp, MAX_PIECES);
    }
    return n_items <= 1 ? Route::K1Direct : Route::K1Split;
}

int build_plan(bdf_ctx *ctx, const PlanKey &key, const std::vector<RowRef> &rows, bool lr_on, Plan &plan)
{
    const int Tp = key.Tp, DB = key.DP / 16;
    const int psz = DB * (DB + 1) / 2 * 4 * 64 + DB * 16;      // doubles per partial slot (Geo<DP>::PSZ)
    std::vector<Item> direct, split;
    std::vector<RowItem> small, lr, lr32;
    std::vector<SplitRow> srows;
    std::vector<bdf_row_ref> crows;
    for (const RowRef &rr : rows) {
        const int32_t row = rr.out;
        int n_items = 0;
        const Route route = classify(key, rr, lr_on, n_items);
        if (route == Route::Column) { crows.push_back(bdf_row_ref{rr.out, rr.orig, rr.qb[0], rr.cnt[0]}); continue; }
        if (route == Route::K1Split) {
            SplitRow sr{row, (int32_t)split.size(), n_items, 0};
            for (int r = 0; r < key.n_terms; r++) {
                const int64_t beg = rr.qb[r], n = rr.cnt[r];
                const int pieces = (int)std::min<int64_t>((n + Tp - 1) / Tp, MAX_PIECES);
                for (int s = 0; s < pieces; s++) {
                    // equal pieces rather than T, T, ..., remainder
                    const int64_t b0 = beg + n * s / pieces, b1 = beg + n * (s + 1) / pieces;
                    split.push_back(Item{row, r, b0, (int32_t)(b1 - b0), (int32_t)split.size(), (int32_t)srows.size(), rr.orig});
                }
            }
            srows.push_back(sr);
            continue;
        }
        Item it{row, 0, 0, 0, -1, -1, rr.orig};      // the row whole: the observations of its one relation that has any
        for (int r = 0; r < key.n_terms; r++)
            if (rr.cnt[r] > 0) { it.term = r; it.q_begin = rr.qb[r]; it.count = (int32_t)rr.cnt[r]; }
        if (route == Route::K1Direct) { direct.push_back(it); continue; }
        (route == Route::Small ? small : (route == Route::LowRank ? lr : lr32)).push_back(RowItem{row, rr.orig, it.q_begin, it.count, 0});
    }
    // launch order.  The items are listed longest first (split pieces, then rows by falling observation count); waves
    // that share a SIMD should be at different phases (the gather/MFMA phase of one under the factorisation of another),
    // so neighbours in launch order should differ in length: a fixed stride permutation of the sorted list.
    const int64_t total = (int64_t)split.size() + (int64_t)direct.size();
    std::vector<int32_t> order((size_t)total);
    {
        auto gcd = [](int64_t x, int64_t y) { while (y) { int64_t t = x % y; x = y; y = t; } return x; };
        int64_t stride = 1;
        if (total > 2) {
            stride = (int64_t)(0.6180339887 * (double)total) | 1;
            while (gcd(stride, total) != 1) stride += 2;
        }
        for (int64_t i = 0; i < total; i++) order[(size_t)i] = (int32_t)((i * stride) % total);
    }
    int rc;
    if (key.col > 0 && (rc = bdf_col_plan_build(ctx, crows, key.col, key.col_slots, plan.col))) return rc;
    plan.rows_lr = (int64_t)lr.size() + (int64_t)lr32.size(); plan.rows_small = (int64_t)small.size(); plan.rows_col = (int64_t)crows.size();
    plan.rows_k1 = (int64_t)direct.size() + (int64_t)srows.size();
    while (small.size() % 4) small.push_back(RowItem{-1, 0, 0, 0, 0});
    plan.n_small = (int64_t)small.size();
    if (!small.empty() && (rc = plan.small_dev.upload(small))) return rc;
    plan.n_lr = (int64_t)lr.size() + (int64_t)lr32.size();
    if (plan.n_lr > 0) {
        // longest first: the waves of a workgroup then have rows of like length
        auto by_count = [](const RowItem &x, const RowItem &y) { return x.count > y.count; };
        std::stable_sort(lr.begin(), lr.end(), by_count);
        std::stable_sort(lr32.begin(), lr32.end(), by_count);
        std::vector<int32_t> lr_rows;
        lr_rows.reserve((size_t)plan.n_lr);
        for (const RowItem &x : lr) lr_rows.push_back(x.row);
        for (const RowItem &x : lr32) lr_rows.push_back(x.row);
        // (the positions in ASCENDING order: they are what the dense passes over the rows walk -- the back-transform x = L^-T q and
        // the per-row prior means -- and a pass over rows in the sampler's order, longest first, reads and writes 512-byte rows at
        // random)
        std::sort(lr_rows.begin(), lr_rows.end());
        while (lr.size() % 4) lr.push_back(RowItem{-1, 0, 0, 0, 0});      // four rows per wave
        while (lr32.size() % 4) lr32.push_back(RowItem{-1, 0, 0, 0, 0});
        plan.n_lr_padded = (int64_t)lr.size();
        plan.n_lr32_padded = (int64_t)lr32.size();
        lr.insert(lr.end(), lr32.begin(), lr32.end());
        if ((rc = plan.lr_dev.upload(lr)) || (rc = plan.lr_rows_dev.upload(lr_rows))) return rc;
    }
    if ((rc = plan.direct_dev.upload(direct)) || (rc = plan.split_dev.upload(split)) ||
        (rc = plan.rows_dev.upload(srows)) || (rc = plan.order_dev.upload(order)) ||
        (rc = plan.partials_dev.alloc_bytes(std::max<size_t>(split.size() * (size_t)psz * sizeof(double), 8))) ||
        (rc = plan.arrived_dev.alloc_bytes(std::max<size_t>(srows.size() * sizeof(int32_t), 8))))
        return rc;
    // on the launch stream: hipMemset runs on the NULL stream and returns before the device has done it, and a kernel on a
    // non-blocking stream does not wait for it -- the first launch of a new plan could have its counters zeroed under it
    // (a split row then never finds its last piece: the row keeps its old content)
    BDF_HIP(hipMemsetAsync(plan.arrived_dev, 0, std::max<size_t>(srows.size() * sizeof(int32_t), 8), ctx->stream));
    plan.dev = PlanDev{plan.direct_dev.get(), (int32_t)direct.size(), plan.split_dev.get(), (int32_t)split.size(), plan.rows_dev.get(),
                       (int32_t)srows.size(), plan.partials_dev.get(), plan.arrived_dev.get(), plan.order_dev.get()};
    return BDF_OK;
}

// ---- step 2: the plan key -- item sizes, and for each of the three other kernels whether (and up to which row length) this
// launch may use it.  M_other: the opposite entity's rows, for the low-rank and the column launch. -----------------------
void route_key(const bdf_ctx *ctx, const SampleArgs &a, const bdf_rel *const *rels, const int *modes, int shard, int n_shards, bool dump,
               PlanKey &key, int64_t &M_other)
{
    const int DP = bdf_rows_dp(a.D);
    memset(&key, 0, sizeof(key));
    for (int r = 0; r < a.n_terms; r++) { key.rel[r] = rels[r]->serial; key.mode[r] = modes[r]; }
    key.n_terms = a.n_terms; key.DP = DP; key.T = ctx->item_size; key.Tp = std::min(ctx->piece_size, ctx->item_size); key.shard = shard; key.n_shards = n_shards;
    if (dump) { key.k0 = ctx->rows_k0; key.k1 = ctx->rows_k1; }
    if (ctx->item_auto) {
        // Rows are cut into pieces so that a launch of a few thousand rows has no wave much longer than the others.  A launch with
        // hundreds of waves per resident slot has no such tail, and every piece costs a partial sum written to the slab and read
        // back (21 KB at D = 64: the 540,000 pieces of configuration C4's item launch moved 22 GB): larger items there -- about
        // sixteen waves per slot, between the default and 2048 observations (the same for every shard of the launch).
        // (a NOMINAL slot count -- 256 CUs -- not the device's or the stream's: the cut of a row, and with it the order of its
        // floating-point sums, must not depend on the CU count or on BDF_RESERVE_CUS)
        int64_t nnz_launch = 0;
        for (int r = 0; r < a.n_terms; r++) nnz_launch += rels[r]->idx[modes[r]].own_nnz;
        const int64_t slots = (int64_t)256 * 4 * (DP == 64 ? 2 : (DP == 32 ? BDF_K1_WAVES32C : 8));
        const int64_t t = std::min<int64_t>(2048, (nnz_launch / (slots * 16) + 63) / 64 * 64);
        if (t > key.T) { key.T = (int)t; key.Tp = (int)(t * 2 / 3); }
    }
    // the spike-and-slab launch (bdf_sample_rows_spike): K1's items for every row, none of the three kernels below
    if (a.spike_state != nullptr) return;
    // D <= 16, one two-mode relation with the lean gather and no per-observation baseline, an entity of many rows: its short
    // rows four to a wave (k_rows_small).  bdf_ctx_set_small_rows: the longest row taken that way (default 48 observations,
    // environment BDF_K1_SMALL; 0: off) and the smallest entity (default 8192 rows, BDF_K1_SMALL_MIN_ROWS: below that the
    // second launch costs more than it saves)
    const int64_t n_rows_all = rels[0]->sharded ? (int64_t)rels[0]->idx[modes[0]].own_orig.size() : (int64_t)rels[0]->idx[modes[0]].order.size();
    if (DP == 16 && !dump && ctx->small_max > 0 && a.n_terms == 1 && a.t[0].lean == 1 && a.t[0].n_other == 1 && a.t[0].linear == nullptr &&
        a.t[0].weight == nullptr && n_rows_all >= ctx->small_min_rows)
        key.small = std::min(ctx->small_max, ctx->item_size);

    // D > 16, one two-mode relation without per-observation baselines (shared or per-row prior means): the rows of few observations
    // by the low-rank sampler (k_rows_lr.hip; bdf_ctx_set_lowrank, environment BDF_LOWRANK:
    // the longest such row, -1 = min(16, D / 2), 0 = off) -- when there are enough of them (decided when the plan is built)
    if (DP > 16 && !dump && ctx->lr_max != 0 && a.n_terms == 1 && a.t[0].n_other == 1 && a.t[0].linear == nullptr && a.t[0].weight == nullptr) {
        const int other = 1 - modes[0];
        M_other = rels[0]->nint[other];
        const int lr_want = ctx->lr_max < 0 ? a.D / 2 : ctx->lr_max;
        key.lr = std::min(std::min(lr_want, bdf_lr_max_observations()), ctx->item_size);
        key.lr32 = DP == 64 ? std::min(std::min(lr_want, bdf_lr32_max_observations()), ctx->item_size) : 0;       // (> key.lr: rows of 17 .. 32 observations too)
        key.lr_min = std::max<int64_t>(ctx->lr_min_rows, 1);
        key.lr_other = ctx->lr_min_rows > 0 ? rels[0]->dims[other] : 0;          // (min_rows = 0, a test hook: whenever the entity has such a row)
    }

    // 16 < D <= 32, one two-mode relation on the lean gather path without per-observation baselines: the rows four to a wave in
    // the column layout (K1c, k_rows_col.hip; bdf_ctx_set_col_rows) -- unless the caller chose K1's item size or its general variant
    static const bool no_col = getenv("BDF_K1_GENERAL_KERNEL") != nullptr;          // (test hook: k_rows' general variant)
    if (DP == 32 && a.D > 16 && !dump && ctx->col_piece > 0 && (ctx->col_explicit || ctx->item_auto) && a.n_terms == 1 && a.t[0].n_other == 1 &&
        a.t[0].lean == 1 && a.t[0].linear == nullptr && a.t[0].weight == nullptr && !no_col) {
        key.col = ctx->col_piece;
        if (!ctx->col_explicit) {
            // A row of more than 4 T observations SPANS waves: every part writes its 6.4 KB of sums through to the slab and the part
            // that arrives last adds them, slot after slot -- ~25 us of a wave's slot per part when thousands of them are in flight
            // (profiles/r05_k1c_piece_size.txt: 1,000 rows of 15,000 observations, the reference's benchmark shape, 2.7 ms at
            // T = 128 in 30,000 parts, 0.70 ms at T = 1,024 in 4,000; 4,000 rows of 3,000: 0.73 -> 0.44 ms).  Small pieces are
            // for launches of ONE generation of waves (MovieLens: the heaviest wave is the launch's tail); a launch with many
            // waves per slot takes larger ones: about eight waves' worth of observations per slot of a NOMINAL 2,048 (not the
            // device's or the stream's: the cut of a row must not depend on them), from the WHOLE entity's count -- the same on
            // every shard, chunk and rank -- between the default and 2,048.
            const int64_t nnz_entity = (int64_t)rels[0]->idx[modes[0]].rowptr.back();
            const int64_t t = std::min<int64_t>(2048, (nnz_entity / (2048 * 8) + 63) / 64 * 64);
            if (t > key.col) key.col = (int)t;
        }
        key.col_slots = std::max(1, ctx->n_cus - ctx->reserve_cus) * 4 * 2;       // two waves per SIMD
        M_other = rels[0]->nint[1 - modes[0]];
    }
}

// ---- step 3: the rows of this shard / chunk, and whether the low-rank sampler is on for the entity ----------------------
bool collect_rows(const PlanKey &key, const bdf_rel *const *rels, const int *modes, std::vector<RowRef> &rows)
{
    if (rels[0]->sharded) {
        // a relation created with a layout holds this rank's rows only, chunk after chunk: `shard` is the chunk
        const bdf_mode_index &ix0 = rels[0]->idx[modes[0]];
        for (int64_t o = ix0.chunk_begin[(size_t)key.shard]; o < ix0.chunk_begin[(size_t)key.shard + 1]; o++) {
            RowRef rr;
            rr.out = ix0.own_pos[(size_t)o]; rr.orig = ix0.own_orig[(size_t)o];
            for (int r = 0; r < key.n_terms; r++) {
                const bdf_mode_index &ix = rels[r]->idx[modes[r]];
                rr.qb[r] = ix.own_q[(size_t)o]; rr.cnt[r] = ix.own_q[(size_t)o + 1] - ix.own_q[(size_t)o];
            }
            rows.push_back(rr);
        }
    } else {
        // rows of this shard: positions shard, shard + n_shards, ... of the degree-descending order of the first
        // relation (the reference deals rows i:P:N to its P workers for the same balance, sampling.jl:154)
        // (key.k1 > 0: entries k0 .. k1 - 1 of that list, and the system of entry k goes to index k - k0)
        const std::vector<int32_t> &order = rels[0]->idx[modes[0]].order;
        const size_t first = (size_t)key.shard + (size_t)key.k0 * (size_t)key.n_shards;
        const size_t last = key.k1 > 0 ? std::min(order.size(), (size_t)key.shard + (size_t)key.k1 * (size_t)key.n_shards) : order.size();
        for (size_t pos = first; pos < last; pos += (size_t)key.n_shards) {
            RowRef rr;
            rr.out = rr.orig = order[pos];
            if (key.k1 > 0) rr.out = (int32_t)((pos - first) / (size_t)key.n_shards);
            for (int r = 0; r < key.n_terms; r++) {
                const auto &rp = rels[r]->idx[modes[r]].rowptr;
                rr.qb[r] = rp[(size_t)rr.orig]; rr.cnt[r] = rp[(size_t)rr.orig + 1] - rp[(size_t)rr.orig];
            }
            rows.push_back(rr);
        }
    }
    // the low-rank sampler pays its set-up (the opposite factor transformed, two more launches) only with enough rows:
    // counted over the WHOLE entity (the host's index is the whole relation's on every rank), so that shards, chunks and
    // ranks decide alike
    if (key.lr <= 0) return false;
    const std::vector<int64_t> &rp = rels[0]->idx[modes[0]].rowptr;
    int64_t cnt = 0;
    for (size_t i = 0; i + 1 < rp.size(); i++) cnt += rp[i + 1] - rp[i] <= key.lr;
    return cnt >= key.lr_min && 2 * cnt >= key.lr_other;
}

// ---- step 6, the two stages with rules of their own --------------------------------------------------------------------
int launch_lowrank(bdf_ctx *ctx, const SampleArgs &a, const Plan &plan, int64_t M_other, int64_t n_rows_entity, int shard, hipEvent_t e0, hipEvent_t e1)
{
    // the constants of the launch (L, the opposite factor transformed): once per entity launch -- a later chunk of the same
    // launch (same inputs, same iteration) finds them in the context
    const LrKey now{a.t[0].fac[0], a.Lambda, a.mu, a.sweep, a.entity_tag, a.D, M_other};
    const bool same = shard > 0 && now == ctx->rows->lr_key;
    int rc = bdf_lr_launch(ctx, a, M_other, n_rows_entity, plan.lr_dev, plan.n_lr, plan.n_lr_padded, plan.n_lr32_padded, plan.lr_rows_dev, !same, e0, e1);
    if (!rc) ctx->rows->lr_key = now;
    return rc;
}

// the context's image of the `rows` rows at `sample` (allocated at first use; its content is the caller's business)
int image_of(bdf_ctx *ctx, const double *sample, int64_t rows, int tier, GatherImage **out)
{
    auto &m = ctx->rows->images;
    auto it = m.find(sample);
    if (it != m.end() && (it->second.rows != rows || it->second.tier != tier)) { m.erase(it); it = m.end(); }
    if (it == m.end()) {
        GatherImage g;
        g.rows = rows; g.tier = tier;
        if (int rc = g.dev.alloc((size_t)std::max<int64_t>(rows, 1) * (size_t)bdf_gather_image_row_doubles(tier))) return rc;
        it = m.emplace(sample, std::move(g)).first;
    }
    *out = &it->second;
    return BDF_OK;
}

// n_rows: the rows of the launch's entity; whole: the launch is the call's only one and the call the entity's only one
int launch_column(bdf_ctx *ctx, const SampleArgs &a, const Plan &plan, int64_t M_other, int64_t n_rows, bool more, bool whole, bool trust,
                  hipEvent_t e0, hipEvent_t e1)
{
    static const bool no_coded = getenv("BDF_K1_NO_CODED") != nullptr;               // test hook: ids and values instead of the packed words
    SampleArgs ac = a;
    if (no_coded) ac.t[0].packed = nullptr;
    // The gather image (k_rows_col.hip, col_gather4): D = 32, the whole entity in one call (no chunks, no layout: `whole`), an
    // opposite entity the image's offsets reach.  The opposite sample's image is the one its own launch left if the caller vouches for
    // it, else packed here; this launch leaves its rows' image when it writes ALL of the entity's rows -- K1-lr or K1s taking some of
    // them leaves none, and the next launch that gathers them packs one.
    const int tier = ctx->gather_image;
    if (tier != 0 && a.D == 32 && whole && M_other > 0 && M_other <= bdf_col_image_max_rows()) {
        int rc;
        bdf_rows_state *st = ctx->rows;
        if (st->images.size() >= 48) st->images.clear();    // (freeing waits for the launches that still read them; addresses no longer in use: callers that pass fresh buffers every call)
        GatherImage *src;
        if ((rc = image_of(ctx, a.t[0].fac[0], M_other, tier, &src))) return rc;
        if (!(trust && src->valid)) {
            if ((rc = bdf_gather_image_pack_launch(ctx, a.t[0].fac[0], M_other, tier, src->dev))) return rc;
            src->valid = true;
            st->image_stats[1]++;
        }
        ac.img_in = src->dev;
        st->image_stats[0]++;
        if (!more && plan.n_lr == 0 && plan.n_small == 0 && plan.rows_col == n_rows && n_rows <= bdf_col_image_max_rows()) {
            GatherImage *dst;
            if ((rc = image_of(ctx, a.out, n_rows, tier, &dst))) return rc;
            ac.img_out = dst->dev;
            dst->valid = true;
            st->image_stats[2]++;
        }
    }
    // the rows' hand-over by counter (SampleArgs::done): only when this launch is ALL of the call's rows
    if (more || plan.n_lr > 0 || plan.n_small > 0) ac.done = nullptr;
    if (ac.done) ctx->rows_done_added = plan.col.n_waves;
    return bdf_col_launch(ctx, ac, plan.col, M_other, tier, e0, e1);
}

}  // namespace

bdf_rows_state *bdf_rows_state_create() { return new bdf_rows_state(); }

void bdf_rows_state_delete(bdf_rows_state *st)
{
    std::lock_guard<std::mutex> lock(g_plans_mutex);
    delete st;
}

const std::array<int64_t, 7> *bdf_rows_dispatch_counts(const bdf_ctx *ctx, uint32_t entity_tag)
{
    auto it = ctx->rows->dispatch.find(entity_tag);
    return it == ctx->rows->dispatch.end() ? nullptr : &it->second;
}

void bdf_gather_image_invalidate(bdf_ctx *ctx, const double *sample)
{
    for (auto &kv : ctx->rows->images)
        if (!sample || kv.first == sample) kv.second.valid = false;
}

// {launches that gathered from an image, images packed from a sample, launches that left the image of their entity's rows} on this
// context so far
extern "C" int bdf_ctx_gather_image_stats(const bdf_ctx *ctx, int64_t out[3])
{
    BDF_REQUIRE(ctx && out, BDF_ERR_ARG, "bdf_ctx_gather_image_stats: NULL argument");
    for (int k = 0; k < 3; k++) out[k] = ctx->rows->image_stats[k];
    return BDF_OK;
}

// parity hook: the image the library holds of the `rows` rows at `sample` (a device address), as a launch left or packed it, into
// host memory (bdf_gather_image_row_doubles per row); an error when it holds none or a stale one
extern "C" int bdf_ctx_gather_image_read(bdf_ctx *ctx, const double *sample, int64_t rows, double *host_out)
{
    BDF_REQUIRE(ctx && sample && host_out, BDF_ERR_ARG, "bdf_ctx_gather_image_read: NULL argument");
    auto it = ctx->rows->images.find(sample);
    BDF_REQUIRE(it != ctx->rows->images.end() && it->second.valid && it->second.rows == rows, BDF_ERR_ARG,
                "bdf_ctx_gather_image_read: no current gather image of %lld rows at this address", (long long)rows);
    BDF_HIP(hipStreamSynchronize(ctx->stream));
    BDF_HIP(hipMemcpy(host_out, it->second.dev, (size_t)rows * (size_t)bdf_gather_image_row_doubles(it->second.tier) * sizeof(double), hipMemcpyDeviceToHost));
    return BDF_OK;
}

// parity hook: the pack kernel on its own -- image_dev = the image (the context's tier) of the `rows` rows of 32 doubles at sample
extern "C" int bdf_gather_image_pack(bdf_ctx *ctx, const double *sample, int64_t rows, double *image_dev)
{
    BDF_REQUIRE(ctx && ctx->gather_image != 0, BDF_ERR_ARG, "bdf_gather_image_pack: the gather image is off on this context");
    return bdf_gather_image_pack_launch(ctx, sample, rows, ctx->gather_image, image_dev);
}

// parity hook: split rows whose pieces did not all arrive in the launches so far (their arrival counters reset themselves
// when the last piece arrives, so any non-zero counter after a completed launch is a row that was never finished)
extern "C" int bdf_rows_unfinished(bdf_ctx *ctx, int64_t *count)
{
    BDF_REQUIRE(ctx && count, BDF_ERR_ARG, "bdf_rows_unfinished: NULL argument");
    BDF_HIP(hipStreamSynchronize(ctx->stream));
    *count = 0;
    std::lock_guard<std::mutex> lock(g_plans_mutex);
    for (auto &kv : ctx->rows->plans) {
        if (kv.second.col.n_split_rows > 0) {
            std::vector<int32_t> hc((size_t)kv.second.col.n_split_rows);
            BDF_HIP(hipMemcpy(hc.data(), kv.second.col.arrived_dev, hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int32_t v : hc) *count += v != 0;
        }
        const int n = kv.second.dev.n_split_rows;
        if (n <= 0) continue;
        std::vector<int32_t> h((size_t)n);
        BDF_HIP(hipMemcpy(h.data(), kv.second.dev.arrived, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t v : h) *count += v != 0;
        static const bool dbg = getenv("BDF_DEBUG_UNFINISHED") != nullptr;
        if (dbg)
            for (int i = 0; i < n; i++)
                if (h[(size_t)i] != 0)
                    fprintf(stderr, "[bdf] unfinished: plan DP=%d T=%d Tp=%d shard %d/%d terms %d, split row %d of %d: counter %d (array %p)\n",
                            kv.first.DP, kv.first.T, kv.first.Tp, kv.first.shard, kv.first.n_shards, kv.first.n_terms, i, n, h[(size_t)i],
                            (void *)kv.second.dev.arrived);
    }
    return BDF_OK;
}

void bdf_plans_release(bdf_ctx *ctx, uint64_t rel_serial)
{
    std::lock_guard<std::mutex> lock(g_plans_mutex);
    auto &plans = ctx->rows->plans;
    for (auto kv = plans.begin(); kv != plans.end();) {
        bool hit = rel_serial == 0;
        for (int r = 0; r < kv->first.n_terms; r++) hit = hit || kv->first.rel[r] == rel_serial;
        if (!hit) { ++kv; continue; }
        kv = plans.erase(kv);
    }
}

int bdf_launch_sample_rows(bdf_ctx *ctx, const SampleArgs &a_in, const bdf_rel *const *rels, const int *modes, int shard,
                           int n_shards, bool dump)
{
    SampleArgs a = a_in;
    int rc;
    // (whatever this call's launches are, they write a.out: its image, if it has one, is stale until a K1c launch leaves a new one)
    const bool image_trust = ctx->gimg_trust;
    ctx->gimg_trust = false;
    struct Range { bdf_ctx *c; ~Range() { c->rows_k0 = c->rows_k1 = 0; } } range_once{ctx};      // (bdf_sample_rows_nonneg's chunk: this launch only)
    bdf_gather_image_invalidate(ctx, a.out);
    const bool spike = a.spike_state != nullptr;      // bdf_sample_rows_spike: every row to K1-style items, finished by k_rows_ss
    if (spike) {
        // the prior of the accumulation is Lambda = diag(tau), mu = 0: the matrix and the zeros by one small launch, then the
        // usual prior pack from them (all of it in the context's scratch: one request, the block may move when it grows)
        const size_t nlm = (size_t)a.D * a.D + a.D, npk = (size_t)a.D + (size_t)bdf_prior_image_doubles(a.D);
        void *pb;
        if ((rc = bdf_scratch(ctx, (nlm + npk) * sizeof(double), &pb))) return rc;
        double *lm = (double *)pb, *pk = lm + nlm;
        if ((rc = bdf_spike_lambda_launch(ctx, a.D, a.spike_state, lm))) return rc;
        if ((rc = bdf_prior_launch(ctx, a.D, lm, lm + (size_t)a.D * a.D, 1, 0, pk, pk + a.D))) return rc;
        a.Lambda = lm; a.mu = lm + (size_t)a.D * a.D; a.mu_is_matrix = 0;
        a.prior_b = pk; a.prior_c = pk + a.D;
    }
    if (a.prior_b == nullptr) {         // no prior pack from bdf_hyper_sample: derive Lambda mu and the image here
        // prior part of b: Lambda mu (one vector) or Lambda mu_i for every row (per-row prior means, macau.jl:104)
        const int64_t nr = a.mu_is_matrix ? rels[0]->nint[modes[0]] : 1;
        void *pb;
        if ((rc = bdf_scratch(ctx, ((size_t)nr * a.D + (size_t)bdf_prior_image_doubles(a.D)) * sizeof(double), &pb))) return rc;
        if ((rc = bdf_prior_launch(ctx, a.D, a.Lambda, a.mu, nr, a.mu_is_matrix, (double *)pb, (double *)pb + nr * a.D))) return rc;
        a.prior_b = (const double *)pb;
        a.prior_c = (const double *)pb + nr * a.D;
    }
    PlanKey key;
    int64_t M_other = 0;
    route_key(ctx, a, rels, modes, shard, n_shards, dump, key, M_other);
    const Plan *plan;
    {
        std::lock_guard<std::mutex> lock(g_plans_mutex);
        auto &plans = ctx->rows->plans;
        auto it = plans.find(key);
        if (it == plans.end()) {
            std::vector<RowRef> rows;
            const bool lr_on = collect_rows(key, rels, modes, rows);
            Plan np;
            if ((rc = build_plan(ctx, key, rows, lr_on, np))) return rc;
            it = plans.emplace(key, std::move(np)).first;
        }
        plan = &it->second;
    }
    const int64_t work[4] = {plan->n_lr, plan->n_small, plan->col.n_waves, (int64_t)plan->dev.n_split + plan->dev.n_direct};      // in launch order
    // bdf_ctx_rows_dispatch: the chunks / shards of one iteration's launch of the entity add up
    std::array<int64_t, 7> &rdsp = ctx->rows->dispatch[a.entity_tag];
    if (rdsp[0] != (int64_t)a.sweep + 1) rdsp = {(int64_t)a.sweep + 1, 0, 0, 0, 0, 0, 0};
    rdsp[1] += plan->rows_lr; rdsp[2] += plan->rows_small; rdsp[3] += plan->rows_col; rdsp[4] += plan->rows_k1;
    rdsp[5] += work[3]; rdsp[6] += work[2];
    // low-rank, small, column, K1.  A caller's timing events (bdf_ctx_time_next_rows) and with them the hand-over of the draw go
    // to the stages that have work: the start to the first, the stop to the last, then both are cleared (a system dump is not timed)
    for (int s = 0; s < 4; s++) {
        if (work[s] <= 0) continue;
        const bool more = std::any_of(work + s + 1, work + 4, [](int64_t w) { return w > 0; });
        const hipEvent_t e0 = dump ? nullptr : ctx->time_start, e1 = (dump || more) ? nullptr : ctx->time_stop;
        if (s == 0) rc = launch_lowrank(ctx, a, *plan, M_other, rels[0]->nint[modes[0]], shard, e0, e1);
        else if (s == 1) rc = bdf_small_launch(ctx, a, plan->small_dev, plan->n_small, e0, e1);
        else if (s == 2) rc = launch_column(ctx, a, *plan, M_other, rels[0]->nint[modes[0]], more, n_shards == 1 && !rels[0]->sharded, image_trust, e0, e1);
        else rc = spike ? bdf_ss_launch(ctx, a, plan->dev, e0, e1) : bdf_k1_launch(ctx, a, plan->dev, dump, e0, e1);
        if (rc) return rc;
        if (!dump) { ctx->time_start = nullptr; if (!more) ctx->time_stop = nullptr; }
    }
    return BDF_OK;
}
