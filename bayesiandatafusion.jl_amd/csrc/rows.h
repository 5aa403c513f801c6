// rows.h -- what the units of the latent-row sampler share: the kernels' argument blocks and work records, and the launchers
// that the router (rows_plan.hip: bdf_launch_sample_rows) calls in turn.
//   k_rows_lr.hip      K1-lr  rows of few observations at D > 16, by the low-rank map        bdf_lr_launch
//   k_rows_small.hip   K1s    short rows at D <= 16, four to a wave                          bdf_small_launch
//   k_rows_col.hip     K1c    one two-mode relation at 16 < D <= 32, column layout           bdf_col_launch
//   k_sample_rows.hip  K1     every other row, one wave per item                             bdf_k1_launch
//   k_rows_ss.hip      K1-ss  every row of a call under the spike-and-slab prior, K1's items   bdf_ss_launch
#pragma once
#include "bdf_common.h"

// kernel launch argument blocks ------------------------------------------------------------
#define BDF_K1_CODES 32            // distinct values up to which K1's coded variant keeps a per-wave table
struct TermDev {
    const int64_t *rowptr;
    const int32_t *colidx;
    const double *vals;
    const int32_t *perm;
    const double *linear;
    const double *fac[BDF_MAX_MODES - 1];
    int64_t nnz;
    int32_t n_other;
    int32_t lean;              // K1 lean gather: 1 = shared baseline, <= 2 other modes, factor matrices < 4 GiB with < 2^24
                               // rows (32-bit offsets); 2 = the same with 64-bit row offsets (D > 32 only); 0 = general path
    double alpha, mean;
    const uint32_t *packed;    // nullable: (value code << 24) | other-mode id per observation, with
    const double *table;       // the code -> value table (256 doubles)
    int32_t n_codes, _padc;
    const double *alpha_dev;   // nullable: the relation's precision in device memory (sampled on the device: sample_alpha inside bdf_gibbs_sweep); else `alpha`
    const double *weight;      // nullable: a precision weight per observation in the caller's COO order (bdf_term.obs_precision): the launch takes k_rows_w
};

__device__ __forceinline__ double term_alpha(const TermDev &T) { return T.alpha_dev ? *T.alpha_dev : T.alpha; }

struct SampleArgs {
    TermDev t[BDF_MAX_TERMS];  // (136 bytes each; with PlanDev the kernels' arguments stay far below the 4 KB a dispatch carries)
    int32_t n_terms, D;
    const double *mu;
    int32_t mu_is_matrix, _pad;
    const double *Lambda;
    uint32_t sweep, _pad3;
    uint64_t seed;
    uint32_t entity_tag, _pad2;
    double *out;
    const double *prior_b;     // Lambda mu (D) or Lambda mu_i (D x N), filled by the launch front-end
    const double *prior_c;     // index-reversed Lambda in the accumulator layout, filled by the launch front-end
    double *P_dump, *b_dump;
    int *flag;
    // nullable: the launch does not wait for the hyperprior draw that writes the prior pack; every wave polls *ready until
    // it reaches ready_want right before it adds the prior (bdf_gibbs_sweep on reserved CUs), and reads the pack past
    // the non-coherent caches
    const uint32_t *ready;
    uint32_t ready_want, _pad4;
    // nullable (bdf_ctx_span_next_rows): {start of the launch's first wave, end of its last} in s_memrealtime ticks (the 100 MHz
    // clock the XCDs share), by one atomic min / max per wave -- a launch's duration without events around it (k_rows_col only)
    unsigned long long *span;  // (64 shards of {start, end}: wave w uses shard w % 64)
    // nullable (bdf_gibbs_sweep, k_rows_col only): 64 counters, 16 words apart; a wave that has written its rows (write-through, drained)
    // adds 1 to counter (wave % 64): what the hyperprior chain polls instead of waiting for the launch's completion event
    uint32_t *done;
    // bdf_sample_rows_spike (k_rows_ss.hip, spike.h) only: the prior's state (4 D doubles) and the entity's CURRENT rows (D x N), from
    // which the coordinate sweep of every row starts
    const double *spike_state;
    const double *u_current;
    // K1c at D = 32 only, both nullable (rows_plan.hip's launch_column fills them in): the gather image of the OTHER entity's sample,
    // which the observations are then gathered from in place of t[0].fac[0], and where the launch leaves the image of the rows it
    // writes (k_rows_col.hip, col_gather4; k_gather_image.hip)
    const double *img_in;
    double *img_out;
};

// the padded dimension the row kernels are compiled for
inline int bdf_rows_dp(int D) { return D <= 16 ? 16 : (D <= 32 ? 32 : 64); }

// ---- the router and its per-context state (rows_plan.hip) -------------------------------------------------------------
int bdf_launch_sample_rows(bdf_ctx *ctx, const SampleArgs &a, const bdf_rel *const *rels, const int *modes, int shard,
                           int n_shards, bool dump);
bdf_rows_state *bdf_rows_state_create();
void bdf_rows_state_delete(bdf_rows_state *st);                   // its plans and images free themselves
void bdf_plans_release(bdf_ctx *ctx, uint64_t rel_serial);        // rel_serial 0: every plan of the context
// {iteration number, rows by K1-lr, K1s, K1c, K1, K1's items, K1c's waves} of the latest launch under entity_tag, or NULL
const std::array<int64_t, 7> *bdf_rows_dispatch_counts(const bdf_ctx *ctx, uint32_t entity_tag);

// ---- one row of ONE two-mode relation, whole: the record of k_rows_small and of the low-rank kernels --------------------
struct RowItem {
    int32_t row;          // where the sample is written (position in the factor matrix); -1: no row (padding to four rows per wave)
    int32_t orig;         // the row's original id (random stream)
    int64_t q_begin;
    int32_t count, _pad;
};

// K1s (k_rows_small.hip): n_items records, a multiple of four
int bdf_small_launch(bdf_ctx *ctx, const SampleArgs &a, const RowItem *items, int64_t n_items, hipEvent_t e0, hipEvent_t e1);
// K1-lr (k_rows_lr.hip)
int bdf_lr_launch(bdf_ctx *ctx, const SampleArgs &a, int64_t M_other, int64_t n_rows_entity, const RowItem *items, int64_t n_items, int64_t n_padded, int64_t n32_padded,
                  const int32_t *rows_dev, bool transform, hipEvent_t e0, hipEvent_t e1);
int bdf_lr_max_observations();
int bdf_lr32_max_observations();

// ---- K1 (k_sample_rows.hip): one wave per item ------------------------------------------------------------------------
struct Item {             // one wave's accumulation work
    int32_t row;          // entity row: where the sample is written (the row's position in the factor matrix)
    int32_t term;
    int64_t q_begin;      // first observation (index into the term's CSR arrays)
    int32_t count;        // observations in this item
    int32_t slot;         // partial slot, or -1 for a direct row
    int32_t srow;         // index of the row in the split-row table (split items)
    int32_t orig;         // the row's ORIGINAL id: keys its random stream (== row unless the relation was created with a layout)
};

struct SplitRow {
    int32_t row;
    int32_t slot_begin, n_slots;
    int32_t _pad;
};

struct PlanDev {
    const Item *direct;   int32_t n_direct;
    const Item *split;    int32_t n_split;
    const SplitRow *rows; int32_t n_split_rows;
    double *partials;                            // n_split * PSZ doubles
    int32_t *arrived;                            // per split row: items that have published their partial (self-resetting)
    const int32_t *order;                        // launch order: wave w takes item order[w] of [split | direct]
};

int bdf_k1_launch(bdf_ctx *ctx, const SampleArgs &a, const PlanDev &p, bool dump, hipEvent_t e0, hipEvent_t e1);
// the same items under the spike-and-slab prior (k_rows_ss.hip): a.spike_state and a.u_current set, a.prior_c the image of diag(tau)
int bdf_ss_launch(bdf_ctx *ctx, const SampleArgs &a, const PlanDev &p, hipEvent_t e0, hipEvent_t e1);
// diag(tau) of a spike_state as a D x D matrix, and D zeros behind it (the prior mean): what bdf_prior_launch takes (k_spike_hyper.hip)
int bdf_spike_lambda_launch(bdf_ctx *ctx, int D, const double *spike_state, double *Lambda_mu_out);
// ---- the non-negative prior (k_nonneg.hip) --------------------------------------------------------
// diag(tau) as a D x D matrix, and D zeros behind it (the prior mean): what bdf_prior_launch takes
int bdf_nonneg_lambda_launch(bdf_ctx *ctx, int D, const double *tau, double *Lambda_mu_out);
// rows per chunk on this context for num_latent = D: the caller's (bdf_ctx_set_nonneg_chunk) or the default under the scratch cap
int64_t bdf_nonneg_chunk_rows(const bdf_ctx *ctx, int D);
// The coordinate sweep of n systems, one lane each: system i is P + i D^2, c + i D.  Its row -- the random stream, and with
// rows != NULL the row of u_current and out -- is rows[pos0 + i * stride], or with rows == NULL row_begin + i, where u_current and
// out are indexed by i.
struct NonnegSweepArgs {
    const double *P, *c, *u_current;
    double *out;
    const int32_t *rows;
    int64_t pos0, stride, row_begin, n;
    uint64_t seed;
    uint32_t sweep, entity_tag;
    int32_t D, wide;           // wide: D is even and P is 16-byte aligned -- a row of P by 16-byte loads
    int *flag;                 // the context's flag word: a diagonal entry that is not positive and finite sets the bit a bad pivot sets
};
int bdf_nonneg_sweep_launch(bdf_ctx *ctx, const NonnegSweepArgs &a);
// the prior pack of a launch: out_b = Lambda mu (nrows = 1, mu_is_matrix = 0) or Lambda mu_i for nrows rows, out_c = the
// accumulator-layout image of the index-reversed Lambda (bdf_prior_image_doubles(D) doubles)
inline int bdf_prior_image_doubles(int D) { const int DB = bdf_rows_dp(D) / 16; return DB * (DB + 1) / 2 * 4 * 64; }
int bdf_prior_launch(bdf_ctx *ctx, int D, const double *Lambda, const double *mu, int64_t nrows, int mu_is_matrix, double *out_b, double *out_c);

// ---- the fold-in of new rows (k_foldin.hip) ------------------------------------------------------------
// the systems of positions k0 .. k1 - 1 of the term's row order by the dump launch, with the caller's prior pack (bdf_api.hip)
int bdf_foldin_systems_launch(bdf_ctx *ctx, int D, int64_t N, const bdf_term *term, const double *mu, int mu_is_matrix, const double *Lambda,
                              const double *prior_b, const double *prior_c, int64_t k0, int64_t k1, double *P_out, double *b_out);

// ---- K1c (k_rows_col.hip): four rows per wave in the column layout ----------------------------------------------------
struct ColJob {           // one lane row of one round
    int32_t row;          // where the sample is written (the row's position in the factor matrix); -1: idle lane row
    int32_t orig;         // the row's ORIGINAL id: keys its random stream
    int64_t q_begin;      // first observation of the piece (index into the term's arrays)
    int32_t count;        // observations of the piece
    int32_t srow;         // a row that spans waves: its entry of the split-row table, else -1
    int32_t slot;         // ... and this part's slot in the slab
    int32_t flags;
};
#define COLF_LEADER 1     // the lane row that writes the sample of its group's row
#define COLF_PAIR 2       // the lane row's sums are added to its neighbour's (lane ^ 16)
#define COLF_QUAD 4       // ... and to the other half's (lane ^ 32)
#define COLF_MULTI 8      // the round is one part of a row that spans waves
struct ColSplit { int32_t slot_begin, n_slots; };
struct ColPlanDev {
    const ColJob *jobs;           // four per round; wave w runs round w
    int32_t n_waves, _pad;
    const ColSplit *rows;
    double *partials;
    int32_t *arrived;             // per split row: parts that have published (self-resetting)
};
struct bdf_row_ref { int32_t out, orig; int64_t qb, cnt; };
struct bdf_col_plan {
    DevBuf<ColJob> jobs_dev;
    DevBuf<ColSplit> rows_dev;
    DevBuf<double> partials_dev;
    DevBuf<int32_t> arrived_dev;
    int32_t n_waves = 0, n_split_rows = 0;
    int64_t n_rounds = 0;
    double cost_max = 0.0, cost_min = 0.0;      // the planner's cost model: the heaviest and the lightest wave
};
int bdf_col_plan_build(bdf_ctx *ctx, const std::vector<bdf_row_ref> &rows, int T, int64_t slots, bdf_col_plan &plan);
// img_tier: the kind of a.img_in (ignored without one)
int bdf_col_launch(bdf_ctx *ctx, const SampleArgs &a, const bdf_col_plan &plan, int64_t M_other, int img_tier, hipEvent_t e0, hipEvent_t e1);

// ---- K1c's gather image (k_gather_image.hip; the registry of a context's images: rows_plan.hip) -----------------------
// tier 1: the pair image, 32 doubles per row; tier 2: the full image, 64 (k_rows_col.hip, col_gather4)
inline int64_t bdf_gather_image_row_doubles(int tier) { return tier == 2 ? 64 : 32; }
int64_t bdf_col_image_max_rows();                                  // the most rows K1c gathers from an image
// image = the image of the M rows of 32 doubles at `sample`, on the context's stream
int bdf_gather_image_pack_launch(bdf_ctx *ctx, const double *sample, int64_t M, int tier, double *image);
// something other than a K1c launch with an image has written the sample at `sample` (NULL: any sample): its image is stale
void bdf_gather_image_invalidate(bdf_ctx *ctx, const double *sample);
