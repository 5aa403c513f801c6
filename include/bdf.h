/*
 * bdf.h -- C ABI of libbdf_hip.so: the MI355X (gfx950) implementation of the Gibbs-sweep
 * hot path of BayesianDataFusion.jl (latent-row sampler + hyperprior + side-information
 * beta update + test-set prediction).
 *
 * The reference has no FFI for this path (pure Julia, multiple dispatch); the entry points
 * below are the seams a maintainer would `ccall` from the reference's own functions.  Each
 * declaration cites the reference interface (file:line under the reference tree) it replaces.
 * INTEGRATION.md shows the Julia-side binding.
 *
 * Conventions
 *   - every function returns BDF_OK (0) or a negative BDF_ERR_* code; bdf_last_error() gives
 *     the message (the reference throws ArgumentError / DimensionMismatch / BoundsError).
 *   - no exceptions, no C++ types, no torch types cross this boundary.
 *   - "dev" pointers are device (HBM) addresses on the context's GPU; "host" pointers are
 *     caller-owned host memory valid for the duration of the call only.
 *   - matrices are column-major as in Julia: an entity's sample matrix is D x N (one column
 *     of D doubles per entity instance), beta is numF x D, a dense F is N x numF.
 *   - ids crossing the boundary from the reference's data model (relation / test pairs) are
 *     1-based like the DataFrame holds them; row lists and ranges are 0-based.
 *   - one host thread per context (macau.jl runs the Gibbs loop on one task); all work is
 *     enqueued on the context's HIP stream, asynchronously unless stated.
 */
#ifndef BDF_H
#define BDF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BDF_OK           0
#define BDF_ERR_ARG     (-1)  /* ArgumentError / DimensionMismatch in the reference */
#define BDF_ERR_BOUNDS  (-2)  /* BoundsError: id outside 1..dims                     */
#define BDF_ERR_HIP     (-3)  /* HIP runtime error                                  */
#define BDF_ERR_NOTPD   (-4)  /* a matrix that must be positive definite is not     */
#define BDF_ERR_NOGPU   (-5)  /* no usable gfx950 device                            */

#define BDF_MAX_MODES 4       /* modes per relation (matrix = 2, tensors up to 4)  */
#define BDF_MAX_TERMS 4       /* relations summed per entity row                   */
#define BDF_MAX_D     64      /* num_latent                                        */

/* RNG stream purposes (DESIGN.md "RNG contract"); Philox4x32-10 counters are
 * (row, pair | row_hi, sweep, purpose<<24 | entity_tag), key = seed. */
#define BDF_P_ROW       1
#define BDF_P_BETA_E1   2
#define BDF_P_BETA_E2   3
#define BDF_P_NW_NORMAL 4
#define BDF_P_GAMMA_N   5
#define BDF_P_GAMMA_U   6
#define BDF_P_NW_MEAN   7
#define BDF_P_BETA_REL1 8   /* sample_beta_rel: noise per observation (row = observation)  */
#define BDF_P_BETA_REL2 9   /* sample_beta_rel: noise per feature    (row = feature)        */
#define BDF_P_HMC_MOMENTUM 10  /* macau_hmc momentum: entity 0 (U) / 1 (V), row = 0-based row, normal k = latent index */
#define BDF_P_HMC_ACCEPT   11  /* macau_hmc Metropolis uniform: entity 0, row 0, pair 0                                */
#define BDF_P_PROBIT       12  /* bdf_probit_draw: uniform per observation (entity 0x800000 | rel_tag, row = observation, pair 0) */
#define BDF_P_CENSORED     13  /* bdf_censored_draw: uniform per observation (entity 0x800000 | rel_tag, row = observation, pair 0) */
#define BDF_P_INTERVAL     14  /* bdf_interval_draw: uniform per observation (entity 0x800000 | rel_tag, row = observation, pair 0) */
#define BDF_P_ORDINAL      15  /* bdf_ordinal_step: entity 0x800000 | rel_tag; row 0, normal k: the proposal's k-th normal; row 1, pair 0: the uniform */
#define BDF_P_ROBUST_N 16      /* bdf_robust_draw: the gamma variate's normals (entity 0x800000 | rel_tag, row = observation, attempt t: normal 2 t) */
#define BDF_P_ROBUST_U 17      /* bdf_robust_draw: ... and its uniforms (the same entity and row, pair = attempt)                               */
#define BDF_P_PG 18            /* bdf_pg_draw: one cursor per observation over the blocks pair = 0, 1, 2, ... (entity 0x800000 | rel_tag, row = observation) */
#define BDF_P_NOISE_N 19       /* bdf_entity_noise_draw: the gamma variate's normals (entity 0x800000 | rel_tag, row = 0-based row of the noise entity, attempt t: normal 2 t) */
#define BDF_P_NOISE_U 20       /* bdf_entity_noise_draw: ... and its uniforms (the same entity and row, pair = attempt; shape < 1: the boost's uniform is pair 0xffff) */
#define BDF_P_SPIKE_N 21       /* bdf_spike_hyper: the gamma variates' normals (entity = entity_tag, row = variate 3 d, 3 d + 1, 3 d + 2 of component d, attempt t: normal 2 t) */
#define BDF_P_SPIKE_U 22       /* bdf_spike_hyper: ... and their uniforms (the same entity and row, pair = attempt; shape < 1: the boost's uniform is pair 0xffff) */
#define BDF_P_SPIKE 23         /* bdf_sample_rows_spike: the inclusion uniform of component d of a row (entity = entity_tag, row = original row, pair d, words x and y) */
#define BDF_P_DENSE 24         /* bdf_dense_impute: the normal of a hole of a dense relation (entity 0x800000 | rel_tag, row = the hole's index, normal 0) */
#define BDF_P_NONNEG 25        /* bdf_sample_rows_nonneg: the uniform of component d of a row (entity = entity_tag, row = original row, pair d, words x and y) */
#define BDF_P_NONNEG_N 26      /* bdf_nonneg_hyper: the gamma variate's normals (entity = entity_tag, row = component d, attempt t: normal 2 t) */
#define BDF_P_NONNEG_U 27      /* bdf_nonneg_hyper: ... and its uniforms (the same entity and row, pair = attempt) */
#define BDF_P_BIAS 28          /* bdf_bias_draw: the normal of a row's bias (entity 0x800000 | rel_tag, row = 0-based row of the biased entity, normal = 0-based mode) */
#define BDF_P_BIAS_N 29        /* bdf_bias_draw: the gamma variate's normals of a mode's bias precision (entity 0x800000 | rel_tag, row = 0-based mode, attempt t: normal 2 t) */
#define BDF_P_BIAS_U 30        /* bdf_bias_draw: ... and its uniforms (the same entity and row, pair = attempt; shape < 1: the boost's uniform is pair 0xffff) */

typedef struct bdf_ctx   bdf_ctx;    /* device, stream, seed, sweep counter, scratch        */
typedef struct bdf_rel   bdf_rel;    /* Relation.data :: IndexedDF / FastIDF on the device  */
typedef struct bdf_pairs bdf_pairs;  /* Relation.test_vec (+ running prediction state)      */
typedef struct bdf_feat  bdf_feat;   /* Entity.F operator (dense / CSR / binary CSR / COO)  */
typedef struct bdf_comm  bdf_comm;   /* the ranks (GPUs) that share the entities' rows       */
typedef struct bdf_gibbs bdf_gibbs;  /* a whole Gibbs iteration enqueued from native code    */
typedef struct bdf_ordinal bdf_ordinal;  /* the sampled cutpoints of an ordinal relation      */

const char *bdf_last_error(void);
int bdf_version(void);

/* ---- context ------------------------------------------------------------------------ */
/* stream: a hipStream_t the caller owns (e.g. torch's current stream); NULL is the device's
 * default stream.  seed keys every random draw of the context. */
int bdf_ctx_create(int device, void *stream, uint64_t seed, bdf_ctx **out);
int bdf_ctx_destroy(bdf_ctx *ctx);
/* Gibbs iteration number (macau.jl:80 loop variable): part of every random-stream address; handed to
 * the launches that follow by value. */
int bdf_ctx_set_sweep(bdf_ctx *ctx, uint32_t sweep);
int bdf_ctx_advance_sweep(bdf_ctx *ctx);
/* A context on ANOTHER stream of main_ctx's device (created and owned by the library; bdf_ctx_destroy frees it), chosen so that
 * kernels on it really run beside those of main_ctx and of the contexts in `apart`: HIP multiplexes streams onto a few
 * hardware queues, and two streams that share one serialise each other (measured: 171 instead of 125 us per sweep).  A
 * timing test (two 60 us spins, together) picks among a few candidate streams; with no passing candidate the last one is
 * returned (correct, only slower).  The hyperprior of entity j is enqueued on such a context beside the rows of entity j+1. */
int bdf_ctx_create_side(bdf_ctx *main_ctx, bdf_ctx *const *apart, int n_apart, int reserved, bdf_ctx **out);
/* A row context on a stream of its own that leaves `reserve_cus` CUs (0, 8, 16, ...: whole CUs per XCD) free of its kernels
 * (hipExtStreamCreateWithCUMask); a side context created from it with reserved = 1 runs on exactly those CUs, with reserved =
 * 0 on the others.  The row sampler fills every CU it may use for the whole launch (its waves hold 468 of a SIMD's 512
 * registers): the hyperprior's small kernels, enqueued beside it, otherwise wait for slots -- measured, a one-workgroup kernel
 * beside a chip-filling one: 194 us on plain streams, 6 - 11 us on its own 16 / 8 CUs (tools/cu_mask_probe.hip).  Worth it
 * when the side work is small (MovieLens-sized entities); with reserve_cus = 0 all streams use the whole chip. */
int bdf_ctx_create_rows(int device, uint64_t seed, int reserve_cus, bdf_ctx **out);
/* Measurement support: HIP events (timing enabled) and "attach this pair to the next bdf_sample_rows launch of ctx":
 * the events ride on the row kernel's own dispatch packet (hipExtLaunchKernelGGL), so start/stop are the kernel's begin and
 * end on its stream without marker packets around it (an event pair recorded around a launch costs the stream ~6 us and
 * is counted into the interval).  bdf_event_elapsed_us waits for `stop`.  Either event may be NULL. */
int bdf_event_create(void **ev);
int bdf_event_destroy(void *ev);
int bdf_event_elapsed_us(void *start, void *stop, double *us);
int bdf_ctx_time_next_rows(bdf_ctx *ctx, void *start, void *stop);
/* the same for the hyperprior chain of ctx: `start` rides on the next bdf_hyper_sums' first kernel, `stop` on the next
 * bdf_hyper_sample's kernel */
int bdf_ctx_time_next_hyper(bdf_ctx *ctx, void *start, void *stop);
int bdf_ctx_sync(bdf_ctx *ctx);   /* waits for the stream; BDF_ERR_NOTPD if a kernel met a non-positive-definite matrix */
/* Conditions that are not errors in the reference either, accumulated by bdf_ctx_sync and returned (and cleared) here:
 * BDF_WARN_CG_MAXITER -- a conjugate-gradient column of the beta solve was still above its tolerance after maxiter iterations
 * (cg_AtA, src/parallel_cg.jl:73-93, returns such a column as it stands, silently; hosts may want to say so). */
#define BDF_WARN_CG_MAXITER 64u
int bdf_ctx_warnings(bdf_ctx *ctx, uint32_t *bits_out);
/* tuning: observations per K1 work item (rows with more are split over several wavefronts; default 192), and the size
 * of the pieces such a row is split into (default 128; set_item_size resets it to 2/3 of the item size).  Until either is set
 * (and again after set_item_size(ctx, 0)) the sizes are automatic: the defaults, and up to 2048 / 1365 for launches with
 * hundreds of waves per resident slot, where pieces only cost partial sums.  Results do not depend on them beyond the order
 * of the floating-point sums. */
int bdf_ctx_set_item_size(bdf_ctx *ctx, int observations);
/* *observations = the most observations one work item of the wave-per-row kernel takes on this context as it is set now: a row of
 * more is cut into pieces (a launch sized automatically may take larger items: rows_plan.hip, route_key) */
int bdf_ctx_item_size(const bdf_ctx *ctx, int *observations);
int bdf_ctx_set_piece_size(bdf_ctx *ctx, int observations);
/* D <= 16, an entity of one two-mode relation: rows of at most max_observations observations are sampled FOUR TO A WAVE (16 lanes
 * and a column-per-lane 16 x 16 system each) by a launch of their own when the entity has at least min_rows rows -- at such
 * D the wave-per-row kernel is bound by its per-row instruction overhead.  Defaults 48 and 8192 (environment BDF_K1_SMALL,
 * BDF_K1_SMALL_MIN_ROWS); max_observations 0 turns it off.  Same sample up to the order of the floating-point sums. */
int bdf_ctx_set_small_rows(bdf_ctx *ctx, int max_observations, int64_t min_rows);
/* D > 16, an entity of one two-mode relation (shared or per-row prior means): rows of at most max_observations observations (at most
 * 16 at num_latent <= 32, 32 above -- rows of 17 .. 32 observations two to a lane, k_rows_lr32; -1 = num_latent / 2 up to that, the
 * default; 0 = off; environment BDF_LOWRANK) are drawn by the LOW-RANK SAMPLER
 * (k_rows_lr.hip) when a launch has at least min_rows of them (default 8192, BDF_LOWRANK_MIN_ROWS) and at least half as many as
 * the opposite entity has rows (min_rows = 0: whenever there is such a row).  It replaces sample_user_basic (src/sampling.jl:200-212) for those rows by another map from
 * standard normals to the SAME conditional distribution N(inv(P_i) b_i, inv(P_i)): D + n normals of the row's stream and an
 * n x n solve instead of a D x D inverse and factorisation (P_i = Lambda + rank n).  Sampled VALUES therefore differ from the
 * reference's map for those rows (the distribution does not: oracle/bdf_oracle.c orc_sample_row_lowrank is the same function,
 * proved equal in mean and covariance to inv(P_i) b_i, inv(P_i)); max_observations = 0 restores the reference's map for
 * every row. */
int bdf_ctx_set_lowrank(bdf_ctx *ctx, int max_observations, int64_t min_rows);
/* 16 < D <= 32, an entity of ONE two-mode relation without per-observation baselines (shared or per-row prior means): its rows are
 * sampled FOUR TO A WAVE in a column-per-lane layout from the first observation to the draw (k_rows_col.hip, "K1c": 16 lanes and
 * two columns per lane for each 32 x 32 system; sample_user_basic, src/sampling.jl:200-212 -- the SAME map from the row's
 * normals to the sample as the wave-per-row kernel, equal to rounding: only the order of the floating-point sums differs).  A row
 * of more than max_piece observations is cut into 2 or 4 equal pieces on neighbouring lane rows of one wave; a row of more than
 * 4 max_piece observations spans waves.  The cut depends on the row's own length and max_piece only, so the values do not depend
 * on the launch, the shard or the number of GPUs.  Default 128 (environment BDF_K1_COL: 0 = off, n = that piece size) for
 * launches whose item size the caller has not set (bdf_ctx_set_item_size keeps the wave-per-row kernel); a call here with
 * 8..4096 applies to every launch of the context, 0 turns it off, -1 restores the default. */
int bdf_ctx_set_col_rows(bdf_ctx *ctx, int max_piece);
/* K1c at D = 32 gathers an observation's factor row from a GATHER IMAGE of the opposite entity's sample: a second copy in the order
 * the kernel's lanes read it -- a lane's two elements side by side, one 16-byte load where the sample takes two of 8
 * (k_gather_image.hip) -- which the K1c launch that sampled those rows left, or which is packed from the sample before the launch.
 * The same fused multiply-adds on the same operands: the values do not change.  on = 1 (the default) or 0: the switch the parity
 * tests compare; 2: the full image, with the two derived vectors of the rank-1 update beside the elements (no select in the loop,
 * twice the bytes: measured slower than the sample itself, kept as the measured alternative). */
int bdf_ctx_set_gather_image(bdf_ctx *ctx, int on);
/* report: out[0] K1c launches of this context that gathered from an image so far, out[1] images packed from a sample (none was
 * there, or it was stale, or the caller was not bdf_gibbs_sweep), out[2] launches that left the image of all their entity's rows */
int bdf_ctx_gather_image_stats(const bdf_ctx *ctx, int64_t out[3]);
/* parity hooks: the image the context holds of the `rows` rows at the device address `sample`, into host memory (32 doubles per
 * row, 64 for the full image; an error when it holds none that is current) | the pack kernel alone: image_dev = the image of the
 * `rows` rows of 32 doubles at `sample` */
int bdf_ctx_gather_image_read(bdf_ctx *ctx, const double *sample, int64_t rows, double *host_out);
int bdf_gather_image_pack(bdf_ctx *ctx, const double *sample, int64_t rows, double *image_dev);
/* report: how the most recent bdf_sample_rows launch of the entity with this entity_tag (all its chunks / shards since the tag's
 * previous iteration number) was dispatched on this context -- out[0] rows drawn by the low-rank sampler (k_rows_lr.hip, a
 * different map from the normals than sample_user_basic's, src/sampling.jl:200-212), out[1] rows by k_rows_small (D <= 16),
 * out[2] rows by k_rows_col (K1c), out[3] rows by the wave-per-row kernel k_rows, out[4] its work items (pieces included),
 * out[5] K1c's waves.  BDF_ERR_ARG if the context has launched no rows under that tag. */
int bdf_ctx_rows_dispatch(const bdf_ctx *ctx, uint32_t entity_tag, int64_t out[6]);
/* measurement: slot (dev, 64 pairs of uint64, each set to {~0, 0} by the caller) receives per pair s {earliest start, latest end}
 * of the waves w = s mod 64 of the NEXT K1c launch of the context, in ticks of the 100 MHz clock the XCDs share (s_memrealtime; one
 * atomic min / max per wave, sharded: one word would serialise two thousand waves): min / max over the pairs = the launch's
 * duration with no event packets around it.  bdf_gibbs_span_rows: the same for the next launch of an entity inside
 * bdf_gibbs_sweep. */
int bdf_ctx_span_next_rows(bdf_ctx *ctx, void *slot_dev);
/* parity hook: which gather path the row kernel takes.  0 = chosen by the sizes (default; env BDF_GATHER=general|wide sets the
 * initial value), 1 = the general path (any number of modes, per-observation baselines), 2 = the lean path with 64-bit row
 * offsets (num_latent > 32; what a factor matrix of 4 GiB or more needs, e.g. 10M rows at D = 64).  Same values on every path. */
int bdf_ctx_set_gather(bdf_ctx *ctx, int mode);
/* device memory for hosts without an allocator of their own (Julia); torch hosts pass tensors */
int bdf_dev_alloc(bdf_ctx *ctx, size_t bytes, void **dptr);
int bdf_dev_free(bdf_ctx *ctx, void *dptr);
/* diagnostic: the blocks, and their bytes as requested, of device and pinned host memory that the library's own objects hold in this
 * process right now -- contexts, relations, pairs, feature matrices, samplers, plans, and the temporaries of a call in flight.  Not the
 * caller's bdf_dev_alloc blocks.  Either pointer may be NULL.  What a handle took is back at its earlier value once it is destroyed. */
int bdf_dev_live(int64_t *blocks, int64_t *bytes);
int bdf_h2d(bdf_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int bdf_d2h(bdf_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);  /* synchronises */

/* ---- a1: IndexedDF / FastIDF  (src/IndexedDF.jl:10-21, 46-70) ----------------------- */
/* Host-only (needs no GPU): the IndexedDF constructor's index (IndexedDF.jl:10-19).  ids: nnz x n_modes
 * column-major, 1-based, id_bytes 4|8.  rowptr[m]: caller array of dims[m]+1 (0-based offsets);
 * rowids[m]: caller array of nnz (1-based COO row numbers, in original row order).
 * Errors: BDF_ERR_BOUNDS for an id outside 1..dims[m]. */
int bdf_index_build(int n_modes, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes,
                    int64_t *const *rowptr, int64_t *const *rowids);
/* ids: nnz x n_modes column-major, 1-based, id_bytes = 4 (Int32) or 8 (Int64); values: nnz.
 * Builds, per mode, the adjacency index in ORIGINAL COO order (bit-exact with
 * IndexedDF.index) and its device CSR.  Errors: BDF_ERR_BOUNDS for an id outside 1..dims. */
/* (A two-mode relation whose values are at most 256 distinct numbers -- ratings -- is also kept as 8-bit value codes packed
 * with the other mode's id, 4 bytes per observation and mode: the row kernel's coded variant, bit-identical results.) */
int bdf_relation_create(bdf_ctx *ctx, int n_modes, const int64_t *dims, int64_t nnz,
                        const void *ids, int id_bytes, const double *values, bdf_rel **out);
int bdf_relation_destroy(bdf_rel *rel);
/* host view of index[mode]: rowptr[dims[mode]+1] (0-based offsets) and rowids[nnz] (1-based
 * COO row numbers), for getData/getCount/getI (IndexedDF.jl:41-43, 67-70) */
int bdf_relation_index(const bdf_rel *rel, int mode, const int64_t **rowptr, const int64_t **rowids);
/* valueMean (IndexedDF.jl:26) */
int bdf_relation_value_mean(const bdf_rel *rel, double *mean);
/* host copy of the degree-descending launch order of `mode` (0-based row numbers, n = dims[mode]) */
int bdf_relation_order(const bdf_rel *rel, int mode, int32_t *order_host);

/* ---- a3-a7: latent rows ---------------------------------------------------------------
 * One relation's contribution to the rows of the entity being sampled:
 * sample_user_basic (src/sampling.jl:200-212 matrix, :215-234 tensor) and the per-relation
 * body of sample_user2 (src/sampling.jl:270-283). */
typedef struct {
    const bdf_rel *rel;
    int32_t mode;                 /* 0-based mode of the sampled entity in rel              */
    int32_t _pad;
    double alpha;                 /* rel.model.alpha                                         */
    double mean_value;            /* rel.model.mean_value                                    */
    const double *linear_values;  /* dev, nullable: rel.temp.linear_values in COO order      */
    const double *factors[BDF_MAX_MODES]; /* dev: D x N_k sample of every mode of rel; [mode] ignored */
    const double *alpha_dev;      /* dev, nullable: rel.model.alpha in device memory (sampled there, bdf_sample_alpha): read instead of `alpha` */
    /* dev, nullable (a zeroed tail is "none"): a precision weight omega_k > 0 per observation in COO order.  The observation then
     * counts with precision alpha omega_k: P_i = Lambda + alpha sum omega_k w w', b_i = Lambda mu_i + alpha sum omega_k (y - base) w.
     * Known weights, or the scale mixture of the Student-t model (bdf_robust_draw).  A call with any weighted term is sampled by
     * the wave-per-row kernel's weighted variant (k_rows_w); weights of exactly 1 give the unweighted general path's bits. */
    const double *obs_precision;
} bdf_term;

/* sample_latent_all2! (src/sampling.jl:149-172) and sample_user2_all! (:251-264):
 * for every listed row i:  P_i = Lambda + sum_r alpha_r sum_obs w w',  b_i = Lambda mu_i + sum_r alpha_r
 * sum_obs w (y - base),  out[:,i] = chol(inv(P_i))' z + inv(P_i) b_i  with z from stream
 * (BDF_P_ROW, entity_tag, i).  mu: dev, D doubles (shared prior mean) or D x N (mu_is_matrix,
 * macau.jl:103-105).  (shard, n_shards): the rows sampled are positions shard, shard + n_shards, ... of
 * bdf_relation_order(terms[0].rel, terms[0].mode) -- the reference deals rows i:P:N to its P workers
 * (sampling.jl:154); (0, 1) = every row.  out: dev D x N; only this shard's rows are written; must not
 * alias any terms[].factors[k] with k != mode.
 * prior_pack (dev, nullable): the pack bdf_hyper_sample wrote for exactly this (mu, Lambda) -- Lambda mu and Lambda
 * laid out for the row kernel; saves the small pre-launch that otherwise derives them.  Ignored with mu_is_matrix. */
int bdf_sample_rows(bdf_ctx *ctx, int D, int64_t N, int n_terms, const bdf_term *terms,
                    const double *mu, int mu_is_matrix, const double *Lambda,
                    uint32_t entity_tag, int shard, int n_shards, double *out, const double *prior_pack);
/* sample_users_blocked (src/sampling.jl:236-249): the nu users of a Block all observed the same nv items and share ONE
 * covariance inv(Lambda + alpha MM MM'), MM = factor[:, vx]: it is accumulated and factored once for the block, every user
 * then costs its right-hand side (alpha MM Yma[:, u] + Lambda mu) and two triangular solves.  vx_dev: dev nv item ids
 * (0-based); Yma: dev nv x nu column-major (values without their mean, Block.Yma); factor: dev D x M sample of the other side;
 * out: dev D x nu, column u drawn with the normals of stream (BDF_P_ROW, entity_tag, row u).  Same value as the reference's
 * expression (and as bdf_sample_rows on the block as a dense relation) for the same normals. */
int bdf_sample_block(bdf_ctx *ctx, int D, int64_t nu, int64_t nv, const int32_t *vx_dev, const double *Yma,
                     const double *factor, double alpha, const double *mu, const double *Lambda, uint32_t entity_tag,
                     double *out);
/* doubles in a prior pack for num_latent = D */
int bdf_prior_pack_doubles(int D);
/* parity hook: the deterministic part only.  P_out: dev D x D x N, b_out: dev D x N */
int bdf_row_system(bdf_ctx *ctx, int D, int64_t N, int n_terms, const bdf_term *terms,
                   const double *mu, int mu_is_matrix, const double *Lambda,
                   double *P_out, double *b_out);
/* parity hook: number of split rows (rows cut into several work items) that the launches so far left unfinished: 0 */
int bdf_rows_unfinished(bdf_ctx *ctx, int64_t *count);
/* parity hook: n standard normals per row of stream (purpose, entity_tag, row) -> dev n x n_rows */
int bdf_normals(bdf_ctx *ctx, uint32_t purpose, uint32_t entity_tag, int64_t row_begin,
                int64_t n_rows, int n, double *out);
/* parity hook: raw Philox4x32-10 block for (purpose, entity_tag, row, pair) at the current sweep */
int bdf_philox(bdf_ctx *ctx, uint32_t purpose, uint32_t entity_tag, uint64_t row, uint32_t pair,
               uint32_t out_host[4]);

/* Spike-and-slab prior of an entity's rows (csrc/k_rows_ss.hip, csrc/k_spike_hyper.hip, csrc/spike.h):
 *   u_id = s_id w_id,  s_id ~ Bernoulli(pi_d),  w_id ~ N(0, 1 / tau_d),  pi_d ~ Beta(incl_a, incl_b),  tau_d ~ Gamma(shape, rate).
 * spike_state (dev, 4 D doubles): pi (D), tau (D), logit pi (D), log tau (D).
 * bdf_sample_rows_spike: the rows of bdf_sample_rows' (shard, n_shards) under this prior.  With P_i and c_i the row system of
 * bdf_row_system for Lambda = diag(tau), mu = 0, and u the row's current value u_current[:, i] (dev, D x N), for d = 0 .. D-1 in order:
 *   lambda = P_dd,  m = (c_d - sum_{k != d} P_dk u_k) / lambda,  lo = logit pi_d + (log tau_d - log lambda) / 2 + lambda m^2 / 2,
 *   s = [U_d < 1 / (1 + exp(-lo))],  u_d = s (m + z_d / sqrt(lambda))          (an excluded loading is +0.0)
 * with z_d normal d of stream (BDF_P_ROW, entity_tag, i) and U_d the uniform of words x and y of block (BDF_P_SPIKE, entity_tag,
 * i, pair d).  out (dev, D x N): must alias neither u_current nor a factor matrix of another mode.  A lambda that is not positive
 * and finite raises the flag of a matrix that is not positive definite (bdf_ctx_sync: BDF_ERR_NOTPD).  Every row is taken by the
 * wave-per-item kernel, long rows split as bdf_sample_rows splits them. */
int bdf_sample_rows_spike(bdf_ctx *ctx, int D, int64_t N, int n_terms, const bdf_term *terms, const double *spike_state,
                          const double *u_current, uint32_t entity_tag, int shard, int n_shards, double *out);
/* The prior's hyper step from the rows in `sample` (dev, D x N): n_d = #{i : u_id != 0} (exact) and q_d = sum_i u_id^2 (blocks of
 * 256 rows in row order, then the blocks in order: independent of the launch), then with Gamma(a, 1) variates by Marsaglia-Tsang
 * on the streams (BDF_P_SPIKE_N, entity_tag, row g) and (BDF_P_SPIKE_U, the same), g = 3 d, 3 d + 1, 3 d + 2:
 *   G1 ~ Gamma(incl_a + n_d),  G2 ~ Gamma(incl_b + N - n_d),  G3 ~ Gamma(shape + n_d / 2),
 *   pi_d = G1 / (G1 + G2),  logit pi_d = log G1 - log G2,  tau_d = G3 / (rate + q_d / 2),  log tau_d
 * into spike_state.  incl_a, incl_b, shape >= 0.5 and finite, rate > 0 and finite.  Two launches on ctx's stream; not reentrant on
 * one context (the partial sums live in the context's scratch). */
int bdf_spike_hyper(bdf_ctx *ctx, int D, int64_t N, const double *sample, double incl_a, double incl_b, double shape, double rate,
                    uint32_t entity_tag, double *spike_state);
/* The running sums of the result, one call per retained draw: row_sum (dev, D x N) += [u_id != 0]; hyper_sum (dev, 3 D) += pi_d,
 * tau_d and n_d (the count of the draw: integers, exact in any order).  The caller zeroes both on ctx's stream. */
int bdf_spike_accumulate(bdf_ctx *ctx, int D, int64_t N, const double *sample, const double *spike_state, double *row_sum,
                         double *hyper_sum);

/* Non-negative prior of an entity's rows (csrc/k_nonneg.hip, csrc/nonneg.h):
 *   u_id ~ N(0, 1 / tau_d) truncated to u_id >= 0,  tau_d ~ Gamma(shape, rate).
 * tau (dev, D doubles): the prior's state.
 * bdf_sample_rows_nonneg: the rows of bdf_sample_rows' (shard, n_shards) under this prior.  With P_i and c_i the row system of
 * bdf_row_system for Lambda = diag(tau), mu = 0, and u the row's current value u_current[:, i] (dev, D x N), for d = 0 .. D-1 in order:
 *   lambda = P_dd,  m = (c_d - sum_{k != d} P_dk u_k) / lambda (k ascending),  u_d = the map of csrc/nonneg.h at (m, lambda, U_d)
 * -- the draw from N(m, 1 / lambda) truncated to [0, inf) by inversion -- with U_d the uniform of words x and y of block
 * (BDF_P_NONNEG, entity_tag, i, pair d).  No normals are drawn.  out (dev, D x N): must alias neither u_current nor a factor matrix
 * of another mode.  The rows go in chunks (bdf_ctx_set_nonneg_chunk): per chunk the wave-per-item kernel leaves the systems in the
 * context's scratch, long rows split as bdf_sample_rows splits them, and a second launch sweeps them, one lane per row.  The
 * result does not depend on the chunk size.  Relations created with a layout are not taken (one rank). */
int bdf_sample_rows_nonneg(bdf_ctx *ctx, int D, int64_t N, int n_terms, const bdf_term *terms, const double *tau,
                           const double *u_current, uint32_t entity_tag, int shard, int n_shards, double *out);
/* parity hook: the sweep alone on given systems in bdf_row_system's layout -- P (dev, D x D x n_rows), c, u_current and out (dev,
 * D x n_rows each); system i is that of original row row_begin + i (its random stream).  In chunks as bdf_sample_rows_nonneg. */
int bdf_nonneg_sweep(bdf_ctx *ctx, int D, int64_t n_rows, const double *P, const double *c, const double *u_current,
                     uint32_t entity_tag, int64_t row_begin, double *out);
/* The prior's hyper step from the rows in `sample` (dev, D x N): q_d = sum_i u_id^2 (blocks of 256 rows in row order, then the
 * blocks in order: independent of the launch), G_d ~ Gamma(shape + N / 2, 1) by Marsaglia-Tsang on the streams (BDF_P_NONNEG_N,
 * entity_tag, row d) and (BDF_P_NONNEG_U, the same), tau_d = G_d / (rate + q_d / 2) into tau (dev, D).  shape >= 0.5 and finite,
 * rate > 0 and finite.  Two launches on ctx's stream; not reentrant on one context (the partial sums live in its scratch). */
int bdf_nonneg_hyper(bdf_ctx *ctx, int D, int64_t N, const double *sample, double shape, double rate, uint32_t entity_tag,
                     double *tau);
/* The running sums of the result, one call per retained draw: row_sum (dev, D x N) += u; hyper_sum (dev, D) += tau.  The caller
 * zeroes both on ctx's stream. */
int bdf_nonneg_accumulate(bdf_ctx *ctx, int D, int64_t N, const double *sample, const double *tau, double *row_sum,
                          double *hyper_sum);
/* rows per chunk of bdf_sample_rows_nonneg and bdf_nonneg_sweep on this context; 0: the default, the most rows whose systems
 * ((D^2 + D) doubles each) stay under 1 GiB of scratch */
int bdf_ctx_set_nonneg_chunk(bdf_ctx *ctx, int64_t rows);

/* ---- a15: hyperprior  (src/sampling.jl:116-127, src/normal_wishart.jl:38-42, macau.jl:120-134) */
/* sumU (dev D) = sum_i U[:,i], UUt (dev D x D) = U U' with U = sample - uhat (uhat nullable);
 * deterministic summation order. */
int bdf_hyper_sums(bdf_ctx *ctx, int D, int64_t N, const double *sample, const double *uhat,
                   double *sumU, double *UUt);
/* Several ranks: the sums over the rows THIS rank owns (chunk c of rank p: positions [(c world + p) cmax, + cmax) of the
 * N = chunks x world x cmax rows, bdf_layout_build) and the ranks' D + D^2 partial sums gathered and added in rank order: the
 * same bits on every rank (src/sampling.jl:117-119 on the master).  comm NULL or one rank: bdf_hyper_sums. */
int bdf_hyper_sums_ranks(bdf_ctx *ctx, bdf_comm *comm, int D, int64_t N, int chunks, const double *sample, const double *uhat,
                         double *sumU, double *UUt);
/* ConditionalNormalWishart + rand(::NormalWishart): draws (mu, Lambda) on the device from the sums.
 * mu0 (dev D), Tinv (dev D x D), b0, nu: the hyper-prior AFTER the feature terms of macau.jl:124-129.
 * params_out (dev, nullable): mu_N (D) followed by inv(T_N) (D x D, the matrix sampling.jl:124 inverts)
 * for parity checks.  prior_pack_out (dev, nullable, bdf_prior_pack_doubles(D) doubles): what bdf_sample_rows needs of
 * the drawn (mu, Lambda), see there.  draws (dev, nullable): output of bdf_hyper_draws for the same arguments. */
int bdf_hyper_sample(bdf_ctx *ctx, int D, int64_t N, const double *sumU, const double *UUt,
                     const double *mu0, double b0, const double *Tinv, double nu,
                     uint32_t entity_tag, double *mu_out, double *Lambda_out, double *params_out, double *prior_pack_out,
                     const double *draws);
/* The random part of bdf_hyper_sample (Bartlett matrix D x D row-major, then the D normals of the mean: D*D + D doubles),
 * which does not depend on the rows: call it for the same (sweep, N, nu, entity_tag) before the rows are done and pass the
 * buffer as `draws` to take the gamma rejection loops off the critical path.  Same streams, same values. */
int bdf_hyper_draws(bdf_ctx *ctx, int D, int64_t N, double nu, uint32_t entity_tag, double *draws_out);

/* Store the pairs sorted by their id in `mode` (stable sort): consecutive pairs then share that mode's factor row, which
 * halves the gather traffic of bdf_predict / bdf_predict_update.  Call before the first update.  The caller's order is
 * kept wherever the interface is per pair: bdf_predict's out and the baseline are indexed through the permutation;
 * bdf_pairs_state returns the running state in STORAGE order, and bdf_pairs_order gives, for every storage position,
 * the caller's index (identity when the pairs were never sorted). */
int bdf_pairs_sort(bdf_pairs *pairs, int mode);
int bdf_pairs_order(const bdf_pairs *pairs, int64_t *orig_host);
/* per-pair baseline (dev, n doubles, borrowed; NULL to clear) that replaces mean_value in bdf_predict / bdf_predict_update for
 * these pairs: mean_value + F_test beta of pred(r, probe_vec, F) (src/sampling.jl:9-14) for a relation with features */
int bdf_pairs_set_baseline(bdf_pairs *pairs, const double *baseline);
/* link 0 (the default): predictions are udot + base; link 1 (probit): bdf_predict, bdf_predict_update, bdf_predict_sse and the
 * test update inside bdf_gibbs_sweep take p = Phi(udot + base), the probability of a 1 under the probit model, BEFORE the clamp,
 * the running average, the running sum of squares and the four statistics (kernels of their own, csrc/k_probit.hip; pairs
 * stored sorted take the general kernel).  BDF_ERR_ARG for any other value. */
int bdf_pairs_set_link(bdf_pairs *pairs, int link);
/* link 2 (logistic): p = 1 / (1 + e^-psi) for psi = udot + base >= 0 and e^psi / (1 + e^psi) otherwise, the probability of a 1 under
 * the logit model, at the same place as the probit link (kernels of their own, csrc/k_pg.hip).  An entry point of its own:
 * bdf_pairs_set_link keeps to 0 and 1 and refuses every other value, as its callers rely on; bdf_pairs_set_link(pairs, 0 | 1)
 * takes the pairs back. */
int bdf_pairs_set_logistic_link(bdf_pairs *pairs);
/* link 3 (counts): predictions are r exp(min(udot + base, 700)), the mean of the negative-binomial model with dispersion r, an
 * integer >= 1 (BDF_ERR_ARG otherwise); at the same place as the other links (csrc/k_pg.hip).  bdf_pairs_lpd_update and
 * bdf_pairs_waic_update refuse pairs with link 2 or 3 (BDF_ERR_ARG): these likelihoods are not scored yet. */
int bdf_pairs_set_count_link(bdf_pairs *pairs, double r);
/* out (dev, rows of F) = mean_value + F beta, beta dev numF: linear_values (macau.jl:91) / the baseline above */
int bdf_feat_linear(bdf_ctx *ctx, const bdf_feat *F, const double *beta, double mean_value, double *out);
/* sum over the pairs of (value - pred)^2, pred = udot + (linear_values[pair] if non-NULL else mean_value): err' err of
 * sample_alpha (macau.jl:86-87).  stats_out (dev, 4 doubles) as bdf_predict_update's; [1] is the sum.  No running state. */
int bdf_predict_sse(bdf_ctx *ctx, const bdf_pairs *pairs, int D, const double *const *factors, double mean_value,
                    const double *linear_values, double *stats_out);

/* ---- f1/f4: relation model (src/macau.jl:83-92) ---------------------------------------------- */
/* sample_alpha (src/sampling.jl:129-134): alpha ~ Wishart(alpha_nu0 + n, 1 / (1/alpha_lambda0 + sum err^2)) in one dimension.
 * sumsq_err (dev, 1 double): sum over the relation's n observations of (pred - value)^2; alpha_out (dev, 1 double).
 * Gamma stream (BDF_P_GAMMA_N/U, entity 0x800000 | rel_tag, row 0). */
int bdf_sample_alpha(bdf_ctx *ctx, double alpha_lambda0, double alpha_nu0, int64_t n, const double *sumsq_err,
                     uint32_t rel_tag, double *alpha_out);
/* sample_beta_rel (src/sampling.jl:322-337) + linear_values (macau.jl:91): relation-level side information F (one row per
 * observation, COO order), FF path (the reference has no other):
 *   beta = (alpha F'F + lambda_beta I) \ (alpha F'(values - udot - mean_value + alpha^-1/2 z1) + sqrt(lambda_beta) z2)
 *   linear_out = mean_value + F beta
 * train: the relation's observations as pairs (bdf_pairs_create on the COO ids and values); factors as for bdf_predict.
 * beta_out dev numF, linear_out dev nnz, rhs_out dev numF nullable (the right-hand side, for parity checks).
 * z1: stream (BDF_P_BETA_REL1, 0x800000 | rel_tag, row = observation), z2: (BDF_P_BETA_REL2, ..., row = feature). */
int bdf_sample_beta_rel(bdf_ctx *ctx, const bdf_feat *F, const bdf_pairs *train, int D, const double *const *factors,
                        double mean_value, double alpha, double lambda_beta, uint32_t rel_tag,
                        double *beta_out, double *linear_out, double *rhs_out);
/* The same over several ranks (the reference computes err and F'v on the master, macau.jl:83-92): rank r holds a
 * block of consecutive observations [first_obs, first_obs + n) -- F is that block of the feature matrix's rows, train the same
 * observations as pairs.  F'v and, once, F'F are summed over the ranks in rank order (bdf_sum_ranks), every rank solves the
 * numF x numF system and ends with the same beta; z1 is keyed by the observation's place in the whole relation, so the chain
 * does not depend on the number of ranks up to the summation order.  linear_out: this rank's n values (the host gathers the
 * blocks with bdf_allgather_block).  comm NULL or one rank: bdf_sample_beta_rel. */
int bdf_sample_beta_rel_ranks(bdf_ctx *ctx, bdf_comm *comm, const bdf_feat *F, const bdf_pairs *train, int64_t first_obs, int D,
                              const double *const *factors, double mean_value, double alpha, double lambda_beta, uint32_t rel_tag,
                              double *beta_out, double *linear_out, double *rhs_out);
/* x (dev, n doubles) := sum over the ranks of x, added block after block in rank order: every rank ends with the same bits
 * (the squared-error sum of sample_alpha over the ranks' blocks of observations; F'v above).  comm NULL or one rank: no-op. */
int bdf_sum_ranks(bdf_ctx *ctx, bdf_comm *comm, double *x, int64_t n);
/* Probit noise model for a 0/1 relation (neither project this one follows has it): y = 1[z > 0] with the
 * latent z ~ N(udot + mean_value, 1).  For observation k of `train` IN THE CALLER'S ORDER (the pairs may be stored sorted):
 *   m = udot_k + mean_value, s = value_k > 0.5 ? +1 : -1, t = s m, u = the uniform of stream (BDF_P_PROBIT, 0x800000 | rel_tag,
 *   row k, pair 0) at the context's sweep;  lo = Phi(-t) + u Phi(t);
 *   x = lo < 1/2 ? Phi^-1(max(lo, DBL_MIN)) : -Phi^-1(max((1 - u) Phi(t), DBL_MIN));  z = m + s x, z = s max(s z, DBL_MIN)
 * -- z drawn from N(m, 1) truncated to value_k's side of 0, always finite and strictly on that side.  linear_out (dev, n):
 * value_k - z_k, which as bdf_term.linear_values with alpha = 1 makes bdf_sample_rows draw the rows of z's Gaussian model;
 * z_out (dev, n, nullable): z_k.  factors as for bdf_predict. */
int bdf_probit_draw(bdf_ctx *ctx, const bdf_pairs *train, int D, const double *const *factors, double mean_value,
                    uint32_t rel_tag, double *linear_out, double *z_out);
/* Censored (Tobit) noise model of a Gaussian relation: observation k of `train` IN THE CALLER'S ORDER (the
 * pairs may be stored sorted) carries the flag c_k = censor_dev[k] (dev, n int8): 0 value_k is the measurement, +1 the true value
 * is at least value_k, -1 at most value_k.  The latent of a flagged observation is z ~ N(udot + mean_value, 1 / alpha) truncated
 * to its side of the bound; alpha_dev (dev, nullable) wins over alpha, which must otherwise be positive and finite:
 *   m = udot_k + mean_value, s = c_k, ra = sqrt(alpha), t = s (m - value_k) ra, u = the uniform of stream (BDF_P_CENSORED,
 *   0x800000 | rel_tag, row k, pair 0) at the context's sweep;  lo = Phi(-t) + u Phi(t);
 *   x = lo < 1/2 ? Phi^-1(max(lo, DBL_MIN)) : -Phi^-1(max((1 - u) Phi(t), DBL_MIN));
 *   z = m + s x / ra, z = value_k + s max(s (z - value_k), 0)
 * -- always finite and never on the wrong side of the bound; for t < -37.5, where Phi(t) underflows, a draw at or near the bound
 * (the exact law there lies within about 1 / (37 ra) of it).  c_k = 0: z = value_k, no uniform is consumed.  linear_out (dev, n):
 * mean_value + (value_k - z_k), which as bdf_term.linear_values makes bdf_sample_rows draw the rows of z's Gaussian model with the
 * relation's alpha (exactly mean_value for a measurement), and as the pairs' baseline makes bdf_predict_sse return the residual
 * sum of squares of z; z_out (dev, n, nullable): z_k.  Any other flag value is undefined.  factors as for bdf_predict. */
int bdf_censored_draw(bdf_ctx *ctx, const bdf_pairs *train, const int8_t *censor_dev, int D, const double *const *factors,
                      double mean_value, double alpha, const double *alpha_dev, uint32_t rel_tag, double *linear_out, double *z_out);
/* Interval-censored noise model of a Gaussian relation: observation k of `train` IN THE CALLER'S ORDER (the
 * pairs may be stored sorted) carries the bounds lo_k = bounds_dev[2 k] <= hi_k = bounds_dev[2 k + 1] (dev, n pairs of doubles,
 * row-major, aligned to 16 bytes; either bound may be infinite).  lo_k == hi_k: value_k is the measurement, z = value_k, no uniform
 * is consumed.  lo_k < hi_k: the latent is z ~ N(udot + mean_value, 1 / alpha) truncated to [lo_k, hi_k]; alpha_dev (dev,
 * nullable) wins over alpha, which must otherwise be positive and finite:
 *   m = udot_k + mean_value, ra = sqrt(alpha), a = (lo_k - m) ra, b = (hi_k - m) ra, u = the uniform of stream (BDF_P_INTERVAL,
 *   0x800000 | rel_tag, row k, pair 0) at the context's sweep;
 *   a + b > 0 (false for NaN):  (a, b, v, v', s) = (-b, -a, 1 - u, u, -1),  else  (a, b, u, 1 - u, +1);
 *   Pa = Phi(a), w = Phi(b) - Pa, p = Pa + v w;
 *   x = p < 1/2 ? Phi^-1(max(p, DBL_MIN)) : -Phi^-1(max(Phi(-b) + v' w, DBL_MIN));
 *   z = min(max(m + s x / ra, lo_k), hi_k)
 * -- always finite for finite value_k and inside the bounds; with both bounds beyond 37.5 standard deviations on one side of m,
 * where Phi underflows, the nearer bound (the exact law there lies within about 1 / (37 ra) of it).  linear_out (dev, n):
 * mean_value + (value_k - z_k), which as bdf_term.linear_values makes bdf_sample_rows draw the rows of z's Gaussian model with the
 * relation's alpha (exactly mean_value for a measurement), and as the pairs' baseline makes bdf_predict_sse return the residual
 * sum of squares of z; z_out (dev, n, nullable): z_k.  lo_k > hi_k or a NaN bound is undefined.  factors as for bdf_predict. */
int bdf_interval_draw(bdf_ctx *ctx, const bdf_pairs *train, const double *bounds_dev, int D, const double *const *factors,
                      double mean_value, double alpha, const double *alpha_dev, uint32_t rel_tag, double *linear_out, double *z_out);
/* Robust (Student-t) noise model of a Gaussian relation (csrc/k_robust.hip, csrc/robust.h):
 *   value_k ~ N(udot_k + mean_value, 1 / (alpha omega_k)),  omega_k ~ Gamma(nu / 2, rate nu / 2)
 * -- value_k is Student-t with nu degrees of freedom and scale alpha^-1/2.  For observation k of `train` IN THE CALLER'S ORDER (the
 * pairs may be stored sorted), with e_k = value_k - mean_value - udot_k, the conditional draw is
 *   omega_k = 2 G_k / (nu + alpha e_k^2),  G_k ~ Gamma((nu + 1) / 2, 1) by Marsaglia-Tsang: d = (nu + 1) / 2 - 1/3, c = 1 / sqrt(9 d);
 *   attempt t = 0, 1, ...: x = normal 2 t of stream (BDF_P_ROBUST_N, 0x800000 | rel_tag, row k), v = (1 + c x)^3 (an attempt with
 *   1 + c x <= 0 is skipped), u = the uniform of (BDF_P_ROBUST_U, the same entity and row, pair t); accepted when
 *   u < 1 - 0.0331 x^4 or log u < x^2 / 2 + d (1 - v + log v); then G_k = d v (after 256 refusals: d)
 * at the context's sweep.  nu >= 1 and finite, so the shape is at least 1.  alpha_dev (dev, nullable) wins over alpha, which must
 * otherwise be positive and finite.  precision_out (dev, n): omega_k, what bdf_term.obs_precision takes.  wsse_out (dev, 1 double,
 * nullable): sum_k omega_k e_k^2 added in a fixed order (bit-identical reruns) -- with it in place of the sum of squares,
 * bdf_sample_alpha draws from alpha's exact conditional.  factors as for bdf_predict.  Not reentrant on one context (the
 * partial sums live in the context's scratch). */
int bdf_robust_draw(bdf_ctx *ctx, const bdf_pairs *train, int D, const double *const *factors, double mean_value, double alpha,
                    const double *alpha_dev, double nu, uint32_t rel_tag, double *precision_out, double *wsse_out);
/* *out (dev, 1 double) = sum_k weights[k] (value_k - mean_value - udot_k)^2 over the pairs, weights (dev, n) in the caller's order,
 * added in the same fixed order: sample_alpha's sum of squares for a relation with known weights (no draw). */
int bdf_pairs_weighted_sse(bdf_ctx *ctx, const bdf_pairs *pairs, int D, const double *const *factors, double mean_value,
                           const double *weights, double *out);
/* Polya-Gamma noise models (csrc/k_pg.hip, csrc/pg.h; Polson, Scott & Windle 2013): with psi_k = udot_k +
 * mean_value a cell's likelihood is (e^psi)^a / (1 + e^psi)^b, and given omega_k ~ PG(b, psi_k) it is a Gaussian pseudo-observation
 * kappa / omega_k of psi_k with precision omega_k, kappa = a - b / 2:
 *   model 1, logit:   value_k in {0, 1}, P(1) = 1 / (1 + e^-psi);                      b = 1,           kappa = value_k - 1/2;
 *   model 2, counts:  value_k = 0, 1, 2, ... negative binomial with mean r e^psi,      b = value_k + r, kappa = (value_k - r) / 2,
 *                     pmf proportional to p^y (1 - p)^r at p = 1 / (1 + e^-psi); r an integer >= 1 (BDF_ERR_ARG otherwise).
 * For observation k of `train` IN THE CALLER'S ORDER (the pairs may be stored sorted) at the context's sweep:
 *   precision_out[k] = omega_k,  linear_out[k] = mean_value + value_k - kappa / omega_k
 * (both dev, n) -- bdf_term.obs_precision and bdf_term.linear_values of the relation's terms, with alpha = 1: the rows are then
 * sampled by the weighted row kernel unchanged.  omega_k is finite and strictly positive for every finite psi_k, and linear_out[k]
 * is finite for every finite value_k.  The values are the caller's contract (the Python setters check them; this entry point does
 * not read them on the host): for a value_k that is negative or no integer under model 2, b is held at 1 and its integer part taken,
 * which keeps the outputs finite and means nothing.
 * The stream: purpose BDF_P_PG, entity 0x800000 | rel_tag, row k; the cell takes its random numbers through ONE cursor over the
 * stream's blocks pair = 0, 1, 2, ... (the pair index is 16 bits wide and wraps).  Every request takes one whole block (x, y, z, w),
 * with U1 = u01(x, y) and U2 = u01(z, w) the block's two doubles:
 *   a uniform:          U1                         an exponential:  -log U1
 *   two exponentials:   -log U1, -log U2           a normal:        sqrt(-2 log U1) cos(2 pi U2)  (normal 2 pair of the stream)
 * PG(1, c) = X / 4 with X ~ J*(1, z = |c| / 2) by Devroye's method, t = 0.64, K = pi^2 / 8 + z^2 / 2,
 * p = pi / (2 K) e^(-K t), q = 2 e^-z [Phi((t z - 1) / sqrt t) + exp(2 z + log Phi(-(t z + 1) / sqrt t))].  A proposal takes a
 * uniform u; u (p + q) < p: X = t + E / K (an exponential); else for t z < 1: two exponentials E, E' per candidate until
 * E^2 <= 2 E' / t, X = t / (1 + t E)^2, kept when a uniform is at most e^(-z^2 X / 2); else per candidate a normal N, Y = N^2,
 * X = mu + mu^2 Y / 2 - mu sqrt(4 mu Y + mu^2 Y^2) / 2 (mu = 1 / z), replaced by mu^2 / X when a uniform exceeds mu / (mu + X), until
 * X <= t.  Then a uniform V, S = a_0(X), y = V S and the alternating series a_n(x) = pi (n + 1/2) (2 / (pi x))^(3/2)
 * e^(-2 (n + 1/2)^2 / x) (x <= t), pi (n + 1/2) e^(-(n + 1/2)^2 pi^2 x / 2) (x > t): odd n subtracts a_n and accepts when y <= S, even n
 * adds it and refuses the proposal when y > S.  PG(b, c), b <= 170: the sum of b such draws on the same cursor.  b > 170: ONE
 * normal N, omega = max(m + sqrt(v) N, DBL_MIN) with PG(b, c)'s mean m = b / (2 c) tanh(c / 2) and variance v = b / (4 c^3)
 * (sinh c - c) sech^2(c / 2) -- an approximation (as BayesLogit's hybrid sampler above the same b).
 * The bounds: after 256 candidates of a truncated inverse Gaussian the last candidate stands, held at t; after 64 partial sums of
 * the series the proposal is accepted; after 256 refused proposals the last proposal is returned.  factors as for bdf_predict. */
int bdf_pg_draw(bdf_ctx *ctx, const bdf_pairs *train, int D, const double *const *factors, double mean_value, int model, double r,
                uint32_t rel_tag, double *precision_out, double *linear_out);
/* A noise precision per row of one entity of a Gaussian relation (csrc/k_entity_noise.hip,
 * csrc/entity_noise.h): a cell whose id in mode `mode` (0-based) of `rel` is j is observed with precision alpha tau_j,
 *   value_k ~ N(udot_k + mean_value, 1 / (alpha tau_j(k))),  tau_j ~ Gamma(shape, rate) (mean shape / rate).
 * `train` holds the cells of `rel` as pairs, observation k of the caller's order being COO row k of the relation (the pairs may be
 * stored sorted); BDF_ERR_ARG when the counts or the numbers of modes differ, and for a relation created with a layout.  With
 * e_k = value_k - (udot_k + mean_value), n_j the cells of row j and S_j the sum of e_k^2 over them, added in the fixed order that
 * csrc/entity_noise.h writes down (a row without cells: S_j = 0, a draw from the prior):
 *   tau_j = G_j / (rate + alpha S_j / 2),  G_j ~ Gamma(a, 1), a = shape + n_j / 2, by Marsaglia-Tsang on the streams (BDF_P_NOISE_N,
 *   0x800000 | rel_tag, row j) and (BDF_P_NOISE_U, the same entity and row) as bdf_robust_draw states it; a < 1: G_j is the variate
 *   of a + 1 times u^(1 / a), u the uniform of pair 0xffff
 * at the context's sweep.  shape and rate positive and finite.  alpha_dev (dev, nullable) wins over alpha, which must otherwise be
 * positive and finite.  tau_out (dev, dims[mode]): tau_j.  precision_out (dev, n; scratch of the first launch, which leaves e_k^2
 * there): tau_j(k) in the caller's order, bit for bit tau_out[j(k)] -- what bdf_term.obs_precision takes.  wsse_out (dev, 1 double,
 * nullable): sum_j tau_j S_j in a fixed order (bit-identical reruns): with it in place of the sum of squares bdf_sample_alpha
 * draws from alpha's exact conditional.  factors as for bdf_predict.  Two launches (a third for wsse_out) on ctx's stream; not
 * reentrant on one context (the partial sums live in the context's scratch). */
int bdf_entity_noise_draw(bdf_ctx *ctx, const bdf_rel *rel, int mode, const bdf_pairs *train, int D, const double *const *factors,
                          double mean_value, double alpha, const double *alpha_dev, double shape, double rate, uint32_t rel_tag,
                          double *tau_out, double *precision_out, double *wsse_out);

/* Row and column biases of a relation's entities (csrc/k_bias.hip, csrc/bias.h): with B the biased modes,
 *   value_k ~ N(mean_value + sum over m in B of b^m_(id_m(k)) + udot_k, 1 / alpha),  b^m_j ~ N(0, 1 / lambda_m),  lambda_m ~ Gamma(shape_m, rate_m).
 * A term names one biased mode (0-based), its prior and where its state lives: bias (dev, dims[mode] doubles) and lambda (dev, 1
 * double; the caller starts it, at shape / rate say).  Terms may be listed in any order; they are taken in rising mode order. */
typedef struct {
    int32_t mode;
    int32_t _pad;
    double shape, rate;
    double *bias;
    double *lambda;
} bdf_bias_term;
/* One Gibbs step on the biases of `rel`, whose cells `train` holds as pairs (observation k of the caller's order being COO row k
 * of the relation; the pairs may be stored sorted; their baseline is not read); BDF_ERR_ARG when the counts or the numbers of
 * modes differ, for a relation created with a layout, for a mode out of range or listed twice and for a shape or rate that is
 * not positive and finite.  At the context's sweep:
 *   1. e_k = value_k - (udot_k + mean_value) into resid_scratch (dev, n doubles), the same bits as value_k - bdf_predict's output;
 *   2. per biased mode m in rising order and row j with n_j cells: S_j = the sum over its cells of e_k minus the other biased
 *      modes' current biases (subtracted in rising mode order; a mode drawn earlier in this call with its new value), added in the
 *      fixed order csrc/bias.h writes down; prec_j = lambda_m + alpha n_j and b^m_j = alpha S_j / prec_j + z_j / sqrt(prec_j), z_j
 *      normal m of stream (BDF_P_BIAS, 0x800000 | rel_tag, row j); a row without cells draws from its prior;
 *   3. lambda_m = G / (rate_m + sum_j (b^m_j)^2 / 2), G ~ Gamma(shape_m + dims[m] / 2, 1) by Marsaglia-Tsang on the streams
 *      (BDF_P_BIAS_N, 0x800000 | rel_tag, row m) and (BDF_P_BIAS_U, the same), the sum in a fixed order; drawn on the device.  The
 *      rows of step 2 read the lambda_m the call found;
 *   4. linear_out[k] = mean_value + the biases of cell k added in rising mode order (dev, n doubles, the caller's order): what
 *      bdf_term.linear_values and bdf_pairs_set_baseline take.
 * alpha_dev (dev, nullable) wins over alpha, which must otherwise be positive and finite.  factors as for bdf_predict.  Bit-identical
 * reruns.  2 + 2 n_bias launches on ctx's stream; not reentrant on one context (the partial sums live in the context's scratch). */
int bdf_bias_draw(bdf_ctx *ctx, const bdf_rel *rel, const bdf_pairs *train, int D, const double *const *factors, double mean_value,
                  double alpha, const double *alpha_dev, uint32_t rel_tag, int n_bias, const bdf_bias_term *terms, double *resid_scratch,
                  double *linear_out);
/* out_dev[k] = mean_value + the biases of pair k added in rising mode order, for any pairs over the same entities (dev, n doubles,
 * the caller's order): the baseline of test pairs or of probe cells.  Of a term only mode and bias are read. */
int bdf_bias_baseline(bdf_ctx *ctx, const bdf_pairs *pairs, int n_bias, const bdf_bias_term *terms, double mean_value, double *out_dev);

/* Ordinal probit noise model (csrc/k_ordinal.hip, csrc/ordinal.h): the training values of a relation are
 * levels 1 .. K (4 <= K <= 16), y = k iff e_{k-1} <= z < e_k for the latent z ~ N(udot + mean_value, 1 / alpha) of the interval
 * model, with e_0 = -inf, e_K = +inf, e_1 = 1.5 and e_{K-1} = K - 1/2 fixed and the K - 3 edges between them sampled under a
 * uniform prior on their order.  The object keeps the edges (they start at k + 1/2), the step size sigma (it starts at `step`, in
 * [1e-8, 10]), two counters and a trace of trace_capacity rows (at most 2^24) of K - 1 edges, all on the device. */
int bdf_ordinal_create(bdf_ctx *ctx, int K, double step, int64_t trace_capacity, bdf_ordinal **out);
int bdf_ordinal_destroy(bdf_ordinal *ord);
/* One Metropolis step on the edges with z integrated out, then the rows' bounds; four launches on ctx's stream, no synchronisation.
 * With the gaps g_k = e_{k+1} - e_k (k = 1 .. K-2), R = e_{K-1} - e_1 and theta_k = log(g_k / g_{K-2}) (k = 1 .. K-3):
 *   theta'_k = theta_k + sigma eps_k, eps_k = normal k of stream (BDF_P_ORDINAL, 0x800000 | rel_tag, row 0) at the context's sweep;
 *   w = (exp theta'_1, ..., exp theta'_{K-3}, 1), g' = R w / sum w, e'_k = e_1 + g'_1 + ... + g'_{k-1};
 *   S = sum over the pairs of [M(m; e'_{y-1}, e'_y) - M(m; e_{y-1}, e_y)] + sum_k log g'_k - sum_k log g_k, M the log mass of
 *   bdf_pairs_lpd_update, m = udot + mean_value (NOT the pairs' baseline), y = codes_dev[k] (dev, one int8 per pair IN THE CALLER'S
 *   ORDER); a pair whose two edges did not move -- levels 1 and K always -- adds an exact 0; the sum is taken in a fixed order;
 *   accepted iff log u < S, u the uniform of stream (BDF_P_ORDINAL, 0x800000 | rel_tag, row 1, pair 0); a proposal with a gap
 *   g' <= 1e-6 is refused outright (S reads -inf): a truncation of the prior, there because equal edges would read as "a
 *   measurement" to bdf_interval_draw.
 * adapt 1: after the i-th step of the object, log sigma += (accepted - 0.3) / sqrt(i), sigma kept in [1e-8, 10]; 0: sigma stays;
 * -1: as 1 while fewer steps than bdf_ordinal_set_adapt stated have been taken, as 0 afterwards (decided on the device).
 * The current edges are appended to the trace (row = steps taken before this one) while it has room.  bounds_dev (dev, n pairs of
 * doubles in the caller's order, aligned to 16 bytes): rewritten to (e_{y-1}, e_y) when the proposal was accepted, untouched
 * otherwise -- the caller starts it from the edges k + 1/2.  alpha_dev (dev, nullable) wins over alpha. */
int bdf_ordinal_step(bdf_ctx *ctx, bdf_ordinal *ord, const bdf_pairs *train, const int8_t *codes_dev, int D, const double *const *factors,
                     double mean_value, double alpha, const double *alpha_dev, uint32_t rel_tag, int adapt, double *bounds_dev);
/* how many steps of the object adapt under adapt = -1 (the burn-in's length; 0 at creation) */
int bdf_ordinal_set_adapt(bdf_ordinal *ord, int64_t steps);
/* bounds_out[k] = (e_{y-1}, e_y) for y = codes_dev[k], k < n, from the current edges (test cells: their bins under this draw's
 * edges); enqueued on ctx's stream, which the caller orders against the stream of the steps. */
int bdf_ordinal_bounds(bdf_ctx *ctx, const bdf_ordinal *ord, const int8_t *codes_dev, int64_t n, double *bounds_out);
/* Waits for the stream of the last step, then: edges (K - 1 doubles e_1 .. e_{K-1}), sigma, the counters, the last step's S, and
 * the first trace_rows rows of the trace (rows no step has written are NaN).  Every output is nullable.  BDF_ERR_ARG when
 * trace_rows exceeds the capacity. */
int bdf_ordinal_read(bdf_ordinal *ord, double *edges, double *sigma, int64_t *proposals, int64_t *accepts, double *last_S,
                     double *trace, int64_t trace_rows);
/* The last step's proposal after the same wait: the proposed e'_1 .. e'_{K-1}, the Jacobian term, whether it was accepted
 * (1 / 0) and the log of its uniform.  Every output is nullable.  Beyond what a sampler needs, and part of the interface on
 * purpose: it is how a step is held against a restatement term by term (bdf_ordinal_read gives only S and the outcome), the
 * way z_out of the latent draws is, and what a caller looks at when a chain's acceptance rate surprises. */
int bdf_ordinal_proposal(bdf_ordinal *ord, double *edges, double *jacobian, int *accepted, double *log_u);


/* ---- f2: test-set prediction (src/sampling.jl:9-45, macau.jl:142-203, 231-241) -------- */
/* ids: n x n_modes column-major 1-based (test_vec[:,1:end-1]); values: n (test_vec[:,end]) */
int bdf_pairs_create(bdf_ctx *ctx, int n_modes, int64_t n, const void *ids, int id_bytes,
                     const double *values, bdf_pairs **out);
int bdf_pairs_destroy(bdf_pairs *p);
/* pred(r, test_vec) = udot + mean_value -> out (dev n) */
int bdf_predict(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors,
                double mean_value, double *out);
/* pred_all(r) (src/sampling.jl:91-97; macau.jl:145-147 accumulates it into predictions_full): udot over EVERY cell of the relation
 * + mean_value.  dims: n_modes (2 .. 4) sizes; factors[k]: dims[k] x D row-major (dev); out (dev): prod(dims) doubles, the cell
 * (i_1, ..., i_n) at ((i_1 dims[1] + i_2) dims[2] + ...) + i_n -- the last mode fastest. */
int bdf_predict_all(bdf_ctx *ctx, int n_modes, const int64_t *dims, int D, const double *const *factors,
                    double mean_value, double *out);
/* one macau.jl:142-203 reporting step: p = pred; phase 0 (burn-in): avg = p; phase 1 (first
 * posterior sample): avg = p, sq = p^2, count = 1; phase 2: running mean / sum of squares.
 * stats_out (dev 4 doubles): sum (y-clamp(avg))^2, sum (y-clamp(p))^2, #correct(avg), #correct(p).
 * clamp_lo > clamp_hi means no clamping. */
int bdf_predict_update(bdf_ctx *ctx, bdf_pairs *p, int D, const double *const *factors,
                       double mean_value, int phase, double clamp_lo, double clamp_hi,
                       double class_cut, double *stats_out);
/* running state: avg (dev n), sq (dev n) */
int bdf_pairs_state(const bdf_pairs *p, double **avg, double **sq, int64_t *n);

/* ---- held-out log pointwise predictive density (csrc/k_lpd.hip, csrc/lpd.h) ----------- */
/* One scoring step on the pairs: l_k = log p(value_k | the rows in `factors`, alpha), the log-likelihood of pair k's kind of
 * record, with m = udot_k + (the pairs' baseline | mean_value), ra = sqrt(alpha), L = log Phi:
 *   pairs with the probit link (bdf_pairs_set_link 1):   l = L(value_k > 1/2 ? m : -m); bounds_dev must be NULL (BDF_ERR_ARG);
 *   bounds_dev NULL, or lo_k == hi_k:                     l = log(alpha / 2 pi) / 2 - alpha (value_k - m)^2 / 2;
 *   lo_k < hi_k (either may be infinite):                 l = log(Phi(b) - Phi(a)), a = (lo_k - m) ra, b = (hi_k - m) ra, taken in
 *     the lower tail (a + b > 0: (a, b) = (-b, -a)) and, where b <= -37, from the asymptotic form of L -- finite wherever a < b
 *     as doubles, 0 for (-inf, +inf).
 * bounds_dev (dev, nullable): n pairs (lo_k, hi_k) in the caller's order, row-major, aligned to 16 bytes; lo_k > hi_k or a NaN
 * bound is undefined.  alpha_dev (dev, nullable) wins over alpha, which must otherwise be positive and finite (ignored with the
 * probit link).  The running state, two doubles per pair that the pairs own (allocated at the first phase >= 1, freed by
 * bdf_pairs_destroy) and a draw counter of its own, is a streaming log-sum-exp:
 *   phase 0 (burn-in): no state is touched, lpd_k = l_k;   phase 1: (M, A) = (l, 1), draws = 1;
 *   phase 2: M' = max(M, l), A = A exp(M - M') + exp(l - M'), M = M', draws += 1;   lpd_k = M + log A - log(draws).
 * stats_out (dev 4 doubles): sum_k l_k of this draw, sum_k lpd_k after it, 0, 0 -- summed in a fixed order (bit-identical
 * reruns).  Enqueued on ctx's stream.  BDF_ERR_ARG for a phase outside 0..2 and for phase 2 before a phase 1. */
int bdf_pairs_lpd_update(bdf_ctx *ctx, bdf_pairs *p, const double *bounds_dev, int D, const double *const *factors,
                         double mean_value, double alpha, const double *alpha_dev, int phase, double *stats_out);
/* A precision scale per row of one mode for bdf_pairs_lpd_update (the per-row noise model, bdf_entity_noise_draw): with tau_dev (dev,
 * one double per row of mode `mode`, 0-based; BORROWED, read at every update) pair k is scored with alpha tau_dev[id_k,mode] in place
 * of alpha, as a Gaussian measurement and as the mass of an interval alike.  NULL clears it (mode is then ignored) and the
 * updates are bit for bit what they were.  BDF_ERR_ARG for a mode outside the pairs' and for pairs with the probit link.
 * bdf_pairs_waic_update refuses pairs with a scale (BDF_ERR_ARG): WAIC under that model is not scored yet. */
int bdf_pairs_set_precision_scale(bdf_pairs *pairs, const double *tau_dev, int mode);
/* lpd_k = M + log A - log(draws) of every pair -> out_dev (dev n), in the caller's order whether or not the pairs are stored
 * sorted.  BDF_ERR_ARG before the first phase 1. */
int bdf_pairs_lpd(bdf_ctx *ctx, const bdf_pairs *p, double *out_dev);

/* ---- WAIC on the training cells (csrc/k_waic.hip, csrc/lpd.h) -------------------------- */
/* One scoring step of the widely applicable information criterion on the pairs (the training table): l_k as
 * bdf_pairs_lpd_update forms it -- the same arguments, kinds of record, refusals and phases -- with ONE difference: given
 * bounds_dev, m = udot_k + mean_value and the pairs' baseline is not read (the training pairs of a censored, interval or ordinal
 * relation carry the latent draw as their baseline; without bounds_dev the baseline stands for mean_value as everywhere).  The
 * running state, four doubles per pair that the pairs own (allocated and zeroed on ctx's stream at the first phase >= 1, freed
 * by bdf_pairs_destroy; separate from bdf_pairs_lpd_update's) and a draw counter of its own, is the streaming log-sum-exp (M, A)
 * of bdf_pairs_lpd_update and Welford's (mean, M2) of l:
 *   phase 0 (burn-in): no state is touched, lppd_k = l_k, V_k = 0;   phase 1: (M, A, mean, M2) = (l, 1, l, 0), draws = 1;
 *   phase 2: draws += 1, (M, A) as bdf_pairs_lpd_update, d = l - mean, mean += d / draws, M2 += d (l - mean);
 *   lppd_k = M + log A - log(draws), V_k = M2 / (draws - 1) (0 while draws < 2).
 * stats_out (dev 4 doubles): sum_k l_k of this draw, sum_k lppd_k after it, sum_k V_k after it, the number of pairs with
 * V_k > 0.4 -- summed in a fixed order (bit-identical reruns).  Enqueued on ctx's stream. */
int bdf_pairs_waic_update(bdf_ctx *ctx, bdf_pairs *p, const double *bounds_dev, int D, const double *const *factors,
                          double mean_value, double alpha, const double *alpha_dev, int phase, double *stats_out);
/* The end of the run.  out_dev (dev, nullable, aligned to 16 bytes): n rows (lppd_k, V_k) in the caller's order whether or not
 * the pairs are stored sorted.  stats_out (dev 4 doubles), from two fixed-order passes: sum_k lppd_k, sum_k V_k,
 * sum_k (elpd_k - e)^2 with elpd_k = lppd_k - V_k and e the mean of elpd_k that the first pass gives, the number of pairs with
 * V_k > 0.4.  (se = sqrt of [2]: n times the population variance of elpd_k.)  BDF_ERR_ARG before the first phase 1. */
int bdf_pairs_waic(bdf_ctx *ctx, const bdf_pairs *p, double *out_dev, double *stats_out);

/* ---- cells of rows that were not in training (csrc/k_newrows.hip, csrc/newrows.h) ------ */
/* Given one posterior draw (mu, Lambda, beta, V, alpha) of an entity with side information, the factor of a NEW row with features
 * f is u* ~ N(uhat, Lambda^-1), uhat = mu + beta' f (bdf_uhat on the new rows' features with mu_matrix_out), and it is integrated
 * out of a cell (i*, j) in closed form -- nothing is drawn:
 *   identity link:  y | draw ~ N(m, q_j + 1 / alpha),   m = mean_value + uhat_i* . v_j,   q_j = v_j' Lambda^-1 v_j;
 *   probit link:    P(y = 1 | draw) = Phi(m / sqrt(1 + q_j)).
 * bdf_newrows_quad: q_out[j] (dev M) = |L^-1 v_j|^2 for every row j of V_dev (dev, M rows of D doubles) with Lambda_dev (dev D x D,
 * symmetric; its lower triangle is read) = L L', factorised once per call by one wavefront; the products run on
 * v_mfma_f64_16x16x4_f64 and a row's squares are added in a fixed order (bit-identical reruns, q >= 0 by construction, error
 * ~ D eps cond(Lambda)).  Any D in 1..BDF_MAX_D.  A Lambda that is not positive definite raises BDF_ERR_NOTPD at the next
 * bdf_ctx_sync (q_out then holds NaNs).  Enqueued on ctx's stream; no host copy, no synchronisation. */
int bdf_newrows_quad(bdf_ctx *ctx, int D, int64_t M, const double *Lambda_dev, const double *V_dev, double *q_out);
/* One prediction step on the new cells.  pairs: two modes, the first mode's ids index the rows of uhat_new_dev (dev, n* rows of D
 * doubles), the second mode's the rows of V_dev and of q_dev (bdf_newrows_quad's output); the last column is the held-out value, NaN
 * where it is unknown.  Pairs with the probit link (bdf_pairs_set_link 1) take the probit form and ignore alpha; links 2 and 3, a
 * baseline and a precision scale are refused (BDF_ERR_ARG).  alpha_dev (dev, nullable) wins over alpha, which must otherwise be
 * positive and finite.  Per cell: the prediction p = m (identity) or the probability above (probit) and, with score_lpd != 0 and a
 * finite value, l = log N(value; m, q + 1 / alpha) or log Phi(+- m / sqrt(1 + q)) by the maps of bdf_pairs_lpd_update.  The
 * running state, five doubles per cell that the pairs own (allocated and zeroed on ctx's stream at the first phase >= 1, freed by
 * bdf_pairs_destroy) and a draw counter of its own: Welford's (mean, M2) of p, the sum of q, the streaming log-sum-exp (M, A) of l.
 *   phase 0 (burn-in): no state is touched;   phase 1: (mean, M2, sum q, M, A) = (p, 0, q, l, 1), draws = 1;
 *   phase 2: draws += 1, d = p - mean, mean += d / draws, M2 += d (p - mean), sum q += q, (M, A) as bdf_pairs_lpd_update.
 * stats_out (dev 8 doubles), over the cells with a finite value, summed in a fixed order (bit-identical reruns):
 *   [0] sum (value - clamp(mean))^2 (phase 0: of this draw's p), [1] sum (value - clamp(p))^2, [2] / [3] the cells whose label
 *   value < class_cut agrees with mean < class_cut / p < class_cut (clamp_lo > clamp_hi: no clamping, as bdf_predict_update),
 *   [4] their count, [5] sum lpd = M + log A - log(draws) after this draw (phase 0: of l), [6] sum l of this draw, [7] 0;
 *   [5] and [6] are 0 without score_lpd.  Cells with a NaN value are predicted and left out of every scalar.
 * Enqueued on ctx's stream; no host copy, no synchronisation.  BDF_ERR_ARG for a phase outside 0..2, for phase 2 before a phase 1
 * and for a score_lpd that differs from the phase 1 call's. */
int bdf_newrows_update(bdf_ctx *ctx, bdf_pairs *pairs, int D, const double *uhat_new_dev, const double *V_dev, const double *q_dev,
                       double mean_value, double alpha, const double *alpha_dev, int phase, double clamp_lo, double clamp_hi,
                       double class_cut, int score_lpd, double *stats_out);
/* out_dev (dev, n rows of 3 doubles, in the caller's order whether or not the pairs are stored sorted): pred = mean;
 * stdev = sqrt(M2 / (draws - 1) + sum q / draws), the posterior sd of the cell's noise-free value (probit: sqrt(M2 / (draws - 1)),
 * of its probability), NaN below two draws; lpd = M + log A - log(draws), NaN without score_lpd and for a NaN value.
 * BDF_ERR_ARG before the first phase 1. */
int bdf_newrows_result(bdf_ctx *ctx, const bdf_pairs *pairs, double *out_dev);
/* (parity hook, as bdf_pairs_state) *state_dev = the running state, five planes of n doubles in STORAGE order -- mean, M2, sum q, M,
 * A -- or NULL before the first phase 1; *draws = the posterior draws it holds */
int bdf_newrows_state(const bdf_pairs *pairs, double **state_dev, double *draws);

/* ---- new rows conditioned on a few cells of their own: the fold-in (csrc/k_foldin.hip) ------ */
/* Given the same draw, a new row i with prior mean mu_i (mu, or mu + beta' f_i with mu_is_matrix: bdf_uhat's mu_matrix_out) whose
 * cells K_i are known has u* | draw, y* ~ N(uhat_i, P_i^-1) with the row system of bdf_row_system,
 *   P_i = Lambda + alpha sum_{j in K_i} v_j v_j',  b_i = Lambda mu_i + alpha sum_{j in K_i} (y_ij - mean_value) v_j,  uhat_i = P_i^-1 b_i,
 * and the cell (i, j) is y | draw ~ N(m, q_ij + 1 / alpha), m = mean_value + uhat_i . v_j, q_ij = v_j' P_i^-1 v_j.  The new row's
 * cells do not feed back into V (the standard fold-in).  A row without a known cell is bdf_newrows_quad's cold row.
 * bdf_foldin_cells: known: ONE term of a two-mode relation of the known cells (created once: dims n_new x M with known->mode = 0, or
 * the other way round), whose other-mode factor is this draw's V (dev, M rows of D doubles) and whose alpha / alpha_dev is the
 * draw's precision; mu (dev, D doubles, or n_new rows of D with mu_is_matrix) and Lambda (dev, D x D) as bdf_row_system's.  The
 * systems come from the row sampler's own accumulation (long rows split and summed as bdf_sample_rows does), the new rows in chunks
 * of bdf_ctx_set_nonneg_chunk's size -- by default the most whose systems stay under the scratch cap of bdf_sample_rows_nonneg --
 * and the result does not depend on the chunk size, bit for bit.  cells: two modes, stored sorted by the new row
 * (bdf_pairs_sort(cells, 0)), the first mode's ids in 1..n_new, the second's in 1..M (checked at the first call: BDF_ERR_BOUNDS).
 * Per new row a workgroup of four waves: one factorises P_i and solves for uhat_i, then all take the row's cells 64 at a time, one
 * lane per cell.
 * m_out, q_out (dev, n doubles each): m and q_ij per cell in the pairs' STORAGE order -- what bdf_newrows_update_cells takes;
 * uhat_out (dev, n_new rows of D doubles): uhat_i of every new row, also of those without a cell.  Any D in 1..BDF_MAX_D.  A P_i
 * that is not positive definite raises BDF_ERR_NOTPD at the next bdf_ctx_sync and leaves NaN in the row's uhat_i, m and q.
 * Enqueued on ctx's stream; no host copy, no synchronisation (the first call uploads the cells' row offsets). */
int bdf_foldin_cells(bdf_ctx *ctx, int D, int64_t n_new, const bdf_term *known, const double *mu, int mu_is_matrix, const double *Lambda,
                     bdf_pairs *cells, double mean_value, double *m_out, double *q_out, double *uhat_out);
/* parity hook: the second half alone on given systems in bdf_row_system's layout -- P (dev, D x D x n_new, every entry of the
 * symmetric matrix) and b (dev, D x n_new), system i that of new row i -- against V (dev, M rows of D doubles) */
int bdf_foldin_solve(bdf_ctx *ctx, int D, int64_t n_new, const double *P, const double *b, bdf_pairs *cells, int64_t M, const double *V,
                     double mean_value, double *m_out, double *q_out, double *uhat_out);
/* bdf_newrows_update on (m, q) per cell (dev, n doubles each, the pairs' STORAGE order: bdf_foldin_cells' output) instead of the
 * gather from uhat, V and q_j.  From there on the two are one text (csrc/newrows.h): the link, the fold, the phases, stats_out and
 * its fixed-order sum, the running state and its counter, which bdf_newrows_result and bdf_newrows_state read for both; the same
 * refusals.  Fed the (m, q_j) of a cold row it leaves the state and the scalars of bdf_newrows_update, bit for bit. */
int bdf_newrows_update_cells(bdf_ctx *ctx, bdf_pairs *pairs, const double *m_dev, const double *q_dev, double alpha, const double *alpha_dev,
                             int phase, double clamp_lo, double clamp_hi, double class_cut, int score_lpd, double *stats_out);

/* ---- AUC_ROC (src/ROC.jl:1-11) and vecnorm on the device (csrc/k_auc.hip) ------------ */
/* bytes of the workspace bdf_auc_roc needs for n scores (-1: n < 0) */
int64_t bdf_auc_workspace_bytes(int64_t n);
/* AUC_ROC(labels, scores) over n scores, every pointer a device pointer: labels n bytes (nonzero = positive), scores n
 * doubles, workspace bdf_auc_workspace_bytes(n) bytes.  The scores are sorted stably (ties keep the caller's order; -0.0 ties
 * with +0.0; NaNs sort last and tie among themselves) and C = the number of (negative, positive) pairs with the negative sorted
 * first, an exact integer; *auc_out = C / (P Nn) with P positives and Nn negatives, NaN when P = 0 or Nn = 0.  counts_out
 * (nullable, 3 int64): {C, P, Nn}.  Enqueued on the context's stream; n < 2^31 - 4096. */
int bdf_auc_roc(bdf_ctx *ctx, int64_t n, const uint8_t *labels, const double *scores, void *workspace, double *auc_out,
                int64_t *counts_out);
/* roc_avg of macau.jl:200: AUC_ROC(values .< class_cut, -avg) over the pairs' running average, in the caller's order (sorted
 * pairs break ties by the caller's index).  The pairs own the workspace (allocated at first use, freed by bdf_pairs_destroy).
 * Enqueued on ctx's stream: pass the context whose stream ran the prediction update (bdf_gibbs_contexts' pred for the native
 * iteration) to have it ordered after that update.  auc_out (dev 1 double), counts_out as bdf_auc_roc's. */
int bdf_pairs_auc(bdf_ctx *ctx, bdf_pairs *p, double class_cut, double *auc_out, int64_t *counts_out);
/* *out (dev 1 double) = ||x||_2 of x (dev n doubles), the squares summed in a fixed order (bit-identical reruns) */
int bdf_norm2(bdf_ctx *ctx, int64_t n, const double *x, double *out);

/* ---- a8-a14: side information (Entity.F operator contract) ------------- */
/* dense: F host N x numF column-major (RelationData.jl:66-90 `F`) */
int bdf_feat_create_dense(bdf_ctx *ctx, int64_t m, int64_t n, const double *F, bdf_feat **out);
/* SparseMatrixCSR (src/parallel_csr.jl:36-54): COO triplets, 1-based */
int bdf_feat_create_csr(bdf_ctx *ctx, int64_t m, int64_t n, int64_t nnz, const int32_t *rows,
                        const int32_t *cols, const double *vals, bdf_feat **out);
/* SparseBinMatrixCSR / SparseBinMatrix (src/sparsebin_csr.jl:22-37, src/parallel_matrix.jl:19-24):
 * implicit 1.0 values; 1-based Int32 rows/cols */
int bdf_feat_create_bin(bdf_ctx *ctx, int64_t m, int64_t n, int64_t nnz, const int32_t *rows,
                        const int32_t *cols, bdf_feat **out);
int bdf_feat_destroy(bdf_feat *f);
/* Several GPUs store an entity's rows at internal positions (bdf_layout_build), and the rows of its F with them.
 * row_ids_host (m entries, nullable to clear): the ORIGINAL id of every row of F (negative: a row nobody owns, all zero) --
 * it keys the per-row noise of bdf_sample_beta (E1, src/sampling.jl:298-300), so that beta does not depend on the layout. */
int bdf_feat_set_row_ids(bdf_feat *f, const int32_t *row_ids_host);
int bdf_feat_size(const bdf_feat *f, int64_t *m, int64_t *n, int64_t *nnz);
/* F*B (transpose=0: B n x ncol -> out m x ncol) or At_mul_B(F,B) (transpose=1: B m x ncol -> out
 * n x ncol); B, out dev column-major (RelationData.jl:314-329, parallel_matrix.jl:520-561) */
int bdf_feat_mul(bdf_ctx *ctx, const bdf_feat *f, const double *B, int ncol, double *out, int transpose);
/* AtA_mul_B! for ncol vectors at once: out = (F'F + lambda I) X (src/parallel_cg.jl:7-14) */
int bdf_feat_AtA_mul(bdf_ctx *ctx, const bdf_feat *f, const double *X, int ncol, double lambda, double *out);
/* uhat = (F beta)' : D x N (F_mul_beta, RelationData.jl:314-320; macau.jl:103,112) and, if
 * mu_matrix_out != NULL, mu_matrix = mu .+ uhat (macau.jl:104,113) */
int bdf_uhat(bdf_ctx *ctx, const bdf_feat *f, int D, const double *beta, const double *mu,
             double *uhat_out, double *mu_matrix_out);
/* hyper-prior feature terms (macau.jl:124-129): Tinv_out = WI + beta' beta * lambda_beta */
int bdf_hyper_feature_terms(bdf_ctx *ctx, int D, int64_t numF, const double *beta, const double *WI,
                            const double *lambda_beta_dev, double *Tinv_out);
/* sample_beta + update_beta! (src/sampling.jl:291-312, 361-370): rhs = F'((sample - mu)' + E1) +
 * sqrt(lb) E2; beta = (F'F + lb I) \ rhs by Cholesky of FF (use_ff, solve_full :314-320) or D
 * simultaneous cg_AtA solves (solve_cg2, parallel_matrix.jl:488-507; cg_AtA parallel_cg.jl:63-94)
 * with per-column stopping ||r|| < tol ||b||, maxiter (<=0: numF).  tol NaN => eps()*numF.
 * lambda_beta lives on the device (lambda_beta_dev, 1 double) so that sample_lambda_beta
 * (sampling.jl:136-142; nu, mu hyper-parameters; enabled by sample_lambda) can update it in place.
 * rhs_out (dev numF x D, nullable), iters_out (dev int32 D, nullable). */
int bdf_sample_beta(bdf_ctx *ctx, const bdf_feat *f, int D, const double *sample, const double *mu,
                    const double *Lambda, double *lambda_beta_dev, int use_ff, double tol, int maxiter,
                    int sample_lambda, double lb_nu, double lb_mu, uint32_t entity_tag,
                    double *beta_out, double *rhs_out, int32_t *iters_out);

/* ---- multi-GPU: rows of every entity shared out over the ranks, exchanged after sampling ---------------------------------
 * The reference: sample_latent_all2! deals the rows i:P:N to P workers and ships every factor matrix to every worker in
 * every call (src/sampling.jl:154-171, remotecall_fetch(sample_latent_range_ref, ...)).  Here: one process per GPU; every
 * rank holds a replica of every factor matrix, the observations of ITS rows only, and after sampling its rows of an entity
 * takes part in one in-place all-gather per chunk.
 *
 * bdf_layout_build (host-only): internal row positions of an entity.  Rows in falling order of `degree` (stable; the
 * observations of the row over all the entity's relations) are dealt round-robin to the ranks, a rank's rows round-robin to
 * `chunks` chunks; row i of chunk c of rank p sits at pos = (c * world + p) * cmax + i.  The factor matrix of the entity then
 * has chunks * world * cmax rows (rows nobody owns stay zero), chunk c of it is one contiguous rank-major region.
 * pos_out: N entries; *cmax_out = ceil(ceil(N / world) / chunks). */
int bdf_layout_build(int64_t N, const int64_t *degree, int world, int chunks, int32_t *pos_out, int64_t *cmax_out);
/* bdf_relation_create with a layout per mode (pos[m], cmax[m] from bdf_layout_build with the same world and chunks): the
 * index is the full IndexedDF index as ever; the DEVICE holds only the observations of the rows `rank` owns, addressed by
 * internal positions.  bdf_sample_rows on such a relation takes (shard, n_shards) = (chunk, chunks), N = chunks * world *
 * cmax, writes the rows at their internal positions and keys every row's random stream by its ORIGINAL id, so that the
 * chain does not depend on the number of GPUs (up to the summation order of the hyperprior's sums). */
int bdf_relation_create_sharded(bdf_ctx *ctx, int n_modes, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes,
                                const double *values, const int32_t *const *pos, const int64_t *cmax, int rank, int world,
                                int chunks, bdf_rel **out);
/* The communicator.  RCCL transport: rank 0 calls bdf_comm_unique_id (128 bytes) and hands the id to the other ranks by
 * whatever channel the host has (Julia: its cluster manager; Python: torch.distributed's store); librccl.so is resolved with
 * dlopen at the first call.  Host transport (test rigs with several ranks on one GPU, where RCCL refuses to run): the block is
 * staged through host memory and `fn` -- recv = world blocks of bytes_per_rank, rank-major -- does the exchange. */
#define BDF_COMM_ID_BYTES 128
int bdf_comm_unique_id(void *id_out);
int bdf_comm_create(bdf_ctx *ctx, int rank, int world, const void *unique_id, bdf_comm **out);
typedef int (*bdf_exchange_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank);
int bdf_comm_create_host(bdf_ctx *ctx, int rank, int world, bdf_exchange_fn fn, void *user, bdf_comm **out);
int bdf_comm_destroy(bdf_comm *comm);
int bdf_comm_size(const bdf_comm *comm, int *rank, int *world);
/* LARGE exchanges by DIRECT ALL-PAIRS COPIES over the point-to-point xGMI links instead of RCCL's ring -- the GPU-side answer to
 * the reference shipping the whole sample matrix to every worker (src/sampling.jl:155-171): every rank exports the allocation its
 * block lives in (hipIpcGetMemHandle), opens its peers', and an exchange of bytes_per_rank >= min_bytes is world - 1 concurrent
 * device-to-device copies, one per link, pulled from the owners' mappings (configuration C4 on 8 GPUs: 640 MB per link per users'
 * half-sweep, ~4.2 ms, where a ring moves 7 x 640 MB through one link after the other).  ORDERED ON THE DEVICE: the owner records
 * an interprocess event behind its row kernel, every peer's copy stream waits for it, the caller's stream waits for the copies in
 * bdf_allgather_join -- no stream is synchronised, the next chunk's rows run beside the copies.  `fn` is the host's all-gather
 * (as for bdf_comm_create_host): it carries a control message per rank and exchange (handle, offset, an error code the ranks
 * agree on) and orders the host CALLS (record before wait), nothing else.  Taken by bdf_allgather_rows only (rotating buffers:
 * bdf_comm.hip); added to a communicator of either kind; bdf_comm_disable_peer takes it off again (collectively: every rank or
 * none).  bdf_comm_peer_selftest (collective): one exchange this way whatever its size, complete on return -- what a host runs
 * before it lets the rows take the path.  Exchanges made this way and the bytes this rank pulled: bdf_comm_peer_stats.
 * Unmeasured on several GPUs; tested with two processes on one. */
int bdf_comm_enable_peer(bdf_comm *comm, bdf_exchange_fn fn, void *user, size_t min_bytes);
int bdf_comm_disable_peer(bdf_comm *comm);
int bdf_comm_peer_selftest(bdf_ctx *ctx, bdf_comm *comm, void *buf, size_t bytes_per_rank);
int bdf_comm_peer_stats(const bdf_comm *comm, int64_t *exchanges, int64_t *bytes_pulled);
/* Exchange of chunk `chunk` of the N x D factor matrix `sample` (dev; N = chunks * world * cmax rows, the layout above): an
 * in-place all-gather of the ranks' blocks (ncclAllGather), ordered after the work enqueued so far on ctx's stream, run on
 * the communicator's own stream -- the row kernel of the next chunk runs beside it.  bdf_allgather_join: ctx's stream waits
 * for every exchange enqueued so far. */
int bdf_allgather_rows(bdf_ctx *ctx, bdf_comm *comm, int D, int64_t N, double *sample, int chunk, int chunks);
int bdf_allgather_join(bdf_ctx *ctx, bdf_comm *comm);
/* the same for any buffer of world equal blocks (dev; rank r's block at buf + r * bytes_per_rank) */
int bdf_allgather_block(bdf_ctx *ctx, bdf_comm *comm, void *buf, size_t bytes_per_rank);
/* bdf_sample_beta on several ranks: solve_cg2 shares the D conjugate-gradient solves out over its workers
 * (src/parallel_matrix.jl:488-507); here every rank forms the right-hand side, solves a contiguous block of ceil(D / world)
 * columns and the blocks (with their iteration counts) are all-gathered: beta, lambda_beta and iters_out end up identical on
 * every rank and equal to the single-rank result.  comm NULL or one rank, or use_ff: exactly bdf_sample_beta. */
int bdf_sample_beta_ranks(bdf_ctx *ctx, bdf_comm *comm, const bdf_feat *f, int D, const double *sample, const double *mu,
                          const double *Lambda, double *lambda_beta_dev, int use_ff, double tol, int maxiter,
                          int sample_lambda, double lb_nu, double lb_mu, uint32_t entity_tag,
                          double *beta_out, double *rhs_out, int32_t *iters_out);

/* ---- background cells: implicit feedback (csrc/k_background.hip) ------------------------------------
 * Every cell of a two-mode N x M relation that is not listed observes a background value with precision alpha c0, c0 below every
 * listed cell's weight omega_k.  With rb = value - mean_value, G = V V' and s = sum_j v_j over ALL M rows of the other entity, row
 * i's conditional is that of an ordinary row whose prior is (Lambda_eff, mu_eff_i) = (Lambda + alpha c0 G, Lambda_eff^-1 (Lambda
 * mu_i + alpha c0 rb s)) and whose listed cells count with weight omega_k - c0 and residual (omega_k r_k - c0 rb) / (omega_k - c0). */
typedef struct {
    const double *sum;            /* dev, D: s, the sum of the other entity's rows (what bdf_hyper_sums leaves in sumU)        */
    const double *gram;           /* dev, D x D: G, their Gram matrix (what bdf_hyper_sums leaves in UUt)                      */
    double alpha;                 /* the relation's precision ...                                                              */
    const double *alpha_dev;      /* ... or, nullable, where it lives on the device (sampled there): read instead of `alpha`  */
    double weight;                /* c0, in (0, 1]                                                                             */
    double resid;                 /* rb = background value - mean_value                                                        */
} bdf_background_term;
/* The effective prior of an entity with n_bg (1 .. BDF_MAX_TERMS) background relations, one workgroup on ctx's stream:
 *   Lambda_out (dev, D x D) = Lambda + sum_k alpha_k c0_k G_k   (added in the order of bg[])
 *   mu_out = Lambda_out^-1 (Lambda mu + sum_k alpha_k c0_k rb_k s_k): dev D doubles for a shared prior mean; with mu_is_matrix
 *   mu and mu_out are D x N and a second launch forms mu_out_i = W mu_i + w0, W = Lambda_out^-1 Lambda, on the matrix cores
 *   prior_pack_out (dev, nullable, bdf_prior_pack_doubles(D) doubles; NULL with mu_is_matrix): the pack of (mu_out, Lambda_out) as
 *   bdf_hyper_sample writes it for its draw, bit for bit what bdf_sample_rows derives itself when it is given none
 *   alpha_rows_out (dev, n_bg doubles): alpha_k (1 - c0_k) -- bdf_term.alpha_dev of a relation whose listed cells all have weight 1,
 *   which then stays on the unweighted row kernels with values y' = mean + (r - c0 rb) / (1 - c0).
 * Lambda_out may not alias Lambda nor mu_out mu.  A Lambda_out that is not positive definite sets the context's row-system flag
 * (BDF_ERR_NOTPD at the next bdf_ctx_sync). */
int bdf_background_prior(bdf_ctx *ctx, int D, int64_t N, int n_bg, const bdf_background_term *bg, const double *mu, int mu_is_matrix,
                         const double *Lambda, double *Lambda_out, double *mu_out, double *prior_pack_out, double *alpha_rows_out);
/* *out (dev, 1 double) = sum over ALL N M cells of c e^2, for sample_alpha with n = N M, from the listed cells alone:
 *   sum_listed [omega_k e_k^2 - c0 (rb - psi_k)^2] + c0 [N M rb^2 - 2 rb (sum U).(sum V) + <U U', V V'>],   psi = u.v, e = y - mean - psi
 * train: the listed cells as pairs (two modes), factors as for bdf_predict; weights (dev, nullable: 1): omega_k in the caller's
 * order; value, weight: the background's; sumU, gramU, sumV, gramV (dev): bdf_hyper_sums of factors[0] (N rows) and factors[1] (M
 * rows).  The gather and the fixed summation order of bdf_pairs_weighted_sse: bit-identical reruns.  Not reentrant on one context. */
int bdf_background_sse(bdf_ctx *ctx, const bdf_pairs *train, int D, const double *const *factors, double mean_value,
                       const double *weights, double value, double weight, const double *sumU, const double *gramU,
                       const double *sumV, const double *gramV, int64_t N, int64_t M, double *out);

/* ---- dense relations (csrc/k_dense.hip, csrc/dense.h) ------------------------------------------------------
 * A two-mode relation whose N x M cells are ALL observed is kept as R (dev, N x M doubles row-major, r_ij = y_ij - mean_value)
 * and is never listed.  With V the other entity's rows, G = V'V and C = R V, row i's conditional is that of an ordinary row whose
 * prior is (Lambda_eff, mu_eff_i) = (Lambda + alpha G, Lambda_eff^-1 (Lambda mu_i + alpha C_i)) and that has no cells of the relation.
 *
 * out = R F (dev, N x D row-major; F: dev M x D row-major), or with `transpose` out = R' F (M x D; F: N x D), on the f64 matrix
 * cores from the one copy of R.  D in 1 .. BDF_MAX_D; rows and columns past N, M, D are predicated off.  Every element is summed in
 * a fixed order: bit-identical reruns.  One launch on ctx's stream. */
int bdf_dense_product(bdf_ctx *ctx, const double *R, int64_t N, int64_t M, int D, const double *F, int transpose, double *out);
typedef struct {
    const double *gram;           /* dev, D x D: the Gram matrix of the other entity's rows (what bdf_hyper_sums leaves in UUt)  */
    const double *C;              /* dev, N x D row-major: a dense term's rows of R V (bdf_dense_product); NULL: a background term */
    const double *sum;            /* dev, D: a background term's sum of the other entity's rows; NULL: a dense term              */
    double alpha;                 /* the relation's precision ...                                                              */
    const double *alpha_dev;      /* ... or, nullable, where it lives on the device (sampled there): read instead of `alpha`  */
    double weight;                /* 1 for a dense term; c0 of a background term, in (0, 1]                                    */
    double resid;                 /* a background term's rb = background value - mean_value                                    */
} bdf_dense_term;
/* The effective prior of an entity with at least one dense relation among its n_terms (1 .. BDF_MAX_TERMS) dense and background
 * terms, two launches on ctx's stream:
 *   Lambda_out (dev, D x D) = Lambda + sum_k alpha_k weight_k G_k   (added in the order of terms[])
 *   mu_out (dev, D x N: ALWAYS one mean per row) = Lambda_out^-1 (Lambda mu_i + sum_dense alpha_k C_k,i + sum_background alpha_k c0_k
 *   rb_k s_k); mu is D doubles, or D x N with mu_is_matrix.  Waves of one launch factor Lambda_out and solve for the columns of Lambda_out^-1 (and
 *   Lambda_out^-1 Lambda), every solve refined once; the rows then take two products on the matrix cores.
 *   alpha_rows_out (dev, n_terms doubles): alpha_k of a dense term, alpha_k (1 - c0_k) of a background term (bdf_background_prior).
 * Lambda_out may not alias Lambda nor mu_out mu.  A Lambda_out that is not positive definite sets the context's row-system flag
 * (BDF_ERR_NOTPD at the next bdf_ctx_sync).  Not reentrant on one context (the solves live in the context's scratch). */
int bdf_dense_prior(bdf_ctx *ctx, int D, int64_t N, int n_terms, const bdf_dense_term *terms, const double *mu, int mu_is_matrix,
                    const double *Lambda, double *Lambda_out, double *mu_out, double *alpha_rows_out);
/* *out (dev, 1 double) = sum over ALL N M cells of (r_ij - u_i.v_j)^2 = sum_r2 - 2 sum_i u_i.C_i + <U'U, V'V>, for sample_alpha with
 * n = N M.  U (dev, N x D), C = R V of the same (U, V) (bdf_dense_product), gramU, gramV (dev, D x D: bdf_hyper_sums of both
 * entities), sum_r2 = the sum of r_ij^2 over the listed cells, which does not change, holes_r2 (dev, nullable: 0) the same over the
 * holes as bdf_dense_impute left it.  Fixed summation order; two launches; not reentrant on one context. */
int bdf_dense_sse(bdf_ctx *ctx, int D, int64_t N, const double *U, const double *C, const double *gramU, const double *gramV,
                  double sum_r2, const double *holes_r2, double *out);
/* The cells of a dense relation that are not listed are holes: latent values of the augmented model, drawn before alpha and the rows
 * of every iteration.  holes: their (i, j) as pairs (two modes; the values are not read); for hole k in the caller's order
 *   R[i M + j] = u_i.v_j + z_k / sqrt(alpha),   z_k normal 0 of stream (BDF_P_DENSE, 0x800000 | rel_tag, row k) at the context's sweep
 * with alpha read from alpha_dev when it is given.  stats_out (dev, 4 doubles): [0] the sum of the new r^2 over the holes, in a
 * fixed order; the rest 0.  No hole: stats_out is zeroed.  A hole outside N x M is skipped.  Not reentrant on one context. */
int bdf_dense_impute(bdf_ctx *ctx, const bdf_pairs *holes, int D, const double *const *factors, double alpha, const double *alpha_dev,
                     uint32_t rel_tag, double *R, int64_t N, int64_t M, double *stats_out);

/* ---- top-K lists per row from the posterior mean score (csrc/k_recommend.hip, csrc/recommend.h) ---------
 * A bdf_scores object keeps sum[i, j] = sum over the pushed draws of u_i . v_j for n_rows scored rows of the first entity and all M
 * rows of the second, n_rows x M doubles row-major, and a ring of `batch` (1 .. 32) slots of draws that are not in the sum yet.
 * Everything is enqueued on ctx's stream.  rows_dev (dev, nullable: the rows 0 .. n_rows - 1): the 0-based row of U of every scored
 * row, copied.  BDF_ERR_HIP with N, M and the byte count in bdf_last_error() when the device memory does not suffice. */
typedef struct bdf_scores bdf_scores;
int bdf_scores_create(bdf_ctx *ctx, int64_t n_rows, int64_t M, int D, int batch, const int32_t *rows_dev, bdf_scores **out);
int bdf_scores_destroy(bdf_scores *sc);
/* this draw's factors (dev; U: N x D row-major, read at the scored rows only; V: M x D) into the next slot of the ring; a full ring
 * is flushed */
int bdf_scores_push(bdf_scores *sc, const double *U, const double *V);
/* the buffered draws into the sum, on v_mfma_f64_16x16x4_f64: every cell's chain starts from the stored sum and runs over the draws
 * in push order, d in ascending blocks of four -- the sum's bits depend neither on `batch` nor on where the flushes fall */
int bdf_scores_flush(bdf_scores *sc);
/* flush, then per scored row the K (1 .. 64) best columns by score = sum / draws + mean_value, the larger score first, equal scores
 * by the smaller column; rel (nullable): the columns listed in the row of this two-mode relation (its first mode's device CSR, at
 * the row's id) are left out.  items_out (dev, n_rows x K int32): 1-based column ids, 0 behind the row's last candidate; scores_out
 * (dev, n_rows x K doubles): their scores, NaN where items_out is 0.  No draws: no candidates */
int bdf_scores_topk(bdf_scores *sc, const bdf_rel *rel, int K, double mean_value, int32_t *items_out, double *scores_out);
/* recall@K, NDCG@K and hit rate of the lists `items` (dev, what bdf_scores_topk wrote) on the held-out cells `test` (two modes) with
 * value > class_cut, means over the scored rows that have such a cell, added in a fixed order; out (dev, 4 doubles): recall, ndcg,
 * hit_rate, the count of those rows.  The relevant cells are indexed by row on the host at the first call */
int bdf_scores_metrics(bdf_scores *sc, const int32_t *items, int K, const bdf_pairs *test, double class_cut, double *out);
/* parity hooks: flush, then copy `count` doubles between the sum (from cell `first`; the sum is followed by 64 doubles of NaN that
 * nothing writes) and buf_dev -- write != 0: into the sum; and the count of draws that scores are divided by */
int bdf_scores_copy(bdf_scores *sc, double *buf_dev, int64_t first, int64_t count, int write);
int bdf_scores_set_draws(bdf_scores *sc, double draws);

/* ---- acquisition lists per row from the moments of u.v over the draws (csrc/k_acquire.hip, csrc/acquire.h) -
 * A bdf_acquire object keeps, for n_rows scored rows of the first entity and all M rows of the second, the planes mean[i, j] and
 * M2[i, j] -- the running mean of u_i . v_j over the pushed draws and the running sum of its squared deviations (Welford) -- and,
 * with want_prob, psum[i, j] = sum over the draws of Phi(sqrt(alpha_b) (u_i . v_j + mean_value - threshold)): n_rows x M doubles
 * each, row-major, every plane followed by 64 doubles of NaN that nothing writes; a fourth plane of that shape holds the scores of
 * the last list; and a ring of `batch` (1 .. 32) slots of draws that are not in the planes yet.  Everything is enqueued on ctx's
 * stream.  rows_dev as for bdf_scores_create.  mean_value and (with want_prob) threshold must be finite.  BDF_ERR_HIP with N, M and
 * the byte count in bdf_last_error() when the device memory does not suffice. */
typedef struct bdf_acquire bdf_acquire;
int bdf_acquire_create(bdf_ctx *ctx, int64_t n_rows, int64_t M, int D, int batch, const int32_t *rows_dev, int want_prob,
                       double mean_value, double threshold, bdf_acquire **out);
int bdf_acquire_destroy(bdf_acquire *ac);
/* this draw's factors (as for bdf_scores_push) and its noise precision into the next slot of the ring; a full ring is flushed.
 * alpha_dev (dev, nullable) wins over alpha, which must otherwise be positive and finite: the value is stored into the slot by the
 * device and never read on the host */
int bdf_acquire_push(bdf_acquire *ac, const double *U, const double *V, double alpha, const double *alpha_dev);
/* the buffered draws into the planes: per draw, in push order, p = u.v on v_mfma_f64_16x16x4_f64 from zero accumulators (d in
 * ascending blocks of four), then with the draw's count n: delta = p - mean; mean += delta / n; M2 += delta (p - mean); psum += Phi(.)
 * -- the planes' bits depend neither on `batch` nor on where the flushes fall */
int bdf_acquire_flush(bdf_acquire *ac);
/* flush, then per scored row the K (1 .. 64) best columns by the acquisition score over the n pushed draws, ordered and padded as
 * bdf_scores_topk's lists, the columns listed in `rel` (nullable) left out.  With m = mean + mean_value and
 * sd = sqrt(M2 / (n - 1)): rule 0 (ucb) m + kappa sd, kappa >= 0 and finite; rule 1 (sd) sd; rule 2 (prob_above, want_prob only)
 * psum / n.  n < 2: no candidates for ucb and sd; n < 1: none for prob_above.  mean_out, sd_out, prob_out (dev, nullable, n_rows x K
 * doubles): m, sd and psum / n at the listed items, NaN where items_out is 0 */
int bdf_acquire_topk(bdf_acquire *ac, const bdf_rel *rel, int K, int rule, double kappa, int32_t *items_out, double *scores_out,
                     double *mean_out, double *sd_out, double *prob_out);
/* parity hooks: flush, then copy `count` doubles between plane 0 (mean), 1 (M2), 2 (psum) or 3 (the last list's scores), from cell
 * `first` (the plane's guard included), and buf_dev -- write != 0: into the plane; and the count of draws n */
int bdf_acquire_copy(bdf_acquire *ac, int plane, double *buf_dev, int64_t first, int64_t count, int write);
int bdf_acquire_set_draws(bdf_acquire *ac, double draws);

/* ---- convergence diagnostics of held-out predictions (csrc/k_diag.hip) -------------------------------------
 * A bdf_diag object keeps every pushed draw of the predictions of n_cells pairs, and of n_scalars (0, 1 or 2) scalars beside them,
 * in one plane of capacity x (n_cells + n_scalars) doubles, draw-major: a row holds the cells in the pairs' STORAGE order, then
 * scalar 0, this draw's sum over the cells of (value - prediction)^2, then scalar 1, its alpha.  From the series down the plane's
 * columns come, per series, the split R-hat, the effective sample size by Geyer's initial monotone sequence and the Monte Carlo
 * standard error of the mean, as section 32 defines them; a series with a value that is not finite or with no variance within
 * its halves gives three NaN.  BDF_ERR_HIP with the byte count in bdf_last_error() when the device memory does not suffice. */
typedef struct bdf_diag bdf_diag;
int bdf_diag_create(bdf_ctx *ctx, int64_t n_cells, int n_scalars, int64_t capacity, bdf_diag **out);
int bdf_diag_destroy(bdf_diag *diag);
/* this draw into the next row, on ctx's stream: every pair's prediction exactly as bdf_predict forms it (the pairs' baseline and link
 * included), the sum of (value - prediction)^2 added in a fixed order and, with two scalars, alpha (alpha_dev, dev and nullable, wins
 * over alpha, which must otherwise be positive and finite).  BDF_ERR_ARG when the plane is full or the pairs' n is not n_cells */
int bdf_diag_push(bdf_ctx *ctx, bdf_diag *diag, const bdf_pairs *pairs, int D, const double *const *factors, double mean_value,
                  double alpha, const double *alpha_dev);
/* parity hooks: row `draw` (0-based, below the capacity) from values_dev (dev, n_cells + n_scalars doubles) on the stream of the
 * context the object was created on -- the plane then holds at least draw + 1 draws; and the plane's address and the draws it holds */
int bdf_diag_write(bdf_diag *diag, int64_t draw, const double *values_dev);
int bdf_diag_plane(const bdf_diag *diag, double **dev_ptr, int64_t *draws);
/* the statistics of the draws held (at least 4), on ctx's stream.  out_dev (dev, nullable): n_cells x 3 doubles, (R-hat, ESS, MCSE)
 * of every cell at the caller's index orig_dev[storage position] (dev int32, nullable: the storage order itself).  stats_out (dev,
 * 6 + 3 n_scalars doubles): over the cells that have figures the largest R-hat and the smallest ESS (NaN when none has), how many
 * have R-hat > rhat_cut, how many ESS < ess_cut, how many cells have none (three NaN), the draws; then (R-hat, ESS, MCSE) per scalar.
 * The counts are whole numbers: nothing of the output depends on the grid or on an order of reduction */
int bdf_diag_compute(bdf_ctx *ctx, const bdf_diag *diag, const int32_t *orig_dev, double rhat_cut, double ess_cut, double *out_dev,
                     double *stats_out);

/* ---- a2: one Gibbs iteration enqueued from native code (src/macau.jl:80-203; relation-level side information and alpha
 * sampling excepted: those iterations are enqueued step by step through the entry points above) ------------------------
 * rows of every entity (+ exchange) -> hyperpriors -> test-set prediction update, on three streams (rows: ctx's; the other
 * two are created here, chosen so that they really run beside it).  Hand-overs: events on the kernels' own dispatch
 * packets; and -- when ctx came from bdf_ctx_create_rows with CUs set aside, one rank, BDF_NO_POLL unset -- the row kernels
 * poll a per-entity word the hyperprior draw publishes instead of the row stream waiting for the draw's event.
 * The host pays one call per iteration.  `sweep` numbers key the random streams only: they need not increase. */
typedef struct {
    int64_t N;                    /* rows of the factor matrix (the entity's count; chunks * world * cmax with a layout)   */
    int64_t n_real;               /* the entity's count (N of ConditionalNormalWishart, src/sampling.jl:117)             */
    uint32_t tag;                 /* entity tag of the random streams (1-based entity number)                             */
    int32_t n_terms;              /* relations the entity takes part in                                                    */
    struct {
        const bdf_rel *rel;
        int32_t mode;             /* 0-based mode of this entity in rel                                                    */
        int32_t entity_of_mode[BDF_MAX_MODES];   /* which entity (index into the array) every mode of rel is                */
        double alpha, mean_value;
    } terms[BDF_MAX_TERMS];
    double *sample[3];            /* dev, D x N each: the rows rotate through three buffers; [0] holds the current rows      */
    double *mu, *Lambda, *mu0, *WI, *sumU, *UUt, *params /*nullable*/, *prior_pack, *draws;   /* dev, as in bdf_hyper_sample */
    double b0, nu0;
    /* side information of the entity (Entity.F; NULL: none -- a zeroed tail of the struct is "no features").  With it the
     * iteration runs uhat = (F beta)' and the per-row prior means before the entity's rows (macau.jl:103-104), the feature
     * terms in its hyperprior (macau.jl:124-129) and update_beta! after the rows of every entity (macau.jl:138-140) */
    const bdf_feat *feat;
    double *beta;                 /* dev, numF x D                                                                          */
    double *uhat, *mu_matrix;     /* dev, D x N each                                                                        */
    double *Tinv;                 /* dev, D x D: WI + beta' beta lambda_beta                                                */
    double *lambda_beta;          /* dev, 1                                                                                 */
    int32_t *cg_iters;            /* dev, D (nullable)                                                                      */
    int32_t use_ff;               /* (F'F + lambda I) \ rhs directly (numF <= compute_ff_size) or by conjugate gradients    */
    int32_t sample_lambda_beta, full_lambda_u;
    int32_t _pad;
    double tol;                   /* NaN: eps() * numF                                                                      */
    double lb_nu, lb_mu;          /* hyper-parameters of sample_lambda_beta (Entity.nu, Entity.mu)                          */
    /* an entity with a background relation (a zeroed tail is "none"; bdf_gibbs_relation.bg_weight): what bdf_background_prior
     * writes before the entity's rows of every iteration, which are then sampled with (bg_mu, bg_Lambda).  Required when one of
     * the entity's relations is registered with a background */
    double *bg_Lambda;            /* dev, D x D                                                                             */
    double *bg_mu;                /* dev, D; with side information D x N                                                    */
    double *bg_pack;              /* dev, bdf_prior_pack_doubles(D)                                                         */
    double *bg_alpha_rows;        /* dev, BDF_MAX_TERMS: per term of this entity, alpha (1 - c0) of a background relation   */
    /* the spike-and-slab prior in place of the Normal-Wishart one (a zeroed tail is "none"): the entity's rows
     * by bdf_sample_rows_spike from its current rows, its hyper step by bdf_spike_hyper.  Ordered like an entity with side
     * information: the rows wait for the hyper step's event.  Neither side information nor a background; one rank              */
    int32_t spike;                /* 1: on                                                                                  */
    int32_t _pad_spike;
    double spike_a, spike_b, spike_shape, spike_rate;   /* incl_a, incl_b, shape, rate of bdf_spike_hyper                   */
    double *spike_state;          /* dev, 4 D: pi, tau, logit pi, log tau (initialised by the caller)                       */
    /* the non-negative prior in place of the Normal-Wishart one (a zeroed tail is "none"): the entity's rows by
     * bdf_sample_rows_nonneg from its current rows, its hyper step by bdf_nonneg_hyper.  Ordered like an entity with the
     * spike-and-slab prior.  Not together with it, side information or a background / dense relation; one rank                    */
    int32_t nonneg;               /* 1: on                                                                                  */
    int32_t _pad_nonneg;
    double nonneg_shape, nonneg_rate;   /* shape, rate of bdf_nonneg_hyper                                                  */
    double *nonneg_tau;           /* dev, D (initialised by the caller)                                                     */
} bdf_gibbs_entity;
int bdf_gibbs_create(bdf_ctx *rows_ctx, int D, int n_entities, const bdf_gibbs_entity *entities, bdf_gibbs **out);
int bdf_gibbs_destroy(bdf_gibbs *g);
/* the contexts of the hyperprior and prediction streams (owned by g), e.g. to create the test pairs' running state there */
int bdf_gibbs_contexts(bdf_gibbs *g, bdf_ctx **hyper, bdf_ctx **pred);
int bdf_ctx_stream(const bdf_ctx *ctx, void **stream);
/* test pairs updated at the end of every iteration (macau.jl:142-184); entity_of_mode: which entity every mode of the pairs is;
 * the other arguments as bdf_predict_update's */
int bdf_gibbs_set_test(bdf_gibbs *g, bdf_pairs *pairs, const int32_t *entity_of_mode, double mean_value, double clamp_lo,
                       double clamp_hi, double class_cut, double *stats_dev);
/* The relation model inside the native iteration (src/macau.jl:83-92): for every relation registered here bdf_gibbs_sweep runs,
 * BEFORE the entities' rows and on the row stream, sample_alpha (src/sampling.jl:129-134) when alpha_sample is set -- the squared
 * error over `train` (this rank's block of the relation's observations as pairs, with linear_values as their baseline when the
 * relation has features), summed over the ranks, the draw into alpha_dev -- and sample_beta_rel + linear_values
 * (src/sampling.jl:322-337, macau.jl:89-92) when `feat` is set; the row kernels of the relation's entities then read alpha_dev
 * and `linear` (terms are matched to relations by their bdf_rel).  feat_test / test_baseline: the registered test pairs'
 * baseline mean_value + F_test beta is refreshed after the draw (sampling.jl:9-14).  `probit`: the latent draw of the probit model
 * (bdf_probit_draw) at the same place, from the previous iteration's rows; the iteration is then z | U,V -> U | z,V -> V | z,U.
 * `censor`: the latent draw of the censored model (bdf_censored_draw, with alpha_dev) after sample_alpha; the iteration is then
 * alpha | U,V,z -> z | U,V,alpha -> U | z,V -> V | z,U.  `interval`: the latent draw of the interval-censored model
 * (bdf_interval_draw, with alpha_dev) at the same place and in the same order.  test_baseline without feat_test: the biases' tail
 * below.  Relations with none of these need no entry. */
typedef struct {
    const bdf_rel *rel;
    int32_t entity_of_mode[BDF_MAX_MODES];   /* which entity (index into bdf_gibbs_create's array) every mode of rel is          */
    double mean_value;
    double *alpha_dev;            /* dev, 1 double: the current alpha (initialised by the caller)                              */
    int32_t alpha_sample;
    uint32_t rel_tag;             /* 1-based relation number: keys the random streams (0x800000 | rel_tag)                      */
    double alpha_lambda0, alpha_nu0;
    int64_t nnz;                  /* observations of the whole relation (n of sample_alpha)                                     */
    bdf_pairs *train;             /* this rank's block of the observations (COO order) as pairs                                */
    int64_t first_obs, obs_block; /* its first observation; observations per rank block (linear is world x obs_block long)     */
    const bdf_feat *feat;         /* nullable: the block's rows of the relation's feature matrix                               */
    double *beta;                 /* dev, numF                                                                                  */
    double *linear;               /* dev, linear_values of the whole relation                                                   */
    double lambda_beta;
    const bdf_feat *feat_test;    /* nullable: feature rows of the registered test pairs ...                                    */
    double *test_baseline;        /* ... and their baseline (dev, one double per test pair)                                     */
    /* probit noise model (a zeroed tail of the struct is "no probit"): bdf_probit_draw over `train` into `linear` before the
     * entities' rows, which then read `linear` and alpha = 1.  Not with feat or alpha_sample; needs train and linear */
    int32_t probit;
    int32_t _pad;
    /* censored noise model (a zeroed tail is "none"): flags (dev, one int8 per observation of `train` in the caller's order).
     * bdf_censored_draw over `train` into `linear` after sample_alpha; the entities' rows then read `linear` and alpha_dev.  The
     * caller gives `train` the baseline `linear` (bdf_pairs_set_baseline) and starts `linear` at mean_value.  Not with probit or
     * feat; needs train and linear */
    const int8_t *censor;
    /* interval-censored noise model (a zeroed tail is "none"): bounds (dev, one (lo, hi) pair of doubles per observation of `train`
     * in the caller's order, aligned to 16 bytes).  bdf_interval_draw over `train` into `linear` after sample_alpha; the entities'
     * rows then read `linear` and alpha_dev.  The caller gives `train` the baseline `linear` (bdf_pairs_set_baseline) and starts
     * `linear` at mean_value.  Not with probit, censor or feat; needs train and linear */
    const double *interval;
    /* ordinal noise model (a zeroed tail is "none"): the sampled edges and the observations' levels (dev, one int8 per observation of
     * `train` in the caller's order).  bdf_ordinal_step (adapt -1) after sample_alpha and before bdf_interval_draw, rewriting
     * `interval`, which is required and therefore not const to the library; one rank, no feat */
    bdf_ordinal *ordinal;
    const int8_t *ordinal_codes;
    /* per-observation precision weights (a zeroed tail is "none"): obs_precision (dev, one double per observation of `train` in the
     * caller's order) is what the entities' rows read as bdf_term.obs_precision.  robust_nu >= 1: the Student-t model --
     * bdf_robust_draw (with alpha_dev: the previous iteration's alpha) rewrites obs_precision BEFORE sample_alpha, which then takes
     * sum omega e^2 in place of the sum of squares; the iteration is omega | U,V,alpha -> alpha | U,V,omega -> U | omega,V -> V |
     * omega,U.  robust_nu == 0: the weights are the caller's and stay; sample_alpha takes bdf_pairs_weighted_sse.  Not with
     * probit, censor, interval, ordinal, feat or a communicator; needs train */
    double robust_nu;
    double *obs_precision;
    /* Polya-Gamma noise models (a zeroed tail is "none"): pg_model 1 logit, 2 counts with the integer dispersion pg_r >= 1.
     * bdf_pg_draw rewrites obs_precision (omega) and linear (mean + y - kappa / omega) where the probit draw runs, before the
     * entities' rows, which read them with alpha = 1 (alpha_dev holds 1): the iteration is omega | U,V -> U | omega,V -> V | omega,U.
     * Needs train, linear and obs_precision; not with probit, censor, interval, ordinal, robust_nu, alpha_sample, feat or a
     * communicator */
    int32_t pg_model;
    int32_t _pad_pg;
    double pg_r;
    /* background cells (a zeroed tail is "none"): bg_weight = c0 > 0, every unlisted cell of the two-mode
     * relation observes bg_value with precision alpha c0.  Before the rows of either entity the iteration takes the sum and the
     * Gram matrix of the OTHER entity's rows (bdf_hyper_sums on the row stream, into bg_sums) and folds them into that entity's
     * prior (bdf_background_prior; the entity's bg_* buffers).  Listed cells of weight 1 (obs_precision NULL): the caller created
     * `rel` from the values mean + (r - c0 rb) / (1 - c0) and the rows read alpha (1 - c0); with weights: obs_precision holds
     * omega_k - c0, `linear` holds y_k - (omega_k r_k - c0 rb) / (omega_k - c0), both constant, and bg_weights the omega_k themselves.
     * alpha_sample: the sum of squares over all N M cells by bdf_background_sse over `train` (the original values), n = N M.
     * Not with probit, censor, interval, ordinal, robust_nu, pg_model, feat or a communicator */
    double bg_weight, bg_value;
    double *bg_sums;              /* dev, 2 (D + D D): for mode m at bg_sums + m (D + D D), the sum of that mode's rows, then their Gram matrix */
    const double *bg_weights;     /* dev, nullable: omega_k per observation of `train` in the caller's order                  */
    /* a noise precision per row of one entity (a zeroed tail is "none"): noise_mode 1-based, the mode of `rel`
     * whose rows carry tau_j ~ Gamma(noise_shape, noise_rate); noise_tau (dev, dims[noise_mode - 1]) receives the draw.
     * bdf_entity_noise_draw (with alpha_dev: the previous iteration's alpha) rewrites noise_tau and obs_precision where
     * bdf_robust_draw runs, BEFORE sample_alpha, which then takes sum_j tau_j S_j in place of the sum of squares; the rows of every
     * entity read obs_precision.  Needs train, obs_precision and noise_tau; not with probit, censor, interval, ordinal, robust_nu,
     * pg_model, a background, feat or a communicator */
    int32_t noise_mode;
    int32_t _pad_noise;
    double noise_shape, noise_rate;
    double *noise_tau;
    /* a dense relation (a zeroed tail is "none"): dense_R (dev, N x M row-major) holds every cell of the
     * two-mode relation without its mean, and `rel` lists NO cell.  Before the rows of either entity the iteration takes the Gram
     * matrix of the OTHER entity's rows (bdf_hyper_sums on the row stream, into dense_sums) and that entity's rows of R V or R' U
     * (bdf_dense_product, into dense_C: the N x D rows of mode 0, then the M x D rows of mode 1) and folds them into the prior
     * (bdf_dense_prior; the entity's bg_* buffers, bg_mu then D x N).  dense_holes (nullable): the cells that were not listed, as
     * pairs; bdf_dense_impute draws them into dense_R before alpha and the rows of every iteration and leaves the sum of their
     * squares in dense_stats (dev, 4 doubles; NULL without holes).  alpha_sample: the sum of squares over all N M cells by
     * bdf_dense_sse, n = N M, with dense_sum_r2 the listed cells' sum of r^2.  Not with any noise model, a background on the same
     * relation, feat or a communicator */
    double *dense_R;
    double *dense_C;
    double *dense_sums;           /* dev, 2 (D + D D): as bg_sums                                                             */
    double dense_sum_r2;
    const bdf_pairs *dense_holes;
    double *dense_stats;
    /* row and column biases (a zeroed tail is "none"): n_bias terms, one per biased mode of `rel`.
     * bdf_bias_draw (with alpha_dev: the previous iteration's alpha) runs BEFORE sample_alpha and rewrites the terms' bias and
     * lambda and `linear`, which the rows of every entity read as linear_values and which the caller has made the baseline of
     * `train` (bdf_pairs_set_baseline), so that sample_alpha's sum of squares sees the new biases.  bias_resid: dev, one double per
     * observation (scratch).  bias_test / test_baseline (both or neither): pairs over the relation's entities whose baseline
     * test_baseline (one double per pair) is refreshed after the draw, behind the prediction updates that read it.  Needs train,
     * linear and bias_resid; Gaussian noise with one precision only: not with probit, censor, interval, ordinal, obs_precision,
     * pg_model, noise_mode, a background, a dense relation, feat or a communicator */
    int32_t n_bias;
    int32_t _pad_bias;
    bdf_bias_term bias[BDF_MAX_MODES];
    double *bias_resid;
    const bdf_pairs *bias_test;
} bdf_gibbs_relation;
int bdf_gibbs_set_relations(bdf_gibbs *g, int n_relations, const bdf_gibbs_relation *rels);
/* several ranks: exchange every entity's rows after sampling them (NULL: none) */
int bdf_gibbs_set_comm(bdf_gibbs *g, bdf_comm *comm);
/* one iteration.  predict_phase: bdf_predict_update's phase (0 burn-in, 1 first posterior sample, 2 later ones), -1: none */
int bdf_gibbs_sweep(bdf_gibbs *g, uint32_t sweep, int predict_phase);      /* predict_phase 3 (set-up): this sample's statistics only, no running state */
/* which of sample[0..2] holds entity's current rows */
int bdf_gibbs_current(const bdf_gibbs *g, int entity, int *buffer);
/* measurement: the row launch of one entity as bdf_gibbs_sweep makes it, and nothing else (no hyperprior update, exchange or
 * prediction update: the chain's state is not kept consistent) */
int bdf_gibbs_rows_only(bdf_gibbs *g, int entity, uint32_t sweep);
/* The iteration piece by piece, for a host that keeps the schedule itself and enqueues the prediction update through the entry
 * points above: the same code bdf_gibbs_sweep runs, with plain stream order (no events, no polling, no done counters) under the
 * iteration number the caller has set on the contexts with bdf_ctx_set_sweep.  Relations, rows and beta go to the row context's
 * stream, draws and hyperprior to the hyperprior context's (bdf_gibbs_contexts) -- or, for an object created with BDF_NO_OVERLAP set
 * in the environment, to the row context's as well.  Nothing of the object's bookkeeping changes but the rows' buffer rotation.
 * bdf_gibbs_step_relations: what the registered relations' models run before the rows (bdf_gibbs_set_relations).
 * bdf_gibbs_step_rows: one entity's rows -- uhat and the per-row prior means with side information, the prior with the background
 * and dense terms folded in, the row launch chunk by chunk, with a communicator every chunk's exchange -- after which the entity's
 * buffers have rotated (bdf_gibbs_current).  pack_valid: the entity's latest hyperprior draw (bdf_hyper_sample) has left its prior
 * pack; 0 before the first draw.  The context's bdf_ctx_time_next_rows events go to the row launch.
 * bdf_gibbs_step_draws: the data-independent part of the entity's hyperprior draw (bdf_hyper_draws) into its draws buffer; may be
 * enqueued before the entity's rows.  Nothing for an entity with the spike-and-slab prior.
 * bdf_gibbs_step_hyper: the entity's hyperprior from its current rows -- the spike-and-slab prior's hyper step, or the feature
 * terms, the sums (with a communicator over the ranks) and the Normal-Wishart draw.  draws_prepared: bdf_gibbs_step_draws has run
 * under this iteration number; 0: the draw makes its own normals (the same values).
 * bdf_gibbs_step_beta: beta (and lambda_beta) of an entity with side information from its current rows and (mu, Lambda); nothing
 * for an entity without. */
int bdf_gibbs_step_relations(bdf_gibbs *g);
int bdf_gibbs_step_rows(bdf_gibbs *g, int entity, int pack_valid);
int bdf_gibbs_step_draws(bdf_gibbs *g, int entity);
int bdf_gibbs_step_hyper(bdf_gibbs *g, int entity, int draws_prepared);
int bdf_gibbs_step_beta(bdf_gibbs *g, int entity);
/* parity hooks: the terms (entity's n_terms of them, the factors at the current samples) and the prior that the entity's next row
 * launch would take.  bdf_gibbs_row_prior enqueues the fold of the background and dense terms on the row stream and hands back
 * device pointers: the prior mean (one, or one per row: *mu_is_matrix), Lambda and the prior pack (NULL: none). */
int bdf_gibbs_terms(bdf_gibbs *g, int entity, bdf_term *out);
int bdf_gibbs_row_prior(bdf_gibbs *g, int entity, int pack_valid, const double **mu, int *mu_is_matrix, const double **Lambda,
                        const double **pack);
/* set-up: brings the device to its working state without advancing the chain.  Full iterations (rows of every entity,
 * hyperprior chains, beta, the prediction kernel on the registered test pairs WITHOUT running state) with iteration numbers
 * no real iteration uses, for about `milliseconds` (with a communicator: milliseconds / 0.1 iterations, the same count on
 * every rank), then the chain's state -- every entity's current sample, (mu, Lambda), sums, prior pack, draws, beta, uhat,
 * lambda_beta, and whether a draw of an earlier iteration exists -- is put back bit for bit.  The buffers rotate meanwhile:
 * ask bdf_gibbs_current afterwards.  (Row launches alone leave a short run of iterations 5 % slower than this does.) */
int bdf_gibbs_warm_device(bdf_gibbs *g, double milliseconds);
/* (set-up) does the entity's hyperprior draw / beta of an earlier iteration exist (bdf_gibbs_sweep takes the next row launch's
 * prior pack from it and waits for it)?  A host that runs iterations whose results it then discards -- the engine's device
 * warm-up: full iterations, then every buffer put back -- puts these two flags back as well. */
int bdf_gibbs_recorded(const bdf_gibbs *g, int entity, int *hyper, int *beta);
int bdf_gibbs_set_recorded(bdf_gibbs *g, int entity, int hyper, int beta);
/* the caller has written the entity's sample itself (any of its three buffers), with nothing of the chain in flight: K1c's gather
 * images of it are stale, the next launch that gathers one packs it anew (bdf_ctx_set_gather_image).  bdf_gibbs_set_recorded
 * says the same.  A sample written without either is gathered as it was before. */
int bdf_gibbs_sample_written(bdf_gibbs *g, int entity);
/* measurement: (start, stop) events ride on the dispatch of entity's next row kernel (bdf_ctx_time_next_rows) */
int bdf_gibbs_time_rows(bdf_gibbs *g, int entity, void *start, void *stop);
int bdf_gibbs_span_rows(bdf_gibbs *g, int entity, void *slot_dev);      /* bdf_ctx_span_next_rows for the next row launch of `entity` */
int bdf_gibbs_sync(bdf_gibbs *g);     /* waits for the three streams; errors as bdf_ctx_sync */

/* ---- synthetic sparse relation of configuration C4 (host-only, needs no GPU) ---------------------------------------
 * The reference's large-scale benchmark draws its relation with sprand (test/benchmark_parallel_latent.jl:8-12).
 * Observations k_begin .. k_end-1 of the relation `seed`: row uniform on 1..n_rows; column Zipf-like, p(c) ~ 1/(c + zipf_offset)
 * (continuous inverse CDF; zipf_offset 0 = uniform); value clip(round(3.5 + <u*_row, v*_col> + 0.5 eps), 1, 5) from a planted
 * rank-8 model with 0.5 N(0,1) factors; held_out[k] = 1 for a test_fraction of the observations (nullable).  Counter-based
 * (Philox, key = seed): observation k does not depend on the range or the number of threads, so every rank of a multi-GPU
 * run can generate the relation (or its part) independently.  rows/cols 1-based int32. */
int bdf_synth_ratings(uint64_t seed, int64_t n_rows, int64_t n_cols, int64_t k_begin, int64_t k_end,
                      double zipf_offset, double test_fraction, int32_t *rows_out, int32_t *cols_out,
                      double *vals_out, uint8_t *held_out);

/* ---- variational BPMF (src/macau_vb.jl: bpmf_vb, VBModel) ---------------------------------------------------------
 * The deterministic mean-field variant of BPMF on ONE two-mode relation (data.relations[1]; side information ignored, as in
 * the reference).  One GPU, matrices only: VB on several GPUs and on tensors is out of scope.  Every row of a VB model is kept
 * on the device as mu (D doubles) and Euu = inv(L) + mu mu' as a packed upper triangle (D (D + 1) / 2 doubles), in a record
 * padded to whole 128-byte lines; the host's VBModel.Euu (D x D x N) is unpacked only by bdf_vb_model.  Results are the same
 * bits from run to run (no floating-point atomics).  The two entities' records take 2 x N x D (D + 1) / 2 x 8 bytes and more:
 * a C4-sized relation (10^7 + 10^6 rows) does not fit at D = 64. */
typedef struct bdf_vb bdf_vb;
/* bpmf_vb's set-up (macau_vb.jl:46-65) and two VBModel(D, N) (:20-37) with the caller's random means.  dims[2]: N_u, N_v;
 * ids: nnz x 2 column-major 1-based (df[:,1], df[:,2]), id_bytes 4|8; values: nnz (df[:,end]); alpha: relations[1].model.alpha
 * (fixed, never sampled).  mean_value = mean(values); values are centred and duplicate (u, v) pairs summed into one entry as
 * sparse() does; the raw pairs are kept for the train RMSE.  mu_init_u / mu_init_v: host D x N_u / D x N_v (randn(D, N)).
 * Errors: BDF_ERR_BOUNDS for an id outside 1..dims; BDF_ERR_ARG for D outside 1..BDF_MAX_D or when the device memory the
 * model needs (the byte count is in bdf_last_error()) exceeds what is free. */
int bdf_vb_create(bdf_ctx *ctx, int D, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes, const double *values,
                  double alpha, const double *mu_init_u, const double *mu_init_v, bdf_vb **out);
int bdf_vb_destroy(bdf_vb *vb);
/* test_vec of relations[1] (macau_vb.jl:56-58) as pairs (borrowed, NULL: none -- the test RMSE is NaN) and the clamp of
 * clamp!(yhat, clamp) (src/sampling.jl:108-114) for both RMSEs: clamp_lo > clamp_hi means no clamping */
int bdf_vb_set_test(bdf_vb *vb, bdf_pairs *test, double clamp_lo, double clamp_hi);
/* n iterations of macau_vb.jl:61-77, enqueued on the context's stream with no host round trip: update_u!(U, V),
 * update_u!(V, U) (:103-130), update_prior!(U), update_prior!(V) (:132-140), then the test and train squared errors of
 * clamp!(mean_value + <mu_u, mu_v>) (:73-76, :142-148).  A precision that fails to factor is reported by the next
 * bdf_vb_stats / bdf_ctx_sync as BDF_ERR_NOTPD. */
int bdf_vb_iterate(bdf_vb *vb, int n);
/* waits for the stream; out[4] = {rmse, rmse_train, vecnorm(U.mu_u), vecnorm(V.mu_u)} of the last iteration (:80); rmse and
 * rmse_train are NaN before the first iteration and rmse without test pairs */
int bdf_vb_stats(bdf_vb *vb, double *out);
/* host copy of a model (entity 0 = U, 1 = V), every output nullable: mu_host D x N (mu_u), Euu_host D x D x N (Euu, full),
 * prior_host D + D x D + 2 doubles (mu_N, W_N, nu_N, b_N) */
int bdf_vb_model(bdf_vb *vb, int entity, double *mu_host, double *Euu_host, double *prior_host);

/* ---- Hamiltonian Monte Carlo BPMF (src/macau_hmc.jl: macau_hmc, HMCModel) -------------------------------------------
 * The leapfrog sampler on ONE two-mode relation (data.relations[1]; side information out of scope), one GPU.  Samples,
 * momenta and start copies are N x D row-major on the device (the host's D x N column-major).  Iteration i draws its momenta
 * from (BDF_P_HMC_MOMENTUM, entity 0 | 1, row, normal k), its Metropolis uniform from (BDF_P_HMC_ACCEPT, 0, 0, pair 0) and
 * the prior from bdf_hyper_sample's streams with entity tags 0 (U) and 1 (V), all at sweep i.  Results are the same bits
 * from run to run (no floating-point atomics). */
typedef struct bdf_hmc bdf_hmc;
/* macau_hmc's set-up (macau_hmc.jl:33-57) after reset!: samples 0, mu 0, Lambda 5 I, mu0 0, b0 2, WI I, nu0 D, and the mass
 * G = diag(Lambda) = 5 (HMCModel, :13-18; it never follows Lambda).  dims[2]: N_u, N_v; ids: nnz x 2 column-major 1-based,
 * id_bytes 4|8; values: nnz; alpha: relations[1].model.alpha (fixed).  mean_value = mean(values); values are centred; the
 * gradient's CSRs (both modes) sum duplicate (u, v) pairs as sparse() does, and keep per entry the multiplicity and the sum of
 * the squared values for the energy, which sums the observations one by one.  Errors as bdf_vb_create's. */
int bdf_hmc_create(bdf_ctx *ctx, int D, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes, const double *values,
                   double alpha, bdf_hmc **out);
int bdf_hmc_destroy(bdf_hmc *hmc);
/* test_vec of relations[1] as pairs (borrowed, NULL: none -- the RMSEs are NaN) and the clamp: clamp_lo > clamp_hi: none.
 * Call before the first iteration. */
int bdf_hmc_set_test(bdf_hmc *hmc, bdf_pairs *test, double clamp_lo, double clamp_hi);
/* the keyword arguments (L, L_inner, prior_freq >= 1, eps > 0 finite, burnin >= 0); eps and L are then adapted by the
 * iterations (a rejection with dH < -6 halves eps and sets L = ceil(1.6 L)).  Defaults: 10, 1, 8, 0.01, 100. */
int bdf_hmc_set_params(bdf_hmc *hmc, int L, int L_inner, int prior_freq, double eps, int burnin);
/* n iterations of macau_hmc.jl:60-132: momenta, 2 L + 1 leapfrog launches (hmc_update_u!), the energies, the Metropolis
 * step, the restore on rejection, update_latent_prior! every prior_freq-th iteration, and yhat = clamp!(pred(test)) with
 * update_yhat_post!'s running mean (of the clamped predictions, as clamp! works in place).  The host needs the adapted L
 * before it can enqueue the next leapfrog: every iteration waits for the previous one's decision (one small device-to-host
 * copy).  A non-finite energy or a prior that fails to factor is reported by the next bdf_hmc_stats / bdf_ctx_sync. */
int bdf_hmc_iterate(bdf_hmc *hmc, int n);
/* waits for the stream; out[16] = the last iteration's record: {i, eps, L (both used), kinetic start, kinetic final,
 * potential start, potential final, dH, accepted (0 | 1), new eps, new L, vecnorm(U), vecnorm(V), the uniform, rmse,
 * rmse_avg}; all 0 / NaN before the first iteration.  log (nullable, log_cap doubles): the momentum norms after each of
 * the 2 L + 1 launches in launch order |r_U|, |r_V|, |r_U|, ..., |r_V|, |r_U|. */
int bdf_hmc_stats(bdf_hmc *hmc, double *out, double *log, int log_cap);
/* host copy of an entity's state (0 = U, 1 = V), every output nullable: sample D x N, momentum D x N, mu D, Lambda D x D */
int bdf_hmc_model(bdf_hmc *hmc, int entity, double *sample, double *momentum, double *mu, double *Lambda);

#ifdef __cplusplus
}
#endif
#endif /* BDF_H */
