// bdf_common.h -- internal declarations shared by the HIP translation units of libbdf_hip.so
#pragma once
#include <map>
#include <memory>
#include <array>
#include <algorithm>
#include <numeric>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <vector>
#include "../../include/bdf.h"

void bdf_set_error(const char *fmt, ...);

#define BDF_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) {                                                           \
            bdf_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return BDF_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define BDF_REQUIRE(cond, code, ...)                                                       \
    do {                                                                                   \
        if (!(cond)) { bdf_set_error(__VA_ARGS__); return (code); }                        \
    } while (0)

#include "dev_buf.h"

// rows 0..N-1 by falling degree(row), rows of equal degree in row order (a stable sort)
template <typename Degree>
std::vector<int32_t> rows_by_degree(int64_t N, Degree degree)
{
    std::vector<int32_t> ord((size_t)N);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return degree(x) > degree(y); });
    return ord;
}

struct bdf_rows_state;
struct bdf_ctx {
    int device = 0;
    int n_cus = 0;             // the device's CUs (multiProcessorCount)
    hipStream_t stream = nullptr;   // borrowed: the caller's, or a pooled one (NULL is the device's default stream)
    uint64_t seed = 0;
    DevBuf<uint32_t> sweep_dev;    // Gibbs iteration counter in device memory
    uint32_t sweep_host = 0;   // mirror of the last bdf_ctx_set_sweep / advance
    // scratch (grown on demand, never shrunk)
    DevBuf<void> scratch;
    DevBuf<void> scratch2;     // second block: split-K partials of the dense products (used while `scratch` is held)
    int small_max = 48;        // k_rows_small: longest row (observations) sampled four to a wave at D <= 16; 0: off
    int64_t small_min_rows = 8192; // ... and the smallest entity (rows) for which it is used
    // k_rows_lr (k_rows_lr.hip): rows of few observations sampled by the low-rank map instead of the reference's
    int lr_max = -1;           // longest row (observations) sampled that way at D > 16; -1: min(16, D / 2); 0: off
    int64_t lr_min_rows = 8192; // ... and the smallest number of such rows in a launch for which it is used
    int col_piece = 128;       // K1c (k_rows_col.hip): one two-mode relation at 16 < D <= 32 four rows per wave in the column layout, rows cut
                               // into pieces of at most this many observations; 0: off
    bool col_explicit = false; // ... set by the caller (bdf_ctx_set_col_rows): taken also when the caller chose K1's item size
    int gather_image = 1;      // K1c at D = 32 gathers from the opposite entity's gather image (k_gather_image.hip): 1 the pair image (the
                               // default), 2 the full image, 0 off -- the sample itself (bdf_ctx_set_gather_image)
    bool gimg_trust = false;   // (library-internal) the next row launch may take the opposite sample's image as its own launch left it: the
                               // caller knows of every write to that sample (bdf_gibbs_sweep); cleared by the launch
    DevBuf<double> lr_T;       // Tf | Tb | Tm (64 x 64 each) | L' mu (64): the launch's constants (k_lr_prep)
    DevBuf<double> lr_mrows;   // per-row prior means transformed (L' mu_i, rows of DP doubles), grown on demand
    DevBuf<double> lr_vt;      // the opposite entity's factor matrix transformed (V L^-T), grown on demand
    int *flag_dev = nullptr;   // not-positive-definite flag (bits 1..32: errors; 64: BDF_WARN_CG_MAXITER): the device address of
    DevBuf<int> flag_host = DevBuf<int>::pinned(kPinnedMappedCoherent);
                               // ... a word of mapped, coherent HOST memory (kernels atomicOr into it on their error paths only;
                               // bdf_ctx_sync reads it without a copy -- a 4-byte blocking device-to-host copy is ~10 us)
    uint32_t warnings = 0;     // non-fatal bits seen by bdf_ctx_sync, until bdf_ctx_warnings takes them
    int item_size = 192;       // K1: observations per work item (rows longer than this are split)
    int piece_size = 128;      // K1: ... into pieces of at most this many observations
    bool item_auto = true;     // K1: neither was set by the caller: large launches take larger items (rows_plan.hip: route_key)
    int gather_mode = 0;       // K1 parity hook: 0 auto, 1 general gather path, 2 lean path with 64-bit row offsets (D > 32)
    // borrowed, the caller's events -- bdf_ctx_time_next_rows: attached to the next row-kernel dispatch, then cleared
    hipEvent_t time_start = nullptr, time_stop = nullptr;
    unsigned long long *rows_span = nullptr;   // borrowed -- bdf_ctx_span_next_rows: SampleArgs::span of the next row launch, then cleared
    const uint32_t *rows_ready = nullptr;      // borrowed (library-internal) SampleArgs::ready of the next row launch, then cleared
    uint32_t rows_ready_want = 0;
    // (library-internal, bdf_gibbs_sweep) the rows' hand-over to the hyperprior chain WITHOUT an event: when the next bdf_sample_rows is
    // one k_rows_col launch, every wave of it -- its rows written through, the stores drained -- adds 1 to shard (wave % 64) of these
    // 64 words (16 words apart), and rows_done_added says how many will; else rows_done_added stays -1 and the caller uses the event
    uint32_t *rows_done = nullptr;             // borrowed
    int64_t rows_done_added = -1;
    // (library-internal, bdf_sample_rows_nonneg) the next system dump takes positions rows_k0 .. rows_k1 - 1 of the shard's row list
    // only and writes the system of position k at index k - rows_k0; rows_k1 = 0: every row at its own index.  Cleared by the launch
    int64_t rows_k0 = 0, rows_k1 = 0;
    int64_t nonneg_chunk = 0;                  // bdf_ctx_set_nonneg_chunk: rows per chunk of the non-negative prior's launches; 0: the default
    const uint32_t *hyper_wait = nullptr;      // borrowed (library-internal) ... and the next one-launch chain (k_hyper_chain) polls their sum for this target
    uint32_t hyper_wait_target = 0;
    uint32_t *hyper_ready = nullptr;           // borrowed (library-internal) word the next bdf_hyper_sample sets to hyper_ready_value once its pack is written, then cleared
    uint32_t hyper_ready_value = 0;
    hipEvent_t time_h_start = nullptr, time_h_stop = nullptr;  // borrowed -- bdf_ctx_time_next_hyper: start of the next sums kernel, end of the next draw kernel
    // batched CG (k_feat_cg.hip): device flag that lets product kernels enqueued ahead return at once (NULL outside a solve),
    // and the host-mapped words through which the device reports (iteration, active columns)
    // CU reservation (bdf_ctx_create_rows): the last... the first `reserve_cus` bits of the CU mask (one CU per XCD each 8)
    // are kept free of this context's kernels, for the side context created with reserved = 1
    int reserve_cus = 0;       // CUs set aside by the row context this one belongs to (0: none)
    int on_reserved = 0;       // this context's stream runs on the reserved CUs only
    const int *skip_flag = nullptr;            // borrowed
    DevBuf<volatile uint64_t> cg_status = DevBuf<volatile uint64_t>::pinned(kPinnedMapped);
    // bdf_gibbs_sweep: the next bdf_hyper_sums of a small entity leaves its work to the bdf_hyper_sample that follows it on this context
    bool hyper_fuse = false;
    // borrowed, the caller's buffers of that call
    const double *hyper_partial = nullptr; int hyper_nblocks = 0; double *hyper_sumU = nullptr, *hyper_UUt = nullptr;
    bool hyper_chain = false;           // ... and launches nothing itself: the draw's launch carries the sums' workgroups (k_hyper_chain)
    int hyper_chain_D = 0; int64_t hyper_chain_N = 0, hyper_chain_rpb = 0; const double *hyper_chain_sample = nullptr, *hyper_chain_uhat = nullptr;   // borrowed
    DevBuf<unsigned> hyper_count;       // partial workgroups finished (k_hyper_chain), allocated at first use
    double *hyper_chain_draws = nullptr; // borrowed (bdf_gibbs_sweep) the chain's launch also makes the entity's random part (k_hyper_draws' values) into this buffer
    DevBuf<double> cg_part;             // partial dot products of the chunked CG step (k_cg_long_*), allocated at first use
    uint32_t cg_gen = 0;
    DevBuf<unsigned> cg_bar;            // the hand-over counter of the one-launch CG solve (k_cg_resident), allocated at first use
    bdf_rows_state *rows = nullptr;     // the row launcher's own (rows_plan.hip): cached plans, dispatch counts, what lr_T / lr_vt were computed from
    DevBuf<double> norm_part;           // bdf_norm2's per-workgroup partial sums (k_auc.hip), allocated at first use
    DevBuf<double> newrows_W;           // bdf_newrows_quad's L^-1 of the call's Lambda (k_newrows.hip: BDF_MAX_D x BDF_MAX_D), allocated at first use

    bdf_ctx() = default;
    bdf_ctx(const bdf_ctx &) = delete;
    ~bdf_ctx();                         // bdf_api.hip: waits for the stream, then the members free themselves
};

int bdf_scratch(bdf_ctx *ctx, size_t bytes, void **out);
int bdf_scratch2(bdf_ctx *ctx, size_t bytes, void **out);
int bdf_sum_ranks_into(bdf_ctx *ctx, bdf_comm *comm, double *x, int64_t n, double *gather);
int bdf_sample_beta_rel_impl(bdf_ctx *ctx, bdf_comm *comm, const bdf_feat *fc, const bdf_pairs *train, int64_t first_obs, int D,
                             const double *const *factors, double mean_value, double alpha, const double *alpha_dev, double lambda_beta,
                             uint32_t rel_tag, double *beta_out, double *linear_out, double *rhs_out);
#define BDF_DRAWS_BATCH 8
int bdf_hyper_draws_batch(bdf_ctx *ctx, int D, int n, const int64_t *N, const double *nu, const uint32_t *entity_tag, double *const *draws_out);

struct bdf_mode_index {
    std::vector<int64_t> rowptr;   // host, dims+1
    std::vector<int64_t> rowids;   // host, nnz, 1-based COO row numbers (IndexedDF.index)
    std::vector<int32_t> order;    // host, rows by descending degree (stable)
    DevBuf<int64_t> rowptr_dev;    // dims+1
    DevBuf<int32_t> colidx_dev;    // (n_modes-1) planes of nnz: 0-based ids of the other modes, mode order
    DevBuf<double> vals_dev;       // nnz values in mode order
    DevBuf<int32_t> perm_dev;      // nnz: 0-based COO row number in mode order
    DevBuf<uint32_t> packed_dev;   // nullable, two-mode relations with <= 256 distinct values: (value code << 24) | other-mode id
    DevBuf<int32_t> order_dev;
    // relation created with a layout (bdf_relation_create_sharded): the device arrays hold only the observations of the rows
    // this rank owns, chunk after chunk in internal-position order, and colidx holds INTERNAL positions of the other modes
    std::vector<int32_t> own_orig;     // original id of every owned row
    std::vector<int32_t> own_pos;      // its internal position (row of the factor matrix)
    std::vector<int64_t> own_q;        // offsets of the owned rows' observations in the device arrays (owned + 1)
    std::vector<int64_t> chunk_begin;  // first owned row of every chunk (chunks + 1)
    int64_t own_nnz = 0;
};

struct bdf_rel {
    bdf_ctx *ctx = nullptr;    // borrowed
    uint64_t serial = 0;       // unique per created relation (keys the K1 plan cache)
    int n_modes = 0;
    int64_t dims[BDF_MAX_MODES] = {};
    int64_t nnz = 0;
    double value_mean = 0.0;
    bdf_mode_index idx[BDF_MAX_MODES];
    int sharded = 0;                   // created with a layout
    int rank = 0, world = 1, chunks = 1;
    int64_t nint[BDF_MAX_MODES] = {};  // rows of the factor matrix of every mode (== dims without a layout)
    // ratings take few distinct values (MovieLens: 5): when there are at most 256 the relation also keeps them as 8-bit codes
    // into this table, packed with the other mode's id (K1's coded two-mode variant: no value registers in its pipeline)
    int n_codes = 0;                   // 0: not coded
    DevBuf<double> table_dev;          // 256 doubles, ascending distinct values (the rest zero)
    ~bdf_rel();                        // bdf_api.hip: waits for the stream and drops the relation's row plans; the members free themselves
};

struct bdf_pairs {
    bdf_ctx *ctx = nullptr;       // borrowed
    int n_modes = 0;
    int64_t n = 0;
    DevBuf<int32_t> ids_dev;      // n_modes planes of n, 0-based
    DevBuf<double> values_dev;    // n
    DevBuf<double> avg_dev, sq_dev;
    double count = 0.0;           // counter_prob (macau.jl:171-183)
    const double *baseline_dev = nullptr;   // nullable, borrowed: per-pair baseline replacing mean_value (relation features)
    DevBuf<int32_t> orig_dev;     // nullable: storage position -> caller's index (bdf_pairs_sort)
    int sorted_mode = -1;         // the mode bdf_pairs_sort sorted by, -1: caller's order
    std::vector<int32_t> ids_host, orig_host;
    std::vector<double> values_host;
    DevBuf<void> auc_ws;          // bdf_pairs_auc's workspace (bdf_auc_workspace_bytes(n)), allocated at first use
    int link = 0;                 // bdf_pairs_set_link: 0 identity, 1 probit (predictions are Phi(udot + base): k_probit.hip), 2 logistic; 3 counts (k_pg.hip)
    double link_r = 0.0;          // bdf_pairs_set_count_link: predictions are link_r exp(udot + base)
    DevBuf<double> lpd_dev;       // bdf_pairs_lpd_update's running state (k_lpd.hip): n maxima M, then n sums A, in storage order; at first use
    double lpd_draws = 0.0;       // ... and the posterior draws it holds (a counter of its own, not `count`)
    DevBuf<double> waic_dev;      // bdf_pairs_waic_update's running state (k_waic.hip): four planes of n in storage order -- M, A, mean, M2; at first use
    double waic_draws = 0.0;      // ... and the posterior draws it holds (a counter of its own)
    const double *scale_dev = nullptr;      // nullable, borrowed (bdf_pairs_set_precision_scale): a precision scale per row of mode scale_mode, for k_lpd
    int scale_mode = 0;
    DevBuf<double> newrows_dev;   // bdf_newrows_update's running state (k_newrows.hip): five planes of n in storage order -- mean, M2, sum q, M, A; at first use
    double newrows_draws = 0.0;   // ... the posterior draws it holds (a counter of its own)
    bool newrows_score = false;   // ... and whether their log-likelihoods were folded in (score_lpd of the phase 1 call)
    DevBuf<int64_t> foldin_ptr_dev;         // bdf_foldin_cells (k_foldin.hip): the pairs sorted by mode 0 as rows -- foldin_rows + 1 offsets into the storage
    int64_t foldin_rows = 0, foldin_cols = 0;   // order; made at the first call for these dims, which every id was checked against
    ~bdf_pairs();                 // k_predict.hip: waits for the context's stream; the members free themselves
};

// bdf_ordinal (k_ordinal.hip): the edges of an ordinal relation and their Metropolis step's state, all of it in ONE device buffer
// of doubles so that a caller who must put a chain back (bdf_gibbs_warm_device) copies one piece
#define BDF_ORD_TABLE 17           // doubles per edge table: e_0 = -inf, e_1 .. e_{K-1}, e_K = +inf (+inf beyond K)
#define BDF_ORD_CUR 0              // the current table
#define BDF_ORD_PROP 17            // the proposed one (behind the current one: the mass kernel loads both as one run)
#define BDF_ORD_JAC 34             // the proposal's log Jacobian term
#define BDF_ORD_SIGMA 35           // the step size
#define BDF_ORD_PROPOSALS 36       // steps taken
#define BDF_ORD_ACCEPTS 37         // ... and accepted
#define BDF_ORD_LAST_S 38          // the last step's log acceptance ratio (-inf: refused by the gap guard)
#define BDF_ORD_ACCEPTED 39        // ... and its decision (1 / 0)
#define BDF_ORD_VALID 40           // the proposal passed the gap guard (1 / 0)
#define BDF_ORD_LOGU 41            // the log of the last step's uniform
#define BDF_ORD_TRACE 48           // then capacity rows of K - 1 edges
#define BDF_ORD_MAX_TRACE ((int64_t)1 << 24)   // rows a trace may have (2 GB of device memory at K = 16)
struct bdf_ordinal {
    bdf_ctx *ctx = nullptr;        // borrowed
    int K = 0;
    int64_t capacity = 0;          // trace rows
    int64_t adapt_steps = 0;       // bdf_ordinal_set_adapt
    size_t state_doubles = 0;
    DevBuf<double> state_dev;
    hipStream_t stream = nullptr;  // borrowed: where the last step was enqueued (bdf_ordinal_read waits for it)
};

struct bdf_feat {
    bdf_ctx *ctx = nullptr;   // borrowed
    int kind = 0;             // 0 dense, 1 csr (real), 2 binary
    int64_t m = 0, n = 0, nnz = 0;
    DevBuf<double> dense_dev; // m x n column-major
    // CSR (rows) and CSC (= CSR of F') so that neither product needs atomics
    DevBuf<int64_t> rowptr_dev; DevBuf<int32_t> colind_dev; DevBuf<double> rvals_dev;
    DevBuf<int64_t> colptr_dev; DevBuf<int32_t> rowind_dev; DevBuf<double> cvals_dev;
    // column panels of the sparse products (k_feat_ops.hip, spmm): entries of row r with a column in panel p are
    // [panel_ptr[p * rows + r], panel_ptr[(p + 1) * rows + r]) -- NULL when the operand is small or a row's entries are not in column order
    DevBuf<int64_t> panel_fwd_dev; int n_panels_fwd = 0;      // F   (rows m, panels over the n columns)
    DevBuf<int64_t> panel_tr_dev; int n_panels_tr = 0;        // F'  (rows n, panels over the m columns)
    DevBuf<double> FF_dev;        // n x n (F'F), built on first use_ff
    DevBuf<int32_t> row_ids_dev;  // nullable (bdf_feat_set_row_ids): original id of every row of F, keys the rows' noise streams
    DevBuf<double> chol_ws;       // workspace of the blocked direct solve (k_chol.hip), grown on demand
    DevBuf<void> gather_dev;      // several ranks: the blocks of beta columns the ranks exchange (bdf_sample_beta_ranks), grown on demand
    // direct solve of a mid-sized feature set (64 < n <= BDF_EIG_MAX): F'F = Q diag(s) Q' once (host, first use), then
    // (F'F + lambda I) \ rhs = Q ((Q' rhs) ./ (s + lambda)) per iteration -- lambda changes every iteration, Q and s do not
    std::unique_ptr<bdf_feat> eig_Q;   // Q as a dense n x n operator (eigenvectors in columns)
    DevBuf<double> eig_s;         // n eigenvalues (dev)
    DevBuf<double> eig_y;         // n x D workspace (dev), grown with D
    bool eig_failed = false;      // the decomposition's QL iteration did not converge: this operator takes the factorisation (bdf_chol_solve) instead
    bool FF_summed = false;       // several ranks, F split by rows (bdf_sample_beta_rel_ranks): FF_dev already holds the sum over the ranks
    ~bdf_feat();                  // k_feat_ops.hip: waits for the context's stream; the members free themselves
};
#define BDF_EIG_MAX 640

// (FF + lambda I) \ rhs for all D right-hand sides by blocked Cholesky (solve_full, src/sampling.jl:314-320)
int bdf_chol_solve(bdf_ctx *ctx, bdf_feat *f, int D, const double *lambda_dev, const double *rhs, double *beta);

// ---------------------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller (host+device).  Counter layout: DESIGN.md "RNG contract".
// ---------------------------------------------------------------------------------------
struct u32x4 { uint32_t x, y, z, w; };

__host__ __device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
        u32x4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

__host__ __device__ __forceinline__ u32x4 bdf_draw(uint64_t seed, uint32_t sweep, uint32_t purpose, uint32_t entity,
                                          uint64_t row, uint32_t pair)
{
    u32x4 c;
    c.x = (uint32_t)row;
    c.y = (uint32_t)((row >> 32) & 0xffffu) | (pair << 16);
    c.z = sweep;
    c.w = (purpose << 24) | (entity & 0xffffffu);
    return philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__host__ __device__ __forceinline__ double bdf_u01(uint32_t lo, uint32_t hi)
{
    uint64_t x = ((uint64_t)hi << 32) | lo;
    return ((double)(x >> 11) + 0.5) * 0x1.0p-53;
}

// How the polynomials below name their coefficients.  BdfLiteral: as literals.  A kernel that keeps many registers live around its
// normals (k_rows_col.hip) passes a policy of its own that hands every coefficient over where it is used: literals of a loop's body
// are otherwise materialised ONCE, in front of the loop, and held in vector registers across all of it.  The same operations on
// the same values either way.
struct BdfLiteral { static __device__ __forceinline__ double c(double x) { return x; } };

// sin(2 pi u), cos(2 pi u) for u in (0, 1).  The argument is reduced in u, exactly: q = nearest integer to 4u, r = u - q/4
// in [-1/8, 1/8]; then the fdlibm kernel polynomials on |2 pi r| <= pi/4 and the quadrant.  Within ~2e-16 of sin / cos of the
// rounded product 2 pi u (the oracle's libm calls) at a seventh of the instructions: the library routines carry a
// Payne-Hanek path and double-double arithmetic for arguments this code never sees, and Box-Muller was a quarter of the
// row kernel's VALU instructions.
template <class KC = BdfLiteral>
__device__ __forceinline__ void bdf_sincos2pi(double u, double &s, double &c)
{
    const double q = rint(4.0 * u);
    const double x = KC::c(6.283185307179586476925286766559) * fma(q, -0.25, u);
    const double z = x * x;
    const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, KC::c(1.58969099521155010221e-10), KC::c(-2.50507602534068634195e-08)),
                                                   KC::c(2.75573137070700676789e-06)), KC::c(-1.98412698298579493134e-04)),
                                     KC::c(8.33333333332248946124e-03)), KC::c(-1.66666666666666324348e-01));
    const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, KC::c(-1.13596475577881948265e-11), KC::c(2.08757232129817482790e-09)),
                                                   KC::c(-2.75573143513906633035e-07)), KC::c(2.48015872894767294178e-05)),
                                     KC::c(-1.38888888888741095749e-03)), KC::c(4.16666666666666019037e-02));
    const double sx = fma(x * z, ps, x);
    const double cx = fma(z * z, pc, fma(z, -0.5, 1.0));
    const int iq = (int)q & 3;
    const double sa = (iq & 1) ? cx : sx, ca = (iq & 1) ? sx : cx;
    s = (iq & 2) ? -sa : sa;
    c = (iq == 1 || iq == 2) ? -ca : ca;
}

// log(x) for a normal x in (0, 1) -- bdf_u01 never returns 0, 1 or a denormal: the fdlibm algorithm (x = 2^k m, m in
// [sqrt(2)/2, sqrt(2)), log m from s = f / (2 + f), f = m - 1), < 1 ulp, without the library routine's special cases
template <class KC = BdfLiteral>
__device__ __forceinline__ double bdf_log01(double x)
{
    int k;
    double m = frexp(x, &k);                        // m in [0.5, 1)
    if (m < KC::c(0.70710678118654752440)) { m *= 2.0; k -= 1; }
    const double f = m - 1.0, dk = (double)k;
    const double s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * fma(w, fma(w, KC::c(1.531383769920937332e-01), KC::c(2.222219843214978396e-01)), KC::c(3.999999999940941908e-01));
    const double t2 = z * fma(w, fma(w, fma(w, KC::c(1.479819860511658591e-01), KC::c(1.818357216161805012e-01)), KC::c(2.857142874366239149e-01)),
                              KC::c(6.666666666666735130e-01));
    const double R = t2 + t1, hfsq = 0.5 * f * f;
    return dk * KC::c(6.93147180369123816490e-01) - ((hfsq - fma(s, hfsq + R, dk * KC::c(1.90821492927058770002e-10))) - f);
}

// standard normal number `n` (0-based) of stream (purpose, entity, row): pair n/2, element n%2
__device__ __forceinline__ double bdf_normal(uint64_t seed, uint32_t sweep, uint32_t purpose, uint32_t entity,
                                    uint64_t row, int n)
{
    u32x4 o = bdf_draw(seed, sweep, purpose, entity, row, (uint32_t)(n >> 1));
    double u1 = bdf_u01(o.x, o.y), u2 = bdf_u01(o.z, o.w);
    double r = sqrt(-2.0 * bdf_log01(u1));
    double s, c;
    bdf_sincos2pi(u2, s, c);
    return (n & 1) ? r * s : r * c;
}

// the two normals of one draw of the generator (bdf_draw's four words): Box-Muller on its two uniforms.  Apart from bdf_normal_pair
// for a kernel that runs the generator's integer rounds and this transform in two places (k_rows_col.hip)
template <class KC = BdfLiteral>
__device__ __forceinline__ void bdf_normal_pair_of(u32x4 o, double &z0, double &z1)
{
    double u1 = bdf_u01(o.x, o.y), u2 = bdf_u01(o.z, o.w);
    double r = sqrt(-2.0 * bdf_log01<KC>(u1));
    double s, c;
    bdf_sincos2pi<KC>(u2, s, c);
    z0 = r * c;
    z1 = r * s;
}

// both normals of pair `pair` of the stream: numbers 2 pair and 2 pair + 1 (the same values bdf_normal returns)
template <class KC = BdfLiteral>
__device__ __forceinline__ void bdf_normal_pair(uint64_t seed, uint32_t sweep, uint32_t purpose, uint32_t entity,
                                       uint64_t row, uint32_t pair, double &z0, double &z1)
{
    bdf_normal_pair_of<KC>(bdf_draw(seed, sweep, purpose, entity, row, pair), z0, z1);
}

__device__ __forceinline__ double bdf_uniform(uint64_t seed, uint32_t sweep, uint32_t purpose, uint32_t entity,
                                     uint64_t row, uint32_t pair)
{
    u32x4 o = bdf_draw(seed, sweep, purpose, entity, row, pair);
    return bdf_u01(o.x, o.y);
}

// Gamma(a, 1), Marsaglia-Tsang, on the streams of the two given purposes (normals, uniforms); variate index g addresses the
// stream, the attempt is the pair
__device__ __forceinline__ double bdf_gamma_on(uint32_t p_normal, uint32_t p_uniform, uint64_t seed, uint32_t sweep, uint32_t entity,
                                               uint64_t g, double a)
{
    double boost = 1.0;
    if (a < 1.0) {
        boost = pow(bdf_uniform(seed, sweep, p_uniform, entity, g, 0xffffu), 1.0 / a);
        a += 1.0;
    }
    double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (uint32_t t = 0; t < 256; t++) {
        double x = bdf_normal(seed, sweep, p_normal, entity, g, (int)(2 * t));
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        double u = bdf_uniform(seed, sweep, p_uniform, entity, g, t);
        if (u < 1.0 - 0.0331 * (x * x) * (x * x)) return boost * d * v;
        if (log(u) < 0.5 * x * x + d * (1.0 - v + log(v))) return boost * d * v;
    }
    return boost * d;
}

// ... on the hyperprior's and sample_alpha's streams (BDF_P_GAMMA_N / BDF_P_GAMMA_U)
__device__ __forceinline__ double bdf_gamma(uint64_t seed, uint32_t sweep, uint32_t entity, uint64_t g, double a)
{
    return bdf_gamma_on(BDF_P_GAMMA_N, BDF_P_GAMMA_U, seed, sweep, entity, g, a);
}

// ---------------------------------------------------------------------------------------
// wave-level helpers (wave = 64 lanes)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double readlane_f64(double v, int lane)   // lane must be wave-uniform
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// the rows' hand-over to the hyperprior chain by counter (SampleArgs::done, rows.h; polled by k_hyper_chain)
#define BDF_DONE_SHARDS 64
#define BDF_DONE_STRIDE 16         // words between two shards

int bdf_predict_plain(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, double *out);
// bdf_predict_update for pairs stored sorted, two modes, D a multiple of 4 up to 32, no baseline (k_update_runs.hip): phase 0..2
int bdf_update_runs(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, int phase, double count,
                    double clamp_lo, double clamp_hi, double class_cut, double *stats_out);
// bdf_predict / bdf_predict_update / bdf_predict_sse for pairs with the probit link (k_probit.hip): phase -1 predict only (out),
// 0..2 the update (count: the pairs' counter before it), 3 statistics only; linear (nullable) overrides the pairs' baseline
int bdf_predict_link(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, const double *linear,
                     double *out, int phase, double count, double clamp_lo, double clamp_hi, double class_cut, double *stats_out);
// ... and what it hands the logistic (2) and the count link (3) to (k_pg.hip)
int bdf_predict_link_pg(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, const double *linear,
                        double *out, int phase, double count, double clamp_lo, double clamp_hi, double class_cut, double *stats_out);
