// k_foldin.hip -- cells of rows that were not in training, predicted from a few cells of their own (setNewObserved; DESIGN.md
// section 29).  Given one posterior draw (mu, Lambda, beta, V, alpha), a new row i with prior mean mu_i (mu + beta' f_i, or mu) and
// known cells K_i has
//   P_i = Lambda + alpha sum_{j in K_i} v_j v_j',   b_i = Lambda mu_i + alpha sum_{j in K_i} (y_ij - mean) v_j,   uhat_i = P_i^-1 b_i,
// u* | draw, y* ~ N(uhat_i, P_i^-1), and it is integrated out of the cell (i, j) in closed form (newrows.h):
//   y | draw ~ N(m, q_ij + 1 / alpha),   m = mean + uhat_i . v_j,   q_ij = v_j' P_i^-1 v_j = |L_i^-1 v_j|^2,   P_i = L_i L_i'.
// The new row's cells do not feed back into V: p(u* | y*, draw), the standard fold-in.
//
//   bdf_foldin_cells   the systems (P_i, b_i) by the row sampler's own accumulation in its dump mode, on a relation of the known
//                      cells (bdf_api.hip: bdf_foldin_systems_launch; long rows split and summed as every row launch does), the new
//                      rows in chunks under the scratch cap of bdf_sample_rows_nonneg; behind every chunk k_foldin_cells<DP>.
//   k_foldin_cells     a workgroup of four waves per new row.  In wave 0 wave_linalg.h factorises P_i (lane c holds column c) and leaves
//                      the factor packed by columns in LDS; two substitutions give uhat_i.  Then the row's test cells in batches of
//                      64, one lane per cell, the batches dealt to the four waves:
//                      the lane gathers v_j into registers and substitutes forward against the factor, column after column --
//                      every lane reads the same LDS address, which broadcasts -- adding p_k w_k^2 and uhat_i . v_j in index order.
//                      A system is one row's alone, so that nothing depends on the chunk.
//   bdf_foldin_solve   parity hook: k_foldin_cells alone on given systems in bdf_row_system's layout.
//
// Plain vector stores, no floating-point atomics, no scratch memory.
#include "bdf_common.h"
#include "rows.h"
#include "wave_linalg.h"

namespace {

struct FoldinArgs {
    int D, wide;                   // wide: D is even and V is 16-byte aligned -- a row of V by 16-byte loads
    const double *P, *b;           // system s: P + s D^2 (symmetric, every entry), b + s D
    const int32_t *rows;           // system s is new row rows[pos0 + s]; NULL: row s
    int64_t pos0;
    const int64_t *cell_ptr;       // per new row: its test cells in the pairs' storage order
    const int32_t *cols;           // per cell: its row of V
    int64_t n_cells;
    const double *V;
    double mean;
    double *m, *q, *uhat;
    int *flag;
};

// mu_chunk[s] = mu_rows[rows[pos0 + s]]: the prior means of a chunk's rows in the chunk's order
__global__ __launch_bounds__(256) void k_foldin_mu(int D, int64_t n, const int32_t *__restrict__ rows, int64_t pos0, const double *__restrict__ mu_rows,
                                                   double *__restrict__ mu_chunk)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * D) return;
    const int64_t s = e / D;
    mu_chunk[e] = mu_rows[(int64_t)rows[pos0 + s] * D + (e - s * D)];
}

// L w = v by columns against the unscaled factor Ah of wave_linalg.h (column k at tri + off(k), entry i at + i - k; rp[k] = 1 / p_k):
// z_k is final at step k, w_k = z_k / p_k in Ah's terms, and the square of element k of L^-1 v is p_k w_k^2 = z_k w_k, added in index
// order.  Every lane reads the same LDS addresses.  The steps are a compile-time recursion, so that every index of z is a constant
// (registers, no scratch memory); steps and chunks of eight rows behind D are skipped (uniform branches).  The compiler-only barrier
// keeps the reads of later columns from being hoisted over a step, which would hold hundreds of registers.
template <int DP, int K>
__device__ __forceinline__ void foldin_subst(double (&z)[DP], const double *tri, const double *rp, int D, double &q)
{
    if constexpr (K < DP) {
        if (K < D) {
            const double *ck = tri + WL<DP>::off(K) - K;           // ck[i] = Ah[i][K], i > K
            const double wk = z[K] * rp[K];
            q = fma(z[K], wk, q);
#pragma unroll
            for (int i0 = K + 1; i0 < DP; i0 += 8) {
                if (i0 < D) {
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        if (i0 + e < DP) z[i0 + e] = fma(-ck[i0 + e], wk, z[i0 + e]);
                }
            }
            asm volatile("" ::: "memory");
        }
        foldin_subst<DP, K + 1>(z, tri, rp, D, q);
    }
}

// A workgroup of four waves per new row.  Wave 0 factorises and solves; the factor, 1 / p and uhat_i go through LDS to all four, which
// then share the row's batches of 64 cells (a MovieLens user has up to two thousand: with one wave per row the longest row WAS the
// launch).  Which wave takes a cell does not change what is computed for it.
// Elements behind D: P is padded with the identity, b and v with zeros, so that they are zero operands of every sum.
template <int DP>
__global__ __launch_bounds__(256) void k_foldin_cells(FoldinArgs a)
{
    using W = WL<DP>;
    __shared__ double tri[W::TRI + 64];
    __shared__ double sRp[DP], sU[DP], sBad[1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), D = a.D;
    const int64_t s = blockIdx.x;
    const int64_t row = a.rows ? (int64_t)a.rows[a.pos0 + s] : s;
    if (wave == 0) {
        const int c = lane % DP;
        const double *P = a.P + s * D * D;
        double col[DP];
#pragma unroll
        for (int i = 0; i < DP; i++) {
            const bool in = i < D && c < D;
            const double v = P[in ? c * D + i : 0];
            col[i] = in ? v : (i == c ? 1.0 : 0.0);
        }
        double p_own, rp_own;
        const bool notpd = wl_factor<DP, true, true>(col, p_own, rp_own, tri, lane);      // (the same in every lane: all groups hold P_i)
        double u = c < D ? a.b[s * D + c] : 0.0;
        u = wl_forward<DP>(col, u, rp_own, lane);
        u = wl_backward<DP, true>(tri, u, rp_own, lane);
        if (notpd) u = NAN;
        if (lane < DP) {
            sRp[c] = rp_own;
            sU[c] = u;
            if (c < D) a.uhat[row * D + c] = u;
        }
        if (lane == 0) {
            sBad[0] = notpd ? 1.0 : 0.0;
            if (notpd) atomicOr_system(a.flag, 1);
        }
    }
    __syncthreads();
    const bool bad = sBad[0] != 0.0;

    const int64_t k_begin = a.cell_ptr[row], k_end = a.cell_ptr[row + 1];        // (cell_rows made them: inside the pairs)
    for (int64_t k0 = k_begin + 64 * wave; k0 < k_end; k0 += 256) {
        const int64_t kc = k0 + lane;
        const bool live = kc < k_end;
        const double *vr = a.V + (int64_t)a.cols[live ? kc : k_end - 1] * D;
        double z[DP];
        if (a.wide) {
#pragma unroll
            for (int d = 0; d < DP; d += 2) {
                double2 t = double2{0.0, 0.0};
                if (d < D) t = *(const double2 *)(vr + d);             // (uniform)
                z[d] = t.x; z[d + 1] = t.y;
            }
        } else {
#pragma unroll
            for (int d = 0; d < DP; d++) {
                double t = 0.0;
                if (d < D) t = vr[d];                                  // (uniform)
                z[d] = t;
            }
        }
        double dot = 0.0;
#pragma unroll
        for (int d0 = 0; d0 < DP; d0 += 8) {
            if (d0 < D) {                                              // (uniform)
#pragma unroll
                for (int e = 0; e < 8; e++) dot = fma(sU[d0 + e], z[d0 + e], dot);
            }
        }
        double q = 0.0;
        foldin_subst<DP, 0>(z, tri, sRp, D, q);
        if (live) {
            a.m[kc] = bad ? NAN : a.mean + dot;
            a.q[kc] = bad ? NAN : q;
        }
    }
}

int launch_cells(bdf_ctx *ctx, const FoldinArgs &a, int64_t n_sys)
{
    if (n_sys <= 0) return BDF_OK;
    const dim3 grid((unsigned)n_sys), block(256);
    const int DP = bdf_rows_dp(a.D);
    if (DP == 16) hipLaunchKernelGGL(k_foldin_cells<16>, grid, block, 0, ctx->stream, a);
    else if (DP == 32) hipLaunchKernelGGL(k_foldin_cells<32>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_foldin_cells<64>, grid, block, 0, ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

// The test cells as rows: the pairs are stored sorted by the new row (bdf_pairs_sort(pairs, 0)); n_new + 1 offsets into that order.
// Made once per pairs and dims, from the pairs' host copy; every id is checked against the dims here, so that the kernel's gathers
// and stores stay inside V, uhat and the planes.
int cell_rows(const char *who, bdf_pairs *p, int64_t n_new, int64_t M)
{
    if (p->foldin_ptr_dev && p->foldin_rows == n_new && p->foldin_cols == M) return BDF_OK;
    BDF_REQUIRE(p->n_modes == 2, BDF_ERR_ARG, "%s: the cells of new rows belong to a two-mode relation, not %d modes", who, p->n_modes);
    BDF_REQUIRE(p->n == 0 || p->sorted_mode == 0, BDF_ERR_ARG, "%s: the cells must be stored sorted by the new row (bdf_pairs_sort(pairs, 0))", who);
    const int64_t n = p->n;
    std::vector<int64_t> ptr((size_t)n_new + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        const size_t o = p->orig_host.empty() ? (size_t)i : (size_t)p->orig_host[(size_t)i];
        const int64_t r = p->ids_host[o], j = p->ids_host[(size_t)n + o];
        BDF_REQUIRE(r < n_new && j < M, BDF_ERR_BOUNDS, "%s: cell (%lld, %lld) is outside the %lld new rows x %lld rows of V", who, (long long)r + 1,
                    (long long)j + 1, (long long)n_new, (long long)M);
        ptr[(size_t)r + 1]++;
    }
    for (int64_t r = 0; r < n_new; r++) ptr[(size_t)r + 1] += ptr[(size_t)r];
    BDF_HIP(hipSetDevice(p->ctx->device));
    int rc = p->foldin_ptr_dev.upload(ptr);
    if (rc) return rc;
    p->foldin_rows = n_new; p->foldin_cols = M;
    return BDF_OK;
}

int common_checks(const char *who, const bdf_ctx *ctx, int D, int64_t n_new, const bdf_pairs *cells, const double *m_out, const double *q_out,
                  const double *uhat_out)
{
    BDF_REQUIRE(ctx && cells && uhat_out, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "%s: num_latent=%d must be in 1..%d", who, D, BDF_MAX_D);
    BDF_REQUIRE(n_new >= 1 && n_new < (int64_t)0x7fffffff, BDF_ERR_ARG, "%s: n_new=%lld must be positive and below 2^31", who, (long long)n_new);
    BDF_REQUIRE(cells->n == 0 || (m_out && q_out), BDF_ERR_ARG, "%s: %lld cells need m_out and q_out", who, (long long)cells->n);
    return BDF_OK;
}

void cell_args(FoldinArgs &a, bdf_ctx *ctx, int D, const bdf_pairs *cells, const double *V, double mean_value, double *m_out, double *q_out,
               double *uhat_out)
{
    a = {};
    a.D = D; a.wide = D % 2 == 0 && ((uintptr_t)V & 15) == 0;
    a.cell_ptr = cells->foldin_ptr_dev; a.cols = cells->ids_dev + cells->n; a.n_cells = cells->n;
    a.V = V; a.mean = mean_value; a.m = m_out; a.q = q_out; a.uhat = uhat_out; a.flag = ctx->flag_dev;
}

}  // namespace

extern "C" int bdf_foldin_cells(bdf_ctx *ctx, int D, int64_t n_new, const bdf_term *known, const double *mu, int mu_is_matrix, const double *Lambda,
                                bdf_pairs *cells, double mean_value, double *m_out, double *q_out, double *uhat_out)
{
    const char *who = "bdf_foldin_cells";
    int rc = common_checks(who, ctx, D, n_new, cells, m_out, q_out, uhat_out);
    if (rc) return rc;
    BDF_REQUIRE(known && known->rel && mu && Lambda, BDF_ERR_ARG, "%s: NULL argument", who);
    const bdf_rel *rel = known->rel;
    BDF_REQUIRE(rel->n_modes == 2 && (known->mode == 0 || known->mode == 1), BDF_ERR_ARG, "%s: the known cells belong to a two-mode relation", who);
    BDF_REQUIRE(!rel->sharded, BDF_ERR_ARG, "%s: a relation created with a layout (one rank only)", who);
    BDF_REQUIRE(rel->nint[known->mode] == n_new, BDF_ERR_ARG, "%s: the relation of the known cells has %lld rows for %lld new rows", who,
                (long long)rel->nint[known->mode], (long long)n_new);
    const double *V = known->factors[1 - known->mode];
    BDF_REQUIRE(V != nullptr, BDF_ERR_ARG, "%s: known->factors[%d] is NULL", who, 1 - known->mode);
    if ((rc = cell_rows(who, cells, n_new, rel->nint[1 - known->mode]))) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    // ONE scratch request (the block may move when it grows): the prior pack -- Lambda mu, or Lambda mu_i of a chunk's rows, and the
    // image of Lambda -- the chunk's prior means in its order, then the chunk's systems
    const int64_t chunk = std::min(bdf_nonneg_chunk_rows(ctx, D), n_new);
    const size_t nb = mu_is_matrix ? (size_t)chunk * D : (size_t)D, nimg = (size_t)bdf_prior_image_doubles(D), nmg = mu_is_matrix ? (size_t)chunk * D : 0;
    const size_t nhead = (nb + nimg + nmg + 1) / 2 * 2;
    void *pb;
    if ((rc = bdf_scratch(ctx, (nhead + (size_t)chunk * ((size_t)D * D + D)) * sizeof(double), &pb))) return rc;
    double *prior_b = (double *)pb, *prior_c = prior_b + nb, *mg = prior_c + nimg, *Ps = prior_b + nhead, *cs = Ps + (size_t)chunk * D * D;
    const int32_t *order = rel->idx[known->mode].order_dev;
    FoldinArgs a;
    cell_args(a, ctx, D, cells, V, mean_value, m_out, q_out, uhat_out);
    a.P = Ps; a.b = cs; a.rows = order;
    if (!mu_is_matrix && (rc = bdf_prior_launch(ctx, D, Lambda, mu, 1, 0, prior_b, prior_c))) return rc;
    for (int64_t k0 = 0; k0 < n_new; k0 += chunk) {
        const int64_t k1 = std::min(k0 + chunk, n_new), nk = k1 - k0;
        if (mu_is_matrix) {
            hipLaunchKernelGGL(k_foldin_mu, dim3((unsigned)((nk * D + 255) / 256)), dim3(256), 0, ctx->stream, D, nk, order, k0, mu, mg);
            BDF_HIP(hipGetLastError());
            if ((rc = bdf_prior_launch(ctx, D, Lambda, mg, nk, 1, prior_b, prior_c))) return rc;
        }
        if ((rc = bdf_foldin_systems_launch(ctx, D, n_new, known, mu_is_matrix ? mg : mu, mu_is_matrix, Lambda, prior_b, prior_c, k0, k1, Ps, cs))) return rc;
        a.pos0 = k0;
        if ((rc = launch_cells(ctx, a, nk))) return rc;
    }
    return BDF_OK;
}

extern "C" int bdf_foldin_solve(bdf_ctx *ctx, int D, int64_t n_new, const double *P, const double *b, bdf_pairs *cells, int64_t M, const double *V,
                                double mean_value, double *m_out, double *q_out, double *uhat_out)
{
    const char *who = "bdf_foldin_solve";
    int rc = common_checks(who, ctx, D, n_new, cells, m_out, q_out, uhat_out);
    if (rc) return rc;
    BDF_REQUIRE(P && b && (V || cells->n == 0) && M >= 0, BDF_ERR_ARG, "%s: NULL argument", who);
    if ((rc = cell_rows(who, cells, n_new, M))) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    FoldinArgs a;
    cell_args(a, ctx, D, cells, V, mean_value, m_out, q_out, uhat_out);
    a.P = P; a.b = b;
    return launch_cells(ctx, a, n_new);
}
