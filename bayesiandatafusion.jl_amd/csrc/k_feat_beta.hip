// k_feat_beta.hip -- K2..K5: the beta update.
//
//   rhs  = F'((sample - mu)' + E1) + sqrt(lb) E2       sample_beta, src/sampling.jl:298-300
//   beta = (F'F + lb I) \ rhs                          solve_full :314-320 | solve_cg2 parallel_matrix.jl:488-507
//   all D conjugate-gradient solves advance together, each column keeping the reference's own stopping rule
//   (cg_AtA, src/parallel_cg.jl:63-94: stop when ||r|| < tol ||b||, checked before an iteration; maxiter).
//   lambda_beta ~ Gamma                                sample_lambda_beta, src/sampling.jl:136-142
#include "feat.h"
#include "wave_linalg.h"
#include <algorithm>
#include <cmath>

namespace {

// ---- noise rows e ~ N(0, Lambda^-1) = chol(inv(Lambda))' z  (sampling.jl:298-300) ----------------------------------
// step 1 (one wave): factor the index-reversed Lambda (wave_linalg.h): Lr = [Ah rows, masked | 1/p | sqrt(p)]
template <int DP>
__global__ __launch_bounds__(64) void k_noise_prep(int D, const double *Lambda, double *Lr, int *flag)
{
    __shared__ double tri[WL<DP>::TRI + 64];
    const int lane = threadIdx.x;
    const int c = lane % DP;
    const int ej = D - 1 - c;
    double col[DP];
#pragma unroll
    for (int i = 0; i < DP; i++) {
        const int ei = D - 1 - i;
        double w = (i == c) ? 1.0 : 0.0;
        if (ei >= 0 && ej >= 0) {
            const int lo = ei < ej ? ei : ej, hi = ei < ej ? ej : ei;    // Symmetric(Lambda): upper triangle
            w = Lambda[lo + (int64_t)hi * D];
        }
        col[i] = w;
    }
    double p_own, rp_own;
    if (wl_factor<DP, true>(col, p_own, rp_own, tri, lane) && lane == 0) atomicOr_system(flag, 4);
    if (lane < DP) {
#pragma unroll
        for (int k = 0; k < DP; k++) Lr[c * DP + k] = col[k];
        Lr[DP * DP + c] = rp_own;
        Lr[DP * DP + DP + c] = p_own * fast_rsqrt(p_own);
    }
}

// step 2: T[:,i] = (sample[:,i] - mu) + e_i   (sample == NULL: T[:,i] = scale * e_i);
// e solves U' e = z, i.e. L~' e~ = z~ in reversed coordinates:  e~_j = (sqrt(p_j) z~_j - sum_{m>j} Ah[m][j] e~_m) / p_j
constexpr int NOISE_RPW = 16;       // rows per workgroup of k_noise_rows
template <int DP>
__global__ __launch_bounds__(256) void k_noise_rows(int D, int64_t n, const double *Lr, const double *sample,
                                                     const double *mu, const double *scale_sq, uint64_t seed,
                                                     uint32_t sweep, uint32_t purpose, uint32_t entity, double *T,
                                                     const int32_t *__restrict__ row_ids)
{
    // row_ids (nullable): the row's ORIGINAL id, which keys its noise stream (rows stored at internal positions when several
    // GPUs share the entity); negative = a row nobody owns: no noise (its feature row is zero)
    // NOISE_RPW rows per workgroup.  Phase 1, all 256 threads: the rows' normals (a Philox block + log + sin/cos per pair is ~40x
    // the arithmetic of the solve: one or two pairs per thread, so that 500 rows already fill 32 workgroups), scaled by
    // sqrt(p_j), into LDS.  Phase 2, DP lanes per row: the substitution.
    __shared__ double sL[DP * DP + 2 * DP];
    __shared__ double sz[NOISE_RPW][DP + 1];
    const int tid = threadIdx.x;
    for (int e = tid; e < DP * DP + 2 * DP; e += 256) sL[e] = Lr[e];
    const int64_t r0 = (int64_t)blockIdx.x * NOISE_RPW;
    const int npairs = (D + 1) / 2;
    for (int e = tid; e < NOISE_RPW * DP; e += 256) sz[e / DP][e % DP] = 0.0;
    __syncthreads();
    for (int e = tid; e < NOISE_RPW * npairs; e += 256) {
        const int lr = e / npairs, pr = e % npairs;
        const int64_t i = r0 + lr;
        if (i >= n) continue;
        const int64_t rid = row_ids ? (int64_t)row_ids[i] : i;
        if (rid < 0) continue;
        const u32x4 o = bdf_draw(seed, sweep, purpose, entity, (uint64_t)rid, (uint32_t)pr);
        const double u1 = bdf_u01(o.x, o.y), u2 = bdf_u01(o.z, o.w);
        const double r = sqrt(-2.0 * log(u1)), t = 6.283185307179586476925286766559 * u2;
        // normal number ej of the row belongs to reversed position j = D - 1 - ej
        const int e0 = 2 * pr, e1 = 2 * pr + 1;
        sz[lr][D - 1 - e0] = r * cos(t) * sL[DP * DP + DP + (D - 1 - e0)];
        if (e1 < D) sz[lr][D - 1 - e1] = r * sin(t) * sL[DP * DP + DP + (D - 1 - e1)];
    }
    __syncthreads();
    // the substitution, DP lanes per row (lane = reversed position): as soon as e~_j is final every lane m < j takes its term
    // Ah[j][m] e~_j -- one broadcast and one fma per step instead of a dot product walked by a single thread per row
    const int sub = tid % DP, grp = tid / DP;
    const double scale = scale_sq ? sqrt(*scale_sq) : 1.0;
    for (int lr = grp; lr < NOISE_RPW; lr += 256 / DP) {
        const int64_t i = r0 + lr;
        if (i >= n) break;
        double sv = sz[lr][sub];
        for (int j = DP - 1; j >= 0; j--) {
            const double ej = __shfl(sv, j, DP) * sL[DP * DP + j];
            if (sub == j) sv = ej;
            else if (sub < j) sv = fma(-sL[j * DP + sub], ej, sv);
        }
        const int ej = D - 1 - sub;
        if (ej >= 0) {
            const int64_t off = i * D + ej;
            T[off] = sample ? (sample[off] - mu[ej]) + sv : scale * sv;
        }
    }
}

template <int DP>
int noise_rows(bdf_ctx *ctx, int D, int64_t n, const double *Lambda, double *Lr, const double *sample, const double *mu,
               const double *scale_sq, uint32_t purpose, uint32_t entity, double *T, bool prep, const int32_t *row_ids = nullptr)
{
    if (prep) {
        hipLaunchKernelGGL(k_noise_prep<DP>, dim3(1), dim3(64), 0, ctx->stream, D, Lambda, Lr, ctx->flag_dev);
        BDF_HIP(hipGetLastError());
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_noise_rows<DP>, dim3((unsigned)((n + NOISE_RPW - 1) / NOISE_RPW)), dim3(256), 0, ctx->stream, D, n, Lr,
                           sample, mu, scale_sq, ctx->seed, ctx->sweep_host, purpose, entity, T, row_ids);
        BDF_HIP(hipGetLastError());
    }
    return BDF_OK;
}

// rhs(f,d) = FtT(f,d) + E2s(d,f)   (E2s is D x numF: row f of the noise is contiguous)
__global__ void k_add_e2(int64_t numF, int D, const double *E2s, double *rhs)
{
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= numF * D) return;
    const int64_t f = idx % numF;
    const int d = (int)(idx / numF);
    rhs[idx] += E2s[f * D + d];
}

// ---- beta' beta, trace(beta'beta Lambda), lambda_beta ~ Gamma ----------------------------------------------------
__global__ void k_tinv_feat(int D, const double *G, const double *WI, const double *lambda_beta, double *Tinv)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < D * D) Tinv[e] = WI[e] + G[e] * (*lambda_beta);      // Tinv += beta'beta * lambda_beta, macau.jl:128
}

__global__ __launch_bounds__(64) void k_lambda_beta(int D, int64_t numF, const double *G, const double *Lambda, double nu,
                                                    double mu, uint64_t seed, uint32_t sweep, uint32_t entity,
                                                    double *lambda_beta)
{
    // trace((beta'beta) Lambda) = sum_ij G[i][j] Lambda[j][i]
    double tr = 0.0;
    for (int e = threadIdx.x; e < D * D; e += 64) {
        const int i = e % D, j = e / D;
        tr = fma(G[i + j * D], Lambda[j + i * D], tr);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) tr += __shfl_xor(tr, off);
    if (threadIdx.x == 0) {
        const double nux = nu + (double)numF * (double)D;
        const double mux = mu * nux / (nu + mu * tr);
        *lambda_beta = bdf_gamma(seed, sweep, entity, (uint64_t)D, 0.5 * nux) * (2.0 * mux / nux);
    }
}

// ---- direct solve for numF <= 64: (FF + lambda I) X = RHS on one wave (solve_full, sampling.jl:314-320) -------------
template <int DP>
__global__ __launch_bounds__(64) void k_solve_small(int n, int ncol, const double *FF, const double *lambda_p,
                                                    const double *rhs, double *X, int *flag)
{
    __shared__ double tri[WL<DP>::TRI + 64];
    const int lane = threadIdx.x;
    const int c = lane % DP;
    const double lambda = *lambda_p;
    double rowm[DP];
#pragma unroll
    for (int i = 0; i < DP; i++) {
        double w = (i == c) ? 1.0 : 0.0;
        if (i < n && c < n) w = FF[i + (int64_t)c * n] + ((i == c) ? lambda : 0.0);
        rowm[i] = w;
    }
    double p_own, rp_own;
    if (wl_factor<DP, true>(rowm, p_own, rp_own, tri, lane) && lane == 0) atomicOr_system(flag, 8);
    for (int q = 0; q < ncol; q++) {
        double b = (lane < DP && c < n) ? rhs[c + (int64_t)q * n] : 0.0;
        b = wl_forward<DP>(rowm, b, rp_own, lane);       // b' = wh p;  yh = w sqrt(p) = b'
        b = wl_backward<DP, true>(tri, b, rp_own, lane);
        if (lane < DP && c < n) X[c + (int64_t)q * n] = b;
    }
}

// G = X' X (D x D) for a column-major numF x D matrix X (beta), through the split-K product
int beta_gram(bdf_ctx *ctx, int D, int64_t numF, const double *X, double *G)
{
    GemmArgs g;
    g.M = D; g.N = D; g.K = numF; g.A = X; g.ars = numF; g.acs = 1; g.B = X; g.brs = 1; g.bcs = numF;
    g.C = G; g.crs = 1; g.ccs = D; g.bias = nullptr; g.C2 = nullptr;
    return feat_gemm(ctx, g);
}

}  // namespace

extern "C" int bdf_hyper_feature_terms(bdf_ctx *ctx, int D, int64_t numF, const double *beta, const double *WI,
                                       const double *lambda_beta_dev, double *Tinv_out)
{
    BDF_REQUIRE(ctx && beta && WI && lambda_beta_dev && Tinv_out, BDF_ERR_ARG, "bdf_hyper_feature_terms: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_hyper_feature_terms: bad num_latent");
    void *G;
    int rc = bdf_scratch(ctx, (size_t)D * D * sizeof(double), &G);
    if (rc) return rc;
    if ((rc = beta_gram(ctx, D, numF, beta, (double *)G))) return rc;
    hipLaunchKernelGGL(k_tinv_feat, dim3((D * D + 255) / 256), dim3(256), 0, ctx->stream, D, (const double *)G, WI,
                       lambda_beta_dev, Tinv_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_sample_beta(bdf_ctx *ctx, const bdf_feat *fc, int D, const double *sample, const double *mu,
                               const double *Lambda, double *lambda_beta_dev, int use_ff, double tol, int maxiter,
                               int sample_lambda, double lb_nu, double lb_mu, uint32_t entity_tag,
                               double *beta_out, double *rhs_out, int32_t *iters_out)
{
    return bdf_sample_beta_ranks(ctx, nullptr, fc, D, sample, mu, Lambda, lambda_beta_dev, use_ff, tol, maxiter, sample_lambda, lb_nu,
                                 lb_mu, entity_tag, beta_out, rhs_out, iters_out);
}

// Several ranks (comm != NULL, conjugate gradients): the D solves are shared out as solve_cg2 shares them over its workers
// (src/parallel_matrix.jl:488-507): every rank forms the whole right-hand side (the same noise streams on every rank: one
// product with F'), solves a contiguous block of ceil(D / P) columns and the blocks are all-gathered.  A column's iterates do
// not depend on which other columns are solved beside it, so beta is the one a single rank computes.  The direct solve
// handles all D right-hand sides in one factorisation and stays whole.
extern "C" int bdf_sample_beta_ranks(bdf_ctx *ctx, bdf_comm *comm, const bdf_feat *fc, int D, const double *sample, const double *mu,
                                     const double *Lambda, double *lambda_beta_dev, int use_ff, double tol, int maxiter,
                                     int sample_lambda, double lb_nu, double lb_mu, uint32_t entity_tag,
                                     double *beta_out, double *rhs_out, int32_t *iters_out)
{
    BDF_REQUIRE(ctx && fc && sample && mu && Lambda && lambda_beta_dev && beta_out, BDF_ERR_ARG, "bdf_sample_beta: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_sample_beta: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    bdf_feat *f = const_cast<bdf_feat *>(fc);
    const int64_t N = f->m, numF = f->n;
    if (std::isnan(tol)) tol = 2.220446049250313e-16 * (double)numF;       // eps()*numF, sampling.jl:294-296
    if (maxiter <= 0) maxiter = (int)numF;
    const int DP = D <= 16 ? 16 : (D <= 32 ? 32 : 64);

    // scratch layout (doubles): Lr | T (D x N) | E2s (D x numF) | rhs | R P Z Tm | scalars
    size_t nLr = (size_t)DP * DP + 2 * DP, nT = (size_t)D * N, nE2 = (size_t)D * numF, nB = (size_t)numF * D, nTm = (size_t)N * D;
    size_t total = nLr + nT + nE2 + nB * 4 + nTm + 3 * (size_t)D + 64 + (size_t)D * D;
    void *sv;
    int rc = bdf_scratch(ctx, total * sizeof(double) + (2 * (size_t)D + 16) * sizeof(int), &sv);      // ints: active D | iters D | nactive | done
    if (rc) return rc;
    double *Lr = (double *)sv, *T = Lr + nLr, *E2s = T + nT, *rhs = E2s + nE2, *R = rhs + nB, *P = R + nB, *Z = P + nB,
           *Tm = Z + nB, *scal = Tm + nTm, *G = scal + 3 * D + 64;
    int *ints = (int *)(G + (size_t)D * D);

    // rhs = F'((sample - mu)' + E1) + sqrt(lb) E2
#define NOISE(DPV)                                                                                                      \
    do {                                                                                                                \
        if ((rc = noise_rows<DPV>(ctx, D, N, Lambda, Lr, sample, mu, nullptr, BDF_P_BETA_E1, entity_tag, T, true, f->row_ids_dev))) return rc; \
        if ((rc = noise_rows<DPV>(ctx, D, numF, Lambda, Lr, nullptr, nullptr, lambda_beta_dev, BDF_P_BETA_E2, entity_tag, E2s, false))) return rc; \
    } while (0)
    if (DP == 16) NOISE(16); else if (DP == 32) NOISE(32); else NOISE(64);
#undef NOISE
    // T holds (target)' as D x N: element (i,d) at T[i*D + d]
    if ((rc = feat_apply(ctx, f, true, T, D, 1, D, rhs, 1, numF))) return rc;
    if (numF * D > 0) {
        hipLaunchKernelGGL(k_add_e2, dim3((unsigned)((numF * D + 255) / 256)), dim3(256), 0, ctx->stream, numF, D, E2s, rhs);
        BDF_HIP(hipGetLastError());
    }
    if (rhs_out) BDF_HIP(hipMemcpyAsync(rhs_out, rhs, nB * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));

    if (use_ff && (rc = feat_ensure_FF(f))) return rc;
    if (use_ff) {
        // solve_full (sampling.jl:314-320): a direct solve, Cholesky on one wave up to 64 features, blocked on the matrix cores above
        if (numF <= 16) hipLaunchKernelGGL(k_solve_small<16>, dim3(1), dim3(64), 0, ctx->stream, (int)numF, D, f->FF_dev, lambda_beta_dev, rhs, beta_out, ctx->flag_dev);
        else if (numF <= 32) hipLaunchKernelGGL(k_solve_small<32>, dim3(1), dim3(64), 0, ctx->stream, (int)numF, D, f->FF_dev, lambda_beta_dev, rhs, beta_out, ctx->flag_dev);
        else if (numF <= 64) hipLaunchKernelGGL(k_solve_small<64>, dim3(1), dim3(64), 0, ctx->stream, (int)numF, D, f->FF_dev, lambda_beta_dev, rhs, beta_out, ctx->flag_dev);
        else if (numF <= BDF_EIG_MAX && !getenv("BDF_NO_EIG")) { if ((rc = feat_eig_solve(ctx, f, D, lambda_beta_dev, rhs, beta_out))) return rc; }
        else if ((rc = bdf_chol_solve(ctx, f, D, lambda_beta_dev, rhs, beta_out))) return rc;
        BDF_HIP(hipGetLastError());
        if (iters_out) BDF_HIP(hipMemsetAsync(iters_out, 0, D * sizeof(int32_t), ctx->stream));
    } else {
        // D simultaneous cg_AtA solves (solve_cg2, parallel_matrix.jl:488-507).  The operator p -> F'(F p) is applied as
        // (F'F) p when F'F is small and cheaper than the two products (numF <= 1024 and numF^2 <= nnz(F): C3's 6040 x 500
        // dense F: 2 MB read per iteration instead of 2 x 24 MB) -- the same operator, formed once per feature matrix
        const bool ff_op = numF > 0 && numF <= 1024 && numF * numF <= f->nnz;
        if (ff_op && (rc = feat_ensure_FF(f))) return rc;
        int *cg_iters = nullptr;
        int rank = 0, world = 1;
        if (comm && (rc = bdf_comm_size(comm, &rank, &world))) return rc;
        if (world <= 1) {
            if ((rc = feat_cg_solve(ctx, f, ff_op, D, lambda_beta_dev, rhs, beta_out, tol, maxiter, R, P, Z, Tm, scal, ints, &cg_iters, E2s))) return rc;      // (E2s: free once rhs is formed)
            if (iters_out) BDF_HIP(hipMemcpyAsync(iters_out, cg_iters, D * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            // this rank's block of columns, solved into its place of a gather buffer of world blocks (>= D columns), then the
            // exchange; the iteration counts travel behind each block's columns
            const int nc = (D + world - 1) / world, c0 = rank * nc, mine = std::max(0, std::min(nc, D - c0));
            const size_t blk = (size_t)nc * numF * sizeof(double) + (size_t)nc * sizeof(int32_t);
            if (int rcg = f->gather_dev.grow(blk * (size_t)world, ctx->stream)) return rcg;
            char *gb = (char *)f->gather_dev.get();
            double *my_beta = (double *)(gb + (size_t)rank * blk);
            int32_t *my_iters = (int32_t *)(gb + (size_t)rank * blk + (size_t)nc * numF * sizeof(double));
            BDF_HIP(hipMemsetAsync(my_beta, 0, blk, ctx->stream));
            if (mine > 0) {
                if ((rc = feat_cg_solve(ctx, f, ff_op, mine, lambda_beta_dev, rhs + (size_t)c0 * numF, my_beta, tol, maxiter, R, P, Z, Tm, scal, ints, &cg_iters, E2s))) return rc;
                BDF_HIP(hipMemcpyAsync(my_iters, cg_iters, (size_t)mine * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
            }
            if ((rc = bdf_allgather_block(ctx, comm, gb, blk)) || (rc = bdf_allgather_join(ctx, comm))) return rc;
            for (int r = 0; r < world; r++) {
                const int rc0 = r * nc, rn = std::max(0, std::min(nc, D - rc0));
                if (rn <= 0) break;
                BDF_HIP(hipMemcpyAsync(beta_out + (size_t)rc0 * numF, gb + (size_t)r * blk, (size_t)rn * numF * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
                if (iters_out)
                    BDF_HIP(hipMemcpyAsync(iters_out + rc0, gb + (size_t)r * blk + (size_t)nc * numF * sizeof(double), (size_t)rn * sizeof(int32_t),
                                           hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
    }
    if (sample_lambda) {
        if ((rc = beta_gram(ctx, D, numF, beta_out, G))) return rc;
        hipLaunchKernelGGL(k_lambda_beta, dim3(1), dim3(64), 0, ctx->stream, D, numF, (const double *)G, Lambda, lb_nu, lb_mu,
                           ctx->seed, ctx->sweep_host, entity_tag, lambda_beta_dev);
        BDF_HIP(hipGetLastError());
    }
    return BDF_OK;
}

// ---- relation-level side information (sample_beta_rel, src/sampling.jl:322-337) and alpha (sample_alpha, :129-134) -----
__global__ void k_rel_target(int64_t N, int64_t first_obs, const double *values, const double *pred, double inv_sqrt_alpha,
                             const double *alpha_dev, uint64_t seed, uint32_t sweep, uint32_t tag, double *v)
{
    if (alpha_dev) inv_sqrt_alpha = 1.0 / sqrt(*alpha_dev);          // (alpha sampled on the device: the same two IEEE operations as the host's)
    // v = (values - udot - mean) + alpha^-1/2 z,  pred = udot + mean; the noise is keyed by the observation's place in the relation
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) v[i] = (values[i] - pred[i]) + inv_sqrt_alpha * bdf_normal(seed, sweep, BDF_P_BETA_REL1, tag, (uint64_t)(first_obs + i), 0);
}

__global__ void k_rel_rhs(int64_t numF, double alpha, const double *alpha_dev, double lambda, uint64_t seed, uint32_t sweep, uint32_t tag,
                          double *rhs, double *rhs_scaled, double *lam_scaled)
{
    if (alpha_dev) alpha = *alpha_dev;
    // aFt_y = alpha F'v + sqrt(lambda) z;  the solve runs on (FF + (lambda / alpha) I) beta = aFt_y / alpha
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < numF) {
        const double r = alpha * rhs[f] + sqrt(lambda) * bdf_normal(seed, sweep, BDF_P_BETA_REL2, tag, (uint64_t)f, 0);
        rhs[f] = r;
        rhs_scaled[f] = r / alpha;
    }
    if (f == 0) *lam_scaled = lambda / alpha;
}

__global__ void k_add_scalar(int64_t n, double a, double *x)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] += a;
}

__global__ void k_sample_alpha(double lambda0, double nu0, double n, const double *sumsq, uint64_t seed, uint32_t sweep,
                               uint32_t tag, double *alpha_out)
{
    // Wishart(nu0 + n, SW) in one dimension: SW * chi2(nu0 + n) = SW * 2 Gamma((nu0 + n) / 2)
    const double SW = 1.0 / (1.0 / lambda0 + *sumsq);
    *alpha_out = SW * 2.0 * bdf_gamma(seed, sweep, tag, 0, 0.5 * (nu0 + n));
}

extern "C" int bdf_feat_linear(bdf_ctx *ctx, const bdf_feat *f, const double *beta, double mean_value, double *out)
{
    // out = mean_value + F beta (one column): linear_values of macau.jl:91, and the test rows' baseline of pred(r, probe, F)
    BDF_REQUIRE(ctx && f && beta && out, BDF_ERR_ARG, "bdf_feat_linear: NULL argument");
    int rc = feat_apply(ctx, f, false, beta, 1, f->n, 1, out, 1, f->m);
    if (rc) return rc;
    if (f->m > 0) {
        hipLaunchKernelGGL(k_add_scalar, dim3((unsigned)((f->m + 255) / 256)), dim3(256), 0, ctx->stream, f->m, mean_value, out);
        BDF_HIP(hipGetLastError());
    }
    return BDF_OK;
}

extern "C" int bdf_sample_alpha(bdf_ctx *ctx, double alpha_lambda0, double alpha_nu0, int64_t n, const double *sumsq_err,
                                uint32_t rel_tag, double *alpha_out)
{
    BDF_REQUIRE(ctx && sumsq_err && alpha_out, BDF_ERR_ARG, "bdf_sample_alpha: NULL argument");
    hipLaunchKernelGGL(k_sample_alpha, dim3(1), dim3(1), 0, ctx->stream, alpha_lambda0, alpha_nu0, (double)n, sumsq_err,
                       ctx->seed, ctx->sweep_host, 0x800000u | rel_tag, alpha_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

// several ranks: x (n doubles) := the sum of the ranks' x, block after block in rank order (every rank ends with the same
// bits); gb: world * n doubles of scratch
__global__ void k_sum_blocks(int64_t n, int world, const double *gb, double *x)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int r = 0; r < world; r++) s += gb[(size_t)r * n + i];
    x[i] = s;
}

static int sum_ranks_in(bdf_ctx *ctx, bdf_comm *comm, int rank, int world, double *x, int64_t n, double *gb)
{
    static const bool force = getenv("BDF_FORCE_COMM") != nullptr;      // (one rank through the collective all the same: tools/soak_determinism.py rccl)
    if ((world <= 1 && !(force && comm)) || n <= 0) return BDF_OK;
    int rc;
    BDF_HIP(hipMemcpyAsync(gb + (size_t)rank * n, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = bdf_allgather_block(ctx, comm, gb, (size_t)n * sizeof(double))) || (rc = bdf_allgather_join(ctx, comm))) return rc;
    hipLaunchKernelGGL(k_sum_blocks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, world, (const double *)gb, x);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

// (internal) the same with the caller's gather buffer (world * n doubles): for callers that hold the context's scratch themselves
int bdf_sum_ranks_into(bdf_ctx *ctx, bdf_comm *comm, double *x, int64_t n, double *gather)
{
    int rank = 0, world = 1, rc;
    if (comm && (rc = bdf_comm_size(comm, &rank, &world))) return rc;
    return sum_ranks_in(ctx, comm, rank, world, x, n, gather);
}

extern "C" int bdf_sum_ranks(bdf_ctx *ctx, bdf_comm *comm, double *x, int64_t n)
{
    BDF_REQUIRE(ctx && x && n >= 0, BDF_ERR_ARG, "bdf_sum_ranks: NULL argument or negative length");
    int rank = 0, world = 1, rc;
    if (comm && (rc = bdf_comm_size(comm, &rank, &world))) return rc;
    if (world <= 1) return BDF_OK;
    void *sv;
    if ((rc = bdf_scratch(ctx, (size_t)world * (size_t)n * sizeof(double), &sv))) return rc;
    return sum_ranks_in(ctx, comm, rank, world, x, n, (double *)sv);
}

extern "C" int bdf_sample_beta_rel(bdf_ctx *ctx, const bdf_feat *fc, const bdf_pairs *train, int D,
                                   const double *const *factors, double mean_value, double alpha, double lambda_beta,
                                   uint32_t rel_tag, double *beta_out, double *linear_out, double *rhs_out)
{
    return bdf_sample_beta_rel_ranks(ctx, nullptr, fc, train, 0, D, factors, mean_value, alpha, lambda_beta, rel_tag, beta_out,
                                     linear_out, rhs_out);
}

extern "C" int bdf_sample_beta_rel_ranks(bdf_ctx *ctx, bdf_comm *comm, const bdf_feat *fc, const bdf_pairs *train,
                                         int64_t first_obs, int D, const double *const *factors, double mean_value, double alpha,
                                         double lambda_beta, uint32_t rel_tag, double *beta_out, double *linear_out, double *rhs_out)
{
    return bdf_sample_beta_rel_impl(ctx, comm, fc, train, first_obs, D, factors, mean_value, alpha, nullptr, lambda_beta, rel_tag, beta_out,
                                    linear_out, rhs_out);
}

// (alpha_dev, nullable: the relation's precision in device memory -- sampled there inside bdf_gibbs_sweep -- instead of `alpha`)
int bdf_sample_beta_rel_impl(bdf_ctx *ctx, bdf_comm *comm, const bdf_feat *fc, const bdf_pairs *train, int64_t first_obs, int D,
                             const double *const *factors, double mean_value, double alpha, const double *alpha_dev, double lambda_beta,
                             uint32_t rel_tag, double *beta_out, double *linear_out, double *rhs_out)
{
    BDF_REQUIRE(ctx && fc && train && factors && beta_out && linear_out, BDF_ERR_ARG, "bdf_sample_beta_rel: NULL argument");
    BDF_REQUIRE((alpha_dev || alpha > 0.0) && lambda_beta >= 0.0, BDF_ERR_ARG, "bdf_sample_beta_rel: alpha must be positive, lambda_beta >= 0");
    BDF_REQUIRE(first_obs >= 0, BDF_ERR_ARG, "bdf_sample_beta_rel: first_obs must not be negative");
    int rank = 0, world = 1;
    if (comm) { int rcw = bdf_comm_size(comm, &rank, &world); if (rcw) return rcw; }
    bdf_feat *f = const_cast<bdf_feat *>(fc);
    const int64_t N = f->m, numF = f->n;
    BDF_REQUIRE(train->n == N, BDF_ERR_ARG,
                "bdf_sample_beta_rel: the relation has %lld observations but its feature matrix has %lld rows (DimensionMismatch)",
                (long long)train->n, (long long)N);
    const uint32_t tag = 0x800000u | rel_tag;
    // scratch (doubles): pred N | v N | t numF | rs numF | R P Z (numF each) | Tm N | scal 4 | lam 1, then ints
    // several ranks: this rank holds the rows [first_obs, first_obs + N) of the relation's feature matrix and the same
    // observations as pairs; F'v and (once) F'F are summed over the ranks in rank order, the solve is repeated on every rank
    const bool sum_ff = world > 1 && !f->FF_summed;
    const size_t gsz = world > 1 ? (size_t)world * (size_t)(sum_ff ? numF * numF : numF) : 0;
    const size_t total = 3 * (size_t)N + 5 * (size_t)numF + 16 + gsz;
    void *sv;
    int rc = bdf_scratch(ctx, total * sizeof(double) + 16 * sizeof(int), &sv);
    if (rc) return rc;
    double *pred = (double *)sv, *v = pred + N, *t = v + N, *rs = t + numF, *R = rs + numF, *P = R + numF, *Z = P + numF,
           *Tm = Z + numF, *scal = Tm + N, *lam = scal + 8, *gb = lam + 8;
    (void)R; (void)P; (void)Z; (void)Tm;
    if ((rc = bdf_predict_plain(ctx, train, D, factors, mean_value, pred))) return rc;
    if (N > 0) {
        hipLaunchKernelGGL(k_rel_target, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, N, first_obs,
                           (const double *)train->values_dev, (const double *)pred, 1.0 / sqrt(alpha), alpha_dev, ctx->seed,
                           ctx->sweep_host, tag, v);
        BDF_HIP(hipGetLastError());
    }
    if ((rc = feat_apply(ctx, f, true, v, 1, N, 1, t, 1, numF))) return rc;
    if ((rc = sum_ranks_in(ctx, comm, rank, world, t, numF, gb))) return rc;
    hipLaunchKernelGGL(k_rel_rhs, dim3((unsigned)((numF + 255) / 256)), dim3(256), 0, ctx->stream, numF, alpha, alpha_dev, lambda_beta,
                       ctx->seed, ctx->sweep_host, tag, t, rs, lam);
    BDF_HIP(hipGetLastError());
    if (rhs_out) BDF_HIP(hipMemcpyAsync(rhs_out, t, numF * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = feat_ensure_FF(f))) return rc;
    if (sum_ff) {
        if ((rc = sum_ranks_in(ctx, comm, rank, world, f->FF_dev, numF * numF, gb))) return rc;
        f->FF_summed = true;
    }
    if (numF <= 16) hipLaunchKernelGGL(k_solve_small<16>, dim3(1), dim3(64), 0, ctx->stream, (int)numF, 1, f->FF_dev, lam, rs, beta_out, ctx->flag_dev);
    else if (numF <= 32) hipLaunchKernelGGL(k_solve_small<32>, dim3(1), dim3(64), 0, ctx->stream, (int)numF, 1, f->FF_dev, lam, rs, beta_out, ctx->flag_dev);
    else if (numF <= 64) hipLaunchKernelGGL(k_solve_small<64>, dim3(1), dim3(64), 0, ctx->stream, (int)numF, 1, f->FF_dev, lam, rs, beta_out, ctx->flag_dev);
    else if ((rc = bdf_chol_solve(ctx, f, 1, lam, rs, beta_out))) return rc;
    BDF_HIP(hipGetLastError());
    // linear_values = mean_value + F beta (macau.jl:91)
    if ((rc = feat_apply(ctx, f, false, beta_out, 1, numF, 1, linear_out, 1, N))) return rc;
    if (N > 0) {
        hipLaunchKernelGGL(k_add_scalar, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, N, mean_value, linear_out);
        BDF_HIP(hipGetLastError());
    }
    return BDF_OK;
}
