// bdf_hmc.hip -- C ABI of Hamiltonian Monte Carlo BPMF (src/macau_hmc.jl): the host-side set-up that macau_hmc does in
// Julia (reset!, the CSR of both modes through two_mode.hip, HMCModel's mass) and the iteration loop, enqueued on the
// context's stream.  The kernels are in k_hmc.hip; the prior reuses bdf_hyper_sums / bdf_hyper_sample.
#include "hmc.h"
#include "two_mode.h"
#include <cmath>

#define HMC_MAX_L (1 << 20)        // the adaptation ceil(1.6 L) is uncapped in the reference; past this the launches' partial
                                   // sums alone would take gigabytes

struct bdf_hmc {
    bdf_ctx *ctx = nullptr;                // borrowed
    int D = 0;
    int64_t N[2] = {}, nnz = 0, nb[2] = {};
    double mean_value = 0.0, alpha = 0.0;
    DevBuf<double> sample[2], mom[2], start[2], G[2], mu[2], Lambda[2], mu0[2], WI[2], sumU[2], UUt[2];
    TwoModeCsr csr[2];
    DevBuf<double> partial;                // room for the launches of an iteration with the largest L so far
    DevBuf<double> rec;                    // the iteration's record, and its copy in pinned host memory: both for the largest L so far
    DevBuf<double> rec_host = DevBuf<double>::pinned(kPinnedDefault);
    DevEvent decided; bool pending = false;   // the record of the last iteration is on its way to rec_host
    bdf_pairs *test = nullptr;             // borrowed (bdf_hmc_set_test)
    double clamp_lo = 1.0, clamp_hi = 0.0; DevBuf<double> avg, tpart; int64_t tnb = 0;
    int L = 10, L_inner = 1, prior_freq = 8, burnin = 100; double eps = 0.01;
    int64_t iters = 0;
    ~bdf_hmc() { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
};

namespace {

size_t partial_bytes(const bdf_hmc *h, int L) { return (size_t)((L + 1) * h->nb[0] + L * h->nb[1]) * HMC_PW * 8; }
size_t rec_bytes(int L) { return (size_t)(HMC_REC_LOG + 2 * L + 1) * 8; }

// room for an iteration with this L (the previous iteration's kernels are done: its decision has been read)
int hmc_reserve(bdf_hmc *h, int L)
{
    int rc;
    if ((rc = h->partial.grow(partial_bytes(h, L)))) return rc;
    if (rec_bytes(L) > h->rec.bytes()) {
        DevBuf<double> rec, host = DevBuf<double>::pinned(kPinnedDefault);
        if ((rc = rec.alloc_bytes(rec_bytes(L)))) return rc;
        BDF_HIP(hipMemset(rec, 0, rec_bytes(L)));
        if ((rc = host.alloc_bytes(rec_bytes(L)))) return rc;
        if (h->rec_host) memcpy(host, h->rec_host, h->rec_host.bytes());
        else memset(host, 0, rec_bytes(L));
        h->rec = std::move(rec); h->rec_host = std::move(host);
    }
    return BDF_OK;
}

// the decision of the last iteration: its eps and L become the next iteration's
int hmc_settle(bdf_hmc *h)
{
    if (!h->pending) return BDF_OK;
    BDF_HIP(hipEventSynchronize(h->decided));
    h->pending = false;
    h->eps = h->rec_host[HMC_REC_EPS_NEW];
    const double L = h->rec_host[HMC_REC_L_NEW];
    BDF_REQUIRE(L >= 1.0 && L <= (double)HMC_MAX_L, BDF_ERR_ARG,
                "bdf_hmc_iterate: the adapted number of leapfrog steps L = %.0f exceeds %d (eps = %.3e)", L, HMC_MAX_L, h->eps);
    h->L = (int)L;
    return BDF_OK;
}

}  // namespace

extern "C" int bdf_hmc_create(bdf_ctx *ctx, int D, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes,
                              const double *values, double alpha, bdf_hmc **out)
{
    BDF_REQUIRE(ctx && dims && out, BDF_ERR_ARG, "bdf_hmc_create: NULL argument");
    int rc = two_mode_check("bdf_hmc_create", D, dims, nnz, ids, id_bytes, values);
    if (rc) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    int64_t nb[2];
    for (int e = 0; e < 2; e++) nb[e] = hmc_row_blocks(D, dims[e]);

    // ---- device-memory budget, before anything is allocated (the partial sums for the default L = 10)
    size_t need = 0;
    for (int e = 0; e < 2; e++)
        need += (size_t)dims[e] * D * 3 * 8 + (size_t)(dims[e] + 1) * 8 + (size_t)dims[e] * 4 + (size_t)(4 * D * D + 5 * D) * 8 +
                (size_t)nb[e] * 11 * HMC_PW * 8;
    need += (size_t)nnz * 2 * (4 + 3 * 8);
    size_t mem_free = 0, mem_total = 0;
    BDF_HIP(hipMemGetInfo(&mem_free, &mem_total));
    BDF_REQUIRE(need <= mem_free, BDF_ERR_ARG, "bdf_hmc_create: the model needs %zu bytes of device memory, %zu are free", need,
                mem_free);

    std::unique_ptr<bdf_hmc> owner(new bdf_hmc());
    bdf_hmc *h = owner.get();
    h->ctx = ctx; h->D = D; h->nnz = nnz; h->alpha = alpha;
    if ((rc = h->decided.create(hipEventDisableTiming))) return rc;
    // the CSR with each entry's multiplicity and sum of squares: the energy's data term over duplicates
    if ((rc = two_mode_build("bdf_hmc_create", dims, nnz, ids, id_bytes, values, true, h->csr, &h->mean_value))) return rc;

    for (int e = 0; e < 2; e++) {
        const int64_t N = dims[e];
        h->N[e] = N; h->nb[e] = nb[e];
        // reset! (RelationData.jl:66-90): sample 0, mu 0, Lambda 5 I, mu0 0, WI I; HMCModel's G = repmat(diag(Lambda), 1, N)
        std::vector<double> zeros((size_t)N * D, 0.0), zd(D, 0.0), G(D, 5.0), Lam((size_t)D * D, 0.0), WI((size_t)D * D, 0.0);
        for (int i = 0; i < D; i++) { Lam[i * D + i] = 5.0; WI[i * D + i] = 1.0; }
        if ((rc = h->sample[e].upload(zeros)) || (rc = h->mom[e].upload(zeros)) || (rc = h->start[e].upload(zeros)) ||
            (rc = h->G[e].upload(G)) || (rc = h->mu[e].upload(zd)) || (rc = h->Lambda[e].upload(Lam)) ||
            (rc = h->mu0[e].upload(zd)) || (rc = h->WI[e].upload(WI)) || (rc = h->sumU[e].upload(zd)) ||
            (rc = h->UUt[e].upload(Lam)))
            return rc;
    }
    if ((rc = hmc_reserve(h, h->L))) return rc;
    BDF_HIP(hipDeviceSynchronize());
    *out = owner.release();
    return BDF_OK;
}

extern "C" int bdf_hmc_destroy(bdf_hmc *hmc)
{
    if (hmc) delete hmc;
    return BDF_OK;
}

extern "C" int bdf_hmc_set_test(bdf_hmc *hmc, bdf_pairs *test, double clamp_lo, double clamp_hi)
{
    BDF_REQUIRE(hmc, BDF_ERR_ARG, "bdf_hmc_set_test: hmc is NULL");
    BDF_REQUIRE(!test || test->n_modes == 2, BDF_ERR_ARG, "bdf_hmc_set_test: the test pairs must have two modes");
    BDF_REQUIRE(hmc->iters == 0, BDF_ERR_ARG, "bdf_hmc_set_test: call before the first iteration");
    BDF_HIP(hipSetDevice(hmc->ctx->device));
    hmc->avg.reset();
    hmc->tpart.reset();
    hmc->test = test && test->n > 0 ? test : nullptr;
    hmc->clamp_lo = clamp_lo; hmc->clamp_hi = clamp_hi;
    if (hmc->test) {
        hmc->tnb = hmc_predict_blocks(test->n);
        int rc;
        if ((rc = hmc->avg.alloc((size_t)test->n)) || (rc = hmc->tpart.alloc((size_t)hmc->tnb * 2))) return rc;
    }
    return BDF_OK;
}

extern "C" int bdf_hmc_set_params(bdf_hmc *hmc, int L, int L_inner, int prior_freq, double eps, int burnin)
{
    BDF_REQUIRE(hmc, BDF_ERR_ARG, "bdf_hmc_set_params: hmc is NULL");
    BDF_REQUIRE(L >= 1 && L <= HMC_MAX_L && L_inner >= 1 && prior_freq >= 1, BDF_ERR_ARG,
                "bdf_hmc_set_params: L=%d, L_inner=%d and prior_freq=%d must be at least 1", L, L_inner, prior_freq);
    BDF_REQUIRE(eps > 0.0 && std::isfinite(eps), BDF_ERR_ARG, "bdf_hmc_set_params: eps=%g must be positive and finite", eps);
    BDF_REQUIRE(burnin >= 0, BDF_ERR_ARG, "bdf_hmc_set_params: burnin=%d must not be negative", burnin);
    int rc = hmc_settle(hmc);
    if (rc) return rc;
    hmc->L = L; hmc->L_inner = L_inner; hmc->prior_freq = prior_freq; hmc->eps = eps; hmc->burnin = burnin;
    return BDF_OK;
}

extern "C" int bdf_hmc_iterate(bdf_hmc *hmc, int n)
{
    BDF_REQUIRE(hmc && n >= 0, BDF_ERR_ARG, "bdf_hmc_iterate: bad argument");
    bdf_ctx *ctx = hmc->ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    const int D = hmc->D;
    for (int it = 0; it < n; it++) {
        int rc;
        if ((rc = hmc_settle(hmc)) || (rc = hmc_reserve(hmc, hmc->L))) return rc;
        const int L = hmc->L;
        const int64_t i = hmc->iters + 1;
        const uint32_t sweep = (uint32_t)i;
        // the leapfrog (macau_hmc.jl:77-85): U(eps/2), then L times V(eps) and, but for the last, U(eps); U(eps/2).
        // Launch s (U for even s) writes its partial sums at slot s.
        int64_t off = 0;
        for (int s = 0; s <= 2 * L; s++) {
            const int e = s & 1;
            HMCLeapArgs a;
            a.D = D; a.L_inner = hmc->L_inner; a.tag = (uint32_t)e; a.N = hmc->N[e];
            a.flags = (e == 0 ? HMC_DATA : 0) | (s <= 1 ? HMC_DRAW : 0) | (s >= 2 * L - 1 ? HMC_FINAL : 0);
            a.order = hmc->csr[e].order; a.rowptr = hmc->csr[e].rowptr; a.colidx = hmc->csr[e].colidx; a.vals = hmc->csr[e].vals;
            a.cs = hmc->csr[e].cs;
            a.other = hmc->sample[1 - e]; a.sample = hmc->sample[e]; a.mom = hmc->mom[e]; a.start = hmc->start[e];
            a.G = hmc->G[e]; a.mu = hmc->mu[e]; a.Lambda = hmc->Lambda[e];
            a.alpha = hmc->alpha; a.eps = (s == 0 || s == 2 * L) ? hmc->eps / 2 : hmc->eps;
            a.seed = ctx->seed; a.sweep = sweep; a.partial = hmc->partial + off;
            if ((rc = hmc_launch_leap(ctx->stream, a))) return rc;
            off += hmc->nb[e] * HMC_PW;
        }
        // dH, the Metropolis step and the adaptation (:88-105); the decision goes to the host for the next L
        HMCAcceptArgs acc;
        acc.partial = hmc->partial; acc.nb[0] = hmc->nb[0]; acc.nb[1] = hmc->nb[1]; acc.L = L; acc.eps = hmc->eps;
        acc.alpha = hmc->alpha; acc.seed = ctx->seed; acc.sweep = sweep; acc.rec = hmc->rec; acc.flag = ctx->flag_dev;
        if ((rc = hmc_launch_accept(ctx->stream, acc))) return rc;
        BDF_HIP(hipMemcpyAsync(hmc->rec_host, hmc->rec, rec_bytes(L), hipMemcpyDeviceToHost, ctx->stream));
        BDF_HIP(hipEventRecord(hmc->decided, ctx->stream));
        hmc->pending = true;
        HMCRestoreArgs rs;
        for (int e = 0; e < 2; e++) { rs.n[e] = hmc->N[e] * D; rs.sample[e] = hmc->sample[e]; rs.start[e] = hmc->start[e]; }
        rs.rec = hmc->rec;
        if ((rc = hmc_launch_restore(ctx->stream, rs))) return rc;
        // update_latent_prior!(en, true) for both entities every prior_freq-th iteration (:108-113)
        if (i % hmc->prior_freq == 0) {
            if ((rc = bdf_ctx_set_sweep(ctx, sweep))) return rc;
            for (int e = 0; e < 2; e++)
                if ((rc = bdf_hyper_sums(ctx, D, hmc->N[e], hmc->sample[e], nullptr, hmc->sumU[e], hmc->UUt[e])) ||
                    (rc = bdf_hyper_sample(ctx, D, hmc->N[e], hmc->sumU[e], hmc->UUt[e], hmc->mu0[e], 2.0, hmc->WI[e], (double)D,
                                           (uint32_t)e, hmc->mu[e], hmc->Lambda[e], nullptr, nullptr, nullptr)))
                    return rc;
        }
        // yhat = clamp!(pred(test)), update_yhat_post! (:115-121)
        if (hmc->test) {
            HMCPredictArgs p;
            p.D = D; p.n = hmc->test->n; p.ids = hmc->test->ids_dev; p.values = hmc->test->values_dev;
            p.U = hmc->sample[0]; p.V = hmc->sample[1]; p.mean = hmc->mean_value; p.lo = hmc->clamp_lo; p.hi = hmc->clamp_hi;
            p.copy = i <= hmc->burnin + 1; p.count = (double)(i - hmc->burnin - 1); p.avg = hmc->avg; p.partial = hmc->tpart;
            if ((rc = hmc_launch_predict(ctx->stream, p))) return rc;
        }
        hmc->iters++;
    }
    return BDF_OK;
}

extern "C" int bdf_hmc_stats(bdf_hmc *hmc, double *out, double *log, int log_cap)
{
    BDF_REQUIRE(hmc && out, BDF_ERR_ARG, "bdf_hmc_stats: NULL argument");
    BDF_HIP(hipSetDevice(hmc->ctx->device));
    int rc = bdf_ctx_sync(hmc->ctx);
    if (rc) return rc;
    const double *r = hmc->rec_host;
    for (int k = 0; k < 14; k++) out[k] = hmc->iters > 0 ? r[k] : (k <= HMC_REC_L ? 0.0 : NAN);
    out[14] = out[15] = NAN;
    if (hmc->iters > 0 && hmc->test) {
        std::vector<double> part((size_t)hmc->tnb * 2);
        BDF_HIP(hipMemcpy(part.data(), hmc->tpart, part.size() * 8, hipMemcpyDeviceToHost));
        double s1 = 0.0, s2 = 0.0;
        for (int64_t b = 0; b < hmc->tnb; b++) { s1 += part[2 * b]; s2 += part[2 * b + 1]; }
        out[14] = std::sqrt(s1 / (double)hmc->test->n);
        out[15] = std::sqrt(s2 / (double)hmc->test->n);
    }
    if (log) {
        const int nlog = hmc->iters > 0 ? 2 * (int)r[HMC_REC_L] + 1 : 0;
        for (int k = 0; k < log_cap; k++) log[k] = k < nlog ? r[HMC_REC_LOG + k] : NAN;
    }
    return BDF_OK;
}

extern "C" int bdf_hmc_model(bdf_hmc *hmc, int entity, double *sample, double *momentum, double *mu, double *Lambda)
{
    BDF_REQUIRE(hmc, BDF_ERR_ARG, "bdf_hmc_model: hmc is NULL");
    BDF_REQUIRE(entity == 0 || entity == 1, BDF_ERR_ARG, "bdf_hmc_model: entity %d must be 0 (U) or 1 (V)", entity);
    BDF_HIP(hipSetDevice(hmc->ctx->device));
    int rc = bdf_ctx_sync(hmc->ctx);
    if (rc) return rc;
    const int D = hmc->D;
    const size_t nd = (size_t)hmc->N[entity] * D * 8;
    if (sample) BDF_HIP(hipMemcpy(sample, hmc->sample[entity], nd, hipMemcpyDeviceToHost));
    if (momentum) BDF_HIP(hipMemcpy(momentum, hmc->mom[entity], nd, hipMemcpyDeviceToHost));
    if (mu) BDF_HIP(hipMemcpy(mu, hmc->mu[entity], (size_t)D * 8, hipMemcpyDeviceToHost));
    if (Lambda) BDF_HIP(hipMemcpy(Lambda, hmc->Lambda[entity], (size_t)D * D * 8, hipMemcpyDeviceToHost));
    return BDF_OK;
}
