// bdf_vb.hip -- C ABI of variational BPMF (src/macau_vb.jl): the host-side set-up that bpmf_vb does in Julia (the CSR of both
// modes through two_mode.hip, VBModel's initial state) and the iteration loop, enqueued on the context's stream.  The kernels
// are in k_vb.hip.
#include "vb.h"
#include "two_mode.h"
#include <cmath>

struct bdf_vb {
    bdf_ctx *ctx = nullptr;        // borrowed
    int D = 0, T = 0, RS = 0, PW = 0;
    int64_t N[2] = {}, nnz = 0;
    double mean_value = 0.0, alpha = 0.0;
    double nu_N[2] = {}, b_N[2] = {}, b_0[2] = {};
    DevBuf<double> rec[2], mu[2], pack[2], W_N[2], mu_N[2], mu0[2], Winv0[2];
    TwoModeCsr csr[2];
    DevBuf<double> partial[2]; int64_t nblocks[2] = {};
    DevBuf<double> slices;
    DevBuf<double> stats;          // dev: [0..4) test statistics, [4..8) train statistics, [8] |U|^2, [9] |V|^2
    std::unique_ptr<bdf_pairs> train;
    bdf_pairs *test = nullptr;     // borrowed (bdf_vb_set_test)
    double clamp_lo = 1.0, clamp_hi = 0.0;
    int64_t iters = 0;
    ~bdf_vb() { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
};

extern "C" int bdf_vb_create(bdf_ctx *ctx, int D, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes,
                             const double *values, double alpha, const double *mu_init_u, const double *mu_init_v, bdf_vb **out)
{
    BDF_REQUIRE(ctx && dims && out && mu_init_u && mu_init_v, BDF_ERR_ARG, "bdf_vb_create: NULL argument");
    int rc = two_mode_check("bdf_vb_create", D, dims, nnz, ids, id_bytes, values);
    if (rc) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    const int T = vb_tri(D), RS = vb_record(D), PW = T + D + 1;
    int64_t nb[2];
    for (int e = 0; e < 2; e++) nb[e] = vb_row_blocks(D, dims[e]);

    // ---- device-memory budget, before anything is allocated
    size_t need = 0;
    for (int e = 0; e < 2; e++)
        need += (size_t)dims[e] * (RS + D) * 8 + (size_t)nb[e] * PW * 8 + (size_t)(dims[e] + 1) * 8 + (size_t)dims[e] * 4 +
                (size_t)(3 * D * D + 3 * D) * 8;
    need += (size_t)nnz * 2 * (4 + 8) + (size_t)nnz * (2 * 4 + 3 * 8) + (size_t)VB_SLICES * PW * 8;
    size_t mem_free = 0, mem_total = 0;
    BDF_HIP(hipMemGetInfo(&mem_free, &mem_total));
    BDF_REQUIRE(need <= mem_free, BDF_ERR_ARG,
                "bdf_vb_create: the model needs %zu bytes of device memory (the packed second moments alone "
                "2 x N x D(D+1)/2 x 8 = %zu), %zu are free", need, (size_t)(dims[0] + dims[1]) * T * 8, mem_free);

    std::unique_ptr<bdf_vb> v(new bdf_vb());
    v->ctx = ctx; v->D = D; v->T = T; v->RS = RS; v->PW = PW; v->nnz = nnz; v->alpha = alpha;
    if ((rc = two_mode_build("bdf_vb_create", dims, nnz, ids, id_bytes, values, false, v->csr, &v->mean_value))) return rc;

    if ((rc = v->stats.alloc(16))) return rc;
    BDF_HIP(hipMemset(v->stats, 0, 16 * sizeof(double)));
    for (int e = 0; e < 2; e++) {
        // ---- VBModel(D, N) (macau_vb.jl:20-37): W_N = I / N, nu_N = D + N, mu_N = 0, b_N = 2 + N, Winv_0 = I, mu_0 = 0, b_0 = 2,
        // Euu[:,:,n] = inv(W_N) + mu_n mu_n'
        const int64_t N = dims[e];
        const double *mi = e == 0 ? mu_init_u : mu_init_v;
        v->N[e] = N;
        v->nu_N[e] = (double)D + (double)N; v->b_N[e] = 2.0 + (double)N; v->b_0[e] = 2.0;
        const double wn = 1.0 / (double)N, winv = 1.0 / wn;
        std::vector<double> rec((size_t)N * RS, 0.0), mu(mi, mi + (size_t)N * D);
        double nsq = 0.0;
        for (int64_t n = 0; n < N; n++) {
            const double *m = mi + n * D;
            double *r = rec.data() + n * RS;
            for (int j = 0; j < D; j++)
                for (int i = 0; i <= j; i++) r[j * (j + 1) / 2 + i] = (i == j ? winv : 0.0) + m[i] * m[j];
            for (int i = 0; i < D; i++) { r[T + i] = m[i]; nsq += m[i] * m[i]; }
        }
        std::vector<double> eye((size_t)D * D, 0.0), W((size_t)D * D, 0.0), A((size_t)D * D + D, 0.0), zero(D, 0.0);
        for (int i = 0; i < D; i++) { eye[i * D + i] = 1.0; W[i * D + i] = wn; A[i * D + i] = wn * v->nu_N[e]; }
        if ((rc = v->rec[e].upload(rec)) || (rc = v->mu[e].upload(mu)) || (rc = v->pack[e].upload(A)) ||
            (rc = v->W_N[e].upload(W)) || (rc = v->mu_N[e].upload(zero)) || (rc = v->mu0[e].upload(zero)) ||
            (rc = v->Winv0[e].upload(eye)) || (rc = v->partial[e].alloc_bytes(std::max<size_t>((size_t)nb[e] * PW * 8, 16))))
            return rc;
        v->nblocks[e] = nb[e];
        BDF_HIP(hipMemcpy(v->stats + 8 + e, &nsq, sizeof(double), hipMemcpyHostToDevice));      // vecnorm(mu_u)^2 before any iteration
    }
    if ((rc = v->slices.alloc((size_t)VB_SLICES * PW))) return rc;

    // ---- the raw training rows (uid, vid, value) for the train RMSE (:75-76)
    bdf_pairs *train;
    if ((rc = bdf_pairs_create(ctx, 2, nnz, ids, id_bytes, values, &train))) return rc;
    v->train.reset(train);
    BDF_HIP(hipDeviceSynchronize());
    *out = v.release();
    return BDF_OK;
}

extern "C" int bdf_vb_destroy(bdf_vb *vb)
{
    if (vb) delete vb;
    return BDF_OK;
}

extern "C" int bdf_vb_set_test(bdf_vb *vb, bdf_pairs *test, double clamp_lo, double clamp_hi)
{
    BDF_REQUIRE(vb, BDF_ERR_ARG, "bdf_vb_set_test: vb is NULL");
    BDF_REQUIRE(!test || test->n_modes == 2, BDF_ERR_ARG, "bdf_vb_set_test: the test pairs must have two modes");
    vb->test = test;
    vb->clamp_lo = clamp_lo; vb->clamp_hi = clamp_hi;
    return BDF_OK;
}

extern "C" int bdf_vb_iterate(bdf_vb *vb, int n)
{
    BDF_REQUIRE(vb && n >= 0, BDF_ERR_ARG, "bdf_vb_iterate: bad argument");
    bdf_ctx *ctx = vb->ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    for (int it = 0; it < n; it++) {
        int rc;
        // update_u!(U, V), then update_u!(V, U) with the new U (macau_vb.jl:62-63)
        for (int e = 0; e < 2; e++) {
            VBRowArgs a;
            a.D = vb->D; a.T = vb->T; a.RS = vb->RS; a.PW = vb->PW; a.N = vb->N[e];
            a.order = vb->csr[e].order; a.rowptr = vb->csr[e].rowptr; a.colidx = vb->csr[e].colidx; a.vals = vb->csr[e].vals;
            a.rec_other = vb->rec[1 - e]; a.rec_out = vb->rec[e]; a.mu_out = vb->mu[e]; a.pack = vb->pack[e];
            a.alpha = vb->alpha; a.partial = vb->partial[e]; a.flag = ctx->flag_dev;
            if ((rc = vb_launch_rows(ctx->stream, a))) return rc;
        }
        // update_prior!(U), update_prior!(V) (:65-66)
        for (int e = 0; e < 2; e++) {
            VBPriorArgs p;
            p.D = vb->D; p.T = vb->T; p.PW = vb->PW; p.nblocks = vb->nblocks[e]; p.partial = vb->partial[e]; p.slices = vb->slices;
            p.nu_N = vb->nu_N[e]; p.b_N = vb->b_N[e]; p.b_0 = vb->b_0[e]; p.mu0 = vb->mu0[e]; p.Winv0 = vb->Winv0[e];
            p.W_N = vb->W_N[e]; p.mu_N = vb->mu_N[e]; p.pack = vb->pack[e]; p.normsq = vb->stats + 8 + e; p.flag = ctx->flag_dev;
            if ((rc = vb_launch_prior(ctx->stream, p))) return rc;
        }
        // test and train squared errors of clamp!(mean_value + <mu_u, mu_v>) (:73-76)
        const double *fac[2] = {vb->mu[0], vb->mu[1]};
        if (vb->test && vb->test->n > 0 &&
            (rc = bdf_predict_update(ctx, vb->test, vb->D, fac, vb->mean_value, 0, vb->clamp_lo, vb->clamp_hi, 0.0, vb->stats)))
            return rc;
        if ((rc = bdf_predict_update(ctx, vb->train.get(), vb->D, fac, vb->mean_value, 0, vb->clamp_lo, vb->clamp_hi, 0.0, vb->stats + 4)))
            return rc;
        vb->iters++;
    }
    return BDF_OK;
}

extern "C" int bdf_vb_stats(bdf_vb *vb, double *out)
{
    BDF_REQUIRE(vb && out, BDF_ERR_ARG, "bdf_vb_stats: NULL argument");
    int rc = bdf_ctx_sync(vb->ctx);
    if (rc) return rc;
    double st[10];
    BDF_HIP(hipMemcpy(st, vb->stats, sizeof(st), hipMemcpyDeviceToHost));
    const bool have = vb->iters > 0;
    const int64_t ntest = vb->test ? vb->test->n : 0;
    out[0] = have && ntest > 0 ? std::sqrt(st[1] / (double)ntest) : NAN;
    out[1] = have ? std::sqrt(st[5] / (double)vb->nnz) : NAN;
    out[2] = std::sqrt(st[8]);
    out[3] = std::sqrt(st[9]);
    return BDF_OK;
}

extern "C" int bdf_vb_model(bdf_vb *vb, int entity, double *mu_host, double *Euu_host, double *prior_host)
{
    BDF_REQUIRE(vb, BDF_ERR_ARG, "bdf_vb_model: vb is NULL");
    BDF_REQUIRE(entity == 0 || entity == 1, BDF_ERR_ARG, "bdf_vb_model: entity %d must be 0 (U) or 1 (V)", entity);
    int rc = bdf_ctx_sync(vb->ctx);
    if (rc) return rc;
    const int D = vb->D, RS = vb->RS;
    const int64_t N = vb->N[entity];
    if (mu_host) BDF_HIP(hipMemcpy(mu_host, vb->mu[entity], (size_t)N * D * 8, hipMemcpyDeviceToHost));
    if (Euu_host) {
        std::vector<double> rec((size_t)N * RS);
        BDF_HIP(hipMemcpy(rec.data(), vb->rec[entity], rec.size() * 8, hipMemcpyDeviceToHost));
        for (int64_t n = 0; n < N; n++) {
            const double *r = rec.data() + n * RS;
            double *E = Euu_host + (size_t)n * D * D;
            for (int j = 0; j < D; j++)
                for (int i = 0; i < D; i++) E[j * D + i] = i <= j ? r[j * (j + 1) / 2 + i] : r[i * (i + 1) / 2 + j];
        }
    }
    if (prior_host) {
        BDF_HIP(hipMemcpy(prior_host, vb->mu_N[entity], (size_t)D * 8, hipMemcpyDeviceToHost));
        BDF_HIP(hipMemcpy(prior_host + D, vb->W_N[entity], (size_t)D * D * 8, hipMemcpyDeviceToHost));
        prior_host[D + D * D] = vb->nu_N[entity];
        prior_host[D + D * D + 1] = vb->b_N[entity];
    }
    return BDF_OK;
}
