// k_feat_eig.hip -- K4: the direct solve of the beta update through the eigendecomposition of F'F.
#include "feat.h"
#include <algorithm>
#include <cmath>

// ---- direct solve through the eigendecomposition of F'F (solve_full, src/sampling.jl:314-320, for 64 < numF <= BDF_EIG_MAX) ----
// The reference factors FF + lambda I anew in every iteration because lambda_beta is resampled.  F'F itself never changes:
// F'F = Q diag(s) Q' (symmetric, s >= 0) is computed ONCE -- on the host, at first use: Householder tridiagonalisation and
// the implicit QL iteration (the EISPACK tred2 / tql2 procedures) -- and every iteration's solve is two small dense products
// on the matrix cores with a scaling between them: beta = Q ((Q' rhs) ./ (s + lambda)).  Same solution as the factorisation
// to rounding (residual ~1e-13 ||rhs|| on C3's matrices); 0.02 ms instead of 0.34 ms per iteration at numF = 500.
namespace {

// symmetric A (n x n, column-major, both triangles) -> eigenvalues d (ascending), eigenvectors in the columns of V
// returns false if the QL iteration did not converge for some eigenvalue within 200 sweeps (the caller then takes the factorisation)
bool eig_sym_host(int n, const double *A, std::vector<double> &d, std::vector<double> &V)
{
    bool converged = true;
    V.assign(A, A + (size_t)n * n);
    d.assign((size_t)n, 0.0);
    std::vector<double> e((size_t)n, 0.0);
    auto v = [&](int i, int j) -> double & { return V[(size_t)i + (size_t)j * n]; };
    // -- Householder reduction to tridiagonal form (tred2)
    for (int j = 0; j < n; j++) d[j] = v(n - 1, j);
    for (int i = n - 1; i > 0; i--) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; k++) scale += fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; j++) { d[j] = v(i - 1, j); v(i, j) = 0.0; v(j, i) = 0.0; }
        } else {
            for (int k = 0; k < i; k++) { d[k] /= scale; h += d[k] * d[k]; }
            double f = d[i - 1], g = sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h -= f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; j++) e[j] = 0.0;
            for (int j = 0; j < i; j++) {
                f = d[j];
                v(j, i) = f;
                g = e[j] + v(j, j) * f;
                for (int k = j + 1; k <= i - 1; k++) { g += v(k, j) * d[k]; e[k] += v(k, j) * f; }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; j++) { e[j] /= h; f += e[j] * d[j]; }
            const double hh = f / (h + h);
            for (int j = 0; j < i; j++) e[j] -= hh * d[j];
            for (int j = 0; j < i; j++) {
                f = d[j]; g = e[j];
                for (int k = j; k <= i - 1; k++) v(k, j) -= (f * e[k] + g * d[k]);
                d[j] = v(i - 1, j);
                v(i, j) = 0.0;
            }
        }
        d[i] = h;
    }
    for (int i = 0; i < n - 1; i++) {
        v(n - 1, i) = v(i, i);
        v(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; k++) d[k] = v(k, i + 1) / h;
            for (int j = 0; j <= i; j++) {
                double g = 0.0;
                for (int k = 0; k <= i; k++) g += v(k, i + 1) * v(k, j);
                for (int k = 0; k <= i; k++) v(k, j) -= g * d[k];
            }
        }
        for (int k = 0; k <= i; k++) v(k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; j++) { d[j] = v(n - 1, j); v(n - 1, j) = 0.0; }
    v(n - 1, n - 1) = 1.0;
    e[0] = 0.0;
    // -- implicit QL iteration on the tridiagonal matrix, accumulating the rotations (tql2)
    for (int i = 1; i < n; i++) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = 2.220446049250313e-16;
    for (int l = 0; l < n; l++) {
        tst1 = std::max(tst1, fabs(d[l]) + fabs(e[l]));
        int m = l;
        while (m < n) { if (fabs(e[m]) <= eps * tst1) break; m++; }
        if (m > l) {
            int iter = 0;
            do {
                iter++;
                double g = d[l], p = (d[l + 1] - g) / (2.0 * e[l]), r = hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; i++) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c, el1 = e[l + 1], s = 0.0, s2 = 0.0;
                for (int i = m - 1; i >= l; i--) {
                    c3 = c2; c2 = c; s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    for (int k = 0; k < n; k++) {
                        h = v(k, i + 1);
                        v(k, i + 1) = s * v(k, i) + c * h;
                        v(k, i) = c * v(k, i) - s * h;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (fabs(e[l]) > eps * tst1 && iter < 200);
            if (fabs(e[l]) > eps * tst1) converged = false;
        }
        d[l] += f;
        e[l] = 0.0;
    }
    return converged;
}

__global__ void k_eig_scale(int64_t n, int D, const double *s, const double *lambda_p, double *Y, int *flag)      // Y(i, c) /= s_i + lambda
{
    const double lambda = *lambda_p;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n * D) {
        const double den = s[t % n] + lambda;          // (s >= 0: clamped when the decomposition was made)
        if (!(den > 0.0) && t < n) atomicOr_system(flag, 8);      // F'F + lambda I not positive definite (what the Cholesky path reports); the flag is host memory
        Y[t] = Y[t] / den;
    }
}

int ensure_eig(bdf_feat *f, int D)
{
    bdf_ctx *ctx = f->ctx;
    const int64_t n = f->n;
    int rc;
    if (!f->eig_Q) {
        if ((rc = feat_ensure_FF(f))) return rc;
        BDF_HIP(hipStreamSynchronize(ctx->stream));
        std::vector<double> A((size_t)n * n), s, Q;
        BDF_HIP(hipMemcpy(A.data(), f->FF_dev, A.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < n; j++)          // exactly symmetric input (the product's two triangles agree to rounding only)
            for (int64_t i = j + 1; i < n; i++) A[(size_t)i + (size_t)j * n] = A[(size_t)j + (size_t)i * n];
        if (!eig_sym_host((int)n, A.data(), s, Q)) { f->eig_failed = true; return BDF_OK; }      // (the caller falls back to bdf_chol_solve)
        for (double &x : s) x = std::max(x, 0.0);       // F'F is positive semi-definite: an eigenvalue below zero is rounding
        std::unique_ptr<bdf_feat> q(new bdf_feat());
        q->ctx = ctx; q->kind = 0; q->m = n; q->n = n; q->nnz = n * n;
        if (q->dense_dev.alloc(Q.size()) || f->eig_s.alloc((size_t)n)) {
            f->eig_s.reset();
            bdf_set_error("ensure_eig: out of device memory");
            return BDF_ERR_HIP;
        }
        BDF_HIP(hipMemcpy(q->dense_dev, Q.data(), Q.size() * sizeof(double), hipMemcpyHostToDevice));
        BDF_HIP(hipMemcpy(f->eig_s, s.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        f->eig_Q = std::move(q);
    }
    return f->eig_y.grow((size_t)n * D * sizeof(double), ctx->stream);
}

}  // namespace

// beta (n x D column-major) = (F'F + lambda I) \ rhs
int feat_eig_solve(bdf_ctx *ctx, bdf_feat *f, int D, const double *lambda_dev, const double *rhs, double *beta_out)
{
    const int64_t n = f->n;
    int rc;
    if (f->eig_failed) return bdf_chol_solve(ctx, f, D, lambda_dev, rhs, beta_out);
    if ((rc = ensure_eig(f, D))) return rc;
    if (f->eig_failed) return bdf_chol_solve(ctx, f, D, lambda_dev, rhs, beta_out);        // the QL iteration did not converge: factor instead
    if ((rc = feat_apply(ctx, f->eig_Q.get(), true, rhs, 1, n, D, f->eig_y, 1, n))) return rc;              // Y = Q' rhs
    hipLaunchKernelGGL(k_eig_scale, dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, ctx->stream, n, D, (const double *)f->eig_s, lambda_dev, f->eig_y,
                       ctx->flag_dev);
    BDF_HIP(hipGetLastError());
    return feat_apply(ctx, f->eig_Q.get(), false, f->eig_y, 1, n, D, beta_out, 1, n);                       // beta = Q Y
}
