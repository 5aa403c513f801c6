// two_mode.hip -- the host set-up that bpmf_vb and macau_hmc share (src/macau_vb.jl:51-55, src/macau_hmc.jl:41-46): the ids, the
// mean, the centring and sparse() with its summed duplicates for both modes.  Host code only.
#include "two_mode.h"

int two_mode_check(const char *who, int D, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes, const double *values)
{
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "%s: num_latent=%d must be in 1..%d", who, D, BDF_MAX_D);
    BDF_REQUIRE(id_bytes == 4 || id_bytes == 8, BDF_ERR_ARG, "%s: id_bytes must be 4 or 8", who);
    BDF_REQUIRE(nnz >= 1 && ids && values, BDF_ERR_ARG, "%s: the relation has no observations", who);
    BDF_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[0] < 0x7fffffff && dims[1] < 0x7fffffff, BDF_ERR_ARG,
                "%s: entity sizes %lld, %lld", who, (long long)dims[0], (long long)dims[1]);
    return BDF_OK;
}

int two_mode_build(const char *who, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes, const double *values,
                   bool with_counts, TwoModeCsr out[2], double *mean_out)
{
    // ---- ids, mean, centred values
    std::vector<int32_t> id[2];
    for (int m = 0; m < 2; m++) {
        id[m].resize(nnz);
        for (int64_t k = 0; k < nnz; k++) {
            const int64_t v = id_bytes == 8 ? ((const int64_t *)ids)[m * nnz + k] : (int64_t)((const int32_t *)ids)[m * nnz + k];
            BDF_REQUIRE(v >= 1 && v <= dims[m], BDF_ERR_BOUNDS, "%s: id %lld of mode %d outside 1..%lld", who, (long long)v, m + 1,
                        (long long)dims[m]);
            id[m][k] = (int32_t)(v - 1);
        }
    }
    double sum = 0.0;
    for (int64_t k = 0; k < nnz; k++) sum += values[k];
    const double mean = sum / (double)nnz;
    *mean_out = mean;

    // ---- Udata = sparse(vid, uid, val): column u holds the v's in ascending order, duplicates summed in input order; Vdata = Udata'.
    // With counts, beside every entry: its multiplicity c and sum(val^2), so that c d^2 - 2 d sum(val) + sum(val^2) is HMC's
    // energy summed over the duplicates (d - val)^2 (computePotential does not sum them, macau_hmc.jl:224-227)
    for (int e = 0; e < 2; e++) {
        const std::vector<int32_t> &own = id[e], &oth = id[1 - e];
        const int64_t N = dims[e];
        std::vector<int64_t> perm(nnz);
        std::iota(perm.begin(), perm.end(), 0);
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
            return own[a] != own[b] ? own[a] < own[b] : oth[a] < oth[b];
        });
        std::vector<int64_t> rowptr(N + 1, 0);
        std::vector<int32_t> col;
        std::vector<double> val, cs;
        col.reserve(nnz); val.reserve(nnz);
        if (with_counts) cs.reserve(2 * nnz);
        for (int64_t q = 0; q < nnz; q++) {
            const int64_t k = perm[q];
            const double x = values[k] - mean;
            if (q > 0 && own[perm[q - 1]] == own[k] && oth[perm[q - 1]] == oth[k]) {
                val.back() += x;
                if (with_counts) { cs[cs.size() - 2] += 1.0; cs.back() += x * x; }
                continue;
            }
            col.push_back(oth[k]); val.push_back(x);
            if (with_counts) { cs.push_back(1.0); cs.push_back(x * x); }
            rowptr[own[k] + 1]++;
        }
        for (int64_t i = 0; i < N; i++) rowptr[i + 1] += rowptr[i];
        const std::vector<int32_t> order = rows_by_degree(N, [&](int32_t i) { return rowptr[i + 1] - rowptr[i]; });
        TwoModeCsr &c = out[e];
        int rc;
        if ((rc = c.rowptr.upload(rowptr)) || (rc = c.colidx.upload(col)) || (rc = c.vals.upload(val)) ||
            (with_counts && (rc = c.cs.upload(cs))) || (rc = c.order.upload(order)))
            return rc;
    }
    return BDF_OK;
}
