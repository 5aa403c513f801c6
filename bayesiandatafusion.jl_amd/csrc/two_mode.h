// two_mode.h -- the training data of one two-mode relation as the trainers on one matrix (bdf_vb.hip, bdf_hmc.hip) keep it
// on the device: the reference's Udata = sparse(vid, uid, val) and Vdata = Udata', with the values centred.
#pragma once
#include "bdf_common.h"

// One mode's rows are that entity's rows.  Row i lists its distinct neighbours (0-based ids in the other mode) in ascending
// order, each with the sum of its centred values val - mean, added in input order.  With counts, cs holds beside every entry
// its multiplicity and the sum of the squares of those centred values.  order: the rows by falling degree (rows_by_degree),
// so that the longest rows start first and rows of similar length share a workgroup.
struct TwoModeCsr {
    DevBuf<int64_t> rowptr;     // N + 1
    DevBuf<int32_t> colidx;     // one per entry
    DevBuf<double> vals, cs;    // one per entry; two per entry (empty without counts)
    DevBuf<int32_t> order;      // N
};

// the argument checks of a trainer's create; who names it in the error messages
int two_mode_check(const char *who, int D, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes,
                   const double *values);

// after two_mode_check: parses and bounds-checks the 1-based ids (mode m's at ids[m * nnz + k], id_bytes 4 or 8), computes the
// mean and uploads both modes' CSR, one mode at a time.
int two_mode_build(const char *who, const int64_t *dims, int64_t nnz, const void *ids, int id_bytes, const double *values,
                   bool with_counts, TwoModeCsr out[2], double *mean);
