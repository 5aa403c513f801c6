// k1_accumulate.h -- the device code K1 (k_sample_rows.hip) shares with the row kernel of the spike-and-slab prior
// (k_rows_ss.hip): the gathers and the f64-MFMA accumulation of one item, the sum of a split row's partials, and the work
// item itself (process_item: accumulate, publish or finish).  The scheme is described at the head of k_sample_rows.hip.
#pragma once
#include "rows.h"
#include "wave_linalg.h"
#include "c_layout_chol.h"
#include "spike.h"
#include <cstdlib>

#ifndef BDF_K1_KS
#define BDF_K1_KS 2               // k-steps (4 observations each) per pipelined trip, matrix relations
#endif
#ifndef BDF_K1_KS64
#define BDF_K1_KS64 2             // ... at D > 32
#endif

#ifdef BDF_K1_SPANS      // diagnostic build: per wave of every launch {start, end, wait for the prior} (s_memrealtime: the 100 MHz clock all XCDs share -- s_memtime is per XCD; plain stores)
#define SPAN_BEGIN() do { if (lane == 0 && a.b_dump && wid < 8192) ((unsigned long long *)a.b_dump)[wid * 3] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define SPAN_END() do { if (lane == 0 && a.b_dump && wid < 8192) ((unsigned long long *)a.b_dump)[wid * 3 + 1] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define SPAN_WAIT(t0) do { if (lane == 0 && a.b_dump && wid < 8192) ((unsigned long long *)a.b_dump)[wid * 3 + 2] = (unsigned long long)__builtin_amdgcn_s_memrealtime() - (t0); } while (0)
#else
#define SPAN_BEGIN() do { } while (0)
#define SPAN_END() do { } while (0)
#define SPAN_WAIT(t0) do { } while (0)
#endif
#ifdef BDF_K1_STAMPS
#define STAMP(slot) do { if (lane == 0 && a.b_dump && wid < 65536) ((unsigned long long *)a.b_dump)[wid * 16 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define STAMP(slot) do { } while (0)
#endif

namespace {

template <int DP>
struct K1Local { static constexpr bool value = DP == 64; };      // D > 32: 8.6 KB of LDS per wave instead of 17.9 (c_layout_chol.h: GeoL)

// ---- accumulate one item, register path (any D, per-observation baselines): acc (MFMA C layout, lower block-triangle)
// and bred (the item's part of b) ------------------------------------------------------------------------------------
// Software pipeline over "trips" of 4*KS observations: the other-mode ids and values of trip t+2 and the gathered
// factor rows of trip t+1 are in flight while the MFMAs of trip t issue.  Lane (j = l & 15, h = l >> 4) handles
// observations h, h+4, h+8, ... of the item and elements 16 I + j of their factor rows (index-reversed).
// WEIGHTED (k_rows_w): observation k carries a precision weight omega_k = T.weight[T.perm[q]] (the caller's order, as `linear`); its
// Hadamard product and its residual are each multiplied by s = sqrt(omega_k) once, so that the same MFMAs accumulate
// sum omega w w' and the same fma sum omega (y - base) w.  A term without weights has s = 1: every product is then exact and
// the sums are those of the unweighted path, bit for bit.
template <int DP, int NO, bool WEIGHTED = false>
__device__ __forceinline__ void accumulate_reg(const SampleArgs &a, const Item &it, int lane, d4 (&acc)[Geo<DP>::NB],
                                  double (&bred)[Geo<DP>::DB])
{
    constexpr int DB = Geo<DP>::DB, NB = Geo<DP>::NB;
    constexpr int KS = (NO == 1) ? BDF_K1_KS : (NO == 2 ? 2 : 1);   // k-steps (of 4 observations) per trip
    const TermDev &T = a.t[it.term];
    const int D = a.D;
    const int j = lane & 15, h = lane >> 4;
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
    double bpart[DB];
    int ec[DB];                               // natural element index of reversed element 16*I + j (negative: padding)
#pragma unroll
    for (int I = 0; I < DB; I++) { bpart[I] = 0.0; ec[I] = D - 1 - (16 * I + j); }
    const int n = it.count;
    const int ntrips = (n + 4 * KS - 1) / (4 * KS);
    const int64_t qb = it.q_begin;

    int32_t ix_n[KS][NO], ix_nn[KS][NO];
    double rr_n[KS], rr_nn[KS];
    double s_n[WEIGHTED ? KS : 1], s_nn[WEIGHTED ? KS : 1];      // sqrt(omega) beside the residual (0 in an invalid lane)
    double w_n[KS][NO][DB];

#define LOAD_IDX(t, IX, RR, SS)                                                                  \
    _Pragma("unroll") for (int k = 0; k < KS; k++) {                                            \
        const int o = (t) * 4 * KS + 4 * k + h;                                                 \
        const bool valid = o < n;                                                               \
        const int64_t q = qb + (valid ? o : 0);                                                 \
        _Pragma("unroll") for (int m = 0; m < NO; m++) IX[k][m] = T.colidx[(int64_t)m * T.nnz + q]; \
        const double base = T.linear ? T.linear[T.perm[q]] : T.mean;                            \
        RR[k] = valid ? T.vals[q] - base : 0.0;                                                 \
        if constexpr (WEIGHTED) SS[k] = valid ? (T.weight ? sqrt(T.weight[T.perm[q]]) : 1.0) : 0.0; \
    }
#define LOAD_DATA(t, IX)                                                                        \
    _Pragma("unroll") for (int k = 0; k < KS; k++) {                                            \
        const bool valid = (t) * 4 * KS + 4 * k + h < n;                                        \
        _Pragma("unroll") for (int m = 0; m < NO; m++) {                                        \
            const double *f = T.fac[m] + (int64_t)IX[k][m] * D;                                 \
            _Pragma("unroll") for (int I = 0; I < DB; I++)                                      \
                w_n[k][m][I] = (valid && ec[I] >= 0) ? f[ec[I]] : 0.0;                          \
        }                                                                                       \
    }

    if (ntrips > 0) {
        LOAD_IDX(0, ix_n, rr_n, s_n)
        if (ntrips > 1) { LOAD_IDX(1, ix_nn, rr_nn, s_nn) }
        LOAD_DATA(0, ix_n)
    }
    for (int t = 0; t < ntrips; t++) {
        double w_c[KS][DB], rr_c[KS];
#pragma unroll
        for (int k = 0; k < KS; k++) {
            rr_c[k] = rr_n[k];
#pragma unroll
            for (int I = 0; I < DB; I++) {
                double v = w_n[k][0][I];
#pragma unroll
                for (int m = 1; m < NO; m++) v *= w_n[k][m][I];      // Hadamard product (sampling.jl:225-227, 277-280)
                if constexpr (WEIGHTED) v *= s_n[k];
                w_c[k][I] = v;
            }
            if constexpr (WEIGHTED) rr_c[k] *= s_n[k];
        }
#pragma unroll
        for (int k = 0; k < KS; k++) {
            rr_n[k] = rr_nn[k];
            if constexpr (WEIGHTED) s_n[k] = s_nn[k];
#pragma unroll
            for (int m = 0; m < NO; m++) ix_n[k][m] = ix_nn[k][m];
        }
        if (t + 1 < ntrips) { LOAD_DATA(t + 1, ix_n) }
        if (t + 2 < ntrips) { LOAD_IDX(t + 2, ix_nn, rr_nn, s_nn) }
#pragma unroll
        for (int k = 0; k < KS; k++) {
            int b = 0;
#pragma unroll
            for (int I = 0; I < DB; I++) {
#pragma unroll
                for (int J = 0; J <= I; J++) {
                    acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(w_c[k][I], w_c[k][J], acc[b], 0, 0, 0);
                    b++;
                }
                bpart[I] = fma(w_c[k][I], rr_c[k], bpart[I]);
            }
        }
    }
#undef LOAD_IDX
#undef LOAD_DATA
    // scale by alpha; reduce b over the four observation groups (lanes j, j+16, j+32, j+48)
    const double alpha = term_alpha(T);
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] *= alpha;
#pragma unroll
    for (int I = 0; I < DB; I++) {
        double v = bpart[I] * alpha;
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        bred[I] = v;
    }
}

// ---- accumulate one item, lean register path: shared baseline (no per-observation linear_values), at most two other
// modes, factor matrices below 4 GiB with fewer than 2^24 rows (TermDev::lean, checked by the host) -----------------------
// Same pipeline as accumulate_reg, with what the general path pays per load taken out: wave-uniform (SGPR) bases with
// 32-bit byte offsets, row offsets by one 24-bit mad, no predicated loads (indices are clamped to the item instead, and
// only the item's last trip masks its operands).
// CODED (a launch with one two-mode relation whose values are at most BDF_K1_CODES distinct numbers -- ratings): the other-mode
// id and the value's 8-bit code arrive as ONE 32-bit word per observation (TermDev::packed), the value minus the mean comes
// from the wave's own table in LDS (the packed factor's space, idle until the factorisation) when it is used.  No value is held in registers two trips ahead: 70 instead of 80 VGPRs, SEVEN
// resident waves per SIMD instead of six, and a third fewer memory instructions per trip.  Same arithmetic, same results.
template <int DP, int NO, bool FULL, bool WIDE = false, bool CODED = false>
__device__ __forceinline__ void accumulate_lean(const SampleArgs &a, const Item &it, int lane, d4 (&acc)[Geo<DP>::NB],
                                       double (&bred)[Geo<DP>::DB], const double *tab = nullptr)
{
    static_assert(!CODED || (NO == 1 && !WIDE), "coded values: one two-mode relation, 32-bit row offsets");
    constexpr int DB = Geo<DP>::DB, NB = Geo<DP>::NB;
    constexpr int KS = (NO == 1) ? (DP == 64 ? BDF_K1_KS64 : BDF_K1_KS) : 1;
    const TermDev &T = a.t[it.term];
    const int D = FULL ? DP : a.D;
    const int j = lane & 15, h = lane >> 4;
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
    double bpart[DB];
    uint32_t eoff[DB];                        // byte offset in a factor row of reversed element 16 I + j
    bool eok[DB];
#pragma unroll
    for (int I = 0; I < DB; I++) {
        bpart[I] = 0.0;
        const int ec = D - 1 - (16 * I + j);
        eok[I] = FULL || ec >= 0;
        eoff[I] = (uint32_t)(ec >= 0 ? ec : 0) * 8u;
    }
    const uint32_t n = (uint32_t)it.count, rowb = (uint32_t)D * 8u;
    const uint32_t ntrips = (n + 4 * KS - 1) / (4 * KS);
    const char *ids[NO], *fac[NO];
#pragma unroll
    for (int m = 0; m < NO; m++) {
        ids[m] = CODED ? (const char *)(T.packed + it.q_begin) : (const char *)(T.colidx + (int64_t)m * T.nnz + it.q_begin);
        fac[m] = (const char *)T.fac[m];
    }
    const char *vals = (const char *)(T.vals + it.q_begin);
    const double mean = T.mean;
    double tab_v = 0.0;
    if (CODED && lane < BDF_K1_CODES) tab_v = T.table[lane] - mean;      // this wave's copy of the table: value - mean by code

    // two register sets, used alternately by even and odd trips (no rotation copies: a copy would have to wait for
    // the load it moves).  Trip t multiplies set t%2; the gathers of trip t+1 fill the other set; the ids and values of
    // trip t+2 are loaded into set t%2 once trip t has used it.
    uint32_t ix[2][KS][NO];
    double rr[2][KS];
    double w[2][KS][NO][DB];
// observation of (trip t, k-step k, lane group h): t * 4 KS + KS h + k -- a lane group's KS observations of a trip are
// neighbours, so that the coded variant fetches their words with ONE load (the packed array carries a spare word at its end)
#define OBS(t, k) ((t) * (4 * KS) + KS * h + (k))
#define LOAD_IDX(t, S)                                                                          \
    if (CODED && KS == 2) {                                                                     \
        uint32_t o = OBS(t, 0);                                                                 \
        o = (o < n ? o : n - 1) * 4u;                                                           \
        const uint2 pw = *(const uint2 *)(ids[0] + o);                                          \
        ix[S][0][0] = pw.x; ix[S][KS - 1][0] = pw.y;                                            \
    } else if (KS == 2 && NO == 1) {          /* the pair's ids and values as one load each (the arrays carry a spare entry) */ \
        uint32_t o = OBS(t, 0);                                                                 \
        o = (o < n ? o : n - 1) * 4u;                                                           \
        const uint2 pi = *(const uint2 *)(ids[0] + o);                                          \
        const d2 pv = *(const d2 *)(vals + 2u * o);                                             \
        ix[S][0][0] = pi.x; ix[S][KS - 1][0] = pi.y;                                            \
        rr[S][0] = pv[0]; rr[S][KS - 1] = pv[1];                                                \
    } else {                                                                                    \
    _Pragma("unroll") for (int k = 0; k < KS; k++) {                                            \
        uint32_t o = OBS(t, k);                                                                 \
        o = (o < n ? o : n - 1) * 4u;                                                           \
        _Pragma("unroll") for (int m = 0; m < NO; m++) ix[S][k][m] = *(const uint32_t *)(ids[m] + o); \
        if (!CODED) rr[S][k] = *(const double *)(vals + 2u * o);                                \
    }                                                                                           \
    }
#define LOAD_DATA(S)                                                                            \
    _Pragma("unroll") for (int k = 0; k < KS; k++)                                              \
        _Pragma("unroll") for (int m = 0; m < NO; m++)                                          \
            _Pragma("unroll") for (int I = 0; I < DB; I++)                                      \
                w[S][k][m][I] = WIDE ? *(const double *)(fac[m] + ((uint64_t)ix[S][k][m] * rowb + eoff[I]))            \
                                     : *(const double *)(fac[m] + (__umul24(ix[S][k][m], rowb) + eoff[I]));
#define TRIP(t, C, X)                                                                           \
    {                                                                                           \
        LOAD_DATA(X)  /* unconditional (ids are clamped to the item): a branch here would cost exact waitcnts */ \
        double w_c[KS][DB];                                                                     \
        _Pragma("unroll") for (int k = 0; k < KS; k++)                                          \
            _Pragma("unroll") for (int I = 0; I < DB; I++) {                                    \
                double v = w[C][k][0][I];                                                       \
                _Pragma("unroll") for (int m = 1; m < NO; m++) v *= w[C][k][m][I];              \
                w_c[k][I] = v;                                                                  \
            }                                                                                   \
        if ((t) + 1 >= ntrips || !FULL) {     /* ragged last trip; padded elements when D < DP */ \
            _Pragma("unroll") for (int k = 0; k < KS; k++) {                                    \
                const bool valid = OBS(t, k) < n;                                               \
                _Pragma("unroll") for (int I = 0; I < DB; I++) w_c[k][I] = (valid && eok[I]) ? w_c[k][I] : 0.0; \
            }                                                                                   \
        }                                                                                       \
        _Pragma("unroll") for (int k = 0; k < KS; k++) {                                        \
            /* (__umul24 in LOAD_DATA takes the low 24 bits of the packed word: the id) */      \
            const double r = CODED ? tab[ix[C][k][0] >> 24] : rr[C][k] - mean;                  \
            int b = 0;                                                                          \
            _Pragma("unroll") for (int I = 0; I < DB; I++) {                                    \
                _Pragma("unroll") for (int J = 0; J <= I; J++) {                                \
                    acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(w_c[k][I], w_c[k][J], acc[b], 0, 0, 0);     \
                    b++;                                                                        \
                }                                                                               \
                bpart[I] = fma(w_c[k][I], r, bpart[I]);                                         \
            }                                                                                   \
        }                                                                                       \
        LOAD_IDX((t) + 2, C)                                                                    \
    }

    LOAD_IDX(0u, 0)
    LOAD_IDX(1u, 1)
    LOAD_DATA(0)
    // (its load was issued before the ids': it has arrived with them; a wave's LDS operations execute in order, so the reads
    // below need no wait for this write, and the factorisation's writes none for those reads)
    if (CODED && lane < BDF_K1_CODES) const_cast<double *>(tab)[lane] = tab_v;
    // trips go in pairs in one straight-line block (a branch between them lets the compiler sink the run-ahead loads to
    // their use); for an odd count the last one is empty: its operands are masked to zero
    for (uint32_t t = 0; t < ntrips; t += 2) {
        TRIP(t, 0, 1)
        TRIP(t + 1, 1, 0)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the run-ahead loads of the last trips
#undef LOAD_IDX
#undef LOAD_DATA
#undef TRIP
#undef OBS
    const double alpha = term_alpha(T);
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] *= alpha;
#pragma unroll
    for (int I = 0; I < DB; I++) {
        double v = bpart[I] * alpha;
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        bred[I] = v;
    }
}

// path and other-mode count are wave-uniform.  MATRIX: the kernel variant for launches whose terms are all two-mode
// relations on the lean path -- without the tensor and general gathers the D <= 32 kernel needs 78 registers instead of
// 92 (6 resident waves per SIMD instead of 5, and room beside 5 of them for a wave of the prediction update)
// WEIGHTED (k_rows_w alone): every term takes the general gather in its weighted form.
template <int DP, bool MATRIX, bool CODED = false, bool WEIGHTED = false>
__device__ __forceinline__ void accumulate_any(const SampleArgs &a, const Item &it, int lane, d4 (&acc)[Geo<DP>::NB],
                                      double (&bred)[Geo<DP>::DB], const double *tab = nullptr)
{
    if constexpr (WEIGHTED) {
        static_assert(!MATRIX && !CODED, "weighted rows: the general gather");
        const int now = a.t[it.term].n_other;
        if (now == 1) accumulate_reg<DP, 1, true>(a, it, lane, acc, bred);
        else if (now == 2) accumulate_reg<DP, 2, true>(a, it, lane, acc, bred);
        else accumulate_reg<DP, 3, true>(a, it, lane, acc, bred);
        return;
    }
    if constexpr (CODED) {                   // one two-mode relation, lean gather, coded values (checked by the host)
        if (a.D == DP) accumulate_lean<DP, 1, true, false, true>(a, it, lane, acc, bred, tab);
        else accumulate_lean<DP, 1, false, false, true>(a, it, lane, acc, bred, tab);
        return;
    }
    const int no = a.t[it.term].n_other;
    if constexpr (DP == 64) {
        if (a.t[it.term].lean == 2) {        // a factor matrix of 4 GiB or more (e.g. 10M rows at D = 64): 64-bit row offsets
            if (a.D == DP) {
                if (MATRIX || no == 1) accumulate_lean<DP, 1, true, true>(a, it, lane, acc, bred);
                else accumulate_lean<DP, 2, true, true>(a, it, lane, acc, bred);
            } else {
                if (MATRIX || no == 1) accumulate_lean<DP, 1, false, true>(a, it, lane, acc, bred);
                else accumulate_lean<DP, 2, false, true>(a, it, lane, acc, bred);
            }
            return;
        }
    }
    if constexpr (MATRIX) {                  // every term of the launch: two modes, lean gather (checked by the host)
        if (a.D == DP) accumulate_lean<DP, 1, true>(a, it, lane, acc, bred);
        else accumulate_lean<DP, 1, false>(a, it, lane, acc, bred);
        return;
    }
    if (a.t[it.term].lean == 1) {
        if (a.D == DP) {
            if (no == 1) accumulate_lean<DP, 1, true>(a, it, lane, acc, bred);
            else accumulate_lean<DP, 2, true>(a, it, lane, acc, bred);
        } else {
            if (no == 1) accumulate_lean<DP, 1, false>(a, it, lane, acc, bred);
            else accumulate_lean<DP, 2, false>(a, it, lane, acc, bred);
        }
        return;
    }
    if (no == 1) accumulate_reg<DP, 1>(a, it, lane, acc, bred);
    else if (no == 2) accumulate_reg<DP, 2>(a, it, lane, acc, bred);
    else accumulate_reg<DP, 3>(a, it, lane, acc, bred);
}

// ---- sum the partials of a split row in slot order (fixed order: the result does not depend on which wave does it) ---
template <int DP>
__device__ __forceinline__ void sum_partials(const PlanDev &p, const SplitRow &sr, int lane, d4 (&acc)[Geo<DP>::NB],
                                    double (&bred)[Geo<DP>::DB])
{
    constexpr int DB = Geo<DP>::DB, NB = Geo<DP>::NB, PSZ = Geo<DP>::PSZ;
    constexpr int U = 1;                              // slots loaded per trip
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int I = 0; I < DB; I++) bred[I] = 0.0;
    for (int s0 = 0; s0 < sr.n_slots; s0 += U) {
        double v[U][NB * 4 + DB];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int s = (s0 + u < sr.n_slots) ? s0 + u : sr.n_slots - 1;
            const double *src = p.partials + (int64_t)(sr.slot_begin + s) * PSZ;
#pragma unroll
            for (int e = 0; e < NB * 4; e++) v[u][e] = src[e * 64 + lane];
#pragma unroll
            for (int I = 0; I < DB; I++) v[u][NB * 4 + I] = src[NB * 4 * 64 + I * 16 + (lane & 15)];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (s0 + u < sr.n_slots) {
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[b][r] += v[u][b * 4 + r];
#pragma unroll
                for (int I = 0; I < DB; I++) bred[I] += v[u][NB * 4 + I];
            }
        }
    }
}

// ---- the launch: wave w < n_split accumulates split item w and publishes its partial; the wave whose publication
// completes a row finishes that row (agent-scope release / acquire around a per-row arrival counter, placement
// independent: cdna_hip_programming.md Guideline 16).  The remaining waves take one direct row each. -----------------------
// One work item (index wi in [split items | direct items]) on one wave.
// SPIKE (k_rows_ss.hip): the row's prior is the spike-and-slab one -- the same accumulation, then spike.h's coordinate sweep
// instead of the factorisation; the wave polls nothing.
template <int DP, bool DUMP, bool MATRIX, bool CODED = false, bool WEIGHTED = false, bool SPIKE = false>
__device__ __forceinline__ void process_item(const SampleArgs &a, const PlanDev &p, const int64_t wid, const int lane, double *tri)
{
    double *const tab = tri;          // CODED: the wave's value table (BDF_K1_CODES doubles) sits in the packed factor's space until the factorisation
    using GG = Geo<DP>;
    constexpr int DB = GG::DB, NB = GG::NB, PSZ = GG::PSZ;
    const int j = lane & 15, h = lane >> 4;
    const int D = a.D;
    d4 acc[NB];
    double bv[DB];
    int64_t row;
    STAMP(0);
    SPAN_BEGIN();
#ifdef BDF_K1_STAMPS
    if (lane == 0 && a.b_dump && wid < 65536) {           // where the wave runs: HW_ID (wave, SIMD, CU, SH, SE) and XCC_ID
        ((unsigned long long *)a.b_dump)[wid * 16 + 9] = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 4) |
            ((unsigned long long)__builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4) );
        ((unsigned long long *)a.b_dump)[wid * 16 + 10] = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20);
    }
#endif

    const bool is_split = wid < p.n_split;                      // wave-uniform
    const Item it = is_split ? p.split[wid] : p.direct[wid - p.n_split];
    row = it.row;
    // a direct row's normals (lane c < D draws number D-1-c of the row's stream) are drawn BEFORE its gathers: the
    // Philox / Box-Muller arithmetic then runs under the matrix-pipe-bound accumulation instead of after it
    double z = 0.0;
    const bool early_z = !DUMP && !is_split;
    if (early_z && lane < D) z = bdf_normal(a.seed, a.sweep, BDF_P_ROW, a.entity_tag, (uint64_t)(uint32_t)it.orig, D - 1 - lane);
    double uu = 0.0;                  // SPIKE: the uniform of the lane's component, drawn where its normal is
    if (SPIKE && early_z && lane < D) uu = bdf_uniform(a.seed, a.sweep, BDF_P_SPIKE, a.entity_tag, (uint64_t)(uint32_t)it.orig, (uint32_t)(D - 1 - lane));
    if (it.count > 0) accumulate_any<DP, MATRIX, CODED, WEIGHTED>(a, it, lane, acc, bv, tab);
    else {
#pragma unroll
        for (int b = 0; b < NB; b++) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int I = 0; I < DB; I++) bv[I] = 0.0;
    }
    STAMP(1);
    if (is_split) {
        // slot layout [block*4 + r][lane] then b[I][j]; write-through (sc1) stores: the slab needs no L2 write-back
        double *dst = p.partials + (int64_t)it.slot * PSZ;
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                __hip_atomic_store(dst + (b * 4 + r) * 64 + lane, acc[b][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane < 16) {
#pragma unroll
            for (int I = 0; I < DB; I++)
                __hip_atomic_store(dst + NB * 4 * 64 + I * 16 + lane, bv[I], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // publish: every lane's write-through stores have completed, then one arrival
        const SplitRow sr = p.rows[it.srow];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(p.arrived + it.srow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        old = __builtin_amdgcn_readfirstlane(old);
        if (old != sr.n_slots - 1) { SPAN_END(); return; }       // not the last item of the row
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) p.arrived[it.srow] = 0;                  // ready for the next launch
        // the finisher's normals before the partial sums are loaded: the Box-Muller arithmetic needs ~40 registers
        if (!DUMP && lane < D) z = bdf_normal(a.seed, a.sweep, BDF_P_ROW, a.entity_tag, (uint64_t)(uint32_t)it.orig, D - 1 - lane);
        if (SPIKE && lane < D) uu = bdf_uniform(a.seed, a.sweep, BDF_P_SPIKE, a.entity_tag, (uint64_t)(uint32_t)it.orig, (uint32_t)(D - 1 - lane));
        sum_partials<DP>(p, sr, lane, acc, bv);
        STAMP(2);
    }
    if (!SPIKE && a.ready) {
        // launched without waiting for the hyperprior draw (bdf_gibbs_sweep: the draw runs on CUs this kernel never uses, so
        // it cannot be starved): poll its flag here, where the prior is first needed -- the gathers above have hidden most of
        // the wait -- and read the pack with agent-scope loads (past the non-coherent L2 lines of the previous sweep's pack)
        int spins = 0;
#ifdef BDF_K1_SPANS
        const unsigned long long t_poll = __builtin_amdgcn_s_memrealtime();
#endif
        while ((int32_t)(__hip_atomic_load(a.ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - a.ready_want) < 0) {
            __builtin_amdgcn_s_sleep(16);
            if (++spins > (1 << 22)) { if (lane == 0) atomicOr_system(a.flag, 16); break; }      // bounded: ~seconds
        }
        SPAN_WAIT(t_poll);
#pragma unroll
        for (int b = 0; b < NB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                acc[b][r] += __hip_atomic_load(a.prior_c + (b * 4 + r) * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int J = 0; J < DB; J++) {
            const int ec = D - 1 - (16 * J + j);
            if (ec >= 0) bv[J] += __hip_atomic_load(a.prior_b + ec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
#pragma unroll
        for (int b = 0; b < NB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) acc[b][r] += a.prior_c[(b * 4 + r) * 64 + lane];
        }
#pragma unroll
        for (int J = 0; J < DB; J++) {
            const int ec = D - 1 - (16 * J + j);
            if (ec >= 0) bv[J] += a.prior_b[(a.mu_is_matrix ? row * D : 0) + ec];
        }
    }
    STAMP(3);

    if (DUMP) {
        // P~ and b of the row (bdf_row_system): element (i, c) of the reversed system is entry (D-1-i, D-1-c) of P
        int b = 0;
#pragma unroll
        for (int I = 0; I < DB; I++)
#pragma unroll
            for (int J = 0; J <= I; J++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int ei = D - 1 - (16 * I + h + 4 * r), ec = D - 1 - (16 * J + j);
                    if (ei >= 0 && ec >= 0) {
                        a.P_dump[(row * D + ec) * D + ei] = acc[b][r];
                        if (I != J) a.P_dump[(row * D + ei) * D + ec] = acc[b][r];
                    }
                }
                b++;
            }
        if (h == 0) {
#pragma unroll
            for (int J = 0; J < DB; J++) {
                const int ec = D - 1 - (16 * J + j);
                if (ec >= 0) a.b_dump[row * D + ec] = bv[J];
            }
        }
        return;
    }

    STAMP(4);
    if constexpr (SPIKE) {
        spike_finish<DP>(a, acc, bv, z, uu, row, lane, tri);
        SPAN_END();
        return;
    }

    double A[NB * 4];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) A[b * 4 + r] = acc[b][r];
    double ts[DB];                                // ts[J] in lane j: t_(16 J + j) once its step has passed; the last column's
#pragma unroll                                    // (and any column's before its step) is still in bv
    for (int J = 0; J < DB; J++) ts[J] = 0.0;
    constexpr bool LOCAL = K1Local<DP>::value;    // DP = 64: one panel of the factor in LDS at a time, the backward solve fed from the registers
    if (D < DP && !LOCAL) zero_packed_factor<DP>(tri, lane);
    if constexpr (LOCAL)
        factor_all_blocked_local<DP>(A, bv, ts, tri, j, h, D, std::make_integer_sequence<int, DP - 1>{});
    else
        factor_all_blocked<DP>(A, bv, ts, tri, j, h, D, std::make_integer_sequence<int, DP - 1>{});
    STAMP(5);

    // lane c = column c: pivot d_c from the packed factor, t_c (the forward solve, unscaled) from the extra row
    const int cK = (lane < DP) ? (lane >> 4) : 0;
    const typename GG::ColRT cr = GG::col_rt(lane < DP ? lane : 0);       // this lane's column of the packed factor
    wave_sync();
    double dv = 1.0, tv = 0.0;
    if (lane < D) dv = LOCAL ? tri[GeoL<DP>::PIV + lane] : tri[cr.cbase + (lane & 3) * cr.nr4];      // the diagonal entry is the first of its row class
    if (!(dv > 0.0)) atomicOr_system(a.flag, 1);                      // a pivot that is not positive (or NaN): not positive definite
#pragma unroll
    for (int J = 0; J < DB; J++) tv = (lane < D && cK == J) ? ts[J] : tv;
    const double rdv = fast_rcp(dv);
    // L w = b, y = w + z carried as yh = y sqrt(d) = t + z sqrt(d);  then Lt' x = yh
    double yh = fma(z, dv * fast_rsqrt(dv), tv);
    if constexpr (LOCAL) {
        backward_rows<DP>(A, yh, rdv, tri, lane);
    } else {
        unsigned colq[4];                          // LDS byte addresses: row i of this lane's column at colq[i & 3] + 8 (i >> 2)
#pragma unroll
        for (int q = 0; q < 4; q++)
            colq[q] = (unsigned)(size_t)(__attribute__((address_space(3))) double *)(tri + cr.cbase + q * cr.nr4 - cr.q);
        backward_all<DP>(yh, rdv, colq, std::make_integer_sequence<int, DP / 16>{});
    }
    if (lane < D) a.out[row * D + (D - 1 - lane)] = yh * rdv;
    STAMP(8);
    SPAN_END();
}

}  // namespace
