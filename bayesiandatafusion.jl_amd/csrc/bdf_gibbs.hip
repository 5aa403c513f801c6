// bdf_gibbs.hip -- one Gibbs iteration of macau (src/macau.jl:80-203) enqueued from native code: the latent rows of every
// entity (sample_latent_all2! / sample_user2_all!, src/sampling.jl:149-289), the exchange of the sampled rows between GPUs,
// every entity's hyperprior (src/sampling.jl:116-127, src/normal_wishart.jl:38-42) and the test-set prediction update
// (macau.jl:142-184), with the beta update and the per-row prior means of side information and the relations' own models.  The
// same pieces can be enqueued one by one, with plain stream order: bdf_gibbs_step_relations, _rows, _draws, _hyper, _beta.
//
// Three HIP streams: rows | hyperpriors | prediction updates.  The hyperprior of entity j runs beside the rows of entity
// j+1, the prediction update of sweep t beside the rows of sweep t+1 (every entity's rows rotate through three buffers).
// Hand-overs towards the hyperprior and prediction streams are HIP events that ride on the producing kernel's own dispatch
// packet (hipExtLaunchKernelGGL stop events): no marker packets on the row stream.  The hand-over BACK to the row stream --
// (mu, Lambda) of the draw, needed by the entity's next row launch -- is, by default, not an event: the draw runs on CUs
// the row kernels never occupy (bdf_ctx_create_rows), publishes a per-entity epoch when its prior pack is written, and
// the row kernel's waves poll that word where they first need the prior (BDF_NO_POLL=1, a profiler that serialises the
// streams, or several ranks: event waits instead).
#include "bdf_common.h"
#include "rows.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

struct bdf_gibbs {
    bdf_ctx *rows = nullptr;             // borrowed: the caller's context
    bdf_ctx *hyper = nullptr, *pred = nullptr;   // owned (own streams): deleted by the destructor, after the gate
    bdf_ctx *gate = nullptr;             // owned, with polling: a second stream on the reserved CUs for the one-wave gate in front of the prediction update
    bdf_ctx *step_hyper = nullptr;       // where bdf_gibbs_step_draws / _hyper enqueue: hyper, or -- BDF_NO_OVERLAP, one stream for everything -- rows
    int D = 0;
    struct Ent {
        bdf_gibbs_entity d{};            // the caller's description: every buffer in it is borrowed
        int cur = 0;                     // buffer holding the current rows
        DevEvent ev_rows, ev_hyper;      // rows of this sweep complete (and exchanged) | (mu, Lambda) of this sweep complete
        DevEvent ev_beta;                // side information: beta (and lambda_beta) of this sweep complete
        bool beta_recorded = false;
        bool hyper_recorded = false;
        // number of hyperprior draws enqueued for this entity so far: the value its next draw publishes in ready_dev and the
        // entity's next row launch polls for.  Private and strictly increasing -- NOT the caller's sweep number, which may
        // repeat or restart (a repeated number would let the poll pass while the draw is still writing the pack)
        uint32_t epoch = 0;
        // the rows' hand-over to the chain by counter (no event): the sum the 64 words of done_dev reach when every row launch of
        // this entity enqueued so far has completed (wraps; compared as a difference)
        DevBuf<uint32_t> done_dev;
        uint32_t done_target = 0;
        hipEvent_t t_start = nullptr, t_stop = nullptr;      // borrowed -- bdf_gibbs_time_rows: attached to the next row launch of this entity
        unsigned long long *span = nullptr;                  // borrowed -- bdf_gibbs_span_rows: SampleArgs::span of the next row launch of this entity
    };
    std::vector<Ent> ent;
    bdf_pairs *test = nullptr;           // borrowed
    int32_t test_entity[BDF_MAX_MODES] = {};
    double test_mean = 0.0, clamp_lo = 0.0, clamp_hi = 0.0, class_cut = 0.0;
    double *stats_dev = nullptr;         // borrowed
    DevEvent ev_pred[3];                 // prediction update number k complete: ev_pred[k % 3]
    uint64_t pred_at[3] = {0, 0, 0};     // ... and the iteration count (n_iter) at which it was enqueued
    uint64_t n_pred = 0;                 // prediction updates enqueued so far
    uint64_t n_iter = 0;                 // iterations enqueued so far (with or without a prediction update)
    bdf_comm *comm = nullptr;            // borrowed, nullable: exchange of the sampled rows between the ranks after every entity
    std::vector<bdf_gibbs_relation> rels; // relations with a model of their own (alpha sampled, relation features): bdf_gibbs_set_relations
    DevBuf<double> rel_sse;              // dev, 8 doubles: the squared-error statistics of sample_alpha
    // The row stream has NO wait for the hyperprior draws when they run on reserved CUs (bdf_ctx_create_rows): a draw there
    // cannot be starved by the chip-filling row kernel, so the row kernel is enqueued right behind its predecessor (back-to-back
    // row kernels start with no gap; a wait for another stream's event costs the row stream ~10 us even when long satisfied:
    // profiles/r02_sweep_timeline_events.txt) and its waves poll ready[entity] where they first need the prior.
    DevBuf<uint32_t> ready_dev;          // per entity: iteration number of the last completed draw
    bool polling = false;
    // BDF_DEBUG: where the host's time in bdf_gibbs_sweep goes (waiting for the prediction update of two sweeps ago = the device
    // is the bottleneck; enqueueing = the host is)
    bool debug = false;
    double host_wait_us = 0.0, host_enqueue_us = 0.0;
    uint64_t n_sweeps = 0;
    ~bdf_gibbs();
};

namespace {

// do kernels on the two streams run side by side?  HIP multiplexes streams onto a few hardware queues; two streams on one
// queue serialise whatever the hand-over mechanism.  Timing test: a 60 us spin on each, together.
__global__ void k_spin(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// Can a kernel on `b` run WHILE a kernel on `a` is running?  (Not under profilers that serialise kernels across queues --
// rocprofv3 --pmc does -- nor if the two streams share a hardware queue.)  A kernel on `a` spins until a flag is set by a
// kernel enqueued on `b` afterwards; bounded at 20 ms.  The row kernels poll for the hyperprior draw only if this holds.
__global__ void k_wait_flag(const uint32_t *flag, long long max_ticks, uint32_t *timed_out)
{
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > max_ticks) { *timed_out = 1; break; }
    }
}
__global__ void k_set_flag(uint32_t *flag) { __hip_atomic_store(flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }

// The gate in front of the prediction update: one wave that returns when the 64 done counters of a row launch (SampleArgs::done)
// sum to `target`, as k_hyper_chain's partial-sum workgroups wait (k_hyper.hip) -- every row of the launch is in memory then.  The
// event on ITS dispatch is what the prediction stream waits for, so that nothing rides on the row launch.  Bounded like the chain's.
__global__ __launch_bounds__(64) void k_rows_gate(const uint32_t *done, uint32_t target, int *flag)
{
    int spins = 0;
    for (;;) {
        uint32_t v = __hip_atomic_load(done + BDF_DONE_STRIDE * threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if ((int32_t)(v - target) >= 0) break;
        __builtin_amdgcn_s_sleep(8);
        if (++spins > (1 << 22)) { if (threadIdx.x == 0) atomicOr_system(flag, 16); break; }      // bounded: a bug must not hang the device
    }
}

// Something other than a row launch has written entity E's sample, or may have: K1c's gather images of its buffers are stale
// (k_gather_image.hip) -- the next launch that gathers one packs it anew.  The row launches of bdf_gibbs_sweep vouch for the images of
// the chain's buffers (bdf_ctx::gimg_trust), so EVERY other writer of a sample comes through here: the state at creation, a state
// put back (bdf_gibbs_warm_device, bdf_gibbs_set_recorded), the host (bdf_gibbs_sample_written).
void sample_written(bdf_gibbs *g, const bdf_gibbs::Ent &E)
{
    for (int b = 0; b < 3; b++) bdf_gather_image_invalidate(g->rows, E.d.sample[b]);
}

int streams_concurrent(hipStream_t a, hipStream_t b, bool *yes)
{
    DevBuf<uint32_t> buf;
    if (int rc = buf.alloc(2)) return rc;
    uint32_t *d = buf.get();
    BDF_HIP(hipMemsetAsync(d, 0, 2 * sizeof(uint32_t), a));
    BDF_HIP(hipStreamSynchronize(a)); BDF_HIP(hipStreamSynchronize(b));
    hipLaunchKernelGGL(k_wait_flag, dim3(1), dim3(1), 0, a, (const uint32_t *)d, 2000000LL, d + 1);
    hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(1), 0, b, d);
    BDF_HIP(hipStreamSynchronize(a)); BDF_HIP(hipStreamSynchronize(b));
    uint32_t h[2] = {0, 0};
    BDF_HIP(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
    *yes = h[1] == 0;
    return BDF_OK;
}

int streams_overlap(hipStream_t a, hipStream_t b, bool *yes)
{
    DevEvent e0, e1, e2;
    int rc;
    if ((rc = e0.create(hipEventDefault)) || (rc = e1.create(hipEventDefault)) || (rc = e2.create(hipEventDefault))) return rc;
    BDF_HIP(hipStreamSynchronize(a)); BDF_HIP(hipStreamSynchronize(b));
    float best = 1e9f;
    for (int rep = 0; rep < 3; rep++) {
        BDF_HIP(hipEventRecord(e0, a));
        BDF_HIP(hipStreamWaitEvent(b, e0, 0));
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, a, 6000LL);       // 100 MHz clock: 60 us
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, b, 6000LL);
        BDF_HIP(hipEventRecord(e1, b));
        BDF_HIP(hipStreamWaitEvent(a, e1, 0));
        BDF_HIP(hipEventRecord(e2, a));
        BDF_HIP(hipEventSynchronize(e2));
        float ms = 0.f;
        BDF_HIP(hipEventElapsedTime(&ms, e0, e2));
        best = std::min(best, ms);
    }
    *yes = best < 0.100f;               // side by side: ~0.065 ms; serialised: ~0.125 ms
    return BDF_OK;
}

// A non-blocking stream, optionally confined to a set of CUs.  CU mask bits are interleaved over the XCDs (bits 0..7 are CU 0
// of shader engine 0 of XCD 0..7: tools/cu_mask_probe.hip), so `reserve` = 8 k bits set aside k CUs in every XCD -- a kernel's
// workgroups are dealt over the XCDs, every XCD must have a CU of the mask.  reserved = true: the stream runs on those CUs
// only; false: on all the others.
// The streams live in a process-wide pool and are never destroyed: host frameworks keep references to a stream they have
// used (torch: allocator pools per stream, events recorded on it) beyond the life of the context that ran on it, and
// destroying it under them crashes at the framework's own teardown.  Slot k of (device, reserve, role) is always the same
// stream, so later engines of a process pick the same streams as the first.
int pooled_stream(int device, int reserve, bool reserved, int slot, hipStream_t *out)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, int>, hipStream_t> pool;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple(device, reserve, reserved ? 1 : 0, slot);
    auto it = pool.find(key);
    if (it != pool.end()) { *out = it->second; return BDF_OK; }
    hipStream_t st;
    if (reserve <= 0) {
        BDF_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    } else {
        hipDeviceProp_t prop;
        BDF_HIP(hipGetDeviceProperties(&prop, device));
        const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
        std::vector<uint32_t> mask((size_t)words, 0u);
        for (int i = 0; i < ncu; i++)
            if ((i < reserve) == reserved) mask[(size_t)(i / 32)] |= 1u << (i % 32);
        BDF_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask.data()));
    }
    pool[key] = st;
    *out = st;
    return BDF_OK;
}

int make_side_ctx(bdf_ctx *main, const std::vector<bdf_ctx *> &apart, bool reserved, bdf_ctx **out)
{
    // a few candidate streams; the first that overlaps with the row stream and with every stream in `apart`
    std::unique_ptr<bdf_ctx> fallback;
    for (int attempt = 0; attempt < 8; attempt++) {
        hipStream_t st;
        // slot 0 of the unreserved role is the row stream itself
        int rc = pooled_stream(main->device, main->reserve_cus, reserved, attempt + 1, &st);
        if (rc) return rc;
        if (st == main->stream) continue;
        bool taken = false;
        for (bdf_ctx *o : apart) taken = taken || o->stream == st;
        if (taken) continue;
        bdf_ctx *made;
        rc = bdf_ctx_create(main->device, (void *)st, main->seed, &made);
        if (rc) return rc;
        std::unique_ptr<bdf_ctx> c(made);
        c->reserve_cus = main->reserve_cus;
        c->on_reserved = (reserved && main->reserve_cus > 0) ? 1 : 0;
        bool ok = true;
        if ((rc = streams_overlap(st, main->stream, &ok))) return rc;
        for (bdf_ctx *o : apart)
            if (ok && (rc = streams_overlap(st, o->stream, &ok))) return rc;
        if (ok) {
            *out = c.release();
            return BDF_OK;
        }
        if (!fallback) fallback = std::move(c);
    }
    *out = fallback.release();                    // no candidate runs beside the others: correct, only slower
    return BDF_OK;
}

}  // namespace

extern "C" int bdf_ctx_create_rows(int device, uint64_t seed, int reserve_cus, bdf_ctx **out)
{
    BDF_REQUIRE(out && reserve_cus >= 0 && reserve_cus % 8 == 0 && reserve_cus <= 64, BDF_ERR_ARG,
                "bdf_ctx_create_rows: reserve_cus must be 0, 8, 16, ... 64 (whole CUs per XCD)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        bdf_set_error("bdf_ctx_create_rows: no HIP device visible (this library has no CPU path)");
        return BDF_ERR_NOGPU;
    }
    BDF_REQUIRE(device >= 0 && device < ndev, BDF_ERR_ARG, "bdf_ctx_create_rows: device %d out of range", device);
    BDF_HIP(hipSetDevice(device));
    hipStream_t st;
    int rc = pooled_stream(device, reserve_cus, false, 0, &st);
    if (rc) return rc;
    bdf_ctx *c;
    if ((rc = bdf_ctx_create(device, (void *)st, seed, &c))) return rc;
    c->reserve_cus = reserve_cus;
    *out = c;
    return BDF_OK;
}

extern "C" int bdf_ctx_create_side(bdf_ctx *main_ctx, bdf_ctx *const *apart, int n_apart, int reserved, bdf_ctx **out)
{
    BDF_REQUIRE(main_ctx && out && n_apart >= 0 && (n_apart == 0 || apart), BDF_ERR_ARG, "bdf_ctx_create_side: bad argument");
    std::vector<bdf_ctx *> ap(apart, apart + n_apart);
    return make_side_ctx(main_ctx, ap, reserved != 0, out);
}

extern "C" int bdf_gibbs_create(bdf_ctx *rows_ctx, int D, int n_entities, const bdf_gibbs_entity *ents, bdf_gibbs **out)
{
    BDF_REQUIRE(rows_ctx && ents && out, BDF_ERR_ARG, "bdf_gibbs_create: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_gibbs_create: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(n_entities >= 1 && n_entities <= 64, BDF_ERR_ARG, "bdf_gibbs_create: 1..64 entities");
    for (int j = 0; j < n_entities; j++) {
        const bdf_gibbs_entity &e = ents[j];
        BDF_REQUIRE(e.n_terms >= 1 && e.n_terms <= BDF_MAX_TERMS, BDF_ERR_ARG, "bdf_gibbs_create: entity %d takes part in %d relations (1..%d)", j, e.n_terms, BDF_MAX_TERMS);
        BDF_REQUIRE(e.sample[0] && e.sample[1] && e.sample[2] && e.mu && e.Lambda && e.mu0 && e.WI && e.sumU && e.UUt && e.prior_pack && e.draws,
                    BDF_ERR_ARG, "bdf_gibbs_create: entity %d has a NULL buffer", j);
        BDF_REQUIRE(!e.feat || (e.beta && e.uhat && e.mu_matrix && e.Tinv && e.lambda_beta), BDF_ERR_ARG,
                    "bdf_gibbs_create: entity %d has side information but a NULL beta / uhat / mu_matrix / Tinv / lambda_beta", j);
        BDF_REQUIRE(!e.spike || (e.spike_state && !e.feat && !e.bg_Lambda), BDF_ERR_ARG,
                    "bdf_gibbs_create: entity %d has the spike-and-slab prior: spike_state must be set, side information and a background are not taken", j);
        BDF_REQUIRE(!e.nonneg || (e.nonneg_tau && !e.spike && !e.feat && !e.bg_Lambda), BDF_ERR_ARG,
                    "bdf_gibbs_create: entity %d has the non-negative prior: nonneg_tau must be set; the spike-and-slab prior, side information and a background / dense relation are not taken", j);
        BDF_REQUIRE(!e.feat || e.feat->m == e.N, BDF_ERR_ARG, "bdf_gibbs_create: entity %d has %lld rows but its feature matrix %lld", j,
                    (long long)e.N, e.feat ? (long long)e.feat->m : 0LL);
        for (int t = 0; t < e.n_terms; t++) {
            BDF_REQUIRE(e.terms[t].rel, BDF_ERR_ARG, "bdf_gibbs_create: entity %d term %d has no relation", j, t);
            for (int k = 0; k < e.terms[t].rel->n_modes; k++)
                BDF_REQUIRE(e.terms[t].entity_of_mode[k] >= 0 && e.terms[t].entity_of_mode[k] < n_entities, BDF_ERR_ARG,
                            "bdf_gibbs_create: entity %d term %d mode %d names entity %d", j, t, k, e.terms[t].entity_of_mode[k]);
        }
    }
    BDF_HIP(hipSetDevice(rows_ctx->device));
    std::unique_ptr<bdf_gibbs> owner(new bdf_gibbs());       // a failure below releases what exists so far
    bdf_gibbs *g = owner.get();
    g->rows = rows_ctx; g->D = D;
    int rc;
    if ((rc = make_side_ctx(rows_ctx, {}, true, &g->hyper)) || (rc = make_side_ctx(rows_ctx, {g->hyper}, false, &g->pred))) return rc;
    g->step_hyper = getenv("BDF_NO_OVERLAP") ? g->rows : g->hyper;
    g->polling = rows_ctx->reserve_cus > 0 && g->hyper->on_reserved && !getenv("BDF_NO_POLL");
    if (g->polling) {
        bool conc = false;
        if ((rc = streams_concurrent(rows_ctx->stream, g->hyper->stream, &conc))) return rc;
        g->polling = conc;              // kernels of the two streams do not run side by side here (a profiler serialising them): events
    }
    // (the gate's stream: on the reserved CUs like the chain's, so that its wave never takes a row slot; beside the other three if it can)
    if (g->polling && (rc = make_side_ctx(rows_ctx, {g->hyper, g->pred}, true, &g->gate))) return rc;
    if (g->polling && !g->gate) g->polling = false;         // (no stream left for it: events everywhere, as without reserved CUs)
    g->debug = getenv("BDF_DEBUG") != nullptr;
    if (g->debug)
        fprintf(stderr, "[bdf_gibbs] reserve_cus=%d hyperprior stream on reserved CUs=%d polling=%d\n", rows_ctx->reserve_cus,
                g->hyper->on_reserved, (int)g->polling);
    if ((rc = g->ready_dev.alloc((size_t)n_entities))) return rc;
    BDF_HIP(hipMemsetAsync(g->ready_dev, 0, (size_t)n_entities * sizeof(uint32_t), rows_ctx->stream));
    BDF_HIP(hipStreamSynchronize(rows_ctx->stream));
    g->ent.resize((size_t)n_entities);
    for (int j = 0; j < n_entities; j++) {
        auto &E = g->ent[(size_t)j];
        E.d = ents[j];
        sample_written(g, E);                         // (the initial state; images an earlier chain left at these addresses)
        if ((rc = E.ev_rows.create(hipEventDefault)) || (rc = E.ev_hyper.create(hipEventDefault))) return rc;      // (they ride on dispatch packets: plain events)
        if (E.d.feat && (rc = E.ev_beta.create(hipEventDisableTiming))) return rc;
    }
    for (int k = 0; k < 3; k++)
        if ((rc = g->ev_pred[k].create(hipEventDisableTiming))) return rc;
    if (g->polling) {
        const size_t bytes = (size_t)BDF_DONE_SHARDS * BDF_DONE_STRIDE * sizeof(uint32_t);
        for (int j = 0; j < n_entities; j++) {
            if ((rc = g->ent[(size_t)j].done_dev.alloc_bytes(bytes))) return rc;
            BDF_HIP(hipMemsetAsync(g->ent[(size_t)j].done_dev, 0, bytes, rows_ctx->stream));
        }
        BDF_HIP(hipStreamSynchronize(rows_ctx->stream));
    }
    *out = owner.release();
    return BDF_OK;
}

bdf_gibbs::~bdf_gibbs()
{
    if (rows) (void)hipStreamSynchronize(rows->stream);
    if (debug && n_sweeps)
        fprintf(stderr, "[bdf_gibbs] %llu sweeps: host enqueue %.1f us per sweep, host wait for the device %.1f us per sweep\n",
                (unsigned long long)n_sweeps, host_enqueue_us / (double)n_sweeps, host_wait_us / (double)n_sweeps);
    if (gate) { (void)hipStreamSynchronize(gate->stream); delete gate; }
    delete pred;
    delete hyper;
}

extern "C" int bdf_gibbs_destroy(bdf_gibbs *g)
{
    if (g) delete g;
    return BDF_OK;
}

extern "C" int bdf_gibbs_contexts(bdf_gibbs *g, bdf_ctx **hyper, bdf_ctx **pred)
{
    BDF_REQUIRE(g, BDF_ERR_ARG, "bdf_gibbs_contexts: NULL argument");
    if (hyper) *hyper = g->hyper;
    if (pred) *pred = g->pred;
    return BDF_OK;
}

extern "C" int bdf_ctx_stream(const bdf_ctx *ctx, void **stream)
{
    BDF_REQUIRE(ctx && stream, BDF_ERR_ARG, "bdf_ctx_stream: NULL argument");
    *stream = (void *)ctx->stream;
    return BDF_OK;
}

extern "C" int bdf_gibbs_set_test(bdf_gibbs *g, bdf_pairs *pairs, const int32_t *entity_of_mode, double mean_value,
                                  double clamp_lo, double clamp_hi, double class_cut, double *stats_dev)
{
    BDF_REQUIRE(g && pairs && entity_of_mode && stats_dev, BDF_ERR_ARG, "bdf_gibbs_set_test: NULL argument");
    for (int k = 0; k < pairs->n_modes; k++) {
        BDF_REQUIRE(entity_of_mode[k] >= 0 && entity_of_mode[k] < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_set_test: mode %d names entity %d", k, entity_of_mode[k]);
        g->test_entity[k] = entity_of_mode[k];
    }
    g->test = pairs; g->test_mean = mean_value; g->clamp_lo = clamp_lo; g->clamp_hi = clamp_hi; g->class_cut = class_cut;
    g->stats_dev = stats_dev;
    return BDF_OK;
}

extern "C" int bdf_gibbs_set_relations(bdf_gibbs *g, int n_relations, const bdf_gibbs_relation *rels)
{
    BDF_REQUIRE(g && n_relations >= 0 && (n_relations == 0 || rels), BDF_ERR_ARG, "bdf_gibbs_set_relations: bad argument");
    for (int k = 0; k < n_relations; k++) {
        const bdf_gibbs_relation &r = rels[k];
        BDF_REQUIRE(r.rel && (r.alpha_dev || r.probit), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d has no handle or no alpha_dev", k);
        BDF_REQUIRE(!(r.alpha_sample || r.feat) || r.train || (r.dense_R && !r.feat), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d needs its observations as pairs (train)", k);
        BDF_REQUIRE(!r.feat || (r.beta && r.linear), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d has features but no beta / linear buffer", k);
        BDF_REQUIRE(!r.feat_test || r.test_baseline, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d has test features but no baseline buffer", k);
        BDF_REQUIRE(!r.probit || (!r.feat && !r.alpha_sample), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: the probit model takes neither relation features nor a sampled alpha", k);
        BDF_REQUIRE(!r.probit || (r.train && r.linear), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: the probit model needs its observations as pairs (train) and a linear buffer", k);
        BDF_REQUIRE(!r.censor || (!r.probit && !r.feat), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: the censored model takes neither the probit model nor relation features", k);
        BDF_REQUIRE(!r.censor || (r.train && r.linear), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: the censored model needs its observations as pairs (train) and a linear buffer", k);
        BDF_REQUIRE(!r.interval || (!r.probit && !r.censor && !r.feat), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: the interval model takes neither the probit model, censoring flags nor relation features", k);
        BDF_REQUIRE(!r.interval || (r.train && r.linear), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: the interval model needs its observations as pairs (train) and a linear buffer", k);
        BDF_REQUIRE(!r.ordinal || (r.interval && r.ordinal_codes && !g->comm), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: the ordinal model needs the interval model's bounds and the observations' levels, on one rank", k);
        if (r.noise_mode != 0) {
            BDF_REQUIRE(r.noise_mode >= 1 && r.noise_mode <= r.rel->n_modes, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: noise_mode=%d must be 0 (none) or one of the relation's modes 1..%d", k, r.noise_mode, r.rel->n_modes);
            BDF_REQUIRE(r.noise_shape > 0.0 && std::isfinite(r.noise_shape) && r.noise_rate > 0.0 && std::isfinite(r.noise_rate), BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: noise_shape=%g and noise_rate=%g must be positive and finite", k, r.noise_shape, r.noise_rate);
            BDF_REQUIRE(r.train && r.obs_precision && r.noise_tau, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: the per-row noise model (noise_mode) needs its observations as pairs (train), an obs_precision and a noise_tau buffer", k);
            BDF_REQUIRE(!r.probit && !r.censor && !r.interval && !r.ordinal && r.robust_nu == 0.0 && !r.pg_model && !(r.bg_weight > 0.0) && !r.feat && !g->comm, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: the per-row noise model (noise_mode) takes neither the probit, censored, interval, ordinal, robust or a Polya-Gamma model, a background, relation features nor a communicator", k);
        }
        if (r.n_bias != 0) {
            BDF_REQUIRE(r.n_bias >= 1 && r.n_bias <= r.rel->n_modes, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: n_bias=%d must be 0 (none) or at most the relation's %d modes", k, r.n_bias, r.rel->n_modes);
            for (int t = 0; t < r.n_bias; t++) {
                const bdf_bias_term &b = r.bias[t];
                BDF_REQUIRE(b.mode >= 0 && b.mode < r.rel->n_modes, BDF_ERR_ARG,
                            "bdf_gibbs_set_relations: relation %d: bias term %d: mode=%d must be in 0..%d", k, t, b.mode, r.rel->n_modes - 1);
                for (int u = 0; u < t; u++)
                    BDF_REQUIRE(r.bias[u].mode != b.mode, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: bias mode %d is listed twice", k, b.mode);
                BDF_REQUIRE(b.shape > 0.0 && std::isfinite(b.shape) && b.rate > 0.0 && std::isfinite(b.rate), BDF_ERR_ARG,
                            "bdf_gibbs_set_relations: relation %d: bias term %d: shape=%g and rate=%g must be positive and finite", k, t, b.shape, b.rate);
                BDF_REQUIRE(b.bias && b.lambda, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: bias term %d has no bias / lambda buffer", k, t);
            }
            BDF_REQUIRE(r.train && r.linear && r.bias_resid, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: biases (n_bias) need the observations as pairs (train), a linear and a bias_resid buffer", k);
            BDF_REQUIRE(!r.probit && !r.censor && !r.interval && !r.ordinal && !r.obs_precision && !r.pg_model && r.noise_mode == 0 && !(r.bg_weight > 0.0) &&
                        !r.dense_R && !r.feat && !g->comm, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: biases (n_bias) take Gaussian noise of one precision: neither another noise model, observation weights, a background, a dense relation, relation features nor a communicator", k);
            BDF_REQUIRE((r.bias_test != nullptr) == (r.test_baseline != nullptr), BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: biases take bias_test and test_baseline together", k);
            BDF_REQUIRE(!r.bias_test || r.bias_test->n_modes == r.rel->n_modes, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: bias_test has %d modes, the relation %d", k, r.bias_test ? r.bias_test->n_modes : 0, r.rel->n_modes);
        } else
            BDF_REQUIRE(!r.bias_test && !r.bias_resid, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: bias_test / bias_resid without n_bias", k);
        BDF_REQUIRE(r.robust_nu == 0.0 || (r.robust_nu >= 1.0 && std::isfinite(r.robust_nu)), BDF_ERR_ARG,
                    "bdf_gibbs_set_relations: relation %d: robust_nu=%g must be 0 (off) or at least 1 and finite", k, r.robust_nu);
        BDF_REQUIRE(!(r.robust_nu > 0.0) || (r.train && r.obs_precision), BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: the robust model needs its observations as pairs (train) and an obs_precision buffer", k);
        BDF_REQUIRE(!r.obs_precision || (!r.probit && !r.censor && !r.interval && !r.ordinal && !r.feat), BDF_ERR_ARG,
                    "bdf_gibbs_set_relations: relation %d: observation weights take neither the probit, censored, interval or ordinal model nor relation features", k);
        BDF_REQUIRE(!r.obs_precision || !g->comm, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: observation weights need one rank", k);
        BDF_REQUIRE(r.pg_model >= 0 && r.pg_model <= 2, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: pg_model=%d must be 0 (none), 1 (logit) or 2 (counts)", k, r.pg_model);
        BDF_REQUIRE(!r.pg_model || (r.train && r.linear && r.obs_precision), BDF_ERR_ARG,
                    "bdf_gibbs_set_relations: relation %d: a Polya-Gamma model needs its observations as pairs (train), a linear and an obs_precision buffer", k);
        BDF_REQUIRE(!r.pg_model || (!r.probit && !r.censor && !r.interval && !r.ordinal && r.robust_nu == 0.0 && !r.feat && !r.alpha_sample && !g->comm), BDF_ERR_ARG,
                    "bdf_gibbs_set_relations: relation %d: a Polya-Gamma model takes neither the probit, censored, interval, ordinal or robust model, relation features, a sampled alpha nor a communicator", k);
        BDF_REQUIRE(r.pg_model != 2 || (r.pg_r >= 1.0 && r.pg_r <= 2147483648.0 && r.pg_r == std::floor(r.pg_r)), BDF_ERR_ARG,
                    "bdf_gibbs_set_relations: relation %d: pg_r=%g must be an integer, at least 1", k, r.pg_r);
        for (int m = 0; m < r.rel->n_modes; m++)
            BDF_REQUIRE(r.entity_of_mode[m] >= 0 && r.entity_of_mode[m] < (int)g->ent.size(), BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d mode %d names entity %d", k, m, r.entity_of_mode[m]);
        BDF_REQUIRE(r.bg_weight >= 0.0 && r.bg_weight <= 1.0 && std::isfinite(r.bg_value), BDF_ERR_ARG,
                    "bdf_gibbs_set_relations: relation %d: bg_weight=%g must be 0 (none) or in (0, 1] and bg_value=%g finite", k, r.bg_weight, r.bg_value);
        // a folded relation: its unlisted cells reach the rows through the prior (a background; a dense relation,
        // section 25).  What both need is stated once; what differs follows.
        const bool bg = r.bg_weight > 0.0, dense = r.dense_R != nullptr;
        if (bg || dense) {
            const char *what = dense ? "a dense relation" : "a background";
            BDF_REQUIRE(r.rel->n_modes == 2 && (dense ? r.dense_sums : r.bg_sums), BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: %s takes a two-mode relation and the %s buffer", k, what, dense ? "dense_sums" : "bg_sums");
            BDF_REQUIRE(!r.probit && !r.censor && !r.interval && !r.ordinal && r.robust_nu == 0.0 && !r.pg_model && !r.feat && !g->comm, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: %s takes neither the probit, censored, interval, ordinal, robust or a Polya-Gamma model, relation features nor a communicator", k, what);
            for (int m = 0; m < 2; m++) {
                const bdf_gibbs_entity &e = g->ent[(size_t)r.entity_of_mode[m]].d;
                BDF_REQUIRE(e.bg_Lambda && e.bg_mu && e.bg_alpha_rows && (dense || e.bg_pack) && !(dense && e.spike) && !e.nonneg, BDF_ERR_ARG,
                            "bdf_gibbs_set_relations: relation %d is %s but entity %d has a NULL bg_Lambda / bg_mu / bg_alpha_rows%s", k, what, r.entity_of_mode[m],
                            e.nonneg ? ", or the non-negative prior" : (dense ? ", or the spike-and-slab prior" : " / bg_pack"));
            }
        }
        BDF_REQUIRE(!bg || !r.obs_precision || (r.linear && r.bg_weights), BDF_ERR_ARG,
                    "bdf_gibbs_set_relations: relation %d: a background with observation weights needs the linear and the bg_weights buffer", k);
        if (dense) {
            BDF_REQUIRE(r.dense_C, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: a dense relation takes the dense_C buffer", k);
            BDF_REQUIRE(!r.obs_precision && r.noise_mode == 0 && !bg, BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: a dense relation takes no observation weights, per-row noise model nor background", k);
            BDF_REQUIRE(r.rel->nnz == 0, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d is dense: `rel` must list no cell (its values live in dense_R)", k);
            BDF_REQUIRE(!r.dense_holes || (r.dense_stats && r.dense_holes->n_modes == 2), BDF_ERR_ARG,
                        "bdf_gibbs_set_relations: relation %d: dense_holes needs two modes and the dense_stats buffer", k);
            BDF_REQUIRE(std::isfinite(r.dense_sum_r2) && r.dense_sum_r2 >= 0.0, BDF_ERR_ARG, "bdf_gibbs_set_relations: relation %d: dense_sum_r2=%g", k, r.dense_sum_r2);
        }
    }
    g->rels.assign(rels, rels + n_relations);
    if (n_relations > 0 && !g->rel_sse) { if (int rca = g->rel_sse.alloc(8)) return rca; }
    return BDF_OK;
}

namespace {
// the registered relation of a term (by its bdf_rel), or NULL
const bdf_gibbs_relation *relation_of(const bdf_gibbs *g, const bdf_rel *rel)
{
    for (const auto &r : g->rels)
        if (r.rel == rel) return &r;
    return nullptr;
}

// does the relation draw a latent z per observation into its linear buffer?  (bdf_gibbs_set_relations admits one of the four; the
// Polya-Gamma models write the pseudo-observation there, and omega beside it.)
inline bool draws_latent(const bdf_gibbs_relation &r) { return r.probit || r.censor || r.interval || r.pg_model; }

// does update_relations() enqueue anything for the relation?  (Known weights alone do not: the rows just read them.)
inline bool has_model(const bdf_gibbs_relation &r)
{
    return r.alpha_sample || r.feat || draws_latent(r) || r.robust_nu > 0.0 || r.noise_mode != 0 || (r.dense_R && r.dense_holes) || r.n_bias != 0;
}

// out[m] = the current sample of the entity that is mode m
void current_factors(const bdf_gibbs *g, const int32_t *entity_of_mode, int n_modes, const double **out)
{
    for (int m = 0; m < n_modes; m++) {
        const auto &O = g->ent[(size_t)entity_of_mode[m]];
        out[m] = O.d.sample[O.cur];
    }
}

// the registered relation of entity e's term t when the term is folded into the prior -- the relation has background cells
// (bdf_gibbs_relation.bg_weight) or is dense (dense_R) -- or NULL
const bdf_gibbs_relation *folded_of(const bdf_gibbs *g, const bdf_gibbs_entity &e, int t)
{
    const bdf_gibbs_relation *gr = relation_of(g, e.terms[t].rel);
    return (gr && (gr->bg_weight > 0.0 || gr->dense_R)) ? gr : nullptr;
}

// a folded relation's sums: per mode, the sum of the entity's rows (D) and their Gram matrix (D x D)
inline double *fold_sums(const bdf_gibbs_relation &r) { return r.dense_R ? r.dense_sums : r.bg_sums; }

// is a term of entity e folded into its prior?  Such an entity's prior is made on the row stream.
bool folds_prior(const bdf_gibbs *g, const bdf_gibbs_entity &e)
{
    for (int t = 0; t < e.n_terms; t++)
        if (folded_of(g, e, t)) return true;
    return false;
}

// bdf_hyper_sums of both entities' current rows into a folded relation's sums, for its sum of squares over all cells
int both_sums(bdf_gibbs *g, const bdf_gibbs_relation &r, const double *const *fac)
{
    const int D = g->D;
    const size_t pk = (size_t)D + (size_t)D * D;
    for (int m = 0; m < 2; m++) {
        double *s = fold_sums(r) + m * pk;
        int rc = bdf_hyper_sums(g->rows, D, g->ent[(size_t)r.entity_of_mode[m]].d.N, fac[m], nullptr, s, s + D);
        if (rc) return rc;
    }
    return BDF_OK;
}

// The prior that entity E's rows are sampled with: the hyperprior's draw as it stands -- or, when terms of the entity are folded
// (background cells; dense relations, section 25), that draw with their Gram terms folded in.  Per folded
// term, in the order of the entity's terms: the sum and the Gram matrix of the OTHER entity's current rows into the relation's own
// buffers (bdf_hyper_sums on the row stream) and, for a dense term, its rows of R V (R' U) from the same rows.  Then one fold into
// the entity's (bg_mu, bg_Lambda) and bg_alpha_rows, which fill_terms hands the terms with unit weights: bdf_dense_prior when a
// dense term is among them (the means are then one per row), else bdf_background_prior, which also leaves bg_pack for a shared
// mean.  pack_valid: the entity's latest draw has left its prior pack.
int row_prior(bdf_gibbs *g, const bdf_gibbs::Ent &E, bool pack_valid, const double **mu, int *mu_is_matrix, const double **Lambda, const double **pack)
{
    const bdf_gibbs_entity &e = E.d;
    const int D = g->D;
    *mu = e.feat ? e.mu_matrix : e.mu;
    *mu_is_matrix = e.feat ? 1 : 0;
    *Lambda = e.Lambda;
    *pack = (pack_valid && !e.feat) ? e.prior_pack : nullptr;
    bdf_dense_term dt[BDF_MAX_TERMS];
    int n = 0, n_dense = 0, rc;
    for (int t = 0; t < e.n_terms; t++) {
        const bdf_gibbs_relation *gr = folded_of(g, e, t);
        if (!gr) continue;
        const int mode = e.terms[t].mode, other = 1 - mode;
        const auto &O = g->ent[(size_t)e.terms[t].entity_of_mode[other]];
        double *s = fold_sums(*gr) + (size_t)other * ((size_t)D + (size_t)D * D);
        if ((rc = bdf_hyper_sums(g->rows, D, O.d.N, O.d.sample[O.cur], nullptr, s, s + D))) return rc;
        dt[n] = {};
        dt[n].gram = s + D; dt[n].alpha_dev = gr->alpha_dev;
        if (gr->dense_R) {
            double *C = gr->dense_C + (mode == 0 ? (size_t)0 : (size_t)gr->rel->dims[0] * D);
            if ((rc = bdf_dense_product(g->rows, gr->dense_R, gr->rel->dims[0], gr->rel->dims[1], D, O.d.sample[O.cur], mode, C))) return rc;
            dt[n].C = C; dt[n].weight = 1.0;
            n_dense++;
        } else {
            dt[n].sum = s; dt[n].weight = gr->bg_weight; dt[n].resid = gr->bg_value - gr->mean_value;
        }
        n++;
    }
    if (n == 0) return BDF_OK;
    if (n_dense > 0) {
        if ((rc = bdf_dense_prior(g->rows, D, e.N, n, dt, *mu, *mu_is_matrix, e.Lambda, e.bg_Lambda, e.bg_mu, e.bg_alpha_rows))) return rc;
        *mu = e.bg_mu; *mu_is_matrix = 1; *Lambda = e.bg_Lambda; *pack = nullptr;
        return BDF_OK;
    }
    bdf_background_term bg[BDF_MAX_TERMS];             // (background terms alone: the entry point with the pack, and its own term type)
    for (int k = 0; k < n; k++) bg[k] = {dt[k].sum, dt[k].gram, 0.0, dt[k].alpha_dev, dt[k].weight, dt[k].resid};
    if ((rc = bdf_background_prior(g->rows, D, e.N, n, bg, *mu, *mu_is_matrix, e.Lambda, e.bg_Lambda, e.bg_mu, e.feat ? nullptr : e.bg_pack, e.bg_alpha_rows)))
        return rc;
    *mu = e.bg_mu; *Lambda = e.bg_Lambda; *pack = e.feat ? nullptr : e.bg_pack;
    return BDF_OK;
}

// the terms of entity e's row launch: a term of a registered relation takes the model's alpha_dev, linear_values and
// obs_precision
void fill_terms(const bdf_gibbs *g, const bdf_gibbs_entity &e, bdf_term *terms)
{
    int n_folded = 0;                                        // (the folded terms before this one: its place in bg_alpha_rows)
    for (int t = 0; t < e.n_terms; t++) {
        terms[t].rel = e.terms[t].rel; terms[t].mode = e.terms[t].mode; terms[t]._pad = 0;
        terms[t].alpha = e.terms[t].alpha; terms[t].mean_value = e.terms[t].mean_value; terms[t].linear_values = nullptr;
        terms[t].alpha_dev = nullptr; terms[t].obs_precision = nullptr;
        if (const bdf_gibbs_relation *gr = relation_of(g, e.terms[t].rel)) {        // a relation with a model of its own
            terms[t].alpha_dev = gr->probit ? nullptr : gr->alpha_dev;
            terms[t].linear_values = (gr->feat || draws_latent(*gr) || gr->n_bias != 0) ? gr->linear : nullptr;      // (biases: mean + the cell's biases)
            if (gr->probit) terms[t].alpha = 1.0;            // the latent's variance
            terms[t].obs_precision = gr->obs_precision;      // known weights, or the omega of the robust draw
            if (gr->bg_weight > 0.0) {
                // background cells: the listed ones count with omega_k - c0 and the pseudo-residual through `linear` (both constant),
                // or -- unit weights, the unweighted kernels -- with alpha (1 - c0), which row_prior's fold has left on the device
                if (gr->obs_precision) terms[t].linear_values = gr->linear;
                else terms[t].alpha_dev = e.bg_alpha_rows + n_folded;
            }
        }
        if (folded_of(g, e, t)) n_folded++;                  // (a dense term is folded too, and shares bg_alpha_rows; none of its cells is listed)
        for (int k = 0; k < BDF_MAX_MODES; k++) terms[t].factors[k] = nullptr;
        current_factors(g, e.terms[t].entity_of_mode, e.terms[t].rel->n_modes, terms[t].factors);
    }
}

// macau.jl:83-92 on the row stream, before the entities' rows
int update_relations(bdf_gibbs *g)
{
    bdf_ctx *R = g->rows;
    const int D = g->D;
    int rc;
    for (const auto &r : g->rels) {
        if (!has_model(r)) continue;
        const double *fac[BDF_MAX_MODES];
        current_factors(g, r.entity_of_mode, r.rel->n_modes, fac);
        // robust: omega of every observation given the rows and the PREVIOUS iteration's alpha, before sample_alpha -- which then takes
        // sum omega e^2 in place of the sum of squares (alpha's exact conditional); the rows then read obs_precision
        if (r.robust_nu > 0.0 && (rc = bdf_robust_draw(R, r.train, D, fac, r.mean_value, 0.0, r.alpha_dev, r.robust_nu, r.rel_tag, r.obs_precision,
                                                      r.alpha_sample ? g->rel_sse + 1 : nullptr)))
            return rc;
        // a noise precision per row of one entity: tau of every row of that entity at the same place and in the same manner; it leaves
        // sum tau_j S_j for sample_alpha and tau of every observation's row in obs_precision
        if (r.noise_mode != 0 && (rc = bdf_entity_noise_draw(R, r.rel, r.noise_mode - 1, r.train, D, fac, r.mean_value, 0.0, r.alpha_dev, r.noise_shape,
                                                             r.noise_rate, r.rel_tag, r.noise_tau, r.obs_precision, r.alpha_sample ? g->rel_sse + 1 : nullptr)))
            return rc;
        // biases: every biased mode's rows and precision given the factors and the PREVIOUS iteration's alpha, before sample_alpha --
        // whose sum of squares then sees the new biases through the training pairs' baseline (`linear`); the rows then read `linear`
        if (r.n_bias != 0) {
            if ((rc = bdf_bias_draw(R, r.rel, r.train, D, fac, r.mean_value, 0.0, r.alpha_dev, r.rel_tag, r.n_bias, r.bias, r.bias_resid, r.linear)))
                return rc;
            if (r.bias_test) {
                // the test pairs' baseline is read by the prediction stream: its updates so far must have completed
                for (int k = 0; k < 3; k++)
                    if (g->n_pred > (uint64_t)k) BDF_HIP(hipStreamWaitEvent(R->stream, g->ev_pred[(g->n_pred - 1 - (uint64_t)k) % 3], 0));
                if ((rc = bdf_bias_baseline(R, r.bias_test, r.n_bias, r.bias, r.mean_value, r.test_baseline))) return rc;
            }
        }
        // dense: the holes given the rows and the PREVIOUS iteration's alpha, into dense_R, before sample_alpha -- whose sum then runs
        // over all N M cells
        if (r.dense_R && r.dense_holes && (rc = bdf_dense_impute(R, r.dense_holes, D, fac, 0.0, r.alpha_dev, r.rel_tag, r.dense_R, r.rel->dims[0],
                                                               r.rel->dims[1], r.dense_stats)))
            return rc;
        if (r.alpha_sample) {
            // err' err over this rank's block (the pairs carry linear_values as their baseline), summed over the ranks; known weights:
            // sum w e^2 (the robust draw above has left its own)
            int64_t n = r.nnz;
            if (r.bg_weight > 0.0) {
                // background cells: the sum of c e^2 over ALL N M cells from the listed ones, the two entities' sums and Gram matrices
                const double *s = fold_sums(r), *s1 = s + D + (size_t)D * D;
                if ((rc = both_sums(g, r, fac))) return rc;
                rc = bdf_background_sse(R, r.train, D, fac, r.mean_value, r.bg_weights, r.bg_value, r.bg_weight, s, s + D, s1, s1 + D, r.rel->dims[0],
                                        r.rel->dims[1], g->rel_sse + 1);
                n = r.rel->dims[0] * r.rel->dims[1];
            } else if (r.dense_R) {
                // dense: the closed form over all N M cells from C = R V and the two entities' Gram matrices
                const double *s = fold_sums(r), *s1 = s + D + (size_t)D * D;
                if ((rc = both_sums(g, r, fac))) return rc;
                if ((rc = bdf_dense_product(R, r.dense_R, r.rel->dims[0], r.rel->dims[1], D, fac[1], 0, r.dense_C))) return rc;
                rc = bdf_dense_sse(R, D, r.rel->dims[0], fac[0], r.dense_C, s + D, s1 + D, r.dense_sum_r2, r.dense_holes ? r.dense_stats : nullptr, g->rel_sse + 1);
                n = r.rel->dims[0] * r.rel->dims[1];
            } else if (r.obs_precision) rc = (r.robust_nu > 0.0 || r.noise_mode != 0) ? BDF_OK : bdf_pairs_weighted_sse(R, r.train, D, fac, r.mean_value, r.obs_precision, g->rel_sse + 1);
            else rc = bdf_predict_sse(R, r.train, D, fac, r.mean_value, nullptr, g->rel_sse);
            if (rc) return rc;
            if (g->comm && (rc = bdf_sum_ranks(R, g->comm, g->rel_sse + 1, 1))) return rc;
            if ((rc = bdf_sample_alpha(R, r.alpha_lambda0, r.alpha_nu0, n, g->rel_sse + 1, r.rel_tag, r.alpha_dev))) return rc;
        }
        // probit: the latent z of every observation given the rows; the rows then see linear = y - z with alpha = 1
        if (r.probit && (rc = bdf_probit_draw(R, r.train, D, fac, r.mean_value, r.rel_tag, r.linear + r.first_obs, nullptr))) return rc;
        // Polya-Gamma (logit, counts): omega of every observation given the rows, at the same place; the rows then see the
        // pseudo-observation through linear and its precision through obs_precision, with alpha = 1
        if (r.pg_model && (rc = bdf_pg_draw(R, r.train, D, fac, r.mean_value, r.pg_model, r.pg_r, r.rel_tag, r.obs_precision, r.linear + r.first_obs)))
            return rc;
        // censored: the latent z of every flagged observation given the rows and the alpha just drawn (the sum of squares above was
        // that of the previous z: the pairs carry linear as their baseline); the rows then see linear = mean + y - z with alpha_dev
        if (r.censor && (rc = bdf_censored_draw(R, r.train, r.censor, D, fac, r.mean_value, 0.0, r.alpha_dev, r.rel_tag, r.linear + r.first_obs, nullptr)))
            return rc;
        // ordinal: one Metropolis step on the edges given the rows and the alpha just drawn, z integrated out; it rewrites the bounds
        // that the interval draw below reads (the step adapts while the object's own count is within its burn-in)
        if (r.ordinal && (rc = bdf_ordinal_step(R, r.ordinal, r.train, r.ordinal_codes, D, fac, r.mean_value, 0.0, r.alpha_dev, r.rel_tag, -1,
                                                const_cast<double *>(r.interval))))
            return rc;
        // interval-censored: the same draw at the same place, between the two bounds of every bounded observation
        if (r.interval && (rc = bdf_interval_draw(R, r.train, r.interval, D, fac, r.mean_value, 0.0, r.alpha_dev, r.rel_tag, r.linear + r.first_obs, nullptr)))
            return rc;
        if (r.feat) {
            if ((rc = bdf_sample_beta_rel_impl(R, g->comm, r.feat, r.train, r.first_obs, D, fac, r.mean_value, 1.0, r.alpha_dev, r.lambda_beta,
                                               r.rel_tag, r.beta, r.linear + r.first_obs, nullptr)))
                return rc;
            if (g->comm) {          // every rank's row kernels read linear_values of their own rows' observations
                if ((rc = bdf_allgather_block(R, g->comm, r.linear, sizeof(double) * (size_t)r.obs_block)) || (rc = bdf_allgather_join(R, g->comm))) return rc;
            }
            if (r.feat_test) {
                // the test pairs' baseline is read by the prediction stream: its updates so far must have completed
                for (int k = 0; k < 3; k++)
                    if (g->n_pred > (uint64_t)k) BDF_HIP(hipStreamWaitEvent(R->stream, g->ev_pred[(g->n_pred - 1 - (uint64_t)k) % 3], 0));
                if ((rc = bdf_feat_linear(R, r.feat_test, r.beta, r.mean_value, r.test_baseline))) return rc;
            }
        }
    }
    return BDF_OK;
}
}  // namespace

extern "C" int bdf_gibbs_set_comm(bdf_gibbs *g, bdf_comm *comm)
{
    BDF_REQUIRE(g, BDF_ERR_ARG, "bdf_gibbs_set_comm: NULL argument");
    g->comm = comm;
    bdf_gather_image_invalidate(g->rows, nullptr);    // (the exchange writes the samples: with a communicator no launch vouches for an image)
    return BDF_OK;
}

namespace {
// the hyperprior's degrees of freedom: nu0 (+ numF with side information and full_lambda_u, macau.jl:124-129)
double hyper_nu(const bdf_gibbs_entity &e) { return e.nu0 + ((e.feat && e.full_lambda_u) ? (double)e.feat->n : 0.0); }
// a prior of its own in place of the Normal-Wishart one (spike-and-slab; non-negative, section 26): no (mu, Lambda)
// draw and none of its hand-overs -- the entity's rows wait for the event of its hyper step
bool own_prior(const bdf_gibbs_entity &e) { return e.spike || e.nonneg; }

// What bdf_gibbs_sweep hangs on an entity's row launch.  All empty (the step entry points, bdf_gibbs_rows_only): plain stream order --
// no events, no polling, no done counter, and the context's timing fields and span slot are the caller's.
struct RowsExtras {
    const uint32_t *poll; uint32_t poll_want;      // the launch's waves poll this word for poll_want where they first need the prior
    uint32_t *counter;                   // the waves add to these 64 words when their rows are in memory (SampleArgs::done)
    hipEvent_t start, stop;              // on the first chunk's dispatch | on the last chunk's
    unsigned long long *span;            // SampleArgs::span
    hipEvent_t joined;                   // a communicator: recorded behind the join of the last chunk's exchange
};

// The row launch of entity E, the only one: the prior (row_prior), the terms (fill_terms), the kernel variant chunk by chunk and, with
// a communicator and `exchange`, every chunk's rows to the other ranks; the entity's next buffer then becomes the current one.
// *by_counter (nullable): the launch hands over through x.counter (a launch that takes another kernel than k_rows_col reports
// rows_done_added < 0: the caller uses an event after all); E.done_target then counts its waves in.
int launch_rows(bdf_gibbs *g, bdf_gibbs::Ent &E, bool pack_valid, bool exchange, const RowsExtras &x, bool *by_counter)
{
    bdf_ctx *R = g->rows;
    const bdf_gibbs_entity &e = E.d;
    int rc;
    // the prior of this launch: the draw's (mu, Lambda) and pack, or -- background cells -- those with the Gram terms folded in
    const double *mu = nullptr, *Lambda = nullptr, *pack = nullptr;
    int is_matrix = 0;
    if (!own_prior(e) && (rc = row_prior(g, E, pack_valid, &mu, &is_matrix, &Lambda, &pack))) return rc;
    bdf_term terms[BDF_MAX_TERMS];
    fill_terms(g, e, terms);
    const int nxt = (E.cur + 1) % 3, nch = e.terms[0].rel->chunks;     // 1 unless the relations were created with a layout
    exchange = exchange && g->comm;
    if (by_counter) *by_counter = false;
    for (int c = 0; c < nch; c++) {
        if (x.start || x.stop) { R->time_start = (c == 0) ? x.start : nullptr; R->time_stop = (c == nch - 1) ? x.stop : nullptr; }
        if (x.span) R->rows_span = x.span;
        if (x.poll) { R->rows_ready = x.poll; R->rows_ready_want = x.poll_want; }
        if (x.counter) R->rows_done = x.counter;
        R->gimg_trust = !g->comm;         // (the chain's own buffers: sample_written() hears of every other writer)
        if ((rc = e.spike ? bdf_sample_rows_spike(R, g->D, e.N, e.n_terms, terms, e.spike_state, e.sample[E.cur], e.tag, c, nch, e.sample[nxt])
                 : e.nonneg ? bdf_sample_rows_nonneg(R, g->D, e.N, e.n_terms, terms, e.nonneg_tau, e.sample[E.cur], e.tag, c, nch, e.sample[nxt])
                          : bdf_sample_rows(R, g->D, e.N, e.n_terms, terms, mu, is_matrix, Lambda, e.tag, c, nch, e.sample[nxt], pack)))
            return rc;
        if (x.counter && R->rows_done_added >= 0) { if (by_counter) *by_counter = true; E.done_target += (uint32_t)R->rows_done_added; }
        if (exchange && (rc = bdf_allgather_rows(R, g->comm, g->D, e.N, e.sample[nxt], c, nch))) return rc;
    }
    if (exchange) {
        if ((rc = bdf_allgather_join(R, g->comm))) return rc;           // the row stream continues after the last chunk's exchange
        if (x.joined) BDF_HIP(hipEventRecord(x.joined, R->stream));
    }
    E.cur = nxt;
    return BDF_OK;
}

// What only bdf_gibbs_sweep sets on the hyperprior context before the calls of hyper_step.  All empty (bdf_gibbs_step_hyper): the
// unfused sums, then the draw kernel, in plain stream order.
struct HyperExtras {
    bool fuse;                           // small entities: the sums and the draw in one launch (k_hyper_chain)
    double *chain_draws;                 // ... which also makes the entity's random part into this buffer
    hipEvent_t stop;                     // on the draw's dispatch
    uint32_t *ready; uint32_t ready_value;         // the draw sets this word to ready_value once its pack is written
    const uint32_t *wait; uint32_t wait_target;    // the chain's partial-sum workgroups poll the sum of these 64 words for wait_target
};

// The hyperprior step of entity E on context H from its current rows, the only one: the spike-and-slab prior's hyper step -- or the
// feature terms, the sums (one rank or several) and the Normal-Wishart draw.  draws: the data-independent part made ahead
// (bdf_hyper_draws into e.draws), or NULL: the draw makes its own normals.  It touches no event and none of E's bookkeeping.
int hyper_step(bdf_gibbs *g, const bdf_gibbs::Ent &E, bdf_ctx *H, const double *draws, const HyperExtras &x)
{
    const bdf_gibbs_entity &e = E.d;
    const int D = g->D;
    int rc;
    // the spike-and-slab prior's hyper step in place of the sums and the Normal-Wishart draw
    if (e.spike) return bdf_spike_hyper(H, D, e.n_real, e.sample[E.cur], e.spike_a, e.spike_b, e.spike_shape, e.spike_rate, e.tag, e.spike_state);
    // ... and the non-negative prior's
    if (e.nonneg) return bdf_nonneg_hyper(H, D, e.n_real, e.sample[E.cur], e.nonneg_shape, e.nonneg_rate, e.tag, e.nonneg_tau);
    if (x.wait) { H->hyper_wait = x.wait; H->hyper_wait_target = x.wait_target; }
    if (x.fuse) H->hyper_fuse = true;
    // side information: U = sample - uhat, T^-1 = WI + beta' beta lambda_beta with the beta of the previous iteration
    const double *Tinv = e.WI;
    if (e.feat && e.full_lambda_u) {
        if ((rc = bdf_hyper_feature_terms(H, D, e.feat->n, e.beta, e.WI, e.lambda_beta, e.Tinv))) return rc;
        Tinv = e.Tinv;
    }
    // (several ranks: every rank sums its own rows, the D + D^2 partial sums are added over the ranks in rank order)
    if ((rc = g->comm ? bdf_hyper_sums_ranks(H, g->comm, D, e.N, e.terms[0].rel->chunks, e.sample[E.cur], e.feat ? e.uhat : nullptr, e.sumU, e.UUt)
                      : bdf_hyper_sums(H, D, e.N, e.sample[E.cur], e.feat ? e.uhat : nullptr, e.sumU, e.UUt)))
        return rc;
    if (x.chain_draws) H->hyper_chain_draws = x.chain_draws;
    if (x.stop) H->time_h_stop = x.stop;
    if (x.ready) { H->hyper_ready = x.ready; H->hyper_ready_value = x.ready_value; }
    return bdf_hyper_sample(H, D, e.n_real, e.sumU, e.UUt, e.mu0, e.b0, Tinv, hyper_nu(e), e.tag, e.mu, e.Lambda, e.params, e.prior_pack, draws);
}

// side information: beta of entity E from its current rows and (mu, Lambda), on the row stream (macau.jl:138-140)
// (several ranks: the conjugate-gradient columns are shared out over them and all-gathered, parallel_matrix.jl:488-507)
int beta_step(bdf_gibbs *g, const bdf_gibbs::Ent &E)
{
    const bdf_gibbs_entity &e = E.d;
    return bdf_sample_beta_ranks(g->rows, g->comm, e.feat, g->D, e.sample[E.cur], e.mu, e.Lambda, e.lambda_beta, e.use_ff, e.tol, 0,
                                 e.sample_lambda_beta, e.lb_nu, e.lb_mu, e.tag, e.beta, nullptr, e.cg_iters);
}
}  // namespace

// measurement: the rows of one entity and nothing else -- the launch bdf_gibbs_sweep makes for it (same kernel variant, same
// inputs), without the hyperprior update, the exchange or the prediction update.  The chain's state is not kept consistent.
extern "C" int bdf_gibbs_rows_only(bdf_gibbs *g, int entity, uint32_t sweep)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_rows_only: bad argument");
    g->rows->sweep_host = sweep;
    auto &E = g->ent[(size_t)entity];
    return launch_rows(g, E, E.hyper_recorded, false, {}, nullptr);
}

// The iteration piece by piece, for a host that keeps the schedule itself (and the prediction update through the entry points of
// bdf.h): what runs before the rows, one entity's rows, the data-independent part of its hyperprior draw, its hyperprior step, its
// beta.  The pieces bdf_gibbs_sweep composes, in plain stream order under the iteration number the caller has set on the contexts
// (bdf_ctx_set_sweep): no events, and nothing of the object's bookkeeping changes but the rows' buffer rotation.  Relations, rows and
// beta on the row stream; draws and hyperprior on the hyperprior context's (BDF_NO_OVERLAP: on the row context too).
extern "C" int bdf_gibbs_step_relations(bdf_gibbs *g)
{
    BDF_REQUIRE(g, BDF_ERR_ARG, "bdf_gibbs_step_relations: NULL argument");
    return g->rels.empty() ? BDF_OK : update_relations(g);
}

extern "C" int bdf_gibbs_step_rows(bdf_gibbs *g, int entity, int pack_valid)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_step_rows: bad argument");
    auto &E = g->ent[(size_t)entity];
    const bdf_gibbs_entity &e = E.d;
    int rc;
    // side information: uhat = (F beta)' with the beta of the previous iteration, per-row prior means mu + uhat (macau.jl:103-104)
    if (e.feat && (rc = bdf_uhat(g->rows, e.feat, g->D, e.beta, e.mu, e.uhat, e.mu_matrix))) return rc;
    return launch_rows(g, E, pack_valid != 0, true, {}, nullptr);
}

extern "C" int bdf_gibbs_step_draws(bdf_gibbs *g, int entity)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_step_draws: bad argument");
    const bdf_gibbs_entity &e = g->ent[(size_t)entity].d;
    // (the spike-and-slab and the non-negative prior's hyper steps draw from the rows' sums: nothing to prepare)
    return own_prior(e) ? BDF_OK : bdf_hyper_draws(g->step_hyper, g->D, e.n_real, hyper_nu(e), e.tag, e.draws);
}

extern "C" int bdf_gibbs_step_hyper(bdf_gibbs *g, int entity, int draws_prepared)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_step_hyper: bad argument");
    const auto &E = g->ent[(size_t)entity];
    return hyper_step(g, E, g->step_hyper, draws_prepared ? E.d.draws : nullptr, {});
}

extern "C" int bdf_gibbs_step_beta(bdf_gibbs *g, int entity)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_step_beta: bad argument");
    const auto &E = g->ent[(size_t)entity];
    return E.d.feat ? beta_step(g, E) : BDF_OK;
}

// parity hooks: the terms and the prior that the entity's next row launch would take
extern "C" int bdf_gibbs_terms(bdf_gibbs *g, int entity, bdf_term *out)
{
    BDF_REQUIRE(g && out && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_terms: bad argument");
    fill_terms(g, g->ent[(size_t)entity].d, out);
    return BDF_OK;
}

extern "C" int bdf_gibbs_row_prior(bdf_gibbs *g, int entity, int pack_valid, const double **mu, int *mu_is_matrix, const double **Lambda,
                                   const double **pack)
{
    BDF_REQUIRE(g && mu && mu_is_matrix && Lambda && pack && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_row_prior: bad argument");
    return row_prior(g, g->ent[(size_t)entity], pack_valid != 0, mu, mu_is_matrix, Lambda, pack);
}

// set-up: bring the device to its working state (clocks, power gating: an iteration right after idle time runs ~10 % slower than
// the same iteration 30 ms into sustained work, and what ran before matters as much as how long: DESIGN.md section 6) with FULL
// iterations whose results are discarded -- rows of every entity, exchanges, hyperprior chains, beta, the relation models, the
// prediction kernel without running state -- under iteration numbers no real iteration uses.  The chain's state (every entity's
// current sample, (mu, Lambda), sums, prior pack, draws, beta, uhat, per-row prior means, lambda_beta, the relations' alpha, beta
// and linear_values, the prediction statistics, the "a draw / beta of an earlier iteration exists" flags) is saved first and put
// back bit for bit afterwards; the buffers have rotated (bdf_gibbs_current).  One rank: iterations for `milliseconds`.  Several
// ranks: every rank must make the same number of exchanges -- the first batch of eight is timed, every rank derives a count from
// its own time, and the ranks agree on the mean of the counts (bdf_sum_ranks).
extern "C" int bdf_gibbs_warm_device(bdf_gibbs *g, double milliseconds)
{
    BDF_REQUIRE(g && milliseconds >= 0.0 && milliseconds <= 10000.0, BDF_ERR_ARG, "bdf_gibbs_warm_device: bad argument");
    if (milliseconds <= 0.0) return BDF_OK;
    bdf_ctx *R = g->rows;
    const int D = g->D, n = (int)g->ent.size();
    int rc;
    if ((rc = bdf_gibbs_sync(g))) return rc;
    // the chain's state: every entity's current sample, (mu, Lambda), sums, posterior parameters, prior pack, draws, and with
    // side information beta, uhat, the per-row prior means, Tinv, lambda_beta, the iteration counts
    struct Piece { void *p; size_t bytes; bool sample; int ent; };
    std::vector<Piece> pieces;
    std::vector<char> flags;
    const size_t DD = (size_t)D * D * sizeof(double), Dv = (size_t)D * sizeof(double);
    for (int j = 0; j < n; j++) {
        auto &E = g->ent[(size_t)j];
        const bdf_gibbs_entity &e = E.d;
        pieces.push_back({e.sample[E.cur], (size_t)e.N * Dv, true, j});
        pieces.push_back({e.mu, Dv, false, j}); pieces.push_back({e.Lambda, DD, false, j});
        pieces.push_back({e.sumU, Dv, false, j}); pieces.push_back({e.UUt, DD, false, j});
        if (e.params) pieces.push_back({e.params, Dv + DD, false, j});
        pieces.push_back({e.prior_pack, (size_t)bdf_prior_pack_doubles(D) * sizeof(double), false, j});
        pieces.push_back({e.draws, DD + Dv, false, j});
        if (e.spike) pieces.push_back({e.spike_state, 4 * Dv, false, j});      // pi, tau, logit pi, log tau of the spike-and-slab prior
        if (e.nonneg) pieces.push_back({e.nonneg_tau, Dv, false, j});          // tau of the non-negative prior
        if (e.feat) {
            pieces.push_back({e.beta, (size_t)e.feat->n * Dv, false, j});
            pieces.push_back({e.uhat, (size_t)e.N * Dv, false, j});
            pieces.push_back({e.mu_matrix, (size_t)e.N * Dv, false, j});
            pieces.push_back({e.Tinv, DD, false, j});
            pieces.push_back({e.lambda_beta, sizeof(double), false, j});
            if (e.cg_iters) pieces.push_back({e.cg_iters, (size_t)D * sizeof(int32_t), false, j});
        }
        flags.push_back(E.hyper_recorded ? 1 : 0); flags.push_back(E.beta_recorded ? 1 : 0);
    }
    if (g->stats_dev) pieces.push_back({g->stats_dev, 4 * sizeof(double), false, 0});       // the prediction statistics of the last real update
    for (const auto &r : g->rels) {         // the relation models: alpha, relation-level beta, linear_values, the test pairs' baseline
        if (r.alpha_dev) pieces.push_back({r.alpha_dev, sizeof(double), false, 0});
        if (r.feat) {
            int world = 1, rk = 0;
            if (g->comm) (void)bdf_comm_size(g->comm, &rk, &world);
            pieces.push_back({r.beta, (size_t)r.feat->n * sizeof(double), false, 0});
            pieces.push_back({r.linear, (size_t)r.obs_block * (size_t)world * sizeof(double), false, 0});
            if (r.feat_test) pieces.push_back({r.test_baseline, (size_t)r.feat_test->m * sizeof(double), false, 0});
        }
        // the last draw: y - z (probit), mean + y - z (censored, interval)
        if (draws_latent(r)) pieces.push_back({r.linear + r.first_obs, (size_t)r.train->n * sizeof(double), false, 0});
        if (r.robust_nu > 0.0 || r.pg_model || r.noise_mode != 0) pieces.push_back({r.obs_precision, (size_t)r.train->n * sizeof(double), false, 0});       // the last omega
        if (r.noise_mode != 0) pieces.push_back({r.noise_tau, (size_t)r.rel->dims[r.noise_mode - 1] * sizeof(double), false, 0});           // ... and the last tau
        if (r.n_bias != 0) {                // the biases, their precisions, the base they leave the rows and the test pairs
            for (int t = 0; t < r.n_bias; t++) {
                pieces.push_back({r.bias[t].bias, (size_t)r.rel->dims[r.bias[t].mode] * sizeof(double), false, 0});
                pieces.push_back({r.bias[t].lambda, sizeof(double), false, 0});
            }
            pieces.push_back({r.linear, (size_t)r.train->n * sizeof(double), false, 0});
            if (r.bias_test) pieces.push_back({r.test_baseline, (size_t)r.bias_test->n * sizeof(double), false, 0});
        }
        if (r.ordinal) {                    // the edges, the step size, the counters and the trace; the bounds made from the edges
            pieces.push_back({r.ordinal->state_dev, r.ordinal->state_doubles * sizeof(double), false, 0});
            pieces.push_back({const_cast<double *>(r.interval), (size_t)r.train->n * 2 * sizeof(double), false, 0});
        }
    }
    size_t total = 0;
    for (auto &pc : pieces) total += (pc.bytes + 255) & ~(size_t)255;
    DevBuf<char> snap_buf;
    if ((rc = snap_buf.alloc_bytes(std::max<size_t>(total, 256)))) return rc;
    char *const snap = snap_buf.get();
    size_t off = 0;
    for (auto &pc : pieces) {
        BDF_HIP(hipMemcpyAsync(snap + off, pc.p, pc.bytes, hipMemcpyDeviceToDevice, R->stream));
        off += (pc.bytes + 255) & ~(size_t)255;
    }
    BDF_HIP(hipStreamSynchronize(R->stream));
    // full iterations with numbers no real iteration uses; the prediction kernel without running state.  One rank: for the
    // time asked for; several ranks: a fixed count (every rank must make the same number of exchanges)
    const uint32_t keep = R->sweep_host;
    int64_t fixed = 0;                  // several ranks: the iteration count they agreed on (0: not yet known / one rank)
    const auto t0 = std::chrono::steady_clock::now();
    int64_t k = 0;
    rc = BDF_OK;
    while (!rc) {
        for (int b = 0; b < 8 && !rc; b++, k++) rc = bdf_gibbs_sweep(g, 0xfffe0000u + (uint32_t)(k & 0xffff), g->test ? 3 : -1);
        if (rc) break;
        if (g->comm && fixed == 0) {
            // the first batch, timed to its end on this rank; the ranks' counts summed in rank order: the same number everywhere
            if ((rc = bdf_gibbs_sync(g))) break;
            const double per_iter = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / 8.0;
            const double mine = std::max(8.0, std::min(20000.0, milliseconds / std::max(per_iter, 1e-3)));
            int rank = 0, world = 1;
            if ((rc = bdf_comm_size(g->comm, &rank, &world))) break;
            void *sv;
            if ((rc = bdf_scratch(R, ((size_t)world + 1) * sizeof(double), &sv))) break;
            double *cnt = (double *)sv;
            BDF_HIP(hipMemcpyAsync(cnt, &mine, sizeof(double), hipMemcpyHostToDevice, R->stream));
            if ((rc = bdf_sum_ranks_into(R, g->comm, cnt, 1, cnt + 1))) break;
            double sum = 0.0;
            BDF_HIP(hipMemcpyAsync(&sum, cnt, sizeof(double), hipMemcpyDeviceToHost, R->stream));
            BDF_HIP(hipStreamSynchronize(R->stream));
            fixed = std::max<int64_t>(8, (int64_t)(sum / (double)world + 0.5));
        }
        if (fixed ? k >= fixed : std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() >= milliseconds) break;
    }
    const int rc_sync = bdf_gibbs_sync(g);
    if (!rc) rc = rc_sync;
    // put the state back: the saved sample into whichever buffer is current now, everything else where it was
    off = 0;
    for (auto &pc : pieces) {
        void *dst = pc.sample ? (void *)g->ent[(size_t)pc.ent].d.sample[g->ent[(size_t)pc.ent].cur] : pc.p;
        BDF_HIP(hipMemcpyAsync(dst, snap + off, pc.bytes, hipMemcpyDeviceToDevice, R->stream));
        off += (pc.bytes + 255) & ~(size_t)255;
    }
    for (int j = 0; j < n; j++) {
        sample_written(g, g->ent[(size_t)j]);
        g->ent[(size_t)j].hyper_recorded = flags[(size_t)2 * j] != 0;
        g->ent[(size_t)j].beta_recorded = flags[(size_t)2 * j + 1] != 0;
    }
    BDF_HIP(hipStreamSynchronize(R->stream));
    R->sweep_host = g->hyper->sweep_host = g->pred->sweep_host = keep;
    return rc;
}

// (set-up) whether the entity's hyperprior draw / beta of an earlier iteration exist -- what the next iteration's row launch
// takes its prior pack from and waits for; a caller that runs iterations and then puts the chain's state back (the engine's
// device warm-up) puts these back with it
extern "C" int bdf_gibbs_recorded(const bdf_gibbs *g, int entity, int *hyper, int *beta)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size() && hyper && beta, BDF_ERR_ARG, "bdf_gibbs_recorded: bad argument");
    *hyper = g->ent[(size_t)entity].hyper_recorded ? 1 : 0;
    *beta = g->ent[(size_t)entity].beta_recorded ? 1 : 0;
    return BDF_OK;
}

extern "C" int bdf_gibbs_set_recorded(bdf_gibbs *g, int entity, int hyper, int beta)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_set_recorded: bad argument");
    g->ent[(size_t)entity].hyper_recorded = hyper != 0;
    g->ent[(size_t)entity].beta_recorded = beta != 0;
    sample_written(g, g->ent[(size_t)entity]);        // (a caller that puts the chain's state back: the sample with it)
    return BDF_OK;
}

// the caller has written entity's sample (any of its three buffers) itself, or is about to, with nothing of the chain in flight
extern "C" int bdf_gibbs_sample_written(bdf_gibbs *g, int entity)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_sample_written: bad argument");
    sample_written(g, g->ent[(size_t)entity]);
    return BDF_OK;
}

extern "C" int bdf_gibbs_time_rows(bdf_gibbs *g, int entity, void *start, void *stop)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_time_rows: bad entity");
    g->ent[(size_t)entity].t_start = (hipEvent_t)start;
    g->ent[(size_t)entity].t_stop = (hipEvent_t)stop;
    return BDF_OK;
}

extern "C" int bdf_gibbs_span_rows(bdf_gibbs *g, int entity, void *slot_dev)
{
    BDF_REQUIRE(g && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_span_rows: bad entity");
    g->ent[(size_t)entity].span = (unsigned long long *)slot_dev;
    return BDF_OK;
}

extern "C" int bdf_gibbs_current(const bdf_gibbs *g, int entity, int *buffer)
{
    BDF_REQUIRE(g && buffer && entity >= 0 && entity < (int)g->ent.size(), BDF_ERR_ARG, "bdf_gibbs_current: bad argument");
    *buffer = g->ent[(size_t)entity].cur;
    return BDF_OK;
}

namespace {
// The row kernels of the NEXT sweep overwrite the buffers that held the rows of sweep - 2, which the prediction update of
// sweep - 2 reads.  The HOST waits here until an update of some sweeps ago has completed (normally it has, long ago): the
// device then needs no wait for the prediction stream anywhere, and the host never runs more than a few prediction updates
// ahead.  (A device-side wait would let row kernels that poll for their prior fill the chip while the prediction kernel
// they transitively wait for still needs slots for its last workgroups.)
// (Whether or not THIS iteration has a prediction update: an update enqueued two or more iterations ago must have
// completed -- iterations without one rotate the buffers all the same.)
// How many iterations back: 3 -- the most the three buffers allow: iteration s overwrites the rows of iteration s - 3, which the
// prediction update of s - 3 read.  (Until round 3: 2.  On a quiet host there is no difference; with 3 an enqueue that takes
// 50 us instead of 23, or a late wake-up, no longer leaves the row stream dry.)
int await_old_predictions(bdf_gibbs *g)
{
    constexpr uint64_t pred_lag = 3;
    for (uint64_t back = 1; back <= std::min<uint64_t>(g->n_pred, 3); back++) {
        const uint64_t k = (g->n_pred - back) % 3;
        if (g->pred_at[k] + pred_lag <= g->n_iter) {          // (and with it the earlier ones)
            // a short spin on the event before the blocking wait: a thread put to sleep here wakes 10-40 us after the event,
            // and with the host one iteration ahead of the device at that moment a late wake-up plus a slow enqueue (50 us on
            // a busy host) leaves the row stream dry
            hipError_t st = hipErrorNotReady;
            const auto t_spin = std::chrono::steady_clock::now();
            while ((st = hipEventQuery(g->ev_pred[k])) == hipErrorNotReady &&
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_spin).count() < 400.0) { }
            if (st == hipErrorNotReady) st = hipEventSynchronize(g->ev_pred[k]);
            BDF_HIP(st);
            break;
        }
    }
    return BDF_OK;
}

// the data-independent part of every entity's hyperprior draw (Bartlett matrix, mean normals): inside the entity's chain
// launch, beside its partial sums, when every entity is small enough for the one-launch chain (the hyperprior stream is
// busy ~85 of an iteration's 90 us: a launch of its own at the head of the iteration is 7 us of that); else ahead of the rows
// (for all entities in one launch, here at the head of the iteration, when they are few).  *in_chain: the chain makes them
int draws_ahead(bdf_gibbs *g, bool *in_chain)
{
    *in_chain = !g->comm;                // (several ranks: the sums are not the chain's, bdf_hyper_sums_ranks)
    for (const auto &E : g->ent) *in_chain = *in_chain && E.d.N <= 16384;
    if (*in_chain || (int)g->ent.size() > BDF_DRAWS_BATCH) return BDF_OK;
    int64_t Ns[BDF_DRAWS_BATCH]; double nus[BDF_DRAWS_BATCH]; uint32_t tags[BDF_DRAWS_BATCH]; double *outs[BDF_DRAWS_BATCH];
    int nb = 0;                           // (an entity with the spike-and-slab or the non-negative prior has no Normal-Wishart draw)
    for (const auto &E : g->ent) {
        const bdf_gibbs_entity &e = E.d;
        if (own_prior(e)) continue;
        Ns[nb] = e.n_real; nus[nb] = hyper_nu(e); tags[nb] = e.tag; outs[nb] = e.draws; nb++;
    }
    return nb > 0 ? bdf_hyper_draws_batch(g->hyper, g->D, nb, Ns, nus, tags, outs) : BDF_OK;
}

// The prediction update reads every entity's rows of this iteration.  Hand-over by counter: a one-wave gate (k_rows_gate) on
// a stream of the reserved CUs polls this launch's done counters, and the prediction stream waits for the event on the
// GATE's dispatch (ev_rows, which nothing else uses on this path).  That orders the update behind all the rows:
//   * the gate returns only after the done counters say every row of this launch is in memory;
//   * the earlier entities' launches of this iteration are ahead of this one on the in-order row stream (and this launch
//     gathers their rows): complete before its first wave started.
// No cycle: the gate is enqueued BEHIND the launch it waits for and waits for nothing else; should its stream share a hardware
// queue with another one, it runs late, never early.  Rows still wait for the prediction stream nowhere on the device.
// (Waiting for ev_hyper of this entity's chain instead -- no kernel, the same order -- starts the update ~28 us after the
// rows instead of at their end, where it stretches BOTH row launches it then meets: 11.2-11.4 k sweeps/s against the
// event's 12.2-12.4 k, profiles/r08_update_handover.txt.)
int gate_prediction(bdf_gibbs *g, const bdf_gibbs::Ent &E)
{
    hipExtLaunchKernelGGL(k_rows_gate, dim3(1), dim3(64), 0, g->gate->stream, nullptr, E.ev_rows, 0, (const uint32_t *)E.done_dev, E.done_target,
                          g->hyper->flag_dev);
    BDF_HIP(hipGetLastError());
    BDF_HIP(hipStreamWaitEvent(g->pred->stream, E.ev_rows, 0));
    return BDF_OK;
}

// the prediction update of this iteration's rows on the prediction stream, and its event
int predict_step(bdf_gibbs *g, int predict_phase)
{
    bdf_ctx *P = g->pred;
    int rc;
    const double *fac[BDF_MAX_MODES];
    current_factors(g, g->test_entity, g->test->n_modes, fac);
    // (phase 3, set-up only: the same kernel on the same pairs, statistics of this sample into stats_dev, no running state)
    if ((rc = predict_phase == 3 ? bdf_predict_sse(P, g->test, g->D, fac, g->test_mean, nullptr, g->stats_dev)
                                 : bdf_predict_update(P, g->test, g->D, fac, g->test_mean, predict_phase, g->clamp_lo, g->clamp_hi, g->class_cut, g->stats_dev)))
        return rc;
    BDF_HIP(hipEventRecord(g->ev_pred[g->n_pred % 3], P->stream));
    g->pred_at[g->n_pred % 3] = g->n_iter;
    g->n_pred++;
    return BDF_OK;
}
}  // namespace

// One iteration: the schedule.  It composes the pieces above -- update_relations, launch_rows, hyper_step, beta_step -- with its events,
// polling and counters; what each piece enqueues is the piece's business.
extern "C" int bdf_gibbs_sweep(bdf_gibbs *g, uint32_t sweep, int predict_phase)
{
    BDF_REQUIRE(g, BDF_ERR_ARG, "bdf_gibbs_sweep: NULL argument");
    bdf_ctx *R = g->rows, *H = g->hyper, *P = g->pred;
    const int D = g->D, n = (int)g->ent.size();
    int rc;
    R->sweep_host = H->sweep_host = P->sweep_host = sweep;
    const auto t_in = std::chrono::steady_clock::now();
    if ((rc = await_old_predictions(g))) return rc;
    const auto t_go = std::chrono::steady_clock::now();
    bool draws_in_chain;
    if ((rc = draws_ahead(g, &draws_in_chain))) return rc;
    // the relation models (alpha, relation-level beta and linear_values) with the rows of the previous iteration (macau.jl:83-92)
    if (!g->rels.empty() && (rc = update_relations(g))) return rc;
    for (int j = 0; j < n; j++) {
        auto &E = g->ent[(size_t)j];
        const bdf_gibbs_entity &e = E.d;
        // (mu, Lambda) of the previous iteration: an event wait, or -- draws on reserved CUs -- the row kernel polls for it
        // (with side information the prior mean is a matrix, computed here from mu: nothing to poll for)
        // (several ranks: event waits unless BDF_POLL_WITH_COMM is set -- the draws of an iteration depend on nothing the rows of
        // the next one produce, so polling cannot deadlock with the exchange's kernels either, but that schedule has only run
        // with a one-rank RCCL communicator: tools/soak_determinism.py rccl)
        static const bool poll_with_comm = getenv("BDF_POLL_WITH_COMM") != nullptr;
        // (an entity with background cells is ordered like one with side information: its prior is made here, on the row stream, from
        // the draw -- behind the draw's event, and its rows join neither the polling nor the hand-over by counter below)
        // (an entity with a dense relation likewise)
        const bool bg = folds_prior(g, e);
        // (so is an entity with the spike-and-slab or the non-negative prior: its rows wait for the event of its hyper step)
        const bool poll = g->polling && (!g->comm || poll_with_comm) && E.hyper_recorded && !e.feat && !bg && !own_prior(e);
        if (E.hyper_recorded && !poll) BDF_HIP(hipStreamWaitEvent(R->stream, E.ev_hyper, 0));
        // side information: uhat = (F beta)' with the beta of the previous iteration, per-row prior means mu + uhat (macau.jl:103-104)
        if (e.feat && (rc = bdf_uhat(R, e.feat, D, e.beta, e.mu, e.uhat, e.mu_matrix))) return rc;
        // the data-independent part of the hyperprior draw (Bartlett matrix, mean normals): beside the rows -- for all entities
        // in one launch at the head of the iteration when they are few
        if (!draws_in_chain && n > BDF_DRAWS_BATCH && !own_prior(e) && (rc = bdf_hyper_draws(H, D, e.n_real, hyper_nu(e), e.tag, e.draws))) return rc;
        // the completion event rides on the row kernel's dispatch (a caller-supplied timing pair takes its place)
        hipEvent_t done = E.t_stop ? E.t_stop : E.ev_rows;
        // The hand-over to the entity's hyperprior chain.  By default an event on the row kernel's dispatch and a wait on the
        // hyperprior stream -- which costs that stream ~10 us per chain even when the event completed long before, and the row
        // stream ~1.7 us per launch.  When the chain is the one-launch kind and runs on reserved CUs (the schedule in which the
        // row kernels poll for the draw), the chain is enqueued AT ONCE instead and its partial-sum workgroups poll a counter
        // the row waves add to when their rows are in memory (SampleArgs::done; k_rows_col only -- a launch that takes another
        // kernel reports -1 and gets the event).  No cycle: the rows of iteration t poll for the draw of t - 1, enqueued before.
        // The last entity's launch is no exception when the prediction update follows it: nothing rides on its dispatch either.  (It
        // carried `done` for the prediction stream to wait on, the one event left on the row stream: the next iteration's first row
        // launch followed it after ~5 us in the kernel trace where the other launches follow each other after 0.)  The prediction
        // stream waits for a one-wave gate on the reserved CUs instead, see gate_prediction.
        // Every other path -- a communicator, side information, chunks, a caller's timing events (E.t_stop), no polling, chains of
        // several launches: `counter` false; a launch that took another kernel: rows_done_added < 0 -- has `done` as before, on the
        // dispatch or recorded right behind it, for the chain and the prediction stream alike.
        const bool counter = E.done_dev && draws_in_chain && g->polling && !g->comm && !e.feat && !bg && !own_prior(e) && e.terms[0].rel->chunks == 1 && !E.t_stop;
        const bool pred_waits = j == n - 1 && g->test && predict_phase >= 0;
        RowsExtras rx{};
        rx.start = E.t_start; rx.span = E.span;
        rx.stop = (!g->comm && !counter) ? done : nullptr; rx.joined = g->comm ? done : nullptr;
        if (poll) { rx.poll = g->ready_dev + j; rx.poll_want = E.epoch; }
        if (counter) rx.counter = E.done_dev;
        bool by_counter = false;
        if ((rc = launch_rows(g, E, E.hyper_recorded, true, rx, &by_counter))) return rc;
        if (counter && !by_counter) BDF_HIP(hipEventRecord(done, R->stream));      // (the launch took another kernel: the event after all)
        E.t_start = E.t_stop = nullptr; E.span = nullptr;
        HyperExtras hx{};
        if (by_counter) { hx.wait = E.done_dev; hx.wait_target = E.done_target; }
        else BDF_HIP(hipStreamWaitEvent(H->stream, done, 0));
        if (!own_prior(e)) {
            hx.fuse = true; hx.chain_draws = draws_in_chain ? e.draws : nullptr;
            hx.stop = E.ev_hyper; hx.ready = g->ready_dev + j; hx.ready_value = ++E.epoch;
            if (e.feat && e.full_lambda_u && E.beta_recorded) BDF_HIP(hipStreamWaitEvent(H->stream, E.ev_beta, 0));
        }
        if ((rc = hyper_step(g, E, H, e.draws, hx))) return rc;
        if (own_prior(e)) BDF_HIP(hipEventRecord(E.ev_hyper, H->stream));         // (its event recorded behind it)
        E.hyper_recorded = true;
        if (pred_waits && by_counter) { if ((rc = gate_prediction(g, E))) return rc; }
        else if (pred_waits) BDF_HIP(hipStreamWaitEvent(P->stream, done, 0));
    }
    // side information: beta of every entity that has it, from this iteration's rows and (mu, Lambda) (macau.jl:138-140)
    for (int j = 0; j < n; j++) {
        auto &E = g->ent[(size_t)j];
        if (!E.d.feat) continue;
        BDF_HIP(hipStreamWaitEvent(R->stream, E.ev_hyper, 0));
        if ((rc = beta_step(g, E))) return rc;
        BDF_HIP(hipEventRecord(E.ev_beta, R->stream));
        E.beta_recorded = true;
    }
    if (g->test && predict_phase >= 0 && (rc = predict_step(g, predict_phase))) return rc;
    g->n_iter++;
    if (g->debug) {
        g->host_wait_us += std::chrono::duration<double, std::micro>(t_go - t_in).count();
        g->host_enqueue_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_go).count();
        g->n_sweeps++;
    }
    return BDF_OK;
}

extern "C" int bdf_gibbs_sync(bdf_gibbs *g)
{
    BDF_REQUIRE(g, BDF_ERR_ARG, "bdf_gibbs_sync: NULL argument");
    int rc;
    if ((rc = bdf_ctx_sync(g->pred)) || (rc = bdf_ctx_sync(g->hyper))) return rc;
    return bdf_ctx_sync(g->rows);
}
