// ofx_loop.h -- data-dependent iteration loops without a host round trip per iteration.
//
// All three solvers have the same shape: `while (error > tol && n < max) { n++; sweep; error = f(sum) }`
// (src/tvl1flow.cpp:113, src/horn_schunck_pyramidal.cpp:143, src/brox_optic_flow_spatial.cpp:315).
// On the GPU every sweep k adds its per-wave partial sums into err[k][wave % 64] (one f64 atomic
// per wave).  The FIRST thing every kernel of sweep k+1 does is fetch the 64 shards of err[k]; it
// reduces them in a fixed butterfly order, applies the reference's own test and returns at once
// when the loop is over -- and then every later launch sees an untouched all-zero slot and is a
// no-op too.  The host enqueues sweeps in chunks; a one-block finalize kernel after each chunk
// publishes {n, done, error} into pinned host memory, and the host reads that record one chunk
// behind the GPU.  `n` is therefore exactly the reference's iteration count.
#pragma once

#include "ofx_internal.h"
#include "ofx_device.h"
#include "ofx_loop_plan.h"

#define OFX_CRIT_MEAN      0   // error = sum / size           (TV-L1, tvl1flow.cpp:162)
#define OFX_CRIT_SQRT_MEAN 1   // error = sqrt(sum / size)     (HS :230, Brox :389)

OFX_DEV double loop_error_from_sum(double sum, int size, int crit)
{
    const double m = sum / size;
    return crit == OFX_CRIT_SQRT_MEAN ? sqrt(m) : m;
}

// Fetch this lane's shard of sweep k-1 (call first, use late: the load overlaps with other loads).
OFX_DEV double loop_fetch_prev(const double *err, int k)
{
    return k > 0 ? err[(size_t) (k - 1) * OFX_NSHARD + (threadIdx.x & 63)] : 0.0;
}

// true when sweep k must run.  Full waves only.
OFX_DEV bool loop_continues(double prev_shard, int k, int size, double thr, int crit)
{
    if (k == 0) return true;
    const double error = loop_error_from_sum(wave_allreduce_sum(prev_shard), size, crit);
    return error > thr;
}

// Add a wave's partial sum into sweep k's slot.  Full waves only; `wave_id` spreads the shards.
OFX_DEV void loop_accumulate(double *err, int k, double lane_value, int wave_id)
{
    const double s = wave_allreduce_sum(lane_value);
    if ((threadIdx.x & 63) == 0) atomicAdd(err + (size_t) k * OFX_NSHARD + (wave_id & (OFX_NSHARD - 1)), s);
}

struct LoopSpec {
    int    max_iter;   // reference's MAX_ITERATIONS / maxiter
    int    size;       // nx * ny of the level
    double thr;        // eps^2 (TV-L1) or TOL (SOR)
    int    crit;       // OFX_CRIT_*
    int    chunk;      // sweeps per poll
    bool   fixed;      // run exactly max_iter sweeps (stopping test disabled)
    bool   pairs;      // the solver fuses two sweeps per launch where it can (TV-L1)
    int    fuse = 0;   // > 2: the solver fuses this many sweeps per launch (TV-L1 tile kernel of the small levels); a loop that
                       // stops inside a launch unit is finished by redo(), which re-runs the unit's first sweeps from its input
    double afac = 0.0; // pairs only: a fused launch whose previous error is <= thr * afac also stores the state between
                       // its two sweeps (0 = never); the finalize kernel reports whether the stopping launch did
};

int ofx_loop_reserve(ofx_ctx *ctx, int max_iter);                      // err slots for max_iter sweeps
int ofx_loop_clear(ofx_ctx *ctx, size_t slots);                        // zero the loop state + the first `slots` error slots
// G problems in lockstep: problem g owns err slots [g * slots_per_problem, ...) and state entry g.
// seq: number the records carry when they are complete (never 0); ofx_loop_wait_poll(slot, G, seq) waits for them
int ofx_loop_finalize_group(ofx_ctx *ctx, const LoopSpec &L, int G, int slots_per_problem, int start, int launched,
                            OfxIterState *host_slot, int seq);
int ofx_loop_finalize_cursor(ofx_ctx *ctx, const LoopSpec &L, int G, int slots_per_problem, int launch_end, int max_range,
                             OfxIterState *host_slot, int seq);
int ofx_loop_wait_poll(ofx_ctx *ctx, int slot, int G, int seq);

// ---- polls: the one way a loop learns where it stands --------------------------------------------------------------------------
// A poll = a finalize kernel behind the launches it covers, writing G records into a slot of the pinned ring, and an event
// behind it.  ofx_poll_issue takes the next sequence number (before it advances the count: every site the same) and slot, has
// finalize(host_slot, seq) enqueue the kernel and records the event; ofx_poll_read waits and copies the G records out -- `spin`:
// on the records' sequence numbers first (ofx_loop_wait_poll: a loop with a chunk of lookahead), else on the event alone (the
// exact SOR batches, which have nothing in flight behind the poll).
struct OfxPoll { int slot, seq; };
template <class FinalizeFn> static int ofx_poll_issue(ofx_ctx *ctx, FinalizeFn finalize, OfxPoll *p)
{
    p->seq = (int) (ctx->poll_seq & 0x3FFFFFFF) + 1;
    p->slot = (int) (ctx->poll_seq++ % OFX_NPOLL);
    OFX_TRY(finalize(&ctx->h_state[p->slot * OFX_MAX_GROUP], p->seq));
    OFX_HIP(ctx, hipEventRecord(ctx->ev_poll[p->slot], ctx->stream));
    return OFX_OK;
}
static int ofx_poll_read(ofx_ctx *ctx, const OfxPoll &p, int G, bool spin, OfxIterState *out)
{
    if (spin) OFX_TRY(ofx_loop_wait_poll(ctx, p.slot, G, p.seq));
    else OFX_HIP(ctx, hipEventSynchronize(ctx->ev_poll[p.slot]));
    for (int g = 0; g < G; g++) out[g] = ctx->h_state[p.slot * OFX_MAX_GROUP + g];
    return OFX_OK;
}

// What ofx_run_loop_group and ofx_run_loop_cursor share: the error slots and the state of G problems (problem g accumulates into
// err slots g * (L.max_iter + 1) + k; + 1: the scratch slot for a re-run's errors), the pump (ofx_loop_plan.h) and the timing.
// more() / enqueue(S, per, &poll) -- a chunk of launches and its poll -- feed the pump; decide(fin) gets the G final records.
// A context that has the device to itself keeps two polls outstanding (the one the host waits for and one chunk of lookahead,
// so the GPU never idles while the host reads a poll) at the price of one chunk of no-op launches behind the stopping
// iteration.  When other contexts share the device (option "concurrency" > 1) their work fills such gaps, so nothing is
// launched speculatively: one outstanding poll.
template <class MoreFn, class EnqueueFn, class DecideFn>
static int ofx_loop_drive_impl(ofx_ctx *ctx, const LoopSpec &L, int G, MoreFn more, EnqueueFn enqueue, DecideFn decide, float *ms_out)
{
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "loop group of %d problems", G);
    const int per = L.max_iter + 1;
    OFX_TRY(ofx_loop_reserve(ctx, G * per));
    LoopSpec S = L;
    if (S.fixed) S.thr = -1.0;          // error >= 0 always passes `error > -1`
    OFX_TRY(ofx_loop_clear(ctx, (size_t) G * per));
    if (ms_out) OFX_HIP(ctx, hipEventRecord(ctx->ev_t0, ctx->stream));
    OfxPoll poll[2];
    OfxIterState fin[OFX_MAX_GROUP];
    bool stopped = false;
    OFX_TRY(ofx_loop_pump(
        ctx->concurrency > 1 ? 1 : 2, more, [&](int i) -> int { return enqueue(S, per, &poll[i]); },
        [&](int i, bool *all) -> int {
            OFX_TRY(ofx_poll_read(ctx, poll[i], G, true, fin));
            *all = true;
            for (int g = 0; g < G; g++) *all = *all && fin[g].done;
            return OFX_OK;
        },
        &stopped));
    if (!stopped) return ofx_fail(ctx, OFX_ERR_HIP, "iteration loop ended without a final state");
    OFX_TRY(decide(fin));
    if (ms_out) {
        OFX_HIP(ctx, hipEventRecord(ctx->ev_t1, ctx->stream));
        OFX_HIP(ctx, hipEventSynchronize(ctx->ev_t1));
        OFX_HIP(ctx, hipEventElapsedTime(ms_out, ctx->ev_t0, ctx->ev_t1));
    }
    return OFX_OK;
}
// An error return must not leave launches or a poll of this loop in flight: the next API call resets the arena these
// kernels work in.  (Stream order already protects the next call's own kernels; the drain makes it hold for anything
// else the caller does with the context.)
template <class MoreFn, class EnqueueFn, class DecideFn>
static int ofx_loop_drive(ofx_ctx *ctx, const LoopSpec &L, int G, MoreFn more, EnqueueFn enqueue, DecideFn decide, float *ms_out)
{
    const int s = ofx_loop_drive_impl(ctx, L, G, more, enqueue, decide, ms_out);
    if (s != OFX_OK) (void) hipStreamSynchronize(ctx->stream);
    return s;
}

// Runs the loop for G independent problems of the same size in LOCKSTEP (TV-L1: G image pairs solved by
// the same launches, blockIdx.y = problem; the SOR solvers use G = 1).  Problem g stops on its own test -- its launches turn
// into no-ops while the others continue; the host stops enqueueing when every problem is done.
//   launch(k, count, thr) must enqueue every kernel of sweeps k .. k+count-1 of ALL problems on ctx->stream
// (count is 2 only when L.pairs and at least two sweeps remain; pairs always start at an even k); kernels
// take (ctx->d_err, k, thr) and use the helpers above (L.fuse > 2: count is up to L.fuse, units start at multiples of it, and
// redo(k_of) must re-run the first n_g - k0 sweeps of the unit that contains sweep k_of[g] = n_g - 1 from that unit's input).
// With L.pairs the second sweep of a pair runs even
// when the first one ended the loop; if that happens for any problem (n odd), redo(k_of) is called ONCE with
// k_of[g] = n_g - 1 for those problems and -1 for the others, and must recompute sweep k_of[g] of each such
// problem alone from the pair's untouched input buffers.  Problems whose stopping launch had stored its intermediate
// state (L.afac, or bit g of amask0 for a loop that stopped in its very first launch) need no redo: took_alt[g] = 1
// tells the caller to continue from that stored state.  Returns the reference's n and error per problem.
template <class LaunchFn, class RedoFn>
static int ofx_run_loop_group(ofx_ctx *ctx, const LoopSpec &L, int G, LaunchFn launch, RedoFn redo, int *n_out,
                              double *err_out, float *ms_out, unsigned amask0 = 0, int *took_alt = nullptr)
{
    const int F = ofx_loop_unit_size(L.pairs, L.fuse);
    OfxChunkSchedule sched(L.max_iter, L.chunk, F);
    auto enqueue = [&](const LoopSpec &S, int per, OfxPoll *p) -> int {
        OFX_TRY(sched.next([&](int k, int cnt) -> int { return launch(k, cnt, S.thr); }));
        return ofx_poll_issue(ctx, [&](OfxIterState *slot, int seq) -> int {
            return ofx_loop_finalize_group(ctx, S, G, per, sched.first, sched.launched, slot, seq); }, p);
    };
    auto decide = [&](const OfxIterState *fin) -> int {
        int redo_k[OFX_MAX_GROUP];
        bool any_redo = false;
        for (int g = 0; g < G; g++) {
            const bool inside = ofx_loop_inside(fin[g].n, F, L.max_iter);
            const bool stored = ofx_loop_took_alt(inside, F, took_alt != nullptr, fin[g].apred, fin[g].n, (amask0 >> g) & 1u);
            if (took_alt) took_alt[g] = stored ? 1 : 0;
            redo_k[g] = inside && !stored ? fin[g].n - 1 : -1;
            any_redo = any_redo || redo_k[g] >= 0;
            n_out[g] = fin[g].n;
            err_out[g] = fin[g].error;
        }
        return any_redo ? redo(redo_k) : OFX_OK;
    };
    return ofx_loop_drive(ctx, L, G, [&] { return sched.more(); }, enqueue, decide, ms_out);
}

// single problem (the SOR solvers); redo(k) as above for the one problem
template <class LaunchFn, class RedoFn>
static int ofx_run_loop(ofx_ctx *ctx, const LoopSpec &L, LaunchFn launch, RedoFn redo, int *n_out, double *err_out,
                        float *ms_out)
{
    return ofx_run_loop_group(ctx, L, 1, launch, [&](const int *k_of) { return redo(k_of[0]); }, n_out, err_out, ms_out);
}


// ---- cursor loops ---------------------------------------------------------------------------------------------------------
// The launch units of a loop have NO fixed size: every launch reads where its pair stands from device memory (OfxLoopDev), picks
// its own iteration count (TV-L1: three or four iterations -- max_unit -- while the loop is far from its threshold, fewer when the
// previous error says the stop is near -- fewer iterations computed past the stop, fewer re-runs) and logs where it started.  A
// launch looks max_unit error slots back, so every launch behind the stop is a no-op.  The host only counts
// launches: launch(L, thr) enqueues launch L for all problems; units_per_chunk launches, then one finalize kernel (which learns
// the iteration range from the device state), polled one chunk behind as in ofx_run_loop_group.  On return unit_out[g] is the
// launch unit that contains iteration n_g - 1 (-1: none ran); when the loop ended INSIDE that unit (inside_out[g]),
// redo(n_of, k0_of, unit_of) -- called once, n_of -1 for the problems that need nothing -- must re-run its first n - k0
// iterations from the unit's input buffers.
template <class LaunchFn, class RedoFn>
static int ofx_run_loop_cursor(ofx_ctx *ctx, const LoopSpec &L, int G, int units_per_chunk, int max_unit, LaunchFn launch, RedoFn redo,
                               int *n_out, double *err_out, int *unit_out, int *inside_out, float *ms_out)
{
    const int upc = units_per_chunk < 1 ? 1 : units_per_chunk;
    int launches = 0;
    auto enqueue = [&](const LoopSpec &S, int per, OfxPoll *p) -> int {
        const int c = OFX_ULOG - launches < upc ? OFX_ULOG - launches : upc;
        for (int i = 0; i < c; i++) OFX_TRY(launch(launches++, S.thr));
        return ofx_poll_issue(ctx, [&](OfxIterState *slot, int seq) -> int {
            return ofx_loop_finalize_cursor(ctx, S, G, per, launches, c * max_unit, slot, seq); }, p);
    };
    auto decide = [&](const OfxIterState *fin) -> int {
        int n_of[OFX_MAX_GROUP], k0_of[OFX_MAX_GROUP], u_of[OFX_MAX_GROUP];
        bool any = false;
        for (int g = 0; g < G; g++) {
            const bool inside = ofx_loop_inside_cursor(fin[g].n, fin[g].k0, fin[g].ucnt);
            n_of[g] = inside ? fin[g].n : -1;
            k0_of[g] = fin[g].k0;
            u_of[g] = fin[g].unit;
            any = any || inside;
            n_out[g] = fin[g].n;
            err_out[g] = fin[g].error;
            unit_out[g] = fin[g].n > 0 ? fin[g].unit : -1;
            if (inside_out) inside_out[g] = inside ? 1 : 0;
        }
        return any ? redo(n_of, k0_of, u_of) : OFX_OK;
    };
    return ofx_loop_drive(ctx, L, G, [&] { return launches < OFX_ULOG; }, enqueue, decide, ms_out);
}
