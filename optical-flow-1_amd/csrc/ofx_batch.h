// ofx_batch.h -- what every multi-context entry (*_batch_dev, *_sequence_dev, *_triples_dev) and every lockstep-group entry
// (*_group_dev) shares on the host: the contexts' agreement, the memory budget, the worker loop over the groups and the shell
// around one group's solve.  Private to libofx.so; the group sizes are ofx_group_plan.h's, and the entries on PAIRS of frames
// (TV-L1, Horn-Schunck, Brox) build their ladder -- group, group with starts, batch, video chain -- on ofx_pairs.h.
#pragma once

#include "ofx_internal.h"
#include "ofx_group_plan.h"

#include <atomic>
#include <thread>

// what the contexts of a batch must have in common with ctxs[0]
enum {
    OFX_SAME_DEVICE = 1,    // everything but the TV-L1 batches, which may span GPUs
    OFX_SAME_FORMAT = 2     // precision, "input" and "input_pitch": every entry that reads device-resident frames
};
static inline int ofx_batch_check_ctxs(ofx_ctx *const *ctxs, int n_ctx, int what)
{
    if (!ctxs || n_ctx < 1) return OFX_ERR_ARG;
    for (int w = 0; w < n_ctx; w++) {
        const ofx_ctx *c = ctxs[w], *c0 = ctxs[0];
        if (!c) return OFX_ERR_ARG;
        if ((what & OFX_SAME_DEVICE) && c->device != c0->device) return OFX_ERR_ARG;
        if ((what & OFX_SAME_FORMAT) && (c->precision != c0->precision || c->input != c0->input || c->input_pitch != c0->input_pitch))
            return OFX_ERR_ARG;
    }
    return OFX_OK;
}

// bytes each of n_ctx contexts on ctx's device (the current one) may use: option "mem_budget", else half of what is free now
static inline int ofx_batch_budget(ofx_ctx *ctx, int n_ctx, double *bytes)
{
    size_t free_b = 0, total_b = 0;
    OFX_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    *bytes = (ctx->mem_budget > 0 ? ctx->mem_budget : 0.5 * (double) free_b) / n_ctx;
    return OFX_OK;
}

// The worker loop: n_items cut into groups of G consecutive items, group q on context q mod n_ctx, a host thread per context at
// work.  group(ctx, first, cnt, st) solves items first .. first + cnt - 1 into the records_per_item * cnt records st, record r of
// item g at st[r * cnt + g]; its work lands at work_pix_iters[r * n_items + first + g] (NULL: nowhere).  share_hint: every
// context's tuning hint `concurrency` is at least the number of workers for the duration -- it picks strip heights, poll depth
// and fused kernels, so an entry keeps the setting it was measured with.  Returns when every context's stream has drained, with
// the first failing status.
template <class GroupFn>
static int ofx_run_groups(ofx_ctx *const *ctxs, int n_ctx, int n_items, int G, int records_per_item, double *work_pix_iters,
                          bool share_hint, GroupFn group)
{
    const int n_groups = (n_items + G - 1) / G;
    const int n_workers = n_ctx < n_groups ? n_ctx : n_groups;
    std::vector<int> conc(n_ctx);
    for (int w = 0; w < n_ctx; w++) {
        conc[w] = ctxs[w]->concurrency;
        if (share_hint && conc[w] < n_workers) ctxs[w]->concurrency = n_workers;
    }
    std::atomic<int> status(OFX_OK);
    auto fail = [&](int s) { int expected = OFX_OK; status.compare_exchange_strong(expected, s); };
    auto worker = [&](int w) {
        std::vector<ofx_stats> st((size_t) records_per_item * G);
        for (int q = w; q < n_groups; q += n_ctx) {
            if (status.load() != OFX_OK) return;
            const int first = q * G, cnt = (n_items - first < G) ? n_items - first : G;
            const int s = group(ctxs[w], first, cnt, st.data());
            if (s != OFX_OK) { fail(s); return; }
            for (int r = 0; work_pix_iters && r < records_per_item; r++)
                for (int g = 0; g < cnt; g++) work_pix_iters[(size_t) r * n_items + first + g] = st[r * cnt + g].work_pix_iters;
        }
        if (hipStreamSynchronize(ctxs[w]->stream) != hipSuccess) fail(ofx_fail(ctxs[w], OFX_ERR_HIP, "hipStreamSynchronize failed"));
    };
    std::vector<std::thread> th;
    for (int w = 1; w < n_workers; w++) th.emplace_back(worker, w);
    worker(0);
    for (auto &t : th) t.join();
    for (int w = 0; w < n_ctx; w++) ctxs[w]->concurrency = conc[w];
    return status.load();
}

// The shell of a lockstep group, after the entry's checks: solve(st) fills n_records records -- the caller's, or local ones
// where stats_out is NULL (~25 KB each: not on the stack); every record gets the group's wall time and record 0 stays in the
// context (stats_out may be &ctx->stats).  After a failing solve the stream is drained: nothing in flight when the arena is reset.
template <class SolveFn>
static int ofx_group_records(ofx_ctx *ctx, int n_records, ofx_stats *stats_out, SolveFn solve)
{
    const double t0 = ofx_now_ms();
    std::vector<ofx_stats> local(stats_out ? 0 : n_records);
    ofx_stats *st = stats_out ? stats_out : local.data();
    const int s = solve(st);
    if (s != OFX_OK) (void) hipStreamSynchronize(ctx->stream);
    const double ms = ofx_now_ms() - t0;
    for (int g = 0; g < n_records; g++) st[g].total_ms = ms;
    if (st != &ctx->stats) ctx->stats = st[0];
    return s;
}
