// ofx_group_plan.h -- how many items (pairs, triples, sequences) a lockstep group of a batch holds (by count and by memory), how many bytes a frame spans
// and which pointers a step of a video chain gets.  Pure functions on ints and pointer tables and nothing but the standard
// library, so a plain host compiler builds them (tests/group_plan_driver.cpp and tests/pair_plan_driver.cpp print them over grids).
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

// option "lockstep" where it is set, clamped to the largest group the entry allows; else dflt
static inline int ofx_plan_lockstep(int lockstep, int max_group, int dflt)
{
    return lockstep > 0 ? std::min(lockstep, max_group) : dflt;
}

// The batch is spread over as few rounds as groups of `cap` permit -- every context gets one group per round -- and the groups
// are evened out: 20 items on 4 contexts = 4 groups of 5, not 5 groups of 4 with one context working alone at the end.
static inline int ofx_plan_even_rounds(int n_items, int n_ctx, int cap)
{
    if (n_items <= 1) return 1;
    const int rounds = (n_items + n_ctx * cap - 1) / (n_ctx * cap);
    return std::max(1, (n_items + n_ctx * rounds - 1) / (n_ctx * rounds));
}

// no group larger than leaves every context one: G against the items per context
static inline int ofx_plan_cap_per_ctx(int G, int n_items, int n_ctx)
{
    return std::min(G, (n_items + n_ctx - 1) / n_ctx);
}

// Groups whose memory depends on what they hold: the largest G' <= G for which every group of a batch of n_items cut into groups
// of G' consecutive items (the last one shorter) fits the budget, 0 if not even groups of one do.  distinct(first, cnt) = what a
// group's memory depends on besides its count (TV-L1 with occlusions: its number of distinct planes), bytes(cnt, distinct) = that
// memory.  *need = the largest group's bytes at the returned G' (at G' = 1 where 0 is returned).
template <class DistinctFn, class BytesFn>
static inline int ofx_plan_fit_groups(int G, int n_items, double budget, DistinctFn distinct, BytesFn bytes, double *need)
{
    for (*need = 0.0; G >= 1; G--) {
        *need = 0.0;
        for (int first = 0; first < n_items; first += G) {
            const int cnt = std::min(G, n_items - first);
            *need = std::max(*need, (double) bytes(cnt, distinct(first, cnt)));
        }
        if (*need <= budget) break;
    }
    return std::max(G, 0);
}

// A frame's bytes as they lie: ny rows of nx elements of elem_bytes bytes, `pitch` bytes from one row's start to the next's --
// from its first row's start to its last row's end; pitch = 0 (or an empty frame): the rows lie back to back.
static inline size_t ofx_frame_span(int nx, int ny, size_t pitch, size_t elem_bytes)
{
    return pitch && nx > 0 && ny > 0 ? (size_t) (ny - 1) * pitch + (size_t) nx * elem_bytes : (size_t) nx * ny * elem_bytes;
}

// The video chain of n_seq sequences of n_frames frames (include/ofx.h): step t solves the pairs (F[q][t], F[q][t + 1]) of all
// sequences as one lockstep group through step(t, a, b, init, out, st), from the payloads of step t - 1 where there is one (init
// is NULL at t = 0); st = n_seq records of type Rec, record q of step t copied to stats_out[q * steps + t] (NULL: nowhere).
// Every step is a group entry on the context's stream, so the start of step t is read after step t - 1 has written it and never
// leaves the device.  The first step that returns a status other than 0 ends the walk with that status.
template <class Rec, class StepFn>
static int ofx_chain_walk(int n_seq, int n_frames, const void *const *dF, void *const *d_flo, Rec *stats_out, StepFn step)
{
    const int steps = n_frames - 1;
    std::vector<Rec> st(n_seq);
    std::vector<const void *> a(n_seq), b(n_seq), init(n_seq);
    std::vector<void *> out(n_seq);
    for (int t = 0; t < steps; t++) {
        for (int q = 0; q < n_seq; q++) {
            a[q] = dF[(size_t) q * n_frames + t];
            b[q] = dF[(size_t) q * n_frames + t + 1];
            init[q] = t ? d_flo[(size_t) q * steps + t - 1] : nullptr;
            out[q] = d_flo[(size_t) q * steps + t];
        }
        const int s = step(t, a.data(), b.data(), t ? init.data() : nullptr, out.data(), st.data());
        if (s) return s;
        for (int q = 0; stats_out && q < n_seq; q++) stats_out[(size_t) q * steps + t] = st[q];
    }
    return 0;
}
