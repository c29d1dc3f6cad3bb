// ofx_loop_plan.h -- the host's decisions in the iteration loops (ofx_loop.h) and their drivers: which launches a chunk holds, whether a
// loop ended inside a launch unit, which buffer of a rotation a unit reads, how tall the strips of a marching kernel are.  Pure
// functions on ints and nothing but the standard library; the pump takes its device actions as callables.  So a plain host compiler
// builds all of it (tests/loop_plan_driver.cpp prints the rules over grids and runs the pump against a scripted device).
#pragma once

#include <climits>

#ifndef OFX_MAX_GROUP
#define OFX_MAX_GROUP 16       // as ofx_internal.h
#endif

static inline int ofx_plan_cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- launch units ------------------------------------------------------------------------------------------------------------
// A launch unit = the iterations one launch runs: F of them, units start at multiples of F, the last unit of a loop is what is
// left of max_iter.

// iterations per unit of a loop whose solver fuses `fuse` (> 2) iterations per launch, else two (`pairs`), else one
static inline int ofx_loop_unit_size(bool pairs, int fuse) { return fuse > 2 ? fuse : (pairs ? 2 : 1); }
// iterations per poll: `chunk`, at least one, rounded up to whole units
static inline int ofx_loop_chunk(int chunk, int F) { return ofx_plan_cdiv(chunk < 1 ? 1 : chunk, F) * F; }

// The launches of a loop chunk by chunk.  next(launch) calls launch(k, cnt) for every unit of the next chunk (cnt < F only for
// the last unit before max_iter) until one returns a status other than 0; the chunk's poll covers iterations [first, launched).
struct OfxChunkSchedule {
    int max_iter, chunk, F, first = 0, launched = 0;
    OfxChunkSchedule(int max_iter_, int chunk_, int F_) : max_iter(max_iter_), chunk(ofx_loop_chunk(chunk_, F_)), F(F_) {}
    bool more() const { return launched < max_iter; }
    template <class LaunchFn> int next(LaunchFn launch)
    {
        first = launched;
        const int end = first + (max_iter - first < chunk ? max_iter - first : chunk);
        while (launched < end) {
            const int cnt = end - launched < F ? end - launched : F;
            if (const int s = launch(launched, cnt)) return s;
            launched += cnt;
        }
        return 0;
    }
};

// the unit that contains iteration n - 1 (n >= 1): its first iteration and its length
struct OfxUnit { int k0, cnt; };
static inline OfxUnit ofx_loop_unit_of(int n, int F, int max_iter)
{
    const int k0 = (n - 1) / F * F;
    return OfxUnit{k0, max_iter - k0 < F ? max_iter - k0 : F};
}
// a loop of n iterations ended INSIDE its unit: n is not the unit's last iteration (F = 2: n odd and not max_iter)
static inline bool ofx_loop_inside(int n, int F, int max_iter)
{
    if (F <= 1 || n <= 0) return false;
    const OfxUnit u = ofx_loop_unit_of(n, F, max_iter);
    return n - u.k0 != u.cnt;
}
// a cursor loop's units are device state: k0 and ucnt come with the poll
static inline bool ofx_loop_inside_cursor(int n, int k0, int ucnt) { return n > 0 && n - k0 < ucnt; }
// F = 2 and a caller that asked (`wants`): the launch in which the loop ended stored the state between its two iterations --
// it had predicted the stop (apred), or it was the loop's very first launch and the pair's bit of amask0 told it to
static inline bool ofx_loop_took_alt(bool inside, int F, bool wants, int apred, int n, bool amask0_bit)
{
    return inside && F == 2 && wants && (apred || (n == 1 && amask0_bit));
}
// what the re-run of a unit of K gets for a loop that ended at n inside it: the unit's number and its first n - j K iterations
struct OfxRedoEntry { int unit, count; };
static inline OfxRedoEntry ofx_loop_redo_entry(int n, int K)
{
    const int j = (n - 1) / K;
    return OfxRedoEntry{j, n - j * K};
}
// units a loop of n iterations ran: the result is the output of the last of them
static inline int ofx_loop_units(int n, int K) { return (n + K - 1) / K; }

// ---- the pump ----------------------------------------------------------------------------------------------------------------
// Keeps up to max_out polls outstanding: while more() and a place is free, enqueue(i) enqueues a chunk and its poll into place i
// (0 | 1); then read(i, &all) waits for the oldest one and says whether every problem is done.  Ends with *stopped = true on the
// first poll that says so -- a poll still in flight then covers launches that are no-ops (their stopping test already fails); it is
// not drained, stream order keeps it ahead of whatever is enqueued next --, with *stopped = false when nothing is left to enqueue
// or to read, or with the first status other than 0 of a callable.
template <class MoreFn, class EnqueueFn, class ReadFn>
static inline int ofx_loop_pump(int max_out, MoreFn more, EnqueueFn enqueue, ReadFn read, bool *stopped)
{
    *stopped = false;
    for (int head = 0, tail = 0;;) {
        for (; more() && head - tail < max_out; head++)
            if (const int s = enqueue(head & 1)) return s;
        if (tail == head) return 0;
        bool all = false;
        if (const int s = read(tail++ & 1, &all)) return s;
        if (all) {
            *stopped = true;
            return 0;
        }
    }
}

// ---- the launch-unit table ---------------------------------------------------------------------------------------------------
// Unit j of pair g reads buffer (b_g + j) % MOD of a rotation and writes (b_g + j + 1) % MOD, b_g = where the pair starts.  MOD = 3
// (TV-L1: the third buffer keeps a unit's input intact, or takes the state between the two iterations of a fused pair), two bits
// per pair in a packed code; MOD = 2 (the SOR tiles' ping-pong), one bit.  `nit` packs four bits of iteration count per pair.
static_assert(OFX_MAX_GROUP * 4 <= 64 && OFX_MAX_GROUP * 2 <= 32,
              "the kernels take 4 bits of iteration count (`nit`, 64 bits) and up to 2 bits of buffer index (`incode`, 32 bits) per pair");
template <unsigned MOD> struct OfxUnitTable {
    static_assert(MOD == 2 || MOD == 3, "a ping-pong or a rotation of three");
    static constexpr int BITS = MOD == 3 ? 2 : 1;
    struct Redo {
        unsigned incode = 0, runmask = 0;
        unsigned long long nit = 0;
    };
    int G;
    unsigned b0[OFX_MAX_GROUP];
    // cur: the packed code of the buffers the pairs start in
    OfxUnitTable(int G_, unsigned cur) : G(G_)
    {
        for (int g = 0; g < G; g++) b0[g] = (cur >> (BITS * g)) & ((1u << BITS) - 1u);
    }
    unsigned all() const { return G >= 32 ? 0xFFFFFFFFu : (1u << G) - 1u; }                 // runmask: every pair
    unsigned at(int g, unsigned j) const { return ((b0[g] + j) % MOD) << (BITS * g); }
    unsigned code(unsigned j) const                                                         // all pairs at unit j
    {
        unsigned c = 0;
        for (int g = 0; g < G; g++) c |= at(g, j);
        return c;
    }
    unsigned long long nit(int cnt) const                                                   // all pairs run cnt iterations
    {
        unsigned long long v = 0;
        for (int g = 0; g < G; g++) v |= (unsigned long long) cnt << (4 * g);
        return v;
    }
    void add(Redo &r, int g, int unit, int count) const
    {
        r.runmask |= 1u << g;
        r.incode |= at(g, (unsigned) unit);
        r.nit |= (unsigned long long) count << (4 * g);
    }
    // fixed units of K: k_of[g] = n_g - 1 for the pairs whose loop ended inside a unit, -1 for the others (ofx_run_loop_group)
    Redo redo(const int *k_of, int K) const
    {
        Redo r;
        for (int g = 0; g < G; g++) {
            if (k_of[g] < 0) continue;
            const OfxRedoEntry e = ofx_loop_redo_entry(k_of[g] + 1, K);
            add(r, g, e.unit, e.count);
        }
        return r;
    }
    // cursor loops: n_of[g] = n_g or -1, the unit and its first iteration as the device logged them (ofx_run_loop_cursor)
    Redo redo(const int *n_of, const int *k0_of, const int *u_of) const
    {
        Redo r;
        for (int g = 0; g < G; g++)
            if (n_of[g] >= 0) add(r, g, u_of[g], n_of[g] - k0_of[g]);
        return r;
    }
    // where the results are after units[g] units; took_alt[g] (two-iteration kernel): in the buffer behind instead, where the
    // stopping launch stored its intermediate state
    unsigned result(const int *units, const int *took_alt = nullptr) const
    {
        unsigned c = 0;
        for (int g = 0; g < G; g++) c |= at(g, (unsigned) units[g] + (took_alt && took_alt[g] ? 1u : 0u));
        return c;
    }
};

// ---- strip heights of the marching TV-L1 kernels -------------------------------------------------------------------------------
// A wave of a strip of r rows executes r + depth marching steps.  The chip holds `waves` waves per SIMD on 1024 SIMDs at once,
// so a launch of W waves takes k = ceil(W / slots) rounds of about r + depth step times: the best strip height is the SMALLEST r
// (up to rmax) whose wave count still fits k rounds exactly, minimised over k = 1 .. 4 (1080p, two iterations: r = 12 -> 32 x 90 =
// 2880 waves, one round; r = 8 -> 4320 waves = 1.4 rounds is 9 % slower).  Very short strips multiply the halo work: `floor` rows
// as long as that still leaves >= 512 waves.  A lockstep group of G pairs is G times the waves of one pair.
// concurrency > 1, several contexts share the device: other pairs' waves fill this launch's partial rounds, so what counts is the
// total work ~ ceil(W / rows_slots) * (r + depth) over the candidates up to cand_max -- taller strips, less halo recomputation
// (measured with 4 pairs in flight: + 8 % job throughput over the single-pair choice).
struct OfxStripModel {
    int strip_out;          // output columns of a strip
    int depth;              // marching steps of a strip beyond its rows
    int waves;              // resident waves per SIMD
    int rmax, floor;
    const int *cand;        // strip heights tried when contexts share the device, ascending
    int ncand;
};
// the two-iteration kernel: r + 3 marching steps + ~2 of start-up; the kernels of N = 3 | 4 iterations: r + 2 N + 1
static inline OfxStripModel ofx_strip_model2(int strip_out, int waves)
{
    static const int cand[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 20, 24};
    return OfxStripModel{strip_out, 5, waves, /* rmax */ 24, /* floor */ 3, cand, (int) (sizeof(cand) / sizeof(cand[0]))};
}
static inline OfxStripModel ofx_strip_model3(int N, int strip_out, int waves)
{
    static const int cand[] = {2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32, 36, 40, 48, 54, 64, 72, 80, 96};
    return OfxStripModel{strip_out, 2 * N + 1, waves, /* rmax */ 32, /* floor */ 4, cand, (int) (sizeof(cand) / sizeof(cand[0]))};
}
static inline int ofx_pick_strip_rows(const OfxStripModel &M, int nx, int ny, int G, int concurrency, int rows_slots, int cand_max)
{
    const long strips_pad = (long) ofx_plan_cdiv(ofx_plan_cdiv(nx, M.strip_out), 4) * 4 * G;
    int best = M.rmax;
    long best_cost = -1;
    if (concurrency > 1) {
        const long slots = rows_slots > 0 ? rows_slots : 1024;
        for (int i = 0; i < M.ncand && M.cand[i] <= cand_max; i++) {
            const int r = M.cand[i];
            const long cost = (strips_pad * ofx_plan_cdiv(ny, r) + slots - 1) / slots * (r + M.depth);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = r; }
        }
        return best;
    }
    const long slots = 1024L * M.waves;
    for (int k = 1; k <= 4; k++) {
        for (int r = 1; r <= M.rmax; r++) {
            if (strips_pad * ofx_plan_cdiv(ny, r) > k * slots) continue;
            const long cost = (long) k * (r + M.depth);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = r; }
            break;
        }
    }
    if (best < M.floor && strips_pad * ofx_plan_cdiv(ny, M.floor) >= 512) best = M.floor;
    return best;
}
