// ofx_group_plan.h -- how many items (pairs, triples, sequences) a lockstep group of a batch holds.  Pure functions on ints and
// nothing but the standard library, so a plain host compiler builds them (tests/group_plan_driver.cpp prints them over a grid).
#pragma once

#include <algorithm>

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
