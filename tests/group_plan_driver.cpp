// Prints the three grouping rules of csrc/ofx_group_plan.h over a grid, one line per point, for tests/test_group_plan.py.
// Plain host C++: no GPU, no library.
#include "ofx_group_plan.h"

#include <cstdio>

int main()
{
    const int max_group = 16;
    for (int n = 0; n <= 70; n++)
        for (int c = 1; c <= 5; c++)
            for (int k = 1; k <= max_group; k++) {
                std::printf("even_rounds %d %d %d %d\n", n, c, k, ofx_plan_even_rounds(n, c, k));
                std::printf("cap_per_ctx %d %d %d %d\n", k, n, c, ofx_plan_cap_per_ctx(k, n, c));
            }
    for (int l = -1; l <= 40; l++)
        for (int d = 1; d <= max_group; d += 5) std::printf("lockstep %d %d %d %d\n", l, max_group, d, ofx_plan_lockstep(l, max_group, d));
    return 0;
}
