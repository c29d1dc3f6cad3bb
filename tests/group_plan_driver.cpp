// Prints the grouping rules of csrc/ofx_group_plan.h over a grid, one line per point, for tests/test_group_plan.py.
// Plain host C++: no GPU, no library.  No argument: the three rules by count.  "occ_sequence": the group size the planner of the
// TV-L1-with-occlusions batches (ofx_occ.hip: cap per context, then ofx_plan_fit_groups) gives a sequence, whose group of cnt
// triples holds cnt + 2 distinct planes, under a memory rule of the library's form in whole bytes and a budget chosen so that
// argv[2] triples fit and one more does not.
#include "ofx_group_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

// OccDevMem's rule without its 5 %, on 64 x 48 with two levels: per level D planes and 3 G of results, 2 D + 27 G full-size
// planes, 13 G hyperplane-major ones of (2 (ny - 1) + nx) ny doubles
static double occ_bytes(int G, int D)
{
    const double level_px = 64 * 48 + 32 * 24, full = 64 * 48, skew = (2 * 47 + 64) * 48;
    return 8.0 * ((D + 3.0 * G) * level_px + (2.0 * D + 27.0 * G) * full + 13.0 * G * skew);
}

int main(int argc, char **argv)
{
    const int max_group = 16;
    if (argc > 2 && !std::strcmp(argv[1], "occ_sequence")) {
        const int fits = std::atoi(argv[2]);
        const double budget = fits ? occ_bytes(fits, fits + 2) : 0.5 * occ_bytes(1, 3);
        for (int n = 1; n <= 200; n++)
            for (int c = 1; c <= 4; c++)
                for (int l : {0, 1, 4, 16, 99}) {
                    double need;
                    const int cap = ofx_plan_cap_per_ctx(ofx_plan_lockstep(l, max_group, max_group), n, c);
                    const int G = ofx_plan_fit_groups(cap, n, budget, [](int, int cnt) { return cnt + 2; }, occ_bytes, &need);
                    std::printf("occ_sequence %d %d %d %d %.17g\n", n, c, l, G, need);
                }
        return 0;
    }
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
