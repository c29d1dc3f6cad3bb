// Prints the two HIP-free pieces of the pair-entry layer (csrc/ofx_group_plan.h) for tests/test_pair_plan.py: the bytes a frame
// spans over a grid, and what every step of a video chain is handed -- fake pointers (integers cast), a recording step function
// that fails at step k where k >= 0.  Plain host C++: no GPU, no library.
#include "ofx_group_plan.h"

#include <cstdint>
#include <cstdio>

static void *fake(long v) { return reinterpret_cast<void *>(static_cast<intptr_t>(v)); }
static long value(const void *p) { return static_cast<long>(reinterpret_cast<intptr_t>(p)); }

// line tags: "step": one pair of one step as the step function saw it (init = -1: the start table was NULL);
// "ret": the walk's status; "rec": one slot of stats_out after the walk (-1: never written)
static void walk(int n_seq, int n_frames, int k, bool with_stats)
{
    const int steps = n_frames - 1;
    std::vector<const void *> dF((size_t) n_seq * n_frames);
    std::vector<void *> d_flo((size_t) n_seq * steps);
    for (size_t i = 0; i < dF.size(); i++) dF[i] = fake(1000 + (long) i);
    for (size_t i = 0; i < d_flo.size(); i++) d_flo[i] = fake(5000 + (long) i);
    std::vector<int> stats((size_t) n_seq * steps, -1);
    const int s = ofx_chain_walk(n_seq, n_frames, dF.data(), d_flo.data(), with_stats ? stats.data() : (int *) nullptr,
                                 [&](int t, const void *const *a, const void *const *b, const void *const *init, void *const *out, int *st) {
                                     for (int q = 0; q < n_seq; q++) {
                                         std::printf("step %d %d %d %d %d %d %ld %ld %ld %ld\n", n_seq, n_frames, k, (int) with_stats, t, q,
                                                     value(a[q]), value(b[q]), init ? value(init[q]) : -1L, value(out[q]));
                                         st[q] = 100 * t + q;
                                     }
                                     return t == k ? 7 : 0;
                                 });
    std::printf("ret %d %d %d %d %d\n", n_seq, n_frames, k, (int) with_stats, s);
    for (size_t i = 0; with_stats && i < stats.size(); i++)
        std::printf("rec %d %d %d %d %d %d\n", n_seq, n_frames, k, (int) with_stats, (int) i, stats[i]);
}

int main()
{
    const int sizes[4] = {0, 1, 2, 7}, bytes[5] = {1, 2, 3, 4, 8};
    for (int nx : sizes)
        for (int ny : sizes)
            for (int b : bytes)
                for (int extra : {-1, 0, 5}) {                  // no pitch, the row's own bytes, five bytes of padding
                    const size_t pitch = extra < 0 ? 0 : (size_t) nx * b + extra;
                    std::printf("span %d %d %d %zu %zu\n", nx, ny, b, pitch, ofx_frame_span(nx, ny, pitch, (size_t) b));
                }
    const int cases[5][2] = {{1, 2}, {1, 3}, {3, 5}, {16, 2}, {16, 4}};
    for (const auto &c : cases) {
        std::vector<int> ks = {-1, 0};                          // no failure, the first step fails ...
        if (c[1] - 2 > 0) ks.push_back(c[1] - 2);               // ... the last step fails, where that is another step
        for (int k : ks)
            for (int with_stats = 0; with_stats < 2; with_stats++) walk(c[0], c[1], k, with_stats != 0);
    }
    return 0;
}
