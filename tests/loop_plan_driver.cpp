// Prints the rules of csrc/ofx_loop_plan.h over grids, one line per point, for tests/test_loop_plan.py.  Plain host C++: no GPU, no
// library.  argv[1] = "loop": the chunk schedule, the unit of every stopping iteration, the took_alt rule and the redo entries;
// "pump": ofx_loop_pump over OfxChunkSchedule, wired as ofx_run_loop_group wires them, against a scripted device that completes
// polls in order and stops pair g at n_g; "units": OfxUnitTable for both rotations; "rows": the strip heights of the three
// parameter sets that ship (strip widths and waves per SIMD as ofx_tvl1.hip defines them).
#include "ofx_loop_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static const int FS[] = {1, 2, 3, 4, 6};

static void loop_rules()
{
    std::vector<int> maxes;
    for (int m = 1; m <= 24; m++) maxes.push_back(m);
    maxes.push_back(300);
    for (int max_iter : maxes)
        for (int F : FS) {
            for (int chunk = 1; chunk <= 13; chunk++) {
                OfxChunkSchedule s(max_iter, chunk, F);
                std::printf("sched %d %d %d :", max_iter, F, chunk);
                while (s.more()) {
                    s.next([&](int k, int cnt) { std::printf(" %d+%d", k, cnt); return 0; });
                    std::printf(" [%d,%d)", s.first, s.launched);
                }
                std::printf("\n");
            }
            for (int n = 1; n <= max_iter; n++) {
                const OfxUnit u = ofx_loop_unit_of(n, F, max_iter);
                const bool inside = ofx_loop_inside(n, F, max_iter);
                const OfxRedoEntry e = ofx_loop_redo_entry(n, F);
                std::printf("unit %d %d %d %d %d %d %d %d %d\n", max_iter, F, n, u.k0, u.cnt, inside ? 1 : 0, e.unit, e.count,
                            ofx_loop_units(n, F));
                for (int bits = 0; bits < 8; bits++)
                    std::printf("alt %d %d %d %d %d %d %d\n", max_iter, F, n, bits & 1, (bits >> 1) & 1, (bits >> 2) & 1,
                                ofx_loop_took_alt(inside, F, bits & 1, (bits >> 1) & 1, n, (bits >> 2) & 1) ? 1 : 0);
            }
        }
}

// one scripted loop: the trace of what the host did.  n_of[g] = 0: pair g never stops before max_iter
static void pump_run(int max_iter, int F, int chunk, int max_out, int G, const int *n_of)
{
    struct Rec { int n, done; };
    OfxChunkSchedule s(max_iter, chunk, F);
    Rec rec[2][OFX_MAX_GROUP], fin[OFX_MAX_GROUP];
    std::string tr;
    auto enqueue = [&](int i) -> int {
        s.next([&](int k, int cnt) { tr += " L" + std::to_string(k) + "+" + std::to_string(cnt); return 0; });
        tr += " P" + std::to_string(s.first) + "," + std::to_string(s.launched);
        for (int g = 0; g < G; g++) {                       // what k_loop_finalize publishes for iterations [.., launched)
            const int stop = n_of[g] > 0 && n_of[g] <= s.launched ? n_of[g] : 0;
            rec[i][g] = Rec{stop ? stop : s.launched, stop || s.launched >= max_iter};
        }
        return 0;
    };
    auto read = [&](int i, bool *all) -> int {
        *all = true;
        for (int g = 0; g < G; g++) {
            fin[g] = rec[i][g];
            *all = *all && fin[g].done;
        }
        tr += *all ? " R1" : " R0";
        return 0;
    };
    bool stopped = false;
    const int st = ofx_loop_pump(max_out, [&] { return s.more(); }, enqueue, read, &stopped);
    std::printf("pump %d %d %d %d %d", max_iter, F, chunk, max_out, G);
    for (int g = 0; g < G; g++) std::printf(" %d", n_of[g]);
    std::printf(" : %d %d :%s :", st, stopped ? 1 : 0, tr.c_str());
    for (int g = 0; g < G; g++) std::printf(" %d/%d", fin[g].n, ofx_loop_inside(fin[g].n, F, max_iter) ? fin[g].n - 1 : -1);
    std::printf("\n");
}

static void pump()
{
    for (int max_iter : {1, 2, 5, 7, 12, 24})
        for (int F : FS)
            for (int chunk : {1, 4, 5, 13})
                for (int max_out = 1; max_out <= 2; max_out++)
                    for (int n = 0; n <= max_iter; n++) {
                        pump_run(max_iter, F, chunk, max_out, 1, &n);
                        const int three[3] = {n, n ? (2 * n) % max_iter + 1 : 1, (n + F + 1) % (max_iter + 1)};
                        pump_run(max_iter, F, chunk, max_out, 3, three);
                    }
}

template <unsigned MOD> static void units()
{
    const int bits = MOD == 3 ? 2 : 1;
    for (int G : {1, 2, 16})
        for (unsigned p = 0; p < MOD; p++)
            for (unsigned s = 0; s < MOD; s++) {            // pair g starts in buffer (p + s g) % MOD
                unsigned cur = 0;
                for (int g = 0; g < G; g++) cur |= ((p + s * g) % MOD) << (bits * g);
                const OfxUnitTable<MOD> t(G, cur);
                for (int j = 0; j < 8; j++) {
                    int ran[OFX_MAX_GROUP], alt[OFX_MAX_GROUP], k_of[OFX_MAX_GROUP], n_of[OFX_MAX_GROUP], k0_of[OFX_MAX_GROUP], u_of[OFX_MAX_GROUP];
                    for (int g = 0; g < G; g++) {
                        ran[g] = (j + g) % 8;
                        alt[g] = (g + j) & 1;
                        k_of[g] = g % 3 == 2 ? -1 : (5 * j + 3 * g) % 24;
                        u_of[g] = (j + 2 * g) % 8;
                        k0_of[g] = 3 * u_of[g];
                        n_of[g] = g % 4 == 1 ? -1 : k0_of[g] + 1 + (g + j) % 3;
                    }
                    std::printf("code %u %d %x %d %x %x %llx\n", MOD, G, cur, j, t.code((unsigned) j), t.all(), t.nit(j % 6 + 1));
                    std::printf("result %u %d %x %d %x %x\n", MOD, G, cur, j, t.result(ran), t.result(ran, alt));
                    for (int K : {2, 3, 4, 6}) {
                        const auto r = t.redo(k_of, K);
                        std::printf("redo %u %d %x %d %d %x %x %llx\n", MOD, G, cur, j, K, r.incode, r.runmask, r.nit);
                    }
                    const auto r = t.redo(n_of, k0_of, u_of);
                    std::printf("redoc %u %d %x %d %x %x %llx\n", MOD, G, cur, j, r.incode, r.runmask, r.nit);
                }
            }
}

static void rows()
{
    static const int dims[] = {2, 3, 55, 56, 57, 60, 61, 120, 135, 240, 270, 480, 540, 960, 1080, 1920, 2160, 3840};
    const OfxStripModel M[3] = {ofx_strip_model2(60, 3), ofx_strip_model3(3, 56, 3), ofx_strip_model3(4, 56, 3)};
    for (int m = 0; m < 3; m++)
        for (int nx : dims)
            for (int ny : dims)
                for (int G : {1, 2, 5, 16})
                    for (int conc : {1, 4})
                        for (int slots : {0, 512})
                            std::printf("rows %d %d %d %d %d %d %d\n", m + 2, nx, ny, G, conc, slots,
                                        ofx_pick_strip_rows(M[m], nx, ny, G, conc, slots, m ? 32 : INT_MAX));
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!std::strcmp(what, "loop")) loop_rules();
    else if (!std::strcmp(what, "pump")) pump();
    else if (!std::strcmp(what, "units")) { units<2>(); units<3>(); }
    else if (!std::strcmp(what, "rows")) rows();
    else return 2;
    return 0;
}
