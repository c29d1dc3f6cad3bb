/* tests/sor_level_shim.c -- the checker's Brox level solver with an initial flow, for tests/sor_warm_ref.py.
 *
 * oracle/ofx_oracle.c exports brox_spatial (the whole pyramid, from zero) and keeps brox_single_scale static.  The warm start's
 * restatement composes the pyramid itself and needs the level alone, so this translation unit includes the checker's source and
 * adds one wrapper.  It is a SECOND copy of the checker's process-global state (thread count, sweep order, tile size, wave
 * levels): whoever loads it sets those on it as well (orc_set_num_threads, orc_set_sor_order, orc_set_sor_tile,
 * orc_set_sor_wave_levels, all exported from here too).
 *
 * Built by tests/sor_warm_ref.py into tests/_build/ with the flags of oracle/Makefile. */
#include "../oracle/ofx_oracle.c"

/* One level of brox_spatial (ofx_oracle.c): u, v hold the start and receive the flow; `level` is the pyramid level the solve
 * stands for (it picks the sweep order under orc_set_sor_order(1): colour levels, wave levels, exact tail); iters receives
 * inner_iter * outer_iter sweep counts.  store_f32: the images and the incoming flow are rounded to float first, as
 * orc_hs_single_scale_mode rounds them.  The order and the level of the copy are restored afterwards. */
void sor_shim_brox_level(const double *I1, const double *I2, double *u, double *v, int nx, int ny, double alpha, double gamma,
                         double TOL, int inner_iter, int outer_iter, int level, int *iters, int store_f32)
{
    const int level_saved = g_sor_level;
    const int order = sor_order_enter_level(level);
    if (!store_f32) {
        brox_single_scale(I1, I2, u, v, nx, ny, alpha, gamma, TOL, inner_iter, outer_iter, orc_max_threads(), 0, iters, 0);
    } else {
        const size_t n = (size_t) nx * ny;
        double *A = dalloc(n), *B = dalloc(n);
        for (size_t i = 0; i < n; i++) { A[i] = rnd_f32(I1[i]); B[i] = rnd_f32(I2[i]); }
        round_f32(u, n);
        round_f32(v, n);
        brox_single_scale(A, B, u, v, nx, ny, alpha, gamma, TOL, inner_iter, outer_iter, orc_max_threads(), 0, iters, 1);
        free(A); free(B);
    }
    g_sor_order = order;
    g_sor_level = level_saved;
}
