/* horn_schunck_seq -- pyramidal Horn-Schunck along a video (ofx_hs_sequence_group_dev): the flow of every pair of consecutive
 * frames, the first pair solved cold on nscales_first scales, every later pair started from the flow of the pair before it on
 * nscales_next scales.
 *
 *   horn_schunck_seq out_prefix nscales_first nscales_next frame0 frame1 [frame2 ...]
 *
 * writes out_prefix0000.flo (frame0 -> frame1), out_prefix0001.flo, ...  The other parameters are horn_schunck_pyramidal's
 * defaults (alpha 7, zoom factor 0.5, 10 warps, TOL 1e-4, maxiter 150), and both scale counts fall under its rule that the
 * smallest pyramid image is not below ~16 pixels across the diagonal.  OFX_PRECISION, OFX_SOR_TOLERANCE and OFX_STATS (the
 * record of the last step) as horn_schunck_pyramidal reads them.
 */
#include <math.h>

#include "ofx_seq_common.h"

typedef struct { int nx, ny, nscales_first, nscales_next; } hs_seq_arg;

static int hs_chain(ofx_ctx *ctx, int n_frames, const void *const *frames, void *const *payloads, void *arg)
{
    const hs_seq_arg *a = (const hs_seq_arg *) arg;
    const double alpha = 7, zfactor = 0.5, TOL = 0.0001;
    const int warps = 10, maxiter = 150;
    return ofx_hs_sequence_group_dev(ctx, 1, n_frames, frames, payloads, a->nx, a->ny, alpha, a->nscales_first, a->nscales_next, zfactor,
                                     warps, warps, TOL, maxiter, NULL);
}

int main(int argc, char *argv[])
{
    if (argc < 6) {
        fprintf(stderr, "Usage: %s out_prefix nscales_first nscales_next frame0 frame1 [frame2 ...]\n", *argv);
        return EXIT_FAILURE;
    }
    cli_phase(NULL);
    hs_seq_arg a = {0, 0, atoi(argv[2]), atoi(argv[3])};
    if (a.nscales_first <= 0) a.nscales_first = 10;         /* horn_schunck_pyramidal's default */
    if (a.nscales_next <= 0) a.nscales_next = 2;
    const int n_frames = argc - 4;
    double **I = seq_read_frames(argc, argv, 4, &a.nx, &a.ny);
    if (!I) return EXIT_FAILURE;
    cli_phase("read_images");
    const double N = 1 + log(hypot(a.nx, a.ny) / 16) / log(1 / 0.5);    /* as horn_schunck_pyramidal */
    if (N < a.nscales_first) a.nscales_first = (int) N;
    if (N < a.nscales_next) a.nscales_next = (int) N;
    const int rc = seq_run(argv[0], argv[1], I, n_frames, a.nx, a.ny, hs_chain, &a);
    for (int t = 0; t < n_frames; t++) free(I[t]);
    free(I);
    return seq_exit(rc);
}
