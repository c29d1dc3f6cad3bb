/* brox_seq -- Brox's spatial method along a video (ofx_brox_sequence_group_dev): the flow of every pair of consecutive frames,
 * the first pair solved cold on nscales_first scales, every later pair started from the flow of the pair before it on
 * nscales_next scales.
 *
 *   brox_seq out_prefix nscales_first nscales_next frame0 frame1 [frame2 ...]
 *
 * writes out_prefix0000.flo (frame0 -> frame1), out_prefix0001.flo, ...  The other parameters are brox_spatial's defaults
 * (alpha 50, gamma 10, zoom factor 0.5, TOL 1e-4, 1 inner and 15 outer iterations), and both scale counts fall under its rule:
 * the smaller side of the smallest pyramid image is not below ~16 pixels, N truncated before the comparison.  OFX_PRECISION,
 * OFX_SOR_TOLERANCE and OFX_STATS (the record of the last step) as brox_spatial reads them.  Unlike brox_spatial, which copies
 * the reference's exit status 0, a failure is reported in the exit status.
 */
#include <math.h>

#include "ofx_seq_common.h"

typedef struct { int nx, ny, nscales_first, nscales_next; } brox_seq_arg;

static int brox_chain(ofx_ctx *ctx, int n_frames, const void *const *frames, void *const *payloads, void *arg)
{
    const brox_seq_arg *a = (const brox_seq_arg *) arg;
    const double alpha = 50, gamma = 10, nu = 0.5, TOL = 0.0001;
    const int inner = 1, outer = 15;
    return ofx_brox_sequence_group_dev(ctx, 1, n_frames, frames, payloads, a->nx, a->ny, alpha, gamma, a->nscales_first, a->nscales_next,
                                       nu, TOL, inner, outer, outer, NULL);
}

int main(int argc, char *argv[])
{
    if (argc < 6) {
        fprintf(stderr, "Usage: %s out_prefix nscales_first nscales_next frame0 frame1 [frame2 ...]\n", *argv);
        return EXIT_FAILURE;
    }
    cli_phase(NULL);
    brox_seq_arg a = {0, 0, atoi(argv[2]), atoi(argv[3])};
    if (a.nscales_first <= 0) a.nscales_first = 10;         /* brox_spatial's default */
    if (a.nscales_next <= 0) a.nscales_next = 2;
    const int n_frames = argc - 4;
    double **I = seq_read_frames(argc, argv, 4, &a.nx, &a.ny);
    if (!I) return EXIT_FAILURE;
    cli_phase("read_images");
    /* as brox_spatial: min(nx, ny), not the diagonal, and N truncated before it is compared */
    const double N = 1 + log((a.nx < a.ny ? a.nx : a.ny) / 16.) / log(1. / 0.5);
    if ((int) N < a.nscales_first) a.nscales_first = (int) N;
    if ((int) N < a.nscales_next) a.nscales_next = (int) N;
    const int rc = seq_run(argv[0], argv[1], I, n_frames, a.nx, a.ny, brox_chain, &a);
    for (int t = 0; t < n_frames; t++) free(I[t]);
    free(I);
    return seq_exit(rc);
}
