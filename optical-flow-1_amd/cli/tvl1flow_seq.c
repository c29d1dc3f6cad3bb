/* tvl1flow_seq -- TV-L1 along a video (ofx_tvl1_sequence_group_dev): the flow of every pair of consecutive frames, the first
 * pair solved cold on nscales_first scales, every later pair started from the flow of the pair before it on nscales_next scales.
 *
 *   tvl1flow_seq out_prefix nscales_first nscales_next frame0 frame1 [frame2 ...]
 *
 * writes out_prefix0000.flo (frame0 -> frame1), out_prefix0001.flo, ...  The other parameters are tvl1flow's defaults (tau 0.25,
 * lambda 0.15, theta 0.3, zfactor 0.5, 5 warps, epsilon 0.01), and both scale counts fall under tvl1flow's rule that the smallest
 * pyramid image is not below ~16x16.  OFX_PRECISION, OFX_TOLERANCE and OFX_STATS (the record of the last step's first pair) as
 * tvl1flow reads them.
 */
#include <math.h>

#include "ofx_seq_common.h"

typedef struct { int nx, ny, nscales_first, nscales_next; } tvl1_seq_arg;

static int tvl1_chain(ofx_ctx *ctx, int n_frames, const void *const *frames, void *const *payloads, void *arg)
{
    const tvl1_seq_arg *a = (const tvl1_seq_arg *) arg;
    const double tau = 0.25, lambda = 0.15, theta = 0.3, zfactor = 0.5, epsilon = 0.01;
    const int nwarps = 5;
    return ofx_tvl1_sequence_group_dev(ctx, 1, n_frames, frames, payloads, a->nx, a->ny, tau, lambda, theta, a->nscales_first,
                                       a->nscales_next, zfactor, nwarps, epsilon, NULL);
}

int main(int argc, char *argv[])
{
    if (argc < 6) {
        fprintf(stderr, "Usage: %s out_prefix nscales_first nscales_next frame0 frame1 [frame2 ...]\n", *argv);
        return EXIT_FAILURE;
    }
    cli_phase(NULL);
    tvl1_seq_arg a = {0, 0, atoi(argv[2]), atoi(argv[3])};
    if (a.nscales_first <= 0) a.nscales_first = 100;        /* tvl1flow's default: as many as the size rule allows */
    if (a.nscales_next <= 0) a.nscales_next = 2;
    const int n_frames = argc - 4;
    double **I = seq_read_frames(argc, argv, 4, &a.nx, &a.ny);
    if (!I) return EXIT_FAILURE;
    cli_phase("read_images");
    const double N = 1 + log(hypot(a.nx, a.ny) / 16.0) / log(1 / 0.5);      /* as tvl1flow */
    if (N < a.nscales_first) a.nscales_first = (int) N;
    if (N < a.nscales_next) a.nscales_next = (int) N;
    const int rc = seq_run(argv[0], argv[1], I, n_frames, a.nx, a.ny, tvl1_chain, &a);
    for (int t = 0; t < n_frames; t++) free(I[t]);
    free(I);
    return seq_exit(rc);
}
