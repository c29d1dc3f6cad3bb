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
#include <unistd.h>

#include "ofx_cli_common.h"

int main(int argc, char *argv[])
{
    if (argc < 6) {
        fprintf(stderr, "Usage: %s out_prefix nscales_first nscales_next frame0 frame1 [frame2 ...]\n", *argv);
        return EXIT_FAILURE;
    }
    cli_phase(NULL);
    (void) cli_save_flow;                   /* the payloads arrive interleaved: ofx_write_flo directly */
    (void) cli_parse;
    const char *prefix = argv[1];
    int nscales_first = atoi(argv[2]), nscales_next = atoi(argv[3]);
    const int n_frames = argc - 4, steps = n_frames - 1;
    const double tau = 0.25, lambda = 0.15, theta = 0.3, zfactor = 0.5, epsilon = 0.01;
    const int nwarps = 5;
    if (nscales_first <= 0) nscales_first = 100;            /* tvl1flow's default: as many as the size rule allows */
    if (nscales_next <= 0) nscales_next = 2;

    int nx = 0, ny = 0, rc = EXIT_SUCCESS;
    double **I = (double **) calloc((size_t) n_frames, sizeof(double *));
    if (!I) return EXIT_FAILURE;
    for (int t = 0; t < n_frames && rc == EXIT_SUCCESS; t++) {
        int w, h;
        I[t] = ofx_read_image_double(argv[4 + t], &w, &h);
        if (!I[t]) {
            fprintf(stderr, "ERROR: could not read image from file \"%s\"\n", argv[4 + t]);
            rc = EXIT_FAILURE;
        } else if (t && (w != nx || h != ny)) {
            fprintf(stderr, "ERROR: input images size mismatch %dx%d != %dx%d\n", nx, ny, w, h);
            rc = EXIT_FAILURE;
        }
        if (!t) { nx = w; ny = h; }
    }
    if (rc != EXIT_SUCCESS) {
        for (int t = 0; t < n_frames; t++) free(I[t]);
        free(I);
        return rc;
    }
    cli_phase("read_images");
    const double N = 1 + log(hypot(nx, ny) / 16.0) / log(1 / zfactor);      /* as tvl1flow */
    if (N < nscales_first) nscales_first = (int) N;
    if (N < nscales_next) nscales_next = (int) N;

    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    cli_phase("wait_for_context");
    const size_t n = (size_t) nx * ny;
    /* the entry reads frames of the context's storage precision and stages host memory itself */
    const void **frames = (const void **) calloc((size_t) n_frames, sizeof(void *));
    void **payload = (void **) calloc((size_t) steps, sizeof(void *));
    float *S = NULL, *flo = (float *) malloc(sizeof(float) * 2 * n * (size_t) steps);
    if (ofx_ctx_precision(ctx) == OFX_F32) S = (float *) malloc(sizeof(float) * n * (size_t) n_frames);
    if (!frames || !payload || !flo || (ofx_ctx_precision(ctx) == OFX_F32 && !S)) {
        fprintf(stderr, "ERROR: out of memory\n");
        rc = EXIT_FAILURE;
    } else {
        for (int t = 0; t < n_frames; t++) {
            frames[t] = I[t];
            if (S) {
                for (size_t i = 0; i < n; i++) S[(size_t) t * n + i] = (float) I[t][i];
                frames[t] = S + (size_t) t * n;
            }
        }
        for (int t = 0; t < steps; t++) payload[t] = flo + 2 * n * (size_t) t;
        int s = ofx_tvl1_sequence_group_dev(ctx, 1, n_frames, frames, payload, nx, ny, tau, lambda, theta, nscales_first, nscales_next,
                                            zfactor, nwarps, epsilon, NULL);
        if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
        cli_phase("solve");
        if (s != OFX_OK) {
            fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
            rc = EXIT_FAILURE;
        }
        for (int t = 0; t < steps && rc == EXIT_SUCCESS; t++) {
            char name[4096];
            snprintf(name, sizeof(name), "%s%04d.flo", prefix, t);
            if (ofx_write_flo(name, flo + 2 * n * (size_t) t, nx, ny)) {
                fprintf(stderr, "ERROR: cannot write \"%s\"\n", name);
                rc = EXIT_FAILURE;
            }
        }
        cli_phase("write_flo");
    }
    free(flo); free(S); free(payload); free(frames);
    for (int t = 0; t < n_frames; t++) free(I[t]);
    free(I);
    cli_write_stats(ctx, argv[0]);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");          /* as tvl1flow: skip the HIP runtime's exit handlers unless OFX_FAST_EXIT=0 */
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
