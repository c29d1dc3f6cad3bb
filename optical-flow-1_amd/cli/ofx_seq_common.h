/* ofx_seq_common.h -- what tvl1flow_seq, horn_schunck_seq and brox_seq share: the frames of a video read into host planes of the
 * context's storage precision, one payload per step, a chain entry called on them, the payloads written as out_prefix0000.flo, ...
 * The chain entries stage host arrays themselves (include/ofx.h). */
#ifndef OFX_SEQ_COMMON_H
#define OFX_SEQ_COMMON_H

#include <unistd.h>

#include "ofx_cli_common.h"

/* argv[first ..]: the frames.  Returns the planes (NULL after a message) and their size. */
static double **seq_read_frames(int argc, char *argv[], int first, int *nx, int *ny)
{
    const int n_frames = argc - first;
    double **I = (double **) calloc((size_t) n_frames, sizeof(double *));
    int ok = I != NULL;
    for (int t = 0; ok && t < n_frames; t++) {
        int w = 0, h = 0;
        I[t] = ofx_read_image_double(argv[first + t], &w, &h);
        if (!I[t]) {
            fprintf(stderr, "ERROR: could not read image from file \"%s\"\n", argv[first + t]);
            ok = 0;
        } else if (t && (w != *nx || h != *ny)) {
            fprintf(stderr, "ERROR: input images size mismatch %dx%d != %dx%d\n", *nx, *ny, w, h);
            ok = 0;
        }
        if (!t) { *nx = w; *ny = h; }
    }
    if (!ok && I) {
        for (int t = 0; t < n_frames; t++) free(I[t]);
        free(I);
        I = NULL;
    }
    return I;
}

/* chain(ctx, n_frames, frames, payloads, arg) solves the steps; returns the program's exit status */
typedef int (*seq_chain_fn)(ofx_ctx *ctx, int n_frames, const void *const *frames, void *const *payloads, void *arg);

static int seq_run(const char *program, const char *prefix, double **I, int n_frames, int nx, int ny, seq_chain_fn chain, void *arg)
{
    (void) cli_save_flow;                   /* the payloads arrive interleaved: ofx_write_flo directly */
    (void) cli_parse;
    const int steps = n_frames - 1;
    int rc = EXIT_SUCCESS;
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    cli_phase("wait_for_context");
    const size_t n = (size_t) nx * ny;
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
        int s = chain(ctx, n_frames, frames, payload, arg);
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
    cli_write_stats(ctx, program);
    ofx_ctx_destroy(ctx);
    return rc;
}

/* as tvl1flow: skip the HIP runtime's exit handlers unless OFX_FAST_EXIT=0 */
static int seq_exit(int rc)
{
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}

#endif
