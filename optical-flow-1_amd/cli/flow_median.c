/* flow_median -- the median filter of a .flo file (ofx_flow_median_dev), whichever solver wrote it: outliers removed, and with a
 * map the flagged vectors filled from their valid neighbours.
 *
 *   flow_median in.flo out.flo [wsize = 5] [occ map]
 *
 * wsize: 3, 5 or 7; each component of out.flo is the median of its wsize x wsize window, borders mirrored.  occ map: a
 * one-channel image as flow_consistency writes it (PGM or PNG), 0 = valid, anything else = flagged; only valid positions take
 * part, and a window without one leaves its vector as it is.  Files that cannot be read or differ in size are an error before
 * the GPU is touched; a wsize that the library refuses is its error.
 */
#include <unistd.h>

#include "ofx_cli_common.h"

int main(int argc, char *argv[])
{
    if (argc < 3) {
        fprintf(stderr, "Usage: %s in.flo out.flo [wsize = 5] [occ map]\n", *argv);
        return EXIT_FAILURE;
    }
    (void) cli_save_flow;
    const int wsize = argc > 3 ? atoi(argv[3]) : 5;
    if (!ofx_has_suffix(argv[2], ".flo")) {
        fprintf(stderr, "ERROR: output \"%s\": only the .flo format is supported\n", argv[2]);
        return EXIT_FAILURE;
    }
    int nx, ny;
    float *in = ofx_read_flo(argv[1], &nx, &ny);
    if (!in) {
        fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", argv[1]);
        return EXIT_FAILURE;
    }
    const size_t n = (size_t) nx * ny;
    unsigned char *occ = NULL;
    if (argc > 4) {
        int mx, my;
        double *m = ofx_read_image_double(argv[4], &mx, &my);
        if (!m || mx != nx || my != ny) {
            if (!m) fprintf(stderr, "ERROR: could not read a map from file \"%s\"\n", argv[4]);
            else fprintf(stderr, "ERROR: map size mismatch %dx%d != %dx%d\n", mx, my, nx, ny);
            free(m); free(in);
            return EXIT_FAILURE;
        }
        occ = (unsigned char *) malloc(n);
        if (occ) for (size_t i = 0; i < n; i++) occ[i] = m[i] != 0.0 ? 255 : 0;
        free(m);
    }
    float *out = (float *) malloc(sizeof(float) * 2 * n);
    if (!out || (argc > 4 && !occ)) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    int rc = EXIT_SUCCESS;
    const void *pi = in, *po = occ;
    void *pd = out;
    int s = ofx_flow_median_dev(ctx, 1, &pi, occ ? &po : NULL, &pd, nx, ny, wsize);                 /* host memory: staged by the entry */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    } else if (ofx_write_flo(argv[2], out, nx, ny)) {
        fprintf(stderr, "ERROR: cannot write \"%s\"\n", argv[2]);
        rc = EXIT_FAILURE;
    }
    free(out); free(occ); free(in);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
