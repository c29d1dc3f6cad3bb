/* flow_color -- a flow field as a picture: Middlebury's colour wheel (ofx_flow_encode_dev, OFX_ENC_WHEEL_RGB8), the coding of every
 * paper figure: hue is the direction, saturation the length, white is no motion.
 *
 *   flow_color in.flo out.ppm|png [maxrad] [occ.png|pgm]
 *
 * maxrad: the length in pixels that is drawn fully saturated; 0 (the default): the longest vector of the field itself.  occ: a map
 * as flow_consistency writes them, 0 = valid; flagged pixels, NaN and Inf vectors and vectors beyond 1e9 (Middlebury's unknown
 * marker) are drawn black.  The picture is written as a binary PPM (P6) whatever the name says.  Files that cannot be read or
 * differ in size are an error before the GPU is touched.
 */
#include <string.h>
#include <unistd.h>

#include "ofx_cli_common.h"

static int usage(const char *prog)
{
    fprintf(stderr, "Usage: %s in.flo out.ppm|png [maxrad] [occ.png|pgm]\n", prog);
    return EXIT_FAILURE;
}

int main(int argc, char *argv[])
{
    (void) cli_save_flow;
    if (argc < 3 || argc > 5) return usage(*argv);
    const char *in = argv[1], *out = argv[2], *occ_name = argc > 4 ? argv[4] : NULL;
    const double maxrad = argc > 3 ? atof(argv[3]) : 0.0;
    int nx = 0, ny = 0;
    float *flo = ofx_read_flo(in, &nx, &ny);
    if (!flo) { fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", in); return EXIT_FAILURE; }
    const size_t n = (size_t) nx * ny;
    unsigned char *occ = NULL;
    if (occ_name) {
        int w = 0, h = 0;
        double *m = ofx_read_image_double(occ_name, &w, &h);
        if (!m || w != nx || h != ny) {
            if (!m) fprintf(stderr, "ERROR: could not read a map from file \"%s\"\n", occ_name);
            else fprintf(stderr, "ERROR: map size mismatch %dx%d != %dx%d\n", w, h, nx, ny);
            return EXIT_FAILURE;
        }
        occ = (unsigned char *) malloc(n);
        if (!occ) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
        for (size_t i = 0; i < n; i++) occ[i] = m[i] != 0.0 ? 255 : 0;
        free(m);
    }
    unsigned char *rgb = (unsigned char *) malloc(3 * n);
    if (!rgb) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    const void *pf = flo, *po = occ;
    void *pd = rgb;
    int rc = EXIT_SUCCESS;
    int s = ofx_flow_encode_dev(ctx, 1, &pf, occ ? &po : NULL, OFX_ENC_WHEEL_RGB8, maxrad, &pd, nx, ny);   /* host memory: staged */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    }
    if (rc == EXIT_SUCCESS && ofx_write_bytes_image(out, rgb, nx, ny, 3)) {
        fprintf(stderr, "ERROR: cannot write \"%s\"\n", out);
        rc = EXIT_FAILURE;
    }
    free(flo); free(occ); free(rgb);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
