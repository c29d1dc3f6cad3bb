/* structure_texture -- the texture part of a frame (ofx_structure_texture_dev), the preprocessing that makes a flow solve robust
 * against gain changes, exposure ramps and shadows (Wedel et al. 2009, section 3.1).
 *
 *   structure_texture in out.pfm [theta = 16  alpha = 0.95  n_iter = 100  [structure.pfm]]
 *
 * in: any image the front-ends read, taken as gray; out.pfm: T = f - alpha S as a one-channel PFM ("Pf": raw floats, first row
 * first), which every front-end reads; structure.pfm: S the same way.  The whole pipeline:
 *   structure_texture a.pgm a_t.pfm && structure_texture b.pgm b_t.pfm && tvl1flow a_t.pfm b_t.pfm out.flo
 * The floats are (float) of the library's doubles in either OFX_PRECISION.  OFX_STATS is accepted and ignored.
 */
#include <unistd.h>

#include "ofx_cli_common.h"

int main(int argc, char *argv[])
{
    if (argc < 3) {
        fprintf(stderr, "Usage: %s in out.pfm [theta = 16  alpha = 0.95  n_iter = 100  [structure.pfm]]\n", *argv);
        return EXIT_FAILURE;
    }
    (void) cli_save_flow;
    const double theta = argc > 3 ? atof(argv[3]) : 16.0, alpha = argc > 4 ? atof(argv[4]) : 0.95;
    const int n_iter = argc > 5 ? atoi(argv[5]) : 100;
    const char *sname = argc > 6 ? argv[6] : NULL;
    int nx, ny;
    double *img = ofx_read_image_double(argv[1], &nx, &ny);
    if (!img) {
        fprintf(stderr, "ERROR: could not read an image from file \"%s\"\n", argv[1]);
        return EXIT_FAILURE;
    }
    const size_t n = (size_t) nx * ny;
    /* the reader's samples are floats widened to double: the frame goes in as floats, exactly */
    float *f = (float *) malloc(n * sizeof(float));
    const char *p = getenv("OFX_PRECISION");
    const int f32 = p && (!strcmp(p, "f32") || !strcmp(p, "F32"));              /* cli_context's rule */
    const size_t el = f32 ? sizeof(float) : sizeof(double);
    void *tex = malloc(n * el), *str = sname ? malloc(n * el) : NULL;
    float *out = (float *) malloc(n * sizeof(float));
    if (!f || !tex || !out || (sname && !str)) {
        fprintf(stderr, "ERROR: out of memory\n");
        return EXIT_FAILURE;
    }
    for (size_t i = 0; i < n; i++) f[i] = (float) img[i];
    free(img);
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    int rc = EXIT_SUCCESS;
    const void *ps = f;
    void *pt = tex, *pstr = str;
    int s = ofx_set_option(ctx, "input", OFX_IN_F32);
    if (s == OFX_OK) s = ofx_structure_texture_dev(ctx, 1, &ps, &pt, sname ? &pstr : NULL, nx, ny, theta, alpha, n_iter);   /* host memory: staged by the entry */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    }
    for (int k = 0; rc == EXIT_SUCCESS && k < (sname ? 2 : 1); k++) {
        const void *res = k ? str : tex;
        const char *name = k ? sname : argv[2];
        for (size_t i = 0; i < n; i++) out[i] = f32 ? ((const float *) res)[i] : (float) ((const double *) res)[i];
        if (ofx_write_pfm(name, out, nx, ny)) {
            fprintf(stderr, "ERROR: cannot write \"%s\"\n", name);
            rc = EXIT_FAILURE;
        }
    }
    free(out); free(tex); free(str); free(f);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
