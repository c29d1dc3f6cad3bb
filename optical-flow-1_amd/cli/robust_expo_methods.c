/* robust_expo_methods -- front-end of the colour method.  The reference's src/robust_expo_methods_main.cpp is an empty
 * file; the program's boundary is the IPOL original's (3rdparty/ipoldfmethods_20160307/main.cpp):
 *
 *   robust_expo_methods I1 I2 [out_file processors method_type alpha gamma lambda nscales zoom_factor TOL
 *                              inner_iter outer_iter verbose]
 *
 * The images keep their channels (PGM / Pf: 1, PPM / PF: 3, PNG: 1..4); both must have the same size and channel count.
 * `processors` is accepted and ignored.  The parameter line goes to stdout whether or not `verbose` is set (:133-137).
 * The original keeps alpha, gamma, lambda, zoom_factor, TOL and the scale bound N in `float`; here they are double, as in the
 * other front-ends (so the default lambda is 0.2, not 0.2f, and for a zoom factor whose N lands within a float's rounding of an
 * integer the scale count can differ by one from the original's).  Images with min(nx, ny) < 16 give N < 1 and so nscales <= 0:
 * the solver refuses that (OFX_ERR_ARG), and the run ends with its message.
 * Unlike the original, which always returns 0, unreadable or mismatched images and a failed solve end with EXIT_FAILURE.
 */
#include <math.h>

#include "ofx_cli_common.h"

/* main.cpp:21-31 (defaults), :103-112 (ranges, silent); method_type's upper end is checked below */
static const cli_opt OPTS[] = {
    {"out_file",    CLI_TEXT, 0,      "flow.flo", CLI_ANY, 0, NULL},
    {"processors",  CLI_INT,  1,      NULL, CLI_ANY, 0, NULL},
    {"method_type", CLI_INT,  1,      NULL, CLI_LE0, 0, NULL},
    {"alpha",       CLI_REAL, 50,     NULL, CLI_LE0, 0, NULL},
    {"gamma",       CLI_REAL, 10,     NULL, CLI_LT0, 0, NULL},
    {"lambda",      CLI_REAL, 0.2,    NULL, CLI_LT0, 0, NULL},
    {"nscales",     CLI_INT,  10,     NULL, CLI_LE0, 0, NULL},
    {"zoom_factor", CLI_REAL, 0.5,    NULL, CLI_LE0 | CLI_GE1, 0, NULL},
    {"TOL",         CLI_REAL, 0.0001, NULL, CLI_LE0, 0, NULL},
    {"inner_iter",  CLI_INT,  1,      NULL, CLI_LE0, 0, NULL},
    {"outer_iter",  CLI_INT,  15,     NULL, CLI_LE0, 0, NULL},
    {"verbose",     CLI_INT,  0,      NULL, CLI_ANY, 0, NULL},
};
enum { O_OUT, O_NPROC, O_METHOD, O_ALPHA, O_GAMMA, O_LAMBDA, O_NSCALES, O_ZFACTOR, O_TOL, O_INNER, O_OUTER, O_VERBOSE, O_COUNT };

int main(int argc, char *argv[])
{
    if (argc < 3) {
        printf("Usage: %s I1 I2 [out_file processors method_type alpha gamma lambda nscales zoom_factor TOL inner_iter outer_iter"
               " verbose]\n", argv[0]);
        return 0;
    }
    const char *image1 = argv[1], *image2 = argv[2];
    cli_val o[O_COUNT];
    cli_parse(argc, argv, 3, OPTS, O_COUNT, o);
    const char *outfile = o[O_OUT].text;
    const int nproc = (int) o[O_NPROC].num, initer = (int) o[O_INNER].num, outiter = (int) o[O_OUTER].num;
    const int verbose = (int) o[O_VERBOSE].num;
    int method = (int) o[O_METHOD].num, nscales = (int) o[O_NSCALES].num;
    if (method > 3) method = 1;
    const double alpha = o[O_ALPHA].num, gamma = o[O_GAMMA].num, lambda = o[O_LAMBDA].num, zfactor = o[O_ZFACTOR].num;
    const double TOL = o[O_TOL].num;

    int nx, ny, nz, nx1, ny1, nz1;
    double *I1 = ofx_read_image_double_vec(image1, &nx, &ny, &nz);
    double *I2 = ofx_read_image_double_vec(image2, &nx1, &ny1, &nz1);
    if (!I1 || !I2 || nx != nx1 || ny != ny1 || nz != nz1) {
        fprintf(stderr, "Cannot read the images or the size of the images are not equal\n");
        free(I1); free(I2);
        return EXIT_FAILURE;
    }
    if (nz > OFX_REXPO_MAX_CHANNELS) {
        fprintf(stderr, "ERROR: images of %d channels (at most %d)\n", nz, OFX_REXPO_MAX_CHANNELS);
        free(I1); free(I2);
        return EXIT_FAILURE;
    }
    /* the smallest level is no smaller than 16x16: N is truncated before the comparison (the rule of :127-128, in double) */
    const double N = 1 + log((nx < ny ? nx : ny) / 16.) / log(1. / zfactor);
    if ((int) N < nscales) nscales = (int) N;
    printf("\n ncores:%d method_type:%d alpha:%g gamma:%g lambda:%g scales:%d nu:%g TOL:%g inner:%d outer:%d\n", nproc, method, alpha,
           gamma, lambda, nscales, zfactor, TOL, initer, outiter);
    fflush(stdout);

    ofx_ctx *ctx = cli_context();
    if (!ctx) { free(I1); free(I2); return EXIT_FAILURE; }
    double *u = (double *) malloc(sizeof(double) * (size_t) nx * ny);
    double *v = (double *) malloc(sizeof(double) * (size_t) nx * ny);
    if (!u || !v) {
        fprintf(stderr, "ERROR: out of memory\n");
        free(u); free(v); free(I1); free(I2);
        ofx_ctx_destroy(ctx);
        return EXIT_FAILURE;
    }
    int s = ofx_robust_expo_pyramid(ctx, I1, I2, u, v, nx, ny, nz, method, alpha, gamma, lambda, nscales, zfactor, TOL, initer,
                                    outiter, verbose);
    if (s != OFX_OK) fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
    else s = cli_save_flow(outfile, u, v, nx, ny);
    free(u); free(v); free(I1); free(I2);
    cli_write_stats(ctx, argv[0]);
    ofx_ctx_destroy(ctx);
    return s == OFX_OK ? 0 : EXIT_FAILURE;
}
