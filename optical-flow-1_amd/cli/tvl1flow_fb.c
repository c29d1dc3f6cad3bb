/* tvl1flow_fb -- TV-L1 in both directions with the forward-backward consistency maps (ofx_tvl1_bidir_group_dev): the two .flo
 * files are byte for byte what `tvl1flow I0 I1` and `tvl1flow I1 I0` write, the maps are those of `flow_consistency` on them
 * (255 = the vector fails the check, 0 = it passes).
 *
 *   tvl1flow_fb I0 I1 [fwd.flo bwd.flo occ_fwd occ_bwd] [tau lambda theta nscales zfactor nwarps epsilon] [fb_alpha fb_beta] [verbose]
 *
 * Defaults, ranges and the auto-nscales rule are tvl1flow's; fb_alpha = 0.01, fb_beta = 0.5 (Sundaram, Brox, Keutzer, ECCV 2010),
 * a negative one is replaced by its default.  The maps are written as ofx_write_gray_bytes writes them: .png names as 8-bit PNG,
 * other names as PGM.
 */
#include <math.h>
#include <unistd.h>

#include "ofx_cli_common.h"

static const cli_opt OPTS[] = {
    {"fwd",      CLI_TEXT, 0,    "fwd.flo", CLI_ANY, 0, NULL},
    {"bwd",      CLI_TEXT, 0,    "bwd.flo", CLI_ANY, 0, NULL},
    {"occ_fwd",  CLI_TEXT, 0,    "occ_fwd.png", CLI_ANY, 0, NULL},
    {"occ_bwd",  CLI_TEXT, 0,    "occ_bwd.png", CLI_ANY, 0, NULL},
    {"tau",      CLI_REAL, 0.25, NULL, CLI_LE0 | CLI_GT_QUARTER, 0, "warning: tau changed to %g\n"},
    {"lambda",   CLI_REAL, 0.15, NULL, CLI_LE0, 0, "warning: lambda changed to %g\n"},
    {"theta",    CLI_REAL, 0.3,  NULL, CLI_LE0, 0, "warning: theta changed to %g\n"},
    {"nscales",  CLI_INT,  100,  NULL, CLI_LE0, 0, "warning: nscales changed to %d\n"},
    {"zfactor",  CLI_REAL, 0.5,  NULL, CLI_LE0 | CLI_GE1, 0, "warning: zfactor changed to %g\n"},
    {"nwarps",   CLI_INT,  5,    NULL, CLI_LE0, 0, "warning: nwarps changed to %d\n"},
    {"epsilon",  CLI_REAL, 0.01, NULL, CLI_LE0, 0, "warning: epsilon changed to %f\n"},
    {"fb_alpha", CLI_REAL, 0.01, NULL, CLI_LT0, 0, "warning: fb_alpha changed to %g\n"},
    {"fb_beta",  CLI_REAL, 0.5,  NULL, CLI_LT0, 0, "warning: fb_beta changed to %g\n"},
    {"verbose",  CLI_INT,  0,    NULL, CLI_ANY, 0, NULL},
};
enum { O_FWD, O_BWD, O_OCC_FWD, O_OCC_BWD, O_TAU, O_LAMBDA, O_THETA, O_NSCALES, O_ZFACTOR, O_NWARPS, O_EPSILON, O_FB_ALPHA, O_FB_BETA,
       O_VERBOSE, O_COUNT };

/* a byte map through the one-channel writer of the front-ends */
static int save_map(const char *name, const unsigned char *m, int nx, int ny)
{
    const size_t n = (size_t) nx * ny;
    float *f = (float *) malloc(sizeof(float) * n);
    if (!f) return 1;
    for (size_t i = 0; i < n; i++) f[i] = (float) m[i];
    const int r = ofx_write_gray_bytes(name, f, nx, ny);
    free(f);
    if (r) fprintf(stderr, "ERROR: cannot write \"%s\"\n", name);
    return r;
}

int main(int argc, char *argv[])
{
    if (argc < 3) {
        fprintf(stderr, "Usage: %s I0 I1 [fwd.flo bwd.flo occ_fwd occ_bwd] [tau lambda theta nscales zfactor nwarps epsilon] "
                        "[fb_alpha fb_beta] [verbose]\n", *argv);
        return EXIT_FAILURE;
    }
    cli_phase(NULL);
    (void) cli_save_flow;                   /* the payloads arrive interleaved: ofx_write_flo directly */
    cli_val o[O_COUNT];
    cli_parse(argc, argv, 3, OPTS, O_COUNT, o);
    int nscales = (int) o[O_NSCALES].num;
    const int nwarps = (int) o[O_NWARPS].num, verbose = (int) o[O_VERBOSE].num;
    const double tau = o[O_TAU].num, lambda = o[O_LAMBDA].num, theta = o[O_THETA].num, zfactor = o[O_ZFACTOR].num;
    const double epsilon = o[O_EPSILON].num, fb_alpha = o[O_FB_ALPHA].num, fb_beta = o[O_FB_BETA].num;
    if (!ofx_has_suffix(o[O_FWD].text, ".flo") || !ofx_has_suffix(o[O_BWD].text, ".flo")) {
        fprintf(stderr, "ERROR: outputs \"%s\", \"%s\": only the .flo format is supported\n", o[O_FWD].text, o[O_BWD].text);
        return EXIT_FAILURE;
    }

    int nx, ny, nx2, ny2;
    double *I0 = ofx_read_image_double(argv[1], &nx, &ny);
    if (!I0) fprintf(stderr, "ERROR: could not read image from file \"%s\"\n", argv[1]);
    double *I1 = ofx_read_image_double(argv[2], &nx2, &ny2);
    if (!I1) fprintf(stderr, "ERROR: could not read image from file \"%s\"\n", argv[2]);
    if (!I0 || !I1 || nx != nx2 || ny != ny2) {
        if (I0 && I1) fprintf(stderr, "ERROR: input images size mismatch %dx%d != %dx%d\n", nx, ny, nx2, ny2);
        free(I0); free(I1);
        return EXIT_FAILURE;
    }
    cli_phase("read_images");
    /* smallest pyramid image not below ~16x16, as tvl1flow */
    const double N = 1 + log(hypot(nx, ny) / 16.0) / log(1 / zfactor);
    if (N < nscales) nscales = (int) N;
    if (verbose)
        fprintf(stderr, "tau=%f lambda=%f theta=%f nscales=%d zfactor=%f nwarps=%d epsilon=%g fb_alpha=%g fb_beta=%g\n", tau, lambda,
                theta, nscales, zfactor, nwarps, epsilon, fb_alpha, fb_beta);

    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    cli_phase("wait_for_context");
    const size_t n = (size_t) nx * ny;
    /* the entry reads frames of the context's storage precision and stages host memory itself */
    const void *f0 = I0, *f1 = I1;
    float *S0 = NULL;
    if (ofx_ctx_precision(ctx) == OFX_F32) {
        S0 = (float *) malloc(sizeof(float) * 2 * n);
        for (size_t i = 0; S0 && i < n; i++) { S0[i] = (float) I0[i]; S0[n + i] = (float) I1[i]; }
        f0 = S0;
        f1 = S0 + n;
    }
    float *flo = (float *) malloc(sizeof(float) * 4 * n);
    unsigned char *occ = (unsigned char *) malloc(2 * n);
    int rc = EXIT_SUCCESS;
    if (!flo || !occ || !f0) {
        fprintf(stderr, "ERROR: out of memory\n");
        rc = EXIT_FAILURE;
    } else {
        void *pf = flo, *pb = flo + 2 * n, *of = occ, *ob = occ + n;
        int s = ofx_tvl1_bidir_group_dev(ctx, 1, &f0, &f1, &pf, &pb, &of, &ob, nx, ny, tau, lambda, theta, nscales, zfactor, nwarps,
                                         epsilon, fb_alpha, fb_beta, NULL);
        if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
        cli_phase("solve");
        if (s != OFX_OK) {
            fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
            rc = EXIT_FAILURE;
        } else {
            if (ofx_write_flo(o[O_FWD].text, flo, nx, ny)) { fprintf(stderr, "ERROR: cannot write \"%s\"\n", o[O_FWD].text); rc = EXIT_FAILURE; }
            if (ofx_write_flo(o[O_BWD].text, flo + 2 * n, nx, ny)) { fprintf(stderr, "ERROR: cannot write \"%s\"\n", o[O_BWD].text); rc = EXIT_FAILURE; }
            if (save_map(o[O_OCC_FWD].text, occ, nx, ny)) rc = EXIT_FAILURE;
            if (save_map(o[O_OCC_BWD].text, occ + n, nx, ny)) rc = EXIT_FAILURE;
        }
        cli_phase("write_results");
    }
    free(flo); free(occ); free(S0); free(I0); free(I1);
    cli_write_stats(ctx, argv[0]);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");          /* as tvl1flow: skip the HIP runtime's exit handlers unless OFX_FAST_EXIT=0 */
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
