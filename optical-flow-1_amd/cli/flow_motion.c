/* flow_motion -- the dominant (camera) motion of a flow field (ofx_flow_motion_fit_dev): a translation, similarity or affine model
 * fitted to a .flo payload by re-weighted least squares with Tukey's biweight, as tvl1flow, horn_schunck_pyramidal and brox_spatial
 * write the payload.
 *
 *   flow_motion [-o prefix] [-x ext] in.flo model n_fits c_first c_last [occ.png]
 *
 * model: translation, similarity or affine (or 2, 4, 6); n_fits: the number of fits, the first one unweighted; c_first, c_last: the
 * cut-off of the weights in pixels, halved from c_first down to c_last; occ: a map as flow_consistency writes them (PGM or PNG),
 * 0 = valid, anything else = flagged.  Prints the record -- "theta" t0 a b t1 c d on the centred coordinates of include/ofx.h,
 * "pixel" p0 p1 p2 q0 q1 q2 (u = p0 + p1 * column + p2 * row), "fit" S1, fits completed, the cut-off of the map and 1 if the call
 * stopped on a degenerate fit -- with %.17g, and writes prefix_resid.flo = the camera-compensated flow, prefix_model.flo = the
 * model's flow and prefix_inlier.ext = the map of the pixels that disagree with the model (255).  -o: the prefix (in.flo without
 * its .flo by default); -x: the extension of the map (png by default; names ending in .png are written as 8-bit PNG, others as
 * PGM, as flow_consistency does).  Files that cannot be read or differ in size are an error before the GPU is touched.
 */
#include <string.h>
#include <unistd.h>

#include "ofx_cli_common.h"

static int usage(const char *prog)
{
    fprintf(stderr, "Usage: %s [-o prefix] [-x ext] in.flo model n_fits c_first c_last [occ.png]   "
                    "(model: translation | similarity | affine)\n", prog);
    return EXIT_FAILURE;
}

static int model_of(const char *s)
{
    if (!strcmp(s, "translation") || !strcmp(s, "2")) return OFX_MOTION_TRANSLATION;
    if (!strcmp(s, "similarity") || !strcmp(s, "4")) return OFX_MOTION_SIMILARITY;
    if (!strcmp(s, "affine") || !strcmp(s, "6")) return OFX_MOTION_AFFINE;
    return 0;
}

static int save_map(const char *name, const unsigned char *m, int nx, int ny)
{
    const size_t n = (size_t) nx * ny;
    float *f = (float *) malloc(sizeof(float) * n);
    if (!f) return 1;
    for (size_t i = 0; i < n; i++) f[i] = (float) m[i];
    const int r = ofx_write_gray_bytes(name, f, nx, ny);
    free(f);
    return r;
}

int main(int argc, char *argv[])
{
    (void) cli_save_flow;
    const char *ext = "png", *prefix = NULL;
    int first = 1;
    while (first + 1 < argc && (!strcmp(argv[first], "-o") || !strcmp(argv[first], "-x"))) {
        if (argv[first][1] == 'o') prefix = argv[first + 1];
        else ext = argv[first + 1];
        first += 2;
    }
    if (argc - first < 5 || argc - first > 6) return usage(*argv);
    const char *in = argv[first], *occ_name = argc - first == 6 ? argv[first + 5] : NULL;
    const int model = model_of(argv[first + 1]), n_fits = atoi(argv[first + 2]);
    const double c_first = atof(argv[first + 3]), c_last = atof(argv[first + 4]);
    if (!model) return usage(*argv);
    char stem[4096];
    if (!prefix) {
        snprintf(stem, sizeof(stem), "%s", in);
        if (ofx_has_suffix(stem, ".flo")) stem[strlen(stem) - 4] = 0;
        prefix = stem;
    }
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
    float *mdl = (float *) malloc(sizeof(float) * 2 * n), *res = (float *) malloc(sizeof(float) * 2 * n);
    unsigned char *inl = (unsigned char *) malloc(n);
    double rec[OFX_MOTION_REC];
    if (!mdl || !res || !inl) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    const void *pf = flo, *po = occ;
    void *pr = rec, *pm = mdl, *ps = res, *pi = inl;
    int rc = EXIT_SUCCESS;
    int s = ofx_flow_motion_fit_dev(ctx, 1, &pf, occ ? &po : NULL, NULL, &pr, model, n_fits, c_first, c_last, &pm, &ps, &pi, nx,
                                    ny);                                    /* host memory: staged by the entry */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    }
    if (rc == EXIT_SUCCESS) {
        printf("theta %.17g %.17g %.17g %.17g %.17g %.17g\n", rec[0], rec[1], rec[2], rec[3], rec[4], rec[5]);
        printf("pixel %.17g %.17g %.17g %.17g %.17g %.17g\n", rec[6], rec[7], rec[8], rec[9], rec[10], rec[11]);
        printf("fit %.17g %.17g %.17g %.17g\n", rec[12], rec[13], rec[14], rec[15]);
        char name[4200];
        snprintf(name, sizeof(name), "%s_resid.flo", prefix);
        if (ofx_write_flo(name, res, nx, ny)) { fprintf(stderr, "ERROR: cannot write \"%s\"\n", name); rc = EXIT_FAILURE; }
        snprintf(name, sizeof(name), "%s_model.flo", prefix);
        if (rc == EXIT_SUCCESS && ofx_write_flo(name, mdl, nx, ny)) { fprintf(stderr, "ERROR: cannot write \"%s\"\n", name); rc = EXIT_FAILURE; }
        snprintf(name, sizeof(name), "%s_inlier.%s", prefix, ext);
        if (rc == EXIT_SUCCESS && save_map(name, inl, nx, ny)) { fprintf(stderr, "ERROR: cannot write \"%s\"\n", name); rc = EXIT_FAILURE; }
    }
    free(flo); free(occ); free(mdl); free(res); free(inl);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
