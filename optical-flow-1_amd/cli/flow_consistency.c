/* flow_consistency -- forward-backward consistency maps of two .flo files (ofx_flow_consistency_dev), whichever solver wrote
 * them: fwd.flo is the flow A -> B on A's grid, bwd.flo the flow B -> A on B's grid.
 *
 *   flow_consistency fwd.flo bwd.flo occ_fwd occ_bwd [alpha beta]
 *
 * A map holds 255 where the vector fails |w(x) + w'(x + w(x))|^2 <= alpha (|w(x)|^2 + |w'(x + w(x))|^2) + beta or leaves the
 * image, 0 where it passes; alpha = 0.01, beta = 0.5 by default (Sundaram, Brox, Keutzer, ECCV 2010), a negative one is replaced
 * by its default.  Names ending in .png are written as 8-bit PNG, others as PGM.  Files that cannot be read or differ in size
 * are an error before the GPU is touched.
 */
#include <unistd.h>

#include "ofx_cli_common.h"

static const cli_opt OPTS[] = {
    {"alpha", CLI_REAL, 0.01, NULL, CLI_LT0, 0, NULL},
    {"beta",  CLI_REAL, 0.5,  NULL, CLI_LT0, 0, NULL},
};

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
    if (argc < 5) {
        fprintf(stderr, "Usage: %s fwd.flo bwd.flo occ_fwd occ_bwd [alpha beta]\n", *argv);
        return EXIT_FAILURE;
    }
    (void) cli_save_flow;
    cli_val o[2];
    cli_parse(argc, argv, 5, OPTS, 2, o);
    int nx, ny, nx2, ny2;
    float *fwd = ofx_read_flo(argv[1], &nx, &ny);
    if (!fwd) fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", argv[1]);
    float *bwd = ofx_read_flo(argv[2], &nx2, &ny2);
    if (!bwd) fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", argv[2]);
    if (!fwd || !bwd || nx != nx2 || ny != ny2) {
        if (fwd && bwd) fprintf(stderr, "ERROR: flow fields size mismatch %dx%d != %dx%d\n", nx, ny, nx2, ny2);
        free(fwd); free(bwd);
        return EXIT_FAILURE;
    }
    const size_t n = (size_t) nx * ny;
    unsigned char *occ = (unsigned char *) malloc(2 * n);
    if (!occ) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    int rc = EXIT_SUCCESS;
    const void *pf = fwd, *pb = bwd;
    void *of = occ, *ob = occ + n;
    int s = ofx_flow_consistency_dev(ctx, 1, &pf, &pb, &of, &ob, nx, ny, o[0].num, o[1].num);      /* host memory: staged by the entry */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    } else {
        if (save_map(argv[3], occ, nx, ny)) rc = EXIT_FAILURE;
        if (save_map(argv[4], occ + n, nx, ny)) rc = EXIT_FAILURE;
    }
    free(occ); free(fwd); free(bwd);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
