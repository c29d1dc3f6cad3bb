/* flow_interpolate -- the frame at time t between two frames, from the flows of both directions (ofx_flow_interpolate_dev): what
 * tvl1flow_fb writes is what this reads.
 *
 *   flow_interpolate A B fwd.flo bwd.flo out [t = 0.5]
 *
 * A, B: 8-bit PGM / PPM / PNG frames of one size, channels kept (1 or 3); fwd.flo: the flow A -> B on A's grid, bwd.flo: B -> A on
 * B's grid; out: the in-between frame as binary PGM (P5) or PPM (P6).  t outside [0, 1] is refused by the library.  Samples that
 * are not bytes, a channel count other than 1 or 3 and sizes that differ are an error before the GPU is touched.
 */
#include <unistd.h>

#include "ofx_cli_common.h"

/* the file's samples as bytes, or NULL with a message (exit status 1) */
static unsigned char *read_bytes(const char *name, int *w, int *h, int *c)
{
    double *d = ofx_read_image_double_vec(name, w, h, c);
    if (!d) {
        fprintf(stderr, "ERROR: could not read an image from file \"%s\"\n", name);
        return NULL;
    }
    if (*c != 1 && *c != 3) {
        fprintf(stderr, "ERROR: \"%s\" has %d channels (1 or 3)\n", name, *c);
        free(d);
        return NULL;
    }
    const size_t n = (size_t) *w * *h * *c;
    unsigned char *b = (unsigned char *) malloc(n ? n : 1);
    for (size_t i = 0; b && i < n; i++) {
        if (!(d[i] >= 0 && d[i] <= 255 && d[i] == (double) (unsigned char) d[i])) {
            fprintf(stderr, "ERROR: \"%s\": sample %g is not a byte (8-bit frames only)\n", name, d[i]);
            free(b);
            b = NULL;
            break;
        }
        b[i] = (unsigned char) d[i];
    }
    free(d);
    return b;
}

int main(int argc, char *argv[])
{
    if (argc < 6) {
        fprintf(stderr, "Usage: %s A B fwd.flo bwd.flo out [t = 0.5]\n", *argv);
        return EXIT_FAILURE;
    }
    (void) cli_save_flow;
    const double t = argc > 6 ? atof(argv[6]) : 0.5;
    int nx, ny, nz, nx2, ny2, nz2, fx, fy, bx, by;
    unsigned char *A = read_bytes(argv[1], &nx, &ny, &nz);
    unsigned char *B = A ? read_bytes(argv[2], &nx2, &ny2, &nz2) : NULL;
    if (!A || !B) { free(A); free(B); return EXIT_FAILURE; }
    if (nx != nx2 || ny != ny2 || nz != nz2) {
        fprintf(stderr, "ERROR: frames differ: %dx%dx%d != %dx%dx%d\n", nx, ny, nz, nx2, ny2, nz2);
        free(A); free(B);
        return EXIT_FAILURE;
    }
    float *fwd = ofx_read_flo(argv[3], &fx, &fy);
    if (!fwd) fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", argv[3]);
    float *bwd = fwd ? ofx_read_flo(argv[4], &bx, &by) : NULL;
    if (fwd && !bwd) fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", argv[4]);
    if (fwd && bwd && (fx != nx || fy != ny || bx != nx || by != ny)) {
        fprintf(stderr, "ERROR: flow fields %dx%d, %dx%d do not match the frames' %dx%d\n", fx, fy, bx, by, nx, ny);
        free(bwd);
        bwd = NULL;
    }
    const size_t n = (size_t) nx * ny * nz;
    unsigned char *out = (fwd && bwd) ? (unsigned char *) malloc(n) : NULL;
    if (!out) { free(A); free(B); free(fwd); free(bwd); return EXIT_FAILURE; }
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    int rc = EXIT_SUCCESS;
    const void *pa = A, *pb = B, *pf = fwd, *pw = bwd;
    void *po = out;
    int s = ofx_set_option(ctx, "input", OFX_IN_U8);
    if (s == OFX_OK) s = ofx_flow_interpolate_dev(ctx, 1, &pa, &pb, &pf, &pw, &t, &po, nx, ny, nz);      /* host memory: staged by the entry */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    } else if (ofx_write_bytes_image(argv[5], out, nx, ny, nz)) {
        fprintf(stderr, "ERROR: cannot write \"%s\"\n", argv[5]);
        rc = EXIT_FAILURE;
    }
    free(out); free(A); free(B); free(fwd); free(bwd);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
