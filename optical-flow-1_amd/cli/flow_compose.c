/* flow_compose -- the step flows of a video chained into long-range flows (ofx_flow_accumulate_dev): s0.flo is the flow of frame
 * 0 -> 1, s1.flo of frame 1 -> 2, ... as tvl1flow_seq, horn_schunck_seq and brox_seq write them.
 *
 *   flow_compose [-x ext] out_prefix s0.flo s1.flo ... [-m m0 m1 ...]
 *
 * Writes out_prefix0000.flo = the flow 0 -> 1, out_prefix0001.flo = 0 -> 2, ... on frame 0's grid, with the numbering of
 * tvl1flow_seq, and beside each payload the map out_prefix0000.png, ...: 255 where the vector was lost on the way -- it left the
 * image or met a flagged position -- and stays where it was lost, 0 where it arrived.  -m: one consistency map per step, as
 * flow_consistency writes them (PGM or PNG), 0 = valid, anything else = flagged.  -x: the extension of the maps written (png by
 * default; names ending in .png are written as 8-bit PNG, others as PGM, as flow_consistency does).  Files that cannot be read
 * or differ in size are an error before the GPU is touched.
 */
#include <string.h>
#include <unistd.h>

#include "ofx_cli_common.h"

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
    (void) cli_save_flow;
    const char *ext = "png";
    int first = 1;
    if (argc > 2 && !strcmp(argv[1], "-x")) { ext = argv[2]; first = 3; }
    int steps = 0, n_maps = 0, m_at = 0;
    for (int k = first + 1; k < argc && !m_at; k++) {
        if (!strcmp(argv[k], "-m")) m_at = k;
        else steps++;
    }
    if (m_at) n_maps = argc - m_at - 1;
    if (argc < first + 2 || steps < 1 || (m_at && n_maps != steps)) {
        fprintf(stderr, "Usage: %s [-x ext] out_prefix s0.flo s1.flo ... [-m m0 m1 ...]   (one map per step)\n", *argv);
        return EXIT_FAILURE;
    }
    const char *prefix = argv[first];
    int nx = 0, ny = 0;
    float **S = (float **) calloc((size_t) steps, sizeof(float *));
    unsigned char **M = (unsigned char **) calloc((size_t) steps, sizeof(unsigned char *));
    if (!S || !M) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    for (int t = 0; t < steps; t++) {
        int w = 0, h = 0;
        S[t] = ofx_read_flo(argv[first + 1 + t], &w, &h);
        if (!S[t]) {
            fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", argv[first + 1 + t]);
            return EXIT_FAILURE;
        }
        if (t && (w != nx || h != ny)) {
            fprintf(stderr, "ERROR: flow fields size mismatch %dx%d != %dx%d\n", nx, ny, w, h);
            return EXIT_FAILURE;
        }
        nx = w; ny = h;
    }
    const size_t n = (size_t) nx * ny;
    for (int t = 0; t < n_maps; t++) {
        int w = 0, h = 0;
        double *m = ofx_read_image_double(argv[m_at + 1 + t], &w, &h);
        if (!m || w != nx || h != ny) {
            if (!m) fprintf(stderr, "ERROR: could not read a map from file \"%s\"\n", argv[m_at + 1 + t]);
            else fprintf(stderr, "ERROR: map size mismatch %dx%d != %dx%d\n", w, h, nx, ny);
            return EXIT_FAILURE;
        }
        M[t] = (unsigned char *) malloc(n);
        if (!M[t]) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
        for (size_t i = 0; i < n; i++) M[t][i] = m[i] != 0.0 ? 255 : 0;
        free(m);
    }
    float *acc = (float *) malloc(sizeof(float) * 2 * n * (size_t) steps);
    unsigned char *occ = (unsigned char *) malloc(n * (size_t) steps);
    const void **ps = (const void **) calloc((size_t) steps, sizeof(void *)), **pm = (const void **) calloc((size_t) steps, sizeof(void *));
    void **pa = (void **) calloc((size_t) steps, sizeof(void *)), **po = (void **) calloc((size_t) steps, sizeof(void *));
    if (!acc || !occ || !ps || !pm || !pa || !po) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    for (int t = 0; t < steps; t++) {
        ps[t] = S[t];
        pm[t] = M[t];
        pa[t] = acc + 2 * n * (size_t) t;
        po[t] = occ + n * (size_t) t;
    }
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    int rc = EXIT_SUCCESS;
    int s = ofx_flow_accumulate_dev(ctx, 1, steps, ps, n_maps ? pm : NULL, pa, po, nx, ny);         /* host memory: staged by the entry */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    }
    for (int t = 0; t < steps && rc == EXIT_SUCCESS; t++) {
        char name[4096];
        snprintf(name, sizeof(name), "%s%04d.flo", prefix, t);
        if (ofx_write_flo(name, acc + 2 * n * (size_t) t, nx, ny)) {
            fprintf(stderr, "ERROR: cannot write \"%s\"\n", name);
            rc = EXIT_FAILURE;
        }
        snprintf(name, sizeof(name), "%s%04d.%s", prefix, t, ext);
        if (rc == EXIT_SUCCESS && save_map(name, occ + n * (size_t) t, nx, ny)) rc = EXIT_FAILURE;
    }
    for (int t = 0; t < steps; t++) { free(S[t]); free(M[t]); }
    free(S); free(M); free(acc); free(occ); free(ps); free(pm); free(pa); free(po);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
