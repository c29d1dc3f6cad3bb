/* flow_tracks -- dense point trajectories through a clip (ofx_track_sequence_dev): points are seeded on a grid where the frame has
 * structure, follow the step flows, and every new frame is seeded again where no live track is.
 *
 *   flow_tracks [-r rho] [-f frac] [-s step] [-c cap] out.txt f0.pgm ... fk.pgm s0.flo ... [-m m0 m1 ...]
 *
 * f0 .. fk: the k + 1 frames (PGM or PNG, gray); s0.flo .. : the k step flows, frame t -> t + 1, as tvl1flow_seq, horn_schunck_seq
 * and brox_seq write them (the arguments ending in .flo).  -m: one consistency map per step, as flow_consistency writes them, 0 =
 * valid.  -r: the Gaussian of the structure tensor (1); -f: the fraction of the mean of the smaller eigenvalue that a seed needs
 * (0.1); -s: the cell size in pixels (4); -c: the largest number of tracks (4 per cell).
 * out.txt: one line per track: t0, len, then the k + 1 positions x y, printed with %.17g: the track lives at the frames t0 .. t0 +
 * len; the positions before repeat the birth position, those after the last one.  The number of seeds dropped for lack of room
 * goes to stderr.  Files that cannot be read or differ in size are an error before the GPU is touched.
 */
#include <string.h>
#include <unistd.h>

#include "ofx_cli_common.h"

static int usage(const char *prog)
{
    fprintf(stderr, "Usage: %s [-r rho] [-f frac] [-s step] [-c cap] out.txt f0 f1 ... s0.flo s1.flo ... [-m m0 m1 ...]   "
                    "(one step less than frames, one map per step)\n", prog);
    return EXIT_FAILURE;
}

int main(int argc, char *argv[])
{
    (void) cli_save_flow;
    double rho = 1.0, frac = 0.1;
    int step = 4, cap = 0, first = 1;
    while (first + 1 < argc && argv[first][0] == '-' && argv[first][1] && !argv[first][2] && strchr("rfsc", argv[first][1])) {
        const char o = argv[first][1], *v = argv[first + 1];
        if (o == 'r') rho = atof(v);
        else if (o == 'f') frac = atof(v);
        else if (o == 's') step = atoi(v);
        else cap = atoi(v);
        first += 2;
    }
    int n_frames = 0, steps = 0, n_maps = 0, m_at = 0;
    for (int k = first + 1; k < argc && !m_at; k++) {
        if (!strcmp(argv[k], "-m")) m_at = k;
        else if (ofx_has_suffix(argv[k], ".flo")) steps++;
        else if (steps) return usage(*argv);                                /* a frame behind a flow */
        else n_frames++;
    }
    if (m_at) n_maps = argc - m_at - 1;
    if (argc < first + 4 || n_frames < 2 || steps != n_frames - 1 || (m_at && n_maps != steps) || step < 1) return usage(*argv);
    const char *out = argv[first];
    int nx = 0, ny = 0;
    double **F = (double **) calloc((size_t) n_frames, sizeof(double *));
    float **S = (float **) calloc((size_t) steps, sizeof(float *));
    unsigned char **M = (unsigned char **) calloc((size_t) steps, sizeof(unsigned char *));
    if (!F || !S || !M) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    for (int t = 0; t < n_frames; t++) {
        int w = 0, h = 0;
        F[t] = ofx_read_image_double(argv[first + 1 + t], &w, &h);
        if (!F[t]) { fprintf(stderr, "ERROR: could not read an image from file \"%s\"\n", argv[first + 1 + t]); return EXIT_FAILURE; }
        if (t && (w != nx || h != ny)) { fprintf(stderr, "ERROR: frame size mismatch %dx%d != %dx%d\n", nx, ny, w, h); return EXIT_FAILURE; }
        nx = w; ny = h;
    }
    const size_t n = (size_t) nx * ny;
    for (int t = 0; t < steps; t++) {
        int w = 0, h = 0;
        const char *name = argv[first + 1 + n_frames + t];
        S[t] = ofx_read_flo(name, &w, &h);
        if (!S[t]) { fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", name); return EXIT_FAILURE; }
        if (w != nx || h != ny) { fprintf(stderr, "ERROR: flow field size mismatch %dx%d != %dx%d\n", w, h, nx, ny); return EXIT_FAILURE; }
    }
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
    if (cap < 1) cap = 4 * (((nx - 1) / step + 1) * ((ny - 1) / step + 1));
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    float **F32 = NULL;
    if (ofx_ctx_precision(ctx) == OFX_F32) {                                /* the frames in the context's element kind */
        F32 = (float **) calloc((size_t) n_frames, sizeof(float *));
        for (int t = 0; F32 && t < n_frames; t++) {
            F32[t] = (float *) malloc(sizeof(float) * n);
            if (!F32[t]) { F32 = NULL; break; }
            for (size_t i = 0; i < n; i++) F32[t][i] = (float) F[t][i];
        }
        if (!F32) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    }
    double *xy = (double *) malloc(sizeof(double) * 2 * (size_t) cap * (size_t) n_frames);
    int *t0 = (int *) malloc(sizeof(int) * (size_t) cap), *len = (int *) malloc(sizeof(int) * (size_t) cap), count[2] = {0, 0};
    const void **pf = (const void **) calloc((size_t) n_frames, sizeof(void *));
    const void **ps = (const void **) calloc((size_t) steps, sizeof(void *)), **pm = (const void **) calloc((size_t) steps, sizeof(void *));
    if (!xy || !t0 || !len || !pf || !ps || !pm) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    for (int t = 0; t < n_frames; t++) pf[t] = F32 ? (const void *) F32[t] : (const void *) F[t];
    for (int t = 0; t < steps; t++) { ps[t] = S[t]; pm[t] = M[t]; }
    void *pxy = xy, *pt0 = t0, *plen = len, *pcount = count;
    int rc = EXIT_SUCCESS;
    int s = ofx_track_sequence_dev(ctx, 1, n_frames, pf, ps, n_maps ? pm : NULL, cap, &pxy, &pt0, &plen, &pcount, nx, ny, rho, frac,
                                   step);                                   /* host memory: staged by the entry */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    }
    if (rc == EXIT_SUCCESS) {
        FILE *f = fopen(out, "w");
        if (!f) { fprintf(stderr, "ERROR: cannot write \"%s\"\n", out); rc = EXIT_FAILURE; }
        for (int k = 0; f && k < count[0]; k++) {
            fprintf(f, "%d %d", t0[k], len[k]);
            for (int t = 0; t < n_frames; t++) {
                const size_t o = 2 * ((size_t) t * (size_t) cap + (size_t) k);
                fprintf(f, " %.17g %.17g", xy[o], xy[o + 1]);
            }
            fprintf(f, "\n");
        }
        if (f && fclose(f)) { fprintf(stderr, "ERROR: cannot write \"%s\"\n", out); rc = EXIT_FAILURE; }
        if (count[1]) fprintf(stderr, "%d tracks, %d seeds dropped: cap = %d\n", count[0], count[1], cap);
    }
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
