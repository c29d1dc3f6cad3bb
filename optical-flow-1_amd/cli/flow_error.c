/* flow_error -- the error statistics of a flow field against its ground truth (ofx_flow_error_dev), both .flo payloads as tvl1flow,
 * horn_schunck_pyramidal and brox_spatial write them and as the Middlebury benchmark ships its truth.
 *
 *   flow_error est.flo gt.flo [occ.png|pgm] [bin_w n_bins]
 *
 * occ: a map as flow_consistency writes them (PGM or PNG), 0 = valid, anything else = flagged; an argument that reads as a number
 * is bin_w.  Truth vectors that are NaN, Inf or beyond 1e9 (Middlebury's unknown marker) and flagged pixels are left out; estimate
 * vectors that are NaN or Inf on known pixels are "bad" and count as outliers of every rate.  Prints, one line each, with %.17g:
 * "known" and "bad" (counts), "AEPE", "RMS", "AAE" (degrees), "max", the outlier rates "R0.5" "R1" "R2" "R3" "R5" (end-point error
 * above that many pixels) and "Fl" (above 3 px and above 5 % of the truth's length) as fractions of the known pixels, and the
 * percentiles "A50" "A75" "A95" of the end-point error, read from the device histogram of n_bins bins of width bin_w (1/64 px and
 * 4096 by default): the upper edge of the bin at which the cumulative count reaches ceil(p * known).  Files that cannot be read or
 * differ in size are an error before the GPU is touched.
 */
#include <math.h>
#include <string.h>
#include <unistd.h>

#include "ofx_cli_common.h"

#define N_THR 6

static int usage(const char *prog)
{
    fprintf(stderr, "Usage: %s est.flo gt.flo [occ.png|pgm] [bin_w n_bins]\n", prog);
    return EXIT_FAILURE;
}

static int is_number(const char *s)
{
    char *end;
    strtod(s, &end);
    return end != s && *end == 0;
}

int main(int argc, char *argv[])
{
    (void) cli_save_flow;
    if (argc < 3 || argc > 6) return usage(*argv);
    int next = 3;
    const char *occ_name = NULL;
    if (argc > next && !is_number(argv[next])) occ_name = argv[next++];
    double bin_w = 1.0 / 64.0;
    int n_bins = 4096;
    if (argc > next) {
        if (argc != next + 2) return usage(*argv);
        bin_w = atof(argv[next]);
        n_bins = atoi(argv[next + 1]);
    }
    int nx = 0, ny = 0, gx = 0, gy = 0;
    float *flo = ofx_read_flo(argv[1], &nx, &ny);
    if (!flo) { fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", argv[1]); return EXIT_FAILURE; }
    float *gt = ofx_read_flo(argv[2], &gx, &gy);
    if (!gt) { fprintf(stderr, "ERROR: could not read a flow field from file \"%s\"\n", argv[2]); return EXIT_FAILURE; }
    if (gx != nx || gy != ny) { fprintf(stderr, "ERROR: flow size mismatch %dx%d != %dx%d\n", gx, gy, nx, ny); return EXIT_FAILURE; }
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
    unsigned int *hist = (unsigned int *) calloc(n_bins > 0 ? (size_t) n_bins : 1, sizeof(unsigned int));
    if (!hist) { fprintf(stderr, "ERROR: out of memory\n"); return EXIT_FAILURE; }
    static const char *names[N_THR] = {"R0.5", "R1", "R2", "R3", "R5", "Fl"};
    const double thr_abs[N_THR] = {0.5, 1.0, 2.0, 3.0, 5.0, 3.0}, thr_rel[N_THR] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.05};
    double rec[OFX_ERROR_REC];
    ofx_ctx *ctx = cli_context();
    if (!ctx) return EXIT_FAILURE;
    const void *pf = flo, *pg = gt, *po = occ;
    void *pr = rec, *ph = hist;
    int rc = EXIT_SUCCESS;
    int s = ofx_flow_error_dev(ctx, 1, &pf, &pg, occ ? &po : NULL, N_THR, thr_abs, thr_rel, &pr, NULL, &ph, n_bins, bin_w, nx,
                               ny);                                         /* host memory: staged by the entry */
    if (s == OFX_OK) s = ofx_ctx_synchronize(ctx);
    if (s != OFX_OK) {
        fprintf(stderr, "ERROR: %s (%s)\n", ofx_strerror(s), ofx_last_error(ctx));
        rc = EXIT_FAILURE;
    }
    if (rc == EXIT_SUCCESS) {
        const double known = rec[0];
        printf("known %.17g\nbad %.17g\nAEPE %.17g\nRMS %.17g\nAAE %.17g\nmax %.17g\n", rec[0], rec[1], rec[2], rec[3], rec[4], rec[5]);
        for (int k = 0; k < N_THR; k++) printf("%s %.17g\n", names[k], known > 0.0 ? rec[8 + k] / known : 0.0);
        static const char *pn[3] = {"A50", "A75", "A95"};
        const double pv[3] = {0.5, 0.75, 0.95};
        for (int q = 0; q < 3; q++) {
            const double need = ceil(pv[q] * known);
            double cum = 0.0, edge = 0.0;
            for (int b = 0; b < n_bins && known > 0.0; b++) {
                cum += (double) hist[b];
                if (cum >= need) { edge = (double) (b + 1) * bin_w; break; }
            }
            printf("%s %.17g\n", pn[q], edge);
        }
    }
    free(flo); free(gt); free(occ); free(hist);
    ofx_ctx_destroy(ctx);
    const char *fe = getenv("OFX_FAST_EXIT");
    if (!fe || atoi(fe) != 0) {
        fflush(NULL);
        _exit(rc);
    }
    return rc;
}
