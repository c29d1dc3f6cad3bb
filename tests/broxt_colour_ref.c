/* broxt_colour_ref.c -- CPU checker of the temporal Brox solver in TWO sweep orders (tests/broxt_colour_ref.py builds and loads it).
 *
 * oracle/ofx_oracle.c has the reference's sweep order only; the tolerance mode of the GPU solver (option sor_exact = 0) sweeps the
 * nz = frames - 1 flow fields of a level in a 3-D red-black order.  This file restates the oracle's brox_t_single_scale and its
 * multiscale driver with a switch:
 *   order 0: the reference's order (frames 1 .. nz-2, then 0, then nz-1; in a frame the interior, the first / last row, the first /
 *            last column, the corners) -- pinned bit for bit to orc_brox_temporal by tests/test_broxt_colour_ref.py
 *   order 1: every voxel with (i + j + f) even, then every voxel with (i + j + f) odd.  No voxel of a colour reads another voxel of
 *            that colour, so the result does not depend on the order inside a colour step.
 * The operators (gradients, warp, Gaussian, zoom) are liboracle.so's.  The update is the oracle's, expression for expression; the
 * stopping sum is ONE chain in visiting order.  Compile with -ffp-contract=off.
 *
 * broxt_colour_ref_mode adds store_f32: the HIP path's float storage (OFX_F32: float in memory, double arithmetic) in either order.
 * With store_f32 = 0 it is broxt_colour_ref bit for bit.  With store_f32 = 1 a value is rounded to float exactly where the float
 * instantiation has a float in memory or calls rnd_to / tile_rnd; all arithmetic and every value not listed stays double.
 * THE CONTRACT OF THE MODE -- rounded are (kernel and array of csrc/ofx_sor.hip, ofx_sor_tile.hip, ofx_ops.hip):
 *   head     the input frames (upload_plane, or float frames of a device entry); the normalised frames, one min / max per sequence
 *            (op_normalize_sets_in / op_normalize_map_in); the Gaussian and the zoom-out as orc_gaussian_mode / orc_zoom_out_mode
 *            (op_gaussian_planes, op_zoom_out_channels_planes); the flow zoomed in and multiplied by 1 / nu, one rounding after the
 *            product (op_zoom_in_flow);
 *   level    Ix, Iy of every frame, Ixx, Ixy, Iyy of frames 1 .. frames - 1 (k_brox_prepare / k_broxt_prepare_group: G1, PA, PB);
 *            the six warps Iw .. Iwyy (k_brox_warp: WA, WB); psis (k_broxt_psis: Psis); div_u, div_v, div_d (k_broxt_div: DV, Dd);
 *            psid and psig (rnd_to in brox_coeff_px); Au, Av, Du, Dv, D (brox_coeff_px: CO, Dm); du and dv after every update
 *            (rnd_to in broxt_point, tile_rnd in bxt_update of k_broxt_rb / k_broxt_tile); u and v after du, dv are added
 *            (k_brox_add: U).
 *   NOT rounded: psi1 .. psi6 (half-sums recomputed in double from psis, broxt_psi6 and the tile kernels); ux .. vt of the flow;
 *            every intermediate of brox_coeff_px but psid and psig.
 * The stopping sums add the squared differences of the rounded values, in double.  tests/test_gpu_sor_f32_temporal_rexpo.py holds
 * the GPU to this bit for bit. */
#include <math.h>
#include <stdlib.h>

void orc_centered_gradient(const double *f, double *dx, double *dy, int nx, int ny);
void orc_centered_gradient3(const double *in, double *dx, double *dy, double *dz, int nx, int ny, int nz);
void orc_dxx(const double *f, double *out, int nx, int ny);
void orc_dyy(const double *f, double *out, int nx, int ny);
void orc_dxy(const double *f, double *out, int nx, int ny);
int orc_gaussian(double *I, int nx, int ny, double sigma);
int orc_gaussian_mode(double *I, int nx, int ny, double sigma, int store_f32);
int orc_zoom_out_mode(const double *I, double *Iout, int nx, int ny, double factor, int store_f32);
void orc_bicubic_warp(const double *in, const double *u, const double *v, double *out, int nx, int ny, int border_out);
void orc_zoom_size(int nx, int ny, int *nxx, int *nyy, double factor);
int orc_zoom_out(const double *I, double *Iout, int nx, int ny, double factor);
void orc_zoom_in(const double *I, double *Iout, int nx, int ny, int nxx, int nyy);
void orc_image_normalization_1(const double *I, double *In, int size);

#define EPSILON 0.001
#define MAXITER 300
#define SOR_W 1.9
#define SIGMA 0.8

/* float storage: a value that the float instantiation keeps as a float in memory, or passes through rnd_to / tile_rnd */
static inline double rnd_f32(double x) { return (double) (float) x; }
static void round_f32(double *x, size_t n)
{
    for (size_t i = 0; i < n; i++) x[i] = rnd_f32(x[i]);
}
#define ST32(x) (f32 ? rnd_f32(x) : (x))

typedef struct {
    const double *Au, *Av, *Du, *Dv, *D, *psi;
    double *du, *dv;
    double alpha;
    int nx, ny, nz;
    int f32;
} Sys;

/* one voxel: a missing neighbour (row, column or frame) is the voxel itself with psi = 0; dv takes the NEW du */
static double sor_point(const Sys *S, int f, int i, int j)
{
    const int nx = S->nx, ny = S->ny, nz = S->nz, df = nx * ny;
    const int k = f * df + i * nx + j;
    const double *psi = S->psi;
    double *du = S->du, *dv = S->dv;
    const int dy1 = (i < ny - 1) ? nx : 0, dy0 = (i > 0) ? nx : 0;
    const int dx1 = (j < nx - 1) ? 1 : 0, dx0 = (j > 0) ? 1 : 0;
    const int df1 = (f < nz - 1) ? df : 0, df0 = (f > 0) ? df : 0;
    const double psi1 = dy1 ? 0.5 * (psi[k + nx] + psi[k]) : 0;
    const double psi2 = dy0 ? 0.5 * (psi[k - nx] + psi[k]) : 0;
    const double psi3 = dx1 ? 0.5 * (psi[k + 1] + psi[k]) : 0;
    const double psi4 = dx0 ? 0.5 * (psi[k - 1] + psi[k]) : 0;
    const double psi5 = df0 ? 0.5 * (psi[k - df] + psi[k]) : 0;
    const double psi6 = df1 ? 0.5 * (psi[k + df] + psi[k]) : 0;
    const double w = SOR_W;
    const int f32 = S->f32;
    const double div_du = psi1 * du[k + dy1] + psi2 * du[k - dy0] + psi3 * du[k + dx1] + psi4 * du[k - dx0] + psi5 * du[k - df0] +
                          psi6 * du[k + df1];
    const double div_dv = psi1 * dv[k + dy1] + psi2 * dv[k - dy0] + psi3 * dv[k + dx1] + psi4 * dv[k - dx0] + psi5 * dv[k - df0] +
                          psi6 * dv[k + df1];
    const double duk = du[k], dvk = dv[k];
    du[k] = ST32((1. - w) * du[k] + w * (S->Au[k] - S->D[k] * dv[k] + S->alpha * div_du) / S->Du[k]);
    dv[k] = ST32((1. - w) * dv[k] + w * (S->Av[k] - S->D[k] * du[k] + S->alpha * div_dv) / S->Dv[k]);
    return (du[k] - duk) * (du[k] - duk) + (dv[k] - dvk) * (dv[k] - dvk);
}

/* one frame of one sweep in the reference's visiting order */
static double sweep_frame(const Sys *S, int f)
{
    const int nx = S->nx, ny = S->ny;
    double e = 0;
    for (int i = 1; i < ny - 1; i++)
        for (int j = 1; j < nx - 1; j++) e += sor_point(S, f, i, j);
    for (int j = 1; j < nx - 1; j++) {
        e += sor_point(S, f, 0, j);
        e += sor_point(S, f, ny - 1, j);
    }
    for (int i = 1; i < ny - 1; i++) {
        e += sor_point(S, f, i, 0);
        e += sor_point(S, f, i, nx - 1);
    }
    e += sor_point(S, f, 0, 0);
    e += sor_point(S, f, 0, nx - 1);
    e += sor_point(S, f, ny - 1, 0);
    e += sor_point(S, f, ny - 1, nx - 1);
    return e;
}

static double sweep(const Sys *S, int order)
{
    const int nx = S->nx, ny = S->ny, nz = S->nz;
    double e = 0;
    if (order == 0) {
        for (int f = 1; f < nz - 1; f++) e += sweep_frame(S, f);
        e += sweep_frame(S, 0);
        e += sweep_frame(S, nz - 1);
    } else {
        for (int colour = 0; colour < 2; colour++)
            for (int f = 0; f < nz; f++)
                for (int i = 0; i < ny; i++)
                    for (int j = (i + f + colour) & 1; j < nx; j += 2) e += sor_point(S, f, i, j);
    }
    return e;
}

static double *dalloc(size_t n)
{
    double *p = (double *) calloc(n ? n : 1, sizeof(double));
    if (!p) abort();
    return p;
}

/* sum over the neighbours that exist of psi * (neighbour - centre), in the order down, up, right, left; a missing term is left out */
static double div_at(const double *f, const double *psi, int i, int j, int nx, int ny)
{
    const int k = i * nx + j;
    double acc = 0;
    int have = 0;
    if (i < ny - 1) { acc = 0.5 * (psi[k + nx] + psi[k]) * (f[k + nx] - f[k]); have = 1; }
    if (i > 0) { const double t = 0.5 * (psi[k - nx] + psi[k]) * (f[k - nx] - f[k]); acc = have ? acc + t : t; have = 1; }
    if (j < nx - 1) { const double t = 0.5 * (psi[k + 1] + psi[k]) * (f[k + 1] - f[k]); acc = have ? acc + t : t; have = 1; }
    if (j > 0) { const double t = 0.5 * (psi[k - 1] + psi[k]) * (f[k - 1] - f[k]); acc = have ? acc + t : t; have = 1; }
    return acc;
}

static void single_scale(const double *I, double *u, double *v, int nx, int ny, int frames, double alpha, double gamma, double TOL,
                         int inner_iter, int outer_iter, int order, int f32, int *iters)
{
    const int nz = frames - 1, df = nx * ny, size = df * frames, size1 = df * nz;
    enum { NA = 26 };
    double *a[NA];
    for (int q = 0; q < NA; q++) a[q] = dalloc((size_t) size1);
    double *du = a[0], *dv = a[1], *ux = a[2], *uy = a[3], *ut = a[4], *vx = a[5], *vy = a[6], *vt = a[7];
    double *Iw = a[8], *Iwx = a[9], *Iwy = a[10], *Ixx = a[11], *Iyy = a[12], *Ixy = a[13];
    double *Iwxx = a[14], *Iwyy = a[15], *Iwxy = a[16], *div_u = a[17], *div_v = a[18], *div_d = a[19];
    double *Au = a[20], *Av = a[21], *Du = a[22], *Dv = a[23], *D = a[24], *psis = a[25];
    double *Ix = dalloc((size_t) size), *Iy = dalloc((size_t) size);
    int solve = 0;

    for (int f = 0; f < frames; f++) orc_centered_gradient(I + (size_t) f * df, Ix + (size_t) f * df, Iy + (size_t) f * df, nx, ny);
    for (int f = 0; f < nz; f++) {
        orc_dxx(I + (size_t) df * (f + 1), Ixx + (size_t) f * df, nx, ny);
        orc_dyy(I + (size_t) df * (f + 1), Iyy + (size_t) f * df, nx, ny);
        orc_dxy(I + (size_t) df * (f + 1), Ixy + (size_t) f * df, nx, ny);
    }
    if (f32) {                                     /* k_brox_prepare: G1, PA, PB */
        round_f32(Ix, (size_t) size);
        round_f32(Iy, (size_t) size);
        round_f32(Ixx, (size_t) size1);
        round_f32(Iyy, (size_t) size1);
        round_f32(Ixy, (size_t) size1);
    }
    for (int no = 0; no < outer_iter; no++) {
        for (int f = 0; f < nz; f++) {
            const size_t o = (size_t) f * df, o1 = (size_t) df * (f + 1);
            orc_bicubic_warp(I + o1, u + o, v + o, Iw + o, nx, ny, 1);
            orc_bicubic_warp(Ix + o1, u + o, v + o, Iwx + o, nx, ny, 1);
            orc_bicubic_warp(Iy + o1, u + o, v + o, Iwy + o, nx, ny, 1);
            orc_bicubic_warp(Ixx + o, u + o, v + o, Iwxx + o, nx, ny, 1);
            orc_bicubic_warp(Ixy + o, u + o, v + o, Iwxy + o, nx, ny, 1);
            orc_bicubic_warp(Iyy + o, u + o, v + o, Iwyy + o, nx, ny, 1);
        }
        if (f32) {                                 /* k_brox_warp: WA, WB */
            round_f32(Iw, (size_t) size1);
            round_f32(Iwx, (size_t) size1);
            round_f32(Iwy, (size_t) size1);
            round_f32(Iwxx, (size_t) size1);
            round_f32(Iwxy, (size_t) size1);
            round_f32(Iwyy, (size_t) size1);
        }
        orc_centered_gradient3(u, ux, uy, ut, nx, ny, nz);
        orc_centered_gradient3(v, vx, vy, vt, nx, ny, nz);
        for (int i = 0; i < size1; i++) {
            const double gu = ux[i] * ux[i] + uy[i] * uy[i] + ut[i] * ut[i];
            const double gv = vx[i] * vx[i] + vy[i] * vy[i] + vt[i] * vt[i];
            const double d2 = gu + gv;
            psis[i] = ST32(1. / sqrt(d2 + EPSILON * EPSILON));               /* k_broxt_psis: Psis */
        }
        /* the divergence of the flow: the in-frame sum, then `+=` the temporal terms as ONE added expression; div_d */
        for (int f = 0; f < nz; f++)
            for (int i = 0; i < ny; i++)
                for (int j = 0; j < nx; j++) {
                    const int k = f * df + i * nx + j;
                    const double *ps = psis + (size_t) f * df;
                    double au = div_at(u + (size_t) f * df, ps, i, j, nx, ny), av = div_at(v + (size_t) f * df, ps, i, j, nx, ny);
                    const double psi5 = (f > 0) ? 0.5 * (psis[k - df] + psis[k]) : 0;
                    const double psi6 = (f < nz - 1) ? 0.5 * (psis[k + df] + psis[k]) : 0;
                    if (nz > 1) {
                        if (f > 0 && f < nz - 1) {
                            au += psi5 * (u[k - df] - u[k]) + psi6 * (u[k + df] - u[k]);
                            av += psi5 * (v[k - df] - v[k]) + psi6 * (v[k + df] - v[k]);
                        } else if (f == 0) {
                            au += psi6 * (u[k + df] - u[k]);
                            av += psi6 * (v[k + df] - v[k]);
                        } else {
                            au += psi5 * (u[k - df] - u[k]);
                            av += psi5 * (v[k - df] - v[k]);
                        }
                    }
                    div_u[k] = ST32(au);                                       /* k_broxt_div: DV, Dd */
                    div_v[k] = ST32(av);
                    const int kk = i * nx + j;
                    const double psi1 = (i < ny - 1) ? 0.5 * (ps[kk + nx] + ps[kk]) : 0;
                    const double psi2 = (i > 0) ? 0.5 * (ps[kk - nx] + ps[kk]) : 0;
                    const double psi3 = (j < nx - 1) ? 0.5 * (ps[kk + 1] + ps[kk]) : 0;
                    const double psi4 = (j > 0) ? 0.5 * (ps[kk - 1] + ps[kk]) : 0;
                    div_d[k] = ST32(alpha * (psi1 + psi2 + psi3 + psi4 + psi5 + psi6));
                    du[k] = dv[k] = 0;
                }
        for (int ni = 0; ni < inner_iter; ni++) {
            for (int i = 0; i < size1; i++) {
                const double dI = Iw[i] - I[i] + Iwx[i] * du[i] + Iwy[i] * dv[i];
                const double dI2 = dI * dI;
                const double p = ST32(1. / sqrt(dI2 + EPSILON * EPSILON));    /* brox_coeff_px: rnd_to(psid), rnd_to(psig) */
                const double dIx = Iwx[i] - Ix[i] + Iwxx[i] * du[i] + Iwxy[i] * dv[i];
                const double dIy = Iwy[i] - Iy[i] + Iwxy[i] * du[i] + Iwyy[i] * dv[i];
                const double dG2 = dIx * dIx + dIy * dIy;
                const double g = gamma * ST32(1. / sqrt(dG2 + EPSILON * EPSILON));
                const double dif = Iw[i] - I[i];
                const double BNu = -p * dif * Iwx[i];
                const double BNv = -p * dif * Iwy[i];
                const double BDu = p * Iwx[i] * Iwx[i];
                const double BDv = p * Iwy[i] * Iwy[i];
                const double dx = (Iwx[i] - Ix[i]);
                const double dy = (Iwy[i] - Iy[i]);
                const double GNu = -g * (dx * Iwxx[i] + dy * Iwxy[i]);
                const double GNv = -g * (dx * Iwxy[i] + dy * Iwyy[i]);
                const double GDu = g * (Iwxx[i] * Iwxx[i] + Iwxy[i] * Iwxy[i]);
                const double GDv = g * (Iwyy[i] * Iwyy[i] + Iwxy[i] * Iwxy[i]);
                const double DI = (Iwxx[i] + Iwyy[i]) * Iwxy[i];
                Au[i] = ST32(BNu + GNu + alpha * div_u[i]);                     /* brox_coeff_px: CO, Dm */
                Av[i] = ST32(BNv + GNv + alpha * div_v[i]);
                Du[i] = ST32(BDu + GDu + div_d[i]);
                Dv[i] = ST32(BDv + GDv + div_d[i]);
                D[i] = ST32(p * Iwy[i] * Iwx[i] + g * DI);
            }
            const Sys S = {Au, Av, Du, Dv, D, psis, du, dv, alpha, nx, ny, nz, f32};
            double error = 1000;
            int nsor = 0;
            while (error > TOL && nsor < MAXITER) {
                nsor++;
                error = sqrt(sweep(&S, order) / size1);
            }
            if (iters) iters[solve] = nsor;
            solve++;
        }
        for (int i = 0; i < size1; i++) { u[i] = ST32(u[i] + du[i]); v[i] = ST32(v[i] + dv[i]); }     /* k_brox_add: U */
    }
    for (int q = 0; q < NA; q++) free(a[q]);
    free(Ix);
    free(Iy);
}

/* u, v: (frames - 1) * nx * ny; iters: [scale][outer * inner].  1 = "sigma too large", 2 = frames <= 2. */
int broxt_colour_ref_mode(const double *I, double *u, double *v, int nxx, int nyy, int frames, double alpha, double gamma, int nscales,
                          double nu, double TOL, int inner_iter, int outer_iter, int order, int store_f32, int *iters)
{
    const int f32 = store_f32;
    if (frames <= 2) return 2;
    int *nx = (int *) malloc(sizeof(int) * nscales), *ny = (int *) malloc(sizeof(int) * nscales);
    double **Is = (double **) calloc(nscales, sizeof(double *));
    double **us = (double **) calloc(nscales, sizeof(double *)), **vs = (double **) calloc(nscales, sizeof(double *));
    int rc = 0;
    nx[0] = nxx;
    ny[0] = nyy;
    Is[0] = dalloc((size_t) nxx * nyy * frames);
    if (f32) {                                     /* the upload into float planes, then op_normalize_*_in<float> */
        const size_t n0 = (size_t) nxx * nyy * frames;
        double *Ir = dalloc(n0);
        for (size_t i = 0; i < n0; i++) Ir[i] = rnd_f32(I[i]);
        orc_image_normalization_1(Ir, Is[0], nxx * nyy * frames);
        round_f32(Is[0], n0);
        free(Ir);
    } else
        orc_image_normalization_1(I, Is[0], nxx * nyy * frames);
    for (int f = 0; f < frames; f++)
        rc |= f32 ? orc_gaussian_mode(Is[0] + (size_t) f * nxx * nyy, nxx, nyy, SIGMA, 1)
                  : orc_gaussian(Is[0] + (size_t) f * nxx * nyy, nxx, nyy, SIGMA);
    us[0] = u;
    vs[0] = v;
    for (int s = 1; s < nscales && !rc; s++) {
        orc_zoom_size(nx[s - 1], ny[s - 1], &nx[s], &ny[s], nu);
        const size_t n = (size_t) nx[s] * ny[s];
        Is[s] = dalloc(n * frames);
        us[s] = dalloc(n * (frames - 1));
        vs[s] = dalloc(n * (frames - 1));
        for (int f = 0; f < frames; f++)
            rc |= f32 ? orc_zoom_out_mode(Is[s - 1] + (size_t) f * nx[s - 1] * ny[s - 1], Is[s] + f * n, nx[s - 1], ny[s - 1], nu, 1)
                      : orc_zoom_out(Is[s - 1] + (size_t) f * nx[s - 1] * ny[s - 1], Is[s] + f * n, nx[s - 1], ny[s - 1], nu);
    }
    if (!rc) {
        const int c = nscales - 1;
        for (int i = 0; i < nx[c] * ny[c] * (frames - 1); i++) us[c][i] = vs[c][i] = 0.0;
        for (int s = nscales - 1; s >= 0; s--) {
            single_scale(Is[s], us[s], vs[s], nx[s], ny[s], frames, alpha, gamma, TOL, inner_iter, outer_iter, order, f32,
                         iters ? iters + s * inner_iter * outer_iter : NULL);
            if (s) {
                const size_t n = (size_t) nx[s] * ny[s], n1 = (size_t) nx[s - 1] * ny[s - 1];
                for (int f = 0; f < frames - 1; f++) {
                    orc_zoom_in(us[s] + f * n, us[s - 1] + f * n1, nx[s], ny[s], nx[s - 1], ny[s - 1]);
                    orc_zoom_in(vs[s] + f * n, vs[s - 1] + f * n1, nx[s], ny[s], nx[s - 1], ny[s - 1]);
                }
                for (size_t i = 0; i < n1 * (frames - 1); i++) {
                    us[s - 1][i] = ST32(us[s - 1][i] * (1.0 / nu));             /* k_zoom_in_flow: one rounding, after the product */
                    vs[s - 1][i] = ST32(vs[s - 1][i] * (1.0 / nu));
                }
            }
        }
    }
    for (int s = 0; s < nscales; s++) {
        free(Is[s]);
        if (s) { free(us[s]); free(vs[s]); }
    }
    free(Is);
    free(us);
    free(vs);
    free(nx);
    free(ny);
    return rc;
}

/* double storage: the entry as it was */
int broxt_colour_ref(const double *I, double *u, double *v, int nxx, int nyy, int frames, double alpha, double gamma, int nscales,
                     double nu, double TOL, int inner_iter, int outer_iter, int order, int *iters)
{
    return broxt_colour_ref_mode(I, u, v, nxx, nyy, frames, alpha, gamma, nscales, nu, TOL, inner_iter, outer_iter, order, 0, iters);
}
