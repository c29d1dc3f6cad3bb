// ofx_motion.hip -- the dominant motion of a flow: a translation, similarity or affine model fitted to a .flo payload by iteratively
// re-weighted least squares with Tukey's biweight (Odobez, Bouthemy, "Robust multiresolution estimation of parametric motion
// models", JVCIR 1995), as Wang, Schmid, "Action recognition with improved trajectories" (ICCV 2013) use it on dense trajectories:
// the model's flow is the camera's part of the motion, the residual the scene's, the pixels that disagree the moving foreground
// (ofx_flow_motion_fit_dev, ofx_flow_motion_apply_dev).
//
// All arithmetic in double, every operation rounded (the build's -ffp-contract=off), division correctly rounded, association as
// written in include/ofx.h:
//     cx = 0.5 * (nx - 1);  cy = 0.5 * (ny - 1);  h = 0.5 * max(nx, ny);  X = (j - cx) / h;  Y = (i - cy) / h
//     mu = (t0 + a * X) + b * Y;  mv = (t1 + c * X) + d * Y
//     valid = map byte 0 and u - u == 0 and v - v == 0
//     du = u - mu;  dv = v - mv;  r2 = du * du + dv * dv;  C2 = C * C;  r2 < C2: q = 1 - r2 / C2, w = q * q;  else w = 0
//     the twelve moments of ofx.h, each sum64 (ofx_sum64.h) over the rows of sum64 over a row's terms; an invalid pixel's term is +0.0
// Pure functions of the payload floats, the map bytes and the record doubles: the same bytes in every storage precision.
#include "ofx_device.h"
#include "ofx_ops.h"
#include "ofx_pairs.h"
#include "ofx_sum64.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <map>

#define MO_NM 12                                 // moments: S1 SX SY SXX SXY SYY U1 UX UY V1 VX VY
#define MO_EPS 1e-12

struct OfxMotionSlots {
    const float2        *flo[OFX_MAX_GROUP];     // may be the slot's resid: no __restrict__
    const unsigned char *occ[OFX_MAX_GROUP];     // NULL: all valid
    const double        *init[OFX_MAX_GROUP];    // NULL: fit 0 is unweighted and starts from zeros
    double              *rec[OFX_MAX_GROUP];     // the record; [15] is the stop flag that the kernels of the later fits read
    float2              *model[OFX_MAX_GROUP];   // NULL: not wanted
    float2              *resid[OFX_MAX_GROUP];
    unsigned char       *inl[OFX_MAX_GROUP];
};

struct MoGrid { double cx, cy, h; };
OFX_DEV MoGrid mo_grid(int nx, int ny)
{
    MoGrid g;
    g.cx = 0.5 * (double) (nx - 1);
    g.cy = 0.5 * (double) (ny - 1);
    g.h = 0.5 * (double) (nx > ny ? nx : ny);
    return g;
}
OFX_DEV bool mo_finite(double u, double v) { return u - u == 0.0 && v - v == 0.0; }

// ---- the moments of a row ---------------------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup; slot z = blockIdx.y.  Lane l takes the columns l, l + 64, ... left to right, the first
// half of sum64 on terms that never reach memory: twelve running sums in registers, started at -0.0 so that the first addition
// leaves the first term's bits (a lane without a column holds +0.0).  The payload is read once, one float2 per lane and round: 512
// contiguous bytes per wave; the map one byte per lane.  An invalid pixel adds +0.0 by a select, so a NaN vector poisons nothing.
// Fit `fit` of the call: fit 0 is weighted from the slot's initial record where it has one, the later fits from the record that
// the solve of the fit before left, unless that record's stop flag is set: then the slot's waves leave at once.
// rows[(z * 12 + m) * ny + i] receives moment m of row i.
__global__ __launch_bounds__(256) void k_motion_rows(OfxMotionSlots P, double *__restrict__ rows, int fit, double c_init, double c_plain,
                                                     int nx, int ny)
{
    const int z = blockIdx.y, i = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (i >= ny) return;                                                     // the same in all lanes of a wave
    const double *init = P.init[z];
    const double *from = fit == 0 ? init : P.rec[z];
    if (fit > 0 && from[15] != 0.0) return;                                  // stopped on a degenerate fit: the same in all lanes
    const bool weighted = from != nullptr;
    const double C = init ? c_init : c_plain, C2 = C * C;
    double t0 = 0.0, a = 0.0, b = 0.0, t1 = 0.0, c = 0.0, d = 0.0;
    if (weighted) { t0 = from[0]; a = from[1]; b = from[2]; t1 = from[3]; c = from[4]; d = from[5]; }
    const MoGrid g = mo_grid(nx, ny);
    const double Y = ((double) i - g.cy) / g.h;
    const float2 *flo = P.flo[z] + (size_t) i * nx;
    const unsigned char *occ = P.occ[z] ? P.occ[z] + (size_t) i * nx : nullptr;
    const int l = (int) threadIdx.x & 63;
    double s[MO_NM];
#pragma unroll
    for (int m = 0; m < MO_NM; m++) s[m] = l < nx ? -0.0 : 0.0;
    for (int j = l; j < nx; j += 64) {
        const float2 f = flo[j];
        const double u = (double) f.x, v = (double) f.y;
        const bool valid = !(occ && occ[j] != 0) && mo_finite(u, v);
        const double X = ((double) j - g.cx) / g.h;
        double w = 1.0;
        if (weighted) {
            const double mu = (t0 + a * X) + b * Y, mv = (t1 + c * X) + d * Y;
            const double du = u - mu, dv = v - mv;
            const double r2 = du * du + dv * dv;
            const double q = 1.0 - r2 / C2;
            w = r2 < C2 ? q * q : 0.0;
        }
        const double wX = w * X, wY = w * Y, wu = w * u, wv = w * v;
        const double t[MO_NM] = {w, wX, wY, wX * X, wX * Y, wY * Y, wu, wu * X, wu * Y, wv, wv * X, wv * Y};
#pragma unroll
        for (int m = 0; m < MO_NM; m++) s[m] = s[m] + (valid ? t[m] : 0.0);
    }
#pragma unroll
    for (int m = 0; m < MO_NM; m++) {
        const double r = tk_sum64_lanes(s[m]);
        if (l == 0) rows[((size_t) z * MO_NM + m) * ny + i] = r;
    }
}

// ---- the solve --------------------------------------------------------------------------------------------------------------------
// the normal equations of ofx.h, without pivoting; false where a pivot test fails (a NaN fails every test)
OFX_DEV bool mo_solve(int model, const double *S, double *th)
{
    const double S1 = S[0], SX = S[1], SY = S[2], SXX = S[3], SXY = S[4], SYY = S[5];
    const double U1 = S[6], UX = S[7], UY = S[8], V1 = S[9], VX = S[10], VY = S[11];
    if (!(S1 > 0.0)) return false;
    if (model == OFX_MOTION_TRANSLATION) {
        th[0] = U1 / S1; th[1] = 0.0; th[2] = 0.0;
        th[3] = V1 / S1; th[4] = 0.0; th[5] = 0.0;
        return true;
    }
    if (model == OFX_MOTION_SIMILARITY) {
        const double Q = SXX + SYY;
        const double D = Q - (SX * SX + SY * SY) / S1;
        if (!(D > MO_EPS * Q)) return false;
        const double a = ((UX + VY) - (SX * U1 + SY * V1) / S1) / D;
        const double c = ((VX - UY) - (SX * V1 - SY * U1) / S1) / D;
        th[0] = ((U1 - SX * a) + SY * c) / S1; th[1] = a; th[2] = -c;
        th[3] = ((V1 - SY * a) - SX * c) / S1; th[4] = c; th[5] = a;
        return true;
    }
    const double l10 = SX / S1, l20 = SY / S1;
    const double a11 = SXX - l10 * SX, a12 = SXY - l10 * SY, a22 = SYY - l20 * SY;
    if (!(a11 > MO_EPS * SXX)) return false;
    const double l21 = a12 / a11;
    const double p2 = a22 - l21 * a12;
    if (!(p2 > MO_EPS * SYY)) return false;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const double r0 = S[6 + 3 * k], r1 = S[7 + 3 * k], r2 = S[8 + 3 * k];
        const double y1 = r1 - l10 * r0;
        const double y2 = (r2 - l20 * r0) - l21 * y1;
        const double z2 = y2 / p2;
        const double z1 = (y1 - a12 * z2) / a11;
        th[3 * k] = ((r0 - SX * z1) - SY * z2) / S1;
        th[3 * k + 1] = z1;
        th[3 * k + 2] = z2;
    }
    return true;
}

// One wave per slot: sum64 over the row sums of each moment, then lane 0 solves and writes the whole record.  A degenerate fit
// leaves the theta that the fit started from, the S1 and the count of the last completed fit, and sets the stop flag.
__global__ __launch_bounds__(64) void k_motion_solve(OfxMotionSlots P, const double *__restrict__ rows, int fit, int model, double c_last,
                                                     int nx, int ny)
{
    const int z = blockIdx.x;
    double *rec = P.rec[z];
    if (fit > 0 && rec[15] != 0.0) return;                                   // the same in all lanes
    double S[MO_NM];
#pragma unroll
    for (int m = 0; m < MO_NM; m++) S[m] = tk_sum64(rows + ((size_t) z * MO_NM + m) * ny, ny);
    if (threadIdx.x != 0) return;
    const double *from = fit == 0 ? P.init[z] : rec;
    double th[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (from)
        for (int k = 0; k < 6; k++) th[k] = from[k];
    double s1 = fit == 0 ? 0.0 : rec[12], done = fit == 0 ? 0.0 : rec[13], stop = 1.0;
    double nt[6];
    if (mo_solve(model, S, nt)) {
        for (int k = 0; k < 6; k++) th[k] = nt[k];
        s1 = S[0];
        done = (double) (fit + 1);
        stop = 0.0;
    }
    const MoGrid g = mo_grid(nx, ny);
    for (int k = 0; k < 2; k++) {
        const double p1 = th[3 * k + 1] / g.h, p2 = th[3 * k + 2] / g.h;
        rec[3 * k] = th[3 * k];
        rec[3 * k + 1] = th[3 * k + 1];
        rec[3 * k + 2] = th[3 * k + 2];
        rec[6 + 3 * k] = (th[3 * k] - p1 * g.cx) - p2 * g.cy;
        rec[7 + 3 * k] = p1;
        rec[8 + 3 * k] = p2;
    }
    rec[12] = s1;
    rec[13] = done;
    rec[14] = c_last;
    rec[15] = stop;
}

// ---- the outputs ------------------------------------------------------------------------------------------------------------------
// A thread owns a pixel, slot z = blockIdx.y: the model's vector, the residual and the inlier byte under theta = rec[0 .. 5] and the
// cut-off C.  A pixel reads only its own element of the payload, before it writes: resid == flo is safe.  Map bytes are stored one
// per lane, 64 contiguous bytes per wave at whatever address the map has; no byte outside a destination is written.
__global__ __launch_bounds__(256) void k_motion_out(OfxMotionSlots P, double C, int nx, int ny)
{
    const int z = blockIdx.y;
    const long long p = (long long) blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long) nx * ny) return;
    float2 *model = P.model[z], *resid = P.resid[z];
    unsigned char *inl = P.inl[z];
    if (!model && !resid && !inl) return;
    const double *rec = P.rec[z];
    const int i = (int) (p / nx), j = (int) (p - (long long) i * nx);
    const MoGrid g = mo_grid(nx, ny);
    const double X = ((double) j - g.cx) / g.h, Y = ((double) i - g.cy) / g.h;
    const double mu = (rec[0] + rec[1] * X) + rec[2] * Y, mv = (rec[3] + rec[4] * X) + rec[5] * Y;
    if (model) model[p] = make_float2((float) mu, (float) mv);
    if (!resid && !inl) return;
    const float2 f = P.flo[z][p];
    const double u = (double) f.x, v = (double) f.y;
    const double du = u - mu, dv = v - mv;
    if (resid) resid[p] = make_float2((float) du, (float) dv);
    if (inl) {
        const bool valid = !(P.occ[z] && P.occ[z][p] != 0) && mo_finite(u, v);
        const double r2 = du * du + dv * dv;
        inl[p] = valid && r2 < C * C ? 0 : 255;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static bool mo_misaligned(const void *p, size_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }
static const void *mo_at(const void *const *t, int g) { return t ? t[g] : nullptr; }
static void *mo_at(void *const *t, int g) { return t ? t[g] : nullptr; }

static int mo_check_size(ofx_ctx *ctx, const char *who, int n, int nx, int ny)
{
    if (n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n = %d (at least 1)", who, n);
    if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: flow field %dx%d too small", who, nx, ny);
    if ((long long) nx * ny > (long long) INT_MAX - 2048) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %dx%d pixels do not fit an int", who, nx, ny);
    return OFX_OK;
}
static int mo_check_cutoff(ofx_ctx *ctx, const char *who, const char *name, double c)
{
    if (!std::isfinite(c) || !(c > 0.0)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %s = %g (finite, above 0)", who, name, c);
    return OFX_OK;
}
// Alignment and aliases of the tables that both entries share.  `rec_in`: the records that the call reads (the fit entry's initial
// records, the apply entry's records); `rec_out`: the fit entry's records, outputs like the three others.
static int mo_check_slots(ofx_ctx *ctx, const char *who, int n, const void *const *d_flo, const void *const *d_occ,
                          const void *const *rec_in, void *const *rec_out, void *const *d_flo_model, void *const *d_flo_resid,
                          void *const *d_inlier)
{
    std::map<const void *, int> in;                                          // how many slots read a buffer
    for (int g = 0; g < n; g++) {
        const void *ins[3] = {mo_at(d_flo, g), mo_at(d_occ, g), mo_at(rec_in, g)};
        if (mo_misaligned(ins[0], sizeof(float2)) || mo_misaligned(mo_at(d_flo_model, g), sizeof(float2)) ||
            mo_misaligned(mo_at(d_flo_resid, g), sizeof(float2)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a payload of slot %d is not 8-byte aligned", who, g);
        if (mo_misaligned(ins[2], sizeof(double)) || mo_misaligned(mo_at(rec_out, g), sizeof(double)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a record of slot %d is not 8-byte aligned", who, g);
        for (int k = 0; k < 3; k++)
            if (ins[k]) in[ins[k]]++;
    }
    for (int g = 0; g < n; g++) {
        const void *flo = mo_at(d_flo, g);
        const void *o[4] = {mo_at(rec_out, g), mo_at(d_flo_model, g), mo_at(d_flo_resid, g), mo_at(d_inlier, g)};
        for (int a = 0; a < 4; a++) {
            if (!o[a]) continue;
            // the residual in place: a pixel reads only its own element, as long as no other slot reads the payload too
            const bool in_place = a == 2 && o[a] == flo && in[flo] == 1;
            if (in.count(o[a]) && !in_place)
                return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination of slot %d is a buffer that the call reads", who, g);
            for (int b = a + 1; b < 4; b++)
                if (o[a] == o[b]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: two destinations of slot %d are the same buffer", who, g);
        }
    }
    return OFX_OK;
}

// the staged buffers of a launch's slots: what to copy back
struct MoStaged { void *rec, *model, *resid, *inl; };
static int mo_stage_slot(ofx_ctx *ctx, OfxMotionSlots &S, MoStaged &st, int z, const void *flo, const void *occ, const void *init,
                         void *rec, bool rec_is_input, void *model, void *resid, void *inl, size_t px)
{
    void *f, *o, *i0;
    OFX_TRY(ofx_stage_in(ctx, flo, px * sizeof(float2), true, &f));
    OFX_TRY(ofx_stage_in(ctx, occ, px, true, &o));
    OFX_TRY(ofx_stage_in(ctx, init, OFX_MOTION_REC * sizeof(double), true, &i0));
    OFX_TRY(ofx_stage_in(ctx, rec, OFX_MOTION_REC * sizeof(double), rec_is_input, &st.rec));
    OFX_TRY(ofx_stage_in(ctx, model, px * sizeof(float2), false, &st.model));
    // in place: the payload's stage is filled and receives the residual too
    if (resid && resid == flo) st.resid = f; else OFX_TRY(ofx_stage_in(ctx, resid, px * sizeof(float2), false, &st.resid));
    OFX_TRY(ofx_stage_in(ctx, inl, px, false, &st.inl));
    S.flo[z] = static_cast<const float2 *>(f);
    S.occ[z] = static_cast<const unsigned char *>(o);
    S.init[z] = static_cast<const double *>(i0);
    S.rec[z] = static_cast<double *>(st.rec);
    S.model[z] = static_cast<float2 *>(st.model);
    S.resid[z] = static_cast<float2 *>(st.resid);
    S.inl[z] = static_cast<unsigned char *>(st.inl);
    return OFX_OK;
}
static int mo_launch_out(ofx_ctx *ctx, int slots, const OfxMotionSlots &S, double C, int nx, int ny)
{
    const int blocks = (int) (((long long) nx * ny + 255) / 256);
    hipLaunchKernelGGL(k_motion_out, dim3(blocks, slots), dim3(256), 0, ctx->stream, S, C, nx, ny);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
static int mo_stage_back(ofx_ctx *ctx, const MoStaged &st, void *model, void *resid, void *inl, size_t px)
{
    if (model) OFX_TRY(ofx_stage_out(ctx, model, st.model, px * sizeof(float2)));
    if (resid) OFX_TRY(ofx_stage_out(ctx, resid, st.resid, px * sizeof(float2)));
    if (inl) OFX_TRY(ofx_stage_out(ctx, inl, st.inl, px));
    return OFX_OK;
}

// Per chunk of OFX_MAX_GROUP slots: n_fits times the row kernel and the solve, then the outputs.  The schedule is the device's: a
// slot that stopped on a degenerate fit is skipped by the kernels of the later fits through its record's flag; nothing is awaited.
extern "C" int ofx_flow_motion_fit_dev(ofx_ctx *ctx, int n, const void *const *d_flo, const void *const *d_occ,
                                       const void *const *d_motion_init, void *const *d_motion, int model, int n_fits, double c_first,
                                       double c_last, void *const *d_flo_model, void *const *d_flo_resid, void *const *d_inlier, int nx,
                                       int ny)
{
    OFX_ENTER(ctx);
    const char *who = "flow_motion_fit";
    if (!d_flo || !d_motion) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    OFX_TRY(mo_check_size(ctx, who, n, nx, ny));
    if (n_fits < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_fits = %d (at least 1)", who, n_fits);
    if (model != OFX_MOTION_TRANSLATION && model != OFX_MOTION_SIMILARITY && model != OFX_MOTION_AFFINE)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: model = %d (2, 4 or 6 parameters)", who, model);
    OFX_TRY(mo_check_cutoff(ctx, who, "c_first", c_first));
    OFX_TRY(mo_check_cutoff(ctx, who, "c_last", c_last));
    if (c_first < c_last) return ofx_fail(ctx, OFX_ERR_ARG, "%s: c_first = %g is below c_last = %g", who, c_first, c_last);
    for (int g = 0; g < n; g++)
        if (!d_flo[g] || !d_motion[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
    OFX_TRY(mo_check_slots(ctx, who, n, d_flo, d_occ, d_motion_init, d_motion, d_flo_model, d_flo_resid, d_inlier));
    const size_t px = (size_t) nx * ny;
    const int per = n < OFX_MAX_GROUP ? n : OFX_MAX_GROUP;
    double *rows;
    OFX_TRY(ofx_alloc(ctx, (size_t) per * MO_NM * ny, &rows));
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxMotionSlots S = {};
        MoStaged st[OFX_MAX_GROUP];
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            OFX_TRY(mo_stage_slot(ctx, S, st[z], z, d_flo[g], mo_at(d_occ, g), mo_at(d_motion_init, g), d_motion[g], false,
                                  mo_at(d_flo_model, g), mo_at(d_flo_resid, g), mo_at(d_inlier, g), px));
        }
        for (int f = 0; f < n_fits; f++) {
            // the cut-off of weighted fit t: a slot with an initial record is at t = f, one without at t = f - 1 (its fit 0 is unweighted)
            const double c_init = std::fmax(c_last, std::ldexp(c_first, -f));
            const double c_plain = std::fmax(c_last, std::ldexp(c_first, f > 0 ? 1 - f : 0));
            hipLaunchKernelGGL(k_motion_rows, dim3(ofx_cdiv(ny, 4), cnt), dim3(256), 0, ctx->stream, S, rows, f, c_init, c_plain, nx, ny);
            OFX_LAUNCH_CHECK(ctx);
            hipLaunchKernelGGL(k_motion_solve, dim3(cnt), dim3(64), 0, ctx->stream, S, rows, f, model, c_last, nx, ny);
            OFX_LAUNCH_CHECK(ctx);
        }
        OFX_TRY(mo_launch_out(ctx, cnt, S, c_last, nx, ny));
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            OFX_TRY(ofx_stage_out(ctx, d_motion[g], st[z].rec, OFX_MOTION_REC * sizeof(double)));
            OFX_TRY(mo_stage_back(ctx, st[z], mo_at(d_flo_model, g), mo_at(d_flo_resid, g), mo_at(d_inlier, g), px));
        }
    }
    return OFX_OK;
}

extern "C" int ofx_flow_motion_apply_dev(ofx_ctx *ctx, int n, const void *const *d_motion, const void *const *d_flo,
                                         const void *const *d_occ, double cutoff, void *const *d_flo_model, void *const *d_flo_resid,
                                         void *const *d_inlier, int nx, int ny)
{
    OFX_ENTER(ctx);
    const char *who = "flow_motion_apply";
    if (!d_motion) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    OFX_TRY(mo_check_size(ctx, who, n, nx, ny));
    OFX_TRY(mo_check_cutoff(ctx, who, "cutoff", cutoff));
    for (int g = 0; g < n; g++) {
        if (!d_motion[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        if ((mo_at(d_flo_resid, g) || mo_at(d_inlier, g)) && !mo_at(d_flo, g))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: slot %d asks for a residual or a map without a payload", who, g);
    }
    OFX_TRY(mo_check_slots(ctx, who, n, d_flo, d_occ, d_motion, nullptr, d_flo_model, d_flo_resid, d_inlier));
    const size_t px = (size_t) nx * ny;
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxMotionSlots S = {};
        MoStaged st[OFX_MAX_GROUP];
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            OFX_TRY(mo_stage_slot(ctx, S, st[z], z, mo_at(d_flo, g), mo_at(d_occ, g), nullptr, const_cast<void *>(d_motion[g]), true,
                                  mo_at(d_flo_model, g), mo_at(d_flo_resid, g), mo_at(d_inlier, g), px));
        }
        OFX_TRY(mo_launch_out(ctx, cnt, S, cutoff, nx, ny));
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            OFX_TRY(mo_stage_back(ctx, st[z], mo_at(d_flo_model, g), mo_at(d_flo_resid, g), mo_at(d_inlier, g), px));
        }
    }
    return OFX_OK;
}
