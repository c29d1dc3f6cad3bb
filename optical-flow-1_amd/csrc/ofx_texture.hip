// ofx_texture.hip -- the structure-texture decomposition of device-resident frames (ofx_structure_texture_dev): the ROF structure
// part S of a frame by n_iter steps of Chambolle's projection, and the texture part T = f - alpha S (Wedel, Pock, Zach, Bischof,
// Cremers, "An Improved Algorithm for TV-L1 Optical Flow", 2009, section 3.1).
//
// A frame is ny rows of nx samples of the context's "input" kind, read under "input_pitch" through the loaders of ofx_device.h
// (ldw).  All arithmetic in double, every operation rounded (the build's -ffp-contract=off), association as written in
// include/ofx.h:
//     u        = f + theta * divergence(p1, p2)            src/operators.cpp:36-78, its border associations (st_div)
//     (ux, uy) = forward_gradient(u)                       src/operators.cpp:87-125
//     g        = 1.0 + r * sqrt(ux * ux + uy * uy);  p1 = (p1 + r * ux) / g;  p2 = (p2 + r * uy) / g
// The duals live in double between launches whatever the storage precision.
#include "ofx_device.h"
#include "ofx_ops.h"
#include "ofx_pairs.h"

#include <climits>
#include <cmath>

// ---- the shape of a workgroup ------------------------------------------------------------------------------------------------------
// One workgroup of ST_NT threads holds an EXTENDED tile of ST_EW x ST_EH cells in LDS: p1, p2 and u, 24 B per cell.  A wave is one row
// of 64 cells, a thread owns the ST_Q cells of its column ST_RS rows apart and keeps their f, p1 and p2 in registers; LDS carries what
// the neighbours need (p1 of the left cell and p2 of the cell above for the divergence, u of the right cell and of the cell below
// for the gradient), two barriers per iteration.  The dependency cone of one iteration is one cell in every direction, so after k
// iterations the duals are right `k` cells inside the extended tile; a launch of k iterations writes the (ST_EW - 2k) x (ST_EH - 2k)
// cells in the middle.  The last launch of a call also needs S = f + theta div(p), one more cell to the left and above: its halo is
// k + 1 there.  The geometry is a run-time function of k: one kernel per source kind serves every "st_fuse".
// Rows that no output cell depends on any more are skipped, a wave at a time: the duals after iteration t (1 .. k) are needed in
// rows t .. ST_EH - t - 1 alone, so iteration t computes u in rows t .. ST_EH - t and the duals in rows t .. ST_EH - t - 1
// (measured 4 - 6 % faster at K = 4; columns are lanes of a wave and cost nothing).
// The border rules of both operators follow the IMAGE coordinates: a cell on the image's border never reads a cell outside it, so
// what cells outside the image hold (zeros, never loaded or stored) reaches no result.
#define ST_EW 64
#define ST_EH 48
#ifndef ST_NT
#define ST_NT 1024                              // measured against 512 and 256: 3 cells per thread, 54 VGPRs, 2 workgroups per CU
#endif
#define ST_RS (ST_NT / ST_EW)                   // rows between the cells of a thread
#define ST_Q  (ST_EW * ST_EH / ST_NT)           // cells per thread
#define ST_CELLS (ST_EW * ST_EH)

struct OfxTexSlots {
    const void    *src[OFX_MAX_GROUP];
    const double2 *pin[OFX_MAX_GROUP];     // the duals the launch starts from (not read by the first launch of a call: zeros)
    double2       *pout[OFX_MAX_GROUP];    // ... and leaves (not written by the last launch)
    void          *tex[OFX_MAX_GROUP];     // the last launch: T, and S where the slot has one
    void          *str[OFX_MAX_GROUP];
};

// divergence at a cell: c / l / u = the cell's own p1 and p2, p1 of its left neighbour, p2 of the one above.  The reference's
// associations: (p1c - p1l) + (p2c - p2u) inside; the first and last ROWS add p2c alone or subtract p2u alone; the first and last
// COLUMNS between them add p2c before they subtract p2u.  Selects, no branches: a - b is a + (-b) bit for bit.
OFX_DEV double st_div(double p1c, double p1l, double p2c, double p2u, bool L, bool R, bool T, bool B)
{
    const double a = L ? p1c : (R ? -p1l : p1c - p1l);
    const double y = T ? p2c : (B ? -p2u : p2c - p2u);
    const double side = (a + p2c) - p2u;
    return ((L || R) && !T && !B) ? side : a + y;
}

// k iterations from the duals in pin (first: from zeros) on the extended tile whose output region starts lo cells in and is
// ow x oh cells; fin: S and T go out instead of the duals.  f32: the destinations are float frames.
template <typename S>
__global__ __launch_bounds__(ST_NT) void k_structure_texture(OfxTexSlots P, int nx, int ny, size_t pitch, int tiles_x, int k, int lo,
                                                             int ow, int oh, int first, int fin, int f32, double theta, double r,
                                                             double alpha)
{
    // one cell of padding in front of p1, one row in front of p2 and behind u: the neighbour of a cell on the tile's edge is an
    // address inside the arrays (what lies there reaches no cell of the output region)
    __shared__ double s_p1[1 + ST_CELLS];
    __shared__ double s_p2[ST_EW + ST_CELLS];
    __shared__ double s_u[ST_CELLS + ST_EW];
    const int z = blockIdx.y, tid = threadIdx.x;
    const int tby = (int) blockIdx.x / tiles_x, tbx = (int) blockIdx.x - tby * tiles_x;
    const int cx = tid & (ST_EW - 1), cy0 = tid / ST_EW;
    const int j = tbx * ow - lo + cx, i0 = tby * oh - lo + cy0;
    const bool jin = j >= 0 && j < nx, L = j == 0, R = j == nx - 1;
    const char *__restrict__ src = static_cast<const char *>(P.src[z]);
    const double2 *__restrict__ pin = P.pin[z];

    double f[ST_Q], p1[ST_Q], p2[ST_Q];
#pragma unroll
    for (int q = 0; q < ST_Q; q++) {
        const int i = i0 + ST_RS * q, c = (cy0 + ST_RS * q) * ST_EW + cx;
        const bool in = jin && i >= 0 && i < ny;
        f[q] = 0.0; p1[q] = 0.0; p2[q] = 0.0;
        if (in) {
            f[q] = ldw(reinterpret_cast<const S *>(src + (size_t) i * pitch) + j);
            if (!first) {
                const double2 v = pin[(size_t) i * nx + j];
                p1[q] = v.x; p2[q] = v.y;
            }
        }
        s_p1[1 + c] = p1[q];
        s_p2[ST_EW + c] = p2[q];
    }
    if (tid == 0) s_p1[0] = 0.0;
    if (tid < ST_EW) { s_p2[tid] = 0.0; s_u[ST_CELLS + tid] = 0.0; }
    __syncthreads();

    for (int it = 0; it < k; it++) {
#pragma unroll
        for (int q = 0; q < ST_Q; q++) {
            const int cy = cy0 + ST_RS * q, i = i0 + ST_RS * q, c = cy * ST_EW + cx;
            if (!(cy > it && cy < ST_EH - it)) continue;                  // a dead row: see above
            s_u[c] = f[q] + theta * st_div(p1[q], s_p1[c], p2[q], s_p2[c], L, R, i == 0, i == ny - 1);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < ST_Q; q++) {
            const int cy = cy0 + ST_RS * q, i = i0 + ST_RS * q, c = cy * ST_EW + cx;
            if (!(cy > it && cy < ST_EH - it - 1)) continue;
            // every cell, those outside the image too: what they hold reaches no cell inside it, and g >= 1
            const double uc = s_u[c], dx = s_u[c + 1] - uc, dy = s_u[c + ST_EW] - uc;      // loads outside the selects: no branches
            const double ux = R ? 0.0 : dx;
            const double uy = i == ny - 1 ? 0.0 : dy;
            const double g = 1.0 + r * sqrt(ux * ux + uy * uy);
            p1[q] = (p1[q] + r * ux) / g;
            p2[q] = (p2[q] + r * uy) / g;
            s_p1[1 + c] = p1[q];
            s_p2[ST_EW + c] = p2[q];
        }
        __syncthreads();
    }

    const bool jout = jin && cx >= lo && cx < lo + ow;
#pragma unroll
    for (int q = 0; q < ST_Q; q++) {
        const int cy = cy0 + ST_RS * q, i = i0 + ST_RS * q, c = cy * ST_EW + cx;
        if (!(jout && cy >= lo && cy < lo + oh && i < ny)) continue;         // i >= 0: cy >= lo
        const size_t e = (size_t) i * nx + j;
        if (!fin) {
            P.pout[z][e] = make_double2(p1[q], p2[q]);
        } else {
            const double s = f[q] + theta * st_div(p1[q], s_p1[c], p2[q], s_p2[c], L, R, i == 0, i == ny - 1);
            const double t = f[q] - alpha * s;
            if (f32) {
                static_cast<float *>(P.tex[z])[e] = (float) t;
                if (P.str[z]) static_cast<float *>(P.str[z])[e] = (float) s;
            } else {
                static_cast<double *>(P.tex[z])[e] = t;
                if (P.str[z]) static_cast<double *>(P.str[z])[e] = s;
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the kernel's maximum of iterations per launch (include/ofx.h): its output region is then 47 x 31 cells of the 64 x 48
static_assert(ST_EW - 2 * OFX_ST_MAX_FUSE - 1 >= 16 && ST_EH - 2 * OFX_ST_MAX_FUSE - 1 >= 16, "an output region is left at the largest K");
// Option "st_fuse" = 0: what tools/bench_structure_texture.py measured fastest at 1920 x 1080 x 16 frames
#define ST_DEFAULT_FUSE 4

template <typename S>
static int st_launch(ofx_ctx *ctx, int slots, const OfxTexSlots &P, int nx, int ny, size_t pitch, int k, bool first, bool fin,
                     double theta, double r, double alpha)
{
    const int lo = fin ? k + 1 : k, ow = ST_EW - lo - k, oh = ST_EH - lo - k;
    const int tx = ofx_cdiv(nx, ow), ty = ofx_cdiv(ny, oh);
    hipLaunchKernelGGL((k_structure_texture<S>), dim3(tx * ty, slots), dim3(ST_NT), 0, ctx->stream, P, nx, ny,
                       pitch ? pitch : (size_t) nx * sizeof(S), tx, k, lo, ow, oh, first ? 1 : 0, fin ? 1 : 0,
                       ctx->precision == OFX_F64 ? 0 : 1, theta, r, alpha);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
static int op_structure_texture(ofx_ctx *ctx, int kind, int slots, const OfxTexSlots &P, int nx, int ny, size_t pitch, int k, bool first,
                                bool fin, double theta, double r, double alpha)
{
    switch (kind) {
    case OFX_SRC_F64: return st_launch<double>(ctx, slots, P, nx, ny, pitch, k, first, fin, theta, r, alpha);
    case OFX_SRC_F32: return st_launch<float>(ctx, slots, P, nx, ny, pitch, k, first, fin, theta, r, alpha);
    case OFX_SRC_U8:  return st_launch<unsigned char>(ctx, slots, P, nx, ny, pitch, k, first, fin, theta, r, alpha);
    case OFX_SRC_U16: return st_launch<unsigned short>(ctx, slots, P, nx, ny, pitch, k, first, fin, theta, r, alpha);
    default:          return st_launch<OfxRgb8>(ctx, slots, P, nx, ny, pitch, k, first, fin, theta, r, alpha);
    }
}

static bool st_misaligned(const void *p, size_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

extern "C" int ofx_structure_texture_dev(ofx_ctx *ctx, int n, const void *const *dSrc, void *const *dTex, void *const *dStruct, int nx,
                                         int ny, double theta, double alpha, int n_iter)
{
    OFX_ENTER(ctx);
    const char *who = "structure_texture";
    if (!dSrc || !dTex) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    if (n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n = %d (at least 1)", who, n);
    if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: frame %dx%d too small", who, nx, ny);
    if ((long long) nx * ny > (long long) INT_MAX - 2048) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %dx%d elements do not fit an int", who, nx, ny);
    if (!std::isfinite(theta) || !(theta > 0.0)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: theta = %g (finite, above 0)", who, theta);
    if (!(alpha >= 0.0 && alpha <= 1.0)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: alpha = %g is outside [0, 1]", who, alpha);
    if (n_iter < 0 || n_iter > OFX_ST_MAX_ITERS)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_iter = %d (0..%d)", who, n_iter, OFX_ST_MAX_ITERS);
    OFX_TRY(ofx_pitch_check(ctx, who, nx));
    const int kind = ofx_src_kind(ctx);
    const size_t al = ofx_src_align(kind), el = ctx->precision == OFX_F64 ? sizeof(double) : sizeof(float);
    for (int g = 0; g < n; g++) {
        if (!dSrc[g] || !dTex[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        void *st = dStruct ? dStruct[g] : nullptr;
        if (st_misaligned(dSrc[g], al)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: the frame of slot %d is not aligned to its element's %d bytes", who, g, (int) al);
        if (st_misaligned(dTex[g], el) || st_misaligned(st, el))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination of slot %d is not aligned to its element's %d bytes", who, g, (int) el);
        if (dTex[g] == dSrc[g] || st == dSrc[g] || st == dTex[g])
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination of slot %d is the frame that the slot reads, or its other destination", who, g);
    }
    const size_t pitch = ofx_src_pitch(ctx, nx), px = (size_t) nx * ny;
    const size_t span = ofx_frame_span(nx, ny, pitch, ofx_src_bytes(kind)), dense = px * el;
    const int K = ctx->st_fuse ? ctx->st_fuse : ST_DEFAULT_FUSE;
    const int launches = n_iter ? ofx_cdiv(n_iter, K) : 1;
    const double r = 0.25 / theta;
    const int per = n < OFX_MAX_GROUP ? n : OFX_MAX_GROUP;
    // the duals of one launch batch, in double, two copies: a tile reads its halo from what the launch before wrote
    double2 *pp[2] = {nullptr, nullptr};
    if (launches > 1) {
        OFX_TRY(ofx_alloc(ctx, (size_t) per * px, &pp[0]));
        OFX_TRY(ofx_alloc(ctx, (size_t) per * px, &pp[1]));
    }
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxTexSlots P = {};
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *src, *tex, *str;
            OFX_TRY(ofx_stage_in(ctx, dSrc[g], span, true, &src));
            OFX_TRY(ofx_stage_in(ctx, dTex[g], dense, false, &tex));
            OFX_TRY(ofx_stage_in(ctx, dStruct ? dStruct[g] : nullptr, dense, false, &str));
            P.src[z] = src;
            P.tex[z] = tex;
            P.str[z] = str;
        }
        for (int l = 0, done = 0; l < launches; l++) {
            const int k = n_iter - done < K ? n_iter - done : K;
            for (int z = 0; z < cnt; z++) {
                P.pin[z] = pp[l & 1] ? pp[l & 1] + (size_t) z * px : nullptr;
                P.pout[z] = pp[(l + 1) & 1] ? pp[(l + 1) & 1] + (size_t) z * px : nullptr;
            }
            OFX_TRY(op_structure_texture(ctx, kind, cnt, P, nx, ny, pitch, k, l == 0, l == launches - 1, theta, r, alpha));
            done += k;
        }
        for (int z = 0; z < cnt; z++) {
            OFX_TRY(ofx_stage_out(ctx, dTex[g0 + z], P.tex[z], dense));
            if (P.str[z]) OFX_TRY(ofx_stage_out(ctx, dStruct[g0 + z], P.str[z], dense));
        }
    }
    return OFX_OK;
}
