// ofx_apply.hip -- a .flo payload applied to device-resident frames: the backward warp with an occlusion map and a fill frame
// (ofx_flow_warp_dev) and the in-between frame of a bidirectional solve (ofx_flow_interpolate_dev; the flow approximation of
// Jiang et al., "Super SloMo", CVPR 2018, eq. 4).
//
// A frame is ny rows of nx pixels of NZ interleaved channels of the element type E (double | float | 8-bit | 16-bit: the context's
// "input" kind), read under "input_pitch"; the result is a dense frame of the same kind.  All arithmetic in double, every operation
// rounded (the build's -ffp-contract=off), association as written in include/ofx.h:
//     inside(x, y)       = 0 <= x <= nx - 1 and 0 <= y <= ny - 1                     (NaN and Inf fail it, before any int cast)
//     sample(I, x, y, k) = bicubic_interpolation_at_color(I, x, y, nx, ny, nz, k, false): bicubic_taps and cubic_cell, the taps and
//                          fractions computed once per pixel and shared by the channels
// Pure functions of the frames' values and the float payloads: the same bytes in every storage precision.
#include "ofx_device.h"
#include "ofx_ops.h"
#include "ofx_pairs.h"

#include <climits>
#include <cmath>

// ---- the shape of a workgroup ----------------------------------------------------------------------------------------------------
// 32 x 8 pixels, a wave = two rows of 32: the centre vectors are one float2 per lane, 256 contiguous bytes per row.  The block
// reduces the bounding box of its taps (a kept sample has x >= 0 and y >= 0, so its taps are the clamped columns x - 1 .. x + 2
// and rows y - 1 .. y + 2), stages the box with coalesced row loads into LDS in the frame's OWN element type -- 48 x 16 pixels: a
// block of flows of a few pixels needs 35 x 11; RGB bytes take 2.3 KB -- and gathers from there.  A block whose box does not fit
// (a motion boundary, a wild vector) gathers from global memory: the same loads' values into the same expressions, equal bits.
#define AP_BX 32
#define AP_BY 8
#define AP_NT (AP_BX * AP_BY)
#define AP_NW (AP_NT / 64)
#define AP_TW 48
#define AP_TH 16

struct OfxWarpSlots {
    const void          *src[OFX_MAX_GROUP];
    const float2        *flo[OFX_MAX_GROUP];
    const unsigned char *occ[OFX_MAX_GROUP];     // NULL: no map for the slot
    const void          *fill[OFX_MAX_GROUP];    // NULL: zeros
    void                *dst[OFX_MAX_GROUP];
};
struct OfxInterpSlots {
    const void   *a[OFX_MAX_GROUP], *b[OFX_MAX_GROUP];
    const float2 *fwd[OFX_MAX_GROUP], *bwd[OFX_MAX_GROUP];
    void         *dst[OFX_MAX_GROUP];
    double        t[OFX_MAX_GROUP];
};

// ---- conv: a double into the frame's element ---------------------------------------------------------------------------------------
template <typename E> OFX_DEV E ap_conv(double x);
template <> OFX_DEV double ap_conv<double>(double x) { return x; }
template <> OFX_DEV float ap_conv<float>(double x) { return (float) x; }
template <> OFX_DEV unsigned char ap_conv<unsigned char>(double x)              // NaN -> 0
{
    return !(x > 0.0) ? (unsigned char) 0 : (x >= 255.0 ? (unsigned char) 255 : (unsigned char) (int) (x + 0.5));
}
template <> OFX_DEV unsigned short ap_conv<unsigned short>(double x)
{
    return !(x > 0.0) ? (unsigned short) 0 : (x >= 65535.0 ? (unsigned short) 65535 : (unsigned short) (int) (x + 0.5));
}

OFX_DEV bool ap_inside(double x, double y, int nx, int ny)
{
    return x >= 0.0 && x <= (double) (nx - 1) && y >= 0.0 && y <= (double) (ny - 1);
}

// The NZ channels at one position.  base: element (x0, y0, channel 0) of the frame -- the frame itself with x0 = y0 = 0, or the LDS
// tile whose first pixel is (x0, y0) --, stride: elements from one row to the next.  O: the offsets' type (unsigned in LDS).
template <typename E, int NZ, typename O>
OFX_DEV void ap_sample(const E *base, O stride, int x0, int y0, const BicubicTaps &t, double *o)
{
    O r[4], c[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        r[q] = (O) (t.row[q] - y0) * stride;
        c[q] = (O) (t.col[q] - x0) * (O) NZ;
    }
#pragma unroll
    for (int k = 0; k < NZ; k++) {
        double cc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double v0 = ldw(base + r[0] + c[q] + k);
            const double v1 = ldw(base + r[1] + c[q] + k);
            const double v2 = ldw(base + r[2] + c[q] + k);
            const double v3 = ldw(base + r[3] + c[q] + k);
            cc[q] = cubic_cell(v0, v1, v2, v3, t.fy);
        }
        o[k] = cubic_cell(cc[0], cc[1], cc[2], cc[3], t.fx);
    }
}

// A position's taps into a box: lo .. hi of the clamped columns and rows (bicubic_taps orders them only up to the clamping)
struct ApBox { int xlo, xhi, ylo, yhi; };
OFX_DEV ApBox ap_box_of(bool need, const BicubicTaps &t)
{
    ApBox b = {0x7fffffff, -1, 0x7fffffff, -1};
    if (need) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            b.xlo = min(b.xlo, t.col[q]); b.xhi = max(b.xhi, t.col[q]);
            b.ylo = min(b.ylo, t.row[q]); b.yhi = max(b.yhi, t.row[q]);
        }
    }
    return b;
}
// ... reduced over the workgroup (every thread calls it; one barrier).  s_box: AP_NW x 4 ints of LDS of this call's own.
OFX_DEV ApBox ap_box_reduce(ApBox b, int (*s_box)[4], int tid)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        b.xlo = min(b.xlo, __shfl_xor(b.xlo, m, 64)); b.xhi = max(b.xhi, __shfl_xor(b.xhi, m, 64));
        b.ylo = min(b.ylo, __shfl_xor(b.ylo, m, 64)); b.yhi = max(b.yhi, __shfl_xor(b.yhi, m, 64));
    }
    if ((tid & 63) == 0) { s_box[tid >> 6][0] = b.xlo; s_box[tid >> 6][1] = b.xhi; s_box[tid >> 6][2] = b.ylo; s_box[tid >> 6][3] = b.yhi; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < AP_NW; w++) {
        b.xlo = min(b.xlo, s_box[w][0]); b.xhi = max(b.xhi, s_box[w][1]);
        b.ylo = min(b.ylo, s_box[w][2]); b.yhi = max(b.yhi, s_box[w][3]);
    }
    return b;
}
// does the box hold a tap at all, and does it fit the tile?  (the same answer in every thread of the block)
OFX_DEV bool ap_box_fits(const ApBox &b) { return b.xhi >= 0 && b.xhi - b.xlo < AP_TW && b.yhi - b.ylo < AP_TH; }

// the box's rows into the tile: consecutive threads take consecutive elements of a row, in the frame's element type
template <typename E, int NZ>
OFX_DEV void ap_stage(E *tile, const E *__restrict__ src, size_t stride, const ApBox &b, int tid)
{
    const unsigned we = (unsigned) (b.xhi - b.xlo + 1) * NZ, cnt = we * (unsigned) (b.yhi - b.ylo + 1);
    const E *__restrict__ org = src + (size_t) b.ylo * stride + (size_t) b.xlo * NZ;
    // k / we without a division per element: ceil(2^32 / we) as a fixed-point reciprocal is exact while k * we < 2^32 (here
    // k < 48 * 16 * 4, we <= 48 * 4), and the box of a frame of two or more columns is two or more elements wide
    const unsigned inv = 0xFFFFFFFFu / we + 1u;
    for (unsigned k = tid; k < cnt; k += AP_NT) {
        const unsigned r = we > 1u ? __umulhi(k, inv) : k, c = k - r * we;
        tile[r * (AP_TW * NZ) + c] = org[(size_t) r * stride + c];
    }
}

// ---- the store -----------------------------------------------------------------------------------------------------------------------
// Elements of four or eight bytes go out from their own threads.  Bytes and 16-bit elements go through LDS, as the map of
// k_flow_consistency does: block row r is a run of (columns in the image) * NZ elements of the destination's row; its elements are
// laid into LDS at the run's address mod 4, so that an LDS word IS an aligned 32-bit word of the destination.  A word wholly inside
// the run is one store; the words across its two ends go out element by element.  Nothing outside the run is written.
template <typename E, int NZ> struct ApOut {
    static constexpr bool packed = sizeof(E) < 4;
    static constexpr int  roww = packed ? (int) (AP_BX * NZ * sizeof(E)) / 4 + 1 : 1;      // words of LDS per block row
    static constexpr int  words = packed ? AP_BY * roww : 1;
};
template <typename E, int NZ>
OFX_DEV void ap_store(E *__restrict__ dst, int nx, int ny, int i0, int j0, int tid, bool in, const E *o, unsigned *s_out)
{
    const int tx = tid & (AP_BX - 1), ty = tid / AP_BX;
    if constexpr (!ApOut<E, NZ>::packed) {
        if (in) {
            E *p = dst + ((size_t) (i0 + ty) * nx + (j0 + tx)) * NZ;
#pragma unroll
            for (int k = 0; k < NZ; k++) p[k] = o[k];
        }
    } else {
        constexpr int RW = ApOut<E, NZ>::roww, PER = 4 / (int) sizeof(E);
        const int cols = min(AP_BX, nx - j0);
        const int run = cols * NZ * (int) sizeof(E);                             // bytes of a block row's run
        char *d = reinterpret_cast<char *>(dst);
        if (in) {
            const size_t lo = ((size_t) (i0 + ty) * nx + j0) * NZ * sizeof(E);
            const int a = (int) (reinterpret_cast<uintptr_t>(d + lo) & 3u);
            E *row = reinterpret_cast<E *>(reinterpret_cast<char *>(s_out + ty * RW) + a);
#pragma unroll
            for (int k = 0; k < NZ; k++) row[tx * NZ + k] = o[k];
        }
        __syncthreads();
        for (int w = tid; w < AP_BY * RW; w += AP_NT) {
            const int r = w / RW, ww = w - r * RW;
            if (i0 + r >= ny) continue;
            const size_t lo = ((size_t) (i0 + r) * nx + j0) * NZ * sizeof(E);
            const int a = (int) (reinterpret_cast<uintptr_t>(d + lo) & 3u);
            const int b0 = 4 * ww - a;                                           // the word's first byte within the run
            if (b0 >= run || b0 + 4 <= 0) continue;
            if (b0 >= 0 && b0 + 4 <= run) {
                *reinterpret_cast<unsigned *>(d + lo + b0) = s_out[w];
            } else {
                const E *e = reinterpret_cast<const E *>(s_out + w);
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int b = b0 + k * (int) sizeof(E);
                    if (b >= 0 && b < run) *reinterpret_cast<E *>(d + lo + b) = e[k];
                }
            }
        }
    }
}

// ---- the backward warp ---------------------------------------------------------------------------------------------------------------
//     (u, v) = flo[i][j];  x = j + u;  y = i + v
//     keep = inside(x, y) && (no map || occ[i nx + j] == 0)
//     keep: dst[i][j][k] = conv(sample(Src, x, y, k));  otherwise Fill[i][j][k] unchanged, or 0 without a fill frame
// Slot z = blockIdx.y, tile blockIdx.x.  stride: elements between the rows of Src and Fill.
template <typename E, int NZ>
__global__ __launch_bounds__(AP_NT) void k_flow_warp(OfxWarpSlots S, int nx, int ny, int tiles_x, size_t stride, int lds)
{
    __shared__ E s_tile[AP_TH * AP_TW * NZ];
    __shared__ int s_box[AP_NW][4];
    __shared__ unsigned s_out[ApOut<E, NZ>::words];
    const int z = blockIdx.y, tid = threadIdx.x;
    const int tby = (int) blockIdx.x / tiles_x, tbx = (int) blockIdx.x - tby * tiles_x;
    const int i0 = tby * AP_BY, j0 = tbx * AP_BX;
    const int i = i0 + tid / AP_BX, j = j0 + (tid & (AP_BX - 1));
    const bool in = j < nx && i < ny;
    const E *__restrict__ src = static_cast<const E *>(S.src[z]);
    const E *__restrict__ fill = static_cast<const E *>(S.fill[z]);
    const unsigned char *__restrict__ occ = S.occ[z];
    BicubicTaps t = {};
    bool keep = false;
    if (in) {
        const size_t p = (size_t) i * nx + j;
        const double2 c = ldw2(S.flo[z] + p);
        const double x = (double) j + c.x, y = (double) i + c.y;
        keep = ap_inside(x, y, nx, ny) && (!occ || occ[p] == 0);
        if (keep) t = bicubic_taps(x, y, nx, ny);
    }
    const ApBox box = ap_box_reduce(ap_box_of(keep, t), s_box, tid);
    const bool tile = lds && ap_box_fits(box);
    if (tile) {
        ap_stage<E, NZ>(s_tile, src, stride, box, tid);
        __syncthreads();
    }
    E o[NZ];
#pragma unroll
    for (int k = 0; k < NZ; k++) o[k] = (E) 0;
    if (keep) {
        double v[NZ];
        if (tile) ap_sample<E, NZ, unsigned>(s_tile, (unsigned) (AP_TW * NZ), box.xlo, box.ylo, t, v);
        else      ap_sample<E, NZ, size_t>(src, stride, 0, 0, t, v);
#pragma unroll
        for (int k = 0; k < NZ; k++) o[k] = ap_conv<E>(v[k]);
    } else if (in && fill) {
        const E *f = fill + (size_t) i * stride + (size_t) j * NZ;
#pragma unroll
        for (int k = 0; k < NZ; k++) o[k] = f[k];
    }
    ap_store<E, NZ>(static_cast<E *>(S.dst[z]), nx, ny, i0, j0, tid, in, o, s_out);
}

// ---- the in-between frame --------------------------------------------------------------------------------------------------------------
//     s = 1 - t;  c0 = s t;  c1 = t t;  c2 = s s
//     (u01, v01) = fwd[i][j];  (u10, v10) = bwd[i][j]
//     xa = j + (c1 u10 - c0 u01);  ya = i + (c1 v10 - c0 v01)              where this pixel is in A
//     xb = j + (c2 u01 - c0 u10);  yb = i + (c2 v01 - c0 v10)              ... and in B
//     both inside: s sample(A) + t sample(B);  one inside: that sample;  neither: s A[i][j][k] + t B[i][j][k]
// One box and one tile per source frame; each takes the LDS or the global path on its own.
template <typename E, int NZ>
__global__ __launch_bounds__(AP_NT) void k_flow_interpolate(OfxInterpSlots S, int nx, int ny, int tiles_x, size_t stride, int lds)
{
    __shared__ E s_ta[AP_TH * AP_TW * NZ];
    __shared__ E s_tb[AP_TH * AP_TW * NZ];
    __shared__ int s_boxa[AP_NW][4];
    __shared__ int s_boxb[AP_NW][4];
    __shared__ unsigned s_out[ApOut<E, NZ>::words];
    const int z = blockIdx.y, tid = threadIdx.x;
    const int tby = (int) blockIdx.x / tiles_x, tbx = (int) blockIdx.x - tby * tiles_x;
    const int i0 = tby * AP_BY, j0 = tbx * AP_BX;
    const int i = i0 + tid / AP_BX, j = j0 + (tid & (AP_BX - 1));
    const bool in = j < nx && i < ny;
    const E *__restrict__ A = static_cast<const E *>(S.a[z]);
    const E *__restrict__ B = static_cast<const E *>(S.b[z]);
    const double tt = S.t[z], s = 1.0 - tt;
    BicubicTaps ta = {}, tb = {};
    bool ina = false, inb = false;
    if (in) {
        const double c0 = s * tt, c1 = tt * tt, c2 = s * s;
        const size_t p = (size_t) i * nx + j;
        const double2 f = ldw2(S.fwd[z] + p), b = ldw2(S.bwd[z] + p);
        const double xa = (double) j + (c1 * b.x - c0 * f.x), ya = (double) i + (c1 * b.y - c0 * f.y);
        const double xb = (double) j + (c2 * f.x - c0 * b.x), yb = (double) i + (c2 * f.y - c0 * b.y);
        ina = ap_inside(xa, ya, nx, ny);
        inb = ap_inside(xb, yb, nx, ny);
        if (ina) ta = bicubic_taps(xa, ya, nx, ny);
        if (inb) tb = bicubic_taps(xb, yb, nx, ny);
    }
    const ApBox boxa = ap_box_reduce(ap_box_of(ina, ta), s_boxa, tid);
    const ApBox boxb = ap_box_reduce(ap_box_of(inb, tb), s_boxb, tid);
    const bool tilea = lds && ap_box_fits(boxa), tileb = lds && ap_box_fits(boxb);
    if (tilea) ap_stage<E, NZ>(s_ta, A, stride, boxa, tid);
    if (tileb) ap_stage<E, NZ>(s_tb, B, stride, boxb, tid);
    if (tilea || tileb) __syncthreads();
    E o[NZ];
#pragma unroll
    for (int k = 0; k < NZ; k++) o[k] = (E) 0;
    if (in) {
        double va[NZ], vb[NZ];
        if (ina) {
            if (tilea) ap_sample<E, NZ, unsigned>(s_ta, (unsigned) (AP_TW * NZ), boxa.xlo, boxa.ylo, ta, va);
            else       ap_sample<E, NZ, size_t>(A, stride, 0, 0, ta, va);
        }
        if (inb) {
            if (tileb) ap_sample<E, NZ, unsigned>(s_tb, (unsigned) (AP_TW * NZ), boxb.xlo, boxb.ylo, tb, vb);
            else       ap_sample<E, NZ, size_t>(B, stride, 0, 0, tb, vb);
        }
        if (!ina && !inb) {
            const size_t q = (size_t) i * stride + (size_t) j * NZ;
#pragma unroll
            for (int k = 0; k < NZ; k++) { va[k] = ldw(A + q + k); vb[k] = ldw(B + q + k); }
        }
#pragma unroll
        for (int k = 0; k < NZ; k++) o[k] = ap_conv<E>(ina == inb ? s * va[k] + tt * vb[k] : (ina ? va[k] : vb[k]));
    }
    ap_store<E, NZ>(static_cast<E *>(S.dst[z]), nx, ny, i0, j0, tid, in, o, s_out);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// One launch for slots <= OFX_MAX_GROUP slots; the pointers are memory of the context's GPU.  pitch: bytes between the rows of the
// frames that are read, 0 = dense.
// Option "apply_lds": 1 / 0 = the LDS tiles / the global gathers for every kind; 2 (default) = what measured faster at 1920 x 1080
// (DESIGN 8.17): the tiles for double frames (warp 175 against 216 us, in-between 314 against 349), the global gathers for byte
// frames (368 against 618 us, 647 against 1165).  Float and 16-bit frames were not measured and go with their neighbour in size.
template <typename E> static int ap_use_lds(const ofx_ctx *ctx) { return ctx->apply_lds == 2 ? (sizeof(E) >= 4 ? 1 : 0) : ctx->apply_lds; }

template <typename E, int NZ>
static int ap_launch_warp(ofx_ctx *ctx, int slots, const OfxWarpSlots &S, int nx, int ny, size_t pitch)
{
    const int tx = ofx_cdiv(nx, AP_BX), ty = ofx_cdiv(ny, AP_BY);
    const size_t stride = pitch ? pitch / sizeof(E) : (size_t) nx * NZ;
    hipLaunchKernelGGL((k_flow_warp<E, NZ>), dim3(tx * ty, slots), dim3(AP_NT), 0, ctx->stream, S, nx, ny, tx, stride, ap_use_lds<E>(ctx));
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename E, int NZ>
static int ap_launch_interp(ofx_ctx *ctx, int slots, const OfxInterpSlots &S, int nx, int ny, size_t pitch)
{
    const int tx = ofx_cdiv(nx, AP_BX), ty = ofx_cdiv(ny, AP_BY);
    const size_t stride = pitch ? pitch / sizeof(E) : (size_t) nx * NZ;
    hipLaunchKernelGGL((k_flow_interpolate<E, NZ>), dim3(tx * ty, slots), dim3(AP_NT), 0, ctx->stream, S, nx, ny, tx, stride,
                       ap_use_lds<E>(ctx));
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
// the element kind and the channel count, chosen at run time, into the kernels' template arguments
#define AP_BY_NZ(fn, E, ...)                                        \
    switch (nz) {                                                   \
    case 1:  return fn<E, 1>(__VA_ARGS__);                          \
    case 2:  return fn<E, 2>(__VA_ARGS__);                          \
    case 3:  return fn<E, 3>(__VA_ARGS__);                          \
    default: return fn<E, 4>(__VA_ARGS__);                          \
    }
#define AP_BY_KIND(fn, ...)                                         \
    switch (kind) {                                                 \
    case OFX_SRC_F64: AP_BY_NZ(fn, double, __VA_ARGS__)             \
    case OFX_SRC_F32: AP_BY_NZ(fn, float, __VA_ARGS__)              \
    case OFX_SRC_U8:  AP_BY_NZ(fn, unsigned char, __VA_ARGS__)      \
    default:          AP_BY_NZ(fn, unsigned short, __VA_ARGS__)     \
    }
static int op_flow_warp(ofx_ctx *ctx, int kind, int nz, int slots, const OfxWarpSlots &S, int nx, int ny, size_t pitch)
{
    AP_BY_KIND(ap_launch_warp, ctx, slots, S, nx, ny, pitch)
}
static int op_flow_interpolate(ofx_ctx *ctx, int kind, int nz, int slots, const OfxInterpSlots &S, int nx, int ny, size_t pitch)
{
    AP_BY_KIND(ap_launch_interp, ctx, slots, S, nx, ny, pitch)
}

// what both entries refuse about sizes and the frames' format, before any work
static int ap_check_format(ofx_ctx *ctx, const char *who, int n, int nx, int ny, int nz)
{
    if (n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n = %d (at least 1)", who, n);
    if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: frame %dx%d too small", who, nx, ny);
    if (nz < 1 || nz > 4) return ofx_fail(ctx, OFX_ERR_ARG, "%s: nz = %d (1..4 interleaved channels)", who, nz);
    if ((long long) nx * ny * nz > (long long) INT_MAX - 2048)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: %dx%dx%d elements do not fit an int", who, nx, ny, nz);
    if (ofx_src_kind(ctx) == OFX_SRC_RGB8)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: OFX_IN_RGB8 collapses a pixel to gray; an HWC byte image is OFX_IN_U8 with nz = 3", who);
    return ofx_pitch_check(ctx, who, nx * nz);
}
static bool ap_misaligned(const void *p, size_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

extern "C" int ofx_flow_warp_dev(ofx_ctx *ctx, int n, const void *const *dSrc, const void *const *d_flo, const void *const *d_occ,
                                 const void *const *dFill, void *const *dDst, int nx, int ny, int nz)
{
    OFX_ENTER(ctx);
    const char *who = "flow_warp";
    if (!dSrc || !d_flo || !dDst) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    OFX_TRY(ap_check_format(ctx, who, n, nx, ny, nz));
    const int kind = ofx_src_kind(ctx);
    const size_t al = ofx_src_align(kind);
    for (int g = 0; g < n; g++) {
        if (!dSrc[g] || !d_flo[g] || !dDst[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        if (ap_misaligned(d_flo[g], sizeof(float2))) return ofx_fail(ctx, OFX_ERR_ARG, "%s: payload of slot %d is not 8-byte aligned", who, g);
        const void *fill = dFill ? dFill[g] : nullptr;
        if (ap_misaligned(dSrc[g], al) || ap_misaligned(dDst[g], al) || ap_misaligned(fill, al))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a frame of slot %d is not aligned to its element's %d bytes", who, g, (int) al);
        if (dDst[g] == dSrc[g] || dDst[g] == fill)
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the destination of slot %d is a frame that the slot reads", who, g);
    }
    const size_t pitch = ofx_src_pitch(ctx, nx * nz), px = (size_t) nx * ny;
    const size_t span = ofx_frame_span(nx * nz, ny, pitch, ofx_src_bytes(kind)), dense = px * nz * ofx_src_bytes(kind);
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxWarpSlots S = {};
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *src, *flo, *occ, *fill, *dst;
            OFX_TRY(ofx_stage_in(ctx, dSrc[g], span, true, &src));
            OFX_TRY(ofx_stage_in(ctx, d_flo[g], px * sizeof(float2), true, &flo));
            OFX_TRY(ofx_stage_in(ctx, d_occ ? d_occ[g] : nullptr, px, true, &occ));
            OFX_TRY(ofx_stage_in(ctx, dFill ? dFill[g] : nullptr, span, true, &fill));
            OFX_TRY(ofx_stage_in(ctx, dDst[g], dense, false, &dst));
            S.src[z] = src;
            S.flo[z] = static_cast<const float2 *>(flo);
            S.occ[z] = static_cast<const unsigned char *>(occ);
            S.fill[z] = fill;
            S.dst[z] = dst;
        }
        OFX_TRY(op_flow_warp(ctx, kind, nz, cnt, S, nx, ny, pitch));
        for (int z = 0; z < cnt; z++) OFX_TRY(ofx_stage_out(ctx, dDst[g0 + z], S.dst[z], dense));
    }
    return OFX_OK;
}

extern "C" int ofx_flow_interpolate_dev(ofx_ctx *ctx, int n, const void *const *dA, const void *const *dB, const void *const *d_flo_fwd,
                                        const void *const *d_flo_bwd, const double *t, void *const *dDst, int nx, int ny, int nz)
{
    OFX_ENTER(ctx);
    const char *who = "flow_interpolate";
    if (!dA || !dB || !d_flo_fwd || !d_flo_bwd || !t || !dDst) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    OFX_TRY(ap_check_format(ctx, who, n, nx, ny, nz));
    const int kind = ofx_src_kind(ctx);
    const size_t al = ofx_src_align(kind);
    for (int g = 0; g < n; g++) {
        if (!dA[g] || !dB[g] || !d_flo_fwd[g] || !d_flo_bwd[g] || !dDst[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        if (!(t[g] >= 0.0 && t[g] <= 1.0)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: t = %g of slot %d is outside [0, 1]", who, t[g], g);
        if (ap_misaligned(d_flo_fwd[g], sizeof(float2)) || ap_misaligned(d_flo_bwd[g], sizeof(float2)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a payload of slot %d is not 8-byte aligned", who, g);
        if (ap_misaligned(dA[g], al) || ap_misaligned(dB[g], al) || ap_misaligned(dDst[g], al))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a frame of slot %d is not aligned to its element's %d bytes", who, g, (int) al);
        if (dDst[g] == dA[g] || dDst[g] == dB[g])
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the destination of slot %d is a frame that the slot reads", who, g);
    }
    const size_t pitch = ofx_src_pitch(ctx, nx * nz), px = (size_t) nx * ny;
    const size_t span = ofx_frame_span(nx * nz, ny, pitch, ofx_src_bytes(kind)), dense = px * nz * ofx_src_bytes(kind);
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxInterpSlots S = {};
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *a, *b, *fwd, *bwd, *dst;
            OFX_TRY(ofx_stage_in(ctx, dA[g], span, true, &a));
            OFX_TRY(ofx_stage_in(ctx, dB[g], span, true, &b));
            OFX_TRY(ofx_stage_in(ctx, d_flo_fwd[g], px * sizeof(float2), true, &fwd));
            OFX_TRY(ofx_stage_in(ctx, d_flo_bwd[g], px * sizeof(float2), true, &bwd));
            OFX_TRY(ofx_stage_in(ctx, dDst[g], dense, false, &dst));
            S.a[z] = a;
            S.b[z] = b;
            S.fwd[z] = static_cast<const float2 *>(fwd);
            S.bwd[z] = static_cast<const float2 *>(bwd);
            S.dst[z] = dst;
            S.t[z] = t[g];
        }
        OFX_TRY(op_flow_interpolate(ctx, kind, nz, cnt, S, nx, ny, pitch));
        for (int z = 0; z < cnt; z++) OFX_TRY(ofx_stage_out(ctx, dDst[g0 + z], S.dst[z], dense));
    }
    return OFX_OK;
}
