// ofx_ops.h -- launchers of the operator / pyramid kernels (device pointers, enqueue on ctx->stream,
// never synchronise).  T is the storage type (double | float); arithmetic is double.
#pragma once

#include "ofx_internal.h"

#include <vector>

#define OFX_GAUSS_MAX_TAPS 64

struct GaussTaps {
    int    size;                       // kernel radius + 1  == (int)(5 sigma) + 1
    int    dirichlet;                  // 1: samples outside the image are 0 (BOUNDARY_CONDITION_DIRICHLET); 0: reflecting (default)
    double B[OFX_GAUSS_MAX_TAPS];
};

// host-side tap computation (src/operators.cpp:515-539); returns OFX_ERR_ARG if > MAX taps
int ofx_gauss_taps(double sigma, GaussTaps *t);

template <typename T> int op_convert_in(ofx_ctx *ctx, const double *src, T *dst, size_t n);
template <typename T> int op_convert_out(ofx_ctx *ctx, const T *src, double *dst, size_t n);
template <typename T> int op_interleave2(ofx_ctx *ctx, const double *a, const double *b,
                                         typename Pix<T>::v2 *dst, size_t n);
template <typename T> int op_deinterleave2(ofx_ctx *ctx, const typename Pix<T>::v2 *src, double *a,
                                           double *b, size_t n);
template <typename T> int op_to_flo(ofx_ctx *ctx, const typename Pix<T>::v2 *src, float2 *dst, size_t n);
template <typename T> int op_fill2(ofx_ctx *ctx, typename Pix<T>::v2 *dst, size_t n);   // zero

// one host plane of n doubles into a new arena array of the storage type
template <typename T>
static int upload_plane(ofx_ctx *ctx, const double *h, size_t n, T **out)
{
    double *stage;
    OFX_TRY(ofx_alloc(ctx, n, &stage));
    OFX_TRY(ofx_alloc(ctx, n, out));
    OFX_HIP(ctx, hipMemcpyAsync(stage, h, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return op_convert_in<T>(ctx, stage, *out, n);
}

// a solve's record before its first level: zeros but for the two counts
static inline void ofx_stats_begin(ofx_stats *st, int nscales, int nsolves)
{
    memset(st, 0, sizeof(*st));
    st->nscales = nscales;
    st->nsolves = nsolves;
}

// ---- joint min / max and the normalisation map (getminmax, image_normalization_1 / _2 / _2_color / _3 / _4, src/utils.cpp) ----
// The sources of one launch reach the kernels through a by-value table of OFX_MM_MAX_SRC (== 2 * OFX_MAX_GROUP ==
// OFX_BROXT_MAX_FRAMES) pointers of type S (double, or the storage type; converted exactly to double).  `per` consecutive
// sources form a SET that shares {min, max}; with nz interleaved channels, channel c of a set has its own {min, max} over
// elements t * nz + c (t < npix) of the set's sources.  One set may come in several CHUNKS (launches): chunk k of `chunks`
// adds its partial results behind those of the chunks before, op_minmax_final reduces them all.  min / max are exact, so the
// reduction order is free.
#define OFX_MM_MAX_SRC 32
static_assert(OFX_MM_MAX_SRC >= 2 * OFX_MAX_GROUP && OFX_MM_MAX_SRC >= OFX_BROXT_MAX_FRAMES, "the table holds a group's pairs and a sequence's frames");
struct OfxSrcPtrs { const void *p[OFX_MM_MAX_SRC]; };
struct OfxDstPtrs { void *p[OFX_MM_MAX_SRC]; };
// doubles of scratch for `nsets` sets of sources of npix * nz elements; the layout is private to ofx_ops.hip
size_t op_minmax_scratch_doubles(int nsets, size_t npix, int nz, int chunks = 1);
template <typename S>
int op_minmax_partial(ofx_ctx *ctx, const OfxSrcPtrs &src, int nsets, int per, size_t npix, int nz, double *scr, int chunk = 0,
                      int chunks = 1);
int op_minmax_final(ofx_ctx *ctx, int nsets, size_t npix, int nz, double *scr, int chunks = 1);
// after op_minmax_final: {min, max} of channel c of set s on the device at op_minmax_result(scr)[2 * (s * nz + c)]
const double *op_minmax_result(const double *scr);
// dst[q][e] = 255 (src[q][e] - min) / (max - min) for the npix * nz elements e of every source q, {min, max} those of q's set and
// e's channel; guard != 0: a copy where max - min <= 0 (image_normalization_3 alone divides regardless, as the reference does)
template <typename T, typename S>
int op_normalize_map(ofx_ctx *ctx, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, size_t npix, int nz,
                     const double *scr, int guard = 1);
// the three steps for sets that come in one chunk; scr: op_minmax_scratch_doubles(nsets, npix, nz) doubles
template <typename T, typename S>
int op_normalize_sets(ofx_ctx *ctx, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, size_t npix, int nz, double *scr,
                      int guard = 1);

// ---- ... with the sources in a kind chosen at run time (OFX_SRC_*, ofx_internal.h: the context's option "input") ----
// OFX_SRC_F64 / _F32 are the launches above with S = double / float.  The byte kinds (U8, U16, RGB8 -- there an element is a pixel
// of three bytes and nz must be 1) run the kernels of ofx_ops.hip that load four elements per lane as aligned 32-bit words, or,
// with the context's input_vec = 0 and for the min / max of nz > 1 channels, the kernels above on S = unsigned char / unsigned
// short / OfxRgb8.  Same scratch, same results: every sample is exact in double.
// The frames are ny rows of nx * nz elements (OFX_SRC_RGB8: of nx pixels), `pitch` bytes from one row's start to the next's.
// pitch = 0: the rows lie back to back, and the launches are those of the flat element count nx * ny (a pitch equal to the row's
// bytes is passed as 0: ofx_src_pitch).  Otherwise the pitched kernels of ofx_ops.hip: the same values from the same
// expressions, no byte outside a row read; pitch is a multiple of the element's alignment and at least the row's bytes.
int op_minmax_partial_in(ofx_ctx *ctx, int kind, const OfxSrcPtrs &src, int nsets, int per, int nx, int ny, size_t pitch, int nz,
                         double *scr, int chunk = 0, int chunks = 1);
template <typename T>
int op_normalize_map_in(ofx_ctx *ctx, int kind, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, int nx, int ny,
                        size_t pitch, int nz, const double *scr, int guard = 1);
template <typename T>
int op_normalize_sets_in(ofx_ctx *ctx, int kind, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, int nx, int ny,
                         size_t pitch, int nz, double *scr, int guard = 1);
// rows of a pitched frame and the tiles a launch cuts them into (ofx_ops.hip; rows_tile in ofx_device.h), passed to kernels by value
struct OfxRows {
    int    w, ny;       // elements (OFX_SRC_RGB8: pixels) per row, rows
    size_t pitch;       // bytes from one row's start to the next's
    int    lbx;         // a tile is 1 << lbx slots of a row wide
    int    cx, tiles;   // tiles per row's length, tiles in all
};
// groups = false: a slot is one of the row's w elements; true: a group of four of them.  A thread takes its slot of 4 rows.
OfxRows op_rows_geom(int w, int ny, size_t pitch, bool groups);
// dst[q][i * nx + j] = element j of row i of src[q], for the `count` <= OFX_MM_MAX_SRC sources of a byte kind (no normalisation)
template <typename T>
int op_convert_sources_in(ofx_ctx *ctx, int kind, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int count, int nx, int ny, size_t pitch);

// generic bicubic resampling out(i1,j1) = bicubic(in, j1/fx, i1/fy, border_out=false)
// (zoom_out: fx=fy=factor, src/zoom.cpp:67-75; zoom_in: per-axis factors, src/zoom.cpp:142-154)
template <typename T> int op_resample(ofx_ctx *ctx, const T *in, T *out, int nx, int ny, int nxx, int nyy,
                                      double fx, double fy);
// zoom_in of an interleaved flow field + `*= scale` (src/tvl1flow.cpp:302-309)
// G > 1: the G flow fields of a lockstep group, back to back in U and Uout, in one launch
template <typename T> int op_zoom_in_flow(ofx_ctx *ctx, const typename Pix<T>::v2 *U, typename Pix<T>::v2 *Uout,
                                          int nx, int ny, int nxx, int nyy, double scale, int G = 1);
// planes one launch of op_gaussian_planes / op_zoom_out_channels_planes serves (blockIdx.z): the pairs of a lockstep group, or the
// distinct planes of a group of indexed triples (TV-L1 with occlusions: up to four per triple)
#define OFX_MAX_PLANES (4 * OFX_MAX_GROUP)
// zoom_out (src/zoom.cpp:41-78) of `count` images (at most OFX_MAX_PLANES) of nz interleaved channels, each channel as zoom_out
// (the IPOL original of robust_expo_methods, zoom.h:45-85), one launch per stage: images 0 .. split - 1 back to back at A (nx*ny*nz
// elements each), the others at B, the results likewise at oA / oB, tmpA / tmpB scratch for count images; OFX_ERR_SIGMA under
// zoom_out's rule, before anything is launched.  A single image is count = split = 1, a plane nz = 1.
template <typename T> int op_zoom_out_channels_planes(ofx_ctx *ctx, int count, int split, const T *A, const T *B, T *oA, T *oB,
                                                      T *tmpA, T *tmpB, int nx, int ny, int nz, double factor);
// ... for the 2 G images of a lockstep group of pairs: A / B = the G first / second images
template <typename T> int op_zoom_out_channels_group(ofx_ctx *ctx, int G, const T *A, const T *B, T *oA, T *oB, T *tmpA, T *tmpB,
                                                     int nx, int ny, int nz, double factor);
// gaussian (src/operators.cpp:506-624) in place on the first nx*ny elements of `count` images, one launch per pass: images
// 0 .. split - 1 start at A, the others at B, each `stride` elements after the one before; tmp holds count planes of nx*ny.  A
// single image is count = split = 1; at most OFX_MAX_PLANES
template <typename T> int op_gaussian_planes(ofx_ctx *ctx, int count, int split, T *A, T *B, size_t stride, T *tmp, int nx, int ny,
                                             double sigma, int dirichlet = 0);
// ... for the 2 G images of a lockstep group of pairs
template <typename T> int op_gaussian_group(ofx_ctx *ctx, int G, T *A, T *B, size_t stride, T *tmp, int nx, int ny, double sigma,
                                            int dirichlet = 0);
// zoom_in (op_resample with per-axis factors) of the G planes of u1, u2 and c in one launch, u1 and u2 then `*= scale`
// (src/tvl1occflow.cpp:466-475): planes back to back, nx*ny in, nxx*nyy out
template <typename T> int op_zoom_in_planes3(ofx_ctx *ctx, int G, const T *u1, const T *u2, const T *c, T *u1o, T *u2o, T *co, int nx,
                                             int ny, int nxx, int nyy, double scale);

// planar operators for the operator-level API
template <typename T> int op_divergence(ofx_ctx *ctx, const T *v1, const T *v2, T *div, int nx, int ny);
template <typename T> int op_forward_gradient(ofx_ctx *ctx, const T *f, T *fx, T *fy, int nx, int ny);
template <typename T> int op_centered_gradient(ofx_ctx *ctx, const T *f, T *dx, T *dy, int nx, int ny);
// ... of `count` planes (at most 65535) back to back (f, dx, dy alike) in one launch
template <typename T> int op_centered_gradient_planes(ofx_ctx *ctx, int count, const T *f, T *dx, T *dy, int nx, int ny);
template <typename T> int op_second_derivative(ofx_ctx *ctx, const T *f, T *out, int nx, int ny, int which);
template <typename T> int op_bicubic_warp(ofx_ctx *ctx, const T *in, const T *u, const T *v, T *out, int nx,
                                          int ny, int border_out);
template <typename T> int op_bicubic_at(ofx_ctx *ctx, const T *in, const double *uu, const double *vv,
                                        double *out, int n, int nx, int ny, int border_out);

// colour / sequence variants of the operator surface (bicubic_interpolation.h:30, operators.h:107, utils.h:119)
template <typename T> int op_bicubic_at_color(ofx_ctx *ctx, const T *in, const double *uu, const double *vv, double *out,
                                              int n, int nx, int ny, int nz, int ch, int border_out);
template <typename T> int op_gradient_dz(ofx_ctx *ctx, const T *in, T *dz, int nx, int ny, int nz);

// pa = (f, centred dx) pairs, pb = centred dy: one pair gather + one scalar gather per bicubic tap serve the
// three warps of (f, fx, fy) (see bicubic_sample3 in ofx_device.h for why not one padded 4-vector)
template <typename T> int op_grad_pack(ofx_ctx *ctx, const T *f, typename Pix<T>::v2 *pa, T *pb, int nx, int ny, int G = 1);

// Shared pyramid prologue (src/tvl1flow.cpp:236-280 == horn_schunck_pyramidal.cpp:279-323 ==
// brox_optic_flow_spatial.cpp:467-509): joint normalisation, presmoothing, zoom_out chain -- op_build_pyramid_group below, on
// levels that the caller lays out (op_pyramid_sizes) with op_pyramid_scratch_doubles() doubles of scratch per pair.
int op_pyramid_sizes(ofx_ctx *ctx, int nxx, int nyy, int nscales, double zfactor, std::vector<int> &nxs, std::vector<int> &nys);
size_t op_pyramid_scratch_doubles();

// device pointers of the caller's G image pairs, passed to kernels by value
struct OfxGroupPtrs {
    const void *a[OFX_MAX_GROUP];
    const void *b[OFX_MAX_GROUP];
};
// pyramids of the G pairs of a lockstep group, one launch per step for all 2 G images (see ofx_ops.hip)
template <typename T>
int op_build_pyramid_group(ofx_ctx *ctx, int G, const void *const *dA, const void *const *dB, int nscales, double zfactor,
                           double presmooth_sigma, const int *nxs, const int *nys, T *const *lvA, T *const *lvB, T *tmpA,
                           T *tmpB, double *scr, int kind = -1,        // kind: OFX_SRC_* of dA / dB; -1 = the storage type
                           size_t pitch = 0);                          // kind >= 0: bytes between the rows of dA / dB, 0 = dense

// ---- the pyramid of a start flow (TV-L1 warm start: ofx_tvl1_group_init_dev, include/ofx.h) ----
// init[g]: the .flo payload (nx * ny interleaved (u, v) float32, 8-byte aligned, memory of the context's GPU) pair g starts from,
// or NULL for a pair that starts from zero.  W_0 = the payload widened to double, a component that is not finite taken as 0;
// W_s = zoom_out(W_{s-1}, zfactor) * zfactor per component, in double storage and arithmetic whatever OUT is.  out[g] receives
// W_{nscales-1} of pair g -- nxs[nscales-1] * nys[nscales-1] interleaved pairs rounded once to OUT (double2 | float2) -- and zeros
// for a pair without a start, from the same launch.  One launch per level for all pairs (two where zfactor != 1/2); the scratch
// comes from the arena.  OFX_ERR_SIGMA under op_build_pyramid_group's rule (op_flow_pyramid_check), before anything is launched.
int op_flow_pyramid_check(ofx_ctx *ctx, int nscales, double zfactor, const int *nxs, const int *nys);
template <typename OUT>
int op_flow_pyramid(ofx_ctx *ctx, int G, const void *const *init, int nscales, double zfactor, const int *nxs, const int *nys,
                    void *const *out);
// bytes of arena scratch op_flow_pyramid takes per pair (the memory rule of ofx_tvl1_batch_group_size)
double op_flow_pyramid_scratch_bytes(int nscales, double zfactor, const int *nxs, const int *nys);

// ---- buffers that are not on the context's GPU (ofx_ops.hip; staged through the arena by ofx_pairs.h) ----
// is p device memory of this context's GPU?  Everything else is reached through a staging copy:
bool ofx_ptr_is_local(const ofx_ctx *ctx, const void *p);
// dst <- src, one of them on this context's GPU, the other anywhere (ofx_staging_route), on the context's stream
int ofx_copy_staged(ofx_ctx *ctx, void *dst, const void *src, size_t bytes);

// ---- forward-backward consistency of .flo payloads (ofx_flow.hip) ----
// slot z of a launch: payload f[z] checked against payload b[z] into the byte map occ[z] (any alignment)
struct OfxFlowSlots {
    const float2  *f[OFX_MAX_GROUP];
    const float2  *b[OFX_MAX_GROUP];
    unsigned char *occ[OFX_MAX_GROUP];
};
// sizes and thresholds every entry refuses before any work (OFX_ERR_ARG, `who` opens the message)
int op_flow_consistency_check(ofx_ctx *ctx, const char *who, int nx, int ny, double alpha, double beta);
// slots <= OFX_MAX_GROUP maps in one launch; the pointers are memory of the context's GPU, the payloads 8-byte aligned
int op_flow_consistency(ofx_ctx *ctx, int slots, const void *const *f, const void *const *b, void *const *occ, int nx, int ny,
                        double alpha, double beta);

// ---- the median of a flow (ofx_median.hip) -----------------------------------------------------------------------------------------
struct OfxMedianSlots {
    const void          *in[OFX_MAX_GROUP];      // nx * ny interleaved (u, v) pairs
    const unsigned char *occ[OFX_MAX_GROUP];     // NULL: no map for the slot
    void                *out[OFX_MAX_GROUP];     // never the slot's `in`
};
// The wsize x wsize median of include/ofx.h ("Median of a flow") of slots <= OFX_MAX_GROUP flows in one launch; esize = 4 | 8: the
// elements are floats (wsize 3, 5, 7) or doubles (3, 5).  The pointers are memory of the context's GPU, aligned to a pair.
int op_flow_median(ofx_ctx *ctx, int esize, int wsize, int slots, const OfxMedianSlots &S, int nx, int ny);
// ... and out[z] copied back over in[z], n pairs each, in one launch
int op_median_copy_back(ofx_ctx *ctx, int esize, int slots, const OfxMedianSlots &S, size_t n);

#define OFX_LAUNCH_CHECK(ctx)                                                                  \
    do {                                                                                         \
        hipError_t e__ = hipGetLastError();                                                      \
        if (e__ != hipSuccess)                                                                   \
            return ofx_fail((ctx), OFX_ERR_HIP, "kernel launch failed: %s (%s:%d)",              \
                            hipGetErrorString(e__), __FILE__, __LINE__);                         \
    } while (0)
