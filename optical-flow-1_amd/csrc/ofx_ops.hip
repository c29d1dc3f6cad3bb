// ofx_ops.hip -- gfx950 kernels + launchers for the shared operators and the pyramid
// (reference: src/operators.cpp, src/bicubic_interpolation.cpp, src/zoom.cpp, src/utils.cpp).
//
// All of these are HBM-bound elementwise / small-stencil / gather kernels: one pixel per lane,
// x fastest so every wave touches 64 consecutive pixels of a row (coalesced), 64x4 blocks so a
// block's four waves share their vertical neighbours through L1.  They run once per pyramid level
// or once per warp, never inside the inner iteration.
#include "ofx_ops.h"
#include "ofx_device.h"

#include <cmath>

#define BX 64
#define BY 4

static inline dim3 grid2d(int nx, int ny) { return dim3(ofx_cdiv(nx, BX), ofx_cdiv(ny, BY)); }
static inline dim3 block2d() { return dim3(BX, BY); }
static inline int grid1d(size_t n) { return (int) ((n + 255) / 256); }

// ---- layout conversions ---------------------------------------------------------------------------
template <typename T>
__global__ void k_convert_in(const double *__restrict__ src, T *__restrict__ dst, size_t n)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stn(dst + i, src[i]);
}

template <typename T>
__global__ void k_convert_out(const T *__restrict__ src, double *__restrict__ dst, size_t n)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = ldw(src + i);
}

template <typename T>
__global__ void k_interleave2(const double *__restrict__ a, const double *__restrict__ b,
                              typename Pix<T>::v2 *__restrict__ dst, size_t n)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stn2(dst + i, make_double2(a[i], b[i]));
}

template <typename T>
__global__ void k_deinterleave2(const typename Pix<T>::v2 *__restrict__ src, double *__restrict__ a,
                                double *__restrict__ b, size_t n)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const double2 v = ldw2(src + i);
        a[i] = v.x;
        b[i] = v.y;
    }
}

// (u,v) -> float32 pairs: the cast of src/tvl1flow_main.cpp:209-213
template <typename T>
__global__ void k_to_flo(const typename Pix<T>::v2 *__restrict__ src, float2 *__restrict__ dst, size_t n)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const double2 v = ldw2(src + i);
        dst[i] = make_float2((float) v.x, (float) v.y);
    }
}

template <typename T> int op_convert_in(ofx_ctx *ctx, const double *src, T *dst, size_t n)
{
    hipLaunchKernelGGL(k_convert_in<T>, dim3(grid1d(n)), dim3(256), 0, ctx->stream, src, dst, n);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T> int op_convert_out(ofx_ctx *ctx, const T *src, double *dst, size_t n)
{
    hipLaunchKernelGGL(k_convert_out<T>, dim3(grid1d(n)), dim3(256), 0, ctx->stream, src, dst, n);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T>
int op_interleave2(ofx_ctx *ctx, const double *a, const double *b, typename Pix<T>::v2 *dst, size_t n)
{
    hipLaunchKernelGGL(k_interleave2<T>, dim3(grid1d(n)), dim3(256), 0, ctx->stream, a, b, dst, n);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T>
int op_deinterleave2(ofx_ctx *ctx, const typename Pix<T>::v2 *src, double *a, double *b, size_t n)
{
    hipLaunchKernelGGL(k_deinterleave2<T>, dim3(grid1d(n)), dim3(256), 0, ctx->stream, src, a, b, n);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T> int op_to_flo(ofx_ctx *ctx, const typename Pix<T>::v2 *src, float2 *dst, size_t n)
{
    hipLaunchKernelGGL(k_to_flo<T>, dim3(grid1d(n)), dim3(256), 0, ctx->stream, src, dst, n);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T> int op_fill2(ofx_ctx *ctx, typename Pix<T>::v2 *dst, size_t n)
{
    OFX_HIP(ctx, hipMemsetAsync(dst, 0, n * sizeof(typename Pix<T>::v2), ctx->stream));
    return OFX_OK;
}

// ---- joint min / max of sets of images and the normalisation map (src/utils.cpp:283-501, getminmax :509-525) --------
// min / max are exact (order-independent): per-block partials, then one block per set and channel.  Scratch of nslots =
// nsets * nz {min, max} results whose partials come in `count` = chunks * blocks-per-chunk pieces each:
//   scr[2 * slot], scr[2 * slot + 1]            {min, max} of slot = set * nz + channel
//   scr[2 * nslots + slot * count + k]          partial minima of the slot
//   scr[2 * nslots + (nslots + slot) * count + k]   partial maxima
#define MM_BLOCKS 1024
static inline int mm_blocks(size_t npix) { return npix > (size_t) MM_BLOCKS * 256 ? MM_BLOCKS : (int) ((npix + 255) / 256); }

OFX_DEV void minmax_block_reduce(double lo, double hi, double *__restrict__ plo, double *__restrict__ phi)
{
    lo = wave_allreduce_min(lo);
    hi = wave_allreduce_max(hi);
    __shared__ double slo[4], shi[4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { slo[w] = lo; shi[w] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) { lo = slo[k] < lo ? slo[k] : lo; hi = shi[k] > hi ? shi[k] : hi; }
        *plo = lo;
        *phi = hi;
    }
}
// block (c * nb + b, set): a stride of channel c of all `per` sources of the set, two sources at a time (their pointers fetched
// once, two loads in flight per lane; an odd last source is read twice); first = this chunk's place among the pieces
template <typename S>
__global__ __launch_bounds__(256) void k_minmax_partial(OfxSrcPtrs src, int per, size_t npix, int nz, int nb, int first, int count,
                                                        double *__restrict__ scr)
{
    const int c = blockIdx.x / nb, b = blockIdx.x - c * nb, set = blockIdx.y;
    const int nslots = gridDim.y * nz, slot = set * nz + c;
    double lo = ldw((const S *) src.p[set * per] + c), hi = lo;
    for (int k = 0; k < per; k += 2) {
        const S *__restrict__ I1 = (const S *) src.p[set * per + k] + c;
        const S *__restrict__ I2 = (const S *) src.p[set * per + (k + 1 < per ? k + 1 : k)] + c;
        for (size_t t = (size_t) b * 256 + threadIdx.x; t < npix; t += (size_t) nb * 256) {
            const double x = ldw(I1 + t * nz), y = ldw(I2 + t * nz);
            lo = x < lo ? x : lo; hi = x > hi ? x : hi;
            lo = y < lo ? y : lo; hi = y > hi ? y : hi;
        }
    }
    double *part = scr + 2 * (size_t) nslots + (size_t) slot * count + first + b;
    minmax_block_reduce(lo, hi, part, part + (size_t) nslots * count);
}
// block = slot
__global__ __launch_bounds__(256) void k_minmax_final(double *__restrict__ scr, int count)
{
    const int nslots = gridDim.x, slot = blockIdx.x;
    const double *plo = scr + 2 * (size_t) nslots + (size_t) slot * count, *phi = plo + (size_t) nslots * count;
    double lo = plo[0], hi = phi[0];
    for (int i = threadIdx.x; i < count; i += 256) {
        lo = plo[i] < lo ? plo[i] : lo;
        hi = phi[i] > hi ? phi[i] : hi;
    }
    minmax_block_reduce(lo, hi, scr + 2 * slot, scr + 2 * slot + 1);
}
// thread = element e of every source of set blockIdx.y
template <typename T, typename S>
__global__ void k_normalize_map(OfxSrcPtrs src, OfxDstPtrs dst, int per, size_t n, int nz, const double *__restrict__ mm, int guard)
{
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int set = blockIdx.y, slot = set * nz + (nz == 1 ? 0 : (int) ((unsigned) e % (unsigned) nz));      // n < 2^31
    const double lo = mm[2 * slot], den = mm[2 * slot + 1] - mm[2 * slot];
    const bool map = !guard || den > 0;
    for (int k = 0; k < per; k += 2) {                           // two sources at a time: both loads before the stores
        const bool two = k + 1 < per;
        const double x = ldw((const S *) src.p[set * per + k] + e), y = two ? ldw((const S *) src.p[set * per + k + 1] + e) : 0.0;
        stn((T *) dst.p[set * per + k] + e, map ? 255.0 * (x - lo) / den : x);
        if (two) stn((T *) dst.p[set * per + k + 1] + e, map ? 255.0 * (y - lo) / den : y);
    }
}

size_t op_minmax_scratch_doubles(int nsets, size_t npix, int nz, int chunks)
{
    return (size_t) nsets * nz * (2 + 2 * (size_t) chunks * mm_blocks(npix));
}
size_t op_pyramid_scratch_doubles() { return 2 + 2 * MM_BLOCKS; }      // a pair: one set, one channel, one chunk
const double *op_minmax_result(const double *scr) { return scr; }

static int minmax_check(ofx_ctx *ctx, int nsets, int per, size_t npix, int nz)
{
    if (nsets < 1 || per < 1 || nsets * per > OFX_MM_MAX_SRC || nz < 1 || npix < 1 || npix * nz > 0x7fffffffULL)
        return ofx_fail(ctx, OFX_ERR_ARG, "minmax: %d sets of %d sources, %zu x %d elements", nsets, per, npix, nz);
    return OFX_OK;
}
template <typename S>
int op_minmax_partial(ofx_ctx *ctx, const OfxSrcPtrs &src, int nsets, int per, size_t npix, int nz, double *scr, int chunk, int chunks)
{
    OFX_TRY(minmax_check(ctx, nsets, per, npix, nz));
    const int nb = mm_blocks(npix);
    hipLaunchKernelGGL(k_minmax_partial<S>, dim3(nb * nz, nsets), dim3(256), 0, ctx->stream, src, per, npix, nz, nb, chunk * nb,
                       chunks * nb, scr);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
int op_minmax_final(ofx_ctx *ctx, int nsets, size_t npix, int nz, double *scr, int chunks)
{
    OFX_TRY(minmax_check(ctx, nsets, 1, npix, nz));
    hipLaunchKernelGGL(k_minmax_final, dim3(nsets * nz), dim3(256), 0, ctx->stream, scr, chunks * mm_blocks(npix));
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T, typename S>
int op_normalize_map(ofx_ctx *ctx, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, size_t npix, int nz,
                     const double *scr, int guard)
{
    OFX_TRY(minmax_check(ctx, nsets, per, npix, nz));
    hipLaunchKernelGGL((k_normalize_map<T, S>), dim3(grid1d(npix * nz), nsets), dim3(256), 0, ctx->stream, src, dst, per, npix * nz, nz,
                       scr, guard);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T, typename S>
int op_normalize_sets(ofx_ctx *ctx, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, size_t npix, int nz, double *scr,
                      int guard)
{
    OFX_TRY(op_minmax_partial<S>(ctx, src, nsets, per, npix, nz, scr));
    OFX_TRY(op_minmax_final(ctx, nsets, npix, nz, scr));
    return op_normalize_map<T, S>(ctx, src, dst, nsets, per, npix, nz, scr, guard);
}

// ---- the same for sources of the byte kinds (context option "input"): four consecutive elements per lane ----------------
// A wave that loads 64 single bytes per instruction wastes the memory pipe, so a lane takes a RUN of four consecutive elements
// as one (U8), two (U16) or three (RGB8: 12 bytes = four pixels) aligned 32-bit words.  A source starts anywhere: its first
// head() elements, up to its own 32-bit boundary, and the last (n - head) % 4 go one by one through the first threads of the
// grid.  Every word of a run lies wholly inside the source.  Integer samples: min / max are taken as integers and converted once.
template <typename S> struct SrcVec;
template <> struct SrcVec<unsigned char> {
    static constexpr int BYTES = 1;
    static OFX_DEV int head(uintptr_t a) { return (int) ((4 - (a & 3)) & 3); }
    static OFX_DEV unsigned load1(const unsigned char *p) { return *p; }
    static OFX_DEV void load4(const unsigned char *p, unsigned v[4])
    {
        const unsigned w = *reinterpret_cast<const unsigned *>(p);
        v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
    }
};
template <> struct SrcVec<unsigned short> {
    static constexpr int BYTES = 2;
    static OFX_DEV int head(uintptr_t a) { return (int) ((a & 3) >> 1); }
    static OFX_DEV unsigned load1(const unsigned char *p) { return *reinterpret_cast<const unsigned short *>(p); }
    static OFX_DEV void load4(const unsigned char *p, unsigned v[4])
    {
        const unsigned w0 = reinterpret_cast<const unsigned *>(p)[0], w1 = reinterpret_cast<const unsigned *>(p)[1];
        v[0] = w0 & 0xffffu; v[1] = w0 >> 16; v[2] = w1 & 0xffffu; v[3] = w1 >> 16;
    }
};
template <> struct SrcVec<OfxRgb8> {
    static constexpr int BYTES = 3;
    static OFX_DEV int head(uintptr_t a) { return (int) (a & 3); }          // (a + 3 h) % 4 == 0 <=> h == a (mod 4)
    static OFX_DEV unsigned load1(const unsigned char *p) { return gray8(p[0], p[1], p[2]); }
    static OFX_DEV void load4(const unsigned char *p, unsigned v[4])
    {
        const unsigned w0 = reinterpret_cast<const unsigned *>(p)[0], w1 = reinterpret_cast<const unsigned *>(p)[1],
                       w2 = reinterpret_cast<const unsigned *>(p)[2];
        v[0] = gray8(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
        v[1] = gray8(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
        v[2] = gray8((w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
        v[3] = gray8((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
    }
};
// four results at d: the widest stores its address allows (a level plane of a group starts at g * size elements, so a double
// plane is only known to be 8-byte aligned; the alignment of a source's runs is the same for all of them)
OFX_DEV void store_run4(double *d, const double o[4])
{
    if ((reinterpret_cast<uintptr_t>(d) & 15) == 0) {
        reinterpret_cast<double2 *>(d)[0] = make_double2(o[0], o[1]);
        reinterpret_cast<double2 *>(d)[1] = make_double2(o[2], o[3]);
    } else {
        d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; d[3] = o[3];
    }
}
OFX_DEV void store_run4(float *d, const double o[4])
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(d);
    if ((a & 15) == 0) {
        *reinterpret_cast<float4 *>(d) = make_float4((float) o[0], (float) o[1], (float) o[2], (float) o[3]);
    } else if ((a & 7) == 0) {
        reinterpret_cast<float2 *>(d)[0] = make_float2((float) o[0], (float) o[1]);
        reinterpret_cast<float2 *>(d)[1] = make_float2((float) o[2], (float) o[3]);
    } else {
        d[0] = (float) o[0]; d[1] = (float) o[1]; d[2] = (float) o[2]; d[3] = (float) o[3];
    }
}
// block (b, set), one channel: the runs of every source of the set block-strided like k_minmax_partial's elements; block 0 also
// takes the heads and tails.  Partials in k_minmax_partial's layout, so k_minmax_final serves both.
template <typename S>
__global__ __launch_bounds__(256) void k_minmax_vec(OfxSrcPtrs src, int per, size_t npix, int nb, int first, int count,
                                                    double *__restrict__ scr)
{
    using V = SrcVec<S>;
    const int b = blockIdx.x, set = blockIdx.y, nslots = gridDim.y;
    unsigned lo = V::load1(static_cast<const unsigned char *>(src.p[set * per])), hi = lo;
    for (int k = 0; k < per; k++) {
        const unsigned char *__restrict__ p = static_cast<const unsigned char *>(src.p[set * per + k]);
        size_t h = (size_t) V::head(reinterpret_cast<uintptr_t>(p));
        if (h > npix) h = npix;
        const size_t runs = (npix - h) / 4, tail0 = h + 4 * runs;
        for (size_t r = (size_t) b * 256 + threadIdx.x; r < runs; r += (size_t) nb * 256) {
            unsigned v[4];
            V::load4(p + (h + 4 * r) * V::BYTES, v);
#pragma unroll
            for (int j = 0; j < 4; j++) { lo = v[j] < lo ? v[j] : lo; hi = v[j] > hi ? v[j] : hi; }
        }
        if (b == 0) {
            const size_t t = threadIdx.x;
            if (t < h) { const unsigned x = V::load1(p + t * V::BYTES); lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
            if (tail0 + t < npix) { const unsigned x = V::load1(p + (tail0 + t) * V::BYTES); lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
        }
    }
    double *part = scr + 2 * (size_t) nslots + (size_t) set * count + first + b;
    minmax_block_reduce((double) lo, (double) hi, part, part + (size_t) nslots * count);
}
// thread r = run r, head element r and tail element r of every source of set blockIdx.y; n = npix * nz elements, the channel
// of element e is e % nz.  mm == nullptr: a plain conversion.  The expression is k_normalize_map's.  LUT (8-bit samples, nz <=
// VEC_LUT_NZ, mm != nullptr): a sample has 256 values, so thread v of a workgroup evaluates that expression on sample v once per
// channel into LDS and an element looks its result up -- the same expression on the same operands, hence the same bits, one
// IEEE division per table entry instead of one per element.
#define VEC_LUT_NZ 4
template <typename T, typename S, bool LUT>
__global__ __launch_bounds__(256) void k_normalize_vec(OfxSrcPtrs src, OfxDstPtrs dst, int per, size_t n, int nz,
                                                       const double *__restrict__ mm, int guard)
{
    using V = SrcVec<S>;
    const size_t r = (size_t) blockIdx.x * 256 + threadIdx.x;
    const int set = blockIdx.y;
    auto eval = [&](int c, unsigned v) -> double {
        const double x = (double) v;
        if (!mm) return x;
        const int slot = set * nz + c;
        const double lo = mm[2 * slot], den = mm[2 * slot + 1] - mm[2 * slot];
        return (!guard || den > 0) ? 255.0 * (x - lo) / den : x;
    };
    __shared__ double tbl[LUT ? VEC_LUT_NZ * 256 : 1];
    if (LUT) {
        for (int c = 0; c < nz; c++) tbl[c * 256 + threadIdx.x] = eval(c, threadIdx.x);
        __syncthreads();
    }
    auto norm = [&](size_t e, unsigned v) -> double {
        const int c = nz == 1 ? 0 : (int) ((unsigned) e % (unsigned) nz);                                      // n < 2^31
        return LUT ? tbl[c * 256 + v] : eval(c, v);
    };
    for (int k = 0; k < per; k++) {
        const unsigned char *__restrict__ p = static_cast<const unsigned char *>(src.p[set * per + k]);
        T *__restrict__ d = static_cast<T *>(dst.p[set * per + k]);
        size_t h = (size_t) V::head(reinterpret_cast<uintptr_t>(p));
        if (h > n) h = n;
        const size_t runs = (n - h) / 4, tail0 = h + 4 * runs;
        if (r < runs) {
            const size_t e = h + 4 * r;
            unsigned v[4];
            V::load4(p + e * V::BYTES, v);
            const double o[4] = {norm(e, v[0]), norm(e + 1, v[1]), norm(e + 2, v[2]), norm(e + 3, v[3])};
            store_run4(d + e, o);
        }
        if (r < h) stn(d + r, norm(r, V::load1(p + r * V::BYTES)));
        if (tail0 + r < n) stn(d + tail0 + r, norm(tail0 + r, V::load1(p + (tail0 + r) * V::BYTES)));
    }
}
static inline int vec_grid(size_t n) { return (int) ((n / 4 + 3) / 256 + 1); }       // threads >= runs, heads and tails (at most 3 each)

template <typename S>
static int minmax_partial_bytes(ofx_ctx *ctx, const OfxSrcPtrs &src, int nsets, int per, size_t npix, int nz, double *scr, int chunk,
                                int chunks)
{
    if (!ctx->input_vec || nz > 1) return op_minmax_partial<S>(ctx, src, nsets, per, npix, nz, scr, chunk, chunks);
    OFX_TRY(minmax_check(ctx, nsets, per, npix, nz));
    const int nb = mm_blocks(npix);
    hipLaunchKernelGGL(k_minmax_vec<S>, dim3(nb, nsets), dim3(256), 0, ctx->stream, src, per, npix, nb, chunk * nb, chunks * nb, scr);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T, typename S>
static int normalize_map_bytes(ofx_ctx *ctx, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, size_t npix, int nz,
                               const double *scr, int guard)
{
    if (!ctx->input_vec) return op_normalize_map<T, S>(ctx, src, dst, nsets, per, npix, nz, scr, guard);
    OFX_TRY(minmax_check(ctx, nsets, per, npix, nz));
    const dim3 grid(vec_grid(npix * nz), nsets);
    if (ctx->input_lut && sizeof(S) != sizeof(unsigned short) && nz <= VEC_LUT_NZ)
        hipLaunchKernelGGL((k_normalize_vec<T, S, true>), grid, dim3(256), 0, ctx->stream, src, dst, per, npix * nz, nz, scr, guard);
    else
        hipLaunchKernelGGL((k_normalize_vec<T, S, false>), grid, dim3(256), 0, ctx->stream, src, dst, per, npix * nz, nz, scr, guard);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
// ---- ... and for frames whose rows are `pitch` bytes apart (context option "input_pitch") ------------------------------------
// A frame is ny rows of w elements (RGB8: pixels), row i at byte i * pitch; the results are dense, element j of row i at i * w + j.
// A workgroup takes a TILE (OfxRows, rows_tile in ofx_device.h): 1 << lbx consecutive SLOTS of a row by (256 >> lbx) * 4 rows, a
// thread one slot of four of those rows; the tile's place is found with one division per workgroup, so a lane's column never
// costs one.  lbx follows the row's length, which keeps the lanes busy on short rows (a 64-column region: 16 or 32 rows per
// workgroup) and a wave on one row of a long one.  Slot = element for the one-element-per-thread kernels, a group of four for the
// byte kinds' (below).  Four rows per thread also spread a workgroup's table of quotients (LUT) over four times the elements.
OfxRows op_rows_geom(int w, int ny, size_t pitch, bool groups)
{
    OfxRows R;
    const int slots = groups ? w / 4 + 2 : w;                  // a row's groups: below
    R.w = w;
    R.ny = ny;
    R.pitch = pitch;
    R.lbx = 2;
    while ((1 << R.lbx) < slots && R.lbx < 8) R.lbx++;
    R.cx = ofx_cdiv(slots, 1 << R.lbx);
    R.tiles = R.cx * ofx_cdiv(ny, (256 >> R.lbx) * 4);
    return R;
}
// k_minmax_partial on pitched rows: block (c * nb + b, set) strides over the tiles, a slot is a PIXEL of nz channels
template <typename S>
__global__ __launch_bounds__(256) void k_minmax_partial_p(OfxSrcPtrs src, int per, OfxRows R, int nz, int nb, int first, int count,
                                                          double *__restrict__ scr)
{
    const int c = blockIdx.x / nb, b = blockIdx.x - c * nb, set = blockIdx.y;
    const int nslots = gridDim.y * nz, slot = set * nz + c;
    double lo = ldw((const S *) src.p[set * per] + c), hi = lo;
    for (int k = 0; k < per; k += 2) {
        const unsigned char *__restrict__ I1 = static_cast<const unsigned char *>(src.p[set * per + k]);
        const unsigned char *__restrict__ I2 = static_cast<const unsigned char *>(src.p[set * per + (k + 1 < per ? k + 1 : k)]);
        for (int t = b; t < R.tiles; t += nb) {
            int q, i0, i1, di;
            rows_tile(t, R.cx, R.lbx, R.ny, 4, q, i0, i1, di);
            if (q >= R.w) continue;
            const size_t e = (size_t) q * nz + c;
            for (int i = i0; i < i1; i += di) {
                const size_t o = (size_t) i * R.pitch;
                const double x = ldw(reinterpret_cast<const S *>(I1 + o) + e), y = ldw(reinterpret_cast<const S *>(I2 + o) + e);
                lo = x < lo ? x : lo; hi = x > hi ? x : hi;
                lo = y < lo ? y : lo; hi = y > hi ? y : hi;
            }
        }
    }
    double *part = scr + 2 * (size_t) nslots + (size_t) slot * count + first + b;
    minmax_block_reduce(lo, hi, part, part + (size_t) nslots * count);
}
// k_normalize_map on pitched rows: a slot is an ELEMENT of the row of w = nx * nz, its channel the column modulo nz -- taken once
// per thread, which keeps its column over the rows of the tile.  The expression is k_normalize_map's.
template <typename T, typename S>
__global__ __launch_bounds__(256) void k_normalize_map_p(OfxSrcPtrs src, OfxDstPtrs dst, int per, OfxRows R, int nz,
                                                         const double *__restrict__ mm, int guard)
{
    int q, i0, i1, di;
    rows_tile(blockIdx.x, R.cx, R.lbx, R.ny, 4, q, i0, i1, di);
    if (q >= R.w) return;
    const int set = blockIdx.y, slot = set * nz + (nz == 1 ? 0 : (int) ((unsigned) q % (unsigned) nz));
    const double lo = mm[2 * slot], den = mm[2 * slot + 1] - mm[2 * slot];
    const bool map = !guard || den > 0;
    for (int i = i0; i < i1; i += di) {
        const size_t o = (size_t) i * R.pitch, e = (size_t) i * R.w + q;
        for (int k = 0; k < per; k += 2) {                       // two sources at a time: both loads before the stores
            const bool two = k + 1 < per;
            const double x = ldw(reinterpret_cast<const S *>(static_cast<const unsigned char *>(src.p[set * per + k]) + o) + q);
            const double y = two ? ldw(reinterpret_cast<const S *>(static_cast<const unsigned char *>(src.p[set * per + k + 1]) + o) + q) : 0.0;
            stn((T *) dst.p[set * per + k] + e, map ? 255.0 * (x - lo) / den : x);
            if (two) stn((T *) dst.p[set * per + k + 1] + e, map ? 255.0 * (y - lo) / den : y);
        }
    }
}
// The byte kinds, four elements per lane PER ROW.  A row starts anywhere (base + i * pitch: its head rotates from row to row when
// pitch % 4 != 0), so the row is cut into GROUPS of four columns [4 g - s, 4 g - s + 4), s = (4 - head) & 3 with head the row's
// elements up to its own 32-bit boundary: group 0 holds the head (its first s places lie before the row), the groups wholly
// inside the row start on a 32-bit boundary and are loaded as SrcVec's aligned words, the last one holds the tail.  A place outside
// [0, w) is never read: the groups across the row's ends, and every group of a row shorter than a word, go element by element.
// At most w / 4 + 2 groups.
// k_minmax_vec on pitched rows (one channel)
template <typename S>
__global__ __launch_bounds__(256) void k_minmax_vec_p(OfxSrcPtrs src, int per, OfxRows R, int nb, int first, int count,
                                                      double *__restrict__ scr)
{
    using V = SrcVec<S>;
    const int b = blockIdx.x, set = blockIdx.y, nslots = gridDim.y;
    unsigned lo = V::load1(static_cast<const unsigned char *>(src.p[set * per])), hi = lo;
    for (int k = 0; k < per; k++) {
        const unsigned char *__restrict__ p = static_cast<const unsigned char *>(src.p[set * per + k]);
        for (int t = b; t < R.tiles; t += nb) {
            int g, i0, i1, di;
            rows_tile(t, R.cx, R.lbx, R.ny, 4, g, i0, i1, di);
            for (int i = i0; i < i1; i += di) {
                const unsigned char *row = p + (size_t) i * R.pitch;
                const long long col0 = 4LL * g - ((4 - V::head(reinterpret_cast<uintptr_t>(row))) & 3);
                if (col0 >= R.w) continue;
                if (col0 >= 0 && col0 + 4 <= R.w) {
                    unsigned v[4];
                    V::load4(row + (size_t) col0 * V::BYTES, v);
#pragma unroll
                    for (int j = 0; j < 4; j++) { lo = v[j] < lo ? v[j] : lo; hi = v[j] > hi ? v[j] : hi; }
                } else {
                    for (int j = 0; j < 4; j++) {
                        const long long col = col0 + j;
                        if (col < 0 || col >= R.w) continue;
                        const unsigned x = V::load1(row + (size_t) col * V::BYTES);
                        lo = x < lo ? x : lo; hi = x > hi ? x : hi;
                    }
                }
            }
        }
    }
    double *part = scr + 2 * (size_t) nslots + (size_t) set * count + first + b;
    minmax_block_reduce((double) lo, (double) hi, part, part + (size_t) nslots * count);
}
// k_normalize_vec on pitched rows: thread = one group of four rows of its tile, of every source of set blockIdx.y; w = nx * nz elements
// per row.
// A row holds whole pixels, so the channel of a place is its column modulo nz: (4 g) % nz once per thread, then by counting.
// mm == nullptr and LUT as k_normalize_vec; the expression is k_normalize_map's.
template <typename T, typename S, bool LUT>
__global__ __launch_bounds__(256) void k_normalize_vec_p(OfxSrcPtrs src, OfxDstPtrs dst, int per, OfxRows R, int nz,
                                                         const double *__restrict__ mm, int guard)
{
    using V = SrcVec<S>;
    const int set = blockIdx.y;
    auto eval = [&](int c, unsigned v) -> double {
        const double x = (double) v;
        if (!mm) return x;
        const int slot = set * nz + c;
        const double lo = mm[2 * slot], den = mm[2 * slot + 1] - mm[2 * slot];
        return (!guard || den > 0) ? 255.0 * (x - lo) / den : x;
    };
    __shared__ double tbl[LUT ? VEC_LUT_NZ * 256 : 1];
    if (LUT) {
        for (int c = 0; c < nz; c++) tbl[c * 256 + threadIdx.x] = eval(c, threadIdx.x);
        __syncthreads();
    }
    auto norm = [&](int c, unsigned v) -> double { return LUT ? tbl[c * 256 + v] : eval(c, v); };
    int g, i0, i1, di;
    rows_tile(blockIdx.x, R.cx, R.lbx, R.ny, 4, g, i0, i1, di);
    const int cg = nz == 1 ? 0 : (int) ((4u * (unsigned) g) % (unsigned) nz);
    for (int i = i0; i < i1; i += di) {
        for (int k = 0; k < per; k++) {
            const unsigned char *__restrict__ row = static_cast<const unsigned char *>(src.p[set * per + k]) + (size_t) i * R.pitch;
            T *__restrict__ d = static_cast<T *>(dst.p[set * per + k]) + (size_t) i * R.w;
            const int s = (4 - V::head(reinterpret_cast<uintptr_t>(row))) & 3;
            const long long col0 = 4LL * g - s;
            if (col0 >= R.w) continue;
            int c = cg - s;                                      // channel of place col0, which may lie before the row: s <= 3, nz >= 2
            if (nz == 1) c = 0;
            if (c < 0) c += nz;
            if (c < 0) c += nz;
            if (col0 >= 0 && col0 + 4 <= R.w) {
                unsigned v[4];
                V::load4(row + (size_t) col0 * V::BYTES, v);
                double o[4];
#pragma unroll
                for (int j = 0; j < 4; j++) { o[j] = norm(c, v[j]); c = c + 1 == nz ? 0 : c + 1; }
                store_run4(d + col0, o);
            } else {
                for (int j = 0; j < 4; j++) {
                    const long long col = col0 + j;
                    if (col >= 0 && col < R.w) stn(d + col, norm(c, V::load1(row + (size_t) col * V::BYTES)));
                    c = c + 1 == nz ? 0 : c + 1;
                }
            }
        }
    }
}

static int rows_check(ofx_ctx *ctx, int kind, int nsets, int per, int nx, int ny, size_t pitch, int nz)
{
    if (kind < OFX_SRC_F64 || kind > OFX_SRC_RGB8) return ofx_fail(ctx, OFX_ERR_ARG, "source kind %d", kind);
    if (kind == OFX_SRC_RGB8 && nz != 1) return ofx_fail(ctx, OFX_ERR_ARG, "RGB8 sources give one gray channel (nz = %d)", nz);
    if (nx < 1 || ny < 1) return ofx_fail(ctx, OFX_ERR_ARG, "minmax: frames of %d x %d", nx, ny);
    OFX_TRY(minmax_check(ctx, nsets, per, (size_t) nx * ny, nz));
    if (pitch && ny > 0x7fffffff - 1024)                      // rows_tile counts rows in int, a tile past the last one included
        return ofx_fail(ctx, OFX_ERR_ARG, "minmax: %d pitched rows (at most 2^31 - 1025)", ny);
    if (pitch && (pitch < (size_t) nx * nz * ofx_src_bytes(kind) || pitch % ofx_src_align(kind)))
        return ofx_fail(ctx, OFX_ERR_ARG, "minmax: pitch of %zu bytes for rows of %zu bytes", pitch, (size_t) nx * nz * ofx_src_bytes(kind));
    return OFX_OK;
}
template <typename S, bool BYTES>                               // BYTES: S is a byte kind (SrcVec<S> exists)
static int minmax_partial_rows(ofx_ctx *ctx, const OfxSrcPtrs &src, int nsets, int per, int nx, int ny, size_t pitch, int nz,
                               double *scr, int chunk, int chunks)
{
    const int nb = mm_blocks((size_t) nx * ny);                 // the flat launch's pieces: one scratch layout, one k_minmax_final
    bool vec = false;
    if constexpr (BYTES) {
        vec = ctx->input_vec && nz == 1;
        if (vec)
            hipLaunchKernelGGL(k_minmax_vec_p<S>, dim3(nb, nsets), dim3(256), 0, ctx->stream, src, per, op_rows_geom(nx, ny, pitch, true),
                               nb, chunk * nb, chunks * nb, scr);
    }
    if (!vec)
        hipLaunchKernelGGL(k_minmax_partial_p<S>, dim3(nb * nz, nsets), dim3(256), 0, ctx->stream, src, per,
                           op_rows_geom(nx, ny, pitch, false), nz, nb, chunk * nb, chunks * nb, scr);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T, typename S, bool BYTES>
static int normalize_map_rows(ofx_ctx *ctx, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, int nx, int ny,
                              size_t pitch, int nz, const double *scr, int guard)
{
    bool vec = false;
    if constexpr (BYTES) vec = ctx->input_vec != 0;
    if (!vec) {
        const OfxRows R = op_rows_geom(nx * nz, ny, pitch, false);
        hipLaunchKernelGGL((k_normalize_map_p<T, S>), dim3(R.tiles, nsets), dim3(256), 0, ctx->stream, src, dst, per, R, nz, scr, guard);
    } else if constexpr (BYTES) {
        const OfxRows R = op_rows_geom(nx * nz, ny, pitch, true);
        if (ctx->input_lut && sizeof(S) != sizeof(unsigned short) && nz <= VEC_LUT_NZ)
            hipLaunchKernelGGL((k_normalize_vec_p<T, S, true>), dim3(R.tiles, nsets), dim3(256), 0, ctx->stream, src, dst, per, R, nz, scr, guard);
        else
            hipLaunchKernelGGL((k_normalize_vec_p<T, S, false>), dim3(R.tiles, nsets), dim3(256), 0, ctx->stream, src, dst, per, R, nz, scr, guard);
    }
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
int op_minmax_partial_in(ofx_ctx *ctx, int kind, const OfxSrcPtrs &src, int nsets, int per, int nx, int ny, size_t pitch, int nz,
                         double *scr, int chunk, int chunks)
{
    OFX_TRY(rows_check(ctx, kind, nsets, per, nx, ny, pitch, nz));
    const size_t npix = (size_t) nx * ny;
    switch (kind) {
    case OFX_SRC_F64: return pitch ? minmax_partial_rows<double, false>(ctx, src, nsets, per, nx, ny, pitch, nz, scr, chunk, chunks)
                                   : op_minmax_partial<double>(ctx, src, nsets, per, npix, nz, scr, chunk, chunks);
    case OFX_SRC_F32: return pitch ? minmax_partial_rows<float, false>(ctx, src, nsets, per, nx, ny, pitch, nz, scr, chunk, chunks)
                                   : op_minmax_partial<float>(ctx, src, nsets, per, npix, nz, scr, chunk, chunks);
    case OFX_SRC_U8:  return pitch ? minmax_partial_rows<unsigned char, true>(ctx, src, nsets, per, nx, ny, pitch, nz, scr, chunk, chunks)
                                   : minmax_partial_bytes<unsigned char>(ctx, src, nsets, per, npix, nz, scr, chunk, chunks);
    case OFX_SRC_U16: return pitch ? minmax_partial_rows<unsigned short, true>(ctx, src, nsets, per, nx, ny, pitch, nz, scr, chunk, chunks)
                                   : minmax_partial_bytes<unsigned short>(ctx, src, nsets, per, npix, nz, scr, chunk, chunks);
    default:          return pitch ? minmax_partial_rows<OfxRgb8, true>(ctx, src, nsets, per, nx, ny, pitch, nz, scr, chunk, chunks)
                                   : minmax_partial_bytes<OfxRgb8>(ctx, src, nsets, per, npix, nz, scr, chunk, chunks);
    }
}
template <typename T>
int op_normalize_map_in(ofx_ctx *ctx, int kind, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, int nx, int ny,
                        size_t pitch, int nz, const double *scr, int guard)
{
    OFX_TRY(rows_check(ctx, kind, nsets, per, nx, ny, pitch, nz));
    const size_t npix = (size_t) nx * ny;
    switch (kind) {
    case OFX_SRC_F64: return pitch ? normalize_map_rows<T, double, false>(ctx, src, dst, nsets, per, nx, ny, pitch, nz, scr, guard)
                                   : op_normalize_map<T, double>(ctx, src, dst, nsets, per, npix, nz, scr, guard);
    case OFX_SRC_F32: return pitch ? normalize_map_rows<T, float, false>(ctx, src, dst, nsets, per, nx, ny, pitch, nz, scr, guard)
                                   : op_normalize_map<T, float>(ctx, src, dst, nsets, per, npix, nz, scr, guard);
    case OFX_SRC_U8:  return pitch ? normalize_map_rows<T, unsigned char, true>(ctx, src, dst, nsets, per, nx, ny, pitch, nz, scr, guard)
                                   : normalize_map_bytes<T, unsigned char>(ctx, src, dst, nsets, per, npix, nz, scr, guard);
    case OFX_SRC_U16: return pitch ? normalize_map_rows<T, unsigned short, true>(ctx, src, dst, nsets, per, nx, ny, pitch, nz, scr, guard)
                                   : normalize_map_bytes<T, unsigned short>(ctx, src, dst, nsets, per, npix, nz, scr, guard);
    default:          return pitch ? normalize_map_rows<T, OfxRgb8, true>(ctx, src, dst, nsets, per, nx, ny, pitch, nz, scr, guard)
                                   : normalize_map_bytes<T, OfxRgb8>(ctx, src, dst, nsets, per, npix, nz, scr, guard);
    }
}
template <typename T>
int op_normalize_sets_in(ofx_ctx *ctx, int kind, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int nsets, int per, int nx, int ny,
                         size_t pitch, int nz, double *scr, int guard)
{
    OFX_TRY(op_minmax_partial_in(ctx, kind, src, nsets, per, nx, ny, pitch, nz, scr));
    OFX_TRY(op_minmax_final(ctx, nsets, (size_t) nx * ny, nz, scr));
    return op_normalize_map_in<T>(ctx, kind, src, dst, nsets, per, nx, ny, pitch, nz, scr, guard);
}
template <typename T>
int op_convert_sources_in(ofx_ctx *ctx, int kind, const OfxSrcPtrs &src, const OfxDstPtrs &dst, int count, int nx, int ny, size_t pitch)
{
    if (kind != OFX_SRC_U8 && kind != OFX_SRC_U16 && kind != OFX_SRC_RGB8) return ofx_fail(ctx, OFX_ERR_ARG, "source kind %d", kind);
    OFX_TRY(rows_check(ctx, kind, 1, count, nx, ny, pitch, 1));
    const size_t n = (size_t) nx * ny;
    const double *none = nullptr;
    if (pitch) {
        const OfxRows R = op_rows_geom(nx, ny, pitch, true);
        const dim3 grid(R.tiles, 1);
        if (kind == OFX_SRC_U8)
            hipLaunchKernelGGL((k_normalize_vec_p<T, unsigned char, false>), grid, dim3(256), 0, ctx->stream, src, dst, count, R, 1, none, 0);
        else if (kind == OFX_SRC_U16)
            hipLaunchKernelGGL((k_normalize_vec_p<T, unsigned short, false>), grid, dim3(256), 0, ctx->stream, src, dst, count, R, 1, none, 0);
        else
            hipLaunchKernelGGL((k_normalize_vec_p<T, OfxRgb8, false>), grid, dim3(256), 0, ctx->stream, src, dst, count, R, 1, none, 0);
        OFX_LAUNCH_CHECK(ctx);
        return OFX_OK;
    }
    const dim3 grid(vec_grid(n), 1);
    if (kind == OFX_SRC_U8)
        hipLaunchKernelGGL((k_normalize_vec<T, unsigned char, false>), grid, dim3(256), 0, ctx->stream, src, dst, count, n, 1, none, 0);
    else if (kind == OFX_SRC_U16)
        hipLaunchKernelGGL((k_normalize_vec<T, unsigned short, false>), grid, dim3(256), 0, ctx->stream, src, dst, count, n, 1, none, 0);
    else
        hipLaunchKernelGGL((k_normalize_vec<T, OfxRgb8, false>), grid, dim3(256), 0, ctx->stream, src, dst, count, n, 1, none, 0);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

// ---- gaussian (src/operators.cpp:506-624) -----------------------------------------------------------
int ofx_gauss_taps(double sigma, GaussTaps *t)
{
    const double den = 2 * sigma * sigma;
    const int size = (int) (5 * sigma) + 1;                 // DEFAULT_GAUSSIAN_WINDOW_SIZE, operators.h:120
    if (size < 1 || size > OFX_GAUSS_MAX_TAPS) return OFX_ERR_ARG;
    t->size = size;
    t->dirichlet = 0;
    for (int i = 0; i < size; i++)
        t->B[i] = 1 / (sigma * sqrt(2.0 * 3.1415926)) * exp(-i * i / den);   // :527 (pi truncated)
    double norm = 0;
    for (int i = 0; i < size; i++) norm += t->B[i];
    norm *= 2;
    norm -= t->B[0];
    for (int i = 0; i < size; i++) t->B[i] /= norm;
    return OFX_OK;
}

// reflecting boundary of :557-562: left of the image the edge sample is NOT repeated (t=-1 -> 1),
// right of it it IS repeated (t=n -> n-1).
OFX_DEV int gauss_reflect(int t, int n) { return t < 0 ? -t : (t >= n ? 2 * n - 1 - t : t); }

// Planes of a batched launch: blockIdx.z in [0, 2 G) = image (A, B) x pair; the G planes of an image are `stride` apart
template <typename T> struct OfxPlanes2 {
    T     *a, *b;
    int    G;
    size_t stride;
    OFX_DEV T *at(int z) const { return (z < G ? a : b) + (size_t) (z < G ? z : z - G) * stride; }
};
template <typename T, bool ALONG_X>
OFX_DEV void gauss_pass_px(const T *__restrict__ in, T *__restrict__ out, int nx, int ny, const GaussTaps &taps)
{
    const int j = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t p = (size_t) i * nx + j;
    double sum = taps.B[0] * ldw(in + p);
    if (taps.dirichlet) {                                    // BOUNDARY_CONDITION_DIRICHLET (:551-555, :591-595): 0 outside the image
        if (ALONG_X) {
            const T *row = in + (size_t) i * nx;
            for (int k = 1; k < taps.size; k++)
                sum += taps.B[k] * ((j - k >= 0 ? ldw(row + j - k) : 0.0) + (j + k < nx ? ldw(row + j + k) : 0.0));
        } else {
            for (int k = 1; k < taps.size; k++)
                sum += taps.B[k] * ((i - k >= 0 ? ldw(in + (size_t) (i - k) * nx + j) : 0.0) +
                                    (i + k < ny ? ldw(in + (size_t) (i + k) * nx + j) : 0.0));
        }
        stn(out + p, sum);
        return;
    }
    if (ALONG_X) {
        const T *row = in + (size_t) i * nx;
        for (int k = 1; k < taps.size; k++)
            sum += taps.B[k] * (ldw(row + gauss_reflect(j - k, nx)) + ldw(row + gauss_reflect(j + k, nx)));
    } else {
        for (int k = 1; k < taps.size; k++)
            sum += taps.B[k] * (ldw(in + (size_t) gauss_reflect(i - k, ny) * nx + j) +
                                ldw(in + (size_t) gauss_reflect(i + k, ny) * nx + j));
    }
    stn(out + p, sum);
}
template <typename T, bool ALONG_X>
__global__ void k_gauss_pass_g(OfxPlanes2<const T> in, OfxPlanes2<T> out, int nx, int ny, GaussTaps taps)
{
    gauss_pass_px<T, ALONG_X>(in.at(blockIdx.z), out.at(blockIdx.z), nx, ny, taps);
}

// Both passes in one launch for the pyramids of a lockstep group: a block brings a (GXY_TH + 2 r) x (64 + 2 r) region of the
// input into LDS (reflected indices resolved while loading), runs the row pass on all of its rows, then the column pass on the
// GXY_TH inner ones -- the intermediate image never touches memory (the two-pass form writes and re-reads it: 4 plane moves
// instead of 2).  Per pixel the same sums in the same order as k_gauss_pass_g, the intermediate rounded to the storage type as
// the two-pass form stores it.  in != out (neighbouring blocks read what a block would overwrite).  Radius <= GXY_RMAX.
#define GXY_TH 32
#define GXY_RMAX 8
template <typename T>
__global__ __launch_bounds__(256) void k_gauss_xy_g(OfxPlanes2<const T> in_p, OfxPlanes2<T> out_p, int nx, int ny, GaussTaps taps)
{
    __shared__ double s_in[(GXY_TH + 2 * GXY_RMAX) * (64 + 2 * GXY_RMAX)];
    __shared__ double s_mid[(GXY_TH + 2 * GXY_RMAX) * 64];
    const T *__restrict__ in = in_p.at(blockIdx.z);
    T *__restrict__ out = out_p.at(blockIdx.z);
    const int R = taps.size - 1, W = 64 + 2 * R, H = GXY_TH + 2 * R;
    const int j0 = blockIdx.x * 64, i0 = blockIdx.y * GXY_TH;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int k = tid; k < W * H; k += 256) {
        const int r = k / W, c = k - r * W;
        // rows / columns beyond the image on the far side of a border block are never used: clamp them into range
        int i = gauss_reflect(i0 - R + r, ny), j = gauss_reflect(j0 - R + c, nx);
        i = i < 0 ? 0 : (i > ny - 1 ? ny - 1 : i);
        j = j < 0 ? 0 : (j > nx - 1 ? nx - 1 : j);
        s_in[r * W + c] = ldw(in + (size_t) i * nx + j);
    }
    __syncthreads();
    for (int r = threadIdx.y; r < H; r += 4) {                   // row pass, :541-575
        const double *row = s_in + r * W + R + threadIdx.x;
        double sum = taps.B[0] * row[0];
        for (int k = 1; k < taps.size; k++) sum += taps.B[k] * (row[-k] + row[k]);
        s_mid[r * 64 + threadIdx.x] = sizeof(T) == sizeof(float) ? (double) (float) sum : sum;
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;
    if (j >= nx) return;
    for (int r = threadIdx.y; r < GXY_TH; r += 4) {              // column pass, :577-611
        const int i = i0 + r;
        if (i >= ny) break;
        const double *col = s_mid + (r + R) * 64 + threadIdx.x;
        double sum = taps.B[0] * col[0];
        for (int k = 1; k < taps.size; k++) sum += taps.B[k] * (col[-k * 64] + col[k * 64]);
        stn(out + (size_t) i * nx + j, sum);
    }
}

// The same with the radius R a template parameter (the pyramids use 4 and 5).  k_gauss_xy_g above spends its time on index
// arithmetic (a division, two reflections and a 64-bit address per loaded element) and on 2 R + 1 LDS reads per output of both
// passes -- 1.2 TB/s of plane traffic.  Here the reflected column of a thread is computed once (it does not depend on the row),
// the reflected row once per row, and the column pass slides a register window down the thread's column: 8 + 2 R reads for 8
// outputs.  Same sums in the same order per pixel.
template <typename T, int R>
__global__ __launch_bounds__(256) void k_gauss_xy_gr(OfxPlanes2<const T> in_p, OfxPlanes2<T> out_p, int nx, int ny, GaussTaps taps)
{
    constexpr int W = 64 + 2 * R, H = GXY_TH + 2 * R;
    __shared__ double s_in[H * W];
    __shared__ double s_mid[H * 64];
    const T *__restrict__ in = in_p.at(blockIdx.z);
    T *__restrict__ out = out_p.at(blockIdx.z);
    const int j0 = blockIdx.x * 64, i0 = blockIdx.y * GXY_TH;
    const int tx = threadIdx.x, ty = threadIdx.y;
    // columns of this thread in the staged region: tx, and tx + 64 for the first 2 R lanes; beyond the image on the far side of
    // a border block: never used, clamped into range
    int ja = gauss_reflect(j0 - R + tx, nx), jb = gauss_reflect(j0 - R + tx + 64, nx);
    ja = ja < 0 ? 0 : (ja > nx - 1 ? nx - 1 : ja);
    jb = jb < 0 ? 0 : (jb > nx - 1 ? nx - 1 : jb);
    for (int r = ty; r < H; r += 4) {
        int i = gauss_reflect(i0 - R + r, ny);
        i = i < 0 ? 0 : (i > ny - 1 ? ny - 1 : i);
        const T *__restrict__ row = in + (size_t) i * nx;
        s_in[r * W + tx] = ldw(row + ja);
        if (tx < 2 * R) s_in[r * W + tx + 64] = ldw(row + jb);
    }
    __syncthreads();
    for (int r = ty; r < H; r += 4) {                            // row pass, :541-575
        const double *row = s_in + r * W + R + tx;
        double sum = taps.B[0] * row[0];
#pragma unroll
        for (int k = 1; k <= R; k++) sum += taps.B[k] * (row[-k] + row[k]);
        s_mid[r * 64 + tx] = sizeof(T) == sizeof(float) ? (double) (float) sum : sum;
    }
    __syncthreads();
    const int j = j0 + tx;
    if (j >= nx) return;
    constexpr int SEG = GXY_TH / 4;                              // rows per thread of the column pass
    double win[SEG + 2 * R];
#pragma unroll
    for (int q = 0; q < SEG + 2 * R; q++) win[q] = s_mid[(ty * SEG + q) * 64 + tx];
#pragma unroll
    for (int o = 0; o < SEG; o++) {                              // column pass, :577-611
        const int i = i0 + ty * SEG + o;
        double sum = taps.B[0] * win[o + R];
#pragma unroll
        for (int k = 1; k <= R; k++) sum += taps.B[k] * (win[o + R - k] + win[o + R + k]);
        if (i < ny) stn(out + (size_t) i * nx + j, sum);
    }
}
// zoom_out with zfactor = 1/2 (src/zoom.cpp:41-78) in ONE launch: the bicubic sample of the smoothed image at (2 j1, 2 i1) is the
// smoothed pixel itself -- at integer coordinates cubic_interpolation_cell returns v1 + 0.5 * 0 * (...) = v1 in both directions
// (src/bicubic_interpolation.cpp:108-145; the smoothed values are >= 0, so no signed zero is involved) -- and 2 j1 <= nx - 1 for
// every output column of zoom_size.  So only the even columns of the row pass and the even rows of the column pass are computed
// (same sums in the same order per pixel), written straight into the coarser level: the smoothed full-size image is neither
// stored nor re-read (26 -> 10 bytes per input pixel) and the resample launch disappears.
#define GXD_THO 12                                               // output rows per block (24 input rows + 2 R of halo)
template <typename T, int R>
__global__ __launch_bounds__(256) void k_gauss_xy_dec(OfxPlanes2<const T> in_p, OfxPlanes2<T> out_p, int nx, int ny, int nxo, int nyo,
                                                      GaussTaps taps)
{
    constexpr int W = 128 + 2 * R, H = 2 * GXD_THO + 2 * R;
    __shared__ double s_in[H * W];
    __shared__ double s_mid[H * 64];
    const T *__restrict__ in = in_p.at(blockIdx.z);
    T *__restrict__ out = out_p.at(blockIdx.z);
    const int j0 = blockIdx.x * 128, i0 = blockIdx.y * 2 * GXD_THO;       // origin of the block's input region
    const int tx = threadIdx.x, ty = threadIdx.y;
    int jc[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        int j = gauss_reflect(j0 - R + tx + 64 * q, nx);
        jc[q] = j < 0 ? 0 : (j > nx - 1 ? nx - 1 : j);
    }
    for (int r = ty; r < H; r += 4) {
        int i = gauss_reflect(i0 - R + r, ny);
        i = i < 0 ? 0 : (i > ny - 1 ? ny - 1 : i);
        const T *__restrict__ row = in + (size_t) i * nx;
        s_in[r * W + tx] = ldw(row + jc[0]);
        s_in[r * W + tx + 64] = ldw(row + jc[1]);
        if (tx < 2 * R) s_in[r * W + tx + 128] = ldw(row + jc[2]);
    }
    __syncthreads();
    for (int r = ty; r < H; r += 4) {                            // row pass at the even columns, operators.cpp:541-575
        const double *row = s_in + r * W + R + 2 * tx;
        double sum = taps.B[0] * row[0];
#pragma unroll
        for (int k = 1; k <= R; k++) sum += taps.B[k] * (row[-k] + row[k]);
        s_mid[r * 64 + tx] = sizeof(T) == sizeof(float) ? (double) (float) sum : sum;
    }
    __syncthreads();
    const int jo = blockIdx.x * 64 + tx;
    if (jo >= nxo) return;
    constexpr int SEG = GXD_THO / 4;                             // output rows per thread
#pragma unroll
    for (int o = 0; o < SEG; o++) {                              // column pass at the even rows, :577-611
        const int lo = ty * SEG + o, io = blockIdx.y * GXD_THO + lo;
        const double *c = s_mid + (R + 2 * lo) * 64 + tx;
        double sum = taps.B[0] * c[0];
#pragma unroll
        for (int k = 1; k <= R; k++) sum += taps.B[k] * (c[-k * 64] + c[k * 64]);
        if (io < nyo) stn(out + (size_t) io * nxo + jo, sum);
    }
}

template <typename T>
static void gauss_xy_launch(ofx_ctx *ctx, dim3 grid, OfxPlanes2<const T> in, OfxPlanes2<T> out, int nx, int ny, const GaussTaps &taps)
{
    const dim3 block(64, 4);
#define OFX_GXY(R_) case R_: hipLaunchKernelGGL((k_gauss_xy_gr<T, R_>), grid, block, 0, ctx->stream, in, out, nx, ny, taps); break
    switch (taps.size - 1) {
        OFX_GXY(1); OFX_GXY(2); OFX_GXY(3); OFX_GXY(4); OFX_GXY(5); OFX_GXY(6); OFX_GXY(7); OFX_GXY(8);
    default: hipLaunchKernelGGL(k_gauss_xy_g<T>, grid, block, 0, ctx->stream, in, out, nx, ny, taps); break;
    }
#undef OFX_GXY
}

// The taps of a Gaussian on an nx x ny image, or the error.  The reference throws when size > xdim (:520-522) and reads out of
// bounds when size == xdim or size >= ydim -- all three are reported as OFX_ERR_SIGMA here.  (Dirichlet: no check, the padded
// line always has room.)
static int gauss_taps_checked(ofx_ctx *ctx, double sigma, int nx, int ny, int dirichlet, GaussTaps *taps)
{
    if (ofx_gauss_taps(sigma, taps) != OFX_OK)
        return ofx_fail(ctx, OFX_ERR_ARG, "gaussian: sigma %g needs more than %d taps", sigma, OFX_GAUSS_MAX_TAPS);
    taps->dirichlet = dirichlet != 0;
    if (!dirichlet && (taps->size >= nx || taps->size >= ny))
        return ofx_fail(ctx, OFX_ERR_SIGMA, "GaussianSmooth: sigma too large (radius %d, image %dx%d)", taps->size, nx, ny);
    return OFX_OK;
}

// gaussian in place on the first nx * ny elements of `count` images, one launch per pass (blockIdx.z = image): images
// 0 .. split - 1 start at A, the others at B, each `stride` elements after the one before; tmp holds count planes of nx * ny.
template <typename T>
int op_gaussian_planes(ofx_ctx *ctx, int count, int split, T *A, T *B, size_t stride, T *tmp, int nx, int ny, double sigma, int dirichlet)
{
    GaussTaps taps;
    if (count < 1 || count > OFX_MAX_PLANES || split < 1 || split > count) return ofx_fail(ctx, OFX_ERR_ARG, "gaussian: %d planes (%d first)", count, split);
    OFX_TRY(gauss_taps_checked(ctx, sigma, nx, ny, dirichlet, &taps));
    const size_t n = (size_t) nx * ny;
    dim3 g = grid2d(nx, ny);
    g.z = count;
    hipLaunchKernelGGL((k_gauss_pass_g<T, true>), g, block2d(), 0, ctx->stream, OfxPlanes2<const T>{A, B, split, stride},
                       OfxPlanes2<T>{tmp, tmp + (size_t) split * n, split, n}, nx, ny, taps);
    OFX_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL((k_gauss_pass_g<T, false>), g, block2d(), 0, ctx->stream, OfxPlanes2<const T>{tmp, tmp + (size_t) split * n, split, n},
                       OfxPlanes2<T>{A, B, split, stride}, nx, ny, taps);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
// the 2 G images of a lockstep group of pairs: A / B = the G first / second images
template <typename T>
int op_gaussian_group(ofx_ctx *ctx, int G, T *A, T *B, size_t stride, T *tmp, int nx, int ny, double sigma, int dirichlet)
{
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "gaussian: group of %d", G);
    return op_gaussian_planes<T>(ctx, 2 * G, G, A, B, stride, tmp, nx, ny, sigma, dirichlet);
}

// ---- bicubic resampling: zoom_out / zoom_in (src/zoom.cpp:41-78,132-155) ---------------------------
template <typename T>
OFX_DEV void resample_px(const T *__restrict__ in, T *__restrict__ out, int nx, int ny, int nxx, int nyy, double fx, double fy)
{
    const int j1 = blockIdx.x * BX + threadIdx.x;
    const int i1 = blockIdx.y * BY + threadIdx.y;
    if (j1 >= nxx || i1 >= nyy) return;
    const double i2 = i1 / fy, j2 = j1 / fx;
    const BicubicTaps t = bicubic_taps(j2, i2, nx, ny);
    stn(out + (size_t) i1 * nxx + j1, bicubic_sample(in, t, nx));
}
template <typename T>
__global__ void k_resample_g(OfxPlanes2<const T> in, OfxPlanes2<T> out, int nx, int ny, int nxx, int nyy, double fx, double fy)
{
    resample_px<T>(in.at(blockIdx.z), out.at(blockIdx.z), nx, ny, nxx, nyy, fx, fy);
}

template <typename T>
__global__ void k_zoom_in_flow(const typename Pix<T>::v2 *__restrict__ U, typename Pix<T>::v2 *__restrict__ Uout,
                               int nx, int ny, int nxx, int nyy, double fx, double fy, double scale)
{
    const int j1 = blockIdx.x * BX + threadIdx.x;
    const int i1 = blockIdx.y * BY + threadIdx.y;
    if (j1 >= nxx || i1 >= nyy) return;
    U += (size_t) blockIdx.z * nx * ny;                          // pair of a lockstep group
    Uout += (size_t) blockIdx.z * nxx * nyy;
    const double i2 = i1 / fy, j2 = j1 / fx;
    const BicubicTaps t = bicubic_taps(j2, i2, nx, ny);
    double c1[4], c2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double2 v0 = ldw2(U + (size_t) t.row[0] * nx + t.col[k]);
        const double2 v1 = ldw2(U + (size_t) t.row[1] * nx + t.col[k]);
        const double2 v2 = ldw2(U + (size_t) t.row[2] * nx + t.col[k]);
        const double2 v3 = ldw2(U + (size_t) t.row[3] * nx + t.col[k]);
        c1[k] = cubic_cell(v0.x, v1.x, v2.x, v3.x, t.fy);
        c2[k] = cubic_cell(v0.y, v1.y, v2.y, v3.y, t.fy);
    }
    double2 r;
    // In float storage the reference-equivalent value would be rounded to T between zoom_in and the
    // `*= 1/zfactor` loop; in double storage both are exact IEEE steps, so one fused store is identical.
    r.x = cubic_cell(c1[0], c1[1], c1[2], c1[3], t.fx) * scale;
    r.y = cubic_cell(c2[0], c2[1], c2[2], c2[3], t.fx) * scale;
    stn2(Uout + (size_t) i1 * nxx + j1, r);
}

// zoom_in of the G planes of each of three arrays in one launch (blockIdx.z = array x plane), the first two arrays -- a flow --
// multiplied by `scale` afterwards: per plane resample_px, then the product the separate `*= scale` pass would store
template <typename T> struct OfxPlanes3 {
    T *p[3];
};
template <typename T>
__global__ void k_zoom_in_planes3(OfxPlanes3<const T> in, OfxPlanes3<T> out, int G, int nx, int ny, int nxx, int nyy, double fx,
                                  double fy, double scale)
{
    const int j1 = blockIdx.x * BX + threadIdx.x;
    const int i1 = blockIdx.y * BY + threadIdx.y;
    if (j1 >= nxx || i1 >= nyy) return;
    const int a = blockIdx.z / G, g = blockIdx.z - a * G;
    const T *__restrict__ src = in.p[a] + (size_t) g * nx * ny;
    T *__restrict__ dst = out.p[a] + (size_t) g * nxx * nyy;
    const double i2 = i1 / fy, j2 = j1 / fx;
    const BicubicTaps t = bicubic_taps(j2, i2, nx, ny);
    double v = bicubic_sample(src, t, nx);
    if (sizeof(T) == sizeof(float)) v = (double) (float) v;         // the value the resample pass stores
    if (a < 2) v *= scale;
    stn(dst + (size_t) i1 * nxx + j1, v);
}

template <typename T>
int op_resample(ofx_ctx *ctx, const T *in, T *out, int nx, int ny, int nxx, int nyy, double fx, double fy)
{
    hipLaunchKernelGGL(k_resample_g<T>, grid2d(nxx, nyy), block2d(), 0, ctx->stream, OfxPlanes2<const T>{in, nullptr, 1, 0},
                       OfxPlanes2<T>{out, nullptr, 1, 0}, nx, ny, nxx, nyy, fx, fy);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

template <typename T>
int op_zoom_in_flow(ofx_ctx *ctx, const typename Pix<T>::v2 *U, typename Pix<T>::v2 *Uout, int nx, int ny,
                    int nxx, int nyy, double scale, int G)
{
    const double fx = ((double) nxx / nx), fy = ((double) nyy / ny);     // zoom.cpp:141-142
    dim3 g = grid2d(nxx, nyy);
    g.z = G;
    hipLaunchKernelGGL(k_zoom_in_flow<T>, g, block2d(), 0, ctx->stream, U, Uout, nx, ny, nxx, nyy, fx, fy, scale);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

template <typename T>
int op_zoom_in_planes3(ofx_ctx *ctx, int G, const T *u1, const T *u2, const T *c, T *u1o, T *u2o, T *co, int nx, int ny, int nxx,
                       int nyy, double scale)
{
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_in: group of %d", G);
    const double fx = ((double) nxx / nx), fy = ((double) nyy / ny);     // zoom.cpp:141-142
    dim3 g = grid2d(nxx, nyy);
    g.z = 3 * G;
    hipLaunchKernelGGL(k_zoom_in_planes3<T>, g, block2d(), 0, ctx->stream, OfxPlanes3<const T>{{u1, u2, c}}, OfxPlanes3<T>{{u1o, u2o, co}},
                       G, nx, ny, nxx, nyy, fx, fy, scale);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

// ---- zoom_out (src/zoom.cpp:41-78), of nz interleaved channels (IPOL original of robust_expo_methods, zoom.h:45-85 with
// gaussian.h:23-168) ----
// Channel k of the result is zoom_out of channel k: per pixel the sums and the cubics of gauss_pass_px / bicubic_sample in the
// same order, on the interleaved image itself; with nz = 1 the row pass is gauss_pass_px<T, true>'s reflecting branch and the
// sample stage resample_px, term for term.
// Row pass: a row is nx * nz contiguous elements, one lane per ELEMENT (a wave loads 64 consecutive elements per tap); the
// taps are nz elements apart and the reflection is taken on the pixel index.  The column pass is k_gauss_pass_g<T, false> on an
// image of nx * nz columns: the channels of a column are independent columns there.
template <typename T>
OFX_DEV void gauss_row_ch_px(const T *__restrict__ in, T *__restrict__ out, int nx, int ny, int nz, const GaussTaps &taps)
{
    const int e = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (e >= nx * nz || i >= ny) return;
    const int j = e / nz, k = e - j * nz;
    const T *row = in + (size_t) i * nx * nz + k;
    double sum = taps.B[0] * ldw(row + (size_t) j * nz);
    for (int t = 1; t < taps.size; t++)
        sum += taps.B[t] * (ldw(row + (size_t) gauss_reflect(j - t, nx) * nz) + ldw(row + (size_t) gauss_reflect(j + t, nx) * nz));
    stn(out + (size_t) i * nx * nz + e, sum);
}
template <typename T>
__global__ void k_gauss_row_ch_g(OfxPlanes2<const T> in, OfxPlanes2<T> out, int nx, int ny, int nz, GaussTaps taps)
{
    gauss_row_ch_px<T>(in.at(blockIdx.z), out.at(blockIdx.z), nx, ny, nz, taps);
}

// Sample stage: the 16 tap indices of an output pixel once, then one bicubic per channel from them
template <typename T>
OFX_DEV void resample_ch_px(const T *__restrict__ in, T *__restrict__ out, int nx, int ny, int nz, int nxx, int nyy, double factor)
{
    const int j1 = blockIdx.x * BX + threadIdx.x;
    const int i1 = blockIdx.y * BY + threadIdx.y;
    if (j1 >= nxx || i1 >= nyy) return;
    const double i2 = i1 / factor, j2 = j1 / factor;
    const BicubicTaps t = bicubic_taps(j2, i2, nx, ny);
    size_t tap[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = 0; q < 4; q++) tap[r][q] = ((size_t) t.row[r] * nx + t.col[q]) * nz;
    T *o = out + ((size_t) i1 * nxx + j1) * nz;
    for (int k = 0; k < nz; k++) {
        double c[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
            c[q] = cubic_cell(ldw(in + tap[0][q] + k), ldw(in + tap[1][q] + k), ldw(in + tap[2][q] + k), ldw(in + tap[3][q] + k), t.fy);
        stn(o + k, cubic_cell(c[0], c[1], c[2], c[3], t.fx));
    }
}
template <typename T>
__global__ void k_resample_ch_g(OfxPlanes2<const T> in, OfxPlanes2<T> out, int nx, int ny, int nz, int nxx, int nyy, double factor)
{
    resample_ch_px<T>(in.at(blockIdx.z), out.at(blockIdx.z), nx, ny, nz, nxx, nyy, factor);
}

// `count` images, one launch per stage (blockIdx.z = image; the counterpart of op_build_pyramid_group for interleaved
// channels): images 0 .. split - 1 lie back to back at A, the others at B, nx * ny * nz elements each, the zoomed ones
// likewise at oA / oB; tmpA, tmpB are scratch for count images of nx * ny * nz.
template <typename T>
int op_zoom_out_channels_planes(ofx_ctx *ctx, int count, int split, const T *A, const T *B, T *oA, T *oB, T *tmpA, T *tmpB, int nx,
                                int ny, int nz, double factor)
{
    int nxx, nyy;
    ofx_zoom_size(nx, ny, &nxx, &nyy, factor);
    const double sigma = 0.6 * sqrt(1.0 / (factor * factor) - 1.0);      // ZOOM_SIGMA_ZERO, zoom.h:21,66
    GaussTaps taps;
    if (count < 1 || count > OFX_MAX_PLANES || split < 1 || split > count)
        return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out_channels: %d images (%d first)", count, split);
    if (nz < 1 || (long long) nx * ny * nz > 0x7fffffffLL) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out_channels: %dx%dx%d", nx, ny, nz);
    OFX_TRY(gauss_taps_checked(ctx, sigma, nx, ny, 0, &taps));
    const size_t st = (size_t) nx * ny * nz, sto = (size_t) nxx * nyy * nz;
    dim3 g = grid2d(nx * nz, ny);
    g.z = count;
    hipLaunchKernelGGL(k_gauss_row_ch_g<T>, g, block2d(), 0, ctx->stream, OfxPlanes2<const T>{A, B, split, st},
                       OfxPlanes2<T>{tmpA, tmpA + (size_t) split * st, split, st}, nx, ny, nz, taps);
    OFX_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL((k_gauss_pass_g<T, false>), g, block2d(), 0, ctx->stream, OfxPlanes2<const T>{tmpA, tmpA + (size_t) split * st, split, st},
                       OfxPlanes2<T>{tmpB, tmpB + (size_t) split * st, split, st}, nx * nz, ny, taps);
    OFX_LAUNCH_CHECK(ctx);
    g = grid2d(nxx, nyy);
    g.z = count;
    hipLaunchKernelGGL(k_resample_ch_g<T>, g, block2d(), 0, ctx->stream, OfxPlanes2<const T>{tmpB, tmpB + (size_t) split * st, split, st},
                       OfxPlanes2<T>{oA, oB, split, sto}, nx, ny, nz, nxx, nyy, factor);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
// the 2 G images of a lockstep group of pairs: A / B = the G first / second images
template <typename T>
int op_zoom_out_channels_group(ofx_ctx *ctx, int G, const T *A, const T *B, T *oA, T *oB, T *tmpA, T *tmpB, int nx, int ny, int nz,
                               double factor)
{
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out_channels: group of %d", G);
    return op_zoom_out_channels_planes<T>(ctx, 2 * G, G, A, B, oA, oB, tmpA, tmpB, nx, ny, nz, factor);
}

// ---- planar stencil operators (operator-level API) --------------------------------------------------
template <typename T>
__global__ void k_divergence(const T *__restrict__ v1, const T *__restrict__ v2, T *__restrict__ div, int nx, int ny)
{
    const int j = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t p = (size_t) i * nx + j;
    const double ac = ldw(v1 + p), bc = ldw(v2 + p);
    const double al = j > 0 ? ldw(v1 + p - 1) : 0.0;
    const double bu = i > 0 ? ldw(v2 + p - nx) : 0.0;
    stn(div + p, div_backward(ac, al, bc, bu, j == 0, j == nx - 1, i == 0, i == ny - 1));
}

// src/operators.cpp:86-125
template <typename T>
__global__ void k_forward_gradient(const T *__restrict__ f, T *__restrict__ fx, T *__restrict__ fy, int nx, int ny)
{
    const int j = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t p = (size_t) i * nx + j;
    const double c = ldw(f + p);
    stn(fx + p, j < nx - 1 ? ldw(f + p + 1) - c : 0.0);
    stn(fy + p, i < ny - 1 ? ldw(f + p + nx) - c : 0.0);
}

// src/operators.cpp:335-406 (nz = 1): the missing neighbour at a border is the pixel itself, factor 1/2 kept
template <typename T>
OFX_DEV void centered_gradient_px(const T *__restrict__ f, T *__restrict__ dx, T *__restrict__ dy, int nx, int ny)
{
    const int j = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
    const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
    const size_t p = (size_t) i * nx + j;
    stn(dx + p, 0.5 * (ldw(f + (size_t) i * nx + jr) - ldw(f + (size_t) i * nx + jl)));
    stn(dy + p, 0.5 * (ldw(f + (size_t) id * nx + j) - ldw(f + (size_t) iu * nx + j)));
}
// planes back to back in all three arrays (blockIdx.z = plane)
template <typename T>
__global__ void k_centered_gradient_g(const T *__restrict__ f, T *__restrict__ dx, T *__restrict__ dy, int nx, int ny)
{
    const size_t o = (size_t) blockIdx.z * nx * ny;
    centered_gradient_px<T>(f + o, dx + o, dy + o, nx, ny);
}

// Dxx / Dyy / Dxy = mask3x3 (src/operators.cpp:132-328) specialised to the three fixed masks.  Taps
// that fall outside fold onto the edge sample and their weights are summed before the multiply, so
// e.g. Dxx at j=0 is in[0]*(1-2) + in[1]; zero-weight taps add +-0 and drop out.
template <typename T>
__global__ void k_second_derivative(const T *__restrict__ f, T *__restrict__ out, int nx, int ny, int which)
{
    const int j = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t p = (size_t) i * nx + j;
    double r;
    if (which == 0) {                       // Dxx: 1 -2 1 along x
        if (j == 0)            r = ldw(f + p) * -1.0 + ldw(f + p + 1);
        else if (j == nx - 1)  r = ldw(f + p - 1) + ldw(f + p) * -1.0;
        else                   r = ldw(f + p - 1) + ldw(f + p) * -2.0 + ldw(f + p + 1);
    } else if (which == 1) {                // Dyy: 1 -2 1 along y
        if (i == 0)            r = ldw(f + p) * -1.0 + ldw(f + p + nx);
        else if (i == ny - 1)  r = ldw(f + p - nx) + ldw(f + p) * -1.0;
        else                   r = ldw(f + p - nx) + ldw(f + p) * -2.0 + ldw(f + p + nx);
    } else {                                // Dxy: +-1/4 on the four diagonal neighbours (clamped)
        const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
        const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
        r = ldw(f + (size_t) iu * nx + jl) * 0.25 + ldw(f + (size_t) iu * nx + jr) * -0.25 +
            ldw(f + (size_t) id * nx + jl) * -0.25 + ldw(f + (size_t) id * nx + jr) * 0.25;
    }
    stn(out + p, r);
}

// src/bicubic_interpolation.cpp:352-374
template <typename T>
__global__ void k_bicubic_warp(const T *__restrict__ in, const T *__restrict__ u, const T *__restrict__ v,
                               T *__restrict__ out, int nx, int ny, int border_out)
{
    const int j = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t p = (size_t) i * nx + j;
    const double uu = j + ldw(u + p), vv = i + ldw(v + p);
    const BicubicTaps t = bicubic_taps(uu, vv, nx, ny);
    stn(out + p, (t.out && border_out) ? 0.0 : bicubic_sample(in, t, nx));
}

template <typename T>
__global__ void k_bicubic_at(const T *__restrict__ in, const double *__restrict__ uu, const double *__restrict__ vv,
                             double *__restrict__ out, int n, int nx, int ny, int border_out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const BicubicTaps t = bicubic_taps(uu[k], vv[k], nx, ny);
    out[k] = (t.out && border_out) ? 0.0 : bicubic_sample(in, t, nx);
}

// bicubic_interpolation_at_color (src/bicubic_interpolation.cpp:253-344): channel k of an image with nz interleaved
// channels, same tap rule as the scalar version
template <typename T>
__global__ void k_bicubic_at_color(const T *__restrict__ in, const double *__restrict__ uu, const double *__restrict__ vv,
                                   double *__restrict__ out, int n, int nx, int ny, int nz, int ch, int border_out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const BicubicTaps t = bicubic_taps(uu[k], vv[k], nx, ny);
    double r = 0.0;
    if (!(t.out && border_out)) {
        double c[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double v0 = ldw(in + ((size_t) t.row[0] * nx + t.col[q]) * nz + ch);
            const double v1 = ldw(in + ((size_t) t.row[1] * nx + t.col[q]) * nz + ch);
            const double v2 = ldw(in + ((size_t) t.row[2] * nx + t.col[q]) * nz + ch);
            const double v3 = ldw(in + ((size_t) t.row[3] * nx + t.col[q]) * nz + ch);
            c[q] = cubic_cell(v0, v1, v2, v3, t.fy);
        }
        r = cubic_cell(c[0], c[1], c[2], c[3], t.fx);
    }
    out[k] = r;
}

// the temporal part of centered_gradient3 (src/operators.cpp:477-498): centred difference between frames,
// one-sided (still x 0.5) in the first / last frame, 0 for a single frame
template <typename T>
__global__ void k_gradient_dz(const T *__restrict__ in, T *__restrict__ dz, size_t df, int nz)
{
    const size_t p = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    if (p >= df) return;
    const size_t k = (size_t) f * df + p;
    double r = 0.0;
    if (nz > 1) {
        const double hi = ldw(in + (f < nz - 1 ? k + df : k)), lo = ldw(in + (f > 0 ? k - df : k));
        r = 0.5 * (hi - lo);
    }
    stn(dz + k, r);
}

template <typename T> int op_divergence(ofx_ctx *ctx, const T *v1, const T *v2, T *div, int nx, int ny)
{
    hipLaunchKernelGGL(k_divergence<T>, grid2d(nx, ny), block2d(), 0, ctx->stream, v1, v2, div, nx, ny);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T> int op_forward_gradient(ofx_ctx *ctx, const T *f, T *fx, T *fy, int nx, int ny)
{
    hipLaunchKernelGGL(k_forward_gradient<T>, grid2d(nx, ny), block2d(), 0, ctx->stream, f, fx, fy, nx, ny);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T> int op_centered_gradient(ofx_ctx *ctx, const T *f, T *dx, T *dy, int nx, int ny)
{
    return op_centered_gradient_planes<T>(ctx, 1, f, dx, dy, nx, ny);
}
template <typename T> int op_centered_gradient_planes(ofx_ctx *ctx, int count, const T *f, T *dx, T *dy, int nx, int ny)
{
    if (count < 1 || count > 65535) return ofx_fail(ctx, OFX_ERR_ARG, "centered_gradient: %d planes", count);     // gridDim.z
    dim3 g = grid2d(nx, ny);
    g.z = count;
    hipLaunchKernelGGL(k_centered_gradient_g<T>, g, block2d(), 0, ctx->stream, f, dx, dy, nx, ny);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T> int op_second_derivative(ofx_ctx *ctx, const T *f, T *out, int nx, int ny, int which)
{
    hipLaunchKernelGGL(k_second_derivative<T>, grid2d(nx, ny), block2d(), 0, ctx->stream, f, out, nx, ny, which);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T>
int op_bicubic_warp(ofx_ctx *ctx, const T *in, const T *u, const T *v, T *out, int nx, int ny, int border_out)
{
    hipLaunchKernelGGL(k_bicubic_warp<T>, grid2d(nx, ny), block2d(), 0, ctx->stream, in, u, v, out, nx, ny, border_out);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}
template <typename T>
int op_bicubic_at(ofx_ctx *ctx, const T *in, const double *uu, const double *vv, double *out, int n, int nx,
                  int ny, int border_out)
{
    hipLaunchKernelGGL(k_bicubic_at<T>, dim3(grid1d((size_t) n)), dim3(256), 0, ctx->stream, in, uu, vv, out, n, nx,
                       ny, border_out);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

// centred gradient next to the image (src/operators.cpp:335-406, nz = 1): pa = (f, fx), pb = fy
template <typename T>
__global__ void k_grad_pack(const T *__restrict__ f, typename Pix<T>::v2 *__restrict__ pa, T *__restrict__ pb, int nx,
                            int ny)
{
    const int j = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t zoff = (size_t) blockIdx.z * nx * ny;      // plane of a lockstep group
    f += zoff;
    pa += zoff;
    pb += zoff;
    const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
    const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
    const size_t p = (size_t) i * nx + j;
    const double fx = 0.5 * (ldw(f + (size_t) i * nx + jr) - ldw(f + (size_t) i * nx + jl));
    const double fy = 0.5 * (ldw(f + (size_t) id * nx + j) - ldw(f + (size_t) iu * nx + j));
    stn2(pa + p, make_double2(ldw(f + p), fx));
    stn(pb + p, fy);
}

// G planes back to back (blockIdx.z = plane)
template <typename T> int op_grad_pack(ofx_ctx *ctx, const T *f, typename Pix<T>::v2 *pa, T *pb, int nx, int ny, int G)
{
    dim3 g = grid2d(nx, ny);
    g.z = G;
    hipLaunchKernelGGL(k_grad_pack<T>, g, block2d(), 0, ctx->stream, f, pa, pb, nx, ny);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

int op_pyramid_sizes(ofx_ctx *ctx, int nxx, int nyy, int nscales, double zfactor, std::vector<int> &nxs, std::vector<int> &nys)
{
    // no fixed limit on the number of levels (the reference allocates its pyramid dynamically; tvl1flow with
    // zfactor = 0.9 at 1080p uses 47): OFX_MAX_SCALES only bounds what ofx_stats RECORDS.  1024 is a sanity bound.
    if (nscales < 1 || nscales > 1024) return ofx_fail(ctx, OFX_ERR_ARG, "nscales=%d", nscales);
    nxs.assign(nscales, 0);
    nys.assign(nscales, 0);
    if (nxx < 2 || nyy < 2) return ofx_fail(ctx, OFX_ERR_ARG, "image %dx%d too small", nxx, nyy);
    if (!(zfactor > 0.0) || !(zfactor < 1.0)) return ofx_fail(ctx, OFX_ERR_ARG, "zoom factor %g", zfactor);
    int nx = nxx, ny = nyy;
    for (int s = 0; s < nscales; s++) {
        if (s) ofx_zoom_size(nxs[s - 1], nys[s - 1], &nx, &ny, zfactor);
        if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_SIGMA, "scale %d would be %dx%d", s, nx, ny);
        nxs[s] = nx;
        nys[s] = ny;
    }
    return OFX_OK;
}

// The pyramid prologue for the G pairs of a lockstep group with ONE launch per step for all 2 G images (per pair it would be
// 39 launches, most of them tiny): lvA[s] / lvB[s] = level arrays holding the G images back to back, tmpA / tmpB = scratch
// for 2 G full-size images each, scr = G * op_pyramid_scratch_doubles() doubles.  Per pixel image_normalization_2, gaussian
// and zoom_out; zoom_out's scratch copy (zoom.cpp:54-57) is not made -- the first Gaussian pass reads the level itself.
template <typename T>
int op_build_pyramid_group(ofx_ctx *ctx, int G, const void *const *dA, const void *const *dB, int nscales, double zfactor,
                           double sigma, const int *nxs, const int *nys, T *const *lvA, T *const *lvB, T *tmpA, T *tmpB,
                           double *scr, int kind, size_t pitch)
{
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "pyramid group of %d", G);
    const int nxx = nxs[0], nyy = nys[0], size = nxx * nyy;
    // fused row + column pass (k_gauss_xy_g) when the radius allows: it cannot work in place, so the normalised images go to
    // the scratch array and the presmoothing writes the level
    GaussTaps t0;
    const double zsigma = 0.6 * sqrt(1.0 / (zfactor * zfactor) - 1.0);          // ZOOM_SIGMA_ZERO, zoom.cpp:15,60
    bool fused = ctx->gauss_fused != 0 && ofx_gauss_taps(sigma, &t0) == OFX_OK && t0.size - 1 <= GXY_RMAX;
    if (fused && nscales > 1) fused = ofx_gauss_taps(zsigma, &t0) == OFX_OK && t0.size - 1 <= GXY_RMAX;
    T *n0 = fused ? tmpA : lvA[0], *n1 = fused ? tmpA + (size_t) G * size : lvB[0];
    OfxSrcPtrs src = {};
    OfxDstPtrs dst = {};
    for (int g = 0; g < G; g++) {                                               // set g = pair g
        src.p[2 * g] = dA[g];
        src.p[2 * g + 1] = dB[g];
        dst.p[2 * g] = n0 + (size_t) g * size;
        dst.p[2 * g + 1] = n1 + (size_t) g * size;
    }
    if (kind < 0) OFX_TRY((op_normalize_sets<T, T>(ctx, src, dst, G, 2, (size_t) size, 1, scr)));
    else OFX_TRY(op_normalize_sets_in<T>(ctx, kind, src, dst, G, 2, nxx, nyy, pitch, 1, scr));
    auto gauss_xy = [&](const T *ia, const T *ib, T *oa, T *ob, int nx, int ny, double sg) -> int {
        GaussTaps taps;
        OFX_TRY(gauss_taps_checked(ctx, sg, nx, ny, 0, &taps));
        const size_t st = (size_t) nx * ny;
        if (ctx->gauss_fused == 2)                         // the generic-radius kernel (A/B and tests)
            hipLaunchKernelGGL(k_gauss_xy_g<T>, dim3(ofx_cdiv(nx, 64), ofx_cdiv(ny, GXY_TH), 2 * G), dim3(64, 4), 0, ctx->stream,
                               OfxPlanes2<const T>{ia, ib, G, st}, OfxPlanes2<T>{oa, ob, G, st}, nx, ny, taps);
        else
            gauss_xy_launch<T>(ctx, dim3(ofx_cdiv(nx, 64), ofx_cdiv(ny, GXY_TH), 2 * G), OfxPlanes2<const T>{ia, ib, G, st},
                               OfxPlanes2<T>{oa, ob, G, st}, nx, ny, taps);
        OFX_LAUNCH_CHECK(ctx);
        return OFX_OK;
    };
    if (fused) {
        OFX_TRY(gauss_xy(n0, n1, lvA[0], lvB[0], nxx, nyy, sigma));
        for (int s = 1; s < nscales; s++) {
            const int nx = nxs[s - 1], ny = nys[s - 1];
            const size_t st = (size_t) nx * ny;
            GaussTaps tz;
            if (ctx->gauss_fused == 1 && zfactor == 0.5 && ofx_gauss_taps(zsigma, &tz) == OFX_OK && tz.size - 1 == 5 && tz.size < nx &&
                tz.size < ny && 2 * (nxs[s] - 1) <= nx - 1 && 2 * (nys[s] - 1) <= ny - 1) {
                // smoothing and the 2:1 sampling in one launch (k_gauss_xy_dec)
                hipLaunchKernelGGL((k_gauss_xy_dec<T, 5>), dim3(ofx_cdiv(nxs[s], 64), ofx_cdiv(nys[s], GXD_THO), 2 * G), dim3(64, 4), 0,
                                   ctx->stream, OfxPlanes2<const T>{lvA[s - 1], lvB[s - 1], G, st},
                                   OfxPlanes2<T>{lvA[s], lvB[s], G, (size_t) nxs[s] * nys[s]}, nx, ny, nxs[s], nys[s], tz);
                OFX_LAUNCH_CHECK(ctx);
                continue;
            }
            OFX_TRY(gauss_xy(lvA[s - 1], lvB[s - 1], tmpB, tmpB + (size_t) G * st, nx, ny, zsigma));
            dim3 g = grid2d(nxs[s], nys[s]);
            g.z = 2 * G;
            hipLaunchKernelGGL(k_resample_g<T>, g, block2d(), 0, ctx->stream, OfxPlanes2<const T>{tmpB, tmpB + (size_t) G * st, G, st},
                               OfxPlanes2<T>{lvA[s], lvB[s], G, (size_t) nxs[s] * nys[s]}, nx, ny, nxs[s], nys[s], zfactor, zfactor);
            OFX_LAUNCH_CHECK(ctx);
        }
        return OFX_OK;
    }
    auto gauss = [&](const T *ia, const T *ib, T *oa, T *ob, T *ta, T *tb, int nx, int ny, double sg) -> int {
        GaussTaps taps;
        OFX_TRY(gauss_taps_checked(ctx, sg, nx, ny, 0, &taps));
        const size_t st = (size_t) nx * ny;
        dim3 g = grid2d(nx, ny);
        g.z = 2 * G;
        hipLaunchKernelGGL((k_gauss_pass_g<T, true>), g, block2d(), 0, ctx->stream, OfxPlanes2<const T>{ia, ib, G, st},
                           OfxPlanes2<T>{ta, tb, G, st}, nx, ny, taps);
        OFX_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL((k_gauss_pass_g<T, false>), g, block2d(), 0, ctx->stream, OfxPlanes2<const T>{ta, tb, G, st},
                           OfxPlanes2<T>{oa, ob, G, st}, nx, ny, taps);
        OFX_LAUNCH_CHECK(ctx);
        return OFX_OK;
    };
    // scratch: first half = the A images of the group, second half = the B images
    OFX_TRY(gauss(lvA[0], lvB[0], lvA[0], lvB[0], tmpA, tmpA + (size_t) G * size, nxx, nyy, sigma));
    for (int s = 1; s < nscales; s++) {
        const int nx = nxs[s - 1], ny = nys[s - 1];
        const size_t st = (size_t) nx * ny;
        OFX_TRY(gauss(lvA[s - 1], lvB[s - 1], tmpB, tmpB + (size_t) G * st, tmpA, tmpA + (size_t) G * st, nx, ny, zsigma));
        dim3 g = grid2d(nxs[s], nys[s]);
        g.z = 2 * G;
        hipLaunchKernelGGL(k_resample_g<T>, g, block2d(), 0, ctx->stream,
                           OfxPlanes2<const T>{tmpB, tmpB + (size_t) G * st, G, st},
                           OfxPlanes2<T>{lvA[s], lvB[s], G, (size_t) nxs[s] * nys[s]}, nx, ny, nxs[s], nys[s], zfactor, zfactor);
        OFX_LAUNCH_CHECK(ctx);
    }
    return OFX_OK;
}

template <typename T>
int op_bicubic_at_color(ofx_ctx *ctx, const T *in, const double *uu, const double *vv, double *out, int n, int nx, int ny,
                        int nz, int ch, int border_out)
{
    hipLaunchKernelGGL(k_bicubic_at_color<T>, dim3(grid1d((size_t) n)), dim3(256), 0, ctx->stream, in, uu, vv, out, n, nx,
                       ny, nz, ch, border_out);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

template <typename T> int op_gradient_dz(ofx_ctx *ctx, const T *in, T *dz, int nx, int ny, int nz)
{
    const size_t df = (size_t) nx * ny;
    hipLaunchKernelGGL(k_gradient_dz<T>, dim3(grid1d(df), nz), dim3(256), 0, ctx->stream, in, dz, df, nz);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

// ---- the pyramid of a start flow (TV-L1 warm start) --------------------------------------------------
// Not the image pyramid run twice: (u, v) stay interleaved, both components share every tap index, Gaussian weight and bicubic
// coefficient, and a tap is ONE 8-byte (the float payload, level 0) or 16-byte (double2) load.  Per component the sums and their
// order are those of gauss_pass_px / resample_px, i.e. of the reference's zoom_out; the chain is double throughout.
struct OfxFlowPlanes {
    const void *in[OFX_MAX_GROUP];      // the finer level of pair blockIdx.z; NULL: the pair has no start
    void       *out[OFX_MAX_GROUP];     // the level to write; NULL: nothing (a pair without a start above the last level)
};
// a payload component that is not finite (NaN, +-Inf) counts as 0: no input can put a NaN into the warp's coordinates
OFX_DEV float flow_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 0.0f : x; }
OFX_DEV float2 ldflow(const float2 *p) { const float2 v = *p; return make_float2(flow_finite(v.x), flow_finite(v.y)); }
OFX_DEV double2 ldflow(const double2 *p) { return *p; }
OFX_DEV double2 widen2(float2 v) { return make_double2((double) v.x, (double) v.y); }
OFX_DEV double2 widen2(double2 v) { return v; }
OFX_DEV bool is_neg_zero(double x) { return __double_as_longlong(x) == (long long) 0x8000000000000000ull; }

// One value of the separable Gaussian straight from memory (the column pass over row-pass values, operators.cpp:541-611) and
// zoom_out's sample of an output pixel from sixteen of them: the reference's operations one by one, for the pixels that the
// fused kernel below cannot settle.  Slow, and all but never taken.
template <typename IN>
OFX_DEV double2 flow_gauss_row_at(const IN *__restrict__ in, int nx, int i, int j, const GaussTaps &taps)
{
    const IN *row = in + (size_t) i * nx;
    const double2 c = widen2(ldflow(row + j));
    double2 sum = make_double2(taps.B[0] * c.x, taps.B[0] * c.y);
#pragma unroll 1
    for (int k = 1; k < taps.size; k++) {
        const double2 a = widen2(ldflow(row + gauss_reflect(j - k, nx))), b = widen2(ldflow(row + gauss_reflect(j + k, nx)));
        sum.x += taps.B[k] * (a.x + b.x);
        sum.y += taps.B[k] * (a.y + b.y);
    }
    return sum;
}
template <typename IN>
OFX_DEV double2 flow_gauss_at(const IN *__restrict__ in, int nx, int ny, int i, int j, const GaussTaps &taps)
{
    const double2 c = flow_gauss_row_at(in, nx, i, j, taps);
    double2 sum = make_double2(taps.B[0] * c.x, taps.B[0] * c.y);
#pragma unroll 1
    for (int k = 1; k < taps.size; k++) {
        const double2 a = flow_gauss_row_at(in, nx, gauss_reflect(i - k, ny), j, taps);
        const double2 b = flow_gauss_row_at(in, nx, gauss_reflect(i + k, ny), j, taps);
        sum.x += taps.B[k] * (a.x + b.x);
        sum.y += taps.B[k] * (a.y + b.y);
    }
    return sum;
}
template <typename IN>
OFX_DEV double2 flow_zoom_out_at(const IN *__restrict__ in, int nx, int ny, int i1, int j1, double factor, const GaussTaps &taps)
{
    const BicubicTaps t = bicubic_taps(j1 / factor, i1 / factor, nx, ny);
    double2 c[4];
#pragma unroll                                                   // (unrolled: no array is indexed by a variable)
    for (int k = 0; k < 4; k++) {
        double2 v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = flow_gauss_at(in, nx, ny, t.row[q], t.col[k], taps);
        c[k].x = cubic_cell(v[0].x, v[1].x, v[2].x, v[3].x, t.fy);
        c[k].y = cubic_cell(v[0].y, v[1].y, v[2].y, v[3].y, t.fy);
    }
    return make_double2(cubic_cell(c[0].x, c[1].x, c[2].x, c[3].x, t.fx), cubic_cell(c[0].y, c[1].y, c[2].y, c[3].y, t.fx));
}

// zoom_out with zfactor = 1/2 and the `* zfactor` in ONE launch per level for all pairs, in the manner of k_gauss_xy_dec: the
// bicubic sample of the smoothed field at (2 j1, 2 i1) is the smoothed value v itself, v + 0.5 * 0 * (...) in both directions --
// unless v is -0.0, where the sign of the sum depends on the sign of the bracket (an image is >= 0 and never meets this; a flow
// can): such a pixel, a (2 R + 1)^2 window of -0.0 in the finer level, is taken through flow_zoom_out_at.  A block stages
// (2 FPD_THO + 2 R) x (128 + 2 R) taps of the finer level in LDS, as the float payload at level 0.
#define FPD_THO 8
template <typename IN, typename OUT, int R>
__global__ __launch_bounds__(256) void k_flow_pyr_dec(OfxFlowPlanes P, int nx, int ny, int nxo, int nyo, double scale, GaussTaps taps)
{
    constexpr int W = 128 + 2 * R, H = 2 * FPD_THO + 2 * R, SEG = FPD_THO / 4;
    __shared__ IN s_in[H * W];
    __shared__ double2 s_mid[H * 64];
    const IN *__restrict__ in = static_cast<const IN *>(P.in[blockIdx.z]);
    OUT *__restrict__ out = static_cast<OUT *>(P.out[blockIdx.z]);
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int jo = blockIdx.x * 64 + tx;
    if (!in) {                                                   // no start: zeros into the last level (the block's pair is one)
        if (!out || jo >= nxo) return;
        for (int o = 0; o < SEG; o++) {
            const int io = blockIdx.y * FPD_THO + ty * SEG + o;
            if (io < nyo) stn2(out + (size_t) io * nxo + jo, make_double2(0.0, 0.0));
        }
        return;
    }
    const int j0 = blockIdx.x * 128, i0 = blockIdx.y * 2 * FPD_THO;
    int jc[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        int j = gauss_reflect(j0 - R + tx + 64 * q, nx);
        jc[q] = j < 0 ? 0 : (j > nx - 1 ? nx - 1 : j);           // beyond the image on the far side of a border block: never used
    }
    for (int r = ty; r < H; r += 4) {
        int i = gauss_reflect(i0 - R + r, ny);
        i = i < 0 ? 0 : (i > ny - 1 ? ny - 1 : i);
        const IN *__restrict__ row = in + (size_t) i * nx;
        s_in[r * W + tx] = ldflow(row + jc[0]);
        s_in[r * W + tx + 64] = ldflow(row + jc[1]);
        if (tx < 2 * R) s_in[r * W + tx + 128] = ldflow(row + jc[2]);
    }
    __syncthreads();
    for (int r = ty; r < H; r += 4) {                            // row pass at the even columns
        const IN *row = s_in + r * W + R + 2 * tx;
        const double2 c = widen2(row[0]);
        double2 sum = make_double2(taps.B[0] * c.x, taps.B[0] * c.y);
#pragma unroll
        for (int k = 1; k <= R; k++) {
            const double2 a = widen2(row[-k]), b = widen2(row[k]);
            sum.x += taps.B[k] * (a.x + b.x);
            sum.y += taps.B[k] * (a.y + b.y);
        }
        s_mid[r * 64 + tx] = sum;
    }
    __syncthreads();
    if (jo >= nxo) return;
#pragma unroll
    for (int o = 0; o < SEG; o++) {                              // column pass at the even rows, then the scale
        const int lo = ty * SEG + o, io = blockIdx.y * FPD_THO + lo;
        if (io >= nyo) break;
        const double2 *c = s_mid + (R + 2 * lo) * 64 + tx;
        double2 sum = make_double2(taps.B[0] * c[0].x, taps.B[0] * c[0].y);
#pragma unroll
        for (int k = 1; k <= R; k++) {
            const double2 a = c[-k * 64], b = c[k * 64];
            sum.x += taps.B[k] * (a.x + b.x);
            sum.y += taps.B[k] * (a.y + b.y);
        }
        if (is_neg_zero(sum.x) || is_neg_zero(sum.y)) sum = flow_zoom_out_at(in, nx, ny, io, jo, 0.5, taps);
        stn2(out + (size_t) io * nxo + jo, make_double2(sum.x * scale, sum.y * scale));
    }
}

// Any other zfactor: the row and the column pass in one launch through LDS (k_gauss_xy_g on pairs; radius <= FPG_RMAX), the
// smoothed field into scratch, ...
#define FPG_TH 16
#define FPG_RMAX 8
template <typename IN>
__global__ __launch_bounds__(256) void k_flow_gauss_xy(OfxFlowPlanes P, int nx, int ny, GaussTaps taps)
{
    __shared__ IN s_in[(FPG_TH + 2 * FPG_RMAX) * (64 + 2 * FPG_RMAX)];
    __shared__ double2 s_mid[(FPG_TH + 2 * FPG_RMAX) * 64];
    const IN *__restrict__ in = static_cast<const IN *>(P.in[blockIdx.z]);
    double2 *__restrict__ out = static_cast<double2 *>(P.out[blockIdx.z]);
    if (!in || !out) return;
    const int R = taps.size - 1, W = 64 + 2 * R, H = FPG_TH + 2 * R;
    const int j0 = blockIdx.x * 64, i0 = blockIdx.y * FPG_TH;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int k = tid; k < W * H; k += 256) {
        const int r = k / W, c = k - r * W;
        int i = gauss_reflect(i0 - R + r, ny), j = gauss_reflect(j0 - R + c, nx);
        i = i < 0 ? 0 : (i > ny - 1 ? ny - 1 : i);
        j = j < 0 ? 0 : (j > nx - 1 ? nx - 1 : j);
        s_in[r * W + c] = ldflow(in + (size_t) i * nx + j);
    }
    __syncthreads();
    for (int r = threadIdx.y; r < H; r += 4) {
        const IN *row = s_in + r * W + R + threadIdx.x;
        const double2 c = widen2(row[0]);
        double2 sum = make_double2(taps.B[0] * c.x, taps.B[0] * c.y);
        for (int k = 1; k < taps.size; k++) {
            const double2 a = widen2(row[-k]), b = widen2(row[k]);
            sum.x += taps.B[k] * (a.x + b.x);
            sum.y += taps.B[k] * (a.y + b.y);
        }
        s_mid[r * 64 + threadIdx.x] = sum;
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;
    if (j >= nx) return;
    for (int r = threadIdx.y; r < FPG_TH; r += 4) {
        const int i = i0 + r;
        if (i >= ny) break;
        const double2 *col = s_mid + (r + R) * 64 + threadIdx.x;
        double2 sum = make_double2(taps.B[0] * col[0].x, taps.B[0] * col[0].y);
        for (int k = 1; k < taps.size; k++) {
            const double2 a = col[-k * 64], b = col[k * 64];
            sum.x += taps.B[k] * (a.x + b.x);
            sum.y += taps.B[k] * (a.y + b.y);
        }
        out[(size_t) i * nx + j] = sum;
    }
}
// ... or, for a wider radius, one pass per launch (gauss_pass_px on pairs)
template <typename IN, bool ALONG_X>
__global__ void k_flow_gauss_pass(OfxFlowPlanes P, int nx, int ny, GaussTaps taps)
{
    const IN *__restrict__ in = static_cast<const IN *>(P.in[blockIdx.z]);
    double2 *__restrict__ out = static_cast<double2 *>(P.out[blockIdx.z]);
    const int j = blockIdx.x * BX + threadIdx.x;
    const int i = blockIdx.y * BY + threadIdx.y;
    if (!in || !out || j >= nx || i >= ny) return;
    const double2 c = widen2(ldflow(in + (size_t) i * nx + j));
    double2 sum = make_double2(taps.B[0] * c.x, taps.B[0] * c.y);
    for (int k = 1; k < taps.size; k++) {
        const size_t pa = ALONG_X ? (size_t) i * nx + gauss_reflect(j - k, nx) : (size_t) gauss_reflect(i - k, ny) * nx + j;
        const size_t pb = ALONG_X ? (size_t) i * nx + gauss_reflect(j + k, nx) : (size_t) gauss_reflect(i + k, ny) * nx + j;
        const double2 a = widen2(ldflow(in + pa)), b = widen2(ldflow(in + pb));
        sum.x += taps.B[k] * (a.x + b.x);
        sum.y += taps.B[k] * (a.y + b.y);
    }
    out[(size_t) i * nx + j] = sum;
}
// ... and the last pass takes zoom_out's bicubic sample (resample_px on pairs) and the `* zfactor` with it
template <typename OUT>
__global__ void k_flow_resample(OfxFlowPlanes P, int nx, int ny, int nxx, int nyy, double factor, double scale)
{
    const double2 *__restrict__ in = static_cast<const double2 *>(P.in[blockIdx.z]);
    OUT *__restrict__ out = static_cast<OUT *>(P.out[blockIdx.z]);
    const int j1 = blockIdx.x * BX + threadIdx.x;
    const int i1 = blockIdx.y * BY + threadIdx.y;
    if (!out || j1 >= nxx || i1 >= nyy) return;
    double2 r = make_double2(0.0, 0.0);
    if (in) {
        const BicubicTaps t = bicubic_taps(j1 / factor, i1 / factor, nx, ny);
        double2 c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double2 v0 = in[(size_t) t.row[0] * nx + t.col[k]], v1 = in[(size_t) t.row[1] * nx + t.col[k]];
            const double2 v2 = in[(size_t) t.row[2] * nx + t.col[k]], v3 = in[(size_t) t.row[3] * nx + t.col[k]];
            c[k].x = cubic_cell(v0.x, v1.x, v2.x, v3.x, t.fy);
            c[k].y = cubic_cell(v0.y, v1.y, v2.y, v3.y, t.fy);
        }
        r.x = cubic_cell(c[0].x, c[1].x, c[2].x, c[3].x, t.fx) * scale;
        r.y = cubic_cell(c[0].y, c[1].y, c[2].y, c[3].y, t.fx) * scale;
    }
    stn2(out + (size_t) i1 * nxx + j1, r);
}
// one level: W_0 itself (the conversion with the non-finite rule), or zeros for a pair without a start
template <typename OUT>
__global__ void k_flow_convert(OfxFlowPlanes P, size_t n)
{
    const float2 *__restrict__ in = static_cast<const float2 *>(P.in[blockIdx.y]);
    OUT *__restrict__ out = static_cast<OUT *>(P.out[blockIdx.y]);
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (!out || i >= n) return;
    stn2(out + i, in ? widen2(ldflow(in + i)) : make_double2(0.0, 0.0));
}

static double flow_zoom_sigma(double zfactor) { return 0.6 * sqrt(1.0 / (zfactor * zfactor) - 1.0); }    // zoom.cpp:15,60
// level s >= 1 is smoothed from level s - 1 with zoom_out's Gaussian: the refusals of op_build_pyramid_group for those levels
int op_flow_pyramid_check(ofx_ctx *ctx, int nscales, double zfactor, const int *nxs, const int *nys)
{
    for (int s = 1; s < nscales; s++) {
        GaussTaps taps;
        OFX_TRY(gauss_taps_checked(ctx, flow_zoom_sigma(zfactor), nxs[s - 1], nys[s - 1], 0, &taps));
    }
    return OFX_OK;
}
// does level s come from the 2:1 kernel?  (the conditions of k_gauss_xy_dec in op_build_pyramid_group)
static bool flow_level_dec(double zfactor, const GaussTaps &tz, int nx, int ny, int nxo, int nyo)
{
    return zfactor == 0.5 && tz.size - 1 == 5 && tz.size < nx && tz.size < ny && 2 * (nxo - 1) <= nx - 1 && 2 * (nyo - 1) <= ny - 1;
}
double op_flow_pyramid_scratch_bytes(int nscales, double zfactor, const int *nxs, const int *nys)
{
    GaussTaps tz;
    if (nscales < 2 || ofx_gauss_taps(flow_zoom_sigma(zfactor), &tz) != OFX_OK) return 0.0;
    double px = 0.0;
    if (nscales > 2) px += (double) nxs[1] * nys[1];
    if (nscales > 3) px += (double) nxs[2] * nys[2];
    if (!flow_level_dec(zfactor, tz, nxs[0], nys[0], nxs[1], nys[1])) px += (tz.size - 1 > FPG_RMAX ? 2.0 : 1.0) * nxs[0] * nys[0];
    return px * sizeof(double2);
}

template <typename IN, typename O>
static int flow_pyramid_level(ofx_ctx *ctx, int G, const OfxFlowPlanes &P, double2 *smooth, double2 *rows, int nx, int ny, int nxo,
                              int nyo, double zfactor, const GaussTaps &tz)
{
    if (flow_level_dec(zfactor, tz, nx, ny, nxo, nyo)) {
        hipLaunchKernelGGL((k_flow_pyr_dec<IN, O, 5>), dim3(ofx_cdiv(nxo, 64), ofx_cdiv(nyo, FPD_THO), G), dim3(64, 4), 0, ctx->stream, P,
                           nx, ny, nxo, nyo, zfactor, tz);
        OFX_LAUNCH_CHECK(ctx);
        return OFX_OK;
    }
    const size_t n = (size_t) nx * ny;
    OfxFlowPlanes S = {}, Z = {};                               // smoothing into scratch, then the sample
    for (int g = 0; g < G; g++) {
        S.in[g] = P.in[g];
        S.out[g] = P.in[g] ? smooth + (size_t) g * n : nullptr;
        Z.in[g] = S.out[g];
        Z.out[g] = P.out[g];
    }
    if (tz.size - 1 <= FPG_RMAX) {
        hipLaunchKernelGGL(k_flow_gauss_xy<IN>, dim3(ofx_cdiv(nx, 64), ofx_cdiv(ny, FPG_TH), G), dim3(64, 4), 0, ctx->stream, S, nx, ny, tz);
        OFX_LAUNCH_CHECK(ctx);
    } else {
        OfxFlowPlanes X = S, Y = S;
        for (int g = 0; g < G; g++) {
            X.out[g] = P.in[g] ? rows + (size_t) g * n : nullptr;
            Y.in[g] = X.out[g];
        }
        dim3 grid = grid2d(nx, ny);
        grid.z = G;
        hipLaunchKernelGGL((k_flow_gauss_pass<IN, true>), grid, block2d(), 0, ctx->stream, X, nx, ny, tz);
        OFX_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL((k_flow_gauss_pass<double2, false>), grid, block2d(), 0, ctx->stream, Y, nx, ny, tz);
        OFX_LAUNCH_CHECK(ctx);
    }
    dim3 grid = grid2d(nxo, nyo);
    grid.z = G;
    hipLaunchKernelGGL(k_flow_resample<O>, grid, block2d(), 0, ctx->stream, Z, nx, ny, nxo, nyo, zfactor, zfactor);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

template <typename OUT>
int op_flow_pyramid(ofx_ctx *ctx, int G, const void *const *init, int nscales, double zfactor, const int *nxs, const int *nys,
                    void *const *out)
{
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "flow pyramid: group of %d", G);
    OFX_TRY(op_flow_pyramid_check(ctx, nscales, zfactor, nxs, nys));
    bool warm = false;
    for (int g = 0; g < G; g++) warm = warm || init[g];
    OfxFlowPlanes P = {};
    if (nscales == 1 || !warm) {                                // the conversion alone, or nothing but zeros
        const size_t n = (size_t) nxs[nscales - 1] * nys[nscales - 1];
        for (int g = 0; g < G; g++) { P.in[g] = warm ? init[g] : nullptr; P.out[g] = out[g]; }
        hipLaunchKernelGGL(k_flow_convert<OUT>, dim3((unsigned) ((n + 255) / 256), G), dim3(256), 0, ctx->stream, P, n);
        OFX_LAUNCH_CHECK(ctx);
        return OFX_OK;
    }
    GaussTaps tz;
    if (ofx_gauss_taps(flow_zoom_sigma(zfactor), &tz) != OFX_OK) return ofx_fail(ctx, OFX_ERR_ARG, "flow pyramid: zoom factor %g", zfactor);
    double2 *lev[2] = {nullptr, nullptr}, *smooth = nullptr, *rows = nullptr;
    if (nscales > 2) OFX_TRY(ofx_alloc(ctx, (size_t) G * nxs[1] * nys[1], &lev[1]));
    if (nscales > 3) OFX_TRY(ofx_alloc(ctx, (size_t) G * nxs[2] * nys[2], &lev[0]));
    if (!flow_level_dec(zfactor, tz, nxs[0], nys[0], nxs[1], nys[1])) {
        OFX_TRY(ofx_alloc(ctx, (size_t) G * nxs[0] * nys[0], &smooth));
        if (tz.size - 1 > FPG_RMAX) OFX_TRY(ofx_alloc(ctx, (size_t) G * nxs[0] * nys[0], &rows));
    }
    for (int s = 1; s < nscales; s++) {                         // level s from level s - 1, ping-pong in lev[s & 1]
        const bool last = s == nscales - 1;
        const size_t nin = (size_t) nxs[s - 1] * nys[s - 1], nout = (size_t) nxs[s] * nys[s];
        for (int g = 0; g < G; g++) {
            P.in[g] = !init[g] ? nullptr : s == 1 ? init[g] : (const void *) (lev[(s - 1) & 1] + (size_t) g * nin);
            P.out[g] = last ? out[g] : init[g] ? (void *) (lev[s & 1] + (size_t) g * nout) : nullptr;
        }
        int st;
        if (s == 1) st = last ? flow_pyramid_level<float2, OUT>(ctx, G, P, smooth, rows, nxs[0], nys[0], nxs[1], nys[1], zfactor, tz)
                              : flow_pyramid_level<float2, double2>(ctx, G, P, smooth, rows, nxs[0], nys[0], nxs[1], nys[1], zfactor, tz);
        else st = last ? flow_pyramid_level<double2, OUT>(ctx, G, P, smooth, rows, nxs[s - 1], nys[s - 1], nxs[s], nys[s], zfactor, tz)
                       : flow_pyramid_level<double2, double2>(ctx, G, P, smooth, rows, nxs[s - 1], nys[s - 1], nxs[s], nys[s], zfactor, tz);
        OFX_TRY(st);
    }
    return OFX_OK;
}
template int op_flow_pyramid<double2>(ofx_ctx *, int, const void *const *, int, double, const int *, const int *, void *const *);
template int op_flow_pyramid<float2>(ofx_ctx *, int, const void *const *, int, double, const int *, const int *, void *const *);

// ---- explicit instantiations -----------------------------------------------------------------------
#define OFX_INSTANTIATE(T)                                                                                           \
    template int op_convert_in<T>(ofx_ctx *, const double *, T *, size_t);                                            \
    template int op_convert_out<T>(ofx_ctx *, const T *, double *, size_t);                                           \
    template int op_interleave2<T>(ofx_ctx *, const double *, const double *, Pix<T>::v2 *, size_t);                  \
    template int op_deinterleave2<T>(ofx_ctx *, const Pix<T>::v2 *, double *, double *, size_t);                      \
    template int op_to_flo<T>(ofx_ctx *, const Pix<T>::v2 *, float2 *, size_t);                                       \
    template int op_fill2<T>(ofx_ctx *, Pix<T>::v2 *, size_t);                                                        \
    template int op_resample<T>(ofx_ctx *, const T *, T *, int, int, int, int, double, double);                       \
    template int op_zoom_in_flow<T>(ofx_ctx *, const Pix<T>::v2 *, Pix<T>::v2 *, int, int, int, int, double, int);    \
    template int op_gaussian_group<T>(ofx_ctx *, int, T *, T *, size_t, T *, int, int, double, int);                   \
    template int op_gaussian_planes<T>(ofx_ctx *, int, int, T *, T *, size_t, T *, int, int, double, int);             \
    template int op_zoom_out_channels_planes<T>(ofx_ctx *, int, int, const T *, const T *, T *, T *, T *, T *, int, int, int, double); \
    template int op_zoom_in_planes3<T>(ofx_ctx *, int, const T *, const T *, const T *, T *, T *, T *, int, int, int, int, double); \
    template int op_centered_gradient_planes<T>(ofx_ctx *, int, const T *, T *, T *, int, int);                        \
    template int op_zoom_out_channels_group<T>(ofx_ctx *, int, const T *, const T *, T *, T *, T *, T *, int, int, int, double); \
    template int op_divergence<T>(ofx_ctx *, const T *, const T *, T *, int, int);                                    \
    template int op_forward_gradient<T>(ofx_ctx *, const T *, T *, T *, int, int);                                    \
    template int op_centered_gradient<T>(ofx_ctx *, const T *, T *, T *, int, int);                                   \
    template int op_second_derivative<T>(ofx_ctx *, const T *, T *, int, int, int);                                   \
    template int op_bicubic_warp<T>(ofx_ctx *, const T *, const T *, const T *, T *, int, int, int);                  \
    template int op_bicubic_at<T>(ofx_ctx *, const T *, const double *, const double *, double *, int, int, int, int);           \
    template int op_grad_pack<T>(ofx_ctx *, const T *, Pix<T>::v2 *, T *, int, int, int);                                       \
    template int op_build_pyramid_group<T>(ofx_ctx *, int, const void *const *, const void *const *, int, double, double,       \
                                           const int *, const int *, T *const *, T *const *, T *, T *, double *, int, size_t); \
    template int op_bicubic_at_color<T>(ofx_ctx *, const T *, const double *, const double *, double *, int, int, int, int, int, int); \
    template int op_gradient_dz<T>(ofx_ctx *, const T *, T *, int, int, int);                                                   \
    template int op_minmax_partial<T>(ofx_ctx *, const OfxSrcPtrs &, int, int, size_t, int, double *, int, int);             \
    template int op_normalize_map<T, T>(ofx_ctx *, const OfxSrcPtrs &, const OfxDstPtrs &, int, int, size_t, int, const double *, int); \
    template int op_normalize_sets<T, T>(ofx_ctx *, const OfxSrcPtrs &, const OfxDstPtrs &, int, int, size_t, int, double *, int); \
    template int op_normalize_map_in<T>(ofx_ctx *, int, const OfxSrcPtrs &, const OfxDstPtrs &, int, int, int, int, size_t, int, const double *, int); \
    template int op_normalize_sets_in<T>(ofx_ctx *, int, const OfxSrcPtrs &, const OfxDstPtrs &, int, int, int, int, size_t, int, double *, int); \
    template int op_convert_sources_in<T>(ofx_ctx *, int, const OfxSrcPtrs &, const OfxDstPtrs &, int, int, int, size_t);

OFX_INSTANTIATE(double)
OFX_INSTANTIATE(float)
// float storage fed with the doubles of a host image (the robust_expo host path rounds after the normalisation)
template int op_normalize_sets<float, double>(ofx_ctx *, const OfxSrcPtrs &, const OfxDstPtrs &, int, int, size_t, int, double *, int);

// ---- buffers that are not on the context's GPU ----
// Is p device memory of this context's GPU?  Everything else -- another GPU's memory, pinned or pageable host memory -- is
// reached through a staging copy (hipMemcpyDefault resolves the direction; between GPUs it is a peer copy over xGMI).
bool ofx_ptr_is_local(const ofx_ctx *ctx, const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void) hipGetLastError();                              // pageable host memory is unknown to the runtime
        return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == ctx->device;
}
// How a buffer that lives on `mem_device` (-1: host memory) reaches a context on `ctx_device`: 0 = in place, 1 = one
// hipMemcpyDefault (host <-> device, or a peer copy over xGMI), 2 = two copies through a host bounce buffer because the two GPUs
// cannot address each other (hipDeviceCanAccessPeer says no: another IOMMU group, peer access disabled, ...).  Pure decision,
// exported so that the host-logic tests cover it without a GPU.
extern "C" int ofx_staging_route(int ctx_device, int mem_device, int can_access_peer)
{
    if (mem_device == ctx_device) return 0;
    if (mem_device < 0) return 1;
    return can_access_peer ? 1 : 2;
}
// dst <- src (one of them on this context's GPU, the other anywhere), on the context's stream.  A route-2 copy is synchronous
// and leaves a note in ofx_last_error (the call still succeeds).  UNEXECUTED on more than one GPU (no multi-GPU box in any round).
int ofx_copy_staged(ofx_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    const void *other = ofx_ptr_is_local(ctx, dst) ? src : dst;
    int mem_device = -1, can = 1;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, other) == hipSuccess) {
        if (a.type == hipMemoryTypeDevice) mem_device = a.device;
    } else {
        (void) hipGetLastError();
    }
    if (mem_device >= 0 && mem_device != ctx->device && hipDeviceCanAccessPeer(&can, ctx->device, mem_device) != hipSuccess) {
        (void) hipGetLastError();
        can = 0;
    }
    if (ofx_staging_route(ctx->device, mem_device, can) < 2) {
        OFX_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, ctx->stream));
        return OFX_OK;
    }
    void *bounce = nullptr;
    OFX_HIP(ctx, hipHostMalloc(&bounce, bytes, hipHostMallocDefault));
    hipError_t e = hipStreamSynchronize(ctx->stream);                                       // src may be this stream's product
    if (e == hipSuccess) e = hipMemcpy(bounce, src, bytes, hipMemcpyDefault);
    if (e == hipSuccess) e = hipMemcpy(dst, bounce, bytes, hipMemcpyDefault);
    (void) hipHostFree(bounce);
    if (e != hipSuccess) return ofx_fail(ctx, OFX_ERR_HIP, "staging through the host failed: %s", hipGetErrorString(e));
    snprintf(ctx->errmsg, sizeof(ctx->errmsg), "note: GPU %d cannot address GPU %d, buffers were staged through the host", ctx->device,
             mem_device);
    return OFX_OK;
}
