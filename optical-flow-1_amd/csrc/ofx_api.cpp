// ofx_api.cpp -- host-pointer entry points of the operator-level C ABI (include/ofx.h).
// Each call: upload double planes -> (convert to the storage type) -> kernel(s) -> convert back ->
// download.  These exist for drop-in / parity use; the solvers never round-trip through the host.
#include "ofx_ops.h"

#include <vector>

namespace {

template <typename T> struct HostOp {
    ofx_ctx *ctx;
    size_t n;
    std::vector<double *> stage;

    // device image of storage type T filled from a host double plane
    int in(const double *h, T **out, size_t count)
    {
        double *s;
        OFX_TRY(ofx_alloc(ctx, count, &s));
        OFX_TRY(ofx_alloc(ctx, count, out));
        OFX_HIP(ctx, hipMemcpyAsync(s, h, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        return op_convert_in<T>(ctx, s, *out, count);
    }
    int out_alloc(T **out, size_t count) { return ofx_alloc(ctx, count, out); }
    // device image -> host double plane
    int out(const T *d, double *h, size_t count)
    {
        double *s;
        OFX_TRY(ofx_alloc(ctx, count, &s));
        OFX_TRY(op_convert_out<T>(ctx, d, s, count));
        OFX_HIP(ctx, hipMemcpyAsync(h, s, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        return OFX_OK;
    }
    int sync()
    {
        OFX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return OFX_OK;
    }
};

int check_dims(ofx_ctx *ctx, int nx, int ny)
{
    if (nx < 2 || ny < 2 || (long long) nx * ny > 0x7fffffffLL) return ofx_fail(ctx, OFX_ERR_ARG, "bad image size %dx%d", nx, ny);
    return OFX_OK;
}

template <typename T> int divergence_t(ofx_ctx *ctx, const double *v1, const double *v2, double *div, int nx, int ny)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny;
    T *a, *b, *o;
    OFX_TRY(h.in(v1, &a, n));
    OFX_TRY(h.in(v2, &b, n));
    OFX_TRY(h.out_alloc(&o, n));
    OFX_TRY(op_divergence<T>(ctx, a, b, o, nx, ny));
    OFX_TRY(h.out(o, div, n));
    return h.sync();
}

template <typename T>
int gradient_t(ofx_ctx *ctx, const double *f, double *gx, double *gy, int nx, int ny, bool centered)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny;
    T *a, *ox, *oy;
    OFX_TRY(h.in(f, &a, n));
    OFX_TRY(h.out_alloc(&ox, n));
    OFX_TRY(h.out_alloc(&oy, n));
    if (centered) OFX_TRY(op_centered_gradient<T>(ctx, a, ox, oy, nx, ny));
    else OFX_TRY(op_forward_gradient<T>(ctx, a, ox, oy, nx, ny));
    OFX_TRY(h.out(ox, gx, n));
    OFX_TRY(h.out(oy, gy, n));
    return h.sync();
}

template <typename T> int second_t(ofx_ctx *ctx, const double *f, double *out, int nx, int ny, int which)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny;
    T *a, *o;
    OFX_TRY(h.in(f, &a, n));
    OFX_TRY(h.out_alloc(&o, n));
    OFX_TRY(op_second_derivative<T>(ctx, a, o, nx, ny, which));
    OFX_TRY(h.out(o, out, n));
    return h.sync();
}

template <typename T> int gaussian_t(ofx_ctx *ctx, double *I, int nx, int ny, double sigma)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny;
    T *a, *tmp;
    OFX_TRY(h.in(I, &a, n));
    OFX_TRY(h.out_alloc(&tmp, n));
    OFX_TRY(op_gaussian_planes<T>(ctx, 1, 1, a, nullptr, n, tmp, nx, ny, sigma));
    OFX_TRY(h.out(a, I, n));
    return h.sync();
}

template <typename T>
int warp_t(ofx_ctx *ctx, const double *in, const double *u, const double *v, double *out, int nx, int ny, int bo)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny;
    T *a, *du, *dv, *o;
    OFX_TRY(h.in(in, &a, n));
    OFX_TRY(h.in(u, &du, n));
    OFX_TRY(h.in(v, &dv, n));
    OFX_TRY(h.out_alloc(&o, n));
    OFX_TRY(op_bicubic_warp<T>(ctx, a, du, dv, o, nx, ny, bo));
    OFX_TRY(h.out(o, out, n));
    return h.sync();
}

template <typename T>
int at_t(ofx_ctx *ctx, const double *in, const double *uu, const double *vv, double *out, int cnt, int nx, int ny, int bo)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny;
    T *a;
    double *du, *dv, *o;
    OFX_TRY(h.in(in, &a, n));
    OFX_TRY(ofx_alloc(ctx, (size_t) cnt, &du));
    OFX_TRY(ofx_alloc(ctx, (size_t) cnt, &dv));
    OFX_TRY(ofx_alloc(ctx, (size_t) cnt, &o));
    OFX_HIP(ctx, hipMemcpyAsync(du, uu, cnt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    OFX_HIP(ctx, hipMemcpyAsync(dv, vv, cnt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    OFX_TRY(op_bicubic_at<T>(ctx, a, du, dv, o, cnt, nx, ny, bo));
    OFX_HIP(ctx, hipMemcpyAsync(out, o, cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return h.sync();
}

template <typename T> int zoom_out_t(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, double factor)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny;
    int nxx, nyy;
    ofx_zoom_size(nx, ny, &nxx, &nyy, factor);
    if (nxx < 1 || nyy < 1) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out: empty output");
    T *a, *o, *t1, *t2;
    OFX_TRY(h.in(I, &a, n));
    OFX_TRY(h.out_alloc(&o, (size_t) nxx * nyy));
    OFX_TRY(h.out_alloc(&t1, n));
    OFX_TRY(h.out_alloc(&t2, n));
    OFX_TRY(op_zoom_out_channels_planes<T>(ctx, 1, 1, a, nullptr, o, nullptr, t1, t2, nx, ny, 1, factor));
    OFX_TRY(h.out(o, Iout, (size_t) nxx * nyy));
    return h.sync();
}

template <typename T> int zoom_out_channels_t(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, int nz, double factor)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny * nz;
    int nxx, nyy;
    ofx_zoom_size(nx, ny, &nxx, &nyy, factor);
    if (nxx < 1 || nyy < 1) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out_channels: empty output");
    GaussTaps taps;                                              // this entry names the factor, not zoom_out's sigma
    if (ofx_gauss_taps(0.6 * sqrt(1.0 / (factor * factor) - 1.0), &taps) != OFX_OK)
        return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out_channels: factor %g needs more than %d taps", factor, OFX_GAUSS_MAX_TAPS);
    T *a, *o, *t1, *t2;
    OFX_TRY(h.in(I, &a, n));
    OFX_TRY(h.out_alloc(&o, (size_t) nxx * nyy * nz));
    OFX_TRY(h.out_alloc(&t1, n));
    OFX_TRY(h.out_alloc(&t2, n));
    OFX_TRY(op_zoom_out_channels_planes<T>(ctx, 1, 1, a, nullptr, o, nullptr, t1, t2, nx, ny, nz, factor));
    OFX_TRY(h.out(o, Iout, (size_t) nxx * nyy * nz));
    return h.sync();
}

template <typename T> int zoom_in_t(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, int nxx, int nyy)
{
    HostOp<T> h{ctx};
    T *a, *o;
    OFX_TRY(h.in(I, &a, (size_t) nx * ny));
    OFX_TRY(h.out_alloc(&o, (size_t) nxx * nyy));
    OFX_TRY(op_resample<T>(ctx, a, o, nx, ny, nxx, nyy, ((double) nxx / nx), ((double) nyy / ny)));
    OFX_TRY(h.out(o, Iout, (size_t) nxx * nyy));
    return h.sync();
}

template <typename T> int norm_t(ofx_ctx *ctx, const double *I1, const double *I2, double *o1, double *o2, int size)
{
    HostOp<T> h{ctx};
    T *a, *b, *x, *y;
    double *scr;
    OFX_TRY(h.in(I1, &a, (size_t) size));
    OFX_TRY(h.in(I2, &b, (size_t) size));
    OFX_TRY(h.out_alloc(&x, (size_t) size));
    OFX_TRY(h.out_alloc(&y, (size_t) size));
    OFX_TRY(ofx_alloc(ctx, op_minmax_scratch_doubles(1, (size_t) size, 1), &scr));
    OFX_TRY((op_normalize_sets<T, T>(ctx, OfxSrcPtrs{{a, b}}, OfxDstPtrs{{x, y}}, 1, 2, (size_t) size, 1, scr)));
    OFX_TRY(h.out(x, o1, (size_t) size));
    OFX_TRY(h.out(y, o2, (size_t) size));
    return h.sync();
}

template <typename T>
int at_color_t(ofx_ctx *ctx, const double *in, const double *uu, const double *vv, double *out, int cnt, int nx, int ny,
               int nz, int ch, int bo)
{
    HostOp<T> h{ctx};
    const size_t n = (size_t) nx * ny * nz;
    T *a;
    double *du, *dv, *o;
    OFX_TRY(h.in(in, &a, n));
    OFX_TRY(ofx_alloc(ctx, (size_t) cnt, &du));
    OFX_TRY(ofx_alloc(ctx, (size_t) cnt, &dv));
    OFX_TRY(ofx_alloc(ctx, (size_t) cnt, &o));
    OFX_HIP(ctx, hipMemcpyAsync(du, uu, cnt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    OFX_HIP(ctx, hipMemcpyAsync(dv, vv, cnt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    OFX_TRY(op_bicubic_at_color<T>(ctx, a, du, dv, o, cnt, nx, ny, nz, ch, bo));
    OFX_HIP(ctx, hipMemcpyAsync(out, o, cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return h.sync();
}

template <typename T>
int gradient3_t(ofx_ctx *ctx, const double *f, double *gx, double *gy, double *gz, int nx, int ny, int nz)
{
    HostOp<T> h{ctx};
    const size_t df = (size_t) nx * ny, n = df * nz;
    T *a, *ox, *oy, *oz;
    OFX_TRY(h.in(f, &a, n));
    OFX_TRY(h.out_alloc(&ox, n));
    OFX_TRY(h.out_alloc(&oy, n));
    OFX_TRY(h.out_alloc(&oz, n));
    OFX_TRY(op_centered_gradient_planes<T>(ctx, nz, a, ox, oy, nx, ny));          // all frames in one launch
    OFX_TRY(op_gradient_dz<T>(ctx, a, oz, nx, ny, nz));
    OFX_TRY(h.out(ox, gx, n));
    OFX_TRY(h.out(oy, gy, n));
    OFX_TRY(h.out(oz, gz, n));
    return h.sync();
}

template <typename T> int norm1_t(ofx_ctx *ctx, const double *I, double *o, int size)
{
    HostOp<T> h{ctx};
    T *a, *x;
    double *scr;
    OFX_TRY(h.in(I, &a, (size_t) size));
    OFX_TRY(h.out_alloc(&x, (size_t) size));
    OFX_TRY(ofx_alloc(ctx, op_minmax_scratch_doubles(1, (size_t) size, 1), &scr));
    OFX_TRY((op_normalize_sets<T, T>(ctx, OfxSrcPtrs{{a}}, OfxDstPtrs{{x}}, 1, 1, (size_t) size, 1, scr)));
    OFX_TRY(h.out(x, o, (size_t) size));
    return h.sync();
}

template <typename T> int minmax_t(ofx_ctx *ctx, const double *x, int size, double *mn, double *mx)
{
    HostOp<T> h{ctx};
    T *a;
    double *scr, mm[2];
    OFX_TRY(h.in(x, &a, (size_t) size));
    OFX_TRY(ofx_alloc(ctx, op_minmax_scratch_doubles(1, (size_t) size, 1), &scr));
    OFX_TRY(op_minmax_partial<T>(ctx, OfxSrcPtrs{{a}}, 1, 1, (size_t) size, 1, scr));
    OFX_TRY(op_minmax_final(ctx, 1, (size_t) size, 1, scr));
    OFX_HIP(ctx, hipMemcpyAsync(mm, op_minmax_result(scr), 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    OFX_TRY(h.sync());
    *mn = mm[0];
    *mx = mm[1];
    return OFX_OK;
}

} // namespace

#define DISPATCH(ctx, fn, ...) ((ctx)->precision == OFX_F64 ? fn<double>(__VA_ARGS__) : fn<float>(__VA_ARGS__))

extern "C" {

void ofx_zoom_size(int nx, int ny, int *nxx, int *nyy, double factor)      // src/zoom.cpp:22-34
{
    *nxx = (int) (nx * factor + 0.5);
    *nyy = (int) (ny * factor + 0.5);
}

int ofx_divergence(ofx_ctx *ctx, const double *v1, const double *v2, double *div, int nx, int ny)
{
    OFX_ENTER(ctx);
    if (!v1 || !v2 || !div) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, divergence_t, ctx, v1, v2, div, nx, ny);
}

int ofx_forward_gradient(ofx_ctx *ctx, const double *f, double *fx, double *fy, int nx, int ny)
{
    OFX_ENTER(ctx);
    if (!f || !fx || !fy) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, gradient_t, ctx, f, fx, fy, nx, ny, false);
}

int ofx_centered_gradient(ofx_ctx *ctx, const double *f, double *dx, double *dy, int nx, int ny)
{
    OFX_ENTER(ctx);
    if (!f || !dx || !dy) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, gradient_t, ctx, f, dx, dy, nx, ny, true);
}

int ofx_dxx(ofx_ctx *ctx, const double *I, double *o, int nx, int ny)
{
    OFX_ENTER(ctx);
    if (!I || !o) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, second_t, ctx, I, o, nx, ny, 0);
}

int ofx_dyy(ofx_ctx *ctx, const double *I, double *o, int nx, int ny)
{
    OFX_ENTER(ctx);
    if (!I || !o) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, second_t, ctx, I, o, nx, ny, 1);
}

int ofx_dxy(ofx_ctx *ctx, const double *I, double *o, int nx, int ny)
{
    OFX_ENTER(ctx);
    if (!I || !o) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, second_t, ctx, I, o, nx, ny, 2);
}

int ofx_gaussian(ofx_ctx *ctx, double *I, int nx, int ny, double sigma)
{
    OFX_ENTER(ctx);
    if (!I) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    if (!(sigma > 0)) return ofx_fail(ctx, OFX_ERR_ARG, "gaussian: sigma=%g", sigma);
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, gaussian_t, ctx, I, nx, ny, sigma);
}

int ofx_bicubic_at(ofx_ctx *ctx, const double *input, const double *uu, const double *vv, double *out, int n,
                   int nx, int ny, int border_out)
{
    OFX_ENTER(ctx);
    if (!input || !uu || !vv || !out || n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer / n < 1");
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, at_t, ctx, input, uu, vv, out, n, nx, ny, border_out);
}

int ofx_bicubic_warp(ofx_ctx *ctx, const double *input, const double *u, const double *v, double *output, int nx,
                     int ny, int border_out)
{
    OFX_ENTER(ctx);
    if (!input || !u || !v || !output) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, warp_t, ctx, input, u, v, output, nx, ny, border_out);
}

int ofx_zoom_out(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, double factor)
{
    OFX_ENTER(ctx);
    if (!I || !Iout) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    if (!(factor > 0) || !(factor < 1)) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out: factor=%g", factor);
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, zoom_out_t, ctx, I, Iout, nx, ny, factor);
}

int ofx_zoom_in(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, int nxx, int nyy)
{
    OFX_ENTER(ctx);
    if (!I || !Iout) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    OFX_TRY(check_dims(ctx, nx, ny));
    if (nxx < 1 || nyy < 1) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_in: bad output size");
    return DISPATCH(ctx, zoom_in_t, ctx, I, Iout, nx, ny, nxx, nyy);
}

int ofx_bicubic_at_color(ofx_ctx *ctx, const double *input, const double *uu, const double *vv, double *out, int n,
                         int nx, int ny, int nz, int k, int border_out)
{
    OFX_ENTER(ctx);
    if (!input || !uu || !vv || !out || n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer / n < 1");
    if (nz < 1 || k < 0 || k >= nz) return ofx_fail(ctx, OFX_ERR_ARG, "bicubic_at_color: channel %d of %d", k, nz);
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, at_color_t, ctx, input, uu, vv, out, n, nx, ny, nz, k, border_out);
}

int ofx_centered_gradient3(ofx_ctx *ctx, const double *f, double *dx, double *dy, double *dz, int nx, int ny, int nz)
{
    OFX_ENTER(ctx);
    if (!f || !dx || !dy || !dz) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    if (nz < 1) return ofx_fail(ctx, OFX_ERR_ARG, "centered_gradient3: nz=%d", nz);
    OFX_TRY(check_dims(ctx, nx, ny));
    return DISPATCH(ctx, gradient3_t, ctx, f, dx, dy, dz, nx, ny, nz);
}

int ofx_zoom_out_color(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, int nz, double factor)
{
    // src/zoom.cpp:85-125 copies and smooths only nx*ny samples of the nz-channel image and then indexes that
    // scratch copy with interleaved-channel offsets: for nz > 1 it reads beyond the allocation (undefined
    // behaviour), for nz == 1 it IS zoom_out.  Only the defined case is provided.
    if (!ctx) return OFX_ERR_ARG;
    if (nz != 1) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out_color: nz=%d (the reference is only defined for nz = 1)", nz);
    return ofx_zoom_out(ctx, I, Iout, nx, ny, factor);
}

int ofx_zoom_out_channels(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, int nz, double factor)
{
    // the zoom_out of the IPOL original (3rdparty/ipoldfmethods_20160307/zoom.h:45-85): every one of the nx*ny*nz elements is
    // copied and smoothed, so each channel is zoom_out of that channel -- the function src/zoom.cpp:85-125 was derived from
    OFX_ENTER(ctx);
    if (!I || !Iout) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer");
    if (nz < 1 || nz > OFX_REXPO_MAX_CHANNELS)
        return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out_channels: nz=%d (1..%d channels)", nz, OFX_REXPO_MAX_CHANNELS);
    if (!(factor > 0) || !(factor < 1)) return ofx_fail(ctx, OFX_ERR_ARG, "zoom_out_channels: factor=%g", factor);
    OFX_TRY(check_dims(ctx, nx, ny));
    if ((long long) nx * ny * nz > 0x7fffffffLL) return ofx_fail(ctx, OFX_ERR_ARG, "bad image size %dx%dx%d", nx, ny, nz);
    return DISPATCH(ctx, zoom_out_channels_t, ctx, I, Iout, nx, ny, nz, factor);
}

int ofx_image_normalization_1(ofx_ctx *ctx, const double *I, double *In, int size)
{
    OFX_ENTER(ctx);
    if (!I || !In || size < 1) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer / size < 1");
    return DISPATCH(ctx, norm1_t, ctx, I, In, size);
}

int ofx_getminmax(ofx_ctx *ctx, const double *x, int n, double *min, double *max)
{
    OFX_ENTER(ctx);
    if (!x || !min || !max || n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer / n < 1");
    return DISPATCH(ctx, minmax_t, ctx, x, n, min, max);
}

// the head of the *_dev solvers on its own: sources in the context's "input" kind, ny rows of nx * nz elements `pitch` bytes apart
// (0: back to back), results in the storage type (include/ofx.h)
static int normalize_frames(ofx_ctx *ctx, int nsets, int per, const void *const *src, void *const *dst, int nx, int ny, int nz, int guard,
                            size_t pitch)
{
    if (!src || !dst) return ofx_fail(ctx, OFX_ERR_ARG, "normalize_frames: NULL pointer array");
    if (nsets < 1 || per < 1 || (long long) nsets * per > OFX_MM_MAX_SRC)
        return ofx_fail(ctx, OFX_ERR_ARG, "normalize_frames: %d sets of %d sources (at most %d sources)", nsets, per, OFX_MM_MAX_SRC);
    if (nx < 1 || ny < 1 || nz < 1 || (long long) nx * ny * nz > 0x7fffffffLL)
        return ofx_fail(ctx, OFX_ERR_ARG, "normalize_frames: %lld x %d elements", (long long) nx * ny, nz);
    const int kind = ofx_src_kind(ctx);
    if (kind == OFX_SRC_RGB8 && nz != 1)
        return ofx_fail(ctx, OFX_ERR_ARG, "normalize_frames: OFX_IN_RGB8 sources give one gray channel (nz = %d)", nz);
    const size_t el = ctx->precision == OFX_F64 ? sizeof(double) : sizeof(float);
    OfxSrcPtrs in = {};
    OfxDstPtrs out = {};
    for (int q = 0; q < nsets * per; q++) {
        if (!src[q] || !dst[q] || reinterpret_cast<uintptr_t>(src[q]) % ofx_src_align(kind) || reinterpret_cast<uintptr_t>(dst[q]) % el)
            return ofx_fail(ctx, OFX_ERR_ARG, "normalize_frames: source or destination %d NULL or misaligned", q);
        in.p[q] = src[q];
        out.p[q] = dst[q];
    }
    double *scr;
    OFX_TRY(ofx_alloc(ctx, op_minmax_scratch_doubles(nsets, (size_t) nx * ny, nz), &scr));
    return ctx->precision == OFX_F64 ? op_normalize_sets_in<double>(ctx, kind, in, out, nsets, per, nx, ny, pitch, nz, scr, guard)
                                     : op_normalize_sets_in<float>(ctx, kind, in, out, nsets, per, nx, ny, pitch, nz, scr, guard);
}
int ofx_normalize_frames_dev(ofx_ctx *ctx, int nsets, int per, const void *const *src, void *const *dst, int npix, int nz, int guard)
{
    OFX_ENTER(ctx);
    if (ctx->input_pitch != 0)
        return ofx_fail(ctx, OFX_ERR_ARG, "normalize_frames: no row length to take the input_pitch of %lld bytes by (ofx_normalize_frames2d_dev)",
                        ctx->input_pitch);
    return normalize_frames(ctx, nsets, per, src, dst, npix, 1, nz, guard, 0);
}
int ofx_normalize_frames2d_dev(ofx_ctx *ctx, int nsets, int per, const void *const *src, void *const *dst, int nx, int ny, int nz, int guard)
{
    OFX_ENTER(ctx);
    if (nx >= 1 && nz >= 1 && (long long) nx * nz <= 0x7fffffffLL) OFX_TRY(ofx_pitch_check(ctx, "normalize_frames", nx * nz));
    return normalize_frames(ctx, nsets, per, src, dst, nx, ny, nz, guard, (nx >= 1 && nz >= 1) ? ofx_src_pitch(ctx, nx * nz) : 0);
}

// the rest of that head on its own: op_build_pyramid_group straight into the caller's level arrays (include/ofx.h)
int ofx_pyramid_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI0, const void *const *dI1, int nx, int ny, int nscales,
                          double zfactor, double sigma, void *const *dL0, void *const *dL1)
{
    OFX_ENTER(ctx);
    if (!dI0 || !dI1 || !dL0 || !dL1) return ofx_fail(ctx, OFX_ERR_ARG, "pyramid: NULL pointer array");
    if (n_pairs < 1 || n_pairs > OFX_MAX_GROUP)
        return ofx_fail(ctx, OFX_ERR_ARG, "pyramid: a lockstep group holds 1..%d pairs (got %d)", OFX_MAX_GROUP, n_pairs);
    if (!(sigma > 0)) return ofx_fail(ctx, OFX_ERR_ARG, "pyramid: sigma=%g", sigma);
    if (nx < 2 || ny < 2 || (long long) 2 * n_pairs * nx * ny > 0x7fffffffLL)
        return ofx_fail(ctx, OFX_ERR_ARG, "pyramid: %d pairs of %dx%d", n_pairs, nx, ny);
    std::vector<int> nxs, nys;
    OFX_TRY(op_pyramid_sizes(ctx, nx, ny, nscales, zfactor, nxs, nys));
    // the builder's own refusals (gauss_taps_checked per Gaussian), taken before anything is enqueued: a refused call writes nothing
    for (int s = 0; s < nscales; s++) {
        GaussTaps taps;
        const double sg = s ? 0.6 * sqrt(1.0 / (zfactor * zfactor) - 1.0) : sigma;      // level s is smoothed from level max(s - 1, 0)
        const int w = nxs[s ? s - 1 : 0], h = nys[s ? s - 1 : 0];
        if (ofx_gauss_taps(sg, &taps) != OFX_OK)
            return ofx_fail(ctx, OFX_ERR_ARG, "pyramid: sigma %g needs more than %d taps", sg, OFX_GAUSS_MAX_TAPS);
        if (taps.size >= w || taps.size >= h)
            return ofx_fail(ctx, OFX_ERR_SIGMA, "GaussianSmooth: sigma too large (radius %d, image %dx%d, scale %d)", taps.size, w, h, s);
    }
    const int kind = ofx_src_kind(ctx);
    OFX_TRY(ofx_pitch_check(ctx, "pyramid", nx));
    const size_t pitch = ofx_src_pitch(ctx, nx);
    const size_t el = ctx->precision == OFX_F64 ? sizeof(double) : sizeof(float);
    for (int g = 0; g < n_pairs; g++)
        if (!dI0[g] || !dI1[g] || reinterpret_cast<uintptr_t>(dI0[g]) % ofx_src_align(kind) || reinterpret_cast<uintptr_t>(dI1[g]) % ofx_src_align(kind))
            return ofx_fail(ctx, OFX_ERR_ARG, "pyramid: image of pair %d NULL or misaligned", g);
    for (int s = 0; s < nscales; s++)
        if (!dL0[s] || !dL1[s] || reinterpret_cast<uintptr_t>(dL0[s]) % el || reinterpret_cast<uintptr_t>(dL1[s]) % el)
            return ofx_fail(ctx, OFX_ERR_ARG, "pyramid: level %d NULL or misaligned", s);
    const size_t full = (size_t) 2 * n_pairs * nx * ny;
    double *scr;
    OFX_TRY(ofx_alloc(ctx, (size_t) n_pairs * op_pyramid_scratch_doubles(), &scr));
    if (ctx->precision == OFX_F64) {
        double *tmpA, *tmpB;
        OFX_TRY(ofx_alloc(ctx, full, &tmpA));
        OFX_TRY(ofx_alloc(ctx, full, &tmpB));
        return op_build_pyramid_group<double>(ctx, n_pairs, dI0, dI1, nscales, zfactor, sigma, nxs.data(), nys.data(),
                                              (double *const *) dL0, (double *const *) dL1, tmpA, tmpB, scr, kind, pitch);
    }
    float *tmpA, *tmpB;
    OFX_TRY(ofx_alloc(ctx, full, &tmpA));
    OFX_TRY(ofx_alloc(ctx, full, &tmpB));
    return op_build_pyramid_group<float>(ctx, n_pairs, dI0, dI1, nscales, zfactor, sigma, nxs.data(), nys.data(),
                                         (float *const *) dL0, (float *const *) dL1, tmpA, tmpB, scr, kind, pitch);
}

int ofx_image_normalization_2(ofx_ctx *ctx, const double *I1, const double *I2, double *I1n, double *I2n, int size)
{
    OFX_ENTER(ctx);
    if (!I1 || !I2 || !I1n || !I2n || size < 1) return ofx_fail(ctx, OFX_ERR_ARG, "NULL pointer / size < 1");
    return DISPATCH(ctx, norm_t, ctx, I1, I2, I1n, I2n, size);
}

} // extern "C"
