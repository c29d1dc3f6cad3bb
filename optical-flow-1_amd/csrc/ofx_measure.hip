// ofx_measure.hip -- measure and show a flow: the error statistics of a .flo payload against its ground truth (end-point error,
// Barron's angular error, outlier rates as Middlebury R-x and KITTI Fl count them, a histogram to take percentiles from:
// ofx_flow_error_dev) and the image encodings of a payload: the Middlebury colour wheel (Baker et al., "A database and evaluation
// methodology for optical flow", IJCV 2011), the bounded 8-bit x / y coding that two-stream action-recognition pipelines store and
// KITTI's 16-bit coding, with the decodings of the latter two (ofx_flow_encode_dev, ofx_flow_decode_dev).
//
// All arithmetic in double, every operation rounded (the build's -ffp-contract=off), division and sqrt correctly rounded,
// association as written in include/ofx.h; acos and atan2 are the device library's.
//     fin(x) = x - x == 0;  shown(u, v) = fin(u) && fin(v) && |u| <= 1e9 && |v| <= 1e9
//     known = map byte 0 && shown(gu, gv);  bad = known && !(fin(u) && fin(v));  good = known && !bad
// Pure functions of the payload floats, the map bytes and the arguments: the same bytes in every storage precision.
#include "ofx_device.h"
#include "ofx_ops.h"
#include "ofx_pairs.h"
#include "ofx_sum64.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#define ME_NT 8                                  // thresholds of a call
#define ME_NR 14                                 // values of a row: Se S2 Sa max known bad out[8]
#define ME_LDS_BINS 4096                         // a histogram of up to this many bins is counted in LDS first
#define ME_UNKNOWN 1e9
#define ME_DEG 57.29577951308232
#define ME_PI 3.141592653589793

struct OfxErrorSlots {
    const float2        *flo[OFX_MAX_GROUP];
    const float2        *gt[OFX_MAX_GROUP];
    const unsigned char *occ[OFX_MAX_GROUP];     // NULL: all valid
    double              *rec[OFX_MAX_GROUP];
    float               *epe[OFX_MAX_GROUP];     // NULL: not wanted
    unsigned int        *hist[OFX_MAX_GROUP];    // NULL: not wanted; zeroed before the launch
};
struct OfxErrorThr { double abs[ME_NT], rel[ME_NT]; };

OFX_DEV bool me_fin(double x) { return x - x == 0.0; }
OFX_DEV bool me_shown(double u, double v) { return me_fin(u) && me_fin(v) && fabs(u) <= ME_UNKNOWN && fabs(v) <= ME_UNKNOWN; }
OFX_DEV int me_count(bool p) { return __popcll(__ballot(p)); }              // the same in all lanes of a wave

// ---- the error statistics of a row ----------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup; slot z = blockIdx.y.  Lane l takes the columns l, l + 64, ... left to right, the first
// half of sum64 on terms that never reach memory: three running sums in registers, started at -0.0 so that the first addition
// leaves the first term's bits (a lane without a column holds +0.0), the running maximum, and the counts as ballots (order-free).
// Both payloads are read once, one float2 per lane and round; the map one byte per lane.  A pixel that is not good adds +0.0 by a
// select.  The EPE map is stored one float per lane; the histogram is counted in LDS where it fits (a block's nonzero bins then go
// to memory as integer atomics), otherwise by integer atomics in memory.  rows[(z * 14 + m) * ny + i] receives value m of row i.
__global__ __launch_bounds__(256) void k_error_rows(OfxErrorSlots P, OfxErrorThr T, double *__restrict__ rows, int n_thr, int n_bins,
                                                    double bin_w, int lds_bins, int nx, int ny)
{
    extern __shared__ unsigned int sh_hist[];
    const int z = blockIdx.y, i = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    unsigned int *hist = P.hist[z];
    const bool in_lds = hist && lds_bins > 0;                                // the same in all threads of a workgroup
    if (in_lds) {
        for (int b = threadIdx.x; b < n_bins; b += 256) sh_hist[b] = 0;
        __syncthreads();
    }
    if (i < ny) {                                                            // the same in all lanes of a wave
        const float2 *flo = P.flo[z] + (size_t) i * nx, *gt = P.gt[z] + (size_t) i * nx;
        const unsigned char *occ = P.occ[z] ? P.occ[z] + (size_t) i * nx : nullptr;
        float *epe = P.epe[z] ? P.epe[z] + (size_t) i * nx : nullptr;
        const int l = (int) threadIdx.x & 63;
        double se = l < nx ? -0.0 : 0.0, s2 = se, sa = se, mx = 0.0;
        int known_n = 0, bad_n = 0, out_n[ME_NT];
#pragma unroll
        for (int k = 0; k < ME_NT; k++) out_n[k] = 0;
        for (int j0 = 0; j0 < nx; j0 += 64) {                                // all lanes stay for the ballots
            const int j = j0 + l;
            const bool in = j < nx;
            const float2 f = in ? flo[j] : make_float2(0.f, 0.f), g = in ? gt[j] : make_float2(0.f, 0.f);
            const double u = (double) f.x, v = (double) f.y, gu = (double) g.x, gv = (double) g.y;
            const bool known = in && !(occ && occ[j] != 0) && me_shown(gu, gv);
            const bool bad = known && !(me_fin(u) && me_fin(v));
            const bool good = known && !bad;
            const double du = u - gu, dv = v - gv;
            const double e2 = du * du + dv * dv;
            const double e = sqrt(e2);
            const double g2 = gu * gu + gv * gv;
            const double gm = sqrt(g2);
            const double num = (u * gu + v * gv) + 1.0;
            const double den = sqrt((u * u + v * v) + 1.0) * sqrt(g2 + 1.0);
            double c = num / den;
            c = c > 1.0 ? 1.0 : c;
            c = c < -1.0 ? -1.0 : c;
            const double ae = acos(good ? c : 1.0);
            if (in) {
                se = se + (good ? e : 0.0);
                s2 = s2 + (good ? e2 : 0.0);
                sa = sa + (good ? ae : 0.0);
            }
            mx = good && e > mx ? e : mx;
            known_n += me_count(known);
            bad_n += me_count(bad);
#pragma unroll
            for (int k = 0; k < ME_NT; k++)
                if (k < n_thr) out_n[k] += me_count(bad || (good && e > T.abs[k] && e > T.rel[k] * gm));
            if (epe && in) epe[j] = good ? (float) e : (bad ? __uint_as_float(0x7F800000u) : __uint_as_float(0x7FC00000u));
            if (hist && known) {
                int bin = n_bins - 1;
                if (good) {
                    const double q = e / bin_w;
                    bin = q >= (double) n_bins ? n_bins - 1 : (int) q;
                }
                if (in_lds) atomicAdd(&sh_hist[bin], 1u);
                else atomicAdd(&hist[bin], 1u);
            }
        }
        se = tk_sum64_lanes(se);
        s2 = tk_sum64_lanes(s2);
        sa = tk_sum64_lanes(sa);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const double o = __shfl_down(mx, s, 64);
            mx = o > mx ? o : mx;
        }
        if (l == 0) {
            double *r = rows + (size_t) z * ME_NR * ny + i;
            r[0] = se;
            r[(size_t) ny] = s2;
            r[(size_t) 2 * ny] = sa;
            r[(size_t) 3 * ny] = mx;
            r[(size_t) 4 * ny] = (double) known_n;
            r[(size_t) 5 * ny] = (double) bad_n;
#pragma unroll
            for (int k = 0; k < ME_NT; k++) r[(size_t) (6 + k) * ny] = (double) out_n[k];
        }
    }
    if (in_lds) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_bins; b += 256) {
            const unsigned int c = sh_hist[b];
            if (c) atomicAdd(&hist[b], c);
        }
    }
}

// One wave per slot: sum64 over the row sums (the counts are integers below 2^31 each and below 2^53 together: every order gives the
// same double), the maximum over the row maxima, then lane 0 writes the whole record.
__global__ __launch_bounds__(64) void k_error_finish(OfxErrorSlots P, const double *__restrict__ rows, int ny)
{
    const int z = blockIdx.x, l = threadIdx.x;
    const double *r = rows + (size_t) z * ME_NR * ny;
    double S[ME_NR];
#pragma unroll
    for (int m = 0; m < ME_NR; m++)
        if (m != 3) S[m] = tk_sum64(r + (size_t) m * ny, ny);
    double mx = 0.0;
    for (int i = l; i < ny; i += 64) {
        const double o = r[(size_t) 3 * ny + i];
        mx = o > mx ? o : mx;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double o = __shfl_down(mx, s, 64);
        mx = o > mx ? o : mx;
    }
    if (l != 0) return;
    double *rec = P.rec[z];
    const double ng = S[4] - S[5];
    const bool any = ng > 0.0;
    rec[0] = S[4];
    rec[1] = S[5];
    rec[2] = any ? S[0] / ng : 0.0;
    rec[3] = any ? sqrt(S[1] / ng) : 0.0;
    rec[4] = any ? (S[2] / ng) * ME_DEG : 0.0;
    rec[5] = any ? mx : 0.0;
    rec[6] = any ? S[0] : 0.0;
    rec[7] = any ? S[2] : 0.0;
#pragma unroll
    for (int k = 0; k < ME_NT; k++) rec[8 + k] = S[6 + k];
}

// ---- the encodings --------------------------------------------------------------------------------------------------------------
struct OfxCodeSlots {
    const void          *src[OFX_MAX_GROUP];     // encode: the payload; decode: the coded image
    const unsigned char *occ[OFX_MAX_GROUP];     // encode: the map read (NULL: all valid)
    void                *dst[OFX_MAX_GROUP];     // encode: the coded image; decode: the payload
    unsigned char       *map[OFX_MAX_GROUP];     // decode: the map written (NULL: not wanted)
};

// max sqrt(u * u + v * v) over the vis pixels of slot z = blockIdx.y, as the bits of a double >= +0.0 (their order is the order
// of the values): a wave's maximum by shuffles, then one integer atomic per wave into maxrad[z], zeroed before the launch.
__global__ __launch_bounds__(256) void k_flow_maxrad(OfxCodeSlots P, unsigned long long *__restrict__ maxrad, int nx, int ny)
{
    const int z = blockIdx.y;
    const long long n = (long long) nx * ny;
    const float2 *flo = static_cast<const float2 *>(P.src[z]);
    const unsigned char *occ = P.occ[z];
    double mx = 0.0;
    for (long long p = (long long) blockIdx.x * 256 + threadIdx.x; p < n; p += (long long) gridDim.x * 256) {
        const float2 f = flo[p];
        const double u = (double) f.x, v = (double) f.y;
        const bool vis = !(occ && occ[p] != 0) && me_shown(u, v);
        const double rad = sqrt(u * u + v * v);
        mx = vis && rad > mx ? rad : mx;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double o = __shfl_down(mx, s, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx > 0.0) atomicMax(&maxrad[z], (unsigned long long) __double_as_longlong(mx));
}

// entry k of the 55-entry wheel: the six segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 of include/ofx.h, integer divisions
OFX_DEV void me_wheel(int k, int &r, int &g, int &b)
{
    if (k < 15) { r = 255; g = 255 * k / 15; b = 0; }
    else if (k < 21) { r = 255 - 255 * (k - 15) / 6; g = 255; b = 0; }
    else if (k < 25) { r = 0; g = 255; b = 255 * (k - 21) / 4; }
    else if (k < 36) { r = 0; g = 255 - 255 * (k - 25) / 11; b = 255; }
    else if (k < 49) { r = 255 * (k - 36) / 13; g = 0; b = 255; }
    else { r = 255; g = 0; b = 255 - 255 * (k - 49) / 6; }
}
OFX_DEV unsigned char me_wheel_byte(int w0, int w1, double f, double rad)
{
    const double c0 = (double) w0 / 255.0, c1 = (double) w1 / 255.0;
    double col = (1.0 - f) * c0 + f * c1;
    col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
    return (unsigned char) (int) (255.0 * col);
}
OFX_DEV unsigned char me_bound(double f, double B)
{
    if (f <= -B) return 0;
    if (f >= B) return 255;
    return (unsigned char) (int) (255.0 * (f + B) / (2.0 * B) + 0.5);
}
OFX_DEV unsigned short me_kitti(double f)
{
    const double x = f * 64.0 + 32768.0;
    if (x <= 0.0) return 0;
    if (x >= 65535.0) return 65535;
    return (unsigned short) (int) (x + 0.5);
}

// A thread owns a pixel, slot z = blockIdx.y.  The 2 or 3 bytes (or 3 uint16) of a pixel are stored one by one at whatever address
// the destination has: a wave writes 128, 192 or 384 contiguous bytes and no byte outside the destination.
__global__ __launch_bounds__(256) void k_flow_encode(OfxCodeSlots P, const unsigned long long *__restrict__ maxrad, int kind, double scale,
                                                     int nx, int ny)
{
    const int z = blockIdx.y;
    const long long p = (long long) blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long) nx * ny) return;
    const float2 f = static_cast<const float2 *>(P.src[z])[p];
    const double u = (double) f.x, v = (double) f.y;
    const bool vis = !(P.occ[z] && P.occ[z][p] != 0) && me_shown(u, v);
    if (kind == OFX_ENC_WHEEL_RGB8) {
        unsigned char *dst = static_cast<unsigned char *>(P.dst[z]) + 3 * p;
        double mr = scale;
        if (maxrad) {
            mr = __longlong_as_double((long long) maxrad[z]);
            mr = mr == 0.0 ? 1.0 : mr;
        }
        unsigned char R = 0, G = 0, B = 0;
        if (vis) {
            const double fx = u / mr, fy = v / mr;
            const double rad = sqrt(fx * fx + fy * fy);
            const double a = atan2(-fy, -fx) / ME_PI;
            const double fk = (a + 1.0) / 2.0 * 54.0;
            const int k0 = (int) fk, k1 = (k0 + 1) % 55;
            const double t = fk - (double) k0;
            int r0, g0, b0, r1, g1, b1;
            me_wheel(k0, r0, g0, b0);
            me_wheel(k1, r1, g1, b1);
            R = me_wheel_byte(r0, r1, t, rad);
            G = me_wheel_byte(g0, g1, t, rad);
            B = me_wheel_byte(b0, b1, t, rad);
        }
        dst[0] = R; dst[1] = G; dst[2] = B;
    } else if (kind == OFX_ENC_BOUND_U8) {
        unsigned char *dst = static_cast<unsigned char *>(P.dst[z]) + 2 * p;
        dst[0] = me_bound(vis ? u : 0.0, scale);
        dst[1] = me_bound(vis ? v : 0.0, scale);
    } else {
        unsigned short *dst = static_cast<unsigned short *>(P.dst[z]) + 3 * p;
        dst[0] = vis ? me_kitti(u) : 0;
        dst[1] = vis ? me_kitti(v) : 0;
        dst[2] = vis ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_flow_decode(OfxCodeSlots P, int kind, double scale, int nx, int ny)
{
    const int z = blockIdx.y;
    const long long p = (long long) blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long) nx * ny) return;
    float2 out;
    unsigned char flag = 0;
    if (kind == OFX_ENC_BOUND_U8) {
        const unsigned char *src = static_cast<const unsigned char *>(P.src[z]) + 2 * p;
        out.x = (float) (((double) src[0] * (2.0 * scale)) / 255.0 - scale);
        out.y = (float) (((double) src[1] * (2.0 * scale)) / 255.0 - scale);
    } else {
        const unsigned short *src = static_cast<const unsigned short *>(P.src[z]) + 3 * p;
        if (src[2] != 0) {
            out.x = (float) (((double) src[0] - 32768.0) / 64.0);
            out.y = (float) (((double) src[1] - 32768.0) / 64.0);
        } else {
            out.x = out.y = __uint_as_float(0x7FC00000u);
            flag = 255;
        }
    }
    static_cast<float2 *>(P.dst[z])[p] = out;
    if (P.map[z]) P.map[z][p] = flag;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static bool me_misaligned(const void *p, size_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }
static const void *me_at(const void *const *t, int g) { return t ? t[g] : nullptr; }
static void *me_at(void *const *t, int g) { return t ? t[g] : nullptr; }

static int me_check_size(ofx_ctx *ctx, const char *who, int n, int nx, int ny)
{
    if (n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n = %d (at least 1)", who, n);
    if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: flow field %dx%d too small", who, nx, ny);
    if ((long long) nx * ny > (long long) INT_MAX - 2048) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %dx%d pixels do not fit an int", who, nx, ny);
    return OFX_OK;
}

// The byte ranges of a call: an output may not touch an input or another output; inputs may share.
struct MeRange { uintptr_t lo, hi; bool out; };
struct MeRanges {
    std::vector<MeRange> v;
    void add(const void *p, size_t bytes, bool out)
    {
        if (p) v.push_back({reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes, out});
    }
    bool clash()
    {
        std::sort(v.begin(), v.end(), [](const MeRange &a, const MeRange &b) { return a.lo < b.lo; });
        uintptr_t end_in = 0, end_out = 0;                                   // the furthest end of the ranges before this one
        for (const MeRange &r : v) {
            if (r.lo < end_out || (r.out && r.lo < end_in)) return true;
            uintptr_t &e = r.out ? end_out : end_in;
            e = std::max(e, r.hi);
        }
        return false;
    }
};

extern "C" int ofx_flow_error_dev(ofx_ctx *ctx, int n, const void *const *d_flo, const void *const *d_flo_gt, const void *const *d_occ,
                                  int n_thr, const double *thr_abs, const double *thr_rel, void *const *d_rec, void *const *d_epe,
                                  void *const *d_hist, int n_bins, double bin_w, int nx, int ny)
{
    OFX_ENTER(ctx);
    const char *who = "flow_error";
    if (!d_flo || !d_flo_gt || !d_rec) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    OFX_TRY(me_check_size(ctx, who, n, nx, ny));
    if (n_thr < 0 || n_thr > ME_NT) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_thr = %d (0 .. %d)", who, n_thr, ME_NT);
    if (n_thr > 0 && (!thr_abs || !thr_rel)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL threshold array", who);
    OfxErrorThr T = {};
    for (int k = 0; k < n_thr; k++) {
        if (!std::isfinite(thr_abs[k]) || thr_abs[k] < 0.0 || !std::isfinite(thr_rel[k]) || thr_rel[k] < 0.0)
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: threshold %d = (%g, %g) (finite, not negative)", who, k, thr_abs[k], thr_rel[k]);
        T.abs[k] = thr_abs[k];
        T.rel[k] = thr_rel[k];
    }
    bool any_hist = false;
    for (int g = 0; g < n; g++) {
        if (!d_flo[g] || !d_flo_gt[g] || !d_rec[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        any_hist = any_hist || me_at(d_hist, g);
    }
    if (any_hist) {
        if (n_bins < 1 || n_bins > 65536) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_bins = %d (1 .. 65536)", who, n_bins);
        if (!std::isfinite(bin_w) || !(bin_w > 0.0)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: bin_w = %g (finite, above 0)", who, bin_w);
    }
    const size_t px = (size_t) nx * ny;
    MeRanges R;
    for (int g = 0; g < n; g++) {
        if (me_misaligned(d_flo[g], sizeof(float2)) || me_misaligned(d_flo_gt[g], sizeof(float2)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a payload of slot %d is not 8-byte aligned", who, g);
        if (me_misaligned(d_rec[g], sizeof(double))) return ofx_fail(ctx, OFX_ERR_ARG, "%s: the record of slot %d is not 8-byte aligned", who, g);
        if (me_misaligned(me_at(d_epe, g), sizeof(float)) || me_misaligned(me_at(d_hist, g), sizeof(unsigned int)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the EPE map or histogram of slot %d is not 4-byte aligned", who, g);
        R.add(d_flo[g], px * sizeof(float2), false);
        R.add(d_flo_gt[g], px * sizeof(float2), false);
        R.add(me_at(d_occ, g), px, false);
        R.add(d_rec[g], OFX_ERROR_REC * sizeof(double), true);
        R.add(me_at(d_epe, g), px * sizeof(float), true);
        R.add(me_at(d_hist, g), (size_t) n_bins * sizeof(unsigned int), true);
    }
    if (R.clash()) return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination overlaps a buffer that the call reads or another destination", who);
    const int per = n < OFX_MAX_GROUP ? n : OFX_MAX_GROUP;
    const int lds_bins = any_hist && n_bins <= ME_LDS_BINS ? n_bins : 0;
    double *rows;
    OFX_TRY(ofx_alloc(ctx, (size_t) per * ME_NR * ny, &rows));
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxErrorSlots S = {};
        void *rec[OFX_MAX_GROUP], *epe[OFX_MAX_GROUP], *hist[OFX_MAX_GROUP];
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *f, *t, *o;
            OFX_TRY(ofx_stage_in(ctx, d_flo[g], px * sizeof(float2), true, &f));
            OFX_TRY(ofx_stage_in(ctx, d_flo_gt[g], px * sizeof(float2), true, &t));
            OFX_TRY(ofx_stage_in(ctx, me_at(d_occ, g), px, true, &o));
            OFX_TRY(ofx_stage_in(ctx, d_rec[g], OFX_ERROR_REC * sizeof(double), false, &rec[z]));
            OFX_TRY(ofx_stage_in(ctx, me_at(d_epe, g), px * sizeof(float), false, &epe[z]));
            OFX_TRY(ofx_stage_in(ctx, me_at(d_hist, g), (size_t) n_bins * sizeof(unsigned int), false, &hist[z]));
            if (hist[z]) OFX_HIP(ctx, hipMemsetAsync(hist[z], 0, (size_t) n_bins * sizeof(unsigned int), ctx->stream));
            S.flo[z] = static_cast<const float2 *>(f);
            S.gt[z] = static_cast<const float2 *>(t);
            S.occ[z] = static_cast<const unsigned char *>(o);
            S.rec[z] = static_cast<double *>(rec[z]);
            S.epe[z] = static_cast<float *>(epe[z]);
            S.hist[z] = static_cast<unsigned int *>(hist[z]);
        }
        hipLaunchKernelGGL(k_error_rows, dim3(ofx_cdiv(ny, 4), cnt), dim3(256), (size_t) lds_bins * sizeof(unsigned int), ctx->stream, S, T,
                           rows, n_thr, n_bins, bin_w, lds_bins, nx, ny);
        OFX_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_error_finish, dim3(cnt), dim3(64), 0, ctx->stream, S, rows, ny);
        OFX_LAUNCH_CHECK(ctx);
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            OFX_TRY(ofx_stage_out(ctx, d_rec[g], rec[z], OFX_ERROR_REC * sizeof(double)));
            if (epe[z]) OFX_TRY(ofx_stage_out(ctx, d_epe[g], epe[z], px * sizeof(float)));
            if (hist[z]) OFX_TRY(ofx_stage_out(ctx, d_hist[g], hist[z], (size_t) n_bins * sizeof(unsigned int)));
        }
    }
    return OFX_OK;
}

static size_t me_code_bytes(int kind) { return kind == OFX_ENC_WHEEL_RGB8 ? 3 : kind == OFX_ENC_BOUND_U8 ? 2 : 6; }

// the checks that the encode and the decode entry share; `coded`: the images, `flo`: the payloads
static int me_check_code(ofx_ctx *ctx, const char *who, int n, const void *const *coded, const void *const *flo, const void *const *d_occ,
                         bool encode, int kind, double scale, int nx, int ny)
{
    if (!coded || !flo) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    OFX_TRY(me_check_size(ctx, who, n, nx, ny));
    if (kind != OFX_ENC_WHEEL_RGB8 && kind != OFX_ENC_BOUND_U8 && kind != OFX_ENC_KITTI_U16)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: kind = %d (not one of the three encodings)", who, kind);
    if (!encode && kind == OFX_ENC_WHEEL_RGB8) return ofx_fail(ctx, OFX_ERR_ARG, "%s: kind = %d: the colour wheel has no decoding", who, kind);
    if (!std::isfinite(scale) || scale < 0.0) return ofx_fail(ctx, OFX_ERR_ARG, "%s: scale = %g (finite, not negative)", who, scale);
    if (kind == OFX_ENC_BOUND_U8 && scale == 0.0) return ofx_fail(ctx, OFX_ERR_ARG, "%s: scale = 0: the bound must be above 0", who);
    if (kind == OFX_ENC_KITTI_U16 && scale != 0.0) return ofx_fail(ctx, OFX_ERR_ARG, "%s: scale = %g: the 16-bit coding takes scale 0", who, scale);
    const size_t px = (size_t) nx * ny;
    MeRanges R;
    for (int g = 0; g < n; g++) {
        if (!coded[g] || !flo[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        if (me_misaligned(flo[g], sizeof(float2))) return ofx_fail(ctx, OFX_ERR_ARG, "%s: the payload of slot %d is not 8-byte aligned", who, g);
        if (kind == OFX_ENC_KITTI_U16 && me_misaligned(coded[g], 2))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the 16-bit image of slot %d is not 2-byte aligned", who, g);
        R.add(flo[g], px * sizeof(float2), !encode);
        R.add(coded[g], px * me_code_bytes(kind), encode);
        R.add(me_at(d_occ, g), px, !encode);
    }
    if (R.clash()) return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination overlaps a buffer that the call reads or another destination", who);
    return OFX_OK;
}

extern "C" int ofx_flow_encode_dev(ofx_ctx *ctx, int n, const void *const *d_flo, const void *const *d_occ, int kind, double scale,
                                   void *const *dDst, int nx, int ny)
{
    OFX_ENTER(ctx);
    const char *who = "flow_encode";
    OFX_TRY(me_check_code(ctx, who, n, dDst, d_flo, d_occ, true, kind, scale, nx, ny));
    const size_t px = (size_t) nx * ny, coded = px * me_code_bytes(kind);
    const bool own_max = kind == OFX_ENC_WHEEL_RGB8 && scale == 0.0;
    unsigned long long *maxrad = nullptr;
    if (own_max) OFX_TRY(ofx_alloc(ctx, (size_t) OFX_MAX_GROUP, &maxrad));
    const int blocks = (int) ((px + 255) / 256);
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxCodeSlots S = {};
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *f, *o;
            OFX_TRY(ofx_stage_in(ctx, d_flo[g], px * sizeof(float2), true, &f));
            OFX_TRY(ofx_stage_in(ctx, me_at(d_occ, g), px, true, &o));
            OFX_TRY(ofx_stage_in(ctx, dDst[g], coded, false, &S.dst[z]));
            S.src[z] = f;
            S.occ[z] = static_cast<const unsigned char *>(o);
        }
        if (own_max) {
            OFX_HIP(ctx, hipMemsetAsync(maxrad, 0, OFX_MAX_GROUP * sizeof(*maxrad), ctx->stream));
            // 64 workgroups per slot: the waves' atomics on a slot's one word serialise, 256 of them cost less than the pass itself
            hipLaunchKernelGGL(k_flow_maxrad, dim3(blocks < 64 ? blocks : 64, cnt), dim3(256), 0, ctx->stream, S, maxrad, nx, ny);
            OFX_LAUNCH_CHECK(ctx);
        }
        hipLaunchKernelGGL(k_flow_encode, dim3(blocks, cnt), dim3(256), 0, ctx->stream, S, maxrad, kind, scale, nx, ny);
        OFX_LAUNCH_CHECK(ctx);
        for (int z = 0; z < cnt; z++) OFX_TRY(ofx_stage_out(ctx, dDst[g0 + z], S.dst[z], coded));
    }
    return OFX_OK;
}

extern "C" int ofx_flow_decode_dev(ofx_ctx *ctx, int n, const void *const *dSrc, int kind, double scale, void *const *d_flo,
                                   void *const *d_occ, int nx, int ny)
{
    OFX_ENTER(ctx);
    const char *who = "flow_decode";
    OFX_TRY(me_check_code(ctx, who, n, dSrc, d_flo, d_occ, false, kind, scale, nx, ny));
    const size_t px = (size_t) nx * ny, coded = px * me_code_bytes(kind);
    const int blocks = (int) ((px + 255) / 256);
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxCodeSlots S = {};
        void *map[OFX_MAX_GROUP];
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *c;
            OFX_TRY(ofx_stage_in(ctx, dSrc[g], coded, true, &c));
            OFX_TRY(ofx_stage_in(ctx, d_flo[g], px * sizeof(float2), false, &S.dst[z]));
            OFX_TRY(ofx_stage_in(ctx, me_at(d_occ, g), px, false, &map[z]));
            S.src[z] = c;
            S.map[z] = static_cast<unsigned char *>(map[z]);
        }
        hipLaunchKernelGGL(k_flow_decode, dim3(blocks, cnt), dim3(256), 0, ctx->stream, S, kind, scale, nx, ny);
        OFX_LAUNCH_CHECK(ctx);
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            OFX_TRY(ofx_stage_out(ctx, d_flo[g], S.dst[z], px * sizeof(float2)));
            if (map[z]) OFX_TRY(ofx_stage_out(ctx, d_occ[g], map[z], px));
        }
    }
    return OFX_OK;
}
