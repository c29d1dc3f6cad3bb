// ofx_median.hip -- the W x W median of a flow, per component, on interleaved (u, v) pairs of float or double: the .flo payloads
// of ofx_flow_median_dev and the planes of Tvl1Level::U (option "tvl1_median").  Definition: include/ofx.h, "Median of a flow".
//
// No arithmetic happens on the values.  An element becomes an unsigned KEY of its own width whose integer order is the order of
// the definition, -Inf < finite < +Inf < NaN:
//     key(x) = all ones                      if x is a NaN (all NaNs are equal)
//            = ~bits(x)                      if the sign bit is set
//            = bits(x) | sign bit            otherwise
// The map is one to one off the NaNs and its inverse sends the all-ones key to a NaN, so selecting among keys selects among the
// values, exactly, in every precision; a compare-exchange is an unsigned min and max, which lose nothing.
//
// The shape: a wave is 64 neighbouring columns and marches down a strip of rows.  A lane keeps the last W rows of its column in
// registers (one coalesced 8- or 16-byte load per lane and row), sorts them once per row (MEDIAN_COL_W), and the sorted column
// travels to the W lanes whose windows contain it by whole-wave DPP shifts (wave_shift_up / _down of ofx_device.h, no LDS).  The
// W sorted columns are W * W wires of the merge network MEDIAN_NET_W (ofx_median_net.h); without a map the result is the one
// wire of rank W * W / 2, and the compiler drops every comparator that wire does not depend on.  The r = W / 2 lanes at either
// end of the wave only feed their neighbours: a wave writes 64 - 2 r columns.  Window positions outside the image are the
// mirrored ones, resolved in the load addresses.
//
// With a map, a flagged position's key is all ones as well and the lanes also carry their column's count of valid positions;
// the network then sorts all wires and the wire of rank cnt / 2 is picked by a chain of selects.  Flagged positions and valid
// NaNs share a key; that is sound because a rank below cnt that lands on an all-ones key can only be a valid NaN.
#include "ofx_device.h"
#include "ofx_median_net.h"
#include "ofx_ops.h"
#include "ofx_pairs.h"

#include <climits>

#define MED_NT 256            // four waves per workgroup, each with a strip of its own (no LDS, no barrier)

// ---- keys ----------------------------------------------------------------------------------------------------------------------------
typedef unsigned med_k32;
typedef unsigned long long med_k64;
struct MedPair32 { med_k32 x, y; };
struct alignas(16) MedPair64 { med_k64 x, y; };
template <typename K> struct MedKey;
template <> struct MedKey<med_k32> {
    using pair = MedPair32;
    static constexpr med_k32 top = 0x80000000u, ones = 0xFFFFFFFFu, mag = 0x7FFFFFFFu, inf = 0x7F800000u;
};
template <> struct MedKey<med_k64> {
    using pair = MedPair64;
    static constexpr med_k64 top = 0x8000000000000000ull, ones = ~0ull, mag = 0x7FFFFFFFFFFFFFFFull, inf = 0x7FF0000000000000ull;
};
template <typename K> OFX_DEV K med_key(K b)
{
    using M = MedKey<K>;
    if ((b & M::mag) > M::inf) return M::ones;
    return (b & M::top) ? ~b : (b | M::top);
}
template <typename K> OFX_DEV K med_bits(K k)
{
    using M = MedKey<K>;
    return (k & M::top) ? (k & M::mag) : ~k;
}
OFX_DEV med_k32 med_shift_up(med_k32 v) { return (med_k32) __builtin_amdgcn_update_dpp((int) v, (int) v, 0x138, 0xf, 0xf, false); }
OFX_DEV med_k32 med_shift_down(med_k32 v) { return (med_k32) __builtin_amdgcn_update_dpp((int) v, (int) v, 0x130, 0xf, 0xf, false); }
OFX_DEV med_k64 med_shift_up(med_k64 v)
{
    return ((med_k64) med_shift_up((med_k32) (v >> 32)) << 32) | med_shift_up((med_k32) v);
}
OFX_DEV med_k64 med_shift_down(med_k64 v)
{
    return ((med_k64) med_shift_down((med_k32) (v >> 32)) << 32) | med_shift_down((med_k32) v);
}

// window index -> sample index: -k -> k - 1, n - 1 + k -> n - k (one reflection: the entries refuse W / 2 > n); lanes past the
// reflected range read the last sample and are never used
OFX_DEV int med_mirror(int i, int n)
{
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

#define MED_CE(a, b) { const K lo_ = v[a] < v[b] ? v[a] : v[b], hi_ = v[a] < v[b] ? v[b] : v[a]; v[a] = lo_; v[b] = hi_; }

template <typename K, int W> OFX_DEV void med_sort_column(K *v)
{
    if constexpr (W == 3) { MEDIAN_COL_3(MED_CE) }
    else if constexpr (W == 5) { MEDIAN_COL_5(MED_CE) }
    else { MEDIAN_COL_7(MED_CE) }
}
// the wires of W sorted columns, sorted; ord: where the ranks are
template <typename K, int W> OFX_DEV void med_merge_columns(K *v)
{
    if constexpr (W == 3) { MEDIAN_NET_3(MED_CE) }
    else if constexpr (W == 5) { MEDIAN_NET_5(MED_CE) }
    else { MEDIAN_NET_7(MED_CE) }
}
template <int W> struct MedOrd;
template <> struct MedOrd<3> { static constexpr int at[9] = {MEDIAN_ORD_3}; };
template <> struct MedOrd<5> { static constexpr int at[25] = {MEDIAN_ORD_5}; };
template <> struct MedOrd<7> { static constexpr int at[49] = {MEDIAN_ORD_7}; };

// One component of one output: col = the lane's W window keys in row order (flagged ones already all ones), cnt = its count of valid
// positions, centre = the key at the pixel itself.
template <typename K, int W, bool MASK> OFX_DEV K med_select(const K *col, int cnt, K centre)
{
    constexpr int R = W / 2, N = W * W;
    K v[N];
    K own[W];
#pragma unroll
    for (int t = 0; t < W; t++) own[t] = col[t];
    med_sort_column<K, W>(own);
#pragma unroll
    for (int t = 0; t < W; t++) v[R * W + t] = own[t];
    {
        K up[W], dn[W];
#pragma unroll
        for (int t = 0; t < W; t++) up[t] = dn[t] = own[t];
        int cu = cnt, cd = cnt;
#pragma unroll
        for (int d = 1; d <= R; d++) {
#pragma unroll
            for (int t = 0; t < W; t++) {
                up[t] = med_shift_up(up[t]);           // the column d lanes below
                dn[t] = med_shift_down(dn[t]);         // ... d lanes above
                v[(R - d) * W + t] = up[t];
                v[(R + d) * W + t] = dn[t];
            }
            if (MASK) {
                cu = (int) med_shift_up((med_k32) cu);
                cd = (int) med_shift_down((med_k32) cd);
                cnt += cu + cd;
            }
        }
    }
    med_merge_columns<K, W>(v);
    if (!MASK) return v[MedOrd<W>::at[N / 2]];
    const int rank = cnt >> 1;
    K res = centre;                                     // cnt = 0: the input, unchanged
#pragma unroll
    for (int t = 0; t < N; t++) res = (cnt > 0 && t == rank) ? v[MedOrd<W>::at[t]] : res;
    return res;
}

// Slot z = blockIdx.y.  Wave t = 4 * blockIdx.x + (its number in the workgroup) takes column strip t % sx (64 - 2 R outputs wide)
// and rows (t / sx) * rows .. + rows - 1.
template <typename K, int W, bool MASK>
__global__ __launch_bounds__(MED_NT) void k_flow_median(OfxMedianSlots S, int nx, int ny, int sx, int rows)
{
    using P = typename MedKey<K>::pair;
    constexpr int R = W / 2, OUT = 64 - 2 * R;
    const int lane = threadIdx.x & 63, t = (int) blockIdx.x * (MED_NT / 64) + ((int) threadIdx.x >> 6);
    const int sy = t / sx, i0 = sy * rows;
    if (i0 >= ny) return;                                   // the whole wave
    const int i1 = min(i0 + rows, ny);
    const int j = (t - sy * sx) * OUT + lane - R;
    const size_t cc = (size_t) med_mirror(j, nx);
    const bool writes = lane >= R && lane < 64 - R && j < nx;
    const int z = blockIdx.y;
    const P *__restrict__ in = static_cast<const P *>(S.in[z]);
    const unsigned char *__restrict__ occ = MASK ? S.occ[z] : nullptr;
    P *__restrict__ out = static_cast<P *>(S.out[z]);

    K wu[W], wv[W];
    int ok[W];
    auto load = [&](int i, K &u, K &v, int &f) {
        const size_t p = (size_t) med_mirror(i, ny) * nx + cc;
        const P q = in[p];
        u = med_key<K>(q.x);
        v = med_key<K>(q.y);
        f = (MASK && occ) ? (occ[p] == 0) : 1;
    };
#pragma unroll
    for (int k = 1; k < W; k++) load(i0 - R + k - 1, wu[k], wv[k], ok[k]);
    K nu, nv;
    int nf;
    load(i0 + R, nu, nv, nf);
    for (int i = i0; i < i1; i++) {
#pragma unroll
        for (int k = 0; k < W - 1; k++) { wu[k] = wu[k + 1]; wv[k] = wv[k + 1]; ok[k] = ok[k + 1]; }
        wu[W - 1] = nu; wv[W - 1] = nv; ok[W - 1] = nf;
        if (i + 1 < i1) load(i + 1 + R, nu, nv, nf);        // the next row is on its way while this one is selected
        K cu[W], cv[W];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < W; k++) {
            cu[k] = (!MASK || ok[k]) ? wu[k] : MedKey<K>::ones;
            cv[k] = (!MASK || ok[k]) ? wv[k] : MedKey<K>::ones;
            cnt += ok[k];
        }
        P r;
        r.x = med_bits<K>(med_select<K, W, MASK>(cu, cnt, wu[R]));
        r.y = med_bits<K>(med_select<K, W, MASK>(cv, cnt, wv[R]));
        if (writes) out[(size_t) i * nx + (size_t) j] = r;
    }
}

// rows per strip: as tall as leaves the device a few thousand waves (a strip of r rows loads r + 2 R)
static int med_pick_rows(int nx, int ny, int slots, int out)
{
    const long cols = (long) ofx_cdiv(nx, out) * slots;
    if (cols * ofx_cdiv(ny, 16) >= 4096) return 16;
    if (cols * ofx_cdiv(ny, 8) >= 2048) return 8;
    return 4;
}

template <typename K, int W>
static int med_launch(ofx_ctx *ctx, int slots, const OfxMedianSlots &S, int nx, int ny)
{
    constexpr int OUT = 64 - 2 * (W / 2);
    bool mask = false;
    for (int z = 0; z < slots; z++) mask = mask || S.occ[z];
    const int rows = med_pick_rows(nx, ny, slots, OUT), sx = ofx_cdiv(nx, OUT);
    const dim3 grid(ofx_cdiv(sx * ofx_cdiv(ny, rows), MED_NT / 64), slots);
    // one launch either way: with a map anywhere, the slots without one run the masked kernel with every position valid
    if (!mask) hipLaunchKernelGGL((k_flow_median<K, W, false>), grid, dim3(MED_NT), 0, ctx->stream, S, nx, ny, sx, rows);
    else       hipLaunchKernelGGL((k_flow_median<K, W, true>), grid, dim3(MED_NT), 0, ctx->stream, S, nx, ny, sx, rows);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

int op_flow_median(ofx_ctx *ctx, int esize, int wsize, int slots, const OfxMedianSlots &S, int nx, int ny)
{
    if (slots < 1 || slots > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "median: %d slots in one launch", slots);
    if (wsize / 2 > nx || wsize / 2 > ny) return ofx_fail(ctx, OFX_ERR_ARG, "median: window %d on %dx%d", wsize, nx, ny);
    if (esize == 4) {
        switch (wsize) {
        case 3: return med_launch<med_k32, 3>(ctx, slots, S, nx, ny);
        case 5: return med_launch<med_k32, 5>(ctx, slots, S, nx, ny);
        case 7: return med_launch<med_k32, 7>(ctx, slots, S, nx, ny);
        }
    } else if (esize == 8) {
        switch (wsize) {
        case 3: return med_launch<med_k64, 3>(ctx, slots, S, nx, ny);
        case 5: return med_launch<med_k64, 5>(ctx, slots, S, nx, ny);
        }
    }
    return ofx_fail(ctx, OFX_ERR_ARG, "median: no kernel for a %dx%d window on %d-byte elements", wsize, wsize, esize);
}

// out[z] back over in[z]: pairs of esize-byte elements, n pairs per slot, 16 bytes per thread
__global__ void k_median_copy_back(OfxMedianSlots S, size_t n16)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n16) return;
    const int z = blockIdx.y;
    static_cast<uint4 *>(const_cast<void *>(S.in[z]))[i] = static_cast<const uint4 *>(S.out[z])[i];
}
int op_median_copy_back(ofx_ctx *ctx, int esize, int slots, const OfxMedianSlots &S, size_t n)
{
    const size_t bytes = n * 2 * (size_t) esize;
    if (bytes % 16 == 0) {
        for (int z = 0; z < slots; z++)
            if (reinterpret_cast<uintptr_t>(S.in[z]) % 16 || reinterpret_cast<uintptr_t>(S.out[z]) % 16) goto plain;
        hipLaunchKernelGGL(k_median_copy_back, dim3((unsigned) ((bytes / 16 + 255) / 256), slots), dim3(256), 0, ctx->stream, S, bytes / 16);
        OFX_LAUNCH_CHECK(ctx);
        return OFX_OK;
    }
plain:
    for (int z = 0; z < slots; z++)
        OFX_HIP(ctx, hipMemcpyAsync(const_cast<void *>(S.in[z]), S.out[z], bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return OFX_OK;
}

// ---- the entry -------------------------------------------------------------------------------------------------------------------------
extern "C" int ofx_flow_median_dev(ofx_ctx *ctx, int n, const void *const *d_flo_in, const void *const *d_occ, void *const *d_flo_out,
                                   int nx, int ny, int wsize)
{
    OFX_ENTER(ctx);
    const char *who = "flow_median";
    if (!d_flo_in || !d_flo_out) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    if (n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n = %d (at least 1)", who, n);
    if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: flow %dx%d too small", who, nx, ny);
    if ((long long) nx * ny > (long long) INT_MAX - 2048) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %dx%d pixels do not fit an int", who, nx, ny);
    if (wsize != 3 && wsize != 5 && wsize != 7) return ofx_fail(ctx, OFX_ERR_ARG, "%s: wsize = %d (3, 5 or 7)", who, wsize);
    if (wsize / 2 > (nx < ny ? nx : ny))
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: half a window of %d does not fit %dx%d (one reflection per border)", who, wsize, nx, ny);
    for (int g = 0; g < n; g++) {
        if (!d_flo_in[g] || !d_flo_out[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        if (reinterpret_cast<uintptr_t>(d_flo_in[g]) % sizeof(float2) || reinterpret_cast<uintptr_t>(d_flo_out[g]) % sizeof(float2))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a payload of slot %d is not 8-byte aligned", who, g);
        if (d_flo_out[g] == d_flo_in[g])
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the destination of slot %d is the payload that the slot reads", who, g);
    }
    const size_t px = (size_t) nx * ny;
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxMedianSlots S = {};
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *in, *occ, *out;
            OFX_TRY(ofx_stage_in(ctx, d_flo_in[g], px * sizeof(float2), true, &in));
            OFX_TRY(ofx_stage_in(ctx, d_occ ? d_occ[g] : nullptr, px, true, &occ));
            OFX_TRY(ofx_stage_in(ctx, d_flo_out[g], px * sizeof(float2), false, &out));
            S.in[z] = in;
            S.occ[z] = static_cast<const unsigned char *>(occ);
            S.out[z] = out;
        }
        OFX_TRY(op_flow_median(ctx, 4, wsize, cnt, S, nx, ny));
        for (int z = 0; z < cnt; z++) OFX_TRY(ofx_stage_out(ctx, d_flo_out[g0 + z], S.out[z], px * sizeof(float2)));
    }
    return OFX_OK;
}
