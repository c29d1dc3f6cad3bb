// ofx_compose.hip -- .flo payloads composed along a sequence: one step (ofx_flow_compose_dev), the accumulated payloads 0 -> 1, 0 -> 2,
// ... of a chain of steps (ofx_flow_accumulate_dev) and sparse point tracks kept in double (ofx_flow_tracks_dev): the trajectories
// of Sundaram, Brox, Keutzer, "Dense point trajectories by GPU-accelerated large displacement optical flow" (ECCV 2010) -- follow a
// point through the step flows, sample each flow at the sub-pixel position reached, stop where the consistency map flags it.
//
// All arithmetic in double, every operation rounded (the build's -ffp-contract=off), association as written in include/ofx.h:
//     inside(x, y)     = 0 <= x <= nx - 1 and 0 <= y <= ny - 1                        (NaN and Inf fail it, before any int cast)
//     sample(S, x, y)  = bicubic_interpolation_at_color(S, x, y, nx, ny, 2, 0 / 1, false): flow_check's sample (ofx_flow.hip), both
//                        channels of a tap in one 8-byte load
//     flagged(M, x, y) = a non-zero byte among the up to four map pixels around an inside position; false without a map
// These three and advance() are ofx_advance.h's, shared with ofx_tracks.hip.
// Pure functions of the float payloads, the byte maps and the double query points: the same bytes in every storage precision.
#include "ofx_advance.h"
#include "ofx_device.h"
#include "ofx_ops.h"
#include "ofx_pairs.h"

#include <climits>
#include <cstdint>
#include <vector>

// ---- the shape of a workgroup ----------------------------------------------------------------------------------------------------
// 32 x 8 pixels as in ofx_apply.hip, a wave = two rows of 32: the centre vectors are one float2 per lane, 256 contiguous bytes per
// row, and the 16 float2 taps of neighbouring pixels of a coherent flow share cache lines -- the global gather path of k_flow_warp.
// There is no LDS tile of the step payload: k_flow_warp's box-and-tile staging measured 3 % BEHIND these gathers at 1920 x 1080
// (464 against 448 us per step of 16 sequences) -- the kernel is bound by its double arithmetic, not by the taps.
#define CP_BX 32
#define CP_BY 8
#define CP_NT (CP_BX * CP_BY)
#define CP_RW (CP_BX / 4 + 1)                    // words of LDS per block row of the map: 32 bytes at the run's address mod 4

struct OfxComposeSlots {
    const float2        *ab[OFX_MAX_GROUP];      // NULL: the zero flow               (may be the slot's ac: no __restrict__)
    const unsigned char *occ_ab[OFX_MAX_GROUP];  // NULL: all valid                   (may be the slot's occ_ac)
    const float2        *bc[OFX_MAX_GROUP];
    const unsigned char *occ_bc[OFX_MAX_GROUP];  // NULL: no map
    float2              *ac[OFX_MAX_GROUP];
    unsigned char       *occ_ac[OFX_MAX_GROUP];  // NULL: the map is not wanted
};

// ---- one step, dense --------------------------------------------------------------------------------------------------------------
//     (U, V) = ab[i][j] (zero without ab);  m = occ_ab[i][j] (0 without it)
//     m != 0 or !inside(j + U, i + V):                 ac = ab bit for bit, occ_ac = 255
//     f = flagged(occ_bc, j + U, i + V);  (bu, bv) = sample(bc, j + U, i + V);  Un = (float) (U + bu);  Vn = (float) (V + bv)
//     f or !inside(j + Un, i + Vn):                    ac = ab bit for bit, occ_ac = 255
//     otherwise:                                       ac = (Un, Vn), occ_ac = 0
// Slot z = blockIdx.y, tile blockIdx.x.  A pixel reads only its own element of ab and occ_ab, before the block's barrier, and the
// block writes only its own pixels' elements of ac and occ_ac behind it: ac == ab and occ_ac == occ_ab are safe.  The map goes out
// as k_flow_warp stores byte frames: block row r is a run of bytes of the map's row, laid into LDS at the run's address mod 4, so
// that an LDS word IS an aligned 32-bit word of the map; a word wholly inside the run is one store, the words across its two ends
// go out byte by byte.  No byte outside the map is written, and a slot without occ_ac skips the LDS and the barrier.
__global__ __launch_bounds__(CP_NT) void k_flow_compose(OfxComposeSlots S, int nx, int ny, int tiles_x)
{
    __shared__ unsigned s_out[CP_BY * CP_RW];
    const int z = blockIdx.y, tid = threadIdx.x;
    const int tby = (int) blockIdx.x / tiles_x, tbx = (int) blockIdx.x - tby * tiles_x;
    const int i0 = tby * CP_BY, j0 = tbx * CP_BX;
    const int tx = tid & (CP_BX - 1), ty = tid / CP_BX;
    const int i = i0 + ty, j = j0 + tx;
    const bool in = j < nx && i < ny;
    const float2 *ab = S.ab[z];
    const unsigned char *occ_ab = S.occ_ab[z];
    unsigned char *occ_ac = S.occ_ac[z];
    unsigned char lost = 0;
    if (in) {
        const size_t p = (size_t) i * nx + j;
        float2 o = make_float2(0.0f, 0.0f);
        if (ab) o = ab[p];
        const double U = (double) o.x, V = (double) o.y;
        const double x = (double) j + U, y = (double) i + V;
        lost = 255;
        if (!(occ_ab && occ_ab[p] != 0) && cp_inside(x, y, nx, ny)) {
            const bool f = cp_flagged(S.occ_bc[z], x, y, nx);
            const double2 b = cp_sample(S.bc[z], x, y, nx, ny);
            const float Un = (float) (U + b.x), Vn = (float) (V + b.y);
            if (!f && cp_inside((double) j + (double) Un, (double) i + (double) Vn, nx, ny)) {
                o = make_float2(Un, Vn);
                lost = 0;
            }
        }
        S.ac[z][p] = o;
    }
    if (!occ_ac) return;                                                     // the same in every thread of the block
    const int cols = min(CP_BX, nx - j0);                                    // bytes of a block row's run
    if (in) {
        const int a = (int) (reinterpret_cast<uintptr_t>(occ_ac + (size_t) i * nx + j0) & 3u);
        reinterpret_cast<unsigned char *>(s_out + ty * CP_RW)[a + tx] = lost;
    }
    __syncthreads();
    if (tid < CP_BY * CP_RW) {
        const int r = tid / CP_RW, ww = tid - r * CP_RW;
        if (i0 + r < ny) {
            unsigned char *d = occ_ac + (size_t) (i0 + r) * nx + j0;
            const int a = (int) (reinterpret_cast<uintptr_t>(d) & 3u);
            const int b0 = 4 * ww - a;                                       // the word's first byte within the run
            if (b0 < cols && b0 + 4 > 0) {
                const unsigned w = s_out[tid];
                if (b0 >= 0 && b0 + 4 <= cols) {
                    *reinterpret_cast<unsigned *>(d + b0) = w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (b0 + k >= 0 && b0 + k < cols) d[b0 + k] = (unsigned char) (w >> (8 * k));      // little endian
                }
            }
        }
    }
}

// ---- sparse tracks ----------------------------------------------------------------------------------------------------------------
// One launch marches all steps; a thread owns a point, sequence q = q0 + blockIdx.y.  The pointers live in one device table T of
// 2 n_seq n_steps + 3 n_seq entries: the step payloads [q * n_steps + t], their maps (NULL entries: no map), then xy0[q], xy[q],
// len[q].  has_occ = 0: no map at all, the second part is not read.
//     p_0 = xy0;  !inside(p_0): len = -1, every p_t = p_0
//     alive: flagged(occ_t, p_t) -> lost;  q = p_t + sample(step_t, p_t);  !inside(q) -> lost;  else p_{t+1} = q
//     the first lost step t: len = t, every later position repeats p_t;  a survivor: len = n_steps
// Positions are loaded and stored as doubles, one at a time: 8-byte alignment is all they need, and a NaN start keeps its bits.
__global__ __launch_bounds__(256) void k_flow_tracks(const void *const *__restrict__ T, int n_seq, int n_steps, int n_pts, int q0,
                                                     int has_occ, int nx, int ny)
{
    const int k = (int) (blockIdx.x * 256u + threadIdx.x);
    if (k >= n_pts) return;
    const int q = q0 + (int) blockIdx.y;
    const size_t ns = (size_t) n_seq * n_steps;
    const void *const *flo = T + (size_t) q * n_steps;
    const void *const *occ = T + ns + (size_t) q * n_steps;
    const double *xy0 = static_cast<const double *>(T[2 * ns + q]);
    double *xy = static_cast<double *>(const_cast<void *>(T[2 * ns + n_seq + q]));
    int *len = static_cast<int *>(const_cast<void *>(T[2 * ns + 2 * (size_t) n_seq + q]));
    double x = xy0[2 * (size_t) k], y = xy0[2 * (size_t) k + 1];
    xy[2 * (size_t) k] = x;
    xy[2 * (size_t) k + 1] = y;
    bool alive = cp_inside(x, y, nx, ny);
    int l = alive ? n_steps : -1;
    for (int t = 0; t < n_steps; t++) {
        if (alive) {
            const unsigned char *M = has_occ ? static_cast<const unsigned char *>(occ[t]) : nullptr;
            if (!cp_advance(static_cast<const float2 *>(flo[t]), M, x, y, nx, ny)) { alive = false; l = t; }
        }
        const size_t o = 2 * ((size_t) (t + 1) * n_pts + k);
        xy[o] = x;
        xy[o + 1] = y;
    }
    len[k] = l;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// One launch for slots <= OFX_MAX_GROUP slots; the pointers are memory of the context's GPU.
static int op_flow_compose(ofx_ctx *ctx, int slots, const OfxComposeSlots &S, int nx, int ny)
{
    const int tx = ofx_cdiv(nx, CP_BX), ty = ofx_cdiv(ny, CP_BY);
    hipLaunchKernelGGL(k_flow_compose, dim3(tx * ty, slots), dim3(CP_NT), 0, ctx->stream, S, nx, ny, tx);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

static int cp_check_size(ofx_ctx *ctx, const char *who, int nx, int ny)
{
    if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: flow field %dx%d too small", who, nx, ny);
    if ((long long) nx * ny > (long long) INT_MAX - 2048) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %dx%d pixels do not fit an int", who, nx, ny);
    return OFX_OK;
}
static bool cp_misaligned(const void *p, size_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

// One slot of one launch: the six buffers staged where they are not on the context's GPU.  ab / occ_ab are device pointers already
// where `local_ab` (the accumulated state of the step before).
struct CpStaged { void *ac, *occ_ac; };
static int cp_stage_slot(ofx_ctx *ctx, OfxComposeSlots &S, int z, const void *ab, const void *occ_ab, bool local_ab, const void *bc,
                         const void *occ_bc, void *ac, void *occ_ac, size_t px, CpStaged &st)
{
    void *a = const_cast<void *>(ab), *oa = const_cast<void *>(occ_ab), *b, *ob;
    st.ac = ac;
    st.occ_ac = occ_ac;
    // in place: the destination's stage is filled and serves as the source too
    const bool flo_inplace = !local_ab && ab && ab == ac, occ_inplace = !local_ab && occ_ab && occ_ab == occ_ac;
    if (!local_ab) {
        OFX_TRY(ofx_stage_in(ctx, ab, px * sizeof(float2), true, &a));
        OFX_TRY(ofx_stage_in(ctx, occ_ab, px, true, &oa));
    }
    OFX_TRY(ofx_stage_in(ctx, bc, px * sizeof(float2), true, &b));
    OFX_TRY(ofx_stage_in(ctx, occ_bc, px, true, &ob));
    if (flo_inplace) st.ac = a; else OFX_TRY(ofx_stage_in(ctx, ac, px * sizeof(float2), false, &st.ac));
    if (occ_inplace) st.occ_ac = oa; else OFX_TRY(ofx_stage_in(ctx, occ_ac, px, false, &st.occ_ac));
    S.ab[z] = static_cast<const float2 *>(a);
    S.occ_ab[z] = static_cast<const unsigned char *>(oa);
    S.bc[z] = static_cast<const float2 *>(b);
    S.occ_bc[z] = static_cast<const unsigned char *>(ob);
    S.ac[z] = static_cast<float2 *>(st.ac);
    S.occ_ac[z] = static_cast<unsigned char *>(st.occ_ac);
    return OFX_OK;
}

extern "C" int ofx_flow_compose_dev(ofx_ctx *ctx, int n, const void *const *d_flo_ab, const void *const *d_occ_ab,
                                    const void *const *d_flo_bc, const void *const *d_occ_bc, void *const *d_flo_ac,
                                    void *const *d_occ_ac, int nx, int ny)
{
    OFX_ENTER(ctx);
    const char *who = "flow_compose";
    if (!d_flo_bc || !d_flo_ac) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    if (n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n = %d (at least 1)", who, n);
    OFX_TRY(cp_check_size(ctx, who, nx, ny));
    for (int g = 0; g < n; g++) {
        if (!d_flo_bc[g] || !d_flo_ac[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        if (cp_misaligned(d_flo_bc[g], sizeof(float2)) || cp_misaligned(d_flo_ac[g], sizeof(float2)) ||
            (d_flo_ab && cp_misaligned(d_flo_ab[g], sizeof(float2))))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a payload of slot %d is not 8-byte aligned", who, g);
        if (d_flo_ac[g] == d_flo_bc[g] || (d_occ_ac && d_occ_bc && d_occ_ac[g] && d_occ_ac[g] == d_occ_bc[g]))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the destination of slot %d is the step that the slot reads at other pixels", who, g);
    }
    const size_t px = (size_t) nx * ny;
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxComposeSlots S = {};
        CpStaged st[OFX_MAX_GROUP];
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            OFX_TRY(cp_stage_slot(ctx, S, z, d_flo_ab ? d_flo_ab[g] : nullptr, d_occ_ab ? d_occ_ab[g] : nullptr, false, d_flo_bc[g],
                                  d_occ_bc ? d_occ_bc[g] : nullptr, d_flo_ac[g], d_occ_ac ? d_occ_ac[g] : nullptr, px, st[z]));
        }
        OFX_TRY(op_flow_compose(ctx, cnt, S, nx, ny));
        for (int z = 0; z < cnt; z++) {
            OFX_TRY(ofx_stage_out(ctx, d_flo_ac[g0 + z], st[z].ac, px * sizeof(float2)));
            if (st[z].occ_ac) OFX_TRY(ofx_stage_out(ctx, d_occ_ac[g0 + z], st[z].occ_ac, px));
        }
    }
    return OFX_OK;
}

// what the two chain entries refuse about their step tables, before any work
static int cp_check_steps(ofx_ctx *ctx, const char *who, int n_seq, int n_steps, const void *const *d_flo_step, int nx, int ny)
{
    if (!d_flo_step) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    if (n_seq < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_seq = %d (at least 1)", who, n_seq);
    if (n_steps < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_steps = %d (at least 1)", who, n_steps);
    OFX_TRY(cp_check_size(ctx, who, nx, ny));
    for (int q = 0; q < n_seq; q++)
        for (int t = 0; t < n_steps; t++) {
            const void *p = d_flo_step[(size_t) q * n_steps + t];
            if (!p) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (step %d of sequence %d)", who, t, q);
            if (cp_misaligned(p, sizeof(float2)))
                return ofx_fail(ctx, OFX_ERR_ARG, "%s: step payload %d of sequence %d is not 8-byte aligned", who, t, q);
        }
    return OFX_OK;
}

// n_steps launches of k_flow_compose per chunk of OFX_MAX_GROUP sequences: step t reads the accumulated payload and the lost state
// that step t - 1 left on the device -- the caller's acc[q][t - 1] and occ_acc[q][t - 1], or their stages, or, where the caller
// wants no map, one workspace map per sequence that every step updates in place.
extern "C" int ofx_flow_accumulate_dev(ofx_ctx *ctx, int n_seq, int n_steps, const void *const *d_flo_step, const void *const *d_occ_step,
                                       void *const *d_flo_acc, void *const *d_occ_acc, int nx, int ny)
{
    OFX_ENTER(ctx);
    const char *who = "flow_accumulate";
    if (!d_flo_acc) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    OFX_TRY(cp_check_steps(ctx, who, n_seq, n_steps, d_flo_step, nx, ny));
    for (int q = 0; q < n_seq; q++)
        for (int t = 0; t < n_steps; t++) {
            const size_t e = (size_t) q * n_steps + t;
            if (!d_flo_acc[e]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (step %d of sequence %d)", who, t, q);
            if (cp_misaligned(d_flo_acc[e], sizeof(float2)))
                return ofx_fail(ctx, OFX_ERR_ARG, "%s: accumulated payload %d of sequence %d is not 8-byte aligned", who, t, q);
            for (int s = t; s < n_steps; s++) {
                const size_t f = (size_t) q * n_steps + s;
                if (d_flo_acc[e] == d_flo_step[f] || (d_occ_acc && d_occ_step && d_occ_acc[e] && d_occ_acc[e] == d_occ_step[f]))
                    return ofx_fail(ctx, OFX_ERR_ARG, "%s: destination %d of sequence %d is step %d that the chain still reads", who, t, q, s);
            }
        }
    const size_t px = (size_t) nx * ny;
    for (int q0 = 0; q0 < n_seq; q0 += OFX_MAX_GROUP) {
        const int cnt = n_seq - q0 < OFX_MAX_GROUP ? n_seq - q0 : OFX_MAX_GROUP;
        const void *prev[OFX_MAX_GROUP] = {}, *prev_occ[OFX_MAX_GROUP] = {};
        unsigned char *ws[OFX_MAX_GROUP] = {};
        for (int t = 0; t < n_steps; t++) {
            OfxComposeSlots S = {};
            CpStaged st[OFX_MAX_GROUP];
            void *occ_dst[OFX_MAX_GROUP];
            for (int z = 0; z < cnt; z++) {
                const size_t e = (size_t) (q0 + z) * n_steps + t;
                occ_dst[z] = d_occ_acc ? d_occ_acc[e] : nullptr;
                void *occ = occ_dst[z];
                if (!occ && t + 1 < n_steps) {                              // the lost state still travels to the next step
                    if (!ws[z]) OFX_TRY(ofx_alloc(ctx, px, &ws[z]));
                    occ = ws[z];
                }
                OFX_TRY(cp_stage_slot(ctx, S, z, prev[z], prev_occ[z], true, d_flo_step[e], d_occ_step ? d_occ_step[e] : nullptr,
                                      d_flo_acc[e], occ, px, st[z]));
            }
            OFX_TRY(op_flow_compose(ctx, cnt, S, nx, ny));
            for (int z = 0; z < cnt; z++) {
                const size_t e = (size_t) (q0 + z) * n_steps + t;
                OFX_TRY(ofx_stage_out(ctx, d_flo_acc[e], st[z].ac, px * sizeof(float2)));
                if (occ_dst[z]) OFX_TRY(ofx_stage_out(ctx, occ_dst[z], st[z].occ_ac, px));
                prev[z] = st[z].ac;
                prev_occ[z] = st[z].occ_ac;
            }
        }
    }
    return OFX_OK;
}

extern "C" int ofx_flow_tracks_dev(ofx_ctx *ctx, int n_seq, int n_steps, const void *const *d_flo_step, const void *const *d_occ_step,
                                   int n_pts, const void *const *d_xy0, void *const *d_xy, void *const *d_len, int nx, int ny)
{
    OFX_ENTER(ctx);
    const char *who = "flow_tracks";
    if (!d_xy0 || !d_xy || !d_len) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    OFX_TRY(cp_check_steps(ctx, who, n_seq, n_steps, d_flo_step, nx, ny));
    if (n_pts < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_pts = %d (at least 1)", who, n_pts);
    for (int q = 0; q < n_seq; q++) {
        if (!d_xy0[q] || !d_xy[q] || !d_len[q]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (sequence %d)", who, q);
        if (cp_misaligned(d_xy0[q], sizeof(double)) || cp_misaligned(d_xy[q], sizeof(double)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the positions of sequence %d are not 8-byte aligned", who, q);
        if (cp_misaligned(d_len[q], sizeof(int))) return ofx_fail(ctx, OFX_ERR_ARG, "%s: the lengths of sequence %d are not 4-byte aligned", who, q);
    }
    const size_t px = (size_t) nx * ny, ns = (size_t) n_seq * n_steps;
    const size_t xy0_bytes = (size_t) n_pts * 2 * sizeof(double), xy_bytes = xy0_bytes * ((size_t) n_steps + 1);
    bool has_occ = false;
    std::vector<const void *> T(2 * ns + 3 * (size_t) n_seq, nullptr);
    for (size_t e = 0; e < ns; e++) {
        void *p;
        OFX_TRY(ofx_stage_in(ctx, d_flo_step[e], px * sizeof(float2), true, &p));
        T[e] = p;
        OFX_TRY(ofx_stage_in(ctx, d_occ_step ? d_occ_step[e] : nullptr, px, true, &p));
        T[ns + e] = p;
        has_occ = has_occ || p;
    }
    for (int q = 0; q < n_seq; q++) {
        void *p;
        OFX_TRY(ofx_stage_in(ctx, d_xy0[q], xy0_bytes, true, &p));
        T[2 * ns + q] = p;
        OFX_TRY(ofx_stage_in(ctx, d_xy[q], xy_bytes, false, &p));
        T[2 * ns + n_seq + q] = p;
        OFX_TRY(ofx_stage_in(ctx, d_len[q], (size_t) n_pts * sizeof(int), false, &p));
        T[2 * ns + 2 * (size_t) n_seq + q] = p;
    }
    // the table is host memory of this call: its upload is awaited before the call returns, the march is not
    const void **dT;
    OFX_TRY(ofx_alloc(ctx, T.size(), &dT));
    OFX_HIP(ctx, hipMemcpyAsync(dT, T.data(), T.size() * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    OFX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int per = 32768;                                                   // sequences per launch: a grid's y extent
    for (int q0 = 0; q0 < n_seq; q0 += per) {
        const int cnt = n_seq - q0 < per ? n_seq - q0 : per;
        hipLaunchKernelGGL(k_flow_tracks, dim3(ofx_cdiv(n_pts, 256), cnt), dim3(256), 0, ctx->stream, dT, n_seq, n_steps, n_pts, q0,
                           has_occ ? 1 : 0, nx, ny);
        OFX_LAUNCH_CHECK(ctx);
    }
    for (int q = 0; q < n_seq; q++) {
        OFX_TRY(ofx_stage_out(ctx, d_xy[q], T[2 * ns + n_seq + q], xy_bytes));
        OFX_TRY(ofx_stage_out(ctx, d_len[q], T[2 * ns + 2 * (size_t) n_seq + q], (size_t) n_pts * sizeof(int)));
    }
    return OFX_OK;
}
