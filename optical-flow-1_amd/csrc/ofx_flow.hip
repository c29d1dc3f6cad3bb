// ofx_flow.hip -- operators on .flo payloads: the forward-backward consistency check (Sundaram, Brox, Keutzer, ECCV 2010).
//
// A payload is what every *_dev solver writes: nx * ny interleaved (u, v) float32.  Given the payload F of A -> B (on A's grid)
// and the payload B of B -> A (on B's grid), the forward map at row i, column j is, in double, every operation rounded (the
// build's -ffp-contract=off), association as written:
//     u = F[i][j].x, v = F[i][j].y;  xt = j + u, yt = i + v
//     255  unless 0 <= xt <= nx - 1 and 0 <= yt <= ny - 1             (NaN and Inf land here, before any int cast)
//     (bu, bv) = bicubic_interpolation_at_color(B, xt, yt, nx, ny, 2, k = 0 / 1, border_out = false)
//     du = u + bu, dv = v + bv
//     0 if du du + dv dv <= alpha ((u u + v v) + (bu bu + bv bv)) + beta, else 255       (a NaN anywhere: 255)
// The backward map is the same with the payloads exchanged.  A pure function of the two float payloads: the same bytes in
// every storage precision and mode.
#include "ofx_device.h"
#include "ofx_ops.h"
#include "ofx_pairs.h"

#include <climits>
#include <cmath>

// One pixel of one slot.  The sample is k_bicubic_at_color's for nz = 2, both channels of a tap in one 8-byte load.
OFX_DEV unsigned flow_check(const float2 *__restrict__ F, const float2 *__restrict__ B, int i, int nx, int ny, double alpha,
                            double beta)
{
    const int row = i / nx, col = i - row * nx;
    const double2 c = ldw2(F + i);
    const double u = c.x, v = c.y;
    const double xt = (double) col + u, yt = (double) row + v;
    if (!(xt >= 0.0 && xt <= (double) (nx - 1) && yt >= 0.0 && yt <= (double) (ny - 1))) return 255u;
    const BicubicTaps t = bicubic_taps(xt, yt, nx, ny);
    double c1[4], c2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double2 v0 = ldw2(B + (size_t) t.row[0] * nx + t.col[k]);
        const double2 v1 = ldw2(B + (size_t) t.row[1] * nx + t.col[k]);
        const double2 v2 = ldw2(B + (size_t) t.row[2] * nx + t.col[k]);
        const double2 v3 = ldw2(B + (size_t) t.row[3] * nx + t.col[k]);
        c1[k] = cubic_cell(v0.x, v1.x, v2.x, v3.x, t.fy);
        c2[k] = cubic_cell(v0.y, v1.y, v2.y, v3.y, t.fy);
    }
    const double bu = cubic_cell(c1[0], c1[1], c1[2], c1[3], t.fx);
    const double bv = cubic_cell(c2[0], c2[1], c2[2], c2[3], t.fx);
    const double du = u + bu, dv = v + bv;
    const double lhs = du * du + dv * dv;
    const double rhs = alpha * ((u * u + v * v) + (bu * bu + bv * bv)) + beta;
    return lhs <= rhs ? 0u : 255u;
}

// Slot z = blockIdx.y (a pair and a direction).  A block serves 1024 pixels under two lane mappings, as k_occ_seq_out does.
// Check: pixel = 256 k + lane, k = 0 .. 3 -- the centre vectors are one float2 per lane, 512 contiguous bytes per wave and
// load, and neighbouring lanes gather neighbouring taps (flows of a few pixels: the 16 taps of a wave fall into the rows its
// centre loads just touched, L1 / L2 serve them).  The verdicts go through 1 KiB of LDS.  Map: a lane owns one ALIGNED 32-bit
// word of the destination, i.e. the pixels 4 w - a .. 4 w - a + 3 where a = address of the map mod 4 (a map needs no
// alignment); a word wholly inside the map is one store, the up to two words across its ends go out byte by byte.  No byte
// outside [occ, occ + n) is written.
__global__ __launch_bounds__(256) void k_flow_consistency(OfxFlowSlots S, int nx, int ny, int n, double alpha, double beta)
{
    __shared__ unsigned verdict[256];
    unsigned char *vb = reinterpret_cast<unsigned char *>(verdict);
    const int z = blockIdx.y;
    const float2 *__restrict__ F = S.f[z];
    const float2 *__restrict__ B = S.b[z];
    unsigned char *__restrict__ occ = S.occ[z];
    const int a = (int) (reinterpret_cast<uintptr_t>(occ) & 3u);
    const int base = (int) (blockIdx.x * 1024u) - a;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int t = 256 * k + (int) threadIdx.x;
        const int i = base + t;
        vb[t] = (unsigned char) ((i >= 0 && i < n) ? flow_check(F, B, i, nx, ny, alpha, beta) : 0u);
    }
    __syncthreads();
    const int i0 = base + 4 * (int) threadIdx.x;
    if (i0 >= n) return;
    const unsigned w = verdict[threadIdx.x];                 // little endian: byte k of the word is pixel i0 + k
    if (i0 >= 0 && i0 + 3 < n) {
        *reinterpret_cast<unsigned *>(occ + i0) = w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i0 + k >= 0 && i0 + k < n) occ[i0 + k] = (unsigned char) (w >> (8 * k));
    }
}

int op_flow_consistency_check(ofx_ctx *ctx, const char *who, int nx, int ny, double alpha, double beta)
{
    if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: flow field %dx%d too small", who, nx, ny);
    if ((long long) nx * ny > (long long) INT_MAX - 2048) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %dx%d pixels do not fit an int", who, nx, ny);
    if (!std::isfinite(alpha) || !std::isfinite(beta) || alpha < 0.0 || beta < 0.0)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: alpha = %g, beta = %g (both must be finite and >= 0)", who, alpha, beta);
    return OFX_OK;
}

// slots <= OFX_MAX_GROUP maps in one launch: slot z checks payload f[z] against b[z] into occ[z]
int op_flow_consistency(ofx_ctx *ctx, int slots, const void *const *f, const void *const *b, void *const *occ, int nx, int ny,
                        double alpha, double beta)
{
    if (slots < 1 || slots > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "flow_consistency: %d slots in one launch", slots);
    OfxFlowSlots S = {};
    for (int z = 0; z < slots; z++) {
        S.f[z] = static_cast<const float2 *>(f[z]);
        S.b[z] = static_cast<const float2 *>(b[z]);
        S.occ[z] = static_cast<unsigned char *>(occ[z]);
    }
    const int n = nx * ny;
    hipLaunchKernelGGL(k_flow_consistency, dim3(ofx_cdiv(n + 3, 1024), slots), dim3(256), 0, ctx->stream, S, nx, ny, n, alpha, beta);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

extern "C" int ofx_flow_consistency_dev(ofx_ctx *ctx, int n_pairs, const void *const *d_flo_fwd, const void *const *d_flo_bwd,
                                        void *const *d_occ_fwd, void *const *d_occ_bwd, int nx, int ny, double alpha, double beta)
{
    OFX_ENTER(ctx);
    if (!d_flo_fwd || !d_flo_bwd || !d_occ_fwd || !d_occ_bwd) return ofx_fail(ctx, OFX_ERR_ARG, "flow_consistency: NULL pointer table");
    if (n_pairs < 1) return ofx_fail(ctx, OFX_ERR_ARG, "flow_consistency: n_pairs = %d (at least 1)", n_pairs);
    OFX_TRY(op_flow_consistency_check(ctx, "flow_consistency", nx, ny, alpha, beta));
    for (int g = 0; g < n_pairs; g++) {
        if (!d_flo_fwd[g] || !d_flo_bwd[g] || !d_occ_fwd[g] || !d_occ_bwd[g])
            return ofx_fail(ctx, OFX_ERR_ARG, "flow_consistency: NULL pointer (pair %d)", g);
        if (reinterpret_cast<uintptr_t>(d_flo_fwd[g]) % sizeof(float2) || reinterpret_cast<uintptr_t>(d_flo_bwd[g]) % sizeof(float2))
            return ofx_fail(ctx, OFX_ERR_ARG, "flow_consistency: payload of pair %d is not 8-byte aligned", g);
    }
    // the kernel's pointer tables hold OFX_MAX_GROUP slots = both directions of OFX_MAX_GROUP / 2 pairs: one launch per chunk.
    // Memory of the context's GPU is used in place; a payload or a map that lives elsewhere (host memory, another GPU) goes
    // through the workspace, as the batch entries stage theirs (ofx_stage_in / ofx_stage_out).
    const size_t n = (size_t) nx * ny;
    const int per = OFX_MAX_GROUP / 2;
    for (int g0 = 0; g0 < n_pairs; g0 += per) {
        const int cnt = n_pairs - g0 < per ? n_pairs - g0 : per;
        const void *f[OFX_MAX_GROUP], *b[OFX_MAX_GROUP];
        void *occ[OFX_MAX_GROUP], *occ_in[OFX_MAX_GROUP];
        for (int g = 0; g < cnt; g++) {
            void *fwd, *bwd;
            OFX_TRY(ofx_stage_in(ctx, d_flo_fwd[g0 + g], n * sizeof(float2), true, &fwd));
            OFX_TRY(ofx_stage_in(ctx, d_flo_bwd[g0 + g], n * sizeof(float2), true, &bwd));
            f[g] = fwd;       b[g] = bwd;       occ_in[g] = d_occ_fwd[g0 + g];
            f[cnt + g] = bwd; b[cnt + g] = fwd; occ_in[cnt + g] = d_occ_bwd[g0 + g];
        }
        for (int z = 0; z < 2 * cnt; z++) OFX_TRY(ofx_stage_in(ctx, occ_in[z], n, false, &occ[z]));
        OFX_TRY(op_flow_consistency(ctx, 2 * cnt, f, b, occ, nx, ny, alpha, beta));
        for (int z = 0; z < 2 * cnt; z++) OFX_TRY(ofx_stage_out(ctx, occ_in[z], occ[z], n));
    }
    return OFX_OK;
}
