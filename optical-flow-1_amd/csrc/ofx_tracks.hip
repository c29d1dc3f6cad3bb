// ofx_tracks.hip -- where point tracks start, and dense point trajectories over device-resident clips: the seeding and re-seeding of
// Sundaram, Brox, Keutzer, "Dense point trajectories by GPU-accelerated large displacement optical flow" (ECCV 2010).  Points are
// placed on a grid of step x step cells and kept where the smaller eigenvalue of the smoothed structure tensor reaches a fraction of
// its image mean (ofx_track_structure_dev, ofx_track_seed_dev); a clip is tracked by the advance rule of ofx_advance.h and every new
// frame is re-seeded in the cells that no live track occupies (ofx_track_sequence_dev).
//
// All arithmetic in double, every operation rounded (the build's -ffp-contract=off), association as written in include/ofx.h:
//     f        = (double) sample                         the context's "input" kind under "input_pitch" (ldw, ofx_device.h)
//     (gx, gy) = centered_gradient(f)                    src/operators.cpp, nz = 1: 0.5 * (f[right] - f[left]), indices clamped
//     a = gx * gx;  b = gx * gy;  c = gy * gy
//     A, B, C  = gaussian(a | b | c, rho)                src/operators.cpp:506-624, reflecting boundary, rows then columns
//     d = A - C;  e = B + B;  r = sqrt(d * d + e * e);  lam2 = 0.5 * ((A + C) - r)
//     mean     = sum64(sum64 of every row of lam2) / (double) (nx * ny)
// Pure functions of the samples, the floats, the map bytes and the doubles: the same bytes in every storage precision.
#include "ofx_advance.h"
#include "ofx_device.h"
#include "ofx_ops.h"
#include "ofx_pairs.h"
#include "ofx_sum64.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <set>

// ---- the structure kernel ---------------------------------------------------------------------------------------------------------
// One workgroup of TK_NT threads writes a TK_W x TK_H tile of lam2 and reads the frame alone: no product plane and no smoothed plane
// reaches memory.  With R = size - 1 the radius of the Gaussian:
//     s_f   the frame tile with a halo of R + 1 = size cells (R taps and 1 for the gradient), widened to double; cell t of the
//           extended row or column holds image index reflect(t) (t < 0 -> -t, t >= n -> 2 n - 1 - t: the Gaussian's boundary)
//     s_p   ONE product plane (a, then b, then c) on the tile with a halo of R: the gradient of the image pixel that a cell stands
//           for.  In the reflected zones the image's right neighbour is the cell to the LEFT and the other way round, and the
//           clamped neighbour of the image's border pixel is a cell that holds the same sample; the only cell whose clamped
//           neighbour is itself is image index 0.
//     s_m   the row pass of that plane on all TK_H + 2 R rows: a halo row is the row pass of the image row it reflects, the same
//           sums in the same order as the reference's whole-plane row pass
// and the column pass leaves A, B and C of a thread's TK_Q pixels in registers.  Three rounds of product / row pass / column
// pass, two barriers each.  R <= RMAX is a run-time value; RMAX sizes the LDS: 5 (rho below 1.2) takes 73 120 bytes, two
// workgroups per CU by the LDS and by the 2048 threads of a CU; OFX_TRACK_MAX_SIZE - 1 = 10 takes 98 720 bytes, one workgroup
// per CU.  The tile is the largest that leaves two workgroups of the common radius in the 160 KiB of a CU.
#define TK_W 64
#define TK_H 32
#ifndef TK_NT
#define TK_NT 1024                               // measured against 256 and 512: the waves hide the LDS latency of the passes
#endif
#define TK_Q (TK_W * TK_H / TK_NT)               // pixels per thread: its column, rows TK_NT / TK_W apart
#define TK_RS (TK_NT / TK_W)
#define TK_RSMALL 5
#define TK_RBIG (OFX_TRACK_MAX_SIZE - 1)

struct OfxTrkFrames {
    const void *src[OFX_MAX_GROUP];
    double     *lam2[OFX_MAX_GROUP];
    double     *mean[OFX_MAX_GROUP];             // NULL: not wanted
};

OFX_DEV int tk_reflect(int t, int n)             // ... then clamped: cells that no output depends on stay inside the frame
{
    t = t < 0 ? -t : (t >= n ? 2 * n - 1 - t : t);
    return t < 0 ? 0 : (t > n - 1 ? n - 1 : t);
}
// cells of the two samples of a centred difference at extended index t (cell c of an array whose neighbours are `s` apart):
// hi - lo is the image's f[min(j + 1, n - 1)] - f[max(j - 1, 0)] at j = reflect(t)
OFX_DEV void tk_diff_cells(int t, int n, int c, int s, int &hi, int &lo)
{
    if (t < 0 || t >= n) { hi = c - s; lo = c + s; }
    else { hi = t < n - 1 ? c + s : c; lo = t > 0 ? c - s : c; }
}

template <typename S, int RMAX>
__global__ __launch_bounds__(TK_NT) void k_trk_structure(OfxTrkFrames P, int nx, int ny, size_t pitch, int tiles_x, GaussTaps taps)
{
    __shared__ double s_f[(TK_H + 2 * RMAX + 2) * (TK_W + 2 * RMAX + 2)];
    __shared__ double s_p[(TK_H + 2 * RMAX) * (TK_W + 2 * RMAX)];
    __shared__ double s_m[(TK_H + 2 * RMAX) * TK_W];
    const int z = blockIdx.y, tid = threadIdx.x;
    const int tby = (int) blockIdx.x / tiles_x, tbx = (int) blockIdx.x - tby * tiles_x;
    const int i0 = tby * TK_H, j0 = tbx * TK_W;
    const int R = taps.size - 1;
    const int Wf = TK_W + 2 * R + 2, Hf = TK_H + 2 * R + 2, Wp = TK_W + 2 * R, Hp = TK_H + 2 * R;
    const char *__restrict__ src = static_cast<const char *>(P.src[z]);
    for (int k = tid; k < Wf * Hf; k += TK_NT) {
        const int r = k / Wf, c = k - r * Wf;
        const int i = tk_reflect(i0 - R - 1 + r, ny), j = tk_reflect(j0 - R - 1 + c, nx);
        s_f[k] = ldw(reinterpret_cast<const S *>(src + (size_t) i * pitch) + j);
    }
    __syncthreads();
    const int cx = tid & (TK_W - 1), ry = tid / TK_W;
    double acc[3][TK_Q];
#pragma unroll
    for (int p = 0; p < 3; p++) {
        for (int k = tid; k < Wp * Hp; k += TK_NT) {
            const int r = k / Wp, c = k - r * Wp;
            const int cf = (r + 1) * Wf + c + 1;
            int hi, lo;
            double g1, g2;
            if (p < 2) {
                tk_diff_cells(j0 - R + c, nx, cf, 1, hi, lo);
                g1 = 0.5 * (s_f[hi] - s_f[lo]);
            }
            if (p > 0) {
                tk_diff_cells(i0 - R + r, ny, cf, Wf, hi, lo);
                g2 = 0.5 * (s_f[hi] - s_f[lo]);
            }
            s_p[k] = p == 0 ? g1 * g1 : (p == 1 ? g1 * g2 : g2 * g2);
        }
        __syncthreads();
        for (int r = ry; r < Hp; r += TK_RS) {                               // row pass, :541-575
            const double *row = s_p + r * Wp + R + cx;
            double sum = taps.B[0] * row[0];
            for (int k = 1; k <= R; k++) sum += taps.B[k] * (row[-k] + row[k]);
            s_m[r * TK_W + cx] = sum;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TK_Q; q++) {                                     // column pass, :577-611
            const double *col = s_m + (ry + TK_RS * q + R) * TK_W + cx;
            double sum = taps.B[0] * col[0];
            for (int k = 1; k <= R; k++) sum += taps.B[k] * (col[-k * TK_W] + col[k * TK_W]);
            acc[p][q] = sum;
        }
    }
    const int j = j0 + cx;
    if (j >= nx) return;
    double *__restrict__ out = P.lam2[z];
#pragma unroll
    for (int q = 0; q < TK_Q; q++) {
        const int i = i0 + ry + TK_RS * q;
        if (i >= ny) break;
        const double A = acc[0][q], B = acc[1][q], C = acc[2][q];
        const double d = A - C, e = B + B;
        const double r = sqrt(d * d + e * e);
        out[(size_t) i * nx + j] = 0.5 * ((A + C) - r);
    }
}

// ---- the mean: sum64 (ofx_sum64.h) over the rows of sum64 over a row ---------------------------------------------------------------
// one wave per row of lam2: rows[z * ny + i]
__global__ __launch_bounds__(256) void k_trk_rowsum(OfxTrkFrames P, double *__restrict__ rows, int nx, int ny)
{
    const int z = blockIdx.y, i = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (i >= ny) return;                                                     // the same in all lanes of a wave
    const double s = tk_sum64(P.lam2[z] + (size_t) i * nx, nx);
    if ((threadIdx.x & 63) == 0) rows[(size_t) z * ny + i] = s;
}
// one wave per slot over its row sums
__global__ __launch_bounds__(64) void k_trk_mean(OfxTrkFrames P, const double *__restrict__ rows, int nx, int ny)
{
    const int z = blockIdx.x;
    const double s = tk_sum64(rows + (size_t) z * ny, ny);
    if (threadIdx.x == 0 && P.mean[z]) *P.mean[z] = s / (double) (nx * ny);
}

// ---- cells, occupancy, compaction -------------------------------------------------------------------------------------------------
// ncx x ncy cells of step x step pixels, cell e = cb * ncx + ca; its candidate is the pixel (ca * step + step / 2, cb * step +
// step / 2), none where that lies beyond the frame.  The occupancy map is one byte per cell; every writer stores 1.
// The seeds of a frame leave in cell order by a scan, never by atomics: k_trk_count counts the flags of every block of 256 cells,
// k_trk_scan turns the counts of a slot into offsets (one workgroup per slot) and settles how many seeds fit, k_trk_scatter
// evaluates the flags again, scans inside the block and stores.  Integer sums: the same from run to run.
struct OfxTrkSeed {
    const double        *lam2[OFX_MAX_GROUP];
    const double        *mean[OFX_MAX_GROUP];
    const double        *pts[OFX_MAX_GROUP];     // k_trk_mark: the occupying points of the seed entry, NULL: none
    double              *xy[OFX_MAX_GROUP];
    int                 *t0[OFX_MAX_GROUP];      // NULL (the seed entry): positions alone
    int                 *len[OFX_MAX_GROUP];
    int                 *count[OFX_MAX_GROUP];   // {slots used, seeds dropped}
    const float2        *flo[OFX_MAX_GROUP];     // k_trk_advance: the step and its map
    const unsigned char *map[OFX_MAX_GROUP];
};

OFX_DEV void tk_occupy(unsigned char *occ, double x, double y, int step, int ncx) { occ[(size_t) ((int) y / step) * ncx + (int) x / step] = 1; }

__global__ __launch_bounds__(256) void k_trk_mark(OfxTrkSeed P, unsigned char *__restrict__ occ, int n_occ, int nx, int ny, int step,
                                                  int ncx, int nc)
{
    const int z = blockIdx.y, k = (int) (blockIdx.x * 256u + threadIdx.x);
    if (k >= n_occ || !P.pts[z]) return;
    const double x = P.pts[z][2 * (size_t) k], y = P.pts[z][2 * (size_t) k + 1];
    if (cp_inside(x, y, nx, ny)) tk_occupy(occ + (size_t) z * nc, x, y, step, ncx);
}

// Step t of the clips of a launch: slot k < count[0] that lives (t0 + len > t: len is the survivor's value from birth on) moves by
// advance(); a loss sets len = t - t0; the position at frame t + 1 is written for every used slot, and a survivor occupies its cell.
__global__ __launch_bounds__(256) void k_trk_advance(OfxTrkSeed P, unsigned char *__restrict__ occ, int t, int cap, int nx, int ny,
                                                     int step, int ncx, int nc)
{
    const int z = blockIdx.y, k = (int) (blockIdx.x * 256u + threadIdx.x);
    if (k >= cap || k >= P.count[z][0]) return;
    const int t0 = P.t0[z][k];
    double *xy = P.xy[z];
    const size_t o = 2 * ((size_t) t * cap + k), o1 = 2 * ((size_t) (t + 1) * cap + k);
    double x = xy[o], y = xy[o + 1];
    if (t0 + P.len[z][k] > t) {
        if (cp_advance(P.flo[z], P.map[z], x, y, nx, ny)) tk_occupy(occ + (size_t) z * nc, x, y, step, ncx);
        else P.len[z][k] = t - t0;
    }
    xy[o1] = x;
    xy[o1 + 1] = y;
}

// is cell e the place of a seed?  A NaN in lam2 or in tau fails the comparison.
OFX_DEV bool tk_flag(const OfxTrkSeed &P, const unsigned char *__restrict__ occ, int z, int e, int nx, int ny, int step, int ncx, int nc,
                     double frac, int &x, int &y)
{
    if (e >= nc) return false;
    const int cb = e / ncx, ca = e - cb * ncx;
    x = ca * step + step / 2;
    y = cb * step + step / 2;
    if (x > nx - 1 || y > ny - 1 || occ[(size_t) z * nc + e]) return false;
    const double tau = frac * *P.mean[z];
    return P.lam2[z][(size_t) y * nx + x] >= tau;
}

// exclusive scan of v over the 256 threads of a workgroup, and the total; s_w: 4 ints of LDS, free again on return
OFX_DEV int tk_block_scan(int v, int *s_w, int &total)
{
    const int lane = (int) threadIdx.x & 63, w = (int) threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(x, d, 64);
        if (lane >= d) x += o;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < w) before += s_w[k];
        total += s_w[k];
    }
    __syncthreads();
    return before + x - v;
}

__global__ __launch_bounds__(256) void k_trk_count(OfxTrkSeed P, const unsigned char *__restrict__ occ, int *__restrict__ blk, int nb,
                                                   int nx, int ny, int step, int ncx, int nc, double frac)
{
    __shared__ int s_w[4];
    const int z = blockIdx.y, e = (int) (blockIdx.x * 256u + threadIdx.x);
    int x, y, total;
    tk_block_scan(tk_flag(P, occ, z, e, nx, ny, step, ncx, nc, frac, x, y) ? 1 : 0, s_w, total);
    if (threadIdx.x == 0) blk[(size_t) z * (nb + 1) + blockIdx.x] = total;
}
// blk[z]: nb counts -> nb offsets; entry nb: the slot's first free place (0 where `fresh`: the counts start here).  count[0] grows
// by the seeds that fit below cap, count[1] by the others.
__global__ __launch_bounds__(256) void k_trk_scan(OfxTrkSeed P, int *__restrict__ blk, int nb, int cap, int fresh)
{
    __shared__ int s_w[4];
    const int z = blockIdx.x;
    int *b = blk + (size_t) z * (nb + 1);
    int run = 0;
    for (int k0 = 0; k0 < nb; k0 += 256) {
        const int k = k0 + (int) threadIdx.x;
        const int v = k < nb ? b[k] : 0;
        int total;
        const int ex = tk_block_scan(v, s_w, total);
        if (k < nb) b[k] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) {
        const int base = fresh ? 0 : P.count[z][0], dropped = fresh ? 0 : P.count[z][1];
        const int fit = run < cap - base ? run : cap - base;
        b[nb] = base;
        P.count[z][0] = base + fit;
        P.count[z][1] = dropped + (run - fit);
    }
}
// the seeds of frame `birth`: slot k = base + (flags before the cell), stored below cap alone; with t0 / len (the sequence entry)
// the position goes to the frames 0 .. birth, t0 = birth and len = the survivor's last - birth
__global__ __launch_bounds__(256) void k_trk_scatter(OfxTrkSeed P, const unsigned char *__restrict__ occ, const int *__restrict__ blk,
                                                     int nb, int cap, int birth, int last, int nx, int ny, int step, int ncx, int nc,
                                                     double frac)
{
    __shared__ int s_w[4];
    const int z = blockIdx.y, e = (int) (blockIdx.x * 256u + threadIdx.x);
    const int *b = blk + (size_t) z * (nb + 1);
    int x, y, total;
    const bool flag = tk_flag(P, occ, z, e, nx, ny, step, ncx, nc, frac, x, y);
    const int ex = tk_block_scan(flag ? 1 : 0, s_w, total);
    if (!flag) return;
    const long long k = (long long) b[nb] + b[blockIdx.x] + ex;
    if (k >= cap) return;
    double *xy = P.xy[z];
    for (int f = 0; f <= birth; f++) {
        const size_t o = 2 * ((size_t) f * cap + (size_t) k);
        xy[o] = (double) x;
        xy[o + 1] = (double) y;
    }
    if (P.t0[z]) {
        P.t0[z][k] = birth;
        P.len[z][k] = last - birth;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static bool tk_misaligned(const void *p, size_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

// the refusals that the three entries share, before any work; leaves the Gaussian's taps
static int tk_check(ofx_ctx *ctx, const char *who, int nx, int ny, double rho, GaussTaps *taps)
{
    if (nx < 2 || ny < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: frame %dx%d too small", who, nx, ny);
    if ((long long) nx * ny > (long long) INT_MAX - 2048) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %dx%d pixels do not fit an int", who, nx, ny);
    if (!std::isfinite(rho) || !(rho > 0.0)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: rho = %g (finite, above 0)", who, rho);
    if (5.0 * rho + 1.0 >= (double) (OFX_TRACK_MAX_SIZE + 1) || ofx_gauss_taps(rho, taps) != OFX_OK || taps->size > OFX_TRACK_MAX_SIZE)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: rho = %g needs more than OFX_TRACK_MAX_SIZE = %d taps", who, rho, OFX_TRACK_MAX_SIZE);
    OFX_TRY(ofx_pitch_check(ctx, who, nx));
    if (taps->size >= nx || taps->size >= ny)
        return ofx_fail(ctx, OFX_ERR_SIGMA, "GaussianSmooth: sigma too large (radius %d, image %dx%d)", taps->size, nx, ny);
    return OFX_OK;
}
static int tk_check_seed(ofx_ctx *ctx, const char *who, int cap, double frac, int step)
{
    if (cap < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: cap = %d (at least 1)", who, cap);
    if (step < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: step = %d (at least 1)", who, step);
    if (!std::isfinite(frac) || !(frac >= 0.0)) return ofx_fail(ctx, OFX_ERR_ARG, "%s: frac = %g (finite, not below 0)", who, frac);
    return OFX_OK;
}

template <typename S>
static void tk_launch_structure(ofx_ctx *ctx, int slots, const OfxTrkFrames &P, int nx, int ny, size_t pitch, const GaussTaps &taps)
{
    const int tx = ofx_cdiv(nx, TK_W), ty = ofx_cdiv(ny, TK_H);
    const size_t pb = pitch ? pitch : (size_t) nx * sizeof(S);
    if (taps.size - 1 <= TK_RSMALL)
        hipLaunchKernelGGL((k_trk_structure<S, TK_RSMALL>), dim3(tx * ty, slots), dim3(TK_NT), 0, ctx->stream, P, nx, ny, pb, tx, taps);
    else
        hipLaunchKernelGGL((k_trk_structure<S, TK_RBIG>), dim3(tx * ty, slots), dim3(TK_NT), 0, ctx->stream, P, nx, ny, pb, tx, taps);
}
// lam2 and the mean of slots <= OFX_MAX_GROUP frames on the context's GPU; rows: slots * ny doubles of workspace
static int op_track_structure(ofx_ctx *ctx, int kind, int slots, const OfxTrkFrames &P, double *rows, int nx, int ny, size_t pitch,
                              const GaussTaps &taps, bool want_mean)
{
    switch (kind) {
    case OFX_SRC_F64: tk_launch_structure<double>(ctx, slots, P, nx, ny, pitch, taps); break;
    case OFX_SRC_F32: tk_launch_structure<float>(ctx, slots, P, nx, ny, pitch, taps); break;
    case OFX_SRC_U8:  tk_launch_structure<unsigned char>(ctx, slots, P, nx, ny, pitch, taps); break;
    case OFX_SRC_U16: tk_launch_structure<unsigned short>(ctx, slots, P, nx, ny, pitch, taps); break;
    default:          tk_launch_structure<OfxRgb8>(ctx, slots, P, nx, ny, pitch, taps); break;
    }
    OFX_LAUNCH_CHECK(ctx);
    if (!want_mean) return OFX_OK;
    hipLaunchKernelGGL(k_trk_rowsum, dim3(ofx_cdiv(ny, 4), slots), dim3(256), 0, ctx->stream, P, rows, nx, ny);
    OFX_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_trk_mean, dim3(slots), dim3(64), 0, ctx->stream, P, rows, nx, ny);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

extern "C" int ofx_track_structure_dev(ofx_ctx *ctx, int n, const void *const *dF, void *const *d_lam2, void *const *d_mean, int nx,
                                       int ny, double rho)
{
    OFX_ENTER(ctx);
    const char *who = "track_structure";
    if (!dF) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    if (n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n = %d (at least 1)", who, n);
    GaussTaps taps;
    OFX_TRY(tk_check(ctx, who, nx, ny, rho, &taps));
    const int kind = ofx_src_kind(ctx);
    std::set<const void *> in;
    for (int g = 0; g < n; g++) {
        if (!dF[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        if (tk_misaligned(dF[g], ofx_src_align(kind)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the frame of slot %d is not aligned to its element's %d bytes", who, g, (int) ofx_src_align(kind));
        in.insert(dF[g]);
    }
    for (int g = 0; g < n; g++) {
        const void *l = d_lam2 ? d_lam2[g] : nullptr, *m = d_mean ? d_mean[g] : nullptr;
        if (tk_misaligned(l, sizeof(double)) || tk_misaligned(m, sizeof(double)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination of slot %d is not 8-byte aligned", who, g);
        if ((l && in.count(l)) || (m && in.count(m)) || (l && l == m))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination of slot %d is a frame that the call reads, or its other destination", who, g);
    }
    const size_t pitch = ofx_src_pitch(ctx, nx), px = (size_t) nx * ny;
    const size_t span = ofx_frame_span(nx, ny, pitch, ofx_src_bytes(kind));
    const int per = n < OFX_MAX_GROUP ? n : OFX_MAX_GROUP;
    double *rows, *ws = nullptr;
    OFX_TRY(ofx_alloc(ctx, (size_t) per * ny, &rows));
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxTrkFrames P = {};
        void *lam[OFX_MAX_GROUP] = {}, *mean[OFX_MAX_GROUP] = {};
        bool want_mean = false;
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *src;
            OFX_TRY(ofx_stage_in(ctx, dF[g], span, true, &src));
            OFX_TRY(ofx_stage_in(ctx, d_lam2 ? d_lam2[g] : nullptr, px * sizeof(double), false, &lam[z]));
            OFX_TRY(ofx_stage_in(ctx, d_mean ? d_mean[g] : nullptr, sizeof(double), false, &mean[z]));
            P.src[z] = src;
            P.mean[z] = static_cast<double *>(mean[z]);
            want_mean = want_mean || mean[z];
            if (lam[z]) P.lam2[z] = static_cast<double *>(lam[z]);
            else {                                                           // only the mean is wanted: lam2 passes through the workspace
                if (!ws) OFX_TRY(ofx_alloc(ctx, (size_t) per * px, &ws));
                P.lam2[z] = ws + (size_t) z * px;
            }
        }
        OFX_TRY(op_track_structure(ctx, kind, cnt, P, rows, nx, ny, pitch, taps, want_mean));
        for (int z = 0; z < cnt; z++) {
            if (lam[z]) OFX_TRY(ofx_stage_out(ctx, d_lam2[g0 + z], lam[z], px * sizeof(double)));
            if (mean[z]) OFX_TRY(ofx_stage_out(ctx, d_mean[g0 + z], mean[z], sizeof(double)));
        }
    }
    return OFX_OK;
}

// the cells of a frame and the launches over them
struct TkCells { int ncx, ncy, nc, nb; };
static TkCells tk_cells(int nx, int ny, int step)
{
    TkCells c;
    c.ncx = (nx - 1) / step + 1;
    c.ncy = (ny - 1) / step + 1;
    c.nc = c.ncx * c.ncy;                                                    // <= nx * ny: fits an int
    c.nb = ofx_cdiv(c.nc, 256);
    return c;
}
// the seeds of the frames whose lam2 and mean S names, into the unoccupied cells of occ: count, scan, scatter
static int op_track_seeds(ofx_ctx *ctx, int slots, const OfxTrkSeed &S, const unsigned char *occ, int *blk, const TkCells &c, int cap,
                          bool fresh, int birth, int last, int nx, int ny, int step, double frac)
{
    hipLaunchKernelGGL(k_trk_count, dim3(c.nb, slots), dim3(256), 0, ctx->stream, S, occ, blk, c.nb, nx, ny, step, c.ncx, c.nc, frac);
    OFX_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_trk_scan, dim3(slots), dim3(256), 0, ctx->stream, S, blk, c.nb, cap, fresh ? 1 : 0);
    OFX_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_trk_scatter, dim3(c.nb, slots), dim3(256), 0, ctx->stream, S, occ, blk, c.nb, cap, birth, last, nx, ny, step,
                       c.ncx, c.nc, frac);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

extern "C" int ofx_track_seed_dev(ofx_ctx *ctx, int n, const void *const *dF, const void *const *d_xy_occ, int n_occ,
                                  void *const *d_xy_new, void *const *d_count, int cap, int nx, int ny, double rho, double frac, int step)
{
    OFX_ENTER(ctx);
    const char *who = "track_seed";
    if (!dF || !d_xy_new || !d_count) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    if (n < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n = %d (at least 1)", who, n);
    if (n_occ < 0) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_occ = %d (not below 0)", who, n_occ);
    OFX_TRY(tk_check_seed(ctx, who, cap, frac, step));
    GaussTaps taps;
    OFX_TRY(tk_check(ctx, who, nx, ny, rho, &taps));
    const int kind = ofx_src_kind(ctx);
    const bool has_occ = d_xy_occ && n_occ > 0;
    std::set<const void *> in;
    for (int g = 0; g < n; g++) {
        if (!dF[g] || !d_xy_new[g] || !d_count[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (slot %d)", who, g);
        if (tk_misaligned(dF[g], ofx_src_align(kind)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the frame of slot %d is not aligned to its element's %d bytes", who, g, (int) ofx_src_align(kind));
        if (tk_misaligned(d_xy_new[g], sizeof(double)) || (has_occ && tk_misaligned(d_xy_occ[g], sizeof(double))))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the positions of slot %d are not 8-byte aligned", who, g);
        if (tk_misaligned(d_count[g], sizeof(int))) return ofx_fail(ctx, OFX_ERR_ARG, "%s: the counts of slot %d are not 4-byte aligned", who, g);
        in.insert(dF[g]);
        if (has_occ && d_xy_occ[g]) in.insert(d_xy_occ[g]);
    }
    for (int g = 0; g < n; g++)
        if (in.count(d_xy_new[g]) || in.count(d_count[g]) || d_xy_new[g] == d_count[g])
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination of slot %d is an array that the call reads, or its other destination", who, g);
    const size_t pitch = ofx_src_pitch(ctx, nx), px = (size_t) nx * ny;
    const size_t span = ofx_frame_span(nx, ny, pitch, ofx_src_bytes(kind));
    const size_t xy_bytes = (size_t) cap * 2 * sizeof(double), occ_bytes = (size_t) n_occ * 2 * sizeof(double);
    const TkCells c = tk_cells(nx, ny, step);
    const int per = n < OFX_MAX_GROUP ? n : OFX_MAX_GROUP;
    double *rows, *lam2, *mean;
    unsigned char *occ;
    int *blk;
    OFX_TRY(ofx_alloc(ctx, (size_t) per * ny, &rows));
    OFX_TRY(ofx_alloc(ctx, (size_t) per * px, &lam2));
    OFX_TRY(ofx_alloc(ctx, (size_t) per, &mean));
    OFX_TRY(ofx_alloc(ctx, (size_t) per * c.nc, &occ));
    OFX_TRY(ofx_alloc(ctx, (size_t) per * (c.nb + 1), &blk));
    for (int g0 = 0; g0 < n; g0 += OFX_MAX_GROUP) {
        const int cnt = n - g0 < OFX_MAX_GROUP ? n - g0 : OFX_MAX_GROUP;
        OfxTrkFrames P = {};
        OfxTrkSeed S = {};
        void *xy[OFX_MAX_GROUP], *count[OFX_MAX_GROUP];
        for (int z = 0; z < cnt; z++) {
            const int g = g0 + z;
            void *src, *pts;
            OFX_TRY(ofx_stage_in(ctx, dF[g], span, true, &src));
            OFX_TRY(ofx_stage_in(ctx, has_occ ? d_xy_occ[g] : nullptr, occ_bytes, true, &pts));
            // filled: what lies beyond the seeds written comes back as it was
            OFX_TRY(ofx_stage_in(ctx, d_xy_new[g], xy_bytes, true, &xy[z]));
            OFX_TRY(ofx_stage_in(ctx, d_count[g], 2 * sizeof(int), false, &count[z]));
            P.src[z] = src;
            P.lam2[z] = lam2 + (size_t) z * px;
            P.mean[z] = mean + z;
            S.lam2[z] = P.lam2[z];
            S.mean[z] = P.mean[z];
            S.pts[z] = static_cast<const double *>(pts);
            S.xy[z] = static_cast<double *>(xy[z]);
            S.count[z] = static_cast<int *>(count[z]);
        }
        OFX_TRY(op_track_structure(ctx, kind, cnt, P, rows, nx, ny, pitch, taps, true));
        OFX_HIP(ctx, hipMemsetAsync(occ, 0, (size_t) cnt * c.nc, ctx->stream));
        if (has_occ) {
            hipLaunchKernelGGL(k_trk_mark, dim3(ofx_cdiv(n_occ, 256), cnt), dim3(256), 0, ctx->stream, S, occ, n_occ, nx, ny, step, c.ncx, c.nc);
            OFX_LAUNCH_CHECK(ctx);
        }
        OFX_TRY(op_track_seeds(ctx, cnt, S, occ, blk, c, cap, true, 0, 0, nx, ny, step, frac));
        for (int z = 0; z < cnt; z++) {
            OFX_TRY(ofx_stage_out(ctx, d_xy_new[g0 + z], xy[z], xy_bytes));
            OFX_TRY(ofx_stage_out(ctx, d_count[g0 + z], count[z], 2 * sizeof(int)));
        }
    }
    return OFX_OK;
}

// Per chunk of OFX_MAX_GROUP clips: the seeds of frame 0, then per step one launch that advances every used slot and marks the
// survivors' cells, the structure pass of frame t + 1 and the three launches of its seeds.  The counts, the tables and the
// occupancy map stay on the device; every launch is sized by cap or by the cell count and reads the counters there.  The pointers
// of a launch travel in its arguments: there is no device table and nothing to await.
extern "C" int ofx_track_sequence_dev(ofx_ctx *ctx, int n_seq, int n_frames, const void *const *dF, const void *const *d_flo_step,
                                      const void *const *d_occ_step, int cap, void *const *d_xy, void *const *d_t0, void *const *d_len,
                                      void *const *d_count, int nx, int ny, double rho, double frac, int step)
{
    OFX_ENTER(ctx);
    const char *who = "track_sequence";
    if (!dF || !d_flo_step || !d_xy || !d_t0 || !d_len || !d_count) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer table", who);
    if (n_seq < 1) return ofx_fail(ctx, OFX_ERR_ARG, "%s: n_seq = %d (at least 1)", who, n_seq);
    if (n_frames < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %d frames (a sequence has at least 2)", who, n_frames);
    OFX_TRY(tk_check_seed(ctx, who, cap, frac, step));
    GaussTaps taps;
    OFX_TRY(tk_check(ctx, who, nx, ny, rho, &taps));
    const int kind = ofx_src_kind(ctx), steps = n_frames - 1;
    std::set<const void *> in;
    for (int q = 0; q < n_seq; q++) {
        for (int f = 0; f < n_frames; f++) {
            const void *p = dF[(size_t) q * n_frames + f];
            if (!p) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL frame %d of sequence %d", who, f, q);
            if (tk_misaligned(p, ofx_src_align(kind)))
                return ofx_fail(ctx, OFX_ERR_ARG, "%s: frame %d of sequence %d is not aligned to its element's %d bytes", who, f, q, (int) ofx_src_align(kind));
            in.insert(p);
        }
        for (int t = 0; t < steps; t++) {
            const void *p = d_flo_step[(size_t) q * steps + t];
            if (!p) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (step %d of sequence %d)", who, t, q);
            if (tk_misaligned(p, sizeof(float2)))
                return ofx_fail(ctx, OFX_ERR_ARG, "%s: step payload %d of sequence %d is not 8-byte aligned", who, t, q);
            in.insert(p);
            if (d_occ_step && d_occ_step[(size_t) q * steps + t]) in.insert(d_occ_step[(size_t) q * steps + t]);
        }
        if (!d_xy[q] || !d_t0[q] || !d_len[q] || !d_count[q]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (sequence %d)", who, q);
        if (tk_misaligned(d_xy[q], sizeof(double))) return ofx_fail(ctx, OFX_ERR_ARG, "%s: the positions of sequence %d are not 8-byte aligned", who, q);
        if (tk_misaligned(d_t0[q], sizeof(int)) || tk_misaligned(d_len[q], sizeof(int)) || tk_misaligned(d_count[q], sizeof(int)))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: the int32 tables of sequence %d are not 4-byte aligned", who, q);
    }
    for (int q = 0; q < n_seq; q++) {
        const void *o[4] = {d_xy[q], d_t0[q], d_len[q], d_count[q]};
        for (int a = 0; a < 4; a++) {
            if (in.count(o[a])) return ofx_fail(ctx, OFX_ERR_ARG, "%s: a destination of sequence %d is an array that the call reads", who, q);
            for (int b = a + 1; b < 4; b++)
                if (o[a] == o[b]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: two destinations of sequence %d are the same array", who, q);
        }
    }
    const size_t pitch = ofx_src_pitch(ctx, nx), px = (size_t) nx * ny;
    const size_t span = ofx_frame_span(nx, ny, pitch, ofx_src_bytes(kind));
    const size_t xy_bytes = (size_t) n_frames * cap * 2 * sizeof(double), tab_bytes = (size_t) cap * sizeof(int);
    const TkCells c = tk_cells(nx, ny, step);
    const int per = n_seq < OFX_MAX_GROUP ? n_seq : OFX_MAX_GROUP;
    double *rows, *lam2, *mean;
    unsigned char *occ;
    int *blk;
    OFX_TRY(ofx_alloc(ctx, (size_t) per * ny, &rows));
    OFX_TRY(ofx_alloc(ctx, (size_t) per * px, &lam2));
    OFX_TRY(ofx_alloc(ctx, (size_t) per, &mean));
    OFX_TRY(ofx_alloc(ctx, (size_t) per * c.nc, &occ));
    OFX_TRY(ofx_alloc(ctx, (size_t) per * (c.nb + 1), &blk));
    for (int q0 = 0; q0 < n_seq; q0 += OFX_MAX_GROUP) {
        const int cnt = n_seq - q0 < OFX_MAX_GROUP ? n_seq - q0 : OFX_MAX_GROUP;
        OfxTrkFrames P = {};
        OfxTrkSeed S = {};
        void *xy[OFX_MAX_GROUP], *t0[OFX_MAX_GROUP], *len[OFX_MAX_GROUP], *count[OFX_MAX_GROUP];
        for (int z = 0; z < cnt; z++) {
            const int q = q0 + z;
            // filled: the slots beyond the count come back as they were
            OFX_TRY(ofx_stage_in(ctx, d_xy[q], xy_bytes, true, &xy[z]));
            OFX_TRY(ofx_stage_in(ctx, d_t0[q], tab_bytes, true, &t0[z]));
            OFX_TRY(ofx_stage_in(ctx, d_len[q], tab_bytes, true, &len[z]));
            OFX_TRY(ofx_stage_in(ctx, d_count[q], 2 * sizeof(int), false, &count[z]));
            P.lam2[z] = lam2 + (size_t) z * px;
            P.mean[z] = mean + z;
            S.lam2[z] = P.lam2[z];
            S.mean[z] = P.mean[z];
            S.xy[z] = static_cast<double *>(xy[z]);
            S.t0[z] = static_cast<int *>(t0[z]);
            S.len[z] = static_cast<int *>(len[z]);
            S.count[z] = static_cast<int *>(count[z]);
        }
        for (int f = 0; f < n_frames; f++) {
            OFX_HIP(ctx, hipMemsetAsync(occ, 0, (size_t) cnt * c.nc, ctx->stream));
            if (f > 0) {
                for (int z = 0; z < cnt; z++) {
                    const size_t e = (size_t) (q0 + z) * steps + f - 1;
                    void *flo, *map;
                    OFX_TRY(ofx_stage_in(ctx, d_flo_step[e], px * sizeof(float2), true, &flo));
                    OFX_TRY(ofx_stage_in(ctx, d_occ_step ? d_occ_step[e] : nullptr, px, true, &map));
                    S.flo[z] = static_cast<const float2 *>(flo);
                    S.map[z] = static_cast<const unsigned char *>(map);
                }
                hipLaunchKernelGGL(k_trk_advance, dim3(ofx_cdiv(cap, 256), cnt), dim3(256), 0, ctx->stream, S, occ, f - 1, cap, nx, ny, step,
                                   c.ncx, c.nc);
                OFX_LAUNCH_CHECK(ctx);
            }
            for (int z = 0; z < cnt; z++) {
                void *src;
                OFX_TRY(ofx_stage_in(ctx, dF[(size_t) (q0 + z) * n_frames + f], span, true, &src));
                P.src[z] = src;
            }
            OFX_TRY(op_track_structure(ctx, kind, cnt, P, rows, nx, ny, pitch, taps, true));
            OFX_TRY(op_track_seeds(ctx, cnt, S, occ, blk, c, cap, f == 0, f, n_frames - 1, nx, ny, step, frac));
        }
        for (int z = 0; z < cnt; z++) {
            const int q = q0 + z;
            OFX_TRY(ofx_stage_out(ctx, d_xy[q], xy[z], xy_bytes));
            OFX_TRY(ofx_stage_out(ctx, d_t0[q], t0[z], tab_bytes));
            OFX_TRY(ofx_stage_out(ctx, d_len[q], len[z], tab_bytes));
            OFX_TRY(ofx_stage_out(ctx, d_count[q], count[z], 2 * sizeof(int)));
        }
    }
    return OFX_OK;
}
