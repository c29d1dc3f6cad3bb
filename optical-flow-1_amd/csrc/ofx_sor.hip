// ofx_sor.hip -- Horn-Schunck pyramidal and Brox spatial on gfx950
// (reference: src/horn_schunck_pyramidal.cpp, src/brox_optic_flow_spatial.cpp, src/brox_spatial_mask.cpp).
//
// Both reference solvers are in-place SOR (w = 1.9) swept in lexicographic order -- a sequential
// recurrence.  The GPU sweeps in colours instead: Horn-Schunck's 8-neighbour stencil needs four
// colours (i%2, j%2), Brox's 5-point stencil two (red-black).  Within one colour no pixel reads
// another pixel of the same colour (borders use clamped neighbour indices, which is what the
// reference's replicated border indices amount to), so the in-place update is race-free and
// deterministic.  Per-pixel arithmetic is the reference's expression for expression; what changes
// is the ORDER in which pixels see each other's new values, hence the trajectory and the sweep at
// which `error > TOL` fails.  Measured against the lexicographic reference (tests):
// Horn-Schunck AEPE 1e-5..5e-5 (inside the 1e-4 bar), Brox up to 1.6e-4 (the reference's own
// 1-vs-8-thread spread is 3.6e-5).  oracle's `set_sor_order(1)` reproduces this file bit for bit.
//
// Storage per level (T = storage type):
//   HS  : U=(u,v) pairs in place; pa=(I2,I2x), pb=I2y; A=(I2wx,I2wy); Dif=dif  -- the five coefficient
//         arrays Au,Av,Du,Dv,D of the reference are recomputed from A, Dif in registers (same ops).
//   Brox: U; G1=(I1x,I1y); PA=(I2,I2x,I2y,I2xx), PB=(I2xy,I2yy); WA/WB = their warps; Psis;
//         DV=(div_u,div_v), Dd=div_d; CO=(Au,Av,Du,Dv), Dm=D; DU=(du,dv) in place.
#include "ofx_ops.h"
#include "ofx_device.h"
#include "ofx_loop.h"
#include "ofx_sor_tile.h"
#include "ofx_pairs.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <thread>

#define HS_SOR_W 1.9                 // src/horn_schunck_pyramidal.cpp:21
#define HS_PLANE_C_SKEW 2             // Horn-Schunck hyperplanes: pos = 2 i + j (k_hs_plane)
#define BROX_PLANE_C_SKEW 1           // Brox hyperplanes: pos = i + j (k_brox_plane)
#define HS_PRESMOOTH_SIGMA 0.8       // src/horn_schunck_pyramidal.cpp:22
#define BROX_EPSILON 0.001           // src/brox_optic_flow_spatial.cpp:23
#define BROX_SOR_W 1.9               // src/brox_optic_flow_spatial.cpp:25
#define BROX_SIGMA 0.8               // src/brox_optic_flow_spatial.cpp:26

static inline dim3 g2d(int nx, int ny) { return dim3(ofx_cdiv(nx, 64), ofx_cdiv(ny, 4)); }
static inline dim3 b2d() { return dim3(64, 4); }

static int sor_pick_chunk(const ofx_ctx *ctx, int nx, int ny, int launches_per_sweep)
{
    if (ctx->chunk > 0) return ctx->chunk;
    const double est_us = fmax(4.0 * launches_per_sweep, (double) nx * ny * 100.0 / 2.0e6);
    int c = (int) (60.0 / est_us);
    return c < 2 ? 2 : (c > 32 ? 32 : c);
}

// ============================================================================================
// Horn-Schunck
// ============================================================================================

// warp of (I2, I2x, I2y) + constant parts of the system, src/horn_schunck_pyramidal.cpp:123-137
// (ucode: bit g set = the flow of pair g lives in U1, the second buffer of the tile sweeps' ping-pong, ofx_sor_tile.hip)
template <typename T>
__global__ void k_hs_warp(const typename Pix<T>::v2 *__restrict__ pa, const T *__restrict__ pb, const T *__restrict__ I1,
                          const typename Pix<T>::v2 *__restrict__ U, const typename Pix<T>::v2 *__restrict__ U1, unsigned ucode,
                          typename Pix<T>::v2 *__restrict__ A, T *__restrict__ Dif, int nx, int ny)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t go = (size_t) blockIdx.z * nx * ny;             // pair of a lockstep group
    if ((ucode >> blockIdx.z) & 1u) U = U1;
    pa += go; pb += go; I1 += go; U += go; A += go; Dif += go;
    const size_t p = (size_t) i * nx + j;
    const double2 u = ldw2(U + p);
    const BicubicTaps t = bicubic_taps(j + u.x, i + u.y, nx, ny);
    double I2w = 0.0, I2wx = 0.0, I2wy = 0.0;
    if (!t.out) {
        bicubic_sample3(pa, pb, t, nx, I2w, I2wx, I2wy);
        I2wx = rnd_to<T>(I2wx);
        I2wy = rnd_to<T>(I2wy);
    }
    const double I2wl = I2wx * u.x + I2wy * u.y;                 // :130
    const double dif = ldw(I1 + p) - I2w + I2wl;                 // :131
    stn2(A + p, make_double2(I2wx, I2wy));
    stn(Dif + p, dif);
}

// ---- how a sweep kernel reaches the in-place unknowns -------------------------------------------------------
// UGlobal: straight from / to the global array (COH: past the L1, see ldu2; SNAP: also into the sweep's snapshot).
// (An accessor that served same-launch hand-offs from an LDS ring was built and measured: correct, but slower --
// a windowed step is bound by the memory latency of the PREVIOUS sweep's values and by one CU's f64 rate, not by
// the store drain the ring removes.  DESIGN.md 5.3.)
// ---- where pixel (i, j) of a plane lives --------------------------------------------------------------------------
// LayRow: row-major, the layout of every array outside the windowed sweeps.
// LaySkew: hyperplane-major.  In the windowed exact sweeps the lanes of a wave are consecutive ROWS of one hyperplane
// (pixel (r, q - c r) for lane r), so in a row-major array every lane of every load sits in a different cache line: 64
// lines per wave instruction, 13 memory instructions per update -- the vector L1 (one line per clock and CU) was the
// bound, and a launch took 16x as long for 16 lockstep pairs (profiles/r02_c_*).  With element (i, j) at
// (c i + j) ny + i the pixels of a hyperplane are contiguous in i, and so are all their neighbours (each lies on a
// hyperplane q + const at row i + const): every access of a wave is one contiguous run.  The plane is padded to
// (c (ny - 1) + nx) * ny elements; c = 2 for the 8-neighbour stencil of Horn-Schunck, 1 for Brox.
struct LayRow {
    int nx;
    OFX_DEV size_t idx(int i, int j) const { return (size_t) i * nx + j; }
};
struct LaySkew {
    int ny, c;
    OFX_DEV size_t idx(int i, int j) const { return (size_t) (c * i + j) * ny + i; }
};
static inline size_t skew_plane_elems(int nx, int ny, int c) { return (size_t) (c * (ny - 1) + nx) * ny; }

template <typename T, bool COH, bool SNAP, class Lay = LayRow> struct UGlobal {
    typename Pix<T>::v2 *U, *snap;
    Lay lay;
    OFX_DEV double2 get(int ii, int jj) const { return ldu2<COH>(U + lay.idx(ii, jj)); }
    // the constant operands of pixel (i, j): HS (A, dif)
    OFX_DEV void coef(const typename Pix<T>::v2 *__restrict__ A, const T *__restrict__ Dif, int i, int j, double2 &a, double &dif) const
    {
        const size_t p = lay.idx(i, j);
        a = ldw2(A + p);
        dif = ldw(Dif + p);
    }
    // Brox: psi_s of pixel (ii, jj); (CO, Dm) of pixel (i, j)
    OFX_DEV double psi(const T *__restrict__ Psis, int ii, int jj) const { return ldw(Psis + lay.idx(ii, jj)); }
    OFX_DEV void coef4(const typename Pix<T>::v4 *__restrict__ CO, const T *__restrict__ Dm, int i, int j, double4 &co, double &D) const
    {
        const size_t p = lay.idx(i, j);
        co = ldw4(CO + p);
        D = ldw(Dm + p);
    }
    OFX_DEV void put(int i, int j, double2 v) const
    {
        const size_t p = lay.idx(i, j);
        stn2(U + p, v);
        if (SNAP) stn2(snap + p, v);
    }
};

// row-major <-> skewed copies of one array of a lockstep group (blockIdx.z = pair): IN = true writes dst[skew] =
// src[row-major], false the other way.  Once per solve and array, next to tens of sweeps.
template <typename V, bool IN>
__global__ void k_skew(const V *__restrict__ src, V *__restrict__ dst, int nx, int ny, int c, size_t plane_s)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const LaySkew lay = {ny, c};
    const size_t rm = (size_t) blockIdx.z * nx * ny + (size_t) i * nx + j, sk = blockIdx.z * plane_s + lay.idx(i, j);
    if (IN) dst[sk] = src[rm];
    else dst[rm] = src[sk];
}
template <typename V, bool IN>
static int op_skew(ofx_ctx *ctx, const V *src, V *dst, int nx, int ny, int c, int G)
{
    hipLaunchKernelGGL((k_skew<V, IN>), dim3(ofx_cdiv(nx, 64), ofx_cdiv(ny, 4), G), dim3(64, 4), 0, ctx->stream, src, dst, nx,
                       ny, c, skew_plane_elems(nx, ny, c));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ofx_fail(ctx, OFX_ERR_HIP, "skew copy launch failed: %s", hipGetErrorString(e));
    return OFX_OK;
}
// SOR update of one pixel, src/horn_schunck_pyramidal.cpp:31-71.  Neighbour indices are the clamped
// coordinates -- exactly what the reference's replicated border indices are (:161-228) -- in the order
// up-left, up-right, bottom-left, bottom-right / up, left, bottom, right, with ONE quirk kept for
// bit-exactness: the bottom-right corner lists its diagonal taps bottom pair first (:222-228).
// Returns the squared update (:70).
// operands of one update, loaded first so that several independent updates can have their loads in flight together
struct HsOps {
    double2 p1, p2, p3, p4, p5, p6, p7, p8, c, a;
    double  dif;
};
template <typename T, class Acc>
OFX_DEV HsOps hs_point_load(const Acc &acc, const typename Pix<T>::v2 *__restrict__ A, const T *__restrict__ Dif, int i, int j,
                            int nx, int ny)
{
    const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
    const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
    HsOps o;
    o.p1 = acc.get(iu, jl); o.p2 = acc.get(iu, jr);
    o.p3 = acc.get(id, jl); o.p4 = acc.get(id, jr);
    if (i == ny - 1 && j == nx - 1) {
        const double2 a1 = o.p1, a2 = o.p2;
        o.p1 = o.p3; o.p2 = o.p4; o.p3 = a1; o.p4 = a2;
    }
    o.p5 = acc.get(iu, j); o.p6 = acc.get(i, jl);
    o.p7 = acc.get(id, j); o.p8 = acc.get(i, jr);
    o.c = acc.get(i, j);
    acc.coef(A, Dif, i, j, o.a, o.dif);
    return o;
}
template <typename T, class Acc>
OFX_DEV double hs_point_finish(const Acc &acc, const HsOps &o, int i, int j, double alpha2)
{
    const double2 a = o.a;
    const double dif = o.dif;
    const double w = HS_SOR_W;
    const double Au = dif * a.x, Av = dif * a.y;                              // :133-134
    const double Du = a.x * a.x + alpha2, Dv = a.y * a.y + alpha2;            // :135-136
    const double D = a.x * a.y;                                               // :137
    const double ula = 1. / 12. * (o.p1.x + o.p2.x + o.p3.x + o.p4.x) + 1. / 6. * (o.p5.x + o.p6.x + o.p7.x + o.p8.x);
    const double vla = 1. / 12. * (o.p1.y + o.p2.y + o.p3.y + o.p4.y) + 1. / 6. * (o.p5.y + o.p6.y + o.p7.y + o.p8.y);
    const double uk = o.c.x, vk = o.c.y;
    const double un = rnd_to<T>((1.0 - w) * uk + w * (Au - D * vk + alpha2 * ula) / Du);   // :66
    const double vn = rnd_to<T>((1.0 - w) * vk + w * (Av - D * un + alpha2 * vla) / Dv);   // :67
    acc.put(i, j, make_double2(un, vn));
    return (un - uk) * (un - uk) + (vn - vk) * (vn - vk);                     // :70
}
template <typename T, class Acc>
OFX_DEV double hs_point_acc(const Acc &acc, const typename Pix<T>::v2 *__restrict__ A, const T *__restrict__ Dif, int i,
                            int j, int nx, int ny, double alpha2)
{
    const HsOps o = hs_point_load<T>(acc, A, Dif, i, j, nx, ny);
    return hs_point_finish<T>(acc, o, i, j, alpha2);
}

template <typename T, bool COH = false, bool SNAP = false>
OFX_DEV double hs_point(typename Pix<T>::v2 *U, const typename Pix<T>::v2 *__restrict__ A,
                        const T *__restrict__ Dif, int i, int j, int nx, int ny, double alpha2,
                        typename Pix<T>::v2 *snap = nullptr)
{
    const UGlobal<T, COH, SNAP, LayRow> acc = {U, snap, LayRow{nx}};
    return hs_point_acc<T>(acc, A, Dif, i, j, nx, ny, alpha2);
}
// the same on hyperplane-major arrays (windowed sweeps)
template <typename T, bool COH, bool SNAP>
OFX_DEV double hs_point_skew(typename Pix<T>::v2 *U, const typename Pix<T>::v2 *__restrict__ A, const T *__restrict__ Dif,
                             int i, int j, int nx, int ny, double alpha2, typename Pix<T>::v2 *snap)
{
    const UGlobal<T, COH, SNAP, LaySkew> acc = {U, snap, LaySkew{ny, HS_PLANE_C_SKEW}};
    return hs_point_acc<T>(acc, A, Dif, i, j, nx, ny, alpha2);
}

// One colour of one SOR sweep (fast, order-changing mode).
template <typename T>
__global__ __launch_bounds__(256) void k_hs_sor(typename Pix<T>::v2 *__restrict__ U,
                                                const typename Pix<T>::v2 *__restrict__ A, const T *__restrict__ Dif,
                                                double *__restrict__ err, int k, int nx, int ny, int ci, int cj,
                                                double alpha2, double tol)
{
    const double prev = loop_fetch_prev(err, k);
    const int j = 2 * (blockIdx.x * 64 + threadIdx.x) + cj;
    const int i = 2 * (blockIdx.y * 4 + threadIdx.y) + ci;
    const bool in = (j < nx) && (i < ny);
    const int gw = (blockIdx.y * gridDim.x + blockIdx.x) * 4 + threadIdx.y;
    if (!loop_continues(prev, k, nx * ny, tol, OFX_CRIT_SQRT_MEAN)) return;
    double e = 0.0;
    if (in) e = hs_point<T>(U, A, Dif, i, j, nx, ny, alpha2);
    loop_accumulate(err, k, e, gw);
}

// ---- exact mode: the reference's sequential sweep order, pipelined over hyperplanes --------------------
// Pixel X of sweep s runs at time t = pos(X) + C s.  pos() is the pixel's rank in a time-skewed version of
// the reference's visiting order (interior rows lexicographic -> first/last row -> first/last column ->
// corners, horn_schunck_pyramidal.cpp:148-228) and C the spacing between consecutive sweeps, chosen so
// that for every two NEIGHBOURING pixels X before Y in that order   t(X,s) < t(Y,s) < t(X,s+1).
// Then (a) all pixels of one time step are mutually independent, (b) the in-place array holds, at the
// moment X of sweep s runs, exactly the versions the sequential sweep would read (Y of sweep s if Y comes
// earlier, of sweep s-1 if later).  One launch = one time step, all sweeps of the batch that are inside
// the image at that time (blockIdx.y = sweep).  HS (8 neighbours): pos = 2i + j in the interior, C = 6.
// The same schedule is executed on the CPU by oracle order 2 and is bit-identical to the reference's
// sequential sweeps (tests/test_oracle_golden.py::test_hyperplane_schedule_is_exact).
#define HS_PLANE_C 6
OFX_DEV bool hs_plane_item(int r, int q, int nx, int ny, int corner, int &i, int &j)
{
    if (r >= 1 && r <= ny - 2) { i = r; j = q - 2 * r; return j >= 1 && j <= nx - 2; }          // interior
    if (r == 0) { i = 0; j = q - 4; return j >= 1 && j <= nx - 2; }                               // first row
    if (r == ny - 1) { i = ny - 1; j = q - 2 * (ny - 1); return j >= 1 && j <= nx - 2; }         // last row
    if (r == ny) { const int d = q - 4; i = d >> 1; j = 0; return !(d & 1) && i >= 1 && i <= ny - 2; }             // first column
    if (r == ny + 1) { const int d = q - nx - 1; i = d >> 1; j = nx - 1; return !(d & 1) && i >= 1 && i <= ny - 2; }  // last column
    if (r == ny + 2) {                                                                            // corners
        if (corner == 0) { i = 0; j = 0; return q == 7; }
        if (corner == 1) { i = 0; j = nx - 1; return q == nx + 4; }
        if (corner == 2) { i = ny - 1; j = 0; return q == 2 * ny + 1; }
        i = ny - 1; j = nx - 1; return q == 2 * ny + nx - 2;
    }
    return false;
}

template <typename T>
__global__ __launch_bounds__(64) void k_hs_plane(typename Pix<T>::v2 *__restrict__ U,
                                                 const typename Pix<T>::v2 *__restrict__ A, const T *__restrict__ Dif,
                                                 double *__restrict__ err, int t, int s_lo, int nx, int ny, double alpha2)
{
    const int s = s_lo + blockIdx.y;
    const int q = t - HS_PLANE_C * s;
    const int r = blockIdx.x * 64 + threadIdx.x;
    double e = 0.0;
    int i, j;
    if (r == ny + 2) {
        for (int corner = 0; corner < 4; corner++)
            if (hs_plane_item(r, q, nx, ny, corner, i, j)) e += hs_point<T>(U, A, Dif, i, j, nx, ny, alpha2);
    } else if (hs_plane_item(r, q, nx, ny, 0, i, j)) {
        e = hs_point<T>(U, A, Dif, i, j, nx, ny, alpha2);
    }
    loop_accumulate(err, s, e, blockIdx.x);
}

// ---- exact mode, windowed: K time steps per launch ----------------------------------------------------------
// One launch per time step makes the exact mode host-launch-bound (~4.5 us per step, thousands of steps per
// solve).  The schedule t = pos + C s stays valid for any LARGER sweep spacing, so sweeps are spaced K + C steps
// apart and a launch executes the K steps [tau0, tau0 + K) of every sweep in flight, ONE WORKGROUP PER SWEEP:
// sweep s runs its local steps q = tau - (K + C) s, thread r of its workgroup owns plane item r (k_hs_plane's
// numbering), and consecutive steps are separated by a store drain + workgroup barrier.  Everything sweep s
// reads from sweep s - 1 (pos <= q + C - 1, i.e. tau' <= tau - K - 1) was written in an EARLIER launch, so
// workgroups never communicate inside a launch: no flags, no spinning, no placement assumptions -- only
// same-workgroup hand-offs (L1-bypassing loads, ldu2) and kernel boundaries.  Launches per batch of S sweeps:
// (qmax + (K + C) S) / K instead of qmax + C S.
// Every sweep also writes its values into its own snapshot plane: the state after sweep n is snapshot n,
// whatever later sweeps of the batch have overwritten in place, so a batch that ran past the stopping sweep
// needs no rollback and re-run.
// OFX_SOR_COH = 1: unknowns are read past the L1 (sc1).  0 (default): plain loads -- within a workgroup the L1 is
// coherent (same CU, write-through), and everything read from other sweeps was written before this launch began.
#ifndef OFX_SOR_COH
#define OFX_SOR_COH 0
#endif
// Geometry of one windowed launch (see sor_window_loop).  A sweep is further cut into row blocks of R rows,
// one workgroup per (sweep, block): block b runs lag_b steps behind block b - 1 of its sweep, sweeps are
// lag_s apart, and a border pixel is executed by the block of the interior row it depends on last.
struct SorWin {
    int tau0, K, lag_s, lag_b, lag_f, s_first, R;      // lag_f: spacing of the frames of a sequence (temporal Brox)
};
// Lockstep group: G image pairs solved by the same launches (blockIdx.z = pair), every array of a level holding the
// pairs back to back.  A lone solve is a latency chain of qmax + lag_s * sweeps dependent steps with a few hundred
// waves of work each; the pairs of a group share that chain.  Each pair keeps its own error slots, snapshots and
// stopping test (bit g of runmask: pair g still sweeps in this solve), so its flow is the one it gets alone.
struct SorGrp {
    unsigned runmask;
    int      err_stride;     // doubles between the error slots of consecutive pairs
    size_t   npix;           // elements of one (hyperplane-major, padded) plane = distance between consecutive pairs
    size_t   snap_stride;    // elements between the snapshot planes of consecutive pairs
};
// which plane item thread t of block b plays: its R rows, then the three shared items (first column, last
// column, corners) of which a block accepts only the pixels assigned to it (sor_border_block)
OFX_DEV int sor_window_item(const SorWin &w, int b, int t, int ny)
{
    if (t < w.R) { const int r = b * w.R + t; return r < ny ? r : -1; }
    return t < w.R + 3 ? ny + (t - w.R) : -1;
}
// block of a border-column / corner pixel: the row below for the columns (the interior pixel (i+1, 1) precedes
// (i, 0) in the reference order), row 2 for the top corners, the last row for the bottom corners
OFX_DEV int sor_border_block(int i, int ny, int R)
{
    int r;
    if (i == 0) r = ny - 1 < 2 ? ny - 1 : 2;
    else if (i == ny - 1) r = ny - 1;
    else r = i + 1;
    return r / R;
}

// Local steps at which row block b has any pixel to update (rows b R .. min(b R + R, ny) - 1 and the border pixels assigned to
// it, sor_border_block): [c b R, c r_last + nx + 5] for the stencil skew c (2 Horn-Schunck, 1 Brox) -- half of the (sweep, block)
// units of a launch lie outside it and leave at once (tools/check_sor_schedule.py unit_range, tests/test_host_logic.py).
OFX_DEV bool sor_unit_idle(const SorWin &w, int b, int q_first, int K, int c, int nx, int ny)
{
    const int rf = b * w.R, rl = (rf + w.R < ny ? rf + w.R : ny) - 1;
    return q_first > c * rl + nx + 5 || q_first + K - 1 < c * rf;
}

// SPW consecutive sweeps of one row block share a workgroup: their updates are independent (lag_s steps apart), so their
// loads are issued together and ONE store drain + barrier per step serves all of them -- the per-step latency, not
// arithmetic or bandwidth, is what bounds a lockstep group (profiles/r02_f_sor_counters.txt).
template <typename T, int SPW, int MAXT>
__global__ __launch_bounds__(MAXT) void k_hs_window(typename Pix<T>::v2 *Ug, typename Pix<T>::v2 *snap,
                                                    const typename Pix<T>::v2 *__restrict__ Ag, const T *__restrict__ Difg,
                                                    double *__restrict__ errg, SorWin w, SorGrp grp, int s_cnt, int nx, int ny,
                                                    double alpha2)
{
    const int b = blockIdx.x, s0 = w.s_first + blockIdx.y * SPW, g = blockIdx.z;
    if (!((grp.runmask >> g) & 1u)) return;                      // this pair's solve has already stopped
    const int qmax = 2 * ny + nx - 2;
    int q_first[SPW];
    bool live[SPW], any = false;
#pragma unroll
    for (int u = 0; u < SPW; u++) {
        q_first[u] = w.tau0 - w.lag_s * (s0 + u) - w.lag_b * b;
        live[u] = (s0 + u < w.s_first + s_cnt) && !sor_unit_idle(w, b, q_first[u], w.K, 2, nx, ny);
        any = any || live[u];
    }
    if (!any) return;                                            // none of these (sweep, block) units has a step in the window
    typename Pix<T>::v2 *U = Ug + g * grp.npix;
    const typename Pix<T>::v2 *__restrict__ A = Ag + g * grp.npix;
    const T *__restrict__ Dif = Difg + g * grp.npix;
    double *__restrict__ err = errg + (size_t) g * grp.err_stride;
    const int r = sor_window_item(w, b, threadIdx.x, ny);
    double e[SPW];
#pragma unroll
    for (int u = 0; u < SPW; u++) e[u] = 0.0;
    for (int k = 0; k < w.K; k++) {
        bool have[SPW];
        int pi[SPW], pj[SPW];
        HsOps ops[SPW];
#pragma unroll
        for (int u = 0; u < SPW; u++) {                          // all loads of this step first ...
            const int q = q_first[u] + k;
            have[u] = live[u] && q >= 0 && q <= qmax && r >= 0 && r != ny + 2 && hs_plane_item(r, q, nx, ny, 0, pi[u], pj[u]) &&
                      (r < ny || sor_border_block(pi[u], ny, w.R) == b);
            if (SPW > 1 && have[u]) {
                const UGlobal<T, OFX_SOR_COH != 0, true, LaySkew> acc = {U, snap + g * grp.snap_stride + (size_t) (s0 + u) * grp.npix,
                                                                         LaySkew{ny, HS_PLANE_C_SKEW}};
                ops[u] = hs_point_load<T>(acc, A, Dif, pi[u], pj[u], nx, ny);
            }
        }
#pragma unroll
        for (int u = 0; u < SPW; u++) {                          // ... then the updates
            typename Pix<T>::v2 *mysnap = snap + g * grp.snap_stride + (size_t) (s0 + u) * grp.npix;
            if (have[u]) {
                const UGlobal<T, OFX_SOR_COH != 0, true, LaySkew> acc = {U, mysnap, LaySkew{ny, HS_PLANE_C_SKEW}};
                // one sweep per workgroup: load and update in one go (the compiler interleaves them in 66 VGPRs = 7 waves
                // per SIMD; holding every operand first would take 106)
                if (SPW > 1) e[u] += hs_point_finish<T>(acc, ops[u], pi[u], pj[u], alpha2);
                else e[u] += hs_point_acc<T>(acc, A, Dif, pi[u], pj[u], nx, ny, alpha2);
            }
            const int q = q_first[u] + k;
            if (live[u] && r == ny + 2 && q >= 0 && q <= qmax) {  // the corner item: up to four pixels, one after the other
                int i, j;
                for (int corner = 0; corner < 4; corner++)
                    if (hs_plane_item(r, q, nx, ny, corner, i, j) && sor_border_block(i, ny, w.R) == b)
                        e[u] += hs_point_skew<T, OFX_SOR_COH != 0, true>(U, A, Dif, i, j, nx, ny, alpha2, mysnap);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this step's stores have reached L2 ...
        __syncthreads();                                       // ... before any wave of the workgroup reads them
    }
#pragma unroll
    for (int u = 0; u < SPW; u++)
        if (live[u]) loop_accumulate(err, s0 + u, e[u], b * 4 + (threadIdx.x >> 6));
}

// ---- windowed exact mode with the launch window staged in LDS ---------------------------------------------------------------
// k_hs_window pays one global round trip per time step: the step's stores have to reach L2 (s_waitcnt vmcnt(0)) before the
// barrier lets the next step load them -- ~1.5 us per step for ~200 instructions of work.  The schedule guarantees that
// everything a workgroup takes from ANOTHER workgroup was written in an earlier launch and is overwritten in a later one, so
// a workgroup can fetch everything its KW steps will touch when the launch starts -- all loads in flight together, one
// memory latency per launch -- and run the steps without global loads: the unknowns live in an LDS window (neighbours are
// LDS reads; an update goes to LDS for the workgroup's own later steps and, without waiting, to the in-place array and the
// sweep's snapshot for everybody else; the per-step barrier waits for LDS only), the constant operands of the KW pixels a
// thread will update wait in LDS slots of its own.  What the KW steps [q0, q0 + KW) of (sweep, row block b) touch
// (tools/check_sor_schedule.py --cover enumerates it, tests/test_host_logic.py checks it): unknowns on hyperplanes
// q0 - 7 .. q0 + KW + 2 of the skewed coordinate c i + j (the border pixels run up to 7 steps behind their own coordinate),
// rows b R - 2 .. b R + R.  Same per-pixel function, same operands: bit-identical to k_hs_window.
template <typename T, int KW> struct HsWinLds {
    static constexpr int NH = KW + 10;          // hyperplanes of unknowns in the window
    static constexpr int BACK = 7;              // window starts at q0 - BACK
    static size_t bytes(int nr, int nt)
    {
        return (size_t) nr * NH * sizeof(double2) + (size_t) nt * KW * (sizeof(double2) + sizeof(double));
    }
};
template <typename T, bool SNAP> struct ULds {
    typename Pix<T>::v2 *U, *snap;               // global arrays (hyperplane-major), written through
    double2 *win;                                // [NH][nr]  unknowns
    int nr, row0, h0;                            // LDS rows, image row of LDS row 0, hyperplane of LDS plane 0
    LaySkew lay;
    double2 a;                                   // constant operands of the pixel being updated (set per step)
    double dif;
    OFX_DEV double2 get(int ii, int jj) const { return win[(2 * ii + jj - h0) * nr + (ii - row0)]; }
    OFX_DEV void coef(const typename Pix<T>::v2 *, const T *, int, int, double2 &a_, double &dif_) const { a_ = a; dif_ = dif; }
    OFX_DEV void put(int i, int j, double2 v) const
    {
        win[(2 * i + j - h0) * nr + (i - row0)] = v;
        const size_t p = lay.idx(i, j);
        stn2(U + p, v);
        if (SNAP) stn2(snap + p, v);
    }
};
// the pixel plane item r updates at local step q in row block b, if any (the rule of k_hs_window)
OFX_DEV bool hs_window_pixel(const SorWin &w, int b, int r, int q, int qmax, int nx, int ny, int &pi, int &pj)
{
    return q >= 0 && q <= qmax && r >= 0 && r != ny + 2 && hs_plane_item(r, q, nx, ny, 0, pi, pj) &&
           (r < ny || sor_border_block(pi, ny, w.R) == b);
}
template <typename T, int KW, int MAXT>
__global__ __launch_bounds__(MAXT) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_hs_window_lds(
    typename Pix<T>::v2 *Ug, typename Pix<T>::v2 *snap, const typename Pix<T>::v2 *__restrict__ Ag, const T *__restrict__ Difg,
    double *__restrict__ errg, SorWin w, SorGrp grp, int s_cnt, int nx, int ny, double alpha2)
{
    using W = HsWinLds<T, KW>;
    extern __shared__ double2 hs_lds[];
    const int b = blockIdx.x, s = w.s_first + blockIdx.y, g = blockIdx.z;
    if (!((grp.runmask >> g) & 1u)) return;                      // this pair's solve has already stopped
    const int qmax = 2 * ny + nx - 2;
    const int q0 = w.tau0 - w.lag_s * s - w.lag_b * b;
    if (sor_unit_idle(w, b, q0, KW, 2, nx, ny)) return;          // no step of this (sweep, block) in the window: uniform
    typename Pix<T>::v2 *U = Ug + g * grp.npix;
    const typename Pix<T>::v2 *__restrict__ A = Ag + g * grp.npix;
    const T *__restrict__ Dif = Difg + g * grp.npix;
    typename Pix<T>::v2 *mysnap = snap + g * grp.snap_stride + (size_t) s * grp.npix;
    double *__restrict__ err = errg + (size_t) g * grp.err_stride;
    const int nr = w.R + 3, row0 = b * w.R - 2, h0 = q0 - W::BACK, t = threadIdx.x;
    const int nt = blockDim.x;
    double2 *win = hs_lds;                                       // [NH][nr] unknowns
    double2 *ca = hs_lds + W::NH * nr;                           // [KW][nt] (I2wx, I2wy) of the pixel thread t updates at step k
    double *cd = reinterpret_cast<double *>(ca + KW * nt);       // [KW][nt] dif
    const LaySkew lay = {ny, HS_PLANE_C_SKEW};
    const int r = sor_window_item(w, b, t, ny);
    // ---- fetch: thread t brings LDS row t (image row row0 + t) of every hyperplane of the window and the constant operands of
    // the KW pixels it will update; every load unconditional (entries outside the image / steps without a pixel read a
    // harmless address and are never used) and issued before the first use: one memory latency for the whole launch
    double2 u_in[W::NH], a_in[KW];
    double d_in[KW];
    {
        const int i = row0 + t, ic = i < 0 ? 0 : (i > ny - 1 ? ny - 1 : i);
        const int hmax = 2 * (ny - 1) + nx - 1;
#pragma unroll
        for (int k = 0; k < W::NH; k++) {
            const int h = h0 + k, hc = h < 0 ? 0 : (h > hmax ? hmax : h);
            u_in[k] = ldw2(U + (size_t) hc * ny + ic);
        }
#pragma unroll
        for (int k = 0; k < KW; k++) {
            int pi, pj;
            const bool have = hs_window_pixel(w, b, r, q0 + k, qmax, nx, ny, pi, pj);
            const size_t p = have ? lay.idx(pi, pj) : 0;
            a_in[k] = ldw2(A + p);
            d_in[k] = ldw(Dif + p);
        }
        if (t < nr) {
#pragma unroll
            for (int k = 0; k < W::NH; k++) win[k * nr + t] = u_in[k];
        }
#pragma unroll
        for (int k = 0; k < KW; k++) { ca[k * nt + t] = a_in[k]; cd[k * nt + t] = d_in[k]; }     // this thread's own slots
    }
    __syncthreads();
    ULds<T, true> acc = {U, mysnap, win, nr, row0, h0, lay, make_double2(0.0, 0.0), 0.0};
    double e = 0.0;
#pragma unroll 1
    for (int k = 0; k < KW; k++) {
        const int q = q0 + k;
        int pi, pj;
        if (hs_window_pixel(w, b, r, q, qmax, nx, ny, pi, pj)) {
            acc.a = ca[k * nt + t];
            acc.dif = cd[k * nt + t];
            e += hs_point_acc<T>(acc, A, Dif, pi, pj, nx, ny, alpha2);
        }
        if (q >= 0 && q <= qmax && r == ny + 2) {                // the corner item: up to four pixels, one after the other
            for (int corner = 0; corner < 4; corner++)
                if (hs_plane_item(r, q, nx, ny, corner, pi, pj) && sor_border_block(pi, ny, w.R) == b) {
                    const size_t p = lay.idx(pi, pj);            // four pixels per sweep: their operands come from memory
                    acc.a = ldw2(A + p);
                    acc.dif = ldw(Dif + p);
                    e += hs_point_acc<T>(acc, A, Dif, pi, pj, nx, ny, alpha2);
                }
        }
        // the next step reads this step's LDS writes: wait for LDS only (the global stores drain on their own)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    loop_accumulate(err, s, e, b * 4 + (t >> 6));
}

// the stopping test of every SOR loop of this file: sqrt(sum of squared updates / size) > TOL.  max_iter -- and chunk and
// fixed in the colour-order loops, which poll -- are the caller's.
static LoopSpec sor_loop_spec(int size, double TOL)
{
    return LoopSpec{/* max_iter */ 0, size, TOL, OFX_CRIT_SQRT_MEAN, /* chunk */ 0, /* fixed */ false, /* pairs */ false};
}

// Batch driver of the windowed exact mode.  launch(w, blocks, sweeps) enqueues one window over `blocks` row
// blocks x `sweeps` sweeps starting at w.s_first; take(n) makes snapshot n - 1 the current state.  Same contract
// as sor_exact_loop.  Spacing: lag_b = K between the row blocks of a sweep, lag_s = 2 K + C between sweeps (K + C
// when a sweep is one block): with these every value a workgroup reads from ANOTHER (sweep, block) was written
// at least one launch earlier and is overwritten at least one launch later (checked exhaustively on small
// images for both stencils, tools/check_sor_schedule.py).
// nz > 1 (temporal Brox): a sweep visits nz frames one after the other; frame number o (in visiting order) runs
// lag_f = K steps behind frame o - 1 and the sweeps move lag_f (nz - 1) further apart.
template <class WindowFn, class TakeFn>
static int sor_window_loop(ofx_ctx *ctx, int G, int size, int ny, double TOL, int maxiter, int qmax, int C, int batch,
                           WindowFn launch, TakeFn take, int *n_out, double *err_out, int nz = 1, int *hint = nullptr,
                           int Kdef = 0, int Rdef = 0)   // Kdef, Rdef: the caller's default steps per launch / rows per block (0 = the rule below)
{
    // G problems in lockstep (SorGrp): launch(w, blocks, sweeps, runmask, err_stride) serves every problem whose bit
    // is set; take(g, n) makes snapshot n - 1 of problem g its current state.  All problems start together, so the
    // ones still sweeping have all run the same number of full batches.
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "sor group of %d problems", G);
    // Measured on MI355X with the hyperplane-major layout (profiles/r02_e_sor_geometry_sweep.jsonl): a lone solve wants
    // many small workgroups (64 rows: more row blocks in flight along the latency chain), a lockstep group has enough
    // workgroups anyway and runs 6-10 % faster with 125 rows (+ the 3 border items = two full waves); 8 steps per launch,
    // 4 for the 4-neighbour stencil in a group (its sweeps are spaced C = 2 apart, so the 2 K lag dominates the pipeline).
    SorWin w;
    w.K = ctx->sor_window > 0 ? ctx->sor_window : (Kdef > 0 ? Kdef : ((G >= 4 && C <= 2) ? 4 : 8));
    w.R = ctx->sor_rows > 0 ? ctx->sor_rows : (Rdef > 0 ? Rdef : (G >= 4 ? 125 : 64));
    if (w.R < 2) w.R = 2;
    if (w.R > 1021) w.R = 1021;                                  // R + 3 threads per workgroup
    const int B = ofx_cdiv(ny, w.R);
    w.lag_b = w.K;
    w.lag_f = nz > 1 ? w.K : 0;
    w.lag_s = (B > 1 ? 2 * w.K : w.K) + C + w.lag_f * (nz - 1);
    const int per = batch + 1;                                   // error slots per problem
    OFX_TRY(ofx_loop_reserve(ctx, G * per));
    LoopSpec LS = sor_loop_spec(size, TOL);
    // Every sweep of a batch costs lag_s steps of pipeline whether it is needed or not, so batches are sized, not
    // maximal (`batch` is the snapshot capacity): the first one from the sweep count of the previous solve at this level
    // (*hint = the largest of the group; consecutive warps / outer iterations converge in similar, usually decreasing,
    // numbers of sweeps) with 25 % + 2 of head room, 32 without a hint; a solve that needs more runs further,
    // half-sized batches.
    int first = batch < 32 ? batch : 32;
    if (ctx->sor_batch > 0) first = batch;                       // explicit option: fixed batches
    else if (hint && *hint > 0) {
        first = *hint + *hint / 4 + 2;
        first = first < 8 ? 8 : (first > batch ? batch : first);
    }
    const int later = ctx->sor_batch > 0 ? batch : (first / 2 < 8 ? (batch < 8 ? batch : 8) : first / 2);
    int niter = 0;                                               // sweeps of the problems that are still active
    unsigned active = (1000 > TOL && maxiter > 0) ? ((G >= 32) ? 0xFFFFFFFFu : ((1u << G) - 1u)) : 0u;
    for (int g = 0; g < G; g++) { n_out[g] = 0; err_out[g] = 1000; }                       // :140 / :312
    while (active) {
        const int want = niter == 0 ? first : later;
        const int ns = (maxiter - niter < want) ? maxiter - niter : want;
        OFX_TRY(ofx_loop_clear(ctx, (size_t) G * per));
        const long tail = (long) w.lag_b * (B - 1) + (long) w.lag_f * (nz - 1);   // the last unit of a sweep ends this much later
        const long total = (long) qmax + 1 + tail + (long) w.lag_s * (ns - 1);
        // Temporal Brox promises a sequence of a lockstep group the stopping VALUES of its lone solve, while a group sizes its
        // batches from the largest hint of its members.  Which steps of a sweep share a launch -- the association of its stopping
        // sum -- depends on (lag_s * s) mod K for its number s within the batch, so a later batch starts its windows up to K - 1
        // steps early: the windows then cut every sweep where the sweep's number in the SOLVE puts them, whatever the batch sizes.
        const long t_first = nz > 1 ? -(((long) w.lag_s * niter) % w.K) : 0;
        for (long tau0 = t_first; tau0 < total; tau0 += w.K) {
            long s_lo = (tau0 - qmax - tail + w.lag_s - 1) / w.lag_s;   // smallest s still inside the image
            if (tau0 - qmax - tail < 0) s_lo = 0;
            long s_hi = (tau0 + w.K - 1) / w.lag_s;              // largest s that has started
            if (s_hi > ns - 1) s_hi = ns - 1;
            if (s_hi < s_lo) continue;
            w.tau0 = (int) tau0;
            w.s_first = (int) s_lo;
            OFX_TRY(launch(w, B, (int) (s_hi - s_lo + 1), active, per * OFX_NSHARD));
        }
        LS.max_iter = ns;
        OfxPoll poll;
        OfxIterState fin[OFX_MAX_GROUP];
        OFX_TRY(ofx_poll_issue(ctx, [&](OfxIterState *slot, int seq) -> int { return ofx_loop_finalize_group(ctx, LS, G, per, 0, ns, slot, seq); }, &poll));
        OFX_TRY(ofx_poll_read(ctx, poll, G, false, fin));       // nothing in flight behind it: the event alone
        for (int g = 0; g < G; g++) {
            if (!((active >> g) & 1u)) continue;
            const OfxIterState &st = fin[g];
            if (st.n < ns) OFX_TRY(take(g, st.n));              // stopped inside the batch: the state is snapshot n - 1
            n_out[g] = niter + st.n;
            err_out[g] = st.error;
            if (!(st.error > TOL && n_out[g] < maxiter)) active &= ~(1u << g);
        }
        niter += ns;
    }
    if (hint) {
        int h = 0;
        for (int g = 0; g < G; g++) h = n_out[g] > h ? n_out[g] : h;
        *hint = h;
    }
    return OFX_OK;
}

// Exact SOR loop:  while (error > TOL && n < maxiter) sweep.   Sweeps run in batches of up to `batch`
// pipelined sweeps (launch_plane(t, s_lo, s_cnt) = one time step).  The per-sweep errors of a batch are
// only known when it has drained, so a batch that ran past the stopping sweep is rolled back to its
// checkpoint (a copy of the unknowns taken before the batch) and re-run with exactly the sweeps that
// count.  qmax = largest pos() of the image, C = sweep spacing.
template <class PlaneFn, class SaveFn, class RestoreFn>
static int sor_exact_loop(ofx_ctx *ctx, int size, double TOL, int maxiter, int qmax, int C, PlaneFn launch_plane,
                          SaveFn save, RestoreFn restore, int *n_out, double *err_out)
{
    int niter = 0;
    double error = 1000;
    const int batch = ctx->sor_batch > 0 ? ctx->sor_batch : 64;
    OFX_TRY(ofx_loop_reserve(ctx, batch + 1));
    LoopSpec LS = sor_loop_spec(size, TOL);
    auto run_batch = [&](int ns, OfxIterState *out) -> int {
        OFX_TRY(ofx_loop_clear(ctx, (size_t) ns));
        const int tmax = qmax + C * (ns - 1);
        for (int t = 0; t <= tmax; t++) {
            int s_lo = (t - qmax + C - 1) / C;                 // smallest s with t - C s <= qmax
            if (t - qmax < 0) s_lo = 0;
            int s_hi = t / C;
            if (s_hi > ns - 1) s_hi = ns - 1;
            if (s_hi < s_lo) continue;
            OFX_TRY(launch_plane(t, s_lo, s_hi - s_lo + 1));
        }
        LS.max_iter = ns;
        // (this loop used to take the sequence number behind the increment of the count, one more than the other loops' polls
        // carry; nothing waits on the number here -- the read below waits on the event alone -- so nothing observable changed)
        OfxPoll poll;
        OFX_TRY(ofx_poll_issue(ctx, [&](OfxIterState *slot, int seq) -> int { return ofx_loop_finalize_group(ctx, LS, 1, 0, 0, ns, slot, seq); }, &poll));
        return ofx_poll_read(ctx, poll, 1, false, out);
    };
    while (error > TOL && niter < maxiter) {
        const int b = (maxiter - niter < batch) ? maxiter - niter : batch;
        OFX_TRY(save());
        OfxIterState st;
        OFX_TRY(run_batch(b, &st));
        if (st.n < b) {                                        // stopped inside the batch: redo exactly st.n sweeps
            const int used = st.n;
            OFX_TRY(restore());
            OFX_TRY(run_batch(used, &st));
            st.n = used;
        }
        niter += st.n;
        error = st.error;
    }
    *n_out = niter;
    *err_out = error;
    return OFX_OK;
}

// snapshot capacity (= most sweeps in one batch) of the windowed mode: option "sor_batch", else 64, capped by maxiter,
// by ~4 GiB of snapshots per pair and -- for all pairs of a lockstep group -- by a third of the device memory that is
// free right now, shared between the contexts expected to solve concurrently (option "concurrency"; the batch entry
// points set it to their number of contexts)
static int sor_pick_batch(const ofx_ctx *ctx, size_t npix, size_t elem_bytes, int maxiter, int G = 1)
{
    int b = ctx->sor_batch > 0 ? ctx->sor_batch : 64;
    const double cap = (double) ((size_t) 4 << 30);
    double cap_group = (double) ((size_t) 40 << 30);
    size_t mfree = 0, mtotal = 0;
    if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess) {
        const double share = 0.33 * (double) mfree / (ctx->concurrency > 1 ? ctx->concurrency : 1);
        if (share < cap_group) cap_group = share;
    } else {
        (void) hipGetLastError();
    }
    const double plane = (double) npix * (double) elem_bytes;
    while (b > 8 && (b * plane > cap || b * plane * G > cap_group)) b /= 2;
    while (b > 1 && b * plane > cap) b /= 2;
    if (b > maxiter) b = maxiter;
    return b < 1 ? 1 : b;
}
// sweeps per workgroup of the windowed kernels: option "sor_spw" (1, 2 or 4), default 1.  Measured with 16 pairs in
// lockstep (profiles/r02_i_sor_sweeps_per_workgroup.jsonl): 2 / 4 sweeps per workgroup -- their loads issued together,
// one store drain + barrier per step for all of them -- run at 0.66x / 0.47x the throughput of 1 (HS 23.9k -> 15.7k ->
// 11.2k Mpix*sweeps/s): the operands of two updates take 151 VGPRs = 3 waves per SIMD instead of 8 at 64, and the
// per-step latency is hidden by resident waves, not by instruction-level parallelism inside one.
static int sor_pick_spw(const ofx_ctx *ctx)
{
    if (ctx->sor_spw == 1 || ctx->sor_spw == 2 || ctx->sor_spw == 4) return ctx->sor_spw;
    return 1;
}
// Which windowed kernel: option "sor_lds" = 0 the per-step global round trip (k_*_window), 2 the LDS-staged launch window
// (k_*_window_lds), 1 (default) by measurement: the LDS window for a lone solve -- a latency chain, where one memory latency
// per launch instead of one per step counts -- and the global kernels for lockstep groups of 4 pairs and more, which are
// bound by resident waves (28 per CU at 64 VGPRs and no LDS against a few LDS-limited workgroups).
// Measured (profiles/r03_e_sor_window_kernels_lds_vs_global.txt, 16 P1 pairs of cfg 3 / cfg 4): Horn-Schunck lone solves
// 572 -> 537 ms with 8 steps per launch (16: 617), lockstep groups of 16 81 -> 147 ms per pair (116 since idle units leave at
// once, profiles/r03_n_hs_window_kernels_counters.txt: 800 resident waves against 2400); Brox lone solves 255 -> 297 ms.
// A step is bound by the ~200 dependent instructions of a lone wave, not by the round trip the window removes.
// lds_for_small_groups: whether sor_lds = 1 takes the LDS window for groups of fewer than 4 (Horn-Schunck does, Brox does not)
static bool sor_use_lds(const ofx_ctx *ctx, int G, bool lds_for_small_groups)
{
    return ctx->sor_lds == 2 || (ctx->sor_lds == 1 && G < 4 && lds_for_small_groups);
}
static int sor_window_threads(int n_items)
{
    const int t = ofx_cdiv(n_items, 64) * 64;
    return t > 1024 ? 1024 : t;
}

// makes *snap hold `batch` snapshot planes of `plane` elements for each of G problems
template <typename V> static int sor_snap_reserve(ofx_ctx *ctx, V **snap, int *planes, size_t plane, int batch, int G)
{
    if (*planes >= batch) return OFX_OK;
    OFX_TRY(ofx_alloc(ctx, plane * batch * G, snap));
    *planes = batch;
    return OFX_OK;
}

// one finished solve (number `solve` of level `scale`) in the work records of the G problems that ran it
static void sor_record_solve(ofx_stats *stats, int G, int scale, int solve, const int *niter, const double *error, float ms,
                             double pixels)
{
    for (int g = 0; g < G; g++) {
        ofx_stats &S = stats[g];
        if (scale < OFX_MAX_SCALES) {
            if (solve < OFX_MAX_SOLVES) { S.iters[scale][solve] = niter[g]; S.error[scale][solve] = error[g]; }
            S.iter_ms[scale] += ms;
            S.iter_launches[scale] += niter[g];
        }
        S.work_pix_iters += (double) niter[g] * pixels;
    }
}

// ---- the exact-mode solve, once for both stencils (S: HsExact, BroxExact) ------------------------------------------------------

// one launch of an exact-mode kernel; dynamic LDS beyond 64 KiB has to be granted to the kernel first
template <class... KA, class... A>
static int sor_launch(ofx_ctx *ctx, void (*kernel)(KA...), dim3 grid, dim3 blk, size_t lds, A... args)
{
    if (lds > 64 * 1024)
        OFX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int) lds));
    hipLaunchKernelGGL(kernel, grid, blk, lds, ctx->stream, args...);
    OFX_LAUNCH_CHECK(ctx);
    return OFX_OK;
}

// the LDS window of KW steps, if that is the launch's length and its footprint fits the 160 KiB of a CU (*done: launched)
template <class S, int KW>
static int sor_window_lds(ofx_ctx *ctx, const S &st, const SorWin &w, const SorGrp &grp, dim3 grid, dim3 blk, int sweeps, bool *done)
{
    const size_t lds = S::template Lds<KW>::bytes(w.R + 3, (int) blk.x);
    *done = w.K == KW && lds <= 160 * 1024;
    return *done ? st.launch(ctx, S::template window_lds<KW>, grid, blk, lds, w, grp, sweeps) : OFX_OK;
}

// One window of `sweeps` sweeps x `blocks` row blocks x G problems: the launch window staged in LDS (one sweep per workgroup,
// steps on LDS only) where sor_use_lds asks for it and a kernel of w.K steps exists, up to 253 rows fit its 256 threads and the
// footprint fits the LDS; else the global kernel with option sor_spw's sweeps per workgroup.
template <class S>
static int sor_window_launch(ofx_ctx *ctx, const S &st, const SorWin &w, const SorGrp &grp, int blocks, int sweeps, int G)
{
    const dim3 blk(sor_window_threads(w.R + 3));
    if constexpr (S::ONE_KERNEL) {
        return st.launch(ctx, S::template window<1, 1024>, dim3(blocks, sweeps, G), blk, 0, w, grp, sweeps);
    } else {
        if (sor_use_lds(ctx, G, S::LDS_FOR_SMALL_GROUPS) && w.R + 3 <= 256) {
            const dim3 grid(blocks, sweeps, G);
            bool done = false;
            int s = sor_window_lds<S, S::LDS_K[0]>(ctx, st, w, grp, grid, blk, sweeps, &done);
            if (!done) s = sor_window_lds<S, S::LDS_K[1]>(ctx, st, w, grp, grid, blk, sweeps, &done);
            if (!done) s = sor_window_lds<S, S::LDS_K[2]>(ctx, st, w, grp, grid, blk, sweeps, &done);
            if (done) return s;
        }
        const int spw = sor_pick_spw(ctx);
        // workgroups of up to 128 threads (the default geometries) are compiled without the 128-VGPR cap that a 1024-thread
        // bound implies: two sweeps per workgroup keep their operands in registers instead of spilling.  One sweep per
        // workgroup: the 64-VGPR build, 8 waves per SIMD.
        const bool small = blk.x <= 128;
        const auto k = spw == 4   ? (small ? S::template window<4, 128> : S::template window<4, 1024>)
                       : spw == 2 ? (small ? S::template window<2, 128> : S::template window<2, 1024>)
                                  : S::template window<1, 1024>;
        return st.launch(ctx, k, dim3(blocks, ofx_cdiv(sweeps, spw), G), blk, 0, w, grp, sweeps);
    }
}

// sor_exact_solve<S> runs one solve of the G problems of a lockstep group in the reference's sweep order: option sor_exact = 1
// on hyperplane-major copies through sor_window_loop, anything else one launch per time step through sor_exact_loop (lone
// problems).  S -- HsExact, BroxExact -- is bound to a level and carries what differs between the solvers:
//   SKEW, C         hyperplane of pixel (i, j) = SKEW i + j (LaySkew; the stencil skew of sor_unit_idle); steps between sweeps
//   qmax(nx, ny)    the last step of a sweep
//   LDS_K, Lds<KW>  the window lengths k_*_window_lds is instantiated for and the footprint Lds<KW>::bytes(rows + 3, threads)
//   LDS_FOR_SMALL_GROUPS   whether option sor_lds = 1 takes the LDS window for groups of fewer than 4 (sor_use_lds)
//   ONE_KERNEL      robust_expo: k_brox_window<T, 1, 1024, true> whatever sor_lds and sor_spw say
//   u(), us(), ck() the unknowns row-major, hyperplane-major, and the checkpoint of the one-launch-per-step path
//   skew_in()       allocates the level's hyperplane-major planes on first use (it writes L.Us, ...) and copies every operand in
//   window<SPW, MAXT>, window_lds<KW>, launch(); plane()   the window kernels and their launcher; the plane kernel's launcher
// size: pixels the stopping sum is divided by; Kdef, Rdef: see sor_window_loop; niter[g], error[g]: sweeps and last stopping
// value of problem g; ms (windowed only), when given: the windows of this solve between two drained streams on the host's clock
// (so with the polls of the stopping test) -- every other caller keeps its schedule
template <class S>
static int sor_exact_solve(ofx_ctx *ctx, const S &st, int G, int size, double TOL, int maxiter, int Kdef, int Rdef, int *niter,
                           double *error, float *ms)
{
    using v2 = typename S::v2;
    auto &L = st.L;
    const int nx = L.nx, ny = L.ny, qmax = S::qmax(nx, ny);
    if (ctx->sor_exact != 1) {
        // one launch per time step (option sor_exact = 2): the reference implementation of the exact schedule
        const size_t ub = (size_t) nx * ny * sizeof(v2);
        auto plane = [&](int t, int s_lo, int s_cnt) -> int { return st.plane(ctx, t, s_lo, s_cnt); };
        auto copy = [&](v2 *dst, const v2 *src) -> int {
            OFX_HIP(ctx, hipMemcpyAsync(dst, src, ub, hipMemcpyDeviceToDevice, ctx->stream));
            return OFX_OK;
        };
        return sor_exact_loop(ctx, size, TOL, maxiter, qmax, S::C, plane, [&] { return copy(st.ck(), st.u()); },
                              [&] { return copy(st.u(), st.ck()); }, niter, error);
    }
    // windowed (default): the sweeps run on hyperplane-major copies of the unknowns and the constant operands
    const size_t ps = skew_plane_elems(nx, ny, S::SKEW);
    const int batch = sor_pick_batch(ctx, ps, sizeof(v2), maxiter, G);
    OFX_TRY(st.skew_in(ctx, ps, G));
    OFX_TRY(sor_snap_reserve(ctx, &L.Snap, &L.snap_planes, ps, batch, G));
    const size_t snap_stride = ps * L.snap_planes;
    auto window = [&](const SorWin &w, int blocks, int sweeps, unsigned runmask, int err_stride) -> int {
        const SorGrp grp = {runmask, err_stride, ps, snap_stride};
        return sor_window_launch(ctx, st, w, grp, blocks, sweeps, G);
    };
    auto take = [&](int g, int n) -> int {
        OFX_HIP(ctx, hipMemcpyAsync(st.us() + g * ps, L.Snap + g * snap_stride + (size_t) (n - 1) * ps, ps * sizeof(v2),
                                    hipMemcpyDeviceToDevice, ctx->stream));
        return OFX_OK;
    };
    if (ms) OFX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double t0 = ofx_now_ms();
    OFX_TRY(sor_window_loop(ctx, G, size, ny, TOL, maxiter, qmax, S::C, batch, window, take, niter, error, 1, &L.sweep_hint, Kdef,
                            Rdef));
    if (ms) {
        OFX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *ms = (float) (ofx_now_ms() - t0);
    }
    return op_skew<v2, false>(ctx, st.us(), st.u(), nx, ny, S::SKEW, G);
}

// One level of a lockstep group: every array holds G pairs back to back (pair g at element g * nx * ny).
template <typename T> struct HsLevel {
    int nx, ny, G;
    T *I1, *I2;
    typename Pix<T>::v2 *pa;    // (I2, I2x)
    T *pb;                      // I2y
    typename Pix<T>::v2 *U, *A, *Uck;
    T *Dif;
    // windowed exact mode, hyperplane-major (LaySkew) and allocated on first use: the unknowns, the coefficients and
    // snap_planes snapshot planes per pair
    typename Pix<T>::v2 *Us, *As, *Snap;
    T *Difs;
    int snap_planes;
    int sweep_hint;             // sweeps of the previous solve at this level (sizes the next first batch)
    unsigned cur;               // tile sweeps (sor_exact = 0): bit g set = the flow of pair g lives in Uck, not U
    size_t n() const { return (size_t) nx * ny; }
    typename Pix<T>::v2 *flow(int g) const { return (((cur >> g) & 1u) ? Uck : U) + (size_t) g * n(); }
};

template <typename T> static int hs_level_alloc(ofx_ctx *ctx, HsLevel<T> &L, int nx, int ny, int G, bool images)
{
    const size_t n = (size_t) nx * ny * G;
    L.nx = nx;
    L.ny = ny;
    L.G = G;
    L.I1 = L.I2 = nullptr;
    if (images) {
        OFX_TRY(ofx_alloc(ctx, n, &L.I1));
        OFX_TRY(ofx_alloc(ctx, n, &L.I2));
    }
    OFX_TRY(ofx_alloc(ctx, n, &L.pa));
    OFX_TRY(ofx_alloc(ctx, n, &L.pb));
    OFX_TRY(ofx_alloc(ctx, n, &L.U));
    OFX_TRY(ofx_alloc(ctx, n, &L.Uck));
    OFX_TRY(ofx_alloc(ctx, n, &L.A));
    OFX_TRY(ofx_alloc(ctx, n, &L.Dif));
    L.Snap = L.Us = L.As = nullptr;
    L.Difs = nullptr;
    L.snap_planes = 0;
    L.sweep_hint = 0;
    L.cur = 0;
    return OFX_OK;
}

struct HsParams {
    double alpha, TOL;
    int warps, maxiter, verbose;
};

// Horn-Schunck's side of sor_exact_solve: unknowns U, constant operands A, Dif, alpha^2 as the kernels' scalar.  L is the
// level itself, not a copy: skew_in() gives it its hyperplane-major planes (Us, As, Difs), the driver its snapshot planes
template <typename T> struct HsExact {
    using v2 = typename Pix<T>::v2;
    static constexpr int SKEW = HS_PLANE_C_SKEW, C = HS_PLANE_C;
    static constexpr int LDS_K[3] = {8, 16, 24};
    static constexpr bool LDS_FOR_SMALL_GROUPS = true, ONE_KERNEL = false;
    template <int KW> using Lds = HsWinLds<T, KW>;
    static int qmax(int nx, int ny) { return 2 * ny + nx - 2; }
    HsLevel<T> &L;
    double alpha2;
    v2 *u() const { return L.U; }
    v2 *us() const { return L.Us; }
    v2 *ck() const { return L.Uck; }
    int skew_in(ofx_ctx *ctx, size_t ps, int G) const
    {
        if (!L.Us) {
            OFX_TRY(ofx_alloc(ctx, ps * G, &L.Us));
            OFX_TRY(ofx_alloc(ctx, ps * G, &L.As));
            OFX_TRY(ofx_alloc(ctx, ps * G, &L.Difs));
        }
        OFX_TRY((op_skew<v2, true>(ctx, L.U, L.Us, L.nx, L.ny, SKEW, G)));
        OFX_TRY((op_skew<v2, true>(ctx, L.A, L.As, L.nx, L.ny, SKEW, G)));
        return op_skew<T, true>(ctx, L.Dif, L.Difs, L.nx, L.ny, SKEW, G);
    }
    template <int SPW, int MAXT> static constexpr auto window = k_hs_window<T, SPW, MAXT>;
    template <int KW> static constexpr auto window_lds = k_hs_window_lds<T, KW, 256>;
    template <class Kernel>
    int launch(ofx_ctx *ctx, Kernel k, dim3 grid, dim3 blk, size_t lds, const SorWin &w, const SorGrp &grp, int sweeps) const
    {
        return sor_launch(ctx, k, grid, blk, lds, L.Us, L.Snap, L.As, L.Difs, ctx->d_err, w, grp, sweeps, L.nx, L.ny, alpha2);
    }
    int plane(ofx_ctx *ctx, int t, int s_lo, int s_cnt) const
    {
        return sor_launch(ctx, k_hs_plane<T>, dim3(ofx_cdiv(L.ny + 3, 64), s_cnt), dim3(64), 0, L.U, L.A, L.Dif, ctx->d_err, t, s_lo,
                          L.nx, L.ny, alpha2);
    }
};

// src/horn_schunck_pyramidal.cpp:78-249 on device data for the G pairs of a lockstep group; L.U holds the incoming
// flows; stats[g] = work record of pair g.
template <typename T>
static int hs_single_scale_dev(ofx_ctx *ctx, HsLevel<T> &L, const HsParams &P, int scale, ofx_stats *stats)
{
    const int nx = L.nx, ny = L.ny, G = L.G;
    const size_t npix = L.n();
    const double alpha2 = P.alpha * P.alpha;
    if (P.verbose && G == 1)
        fprintf(stderr, "Single-scale Horn-Schunck of a %dx%d image\n\ta=%g nw=%d eps=%g mi=%d v=%d\n", nx, ny, P.alpha,
                P.warps, P.TOL, P.maxiter, P.verbose);
    const bool windowed = ctx->sor_exact == 1 && nx >= 3 && ny >= 3;
    const bool tiled = ctx->sor_exact == 0 && ctx->sor_fuse >= 0;        // colour order, K sweeps per launch (ofx_sor_tile.hip)
    if (G > 1 && !windowed && !tiled)
        return ofx_fail(ctx, OFX_ERR_ARG, "hs: lockstep groups need sor_exact = 1 (levels of at least 3x3, this one %dx%d) or the tile sweeps of sor_exact = 0", nx, ny);
    for (int g = 0; g < G; g++)
        OFX_TRY(op_grad_pack<T>(ctx, L.I2 + g * npix, L.pa + g * npix, L.pb + g * npix, nx, ny));      // :114
    const dim3 gw(ofx_cdiv(nx, 64), ofx_cdiv(ny, 4), G);
    const dim3 gc(ofx_cdiv(ofx_cdiv(nx, 2), 64), ofx_cdiv(ofx_cdiv(ny, 2), 4));
    for (int w = 0; w < P.warps; w++) {
        if (P.verbose && G == 1) fprintf(stderr, "Warping %d:", w);
        hipLaunchKernelGGL(k_hs_warp<T>, gw, b2d(), 0, ctx->stream, L.pa, (const T *) L.pb, (const T *) L.I1, L.U, L.Uck, L.cur,
                           L.A, L.Dif, nx, ny);                                               // :123-137
        OFX_LAUNCH_CHECK(ctx);
        int niter[OFX_MAX_GROUP] = {0};
        double error[OFX_MAX_GROUP];
        for (int g = 0; g < G; g++) error[g] = 1000;                                          // :140
        float ms = 0.f;
        if (tiled) {
            OFX_TRY(ofx_hs_tile_solve<T>(ctx, G, L.U, L.Uck, &L.cur, L.A, (const T *) L.Dif, nx, ny, alpha2, P.TOL, P.maxiter,
                                         ctx->sor_fuse, niter, error, ctx->profile ? &ms : nullptr));
        } else if (ctx->sor_exact && nx >= 3 && ny >= 3) {
            OFX_TRY(sor_exact_solve(ctx, HsExact<T>{L, alpha2}, G, nx * ny, P.TOL, P.maxiter, 0, 0, niter, error, nullptr));
        } else if (P.maxiter > 0 && error[0] > P.TOL) {
            LoopSpec LS = sor_loop_spec(nx * ny, P.TOL);
            LS.max_iter = P.maxiter;
            LS.chunk = sor_pick_chunk(ctx, nx, ny, 4);
            LS.fixed = ctx->fixed_work != 0;
            auto launch = [&](int k, int, double thr) -> int {
                for (int col = 0; col < 4; col++)
                    hipLaunchKernelGGL(k_hs_sor<T>, gc, b2d(), 0, ctx->stream, L.U, L.A, (const T *) L.Dif, ctx->d_err, k,
                                       nx, ny, col >> 1, col & 1, alpha2, thr);
                OFX_LAUNCH_CHECK(ctx);
                return OFX_OK;
            };
            OFX_TRY(ofx_run_loop(ctx, LS, launch, [](int) { return OFX_OK; }, &niter[0], &error[0], ctx->profile ? &ms : nullptr));
        }
        if (P.verbose && G == 1) fprintf(stderr, "Iterations %d (%g)\n", niter[0], error[0]);   // :233-235
        sor_record_solve(stats, G, scale, w, niter, error, ms, (double) nx * ny);
    }
    return OFX_OK;
}

template <typename T>
static int download_flow(ofx_ctx *ctx, const typename Pix<T>::v2 *U, double *u, double *v, size_t n)
{
    double *d1, *d2;
    OFX_TRY(ofx_alloc(ctx, n, &d1));
    OFX_TRY(ofx_alloc(ctx, n, &d2));
    OFX_TRY(op_deinterleave2<T>(ctx, U, d1, d2, n));
    OFX_HIP(ctx, hipMemcpyAsync(u, d1, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    OFX_HIP(ctx, hipMemcpyAsync(v, d2, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    OFX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return OFX_OK;
}

template <typename T>
static int hs_single_scale_host(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx, int ny,
                                const HsParams &P)
{
    const size_t n = (size_t) nx * ny;
    ofx_stats_begin(&ctx->stats, 1, P.warps);
    ctx->stats.nx[0] = nx;
    ctx->stats.ny[0] = ny;
    HsLevel<T> L;
    OFX_TRY(hs_level_alloc<T>(ctx, L, nx, ny, 1, false));
    OFX_TRY(upload_plane<T>(ctx, I1, n, &L.I1));
    OFX_TRY(upload_plane<T>(ctx, I2, n, &L.I2));
    double *d1, *d2;
    OFX_TRY(ofx_alloc(ctx, n, &d1));
    OFX_TRY(ofx_alloc(ctx, n, &d2));
    OFX_HIP(ctx, hipMemcpyAsync(d1, u, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    OFX_HIP(ctx, hipMemcpyAsync(d2, v, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    OFX_TRY(op_interleave2<T>(ctx, d1, d2, L.U, n));
    OFX_TRY(hs_single_scale_dev<T>(ctx, L, P, 0, &ctx->stats));
    return download_flow<T>(ctx, L.flow(0), u, v, n);
}

// src/horn_schunck_pyramidal.cpp:258-370 for G pairs in lockstep.  dI1[g] / dI2[g]: device images of storage type T.
// On success lv[0].flow(g) holds the flow of pair g.
template <typename T>
static int hs_pyramidal_dev(ofx_ctx *ctx, int G, const T *const *dI1, const T *const *dI2, int nx, int ny, const HsParams &P,
                            int nscales, double zfactor, std::vector<HsLevel<T>> &lv, ofx_stats *stats, int kind = -1,
                            size_t pitch = 0,               // kind >= 0: bytes between the images' rows, 0 = dense
                            const void *const *init = nullptr)     // G start payloads (NULL entry: zero start); nullptr: all zero
{
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "hs: group of %d pairs", G);
    if (P.verbose && G == 1)
        fprintf(stderr, "Multiscale Horn-Schunck of a %dx%d pair\n\ta=%g ns=%d zf=%g nw=%d eps=%g mi=%d\n", nx, ny,
                P.alpha, nscales, zfactor, P.warps, P.TOL, P.maxiter);
    using V2 = typename Pix<T>::v2;
    auto levels = [&](const std::vector<int> &nxs, const std::vector<int> &nys, T **lA, T **lB, V2 **U) -> int {
        lv.resize(nscales);
        for (int s = 0; s < nscales; s++) {
            OFX_TRY(hs_level_alloc<T>(ctx, lv[s], nxs[s], nys[s], G, true));
            lA[s] = lv[s].I1;
            lB[s] = lv[s].I2;
        }
        *U = lv[nscales - 1].U;
        return OFX_OK;
    };
    OFX_TRY(ofx_pyramid_head<T>(ctx, G, G, (const void *const *) dI1, (const void *const *) dI2, nx, ny, nscales, zfactor,
                                HS_PRESMOOTH_SIGMA, P.warps, stats, kind, pitch, init, levels));               // :279-323
    for (int s = nscales - 1; s >= 0; s--) {                                                           // :326
        if (P.verbose && G == 1) fprintf(stderr, "Scale: %d %dx%d\n", s, lv[s].nx, lv[s].ny);
        OFX_TRY(hs_single_scale_dev<T>(ctx, lv[s], P, s, stats));
        if (!s) break;
        for (int g = 0; g < G; g++)
            OFX_TRY(op_zoom_in_flow<T>(ctx, lv[s].flow(g), lv[s - 1].U + g * lv[s - 1].n(), lv[s].nx, lv[s].ny,
                                       lv[s - 1].nx, lv[s - 1].ny, 1.0 / zfactor));                    // :345-352
    }
    return OFX_OK;
}

template <typename T>
static int hs_pyramidal_host(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx, int ny,
                             const HsParams &P, int nscales, double zfactor)
{
    const size_t n = (size_t) nx * ny;
    T *dI1, *dI2;
    OFX_TRY(upload_plane<T>(ctx, I1, n, &dI1));
    OFX_TRY(upload_plane<T>(ctx, I2, n, &dI2));
    std::vector<HsLevel<T>> lv;
    const T *a = dI1, *b = dI2;
    OFX_TRY(hs_pyramidal_dev<T>(ctx, 1, &a, &b, nx, ny, P, nscales, zfactor, lv, &ctx->stats));
    return download_flow<T>(ctx, lv[0].flow(0), u, v, n);
}

// ---- the pair entries of Horn-Schunck and Brox, written once over ofx_pairs.h ----
// A solver S brings: Params and Level<T>; who (opens its messages); check(ctx, P), its parameters' refusals; pyramid<T>, its
// coarse-to-fine driver (hs_pyramidal_dev / brox_spatial_dev); flow<T>(L, g), where the flow of pair g lies in the finest level.
struct HsPairs {
    using Params = HsParams;
    template <typename T> using Level = HsLevel<T>;
    static constexpr const char *who = "hs";
    static int check(ofx_ctx *ctx, const HsParams &P)
    {
        if (P.warps < 1) return ofx_fail(ctx, OFX_ERR_ARG, "hs: warps=%d", P.warps);
        if (P.maxiter > OFX_HS_MAX_MAXITER) return ofx_fail(ctx, OFX_ERR_ARG, "hs: maxiter > %d", OFX_HS_MAX_MAXITER);
        return OFX_OK;
    }
    template <typename T, class... A> static int pyramid(A &&...a) { return hs_pyramidal_dev<T>(a...); }
    template <typename T> static const typename Pix<T>::v2 *flow(const HsLevel<T> &L, int g) { return L.flow(g); }
};

// stage -> pyramid -> payloads -> unstage.  stage_all: the video chain, whose frames and payloads may lie anywhere
template <class S, typename T>
static int sor_pair_devapi(ofx_ctx *ctx, int G, const void *const *dI1, const void *const *dI2, void *const *d_flo, int nx, int ny,
                           const typename S::Params &P, int nscales, double z, ofx_stats *stats,
                           const void *const *init_in,      // G start payloads (NULL entry: zero start), or nullptr
                           bool stage_all)
{
    const size_t n = (size_t) nx * ny;
    OfxPairIO io;
    OFX_TRY(ofx_pairs_stage(ctx, G, dI1, dI2, init_in, d_flo, nx, ny, stage_all, io));
    std::vector<typename S::template Level<T>> lv;
    OFX_TRY(S::template pyramid<T>(ctx, G, (const T *const *) io.a, (const T *const *) io.b, nx, ny, P, nscales, z, lv, stats, io.kind,
                                   io.pitch, init_in ? io.init : nullptr));
    for (int g = 0; g < G; g++) OFX_TRY(op_to_flo<T>(ctx, S::template flow<T>(lv[0], g), (float2 *) io.flo[g], n));
    return ofx_pairs_unstage(ctx, G, d_flo, io, n);
}

// the lockstep group behind ofx_*_group_dev (d_flo_init = nullptr), ofx_*_group_init_dev and every step of a chain (stage_all)
template <class S>
static int sor_pair_group(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2, const void *const *d_flo_init,
                          void *const *d_flo, int nx, int ny, const typename S::Params &P, int nscales, double z,
                          ofx_stats *stats_out, bool stage_all = false)
{
    OFX_ENTER(ctx);
    auto check = [&]() -> int {
        OFX_TRY(S::check(ctx, P));
        OFX_TRY(ofx_pitch_check(ctx, S::who, nx));
        return ofx_start_check(ctx, S::who, n_pairs, d_flo_init, nx, ny, nscales, z);
    };
    return ofx_pair_group_entry(ctx, S::who, n_pairs, dI1, dI2, d_flo, stats_out, check, [&](ofx_stats *st) {
        return ctx->precision == OFX_F64
                   ? sor_pair_devapi<S, double>(ctx, n_pairs, dI1, dI2, d_flo, nx, ny, P, nscales, z, st, d_flo_init, stage_all)
                   : sor_pair_devapi<S, float>(ctx, n_pairs, dI1, dI2, d_flo, nx, ny, P, nscales, z, st, d_flo_init, stage_all);
    });
}

// ---- batches of pairs for the SOR solvers: lockstep groups over the contexts (ofx_run_groups, with the `concurrency` hint:
// memory budgets are shared between the workers) ----
// group size: option "lockstep" of ctxs[0], else as large as possible (16), evened out over the contexts
static int sor_batch_group_size(ofx_ctx *const *ctxs, int n_ctx, int n_pairs)
{
    return ofx_plan_lockstep(ctxs[0]->lockstep, OFX_MAX_GROUP, ofx_plan_even_rounds(n_pairs, n_ctx, OFX_MAX_GROUP));
}

// The batches behind ofx_*_batch_dev (d_flo_init = nullptr) and ofx_*_batch_init_dev: a start per pair where d_flo_init is a table
// (NULL entry: that pair starts from zero).  d_flo_init[g] == d_flo[g] is allowed; a start that is ANOTHER pair's payload of the
// same batch is not (groups run concurrently).  The start's scratch comes from the group's arena and does not enter the group size.
template <class S>
static int sor_pair_batch(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                          const void *const *d_flo_init, void *const *d_flo, int n_pairs, int nx, int ny, const typename S::Params &P,
                          int nscales, double z, double *work_pix_iters)
{
    OFX_TRY(ofx_batch_check_ctxs(ctxs, n_ctx, OFX_SAME_DEVICE | OFX_SAME_FORMAT));
    if (n_pairs < 0 || !dI1 || !dI2 || !d_flo) return OFX_ERR_ARG;
    if (n_pairs == 0) return OFX_OK;
    OFX_TRY(ofx_batch_start_check(ctxs, n_ctx, S::who, n_pairs, d_flo_init, nx, ny, nscales, z));
    const int G = sor_batch_group_size(ctxs, n_ctx, n_pairs);
    return ofx_run_groups(ctxs, n_ctx, n_pairs, G, 1, work_pix_iters, true, [&](ofx_ctx *c, int first, int cnt, ofx_stats *st) {
        return sor_pair_group<S>(c, cnt, dI1 + first, dI2 + first, d_flo_init ? d_flo_init + first : nullptr, d_flo + first, nx, ny, P,
                                 nscales, z, st);
    });
}

extern "C" int ofx_hs_single_scale(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx,
                                   int ny, double alpha, int warps, double TOL, int maxiter, int verbose)
{
    OFX_ENTER(ctx);
    if (!I1 || !I2 || !u || !v) return ofx_fail(ctx, OFX_ERR_ARG, "hs: NULL pointer");
    if (nx < 2 || ny < 2 || warps < 1) return ofx_fail(ctx, OFX_ERR_ARG, "hs: bad size / warps");
    if (maxiter > OFX_HS_MAX_MAXITER) return ofx_fail(ctx, OFX_ERR_ARG, "hs: maxiter > %d", OFX_HS_MAX_MAXITER);
    const double t0 = ofx_now_ms();
    const HsParams P = {alpha, TOL, warps, maxiter, verbose};
    int s = ctx->precision == OFX_F64 ? hs_single_scale_host<double>(ctx, I1, I2, u, v, nx, ny, P)
                                      : hs_single_scale_host<float>(ctx, I1, I2, u, v, nx, ny, P);
    ctx->stats.total_ms = ofx_now_ms() - t0;
    return s;
}

extern "C" int ofx_hs_pyramidal(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx, int ny,
                                double alpha, int nscales, double zfactor, int warps, double TOL, int maxiter,
                                int verbose)
{
    OFX_ENTER(ctx);
    if (!I1 || !I2 || !u || !v) return ofx_fail(ctx, OFX_ERR_ARG, "hs: NULL pointer");
    if (warps < 1) return ofx_fail(ctx, OFX_ERR_ARG, "hs: warps=%d", warps);
    if (maxiter > OFX_HS_MAX_MAXITER) return ofx_fail(ctx, OFX_ERR_ARG, "hs: maxiter > %d", OFX_HS_MAX_MAXITER);
    const double t0 = ofx_now_ms();
    const HsParams P = {alpha, TOL, warps, maxiter, verbose};
    int s = ctx->precision == OFX_F64 ? hs_pyramidal_host<double>(ctx, I1, I2, u, v, nx, ny, P, nscales, zfactor)
                                      : hs_pyramidal_host<float>(ctx, I1, I2, u, v, nx, ny, P, nscales, zfactor);
    ctx->stats.total_ms = ofx_now_ms() - t0;
    return s;
}

extern "C" int ofx_hs_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2,
                                void *const *d_flo, int nx, int ny, double alpha, int nscales, double zfactor, int warps,
                                double TOL, int maxiter, ofx_stats *stats_out)
{
    return sor_pair_group<HsPairs>(ctx, n_pairs, dI1, dI2, nullptr, d_flo, nx, ny, {alpha, TOL, warps, maxiter, 0}, nscales, zfactor,
                                   stats_out);
}

extern "C" int ofx_hs_group_init_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2,
                                     const void *const *d_flo_init, void *const *d_flo, int nx, int ny, double alpha, int nscales,
                                     double zfactor, int warps, double TOL, int maxiter, ofx_stats *stats_out)
{
    return sor_pair_group<HsPairs>(ctx, n_pairs, dI1, dI2, d_flo_init, d_flo, nx, ny, {alpha, TOL, warps, maxiter, 0}, nscales,
                                   zfactor, stats_out);
}

// The video chain (ofx_chain_check, ofx_chain_walk): every step is a group entry with that step's scale and warp counts.
extern "C" int ofx_hs_sequence_group_dev(ofx_ctx *ctx, int n_seq, int n_frames, const void *const *dF, void *const *d_flo, int nx,
                                         int ny, double alpha, int nscales_first, int nscales_next, double zfactor, int warps_first,
                                         int warps_next, double TOL, int maxiter, ofx_stats *stats_out)
{
    OFX_ENTER(ctx);
    if (warps_first < 1 || warps_next < 1) return ofx_fail(ctx, OFX_ERR_ARG, "hs_sequence: warps=%d, %d", warps_first, warps_next);
    if (maxiter > OFX_HS_MAX_MAXITER) return ofx_fail(ctx, OFX_ERR_ARG, "hs_sequence: maxiter > %d", OFX_HS_MAX_MAXITER);
    OFX_TRY(ofx_chain_check(ctx, "hs_sequence", n_seq, n_frames, dF, d_flo, nx, ny, nscales_first, nscales_next, zfactor,
                            HS_PRESMOOTH_SIGMA));
    return ofx_chain_walk(n_seq, n_frames, dF, d_flo, stats_out,
                          [&](int t, const void *const *a, const void *const *b, const void *const *init, void *const *out,
                              ofx_stats *st) {
                              return sor_pair_group<HsPairs>(ctx, n_seq, a, b, init, out, nx, ny,
                                                             {alpha, TOL, t ? warps_next : warps_first, maxiter, 0},
                                                             t ? nscales_next : nscales_first, zfactor, st, true);
                          });
}

extern "C" int ofx_hs_batch_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                                void *const *d_flo, int n_pairs, int nx, int ny, double alpha, int nscales, double zfactor,
                                int warps, double TOL, int maxiter, double *work_pix_iters)
{
    return sor_pair_batch<HsPairs>(ctxs, n_ctx, dI1, dI2, nullptr, d_flo, n_pairs, nx, ny, {alpha, TOL, warps, maxiter, 0}, nscales,
                                   zfactor, work_pix_iters);
}

extern "C" int ofx_hs_batch_init_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                                     const void *const *d_flo_init, void *const *d_flo, int n_pairs, int nx, int ny, double alpha,
                                     int nscales, double zfactor, int warps, double TOL, int maxiter, double *work_pix_iters)
{
    return sor_pair_batch<HsPairs>(ctxs, n_ctx, dI1, dI2, d_flo_init, d_flo, n_pairs, nx, ny, {alpha, TOL, warps, maxiter, 0},
                                   nscales, zfactor, work_pix_iters);
}

// ============================================================================================
// Brox spatial
// ============================================================================================

// clamped centred differences / second derivatives at one pixel (src/operators.cpp:132-406, nz = 1)
template <typename T> OFX_DEV double cdx(const T *f, int i, int j, int nx, int ny)
{
    const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
    return 0.5 * (ldw(f + (size_t) i * nx + jr) - ldw(f + (size_t) i * nx + jl));
}
template <typename T> OFX_DEV double cdy(const T *f, int i, int j, int nx, int ny)
{
    const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
    return 0.5 * (ldw(f + (size_t) id * nx + j) - ldw(f + (size_t) iu * nx + j));
}
template <typename T> OFX_DEV double d2xx(const T *f, int i, int j, int nx, int ny)
{
    const size_t p = (size_t) i * nx + j;
    if (j == 0) return ldw(f + p) * -1.0 + ldw(f + p + 1);
    if (j == nx - 1) return ldw(f + p - 1) + ldw(f + p) * -1.0;
    return ldw(f + p - 1) + ldw(f + p) * -2.0 + ldw(f + p + 1);
}
template <typename T> OFX_DEV double d2yy(const T *f, int i, int j, int nx, int ny)
{
    const size_t p = (size_t) i * nx + j;
    if (i == 0) return ldw(f + p) * -1.0 + ldw(f + p + nx);
    if (i == ny - 1) return ldw(f + p - nx) + ldw(f + p) * -1.0;
    return ldw(f + p - nx) + ldw(f + p) * -2.0 + ldw(f + p + nx);
}
template <typename T> OFX_DEV double d2xy(const T *f, int i, int j, int nx, int ny)
{
    const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
    const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
    return ldw(f + (size_t) iu * nx + jl) * 0.25 + ldw(f + (size_t) iu * nx + jr) * -0.25 +
           ldw(f + (size_t) id * nx + jl) * -0.25 + ldw(f + (size_t) id * nx + jr) * 0.25;
}

// src/brox_optic_flow_spatial.cpp:235-241: gradient of I1; I2 with its first and second derivatives
template <typename T>
OFX_DEV void brox_prepare_px(const T *__restrict__ I1, const T *__restrict__ I2, typename Pix<T>::v2 *__restrict__ G1,
                             typename Pix<T>::v4 *__restrict__ PA, typename Pix<T>::v2 *__restrict__ PB, int i, int j, int nx, int ny)
{
    const size_t p = (size_t) i * nx + j;
    stn2(G1 + p, make_double2(cdx(I1, i, j, nx, ny), cdy(I1, i, j, nx, ny)));
    stn4(PA + p, make_double4(ldw(I2 + p), cdx(I2, i, j, nx, ny), cdy(I2, i, j, nx, ny), d2xx(I2, i, j, nx, ny)));
    stn2(PB + p, make_double2(d2xy(I2, i, j, nx, ny), d2yy(I2, i, j, nx, ny)));
}
template <typename T>
__global__ void k_brox_prepare(const T *__restrict__ I1, const T *__restrict__ I2, typename Pix<T>::v2 *__restrict__ G1,
                               typename Pix<T>::v4 *__restrict__ PA, typename Pix<T>::v2 *__restrict__ PB, int nx, int ny)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t go = (size_t) blockIdx.z * nx * ny;             // pair of a lockstep group
    brox_prepare_px<T>(I1 + go, I2 + go, G1 + go, PA + go, PB + go, i, j, nx, ny);
}
// ... for a lockstep group of temporal Brox: blockIdx.z = flow field of sequences of `fields` fields back to back, whose images
// are sequences of fields + 1 frames back to back -- field z is frame z + z / fields (I1) and the one after it (I2)
template <typename T>
__global__ void k_broxt_prepare_group(const T *__restrict__ I, typename Pix<T>::v2 *__restrict__ G1, typename Pix<T>::v4 *__restrict__ PA,
                                      typename Pix<T>::v2 *__restrict__ PB, int nx, int ny, int fields)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t n = (size_t) nx * ny, go = blockIdx.z * n, gi = (blockIdx.z + blockIdx.z / fields) * n;
    brox_prepare_px<T>(I + gi, I + gi + n, G1 + go, PA + go, PB + go, i, j, nx, ny);
}

// the six fields (I2, I2x, I2y, I2xx | I2xy, I2yy) of one image or channel at a pixel's bicubic taps; 0 when the taps lie outside
template <typename T>
OFX_DEV void bicubic_cell6(const BicubicTaps &t, const typename Pix<T>::v4 *__restrict__ PA,
                           const typename Pix<T>::v2 *__restrict__ PB, int nx, double4 &wa, double2 &wb)
{
    wa = make_double4(0.0, 0.0, 0.0, 0.0);
    wb = make_double2(0.0, 0.0);
    if (t.out) return;
    double c[6][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double4 a[4];
        double2 b[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            a[r] = ldw4(PA + (size_t) t.row[r] * nx + t.col[k]);
            b[r] = ldw2(PB + (size_t) t.row[r] * nx + t.col[k]);
        }
        c[0][k] = cubic_cell(a[0].x, a[1].x, a[2].x, a[3].x, t.fy);
        c[1][k] = cubic_cell(a[0].y, a[1].y, a[2].y, a[3].y, t.fy);
        c[2][k] = cubic_cell(a[0].z, a[1].z, a[2].z, a[3].z, t.fy);
        c[3][k] = cubic_cell(a[0].w, a[1].w, a[2].w, a[3].w, t.fy);
        c[4][k] = cubic_cell(b[0].x, b[1].x, b[2].x, b[3].x, t.fy);
        c[5][k] = cubic_cell(b[0].y, b[1].y, b[2].y, b[3].y, t.fy);
    }
    wa.x = cubic_cell(c[0][0], c[0][1], c[0][2], c[0][3], t.fx);
    wa.y = cubic_cell(c[1][0], c[1][1], c[1][2], c[1][3], t.fx);
    wa.z = cubic_cell(c[2][0], c[2][1], c[2][2], c[2][3], t.fx);
    wa.w = cubic_cell(c[3][0], c[3][1], c[3][2], c[3][3], t.fx);
    wb.x = cubic_cell(c[4][0], c[4][1], c[4][2], c[4][3], t.fx);
    wb.y = cubic_cell(c[5][0], c[5][1], c[5][2], c[5][3], t.fx);
}

// six bicubic warps with one set of taps, :246-251
template <typename T>
__global__ void k_brox_warp(const typename Pix<T>::v4 *__restrict__ PA, const typename Pix<T>::v2 *__restrict__ PB,
                            const typename Pix<T>::v2 *__restrict__ U, typename Pix<T>::v4 *__restrict__ WA,
                            typename Pix<T>::v2 *__restrict__ WB, int nx, int ny)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t go = (size_t) blockIdx.z * nx * ny;             // pair of a lockstep group
    PA += go; PB += go; U += go; WA += go; WB += go;
    const size_t p = (size_t) i * nx + j;
    const double2 u = ldw2(U + p);
    const BicubicTaps t = bicubic_taps(j + u.x, i + u.y, nx, ny);
    double4 wa;
    double2 wb;
    bicubic_cell6<T>(t, PA, PB, nx, wa, wb);
    stn4(WA + p, wa);
    stn2(WB + p, wb);
}

// psi_smooth of the centred flow gradient, :254-258 + :99-122
// Expo != nullptr: robust_expo_psi_smooth (src/robust_expo_smoothness.cpp:26-44), the flow gradient weighed by expo
template <typename T>
__global__ void k_brox_psis(const typename Pix<T>::v2 *__restrict__ U, T *__restrict__ Psis, int nx, int ny,
                            const T *__restrict__ Expo = nullptr)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t go = (size_t) blockIdx.z * nx * ny;             // pair of a lockstep group
    U += go; Psis += go;
    if (Expo) Expo += go;
    const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
    const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
    const double2 r = ldw2(U + (size_t) i * nx + jr), l = ldw2(U + (size_t) i * nx + jl);
    const double2 d = ldw2(U + (size_t) id * nx + j), t = ldw2(U + (size_t) iu * nx + j);
    const double ux = 0.5 * (r.x - l.x), uy = 0.5 * (d.x - t.x);
    const double vx = 0.5 * (r.y - l.y), vy = 0.5 * (d.y - t.y);
    if (Expo) {
        const double e = ldw(Expo + (size_t) i * nx + j);
        const double du = e * ux * ux + e * uy * uy;
        const double dv = e * vx * vx + e * vy * vy;
        const double normFlow = du + dv;
        stn(Psis + (size_t) i * nx + j, e / sqrt(normFlow + BROX_EPSILON * BROX_EPSILON));       // ROBUST_EXPO_EPSILON = 0.001 too
        return;
    }
    const double du = ux * ux + uy * uy;
    const double dv = vx * vx + vy * vy;
    const double d2 = du + dv;
    stn(Psis + (size_t) i * nx + j, 1. / sqrt(d2 + BROX_EPSILON * BROX_EPSILON));
}

// psi1..4 of src/brox_spatial_mask.cpp:16-93 at one pixel (0 across the image border)
struct Psi4 { double p1, p2, p3, p4; };
template <typename T, class Lay> OFX_DEV Psi4 brox_psi4_lay(const T *Psis, const Lay &lay, int i, int j, int nx, int ny)
{
    const double c = ldw(Psis + lay.idx(i, j));
    Psi4 r;
    r.p1 = (i < ny - 1) ? 0.5 * (ldw(Psis + lay.idx(i + 1, j)) + c) : 0.0;
    r.p2 = (i > 0) ? 0.5 * (ldw(Psis + lay.idx(i - 1, j)) + c) : 0.0;
    r.p3 = (j < nx - 1) ? 0.5 * (ldw(Psis + lay.idx(i, j + 1)) + c) : 0.0;
    r.p4 = (j > 0) ? 0.5 * (ldw(Psis + lay.idx(i, j - 1)) + c) : 0.0;
    return r;
}
template <typename T> OFX_DEV Psi4 brox_psi4(const T *Psis, int i, int j, int nx, int ny)
{
    return brox_psi4_lay(Psis, LayRow{nx}, i, j, nx, ny);
}

// div_u, div_v (src/brox_spatial_mask.cpp:100-171), div_d and du = dv = 0 (:261-274)
template <typename T>
__global__ void k_brox_div(const typename Pix<T>::v2 *__restrict__ U, const T *__restrict__ Psis,
                           typename Pix<T>::v2 *__restrict__ DV, T *__restrict__ Dd, typename Pix<T>::v2 *__restrict__ DU,
                           int nx, int ny, double alpha, int rx = 0)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t go = (size_t) blockIdx.z * nx * ny;             // pair of a lockstep group
    U += go; Psis += go; DV += go; Dd += go; DU += go;
    const size_t k = (size_t) i * nx + j;
    const Psi4 s = brox_psi4(Psis, i, j, nx, ny);
    const double2 c = ldw2(U + k);
    if (rx) {
        // robust_expo_divergence / div_d (src/robust_expo_generic_tensor.cpp:97-168, robust_expo_methods.cpp:266): the same
        // terms in the order right, left, down, up
        double du = 0.0, dv = 0.0;
        bool have = false;
        if (j < nx - 1) { const double2 q = ldw2(U + k + 1); du = s.p3 * (q.x - c.x); dv = s.p3 * (q.y - c.y); have = true; }
        if (j > 0) {
            const double2 q = ldw2(U + k - 1);
            const double a = s.p4 * (q.x - c.x), b = s.p4 * (q.y - c.y);
            du = have ? du + a : a; dv = have ? dv + b : b; have = true;
        }
        if (i < ny - 1) {
            const double2 q = ldw2(U + k + nx);
            const double a = s.p1 * (q.x - c.x), b = s.p1 * (q.y - c.y);
            du = have ? du + a : a; dv = have ? dv + b : b; have = true;
        }
        if (i > 0) {
            const double2 q = ldw2(U + k - nx);
            const double a = s.p2 * (q.x - c.x), b = s.p2 * (q.y - c.y);
            du = have ? du + a : a; dv = have ? dv + b : b; have = true;
        }
        stn2(DV + k, make_double2(du, dv));
        stn(Dd + k, alpha * (s.p3 + s.p4 + s.p1 + s.p2));
        stn2(DU + k, make_double2(0.0, 0.0));
        return;
    }
    // terms that exist, accumulated in the order down, up, right, left; missing terms are left out
    double du = 0.0, dv = 0.0;
    bool have = false;
    if (i < ny - 1) { const double2 q = ldw2(U + k + nx); du = s.p1 * (q.x - c.x); dv = s.p1 * (q.y - c.y); have = true; }
    if (i > 0) {
        const double2 q = ldw2(U + k - nx);
        const double a = s.p2 * (q.x - c.x), b = s.p2 * (q.y - c.y);
        du = have ? du + a : a; dv = have ? dv + b : b; have = true;
    }
    if (j < nx - 1) {
        const double2 q = ldw2(U + k + 1);
        const double a = s.p3 * (q.x - c.x), b = s.p3 * (q.y - c.y);
        du = have ? du + a : a; dv = have ? dv + b : b; have = true;
    }
    if (j > 0) {
        const double2 q = ldw2(U + k - 1);
        const double a = s.p4 * (q.x - c.x), b = s.p4 * (q.y - c.y);
        du = have ? du + a : a; dv = have ? dv + b : b; have = true;
    }
    stn2(DV + k, make_double2(du, dv));
    stn(Dd + k, alpha * (s.p1 + s.p2 + s.p3 + s.p4));                  // :270
    stn2(DU + k, make_double2(0.0, 0.0));                               // :273
}

// psi_data, psi_gradient and the constant parts of the scheme, :279-309 (+ :33-92)
// element i of the level's arrays; i1 = its value of the first image
template <typename T>
OFX_DEV void brox_coeff_px(double i1, const typename Pix<T>::v2 *__restrict__ G1, const typename Pix<T>::v4 *__restrict__ WA,
                           const typename Pix<T>::v2 *__restrict__ WB, const typename Pix<T>::v2 *__restrict__ DU,
                           const typename Pix<T>::v2 *__restrict__ DV, const T *__restrict__ Dd, typename Pix<T>::v4 *__restrict__ CO,
                           T *__restrict__ Dm, size_t i, double alpha, double gamma)
{
    const double2 g1 = ldw2(G1 + i);
    const double4 wa = ldw4(WA + i);
    const double2 wb = ldw2(WB + i);
    const double2 d = ldw2(DU + i);
    const double I2w = wa.x, I2wx = wa.y, I2wy = wa.z, I2wxx = wa.w, I2wxy = wb.x, I2wyy = wb.y;
    const double eps2 = BROX_EPSILON * BROX_EPSILON;
    const double dI = I2w - i1 + I2wx * d.x + I2wy * d.y;                              // psi_data :51
    const double psid = rnd_to<T>(1. / sqrt(dI * dI + eps2));
    const double dIx = I2wx - g1.x + I2wxx * d.x + I2wxy * d.y;                        // psi_gradient :86-87
    const double dIy = I2wy - g1.y + I2wxy * d.x + I2wyy * d.y;
    const double dI2 = dIx * dIx + dIy * dIy;
    const double psig = rnd_to<T>(1. / sqrt(dI2 + eps2));
    const double p = psid;
    const double g = gamma * psig;
    const double dif = I2w - i1;
    const double BNu = -p * dif * I2wx;
    const double BNv = -p * dif * I2wy;
    const double BDu = p * I2wx * I2wx;
    const double BDv = p * I2wy * I2wy;
    const double dx = (I2wx - g1.x);
    const double dy = (I2wy - g1.y);
    const double GNu = -g * (dx * I2wxx + dy * I2wxy);
    const double GNv = -g * (dx * I2wxy + dy * I2wyy);
    const double GDu = g * (I2wxx * I2wxx + I2wxy * I2wxy);
    const double GDv = g * (I2wyy * I2wyy + I2wxy * I2wxy);
    const double DI = (I2wxx + I2wyy) * I2wxy;
    const double Duv = p * I2wy * I2wx + g * DI;
    const double2 dv = ldw2(DV + i);
    const double dd = ldw(Dd + i);
    stn4(CO + i, make_double4(BNu + GNu + alpha * dv.x, BNv + GNv + alpha * dv.y, BDu + GDu + dd, BDv + GDv + dd));
    stn(Dm + i, Duv);
}
template <typename T>
__global__ void k_brox_coeff(const T *__restrict__ I1, const typename Pix<T>::v2 *__restrict__ G1,
                             const typename Pix<T>::v4 *__restrict__ WA, const typename Pix<T>::v2 *__restrict__ WB,
                             const typename Pix<T>::v2 *__restrict__ DU, const typename Pix<T>::v2 *__restrict__ DV,
                             const T *__restrict__ Dd, typename Pix<T>::v4 *__restrict__ CO, T *__restrict__ Dm, int n,
                             double alpha, double gamma)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t) n) return;
    brox_coeff_px<T>(ldw(I1 + i), G1, WA, WB, DU, DV, Dd, CO, Dm, i, alpha, gamma);
}
// ... for a lockstep group of temporal Brox: sequences of seq_elems field elements back to back; the images of each hold one frame
// of `plane` elements more, so sequence q's frames start q planes further on (n < 2^31)
template <typename T>
__global__ void k_broxt_coeff_group(const T *__restrict__ I, const typename Pix<T>::v2 *__restrict__ G1,
                                    const typename Pix<T>::v4 *__restrict__ WA, const typename Pix<T>::v2 *__restrict__ WB,
                                    const typename Pix<T>::v2 *__restrict__ DU, const typename Pix<T>::v2 *__restrict__ DV,
                                    const T *__restrict__ Dd, typename Pix<T>::v4 *__restrict__ CO, T *__restrict__ Dm, int n,
                                    double alpha, double gamma, int seq_elems, int plane)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t) n) return;
    const double i1 = ldw(I + i + (size_t) ((unsigned) i / (unsigned) seq_elems) * (size_t) plane);
    brox_coeff_px<T>(i1, G1, WA, WB, DU, DV, Dd, CO, Dm, i, alpha, gamma);
}

// SOR update of one pixel, src/brox_optic_flow_spatial.cpp:129-172, in two halves (operands first, see HsOps);
// returns the squared update (:166)
struct BroxOps {
    Psi4    s;
    double2 c, dn, up, rt, lf;
    double4 co;
    double  D;
};
// psi1..4 through a sweep accessor (UGlobal: the arrays; BLds: the launch window in LDS); brox_psi4_lay's arithmetic
template <typename T, class Acc> OFX_DEV Psi4 brox_psi4_acc(const Acc &acc, const T *Psis, int i, int j, int nx, int ny)
{
    const double c = acc.psi(Psis, i, j);
    Psi4 r;
    r.p1 = (i < ny - 1) ? 0.5 * (acc.psi(Psis, i + 1, j) + c) : 0.0;
    r.p2 = (i > 0) ? 0.5 * (acc.psi(Psis, i - 1, j) + c) : 0.0;
    r.p3 = (j < nx - 1) ? 0.5 * (acc.psi(Psis, i, j + 1) + c) : 0.0;
    r.p4 = (j > 0) ? 0.5 * (acc.psi(Psis, i, j - 1) + c) : 0.0;
    return r;
}
template <typename T, class Acc>
OFX_DEV BroxOps brox_point_load(const Acc &acc, const typename Pix<T>::v4 *__restrict__ CO, const T *__restrict__ Dm,
                                const T *__restrict__ Psis, int i, int j, int nx, int ny)
{
    BroxOps o;
    o.s = brox_psi4_acc<T>(acc, Psis, i, j, nx, ny);
    // a missing neighbour is addressed as the pixel itself (offset 0) with psi = 0, :332-388
    o.c = acc.get(i, j);
    o.dn = (i < ny - 1) ? acc.get(i + 1, j) : o.c;
    o.up = (i > 0) ? acc.get(i - 1, j) : o.c;
    o.rt = (j < nx - 1) ? acc.get(i, j + 1) : o.c;
    o.lf = (j > 0) ? acc.get(i, j - 1) : o.c;
    acc.coef4(CO, Dm, i, j, o.co, o.D);
    return o;
}
// RX: robust_expo_methods.cpp:138-148 -- the same taps summed right, left, down, up
template <typename T, class Acc, bool RX = false>
OFX_DEV double brox_point_finish(const Acc &acc, const BroxOps &o, int i, int j, double alpha)
{
    const Psi4 s = o.s;
    const double4 co = o.co;
    const double D = o.D;
    const double w = BROX_SOR_W;
    const double div_du = RX ? s.p3 * o.rt.x + s.p4 * o.lf.x + s.p1 * o.dn.x + s.p2 * o.up.x
                             : s.p1 * o.dn.x + s.p2 * o.up.x + s.p3 * o.rt.x + s.p4 * o.lf.x;      // :153-154
    const double div_dv = RX ? s.p3 * o.rt.y + s.p4 * o.lf.y + s.p1 * o.dn.y + s.p2 * o.up.y
                             : s.p1 * o.dn.y + s.p2 * o.up.y + s.p3 * o.rt.y + s.p4 * o.lf.y;      // :155-156
    const double duk = o.c.x, dvk = o.c.y;
    const double dun = rnd_to<T>((1. - w) * duk + w * (co.x - D * dvk + alpha * div_du) / co.z);   // :162
    const double dvn = rnd_to<T>((1. - w) * dvk + w * (co.y - D * dun + alpha * div_dv) / co.w);   // :163
    acc.put(i, j, make_double2(dun, dvn));
    return (dun - duk) * (dun - duk) + (dvn - dvk) * (dvn - dvk);                     // :166
}
template <typename T, class Acc, bool RX = false>
OFX_DEV double brox_point_acc(const Acc &acc, const typename Pix<T>::v4 *__restrict__ CO, const T *__restrict__ Dm,
                              const T *__restrict__ Psis, int i, int j, int nx, int ny, double alpha)
{
    const BroxOps o = brox_point_load<T>(acc, CO, Dm, Psis, i, j, nx, ny);
    return brox_point_finish<T, Acc, RX>(acc, o, i, j, alpha);
}

template <typename T, bool COH = false, bool SNAP = false>
OFX_DEV double brox_point(typename Pix<T>::v2 *DU, const typename Pix<T>::v4 *__restrict__ CO,
                          const T *__restrict__ Dm, const T *__restrict__ Psis, int i, int j, int nx, int ny, double alpha,
                          typename Pix<T>::v2 *snap = nullptr)
{
    const UGlobal<T, COH, SNAP, LayRow> acc = {DU, snap, LayRow{nx}};
    return brox_point_acc<T>(acc, CO, Dm, Psis, i, j, nx, ny, alpha);
}
// the same on hyperplane-major arrays (windowed sweeps)
template <typename T, bool COH, bool SNAP>
OFX_DEV double brox_point_skew(typename Pix<T>::v2 *DU, const typename Pix<T>::v4 *__restrict__ CO, const T *__restrict__ Dm,
                               const T *__restrict__ Psis, int i, int j, int nx, int ny, double alpha,
                               typename Pix<T>::v2 *snap)
{
    const UGlobal<T, COH, SNAP, LaySkew> acc = {DU, snap, LaySkew{ny, BROX_PLANE_C_SKEW}};
    return brox_point_acc<T>(acc, CO, Dm, Psis, i, j, nx, ny, alpha);
}

// one colour of one SOR sweep (fast, order-changing mode): every pixel with (i + j) % 2 == colour
// (blockIdx.z = pair of a lockstep group: its own error slots, err_stride doubles apart)
template <typename T>
__global__ __launch_bounds__(256) void k_brox_sor(typename Pix<T>::v2 *__restrict__ DU,
                                                  const typename Pix<T>::v4 *__restrict__ CO, const T *__restrict__ Dm,
                                                  const T *__restrict__ Psis, double *__restrict__ err, int k, int nx,
                                                  int ny, int colour, double alpha, double tol, int err_stride)
{
    const size_t go = (size_t) blockIdx.z * nx * ny;
    DU += go; CO += go; Dm += go; Psis += go;
    err += (size_t) blockIdx.z * err_stride;
    const double prev = loop_fetch_prev(err, k);
    const int i = blockIdx.y * 4 + threadIdx.y;
    const int j = 2 * (blockIdx.x * 64 + threadIdx.x) + ((i + colour) & 1);
    const bool in = (j < nx) && (i < ny);
    const int gw = (blockIdx.y * gridDim.x + blockIdx.x) * 4 + threadIdx.y;
    if (!loop_continues(prev, k, nx * ny, tol, OFX_CRIT_SQRT_MEAN)) return;
    double e = 0.0;
    if (in) e = brox_point<T>(DU, CO, Dm, Psis, i, j, nx, ny, alpha);
    loop_accumulate(err, k, e, gw);
}

// exact mode (see k_hs_plane): 5-point stencil -> pos = i + j in the interior, C = 2
// (visiting order brox_optic_flow_spatial.cpp:320-387)
#define BROX_PLANE_C 2
OFX_DEV bool brox_plane_item(int r, int q, int nx, int ny, int corner, int &i, int &j)
{
    if (r >= 1 && r <= ny - 2) { i = r; j = q - r; return j >= 1 && j <= nx - 2; }
    if (r == 0) { i = 0; j = q - 2; return j >= 1 && j <= nx - 2; }
    if (r == ny - 1) { i = ny - 1; j = q - (ny - 1); return j >= 1 && j <= nx - 2; }
    if (r == ny) { i = q - 2; j = 0; return i >= 1 && i <= ny - 2; }
    if (r == ny + 1) { i = q - (nx - 1); j = nx - 1; return i >= 1 && i <= ny - 2; }
    if (r == ny + 2) {
        if (corner == 0) { i = 0; j = 0; return q == 4; }
        if (corner == 1) { i = 0; j = nx - 1; return q == nx + 1; }
        if (corner == 2) { i = ny - 1; j = 0; return q == ny + 1; }
        i = ny - 1; j = nx - 1; return q == ny + nx - 2;
    }
    return false;
}

template <typename T>
__global__ __launch_bounds__(64) void k_brox_plane(typename Pix<T>::v2 *__restrict__ DU,
                                                   const typename Pix<T>::v4 *__restrict__ CO, const T *__restrict__ Dm,
                                                   const T *__restrict__ Psis, double *__restrict__ err, int t, int s_lo,
                                                   int nx, int ny, double alpha)
{
    const int s = s_lo + blockIdx.y;
    const int q = t - BROX_PLANE_C * s;
    const int r = blockIdx.x * 64 + threadIdx.x;
    double e = 0.0;
    int i, j;
    if (r == ny + 2) {
        for (int corner = 0; corner < 4; corner++)
            if (brox_plane_item(r, q, nx, ny, corner, i, j)) e += brox_point<T>(DU, CO, Dm, Psis, i, j, nx, ny, alpha);
    } else if (brox_plane_item(r, q, nx, ny, 0, i, j)) {
        e = brox_point<T>(DU, CO, Dm, Psis, i, j, nx, ny, alpha);
    }
    loop_accumulate(err, s, e, blockIdx.x);
}

// windowed exact mode (see k_hs_window): K steps per launch, one workgroup per (SPW sweeps, row block)
template <typename T, int SPW, int MAXT, bool RX = false>
__global__ __launch_bounds__(MAXT) void k_brox_window(typename Pix<T>::v2 *DUg, typename Pix<T>::v2 *snap,
                                                      const typename Pix<T>::v4 *__restrict__ COg, const T *__restrict__ Dmg,
                                                      const T *__restrict__ Psisg, double *__restrict__ errg, SorWin w,
                                                      SorGrp grp, int s_cnt, int nx, int ny, double alpha)
{
    const int b = blockIdx.x, s0 = w.s_first + blockIdx.y * SPW, g = blockIdx.z;
    if (!((grp.runmask >> g) & 1u)) return;
    const int qmax = ny + nx - 2;
    int q_first[SPW];
    bool live[SPW], any = false;
#pragma unroll
    for (int u = 0; u < SPW; u++) {
        q_first[u] = w.tau0 - w.lag_s * (s0 + u) - w.lag_b * b;
        live[u] = (s0 + u < w.s_first + s_cnt) && !sor_unit_idle(w, b, q_first[u], w.K, 1, nx, ny);
        any = any || live[u];
    }
    if (!any) return;
    typename Pix<T>::v2 *DU = DUg + g * grp.npix;
    const typename Pix<T>::v4 *__restrict__ CO = COg + g * grp.npix;
    const T *__restrict__ Dm = Dmg + g * grp.npix;
    const T *__restrict__ Psis = Psisg + g * grp.npix;
    double *__restrict__ err = errg + (size_t) g * grp.err_stride;
    const int r = sor_window_item(w, b, threadIdx.x, ny);
    double e[SPW];
#pragma unroll
    for (int u = 0; u < SPW; u++) e[u] = 0.0;
    for (int k = 0; k < w.K; k++) {
        bool have[SPW];
        int pi[SPW], pj[SPW];
        BroxOps ops[SPW];
#pragma unroll
        for (int u = 0; u < SPW; u++) {
            const int q = q_first[u] + k;
            have[u] = live[u] && q >= 0 && q <= qmax && r >= 0 && r != ny + 2 && brox_plane_item(r, q, nx, ny, 0, pi[u], pj[u]) &&
                      (r < ny || sor_border_block(pi[u], ny, w.R) == b);
            if (SPW > 1 && have[u]) {
                const UGlobal<T, OFX_SOR_COH != 0, true, LaySkew> acc = {DU, snap + g * grp.snap_stride + (size_t) (s0 + u) * grp.npix,
                                                                         LaySkew{ny, BROX_PLANE_C_SKEW}};
                ops[u] = brox_point_load<T>(acc, CO, Dm, Psis, pi[u], pj[u], nx, ny);
            }
        }
#pragma unroll
        for (int u = 0; u < SPW; u++) {
            typename Pix<T>::v2 *mysnap = snap + g * grp.snap_stride + (size_t) (s0 + u) * grp.npix;
            if (have[u]) {
                const UGlobal<T, OFX_SOR_COH != 0, true, LaySkew> acc = {DU, mysnap, LaySkew{ny, BROX_PLANE_C_SKEW}};
                using AccT = UGlobal<T, OFX_SOR_COH != 0, true, LaySkew>;
                if (SPW > 1) e[u] += brox_point_finish<T, AccT, RX>(acc, ops[u], pi[u], pj[u], alpha);
                else e[u] += brox_point_acc<T, AccT, RX>(acc, CO, Dm, Psis, pi[u], pj[u], nx, ny, alpha);
            }
            const int q = q_first[u] + k;
            if (live[u] && r == ny + 2 && q >= 0 && q <= qmax) {
                int i, j;
                for (int corner = 0; corner < 4; corner++)
                    if (brox_plane_item(r, q, nx, ny, corner, i, j) && sor_border_block(i, ny, w.R) == b) {
                        using AccT = UGlobal<T, OFX_SOR_COH != 0, true, LaySkew>;
                        const AccT cacc = {DU, mysnap, LaySkew{ny, BROX_PLANE_C_SKEW}};
                        e[u] += brox_point_acc<T, AccT, RX>(cacc, CO, Dm, Psis, i, j, nx, ny, alpha);
                    }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < SPW; u++)
        if (live[u]) loop_accumulate(err, s0 + u, e[u], b * 4 + (threadIdx.x >> 6));
}

// The Brox sweep with its launch window in LDS (see k_hs_window_lds).  What the KW steps of (sweep, row block b) touch
// (tools/check_sor_schedule.py --cover): unknowns and psi_s on hyperplanes q0 - 4 .. q0 + KW of the skewed coordinate i + j,
// rows b R - 2 .. b R + R -- an LDS window each; (CO, Dm) of the KW pixels a thread updates -- LDS slots of its own.
template <typename T, int KW> struct BroxWinLds {
    static constexpr int NH = KW + 5;
    static constexpr int BACK = 4;
    static size_t bytes(int nr, int nt)
    {
        return (size_t) nt * KW * (sizeof(double4) + sizeof(double)) + (size_t) nr * NH * (sizeof(double2) + sizeof(double));
    }
};
template <typename T, bool SNAP> struct BLds {
    typename Pix<T>::v2 *U, *snap;
    double2 *win;                                // [NH][nr] (du, dv)
    const double *ps;                            // [NH][nr] psi_s
    int nr, row0, h0;
    LaySkew lay;
    double4 co;                                  // constant operands of the pixel being updated (set per step)
    double  D;
    OFX_DEV double2 get(int ii, int jj) const { return win[(ii + jj - h0) * nr + (ii - row0)]; }
    OFX_DEV double psi(const T *, int ii, int jj) const { return ps[(ii + jj - h0) * nr + (ii - row0)]; }
    OFX_DEV void coef4(const typename Pix<T>::v4 *, const T *, int, int, double4 &c, double &D_) const { c = co; D_ = D; }
    OFX_DEV void put(int i, int j, double2 v) const
    {
        win[(i + j - h0) * nr + (i - row0)] = v;
        const size_t p = lay.idx(i, j);
        stn2(U + p, v);
        if (SNAP) stn2(snap + p, v);
    }
};
OFX_DEV bool brox_window_pixel(const SorWin &w, int b, int r, int q, int qmax, int nx, int ny, int &pi, int &pj)
{
    return q >= 0 && q <= qmax && r >= 0 && r != ny + 2 && brox_plane_item(r, q, nx, ny, 0, pi, pj) &&
           (r < ny || sor_border_block(pi, ny, w.R) == b);
}
template <typename T, int KW, int MAXT>
__global__ __launch_bounds__(MAXT) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_brox_window_lds(
    typename Pix<T>::v2 *DUg, typename Pix<T>::v2 *snap, const typename Pix<T>::v4 *__restrict__ COg, const T *__restrict__ Dmg,
    const T *__restrict__ Psisg, double *__restrict__ errg, SorWin w, SorGrp grp, int s_cnt, int nx, int ny, double alpha)
{
    using W = BroxWinLds<T, KW>;
    extern __shared__ double4 brox_lds[];
    const int b = blockIdx.x, s = w.s_first + blockIdx.y, g = blockIdx.z;
    if (!((grp.runmask >> g) & 1u)) return;
    const int qmax = ny + nx - 2;
    const int q0 = w.tau0 - w.lag_s * s - w.lag_b * b;
    if (sor_unit_idle(w, b, q0, KW, 1, nx, ny)) return;
    typename Pix<T>::v2 *DU = DUg + g * grp.npix;
    const typename Pix<T>::v4 *__restrict__ CO = COg + g * grp.npix;
    const T *__restrict__ Dm = Dmg + g * grp.npix;
    const T *__restrict__ Psis = Psisg + g * grp.npix;
    typename Pix<T>::v2 *mysnap = snap + g * grp.snap_stride + (size_t) s * grp.npix;
    double *__restrict__ err = errg + (size_t) g * grp.err_stride;
    const int nr = w.R + 3, row0 = b * w.R - 2, h0 = q0 - W::BACK, t = threadIdx.x, nt = blockDim.x;
    double4 *cco = brox_lds;                                     // [KW][nt]: 32-byte entries first (alignment)
    double2 *win = reinterpret_cast<double2 *>(cco + KW * nt);   // [NH][nr]
    double *ps = reinterpret_cast<double *>(win + W::NH * nr);   // [NH][nr]
    double *cdm = ps + W::NH * nr;                               // [KW][nt]
    const LaySkew lay = {ny, BROX_PLANE_C_SKEW};
    const int r = sor_window_item(w, b, t, ny);
    {
        const int i = row0 + t, ic = i < 0 ? 0 : (i > ny - 1 ? ny - 1 : i);
        const int hmax = (ny - 1) + nx - 1;
        double2 u_in[W::NH];
        double p_in[W::NH], d_in[KW];
        double4 c_in[KW];
#pragma unroll
        for (int k = 0; k < W::NH; k++) {
            const int h = h0 + k, hc = h < 0 ? 0 : (h > hmax ? hmax : h);
            u_in[k] = ldw2(DU + (size_t) hc * ny + ic);
            p_in[k] = ldw(Psis + (size_t) hc * ny + ic);
        }
#pragma unroll
        for (int k = 0; k < KW; k++) {
            int pi, pj;
            const bool have = brox_window_pixel(w, b, r, q0 + k, qmax, nx, ny, pi, pj);
            const size_t p = have ? lay.idx(pi, pj) : 0;
            c_in[k] = ldw4(CO + p);
            d_in[k] = ldw(Dm + p);
        }
        if (t < nr) {
#pragma unroll
            for (int k = 0; k < W::NH; k++) { win[k * nr + t] = u_in[k]; ps[k * nr + t] = p_in[k]; }
        }
#pragma unroll
        for (int k = 0; k < KW; k++) { cco[k * nt + t] = c_in[k]; cdm[k * nt + t] = d_in[k]; }
    }
    __syncthreads();
    BLds<T, true> acc = {DU, mysnap, win, ps, nr, row0, h0, lay, make_double4(0.0, 0.0, 0.0, 0.0), 0.0};
    double e = 0.0;
#pragma unroll 1
    for (int k = 0; k < KW; k++) {
        const int q = q0 + k;
        int pi, pj;
        if (brox_window_pixel(w, b, r, q, qmax, nx, ny, pi, pj)) {
            acc.co = cco[k * nt + t];
            acc.D = cdm[k * nt + t];
            e += brox_point_acc<T>(acc, CO, Dm, Psis, pi, pj, nx, ny, alpha);
        }
        if (q >= 0 && q <= qmax && r == ny + 2) {
            for (int corner = 0; corner < 4; corner++)
                if (brox_plane_item(r, q, nx, ny, corner, pi, pj) && sor_border_block(pi, ny, w.R) == b) {
                    const size_t p = lay.idx(pi, pj);
                    acc.co = ldw4(CO + p);
                    acc.D = ldw(Dm + p);
                    e += brox_point_acc<T>(acc, CO, Dm, Psis, pi, pj, nx, ny, alpha);
                }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    loop_accumulate(err, s, e, b * 4 + (t >> 6));
}

// u += du, v += dv, :398-401
template <typename T>
__global__ void k_brox_add(typename Pix<T>::v2 *__restrict__ U, const typename Pix<T>::v2 *__restrict__ DU, int n)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t) n) return;
    const double2 u = ldw2(U + i), d = ldw2(DU + i);
    stn2(U + i, make_double2(u.x + d.x, u.y + d.y));
}

// ============================================================================================
// robust_expo_methods on nz interleaved channels (src/robust_expo_methods.cpp:162-455)
// ============================================================================================
// Device layout: channel-planar packs, pair-major in a lockstep group.  Channel c of pair g of I1, (I1x, I1y),
// (I2, I2x, I2y, I2xx), (I2xy, I2yy) and of their warps lies at element (g * nz + c) * nx * ny of the level's I1, G1, PA, PB,
// WA, WB; the one-plane arrays (U, DU, DV, Dd, CO, Dm, Psis, Expo, Mg) keep pair g at g * nx * ny, and the interleaved images
// a level starts from lie back to back, pair g at g * nx * ny * nz.  The C ABI keeps the reference's interleaved order.

// The five derivatives the reference leaves at FLAT element k = (i * nx + j) * nz + c of its derivative arrays
// (centered_gradient, Dxx, Dyy, Dxy with nz channels, src/operators.cpp:132-406).  Below the first row they are the clamped
// one-channel stencils applied to channel c, with one exception: in the last row the right-hand tap of the mask is read at
// k + 1 instead of k + nz (:189).  In the FIRST row the source's loops address their output by the column alone
// (dx[j], output[j], :176, :363-364), so for nz > 1 flat elements 1 .. nx - 2 receive the stencil of "column k" of the last
// channel -- its second-row taps read at nx * nz + k (:172-174) --, the corner elements that are written afterwards keep
// their own values, and every other element of the row is never written.  The compiled reference allocates zeroed arrays, so
// those read 0; that is what is reproduced.  For nz = 1 all of this is cdx, cdy, d2xx, d2yy, d2xy of the Brox section.
struct RexpoDerivs { double x, y, xx, xy, yy; };
template <typename T>
OFX_DEV RexpoDerivs rexpo_derivs_proper(const T *__restrict__ in, int i, int j, int c, int nx, int ny, int nz)
{
    const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
    const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
#define RX_P(ii, jj) ldw(in + ((size_t) (ii) * nx + (jj)) * nz + c)
    // the mask's right-hand tap of the last row, :189
    const bool odd = i == ny - 1 && j > 0 && j < nx - 1;
    const double rgt = odd ? ldw(in + ((size_t) i * nx + j) * nz + c + 1) : RX_P(i, jr);
    RexpoDerivs d;
    d.x = 0.5 * (RX_P(i, jr) - RX_P(i, jl));
    d.y = 0.5 * (RX_P(id, j) - RX_P(iu, j));
    if (j == 0) d.xx = RX_P(i, j) * -1.0 + RX_P(i, j + 1);
    else if (j == nx - 1) d.xx = RX_P(i, j - 1) + RX_P(i, j) * -1.0;
    else d.xx = RX_P(i, j - 1) + RX_P(i, j) * -2.0 + rgt;
    if (i == 0) d.yy = RX_P(i, j) * -1.0 + RX_P(i + 1, j);
    else if (i == ny - 1) d.yy = RX_P(i - 1, j) + RX_P(i, j) * -1.0;
    else d.yy = RX_P(i - 1, j) + RX_P(i, j) * -2.0 + RX_P(i + 1, j);
    d.xy = RX_P(iu, jl) * 0.25 + RX_P(iu, jr) * -0.25 + RX_P(id, jl) * -0.25 + (odd ? rgt : RX_P(id, jr)) * 0.25;
#undef RX_P
    return d;
}
template <typename T>
OFX_DEV RexpoDerivs rexpo_derivs(const T *__restrict__ in, int i, int j, int c, int nx, int ny, int nz)
{
    if (i > 0) return rexpo_derivs_proper(in, i, j, c, nx, ny, nz);
    const int f = j * nz + c;                                    // flat element of the first row
    const bool row_loop = f >= 1 && f <= nx - 2;                 // written as dx[f] / output[f] by every channel's pass
    if (f < nz && !(row_loop && f < nz - 1)) return rexpo_derivs_proper(in, 0, 0, f, nx, ny, nz);     // corner (0, 0) of channel f
    if (row_loop) {                                              // the last channel's pass wins
        const size_t idx = (size_t) f * nz + (nz - 1), row1 = (size_t) nx * nz + f;
        RexpoDerivs d;
        d.x = 0.5 * (ldw(in + idx + nz) - ldw(in + idx - nz));
        d.y = 0.5 * (ldw(in + idx + (size_t) nx * nz) - ldw(in + idx));
        d.xx = ldw(in + idx - nz) + ldw(in + idx) * -2.0 + ldw(in + idx + nz);
        d.yy = ldw(in + idx) * -1.0 + ldw(in + row1);
        d.xy = ldw(in + idx - nz) * 0.25 + ldw(in + idx + nz) * -0.25 + ldw(in + row1 - nz) * -0.25 + ldw(in + row1 + nz) * 0.25;
        return d;
    }
    if (f >= (nx - 1) * nz) return rexpo_derivs_proper(in, 0, nx - 1, f - (nx - 1) * nz, nx, ny, nz);   // corner (0, nx - 1)
    return RexpoDerivs{0.0, 0.0, 0.0, 0.0, 0.0};                 // never written by the source
}

// :221-227: gradient of I1; I2 with its first and second derivatives; interleaved in, channel-planar packs out
// (blockIdx.z = pair * nz + channel).  Needs nx, ny >= 3.
template <typename T>
__global__ void k_rexpo_prepare_c(const T *__restrict__ I1i, const T *__restrict__ I2i, T *__restrict__ I1,
                                  typename Pix<T>::v2 *__restrict__ G1, typename Pix<T>::v4 *__restrict__ PA,
                                  typename Pix<T>::v2 *__restrict__ PB, int nx, int ny, int nz)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    const int pair = blockIdx.z / nz, c = blockIdx.z - pair * nz;
    if (j >= nx || i >= ny) return;
    const size_t p = (size_t) i * nx + j, q = (size_t) blockIdx.z * nx * ny + p;
    I1i += (size_t) pair * nx * ny * nz;
    I2i += (size_t) pair * nx * ny * nz;
    const RexpoDerivs a = rexpo_derivs(I1i, i, j, c, nx, ny, nz), b = rexpo_derivs(I2i, i, j, c, nx, ny, nz);
    stn(I1 + q, ldw(I1i + p * nz + c));
    stn2(G1 + q, make_double2(a.x, a.y));
    stn4(PA + q, make_double4(ldw(I2i + p * nz + c), b.x, b.y, b.xx));
    stn2(PB + q, make_double2(b.xy, b.yy));
}

// max_gradients (src/robust_expo_smoothness.cpp:51-73): the largest gradient magnitude of a pixel's channels
// (blockIdx.y = pair)
template <typename T>
__global__ void k_rexpo_maxgrad(const typename Pix<T>::v2 *__restrict__ G1, double *__restrict__ Mg, int n, int nz)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t) n) return;
    G1 += (size_t) blockIdx.y * nz * n;
    Mg += (size_t) blockIdx.y * n;
    double2 g = ldw2(G1 + i);
    double m = sqrt(g.x * g.x + g.y * g.y);
    for (int c = 1; c < nz; c++) {
        g = ldw2(G1 + (size_t) c * n + i);
        const double gc = sqrt(g.x * g.x + g.y * g.y);
        if (m < gc) m = gc;
    }
    Mg[i] = m;
}

// :236-241: the six warps of every channel with the pixel's one set of bicubic taps (blockIdx.z = pair)
template <typename T>
__global__ void k_rexpo_warp_c(const typename Pix<T>::v4 *__restrict__ PA, const typename Pix<T>::v2 *__restrict__ PB,
                               const typename Pix<T>::v2 *__restrict__ U, typename Pix<T>::v4 *__restrict__ WA,
                               typename Pix<T>::v2 *__restrict__ WB, int nx, int ny, int nz)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= nx || i >= ny) return;
    const size_t n = (size_t) nx * ny, p = (size_t) i * nx + j;
    const size_t go = (size_t) blockIdx.z * nz * n;              // pair of a lockstep group
    PA += go; PB += go; WA += go; WB += go;
    const double2 u = ldw2(U + (size_t) blockIdx.z * n + p);
    const BicubicTaps t = bicubic_taps(j + u.x, i + u.y, nx, ny);
    for (int ch = 0; ch < nz; ch++) {
        double4 wa;
        double2 wb;
        bicubic_cell6<T>(t, PA + ch * n, PB + ch * n, nx, wa, wb);
        stn4(WA + ch * n + p, wa);
        stn2(WB + ch * n + p, wb);
    }
}

// psi_data, psi_gradient and the constant parts of the scheme for nz channels (:53-63, :92-104, :276-318): every sum over the
// channels runs in ascending order onto 0, psi multiplies the finished sums.
// One lane per pixel of the G pairs; n = pixels of ONE pair.
template <typename T>
__global__ void k_rexpo_coeff_c(const T *__restrict__ I1, const typename Pix<T>::v2 *__restrict__ G1,
                                const typename Pix<T>::v4 *__restrict__ WA, const typename Pix<T>::v2 *__restrict__ WB,
                                const typename Pix<T>::v2 *__restrict__ DU, const typename Pix<T>::v2 *__restrict__ DV,
                                const T *__restrict__ Dd, typename Pix<T>::v4 *__restrict__ CO, T *__restrict__ Dm, int n, int nz,
                                int G, double alpha, double gamma)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t) n * G) return;
    const size_t pair = i / (size_t) n, c0 = pair * nz * n + (i - pair * n);     // channel 0 of this pixel
    const double2 d = ldw2(DU + i);
    const double eps2 = BROX_EPSILON * BROX_EPSILON;
    double sd = 0.0, sg = 0.0, BNu = 0.0, BNv = 0.0, BDu = 0.0, BDv = 0.0, DI_Data = 0.0;
    double GNu = 0.0, GNv = 0.0, GDu = 0.0, GDv = 0.0, DI_Gradient = 0.0;
    for (int c = 0; c < nz; c++) {
        const size_t q = (size_t) c * n + c0;
        const double i1 = ldw(I1 + q);
        const double2 g1 = ldw2(G1 + q);
        const double4 wa = ldw4(WA + q);
        const double2 wb = ldw2(WB + q);
        const double I2w = wa.x, I2wx = wa.y, I2wy = wa.z, I2wxx = wa.w, I2wxy = wb.x, I2wyy = wb.y;
        const double dI = I2w + I2wx * d.x + I2wy * d.y - i1;
        sd += dI * dI;
        const double dIx = I2wx + I2wxx * d.x + I2wxy * d.y - g1.x;
        const double dIy = I2wy + I2wxy * d.x + I2wyy * d.y - g1.y;
        sg += dIx * dIx + dIy * dIy;
        const double dif = I2w - i1;
        BNu += dif * I2wx;
        BNv += dif * I2wy;
        BDu += I2wx * I2wx;
        BDv += I2wy * I2wy;
        DI_Data += (I2wy * I2wx);
        const double dx = (I2wx - g1.x), dy = (I2wy - g1.y);
        GNu += (dx * I2wxx + dy * I2wxy);
        GNv += (dx * I2wxy + dy * I2wyy);
        GDu += (I2wxx * I2wxx + I2wxy * I2wxy);
        GDv += (I2wyy * I2wyy + I2wxy * I2wxy);
        DI_Gradient += (I2wxx + I2wyy) * I2wxy;
    }
    const double psid = rnd_to<T>(1. / sqrt(sd + eps2));
    const double psig = rnd_to<T>(1. / sqrt(sg + eps2));
    const double g = gamma * psig;
    BNu = -psid * BNu; BNv = -psid * BNv; BDu = psid * BDu; BDv = psid * BDv;
    GNu = -g * GNu; GNv = -g * GNv; GDu = g * GDu; GDv = g * GDv;
    const double2 dvv = ldw2(DV + i);
    const double dd = ldw(Dd + i);
    stn4(CO + i, make_double4(BNu + GNu + alpha * dvv.x, BNv + GNv + alpha * dvv.y, BDu + GDu + dd, BDv + GDv + dd));
    stn(Dm + i, psid * DI_Data + g * DI_Gradient);
}

// One level of a lockstep group: every array holds G pairs back to back (pair g at element g * nx * ny).
template <typename T> struct BroxLevel {
    using v2 = typename Pix<T>::v2;
    using v4 = typename Pix<T>::v4;
    int nx, ny, G;
    // robust_expo: nz >= 1 channels; I1, G1, PA, PB, WA, WB hold nz channel planes each, I1c / I2c the interleaved images the
    // level starts from (rexpo_level_host, rexpo_pyramid_dev) and Mg the largest gradient magnitude of each pixel's channels.  Brox: nz = 1 and the
    // level starts from the planes I1 and I2.
    int nz = 1;
    T *I1c = nullptr, *I2c = nullptr;
    double *Mg = nullptr;
    T *I1, *I2, *Psis, *Dd, *Dm;
    v2 *G1, *PB, *WB, *U, *DV, *DU, *DUck;
    v4 *PA, *WA, *CO;
    // windowed exact mode, hyperplane-major (LaySkew), allocated on first use: (du, dv), the coefficients, psi_s and
    // snap_planes snapshot planes per pair
    v2 *DUs, *Snap;
    v4 *COs;
    T  *Dms, *Psiss;
    v2 *DUb = nullptr;    // tolerance mode (k_brox_wave): band-skewed copies of DU, CO, Dm, psi_s, allocated on first use
    v4 *COb = nullptr;
    T  *Dmb = nullptr, *Psb = nullptr;
    T  *Expo = nullptr;   // robust_expo: the smoothness weight of the level (allocated when needed)
    int snap_planes;
    int sweep_hint;
    size_t n() const { return (size_t) nx * ny; }
};

template <typename T> static int brox_level_alloc(ofx_ctx *ctx, BroxLevel<T> &L, int nx, int ny, int G, int nz = 1)
{
    const size_t n = (size_t) nx * ny * G, nc = n * nz;
    L.nx = nx;
    L.ny = ny;
    L.G = G;
    L.nz = nz;
    OFX_TRY(ofx_alloc(ctx, nc, &L.I1));
    OFX_TRY(ofx_alloc(ctx, n, &L.I2));
    OFX_TRY(ofx_alloc(ctx, n, &L.Psis));
    OFX_TRY(ofx_alloc(ctx, n, &L.Dd));
    OFX_TRY(ofx_alloc(ctx, n, &L.Dm));
    OFX_TRY(ofx_alloc(ctx, nc, &L.G1));
    OFX_TRY(ofx_alloc(ctx, nc, &L.PB));
    OFX_TRY(ofx_alloc(ctx, nc, &L.WB));
    OFX_TRY(ofx_alloc(ctx, n, &L.U));
    OFX_TRY(ofx_alloc(ctx, n, &L.DV));
    OFX_TRY(ofx_alloc(ctx, n, &L.DU));
    OFX_TRY(ofx_alloc(ctx, n, &L.DUck));
    OFX_TRY(ofx_alloc(ctx, nc, &L.PA));
    OFX_TRY(ofx_alloc(ctx, nc, &L.WA));
    OFX_TRY(ofx_alloc(ctx, n, &L.CO));
    L.Snap = L.DUs = nullptr;
    L.COs = nullptr;
    L.Dms = L.Psiss = nullptr;
    L.snap_planes = 0;
    L.sweep_hint = 0;
    return OFX_OK;
}

struct BroxParams {
    double alpha, gamma, TOL;
    int inner_iter, outer_iter, verbose;
    // robust_expo_methods: Brox's scheme with the image-driven smoothness weight `expo` and that source's own
    // summation orders (the kernels' rx / RX variants); 0 = Brox
    int robust = 0, method = 1;
    double lambda = 0.0;
    int time_windows = 0;     // ofx_robust_expo_group_dev under option "profile": iter_ms = the host's clock around the windows
};

// robust_expo_exponential_calculation (src/robust_expo_smoothness.cpp:128-187): expo = exp(-lambda |grad I1|)
// (+ 0.001 for method 2), method 3 with a per-pixel lambda bounded by the value at the 0.94 quantile of the sorted gradient
// magnitudes.  Evaluated on the HOST once per level: the reference calls libm's exp and log, whose last bit the device's
// math library does not promise to share, and method 3 sorts the level (std::sort there, here).  |grad I1| is the largest
// magnitude of the pixel's channels (k_rexpo_maxgrad on the (I1x, I1y) pairs the prepare kernel has just written).
// One pair: mg = its n gradient magnitudes, expo = its n weights, ord = n doubles of scratch for method 3's sort.
template <typename T> static void rexpo_pair_expo(const double *mg, T *expo, double *ord, size_t n, const BroxParams &P)
{
    if (P.method == 1 || P.method == 2) {
        const double beta = P.method == 2 ? 0.001 : 0.0;
        for (size_t i = 0; i < n; i++) expo[i] = (T) (exp(-P.lambda * mg[i]) + beta);
    } else {
        std::copy(mg, mg + n, ord);
        std::sort(ord, ord + n);
        const double c = -log(0.05) + log(P.alpha);
        long pos_ref = (long) (int) (0.94 * (double) (int) n);
        double lambda_omega;
        while (pos_ref < (long) n && c / 2 > ord[pos_ref - 1]) pos_ref++;
        if (pos_ref == (long) n) lambda_omega = 0;
        else lambda_omega = c / ord[pos_ref - 1];
        for (size_t i = 0; i < n; i++) {
            const double lp = (-log(0.05) + log(P.alpha)) / mg[i];
            double lambda_pi = lambda_omega;
            if (lambda_omega > lp) lambda_pi = lp;
            expo[i] = (T) exp(-lambda_pi * mg[i]);
        }
    }
}

// The G pairs of a lockstep group: ONE download of all gradient magnitudes, the pairs evaluated independently (method 3 sorts
// and takes its quantile per pair) on up to 16 / concurrency host threads -- ofx_run_groups sets `concurrency` to the number of
// contexts working at once, so a batch runs at most 16 of them --, ONE upload.  A pair is evaluated by one thread in pixel
// order whatever the thread count, so the result does not depend on it.  Levels of fewer than RX_EXPO_SERIAL pixels over all
// pairs (the coarse ones, where starting a thread costs more than the pair's exp calls) are evaluated by the caller alone.
// Every buffer is allocated here, before a thread starts: the workers allocate nothing.
#define RX_EXPO_SERIAL 32768
template <typename T> static int rexpo_level_expo(ofx_ctx *ctx, BroxLevel<T> &L, const BroxParams &P, double *host_ms)
{
    const size_t n = L.n(), ng = n * L.G;
    const int G = L.G;
    if (!L.Expo) OFX_TRY(ofx_alloc(ctx, ng, &L.Expo));
    std::vector<T> expo;
    std::vector<double> mg, ord;
    try {
        expo.resize(ng);
        mg.resize(ng);
        if (P.method == 3) ord.resize(ng);
    } catch (const std::bad_alloc &) {
        return ofx_fail(ctx, OFX_ERR_NOMEM, "robust_expo: no host memory for the expo stage of %zu pixels", ng);
    }
    if (!L.Mg) OFX_TRY(ofx_alloc(ctx, ng, &L.Mg));
    hipLaunchKernelGGL(k_rexpo_maxgrad<T>, dim3((unsigned) ((n + 255) / 256), G), dim3(256), 0, ctx->stream, L.G1, L.Mg, (int) n, L.nz);
    OFX_LAUNCH_CHECK(ctx);
    OFX_HIP(ctx, hipMemcpyAsync(mg.data(), L.Mg, ng * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    OFX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double t0 = ofx_now_ms();
    auto pairs = [&](int first, int step) {
        for (int q = first; q < G; q += step)
            rexpo_pair_expo<T>(mg.data() + q * n, expo.data() + q * n, ord.data() + (ord.empty() ? 0 : q * n), n, P);
    };
    int nt = 16 / (ctx->concurrency > 1 ? ctx->concurrency : 1);
    if (nt > G) nt = G;
    if (nt < 1 || ng < RX_EXPO_SERIAL) nt = 1;
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(pairs, t, nt);
    pairs(0, nt);
    for (auto &t : th) t.join();
    if (host_ms) *host_ms += ofx_now_ms() - t0;
    OFX_HIP(ctx, hipMemcpyAsync(L.Expo, expo.data(), ng * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    OFX_HIP(ctx, hipStreamSynchronize(ctx->stream));               // `expo` is a local
    return OFX_OK;
}

// Brox's side of sor_exact_solve: unknowns DU, constant operands CO, Dm, psi_s, alpha as the kernels' scalar.  RX: robust_expo,
// the global window kernel with that source's summation order and nothing else.  L is the level itself, as in HsExact:
// skew_in() gives it DUs, COs, Dms, Psiss
template <typename T, bool RX> struct BroxExact {
    using v2 = typename Pix<T>::v2;
    using v4 = typename Pix<T>::v4;
    static constexpr int SKEW = BROX_PLANE_C_SKEW, C = BROX_PLANE_C;
    static constexpr int LDS_K[3] = {4, 8, 16};
    static constexpr bool LDS_FOR_SMALL_GROUPS = false, ONE_KERNEL = RX;
    template <int KW> using Lds = BroxWinLds<T, KW>;
    static int qmax(int nx, int ny) { return ny + nx - 2; }
    BroxLevel<T> &L;
    double alpha;
    v2 *u() const { return L.DU; }
    v2 *us() const { return L.DUs; }
    v2 *ck() const { return L.DUck; }
    int skew_in(ofx_ctx *ctx, size_t ps, int G) const
    {
        if (!L.DUs) {
            OFX_TRY(ofx_alloc(ctx, ps * G, &L.DUs));
            OFX_TRY(ofx_alloc(ctx, ps * G, &L.COs));
            OFX_TRY(ofx_alloc(ctx, ps * G, &L.Dms));
            OFX_TRY(ofx_alloc(ctx, ps * G, &L.Psiss));
        }
        OFX_TRY((op_skew<v2, true>(ctx, L.DU, L.DUs, L.nx, L.ny, SKEW, G)));
        OFX_TRY((op_skew<v4, true>(ctx, L.CO, L.COs, L.nx, L.ny, SKEW, G)));
        OFX_TRY((op_skew<T, true>(ctx, L.Dm, L.Dms, L.nx, L.ny, SKEW, G)));
        return op_skew<T, true>(ctx, L.Psis, L.Psiss, L.nx, L.ny, SKEW, G);
    }
    template <int SPW, int MAXT> static constexpr auto window = k_brox_window<T, SPW, MAXT, RX>;
    template <int KW> static constexpr auto window_lds = k_brox_window_lds<T, KW, 256>;
    template <class Kernel>
    int launch(ofx_ctx *ctx, Kernel k, dim3 grid, dim3 blk, size_t lds, const SorWin &w, const SorGrp &grp, int sweeps) const
    {
        return sor_launch(ctx, k, grid, blk, lds, L.DUs, L.Snap, L.COs, L.Dms, L.Psiss, ctx->d_err, w, grp, sweeps, L.nx, L.ny, alpha);
    }
    int plane(ofx_ctx *ctx, int t, int s_lo, int s_cnt) const
    {
        return sor_launch(ctx, k_brox_plane<T>, dim3(ofx_cdiv(L.ny + 3, 64), s_cnt), dim3(64), 0, L.DU, L.CO, L.Dm, L.Psis,
                          ctx->d_err, t, s_lo, L.nx, L.ny, alpha);
    }
};

// src/brox_optic_flow_spatial.cpp:179-444 on device data for the G pairs of a lockstep group; stats[g] = record of pair g.
// P.robust: src/robust_expo_methods.cpp:162-455 on the level's nz >= 1 interleaved channels (the k_rexpo_* kernels)
template <typename T>
static int brox_single_scale_dev(ofx_ctx *ctx, BroxLevel<T> &L, const BroxParams &P, int scale, ofx_stats *stats)
{
    const int nx = L.nx, ny = L.ny, n = nx * ny, G = L.G;
    const size_t npix = L.n();
    const dim3 g(ofx_cdiv(nx, 64), ofx_cdiv(ny, 4), G), b = b2d();
    const dim3 g1((unsigned) ((npix * G + 255) / 256)), b1(256);
    const dim3 gc(ofx_cdiv(ofx_cdiv(nx, 2) + 1, 64), ofx_cdiv(ny, 4));
    if ((long long) npix * G >= (1LL << 31)) return ofx_fail(ctx, OFX_ERR_ARG, "brox: group larger than 2^31 pixels");
    const bool windowed = ctx->sor_exact == 1 && nx >= 3 && ny >= 3;
    // tolerance mode (sor_exact = 0, ofx_sor_tile.hip): the finest levels sweep a checkerboard of tiles in the reference's order
    // inside a tile, the coarser ones red-black; both serve lockstep groups
    const bool tol_mode = ctx->sor_exact == 0 && ctx->sor_fuse >= 0 && !P.robust;
    const bool wave = tol_mode && scale < ctx->sor_wave_levels;
    if (G > 1 && !windowed && !tol_mode)
        return ofx_fail(ctx, OFX_ERR_ARG, "brox: lockstep groups need sor_exact = 1 (levels of at least 3x3, this one %dx%d) or the tile sweeps of sor_exact = 0", nx, ny);
    int solve = 0;
    const int rx = P.robust;
    if (rx && !windowed)
        return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: needs sor_exact = 1 and levels of at least 3x3 (%dx%d)", nx, ny);
    const int nz = L.nz;                                         // robust_expo: channels (channel-planar packs)
    if (nz > 1 && !rx) return ofx_fail(ctx, OFX_ERR_ARG, "brox: only robust_expo takes %d channels", nz);
    if (rx && (!L.I1c || !L.I2c)) return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: level without its interleaved images");
    if (rx)
        hipLaunchKernelGGL(k_rexpo_prepare_c<T>, dim3(g.x, g.y, G * nz), b, 0, ctx->stream, (const T *) L.I1c, (const T *) L.I2c, L.I1, L.G1,
                           L.PA, L.PB, nx, ny, nz);
    else
        hipLaunchKernelGGL(k_brox_prepare<T>, g, b, 0, ctx->stream, (const T *) L.I1, (const T *) L.I2, L.G1, L.PA, L.PB, nx, ny);
    OFX_LAUNCH_CHECK(ctx);
    if (rx) OFX_TRY(rexpo_level_expo<T>(ctx, L, P, &ctx->expo_host_ms));                          // robust_expo_methods.cpp:231
    for (int no = 0; no < P.outer_iter; no++) {                                                   // :244
        if (rx) hipLaunchKernelGGL(k_rexpo_warp_c<T>, g, b, 0, ctx->stream, L.PA, L.PB, L.U, L.WA, L.WB, nx, ny, nz);
        else hipLaunchKernelGGL(k_brox_warp<T>, g, b, 0, ctx->stream, L.PA, L.PB, L.U, L.WA, L.WB, nx, ny);
        hipLaunchKernelGGL(k_brox_psis<T>, g, b, 0, ctx->stream, L.U, L.Psis, nx, ny, (const T *) (rx ? L.Expo : nullptr));
        hipLaunchKernelGGL(k_brox_div<T>, g, b, 0, ctx->stream, L.U, (const T *) L.Psis, L.DV, L.Dd, L.DU, nx, ny, P.alpha, rx);
        OFX_LAUNCH_CHECK(ctx);
        for (int ni = 0; ni < P.inner_iter; ni++) {                                               // :277
            if (rx)
                hipLaunchKernelGGL(k_rexpo_coeff_c<T>, g1, b1, 0, ctx->stream, (const T *) L.I1, L.G1, L.WA, L.WB, L.DU, L.DV,
                                   (const T *) L.Dd, L.CO, L.Dm, n, nz, G, P.alpha, P.gamma);
            else
                hipLaunchKernelGGL(k_brox_coeff<T>, g1, b1, 0, ctx->stream, (const T *) L.I1, L.G1, L.WA, L.WB, L.DU, L.DV,
                                   (const T *) L.Dd, L.CO, L.Dm, (int) (npix * G), P.alpha, P.gamma);
            OFX_LAUNCH_CHECK(ctx);
            int nsor[OFX_MAX_GROUP] = {0};
            double error[OFX_MAX_GROUP];
            for (int q = 0; q < G; q++) error[q] = 1000;                                          // :312
            float ms = 0.f;
            if (wave) {
                // band-skewed copies of DU, CO, Dm, psi_s (k_brox_wave)
                const size_t ps = ofx_band_plane_elems(nx, ny);
                if (!L.DUb) {
                    OFX_TRY(ofx_alloc(ctx, ps * G, &L.DUb));
                    OFX_TRY(ofx_alloc(ctx, ps * G, &L.COb));
                    OFX_TRY(ofx_alloc(ctx, ps * G, &L.Dmb));
                    OFX_TRY(ofx_alloc(ctx, ps * G, &L.Psb));
                }
                OFX_TRY((ofx_band_copy<typename Pix<T>::v2, true>(ctx, L.DU, L.DUb, nx, ny, G)));
                OFX_TRY((ofx_band_copy<typename Pix<T>::v4, true>(ctx, L.CO, L.COb, nx, ny, G)));
                OFX_TRY((ofx_band_copy<T, true>(ctx, L.Dm, L.Dmb, nx, ny, G)));
                OFX_TRY((ofx_band_copy<T, true>(ctx, L.Psis, L.Psb, nx, ny, G)));
                OFX_TRY(ofx_brox_wave_solve<T>(ctx, G, L.DUb, L.COb, (const T *) L.Dmb, (const T *) L.Psb, nx, ny, P.alpha, P.TOL,
                                               OFX_BROX_MAX_ITERATIONS, nsor, error, ctx->profile ? &ms : nullptr));
                OFX_TRY((ofx_band_copy<typename Pix<T>::v2, false>(ctx, L.DUb, L.DU, nx, ny, G)));
            } else if (ctx->sor_exact && nx >= 3 && ny >= 3) {
                // robust_expo_methods.cpp:400: the stopping value divides by nx * ny * nz.  A robust_expo group promises each pair
                // the lone solve's stopping VALUES, and the association of the stopping sum follows the window geometry (a
                // thread's K steps, then the row block's waves): its groups keep the lone geometry, 8 steps and 64 rows, where
                // Brox groups of >= 4 pairs switch to 125 rows.  Options sor_window / sor_rows still override both alike.
                // time_windows: the robust_expo group entry under option "profile"
                auto exact = [&](auto st, int Kdef, int Rdef) -> int {
                    return sor_exact_solve(ctx, st, G, n * nz, P.TOL, OFX_BROX_MAX_ITERATIONS, Kdef, Rdef, nsor, error,
                                           P.time_windows ? &ms : nullptr);
                };
                OFX_TRY(rx ? exact(BroxExact<T, true>{L, P.alpha}, 8, 64) : exact(BroxExact<T, false>{L, P.alpha}, 0, 0));
            } else if (tol_mode && ctx->sor_fuse != 9) {
                // the coarser levels of the tolerance mode: red-black, K sweeps per launch on LDS tiles (k_brox_tile; sor_fuse = 9:
                // the two launches per sweep of k_brox_sor below, for A/B)
                OFX_TRY(ofx_brox_tile_solve<T>(ctx, G, L.DU, L.DUck, L.CO, (const T *) L.Dm, (const T *) L.Psis, nx, ny, P.alpha, P.TOL,
                                               OFX_BROX_MAX_ITERATIONS, ctx->sor_fuse, nsor, error, ctx->profile ? &ms : nullptr));
            } else if (error[0] > P.TOL) {
                LoopSpec LS = sor_loop_spec(n, P.TOL);
                LS.max_iter = OFX_BROX_MAX_ITERATIONS;
                LS.chunk = sor_pick_chunk(ctx, nx, ny, 2);
                LS.fixed = ctx->fixed_work != 0;
                const int err_stride = (LS.max_iter + 1) * OFX_NSHARD;
                const dim3 gcg(gc.x, gc.y, G);
                auto launch = [&](int k, int, double thr) -> int {
                    for (int col = 0; col < 2; col++)
                        hipLaunchKernelGGL(k_brox_sor<T>, gcg, b, 0, ctx->stream, L.DU, L.CO, (const T *) L.Dm,
                                           (const T *) L.Psis, ctx->d_err, k, nx, ny, col, P.alpha, thr, err_stride);
                    OFX_LAUNCH_CHECK(ctx);
                    return OFX_OK;
                };
                OFX_TRY(ofx_run_loop_group(ctx, LS, G, launch, [](const int *) { return OFX_OK; }, nsor, error, ctx->profile ? &ms : nullptr));
            }
            if (P.verbose && G == 1) {                                                            // :392-394 / robust :414-416
                if (rx) printf("Iterations: %d Error: %g\n", nsor[0], error[0]);
                else printf("Iterations: %d\n", nsor[0]);
                fflush(stdout);
            }
            sor_record_solve(stats, G, scale, solve++, nsor, error, ms, (double) n);
        }
        hipLaunchKernelGGL(k_brox_add<T>, g1, b1, 0, ctx->stream, L.U, L.DU, (int) (npix * G));   // :398-401
        OFX_LAUNCH_CHECK(ctx);
    }
    return OFX_OK;
}

// src/brox_optic_flow_spatial.cpp:451-549 for G pairs in lockstep; on success lv[0].U holds the flows
template <typename T>
static int brox_spatial_dev(ofx_ctx *ctx, int G, const T *const *dI1, const T *const *dI2, int nx, int ny,
                            const BroxParams &P, int nscales, double nu, std::vector<BroxLevel<T>> &lv, ofx_stats *stats,
                            int kind = -1,                  // kind >= 0: the images are of that element kind (OFX_SRC_*), not T
                            size_t pitch = 0,               // ... their rows that many bytes apart, 0 = dense
                            const void *const *init = nullptr)     // G start payloads (NULL entry: zero start); nullptr: all zero
{
    if (G < 1 || G > OFX_MAX_GROUP) return ofx_fail(ctx, OFX_ERR_ARG, "brox: group of %d pairs", G);
    using V2 = typename Pix<T>::v2;
    auto levels = [&](const std::vector<int> &nxs, const std::vector<int> &nys, T **lA, T **lB, V2 **U) -> int {
        lv.resize(nscales);
        for (int s = 0; s < nscales; s++) {
            OFX_TRY(brox_level_alloc<T>(ctx, lv[s], nxs[s], nys[s], G));
            lA[s] = lv[s].I1;
            lB[s] = lv[s].I2;
        }
        *U = lv[nscales - 1].U;
        return OFX_OK;
    };
    OFX_TRY(ofx_pyramid_head<T>(ctx, G, G, (const void *const *) dI1, (const void *const *) dI2, nx, ny, nscales, nu, BROX_SIGMA,
                                P.inner_iter * P.outer_iter, stats, kind, pitch, init, levels));          // :467-509
    for (int s = nscales - 1; s >= 0; s--) {                                                      // :516
        if (P.verbose && G == 1) { printf("Scale: %d\n", s); fflush(stdout); }
        OFX_TRY(brox_single_scale_dev<T>(ctx, lv[s], P, s, stats));
        if (s)
            for (int g = 0; g < G; g++)
                OFX_TRY(op_zoom_in_flow<T>(ctx, lv[s].U + g * lv[s].n(), lv[s - 1].U + g * lv[s - 1].n(), lv[s].nx, lv[s].ny,
                                           lv[s - 1].nx, lv[s - 1].ny, 1.0 / nu));                // :529-535
    }
    return OFX_OK;
}

template <typename T>
static int brox_spatial_host(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx, int ny,
                             const BroxParams &P, int nscales, double nu)
{
    const size_t n = (size_t) nx * ny;
    T *dI1, *dI2;
    OFX_TRY(upload_plane<T>(ctx, I1, n, &dI1));
    OFX_TRY(upload_plane<T>(ctx, I2, n, &dI2));
    std::vector<BroxLevel<T>> lv;
    const T *a = dI1, *b = dI2;
    OFX_TRY(brox_spatial_dev<T>(ctx, 1, &a, &b, nx, ny, P, nscales, nu, lv, &ctx->stats));
    return download_flow<T>(ctx, lv[0].U, u, v, n);
}

// Brox's side of the pair entries (HsPairs above)
struct BroxPairs {
    using Params = BroxParams;
    template <typename T> using Level = BroxLevel<T>;
    static constexpr const char *who = "brox";
    static int check(ofx_ctx *ctx, const BroxParams &P)
    {
        if (P.inner_iter < 0 || P.outer_iter < 0) return ofx_fail(ctx, OFX_ERR_ARG, "brox: negative iteration count");
        return OFX_OK;
    }
    template <typename T, class... A> static int pyramid(A &&...a) { return brox_spatial_dev<T>(a...); }
    template <typename T> static const typename Pix<T>::v2 *flow(const BroxLevel<T> &L, int g) { return L.U + g * L.n(); }
};

extern "C" int ofx_brox_spatial(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nxx,
                                int nyy, double alpha, double gamma, int nscales, double nu, double TOL,
                                int inner_iter, int outer_iter, int verbose)
{
    OFX_ENTER(ctx);
    if (!I1 || !I2 || !u || !v) return ofx_fail(ctx, OFX_ERR_ARG, "brox: NULL pointer");
    if (inner_iter < 0 || outer_iter < 0) return ofx_fail(ctx, OFX_ERR_ARG, "brox: negative iteration count");
    const double t0 = ofx_now_ms();
    const BroxParams P = {alpha, gamma, TOL, inner_iter, outer_iter, verbose};
    int s = ctx->precision == OFX_F64 ? brox_spatial_host<double>(ctx, I1, I2, u, v, nxx, nyy, P, nscales, nu)
                                      : brox_spatial_host<float>(ctx, I1, I2, u, v, nxx, nyy, P, nscales, nu);
    ctx->stats.total_ms = ofx_now_ms() - t0;
    return s;
}

// The head of the multiscale overload (src/robust_expo_methods.cpp:494-498) for the G pairs of a lockstep group, every launch
// for all of them: image_normalization_2_color and the source's Gaussian call.  src = the G image pairs on the device in type
// S (kind >= 0: in that element kind, OFX_SRC_*), nz interleaved channels each; A, B = the level-0 images, G * nx * ny * nz
// elements each, pair g at g * nx * ny * nz.
template <typename T, typename S>
static int rexpo_normalise_presmooth_dev(ofx_ctx *ctx, int G, const OfxGroupPtrs &src, int nx, int ny, int nz, T *A, T *B, int kind,
                                         size_t pitch)         // kind >= 0: bytes between the rows of nx * nz elements, 0 = dense
{
    const size_t n = (size_t) nx * ny, nc = n * nz;
    double *scr;
    T *tmp;
    OFX_TRY(ofx_alloc(ctx, op_minmax_scratch_doubles(G, n, nz), &scr));
    OFX_TRY(ofx_alloc(ctx, (size_t) 2 * G * n, &tmp));
    // image_normalization_2_color (src/utils.cpp:334-406): per pair and channel the joint minimum / maximum of both images,
    // then 255 (x - min) / den, or a copy when den <= 0
    OfxSrcPtrs in = {};
    OfxDstPtrs out = {};
    for (int g = 0; g < G; g++) {
        in.p[2 * g] = src.a[g];
        in.p[2 * g + 1] = src.b[g];
        out.p[2 * g] = A + g * nc;
        out.p[2 * g + 1] = B + g * nc;
    }
    if (kind < 0) OFX_TRY((op_normalize_sets<T, S>(ctx, in, out, G, 2, n, nz, scr)));
    else OFX_TRY(op_normalize_sets_in<T>(ctx, kind, in, out, G, 2, nx, ny, pitch, nz, scr));
    // :497-498: gaussian(I, nxx, nyy, nzz, GAUSSIAN_SIGMA) against gaussian(I, xdim, ydim, sigma, boundary_condition, window):
    // sigma = the number of channels, boundary condition (int) 0.8 = Dirichlet, and the buffer is taken for ONE nx x ny plane --
    // so only the first nx * ny elements of each interleaved image are smoothed (across pixels and channels alike)
    return op_gaussian_group<T>(ctx, G, A, B, nc, tmp, nx, ny, (double) nz, 1);
}

// the single-scale overload itself (src/robust_expo_methods.cpp:162-178) on ONE level of nz interleaved channels: the images
// as they come, (u, v) is the initial flow
template <typename T>
static int rexpo_level_host(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx, int ny, int nz,
                            const BroxParams &P)
{
    if (nx < 1 || ny < 1) return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: bad size %dx%d", nx, ny);
    const size_t n = (size_t) nx * ny, nc = n * nz;
    if ((long long) nc >= (1LL << 31)) return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: more than 2^31 image elements");
    ofx_stats_begin(&ctx->stats, 1, P.inner_iter * P.outer_iter);
    ctx->stats.nx[0] = nx;
    ctx->stats.ny[0] = ny;
    BroxLevel<T> L;
    OFX_TRY(brox_level_alloc<T>(ctx, L, nx, ny, 1, nz));
    double *du, *dv;
    OFX_TRY(upload_plane<T>(ctx, I1, nc, &L.I1c));
    OFX_TRY(upload_plane<T>(ctx, I2, nc, &L.I2c));
    OFX_TRY(ofx_alloc(ctx, n, &du));
    OFX_TRY(ofx_alloc(ctx, n, &dv));
    OFX_HIP(ctx, hipMemcpyAsync(du, u, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    OFX_HIP(ctx, hipMemcpyAsync(dv, v, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    OFX_TRY(op_interleave2<T>(ctx, du, dv, L.U, n));
    OFX_TRY(brox_single_scale_dev<T>(ctx, L, P, 0, &ctx->stats));
    return download_flow<T>(ctx, L.U, u, v, n);
}

// The multiscale overload (src/robust_expo_methods.cpp:482-566) on nz interleaved channels at any number of scales, with ONE
// call replaced: the levels come from op_zoom_out_channels_group -- the zoom_out of the IPOL original, each channel as zoom_out --
// where the reference's zoom_out_color reads beyond its scratch copy (zoom.cpp:96-118).  Everything else is the reference's
// driver: the head above, a zero flow at the coarsest level, brox_single_scale_dev and op_zoom_in_flow per level.  Every
// robust_expo entry but the single-scale one runs it.

// Every level of G pairs is checked here, before anything is uploaded or launched.
static int rexpo_pyramid_check(ofx_ctx *ctx, int G, int nx, int ny, int nz, int nscales, double nu, std::vector<int> &nxs,
                               std::vector<int> &nys)
{
    OFX_TRY(op_pyramid_sizes(ctx, nx, ny, nscales, nu, nxs, nys));
    if ((long long) nx * ny * nz * G >= (1LL << 31)) return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: more than 2^31 image elements");
    if (nscales > 1) {
        GaussTaps taps;
        if (ofx_gauss_taps(0.6 * sqrt(1.0 / (nu * nu) - 1.0), &taps) != OFX_OK)
            return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: zoom factor %g needs more than %d taps", nu, OFX_GAUSS_MAX_TAPS);
        for (int s = 0; s + 1 < nscales; s++)
            if (taps.size >= nxs[s] || taps.size >= nys[s])
                return ofx_fail(ctx, OFX_ERR_SIGMA, "GaussianSmooth: sigma too large (radius %d, scale %d is %dx%d)", taps.size, s,
                                nxs[s], nys[s]);
    }
    for (int s = 0; s < nscales; s++)
        if (nxs[s] < 3 || nys[s] < 3)
            return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: needs levels of at least 3x3 (scale %d is %dx%d)", s, nxs[s], nys[s]);
    return OFX_OK;
}

// The G pairs of a lockstep group (src: their images on the device in type S, see rexpo_normalise_presmooth_dev); every launch
// serves all of them.  nxs, nys come from rexpo_pyramid_check; on success lv[0].U holds the G flows, stats[g] the record of pair g.
template <typename T, typename S>
static int rexpo_pyramid_dev(ofx_ctx *ctx, int G, const OfxGroupPtrs &src, int nz, const BroxParams &P, int nscales, double nu,
                             const std::vector<int> &nxs, const std::vector<int> &nys, std::vector<BroxLevel<T>> &lv,
                             ofx_stats *stats, bool t0_recorded = false,   // the caller has started the pyramid phase's clock
                             int kind = -1, size_t pitch = 0)
{
    const size_t nc = (size_t) nxs[0] * nys[0] * nz;
    for (int g = 0; g < G; g++) {
        ofx_stats_begin(&stats[g], nscales, P.inner_iter * P.outer_iter);
        for (int s = 0; s < nscales && s < OFX_MAX_SCALES; s++) { stats[g].nx[s] = nxs[s]; stats[g].ny[s] = nys[s]; }
    }
    lv.resize(nscales);
    for (int s = 0; s < nscales; s++) {
        OFX_TRY(brox_level_alloc<T>(ctx, lv[s], nxs[s], nys[s], G, nz));
        OFX_TRY(ofx_alloc(ctx, (size_t) G * nxs[s] * nys[s] * nz, &lv[s].I1c));
        OFX_TRY(ofx_alloc(ctx, (size_t) G * nxs[s] * nys[s] * nz, &lv[s].I2c));
    }
    if (ctx->profile && !t0_recorded) OFX_HIP(ctx, hipEventRecord(ctx->ev_t0, ctx->stream));
    OFX_TRY((rexpo_normalise_presmooth_dev<T, S>(ctx, G, src, nxs[0], nys[0], nz, lv[0].I1c, lv[0].I2c, kind, pitch)));  // :494-498
    if (nscales > 1) {
        T *tmpA, *tmpB;                                   // all 2 G images of a level per launch
        OFX_TRY(ofx_alloc(ctx, (size_t) 2 * G * nc, &tmpA));
        OFX_TRY(ofx_alloc(ctx, (size_t) 2 * G * nc, &tmpB));
        for (int s = 1; s < nscales; s++)                                                          // :512-520
            OFX_TRY(op_zoom_out_channels_group<T>(ctx, G, lv[s - 1].I1c, lv[s - 1].I2c, lv[s].I1c, lv[s].I2c, tmpA, tmpB, nxs[s - 1],
                                                  nys[s - 1], nz, nu));
    }
    double pyramid_ms = 0.0;
    if (ctx->profile) {
        float ms;
        OFX_HIP(ctx, hipEventRecord(ctx->ev_t1, ctx->stream));
        OFX_HIP(ctx, hipEventSynchronize(ctx->ev_t1));
        OFX_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_t0, ctx->ev_t1));
        pyramid_ms = ms;
    }
    OFX_TRY(op_fill2<T>(ctx, lv[nscales - 1].U, lv[nscales - 1].n() * G));                         // :522-524
    for (int s = nscales - 1; s >= 0; s--) {                                                      // :530
        if (P.verbose && G == 1) { printf("Scale: %d\n", s); fflush(stdout); }
        OFX_TRY(brox_single_scale_dev<T>(ctx, lv[s], P, s, stats));
        if (s)
            OFX_TRY(op_zoom_in_flow<T>(ctx, lv[s].U, lv[s - 1].U, lv[s].nx, lv[s].ny, lv[s - 1].nx, lv[s - 1].ny, 1.0 / nu, G));
    }
    for (int g = 0; g < G; g++) stats[g].pyramid_ms = pyramid_ms;
    return OFX_OK;
}

// One host image on the device in type S: the storage type through upload_plane, doubles copied as they are
template <typename S> static int rexpo_upload(ofx_ctx *ctx, const double *h, size_t n, S **out)
{
    return upload_plane<S>(ctx, h, n, out);
}
template <> int rexpo_upload<double>(ofx_ctx *ctx, const double *h, size_t n, double **out)
{
    OFX_TRY(ofx_alloc(ctx, n, out));
    OFX_HIP(ctx, hipMemcpyAsync(*out, h, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return OFX_OK;
}

// One pair of host images, uploaded in type S: double, so that the float mode rounds after the normalisation, or the storage
// type, which rounds the images as they come
template <typename T, typename S>
static int rexpo_pyramid_host(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx, int ny, int nz,
                              const BroxParams &P, int nscales, double nu)
{
    std::vector<int> nxs, nys;
    OFX_TRY(rexpo_pyramid_check(ctx, 1, nx, ny, nz, nscales, nu, nxs, nys));
    const size_t n = (size_t) nx * ny;
    S *a, *b;
    OfxGroupPtrs src;
    std::vector<BroxLevel<T>> lv;
    if (ctx->profile) OFX_HIP(ctx, hipEventRecord(ctx->ev_t0, ctx->stream));
    OFX_TRY(rexpo_upload<S>(ctx, I1, n * nz, &a));
    OFX_TRY(rexpo_upload<S>(ctx, I2, n * nz, &b));
    memset(&src, 0, sizeof(src));
    src.a[0] = a;
    src.b[0] = b;
    OFX_TRY((rexpo_pyramid_dev<T, S>(ctx, 1, src, nz, P, nscales, nu, nxs, nys, lv, &ctx->stats, true)));
    return download_flow<T>(ctx, lv[0].U, u, v, n);
}

template <typename T>
static int rexpo_group_devapi(ofx_ctx *ctx, int G, const void *const *dI1, const void *const *dI2, void *const *d_flo,
                              int nz, const BroxParams &P, int nscales, double nu, const std::vector<int> &nxs,
                              const std::vector<int> &nys, ofx_stats *stats)
{
    OfxGroupPtrs src;
    for (int g = 0; g < OFX_MAX_GROUP; g++) { src.a[g] = g < G ? dI1[g] : nullptr; src.b[g] = g < G ? dI2[g] : nullptr; }
    std::vector<BroxLevel<T>> lv;
    OFX_TRY((rexpo_pyramid_dev<T, T>(ctx, G, src, nz, P, nscales, nu, nxs, nys, lv, stats, false, ofx_src_kind(ctx),
                                     ofx_src_pitch(ctx, nxs[0] * nz))));
    const size_t n = (size_t) nxs[0] * nys[0];
    for (int g = 0; g < G; g++) OFX_TRY(op_to_flo<T>(ctx, lv[0].U + g * n, (float2 *) d_flo[g], n));
    return OFX_OK;
}

static int rexpo_check_params(ofx_ctx *ctx, int nz, int method_type, int inner_iter, int outer_iter)
{
    if (nz < 1 || nz > OFX_REXPO_MAX_CHANNELS)
        return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: nz=%d (1..%d channels)", nz, OFX_REXPO_MAX_CHANNELS);
    if (method_type < 1 || method_type > 3) return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: method_type=%d (1, 2 or 3)", method_type);
    if (inner_iter < 0 || outer_iter < 0) return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: negative iteration count");
    if (ctx->sor_exact != 1) return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: needs the default option sor_exact = 1");
    return OFX_OK;
}
static int rexpo_check_args(ofx_ctx *ctx, const double *I1, const double *I2, const double *u, const double *v, int nz, int method_type,
                            int inner_iter, int outer_iter)
{
    if (!I1 || !I2 || !u || !v) return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: NULL pointer");
    return rexpo_check_params(ctx, nz, method_type, inner_iter, outer_iter);
}

// the parameter set of every robust_expo entry; alpha as the level solver takes it
static BroxParams rexpo_params(int method_type, double alpha, double gamma, double lambda, double TOL, int inner_iter, int outer_iter,
                               int verbose)
{
    BroxParams P = {alpha, gamma, TOL, inner_iter, outer_iter, verbose};
    P.robust = 1;
    P.method = method_type;
    P.lambda = lambda;
    return P;
}
// the multiscale overload's alpha (:527): alpha * nzz as an int
static double rexpo_multiscale_alpha(double alpha, int nzz) { return (double) (int) (alpha * nzz); }

// robust_expo_methods (src/robust_expo_methods.h:21-38): one channel at any number of scales, colour at one scale.
// One channel is rounded to the storage type as it comes, before the normalisation; colour after it.
extern "C" int ofx_robust_expo(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nxx, int nyy, int nzz,
                               int method_type, double alpha, double gamma, double lambda, int nscales, double nu, double TOL,
                               int inner_iter, int outer_iter, int verbose)
{
    OFX_ENTER(ctx);
    OFX_TRY(rexpo_check_args(ctx, I1, I2, u, v, nzz, method_type, inner_iter, outer_iter));
    if (nzz != 1 && nscales != 1)
        return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: nzz=%d with nscales=%d (colour at one scale only: the reference's colour pyramid "
                                          "reads beyond its scratch copy, zoom.cpp:96-118)", nzz, nscales);
    const double t0 = ofx_now_ms();
    const BroxParams P = rexpo_params(method_type, rexpo_multiscale_alpha(alpha, nzz), gamma, lambda, TOL, inner_iter, outer_iter,
                                      verbose);
    int s;
    if (ctx->precision == OFX_F64) s = rexpo_pyramid_host<double, double>(ctx, I1, I2, u, v, nxx, nyy, nzz, P, nscales, nu);
    else if (nzz == 1) s = rexpo_pyramid_host<float, float>(ctx, I1, I2, u, v, nxx, nyy, nzz, P, nscales, nu);
    else s = rexpo_pyramid_host<float, double>(ctx, I1, I2, u, v, nxx, nyy, nzz, P, nscales, nu);
    ctx->stats.total_ms = ofx_now_ms() - t0;
    return s;
}

// ofx_robust_expo's argument list, any nzz in 1 .. OFX_REXPO_MAX_CHANNELS at any number of scales: the reference's driver on
// levels built by the per-channel zoom-out of the IPOL original.  Every channel count is rounded to the storage type after the
// normalisation.
extern "C" int ofx_robust_expo_pyramid(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nxx, int nyy,
                                       int nzz, int method_type, double alpha, double gamma, double lambda, int nscales, double nu,
                                       double TOL, int inner_iter, int outer_iter, int verbose)
{
    OFX_ENTER(ctx);
    OFX_TRY(rexpo_check_args(ctx, I1, I2, u, v, nzz, method_type, inner_iter, outer_iter));
    const double t0 = ofx_now_ms();
    const BroxParams P = rexpo_params(method_type, rexpo_multiscale_alpha(alpha, nzz), gamma, lambda, TOL, inner_iter, outer_iter,
                                      verbose);
    int s = ctx->precision == OFX_F64 ? rexpo_pyramid_host<double, double>(ctx, I1, I2, u, v, nxx, nyy, nzz, P, nscales, nu)
                                      : rexpo_pyramid_host<float, double>(ctx, I1, I2, u, v, nxx, nyy, nzz, P, nscales, nu);
    ctx->stats.total_ms = ofx_now_ms() - t0;
    return s;
}

// the single-scale overload (src/robust_expo_methods.cpp:162-178): no normalisation, no presmoothing, alpha as given, and
// (u, v) is read as the initial flow
extern "C" int ofx_robust_expo_single_scale(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx, int ny,
                                            int nz, int method_type, double alpha, double gamma, double lambda, double TOL,
                                            int inner_iter, int outer_iter, int number_of_threads, int verbose)
{
    OFX_ENTER(ctx);
    (void) number_of_threads;
    OFX_TRY(rexpo_check_args(ctx, I1, I2, u, v, nz, method_type, inner_iter, outer_iter));
    const double t0 = ofx_now_ms();
    const BroxParams P = rexpo_params(method_type, alpha, gamma, lambda, TOL, inner_iter, outer_iter, verbose);
    int s = ctx->precision == OFX_F64 ? rexpo_level_host<double>(ctx, I1, I2, u, v, nx, ny, nz, P)
                                      : rexpo_level_host<float>(ctx, I1, I2, u, v, nx, ny, nz, P);
    ctx->stats.total_ms = ofx_now_ms() - t0;
    return s;
}

extern "C" int ofx_brox_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2,
                                  void *const *d_flo, int nxx, int nyy, double alpha, double gamma, int nscales, double nu,
                                  double TOL, int inner_iter, int outer_iter, ofx_stats *stats_out)
{
    return sor_pair_group<BroxPairs>(ctx, n_pairs, dI1, dI2, nullptr, d_flo, nxx, nyy, {alpha, gamma, TOL, inner_iter, outer_iter, 0},
                                     nscales, nu, stats_out);
}

extern "C" int ofx_brox_group_init_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2,
                                       const void *const *d_flo_init, void *const *d_flo, int nxx, int nyy, double alpha,
                                       double gamma, int nscales, double nu, double TOL, int inner_iter, int outer_iter,
                                       ofx_stats *stats_out)
{
    return sor_pair_group<BroxPairs>(ctx, n_pairs, dI1, dI2, d_flo_init, d_flo, nxx, nyy,
                                     {alpha, gamma, TOL, inner_iter, outer_iter, 0}, nscales, nu, stats_out);
}

extern "C" int ofx_brox_sequence_group_dev(ofx_ctx *ctx, int n_seq, int n_frames, const void *const *dF, void *const *d_flo, int nxx,
                                           int nyy, double alpha, double gamma, int nscales_first, int nscales_next, double nu,
                                           double TOL, int inner_iter, int outer_first, int outer_next, ofx_stats *stats_out)
{
    OFX_ENTER(ctx);
    if (inner_iter < 0 || outer_first < 0 || outer_next < 0)
        return ofx_fail(ctx, OFX_ERR_ARG, "brox_sequence: negative iteration count");
    OFX_TRY(ofx_chain_check(ctx, "brox_sequence", n_seq, n_frames, dF, d_flo, nxx, nyy, nscales_first, nscales_next, nu, BROX_SIGMA));
    return ofx_chain_walk(n_seq, n_frames, dF, d_flo, stats_out,
                          [&](int t, const void *const *a, const void *const *b, const void *const *init, void *const *out,
                              ofx_stats *st) {
                              return sor_pair_group<BroxPairs>(ctx, n_seq, a, b, init, out, nxx, nyy,
                                                               {alpha, gamma, TOL, inner_iter, t ? outer_next : outer_first, 0},
                                                               t ? nscales_next : nscales_first, nu, st, true);
                          });
}

// ofx_robust_expo_pyramid for the pairs of a lockstep group on device-resident images (include/ofx.h)
extern "C" int ofx_robust_expo_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2,
                                         void *const *d_flo, int nxx, int nyy, int nzz, int method_type, double alpha,
                                         double gamma, double lambda, int nscales, double nu, double TOL, int inner_iter,
                                         int outer_iter, ofx_stats *stats_out)
{
    OFX_ENTER(ctx);
    std::vector<int> nxs, nys;
    auto check = [&]() -> int {
        OFX_TRY(rexpo_check_params(ctx, nzz, method_type, inner_iter, outer_iter));
        if (ctx->input == OFX_IN_RGB8 && nzz != 1)
            return ofx_fail(ctx, OFX_ERR_ARG, "robust_expo: OFX_IN_RGB8 frames give one gray channel (nzz = %d); interleaved channels are OFX_IN_U8", nzz);
        OFX_TRY(rexpo_pyramid_check(ctx, n_pairs, nxx, nyy, nzz, nscales, nu, nxs, nys));
        return ofx_pitch_check(ctx, "robust_expo", nxx * nzz);
    };
    return ofx_pair_group_entry(ctx, "robust_expo", n_pairs, dI1, dI2, d_flo, stats_out, check, [&](ofx_stats *st) {
        BroxParams P = rexpo_params(method_type, rexpo_multiscale_alpha(alpha, nzz), gamma, lambda, TOL, inner_iter, outer_iter, 0);
        P.time_windows = ctx->profile;
        return ctx->precision == OFX_F64 ? rexpo_group_devapi<double>(ctx, n_pairs, dI1, dI2, d_flo, nzz, P, nscales, nu, nxs, nys, st)
                                         : rexpo_group_devapi<float>(ctx, n_pairs, dI1, dI2, d_flo, nzz, P, nscales, nu, nxs, nys, st);
    });
}

extern "C" int ofx_brox_batch_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                                  void *const *d_flo, int n_pairs, int nxx, int nyy, double alpha, double gamma, int nscales,
                                  double nu, double TOL, int inner_iter, int outer_iter, double *work_pix_iters)
{
    return sor_pair_batch<BroxPairs>(ctxs, n_ctx, dI1, dI2, nullptr, d_flo, n_pairs, nxx, nyy,
                                     {alpha, gamma, TOL, inner_iter, outer_iter, 0}, nscales, nu, work_pix_iters);
}

extern "C" int ofx_brox_batch_init_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                                       const void *const *d_flo_init, void *const *d_flo, int n_pairs, int nxx, int nyy,
                                       double alpha, double gamma, int nscales, double nu, double TOL, int inner_iter,
                                       int outer_iter, double *work_pix_iters)
{
    return sor_pair_batch<BroxPairs>(ctxs, n_ctx, dI1, dI2, d_flo_init, d_flo, n_pairs, nxx, nyy,
                                     {alpha, gamma, TOL, inner_iter, outer_iter, 0}, nscales, nu, work_pix_iters);
}

// the robust_expo batch: the contexts' agreement, group size and runner of the SOR batches (sor_pair_batch) around its own group
extern "C" int ofx_robust_expo_batch_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                                         void *const *d_flo, int n_pairs, int nxx, int nyy, int nzz, int method_type,
                                         double alpha, double gamma, double lambda, int nscales, double nu, double TOL,
                                         int inner_iter, int outer_iter, double *work_pix_iters)
{
    OFX_TRY(ofx_batch_check_ctxs(ctxs, n_ctx, OFX_SAME_DEVICE | OFX_SAME_FORMAT));
    if (n_pairs < 0 || !dI1 || !dI2 || !d_flo) return OFX_ERR_ARG;
    if (n_pairs == 0) return OFX_OK;
    const int G = sor_batch_group_size(ctxs, n_ctx, n_pairs);
    return ofx_run_groups(ctxs, n_ctx, n_pairs, G, 1, work_pix_iters, true, [&](ofx_ctx *c, int first, int cnt, ofx_stats *st) {
        return ofx_robust_expo_group_dev(c, cnt, dI1 + first, dI2 + first, d_flo + first, nxx, nyy, nzz, method_type, alpha, gamma,
                                         lambda, nscales, nu, TOL, inner_iter, outer_iter, st);
    });
}

extern "C" double ofx_ctx_expo_host_ms(const ofx_ctx *ctx) { return ctx ? ctx->expo_host_ms : 0.0; }

// ============================================================================================
// Brox temporal: src/brox_optic_flow_temporal.cpp, src/brox_temporal_mask.cpp
// ============================================================================================
// A sequence of `frames` images gives nz = frames - 1 flow fields, coupled by a temporal smoothness term.  All
// arrays are frame-major (frame f at element f * nx * ny); flow field f uses I1 = frame f, I2 = frame f + 1, so the
// per-frame kernels of the spatial method (prepare, warp, coefficient assembly) are reused unchanged.  New: the
// smoothness weight with the temporal flow derivative, psi5 / psi6 and their divergence terms, the 7-point SOR
// update, and the frame dimension in the exact schedule (a sweep visits frames 1 .. nz-2, then 0, then nz-1,
// :439-459; every frame in the spatial method's pixel order).  Option sor_exact = 0 sweeps in a 3-D red-black order
// instead (ofx_broxt_tile_solve, ofx_sor_tile.hip); everything outside the sweeps is the same code.

struct Psi6 { double p1, p2, p3, p4, p5, p6; };
// src/brox_temporal_mask.cpp:18-132 at one pixel: psi1..4 within the frame, psi5 / psi6 = half-sums with the previous /
// following frame (0 outside the sequence)
template <typename T> OFX_DEV Psi6 broxt_psi6(const T *Psis, int f, int i, int j, int nx, int ny, int nz)
{
    const size_t df = (size_t) nx * ny;
    const Psi4 a = brox_psi4(Psis + f * df, i, j, nx, ny);
    const size_t k = f * df + (size_t) i * nx + j;
    const double c = ldw(Psis + k);
    Psi6 r;
    r.p1 = a.p1; r.p2 = a.p2; r.p3 = a.p3; r.p4 = a.p4;
    r.p5 = (f > 0) ? 0.5 * (ldw(Psis + k - df) + c) : 0.0;
    r.p6 = (f < nz - 1) ? 0.5 * (ldw(Psis + k + df) + c) : 0.0;
    return r;
}

// psi_smooth (:94-118) of centered_gradient3 (src/operators.cpp:413-499): the in-frame centred gradient plus the
// temporal centred difference (one-sided, still x 0.5, in the first / last frame)
// GRP (a lockstep group): blockIdx.z = g * nz + f, the temporal taps take the field f WITHIN its sequence g and never leave it
template <typename T, bool GRP>
__global__ void k_broxt_psis(const typename Pix<T>::v2 *__restrict__ U, T *__restrict__ Psis, int nx, int ny, int nz)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    const int f = GRP ? blockIdx.z % nz : blockIdx.z;
    if (j >= nx || i >= ny) return;
    const size_t df = (size_t) nx * ny;
    if (GRP) {
        const size_t so = (size_t) (blockIdx.z - f) * df;        // the sequence's first field
        U += so; Psis += so;
    }
    const typename Pix<T>::v2 *Uf = U + f * df;
    const int jl = j > 0 ? j - 1 : 0, jr = j < nx - 1 ? j + 1 : nx - 1;
    const int iu = i > 0 ? i - 1 : 0, id = i < ny - 1 ? i + 1 : ny - 1;
    const size_t p = (size_t) i * nx + j;
    const double2 r = ldw2(Uf + (size_t) i * nx + jr), l = ldw2(Uf + (size_t) i * nx + jl);
    const double2 d = ldw2(Uf + (size_t) id * nx + j), t = ldw2(Uf + (size_t) iu * nx + j);
    const double2 hi = ldw2(U + (f < nz - 1 ? f + 1 : f) * df + p), lo = ldw2(U + (f > 0 ? f - 1 : f) * df + p);
    const double ux = 0.5 * (r.x - l.x), uy = 0.5 * (d.x - t.x), ut = 0.5 * (hi.x - lo.x);
    const double vx = 0.5 * (r.y - l.y), vy = 0.5 * (d.y - t.y), vt = 0.5 * (hi.y - lo.y);
    const double du = ux * ux + uy * uy + ut * ut;
    const double dv = vx * vx + vy * vy + vt * vt;
    const double d2 = du + dv;
    stn(Psis + f * df + p, 1. / sqrt(d2 + BROX_EPSILON * BROX_EPSILON));
}

// div_u, div_v (src/brox_temporal_mask.cpp:140-239: the in-frame sum, then `+=` the temporal terms as ONE added
// expression), div_d = alpha (psi1 + ... + psi6) and du = dv = 0 (:383-390)
template <typename T, bool GRP>
__global__ void k_broxt_div(const typename Pix<T>::v2 *__restrict__ U, const T *__restrict__ Psis,
                            typename Pix<T>::v2 *__restrict__ DV, T *__restrict__ Dd, typename Pix<T>::v2 *__restrict__ DU,
                            int nx, int ny, int nz, double alpha)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    const int f = GRP ? blockIdx.z % nz : blockIdx.z;            // as k_broxt_psis
    if (j >= nx || i >= ny) return;
    const size_t df = (size_t) nx * ny;
    if (GRP) {
        const size_t so = (size_t) (blockIdx.z - f) * df;
        U += so; Psis += so; DV += so; Dd += so; DU += so;
    }
    const size_t k = f * df + (size_t) i * nx + j;
    const Psi6 s = broxt_psi6(Psis, f, i, j, nx, ny, nz);
    const double2 c = ldw2(U + k);
    double du = 0.0, dv = 0.0;
    bool have = false;
    if (i < ny - 1) { const double2 q = ldw2(U + k + nx); du = s.p1 * (q.x - c.x); dv = s.p1 * (q.y - c.y); have = true; }
    if (i > 0) {
        const double2 q = ldw2(U + k - nx);
        const double a = s.p2 * (q.x - c.x), b = s.p2 * (q.y - c.y);
        du = have ? du + a : a; dv = have ? dv + b : b; have = true;
    }
    if (j < nx - 1) {
        const double2 q = ldw2(U + k + 1);
        const double a = s.p3 * (q.x - c.x), b = s.p3 * (q.y - c.y);
        du = have ? du + a : a; dv = have ? dv + b : b; have = true;
    }
    if (j > 0) {
        const double2 q = ldw2(U + k - 1);
        const double a = s.p4 * (q.x - c.x), b = s.p4 * (q.y - c.y);
        du = have ? du + a : a; dv = have ? dv + b : b; have = true;
    }
    if (nz > 1) {
        if (f > 0 && f < nz - 1) {
            const double2 lo = ldw2(U + k - df), hi = ldw2(U + k + df);
            du += s.p5 * (lo.x - c.x) + s.p6 * (hi.x - c.x);
            dv += s.p5 * (lo.y - c.y) + s.p6 * (hi.y - c.y);
        } else if (f == 0) {
            const double2 hi = ldw2(U + k + df);
            du += s.p6 * (hi.x - c.x);
            dv += s.p6 * (hi.y - c.y);
        } else {
            const double2 lo = ldw2(U + k - df);
            du += s.p5 * (lo.x - c.x);
            dv += s.p5 * (lo.y - c.y);
        }
    }
    stn2(DV + k, make_double2(du, dv));
    stn(Dd + k, alpha * (s.p1 + s.p2 + s.p3 + s.p4 + s.p5 + s.p6));
    stn2(DU + k, make_double2(0.0, 0.0));
}

// SOR update of one pixel of frame f, :120-170; a missing neighbour (row, column or frame) is the pixel itself with
// psi = 0.  The new value also goes into the sweep's snapshot.
template <typename T>
OFX_DEV double broxt_point(typename Pix<T>::v2 *DU, typename Pix<T>::v2 *snap, const typename Pix<T>::v4 *__restrict__ CO,
                           const T *__restrict__ Dm, const T *__restrict__ Psis, int f, int i, int j, int nx, int ny, int nz,
                           double alpha)
{
    const size_t df = (size_t) nx * ny;
    const size_t k = f * df + (size_t) i * nx + j;
    const Psi6 s = broxt_psi6(Psis, f, i, j, nx, ny, nz);
    const double2 c = ldw2(DU + k);
    const double2 dn = (i < ny - 1) ? ldw2(DU + k + nx) : c, up = (i > 0) ? ldw2(DU + k - nx) : c;
    const double2 rt = (j < nx - 1) ? ldw2(DU + k + 1) : c, lf = (j > 0) ? ldw2(DU + k - 1) : c;
    const double2 pv = (f > 0) ? ldw2(DU + k - df) : c, nxt = (f < nz - 1) ? ldw2(DU + k + df) : c;
    const double4 co = ldw4(CO + k);
    const double D = ldw(Dm + k);
    const double w = BROX_SOR_W;
    const double div_du = s.p1 * dn.x + s.p2 * up.x + s.p3 * rt.x + s.p4 * lf.x + s.p5 * pv.x + s.p6 * nxt.x;      // :157-159
    const double div_dv = s.p1 * dn.y + s.p2 * up.y + s.p3 * rt.y + s.p4 * lf.y + s.p5 * pv.y + s.p6 * nxt.y;      // :160-162
    const double duk = c.x, dvk = c.y;
    const double dun = rnd_to<T>((1. - w) * duk + w * (co.x - D * dvk + alpha * div_du) / co.z);   // :167
    const double dvn = rnd_to<T>((1. - w) * dvk + w * (co.y - D * dun + alpha * div_dv) / co.w);   // :168
    stn2(DU + k, make_double2(dun, dvn));
    stn2(snap + k, make_double2(dun, dvn));
    return (dun - duk) * (dun - duk) + (dvn - dvk) * (dvn - dvk);                                  // :171
}

// Windowed exact schedule (k_brox_window) with the frame dimension: one workgroup per (sequence, sweep, frame, row block).
// broxt_window_unit is the K steps of one such unit on the sequence's own arrays, snapshot plane and error slots; o = the position
// of the frame in the sweep's visiting order: frames 1 .. nz-2, then 0, then nz-1 (:439-459).  In a lockstep group
// (k_broxt_window_group) blockIdx.y = g * nz + o for sequence g (SorGrp: npix = the nz fields of one sequence).  A sequence whose
// solve has stopped and an idle unit leave before the first barrier; both tests are uniform over the workgroup.
template <typename T>
OFX_DEV void broxt_window_unit(typename Pix<T>::v2 *DU, typename Pix<T>::v2 *mysnap, const typename Pix<T>::v4 *__restrict__ CO,
                               const T *__restrict__ Dm, const T *__restrict__ Psis, double *__restrict__ err, const SorWin &w, int o,
                               int s, int q_first, int nx, int ny, int nz, double alpha)
{
    const int b = blockIdx.x;
    const int f = (o < nz - 2) ? o + 1 : (o == nz - 2 ? 0 : nz - 1);
    const int qmax = ny + nx - 2;
    const int r = sor_window_item(w, b, threadIdx.x, ny);
    double e = 0.0;
    for (int q = q_first; q < q_first + w.K; q++) {
        if (q >= 0 && q <= qmax && r >= 0) {
            int i, j;
            if (r == ny + 2) {
                for (int corner = 0; corner < 4; corner++)
                    if (brox_plane_item(r, q, nx, ny, corner, i, j) && sor_border_block(i, ny, w.R) == b)
                        e += broxt_point<T>(DU, mysnap, CO, Dm, Psis, f, i, j, nx, ny, nz, alpha);
            } else if (brox_plane_item(r, q, nx, ny, 0, i, j) && (r < ny || sor_border_block(i, ny, w.R) == b)) {
                e += broxt_point<T>(DU, mysnap, CO, Dm, Psis, f, i, j, nx, ny, nz, alpha);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // One shard per (frame, row block, wave) while nz * row blocks * waves <= OFX_NSHARD (640x480 x 5 frames: 4 * 8 * 2): every
    // shard then receives ONE add per launch, in stream order, and the stopping sum is associated the same way in every run, alone
    // or in a group.  (The former (o * 8 + b) * 4 + wave wrapped at o = 2, so frames o and o + 2 raced for a shard.)  Larger
    // levels wrap and add atomically into shared shards.
    loop_accumulate(err, s, e, (o * (int) gridDim.x + b) * (int) (blockDim.x >> 6) + (threadIdx.x >> 6));
}
// a lone sequence: blockIdx.y = o.  The exact mode of a lone solve is bound by the host's launch rate, so this kernel keeps the
// short argument list and the group has a kernel of its own.
template <typename T>
__global__ __launch_bounds__(1024) void k_broxt_window(typename Pix<T>::v2 *DU, typename Pix<T>::v2 *snap,
                                                       const typename Pix<T>::v4 *__restrict__ CO, const T *__restrict__ Dm,
                                                       const T *__restrict__ Psis, double *__restrict__ err, SorWin w,
                                                       int nx, int ny, int nz, double alpha)
{
    const int o = blockIdx.y, s = w.s_first + blockIdx.z;
    const int q_first = w.tau0 - w.lag_s * s - w.lag_f * o - w.lag_b * (int) blockIdx.x;
    if (sor_unit_idle(w, blockIdx.x, q_first, w.K, 1, nx, ny)) return;
    broxt_window_unit<T>(DU, snap + (size_t) s * nz * nx * ny, CO, Dm, Psis, err, w, o, s, q_first, nx, ny, nz, alpha);
}
template <typename T>
__global__ __launch_bounds__(1024) void k_broxt_window_group(typename Pix<T>::v2 *DU, typename Pix<T>::v2 *snap,
                                                             const typename Pix<T>::v4 *__restrict__ CO, const T *__restrict__ Dm,
                                                             const T *__restrict__ Psis, double *__restrict__ err, SorWin w, SorGrp grp,
                                                             int nx, int ny, int nz, double alpha)
{
    const int g = blockIdx.y / nz;
    if (!((grp.runmask >> g) & 1u)) return;                      // this sequence's solve has already stopped
    const int o = blockIdx.y - g * nz, s = w.s_first + blockIdx.z;
    const int q_first = w.tau0 - w.lag_s * s - w.lag_f * o - w.lag_b * (int) blockIdx.x;
    if (sor_unit_idle(w, blockIdx.x, q_first, w.K, 1, nx, ny)) return;
    broxt_window_unit<T>(DU + g * grp.npix, snap + g * grp.snap_stride + (size_t) s * grp.npix, CO + g * grp.npix, Dm + g * grp.npix,
                         Psis + g * grp.npix, err + (size_t) g * grp.err_stride, w, o, s, q_first, nx, ny, nz, alpha);
}

// One level of G sequences in lockstep: sequence g's frames at frame g * frames of I, its flow fields at field g * nz of
// every other array -- a sequence is nz planes back to back, a group G sequences back to back.
template <typename T> struct BroxtLevel {
    using v2 = typename Pix<T>::v2;
    using v4 = typename Pix<T>::v4;
    int nx, ny;
    T *I;                       // G * frames * n
    T *Psis, *Dd, *Dm;          // G * nz * n each
    v2 *G1, *PB, *WB, *U, *DV, *DU, *Snap;
    v4 *PA, *WA, *CO;
    int snap_planes, sweep_hint;
};

template <typename T> static int broxt_level_alloc(ofx_ctx *ctx, BroxtLevel<T> &L, int nx, int ny, int frames, int G)
{
    const size_t n1 = (size_t) nx * ny * (frames - 1) * G;
    L.nx = nx;
    L.ny = ny;
    OFX_TRY(ofx_alloc(ctx, (size_t) nx * ny * frames * G, &L.I));
    OFX_TRY(ofx_alloc(ctx, n1, &L.Psis));
    OFX_TRY(ofx_alloc(ctx, n1, &L.Dd));
    OFX_TRY(ofx_alloc(ctx, n1, &L.Dm));
    OFX_TRY(ofx_alloc(ctx, n1, &L.G1));
    OFX_TRY(ofx_alloc(ctx, n1, &L.PB));
    OFX_TRY(ofx_alloc(ctx, n1, &L.WB));
    OFX_TRY(ofx_alloc(ctx, n1, &L.U));
    OFX_TRY(ofx_alloc(ctx, n1, &L.DV));
    OFX_TRY(ofx_alloc(ctx, n1, &L.DU));
    OFX_TRY(ofx_alloc(ctx, n1, &L.PA));
    OFX_TRY(ofx_alloc(ctx, n1, &L.WA));
    OFX_TRY(ofx_alloc(ctx, n1, &L.CO));
    L.Snap = nullptr;
    L.snap_planes = 0;
    L.sweep_hint = 0;
    return OFX_OK;
}

// src/brox_optic_flow_temporal.cpp:282-512 on device data
template <typename T>
static int broxt_single_scale_dev(ofx_ctx *ctx, BroxtLevel<T> &L, const BroxParams &P, int frames, int scale, int G, ofx_stats *stats)
{
    const int nx = L.nx, ny = L.ny, nz = frames - 1, n = nx * ny;
    const size_t n1 = (size_t) n * nz, nG = n1 * G;              // the fields of one sequence, of the group
    if ((long long) n * frames * G >= (1LL << 31)) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: group larger than 2^31 pixels");
    if (nx < 3 || ny < 3) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: level %dx%d has no interior", nx, ny);
    const dim3 g = g2d(nx, ny), b = b2d(), g3(g.x, g.y, G * nz);
    const dim3 g1((unsigned) ((nG + 255) / 256)), b1(256);
    int solve = 0;
    // :346-355 for all flow fields of all sequences at once (blockIdx.z = g * nz + f): I1 = frame f, I2 = frame f + 1 of
    // sequence g of the frame-major level
    // (a lone sequence launches the lone kernels with their short argument lists throughout: it is bound by the host's launch rate)
    if (G == 1) hipLaunchKernelGGL(k_brox_prepare<T>, g3, b, 0, ctx->stream, (const T *) L.I, (const T *) (L.I + n), L.G1, L.PA, L.PB, nx, ny);
    else hipLaunchKernelGGL(k_broxt_prepare_group<T>, g3, b, 0, ctx->stream, (const T *) L.I, L.G1, L.PA, L.PB, nx, ny, nz);
    OFX_LAUNCH_CHECK(ctx);
    for (int no = 0; no < P.outer_iter; no++) {                                                      // :358
        hipLaunchKernelGGL(k_brox_warp<T>, g3, b, 0, ctx->stream, L.PA, L.PB, L.U, L.WA, L.WB, nx, ny);   // :360-367
        if (G == 1) {
            hipLaunchKernelGGL((k_broxt_psis<T, false>), g3, b, 0, ctx->stream, L.U, L.Psis, nx, ny, nz);      // :370-374
            hipLaunchKernelGGL((k_broxt_div<T, false>), g3, b, 0, ctx->stream, L.U, (const T *) L.Psis, L.DV, L.Dd, L.DU, nx, ny, nz,
                               P.alpha);                                                             // :377-390
        } else {
            hipLaunchKernelGGL((k_broxt_psis<T, true>), g3, b, 0, ctx->stream, L.U, L.Psis, nx, ny, nz);
            hipLaunchKernelGGL((k_broxt_div<T, true>), g3, b, 0, ctx->stream, L.U, (const T *) L.Psis, L.DV, L.Dd, L.DU, nx, ny, nz,
                               P.alpha);
        }
        OFX_LAUNCH_CHECK(ctx);
        for (int ni = 0; ni < P.inner_iter; ni++) {                                                  // :394
            if (G == 1)
                hipLaunchKernelGGL(k_brox_coeff<T>, g1, b1, 0, ctx->stream, (const T *) L.I, L.G1, L.WA, L.WB, L.DU, L.DV,
                                   (const T *) L.Dd, L.CO, L.Dm, (int) nG, P.alpha, P.gamma);        // :396-427
            else
                hipLaunchKernelGGL(k_broxt_coeff_group<T>, g1, b1, 0, ctx->stream, (const T *) L.I, L.G1, L.WA, L.WB, L.DU, L.DV,
                                   (const T *) L.Dd, L.CO, L.Dm, (int) nG, P.alpha, P.gamma, (int) n1, n);
            OFX_LAUNCH_CHECK(ctx);
            int nsor[OFX_MAX_GROUP] = {0};
            double error[OFX_MAX_GROUP];
            for (int q = 0; q < G; q++) error[q] = 1000;
            if (ctx->sor_exact == 0) {
                // tolerance mode: 3-D red-black sweeps (ofx_sor_tile.hip).  No snapshots; ONE plane of them per sequence is the
                // second buffer of the tile kernel's ping-pong, so the memory rule of the exact mode bounds this one too.
                OFX_TRY(sor_snap_reserve(ctx, &L.Snap, &L.snap_planes, n1, 1, G));
                OFX_TRY(ofx_broxt_tile_solve<T>(ctx, G, L.DU, L.Snap, L.CO, (const T *) L.Dm, (const T *) L.Psis, nx, ny, nz, P.alpha,
                                                P.TOL, OFX_BROX_MAX_ITERATIONS, ctx->sor_fuse, nsor, error, nullptr));
                if (P.verbose && G == 1) { printf("Iterations: %d\n", nsor[0]); fflush(stdout); }    // :463-465
                sor_record_solve(stats, G, scale, solve++, nsor, error, 0.f, (double) n1);
                continue;
            }
            // Every sequence of a group gets the stopping VALUES of its lone solve, and the association of the stopping sum
            // follows the window geometry (a thread's K steps, then the shard of its frame, row block and wave): groups keep the lone
            // geometry, 8 steps and 64 rows, as the robust_expo groups do.  Options sor_window / sor_rows override both alike.
            const size_t ub = n1 * sizeof(typename Pix<T>::v2);
            const int batch = sor_pick_batch(ctx, n1, sizeof(typename Pix<T>::v2), OFX_BROX_MAX_ITERATIONS, G);
            OFX_TRY(sor_snap_reserve(ctx, &L.Snap, &L.snap_planes, n1, batch, G));
            const size_t snap_stride = n1 * L.snap_planes;
            auto window = [&](const SorWin &w, int blocks, int sweeps, unsigned runmask, int err_stride) -> int {
                const SorGrp grp = {runmask, err_stride, n1, snap_stride};
                const dim3 grid(blocks, G * nz, sweeps), blk(sor_window_threads(w.R + 3));
                if (G == 1)
                    hipLaunchKernelGGL(k_broxt_window<T>, grid, blk, 0, ctx->stream, L.DU, L.Snap, L.CO, (const T *) L.Dm,
                                       (const T *) L.Psis, ctx->d_err, w, nx, ny, nz, P.alpha);
                else
                    hipLaunchKernelGGL(k_broxt_window_group<T>, grid, blk, 0, ctx->stream, L.DU, L.Snap, L.CO, (const T *) L.Dm,
                                       (const T *) L.Psis, ctx->d_err, w, grp, nx, ny, nz, P.alpha);
                OFX_LAUNCH_CHECK(ctx);
                return OFX_OK;
            };
            auto take = [&](int q, int k) -> int {
                OFX_HIP(ctx, hipMemcpyAsync(L.DU + q * n1, L.Snap + q * snap_stride + (size_t) (k - 1) * n1, ub,
                                            hipMemcpyDeviceToDevice, ctx->stream));
                return OFX_OK;
            };
            OFX_TRY(sor_window_loop(ctx, G, (int) n1, ny, P.TOL, OFX_BROX_MAX_ITERATIONS, ny + nx - 2, BROX_PLANE_C, batch, window,
                                    take, nsor, error, nz, &L.sweep_hint, 8, 64));                                  // :430-461
            if (P.verbose && G == 1) { printf("Iterations: %d\n", nsor[0]); fflush(stdout); }        // :463-465
            sor_record_solve(stats, G, scale, solve++, nsor, error, 0.f, (double) n1);
        }
        hipLaunchKernelGGL(k_brox_add<T>, g1, b1, 0, ctx->stream, L.U, L.DU, (int) nG);                // :469-472
        OFX_LAUNCH_CHECK(ctx);
    }
    return OFX_OK;
}

// ---- the driver, src/brox_optic_flow_temporal.cpp:520-627, on a device-resident sequence ------------------------------------
// Every stage outside the level solver is one launch for all frames / flow fields (the frame or field in blockIdx.z or .y) with
// the operators' per-pixel code.  The caller's frames reach the head through the by-value pointer table of ofx_ops.h
// (OFX_BROXT_MAX_FRAMES entries); a longer sequence (the host entry takes any length) goes through in chunks of that many.
struct BroxtFlos { float2 *flo[OFX_BROXT_MAX_FRAMES]; };
// the .flo payloads of flow fields blockIdx.z of a chunk: (float) u, (float) v interleaved, as k_to_flo
template <typename T> __global__ void k_broxt_out(const typename Pix<T>::v2 *__restrict__ U, BroxtFlos out, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 v = ldw2(U + (size_t) blockIdx.z * n + i);
    out.flo[blockIdx.z][i] = make_float2((float) v.x, (float) v.y);
}

// What every temporal entry checks before any work, in the order in which the solve would meet it: the pyramid's sizes, the
// presmoothing Gaussian on level 0 and the zoom Gaussian on every level that is zoomed out (op_gaussian_planes' rule), the 3x3
// minimum of the level solver and the index range.
static int broxt_check(ofx_ctx *ctx, int frames, int nxx, int nyy, int nscales, double nu, int inner_iter, int outer_iter,
                       std::vector<int> &nxs, std::vector<int> &nys)
{
    if (frames <= 2) return ofx_fail(ctx, OFX_ERR_ARG, "The method needs more than two frames");     // :537-541
    if (inner_iter < 0 || outer_iter < 0) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: negative iteration count");
    if (nxx < 3 || nyy < 3) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: images smaller than 3x3");
    OFX_TRY(op_pyramid_sizes(ctx, nxx, nyy, nscales, nu, nxs, nys));
    for (int pass = 0; pass < (nscales > 1 ? 2 : 1); pass++) {     // presmoothing: level 0; zoom-out: every level but the coarsest
        const double sigma = pass ? 0.6 * sqrt(1.0 / (nu * nu) - 1.0) : BROX_SIGMA;
        GaussTaps taps;
        if (ofx_gauss_taps(sigma, &taps) != OFX_OK)
            return ofx_fail(ctx, OFX_ERR_ARG, "gaussian: sigma %g needs more than %d taps", sigma, OFX_GAUSS_MAX_TAPS);
        for (int s = 0; s < (pass ? nscales - 1 : 1); s++)
            if (taps.size >= nxs[s] || taps.size >= nys[s])
                return ofx_fail(ctx, OFX_ERR_SIGMA, "GaussianSmooth: sigma too large (radius %d, scale %d is %dx%d)", taps.size, s,
                                nxs[s], nys[s]);
    }
    for (int s = 0; s < nscales; s++)
        if (nxs[s] < 3 || nys[s] < 3)
            return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: level %dx%d has no interior", nxs[s], nys[s]);
    if ((long long) nxx * nyy * frames >= (1LL << 31)) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: sequence larger than 2^31 pixels");
    return OFX_OK;
}

// The solve of G sequences in lockstep: dF = their frames on the device in storage type T (kind >= 0: in that element kind,
// OFX_SRC_*), sequence g's at dF + g * frames; nxs,
// nys from broxt_check.  On success lv[0].U holds the G * (frames - 1) flows of the finest level and stats[g] the record of
// sequence g.  Every launch of the head serves as many planes of the group as the by-value tables hold.
template <typename T>
static int broxt_sequence_dev(ofx_ctx *ctx, int G, int frames, const void *const *dF, const BroxParams &P, int nscales, double nu,
                              const std::vector<int> &nxs, const std::vector<int> &nys, std::vector<BroxtLevel<T>> &lv, ofx_stats *stats,
                              int kind = -1, size_t pitch = 0)       // kind >= 0: bytes between the frames' rows, 0 = dense
{
    const int nx = nxs[0], ny = nys[0], MF = OFX_BROXT_MAX_FRAMES;
    if (kind < 0) kind = ofx_storage_kind(ctx);
    const size_t n = (size_t) nx * ny;
    if (G < 1 || G > OFX_MAX_GROUP || (G > 1 && frames > MF)) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: group of %d sequences", G);
    const int planes = G * frames, tmp_planes = planes < MF ? planes : MF;
    for (int g = 0; g < G; g++) ofx_stats_begin(&stats[g], nscales, P.inner_iter * P.outer_iter);
    T *tmpA, *tmpB = nullptr;
    double *mm;
    // image_normalization_1 (:548) has one {min, max} set per SEQUENCE.  A table holds the frames of `per_launch` whole sequences
    // (sets of one chunk); a sequence longer than the table (host entry, G = 1) is one set in `chunks` chunks.
    const int chunks = (frames + MF - 1) / MF, per_launch = frames <= MF ? MF / frames : 1;
    const size_t mm_doubles = op_minmax_scratch_doubles(per_launch, n, 1, chunks);
    OFX_TRY(ofx_alloc(ctx, n * tmp_planes, &tmpA));
    if (nscales > 1) OFX_TRY(ofx_alloc(ctx, n * tmp_planes, &tmpB));
    OFX_TRY(ofx_alloc(ctx, mm_doubles * ((G + per_launch - 1) / per_launch), &mm));
    lv.resize(nscales);
    for (int s = 0; s < nscales; s++) {
        OFX_TRY(broxt_level_alloc<T>(ctx, lv[s], nxs[s], nys[s], frames, G));
        for (int g = 0; g < G && s < OFX_MAX_SCALES; g++) { stats[g].nx[s] = nxs[s]; stats[g].ny[s] = nys[s]; }
    }
    if (chunks > 1) {                                            // one long sequence: a chunk of the table's size per launch
        for (int f0 = 0; f0 < frames; f0 += MF) {
            const int cnt = frames - f0 < MF ? frames - f0 : MF;
            OfxSrcPtrs in = {};
            for (int k = 0; k < cnt; k++) in.p[k] = dF[f0 + k];
            OFX_TRY(op_minmax_partial_in(ctx, kind, in, 1, cnt, nx, ny, pitch, 1, mm, f0 / MF, chunks));
        }
        OFX_TRY(op_minmax_final(ctx, 1, n, 1, mm, chunks));
        for (int f0 = 0; f0 < frames; f0 += MF) {
            const int cnt = frames - f0 < MF ? frames - f0 : MF;
            OfxSrcPtrs in = {};
            OfxDstPtrs out = {};
            for (int k = 0; k < cnt; k++) { in.p[k] = dF[f0 + k]; out.p[k] = lv[0].I + (f0 + k) * n; }
            OFX_TRY(op_normalize_map_in<T>(ctx, kind, in, out, 1, cnt, nx, ny, pitch, 1, mm));
        }
    } else {
        for (int g0 = 0; g0 < G; g0 += per_launch) {
            const int sets = G - g0 < per_launch ? G - g0 : per_launch;
            OfxSrcPtrs in = {};
            OfxDstPtrs out = {};
            for (int k = 0; k < sets * frames; k++) { in.p[k] = dF[g0 * frames + k]; out.p[k] = lv[0].I + (size_t) (g0 * frames + k) * n; }
            OFX_TRY(op_normalize_sets_in<T>(ctx, kind, in, out, sets, frames, nx, ny, pitch, 1, mm + (g0 / per_launch) * mm_doubles));
        }
    }
    for (int f0 = 0; f0 < planes; f0 += MF) {                                                        // :551-553
        const int cnt = planes - f0 < MF ? planes - f0 : MF;
        OFX_TRY(op_gaussian_planes<T>(ctx, cnt, cnt, lv[0].I + f0 * n, nullptr, n, tmpA, nx, ny, BROX_SIGMA));
    }
    for (int s = 1; s < nscales; s++) {                                                              // :561-575
        const size_t np = (size_t) nxs[s - 1] * nys[s - 1], nc = (size_t) nxs[s] * nys[s];
        for (int f0 = 0; f0 < planes; f0 += MF) {
            const int cnt = planes - f0 < MF ? planes - f0 : MF;
            OFX_TRY(op_zoom_out_channels_planes<T>(ctx, cnt, cnt, lv[s - 1].I + f0 * np, nullptr, lv[s].I + f0 * nc, nullptr, tmpA, tmpB,
                                                   nxs[s - 1], nys[s - 1], 1, nu));
        }
    }
    BroxtLevel<T> &C = lv[nscales - 1];
    OFX_TRY(op_fill2<T>(ctx, C.U, (size_t) C.nx * C.ny * (frames - 1) * G));                         // :578-580
    for (int s = nscales - 1; s >= 0; s--) {                                                        // :587
        if (P.verbose && G == 1) { printf("Scale: %d\n", s); fflush(stdout); }
        OFX_TRY(broxt_single_scale_dev<T>(ctx, lv[s], P, frames, s, G, stats));
        if (s)
            OFX_TRY(op_zoom_in_flow<T>(ctx, lv[s].U, lv[s - 1].U, lv[s].nx, lv[s].ny, lv[s - 1].nx, lv[s - 1].ny, 1.0 / nu,
                                       (frames - 1) * G));                                           // :600-612
    }
    return OFX_OK;
}

// host planes: upload the frames in the storage type, the driver, download
template <typename T>
static int broxt_host(ofx_ctx *ctx, const double *I, double *u, double *v, int frames, const BroxParams &P, int nscales, double nu,
                      const std::vector<int> &nxs, const std::vector<int> &nys)
{
    const size_t n = (size_t) nxs[0] * nys[0];
    T *dI;
    OFX_TRY(upload_plane<T>(ctx, I, n * frames, &dI));
    std::vector<const void *> dF(frames);
    for (int k = 0; k < frames; k++) dF[k] = dI + k * n;
    std::vector<BroxtLevel<T>> lv;
    OFX_TRY(broxt_sequence_dev<T>(ctx, 1, frames, dF.data(), P, nscales, nu, nxs, nys, lv, &ctx->stats));
    return download_flow<T>(ctx, lv[0].U, u, v, n * (frames - 1));
}

extern "C" int ofx_brox_temporal(ofx_ctx *ctx, const double *I, double *u, double *v, int nxx, int nyy, int frames,
                                 double alpha, double gamma, int nscales, double nu, double TOL, int inner_iter,
                                 int outer_iter, int verbose)
{
    OFX_ENTER(ctx);
    if (!I || !u || !v) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: NULL pointer");
    std::vector<int> nxs, nys;
    OFX_TRY(broxt_check(ctx, frames, nxx, nyy, nscales, nu, inner_iter, outer_iter, nxs, nys));
    const double t0 = ofx_now_ms();
    const BroxParams P = {alpha, gamma, TOL, inner_iter, outer_iter, verbose};
    int s = ctx->precision == OFX_F64 ? broxt_host<double>(ctx, I, u, v, frames, P, nscales, nu, nxs, nys)
                                      : broxt_host<float>(ctx, I, u, v, frames, P, nscales, nu, nxs, nys);
    ctx->stats.total_ms = ofx_now_ms() - t0;
    return s;
}

// the pointer tables of n_seq sequences: no NULL, the frames aligned to their element, the payloads to a float2
static int broxt_check_ptrs(ofx_ctx *ctx, int n_seq, int frames, const void *const *dF, void *const *d_flo)
{
    if (!dF || !d_flo) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: NULL pointer array");
    const size_t el = ofx_src_align(ofx_src_kind(ctx));
    for (int k = 0; k < n_seq * frames; k++)
        if (!dF[k] || reinterpret_cast<uintptr_t>(dF[k]) % el)
            return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: frame %d (sequence %d) NULL or misaligned", k % frames, k / frames);
    for (int k = 0; k < n_seq * (frames - 1); k++)
        if (!d_flo[k] || reinterpret_cast<uintptr_t>(d_flo[k]) % sizeof(float2))
            return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: payload pointer %d (sequence %d) NULL or misaligned", k % (frames - 1),
                            k / (frames - 1));
    return OFX_OK;
}
// everything the device entries refuse, for n_seq sequences
static int broxt_dev_check(ofx_ctx *ctx, int n_seq, int frames, const void *const *dF, void *const *d_flo, int nxx, int nyy,
                           int nscales, double nu, int inner_iter, int outer_iter, std::vector<int> &nxs, std::vector<int> &nys)
{
    OFX_TRY(broxt_check(ctx, frames, nxx, nyy, nscales, nu, inner_iter, outer_iter, nxs, nys));
    if (frames > OFX_BROXT_MAX_FRAMES)
        return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: %d frames (a device-resident sequence holds at most %d)", frames, OFX_BROXT_MAX_FRAMES);
    OFX_TRY(ofx_pitch_check(ctx, "brox temporal", nxx));
    return broxt_check_ptrs(ctx, n_seq, frames, dF, d_flo);
}

// G sequences in lockstep and their payloads: the table of k_broxt_out holds OFX_BROXT_MAX_FRAMES fields per launch
template <typename T>
static int broxt_devapi(ofx_ctx *ctx, int G, int frames, const void *const *dF, void *const *d_flo, const BroxParams &P, int nscales,
                        double nu, const std::vector<int> &nxs, const std::vector<int> &nys, ofx_stats *stats)
{
    std::vector<BroxtLevel<T>> lv;
    OFX_TRY(broxt_sequence_dev<T>(ctx, G, frames, dF, P, nscales, nu, nxs, nys, lv, stats, ofx_src_kind(ctx), ofx_src_pitch(ctx, nxs[0])));
    const size_t n = (size_t) nxs[0] * nys[0];
    const int fields = G * (frames - 1);
    for (int f0 = 0; f0 < fields; f0 += OFX_BROXT_MAX_FRAMES) {
        const int cnt = fields - f0 < OFX_BROXT_MAX_FRAMES ? fields - f0 : OFX_BROXT_MAX_FRAMES;
        BroxtFlos out = {};
        for (int f = 0; f < cnt; f++) out.flo[f] = static_cast<float2 *>(d_flo[f0 + f]);
        hipLaunchKernelGGL(k_broxt_out<T>, dim3((unsigned) ((n + 255) / 256), 1, cnt), dim3(256), 0, ctx->stream, lv[0].U + f0 * n, out,
                           (int) n);
        OFX_LAUNCH_CHECK(ctx);
    }
    return OFX_OK;
}

// the checked solve of G sequences under the group shell; stats_out: G records, or NULL
static int broxt_dev_run(ofx_ctx *ctx, int G, int frames, const void *const *dF, void *const *d_flo, double alpha, double gamma,
                         int nscales, double nu, double TOL, int inner_iter, int outer_iter, const std::vector<int> &nxs,
                         const std::vector<int> &nys, ofx_stats *stats_out)
{
    const BroxParams P = {alpha, gamma, TOL, inner_iter, outer_iter, 0};
    return ofx_group_records(ctx, G, stats_out, [&](ofx_stats *st) {
        return ctx->precision == OFX_F64 ? broxt_devapi<double>(ctx, G, frames, dF, d_flo, P, nscales, nu, nxs, nys, st)
                                         : broxt_devapi<float>(ctx, G, frames, dF, d_flo, P, nscales, nu, nxs, nys, st);
    });
}

// ofx_brox_temporal on a device-resident sequence (include/ofx.h)
extern "C" int ofx_brox_temporal_dev(ofx_ctx *ctx, int frames, const void *const *dF, void *const *d_flo, int nxx, int nyy,
                                     double alpha, double gamma, int nscales, double nu, double TOL, int inner_iter, int outer_iter)
{
    OFX_ENTER(ctx);
    std::vector<int> nxs, nys;
    OFX_TRY(broxt_dev_check(ctx, 1, frames, dF, d_flo, nxx, nyy, nscales, nu, inner_iter, outer_iter, nxs, nys));
    return broxt_dev_run(ctx, 1, frames, dF, d_flo, alpha, gamma, nscales, nu, TOL, inner_iter, outer_iter, nxs, nys, &ctx->stats);
}

// what a group adds to broxt_dev_check: its size, and the index range over all its sequences
static int broxt_group_check(ofx_ctx *ctx, int n_seq, int frames, const void *const *dF, void *const *d_flo, int nxx, int nyy,
                             int nscales, double nu, int inner_iter, int outer_iter, std::vector<int> &nxs, std::vector<int> &nys)
{
    if (n_seq < 1 || n_seq > OFX_MAX_GROUP)
        return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: a lockstep group holds 1..%d sequences (got %d)", OFX_MAX_GROUP, n_seq);
    OFX_TRY(broxt_dev_check(ctx, n_seq, frames, dF, d_flo, nxx, nyy, nscales, nu, inner_iter, outer_iter, nxs, nys));
    if ((long long) nxx * nyy * frames * n_seq >= (1LL << 31))
        return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal: group of %d sequences larger than 2^31 voxels", n_seq);
    return OFX_OK;
}

// n_seq sequences through the same launches, each with its own normalisation, stopping test and snapshots (include/ofx.h)
extern "C" int ofx_brox_temporal_group_dev(ofx_ctx *ctx, int n_seq, int frames, const void *const *dF, void *const *d_flo, int nxx,
                                           int nyy, double alpha, double gamma, int nscales, double nu, double TOL, int inner_iter,
                                           int outer_iter, ofx_stats *stats_out)
{
    OFX_ENTER(ctx);
    std::vector<int> nxs, nys;
    OFX_TRY(broxt_group_check(ctx, n_seq, frames, dF, d_flo, nxx, nyy, nscales, nu, inner_iter, outer_iter, nxs, nys));
    return broxt_dev_run(ctx, n_seq, frames, dF, d_flo, alpha, gamma, nscales, nu, TOL, inner_iter, outer_iter, nxs, nys, stats_out);
}

// n_seq independent sequences over the contexts (include/ofx.h).  Option "lockstep" of ctxs[0] = 0 or 1: sequence q alone on
// context q mod (contexts at work), each context under its own options.  L >= 2: lockstep groups of L consecutive sequences
// (ofx_brox_temporal_group_dev), group q on context q mod (contexts at work), every context under ctxs[0]'s sor_exact / sor_fuse
// -- also when the memory rule or n_seq leaves groups of one.
extern "C" int ofx_brox_temporal_batch_dev(ofx_ctx *const *ctxs, int n_ctx, int n_seq, int frames, const void *const *dF,
                                           void *const *d_flo, int nxx, int nyy, double alpha, double gamma, int nscales, double nu,
                                           double TOL, int inner_iter, int outer_iter, double *work_pix_iters)
{
    if (!ctxs || n_ctx < 1 || !ctxs[0]) return OFX_ERR_ARG;
    ofx_ctx *ctx = ctxs[0];
    OFX_ENTER(ctx);
    if (ofx_batch_check_ctxs(ctxs, n_ctx, OFX_SAME_DEVICE | OFX_SAME_FORMAT) != OFX_OK)
        return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal batch: a context is NULL, on another device, of another precision, \"input\" or \"input_pitch\"");
    if (n_seq < 1) return ofx_fail(ctx, OFX_ERR_ARG, "brox temporal batch: %d sequences", n_seq);
    std::vector<int> nxs, nys;
    OFX_TRY(broxt_dev_check(ctx, n_seq, frames, dF, d_flo, nxx, nyy, nscales, nu, inner_iter, outer_iter, nxs, nys));
    int L = ctx->lockstep < 2 ? 1 : (ctx->lockstep > OFX_MAX_GROUP ? OFX_MAX_GROUP : ctx->lockstep);
    if (L > n_seq) L = n_seq;
    while (L > 1 && (long long) nxx * nyy * frames * L >= (1LL << 31)) L--;
    int n_use = 1;
    {
        double budget;                                           // of the whole batch: this entry fits groups x contexts into it
        OFX_TRY(ofx_batch_budget(ctx, 1, &budget));
        const double el = ctx->precision == OFX_F64 ? 8.0 : 4.0, B = ctx->sor_batch > 0 ? ctx->sor_batch : 64;
        double level_px = 0.0;
        for (int s = 0; s < nscales; s++) level_px += (double) nxs[s] * nys[s];
        const double per = 1.05 * el * (level_px * (frames + (27.0 + 2.0 * B) * (frames - 1)) + 2.0 * frames * (double) nxx * nyy);
        const double fit = budget / per;                         // sequences that fit: the per-sequence rule times the group size
        if (fit < 1.0)
            return ofx_fail(ctx, OFX_ERR_NOMEM, "brox temporal batch: %.3f GB for one sequence, %.3f GB available", per / 1e9, budget / 1e9);
        const int n_groups = (n_seq + L - 1) / L;
        n_use = n_ctx < n_groups ? n_ctx : n_groups;
        while (L > 1 && fit < (double) n_use * L) {              // the group size first ...
            L--;
            const int ng = (n_seq + L - 1) / L;
            n_use = n_ctx < ng ? n_ctx : ng;
        }
        if (fit < n_use) n_use = (int) fit;                      // ... then the contexts
    }
    if (ctx->lockstep < 2)
        return ofx_run_groups(ctxs, n_use, n_seq, 1, 1, work_pix_iters, true, [&](ofx_ctx *c, int q, int, ofx_stats *st) {
            OFX_ENTER(c);
            return broxt_dev_run(c, 1, frames, dF + (size_t) q * frames, d_flo + (size_t) q * (frames - 1), alpha, gamma, nscales, nu, TOL,
                                 inner_iter, outer_iter, nxs, nys, st);
        });
    const int exact = ctx->sor_exact, fuse = ctx->sor_fuse;
    return ofx_run_groups(ctxs, n_use, n_seq, L, 1, work_pix_iters, true, [&](ofx_ctx *c, int first, int cnt, ofx_stats *st) {
        OFX_ENTER(c);
        const int exact_c = c->sor_exact, fuse_c = c->sor_fuse;
        c->sor_exact = exact;
        c->sor_fuse = fuse;
        const int s = broxt_dev_run(c, cnt, frames, dF + (size_t) first * frames, d_flo + (size_t) first * (frames - 1), alpha, gamma,
                                    nscales, nu, TOL, inner_iter, outer_iter, nxs, nys, st);
        c->sor_exact = exact_c;
        c->sor_fuse = fuse_c;
        return s;
    });
}


// ============================================================================================
// Classic Horn-Schunck: src/horn_schunck_classic.cpp -- n Jacobi iterations from a zero flow
// ============================================================================================
// Jacobi, so exactly parallel: one launch per iteration on ping-pong (u, v) pairs.  Per pixel and iteration:
// read (Ex, Ey) + Et (3 T) and the 3x3 neighbourhood of (u, v) (2 T compulsory), write (u, v) (2 T) = 7 T = 56 B
// in f64 -- HBM-bound.  Sample p(x, i, j) = column i, row j with clamped indices (:22-43).
template <typename T> OFX_DEV double hsc_p(const T *x, int w, int h, int i, int j)
{
    i = i < 0 ? 0 : (i >= w ? w - 1 : i);
    j = j < 0 ? 0 : (j >= h ? h - 1 : j);
    return ldw(x + (size_t) j * w + i);
}

// compute_input_derivatives, :46-73 (every sum in the reference's left-to-right order)
template <typename T>
__global__ void k_hsc_derivs(const T *__restrict__ a, const T *__restrict__ b, typename Pix<T>::v2 *__restrict__ E,
                             T *__restrict__ Et, int w, int h)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    if (i >= w || j >= h) return;
    const double a00 = hsc_p(a, w, h, i, j), a10 = hsc_p(a, w, h, i + 1, j), a01 = hsc_p(a, w, h, i, j + 1),
                 a11 = hsc_p(a, w, h, i + 1, j + 1);
    const double b00 = hsc_p(b, w, h, i, j), b10 = hsc_p(b, w, h, i + 1, j), b01 = hsc_p(b, w, h, i, j + 1),
                 b11 = hsc_p(b, w, h, i + 1, j + 1);
    const double ey = (1.0 / 4) * (a01 - a00 + a11 - a10 + b01 - b00 + b11 - b10);
    const double ex = (1.0 / 4) * (a10 - a00 + a11 - a01 + b10 - b00 + b11 - b01);
    const double et = (1.0 / 4) * (b00 - a00 + b10 - a10 + b01 - a01 + b11 - a11);
    const size_t p = (size_t) j * w + i;
    stn2(E + p, make_double2(ex, ey));
    stn(Et + p, et);
}

// compute_bar + hs_iteration, :76-122
template <typename T>
__global__ __launch_bounds__(256) void k_hsc_iter(const typename Pix<T>::v2 *__restrict__ Uin,
                                                  typename Pix<T>::v2 *__restrict__ Uout,
                                                  const typename Pix<T>::v2 *__restrict__ E, const T *__restrict__ Et, int w,
                                                  int h, double alpha)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    if (i >= w || j >= h) return;
    const int il = i > 0 ? i - 1 : 0, ir = i < w - 1 ? i + 1 : w - 1;
    const unsigned rc = (unsigned) j * w, ru = (unsigned) (j > 0 ? j - 1 : 0) * w, rd = (unsigned) (j < h - 1 ? j + 1 : h - 1) * w;
    const double2 l = ldw2(Uin + rc + il), r = ldw2(Uin + rc + ir), t = ldw2(Uin + ru + i), d = ldw2(Uin + rd + i);
    const double2 tl = ldw2(Uin + ru + il), tr = ldw2(Uin + ru + ir), dl = ldw2(Uin + rd + il), dr = ldw2(Uin + rd + ir);
    const double ubar = (1.0 / 6) * (l.x + r.x + t.x + d.x) + (1.0 / 12) * (tl.x + tr.x + dl.x + dr.x);
    const double vbar = (1.0 / 6) * (l.y + r.y + t.y + d.y) + (1.0 / 12) * (tl.y + tr.y + dl.y + dr.y);
    const double2 e = ldw2(E + rc + i);
    const double et = ldw(Et + rc + i);
    double tt = e.x * ubar + e.y * vbar + et;
    tt /= alpha * alpha + e.x * e.x + e.y * e.y;
    stn2(Uout + rc + i, make_double2(rnd_to<T>(ubar - e.x * tt), rnd_to<T>(vbar - e.y * tt)));
}

template <typename T>
static int hs_classic_host(ofx_ctx *ctx, const double *a, const double *b, double *u, double *v, int w, int h, int niter,
                           double alpha)
{
    const size_t n = (size_t) w * h;
    T *da, *db, *Et;
    typename Pix<T>::v2 *U[2], *E;
    OFX_TRY(upload_plane<T>(ctx, a, n, &da));
    OFX_TRY(upload_plane<T>(ctx, b, n, &db));
    OFX_TRY(ofx_alloc(ctx, n, &U[0]));
    OFX_TRY(ofx_alloc(ctx, n, &U[1]));
    OFX_TRY(ofx_alloc(ctx, n, &E));
    OFX_TRY(ofx_alloc(ctx, n, &Et));
    hipLaunchKernelGGL(k_hsc_derivs<T>, g2d(w, h), b2d(), 0, ctx->stream, (const T *) da, (const T *) db, E, Et, w, h);
    OFX_LAUNCH_CHECK(ctx);
    OFX_TRY(op_fill2<T>(ctx, U[0], n));                                                            // :139-141
    int cur = 0;
    for (int it = 0; it < niter; it++) {                                                           // :142-144
        hipLaunchKernelGGL(k_hsc_iter<T>, g2d(w, h), b2d(), 0, ctx->stream, U[cur], U[cur ^ 1], E, (const T *) Et, w, h,
                           alpha);
        cur ^= 1;
    }
    OFX_LAUNCH_CHECK(ctx);
    ofx_stats_begin(&ctx->stats, 1, 1);
    ctx->stats.nx[0] = w;
    ctx->stats.ny[0] = h;
    ctx->stats.iters[0][0] = niter;
    ctx->stats.work_pix_iters = (double) niter * n;
    return download_flow<T>(ctx, U[cur], u, v, n);
}

extern "C" int ofx_hs_classic(ofx_ctx *ctx, const double *a, const double *b, double *u, double *v, int w, int h, int niter,
                              double alpha)
{
    OFX_ENTER(ctx);
    if (!a || !b || !u || !v) return ofx_fail(ctx, OFX_ERR_ARG, "hs_classic: NULL pointer");
    if (w < 1 || h < 1 || (long long) w * h >= (1LL << 28)) return ofx_fail(ctx, OFX_ERR_ARG, "hs_classic: bad size %dx%d", w, h);
    if (niter < 0) niter = 0;                                   // the reference's loop simply does not run
    const double t0 = ofx_now_ms();
    int s = ctx->precision == OFX_F64 ? hs_classic_host<double>(ctx, a, b, u, v, w, h, niter, alpha)
                                      : hs_classic_host<float>(ctx, a, b, u, v, w, h, niter, alpha);
    ctx->stats.total_ms = ofx_now_ms() - t0;
    return s;
}
