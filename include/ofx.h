/* include/ofx.h -- C ABI of libofx.so: the MI355X (gfx950) implementation of the variational
 * optical-flow hot path of 12334zq/optical-flow-1 (TV-L1 primal-dual solver + the shared stencil /
 * warp / pyramid operators; Horn-Schunck-pyramidal and Brox-spatial SOR solvers on top of them).
 *
 * The reference has no FFI / plugin layer: its boundary is the C++ library libof.a (mangled names,
 * `bool` and default arguments) called by its command-line programs.  Every entry
 * point below replaces one reference prototype 1:1 -- same argument order and meaning, with
 *   - a leading `ofx_ctx *` (one context = one GPU + one HIP stream + its workspace),
 *   - `bool` -> `int`,
 *   - an `int` status return instead of `void` + C++ exceptions (0 = OFX_OK).
 * Host-pointer entry points take/return dense row-major `double` arrays (the reference's ofpix_t,
 * src/of.h:4-10), index p = i*nx + j; device residency is internal.  The *_dev entry points take
 * device pointers (hipMalloc / torch tensors) and run on the context's stream.
 *
 * There is NO CPU fallback: without a usable gfx950 device ofx_ctx_create fails with
 * OFX_ERR_NODEV and every other call needs a context.
 *
 * Thread-safety: calls on different contexts are independent; one context must not be used from
 * two threads at once.  Calls are blocking (they return after the result is in the caller's
 * buffer), except where noted for *_dev.
 */
#ifndef OFX_H
#define OFX_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFX_VERSION 102

/* status codes */
#define OFX_OK          0
#define OFX_ERR_ARG     1   /* bad size / NULL pointer / parameter out of range                  */
#define OFX_ERR_SIGMA   2   /* replaces std::runtime_error("GaussianSmooth: sigma too large"),
                               src/operators.cpp:520-522 (also returned where the reference would
                               read out of bounds: kernel radius >= image width or height)       */
#define OFX_ERR_NOMEM   3   /* replaces std::bad_alloc (device or host allocation failed)         */
#define OFX_ERR_HIP     4   /* a HIP runtime call or kernel launch failed                        */
#define OFX_ERR_NODEV   5   /* no gfx950 device / device index out of range                      */

/* storage precision of the device-resident arrays; arithmetic is ALWAYS double in registers.   */
#define OFX_F64 0           /* strict mode: double storage, per-pixel arithmetic bit-identical to
                               the reference (glibc-exact hypot, IEEE divisions, no FMA contraction) */
#define OFX_F32 1           /* fast mode: float storage (half the HBM traffic) and, in the TV-L1
                               dual update, hypot = sqrt(x*x+y*y) and one reciprocal per denominator;
                               AEPE vs the double reference ~1e-5, not bit-compatible             */

/* solver limits mirrored from the reference's #defines */
#define OFX_TVL1_MAX_ITERATIONS 300   /* src/tvl1flow.cpp:22  */
#define OFX_BROX_MAX_ITERATIONS 300   /* src/brox_optic_flow_spatial.cpp:24 */
#define OFX_HS_MAX_MAXITER 65536      /* largest Horn-Schunck `maxiter` accepted (reference: unbounded) */
#define OFX_MAX_SCALES 32             /* pyramid levels ofx_stats RECORDS; the solvers accept any number of levels
                                         (e.g. tvl1flow with zfactor = 0.9 at 1080p uses 47), levels >= 32 are solved
                                         but not itemised in the record (work_pix_iters still counts them)       */
#define OFX_MAX_SOLVES 64             /* warps (TV-L1, HS) or outer*inner solves (Brox) per scale */

typedef struct ofx_ctx ofx_ctx;

/* Work / timing record of the last solver call on a context (the reference only prints these on
 * stderr when `verbose`: src/tvl1flow.cpp:184-188,284-286). */
typedef struct ofx_stats {
    int    nscales;                                   /* pyramid levels actually used            */
    int    nsolves;                                   /* warps per scale (Brox: outer*inner)     */
    int    nx[OFX_MAX_SCALES], ny[OFX_MAX_SCALES];    /* level sizes, 0 = finest                 */
    int    iters[OFX_MAX_SCALES][OFX_MAX_SOLVES];     /* inner iterations / SOR sweeps per solve */
    double error[OFX_MAX_SCALES][OFX_MAX_SOLVES];     /* stopping-criterion value at exit        */
    double iter_ms[OFX_MAX_SCALES];                   /* HIP-event time of the inner-iteration
                                                         launches of a level (0 unless profiling) */
    long long iter_launches[OFX_MAX_SCALES];          /* iteration kernels that did real work    */
    double work_pix_iters;                            /* sum n_iter * nx_s * ny_s                */
    double total_ms;                                  /* wall time of the call on the host       */
    int    odd_stops;                                 /* TV-L1: loops that stopped on the first iteration of a
                                                         fused pair ...                                        */
    int    odd_stops_stored;                          /* ... of which the launch had stored its intermediate
                                                         state (option "store_a"): no recomputation needed     */
    int    fused[OFX_MAX_SCALES];                     /* TV-L1: iterations per iteration launch at each level
                                                         (1, 2, 3, or the tile kernel's 4 | 6); odd_stops then
                                                         counts the loops that ended inside such a launch unit  */
    double pyramid_ms;                                /* ofx_robust_expo, _pyramid: HIP-event time from the upload of the
                                                         images to the last level of both pyramids (0 unless profiling) */
} ofx_stats;

/* ---- context ---------------------------------------------------------------------------------*/
int  ofx_device_count(void);                                   /* number of usable HIP devices    */
int  ofx_ctx_create(ofx_ctx **out, int device, int precision); /* precision: OFX_F64 | OFX_F32   */
void ofx_ctx_destroy(ofx_ctx *ctx);
const char *ofx_strerror(int status);
const char *ofx_last_error(const ofx_ctx *ctx);                /* detail text of the last failure */
void *ofx_ctx_stream(const ofx_ctx *ctx);                      /* the context's hipStream_t       */
int   ofx_ctx_precision(const ofx_ctx *ctx);
int   ofx_ctx_synchronize(ofx_ctx *ctx);
int   ofx_set_option(ofx_ctx *ctx, const char *name, double value);
/* options (value 0 = default / automatic unless noted):
 *   "profile"        0/1  bracket the inner-iteration launches with HIP events -> stats.iter_ms (and the pyramid phase of
 *                         ofx_robust_expo / _pyramid / _group_dev -> stats.pyramid_ms; _group_dev: iter_ms on the host's clock)
 *   "fixed_work"     0/1  TV-L1: every warp runs exactly OFX_TVL1_MAX_ITERATIONS iterations (stopping
 *                         test disabled; the reference with epsilon = 0)
 *   "sor_exact"      HS / Brox: 1 (default) = the reference's sweep order, bit-identical results, K time steps
 *                         of the pipelined schedule per launch; 2 = the same schedule, one launch per time step;
 *                         0 = the TOLERANCE mode, re-ordered sweeps inside north_star's bar (AEPE < 1e-4 against the reference
 *                         on the BASELINE configs; csrc/ofx_sor_tile.hip): Horn-Schunck four-colour sweeps, K per launch on LDS
 *                         tiles (AEPE 9e-6 at config 3); Brox a checkerboard of 64 x 128-pixel tiles swept in the reference's
 *                         order inside a tile on the finest level and red-black sweeps below (AEPE 1.1e-5 at config 4; red-black
 *                         everywhere: 1.3e-4).  Lone solves 5-10x faster than exact, lockstep groups supported.  On inputs where
 *                         the solves run into maxiter unconverged (the discontinuous pair P1 at 1080p) ANY re-ordering moves the
 *                         flow by as much as the reference's own OpenMP threads do (AEPE 2.5e-2) -- use the exact mode there.
 *                         Temporal Brox (all three entries), 0: 3-D red-black sweeps over the frames - 1 flow fields of a level,
 *                         every voxel with (row + column + field) even, then every voxel with it odd; the update, omega and the
 *                         stopping test are the reference's.  AEPE 6.7e-6 against the reference's order on 640x480 x 5 frames
 *                         (2086 sweeps against 2123), lone solve 7.7x faster than exact
 *                         (profiles/r11_brox_temporal_tolerance_640x480.json).  1 and 2 both run the windowed exact schedule.
 *   "sor_fuse"      sor_exact = 0: sweeps per launch of the tile kernels, K = 1..4 (0 = default: Horn-Schunck 2 in lockstep groups of >= 4 pairs, else 4; Brox's red-black
 *                         levels 4); 9 = Brox's red-black levels through k_brox_sor, two launches per sweep (A/B); -1 = the round-1
 *                         kernels, one launch per colour and sweep (single pairs only; Brox: red-black on every level).  Results
 *                         do not depend on K.  Temporal Brox: K = 1, 2, 4 (3 = 2; 0 = default: 2) sweeps per launch on LDS tiles
 *                         that hold every flow field, for sequences of up to 5 frames (4 flow fields); 9 or -1, and every value
 *                         for longer sequences: one launch per colour and sweep from global memory.  The order alone decides
 *                         the result: the same bits for every value.
 *   "sor_tile"      sor_exact = 0, Horn-Schunck: tile geometry 1 = 128 x 32 pixels on 16 waves, 2 = on 8 waves (default),
 *                         3 = 128 x 48 on 12 waves.  Results do not depend on it.
 *   "sor_wave_levels"  sor_exact = 0, Brox: pyramid levels 0 .. n - 1 use the checkerboard-of-tiles sweeps (default 1: the
 *                         finest), the coarser ones red-black.  PART OF THE RESULT (as is "sor_tile_w").
 *   "sor_tile_w"     ... columns per tile, 1..128 (default 128); "sor_wave_p": anti-diagonals of operand prefetch, 2 | 4 | 6 | 8
 *                         (default 4; results do not depend on it)
 *   "sor_batch"      sweeps in flight per batch in the exact modes (default 32 / 64)
 *   "sor_window"     time steps per launch of sor_exact = 1 (default 8; 4 for Brox in lockstep groups of >= 4 pairs)
 *   "sor_rows"       rows per workgroup (row block of a sweep) of sor_exact = 1 (default 64; 125 in lockstep groups
 *                         of >= 4 pairs)
 *   "sor_spw"        consecutive sweeps of a row block that share a workgroup in sor_exact = 1 (1, 2 or 4; default 0 = 1,
 *                         the fastest measured; results do not depend on it)
 *   "fuse2"          1/0  TV-L1: two iterations per kernel launch (default 1)
 *   "fuse3", "fuse3_min_px"  TV-L1: three iterations per launch (k_tvl1_iter3): 0 never, 1 on every level of at least
 *                         fuse3_min_px pixels x pairs, 2 (default) by measurement: not in strict mode, only for lockstep groups
 *                         or contexts sharing the device, levels of >= 500 000 pixels x pairs.  Results do not depend on it.
 *   "fuse4", "fuse4_min_px"  TV-L1: four iterations per launch (k_tvl1_iter4): 0 never, 1 on every level of at least
 *                         fuse4_min_px pixels x pairs, 2 (default) by measurement: where "fuse3" = 2 takes three and the level
 *                         has at least 2 000 000 pixels x pairs (fuse4_min_px > 0 replaces that figure).  Results do not depend
 *                         on it.  "fuse4_afac3": error / threshold ratio below which a unit of that kernel runs three
 *                         iterations ("fuse3_afac2" / "fuse3_afac1": two / one); 0 (default) = never three.
 *   "store_a"        TV-L1, fused pairs: a loop that stops on the first iteration of a pair needs the state between the
 *                         two iterations; 1 (default) = a launch also stores it when the previous error is within 1.5x
 *                         of the threshold (the host then just switches buffers), 0 = never (the iteration is
 *                         recomputed alone), 2 = always.  Results are bit-identical in all three settings.
 *   "nt_stores"      fused TV-L1 kernel: 0 (default) non-temporal stores when a launch's working set exceeds the Infinity
 *                    Cache, 1 always, 2 never (A/B measurements)
 *   "relaxed_dual"   0/1  TV-L1 in OFX_F64 storage: 1 = the tolerance mode -- double storage and arithmetic, but sqrt(x^2 + y^2)
 *                         for libm's hypot and reciprocals for the IEEE quotients of the dual update (one refinement step on
 *                         v_rsq_f64 / v_rcp_f64: relative error ~2^-45); NOT bit-identical: AEPE vs the reference ~1e-12 px on
 *                         the BASELINE configs (bar 1e-4), iteration tables equal there, 25-40 % faster than strict.
 *                         0 (default) = strict.  The front-ends read OFX_TOLERANCE=1 for it.
 *   "tile", "tile_max_px"  TV-L1: levels of at most tile_max_px pixels x pairs (default 200 000) run K = 4 | 6 iterations per
 *                         launch on 2-D tiles instead of the marching strips (0 = off, the default: measured no faster)
 *   "sor_lds"        windowed exact SOR sweeps: 0 = one global round trip per time step, 2 = the launch window staged in LDS,
 *                         1 (default) = by measurement (LDS for lone Horn-Schunck solves).  Results do not depend on it.
 *   "rof_pipe"       1/0  TV-L1 with occlusions / Scalar_ROF_BoxCellCentered: all iterations of a call in flight, the sweep
 *                         of iteration s 120 positions behind the sweep of s - 1 (default 1); 0 = one iteration at a time
 *   "rof_window"     steps per launch of the ROF box sweeps: 10 (default) or 24 (the round-2 geometry, 143 KB of LDS per workgroup)
 *   "chi_fuse"       1/0  Solver_wrt_chi: 5 iterations per launch on overlapping LDS tiles (default 1); 0 = two launches per
 *                         iteration.  Results do not depend on either.
 *   "gauss_fused"    pyramids of lockstep groups: 1 (default) row + column pass of the Gaussian in one launch, and for zfactor = 1/2
 *                         the whole zoom_out (smoothing + 2:1 sampling) in one; 3 = without the zoom_out fusion, 2 = the
 *                         generic-radius fused kernel, 0 = two passes.  Results do not depend on it.
 *   "spin_us"        microseconds the host spins on a convergence poll's pinned record before it sleeps in
 *                         hipEventSynchronize (default 150; 0 = never)
 *   "warp_lds"       1/0  TV-L1 warp with the bicubic taps staged through LDS (default 1)
 *   "apply_lds"      ofx_flow_warp_dev / ofx_flow_interpolate_dev: 1 = the bicubic taps staged through LDS (a workgroup whose taps
 *                         do not fit its tile gathers from global memory), 0 = gathered from global memory alone, 2 (default) = by
 *                         measurement: 1 for float and double frames, 0 for 8- and 16-bit frames.  Any other value is OFX_ERR_ARG.
 *                         Results do not depend on it.
 *   "tvl1_median"    TV-L1 (every entry but the solvers with occlusions, which have the reference's own median): 3 | 5 = after the
 *                         inner loop of EVERY warp at EVERY level, u1 and u2 of every pair become their 3x3 | 5x5 median (Wedel et
 *                         al. 2009, section 3.2; "Median of a flow" below, without a map), the last warp included, so the flow that
 *                         zoom_in takes up and the final payload are filtered; the dual variables stay as they are.  0 (default) =
 *                         off: not one launch more.  Any other value is OFX_ERR_ARG and leaves the option as it was.  Iteration
 *                         tables and ofx_stats keep their meaning.  The front-ends read OFX_TVL1_MEDIAN=3|5 for it.
 *   "st_fuse"        ofx_structure_texture_dev: iterations per kernel launch on LDS tiles with a halo of that many pixels: 0 (default) =
 *                         chosen by measurement, 1 .. OFX_ST_MAX_FUSE = that many (1 = one launch per iteration, the A/B
 *                         baseline).  Any other value is OFX_ERR_ARG.  Results do not depend on it.
 *   "lockstep"       pairs per lockstep group in ofx_tvl1_batch_dev (default 0 = ofx_tvl1_batch_group_size's
 *                         rule: as large as possible, evened out over the contexts; at most 16)
 *   "mem_budget"     bytes the level arrays of all contexts of a batch may occupy when the group size is chosen
 *                         (default 0 = half of the device memory that is free at the time of the call)
 *   "concurrency"    number of contexts that will be solving on the same device at the same time
 *                         (default 1); a scheduling hint for the strip height of the TV-L1 kernels
 *   "rows_per_wave", "rows_per_wave2", "chunk"   tuning of the TV-L1 kernels / launch batching
 *   "input"          element type of the FRAMES that the *_dev entries read (OFX_IN_* below; default OFX_IN_STORAGE); any other
 *                         value is OFX_ERR_ARG
 *   "input_pitch"    bytes from the start of one row of a FRAME that the *_dev entries read to the start of the next (default 0 =
 *                         dense: the rows lie back to back).  One pitch per call, for all its frames; see option "input" below.  A
 *                         negative, fractional or >= 2^31 value is OFX_ERR_ARG and leaves the option as it was.
 *   "input_vec"      1/0  the byte kinds of "input" through the kernels that load a run of four elements per lane as aligned
 *                         32-bit words (default 1); 0 = one element per thread (A/B).  Results do not depend on it.
 *   "input_lut"      1/0  ... and the 8-bit kinds take 255 (x - min) / (max - min) from a per-workgroup table of its 256 possible
 *                         values (default 1); 0 = one division per element (A/B).  The same expression on the same operands:
 *                         results do not depend on it. */
int   ofx_get_stats(const ofx_ctx *ctx, ofx_stats *out);

/* Option "input": what a frame pointer of a *_dev entry points at.  The entries that take frames as device pointers --
 * ofx_tvl1_multiscale_dev / _group_dev / _batch_dev, ofx_tvl1_group_init_dev / ofx_tvl1_batch_init_dev / ofx_tvl1_sequence_group_dev,
 * ofx_tvl1_bidir_group_dev / _bidir_batch_dev, ofx_hs_group_dev / _batch_dev, ofx_brox_group_dev / _batch_dev,
 * ofx_hs_group_init_dev / ofx_hs_batch_init_dev / ofx_hs_sequence_group_dev, ofx_brox_group_init_dev / ofx_brox_batch_init_dev /
 * ofx_brox_sequence_group_dev,
 * ofx_robust_expo_group_dev / _batch_dev, ofx_brox_temporal_dev / _group_dev / _batch_dev, ofx_tvl1occ_sequence_group_dev /
 * _sequence_dev / _triples_group_dev / _triples_dev, ofx_normalize_frames_dev / ofx_normalize_frames2d_dev, ofx_pyramid_group_dev and
 * ofx_flow_warp_dev / ofx_flow_interpolate_dev (which also WRITE that kind, and refuse OFX_IN_RGB8) and
 * ofx_structure_texture_dev -- read
 * elements of this kind wherever their
 * comments say "the context's storage precision"; a frame is aligned to its element (OFX_IN_RGB8: to a byte).  Every sample
 * converts exactly to double, so payloads, occlusion maps and iteration / sweep tables are BIT-IDENTICAL to the same call under
 * OFX_IN_STORAGE on planes that hold the same values (stopping values too, up to the order in which the pair solvers' atomics add
 * them, which no two runs of one call share).  Entries that take host planes ignore the option; entries
 * that take several contexts want the same value on all of them (OFX_ERR_ARG otherwise, before any work).
 * Option "input_pitch": the row pitch of those frames, for the same entries and every kind, OFX_IN_STORAGE included.  A frame
 * is ny rows of nx * nz elements (OFX_IN_RGB8: of nx pixels of three bytes; the interleaved colour images of
 * ofx_robust_expo_group_dev / _batch_dev: of nxx * nzz elements); 0, the default, means dense -- element (or pixel) e of a frame
 * at e times the element size -- and otherwise row i starts pitch * i bytes after the frame pointer, as in a decoder's surface,
 * a crop of a larger image or a torch slice video[:, y0:y1, x0:x1].  A region of interest needs nothing else: pass the address of
 * its first element and its parent's pitch.  No byte outside the rows is read, neither the padding between them nor any after
 * the last row's end, and the results are BIT-IDENTICAL to the same call on dense copies of the rows.  A pitch equal to the row's
 * bytes is the dense layout.  A non-zero pitch below the row's bytes, or not a multiple of the element's alignment (8 for double, 4
 * for float, 2 for OFX_IN_U16, 1 for OFX_IN_U8 and OFX_IN_RGB8), is OFX_ERR_ARG before any work, nothing written (ofx_last_error
 * names the pitch and the row's bytes); the frame pointer stays aligned to its element.  One pitch serves all frames of a call;
 * host-plane entries ignore it, entries that take several contexts want the same value on all of them, and
 * ofx_normalize_frames_dev, which has no row length, is OFX_ERR_ARG while it is non-zero (ofx_normalize_frames2d_dev takes
 * one).  ofx_tvl1_batch_dev stages a frame that is not on its context's device as it lies, (ny - 1) * pitch + the row's bytes.
 * Payloads and maps are written dense; a pitched frame has fewer than 2^31 - 1024 rows.
 * ofx_robust_expo_group_dev / _batch_dev with nzz > 1 keep their channels interleaved (an HWC uint8 image is that layout as it
 * stands); OFX_IN_RGB8 there is OFX_ERR_ARG unless nzz == 1. */
#define OFX_IN_STORAGE 0   /* the context's storage precision (double | float): the default                                    */
#define OFX_IN_U8      1   /* one byte per element                                                                             */
#define OFX_IN_U16     2   /* one host-order uint16_t per element                                                              */
#define OFX_IN_F32     3   /* float elements whatever the storage precision                                                    */
#define OFX_IN_RGB8    4   /* three interleaved bytes per pixel, collapsed to ONE gray sample while loading by the front-ends'
                              8-bit rule (uint8_t) (.299 R + .587 G + .114 B): the three products and the two sums each rounded
                              to double, left to right, no contraction, the result truncated                                   */

/* ---- operators (replace src/operators.h:29-134) ---------------------------------------------*/
int ofx_divergence(ofx_ctx *ctx, const double *v1, const double *v2, double *div, int nx, int ny);
int ofx_forward_gradient(ofx_ctx *ctx, const double *f, double *fx, double *fy, int nx, int ny);
int ofx_centered_gradient(ofx_ctx *ctx, const double *f, double *dx, double *dy, int nx, int ny);  /* nz = 1 */
int ofx_dxx(ofx_ctx *ctx, const double *I, double *Ixx, int nx, int ny);                         /* nz = 1 */
int ofx_dyy(ofx_ctx *ctx, const double *I, double *Iyy, int nx, int ny);
int ofx_dxy(ofx_ctx *ctx, const double *I, double *Ixy, int nx, int ny);
/* in-place separable Gaussian with the reference's default arguments (reflecting boundary,
 * window 5): src/operators.cpp:506-624 */
int ofx_gaussian(ofx_ctx *ctx, double *I, int nx, int ny, double sigma);

/* centered_gradient3 (src/operators.h:107-114): f holds nz frames of nx*ny; dx, dy per frame, dz between frames */
int ofx_centered_gradient3(ofx_ctx *ctx, const double *f, double *dx, double *dy, double *dz, int nx, int ny, int nz);

/* ---- bicubic interpolation (replace src/bicubic_interpolation.h:16-52) -----------------------*/
/* n samples at (uu[k], vv[k]) -> out[k]; one call of the reference's bicubic_interpolation_at
 * per sample */
int ofx_bicubic_at(ofx_ctx *ctx, const double *input, const double *uu, const double *vv, double *out,
                   int n, int nx, int ny, int border_out);
int ofx_bicubic_warp(ofx_ctx *ctx, const double *input, const double *u, const double *v, double *output,
                     int nx, int ny, int border_out);
/* bicubic_interpolation_at_color (src/bicubic_interpolation.h:30-43): channel k of nz interleaved channels */
int ofx_bicubic_at_color(ofx_ctx *ctx, const double *input, const double *uu, const double *vv, double *out,
                         int n, int nx, int ny, int nz, int k, int border_out);

/* ---- pyramid zoom (replace src/zoom.h:20-63) -------------------------------------------------*/
void ofx_zoom_size(int nx, int ny, int *nxx, int *nyy, double factor);      /* pure host arithmetic */
int  ofx_zoom_out(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, double factor);
int  ofx_zoom_in(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, int nxx, int nyy);
/* zoom_out_color (src/zoom.h:44-55).  The reference is only defined for nz = 1 (for nz > 1 it reads beyond its
 * nx*ny scratch copy, src/zoom.cpp:96-118); nz = 1 is zoom_out, any other nz is OFX_ERR_ARG. */
int  ofx_zoom_out_color(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, int nz, double factor);
/* zoom_out of nz interleaved channels as the IPOL ORIGINAL of robust_expo_methods defines it
 * (3rdparty/ipoldfmethods_20160307/zoom.h:45-85 with gaussian.h:23-168): all nx*ny*nz elements are smoothed, one separable
 * reflecting Gaussian per channel, and every channel is sampled with the same bicubic -- channel k of the result is
 * ofx_zoom_out of channel k, nz = 1 is ofx_zoom_out bit for bit.  This is NOT a reference prototype: ofx_zoom_out_color above
 * keeps the reference's name and keeps refusing nz > 1, where the reference is undefined.
 * I: element (i * nx + j) * nz + k; Iout: nxx * nyy * nz with (nxx, nyy) from ofx_zoom_size.  nz in 1 .. OFX_REXPO_MAX_CHANNELS
 * (OFX_ERR_ARG otherwise); OFX_ERR_SIGMA under ofx_zoom_out's rule (kernel radius >= width or height). */
int  ofx_zoom_out_channels(ofx_ctx *ctx, const double *I, double *Iout, int nx, int ny, int nz, double factor);

/* ---- normalisation (replace src/utils.h:27-32) -----------------------------------------------*/
int ofx_image_normalization_2(ofx_ctx *ctx, const double *I1, const double *I2, double *I1n, double *I2n,
                              int size);
int ofx_image_normalization_1(ofx_ctx *ctx, const double *I, double *In, int size);      /* src/utils.h:17-20 */
int ofx_getminmax(ofx_ctx *ctx, const double *x, int n, double *min, double *max);        /* src/utils.h:119 */
/* The joint normalisation that opens every *_dev solver, on device-resident frames: dst[q][e] = 255 (src[q][e] - min) / (max - min)
 * for source q < nsets * per and element e < npix * nz.  src[q]: npix * nz elements of the context's "input" kind (under
 * OFX_IN_RGB8 npix PIXELS of three bytes, and nz must be 1), dense, aligned to the element; dst[q]: npix * nz elements of the
 * storage precision.  `per` consecutive sources form a set that shares {min, max}, per channel when nz > 1 interleaved channels;
 * guard != 0 as image_normalization_2: a copy where max - min <= 0; guard == 0 divides regardless (image_normalization_3).
 * nsets * per <= 32 and npix * nz < 2^31 (OFX_ERR_ARG otherwise, nothing written).  Asynchronous on the context's stream. */
/* dst[q][e] = normalisation of src[q][e] (elements of the context's "input" kind) into the storage type: nsets sets of `per`
 * sources share {min, max} per channel; guard as image_normalization_2 (copy where max - min <= 0); nsets * per <= 32 */
int ofx_normalize_frames_dev(ofx_ctx *ctx, int nsets, int per, const void *const *src, void *const *dst, int npix, int nz, int guard);
/* ... on frames of ny rows of nx * nz elements (OFX_IN_RGB8: nx pixels), read under the options "input" and "input_pitch"; dst[q]
 * is dense, nx * ny * nz elements.  With "input_pitch" = 0 it is ofx_normalize_frames_dev with npix = nx * ny, bit for bit; the
 * same limits and errors, and those of the pitch (option "input" above). */
int ofx_normalize_frames2d_dev(ofx_ctx *ctx, int nsets, int per, const void *const *src, void *const *dst, int nx, int ny, int nz, int guard);
/* The whole pyramid head of the pyramidal *_dev solvers on its own, for n_pairs = 1..16 pairs in lockstep: per pair
 * image_normalization_2, the presmoothing gaussian(sigma) and nscales - 1 times zoom_out(zfactor), built by the schedule that the
 * option "gauss_fused" selects (every schedule gives the same planes).  dI0[g], dI1[g]: the nx x ny device images of pair g, read
 * exactly as the *_group_dev solvers read them (the context's "input" kind).  dL0[s], dL1[s], s < nscales: level s of all first /
 * all second images -- n_pairs planes of nxs[s] * nys[s] elements of the storage precision back to back, level 0 being nx x ny and
 * level s the ofx_zoom_size of level s - 1.  OFX_ERR_ARG for a group size outside 1..16, OFX_ERR_SIGMA where a level is too small
 * for the Gaussian that is taken on it (kernel radius + 1 >= width or height): a refused call writes nothing.  Asynchronous on the
 * context's stream. */
int ofx_pyramid_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI0, const void *const *dI1, int nx, int ny, int nscales,
                          double zfactor, double sigma, void *const *dL0, void *const *dL1);

/* ---- TV-L1 (replace src/tvl1flow.h:36-70) ----------------------------------------------------*/
/* single scale: u1/u2 are read as the initial flow and overwritten with the result */
int ofx_tvl1_single_scale(ofx_ctx *ctx, const double *I0, const double *I1, double *u1, double *u2,
                          int nx, int ny, double tau, double lambda, double theta, int warps,
                          double epsilon, int verbose);
/* multiscale: incoming u1/u2 content is ignored (zeroed at the coarsest level) */
int ofx_tvl1_multiscale(ofx_ctx *ctx, const double *I0, const double *I1, double *u1, double *u2,
                        int nx, int ny, double tau, double lambda, double theta, int nscales,
                        double zfactor, int warps, double epsilon, int verbose);

/* Device-resident variant: dI0/dI1 are device arrays of nx*ny elements of the context's storage
 * precision (double for OFX_F64, float for OFX_F32); d_flo receives the Middlebury .flo payload,
 * nx*ny interleaved (u,v) float32 pairs (src/tvl1flow_main.cpp:209-213).  Runs on the context's
 * stream; returns after the solve has been fully enqueued AND its convergence tests resolved
 * (the result itself is complete once the stream is synchronised). */
int ofx_tvl1_multiscale_dev(ofx_ctx *ctx, const void *dI0, const void *dI1, void *d_flo,
                            int nx, int ny, double tau, double lambda, double theta, int nscales,
                            double zfactor, int warps, double epsilon, int verbose);

/* Lockstep group: n_pairs (1..16) independent pairs of the same size solved by ONE context with shared
 * kernel launches (every level array holds the pairs back to back, blockIdx.y = pair).  Each pair keeps
 * its own stopping test, iteration counts and ping-pong phase, so every flow is bit-identical to what
 * ofx_tvl1_multiscale_dev computes for that pair alone; what is shared is the launch latency of the small
 * pyramid levels and the host's convergence polls.  dI0/dI1/d_flo: n_pairs device pointers (layout of
 * ofx_tvl1_multiscale_dev); stats_out: optional, n_pairs records.  Asynchronous like the single-pair call. */
int ofx_tvl1_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI0, const void *const *dI1,
                       void *const *d_flo, int nx, int ny, double tau, double lambda, double theta,
                       int nscales, double zfactor, int warps, double epsilon, ofx_stats *stats_out);

/* Batch of independent pairs on one OR SEVERAL devices (the unit of parallel work is the image pair).
 * The pairs are cut into lockstep groups of ofx_tvl1_batch_group_size() consecutive pairs;
 * group q is solved on context ctxs[q % n_ctx] with ofx_tvl1_group_dev, one host thread per context, so
 * n_ctx groups are in flight at a time (each context = its own HIP stream and workspace; same precision).
 * The contexts may live on different GPUs: a group whose images or payload arrays are not device memory of
 * its context's GPU -- another GPU's memory, pinned or pageable host memory -- is staged through the context's
 * workspace (peer / host copies on the context's stream) and its payloads are copied back into the caller's
 * arrays: a single-process multi-GPU batch with the results gathered where the caller wants them.
 * Arrays dI0/dI1/d_flo hold n_pairs pointers with the layout of ofx_tvl1_multiscale_dev.  work_pix_iters (optional, n_pairs doubles)
 * receives sum n_iter*nx_s*ny_s per pair.  Returns after every pair has been fully solved (all
 * streams synchronised); the first failing group's status is returned. */
int ofx_tvl1_batch_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI0, const void *const *dI1,
                       void *const *d_flo, int n_pairs, int nx, int ny, double tau, double lambda,
                       double theta, int nscales, double zfactor, int warps, double epsilon,
                       double *work_pix_iters);

/* Group size ofx_tvl1_batch_dev picks for this batch: the "lockstep" option of ctxs[0] if > 0, else the batch
 * is spread over the fewest rounds a group of 16 (less if device memory is short) allows, one group per
 * context and round, with the groups evened out.  Returns the size (>= 1), or -status (e.g. -OFX_ERR_ARG,
 * -OFX_ERR_SIGMA for a pyramid that cannot be built) on error. */
int ofx_tvl1_batch_group_size(ofx_ctx *const *ctxs, int n_ctx, int n_pairs, int nx, int ny, int nscales,
                              double zfactor);

/* ---- TV-L1 warm start: a flow to start from, and the video chain ------------------------------------------------
 * The start of a pair is a .flo payload P as every solver writes it: nx * ny interleaved (u, v) float32, 8-byte aligned.  It
 * enters the solve as follows (restated in tests/tvl1_warm_ref.py):
 *   W_0 = ((double) P.u, (double) P.v), a component that is not finite (NaN, +-Inf) taken as 0.0 -- part of the result: no input
 *         can put a NaN into the warp's coordinates;
 *   W_s = zoom_out(W_{s-1}, zfactor) * zfactor for s = 1 .. nscales - 1, per component: the reference's zoom_out (src/zoom.cpp)
 *         exactly as ofx_zoom_out and the image pyramid compute it, then ONE rounded multiply -- the mirror of the
 *         `*= 1.0 / zfactor` of src/tvl1flow.cpp:306-309 -- in double storage and arithmetic whatever the context's precision;
 *   the flow at the coarsest level is W_{nscales-1}, rounded once to the storage type; everything after that is the driver of
 *   ofx_tvl1_group_dev, unchanged.
 * A pair without a start (NULL) begins at zero as it always did, a NULL table is ofx_tvl1_group_dev itself, and an all-zero
 * payload therefore gives ofx_tvl1_group_dev's result bit for bit.
 * Out of scope: a start for the bidirectional entries (ofx_tvl1_bidir_*) and for the host-plane entries (ofx_tvl1_multiscale;
 * ofx_tvl1_single_scale has always read u1 / u2 as its start).
 *
 * ofx_tvl1_group_init_dev is ofx_tvl1_group_dev with that start: d_flo_init is NULL, or n_pairs pointers, each NULL or a payload.
 * d_flo_init[g] == d_flo[g] is allowed: the start is consumed before any payload is written.  Per pair the result is what the same
 * call computes for that pair alone; warm and cold pairs may share a group.  Frames are read under "input" / "input_pitch" like
 * ofx_tvl1_group_dev's; start payloads that are not on the context's GPU are staged as ofx_tvl1_batch_dev stages its buffers.
 * Refusals, before any work, nothing written, the reason in ofx_last_error: those of ofx_tvl1_group_dev; a start pointer that is
 * not 8-byte aligned (OFX_ERR_ARG, its pair index named); OFX_ERR_SIGMA as the image pyramid gives it (same levels, same sigma). */
int ofx_tvl1_group_init_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI0, const void *const *dI1,
                            const void *const *d_flo_init, void *const *d_flo, int nx, int ny, double tau, double lambda,
                            double theta, int nscales, double zfactor, int warps, double epsilon, ofx_stats *stats_out);
/* ofx_tvl1_batch_dev with the same extra table after dI1; the same grouping rule (ofx_tvl1_batch_group_size, whose memory rule
 * counts the start's scratch).  Groups run concurrently: a start may be the pair's own slot of d_flo, not another pair's. */
int ofx_tvl1_batch_init_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI0, const void *const *dI1,
                            const void *const *d_flo_init, void *const *d_flo, int n_pairs, int nx, int ny, double tau,
                            double lambda, double theta, int nscales, double zfactor, int warps, double epsilon,
                            double *work_pix_iters);
/* The video chain for n_seq (1..16) device-resident sequences (cameras) of n_frames >= 2 frames: sequence q is the frames
 * dF[q * n_frames + t] and the payloads d_flo[q * (n_frames - 1) + t].  Step t solves the pairs (F[q][t], F[q][t + 1]) of all
 * sequences as one lockstep group: step 0 cold with nscales_first scales, step t > 0 from d_flo[q][t - 1] with nscales_next
 * scales -- that payload is on the device already, so there is no host round trip between steps.  Each payload is bit for bit
 * what the chained ofx_tvl1_group_init_dev calls write.  Consecutive steps do not share a frame's pyramid: image_normalization_2
 * takes min / max over the two images of a pair, so a frame is a different plane in each of its two pairs.  stats_out: NULL or
 * n_seq * (n_frames - 1) records, laid out like d_flo.  Both pyramids (nscales_first, nscales_next) are validated before any
 * work.  Refusals as ofx_tvl1_group_init_dev, and OFX_ERR_ARG for n_seq outside 1..16, n_frames < 2, a payload that is not
 * 8-byte aligned. */
int ofx_tvl1_sequence_group_dev(ofx_ctx *ctx, int n_seq, int n_frames, const void *const *dF, void *const *d_flo, int nx, int ny,
                                double tau, double lambda, double theta, int nscales_first, int nscales_next, double zfactor,
                                int warps, double epsilon, ofx_stats *stats_out);
/* The start's pyramid alone, a test and inspection hook like ofx_pyramid_group_dev: d_flo[g], g < n_flows (1..16): a payload on
 * the context's GPU; d_uv[g] receives W_{nscales-1} as nxs * nys interleaved (u, v) DOUBLES, 16-byte aligned, in either
 * precision.  nscales = 1 is the conversion with the non-finite rule alone.  Refusals as above.  Asynchronous. */
int ofx_flow_pyramid_dev(ofx_ctx *ctx, int n_flows, const void *const *d_flo, int nx, int ny, int nscales, double zfactor,
                         void *const *d_uv);

/* Forward-backward consistency of two .flo payloads, from any solver (Sundaram, Brox, Keutzer, ECCV 2010): the per-pixel
 * occlusion / reliability maps of n_pairs >= 1 pairs of flow fields, both directions, on the device.
 * d_flo_fwd[g], d_flo_bwd[g]: payloads as every *_dev solver writes them, nx * ny interleaved (u, v) float32, 8-byte aligned; the
 * forward one is A -> B on A's grid, the backward one B -> A on B's grid.  d_occ_fwd[g], d_occ_bwd[g]: nx * ny bytes each, at ANY
 * byte alignment, written dense; 255 = the vector fails the check, 0 = it passes (the convention of the tvl1occ maps).  No byte
 * outside a map's nx * ny is written.  The pointers are DEVICE memory of the context's GPU, used in place; a payload or a map
 * that lives elsewhere (pinned or pageable host memory, another GPU) is staged through the context's workspace as
 * ofx_tvl1_batch_dev stages its buffers -- the front-end's route, at the cost of the copies.
 * The forward map at row i, column j, in double, every operation rounded, nothing contracted, association as written:
 *     u = F[i][j].x, v = F[i][j].y;  xt = j + u, yt = i + v
 *     255 unless 0 <= xt <= nx - 1 and 0 <= yt <= ny - 1         (the vector leaves the image; NaN and Inf land here)
 *     (bu, bv) = bicubic_interpolation_at_color(B, xt, yt, nx, ny, 2, 0 / 1, false), B = the backward payload as a 2-channel
 *                interleaved image (src/bicubic_interpolation.h:30-43: Neumann boundary, the reference's tap rule)
 *     du = u + bu, dv = v + bv
 *     0 if du du + dv dv <= alpha ((u u + v v) + (bu bu + bv bv)) + beta, else 255                   (a NaN anywhere: 255)
 * and the backward map is the same with the payloads exchanged.  The paper's thresholds are alpha = 0.01, beta = 0.5.  A pure
 * function of the float payloads: the same bytes in every precision and mode.
 * OFX_ERR_ARG before any work, nothing written, the reason in ofx_last_error: a NULL table or entry, n_pairs < 1, nx < 2 or
 * ny < 2 (or nx * ny beyond an int), alpha or beta negative or not finite, a payload that is not 8-byte aligned.
 * Asynchronous on the context's stream. */
int ofx_flow_consistency_dev(ofx_ctx *ctx, int n_pairs, const void *const *d_flo_fwd, const void *const *d_flo_bwd,
                             void *const *d_occ_fwd, void *const *d_occ_bwd, int nx, int ny, double alpha, double beta);

/* TV-L1 in both directions with the consistency maps: n_pairs (1..8) pairs in 2 * n_pairs lockstep slots of ONE context -- slot g
 * solves (dI0[g], dI1[g]), slot n_pairs + g solves (dI1[g], dI0[g]) -- over one pyramid: image_normalization_2 takes its
 * min / max over both images, so each image is normalised, presmoothed and zoomed once and serves as first image of one slot
 * and second image of the other.  d_flo_fwd[g] is BIT FOR BIT what ofx_tvl1_multiscale_dev(dI0[g], dI1[g]) writes, d_flo_bwd[g]
 * what ofx_tvl1_multiscale_dev(dI1[g], dI0[g]) writes, with equal iteration tables, in every mode and under every option.
 * d_occ_fwd[g], d_occ_bwd[g]: the maps of ofx_flow_consistency_dev(alpha = fb_alpha, beta = fb_beta) on those payloads, written
 * by one launch for all slots.  Frames as ofx_tvl1_group_dev reads them (options "input", "input_pitch"); frames, payloads and
 * maps that are not on the context's GPU are staged as ofx_tvl1_batch_dev stages them.  stats_out: optional, 2 * n_pairs
 * records, the forward slots first.  Refusals (OFX_ERR_ARG before any work): those of ofx_tvl1_group_dev and of
 * ofx_flow_consistency_dev; a group size outside 1..8 names the limit.  Asynchronous like ofx_tvl1_group_dev. */
int ofx_tvl1_bidir_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI0, const void *const *dI1,
                             void *const *d_flo_fwd, void *const *d_flo_bwd, void *const *d_occ_fwd, void *const *d_occ_bwd,
                             int nx, int ny, double tau, double lambda, double theta, int nscales, double zfactor, int warps,
                             double epsilon, double fb_alpha, double fb_beta, ofx_stats *stats_out);
/* ... a batch of them, with the shape of ofx_tvl1_batch_dev: groups of consecutive pairs, group q on ctxs[q % n_ctx], one host
 * thread per context, the contexts agreeing on precision, "input" and "input_pitch"; the first failing group's status is
 * returned.  Option "lockstep" counts SLOTS: a group holds max(1, lockstep / 2) pairs, else
 * max(1, ofx_tvl1_batch_group_size(ctxs, n_ctx, 2 * n_pairs, ...) / 2).  work_pix_iters: optional, 2 * n_pairs doubles, the forward
 * solves first, then the backward ones. */
int ofx_tvl1_bidir_batch_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI0, const void *const *dI1,
                             void *const *d_flo_fwd, void *const *d_flo_bwd, void *const *d_occ_fwd, void *const *d_occ_bwd,
                             int n_pairs, int nx, int ny, double tau, double lambda, double theta, int nscales, double zfactor,
                             int warps, double epsilon, double fb_alpha, double fb_beta, double *work_pix_iters);

/* ---- a flow applied to frames on the device: warped frames and in-between frames ---------------------------------------------
 * What consumes the payloads and maps above.  FRAMES (dSrc, dFill, dA, dB, dDst): ny rows of nx pixels of nz interleaved
 * channels, nz = 1..4, of the element kind that option "input" selects -- OFX_IN_STORAGE (the context's double or float),
 * OFX_IN_U8, OFX_IN_U16, OFX_IN_F32; OFX_IN_RGB8 is OFX_ERR_ARG (its meaning is "collapse to gray": an HWC byte image is OFX_IN_U8
 * with nz = 3, as for ofx_robust_expo_group_dev).  The frames that are READ honour "input_pitch" (rows of nx * nz elements, the
 * rules above; no byte outside the rows is read); dDst[g] has the same element kind, is written DENSE, is aligned to its element
 * -- a byte image may sit at any byte address -- and no byte outside its nx * ny * nz elements is written.  PAYLOADS: as every
 * *_dev solver writes them, nx * ny interleaved (u, v) float32, 8-byte aligned.  d_occ[g]: a byte map in the convention of
 * ofx_flow_consistency_dev, 0 = keep, non-zero = flagged, at any alignment.
 * All arithmetic in double, every operation rounded once, nothing contracted, association as written; every frame element
 * converts exactly to double.
 *     inside(x, y)       = x >= 0 && x <= nx - 1 && y >= 0 && y <= ny - 1          (NaN and Inf fail it, before any cast to int)
 *     sample(I, x, y, k) = bicubic_interpolation_at_color(I, x, y, nx, ny, nz, k, false)   (src/bicubic_interpolation.h:30-43)
 *     conv(x)            = x for double frames; (float) x for float frames; for U8 / U16 with max = 255 / 65535: NaN -> 0,
 *                          x <= 0 -> 0, x >= max -> max, otherwise (int) (x + 0.5)
 * ofx_flow_warp_dev, the backward warp of slot g at row i, column j:
 *     (u, v) = flo[i][j];  x = j + u;  y = i + v
 *     keep = inside(x, y) && (no map for this slot || occ[i * nx + j] == 0)
 *     keep      : dst[i][j][k] = conv(sample(Src, x, y, k))
 *     otherwise : dst[i][j][k] = Fill[i][j][k] copied unchanged (same kind and pitch as Src), or 0 where the slot has no fill frame
 * d_occ and dFill may be NULL, and so may their entries.  A zero payload writes Src exactly.
 * ofx_flow_interpolate_dev, the in-between frame at time t[g] in [0, 1] (t: a HOST array of n values, read before the call
 * returns) from the two payloads of a bidirectional solve -- fwd: A -> B on A's grid, bwd: B -> A on B's grid -- with the flow
 * approximation of Jiang et al., "Super SloMo", CVPR 2018, eq. 4:
 *     s = 1 - t;  c0 = s * t;  c1 = t * t;  c2 = s * s
 *     (u01, v01) = fwd[i][j];  (u10, v10) = bwd[i][j]
 *     xa = j + (c1 * u10 - c0 * u01);  ya = i + (c1 * v10 - c0 * v01)              where this pixel is in A
 *     xb = j + (c2 * u01 - c0 * u10);  yb = i + (c2 * v01 - c0 * v10)              ... and in B
 *     ina = inside(xa, ya);  inb = inside(xb, yb)
 *     o_k = ina && inb ? s * sample(A, xa, ya, k) + t * sample(B, xb, yb, k)
 *         : ina ? sample(A, xa, ya, k) : inb ? sample(B, xb, yb, k) : s * A[i][j][k] + t * B[i][j][k]
 *     dst[i][j][k] = conv(o_k)
 * t = 0 writes A exactly and t = 1 writes B exactly (finite payloads).  The consistency maps take no part: gating the blend by
 * them measured no better; they do their work in the warp, where a flagged pixel takes the fill frame.
 * Both results are pure functions of the frames' values and the float payloads: for U8, U16 and F32 frames an f64 and an f32
 * context write the same bytes, and option "apply_lds" changes nothing.
 * n >= 1 slots of any number, OFX_MAX_GROUP = 16 per launch; several slots may name the same frames and payloads (three in-between
 * frames of one pair in one launch).  A frame, payload, map or destination that is not on the context's GPU is staged as
 * ofx_tvl1_batch_dev stages its buffers, a pitched frame as it lies.  Asynchronous on the context's stream.
 * OFX_ERR_ARG before any work, nothing written, the reason in ofx_last_error: a NULL table or entry (but d_occ, dFill and their
 * entries), n < 1, nx < 2 or ny < 2, nx * ny * nz beyond an int, nz outside 1..4, a t[g] outside [0, 1] or not finite, a payload
 * that is not 8-byte aligned, a frame that is not aligned to its element, "input" = OFX_IN_RGB8, the refusals of "input_pitch",
 * a dDst[g] equal to a frame pointer that its own slot reads. */
int ofx_flow_warp_dev(ofx_ctx *ctx, int n, const void *const *dSrc, const void *const *d_flo, const void *const *d_occ,
                      const void *const *dFill, void *const *dDst, int nx, int ny, int nz);
int ofx_flow_interpolate_dev(ofx_ctx *ctx, int n, const void *const *dA, const void *const *dB, const void *const *d_flo_fwd,
                             const void *const *d_flo_bwd, const double *t, void *const *dDst, int nx, int ny, int nz);

/* ---- Median of a flow: outliers removed, flagged vectors filled from their neighbours -----------------------------------------
 * What cleans a payload between ofx_flow_consistency_dev and ofx_flow_warp_dev.  d_flo_in[g], d_flo_out[g]: payloads as every
 * *_dev solver writes them, nx * ny interleaved (u, v) float32, 8-byte aligned.  d_occ[g]: a byte map in the convention of
 * ofx_flow_consistency_dev, 0 = valid, non-zero = flagged, at any byte alignment; d_occ and its entries may be NULL.
 * For each component on its own, at row i, column j:
 *   - The window is W x W around the pixel, W = wsize.
 *   - Indices are mirrored with repetition of the border sample: -k -> k - 1, n - 1 + k -> n - k (the rule of
 *     me_median_filtering, src/utils.cpp:150-213).  It needs W / 2 <= nx and W / 2 <= ny.
 *   - A mirrored position counts as often as it occurs.
 * Unmasked result: the output is element [W * W / 2] of the sorted window.
 * Masked result, where the slot has a map:
 *   - Only window positions whose map byte is 0 take part.
 *   - The output is element [cnt / 2] of the cnt sorted valid values.
 *   - If cnt = 0, the input value is copied unchanged.
 *   - A flagged pixel with valid neighbours is therefore filled from them.  A valid pixel is filtered among valid ones only.
 * Order: -Inf < finite < +Inf < NaN, which is what np.sort does.
 *   - All NaNs are equal.
 *   - -0.0 equals +0.0, and which of two equal values is emitted cannot be told.
 *   - So results are compared with == plus equal NaN positions.
 *   - A NaN in one window comes out where and only where the definition puts it.
 * No arithmetic happens on the values.  The result is a selection, exact in every precision: a pure function of the floats and the
 * bytes, the same bytes from an f64 and an f32 context.  An all-zero map gives what no map gives; an all-flagged map returns the
 * input.  No byte outside a destination's nx * ny * 8 is written.
 * n >= 1 slots of any number, OFX_MAX_GROUP = 16 per launch; several slots may read the same payload.  A payload, map or
 * destination that is not on the context's GPU is staged as ofx_flow_warp_dev stages its buffers.  Asynchronous on the context's
 * stream.
 * OFX_ERR_ARG before any work, nothing written, the reason in ofx_last_error: a NULL table or entry (but d_occ and its entries),
 * n < 1, nx < 2 or ny < 2, nx * ny beyond an int, wsize not in {3, 5, 7}, wsize / 2 > min(nx, ny), a payload that is not 8-byte
 * aligned, a d_flo_out[g] equal to the payload that its own slot reads. */
int ofx_flow_median_dev(ofx_ctx *ctx, int n, const void *const *d_flo_in, const void *const *d_occ, void *const *d_flo_out, int nx,
                        int ny, int wsize);

/* ---- Flows composed along a sequence: long-range flows and point tracks ---------------------------------------------------------
 * "Where did this pixel of frame 0 go by frame k?"  The step payloads of a video (ofx_tvl1_sequence_group_dev and its kin) are
 * chained on the device: follow a point through the step flows, sample each flow at the sub-pixel position reached, stop where the
 * consistency map flags the position (Sundaram, Brox, Keutzer, "Dense point trajectories by GPU-accelerated large displacement
 * optical flow", ECCV 2010).  PAYLOADS: as every *_dev solver writes them, nx * ny interleaved (u, v) float32, 8-byte aligned.
 * MAPS: bytes in the convention of ofx_flow_consistency_dev, 0 = valid, non-zero = flagged / lost, at ANY byte alignment, written
 * dense with 0 and 255.  No byte outside a destination is written.
 * All arithmetic in double, every operation rounded once, nothing contracted, association as written:
 *     inside(x, y)     = x >= 0 && x <= nx - 1 && y >= 0 && y <= ny - 1            (NaN and Inf fail it, before any cast to int)
 *     sample(S, x, y)  = (bicubic_interpolation_at_color(S, x, y, nx, ny, 2, 0, false), (..., 1, false)), S = a step payload as a
 *                        2-channel interleaved image of doubles converted exactly from its floats: the sampling of
 *                        ofx_flow_consistency_dev
 *     flagged(M, x, y) = for an inside position and a map M: x0 = (int) x, x1 = x0 + (x > x0), y0 = (int) y, y1 = y0 + (y > y0);
 *                        true if any of M[y0][x0], M[y0][x1], M[y1][x0], M[y1][x1] is non-zero.  At an integer position only the
 *                        pixel itself counts; no index leaves the map; without a map it is false.
 *     advance(p, S, M) = one step of a point at the inside position p = (x, y): flagged(M, x, y) -> lost; otherwise (bu, bv) =
 *                        sample(S, x, y), q = (x + bu, y + bv); !inside(q) -> lost (a NaN or Inf in the step lands here);
 *                        otherwise the point moves to q.
 * ofx_flow_compose_dev, one step for slot g at row i, column j:
 *     (U, V) = ab[i][j];  m = occ_ab[i][j]      (a NULL d_flo_ab table or entry: the zero flow; a NULL d_occ_ab table or entry: 0)
 *     m != 0 || !inside(j + U, i + V) :  ac[i][j] = ab[i][j] bit for bit, occ_ac[i][j] = 255
 *     f = flagged(occ_bc, j + U, i + V);  (bu, bv) = sample(bc, j + U, i + V);  Un = (float) (U + bu);  Vn = (float) (V + bv)
 *     f || !inside(j + Un, i + Vn)    :  ac[i][j] = ab[i][j] bit for bit, occ_ac[i][j] = 255
 *     otherwise                       :  ac[i][j] = (Un, Vn), occ_ac[i][j] = 0
 * A lost vector stays where it was lost and stays lost.  With the zero flow for ab the result is bc itself wherever bc's vector
 * stays inside and is unflagged.  An all-zero bc returns ab with lost vectors flagged.
 * d_occ_bc, d_occ_ac and their entries may be NULL (no map / the map is not wanted).  d_flo_ac[g] == d_flo_ab[g] and d_occ_ac[g] ==
 * d_occ_ab[g] are allowed -- a pixel reads only its own element of them: the streaming use, one accumulated payload advanced step
 * by step.  d_flo_ac[g] == d_flo_bc[g] is refused (and d_occ_ac[g] == d_occ_bc[g]): the step is read at other pixels.
 * n >= 1 slots of any number, OFX_MAX_GROUP = 16 per launch.
 * ofx_flow_accumulate_dev, the chain: tables laid out like d_flo of ofx_tvl1_sequence_group_dev, step t of sequence q is element
 * q * n_steps + t.
 *     acc[q][0] = compose(zero flow, step[q][0]);  acc[q][t] = compose(acc[q][t - 1], step[q][t])
 * with occ_acc[q][t] the map of that call and occ_step[q][t] the step's own map.  Every payload and map is bit for bit what the
 * chained ofx_flow_compose_dev calls write: n_steps launches over all sequences.  n_seq >= 1 of any number, n_steps >= 1.
 * d_occ_step and d_occ_acc may be NULL, tables or entries; without d_occ_acc the lost state still travels from step to step,
 * through the context's workspace.  acc[q][t] may be acc[q][t - 1] (only the last payload is wanted); it may not be a step payload
 * that the chain has yet to read.  A chain backwards in time is the backward payloads handed over in reverse order: step[q][t] =
 * the payload of frame k - t -> frame k - t - 1 gives acc[q][t] = frame k -> frame k - t - 1 on frame k's grid.
 * acc[q][k - 1] with its map goes into ofx_flow_warp_dev (frame k registered onto frame 0), into ofx_flow_median_dev (lost vectors
 * filled from surviving neighbours) and into ofx_tvl1_group_init_dev as the start of a direct 0 -> k solve.
 * ofx_flow_tracks_dev, sparse query points kept in double, no float rounding between steps.  d_xy0[q]: n_pts interleaved (x, y)
 * doubles; d_xy[q]: (n_steps + 1) * n_pts interleaved doubles, step-major (position t of point k at 2 * (t * n_pts + k));
 * d_len[q]: n_pts int32.  Per point:
 *     p_0 = xy0;  !inside(p_0): len = -1 and every p_t = p_0 bit for bit
 *     p_{t+1} = advance(p_t, step[q][t], occ_step[q][t]) while the point lives
 *     the first lost step t sets len = t and every later position repeats p_t;  a point that survives has len = n_steps
 * One launch marches all steps, a thread owns a point; the step pointers go through a device table, whose upload the call awaits
 * (it waits for the stream's earlier work), the march itself is asynchronous.
 * All three are pure functions of the floats, the bytes and the query doubles: the same bytes from an f64 and an f32 context.
 * A payload, map, position array or destination that is not on the context's GPU is staged as ofx_flow_warp_dev stages its
 * buffers.  Asynchronous on the context's stream.
 * OFX_ERR_ARG before any work, nothing written, the reason in ofx_last_error: a NULL d_flo_bc / d_flo_ac / d_flo_step / d_flo_acc /
 * d_xy0 / d_xy / d_len table or entry, n < 1, n_seq < 1, n_steps < 1, n_pts < 1, nx < 2 or ny < 2, nx * ny beyond an int, a payload
 * or position array that is not 8-byte aligned, a d_len[q] that is not 4-byte aligned, the refused aliases. */
int ofx_flow_compose_dev(ofx_ctx *ctx, int n, const void *const *d_flo_ab, const void *const *d_occ_ab, const void *const *d_flo_bc,
                         const void *const *d_occ_bc, void *const *d_flo_ac, void *const *d_occ_ac, int nx, int ny);
int ofx_flow_accumulate_dev(ofx_ctx *ctx, int n_seq, int n_steps, const void *const *d_flo_step, const void *const *d_occ_step,
                            void *const *d_flo_acc, void *const *d_occ_acc, int nx, int ny);
int ofx_flow_tracks_dev(ofx_ctx *ctx, int n_seq, int n_steps, const void *const *d_flo_step, const void *const *d_occ_step, int n_pts,
                        const void *const *d_xy0, void *const *d_xy, void *const *d_len, int nx, int ny);

/* ---- Track seeds and dense point trajectories ----------------------------------------------------------------------------------
 * Where the tracks of ofx_flow_tracks_dev should start, and new tracks while a clip runs: the seeding of Sundaram, Brox, Keutzer
 * (ECCV 2010).  Points are placed on a grid of step x step cells, kept where the smaller eigenvalue of the smoothed structure
 * tensor reaches a fraction of its image mean, and every new frame is seeded again in the cells that no live track occupies.
 * FRAMES: ONE-channel frames of the element kind that option "input" selects (all five kinds; OFX_IN_RGB8 collapses to gray),
 * read under "input_pitch" exactly as ofx_structure_texture_dev reads them.  PAYLOADS and MAPS: as ofx_flow_tracks_dev takes them.
 * All arithmetic in double whatever the context's precision, every operation rounded once, nothing contracted, association as
 * written, sqrt correctly rounded:
 *     f          = (double) sample
 *     (gx, gy)   = centered_gradient(f)               src/operators.cpp, nz = 1, its border rule: what ofx_centered_gradient computes
 *     a = gx * gx;  b = gx * gy;  c = gy * gy
 *     A, B, C    = gaussian(a | b | c, nx, ny, rho)   src/operators.cpp:506-624 with its defaults (reflecting boundary, window 5):
 *                                                     size = (int) (5 * rho) + 1 taps, rows of the whole plane, then columns, the
 *                                                     coefficients computed on the host with libm as ofx_gaussian has them
 *     d = A - C;  e = B + B;  r = sqrt(d * d + e * e)
 *     lam2       = 0.5 * ((A + C) - r)
 *     sum64(v)   = p[l] = v[l] + v[l + 64] + v[l + 128] + ... left to right, l = 0 .. 63 (a lane without an element is +0.0);
 *                  then for s = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + s] for l < s; the value is p[0]
 *     mean       = sum64([sum64(row i of lam2) for i = 0 .. ny - 1]) / (double) (nx * ny)
 *     tau        = frac * mean
 * CELLS are step x step pixels; cell (ca, cb) has the candidate pixel x = ca * step + step / 2, y = cb * step + step / 2 (integer
 * division), none where that lies beyond nx - 1 or ny - 1.  A candidate has STRUCTURE when lam2[y][x] >= tau (a NaN fails).  A
 * point p OCCUPIES cell ((int) px / step, (int) py / step) when inside(p) of the section above holds; other points occupy
 * nothing.  The SEEDS of a frame are the candidates with structure in unoccupied cells, as (x, y) doubles in row-major cell order,
 * cb outer: the order is part of the result, the same from run to run (a scan, no atomics).
 * ofx_track_structure_dev: d_lam2[g] receives lam2 of frame dF[g] as nx * ny doubles, d_mean[g] its mean as one double.  d_lam2 and
 * d_mean may be NULL, tables or entries.  The inspection hook of the fused kernel.
 * ofx_track_seed_dev: the seeds of n frames.  d_xy_occ: NULL, or a table (NULL entries allowed) of n_occ interleaved (x, y) doubles
 * per slot that occupy cells.  d_xy_new[g] receives at most cap seeds; d_count[g] two int32: the seeds written, and the seeds
 * dropped for lack of room -- the last in cell order.  No byte beyond the seeds written is touched.
 * ofx_track_sequence_dev: n_seq clips of n_frames frames, tables laid out like those of ofx_flow_accumulate_dev: frame f of clip
 * q at q * n_frames + f, step t at q * (n_frames - 1) + t; d_occ_step optional, table or entries.  d_xy[q]: n_frames * cap
 * interleaved doubles, frame-major (slot k at frame f at 2 * (f * cap + k)); d_t0[q], d_len[q]: cap int32; d_count[q]: two int32,
 * slots used and seeds dropped.  The slots start as the seeds of frame 0 with t0 = 0.  For t = 0 .. n_frames - 2:
 *     every live slot moves by advance(p, step[t], occ_step[t]); a slot lost there keeps len = t - t0 and is dead from frame t + 1 on;
 *     then the survivors' positions at frame t + 1 occupy cells;
 *     then the seeds of frame t + 1 are appended in cell order with t0 = t + 1.
 * A slot that survives to the end has len = n_frames - 1 - t0.  Every used slot has all n_frames positions written: the frames
 * before t0 repeat the birth position bit for bit, the frames after the loss repeat the last one.  Slots beyond the count are not
 * written at all.  The slots born at frame 0 are bit for bit the tracks of ofx_flow_tracks_dev from the seeds of frame 0.
 * Counts and tables stay on the device between the steps: the call makes no host synchronisation; its launches are sized by cap
 * and the cell count and read the counters on the device.  Up to OFX_MAX_GROUP = 16 frames or clips share every launch, any n.
 * Pure functions of the samples, floats, map bytes and doubles: the same bytes from an f64 and an f32 context on the same sample
 * values.  Buffers that are not on the context's GPU are staged as ofx_flow_warp_dev stages them.  Asynchronous on the context's
 * stream.
 * OFX_ERR_ARG before any work, nothing written, the reason in ofx_last_error: NULL required tables or entries; n, n_seq or cap < 1,
 * n_occ < 0, n_frames < 2, step < 1, nx < 2 or ny < 2, nx * ny beyond an int; rho not finite or <= 0, or more than
 * OFX_TRACK_MAX_SIZE taps; frac not finite or < 0; misaligned frames, doubles or int32s; the refusals of "input_pitch"; an output
 * that is an input of the call or another output of its slot.  OFX_ERR_SIGMA under ofx_zoom_out's rule: size >= nx or size >= ny. */
#define OFX_TRACK_MAX_SIZE 11   /* the largest (int) (5 * rho) + 1: rho below 2.2 */
int ofx_track_structure_dev(ofx_ctx *ctx, int n, const void *const *dF, void *const *d_lam2, void *const *d_mean, int nx, int ny,
                            double rho);
int ofx_track_seed_dev(ofx_ctx *ctx, int n, const void *const *dF, const void *const *d_xy_occ, int n_occ, void *const *d_xy_new,
                       void *const *d_count, int cap, int nx, int ny, double rho, double frac, int step);
int ofx_track_sequence_dev(ofx_ctx *ctx, int n_seq, int n_frames, const void *const *dF, const void *const *d_flo_step,
                           const void *const *d_occ_step, int cap, void *const *d_xy, void *const *d_t0, void *const *d_len,
                           void *const *d_count, int nx, int ny, double rho, double frac, int step);

/* ---- The dominant motion of a flow: a robust parametric fit ---------------------------------------------------------------------
 * How much of a flow is the camera's?  A global motion model -- a translation, a similarity or an affine map -- is fitted to a .flo
 * payload by iteratively re-weighted least squares with Tukey's biweight (Odobez, Bouthemy, "Robust multiresolution estimation of
 * parametric motion models", JVCIR 1995); the model's flow, the camera-compensated residual flow and the pixels that disagree with
 * the model -- the moving foreground -- are what Wang, Schmid, "Action recognition with improved trajectories" (ICCV 2013) build on.
 * PAYLOADS and MAPS: as ofx_flow_compose_dev takes them: nx * ny interleaved (u, v) float32, 8-byte aligned; bytes at ANY
 * alignment, 0 = valid, written dense with 0 and 255.  No byte outside a destination is written.  A RECORD is OFX_MOTION_REC = 16
 * doubles, 8-byte aligned.
 * All arithmetic in double whatever the context's precision, every operation rounded once, nothing contracted, division correctly
 * rounded, association as written.  At row i, column j:
 *     cx = 0.5 * (nx - 1);  cy = 0.5 * (ny - 1);  h = 0.5 * max(nx, ny);  X = (j - cx) / h;  Y = (i - cy) / h
 *     theta = (t0, a, b, t1, c, d);  mu = (t0 + a * X) + b * Y;  mv = (t1 + c * X) + d * Y          the model's flow
 *     valid(i, j) = the map byte is 0 (no map: true) && u - u == 0 && v - v == 0                    (NaN and Inf vectors are not)
 * The WEIGHT of a valid pixel under theta and a cut-off C, in this order:
 *     du = u - mu;  dv = v - mv;  r2 = du * du + dv * dv;  C2 = C * C
 *     r2 < C2:  q = 1.0 - r2 / C2;  w = q * q        otherwise w = 0        an unweighted fit has w = 1 on every valid pixel
 * The twelve MOMENTS:
 *     S1 = sum w;        SX = sum w * X;          SY = sum w * Y
 *     SXX = sum (w * X) * X;  SXY = sum (w * X) * Y;  SYY = sum (w * Y) * Y
 *     U1 = sum w * u;    UX = sum (w * u) * X;    UY = sum (w * u) * Y;    V1, VX, VY the same with v
 * where an invalid pixel contributes +0.0 to every sum (its terms are not evaluated: a NaN vector poisons nothing) and "sum" is
 * sum64 over the rows of sum64 over the terms of a row, exactly as the mean of ofx_track_structure_dev is defined above: no
 * atomics, the order is part of the result, the same from run to run.
 * The SOLVE, with eps = 1e-12; a fit is DEGENERATE where one of its tests fails, and a NaN fails every test:
 *     translation:  t0 = U1 / S1;  t1 = V1 / S1;  a = b = c = d = 0                                  test: S1 > 0
 *     similarity (b = -c, d = a):
 *         Q = SXX + SYY;  D = Q - (SX * SX + SY * SY) / S1
 *         a = ((UX + VY) - (SX * U1 + SY * V1) / S1) / D;   c = ((VX - UY) - (SX * V1 - SY * U1) / S1) / D
 *         t0 = ((U1 - SX * a) + SY * c) / S1;               t1 = ((V1 - SY * a) - SX * c) / S1      tests: S1 > 0, D > eps * Q
 *     affine: the u and the v system share the matrix [S1 SX SY; SX SXX SXY; SY SXY SYY]; elimination without pivoting:
 *         l10 = SX / S1;  l20 = SY / S1;  a11 = SXX - l10 * SX;  a12 = SXY - l10 * SY;  a22 = SYY - l20 * SY
 *         l21 = a12 / a11;  p2 = a22 - l21 * a12
 *         per right side (r0, r1, r2) = (U1, UX, UY) -> (t0, a, b) and (V1, VX, VY) -> (t1, c, d):
 *         y1 = r1 - l10 * r0;  y2 = (r2 - l20 * r0) - l21 * y1;  z2 = y2 / p2;  z1 = (y1 - a12 * z2) / a11
 *         z0 = ((r0 - SX * z1) - SY * z2) / S1;  the solution is (z0, z1, z2)          tests: S1 > 0, a11 > eps * SXX, p2 > eps * SYY
 * The SCHEDULE of ofx_flow_motion_fit_dev: n_fits >= 1 fits per slot.  A slot without an initial record (a NULL d_motion_init table
 * or entry) starts from theta = 0 and its fit 0 is unweighted; a slot with one starts from that record's [0..5] and its fit 0 is
 * weighted from it.  Every later fit is weighted from the theta of the fit before.  The t-th WEIGHTED fit of a slot (t = 0, 1, ...)
 * uses C_t = max(c_last, c_first * 2^-t), the scaling exact.  A degenerate fit keeps the theta it started from -- for fit 0 the
 * initial record's theta, or zeros -- and all later fits of the slot are skipped.  The schedule is decided on the device, through
 * a flag in the record that the kernels of the later fits read: the call makes no host synchronisation.  Launches per call and
 * chunk of up to OFX_MAX_GROUP = 16 slots: two for each fit and one for the outputs; any n >= 1.
 * The RECORD d_motion[g]:
 *     [0..5]   theta
 *     [6..11]  the same map on pixel indices, u = p0 + p1 * j + p2 * i, v = q0 + q1 * j + q2 * i:
 *              p1 = a / h;  p2 = b / h;  p0 = (t0 - p1 * cx) - p2 * cy;  q0, q1, q2 likewise from t1, c, d
 *     [12]     S1 of the last completed fit (0 if none)        [13]  fits completed
 *     [14]     the cut-off of the inlier map, c_last           [15]  1.0 if the call stopped on a degenerate fit, otherwise 0.0
 * The OUTPUTS, under the final theta and C = c_last (ofx_flow_motion_fit_dev) or under [0..5] of the record d_motion[g] and C =
 * cutoff (ofx_flow_motion_apply_dev: a record may also come from the caller, for example a smoothed camera path):
 *     d_flo_model[g]:  ((float) mu, (float) mv)
 *     d_flo_resid[g]:  ((float) (u - mu), (float) (v - mv))     the camera-compensated flow; a NaN stays NaN
 *     d_inlier[g]:     0 where valid && r2 < C2, otherwise 255   the moving foreground and the flagged pixels together
 * A payload that is exactly the model flow of some theta, on valid pixels, has an all-zero inlier map.  The residual payload in
 * place turns a flow into the camera-compensated flow.  The model payload goes into ofx_flow_warp_dev as it is.  A slot whose map
 * flags every pixel returns the starting theta with [15] = 1.
 * d_occ, d_motion_init, d_flo_model, d_flo_resid and d_inlier may be NULL, tables or entries; in the apply entry d_flo too, then
 * only the model payload can be asked for.  d_flo_resid[g] == d_flo[g] is allowed where no other slot reads that payload -- a pixel
 * reads only its own element; every other alias between an output and an input of the call, or between two outputs of a slot, is
 * refused.  Pure functions of the floats, the bytes and the doubles: the same bytes from an f64 and an f32 context.  A buffer that
 * is not on the context's GPU is staged as ofx_flow_warp_dev stages its buffers.  Asynchronous on the context's stream.
 * OFX_ERR_ARG before any work, nothing written, the reason in ofx_last_error: NULL required tables or entries (d_flo and d_motion
 * of the fit entry, d_motion of the apply entry); n < 1, n_fits < 1; a model that is not one of the three; nx < 2 or ny < 2, nx * ny
 * beyond an int; c_first, c_last or cutoff not finite or <= 0; c_first < c_last; payloads or records that are not 8-byte aligned;
 * the refused aliases; the apply entry asked for a residual or a map without d_flo. */
#define OFX_MOTION_TRANSLATION 2
#define OFX_MOTION_SIMILARITY  4
#define OFX_MOTION_AFFINE      6
#define OFX_MOTION_REC 16       /* doubles per motion record */
int ofx_flow_motion_fit_dev(ofx_ctx *ctx, int n, const void *const *d_flo, const void *const *d_occ,
                            const void *const *d_motion_init, void *const *d_motion, int model, int n_fits,
                            double c_first, double c_last, void *const *d_flo_model, void *const *d_flo_resid,
                            void *const *d_inlier, int nx, int ny);
int ofx_flow_motion_apply_dev(ofx_ctx *ctx, int n, const void *const *d_motion, const void *const *d_flo,
                              const void *const *d_occ, double cutoff, void *const *d_flo_model,
                              void *const *d_flo_resid, void *const *d_inlier, int nx, int ny);

/* ---- Measure and show a flow: error statistics and image encodings ---------------------------------------------------------------
 * How good is a flow, and what does it look like?  ofx_flow_error_dev compares .flo payloads with their ground truth on the device:
 * end-point error, Barron's angular error, outlier rates (Middlebury's R-x, KITTI's Fl) and a histogram to take percentiles from.
 * ofx_flow_encode_dev turns payloads into images: Middlebury's colour wheel (Baker et al., "A database and evaluation methodology
 * for optical flow", IJCV 2011; colorcode.cpp of its flow-code), the bounded 8-bit x / y coding that two-stream action-recognition
 * pipelines store, and KITTI's 16-bit coding; ofx_flow_decode_dev reads the latter two back.
 * PAYLOADS, MAPS, SLOTS as ofx_flow_motion_fit_dev takes them: nx * ny interleaved (u, v) float32, 8-byte aligned; bytes at ANY
 * alignment, 0 = valid; any n >= 1, OFX_MAX_GROUP = 16 per launch.  A buffer that is not on the context's GPU is staged as
 * ofx_flow_warp_dev stages its buffers.  Asynchronous on the context's stream, no host synchronisation inside.
 * All arithmetic in double whatever the context's precision, every operation rounded once, nothing contracted, division and sqrt
 * correctly rounded, association as written.  Pure functions of the floats and bytes: the same bytes from an f64 and an f32
 * context.  No byte outside a destination is written.
 *     fin(x) = (x - x == 0);   shown(u, v) = fin(u) && fin(v) && |u| <= 1e9 && |v| <= 1e9     (Middlebury's unknown marker is not)
 *
 * ofx_flow_error_dev.  thr_abs, thr_rel: HOST arrays of n_thr (0 .. 8) values, read before the call returns.  d_occ, d_epe and
 * d_hist may be NULL, as tables or as entries.  Per pixel, (u, v) the estimate d_flo[g], (gu, gv) the truth d_flo_gt[g]:
 *     known = (map byte == 0 or no map) && shown(gu, gv);   bad = known && !(fin(u) && fin(v));   good = known && !bad
 *     good:  du = u - gu;  dv = v - gv;  e2 = du * du + dv * dv;  e = sqrt(e2);  gm = sqrt(gu * gu + gv * gv)
 *            num = (u * gu + v * gv) + 1.0;   den = sqrt((u * u + v * v) + 1.0) * sqrt((gu * gu + gv * gv) + 1.0)
 *            c = num / den;  c > 1 -> 1;  c < -1 -> -1;  ae = acos(c)          Barron's angular error in radians, the library's acos
 *     out_k = bad || (good && e > thr_abs[k] && e > thr_rel[k] * gm)            R1.0 is (1, 0), KITTI's Fl is (3, 0.05)
 *     bin   = bad ? n_bins - 1 : (q = e / bin_w;  q >= n_bins ? n_bins - 1 : (int) q)         counted over the known pixels
 * The sums Se = sum e, S2 = sum e2, Sa = sum ae run over the good pixels: a pixel that is not good contributes +0.0 by a select
 * (its terms are not evaluated), and "sum" is sum64 over the rows of sum64 over the terms of a row, exactly as the moments of
 * ofx_flow_motion_fit_dev: no floating-point atomics, the order is part of the result.  Counts and the maximum are order-free.
 * The RECORD d_rec[g]: OFX_ERROR_REC = 16 doubles, 8-byte aligned; ng = [0] - [1]; where ng = 0, [2..7] are 0.0:
 *     [0] known pixels     [1] bad pixels     [2] Se / ng     [3] sqrt(S2 / ng)     [4] (Sa / ng) * 57.29577951308232  (degrees)
 *     [5] max e over the good pixels     [6] Se     [7] Sa     (a caller pools slots exactly from [0], [1], [6] and [7])
 *     [8 + k] the count of out_k; 0.0 for k >= n_thr
 * d_epe[g]: one float32 per pixel, 4-byte aligned: (float) e where good, +Inf where bad, the quiet NaN 0x7FC00000 elsewhere.
 * d_hist[g]: n_bins uint32, 4-byte aligned, written, not accumulated.
 *
 * ofx_flow_encode_dev / ofx_flow_decode_dev.  Destinations are dense; bytes may sit at any byte address, uint16 images are 2-byte
 * aligned.  vis = (map byte == 0 or no map) && shown(u, v).
 * OFX_ENC_WHEEL_RGB8: 3 bytes per pixel, R G B.  maxrad = scale where scale > 0; where scale == 0 the slot's own
 * max sqrt(u * u + v * v) over its vis pixels, 1.0 if that is 0 or no pixel is vis: found on the device and read by the encode
 * launch, the call awaits nothing.  A pixel that is not vis is (0, 0, 0).  The wheel has 55 integer RGB entries, six segments,
 * entry i of a segment, integer divisions:
 *     RY 15: (255, 255*i/15, 0)       YG 6: (255 - 255*i/6, 255, 0)     GC 4:  (0, 255, 255*i/4)
 *     CB 11: (0, 255 - 255*i/11, 255)  BM 13: (255*i/13, 0, 255)          MR 6:  (255, 0, 255 - 255*i/6)
 *     fx = u / maxrad;  fy = v / maxrad;  rad = sqrt(fx * fx + fy * fy);  a = atan2(-fy, -fx) / 3.141592653589793
 *     fk = (a + 1.0) / 2.0 * 54.0;  k0 = (int) fk;  k1 = (k0 + 1) % 55;  f = fk - k0
 *     per channel b:  c0 = wheel[k0][b] / 255.0;  c1 = wheel[k1][b] / 255.0;  col = (1.0 - f) * c0 + f * c1
 *                     rad <= 1 ? col = 1.0 - rad * (1.0 - col) : col = col * 0.75;   byte = (int) (255.0 * col)
 * The zero vector is white; at scale = 4 the vector (1, 0) is (255, 191, 191) and (-1, 0) is (191, 243, 255).
 * OFX_ENC_BOUND_U8: 2 bytes per pixel, x then y; scale = the bound B > 0.  Per component f of a vis pixel: f <= -B gives 0,
 * f >= B gives 255, otherwise (int) (255.0 * (f + B) / (2.0 * B) + 0.5); a pixel that is not vis gets the code of 0.0, 128.
 * Decoded: f = (float) ((code * (2.0 * B)) / 255.0 - B), the map all 0.
 * OFX_ENC_KITTI_U16: 3 uint16 per pixel; scale must be 0.  A vis pixel is (q(u), q(v), 1) with x = f * 64.0 + 32768.0: x <= 0
 * gives 0, x >= 65535 gives 65535, otherwise (int) (x + 0.5); a pixel that is not vis is (0, 0, 0).  Decoded, where the third
 * value is not 0: f = (float) ((code - 32768.0) / 64.0), map 0; otherwise the payload is (NaN, NaN) and the map 255 -- the error
 * entry then treats it as unknown even without the map.  d_occ of the decode entry may be NULL, as a table or as entries.
 *
 * OFX_ERR_ARG before any work, nothing written, the reason in ofx_last_error: a NULL required table or entry (d_flo, d_flo_gt,
 * d_rec; d_flo, dDst; dSrc, d_flo); n < 1; nx < 2 or ny < 2, nx * ny beyond an int; n_thr outside 0 .. 8, n_thr > 0 with a NULL
 * threshold array, a threshold that is negative or not finite; d_hist given with n_bins outside 1 .. 65536 or bin_w not finite or
 * <= 0; a misaligned payload, record, EPE map, histogram or uint16 image; any output equal to, or overlapping, an input or
 * another output of the call; a kind that is not one of the three, a scale that is not finite or < 0, scale == 0 for BOUND,
 * scale != 0 for KITTI, WHEEL in the decode entry. */
#define OFX_ERROR_REC 16        /* doubles per error record */
#define OFX_ENC_WHEEL_RGB8 1
#define OFX_ENC_BOUND_U8   2
#define OFX_ENC_KITTI_U16  3
int ofx_flow_error_dev(ofx_ctx *ctx, int n, const void *const *d_flo, const void *const *d_flo_gt, const void *const *d_occ,
                       int n_thr, const double *thr_abs, const double *thr_rel, void *const *d_rec, void *const *d_epe,
                       void *const *d_hist, int n_bins, double bin_w, int nx, int ny);
int ofx_flow_encode_dev(ofx_ctx *ctx, int n, const void *const *d_flo, const void *const *d_occ, int kind, double scale,
                        void *const *dDst, int nx, int ny);
int ofx_flow_decode_dev(ofx_ctx *ctx, int n, const void *const *dSrc, int kind, double scale, void *const *d_flo,
                        void *const *d_occ, int nx, int ny);

/* ---- structure-texture decomposition on the device: frames for an illumination-robust flow -----------------------------------
 * dTex[g] receives the texture part T = f - alpha * S of frame dSrc[g], S being the structure part: the ROF (total variation)
 * smoothing of f by n_iter steps of Chambolle's projection -- the preprocessing of Wedel, Pock, Zach, Bischof, Cremers, "An
 * Improved Algorithm for TV-L1 Optical Flow" (2009), section 3.1.  A gain change, an exposure ramp or a soft shadow lives in S;
 * a solver that is given T for both frames no longer sees it.
 * dSrc[g]: a ONE-channel frame of ny rows of nx samples of the element kind that option "input" selects (all five kinds;
 * OFX_IN_RGB8 collapses to gray by the loader's rule above), read under "input_pitch" exactly as ofx_normalize_frames2d_dev reads
 * it; no byte outside the rows is read.  dTex[g]: nx * ny elements of the context's storage precision, dense, aligned to the
 * element.  dStruct: NULL, or a table whose entries may be NULL; a non-NULL entry receives S the same way.  No byte outside a
 * destination's nx * ny elements is written.
 * All arithmetic in double, every operation rounded once, nothing contracted, association as written, sqrt correctly rounded,
 * / the IEEE quotient:
 *     f  = (double) sample                               r = 0.25 / theta        (one division, on the host)
 *     p1 = p2 = 0
 *     repeat n_iter times:
 *         u        = f + theta * divergence(p1, p2)      src/operators.cpp:36-78, its border associations included
 *         (ux, uy) = forward_gradient(u)                 src/operators.cpp:87-125
 *         g        = 1.0 + r * sqrt(ux * ux + uy * uy)
 *         p1       = (p1 + r * ux) / g;  p2 = (p2 + r * uy) / g
 *     S = f + theta * divergence(p1, p2)
 *     T = f - alpha * S
 *     dStruct[g] = (storage type) S;  dTex[g] = (storage type) T
 * p1 and p2 are held in double between kernel launches whatever the context's precision: the float frames of an f32 context are
 * (float) of the f64 context's doubles, element for element.
 * n_iter = 0 writes S = f, exactly.
 * A constant frame writes S = f and T = f - alpha * f exactly, for every n_iter.
 * The result does not depend on "st_fuse".
 * theta is in the units of the samples: for 8-bit frames 16 is Wedel's 1/8 of the half range.  Recommended: theta = 16 * range /
 * 255, alpha = 0.95, n_iter = 100.  Measured on the CPU with the reference solver (TV-L1 defaults, 4 scales, synthetic pairs at
 * 160x120 and 131x77, average end-point error against the truth): a 20 % gain change with a ramp costs the raw frames 1.8 - 2.5
 * px and a soft shadow 3.0 - 6.4 px; on the texture frames 0.05 - 0.30 px and 0.08 - 0.64 px; unchanged pairs move by about
 * 0.01 px; 40 iterations give the same within 0.02 px.
 * The texture frames go into any *_dev solver as OFX_IN_STORAGE frames; the solvers normalise per pair, so the small range of T
 * needs no care.
 * n >= 1 slots of any number, OFX_MAX_GROUP = 16 per launch.  A source or destination that is not on the context's GPU is staged
 * as ofx_tvl1_batch_dev stages its buffers, a pitched frame as it lies.  Asynchronous on the context's stream.
 * OFX_ERR_ARG before any work, nothing written, the reason and the slot in ofx_last_error: a NULL dSrc or dTex table or entry,
 * n < 1, nx < 2 or ny < 2, nx * ny beyond an int, theta not finite or <= 0, alpha not finite or outside [0, 1], n_iter < 0 or
 * above OFX_ST_MAX_ITERS, a frame or destination that is not aligned to its element, the refusals of "input_pitch", a destination
 * equal to the source of its own slot (the sources are re-read by every launch) or to the slot's other destination. */
#define OFX_ST_MAX_ITERS 10000
#define OFX_ST_MAX_FUSE  8      /* the largest "st_fuse" */
int ofx_structure_texture_dev(ofx_ctx *ctx, int n, const void *const *dSrc, void *const *dTex, void *const *dStruct,
                              int nx, int ny, double theta, double alpha, int n_iter);

/* Fixed-work inner loop only (src/tvl1flow.cpp:113-182 run exactly n_iter times on linearised
 * data, all arrays host double planes; u/p updated in place).  Returns the last error in *error.
 * Used by the kernel-level parity tests and the roofline measurement. */
int ofx_tvl1_iterations(ofx_ctx *ctx, double *u1, double *u2, double *p11, double *p12, double *p21,
                        double *p22, const double *I1wx, const double *I1wy, const double *rho_c,
                        int nx, int ny, double tau, double lambda, double theta, int n_iter,
                        double *error);

/* libm's hypot as the TV-L1 dual update calls it (src/tvl1flow.cpp:172-173), n independent evaluations on the device:
 * out[k] = hypot(x[k], y[k]) with the operation sequence of glibc >= 2.35, bit-identical to it over the whole
 * double range.  An operator entry for direct parity tests of the one libm function on the path. */
int ofx_hypot(ofx_ctx *ctx, const double *x, const double *y, double *out, int n);

/* How ofx_tvl1_batch_dev reaches a buffer on `mem_device` (-1 = host memory) from a context on `ctx_device`: 0 = in place,
 * 1 = one copy (host <-> device, or a peer copy when hipDeviceCanAccessPeer says yes), 2 = two copies through a pinned host
 * bounce buffer (the GPUs cannot address each other; the call succeeds and leaves a note in ofx_last_error).  A pure decision,
 * exported for the host-logic tests.  The cross-GPU path itself has never executed: no multi-GPU box was available in any round. */
int ofx_staging_route(int ctx_device, int mem_device, int can_access_peer);

/* ---- Horn-Schunck pyramidal (replace src/horn_schunck.h:15-48) --------------------------------*/
int ofx_hs_single_scale(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v,
                        int nx, int ny, double alpha, int warps, double TOL, int maxiter, int verbose);
int ofx_hs_pyramidal(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v,
                     int nx, int ny, double alpha, int nscales, double zfactor, int warps,
                     double TOL, int maxiter, int verbose);

/* Device-resident lockstep groups / batches of the SOR solvers, the counterparts of ofx_tvl1_group_dev and
 * ofx_tvl1_batch_dev (same pointer layout: n_pairs device images of the context's storage precision in, n_pairs
 * .flo payloads of nx*ny interleaved (u,v) float32 out).  The pairs of a group share every launch of the windowed
 * exact sweeps (blockIdx.z = pair) -- a lone solve is a latency chain of thousands of dependent steps with little
 * work each -- while every pair keeps its own error slots, snapshots, sweep counts and stopping test: each flow is
 * bit-identical to the one ofx_hs_pyramidal / ofx_brox_spatial compute for that pair alone.  Groups need the
 * default option sor_exact = 1 or the tile sweeps of sor_exact = 0.  The group size of the batch calls is option "lockstep" of ctxs[0] if > 0, else
 * as large as possible (<= 16), evened out over the contexts. */
int ofx_hs_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2, void *const *d_flo,
                     int nx, int ny, double alpha, int nscales, double zfactor, int warps, double TOL, int maxiter,
                     ofx_stats *stats_out);
int ofx_hs_batch_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                     void *const *d_flo, int n_pairs, int nx, int ny, double alpha, int nscales, double zfactor,
                     int warps, double TOL, int maxiter, double *work_pix_iters);

/* classic Horn-Schunck (replace src/horn_schunck.h:7-8, src/horn_schunck_classic.cpp:125-149): niter Jacobi
 * iterations from a zero flow; a / b are the two images, w x h */
int ofx_hs_classic(ofx_ctx *ctx, const double *a, const double *b, double *u, double *v, int w, int h, int niter,
                   double alpha);

/* ---- Brox spatial (replace src/brox_optic_flow.h:19-33) ---------------------------------------*/
int ofx_brox_spatial(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v,
                     int nxx, int nyy, double alpha, double gamma, int nscales, double nu,
                     double TOL, int inner_iter, int outer_iter, int verbose);

int ofx_brox_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2, void *const *d_flo,
                       int nxx, int nyy, double alpha, double gamma, int nscales, double nu, double TOL,
                       int inner_iter, int outer_iter, ofx_stats *stats_out);
int ofx_brox_batch_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                       void *const *d_flo, int n_pairs, int nxx, int nyy, double alpha, double gamma, int nscales,
                       double nu, double TOL, int inner_iter, int outer_iter, double *work_pix_iters);

/* ---- SOR warm start: a flow to start Horn-Schunck and Brox from, and their video chains ---------------------------
 * The start of a pair is a .flo payload P as every solver writes it: nx * ny interleaved (u, v) float32, 8-byte aligned.  It
 * enters exactly as the TV-L1 warm start does (above; restated in tests/sor_warm_ref.py), with z = zfactor for Horn-Schunck
 * and z = nu for Brox:
 *   W_0 = ((double) P.u, (double) P.v), a component that is not finite (NaN, +-Inf) taken as 0.0;
 *   W_s = zoom_out(W_{s-1}, z) * z for s = 1 .. nscales - 1, per component, in double storage and arithmetic whatever the
 *         context's precision -- the mirror of the `*= 1.0 / zfactor` of src/horn_schunck_pyramidal.cpp:345-352 and of the
 *         1 / nu of src/brox_optic_flow_spatial.cpp:529-535;
 *   the flow of the coarsest level is W_{nscales-1}, rounded once to the storage type, in place of the reference's zeros.
 * Everything after the start is the driver of ofx_hs_group_dev / ofx_brox_group_dev, unchanged, under every setting of the
 * options sor_exact, sor_fuse, sor_lds and sor_tile: the start does not depend on the sweep order.  A NULL table is the plain
 * entry itself, a NULL entry is a zero start, and an all-zero payload gives the plain entry's payload, sweep table and, in
 * exact mode, stopping values bit for bit.  d_flo_init[g] == d_flo[g] is allowed: the start is consumed before any payload is
 * written.  Warm and cold pairs may share a group; each pair gets what the same call computes for that pair alone.  Frames are
 * read under "input" / "input_pitch"; a start that is not on the context's GPU is staged as ofx_tvl1_batch_dev stages its
 * buffers.
 * Refusals, before any work, nothing written, the reason in ofx_last_error: those of the plain entries; a start pointer that is
 * not 8-byte aligned (OFX_ERR_ARG, its pair index named); OFX_ERR_SIGMA as the image pyramid gives it (same levels, same sigma).
 * Out of scope: a start for ofx_robust_expo_*, ofx_brox_temporal_* and ofx_tvl1occ_*, for the host-plane entries
 * (ofx_hs_pyramidal, ofx_brox_spatial; ofx_hs_single_scale has always read u and v as its start), and bidirectional SOR entries.
 *
 * The batch entries take the same table after dI2 and keep the grouping rule of ofx_hs_batch_dev / ofx_brox_batch_dev (the
 * start's scratch comes from the group's workspace and does not enter the group size).  Groups run concurrently: a start may be
 * the pair's own slot of d_flo, not another pair's; the starts' refusals are raised for the whole batch before any group runs,
 * the pair named by its index in the batch. */
int ofx_hs_group_init_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2,
                          const void *const *d_flo_init, void *const *d_flo, int nx, int ny, double alpha, int nscales,
                          double zfactor, int warps, double TOL, int maxiter, ofx_stats *stats_out);
int ofx_hs_batch_init_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                          const void *const *d_flo_init, void *const *d_flo, int n_pairs, int nx, int ny, double alpha,
                          int nscales, double zfactor, int warps, double TOL, int maxiter, double *work_pix_iters);
int ofx_brox_group_init_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2,
                            const void *const *d_flo_init, void *const *d_flo, int nxx, int nyy, double alpha, double gamma,
                            int nscales, double nu, double TOL, int inner_iter, int outer_iter, ofx_stats *stats_out);
int ofx_brox_batch_init_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                            const void *const *d_flo_init, void *const *d_flo, int n_pairs, int nxx, int nyy, double alpha,
                            double gamma, int nscales, double nu, double TOL, int inner_iter, int outer_iter,
                            double *work_pix_iters);
/* The SOR video chains, with the layout of ofx_tvl1_sequence_group_dev: n_seq (1..16) device-resident sequences of n_frames >= 2
 * frames, sequence q = the frames dF[q * n_frames + t] and the payloads d_flo[q * (n_frames - 1) + t].  Step t solves the pairs
 * (F[q][t], F[q][t + 1]) of all sequences as one lockstep group: step 0 cold with nscales_first scales and warps_first warps
 * (Brox: outer_first outer iterations), step t > 0 from d_flo[q][t - 1] with nscales_next and warps_next (outer_next) -- these
 * loops run a fixed count whatever the start, so a warm step may be given fewer.  The payload of the step before is on the
 * device already: no host round trip between steps.  Each payload is bit for bit what the chained ofx_*_group_init_dev calls
 * write; consecutive steps do not share a frame's pyramid (image_normalization_2 works on a pair).  stats_out: NULL or
 * n_seq * (n_frames - 1) records, laid out like d_flo.  Both pyramids are validated before any work.  Frames and payloads
 * that are not on the context's GPU (host arrays: the front-ends' route) are staged step by step as ofx_tvl1_batch_dev stages
 * its buffers, at the cost of the copies.  Refusals as the group entries, and OFX_ERR_ARG for n_seq outside 1..16,
 * n_frames < 2, a payload that is NULL or not 8-byte aligned. */
int ofx_hs_sequence_group_dev(ofx_ctx *ctx, int n_seq, int n_frames, const void *const *dF, void *const *d_flo, int nx, int ny,
                              double alpha, int nscales_first, int nscales_next, double zfactor, int warps_first, int warps_next,
                              double TOL, int maxiter, ofx_stats *stats_out);
int ofx_brox_sequence_group_dev(ofx_ctx *ctx, int n_seq, int n_frames, const void *const *dF, void *const *d_flo, int nxx,
                                int nyy, double alpha, double gamma, int nscales_first, int nscales_next, double nu, double TOL,
                                int inner_iter, int outer_first, int outer_next, ofx_stats *stats_out);

/* ---- robust_expo_methods (replace src/robust_expo_methods.h:21-38) -----------------------------------*/
/* Brox's scheme with an image-driven weight in the smoothness term: method_type 1 = exp(-lambda |grad I1|), 2 = the same
 * + 0.001, 3 = lambda chosen per pixel from alpha and the gradient distribution.  The reference's argument order.
 * I1, I2: nxx * nyy * nzz doubles, channels interleaved (element (i * nxx + j) * nzz + k); u, v: nxx * nyy.
 * nzz = 1: any number of scales.  nzz = 2 .. OFX_REXPO_MAX_CHANNELS: nscales must be 1 (OFX_ERR_ARG otherwise): the
 * reference's colour pyramid reads beyond its scratch copy (zoom.cpp:96-118), its colour solver at one scale is defined.
 * Other nzz: OFX_ERR_ARG.  Levels smaller than 3x3 and option sor_exact != 1: OFX_ERR_ARG; a level too small for the zoom
 * Gaussian: OFX_ERR_SIGMA; all found before any work.  One driver serves this entry and ofx_robust_expo_pyramid.
 * Kept quirks of the source:
 *  - the presmoothing is gaussian(I, nxx, nyy, nzz, 0.8) against (I, xdim, ydim, sigma, boundary, window)
 *    (robust_expo_methods.cpp:497-498): sigma = nzz, the DIRICHLET boundary, and the buffer taken for one nxx x nyy plane, so
 *    for nzz > 1 only the first nxx * nyy elements of the interleaved image are smoothed;
 *  - alpha * nzz is truncated to an int (:527);
 *  - the SOR stopping value is sqrt(error / (nx ny nz)) (:400);
 *  - for nzz > 1 the first row of the derivative arrays: centered_gradient and the 3x3 masks address it by the column alone
 *    (operators.cpp:176, :363-364), so elements 1 .. nx - 2 hold the last channel's stencil of "column k", the corner
 *    elements their own values and the rest of the row is never written -- 0 here, as in the reference built with zeroed
 *    arrays, which is the build this library is checked against; and the right-hand tap of the masks in the last row is
 *    read one ELEMENT further instead of one pixel (:189).
 * SOR sweeps run in the reference's order (windowed exact schedule, option sor_exact = 1); sweep counts equal to the
 * reference's on one thread, flows to 1e-11 (the order of the stopping sum). */
#define OFX_REXPO_MAX_CHANNELS 4
int ofx_robust_expo(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nxx, int nyy, int nzz,
                    int method_type, double alpha, double gamma, double lambda, int nscales, double nu, double TOL,
                    int inner_iter, int outer_iter, int verbose);
/* Colour on a pyramid: ofx_robust_expo's argument list, any nzz in 1 .. OFX_REXPO_MAX_CHANNELS with any nscales >= 1.
 * The REFERENCE's: the multiscale driver (robust_expo_methods.cpp:482-566) step for step with every quirk listed above, and
 * the level solver.  The IPOL ORIGINAL's: the one call that builds level s from level s - 1, ofx_zoom_out_channels
 * (3rdparty/ipoldfmethods_20160307/zoom.h:45-85) in place of the reference's zoom_out_color (zoom.cpp:85-125), which reads
 * beyond its scratch copy for nzz > 1.  ofx_robust_expo and ofx_zoom_out_color keep the reference's names and keep refusing
 * there; this entry is an extra under a name of its own.
 * In f64 storage nzz = 1 gives ofx_robust_expo's result at the same nscales bit for bit (in f32 storage the one-channel entry
 * rounds the planes to float BEFORE the normalisation, this one after it, so the two may differ there); nscales = 1 gives
 * ofx_robust_expo's colour result bit for bit in either storage.  Against the reference's entry points composed the same way on one thread: equal sweep counts, flows to 1e-11.
 * Errors, all found before any work (no flow is written): OFX_ERR_ARG as ofx_robust_expo, and for a level smaller than 3x3;
 * OFX_ERR_SIGMA for a level too small for the zoom Gaussian.  ofx_get_stats: the level sizes, sweeps and stopping values per
 * level and solve; with verbose the reference's "Scale: s" lines. */
int ofx_robust_expo_pyramid(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nxx, int nyy, int nzz,
                            int method_type, double alpha, double gamma, double lambda, int nscales, double nu, double TOL,
                            int inner_iter, int outer_iter, int verbose);
/* ofx_robust_expo_pyramid for the pairs of a lockstep group / of a batch, on device-resident images; the conventions of
 * ofx_brox_group_dev and ofx_brox_batch_dev: n_pairs in 1..16 for a group, the pairs of a group share every launch (the pair is
 * a grid dimension) and each keeps its own stopping test; dI1, dI2, d_flo are arrays of n_pairs device pointers; stats_out is
 * NULL or n_pairs records; the call is asynchronous on the context's stream (ofx_ctx_synchronize).  A batch is cut into groups
 * by the rule of the other SOR batches (option "lockstep" of ctxs[0], else as large as possible and evened out over the
 * contexts), group q runs on ctxs[q % n_ctx] on a worker thread of its own, work_pix_iters (NULL or n_pairs doubles) receives
 * sum sweeps * nx_s * ny_s per pair, and n_pairs = 0 is OFX_OK.
 * dI1[g], dI2[g]: nxx * nyy * nzz elements of the context's storage precision (double | float), channels interleaved, element
 * (i * nxx + j) * nzz + k.  d_flo[g]: the .flo payload, nxx * nyy interleaved (u, v) float32.
 * Every pair gets what ofx_robust_expo_pyramid computes for that pair alone -- any nzz in 1 .. OFX_REXPO_MAX_CHANNELS at any
 * nscales >= 1, with every quirk listed above.  In f64 storage the payload of pair g is bit-identical to float32 of the flow
 * that entry returns for the pair, and the pair's sweep table and stopping values equal that solve's.  In f32 storage the same
 * holds whenever the input values are exactly representable in float: the lone entry receives doubles and rounds to float AFTER
 * the normalisation, the device images here are float already, and the two coincide on such inputs (8-bit or 16-bit image
 * data, for instance); on other inputs the group sees the rounded images.
 * (The stopping values depend on options sor_window / sor_rows in their last bits: the stopping sum is associated along the
 * window geometry.  The groups therefore keep the lone entry's defaults, 8 steps and 64 rows, also where Brox groups of >= 4
 * pairs switch to 4 steps and 125 rows, and the equality holds whenever both calls run under the same options.  One limit, of
 * the lone entry as well: the sum of a sweep is kept in 64 shards, one per wave of a row block, so with more than 16 row
 * blocks -- levels of more than 1024 rows at the default 64 rows per block -- two blocks add atomically into one shard and
 * the last bits of a stopping value are not reproducible from run to run, for two lone solves as little as for a group.)
 * The `expo` weights of a level are evaluated on the host (libm's exp / log, std::sort), all pairs of the group from one
 * download, on up to 16 / concurrency threads per context; results do not depend on the thread count.
 * Errors, all found before any work (no d_flo element is written): those of ofx_robust_expo_pyramid -- nzz, method_type,
 * negative iteration counts, option sor_exact != 1, a level smaller than 3x3 (OFX_ERR_ARG), a level too small for the zoom
 * Gaussian (OFX_ERR_SIGMA) -- and those of ofx_brox_group_dev: n_pairs outside 1..16, a NULL array or a NULL pointer at pair g.
 * Option "profile": pyramid_ms = the group's pyramid phase (normalisation to the last level of all 2 n_pairs pyramids), in every
 * record of the group; iter_ms[s] = the SOR windows of level s on the HOST's clock, between two drains of the stream that only
 * this entry adds under "profile": wall time with the polls of the stopping test, not kernel time (the lone robust_expo
 * entries leave iter_ms 0); ofx_ctx_expo_host_ms = the host part of the expo stage. */
int ofx_robust_expo_group_dev(ofx_ctx *ctx, int n_pairs, const void *const *dI1, const void *const *dI2, void *const *d_flo,
                              int nxx, int nyy, int nzz, int method_type, double alpha, double gamma, double lambda,
                              int nscales, double nu, double TOL, int inner_iter, int outer_iter, ofx_stats *stats_out);
int ofx_robust_expo_batch_dev(ofx_ctx *const *ctxs, int n_ctx, const void *const *dI1, const void *const *dI2,
                              void *const *d_flo, int n_pairs, int nxx, int nyy, int nzz, int method_type, double alpha,
                              double gamma, double lambda, int nscales, double nu, double TOL, int inner_iter, int outer_iter,
                              double *work_pix_iters);
/* milliseconds the host spent evaluating `expo` (without the transfers), all levels, during the LAST API call on this context:
 * every solver and operator entry zeroes it on entry (the ofx_ctx_* calls and ofx_set_option do not), so it is non-zero only
 * straight after a robust_expo entry
 * (ofx_robust_expo, _single_scale, _pyramid, _group_dev; after ofx_robust_expo_batch_dev each context holds its last group's).
 * Measured always; NULL reads 0. */
double ofx_ctx_expo_host_ms(const ofx_ctx *ctx);
/* The reference's single-scale overload (robust_expo_methods.cpp:162-178, declared in none of its headers): the solver of one
 * level with no normalisation, no presmoothing and alpha as given; u, v are READ as the initial flow and overwritten with
 * the result -- what a caller needs to run colour on a pyramid of their own.  nz in 1 .. OFX_REXPO_MAX_CHANNELS, images
 * interleaved as above.  number_of_threads is accepted for the argument order's sake and ignored.  ofx_get_stats: scale 0. */
int ofx_robust_expo_single_scale(ofx_ctx *ctx, const double *I1, const double *I2, double *u, double *v, int nx, int ny, int nz,
                                 int method_type, double alpha, double gamma, double lambda, double TOL, int inner_iter,
                                 int outer_iter, int number_of_threads, int verbose);

/* ---- Brox temporal (replace src/brox_optic_flow.h:41-55) ---------------------------*/
/* I: `frames` images of nx*ny, frame-major; u, v: frames - 1 flow fields (u[f] takes frame f to frame f + 1).
 * frames <= 2 is an error ("The method needs more than two frames", brox_optic_flow_temporal.cpp:537-541: the
 * reference prints that and returns).  SOR sweeps run in the reference's order (windowed exact schedule) by default; option
 * sor_exact = 0 sweeps in the 3-D red-black order described there (AEPE < 1e-4 against the reference's order, several times
 * faster), sor_fuse picks its kernel.  Levels below 3x3 are OFX_ERR_ARG in every mode. */
int ofx_brox_temporal(ofx_ctx *ctx, const double *I, double *u, double *v, int nxx, int nyy, int frames,
                      double alpha, double gamma, int nscales, double nu, double TOL, int inner_iter,
                      int outer_iter, int verbose);

/* The same solve on a device-resident sequence.  dF[k], k < frames: frame k, nxx * nyy elements of the context's storage type
 * (double for OFX_F64, float for OFX_F32), aligned to the element; the frames need not be contiguous nor distinct (a still
 * frame may be passed twice).  d_flo[f], f < frames - 1: the .flo payload of the flow from frame f to f + 1, nxx * nyy
 * interleaved (u, v) float32 pairs, 8-byte aligned (stored as float2): bit for bit (float) of what ofx_brox_temporal returns on
 * the same values under equal options (sor_exact, sor_fuse: the entries share the level solver).  3 <= frames <= OFX_BROXT_MAX_FRAMES (the frames reach the kernels through a by-value pointer table).
 * Asynchronous on the context's stream: the stopping tests are resolved on return, the payloads are complete once the stream
 * is synchronised.  ofx_get_stats is filled as by ofx_brox_temporal.
 * The stopping values of the exact mode (ofx_stats.error, for this entry and ofx_brox_temporal alike) are the same in every run while
 * (frames - 1) * row blocks of 64 rows * waves per block <= 64 on every level: each then adds into a shard of its own; on larger
 * levels several workgroups add atomically into one shard and the last bits may depend on the order in which they arrive.
 * Every error is found before any work and no byte of d_flo is written: what ofx_brox_temporal rejects (frames <= 2, images
 * or a level below 3x3, negative iteration counts, OFX_ERR_SIGMA when a Gaussian of the pyramid does not fit its level), more
 * than OFX_BROXT_MAX_FRAMES frames, a NULL array, a NULL or misaligned pointer (its index is in ofx_last_error). */
#define OFX_BROXT_MAX_FRAMES 32
int ofx_brox_temporal_dev(ofx_ctx *ctx, int frames, const void *const *dF, void *const *d_flo, int nxx, int nyy, double alpha,
                          double gamma, int nscales, double nu, double TOL, int inner_iter, int outer_iter);

/* A LOCKSTEP GROUP of n_seq (1 .. 16) sequences of `frames` frames each through the same kernel launches on one context: dF holds
 * n_seq * frames pointers (sequence q at dF + q * frames), d_flo n_seq * (frames - 1) (sequence q at d_flo + q * (frames - 1)),
 * frames and payloads as for ofx_brox_temporal_dev; frames may be shared between sequences or repeated within one.  Every
 * sequence keeps its own normalisation (image_normalization_1 over that sequence alone), stopping test, sweep counts, snapshots
 * and, under sor_exact = 0, ping-pong phase: sequence q's payload is bit for bit what ofx_brox_temporal_dev writes for it
 * alone on a context with the same options (sor_exact = 1, 2 or 0, every sor_fuse, both storage types), and its sweep table
 * [scale][solve] is the lone solve's.  In the exact mode its stopping values are the lone solve's too: a group keeps the lone
 * entry's window geometry (8 steps per launch, 64 rows per block; options sor_window / sor_rows override both entries alike)
 * and its windows cut every sweep by the sweep's number in the solve, so the stopping sum is associated as alone.  (Every
 * frame, row block and wave of a sweep adds into a shard of its own while (frames - 1) * row blocks * waves per block <= 64;
 * on larger levels several workgroups add atomically into one shard, for the lone entry as for a group, and the last bits of
 * a stopping value may then depend on the order in which they arrive.)
 * What a group shares is every launch: normalisation, presmoothing and the pyramid over all n_seq * frames planes (as many
 * per launch as the by-value pointer tables hold), the per-level kernels and the SOR windows / tile sweeps with the sequence in
 * the grid.  A sequence that has stopped drops out of the windows that follow.
 * stats_out: NULL or n_seq records, each filled as ofx_brox_temporal_dev fills the context's; ofx_get_stats holds sequence 0's
 * afterwards.  Asynchronous on the context's stream like ofx_brox_temporal_dev.  Memory: n_seq times the per-sequence figure
 * given for the batch entry below.
 * Every error is found before any work and no byte of any payload is written: what ofx_brox_temporal_dev rejects, checked for
 * every sequence (sequence and frame index in ofx_last_error), n_seq outside 1 .. 16, and a group of 2^31 voxels (nxx * nyy *
 * frames * n_seq) or more. */
int ofx_brox_temporal_group_dev(ofx_ctx *ctx, int n_seq, int frames, const void *const *dF, void *const *d_flo, int nxx, int nyy,
                                double alpha, double gamma, int nscales, double nu, double TOL, int inner_iter, int outer_iter,
                                ofx_stats *stats_out);

/* n_seq independent sequences of `frames` frames each: dF holds n_seq * frames pointers (sequence q at dF + q * frames), d_flo
 * n_seq * (frames - 1) (sequence q at d_flo + q * (frames - 1)).
 * Option "lockstep" of ctxs[0] = L >= 2 (opt-in): lockstep groups of L consecutive sequences (a last, smaller group is normal),
 * group q through ofx_brox_temporal_group_dev on ctxs[q % contexts at work], EVERY context under ctxs[0]'s sor_exact / sor_fuse
 * for the call (also when the memory rule or n_seq leaves groups of one); the payloads are bit for bit the lone entry's under those options.  The memory rule below then counts the
 * group size times one sequence per context: L is reduced first until contexts at work x L sequences fit the budget, then the
 * number of contexts; OFX_ERR_NOMEM before any work if one sequence does not fit.
 * Option "lockstep" of ctxs[0] = 0 or 1 (default): sequence q is solved by ofx_brox_temporal_dev on
 * ctxs[q % n_ctx], one worker thread and stream per context; the solves are independent (no lockstep).  Each context solves
 * under its OWN options: the payloads are bit for bit the host entry's when sor_exact / sor_fuse are equal on every context.  All contexts on ONE
 * device and of one precision; option "concurrency" of the contexts is raised to the number at work for the call.  Returns when
 * every payload is complete, with the first failing status.  work_pix_iters: NULL or one double per sequence
 * (ofx_stats.work_pix_iters of its solve).
 * Memory: one sequence takes, in elements of the storage type per pixel of a pyramid level, `frames` (the level's images) +
 * 27 (frames - 1) (the level's twelve work arrays: 3 scalar, 6 pair and 3 quadruple planes per flow field) + 2 B (frames - 1)
 * (B snapshot planes of pairs, B = option "sor_batch" or 64), and 2 * frames full-size planes of pyramid scratch; plus 5 %.
 * Under option "mem_budget" of ctxs[0] (default: half of the free device memory) only as many contexts work at once as
 * sequences fit, sequence q then on ctxs[q % that number]; if not even one fits: OFX_ERR_NOMEM before any work.
 * Errors as ofx_brox_temporal_dev, found for every sequence before any work, and: n_seq < 1, n_ctx < 1, a NULL context,
 * contexts on different devices or of different precision. */
int ofx_brox_temporal_batch_dev(ofx_ctx *const *ctxs, int n_ctx, int n_seq, int frames, const void *const *dF,
                                void *const *d_flo, int nxx, int nyy, double alpha, double gamma, int nscales, double nu,
                                double TOL, int inner_iter, int outer_iter, double *work_pix_iters);

/* ---- colour operators (replace src/bicubic_interpolation.h:66-75, src/utils.h:39-96) -----------------*/
/* bicubic_interpolation_warp_color: nz interleaved channels, every sample through bicubic_interpolation_at_color */
int ofx_bicubic_warp_color(ofx_ctx *ctx, const double *input, const double *u, const double *v, double *output,
                           int nx, int ny, int nz, int border_out);
/* image_normalization_2_color: per channel joint min / max of both images; `size` = number of ELEMENTS (pixels * nz,
 * a multiple of nz: the reference reads past its arrays otherwise), copy when max == min */
int ofx_image_normalization_2_color(ofx_ctx *ctx, const double *I1, const double *I2, double *I1n, double *I2n,
                                    int size, int nz);
/* image_normalization_3: joint min / max of three images, IN PLACE, no test for max == min (as the reference) */
int ofx_image_normalization_3(ofx_ctx *ctx, double *I0, double *I1, double *I2, int size);
int ofx_image_normalization_4(ofx_ctx *ctx, const double *I_1, const double *I0, const double *I1, const double *filtI0,
                              double *I_1n, double *I0n, double *I1n, double *filtI0n, int size);

/* ---- building blocks of TV-L1 with occlusions ---------------------------------------------------------------
 * The reference PROGRAM (tvl1occflow) is not reproducible by any implementation: Solver_wrt_chi reads its dual variable
 * uninitialised and Solver_wrt_u keeps its dual variables in function-local statics across calls
 * (src/tvl1occflow_solvers.cpp:161-186,239-263).  Its functions are deterministic once that state is explicit: */
/* me_median_filtering (src/utils.h:10, src/utils.cpp:150-213): wsize x wsize median, in place; wsize <= 9 */
int ofx_me_median_filtering(ofx_ctx *ctx, double *in, int nx, int ny, int wsize);
/* Solver_wrt_v (src/tvl1occflow_solvers.h, src/tvl1occflow_solvers.cpp:56-147); same argument order */
int ofx_solver_wrt_v(ofx_ctx *ctx, const double *u1, const double *u2, double *v1, double *v2, const double *chi,
                     const double *I1wx, const double *I1wy, const double *I_1wx, const double *I_1wy,
                     const double *rho1_c, const double *rho3_c, double *Vfwd_1, double *Vfwd_2, double *Vbck_1,
                     double *Vbck_2, const double *grad1, const double *grad3, double alpha, double theta, double lambda,
                     int nx, int ny);
/* Scalar_ROF_BoxCellCentered (src/tvl1occflow_tv_rof_box.h:52-55): nIter x { alfa from u; one in-place box-relaxation sweep in
 * the reference's cell order (executed on hyperplanes, bit-identical); u = lambda f + lambda div P }.  u: in = seed, out =
 * result; initialP1 / initialP2: in/out dual values on the south / east cell edges.  nx, ny >= 2. */
int ofx_scalar_rof_box_cell_centered(ofx_ctx *ctx, double *u, const double *f, double *initialP1, double *initialP2,
                                     const double *g_function, double lambda, double omega, int nx, int ny, int nIter);
/* Solver_wrt_u (src/tvl1occflow_solvers.cpp:150-216); the reference's argument order, followed by its four dual planes as
 * explicit in/out state (the reference keeps them in function-local statics, zeroed when the image width changes) and the
 * iteration count per flow component (the reference's MAX_ITERATIONS_U = 10) */
int ofx_solver_wrt_u(ofx_ctx *ctx, double *u1, double *u2, const double *v1, const double *v2, const double *chi,
                     const double *g, double theta, double beta, int nx, int ny, double *p11, double *p12, double *p21,
                     double *p22, int n_iter);
/* Solver_wrt_chi (src/tvl1occflow_solvers.cpp:218-337); the reference's argument order, followed by the dual variable
 * (eta1, eta2) as explicit in/out state -- zero it for what the reference computes on a zero-filled heap -- and the
 * iteration count (the reference's MAX_ITERATIONS_CHI = 100) */
int ofx_solver_wrt_chi(ofx_ctx *ctx, const double *u1, const double *u2, double *chi, const double *I1wx,
                       const double *I1wy, const double *I_1wx, const double *I_1wy, const double *rho1_c,
                       const double *rho3_c, const double *Vfwd_1, const double *Vfwd_2, const double *Vbck_1,
                       const double *Vbck_2, const double *g, double lambda, double theta, double alpha, double beta,
                       double tau_chi, double tau_eta, int nx, int ny, double *eta1, double *eta2, int n_iter);

/* The whole TV-L1-with-occlusions solve (replaces Dual_TVL1_optic_flow_multiscale, src/tvl1occflow.h / tvl1occflow.cpp:337-481;
 * the single-scale loop :144-329 runs on the device per level): I_1 / I0 / I1 = previous, current, next frame, filtI0 = the image
 * g = 1 / (1 + 0.05 |grad filtI0|) is taken from (the CLI passes I0 when no smoothed image is given); u1 / u2 / chi are outputs
 * (chi thresholded at 0.75 to {0, 1} as the reference does).  Host planes of nxx * nyy doubles; everything in between --
 * pyramids, warps, the three sub-solvers, the median, the stopping test -- stays on the device.  Double arithmetic and storage
 * whatever the context's precision.  The reference keeps the dual variables of Solver_wrt_u / Solver_wrt_chi in statics it
 * allocates uninitialised once per level; this entry point implements the zero-initialised reading.
 * ofx_get_stats: iters[scale][warp] = outer iterations, error = last L2 error. */
int ofx_tvl1occ_multiscale(ofx_ctx *ctx, const double *I_1, const double *I0, const double *I1, const double *filtI0, double *u1,
                           double *u2, double *chi, int nxx, int nyy, double lambda, double alpha, double beta, double theta,
                           int nscales, double zfactor, int warps, double epsilon, int verbose);
/* n_triples independent solves (e.g. the frames of a sequence) in lockstep groups of consecutive triples: the triples of a group
 * share every kernel launch of a context, group q runs on context q mod n_ctx (one host thread and one stream per context, all on
 * one device).  The group size and its memory rule are ofx_tvl1occ_triples_dev's below, the ONE rule of every tvl1occ batch entry:
 * the table is built from the host pointers of the four roles -- equal ADDRESS means one plane, nothing else about the arrays is
 * compared -- so D, a group's count of distinct planes, is 4 G for arrays that are all different, 3 G where filtI0 is I0, and
 * G + 2 for the consecutive triples of a sequence passed as the same arrays, each of which is uploaded and built once per group.
 * Every result is bit-identical to the triple solved alone.  Arrays of n_triples host pointers; host planes are dense doubles
 * whatever the contexts' "input" and "input_pitch" options say.  Both host entries find everything they reject before any work
 * (no output plane is written): sizes, nscales, warps, zfactor, theta, lambda, a coarsest level below 2x2, OFX_ERR_SIGMA for a
 * level too small for its Gaussian, OFX_ERR_NOMEM where one triple does not fit.  Returns the first failing status (detail text
 * on that context). */
int ofx_tvl1occ_batch(ofx_ctx *const *ctxs, int n_ctx, int n_triples, const double *const *I_1, const double *const *I0,
                      const double *const *I1, const double *const *filtI0, double *const *u1, double *const *u2,
                      double *const *chi, int nxx, int nyy, double lambda, double alpha, double beta, double theta, int nscales,
                      double zfactor, int warps, double epsilon);

/* The same solve over a DEVICE-RESIDENT SEQUENCE of frames: the counterparts of the *_group_dev / *_batch_dev entries of the
 * other solvers, with the sequence as the unit of work.  n_frames frames give n_frames - 2 triples, triple t =
 * (F[t], F[t + 1], F[t + 2]), and each triple gets what ofx_tvl1occ_multiscale(F[t], F[t + 1], F[t + 2], filtI0 = F[t + 1])
 * computes on those values -- the front-end's default when no smoothed image is given -- with its own stopping test and
 * outer-iteration counts.
 *   dF[k]     n_frames device pointers, nxx * nyy elements of the context's storage precision each (double for OFX_F64, float for
 *             OFX_F32), aligned to that element.  They are converted exactly to double; arithmetic and internal storage stay
 *             double, as ofx_tvl1occ_multiscale promises.
 *   d_flo[t]  n_frames - 2 device pointers: the .flo payload, nxx * nyy interleaved (u1, u2) float32, bit-identical to (float) of
 *             the lone entry's u1, u2.  Stored as float2 like every payload of the library: 8-byte aligned.
 *   d_occ[t]  n_frames - 2 device pointers: nxx * nyy bytes, 255 where the thresholded chi is 1, else 0 -- the bytes tvl1occflow
 *             writes as its occlusion map.  No alignment needed.
 * What is shared: no normalisation is applied to the images (the reference overwrites it, tvl1occflow.cpp:382-395), so the
 * presmoothed pyramid of a frame and its centred gradients depend on that frame alone.  A group keeps every frame once per level;
 * a sequence is the table of triples (t, t + 1, t + 2, filt = -1) of ofx_tvl1occ_triples_dev below, and the roles a frame plays in
 * consecutive triples (I1, then I0 and filtI0, then I_1) are indices into that array -- the one layout of every tvl1occ entry.  The
 * pyramid, the gradients, the zoom-in of (u1, u2, chi) and the results take one launch per stage for the whole group.
 * ofx_tvl1occ_sequence_group_dev: one lockstep group, n_frames in 3 .. 18.  stats_out: NULL or n_frames - 2 records (level sizes,
 * iters[scale][warp], error, work_pix_iters, total_ms as ofx_tvl1occ_multiscale fills them).  Asynchronous on the context's stream
 * like the other *_group_dev entries: the stopping tests are resolved on return, the results are complete once the stream is
 * synchronised.
 * ofx_tvl1occ_sequence_dev: any n_frames >= 3 on one or several contexts of ONE device and one precision.  The triples are cut
 * into groups of G consecutive triples, group q = frames q G .. q G + cnt + 1 on ctxs[q % n_ctx], a worker thread per context; the
 * two frames neighbouring groups share are built by both.  G = the smallest of: option "lockstep" of ctxs[0] if positive; 16; what
 * the memory rule allows; ceil(triples / n_ctx).  The memory rule is ofx_tvl1occ_triples_dev's with D = G + 2, under option
 * "mem_budget" (default: half of the free device memory), divided by n_ctx: a group of G triples takes, in doubles, G + 2 frames
 * and 3 G result planes per pyramid level, 2 (G + 2) + 27 G full-size planes and 13 G hyperplane-major ones, plus 5 %; if one
 * triple does not fit: OFX_ERR_NOMEM.  work_pix_iters: NULL or one double per triple.  Returns when every payload is complete.
 * Errors, all found before any work (no byte of d_flo / d_occ is written): everything ofx_tvl1occ_multiscale rejects (sizes,
 * nscales, warps, zfactor, theta, lambda, a coarsest level below 2x2), a pyramid that cannot be built (OFX_ERR_SIGMA: a level too
 * small for its Gaussian), n_frames < 3, n_frames > 18 for the group entry, a NULL array, a NULL or misaligned pointer at index k,
 * contexts on different devices or of different precision.
 * Device-resident triples that are not consecutive frames of one sequence, and a separate filtI0, go through
 * ofx_tvl1occ_triples_group_dev / ofx_tvl1occ_triples_dev below. */
int ofx_tvl1occ_sequence_group_dev(ofx_ctx *ctx, int n_frames, const void *const *dF, void *const *d_flo,
                                   void *const *d_occ, int nxx, int nyy, double lambda, double alpha, double beta,
                                   double theta, int nscales, double zfactor, int warps, double epsilon,
                                   ofx_stats *stats_out);
int ofx_tvl1occ_sequence_dev(ofx_ctx *const *ctxs, int n_ctx, int n_frames, const void *const *dF, void *const *d_flo,
                             void *const *d_occ, int nxx, int nyy, double lambda, double alpha, double beta, double theta,
                             int nscales, double zfactor, int warps, double epsilon, double *work_pix_iters);

/* The same solve over INDEXED TRIPLES of a table of device-resident planes: the backward triple (F[t + 1], F[t], F[t - 1]), strided
 * triples (F[t - s], F[t], F[t + s]), a g-image of the caller's own (the I0_Smoothed argument of tvl1occflow) -- any combination
 * of planes.  Triple k gets what ofx_tvl1occ_multiscale(dF[prev], dF[cur], dF[next], filtI0 = dF[filt]) computes on those values,
 * bit for bit, with its own stopping test and outer-iteration counts.
 *   dF[i]     the frame table, n_frames >= 1 device pointers as above (nxx * nyy elements of the context's storage precision,
 *             aligned to the element, converted exactly to double).  A g-image of the caller's own is simply another plane of the
 *             table.  Only planes that some triple references are dereferenced: unreferenced entries may be NULL.
 *   tr[k]     n_triples records of indices into the table; filt = -1 means cur.  Planes are told apart by INDEX, not by pointer:
 *             two indices with the same pointer are two planes.
 *   d_flo[k], d_occ[k]  n_triples payloads and maps as above (8-byte aligned | no alignment).
 * What is shared: as above, a plane's presmoothed pyramid and centred gradients depend on that plane alone, whatever role it plays
 * in whichever triple.  A group keeps each distinct referenced plane once per level and the roles of a triple are indices into
 * that array (a by-value table of 4 x 16 bytes, read by the two kernels that read images).  The host entries and the sequence
 * entries above are tables of this kind in front of the same group solve.
 * ofx_tvl1occ_triples_group_dev: one lockstep group, n_triples in 1 .. 16, hence at most 64 distinct planes: a group never fails
 * for having "too many frames".  stats_out: NULL or n_triples records, filled as the sequence group entry fills them.
 * Asynchronous on the context's stream in the same sense.
 * ofx_tvl1occ_triples_dev: any n_triples >= 1 (0: OFX_OK, nothing done) on one or several contexts of ONE device and one
 * precision.  Groups are G consecutive triples IN THE CALLER'S ORDER, group q on ctxs[q % n_ctx], a worker thread per context;
 * a plane that two groups share is built by both, so order the triples so that neighbours share frames (forward and backward
 * triple of one centre next to each other, centres in sequence order).  G = the smallest of: option "lockstep" of ctxs[0] if
 * positive; 16; ceil(n_triples / n_ctx); the largest G for which every group fits the memory rule under option "mem_budget"
 * (default: half of the free device memory) divided by n_ctx.  The memory rule, the one of every tvl1occ batch entry, with D the
 * group's own count of distinct planes: in doubles, D + 3 G planes per pyramid level, 2 D + 27 G full-size planes and 13 G
 * hyperplane-major ones, plus 5 %; if one triple does not fit: OFX_ERR_NOMEM.  work_pix_iters: NULL or one double per triple.
 * Returns when every payload is complete.
 * ofx_tvl1occ_triples_frames: the decision both entries build their tables with, pure host code (no context, no device).  Returns
 * D, the number of distinct referenced indices, or -OFX_ERR_ARG (n_frames < 1, an index outside 0 .. n_frames - 1 other than
 * filt = -1).  frames_out (NULL or room for 4 * n_triples): the indices in order of first appearance, scanning the triples in
 * order and the roles prev, cur, next, filt.  roles_out (NULL or [n_triples][4] bytes, n_triples <= 64): the position in
 * frames_out of role r of triple k, filt = -1 resolved to cur's position.
 * Errors, all found before any work (no byte of d_flo / d_occ is written): everything ofx_tvl1occ_sequence_group_dev rejects
 * (sizes, nscales, warps, zfactor, theta, lambda, a coarsest level below 2x2, OFX_ERR_SIGMA for a level too small for its
 * Gaussian), n_triples outside 1 .. 16 for the group entry, a NULL array, an index outside the table (ofx_last_error names the
 * triple and the role), a referenced plane that is NULL or misaligned, a NULL or misaligned result pointer, contexts on different
 * devices or of different precision. */
typedef struct ofx_occ_triple { int prev, cur, next, filt; } ofx_occ_triple;
int ofx_tvl1occ_triples_group_dev(ofx_ctx *ctx, int n_frames, const void *const *dF, int n_triples, const ofx_occ_triple *tr,
                                  void *const *d_flo, void *const *d_occ, int nxx, int nyy, double lambda, double alpha,
                                  double beta, double theta, int nscales, double zfactor, int warps, double epsilon,
                                  ofx_stats *stats_out);
int ofx_tvl1occ_triples_dev(ofx_ctx *const *ctxs, int n_ctx, int n_frames, const void *const *dF, int n_triples,
                            const ofx_occ_triple *tr, void *const *d_flo, void *const *d_occ, int nxx, int nyy, double lambda,
                            double alpha, double beta, double theta, int nscales, double zfactor, int warps, double epsilon,
                            double *work_pix_iters);
int ofx_tvl1occ_triples_frames(int n_frames, int n_triples, const ofx_occ_triple *tr, int *frames_out, unsigned char *roles_out);

#ifdef __cplusplus
}
#endif
#endif /* OFX_H */
