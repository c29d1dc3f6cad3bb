// ofx_pairs.h -- the entry layer of the solvers that take PAIRS of frames (TV-L1, Horn-Schunck, Brox): the ladder lockstep group
// -> group with a start per pair -> batch over several contexts -> video chain, each rung written once.  Private to libofx.so.
// What a solver brings: its parameters and their refusals, its pyramid driver and where its finest flow lies ("The
// pair-entry layer").  The chain walker and the frame span are ofx_group_plan.h's (no HIP); the group runner and the record
// shell are ofx_batch.h's.
#pragma once

#include "ofx_batch.h"
#include "ofx_ops.h"

// ---- staging ------------------------------------------------------------------------------------------------------------------
// Buffers that do not live on this context's GPU (a batch spread over several GPUs by ofx_tvl1_batch_dev, or host buffers: the
// front-ends' route) are staged through the arena, on the context's stream.  In: *out = p itself where it is local or NULL, else
// an arena buffer of `bytes` bytes -- filled from p (fill: what the solve reads) or left for the solve to write ...
static inline int ofx_stage_in(ofx_ctx *ctx, const void *p, size_t bytes, bool fill, void **out)
{
    *out = const_cast<void *>(p);
    if (!p || ofx_ptr_is_local(ctx, p)) return OFX_OK;
    char *stage;
    OFX_TRY(ofx_alloc(ctx, bytes, &stage));
    *out = stage;
    return fill ? ofx_copy_staged(ctx, stage, p, bytes) : OFX_OK;
}
// ... out: back into the caller's array where the solve wrote a stage
static inline int ofx_stage_out(ofx_ctx *ctx, void *p, const void *staged, size_t bytes)
{
    return staged != p ? ofx_copy_staged(ctx, p, staged, bytes) : OFX_OK;
}

// ---- the pair tables of a group -----------------------------------------------------------------------------------------------
// The buffers of a group as its solve uses them, with the format its frames come in.  A start that is not on this context's GPU
// is always read through a stage.  stage_all: so are the frames and the payloads -- every TV-L1 entry, and the video chains of
// all three solvers; the plain Horn-Schunck and Brox entries use the caller's frames and payloads in place, as they always did.
struct OfxPairIO {
    void *a[OFX_MAX_GROUP], *b[OFX_MAX_GROUP], *init[OFX_MAX_GROUP], *flo[OFX_MAX_GROUP];
    int kind;           // OFX_SRC_*: the context's "input" kind
    size_t pitch;       // bytes between the frames' rows, 0 = dense: a pitched frame keeps its pitch through a stage
};
static inline int ofx_pairs_stage(ofx_ctx *ctx, int G, const void *const *dA, const void *const *dB, const void *const *init_in,
                                  void *const *d_flo, int nx, int ny, bool stage_all, OfxPairIO &io)
{
    const size_t n = (size_t) nx * ny;
    io.kind = ofx_src_kind(ctx);
    io.pitch = nx > 0 ? ofx_src_pitch(ctx, nx) : 0;
    const size_t span = ofx_frame_span(nx, ny, io.pitch, ofx_src_bytes(io.kind));
    for (int g = 0; g < G; g++) {
        io.a[g] = const_cast<void *>(dA[g]);
        io.b[g] = const_cast<void *>(dB[g]);
        io.flo[g] = d_flo[g];
        io.init[g] = nullptr;
        if (stage_all) {
            OFX_TRY(ofx_stage_in(ctx, dA[g], span, true, &io.a[g]));
            OFX_TRY(ofx_stage_in(ctx, dB[g], span, true, &io.b[g]));
            OFX_TRY(ofx_stage_in(ctx, d_flo[g], n * sizeof(float2), false, &io.flo[g]));
        }
        if (init_in) OFX_TRY(ofx_stage_in(ctx, init_in[g], n * sizeof(float2), true, &io.init[g]));
    }
    return OFX_OK;
}
// ... and back into the caller's payloads where the solve wrote a stage
static inline int ofx_pairs_unstage(ofx_ctx *ctx, int G, void *const *d_flo, const OfxPairIO &io, size_t n)
{
    for (int g = 0; g < G; g++) OFX_TRY(ofx_stage_out(ctx, d_flo[g], io.flo[g], n * sizeof(float2)));
    return OFX_OK;
}

// ---- refusals -----------------------------------------------------------------------------------------------------------------
// the start's own refusals, before any work: the alignment of every payload, then the Gaussians of its pyramid
static inline int ofx_start_check(ofx_ctx *ctx, const char *who, int n_pairs, const void *const *d_flo_init, int nx, int ny,
                                  int nscales, double z)
{
    if (!d_flo_init) return OFX_OK;
    for (int g = 0; g < n_pairs; g++)
        if (reinterpret_cast<uintptr_t>(d_flo_init[g]) % sizeof(float2))
            return ofx_fail(ctx, OFX_ERR_ARG, "%s: start payload of pair %d is not 8-byte aligned", who, g);
    std::vector<int> nxs, nys;
    OFX_TRY(op_pyramid_sizes(ctx, nx, ny, nscales, z, nxs, nys));
    return op_flow_pyramid_check(ctx, nscales, z, nxs.data(), nys.data());
}
// The starts' refusals for the whole batch, before any group runs (groups run concurrently: a refusal inside one would find the
// others at work).  The pair is named by its index in the batch, the reason is left in every context.
static inline int ofx_batch_start_check(ofx_ctx *const *ctxs, int n_ctx, const char *who, int n_pairs, const void *const *d_flo_init,
                                        int nx, int ny, int nscales, double z)
{
    if (!d_flo_init) return OFX_OK;
    int s = OFX_OK;
    for (int w = 0; w < n_ctx; w++) {
        const int sw = ofx_start_check(ctxs[w], who, n_pairs, d_flo_init, nx, ny, nscales, z);
        if (s == OFX_OK) s = sw;
    }
    return s;
}

// What every ofx_*_group_dev entry on pairs shares: the checks of the pointer tables and the group size, then the solver's own
// (check), then solve(st) under the group shell (ofx_group_records).
template <class CheckFn, class SolveFn>
static int ofx_pair_group_entry(ofx_ctx *ctx, const char *who, int n_pairs, const void *const *dA, const void *const *dB,
                                void *const *d_flo, ofx_stats *stats_out, CheckFn check, SolveFn solve)
{
    if (!dA || !dB || !d_flo) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer", who);
    if (n_pairs < 1 || n_pairs > OFX_MAX_GROUP)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: a lockstep group holds 1..%d pairs (got %d)", who, OFX_MAX_GROUP, n_pairs);
    for (int g = 0; g < n_pairs; g++)
        if (!dA[g] || !dB[g] || !d_flo[g]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer (pair %d)", who, g);
    OFX_TRY(check());
    return ofx_group_records(ctx, n_pairs, stats_out, solve);
}

// What the video chains check before any work (include/ofx.h), after the solver's parameters: the tables, then both pyramids --
// sizes, the pre-smoothing Gaussian of the frames (sigma) and the Gaussians of the start's pyramid.  The walk itself is
// ofx_chain_walk (ofx_group_plan.h); frames and payloads that are not on the context's GPU (the front-ends' host arrays) are
// staged step by step (stage_all).
static inline int ofx_chain_check(ofx_ctx *ctx, const char *who, int n_seq, int n_frames, const void *const *dF, void *const *d_flo,
                                  int nx, int ny, int nscales_first, int nscales_next, double z, double sigma)
{
    if (!dF || !d_flo) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL pointer", who);
    if (n_seq < 1 || n_seq > OFX_MAX_GROUP)
        return ofx_fail(ctx, OFX_ERR_ARG, "%s: a lockstep group holds 1..%d sequences (got %d)", who, OFX_MAX_GROUP, n_seq);
    if (n_frames < 2) return ofx_fail(ctx, OFX_ERR_ARG, "%s: %d frames (a sequence has at least 2)", who, n_frames);
    const int steps = n_frames - 1;
    for (int q = 0; q < n_seq; q++) {
        for (int t = 0; t < n_frames; t++)
            if (!dF[(size_t) q * n_frames + t]) return ofx_fail(ctx, OFX_ERR_ARG, "%s: NULL frame %d of sequence %d", who, t, q);
        for (int t = 0; t < steps; t++) {
            const void *p = d_flo[(size_t) q * steps + t];
            if (!p || reinterpret_cast<uintptr_t>(p) % sizeof(float2))
                return ofx_fail(ctx, OFX_ERR_ARG, "%s: payload %d of sequence %d NULL or not 8-byte aligned", who, t, q);
        }
    }
    OFX_TRY(ofx_pitch_check(ctx, who, nx));
    for (int k = 0; k < 2; k++) {
        const int nscales = k ? nscales_next : nscales_first;
        std::vector<int> nxs, nys;
        OFX_TRY(op_pyramid_sizes(ctx, nx, ny, nscales, z, nxs, nys));
        GaussTaps taps;
        if (ofx_gauss_taps(sigma, &taps) == OFX_OK && (taps.size >= nx || taps.size >= ny))
            return ofx_fail(ctx, OFX_ERR_SIGMA, "GaussianSmooth: sigma too large (radius %d, image %dx%d)", taps.size, nx, ny);
        OFX_TRY(op_flow_pyramid_check(ctx, nscales, z, nxs.data(), nys.data()));
    }
    return OFX_OK;
}

// ---- the head of every coarse-to-fine driver ------------------------------------------------------------------------------------
// src/tvl1flow.cpp:236-280 == horn_schunck_pyramidal.cpp:279-323 == brox_optic_flow_spatial.cpp:467-509 for the G solves of a
// lockstep group over the images of Gp pairs (Gp = G but for TV-L1 both ways, where two solves share a pair's images): the level
// sizes, into every record too; the levels -- levels(nxs, nys, lA, lB, &U) allocates them and tells where each level's first
// and second images lie (Gp planes each) and where the flows of the coarsest level start (solve g at U + g * its pixels); the two
// temporaries and the scratch; the image pyramids in one launch per step (op_build_pyramid_group); and the start -- zeros, or
// with a table of G start payloads (NULL entry: zero start) the payloads' own pyramid (op_flow_pyramid), its last level rounded
// once into U.  The arena hands out the levels, the temporaries, the scratch and the start's scratch, in that order.
template <typename T, class LevelsFn>
static int ofx_pyramid_head(ofx_ctx *ctx, int G, int Gp, const void *const *dA, const void *const *dB, int nx, int ny, int nscales,
                            double zfactor, double sigma, int nsolves, ofx_stats *stats, int kind, size_t pitch,
                            const void *const *init, LevelsFn levels)
{
    std::vector<int> nxs, nys;
    OFX_TRY(op_pyramid_sizes(ctx, nx, ny, nscales, zfactor, nxs, nys));
    for (int g = 0; g < G; g++) {
        ofx_stats_begin(&stats[g], nscales, nsolves);
        for (int s = 0; s < nscales && s < OFX_MAX_SCALES; s++) { stats[g].nx[s] = nxs[s]; stats[g].ny[s] = nys[s]; }
    }
    std::vector<T *> lA(nscales), lB(nscales);
    typename Pix<T>::v2 *U;
    OFX_TRY(levels(nxs, nys, lA.data(), lB.data(), &U));
    T *tmpA, *tmpB;                                   // all 2 Gp images of the group per launch (op_build_pyramid_group)
    double *scr;
    OFX_TRY(ofx_alloc(ctx, (size_t) 2 * Gp * nx * ny, &tmpA));
    OFX_TRY(ofx_alloc(ctx, (size_t) 2 * Gp * nx * ny, &tmpB));
    OFX_TRY(ofx_alloc(ctx, (size_t) Gp * op_pyramid_scratch_doubles(), &scr));
    OFX_TRY(op_build_pyramid_group<T>(ctx, Gp, dA, dB, nscales, zfactor, sigma, nxs.data(), nys.data(), lA.data(), lB.data(), tmpA,
                                      tmpB, scr, kind, pitch));
    const size_t nc = (size_t) nxs[nscales - 1] * nys[nscales - 1];
    if (!init) return op_fill2<T>(ctx, U, nc * G);
    void *dst[OFX_MAX_GROUP];
    for (int g = 0; g < G; g++) dst[g] = U + g * nc;
    return op_flow_pyramid<typename Pix<T>::v2>(ctx, G, init, nscales, zfactor, nxs.data(), nys.data(), dst);
}
