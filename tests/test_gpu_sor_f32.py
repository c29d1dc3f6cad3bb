"""The SOR solvers in float storage (OFX_F32: float in memory, double arithmetic), csrc/ofx_sor.hip and csrc/ofx_sor_tile.hip.

Schedule invariance.  The kernels keep doubles in LDS and round a new value to float before it goes to LDS and to memory, so in
float storage -- as in double -- every schedule of one sweep order must give the same bits: one launch per time step, windowed
sweeps from global memory or from an LDS window, any window length, row-block height, batch size or number of sweeps per
workgroup, k_hs_tile for every K and geometry, k_brox_wave / k_brox_tile for every tile width, prefetch depth and K, a lone pair
or a lockstep group of 16.  For every family one BASE schedule -- the simplest code -- is solved once per case on the float
context and every variant is compared with it:

 * flows bit for bit (int64 views of the returned doubles, int32 views of .flo payloads);
 * sweep tables equal; a table that differs is reported with both stopping values and TOL;
 * stopping values to nx ny 2^-52 relative.  A stopping value is sqrt(sum of nx ny squared updates / size): every term is >= 0
   and the same in every schedule, only the order of the sum differs.  A sum of n non-negative doubles carries a relative error
   of at most (n - 1) 2^-53 in any order, so two orders differ by at most n 2^-52 (the square root halves it) -- derived, not
   measured.

The frames of `synth` are integers and so exact in float: the host entries and the device entries on torch.float32 tensors see
the same values.  Every base result is finite and float-representable, and non-zero wherever a sweep ran.

The anchor outside the library.  Invariance cannot see an error that every schedule shares -- a rounding missing in a per-pixel
function -- so the second half pins the float solvers to the oracle's restatement of float storage (orc_*_mode with store_f32 =
1; oracle/ofx_oracle.h lists what is rounded; checked on the CPU in tests/test_oracle_sor_f32.py): the exact mode against order
0, the tolerance mode against orders 1 and 3.  The bar is 100 % of the elements and 0 float ulps: both sides compute correctly
rounded double arithmetic without contraction and round to float at the same places, so it follows from the construction and is
no measurement.  OFX_MEASURE_OUT=<file> records the observed share and worst ulp (profiles/r16_sor_f32_restatement.json).

Options are set through `options` (library defaults restored in `finally`)."""
import contextlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the library's defaults of every option this file touches (ofx_ctx.cpp)
DEFAULTS = dict(sor_exact=1, sor_batch=0, sor_fuse=0, sor_tile=0, sor_tile_w=0, sor_wave_levels=1, sor_wave_p=0, sor_window=0,
                sor_rows=0, sor_spw=0, sor_lds=1)


@contextlib.contextmanager
def options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, DEFAULTS[k])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def is_f32(a):
    a = np.asarray(a, np.float64)
    return np.array_equal(bits(a), bits(a.astype(np.float32).astype(np.float64)))


class Solve:
    """flows, sweep table and stopping values of one solve"""

    def __init__(self, u, v, st):
        self.u, self.v = u, v
        self.it, self.err = st.iterations().copy(), st.errors().copy()


def run(gpu, fn, *args, opts=None, **kw):
    with options(gpu, **(opts or {})):
        u, v = fn(*args, **kw)
        return Solve(u, v, gpu.stats())


def check_tables(it_g, err_g, it_b, err_b, TOL, npix, where):
    """sweep tables equal (else: both stopping values and TOL), stopping values to npix 2^-52 relative"""
    it_g, it_b = np.asarray(it_g), np.asarray(it_b)
    assert it_g.shape == it_b.shape, (where, it_g.shape, it_b.shape)
    if not np.array_equal(it_g, it_b):
        bad = np.argwhere(it_g != it_b)
        raise AssertionError("%s: sweep tables differ at %s: variant %s / base %s, stopping values variant %s / base %s, TOL %g" % (
            where, bad.tolist(), it_g[tuple(bad.T)], it_b[tuple(bad.T)], err_g[tuple(bad.T)], err_b[tuple(bad.T)], TOL))
    ran = it_b > 0
    rel = np.abs(err_g[ran] - err_b[ran]) / np.maximum(np.abs(err_b[ran]), 1e-300)
    assert (rel <= npix * 2.0 ** -52).all(), (where, "stopping values", float(rel.max()), err_g[ran], err_b[ran])


def check_same(got, base, TOL, where):
    check_tables(got.it, got.err, base.it, base.err, TOL, base.u[0].size if base.u.ndim == 3 else base.u.size, where)
    assert np.array_equal(bits(got.u), bits(base.u)), (where, "u", int((bits(got.u) != bits(base.u)).sum()),
                                                       np.argwhere(bits(got.u) != bits(base.u))[:4].tolist())
    assert np.array_equal(bits(got.v), bits(base.v)), (where, "v", int((bits(got.v) != bits(base.v)).sum()),
                                                       np.argwhere(bits(got.v) != bits(base.v))[:4].tolist())


def start_flow(nx, ny, seed=11):
    """a non-zero incoming flow for the single-scale entries.  On images of up to 3 pixels a side every bicubic tap is clamped,
    the warps are zero by the reference's border rule and a solve from a zero flow stays zero: only a non-zero start makes
    the sweeps compute anything there."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (ny, nx)), rng.uniform(-1.0, 1.0, (ny, nx))


def check_base(base, where):
    for a in (base.u, base.v):
        assert np.isfinite(a).all(), where
        assert is_f32(a), (where, "not float-representable")
    if base.it.sum() > 0:
        assert base.u.any() and base.v.any(), (where, "zero flow")


# the exact mode's schedules: (sor_window, sor_rows) under both windowed kernels, fixed batches, sweeps per workgroup of the
# global kernel
WINDOWS = [(1, 2), (5, 3), (8, 7), (32, 0), (16, 9), (8, 1000)]
EXACT_VARIANTS = ([dict(sor_exact=1, sor_lds=lds, sor_window=w, sor_rows=r) for lds in (0, 2) for w, r in WINDOWS]
                  + [dict(sor_exact=1, sor_batch=b) for b in (1, 5, 300)]
                  + [dict(sor_exact=1, sor_lds=0, sor_spw=s) for s in (1, 2, 4)]
                  + [dict(sor_exact=1, sor_lds=0, sor_spw=s, sor_window=5, sor_rows=3, sor_batch=5) for s in (2, 4)]
                  + [dict(sor_exact=1)])
EXACT_BASE = dict(sor_exact=2)


# ---- Horn-Schunck, exact mode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(3, 3), (3, 40), (40, 3), (9, 8), (33, 47), (90, 61), (20, 1030)])
def test_hs_exact_schedules(gpu32, synth, nx, ny):
    """the smallest images with an interior, sizes below / above a row block and a window, and ny + 3 > 1024: more plane items
    than threads of a workgroup"""
    I1, I2 = synth.pair("P1", nx, ny, 2)
    u0, v0 = start_flow(nx, ny)
    kw = dict(alpha=15.0, warps=3 if (nx, ny) == (90, 61) else 2, TOL=1e-4, maxiter=40)
    base = run(gpu32, gpu32.hs_single_scale, I1, I2, u0, v0, opts=EXACT_BASE, **kw)
    check_base(base, (nx, ny))
    assert base.it.sum() > 0
    for opts in EXACT_VARIANTS:
        got = run(gpu32, gpu32.hs_single_scale, I1, I2, u0, v0, opts=opts, **kw)
        check_same(got, base, kw["TOL"], (nx, ny, opts))


def test_hs_exact_without_an_interior_is_the_colour_sweep(gpu32, synth):
    """7x2 has no interior: the exact schedules are not defined and every sor_exact runs the colour kernels"""
    I1, I2 = synth.pair("P1", 7, 2)
    z = start_flow(7, 2)
    kw = dict(alpha=20.0, warps=2, TOL=1e-4, maxiter=150)
    base = run(gpu32, gpu32.hs_single_scale, I1, I2, *z, opts=dict(sor_exact=0, sor_fuse=-1), **kw)
    check_base(base, "7x2")
    assert base.it.sum() > 0
    for opts in (dict(sor_exact=1), dict(sor_exact=2), dict(sor_exact=1, sor_lds=0, sor_window=5, sor_rows=3)):
        check_same(run(gpu32, gpu32.hs_single_scale, I1, I2, *z, opts=opts, **kw), base, kw["TOL"], opts)


# ---- Horn-Schunck, tolerance mode ----------------------------------------------------------------------------------------------
HS_SIZES = [("P0", 64, 48, 2), ("P1", 135, 68, 3), ("P1", 33, 47, 2), ("P1", 300, 130, 2), ("P0", 9, 8, 1), ("P1", 257, 75, 1), ("P1", 2, 2, 1),
            ("P0", 131, 3, 1)]
TILE_BASE = dict(sor_exact=0, sor_fuse=-1)            # one launch per colour and sweep
TILE_VARIANTS = [dict(sor_exact=0, sor_fuse=K, sor_tile=g) for K in (0, 1, 2, 3, 4) for g in (1, 2, 3)] + [dict(sor_exact=0)]


@pytest.mark.parametrize("pair,nx,ny,ns", HS_SIZES)
def test_hs_tile_schedules(gpu32, synth, pair, nx, ny, ns):
    """k_hs_tile for every K and tile geometry against the per-colour kernels"""
    I1, I2 = synth.pair(pair, nx, ny)
    if ns == 1:                             # levels too small for the pyramid's Gaussian: the single-scale entry
        fn, args, kw = gpu32.hs_single_scale, (I1, I2, *start_flow(nx, ny)), dict(alpha=20.0, warps=3, TOL=1e-4, maxiter=150)
    else:
        fn, args, kw = gpu32.hs_pyramidal, (I1, I2), dict(alpha=20.0, nscales=ns, zfactor=0.5, warps=4, TOL=1e-4, maxiter=150)
    base = run(gpu32, fn, *args, opts=TILE_BASE, **kw)
    check_base(base, (nx, ny))
    assert base.it.sum() > 0
    for opts in TILE_VARIANTS:
        check_same(run(gpu32, fn, *args, opts=opts, **kw), base, kw["TOL"], (nx, ny, opts))


def test_hs_tile_loop_ends(gpu32, synth):
    """loops that end inside a launch unit, at maxiter (a multiple of K or not), at once, or never start"""
    I1, I2 = synth.pair("P1", 150, 97)
    z = np.zeros((97, 150))
    ends = set()
    for kw in (dict(maxiter=0), dict(maxiter=1), dict(maxiter=3), dict(maxiter=7), dict(maxiter=8), dict(TOL=2000.0), dict(TOL=0.3),
               dict(TOL=1e-2), dict(TOL=1e-3), dict(TOL=3e-4), dict(TOL=1e-5, maxiter=41)):
        base = run(gpu32, gpu32.hs_single_scale, I1, I2, z, z, opts=TILE_BASE, alpha=15.0, warps=3, **kw)
        check_base(base, kw)
        ends.update(int(n) for n in base.it.ravel())
        for K in (1, 2, 3, 4):
            got = run(gpu32, gpu32.hs_single_scale, I1, I2, z, z, opts=dict(sor_exact=0, sor_fuse=K), alpha=15.0, warps=3, **kw)
            check_same(got, base, kw.get("TOL", 1e-4), (kw, K))
    assert {0, 1, 3, 7, 8, 41} <= ends and len({n % 4 for n in ends}) == 4


# ---- Brox spatial --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,kw", [
    (90, 61, dict(alpha=50.0, gamma=10.0, nscales=2, nu=0.5, TOL=1e-4, inner=2, outer=3)),
    (6, 40, dict(alpha=30.0, gamma=5.0, nscales=1, nu=0.5, TOL=1e-4, inner=1, outer=2)),      # 6: the smallest size the presmoothing takes
    (40, 6, dict(alpha=30.0, gamma=5.0, nscales=1, nu=0.5, TOL=1e-4, inner=1, outer=2)),
    (6, 6, dict(alpha=30.0, gamma=5.0, nscales=1, nu=0.5, TOL=1e-4, inner=1, outer=2)),
    (20, 1030, dict(alpha=30.0, gamma=5.0, nscales=1, nu=0.5, TOL=1e-4, inner=1, outer=1))])
def test_brox_exact_schedules(gpu32, synth, nx, ny, kw):
    I1, I2 = synth.pair("P1", nx, ny, 2)
    base = run(gpu32, gpu32.brox_spatial, I1, I2, opts=EXACT_BASE, **kw)
    check_base(base, (nx, ny))
    assert base.it.sum() > 0
    for opts in EXACT_VARIANTS:
        check_same(run(gpu32, gpu32.brox_spatial, I1, I2, opts=opts, **kw), base, kw["TOL"], (nx, ny, opts))


# (pair, nx, ny, nscales, tile width, wave levels): tile width 32 with two wave levels, widths and heights off the tile pitch, a
# level smaller than a tile, no wave level at all; k_brox_tile sweeps the levels below the wave levels, so three cases leave it some
BROX_CASES = [("P1", 135, 68, 2, 32, 2), ("P1", 70, 129, 1, 128, 1), ("P1", 257, 75, 2, 64, 2), ("P0", 16, 12, 1, 128, 1),
              ("P1", 300, 130, 3, 128, 0), ("P0", 33, 70, 1, 16, 1), ("P1", 160, 120, 3, 128, 1), ("P1", 135, 68, 2, 128, 0)]


@pytest.mark.parametrize("pair,nx,ny,ns,tw,wl", BROX_CASES)
def test_brox_tile_schedules(gpu32, synth, pair, nx, ny, ns, tw, wl):
    """prefetch depth of k_brox_wave x sweeps per launch of k_brox_tile; sor_fuse = 9 is k_brox_sor, two launches per sweep"""
    I1, I2 = synth.pair(pair, nx, ny)
    kw = dict(alpha=50.0, gamma=10.0, nscales=ns, nu=0.5, TOL=1e-4, inner=2, outer=4)
    geom = dict(sor_exact=0, sor_tile_w=tw, sor_wave_levels=wl)
    base = run(gpu32, gpu32.brox_spatial, I1, I2, opts=dict(geom, sor_wave_p=4, sor_fuse=9), **kw)
    check_base(base, (nx, ny))
    assert base.it.sum() > 0
    for P, K in ((0, 0), (2, 1), (8, 4)):
        got = run(gpu32, gpu32.brox_spatial, I1, I2, opts=dict(geom, sor_wave_p=P, sor_fuse=K), **kw)
        check_same(got, base, kw["TOL"], (nx, ny, P, K))


# ---- lockstep groups on float tensors: every pair equals the lone solve of that pair ---------------------------------------------
MODES = {"exact": dict(), "tolerance": dict(sor_exact=0)}


def _group_inputs(synth, G, nx, ny, name=lambda k: "P0" if k % 3 == 2 else "P1"):
    import torch
    pairs = [synth.pair(name(k), nx, ny, k) for k in range(G)]
    d0 = [torch.from_numpy(p[0]).to(torch.float32).cuda() for p in pairs]
    d1 = [torch.from_numpy(p[1]).to(torch.float32).cuda() for p in pairs]
    flo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return pairs, d0, d1, flo


def _ptr(ts):
    return [t.data_ptr() for t in ts]


def _group(gpu, group_fn, d0, d1, flo, nx, ny, **kw):
    flo.zero_()
    st = group_fn(_ptr(d0), _ptr(d1), [flo[k].data_ptr() for k in range(len(d0))], nx, ny, **kw)
    gpu.synchronize()
    return st, flo.cpu().numpy().copy()


def check_group(st, got, lone, TOL, where):
    """records and payloads of a group against the lone solves of its pairs"""
    for k, base in enumerate(lone):
        check_tables(st[k].iterations(), st[k].errors(), base.it, base.err, TOL, base.u.size, (where, k))
        want = np.stack([base.u, base.v], axis=-1).astype(np.float32)      # exact: the flows are floats
        assert np.array_equal(got[k].view(np.int32), want.view(np.int32)), (where, k, int((got[k] != want).sum()))


@pytest.mark.parametrize("G", [1, 3, 5, 16])
@pytest.mark.parametrize("mode", list(MODES))
def test_hs_group_equals_pairs_solved_alone(gpu32, synth, mode, G):
    """the default geometry of a group of >= 4 (125 rows, global steps) differs from a lone solve's (64 rows, LDS window)"""
    nx, ny = 150, 97
    kw = dict(alpha=15.0, nscales=3, zfactor=0.5, warps=4, TOL=1e-4, maxiter=150)
    pairs, d0, d1, flo = _group_inputs(synth, G, nx, ny)
    with options(gpu32, **MODES[mode]):
        st, got = _group(gpu32, gpu32.hs_group_dev, d0, d1, flo, nx, ny, **kw)
        lone = [run(gpu32, gpu32.hs_pyramidal, p[0], p[1], **kw) for p in pairs]
    for base in lone:
        check_base(base, (mode, G))
    check_group(st, got, lone, kw["TOL"], (mode, G))
    if G >= 5:
        assert len({tuple(int(x) for x in b.it.ravel()) for b in lone}) > 1        # the pairs really stop at different sweeps


@pytest.mark.parametrize("G", [1, 3, 16])
@pytest.mark.parametrize("mode", list(MODES))
def test_brox_group_equals_pairs_solved_alone(gpu32, synth, mode, G):
    nx, ny = 140, 90
    kw = dict(alpha=50.0, gamma=10.0, nscales=3, nu=0.5, TOL=1e-4, inner=2, outer=4)
    pairs, d0, d1, flo = _group_inputs(synth, G, nx, ny)
    with options(gpu32, **MODES[mode]):
        st, got = _group(gpu32, gpu32.brox_group_dev, d0, d1, flo, nx, ny, **kw)
        lone = [run(gpu32, gpu32.brox_spatial, p[0], p[1], **kw) for p in pairs]
    for base in lone:
        check_base(base, (mode, G))
    check_group(st, got, lone, kw["TOL"], (mode, G))


def test_groups_with_small_batches_and_odd_windows(gpu32, synth):
    """pairs that stop in different batches of a solve (small snapshot capacity) and odd window / row-block sizes"""
    nx, ny, G = 96, 70, 4
    pairs, d0, d1, flo = _group_inputs(synth, G, nx, ny)
    hk = dict(alpha=10.0, nscales=2, zfactor=0.5, warps=3, TOL=1e-5, maxiter=90)
    bk = dict(alpha=50.0, gamma=10.0, nscales=2, nu=0.5, TOL=1e-4, inner=1, outer=3)
    for group_fn, lone_fn, kw, geoms in (
            (gpu32.hs_group_dev, gpu32.hs_pyramidal, hk, ((5, 3, 16, 1), (9, 8, 64, 2), (300, 5, 7, 4), (7, 8, 125, 2), (64, 4, 200, 4))),
            (gpu32.brox_group_dev, gpu32.brox_spatial, bk, ((6, 3, 16, 2), (300, 4, 125, 4), (9, 8, 61, 1)))):
        lone = [run(gpu32, lone_fn, p[0], p[1], **kw) for p in pairs]
        for batch, window, rows, spw in geoms:
            with options(gpu32, sor_batch=batch, sor_window=window, sor_rows=rows, sor_spw=spw):
                st, got = _group(gpu32, group_fn, d0, d1, flo, nx, ny, **kw)
            check_group(st, got, lone, kw["TOL"], (batch, window, rows, spw))


# ---- Brox temporal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,frames,k,kw", [(40, 33, 5, 1, dict(nscales=1, outer=2, inner=1)),
                                               (48, 40, 3, 0, dict(nscales=2, outer=3))])         # nz = 2: no interior frame
def test_brox_temporal_exact_schedules(gpu32, synth, nx, ny, frames, k, kw):
    I = synth.sequence(nx, ny, frames, k)
    base = run(gpu32, gpu32.brox_temporal, I, **kw)
    check_base(base, (nx, ny, frames))
    assert base.it.sum() > 0
    for window, rows in ((1, 2), (5, 3), (32, 0), (8, 1000)):
        got = run(gpu32, gpu32.brox_temporal, I, opts=dict(sor_window=window, sor_rows=rows), **kw)
        check_same(got, base, 1e-4, (nx, ny, frames, window, rows))


@pytest.mark.parametrize("nx,ny,frames", [(33, 47, 4), (135, 68, 5)])
def test_brox_temporal_tile_schedules(gpu32, synth, nx, ny, frames):
    """3-D red-black sweeps: the per-colour kernel (sor_fuse = 9) against 1, 2 and 4 sweeps per launch on LDS tiles"""
    I = synth.sequence(nx, ny, frames)
    base = run(gpu32, gpu32.brox_temporal, I, opts=dict(sor_exact=0, sor_fuse=9), nscales=2)
    check_base(base, (nx, ny, frames))
    assert base.it.sum() > 0
    for K in (0, 1, 2, 4):
        got = run(gpu32, gpu32.brox_temporal, I, opts=dict(sor_exact=0, sor_fuse=K), nscales=2)
        check_same(got, base, 1e-4, (nx, ny, frames, K))


# ---- robust_expo, one channel: one kernel (k_brox_window<T, 1, 1024, true>), so sor_lds / sor_spw do not apply -------------------
REXPO = {1: dict(method=1, alpha=50.0, gamma=10.0, lam=0.1, outer=4), 2: dict(method=2, alpha=18.7, gamma=5.0, lam=0.05, outer=3, inner=2),
         3: dict(method=3, alpha=30.0, gamma=10.0, lam=1.0, outer=3)}


@pytest.mark.parametrize("nx,ny", [(64, 48), (80, 60)])
@pytest.mark.parametrize("method", [1, 2, 3])
def test_robust_expo_schedules(gpu32, synth, method, nx, ny):
    I1, I2 = synth.pair("P1", nx, ny)
    kw = dict(REXPO[method], nscales=2)
    base = run(gpu32, gpu32.robust_expo, I1, I2, **kw)
    check_base(base, (method, nx, ny))
    assert base.it.sum() > 0
    for opts in [dict(sor_window=w, sor_rows=r) for w, r in WINDOWS] + [dict(sor_batch=b) for b in (1, 5, 300)]:
        check_same(run(gpu32, gpu32.robust_expo, I1, I2, opts=opts, **kw), base, 1e-4, (method, nx, ny, opts))


# ---- seeded random groups: a longer soak with other draws through OFX_FUZZ_SEED, as tests/test_gpu_fuzz.py ------------------------
FUZZ_SEED = int(os.environ.get("OFX_FUZZ_SEED", "2026"))


@pytest.mark.parametrize("seed", range(3))
def test_random_groups_equal_pairs_solved_alone(gpu32, synth, seed):
    """random size, group, mode and options: the group runs under them, every pair alone under the library's defaults of the mode"""
    rng = np.random.default_rng((2300 if FUZZ_SEED == 2026 else 8000 * FUZZ_SEED) + seed)
    nx, ny, G = int(rng.integers(20, 200)), int(rng.integers(16, 140)), int(rng.choice([2, 3, 5, 9, 16]))
    ns = 3 if min(nx, ny) >= 80 else (2 if min(nx, ny) >= 40 else 1)
    pairs, d0, d1, flo = _group_inputs(synth, G, nx, ny, lambda k: "P0" if k % 4 == 3 else "P1")
    if seed % 2 == 0:
        mode = dict()
        opts = dict(sor_window=int(rng.choice([0, 3, 8])), sor_rows=int(rng.choice([0, 9, 61])), sor_batch=int(rng.choice([0, 7, 40])),
                    sor_spw=int(rng.choice([0, 1, 2, 4])), sor_lds=int(rng.choice([0, 1, 2])))
    else:
        mode = dict(sor_exact=0, sor_tile_w=int(rng.choice([16, 50, 64, 128])), sor_wave_levels=int(rng.choice([0, 1, 1, 2])))
        opts = dict(sor_fuse=int(rng.choice([0, 1, 2, 3, 4])), sor_tile=int(rng.choice([0, 1, 2, 3])), sor_wave_p=int(rng.choice([0, 2, 6])))
    hk = dict(alpha=float(rng.choice([7.0, 20.0])), nscales=ns, zfactor=0.5, warps=int(rng.integers(1, 4)),
              TOL=float(rng.choice([1e-4, 1e-3])), maxiter=int(rng.choice([5, 6, 7, 150])))
    bk = dict(alpha=float(rng.choice([50.0, 18.0])), gamma=float(rng.choice([10.0, 0.0])), nscales=ns, nu=0.5, TOL=1e-4,
              inner=int(rng.integers(1, 3)), outer=int(rng.integers(1, 4)))
    for group_fn, lone_fn, kw in ((gpu32.hs_group_dev, gpu32.hs_pyramidal, hk), (gpu32.brox_group_dev, gpu32.brox_spatial, bk)):
        with options(gpu32, **mode):
            lone = [run(gpu32, lone_fn, p[0], p[1], **kw) for p in pairs]
            with options(gpu32, **opts):
                st, got = _group(gpu32, group_fn, d0, d1, flo, nx, ny, **kw)
        for base in lone:
            check_base(base, (nx, ny, G, mode, opts))
        check_group(st, got, lone, kw["TOL"], (nx, ny, G, mode, opts, kw))


# ---- the anchor: gpu32 against the oracle's restatement of float storage ----------------------------------------------------------
F32_SAME, F32_ULPS = 1.0, 0                 # by construction (module docstring), not measured
MEASURED = {}


def _measure(key, value, worst=max):
    MEASURED[key] = worst(MEASURED.get(key, value), value)


@pytest.fixture(scope="module", autouse=True)
def _record():
    """OFX_MEASURE_OUT=<file>: write the worst deviations seen, as tests/test_gpu_relaxed_modes.py does"""
    yield
    out = os.environ.get("OFX_MEASURE_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def check_restatement(family, got, want, where):
    """got: a Solve or (u, v, table); want: the oracle's (u, v, table)"""
    ug, vg, it_g = (got.u, got.v, got.it) if isinstance(got, Solve) else got
    uo, vo, it_o = want
    it_g, it_o = np.asarray(it_g), np.asarray(it_o).reshape(np.asarray(it_g).shape)
    if not np.array_equal(it_g, it_o):
        bad = np.argwhere(it_g != it_o)
        raise AssertionError("%s %s: sweep tables differ at %s: gpu %s / restatement %s" % (
            family, where, bad.tolist(), it_g[tuple(bad.T)], it_o[tuple(bad.T)]))
    g, w = np.concatenate([ug.ravel(), vg.ravel()]), np.concatenate([uo.ravel(), vo.ravel()])
    assert np.isfinite(g).all() and is_f32(g), (family, where)
    same = float(np.mean(bits(g) == bits(w)))
    ulps = float((np.abs(g - w) / np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)).max())
    _measure(family + "_same_frac", same, min)
    _measure(family + "_ulps", ulps)
    _measure(family + "_cases", MEASURED.get(family + "_cases", 0) + 1)
    if ulps > F32_ULPS or same < F32_SAME:
        first = np.argwhere((bits(ug) != bits(uo)) | (bits(vg) != bits(vo)))[0].tolist()
        raise AssertionError("%s %s: %.6f of the elements equal, worst %.3g float ulps, first difference at pixel %s" % (
            family, where, same, ulps, first))


ANCHOR_SHAPES = [("P1", 9, 8, 1), ("P1", 33, 47, 1), ("P1", 90, 61, 1), ("P1", 135, 68, 1), ("P1", 257, 75, 1), ("P0", 64, 48, 3),
                 ("P1", 160, 120, 3)]


@pytest.mark.parametrize("pair,nx,ny,ns", ANCHOR_SHAPES)
def test_hs_exact_equals_the_restatement(gpu32, orc, synth, pair, nx, ny, ns):
    """order 0; at one scale the single-scale entry from a non-zero flow and the pyramid entry (normalisation + presmoothing)"""
    I1, I2 = synth.pair(pair, nx, ny)
    kw = dict(alpha=20.0, nscales=ns, zfactor=0.5, warps=4, TOL=1e-4, maxiter=150)
    check_restatement("hs_exact", run(gpu32, gpu32.hs_pyramidal, I1, I2, **kw), orc.hs_pyramidal_mode(I1, I2, store_f32=1, **kw),
                      (nx, ny, ns))
    if ns == 1:
        u0, v0 = start_flow(nx, ny)
        sk = dict(alpha=15.0, warps=3, TOL=1e-4, maxiter=150)
        check_restatement("hs_exact", run(gpu32, gpu32.hs_single_scale, I1, I2, u0, v0, **sk),
                          orc.hs_single_scale_mode(I1, I2, u0, v0, store_f32=1, **sk), (nx, ny, "single scale"))


@pytest.mark.parametrize("pair,nx,ny,ns", ANCHOR_SHAPES)
def test_hs_tolerance_equals_the_restatement(gpu32, orc, synth, pair, nx, ny, ns):
    """order 1 (four colours): the library's default tile sweeps and the per-colour kernels"""
    I1, I2 = synth.pair(pair, nx, ny)
    kw = dict(alpha=20.0, nscales=ns, zfactor=0.5, warps=4, TOL=1e-4, maxiter=150)
    orc.set_sor_order(1)
    want = orc.hs_pyramidal_mode(I1, I2, store_f32=1, **kw)
    for opts in (dict(sor_exact=0), dict(sor_exact=0, sor_fuse=-1)):
        check_restatement("hs_tolerance", run(gpu32, gpu32.hs_pyramidal, I1, I2, opts=opts, **kw), want, (nx, ny, ns, opts))


@pytest.mark.parametrize("pair,nx,ny,ns", ANCHOR_SHAPES)
def test_brox_exact_equals_the_restatement(gpu32, orc, synth, pair, nx, ny, ns):
    I1, I2 = synth.pair(pair, nx, ny)
    kw = dict(alpha=50.0, gamma=10.0, nscales=ns, nu=0.5, TOL=1e-4, inner=2, outer=3)
    check_restatement("brox_exact", run(gpu32, gpu32.brox_spatial, I1, I2, **kw), orc.brox_spatial_mode(I1, I2, store_f32=1, **kw),
                      (nx, ny, ns))


@pytest.mark.parametrize("pair,nx,ny,ns", ANCHOR_SHAPES)
def test_brox_tolerance_equals_the_restatement(gpu32, orc, synth, pair, nx, ny, ns):
    """order 1 with (tile width, wave levels) = the library's default, narrow tiles on two levels, and red-black everywhere; and
    order 3 asked for directly (every level a checkerboard of tiles: sor_wave_levels = 64)"""
    I1, I2 = synth.pair(pair, nx, ny)
    kw = dict(alpha=50.0, gamma=10.0, nscales=ns, nu=0.5, TOL=1e-4, inner=2, outer=3)
    for order, tw, wl in ((1, 128, 1), (1, 32, 2), (1, 128, 0), (3, 32, 64)):
        orc.set_sor_order(order)
        orc.set_sor_tile(tw, 64)
        orc.set_sor_wave_levels(wl)
        want = orc.brox_spatial_mode(I1, I2, store_f32=1, **kw)
        got = run(gpu32, gpu32.brox_spatial, I1, I2, opts=dict(sor_exact=0, sor_tile_w=tw, sor_wave_levels=wl), **kw)
        check_restatement("brox_tolerance", got, want, (nx, ny, ns, order, tw, wl))


@pytest.mark.parametrize("nx,ny,niter", [(64, 48, 50), (135, 68, 200), (33, 21, 7), (5, 4, 3), (2, 2, 1), (320, 240, 0)])
def test_hs_classic_equals_the_restatement(gpu32, orc, synth, nx, ny, niter):
    a, b = synth.pair("P1", max(nx, 8), max(ny, 8))
    a, b = np.ascontiguousarray(a[:ny, :nx]) + 0.3, np.ascontiguousarray(b[:ny, :nx]) * 1.01       # no floats: the upload rounds
    uo, vo = orc.hs_classic_mode(a, b, niter, 15.0, store_f32=1)
    ug, vg = gpu32.hs_classic(a, b, niter, 15.0)
    check_restatement("hs_classic", (ug, vg, np.zeros(1, int)), (uo, vo, np.zeros(1, int)), (nx, ny, niter))
