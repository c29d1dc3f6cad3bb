"""The two modes behind the published speed numbers, pinned to the oracle's restatement of their arithmetic
(oracle/ofx_oracle.c, the *_mode entry points; checked on the CPU in tests/test_oracle_modes.py):

* the f64 tolerance mode (option relaxed_dual = 1, what bench.py's headline times): double storage, the dual update with
  sqrt_tol / rcp_tol and the primal with -rho * rcp_tol(grad).  The restatement (relaxed = 1) uses the exact sqrt and 1 / x,
  so the kernels may differ from it by the ~2^-45 of one refinement step per operation -- bars of 1e-10 and below, not the
  1e-4 of the stated tolerance;
* float storage (OFX_F32): double arithmetic, every stored value rounded to float.  The restatement (store_f32 = 1) rounds
  exactly where the kernels store T: the operators are bit-exact, and so -- measured -- are the iteration kernels (the
  ~2^-45 of the tolerance arithmetic could move a float rounding; on these states it never does).

Every iteration kernel and its variants (strip heights, non-temporal stores, K-iteration tiles) must also give the same bits
as every other in both modes, in single launches and in whole lockstep-group solves.

Kernel choices are explicit options here (reset in `finally`), not test_gpu_tvl1's autouse fixture."""
import contextlib
import json
import os

import numpy as np
import pytest
from test_oracle_modes import patched_state

pytestmark = pytest.mark.gpu

PAR = dict(tau=0.25, lam=0.15, theta=0.3)

# the library's defaults of every option this file touches (ofx_ctx.cpp)
DEFAULTS = dict(relaxed_dual=0, fuse2=1, fuse3=2, fuse3_min_px=0, fuse3_cursor=1, tile=0, tile_max_px=0, nt_stores=0,
                rows_per_wave=0, rows_per_wave2=0, rows_per_wave3=0, store_a=1, gauss_fused=1, warp_lds=1)

# iteration kernels and variants: one iteration per launch (k_tvl1_iter), two (k_tvl1_iter2, the default for a lone pair),
# three (k_tvl1_iter3), K on 2-D tiles (k_tvl1_tile), non-temporal stores, strip heights
KERNELS = {
    "iter1": dict(fuse2=0),
    "iter1_rows3": dict(fuse2=0, rows_per_wave=3),
    "iter2": dict(fuse3=0),
    "iter2_rows5": dict(fuse3=0, rows_per_wave2=5),
    "iter2_nt": dict(fuse3=0, nt_stores=1),
    "iter3": dict(fuse3=1, fuse3_min_px=0),
    "iter3_rows4": dict(fuse3=1, fuse3_min_px=0, rows_per_wave3=4),
    "iter3_nt": dict(fuse3=1, fuse3_min_px=0, nt_stores=1),
    "tile4": dict(tile=4, tile_max_px=1e9),
    "tile6": dict(tile=6, tile_max_px=1e9),
}
BASE = "iter2"

# output columns per wave: 62 (iter), 60 (iter2), 56 (iter3); tile pitch 56 x 8 (K = 4) and 52 x 4 (K = 6)
SHAPES = [(5, 4), (2, 2), (64, 3), (3, 64), (52, 5), (53, 4), (55, 9), (56, 17), (57, 6), (59, 11), (60, 13), (61, 33), (62, 9),
          (63, 17), (104, 17), (111, 20), (113, 16), (116, 35), (121, 19), (240, 135), (447, 301)]
N_ITERS = [1, 2, 3, 4, 5, 7]

# Bars of the iteration kernels against the restatement, set from one MI355X run over every kernel x shape x n_iter of this
# file (patched_state, seed 0) with a margin of >= 100x:
#   f64 tolerance mode:  max |delta| / max(1, |x|) of the six state arrays  measured 2.2e-15  -> bar 3e-13
#                        |delta error| / error                                 measured 1.5e-14  -> bar 2e-12
#   f32 storage:         elements bit-identical                                measured 100 %    -> bar 100 %
#                        max |delta| in float ulps of the reference value     measured 0        -> bar 0
#                        |delta error| / error (order of the sum)              measured 5.1e-14  -> bar 5e-12
# (in float storage the ~2^-45 of sqrt_tol / rcp_tol never moved a rounding on these states: the kernels ARE the restatement)
TOL64_REL, TOL64_ERR = 3e-13, 2e-12
F32_SAME, F32_ULPS, F32_ERR = 1.0, 0, 5e-12

MEASURED = {}


def _measure(key, value, worst=max):
    MEASURED[key] = worst(MEASURED.get(key, value), value)


@pytest.fixture(scope="module", autouse=True)
def _record():
    """OFX_MEASURE_OUT=<file>: write the worst deviations seen (the numbers behind the bars above)"""
    yield
    out = os.environ.get("OFX_MEASURE_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


@contextlib.contextmanager
def options(*ctxs, **kw):
    try:
        for c in ctxs:
            for k, v in kw.items():
                c.set_option(k, v)
        yield
    finally:
        for c in ctxs:
            for k in kw:
                c.set_option(k, DEFAULTS[k])


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


# ---- a. the float instantiations of every DISPATCHed operator, bit for bit --------------------------------------------------
# Expected: the double oracle on float-rounded inputs, its output rounded to float (the *_mode variants where the GPU stores an
# intermediate).  bicubic_at / bicubic_at_color take double coordinates and return doubles: only the image is float.
def rnd(seed, ny, nx, scale=1.0, shift=0.0):
    return np.random.default_rng(seed).standard_normal((ny, nx)) * scale + shift


@pytest.mark.parametrize("nx,ny", [(2, 2), (5, 7), (16, 16), (47, 33), (135, 68), (640, 480)])
def test_f32_stencils_bitexact(gpu32, orc, nx, ny):
    a, b = rnd(1, ny, nx, 50, 100), rnd(2, ny, nx, 3)
    A, B = f32(a), f32(b)
    assert same_bits(gpu32.divergence(a, b), f32(orc.divergence(A, B)))
    for g, o in zip(gpu32.forward_gradient(a), orc.forward_gradient(A)):
        assert same_bits(g, f32(o))
    for g, o in zip(gpu32.centered_gradient(a), orc.centered_gradient(A)):
        assert same_bits(g, f32(o))
    for name in ("dxx", "dyy", "dxy"):
        assert same_bits(getattr(gpu32, name)(a), f32(getattr(orc, name)(A))), name


@pytest.mark.parametrize("nx,ny", [(16, 16), (47, 33), (135, 68), (640, 480)])
@pytest.mark.parametrize("sigma", [0.8, 0.6 * np.sqrt(3.0), 1.7, 2.6])
def test_f32_gaussian_bitexact(gpu32, orc, nx, ny, sigma):
    a = rnd(3, ny, nx, 50, 100)
    assert same_bits(gpu32.gaussian(a, sigma), orc.gaussian_mode(a, sigma, 1))


@pytest.mark.parametrize("nx,ny", [(16, 16), (47, 33), (135, 68), (640, 480)])
def test_f32_bicubic_zoom_and_normalisation_bitexact(gpu32, orc, nx, ny):
    a = rnd(4, ny, nx, 50, 100)
    u, v = rnd(5, ny, nx, 3), rnd(6, ny, nx, 3)
    A, U, V = f32(a), f32(u), f32(v)
    for bo in (True, False):
        assert same_bits(gpu32.bicubic_warp(a, u, v, bo), f32(orc.bicubic_warp(A, U, V, bo)))
        assert same_bits(gpu32.bicubic_warp(a, u * 30, v * 30, bo), f32(orc.bicubic_warp(A, f32(u * 30), f32(v * 30), bo)))
        assert same_bits(gpu32.bicubic_warp(a, np.round(u), np.round(v), bo), f32(orc.bicubic_warp(A, np.round(U), np.round(V), bo)))
    for f in (0.5, 0.62, 0.75):
        assert same_bits(gpu32.zoom_out(a, f), orc.zoom_out_mode(a, f, 1)), f
    for nxx, nyy in ((2 * nx - 1, 2 * ny), (nx + 3, ny + 5)):
        assert same_bits(gpu32.zoom_in(a, nxx, nyy), f32(orc.zoom_in(A, nxx, nyy)))
    b = a * 0.5 + 3
    for g, o in zip(gpu32.image_normalization_2(a, b), orc.image_normalization_2(A, f32(b))):
        assert same_bits(g, f32(o))
    assert same_bits(gpu32.image_normalization_1(a), f32(orc.image_normalization_1(A)))
    assert gpu32.getminmax(a) == (A.min(), A.max())


def test_f32_point_samplers_and_sequences_bitexact(gpu32, orc):
    rng = np.random.default_rng(12)
    a = rng.standard_normal((20, 31)) * 50 + 100
    uu = np.concatenate([[-3.5, -0.5, 0.0, 0.25, 1.0, 1.5, 27.999, 28.0, 30.0, 30.5, 40.0], rng.uniform(-3, 33, 300)])
    vv = np.concatenate([[2.5, -0.25, 0.0, 18.5, 1.0, 17.0, 5.0, 19.0, 21.0, 7.7, -9.0], rng.uniform(-3, 22, 300)])
    for bo in (False, True):
        want = np.array([orc.bicubic_at(f32(a), x, y, bo) for x, y in zip(uu, vv)])      # double coordinates, double result
        assert same_bits(gpu32.bicubic_at(a, uu, vv, bo), want)
    img = rng.standard_normal((13, 17, 3)) * 40
    for k in range(3):
        want = np.array([orc.bicubic_at_color(f32(img), x, y, k, True) for x, y in zip(uu[:100], vv[:100])])
        assert same_bits(gpu32.bicubic_at_color(img, uu[:100], vv[:100], k, True), want)
    for nz in (1, 2, 5):
        f = rng.standard_normal((nz, 11, 14)) * 30
        for g, o in zip(gpu32.centered_gradient3(f), orc.centered_gradient3(f32(f))):
            assert same_bits(g, f32(o))
    seq = rng.uniform(3, 200, (4, 9, 12))
    assert same_bits(gpu32.image_normalization_1(seq), f32(orc.image_normalization_1(f32(seq))))


# ---- b / c. the iteration kernels against the restatement, and against each other ---------------------------------------------
_states, _refs, _base = {}, {}, {}


def _state(orc, synth, nx, ny):
    if (nx, ny) not in _states:
        _states[nx, ny] = patched_state(orc, synth, nx, ny)
    return _states[nx, ny]


def _reference(orc, synth, mode, nx, ny, n_iter):
    key = (mode, nx, ny, n_iter)
    if key not in _refs:
        u1, u2, p, I1wx, I1wy, rho_c, grad = _state(orc, synth, nx, ny)
        st = [x.copy() for x in (u1, u2, *p)]
        e = orc.tvl1_iterations_mode(*st, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], n_iter, 1,
                                     int(mode == "f32"))
        _refs[key] = (st, e)
    return _refs[key]


def _run(gpu, orc, synth, nx, ny, n_iter, **opts):
    u1, u2, p, I1wx, I1wy, rho_c, _ = _state(orc, synth, nx, ny)
    st = [x.copy() for x in (u1, u2, *p)]
    with options(gpu, **opts):
        e = gpu.tvl1_iterations(*st, I1wx, I1wy, rho_c, PAR["tau"], PAR["lam"], PAR["theta"], n_iter)
        assert gpu.stats().iterations()[0][0] == n_iter
    return st, e


def _gpu(mode, gpu64, gpu32):
    return gpu32 if mode == "f32" else gpu64


def _mode_opts(mode):
    return dict(relaxed_dual=1) if mode == "tol64" else {}


def _baseline(mode, gpu, orc, synth, nx, ny, n_iter):
    key = (mode, nx, ny, n_iter)
    if key not in _base:
        _base[key] = _run(gpu, orc, synth, nx, ny, n_iter, **_mode_opts(mode), **KERNELS[BASE])
    return _base[key]


NAMES = ("u1", "u2", "p11", "p12", "p21", "p22")


def _check_against_restatement(mode, got, e_g, want, e_w, where):
    if mode == "tol64":
        for name, g, w in zip(NAMES, got, want):
            assert np.isfinite(g).all(), (where, name)
            d = float(np.abs(g - w).max()) / max(1.0, float(np.abs(w).max()))
            _measure("tol64_rel", d)
            assert d <= TOL64_REL, (where, name, d)
        de = abs(e_g - e_w) / max(e_w, 1e-300)
        _measure("tol64_err_rel", de)
        assert de <= TOL64_ERR, (where, e_g, e_w)
    else:
        g, w = np.concatenate([x.ravel() for x in got]), np.concatenate([x.ravel() for x in want])
        assert np.isfinite(g).all(), where
        assert same_bits(g, f32(g)), where                          # the kernel stored floats
        same = float(np.mean(g == w))
        ulps = float((np.abs(g - w) / np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)).max())
        de = abs(e_g - e_w) / max(e_w, 1e-300)
        _measure("f32_same_frac", same, min)
        _measure("f32_ulps", ulps)
        _measure("f32_err_rel", de)
        assert ulps <= F32_ULPS, (where, ulps, same)
        assert same >= F32_SAME, (where, same)
        assert de <= F32_ERR, (where, e_g, e_w)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("mode", ["tol64", "f32"])
def test_iteration_kernels_against_the_restatement(gpu64, gpu32, orc, synth, mode, kernel):
    """b: every kernel choice x shape x n_iter against orc_tvl1_iterations_mode(relaxed = 1, store_f32 = f32);
    c: the same bits as the default two-iteration kernel"""
    gpu = _gpu(mode, gpu64, gpu32)
    for nx, ny in SHAPES:
        for n_iter in N_ITERS:
            where = (kernel, nx, ny, n_iter)
            want, e_w = _reference(orc, synth, mode, nx, ny, n_iter)
            base, e_b = _baseline(mode, gpu, orc, synth, nx, ny, n_iter)
            got, e_g = _run(gpu, orc, synth, nx, ny, n_iter, **_mode_opts(mode), **KERNELS[kernel])
            _check_against_restatement(mode, got, e_g, want, e_w, where)
            for name, g, b in zip(NAMES, got, base):
                assert same_bits(g, b), (where, name, "differs from " + BASE)
            # the error differs from the base kernel's by the order of its sum only
            assert abs(e_g - e_b) <= 1e-12 * max(e_b, 1e-300), (where, e_g, e_b)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_tolerance_mode_really_runs(gpu64, orc, synth, kernel):
    """e: a dispatch that ran the strict instantiation in the tolerance mode would pass every bar above the 2^-45 level -- the
    tolerance-mode output must NOT be the strict output, while the strict mode still is the strict oracle's bit for bit"""
    nx, ny, n_iter = 200, 150, 5
    u1, u2, p, I1wx, I1wy, rho_c, grad = _state(orc, synth, nx, ny)
    strict = [x.copy() for x in (u1, u2, *p)]
    orc.tvl1_iterations(*strict, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], n_iter)
    got_s, _ = _run(gpu64, orc, synth, nx, ny, n_iter, **KERNELS[kernel])
    for name, g, w in zip(NAMES, got_s, strict):
        assert same_bits(g, w), (kernel, name)
    got_t, e_t = _run(gpu64, orc, synth, nx, ny, n_iter, relaxed_dual=1, **KERNELS[kernel])
    assert not all(same_bits(g, w) for g, w in zip(got_t, strict)), kernel
    want, e_w = _reference(orc, synth, "tol64", nx, ny, n_iter)
    _check_against_restatement("tol64", got_t, e_t, want, e_w, (kernel, nx, ny, n_iter))


# ---- c. whole lockstep-group solves: every kernel choice, the pair solved alone ---------------------------------------------
GROUP_KERNELS = {
    "iter2": dict(fuse3=0),
    "iter1": dict(fuse2=0),
    "iter3_cursor": dict(fuse3=1, fuse3_min_px=0, fuse3_cursor=1),
    "iter3_fixed_units": dict(fuse3=1, fuse3_min_px=0, fuse3_cursor=0),
    "tile4": dict(tile=4, tile_max_px=1e9),
    "tile6": dict(tile=6, tile_max_px=1e9),
}


def _device_pairs(synth, G, nx, ny, dtype):
    import torch
    pairs = [synth.pair("P0" if k % 3 == 2 else "P1", nx, ny, k) for k in range(G)]
    d0 = [torch.from_numpy(p[0]).to(dtype).cuda() for p in pairs]
    d1 = [torch.from_numpy(p[1]).to(dtype).cuda() for p in pairs]
    torch.cuda.synchronize()
    return pairs, d0, d1


@pytest.mark.parametrize("G", [1, 3, 5, 16])
@pytest.mark.parametrize("mode", ["tol64", "f32"])
def test_group_solves_give_the_same_bits_with_every_kernel(gpu64, gpu32, synth, mode, G):
    import torch
    gpu = _gpu(mode, gpu64, gpu32)
    nx, ny = 150, 97
    kw = dict(nscales=3, **PAR)
    _, d0, d1 = _device_pairs(synth, G, nx, ny, torch.float32 if mode == "f32" else torch.float64)
    solo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device="cuda")
    tables = []
    with options(gpu, **_mode_opts(mode), fuse3=0):
        for k in range(G):
            gpu.tvl1_multiscale_dev(d0[k].data_ptr(), d1[k].data_ptr(), solo[k].data_ptr(), nx, ny, **kw)
            gpu.synchronize()
            tables.append(gpu.stats().iterations().copy())
    assert torch.isfinite(solo).all() and float(solo.abs().max()) > 0.0
    flo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device="cuda")
    for name, opts in GROUP_KERNELS.items():
        for store_a in (0, 1, 2):
            flo.zero_()
            with options(gpu, **_mode_opts(mode), store_a=store_a, **opts):
                st = gpu.tvl1_group_dev([t.data_ptr() for t in d0], [t.data_ptr() for t in d1], [flo[k].data_ptr() for k in range(G)],
                                        nx, ny, **kw)
                gpu.synchronize()
            for k in range(G):
                assert np.array_equal(st[k].iterations(), tables[k]), (name, store_a, k)
            assert torch.equal(flo.view(torch.int32), solo.view(torch.int32)), (name, store_a)


@pytest.mark.parametrize("nx,ny", [(203, 131), (204, 130)])
@pytest.mark.parametrize("zfactor", [0.5, 0.62, 0.75, 0.9])
def test_f32_fused_gaussian_kernels_agree(gpu32, synth, nx, ny, zfactor):
    """test_gpu_tvl1's test_fused_gaussian_kernels_agree in float storage: the float instantiations of the two-pass Gaussian,
    k_gauss_xy_g, k_gauss_xy_gr and k_gauss_xy_dec (the intermediate rounded to float in LDS) -- odd and even level sizes"""
    import torch
    dev = torch.device("cuda")
    G = 3
    pairs = [synth.pair_device("P1", nx, ny, k, dev, torch.float32) for k in range(G)]
    outs, tables = [], []
    for mode in (0, 1, 2, 3):
        flo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with options(gpu32, gauss_fused=mode):
            st = gpu32.tvl1_group_dev([p[0].data_ptr() for p in pairs], [p[1].data_ptr() for p in pairs],
                                      [flo[k].data_ptr() for k in range(G)], nx, ny, nscales=3, zfactor=zfactor, warps=2, **PAR)
            gpu32.synchronize()
        outs.append(flo)
        tables.append([s.iterations().copy() for s in st])
    for m in (1, 2, 3):
        assert torch.equal(outs[0].view(torch.int32), outs[m].view(torch.int32)), m
        assert all(np.array_equal(a, b) for a, b in zip(tables[0], tables[m])), m
    assert torch.isfinite(outs[1]).all() and float(outs[1].abs().max()) > 0.0


@pytest.mark.parametrize("amp", [0.5, 6.0, 40.0])
def test_f32_warp_tile_and_gather_paths_agree(gpu32, synth, amp):
    """the LDS-staged warp and the global gather (amp = 40 scatters a block's taps over +-40 pixels) in float storage"""
    nx, ny = 200, 150
    I0, I1 = synth.pair("P1", nx, ny)
    rng = np.random.default_rng(7)
    u0, v0 = rng.uniform(-amp, amp, (ny, nx)), rng.uniform(-amp, amp, (ny, nx))
    res, its = {}, {}
    for lds in (1, 0):
        with options(gpu32, warp_lds=lds):
            res[lds] = gpu32.tvl1_single_scale(I0, I1, u0, v0, warps=2, **PAR)
            its[lds] = gpu32.stats().iterations().copy()
    assert np.array_equal(its[0], its[1])
    assert same_bits(res[1][0], res[0][0]) and same_bits(res[1][1], res[0][1])
    assert np.isfinite(res[1][0]).all()


# ---- d. tolerance-mode whole solves against the relaxed restatement -------------------------------------------------------------
def check_tolerance_solve(st, ug, vg, want, where):
    """iteration tables equal, flows within the strict fuzz tests' 1e-9 (measured on P0 / P1 640x480: 1.6e-12), errors to 1e-9.
    A differing table is reported with the errors of both sides -- a genuine threshold tie has to be shown, not absorbed by a
    wider bar."""
    uo, vo, it_o, err_o = want
    it_g, err_g = st.iterations(), st.errors()
    if not np.array_equal(it_g, it_o):
        bad = np.argwhere(it_g != np.asarray(it_o))
        raise AssertionError("%s: iteration tables differ at %s: gpu %s / oracle %s, errors gpu %s / oracle %s" % (
            where, bad.tolist(), it_g[tuple(bad.T)], np.asarray(it_o)[tuple(bad.T)], err_g[tuple(bad.T)], err_o[tuple(bad.T)]))
    d = max(float(np.abs(ug - uo).max()), float(np.abs(vg - vo).max()))
    _measure("solve_tol64_max_abs", d)
    assert d < 1e-9, (where, d)
    assert np.allclose(err_g, err_o, rtol=1e-9, atol=1e-300), where


@pytest.mark.parametrize("pair", ["P0", "P1"])
def test_tolerance_mode_solve_640x480_equals_the_restatement(gpu64, orc, synth, pair):
    I0, I1 = synth.pair(pair, 640, 480)
    want = orc.tvl1_multiscale_mode(I0, I1, nscales=5, relaxed=1, **PAR)
    with options(gpu64, relaxed_dual=1):
        ug, vg = gpu64.tvl1_multiscale(I0, I1, nscales=5, **PAR)
        st = gpu64.stats()
    check_tolerance_solve(st, ug, vg, want, pair)
