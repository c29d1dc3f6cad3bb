"""The oracle's restatement of the HIP path's two non-strict modes (oracle/ofx_oracle.c, the *_mode entry points), on the CPU:

* with both switches off every *_mode function IS its reference counterpart, bit for bit;
* store_f32 leaves only float-representable values behind;
* the relaxed algebra (exact sqrt and reciprocal in place of hypot and the divisions) stays within ~1e-13 of the strict one --
  a sanity check that it restates the intended arithmetic, not a copy of a kernel.

`patched_state` is shared with tests/test_gpu_relaxed_modes.py."""
import numpy as np
import pytest

PAR = dict(tau=0.25, lam=0.15, theta=0.3)


def patched_state(orc, synth, nx, ny, seed=0):
    """The inner-loop state of test_gpu_tvl1.linearised_state (a synthetic pair warped by a small random flow, random duals) on an
    image of at least 8 x 8, cropped to ny x nx, with two FLAT patches: I1wx = I1wy = 0, p = 0 and u constant.  Inside them |grad u|
    is exactly zero over whole waves -- where the tolerance mode's 2^-600 clamp of the dual update matters -- and stays zero for
    the first iterations (a patch erodes by about one pixel per iteration from its borders).  Patch B touches the right and the
    bottom edge, where the forward gradient is zero by rule."""
    NX, NY = max(nx, 8), max(ny, 8)
    I0, I1 = synth.pair_p1(NX, NY)
    rng = np.random.default_rng(seed)
    u1, u2 = rng.standard_normal((NY, NX)) * 0.5, rng.standard_normal((NY, NX)) * 0.5
    I1x, I1y = orc.centered_gradient(I1)
    I1w, I1wx, I1wy = (orc.bicubic_warp(x, u1, u2, True) for x in (I1, I1x, I1y))
    rho_c = I1w - I1wx * u1 - I1wy * u2 - I0
    p = [rng.standard_normal((NY, NX)) * 0.1 for _ in range(4)]
    crop = lambda a: np.ascontiguousarray(a[:ny, :nx])
    u1, u2, I1wx, I1wy, rho_c = (crop(a) for a in (u1, u2, I1wx, I1wy, rho_c))
    p = [crop(a) for a in p]
    for rows, cols in ((slice(ny // 4, ny // 2), slice(nx // 5, nx - nx // 4)),       # A: interior band
                       (slice(ny - ny // 4, ny), slice(nx - nx // 3, nx))):          # B: bottom-right corner
        I1wx[rows, cols] = 0.0
        I1wy[rows, cols] = 0.0
        u1[rows, cols] = 0.375
        u2[rows, cols] = -1.25
        for a in p:
            a[rows, cols] = 0.0
    grad = I1wx * I1wx + I1wy * I1wy
    return u1, u2, p, I1wx, I1wy, rho_c, grad


SHAPES = [(5, 4), (2, 2), (64, 3), (3, 64), (61, 33), (130, 77)]


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("n_iter", [1, 4])
def test_iterations_mode_off_is_the_reference_iteration(orc, synth, nx, ny, n_iter):
    u1, u2, p, I1wx, I1wy, rho_c, grad = patched_state(orc, synth, nx, ny)
    a = [x.copy() for x in (u1, u2, *p)]
    b = [x.copy() for x in (u1, u2, *p)]
    e_a = orc.tvl1_iterations(*a, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], n_iter)
    e_b = orc.tvl1_iterations_mode(*b, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], n_iter, 0, 0)
    assert e_a == e_b
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))


@pytest.mark.parametrize("pair,nx,ny,nscales,zfactor", [("P0", 64, 48, 3, 0.5), ("P1", 135, 68, 3, 0.75), ("P1", 97, 61, 2, 0.6)])
def test_solves_mode_off_are_the_reference_solves(orc, synth, pair, nx, ny, nscales, zfactor):
    I0, I1 = synth.pair(pair, nx, ny)
    a = orc.tvl1_multiscale(I0, I1, nscales=nscales, zfactor=zfactor, warps=3, **PAR)
    b = orc.tvl1_multiscale_mode(I0, I1, nscales=nscales, zfactor=zfactor, warps=3, relaxed=0, **PAR)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    rng = np.random.default_rng(1)
    u0, v0 = rng.uniform(-2, 2, (ny, nx)), rng.uniform(-2, 2, (ny, nx))
    a = orc.tvl1_single_scale(I0, I1, u0, v0, warps=2, **PAR)
    b = orc.tvl1_single_scale_mode(I0, I1, u0, v0, warps=2, relaxed=0, **PAR)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("nx,ny", [(16, 16), (47, 33), (135, 68)])
def test_gaussian_and_zoom_out_mode_off_are_the_reference(orc, nx, ny):
    a = np.random.default_rng(3).standard_normal((ny, nx)) * 50 + 100
    for sigma in (0.8, 0.6 * np.sqrt(3.0)):
        assert np.array_equal(orc.gaussian_mode(a, sigma, 0), orc.gaussian(a, sigma))
    for f in (0.5, 0.62, 0.75):
        assert np.array_equal(orc.zoom_out_mode(a, f, 0), orc.zoom_out(a, f))


def _is_f32(a):
    return np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), a)


@pytest.mark.parametrize("relaxed", [0, 1])
def test_store_f32_leaves_only_float_values(orc, synth, relaxed):
    nx, ny = 130, 77
    u1, u2, p, I1wx, I1wy, rho_c, grad = patched_state(orc, synth, nx, ny, seed=2)
    st = [x.copy() for x in (u1, u2, *p)]
    assert not all(_is_f32(x) for x in st)
    e = orc.tvl1_iterations_mode(*st, I1wx, I1wy, rho_c, None, PAR["tau"], PAR["lam"], PAR["theta"], 3, relaxed, 1)
    assert np.isfinite(e) and e > 0
    for x in st:
        assert _is_f32(x) and np.isfinite(x).all()
    # the error is the one of the rounded u: one more iteration from the rounded state, by hand
    a = [x.copy() for x in st]
    e1 = orc.tvl1_iterations_mode(*a, I1wx, I1wy, rho_c, None, PAR["tau"], PAR["lam"], PAR["theta"], 1, relaxed, 1)
    d = ((a[0] - st[0]) ** 2 + (a[1] - st[1]) ** 2).sum() / (nx * ny)
    assert abs(e1 - d) <= 1e-12 * d
    img = np.random.default_rng(4).standard_normal((ny, nx)) * 50 + 100
    assert _is_f32(orc.gaussian_mode(img, 0.8, 1))
    for f in (0.5, 0.62):
        assert _is_f32(orc.zoom_out_mode(img, f, 1))
    # float storage is not the double oracle: the rounding really happens
    assert not np.array_equal(orc.gaussian_mode(img, 0.8, 1), orc.gaussian(img, 0.8))


def test_store_f32_rounds_the_intermediate_of_the_two_gaussian_passes(orc):
    """the column pass reads the float-stored row pass: differs from rounding only the double result"""
    img = np.random.default_rng(5).standard_normal((40, 50)).astype(np.float32).astype(np.float64) * 1000
    once = orc.gaussian(img, 1.7).astype(np.float32).astype(np.float64)
    assert not np.array_equal(orc.gaussian_mode(img, 1.7, 1), once)
    assert np.abs(orc.gaussian_mode(img, 1.7, 1) - once).max() <= 4 * np.spacing(np.float32(np.abs(img).max()))


@pytest.mark.parametrize("nx,ny", [(64, 3), (61, 33), (200, 150)])
def test_relaxed_restatement_is_the_strict_algebra_to_1e_13(orc, synth, nx, ny):
    u1, u2, p, I1wx, I1wy, rho_c, grad = patched_state(orc, synth, nx, ny, seed=1)
    a = [x.copy() for x in (u1, u2, *p)]
    b = [x.copy() for x in (u1, u2, *p)]
    e_s = orc.tvl1_iterations(*a, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], 5)
    e_r = orc.tvl1_iterations_mode(*b, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], 5, 1, 0)
    for x, y in zip(a, b):
        assert np.isfinite(y).all()
        assert np.abs(x - y).max() <= 1e-13 * max(1.0, np.abs(x).max())
    assert abs(e_s - e_r) <= 1e-12 * e_s
    # it is a different algebra: some last bits move
    assert any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_relaxed_restatement_keeps_flat_regions_flat(orc, synth):
    """|grad u| = 0 exactly over the patches: the clamp makes 1 + taut g exactly 1, p stays exactly 0 inside"""
    nx, ny = 200, 150
    u1, u2, p, I1wx, I1wy, rho_c, grad = patched_state(orc, synth, nx, ny, seed=1)
    st = [x.copy() for x in (u1, u2, *p)]
    orc.tvl1_iterations_mode(*st, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], 2, 1, 0)
    rows, cols = slice(ny // 4 + 3, ny // 2 - 3), slice(nx // 5 + 3, nx - nx // 4 - 3)
    assert (st[0][rows, cols] == 0.375).all() and (st[1][rows, cols] == -1.25).all()
    for a in st[2:]:
        assert (a[rows, cols] == 0.0).all()


@pytest.mark.parametrize("pair,nx,ny", [("P0", 64, 48), ("P1", 135, 68)])
def test_relaxed_multiscale_close_to_strict(orc, synth, pair, nx, ny):
    I0, I1 = synth.pair(pair, nx, ny)
    us, vs, its, _ = orc.tvl1_multiscale(I0, I1, nscales=3, **PAR)
    ur, vr, itr, _ = orc.tvl1_multiscale_mode(I0, I1, nscales=3, relaxed=1, **PAR)
    assert np.array_equal(its, itr)
    assert np.abs(us - ur).max() < 1e-9 and np.abs(vs - vr).max() < 1e-9
