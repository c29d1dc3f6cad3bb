"""The pyramid head plane by plane: every level that op_build_pyramid_group writes, read back through ofx_pyramid_group_dev.

f64 storage against the oracle's own chain (image_normalization_2, gaussian, zoom_out per pair); f32 storage against the same
chain restated stage by stage with a rounding to float wherever the float instantiation stores an element
(tests/pyramid_head_ref.py, which tests/test_pyramid_head_ref.py holds bit-identical to the oracle without the roundings).  The
sizes put level 0 and level 1 on, one short of and one past the edges of the three tilings of the fused kernels (64 / 128
columns; 32, 24 and 12 rows; the tx < 2 R tail of the staged region), the radii cover every instantiation of k_gauss_xy_gr and
both fallbacks to the unfused kernels, and every pair of a group has a range of its own.

Every comparison is np.array_equal; the guards around every level array must still hold the sentinel and the inputs their
values."""
from contextlib import contextmanager

import numpy as np
import pytest

import pyramid_head_ref as ph

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_SIGMA = 1, 2
DEFAULTS = {"gauss_fused": 1, "input": 0}
MODES = [0, 1, 2, 3]
SIGMA, ZF = 0.8, 0.5

# nx x ny: levels 0 / 1 around 64 and 128 columns, 32 / 24 / 12 rows; 7 is the narrowest legal level for the zoom's radius 5
EDGE_SIZES = [(7, 7), (7, 40), (40, 7), (63, 12), (64, 24), (65, 25), (127, 31), (128, 32), (129, 33), (130, 47), (193, 49), (257, 13)]
F32_SIZES = [(7, 7), (64, 24), (65, 25), (129, 33), (130, 47)]
# presmoothing sigma -> radius; 1.9 is past GXY_RMAX = 8: the unfused kernels in every mode
SIGMAS = [(0.25, 1), (0.5, 2), (0.7, 3), (0.8, 4), (1.0, 5), (1.3, 6), (1.5, 7), (1.7, 8), (1.9, 9)]
# zfactor -> radius of zoom_out's Gaussian; 0.45 is radius 5 without the decimating kernel, 0.3 the whole-pyramid fallback
ZFACTORS = [(0.9, 1), (0.75, 2), (0.62, 3), (0.45, 5), (0.4, 6), (0.35, 8), (0.3, 9)]
RNX, RNY = 97, 45


@contextmanager
def options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, DEFAULTS[k])


def _const_slot(G):
    return None if G == 1 else (G - 1 if G == 2 else G - 2)


def _pair(synth, G, g, nx, ny):
    """pair g of a group of G (float32-representable): P1 (variant g) scaled by 0.2 + 0.05 g and shifted by 3 g, so that a plane
    read for the wrong pair cannot pass; one slot of a group of two or more is constant (both images 7.0: max - min = 0)"""
    if g == _const_slot(G):
        return np.full((ny, nx), 7.0), np.full((ny, nx), 7.0)
    a, b = synth.pair("P1", nx, ny, g)
    return ph.f32(a * (0.2 + 0.05 * g) + 3.0 * g), ph.f32(b * (0.2 + 0.05 * g) + 3.0 * g)


_EXPECTED = {}


def _expected(orc, synth, prec, G, g, nx, ny, nscales, zf, sigma):
    """levels of pair g: ([level s of the first image], [... of the second]); computed once per case, shared, never written"""
    const = g == _const_slot(G)
    key = (prec, nx, ny, "const" if const else g, nscales, zf, sigma)
    if key not in _EXPECTED:
        a, b = _pair(synth, G, g, nx, ny)
        lv = ph.head_oracle(orc, a, b, nscales, zf, sigma) if prec == "f64" else ph.head(orc, a, b, nscales, zf, sigma, ph.f32)
        for plane in lv[0] + lv[1]:
            plane.setflags(write=False)
        _EXPECTED[key] = lv
    return _EXPECTED[key]


def _build(gpu, pairs, nx, ny, nscales, zf, sigma, mode):
    """the levels of `pairs` under gauss_fused = mode -> (L0, L1) as float64; guards and inputs are checked here"""
    import torch
    dt = np.float64 if gpu.precision == 0 else np.float32
    host = [[np.ascontiguousarray(p[k], dtype=dt) for p in pairs] for k in range(2)]
    dev = [[torch.from_numpy(h).cuda() for h in host[k]] for k in range(2)]
    torch.cuda.synchronize()
    with options(gpu, gauss_fused=mode):
        L0, L1, guards = gpu.pyramid_group_dev([t.data_ptr() for t in dev[0]], [t.data_ptr() for t in dev[1]], nx, ny, nscales, zf, sigma)
    assert guards.shape == (nscales, 2, 2, gpu.PYRAMID_GUARD) and (guards == gpu.PYRAMID_SENTINEL).all()
    for k in range(2):
        for t, h in zip(dev[k], host[k]):
            assert np.array_equal(t.cpu().numpy(), h)
    for s, (w, h) in enumerate(ph.level_sizes(nx, ny, nscales, zf)):
        assert L0[s].shape == L1[s].shape == (len(pairs), h, w) and L0[s].dtype == dt
    return [x.astype(np.float64) for x in L0], [x.astype(np.float64) for x in L1]


def _where(got, want):
    """first differing (row, column) and the two values: a mismatch is located by level, plane, row and column"""
    bad = np.argwhere(got != want)
    i, j = bad[0]
    return "%d differ, first at row %d column %d: %r != %r" % (len(bad), i, j, got[i, j], want[i, j])


def _check(gpu, orc, synth, prec, G, nx, ny, nscales, zf, sigma, mode):
    pairs = [_pair(synth, G, g, nx, ny) for g in range(G)]
    L = _build(gpu, pairs, nx, ny, nscales, zf, sigma, mode)
    for g in range(G):
        want = _expected(orc, synth, prec, G, g, nx, ny, nscales, zf, sigma)
        for k in range(2):
            for s in range(nscales):
                got = L[k][s][g]
                assert np.array_equal(got, want[k][s]), "mode %d image %d level %d pair %d: %s" % (mode, k, s, g, _where(got, want[k][s]))
        if g == _const_slot(G):
            assert np.abs(want[0][0] - 7.0).max() < 1e-5           # copied by the normalisation, not mapped to 0 / NaN
        else:
            assert want[0][0].max() - want[0][0].min() > 50.0      # ... and the others are stretched towards 0..255
    return L


# ---- a. tile edges, every schedule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nx,ny", EDGE_SIZES)
def test_tile_edges_every_schedule(gpu64, orc, synth, nx, ny, mode):
    nscales = ph.legal_scales(nx, ny, ZF, SIGMA, 3)
    assert nscales == (3 if min(ph.zoom_size(nx, ny, ZF)) > 6 else 2)
    assert ph.radius(SIGMA) == 4 and ph.radius(ph.zoom_sigma(ZF)) == 5
    _check(gpu64, orc, synth, "f64", 3, nx, ny, nscales, ZF, SIGMA, mode)


# ---- b. every radius -----------------------------------------------------------------------------------------------------------------
def test_the_radii_are_what_the_lists_claim():
    assert [int(5 * s) for s, _ in SIGMAS] == [r for _, r in SIGMAS] == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert [int(5 * ph.zoom_sigma(z)) for z, _ in ZFACTORS] == [r for _, r in ZFACTORS] == [1, 2, 3, 5, 6, 8, 9]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sigma,r", SIGMAS)
def test_every_presmoothing_radius(gpu64, orc, synth, sigma, r, mode):
    assert int(5 * sigma) == r
    for G in (1, 2):
        _check(gpu64, orc, synth, "f64", G, RNX, RNY, 1, ZF, sigma, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("zf,r", ZFACTORS)
def test_every_zoom_radius(gpu64, orc, synth, zf, r, mode):
    assert int(5 * ph.zoom_sigma(zf)) == r and ph.legal_scales(RNX, RNY, zf, SIGMA, 2) == 2
    for G in (1, 2):
        _check(gpu64, orc, synth, "f64", G, RNX, RNY, 2, zf, SIGMA, mode)


# ---- c. group mapping ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2, 16])
def test_plane_g_is_pair_g(gpu64, orc, synth, G):
    nx, ny = 65, 33
    L = _check(gpu64, orc, synth, "f64", G, nx, ny, 2, ZF, SIGMA, 1)
    for g in range(G):
        alone = _build(gpu64, [_pair(synth, G, g, nx, ny)], nx, ny, 2, ZF, SIGMA, 1)
        for k in range(2):
            for s in range(2):
                assert np.array_equal(L[k][s][g], alone[k][s][0]), (k, s, g)
    if G > 2:                                                        # the ranges do tell the planes apart
        assert not np.array_equal(L[0][1][0], L[0][1][2])


# ---- d. float storage ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nx,ny", F32_SIZES)
def test_f32_tile_edges_every_schedule(gpu32, orc, synth, nx, ny, mode):
    _check(gpu32, orc, synth, "f32", 3, nx, ny, ph.legal_scales(nx, ny, ZF, SIGMA, 3), ZF, SIGMA, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sigma,r", SIGMAS)
def test_f32_every_presmoothing_radius(gpu32, orc, synth, sigma, r, mode):
    assert int(5 * sigma) == r
    _check(gpu32, orc, synth, "f32", 2, RNX, RNY, 1, ZF, sigma, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("zf,r", ZFACTORS)
def test_f32_every_zoom_radius(gpu32, orc, synth, zf, r, mode):
    assert int(5 * ph.zoom_sigma(zf)) == r
    _check(gpu32, orc, synth, "f32", 2, RNX, RNY, 2, zf, SIGMA, mode)


def test_f32_expected_values_differ_from_the_rounded_oracle(orc, synth):
    """the staged roundings matter: rounding the oracle's f64 level once is NOT what float storage holds, so the f32 tests above
    could not pass against it"""
    a, b = _pair(synth, 3, 0, 65, 25)
    staged = ph.head(orc, a, b, 2, ZF, SIGMA, ph.f32)
    once = ph.head_oracle(orc, a, b, 2, ZF, SIGMA)
    assert not np.array_equal(staged[0][1], ph.f32(once[0][1]))
    assert np.abs(staged[0][1] - once[0][1]).max() < 1e-3


# ---- e. input kinds ------------------------------------------------------------------------------------------------------------------
def _gray(rgb):
    """the 8-bit rule of OFX_IN_RGB8: three products and two sums, each a float64 operation of its own, then truncation"""
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    s = .299 * r + .587 * g
    s = s + .114 * b
    return s.astype(np.uint8)


@pytest.mark.parametrize("kind", ["U8", "U16", "F32", "RGB8"])
def test_input_kinds_equal_the_storage_type(ofx_mod, gpu64, orc, kind):
    import torch
    nx, ny, G = 65, 25, 2
    rng = np.random.default_rng(21)
    if kind == "U8":
        raw = rng.integers(0, 256, (2 * G, ny, nx), dtype=np.uint8)
    elif kind == "U16":
        raw = rng.integers(0, 65536, (2 * G, ny, nx), dtype=np.uint16)
    elif kind == "F32":
        raw = (rng.integers(0, 65536 * 8, (2 * G, ny, nx)) / 8.0 - 100.0).astype(np.float32)
    else:
        raw = rng.integers(0, 256, (2 * G, ny, nx, 3), dtype=np.uint8)
    raw[2:] = raw[2:] // 3 if kind != "F32" else raw[2:] * np.float32(0.25)   # pair 1: a range of its own
    vals = (_gray(raw) if kind == "RGB8" else raw).astype(np.float64)
    pairs = [(vals[2 * g], vals[2 * g + 1]) for g in range(G)]
    want = _build(gpu64, pairs, nx, ny, 3, ZF, SIGMA, 1)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in raw]
    torch.cuda.synchronize()
    with options(gpu64, input=getattr(ofx_mod, "IN_" + kind)):
        L0, L1, guards = gpu64.pyramid_group_dev([dev[2 * g].data_ptr() for g in range(G)], [dev[2 * g + 1].data_ptr() for g in range(G)],
                                                 nx, ny, 3, ZF, SIGMA)
    assert (guards == gpu64.PYRAMID_SENTINEL).all()
    for d, x in zip(dev, raw):
        assert np.array_equal(d.cpu().numpy(), x)
    for s in range(3):
        assert np.array_equal(L0[s], want[0][s]) and np.array_equal(L1[s], want[1][s]), s
    for g, (a, b) in enumerate(pairs):                               # ... and the storage-type result is the oracle's
        o = ph.head_oracle(orc, a, b, 3, ZF, SIGMA)
        for s in range(3):
            assert np.array_equal(L0[s][g], o[0][s]) and np.array_equal(L1[s][g], o[1][s]), (g, s)


# ---- f. refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(ofx_mod, gpu, G, nx, ny, nscales, status):
    import torch
    img = torch.from_numpy(np.random.default_rng(5).uniform(0.0, 255.0, (ny, nx))).cuda()
    torch.cuda.synchronize()
    with pytest.raises(ofx_mod.OfxError) as e:
        gpu.pyramid_group_dev([img.data_ptr()] * G, [img.data_ptr()] * G, nx, ny, nscales, ZF, SIGMA)
    assert e.value.status == status
    L0, L1, guards = e.value.outputs
    assert len(L0) == len(L1) == nscales and (guards == gpu.PYRAMID_SENTINEL).all()
    for lv in L0 + L1:
        assert lv.shape[0] == G and (lv == gpu.PYRAMID_SENTINEL).all()


def test_refuses_a_level_too_small_for_its_gaussian(ofx_mod, gpu64):
    assert ph.legal_scales(16, 16, ZF, SIGMA, 4) == 3 and ph.level_sizes(16, 16, 4, ZF)[2] == (4, 4)
    _refused(ofx_mod, gpu64, 2, 16, 16, 4, ERR_SIGMA)                # level 3 would be smoothed from 4 x 4 with 6 taps a side
    _refused(ofx_mod, gpu64, 2, 6, 40, 2, ERR_SIGMA)                 # zoom_out's Gaussian: size 6 >= nx
    _refused(ofx_mod, gpu64, 2, 40, 6, 2, ERR_SIGMA)
    _refused(ofx_mod, gpu64, 2, 5, 40, 1, ERR_SIGMA)                 # the presmoothing: size 5 >= nx


def test_refuses_a_group_of_0_or_17(ofx_mod, gpu64, gpu32):
    for gpu in (gpu64, gpu32):
        _refused(ofx_mod, gpu, 0, 65, 25, 2, ERR_ARG)
        _refused(ofx_mod, gpu, 17, 65, 25, 2, ERR_ARG)


def test_refuses_a_null_or_misaligned_image(ofx_mod, gpu64):
    import torch
    nx, ny = 65, 25
    img = torch.from_numpy(np.random.default_rng(6).uniform(0.0, 255.0, (ny, nx + 1))).cuda()
    torch.cuda.synchronize()
    ok = img.data_ptr()
    for d0, d1 in [([ok, None], [ok, ok]), ([ok, ok], [None, ok]), ([ok, ok + 4], [ok, ok]), ([ok, ok], [ok + 2, ok])]:
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.pyramid_group_dev(d0, d1, nx, ny, 2, ZF, SIGMA)
        assert e.value.status == ERR_ARG
        L0, L1, guards = e.value.outputs
        assert (guards == gpu64.PYRAMID_SENTINEL).all() and all((lv == gpu64.PYRAMID_SENTINEL).all() for lv in L0 + L1)


def test_one_more_column_is_accepted(gpu64, orc, synth):
    """the other side of the refusal border: 7 x 40 and 40 x 7 at two levels build (and equal the oracle)"""
    _check(gpu64, orc, synth, "f64", 2, 7, 40, 2, ZF, SIGMA, 1)
    _check(gpu64, orc, synth, "f64", 2, 40, 7, 2, ZF, SIGMA, 1)
