"""tests/pyramid_head_ref.py against the oracle on the CPU: without a rounding hook the staged restatement IS the oracle's chain,
bit for bit -- so with the hook it differs from it by the roundings of float storage alone."""
import numpy as np
import pytest

import pyramid_head_ref as ph

SIZES = [(7, 7), (7, 40), (40, 7), (63, 12), (64, 24), (65, 25), (127, 31), (128, 32), (129, 33), (130, 47), (193, 49), (257, 13)]
SIGMAS = [0.25, 0.5, 0.7, 0.8, 1.0, 1.3, 1.5, 1.7, 1.9]


def _img(nx, ny, seed=0):
    return ph.f32(np.random.default_rng(1000 * nx + ny + seed).uniform(-20.0, 300.0, (ny, nx)))


@pytest.mark.parametrize("nx,ny", SIZES)
def test_gaussian_restatement_is_the_oracle(orc, nx, ny):
    a = _img(nx, ny)
    for sigma in SIGMAS:
        if ph.radius(sigma) + 1 >= min(nx, ny):
            with pytest.raises(ValueError):
                orc.gaussian(a, sigma)                   # the refusal border of the restatement is the oracle's
            continue
        assert np.array_equal(ph.gaussian(a, sigma), orc.gaussian(a, sigma)), sigma


@pytest.mark.parametrize("sigma", SIGMAS)
def test_gaussian_restatement_at_the_narrowest_legal_shapes(orc, sigma):
    size = ph.radius(sigma) + 1
    for nx, ny in [(size + 1, size + 1), (size + 1, 40), (40, size + 1)]:
        a = _img(nx, ny, 1)
        assert np.array_equal(ph.gaussian(a, sigma), orc.gaussian(a, sigma)), (nx, ny)


@pytest.mark.parametrize("nx,ny", SIZES)
def test_zoom_out_restatement_is_the_oracle(orc, nx, ny):
    a = _img(nx, ny, 2)
    for zf in (0.5, 0.75, 0.9):
        if ph.radius(ph.zoom_sigma(zf)) + 1 >= min(nx, ny):
            continue
        assert np.array_equal(ph.zoom_out(orc, a, zf), orc.zoom_out(a, zf)), zf
    sm = ph.gaussian(a, ph.zoom_sigma(0.5))
    assert np.array_equal(sm[::2, ::2], orc.zoom_out(a, 0.5))          # what the decimating kernel relies on
    sm = ph.gaussian(a, ph.zoom_sigma(0.5), ph.f32)                    # ... in float storage too: rounded once = sampled and rounded again
    assert np.array_equal(sm[::2, ::2], ph.zoom_out(orc, a, 0.5, ph.f32))


@pytest.mark.parametrize("zf,r", [(0.9, 1), (0.75, 2), (0.62, 3), (0.5, 5), (0.45, 5), (0.4, 6), (0.35, 8), (0.3, 9)])
def test_zoom_radii_and_wide_kernels(orc, zf, r):
    assert ph.radius(ph.zoom_sigma(zf)) == r
    a = _img(97, 45, 3)
    assert np.array_equal(ph.zoom_out(orc, a, zf), orc.zoom_out(a, zf))


def test_head_restatement_is_the_oracles_chain(orc):
    a, b = _img(65, 25, 4) * 0.3 + 3.0, _img(65, 25, 5) * 0.3 + 3.0
    n = ph.legal_scales(65, 25, 0.5, 0.8, 3)
    assert n == 3 and ph.level_sizes(65, 25, 3, 0.5) == [(65, 25), (33, 13), (17, 7)]
    for got, want in zip(ph.head(orc, a, b, n, 0.5, 0.8), ph.head_oracle(orc, a, b, n, 0.5, 0.8)):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    c = np.full((25, 65), 7.0)
    l0, l1 = ph.head(orc, c, c, 2, 0.5, 0.8, ph.f32)
    assert l0[1].shape == (13, 33) and np.abs(l0[1] - 7.0).max() < 1e-5   # a constant pair is copied, not normalised


def test_legal_scales():
    assert ph.legal_scales(7, 7, 0.5, 0.8, 3) == 2 and ph.legal_scales(63, 12, 0.5, 0.8, 3) == 2
    assert ph.legal_scales(257, 13, 0.5, 0.8, 3) == 3 and ph.legal_scales(6, 40, 0.5, 0.8, 2) == 1
    assert ph.legal_scales(16, 16, 0.5, 0.8, 4) == 3 and ph.legal_scales(5, 40, 0.5, 0.8, 2) == 0
