"""Expected values of the pyramid head (a helper, not a test): image_normalization_2, gaussian(sigma) and the zoom_out chain
restated STAGE BY STAGE in float64, with a rounding hook wherever the float instantiation of the library stores an element of
its storage type:

    the normalised image                        k_normalize_*        stores T
    the row pass of every Gaussian              k_gauss_pass_g<T, true> stores T; the fused kernels round s_mid to T
    the column pass of every Gaussian           stores T (k_gauss_xy_dec: this value IS the level)
    the bicubic sample of the smoothed plane    k_resample_g         stores T

rnd = None is the oracle's own chain (tests/test_pyramid_head_ref.py holds the two bit-identical on the CPU); rnd = f32 is the
contract of float storage.  The taps are ofx_gauss_taps (csrc/ofx_ops.hip) with libm's exp, the sample is the oracle's
bicubic_interpolation_at, called once per output pixel: the levels these helpers are used on are small."""
import math

import numpy as np


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def radius(sigma):
    """int(5 sigma): the Gaussian reaches `radius` samples to each side and has radius + 1 distinct taps"""
    return int(5 * sigma)


def zoom_sigma(zfactor):
    return 0.6 * math.sqrt(1.0 / (zfactor * zfactor) - 1.0)                # ZOOM_SIGMA_ZERO, zoom.cpp:15,60


def zoom_size(nx, ny, zfactor):
    return int(nx * zfactor + 0.5), int(ny * zfactor + 0.5)


def level_sizes(nx, ny, nscales, zfactor):
    s = [(nx, ny)]
    for _ in range(1, nscales):
        s.append(zoom_size(s[-1][0], s[-1][1], zfactor))
    return s


def legal_scales(nx, ny, zfactor, sigma, most):
    """the number of levels <= most that the head builds without a refusal: a Gaussian of radius r needs r + 1 < width, height"""
    if radius(sigma) + 1 >= min(nx, ny):
        return 0
    n, rz = 1, radius(zoom_sigma(zfactor))
    while n < most and rz + 1 < min(nx, ny):
        nx, ny = zoom_size(nx, ny, zfactor)
        if min(nx, ny) < 2:
            break
        n += 1
    return n


def gauss_taps(sigma):
    size = radius(sigma) + 1
    den = 2 * sigma * sigma
    B = [1 / (sigma * math.sqrt(2.0 * 3.1415926)) * math.exp(-i * i / den) for i in range(size)]
    norm = 0.0
    for b in B:
        norm += b
    norm *= 2
    norm -= B[0]
    return [b / norm for b in B]


def _reflect(t, n):
    """left of the image the edge sample is not repeated (-1 -> 1), right of it it is (n -> n - 1)"""
    return np.where(t < 0, -t, np.where(t >= n, 2 * n - 1 - t, t))


def gauss_pass(a, B, axis):
    n = a.shape[axis]
    at = np.arange(n)
    s = B[0] * a
    for k in range(1, len(B)):
        s = s + B[k] * (np.take(a, _reflect(at - k, n), axis=axis) + np.take(a, _reflect(at + k, n), axis=axis))
    return s


def gaussian(a, sigma, rnd=None):
    rnd = rnd or (lambda x: x)
    B = gauss_taps(sigma)
    assert len(B) < min(a.shape), "the library refuses this Gaussian"
    return rnd(gauss_pass(rnd(gauss_pass(a, B, 1)), B, 0))                  # rows first


def zoom_out(orc, a, zfactor, rnd=None):
    rnd = rnd or (lambda x: x)
    ny, nx = a.shape
    sm = np.ascontiguousarray(gaussian(a, zoom_sigma(zfactor), rnd))
    nxx, nyy = zoom_size(nx, ny, zfactor)
    out = np.empty((nyy, nxx))
    for i in range(nyy):
        for j in range(nxx):
            out[i, j] = orc.bicubic_at(sm, j / zfactor, i / zfactor)
    return rnd(out)


def head(orc, a, b, nscales, zfactor, sigma, rnd=None):
    """-> ([levels of a], [levels of b]); a constant pair (max - min = 0) is copied by the normalisation"""
    r = rnd or (lambda x: x)
    out = []
    for x in orc.image_normalization_2(np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)):
        lv = [gaussian(r(x), sigma, rnd)]
        for _ in range(1, nscales):
            lv.append(zoom_out(orc, lv[-1], zfactor, rnd))
        out.append(lv)
    return out[0], out[1]


def head_oracle(orc, a, b, nscales, zfactor, sigma):
    """the same chain through the oracle's own gaussian and zoom_out"""
    out = []
    for x in orc.image_normalization_2(np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)):
        lv = [orc.gaussian(x, sigma)]
        for _ in range(1, nscales):
            lv.append(orc.zoom_out(lv[-1], zfactor))
        out.append(lv)
    return out[0], out[1]
