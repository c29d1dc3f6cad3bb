"""TV-L1 with a median filter on the flow after every warp, and the median of a .flo payload, restated (CPU only).

1. The multiscale TV-L1 driver of src/tvl1flow.cpp:46-328 composed from the Oracle's pieces -- image_normalization_2, gaussian,
   zoom_out, centered_gradient, bicubic_warp (border_out = True), tvl1_iterations(n_iter = 1) in a loop, zoom_in -- so that a step
   can be put between two warps.  median = 0 is Oracle.tvl1_multiscale bit for bit (tests/test_tvl1_median_ref.py); median = 3 | 5
   replaces u and v by Oracle.median_filtering after the inner loop of every warp at every level (Wedel et al. 2009, section 3.2;
   option "tvl1_median" of include/ofx.h), the duals untouched.  relaxed = 1 takes the inner iteration from
   tvl1_iterations_mode(relaxed = 1), the f64 tolerance mode's restatement.

2. The median of include/ofx.h ("Median of a flow") in numpy: the windows gathered with mirrored indices and np.sort, with and
   without a map.

Also the inputs the tests around it share."""
import functools

import numpy as np

PRESMOOTHING_SIGMA = 0.8            # src/tvl1flow.cpp:23
MAX_ITERATIONS = 300                # src/tvl1flow.cpp:22


def single_scale(lib, I0, I1, u, v, median=0, tau=0.25, lam=0.15, theta=0.3, warps=5, epsilon=0.01, relaxed=0):
    """src/tvl1flow.cpp:46-212 -> (u, v, iterations per warp, error per warp)"""
    I0, I1 = np.ascontiguousarray(I0, dtype=np.float64), np.ascontiguousarray(I1, dtype=np.float64)
    u, v = np.array(u, dtype=np.float64, order="C"), np.array(v, dtype=np.float64, order="C")
    I1x, I1y = lib.centered_gradient(I1)
    p11, p12, p21, p22 = (np.zeros(I0.shape) for _ in range(4))
    iters, errs = [], []
    for _ in range(warps):
        I1w = lib.bicubic_warp(I1, u, v, True)
        I1wx = lib.bicubic_warp(I1x, u, v, True)
        I1wy = lib.bicubic_warp(I1y, u, v, True)
        grad = I1wx * I1wx + I1wy * I1wy
        rho_c = ((I1w - I1wx * u) - I1wy * v) - I0
        it, error = 0, np.inf
        while error > epsilon * epsilon and it < MAX_ITERATIONS:
            it += 1
            if relaxed:
                error = lib.tvl1_iterations_mode(u, v, p11, p12, p21, p22, I1wx, I1wy, rho_c, grad, tau, lam, theta, 1, relaxed=1)
            else:
                error = lib.tvl1_iterations(u, v, p11, p12, p21, p22, I1wx, I1wy, rho_c, grad, tau, lam, theta, 1)
        iters.append(it)
        errs.append(error)
        if median:
            u, v = lib.median_filtering(u, median), lib.median_filtering(v, median)
    return u, v, iters, errs


def tvl1_multiscale_median(lib, I0, I1, median=0, tau=0.25, lam=0.15, theta=0.3, nscales=5, zfactor=0.5, warps=5, epsilon=0.01,
                           relaxed=0, start=None):
    """-> (u, v, iterations (nscales, warps), errors (nscales, warps)), as Oracle.tvl1_multiscale returns them.
    start: None, or the (u, v) planes at the coarsest level (tvl1_warm_ref.start_pyramid)"""
    a, b = lib.image_normalization_2(I0, I1)
    A, B = [lib.gaussian(a, PRESMOOTHING_SIGMA)], [lib.gaussian(b, PRESMOOTHING_SIGMA)]
    for _ in range(1, nscales):
        A.append(lib.zoom_out(A[-1], zfactor))
        B.append(lib.zoom_out(B[-1], zfactor))
    u, v = (np.zeros(A[-1].shape), np.zeros(A[-1].shape)) if start is None else start
    iters, errs = np.zeros((nscales, warps), dtype=int), np.zeros((nscales, warps))
    for s in range(nscales - 1, -1, -1):
        u, v, iters[s], errs[s] = single_scale(lib, A[s], B[s], u, v, median, tau, lam, theta, warps, epsilon, relaxed)
        if s:
            nyy, nxx = A[s - 1].shape
            u = lib.zoom_in(u, nxx, nyy) * (1.0 / zfactor)
            v = lib.zoom_in(v, nxx, nyy) * (1.0 / zfactor)
    return u, v, iters, errs


# ---- the median of a payload ---------------------------------------------------------------------------------------------------------
def mirror(idx, n):
    """-k -> k - 1, n - 1 + k -> n - k"""
    idx = np.where(idx < 0, -idx - 1, idx)
    return np.where(idx >= n, 2 * n - 1 - idx, idx)


def median_plane(x, wsize, occ=None):
    """one component: (ny, nx) of any float dtype -> the same dtype.  occ: None or (ny, nx) bytes, 0 = valid"""
    ny, nx = x.shape
    r = wsize // 2
    assert r <= nx and r <= ny
    ii = mirror(np.arange(-r, ny + r), ny)
    jj = mirror(np.arange(-r, nx + r), nx)
    pad = x[np.ix_(ii, jj)]
    win = np.stack([pad[a:a + ny, b:b + nx] for a in range(wsize) for b in range(wsize)], axis=-1)         # (ny, nx, W * W)
    if occ is None:
        return np.sort(win, axis=-1)[..., wsize * wsize // 2]
    opad = np.asarray(occ)[np.ix_(ii, jj)]
    valid = np.stack([opad[a:a + ny, b:b + nx] == 0 for a in range(wsize) for b in range(wsize)], axis=-1)
    cnt = valid.sum(axis=-1)
    # np.sort puts NaN last; an invalid position must come behind every valid one, valid NaNs included: sort by (invalid, value)
    order = np.lexsort((win, ~valid), axis=-1)
    srt = np.take_along_axis(win, order, axis=-1)
    out = np.take_along_axis(srt, (cnt // 2)[..., None], axis=-1)[..., 0]
    return np.where(cnt == 0, x, out)


def median_payload(P, wsize, occ=None):
    """(ny, nx, 2) float32 -> (ny, nx, 2) float32"""
    P = np.asarray(P, dtype=np.float32)
    return np.stack([median_plane(P[..., 0], wsize, occ), median_plane(P[..., 1], wsize, occ)], axis=-1)


def same(a, b):
    """== plus equal NaN positions"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(np.isnan(a), np.isnan(b))) and bool(np.all((a == b) | np.isnan(a)))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def impulses(I, a, b, m, hi):
    """the pixels with (a i + b j) % m == 0 set to hi"""
    ny, nx = I.shape
    i, j = np.mgrid[0:ny, 0:nx]
    out = I.copy()
    out[(a * i + b * j) % m == 0] = hi
    return out


IMPULSES = {"clean": None, "1/53": (53, 59, 61, 67), "1/23": (23, 29, 31, 37)}


def noisy_pair(synth, name, kind, nx=160, ny=120):
    I0, I1 = synth.pair(name, nx, ny)
    m = IMPULSES[kind]
    if m is None:
        return I0, I1
    I0 = impulses(impulses(I0, 7, 13, m[0], 255.0), 11, 5, m[1], 0.0)
    I1 = impulses(impulses(I1, 3, 17, m[2], 255.0), 13, 7, m[3], 0.0)
    return I0, I1


def maps(nx, ny):
    """name -> byte map, for the masked cases: all valid, all flagged, a hole larger than a 7 x 7 window, a flagged border column"""
    hole = np.zeros((ny, nx), dtype=np.uint8)
    hole[max(ny // 2 - 5, 0): ny // 2 + 5, max(nx // 2 - 6, 0): nx // 2 + 6] = 255
    hole[0, 0] = 1                                                # any non-zero byte flags
    col = np.zeros((ny, nx), dtype=np.uint8)
    col[:, 0] = 255
    col[ny // 2, nx - 1] = 7
    return {"zero": np.zeros((ny, nx), dtype=np.uint8), "all": np.full((ny, nx), 255, dtype=np.uint8), "hole": hole, "column": col}


@functools.lru_cache(maxsize=None)
def solve(orc_key, name, k, nx, ny, nscales, zfactor, median, relaxed=0):
    """the restatement's (payload, iteration table) for synth.pair(name, nx, ny, k), computed once per session; read-only.
    orc_key: (oracle, synth) in a tuple that hashes by identity"""
    orc, synth = orc_key
    I0, I1 = synth.pair(name, nx, ny, k)
    u, v, it, _ = tvl1_multiscale_median(orc, I0, I1, median, nscales=nscales, zfactor=zfactor, relaxed=relaxed)
    P = np.stack([u, v], axis=-1)
    P.setflags(write=False)
    return P, it
