"""The TV-L1 warm start restated from the checker's pieces (include/ofx.h, "TV-L1 warm start"; CPU only).

`lib` is the Oracle or the compiled reference (oracle.Ref): both offer image_normalization_2, gaussian, zoom_out, zoom_in and
tvl1_single_scale, which reads u1 / u2 as the initial flow.  The multiscale driver of src/tvl1flow.cpp:219-328 is composed from
them, with the flow at the coarsest level taken from a .flo payload instead of zero:

    W_0 = ((double) P.u, (double) P.v), a component that is not finite taken as 0.0
    W_s = zoom_out(W_{s-1}, zfactor) * zfactor          per component, s = 1 .. nscales - 1, in double
    u, v at the coarsest level = W_{nscales-1}

payload = None is the zero start, i.e. tvl1_multiscale itself.
"""
import numpy as np

PRESMOOTHING_SIGMA = 0.8            # src/tvl1flow.cpp:23


def start_level0(payload):
    """W_0: (u, v) float64 planes of a (ny, nx, 2) float32 payload, non-finite components as 0.0"""
    P = np.asarray(payload, dtype=np.float32)
    W = P.astype(np.float64)
    W[~np.isfinite(W)] = 0.0
    return np.ascontiguousarray(W[..., 0]), np.ascontiguousarray(W[..., 1])


def start_pyramid(lib, payload, nscales, zfactor):
    """W_{nscales-1} as (u, v) float64 planes"""
    u, v = start_level0(payload)
    for _ in range(1, nscales):
        u = lib.zoom_out(u, zfactor) * zfactor
        v = lib.zoom_out(v, zfactor) * zfactor
    return u, v


def tvl1_multiscale_warm(lib, I0, I1, payload=None, tau=0.25, lam=0.15, theta=0.3, nscales=5, zfactor=0.5, warps=5, epsilon=0.01,
                         relaxed=0):
    """-> (u, v, iterations (nscales, warps), errors (nscales, warps)), as Oracle.tvl1_multiscale returns them.
    relaxed = 1: the levels through Oracle.tvl1_single_scale_mode(relaxed=1), the f64 tolerance mode's restatement."""
    a, b = lib.image_normalization_2(I0, I1)
    A, B = [lib.gaussian(a, PRESMOOTHING_SIGMA)], [lib.gaussian(b, PRESMOOTHING_SIGMA)]
    for _ in range(1, nscales):
        A.append(lib.zoom_out(A[-1], zfactor))
        B.append(lib.zoom_out(B[-1], zfactor))
    if payload is None:
        u, v = np.zeros(A[-1].shape), np.zeros(A[-1].shape)
    else:
        u, v = start_pyramid(lib, payload, nscales, zfactor)
    iters, errs = np.zeros((nscales, warps), dtype=int), np.zeros((nscales, warps))
    for s in range(nscales - 1, -1, -1):
        kw = dict(tau=tau, lam=lam, theta=theta, warps=warps, epsilon=epsilon)
        if relaxed:
            u, v, it, er = lib.tvl1_single_scale_mode(A[s], B[s], u, v, relaxed=1, **kw)
        else:
            u, v, it, er = (tuple(lib.tvl1_single_scale(A[s], B[s], u, v, **kw)) + (0, 0.0))[:4]
        iters[s], errs[s] = it, er                          # (the compiled reference returns the flow alone: its tables stay 0)
        if s:
            nyy, nxx = A[s - 1].shape
            u = lib.zoom_in(u, nxx, nyy) * (1.0 / zfactor)
            v = lib.zoom_in(v, nxx, nyy) * (1.0 / zfactor)
    return u, v, iters, errs


def payload_of(u, v):
    """the .flo payload of a flow: (ny, nx, 2) float32"""
    return np.stack([u, v], axis=-1).astype(np.float32)


# the shapes every warm-start test uses: (nx, ny, nscales, zfactor)
SHAPES = [(67, 45, 3, 0.5),         # levels 67x45, 34x23, 17x12: the width crosses one 64-lane boundary
          (50, 38, 3, 0.7),         # the path without the 2:1 kernel
          (131, 77, 4, 0.5)]        # two boundaries, odd everywhere


def smooth_flow(nx, ny, k=0):
    """a smooth flow of a few pixels"""
    i, j = np.mgrid[0:ny, 0:nx].astype(np.float64)
    return payload_of(1.5 + 0.5 * np.sin(0.05 * i + k) + 0.01 * j, -0.75 + 0.25 * np.cos(0.07 * j - k) - 0.02 * i)


def edge_flow(nx, ny):
    """a flow with a step edge (a moving foreground), negative on one side"""
    P = np.zeros((ny, nx, 2), dtype=np.float32)
    P[:, : nx // 3] = (2.25, -1.0)
    P[ny // 2:, nx // 3:] = (-3.5, 0.125)
    return P


def broken_flow(nx, ny):
    """smooth_flow with NaN, +Inf and -Inf entries: isolated, at the corners and the borders, a block and one component only"""
    P = smooth_flow(nx, ny, 1).copy()
    P[0, 0, 0] = np.nan
    P[ny - 1, nx - 1] = (np.inf, -np.inf)
    P[ny // 2, 0, 1] = -np.inf
    P[0, nx // 2] = np.nan
    P[ny // 3: ny // 3 + 4, nx // 2: nx // 2 + 5, 0] = np.inf
    P[ny - 2, 3, 1] = np.nan
    return P
