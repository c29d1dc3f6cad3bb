"""The warm start of the two SOR solvers restated from the checker's pieces (include/ofx.h, "SOR warm start"; CPU only).

The multiscale drivers of src/horn_schunck_pyramidal.cpp:258-370 and src/brox_optic_flow_spatial.cpp:451-549 are composed from
image_normalization_2, gaussian(0.8), zoom_out, the level solver and zoom_in * (1 / z), with the flow of the coarsest level taken
from a .flo payload instead of zero (tests/tvl1_warm_ref.py: start_pyramid, z = zfactor for Horn-Schunck and nu for Brox):

    W_0 = ((double) P.u, (double) P.v), a component that is not finite taken as 0.0
    W_s = zoom_out(W_{s-1}, z) * z                      per component, s = 1 .. nscales - 1, in double
    u, v at the coarsest level = W_{nscales-1}

payload = None is the zero start, i.e. hs_pyramidal / brox_spatial themselves.

`lib` is the Oracle or the compiled reference (oracle.Ref).  The Horn-Schunck level is lib.hs_single_scale, which reads u and v.
No exported checker solves ONE Brox level from a start, so tests/sor_level_shim.c (the checker's source plus one wrapper around its
static brox_single_scale) is built into tests/_build/ and loaded here: a second copy of the checker's process-global state, kept at
one thread; sync_orders() sets the sweep order, tile and wave levels on it that a test set on the oracle.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tvl1_warm_ref import start_pyramid

PRESMOOTH_SIGMA = 0.8               # src/horn_schunck_pyramidal.cpp:22, src/brox_optic_flow_spatial.cpp:26
HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_FLAGS = ["-O3", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile: COMMON

# the shapes of the SOR warm-start tests: (nx, ny, nscales of Horn-Schunck, nscales of Brox, z)
SHAPES = [(67, 45, 3, 3, 0.5), (50, 38, 3, 3, 0.7), (131, 77, 4, 3, 0.5)]

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_shim = None


def shim():
    """tests/_build/libsor_level_shim.so, built on first use (the way tests/test_group_plan.py builds its driver)"""
    global _shim
    if _shim is None:
        out = os.path.join(HERE, "_build", "libsor_level_shim.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        src = os.path.join(HERE, "sor_level_shim.c")
        deps = [src, os.path.join(HERE, "..", "oracle", "ofx_oracle.c"), os.path.join(HERE, "..", "oracle", "ofx_oracle.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            tmp = "%s.%d" % (out, os.getpid())
            r = subprocess.run([os.environ.get("CC", "gcc"), "-std=c11"] + ORACLE_FLAGS + ["-shared", "-o", tmp, src, "-lm"],
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            os.replace(tmp, out)
        L = C.CDLL(out)
        L.orc_set_num_threads.argtypes = [C.c_int]
        L.orc_set_sor_order.argtypes = [C.c_int]
        L.orc_set_sor_tile.argtypes = [C.c_int, C.c_int]
        L.orc_set_sor_wave_levels.argtypes = [C.c_int]
        L.sor_shim_brox_level.restype = None
        L.sor_shim_brox_level.argtypes = [_dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                          C.c_int, C.POINTER(C.c_int), C.c_int]
        L.orc_set_num_threads(1)
        _shim = L
    return _shim


def sync_orders(order=0, tile=(128, 64), wave_levels=0):
    """the sweep order, tile size and wave levels of the shim's copy of the checker (conftest.orc's defaults without arguments)"""
    L = shim()
    L.orc_set_num_threads(1)
    L.orc_set_sor_order(order)
    L.orc_set_sor_tile(*tile)
    L.orc_set_sor_wave_levels(wave_levels)


def brox_level(I1, I2, u, v, level, alpha=50.0, gamma=10.0, TOL=1e-4, inner=1, outer=15, store_f32=0):
    """one Brox level from the start (u, v) -> (u, v, sweeps per solve)"""
    ny, nx = I1.shape
    u, v = np.ascontiguousarray(u, dtype=np.float64).copy(), np.ascontiguousarray(v, dtype=np.float64).copy()
    iters = (C.c_int * max(inner * outer, 1))()
    shim().sor_shim_brox_level(np.ascontiguousarray(I1, dtype=np.float64), np.ascontiguousarray(I2, dtype=np.float64), u, v, nx, ny,
                               alpha, gamma, TOL, inner, outer, level, iters, int(store_f32))
    return u, v, list(iters)[:inner * outer]


def _pyramid(lib, I1, I2, nscales, z):
    a, b = lib.image_normalization_2(I1, I2)
    A, B = [lib.gaussian(a, PRESMOOTH_SIGMA)], [lib.gaussian(b, PRESMOOTH_SIGMA)]
    for _ in range(1, nscales):
        A.append(lib.zoom_out(A[-1], z))
        B.append(lib.zoom_out(B[-1], z))
    return A, B


def _start(lib, payload, shape, nscales, z):
    if payload is None:
        return np.zeros(shape), np.zeros(shape)
    return start_pyramid(lib, payload, nscales, z)


def _multiscale(lib, A, B, u, v, nscales, z, n_solves, level):
    iters = np.zeros((nscales, n_solves), dtype=int)
    for s in range(nscales - 1, -1, -1):
        u, v, it = level(A[s], B[s], u, v, s)
        iters[s] = it
        if s:
            nyy, nxx = A[s - 1].shape
            u = lib.zoom_in(u, nxx, nyy) * (1.0 / z)
            v = lib.zoom_in(v, nxx, nyy) * (1.0 / z)
    return u, v, iters


def hs_pyramidal_warm(lib, I1, I2, payload=None, alpha=7.0, nscales=10, zfactor=0.5, warps=10, TOL=1e-4, maxiter=150):
    """-> (u, v, sweeps (nscales, warps)), as Oracle.hs_pyramidal returns them (the compiled reference reports no sweeps: zeros)"""
    A, B = _pyramid(lib, I1, I2, nscales, zfactor)
    u, v = _start(lib, payload, A[-1].shape, nscales, zfactor)

    def level(a, b, u, v, s):
        r = tuple(lib.hs_single_scale(a, b, u, v, alpha=alpha, warps=warps, TOL=TOL, maxiter=maxiter))
        return r if len(r) == 3 else r + (0,)

    return _multiscale(lib, A, B, u, v, nscales, zfactor, warps, level)


def brox_spatial_warm(lib, I1, I2, payload=None, alpha=50.0, gamma=10.0, nscales=10, nu=0.5, TOL=1e-4, inner=1, outer=15):
    """-> (u, v, sweeps (nscales, inner * outer)), as Oracle.brox_spatial returns them; the levels through the shim"""
    A, B = _pyramid(lib, I1, I2, nscales, nu)
    u, v = _start(lib, payload, A[-1].shape, nscales, nu)

    def level(a, b, u, v, s):
        return brox_level(a, b, u, v, s, alpha=alpha, gamma=gamma, TOL=TOL, inner=inner, outer=outer)

    return _multiscale(lib, A, B, u, v, nscales, nu, inner * outer, level)
