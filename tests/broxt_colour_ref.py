"""Loader of tests/broxt_colour_ref.c: the temporal Brox solver on the CPU in the reference's sweep order (order 0) or the 3-D
red-black order of the GPU's tolerance mode (order 1).  The C file is compiled on first use with the system C compiler (its operators are
oracle/liboracle.so's, resolved when it is loaded), with the oracle's own floating-point flags, into tests/_build/ (git-ignored).
Not used by bench.py or smoke()."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "broxt_colour_ref.c")
OUT = os.path.join(HERE, "_build", "libbroxt_colour_ref.so")
_lib = None


def _build():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = OUT + ".%d.tmp" % os.getpid()
    # the orc_* operators stay undefined here: lib() loads liboracle.so with RTLD_GLOBAL first, wherever the tree lies
    cmd = [os.environ.get("CC", "gcc"), "-std=c11", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared",
           "-o", tmp, SRC, "-lm"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode:
        raise RuntimeError("broxt_colour_ref build failed:\n" + out.stdout + out.stderr)
    os.replace(tmp, OUT)


def lib(oracle_mod):
    """the loaded checker; oracle_mod: the `oracle` package with liboracle.so built"""
    global _lib
    if _lib is None:
        so = oracle_mod.ORACLE_SO
        if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(so)):
            _build()
        C.CDLL(so, mode=C.RTLD_GLOBAL)
        _lib = C.CDLL(OUT)
        dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
        _lib.broxt_colour_ref.restype = C.c_int
        _lib.broxt_colour_ref.argtypes = [dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                          C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        _lib.broxt_colour_ref_mode.restype = C.c_int
        _lib.broxt_colour_ref_mode.argtypes = [dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                               C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return _lib


def brox_temporal(oracle_mod, I, order, alpha=18.0, gamma=7.0, nscales=10, nu=0.75, TOL=1e-4, inner=1, outer=15, store_f32=None):
    """I: (frames, ny, nx).  Returns u, v of shape (frames - 1, ny, nx) and the sweep counts [scale][solve], as Oracle.brox_temporal.
    The oracle's thread count must be 1 (the `orc` fixture sets it): the operators are liboracle.so's.
    store_f32: None = the entry without the switch (broxt_colour_ref); 0 / 1 = broxt_colour_ref_mode in double / float storage
    (the header of broxt_colour_ref.c lists what float storage rounds)."""
    frames, ny, nx = I.shape
    u, v = np.zeros((frames - 1, ny, nx)), np.zeros((frames - 1, ny, nx))
    iters = (C.c_int * (inner * outer * nscales))()
    I = np.ascontiguousarray(I, dtype=np.float64)
    if store_f32 is None:
        rc = lib(oracle_mod).broxt_colour_ref(I, u, v, nx, ny, frames, alpha, gamma, nscales, nu, TOL, inner, outer, order, iters)
    else:
        rc = lib(oracle_mod).broxt_colour_ref_mode(I, u, v, nx, ny, frames, alpha, gamma, nscales, nu, TOL, inner, outer, order,
                                                   int(store_f32), iters)
    if rc == 1:
        raise ValueError("GaussianSmooth: sigma too large")
    if rc:
        raise ValueError("The method needs more than two frames")
    return u, v, np.array(list(iters)).reshape(nscales, inner * outer)
