"""robust_expo_methods on colour images (SURVEY 8f.4 at one scale): ofx_robust_expo with nzz > 1 and nscales = 1, and
ofx_robust_expo_single_scale, against recorded results of the compiled reference and against the reference itself.

The bound on the flows, 1e-11, is the one the one-channel solver is held to (tests/test_gpu_sor.py): the sweep tables are
equal and the order of the stopping sum is the only difference."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUND = 1e-11


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_color", os.path.join(GOLDEN, "make_golden_color.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _maker()
CASES = json.load(open(os.path.join(GOLDEN, "cases_color.json")))


def _gpu(gpu64, c, I1, I2, u0, v0):
    if c["entry"] == "multi":
        return gpu64.robust_expo(I1, I2, nscales=1, **c["params"])
    return gpu64.robust_expo_single_scale(I1, I2, u0, v0, **c["params"])


def _report(tag, ug, vg, ur, vr):
    du, dv = float(np.abs(ug - ur).max()), float(np.abs(vg - vr).max())
    print("%s: max|du| = %.3g, max|dv| = %.3g" % (tag, du, dv))
    return du, dv


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture(gpu64, name):
    """1. every recorded case: sweep table equal, flows to < 1e-11"""
    c, g = CASES[name], np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    I1, I2, u0, v0 = MK.inputs(c)
    if c["nz"] == 1:
        I1, I2 = I1[..., 0], I2[..., 0]
    u, v = _gpu(gpu64, c, I1, I2, u0, v0)
    st = gpu64.stats()
    got = list(st.iterations()[0, :len(g["iters"])])
    print(name, "sweeps", got, "reference", list(g["iters"]))
    du, dv = _report(name, u, v, g["u"], g["v"])
    assert got == list(g["iters"])
    assert du < BOUND and dv < BOUND


LIVE = [
    # entry, pair, nx, ny, nz, u0, v0, parameters
    ("multi", "P1", 320, 240, 3, 0, 0, dict(method=1, alpha=50.0, gamma=10.0, lam=0.1, outer=5)),
    ("multi", "P0", 320, 240, 3, 0, 0, dict(method=2, alpha=18.7, gamma=5.0, lam=0.05, outer=4, inner=2)),
    ("multi", "P1", 320, 240, 3, 0, 0, dict(method=3, alpha=30.0, gamma=10.0, lam=1.0, outer=5)),
    ("multi", "P1", 640, 480, 3, 0, 0, dict(method=1, alpha=50.0, gamma=10.0, lam=0.1, outer=4)),
    ("multi", "P1", 131, 67, 3, 0, 0, dict(method=1, alpha=33.3, gamma=10.0, lam=0.1, outer=5)),
    ("multi", "P0", 33, 21, 4, 0, 0, dict(method=2, alpha=7.9, gamma=4.0, lam=0.3, outer=5)),
    ("multi", "P1", 3, 3, 3, 0, 0, dict(method=1, alpha=20.0, gamma=10.0, lam=0.1, outer=3)),
    ("multi", "P1", 96, 64, 3, 0, 0, dict(method=1, alpha=50.0, gamma=0.0, lam=0.1, outer=4)),
    ("single", "P1", 320, 240, 3, 0.75, -0.5, dict(method=1, alpha=150.0, gamma=10.0, lam=0.1, outer=4)),
    ("single", "P0", 131, 67, 2, -0.3, 0.2, dict(method=3, alpha=61.5, gamma=10.0, lam=1.0, outer=4)),
    ("single", "P1", 33, 21, 3, 0, 0, dict(method=2, alpha=40.0, gamma=0.0, lam=0.05, outer=4)),
    ("single", "P1", 3, 3, 4, 0.1, 0.1, dict(method=1, alpha=20.0, gamma=10.0, lam=0.1, outer=3)),
]


@pytest.mark.parametrize("entry,pair,nx,ny,nz,u0,v0,kw", LIVE, ids=["%s-%s-%dx%dx%d-m%d" % (c[0], c[1], c[2], c[3], c[4], c[7]["method"])
                                                                     + ("-g0" if c[7]["gamma"] == 0 else "") for c in LIVE])
def test_live_against_the_reference(gpu64, ref, entry, pair, nx, ny, nz, u0, v0, kw):
    """2. the compiled reference on one thread, now: flows to < 1e-11"""
    c = dict(entry=entry, pair=pair, nx=nx, ny=ny, nz=nz, u0=float(u0), v0=float(v0), params=kw)
    I1, I2, uu, vv = MK.inputs(c)
    ur, vr = MK.run_case(ref.lib, c)
    ug, vg = _gpu(gpu64, c, I1, I2, uu, vv)
    du, dv = _report("%s %s %dx%dx%d" % (entry, pair, nx, ny, nz), ug, vg, ur, vr)
    assert np.isfinite(ur).all() and np.isfinite(vr).all()
    assert du < BOUND and dv < BOUND


@pytest.mark.parametrize("pair,nx,ny,kw", [("P1", 96, 64, dict(method=1, alpha=50.7, gamma=10.0, lam=0.1, outer=4)),
                                           ("P0", 131, 67, dict(method=3, alpha=30.2, gamma=5.0, lam=1.0, outer=3, inner=2))])
def test_one_channel_entries_share_the_solver(gpu64, ref, synth, pair, nx, ny, kw):
    """3. nz = 1: the single-scale entry on normalised, Dirichlet-smoothed planes with a zero flow and the truncated alpha IS
    ofx_robust_expo(nscales = 1) on the raw planes"""
    I1, I2 = synth.pair(pair, nx, ny)
    ua, va = gpu64.robust_expo(I1, I2, nscales=1, **kw)
    ita = gpu64.stats().iterations()[0].copy()
    n1, n2 = ref.image_normalization_2(I1, I2)
    s1, s2 = ref.gaussian_bc(n1, 1.0, 0), ref.gaussian_bc(n2, 1.0, 0)
    kw2 = dict(kw, alpha=float(int(kw["alpha"])))
    z = np.zeros((ny, nx))
    ub, vb = gpu64.robust_expo_single_scale(s1, s2, z, z, **kw2)
    itb = gpu64.stats().iterations()[0]
    assert np.array_equal(ita, itb)
    assert np.array_equal(ua, ub) and np.array_equal(va, vb)
    # and a (ny, nx, 1) image is the plane
    uc, vc = gpu64.robust_expo_single_scale(s1[..., None], s2[..., None], z, z, **kw2)
    assert np.array_equal(ua, uc) and np.array_equal(va, vc)


def test_errors_leave_the_context_usable(gpu64, ofx_mod, synth):
    """4. argument errors: status 1, and the next valid call is served"""
    import ctypes as C
    I1, I2 = synth.colour_pair("P1", 32, 24, 3)
    z = np.zeros((24, 32))
    L, h = gpu64.L, gpu64.h
    dp = C.POINTER(C.c_double)

    def raw_multi(a, b, u, v, nx, ny, nz, method=1, nscales=1):
        return L.ofx_robust_expo(h, a, b, u, v, nx, ny, nz, method, 50.0, 10.0, 0.1, nscales, 0.5, 1e-4, 1, 2, 0)

    def raw_single(a, b, u, v, nx, ny, nz, method=1):
        return L.ofx_robust_expo_single_scale(h, a, b, u, v, nx, ny, nz, method, 50.0, 10.0, 0.1, 1e-4, 1, 2, 1, 0)

    u, v = z.copy(), z.copy()
    for nz in (0, 5, -1):
        assert raw_multi(I1, I2, u, v, 32, 24, nz) == 1
        assert raw_single(I1, I2, u, v, 32, 24, nz) == 1
    assert raw_multi(I1, I2, u, v, 32, 24, 3, nscales=2) == 1
    assert "zoom.cpp:96-118" in ofx_mod.lib().ofx_last_error(h).decode()
    for method in (0, 4):
        assert raw_multi(I1, I2, u, v, 32, 24, 3, method=method) == 1
        assert raw_single(I1, I2, u, v, 32, 24, 3, method=method) == 1
    assert raw_multi(I1, I2, u, v, 2, 2, 3) == 1 and raw_single(I1, I2, u, v, 2, 2, 3) == 1          # smaller than 3x3
    # NULL pointers: ctypes' ndpointer argument types refuse None, so these two calls go through plain pointer types
    for fn, nargs in ((L.ofx_robust_expo, 18), (L.ofx_robust_expo_single_scale, 17)):
        saved = fn.argtypes
        try:
            fn.argtypes = [C.c_void_p, dp, dp, dp, dp] + list(saved[5:])
            ptr = [x.ctypes.data_as(dp) for x in (np.ascontiguousarray(I1), np.ascontiguousarray(I2), u, v)]
            for k in range(4):
                args = list(ptr)
                args[k] = None
                if nargs == 18:
                    rc = fn(h, *args, 32, 24, 3, 1, 50.0, 10.0, 0.1, 1, 0.5, 1e-4, 1, 2, 0)
                else:
                    rc = fn(h, *args, 32, 24, 3, 1, 50.0, 10.0, 0.1, 1e-4, 1, 2, 1, 0)
                assert rc == 1
        finally:
            fn.argtypes = saved
    assert np.array_equal(u, z) and np.array_equal(v, z)          # no failed call wrote a flow
    for bad in (dict(nscales=2), dict(method=0), dict(method=4), dict(inner=-1)):
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.robust_expo(I1, I2, **dict(dict(nscales=1), **bad))
        assert e.value.status == 1
    with pytest.raises(ofx_mod.OfxError) as e:
        gpu64.robust_expo_single_scale(I1, I2, z, z, method=4)
    assert e.value.status == 1
    gpu64.set_option("sor_exact", 0)
    try:
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.robust_expo(I1, I2, nscales=1, outer=2)
        assert e.value.status == 1
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.robust_expo_single_scale(I1, I2, z, z, outer=2)
        assert e.value.status == 1
    finally:
        gpu64.set_option("sor_exact", 1)
    # the context still solves
    name = "rexpoc_m1_p1_64x48x3"
    c, g = CASES[name], np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    a, b, _, _ = MK.inputs(c)
    ug, vg = gpu64.robust_expo(a, b, nscales=1, **c["params"])
    assert np.abs(ug - g["u"]).max() < BOUND and np.abs(vg - g["v"]).max() < BOUND


def test_workspace_reuse_across_channel_counts(gpu64, ofx_mod, synth):
    """5. after a colour solve, a one-channel robust_expo and a brox_spatial on the same context are bit-equal to a fresh context's"""
    P1, P2 = synth.pair("P1", 96, 64)
    C1, C2 = synth.colour_pair("P0", 131, 67, 4)
    kw = dict(method=1, alpha=50.0, gamma=10.0, lam=0.1, nscales=3, outer=4)
    fresh = ofx_mod.Ofx(0, ofx_mod.F64)
    ur, vr = fresh.robust_expo(P1, P2, **kw)
    ub, vb = fresh.brox_spatial(P1, P2, nscales=3, outer=3)
    del fresh
    gpu64.robust_expo(C1, C2, nscales=1, method=2, alpha=20.0, lam=0.1, outer=3)
    u1, v1 = gpu64.robust_expo(P1, P2, **kw)
    assert np.array_equal(u1, ur) and np.array_equal(v1, vr)
    z = np.zeros((67, 131))
    gpu64.robust_expo_single_scale(C1, C2, z + 0.5, z - 0.25, method=3, alpha=60.0, outer=2)
    u2, v2 = gpu64.brox_spatial(P1, P2, nscales=3, outer=3)
    assert np.array_equal(u2, ub) and np.array_equal(v2, vb)
