"""Loops that run to their iteration limit, through every loop driver, alone and in a lockstep group of three, in two ways:
"fixed" -- option fixed_work = 1: the stopping test is off (the loop runners pass the kernels a threshold no error falls below) --
and "limit" -- the test is on with a threshold of zero, which no error of these pairs reaches, so the loop ends because nothing is
left to launch.  Either way every loop runs through whole launch units and a shorter last one, and nothing is re-run.  Expected
values: the oracle with a threshold of zero, bit for bit in f64 strict mode -- flows and iteration tables.  130 x 37: three
strips wide, more than one strip high for every marching kernel, several tile rows; the limits (300 iterations, 300 or `maxiter`
sweeps) are no multiples of four or six (41 of none of the unit sizes), so the last unit of most drivers is a short one.

The drivers: TV-L1 with one and two iterations per launch, tiles of K = 4 and 6, three and four per launch (as cursor loops
under "limit"; fixed_work takes their fixed units: the cursor loop needs a stopping test) -- and the Horn-Schunck, Brox and
temporal Brox tiles."""
import contextlib
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NX, NY, G = 130, 37, 3
TVL1 = dict(tau=0.25, lam=0.15, theta=0.3, nscales=2, warps=2)
TVL1_DEFAULTS = dict(fuse2=1, tile=0, fuse3=2, fuse3_min_px=0, fuse4=2, fuse4_min_px=0)
TVL1_DRIVERS = {
    "one": (dict(fuse2=0, fuse3=0, fuse4=0), 1),
    "two": (dict(fuse3=0, fuse4=0), 2),
    "tile4": (dict(tile=4, fuse3=0, fuse4=0), 4),
    "tile6": (dict(tile=6, fuse3=0, fuse4=0), 6),
    "three": (dict(fuse3=1, fuse3_min_px=0, fuse4=0), 3),
    "four": (dict(fuse4=1, fuse4_min_px=0), 4),
}
SOR_DEFAULTS = dict(sor_exact=1, sor_fuse=0, sor_wave_levels=1)


ENDINGS = ["fixed", "limit"]


@contextlib.contextmanager
def options(ctx, ending, defaults, **opts):
    try:
        ctx.set_option("fixed_work", 1 if ending == "fixed" else 0)
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield
    finally:
        ctx.set_option("fixed_work", 0)
        for k in opts:
            ctx.set_option(k, defaults[k])


def _pairs(synth):
    return [synth.pair("P0" if k == 2 else "P1", NX, NY, k) for k in range(G)]


def _on_device(pairs):
    import torch
    d0 = [torch.from_numpy(p[0]).cuda() for p in pairs]
    d1 = [torch.from_numpy(p[1]).cuda() for p in pairs]
    flo = torch.zeros((len(pairs), NY, NX, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return d0, d1, flo


def _ptr(ts):
    return [t.data_ptr() for t in ts]


def _check_group(gpu, st, flo, want):
    gpu.synchronize()
    got = flo.cpu().numpy()
    for k, (uo, vo, it_o) in enumerate(want):
        assert np.array_equal(st[k].iterations(), it_o), k
        assert np.array_equal(got[k], np.stack([uo, vo], axis=-1).astype(np.float32)), k


_want = {}


def _expected(key, make):
    if key not in _want:
        _want[key] = make()
    return _want[key]


@pytest.mark.parametrize("ending", ENDINGS)
@pytest.mark.parametrize("driver", sorted(TVL1_DRIVERS))
def test_tvl1(gpu64, orc, synth, driver, ending):
    opts, unit = TVL1_DRIVERS[driver]
    pairs = _pairs(synth)
    want = _expected("tvl1", lambda: [orc.tvl1_multiscale(p[0], p[1], epsilon=0.0, **TVL1)[:3] for p in pairs])
    assert all((np.asarray(w[2]) == 300).all() for w in want)
    d0, d1, flo = _on_device(pairs)
    eps = 0.01 if ending == "fixed" else 0.0
    with options(gpu64, ending, TVL1_DEFAULTS, **opts):
        u, v = gpu64.tvl1_multiscale(pairs[0][0], pairs[0][1], epsilon=eps, **TVL1)
        s = gpu64.stats()
        assert np.array_equal(s.iterations(), want[0][2]) and np.array_equal(u, want[0][0]) and np.array_equal(v, want[0][1])
        assert list(s.fused[:2]) == [unit, unit], list(s.fused[:2])       # the driver that was asked for really ran
        st = gpu64.tvl1_group_dev(_ptr(d0), _ptr(d1), _ptr(flo), NX, NY, epsilon=eps, **TVL1)
        _check_group(gpu64, st, flo, want)


@pytest.mark.parametrize("ending", ENDINGS)
@pytest.mark.parametrize("K", [2, 4])
def test_hs_tile(gpu64, orc, synth, K, ending):
    kw = dict(alpha=15.0, nscales=2, zfactor=0.5, warps=2, maxiter=41)
    pairs = _pairs(synth)
    orc.set_sor_order(1)
    try:
        want = _expected("hs", lambda: [orc.hs_pyramidal(p[0], p[1], TOL=0.0, **kw) for p in pairs])
    finally:
        orc.set_sor_order(0)
    assert all((np.asarray(w[2]) == 41).all() for w in want)
    d0, d1, flo = _on_device(pairs)
    with options(gpu64, ending, SOR_DEFAULTS, sor_exact=0, sor_fuse=K):
        u, v = gpu64.hs_pyramidal(pairs[0][0], pairs[0][1], TOL=1e-2 if ending == "fixed" else 0.0, **kw)
        assert np.array_equal(gpu64.stats().iterations(), want[0][2]) and np.array_equal(u, want[0][0]) and np.array_equal(v, want[0][1])
        st = gpu64.hs_group_dev(_ptr(d0), _ptr(d1), _ptr(flo), NX, NY, TOL=1e-2 if ending == "fixed" else 0.0, **kw)
        _check_group(gpu64, st, flo, want)


@pytest.mark.parametrize("ending", ENDINGS)
@pytest.mark.parametrize("K", [2, 4])
def test_brox_tile(gpu64, orc, synth, K, ending):
    kw = dict(alpha=50.0, gamma=10.0, nscales=2, nu=0.5, inner=1, outer=2)
    pairs = _pairs(synth)
    orc.set_sor_order(1)
    orc.set_sor_wave_levels(0)
    try:
        want = _expected("brox", lambda: [orc.brox_spatial(p[0], p[1], TOL=0.0, **kw) for p in pairs])
    finally:
        orc.set_sor_order(0)
    assert all((np.asarray(w[2]) == 300).all() for w in want)
    d0, d1, flo = _on_device(pairs)
    with options(gpu64, ending, SOR_DEFAULTS, sor_exact=0, sor_fuse=K, sor_wave_levels=0):
        u, v = gpu64.brox_spatial(pairs[0][0], pairs[0][1], TOL=1e-2 if ending == "fixed" else 0.0, **kw)
        assert np.array_equal(gpu64.stats().iterations(), want[0][2]) and np.array_equal(u, want[0][0]) and np.array_equal(v, want[0][1])
        st = gpu64.brox_group_dev(_ptr(d0), _ptr(d1), _ptr(flo), NX, NY, TOL=1e-2 if ending == "fixed" else 0.0, **kw)
        _check_group(gpu64, st, flo, want)


def _checker():
    spec = importlib.util.spec_from_file_location("broxt_colour_ref", os.path.join(HERE, "broxt_colour_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("ending", ENDINGS)
@pytest.mark.parametrize("K", [2, 4])
def test_temporal_brox_tile(gpu64, oracle_mod, synth, K, ending):
    """expected: the 3-D red-black checker (tests/broxt_colour_ref.py, pinned to the oracle by tests/test_broxt_colour_ref.py)"""
    import torch
    frames, kw = 3, dict(nscales=1, outer=2)
    clips = [synth.sequence(NX, NY, frames, k) for k in range(G)]
    want = _expected("broxt", lambda: [_checker().brox_temporal(oracle_mod, I, 1, TOL=0.0, **kw) for I in clips])
    assert all((np.asarray(w[2]) == 300).all() for w in want)
    dev = [torch.from_numpy(np.ascontiguousarray(I)).cuda() for I in clips]
    flo = torch.zeros((G * (frames - 1), NY, NX, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with options(gpu64, ending, SOR_DEFAULTS, sor_exact=0, sor_fuse=K):
        u, v = gpu64.brox_temporal(clips[0], TOL=1e-2 if ending == "fixed" else 0.0, **kw)
        assert np.array_equal(gpu64.stats().iterations(), want[0][2]) and np.array_equal(u, want[0][0]) and np.array_equal(v, want[0][1])
        st = gpu64.brox_temporal_group_dev([t[f].data_ptr() for t in dev for f in range(frames)], [flo[k].data_ptr() for k in range(flo.shape[0])],
                                           NX, NY, frames, TOL=1e-2 if ending == "fixed" else 0.0, **kw)
        gpu64.synchronize()
        got = flo.cpu().numpy().reshape(G, frames - 1, NY, NX, 2)
        for q, (uo, vo, it_o) in enumerate(want):
            assert np.array_equal(st[q].iterations(), it_o), q
            assert np.array_equal(got[q], np.stack([uo, vo], axis=-1).astype(np.float32)), q
