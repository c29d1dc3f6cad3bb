"""GPU parity of the temporal Brox solver's tolerance mode (option sor_exact = 0; k_broxt_rb and k_broxt_tile, csrc/ofx_sor_tile.hip).

The mode sweeps the nz = frames - 1 flow fields of a level in a 3-D red-black order: every voxel with (i + j + f) even, then every
voxel with (i + j + f) odd.  A colour step is a parallel map, so the result depends on nothing but the order, and the expected
value is the CPU checker tests/broxt_colour_ref.c in order 1 (pinned to the oracle in order 0 by tests/test_broxt_colour_ref.py):
flows and sweep tables are compared with np.array_equal for every number of sweeps per launch (sor_fuse = 0, 1, 2, 4) and for the
per-colour kernel (sor_fuse = 9).  Against the reference's own order the bar is the project's: AEPE < 1e-4 px."""
import contextlib
import importlib.util
import os

import numpy as np
import pytest

from conftest import aepe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FUSE = (0, 1, 2, 4, 9)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CK = _load("broxt_colour_ref", os.path.join(HERE, "broxt_colour_ref.py"))
_cache = {}


def _expected(oracle_mod, synth, nx, ny, frames, kw):
    """the checker in order 1, computed once per case"""
    key = (nx, ny, frames, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = CK.brox_temporal(oracle_mod, synth.sequence(nx, ny, frames), 1, **kw)
    return _cache[key]


@contextlib.contextmanager
def _tolerance(*ctxs):
    for c in ctxs:
        c.set_option("sor_exact", 0)
    try:
        yield
    finally:
        for c in ctxs:
            c.set_option("sor_exact", 1)
            c.set_option("sor_fuse", 0)


@pytest.fixture
def tol(gpu64, gpu32):
    """both contexts in the tolerance mode; sor_exact and sor_fuse back to the defaults afterwards"""
    with _tolerance(gpu64, gpu32):
        yield


SHAPES = [
    (6, 6, 3, dict(nscales=1)),             # nz = 2: no interior field, both one-sided temporal taps adjacent
    (7, 6, 4, dict(nscales=1)),             # nz = 3, odd width
    (33, 47, 4, dict(nscales=2)),
    (135, 68, 5, dict(nscales=2)),          # several tiles both ways, sizes no multiple of a tile's output
    (130, 9, 3, dict(nscales=1)),           # fewer rows than a tile's halo
    (24, 20, 10, dict(nscales=1)),          # nz = 9: more fields than a tile holds, the per-colour kernel for every sor_fuse
]


@pytest.mark.parametrize("nx,ny,frames,kw", SHAPES)
def test_equals_the_checker_for_every_fuse(tol, gpu64, oracle_mod, orc, synth, nx, ny, frames, kw):
    uc, vc, it_c = _expected(oracle_mod, synth, nx, ny, frames, kw)
    I = synth.sequence(nx, ny, frames)
    assert uc.any() and it_c.sum() > 0
    for K in FUSE:
        gpu64.set_option("sor_fuse", K)
        ug, vg = gpu64.brox_temporal(I, **kw)
        assert np.array_equal(gpu64.stats().iterations(), it_c), (K, gpu64.stats().iterations(), it_c)
        assert np.array_equal(ug, uc) and np.array_equal(vg, vc), K


@pytest.mark.parametrize("K", [2, 4])
def test_loop_ends(tol, gpu64, oracle_mod, orc, synth, K):
    """a stop before the first sweep, on the first, a middle and the last sweep of a launch unit, and at the iteration limit"""
    gpu64.set_option("sor_fuse", K)
    I = synth.sequence(150, 97, 4)
    seen = set()
    for TOL in (2000.0, 0.3, 1e-2, 1e-3, 3e-4, 0.0):
        kw = dict(nscales=1, outer=2, TOL=TOL)
        uc, vc, it_c = _expected(oracle_mod, synth, 150, 97, 4, kw)
        ug, vg = gpu64.brox_temporal(I, **kw)
        it_g = gpu64.stats().iterations()
        print("K", K, "TOL", TOL, "sweeps", it_g.ravel(), "checker", it_c.ravel())
        assert np.array_equal(it_g, it_c), TOL
        assert np.array_equal(ug, uc) and np.array_equal(vg, vc), TOL
        seen.update(int(n) for n in it_c.ravel())
    assert 0 in seen and 300 in seen


def test_float_storage(tol, gpu32, orc, synth):
    """float storage through the same kernels: as close to the double reference as the exact mode's float storage (1e-3).  This
    is the coarse guard only -- a temporal weight taken from the wrong field in the float instantiation stays under it.  What the
    right float answer is, bit for bit, is pinned by tests/test_gpu_sor_f32_temporal_rexpo.py against tests/broxt_colour_ref.c
    with store_f32 = 1; on this input that restatement drifts 1.0e-5 from the double checker (tests/test_broxt_colour_ref.py)."""
    I = synth.sequence(160, 120, 4)
    uo, vo, _ = orc.brox_temporal(I, nscales=3)
    ug, vg = gpu32.brox_temporal(I, nscales=3)
    e = aepe(ug, vg, uo, vo)
    print("f32 storage, tolerance mode: AEPE vs reference order %.3e" % e)
    assert e < 1e-3


def test_inside_the_parity_bar(tol, gpu64, orc, synth):
    I = synth.sequence(160, 120, 4)
    uo, vo, it_o = orc.brox_temporal(I, nscales=3)
    ug, vg = gpu64.brox_temporal(I, nscales=3)
    it_g = gpu64.stats().iterations()
    e = aepe(ug, vg, uo, vo)
    print("tolerance mode: AEPE vs reference order %.3e, sweeps %d vs %d" % (e, it_g.sum(), it_o.sum()))
    assert not np.array_equal(ug, uo)
    assert e < 1e-4
    assert abs(int(it_g.sum()) - int(it_o.sum())) <= 0.1 * it_o.sum()


def test_default_untouched(gpu64, orc, synth):
    """after a tolerance-mode solve and the fixture's restore the exact branch runs again: the oracle bit for bit"""
    I = synth.sequence(40, 33, 4)
    kw = dict(nscales=2, outer=3)
    with _tolerance(gpu64):
        ut, vt = gpu64.brox_temporal(I, **kw)
    uo, vo, it_o = orc.brox_temporal(I, **kw)
    ug, vg = gpu64.brox_temporal(I, **kw)
    assert np.array_equal(gpu64.stats().iterations(), it_o)
    assert np.array_equal(ug, uo) and np.array_equal(vg, vo)
    assert not np.array_equal(ut, uo)
