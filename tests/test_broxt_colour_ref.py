"""The CPU checker of the temporal Brox solver's two sweep orders (tests/broxt_colour_ref.c) is pinned before anything uses it:

1. in order 0 (the reference's sweep order) it IS oracle.brox_temporal, bit for bit -- and the oracle is pinned to the compiled
   reference by tests/test_oracle_vs_ref.py;
2. in order 1 (3-D red-black, the order of the GPU's tolerance mode, option sor_exact = 0) it stays inside the project's parity
   bar, an average end-point error below 1e-4 px against the reference's order, with about the same number of sweeps."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import aepe

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CK = _load("broxt_colour_ref", os.path.join(HERE, "broxt_colour_ref.py"))


@pytest.mark.parametrize("nx,ny,frames,kw", [
    (6, 6, 3, dict(nscales=1)),                             # nz = 2: no interior field
    (40, 33, 4, dict(nscales=2, outer=3)),
])
def test_order_0_is_the_oracle(oracle_mod, orc, synth, nx, ny, frames, kw):
    I = synth.sequence(nx, ny, frames)
    uo, vo, it_o = orc.brox_temporal(I, **kw)
    uc, vc, it_c = CK.brox_temporal(oracle_mod, I, 0, **kw)
    assert np.array_equal(it_c, it_o)
    assert np.array_equal(uc, uo) and np.array_equal(vc, vo)
    assert uo.any() and it_o.sum() > 0


def test_colour_order_is_inside_the_parity_bar(oracle_mod, orc, synth):
    I = synth.sequence(160, 120, 4)
    kw = dict(nscales=3)
    uo, vo, it_o = orc.brox_temporal(I, **kw)
    uc, vc, it_c = CK.brox_temporal(oracle_mod, I, 1, **kw)
    e = aepe(uc, vc, uo, vo)
    print("AEPE colour order vs reference order %.3e, sweeps %d vs %d" % (e, it_c.sum(), it_o.sum()))
    assert not np.array_equal(uc, uo)                       # another order, not the same one twice
    assert e < 1e-4
    assert abs(int(it_c.sum()) - int(it_o.sum())) <= 0.1 * it_o.sum()
    # what this checker gives here: AEPE 1.42e-5, 2030 sweeps against 2049.  Twice that value is the guard against a restatement
    # that drifts while staying under the bar.
    assert e < 2 * 1.42e-5


# ---- the float-storage switch (broxt_colour_ref_mode; the header of broxt_colour_ref.c lists what is rounded) ------------------------
MODE_SHAPES = [(6, 6, 3, dict(nscales=1, outer=3)),                 # nz = 2: no interior field
               (33, 47, 4, dict(nscales=2, outer=3, inner=2)),
               (24, 20, 10, dict(nscales=1, outer=2))]               # nz = 9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _is_f32(a):
    return np.array_equal(_bits(a), _bits(np.asarray(a).astype(np.float32).astype(np.float64)))


@pytest.mark.parametrize("nx,ny,frames,kw", MODE_SHAPES)
def test_mode_off_is_the_existing_entry(oracle_mod, orc, synth, nx, ny, frames, kw):
    """store_f32 = 0 is the entry without the switch in both orders, sweep tables included, and in order 0 the oracle.  (The entry
    without the switch now calls the other with 0; what holds order 1 where it was is tests/test_gpu_broxt_tile.py, which compares
    the GPU's double solve with it bit for bit.)"""
    I = synth.sequence(nx, ny, frames)
    for order in (0, 1):
        u0, v0, it0 = CK.brox_temporal(oracle_mod, I, order, **kw)
        u1, v1, it1 = CK.brox_temporal(oracle_mod, I, order, store_f32=0, **kw)
        assert np.array_equal(it0, it1) and it0.sum() > 0
        assert np.array_equal(_bits(u0), _bits(u1)) and np.array_equal(_bits(v0), _bits(v1))
        if order == 0:
            uo, vo, it_o = orc.brox_temporal(I, **kw)
            assert np.array_equal(it1, it_o)
            assert np.array_equal(_bits(u1), _bits(uo)) and np.array_equal(_bits(v1), _bits(vo))


@pytest.mark.parametrize("nx,ny,frames,kw", MODE_SHAPES)
def test_float_storage_leaves_floats(oracle_mod, orc, synth, nx, ny, frames, kw):
    I = synth.sequence(nx, ny, frames) + 0.3                  # no floats: the entry rounds them
    for order in (0, 1):
        u, v, it = CK.brox_temporal(oracle_mod, I, order, store_f32=1, **kw)
        assert np.isfinite(u).all() and np.isfinite(v).all() and u.any() and v.any() and it.sum() > 0
        assert _is_f32(u) and _is_f32(v)


def test_float_storage_differs_from_double(oracle_mod, orc, synth):
    """the switch does something: a float solve is not the double solve rounded at the end"""
    I = synth.sequence(33, 47, 4)
    for order in (0, 1):
        d = CK.brox_temporal(oracle_mod, I, order, store_f32=0, nscales=2, outer=3)
        f = CK.brox_temporal(oracle_mod, I, order, store_f32=1, nscales=2, outer=3)
        assert not np.array_equal(_bits(f[0]), _bits(d[0].astype(np.float32).astype(np.float64)))


# temporal Brox in float storage against the double checker of the same order, measured with this restatement on the CPU
# (160x120x4, three scales, the shape of tests/test_gpu_broxt_tile.py::test_float_storage): order: (AEPE, max |delta|)
BROXT_DRIFT = {0: (4.180e-07, 5.176e-03), 1: (1.028e-05, 1.762e-02)}


@pytest.mark.parametrize("order", [0, 1])
def test_float_storage_stays_in_the_band(oracle_mod, orc, synth, order):
    """the project's bar for float storage (1e-3) and, beside it, 10 x the drift measured on this input: solves that stop
    unconverged amplify a rounding differently per input, hence the factor (as BROX_DRIFT in tests/test_oracle_sor_f32.py)"""
    I = synth.sequence(160, 120, 4)
    ud, vd, _ = CK.brox_temporal(oracle_mod, I, order, store_f32=0, nscales=3)
    uf, vf, _ = CK.brox_temporal(oracle_mod, I, order, store_f32=1, nscales=3)
    drift, worst = aepe(uf, vf, ud, vd), max(float(np.abs(uf - ud).max()), float(np.abs(vf - vd).max()))
    print("order %d: AEPE %.3e, max |delta| %.3e" % (order, drift, worst))
    assert drift < 1e-3
    assert drift < 10 * BROXT_DRIFT[order][0], (drift, BROXT_DRIFT[order])
    assert worst < 10 * BROXT_DRIFT[order][1], (worst, BROXT_DRIFT[order])
