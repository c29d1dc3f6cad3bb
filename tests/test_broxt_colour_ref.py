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
