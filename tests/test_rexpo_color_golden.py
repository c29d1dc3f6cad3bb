"""tests/golden/rexpoc_*.npz (robust_expo_methods on colour images, one scale) against the compiled reference that wrote them,
and the determinism of their inputs.  CPU only; skips where the reference is not built."""
import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_color", os.path.join(GOLDEN, "make_golden_color.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _maker()


def test_cases_file_matches_the_generator():
    meta = json.load(open(os.path.join(GOLDEN, "cases_color.json")))
    assert sorted(meta) == sorted(MK.CASES)
    for name, c in MK.CASES.items():
        assert os.path.exists(os.path.join(GOLDEN, name + ".npz")), name
        for k, val in c.items():
            assert meta[name][k] == val, (name, k)
        g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        assert g["u"].shape == (c["ny"], c["nx"]) and g["v"].shape == (c["ny"], c["nx"])
        assert len(g["iters"]) == c["params"]["inner"] * c["params"]["outer"] and int(g["iters"].sum()) == meta[name]["iters"]
        assert np.isfinite(g["u"]).all() and np.isfinite(g["v"]).all()
    # the cases the fixtures are there for: every method, inner > 1, two channels, and the single-scale entry from a zero flow,
    # from a non-zero flow and on one channel
    multi = [c for c in MK.CASES.values() if c["entry"] == "multi"]
    single = [c for c in MK.CASES.values() if c["entry"] == "single"]
    assert {c["params"]["method"] for c in multi if c["nz"] == 3} == {1, 2, 3}
    assert any(c["params"]["inner"] == 2 for c in multi) and any(c["nz"] == 2 for c in multi)
    assert any(c["nz"] == 3 and c["u0"] == 0 and c["v0"] == 0 for c in single)
    assert any(c["nz"] == 3 and c["u0"] != 0 and c["v0"] != 0 for c in single) and any(c["nz"] == 1 for c in single)
    assert all(c["nx"] * c["ny"] <= 96 * 64 for c in MK.CASES.values())


def test_colour_pair_is_deterministic(synth):
    for name, nx, ny, nz in (("P1", 64, 48, 3), ("P0", 33, 21, 4), ("P1", 16, 9, 1), ("P0", 20, 10, 2)):
        a1, a2 = synth.colour_pair(name, nx, ny, nz)
        b1, b2 = synth.colour_pair(name, nx, ny, nz)
        assert a1.shape == (ny, nx, nz) and a1.flags["C_CONTIGUOUS"] and a1.dtype == np.float64
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
        p1, p2 = synth.pair(name, nx, ny)
        assert np.array_equal(a1[..., 0], p1) and np.array_equal(a2[..., 0], p2)
        if nz > 1:                                    # + - * / of the plane only
            assert np.array_equal(a1[..., 1], 0.6 * (255.0 - p1) + 20.0)
        if nz > 2:
            assert np.array_equal(a2[..., 2], p2 * p2 / 255.0)
        assert a1.min() >= 0 and a1.max() <= 255
    with pytest.raises(ValueError):
        synth.colour_pair("P1", 8, 8, 5)


@pytest.mark.parametrize("name", sorted(MK.CASES))
def test_fixture_is_what_the_reference_computes(ref, name):
    """one thread (the `ref` fixture): the only configuration in which the reference repeats itself"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    u, v = MK.run_case(ref.lib, name)
    assert np.array_equal(u, g["u"]) and np.array_equal(v, g["v"])
