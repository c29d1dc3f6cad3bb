"""The definition of ofx_structure_texture_dev, pinned on the CPU: the operators of tests/structure_texture_ref.py against the
oracle's, the consequences that include/ofx.h states, and what the decomposition buys a TV-L1 solve under illumination changes.
These tests pin the definition, not the kernel."""
import numpy as np
import pytest

import structure_texture_ref as st


@pytest.mark.parametrize("nx,ny", [(2, 2), (2, 5), (5, 2), (7, 9), (131, 3)])
def test_operators_equal_the_oracle(orc, nx, ny):
    """bit for bit, border associations included (a cumulative-sum formulation is not: this is the test that catches it)"""
    rng = np.random.default_rng(nx * 100 + ny)
    for _ in range(3):
        p1, p2 = rng.uniform(-1.0, 1.0, (ny, nx)), rng.uniform(-1.0, 1.0, (ny, nx))
        assert np.array_equal(st.divergence(p1, p2), orc.divergence(p1, p2))
        fx, fy = st.forward_gradient(p1 * 100.0)
        ox, oy = orc.forward_gradient(p1 * 100.0)
        assert np.array_equal(fx, ox) and np.array_equal(fy, oy)


@pytest.mark.parametrize("kind", ["f64", "u8", "u16", "rgb8"])
def test_no_iteration_writes_the_frame(kind):
    """n_iter = 0 writes S = f, exactly"""
    f = st.frame(67, 45, kind)[1]
    S, T = st.decompose(f, st.theta_for(kind), st.ALPHA, 0)
    assert np.array_equal(S, f)
    assert np.array_equal(T, f - st.ALPHA * f)


@pytest.mark.parametrize("value", [0.0, 37.0, 255.0, -3.25, 1.0 / 3.0])
@pytest.mark.parametrize("n_iter", [0, 1, 5, 37])
def test_a_constant_frame_is_its_own_structure(value, n_iter):
    """a constant frame writes S = f and T = f - alpha f exactly, for every n_iter"""
    f = np.full((9, 13), value)
    S, T = st.decompose(f, 16.0, 0.95, n_iter)
    assert np.array_equal(S, f)
    assert np.array_equal(T, f - 0.95 * f)


def test_float_frames_are_the_rounded_doubles():
    """what an f32 context writes: (float) of the double result, a value the definition fixes -- and the decomposition does something"""
    f = st.frame(67, 45, "u8")[1]
    S, T = st.want(67, 45, "u8", 37)
    assert np.array_equal(T, f - st.ALPHA * S)
    assert np.abs(T.astype(np.float32).astype(np.float64) - T).max() <= np.abs(T).max() * 2.0 ** -24
    assert np.abs(S - f).max() > 1.0 and np.abs(S).max() <= 255.0 + 1e-9
    # total variation falls: S is the smooth part
    tv = lambda a: np.abs(np.diff(a, axis=0)).sum() + np.abs(np.diff(a, axis=1)).sum()
    assert tv(S) < 0.5 * tv(f)


# ---- quality: AEPE against the synthetic truth, raw frames against texture frames -----------------------------------------------
_AEPE = {}


def _aepe(orc, synth, name, change):
    """(raw, texture) for the case, computed once"""
    key = (name, change)
    if key not in _AEPE:
        I0, I1 = st.quality_pair(synth, name, change)
        u, v = orc.tvl1_multiscale(I0, I1, nscales=4)[:2]
        ut, vt = orc.tvl1_multiscale(st.texture(I0), st.texture(I1), nscales=4)[:2]
        _AEPE[key] = (st.aepe_truth(synth, name, u, v), st.aepe_truth(synth, name, ut, vt))
        print("AEPE %s %s: raw %.4f texture %.4f" % (name, change, *_AEPE[key]))
    return _AEPE[key]


@pytest.mark.parametrize("change", ["gain_ramp", "shadow"])
@pytest.mark.parametrize("name", ["P0", "P1"])
def test_texture_frames_survive_an_illumination_change(orc, synth, name, change):
    raw, tex = _aepe(orc, synth, name, change)
    assert tex <= 0.25 * raw, (name, change, raw, tex)


@pytest.mark.parametrize("name", ["P0", "P1"])
def test_texture_frames_cost_an_unchanged_pair_nothing(orc, synth, name):
    raw, tex = _aepe(orc, synth, name, "unchanged")
    assert tex <= raw + 0.03, (name, raw, tex)
