"""The warm-start restatement (tests/tvl1_warm_ref.py) against the checkers it is composed from (CPU only)."""
import numpy as np
import pytest

import tvl1_warm_ref as W

PAR = dict(tau=0.25, lam=0.15, theta=0.3)
IDS = ["%dx%d_%d_%g" % s for s in W.SHAPES]


@pytest.fixture(scope="module")
def cold(_orc_session, synth):
    """Oracle.tvl1_multiscale on P1 at the three shapes, computed once"""
    _orc_session.set_num_threads(1)
    out = {}
    for nx, ny, nscales, zfactor in W.SHAPES:
        I0, I1 = synth.pair("P1", nx, ny)
        out[(nx, ny)] = (I0, I1, _orc_session.tvl1_multiscale(I0, I1, nscales=nscales, zfactor=zfactor, **PAR))
    return out


@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_zero_start_is_the_multiscale_solve_bit_for_bit(orc, cold, shape):
    nx, ny, nscales, zfactor = shape
    I0, I1, (u, v, it, err) = cold[(nx, ny)]
    for payload in (None, np.zeros((ny, nx, 2), dtype=np.float32)):
        got = W.tvl1_multiscale_warm(orc, I0, I1, payload, nscales=nscales, zfactor=zfactor, **PAR)
        assert np.array_equal(got[0], u) and np.array_equal(got[1], v)
        assert np.array_equal(got[2], it) and np.array_equal(got[3], err)


@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_composition_from_the_compiled_reference_is_the_same(orc, ref, synth, shape):
    nx, ny, nscales, zfactor = shape
    I0, I1 = synth.pair("P1", nx, ny)
    for payload in (W.smooth_flow(nx, ny), W.edge_flow(nx, ny)):
        a = W.tvl1_multiscale_warm(orc, I0, I1, payload, nscales=nscales, zfactor=zfactor, **PAR)
        b = W.tvl1_multiscale_warm(ref, I0, I1, payload, nscales=nscales, zfactor=zfactor, **PAR)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])       # (the reference reports no tables)
        assert not np.array_equal(a[0], W.tvl1_multiscale_warm(orc, I0, I1, None, nscales=nscales, zfactor=zfactor, **PAR)[0])


@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_a_component_that_is_not_finite_counts_as_zero(orc, synth, shape):
    nx, ny, nscales, zfactor = shape
    I0, I1 = synth.pair("P1", nx, ny)
    broken = W.broken_flow(nx, ny)
    assert not np.isfinite(broken).all()
    mended = np.where(np.isfinite(broken), broken, np.float32(0.0))
    for x, y in zip(W.start_pyramid(orc, broken, nscales, zfactor), W.start_pyramid(orc, mended, nscales, zfactor)):
        assert np.array_equal(x, y) and np.isfinite(x).all()
    a = W.tvl1_multiscale_warm(orc, I0, I1, broken, nscales=nscales, zfactor=zfactor, **PAR)
    b = W.tvl1_multiscale_warm(orc, I0, I1, mended, nscales=nscales, zfactor=zfactor, **PAR)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()


@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_a_solve_from_its_own_answer_takes_fewer_iterations(orc, cold, shape):
    """one scale from the pair's own cold payload against the cold solve over all its scales (measured: 62 against 450, 78
    against 431, 51 against 381 inner iterations)"""
    nx, ny, nscales, zfactor = shape
    I0, I1, (u, v, it, _) = cold[(nx, ny)]
    warm = W.tvl1_multiscale_warm(orc, I0, I1, W.payload_of(u, v), nscales=1, zfactor=zfactor, **PAR)
    print("iterations warm %d, cold %d" % (warm[2].sum(), it.sum()))
    assert warm[2].sum() < it.sum()
