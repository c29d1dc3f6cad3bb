"""The SOR warm-start restatement (tests/sor_warm_ref.py) against the checkers it is composed from (CPU only).

Recorded, not asserted -- the oracle on synth.sequence(131, 77, 5), reference defaults, one thread, every step started from the
float32 payload of the step before (HS cold on 4 scales, Brox cold on 3):

    solver  nscales_next  sweeps per step warm / cold   pixel-sweeps warm / cold      AEPE warm against cold, px
    HS      1             700-760   / 2608-2796         7.1-7.7 M / 10.2-10.3 M       0.018-0.019
    HS      2             1432-1447 / 2608-2796         8.9-9.1 M / 10.2-10.3 M       0.009-0.019
    Brox    1             622-684   / 1719-1796         6.3-6.9 M / 7.3-8.1 M         4e-4-1.7e-3
    Brox    2             1044-1188 / 1719-1796         6.7-7.7 M / 7.3-8.1 M         1e-5-1.4e-4

(the AEPE is the distance between two answers under one stopping rule, not an error against a truth).
"""
import numpy as np
import pytest

import sor_warm_ref as S
import tvl1_warm_ref as W

IDS = ["%dx%d_%d_%d_%g" % s for s in S.SHAPES]
HS = dict(alpha=7.0, warps=10, TOL=1e-4, maxiter=150)                      # the reference's defaults
BROX = dict(alpha=50.0, gamma=10.0, TOL=1e-4, inner=1, outer=15)


@pytest.fixture(autouse=True)
def _shim_defaults():
    S.sync_orders()


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_zero_start_is_hs_pyramidal_bit_for_bit(orc, synth, shape):
    nx, ny, ns, _, z = shape
    I1, I2 = synth.pair("P1", nx, ny)
    u, v, it = orc.hs_pyramidal(I1, I2, nscales=ns, zfactor=z, **HS)
    for payload in (None, np.zeros((ny, nx, 2), dtype=np.float32)):
        got = S.hs_pyramidal_warm(orc, I1, I2, payload, nscales=ns, zfactor=z, **HS)
        assert np.array_equal(got[0], u) and np.array_equal(got[1], v)
        assert np.array_equal(got[2], it)


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_zero_start_is_brox_spatial_bit_for_bit(orc, synth, shape):
    nx, ny, _, ns, z = shape
    I1, I2 = synth.pair("P1", nx, ny)
    u, v, it = orc.brox_spatial(I1, I2, nscales=ns, nu=z, **BROX)
    for payload in (None, np.zeros((ny, nx, 2), dtype=np.float32)):
        got = S.brox_spatial_warm(orc, I1, I2, payload, nscales=ns, nu=z, **BROX)
        assert np.array_equal(got[0], u) and np.array_equal(got[1], v)
        assert np.array_equal(got[2], it)


def test_the_shim_follows_the_sweep_orders_of_the_oracle(orc, synth):
    """colour order below a checkerboard of tiles on the finest level (the tolerance mode's orders): still brox_spatial bit for bit"""
    nx, ny, _, ns, z = S.SHAPES[2]
    I1, I2 = synth.pair("P1", nx, ny)
    kw = dict(alpha=50.0, gamma=10.0, TOL=1e-4, inner=1, outer=6)
    plain = orc.brox_spatial(I1, I2, nscales=ns, nu=z, **kw)
    orc.set_sor_order(1)
    orc.set_sor_wave_levels(1)
    orc.set_sor_tile(64, 64)
    try:
        S.sync_orders(1, (64, 64), 1)
        u, v, it = orc.brox_spatial(I1, I2, nscales=ns, nu=z, **kw)
        got = S.brox_spatial_warm(orc, I1, I2, None, nscales=ns, nu=z, **kw)
        hu, hv, hit = orc.hs_pyramidal(I1, I2, nscales=ns, zfactor=z, **HS)
        hgot = S.hs_pyramidal_warm(orc, I1, I2, None, nscales=ns, zfactor=z, **HS)
    finally:
        orc.set_sor_order(0)
        orc.set_sor_wave_levels(0)
        orc.set_sor_tile(128, 64)
        S.sync_orders()
    assert np.array_equal(got[0], u) and np.array_equal(got[1], v) and np.array_equal(got[2], it)
    assert np.array_equal(hgot[0], hu) and np.array_equal(hgot[1], hv) and np.array_equal(hgot[2], hit)
    assert not np.array_equal(u, plain[0])                                  # the orders do reach the solve


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_composition_from_the_compiled_reference_is_the_reference(orc, ref, synth, shape):
    nx, ny, hs_ns, bx_ns, z = shape
    I1, I2 = synth.pair("P1", nx, ny)
    u, v = ref.hs_pyramidal(I1, I2, nscales=hs_ns, zfactor=z, **HS)
    got = S.hs_pyramidal_warm(ref, I1, I2, None, nscales=hs_ns, zfactor=z, **HS)
    assert np.array_equal(got[0], u) and np.array_equal(got[1], v)
    u, v = ref.brox_spatial(I1, I2, nscales=bx_ns, nu=z, **BROX)
    got = S.brox_spatial_warm(ref, I1, I2, None, nscales=bx_ns, nu=z, **BROX)      # the reference's pieces, the shim's levels
    assert np.array_equal(got[0], u) and np.array_equal(got[1], v)
    P = W.edge_flow(nx, ny)                                                 # ... and from a start both compositions agree
    a = S.hs_pyramidal_warm(orc, I1, I2, P, nscales=hs_ns, zfactor=z, **HS)
    b = S.hs_pyramidal_warm(ref, I1, I2, P, nscales=hs_ns, zfactor=z, **HS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_a_start_reaches_the_solve_and_a_component_that_is_not_finite_counts_as_zero(orc, synth, shape):
    nx, ny, hs_ns, bx_ns, z = shape
    I1, I2 = synth.pair("P1", nx, ny)
    broken = W.broken_flow(nx, ny)
    mended = np.where(np.isfinite(broken), broken, np.float32(0.0))
    hk = dict(alpha=7.0, warps=4, TOL=1e-4, maxiter=150)
    bk = dict(alpha=50.0, gamma=10.0, TOL=1e-4, inner=1, outer=6)
    for warm, ns, kw, zk in ((S.hs_pyramidal_warm, hs_ns, hk, "zfactor"), (S.brox_spatial_warm, bx_ns, bk, "nu")):
        a = warm(orc, I1, I2, broken, nscales=ns, **{zk: z}, **kw)
        b = warm(orc, I1, I2, mended, nscales=ns, **{zk: z}, **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
        assert not np.array_equal(a[0], warm(orc, I1, I2, None, nscales=ns, **{zk: z}, **kw)[0])


def test_a_pair_restarted_from_its_own_answer_takes_one_sweep_per_solve(orc, synth):
    """P0 at 131x77 on one scale from its own cold payload: every warp / outer iteration stops after its first sweep (the loops
    run a fixed count whatever the start, which is why a warm step may be given fewer)"""
    nx, ny, hs_ns, bx_ns, z = S.SHAPES[2]
    I1, I2 = synth.pair("P0", nx, ny)
    u, v, it = orc.hs_pyramidal(I1, I2, nscales=hs_ns, zfactor=z, **HS)
    warm = S.hs_pyramidal_warm(orc, I1, I2, W.payload_of(u, v), nscales=1, zfactor=z, **HS)
    print("HS sweeps warm %s, cold %d" % (warm[2][0].tolist(), it.sum()))
    assert list(warm[2][0]) == [1] * HS["warps"]
    u, v, it = orc.brox_spatial(I1, I2, nscales=bx_ns, nu=z, **BROX)
    warm = S.brox_spatial_warm(orc, I1, I2, W.payload_of(u, v), nscales=1, nu=z, **BROX)
    print("Brox sweeps warm %s, cold %d" % (warm[2][0].tolist(), it.sum()))
    assert list(warm[2][0]) == [1] * BROX["outer"]


def test_a_video_step_from_the_previous_payload_takes_fewer_sweeps(orc, synth):
    """one step of synth.sequence(131, 77): from the payload of the step before on one scale against cold on all (the table above)"""
    nx, ny, hs_ns, bx_ns, z = S.SHAPES[2]
    F = synth.sequence(nx, ny, 3)
    u, v, _ = orc.hs_pyramidal(F[0], F[1], nscales=hs_ns, zfactor=z, **HS)
    cold = orc.hs_pyramidal(F[1], F[2], nscales=hs_ns, zfactor=z, **HS)[2].sum()
    warm = S.hs_pyramidal_warm(orc, F[1], F[2], W.payload_of(u, v), nscales=1, zfactor=z, **HS)[2].sum()
    print("HS sweeps warm %d, cold %d" % (warm, cold))
    assert warm < cold
    u, v, _ = orc.brox_spatial(F[0], F[1], nscales=bx_ns, nu=z, **BROX)
    cold = orc.brox_spatial(F[1], F[2], nscales=bx_ns, nu=z, **BROX)[2].sum()
    warm = S.brox_spatial_warm(orc, F[1], F[2], W.payload_of(u, v), nscales=1, nu=z, **BROX)[2].sum()
    print("Brox sweeps warm %d, cold %d" % (warm, cold))
    assert warm < cold
