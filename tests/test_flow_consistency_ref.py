"""The inputs of the consistency tests, pinned on the CPU: what keeps tests/test_gpu_flow_consistency.py from passing vacuously.

Every case must flag a real share of its pixels in EACH map -- between 5 % and 95 % -- and no pixel may sit on the threshold:
the smallest relative margin |lhs - rhs| / rhs over the pixels that reach the comparison must exceed 1e-9, seven orders above a
last-bit difference of the two sides, so the device maps can be required to be EQUAL to the restatement.

Measured: P1 64 x 48 (3 scales) 8.1 % forward / 8.0 % backward, margin 5.9e-5; P1 37 x 29 (2 scales) 16.6 % / 16.6 %, margin
1.0e-2; the seeded sine-plus-noise payloads 45 .. 87 %, margins >= 6e-5 (2 x 2: 75 %, three of four vectors leave)."""
import numpy as np
import pytest

import flow_consistency_ref as fcr


@pytest.mark.parametrize("name", fcr.ALL_CASES)
def test_case_is_not_vacuous(orc, synth, name):
    fwd, bwd = fcr.case_payloads(orc, synth, name)
    of, ob, margin = fcr.case_maps(orc, synth, name)
    nx, ny = fwd.shape[1], fwd.shape[0]
    assert of.shape == ob.shape == (ny, nx) and of.dtype == np.uint8
    assert set(np.unique(of)) <= {0, 255} and set(np.unique(ob)) <= {0, 255}
    sf, sb = float((of == 255).mean()), float((ob == 255).mean())
    print("%s: %.1f %% forward, %.1f %% backward, margin %.3g" % (name, 100 * sf, 100 * sb, margin))
    assert 0.05 <= sf <= 0.95 and 0.05 <= sb <= 0.95, (sf, sb)
    assert margin > 1e-9, margin


def test_main_case_is_the_oracles_tvl1(orc, synth):
    """the main case is what it says: the oracle's flows of P1 at 64 x 48 in both directions, rounded to float32"""
    A, B = synth.pair("P1", 64, 48)
    fwd, bwd = fcr.tvl1_payloads(orc, synth, "p1_64x48")
    u, v = orc.tvl1_multiscale(A, B, nscales=3)[:2]
    assert np.array_equal(fwd, np.stack([u, v], axis=-1).astype(np.float32))
    u, v = orc.tvl1_multiscale(B, A, nscales=3)[:2]
    assert np.array_equal(bwd, np.stack([u, v], axis=-1).astype(np.float32))


def test_restatement_by_hand(orc):
    """a few pixels worked out without the vectorised code: scalar Python floats, the same association"""
    rng = np.random.default_rng(7)
    F = (rng.normal(0.0, 1.2, (6, 7, 2))).astype(np.float32)
    B = (-F + rng.normal(0.0, 0.5, (6, 7, 2)).astype(np.float32)).astype(np.float32)
    got, _ = fcr.one_map(orc, F, B, 0.01, 0.5)
    B64 = np.ascontiguousarray(B.astype(np.float64))
    for i in range(6):
        for j in range(7):
            u, v = float(F[i, j, 0]), float(F[i, j, 1])
            xt, yt = j + u, i + v
            if not (0 <= xt <= 6 and 0 <= yt <= 5):
                want = 255
            else:
                bu = orc.bicubic_at_color(B64, xt, yt, 0)
                bv = orc.bicubic_at_color(B64, xt, yt, 1)
                du, dv = u + bu, v + bv
                want = 0 if du * du + dv * dv <= 0.01 * ((u * u + v * v) + (bu * bu + bv * bv)) + 0.5 else 255
            assert got[i, j] == want, (i, j)


def test_special_values(orc):
    """NaN and Inf components and vectors that leave the image give 255; a vector landing exactly on the last column / row is
    sampled; zero against zero passes everywhere"""
    z = np.zeros((4, 5, 2), dtype=np.float32)
    assert not fcr.one_map(orc, z, z)[0].any()
    F = z.copy()
    F[0, 0, 0] = np.nan
    F[1, 1, 1] = np.inf
    F[2, 2, 0] = -np.inf
    F[3, 0, 0] = -0.5          # leaves on the left
    F[0, 4, 0] = 0.25          # ... on the right
    F[0, 2, 1] = -0.25         # ... at the top
    F[3, 3, 1] = 0.125         # ... at the bottom
    F[1, 3, 0] = 1.0           # lands on column nx - 1: sampled, and fails only by its length: 1 > 0.01 * 1 + 0.5
    got = fcr.one_map(orc, F, z)[0]
    want = np.zeros((4, 5), dtype=np.uint8)
    for r, c in ((0, 0), (1, 1), (2, 2), (3, 0), (0, 4), (0, 2), (3, 3), (1, 3)):
        want[r, c] = 255
    assert np.array_equal(got, want)
    assert fcr.one_map(orc, F, z, 0.0, 1.0)[0][1, 3] == 0          # 1 <= 1: the comparison is <=
