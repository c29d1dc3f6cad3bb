"""The restatement of ofx_flow_warp_dev / ofx_flow_interpolate_dev (tests/flow_apply_ref.py) and the inputs the GPU tests share,
pinned on the CPU so that equality on the GPU cannot hold vacuously: every branch is taken, byte results are clamped at both
ends, no unclamped value sits on a rounding boundary, some blocks fit the LDS tile and some do not -- and the definition does
what it is for: the in-between frame is far closer to the true one than the plain average."""
import numpy as np
import pytest

import flow_apply_ref as far

# the GPU tests' times.  Sevenths and ninths: s A + t B of two integers (the branch where neither sample is inside, and every sample at
# an integer position) is a multiple of 1/7 or 1/9 up to rounding and so never k + 0.5, which tenths and the half can hit exactly
T = (3.0 / 7.0, 5.0 / 7.0, 2.0 / 9.0)
PINNED = ("p1_64x48", "p1_37x29", "130x70", far.JUMP)
INT_KINDS = (("u8", 255.0), ("u16", 65535.0))


def _shares(ina, inb):
    n = float(ina.size)
    return ((ina & inb).sum() / n, (ina & ~inb).sum() / n, (~ina & inb).sum() / n, int((~ina & ~inb).sum()))


def _margin(o, top):
    """smallest distance of an unclamped value to a rounding boundary k + 0.5"""
    m = (o > 0) & (o < top)
    return float(np.abs((o[m] - np.floor(o[m])) - 0.5).min())


@pytest.mark.parametrize("name,want", [("seq_64x48", (0.918, 0.040, 0.042, 3)), ("seq_131x77", (0.950, 0.025, 0.025, 3))])
def test_halfway_frame_takes_every_branch_and_beats_the_average(orc, synth, name, want):
    """frames 0 and 2 of synth.sequence against the true frame 1, the oracle's TV-L1 both ways: the branch counts of the issue, and
    an RMSE below half of the plain average's (measured ratios 0.23 and 0.20; one half leaves a factor of two for a restatement that
    differs in rounding only)"""
    A, M, B = far.seq_frames(synth, name)
    fwd, bwd = far.payloads(orc, synth, name)
    ina, inb, o = far.interp_parts(orc, A, B, fwd, bwd, 0.5)
    both, only_a, only_b, neither = _shares(ina, inb)
    print("%s: both %.4f, only A %.4f, only B %.4f, neither %d pixels" % (name, both, only_a, only_b, neither))
    assert abs(both - want[0]) < 5e-4 and abs(only_a - want[1]) < 5e-4 and abs(only_b - want[2]) < 5e-4 and neither == want[3]
    assert only_a >= 0.01 and only_b >= 0.01 and neither >= 1 and both > 0
    rmse = float(np.sqrt(np.mean((o - M) ** 2)))
    plain = float(np.sqrt(np.mean((0.5 * A + 0.5 * B - M) ** 2)))
    print("%s: RMSE against the true frame %.3f, of the plain average %.3f, ratio %.3f" % (name, rmse, plain, rmse / plain))
    assert rmse < 0.5 * plain


@pytest.mark.parametrize("name", PINNED + tuple(far.SEQ_CASES))
def test_in_between_cases_take_every_branch(orc, synth, name):
    nz = 1 if name in far.SEQ_CASES else 3
    fwd, bwd = far.payloads(orc, synth, name)
    for kind, top in INT_KINDS:
        A, B = far.frames(synth, name, nz, kind)
        for t in T:
            ina, inb, o = far.interp_parts(orc, A, B, fwd, bwd, t)
            both, only_a, only_b, neither = _shares(ina, inb)
            assert both > 0 and neither >= 1 and only_a >= 0.01 and only_b >= 0.01, (name, t, both, only_a, only_b, neither)
            assert (o <= 0).any() and (o >= top).any(), (name, kind, t, "clamped at 0 / at max")
            assert _margin(o, top) > 1e-9, (name, kind, t)


@pytest.mark.parametrize("name", PINNED)
def test_warp_cases_hold_every_class(orc, synth, name):
    fwd = far.payloads(orc, synth, name)[0]
    occ = far.occ_maps(orc, synth, name)[0]
    for kind, top in INT_KINDS:
        A, B = far.frames(synth, name, 3, kind)
        keep, left, smp = far.warp_parts(orc, B, fwd, occ)
        flagged = ~left & (occ != 0)
        print("%s %s: kept %.3f, left the frame %.3f, flagged %.3f" % (name, kind, keep.mean(), left.mean(), flagged.mean()))
        assert keep.mean() >= 0.02 and left.mean() >= 0.02 and flagged.mean() >= 0.02
        assert (smp[keep] <= 0).any() and (smp[keep] >= top).any(), (name, kind, "clamped at 0 / at max")
        assert _margin(smp[keep], top) > 1e-9, (name, kind)
        got = far.warp(orc, B, fwd, occ, A)
        assert np.array_equal(got[~keep], A[~keep])                     # the fill frame, unchanged


def test_every_shape_of_the_gpu_tests_stays_off_the_rounding_boundaries(orc, synth):
    for name in far.SIZES:
        nz = 1 if name in far.SEQ_CASES else 3
        fwd, bwd = far.payloads(orc, synth, name)
        occ = far.occ_maps(orc, synth, name)[0]
        for kind, top in INT_KINDS:
            A, B = far.frames(synth, name, nz, kind)
            keep, _, smp = far.warp_parts(orc, B, fwd, occ)
            assert not keep.any() or _margin(smp[keep], top) > 1e-9, (name, kind)
            for t in T:
                assert _margin(far.interp_parts(orc, A, B, fwd, bwd, t)[2], top) > 1e-9, (name, kind, t)


def test_the_jump_case_misses_the_tile_in_some_blocks_and_fits_it_in_others(orc, synth):
    nx, ny = far.SIZES[far.JUMP]
    fwd, bwd = far.payloads(orc, synth, far.JUMP)
    A, B = far.frames(synth, far.JUMP, 1, "f64")
    u, v = fwd[..., 0].astype(np.float64), fwd[..., 1].astype(np.float64)
    keep = far.warp_parts(orc, B, fwd, None)[0]                     # without the map, which flags the jump
    fit, miss = far.tile_use(u, v, keep, nx, ny)
    print("warp without a map: %d blocks fit the tile, %d miss it" % (fit, miss))
    assert fit >= 4 and miss >= 1
    u10, v10 = bwd[..., 0].astype(np.float64), bwd[..., 1].astype(np.float64)
    missed = {"A": 0, "B": 0}
    for t in T:
        s = 1.0 - t
        c0, c1, c2 = s * t, t * t, s * s
        ina, inb, _ = far.interp_parts(orc, A, B, fwd, bwd, t)
        fa = far.tile_use(c1 * u10 - c0 * u, c1 * v10 - c0 * v, ina, nx, ny)
        fb = far.tile_use(c2 * u - c0 * u10, c2 * v - c0 * v10, inb, nx, ny)
        print("t = %.2f: A %d fit, %d miss; B %d fit, %d miss" % (t, fa[0], fa[1], fb[0], fb[1]))
        assert fa[0] >= 4 and fb[0] >= 4
        missed["A"] += fa[1]
        missed["B"] += fb[1]
    assert missed["A"] >= 1 and missed["B"] >= 1
    # ... while the TV-L1 case never leaves the tile
    f2 = far.payloads(orc, synth, "p1_64x48")[0]
    k2 = far.warp_parts(orc, far.frames(synth, "p1_64x48", 1, "f64")[1], f2, None)[0]
    assert far.tile_use(f2[..., 0].astype(np.float64), f2[..., 1].astype(np.float64), k2, 64, 48)[1] == 0


@pytest.mark.parametrize("kind", tuple(far.KINDS))
def test_identities(orc, synth, kind):
    """t = 0 gives A, t = 1 gives B, a zero payload gives Src, an integer translation the shifted frame: exactly"""
    name, nz = "p1_37x29", 3
    A, B = far.frames(synth, name, nz, kind)
    fwd, bwd = far.payloads(orc, synth, name)
    ny, nx, _ = A.shape
    assert np.array_equal(far.interpolate(orc, A, B, fwd, bwd, 0.0), A)
    assert np.array_equal(far.interpolate(orc, A, B, fwd, bwd, 1.0), B)
    zero = np.zeros_like(fwd)
    assert np.array_equal(far.warp(orc, B, zero), B)
    shift = zero.copy()
    shift[..., 0], shift[..., 1] = 3.0, -2.0
    want = np.zeros_like(B)
    want[2:, :nx - 3] = B[:ny - 2, 3:]
    assert np.array_equal(far.warp(orc, B, shift), want)
    want = np.array(A)
    want[2:, :nx - 3] = B[:ny - 2, 3:]
    assert np.array_equal(far.warp(orc, B, shift, None, A), want)


def test_conv_rounds_clamps_and_drops_nan():
    x = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 0.49, 0.5, 1.49999, 254.4999, 254.5, 255.0, 300.0, np.inf, 65534.5, 65535.0, 7e4])
    assert far.conv(x, np.uint8).tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 254, 255, 255, 255, 255, 255, 255, 255]
    assert far.conv(x, np.uint16).tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 254, 255, 255, 300, 65535, 65535, 65535, 65535]
    assert far.conv(x, np.float64) is x
    assert far.conv(np.array([0.1, 1e300]), np.float32).tolist() == [float(np.float32(0.1)), np.inf]


def test_positions_that_fail_inside_never_reach_the_sampler(orc, synth):
    """NaN, Inf and vectors beyond an int in a payload: the restatement answers with the fill frame or the plain blend"""
    A, B = far.frames(synth, "3x5", 1, "f64")
    F = np.zeros((5, 3, 2), dtype=np.float32)
    F[0, 0], F[1, 1], F[2, 2], F[3, 0] = (np.nan, 0), (0, np.inf), (-np.inf, np.nan), (3e9, -3e9)
    keep, left, _ = far.warp_parts(orc, B, F)
    assert [bool(left[r, c]) for r, c in ((0, 0), (1, 1), (2, 2), (3, 0))] == [True] * 4 and keep.sum() == 11
    got = far.warp(orc, B, F, None, A)
    assert np.array_equal(got[left], A[left]) and np.array_equal(got[keep], B[keep])
    mid = far.interpolate(orc, A, B, F, F, 0.5)
    assert np.array_equal(mid[left], 0.5 * A[left] + 0.5 * B[left])
