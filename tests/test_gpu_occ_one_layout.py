"""TV-L1 with occlusions: the host entries on the one group layout (a table of triples over the group's distinct planes).

A host plane is an ADDRESS: triples that pass the same array share one plane of the group -- uploaded once, one pyramid, one pair
of gradients -- and must get what they get from arrays of their own.  Host planes are dense doubles whatever the context's
"input" and "input_pitch" options say (those describe device-resident frames).  A pyramid level too small for its Gaussian is
refused before any work."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY = 64, 48
KW = dict(nscales=2, warps=1)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def frames(synth):
    return [np.ascontiguousarray(f, dtype=np.float64) for f in synth.sequence(NX, NY, 6, 1)]


@pytest.fixture(scope="module")
def alone(gpu64, frames):
    """the four consecutive triples of the six frames, each solved alone through the lone host entry"""
    return [gpu64.tvl1occ_multiscale(frames[t], frames[t + 1], frames[t + 2], **KW) for t in range(4)]


@pytest.mark.parametrize("n_ctx", [1, 3])
def test_host_batch_over_shared_planes(ofx_mod, frames, alone, n_ctx):
    """one context: one group of four triples over six planes; three: groups of 2 and 2 over four planes each"""
    ctxs = [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(n_ctx)]
    try:
        shared = [(frames[t], frames[t + 1], frames[t + 2]) for t in range(4)]
        assert shared[0][1] is shared[1][0] and shared[0][2] is shared[2][0]        # the same arrays: the same addresses
        got = ofx_mod.tvl1occ_batch(ctxs, shared, **KW)
        fresh = [tuple(f.copy() for f in t) + (t[1].copy(),) for t in shared]       # every role an array of its own, filtI0 too
        assert len({f.ctypes.data for t in fresh for f in t}) == 16
        apart = ofx_mod.tvl1occ_batch(ctxs, fresh, **KW)
    finally:
        for c in ctxs:
            c.close()
    for t in range(4):
        for a, b, c in zip(got[t], alone[t], apart[t]):
            assert np.array_equal(a, b) and np.array_equal(a, c), t
    assert got[0][0].any() and got[0][2].any()
    assert not np.array_equal(got[0][0], got[1][0])


@pytest.mark.parametrize("option", ["input_pitch", "input_pitch_below_a_row", "input"])
def test_host_planes_ignore_the_input_options(ofx_mod, orc, frames, alone, option):
    """a pitch the device entries would read rows by, one they would refuse (7 bytes: less than a row, no multiple of an element),
    a byte kind: the host entry reads dense doubles"""
    ctx = ofx_mod.Ofx(0, ofx_mod.F64)
    try:
        if option == "input":
            ctx.set_option("input", ofx_mod.IN_U8)
        else:
            ctx.set_option("input_pitch", 8 * NX + 64 if option == "input_pitch" else 7)
        u, v, c = ctx.tvl1occ_multiscale(frames[0], frames[1], frames[2], **KW)
        bu, bv, bc = ofx_mod.tvl1occ_batch([ctx], [(frames[0], frames[1], frames[2])], **KW)[0]
    finally:
        ctx.close()
    uo, vo, co, _ = orc.tvl1occ_multiscale(frames[0], frames[1], frames[2], **KW)
    assert np.array_equal(u, uo) and np.array_equal(v, vo) and np.array_equal(c, co)
    assert np.array_equal(bu, uo) and np.array_equal(bv, vo) and np.array_equal(bc, co)
    assert np.array_equal(u, alone[0][0])


def test_a_level_too_small_for_its_gaussian_is_refused_before_any_work(ofx_mod, gpu64, orc, frames):
    """the zoom to level s smooths level s - 1 with sigma = 0.6 sqrt(1 / z^2 - 1), radius int(5 sigma) + 1 (ofx_gauss_taps), and a
    level must be larger than the radius both ways"""
    radius = int(5 * 0.6 * math.sqrt(1 / 0.25 - 1)) + 1
    nx, ny, nscales = NX, NY, 1
    while min(nx, ny) > radius:                          # down to the first level the zoom Gaussian does not fit ...
        nx, ny = ofx_mod.zoom_size(nx, ny, 0.5)
        nscales += 1
    nscales += 1                                         # ... and one more level below it
    cx, cy = ofx_mod.zoom_size(nx, ny, 0.5)
    assert (nx, ny, nscales) == (8, 6, 5) and min(cx, cy) >= 2     # a level of its own right: the refusal is the Gaussian's
    kw = dict(nscales=nscales, warps=1)
    with pytest.raises(ValueError):                      # the CPU restatement of the reference refuses it too
        orc.tvl1occ_multiscale(frames[0], frames[1], frames[2], **kw)
    out = tuple(np.full((NY, NX), SENTINEL) for _ in range(3))
    with pytest.raises(ofx_mod.OfxError) as e:
        gpu64.tvl1occ_multiscale(frames[0], frames[1], frames[2], out=out, **kw)
    assert e.value.status == 2                           # OFX_ERR_SIGMA
    outs = [tuple(np.full((NY, NX), SENTINEL) for _ in range(3)) for _ in range(2)]
    with pytest.raises(ofx_mod.OfxError) as e:
        ofx_mod.tvl1occ_batch([gpu64], [(frames[0], frames[1], frames[2]), (frames[1], frames[2], frames[3])], out=outs, **kw)
    assert e.value.status == 2
    for plane in out + outs[0] + outs[1]:
        assert (plane == SENTINEL).all()
    u, v, c = gpu64.tvl1occ_multiscale(frames[0], frames[1], frames[2], nscales=nscales - 1, warps=1)   # one level fewer is served
    assert np.isfinite(u).all() and np.isfinite(v).all() and set(np.unique(c)) <= {0.0, 1.0}
