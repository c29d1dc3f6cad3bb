"""ofx_flow_pyramid_dev: the pyramid of a TV-L1 start flow, bit for bit the oracle's chain (tests/tvl1_warm_ref.py:
W_0 = the payload in double with non-finite components as 0, W_s = zoom_out(W_{s-1}) * zfactor per component), in a context of
either precision, with no byte written outside the result."""
import numpy as np
import pytest

import tvl1_warm_ref as W

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -12345.0          # doubles before and after every result
# the three shapes of the warm-start tests, the conversion alone, a radius beyond the fused Gaussian's (zoom sigma 1.9: 9 taps a
# side) and the smallest pyramid the 2:1 kernel takes
SHAPES = W.SHAPES + [(67, 45, 1, 0.5), (131, 77, 2, 0.3), (13, 9, 2, 0.5)]
IDS = ["%dx%d_%d_%g" % s for s in SHAPES]


def _flows(nx, ny):
    """five payloads: smooth, step edge, NaN / Inf entries, smooth, negative zeros (everywhere in v, a block in u)"""
    z = W.smooth_flow(nx, ny, 3).copy()
    z[..., 1] = -0.0
    z[: ny // 2, : nx // 2, 0] = -0.0
    return [W.smooth_flow(nx, ny), W.edge_flow(nx, ny), W.broken_flow(nx, ny), W.smooth_flow(nx, ny, 2), z]


@pytest.fixture(scope="module")
def want(_orc_session):
    """the oracle chain of every shape's five flows, computed once: {shape: [(u, v), ..]}"""
    _orc_session.set_num_threads(1)
    return {s: [W.start_pyramid(_orc_session, P, s[2], s[3]) for P in _flows(s[0], s[1])] for s in SHAPES}


def _run(ofx_mod, ctx, payloads, nx, ny, nscales, zfactor):
    """-> (results [(u, v)], guards (n, 2, GUARD)) of the hook on device copies of the payloads"""
    import torch
    sizes = [(nx, ny)]
    for _ in range(1, nscales):
        sizes.append(ofx_mod.zoom_size(sizes[-1][0], sizes[-1][1], zfactor))
    w, h = sizes[-1]
    d = [torch.from_numpy(np.ascontiguousarray(P)).cuda() for P in payloads]
    out = torch.full((len(payloads), 2 * GUARD + 2 * w * h), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.flow_pyramid_dev([t.data_ptr() for t in d], [out[g].data_ptr() + 8 * GUARD for g in range(len(d))], nx, ny, nscales, zfactor)
    ctx.synchronize()
    host = out.cpu().numpy()
    res = [host[g, GUARD:GUARD + 2 * w * h].reshape(h, w, 2) for g in range(len(d))]
    guards = np.stack([np.stack([host[g, :GUARD], host[g, GUARD + 2 * w * h:]]) for g in range(len(d))])
    return [(r[..., 0], r[..., 1]) for r in res], guards


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("pick", [[2], [0, 1, 2, 3, 4]], ids=["1flow", "5flows"])
def test_the_hook_is_the_oracle_chain_bit_for_bit(ofx_mod, gpu64, gpu32, want, prec, shape, pick):
    nx, ny, nscales, zfactor = shape
    ctx = gpu64 if prec == "f64" else gpu32
    flows = _flows(nx, ny)
    got, guards = _run(ofx_mod, ctx, [flows[k] for k in pick], nx, ny, nscales, zfactor)
    assert (guards == SENTINEL).all(), "bytes outside d_uv were written"
    for (u, v), k in zip(got, pick):
        wu, wv = want[shape][k]
        assert np.isfinite(u).all() and np.isfinite(v).all()
        assert _same_bits(u, wu), ("u of flow %d" % k, float(np.abs(u - wu).max()))
        assert _same_bits(v, wv), ("v of flow %d" % k, float(np.abs(v - wv).max()))


def test_refusals_write_nothing(gpu64, ofx_mod):
    import torch
    nx, ny = 67, 45
    P = torch.from_numpy(W.smooth_flow(nx, ny)).cuda()
    out = torch.full((2 * GUARD + 2 * nx * ny,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    cases = [dict(d_flo=[P.data_ptr() + 4], d_uv=[out.data_ptr()], nscales=2),            # payload off its 8 bytes
             dict(d_flo=[P.data_ptr()], d_uv=[out.data_ptr() + 8], nscales=2),            # result off its 16 bytes
             dict(d_flo=[P.data_ptr()] * 17, d_uv=[out.data_ptr()] * 17, nscales=2),      # more than a group
             dict(d_flo=[P.data_ptr()], d_uv=[out.data_ptr()], nscales=6)]                # a level too small for the Gaussian
    for k, c in enumerate(cases):
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.flow_pyramid_dev(c["d_flo"], c["d_uv"], nx, ny, c["nscales"], 0.5)
        assert e.value.status == (2 if k == 3 else 1), k
    gpu64.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
