"""Temporal Brox on device-resident sequences under the tolerance mode (option sor_exact = 0): the device and batch entries share
the host entry's level solver, so under equal options payload f == float32 of (u[f], v[f]) of ofx_brox_temporal, bit for bit, with
equal sweep tables."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
NX, NY, FRAMES = 64, 48, 4
KW = dict(nscales=2, inner=2, outer=3, TOL=1e-4)


def _payloads(n_flo):
    import torch
    flo = torch.full((n_flo, NY, NX, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return flo


def _clip(I, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(I, dtype=dtype)).cuda()


def _ptrs(t):
    return [t[k].data_ptr() for k in range(t.shape[0])]


def _tolerance_on(ctxs):
    for c in ctxs:
        c.set_option("sor_exact", 0)


def _defaults(ctxs):
    for c in ctxs:
        c.set_option("sor_exact", 1)
        c.set_option("sor_fuse", 0)


def _dev(gpu, clip):
    flo = _payloads(FRAMES - 1)
    gpu.brox_temporal_dev(_ptrs(clip), _ptrs(flo), NX, NY, **KW)
    gpu.synchronize()
    return flo.cpu().numpy(), gpu.stats().iterations().copy()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_device_entry_equals_host_entry(gpu64, gpu32, synth, prec):
    gpu, dtype = (gpu64, np.float64) if prec == "f64" else (gpu32, np.float32)
    I = synth.sequence(NX, NY, FRAMES, 1)                   # integers: exact in float32 too
    _tolerance_on([gpu])
    try:
        u, v = gpu.brox_temporal(I, **KW)
        it_h = gpu.stats().iterations().copy()
        got, it_d = _dev(gpu, _clip(I, dtype))
    finally:
        _defaults([gpu])
    ue, ve = gpu.brox_temporal(I, **KW)                     # the exact mode: another order, another result
    assert not np.array_equal(ue, u)
    assert not (got == SENTINEL).any()
    assert np.array_equal(it_d, it_h)
    assert np.array_equal(got, np.stack([u, v], axis=-1).astype(np.float32))


def test_batch_equals_the_device_entry(ofx_mod, gpu64, synth):
    ctxs = [gpu64, ofx_mod.Ofx(0, ofx_mod.F64)]
    clips = [_clip(synth.sequence(NX, NY, FRAMES, k), np.float64) for k in range(3)]
    _tolerance_on(ctxs)
    try:
        lone = [_dev(gpu64, c)[0] for c in clips]
        flo = _payloads(3 * (FRAMES - 1))
        work = ofx_mod.brox_temporal_batch_dev(ctxs, [p for c in clips for p in _ptrs(c)], _ptrs(flo), NX, NY, FRAMES, **KW)
    finally:
        _defaults(ctxs)
    got = flo.cpu().numpy().reshape(3, FRAMES - 1, NY, NX, 2)
    assert len({l.tobytes() for l in lone}) == 3            # three different problems
    for q in range(3):
        assert work[q] > 0
        assert np.array_equal(got[q], lone[q]), q
    exact = _dev(gpu64, clips[0])[0]                        # back in the exact mode: not the tolerance mode's payloads
    assert not np.array_equal(exact, lone[0])
