"""TV-L1 with occlusions over device-resident frame sequences: ofx_tvl1occ_sequence_group_dev and ofx_tvl1occ_sequence_dev.

Frames are slices of one (F, ny, nx) device tensor, payloads and maps slices of one tensor each, prefilled with a sentinel.
Every triple must be what the lone host entry (ofx_tvl1occ_multiscale with filtI0 = I0) computes on its three frames, bit for
bit: payload = float32 of (u1, u2), map = uint8(255 chi), equal outer-iteration tables and stopping values.  Selected triples
are also compared with the CPU oracle, and with the oracle's iteration tables as recorded below (iters[scale][warp], finest
scale first).  The frames are integers (synth.sequence floors), hence exact in float32 as well."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLO_SENTINEL = -7.0
OCC_SENTINEL = 7

# 1. odd n = 3015, partial blocks, map slices at every alignment
SEQ1 = dict(nx=67, ny=45, order=(0, 1, 2, 3, 3), kw=dict(nscales=2, warps=2, epsilon=0.01),
            tables=[(2, 1, 3, 1), (2, 1, 3, 1), (1, 1, 1, 1)])
# 2. triples that stop at different iterations in one group, two of them static
SEQ2 = dict(nx=96, ny=72, order=(0, 1, 2, 2, 2, 3, 1), kw=dict(nscales=3, warps=2, epsilon=0.002),
            tables=[(2, 1, 4, 2, 4, 1), (1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 1, 1), (2, 1, 3, 2, 3, 2), (7, 4, 4, 3, 6, 2)])


def _frames(synth, case):
    s = synth.sequence(case["nx"], case["ny"], 4, 1)
    return [s[k] for k in case["order"]]


def _device(frames, dtype=np.float64):
    """(frames tensor, payload tensor, map tensor) on the device, results prefilled with the sentinels"""
    import torch
    ny, nx = frames[0].shape
    T = max(len(frames) - 2, 1)
    dF = torch.from_numpy(np.stack(frames).astype(dtype)).cuda()
    flo = torch.full((T, ny, nx, 2), FLO_SENTINEL, dtype=torch.float32, device="cuda")
    occ = torch.full((T, ny * nx), OCC_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return dF, flo, occ


def _ptrs(t, n=None):
    return [t[k].data_ptr() for k in range(t.shape[0] if n is None else n)]


def _untouched(flo, occ):
    import torch
    torch.cuda.synchronize()
    return bool((flo == FLO_SENTINEL).all().item()) and bool((occ == OCC_SENTINEL).all().item())


def _table(st, kw):
    return tuple(st.iters[s][w] for s in range(kw["nscales"]) for w in range(kw["warps"]))


_LONE = {}


def _lone(gpu64, tag, t, frames, kw):
    """the lone host entry on triple t -> (payload, map, table, errors, Stats fields); solved once per module"""
    key = (tag, t)
    if key not in _LONE:
        u, v, c = gpu64.tvl1occ_multiscale(frames[t], frames[t + 1], frames[t + 2], **kw)
        st = gpu64.stats()
        err = tuple(st.error[s][w] for s in range(kw["nscales"]) for w in range(kw["warps"]))
        _LONE[key] = (np.stack([u, v], axis=-1).astype(np.float32), (255 * c).astype(np.uint8), _table(st, kw), err,
                      (st.nscales, st.nsolves, tuple(st.nx), tuple(st.ny), st.work_pix_iters))
    return _LONE[key]


def _group(gpu, frames, kw, dtype=np.float64):
    dF, flo, occ = _device(frames, dtype)
    ny, nx = frames[0].shape
    st = gpu.tvl1occ_sequence_group_dev(_ptrs(dF), _ptrs(flo), _ptrs(occ), nx, ny, **kw)
    gpu.synchronize()
    return st, flo.cpu().numpy(), occ.cpu().numpy().reshape(-1, ny, nx)


def _check_against_lone(gpu64, tag, case, frames, st, flo, occ):
    kw = case["kw"]
    tables = []
    for t in range(len(frames) - 2):
        pay, chi, table, err, _ = _lone(gpu64, tag, t, frames, kw)
        assert np.array_equal(flo[t], pay), t
        assert np.array_equal(occ[t], chi), t
        assert _table(st[t], kw) == table, (t, _table(st[t], kw), table)
        assert tuple(st[t].error[s][w] for s in range(kw["nscales"]) for w in range(kw["warps"])) == err, t
        tables.append(table)
    assert tables == case["tables"], tables          # the oracle's, recorded
    return tables


def _check_against_oracle(orc, frames, kw, t, flo, occ):
    uo, vo, co, it = orc.tvl1occ_multiscale(frames[t], frames[t + 1], frames[t + 2], **kw)
    assert np.array_equal(flo[t], np.stack([uo, vo], axis=-1).astype(np.float32)), t
    assert np.array_equal(occ[t], (255 * co).astype(np.uint8)), t
    assert 0 < occ[t].mean() < 255                   # both map values occur


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_odd_size_and_unaligned_slices(gpu64, gpu32, synth, orc, prec):
    frames = _frames(synth, SEQ1)
    gpu, dtype = (gpu64, np.float64) if prec == "f64" else (gpu32, np.float32)
    st, flo, occ = _group(gpu, frames, SEQ1["kw"], dtype)
    _check_against_lone(gpu64, "seq1", SEQ1, frames, st, flo, occ)
    _check_against_oracle(orc, frames, SEQ1["kw"], 0, flo, occ)


def test_triples_that_stop_at_different_iterations(gpu64, synth, orc):
    frames = _frames(synth, SEQ2)
    st, flo, occ = _group(gpu64, frames, SEQ2["kw"])
    tables = _check_against_lone(gpu64, "seq2", SEQ2, frames, st, flo, occ)
    assert len(set(tables)) > 1
    for t in (0, 4):
        _check_against_oracle(orc, frames, SEQ2["kw"], t, flo, occ)
    for t in (1, 2):                                 # the static triples
        assert not flo[t].any() and not occ[t].any()


def test_group_boundaries(ofx_mod, gpu64, synth):
    frames = _frames(synth, SEQ2)
    kw = SEQ2["kw"]
    _, want_flo, want_occ = _group(gpu64, frames, kw)
    ny, nx = frames[0].shape
    ctxs = [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(3)]

    def run(cs, lockstep, n_frames=len(frames)):
        dF, flo, occ = _device(frames[:n_frames])
        cs[0].set_option("lockstep", lockstep)
        try:
            work = ofx_mod.tvl1occ_sequence_dev(cs, _ptrs(dF), _ptrs(flo), _ptrs(occ), nx, ny, **kw)
        finally:
            cs[0].set_option("lockstep", 0)
        return work, flo.cpu().numpy(), occ.cpu().numpy().reshape(-1, ny, nx)

    for cs, lockstep in ((ctxs[:1], 2), (ctxs, 2), (ctxs[:1], 16), (ctxs, 0)):      # groups of 2, 2, 1 | the same on three | of 5 | 2, 2, 1
        work, flo, occ = run(cs, lockstep)
        assert np.array_equal(flo, want_flo) and np.array_equal(occ, want_occ), (len(cs), lockstep)
        assert len(work) == 5
    work, flo, occ = run(ctxs[:1], 0, 3)             # a single triple
    assert len(work) == 1 and np.array_equal(flo[0], want_flo[0]) and np.array_equal(occ[0], want_occ[0])


def test_stats_records(ofx_mod, gpu64, synth):
    frames = _frames(synth, SEQ2)
    kw = SEQ2["kw"]
    ny, nx = frames[0].shape
    dF, flo, occ = _device(frames)
    st = gpu64.tvl1occ_sequence_group_dev(_ptrs(dF), _ptrs(flo), _ptrs(occ), nx, ny, **kw)
    gpu64.synchronize()
    work = ofx_mod.tvl1occ_sequence_dev([gpu64], _ptrs(dF), _ptrs(flo), _ptrs(occ), nx, ny, **kw)
    for t in range(5):
        nscales, nsolves, lx, ly, w = _lone(gpu64, "seq2", t, frames, kw)[4]
        assert (st[t].nscales, st[t].nsolves, tuple(st[t].nx), tuple(st[t].ny)) == (nscales, nsolves, lx, ly)
        assert st[t].work_pix_iters == w == work[t]
        assert st[t].total_ms > 0


def test_errors_leave_the_outputs_untouched(ofx_mod, gpu64, gpu32, synth):
    """every case of the header's error list that one device can produce (contexts on different devices need two)"""
    frames = _frames(synth, SEQ2)
    ny, nx = frames[0].shape
    dF, flo, occ = _device(frames)
    F, P, O = _ptrs(dF), _ptrs(flo), _ptrs(occ)
    kw = SEQ2["kw"]

    def both(status, f, p, o, x=nx, y=ny, **over):
        args = dict(kw, **over)
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.tvl1occ_sequence_group_dev(f, p, o, x, y, **args)
        assert e.value.status in status, (over, e.value.status)
        with pytest.raises(ofx_mod.OfxError) as e:
            ofx_mod.tvl1occ_sequence_dev([gpu64], f, p, o, x, y, **args)
        assert e.value.status in status, (over, e.value.status)

    for over in (dict(nscales=0), dict(warps=0), dict(warps=65), dict(zfactor=1.0), dict(zfactor=0.0), dict(theta=0.0), dict(lam=0.0)):
        both((1,), F, P, O, **over)                          # occ_check's arguments
    both((1,), F, P, O, x=1, y=ny)                           # bad size
    both((1, 2), F, P, O, nscales=9)                         # a pyramid that cannot be built / coarsest level
    both((2,), F, P, O, nscales=6)                           # 6 x 5 is too small for the zoom Gaussian
    both((1,), F[:2], P[:1], O[:1])                          # n_frames < 3
    for k in (0, 3, 6):                                      # a NULL pointer at index k
        both((1,), F[:k] + [None] + F[k + 1:], P, O)
    for k in (0, 4):
        both((1,), F, P[:k] + [None] + P[k + 1:], O)
        both((1,), F, P, O[:k] + [None] + O[k + 1:])
    with pytest.raises(ofx_mod.OfxError) as e:               # n_frames > 18, the group entry only
        gpu64.tvl1occ_sequence_group_dev(F[:1] * 19, P[:1] * 17, O[:1] * 17, nx, ny, **kw)
    assert e.value.status == 1
    L = ofx_mod.lib()                                        # a NULL array
    arr = lambda xs: (C.c_void_p * len(xs))(*xs)
    tail = (nx, ny, 0.15, 0.01, 0.15, 0.3, 3, 0.5, 2, 0.002, None)
    for f, p, o in ((None, arr(P), arr(O)), (arr(F), None, arr(O)), (arr(F), arr(P), None)):
        assert L.ofx_tvl1occ_sequence_group_dev(gpu64.h, 7, f, p, o, *tail) == 1
        assert L.ofx_tvl1occ_sequence_dev(arr([gpu64.h.value]), 1, 7, f, p, o, *tail) == 1
    assert L.ofx_tvl1occ_sequence_dev(None, 1, 7, arr(F), arr(P), arr(O), *tail) == 1
    with pytest.raises(ofx_mod.OfxError) as e:               # contexts of different precision
        ofx_mod.tvl1occ_sequence_dev([gpu64, gpu32], F, P, O, nx, ny, **kw)
    assert e.value.status == 1
    gpu64.set_option("mem_budget", 1)
    try:
        with pytest.raises(ofx_mod.OfxError) as e:
            ofx_mod.tvl1occ_sequence_dev([gpu64], F, P, O, nx, ny, **kw)
        assert e.value.status == 3
    finally:
        gpu64.set_option("mem_budget", 0)
    assert _untouched(flo, occ)
