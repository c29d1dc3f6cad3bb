"""Temporal Brox on device-resident sequences: ofx_brox_temporal_dev and ofx_brox_temporal_batch_dev.

Frames live in device tensors of the context's storage type, payloads in one float32 tensor prefilled with a sentinel.  The
contract is bit for bit: payload f == float32 of (u[f], v[f]) of the host entry ofx_brox_temporal on the same values, with equal
sweep tables.  Every comparison is np.array_equal.  The frames are integers (synth.sequence floors), exact in float32 too.

Two shapes of the issue's list, 3x3 and 67x5, are not solvable by EITHER entry: the presmoothing Gaussian (sigma 0.8, radius
(int) (5 sigma) + 1 = 5) must be smaller than both image sides (op_gaussian_planes' rule: the reference throws or reads out of bounds
there), so ofx_brox_temporal returns OFX_ERR_SIGMA on them, and did before the device entries existed.  "Equal to the host entry"
is therefore asserted uniformly for every shape as: the same status, and on success the same payload and sweep table; on an
error the sentinel-filled payloads are untouched.  The smallest shapes that do solve, 6x6 (the one-sided temporal differences
of 3 frames are adjacent) and 67x6 (a width across the 64-lane tile edge, a height that is no multiple of the block's 4 rows),
are in the list beside them."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
KW = dict(inner=2, outer=3, TOL=1e-4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("alpha", "gamma", "nscales", "nu", "TOL", "inner", "outer")


def _payloads(n_flo, ny, nx):
    import torch
    flo = torch.full((n_flo, ny, nx, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return flo


def _clip(I, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(I, dtype=dtype)).cuda()


def _ptrs(t):
    return [t[k].data_ptr() for k in range(t.shape[0])]


def _untouched(flo):
    import torch
    torch.cuda.synchronize()
    return bool((flo == SENTINEL).all().item())


def _host(gpu, I, kw):
    """the host entry -> (payloads (frames - 1, ny, nx, 2) float32, sweep table, work)"""
    u, v = gpu.brox_temporal(I, **kw)
    st = gpu.stats()
    return np.stack([u, v], axis=-1).astype(np.float32), st.iterations().copy(), st.work_pix_iters


def _dev(gpu, dF, ny, nx, kw):
    """the device entry on the frame pointers dF -> (payloads, sweep table, work)"""
    flo = _payloads(len(dF) - 1, ny, nx)
    gpu.brox_temporal_dev(dF, _ptrs(flo), nx, ny, **kw)
    gpu.synchronize()
    st = gpu.stats()
    return flo.cpu().numpy(), st.iterations().copy(), st.work_pix_iters


def _same_as_host(ofx_mod, gpu, I, kw, dtype=np.float64):
    """both entries on the same values: the same status; on success the same payloads, sweep table and work"""
    frames, ny, nx = I.shape
    clip = _clip(I, dtype)
    try:
        want = _host(gpu, I, kw)
    except ofx_mod.OfxError as e:
        flo = _payloads(frames - 1, ny, nx)
        with pytest.raises(ofx_mod.OfxError) as d:
            gpu.brox_temporal_dev(_ptrs(clip), _ptrs(flo), nx, ny, **kw)
        assert d.value.status == e.status
        assert _untouched(flo)
        return None
    got = _dev(gpu, _ptrs(clip), ny, nx, kw)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert got[2] == want[2] > 0
    return got


@pytest.mark.parametrize("name", ["broxt_seq3_48x40", "broxt_seq4_64x48"])
def test_recorded_sequences(ofx_mod, gpu64, synth, name):
    c, g = json.load(open(os.path.join(GOLDEN, "cases.json")))[name], np.load(os.path.join(GOLDEN, name + ".npz"))
    kw = {k: c["params"][k] for k in KEYS if k in c["params"]}
    I = synth.sequence(c["nx"], c["ny"], c["pair"])
    got = _same_as_host(ofx_mod, gpu64, I, kw)
    assert got is not None
    assert list(got[1][::-1].ravel()) == list(g["iters"])
    # the existing fixture test's bound on the doubles, 1e-11, plus what the payload's float32 may round away: half an ulp
    for k, key in enumerate(("u", "v")):
        d = np.abs(got[0][..., k].astype(np.float64) - g[key])
        print(name, key, "max |payload - recorded| =", d.max())
        assert (d <= 1e-11 + 0.5 * np.spacing(np.abs(got[0][..., k])).astype(np.float64)).all()


@pytest.mark.parametrize("nx,ny,frames,kw,solves", [
    (3, 3, 3, dict(nscales=1), False),                      # smaller than the presmoothing Gaussian: both entries refuse
    (67, 5, 3, dict(nscales=1), False),                     # the same, by the height
    (6, 6, 3, dict(nscales=1), True),                       # the smallest problem: both one-sided temporal differences adjacent
    (67, 6, 3, dict(nscales=1), True),                      # across the 64-lane tile edge, rows no multiple of the block's
    (37, 29, 5, dict(nscales=3, nu=0.75), True),            # odd level sizes; zoom-out and zoom-in over all planes
    (16, 12, 32, dict(nscales=1, outer=2), True),           # the last slot of the pointer table
])
def test_device_entry_equals_host_entry(ofx_mod, gpu64, synth, nx, ny, frames, kw, solves):
    got = _same_as_host(ofx_mod, gpu64, synth.sequence(nx, ny, frames), dict(KW, **kw))
    assert (got is not None) == solves
    if solves:
        assert got[0].any()                                 # a flow, not zeros


def test_f32_context_with_float_frames(ofx_mod, gpu32, synth):
    I = synth.sequence(64, 48, 4, 1) + 0.3                  # not representable in float32: the host entry gets the rounded values
    I32 = I.astype(np.float32)
    assert not np.array_equal(I32.astype(np.float64), I)
    frames, ny, nx = I.shape
    kw = dict(KW, nscales=2)
    want = _host(gpu32, I32.astype(np.float64), kw)
    clip = _clip(I32, np.float32)                           # kept alive: the pointers are all the library holds
    got = _dev(gpu32, _ptrs(clip), ny, nx, kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].any()


def test_frames_in_separate_allocations_in_shuffled_order(gpu64, synth):
    I = synth.sequence(40, 32, 5)
    frames, ny, nx = I.shape
    kw = dict(KW, nscales=2)
    clip = _clip(I)
    want = _dev(gpu64, _ptrs(clip), ny, nx, kw)
    pad = [_clip(np.zeros((1, 3 + 5 * k))) for k in range(4)]         # odd-sized neighbours between the frames
    alloc = {}
    for k in (3, 0, 4, 2, 1):                                          # memory order != frame order
        alloc[k] = _clip(I[k])
        pad.append(_clip(np.zeros((1, 7 + k))))
    got = _dev(gpu64, [alloc[k].data_ptr() for k in range(frames)], ny, nx, kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_repeated_frame_pointer(gpu64, synth):
    I = synth.sequence(40, 32, 3)
    _, ny, nx = I.shape
    kw = dict(KW, nscales=2)
    order = [0, 1, 1, 2]                                               # a still frame in the middle
    want = _host(gpu64, I[order], kw)
    clip = _clip(I)
    p = _ptrs(clip)
    got = _dev(gpu64, [p[k] for k in order], ny, nx, kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- batch ----------------------------------------------------------------------------------------------------------
B_NX, B_NY, B_FRAMES, B_SEQ = 40, 32, 4, 5
B_KW = dict(KW, nscales=2)


@pytest.fixture(scope="module")
def batch_case(ofx_mod, gpu64, synth):
    """5 sequences of 4 frames at 40x32 on the device, and the device entry's result for each, computed once"""
    clips = [_clip(synth.sequence(B_NX, B_NY, B_FRAMES, k)) for k in range(B_SEQ)]
    lone = [_dev(gpu64, _ptrs(c), B_NY, B_NX, B_KW) for c in clips]
    assert len({l[0].tobytes() for l in lone}) == B_SEQ                # five different problems
    return clips, lone


def _batch(ofx_mod, ctxs, clips):
    flo = _payloads(B_SEQ * (B_FRAMES - 1), B_NY, B_NX)
    dF = [p for c in clips for p in _ptrs(c)]
    work = ofx_mod.brox_temporal_batch_dev(ctxs, dF, _ptrs(flo), B_NX, B_NY, B_FRAMES, **B_KW)
    return work, flo.cpu().numpy().reshape(B_SEQ, B_FRAMES - 1, B_NY, B_NX, 2)


def _one_sequence_bytes(ofx_mod):
    """the header's memory rule for one sequence of the batch case, f64 storage, default sor_batch"""
    nx1, ny1 = ofx_mod.zoom_size(B_NX, B_NY, B_KW.get("nu", 0.75))
    level_px = B_NX * B_NY + nx1 * ny1
    return 1.05 * 8 * (level_px * (B_FRAMES + (27 + 2 * 64) * (B_FRAMES - 1)) + 2 * B_FRAMES * B_NX * B_NY)


@pytest.mark.parametrize("n_ctx", [1, 2, 3])
def test_batch_equals_the_device_entry(ofx_mod, gpu64, batch_case, n_ctx):
    clips, lone = batch_case
    ctxs = [gpu64] + [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(n_ctx - 1)]
    work, flo = _batch(ofx_mod, ctxs, clips)
    for q in range(B_SEQ):
        assert np.array_equal(flo[q], lone[q][0]), q
        assert work[q] == lone[q][2] > 0, q


def test_batch_under_a_memory_budget(ofx_mod, gpu64, batch_case):
    clips, lone = batch_case
    ctxs = [gpu64] + [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)]
    per = _one_sequence_bytes(ofx_mod)
    gpu64.set_option("mem_budget", 1.5 * per)                          # holds one sequence: one context at a time
    try:
        work, flo = _batch(ofx_mod, ctxs, clips)
    finally:
        gpu64.set_option("mem_budget", 0)
    for q in range(B_SEQ):
        assert np.array_equal(flo[q], lone[q][0]) and work[q] == lone[q][2], q
    gpu64.set_option("mem_budget", 0.5 * per)                          # holds none
    flo = _payloads(B_SEQ * (B_FRAMES - 1), B_NY, B_NX)
    try:
        with pytest.raises(ofx_mod.OfxError) as e:
            ofx_mod.brox_temporal_batch_dev(ctxs, [p for c in clips for p in _ptrs(c)], _ptrs(flo), B_NX, B_NY, B_FRAMES, **B_KW)
    finally:
        gpu64.set_option("mem_budget", 0)
    assert e.value.status == 3
    assert _untouched(flo)


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_errors_leave_the_payloads_untouched(ofx_mod, gpu64, gpu32, synth):
    """every case of the header's error list that one device can produce (contexts on different devices need two)"""
    nx, ny, frames = 40, 32, 4
    clip = _clip(synth.sequence(nx, ny, frames))
    flo = _payloads(2 * (frames - 1), ny, nx)
    F, P = _ptrs(clip), _ptrs(flo)[:frames - 1]
    F2, P2 = F + F, _ptrs(flo)
    kw = dict(KW, nscales=2)

    def both(status, f, p, x=nx, y=ny, where=None, **over):
        """the device entry on (f, p) and the batch entry on two such sequences"""
        args = dict(kw, **over)
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.brox_temporal_dev(f, p, x, y, **args)
        assert e.value.status == status, (over, e.value.status)
        if where is not None:
            assert where in str(e.value), str(e.value)
        with pytest.raises(ofx_mod.OfxError) as e:
            ofx_mod.brox_temporal_batch_dev([gpu64], f + f, p + p, x, y, len(f), **args)
        assert e.value.status == status, (over, e.value.status)

    both(1, F[:2], P[:1])                                              # frames <= 2
    both(1, F, P, x=2, y=ny)                                           # below 3x3
    both(1, F, P, x=nx, y=2)
    both(1, F, P, inner=-1)
    both(1, F, P, outer=-1)
    both(1, F, P, nscales=0)
    both(1, F, P, nu=1.0)
    assert [ofx_mod.zoom_size(s, s, 0.8325)[0] for s in (6, 5, 4, 3)] == [5, 4, 3, 2]
    both(1, F, P, x=6, y=6, nscales=5, nu=0.8325)                      # levels 6, 5, 4, 3, 2: the coarsest has no interior
    both(2, F, P, x=5, y=ny, nscales=1)                                # the presmoothing Gaussian (radius 5) does not fit
    both(2, F, P, nscales=11)                                          # nor the zoom Gaussian (radius 3) level 9, 4 x 3
    with pytest.raises(ofx_mod.OfxError) as e:                         # more frames than the pointer table holds
        gpu64.brox_temporal_dev(F[:1] * 33, P[:1] * 32, nx, ny, **kw)
    assert e.value.status == 1
    for k in (0, 3):                                                   # a NULL / misaligned frame pointer, with its index
        both(1, F[:k] + [None] + F[k + 1:], P, where="frame %d" % k)
        both(1, F[:k] + [F[k] + 4] + F[k + 1:], P, where="frame %d" % k)
    for k in (0, 2):                                                   # ... payload pointer
        both(1, F, P[:k] + [None] + P[k + 1:], where="pointer %d" % k)
        both(1, F, P[:k] + [P[k] + 4] + P[k + 1:], where="pointer %d" % k)
    with pytest.raises(ofx_mod.OfxError) as e:                         # float frames need 4-byte alignment only ...
        gpu32.brox_temporal_dev([F[0] + 2] + F[1:], P, nx, ny, **kw)
    assert e.value.status == 1 and "frame 0" in str(e.value)
    L = ofx_mod.lib()                                                  # a NULL array
    arr = lambda xs: (C.c_void_p * len(xs))(*xs)
    tail = (nx, ny, 18.0, 7.0, 2, 0.75, 1e-4, 2, 3)
    for f, p in ((None, arr(P)), (arr(F), None)):
        assert L.ofx_brox_temporal_dev(gpu64.h, frames, f, p, *tail) == 1
    for f, p in ((None, arr(P2)), (arr(F2), None)):
        assert L.ofx_brox_temporal_batch_dev(arr([gpu64.h.value]), 1, 2, frames, f, p, *tail, None) == 1
    assert L.ofx_brox_temporal_batch_dev(None, 1, 2, frames, arr(F2), arr(P2), *tail, None) == 1
    assert L.ofx_brox_temporal_batch_dev(arr([gpu64.h.value]), 0, 2, frames, arr(F2), arr(P2), *tail, None) == 1
    assert L.ofx_brox_temporal_batch_dev(arr([gpu64.h.value, None]), 2, 2, frames, arr(F2), arr(P2), *tail, None) == 1
    assert L.ofx_brox_temporal_batch_dev(arr([gpu64.h.value]), 1, 0, frames, arr(F2), arr(P2), *tail, None) == 1      # n_seq < 1
    with pytest.raises(ofx_mod.OfxError) as e:                         # contexts of different precision
        ofx_mod.brox_temporal_batch_dev([gpu64, gpu32], F2, P2, nx, ny, frames, **kw)
    assert e.value.status == 1
    with pytest.raises(ofx_mod.OfxError) as e:                         # a bad pointer in the SECOND sequence of a batch
        ofx_mod.brox_temporal_batch_dev([gpu64], F + [None] + F[1:], P2, nx, ny, frames, **kw)
    assert e.value.status == 1 and "sequence 1" in str(e.value)
    assert _untouched(flo)
