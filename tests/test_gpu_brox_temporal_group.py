"""Temporal Brox in lockstep groups of device-resident sequences: ofx_brox_temporal_group_dev, and ofx_brox_temporal_batch_dev
under option "lockstep" >= 2.

The expected values are the lone device entry's (ofx_brox_temporal_dev) on the same context under the same options; other test
files pin that entry to the oracle and to the colour-order checker.  The contract is bit for bit: every payload np.array_equal,
every sweep table equal and, in the exact mode, every stopping value equal.  A lone solve is computed once per (context, clip,
parameters, options) and shared between the tests.

Clips are synth.sequence(nx, ny, frames, k); the STILL clip is frame 0 of k = 0 passed `frames` times (one allocation, the
same pointer in every slot), whose every solve stops after one sweep -- so a group that holds it has a member that leaves the
windows at once while the others run for 60 to 120 sweeps."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
KW = dict(alpha=18.0, gamma=7.0, nu=0.75, outer=3)
DEFAULTS = dict(sor_exact=1, sor_fuse=0, lockstep=0, mem_budget=0)
STILL = "still"

_DEV = {}       # (dtype, nx, ny, frames, k) -> (tensor kept alive, frame pointers)
_LONE = {}      # (context, clip, parameters, options) -> (payload, sweep table, stopping values, work)


@contextmanager
def _options(ctxs, **opts):
    ctxs = ctxs if isinstance(ctxs, (list, tuple)) else [ctxs]
    try:
        for c in ctxs:
            for name, val in opts.items():
                c.set_option(name, val)
        yield
    finally:
        for c in ctxs:
            for name in opts:
                c.set_option(name, DEFAULTS[name])


def _payloads(n_flo, ny, nx):
    import torch
    flo = torch.full((n_flo, ny, nx, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return flo


def _ptrs(t):
    return [t[k].data_ptr() for k in range(t.shape[0])]


def _untouched(flo):
    import torch
    torch.cuda.synchronize()
    return bool((flo == SENTINEL).all().item())


def _seq(synth, nx, ny, frames, k, dtype=np.float64):
    """frame pointers of clip k on the device (STILL: one frame, its pointer `frames` times)"""
    import torch
    key = (np.dtype(dtype).name, nx, ny, frames, k)
    if key not in _DEV:
        I = synth.sequence(nx, ny, frames, 0)[:1] if k == STILL else synth.sequence(nx, ny, frames, k)
        t = torch.from_numpy(np.ascontiguousarray(I, dtype=dtype)).cuda()
        _DEV[key] = (t, _ptrs(t) * frames if k == STILL else _ptrs(t))
    return _DEV[key][1]


def _lone(gpu, tag, synth, nx, ny, frames, k, kw, opts, dtype=np.float64):
    """ofx_brox_temporal_dev on clip k alone, under the options the caller has set (`opts` names them for the cache)"""
    key = (tag, np.dtype(dtype).name, nx, ny, frames, k, tuple(sorted(kw.items())), tuple(sorted(opts.items())))
    if key not in _LONE:
        flo = _payloads(frames - 1, ny, nx)
        gpu.brox_temporal_dev(_seq(synth, nx, ny, frames, k, dtype), _ptrs(flo), nx, ny, **kw)
        gpu.synchronize()
        st = gpu.stats()
        _LONE[key] = (flo.cpu().numpy(), st.iterations().copy(), st.errors().copy(), st.work_pix_iters)
    return _LONE[key]


def _group(gpu, synth, nx, ny, frames, ks, kw, dtype=np.float64):
    flo = _payloads(len(ks) * (frames - 1), ny, nx)
    dF = [p for k in ks for p in _seq(synth, nx, ny, frames, k, dtype)]
    st = gpu.brox_temporal_group_dev(dF, _ptrs(flo), nx, ny, frames, **kw)
    gpu.synchronize()
    return st, flo.cpu().numpy().reshape(len(ks), frames - 1, ny, nx, 2)


def _equals_alone(gpu, tag, synth, nx, ny, frames, ks, kw, opts=None, dtype=np.float64, values=True):
    """a group of the clips ks against each of them alone; returns the lone sweep tables and the group's payloads"""
    opts = opts or {}
    with _options(gpu, **opts):
        lone = [_lone(gpu, tag, synth, nx, ny, frames, k, kw, opts, dtype) for k in ks]
        st, got = _group(gpu, synth, nx, ny, frames, ks, kw, dtype)
    assert len(st) == len(ks)
    for q, (flo, iters, errs, work) in enumerate(lone):
        print("sequence", q, "clip", ks[q], "sweeps", st[q].iterations().tolist(), "alone", iters.tolist())
        assert np.array_equal(got[q], flo), q
        assert np.array_equal(st[q].iterations(), iters), q
        if values:
            assert np.array_equal(st[q].errors(), errs), (q, st[q].errors().tolist(), errs.tolist())
        assert st[q].work_pix_iters == work, q
    assert got.any() or not any(l[1].any() for l in lone)              # a flow, not zeros (unless no solve swept at all)
    return [tuple(int(x) for x in l[1].ravel()) for l in lone], got


CASES = {
    "a": dict(nx=6, ny=6, frames=3, ks=[0, 1], kw=dict(KW, nscales=1, outer=2)),
    "b": dict(nx=40, ny=32, frames=4, ks=[0, 1, 2, STILL], kw=dict(KW, nscales=2)),
    "c": dict(nx=24, ny=70, frames=3, ks=[0, 1, 2], kw=dict(KW, nscales=1, outer=2)),
    "d": dict(nx=33, ny=47, frames=3, ks=list(range(16)), kw=dict(KW, nscales=2)),
    "e": dict(nx=24, ny=20, frames=10, ks=[0, 1, 2, 3], kw=dict(KW, nscales=1)),
}


# ---- 1. exact mode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_group_equals_the_sequences_alone(gpu64, synth, case):
    c = CASES[case]
    tables, _ = _equals_alone(gpu64, "f64", synth, c["nx"], c["ny"], c["frames"], c["ks"], c["kw"])
    if case == "a":
        assert all(set(t) == {300} for t in tables), tables             # both clips run into the sweep limit
    if case in ("b", "c"):
        assert len(set(tables)) > 1, tables                             # the members stop at different sweeps
    if case == "b":
        assert set(tables[3]) == {1}, tables[3]                         # the still clip: one sweep per solve


# ---- 2. loop ends ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TOL,sweeps", [(2000.0, 0), (0.0, 300)])
def test_loop_ends_in_a_group(gpu64, synth, TOL, sweeps):
    c = CASES["b"]
    tables, _ = _equals_alone(gpu64, "f64", synth, c["nx"], c["ny"], c["frames"], c["ks"], dict(c["kw"], TOL=TOL))
    assert all(set(t) == {sweeps} for t in tables[:3]), tables
    # the still clip's first sweep changes nothing: its stopping value is exactly 0, and `0 > TOL` ends the loop even for TOL = 0,
    # in the reference as here -- one member at the sweep limit's other end
    assert set(tables[3]) == {min(sweeps, 1)}, tables[3]


def test_sor_exact_2_in_a_group(gpu64, synth):
    c = CASES["a"]
    _equals_alone(gpu64, "f64", synth, c["nx"], c["ny"], c["frames"], c["ks"], c["kw"], opts=dict(sor_exact=2))


# ---- 3. tolerance mode -----------------------------------------------------------------------------------------------------
def test_tolerance_group_for_every_sor_fuse(gpu64, synth):
    c = CASES["b"]
    first = None
    for fuse in (0, 1, 2, 4, 9):
        tables, got = _equals_alone(gpu64, "f64", synth, c["nx"], c["ny"], c["frames"], c["ks"], c["kw"],
                                    opts=dict(sor_exact=0, sor_fuse=fuse), values=False)
        assert len(set(tables)) > 1, tables
        if first is None:
            first = got
        assert np.array_equal(got, first), fuse                         # every sor_fuse gives the same payload


def test_tolerance_group_over_several_tiles(gpu64, synth):
    _equals_alone(gpu64, "f64", synth, 135, 68, 5, [0, 1], dict(KW, nscales=2), opts=dict(sor_exact=0, sor_fuse=0), values=False)


def test_tolerance_group_of_nine_fields_takes_the_colour_kernel(gpu64, synth):
    _equals_alone(gpu64, "f64", synth, 24, 20, 10, [0, 1], dict(KW, nscales=1), opts=dict(sor_exact=0, sor_fuse=0), values=False)


# ---- 4. f32 storage --------------------------------------------------------------------------------------------------------
def test_f32_context_with_float_frames(gpu32, synth):
    c = CASES["b"]
    _equals_alone(gpu32, "f32", synth, c["nx"], c["ny"], c["frames"], c["ks"], c["kw"], dtype=np.float32)


# ---- 5. sharing ------------------------------------------------------------------------------------------------------------
def test_sequences_may_share_their_frames(gpu64, synth):
    c = CASES["b"]
    nx, ny, frames, kw = c["nx"], c["ny"], c["frames"], c["kw"]
    tables, got = _equals_alone(gpu64, "f64", synth, nx, ny, frames, [1, 1], kw)           # the same clip twice
    assert np.array_equal(got[0], got[1])
    # two sequences that share ONE frame pointer: clip 0, and clip 0 with its last frame in the middle too
    p = _seq(synth, nx, ny, frames, 0)
    other = [p[0], p[3], p[2], p[3]]
    flo = _payloads(frames - 1, ny, nx)
    gpu64.brox_temporal_dev(other, _ptrs(flo), nx, ny, **kw)
    gpu64.synchronize()
    want = [_lone(gpu64, "f64", synth, nx, ny, frames, 0, kw, {})[0], flo.cpu().numpy()]
    flo2 = _payloads(2 * (frames - 1), ny, nx)
    gpu64.brox_temporal_group_dev(p + other, _ptrs(flo2), nx, ny, frames, **kw)
    gpu64.synchronize()
    got = flo2.cpu().numpy().reshape(2, frames - 1, ny, nx, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[0], got[1])


# ---- 6. errors -------------------------------------------------------------------------------------------------------------
def test_errors_are_found_before_any_work(ofx_mod, gpu64, synth):
    c = CASES["b"]
    nx, ny, frames, kw = c["nx"], c["ny"], c["frames"], c["kw"]
    F = [p for k in (0, 1) for p in _seq(synth, nx, ny, frames, k)]
    flo = _payloads(17 * 32, ny, nx)
    P = _ptrs(flo)[:2 * (frames - 1)]

    def refused(status, f, p, fr=frames, x=nx, y=ny, where=None, **over):
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.brox_temporal_group_dev(f, p, x, y, fr, **dict(kw, **over))
        assert e.value.status == status, (over, e.value.status, str(e.value))
        for w in ([where] if isinstance(where, str) else (where or [])):
            assert w in str(e.value), str(e.value)

    L = ofx_mod.lib()
    arr = lambda xs: (C.c_void_p * len(xs))(*xs)
    tail = (nx, ny, 18.0, 7.0, 2, 0.75, 1e-4, 1, 3, None)
    assert L.ofx_brox_temporal_group_dev(gpu64.h, 0, frames, arr(F), arr(P), *tail) == 1                  # n_seq 0
    assert "1..16" in L.ofx_last_error(gpu64.h).decode()
    refused(1, F[:frames] * 17, _ptrs(flo)[:17 * (frames - 1)], where="1..16")                          # n_seq 17
    refused(1, F[:4], _ptrs(flo)[:2], fr=2)                                                              # frames 2
    refused(1, F[:1] * 66, _ptrs(flo)[:64], fr=33)                                                       # frames 33
    for f, p in ((None, arr(P)), (arr(F), None)):                                                        # a NULL array
        assert L.ofx_brox_temporal_group_dev(gpu64.h, 2, frames, f, p, *tail) == 1
    k = frames + 2                                                                                       # frame 2 of sequence 1
    refused(1, F[:k] + [None] + F[k + 1:], P, where=["frame 2", "sequence 1"])
    refused(1, F[:k] + [F[k] + 4] + F[k + 1:], P, where=["frame 2", "sequence 1"])
    k = (frames - 1) + 1                                                                                 # payload 1 of sequence 1
    refused(1, F, P[:k] + [None] + P[k + 1:], where=["pointer 1", "sequence 1"])
    refused(1, F, P[:k] + [P[k] + 4] + P[k + 1:], where=["pointer 1", "sequence 1"])
    refused(1, F, P, inner=-1)
    refused(1, F, P, outer=-1)
    refused(1, F, P, x=2, y=2, nscales=1)                                                                # a 2x2 level
    refused(2, F, P, x=5, y=ny, nscales=1)                                                               # the presmoothing Gaussian does not fit
    refused(2, F, P, nscales=11)                                                                         # nor the zoom Gaussian its level
    assert _untouched(flo)
    _equals_alone(gpu64, "f64", synth, nx, ny, frames, [0, 1], kw)                                       # the context is as good as new


# ---- 7. batch --------------------------------------------------------------------------------------------------------------
B_SEQ = 5


def _one_sequence_bytes(ofx_mod, nx, ny, frames, nu):
    """the header's memory rule for one sequence at two scales, f64 storage, default sor_batch"""
    nx1, ny1 = ofx_mod.zoom_size(nx, ny, nu)
    level_px = nx * ny + nx1 * ny1
    return 1.05 * 8 * (level_px * (frames + (27 + 2 * 64) * (frames - 1)) + 2 * frames * nx * ny)


def _batch(ofx_mod, ctxs, synth, nx, ny, frames, kw):
    flo = _payloads(B_SEQ * (frames - 1), ny, nx)
    dF = [p for k in range(B_SEQ) for p in _seq(synth, nx, ny, frames, k)]
    work = ofx_mod.brox_temporal_batch_dev(ctxs, dF, _ptrs(flo), nx, ny, frames, **kw)
    return work, flo


@pytest.mark.parametrize("n_ctx", [1, 2])
def test_batch_in_lockstep_groups(ofx_mod, gpu64, synth, n_ctx):
    c = CASES["b"]
    nx, ny, frames, kw = c["nx"], c["ny"], c["frames"], c["kw"]
    lone = [_lone(gpu64, "f64", synth, nx, ny, frames, k, kw, {}) for k in range(B_SEQ)]
    assert len({l[0].tobytes() for l in lone}) == B_SEQ
    ctxs = [gpu64] + [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(n_ctx - 1)]
    per = _one_sequence_bytes(ofx_mod, nx, ny, frames, kw["nu"])
    # groups of 2, 2, 1; then a budget of one sequence per context; groups of 4 asked for under a budget of two sequences per
    # context (the group size is reduced and stays a group); then a budget that holds none
    for lockstep, budget in ((2, 0), (2, (n_ctx + 0.5) * per), (4, (2 * n_ctx + 0.5) * per)):
        with _options(gpu64, lockstep=lockstep, mem_budget=budget):
            work, flo = _batch(ofx_mod, ctxs, synth, nx, ny, frames, kw)
        got = flo.cpu().numpy().reshape(B_SEQ, frames - 1, ny, nx, 2)
        for q in range(B_SEQ):
            assert np.array_equal(got[q], lone[q][0]), (budget, q)
            assert work[q] == lone[q][3] > 0, (budget, q)
    with _options(gpu64, lockstep=2, mem_budget=0.5 * per):
        with pytest.raises(ofx_mod.OfxError) as e:
            work, flo = _batch(ofx_mod, ctxs, synth, nx, ny, frames, kw)
    assert e.value.status == 3


def test_batch_without_memory_leaves_the_payloads_untouched(ofx_mod, gpu64, synth):
    c = CASES["b"]
    nx, ny, frames, kw = c["nx"], c["ny"], c["frames"], c["kw"]
    flo = _payloads(B_SEQ * (frames - 1), ny, nx)
    dF = [p for k in range(B_SEQ) for p in _seq(synth, nx, ny, frames, k)]
    with _options(gpu64, lockstep=2, mem_budget=0.5 * _one_sequence_bytes(ofx_mod, nx, ny, frames, kw["nu"])):
        with pytest.raises(ofx_mod.OfxError) as e:
            ofx_mod.brox_temporal_batch_dev([gpu64], dF, _ptrs(flo), nx, ny, frames, **kw)
    assert e.value.status == 3
    assert _untouched(flo)


def test_batch_groups_run_under_the_first_contexts_mode(ofx_mod, gpu64, synth):
    """every context of a lockstep batch solves under ctxs[0]'s sor_exact / sor_fuse, and has its own back afterwards"""
    c = CASES["b"]
    nx, ny, frames, kw = c["nx"], c["ny"], c["frames"], c["kw"]
    opts = dict(sor_exact=0, sor_fuse=2)
    with _options(gpu64, **opts):
        lone = [_lone(gpu64, "f64", synth, nx, ny, frames, k, kw, opts) for k in range(B_SEQ)]
    other = ofx_mod.Ofx(0, ofx_mod.F64)                                 # left in the exact mode
    with _options(gpu64, lockstep=2, **opts):
        work, flo = _batch(ofx_mod, [gpu64, other], synth, nx, ny, frames, kw)
    got = flo.cpu().numpy().reshape(B_SEQ, frames - 1, ny, nx, 2)
    for q in range(B_SEQ):
        assert np.array_equal(got[q], lone[q][0]) and work[q] == lone[q][3], q
    # ... also when the memory rule leaves groups of one
    per = _one_sequence_bytes(ofx_mod, nx, ny, frames, kw["nu"])
    with _options(gpu64, lockstep=2, mem_budget=2.5 * per, **opts):
        work, flo = _batch(ofx_mod, [gpu64, other], synth, nx, ny, frames, kw)
    got = flo.cpu().numpy().reshape(B_SEQ, frames - 1, ny, nx, 2)
    for q in range(B_SEQ):
        assert np.array_equal(got[q], lone[q][0]) and work[q] == lone[q][3], q
    exact = _lone(gpu64, "f64", synth, nx, ny, frames, 0, kw, {})
    flo = _payloads(frames - 1, ny, nx)
    other.brox_temporal_dev(_seq(synth, nx, ny, frames, 0), _ptrs(flo), nx, ny, **kw)
    other.synchronize()
    assert np.array_equal(flo.cpu().numpy(), exact[0]) and np.array_equal(other.stats().iterations(), exact[1])


# ---- 8. the lone entry is untouched ----------------------------------------------------------------------------------------
def test_lone_entry_after_a_group_call(gpu64, synth):
    c = CASES["b"]
    nx, ny, frames, kw = c["nx"], c["ny"], c["frames"], c["kw"]
    before = _lone(gpu64, "f64", synth, nx, ny, frames, 1, kw, {})
    st, _ = _group(gpu64, synth, nx, ny, frames, c["ks"], kw)
    assert np.array_equal(gpu64.stats().iterations(), st[0].iterations())    # the context's record: sequence 0's
    flo = _payloads(frames - 1, ny, nx)
    gpu64.brox_temporal_dev(_seq(synth, nx, ny, frames, 1), _ptrs(flo), nx, ny, **kw)
    gpu64.synchronize()
    after = gpu64.stats()
    assert np.array_equal(flo.cpu().numpy(), before[0])
    assert np.array_equal(after.iterations(), before[1]) and np.array_equal(after.errors(), before[2])
