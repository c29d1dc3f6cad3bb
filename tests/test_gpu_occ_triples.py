"""TV-L1 with occlusions on indexed triples of device-resident planes: ofx_tvl1occ_triples_group_dev and ofx_tvl1occ_triples_dev.

The frame table is a list of slices of device tensors (or None where no triple refers to the entry), payloads and maps slices of
one tensor each, prefilled with a sentinel.  Triple (prev, cur, next, filt) must be what the lone host entry
ofx_tvl1occ_multiscale(F[prev], F[cur], F[next], filtI0 = F[filt]) computes, bit for bit: payload = float32 of (u1, u2), map =
uint8(255 chi), equal outer-iteration tables and stopping values.  Selected triples are also compared with the CPU oracle.  The
planes are integers (synth.sequence floors, the box mean below floors), hence exact in float32 as well."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLO_SENTINEL = -7.0
OCC_SENTINEL = 7

# the sizes of tests/test_gpu_occ_sequence.py: odd n = 3015, partial blocks, map slices at every byte alignment | triples that
# stop at different outer iterations
SMALL = dict(nx=67, ny=45, kw=dict(nscales=2, warps=2, epsilon=0.01))
MID = dict(nx=96, ny=72, kw=dict(nscales=3, warps=2, epsilon=0.002))
# forward, backward and stride-2 triples over five frames
MIXED = [(0, 1, 2), (2, 1, 0), (1, 2, 3), (3, 2, 1), (0, 2, 4), (4, 2, 0), (2, 3, 4)]


def _frames(synth, case, n=4):
    return list(synth.sequence(case["nx"], case["ny"], n, 1))


def _box3(f):
    """3 x 3 box mean, edges replicated, floored: an integer g-image that is not a frame"""
    ny, nx = f.shape
    p = np.pad(f, 1, mode="edge")
    return np.floor(sum(p[dy:dy + ny, dx:dx + nx] for dy in range(3) for dx in range(3)) / 9.0)


def _full(t):
    return tuple(t) if len(t) == 4 else tuple(t) + (-1,)


def _table(planes, dtype=np.float64):
    """device tensors of the planes (None stays None) and their pointers"""
    import torch
    keep = [None if p is None else torch.from_numpy(np.ascontiguousarray(p).astype(dtype)).cuda() for p in planes]
    return keep, [None if t is None else t.data_ptr() for t in keep]


def _results(n, nx, ny):
    import torch
    flo = torch.full((n, ny, nx, 2), FLO_SENTINEL, dtype=torch.float32, device="cuda")
    occ = torch.full((n, ny * nx), OCC_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return flo, occ


def _ptrs(t):
    return [t[k].data_ptr() for k in range(t.shape[0])]


def _untouched(flo, occ):
    import torch
    torch.cuda.synchronize()
    return bool((flo == FLO_SENTINEL).all().item()) and bool((occ == OCC_SENTINEL).all().item())


def _iters(st, kw):
    return tuple(st.iters[s][w] for s in range(kw["nscales"]) for w in range(kw["warps"]))


def _errors(st, kw):
    return tuple(st.error[s][w] for s in range(kw["nscales"]) for w in range(kw["warps"]))


def _group(gpu, planes, triples, case, dtype=np.float64, **over):
    """one group call -> (records, payloads, maps) on the host"""
    keep, F = _table(planes, dtype)
    flo, occ = _results(len(triples), case["nx"], case["ny"])
    st = gpu.tvl1occ_triples_group_dev(F, triples, _ptrs(flo), _ptrs(occ), case["nx"], case["ny"], **dict(case["kw"], **over))
    gpu.synchronize()
    return st, flo.cpu().numpy(), occ.cpu().numpy().reshape(-1, case["ny"], case["nx"])


_LONE = {}


def _lone(gpu64, tag, planes, triple, kw):
    """the lone host entry on one triple of `planes` -> (payload, map, iteration table, errors, Stats fields); solved once per
    module and key"""
    a, b, c, f = _full(triple)
    key = (tag, a, b, c, b if f < 0 else f, tuple(sorted(kw.items())))
    if key not in _LONE:
        u, v, chi = gpu64.tvl1occ_multiscale(planes[a], planes[b], planes[c], filtI0=planes[b if f < 0 else f], **kw)
        st = gpu64.stats()
        _LONE[key] = (np.stack([u, v], axis=-1).astype(np.float32), (255 * chi).astype(np.uint8), _iters(st, kw), _errors(st, kw),
                      (st.nscales, st.nsolves, tuple(st.nx), tuple(st.ny), st.work_pix_iters))
    return _LONE[key]


def _equals_lone(gpu64, tag, planes, triple, kw, st, flo, occ):
    pay, chi, table, err, _ = _lone(gpu64, tag, planes, triple, kw)
    assert np.array_equal(flo, pay), triple
    assert np.array_equal(occ, chi), triple
    assert _iters(st, kw) == table, (triple, _iters(st, kw), table)
    assert _errors(st, kw) == err, triple


def _equals_oracle(orc, planes, triple, kw, flo, occ):
    a, b, c, f = _full(triple)
    uo, vo, co, _ = orc.tvl1occ_multiscale(planes[a], planes[b], planes[c], filtI0=planes[b if f < 0 else f], **kw)
    assert np.array_equal(flo, np.stack([uo, vo], axis=-1).astype(np.float32)), triple
    assert np.array_equal(occ, (255 * co).astype(np.uint8)), triple
    assert 0 < occ.mean() < 255                      # both map values occur


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_consecutive_triples_equal_the_sequence_entry(gpu64, synth):
    s = _frames(synth, MID)
    planes = [s[k] for k in (0, 1, 2, 2, 2, 3, 1)]
    kw = MID["kw"]
    triples = [(t, t + 1, t + 2, -1) for t in range(5)]
    st, flo, occ = _group(gpu64, planes, triples, MID)
    keep, F = _table(planes)
    sflo, socc = _results(5, MID["nx"], MID["ny"])
    sst = gpu64.tvl1occ_sequence_group_dev(F, _ptrs(sflo), _ptrs(socc), MID["nx"], MID["ny"], **kw)
    gpu64.synchronize()
    assert np.array_equal(flo, sflo.cpu().numpy())
    assert np.array_equal(occ, socc.cpu().numpy().reshape(occ.shape))
    for t in range(5):
        assert _iters(st[t], kw) == _iters(sst[t], kw) and _errors(st[t], kw) == _errors(sst[t], kw), t
        assert st[t].work_pix_iters == sst[t].work_pix_iters
    assert len({_iters(r, kw) for r in st}) > 1      # triples that stop at different outer iterations in one group
    for t in (1, 2):                                 # the static triples
        assert not flo[t].any() and not occ[t].any()
    assert flo[0].any() and occ[0].any()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_forward_and_backward_triples(gpu64, gpu32, synth, orc, prec):
    planes = _frames(synth, SMALL)
    kw = SMALL["kw"]
    triples = [(0, 1, 2), (2, 1, 0), (1, 2, 3), (3, 2, 1)]
    gpu, dtype = (gpu64, np.float64) if prec == "f64" else (gpu32, np.float32)
    st, flo, occ = _group(gpu, planes, triples, SMALL, dtype)
    for k, t in enumerate(triples):
        _equals_lone(gpu64, "small", planes, t, kw, st[k], flo[k], occ[k])
    _equals_oracle(orc, planes, triples[0], kw, flo[0], occ[0])
    _equals_oracle(orc, planes, triples[3], kw, flo[3], occ[3])
    assert not np.array_equal(flo[0], flo[1]) and not np.array_equal(flo[2], flo[3])


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_g_image_of_the_callers_own(gpu64, synth, orc):
    planes = _frames(synth, SMALL)
    planes.append(_box3(planes[1]))                  # index 4: not a frame
    assert np.array_equal(planes[4], np.floor(planes[4])) and not np.array_equal(planes[4], planes[1])
    kw = SMALL["kw"]
    triples = [(0, 1, 2, 4), (0, 1, 2, -1), (2, 1, 0, 4), (0, 1, 2, 1)]
    st, flo, occ = _group(gpu64, planes, triples, SMALL)
    for k, t in enumerate(triples):
        _equals_lone(gpu64, "small", planes, t, kw, st[k], flo[k], occ[k])
    _equals_oracle(orc, planes, triples[0], kw, flo[0], occ[0])
    _equals_oracle(orc, planes, triples[1], kw, flo[1], occ[1])     # the oracle alone already tells the two apart
    assert not np.array_equal(flo[0], flo[1])
    assert np.array_equal(flo[1], flo[3]) and np.array_equal(occ[1], occ[3])      # filt = -1 is filt = cur


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_table_capacity_and_repeats(gpu64, synth):
    s = _frames(synth, SMALL)
    planes = [np.roll(s[f], k, axis=1) for k in range(16) for f in range(4)]      # 64 planes: cyclic shifts of the four frames
    assert len({p.tobytes() for p in planes}) == 64
    over = dict(nscales=2, warps=1)
    kw = dict(SMALL["kw"], **over)
    triples = [(4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3) for k in range(16)]       # 16 triples, 64 distinct planes, all referenced
    st, flo, occ = _group(gpu64, planes, triples, SMALL, **over)
    for k in (0, 7, 15):
        _equals_lone(gpu64, "rolled", planes, triples[k], kw, st[k], flo[k], occ[k])
    assert len({flo[k].tobytes() for k in range(16)}) == 16
    # a sparse table: NULL wherever no triple refers to the entry; one plane in all four roles is a static triple
    triples = [(5, 5, 5, 5), (60, 61, 62, 63), (33, 33, 33, -1), (63, 5, 33, 60)]
    used = {i for t in triples for i in t if i >= 0}
    sparse = [p if i in used else None for i, p in enumerate(planes)]
    st, flo, occ = _group(gpu64, sparse, triples, SMALL, **over)
    for k in (0, 2):
        assert not flo[k].any() and not occ[k].any()
    for k in (1, 3):
        _equals_lone(gpu64, "rolled", planes, triples[k], kw, st[k], flo[k], occ[k])


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def _group_bytes(ofx_mod, case, G, D):
    """the header's memory rule for a group of G triples over D distinct planes"""
    nx, ny, level_px = case["nx"], case["ny"], 0
    for _ in range(case["kw"]["nscales"]):
        level_px += nx * ny
        nx, ny = ofx_mod.zoom_size(nx, ny, 0.5)
    full = case["nx"] * case["ny"]
    skew = (2 * (case["ny"] - 1) + case["nx"]) * case["ny"]
    return 8.0 * 1.05 * ((D + 3 * G) * level_px + (2 * D + 27 * G) * full + 13 * G * skew)


def test_group_boundaries(ofx_mod, gpu64, synth):
    planes = _frames(synth, MID, 5)
    kw = MID["kw"]
    nx, ny = MID["nx"], MID["ny"]
    st, want_flo, want_occ = _group(gpu64, planes, MIXED, MID)
    want_work = [r.work_pix_iters for r in st]
    keep, F = _table(planes)
    ctxs = [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(3)]

    def run(cs, lockstep=0, mem_budget=0.0):
        flo, occ = _results(len(MIXED), nx, ny)
        cs[0].set_option("lockstep", lockstep)
        cs[0].set_option("mem_budget", mem_budget)
        try:
            work = ofx_mod.tvl1occ_triples_dev(cs, F, MIXED, _ptrs(flo), _ptrs(occ), nx, ny, **kw)
        finally:
            cs[0].set_option("lockstep", 0)
            cs[0].set_option("mem_budget", 0)
        return work, flo, occ

    for cs, lockstep in ((ctxs[:1], 2), (ctxs, 2), (ctxs[:1], 16), (ctxs, 16), (ctxs[:1], 0), (ctxs, 0)):
        work, flo, occ = run(cs, lockstep)           # groups of 2, 2, 2, 1 | the same on three | of 7 | 3, 3, 1 | 7 | 3, 3, 1
        assert np.array_equal(flo.cpu().numpy(), want_flo), (len(cs), lockstep)
        assert np.array_equal(occ.cpu().numpy().reshape(want_occ.shape), want_occ), (len(cs), lockstep)
        assert len(work) == 7 and work == want_work, (len(cs), lockstep)
    # room for two triples (three planes: a forward / backward pair) but not for three (four planes)
    assert _group_bytes(ofx_mod, MID, 2, 3) < _group_bytes(ofx_mod, MID, 3, 4)
    work, flo, occ = run(ctxs[:1], 0, 1.001 * _group_bytes(ofx_mod, MID, 2, 3))
    assert np.array_equal(flo.cpu().numpy(), want_flo) and np.array_equal(occ.cpu().numpy().reshape(want_occ.shape), want_occ)
    assert work == want_work
    # ... and for none
    flo, occ = _results(len(MIXED), nx, ny)
    ctxs[0].set_option("mem_budget", 0.9 * _group_bytes(ofx_mod, MID, 1, 3))
    try:
        with pytest.raises(ofx_mod.OfxError) as e:
            ofx_mod.tvl1occ_triples_dev(ctxs[:1], F, MIXED, _ptrs(flo), _ptrs(occ), nx, ny, **kw)
        assert e.value.status == 3
    finally:
        ctxs[0].set_option("mem_budget", 0)
    assert _untouched(flo, occ)
    assert ofx_mod.tvl1occ_triples_dev(ctxs, F, [], [], [], nx, ny, **kw) == []      # no triples: OFX_OK


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(ofx_mod, gpu64, gpu32, synth):
    """every case of the header's error list that one device can produce (contexts on different devices need two)"""
    planes = _frames(synth, MID, 5)
    kw = MID["kw"]
    nx, ny = MID["nx"], MID["ny"]
    keep, F = _table(planes)
    flo, occ = _results(len(MIXED), nx, ny)
    P, O = _ptrs(flo), _ptrs(occ)

    def both(status, f, tr, p, o, x=nx, y=ny, text=None, **over):
        args = dict(kw, **over)
        for call in (lambda: gpu64.tvl1occ_triples_group_dev(f, tr, p, o, x, y, **args),
                     lambda: ofx_mod.tvl1occ_triples_dev([gpu64], f, tr, p, o, x, y, **args)):
            with pytest.raises(ofx_mod.OfxError) as e:
                call()
            assert e.value.status in status, (over, e.value.status)
            if text:
                assert text in str(e.value), (text, str(e.value))

    for over in (dict(nscales=0), dict(warps=0), dict(warps=65), dict(zfactor=1.0), dict(zfactor=0.0), dict(theta=0.0), dict(lam=0.0)):
        both((1,), F, MIXED, P, O, **over)                   # occ_check's arguments
    both((1,), F, MIXED, P, O, x=1, y=ny)                    # bad size
    both((1, 2), F, MIXED, P, O, nscales=9)                  # a pyramid that cannot be built / coarsest level
    both((2,), F, MIXED, P, O, nscales=6)                    # 6 x 5 is too small for the zoom Gaussian
    # an index outside the table: the triple and the role are named
    for k, r, name, bad in ((0, 0, "prev", 5), (3, 1, "cur", -1), (6, 2, "next", 99), (2, 3, "filt", 5), (4, 3, "filt", -2)):
        tr = [list(_full(t)) for t in MIXED]
        tr[k][r] = bad
        both((1,), F, tr, P, O, text="triple %d role %s" % (k, name))
    # a referenced plane that is NULL or misaligned (an unreferenced one may be either: test_table_capacity_and_repeats)
    both((1,), F[:3] + [None] + F[4:], MIXED, P, O, text="triple 2 role next")
    both((1,), F[:1] + [F[1] + 4] + F[2:], MIXED, P, O, text="triple 0 role cur")
    both((1,), F + [None], [(0, 1, 2, 5)] + MIXED[1:], P, O, text="triple 0 role filt")
    for k in (0, 6):                                         # a NULL or misaligned result pointer
        both((1,), F, MIXED, P[:k] + [None] + P[k + 1:], O, text="triple %d" % k)
        both((1,), F, MIXED, P[:k] + [P[k] + 4] + P[k + 1:], O, text="triple %d" % k)
        both((1,), F, MIXED, P, O[:k] + [None] + O[k + 1:], text="triple %d" % k)
    for n in (0, 17):                                        # n_triples outside 1 .. 16, the group entry only
        with pytest.raises(ofx_mod.OfxError) as e:
            gpu64.tvl1occ_triples_group_dev(F, MIXED[:1] * n, P[:1] * n, O[:1] * n, nx, ny, **kw)
        assert e.value.status == 1
    L = ofx_mod.lib()                                        # a NULL array
    arr = lambda xs: (C.c_void_p * len(xs))(*xs)
    tr = (ofx_mod.OccTriple * 7)(*[ofx_mod.OccTriple(*_full(t)) for t in MIXED])
    tail = (nx, ny, 0.15, 0.01, 0.15, 0.3, 3, 0.5, 2, 0.002, None)
    for f, t, p, o in ((None, tr, arr(P), arr(O)), (arr(F), None, arr(P), arr(O)), (arr(F), tr, None, arr(O)), (arr(F), tr, arr(P), None)):
        assert L.ofx_tvl1occ_triples_group_dev(gpu64.h, 5, f, 7, t, p, o, *tail) == 1
        assert L.ofx_tvl1occ_triples_dev(arr([gpu64.h.value]), 1, 5, f, 7, t, p, o, *tail) == 1
    assert L.ofx_tvl1occ_triples_dev(None, 1, 5, arr(F), 7, tr, arr(P), arr(O), *tail) == 1
    assert L.ofx_tvl1occ_triples_group_dev(gpu64.h, 0, arr(F), 7, tr, arr(P), arr(O), *tail) == 1      # an empty table
    with pytest.raises(ofx_mod.OfxError) as e:               # contexts of different precision
        ofx_mod.tvl1occ_triples_dev([gpu64, gpu32], F, MIXED, P, O, nx, ny, **kw)
    assert e.value.status == 1
    assert _untouched(flo, occ)
    # the context serves a valid call afterwards
    st = gpu64.tvl1occ_triples_group_dev(F, MIXED[:2], P[:2], O[:2], nx, ny, **kw)
    gpu64.synchronize()
    for k in range(2):
        _equals_lone(gpu64, "mid", planes, MIXED[k], kw, st[k], flo[k].cpu().numpy(), occ[k].cpu().numpy().reshape(ny, nx))
    assert _untouched(flo[2:], occ[2:])


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_stats_records(ofx_mod, gpu64, synth):
    planes = _frames(synth, MID, 5)
    kw = MID["kw"]
    nx, ny = MID["nx"], MID["ny"]
    triples = [MIXED[0], MIXED[1], MIXED[4]]         # forward, backward, stride 2
    keep, F = _table(planes)
    flo, occ = _results(3, nx, ny)
    st = gpu64.tvl1occ_triples_group_dev(F, triples, _ptrs(flo), _ptrs(occ), nx, ny, **kw)
    gpu64.synchronize()
    work = ofx_mod.tvl1occ_triples_dev([gpu64], F, triples, _ptrs(flo), _ptrs(occ), nx, ny, **kw)
    for k, t in enumerate(triples):
        nscales, nsolves, lx, ly, w = _lone(gpu64, "mid", planes, t, kw)[4]
        assert (st[k].nscales, st[k].nsolves, tuple(st[k].nx), tuple(st[k].ny)) == (nscales, nsolves, lx, ly)
        assert st[k].work_pix_iters == w == work[k]
        assert st[k].total_ms > 0
