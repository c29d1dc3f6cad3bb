"""TV-L1 warm start on the device: ofx_tvl1_group_init_dev, ofx_tvl1_batch_init_dev and ofx_tvl1_sequence_group_dev.

Strict f64 is held to the restatement (tests/tvl1_warm_ref.py) as tests/test_gpu_tvl1.py holds the plain solve to the oracle:
equal iteration tables, flows to 1e-9.  Everything else is GPU against GPU and BYTES-EQUAL in all three modes (strict, the f64
tolerance mode, float storage): a zero start is the plain entry, a pair of a mixed group is the pair alone, the start may be the
payload's own buffer, a batch is its groups, the video chain is the chained group calls, pitched 8-bit frames are the dense ones."""
import numpy as np
import pytest
from conftest import aepe

import tvl1_warm_ref as W

pytestmark = pytest.mark.gpu

PAR = dict(tau=0.25, lam=0.15, theta=0.3)
IDS = ["%dx%d_%d_%g" % s for s in W.SHAPES]
MODES = ["strict", "relaxed", "f32"]
FILL = -7.0
ERR_ARG = 1


@pytest.fixture(scope="module")
def ctxs(ofx_mod):
    """contexts of this module alone (their options must not leak into the session's): two per mode, for the batches"""
    c = {"strict": [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)], "relaxed": [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)],
         "f32": [ofx_mod.Ofx(0, ofx_mod.F32) for _ in range(2)]}
    for x in c["relaxed"]:
        x.set_option("relaxed_dual", 1)
    yield c
    for v in c.values():
        for x in v:
            x.close()


def _dtype(mode):
    import torch
    return torch.float32 if mode == "f32" else torch.float64


def _dev(planes, dtype):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p)).to("cuda", dtype) for p in planes]


def _group(ctx, A, B, init, nx, ny, inplace=False, plain=False, **kw):
    """ofx_tvl1_group_init_dev (plain: ofx_tvl1_group_dev) on lists of device tensors; init: None, or per pair None | a (ny, nx, 2)
    float32 array.  inplace: the start lies in the payload's own buffer.  -> (payloads (G, ny, nx, 2), iteration tables)"""
    import torch
    G = len(A)
    flo = torch.full((G, ny, nx, 2), FILL, dtype=torch.float32, device="cuda")
    starts = None
    if init is not None:
        starts = []
        keep = []
        for g, P in enumerate(init):
            if P is None:
                starts.append(None)
            elif inplace:
                flo[g].copy_(torch.from_numpy(np.ascontiguousarray(P)))
                starts.append(flo[g].data_ptr())
            else:
                keep.append(torch.from_numpy(np.ascontiguousarray(P)).cuda())
                starts.append(keep[-1].data_ptr())
    torch.cuda.synchronize()
    a, b, f = [t.data_ptr() for t in A], [t.data_ptr() for t in B], [flo[g].data_ptr() for g in range(G)]
    st = ctx.tvl1_group_dev(a, b, f, nx, ny, **kw) if plain else ctx.tvl1_group_init_dev(a, b, starts, f, nx, ny, **kw)
    ctx.synchronize()
    return flo.cpu().numpy(), [s.iterations().copy() for s in st]


def _mixed(synth, nx, ny):
    """five pairs (P0 and P1 variants) and their starts: warm and cold pairs in one group, a start with NaN / Inf among them"""
    spec = [("P1", 0), ("P0", 0), ("P1", 3), ("P0", 2), ("P1", 5)]
    pairs = [synth.pair(name, nx, ny, k) for name, k in spec]
    init = [W.smooth_flow(nx, ny), None, W.edge_flow(nx, ny), None, W.broken_flow(nx, ny)]
    return pairs, init


# ---- strict f64 against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_strict_f64_is_the_restatement(ctxs, orc, synth, shape):
    nx, ny, nscales, zfactor = shape
    ctx = ctxs["strict"][0]
    I0, I1 = synth.pair("P1", nx, ny)
    for name, P in (("smooth", W.smooth_flow(nx, ny)), ("broken", W.broken_flow(nx, ny))):
        uo, vo, it_o, _ = W.tvl1_multiscale_warm(orc, I0, I1, P, nscales=nscales, zfactor=zfactor, **PAR)
        got, it = _group(ctx, _dev([I0], _dtype("strict")), _dev([I1], _dtype("strict")), [P], nx, ny, nscales=nscales, zfactor=zfactor,
                         **PAR)
        assert np.array_equal(it[0], it_o), (name, it[0], it_o)
        want = W.payload_of(uo, vo)
        d = float(np.abs(got[0].astype(np.float64) - want.astype(np.float64)).max())
        print("%s: max abs against the restatement's payload %.3g" % (name, d))
        assert d < 1e-9, (name, d)


# ---- GPU against GPU, bytes equal ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_zero_start_is_the_plain_entry(ctxs, synth, mode, shape):
    nx, ny, nscales, zfactor = shape
    ctx = ctxs[mode][0]
    pairs = [synth.pair("P1", nx, ny), synth.pair("P0", nx, ny)]
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    kw = dict(nscales=nscales, zfactor=zfactor, **PAR)
    want, it_w = _group(ctx, A, B, None, nx, ny, plain=True, **kw)
    assert np.isfinite(want).all()
    zero = np.zeros((ny, nx, 2), dtype=np.float32)
    for name, init in (("NULL table", None), ("NULL entries", [None, None]), ("zero payloads", [zero, zero]), ("mixed", [zero, None])):
        got, it = _group(ctx, A, B, init, nx, ny, **kw)
        assert got.tobytes() == want.tobytes(), name
        assert all(np.array_equal(x, y) for x, y in zip(it, it_w)), name


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_every_pair_of_a_mixed_group_is_the_pair_alone_and_the_start_may_be_in_place(ctxs, synth, mode, shape):
    nx, ny, nscales, zfactor = shape
    ctx = ctxs[mode][0]
    pairs, init = _mixed(synth, nx, ny)
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    kw = dict(nscales=nscales, zfactor=zfactor, **PAR)
    got, it = _group(ctx, A, B, init, nx, ny, **kw)
    assert np.isfinite(got).all()
    for g in range(len(pairs)):
        lone, it_l = _group(ctx, [A[g]], [B[g]], [init[g]], nx, ny, **kw)
        assert got[g].tobytes() == lone[0].tobytes(), g
        assert np.array_equal(it[g], it_l[0]), g
    assert got[0].tobytes() != _group(ctx, [A[0]], [B[0]], None, nx, ny, **kw)[0][0].tobytes()      # the start does reach the solve
    same, it_s = _group(ctx, A, B, init, nx, ny, inplace=True, **kw)
    assert same.tobytes() == got.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(it, it_s))


@pytest.mark.parametrize("mode", MODES)
def test_batch_on_two_contexts_is_the_group_entry(ofx_mod, ctxs, synth, mode):
    import torch
    nx, ny, nscales, zfactor = W.SHAPES[0]
    pairs, init = _mixed(synth, nx, ny)
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    kw = dict(nscales=nscales, zfactor=zfactor, **PAR)
    want, _ = _group(ctxs[mode][0], A, B, init, nx, ny, **kw)
    starts = [None if P is None else torch.from_numpy(P).cuda() for P in init]
    flo = torch.full((len(pairs), ny, nx, 2), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    work = ofx_mod.tvl1_batch_init_dev(ctxs[mode], [t.data_ptr() for t in A], [t.data_ptr() for t in B],
                                       [None if t is None else t.data_ptr() for t in starts], [flo[g].data_ptr() for g in range(len(pairs))],
                                       nx, ny, **kw)
    assert len(work) == len(pairs) and all(w > 0 for w in work)
    assert flo.cpu().numpy().tobytes() == want.tobytes()
    # ... and without a table it is the plain batch
    plain = torch.full_like(flo, FILL)
    again = torch.full_like(flo, FILL)
    torch.cuda.synchronize()
    ptrs = lambda t: [t[g].data_ptr() for g in range(len(pairs))]
    ofx_mod.tvl1_batch_dev(ctxs[mode], [t.data_ptr() for t in A], [t.data_ptr() for t in B], ptrs(plain), nx, ny, **kw)
    ofx_mod.tvl1_batch_init_dev(ctxs[mode], [t.data_ptr() for t in A], [t.data_ptr() for t in B], None, ptrs(again), nx, ny, **kw)
    assert again.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nscales_next", [1, 2])
def test_the_video_chain_is_the_chained_group_calls(ctxs, synth, mode, nscales_next):
    import torch
    nx, ny, n_seq, n_frames, nscales_first = 67, 45, 3, 4, 3
    ctx = ctxs[mode][0]
    F = [_dev(synth.sequence(nx, ny, n_frames, k), _dtype(mode)) for k in range(n_seq)]
    flo = torch.full((n_seq, n_frames - 1, ny, nx, 2), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = ctx.tvl1_sequence_group_dev([[t.data_ptr() for t in f] for f in F],
                                     [[flo[q, t].data_ptr() for t in range(n_frames - 1)] for q in range(n_seq)], nx, ny,
                                     nscales_first=nscales_first, nscales_next=nscales_next, **PAR)
    ctx.synchronize()
    got = flo.cpu().numpy()
    assert np.isfinite(got).all()
    prev = None
    for t in range(n_frames - 1):
        ns = nscales_next if t else nscales_first
        want, it = _group(ctx, [f[t] for f in F], [f[t + 1] for f in F], prev, nx, ny, nscales=ns, **PAR)
        for q in range(n_seq):
            assert got[q, t].tobytes() == want[q].tobytes(), (q, t)
            assert st[q][t].nscales == ns and np.array_equal(st[q][t].iterations(), it[q]), (q, t)
        prev = [want[q] for q in range(n_seq)]
    assert got[0, 1].tobytes() != got[0, 0].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_pitched_8_bit_frames_are_the_dense_ones(ofx_mod, ctxs, synth, mode):
    import torch
    nx, ny, nscales, zfactor = W.SHAPES[0]
    ctx = ctxs[mode][0]
    I0, I1 = synth.pair("P0", nx, ny)                            # integer grey levels
    assert np.array_equal(I0, I0.astype(np.uint8)) and np.array_equal(I1, I1.astype(np.uint8))
    P = W.smooth_flow(nx, ny)
    kw = dict(nscales=nscales, zfactor=zfactor, **PAR)
    want, it_w = _group(ctx, _dev([I0], _dtype(mode)), _dev([I1], _dtype(mode)), [P], nx, ny, **kw)
    pitch = 96
    surf = torch.full((2, ny, pitch), 201, dtype=torch.uint8, device="cuda")
    surf[0, :, :nx] = torch.from_numpy(I0.astype(np.uint8))
    surf[1, :, :nx] = torch.from_numpy(I1.astype(np.uint8))
    ctx.set_option("input", ofx_mod.IN_U8)
    ctx.set_option("input_pitch", pitch)
    try:
        got, it = _group(ctx, [surf[0]], [surf[1]], [P], nx, ny, **kw)
    finally:
        ctx.set_option("input", ofx_mod.IN_STORAGE)
        ctx.set_option("input_pitch", 0)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(it[0], it_w[0])


# ---- the f64 tolerance mode against its restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_tolerance_mode_is_its_restatement(ctxs, orc, synth, shape):
    """the bars of tests/test_gpu_relaxed_modes.py for the plain multiscale solve (check_tolerance_solve): equal iteration tables,
    flows within 1e-9.  The entry hands out float32, so the 1e-9 is taken before the rounding: every component lies between the
    float32 of the restatement's value - 1e-9 and that of its value + 1e-9."""
    nx, ny, nscales, zfactor = shape
    ctx = ctxs["relaxed"][0]
    I0, I1 = synth.pair("P1", nx, ny)
    P = W.smooth_flow(nx, ny)
    uo, vo, it_o, _ = W.tvl1_multiscale_warm(orc, I0, I1, P, nscales=nscales, zfactor=zfactor, relaxed=1, **PAR)
    got, it = _group(ctx, _dev([I0], _dtype("relaxed")), _dev([I1], _dtype("relaxed")), [P], nx, ny, nscales=nscales, zfactor=zfactor, **PAR)
    assert np.array_equal(it[0], it_o), (it[0], it_o)
    want = np.stack([uo, vo], axis=-1)
    lo, hi = (want - 1e-9).astype(np.float32), (want + 1e-9).astype(np.float32)
    print("components off the restatement's own float32: %d" % int((got[0] != want.astype(np.float32)).sum()))
    assert ((got[0] >= lo) & (got[0] <= hi)).all()


# ---- float storage against the strict warm result ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_f32_storage_stays_inside_the_north_star(ctxs, synth, shape):
    """AEPE against the strict warm result below the project's 1e-4 px (BASELINE north star), on P0, where the cold float solve is
    inside it (test_multiscale_f32_storage)"""
    nx, ny, nscales, zfactor = shape
    I0, I1 = synth.pair("P0", nx, ny)
    P = W.smooth_flow(nx, ny)
    kw = dict(nscales=nscales, zfactor=zfactor, **PAR)
    s, _ = _group(ctxs["strict"][0], _dev([I0], _dtype("strict")), _dev([I1], _dtype("strict")), [P], nx, ny, **kw)
    f, _ = _group(ctxs["f32"][0], _dev([I0], _dtype("f32")), _dev([I1], _dtype("f32")), [P], nx, ny, **kw)
    e = aepe(f[0, ..., 0].astype(np.float64), f[0, ..., 1].astype(np.float64), s[0, ..., 0].astype(np.float64), s[0, ..., 1].astype(np.float64))
    print("AEPE f32 storage against strict, warm: %.3g" % e)
    assert e < 1e-4, e


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_invalid_arguments_and_write_nothing(ofx_mod, ctxs, synth):
    import torch
    nx, ny = 67, 45
    ctx = ctxs["strict"][0]
    F = _dev(synth.sequence(nx, ny, 3), torch.float64)
    start = torch.from_numpy(np.concatenate([W.smooth_flow(nx, ny).ravel(), np.zeros(2, dtype=np.float32)])).cuda()
    flo = torch.full((17, 2, ny, nx, 2), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ofx_mod.OfxError) as e:                   # a start off its 8 bytes, its pair named
        ctx.tvl1_group_init_dev([F[0].data_ptr()] * 2, [F[1].data_ptr()] * 2, [start.data_ptr(), start.data_ptr() + 4],
                                [flo[0, 0].data_ptr(), flo[1, 0].data_ptr()], nx, ny, nscales=3, **PAR)
    assert e.value.status == ERR_ARG and "pair 1" in str(e.value)
    with pytest.raises(ofx_mod.OfxError) as e:                   # 17 sequences
        ctx.tvl1_sequence_group_dev([[t.data_ptr() for t in F]] * 17, [[flo[q, t].data_ptr() for t in range(2)] for q in range(17)], nx,
                                    ny, nscales_first=3, nscales_next=1, **PAR)
    assert e.value.status == ERR_ARG
    with pytest.raises(ofx_mod.OfxError) as e:                   # one frame
        ctx.tvl1_sequence_group_dev([[F[0].data_ptr()]], [[]], nx, ny, nscales_first=3, nscales_next=1, **PAR)
    assert e.value.status == ERR_ARG
    with pytest.raises(ofx_mod.OfxError) as e:                   # the second pyramid is checked before the first step runs
        ctx.tvl1_sequence_group_dev([[t.data_ptr() for t in F]], [[flo[0, t].data_ptr() for t in range(2)]], nx, ny, nscales_first=3,
                                    nscales_next=7, **PAR)
    assert e.value.status == 2
    ctx.synchronize()
    assert (flo.cpu().numpy() == FILL).all()
