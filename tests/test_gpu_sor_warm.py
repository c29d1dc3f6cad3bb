"""SOR warm start on the device: ofx_hs_/ofx_brox_ group_init_dev, batch_init_dev and sequence_group_dev.

Exact mode in f64 is held to the restatement (tests/sor_warm_ref.py) with the bars tests/test_gpu_sor.py holds for the plain solves:
equal sweep tables, Horn-Schunck to 1e-12 and Brox to 1e-11 -- taken on the float32 payload, so a component may also be off by the
rounding to float, 2^-24 of its size.  The tolerance mode (sor_exact = 0, the tile sweeps) is held to the restatement in the same
sweep order as tests/test_gpu_sor_tile.py holds the plain groups: the payload is the float32 of the restatement's flow, bit for bit.
Everything else is GPU against GPU and BYTES-EQUAL in three modes (exact f64, tile sweeps, float storage): a NULL table, NULL
entries and zero payloads are the plain entry, a pair of a mixed group is the pair alone, the start may lie in the payload's own
buffer, a batch is its groups, the video chain is the chained group calls, pitched 8-bit frames are the dense ones."""
import numpy as np
import pytest
from conftest import aepe

import sor_warm_ref as S
import tvl1_warm_ref as W

pytestmark = pytest.mark.gpu

IDS = ["%dx%d_%d_%d_%g" % s for s in S.SHAPES]
MODES = ["exact", "tile", "f32"]
SOLVERS = ["hs", "brox"]
FILL = -7.0
ERR_ARG, ERR_SIGMA = 1, 2
HS = dict(alpha=15.0, warps=4, TOL=1e-4, maxiter=150)
BROX = dict(alpha=50.0, gamma=10.0, TOL=1e-4, inner=1, outer=6)               # as test_brox_exact
BAR = {"hs": 1e-12, "brox": 1e-11}                                          # tests/test_gpu_sor.py, exact mode


@pytest.fixture(scope="module")
def ctxs(ofx_mod):
    """contexts of this module alone (their options must not leak into the session's): two per mode, for the batches"""
    c = {"exact": [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)], "tile": [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)],
         "f32": [ofx_mod.Ofx(0, ofx_mod.F32) for _ in range(2)]}
    for x in c["tile"]:
        x.set_option("sor_exact", 0)
    yield c
    for v in c.values():
        for x in v:
            x.close()


@pytest.fixture()
def tol_orc(orc):
    """the oracle and the shim's copy of it in the tolerance mode's sweep orders: colour order, the finest Brox level as a
    checkerboard of 128 x 64 tiles (the defaults of sor_tile_w and sor_wave_levels)"""
    orc.set_sor_order(1)
    orc.set_sor_wave_levels(1)
    orc.set_sor_tile(128, 64)
    S.sync_orders(1, (128, 64), 1)
    yield orc
    orc.set_sor_order(0)
    orc.set_sor_wave_levels(0)
    S.sync_orders()


def _dtype(mode):
    import torch
    return torch.float32 if mode == "f32" else torch.float64


def _dev(planes, dtype):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p)).to("cuda", dtype) for p in planes]


def _kw(solver, shape, **over):
    nx, ny, hs_ns, bx_ns, z = shape
    kw = dict(HS, nscales=hs_ns, zfactor=z) if solver == "hs" else dict(BROX, nscales=bx_ns, nu=z)
    kw.update(over)
    return kw


def _restate(solver, lib, I1, I2, P, **kw):
    return (S.hs_pyramidal_warm if solver == "hs" else S.brox_spatial_warm)(lib, I1, I2, P, **kw)


def _group(ctx, solver, A, B, init, nx, ny, inplace=False, plain=False, **kw):
    """ofx_*_group_init_dev (plain: ofx_*_group_dev) on lists of device tensors; init: None, or per pair None | a (ny, nx, 2)
    float32 array.  inplace: the start lies in the payload's own buffer.  -> (payloads (G, ny, nx, 2), sweep tables, records)"""
    import torch
    G = len(A)
    flo = torch.full((G, ny, nx, 2), FILL, dtype=torch.float32, device="cuda")
    starts, keep = None, []
    if init is not None:
        starts = []
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
    if plain:
        st = (ctx.hs_group_dev if solver == "hs" else ctx.brox_group_dev)(a, b, f, nx, ny, **kw)
    else:
        st = (ctx.hs_group_init_dev if solver == "hs" else ctx.brox_group_init_dev)(a, b, starts, f, nx, ny, **kw)
    ctx.synchronize()
    return flo.cpu().numpy(), [s.iterations().copy() for s in st], st


def _inside(got, u, v, bar):
    """|double(payload) - restatement| <= 2^-24 |restatement| + bar, per component; returns the largest excess over the rounding"""
    want = np.stack([u, v], axis=-1)
    d = np.abs(got.astype(np.float64) - want)
    print("max abs against the restatement %.3g (its float32 is off by up to %.3g)" % (d.max(), (2.0 ** -24 * np.abs(want)).max()))
    return bool((d <= 2.0 ** -24 * np.abs(want) + bar).all())


def _mixed(synth, nx, ny):
    """five pairs (P0 and P1 variants) and their starts: warm, cold and NULL pairs in one group, a start with NaN / Inf among them"""
    spec = [("P1", 0), ("P0", 0), ("P1", 3), ("P0", 2), ("P1", 5)]
    pairs = [synth.pair(name, nx, ny, k) for name, k in spec]
    init = [W.smooth_flow(nx, ny), None, W.edge_flow(nx, ny), np.zeros((ny, nx, 2), dtype=np.float32), W.broken_flow(nx, ny)]
    return pairs, init


# ---- 1. exact mode, f64, against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_exact_f64_is_the_restatement(ctxs, orc, synth, solver, shape):
    nx, ny = shape[:2]
    ctx = ctxs["exact"][0]
    kw = _kw(solver, shape)
    I1, I2 = synth.pair("P1", nx, ny)
    starts = [W.smooth_flow(nx, ny), W.edge_flow(nx, ny), W.broken_flow(nx, ny)]
    want = [_restate(solver, orc, I1, I2, P, **kw) for P in starts]
    A, B = _dev([I1] * 3, _dtype("exact")), _dev([I2] * 3, _dtype("exact"))
    try:
        for lds in (0, 2):
            ctx.set_option("sor_lds", lds)
            got, it, _ = _group(ctx, solver, A, B, starts, nx, ny, **kw)
            for g, (u, v, it_o) in enumerate(want):
                assert np.array_equal(it[g], it_o), (lds, g, it[g], it_o)
                assert _inside(got[g], u, v, BAR[solver]), (lds, g)
    finally:
        ctx.set_option("sor_lds", 1)


# ---- 2. NULL table, NULL entries and zero payloads against the plain entries -------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_zero_start_is_the_plain_entry(ctxs, synth, solver, mode, shape):
    nx, ny = shape[:2]
    ctx = ctxs[mode][0]
    kw = _kw(solver, shape)
    pairs = [synth.pair("P1", nx, ny), synth.pair("P0", nx, ny)]
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    want, it_w, st_w = _group(ctx, solver, A, B, None, nx, ny, plain=True, **kw)
    assert np.isfinite(want).all()
    zero = np.zeros((ny, nx, 2), dtype=np.float32)
    for name, init in (("NULL table", None), ("NULL entries", [None, None]), ("zero payloads", [zero, zero]), ("mixed", [zero, None])):
        got, it, st = _group(ctx, solver, A, B, init, nx, ny, **kw)
        assert got.tobytes() == want.tobytes(), name
        assert all(np.array_equal(x, y) for x, y in zip(it, it_w)), name
        if mode == "exact":                                      # the stopping values too
            assert all(np.array_equal(x.errors(), y.errors()) for x, y in zip(st, st_w)), name


# ---- 3. groups, batches and pitched frames -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_every_pair_of_a_mixed_group_is_the_pair_alone_and_the_start_may_be_in_place(ctxs, synth, solver, mode, shape):
    nx, ny = shape[:2]
    ctx = ctxs[mode][0]
    kw = _kw(solver, shape)
    pairs, init = _mixed(synth, nx, ny)
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    got, it, _ = _group(ctx, solver, A, B, init, nx, ny, **kw)
    assert np.isfinite(got).all()
    for g in range(len(pairs)):
        lone, it_l, _ = _group(ctx, solver, [A[g]], [B[g]], [init[g]], nx, ny, **kw)
        assert got[g].tobytes() == lone[0].tobytes(), g
        assert np.array_equal(it[g], it_l[0]), g
    assert got[0].tobytes() != _group(ctx, solver, [A[0]], [B[0]], None, nx, ny, **kw)[0][0].tobytes()   # the start does reach the solve
    same, it_s, _ = _group(ctx, solver, A, B, init, nx, ny, inplace=True, **kw)
    assert same.tobytes() == got.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(it, it_s))


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("mode", MODES)
def test_batch_on_two_contexts_is_the_group_entry(ofx_mod, ctxs, synth, solver, mode):
    import torch
    shape = S.SHAPES[0]
    nx, ny = shape[:2]
    kw = _kw(solver, shape)
    pairs, init = _mixed(synth, nx, ny)
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    want, _, _ = _group(ctxs[mode][0], solver, A, B, init, nx, ny, **kw)
    starts = [None if P is None else torch.from_numpy(P).cuda() for P in init]
    flo = torch.full((len(pairs), ny, nx, 2), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    batch_init = ofx_mod.hs_batch_init_dev if solver == "hs" else ofx_mod.brox_batch_init_dev
    batch = ofx_mod.hs_batch_dev if solver == "hs" else ofx_mod.brox_batch_dev
    ptrs = lambda t: [t[g].data_ptr() for g in range(len(pairs))]
    a, b = [t.data_ptr() for t in A], [t.data_ptr() for t in B]
    work = batch_init(ctxs[mode], a, b, [None if t is None else t.data_ptr() for t in starts], ptrs(flo), nx, ny, **kw)
    assert len(work) == len(pairs) and all(w > 0 for w in work)
    assert flo.cpu().numpy().tobytes() == want.tobytes()
    # ... and without a table it is the plain batch
    plain = torch.full_like(flo, FILL)
    again = torch.full_like(flo, FILL)
    torch.cuda.synchronize()
    batch(ctxs[mode], a, b, ptrs(plain), nx, ny, **kw)
    batch_init(ctxs[mode], a, b, None, ptrs(again), nx, ny, **kw)
    assert again.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("mode", MODES)
def test_pitched_8_bit_frames_are_the_dense_ones(ofx_mod, ctxs, synth, solver, mode):
    import torch
    shape = S.SHAPES[0]
    nx, ny = shape[:2]
    ctx = ctxs[mode][0]
    kw = _kw(solver, shape)
    I1, I2 = synth.pair("P0", nx, ny)                            # integer grey levels
    assert np.array_equal(I1, I1.astype(np.uint8)) and np.array_equal(I2, I2.astype(np.uint8))
    P = W.smooth_flow(nx, ny)
    want, it_w, _ = _group(ctx, solver, _dev([I1], _dtype(mode)), _dev([I2], _dtype(mode)), [P], nx, ny, **kw)
    pitch = 96
    surf = torch.full((2, ny, pitch), 201, dtype=torch.uint8, device="cuda")
    surf[0, :, :nx] = torch.from_numpy(I1.astype(np.uint8))
    surf[1, :, :nx] = torch.from_numpy(I2.astype(np.uint8))
    ctx.set_option("input", ofx_mod.IN_U8)
    ctx.set_option("input_pitch", pitch)
    try:
        got, it, _ = _group(ctx, solver, [surf[0]], [surf[1]], [P], nx, ny, **kw)
    finally:
        ctx.set_option("input", ofx_mod.IN_STORAGE)
        ctx.set_option("input_pitch", 0)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(it[0], it_w[0])


# ---- 4. the video chains -----------------------------------------------------------------------------------------------------------
def _sequence(ctx, solver, F, nx, ny, nscales_first, nscales_next, z):
    """the chain entry on lists of device frames, a warm step with half the warps / outer iterations -> (payloads, records)"""
    import torch
    n_seq, n_frames = len(F), len(F[0])
    flo = torch.full((n_seq, n_frames - 1, ny, nx, 2), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dF = [[t.data_ptr() for t in f] for f in F]
    dP = [[flo[q, t].data_ptr() for t in range(n_frames - 1)] for q in range(n_seq)]
    if solver == "hs":
        st = ctx.hs_sequence_group_dev(dF, dP, nx, ny, alpha=HS["alpha"], nscales_first=nscales_first, nscales_next=nscales_next,
                                       zfactor=z, warps_first=HS["warps"], warps_next=HS["warps"] // 2, TOL=HS["TOL"],
                                       maxiter=HS["maxiter"])
    else:
        st = ctx.brox_sequence_group_dev(dF, dP, nx, ny, alpha=BROX["alpha"], gamma=BROX["gamma"], nscales_first=nscales_first,
                                         nscales_next=nscales_next, nu=z, TOL=BROX["TOL"], inner=BROX["inner"],
                                         outer_first=BROX["outer"], outer_next=BROX["outer"] // 2)
    ctx.synchronize()
    return flo.cpu().numpy(), st


def _step_kw(solver, shape, t, nscales_first, nscales_next):
    kw = _kw(solver, shape, nscales=nscales_next if t else nscales_first)
    if t:
        kw.update(dict(warps=HS["warps"] // 2) if solver == "hs" else dict(outer=BROX["outer"] // 2))
    return kw


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nscales_next", [1, 2])
def test_the_video_chain_is_the_chained_group_calls(ctxs, orc, synth, solver, mode, nscales_next):
    shape = S.SHAPES[0]
    nx, ny, z = shape[0], shape[1], shape[4]
    n_seq, n_frames, nscales_first = 3, 4, 3
    ctx = ctxs[mode][0]
    frames = [synth.sequence(nx, ny, n_frames, k) for k in range(n_seq)]
    F = [_dev(f, _dtype(mode)) for f in frames]
    got, st = _sequence(ctx, solver, F, nx, ny, nscales_first, nscales_next, z)
    assert np.isfinite(got).all()
    prev = None
    for t in range(n_frames - 1):
        kw = _step_kw(solver, shape, t, nscales_first, nscales_next)
        want, it, _ = _group(ctx, solver, [f[t] for f in F], [f[t + 1] for f in F], prev, nx, ny, **kw)
        for q in range(n_seq):
            assert got[q, t].tobytes() == want[q].tobytes(), (q, t)
            assert st[q][t].nscales == kw["nscales"] and np.array_equal(st[q][t].iterations(), it[q]), (q, t)
            if mode == "exact":
                # ... and the restatement fed the GPU's own previous payload, so nothing accumulates along the chain
                u, v, it_o = _restate(solver, orc, frames[q][t], frames[q][t + 1], None if prev is None else prev[q], **kw)
                assert np.array_equal(it[q], it_o), (q, t, it[q], it_o)
                assert _inside(got[q, t], u, v, BAR[solver]), (q, t)
        prev = [want[q] for q in range(n_seq)]
    assert got[0, 1].tobytes() != got[0, 0].tobytes()


# ---- 5. the tolerance mode against its restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_tolerance_mode_is_its_restatement(ctxs, tol_orc, synth, solver, shape):
    """the bars of tests/test_gpu_sor_tile.py for the plain groups in the same sweep order: equal sweep tables, and the payload is
    the float32 of the restatement's flow (the start's pyramid is the checker's bit for bit: tests/test_gpu_flow_pyramid.py)"""
    nx, ny = shape[:2]
    ctx = ctxs["tile"][0]
    kw = _kw(solver, shape)
    I1, I2 = synth.pair("P1", nx, ny)
    starts = [W.smooth_flow(nx, ny), W.broken_flow(nx, ny)]
    got, it, _ = _group(ctx, solver, _dev([I1] * 2, _dtype("tile")), _dev([I2] * 2, _dtype("tile")), starts, nx, ny, **kw)
    for g, P in enumerate(starts):
        u, v, it_o = _restate(solver, tol_orc, I1, I2, P, **kw)
        assert np.array_equal(it[g], it_o), (g, it[g], it_o)
        want = np.stack([u, v], axis=-1).astype(np.float32)
        print("components off the restatement's float32: %d" % int((got[g] != want).sum()))
        assert np.array_equal(got[g], want), g


# ---- 6. float storage against the strict warm result -------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_f32_storage_stays_inside_the_north_star(ctxs, synth, solver, shape):
    """AEPE against the exact f64 warm result below the project's 1e-4 px (BASELINE north star), on P0.  Measured on an MI355X:
    see DESIGN 8.15."""
    nx, ny = shape[:2]
    kw = _kw(solver, shape)
    I1, I2 = synth.pair("P0", nx, ny)
    P = W.smooth_flow(nx, ny)
    s, _, _ = _group(ctxs["exact"][0], solver, _dev([I1], _dtype("exact")), _dev([I2], _dtype("exact")), [P], nx, ny, **kw)
    f, _, _ = _group(ctxs["f32"][0], solver, _dev([I1], _dtype("f32")), _dev([I2], _dtype("f32")), [P], nx, ny, **kw)
    e = aepe(f[0, ..., 0].astype(np.float64), f[0, ..., 1].astype(np.float64), s[0, ..., 0].astype(np.float64), s[0, ..., 1].astype(np.float64))
    print("AEPE f32 storage against exact f64, warm, %s %dx%d: %.3g" % (solver, nx, ny, e))
    assert e < 1e-4, e


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
def test_refusals_are_invalid_arguments_and_write_nothing(ofx_mod, ctxs, synth, solver):
    import torch
    shape = S.SHAPES[0]
    nx, ny = shape[:2]
    ctx = ctxs["exact"][0]
    kw = _kw(solver, shape)
    group = ctx.hs_group_init_dev if solver == "hs" else ctx.brox_group_init_dev
    seq = ctx.hs_sequence_group_dev if solver == "hs" else ctx.brox_sequence_group_dev
    batch = ofx_mod.hs_batch_init_dev if solver == "hs" else ofx_mod.brox_batch_init_dev
    F = _dev(synth.sequence(nx, ny, 3), torch.float64)
    guard = 16
    start = torch.from_numpy(np.concatenate([W.smooth_flow(nx, ny).ravel(), np.zeros(2, dtype=np.float32)])).cuda()
    flo = torch.full((17 * 2 * ny * nx * 2 + 2 * guard,), FILL, dtype=torch.float32, device="cuda")
    slot = lambda q, t: flo[guard:].data_ptr() + 4 * ((q * 2 + t) * ny * nx * 2)
    torch.cuda.synchronize()
    a, b = [F[0].data_ptr()] * 2, [F[1].data_ptr()] * 2
    with pytest.raises(ofx_mod.OfxError) as e:                   # a start off its 8 bytes, its pair named
        group(a, b, [start.data_ptr(), start.data_ptr() + 4], [slot(0, 0), slot(1, 0)], nx, ny, **kw)
    assert e.value.status == ERR_ARG and "pair 1" in str(e.value) and "8-byte" in str(e.value)
    with pytest.raises(ofx_mod.OfxError) as e:                   # ... through the batch as well
        batch(ctxs["exact"], a, b, [start.data_ptr(), start.data_ptr() + 4], [slot(0, 0), slot(1, 0)], nx, ny, **kw)
    assert e.value.status == ERR_ARG and "pair 1" in str(e.value)
    with pytest.raises(ofx_mod.OfxError) as e:                   # a pyramid whose Gaussian does not fit: before any work
        group(a, b, [start.data_ptr(), None], [slot(0, 0), slot(1, 0)], nx, ny, **dict(kw, nscales=7))
    assert e.value.status == ERR_SIGMA and "sigma" in str(e.value)
    with pytest.raises(ofx_mod.OfxError) as e:                   # the plain entries' refusals: 17 pairs
        group([a[0]] * 17, [b[0]] * 17, [None] * 17, [slot(q, 0) for q in range(17)], nx, ny, **kw)
    assert e.value.status == ERR_ARG and "1..16" in str(e.value)
    sk = {k: v for k, v in kw.items() if k not in ("nscales", "warps", "outer", "zfactor", "nu")}
    frames = [t.data_ptr() for t in F]
    with pytest.raises(ofx_mod.OfxError) as e:                   # 17 sequences
        seq([frames] * 17, [[slot(q, t) for t in range(2)] for q in range(17)], nx, ny, nscales_first=3, nscales_next=1, **sk)
    assert e.value.status == ERR_ARG and "1..16" in str(e.value)
    with pytest.raises(ofx_mod.OfxError) as e:                   # one frame
        seq([[frames[0]]], [[]], nx, ny, nscales_first=3, nscales_next=1, **sk)
    assert e.value.status == ERR_ARG and "frames" in str(e.value)
    with pytest.raises(ofx_mod.OfxError) as e:                   # a payload off its 8 bytes
        seq([frames], [[slot(0, 0), slot(0, 1) + 4]], nx, ny, nscales_first=3, nscales_next=1, **sk)
    assert e.value.status == ERR_ARG and "8-byte" in str(e.value)
    with pytest.raises(ofx_mod.OfxError) as e:                   # the second pyramid is checked before the first step runs
        seq([frames], [[slot(0, t) for t in range(2)]], nx, ny, nscales_first=3, nscales_next=7, **sk)
    assert e.value.status == ERR_SIGMA and "sigma" in str(e.value)
    with pytest.raises(ofx_mod.OfxError) as e:                   # a warm step without a warp / with a negative count
        seq([frames], [[slot(0, t) for t in range(2)]], nx, ny, nscales_first=3, nscales_next=1,
            **dict(sk, **(dict(warps_next=0) if solver == "hs" else dict(outer_next=-1))))
    assert e.value.status == ERR_ARG
    ctx.synchronize()
    assert (flo.cpu().numpy() == FILL).all()                     # payloads and the guard bytes around them
