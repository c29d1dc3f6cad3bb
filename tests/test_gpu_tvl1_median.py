"""Option "tvl1_median": TV-L1 with the flow median-filtered after every warp, on the device.

Strict f64 is held to the restatement (tests/tvl1_median_ref.py) bit for bit: equal iteration tables, maximum absolute difference
of the payloads 0.0.  The f64 tolerance mode is held to its restatement under the bars of
tests/test_gpu_tvl1_warm.py::test_tolerance_mode_is_its_restatement (equal tables, every component between the float32 of the
restatement's value -+ 1e-9), float storage under the bar of test_f32_storage_stays_inside_the_north_star (AEPE against the strict
result below 1e-4 px on P0); the median selects, it cannot widen them.  Everything else is GPU against GPU and bytes-equal: a pair
of a group is the pair alone under every kernel choice, the warm-start, bidirectional and sequence entries are the lone solves,
option 0 after option 5 is the plain solve, and values other than 0, 3, 5 are refused."""
import numpy as np
import pytest
from conftest import aepe

import tvl1_median_ref as M
import tvl1_warm_ref as W

pytestmark = pytest.mark.gpu

PAR = dict(tau=0.25, lam=0.15, theta=0.3)
IDS = ["%dx%d_%d_%g" % s for s in W.SHAPES]
MODES = ["strict", "relaxed", "f32"]
ERR_ARG = 1
KERNELS = {                                     # forced on every level: the shapes are far below the automatic thresholds
    "defaults": dict(),
    "store_a=0": dict(store_a=0),
    "store_a=2": dict(store_a=2),
    "iter3,store_a=0": dict(store_a=0, fuse3=1, fuse3_min_px=0, fuse4=0),
    "iter3,store_a=2": dict(store_a=2, fuse3=1, fuse3_min_px=0, fuse4=0),
    "iter4,store_a=0": dict(store_a=0, fuse4=1, fuse4_min_px=0),
    "iter4,store_a=2": dict(store_a=2, fuse4=1, fuse4_min_px=0),
}
DEFAULTS = dict(store_a=1, fuse3=2, fuse3_min_px=0, fuse4=2, fuse4_min_px=0, tvl1_median=0)


@pytest.fixture(scope="module")
def ctxs(ofx_mod):
    """contexts of this module alone: their options must not leak into the session's"""
    c = {"strict": ofx_mod.Ofx(0, ofx_mod.F64), "relaxed": ofx_mod.Ofx(0, ofx_mod.F64), "f32": ofx_mod.Ofx(0, ofx_mod.F32)}
    c["relaxed"].set_option("relaxed_dual", 1)
    yield c
    for x in c.values():
        x.close()


class options:
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, DEFAULTS[k])


def _dtype(mode):
    import torch
    return torch.float32 if mode == "f32" else torch.float64


def _dev(planes, dtype):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p)).to("cuda", dtype) for p in planes]


def _lone(ctx, a, b, nx, ny, **kw):
    """ofx_tvl1_multiscale_dev on two device tensors -> (payload (ny, nx, 2), iteration table)"""
    import torch
    flo = torch.full((ny, nx, 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.tvl1_multiscale_dev(a.data_ptr(), b.data_ptr(), flo.data_ptr(), nx, ny, **kw)
    ctx.synchronize()
    return flo.cpu().numpy(), ctx.stats().iterations().copy()


def _group(ctx, A, B, nx, ny, init=None, **kw):
    import torch
    G = len(A)
    flo = torch.full((G, ny, nx, 2), -7.0, dtype=torch.float32, device="cuda")
    keep = [None if P is None else torch.from_numpy(np.ascontiguousarray(P)).cuda() for P in (init or [])]
    torch.cuda.synchronize()
    a, b, f = [t.data_ptr() for t in A], [t.data_ptr() for t in B], [flo[g].data_ptr() for g in range(G)]
    if init is None:
        st = ctx.tvl1_group_dev(a, b, f, nx, ny, **kw)
    else:
        st = ctx.tvl1_group_init_dev(a, b, [None if t is None else t.data_ptr() for t in keep], f, nx, ny, **kw)
    ctx.synchronize()
    return flo.cpu().numpy(), [s.iterations().copy() for s in st]


def _three(synth, nx, ny):
    """three different pairs: different stopping iterations, so different buffers of the rotation at the end of a loop"""
    return [synth.pair("P0", nx, ny), synth.pair("P1", nx, ny, 0), synth.pair("P1", nx, ny, 1)]


# ---- against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("median", [3, 5])
@pytest.mark.parametrize("name", ["P0", "P1"])
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_strict_f64_is_the_restatement_bit_for_bit(ctxs, orc, synth, shape, name, median):
    nx, ny, nscales, zfactor = shape
    ctx = ctxs["strict"]
    I0, I1 = synth.pair(name, nx, ny)
    want, it_o = M.solve((orc, synth), name, 0, nx, ny, nscales, zfactor, median)
    plain, _ = M.solve((orc, synth), name, 0, nx, ny, nscales, zfactor, 0)
    assert want.astype(np.float32).tobytes() != plain.astype(np.float32).tobytes()                   # the filter does act
    a, b = _dev([I0, I1], _dtype("strict"))
    with options(ctx, tvl1_median=median):
        got, it = _lone(ctx, a, b, nx, ny, nscales=nscales, zfactor=zfactor, **PAR)
    assert np.array_equal(it, it_o), (it, it_o)
    d = float(np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max())
    print("max abs against the restatement's payload: %.3g" % d)
    assert d == 0.0, d


@pytest.mark.parametrize("median", [3, 5])
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_tolerance_mode_is_its_restatement(ctxs, orc, synth, shape, median):
    nx, ny, nscales, zfactor = shape
    ctx = ctxs["relaxed"]
    I0, I1 = synth.pair("P1", nx, ny)
    want, it_o = M.solve((orc, synth), "P1", 0, nx, ny, nscales, zfactor, median, 1)
    a, b = _dev([I0, I1], _dtype("relaxed"))
    with options(ctx, tvl1_median=median):
        got, it = _lone(ctx, a, b, nx, ny, nscales=nscales, zfactor=zfactor, **PAR)
    assert np.array_equal(it, it_o), (it, it_o)
    lo, hi = (want - 1e-9).astype(np.float32), (want + 1e-9).astype(np.float32)
    print("components off the restatement's own float32: %d" % int((got != want.astype(np.float32)).sum()))
    assert ((got >= lo) & (got <= hi)).all()


@pytest.mark.parametrize("median", [3, 5])
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_f32_storage_stays_inside_the_north_star(ctxs, orc, synth, shape, median):
    nx, ny, nscales, zfactor = shape
    I0, I1 = synth.pair("P0", nx, ny)
    want, _ = M.solve((orc, synth), "P0", 0, nx, ny, nscales, zfactor, median)
    a, b = _dev([I0, I1], _dtype("f32"))
    with options(ctxs["f32"], tvl1_median=median):
        got, _ = _lone(ctxs["f32"], a, b, nx, ny, nscales=nscales, zfactor=zfactor, **PAR)
    e = aepe(got[..., 0].astype(np.float64), got[..., 1].astype(np.float64), want[..., 0], want[..., 1])
    print("AEPE f32 storage against the strict restatement: %.3g" % e)
    assert np.isfinite(got).all() and e < 1e-4, e


# ---- GPU against GPU, bytes equal ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_every_pair_of_a_group_is_the_pair_alone_with_every_kernel(ctxs, synth, mode, shape):
    nx, ny, nscales, zfactor = shape
    ctx = ctxs[mode]
    pairs = _three(synth, nx, ny)
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    kw = dict(nscales=nscales, zfactor=zfactor, **PAR)
    for median in (3, 5):
        with options(ctx, tvl1_median=median):
            lone = [_lone(ctx, A[g], B[g], nx, ny, **kw) for g in range(3)]
            assert len({tuple(it.ravel()) for _, it in lone}) >= 2                  # the pairs do stop at different iterations
            for kname, opts in KERNELS.items():
                with options(ctx, **opts):
                    got, it = _group(ctx, A, B, nx, ny, **kw)
                for g in range(3):
                    assert np.array_equal(it[g], lone[g][1]), (median, kname, g)
                    assert got[g].tobytes() == lone[g][0].tobytes(), (median, kname, g)


@pytest.mark.parametrize("mode", MODES)
def test_warm_start_bidirectional_and_sequence_entries_are_the_lone_solves(ctxs, synth, mode):
    import torch
    nx, ny, nscales, zfactor = W.SHAPES[0]
    ctx = ctxs[mode]
    kw = dict(nscales=nscales, zfactor=zfactor, **PAR)
    pairs = _three(synth, nx, ny)
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    with options(ctx, tvl1_median=5):
        # a non-zero start: pair g of the group is the pair alone from the same start
        init = [W.smooth_flow(nx, ny), None, W.edge_flow(nx, ny)]
        got, it = _group(ctx, A, B, nx, ny, init=init, **kw)
        for g in range(3):
            lone, it_l = _group(ctx, [A[g]], [B[g]], nx, ny, init=[init[g]], **kw)
            assert got[g].tobytes() == lone[0].tobytes() and np.array_equal(it[g], it_l[0]), g
        cold, _ = _group(ctx, A, B, nx, ny, **kw)
        assert got[0].tobytes() != cold[0].tobytes()
        # both directions of two pairs
        flo = torch.full((4, ny, nx, 2), -7.0, dtype=torch.float32, device="cuda")
        occ = torch.zeros((4, ny, nx), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.tvl1_bidir_group_dev([A[1].data_ptr(), A[2].data_ptr()], [B[1].data_ptr(), B[2].data_ptr()], [flo[0].data_ptr(), flo[1].data_ptr()],
                                 [flo[2].data_ptr(), flo[3].data_ptr()], [occ[0].data_ptr(), occ[1].data_ptr()],
                                 [occ[2].data_ptr(), occ[3].data_ptr()], nx, ny, **kw)
        ctx.synchronize()
        f = flo.cpu().numpy()
        for g, (a, b) in enumerate([(A[1], B[1]), (A[2], B[2]), (B[1], A[1]), (B[2], A[2])]):
            assert f[g].tobytes() == _lone(ctx, a, b, nx, ny, **kw)[0].tobytes(), g
        # two sequences of three frames: the chained group calls
        F = [_dev(synth.sequence(nx, ny, 3, k), _dtype(mode)) for k in range(2)]
        sflo = torch.full((2, 2, ny, nx, 2), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.tvl1_sequence_group_dev([[t.data_ptr() for t in fr] for fr in F], [[sflo[q, t].data_ptr() for t in range(2)] for q in range(2)],
                                    nx, ny, nscales_first=nscales, nscales_next=2, **PAR)
        ctx.synchronize()
        s = sflo.cpu().numpy()
        prev = None
        for t in range(2):
            want, _ = _group(ctx, [fr[t] for fr in F], [fr[t + 1] for fr in F], nx, ny, init=prev,
                             nscales=2 if t else nscales, **PAR)
            for q in range(2):
                assert s[q, t].tobytes() == want[q].tobytes(), (q, t)
            prev = [want[q] for q in range(2)]
    # ... and the option did reach every one of them
    plain, _ = _group(ctx, A, B, nx, ny, **kw)
    assert plain[1].tobytes() != cold[1].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_option_0_after_option_5_is_the_plain_solve_and_other_values_are_refused(ofx_mod, ctxs, synth, mode):
    nx, ny, nscales, zfactor = W.SHAPES[2]
    ctx = ctxs[mode]
    I0, I1 = synth.pair("P1", nx, ny)
    a, b = _dev([I0, I1], _dtype(mode))
    kw = dict(nscales=nscales, zfactor=zfactor, **PAR)
    before, it_b = _lone(ctx, a, b, nx, ny, **kw)
    ctx.set_option("tvl1_median", 5)
    with5, _ = _lone(ctx, a, b, nx, ny, **kw)
    for bad in (4, 7, -1, 1, 3.5):
        with pytest.raises(ofx_mod.OfxError) as e:
            ctx.set_option("tvl1_median", bad)
        assert e.value.status == ERR_ARG and "tvl1_median" in str(e.value)
    again5, _ = _lone(ctx, a, b, nx, ny, **kw)                       # a refused value stores nothing
    assert again5.tobytes() == with5.tobytes() and with5.tobytes() != before.tobytes()
    ctx.set_option("tvl1_median", 0)
    after, it_a = _lone(ctx, a, b, nx, ny, **kw)
    assert after.tobytes() == before.tobytes() and np.array_equal(it_a, it_b)
