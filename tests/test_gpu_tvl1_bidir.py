"""ofx_tvl1_bidir_group_dev / _batch_dev: TV-L1 in both directions over one shared pyramid, with the consistency maps.

The contract is the project's usual one: the forward payload is BYTES-EQUAL to ofx_tvl1_multiscale_dev(A, B), the backward one to
ofx_tvl1_multiscale_dev(B, A) on the same context, with equal iteration tables, in every mode; the maps equal the restatement
(tests/flow_consistency_ref.py) on the entry's own payloads, and ofx_flow_consistency_dev on them.  In strict f64 the payloads
are the oracle's flows, so there the maps are the ones tests/test_flow_consistency_ref.py pins."""
import numpy as np
import pytest

import flow_consistency_ref as fcr

pytestmark = pytest.mark.gpu

FILL = 0xA5
ERR_ARG = 1


@pytest.fixture(scope="module")
def ctxs(ofx_mod):
    """contexts of this module alone (their options must not leak into the session's)"""
    c = {"f64": [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)], "f32": [ofx_mod.Ofx(0, ofx_mod.F32)],
         "relaxed": [ofx_mod.Ofx(0, ofx_mod.F64)]}
    c["relaxed"][0].set_option("relaxed_dual", 1)
    yield c
    for v in c.values():
        for x in v:
            x.close()


def _dtype(mode):
    import torch
    return torch.float32 if mode == "f32" else torch.float64


def _pairs(synth, spec, nx, ny):
    """spec: a list of (pair name, k) -> [(A, B), ..] as numpy planes"""
    return [synth.pair(name, nx, ny, k) for name, k in spec]


def _lone(ctx, a, b, nx, ny, **kw):
    """ofx_tvl1_multiscale_dev on device tensors (or pointers) -> (payload (ny, nx, 2) float32, iteration table)"""
    import torch
    flo = torch.full((ny, nx, 2), np.nan, dtype=torch.float32, device="cuda")
    ptr = lambda t: t if isinstance(t, int) else t.data_ptr()
    ctx.tvl1_multiscale_dev(ptr(a), ptr(b), flo.data_ptr(), nx, ny, **kw)
    ctx.synchronize()
    return flo.cpu().numpy(), ctx.stats().iterations().copy()


def _bidir(ctx, A, B, nx, ny, **kw):
    """the group entry on lists of device tensors (or pointers) -> (fwd payloads, bwd payloads, fwd maps, bwd maps, records)"""
    import torch
    G = len(A)
    flo = torch.full((2, G, ny, nx, 2), np.nan, dtype=torch.float32, device="cuda")
    occ = torch.full((2, G, ny, nx), FILL, dtype=torch.uint8, device="cuda")
    ptr = lambda t: t if isinstance(t, int) else t.data_ptr()
    st = ctx.tvl1_bidir_group_dev([ptr(t) for t in A], [ptr(t) for t in B], [flo[0, g].data_ptr() for g in range(G)],
                                  [flo[1, g].data_ptr() for g in range(G)], [occ[0, g].data_ptr() for g in range(G)],
                                  [occ[1, g].data_ptr() for g in range(G)], nx, ny, **kw)
    ctx.synchronize()
    assert len(st) == 2 * G
    f, o = flo.cpu().numpy(), occ.cpu().numpy()
    return f[0], f[1], o[0], o[1], st


def _consistency(ctx, fwd, bwd):
    """ofx_flow_consistency_dev on downloaded payloads (G, ny, nx, 2) -> (fwd maps, bwd maps)"""
    import torch
    G, ny, nx, _ = fwd.shape
    f, b = torch.from_numpy(fwd).cuda(), torch.from_numpy(bwd).cuda()
    occ = torch.full((2, G, ny, nx), FILL, dtype=torch.uint8, device="cuda")
    ctx.flow_consistency_dev([f[g].data_ptr() for g in range(G)], [b[g].data_ptr() for g in range(G)],
                             [occ[0, g].data_ptr() for g in range(G)], [occ[1, g].data_ptr() for g in range(G)], nx, ny)
    ctx.synchronize()
    o = occ.cpu().numpy()
    return o[0], o[1]


def _check_group(ctx, orc, A, B, nx, ny, lone_of=None, **kw):
    """the whole contract for one group.  A, B: lists of device tensors; lone_of(g) -> the (a, b) arguments of the lone solves of
    pair g (default: the tensors themselves)"""
    G = len(A)
    fwd, bwd, of, ob, st = _bidir(ctx, A, B, nx, ny, **kw)
    assert np.isfinite(fwd).all() and np.isfinite(bwd).all()
    for g in range(G):
        a, b = lone_of(g) if lone_of else (A[g], B[g])
        pf, itf = _lone(ctx, a, b, nx, ny, **kw)
        pb, itb = _lone(ctx, b, a, nx, ny, **kw)
        assert fwd[g].tobytes() == pf.tobytes(), ("forward payload", g)
        assert bwd[g].tobytes() == pb.tobytes(), ("backward payload", g)
        assert np.array_equal(st[g].iterations(), itf), ("forward iterations", g)
        assert np.array_equal(st[G + g].iterations(), itb), ("backward iterations", g)
    cf, cb = _consistency(ctx, fwd, bwd)
    assert np.array_equal(of, cf) and np.array_equal(ob, cb)
    for g in sorted({0, G - 1}):                        # the restatement on the entry's own payloads (the ends of a group)
        rf, rb, _ = fcr.maps(orc, fwd[g], bwd[g])
        assert np.array_equal(of[g], rf) and np.array_equal(ob[g], rb), g
        share = float((of[g] == 255).mean())
        assert 0.0 < share < 1.0, share
    return fwd, bwd, of, ob, st


def _dev(planes, dtype):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p)).to("cuda", dtype) for p in planes]


CASES = {
    "p1_64x48_g1": ([("P1", 0)], 64, 48, 3),
    "p0_64x48_g1": ([("P0", 0)], 64, 48, 3),
    "mix_37x29_g3": ([("P1", 0), ("P0", 0), ("P1", 2)], 37, 29, 2),
    "p1_64x48_g8": ([("P1", k) for k in range(8)], 64, 48, 3),
    "p1_160x120_g1": ([("P1", 1)], 160, 120, 4),
}


@pytest.mark.parametrize("mode", ["f64", "relaxed", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_payloads_and_maps(ctxs, orc, synth, case, mode):
    spec, nx, ny, nscales = CASES[case]
    pairs = _pairs(synth, spec, nx, ny)
    A, B = _dev([p[0] for p in pairs], _dtype(mode)), _dev([p[1] for p in pairs], _dtype(mode))
    _check_group(ctxs[mode][0], orc, A, B, nx, ny, nscales=nscales)


def test_u8_frames_with_a_row_pitch(ofx_mod, ctxs, orc, synth):
    """option "input" = OFX_IN_U8 with a padded "input_pitch": regions of interest of poisoned parents, 3 pairs"""
    import torch
    nx, ny, pitch = 37, 29, 48
    ctx = ctxs["f64"][0]
    pairs = _pairs(synth, [("P1", 0), ("P1", 1), ("P0", 0)], nx, ny)
    parents = []
    for p in pairs:
        for plane in p:
            assert plane.min() >= 0 and plane.max() <= 255
            host = np.full((ny, pitch), 255, dtype=np.uint8)
            host[:, 1::2] = 0
            host[:, 3:3 + nx] = plane.astype(np.uint8)
            parents.append(torch.from_numpy(host).cuda())
    ptrs = [t.data_ptr() + 3 for t in parents]
    ctx.set_option("input", ofx_mod.IN_U8)
    ctx.set_option("input_pitch", pitch)
    try:
        _check_group(ctx, orc, ptrs[0::2], ptrs[1::2], nx, ny, nscales=2)
    finally:
        ctx.set_option("input_pitch", 0)
        ctx.set_option("input", ofx_mod.IN_STORAGE)


def test_two_pass_gaussians(ctxs, orc, synth):
    """option "gauss_fused" = 0: the pyramid head's other schedule over the shared planes"""
    import torch
    nx, ny = 64, 48
    ctx = ctxs["f64"][0]
    pairs = _pairs(synth, [("P1", 0), ("P1", 3)], nx, ny)
    A, B = _dev([p[0] for p in pairs], torch.float64), _dev([p[1] for p in pairs], torch.float64)
    ctx.set_option("gauss_fused", 0)
    try:
        _check_group(ctx, orc, A, B, nx, ny, nscales=3)
    finally:
        ctx.set_option("gauss_fused", 1)


def test_strict_f64_against_the_oracle(ctxs, orc, synth):
    """the end-to-end statement: both payloads are the oracle's flows (max abs difference 0.0), both maps the pinned ones"""
    import torch
    nx, ny = 64, 48
    I0, I1 = synth.pair("P1", nx, ny)
    A, B = _dev([I0], torch.float64), _dev([I1], torch.float64)
    fwd, bwd, of, ob, st = _bidir(ctxs["f64"][0], A, B, nx, ny, nscales=3)
    want_f, want_b = fcr.tvl1_payloads(orc, synth, "p1_64x48")
    df, db = float(np.abs(fwd[0] - want_f).max()), float(np.abs(bwd[0] - want_b).max())
    print("max abs difference to the oracle: forward %g, backward %g" % (df, db))
    assert df == 0.0 and db == 0.0
    it_f = orc.tvl1_multiscale(I0, I1, nscales=3)[2]
    it_b = orc.tvl1_multiscale(I1, I0, nscales=3)[2]
    assert np.array_equal(st[0].iterations(), it_f) and np.array_equal(st[1].iterations(), it_b)
    pin_f, pin_b, _ = fcr.case_maps(orc, synth, "p1_64x48")
    assert np.array_equal(of[0], pin_f) and np.array_equal(ob[0], pin_b)


def test_batch_equals_groups_and_stages_host_buffers(ofx_mod, ctxs, synth):
    """5 pairs over 2 contexts with lockstep = 4 slots: groups of 2, 2 and 1 pairs; pair 3's payload and map arrays are pinned
    host memory (staged).  Everything equals the group entry pair for pair."""
    import torch
    nx, ny, n_pairs = 64, 48, 5
    two = ctxs["f64"]
    pairs = _pairs(synth, [("P1", k) for k in range(n_pairs)], nx, ny)
    A, B = _dev([p[0] for p in pairs], torch.float64), _dev([p[1] for p in pairs], torch.float64)
    want_f, want_b, want_of, want_ob, want_st = _bidir(two[0], A, B, nx, ny, nscales=3)

    flo = torch.full((2, n_pairs, ny, nx, 2), np.nan, dtype=torch.float32, device="cuda")
    occ = torch.full((2, n_pairs, ny, nx), FILL, dtype=torch.uint8, device="cuda")
    hflo = torch.full((2, ny, nx, 2), np.nan, dtype=torch.float32).pin_memory()
    hocc = torch.full((2, ny, nx), FILL, dtype=torch.uint8).pin_memory()
    H = 3
    tab = lambda dev, host, d: [host[d].data_ptr() if g == H else dev[d, g].data_ptr() for g in range(n_pairs)]
    for c in two:
        c.set_option("lockstep", 4)
    try:
        work = ofx_mod.tvl1_bidir_batch_dev(two, [t.data_ptr() for t in A], [t.data_ptr() for t in B], tab(flo, hflo, 0), tab(flo, hflo, 1),
                                            tab(occ, hocc, 0), tab(occ, hocc, 1), nx, ny, nscales=3)
    finally:
        for c in two:
            c.set_option("lockstep", 0)
    torch.cuda.synchronize()
    f, o = flo.cpu().numpy(), occ.cpu().numpy()
    f[:, H], o[:, H] = hflo.numpy(), hocc.numpy()
    assert f[0].tobytes() == want_f.tobytes() and f[1].tobytes() == want_b.tobytes()
    assert np.array_equal(o[0], want_of) and np.array_equal(o[1], want_ob)
    assert len(work) == 2 * n_pairs
    assert work == [s.work_pix_iters for s in want_st]              # forward first, then backward
    assert 0.0 < float((o[0] == 255).mean()) < 1.0


def test_refusals_write_nothing(ofx_mod, ctxs, synth):
    import torch
    nx, ny = 37, 29
    ctx = ctxs["f64"][0]
    I0, I1 = synth.pair("P1", nx, ny)
    a, b = _dev([I0], torch.float64)[0], _dev([I1], torch.float64)[0]
    flo = torch.full((2, 9, ny, nx, 2), 7.0, dtype=torch.float32, device="cuda")
    occ = torch.full((2, 9, ny, nx), FILL, dtype=torch.uint8, device="cuda")

    def call(n, null=None, **kw):
        t = [[a.data_ptr()] * n, [b.data_ptr()] * n, [flo[0, g].data_ptr() for g in range(n)], [flo[1, g].data_ptr() for g in range(n)],
             [occ[0, g].data_ptr() for g in range(n)], [occ[1, g].data_ptr() for g in range(n)]]
        if null is not None:
            t[null][n - 1] = None
        with pytest.raises(ofx_mod.OfxError) as e:
            ctx.tvl1_bidir_group_dev(*t, nx, ny, nscales=2, **kw)
        ctx.synchronize()
        assert e.value.status == ERR_ARG
        assert ctx.L.ofx_last_error(ctx.h), "ofx_last_error is empty"
        assert (flo.cpu().numpy() == 7.0).all() and (occ.cpu().numpy() == FILL).all()
        return str(e.value)

    call(0)
    assert "1..8" in call(9)                                        # the limit is named
    for k in range(6):
        call(2, null=k)
    call(1, fb_beta=-0.5)
    call(1, fb_alpha=float("nan"))
    # and the same call without a fault goes through
    ctx.tvl1_bidir_group_dev([a.data_ptr()], [b.data_ptr()], [flo[0, 0].data_ptr()], [flo[1, 0].data_ptr()], [occ[0, 0].data_ptr()],
                             [occ[1, 0].data_ptr()], nx, ny, nscales=2)
    ctx.synchronize()
    assert not (flo[:, 0].cpu().numpy() == 7.0).all()
