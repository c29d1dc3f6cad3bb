"""ofx_flow_median_dev against the numpy restatement (tests/tvl1_median_ref.py): == plus equal NaN positions, W = 3, 5, 7, with and
without maps, at the smallest shapes where the kernel can go wrong -- 2x2 and 3x3 (every index mirrored), 64x4 and 65x5 (the lane
boundary of a wave, fewer rows than a strip), 129x9 and 67x45 (several strips) --, payloads 8 but not 16 bytes aligned, maps at odd
addresses, guard bytes behind every output, 17 slots, shared inputs, both storage precisions, and every refusal."""
import numpy as np
import pytest

import tvl1_median_ref as M
import tvl1_warm_ref as W

pytestmark = pytest.mark.gpu

ERR_ARG = 1
GUARD = 64                                 # bytes behind every output
FILL = 0xA5
SHAPES = [(2, 2), (3, 3), (64, 4), (65, 5), (129, 9), (67, 45)]
IDS = ["%dx%d" % s for s in SHAPES]


def windows(nx, ny):
    return [w for w in (3, 5, 7) if w // 2 <= min(nx, ny)]


def payloads(nx, ny):
    rng = np.random.default_rng(nx * 1000 + ny)
    noisy = W.smooth_flow(nx, ny).copy()
    noisy[rng.random((ny, nx)) < 0.15] = (40.0, -40.0)                 # outliers, and ties among them
    noisy[rng.random((ny, nx)) < 0.1, 1] = -0.0
    broken = np.ascontiguousarray(W.broken_flow(max(nx, 8), max(ny, 8))[:ny, :nx])        # (broken_flow needs four columns)
    return {"smooth": W.smooth_flow(nx, ny), "edge": W.edge_flow(nx, ny), "broken": broken, "noisy": noisy}


def run(ctx, P, wsize, occ=None, flo_off=0, occ_off=0, n=None):
    """P: list of (ny, nx, 2) float32; occ: None or a list of None | (ny, nx) uint8.  flo_off: bytes (a multiple of 8) by which
    every input and output payload is moved off its 16-byte aligned allocation; occ_off likewise for the maps.
    -> list of outputs; asserts the guard bytes"""
    import torch
    ny, nx = P[0].shape[:2]
    nb = nx * ny * 8
    keep, pin, pocc, pout, outs = [], [], [], [], []
    for g, p in enumerate(P):
        t = torch.zeros(nb + 32, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        t[flo_off:flo_off + nb] = torch.from_numpy(np.frombuffer(np.ascontiguousarray(p).tobytes(), dtype=np.uint8).copy()).cuda()
        keep.append(t)
        pin.append(t.data_ptr() + flo_off)
        o = torch.full((flo_off + nb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        outs.append(o)
        pout.append(o.data_ptr() + flo_off)
        if occ is not None:
            if occ[g] is None:
                pocc.append(None)
            else:
                m = torch.zeros(nx * ny + 16, dtype=torch.uint8, device="cuda")
                m[occ_off:occ_off + nx * ny] = torch.from_numpy(np.ascontiguousarray(occ[g]).ravel()).cuda()
                keep.append(m)
                pocc.append(m.data_ptr() + occ_off)
    torch.cuda.synchronize()
    ctx.flow_median_dev(pin, pout, nx, ny, wsize, d_occ=pocc if occ is not None else None)
    ctx.synchronize()
    res = []
    for o in outs:
        raw = o.cpu().numpy()
        assert (raw[:flo_off] == FILL).all() and (raw[flo_off + nb:] == FILL).all(), "bytes outside the payload were written"
        res.append(np.frombuffer(raw[flo_off:flo_off + nb].tobytes(), dtype=np.float32).reshape(ny, nx, 2))
    return res


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_without_a_map_is_the_restatement(gpu64, shape):
    nx, ny = shape
    for wsize in windows(nx, ny):
        names, P = zip(*payloads(nx, ny).items())
        got = run(gpu64, list(P), wsize)
        for name, p, g in zip(names, P, got):
            assert M.same(g, M.median_payload(p, wsize)), (name, wsize)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_with_maps_is_the_restatement(gpu64, shape):
    nx, ny = shape
    maps = M.maps(nx, ny)
    for wsize in windows(nx, ny):
        for pname in ("broken", "noisy"):
            p = payloads(nx, ny)[pname]
            names = list(maps) + ["none"]
            occ = [maps[k] for k in maps] + [None]                   # a slot without a map among slots with one
            got = dict(zip(names, run(gpu64, [p] * len(names), wsize, occ)))
            for k in maps:
                assert M.same(got[k], M.median_payload(p, wsize, maps[k])), (pname, wsize, k)
            assert M.same(got["none"], M.median_payload(p, wsize)), (pname, wsize)
            assert M.same(got["zero"], got["none"]), (pname, wsize)             # an all-zero map is no map
            assert M.same(got["all"], p), (pname, wsize)                         # all flagged: the input, NaNs included


@pytest.mark.parametrize("shape", [(65, 5), (67, 45)], ids=["65x5", "67x45"])
def test_payloads_8_bytes_off_and_maps_at_odd_addresses(gpu64, shape):
    nx, ny = shape
    p = payloads(nx, ny)["broken"]
    occ = M.maps(nx, ny)["hole"]
    for wsize in windows(nx, ny):
        got = run(gpu64, [p, p], wsize, [occ, None], flo_off=8, occ_off=3)
        assert M.same(got[0], M.median_payload(p, wsize, occ)) and M.same(got[1], M.median_payload(p, wsize)), wsize
        got = run(gpu64, [p], wsize, None, flo_off=8)
        assert M.same(got[0], M.median_payload(p, wsize)), wsize


def test_17_slots_take_two_launches_and_slots_may_share_a_payload(gpu64):
    nx, ny = 67, 45
    base = payloads(nx, ny)
    P = [base["noisy"], base["noisy"]] + [W.smooth_flow(nx, ny, k) for k in range(15)]
    occ = [M.maps(nx, ny)["hole"], None] + [None] * 14 + [M.maps(nx, ny)["column"]]        # the second launch has a map as well
    got = run(gpu64, P, 5, occ)
    assert len(got) == 17
    for g in range(17):
        assert M.same(got[g], M.median_payload(P[g], 5, occ[g])), g
    # one device buffer read by two slots
    import torch
    t = torch.from_numpy(base["broken"]).cuda()
    o = torch.zeros((2, ny, nx, 2), dtype=torch.float32, device="cuda")
    gpu64.flow_median_dev([t.data_ptr()] * 2, [o[0].data_ptr(), o[1].data_ptr()], nx, ny, 3)
    gpu64.synchronize()
    want = M.median_payload(base["broken"], 3)
    assert M.same(o[0].cpu().numpy(), want) and M.same(o[1].cpu().numpy(), want)


def test_f64_and_f32_contexts_write_the_same_bytes_and_host_buffers_are_staged(gpu64, gpu32):
    nx, ny = 129, 9
    p = payloads(nx, ny)["broken"]
    occ = M.maps(nx, ny)["column"]
    for wsize in (3, 5, 7):
        a = run(gpu64, [p, p], wsize, [None, occ])
        b = run(gpu32, [p, p], wsize, [None, occ])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), wsize
    # host memory in, host memory out (the front-end's route)
    src, m = np.ascontiguousarray(p), np.ascontiguousarray(occ)
    dst = np.full((ny * nx * 2 + 4,), -7.0, dtype=np.float32)
    gpu64.flow_median_dev([src.ctypes.data], [dst.ctypes.data], nx, ny, 5, d_occ=[m.ctypes.data])
    gpu64.synchronize()
    assert M.same(dst[:ny * nx * 2].reshape(ny, nx, 2), M.median_payload(p, 5, occ)) and (dst[ny * nx * 2:] == -7.0).all()


def test_refusals_are_invalid_arguments_and_write_nothing(ofx_mod, gpu64):
    import ctypes as C
    import torch
    nx, ny = 9, 7
    src = torch.from_numpy(np.concatenate([W.smooth_flow(nx, ny).ravel(), np.zeros(2, dtype=np.float32)])).cuda()
    dst = torch.full((nx * ny * 2 + 2,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s, d = src.data_ptr(), dst.data_ptr()
    vp = C.c_void_p
    L, h = gpu64.L, gpu64.h
    tab = lambda *xs: (vp * len(xs))(*xs)

    def refused(n, tin, tocc, tout, nx_, ny_, w, word):
        assert L.ofx_flow_median_dev(h, n, tin, tocc, tout, nx_, ny_, w) == ERR_ARG, word
        assert word in L.ofx_last_error(h).decode(), (word, L.ofx_last_error(h))

    refused(1, None, None, tab(d), nx, ny, 3, "NULL")
    refused(1, tab(s), None, None, nx, ny, 3, "NULL")
    refused(1, tab(None), None, tab(d), nx, ny, 3, "NULL")
    refused(2, tab(s, s), None, tab(d, None), nx, ny, 3, "slot 1")
    refused(0, tab(s), None, tab(d), nx, ny, 3, "n = 0")
    refused(-1, tab(s), None, tab(d), nx, ny, 3, "n = -1")
    refused(1, tab(s), None, tab(d), 1, ny, 3, "too small")
    refused(1, tab(s), None, tab(d), nx, 1, 3, "too small")
    refused(1, tab(s), None, tab(d), 65536, 65536, 3, "int")
    for w in (0, 1, 2, 4, 6, 9, -3):
        refused(1, tab(s), None, tab(d), nx, ny, w, "wsize")
    refused(1, tab(s), None, tab(d), nx, 2, 7, "does not fit")       # 7 / 2 = 3 > min(9, 2)
    refused(1, tab(s), None, tab(d), 2, 2, 7, "does not fit")
    refused(1, tab(s + 4), None, tab(d), nx, ny, 3, "8-byte")
    refused(1, tab(s), None, tab(d + 4), nx, ny, 3, "8-byte")
    refused(1, tab(s), None, tab(s), nx, ny, 3, "reads")
    refused(2, tab(s, d), None, tab(d + 8, d), nx, ny, 3, "slot 1")  # the second slot is in place
    gpu64.synchronize()
    assert (dst.cpu().numpy() == -7.0).all()
    # NULL maps and NULL map entries are fine
    assert L.ofx_flow_median_dev(h, 1, tab(s), tab(None), tab(d), nx, ny, 3) == 0
    gpu64.synchronize()
    assert M.same(dst.cpu().numpy()[:nx * ny * 2].reshape(ny, nx, 2), M.median_payload(W.smooth_flow(nx, ny), 3))
