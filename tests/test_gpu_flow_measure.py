"""ofx_flow_error_dev, ofx_flow_encode_dev and ofx_flow_decode_dev against the numpy restatement (tests/flow_measure_ref.py): records,
EPE maps, histograms and the BOUND and KITTI codings bit for bit, the two angular entries of the record at 1e-12 relative, the wheel
under the three-way rule -- at 2x2, 3x5, 64x2, 65x3 (one element in a second lane round), 63x65 and 130x131 (rows and row sums both
beyond 64 and 128); 1, 3, 16 and 17 slots (two launches); maps at byte offsets 0, 1 and 3, payloads 8 but not 16 bytes aligned, RGB
and 2-byte destinations at offsets 0, 1 and 3; guard bytes around every destination; NaN, Inf and 1e10 vectors in estimate and truth;
all-flagged and all-bad slots beside healthy ones; 0 and 8 thresholds; 1, 4096 and 5000 bins (the histogram counted in LDS and in
memory); both storage precisions; host buffers; every refusal.

The two angular entries [4] and [7] hold sums of acos values of two libraries on bit-equal arguments: each acos is within a few ulp
(<= 2^-50 relative), all terms are >= 0 and at most 17 030 of them are added in one fixed order, so the sums differ by about 1e-15
relative at most; 1e-12 leaves a margin of about 1000."""
import numpy as np
import pytest

import flow_measure_ref as R
from test_gpu_flow_motion import Dev, sync

pytestmark = pytest.mark.gpu

ERR_ARG = 1
SIZES = [(2, 2), (3, 5), (64, 2), (65, 3), (63, 65), (130, 131)]
EXACT = [0, 1, 2, 3, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15]
THR8_ABS = R.THR_ABS + (0.0, 0.25)
THR8_REL = R.THR_REL + (0.0, 0.5)
_want = {}
worst_angular = [0.0]


def none_if_empty(xs):
    return xs if any(x is not None for x in xs) else None


def run_error(ctx, slots, thr_abs=(), thr_rel=(), n_bins=0, bin_w=0.0, flo_off=0, occ_off=0, epe=True):
    """slots: list of (estimate, truth, map | None) -> list of dicts rec, epe, hist (None: not asked for)"""
    ny, nx, _ = slots[0][0].shape
    d = Dev()
    tab = {k: [] for k in ("flo", "gt", "occ", "rec", "epe", "hist")}
    handles = []
    for flo, gt, occ in slots:
        h = {}
        tab["flo"].append(d.put(flo, flo_off))
        tab["gt"].append(d.put(gt, flo_off))
        tab["occ"].append(d.put(occ, occ_off))
        p, h["rec"] = d.out(128, 8)
        tab["rec"].append(p)
        p, h["epe"] = d.out(nx * ny * 4, 4) if epe else (None, None)
        tab["epe"].append(p)
        p, h["hist"] = d.out(n_bins * 4, 4) if n_bins else (None, None)
        tab["hist"].append(p)
        handles.append(h)
    sync()
    ctx.flow_error_dev(tab["flo"], tab["gt"], tab["rec"], nx, ny, thr_abs=thr_abs, thr_rel=thr_rel, d_occ=none_if_empty(tab["occ"]),
                       d_epe=none_if_empty(tab["epe"]), d_hist=none_if_empty(tab["hist"]), n_bins=n_bins, bin_w=bin_w)
    ctx.synchronize()
    kinds = {"rec": (np.float64, (16,)), "epe": (np.float32, (ny, nx)), "hist": (np.uint32, (n_bins,))}
    return [{k: None if h[k] is None else d.get(h[k], *kinds[k]) for k in kinds} for h in handles]


def want_error(slot, thr_abs, thr_rel, n_bins, bin_w, key=None):
    k = None if key is None else (key, thr_abs, thr_rel, n_bins, bin_w)
    if k is None or k not in _want:
        rec, epe, hist = R.error(slot[0], slot[1], slot[2], thr_abs, thr_rel, n_bins, bin_w)
        got = dict(rec=rec, epe=epe, hist=hist)
        if k is None:
            return got
        _want[k] = got
    return _want[k]


def same_error(got, exp, what=""):
    assert got["rec"][EXACT].tobytes() == exp["rec"][EXACT].tobytes(), (what, got["rec"], exp["rec"])
    for k in (4, 7):
        a, b = got["rec"][k], exp["rec"][k]
        dev = abs(a - b) / b if b != 0 else abs(a)
        worst_angular[0] = max(worst_angular[0], dev)
        assert dev <= 1e-12, (what, k, a, b)
    if got["epe"] is not None:
        assert got["epe"].tobytes() == exp["epe"].tobytes(), (what, "epe")
    if got["hist"] is not None:
        assert got["hist"].tobytes() == exp["hist"].tobytes(), (what, "hist")


def error_slots(nx, ny):
    """a plain slot, one with a map, one with a map and NaN / Inf / 1e10 vectors in estimate and truth"""
    gt, flo = R.truth(nx, ny), R.estimate(nx, ny)
    return [(flo, gt, None), (flo, gt, R.flags(nx, ny)), (R.spoiled(flo, 1), R.spoiled(gt, 2), R.flags(nx, ny, 1))]


@pytest.mark.parametrize("nx,ny", SIZES)
def test_error_is_the_restatement(gpu64, nx, ny):
    slots = error_slots(nx, ny)
    exp = [want_error(s, THR8_ABS, THR8_REL, 4096, 1.0 / 64, key=(nx, ny, g)) for g, s in enumerate(slots)]
    for flo_off, occ_off in ((0, 0), (8, 1), (0, 3)):
        got = run_error(gpu64, slots, THR8_ABS, THR8_REL, 4096, 1.0 / 64, flo_off, occ_off)
        for g in range(len(slots)):
            same_error(got[g], exp[g], (flo_off, occ_off, g))
    # the records alone, without thresholds; one bin; more bins than LDS holds
    got = run_error(gpu64, slots, epe=False)
    for g in range(len(slots)):
        assert got[g]["epe"] is None and got[g]["hist"] is None and not got[g]["rec"][8:].any()
        same_error(got[g], want_error(slots[g], (), (), 0, 0.0, key=(nx, ny, g)), g)
    for n_bins, bin_w in ((1, 0.5), (5000, 1.0 / 256)):
        got = run_error(gpu64, slots, (3.0,), (0.05,), n_bins, bin_w, epe=False)
        for g in range(len(slots)):
            same_error(got[g], want_error(slots[g], (3.0,), (0.05,), n_bins, bin_w, key=(nx, ny, g)), (n_bins, g))
    print("largest relative deviation of the angular entries so far: %.3g" % worst_angular[0])


def error_pool(nx, ny):
    gt, flo = R.truth(nx, ny), R.estimate(nx, ny)
    return [(flo, gt, None),                                                          # healthy
            (flo, gt, np.full((ny, nx), 7, dtype=np.uint8)),                          # all flagged: a record of zeros
            (flo, gt, R.flags(nx, ny)),                                               # healthy, with a map
            (np.full_like(flo, np.nan), gt, None),                                    # all bad
            (flo, np.full_like(gt, 1e10), None),                                      # no truth at all
            (R.spoiled(flo, 3), R.spoiled(gt, 4), R.flags(nx, ny, 2)),
            (gt, gt, None)]                                                           # a perfect estimate: zeros, all in bin 0


@pytest.mark.parametrize("n", [1, 3, 16, 17])
def test_any_number_of_slots_and_degenerate_slots_beside_healthy_ones(gpu64, n):
    nx, ny = 37, 29
    pool = error_pool(nx, ny)
    pick = [(3 * g + 2) % len(pool) for g in range(n)]
    got = run_error(gpu64, [pool[k] for k in pick], R.THR_ABS, R.THR_REL, 64, 0.25, occ_off=1)
    assert len(got) == n
    for g in range(n):
        same_error(got[g], want_error(pool[pick[g]], R.THR_ABS, R.THR_REL, 64, 0.25, key=("pool", pick[g])), g)
    if n >= 16:
        by = {pick[g]: got[g] for g in range(n)}
        assert not by[1]["rec"].any() and not by[1]["hist"].any() and np.isnan(by[1]["epe"]).all()
        assert by[3]["rec"][0] == by[3]["rec"][1] == by[3]["rec"][8] == nx * ny and by[3]["hist"][-1] == nx * ny
        assert not by[4]["rec"].any()
        # a perfect estimate: every end-point entry is zero (the angular ones hold the rounding of num / den, a few 1e-7 degrees)
        assert by[6]["rec"][0] == nx * ny and not by[6]["rec"][[1, 2, 3, 5, 6]].any() and not by[6]["rec"][8:].any()
        assert by[6]["rec"][4] < 1e-5 and by[6]["hist"][0] == nx * ny


def test_mixed_null_entries_of_the_optional_tables(gpu64):
    nx, ny = 130, 70
    slots = error_slots(nx, ny)
    d = Dev()
    flo, gt = [d.put(s[0]) for s in slots], [d.put(s[1]) for s in slots]
    recs = [d.out(128) for _ in slots]
    o_epe, o_hist = d.out(nx * ny * 4), d.out(64 * 4)
    sync()
    gpu64.flow_error_dev(flo, gt, [r[0] for r in recs], nx, ny, thr_abs=(1.0,), thr_rel=(0.0,), d_occ=[None, d.put(slots[1][2], 3), None],
                         d_epe=[None, o_epe[0], None], d_hist=[None, None, o_hist[0]], n_bins=64, bin_w=0.25)
    gpu64.synchronize()
    noocc = (slots[2][0], slots[2][1], None)
    exp = [want_error(s, (1.0,), (0.0,), 64, 0.25) for s in (slots[0], slots[1], noocc)]
    for g in range(3):
        same_error(dict(rec=d.get(recs[g][1], np.float64, (16,)), epe=None, hist=None), exp[g], g)
    assert d.get(o_epe[1], np.float32, (ny, nx)).tobytes() == exp[1]["epe"].tobytes()
    assert d.get(o_hist[1], np.uint32, (64,)).tobytes() == exp[2]["hist"].tobytes()


# ---- the encodings ----------------------------------------------------------------------------------------------------------------
def run_encode(ctx, slots, kind, scale, flo_off=0, occ_off=0, dst_off=0):
    """slots: list of (payload, map | None) -> list of coded images"""
    ny, nx, _ = slots[0][0].shape
    per, dtype = {R.WHEEL_RGB8: (3, np.uint8), R.BOUND_U8: (2, np.uint8), R.KITTI_U16: (3, np.uint16)}[kind]
    d = Dev()
    tab = {k: [] for k in ("flo", "occ", "dst")}
    handles = []
    for flo, occ in slots:
        tab["flo"].append(d.put(flo, flo_off))
        tab["occ"].append(d.put(occ, occ_off))
        p, h = d.out(nx * ny * per * np.dtype(dtype).itemsize, dst_off)
        tab["dst"].append(p)
        handles.append(h)
    sync()
    ctx.flow_encode_dev(tab["flo"], tab["dst"], nx, ny, kind=kind, scale=scale, d_occ=none_if_empty(tab["occ"]))
    ctx.synchronize()
    return [d.get(h, dtype, (ny, nx, per)) for h in handles]


def run_decode(ctx, codes, kind, scale, src_off=0, occ_off=0, maps=True):
    ny, nx, _ = codes[0].shape
    d = Dev()
    src, flo, occ = [], [], []
    for c in codes:
        src.append(d.put(c, src_off))
        flo.append(d.out(nx * ny * 8, 8))
        occ.append(d.out(nx * ny, occ_off) if maps else (None, None))
    sync()
    ctx.flow_decode_dev(src, [f[0] for f in flo], nx, ny, kind=kind, scale=scale, d_occ=[o[0] for o in occ] if maps else None)
    ctx.synchronize()
    return [(d.get(f[1], np.float32, (ny, nx, 2)), d.get(o[1], np.uint8, (ny, nx)) if maps else None) for f, o in zip(flo, occ)]


def code_slots(nx, ny):
    """a plain slot, one with a map, one with a map and NaN / Inf / 1e10 vectors, one that is all zero"""
    flo = R.truth(nx, ny)
    return [(flo, None), (flo, R.flags(nx, ny)), (R.spoiled(flo, 5), R.flags(nx, ny, 1)), (np.zeros_like(flo), None)]


def same_wheel(got, slot, scale, what=""):
    ok, exempt = R.wheel_ok(got, slot[0], slot[1], scale)
    assert ok, what
    return exempt


@pytest.mark.parametrize("nx,ny", SIZES)
def test_encodings_are_the_restatement(gpu64, nx, ny):
    slots = code_slots(nx, ny)
    for flo_off, occ_off, dst_off in ((0, 0, 0), (8, 1, 1), (0, 3, 3)):
        for scale in (0.0, 4.0):
            got = run_encode(gpu64, slots, R.WHEEL_RGB8, scale, flo_off, occ_off, dst_off)
            for g, s in enumerate(slots):
                exempt = same_wheel(got[g], s, scale, (scale, dst_off, g))
                assert g >= 2 or exempt <= 0.01 * nx * ny, (scale, g, exempt)       # slots 0 and 1 are the field image
        got = run_encode(gpu64, slots, R.BOUND_U8, 8.0, flo_off, occ_off, dst_off)
        for g, s in enumerate(slots):
            assert got[g].tobytes() == R.encode_bound(s[0], s[1], 8.0).tobytes(), (dst_off, g)
        got = run_encode(gpu64, slots, R.KITTI_U16, 0.0, flo_off, occ_off, 2 * (dst_off % 2) + 2 * (dst_off // 3))
        for g, s in enumerate(slots):
            assert got[g].tobytes() == R.encode_kitti(s[0], s[1]).tobytes(), (dst_off, g)
    # ... and back
    codes = [R.encode_bound(s[0], s[1], 8.0) for s in slots]
    for src_off, occ_off in ((0, 0), (1, 1), (3, 3)):
        for (flo, m), c in zip(run_decode(gpu64, codes, R.BOUND_U8, 8.0, src_off, occ_off), codes):
            wf, wm = R.decode_bound(c, 8.0)
            assert flo.tobytes() == wf.tobytes() and m.tobytes() == wm.tobytes(), src_off
    codes = [R.encode_kitti(s[0], s[1]) for s in slots]
    for src_off, occ_off, maps in ((0, 0, True), (2, 1, True), (6, 3, False)):
        for (flo, m), c in zip(run_decode(gpu64, codes, R.KITTI_U16, 0.0, src_off, occ_off, maps), codes):
            wf, wm = R.decode_kitti(c)
            assert flo.tobytes() == wf.tobytes() and (m is None or m.tobytes() == wm.tobytes()), src_off


def test_the_known_values_of_the_wheel_on_the_device(gpu64):
    from test_flow_measure_ref import KNOWN
    flo = np.array([[k[0] for k in KNOWN], [k[0] for k in KNOWN[::-1]]], dtype=np.float32)
    got = run_encode(gpu64, [(flo, None)], R.WHEEL_RGB8, 4.0, dst_off=1)[0]
    same_wheel(got, (flo, None), 4.0)
    # the vectors off the axes are no boundary of the wheel: their bytes are the table's
    for k in (5, 6, 7):
        assert got[0, k].tolist() == list(KNOWN[k][1]), k
    assert got[0, 0].tolist() == [255, 255, 255]


@pytest.mark.parametrize("n", [1, 3, 16, 17])
def test_any_number_of_slots_through_the_encodings(gpu64, n):
    nx, ny = 37, 29
    pool = code_slots(nx, ny) + [(R.estimate(nx, ny), np.full((ny, nx), 9, dtype=np.uint8)), (R.estimate(nx, ny), None)]
    pick = [(5 * g + 1) % len(pool) for g in range(n)]
    slots = [pool[k] for k in pick]
    got = run_encode(gpu64, slots, R.WHEEL_RGB8, 0.0, occ_off=1, dst_off=1)         # every slot its own maximum
    for g in range(n):
        same_wheel(got[g], slots[g], 0.0, g)
    if n >= 16:
        by = {pick[g]: got[g] for g in range(n)}
        assert not by[4].any() and (by[3] == 255).all()                               # all flagged: black; all zero: white
    kitti = run_encode(gpu64, slots, R.KITTI_U16, 0.0, occ_off=3)
    bound = run_encode(gpu64, slots, R.BOUND_U8, 20.0, dst_off=3)
    for g in range(n):
        assert kitti[g].tobytes() == R.encode_kitti(*slots[g]).tobytes() and bound[g].tobytes() == R.encode_bound(*slots[g], 20.0).tobytes(), g
    back = run_decode(gpu64, kitti, R.KITTI_U16, 0.0)
    for g in range(n):
        wf, wm = R.decode_kitti(kitti[g])
        assert back[g][0].tobytes() == wf.tobytes() and back[g][1].tobytes() == wm.tobytes(), g


def test_f64_and_f32_contexts_write_the_same_bytes_and_host_buffers_are_staged(gpu64, gpu32):
    nx, ny = 67, 35
    slots = error_slots(nx, ny)
    a = run_error(gpu64, slots, THR8_ABS, THR8_REL, 4096, 1.0 / 64, occ_off=1)
    b = run_error(gpu32, slots, THR8_ABS, THR8_REL, 4096, 1.0 / 64, occ_off=1)
    exp = [want_error(s, THR8_ABS, THR8_REL, 4096, 1.0 / 64) for s in slots]
    for g in range(len(slots)):
        same_error(a[g], exp[g], g)
        for k in ("rec", "epe", "hist"):
            assert a[g][k].tobytes() == b[g][k].tobytes(), (g, k)
    cs = code_slots(nx, ny)
    for kind, scale in ((R.WHEEL_RGB8, 0.0), (R.WHEEL_RGB8, 4.0), (R.BOUND_U8, 8.0), (R.KITTI_U16, 0.0)):
        x, y = run_encode(gpu64, cs, kind, scale, occ_off=1, dst_off=0), run_encode(gpu32, cs, kind, scale, occ_off=1, dst_off=0)
        for g in range(len(cs)):
            assert x[g].tobytes() == y[g].tobytes(), (kind, g)
    # host memory in, host memory out (the front-ends' route)
    n = len(slots)
    flo, gt = [np.array(s[0]) for s in slots], [np.array(s[1]) for s in slots]
    occ = [None if s[2] is None else np.array(s[2]) for s in slots]
    rec = np.full((n, 18), -7.0)
    epe = np.full((n, ny * nx + 4), -7.0, dtype=np.float32)
    hist = np.full((n, 4096 + 4), 9, dtype=np.uint32)
    ptr = lambda xs: [None if x is None else x.ctypes.data for x in xs]
    gpu64.flow_error_dev(ptr(flo), ptr(gt), [rec[g].ctypes.data for g in range(n)], nx, ny, thr_abs=THR8_ABS, thr_rel=THR8_REL,
                         d_occ=ptr(occ), d_epe=[epe[g].ctypes.data for g in range(n)], d_hist=[hist[g].ctypes.data for g in range(n)],
                         n_bins=4096, bin_w=1.0 / 64)
    gpu64.synchronize()
    for g in range(n):
        assert rec[g][:16].tobytes() == a[g]["rec"].tobytes() and (rec[g][16:] == -7.0).all(), g
        assert epe[g][:ny * nx].tobytes() == exp[g]["epe"].tobytes() and (epe[g][ny * nx:] == -7.0).all(), g
        assert hist[g][:4096].tobytes() == exp[g]["hist"].tobytes() and (hist[g][4096:] == 9).all(), g
    rgb = np.full((nx * ny * 3 + 5,), 7, dtype=np.uint8)
    k16 = np.full((nx * ny * 3 + 5,), 7, dtype=np.uint16)
    s = cs[2]
    f, m = np.array(s[0]), np.array(s[1])
    gpu64.flow_encode_dev([f.ctypes.data], [rgb[1:].ctypes.data], nx, ny, kind=R.WHEEL_RGB8, scale=0.0, d_occ=[m.ctypes.data])
    gpu64.flow_encode_dev([f.ctypes.data], [k16[1:].ctypes.data], nx, ny, kind=R.KITTI_U16, d_occ=[m.ctypes.data])
    gpu64.synchronize()
    assert rgb[0] == 7 and (rgb[1 + nx * ny * 3:] == 7).all() and k16[0] == 7 and (k16[1 + nx * ny * 3:] == 7).all()
    same_wheel(rgb[1:1 + nx * ny * 3].reshape(ny, nx, 3), s, 0.0)
    assert k16[1:1 + nx * ny * 3].tobytes() == R.encode_kitti(f, m).tobytes()
    back = np.full((nx * ny * 2 + 4,), -7.0, dtype=np.float32)
    bmap = np.full((nx * ny + 4,), 9, dtype=np.uint8)
    code = np.ascontiguousarray(k16[1:1 + nx * ny * 3])
    gpu64.flow_decode_dev([code.ctypes.data], [back.ctypes.data], nx, ny, kind=R.KITTI_U16, d_occ=[bmap.ctypes.data])
    gpu64.synchronize()
    wf, wm = R.decode_kitti(code.reshape(ny, nx, 3))
    assert back[:nx * ny * 2].tobytes() == wf.tobytes() and (back[nx * ny * 2:] == -7.0).all()
    assert bmap[:nx * ny].tobytes() == wm.tobytes() and (bmap[nx * ny:] == 9).all()


def test_refusals_are_invalid_arguments_and_write_nothing(gpu64):
    import ctypes as C
    import torch
    nx, ny = 9, 7
    n = nx * ny
    rng = np.random.default_rng(3)
    src = torch.from_numpy(rng.normal(0.0, 1.0, (4, n * 2 + 2)).astype(np.float32)).cuda()
    before = src.cpu().numpy().copy()
    dst = torch.full((4, n * 2 + 2), -7.0, dtype=torch.float32, device="cuda")           # n * 8 bytes each: room for every output
    imap = torch.zeros((n + 8,), dtype=torch.uint8, device="cuda")
    recs = torch.full((3, 18), -7.0, dtype=torch.float64, device="cuda")
    sync()
    s = [src[k].data_ptr() for k in range(4)]
    d = [dst[k].data_ptr() for k in range(4)]
    r = [recs[k].data_ptr() for k in range(3)]
    m = imap.data_ptr()
    vp, dbl = C.c_void_p, C.c_double
    L, h = gpu64.L, gpu64.h
    tab = lambda *xs: (vp * len(xs))(*xs)
    thr = lambda *xs: (dbl * max(len(xs), 1))(*xs)
    nan, inf = float("nan"), float("inf")

    def refused(status, word):
        assert status == ERR_ARG, word
        assert word in L.ofx_last_error(h).decode(), (word, L.ofx_last_error(h))

    def err(n_=1, flo=tab(s[0]), gt=tab(s[1]), occ=None, n_thr=1, ta=thr(1.0), tr=thr(0.0), rec=tab(r[0]), epe=None, hist=None, n_bins=16,
            bin_w=0.5, nx_=nx, ny_=ny):
        return L.ofx_flow_error_dev(h, n_, flo, gt, occ, n_thr, ta, tr, rec, epe, hist, n_bins, bin_w, nx_, ny_)

    refused(err(flo=None), "NULL")
    refused(err(gt=None), "NULL")
    refused(err(rec=None), "NULL")
    refused(err(flo=tab(None)), "NULL")
    refused(err(gt=tab(None)), "NULL")
    refused(err(n_=2, flo=tab(s[0], s[2]), gt=tab(s[1], s[3]), rec=tab(r[0], None)), "slot 1")
    refused(err(n_=0), "n = 0")
    refused(err(n_=-1), "n = -1")
    refused(err(nx_=1), "too small")
    refused(err(ny_=1), "too small")
    refused(err(nx_=65536, ny_=65536), "int")
    refused(err(n_thr=-1), "n_thr = -1")
    refused(err(n_thr=9), "n_thr = 9")
    refused(err(ta=None), "threshold")
    refused(err(tr=None), "threshold")
    for bad in (-1.0, nan, inf):
        refused(err(ta=thr(bad)), "threshold 0")
        refused(err(n_thr=2, ta=thr(1.0, 2.0), tr=thr(0.0, bad)), "threshold 1")
    for bad in (0, -1, 65537):
        refused(err(hist=tab(d[1]), n_bins=bad), "n_bins = %d" % bad)
    for bad in (0.0, -1.0, nan, inf):
        refused(err(hist=tab(d[1]), bin_w=bad), "bin_w")
    refused(err(flo=tab(s[0] + 4)), "8-byte")
    refused(err(gt=tab(s[1] + 4)), "8-byte")
    refused(err(rec=tab(r[0] + 4)), "8-byte")
    refused(err(epe=tab(d[0] + 2)), "4-byte")
    refused(err(hist=tab(d[0] + 2)), "4-byte")
    refused(err(rec=tab(s[0])), "overlaps")                                          # the record onto the estimate
    refused(err(epe=tab(s[1])), "overlaps")
    refused(err(epe=tab(s[1] + 8 * (n - 1))), "overlaps")                            # ... onto its last element only
    refused(err(hist=tab(m), occ=tab(m)), "overlaps")
    refused(err(epe=tab(d[0]), hist=tab(d[0])), "overlaps")
    refused(err(epe=tab(d[0]), hist=tab(d[0] + 4 * (n - 1))), "overlaps")
    refused(err(rec=tab(d[0] + 8), epe=tab(d[0])), "overlaps")
    refused(err(n_=2, flo=tab(s[0], s[2]), gt=tab(s[1], s[3]), rec=tab(r[0], r[0])), "overlaps")      # two slots, one record
    refused(err(n_=2, flo=tab(s[0], s[2]), gt=tab(s[1], s[3]), rec=tab(r[0], r[1]), epe=tab(d[0], s[0])), "overlaps")

    def enc(n_=1, flo=tab(s[0]), occ=None, kind=R.WHEEL_RGB8, scale=0.0, out=tab(d[0]), nx_=nx, ny_=ny):
        return L.ofx_flow_encode_dev(h, n_, flo, occ, kind, scale, out, nx_, ny_)

    def dec(n_=1, code=tab(s[0]), kind=R.KITTI_U16, scale=0.0, flo=tab(d[0]), occ=None, nx_=nx, ny_=ny):
        return L.ofx_flow_decode_dev(h, n_, code, kind, scale, flo, occ, nx_, ny_)

    for call, a, b in ((enc, "flo", "out"), (dec, "code", "flo")):
        refused(call(**{a: None}), "NULL")
        refused(call(**{b: None}), "NULL")
        refused(call(**{a: tab(None)}), "NULL")
        refused(call(**{b: tab(None)}), "NULL")
        refused(call(n_=0), "n = 0")
        refused(call(nx_=1), "too small")
        refused(call(nx_=65536, ny_=65536), "int")
        for bad in (0, 4, -1):
            refused(call(kind=bad), "kind = %d" % bad)
        for bad in (-1.0, nan, inf):
            refused(call(kind=R.BOUND_U8, scale=bad), "scale")
        refused(call(kind=R.BOUND_U8, scale=0.0), "scale = 0")
        refused(call(kind=R.KITTI_U16, scale=1.0), "scale = 1")
    refused(enc(scale=-1.0), "scale")
    refused(dec(kind=R.WHEEL_RGB8), "no decoding")
    refused(enc(flo=tab(s[0] + 4)), "8-byte")
    refused(dec(flo=tab(d[0] + 4)), "8-byte")
    refused(enc(kind=R.KITTI_U16, out=tab(d[0] + 1)), "2-byte")
    refused(dec(code=tab(s[0] + 1)), "2-byte")
    refused(enc(out=tab(s[0])), "overlaps")
    refused(enc(out=tab(s[0] + 8 * n - 1)), "overlaps")
    refused(enc(out=tab(m), occ=tab(m)), "overlaps")
    refused(enc(n_=2, flo=tab(s[0], s[1]), out=tab(d[0], d[0] + 3 * n - 1)), "overlaps")
    refused(dec(flo=tab(s[0])), "overlaps")
    refused(dec(flo=tab(d[0]), occ=tab(d[0] + 8 * n - 1)), "overlaps")
    refused(dec(n_=2, code=tab(s[0], s[1]), flo=tab(d[0], d[0])), "overlaps")
    gpu64.synchronize()
    assert (dst.cpu().numpy() == -7.0).all() and (recs.cpu().numpy() == -7.0).all() and not imap.cpu().numpy().any()
    assert src.cpu().numpy().tobytes() == before.tobytes()
    # NULL optional tables and NULL entries in them are fine; inputs may share; adjacent buffers do not overlap
    flo = before[0][:n * 2].reshape(ny, nx, 2)
    assert err(gt=tab(s[0]), occ=tab(None), n_thr=0, ta=None, tr=None, epe=tab(None), hist=tab(None), n_bins=0, bin_w=0.0) == 0
    gpu64.synchronize()
    got = recs[0].cpu().numpy()
    assert got[0] == n and not got[[1, 2, 3, 5, 6]].any() and not got[8:16].any() and (got[16:] == -7.0).all()
    assert enc(kind=R.BOUND_U8, scale=2.0, out=tab(d[1])) == 0 and dec(code=tab(d[1]), kind=R.BOUND_U8, scale=2.0, flo=tab(d[2]), occ=tab(d[1] + 2 * n)) == 0
    gpu64.synchronize()
    raw = dst[1].cpu().numpy().view(np.uint8)
    assert raw[:2 * n].tobytes() == R.encode_bound(flo, None, 2.0).tobytes() and not raw[2 * n:3 * n].any()
    assert dst[2].cpu().numpy()[:2 * n].tobytes() == R.decode_bound(R.encode_bound(flo, None, 2.0), 2.0)[0].tobytes()
    assert (dst[2].cpu().numpy()[2 * n:] == -7.0).all()
