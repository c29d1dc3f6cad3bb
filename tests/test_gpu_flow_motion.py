"""ofx_flow_motion_fit_dev and ofx_flow_motion_apply_dev against the numpy restatement (tests/flow_motion_ref.py): records double for
double, payloads float for float, maps byte for byte -- at 2x2, 3x5, 64x2, 65x3 (one element in a second lane round), 63x65 and
130x131 (rows and row sums both beyond 64 and 128); 1, 3, 16 and 17 slots (two launches); maps at byte offsets 0, 1 and 3, payloads
8 but not 16 bytes aligned; guard bytes around every destination; the residual in place; NaN and Inf vectors; an initial record;
every model; degenerate slots beside healthy ones; both storage precisions; host buffers; the apply entry; every refusal."""
import numpy as np
import pytest

import flow_motion_ref as R

pytestmark = pytest.mark.gpu

ERR_ARG = 1
GUARD = 64                                 # bytes before and behind every destination
FILL = 0xA5
SIZES = [(2, 2), (3, 5), (64, 2), (65, 3), (63, 65), (130, 131)]
MODELS = (R.TRANSLATION, R.SIMILARITY, R.AFFINE)
_want = {}


class Dev:
    """device buffers of one call: inputs at a byte offset into their allocation, destinations between guard bytes"""

    def __init__(self):
        self.keep = []

    def put(self, arr, off=0):
        import torch
        if arr is None:
            return None
        raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8).copy()
        t = torch.zeros(off + raw.size + 16, dtype=torch.uint8, device="cuda")
        t[off:off + raw.size] = torch.from_numpy(raw).cuda()
        self.keep.append(t)
        return t.data_ptr() + off

    def out(self, nbytes, off=0, init=None):
        """-> (pointer, handle for get); init: bytes that the destination holds before the call (in place)"""
        import torch
        t = torch.full((GUARD + off + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        if init is not None:
            t[GUARD + off:GUARD + off + nbytes] = torch.from_numpy(np.frombuffer(np.ascontiguousarray(init).tobytes(), dtype=np.uint8).copy()).cuda()
        self.keep.append(t)
        return t.data_ptr() + GUARD + off, (t, off, nbytes)

    @staticmethod
    def get(handle, dtype, shape):
        t, off, nbytes = handle
        raw = t.cpu().numpy()
        assert (raw[:GUARD + off] == FILL).all() and (raw[GUARD + off + nbytes:] == FILL).all(), "bytes outside the destination were written"
        return np.frombuffer(raw[GUARD + off:GUARD + off + nbytes].tobytes(), dtype=dtype).reshape(shape)


def sync():
    import torch
    torch.cuda.synchronize()


def run_fit(ctx, slots, model, n_fits, c_first, c_last, flo_off=0, occ_off=0, outs=("model", "resid", "inl"), inplace=False):
    """slots: list of (payload, map | None, initial record | None) -> list of dicts rec, model, resid, inl (None: not asked for)"""
    ny, nx, _ = slots[0][0].shape
    d = Dev()
    tab = {k: [] for k in ("flo", "occ", "init", "rec", "model", "resid", "inl")}
    handles = []
    for flo, occ, init in slots:
        h = {}
        if inplace:
            p, h["resid"] = d.out(nx * ny * 8, flo_off, init=flo)
            tab["flo"].append(p)
            tab["resid"].append(p)
        else:
            tab["flo"].append(d.put(flo, flo_off))
            p, h["resid"] = d.out(nx * ny * 8, flo_off) if "resid" in outs else (None, None)
            tab["resid"].append(p)
        tab["occ"].append(d.put(occ, occ_off))
        tab["init"].append(d.put(init, 8))
        p, h["rec"] = d.out(128, 8)
        tab["rec"].append(p)
        p, h["model"] = d.out(nx * ny * 8, flo_off) if "model" in outs else (None, None)
        tab["model"].append(p)
        p, h["inl"] = d.out(nx * ny, occ_off) if "inl" in outs else (None, None)
        tab["inl"].append(p)
        handles.append(h)
    sync()
    none_if_empty = lambda xs: xs if any(x is not None for x in xs) else None
    ctx.flow_motion_fit_dev(tab["flo"], tab["rec"], nx, ny, model=model, n_fits=n_fits, c_first=c_first, c_last=c_last,
                            d_occ=none_if_empty(tab["occ"]), d_motion_init=none_if_empty(tab["init"]),
                            d_flo_model=none_if_empty(tab["model"]), d_flo_resid=none_if_empty(tab["resid"]),
                            d_inlier=none_if_empty(tab["inl"]))
    ctx.synchronize()
    return [collect(d, h, nx, ny) for h in handles]


def collect(d, h, nx, ny):
    kinds = {"rec": (np.float64, (16,)), "model": (np.float32, (ny, nx, 2)), "resid": (np.float32, (ny, nx, 2)), "inl": (np.uint8, (ny, nx))}
    return {k: None if h.get(k) is None else d.get(h[k], *kinds[k]) for k in kinds}


def want(slot, model, n_fits, c_first, c_last, key=None):
    """the restatement's record and outputs of one slot; `key` caches it"""
    k = None if key is None else (key, model, n_fits, c_first, c_last)
    if k is None or k not in _want:
        flo, occ, init = slot
        rec = R.fit(flo, occ, model, n_fits, c_first, c_last, init)
        mdl, res, inl = R.outputs(rec[:6], c_last, flo, occ)
        if k is None:
            return dict(rec=rec, model=mdl, resid=res, inl=inl)
        _want[k] = dict(rec=rec, model=mdl, resid=res, inl=inl)
    return _want[k]


def same(got, exp, what=""):
    for k in ("rec", "model", "resid", "inl"):
        if got[k] is not None:
            assert got[k].tobytes() == exp[k].tobytes(), (what, k, got[k] if k == "rec" else "", exp[k] if k == "rec" else "")


def slots_of(nx, ny):
    """a plain slot, one with a map, one with a map and NaN / Inf vectors, one that starts from a record"""
    flo, _ = R.scene(nx, ny)
    init = R.record(np.array([1.0, 2.5, -1.0, -1.0, 0.25, 1.5]), nx, ny, 0.0, 0, 1.0, False)
    return [(flo, None, None), (flo, R.flags(nx, ny), None), (R.nonfinite(flo), R.flags(nx, ny, 1), None), (flo, None, init)]


@pytest.mark.parametrize("nx,ny", SIZES)
def test_fit_is_the_restatement(gpu64, nx, ny):
    slots = slots_of(nx, ny)
    for model in MODELS:
        exp = [want(s, model, 3, 8.0, 1.0, key=(nx, ny, g)) for g, s in enumerate(slots)]
        for flo_off, occ_off in ((0, 0), (8, 1), (0, 3)):
            got = run_fit(gpu64, slots, model, 3, 8.0, 1.0, flo_off, occ_off)
            for g in range(len(slots)):
                same(got[g], exp[g], (model, flo_off, occ_off, g))
    got = run_fit(gpu64, slots, R.AFFINE, 3, 8.0, 1.0, outs=())                       # the records alone
    for g in range(len(slots)):
        assert got[g]["model"] is None and got[g]["inl"] is None
        same(got[g], want(slots[g], R.AFFINE, 3, 8.0, 1.0, key=(nx, ny, g)), g)


def test_eight_reweighted_fits_recover_the_camera_on_the_device(gpu64):
    nx, ny = 131, 77
    flo, fg = R.scene(nx, ny)
    got = run_fit(gpu64, [(flo, None, None)], R.AFFINE, 9, 16.0, 1.0)[0]
    same(got, want((flo, None, None), R.AFFINE, 9, 16.0, 1.0))
    assert got["rec"][13] == 9 and got["rec"][15] == 0
    assert R.mean_epe(got["rec"][:6], R.TRUE[R.AFFINE], nx, ny) < 0.02 and np.array_equal(got["inl"] == 0, ~fg)


def degenerate_pool(nx, ny):
    flo, _ = R.scene(nx, ny)
    column = np.full((ny, nx), 255, dtype=np.uint8)
    column[:, 5] = 0
    far = np.array(flo)
    far[..., 0] += np.where(np.arange(nx) % 2 == 0, 50.0, -50.0).astype(np.float32)[None, :]
    init = R.record(np.array(R.TRUE[R.AFFINE]), nx, ny, 5.0, 3, 1.0, False)
    return [(flo, None, None),                                                        # healthy
            (flo, np.full((ny, nx), 7, dtype=np.uint8), None),                        # all pixels flagged: zeros, stopped at fit 0
            (flo, R.flags(nx, ny), None),                                             # healthy, with a map
            (flo, column, None),                                                      # one valid column: no affine fit
            (far, None, None),                                                        # every weight is zero at the second fit
            (flo, np.full((ny, nx), 255, dtype=np.uint8), init),                      # all flagged, from a record: the record's theta
            (R.nonfinite(flo), None, init)]


@pytest.mark.parametrize("n", [1, 3, 16, 17])
def test_any_number_of_slots_and_degenerate_slots_beside_healthy_ones(gpu64, n):
    nx, ny = 37, 29
    pool = degenerate_pool(nx, ny)
    pick = [(3 * g + 2) % len(pool) for g in range(n)]                               # slot 16, the second launch, is degenerate
    got = run_fit(gpu64, [pool[k] for k in pick], R.AFFINE, 4, 2.0, 1.0, occ_off=1)
    assert len(got) == n
    for g in range(n):
        same(got[g], want(pool[pick[g]], R.AFFINE, 4, 2.0, 1.0, key=("pool", pick[g])), g)
    if n >= 16:
        stopped = [got[g]["rec"][15] for g in range(n)]
        done = [got[g]["rec"][13] for g in range(n)]
        assert 1.0 in stopped and 0.0 in stopped and {0.0, 1.0, 4.0} <= set(done)


def test_degenerate_slots_of_every_model(gpu64):
    nx, ny = 37, 29
    pool = degenerate_pool(nx, ny)
    for model in MODELS:
        got = run_fit(gpu64, pool, model, 3, 2.0, 1.0)
        for g in range(len(pool)):
            same(got[g], want(pool[g], model, 3, 2.0, 1.0, key=("pool", g)), (model, g))
        assert got[1]["rec"][15] == 1.0 and not got[1]["rec"][:14].any() and (got[1]["inl"] == 255).all()
        assert np.array_equal(got[5]["rec"][:12], pool[5][2][:12]) and got[5]["rec"][15] == 1.0
    assert got[3]["rec"][15] == 1.0 and got[4]["rec"][13] == 1.0 and got[4]["rec"][15] == 1.0


def test_residual_in_place_and_mixed_null_entries(gpu64):
    nx, ny = 130, 70
    slots = slots_of(nx, ny)
    got = run_fit(gpu64, slots, R.SIMILARITY, 3, 8.0, 1.0, flo_off=8, occ_off=3, inplace=True)
    for g in range(len(slots)):
        same(got[g], want(slots[g], R.SIMILARITY, 3, 8.0, 1.0, key=(nx, ny, g)), g)
    # every output asked for by one slot only
    d = Dev()
    flo = [d.put(s[0]) for s in slots]
    recs = [d.out(128) for _ in slots]
    o_model, o_resid, o_inl = d.out(nx * ny * 8), d.out(nx * ny * 8), d.out(nx * ny, 1)
    sync()
    gpu64.flow_motion_fit_dev(flo, [r[0] for r in recs], nx, ny, model=R.SIMILARITY, n_fits=3, c_first=8.0, c_last=1.0,
                              d_occ=[None, d.put(slots[1][1]), d.put(slots[2][1], 3), None], d_motion_init=[None, None, None, d.put(slots[3][2])],
                              d_flo_model=[o_model[0], None, None, None], d_flo_resid=[None, o_resid[0], None, None],
                              d_inlier=[None, None, o_inl[0], None])
    gpu64.synchronize()
    exp = [want(slots[g], R.SIMILARITY, 3, 8.0, 1.0, key=(nx, ny, g)) for g in range(4)]
    for g in range(4):
        assert d.get(recs[g][1], np.float64, (16,)).tobytes() == exp[g]["rec"].tobytes(), g
    assert d.get(o_model[1], np.float32, (ny, nx, 2)).tobytes() == exp[0]["model"].tobytes()
    assert d.get(o_resid[1], np.float32, (ny, nx, 2)).tobytes() == exp[1]["resid"].tobytes()
    assert d.get(o_inl[1], np.uint8, (ny, nx)).tobytes() == exp[2]["inl"].tobytes()


def test_an_exact_model_flow_has_an_all_zero_map_and_its_theta_comes_back(gpu64):
    nx, ny = 67, 35
    for model in MODELS:
        flo = R.model_payload(R.TRUE[model], nx, ny)
        got = run_fit(gpu64, [(flo, None, None)], model, 4, 16.0, 1.0)[0]
        same(got, want((flo, None, None), model, 4, 16.0, 1.0))
        assert not got["inl"].any() and np.max(np.abs(got["rec"][:6] - np.array(R.TRUE[model]))) < 1e-6


def run_apply(ctx, nx, ny, recs, slots, cutoff, outs=("model", "resid", "inl"), flo_off=0, occ_off=0):
    """recs: records; slots: list of (payload | None, map | None)"""
    d = Dev()
    tab = {k: [] for k in ("rec", "flo", "occ", "model", "resid", "inl")}
    handles = []
    for rec, (flo, occ) in zip(recs, slots):
        h = {}
        tab["rec"].append(d.put(rec, 8))
        tab["flo"].append(d.put(flo, flo_off))
        tab["occ"].append(d.put(occ, occ_off))
        for k, nb, off in (("model", nx * ny * 8, flo_off), ("resid", nx * ny * 8, flo_off), ("inl", nx * ny, occ_off)):
            p, h[k] = d.out(nb, off) if k in outs and (k == "model" or flo is not None) else (None, None)
            tab[k].append(p)
        handles.append(h)
    sync()
    none_if_empty = lambda xs: xs if any(x is not None for x in xs) else None
    ctx.flow_motion_apply_dev(tab["rec"], nx, ny, cutoff=cutoff, d_flo=none_if_empty(tab["flo"]), d_occ=none_if_empty(tab["occ"]),
                              d_flo_model=none_if_empty(tab["model"]), d_flo_resid=none_if_empty(tab["resid"]),
                              d_inlier=none_if_empty(tab["inl"]))
    ctx.synchronize()
    return [collect(d, h, nx, ny) for h in handles]


@pytest.mark.parametrize("n", [4, 17])
def test_apply_equals_the_fit_entrys_outputs_and_takes_the_callers_records(gpu64, n):
    nx, ny = 65, 35
    base = slots_of(nx, ny)
    slots = [base[g % 4] for g in range(n)]
    fitted = run_fit(gpu64, slots, R.AFFINE, 3, 8.0, 0.75, occ_off=1)
    got = run_apply(gpu64, nx, ny, [f["rec"] for f in fitted], [(s[0], s[1]) for s in slots], 0.75, flo_off=8, occ_off=3)
    for g in range(n):
        for k in ("model", "resid", "inl"):
            assert got[g][k].tobytes() == fitted[g][k].tobytes(), (g, k)
    # a record of the caller's, another cut-off, and slots without a payload: the model payload alone
    mine = [R.record(np.array([0.5 * g, 1.0, -2.0, 3.0, 0.125 * g, -1.0]), nx, ny, 0.0, 0, 1.0, False) for g in range(n)]
    some = [(None, None) if g % 3 == 1 else (s[0], s[1]) for g, s in enumerate(slots)]
    got = run_apply(gpu64, nx, ny, mine, some, 2.5, occ_off=1)
    for g in range(n):
        flo, occ = some[g]
        if flo is None:
            assert got[g]["resid"] is None and got[g]["model"].tobytes() == R.model_payload(mine[g][:6], nx, ny).tobytes(), g
        else:
            mdl, res, inl = R.outputs(mine[g][:6], 2.5, flo, occ)
            assert got[g]["model"].tobytes() == mdl.tobytes() and got[g]["resid"].tobytes() == res.tobytes(), g
            assert got[g]["inl"].tobytes() == inl.tobytes(), g


def test_f64_and_f32_contexts_write_the_same_bytes_and_host_buffers_are_staged(gpu64, gpu32):
    nx, ny = 67, 35
    slots = slots_of(nx, ny)
    a, b = run_fit(gpu64, slots, R.AFFINE, 3, 8.0, 1.0, occ_off=1), run_fit(gpu32, slots, R.AFFINE, 3, 8.0, 1.0, occ_off=1)
    exp = [want(s, R.AFFINE, 3, 8.0, 1.0, key=(nx, ny, g)) for g, s in enumerate(slots)]
    for g in range(len(slots)):
        same(a[g], exp[g], g)
        same(b[g], exp[g], g)
    # host memory in, host memory out (the front-end's route), the residual in place in slot 1
    n = len(slots)
    flo = [np.array(s[0]) for s in slots]
    occ = [None if s[1] is None else np.array(s[1]) for s in slots]
    init = [None if s[2] is None else np.array(s[2]) for s in slots]
    rec = np.full((n, 18), -7.0)
    mdl = np.full((n, ny * nx * 2 + 4), -7.0, dtype=np.float32)
    res = np.full((n, ny * nx * 2 + 4), -7.0, dtype=np.float32)
    inl = np.full((n, ny * nx + 4), 9, dtype=np.uint8)
    ptr = lambda xs: [None if x is None else x.ctypes.data for x in xs]
    gpu64.flow_motion_fit_dev(ptr(flo), [rec[g].ctypes.data for g in range(n)], nx, ny, model=R.AFFINE, n_fits=3, c_first=8.0, c_last=1.0,
                              d_occ=ptr(occ), d_motion_init=ptr(init), d_flo_model=[mdl[g].ctypes.data for g in range(n)],
                              d_flo_resid=[flo[1].ctypes.data if g == 1 else res[g].ctypes.data for g in range(n)],
                              d_inlier=[inl[g].ctypes.data for g in range(n)])
    gpu64.synchronize()
    for g in range(n):
        assert rec[g][:16].tobytes() == exp[g]["rec"].tobytes() and (rec[g][16:] == -7.0).all(), g
        assert mdl[g][:ny * nx * 2].tobytes() == exp[g]["model"].tobytes() and (mdl[g][ny * nx * 2:] == -7.0).all(), g
        r = flo[1].ravel() if g == 1 else res[g][:ny * nx * 2]
        assert r.tobytes() == exp[g]["resid"].tobytes() and (res[g][ny * nx * 2:] == -7.0).all(), g
        assert inl[g][:ny * nx].tobytes() == exp[g]["inl"].tobytes() and (inl[g][ny * nx:] == 9).all(), g
    out = np.full((ny * nx * 2 + 4,), -7.0, dtype=np.float32)
    gpu64.flow_motion_apply_dev([rec[0].ctypes.data], nx, ny, d_flo_model=[out.ctypes.data])
    gpu64.synchronize()
    assert out[:ny * nx * 2].tobytes() == exp[0]["model"].tobytes() and (out[ny * nx * 2:] == -7.0).all()


def test_refusals_are_invalid_arguments_and_write_nothing(gpu64):
    import ctypes as C
    import torch
    nx, ny = 9, 7
    n = nx * ny
    rng = np.random.default_rng(3)
    src = torch.from_numpy(rng.normal(0.0, 1.0, (3, n * 2 + 2)).astype(np.float32)).cuda()
    dst = torch.full((4, n * 2 + 2), -7.0, dtype=torch.float32, device="cuda")
    omap = torch.full((2, n + 8), 9, dtype=torch.uint8, device="cuda")
    imap = torch.zeros((n + 8,), dtype=torch.uint8, device="cuda")
    recs = torch.full((3, 18), -7.0, dtype=torch.float64, device="cuda")
    init = torch.zeros((18,), dtype=torch.float64, device="cuda")
    sync()
    s = [src[k].data_ptr() for k in range(3)]
    d = [dst[k].data_ptr() for k in range(4)]
    o = [omap[k].data_ptr() for k in range(2)]
    r = [recs[k].data_ptr() for k in range(3)]
    m, i0 = imap.data_ptr(), init.data_ptr()
    vp = C.c_void_p
    L, h = gpu64.L, gpu64.h
    tab = lambda *xs: (vp * len(xs))(*xs)

    def refused(status, word):
        assert status == ERR_ARG, word
        assert word in L.ofx_last_error(h).decode(), (word, L.ofx_last_error(h))

    def fit(n_=1, flo=tab(s[0]), occ=None, ini=None, rec=tab(r[0]), model=6, n_fits=2, c_first=4.0, c_last=1.0, mdl=None, res=None,
            inl=None, nx_=nx, ny_=ny):
        return L.ofx_flow_motion_fit_dev(h, n_, flo, occ, ini, rec, model, n_fits, c_first, c_last, mdl, res, inl, nx_, ny_)

    refused(fit(flo=None), "NULL")
    refused(fit(rec=None), "NULL")
    refused(fit(flo=tab(None)), "NULL")
    refused(fit(n_=2, flo=tab(s[0], s[1]), rec=tab(r[0], None)), "slot 1")
    refused(fit(n_=0), "n = 0")
    refused(fit(n_=-1), "n = -1")
    refused(fit(n_fits=0), "n_fits = 0")
    for bad in (0, 1, 3, 5, 7, -6):
        refused(fit(model=bad), "model = %d" % bad)
    refused(fit(nx_=1), "too small")
    refused(fit(ny_=1), "too small")
    refused(fit(nx_=65536, ny_=65536), "int")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(fit(c_first=bad), "c_first")
        refused(fit(c_last=bad), "c_last")
    refused(fit(c_first=1.0, c_last=2.0), "below c_last")
    refused(fit(flo=tab(s[0] + 4)), "8-byte")
    refused(fit(mdl=tab(d[0] + 4)), "8-byte")
    refused(fit(res=tab(d[0] + 4)), "8-byte")
    refused(fit(rec=tab(r[0] + 4)), "8-byte")
    refused(fit(ini=tab(i0 + 4)), "8-byte")
    refused(fit(mdl=tab(s[0])), "reads")                                             # the model payload onto the payload read
    refused(fit(inl=tab(m), occ=tab(m)), "reads")
    refused(fit(ini=tab(i0), rec=tab(i0)), "reads")
    refused(fit(n_=2, flo=tab(s[0], s[1]), rec=tab(r[0], r[1]), res=tab(s[1], d[1])), "slot 0")       # another slot's payload
    refused(fit(n_=2, flo=tab(s[0], s[0]), rec=tab(r[0], r[1]), res=tab(s[0], d[1])), "slot 0")       # in place, but slot 1 reads it too
    refused(fit(mdl=tab(d[0]), res=tab(d[0])), "same buffer")
    refused(fit(rec=tab(d[0]), mdl=tab(d[0])), "same buffer")
    refused(fit(n_=2, flo=tab(s[0], s[1]), rec=tab(r[0], r[1]), mdl=tab(d[0], d[1]), inl=tab(o[0], d[1])), "slot 1")

    def apply(n_=1, rec=tab(r[2]), flo=tab(s[0]), occ=None, cutoff=1.0, mdl=None, res=None, inl=None, nx_=nx, ny_=ny):
        return L.ofx_flow_motion_apply_dev(h, n_, rec, flo, occ, cutoff, mdl, res, inl, nx_, ny_)

    refused(apply(rec=None), "NULL")
    refused(apply(rec=tab(None)), "NULL")
    refused(apply(n_=0), "n = 0")
    refused(apply(nx_=1), "too small")
    refused(apply(nx_=65536, ny_=65536), "int")
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        refused(apply(cutoff=bad), "cutoff")
    refused(apply(rec=tab(r[2] + 4)), "8-byte")
    refused(apply(flo=tab(s[0] + 4)), "8-byte")
    refused(apply(mdl=tab(d[0] + 4)), "8-byte")
    refused(apply(flo=None, res=tab(d[0])), "without a payload")
    refused(apply(flo=tab(None), inl=tab(o[0])), "without a payload")
    refused(apply(mdl=tab(s[0])), "reads")
    refused(apply(mdl=tab(r[2])), "reads")
    refused(apply(mdl=tab(d[0]), res=tab(d[0])), "same buffer")
    gpu64.synchronize()
    assert (dst.cpu().numpy() == -7.0).all() and (omap.cpu().numpy() == 9).all() and (recs.cpu().numpy() == -7.0).all()
    # NULL optional tables and NULL entries in them are fine, and so is the residual in place
    flo = src[0].cpu().numpy()[:n * 2].reshape(ny, nx, 2).copy()
    assert fit(occ=tab(None), ini=tab(None), mdl=tab(None), res=tab(s[0]), inl=tab(None)) == 0
    gpu64.synchronize()
    exp = want((flo, None, None), R.AFFINE, 2, 4.0, 1.0)
    assert recs[0].cpu().numpy()[:16].tobytes() == exp["rec"].tobytes() and (recs[0].cpu().numpy()[16:] == -7.0).all()
    assert src[0].cpu().numpy()[:n * 2].tobytes() == exp["resid"].tobytes()
    assert apply(rec=tab(r[0]), flo=None, mdl=tab(d[0])) == 0
    gpu64.synchronize()
    assert dst[0].cpu().numpy()[:n * 2].tobytes() == exp["model"].tobytes() and (dst[0].cpu().numpy()[n * 2:] == -7.0).all()
