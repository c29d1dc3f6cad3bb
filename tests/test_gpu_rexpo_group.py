"""robust_expo_methods for lockstep groups and batches of colour pairs on device-resident images: ofx_robust_expo_group_dev and
ofx_robust_expo_batch_dev against the recorded fixtures, the compiled reference composed as tests/rexpo_pyramid_ref.py does, and
the library's own lone entry (ofx_robust_expo_pyramid), which every pair of a group must reproduce bit for bit.

Bound against the reference: BOUND = 1e-11 of tests/test_gpu_rexpo_color.py on the flow (the order of the stopping sum is the
only difference) plus 2^-24 |value|, half a float32 ulp, for the payload's rounding.

Slot 0 of a group is colour_pair(name, ..., k = 0), the input of the fixtures; the other slots are P1 with k = 1, 2, ..., all
distinct, and ONE P0 at most (P0 ignores k, so two P0 slots hold the same images and a mix-up between them could not be seen).

Every comparison with the reference prints its figures before it asserts (run with -s to keep them)."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUND = 1e-11
SENTINEL = -7.0


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


H = _load("rexpo_pyramid_ref", os.path.join(HERE, "rexpo_pyramid_ref.py"))
CASES = json.load(open(os.path.join(GOLDEN, "cases_color_pyramid.json")))


def _slots(name0, G):
    """(pair name, k) of every slot of a group: no two slots hold the same images"""
    return [(name0, 0)] + [("P0" if k == 2 and name0 != "P0" else "P1", k) for k in range(1, G)]


def _inputs(synth, slots, nx, ny, nz, dtype=np.float64, integer=False):
    """host pairs, device images (ny, nx, nz) of `dtype`, and a payload array prefilled with SENTINEL"""
    import torch
    pairs = [synth.colour_pair(name, nx, ny, nz, k) for name, k in slots]
    if integer:
        pairs = [(np.floor(a), np.floor(b)) for a, b in pairs]
    d1 = [torch.from_numpy(p[0].astype(dtype)).cuda() for p in pairs]
    d2 = [torch.from_numpy(p[1].astype(dtype)).cuda() for p in pairs]
    flo = torch.full((len(slots), ny, nx, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return pairs, d1, d2, flo


def _ptr(ts):
    return [t.data_ptr() for t in ts]


def _group(gpu, d1, d2, flo, nx, ny, nz, **kw):
    st = gpu.robust_expo_group_dev(_ptr(d1), _ptr(d2), [flo[k].data_ptr() for k in range(len(d1))], nx, ny, nz, **kw)
    gpu.synchronize()
    return st, flo.cpu().numpy().copy()


_LONE = {}


def _lone(gpu, tag, slot, pair, **kw):
    """robust_expo_pyramid of one pair alone -> (float32 payload, sweep table, stopping values); solved once per module"""
    key = (tag, slot, pair[0].shape, tuple(sorted(kw.items())))
    if key not in _LONE:
        u, v = gpu.robust_expo_pyramid(pair[0], pair[1], **kw)
        st = gpu.stats()
        _LONE[key] = (np.stack([u, v], axis=-1).astype(np.float32), st.iterations().copy(), st.errors().copy(), st.work_pix_iters)
    return _LONE[key]


def _within(tag, got, u, v):
    """payload against a reference flow: 1e-11 + half a float32 ulp"""
    du, dv = np.abs(got[..., 0] - u), np.abs(got[..., 1] - v)
    su, sv = float((du - 2.0 ** -24 * np.abs(u)).max()), float((dv - 2.0 ** -24 * np.abs(v)).max())
    print("%s: max|du| = %.3g, max|dv| = %.3g; beyond half an ulp: %.3g, %.3g" % (tag, du.max(), dv.max(), max(su, 0), max(sv, 0)))
    return bool((du <= BOUND + 2.0 ** -24 * np.abs(u)).all() and (dv <= BOUND + 2.0 ** -24 * np.abs(v)).all())


# ---- 1. the recorded reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rexpocp_m1_p1_96x64x3_s3", "rexpocp_m3_p0_131x67x4_s3", "rexpocp_m1_p1_72x56x3_s2_nu07",
                                  "rexpocp_m1_p1_64x48x1_s3"])
def test_pair_0_of_a_group_against_the_recorded_reference(gpu64, synth, name):
    c, g = CASES[name], np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    pairs, d1, d2, flo = _inputs(synth, _slots(c["pair"], 3), nx, ny, nz)
    st, got = _group(gpu64, d1, d2, flo, nx, ny, nz, nscales=c["nscales"], nu=c["nu"], **c["params"])
    print(name, "sweeps", st[0].iterations().tolist(), "recorded", g["iters"].tolist())
    ok = _within(name, got[0], g["u"], g["v"])
    assert np.array_equal(st[0].iterations(), g["iters"])
    assert ok


# ---- 2. live against the compiled reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [1, 2, 3])
def test_every_pair_of_a_group_against_the_compiled_reference(gpu64, ref, synth, method):
    nx, ny, nz, ns = 96, 64, 3, 3
    kw = dict(method=method, alpha=50.0, gamma=10.0, lam=0.1, outer=3)
    pairs, d1, d2, flo = _inputs(synth, _slots("P1", 3), nx, ny, nz)
    st, got = _group(gpu64, d1, d2, flo, nx, ny, nz, nscales=ns, **kw)
    oks = []
    for k, (I1, I2) in enumerate(pairs):
        ur, vr = H.compose(ref, I1, I2, ns, 0.5, **kw)
        assert np.isfinite(ur).all() and np.abs(ur).max() > 0.1
        oks.append(_within("method %d pair %d" % (method, k), got[k], ur, vr))
    assert all(oks), oks


# ---- 3. a group equals the pairs alone ----------------------------------------------------------------------------------------
def _equals_alone(gpu, tag, synth, G, nx, ny, nz, name0="P1", **kw):
    slots = _slots(name0, G)
    pairs, d1, d2, flo = _inputs(synth, slots, nx, ny, nz)
    st, got = _group(gpu, d1, d2, flo, nx, ny, nz, **kw)
    tables = set()
    for k in range(G):
        want, iters, errs, work = _lone(gpu, tag, slots[k], pairs[k], **kw)
        assert np.array_equal(got[k], want), k
        assert np.array_equal(st[k].iterations(), iters), k
        assert np.array_equal(st[k].errors(), errs), k
        assert st[k].work_pix_iters == work, k
        tables.add(tuple(int(x) for x in iters.ravel()))
    return tables


@pytest.mark.parametrize("G", [1, 2, 5, 16])
def test_group_equals_the_pairs_solved_alone(gpu64, synth, G):
    tables = _equals_alone(gpu64, "f64", synth, G, 64, 48, 3, method=1, alpha=50.0, gamma=10.0, lam=0.1, nscales=2, outer=3)
    if G >= 5:
        assert len(tables) > 1          # the pairs really stop at different sweeps


def test_group_of_four_channels_three_scales_two_inner(gpu64, synth):
    _equals_alone(gpu64, "f64", synth, 3, 131, 67, 4, name0="P0", method=3, alpha=30.0, gamma=10.0, lam=1.0, nscales=3, inner=2, outer=2)


def test_no_two_slots_of_a_group_share_their_images(synth):
    for name0 in ("P0", "P1"):
        pairs = [synth.colour_pair(name, 64, 48, 3, k) for name, k in _slots(name0, 16)]
        for a in range(16):
            for b in range(a + 1, 16):
                assert not np.array_equal(pairs[a][0], pairs[b][0]) or not np.array_equal(pairs[a][1], pairs[b][1]), (name0, a, b)


# ---- 4. one channel --------------------------------------------------------------------------------------------------------------
def test_one_channel_group_is_the_reference_named_entry(gpu64, synth):
    nx, ny, ns = 64, 48, 3
    kw = dict(method=1, alpha=37.5, gamma=10.0, lam=0.1, outer=3)
    pairs, d1, d2, flo = _inputs(synth, _slots("P1", 3), nx, ny, 1)
    st, got = _group(gpu64, d1, d2, flo, nx, ny, 1, nscales=ns, **kw)
    for k, (I1, I2) in enumerate(pairs):
        u, v = gpu64.robust_expo(np.ascontiguousarray(I1[..., 0]), np.ascontiguousarray(I2[..., 0]), nscales=ns, **kw)
        assert np.array_equal(got[k], np.stack([u, v], axis=-1).astype(np.float32)), k
        assert np.array_equal(st[k].iterations(), gpu64.stats().iterations()), k


# ---- 5. schedule independence -------------------------------------------------------------------------------------------------
def test_group_does_not_depend_on_batches_windows_and_rows(gpu64, synth):
    nx, ny, nz, G = 96, 64, 3, 5
    kw = dict(method=1, alpha=50.0, gamma=10.0, lam=0.1, nscales=2, outer=3)
    pairs, d1, d2, flo = _inputs(synth, _slots("P1", G), nx, ny, nz)
    st0, got0 = _group(gpu64, d1, d2, flo, nx, ny, nz, **kw)
    tables = [s.iterations().copy() for s in st0]
    assert len(set(tuple(int(x) for x in t.ravel()) for t in tables)) > 1
    for batch, window, rows in ((6, 3, 16), (300, 4, 125), (9, 8, 61)):
        for name, val in (("sor_batch", batch), ("sor_window", window), ("sor_rows", rows)):
            gpu64.set_option(name, val)
        try:
            st, got = _group(gpu64, d1, d2, flo, nx, ny, nz, **kw)
        finally:
            for name in ("sor_batch", "sor_window", "sor_rows"):
                gpu64.set_option(name, 0)
        for k in range(G):
            assert np.array_equal(st[k].iterations(), tables[k]), (batch, k)
            assert np.array_equal(got[k], got0[k]), (batch, k)


# ---- 6. f32 storage ------------------------------------------------------------------------------------------------------------
def test_f32_group_equals_the_lone_entry_on_integer_images(gpu32, synth):
    nx, ny, nz = 64, 48, 3
    kw = dict(method=1, alpha=50.0, gamma=10.0, lam=0.1, nscales=2, outer=3)
    pairs, d1, d2, flo = _inputs(synth, _slots("P1", 2), nx, ny, nz, dtype=np.float32, integer=True)
    st, got = _group(gpu32, d1, d2, flo, nx, ny, nz, **kw)
    for k, (I1, I2) in enumerate(pairs):
        assert np.array_equal(I1, I1.astype(np.float32)) and np.array_equal(I2, I2.astype(np.float32))
        u, v = gpu32.robust_expo_pyramid(I1, I2, **kw)
        assert np.array_equal(got[k], np.stack([u, v], axis=-1).astype(np.float32)), k
        assert np.array_equal(st[k].iterations(), gpu32.stats().iterations()), k


# ---- stats under option "profile" ------------------------------------------------------------------------------------------------
def test_profile_fills_every_record_and_leaves_the_lone_entry_alone(gpu64, synth):
    """pyramid_ms of the group in every record, iter_ms of the group entry only, ofx_ctx_expo_host_ms after a robust_expo entry
    and 0 after any other; the payloads do not move"""
    nx, ny, nz, G = 64, 48, 3, 3
    kw = dict(method=1, alpha=50.0, gamma=10.0, lam=0.1, nscales=2, outer=3)
    slots = _slots("P1", G)
    pairs, d1, d2, flo = _inputs(synth, slots, nx, ny, nz)
    gpu64.set_option("profile", 1)
    try:
        st, got = _group(gpu64, d1, d2, flo, nx, ny, nz, **kw)
        host_ms = gpu64.expo_host_ms()
        gpu64.robust_expo_pyramid(pairs[0][0], pairs[0][1], **kw)
        lone, lone_host_ms = gpu64.stats(), gpu64.expo_host_ms()
    finally:
        gpu64.set_option("profile", 0)
    assert host_ms > 0.0 and lone_host_ms > 0.0
    assert st[0].pyramid_ms > 0.0 and all(s.pyramid_ms == st[0].pyramid_ms for s in st)
    assert all(s.iter_ms[lv] > 0.0 for s in st for lv in range(2))
    assert lone.pyramid_ms > 0.0 and all(lone.iter_ms[lv] == 0.0 for lv in range(2))       # as before the group entries
    for k in range(G):
        want, iters, _, _ = _lone(gpu64, "f64", slots[k], pairs[k], **kw)
        assert np.array_equal(got[k], want) and np.array_equal(st[k].iterations(), iters), k
    I0, I1 = synth.pair("P1", 64, 48)
    gpu64.tvl1_multiscale(I0, I1, nscales=2)
    assert gpu64.expo_host_ms() == 0.0                   # every solver entry zeroes it


# ---- 7. the batch entry ----------------------------------------------------------------------------------------------------------
def test_batch_entry(ofx_mod, synth):
    """7 pairs on 2 contexts: groups of 4 + 3; payloads and the per-pair work equal the lone solves'"""
    nx, ny, nz, n = 64, 48, 3, 7
    kw = dict(method=1, alpha=50.0, gamma=10.0, lam=0.1, nscales=2, outer=3)
    slots = _slots("P1", n)
    pairs, d1, d2, flo = _inputs(synth, slots, nx, ny, nz)
    ctxs = [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)]
    solo = ofx_mod.Ofx(0, ofx_mod.F64)
    try:
        work = ofx_mod.robust_expo_batch_dev(ctxs, _ptr(d1), _ptr(d2), [flo[k].data_ptr() for k in range(n)], nx, ny, nz, **kw)
        got = flo.cpu().numpy().copy()
        for k in range(n):
            want, iters, _, w = _lone(solo, "f64", slots[k], pairs[k], **kw)
            assert np.array_equal(got[k], want), k
            sizes = [(64, 48), (32, 24)]
            assert work[k] == w == float(sum(int(iters[s].sum()) * sizes[s][0] * sizes[s][1] for s in range(2))), k
        assert ofx_mod.robust_expo_batch_dev(ctxs, [], [], [], nx, ny, nz, **kw) == []      # n_pairs = 0: OFX_OK
    finally:
        for c in ctxs + [solo]:
            c.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_are_found_before_any_work(gpu64, ofx_mod, synth):
    nx, ny, nz, G = 32, 24, 3, 2
    pairs, d1, d2, flo = _inputs(synth, _slots("P1", G), nx, ny, nz)
    a, b, f = _ptr(d1), _ptr(d2), [flo[k].data_ptr() for k in range(G)]
    ok = dict(nx=nx, ny=ny, nz=nz, method=1, alpha=50.0, gamma=10.0, lam=0.1, nscales=2, outer=2)

    def status(a=a, b=b, f=f, **over):
        kw = dict(ok, **over)
        try:
            gpu64.robust_expo_group_dev(a, b, f, kw.pop("nx"), kw.pop("ny"), kw.pop("nz"), **kw)
        except ofx_mod.OfxError as e:
            return e.status
        return 0

    for bad in (0, 5):
        assert status(nz=bad) == 1
    for bad in (0, 4):
        assert status(method=bad) == 1
    assert status(a=[], b=[], f=[]) == 1                               # n_pairs = 0
    assert status(a=a[:1] * 17, b=b[:1] * 17, f=f[:1] * 17) == 1       # n_pairs = 17
    assert status(a=[a[0], None]) == 1 and "pair 1" in gpu64.L.ofx_last_error(gpu64.h).decode()
    assert status(b=[b[0], None]) == 1 and status(f=[f[0], None]) == 1
    assert status(inner=-1) == 1 and status(outer=-1) == 1 and status(nscales=0) == 1
    gpu64.set_option("sor_exact", 0)
    try:
        assert status() == 1
    finally:
        gpu64.set_option("sor_exact", 1)
    assert status(nx=2, ny=2, nscales=1) == 1 and "3x3" in gpu64.L.ofx_last_error(gpu64.h).decode()
    assert status(nscales=4) == 2                                      # 32x24 -> 16x12 -> 8x6: the zoom Gaussian's radius is 6
    gpu64.synchronize()
    assert (flo.cpu().numpy() == SENTINEL).all()                       # no failed call wrote a payload
    # the context serves the next valid call
    st, got = _group(gpu64, d1, d2, flo, nx, ny, nz, **{k: v for k, v in ok.items() if k not in ("nx", "ny", "nz")})
    for k in range(G):
        want, iters, _, _ = _lone(gpu64, "f64", ("P1", k), pairs[k], **{k2: v for k2, v in ok.items() if k2 not in ("nx", "ny", "nz")})
        assert np.array_equal(got[k], want) and np.array_equal(st[k].iterations(), iters), k
