"""Context option "input": 8-bit, 16-bit, float and interleaved-RGB frames straight into the device-resident entries.

Every sample of these kinds is exact in double and in float, so the contract is bit identity: the operator
ofx_normalize_frames_dev against numpy in float64, and every *_dev solver family under "input" != 0 against the same call under
"input" = 0 on planes of the storage type that hold the same values -- payload bytes, occlusion maps, iteration / sweep tables
and stopping values with array_equal.  Sources are carved out of ONE device byte buffer so that every alignment a kernel has a
path for occurs in one pointer table; destinations are rows of one sentinel-filled tensor at shifting offsets."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = 1
SENTINEL = -7.0
KINDS = ("STORAGE", "U8", "U16", "F32", "RGB8")
NX, NY = 67, 45                                     # 3015 pixels: odd, so consecutive frames of a byte tensor change alignment


@pytest.fixture(scope="module")
def ctxs(ofx_mod):
    """contexts of this module alone (the option must not leak into the session's): two per storage precision"""
    c = {"f64": [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)], "f32": [ofx_mod.Ofx(0, ofx_mod.F32) for _ in range(2)]}
    yield c
    for v in c.values():
        for x in v:
            x.close()


def _set(ofx_mod, ctx, kind, vec=1, lut=1):
    ctx.set_option("input", getattr(ofx_mod, "IN_" + kind))
    ctx.set_option("input_vec", vec)
    ctx.set_option("input_lut", lut)


def _np_storage(prec):
    return np.float64 if prec == "f64" else np.float32


def _gray(rgb):
    """the front-ends' 8-bit rule: three products and two sums, each a float64 operation of its own, then truncation"""
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    pr, pg, pb = .299 * r, .587 * g, .114 * b
    s = pr + pg
    s = s + pb
    return s.astype(np.uint8)


def _align(kind, prec):
    return {"U8": 1, "U16": 2, "F32": 4, "RGB8": 1, "STORAGE": 8 if prec == "f64" else 4}[kind]


def _carve(pieces, align):
    """one device byte buffer holding the byte images `pieces`; piece k starts at a 4-byte boundary plus (k * align) % 4 bytes (an
    8-byte element: at an 8-byte boundary), so byte offsets 0, 1, 2, 3 (0 / 2 for 16-bit elements) all occur -> (tensor, pointers)"""
    import torch
    starts, cur = [], 0
    for k, p in enumerate(pieces):
        step = max(align, 4)
        cur = (cur + step - 1) // step * step + (k * align) % 4
        starts.append(cur)
        cur += p.size
    host = np.zeros(cur + 8, dtype=np.uint8)
    for s, p in zip(starts, pieces):
        host[s:s + p.size] = p
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 8 == 0
    return buf, [buf.data_ptr() + s for s in starts]


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def _dst(nsrc, n, prec):
    """sentinel-filled rows of n + 8 storage elements; result q starts q % 4 elements into its row -> (tensor, pointers, offsets)"""
    import torch
    t = torch.full((nsrc, n + 8), SENTINEL, dtype=torch.float64 if prec == "f64" else torch.float32, device="cuda")
    off = [q % 4 for q in range(nsrc)]
    return t, [t[q].data_ptr() + off[q] * t.element_size() for q in range(nsrc)], off


def _random_sources(rng, kind, prec, nsrc, npix, nz):
    """-> (byte images, their float64 values of shape (nsrc, npix * nz)); the extreme values of the kind are present"""
    n = npix * nz
    if kind == "U8":
        a = rng.integers(0, 256, (nsrc, n), dtype=np.uint8)
        if n >= 2:
            a[0, 0], a[0, -1] = 0, 255
        return [_bytes(x) for x in a], a.astype(np.float64)
    if kind == "U16":
        a = rng.integers(0, 65536, (nsrc, n), dtype=np.uint16)
        if n >= 2:
            a[0, 0], a[0, -1] = 0, 65535
        return [_bytes(x) for x in a], a.astype(np.float64)
    if kind == "RGB8":
        a = rng.integers(0, 256, (nsrc, npix, 3), dtype=np.uint8)
        if npix >= 2:
            a[0, 0], a[0, -1] = 0, 255
        return [_bytes(x) for x in a], _gray(a).astype(np.float64)
    dt = np.float32 if kind == "F32" or prec == "f32" else np.float64
    a = (rng.integers(0, 65536 * 8, (nsrc, n)) / 8.0 - 100.0).astype(dt)            # exact in float32, fractions and negatives
    return [_bytes(x) for x in a], a.astype(np.float64)


def _expected(vals, per, npix, nz, guard, prec):
    """numpy in float64: (255.0 * (x - lo)) / den per set and channel, the copy where den <= 0 under guard; rounded once to storage"""
    nsrc = vals.shape[0]
    out = np.empty_like(vals)
    for s in range(nsrc // per):
        x = vals[s * per:(s + 1) * per].reshape(per, npix, nz)
        lo, hi = x.min(axis=(0, 1)), x.max(axis=(0, 1))
        den = hi - lo
        with np.errstate(divide="ignore", invalid="ignore"):
            y = (255.0 * (x - lo)) / den
        if guard:
            y = np.where(den > 0, y, x)
        out[s * per:(s + 1) * per] = y.reshape(per, npix * nz)
    return out.astype(_np_storage(prec))


def _run_operator(ofx_mod, ctx, kind, prec, pieces, npix, nz, per, guard=1, vec=1, lut=1):
    nsrc, n = len(pieces), npix * nz
    keep, src = _carve(pieces, _align(kind, prec))
    t, dst, off = _dst(nsrc, n, prec)
    _set(ofx_mod, ctx, kind, vec, lut)
    try:
        ctx.normalize_frames_dev(src, dst, npix, nz=nz, per=per, guard=guard)
        ctx.synchronize()
    finally:
        _set(ofx_mod, ctx, "STORAGE")
    h = t.cpu().numpy()
    got = np.stack([h[q, off[q]:off[q] + n] for q in range(nsrc)])
    for q in range(nsrc):                                                           # nothing outside the npix * nz elements
        assert (h[q, :off[q]] == SENTINEL).all() and (h[q, off[q] + n:] == SENTINEL).all(), q
    return got


# npix: 1, 7, 8, 9 around a run; 3015 = 67 x 45, odd; 262 400 = 640 x 410, past the 1024 x 256 elements at which the min / max blocks stride
SHAPES = [(npix, nz, per) for npix in (1, 7, 8, 9, 3015) for nz in (1, 3) for per in (1, 2, 5)] + [(262400, 1, 2), (262400, 3, 5)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_operator_equals_numpy(ofx_mod, ctxs, kind, prec):
    rng = np.random.default_rng(14)
    ctx = ctxs[prec][0]
    for npix, nz, per in SHAPES:
        if kind == "RGB8" and nz != 1:
            continue
        nsrc = 2 * per                                                              # two sets
        pieces, vals = _random_sources(rng, kind, prec, nsrc, npix, nz)
        got = _run_operator(ofx_mod, ctx, kind, prec, pieces, npix, nz, per)
        assert np.array_equal(got, _expected(vals, per, npix, nz, 1, prec)), (npix, nz, per)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["U8", "U16", "RGB8"])
@pytest.mark.parametrize("path", ["one_per_thread", "no_lut"])
def test_operator_other_paths(ofx_mod, ctxs, path, kind, prec):
    """input_vec = 0, the plain kernels on the byte kinds, and input_lut = 0, a division per element instead of the LDS table of
    the 256 quotients: the same bits as the default path"""
    rng = np.random.default_rng(15)
    vec, lut = (0, 1) if path == "one_per_thread" else (1, 0)
    for npix, nz, per, guard in [(9, 1, 2, 1), (3015, 1, 5, 1), (3015, 3, 2, 1), (3015, 3, 2, 0), (262400, 1, 2, 1)]:
        if kind == "RGB8" and nz != 1:
            continue
        pieces, vals = _random_sources(rng, kind, prec, 2 * per, npix, nz)
        got = _run_operator(ofx_mod, ctxs[prec][0], kind, prec, pieces, npix, nz, per, guard=guard, vec=vec, lut=lut)
        assert np.array_equal(got, _expected(vals, per, npix, nz, guard, prec)), (npix, nz, per)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["U8", "U16", "F32", "RGB8"])
def test_constant_frames_are_copied_under_guard(ofx_mod, ctxs, kind, prec):
    """set 0 constant (max - min = 0: the copy of image_normalization_2), set 1 not; guard = 0 on a non-constant set is the map"""
    rng = np.random.default_rng(16)
    npix, nz, per = 3015, 1, 2
    pieces, vals = _random_sources(rng, kind, prec, 2 * per, npix, nz)
    const = {"U8": np.full(npix, 255, np.uint8), "U16": np.full(npix, 65535, np.uint16), "F32": np.full(npix, 3.5, np.float32),
             "RGB8": np.full((npix, 3), 200, np.uint8)}[kind]
    pieces[0] = pieces[1] = _bytes(const)
    vals[0] = vals[1] = _gray(const).astype(np.float64) if kind == "RGB8" else const.astype(np.float64)
    got = _run_operator(ofx_mod, ctxs[prec][0], kind, prec, pieces, npix, nz, per, guard=1)
    assert np.array_equal(got, _expected(vals, per, npix, nz, 1, prec))
    assert np.array_equal(got[0], vals[0].astype(_np_storage(prec)))                # the copy
    got = _run_operator(ofx_mod, ctxs[prec][0], kind, prec, pieces[2:], npix, nz, per, guard=0)
    assert np.array_equal(got, _expected(vals[2:], per, npix, nz, 0, prec))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_gray_rule(ofx_mod, ctxs, prec):
    """all 256 triples (v, v, v) -- where the truncation bites --, the eight corners of the cube and 4096 seeded random triples:
    RGB8 sources against U8 sources that hold the expected gray bytes"""
    rng = np.random.default_rng(17)
    v = np.arange(256, dtype=np.uint8)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.uint8)
    rgb = np.concatenate([np.stack([v, v, v], axis=1), corners, rng.integers(0, 256, (4096, 3), dtype=np.uint8)])
    gray = _gray(rgb)
    assert (gray[:256] != v).any()                                                  # .299 + .587 + .114 falls short of 1 somewhere
    npix = rgb.shape[0]
    ctx = ctxs[prec][0]
    for shift in (0, 1, 2, 3):                                                      # the same pixels at every source alignment
        a = _run_operator(ofx_mod, ctx, "RGB8", prec, [_bytes(rgb)] * (shift + 1), npix, 1, 1)[shift]
        b = _run_operator(ofx_mod, ctx, "U8", prec, [_bytes(gray)] * (shift + 1), npix, 1, 1)[shift]
        assert np.array_equal(a, b), shift
        assert np.array_equal(a, _expected(gray.astype(np.float64)[None], 1, npix, 1, 1, prec)[0]), shift


# ---- every ingestion site: "input" != 0 against "input" = 0 on the same values in the storage type -----------------------------
def _frames_u8(synth, n, nx=NX, ny=NY, k=1):
    f = synth.sequence(nx, ny, n, k)
    assert f.min() >= 0 and f.max() <= 255
    return f.astype(np.uint8)


def _as_kind(kind, u8):
    """frames of 8-bit values (n, ...) as sources of `kind` -> (byte images, the float64 values they stand for)"""
    if kind == "U8":
        return [_bytes(f) for f in u8], u8.astype(np.float64)
    if kind == "U16":
        a = u8.astype(np.uint16) * 257 + 3
        return [_bytes(f) for f in a], a.astype(np.float64)
    if kind == "F32":
        a = u8.astype(np.float32) + 0.25
        return [_bytes(f) for f in a], a.astype(np.float64)
    rgb = np.stack([u8, np.roll(u8, 5, axis=-1), 255 - u8], axis=-1)
    return [_bytes(f) for f in rgb], _gray(rgb).astype(np.float64)


def _both(ofx_mod, ctx, kind, prec, u8, call):
    """call(frame pointers) under `kind` on carved bytes, then under the storage type on the same values -> the two results"""
    import torch
    pieces, vals = _as_kind(kind, u8)
    keep, ptr = _carve(pieces, _align(kind, prec))
    _set(ofx_mod, ctx, kind)
    try:
        a = call(ptr)
    finally:
        _set(ofx_mod, ctx, "STORAGE")
    st = [torch.from_numpy(np.ascontiguousarray(v).astype(_np_storage(prec))).cuda() for v in vals]
    b = call([t.data_ptr() for t in st])
    return a, b


def _flo(n, nx, ny):
    import torch
    t = torch.full((n, ny, nx, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return t, [t[k].data_ptr() for k in range(n)]


def _tables(st):
    ns, nw = st.nscales, min(st.nsolves, 64)
    return ([st.iters[s][w] for s in range(ns) for w in range(nw)], [st.error[s][w] for s in range(ns) for w in range(nw)],
            st.work_pix_iters)


def _same(a, b, exact_errors=False):
    """payload bytes, iteration / sweep tables and work equal.  Stopping values: equal where the solver sums them in a fixed order
    (temporal Brox); the pair solvers add a wave's partial sums into 64 shards with atomics in no fixed order (loop_accumulate), so
    two runs of ONE call already differ in the last bits -- there to 1e-10 relative, the bound tests/test_gpu_tvl1.py uses against
    the oracle (n 2^-53 for the n <= 262 400 terms of these sizes is 3e-11)"""
    (flo_a, st_a), (flo_b, st_b) = a, b
    assert np.array_equal(flo_a.view(np.uint32), flo_b.view(np.uint32))             # payload BYTES
    assert np.isfinite(flo_a).all() and flo_a.any()
    for sa, sb in zip(st_a, st_b):
        (it_a, err_a, work_a), (it_b, err_b, work_b) = _tables(sa), _tables(sb)
        assert it_a == it_b and work_a == work_b
        assert err_a == err_b if exact_errors else np.allclose(err_a, err_b, rtol=1e-10, atol=0)
    assert len(st_a) == len(st_b) and sum(_tables(st_a[0])[0]) > 0                  # it iterated


def _pairs_call(ctx, fn, n_pairs, nx, ny, **kw):
    def call(ptr):
        flo, d_flo = _flo(n_pairs, nx, ny)
        st = fn(ptr[:n_pairs], ptr[1:n_pairs + 1], d_flo, nx, ny, **kw)
        ctx.synchronize()
        return flo.cpu().numpy(), st
    return call


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U8", "f32"), ("U16", "f64"), ("F32", "f64"), ("RGB8", "f64"), ("RGB8", "f32")])
def test_tvl1_group(ofx_mod, ctxs, synth, kind, prec):
    ctx = ctxs[prec][0]
    _same(*_both(ofx_mod, ctx, kind, prec, _frames_u8(synth, 4), _pairs_call(ctx, ctx.tvl1_group_dev, 3, NX, NY, nscales=2, warps=1)))


def test_tvl1_group_640x410(ofx_mod, ctxs, synth):
    ctx = ctxs["f64"][0]
    _same(*_both(ofx_mod, ctx, "U8", "f64", _frames_u8(synth, 3, 640, 410), _pairs_call(ctx, ctx.tvl1_group_dev, 2, 640, 410, nscales=2, warps=1)))


def test_tvl1_multiscale_dev(ofx_mod, ctxs, synth):
    ctx = ctxs["f64"][0]

    def call(ptr):
        flo, d_flo = _flo(1, NX, NY)
        ctx.tvl1_multiscale_dev(ptr[0], ptr[1], d_flo[0], NX, NY, nscales=2, warps=1)
        ctx.synchronize()
        return flo.cpu().numpy(), [ctx.stats()]
    _same(*_both(ofx_mod, ctx, "U8", "f64", _frames_u8(synth, 2), call))


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U8", "f32"), ("RGB8", "f64")])
def test_hs_group(ofx_mod, ctxs, synth, kind, prec):
    ctx = ctxs[prec][0]
    _same(*_both(ofx_mod, ctx, kind, prec, _frames_u8(synth, 3), _pairs_call(ctx, ctx.hs_group_dev, 2, NX, NY, nscales=2, warps=1, maxiter=8)))


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U16", "f64"), ("F32", "f64"), ("U8", "f32")])
def test_brox_group(ofx_mod, ctxs, synth, kind, prec):
    ctx = ctxs[prec][0]
    _same(*_both(ofx_mod, ctx, kind, prec, _frames_u8(synth, 3), _pairs_call(ctx, ctx.brox_group_dev, 2, NX, NY, nscales=2, inner=1, outer=2)))


def _colour_u8(synth, n):
    f = _frames_u8(synth, n).astype(np.int32)
    return np.stack([f, (153 - 3 * f // 5) + 20, f * f // 255], axis=-1).astype(np.uint8)      # (n, ny, nx, 3), HWC


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_robust_expo_group_interleaved_u8(ofx_mod, ctxs, synth, prec):
    """nzz = 3: an HWC uint8 image is the interleaved layout as it stands"""
    ctx = ctxs[prec][0]
    call = _pairs_call(ctx, ctx.robust_expo_group_dev, 2, NX, NY, nz=3, nscales=2, inner=1, outer=2)
    _same(*_both(ofx_mod, ctx, "U8", prec, _colour_u8(synth, 3), call))


def test_robust_expo_group_rgb8_one_channel(ofx_mod, ctxs, synth):
    ctx = ctxs["f64"][0]
    call = _pairs_call(ctx, ctx.robust_expo_group_dev, 2, NX, NY, nz=1, nscales=2, inner=1, outer=2)
    _same(*_both(ofx_mod, ctx, "RGB8", "f64", _frames_u8(synth, 3), call))


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U16", "f32"), ("RGB8", "f64"), ("F32", "f64")])
def test_brox_temporal_group(ofx_mod, ctxs, synth, kind, prec):
    """2 sequences x 3 frames"""
    ctx = ctxs[prec][0]
    u8 = np.concatenate([_frames_u8(synth, 3, k=1), _frames_u8(synth, 3, k=2)])

    def call(ptr):
        flo, d_flo = _flo(4, NX, NY)
        st = ctx.brox_temporal_group_dev(ptr, d_flo, NX, NY, 3, nscales=2, inner=1, outer=2)
        ctx.synchronize()
        return flo.cpu().numpy(), st
    _same(*_both(ofx_mod, ctx, kind, prec, u8, call), exact_errors=True)


def test_brox_temporal_dev(ofx_mod, ctxs, synth):
    """one sequence of 4 frames through ofx_brox_temporal_dev"""
    ctx = ctxs["f64"][0]

    def call(ptr):
        flo, d_flo = _flo(3, NX, NY)
        ctx.brox_temporal_dev(ptr, d_flo, NX, NY, nscales=2, inner=1, outer=2)
        ctx.synchronize()
        return flo.cpu().numpy(), [ctx.stats()]
    _same(*_both(ofx_mod, ctx, "U8", "f64", _frames_u8(synth, 4), call), exact_errors=True)


def _occ_same(a, b):
    (flo_a, occ_a, st_a), (flo_b, occ_b, st_b) = a, b
    assert np.array_equal(flo_a.view(np.uint32), flo_b.view(np.uint32))
    assert np.array_equal(occ_a, occ_b)
    assert flo_a.any() and set(np.unique(occ_a)) <= {0, 255}
    assert [_tables(s) for s in st_a] == [_tables(s) for s in st_b]


def _occ_results(n):
    import torch
    flo, d_flo = _flo(n, NX, NY)
    occ = torch.full((n, NX * NY), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return flo, d_flo, occ, [occ[k].data_ptr() for k in range(n)]


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U16", "f64"), ("F32", "f64"), ("RGB8", "f64"), ("U8", "f32")])
def test_tvl1occ_sequence(ofx_mod, ctxs, synth, kind, prec):
    """5 frames, 3 triples"""
    ctx = ctxs[prec][0]

    def call(ptr):
        flo, d_flo, occ, d_occ = _occ_results(3)
        st = ctx.tvl1occ_sequence_group_dev(ptr, d_flo, d_occ, NX, NY, nscales=2, warps=1)
        ctx.synchronize()
        return flo.cpu().numpy(), occ.cpu().numpy(), st
    _occ_same(*_both(ofx_mod, ctx, kind, prec, _frames_u8(synth, 5), call))


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("RGB8", "f64"), ("U16", "f32")])
def test_tvl1occ_triples(ofx_mod, ctxs, synth, kind, prec):
    ctx = ctxs[prec][0]
    triples = [(0, 1, 2), (2, 1, 0), (0, 2, 4, 3)]

    def call(ptr):
        flo, d_flo, occ, d_occ = _occ_results(3)
        st = ctx.tvl1occ_triples_group_dev(ptr, triples, d_flo, d_occ, NX, NY, nscales=2, warps=1)
        ctx.synchronize()
        return flo.cpu().numpy(), occ.cpu().numpy(), st
    _occ_same(*_both(ofx_mod, ctx, kind, prec, _frames_u8(synth, 5), call))


def test_tvl1occ_sequence_dev_two_contexts(ofx_mod, ctxs, synth):
    """the multi-context entry under U8 on both contexts against the group entry under the storage type"""
    c0, c1 = ctxs["f64"]
    u8 = _frames_u8(synth, 5)

    def batch(ptr):
        flo, d_flo, occ, d_occ = _occ_results(3)
        ofx_mod.tvl1occ_sequence_dev([c0, c1], ptr, d_flo, d_occ, NX, NY, nscales=2, warps=1)
        return flo.cpu().numpy(), occ.cpu().numpy()

    def group(ptr):
        flo, d_flo, occ, d_occ = _occ_results(3)
        c0.tvl1occ_sequence_group_dev(ptr, d_flo, d_occ, NX, NY, nscales=2, warps=1)
        c0.synchronize()
        return flo.cpu().numpy(), occ.cpu().numpy()
    import torch
    keep, ptr = _carve(_as_kind("U8", u8)[0], 1)
    _set(ofx_mod, c0, "U8")
    _set(ofx_mod, c1, "U8")
    try:
        a = batch(ptr)
    finally:
        _set(ofx_mod, c0, "STORAGE")
        _set(ofx_mod, c1, "STORAGE")
    st = [torch.from_numpy(f.astype(np.float64)).cuda() for f in u8]
    b = group([t.data_ptr() for t in st])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


# ---- batch entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "pinned"])
def test_tvl1_batch_two_contexts_u8(ofx_mod, ctxs, synth, where):
    """U8 frames in device memory, and in pinned host memory (staged: the copies are sized by the source element), against the
    group entry on doubles"""
    import torch
    c0, c1 = ctxs["f64"]
    u8 = _frames_u8(synth, 4)
    kw = dict(nscales=2, warps=1)
    st = [torch.from_numpy(f.astype(np.float64)).cuda() for f in u8]
    flo_g, d_flo = _flo(3, NX, NY)
    c0.tvl1_group_dev([t.data_ptr() for t in st[:3]], [t.data_ptr() for t in st[1:]], d_flo, NX, NY, **kw)
    c0.synchronize()
    if where == "device":
        keep, ptr = _carve([_bytes(f) for f in u8], 1)
    else:
        keep = [torch.from_numpy(np.ascontiguousarray(f)).pin_memory() for f in u8]
        ptr = [t.data_ptr() for t in keep]
    flo_b, d_flo = _flo(3, NX, NY)
    _set(ofx_mod, c0, "U8")
    _set(ofx_mod, c1, "U8")
    try:
        work = ofx_mod.tvl1_batch_dev([c0, c1], ptr[:3], ptr[1:], d_flo, NX, NY, **kw)
    finally:
        _set(ofx_mod, c0, "STORAGE")
        _set(ofx_mod, c1, "STORAGE")
    torch.cuda.synchronize()
    assert np.array_equal(flo_b.cpu().numpy().view(np.uint32), flo_g.cpu().numpy().view(np.uint32))
    assert all(w > 0 for w in work)


def test_batches_refuse_mixed_input_kinds(ofx_mod, ctxs, synth):
    import torch
    c0, c1 = ctxs["f64"]
    keep, ptr = _carve([_bytes(f) for f in _frames_u8(synth, 5)], 1)
    flo, d_flo, occ, d_occ = _occ_results(3)
    _set(ofx_mod, c0, "U8")
    try:
        for fn in (lambda: ofx_mod.tvl1_batch_dev([c0, c1], ptr[:3], ptr[1:4], d_flo, NX, NY, nscales=2, warps=1),
                   lambda: ofx_mod.hs_batch_dev([c0, c1], ptr[:3], ptr[1:4], d_flo, NX, NY, nscales=2, warps=1, maxiter=8),
                   lambda: ofx_mod.brox_batch_dev([c0, c1], ptr[:3], ptr[1:4], d_flo, NX, NY, nscales=2, inner=1, outer=2),
                   lambda: ofx_mod.robust_expo_batch_dev([c0, c1], ptr[:3], ptr[1:4], d_flo, NX, NY, 1, nscales=2, inner=1, outer=2),
                   lambda: ofx_mod.brox_temporal_batch_dev([c0, c1], ptr[:3], d_flo[:2], NX, NY, 3, nscales=2, inner=1, outer=2),
                   lambda: ofx_mod.tvl1occ_sequence_dev([c0, c1], ptr, d_flo, d_occ, NX, NY, nscales=2, warps=1),
                   lambda: ofx_mod.tvl1occ_triples_dev([c0, c1], ptr, [(0, 1, 2), (1, 2, 3), (2, 3, 4)], d_flo, d_occ, NX, NY, nscales=2,
                                                       warps=1)):
            with pytest.raises(ofx_mod.OfxError) as e:
                fn()
            assert e.value.status == ERR_ARG
    finally:
        _set(ofx_mod, c0, "STORAGE")
    torch.cuda.synchronize()
    assert bool((flo == SENTINEL).all().item()) and bool((occ == 7).all().item())


# ---- errors, each with no output written -----------------------------------------------------------------------------------------
def test_bad_option_values(ofx_mod, ctxs):
    ctx = ctxs["f64"][0]
    for bad in (-1, 5, 1.5, 255):
        with pytest.raises(ofx_mod.OfxError) as e:
            ctx.set_option("input", bad)
        assert e.value.status == ERR_ARG
    assert (ofx_mod.IN_STORAGE, ofx_mod.IN_U8, ofx_mod.IN_U16, ofx_mod.IN_F32, ofx_mod.IN_RGB8) == (0, 1, 2, 3, 4)
    for ok in (4, 3, 2, 1, 0):
        ctx.set_option("input", ok)


def test_rgb8_refuses_interleaved_channels(ofx_mod, ctxs, synth):
    import torch
    ctx = ctxs["f64"][0]
    keep, ptr = _carve([_bytes(f) for f in _colour_u8(synth, 2)], 1)
    flo, d_flo = _flo(1, NX, NY)
    t, dst, off = _dst(1, NX * NY * 3, "f64")
    _set(ofx_mod, ctx, "RGB8")
    try:
        with pytest.raises(ofx_mod.OfxError) as e:
            ctx.robust_expo_group_dev(ptr[:1], ptr[1:], d_flo, NX, NY, 3, nscales=2, inner=1, outer=2)
        assert e.value.status == ERR_ARG
        with pytest.raises(ofx_mod.OfxError) as e:                                  # the operator: nz != 1
            ctx.normalize_frames_dev(ptr[:1], dst, NX * NY, nz=3)
        assert e.value.status == ERR_ARG
    finally:
        _set(ofx_mod, ctx, "STORAGE")
    torch.cuda.synchronize()
    assert bool((flo == SENTINEL).all().item()) and bool((t == SENTINEL).all().item())


def test_operator_refuses_more_than_32_sources(ofx_mod, ctxs):
    import torch
    ctx = ctxs["f64"][0]
    keep, ptr = _carve([np.arange(16, dtype=np.uint8)] * 33, 1)
    t, dst, off = _dst(33, 16, "f64")
    _set(ofx_mod, ctx, "U8")
    try:
        for per in (33, 11, 1):                                                     # 1 x 33, 3 x 11, 33 x 1
            with pytest.raises(ofx_mod.OfxError) as e:
                ctx.normalize_frames_dev(ptr, dst, 16, per=per)
            assert e.value.status == ERR_ARG
        ctx.normalize_frames_dev(ptr[:32], dst[:32], 16, per=16)                     # 32 is served
        ctx.synchronize()
    finally:
        _set(ofx_mod, ctx, "STORAGE")
    h = t.cpu().numpy()
    assert (h[32] == SENTINEL).all()
    assert np.array_equal(h[5, off[5]:off[5] + 16], 17.0 * np.arange(16))           # 255 x / 15
