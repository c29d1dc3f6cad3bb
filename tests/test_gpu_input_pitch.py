"""Context option "input_pitch": frames whose rows are a pitch apart -- decoder surfaces, crops, torch slices -- straight into the
device-resident entries.

The contract is bit identity.  ofx_normalize_frames2d_dev against numpy in float64 on the rows' values (the arithmetic of
tests/test_gpu_input_kinds.py), over row lengths around a 32-bit word and a group of four, pitches that rotate a row's alignment,
base pointers at every byte offset, with the padding between the rows POISONED: integer samples lie in 1 .. max - 1 with both ends
of that range placed where a row kernel could lose them (the head element of a middle row, the tail element of the last row) and
the padding holds 0 and the type's maximum, float padding is NaN.  Then every *_dev solver family on regions of interest of
poisoned parents against the same call on dense copies."""
import numpy as np
import pytest

from test_gpu_input_kinds import (ERR_ARG, NX, NY, SENTINEL, _bytes, _carve, _colour_u8, _dst, _expected, _flo, _frames_u8, _gray,
                                  _np_storage, _occ_results, _occ_same, _same, _set)

pytestmark = pytest.mark.gpu

KINDS = ("STORAGE", "U8", "U16", "F32", "RGB8")
# row lengths around one word / one group of four, rows 1, 2, 5; 67 x 5; 1031 x 3: a row of more than one tile of groups
SIZES = [(nx, ny) for nx in (1, 2, 3, 4, 5, 7, 8, 9, 13) for ny in (1, 2, 5)] + [(67, 5), (1031, 3)]
EXTRA = (0, 1, 2, 3, 5)                             # pitch = the row's bytes + this many units of the element's alignment
PX, PY, X0, Y0 = 96, 64, 5, 3                       # parents of the regions of interest, and where the regions start


@pytest.fixture(scope="module")
def ctxs(ofx_mod):
    """contexts of this module alone (the options must not leak into the session's): two per storage precision"""
    c = {"f64": [ofx_mod.Ofx(0, ofx_mod.F64) for _ in range(2)], "f32": [ofx_mod.Ofx(0, ofx_mod.F32) for _ in range(2)]}
    yield c
    for v in c.values():
        for x in v:
            x.close()


def _elem(kind, prec):
    """(numpy type of an element, elements per pixel, alignment = the pitch's unit)"""
    if kind == "U8":
        return np.uint8, 1, 1
    if kind == "U16":
        return np.uint16, 1, 2
    if kind == "RGB8":
        return np.uint8, 3, 1
    dt = np.float32 if kind == "F32" or prec == "f32" else np.float64
    return dt, 1, np.dtype(dt).itemsize


def _poison(kind, prec, nbytes):
    """nbytes of padding: runs of 0 and of the type's maximum for the integer kinds, NaN for the float kinds"""
    dt, _, _ = _elem(kind, prec)
    if np.issubdtype(dt, np.floating):
        return np.full(nbytes // np.dtype(dt).itemsize + 1, np.nan, dtype=dt).view(np.uint8)[:nbytes].copy()
    return np.where((np.arange(nbytes) // 6) % 2, 255, 0).astype(np.uint8)


def _samples(rng, kind, prec, nsrc, ny, w):
    """nsrc frames of ny rows of w elements (RGB8: pixels) -> (arrays (ny, w[, 3]) of the element type, float64 values (nsrc, ny * w)).
    Integer kinds: samples strictly inside the range whose two ends sit at the head of a middle row and the tail of the last row"""
    dt, epp, _ = _elem(kind, prec)
    if kind in ("U8", "U16"):
        top = 255 if kind == "U8" else 65535
        a = rng.integers(2, top - 1, (nsrc, ny, w)).astype(dt)
        a[0, ny // 2, 0] = 1
        a[-1, ny - 1, w - 1] = top - 1
        return list(a), a.reshape(nsrc, -1).astype(np.float64)
    if kind == "RGB8":
        a = rng.integers(8, 248, (nsrc, ny, w, 3)).astype(np.uint8)
        a[0, ny // 2, 0] = 2
        a[-1, ny - 1, w - 1] = 253
        return list(a), _gray(a).reshape(nsrc, -1).astype(np.float64)
    a = (rng.integers(0, 65536 * 8, (nsrc, ny, w)) / 8.0 - 100.0).astype(dt)        # exact in float32, fractions and negatives
    return list(a), a.reshape(nsrc, -1).astype(np.float64)


def _lay_out(kind, prec, frames, pitch):
    """one device byte buffer of poison holding the frames with `pitch` bytes between their rows; frame k starts at a 4-byte boundary
    plus (k * alignment) % 4 bytes (an 8-byte element: at an 8-byte boundary), and the buffer ends with the last row of the last
    frame: there is no padding after it -> (tensor, pointers)"""
    import torch
    _, _, align = _elem(kind, prec)
    rows = [np.ascontiguousarray(f).view(np.uint8).reshape(f.shape[0], -1) for f in frames]
    starts, cur = [], 0
    for k, r in enumerate(rows):
        step = max(align, 4)
        cur = (cur + step - 1) // step * step + (k * align) % 4
        starts.append(cur)
        cur += (r.shape[0] - 1) * pitch + r.shape[1]
    host = _poison(kind, prec, cur)
    for s, r in zip(starts, rows):
        for i in range(r.shape[0]):
            host[s + i * pitch:s + i * pitch + r.shape[1]] = r[i]
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 8 == 0
    return buf, [buf.data_ptr() + s for s in starts]


def _call2d(ofx_mod, ctx, kind, prec, src, nsrc, nx, ny, nz, per, guard, pitch, vec=1, lut=1, flat=False):
    """one call into sentinel-guarded destinations -> the results (nsrc, nx * ny * nz)"""
    n = nx * ny * nz
    t, dst, off = _dst(nsrc, n, prec)
    _set(ofx_mod, ctx, kind, vec, lut)
    ctx.set_option("input_pitch", pitch)
    try:
        if flat:
            ctx.normalize_frames_dev(src, dst, nx * ny, nz=nz, per=per, guard=guard)
        else:
            ctx.normalize_frames2d_dev(src, dst, nx, ny, nz=nz, per=per, guard=guard)
        ctx.synchronize()
    finally:
        ctx.set_option("input_pitch", 0)
        _set(ofx_mod, ctx, "STORAGE")
    h = t.cpu().numpy()
    for q in range(nsrc):                                                           # nothing outside the nx * ny * nz elements
        assert (h[q, :off[q]] == SENTINEL).all() and (h[q, off[q] + n:] == SENTINEL).all(), q
    return np.stack([h[q, off[q]:off[q] + n] for q in range(nsrc)])


def _modes(kind):
    """(input_vec, input_lut) settings that select different kernels for the kind"""
    if kind in ("U8", "RGB8"):
        return [(1, 1), (1, 0), (0, 1)]
    return [(1, 1), (0, 1)] if kind == "U16" else [(1, 1)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_operator_equals_numpy(ofx_mod, ctxs, kind, prec):
    """four sources at the byte offsets 0 .. 3 (0 / 2 for 16-bit elements) per call; every size, pitch, channel count, set size,
    guard and kernel selection"""
    rng = np.random.default_rng(31)
    ctx = ctxs[prec][0]
    _, epp, align = _elem(kind, prec)
    esz = np.dtype(_elem(kind, prec)[0]).itemsize * epp
    nsrc = 4
    for nx, ny in SIZES:
        for nz in ((1,) if kind == "RGB8" else (1, 3)):
            frames, vals = _samples(rng, kind, prec, nsrc, ny, nx * nz)
            want = {(per, guard): _expected(vals, per, nx * ny, nz, guard, prec) for per in (1, 2) for guard in (0, 1)}
            for extra in EXTRA:
                pitch = nx * nz * esz + extra * align
                keep, src = _lay_out(kind, prec, frames, pitch)
                for vec, lut in _modes(kind):
                    for (per, guard), exp in want.items():
                        got = _call2d(ofx_mod, ctx, kind, prec, src, nsrc, nx, ny, nz, per, guard, pitch, vec, lut)
                        assert np.array_equal(got, exp, equal_nan=True), (nx, ny, nz, extra, vec, lut, per, guard)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_pitch_0_is_the_flat_entry_and_row_bytes_is_pitch_0(ofx_mod, ctxs, kind, prec):
    rng = np.random.default_rng(32)
    ctx = ctxs[prec][0]
    _, epp, _ = _elem(kind, prec)
    esz = np.dtype(_elem(kind, prec)[0]).itemsize * epp
    for nx, ny, nz in [(13, 5, 1), (67, 45, 1), (67, 5, 3), (1031, 3, 1)]:
        if kind == "RGB8" and nz != 1:
            continue
        frames, vals = _samples(rng, kind, prec, 4, ny, nx * nz)
        keep, src = _lay_out(kind, prec, frames, nx * nz * esz)                     # dense
        flat = _call2d(ofx_mod, ctx, kind, prec, src, 4, nx, ny, nz, 2, 1, 0, flat=True)
        assert np.array_equal(flat, _expected(vals, 2, nx * ny, nz, 1, prec)), (nx, ny, nz)
        for pitch in (0, nx * nz * esz):
            got = _call2d(ofx_mod, ctx, kind, prec, src, 4, nx, ny, nz, 2, 1, pitch)
            assert got.tobytes() == flat.tobytes(), (nx, ny, nz, pitch)


# ---- every family: regions of interest of poisoned parents against dense copies of the same values -----------------------------
def _as_kind(kind, prec, u8):
    """frames of 8-bit values (n, ny, nx[, c]) as elements of `kind` (the samples of tests/test_gpu_input_kinds.py)"""
    if kind == "U8":
        return u8
    if kind == "U16":
        return u8.astype(np.uint16) * 257 + 3
    return (u8.astype(np.float32) + 0.25).astype(_np_storage(prec))                 # STORAGE


def _regions(kind, prec, frames):
    """every frame (ny, nx[, c]) as the region at (X0, Y0) of a PX x PY parent of its own whose other pixels are poison
    -> (tensor, pointers, pitch)"""
    import torch
    ny, nx = frames[0].shape[:2]
    c = frames[0].shape[2] if frames[0].ndim == 3 else 1
    esz = frames[0].dtype.itemsize
    pitch = PX * c * esz
    parent_bytes = PY * pitch
    host = _poison(kind, prec, parent_bytes * len(frames))
    for k, f in enumerate(frames):
        rows = np.ascontiguousarray(f).view(np.uint8).reshape(ny, -1)
        for i in range(ny):
            o = k * parent_bytes + (Y0 + i) * pitch + X0 * c * esz
            host[o:o + rows.shape[1]] = rows[i]
    buf = torch.from_numpy(host).cuda()
    return buf, [buf.data_ptr() + k * parent_bytes + Y0 * pitch + X0 * c * esz for k in range(len(frames))], pitch


def _both(ofx_mod, cs, kind, prec, frames, call):
    """call(frame pointers) on regions of interest under their parents' pitch, then on dense copies under pitch 0, all contexts
    `cs` under the same options -> the two results"""
    align = {"U8": 1, "U16": 2, "STORAGE": 8 if prec == "f64" else 4}[kind]
    keep_p, ptr_p, pitch = _regions(kind, prec, frames)
    keep_d, ptr_d = _carve([_bytes(f) for f in frames], align)
    out = []
    for ptr, p in ((ptr_p, pitch), (ptr_d, 0)):
        for c in cs:
            _set(ofx_mod, c, kind)
            c.set_option("input_pitch", p)
        try:
            out.append(call(ptr))
        finally:
            for c in cs:
                c.set_option("input_pitch", 0)
                _set(ofx_mod, c, "STORAGE")
    return out


def _pairs_call(ctx, fn, n_pairs, **kw):
    def call(ptr):
        flo, d_flo = _flo(n_pairs, NX, NY)
        st = fn(ptr[:n_pairs], ptr[1:n_pairs + 1], d_flo, NX, NY, **kw)
        ctx.synchronize()
        return flo.cpu().numpy(), st
    return call


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U8", "f32"), ("STORAGE", "f64"), ("U16", "f32")])
def test_tvl1_group(ofx_mod, ctxs, synth, kind, prec):
    ctx = ctxs[prec][0]
    frames = list(_as_kind(kind, prec, _frames_u8(synth, 4)))
    _same(*_both(ofx_mod, [ctx], kind, prec, frames, _pairs_call(ctx, ctx.tvl1_group_dev, 3, nscales=2, warps=1)))


def test_tvl1_multiscale_dev(ofx_mod, ctxs, synth):
    ctx = ctxs["f64"][0]

    def call(ptr):
        flo, d_flo = _flo(1, NX, NY)
        ctx.tvl1_multiscale_dev(ptr[0], ptr[1], d_flo[0], NX, NY, nscales=2, warps=1)
        ctx.synchronize()
        return flo.cpu().numpy(), [ctx.stats()]
    _same(*_both(ofx_mod, [ctx], "U8", "f64", list(_frames_u8(synth, 2)), call))


def test_tvl1_batch_two_contexts(ofx_mod, ctxs, synth):
    import torch
    cs = ctxs["f64"]

    def call(ptr):
        flo, d_flo = _flo(3, NX, NY)
        work = ofx_mod.tvl1_batch_dev(cs, ptr[:3], ptr[1:4], d_flo, NX, NY, nscales=2, warps=1)
        torch.cuda.synchronize()
        return flo.cpu().numpy(), work
    (flo_a, work_a), (flo_b, work_b) = _both(ofx_mod, cs, "U8", "f64", list(_frames_u8(synth, 4)), call)
    assert np.array_equal(flo_a.view(np.uint32), flo_b.view(np.uint32)) and flo_a.any()
    assert list(work_a) == list(work_b) and all(w > 0 for w in work_a)


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U16", "f64")])
def test_hs_group(ofx_mod, ctxs, synth, kind, prec):
    ctx = ctxs[prec][0]
    frames = list(_as_kind(kind, prec, _frames_u8(synth, 3)))
    _same(*_both(ofx_mod, [ctx], kind, prec, frames, _pairs_call(ctx, ctx.hs_group_dev, 2, nscales=2, warps=1, maxiter=8)))


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("STORAGE", "f32")])
def test_brox_group(ofx_mod, ctxs, synth, kind, prec):
    ctx = ctxs[prec][0]
    frames = list(_as_kind(kind, prec, _frames_u8(synth, 3)))
    _same(*_both(ofx_mod, [ctx], kind, prec, frames, _pairs_call(ctx, ctx.brox_group_dev, 2, nscales=2, inner=1, outer=2)))


def test_hs_batch_two_contexts(ofx_mod, ctxs, synth):
    import torch
    cs = ctxs["f64"]

    def call(ptr):
        flo, d_flo = _flo(3, NX, NY)
        work = ofx_mod.hs_batch_dev(cs, ptr[:3], ptr[1:4], d_flo, NX, NY, nscales=2, warps=1, maxiter=8)
        torch.cuda.synchronize()
        return flo.cpu().numpy(), work
    (flo_a, work_a), (flo_b, work_b) = _both(ofx_mod, cs, "U8", "f64", list(_frames_u8(synth, 4)), call)
    assert np.array_equal(flo_a.view(np.uint32), flo_b.view(np.uint32)) and flo_a.any()
    assert list(work_a) == list(work_b) and all(w > 0 for w in work_a)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_robust_expo_group_interleaved_u8(ofx_mod, ctxs, synth, prec):
    """nzz = 3: a row is 67 pixels of three interleaved bytes, the parent's pitch 96 * 3"""
    ctx = ctxs[prec][0]
    call = _pairs_call(ctx, ctx.robust_expo_group_dev, 2, nz=3, nscales=2, inner=1, outer=2)
    _same(*_both(ofx_mod, [ctx], "U8", prec, list(_colour_u8(synth, 3)), call))


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U16", "f32")])
def test_brox_temporal_group(ofx_mod, ctxs, synth, kind, prec):
    """2 sequences x 3 frames"""
    ctx = ctxs[prec][0]
    u8 = np.concatenate([_frames_u8(synth, 3, k=1), _frames_u8(synth, 3, k=2)])

    def call(ptr):
        flo, d_flo = _flo(4, NX, NY)
        st = ctx.brox_temporal_group_dev(ptr, d_flo, NX, NY, 3, nscales=2, inner=1, outer=2)
        ctx.synchronize()
        return flo.cpu().numpy(), st
    _same(*_both(ofx_mod, [ctx], kind, prec, list(_as_kind(kind, prec, u8)), call), exact_errors=True)


def test_brox_temporal_dev(ofx_mod, ctxs, synth):
    ctx = ctxs["f64"][0]

    def call(ptr):
        flo, d_flo = _flo(3, NX, NY)
        ctx.brox_temporal_dev(ptr, d_flo, NX, NY, nscales=2, inner=1, outer=2)
        ctx.synchronize()
        return flo.cpu().numpy(), [ctx.stats()]
    _same(*_both(ofx_mod, [ctx], "U8", "f64", list(_frames_u8(synth, 4)), call), exact_errors=True)


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("STORAGE", "f64"), ("STORAGE", "f32"), ("U16", "f64")])
def test_tvl1occ_sequence(ofx_mod, ctxs, synth, kind, prec):
    """5 frames, 3 triples; STORAGE under f64 / f32 are the two instances of the pitched k_occ_seq_in"""
    ctx = ctxs[prec][0]

    def call(ptr):
        flo, d_flo, occ, d_occ = _occ_results(3)
        st = ctx.tvl1occ_sequence_group_dev(ptr, d_flo, d_occ, NX, NY, nscales=2, warps=1)
        ctx.synchronize()
        return flo.cpu().numpy(), occ.cpu().numpy(), st
    _occ_same(*_both(ofx_mod, [ctx], kind, prec, list(_as_kind(kind, prec, _frames_u8(synth, 5))), call))


def test_tvl1occ_triples(ofx_mod, ctxs, synth):
    ctx = ctxs["f64"][0]
    triples = [(0, 1, 2), (2, 1, 0), (0, 2, 4, 3)]

    def call(ptr):
        flo, d_flo, occ, d_occ = _occ_results(3)
        st = ctx.tvl1occ_triples_group_dev(ptr, triples, d_flo, d_occ, NX, NY, nscales=2, warps=1)
        ctx.synchronize()
        return flo.cpu().numpy(), occ.cpu().numpy(), st
    _occ_same(*_both(ofx_mod, [ctx], "U8", "f64", list(_frames_u8(synth, 5)), call))


@pytest.mark.parametrize("kind,prec", [("U8", "f64"), ("U8", "f32"), ("STORAGE", "f64")])
def test_pyramid_group(ofx_mod, ctxs, synth, kind, prec):
    """every level of both images of both pairs"""
    ctx = ctxs[prec][0]

    def call(ptr):
        return ctx.pyramid_group_dev(ptr[:2], ptr[1:3], NX, NY, nscales=3)
    (a0, a1, ga), (b0, b1, gb) = _both(ofx_mod, [ctx], kind, prec, list(_as_kind(kind, prec, _frames_u8(synth, 3))), call)
    for s in range(3):
        assert np.array_equal(a0[s], b0[s]) and np.array_equal(a1[s], b1[s]), s
        assert np.isfinite(a0[s]).all() and a0[s].any()
    assert (ga == ctx.PYRAMID_SENTINEL).all() and (gb == ctx.PYRAMID_SENTINEL).all()


# ---- errors, each with no output written -----------------------------------------------------------------------------------------
def test_bad_option_values_leave_the_option(ofx_mod, ctxs, synth):
    import torch
    ctx = ctxs["f64"][0]
    frames = list(_frames_u8(synth, 2))
    keep, ptr, pitch = _regions("U8", "f64", frames)
    _set(ofx_mod, ctx, "U8")
    ctx.set_option("input_pitch", pitch)
    try:
        for bad in (-1, -96.0, 96.5, 0.25, 2.0 ** 31, float("nan")):
            with pytest.raises(ofx_mod.OfxError) as e:
                ctx.set_option("input_pitch", bad)
            assert e.value.status == ERR_ARG
        # the option is unchanged: the regions are still read under their parents' pitch
        got = _call_keep_pitch(ofx_mod, ctx, ptr, pitch)
        assert np.array_equal(got, _expected(np.stack([f.ravel() for f in frames]).astype(np.float64), 2, NX * NY, 1, 1, "f64"))
    finally:
        ctx.set_option("input_pitch", 0)
        _set(ofx_mod, ctx, "STORAGE")
    torch.cuda.synchronize()


def _call_keep_pitch(ofx_mod, ctx, ptr, pitch):
    """ofx_normalize_frames2d_dev under whatever options the context holds"""
    t, dst, off = _dst(2, NX * NY, "f64")
    ctx.normalize_frames2d_dev(ptr, dst, NX, NY)
    ctx.synchronize()
    h = t.cpu().numpy()
    return np.stack([h[q, off[q]:off[q] + NX * NY] for q in range(2)])


def test_refused_pitches_write_nothing(ofx_mod, ctxs, synth):
    """below the row's bytes and off the element's alignment, at the operator and at a solver of every family"""
    import torch
    for kind, prec, bad in [("U8", "f64", [NX - 1, 1]), ("U16", "f64", [2 * NX - 2, 2 * NX + 1, 2 * PX + 1]),
                            ("STORAGE", "f64", [8 * NX - 8, 8 * NX + 4, 8 * PX + 4]), ("STORAGE", "f32", [4 * NX - 4, 4 * NX + 2, 4 * PX + 2]),
                            ("F32", "f64", [4 * NX + 2])]:
        ctx = ctxs[prec][0]
        src = _as_kind("STORAGE" if kind == "F32" else kind, "f32" if kind == "F32" else prec, _frames_u8(synth, 5))
        keep, ptr, _ = _regions(kind, prec, list(src))
        flo, d_flo, occ, d_occ = _occ_results(4)
        t, dst, off = _dst(2, NX * NY, prec)
        calls = [lambda: ctx.normalize_frames2d_dev(ptr[:2], dst, NX, NY),
                 lambda: ctx.tvl1_multiscale_dev(ptr[0], ptr[1], d_flo[0], NX, NY, nscales=2, warps=1),
                 lambda: ctx.tvl1_group_dev(ptr[:2], ptr[1:3], d_flo[:2], NX, NY, nscales=2, warps=1),
                 lambda: ctx.hs_group_dev(ptr[:2], ptr[1:3], d_flo[:2], NX, NY, nscales=2, warps=1, maxiter=8),
                 lambda: ctx.brox_group_dev(ptr[:2], ptr[1:3], d_flo[:2], NX, NY, nscales=2, inner=1, outer=2),
                 lambda: ctx.robust_expo_group_dev(ptr[:2], ptr[1:3], d_flo[:2], NX, NY, 1, nscales=2, inner=1, outer=2),
                 lambda: ctx.brox_temporal_dev(ptr[:3], d_flo[:2], NX, NY, nscales=2, inner=1, outer=2),
                 lambda: ctx.brox_temporal_group_dev(ptr[:3], d_flo[:2], NX, NY, 3, nscales=2, inner=1, outer=2),
                 lambda: ctx.tvl1occ_sequence_group_dev(ptr, d_flo[:3], d_occ[:3], NX, NY, nscales=2, warps=1),
                 lambda: ctx.tvl1occ_triples_group_dev(ptr, [(0, 1, 2)], d_flo[:1], d_occ[:1], NX, NY, nscales=2, warps=1)]
        _set(ofx_mod, ctx, kind)
        try:
            for pitch in bad:
                ctx.set_option("input_pitch", pitch)
                for k, fn in enumerate(calls):
                    with pytest.raises(ofx_mod.OfxError) as e:
                        fn()
                    assert e.value.status == ERR_ARG, (kind, pitch, k)
                    assert str(pitch) in str(e.value) and "row" in str(e.value), (kind, pitch, k, str(e.value))
                try:                                                                 # pyramid_group_dev hands its outputs over
                    ctx.pyramid_group_dev(ptr[:1], ptr[1:2], NX, NY, nscales=2)
                    assert False, (kind, pitch)
                except ofx_mod.OfxError as e:
                    assert e.status == ERR_ARG
                    assert all((lv == ctx.PYRAMID_SENTINEL).all() for im in e.outputs[:2] for lv in im)
        finally:
            ctx.set_option("input_pitch", 0)
            _set(ofx_mod, ctx, "STORAGE")
        torch.cuda.synchronize()
        assert bool((flo == SENTINEL).all().item()) and bool((occ == 7).all().item()) and bool((t == SENTINEL).all().item())


def test_batches_refuse_mixed_pitches(ofx_mod, ctxs, synth):
    import torch
    c0, c1 = ctxs["f64"]
    keep, ptr, pitch = _regions("U8", "f64", list(_frames_u8(synth, 5)))
    flo, d_flo, occ, d_occ = _occ_results(3)
    _set(ofx_mod, c0, "U8")
    _set(ofx_mod, c1, "U8")
    c0.set_option("input_pitch", pitch)
    c1.set_option("input_pitch", pitch + 1)
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
        for c in (c0, c1):
            c.set_option("input_pitch", 0)
            _set(ofx_mod, c, "STORAGE")
    torch.cuda.synchronize()
    assert bool((flo == SENTINEL).all().item()) and bool((occ == 7).all().item())


def test_flat_entry_refuses_a_pitch(ofx_mod, ctxs, synth):
    import torch
    ctx = ctxs["f64"][0]
    keep, ptr = _carve([_bytes(f) for f in _frames_u8(synth, 2)], 1)
    t, dst, off = _dst(2, NX * NY, "f64")
    _set(ofx_mod, ctx, "U8")
    ctx.set_option("input_pitch", NX)                    # even the dense pitch: the entry has no row length to compare it with
    try:
        with pytest.raises(ofx_mod.OfxError) as e:
            ctx.normalize_frames_dev(ptr, dst, NX * NY)
        assert e.value.status == ERR_ARG
    finally:
        ctx.set_option("input_pitch", 0)
        _set(ofx_mod, ctx, "STORAGE")
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all().item())
