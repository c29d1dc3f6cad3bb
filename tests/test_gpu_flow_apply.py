"""ofx_flow_warp_dev and ofx_flow_interpolate_dev against their numpy restatement (tests/flow_apply_ref.py): the frames are EQUAL,
element for element.

The inputs are those that tests/test_flow_apply_ref.py pins on the CPU (every branch taken, clamped pixels, no value within 1e-9
of a rounding boundary, blocks that fit the LDS tile and blocks that do not), so equality is a fair demand and cannot hold
vacuously.  Both results are pure functions of the frames' values and the float payloads: U8, U16 and F32 frames give the same
bytes from an f64 and an f32 context."""
import ctypes as C

import numpy as np
import pytest

import flow_apply_ref as far

pytestmark = pytest.mark.gpu

FILL = 0xA5            # guard bytes around every destination
POISON = 0xEE          # padding between the rows of a pitched frame
ERR_ARG = 1
T = (3.0 / 7.0, 5.0 / 7.0, 2.0 / 9.0)        # tests/test_flow_apply_ref.py pins the inputs at these times

# (case, nz): the smallest shapes where the kernel can go wrong -- 2 x 2; nx < 4; byte rows that end off a word and a row longer
# than a wave; 131 x 3; ragged tiles both ways (every channel count there); the TV-L1 payloads; several tiles and the jump
SHAPES = [("2x2", 1), ("2x2", 3), ("3x5", 1), ("3x5", 3), ("67x5", 1), ("67x5", 3), ("131x3", 1), ("131x3", 3),
          ("p1_37x29", 1), ("p1_37x29", 2), ("p1_37x29", 3), ("p1_37x29", 4), ("p1_64x48", 1), ("p1_64x48", 3),
          (far.JUMP, 1), (far.JUMP, 3)]
KINDS = ("f64", "f32", "u8", "u16")


def _contexts(gpu64, gpu32, kind):
    """[(context, value of option "input")]: double frames on the f64 context, float frames on the f32 context and as OFX_IN_F32 on
    the f64 one, the integer kinds on both"""
    if kind == "f64":
        return [(gpu64, 0)]
    if kind == "f32":
        return [(gpu32, 0), (gpu64, far.IN_OPTION["f32"]), (gpu32, far.IN_OPTION["f32"])]
    return [(gpu64, far.IN_OPTION[kind]), (gpu32, far.IN_OPTION[kind])]


class _Options:
    """options of a session-wide context for the length of a `with`, then back to their defaults"""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in (("input", 0), ("input_pitch", 0), ("apply_lds", 2)):
            self.ctx.set_option(k, v)


def _up(a, offset=0):
    """a copy of the array's bytes on the device, `offset` bytes past an 8-byte boundary -> (tensor to keep, pointer)"""
    import torch
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
    t = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 8 == 0
    t[offset:offset + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return t, t.data_ptr() + offset


def _up_frame(a, pitch=0):
    """a frame on the device, dense or with `pitch` bytes between its rows and POISON between and behind them"""
    if not pitch:
        return _up(a)
    ny = a.shape[0]
    row = a[0].nbytes
    host = np.full(ny * pitch + 64, POISON, dtype=np.uint8)
    for i in range(ny):
        host[i * pitch:i * pitch + row] = np.frombuffer(np.ascontiguousarray(a[i]).tobytes(), dtype=np.uint8)
    return _up(host)


class _Dst:
    """n destinations of `shape` and `dtype` carved out of one byte buffer pre-filled with FILL, each `offset` bytes past an 8-byte
    boundary with guard bytes around it; frames() asserts that no other byte changed"""

    def __init__(self, n, shape, dtype, offset=0):
        import torch
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        stride = (self.nbytes + 7) // 8 * 8 + 16
        self.buf = torch.full((n * stride + 16,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 8 == 0
        self.starts = [8 + offset + k * stride for k in range(n)]
        self.ptrs = [self.buf.data_ptr() + s for s in self.starts]
        torch.cuda.synchronize()       # the fills and uploads so far ran on torch's stream; the entries run on the context's

    def frames(self):
        h = self.buf.cpu().numpy()
        mask = np.ones(h.size, dtype=bool)
        for s in self.starts:
            mask[s:s + self.nbytes] = False
        assert (h[mask] == FILL).all(), "bytes outside the destinations were written"
        return [np.frombuffer(h[s:s + self.nbytes].tobytes(), dtype=self.dtype).reshape(self.shape) for s in self.starts]

    def untouched(self):
        return bool((self.buf.cpu().numpy() == FILL).all())


def _warp(ctx, slots, pitch=0, offset=0, occ_offset=0):
    """slots: [(src, flo, occ or None, fill or None)] through ONE call -> the warped frames"""
    src0 = slots[0][0]
    ny, nx, nz = src0.shape
    keep, ps, pf, po, pl = [], [], [], [], []
    for src, flo, occ, fill in slots:
        for arr, out, up in ((src, ps, lambda a: _up_frame(a, pitch)), (flo, pf, _up), (occ, po, lambda a: _up(a, occ_offset)),
                             (fill, pl, lambda a: _up_frame(a, pitch))):
            if arr is None:
                out.append(None)
            else:
                t, p = up(arr)
                keep.append(t)
                out.append(p)
    dst = _Dst(len(slots), src0.shape, src0.dtype, offset)
    ctx.flow_warp_dev(ps, pf, dst.ptrs, nx, ny, nz, d_occ=po if any(p is not None for p in po) else None,
                      dFill=pl if any(p is not None for p in pl) else None)
    ctx.synchronize()
    return dst.frames()


def _interp(ctx, slots, pitch=0, offset=0):
    """slots: [(A, B, fwd, bwd, t)] through ONE call; equal arrays (by identity) are uploaded once and shared by their slots"""
    A0 = slots[0][0]
    ny, nx, nz = A0.shape
    seen = {}

    def up(a, frame):
        if id(a) not in seen:
            seen[id(a)] = _up_frame(a, pitch) if frame else _up(a)
        return seen[id(a)][1]

    pa = [up(s[0], True) for s in slots]
    pb = [up(s[1], True) for s in slots]
    pf = [up(s[2], False) for s in slots]
    pw = [up(s[3], False) for s in slots]
    dst = _Dst(len(slots), A0.shape, A0.dtype, offset)
    ctx.flow_interpolate_dev(pa, pb, pf, pw, [s[4] for s in slots], dst.ptrs, nx, ny, nz)
    ctx.synchronize()
    return dst.frames()


def _same(got, want):
    """equal, bit for bit where the elements are floats (NaN compares equal to itself here)"""
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == np.ascontiguousarray(want).tobytes()


def _inputs(orc, synth, name, nz, kind):
    A, B = far.frames(synth, name, nz, kind)
    fwd, bwd = far.payloads(orc, synth, name)
    return A, B, fwd, bwd, far.occ_maps(orc, synth, name)[0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,nz", SHAPES)
def test_warp_equals_the_restatement(gpu64, gpu32, orc, synth, name, nz, kind):
    """B warped onto A's grid by the forward payload, flagged pixels and pixels that leave from A; and without the map (which
    flags the jump of the jump case: only then do blocks of it miss the tile)"""
    A, B, fwd, _, occ = _inputs(orc, synth, name, nz, kind)
    want = far.want_warp(orc, synth, name, nz, kind)
    want_mapless = far.want_warp(orc, synth, name, nz, kind, with_map=False)
    for ctx, inp in _contexts(gpu64, gpu32, kind):
        with _Options(ctx, input=inp):
            got, mapless = _warp(ctx, [(B, fwd, occ, A), (B, fwd, None, A)])
        assert _same(got, want), (name, nz, kind, inp, int((got != want).sum()))
        assert _same(mapless, want_mapless), (name, nz, kind, inp, int((mapless != want_mapless).sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,nz", SHAPES)
def test_interpolation_equals_the_restatement(gpu64, gpu32, orc, synth, name, nz, kind):
    A, B, fwd, bwd, _ = _inputs(orc, synth, name, nz, kind)
    want = far.want_interp(orc, synth, name, nz, kind, T[0])
    for ctx, inp in _contexts(gpu64, gpu32, kind):
        with _Options(ctx, input=inp):
            got, = _interp(ctx, [(A, B, fwd, bwd, T[0])])
        assert _same(got, want), (name, nz, kind, inp, int((got != want).sum()))


@pytest.mark.parametrize("name,nz,kind", [(far.JUMP, 3, "u8"), (far.JUMP, 1, "f64"), (far.JUMP, 2, "u16"), (far.JUMP, 4, "f32"),
                                          ("p1_64x48", 3, "u8"), ("p1_37x29", 2, "u16"), ("p1_37x29", 4, "u8"), ("p1_37x29", 3, "f32"),
                                          ("67x5", 3, "u8"), ("131x3", 1, "u16"), ("3x5", 1, "u8"), ("2x2", 3, "u8"), ("2x2", 1, "f64")])
def test_apply_lds_changes_nothing(gpu64, orc, synth, name, nz, kind):
    """option apply_lds = 0 (global gathers alone) and 1 (LDS tiles, global gathers for the blocks that miss) give the restatement:
    the default, 2, picks one of them by the element's size, so each kind runs here on the path it does not take by default"""
    A, B, fwd, bwd, occ = _inputs(orc, synth, name, nz, kind)
    for lds in (0, 1):
        with _Options(gpu64, input=far.IN_OPTION.get(kind, 0), apply_lds=lds):
            got, mapless = _warp(gpu64, [(B, fwd, occ, A), (B, fwd, None, A)])
            assert _same(got, far.want_warp(orc, synth, name, nz, kind)), lds
            assert _same(mapless, far.want_warp(orc, synth, name, nz, kind, with_map=False)), lds
            for t in T:
                got, = _interp(gpu64, [(A, B, fwd, bwd, t)])
                assert _same(got, far.want_interp(orc, synth, name, nz, kind, t)), (lds, t)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,nz", [("67x5", 3), ("p1_37x29", 2), ("3x5", 1)])
def test_pitched_frames(gpu64, gpu32, orc, synth, name, nz, kind):
    """input_pitch padded to a multiple of 256 bytes, and the row's bytes + the element's alignment (the smallest valid padding):
    both equal the dense call; the poisoned padding never reaches the result"""
    A, B, fwd, bwd, occ = _inputs(orc, synth, name, nz, kind)
    row = A[0].nbytes
    ctx, inp = _contexts(gpu64, gpu32, kind)[0]
    for pitch in ((row + 255) // 256 * 256 + 256, row + A.dtype.itemsize):
        with _Options(ctx, input=inp, input_pitch=pitch):
            got, = _warp(ctx, [(B, fwd, occ, A)], pitch=pitch)
            assert _same(got, far.want_warp(orc, synth, name, nz, kind)), pitch
            got, = _interp(ctx, [(A, B, fwd, bwd, T[0])], pitch=pitch)
            assert _same(got, far.want_interp(orc, synth, name, nz, kind, T[0])), pitch


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("name,nz", [("67x5", 3), ("3x5", 1), ("p1_37x29", 3), ("2x2", 1), ("131x3", 1)])
def test_byte_destinations_off_a_word(gpu64, orc, synth, name, nz, offset):
    """byte frames written 1, 2 and 3 bytes past a word boundary (and a map at an odd address): equal, and not a byte outside"""
    A, B, fwd, bwd, occ = _inputs(orc, synth, name, nz, "u8")
    with _Options(gpu64, input=far.IN_OPTION["u8"]):
        got, = _warp(gpu64, [(B, fwd, occ, A)], offset=offset, occ_offset=1)
        assert _same(got, far.want_warp(orc, synth, name, nz, "u8"))
        got, = _interp(gpu64, [(A, B, fwd, bwd, T[0])], offset=offset)
        assert _same(got, far.want_interp(orc, synth, name, nz, "u8", T[0]))


def test_u16_destination_off_a_word(gpu64, orc, synth):
    A, B, fwd, bwd, occ = _inputs(orc, synth, "67x5", 3, "u16")
    with _Options(gpu64, input=far.IN_OPTION["u16"]):
        got, = _warp(gpu64, [(B, fwd, occ, A)], offset=2)
        assert _same(got, far.want_warp(orc, synth, "67x5", 3, "u16"))
        got, = _interp(gpu64, [(A, B, fwd, bwd, T[0])], offset=2)
        assert _same(got, far.want_interp(orc, synth, "67x5", 3, "u16", T[0]))


@pytest.mark.parametrize("n,offset", [(5, 1), (17, 3)])
def test_many_slots_in_one_call(gpu64, orc, synth, n, offset):
    """5 slots = one launch; 17 = two (16 + 1).  The slots differ: the payloads are exchanged in odd slots, slot 4 has the zero
    payload, no map and no fill frame, and the t values rotate"""
    A, B, fwd, bwd, occ = _inputs(orc, synth, "67x5", 3, "u8")
    zero = np.zeros_like(fwd)
    ws, iss = [], []
    for k in range(n):
        f, b = (zero, zero) if k == 4 else ((bwd, fwd) if k % 2 else (fwd, bwd))
        ws.append((B, f, None if k == 4 else occ, None if k == 4 else A))
        iss.append((A, B, f, b, T[k % 3]))
    with _Options(gpu64, input=far.IN_OPTION["u8"]):
        got_w = _warp(gpu64, ws, offset=offset)
        got_i = _interp(gpu64, iss, offset=offset)
    want_w, want_i = {}, {}
    for k in range(n):
        kw = (id(ws[k][1]), ws[k][2] is None)
        if kw not in want_w:
            want_w[kw] = far.warp(orc, *ws[k])
        assert _same(got_w[k], want_w[kw]), ("warp", k)
        ki = (id(iss[k][2]), iss[k][4])
        if ki not in want_i:
            want_i[ki] = far.interpolate(orc, *iss[k])
        assert _same(got_i[k], want_i[ki]), ("interpolate", k)
    assert _same(got_w[4], B)                                     # a zero payload writes Src exactly


@pytest.mark.parametrize("kind,nz", [("u8", 3), ("f64", 1)])
def test_three_times_on_one_pair(gpu64, orc, synth, kind, nz):
    """three in-between frames of one pair in one launch: the slots name the same frames and payloads"""
    A, B, fwd, bwd, _ = _inputs(orc, synth, far.JUMP, nz, kind)
    with _Options(gpu64, input=far.IN_OPTION.get(kind, 0)):
        got = _interp(gpu64, [(A, B, fwd, bwd, t) for t in T])
    for k, t in enumerate(T):
        assert _same(got[k], far.want_interp(orc, synth, far.JUMP, nz, kind, t)), t


def _hand_built(nx, ny):
    F = np.zeros((ny, nx, 2), dtype=np.float32)
    F[2, 0, 0] = -0.5            # leaves on the left
    F[2, 8, 0] = 0.25            # ... on the right
    F[0, 3, 1] = -0.25           # ... at the top
    F[5, 3, 1] = 0.125           # ... at the bottom
    F[1, 1, 0] = np.nan
    F[1, 2, 1] = np.nan
    F[3, 1, 0] = np.inf
    F[3, 2, 1] = -np.inf
    F[3, 3, 0] = -np.inf
    F[4, 4, 1] = np.inf
    F[2, 7, 0] = 1.0             # lands exactly on column nx - 1: sampled
    F[4, 6, 1] = 1.0             # ... on row ny - 1
    F[1, 5] = (1.5, 0.75)        # an ordinary vector
    F[2, 3] = (3e9, -3e9)        # beyond an int
    return F


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_hand_built_payloads(gpu64, orc, synth, kind):
    nx, ny = 9, 6
    A, B = (np.ascontiguousarray(x[:ny, :nx]) for x in far.frames(synth, "p1_37x29", 3, kind))
    F = _hand_built(nx, ny)
    Z = np.zeros_like(F)
    left = [(2, 0), (2, 8), (0, 3), (5, 3), (1, 1), (1, 2), (3, 1), (3, 2), (3, 3), (4, 4), (2, 3)]
    occ = np.zeros((ny, nx), dtype=np.uint8)
    occ[4, 1], occ[1, 5] = 255, 1                                  # any non-zero byte flags
    with _Options(gpu64, input=far.IN_OPTION.get(kind, 0)):
        plain, filled, mapped, mapped_filled = _warp(gpu64, [(B, F, None, None), (B, F, None, A), (B, F, occ, None), (B, F, occ, A)],
                                                     occ_offset=1)
        for got, o, f in ((plain, None, None), (filled, None, A), (mapped, occ, None), (mapped_filled, occ, A)):
            assert _same(got, far.warp(orc, B, F, o, f))
        for r, c in left:
            assert not plain[r, c].any() and _same(filled[r, c], A[r, c]), (r, c)
        assert _same(plain[2, 7], B[2, 8]) and _same(plain[4, 6], B[5, 6])          # on the last column / row: sampled, not refused
        assert not mapped[4, 1].any() and not mapped[1, 5].any() and _same(mapped_filled[4, 1], A[4, 1])
        got = _interp(gpu64, [(A, B, F, Z, T[0]), (A, B, Z, F, T[1]), (A, B, F, F, T[2]), (A, B, F, F, 0.0), (A, B, F, F, 1.0),
                              (A, B, Z, Z, 0.0), (A, B, Z, Z, 1.0)])
        for g, (f, b, t) in zip(got, ((F, Z, T[0]), (Z, F, T[1]), (F, F, T[2]), (F, F, 0.0), (F, F, 1.0))):
            assert _same(g, far.interpolate(orc, A, B, f, b, t)), t
        assert _same(got[5], A) and _same(got[6], B)               # t = 0 writes A, t = 1 writes B
        # an integer translation gives the shifted frame
        S = Z.copy()
        S[..., 0], S[..., 1] = 2.0, -1.0
        got, = _warp(gpu64, [(B, S, None, None)])
        want = np.zeros_like(B)
        want[1:, :nx - 2] = B[:ny - 1, 2:]
        assert _same(got, want)


def test_buffers_in_pageable_host_memory(gpu64, orc, synth):
    """a payload and a destination (and, for the in-between frame, a frame) in pageable host memory: staged by the entries"""
    name, nz, kind = "p1_37x29", 3, "u8"
    A, B, fwd, bwd, occ = _inputs(orc, synth, name, nz, kind)
    ny, nx, _ = A.shape
    hf = np.array(fwd)
    hb = np.array(B)
    out_w = np.full(A.shape, FILL, dtype=np.uint8)
    out_i = np.full(A.shape, FILL, dtype=np.uint8)
    keep = [_up(x) for x in (A, B, bwd, occ)]
    dA, dB, dbwd, docc = (p for _, p in keep)
    import torch
    torch.cuda.synchronize()
    with _Options(gpu64, input=far.IN_OPTION[kind]):
        gpu64.flow_warp_dev([dB], [hf.ctypes.data], [out_w.ctypes.data], nx, ny, nz, d_occ=[docc], dFill=[dA])
        gpu64.synchronize()
        gpu64.flow_interpolate_dev([dA], [hb.ctypes.data], [hf.ctypes.data], [dbwd], [T[0]], [out_i.ctypes.data], nx, ny, nz)
        gpu64.synchronize()
    assert _same(out_w, far.want_warp(orc, synth, name, nz, kind))
    assert _same(out_i, far.want_interp(orc, synth, name, nz, kind, T[0]))


def test_refusals_write_nothing(ofx_mod, gpu64):
    import torch
    nx, ny, nz = 8, 6, 3
    n = nx * ny
    flo = torch.zeros((2, n + 1, 2), dtype=torch.float32, device="cuda")
    frm = torch.zeros((3, n * nz + 8), dtype=torch.float64, device="cuda")
    occ = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    dst = _Dst(1, (ny, nx, nz), np.float64)
    f, b = flo[0].data_ptr(), flo[1].data_ptr()
    a, bb, fl, d = frm[0].data_ptr(), frm[1].data_ptr(), frm[2].data_ptr(), dst.ptrs[0]
    L, h = gpu64.L, gpu64.h
    arr = lambda xs: (ofx_mod._vp * len(xs))(*xs)
    one_t = lambda t: (C.c_double * 1)(t)

    def refused(status):
        gpu64.synchronize()
        assert status == ERR_ARG, status
        assert L.ofx_last_error(h), "ofx_last_error is empty"
        assert dst.untouched()

    def warp(n_=1, src=a, flo_=f, occ_=occ.data_ptr(), fill=fl, dst_=d, nx_=nx, ny_=ny, nz_=nz, tables=None):
        t = [arr([src]), arr([flo_]), arr([occ_]), arr([fill]), arr([dst_])]
        for k, v in (tables or {}).items():
            t[k] = v
        return L.ofx_flow_warp_dev(h, n_, *t, nx_, ny_, nz_)

    def interp(n_=1, A=a, B=bb, fwd=f, bwd=b, t=0.5, dst_=d, nx_=nx, ny_=ny, nz_=nz, tables=None):
        tb = [arr([A]), arr([B]), arr([fwd]), arr([bwd]), one_t(t), arr([dst_])]
        for k, v in (tables or {}).items():
            tb[k] = v
        return L.ofx_flow_interpolate_dev(h, n_, *tb, nx_, ny_, nz_)

    try:
        for k in (0, 1, 4):                                        # a NULL table, a NULL entry (d_occ and dFill may be NULL)
            refused(warp(tables={k: None}))
            refused(warp(tables={k: arr([None])}))
        for k in (0, 1, 2, 3, 5):
            refused(interp(tables={k: None}))
            refused(interp(tables={k: arr([None])}))
        refused(interp(tables={4: None}))                          # t itself
        for call in (warp, interp):
            refused(call(n_=0))
            refused(call(n_=-2))
            refused(call(nx_=1))
            refused(call(ny_=1))
            refused(call(nx_=65536, ny_=32768, nz_=1))             # 2^31 elements
            refused(call(nx_=32768, ny_=32768, nz_=3))
            refused(call(nz_=0))
            refused(call(nz_=5))
            refused(call(dst_=d + 4))                              # a double frame off its alignment
        refused(warp(flo_=f + 4))
        refused(warp(src=a + 4))
        refused(warp(fill=fl + 4))
        refused(interp(fwd=f + 4))
        refused(interp(bwd=b + 4))
        refused(interp(A=a + 4))
        refused(interp(B=bb + 4))
        for t in (-0.01, 1.01, float("nan"), float("inf"), float("-inf")):
            refused(interp(t=t))
        refused(warp(src=d))                                       # the destination is a frame its own slot reads
        refused(warp(fill=d))
        refused(interp(A=d))
        refused(interp(B=d))
        gpu64.set_option("input", 4)                               # OFX_IN_RGB8
        refused(warp())
        refused(interp())
        gpu64.set_option("input", 0)
        gpu64.set_option("input_pitch", nx * nz * 8 - 8)           # below the row's bytes
        refused(warp())
        refused(interp())
        gpu64.set_option("input_pitch", nx * nz * 8 + 4)           # not a multiple of the element's alignment
        refused(warp())
        refused(interp())
        gpu64.set_option("input_pitch", 0)
        for bad in (3, -1, 0.5):                                   # option apply_lds takes 0, 1 and 2
            assert L.ofx_set_option(h, b"apply_lds", float(bad)) == ERR_ARG
        # and the same calls without a fault go through
        assert warp() == 0
        gpu64.synchronize()
        assert not dst.frames()[0].any()
        frm[0].fill_(2.0)
        frm[1].fill_(4.0)
        torch.cuda.synchronize()
        assert interp(t=0.25) == 0
        gpu64.synchronize()
        assert (dst.frames()[0] == 2.5).all()
    finally:
        gpu64.set_option("input", 0)
        gpu64.set_option("input_pitch", 0)


def test_a_bidirectional_solve_feeds_both_entries_in_place(gpu64, orc, synth):
    """ofx_tvl1_bidir_group_dev on synth.pair("P1", 64, 48): its device payloads and maps go straight into both entries; the
    results equal the restatement on the oracle's payloads"""
    import torch
    nx, ny = 64, 48
    I0, I1 = synth.pair("P1", nx, ny)
    A, B = torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda()
    flo = torch.zeros((2, ny, nx, 2), dtype=torch.float32, device="cuda")
    occ = torch.zeros((2, ny, nx), dtype=torch.uint8, device="cuda")
    dst = _Dst(2, (ny, nx, 1), np.float64)
    gpu64.tvl1_bidir_group_dev([A.data_ptr()], [B.data_ptr()], [flo[0].data_ptr()], [flo[1].data_ptr()], [occ[0].data_ptr()],
                               [occ[1].data_ptr()], nx, ny, nscales=3)
    gpu64.flow_warp_dev([B.data_ptr()], [flo[0].data_ptr()], dst.ptrs[:1], nx, ny, 1, d_occ=[occ[0].data_ptr()], dFill=[A.data_ptr()])
    gpu64.flow_interpolate_dev([A.data_ptr()], [B.data_ptr()], [flo[0].data_ptr()], [flo[1].data_ptr()], [T[0]], dst.ptrs[1:], nx, ny, 1)
    gpu64.synchronize()
    got_w, got_i = dst.frames()
    assert _same(got_w, far.want_warp(orc, synth, "p1_64x48", 1, "f64"))
    assert _same(got_i, far.want_interp(orc, synth, "p1_64x48", 1, "f64", T[0]))
