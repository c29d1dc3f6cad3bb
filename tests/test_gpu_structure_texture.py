"""ofx_structure_texture_dev against its numpy restatement (tests/structure_texture_ref.py): every destination is EQUAL to it,
element for element -- the doubles of an f64 context, and for an f32 context (float) of those doubles -- under every "st_fuse",
input kind and pitch, and nothing outside a destination is written.  Then the point of it: TV-L1 on the device's texture frames."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import structure_texture_ref as st

pytestmark = pytest.mark.gpu

FILL = 0xA5            # guard bytes around every destination
POISON = 0xEE          # padding between the rows of a pitched frame
ERR_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(path, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(os.path.join(ROOT, path)).read()).group(1))


K_DEFAULT = _define("optical-flow-1_amd/csrc/ofx_texture.hip", "ST_DEFAULT_FUSE")
K_MAX = _define("include/ofx.h", "OFX_ST_MAX_FUSE")
MAX_ITERS = _define("include/ofx.h", "OFX_ST_MAX_ITERS")
# (nx, ny): smaller than any halo; one axis inside one tile and the other ragged; ragged both ways; and three or more of the
# kernel's 64 x 48-cell tiles on each axis for every K (an output region is at most 62 x 46 cells)
SHAPES = [(2, 2), (3, 5), (5, 67), (131, 3), (67, 45), (389, 197)]
KINDS = ("f64", "f32", "u8", "u16", "rgb8")
N_ITERS = sorted({0, 1, 2, K_DEFAULT - 1, K_DEFAULT, K_DEFAULT + 1, 37})


def _contexts(gpu64, gpu32, kind):
    """[(context, value of option "input", dtype of its destinations)]"""
    if kind == "f64":
        return [(gpu64, 0, np.float64)]
    if kind == "f32":
        return [(gpu32, 0, np.float32), (gpu64, st.IN_OPTION["f32"], np.float64), (gpu32, st.IN_OPTION["f32"], np.float32)]
    return [(gpu64, st.IN_OPTION[kind], np.float64), (gpu32, st.IN_OPTION[kind], np.float32)]


class _Options:
    """options of a session-wide context for the length of a `with`, then back to their defaults"""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in ("input", "input_pitch", "st_fuse"):
            self.ctx.set_option(k, 0)


def _up(a):
    """a copy of the array's bytes on the device -> (tensor to keep, pointer)"""
    import torch
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
    t = torch.from_numpy(raw.copy()).cuda()
    assert t.data_ptr() % 8 == 0
    return t, t.data_ptr()


def _pitched(a, pitch):
    """the frame's rows `pitch` bytes apart, POISON between them, and NOTHING behind the last row's end"""
    ny = a.shape[0]
    row = a[0].nbytes
    host = np.full((ny - 1) * pitch + row, POISON, dtype=np.uint8)
    for i in range(ny):
        host[i * pitch:i * pitch + row] = np.frombuffer(np.ascontiguousarray(a[i]).tobytes(), dtype=np.uint8)
    return host


class _Dst:
    """n destinations of `shape` and `dtype` carved out of one byte buffer pre-filled with FILL, with guard bytes around each;
    frames() asserts that no other byte changed"""

    def __init__(self, n, shape, dtype):
        import torch
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        stride = (self.nbytes + 7) // 8 * 8 + 16
        self.buf = torch.full((n * stride + 16,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 8 == 0
        self.starts = [8 + k * stride for k in range(n)]
        self.ptrs = [self.buf.data_ptr() + s for s in self.starts]
        torch.cuda.synchronize()       # the fills and uploads so far ran on torch's stream; the entry runs on the context's

    def frames(self, written=None):
        h = self.buf.cpu().numpy()
        mask = np.ones(h.size, dtype=bool)
        for k, s in enumerate(self.starts):
            if written is None or written[k]:
                mask[s:s + self.nbytes] = False
        assert (h[mask] == FILL).all(), "bytes outside the destinations were written"
        return [np.frombuffer(h[s:s + self.nbytes].tobytes(), dtype=self.dtype).reshape(self.shape) for s in self.starts]

    def untouched(self):
        return bool((self.buf.cpu().numpy() == FILL).all())


def _run(ctx, dtype, frames, nx, ny, theta, n_iter, alpha=st.ALPHA, pitch=0, structure=True):
    """frames through ONE call -> ([T], [S or None]).  structure: True, False, or one flag per slot"""
    flags = [structure] * len(frames) if isinstance(structure, bool) else list(structure)
    keep = [_up(_pitched(f, pitch) if pitch else f) for f in frames]
    tex, stru = _Dst(len(frames), (ny, nx), dtype), _Dst(len(frames), (ny, nx), dtype)
    ds = None if not any(flags) else [p if fl else None for p, fl in zip(stru.ptrs, flags)]
    ctx.structure_texture_dev([p for _, p in keep], tex.ptrs, nx, ny, theta=theta, alpha=alpha, n_iter=n_iter, dStruct=ds)
    ctx.synchronize()
    S = stru.frames(written=flags)
    return tex.frames(), [s if fl else None for s, fl in zip(S, flags)]


def _same(got, want, dtype):
    want = np.ascontiguousarray(want.astype(dtype))
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_frames_equal_the_restatement(gpu64, gpu32, nx, ny, kind):
    """37 iterations under the default schedule: launches of K and a last one of 37 mod K; every kind on both contexts"""
    a = st.frame(nx, ny, kind)[0]
    S, T = st.want(nx, ny, kind, 37)
    for ctx, inp, dtype in _contexts(gpu64, gpu32, kind):
        with _Options(ctx, input=inp):
            (t,), (s,) = _run(ctx, dtype, [a], nx, ny, st.theta_for(kind), 37)
        assert _same(t, T, dtype), (kind, inp, dtype, int((t != T.astype(dtype)).sum()))
        assert _same(s, S, dtype), (kind, inp, dtype, int((s != S.astype(dtype)).sum()))


@pytest.mark.parametrize("fuse", sorted({1, 2, 0, K_MAX}))
@pytest.mark.parametrize("nx,ny", [(3, 5), (131, 3), (67, 45)])
def test_every_iteration_count_under_every_schedule(gpu64, nx, ny, fuse):
    """n_iter around the default K and the forced ones: a call of a single launch, launches of K alone, a short last launch"""
    a = st.frame(nx, ny, "u8")[0]
    for n_iter in N_ITERS:
        S, T = st.want(nx, ny, "u8", n_iter)
        with _Options(gpu64, input=st.IN_OPTION["u8"], st_fuse=fuse):
            (t,), (s,) = _run(gpu64, np.float64, [a], nx, ny, st.THETA, n_iter)
        assert _same(t, T, np.float64) and _same(s, S, np.float64), (fuse, n_iter)
    if fuse == 0:
        assert np.array_equal(st.want(nx, ny, "u8", 0)[0], st.frame(nx, ny, "u8")[1])       # n_iter = 0 writes S = f


@pytest.mark.parametrize("fuse", sorted({1, 2, 3, K_MAX}))
def test_schedules_agree_on_many_tiles(gpu64, gpu32, fuse):
    """389 x 197: three or more tiles each way for every K; the f32 context's floats are (float) of the doubles"""
    nx, ny = 389, 197
    a = st.frame(nx, ny, "f64")[0]
    S, T = st.want(nx, ny, "f64", 37)
    with _Options(gpu64, st_fuse=fuse):
        (t,), (s,) = _run(gpu64, np.float64, [a], nx, ny, st.THETA, 37)
    assert _same(t, T, np.float64) and _same(s, S, np.float64), fuse
    a32 = st.frame(nx, ny, "f32")[0]
    S, T = st.want(nx, ny, "f32", 37)
    with _Options(gpu32, st_fuse=fuse):
        (t,), (s,) = _run(gpu32, np.float32, [a32], nx, ny, st.THETA, 37)
    assert _same(t, T, np.float32) and _same(s, S, np.float32), fuse


@pytest.mark.parametrize("kind,extra", [("u8", 1), ("f64", 8), ("rgb8", 1), ("u16", 2), ("f32", 4), ("u8", 61)])
def test_pitched_frames(gpu64, kind, extra):
    """rows `extra` bytes further apart than they are long (one element more, or a decoder's padding), poison in the padding, the
    buffer ends with the last row: no byte outside the rows is read"""
    nx, ny = 67, 45
    a = st.frame(nx, ny, kind)[0]
    S, T = st.want(nx, ny, kind, 37)
    pitch = a[0].nbytes + extra
    with _Options(gpu64, input=st.IN_OPTION.get(kind, 0), input_pitch=pitch):
        (t,), (s,) = _run(gpu64, np.float64, [a], nx, ny, st.theta_for(kind), 37, pitch=pitch)
    assert _same(t, T, np.float64) and _same(s, S, np.float64)


def test_seventeen_frames_and_structure_for_some(gpu64, gpu32):
    """the second launch batch; dStruct present for some slots only, and absent"""
    nx, ny, n = 67, 45, 17
    frames = [st.frame(nx, ny, "u8", seed)[0] for seed in range(n)]
    flags = [g % 3 != 1 for g in range(n)]
    for ctx, dtype in ((gpu64, np.float64), (gpu32, np.float32)):
        with _Options(ctx, input=st.IN_OPTION["u8"]):
            T, S = _run(ctx, dtype, frames, nx, ny, st.THETA, 9, structure=flags)
            T2, S2 = _run(ctx, dtype, frames[:2], nx, ny, st.THETA, 9, structure=False)
        for g in range(n):
            ws, wt = st.want(nx, ny, "u8", 9, g)
            assert _same(T[g], wt, dtype), g
            assert (S[g] is None) if not flags[g] else _same(S[g], ws, dtype), g
        assert _same(T2[0], st.want(nx, ny, "u8", 9, 0)[1], dtype) and _same(T2[1], st.want(nx, ny, "u8", 9, 1)[1], dtype)
        assert S2 == [None, None]
    assert len({st.want(nx, ny, "u8", 9, g)[1].tobytes() for g in range(n)}) == n       # 17 distinct frames


def test_host_buffers_are_staged(gpu64):
    """a source and destinations in pageable host memory"""
    nx, ny = 67, 45
    a = np.array(st.frame(nx, ny, "u8")[0])
    S, T = st.want(nx, ny, "u8", 37)
    out = np.full((2, ny * nx + 2), np.nan)
    with _Options(gpu64, input=st.IN_OPTION["u8"]):
        gpu64.structure_texture_dev([a.ctypes.data], [out[0, 1:].ctypes.data], nx, ny, n_iter=37, dStruct=[out[1, 1:].ctypes.data])
        gpu64.synchronize()
    assert np.array_equal(out[0, 1:-1].reshape(ny, nx), T) and np.array_equal(out[1, 1:-1].reshape(ny, nx), S)
    assert np.isnan(out[:, [0, -1]]).all()


def test_constant_frames_and_alpha(gpu64):
    """a constant frame writes S = f and T = f - alpha f exactly; alpha = 0 and 1 are accepted"""
    nx, ny = 67, 45
    f = np.full((ny, nx), 1.0 / 3.0)
    for alpha in (0.0, 0.95, 1.0):
        (t,), (s,) = _run(gpu64, np.float64, [f], nx, ny, 16.0, 11, alpha=alpha)
        assert np.array_equal(s, f) and np.array_equal(t, f - alpha * f)
    a = st.frame(nx, ny, "f64")[0]
    (t,), (s,) = _run(gpu64, np.float64, [a], nx, ny, 16.0, 37, alpha=0.0)
    assert np.array_equal(t, a) and _same(s, st.want(nx, ny, "f64", 37)[0], np.float64)


def test_refusals_write_nothing(ofx_mod, gpu64):
    import torch
    nx, ny = 8, 6
    n = nx * ny
    frm = torch.zeros((2, n + 8), dtype=torch.float64, device="cuda")
    tex, stru = _Dst(2, (ny, nx), np.float64), _Dst(2, (ny, nx), np.float64)
    a, b = frm[0].data_ptr(), frm[1].data_ptr()
    L, h = gpu64.L, gpu64.h
    arr = lambda xs: (ofx_mod._vp * len(xs))(*xs)

    def refused(status, slot=None):
        gpu64.synchronize()
        assert status == ERR_ARG, status
        msg = (L.ofx_last_error(h) or b"").decode()
        assert msg.startswith("structure_texture"), msg
        if slot is not None:
            assert "slot %d" % slot in msg, msg
        assert tex.untouched() and stru.untouched()

    def call(n_=2, src=(a, b), t=None, s=None, nx_=nx, ny_=ny, theta=16.0, alpha=0.95, n_iter=3, tables=None):
        tb = [arr(list(src)), arr(list(t or tex.ptrs)), arr(list(s or stru.ptrs))]
        for k, v in (tables or {}).items():
            tb[k] = v
        return L.ofx_structure_texture_dev(h, n_, *tb, nx_, ny_, theta, alpha, n_iter)

    try:
        for k, first in ((0, a), (1, tex.ptrs[0])):                 # a NULL table, a NULL entry (dStruct and its entries may be NULL)
            refused(call(tables={k: None}))
            refused(call(tables={k: arr([first, None])}), slot=1)
        refused(call(n_=0))
        refused(call(n_=-2))
        refused(call(nx_=1))
        refused(call(ny_=1))
        refused(call(nx_=65536, ny_=32768))                         # 2^31 elements
        for theta in (0.0, -1.0, float("nan"), float("inf")):
            refused(call(theta=theta))
        for alpha in (-0.01, 1.01, float("nan"), float("inf"), float("-inf")):
            refused(call(alpha=alpha))
        refused(call(n_iter=-1))
        refused(call(n_iter=MAX_ITERS + 1))
        refused(call(src=(a, b + 4)), slot=1)                       # a double frame off its alignment
        refused(call(t=(tex.ptrs[0], tex.ptrs[1] + 4)), slot=1)
        refused(call(s=(stru.ptrs[0], stru.ptrs[1] + 4)), slot=1)
        refused(call(src=(a, tex.ptrs[1])), slot=1)                 # a destination is the source of its own slot
        refused(call(src=(a, stru.ptrs[1])), slot=1)
        gpu64.set_option("input_pitch", nx * 8 - 8)                 # below the row's bytes
        refused(call())
        gpu64.set_option("input_pitch", nx * 8 + 4)                 # not a multiple of the element's alignment
        refused(call())
        gpu64.set_option("input_pitch", 0)
        for bad in (K_MAX + 1, -1, 0.5, float("nan")):              # option st_fuse takes 0 .. the maximum
            assert L.ofx_set_option(h, b"st_fuse", float(bad)) == ERR_ARG
        # and the same call without a fault goes through: zero frames give zero frames
        assert call() == 0
        gpu64.synchronize()
        assert not any(f.any() for f in tex.frames() + stru.frames())
    finally:
        gpu64.set_option("input_pitch", 0)
        gpu64.set_option("st_fuse", 0)


@pytest.mark.parametrize("name,change", [("P0", "shadow"), ("P1", "gain_ramp")])
def test_tvl1_on_the_device_texture_frames(gpu64, orc, synth, name, change):
    """ofx_structure_texture_dev straight into ofx_tvl1_group_dev (strict f64), raw frames beside them: the payload and the
    iteration table equal the oracle's on the restated frames (the strict-mode comparison of tests/test_gpu_tvl1.py), and the
    texture frames bring the error against the truth down as they do on the CPU"""
    import torch
    nx, ny = 160, 120
    I0, I1 = st.quality_pair(synth, name, change)
    raw = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (I0, I1)]
    tex = torch.zeros((2, ny, nx), dtype=torch.float64, device="cuda")
    flo = torch.zeros((2, ny, nx, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu64.structure_texture_dev([t.data_ptr() for t in raw], [tex[0].data_ptr(), tex[1].data_ptr()], nx, ny)
    stt = gpu64.tvl1_group_dev([tex[0].data_ptr(), raw[0].data_ptr()], [tex[1].data_ptr(), raw[1].data_ptr()],
                               [flo[0].data_ptr(), flo[1].data_ptr()], nx, ny, nscales=4)
    gpu64.synchronize()
    got = flo.cpu().numpy()
    T0, T1 = st.texture(I0), st.texture(I1)
    assert np.array_equal(tex.cpu().numpy(), np.stack([T0, T1]))
    uo, vo, it, _ = orc.tvl1_multiscale(T0, T1, nscales=4)
    assert np.array_equal(stt[0].iterations(), it)
    assert np.array_equal(got[0], np.stack([uo, vo], axis=-1).astype(np.float32))
    e_tex = st.aepe_truth(synth, name, got[0, ..., 0].astype(np.float64), got[0, ..., 1].astype(np.float64))
    e_raw = st.aepe_truth(synth, name, got[1, ..., 0].astype(np.float64), got[1, ..., 1].astype(np.float64))
    print("AEPE %s %s on the device: raw %.4f texture %.4f" % (name, change, e_raw, e_tex))
    assert e_tex <= 0.25 * e_raw, (e_raw, e_tex)


@pytest.mark.parametrize("name", ["P0", "P1"])
def test_tvl1_on_the_device_texture_frames_of_an_unchanged_pair(gpu64, synth, name):
    import torch
    nx, ny = 160, 120
    I0, I1 = st.quality_pair(synth, name, "unchanged")
    raw = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (I0, I1)]
    tex = torch.zeros((2, ny, nx), dtype=torch.float64, device="cuda")
    flo = torch.zeros((2, ny, nx, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu64.structure_texture_dev([t.data_ptr() for t in raw], [tex[0].data_ptr(), tex[1].data_ptr()], nx, ny)
    gpu64.tvl1_group_dev([tex[0].data_ptr(), raw[0].data_ptr()], [tex[1].data_ptr(), raw[1].data_ptr()],
                         [flo[0].data_ptr(), flo[1].data_ptr()], nx, ny, nscales=4)
    gpu64.synchronize()
    got = flo.cpu().numpy().astype(np.float64)
    e_tex, e_raw = (st.aepe_truth(synth, name, got[k, ..., 0], got[k, ..., 1]) for k in (0, 1))
    assert e_tex <= e_raw + 0.03, (e_raw, e_tex)
