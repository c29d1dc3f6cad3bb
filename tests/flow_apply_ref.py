"""ofx_flow_warp_dev and ofx_flow_interpolate_dev (include/ofx.h) restated in numpy, and the inputs that the tests of them share.

A frame is an (ny, nx, nz) array of float64, float32, uint8 or uint16; a payload an (ny, nx, 2) float32 array, (u, v) interleaved;
a map an (ny, nx) uint8 array, 0 = keep.  All arithmetic in float64, one rounding per operation, association as written:

    inside(x, y)  = x >= 0 and x <= nx - 1 and y >= 0 and y <= ny - 1                      (NaN and Inf fail it)
    sample(I, ..) = Oracle.bicubic_warp_color(I, dx, dy, border_out=False), which samples at (j + dx, i + dy): the reference's
                    bicubic_interpolation_at_color.  The C code casts the coordinate to int, so the displacement of every pixel
                    that fails `inside` is replaced by 0 before the call: NaN, Inf and far-outside positions never reach it.
    conv(x)       = x | float32(x) | for uint8 / uint16 with max = 255 / 65535: NaN -> 0, x <= 0 -> 0, x >= max -> max,
                    otherwise int(x + 0.5)

warp:         (u, v) = flo[i, j];  x = j + u;  y = i + v;  keep = inside(x, y) and (no map or occ[i, j] == 0)
              keep: conv(sample(Src, x, y, k));  otherwise Fill[i, j, k] unchanged, or 0 without a fill frame
interpolate:  s = 1 - t;  c0 = s t;  c1 = t t;  c2 = s s;  (u01, v01) = fwd[i, j];  (u10, v10) = bwd[i, j]
              xa = j + (c1 u10 - c0 u01);  ya = i + (c1 v10 - c0 v01);  xb = j + (c2 u01 - c0 u10);  yb = i + (c2 v01 - c0 v10)
              both inside: s sample(A) + t sample(B);  one inside: that sample;  neither: s A[i, j, k] + t B[i, j, k];  then conv
numpy's elementwise float64 operations round once each and contract nothing, so the expressions below are that definition."""
import numpy as np

import flow_consistency_ref as fcr

KINDS = {"f64": np.float64, "f32": np.float32, "u8": np.uint8, "u16": np.uint16}
IN_OPTION = {"u8": 1, "u16": 2, "f32": 3}            # OFX_IN_* of a kind that is not the context's storage type
BLOCK, TILE = (32, 8), (48, 16)                      # pixels of a workgroup and of its LDS tile (csrc/ofx_apply.hip), columns x rows


def _grid(ny, nx):
    return np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")


def inside(x, y, nx, ny):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= nx - 1) & (y >= 0) & (y <= ny - 1)


def sample(orc, I64, dx, dy, ok):
    """(ny, nx, nz) samples at (j + dx, i + dy) where ok, at (j, i) elsewhere (never used there)"""
    return orc.bicubic_warp_color(I64, np.where(ok, dx, 0.0), np.where(ok, dy, 0.0), False)


def conv(x, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return x
    if dtype == np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            return x.astype(np.float32)
    top = float(np.iinfo(dtype).max)
    with np.errstate(invalid="ignore"):
        pos = x > 0                                   # NaN: False
        hi = pos & (x >= top)
        mid = pos & ~hi
    out = np.zeros(x.shape, dtype=dtype)
    out[hi] = int(top)
    out[mid] = (x[mid] + 0.5).astype(np.int64).astype(dtype)      # astype(int64) truncates, as (int) does
    return out


def _f64(I):
    return np.ascontiguousarray(np.asarray(I).astype(np.float64))


def warp_parts(orc, src, flo, occ=None):
    """-> (keep (ny, nx) bool, left (ny, nx) bool: the vector leaves the frame, samples (ny, nx, nz) float64 before conv)"""
    ny, nx, _ = src.shape
    i, j = _grid(ny, nx)
    u, v = flo[..., 0].astype(np.float64), flo[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ins = inside(j + u, i + v, nx, ny)
    keep = ins if occ is None else ins & (np.asarray(occ) == 0)
    return keep, ~ins, sample(orc, _f64(src), u, v, keep)


def warp(orc, src, flo, occ=None, fill=None):
    keep, _, smp = warp_parts(orc, src, flo, occ)
    other = np.zeros_like(src) if fill is None else np.asarray(fill)
    return np.where(keep[..., None], conv(smp, src.dtype), other)


def interp_parts(orc, A, B, fwd, bwd, t):
    """-> (ina, inb (ny, nx) bool, o (ny, nx, nz) float64 before conv)"""
    ny, nx, _ = A.shape
    i, j = _grid(ny, nx)
    t = np.float64(t)
    s = np.float64(1.0) - t
    c0, c1, c2 = s * t, t * t, s * s
    u01, v01 = fwd[..., 0].astype(np.float64), fwd[..., 1].astype(np.float64)
    u10, v10 = bwd[..., 0].astype(np.float64), bwd[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dxa, dya = c1 * u10 - c0 * u01, c1 * v10 - c0 * v01
        dxb, dyb = c2 * u01 - c0 * u10, c2 * v01 - c0 * v10
        ina = inside(j + dxa, i + dya, nx, ny)
        inb = inside(j + dxb, i + dyb, nx, ny)
    A64, B64 = _f64(A), _f64(B)
    sa = sample(orc, A64, dxa, dya, ina)
    sb = sample(orc, B64, dxb, dyb, inb)
    both, none = (ina & inb)[..., None], (~ina & ~inb)[..., None]
    o = np.where(both, s * sa + t * sb, np.where(none, s * A64 + t * B64, np.where(ina[..., None], sa, sb)))
    return ina, inb, o


def interpolate(orc, A, B, fwd, bwd, t):
    return conv(interp_parts(orc, A, B, fwd, bwd, t)[2], A.dtype)


def tile_use(dx, dy, need, nx, ny):
    """(blocks whose taps fit the LDS tile, blocks that take the global path although they sample) for positions (j + dx, i + dy)
    where `need`: the box rule of csrc/ofx_apply.hip -- the clamped columns x - 1 .. x + 2 and rows y - 1 .. y + 2 of every sample"""
    i, j = _grid(ny, nx)
    x = np.where(need, j + np.where(need, dx, 0.0), 0.0).astype(np.int64)
    y = np.where(need, i + np.where(need, dy, 0.0), 0.0).astype(np.int64)
    fit = miss = 0
    for r0 in range(0, ny, BLOCK[1]):
        for c0 in range(0, nx, BLOCK[0]):
            m = need[r0:r0 + BLOCK[1], c0:c0 + BLOCK[0]]
            if not m.any():
                continue
            bx, by = x[r0:r0 + BLOCK[1], c0:c0 + BLOCK[0]][m], y[r0:r0 + BLOCK[1], c0:c0 + BLOCK[0]][m]
            w = min(bx.max() + 2, nx - 1) - max(bx.min() - 1, 0) + 1
            h = min(by.max() + 2, ny - 1) - max(by.min() - 1, 0) + 1
            if w <= TILE[0] and h <= TILE[1]:
                fit += 1
            else:
                miss += 1
    return fit, miss


# ---- the shared inputs: computed once per process, never modified (read-only arrays) -------------------------------------------------
JUMP = "jump_130x70"
SEQ_CASES = {"seq_64x48": (64, 48, 3), "seq_131x77": (131, 77, 4)}         # synth.sequence(nx, ny, 3), TV-L1 scales
SIZES = {"p1_64x48": (64, 48), "p1_37x29": (37, 29), JUMP: (130, 70)}
SIZES.update({k: v[:2] for k, v in fcr.NOISE_CASES.items()})
SIZES.update({k: v[:2] for k, v in SEQ_CASES.items()})
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def seq_frames(synth, name):
    """frames 0, 1, 2 of the named sequence as (ny, nx, 1) float64: A, the true in-between frame, B"""
    nx, ny, _ = SEQ_CASES[name]
    return _once(("seqf", name), lambda: tuple(_frozen(np.ascontiguousarray(f[..., None])) for f in synth.sequence(nx, ny, 3)))


def payloads(orc, synth, name):
    """(forward, backward) payload of a named case"""
    if name == JUMP:
        def make():
            f, b = fcr.noise_payloads("130x70")
            f, b = f.copy(), b.copy()
            f[:35, 80:, 0] += 40.0                     # upper half: the right part jumps 40 pixels to the right ...
            b[:35, 40:112, 0] -= 40.0                  # ... and a band of the backward flow 40 pixels to the left
            return _frozen(f), _frozen(b)
        return _once(("flo", name), make)
    if name in SEQ_CASES:
        def make():
            nx, ny, nscales = SEQ_CASES[name]
            A, _, B = seq_frames(synth, name)
            uf, vf = orc.tvl1_multiscale(A[..., 0], B[..., 0], nscales=nscales)[:2]
            ub, vb = orc.tvl1_multiscale(B[..., 0], A[..., 0], nscales=nscales)[:2]
            return _frozen(fcr.payload(uf, vf)), _frozen(fcr.payload(ub, vb))
        return _once(("flo", name), make)
    return fcr.case_payloads(orc, synth, name)


def occ_maps(orc, synth, name):
    """(forward, backward) consistency map of a named case, default thresholds"""
    if name in fcr.ALL_CASES:
        return fcr.case_maps(orc, synth, name)[:2]
    return _once(("occ", name), lambda: tuple(_frozen(m) for m in fcr.maps(orc, *payloads(orc, synth, name))[:2]))


def frames(synth, name, nz, kind):
    """(A, B) of a named case as (ny, nx, nz) arrays of the kind.  The sequence cases: frames 0 and 2 (nz = 1); the others:
    synth.colour_pair("P1").  f64: the values as they are.  f32: a hundredth of them (values that are no integers).  u8: stretched by
    2 about 127.5 and clipped, so that flat runs of 0 and of 255 exist and samples beside them overshoot; u16: 257 times the bytes."""
    def make():
        nx, ny = SIZES[name]
        if name in SEQ_CASES:
            assert nz == 1
            A, _, B = seq_frames(synth, name)
        else:
            A, B = synth.colour_pair("P1", nx, ny, nz)

        def cast(p):
            if kind == "f64":
                return np.array(p)
            if kind == "f32":
                return (p * 0.01).astype(np.float32)
            q = np.clip(np.floor(2.0 * (p - 127.5) + 127.5), 0.0, 255.0)
            return q.astype(np.uint8) if kind == "u8" else (q * 257.0).astype(np.uint16)
        return _frozen(np.ascontiguousarray(cast(A))), _frozen(np.ascontiguousarray(cast(B)))
    return _once(("frames", name, nz, kind), make)


def want_warp(orc, synth, name, nz, kind, with_map=True, with_fill=True):
    """frame B of the case warped onto A's grid by the forward payload, flagged pixels from A: the restatement, computed once"""
    def make():
        A, B = frames(synth, name, nz, kind)
        occ = occ_maps(orc, synth, name)[0] if with_map else None
        return _frozen(warp(orc, B, payloads(orc, synth, name)[0], occ, A if with_fill else None))
    return _once(("warp", name, nz, kind, with_map, with_fill), make)


def want_interp(orc, synth, name, nz, kind, t):
    def make():
        A, B = frames(synth, name, nz, kind)
        return _frozen(interpolate(orc, A, B, *payloads(orc, synth, name), t))
    return _once(("interp", name, nz, kind, float(t)), make)
