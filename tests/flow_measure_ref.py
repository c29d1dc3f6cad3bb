"""ofx_flow_error_dev, ofx_flow_encode_dev and ofx_flow_decode_dev (include/ofx.h) restated in numpy, and the inputs that the tests of
them share.

A payload is an (ny, nx, 2) float32 array, a map an (ny, nx) uint8 array (0 = valid) or None, a record 16 float64.  All arithmetic
in float64, one rounding per operation, association as written in the header:

    fin(x) = x - x == 0;  shown(u, v) = fin(u) && fin(v) && |u| <= 1e9 && |v| <= 1e9
    known = map byte 0 && shown(gu, gv);  bad = known && !(fin(u) && fin(v));  good = known && !bad
    the three sums: sum64 (track_seed_ref) over the rows of sum64 over a row's terms (flow_motion_ref.total); a pixel that is not
    good contributes +0.0
numpy's elementwise float64 operations round once each and contract nothing; np.sqrt and / are correctly rounded.  np.arccos and
np.arctan2 are the C library's: the tests compare the two entries of the record that hold an acos at 1e-12 relative, and the wheel
under the three-way rule of wheel3()."""
import numpy as np

from flow_motion_ref import flags, total  # noqa: F401  (flags: the maps the tests use)

F = np.float64
REC = 16
WHEEL_RGB8, BOUND_U8, KITTI_U16 = 1, 2, 3
UNKNOWN = 1e9
DEG = 57.29577951308232
PI = 3.141592653589793
QNAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), dtype=np.float32)[0]
# Middlebury's R0.5 R1 R2 R3 R5 and KITTI's Fl, as the front-end flow_error asks for them
THR_ABS = (0.5, 1.0, 2.0, 3.0, 5.0, 3.0)
THR_REL = (0.0, 0.0, 0.0, 0.0, 0.0, 0.05)
_quiet = dict(invalid="ignore", over="ignore", divide="ignore")


def fin(x):
    with np.errstate(**_quiet):
        return x - x == 0.0


def shown(u, v):
    with np.errstate(**_quiet):
        return fin(u) & fin(v) & (np.abs(u) <= UNKNOWN) & (np.abs(v) <= UNKNOWN)


def _uv(flo):
    return flo[..., 0].astype(F), flo[..., 1].astype(F)


def classes(flo, gt, occ):
    """-> known, bad, good (ny, nx) bool"""
    u, v = _uv(flo)
    gu, gv = _uv(gt)
    known = shown(gu, gv) if occ is None else shown(gu, gv) & (occ == 0)
    bad = known & ~(fin(u) & fin(v))
    return known, bad, known & ~bad


def pixel_terms(flo, gt):
    """-> e, e2, ae, gm (ny, nx) float64 of every pixel as if it were good"""
    u, v = _uv(flo)
    gu, gv = _uv(gt)
    with np.errstate(**_quiet):
        du, dv = u - gu, v - gv
        e2 = du * du + dv * dv
        e = np.sqrt(e2)
        gm = np.sqrt(gu * gu + gv * gv)
        num = (u * gu + v * gv) + 1.0
        den = np.sqrt((u * u + v * v) + 1.0) * np.sqrt((gu * gu + gv * gv) + 1.0)
        c = num / den
        c = np.where(c > 1.0, 1.0, c)
        c = np.where(c < -1.0, -1.0, c)
    return e, e2, c, gm


def error(flo, gt, occ=None, thr_abs=(), thr_rel=(), n_bins=0, bin_w=0.0):
    """-> record (16,) float64, EPE map (ny, nx) float32, histogram (n_bins,) uint32 (None where n_bins is 0)"""
    known, bad, good = classes(flo, gt, occ)
    e, e2, c, gm = pixel_terms(flo, gt)
    ae = np.arccos(np.where(good, c, 1.0))
    Se, S2, Sa = (total(np.where(good, t, 0.0)) for t in (e, e2, ae))
    rec = np.zeros(REC)
    rec[0], rec[1] = np.count_nonzero(known), np.count_nonzero(bad)
    ng = F(rec[0] - rec[1])
    if ng > 0:
        rec[2] = Se / ng
        rec[3] = np.sqrt(S2 / ng)
        rec[4] = (Sa / ng) * F(DEG)
        rec[5] = np.max(e[good])
        rec[6], rec[7] = Se, Sa
    with np.errstate(**_quiet):
        for k in range(len(thr_abs)):
            rec[8 + k] = np.count_nonzero(bad | (good & (e > F(thr_abs[k])) & (e > F(thr_rel[k]) * gm)))
    with np.errstate(**_quiet):
        epe = np.where(good, e, np.where(bad, np.inf, 0.0)).astype(np.float32)
    epe[~known] = QNAN
    hist = None
    if n_bins:
        with np.errstate(**_quiet):
            q = e / F(bin_w)
        inside = good & (q < n_bins)
        bins = np.where(inside, np.where(inside, q, 0.0).astype(np.int64), n_bins - 1)
        hist = np.bincount(bins[known], minlength=n_bins).astype(np.uint32)
    return rec, epe, hist


def percentile_edge(hist, known, p, bin_w):
    """the upper edge of the bin at which the cumulative count reaches ceil(p * known), as the front-end flow_error reads it"""
    need = np.ceil(F(p) * F(known))
    cum = 0.0
    for b in range(len(hist)):
        cum += float(hist[b])
        if known > 0 and cum >= need:
            return F(b + 1) * F(bin_w)
    return F(0.0)


# ---- the encodings ----------------------------------------------------------------------------------------------------------------
def wheel_table():
    """the 55 integer RGB entries: RY 15, YG 6, GC 4, CB 11, BM 13, MR 6, integer divisions"""
    w = []
    w += [(255, 255 * i // 15, 0) for i in range(15)]
    w += [(255 - 255 * i // 6, 255, 0) for i in range(6)]
    w += [(0, 255, 255 * i // 4) for i in range(4)]
    w += [(0, 255 - 255 * i // 11, 255) for i in range(11)]
    w += [(255 * i // 13, 0, 255) for i in range(13)]
    w += [(255, 0, 255 - 255 * i // 6) for i in range(6)]
    return np.array(w, dtype=np.int64)


WHEEL = wheel_table()


def vis(flo, occ):
    u, v = _uv(flo)
    return shown(u, v) if occ is None else shown(u, v) & (occ == 0)


def maxrad_of(flo, occ, scale):
    if scale > 0:
        return F(scale)
    u, v = _uv(flo)
    ok = vis(flo, occ)
    with np.errstate(**_quiet):
        rad = np.sqrt(u * u + v * v)
    m = F(np.max(rad[ok])) if ok.any() else F(0.0)
    return m if m != 0.0 else F(1.0)


def encode_wheel(flo, occ=None, scale=0.0, da=0.0):
    """-> (ny, nx, 3) uint8; da: added to a = atan2(-fy, -fx) / pi, the sum clamped to [-1, 1]"""
    u, v = _uv(flo)
    ok = vis(flo, occ)
    mr = maxrad_of(flo, occ, scale)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    with np.errstate(**_quiet):
        fx, fy = u / mr, v / mr
        rad = np.sqrt(fx * fx + fy * fy)
        a = np.arctan2(-fy, -fx) / F(PI)
        if da != 0.0:
            a = np.clip(a + F(da), -1.0, 1.0)
        fk = (a + 1.0) / 2.0 * 54.0
        k0 = fk.astype(np.int64)
        k1 = (k0 + 1) % 55
        f = fk - k0
        out = np.zeros(u.shape + (3,), dtype=np.uint8)
        for b in range(3):
            c0, c1 = WHEEL[k0, b] / 255.0, WHEEL[k1, b] / 255.0
            col = (1.0 - f) * c0 + f * c1
            col = np.where(rad <= 1.0, 1.0 - rad * (1.0 - col), col * 0.75)
            out[..., b] = np.where(ok, (255.0 * col).astype(np.int64), 0)
    return out


def wheel3(flo, occ=None, scale=0.0, eps=1e-12):
    """-> the three restatements (da = 0, -eps, +eps) and the mask of the pixels at which they do not all agree"""
    three = [encode_wheel(flo, occ, scale, da) for da in (0.0, -eps, eps)]
    differ = (three[0] != three[1]).any(axis=-1) | (three[0] != three[2]).any(axis=-1)
    return three, differ


def wheel_ok(got, flo, occ=None, scale=0.0):
    """the three-way rule: where the three agree, `got` equals them; elsewhere it equals one of them -> (ok, exempted pixels)"""
    three, differ = wheel3(flo, occ, scale)
    same = [(got == t).all(axis=-1) for t in three]
    ok = np.where(differ, same[0] | same[1] | same[2], same[0])
    return bool(ok.all()), int(np.count_nonzero(differ))


def encode_bound(flo, occ=None, B=20.0):
    """-> (ny, nx, 2) uint8"""
    ok = vis(flo, occ)
    B = F(B)
    out = np.zeros(flo.shape, dtype=np.uint8)
    for k, f in enumerate(_uv(flo)):
        f = np.where(ok, f, 0.0)
        code = (255.0 * (f + B) / (2.0 * B) + 0.5).astype(np.int64)
        out[..., k] = np.where(f <= -B, 0, np.where(f >= B, 255, code))
    return out


def decode_bound(code, B):
    B = F(B)
    return ((code.astype(F) * (2.0 * B)) / 255.0 - B).astype(np.float32), np.zeros(code.shape[:2], dtype=np.uint8)


def encode_kitti(flo, occ=None):
    """-> (ny, nx, 3) uint16"""
    ok = vis(flo, occ)
    out = np.zeros(flo.shape[:2] + (3,), dtype=np.uint16)
    for k, f in enumerate(_uv(flo)):
        x = np.where(ok, f, 0.0) * 64.0 + 32768.0
        q = np.where(x <= 0.0, 0, np.where(x >= 65535.0, 65535, (np.clip(x, 0.0, 65535.0) + 0.5).astype(np.int64)))
        out[..., k] = np.where(ok, q, 0)
    out[..., 2] = ok
    return out


def decode_kitti(code):
    """-> payload (ny, nx, 2) float32, map (ny, nx) uint8"""
    valid = code[..., 2] != 0
    flo = ((code[..., :2].astype(F) - 32768.0) / 64.0).astype(np.float32)
    flo[~valid] = QNAN
    return flo, np.where(valid, 0, 255).astype(np.uint8)


# ---- the shared inputs: computed once per process, never modified ----------------------------------------------------------------------
_cache = {}


def field(nx, ny):
    """-> u, v (ny, nx) float32"""
    i, j = np.meshgrid(np.arange(ny, dtype=F), np.arange(nx, dtype=F), indexing="ij")
    u = 6 * np.sin(0.11 * j + 0.05 * i) + 0.03 * (j - nx / 2)
    v = 4 * np.cos(0.07 * i - 0.02 * j) - 0.02 * (i - ny / 2)
    return u.astype(np.float32), v.astype(np.float32)


def truth(nx, ny):
    """field() as a payload"""
    key = ("truth", nx, ny)
    if key not in _cache:
        p = np.stack(field(nx, ny), axis=-1)
        p.setflags(write=False)
        _cache[key] = p
    return _cache[key]


def estimate(nx, ny, seed=0, sigma=0.8):
    """truth() with noise of sigma px per component and a block that is 6 px off"""
    key = ("estimate", nx, ny, seed, sigma)
    if key not in _cache:
        rng = np.random.default_rng(300 + seed)
        p = np.array(truth(nx, ny), dtype=F) + rng.normal(0.0, sigma, (ny, nx, 2))
        p[: max(1, ny // 3), : max(1, nx // 4), 0] += 6.0
        p = p.astype(np.float32)
        p.setflags(write=False)
        _cache[key] = p
    return _cache[key]


def spoiled(flo, seed=0):
    """the payload with NaN, Inf and 1e10 vectors scattered over a twelfth of it"""
    rng = np.random.default_rng(400 + seed)
    out = np.array(flo)
    ny, nx, _ = out.shape
    k = rng.random((ny, nx))
    out[k < 0.02, 0] = np.nan
    out[(k >= 0.02) & (k < 0.04), 1] = np.inf
    out[(k >= 0.04) & (k < 0.06)] = (1e10, 1e10)
    out[(k >= 0.06) & (k < 0.08), 1] = -1e10
    out[(k >= 0.08) & (k < 0.085)] = (-np.inf, np.nan)
    return out
