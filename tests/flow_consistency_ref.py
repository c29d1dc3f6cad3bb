"""The forward-backward consistency check of ofx_flow_consistency_dev (include/ofx.h) restated in numpy, and the payloads that the
tests of it share.

A payload is an (ny, nx, 2) float32 array, (u, v) interleaved: forward = A -> B on A's grid, backward = B -> A on B's grid.
The forward map at row i, column j, all in float64, one rounding per operation, association as written:

    u, v = F[i, j];  xt = j + u;  yt = i + v
    255 unless 0 <= xt <= nx - 1 and 0 <= yt <= ny - 1                       (NaN and Inf land here)
    bu, bv = Oracle.bicubic_at_color(B, xt, yt, k = 0 / 1, border_out = False)
    du = u + bu;  dv = v + bv
    0 if du du + dv dv <= alpha ((u u + v v) + (bu bu + bv bv)) + beta else 255   (a NaN anywhere: 255)

and the backward map is the same with the payloads exchanged.  numpy's elementwise float64 operations round once each and
contract nothing, so the expressions below are that definition; the two samples are the oracle's bicubic_at_color, i.e. the
reference's bicubic_interpolation_at_color."""
import numpy as np

ALPHA, BETA = 0.01, 0.5          # Sundaram, Brox, Keutzer (ECCV 2010)


def one_map(orc, F, B, alpha=ALPHA, beta=BETA):
    """-> (map (ny, nx) uint8, smallest |lhs - rhs| / rhs over the pixels that reach the comparison with rhs > 0; inf if none)"""
    F = np.asarray(F)
    B = np.asarray(B)
    assert F.dtype == np.float32 and B.dtype == np.float32 and F.shape == B.shape and F.shape[2] == 2
    ny, nx, _ = F.shape
    B64 = np.ascontiguousarray(B.astype(np.float64))
    u = F[..., 0].astype(np.float64)
    v = F[..., 1].astype(np.float64)
    i, j = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        xt = j + u
        yt = i + v
        inside = (xt >= 0) & (xt <= nx - 1) & (yt >= 0) & (yt <= ny - 1)
        bu = np.zeros((ny, nx))
        bv = np.zeros((ny, nx))
        for r, c in np.argwhere(inside):
            bu[r, c] = orc.bicubic_at_color(B64, float(xt[r, c]), float(yt[r, c]), 0)
            bv[r, c] = orc.bicubic_at_color(B64, float(xt[r, c]), float(yt[r, c]), 1)
        du = u + bu
        dv = v + bv
        lhs = du * du + dv * dv
        rhs = alpha * ((u * u + v * v) + (bu * bu + bv * bv)) + beta
        ok = inside & (lhs <= rhs)
        sel = inside & np.isfinite(lhs) & np.isfinite(rhs) & (rhs > 0)
        margin = float(np.min(np.abs(lhs[sel] - rhs[sel]) / rhs[sel])) if sel.any() else float("inf")
    return np.where(ok, 0, 255).astype(np.uint8), margin


def maps(orc, fwd, bwd, alpha=ALPHA, beta=BETA):
    """-> (forward map, backward map, smallest relative margin of the two)"""
    of, mf = one_map(orc, fwd, bwd, alpha, beta)
    ob, mb = one_map(orc, bwd, fwd, alpha, beta)
    return of, ob, min(mf, mb)


def payload(u, v):
    return np.ascontiguousarray(np.stack([u, v], axis=-1).astype(np.float32))


# ---- the shared inputs: computed once per process, never modified (read-only arrays) -------------------------------------------------
TVL1_CASES = {"p1_64x48": ("P1", 64, 48, 3), "p1_37x29": ("P1", 37, 29, 2)}
# (nx, ny, amplitude of the sine fields in pixels, seed); the noise is 0.2 / (4 / 15) of the amplitude: 0.3 px and 0.4 px at 1.5 px
NOISE_CASES = {"3x5": (3, 5, 1.5, 3), "67x5": (67, 5, 1.5, 1), "131x3": (131, 3, 1.5, 1), "64x64": (64, 64, 1.5, 1),
               "130x70": (130, 70, 1.5, 1), "2x2": (2, 2, 0.3, 1)}
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def tvl1_payloads(orc, synth, name):
    """the oracle's TV-L1 flows of the named pair in both directions, as float32 payloads"""
    key = ("tvl1", name)
    if key not in _cache:
        pair, nx, ny, nscales = TVL1_CASES[name]
        A, B = synth.pair(pair, nx, ny)
        uf, vf = orc.tvl1_multiscale(A, B, nscales=nscales)[:2]
        ub, vb = orc.tvl1_multiscale(B, A, nscales=nscales)[:2]
        _cache[key] = (_frozen(payload(uf, vf)), _frozen(payload(ub, vb)))
    return _cache[key]


def noise_payloads(name):
    """smooth sine fields plus Gaussian noise; the backward payload is the negated forward one plus more noise"""
    key = ("noise", name)
    if key not in _cache:
        nx, ny, amp, seed = NOISE_CASES[name]
        rng = np.random.default_rng(seed)
        i, j = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
        u = amp * np.sin(0.31 * j + 0.17 * i + 0.5) + rng.normal(0.0, 0.2 * amp, (ny, nx))
        v = amp * np.cos(0.23 * i - 0.11 * j + 0.2) + rng.normal(0.0, 0.2 * amp, (ny, nx))
        ub = -u + rng.normal(0.0, amp * 4.0 / 15.0, (ny, nx))
        vb = -v + rng.normal(0.0, amp * 4.0 / 15.0, (ny, nx))
        _cache[key] = (_frozen(payload(u, v)), _frozen(payload(ub, vb)))
    return _cache[key]


def case_payloads(orc, synth, name):
    return tvl1_payloads(orc, synth, name) if name in TVL1_CASES else noise_payloads(name)


def case_maps(orc, synth, name):
    """(forward map, backward map, margin) of a named case with the default thresholds, computed once"""
    key = ("maps", name)
    if key not in _cache:
        f, b = case_payloads(orc, synth, name)
        of, ob, m = maps(orc, f, b)
        _cache[key] = (_frozen(of), _frozen(ob), m)
    return _cache[key]


ALL_CASES = tuple(TVL1_CASES) + tuple(NOISE_CASES)
