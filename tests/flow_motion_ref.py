"""ofx_flow_motion_fit_dev and ofx_flow_motion_apply_dev (include/ofx.h) restated in numpy, and the inputs that the tests of them
share.

A payload is an (ny, nx, 2) float32 array, a map an (ny, nx) uint8 array (0 = valid) or None, a record 16 float64.  All arithmetic
in float64, one rounding per operation, as written in the header:

    cx = 0.5 * (nx - 1);  cy = 0.5 * (ny - 1);  h = 0.5 * max(nx, ny);  X = (j - cx) / h;  Y = (i - cy) / h
    mu = (t0 + a * X) + b * Y;  mv = (t1 + c * X) + d * Y
    valid = map byte 0 and u - u == 0 and v - v == 0
    du = u - mu;  dv = v - mv;  r2 = du * du + dv * dv;  C2 = C * C;  r2 < C2: q = 1 - r2 / C2, w = q * q;  else w = 0
    the twelve moments: sum64 (track_seed_ref) over the rows of sum64 over a row's terms; an invalid pixel's term is +0.0
    solve(), record(), fit(): the words of the header, below
numpy's elementwise float64 operations round once each and contract nothing.  sum64_rows() is sum64 on every row of a plane at
once, the same additions in the same order (tests/test_flow_motion_ref.py holds it to sum64 bit for bit)."""
import numpy as np

from track_seed_ref import sum64

TRANSLATION, SIMILARITY, AFFINE = 2, 4, 6
EPS = 1e-12
F = np.float64


def grid(nx, ny):
    """-> X (nx,), Y (ny,), cx, cy, h"""
    cx, cy, h = F(0.5) * F(nx - 1), F(0.5) * F(ny - 1), F(0.5) * F(max(nx, ny))
    return (np.arange(nx, dtype=F) - cx) / h, (np.arange(ny, dtype=F) - cy) / h, cx, cy, h


def model_flow(theta, nx, ny):
    """-> mu, mv (ny, nx) float64"""
    X, Y, _, _, _ = grid(nx, ny)
    t0, a, b, t1, c, d = [F(t) for t in theta]
    with np.errstate(invalid="ignore", over="ignore"):
        return (t0 + a * X)[None, :] + (b * Y)[:, None], (t1 + c * X)[None, :] + (d * Y)[:, None]


def model_payload(theta, nx, ny):
    mu, mv = model_flow(theta, nx, ny)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([mu, mv], axis=-1).astype(np.float32)


def valid(flo, occ):
    u, v = flo[..., 0].astype(F), flo[..., 1].astype(F)
    with np.errstate(invalid="ignore"):
        ok = (u - u == 0.0) & (v - v == 0.0)
    return ok if occ is None else ok & (occ == 0)


def residual(flo, theta):
    """-> du, dv, r2 (ny, nx) float64"""
    ny, nx, _ = flo.shape
    mu, mv = model_flow(theta, nx, ny)
    with np.errstate(invalid="ignore", over="ignore"):
        du, dv = flo[..., 0].astype(F) - mu, flo[..., 1].astype(F) - mv
        return du, dv, du * du + dv * dv


def weights(flo, theta, C):
    """Tukey's biweight of every pixel as if it were valid (the moments leave the invalid ones out)"""
    _, _, r2 = residual(flo, theta)
    C2 = F(C) * F(C)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = 1.0 - r2 / C2
        return np.where(r2 < C2, q * q, 0.0)


def sum64_rows(A):
    """sum64 of every row of A (ny, n) -> (ny,)"""
    A = np.asarray(A, dtype=F)
    ny, n = A.shape
    p = np.zeros((ny, 64))
    k = min(64, n)
    p[:, :k] = A[:, :k]
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(64, n, 64):
            seg = A[:, j0:j0 + 64]
            p[:, :seg.shape[1]] = p[:, :seg.shape[1]] + seg
        s = 32
        while s >= 1:
            p[:, :s] = p[:, :s] + p[:, s:2 * s]
            s //= 2
    return p[:, 0].copy()


def total(T):
    return F(sum64(sum64_rows(T)))


def moments(flo, occ, w=None):
    """the twelve moments in the header's order: S1 SX SY SXX SXY SYY U1 UX UY V1 VX VY; w None: the unweighted fit"""
    ny, nx, _ = flo.shape
    X, Y, _, _, _ = grid(nx, ny)
    X, Y = np.broadcast_to(X[None, :], (ny, nx)), np.broadcast_to(Y[:, None], (ny, nx))
    u, v = flo[..., 0].astype(F), flo[..., 1].astype(F)
    ok = valid(flo, occ)
    if w is None:
        w = np.ones((ny, nx))
    with np.errstate(invalid="ignore", over="ignore"):
        wX, wY, wu, wv = w * X, w * Y, w * u, w * v
        terms = [w, wX, wY, wX * X, wX * Y, wY * Y, wu, wu * X, wu * Y, wv, wv * X, wv * Y]
    return [total(np.where(ok, t, 0.0)) for t in terms]


def solve(model, S):
    """-> theta (6,) float64, or None where the fit is degenerate"""
    S1, SX, SY, SXX, SXY, SYY, U1, UX, UY, V1, VX, VY = S
    if not S1 > 0.0:
        return None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if model == TRANSLATION:
            return np.array([U1 / S1, 0.0, 0.0, V1 / S1, 0.0, 0.0])
        if model == SIMILARITY:
            Q = SXX + SYY
            D = Q - (SX * SX + SY * SY) / S1
            if not D > EPS * Q:
                return None
            a = ((UX + VY) - (SX * U1 + SY * V1) / S1) / D
            c = ((VX - UY) - (SX * V1 - SY * U1) / S1) / D
            t0 = ((U1 - SX * a) + SY * c) / S1
            t1 = ((V1 - SY * a) - SX * c) / S1
            return np.array([t0, a, -c, t1, c, a])
        assert model == AFFINE
        l10, l20 = SX / S1, SY / S1
        a11, a12, a22 = SXX - l10 * SX, SXY - l10 * SY, SYY - l20 * SY
        if not a11 > EPS * SXX:
            return None
        l21 = a12 / a11
        p2 = a22 - l21 * a12
        if not p2 > EPS * SYY:
            return None
        th = []
        for r0, r1, r2 in ((U1, UX, UY), (V1, VX, VY)):
            y1 = r1 - l10 * r0
            y2 = (r2 - l20 * r0) - l21 * y1
            z2 = y2 / p2
            z1 = (y1 - a12 * z2) / a11
            z0 = ((r0 - SX * z1) - SY * z2) / S1
            th += [z0, z1, z2]
        return np.array(th)


def record(theta, nx, ny, s1, done, c_last, stopped):
    _, _, cx, cy, h = grid(nx, ny)
    rec = np.zeros(16)
    rec[:6] = theta
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(2):
            t, a, b = [F(x) for x in theta[3 * k:3 * k + 3]]
            p1, p2 = a / h, b / h
            rec[6 + 3 * k:9 + 3 * k] = (t - p1 * cx) - p2 * cy, p1, p2
    rec[12:] = s1, done, c_last, 1.0 if stopped else 0.0
    return rec


def cutoff(t, c_first, c_last):
    return max(F(c_last), F(np.ldexp(F(c_first), -t)))


def fit(flo, occ, model, n_fits, c_first, c_last, init=None):
    """-> the record (16,) float64"""
    ny, nx, _ = flo.shape
    theta = np.zeros(6) if init is None else np.array(init[:6], dtype=F)
    s1, done, stopped = F(0.0), 0, False
    for f in range(n_fits):
        if init is None and f == 0:
            w = None
        else:
            w = weights(flo, theta, cutoff(f if init is not None else f - 1, c_first, c_last))
        S = moments(flo, occ, w)
        new = solve(model, S)
        if new is None:
            stopped = True
            break
        theta, s1, done = new, S[0], f + 1
    return record(theta, nx, ny, s1, done, c_last, stopped)


def outputs(theta, C, flo, occ=None):
    """-> model payload, residual payload, inlier map under theta and the cut-off C"""
    ny, nx, _ = flo.shape
    du, dv, r2 = residual(flo, theta)
    with np.errstate(invalid="ignore", over="ignore"):
        res = np.stack([du, dv], axis=-1).astype(np.float32)
        inl = np.where(valid(flo, occ) & (r2 < F(C) * F(C)), 0, 255).astype(np.uint8)
    return model_payload(theta, nx, ny), res, inl


def mean_epe(theta, truth, nx, ny):
    mu, mv = model_flow(theta, nx, ny)
    tu, tv = model_flow(truth, nx, ny)
    return float(np.mean(np.hypot(mu - tu, mv - tv)))


# ---- the shared inputs: computed once per process, never modified ----------------------------------------------------------------------
TRUE = {AFFINE: (1.5, 2.0, -1.25, -0.75, 0.5, 1.75), SIMILARITY: (1.5, 2.0, -0.5, -0.75, 0.5, 2.0), TRANSLATION: (1.5, 0.0, 0.0, -0.75, 0.0, 0.0)}
MOVE = (8.0, 5.0)
_cache = {}


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def foreground(nx, ny):
    """a rectangle that covers 30 % of the pixels"""
    fg = np.zeros((ny, nx), dtype=bool)
    i0, j0 = ny // 5, nx // 4
    fg[i0:i0 + (ny + 1) // 2, j0:j0 + int(round(0.6 * nx))] = True
    return fg


def scene(nx, ny, model=AFFINE, seed=5, sigma=0.1):
    """a camera flow of TRUE[model] with noise of sigma px per component, and a rectangle that moves by MOVE on top of it
    -> (payload, foreground mask)"""
    key = ("scene", nx, ny, model, seed, sigma)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        mu, mv = model_flow(TRUE[model], nx, ny)
        fg = foreground(nx, ny)
        u = mu + rng.normal(0.0, sigma, (ny, nx)) + np.where(fg, MOVE[0], 0.0)
        v = mv + rng.normal(0.0, sigma, (ny, nx)) + np.where(fg, MOVE[1], 0.0)
        _cache[key] = _frozen(np.stack([u, v], axis=-1).astype(np.float32), fg)
    return _cache[key]


def flags(nx, ny, seed=0):
    """a map that flags a scattering of pixels and a block"""
    key = ("flags", nx, ny, seed)
    if key not in _cache:
        rng = np.random.default_rng(100 + seed)
        m = np.where(rng.random((ny, nx)) < 0.1, rng.integers(1, 256, (ny, nx)), 0).astype(np.uint8)
        m[ny // 2:, :max(1, nx // 5)] = 255
        _cache[key] = _frozen(m)[0]
    return _cache[key]


def nonfinite(flo, seed=0):
    """the payload with NaN and Inf vectors scattered over a twentieth of it"""
    rng = np.random.default_rng(200 + seed)
    out = np.array(flo)
    ny, nx, _ = out.shape
    k = rng.random((ny, nx))
    out[k < 0.02, 0] = np.nan
    out[(k >= 0.02) & (k < 0.03), 1] = np.inf
    out[(k >= 0.03) & (k < 0.04)] = (-np.inf, np.nan)
    out[(k >= 0.04) & (k < 0.05), 0] = -np.inf
    return out
