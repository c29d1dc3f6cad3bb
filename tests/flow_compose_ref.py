"""ofx_flow_compose_dev, ofx_flow_accumulate_dev and ofx_flow_tracks_dev (include/ofx.h) restated in numpy, and the inputs that the
tests of them share.

A payload is an (ny, nx, 2) float32 array, (u, v) interleaved; a map an (ny, nx) uint8 array, 0 = valid; query points an (n_pts, 2)
float64 array of (x, y).  All arithmetic in float64, one rounding per operation, association as written:

    inside(x, y)     = x >= 0 and x <= nx - 1 and y >= 0 and y <= ny - 1                     (NaN and Inf fail it)
    sample(S, x, y)  = the reference's bicubic_interpolation_at_color(S, x, y, nx, ny, 2, 0 / 1, false) restated below in numpy
                       (taps, cubic_cell): no oracle is needed, tests/test_flow_compose_ref.py pins it to the oracle's bits
    flagged(M, x, y) = x0 = int(x), x1 = x0 + (x > x0), y0 = int(y), y1 = y0 + (y > y0); any of M[y0, x0], M[y0, x1], M[y1, x0],
                       M[y1, x1] non-zero; False without a map
    advance(p, S, M) = flagged -> lost;  q = p + sample(S, p);  not inside(q) -> lost;  else the point moves to q

compose:   (U, V) = ab[i, j] (zeros without ab);  m = occ_ab[i, j] (0 without it)
           m != 0 or not inside(j + U, i + V):              ac = ab bit for bit, occ_ac = 255
           f = flagged(occ_bc, j + U, i + V);  (bu, bv) = sample(bc, j + U, i + V);  Un = float32(U + bu);  Vn = float32(V + bv)
           f or not inside(j + Un, i + Vn):                 ac = ab bit for bit, occ_ac = 255
           otherwise:                                       ac = (Un, Vn), occ_ac = 0
accumulate: acc[0] = compose(None, step[0]);  acc[t] = compose(acc[t - 1], step[t]), the lost state handed on
tracks:    p_0 = xy0;  not inside(p_0): len = -1, every p_t = p_0;  p_{t+1} = advance(p_t, step[t], occ[t]) while the point lives;
           the first lost step t: len = t, later positions repeat p_t;  a survivor: len = n_steps
numpy's elementwise float64 operations round once each and contract nothing, so the expressions below are that definition.  The
positions of pixels that take no sample are replaced by 0 before any cast to int, as the C code never casts them."""
import numpy as np

import flow_apply_ref as far
import flow_consistency_ref as fcr


def _grid(ny, nx):
    return np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")


def inside(x, y, nx, ny):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= nx - 1) & (y >= 0) & (y <= ny - 1)


def cubic_cell(v0, v1, v2, v3, x):
    """src/bicubic_interpolation.cpp:108-123, the Horner form as written"""
    return v1 + 0.5 * x * (v2 - v0 + x * (2.0 * v0 - 5.0 * v1 + 4.0 * v2 - v3 + x * (3.0 * (v1 - v2) + v3 - v0)))


def taps(x, y, nx, ny):
    """src/bicubic_interpolation.cpp:150-245 with border_out = false (Neumann): the four clamped columns and rows -- `my` offset by sx,
    as there -- and the fractions against the clamped base index"""
    sx = np.where(x < 0, -1, 1)
    sy = np.where(y < 0, -1, 1)
    iu, iv = x.astype(np.int64), y.astype(np.int64)                  # truncation toward zero, as (int)
    cx = lambda c: np.clip(c, 0, nx - 1)
    cy = lambda r: np.clip(r, 0, ny - 1)
    col = [cx(iu - sx), cx(iu), cx(iu + sx), cx(iu + 2 * sx)]
    row = [cy(iv - sx), cy(iv), cy(iv + sy), cy(iv + 2 * sy)]
    return col, row, x - col[1], y - row[1]


def sample(S, x, y, ok):
    """(bu, bv) at the positions (x, y) where ok (any shape); 0 elsewhere.  S: a float32 payload"""
    S64 = np.asarray(S).astype(np.float64)
    ny, nx, _ = S64.shape
    xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    col, row, fx, fy = taps(xs, ys, nx, ny)
    fx, fy = fx[..., None], fy[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        c = [cubic_cell(S64[row[0], col[k]], S64[row[1], col[k]], S64[row[2], col[k]], S64[row[3], col[k]], fy) for k in range(4)]
        o = cubic_cell(c[0], c[1], c[2], c[3], fx)
    o = np.where(ok[..., None], o, 0.0)
    return o[..., 0], o[..., 1]


def flagged_parts(M, x, y, ok):
    """-> (flagged, own): flagged where ok and one of the up to four map pixels around (x, y) is non-zero; own: M[y0, x0] is"""
    if M is None:
        z = np.zeros(np.shape(x), dtype=bool)
        return z, z
    M = np.asarray(M)
    xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    x0, y0 = xs.astype(np.int64), ys.astype(np.int64)
    x1, y1 = x0 + (xs > x0), y0 + (ys > y0)
    own = ok & (M[y0, x0] != 0)
    return ok & ((M[y0, x0] | M[y0, x1] | M[y1, x0] | M[y1, x1]) != 0), own


def flagged(M, x, y, ok):
    return flagged_parts(M, x, y, ok)[0]


def compose_parts(ab, bc, occ_ab=None, occ_bc=None):
    """-> (ac, occ_ac, branch): branch an (ny, nx) array of the BR_* codes below"""
    bc = np.asarray(bc)
    assert bc.dtype == np.float32 and bc.shape[2] == 2
    ny, nx, _ = bc.shape
    old = np.zeros((ny, nx, 2), dtype=np.float32) if ab is None else np.asarray(ab)
    assert old.dtype == np.float32 and old.shape == bc.shape
    i, j = _grid(ny, nx)
    U, V = old[..., 0].astype(np.float64), old[..., 1].astype(np.float64)
    m = np.zeros((ny, nx), dtype=bool) if occ_ab is None else np.asarray(occ_ab) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = j + U, i + V
        go = ~m & inside(x, y, nx, ny)
        f, own = flagged_parts(occ_bc, x, y, go)
        bu, bv = sample(bc, x, y, go)
        Un, Vn = (U + bu).astype(np.float32), (V + bv).astype(np.float32)
        arrives = inside(j + Un.astype(np.float64), i + Vn.astype(np.float64), nx, ny)
    ok = go & ~f & arrives
    ac = np.where(ok[..., None], np.stack([Un, Vn], axis=-1), old)
    integer = (x == np.floor(x)) & (y == np.floor(y))
    branch = np.full((ny, nx), BR_OK, dtype=np.uint8)
    branch[go & ~f & ~arrives] = BR_LEAVES_AFTER
    branch[go & ~f & ~arrives & ~(np.isfinite(bu) & np.isfinite(bv))] = BR_NONFINITE
    branch[go & f & ~own] = BR_FLAGGED_NEIGHBOUR
    branch[go & f & own] = BR_FLAGGED_OWN
    branch[go & f & own & integer] = BR_FLAGGED_AT_PIXEL
    branch[~m & ~go] = BR_LEAVES_BEFORE
    branch[m] = BR_FROZEN
    return ac, np.where(ok, 0, 255).astype(np.uint8), branch


# why a vector is lost in one compose: in the order the definition tests them
BR_OK, BR_FROZEN, BR_LEAVES_BEFORE, BR_FLAGGED_AT_PIXEL, BR_FLAGGED_OWN, BR_FLAGGED_NEIGHBOUR, BR_NONFINITE, BR_LEAVES_AFTER = range(8)


def compose(ab, bc, occ_ab=None, occ_bc=None):
    return compose_parts(ab, bc, occ_ab, occ_bc)[:2]


def accumulate(steps, occ_steps=None):
    """-> [(acc_t, occ_acc_t, branch_t)] for t < len(steps)"""
    out, ab, occ = [], None, None
    for t, s in enumerate(steps):
        ab, occ, br = compose_parts(ab, s, occ, None if occ_steps is None else occ_steps[t])
        out.append((ab, occ, br))
    return out


def tracks(steps, xy0, occ_steps=None):
    """-> (xy (n_steps + 1, n_pts, 2) float64, len (n_pts,) int32)"""
    xy0 = np.asarray(xy0, dtype=np.float64)
    n_steps, n_pts = len(steps), xy0.shape[0]
    ny, nx, _ = steps[0].shape
    xy = np.empty((n_steps + 1, n_pts, 2))
    p = xy0.copy()
    xy[0] = p
    alive = inside(p[:, 0], p[:, 1], nx, ny)
    length = np.where(alive, n_steps, -1).astype(np.int32)
    for t, s in enumerate(steps):
        x, y = p[:, 0], p[:, 1]
        go = alive & ~flagged(None if occ_steps is None else occ_steps[t], x, y, alive)
        bu, bv = sample(s, x, y, go)
        with np.errstate(invalid="ignore", over="ignore"):
            qx, qy = x + bu, y + bv
            mv = go & inside(qx, qy, nx, ny)
        length[alive & ~mv] = t
        alive = mv
        p = np.where(mv[:, None], np.stack([qx, qy], axis=-1), p)
        xy[t + 1] = p
    return xy, length


# ---- the shared inputs: computed once per process, never modified (read-only arrays) -------------------------------------------------
JUMP = far.JUMP
MAX_STEPS = 5
# (nx, ny, amplitude of the sine fields in pixels, seed of step 0): step t takes seed + t
CASES = {"2x2": (2, 2, 0.3, 11), "3x5": (3, 5, 1.5, 13), "67x5": (67, 5, 1.5, 21), "131x3": (131, 3, 1.5, 31),
         "37x29": (37, 29, 1.5, 41), "130x70": (130, 70, 1.5, 51), JUMP: (130, 70, 1.5, 61)}
# The step maps are flow_consistency_ref.maps with alpha = 0.01 and beta = STEP_BETA.  The check's residual on these payloads is
# noise by construction: du = u(x) + ub(x + u) = n_f(x) - n_f(x + u) + n_b, Gaussians of sigma 0.3, about 0.3 and 0.4 px, a
# variance of about 0.3 per component, so du^2 + dv^2 exceeds b with a probability near exp(-b / 0.6): the paper's beta = 0.5
# flags close to half of the vectors (0.45 at 130x70), and with the four map pixels around a position 0.1 % of the pixels survive
# four steps, whatever the seeds (0.55 / 0.06 / 0.009 / 0.001 after steps 1 .. 4).  beta = 3 flags about 5 % (with the vectors that
# leave the image), the four neighbours 10 - 15 % per step: 72 % survive four steps.
STEP_ALPHA, STEP_BETA = 0.01, 3.0
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def noise_step(nx, ny, amp, seed):
    """(forward, backward) payload by the formula of flow_consistency_ref.noise_payloads with the seed as a parameter"""
    rng = np.random.default_rng(seed)
    i, j = _grid(ny, nx)
    u = amp * np.sin(0.31 * j + 0.17 * i + 0.5) + rng.normal(0.0, 0.2 * amp, (ny, nx))
    v = amp * np.cos(0.23 * i - 0.11 * j + 0.2) + rng.normal(0.0, 0.2 * amp, (ny, nx))
    ub = -u + rng.normal(0.0, amp * 4.0 / 15.0, (ny, nx))
    vb = -v + rng.normal(0.0, amp * 4.0 / 15.0, (ny, nx))
    return fcr.payload(u, v), fcr.payload(ub, vb)


def _pairs(name):
    def make():
        nx, ny, amp, seed = CASES[name]
        out = [noise_step(nx, ny, amp, seed + t) for t in range(MAX_STEPS)]
        if name == JUMP:
            out[0] = tuple(np.array(p) for p in far.payloads(None, None, JUMP))      # the jump case needs neither oracle nor frames
        return tuple((_frozen(f), _frozen(b)) for f, b in out)
    return _once(("pairs", name), make)


def steps(name, n_steps=MAX_STEPS):
    """the step payloads of a named case"""
    return [p[0] for p in _pairs(name)[:n_steps]]


def step_maps(orc, name, n_steps=MAX_STEPS):
    """the forward consistency maps of the steps (flow_consistency_ref.maps, STEP_ALPHA and STEP_BETA)"""
    full = _once(("maps", name), lambda: tuple(_frozen(fcr.maps(orc, f, b, STEP_ALPHA, STEP_BETA)[0]) for f, b in _pairs(name)))
    return list(full[:n_steps])


def nonfinite_steps(name="37x29"):
    """the steps of a case with a NaN vector in step 1 and an Inf vector in step 2"""
    def make():
        s = [np.array(p) for p in steps(name)]
        ny, nx, _ = s[0].shape
        s[1][ny // 2, nx // 2] = (np.nan, 0.25)
        s[2][ny // 3, nx // 3] = (0.5, np.inf)
        s[2][2, nx - 3] = (-np.inf, np.nan)
        return tuple(_frozen(p) for p in s)
    return list(_once(("nonfinite", name), make))


def constant_steps(nx, ny, n_steps, vec=(2.0, -1.0)):
    return [np.ascontiguousarray(np.broadcast_to(np.array(vec, dtype=np.float32), (ny, nx, 2))) for _ in range(n_steps)]


def smooth_steps(nx, ny, n_steps, amp=1.5):
    """the sine fields alone: steps whose Jacobian has a norm below 1 (the bound of the tracks-against-dense test)"""
    i, j = _grid(ny, nx)
    return [fcr.payload(amp * np.sin(0.31 * j + 0.17 * i + 0.5 + 0.7 * t), amp * np.cos(0.23 * i - 0.11 * j + 0.2 - 0.4 * t))
            for t in range(n_steps)]


def want(orc, name, n_steps, with_maps):
    """accumulate() of a named case, computed once"""
    return _once(("acc", name, n_steps, with_maps),
                 lambda: accumulate(steps(name, n_steps), step_maps(orc, name, n_steps) if with_maps else None))


def query_points(nx, ny, n_pts, seed=5):
    """n_pts starts: the four corners, points on the edges, points outside (one NaN, one Inf), the rest uniform over the frame"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0.0, nx - 1.0, n_pts), rng.uniform(0.0, ny - 1.0, n_pts)], axis=-1)
    fixed = [(0.0, 0.0), (nx - 1.0, 0.0), (0.0, ny - 1.0), (nx - 1.0, ny - 1.0), (0.5, 0.0), (nx - 1.0, 0.75), (0.0, ny - 1.5),
             (-0.25, 0.5), (nx - 0.5, 1.0), (1.0, -1e-9), (0.5, ny - 1.0 + 1e-9), (np.nan, 1.0), (1.0, np.inf), (-np.inf, 0.0)]
    k = min(len(fixed), n_pts)
    p[:k] = fixed[:k]
    return p
