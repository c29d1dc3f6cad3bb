"""The algebra of the f64 tolerance mode's primal stage (csrc/ofx_tvl1.hip, tvl1_primal<double, false>), on the CPU.

The kernels no longer run the reference's three-way thresholding in that mode but its clamp form,

    fi = -rho / max(grad, 2^-600),   d = clamp(fi, -l_t, +l_t) (I1wx, I1wy),   and the factor 0 where grad < 1e-10 and the clamp idle,

which is the same function of (rho, grad) up to the rounding of fi at the two thresholds.  Here a numpy restatement of that form
(no FMA, exact 1 / x and sqrt) is held against the oracle's restatement of the mode, orc.tvl1_iterations_mode(relaxed = 1), at
the bars of tests/test_gpu_relaxed_modes.py -- on states that HAVE the pixels where the two could part:

* flat pixels, 0 < grad < 1e-10, on both sides of |rho| = l_t grad: the reference sets d = 0 inside and +-l_t I1w outside; a clamp
  form without the flat-pixel rule gives fi I1w inside, wrong by up to l_t |I1w| (patched_state alone has only grad == 0 exactly,
  where every form gives 0 -- the second test shows that the crafted states see the difference);
* ties, rho = +-l_t grad up to its rounding, on pixels with an ordinary gradient: the branches meet there.

`crafted_state` and `clamp_form_iterations` are shared with tests/test_gpu_tvl1_tolerance_algebra.py."""
import numpy as np
import pytest
from test_oracle_modes import patched_state

PAR = dict(tau=0.25, lam=0.15, theta=0.3)
GRAD_IS_ZERO = 1e-10                      # TVL1_GRAD_IS_ZERO

# the bars of tests/test_gpu_relaxed_modes.py (TOL64_REL, TOL64_ERR; that module is marked gpu as a whole, so they are copied):
# max |delta| / max(1, |x|) of the six state arrays, |delta error| / error.  Measured here: 6.7e-16 and 6.0e-15.
TOL64_REL, TOL64_ERR = 3e-13, 2e-12
# a restatement WITHOUT the flat-pixel rule must miss the first bar by orders: it is wrong by ~l_t |I1w| ~ 1e-7 on the flat pixels
FLAT_RULE_MIN_DEVIATION = 1e-9

SHAPES = [(5, 4), (64, 3), (3, 64), (61, 33), (113, 16), (130, 77)]
N_ITERS = [1, 2, 3, 4, 7]
NAMES = ("u1", "u2", "p11", "p12", "p21", "p22")


def crafted_state(orc, synth, nx, ny, seed=0):
    """patched_state with a first eighth of the pixels (at least two) made flat -- gradient components ~ N(0, 3e-6), so that
    0 < grad < 1e-10 -- and rho_c set so that rho = s l_t grad, s uniform in (-2, 2) (the first two: |s| = 0.5 and 1.5, one on
    each side of the threshold whatever the size); and a second eighth, of pixels with an ordinary gradient, set to the ties
    rho = +-l_t grad.  Returns patched_state's tuple and the flat indices of the two sets."""
    u1, u2, p, I1wx, I1wy, rho_c, _ = patched_state(orc, synth, nx, ny, seed)
    I1wx, I1wy, rho_c = I1wx.copy(), I1wy.copy(), rho_c.copy()
    l_t = PAR["lam"] * PAR["theta"]
    rng = np.random.default_rng(1000 + seed)
    n = nx * ny
    k = max(n // 8, 2)
    perm = rng.permutation(n)
    flat = perm[:k]
    gx, gy = rng.standard_normal(k) * 3e-6, rng.standard_normal(k) * 3e-6
    gx[gx == 0.0] = 3e-6
    while True:
        big = gx * gx + gy * gy >= 0.9 * GRAD_IS_ZERO
        if not big.any():
            break
        gx[big] *= 0.5
        gy[big] *= 0.5
    I1wx.ravel()[flat], I1wy.ravel()[flat] = gx, gy
    grad = I1wx * I1wx + I1wy * I1wy
    s = rng.uniform(-2.0, 2.0, k)
    s[0] = np.copysign(0.5, s[0])
    s[1] = np.copysign(1.5, s[1])
    lin = I1wx * u1 + I1wy * u2
    rho_c.ravel()[flat] = s * l_t * grad.ravel()[flat] - lin.ravel()[flat]
    rest = perm[k:]
    ties = rest[grad.ravel()[rest] >= GRAD_IS_ZERO][:k]
    sign = np.where(rng.integers(0, 2, ties.size) == 1, 1.0, -1.0)
    rho_c.ravel()[ties] = sign * l_t * grad.ravel()[ties] - lin.ravel()[ties]
    return (u1, u2, p, I1wx, I1wy, rho_c, grad), flat, ties


def clamp_form_iterations(orc, st, I1wx, I1wy, rho_c, tau, lam, theta, n_iter, flat_rule=True):
    """n_iter iterations of the f64 tolerance mode in its clamp form, on st = [u1, u2, p11, p12, p21, p22] in place; returns the
    last error.  Plain IEEE double operations in numpy; the stencils are the oracle's."""
    l_t, taut = lam * theta, tau / theta
    u1, u2, p11, p12, p21, p22 = st
    grad = I1wx * I1wx + I1wy * I1wy
    inv = 1.0 / np.maximum(grad, 2.0 ** -600)
    error = np.inf
    for _ in range(n_iter):
        rho = rho_c + (I1wx * u1 + I1wy * u2)
        fi = -rho * inv
        fic = np.minimum(np.maximum(fi, -l_t), l_t)
        if flat_rule:
            fic = np.where((grad < GRAD_IS_ZERO) & (fic == fi), 0.0, fic)
        n1 = (u1 + fic * I1wx) + theta * orc.divergence(p11, p12)
        n2 = (u2 + fic * I1wy) + theta * orc.divergence(p21, p22)
        error = float(np.sum((n1 - u1) * (n1 - u1) + (n2 - u2) * (n2 - u2))) / u1.size
        u1[...], u2[...] = n1, n2
        u1x, u1y = orc.forward_gradient(u1)
        u2x, u2y = orc.forward_gradient(u2)
        i1 = 1.0 / (1.0 + taut * np.sqrt(np.maximum(u1x * u1x + u1y * u1y, 2.0 ** -600)))
        i2 = 1.0 / (1.0 + taut * np.sqrt(np.maximum(u2x * u2x + u2y * u2y, 2.0 ** -600)))
        p11[...] = (p11 + taut * u1x) * i1
        p12[...] = (p12 + taut * u1y) * i1
        p21[...] = (p21 + taut * u2x) * i2
        p22[...] = (p22 + taut * u2y) * i2
    return error


def deviations(got, e_g, want, e_w):
    """(worst max |delta| / max(1, |x|) over the six state arrays, |delta error| / error): the two figures the bars are on"""
    rel = max(float(np.abs(g - w).max()) / max(1.0, float(np.abs(w).max())) for g, w in zip(got, want))
    return rel, abs(e_g - e_w) / max(e_w, 1e-300)


_cache = {}


def crafted(orc, synth, nx, ny):
    if (nx, ny) not in _cache:
        _cache[nx, ny] = crafted_state(orc, synth, nx, ny)
    return _cache[nx, ny]


def oracle_reference(orc, synth, nx, ny, n_iter, _refs={}):
    """the oracle's tolerance-mode restatement on the crafted state: computed once per (shape, n_iter), never modified"""
    if (nx, ny, n_iter) not in _refs:
        (u1, u2, p, I1wx, I1wy, rho_c, grad), _, _ = crafted(orc, synth, nx, ny)
        st = [x.copy() for x in (u1, u2, *p)]
        e = orc.tvl1_iterations_mode(*st, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], n_iter, 1, 0)
        _refs[nx, ny, n_iter] = (st, e)
    return _refs[nx, ny, n_iter]


def _restated(orc, synth, nx, ny, n_iter, flat_rule):
    (u1, u2, p, I1wx, I1wy, rho_c, _), _, _ = crafted(orc, synth, nx, ny)
    st = [x.copy() for x in (u1, u2, *p)]
    e = clamp_form_iterations(orc, st, I1wx, I1wy, rho_c, PAR["tau"], PAR["lam"], PAR["theta"], n_iter, flat_rule)
    return st, e


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_crafted_states_hold_their_hard_pixels(orc, synth, nx, ny):
    (u1, u2, _, I1wx, I1wy, rho_c, grad), flat, ties = crafted(orc, synth, nx, ny)
    l_t = PAR["lam"] * PAR["theta"]
    rho = (rho_c + (I1wx * u1 + I1wy * u2)).ravel()
    g = grad.ravel()
    assert np.array_equal(g, (I1wx * I1wx + I1wy * I1wy).ravel())
    assert ((g[flat] > 0.0) & (g[flat] < GRAD_IS_ZERO)).all()
    inside = np.abs(rho[flat]) < l_t * g[flat]
    outside = np.abs(rho[flat]) > l_t * g[flat]
    assert inside.any() and outside.any(), (int(inside.sum()), int(outside.sum()))
    # s is met to the rounding of rho (~1e-9 of it: rho_c cancels against I1w . u), far from the threshold on both sides
    assert (np.abs(rho[flat][:2]) / (l_t * g[flat][:2])).round(6).tolist() == [0.5, 1.5]
    assert ties.size >= 1 and (g[ties] >= GRAD_IS_ZERO).all()
    assert np.allclose(np.abs(rho[ties]), l_t * g[ties], rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("n_iter", N_ITERS)
def test_clamp_form_is_the_tolerance_mode(orc, synth, nx, ny, n_iter):
    want, e_w = oracle_reference(orc, synth, nx, ny, n_iter)
    got, e_g = _restated(orc, synth, nx, ny, n_iter, True)
    assert all(np.isfinite(g).all() for g in got)
    rel, err = deviations(got, e_g, want, e_w)
    print("clamp form vs oracle %dx%d n_iter %d: state %.3g error %.3g" % (nx, ny, n_iter, rel, err))
    assert rel <= TOL64_REL, (nx, ny, n_iter, rel)
    assert err <= TOL64_ERR, (nx, ny, n_iter, e_g, e_w)


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("n_iter", N_ITERS)
def test_without_the_flat_pixel_rule_the_crafted_states_tell(orc, synth, nx, ny, n_iter):
    """the same restatement with the rule left out must MISS the bar, by orders: the crafted states are sensitive to it"""
    want, e_w = oracle_reference(orc, synth, nx, ny, n_iter)
    got, e_g = _restated(orc, synth, nx, ny, n_iter, False)
    rel, _ = deviations(got, e_g, want, e_w)
    print("no flat-pixel rule vs oracle %dx%d n_iter %d: state %.3g" % (nx, ny, n_iter, rel))
    assert rel > FLAT_RULE_MIN_DEVIATION, (nx, ny, n_iter, rel)
