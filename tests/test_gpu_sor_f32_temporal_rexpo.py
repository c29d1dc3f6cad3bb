"""Temporal Brox and one-channel robust_expo in float storage (OFX_F32) against a restatement of float storage outside the library.

tests/test_gpu_sor_f32.py pins Horn-Schunck and spatial Brox this way; the two families here were guarded only by gpu32-against-gpu32
comparisons (schedule invariance, device entry against host entry, group against lone solve) and one AEPE bar against the double
reference -- none of which sees a rounding that every schedule shares, or a wrong load in the float instantiation.  The anchors:

 * temporal Brox: tests/broxt_colour_ref.c with store_f32 = 1 (its header lists what is rounded; checked on the CPU in
   tests/test_broxt_colour_ref.py), order 0 for the exact mode (k_broxt_window, k_broxt_window_group) and order 1 for the tolerance
   mode (k_broxt_rb, k_broxt_tile<float, K> for every K);
 * robust_expo, methods 1 to 3: orc_robust_expo_mode / orc_rexpo_single_scale_mode with store_f32 = 1 (oracle/ofx_oracle.h lists what
   is rounded; checked on the CPU in tests/test_oracle_sor_f32.py).  The restatement follows ofx_robust_expo, which rounds a
   one-channel image before the normalisation; robust_expo_pyramid and the group entry round after it and are compared on
   float-representable images.

The bar is the one of test_gpu_sor_f32.py and holds by construction: sweep tables equal, 100 % of the elements bit-identical, 0
float ulps (F32_SAME, F32_ULPS there; check_restatement asserts it).  Both sides compute correctly rounded double arithmetic without
contraction and round to float at the same places.  Every case also asserts that the solve did work -- a non-zero flow and a sweep
table with a sum > 0 -- so that a solve that trivially stays zero cannot hide a difference.

OFX_MEASURE_OUT=<file> records cases, worst ulps and the share of equal elements per family
(profiles/r18_sor_f32_temporal_rexpo.json)."""
import importlib.util
import math
import os

import numpy as np
import pytest

from test_gpu_sor_f32 import MEASURED, Solve, _record, check_restatement, options, run, start_flow  # noqa: F401 (_record: the fixture)
from test_gpu_sor_f32 import REXPO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CK = _load("broxt_colour_ref", os.path.join(HERE, "broxt_colour_ref.py"))
_cache = {}


def _expected(oracle_mod, I, tag, order, kw):
    """the float-storage checker, computed once per case (tag names the input)"""
    key = (tag, order, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = CK.brox_temporal(oracle_mod, I, order, store_f32=1, **kw)
    return _cache[key]


def did_work(got, where):
    u, v, it = (got.u, got.v, got.it) if isinstance(got, Solve) else got
    assert np.asarray(it).sum() > 0, (where, "no sweep ran")
    assert np.asarray(u).any() and np.asarray(v).any(), (where, "zero flow")


# ---- temporal Brox -------------------------------------------------------------------------------------------------------------------
BT = dict(alpha=18.0, gamma=7.0, nu=0.75, TOL=1e-4, inner=1, outer=4)
# (nx, ny, frames, nscales, changes to BT, options of the exact mode)
BT_SHAPES = [
    (6, 6, 3, 1, dict(), dict()),                                   # nz = 2: both temporal taps one-sided, no field is interior
    (7, 6, 4, 1, dict(), dict()),                                   # nz = 3, odd width
    (33, 47, 4, 2, dict(inner=2, outer=3), dict()),                 # inner = 2: psid / psig recomputed from a non-zero rounded du
    (40, 33, 5, 1, dict(), dict(sor_window=5, sor_rows=3)),         # a window schedule away from the default
    (135, 68, 5, 2, dict(outer=3), dict()),                         # several row blocks and tiles, sizes off their pitch
    (24, 20, 10, 1, dict(outer=3), dict()),                         # nz = 9
]


@pytest.mark.parametrize("nx,ny,frames,ns,ch,opts", BT_SHAPES)
def test_brox_temporal_exact_equals_the_restatement(gpu32, oracle_mod, orc, synth, nx, ny, frames, ns, ch, opts):
    """order 0: k_broxt_psis, k_broxt_div and broxt_point in k_broxt_window"""
    I = synth.sequence(nx, ny, frames)
    kw = dict(BT, nscales=ns, **ch)
    want = _expected(oracle_mod, I, (nx, ny, frames), 0, kw)
    got = run(gpu32, gpu32.brox_temporal, I, opts=opts, **kw)
    did_work(got, (nx, ny, frames))
    check_restatement("broxt_exact", got, want, (nx, ny, frames, ns, opts))


@pytest.mark.parametrize("nx,ny,frames,ns,ch", [s[:5] for s in BT_SHAPES] + [(130, 9, 3, 1, dict())])     # fewer rows than a tile's halo
def test_brox_temporal_tolerance_equals_the_restatement(gpu32, oracle_mod, orc, synth, nx, ny, frames, ns, ch):
    """order 1: k_broxt_tile<float, K> for K = 1, 2, 4 (0: the library's choice) and k_broxt_rb<float> (sor_fuse = 9), each
    against the restatement directly"""
    I = synth.sequence(nx, ny, frames)
    kw = dict(BT, nscales=ns, **ch)
    want = _expected(oracle_mod, I, (nx, ny, frames), 1, kw)
    did_work(want, (nx, ny, frames))
    for K in (0, 1, 2, 4, 9):
        got = run(gpu32, gpu32.brox_temporal, I, opts=dict(sor_exact=0, sor_fuse=K), **kw)
        did_work(got, (nx, ny, frames, K))
        check_restatement("broxt_tolerance", got, want, (nx, ny, frames, ns, K))


def test_brox_temporal_tolerance_loop_ends(gpu32, oracle_mod, orc, synth):
    """K = 4: a stop before the first sweep (TOL = 2000: no sweep, a zero flow -- the one series where that is right), inside a launch
    unit, and at the iteration limit"""
    I = synth.sequence(150, 97, 4)
    seen = set()
    for TOL in (2000.0, 1e-2, 3e-4, 0.0):
        kw = dict(BT, nscales=1, outer=2, TOL=TOL)
        want = _expected(oracle_mod, I, (150, 97, 4), 1, kw)
        got = run(gpu32, gpu32.brox_temporal, I, opts=dict(sor_exact=0, sor_fuse=4), **kw)
        print("TOL", TOL, "sweeps", got.it.ravel(), "restatement", want[2].ravel())
        if TOL < 2000.0:
            did_work(got, TOL)
        check_restatement("broxt_tolerance", got, want, ("loop ends", TOL))
        seen.update(int(n) for n in want[2].ravel())
    assert 0 in seen and 300 in seen and any(0 < n < 300 and n % 4 for n in seen), seen


def _device_frames(I):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(I, dtype=np.float32)).cuda()       # the upload rounds frames + 0.3
    torch.cuda.synchronize()
    return t


def _payloads(n_flo, ny, nx):
    import torch
    flo = torch.zeros((n_flo, ny, nx, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return flo


def _ptrs(t):
    return [t[k].data_ptr() for k in range(t.shape[0])]


@pytest.mark.parametrize("mode", ["exact", "tolerance"])
def test_brox_temporal_dev_equals_the_restatement(gpu32, oracle_mod, orc, synth, mode):
    """the device entry on float frames: integer frames, and frames + 0.3, which only the conversion to float makes representable"""
    nx, ny, frames = 40, 33, 4
    kw = dict(BT, nscales=2, outer=3)
    for shift in (0.0, 0.3):
        I = synth.sequence(nx, ny, frames) + shift
        want = _expected(oracle_mod, I, (nx, ny, frames, shift), 0 if mode == "exact" else 1, kw)
        t, flo = _device_frames(I), _payloads(frames - 1, ny, nx)
        with options(gpu32, sor_exact=1 if mode == "exact" else 0):
            gpu32.brox_temporal_dev(_ptrs(t), _ptrs(flo), nx, ny, **kw)
            gpu32.synchronize()
            it = gpu32.stats().iterations().copy()
        out = flo.cpu().numpy().astype(np.float64)
        got = (out[..., 0], out[..., 1], it)
        did_work(got, (mode, shift))
        check_restatement("broxt_dev", got, want, (mode, shift))


@pytest.mark.parametrize("mode", ["exact", "tolerance"])
def test_brox_temporal_group_equals_the_restatement(gpu32, oracle_mod, orc, synth, mode):
    """a lockstep group of 3 sequences (k_broxt_prepare_group, k_broxt_coeff_group, k_broxt_window_group / the tile kernels' group
    path): every sequence against the restatement of that sequence"""
    import torch
    nx, ny, frames, G = 40, 33, 4, 3
    kw = dict(BT, nscales=2, outer=3)
    seqs = [synth.sequence(nx, ny, frames, k) + (0.3 if k == 1 else 0.0) for k in range(G)]
    ts, flo = [_device_frames(I) for I in seqs], _payloads(G * (frames - 1), ny, nx)
    with options(gpu32, sor_exact=1 if mode == "exact" else 0):
        st = gpu32.brox_temporal_group_dev([p for t in ts for p in _ptrs(t)], _ptrs(flo), nx, ny, frames, **kw)
        gpu32.synchronize()
    torch.cuda.synchronize()
    out = flo.cpu().numpy().astype(np.float64).reshape(G, frames - 1, ny, nx, 2)
    for g in range(G):
        want = _expected(oracle_mod, seqs[g], (nx, ny, frames, "group", g), 0 if mode == "exact" else 1, kw)
        got = (out[g, ..., 0], out[g, ..., 1], st[g].iterations().copy())
        did_work(got, (mode, g))
        check_restatement("broxt_group", got, want, (mode, g))


# ---- robust_expo, one channel -------------------------------------------------------------------------------------------------------
RX_SHAPES = [(9, 8, 1), (33, 47, 1), (64, 48, 2), (80, 60, 3), (257, 75, 1)]


def quantile_walk(orc, I1, I2, alpha):
    """method 3 at level 0 of ofx_robust_expo in float storage: (first position, final position, pixels) of the quantile loop of
    robust_expo_exponential_calculation -- it advances while (-log 0.05 + log alpha) / 2 exceeds the sorted gradient magnitude"""
    f = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    a, b = f(I1), f(I2)
    mn, mx = min(a.min(), b.min()), max(a.max(), b.max())
    A = f(255.0 * (a - mn) / (mx - mn))
    # the restated Dirichlet Gaussian rounds each pass; one rounding at the end differs from it by an ulp of the image at most, far
    # below the distance of any magnitude here from the threshold -- this only LABELS the cases, the comparison does not use it
    A = f(orc.gaussian_dirichlet(A, 1.0))
    gx, gy = orc.centered_gradient(A)
    mg = np.sort(np.hypot(f(gx), f(gy)).ravel())
    n, c = mg.size, -math.log(0.05) + math.log(float(int(alpha)))
    first = pos = int(0.94 * n)
    while pos < n and c / 2 > mg[pos - 1]:
        pos += 1
    return first, pos, n


def flat_pair(synth, nx, ny):
    """the P1 pair at 4 % contrast with one bright block: after the normalisation stretches the block to 255, more than 94 % of the
    gradient magnitudes lie under method 3's threshold and its quantile loop has to walk up to the block's edge (from 64x48 on: on
    smaller images the block's edge alone is more than 6 % of the pixels)"""
    I1, I2 = synth.pair("P1", nx, ny)
    m = 0.5 * (I1.mean() + I2.mean())
    out = []
    for I in (I1, I2):
        J = m + 0.04 * (I - m)
        J[3:7, 3:9] += 150.0
        out.append(J.astype(np.float32).astype(np.float64))
    return out


@pytest.mark.parametrize("nx,ny,ns", RX_SHAPES)
@pytest.mark.parametrize("method", [1, 2, 3])
def test_robust_expo_equals_the_restatement(gpu32, orc, synth, method, nx, ny, ns):
    """gpu32.robust_expo on the pyramid; at one scale also the level solve (robust_expo_single_scale) from a non-zero flow, on
    images that only the upload makes float-representable.  Method 3 on these images: the quantile loop does NOT advance (asserted);
    test_robust_expo_method_3_with_a_moving_quantile has the other case."""
    I1, I2 = synth.pair("P1", nx, ny)
    kw = dict(REXPO[method], nscales=ns)
    if method == 3:
        first, pos, n = quantile_walk(orc, I1, I2, kw["alpha"])
        assert pos == first < n, (first, pos, n)
    got = run(gpu32, gpu32.robust_expo, I1, I2, **kw)
    did_work(got, (method, nx, ny, ns))
    check_restatement("rexpo", got, orc.robust_expo_mode(I1, I2, store_f32=1, **kw), (method, nx, ny, ns))
    if ns == 1:
        u0, v0 = start_flow(nx, ny)
        sk = dict(REXPO[method])
        a, b = I1 + 0.3, I2 * 1.01                          # no floats: the upload rounds
        got = run(gpu32, gpu32.robust_expo_single_scale, a, b, u0, v0, **sk)
        did_work(got, (method, nx, ny, "single scale"))
        check_restatement("rexpo_single_scale", got, orc.rexpo_single_scale_mode(a, b, u0, v0, store_f32=1, **sk),
                          (method, nx, ny, "single scale"))


@pytest.mark.parametrize("nx,ny", [(64, 48), (80, 60)])
def test_robust_expo_method_3_with_a_moving_quantile(gpu32, orc, synth, nx, ny):
    """method 3 where the quantile loop DOES advance (asserted: it moves, and stops before the last pixel, so lambda_omega > 0 comes
    from a magnitude further up the sorted list)"""
    I1, I2 = flat_pair(synth, nx, ny)
    kw = dict(REXPO[3], nscales=1)
    first, pos, n = quantile_walk(orc, I1, I2, kw["alpha"])
    print("quantile loop: from %d to %d of %d" % (first, pos, n))
    assert first < pos < n, (first, pos, n)
    got = run(gpu32, gpu32.robust_expo, I1, I2, **kw)
    did_work(got, (nx, ny))
    check_restatement("rexpo", got, orc.robust_expo_mode(I1, I2, store_f32=1, **kw), (3, nx, ny, "moving quantile"))


@pytest.mark.parametrize("method", [1, 2, 3])
def test_robust_expo_pyramid_equals_the_restatement(gpu32, orc, synth, method):
    """ofx_robust_expo_pyramid rounds after the normalisation: on float-representable images the same solve"""
    I1, I2 = synth.pair("P1", 80, 60)
    assert np.array_equal(I1, I1.astype(np.float32)) and np.array_equal(I2, I2.astype(np.float32))
    kw = dict(REXPO[method], nscales=3)
    got = run(gpu32, gpu32.robust_expo_pyramid, I1, I2, **kw)
    did_work(got, method)
    check_restatement("rexpo_pyramid", got, orc.robust_expo_mode(I1, I2, store_f32=1, **kw), (method, "pyramid"))


@pytest.mark.parametrize("method", [1, 2, 3])
def test_robust_expo_group_equals_the_restatement(gpu32, orc, synth, method):
    """a lockstep group of 3 pairs of float images (nz = 1): every pair against the restatement of that pair"""
    import torch
    nx, ny, G = 64, 48, 3
    kw = dict(REXPO[method], nscales=2)
    pairs = [synth.pair("P0" if k == 2 else "P1", nx, ny, k) for k in range(G)]
    d1 = [torch.from_numpy(p[0]).to(torch.float32).cuda() for p in pairs]
    d2 = [torch.from_numpy(p[1]).to(torch.float32).cuda() for p in pairs]
    flo = _payloads(G, ny, nx)
    st = gpu32.robust_expo_group_dev([t.data_ptr() for t in d1], [t.data_ptr() for t in d2], _ptrs(flo), nx, ny, 1, **kw)
    gpu32.synchronize()
    out = flo.cpu().numpy().astype(np.float64)
    for g, (I1, I2) in enumerate(pairs):
        assert np.array_equal(I1, I1.astype(np.float32)) and np.array_equal(I2, I2.astype(np.float32))
        got = (out[g, ..., 0], out[g, ..., 1], st[g].iterations().copy())
        did_work(got, (method, g))
        check_restatement("rexpo_group", got, orc.robust_expo_mode(I1, I2, store_f32=1, **kw), (method, "group", g))
