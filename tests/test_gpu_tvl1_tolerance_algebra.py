"""The f64 tolerance mode's arithmetic -- the clamp-form primal stage and the FMAs of tvl1_primal / tvl1_dual<double, false>
(csrc/ofx_tvl1.hip) -- on the crafted states of tests/test_tvl1_clamp_form.py: flat pixels (0 < grad < 1e-10) on both sides of
|rho| = l_t grad, where a clamp form that forgot the flat-pixel rule is wrong by ~1e-7, and ties rho = +-l_t grad.

* every iteration kernel in tolerance mode against the oracle's restatement (relaxed = 1) at the bars of
  tests/test_gpu_relaxed_modes.py, and bit-identical to the two-iteration kernel: all kernels call the same two functions;
  k_tvl1_iter4 also at strip heights 4 and 13, so that the fill, the steady state and the drain of its three-phase march run;
* the strict mode on the same states is the reference bit for bit: none of the new arithmetic leaks into it;
* one whole lockstep-group solve, tolerance against strict: iteration tables equal, AEPE < 1e-8."""
import contextlib

import numpy as np
import pytest
from test_tvl1_clamp_form import NAMES, PAR, TOL64_ERR, TOL64_REL, crafted, deviations, oracle_reference

pytestmark = pytest.mark.gpu

# the library's defaults of every option this file touches (ofx_ctx.cpp)
DEFAULTS = dict(relaxed_dual=0, fuse2=1, fuse3=2, fuse3_min_px=0, fuse4=2, fuse4_min_px=0, tile=0, tile_max_px=0, rows_per_wave3=0)

KERNELS = {
    "iter1": dict(fuse2=0),
    "iter2": dict(fuse3=0),
    "iter3": dict(fuse3=1, fuse3_min_px=0),
    "iter4": dict(fuse4=1, fuse4_min_px=0),
    "iter4_rows4": dict(fuse4=1, fuse4_min_px=0, rows_per_wave3=4),
    "iter4_rows13": dict(fuse4=1, fuse4_min_px=0, rows_per_wave3=13),
    "tile4": dict(tile=4, tile_max_px=1e9),
}
BASE = "iter2"
SHAPES = [(5, 4), (64, 3), (3, 64), (61, 33), (113, 16), (64, 41)]
N_ITERS = [1, 2, 3, 4, 7]


@contextlib.contextmanager
def options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, DEFAULTS[k])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


_base = {}


def _run(gpu, orc, synth, nx, ny, n_iter, **opts):
    (u1, u2, p, I1wx, I1wy, rho_c, _), _, _ = crafted(orc, synth, nx, ny)
    st = [x.copy() for x in (u1, u2, *p)]
    with options(gpu, **opts):
        e = gpu.tvl1_iterations(*st, I1wx, I1wy, rho_c, PAR["tau"], PAR["lam"], PAR["theta"], n_iter)
        assert gpu.stats().iterations()[0][0] == n_iter
    return st, e


def _baseline(gpu, orc, synth, nx, ny, n_iter):
    if (nx, ny, n_iter) not in _base:
        _base[nx, ny, n_iter] = _run(gpu, orc, synth, nx, ny, n_iter, relaxed_dual=1, **KERNELS[BASE])
    return _base[nx, ny, n_iter]


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_tolerance_kernels_on_the_crafted_states(gpu64, orc, synth, kernel):
    worst_rel = worst_err = 0.0
    for nx, ny in SHAPES:
        for n_iter in N_ITERS:
            where = (kernel, nx, ny, n_iter)
            want, e_w = oracle_reference(orc, synth, nx, ny, n_iter)
            base, e_b = _baseline(gpu64, orc, synth, nx, ny, n_iter)
            got, e_g = _run(gpu64, orc, synth, nx, ny, n_iter, relaxed_dual=1, **KERNELS[kernel])
            for name, g in zip(NAMES, got):
                assert np.isfinite(g).all(), (where, name)
            rel, err = deviations(got, e_g, want, e_w)
            worst_rel, worst_err = max(worst_rel, rel), max(worst_err, err)
            assert rel <= TOL64_REL, (where, rel)
            assert err <= TOL64_ERR, (where, e_g, e_w)
            for name, g, b in zip(NAMES, got, base):
                assert same_bits(g, b), (where, name, "differs from " + BASE)
            # the error differs from the base kernel's by the order of its sum only
            assert abs(e_g - e_b) <= 1e-12 * max(e_b, 1e-300), (where, e_g, e_b)
    print("%s vs the restatement, worst: state %.3g error %.3g" % (kernel, worst_rel, worst_err))


@pytest.mark.parametrize("kernel", ["iter2", "iter3", "iter4"])
def test_strict_mode_on_the_crafted_states_is_the_reference(gpu64, orc, synth, kernel):
    for nx, ny in SHAPES:
        (u1, u2, p, I1wx, I1wy, rho_c, grad), _, _ = crafted(orc, synth, nx, ny)
        for n_iter in N_ITERS:
            want = [x.copy() for x in (u1, u2, *p)]
            orc.tvl1_iterations(*want, I1wx, I1wy, rho_c, grad, PAR["tau"], PAR["lam"], PAR["theta"], n_iter)
            got, _ = _run(gpu64, orc, synth, nx, ny, n_iter, **KERNELS[kernel])
            for name, g, w in zip(NAMES, got, want):
                assert same_bits(g, w), (kernel, nx, ny, n_iter, name)


def test_group_solve_tolerance_against_strict(gpu64, synth):
    """three pairs at 160 x 120 in lockstep, 3 scales, default parameters: equal iteration tables, AEPE < 1e-8"""
    import torch
    nx, ny, G = 160, 120, 3
    pairs = [synth.pair("P0" if k % 3 == 2 else "P1", nx, ny, k) for k in range(G)]
    d0 = [torch.from_numpy(p[0]).to(torch.float64).cuda() for p in pairs]
    d1 = [torch.from_numpy(p[1]).to(torch.float64).cuda() for p in pairs]
    torch.cuda.synchronize()
    res = {}
    for relaxed in (0, 1):
        flo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with options(gpu64, relaxed_dual=relaxed):
            st = gpu64.tvl1_group_dev([t.data_ptr() for t in d0], [t.data_ptr() for t in d1], [flo[k].data_ptr() for k in range(G)],
                                      nx, ny, nscales=3)
            gpu64.synchronize()
        res[relaxed] = (flo.cpu().numpy().astype(np.float64), [s.iterations().copy() for s in st])
    (f_s, t_s), (f_t, t_t) = res[0], res[1]
    assert np.isfinite(f_t).all() and float(np.abs(f_t).max()) > 0.0
    for k in range(G):
        assert np.array_equal(t_t[k], t_s[k]), (k, t_t[k], t_s[k])
        aepe = float(np.mean(np.hypot(f_t[k, ..., 0] - f_s[k, ..., 0], f_t[k, ..., 1] - f_s[k, ..., 1])))
        print("pair %d: AEPE tolerance vs strict %.3g" % (k, aepe))
        assert aepe < 1e-8, (k, aepe)
