"""The marching phases of k_tvl1_iter4 (fill, steady state written out three steps at a time, drain) and the one loop of k_tvl1_iter3.

A full unit of k_tvl1_iter4 runs guarded steps until its last stage has a row, then whole bodies of three unguarded steps, then
guarded steps again; the step counts of the three phases follow from the strip height, the band's place in the image and the
image height.  tests/test_gpu_tvl1_iter4.py stops at strips of 8 rows and images of 30, where the steady state is 0 - 5 steps
long.  Here the strip height takes every value 1 .. 13, 16 and 32 on images of 41 and 64 rows: top bands, interior bands, partial
and full bottom bands, steady lengths in every residue modulo 3, zero and negative ones included (an interior band of r rows has
r - 4 steady steps, a full bottom band r - 8).  Both kernels are forced in turn and compared with the one-iteration kernel
(fuse2 = 0): u1, u2, p11, p12, p21, p22 bit for bit, the error to 1e-12 relative (a sum over waves, added up in another order),
in the strict f64, the f64 tolerance and the f32 storage modes."""
import contextlib

import numpy as np
import pytest
import torch
from test_oracle_modes import patched_state

pytestmark = pytest.mark.gpu

PAR = dict(tau=0.25, lam=0.15, theta=0.3)
DEFAULTS = dict(relaxed_dual=0, fuse2=1, fuse3=2, fuse3_min_px=0, fuse4=2, fuse4_min_px=0, rows_per_wave3=0, nt_stores=0)
MODES = ["strict64", "tol64", "f32"]
ITER1 = dict(fuse2=0, fuse4=0)
KERNELS = {"iter4": dict(fuse4=1, fuse4_min_px=0), "iter3": dict(fuse4=0, fuse3=1, fuse3_min_px=0)}
ROWS = list(range(1, 14)) + [16, 32]
SHAPES = [(nx, ny) for nx in (57, 130) for ny in (41, 64)]    # one partial strip of 56 columns, and three
COUNTS = [3, 4, 5, 8]                                         # a full unit of each kernel, full units plus a tail, two full units
NT_SHAPE = (130, 41)                                          # non-temporal stores as well on this one

_states, _want = {}, {}


@contextlib.contextmanager
def options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, DEFAULTS[k])


def _gpu(mode, gpu64, gpu32):
    return gpu32 if mode == "f32" else gpu64


def _mode_opts(mode):
    return dict(relaxed_dual=1) if mode == "tol64" else {}


def _iterations(gpu, orc, synth, nx, ny, n_iter, **opts):
    if (nx, ny) not in _states:
        _states[nx, ny] = patched_state(orc, synth, nx, ny)
    u1, u2, p, I1wx, I1wy, rho_c, _ = _states[nx, ny]
    st = [x.copy() for x in (u1, u2, *p)]
    with options(gpu, **opts):
        e = gpu.tvl1_iterations(*st, I1wx, I1wy, rho_c, PAR["tau"], PAR["lam"], PAR["theta"], n_iter)
        assert gpu.stats().iterations()[0][0] == n_iter
    return st, e


def _baseline(gpu, orc, synth, mode, nx, ny, n_iter):
    key = (mode, nx, ny, n_iter)
    if key not in _want:
        _want[key] = _iterations(gpu, orc, synth, nx, ny, n_iter, **_mode_opts(mode), **ITER1)
    return _want[key]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("mode", MODES)
def test_every_strip_height_equals_the_one_iteration_kernel(gpu64, gpu32, orc, synth, mode, kernel):
    gpu = _gpu(mode, gpu64, gpu32)
    for nx, ny in SHAPES:
        for n_iter in COUNTS:
            want, e_w = _baseline(gpu, orc, synth, mode, nx, ny, n_iter)
            for rows in ROWS:
                for nt in ((0, 1) if (nx, ny) == NT_SHAPE else (0,)):
                    got, e_g = _iterations(gpu, orc, synth, nx, ny, n_iter, **_mode_opts(mode), **KERNELS[kernel],
                                           rows_per_wave3=rows, nt_stores=nt)
                    for name, g, w in zip(("u1", "u2", "p11", "p12", "p21", "p22"), got, want):
                        assert np.isfinite(g).all(), (nx, ny, n_iter, rows, nt, name)
                        assert np.array_equal(g, w), (nx, ny, n_iter, rows, nt, name)
                    assert abs(e_g - e_w) <= 1e-12 * max(e_w, 1e-300), (nx, ny, n_iter, rows, nt, e_g, e_w)


@pytest.mark.parametrize("rows", [5, 12])
@pytest.mark.parametrize("mode", MODES)
def test_group_solve_equals_the_pairs_alone(gpu64, gpu32, synth, mode, rows):
    """130 x 70, three pairs in lockstep, three scales: the payloads and the iteration tables of the pairs solved alone with the
    one-iteration kernel"""
    gpu = _gpu(mode, gpu64, gpu32)
    nx, ny, G = 130, 70, 3
    kw = dict(nscales=3, **PAR)
    dt = torch.float32 if mode == "f32" else torch.float64
    pairs = [synth.pair("P0" if k % 3 == 2 else "P1", nx, ny, k) for k in range(G)]
    d0 = [torch.from_numpy(p[0]).to(dt).cuda() for p in pairs]
    d1 = [torch.from_numpy(p[1]).to(dt).cuda() for p in pairs]
    solo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tables = []
    with options(gpu, **_mode_opts(mode), **ITER1):
        for k in range(G):
            gpu.tvl1_multiscale_dev(d0[k].data_ptr(), d1[k].data_ptr(), solo[k].data_ptr(), nx, ny, **kw)
            gpu.synchronize()
            tables.append(gpu.stats().iterations().copy())
    for kernel, opts in KERNELS.items():
        flo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device="cuda")
        with options(gpu, **_mode_opts(mode), **opts, rows_per_wave3=rows):
            st = gpu.tvl1_group_dev([t.data_ptr() for t in d0], [t.data_ptr() for t in d1], [flo[k].data_ptr() for k in range(G)],
                                    nx, ny, **kw)
            gpu.synchronize()
        for k in range(G):
            assert np.array_equal(st[k].iterations(), tables[k]), (kernel, k)
            if kernel == "iter4":
                assert all(f == 4 for f in st[k].fused[:3]), list(st[k].fused[:3])
        assert torch.equal(flo.view(torch.int32), solo.view(torch.int32)), kernel
