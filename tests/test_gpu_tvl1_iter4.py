"""k_tvl1_iter4: four TV-L1 iterations per launch, the (I1wx, I1wy) / rho_c delay lines of the pipeline in a wave-private LDS ring.

The kernel is forced (fuse4 = 1, fuse4_min_px = 0) and compared with the one-iteration kernel (fuse2 = 0) bit for bit -- the same
per-pixel functions in the same order -- on U, P1, P2 and the iteration tables, in the strict f64, the f64 tolerance and the f32
storage modes: widths around the 56-column strips, heights around the halo depth and the strip boundaries, every length of a
launch unit and of a tail (fixed counts 1..9), loops that end on every position inside a unit, pairs of a lockstep group that
end at different iterations, an iteration limit that is no multiple of four."""
import contextlib

import numpy as np
import pytest
from test_oracle_modes import patched_state

pytestmark = pytest.mark.gpu

PAR = dict(tau=0.25, lam=0.15, theta=0.3)
DEFAULTS = dict(relaxed_dual=0, fuse2=1, fuse3=2, fuse3_cursor=1, fuse3_afac1=0, fuse3_afac2=0, fuse4=2, fuse4_min_px=0,
                fuse4_afac3=0, rows_per_wave3=0, nt_stores=0)
ITER1 = dict(fuse2=0, fuse4=0)
ITER4 = dict(fuse4=1, fuse4_min_px=0)
MODES = ["strict64", "tol64", "f32"]

WIDTHS = [2, 5, 55, 56, 57, 60, 64, 112, 113, 130]            # one, two and three strips of 56 columns
HEIGHTS = [2, 3, 4, 5, 7, 8, 9]                               # the halo depth (3 rows); rows - 1, rows, rows + 1 for rows = 4 and 8
SHAPES = [(nx, 9) for nx in WIDTHS] + [(57, ny) for ny in HEIGHTS if ny != 9] + [(57, 30), (130, 30)]   # 30 rows: 8 / 4 bands


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


_states, _base = {}, {}


def _iterations(gpu, orc, synth, nx, ny, n_iter, **opts):
    if (nx, ny) not in _states:
        _states[nx, ny] = patched_state(orc, synth, nx, ny)
    u1, u2, p, I1wx, I1wy, rho_c, _ = _states[nx, ny]
    st = [x.copy() for x in (u1, u2, *p)]
    with options(gpu, **opts):
        e = gpu.tvl1_iterations(*st, I1wx, I1wy, rho_c, PAR["tau"], PAR["lam"], PAR["theta"], n_iter)
        assert gpu.stats().iterations()[0][0] == n_iter
    return st, e


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("mode", MODES)
def test_fixed_counts_equal_the_one_iteration_kernel(gpu64, gpu32, orc, synth, mode, rows):
    """units 4, 4 + 1 .. 4 + 4 + 1 and the tails of 1, 2 and 3 (counts that are no multiple of four) on every shape"""
    gpu = _gpu(mode, gpu64, gpu32)
    for nx, ny in SHAPES:
        for n_iter in range(1, 10):
            key = (mode, nx, ny, n_iter)
            if key not in _base:
                _base[key] = _iterations(gpu, orc, synth, nx, ny, n_iter, **_mode_opts(mode), **ITER1)
            want, e_w = _base[key]
            for nt in ((0, 1) if (nx, ny) == (130, 30) else (0,)):
                got, e_g = _iterations(gpu, orc, synth, nx, ny, n_iter, **_mode_opts(mode), **ITER4, rows_per_wave3=rows, nt_stores=nt)
                for name, g, w in zip(("u1", "u2", "p11", "p12", "p21", "p22"), got, want):
                    assert np.isfinite(g).all(), (nx, ny, n_iter, name)
                    assert np.array_equal(g, w), (nx, ny, n_iter, nt, name)
                # the error is a sum over waves: the strips of the two kernels add it up in another order
                assert abs(e_g - e_w) <= 1e-12 * max(e_w, 1e-300), (nx, ny, n_iter, e_g, e_w)


def test_options_are_validated_before_they_are_stored(gpu64):
    for name in ("fuse3_afac1", "fuse3_afac2", "fuse4_afac3", "fuse4_min_px"):
        with pytest.raises(Exception):
            gpu64.set_option(name, -1.0)
    with pytest.raises(Exception):
        gpu64.set_option("fuse4", 3)


def test_kernel_is_reported(gpu64, synth):
    """the work record names the kernel that ran: forced, switched off, and left to the library on a lone small pair"""
    I0, I1 = synth.pair("P1", 57, 9)
    z = np.zeros((9, 57))
    for opts, unit in ((ITER4, 4), (dict(fuse4=0, fuse3=1), 3), (dict(), 2)):
        with options(gpu64, **opts):
            gpu64.tvl1_single_scale(I0, I1, z, z, warps=1, **PAR)
            assert gpu64.stats().fused[0] == unit, opts


EPSILONS = [0.08, 0.05, 0.03, 0.02, 0.012, 0.008]
LOOPS = {
    "cursor": dict(),
    "fixed_units": dict(fuse3_cursor=0),
    "cursor_rows4": dict(rows_per_wave3=4),
    "units_of_3": dict(fuse3_afac1=1e-30, fuse3_afac2=1e-30, fuse4_afac3=1e300),
    "units_of_1": dict(fuse3_afac1=1e300),
}


@pytest.mark.parametrize("mode", MODES)
def test_loops_end_on_every_position_inside_a_unit(gpu64, gpu32, synth, mode):
    """five warps per solve at six thresholds: with fixed units (fuse3_cursor = 0) a loop of n iterations ends on position
    (n - 1) % 4 of its unit, and the thirty loops cover all four; the cursor loop shortens its units near the stop, and with the
    ratios forced it runs units of three or of one throughout"""
    gpu = _gpu(mode, gpu64, gpu32)
    nx, ny = 113, 30
    I0, I1 = synth.pair("P1", nx, ny)
    z = np.zeros((ny, nx))
    ends = set()
    for eps in EPSILONS:
        with options(gpu, **_mode_opts(mode), **ITER1):
            want = gpu.tvl1_single_scale(I0, I1, z, z, warps=5, epsilon=eps, **PAR)
            table = gpu.stats().iterations().copy()
        ends |= {(int(n) - 1) % 4 for n in table.ravel()}
        for name, opts in LOOPS.items():
            with options(gpu, **_mode_opts(mode), **ITER4, **opts):
                got = gpu.tvl1_single_scale(I0, I1, z, z, warps=5, epsilon=eps, **PAR)
                st = gpu.stats()
            assert np.array_equal(st.iterations(), table), (name, eps, st.iterations(), table)
            assert st.fused[0] == 4
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, eps)
    assert ends == {0, 1, 2, 3}, ends


@pytest.mark.parametrize("mode", MODES)
def test_iteration_limit_that_is_no_multiple_of_the_unit(gpu64, gpu32, synth, mode):
    """a threshold far below any error: the loops run into the limit of 300 iterations; with units of three after the first unit
    of four the last unit is cut to 300 - 298 = 2 iterations"""
    gpu = _gpu(mode, gpu64, gpu32)
    nx, ny = 60, 9
    I0, I1 = synth.pair("P1", nx, ny)
    z = np.zeros((ny, nx))
    with options(gpu, **_mode_opts(mode), **ITER1):
        want = gpu.tvl1_single_scale(I0, I1, z, z, warps=2, epsilon=1e-30, **PAR)
        table = gpu.stats().iterations().copy()
    assert (table == 300).any(), table
    for name in ("cursor", "units_of_3", "fixed_units"):
        with options(gpu, **_mode_opts(mode), **ITER4, **LOOPS[name]):
            got = gpu.tvl1_single_scale(I0, I1, z, z, warps=2, epsilon=1e-30, **PAR)
            assert np.array_equal(gpu.stats().iterations(), table), name
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


@pytest.mark.parametrize("mode", MODES)
def test_pairs_of_a_group_stop_on_their_own(gpu64, gpu32, synth, mode):
    """three pairs in lockstep whose loops end at different iterations: each equals the pair solved alone"""
    import torch
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
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[0], tables[2])
    flo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device="cuda")
    for name in ("cursor", "fixed_units", "cursor_rows4"):
        flo.zero_()
        with options(gpu, **_mode_opts(mode), **ITER4, **LOOPS[name]):
            st = gpu.tvl1_group_dev([t.data_ptr() for t in d0], [t.data_ptr() for t in d1], [flo[k].data_ptr() for k in range(G)],
                                    nx, ny, **kw)
            gpu.synchronize()
        for k in range(G):
            assert np.array_equal(st[k].iterations(), tables[k]), (name, k)
            assert all(f == 4 for f in st[k].fused[:3]), (name, list(st[k].fused[:3]))
        assert torch.equal(flo.view(torch.int32), solo.view(torch.int32)), name


def test_multiscale_solve_against_the_oracle(gpu64, orc, synth):
    """130 x 70, three scales, strict mode: the oracle's iteration tables, the one-iteration kernel's flow"""
    I0, I1 = synth.pair("P1", 130, 70)
    _, _, it_o, _ = orc.tvl1_multiscale(I0, I1, nscales=3, **PAR)
    with options(gpu64, **ITER1):
        u1, v1 = gpu64.tvl1_multiscale(I0, I1, nscales=3, **PAR)
    with options(gpu64, **ITER4):
        u4, v4 = gpu64.tvl1_multiscale(I0, I1, nscales=3, **PAR)
        st = gpu64.stats()
    assert np.array_equal(st.iterations(), it_o), (st.iterations(), it_o)
    assert all(f == 4 for f in st.fused[:3])
    assert np.array_equal(u4, u1) and np.array_equal(v4, v1)
