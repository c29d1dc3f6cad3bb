"""The degenerate frames of tests/regimes.py through the TV-L1 family, TV-L1 with occlusions and the SOR solvers.

Every other whole-solver test feeds smooth textures with 1-6 px of motion.  Here the inputs are still, constant, half constant,
binary, almost without contrast, far outside 0..255, noisy, and displaced further than the pyramid can follow (what each of
them means is pinned on the CPU in tests/test_regimes_cpu.py).  Three mechanisms are at stake:

* stop detection on the device from error slots that start as zeros: on a still or constant pair the error of the very first
  sweep is exactly 0.0, the value of an untouched slot, and the loop ends inside its first launch unit of 2, 3 or 4 iterations
  (or a tile of K), so iteration 1 has to be rebuilt from the unit's input -- alone, and frozen from the first launch in a
  lockstep group whose other pairs run into the limit of 300;
* the flat-pixel rule (grad < 1e-10 gives d = 0) and its clamp form in the tolerance mode, on whole waves of flat pixels beside
  live ones inside a solve;
* the out-of-image branch of the bicubic warp with its mask, for many pixels at once.

No bar is new: every assertion is the one the suite holds for the same entry and mode on synth.pair (named at each test).
131 x 77, three scales, two warps unless stated.

Measured on an MI355X (OFX_MEASURE_OUT=<file> writes them), worst over the five schedules and both thresholds.  strict: lone
strict f64 solve against the oracle, max |delta flow|; tolerance: lone tolerance-mode solve against its restatement, max |delta
flow|, beside the largest bar it is held to, max(1e-9, 10 cond), cond being the distance of the two CPU restatements; float:
float storage in the group of 8 against the strict oracle, AEPE in px (bar 1e-4):

               strict    tolerance   (bar)       float
    still      0.0       0.0         1e-9        0.0
    flat       0.0       0.0         1e-9        0.0
    halfflat   0.0       3.1e-13     1e-9        3.7e-06
    binary     0.0       4.4e-11     1e-9        1.6e-06
    faded      0.0       1.7e-13     1e-9        7.3e-06
    wide       0.0       1.6e-13     1e-9        3.1e-07
    noisy      0.0       7.1e-13     1e-9        3.9e-07
    far        0.0       5.7e-09     8.1e-9      6.1e-05

(`far` at epsilon = 0, 300 iterations in every cell, is the one solve that carries a last-bit difference beyond 1e-9: its two CPU
restatements differ by 8.1e-10 there; at epsilon = 0.01 it differs from its restatement by 9.7e-11.)

The file was also run against three deliberately wrong builds of the library (decisions and arithmetic only, no address depends
on them): a first-sweep error of 0.0 reported as n = 2 by the finalize kernels fails 71 of the 215 tests (a, b, c, d, f); every
pair of a lockstep group read from the buffer in which the longest-running pair ended fails 15 (c, d); the flat-pixel threshold
lowered from 1e-10 to 1e-30 fails 49 (a, b, strict c, the video chain -- `halfflat` and `binary` alone, as intended).
"""
import contextlib
import json
import os

import numpy as np
import pytest
from conftest import aepe

import flow_consistency_ref as fcr
import regimes as R
import tvl1_warm_ref as W

pytestmark = pytest.mark.gpu

NX, NY = R.NX, R.NY
PAR = dict(tau=0.25, lam=0.15, theta=0.3)
EPSILONS = [0.01, 0.0]
ONES = np.ones((R.TVL1["nscales"], R.TVL1["warps"]), dtype=int)

# the library's defaults of every option this file touches (ofx_ctx.cpp)
DEFAULTS = dict(relaxed_dual=0, tile=0, fuse3=2, fuse3_cursor=1, fuse4=2, fuse4_min_px=0, rof_pipe=1, chi_fuse=1, rof_window=0,
                sor_exact=1, sor_fuse=0)

# the four schedules of test_gpu_tvl1.py's tile_mode fixture and the four-iteration kernel as test_gpu_tvl1_iter4.py forces it
# -> (options, iterations per launch unit that the work record must name)
SCHEDULES = {
    "strips": (dict(tile=0, fuse3=0), 2),
    "tile4": (dict(tile=4, fuse3=0), 4),
    "fuse3": (dict(tile=0, fuse3=1, fuse3_cursor=1), 3),
    "fuse3_fixed_units": (dict(tile=0, fuse3=1, fuse3_cursor=0), 3),
    "fuse4": (dict(fuse4=1, fuse4_min_px=0), 4),
}
GROUP_SCHEDULES = {"default": {}, "fuse3": dict(fuse3=1, fuse3_cursor=1), "fuse4": dict(fuse4=1, fuse4_min_px=0)}
GROUP_CASES = [(8, "default"), (8, "fuse3"), (8, "fuse4"), (16, "default")]

MEASURED = {}


def _measure(key, value):
    MEASURED[key] = max(MEASURED.get(key, value), value)


@pytest.fixture(scope="module", autouse=True)
def _record():
    """OFX_MEASURE_OUT=<file>: write the worst deviations seen (the numbers of the header)"""
    yield
    out = os.environ.get("OFX_MEASURE_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


@contextlib.contextmanager
def options(*ctxs, **kw):
    try:
        for c in ctxs:
            for k, v in kw.items():
                c.set_option(k, v)
        yield
    finally:
        for c in ctxs:
            for k in kw:
                c.set_option(k, DEFAULTS[k])


def _dev(planes, dtype):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(p)).to("cuda", dtype) for p in planes]
    torch.cuda.synchronize()
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _payload(u, v):
    return np.stack([u, v], axis=-1).astype(np.float32)


def _tvl1_group(ctx, d0, d1, **kw):
    """ofx_tvl1_group_dev on lists of device tensors -> (payloads (G, ny, nx, 2) float32, iteration tables)"""
    import torch
    G = len(d0)
    flo = torch.full((G, NY, NX, 2), np.nan, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = ctx.tvl1_group_dev(_ptrs(d0), _ptrs(d1), [flo[g].data_ptr() for g in range(G)], NX, NY, **kw)
    ctx.synchronize()
    return flo.cpu().numpy(), [s.iterations().copy() for s in st]


def _tvl1_lone(ctx, a, b, **kw):
    """ofx_tvl1_multiscale_dev -> (payload (ny, nx, 2) float32, iteration table)"""
    import torch
    flo = torch.full((NY, NX, 2), np.nan, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.tvl1_multiscale_dev(a.data_ptr(), b.data_ptr(), flo.data_ptr(), NX, NY, **kw)
    ctx.synchronize()
    return flo.cpu().numpy(), ctx.stats().iterations().copy()


# ---- a. lone TV-L1, strict: test_gpu_tvl1.py's test_multiscale_matches_oracle / test_gpu_fuzz.py's test_tvl1_random_configurations ----
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("name", R.NAMES)
def test_lone_strict_is_the_oracle(gpu64, orc, name, schedule, epsilon):
    """iteration tables equal, errors to 1e-9 relative -- an error of exactly 0.0 where the oracle's is --, flows to 1e-9 (0.0 is
    expected and printed); a still or constant pair gives n = 1 in every cell and an exactly zero flow"""
    I0, I1 = R.pair(name, NX, NY)
    uo, vo, it_o, err_o = R.oracle_tvl1(orc, name, epsilon)
    opts, unit = SCHEDULES[schedule]
    with options(gpu64, **opts):
        ug, vg = gpu64.tvl1_multiscale(I0, I1, epsilon=epsilon, **R.TVL1)
        st = gpu64.stats()
    assert all(f == unit for f in st.fused[:R.TVL1["nscales"]]), list(st.fused[:R.TVL1["nscales"]])     # the kernel that was asked for
    assert np.array_equal(st.iterations(), it_o), (st.iterations(), it_o, st.errors(), err_o)
    assert np.allclose(st.errors(), err_o, rtol=1e-9, atol=0.0), (st.errors(), err_o)
    d = max(float(np.abs(ug - uo).max()), float(np.abs(vg - vo).max()))
    print("%s %s epsilon=%g: max abs against the oracle %.3g" % (name, schedule, epsilon, d))
    _measure("strict_max_abs/" + name, d)
    assert d < 1e-9, d
    if name in R.FROZEN:
        assert np.array_equal(st.iterations(), ONES)
        assert np.array_equal(st.errors(), np.zeros(ONES.shape))
        assert np.array_equal(ug, np.zeros((NY, NX))) and np.array_equal(vg, np.zeros((NY, NX)))


# ---- b. lone TV-L1, tolerance mode: the rule of test_gpu_fuzz.py's test_tolerance_mode_random_configurations ------------------------
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("name", R.NAMES)
def test_lone_tolerance_mode_is_its_restatement(gpu64, orc, name, schedule, epsilon):
    """against orc.tvl1_multiscale_mode(relaxed = 1): equal tables, flows within max(1e-9, 10 cond), errors within
    max(1e-9, 10 cond_err) relative, cond being the distance of the two CPU restatements (never a GPU figure)"""
    I0, I1 = R.pair(name, NX, NY)
    ur, vr, it_r, err_r = R.oracle_tvl1(orc, name, epsilon, relaxed=1)
    cond, cond_err = R.cond(orc, name, epsilon)
    opts, unit = SCHEDULES[schedule]
    with options(gpu64, relaxed_dual=1, **opts):
        ug, vg = gpu64.tvl1_multiscale(I0, I1, epsilon=epsilon, **R.TVL1)
        st = gpu64.stats()
    assert all(f == unit for f in st.fused[:R.TVL1["nscales"]]), list(st.fused[:R.TVL1["nscales"]])
    assert np.isfinite(ug).all() and np.isfinite(vg).all()
    assert np.array_equal(st.iterations(), it_r), (st.iterations(), it_r, st.errors(), err_r)
    d = max(float(np.abs(ug - ur).max()), float(np.abs(vg - vr).max()))
    print("%s %s epsilon=%g: max abs against the restatement %.3g (cond %.3g)" % (name, schedule, epsilon, d, cond))
    _measure("tolerance_max_abs/" + name, d)
    assert d < max(1e-9, 10 * cond), (d, cond)
    assert np.allclose(st.errors(), err_r, rtol=max(1e-9, 10 * cond_err), atol=0.0), (st.errors(), err_r, cond_err)
    if name in R.FROZEN:
        assert np.array_equal(st.iterations(), ONES)
        assert np.array_equal(ug, np.zeros((NY, NX))) and np.array_equal(vg, np.zeros((NY, NX)))


# ---- c. mixed lockstep groups ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("G,schedule", GROUP_CASES)
def test_mixed_group_strict_is_the_oracle_pair_for_pair(gpu64, orc, G, schedule, epsilon):
    """test_gpu_tvl1.py's test_lockstep_group_equals_pairs_solved_alone: every table the oracle's, every float32 payload the
    oracle's flow cast to float32, bit for bit -- in a group with pairs frozen from the first launch (first and last slot of 16)
    beside pairs that run into the limit"""
    import torch
    names = R.group_names(G)
    pairs = R.group(NX, NY, G)
    d0, d1 = _dev([p[0] for p in pairs], torch.float64), _dev([p[1] for p in pairs], torch.float64)
    with options(gpu64, **GROUP_SCHEDULES[schedule]):
        got, tables = _tvl1_group(gpu64, d0, d1, epsilon=epsilon, **R.TVL1)
    # the group is what it claims
    assert any(np.array_equal(t, ONES) for t in tables), tables
    if epsilon == 0.0:
        assert any((t == R.MAX_ITERATIONS).all() for t in tables), tables
    if G == 16:
        assert np.array_equal(tables[0], ONES) and np.array_equal(tables[-1], ONES)
    for g, name in enumerate(names):
        uo, vo, it_o, _ = R.oracle_tvl1(orc, name, epsilon)
        assert np.array_equal(tables[g], it_o), (g, name, tables[g], it_o)
        assert np.array_equal(got[g], _payload(uo, vo)), (g, name, float(np.abs(got[g][..., 0] - uo).max()))
        if name in R.FROZEN:
            assert not got[g].any(), (g, name)


_alone = {}


def _solved_alone(mode, gpu, name, epsilon):
    """ofx_tvl1_multiscale_dev on one pair with the library's own kernel choice, once per (mode, regime, epsilon)"""
    import torch
    key = (mode, name, epsilon)
    if key not in _alone:
        dt = torch.float32 if mode == "f32" else torch.float64
        a, b = _dev(R.pair(name, NX, NY), dt)
        with options(gpu, **(dict(relaxed_dual=1) if mode == "tol64" else {})):
            _alone[key] = _tvl1_lone(gpu, a, b, epsilon=epsilon, **R.TVL1)
    return _alone[key]


@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("G,schedule", GROUP_CASES)
@pytest.mark.parametrize("mode", ["tol64", "f32"])
def test_mixed_group_in_the_other_modes_is_the_pair_alone(gpu64, gpu32, mode, G, schedule, epsilon):
    """the f64 tolerance mode and float storage (test_gpu_relaxed_modes.py's test_group_solves_give_the_same_bits_with_every_kernel):
    payload and table of every pair equal ofx_tvl1_multiscale_dev on that pair alone, bit for bit; still and flat give exact
    zeros and tables of ones; everything is finite"""
    import torch
    gpu = gpu32 if mode == "f32" else gpu64
    dt = torch.float32 if mode == "f32" else torch.float64
    names = R.group_names(G)
    pairs = R.group(NX, NY, G)
    d0, d1 = _dev([p[0] for p in pairs], dt), _dev([p[1] for p in pairs], dt)
    with options(gpu, **(dict(relaxed_dual=1) if mode == "tol64" else {}), **GROUP_SCHEDULES[schedule]):
        got, tables = _tvl1_group(gpu, d0, d1, epsilon=epsilon, **R.TVL1)
    assert np.isfinite(got).all()
    for g, name in enumerate(names):
        want, it_w = _solved_alone(mode, gpu, name, epsilon)
        assert np.array_equal(tables[g], it_w), (g, name, tables[g], it_w)
        assert got[g].tobytes() == want.tobytes(), (g, name, float(np.abs(got[g] - want).max()))
        if name in R.FROZEN:
            assert np.array_equal(tables[g], ONES) and not got[g].any(), (g, name)
    if epsilon == 0.0:
        assert any((t == R.MAX_ITERATIONS).all() for t in tables), tables


def test_mixed_group_float_storage_against_the_strict_oracle(gpu32, orc):
    """BASELINE.json's north star (AEPE < 1e-4 px) on the regimes whose two CPU restatements agree to 1e-9 (which
    tests/test_regimes_cpu.py asserts of every regime at this threshold); the others are printed only"""
    import torch
    names = R.group_names(8)
    pairs = R.group(NX, NY, 8)
    d0, d1 = _dev([p[0] for p in pairs], torch.float32), _dev([p[1] for p in pairs], torch.float32)
    got, _ = _tvl1_group(gpu32, d0, d1, epsilon=0.01, **R.TVL1)
    assert np.isfinite(got).all()
    failed = []
    for g, name in enumerate(names):
        uo, vo, _, _ = R.oracle_tvl1(orc, name, 0.01)
        e = aepe(got[g][..., 0].astype(np.float64), got[g][..., 1].astype(np.float64), uo, vo)
        asserted = R.cond(orc, name, 0.01)[0] < 1e-9
        print("%s: AEPE of float storage against the strict oracle %.3g px%s" % (name, e, "" if asserted else " (not asserted)"))
        _measure("f32_aepe/" + name, e)
        if asserted and not e < 1e-4:
            failed.append((name, e))
    assert not failed, failed


# ---- d. both ways, and the video chain ----------------------------------------------------------------------------------------------------
def test_both_ways_on_the_mixed_group(gpu64, orc):
    """test_gpu_tvl1_bidir.py's contract: both payloads and tables of every pair equal the lone solve of the ordered pair, the
    byte maps equal tests/flow_consistency_ref.py on the payloads"""
    import torch
    G = 8
    names = R.group_names(G)
    pairs = R.group(NX, NY, G)
    A, B = _dev([p[0] for p in pairs], torch.float64), _dev([p[1] for p in pairs], torch.float64)
    flo = torch.full((2, G, NY, NX, 2), np.nan, dtype=torch.float32, device="cuda")
    occ = torch.full((2, G, NY, NX), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = gpu64.tvl1_bidir_group_dev(_ptrs(A), _ptrs(B), [flo[0, g].data_ptr() for g in range(G)], [flo[1, g].data_ptr() for g in range(G)],
                                    [occ[0, g].data_ptr() for g in range(G)], [occ[1, g].data_ptr() for g in range(G)], NX, NY, **R.TVL1)
    gpu64.synchronize()
    f, o = flo.cpu().numpy(), occ.cpu().numpy()
    assert len(st) == 2 * G and np.isfinite(f).all()
    for g, name in enumerate(names):
        pf, itf = _tvl1_lone(gpu64, A[g], B[g], **R.TVL1)
        pb, itb = _tvl1_lone(gpu64, B[g], A[g], **R.TVL1)
        assert f[0, g].tobytes() == pf.tobytes(), ("forward payload", name)
        assert f[1, g].tobytes() == pb.tobytes(), ("backward payload", name)
        assert np.array_equal(st[g].iterations(), itf), ("forward iterations", name, st[g].iterations(), itf)
        assert np.array_equal(st[G + g].iterations(), itb), ("backward iterations", name, st[G + g].iterations(), itb)
        rf, rb, _ = fcr.maps(orc, f[0, g], f[1, g])
        assert np.array_equal(o[0, g], rf) and np.array_equal(o[1, g], rb), name
        if name in R.FROZEN:
            assert np.array_equal(st[g].iterations(), ONES) and np.array_equal(st[G + g].iterations(), ONES), name
            assert not f[:, g].any() and not o[:, g].any(), name               # zero flows are consistent everywhere
    assert (o == 255).any()                                                     # ... and the others are not


def test_video_chain_on_degenerate_sequences(gpu64, orc):
    """test_gpu_tvl1_warm.py's two statements for ofx_tvl1_sequence_group_dev: every step is the lone warm entry on that pair from
    the payload of the step before (bytes, tables), and the restatement of tests/tvl1_warm_ref.py (tables, flows to 1e-9).  A
    warm start from an all-zero payload on a still pair stays exactly zero."""
    import torch
    names = ["still", "flat", "halfflat", "noisy"]
    n_frames, ns_first, ns_next = 4, 3, 1
    kw = dict(warps=R.TVL1["warps"], **PAR)
    seqs = [R.sequence(name, NX, NY, n_frames) for name in names]
    F = [_dev(s, torch.float64) for s in seqs]
    flo = torch.full((len(names), n_frames - 1, NY, NX, 2), np.nan, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = gpu64.tvl1_sequence_group_dev([_ptrs(f) for f in F], [[flo[q, t].data_ptr() for t in range(n_frames - 1)] for q in range(len(names))],
                                       NX, NY, nscales_first=ns_first, nscales_next=ns_next, **kw)
    gpu64.synchronize()
    got = flo.cpu().numpy()
    assert np.isfinite(got).all()
    for q, name in enumerate(names):
        for t in range(n_frames - 1):
            ns = ns_next if t else ns_first
            table = st[q][t].iterations()
            assert st[q][t].nscales == ns
            prev = got[q, t - 1] if t else None
            start = torch.from_numpy(prev).cuda() if t else None
            lone = torch.full((NY, NX, 2), np.nan, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            st1 = gpu64.tvl1_group_init_dev([F[q][t].data_ptr()], [F[q][t + 1].data_ptr()], [start.data_ptr() if t else None],
                                            [lone.data_ptr()], NX, NY, nscales=ns, **kw)
            gpu64.synchronize()
            assert got[q, t].tobytes() == lone.cpu().numpy().tobytes(), (name, t)
            assert np.array_equal(table, st1[0].iterations()), (name, t)
            uo, vo, it_o, _ = W.tvl1_multiscale_warm(orc, seqs[q][t], seqs[q][t + 1], prev, nscales=ns, **kw)
            assert np.array_equal(table, it_o), (name, t, table, it_o)
            d = float(np.abs(got[q, t].astype(np.float64) - W.payload_of(uo, vo).astype(np.float64)).max())
            assert d < 1e-9, (name, t, d)
            if name in R.FROZEN:
                assert (table == 1).all() and not got[q, t].any(), (name, t, table)
    assert got[2].any() and got[3].any()


# ---- e. TV-L1 with occlusions ---------------------------------------------------------------------------------------------------------------
OCC = dict(lam=0.15, alpha=0.01, beta=0.15, theta=0.3, nscales=2, zfactor=0.5, warps=1, epsilon=0.01)
_occ_oracle = {}


def _occ_want(orc, name):
    if name not in _occ_oracle:
        seq = R.sequence(name, NX, NY, 3)
        _occ_oracle[name] = orc.tvl1occ_multiscale(seq[0], seq[1], seq[2], **OCC)
    return _occ_oracle[name]


@pytest.mark.parametrize("pipe", [1, 0], ids=["pipelined", "serial"])
@pytest.mark.parametrize("name", R.NAMES)
def test_tvl1occ_is_the_oracle(gpu64, orc, name, pipe):
    """test_gpu_occ.py's test_tvl1occ_multiscale: flows, occlusion map and outer-iteration table bit-equal to the oracle, under
    both schedules of the iterative solvers"""
    seq = R.sequence(name, NX, NY, 3)
    uo, vo, co, it = _occ_want(orc, name)
    with options(gpu64, rof_pipe=pipe, chi_fuse=pipe, rof_window=0):
        u, v, c = gpu64.tvl1occ_multiscale(seq[0], seq[1], seq[2], **OCC)
        st = gpu64.stats()
    got = np.array([[st.iters[s][w] for w in range(OCC["warps"])] for s in range(OCC["nscales"])])
    assert np.array_equal(got, it), (got, it)
    assert np.array_equal(u, uo) and np.array_equal(v, vo) and np.array_equal(c, co), float(np.abs(u - uo).max())
    if name in R.FROZEN:
        assert not u.any() and not v.any()


def test_tvl1occ_all_regimes_in_one_batch(ofx_mod, gpu64):
    """test_gpu_occ.py's test_tvl1occ_lockstep_group_with_different_iteration_counts: the eight triples in lockstep on one context
    (one group of 8, and lockstep = 4: two groups of 4), every result equal to the triple solved alone"""
    ctx = ofx_mod.Ofx(0, ofx_mod.F64)
    try:
        triples = [tuple(R.sequence(name, NX, NY, 3)) for name in R.NAMES]
        alone, tables = [], []
        for t in triples:
            alone.append(gpu64.tvl1occ_multiscale(*t, **OCC))
            st = gpu64.stats()
            tables.append(tuple(st.iters[s][w] for s in range(OCC["nscales"]) for w in range(OCC["warps"])))
        assert len(set(tables)) > 1, tables                     # the group is heterogeneous
        for lockstep in (0, 4):
            ctx.set_option("lockstep", lockstep)
            got = ofx_mod.tvl1occ_batch([ctx], triples, **OCC)
            for name, g, w in zip(R.NAMES, got, alone):
                assert all(np.array_equal(x, y) for x, y in zip(g, w)), (name, lockstep)
    finally:
        ctx.close()


# ---- f. Horn-Schunck and Brox spatial --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_sor_lone_entries_are_the_oracle(gpu64, orc, name):
    """test_gpu_fuzz.py's test_sor_random_configurations: equal sweep tables, flows to 1e-11 (Horn-Schunck) and 1e-10 (Brox)"""
    I0, I1 = R.pair(name, NX, NY)
    uo, vo, it_o = R.oracle_sor(orc, "hs", name)
    ug, vg = gpu64.hs_pyramidal(I0, I1, **R.HS)
    assert np.array_equal(gpu64.stats().iterations(), it_o), (gpu64.stats().iterations(), it_o)
    assert np.abs(ug - uo).max() < 1e-11 and np.abs(vg - vo).max() < 1e-11
    if name in R.FROZEN:
        assert (it_o == 1).all() and not ug.any() and not vg.any()
    uo, vo, it_o = R.oracle_sor(orc, "brox", name)
    ug, vg = gpu64.brox_spatial(I0, I1, **R.BROX)
    assert np.array_equal(gpu64.stats().iterations(), it_o), (gpu64.stats().iterations(), it_o)
    assert np.abs(ug - uo).max() < 1e-10 and np.abs(vg - vo).max() < 1e-10
    if name in R.FROZEN:
        assert (it_o == 1).all() and not ug.any() and not vg.any()


def _sor_groups(gpu64, d0, d1):
    """ofx_hs_group_dev and ofx_brox_group_dev on the group -> {"hs" | "brox": (payloads, sweep tables)}"""
    import torch
    G = len(d0)
    out = {}
    for kind, run, kw in (("hs", gpu64.hs_group_dev, R.HS), ("brox", gpu64.brox_group_dev, R.BROX)):
        flo = torch.full((G, NY, NX, 2), np.nan, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = run(_ptrs(d0), _ptrs(d1), [flo[g].data_ptr() for g in range(G)], NX, NY, **kw)
        gpu64.synchronize()
        out[kind] = (flo.cpu().numpy(), [s.iterations().copy() for s in st])
    return out


def _group_holds_a_frozen_and_a_capped_pair(tables):
    assert any((t == 1).all() for t in tables), tables
    assert any((t == R.HS["maxiter"]).any() for t in tables), tables


def test_sor_exact_mixed_groups(gpu64, orc):
    """test_gpu_fuzz.py's test_sor_random_lockstep_groups: sweep tables equal the oracle's (reference sweep order); the Horn-Schunck
    payload is the oracle's flow cast to float32, Brox's within 1e-6 with fewer than 1e-3 of the float32 casts off"""
    import torch
    names = R.group_names(8)
    pairs = R.group(NX, NY, 8)
    res = _sor_groups(gpu64, _dev([p[0] for p in pairs], torch.float64), _dev([p[1] for p in pairs], torch.float64))
    _group_holds_a_frozen_and_a_capped_pair(res["hs"][1])
    for g, name in enumerate(names):
        got, tables = res["hs"]
        uo, vo, it = R.oracle_sor(orc, "hs", name)
        assert np.array_equal(tables[g], it), ("hs", name, tables[g], it)
        assert np.abs(got[g][..., 0] - uo).max() < 1e-6 and np.array_equal(got[g], _payload(uo, vo)), ("hs", name)
        got, tables = res["brox"]
        uo, vo, it = R.oracle_sor(orc, "brox", name)
        assert np.array_equal(tables[g], it), ("brox", name, tables[g], it)
        assert np.abs(got[g][..., 0] - uo).max() < 1e-6, ("brox", name)
        assert np.mean(got[g] != _payload(uo, vo)) < 1e-3, ("brox", name)
        if name in R.FROZEN:
            assert not res["hs"][0][g].any() and not res["brox"][0][g].any(), name


@pytest.mark.parametrize("sor_fuse", [0, 2])
def test_sor_tolerance_mode_mixed_groups(gpu64, orc, sor_fuse):
    """test_gpu_fuzz.py's test_sor_tolerance_mode_random_lockstep_groups with the library's default geometry (colour order, tiles
    of 128 x 64, the finest level as a checkerboard of tiles): tables and payloads bit-equal to the oracle's restatement"""
    import torch
    names = R.group_names(8)
    pairs = R.group(NX, NY, 8)
    d0, d1 = _dev([p[0] for p in pairs], torch.float64), _dev([p[1] for p in pairs], torch.float64)
    orc.set_sor_order(1)
    orc.set_sor_tile(128, 64)
    orc.set_sor_wave_levels(1)
    try:
        with options(gpu64, sor_exact=0, sor_fuse=sor_fuse):
            res = _sor_groups(gpu64, d0, d1)
        _group_holds_a_frozen_and_a_capped_pair(res["hs"][1])
        for g, name in enumerate(names):
            for kind in ("hs", "brox"):
                got, tables = res[kind]
                uo, vo, it = R.oracle_sor(orc, kind + "_tol", name)
                assert np.isfinite(got[g]).all(), (kind, name)
                assert np.array_equal(tables[g], it), (kind, name, tables[g], it)
                assert np.array_equal(got[g], _payload(uo, vo)), (kind, name, float(np.abs(got[g][..., 0] - uo).max()))
                if name in R.FROZEN:
                    assert (it == 1).all() and not got[g].any(), (kind, name)
    finally:
        orc.set_sor_order(0)
        orc.set_sor_tile(128, 64)
        orc.set_sor_wave_levels(0)
