"""ofx_flow_compose_dev, ofx_flow_accumulate_dev and ofx_flow_tracks_dev against the numpy restatement (tests/flow_compose_ref.py):
payload floats bit for bit, the frozen ones included, maps byte for byte, track doubles and lengths equal -- at 2x2, 3x5, 67x5,
131x3 (fewer rows than a workgroup, a last column block of 3), 37x29, 130x70 (several blocks both ways) and the jump; 1, 3, 16 and
17 slots or sequences (two launches); 1, 2 and 5 steps; maps at byte offsets 0, 1 and 3, payloads 8 but not 16 bytes aligned; guard
bytes around every destination; in place; NaN and Inf; both storage precisions; host buffers; every refusal."""
import numpy as np
import pytest

import flow_compose_ref as R

pytestmark = pytest.mark.gpu

ERR_ARG = 1
GUARD = 64                                 # bytes before and behind every destination
FILL = 0xA5
SHAPES = list(R.CASES)


class Dev:
    """device buffers of one call: inputs at a byte offset into their allocation, destinations between guard bytes"""

    def __init__(self):
        self.keep, self.outs = [], []

    def put(self, arr, off=0):
        import torch
        if arr is None:
            return None
        raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8).copy()
        t = torch.zeros(off + raw.size + 16, dtype=torch.uint8, device="cuda")
        t[off:off + raw.size] = torch.from_numpy(raw).cuda()
        self.keep.append(t)
        return t.data_ptr() + off

    def out(self, nbytes, off=0, init=None):
        """-> (pointer, handle for get); init: bytes that the destination holds before the call (in place)"""
        import torch
        t = torch.full((GUARD + off + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        if init is not None:
            t[GUARD + off:GUARD + off + nbytes] = torch.from_numpy(np.frombuffer(np.ascontiguousarray(init).tobytes(), dtype=np.uint8).copy()).cuda()
        self.outs.append(t)
        return t.data_ptr() + GUARD + off, (t, off, nbytes)

    @staticmethod
    def get(handle, dtype, shape):
        t, off, nbytes = handle
        raw = t.cpu().numpy()
        assert (raw[:GUARD + off] == FILL).all() and (raw[GUARD + off + nbytes:] == FILL).all(), "bytes outside the destination were written"
        return np.frombuffer(raw[GUARD + off:GUARD + off + nbytes].tobytes(), dtype=dtype).reshape(shape)


def sync():
    import torch
    torch.cuda.synchronize()


def run_compose(ctx, slots, flo_off=0, occ_off=0, want_map=True, inplace=False):
    """slots: list of (ab | None, occ_ab | None, bc, occ_bc | None) -> list of (ac, occ_ac | None)"""
    ny, nx, _ = slots[0][2].shape
    d = Dev()
    tab = {k: [] for k in ("ab", "occ_ab", "bc", "occ_bc", "ac", "occ_ac")}
    handles = []
    for ab, occ_ab, bc, occ_bc in slots:
        tab["bc"].append(d.put(bc, flo_off))
        tab["occ_bc"].append(d.put(occ_bc, occ_off))
        if inplace:
            pa, ha = d.out(nx * ny * 8, flo_off, init=np.zeros_like(bc) if ab is None else ab)
            po, ho = d.out(nx * ny, occ_off, init=np.zeros((ny, nx), dtype=np.uint8) if occ_ab is None else occ_ab)
            tab["ab"].append(pa)
            tab["occ_ab"].append(po)
        else:
            tab["ab"].append(d.put(ab, flo_off))
            tab["occ_ab"].append(d.put(occ_ab, occ_off))
            pa, ha = d.out(nx * ny * 8, flo_off)
            po, ho = d.out(nx * ny, occ_off) if want_map else (None, None)
        tab["ac"].append(pa)
        tab["occ_ac"].append(po)
        handles.append((ha, ho))
    sync()
    none_if_empty = lambda xs: xs if any(x is not None for x in xs) else None
    ctx.flow_compose_dev(tab["bc"], tab["ac"], nx, ny, d_flo_ab=none_if_empty(tab["ab"]), d_occ_ab=none_if_empty(tab["occ_ab"]),
                         d_occ_bc=none_if_empty(tab["occ_bc"]), d_occ_ac=none_if_empty(tab["occ_ac"]))
    ctx.synchronize()
    return [(d.get(ha, np.float32, (ny, nx, 2)), None if ho is None else d.get(ho, np.uint8, (ny, nx))) for ha, ho in handles]


def chain_slots(orc, name, n_steps, with_maps):
    """the chain of a case as independent compose slots: slot t composes the restatement's acc[t - 1] with step t"""
    steps = R.steps(name, n_steps)
    maps = R.step_maps(orc, name, n_steps) if with_maps else [None] * n_steps
    acc = R.want(orc, name, n_steps, with_maps)
    slots = [(None if t == 0 else acc[t - 1][0], None if t == 0 else acc[t - 1][1], steps[t], maps[t]) for t in range(n_steps)]
    return slots, acc


def same(got, want):
    return got[0].tobytes() == want[0].tobytes() and (got[1] is None or got[1].tobytes() == want[1].tobytes())


@pytest.mark.parametrize("name", SHAPES)
def test_compose_is_the_restatement(gpu64, orc, name):
    for with_maps in (False, True):
        slots, acc = chain_slots(orc, name, 5, with_maps)
        for flo_off, occ_off in ((0, 0), (8, 1), (0, 3)):
            got = run_compose(gpu64, slots, flo_off, occ_off)
            for t in range(5):
                assert same(got[t], acc[t]), (with_maps, flo_off, occ_off, t)
        got = run_compose(gpu64, slots, want_map=False)                  # the map is not wanted: the payloads are the same
        for t in range(5):
            assert got[t][1] is None and same(got[t], acc[t]), (with_maps, t)


@pytest.mark.parametrize("n", [1, 3, 16, 17])
def test_any_number_of_slots_16_per_launch(gpu64, orc, n):
    base = []
    for name in ("37x29",):
        for with_maps in (True, False):
            slots, acc = chain_slots(orc, name, 5, with_maps)
            base += list(zip(slots, acc))
    picked = [base[(3 * g) % len(base)] for g in range(n)]             # slot 16, the second launch, has maps
    got = run_compose(gpu64, [s for s, _ in picked], occ_off=1)
    assert len(got) == n
    for g in range(n):
        assert same(got[g], picked[g][1]), g


def test_in_place_streaming_and_mixed_null_entries(gpu64, orc):
    name = "130x70"
    slots, acc = chain_slots(orc, name, 5, True)
    got = run_compose(gpu64, slots, flo_off=8, occ_off=3, inplace=True)          # ac == ab and occ_ac == occ_ab
    for t in range(5):
        assert same(got[t], acc[t]), t
    # slots with and without each optional buffer in one launch
    s4 = slots[4]
    mixed = [s4, (s4[0], None, s4[2], s4[3]), (s4[0], s4[1], s4[2], None), (None, None, s4[2], None)]
    got = run_compose(gpu64, mixed, occ_off=1)
    for g, (ab, occ_ab, bc, occ_bc) in enumerate(mixed):
        assert same(got[g], R.compose(ab, bc, occ_ab, occ_bc)), g


def test_nan_and_inf_step_vectors_and_frozen_nan_bits(gpu64, orc):
    steps = R.nonfinite_steps()
    maps = R.step_maps(orc, "37x29")
    acc = R.accumulate(steps, maps)
    assert any((b == R.BR_NONFINITE).any() for _, _, b in acc)
    slots = [(None if t == 0 else acc[t - 1][0], None if t == 0 else acc[t - 1][1], steps[t], maps[t]) for t in range(5)]
    # an accumulated payload that holds NaNs with payload bits and an Inf: frozen bit for bit, with and without a map that says so
    a = np.array(acc[1][0])
    a[3, 4] = np.frombuffer(np.array([0x7FC12345, 0xFF800000], dtype=np.uint32).tobytes(), dtype=np.float32)
    a[5, 6] = np.frombuffer(np.array([0xFFC00001, 0x3F800000], dtype=np.uint32).tobytes(), dtype=np.float32)
    slots += [(a, acc[1][1], steps[2], maps[2]), (a, None, steps[2], None)]
    want = list(acc) + [R.compose(a, steps[2], acc[1][1], maps[2]), R.compose(a, steps[2])]
    got = run_compose(gpu64, slots)
    for g in range(len(slots)):
        assert same(got[g], want[g]), g
    assert got[6][0][3, 4].tobytes() == a[3, 4].tobytes() and got[6][1][3, 4] == 255 and got[6][1][5, 6] == 255


def test_zero_flow_and_zero_step_consequences(gpu64, orc):
    for name in ("37x29", R.JUMP):
        bc, m = R.steps(name)[0], R.step_maps(orc, name)[0]
        ab = R.steps(name)[1]
        ny, nx, _ = bc.shape
        zero = np.zeros_like(bc)
        got = run_compose(gpu64, [(None, None, bc, None), (zero, None, bc, m), (ab, None, zero, None)])
        i, j = R._grid(ny, nx)
        stays = R.inside(j + bc[..., 0].astype(np.float64), i + bc[..., 1].astype(np.float64), nx, ny)
        assert np.array_equal(got[0][1] == 0, stays) and got[0][0][stays].tobytes() == bc[stays].tobytes() and not got[0][0][~stays].any()
        ok = stays & (m == 0)
        assert np.array_equal(got[1][1] == 0, ok) and got[1][0][ok].tobytes() == bc[ok].tobytes() and not got[1][0][~ok].any()
        goes = R.inside(j + ab[..., 0].astype(np.float64), i + ab[..., 1].astype(np.float64), nx, ny)
        assert got[2][0].tobytes() == ab.tobytes() and np.array_equal(got[2][1] == 0, goes)


def run_accumulate(ctx, seqs, maps=None, occ_out="all", flo_off=0, occ_off=0, inplace=False):
    """seqs: [sequence][step] payloads; maps: None or the same shape (entries may be None); occ_out: "all", None (no table) or a
    function (q, t) -> bool.  -> [sequence][step] (acc, occ | None)"""
    ny, nx, _ = seqs[0][0].shape
    d = Dev()
    step = [[d.put(s, flo_off) for s in q] for q in seqs]
    occ_step = None if maps is None else [[d.put(m, occ_off) for m in q] for q in maps]
    acc, occ_acc, handles = [], [], []
    for qi, q in enumerate(seqs):
        pa, po, hs = [], [], []
        shared = d.out(nx * ny * 8, flo_off) if inplace else None
        for t in range(len(q)):
            p, h = shared if inplace else d.out(nx * ny * 8, flo_off)
            wanted = occ_out == "all" or (callable(occ_out) and occ_out(qi, t))
            o, ho = d.out(nx * ny, occ_off) if wanted else (None, None)
            pa.append(p); po.append(o); hs.append((h, ho))
        acc.append(pa); occ_acc.append(po); handles.append(hs)
    sync()
    ctx.flow_accumulate_dev(step, acc, nx, ny, d_occ_step=occ_step, d_occ_acc=None if occ_out is None else occ_acc)
    ctx.synchronize()
    return [[(d.get(h, np.float32, (ny, nx, 2)), None if ho is None else d.get(ho, np.uint8, (ny, nx))) for h, ho in hs] for hs in handles]


NAMES = ("37x29", "67x5", "131x3", "3x5", "2x2", "130x70", R.JUMP)


@pytest.mark.parametrize("n_steps", [1, 2, 5])
@pytest.mark.parametrize("n_seq", [1, 3, 17])
def test_accumulate_is_the_restatement(gpu64, orc, n_seq, n_steps):
    # sequences of one launch share a shape: 17 sequences of 37x29 rotate the steps of the case, with and without maps
    name = "37x29" if n_seq == 17 else ("130x70" if n_seq == 3 else R.JUMP)
    steps, smaps = R.steps(name), R.step_maps(orc, name)
    seqs = [[steps[(q + t) % 5] for t in range(n_steps)] for q in range(n_seq)]
    maps = [[smaps[(q + t) % 5] if q % 2 == 0 else None for t in range(n_steps)] for q in range(n_seq)]
    want = [R.accumulate(seqs[q], None if q % 2 else maps[q]) for q in range(n_seq)]
    for kw in (dict(), dict(flo_off=8, occ_off=3), dict(occ_out=None), dict(occ_out=lambda q, t: (q + t) % 2 == 0, occ_off=1)):
        got = run_accumulate(gpu64, seqs, maps, **kw)
        for q in range(n_seq):
            for t in range(n_steps):
                assert same(got[q][t], want[q][t]), (kw, q, t)
    got = run_accumulate(gpu64, seqs, None)                              # no step maps at all
    for q in range(n_seq):
        plain = R.accumulate(seqs[q])
        for t in range(n_steps):
            assert same(got[q][t], plain[t]), (q, t)


@pytest.mark.parametrize("name", NAMES)
def test_accumulate_equals_chained_compose_calls(gpu64, orc, name):
    steps, maps = R.steps(name), R.step_maps(orc, name)
    got = run_accumulate(gpu64, [steps], [maps])[0]
    ab, occ = None, None
    for t in range(5):
        ab, occ = run_compose(gpu64, [(ab, occ, steps[t], maps[t])])[0]
        assert same(got[t], (ab, occ)), t
        assert same(got[t], R.want(orc, name, 5, True)[t]), t
    # every acc[q][t] the same buffer: only the last payload is kept
    last = run_accumulate(gpu64, [steps], [maps], inplace=True)[0]
    assert last[4][0].tobytes() == got[4][0].tobytes() and last[4][1].tobytes() == got[4][1].tobytes()


def test_f64_and_f32_contexts_write_the_same_bytes_and_host_buffers_are_staged(gpu64, gpu32, orc):
    name = "67x5"
    nx, ny = R.CASES[name][:2]
    steps, maps = R.steps(name), R.step_maps(orc, name)
    want = R.want(orc, name, 5, True)
    a, b = run_accumulate(gpu64, [steps], [maps])[0], run_accumulate(gpu32, [steps], [maps])[0]
    for t in range(5):
        assert same(a[t], want[t]) and same(b[t], want[t]), t
    p0 = R.query_points(nx, ny, 64)
    assert run_tracks(gpu32, [steps], [maps], [p0])[0][0].tobytes() == run_tracks(gpu64, [steps], [maps], [p0])[0][0].tobytes()
    # host memory in, host memory out (the front-end's route): compose in place, accumulate, tracks
    hs = [np.ascontiguousarray(s) for s in steps]
    hm = [np.ascontiguousarray(m) for m in maps]
    acc = np.full((5, ny * nx * 2 + 4), -7.0, dtype=np.float32)
    occ = np.full((5, ny * nx + 4), 9, dtype=np.uint8)
    gpu64.flow_accumulate_dev([[s.ctypes.data for s in hs]], [[acc[t].ctypes.data for t in range(5)]], nx, ny,
                              d_occ_step=[[m.ctypes.data for m in hm]], d_occ_acc=[[occ[t].ctypes.data for t in range(5)]])
    gpu64.synchronize()
    for t in range(5):
        assert acc[t][:ny * nx * 2].tobytes() == want[t][0].tobytes() and (acc[t][ny * nx * 2:] == -7.0).all(), t
        assert occ[t][:ny * nx].tobytes() == want[t][1].tobytes() and (occ[t][ny * nx:] == 9).all(), t
    ab, om = np.array(want[1][0]), np.array(want[1][1])
    gpu64.flow_compose_dev([hs[2].ctypes.data], [ab.ctypes.data], nx, ny, d_flo_ab=[ab.ctypes.data], d_occ_ab=[om.ctypes.data],
                           d_occ_bc=[hm[2].ctypes.data], d_occ_ac=[om.ctypes.data])
    gpu64.synchronize()
    assert ab.tobytes() == want[2][0].tobytes() and om.tobytes() == want[2][1].tobytes()
    xy = np.full((6 * 64 * 2 + 2,), -7.0)
    ln = np.full((64 + 2,), -9, dtype=np.int32)
    gpu64.flow_tracks_dev([[s.ctypes.data for s in hs]], 64, [p0.ctypes.data], [xy.ctypes.data], [ln.ctypes.data], nx, ny,
                          d_occ_step=[[m.ctypes.data for m in hm]])
    gpu64.synchronize()
    wxy, wl = R.tracks(steps, p0, maps)
    assert xy[:6 * 64 * 2].tobytes() == wxy.tobytes() and (xy[6 * 64 * 2:] == -7.0).all()
    assert np.array_equal(ln[:64], wl) and (ln[64:] == -9).all()


def run_tracks(ctx, seqs, maps, pts, xy_off=0):
    """seqs: [sequence][step] payloads; maps: None or the same shape; pts: [sequence] (n_pts, 2) float64 -> [(xy, len)]"""
    ny, nx, _ = seqs[0][0].shape
    n_steps, n_pts = len(seqs[0]), pts[0].shape[0]
    d = Dev()
    step = [[d.put(s, 8) for s in q] for q in seqs]
    occ_step = None if maps is None else [[d.put(m, 3) for m in q] for q in maps]
    xy0 = [d.put(p, xy_off) for p in pts]
    outs = [(d.out((n_steps + 1) * n_pts * 16, xy_off), d.out(n_pts * 4, 4)) for _ in seqs]
    sync()
    ctx.flow_tracks_dev(step, n_pts, xy0, [o[0][0] for o in outs], [o[1][0] for o in outs], nx, ny, d_occ_step=occ_step)
    ctx.synchronize()
    return [(d.get(o[0][1], np.float64, (n_steps + 1, n_pts, 2)), d.get(o[1][1], np.int32, (n_pts,))) for o in outs]


@pytest.mark.parametrize("n_pts", [1, 64, 1000])
@pytest.mark.parametrize("name", ["2x2", "131x3", "37x29", R.JUMP])
def test_tracks_are_the_restatement(gpu64, orc, name, n_pts):
    nx, ny = R.CASES[name][:2]
    steps = R.nonfinite_steps() if name == "37x29" else R.steps(name)
    maps = R.step_maps(orc, name)
    pts = [R.query_points(nx, ny, n_pts, seed) for seed in (5, 6, 7)]
    if n_pts == 1:
        pts[1][0] = (-1.0, 0.0)                                          # a lone point that starts outside
    for n_steps in (1, 2, 5):
        seqs = [steps[:n_steps], steps[5 - n_steps:], steps[:n_steps]]
        for with_maps in (False, True):
            ms = [maps[:n_steps], [None] * n_steps, maps[:n_steps]] if with_maps else None
            got = run_tracks(gpu64, seqs, ms, pts, xy_off=8 if with_maps else 0)
            for q in range(3):
                wxy, wl = R.tracks(seqs[q], pts[q], ms[q] if with_maps else None)
                assert got[q][0].tobytes() == wxy.tobytes() and np.array_equal(got[q][1], wl), (n_steps, with_maps, q)
    if n_pts >= 64 and ny >= 29:                                        # (in a frame of 2 or 3 rows nothing survives five steps)
        wl = R.tracks(steps, pts[0], maps)[1]
        assert (wl == -1).any() and (wl == 5).any() and ((wl >= 0) & (wl < 5)).any()       # outside, survivors, lost mid-way


def test_tracks_17_sequences_and_pixel_grid_starts_follow_the_dense_chain(gpu64, orc):
    name = "37x29"
    nx, ny = R.CASES[name][:2]
    steps, maps = R.steps(name), R.step_maps(orc, name)
    seqs = [[steps[(q + t) % 5] for t in range(2)] for q in range(17)]
    ms = [[maps[(q + t) % 5] for t in range(2)] for q in range(17)]
    pts = [R.query_points(nx, ny, 64, 100 + q) for q in range(17)]
    got = run_tracks(gpu64, seqs, ms, pts)
    for q in range(17):
        wxy, wl = R.tracks(seqs[q], pts[q], ms[q])
        assert got[q][0].tobytes() == wxy.tobytes() and np.array_equal(got[q][1], wl), q
    # the first step of a track from a pixel is the dense chain's first step, exactly: both are the step's own vector
    i, j = R._grid(ny, nx)
    grid = np.stack([j.ravel(), i.ravel()], axis=-1)
    xy, ln = run_tracks(gpu64, [steps[:1]], [maps[:1]], [grid])[0]
    ac, occ = run_accumulate(gpu64, [steps[:1]], [maps[:1]])[0][0]
    ok = (occ == 0).ravel()
    assert np.array_equal(ln == 1, ok)
    assert np.array_equal(xy[1][ok], (grid + ac.reshape(-1, 2).astype(np.float64))[ok])


def test_refusals_are_invalid_arguments_and_write_nothing(gpu64, orc):
    import ctypes as C
    import torch
    nx, ny, n_pts = 9, 7, 5
    n = nx * ny
    rng = np.random.default_rng(3)
    src = torch.from_numpy(rng.normal(0.0, 1.0, (3, n * 2 + 2)).astype(np.float32)).cuda()
    dst = torch.full((3, n * 2 + 2), -7.0, dtype=torch.float32, device="cuda")
    omap = torch.full((n + 8,), 9, dtype=torch.uint8, device="cuda")
    xy0 = torch.from_numpy(rng.uniform(0.0, 6.0, (n_pts * 2 + 1,))).cuda()
    xy = torch.full((3 * n_pts * 2 + 1,), -7.0, dtype=torch.float64, device="cuda")
    ln = torch.full((n_pts + 1,), -9, dtype=torch.int32, device="cuda")
    sync()
    s = [src[k].data_ptr() for k in range(3)]
    d = [dst[k].data_ptr() for k in range(3)]
    o, x0, x, l = omap.data_ptr(), xy0.data_ptr(), xy.data_ptr(), ln.data_ptr()
    vp = C.c_void_p
    L, h = gpu64.L, gpu64.h
    tab = lambda *xs: (vp * len(xs))(*xs)

    def refused(status, word):
        assert status == ERR_ARG, word
        assert word in L.ofx_last_error(h).decode(), (word, L.ofx_last_error(h))

    def compose(n_, ab, bc, ac, nx_=nx, ny_=ny, occ_bc=None, occ_ac=None):
        return L.ofx_flow_compose_dev(h, n_, ab, None, bc, occ_bc, ac, occ_ac, nx_, ny_)

    refused(compose(1, None, None, tab(d[0])), "NULL")
    refused(compose(1, None, tab(s[0]), None), "NULL")
    refused(compose(1, None, tab(None), tab(d[0])), "NULL")
    refused(compose(2, None, tab(s[0], s[1]), tab(d[0], None)), "slot 1")
    refused(compose(0, None, tab(s[0]), tab(d[0])), "n = 0")
    refused(compose(-1, None, tab(s[0]), tab(d[0])), "n = -1")
    refused(compose(1, None, tab(s[0]), tab(d[0]), nx_=1), "too small")
    refused(compose(1, None, tab(s[0]), tab(d[0]), ny_=1), "too small")
    refused(compose(1, None, tab(s[0]), tab(d[0]), nx_=65536, ny_=65536), "int")
    refused(compose(1, None, tab(s[0] + 4), tab(d[0])), "8-byte")
    refused(compose(1, None, tab(s[0]), tab(d[0] + 4)), "8-byte")
    refused(compose(1, tab(s[1] + 4), tab(s[0]), tab(d[0])), "8-byte")
    refused(compose(1, None, tab(d[0]), tab(d[0])), "step")
    refused(compose(2, None, tab(s[0], d[1]), tab(d[0], d[1])), "slot 1")
    refused(compose(1, None, tab(s[0]), tab(d[0]), occ_bc=tab(o), occ_ac=tab(o)), "step")

    def accumulate(n_seq, n_steps, step, acc, nx_=nx, ny_=ny):
        return L.ofx_flow_accumulate_dev(h, n_seq, n_steps, step, None, acc, None, nx_, ny_)

    refused(accumulate(1, 2, None, tab(d[0], d[1])), "NULL")
    refused(accumulate(1, 2, tab(s[0], s[1]), None), "NULL")
    refused(accumulate(1, 2, tab(s[0], None), tab(d[0], d[1])), "step 1")
    refused(accumulate(1, 2, tab(s[0], s[1]), tab(d[0], None)), "step 1")
    refused(accumulate(0, 2, tab(s[0], s[1]), tab(d[0], d[1])), "n_seq = 0")
    refused(accumulate(1, 0, tab(s[0], s[1]), tab(d[0], d[1])), "n_steps = 0")
    refused(accumulate(1, 2, tab(s[0], s[1]), tab(d[0], d[1]), nx_=1), "too small")
    refused(accumulate(1, 2, tab(s[0], s[1]), tab(d[0], d[1]), nx_=65536, ny_=65536), "int")
    refused(accumulate(1, 2, tab(s[0], s[1] + 4), tab(d[0], d[1])), "8-byte")
    refused(accumulate(1, 2, tab(s[0], s[1]), tab(d[0] + 4, d[1])), "8-byte")
    refused(accumulate(1, 2, tab(s[0], d[1]), tab(d[0], d[1])), "still reads")
    refused(accumulate(1, 2, tab(s[0], d[0]), tab(d[0], d[1])), "still reads")           # step 1 would be overwritten by step 0

    def tracks(n_seq, n_steps, step, n_pts_, txy0, txy, tlen, nx_=nx, ny_=ny):
        return L.ofx_flow_tracks_dev(h, n_seq, n_steps, step, None, n_pts_, txy0, txy, tlen, nx_, ny_)

    refused(tracks(1, 2, None, n_pts, tab(x0), tab(x), tab(l)), "NULL")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, None, tab(x), tab(l)), "NULL")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, tab(x0), None, tab(l)), "NULL")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, tab(x0), tab(x), None), "NULL")
    refused(tracks(1, 2, tab(s[0], None), n_pts, tab(x0), tab(x), tab(l)), "step 1")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, tab(None), tab(x), tab(l)), "sequence 0")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, tab(x0), tab(x), tab(None)), "sequence 0")
    refused(tracks(0, 2, tab(s[0], s[1]), n_pts, tab(x0), tab(x), tab(l)), "n_seq = 0")
    refused(tracks(1, 0, tab(s[0], s[1]), n_pts, tab(x0), tab(x), tab(l)), "n_steps = 0")
    refused(tracks(1, 2, tab(s[0], s[1]), 0, tab(x0), tab(x), tab(l)), "n_pts = 0")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, tab(x0), tab(x), tab(l), ny_=1), "too small")
    refused(tracks(1, 2, tab(s[0] + 4, s[1]), n_pts, tab(x0), tab(x), tab(l)), "8-byte")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, tab(x0 + 4), tab(x), tab(l)), "8-byte")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, tab(x0), tab(x + 4), tab(l)), "8-byte")
    refused(tracks(1, 2, tab(s[0], s[1]), n_pts, tab(x0), tab(x), tab(l + 2)), "4-byte")
    gpu64.synchronize()
    assert (dst.cpu().numpy() == -7.0).all() and (omap.cpu().numpy() == 9).all()
    assert (xy.cpu().numpy() == -7.0).all() and (ln.cpu().numpy() == -9).all()
    # NULL optional tables and NULL entries in them are fine
    assert L.ofx_flow_compose_dev(h, 1, tab(None), tab(None), tab(s[0]), tab(None), tab(d[0]), tab(None), nx, ny) == 0
    gpu64.synchronize()
    bc = src[0].cpu().numpy()[:n * 2].reshape(ny, nx, 2)
    assert dst[0].cpu().numpy()[:n * 2].tobytes() == R.compose(None, bc)[0].tobytes() and (dst[0].cpu().numpy()[n * 2:] == -7.0).all()
