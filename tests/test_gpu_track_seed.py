"""ofx_track_structure_dev, ofx_track_seed_dev and ofx_track_sequence_dev against the numpy restatement (tests/track_seed_ref.py):
lam2 and its mean bit for bit -- at 7x9 (the smallest that rho = 1 allows), 67x13, 131x37 and 130x70 (several tiles both ways, widths
that are no multiple of 64, fewer rows than a tile), rho 0.5, 1 and 2, all five "input" kinds, pitched rows, 1, 3 and 17 slots;
seeds and their counts in cell order for step 1, 3, 4 and 8; whole sequences table by table; guard bytes around every destination;
both storage precisions; host buffers; every refusal."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import flow_compose_ref as fcr
import track_seed_ref as R
from test_gpu_flow_compose import FILL, Dev, sync

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_SIGMA = 1, 2
IN_OPTION = {"f64": 0, "u8": 1, "u16": 2, "f32": 3, "rgb8": 4}
ALIGN = {"f64": 8, "u8": 1, "u16": 2, "f32": 4, "rgb8": 1}
SHAPES = [(7, 9), (67, 13), (131, 37), (130, 70)]


@contextlib.contextmanager
def options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, 0)


def pitched(arr, pitch):
    """the frame's rows `pitch` bytes apart, the bytes between them 0xEE"""
    rows = np.ascontiguousarray(arr).reshape(arr.shape[0], -1).view(np.uint8)
    out = np.full((arr.shape[0], pitch), 0xEE, dtype=np.uint8)
    out[:, :rows.shape[1]] = rows
    return out.reshape(-1)[:(arr.shape[0] - 1) * pitch + rows.shape[1]]


def run_structure(ctx, ups, nx, ny, rho, want_lam2=None, want_mean=None):
    """ups: the frames as uploaded -> [(lam2 | None, mean | None)]"""
    n = len(ups)
    want_lam2 = [True] * n if want_lam2 is None else want_lam2
    want_mean = [True] * n if want_mean is None else want_mean
    d = Dev()
    src = [d.put(u) for u in ups]
    lam = [d.out(nx * ny * 8) if w else (None, None) for w in want_lam2]
    mean = [d.out(8) if w else (None, None) for w in want_mean]
    sync()
    ctx.track_structure_dev(src, nx, ny, rho, d_lam2=[p for p, _ in lam] if any(want_lam2) else None,
                            d_mean=[p for p, _ in mean] if any(want_mean) else None)
    ctx.synchronize()
    return [(None if h is None else d.get(h, np.float64, (ny, nx)), None if m is None else d.get(m, np.float64, (1,))[0])
            for (_, h), (_, m) in zip(lam, mean)]


def same_structure(got, want):
    l2, mean = want
    return (got[0] is None or got[0].tobytes() == l2.tobytes()) and (got[1] is None or np.float64(got[1]).tobytes() == np.float64(mean).tobytes())


@pytest.mark.parametrize("rho", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_lam2_and_mean_are_the_restatement(gpu64, orc, shape, rho):
    nx, ny = shape
    size = int(5 * rho) + 1
    if size >= nx or size >= ny:                                         # 7x9 at rho = 2: the refusal of the Gaussian
        d = Dev()
        p = d.put(R.kind_frame(nx, ny, "f64")[0])
        out, h = d.out(nx * ny * 8)
        sync()
        tab = lambda *xs: (C.c_void_p * len(xs))(*xs)
        assert gpu64.L.ofx_track_structure_dev(gpu64.h, 1, tab(p), tab(out), None, nx, ny, rho) == ERR_SIGMA
        gpu64.synchronize()
        assert (d.get(h, np.uint8, (nx * ny * 8,)) == FILL).all()
        return
    frames = [R.kind_frame(nx, ny, "f64", seed) for seed in (0, 1, 2)]
    got = run_structure(gpu64, [f[0] for f in frames], nx, ny, rho)
    for g, f in enumerate(frames):
        want = R.structure(orc, f[1], rho)
        assert np.isfinite(want[1]) and want[1] > 0.0
        assert same_structure(got[g], want), (g, float(np.abs(got[g][0] - want[0]).max()), got[g][1], want[1])


@pytest.mark.parametrize("kind", ["f64", "f32", "u8", "u16", "rgb8"])
def test_every_input_kind_dense_and_pitched(gpu64, gpu32, orc, kind):
    for nx, ny in ((67, 13), (131, 37)):
        up, vals = R.kind_frame(nx, ny, kind)
        want = R.structure(orc, vals, 1.0)
        row = up.reshape(ny, -1).view(np.uint8).shape[1]
        ctxs = [(gpu64, IN_OPTION[kind])] + ([(gpu32, 0)] if kind == "f32" else [(gpu32, IN_OPTION[kind])] if kind == "u8" else [])
        for ctx, inp in ctxs:
            with options(ctx, input=inp):
                assert same_structure(run_structure(ctx, [up], nx, ny, 1.0)[0], want), (nx, ny, "dense")
            for pitch in (row + ALIGN[kind], ((row + 255) // 256) * 256):
                with options(ctx, input=inp, input_pitch=pitch):
                    assert same_structure(run_structure(ctx, [pitched(up, pitch)], nx, ny, 1.0)[0], want), (nx, ny, pitch)


@pytest.mark.parametrize("n", [1, 3, 17])
def test_any_number_of_slots_and_null_destinations(gpu64, orc, n):
    nx, ny = 67, 13
    frames = [R.kind_frame(nx, ny, "f64", g % 4) for g in range(n)]
    want = [R.structure(orc, f[1], 1.0) for f in frames[:4]]
    wl = [g % 3 != 1 for g in range(n)]
    wm = [g % 3 != 2 for g in range(n)] if n > 1 else [True]
    got = run_structure(gpu64, [f[0] for f in frames], nx, ny, 1.0, wl, wm)
    for g in range(n):
        assert (got[g][0] is not None) == wl[g] and (got[g][1] is not None) == wm[g]
        assert same_structure(got[g], want[g % 4]), g
    if n == 1:                                                           # a NULL table for each
        assert same_structure(run_structure(gpu64, [frames[0][0]], nx, ny, 1.0, [False], [True])[0], want[0])
        assert same_structure(run_structure(gpu64, [frames[0][0]], nx, ny, 1.0, [True], [False])[0], want[0])


def test_a_nan_sample_spreads_as_in_the_restatement(gpu64, orc):
    nx, ny = 37, 29
    vals = np.array(R.clip(nx, ny)[1][0])
    vals[14, 18] = np.nan
    want = R.structure(orc, vals, 1.0)
    got = run_structure(gpu64, [vals], nx, ny, 1.0)[0]
    assert np.array_equal(np.isnan(got[0]), np.isnan(want[0])) and np.isnan(got[1])
    ok = ~np.isnan(want[0])
    assert got[0][ok].tobytes() == want[0][ok].tobytes()


def run_seeds(ctx, ups, nx, ny, cap, frac, step, occ=None, rho=R.RHO):
    """-> [(xy (cap, 2) as the buffer holds it, count (2,))]"""
    d = Dev()
    src = [d.put(u) for u in ups]
    pts = None if occ is None else [d.put(o) for o in occ]
    n_occ = 0 if occ is None else max(len(o) for o in occ if o is not None)
    outs = [(d.out(cap * 16), d.out(8)) for _ in ups]
    sync()
    ctx.track_seed_dev(src, [o[0][0] for o in outs], [o[1][0] for o in outs], cap, nx, ny, rho, frac, step, d_xy_occ=pts, n_occ=n_occ)
    ctx.synchronize()
    return [(d.get(o[0][1], np.uint8, (cap * 16,)), d.get(o[1][1], np.int32, (2,))) for o in outs]


def same_seeds(got, want, cap):
    xy, written, dropped = want
    raw, count = got
    return (tuple(count) == (written, dropped) and raw[:written * 16].tobytes() == xy.tobytes() and (raw[written * 16:] == FILL).all())


@pytest.mark.parametrize("step", [1, 3, 4, 8])
@pytest.mark.parametrize("name", ["37x29", "130x70"])
def test_seeds_are_the_restatement_in_cell_order(gpu64, orc, name, step):
    nx, ny = fcr.CASES[name][:2]
    up, vals = R.clip(nx, ny)
    frac = R.pick_frac(orc, vals)
    st = [R.structure(orc, vals[f], R.RHO) for f in range(3)]
    full = [R.seeds(l2, mean, frac, step) for l2, mean in st]
    n0 = full[0][1]
    assert n0 > 4
    pts = np.concatenate([full[0][0][1::3], [[np.nan, 2.0], [1.0, np.inf], [-0.5, 3.0], [nx - 0.5, 1.0], [nx - 1.0, ny - 1.0], [0.25, 0.75]]])
    with options(gpu64, input=1):
        for cap in (n0 - 3, n0, n0 + 5):
            got = run_seeds(gpu64, [up[f] for f in range(3)], nx, ny, cap, frac, step)
            for f in range(3):
                assert same_seeds(got[f], R.seeds(st[f][0], st[f][1], frac, step, cap=cap), cap), (cap, f, got[f][1])
        cap = n0
        occ = [pts, None, pts[::-1].copy()]
        got = run_seeds(gpu64, [up[0]] * 3, nx, ny, cap, frac, step, occ=occ)
        again = run_seeds(gpu64, [up[0]] * 3, nx, ny, cap, frac, step, occ=occ)
        for g in range(3):
            want = R.seeds(st[0][0], st[0][1], frac, step, occ_points=occ[g], cap=cap)
            assert same_seeds(got[g], want, cap), (g, got[g][1], want[1:])
            assert got[g][0].tobytes() == again[g][0].tobytes() and got[g][1].tobytes() == again[g][1].tobytes()
        assert got[0][1][0] < got[1][1][0] and got[0][0].tobytes() == got[2][0].tobytes()


def run_sequence(ctx, clips, steps, maps, cap, nx, ny, frac, step=R.STEP, rho=R.RHO):
    """clips: [clip][frame] arrays as uploaded; steps: [clip][step]; maps: None or [clip][step] with None entries
    -> [(xy (n_frames, cap, 2) raw uint8, t0 raw, len raw, count)]"""
    n_frames = len(clips[0])
    d = Dev()
    memo = {}

    def put(a):
        if a is None:
            return None
        if id(a) not in memo:
            memo[id(a)] = d.put(a)
        return memo[id(a)]

    dF = [[put(f) for f in q] for q in clips]
    dS = [[put(s) for s in q] for q in steps]
    dM = None if maps is None else [[put(m) for m in q] for q in maps]
    outs = [(d.out(n_frames * cap * 16), d.out(cap * 4), d.out(cap * 4), d.out(8)) for _ in clips]
    sync()
    ctx.track_sequence_dev(dF, dS, cap, *[[o[k][0] for o in outs] for k in range(4)], nx, ny, rho, frac, step, d_occ_step=dM)
    ctx.synchronize()
    return [(d.get(o[0][1], np.uint8, (n_frames, cap, 16)), d.get(o[1][1], np.uint8, (cap, 4)), d.get(o[2][1], np.uint8, (cap, 4)),
             d.get(o[3][1], np.int32, (2,))) for o in outs]


def decode(got):
    """the used slots of a raw result as the restatement's dict (without `structure`)"""
    xy, t0, ln, count = got
    used = int(count[0])
    n_frames = xy.shape[0]
    return dict(xy=np.frombuffer(np.ascontiguousarray(xy[:, :used]).tobytes(), dtype=np.float64).reshape(n_frames, used, 2),
                t0=np.frombuffer(t0[:used].tobytes(), dtype=np.int32), len=np.frombuffer(ln[:used].tobytes(), dtype=np.int32),
                count=(used, int(count[1])))


def same_sequence(got, want):
    xy, t0, ln, count = got
    used = want["count"][0]
    return (tuple(count) == tuple(want["count"]) and np.ascontiguousarray(xy[:, :used]).tobytes() == want["xy"].tobytes()
            and t0[:used].tobytes() == want["t0"].tobytes() and ln[:used].tobytes() == want["len"].tobytes()
            and (xy[:, used:] == FILL).all() and (t0[used:] == FILL).all() and (ln[used:] == FILL).all())


CAPS = {"37x29": 40, "130x70": 600}                    # 37x29: seeds of the later frames are dropped; 130x70: room for all


@pytest.mark.parametrize("n_frames", [2, 3, 5])
@pytest.mark.parametrize("name", ["37x29", "130x70"])
def test_sequences_are_the_restatement_table_by_table(gpu64, gpu32, orc, name, n_frames):
    nx, ny = fcr.CASES[name][:2]
    cap = CAPS[name]
    up = R.clip(nx, ny)[0]
    steps, maps = fcr.steps(name, n_frames - 1), fcr.step_maps(orc, name, n_frames - 1)
    want_m, frac = R.want_sequence(orc, name, n_frames, True, cap)
    want_0, _ = R.want_sequence(orc, name, n_frames, False, cap)
    frames = [up[f] for f in range(n_frames)]
    with options(gpu64, input=1):
        got = run_sequence(gpu64, [frames] * 3, [steps] * 3, [maps, [None] * (n_frames - 1), maps], cap, nx, ny, frac)
        assert same_sequence(got[0], want_m) and same_sequence(got[1], want_0) and same_sequence(got[2], want_m), [g[3] for g in got]
        none = run_sequence(gpu64, [frames], [steps], None, cap, nx, ny, frac)[0]                      # no table of maps at all
        assert same_sequence(none, want_0)
    # the same bytes from the f32 context
    with options(gpu32, input=1):
        got32 = run_sequence(gpu32, [frames], [steps], [maps], cap, nx, ny, frac)[0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got32, got[0]))
    # the density invariant on the device result
    res = dict(decode(got[0]), structure=want_m["structure"])
    assert R.density_holes(res, frac, R.STEP, nx, ny, cap) == []
    if n_frames == 5:
        assert (res["t0"] > 0).any() and len(want_m["lost_map"]) > 0 and len(want_0["lost_leave"]) > 0
        if name == "37x29":
            assert want_m["count"][1] > 0 and want_m["count"][0] == cap


@pytest.mark.parametrize("name", ["37x29", "130x70"])
def test_slots_born_at_frame_0_are_flow_tracks_on_its_seeds(gpu64, orc, name):
    from test_gpu_flow_compose import run_tracks
    nx, ny = fcr.CASES[name][:2]
    cap = CAPS[name]
    up = R.clip(nx, ny)[0]
    steps, maps = fcr.steps(name, 4), fcr.step_maps(orc, name, 4)
    frac = R.pick_frac(orc, R.clip(nx, ny)[1])
    with options(gpu64, input=1):
        res = decode(run_sequence(gpu64, [list(up)], [steps], [maps], cap, nx, ny, frac)[0])
    born0 = res["t0"] == 0
    assert born0.sum() > 10
    xy, ln = run_tracks(gpu64, [steps], [maps], [np.ascontiguousarray(res["xy"][0][born0])])[0]
    assert xy.tobytes() == np.ascontiguousarray(res["xy"][:, born0]).tobytes() and np.array_equal(ln, res["len"][born0])


@pytest.mark.parametrize("n_seq", [1, 3, 17])
def test_any_number_of_clips_16_per_launch(gpu64, orc, n_seq):
    name, n_frames, cap = "37x29", 3, 40
    nx, ny = fcr.CASES[name][:2]
    up, vals = R.clip(nx, ny)
    frac = R.pick_frac(orc, vals)
    steps, maps = fcr.steps(name), fcr.step_maps(orc, name)
    # clip q: the frames from q % 3 on, the steps from q % 4 on, maps for the even clips
    pick = lambda q: (q % 3, q % 4, q % 2 == 0)
    want = {}
    for q in range(n_seq):
        f0, s0, m = pick(q)
        if pick(q) not in want:
            want[pick(q)] = R.sequence(orc, list(vals[f0:f0 + n_frames]), steps[s0:s0 + 2], maps[s0:s0 + 2] if m else None, cap, R.RHO,
                                       frac, R.STEP)
    clips = [[up[pick(q)[0] + f] for f in range(n_frames)] for q in range(n_seq)]
    st = [steps[pick(q)[1]:pick(q)[1] + 2] for q in range(n_seq)]
    ms = [maps[pick(q)[1]:pick(q)[1] + 2] if pick(q)[2] else [None, None] for q in range(n_seq)]
    with options(gpu64, input=1):
        got = run_sequence(gpu64, clips, st, ms, cap, nx, ny, frac)
    for q in range(n_seq):
        assert same_sequence(got[q], want[pick(q)]), (q, got[q][3], want[pick(q)]["count"])


def test_host_buffers(gpu64, orc):
    name, n_frames, cap = "37x29", 3, 40
    nx, ny = fcr.CASES[name][:2]
    up = R.clip(nx, ny)[0]
    want, frac = R.want_sequence(orc, name, n_frames, True, cap)
    frames = [np.array(up[f]) for f in range(n_frames)]
    steps = [np.array(s) for s in fcr.steps(name, n_frames - 1)]
    maps = [np.array(m) for m in fcr.step_maps(orc, name, n_frames - 1)]
    xy = np.full((n_frames * cap * 2 + 2,), -7.0)
    t0, ln = np.full((cap + 1,), -9, dtype=np.int32), np.full((cap + 1,), -9, dtype=np.int32)
    count = np.full((3,), -9, dtype=np.int32)
    ptr = lambda a: a.ctypes.data
    with options(gpu64, input=1):
        gpu64.track_sequence_dev([[ptr(f) for f in frames]], [[ptr(s) for s in steps]], cap, [ptr(xy)], [ptr(t0)], [ptr(ln)], [ptr(count)],
                                 nx, ny, R.RHO, frac, R.STEP, d_occ_step=[[ptr(m) for m in maps]])
        gpu64.synchronize()
        used = want["count"][0]
        assert tuple(count[:2]) == tuple(want["count"]) and count[2] == -9
        got = xy[:n_frames * cap * 2].reshape(n_frames, cap, 2)
        assert np.ascontiguousarray(got[:, :used]).tobytes() == want["xy"].tobytes() and (got[:, used:] == -7.0).all() and (xy[-2:] == -7.0).all()
        assert np.array_equal(t0[:used], want["t0"]) and (t0[used:] == -9).all()
        assert np.array_equal(ln[:used], want["len"]) and (ln[used:] == -9).all()
        # the seed entry and the structure entry
        l2, mean = want["structure"][0]
        sxy, scount = np.full((cap * 2 + 2,), -7.0), np.full((3,), -9, dtype=np.int32)
        gpu64.track_seed_dev([ptr(frames[0])], [ptr(sxy)], [ptr(scount)], cap, nx, ny, R.RHO, frac, R.STEP)
        hl, hm = np.full((nx * ny + 1,), -7.0), np.full((2,), -7.0)
        gpu64.track_structure_dev([ptr(frames[0])], nx, ny, R.RHO, d_lam2=[ptr(hl)], d_mean=[ptr(hm)])
        gpu64.synchronize()
    w = R.seeds(l2, mean, frac, R.STEP, cap=cap)
    assert tuple(scount[:2]) == w[1:] and sxy[:w[1] * 2].tobytes() == w[0].tobytes() and (sxy[w[1] * 2:] == -7.0).all()
    assert hl[:nx * ny].tobytes() == l2.tobytes() and hl[-1] == -7.0 and hm[0] == mean and hm[1] == -7.0


def test_refusals_are_returned_and_write_nothing(gpu64, orc):
    import torch
    nx, ny, cap = 9, 8, 6
    n = nx * ny
    rng = np.random.default_rng(3)
    fr = torch.from_numpy(rng.uniform(0.0, 255.0, (3, n + 1))).cuda()
    flo = torch.from_numpy(rng.normal(0.0, 1.0, (2, n * 2 + 2)).astype(np.float32)).cuda()
    pts = torch.from_numpy(rng.uniform(0.0, 6.0, (5,))).cuda()
    lam = torch.full((n + 1,), -7.0, dtype=torch.float64, device="cuda")
    mean = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    xy = torch.full((3 * cap * 2 + 1,), -7.0, dtype=torch.float64, device="cuda")
    t0 = torch.full((cap + 1,), -9, dtype=torch.int32, device="cuda")
    ln = torch.full((cap + 1,), -9, dtype=torch.int32, device="cuda")
    cnt = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    sync()
    f = [fr[k].data_ptr() for k in range(3)]
    s = [flo[k].data_ptr() for k in range(2)]
    p, l, m, x, a, b, c = (t.data_ptr() for t in (pts, lam, mean, xy, t0, ln, cnt))
    L, h = gpu64.L, gpu64.h
    tab = lambda *xs: (C.c_void_p * len(xs))(*xs)

    def refused(status, word, want=ERR_ARG):
        assert status == want, (word, status)
        assert word in L.ofx_last_error(h).decode(), (word, L.ofx_last_error(h))

    def structure(n_=1, dF=tab(f[0]), dl=tab(l), dm=tab(m), nx_=nx, ny_=ny, rho=1.0):
        return L.ofx_track_structure_dev(h, n_, dF, dl, dm, nx_, ny_, rho)

    refused(structure(dF=None), "NULL")
    refused(structure(dF=tab(None)), "slot 0")
    refused(structure(n_=0), "n = 0")
    refused(structure(nx_=1), "too small")
    refused(structure(ny_=1), "too small")
    refused(structure(nx_=65536, ny_=65536), "int")
    for rho in (0.0, -1.0, float("nan"), float("inf")):
        refused(structure(rho=rho), "rho")
    refused(structure(rho=2.2), "OFX_TRACK_MAX_SIZE")
    refused(structure(rho=1e300), "OFX_TRACK_MAX_SIZE")
    refused(structure(rho=1.6), "sigma too large", ERR_SIGMA)          # 9 taps against 9 columns
    refused(structure(rho=1.4), "sigma too large", ERR_SIGMA)          # 8 taps against 8 rows
    refused(structure(dF=tab(f[0] + 4)), "aligned")
    refused(structure(dl=tab(l + 4)), "8-byte")
    refused(structure(dm=tab(m + 4)), "8-byte")
    refused(structure(dl=tab(f[0])), "reads")
    refused(structure(n_=2, dF=tab(f[0], f[1]), dl=tab(l, f[0]), dm=None), "slot 1")
    refused(structure(dl=tab(l), dm=tab(l)), "other destination")
    with options(gpu64, input_pitch=nx * 8 - 8):
        refused(structure(), "pitch")
    with options(gpu64, input_pitch=nx * 8 + 4):
        refused(structure(), "pitch")

    def seed(n_=1, dF=tab(f[0]), occ=None, n_occ=0, dxy=tab(x), dc=tab(c), cap_=cap, nx_=nx, ny_=ny, rho=1.0, frac=0.5, step=2):
        return L.ofx_track_seed_dev(h, n_, dF, occ, n_occ, dxy, dc, cap_, nx_, ny_, rho, frac, step)

    refused(seed(dF=None), "NULL")
    refused(seed(dxy=None), "NULL")
    refused(seed(dc=None), "NULL")
    refused(seed(dxy=tab(None)), "slot 0")
    refused(seed(dc=tab(None)), "slot 0")
    refused(seed(n_=0), "n = 0")
    refused(seed(n_occ=-1), "n_occ")
    refused(seed(cap_=0), "cap = 0")
    refused(seed(step=0), "step = 0")
    refused(seed(nx_=1), "too small")
    refused(seed(nx_=65536, ny_=65536), "int")
    refused(seed(rho=0.0), "rho")
    refused(seed(rho=1.6), "sigma too large", ERR_SIGMA)
    for frac in (-0.1, float("nan"), float("inf")):
        refused(seed(frac=frac), "frac")
    refused(seed(dxy=tab(x + 4)), "8-byte")
    refused(seed(occ=tab(p + 4), n_occ=2), "8-byte")
    refused(seed(dc=tab(c + 2)), "4-byte")
    refused(seed(dxy=tab(f[0])), "reads")
    refused(seed(occ=tab(x), n_occ=2), "reads")

    def sequence(n_seq=1, n_frames=3, dF=tab(*f), st=tab(*s), occ=None, cap_=cap, dxy=tab(x), d0=tab(a), dl=tab(b), dc=tab(c), nx_=nx,
                 ny_=ny, rho=1.0, frac=0.5, step=2):
        return L.ofx_track_sequence_dev(h, n_seq, n_frames, dF, st, occ, cap_, dxy, d0, dl, dc, nx_, ny_, rho, frac, step)

    for k in ("dF", "st", "dxy", "d0", "dl", "dc"):
        refused(sequence(**{k: None}), "NULL")
    refused(sequence(dF=tab(f[0], None, f[2])), "frame 1")
    refused(sequence(st=tab(s[0], None)), "step 1")
    for k in ("dxy", "d0", "dl", "dc"):
        refused(sequence(**{k: tab(None)}), "sequence 0")
    refused(sequence(n_seq=0), "n_seq = 0")
    refused(sequence(n_frames=1), "1 frames")
    refused(sequence(cap_=0), "cap = 0")
    refused(sequence(step=0), "step = 0")
    refused(sequence(ny_=1), "too small")
    refused(sequence(nx_=65536, ny_=65536), "int")
    refused(sequence(rho=float("nan")), "rho")
    refused(sequence(rho=1.6), "sigma too large", ERR_SIGMA)
    refused(sequence(frac=-1.0), "frac")
    refused(sequence(dF=tab(f[0], f[1] + 4, f[2])), "frame 1")
    refused(sequence(st=tab(s[0], s[1] + 4)), "8-byte")
    refused(sequence(dxy=tab(x + 4)), "8-byte")
    refused(sequence(d0=tab(a + 2)), "4-byte")
    refused(sequence(dl=tab(b + 2)), "4-byte")
    refused(sequence(dc=tab(c + 2)), "4-byte")
    refused(sequence(dxy=tab(f[2])), "reads")
    refused(sequence(d0=tab(s[1])), "reads")
    refused(sequence(d0=tab(a), dl=tab(a)), "same array")
    gpu64.synchronize()
    assert (lam.cpu().numpy() == -7.0).all() and (mean.cpu().numpy() == -7.0).all() and (xy.cpu().numpy() == -7.0).all()
    assert (t0.cpu().numpy() == -9).all() and (ln.cpu().numpy() == -9).all() and (cnt.cpu().numpy() == -9).all()
    # NULL optional tables and NULL entries in them are fine
    assert L.ofx_track_seed_dev(h, 1, tab(f[0]), tab(None), 2, tab(x), tab(c), cap, nx, ny, 1.0, 0.5, 2) == 0
    assert L.ofx_track_sequence_dev(h, 1, 3, tab(*f), tab(*s), tab(None, None), cap, tab(x), tab(a), tab(b), tab(c), nx, ny, 1.0, 0.5, 2) == 0
    gpu64.synchronize()
    got = cnt.cpu().numpy()
    vals = fr.cpu().numpy()[:, :n].reshape(3, ny, nx)
    sf = [np.frombuffer(flo[k].cpu().numpy()[:n * 2].tobytes(), dtype=np.float32).reshape(ny, nx, 2) for k in range(2)]
    want = R.sequence(orc, list(vals), sf, None, cap, 1.0, 0.5, 2)
    assert tuple(got[:2]) == tuple(want["count"]) and got[2] == -9
