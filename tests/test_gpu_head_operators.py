"""The pyramid-head operators -- joint min / max of a SET of images, 255 (x - min) / (max - min) -- behind every entry that
uses them.  One partial reduction, one final reduction and one map serve all of them (csrc/ofx_ops.hip); what could go wrong is
a source reduced into the wrong set, a tail of a source that is not read, or a chunk of a long sequence that is dropped.  So
every case places its extremes where only a complete reduction of the right set finds them, gives every set (pair, channel,
sequence) a range of its own, and makes one set constant (max - min = 0: a copy) next to sets that are not.

Every comparison is np.array_equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 1 element; around one block of 256 threads; 513 x 512 > 1024 blocks x 256 threads, so the grid-stride loop runs twice
SHAPES = [(1,), (255,), (256,), (257,), (513, 512)]
SENTINEL = -7.0


def _f32(x):
    return x.astype(np.float32).astype(np.float64)


def _set(k, shape, swap, seed=0):
    """k images (float32-representable values) whose joint minimum is the FIRST element of the first image and whose joint
    maximum is the LAST element of the last one -- or the other way round"""
    rng = np.random.default_rng(100 * k + seed)
    imgs = [_f32(rng.uniform(10.0, 200.0, shape)) for _ in range(k)]
    lo, hi = (977.25, -3.5) if swap else (-3.5, 977.25)
    imgs[-1].flat[-1] = hi
    imgs[0].flat[0] = lo             # one image of one element: the set is {lo}, max - min = 0
    return imgs


# ---- operator level ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_operators_f64(gpu64, orc, shape, swap):
    a, = _set(1, shape, swap)
    assert gpu64.getminmax(a) == orc.getminmax(a) == (a.min(), a.max())
    assert np.array_equal(gpu64.image_normalization_1(a), orc.image_normalization_1(a))
    a, b = _set(2, shape, swap)
    for g, o in zip(gpu64.image_normalization_2(a, b), orc.image_normalization_2(a, b)):
        assert np.array_equal(g, o)
    s3 = _set(3, shape, swap)
    for g, o in zip(gpu64.image_normalization_3(*s3), orc.image_normalization_3(*s3)):
        assert np.array_equal(g, o)
    s4 = _set(4, shape, swap)
    for g, o in zip(gpu64.image_normalization_4(*s4), orc.image_normalization_4(*s4)):
        assert np.array_equal(g, o)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_operators_f32_storage(gpu32, orc, shape, swap):
    """float storage: the (float32-representable) input is held as float, the arithmetic is the oracle's in double, the result is
    rounded to float once"""
    a, = _set(1, shape, swap)
    assert gpu32.getminmax(a) == orc.getminmax(a)
    assert np.array_equal(gpu32.image_normalization_1(a), _f32(orc.image_normalization_1(a)))
    a, b = _set(2, shape, swap)
    for g, o in zip(gpu32.image_normalization_2(a, b), orc.image_normalization_2(a, b)):
        assert np.array_equal(g, _f32(o))


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("nx,ny", [(7, 5), (67, 131)])
def test_normalization_2_color_every_channel_its_own_range(gpu64, orc, nx, ny, swap):
    """nz = 3: channel c spans a range of its own, its extremes at the first pixel of the first image and the last pixel of the
    second; channel 1 is constant in both images (its den is 0: a copy) while the others are not"""
    rng = np.random.default_rng(nx)
    a, b = rng.uniform(10.0, 200.0, (ny, nx, 3)), rng.uniform(10.0, 200.0, (ny, nx, 3))
    for c in (0, 2):
        a[..., c] = a[..., c] * (0.5 + c) + 40.0 * c
        b[..., c] = b[..., c] * (0.5 + c) + 40.0 * c
        lo, hi = -3.5 - c, 977.25 + 100.0 * c
        a[0, 0, c], b[-1, -1, c] = (hi, lo) if swap else (lo, hi)
    a[..., 1] = b[..., 1] = 7.0
    ga, gb = gpu64.image_normalization_2_color(a, b)
    oa, ob = orc.image_normalization_2_color(a, b)
    assert np.array_equal(ga, oa) and np.array_equal(gb, ob)
    assert np.array_equal(ga[..., 1], a[..., 1]) and np.array_equal(gb[..., 1], b[..., 1])
    for c in (0, 2):
        assert min(ga[..., c].min(), gb[..., c].min()) == 0.0 and not np.array_equal(ga[..., c], a[..., c])


# ---- sets in a lockstep group: every pair its own range, one pair constant -------------------------------------------------------
def _ranged_pairs(synth, G, nx, ny):
    """pair g = P1 (variant g) scaled by 0.2 + 0.05 g and shifted by 3 g; the last but one slot is constant (both images 7.0)"""
    pairs = []
    for g in range(G):
        a, b = synth.pair("P1", nx, ny, g)
        pairs.append((a * (0.2 + 0.05 * g) + 3.0 * g, b * (0.2 + 0.05 * g) + 3.0 * g))
    const = G - 1 if G == 2 else G - 2
    pairs[const] = (np.full((ny, nx), 7.0), np.full((ny, nx), 7.0))
    return pairs, const


def _run_group(gpu, entry, pairs, nx, ny, **kw):
    import torch
    d0 = [torch.from_numpy(np.ascontiguousarray(p[0])).cuda() for p in pairs]
    d1 = [torch.from_numpy(np.ascontiguousarray(p[1])).cuda() for p in pairs]
    flo = torch.full((len(pairs), ny, nx, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    getattr(gpu, entry)([t.data_ptr() for t in d0], [t.data_ptr() for t in d1], [flo[k].data_ptr() for k in range(len(pairs))], nx, ny, **kw)
    gpu.synchronize()
    return flo.cpu().numpy().copy()


@pytest.mark.parametrize("G", [2, 16])
@pytest.mark.parametrize("entry,solver", [("tvl1_group_dev", "tvl1_multiscale"), ("hs_group_dev", "hs_pyramidal")])
def test_group_of_pairs_with_ranges_of_their_own(gpu64, orc, synth, entry, solver, G):
    """ofx_tvl1_group_dev / ofx_hs_group_dev, 67 x 35 at 2 levels: the payload of every pair is that of the pair solved alone,
    and for the textured pairs the oracle's flow cast as the payload casts"""
    nx, ny = 67, 35
    pairs, const = _ranged_pairs(synth, G, nx, ny)
    got = _run_group(gpu64, entry, pairs, nx, ny, nscales=2)
    for g, (a, b) in enumerate(pairs):
        alone = _run_group(gpu64, entry, [(a, b)], nx, ny, nscales=2)
        assert np.array_equal(got[g], alone[0]), g
        if g != const:
            uo, vo = getattr(orc, solver)(a, b, nscales=2)[:2]
            assert np.array_equal(got[g], np.stack([uo, vo], axis=-1).astype(np.float32)), g
            assert np.abs(uo).max() > 0


@pytest.mark.parametrize("G", [2, 16])
def test_robust_expo_group_pairs_and_channels_with_ranges_of_their_own(gpu64, synth, G):
    """ofx_robust_expo_group_dev, nz = 3, 32 x 24 at 2 levels: G x nz sets of two.  Pair g, channel c is scaled and shifted by
    its own amounts; channel 2 of pair 1 is constant in both images.  Every pair equals the host entry ofx_robust_expo_pyramid
    on that pair (which tests/rexpo_pyramid_ref.py pins to the CPU)."""
    import torch
    nx, ny, nz = 32, 24, 3
    kw = dict(method=1, nscales=2, outer=2)
    pairs = []
    for g in range(G):
        a, b = synth.colour_pair("P1", nx, ny, nz, g)
        a, b = a.copy(), b.copy()
        for c in range(nz):
            a[..., c] = a[..., c] * (0.2 + 0.05 * g + 0.1 * c) + 3.0 * g + c
            b[..., c] = b[..., c] * (0.2 + 0.05 * g + 0.1 * c) + 3.0 * g + c
        pairs.append((a, b))
    pairs[1][0][..., 2] = pairs[1][1][..., 2] = 7.0
    d1 = [torch.from_numpy(np.ascontiguousarray(p[0])).cuda() for p in pairs]
    d2 = [torch.from_numpy(np.ascontiguousarray(p[1])).cuda() for p in pairs]
    flo = torch.full((G, ny, nx, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu64.robust_expo_group_dev([t.data_ptr() for t in d1], [t.data_ptr() for t in d2], [flo[k].data_ptr() for k in range(G)], nx, ny, nz, **kw)
    gpu64.synchronize()
    got = flo.cpu().numpy()
    for g, (a, b) in enumerate(pairs):
        u, v = gpu64.robust_expo_pyramid(a, b, **kw)
        assert np.array_equal(got[g], np.stack([u, v], axis=-1).astype(np.float32)), g
        assert np.isfinite(u).all() and np.abs(u).max() > 0


# ---- temporal Brox: ONE set over all frames; beyond 32 frames the host entry feeds the head in chunks ------------------------------
BROXT = dict(nscales=1, inner=1, outer=2)


def _ranged_sequence(synth, frames, nx=6, ny=6):
    I = synth.sequence(nx, ny, frames)
    return np.stack([I[f] * (0.3 + 0.02 * f) + 3.0 * f for f in range(frames)])


_BROXT_ORACLE = {}


def _broxt_oracle(orc, synth, frames):
    if frames not in _BROXT_ORACLE:
        I = _ranged_sequence(synth, frames)
        u, v = orc.brox_temporal(I, **BROXT)[:2]
        assert np.isfinite(u).all() and np.isfinite(v).all() and np.abs(u).max() > 0
        _BROXT_ORACLE[frames] = (I, u, v)
    return _BROXT_ORACLE[frames]


@pytest.mark.parametrize("frames", [3, 32, 33])
def test_temporal_brox_host_entry_one_set_over_all_frames(gpu64, orc, synth, frames):
    I, uo, vo = _broxt_oracle(orc, synth, frames)
    u, v = gpu64.brox_temporal(I, **BROXT)
    assert np.array_equal(u, uo) and np.array_equal(v, vo)


@pytest.mark.parametrize("frames", [3, 32])
def test_temporal_brox_device_entry_one_set_over_all_frames(gpu64, orc, synth, frames):
    import torch
    I, uo, vo = _broxt_oracle(orc, synth, frames)
    clip = torch.from_numpy(np.ascontiguousarray(I)).cuda()
    flo = torch.full((frames - 1, 6, 6, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu64.brox_temporal_dev([clip[f].data_ptr() for f in range(frames)], [flo[f].data_ptr() for f in range(frames - 1)], 6, 6, **BROXT)
    gpu64.synchronize()
    assert np.array_equal(flo.cpu().numpy(), np.stack([uo, vo], axis=-1).astype(np.float32))


def test_temporal_brox_device_entry_refuses_33_frames(ofx_mod, gpu64, synth):
    import torch
    clip = torch.from_numpy(np.ascontiguousarray(_ranged_sequence(synth, 33))).cuda()
    flo = torch.full((32, 6, 6, 2), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ofx_mod.OfxError) as e:
        gpu64.brox_temporal_dev([clip[f].data_ptr() for f in range(33)], [flo[f].data_ptr() for f in range(32)], 6, 6, **BROXT)
    assert e.value.status == 1                                    # OFX_ERR_ARG
    torch.cuda.synchronize()
    assert bool((flo == SENTINEL).all().item())
