"""ofx_flow_consistency_dev against its numpy restatement (tests/flow_consistency_ref.py): the maps are EQUAL, byte for byte.

The inputs are those that tests/test_flow_consistency_ref.py pins on the CPU (a real share of flagged pixels in each map, no
pixel within 1e-9 of the threshold), so equality is a fair demand and cannot hold vacuously.  The map is a pure function of the
float payloads: the same bytes from an f64 and an f32 context."""
import numpy as np
import pytest

import flow_consistency_ref as fcr

pytestmark = pytest.mark.gpu

FILL = 0xA5
ERR_ARG = 1


def _up(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()                      # a copy: the shared inputs are read-only
    assert t.data_ptr() % 8 == 0
    return t


def _run(ctx, pairs, nx, ny, offset=0, alpha=fcr.ALPHA, beta=fcr.BETA):
    """the maps of `pairs` [(fwd, bwd), ..] through ONE call, carved out of one byte buffer pre-filled with FILL, map k starting
    `offset` bytes past a 4-byte boundary, guard bytes around each -> [(occ_fwd, occ_bwd), ..]; asserts that no other byte changed"""
    import torch
    n = nx * ny
    stride = (n + 3) // 4 * 4 + 8                      # a multiple of 4: every map starts at the same offset mod 4
    buf = torch.full((2 * len(pairs) * stride + 8,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    starts = [4 + offset + k * stride for k in range(2 * len(pairs))]
    keep = [(_up(f), _up(b)) for f, b in pairs]
    ctx.flow_consistency_dev([f.data_ptr() for f, _ in keep], [b.data_ptr() for _, b in keep],
                             [buf.data_ptr() + starts[2 * k] for k in range(len(pairs))],
                             [buf.data_ptr() + starts[2 * k + 1] for k in range(len(pairs))], nx, ny, alpha, beta)
    ctx.synchronize()
    h = buf.cpu().numpy()
    mask = np.ones(h.size, dtype=bool)
    for s in starts:
        mask[s:s + n] = False
    assert (h[mask] == FILL).all(), "bytes outside the maps were written"
    return [(h[starts[2 * k]:starts[2 * k] + n].reshape(ny, nx), h[starts[2 * k + 1]:starts[2 * k + 1] + n].reshape(ny, nx))
            for k in range(len(pairs))]


@pytest.mark.parametrize("name", fcr.ALL_CASES)
def test_maps_equal_the_restatement(gpu64, gpu32, orc, synth, name):
    """every pinned case (nx not a multiple of 4, nx < 4, more than one wave per row, more than one block), both precisions"""
    fwd, bwd = fcr.case_payloads(orc, synth, name)
    of, ob, _ = fcr.case_maps(orc, synth, name)
    ny, nx = of.shape
    for ctx in (gpu64, gpu32):
        (gf, gb), = _run(ctx, [(fwd, bwd)], nx, ny)
        assert np.array_equal(gf, of), (name, int((gf != of).sum()))
        assert np.array_equal(gb, ob), (name, int((gb != ob).sum()))


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("name", ["67x5", "p1_37x29", "3x5", "2x2"])
def test_unaligned_maps(gpu64, orc, synth, name, offset):
    """maps at byte offsets 1, 2, 3 from a word boundary: equal, and not a byte outside their nx * ny touched"""
    fwd, bwd = fcr.case_payloads(orc, synth, name)
    of, ob, _ = fcr.case_maps(orc, synth, name)
    ny, nx = of.shape
    (gf, gb), = _run(gpu64, [(fwd, bwd)], nx, ny, offset)
    assert np.array_equal(gf, of) and np.array_equal(gb, ob)


@pytest.mark.parametrize("n_pairs,offset", [(5, 1), (17, 3), (17, 0)])
def test_many_pairs_in_one_call(gpu64, orc, synth, n_pairs, offset):
    """5 pairs = one launch of 10 slots; 17 pairs = three launches (8 + 8 + 1 pairs); the pairs differ: pair k is the 67 x 5 case
    with its two payloads exchanged when k is odd and pair 4 is the zero flow"""
    fwd, bwd = fcr.case_payloads(orc, synth, "67x5")
    of, ob, _ = fcr.case_maps(orc, synth, "67x5")
    ny, nx = of.shape
    zero = np.zeros_like(fwd)
    pairs, want = [], []
    for k in range(n_pairs):
        if k == 4:
            pairs.append((zero, zero))
            want.append((np.zeros_like(of), np.zeros_like(of)))
        elif k % 2:
            pairs.append((bwd, fwd))
            want.append((ob, of))
        else:
            pairs.append((fwd, bwd))
            want.append((of, ob))
    got = _run(gpu64, pairs, nx, ny, offset)
    for k in range(n_pairs):
        assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), k


def test_hand_built_payloads(gpu64, orc):
    nx, ny = 9, 6
    z = np.zeros((ny, nx, 2), dtype=np.float32)
    (gf, gb), = _run(gpu64, [(z, z)], nx, ny)
    assert not gf.any() and not gb.any()                           # zero against zero passes everywhere

    F = z.copy()
    F[2, 0, 0] = -0.5            # leaves on the left
    F[2, 8, 0] = 0.25            # ... on the right
    F[0, 3, 1] = -0.25           # ... at the top
    F[5, 3, 1] = 0.125           # ... at the bottom
    F[1, 1, 0] = np.nan
    F[1, 2, 1] = np.nan
    F[3, 1, 0] = np.inf
    F[3, 2, 1] = -np.inf
    F[3, 3, 0] = -np.inf
    F[4, 4, 1] = np.inf
    F[2, 7, 0] = 1.0             # lands exactly on column nx - 1: sampled (1 > 0.01 + 0.5 fails it, 1 <= 1 below passes it)
    F[4, 6, 1] = 1.0             # ... on row ny - 1
    want = np.zeros((ny, nx), dtype=np.uint8)
    for r, c in ((2, 0), (2, 8), (0, 3), (5, 3), (1, 1), (1, 2), (3, 1), (3, 2), (3, 3), (4, 4), (2, 7), (4, 6)):
        want[r, c] = 255
    ref_f, ref_b, _ = fcr.maps(orc, F, z)
    assert np.array_equal(ref_f, want)
    (gf, gb), = _run(gpu64, [(F, z)], nx, ny)
    assert np.array_equal(gf, want) and np.array_equal(gb, ref_b)
    (gf, _), = _run(gpu64, [(F, z)], nx, ny, alpha=0.0, beta=1.0)
    assert gf[2, 7] == 0 and gf[4, 6] == 0                         # sampled, not refused: |w|^2 = 1 <= 1

    # exactly inverse integer translations, alpha = beta = 0: 0 wherever the vector stays inside, 255 where it leaves
    T = z.copy()
    T[..., 0], T[..., 1] = 2.0, -1.0
    Tb = z.copy()
    Tb[..., 0], Tb[..., 1] = -2.0, 1.0
    i, j = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    want_f = np.where((j + 2 <= nx - 1) & (i - 1 >= 0), 0, 255).astype(np.uint8)
    want_b = np.where((j - 2 >= 0) & (i + 1 <= ny - 1), 0, 255).astype(np.uint8)
    (gf, gb), = _run(gpu64, [(T, Tb)], nx, ny, alpha=0.0, beta=0.0)
    assert np.array_equal(gf, want_f) and np.array_equal(gb, want_b)
    ref_f, ref_b, _ = fcr.maps(orc, T, Tb, 0.0, 0.0)
    assert np.array_equal(ref_f, want_f) and np.array_equal(ref_b, want_b)


def test_refusals_write_nothing(ofx_mod, gpu64):
    import torch
    nx, ny = 8, 6
    n = nx * ny
    flo = torch.zeros((2, n + 1, 2), dtype=torch.float32, device="cuda")
    occ = torch.full((2, n), FILL, dtype=torch.uint8, device="cuda")
    f, b = flo[0].data_ptr(), flo[1].data_ptr()
    of, ob = occ[0].data_ptr(), occ[1].data_ptr()
    L, h = gpu64.L, gpu64.h
    arr = lambda xs: (ofx_mod._vp * len(xs))(*xs)

    def refused(status):
        gpu64.synchronize()
        assert status == ERR_ARG, status
        assert L.ofx_last_error(h), "ofx_last_error is empty"
        assert (occ.cpu().numpy() == FILL).all()

    ok = (arr([f]), arr([b]), arr([of]), arr([ob]))
    for k in range(4):                                             # a NULL table, a NULL entry
        t = list(ok)
        t[k] = None
        refused(L.ofx_flow_consistency_dev(h, 1, *t, nx, ny, 0.01, 0.5))
        t[k] = arr([None])
        refused(L.ofx_flow_consistency_dev(h, 1, *t, nx, ny, 0.01, 0.5))
    refused(L.ofx_flow_consistency_dev(h, 0, *ok, nx, ny, 0.01, 0.5))
    refused(L.ofx_flow_consistency_dev(h, -3, *ok, nx, ny, 0.01, 0.5))
    refused(L.ofx_flow_consistency_dev(h, 1, *ok, 1, ny, 0.01, 0.5))
    refused(L.ofx_flow_consistency_dev(h, 1, *ok, nx, 1, 0.01, 0.5))
    for alpha, beta in ((-0.01, 0.5), (0.01, -0.5), (float("nan"), 0.5), (0.01, float("nan")), (float("inf"), 0.5), (0.01, float("inf"))):
        refused(L.ofx_flow_consistency_dev(h, 1, *ok, nx, ny, alpha, beta))
    refused(L.ofx_flow_consistency_dev(h, 1, arr([f + 4]), arr([b]), arr([of]), arr([ob]), nx, ny, 0.01, 0.5))
    refused(L.ofx_flow_consistency_dev(h, 1, arr([f]), arr([b + 4]), arr([of]), arr([ob]), nx, ny, 0.01, 0.5))
    # and the same call without the fault goes through
    gpu64.flow_consistency_dev([f], [b], [of], [ob], nx, ny)
    gpu64.synchronize()
    assert not occ.cpu().numpy().any()
