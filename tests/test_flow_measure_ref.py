"""The numpy restatement of ofx_flow_error_dev, ofx_flow_encode_dev and ofx_flow_decode_dev (tests/flow_measure_ref.py) on its own:
against a straight numpy computation, the known values of the colour wheel, the round trips of the two decodable codings, an oracle
TV-L1 flow against its ground truth, and the share of a picture that the wheel's three-way rule exempts (CPU only)."""
import numpy as np
import pytest

import flow_measure_ref as R

# the sizes of tests/test_gpu_flow_measure.py and of the front-end test
GPU_SIZES = [(2, 2), (3, 5), (64, 2), (65, 3), (63, 65), (130, 131), (37, 29), (67, 35)]


@pytest.mark.parametrize("nx,ny", [(131, 77), (65, 3), (2, 2)])
def test_error_record_against_a_straight_numpy_computation(nx, ny):
    gt = R.spoiled(R.truth(nx, ny), 1)
    flo = R.spoiled(R.estimate(nx, ny), 2)
    occ = R.flags(nx, ny)
    for m in (None, occ):
        rec, epe, hist = R.error(flo, gt, m, R.THR_ABS, R.THR_REL, 64, 0.125)
        u, v, gu, gv = (a.astype(np.float64) for a in (flo[..., 0], flo[..., 1], gt[..., 0], gt[..., 1]))
        known = np.isfinite(gu) & np.isfinite(gv) & (np.abs(gu) <= 1e9) & (np.abs(gv) <= 1e9)
        if m is not None:
            known &= m == 0
        good = known & np.isfinite(u) & np.isfinite(v)
        bad = known & ~good
        assert rec[0] == known.sum() and rec[1] == bad.sum()
        with np.errstate(all="ignore"):
            e = np.hypot(u - gu, v - gv)
            ae = np.arccos(np.clip((u * gu + v * gv + 1.0) / np.sqrt((u * u + v * v + 1.0) * (gu * gu + gv * gv + 1.0)), -1.0, 1.0))
            gm = np.hypot(gu, gv)
        if good.any():
            assert abs(rec[2] - np.mean(e[good])) <= 1e-12 * np.mean(e[good])
            assert abs(rec[3] - np.sqrt(np.mean(e[good] ** 2))) <= 1e-12 * rec[3]
            assert abs(rec[4] - np.degrees(np.mean(ae[good]))) <= 1e-12 * rec[4]
            assert abs(rec[5] - e[good].max()) <= 1e-12 * rec[5]
            assert abs(rec[6] - e[good].sum()) <= 1e-12 * rec[6] and abs(rec[7] - ae[good].sum()) <= 1e-12 * rec[7]
        else:
            assert not rec[2:8].any()
        for k in range(6):
            with np.errstate(all="ignore"):
                out = bad | (good & (e > R.THR_ABS[k]) & (e > R.THR_REL[k] * gm))
            assert rec[8 + k] == out.sum(), k
        assert not rec[14:].any()
        # the histogram: np.histogram of the good pixels' errors with the last bin open, plus the bad pixels in the last bin
        want = np.histogram(np.minimum(e[good], 64 * 0.125 - 1e-9), bins=64, range=(0.0, 64 * 0.125))[0]
        want[-1] += bad.sum()
        assert np.array_equal(hist, want) and hist.sum() == rec[0] and hist.dtype == np.uint32
        assert np.array_equal(np.isnan(epe), ~known) and np.isposinf(epe[bad]).all()
        assert np.allclose(epe[good], e[good], rtol=1e-6, atol=0.0)
        assert epe[~known].view(np.uint32).tolist() == [0x7FC00000] * int((~known).sum())
    # no threshold, no histogram
    rec0, _, none = R.error(flo, gt)
    assert none is None and not rec0[8:].any()


def test_degenerate_slots_and_percentiles():
    nx, ny = 9, 7
    gt, flo = R.truth(nx, ny), R.estimate(nx, ny)
    rec, epe, hist = R.error(flo, gt, np.full((ny, nx), 3, dtype=np.uint8), (1.0,), (0.0,), 4, 1.0)
    assert not rec.any() and not hist.any() and np.isnan(epe).all()
    allbad = np.full_like(flo, np.nan)
    rec, epe, hist = R.error(allbad, gt, None, (1.0,), (0.0,), 4, 1.0)
    assert rec[0] == rec[1] == rec[8] == nx * ny and not rec[2:8].any() and hist.tolist() == [0, 0, 0, nx * ny] and np.isposinf(epe).all()
    # an unknown truth (Middlebury's 1e10 marker, a decoded KITTI hole) leaves the pixel out whatever the estimate is
    hole = np.array(gt)
    hole[0, 0] = (1e10, 1e10)
    hole[1, 1] = (np.nan, np.nan)
    assert R.error(flo, hole)[0][0] == nx * ny - 2
    # a percentile is the upper edge of the bin at which the cumulative count reaches ceil(p * known)
    h = np.array([5, 0, 3, 2], dtype=np.uint32)
    assert R.percentile_edge(h, 10, 0.5, 0.25) == 0.25 and R.percentile_edge(h, 10, 0.75, 0.25) == 0.75
    assert R.percentile_edge(h, 10, 0.95, 0.25) == 1.0 and R.percentile_edge(h, 0, 0.5, 0.25) == 0.0


KNOWN = [((0, 0), (255, 255, 255)), ((1, 0), (255, 191, 191)), ((-1, 0), (191, 243, 255)), ((0, 1), (255, 248, 191)),
         ((0, -1), (213, 191, 255)), ((2, 2), (255, 155, 74)), ((-2, 2), (97, 255, 74)), ((3, -3), (164, 0, 191))]


def test_the_known_values_of_the_wheel():
    assert R.WHEEL.shape == (55, 3) and R.WHEEL[0].tolist() == [255, 0, 0] and R.WHEEL[15].tolist() == [255, 255, 0]
    assert R.WHEEL[21].tolist() == [0, 255, 0] and R.WHEEL[25].tolist() == [0, 255, 255] and R.WHEEL[36].tolist() == [0, 0, 255]
    assert R.WHEEL[49].tolist() == [255, 0, 255] and R.WHEEL[54].tolist() == [255, 0, 43]
    flo = np.array([[k[0] for k in KNOWN]], dtype=np.float32)
    got = R.encode_wheel(flo, None, 4.0)
    assert got[0].tolist() == [list(k[1]) for k in KNOWN]
    # its own maximum: the longest vector, (3, -3), sits on the rim
    own = R.encode_wheel(flo, None, 0.0)
    assert R.maxrad_of(flo, None, 0.0) == np.sqrt(18.0) and own[0, 0].tolist() == [255, 255, 255]
    # what is not shown is black; an all-zero field has maxrad 1
    flo2 = np.array(flo)
    flo2[0, 1] = (np.nan, 0.0)
    flo2[0, 2] = (1e10, 1e10)
    occ = np.zeros((1, 8), dtype=np.uint8)
    occ[0, 3] = 1
    got = R.encode_wheel(flo2, occ, 4.0)
    assert not got[0, 1:4].any() and got[0, 4:].tolist() == [list(k[1]) for k in KNOWN[4:]]
    assert R.maxrad_of(np.zeros((2, 2, 2), dtype=np.float32), None, 0.0) == 1.0
    assert (R.encode_wheel(np.zeros((2, 2, 2), dtype=np.float32)) == 255).all()


def test_round_trips_of_the_two_decodable_codings():
    nx, ny = 67, 35
    flo = R.estimate(nx, ny)
    # KITTI: exact where 64 f is an integer in range
    q = (np.round(flo.astype(np.float64) * 64.0) / 64.0 + 0.0).astype(np.float32)       # + 0.0: a -0.0 comes back as +0.0
    back, m = R.decode_kitti(R.encode_kitti(q))
    assert back.tobytes() == q.tobytes() and not m.any()
    code = R.encode_kitti(flo)
    back, m = R.decode_kitti(code)
    assert np.max(np.abs(back - flo)) <= 1.0 / 128 + 1e-6 and (code[..., 2] == 1).all()
    big = np.array([[(600.0, -600.0), (511.984375, -512.0)]], dtype=np.float32)
    assert R.encode_kitti(big)[0].tolist() == [[65535, 0, 1], [65535, 0, 1]]
    # holes: flagged and unshown pixels are (0, 0, 0) and decode to NaN with the map set
    occ = R.flags(nx, ny)
    sp = R.spoiled(flo)
    code = R.encode_kitti(sp, occ)
    hole = ~R.vis(sp, occ)
    assert hole.any() and not code[hole].any() and (code[~hole][:, 2] == 1).all()
    back, m = R.decode_kitti(code)
    assert np.array_equal(m != 0, hole) and np.isnan(back[hole]).all() and np.isfinite(back[~hole]).all()
    rec = R.error(flo, back)[0]
    assert rec[0] == np.count_nonzero(~hole)                      # the error entry leaves the holes out without the map
    # BOUND: within B / 255 inside the bound, clamped outside it, 128 where not shown
    for B in (20.0, 8.0):
        code = R.encode_bound(flo, None, B)
        back, m = R.decode_bound(code, B)
        inside = (np.abs(flo) < B).all(axis=-1)
        assert np.max(np.abs(back[inside] - flo[inside])) <= B / 255 + 1e-6 and not m.any()
        assert inside.all() == (B == 20.0)
        assert (code[flo >= B] == 255).all() and (code[flo <= -B] == 0).all()
    assert (R.encode_bound(sp, occ, 20.0)[hole] == 128).all()
    assert R.encode_bound(np.array([[(-20.0, 20.0), (0.0, 19.99)]], dtype=np.float32), None, 20.0)[0].tolist() == [[0, 255], [128, 255]]


def test_record_of_an_oracle_tvl1_flow_is_the_hypot_mean_of_the_existing_tests(orc, synth):
    nx, ny = 160, 120
    I0, I1 = synth.pair("P0", nx, ny)
    u, v = orc.tvl1_multiscale(I0, I1, nscales=4)[:2]
    i, j = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    fx, fy = synth._flow(i, j)
    flo = np.stack([u, v], axis=-1).astype(np.float32)
    gt = np.stack([fx, fy], axis=-1).astype(np.float32)
    rec, _, hist = R.error(flo, gt, None, R.THR_ABS, R.THR_REL, 4096, 1.0 / 64)
    want = float(np.mean(np.hypot(flo[..., 0].astype(np.float64) - gt[..., 0], flo[..., 1].astype(np.float64) - gt[..., 1])))
    print("oracle TV-L1 on P0 %dx%d: AEPE %.6f px, AAE %.4f deg, R1 %.4f, A95 %.4f px" %
          (nx, ny, rec[2], rec[4], rec[9] / rec[0], R.percentile_edge(hist, rec[0], 0.95, 1.0 / 64)))
    assert rec[0] == nx * ny and rec[1] == 0
    assert abs(rec[2] - want) <= 1e-12 * want
    assert rec[2] < 0.5 and rec[8] >= rec[9] >= rec[10] >= rec[11] >= rec[12]


def test_the_three_way_rule_exempts_at_most_one_percent_of_a_picture():
    worst = 0.0
    for nx, ny in GPU_SIZES + [(131, 77), (64, 48)]:
        flo = R.truth(nx, ny)
        for scale in (0.0, 4.0):
            three, differ = R.wheel3(flo, None, scale)
            share = differ.mean()
            print("%dx%d maxrad %s: the three restatements differ at %d of %d pixels" %
                  (nx, ny, "own" if scale == 0 else scale, differ.sum(), nx * ny))
            worst = max(worst, share)
            assert share <= 0.01, (nx, ny, scale)
            ok, _ = R.wheel_ok(three[0], flo, None, scale)
            assert ok
    flo = np.array([[k[0] for k in KNOWN]], dtype=np.float32)
    assert R.wheel_ok(R.encode_wheel(flo, None, 4.0), flo, None, 4.0)[0]
    wrong = R.encode_wheel(flo, None, 4.0)
    wrong[0, 5, 1] ^= 1
    assert not R.wheel_ok(wrong, flo, None, 4.0)[0]
