"""What the regimes of tests/regimes.py mean, pinned on the CPU: tests/test_gpu_regimes.py runs the library on them, and a
later change to the oracle or to synth must not silently turn `still` into a pair that moves or `far` into one that stays inside
the image.

* the oracle equals the compiled reference bit for bit on every regime (TV-L1, Horn-Schunck, Brox spatial, TV-L1 with
  occlusions);
* `still` and `flat` stop every loop at n = 1 with error 0.0 and flow 0.0, at epsilon = 0.01 and at epsilon = 0; every other
  regime runs into the limit of 300 iterations at epsilon = 0;
* no stopping error lies within 1e-4 (relative) of the threshold epsilon^2: the order of the error sum, the one quantity in which
  the kernels may differ from the oracle, cannot legitimately move an iteration count (the closest is `binary`, 1.3e-3);
* the strict oracle and the restatement of the tolerance mode have equal tables, their flows differ by `regimes.cond`;
* every regime does what its name says."""
import numpy as np
import pytest

import regimes as R

EPSILONS = [0.01, 0.0]
OCC = dict(lam=0.15, alpha=0.01, beta=0.15, theta=0.3, nscales=2, zfactor=0.5, warps=1, epsilon=0.01)


def _finest_level(orc, name):
    """the two frames as the finest pyramid level sees them"""
    I0, I1 = orc.image_normalization_2(*R.pair(name, R.NX, R.NY))
    return orc.gaussian(I0, 0.8), orc.gaussian(I1, 0.8)


# ---- the oracle against the compiled reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_oracle_is_the_reference_tvl1(orc, ref, name):
    I0, I1 = R.pair(name, R.NX, R.NY)
    uo, vo, _, _ = R.oracle_tvl1(orc, name, 0.01)
    ur, vr = ref.tvl1_multiscale(I0, I1, epsilon=0.01, **R.TVL1)
    assert np.isfinite(uo).all() and np.isfinite(vo).all()
    assert np.array_equal(uo, ur) and np.array_equal(vo, vr)


@pytest.mark.parametrize("name", R.NAMES)
def test_oracle_is_the_reference_hs_and_brox(orc, ref, name):
    I0, I1 = R.pair(name, R.NX, R.NY)
    ref.set_num_threads(1)
    for kind, run, kw in (("hs", ref.hs_pyramidal, R.HS), ("brox", ref.brox_spatial, R.BROX)):
        uo, vo, _ = R.oracle_sor(orc, kind, name)
        ur, vr = run(I0, I1, **kw)
        assert np.isfinite(uo).all() and np.isfinite(vo).all(), kind
        assert np.array_equal(uo, ur) and np.array_equal(vo, vr), kind


@pytest.mark.parametrize("name", R.NAMES)
def test_oracle_is_the_reference_tvl1_with_occlusions(orc, ref, name):
    seq = R.sequence(name, R.NX, R.NY, 3)
    uo, vo, co, _ = orc.tvl1occ_multiscale(seq[0], seq[1], seq[2], **OCC)
    ur, vr, cr = ref.tvl1occ_multiscale(seq[0], seq[1], seq[2], **OCC)
    assert np.isfinite(uo).all() and np.isfinite(vo).all() and np.isfinite(co).all()
    assert np.array_equal(uo, ur) and np.array_equal(vo, vr) and np.array_equal(co, cr)


# ---- iteration tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("name", R.FROZEN)
def test_frozen_regimes_stop_at_the_first_iteration_with_error_zero(orc, name, epsilon):
    for relaxed in (0, 1):
        u, v, it, err = R.oracle_tvl1(orc, name, epsilon, relaxed)
        assert np.array_equal(it, np.ones((R.TVL1["nscales"], R.TVL1["warps"]), dtype=int)), (relaxed, it)
        assert np.array_equal(err, np.zeros_like(err)), (relaxed, err)
        assert np.array_equal(u, np.zeros_like(u)) and np.array_equal(v, np.zeros_like(v)), relaxed
    for kind in ("hs", "brox"):
        u, v, it = R.oracle_sor(orc, kind, name)
        assert (it == 1).all(), (kind, it)
        assert np.array_equal(u, np.zeros_like(u)) and np.array_equal(v, np.zeros_like(v)), kind


@pytest.mark.parametrize("name", [n for n in R.NAMES if n not in R.FROZEN])
def test_live_regimes_run_into_the_limit_at_epsilon_zero(orc, name):
    for relaxed in (0, 1):
        _, _, it, err = R.oracle_tvl1(orc, name, 0.0, relaxed)
        assert (it == R.MAX_ITERATIONS).all(), (relaxed, it)
        assert (err > 0.0).all(), (relaxed, err)


@pytest.mark.parametrize("name", R.NAMES)
def test_no_stopping_error_lies_at_the_threshold(orc, name):
    """a condition on the inputs, not a measurement: if a later edit of a regime breaks it, change the regime, not the bar"""
    eps2 = 0.01 * 0.01
    for relaxed in (0, 1):
        _, _, it, err = R.oracle_tvl1(orc, name, 0.01, relaxed)
        gap = np.abs(err - eps2) / eps2
        print("%s relaxed=%d: iterations %s, closest stopping error %.3g of the threshold away" % (name, relaxed, it.ravel().tolist(),
                                                                                                   gap.min()))
        assert gap.min() >= 1e-4, (relaxed, err)
        assert ((err < eps2) == (it < R.MAX_ITERATIONS)).all(), (relaxed, it, err)


# ---- strict against tolerance oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("name", R.NAMES)
def test_strict_and_tolerance_oracle_have_equal_tables(orc, name, epsilon):
    it_s, it_r = R.oracle_tvl1(orc, name, epsilon, 0)[2], R.oracle_tvl1(orc, name, epsilon, 1)[2]
    assert np.array_equal(it_s, it_r), (it_s, it_r)
    c, ce = R.cond(orc, name, epsilon)
    print("%s epsilon=%g: cond %.3g, cond_err %.3g" % (name, epsilon, c, ce))
    assert np.isfinite(c) and np.isfinite(ce)
    if name in R.FROZEN:
        assert c == 0.0 and ce == 0.0


@pytest.mark.parametrize("name", R.NAMES)
def test_float_storage_bar_applies_where_the_solve_is_well_conditioned(orc, name):
    """tests/test_gpu_regimes.py holds float storage to the 1e-4 px of BASELINE.json on the regimes whose two restatements agree
    to 1e-9 (epsilon = 0.01): that is every regime"""
    assert R.cond(orc, name, 0.01)[0] < 1e-9


# ---- each regime does what its name says --------------------------------------------------------------------------------------------
def test_halfflat_has_whole_waves_of_flat_pixels(orc):
    _, I1 = _finest_level(orc, "halfflat")
    gx, gy = orc.centered_gradient(I1)
    flat = (gx == 0.0) & (gy == 0.0)
    assert flat.mean() >= 0.45, flat.mean()
    assert flat[:, :56].all() and not flat[:, R.FLAT_COLUMNS + 8:].all()        # a whole strip of every kernel, beside live pixels


def test_far_leaves_the_image(orc):
    """the final flow sends at least 5 % of the pixels out of the image, where the bicubic warp takes its out-of-image branch and
    the mask.  Measured for a roll of 50 / 55 / 60 / 65 / 70 / 80 / 90 / 100 columns: 3.8 / 8.4 / 6.2 / 2.8 / 4.6 / 5.7 / 9.8 /
    7.8 %; through x + u alone 2.5 / 2.6 / 3.5 / 0.8 / 1.5 / 1.4 / 0.0 / 0.4 % -- no roll reaches 5 % that way (the solver never
    follows such a displacement, it leaves through the rows as often as through the columns), so the position counts, and the
    roll is 55."""
    u, v, _, _ = R.oracle_tvl1(orc, "far", 0.01)
    x = np.arange(R.NX)[None, :] + u
    y = np.arange(R.NY)[:, None] + v
    out = (x < 0.0) | (x > R.NX - 1) | (y < 0.0) | (y > R.NY - 1)
    print("far: %.1f %% of the pixels point out of the image" % (100 * out.mean()))
    assert out.mean() >= 0.05, out.mean()
    assert np.abs(u).max() > 10.0                                                # and by far more than the 1-6 px of synth.pair


def test_binary_stops_at_one_and_at_two(orc):
    it = R.oracle_tvl1(orc, "binary", 0.01)[2]
    assert (it == 1).any() and (it == 2).any(), it


def test_faded_and_wide_ranges():
    for I in R.pair("faded", R.NX, R.NY):
        assert I.max() - I.min() < 3.0 and not np.array_equal(I, np.floor(I))
    for I in R.pair("wide", R.NX, R.NY):
        assert I.min() < -1000.0 and I.max() > 30000.0


def test_hs_halfflat_holds_the_sweep_cap_and_an_early_stop(orc):
    it = R.oracle_sor(orc, "hs", "halfflat")[2]
    assert (it == R.HS["maxiter"]).any() and (it < R.HS["maxiter"]).any(), it


# ---- the helper itself --------------------------------------------------------------------------------------------------------------
def test_pairs_sequences_and_groups():
    for name in R.NAMES:
        a, b = R.pair(name, R.NX, R.NY)
        a2, b2 = R.pair(name, R.NX, R.NY)
        assert a.shape == b.shape == (R.NY, R.NX) and a.dtype == b.dtype == np.float64
        assert np.array_equal(a, a2) and np.array_equal(b, b2)                   # deterministic
        s = R.sequence(name, R.NX, R.NY, 4)
        assert s.shape == (4, R.NY, R.NX) and np.isfinite(s).all()
        assert np.array_equal(s, R.sequence(name, R.NX, R.NY, 4))
        assert np.array_equal(s[:3], R.sequence(name, R.NX, R.NY, 3))            # a longer sequence continues a shorter one
        if name in R.FROZEN:
            assert np.array_equal(a, b) and all(np.array_equal(s[0], s[t]) for t in range(1, 4))
        else:
            assert not np.array_equal(a, b) and not np.array_equal(s[0], s[1]) and not np.array_equal(s[1], s[2])
    assert np.array_equal(R.sequence("binary", R.NX, R.NY, 2), np.stack(R.pair("binary", R.NX, R.NY)))
    assert R.group_names(8) == ["still", "flat", "halfflat", "binary", "far", "noisy", "wide", "faded"]
    assert R.group_names(16)[0] == "still" and R.group_names(16)[-1] == "still" and set(R.group_names(16)) == set(R.NAMES)
    assert len(R.group(R.NX, R.NY, 8)) == 8
    for bad in ((79, 60), (80, 59)):
        with pytest.raises(ValueError):
            R.pair("binary", *bad)
        with pytest.raises(ValueError):
            R.sequence("halfflat", *bad, 3)
    with pytest.raises(ValueError):
        R.pair("moving", R.NX, R.NY)
