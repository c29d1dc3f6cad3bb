"""The numpy restatement of ofx_flow_motion_fit_dev (tests/flow_motion_ref.py) on its own: its row sums are sum64, a least-squares
fit is not enough where a third of the frame moves on its own while the re-weighted fits recover the camera's motion, an exact
model flow is recovered for each model, the degenerate cases stop as the header says (CPU only)."""
import numpy as np
import pytest

import flow_motion_ref as R
from track_seed_ref import sum64

MODELS = (R.TRANSLATION, R.SIMILARITY, R.AFFINE)


def test_sum64_rows_is_sum64_of_every_row_bit_for_bit():
    rng = np.random.default_rng(1)
    for n in (1, 2, 63, 64, 65, 130, 200):
        A = rng.normal(0.0, 1.0, (7, n)) * 10.0 ** rng.integers(-3, 4, (7, n))
        A[1] = -0.0                                                    # a sum of negative zeros keeps its sign
        A[2, ::2] = 0.0
        A[3, :] = 0.0
        A[3, n // 2] = -0.0
        got = R.sum64_rows(A)
        want = np.array([sum64(A[i]) for i in range(7)])
        assert got.tobytes() == want.tobytes(), n
    assert np.signbit(R.sum64_rows(np.full((1, 128), -0.0))[0]) and not np.signbit(R.sum64_rows(np.array([[-0.0, 0.0]]))[0])


@pytest.mark.parametrize("nx,ny", [(131, 77), (160, 120)])
def test_least_squares_is_not_enough_and_the_reweighted_fits_recover_the_camera(nx, ny):
    """Measured with this restatement (mean end-point error of the model against the true camera flow, inlier map against the
    background): 131x77 least squares 2.8837 px, 8 re-weighted fits 0.0024 px, 100 %; 160x120 2.8315 px, 0.0025 px, 100 %."""
    flo, fg = R.scene(nx, ny)
    truth = R.TRUE[R.AFFINE]
    ls = R.fit(flo, None, R.AFFINE, 1, 16.0, 1.0)
    rb = R.fit(flo, None, R.AFFINE, 9, 16.0, 1.0)                      # the unweighted fit and 8 re-weighted ones: 16, 8, 4, 2, 1, 1, 1, 1
    e_ls, e_rb = R.mean_epe(ls[:6], truth, nx, ny), R.mean_epe(rb[:6], truth, nx, ny)
    inl = R.outputs(rb[:6], rb[14], flo)[2]
    agree = float(np.mean((inl == 0) == ~fg))
    print("%dx%d: least squares %.4f px, re-weighted %.4f px, inlier map agrees on %.2f %%" % (nx, ny, e_ls, e_rb, 100.0 * agree))
    assert 0.29 < fg.mean() < 0.31
    assert ls[13] == 1 and rb[13] == 9 and rb[15] == 0 and rb[14] == 1.0
    assert e_ls > 1.0                                                  # the input needs robustness
    assert e_rb < 0.02                                                 # a fifth of the per-vector noise
    assert agree >= 0.99
    assert rb[12] < ls[12] == nx * ny                                  # S1: the weights of the last fit leave the rectangle out


@pytest.mark.parametrize("model", MODELS)
def test_an_exact_model_flow_is_recovered_and_has_an_all_zero_map(model):
    nx, ny = 67, 35
    truth = np.array(R.TRUE[model])
    flo = R.model_payload(truth, nx, ny)
    for n_fits in (1, 4):
        rec = R.fit(flo, None, model, n_fits, 16.0, 1.0)
        assert rec[13] == n_fits and rec[15] == 0
        assert np.max(np.abs(rec[:6] - truth)) < 1e-6                  # the float rounding of the payload
        mdl, res, inl = R.outputs(rec[:6], 1.0, flo)
        assert not inl.any() and np.max(np.abs(res)) < 1e-5
    # [6..11] is the same map on pixel indices
    i, j = np.mgrid[0:ny, 0:nx].astype(np.float64)
    mu, mv = R.model_flow(rec[:6], nx, ny)
    assert np.allclose(rec[6] + rec[7] * j + rec[8] * i, mu, atol=1e-9) and np.allclose(rec[9] + rec[10] * j + rec[11] * i, mv, atol=1e-9)
    # a wider model holds a narrower one
    if model != R.AFFINE:
        assert np.max(np.abs(R.fit(flo, None, R.AFFINE, 2, 16.0, 1.0)[:6] - truth)) < 1e-6


def test_flagged_and_nonfinite_vectors_take_no_part():
    nx, ny = 67, 35
    flo, fg = R.scene(nx, ny)
    clean = np.array(flo)
    occ = np.where(fg, 255, 0).astype(np.uint8)                        # the map flags the rectangle: least squares is enough
    rec = R.fit(flo, occ, R.AFFINE, 1, 16.0, 1.0)
    assert R.mean_epe(rec[:6], R.TRUE[R.AFFINE], nx, ny) < 0.05 and rec[12] == np.count_nonzero(~fg)
    bad = R.nonfinite(clean)
    hit = ~np.isfinite(bad).all(axis=-1)
    assert 0.02 < hit.mean() < 0.1
    rec = R.fit(bad, occ, R.AFFINE, 3, 16.0, 1.0)
    assert np.isfinite(rec).all() and rec[15] == 0
    mdl, res, inl = R.outputs(rec[:6], 1.0, bad, occ)
    assert (inl[hit] == 255).all() and (inl[occ != 0] == 255).all() and np.isnan(res[np.isnan(bad)]).all()
    assert np.isfinite(mdl).all()


def test_degenerate_fits_keep_the_theta_they_started_from_and_stop():
    nx, ny = 33, 21
    flo, _ = R.scene(nx, ny)
    everything = np.full((ny, nx), 7, dtype=np.uint8)
    init = R.record(np.array(R.TRUE[R.AFFINE]), nx, ny, 5.0, 3, 1.0, False)
    for model in MODELS:
        rec = R.fit(flo, everything, model, 4, 16.0, 1.0)
        assert not rec[:14].any() and rec[14] == 1.0 and rec[15] == 1.0
        rec = R.fit(flo, everything, model, 4, 16.0, 1.0, init)
        assert np.array_equal(rec[:12], init[:12]) and rec[12] == 0 and rec[13] == 0 and rec[15] == 1.0
    # one valid column: a translation can be fitted, a similarity (with more than one row) too, an affine map cannot
    column = np.full((ny, nx), 255, dtype=np.uint8)
    column[:, 5] = 0
    assert R.fit(flo, column, R.TRANSLATION, 1, 16.0, 1.0)[15] == 0
    assert R.fit(flo, column, R.AFFINE, 3, 16.0, 1.0)[15] == 1.0
    # a cut-off that zeroes every weight at the second fit: the first fit's theta stays, one fit completed
    far = np.array(flo)
    far[..., 0] += np.where(np.arange(nx) % 2 == 0, 50.0, -50.0).astype(np.float32)[None, :]
    one = R.fit(far, None, R.AFFINE, 1, 2.0, 1.0)
    rec = R.fit(far, None, R.AFFINE, 5, 2.0, 1.0)
    assert rec[15] == 1.0 and rec[13] == 1 and np.array_equal(rec[:13], one[:13])


def test_the_schedule_of_cut_offs_and_a_start_from_a_record():
    assert [R.cutoff(t, 16.0, 1.0) for t in range(7)] == [16.0, 8.0, 4.0, 2.0, 1.0, 1.0, 1.0]
    assert R.cutoff(2, 3.0, 0.5) == 0.75 and R.cutoff(3, 3.0, 0.5) == 0.5 and R.cutoff(4000, 3.0, 0.5) == 0.5
    nx, ny = 67, 35
    flo, fg = R.scene(nx, ny)
    # weighted from the truth with a tight cut-off, one fit is enough; from zeros with the same cut-off it is not
    init = R.record(np.array(R.TRUE[R.AFFINE]), nx, ny, 0.0, 0, 1.0, False)
    rec = R.fit(flo, None, R.AFFINE, 1, 1.0, 1.0, init)
    assert rec[13] == 1 and R.mean_epe(rec[:6], R.TRUE[R.AFFINE], nx, ny) < 0.02
    # a call of n fits is a call of k fits followed by a call from its record with the cut-off where the first one left it
    whole = R.fit(flo, None, R.AFFINE, 5, 16.0, 1.0)
    part = R.fit(flo, None, R.AFFINE, 3, 16.0, 1.0)
    rest = R.fit(flo, None, R.AFFINE, 2, 4.0, 1.0, part)
    assert np.array_equal(whole[:13], rest[:13])


def test_camera_motion_from_an_oracle_tvl1_flow(orc, synth):
    """Frame 0 is frame 1 sampled along a known affine flow, with a patch that moves on its own; the flow is the oracle's TV-L1.
    Recorded for DESIGN 8.23 (mean end-point error of the fitted model against the known affine flow): least squares 0.466 px,
    8 re-weighted fits 0.028 px.  Asserted only as robust < least squares."""
    nx, ny = 131, 77
    truth = (1.0, 1.5, -1.0, -0.5, 0.75, 1.0)
    mu, mv = R.model_flow(truth, nx, ny)
    fg = np.zeros((ny, nx), dtype=bool)
    fg[20:50, 40:85] = True
    U, V = mu + np.where(fg, 3.0, 0.0), mv + np.where(fg, -2.0, 0.0)
    i, j = np.mgrid[0:ny, 0:nx].astype(np.float64)
    I0, I1 = synth._tex(j + U, i + V), synth._tex(j, i)
    u, v = orc.tvl1_multiscale(I0, I1, nscales=4)[:2]
    flo = np.stack([u, v], axis=-1).astype(np.float32)
    ls = R.fit(flo, None, R.AFFINE, 1, 16.0, 0.5)
    rb = R.fit(flo, None, R.AFFINE, 9, 16.0, 0.5)
    e_ls, e_rb = R.mean_epe(ls[:6], truth, nx, ny), R.mean_epe(rb[:6], truth, nx, ny)
    print("oracle TV-L1 at %dx%d: least squares %.3f px, re-weighted %.3f px" % (nx, ny, e_ls, e_rb))
    assert e_rb < e_ls
