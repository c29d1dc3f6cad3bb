"""The numpy restatement of ofx_flow_compose_dev, ofx_flow_accumulate_dev and ofx_flow_tracks_dev (tests/flow_compose_ref.py) and the
inputs that the GPU tests share: its sampling is the oracle's to the bit, every branch of the definition occurs over the case set,
closed forms, the tracks against the dense chain, and what an accumulated flow is good for (CPU only)."""
import numpy as np

import flow_apply_ref as far
import flow_compose_ref as R
import flow_consistency_ref as fcr


def test_the_step_payloads_follow_the_formula_of_the_consistency_cases():
    nx, ny, amp, seed = fcr.NOISE_CASES["130x70"]
    f, b = R.noise_step(nx, ny, amp, seed)
    wf, wb = fcr.noise_payloads("130x70")
    assert f.tobytes() == wf.tobytes() and b.tobytes() == wb.tobytes()
    for name, (nx, ny, amp, seed) in R.CASES.items():
        s = R.steps(name)
        assert len(s) == R.MAX_STEPS and all(p.shape == (ny, nx, 2) and p.dtype == np.float32 for p in s)
        assert len({p.tobytes() for p in s}) == R.MAX_STEPS                         # one seed per step
    assert R.steps(R.JUMP)[0].tobytes() == far.payloads(None, None, far.JUMP)[0].tobytes()


def test_sample_is_the_oracles_bicubic_to_the_bit(orc):
    for name in ("3x5", "37x29", R.JUMP):
        S = R.steps(name)[1]
        ny, nx, _ = S.shape
        S64 = np.ascontiguousarray(S.astype(np.float64))
        # dense, at (j + U, i + V): Oracle.bicubic_warp_color
        U, V = R.steps(name)[0][..., 0].astype(np.float64), R.steps(name)[0][..., 1].astype(np.float64)
        i, j = R._grid(ny, nx)
        ok = R.inside(j + U, i + V, nx, ny)
        assert ok.any() and not ok.all()
        bu, bv = R.sample(S, j + U, i + V, ok)
        w = orc.bicubic_warp_color(S64, np.where(ok, U, 0.0), np.where(ok, V, 0.0), False)
        assert np.array_equal(bu[ok], w[..., 0][ok]) and np.array_equal(bv[ok], w[..., 1][ok])
        assert not bu[~ok].any() and not bv[~ok].any()
        # points: Oracle.bicubic_at_color, edges and corners among them
        p = R.query_points(nx, ny, 64)
        okp = R.inside(p[:, 0], p[:, 1], nx, ny)
        pu, pv = R.sample(S, p[:, 0], p[:, 1], okp)
        for k in np.flatnonzero(okp):
            assert pu[k] == orc.bicubic_at_color(S64, float(p[k, 0]), float(p[k, 1]), 0), (name, k)
            assert pv[k] == orc.bicubic_at_color(S64, float(p[k, 0]), float(p[k, 1]), 1), (name, k)


def test_flagged_takes_the_pixels_around_a_position_and_never_leaves_the_map():
    M = np.zeros((4, 5), dtype=np.uint8)
    M[1, 2] = 7
    pts = {(2.0, 1.0): True, (1.0, 1.0): False, (1.5, 1.0): True, (1.0, 0.5): False, (2.0, 0.25): True, (2.5, 1.5): True,
           (3.0, 1.0): False, (1.25, 1.75): True, (4.0, 3.0): False, (3.5, 3.0): False, (0.0, 0.0): False}
    x, y = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    ok = np.ones(len(pts), dtype=bool)
    assert list(R.flagged(M, x, y, ok)) == list(pts.values())
    assert not R.flagged(None, x, y, ok).any()
    M[:] = 0
    M[3, 4] = 255                                                        # the last pixel: reached only by positions around it
    assert list(R.flagged(M, np.array([4.0, 3.5, 4.0, 3.0]), np.array([3.0, 2.5, 2.0, 3.0]), np.ones(4, dtype=bool))) == [True, True, False, False]


def test_every_branch_of_the_definition_occurs_over_the_case_set(orc):
    seen = {}

    def add(where, branches):
        for code in np.unique(branches):
            seen.setdefault(int(code), where)

    first_step = np.zeros(8, dtype=np.int64)
    for name in R.CASES:
        for with_maps in (False, True):
            for t, (_, occ, br) in enumerate(R.want(orc, name, R.MAX_STEPS, with_maps)):
                add((name, with_maps, t), br)
                assert np.array_equal(occ != 0, br != R.BR_OK)
                if t == 0:
                    first_step += np.bincount(br.ravel(), minlength=8)
    assert first_step[R.BR_FLAGGED_AT_PIXEL] > 0 and first_step[R.BR_FROZEN] == 0            # lost by the map at the start
    add("nonfinite", np.concatenate([b.ravel() for _, _, b in R.accumulate(R.nonfinite_steps())]))
    # a plain compose of two payloads without maps: the first vector itself leaves
    a, b = R.steps("37x29")[:2]
    add("compose", R.compose_parts(a, b)[2])
    for code in (R.BR_OK, R.BR_FROZEN, R.BR_LEAVES_BEFORE, R.BR_FLAGGED_AT_PIXEL, R.BR_FLAGGED_OWN, R.BR_FLAGGED_NEIGHBOUR,
                 R.BR_NONFINITE, R.BR_LEAVES_AFTER):
        assert code in seen, code


def test_at_130x70_after_4_steps_a_quarter_survives_and_a_hundredth_is_lost(orc):
    for with_maps in (False, True):
        occ = R.want(orc, "130x70", 4, with_maps)[3][1]
        survive = float((occ == 0).mean())
        print("130x70, 4 steps, maps %s: %.1f %% survive" % (with_maps, 100.0 * survive))
        assert survive >= 0.25 and 1.0 - survive >= 0.01


def test_lost_vectors_stay_where_they_were_lost_bit_for_bit(orc):
    acc = R.accumulate(R.nonfinite_steps(), R.step_maps(orc, "37x29"))
    for t in range(1, len(acc)):
        gone = acc[t - 1][1] != 0
        assert gone.any() and (acc[t][1][gone] == 255).all()
        assert acc[t][0][gone].tobytes() == acc[t - 1][0][gone].tobytes()
        assert (acc[t][2][gone] == R.BR_FROZEN).all()
    # a NaN that is frozen keeps its bits: compose of a payload that holds one, under a map that flags it
    a = np.array(R.steps("37x29")[0])
    a[3, 4] = np.frombuffer(np.array([0x7FC12345, 0xFF800000], dtype=np.uint32).tobytes(), dtype=np.float32)
    m = np.zeros(a.shape[:2], dtype=np.uint8)
    m[3, 4] = 1
    for occ_ab in (m, None):                                             # flagged by the map, or lost because NaN is not inside
        ac, occ = R.compose(a, R.steps("37x29")[1], occ_ab)
        assert ac[3, 4].tobytes() == a[3, 4].tobytes() and occ[3, 4] == 255


def test_closed_form_constant_integer_steps():
    nx, ny, n_steps = 23, 11, 5
    i, j = R._grid(ny, nx)
    acc = R.accumulate(R.constant_steps(nx, ny, n_steps))
    prev, prev_ok = np.zeros((ny, nx, 2), dtype=np.float32), np.ones((ny, nx), dtype=bool)
    for t, (ac, occ, _) in enumerate(acc, start=1):
        ok = prev_ok & R.inside(j + 2.0 * t, i - 1.0 * t, nx, ny)
        want = np.where(ok[..., None], np.array([2.0 * t, -1.0 * t], dtype=np.float32), prev)
        assert np.array_equal(ac, want) and np.array_equal(occ, np.where(ok, 0, 255))
        prev, prev_ok = want, ok
    assert prev_ok.any() and not prev_ok.all()


def test_the_two_consequences_of_the_header(orc):
    for name in ("37x29", R.JUMP):
        bc, occ_bc = R.steps(name)[0], R.step_maps(orc, name)[0]
        ny, nx, _ = bc.shape
        i, j = R._grid(ny, nx)
        stays = R.inside(j + bc[..., 0].astype(np.float64), i + bc[..., 1].astype(np.float64), nx, ny)
        for m in (None, occ_bc):
            ok = stays if m is None else stays & (m == 0)
            for ab in (None, np.zeros_like(bc)):
                ac, occ = R.compose(ab, bc, None, m)
                assert np.array_equal(occ == 0, ok) and ac[ok].tobytes() == bc[ok].tobytes() and not ac[~ok].any()
        # an all-zero step: ab itself, the vectors that leave flagged
        ab = R.steps(name)[1]
        goes = R.inside(j + ab[..., 0].astype(np.float64), i + ab[..., 1].astype(np.float64), nx, ny)
        ac, occ = R.compose(ab, np.zeros_like(bc))
        assert ac.tobytes() == ab.tobytes() and np.array_equal(occ == 0, goes) and not goes.all()


def test_tracks_started_on_the_pixel_grid_agree_with_the_dense_chain_to_float_rounding():
    """The dense chain rounds (U + bu, V + bv) to float once per step; the tracks do not.  With e_t the distance between the two
    positions of a pixel after step t, per component: e_{t+1} <= (1 + L) e_t + h_{t+1}, where h_t is half an ulp of the largest
    accumulated component after step t and L bounds the change of a sampled step vector per unit of position.  The steps here are
    the sine fields alone, amplitude 1.5: their Jacobian's entries are at most 1.5 * (0.31, 0.17, 0.11, 0.23), Frobenius norm
    below 0.65, and the Keys cubic through samples of so smooth a field stays within a quarter of that: 1 + L < 2.  Hence
    e_T <= sum_t 2^(T - t) h_t, asserted per component over the pixels that survive in both."""
    nx, ny, n_steps = 64, 40, 4
    steps = R.smooth_steps(nx, ny, n_steps)
    acc = R.accumulate(steps)
    i, j = R._grid(ny, nx)
    xy, length = R.tracks(steps, np.stack([j.ravel(), i.ravel()], axis=-1))
    bound = 0.0
    for t in range(1, n_steps + 1):
        ac, occ, _ = acc[t - 1]
        h = 0.5 * float(np.spacing(np.abs(ac[occ == 0]).max()))           # float32 spacing: ac is float32
        bound = 2.0 * bound + h if t > 1 else h
        both = (occ == 0).ravel() & (length >= t)
        dense = np.stack([j + ac[..., 0].astype(np.float64), i + ac[..., 1].astype(np.float64)], axis=-1).reshape(-1, 2)
        err = float(np.abs(dense[both] - xy[t][both]).max())
        print("step %d: %d pixels in both, max |dense - track| = %.3g, bound %.3g" % (t, int(both.sum()), err, bound))
        assert both.sum() > nx * ny // 2 and err <= bound


def test_tracks_lengths_and_frozen_positions(orc):
    name = "37x29"
    nx, ny = R.CASES[name][:2]
    steps, maps = R.nonfinite_steps(name), R.step_maps(orc, name)
    p0 = R.query_points(nx, ny, 64)
    for occ in (None, maps):
        xy, length = R.tracks(steps, p0, occ)
        assert xy[0].tobytes() == p0.tobytes()
        out = ~R.inside(p0[:, 0], p0[:, 1], nx, ny)
        assert out.sum() >= 7 and (length[out] == -1).all() and (length[~out] >= 0).all()
        for k in range(len(p0)):
            stop = max(int(length[k]), 0)
            for t in range(stop, len(steps) + 1):
                assert xy[t][k].tobytes() == xy[stop][k].tobytes()          # a NaN start included
            for t in range(1, stop + 1):
                assert R.inside(xy[t][k, 0], xy[t][k, 1], nx, ny) and xy[t][k].tobytes() != xy[t - 1][k].tobytes()
        assert (length == len(steps)).any() and ((length >= 0) & (length < len(steps))).any()
    # the corners and the edge points start inside
    assert (R.tracks(steps, p0[:7])[1] >= 0).all()


def test_an_accumulated_flow_registers_frame_t_onto_frame_0(orc, synth):
    """oracle TV-L1 steps on synth.sequence(131, 77, 4): over the surviving pixels, frame t warped by the accumulated flow 0 -> t is
    closer to frame 0 than frame t itself.  The figures, and the end-point error against the direct solve 0 -> t, are printed for
    DESIGN 8.21."""
    nx, ny, nscales = 131, 77, 4
    F = synth.sequence(nx, ny, 4)
    steps = [fcr.payload(*orc.tvl1_multiscale(F[t], F[t + 1], nscales=nscales)[:2]) for t in range(3)]
    acc = R.accumulate(steps)
    for t in range(1, 4):
        ac, occ, _ = acc[t - 1]
        ok = occ == 0
        warped = far.warp(orc, np.ascontiguousarray(F[t][..., None]), ac, occ)[..., 0]
        rmse = lambda a: float(np.sqrt(np.mean((a[ok] - F[0][ok]) ** 2)))
        r_warp, r_raw = rmse(warped), rmse(F[t])
        ud, vd = orc.tvl1_multiscale(F[0], F[t], nscales=nscales)[:2] if t > 1 else (steps[0][..., 0], steps[0][..., 1])
        aepe = float(np.mean(np.hypot(ac[..., 0][ok] - ud[ok], ac[..., 1][ok] - vd[ok])))
        print("0 -> %d: %.1f %% survive, RMSE warped %.3f against unwarped %.3f, AEPE against the direct solve %.3f px"
              % (t, 100.0 * ok.mean(), r_warp, r_raw, aepe))
        assert ok.mean() > 0.5 and r_warp < r_raw
