"""The restatement of the track seeds and dense point trajectories (tests/track_seed_ref.py) on the CPU: every branch of the rule
occurs over the shared cases, the density invariant holds, and what re-seeding is good for is printed for README and DESIGN 8.22.

A candidate that fails on a NaN can only occur in a frame whose mean is NaN too (the mean sums every lam2), so there nothing has
structure: the NaN case is a frame of its own, outside the cases whose structured share is asserted."""
import numpy as np

import flow_compose_ref as fcr
import flow_consistency_ref as fcons
import track_seed_ref as R

CASES = ("37x29", "130x70")
CAP = {"37x29": 40, "130x70": 2000}                    # 37x29 starts 43 or 44 tracks without a cap: seeds of the later frames are
                                                       # dropped; 130x70 starts about 470: room for all


def test_sum64_is_the_fixed_tree_and_not_the_running_sum():
    rng = np.random.default_rng(1)
    for n in (1, 7, 63, 64, 65, 130, 1000):
        v = rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-8, 8, n)
        lanes = []
        for l in range(64):
            acc = 0.0
            for k, x in enumerate(v[l::64]):
                acc = x if k == 0 else acc + x
            lanes.append(acc)
        while len(lanes) > 1:
            h = len(lanes) // 2
            lanes = [lanes[l] + lanes[l + h] for l in range(h)]
        assert R.sum64(v) == lanes[0], n
    v = np.zeros(64)
    v[0], v[1], v[33] = 2.0 ** 53, 1.0, 1.0                             # lanes 1 and 33 meet first: a running sum loses both ones
    assert R.sum64(v) == 2.0 ** 53 + 2.0 and float(np.cumsum(v)[-1]) == 2.0 ** 53
    assert np.signbit(R.sum64([-0.0])) == False                         # the empty lanes are +0.0


def test_every_branch_occurs_over_the_shared_cases(orc):
    seen = set()
    for name in CASES:
        nx, ny = fcr.CASES[name][:2]
        vals = R.clip(nx, ny)[1]
        frac = R.pick_frac(orc, vals)
        ncx, ncy = R.cells(nx, ny, R.STEP)
        cand = {e for e, _, _ in R.candidates(nx, ny, R.STEP)}
        if any(cb * ncx + ncx - 1 not in cand for cb in range(ncy)):
            seen.add("no candidate at the right edge")
        if any((ncy - 1) * ncx + ca not in cand for ca in range(ncx)):
            seen.add("no candidate at the bottom edge")
        for with_maps in (False, True):
            res, _ = R.want_sequence(orc, name, 5, with_maps, CAP[name])
            for f, (l2, mean) in enumerate(res["structure"]):
                s = R.share(l2, mean, frac, R.STEP)
                print("%s frame %d: %.1f %% of the candidates have structure (frac %.4g)" % (name, f, 100.0 * s, frac))
                assert 0.10 < s < 0.90, (name, f, s)
                st = R.structured(l2, mean, frac, R.STEP)
                seen.add("above tau")
                if len(st) < len(cand):
                    seen.add("below tau")
                live = (res["t0"] <= f) & (res["t0"] + res["len"] >= f)
                born = res["t0"] == f
                if R.occupied(res["xy"][f][live & ~born], nx, ny, R.STEP) & set(st):
                    seen.add("occupied cell")
            freed = {(f, e) for f, e in res["freed"]}
            births = {(int(t), int(e)) for t, e in zip(res["t0"], [int(p[1]) // R.STEP * ncx + int(p[0]) // R.STEP
                                                                    for p in res["xy"][0]])}
            if any(t > 0 for t, _ in births):
                seen.add("born after frame 0")
            if freed & births:
                seen.add("cell freed by a loss and seeded again")
            if res["count"][1] > 0:
                seen.add("dropped by cap")
                assert res["count"][0] == CAP[name]
            if res["lost_map"]:
                seen.add("lost by the map")
            if res["lost_leave"]:
                seen.add("lost by leaving")
    # the NaN frame: a NaN sample makes lam2 NaN around it and the mean NaN: every candidate fails the comparison
    vals = np.array(R.clip(37, 29)[1][0])
    vals[14, 18] = np.nan
    l2, mean = R.structure(orc, vals, R.RHO)
    assert np.isnan(l2[14, 18]) and np.isnan(mean) and np.isfinite(l2[2, 2])
    assert R.seeds(l2, mean, 0.0, R.STEP)[1] == 0
    seen.add("fails on NaN")
    want = {"above tau", "below tau", "fails on NaN", "occupied cell", "cell freed by a loss and seeded again",
            "no candidate at the right edge", "no candidate at the bottom edge", "dropped by cap", "born after frame 0",
            "lost by the map", "lost by leaving"}
    assert seen == want, want - seen


def test_seeds_come_in_cell_order_and_cap_drops_the_last(orc):
    nx, ny = 37, 29
    vals = R.clip(nx, ny)[1]
    frac = R.pick_frac(orc, vals)
    l2, mean = R.structure(orc, vals[0], R.RHO)
    for step in (1, 3, 4, 8):
        xy, w, d = R.seeds(l2, mean, frac, step)
        assert d == 0 and w == len(xy) > 2
        key = (xy[:, 1].astype(int) // step) * 1000 + xy[:, 0].astype(int) // step
        assert (np.diff(key) > 0).all()
        xy2, w2, d2 = R.seeds(l2, mean, frac, step, cap=w - 2)
        assert w2 == w - 2 and d2 == 2 and np.array_equal(xy2, xy[:w - 2])
        occ = np.array([xy[1], [np.nan, 2.0], [-1.0, 0.0], [nx - 0.5, 3.0]])
        xy3, w3, _ = R.seeds(l2, mean, frac, step, occ_points=occ)
        assert w3 == w - 1 and np.array_equal(xy3, np.delete(xy, 1, axis=0))


def test_the_density_invariant_holds(orc):
    for name in CASES:
        nx, ny = fcr.CASES[name][:2]
        for with_maps in (False, True):
            for cap in (CAP[name], 100000):
                res, frac = R.want_sequence(orc, name, 5, with_maps, cap)
                assert R.density_holes(res, frac, R.STEP, nx, ny, cap) == []
            # ... and does not without re-seeding: the check can fail
            res, frac = R.want_sequence(orc, name, 5, with_maps, 100000, reseed=False)
            assert R.density_holes(res, frac, R.STEP, nx, ny, 100000) != []


def test_slots_are_written_as_the_header_says(orc):
    res, _ = R.want_sequence(orc, "130x70", 5, True, CAP["130x70"])
    xy, t0, ln = res["xy"], res["t0"], res["len"]
    assert (np.diff(t0) >= 0).all() and ((ln >= 0) & (t0 + ln <= 4)).all()
    for k in range(len(t0)):
        for f in range(t0[k]):
            assert xy[f, k].tobytes() == xy[t0[k], k].tobytes()
        for f in range(t0[k] + ln[k] + 1, 5):
            assert xy[f, k].tobytes() == xy[t0[k] + ln[k], k].tobytes()
    born0 = t0 == 0
    wxy, wl = fcr.tracks(fcr.steps("130x70", 4), xy[0][born0], fcr.step_maps(orc, "130x70", 4))
    assert wxy.tobytes() == np.ascontiguousarray(xy[:, born0]).tobytes() and np.array_equal(wl, ln[born0])


def test_what_reseeding_is_good_for(orc, synth):
    """synth.sequence(131, 77, 5) with oracle TV-L1 steps both ways and their consistency maps: the share of the structured cells
    of the last frame that hold a live track, with re-seeding and from the seeds of frame 0 alone.  Printed, not asserted."""
    nx, ny, nscales = 131, 77, 4
    F = synth.sequence(nx, ny, 5)
    steps, maps = [], []
    for t in range(4):
        fw = fcons.payload(*orc.tvl1_multiscale(F[t], F[t + 1], nscales=nscales)[:2])
        bw = fcons.payload(*orc.tvl1_multiscale(F[t + 1], F[t], nscales=nscales)[:2])
        steps.append(fw)
        maps.append(fcons.maps(orc, fw, bw, 0.01, 0.5)[0])
    frac = 0.1
    for reseed in (True, False):
        res = R.sequence(orc, list(F), steps, maps, 100000, R.RHO, frac, R.STEP, reseed)
        l2, mean = res["structure"][4]
        st = set(R.structured(l2, mean, frac, R.STEP))
        live = (res["t0"] <= 4) & (res["t0"] + res["len"] >= 4)
        held = R.occupied(res["xy"][4][live], nx, ny, R.STEP) & st
        print("131x77, 5 frames, frac 0.1, step 4, %s: %d tracks, %d live at the last frame, %.1f %% of its %d structured cells hold one"
              % ("re-seeded" if reseed else "frame-0 seeds only", len(res["t0"]), int(live.sum()), 100.0 * len(held) / len(st), len(st)))
