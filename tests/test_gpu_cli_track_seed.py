"""The front-end flow_tracks writes, for a 64x48 clip of four frames, the tracks of the restatement (tests/track_seed_ref.py): t0, len
and every position as %.17g prints it, with and without step maps as flow_consistency writes them."""
import os

import numpy as np
import pytest

import flow_compose_ref as fcr
import flow_consistency_ref as fcons
import track_seed_ref as R
from test_gpu_cli_flow_compose import run, write_flo, write_pgm

pytestmark = pytest.mark.gpu

NX, NY, FRAMES = 64, 48, 4


def read_tracks(path):
    rows = [line.split() for line in open(path).read().splitlines()]
    t0 = np.array([int(r[0]) for r in rows], dtype=np.int32)
    ln = np.array([int(r[1]) for r in rows], dtype=np.int32)
    xy = np.array([[float(v) for v in r[2:]] for r in rows], dtype=np.float64).reshape(len(rows), FRAMES, 2)
    return t0, ln, np.ascontiguousarray(xy.transpose(1, 0, 2))


def test_flow_tracks_writes_the_restatements_tracks(orc, tmp_path):
    up, vals = R.clip(NX, NY, FRAMES)
    pairs = [fcr.noise_step(NX, NY, 1.5, 71 + t) for t in range(FRAMES - 1)]
    steps = [p[0] for p in pairs]
    maps = [fcons.maps(orc, f, b, fcr.STEP_ALPHA, fcr.STEP_BETA)[0] for f, b in pairs]
    frac = R.pick_frac(orc, vals)
    fn = [tmp_path / ("f%d.pgm" % t) for t in range(FRAMES)]
    sn = [tmp_path / ("s%d.flo" % t) for t in range(FRAMES - 1)]
    mn = [tmp_path / ("m%d.pgm" % t) for t in range(FRAMES - 1)]
    for t in range(FRAMES):
        write_pgm(fn[t], up[t])
    for t in range(FRAMES - 1):
        write_flo(sn[t], steps[t])
        write_pgm(mn[t], maps[t])
    for tag, ms, margs, cap in (("plain", None, (), 100000), ("maps", maps, ("-m", *mn), 100000), ("cap", maps, ("-m", *mn), 120)):
        out = tmp_path / (tag + ".txt")
        r = run("flow_tracks", "-f", repr(frac), "-s", R.STEP, "-r", R.RHO, "-c", cap, out, *fn, *sn, *margs)
        assert r.returncode == 0, r.stderr
        want = R.sequence(orc, list(vals), steps, ms, cap, R.RHO, frac, R.STEP)
        t0, ln, xy = read_tracks(out)
        assert len(t0) == want["count"][0] > 50
        assert np.array_equal(t0, want["t0"]) and np.array_equal(ln, want["len"]) and xy.tobytes() == want["xy"].tobytes(), tag
        assert ("dropped" in r.stderr) == (want["count"][1] > 0)
    assert want["count"][1] > 0 and (want["t0"] > 0).any()
    # refusals before the GPU is touched
    r = run("flow_tracks", tmp_path / "x.txt", *fn, *sn[:-1])
    assert r.returncode == 1 and "Usage" in r.stderr
    r = run("flow_tracks", tmp_path / "x.txt", *fn, *sn, "-m", mn[0])
    assert r.returncode == 1 and "Usage" in r.stderr
    r = run("flow_tracks", tmp_path / "x.txt", *fn[:-1], tmp_path / "missing.pgm", *sn)
    assert r.returncode == 1 and "could not read" in r.stderr
    small = tmp_path / "small.pgm"
    write_pgm(small, maps[0][:-1])
    r = run("flow_tracks", tmp_path / "x.txt", *fn, *sn, "-m", small, *mn[1:])
    assert r.returncode == 1 and "mismatch" in r.stderr
    # ... and the library's own, passed on
    r = run("flow_tracks", "-r", 0, tmp_path / "x.txt", *fn, *sn)
    assert r.returncode == 1 and "rho" in r.stderr
    assert not os.path.exists(tmp_path / "x.txt")
