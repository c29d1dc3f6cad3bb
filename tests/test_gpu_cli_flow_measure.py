"""The front-end flow_error prints, for a 67x35 flow, the record of ofx_flow_error_dev, the outlier rates and the percentiles as the
numpy restatement gives them; flow_color writes the colour wheel's bytes under the three-way rule; exit statuses."""
import os

import numpy as np
import pytest

import flow_measure_ref as R
from test_gpu_cli_flow_compose import run, write_flo, write_pgm

pytestmark = pytest.mark.gpu

NX, NY = 67, 35
NAMES = ("R0.5", "R1", "R2", "R3", "R5", "Fl")


def printed(stdout):
    return {line.split()[0]: float(line.split()[1]) for line in stdout.splitlines()}


def check_lines(got, flo, gt, occ, bin_w, n_bins):
    rec, _, hist = R.error(flo, gt, occ, R.THR_ABS, R.THR_REL, n_bins, bin_w)
    assert [got["known"], got["bad"], got["AEPE"], got["RMS"], got["max"]] == [rec[0], rec[1], rec[2], rec[3], rec[5]]
    assert abs(got["AAE"] - rec[4]) <= 1e-12 * rec[4]
    for k, name in enumerate(NAMES):
        assert got[name] == rec[8 + k] / rec[0], name
    for name, p in (("A50", 0.5), ("A75", 0.75), ("A95", 0.95)):
        assert got[name] == R.percentile_edge(hist, rec[0], p, bin_w), name
    return rec


def test_flow_error_prints_the_restatements_figures(tmp_path):
    gt, flo = R.spoiled(R.truth(NX, NY), 1), R.spoiled(R.estimate(NX, NY), 2)
    occ = R.flags(NX, NY)
    est, truth, mname = tmp_path / "est.flo", tmp_path / "gt.flo", tmp_path / "occ.pgm"
    write_flo(est, flo)
    write_flo(truth, gt)
    write_pgm(mname, occ)
    r = run("flow_error", est, truth)
    assert r.returncode == 0, r.stderr
    rec = check_lines(printed(r.stdout), flo, gt, None, 1.0 / 64, 4096)
    assert 0 < rec[1] < rec[0] < NX * NY and [line.split()[0] for line in r.stdout.splitlines()] == [
        "known", "bad", "AEPE", "RMS", "AAE", "max"] + list(NAMES) + ["A50", "A75", "A95"]
    r = run("flow_error", est, truth, mname)
    assert r.returncode == 0, r.stderr
    check_lines(printed(r.stdout), flo, gt, occ, 1.0 / 64, 4096)
    r = run("flow_error", est, truth, mname, 0.25, 8)
    assert r.returncode == 0, r.stderr
    check_lines(printed(r.stdout), flo, gt, occ, 0.25, 8)
    r = run("flow_error", est, truth, 0.5, 3)
    assert r.returncode == 0, r.stderr
    check_lines(printed(r.stdout), flo, gt, None, 0.5, 3)
    # refusals before the GPU is touched
    r = run("flow_error", est)
    assert r.returncode == 1 and "Usage" in r.stderr
    r = run("flow_error", est, truth, 0.5)
    assert r.returncode == 1 and "Usage" in r.stderr
    r = run("flow_error", est, tmp_path / "missing.flo")
    assert r.returncode == 1 and "could not read" in r.stderr
    small = tmp_path / "small.flo"
    write_flo(small, gt[:-1])
    r = run("flow_error", est, small)
    assert r.returncode == 1 and "mismatch" in r.stderr
    smap = tmp_path / "small.pgm"
    write_pgm(smap, occ[:-1])
    r = run("flow_error", est, truth, smap)
    assert r.returncode == 1 and "mismatch" in r.stderr
    # ... and the library's own, passed on
    r = run("flow_error", est, truth, 0.0, 8)
    assert r.returncode == 1 and "bin_w" in r.stderr and r.stdout == ""
    r = run("flow_error", est, truth, 0.5, 70000)
    assert r.returncode == 1 and "n_bins" in r.stderr


def read_ppm(path, nx, ny):
    raw = open(path, "rb").read()
    assert raw[:2] == b"P6" and raw.split()[1:4] == [b"%d" % nx, b"%d" % ny, b"255"]
    return np.frombuffer(raw[len(raw) - 3 * nx * ny:], dtype=np.uint8).reshape(ny, nx, 3)


def test_flow_color_writes_the_wheel(tmp_path):
    flo = R.spoiled(R.truth(NX, NY), 5)
    occ = R.flags(NX, NY)
    name, mname, out = tmp_path / "in.flo", tmp_path / "occ.pgm", tmp_path / "out.ppm"
    write_flo(name, flo)
    write_pgm(mname, occ)
    for args, m, scale in (((), None, 0.0), ((4,), None, 4.0), ((0, mname), occ, 0.0), ((2.5, mname), occ, 2.5)):
        if os.path.exists(out):
            os.remove(out)
        r = run("flow_color", name, out, *args)
        assert r.returncode == 0, r.stderr
        got = read_ppm(out, NX, NY)
        ok, exempt = R.wheel_ok(got, flo, m, scale)
        assert ok and exempt <= 0.01 * NX * NY, (args, exempt)
        assert not got[~R.vis(flo, m)].any()
    r = run("flow_color", name)
    assert r.returncode == 1 and "Usage" in r.stderr
    r = run("flow_color", tmp_path / "missing.flo", out)
    assert r.returncode == 1 and "could not read" in r.stderr
    smap = tmp_path / "small.pgm"
    write_pgm(smap, occ[:-1])
    r = run("flow_color", name, out, 0, smap)
    assert r.returncode == 1 and "mismatch" in r.stderr
    r = run("flow_color", name, tmp_path / "no.ppm", -1)
    assert r.returncode == 1 and "scale" in r.stderr and not os.path.exists(tmp_path / "no.ppm")
