"""The front-ends tvl1flow_fb and flow_consistency: the .flo files are byte-identical to tvl1flow's in either direction, the maps
are the restatement's (tests/flow_consistency_ref.py) on those payloads, whichever of the two programs wrote them."""
import os
import subprocess

import numpy as np
import pytest

import flow_consistency_ref as fcr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "optical-flow-1_amd", "bin")


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.astype(np.uint8).tobytes())


def read_pgm(path):
    raw = open(path, "rb").read()
    tok = raw.split(None, 4)
    w, h, maxval = int(tok[1]), int(tok[2]), int(tok[3])
    assert maxval == 255
    if tok[0] == b"P2":
        a = np.array(raw.split()[4:], dtype=np.int64)
    else:
        assert tok[0] == b"P5"
        a = np.frombuffer(raw[len(raw) - w * h:], dtype=np.uint8)
    assert a.size == w * h
    return a.reshape(h, w).astype(np.uint8)


def run(*args):
    return subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True)


def test_front_ends(orc, synth, tmp_path):
    nx, ny = 64, 48
    I0, I1 = synth.pair("P1", nx, ny)
    a, b = tmp_path / "a.pgm", tmp_path / "b.pgm"
    write_pgm(a, I0)
    write_pgm(b, I1)
    r = run("tvl1flow", a, b, tmp_path / "ab.flo")
    assert r.returncode == 0, r.stderr
    r = run("tvl1flow", b, a, tmp_path / "ba.flo")
    assert r.returncode == 0, r.stderr
    names = [tmp_path / n for n in ("fwd.flo", "bwd.flo", "occ_fwd.pgm", "occ_bwd.pgm")]
    r = run("tvl1flow_fb", a, b, *names)
    assert r.returncode == 0, r.stderr
    assert open(names[0], "rb").read() == open(tmp_path / "ab.flo", "rb").read()
    assert open(names[1], "rb").read() == open(tmp_path / "ba.flo", "rb").read()

    raw = open(names[0], "rb").read()
    assert raw[:4] == b"PIEH" and tuple(np.frombuffer(raw[4:12], dtype=np.uint32)) == (nx, ny)
    fwd = np.frombuffer(raw[12:], dtype=np.float32).reshape(ny, nx, 2)
    bwd = np.frombuffer(open(names[1], "rb").read()[12:], dtype=np.float32).reshape(ny, nx, 2)
    want_f, want_b, margin = fcr.maps(orc, fwd, bwd)
    share = float((want_f == 255).mean())
    print("share of 255 forward %.3f, margin %.3g" % (share, margin))
    assert 0.05 <= share <= 0.95 and margin > 1e-9
    assert np.array_equal(read_pgm(names[2]), want_f) and np.array_equal(read_pgm(names[3]), want_b)

    # the same maps from the two files alone
    r = run("flow_consistency", names[0], names[1], tmp_path / "cf.pgm", tmp_path / "cb.pgm")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_pgm(tmp_path / "cf.pgm"), want_f) and np.array_equal(read_pgm(tmp_path / "cb.pgm"), want_b)
    # other thresholds reach the entry: alpha = 0, beta = 0 passes nothing but exact inverses
    r = run("flow_consistency", names[0], names[1], tmp_path / "zf.pgm", tmp_path / "zb.pgm", "0", "0")
    assert r.returncode == 0, r.stderr
    zf, zb, _ = fcr.maps(orc, fwd, bwd, 0.0, 0.0)
    assert np.array_equal(read_pgm(tmp_path / "zf.pgm"), zf) and np.array_equal(read_pgm(tmp_path / "zb.pgm"), zb)


def test_flow_consistency_refuses_bad_files(tmp_path):
    def write_flo(path, w, h):
        with open(path, "wb") as f:
            f.write(b"PIEH" + np.array([w, h], dtype=np.uint32).tobytes() + np.zeros(w * h * 2, dtype=np.float32).tobytes())

    write_flo(tmp_path / "a.flo", 8, 6)
    write_flo(tmp_path / "b.flo", 6, 8)
    out = [tmp_path / "of.pgm", tmp_path / "ob.pgm"]
    r = run("flow_consistency", tmp_path / "a.flo", tmp_path / "b.flo", *out)
    assert r.returncode != 0 and "mismatch" in r.stderr
    r = run("flow_consistency", tmp_path / "a.flo", tmp_path / "missing.flo", *out)
    assert r.returncode != 0 and "could not read" in r.stderr
    r = run("flow_consistency", tmp_path / "a.flo")
    assert r.returncode != 0 and "Usage" in r.stderr
    assert not out[0].exists() and not out[1].exists()
