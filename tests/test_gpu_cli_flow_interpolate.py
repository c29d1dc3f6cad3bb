"""The front-end flow_interpolate: on P5 and P6 frames it writes the bytes of the restatement (tests/flow_apply_ref.py), from pinned
payloads and from what tvl1flow_fb writes; its three error exits return status 1."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import flow_apply_ref as far

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "optical-flow-1_amd", "bin")
T = 3.0 / 7.0


def write_pnm(path, img, maxval=255):
    """(ny, nx, 1 | 3) -> P5 | P6; two big-endian bytes per sample above 255"""
    ny, nx, c = img.shape
    with open(path, "wb") as f:
        f.write(b"P%d\n%d %d\n%d\n" % (5 if c == 1 else 6, nx, ny, maxval))
        f.write(img.astype(np.uint8).tobytes() if maxval < 256 else img.astype(">u2").tobytes())


def read_pnm(path):
    raw = open(path, "rb").read()
    tok = raw.split(None, 4)
    c = {b"P5": 1, b"P6": 3}[tok[0]]
    w, h, maxval = int(tok[1]), int(tok[2]), int(tok[3])
    assert maxval == 255
    return np.frombuffer(raw[len(raw) - w * h * c:], dtype=np.uint8).reshape(h, w, c)


def write_flo(path, flo):
    with open(path, "wb") as f:
        f.write(b"PIEH" + np.array([flo.shape[1], flo.shape[0]], dtype=np.uint32).tobytes() + np.ascontiguousarray(flo).tobytes())


def read_flo(path):
    raw = open(path, "rb").read()
    w, h = (int(x) for x in np.frombuffer(raw[4:12], dtype=np.uint32))
    return np.frombuffer(raw[12:], dtype=np.float32).reshape(h, w, 2)


def write_png_gray_alpha(path, nx, ny):
    """an 8-bit gray + alpha PNG (two channels), no filter"""
    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    rows = b"".join(b"\x00" + bytes([(7 * i + j) % 256 for j in range(2 * nx)]) for i in range(ny))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", nx, ny, 8, 4, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows))
                + chunk(b"IEND", b""))


def run(*args):
    return subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True)


@pytest.mark.parametrize("nz", [1, 3])
def test_writes_the_restatements_bytes(orc, synth, tmp_path, nz):
    name = "p1_37x29"
    A, B = far.frames(synth, name, nz, "u8")
    fwd, bwd = far.payloads(orc, synth, name)
    a, b, f, w, out = (tmp_path / n for n in ("a.pnm", "b.pnm", "fwd.flo", "bwd.flo", "out.pnm"))
    write_pnm(a, A)
    write_pnm(b, B)
    write_flo(f, fwd)
    write_flo(w, bwd)
    r = run("flow_interpolate", a, b, f, w, out, repr(T))
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read().startswith(b"P5" if nz == 1 else b"P6")
    assert np.array_equal(read_pnm(out), far.want_interp(orc, synth, name, nz, "u8", T))
    r = run("flow_interpolate", a, b, f, w, out)                     # t = 0.5 by default
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_pnm(out), far.interpolate(orc, A, B, fwd, bwd, 0.5))
    r = run("flow_interpolate", a, b, f, w, out, "1.5")              # the library's refusal reaches the exit status
    assert r.returncode == 1 and "outside [0, 1]" in r.stderr


def test_consumes_what_tvl1flow_fb_writes(orc, synth, tmp_path):
    A, B = far.frames(synth, "p1_64x48", 1, "u8")
    a, b, out = tmp_path / "a.pgm", tmp_path / "b.pgm", tmp_path / "mid.pgm"
    write_pnm(a, A)
    write_pnm(b, B)
    names = [tmp_path / n for n in ("fwd.flo", "bwd.flo", "occ_fwd.pgm", "occ_bwd.pgm")]
    r = run("tvl1flow_fb", a, b, *names)
    assert r.returncode == 0, r.stderr
    r = run("flow_interpolate", a, b, names[0], names[1], out, repr(T))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_pnm(out), far.interpolate(orc, A, B, read_flo(names[0]), read_flo(names[1]), T))


def test_error_exits(orc, synth, tmp_path):
    nx, ny = 37, 29
    A, B = far.frames(synth, "p1_37x29", 1, "u8")
    fwd, bwd = far.payloads(orc, synth, "p1_37x29")
    a, b, f, w, out = (tmp_path / n for n in ("a.pgm", "b.pgm", "fwd.flo", "bwd.flo", "out.pgm"))
    write_pnm(a, A)
    write_pnm(b, B)
    write_flo(f, fwd)
    write_flo(w, bwd)
    # samples that are not bytes
    deep = tmp_path / "deep.pgm"
    write_pnm(deep, A.astype(np.uint16) + 300, maxval=65535)
    r = run("flow_interpolate", deep, b, f, w, out)
    assert r.returncode == 1 and "not a byte" in r.stderr, r.stderr
    # a channel count other than 1 or 3 (a gray + alpha PNG; without the system's libpng the file is unreadable: status 1 as well)
    ga = tmp_path / "ga.png"
    write_png_gray_alpha(ga, nx, ny)
    r = run("flow_interpolate", ga, b, f, w, out)
    assert r.returncode == 1 and ("2 channels" in r.stderr or "could not read" in r.stderr), r.stderr
    # size mismatches: the frames, a payload, the channel counts
    small = tmp_path / "small.pgm"
    write_pnm(small, A[:ny - 1])
    r = run("flow_interpolate", a, small, f, w, out)
    assert r.returncode == 1 and "differ" in r.stderr, r.stderr
    short = tmp_path / "short.flo"
    write_flo(short, bwd[:ny - 1])
    r = run("flow_interpolate", a, b, f, short, out)
    assert r.returncode == 1 and "do not match" in r.stderr, r.stderr
    rgb = tmp_path / "rgb.ppm"
    write_pnm(rgb, far.frames(synth, "p1_37x29", 3, "u8")[1])
    r = run("flow_interpolate", a, rgb, f, w, out)
    assert r.returncode == 1 and "differ" in r.stderr, r.stderr
    r = run("flow_interpolate", a, b, f, tmp_path / "missing.flo", out)
    assert r.returncode == 1 and "could not read" in r.stderr, r.stderr
    r = run("flow_interpolate", a, b)
    assert r.returncode == 1 and "Usage" in r.stderr
    assert not out.exists()
