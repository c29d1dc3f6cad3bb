"""The front-ends horn_schunck_seq and brox_seq: the .flo files along a video are byte for byte the payloads of
ofx_hs_sequence_group_dev / ofx_brox_sequence_group_dev under the front-ends' defaults and their own auto-nscales rules."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "optical-flow-1_amd", "bin")
NX, NY = 67, 45


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.astype(np.uint8).tobytes())


def run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True, env=e)


@pytest.fixture()
def video(synth, tmp_path):
    frames = [np.floor(f) for f in synth.sequence(NX, NY, 3)]            # what a PGM holds
    names = []
    for t, f in enumerate(frames):
        assert f.min() >= 0 and f.max() <= 255
        names.append(tmp_path / ("f%d.pgm" % t))
        write_pgm(names[-1], f)
    return frames, names


def _check(tmp_path, want):
    for t in range(2):
        raw = open(tmp_path / ("out_%04d.flo" % t), "rb").read()
        assert raw[:4] == b"PIEH" and tuple(np.frombuffer(raw[4:12], dtype=np.uint32)) == (NX, NY)
        assert raw[12:] == want[t].tobytes(), t
    assert not (tmp_path / "out_0002.flo").exists()
    assert want[1].tobytes() != want[0].tobytes() and np.isfinite(want).all()


def _chain(ctx, entry, frames, **kw):
    import torch
    F = [torch.from_numpy(f).cuda() for f in frames]
    flo = torch.zeros((2, NY, NX, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    entry([[t.data_ptr() for t in F]], [[flo[0].data_ptr(), flo[1].data_ptr()]], NX, NY, **kw)
    ctx.synchronize()
    return flo.cpu().numpy()


def test_horn_schunck_seq(gpu64, video, tmp_path):
    """1 + log2(hypot(67, 45) / 16) = 3.3: 5 scales asked for become 3"""
    frames, names = video
    r = run("horn_schunck_seq", tmp_path / "out_", 5, 1, *names)
    assert r.returncode == 0, r.stderr
    _check(tmp_path, _chain(gpu64, gpu64.hs_sequence_group_dev, frames, nscales_first=3, nscales_next=1))


def test_brox_seq(gpu64, video, tmp_path):
    """(int) (1 + log2(min(67, 45) / 16)) = 2: Brox's own rule, on the smaller side"""
    frames, names = video
    r = run("brox_seq", tmp_path / "out_", 3, 1, *names)
    assert r.returncode == 0, r.stderr
    _check(tmp_path, _chain(gpu64, gpu64.brox_sequence_group_dev, frames, nscales_first=2, nscales_next=1))


def test_horn_schunck_seq_in_tolerance_mode(gpu64, video, tmp_path):
    frames, names = video
    r = run("horn_schunck_seq", tmp_path / "out_", 3, 2, *names, env={"OFX_SOR_TOLERANCE": "1"})
    assert r.returncode == 0, r.stderr
    exact = _chain(gpu64, gpu64.hs_sequence_group_dev, frames, nscales_first=3, nscales_next=2)
    gpu64.set_option("sor_exact", 0)
    try:
        want = _chain(gpu64, gpu64.hs_sequence_group_dev, frames, nscales_first=3, nscales_next=2)
    finally:
        gpu64.set_option("sor_exact", 1)
    _check(tmp_path, want)
    assert want.tobytes() != exact.tobytes()                             # the variable does reach the solve


@pytest.mark.parametrize("prog", ["horn_schunck_seq", "brox_seq"])
def test_usage_and_bad_files(prog, tmp_path):
    r = run(prog, tmp_path / "out_", 3, 1, tmp_path / "only_one.pgm")
    assert r.returncode != 0 and "Usage" in r.stderr
    write_pgm(tmp_path / "a.pgm", np.zeros((20, 30)))
    write_pgm(tmp_path / "b.pgm", np.zeros((30, 20)))
    r = run(prog, tmp_path / "out_", 3, 1, tmp_path / "a.pgm", tmp_path / "b.pgm")
    assert r.returncode != 0 and "mismatch" in r.stderr
    r = run(prog, tmp_path / "out_", 3, 1, tmp_path / "a.pgm", tmp_path / "missing.pgm")
    assert r.returncode != 0 and "could not read" in r.stderr
    assert not (tmp_path / "out_0000.flo").exists()
