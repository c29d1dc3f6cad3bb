"""The front-end tvl1flow_seq: the .flo files along a video are byte for byte the payloads of ofx_tvl1_sequence_group_dev."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "optical-flow-1_amd", "bin")


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.astype(np.uint8).tobytes())


def run(*args):
    return subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True)


def test_three_frames(gpu64, synth, tmp_path):
    import torch
    nx, ny, nscales_first, nscales_next = 67, 45, 3, 1
    frames = [np.floor(f) for f in synth.sequence(nx, ny, 3)]             # what a PGM holds
    names = []
    for t, f in enumerate(frames):
        assert f.min() >= 0 and f.max() <= 255
        names.append(tmp_path / ("f%d.pgm" % t))
        write_pgm(names[-1], f)
    r = run("tvl1flow_seq", tmp_path / "out_", nscales_first, nscales_next, *names)
    assert r.returncode == 0, r.stderr

    F = [torch.from_numpy(f).cuda() for f in frames]
    flo = torch.zeros((2, ny, nx, 2), dtype=torch.float32, device="cuda")
    gpu64.tvl1_sequence_group_dev([[t.data_ptr() for t in F]], [[flo[0].data_ptr(), flo[1].data_ptr()]], nx, ny,
                                  nscales_first=nscales_first, nscales_next=nscales_next)
    gpu64.synchronize()
    want = flo.cpu().numpy()
    for t in range(2):
        raw = open(tmp_path / ("out_%04d.flo" % t), "rb").read()
        assert raw[:4] == b"PIEH" and tuple(np.frombuffer(raw[4:12], dtype=np.uint32)) == (nx, ny)
        assert raw[12:] == want[t].tobytes(), t
    assert not (tmp_path / "out_0002.flo").exists()
    assert want[1].tobytes() != want[0].tobytes() and np.isfinite(want).all()


def test_usage_and_bad_files(tmp_path):
    r = run("tvl1flow_seq", tmp_path / "out_", 3, 1, tmp_path / "only_one.pgm")
    assert r.returncode != 0 and "Usage" in r.stderr
    write_pgm(tmp_path / "a.pgm", np.zeros((20, 30)))
    write_pgm(tmp_path / "b.pgm", np.zeros((30, 20)))
    r = run("tvl1flow_seq", tmp_path / "out_", 3, 1, tmp_path / "a.pgm", tmp_path / "b.pgm")
    assert r.returncode != 0 and "mismatch" in r.stderr
    r = run("tvl1flow_seq", tmp_path / "out_", 3, 1, tmp_path / "a.pgm", tmp_path / "missing.pgm")
    assert r.returncode != 0 and "could not read" in r.stderr
    assert not (tmp_path / "out_0000.flo").exists()
