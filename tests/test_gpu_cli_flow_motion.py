"""The front-end flow_motion prints, for a 67x35 flow, the record of ofx_flow_motion_fit_dev as %.17g prints it and writes the entry's
residual payload, model payload and inlier map byte for byte, with and without a map."""
import ctypes.util
import os

import numpy as np
import pytest

import flow_motion_ref as R
from test_gpu_cli_flow_compose import read_flo, read_pgm, run, write_flo, write_pgm

pytestmark = pytest.mark.gpu

NX, NY = 67, 35


def library(gpu64, flo, occ, model, n_fits, c_first, c_last):
    import torch
    f = torch.from_numpy(np.ascontiguousarray(flo)).cuda()
    m = None if occ is None else torch.from_numpy(np.ascontiguousarray(occ)).cuda()
    rec = torch.zeros(16, dtype=torch.float64, device="cuda")
    out = torch.zeros((2, NY, NX, 2), dtype=torch.float32, device="cuda")
    inl = torch.zeros((NY, NX), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu64.flow_motion_fit_dev([f.data_ptr()], [rec.data_ptr()], NX, NY, model=model, n_fits=n_fits, c_first=c_first, c_last=c_last,
                              d_occ=None if m is None else [m.data_ptr()], d_flo_model=[out[0].data_ptr()],
                              d_flo_resid=[out[1].data_ptr()], d_inlier=[inl.data_ptr()])
    gpu64.synchronize()
    return rec.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy(), inl.cpu().numpy()


def printed(stdout):
    rows = {line.split()[0]: [float(x) for x in line.split()[1:]] for line in stdout.splitlines()}
    return np.array(rows["theta"] + rows["pixel"] + rows["fit"])


def test_flow_motion_prints_the_record_and_writes_the_librarys_bytes(gpu64, tmp_path):
    flo, fg = R.scene(NX, NY)
    occ = R.flags(NX, NY)
    name, mname = tmp_path / "in.flo", tmp_path / "occ.pgm"
    write_flo(name, flo)
    write_pgm(mname, occ)
    for tag, m, margs, model, word in (("plain", None, (), R.AFFINE, "affine"), ("map", occ, (mname,), R.SIMILARITY, "4")):
        prefix = str(tmp_path / tag)
        r = run("flow_motion", "-o", prefix, "-x", "pgm", name, word, 9, 16, 1, *margs)
        assert r.returncode == 0, r.stderr
        rec, mdl, res, inl = library(gpu64, flo, m, model, 9, 16.0, 1.0)
        assert printed(r.stdout).tobytes() == rec.tobytes(), tag
        assert read_flo(prefix + "_resid.flo").tobytes() == res.tobytes(), tag
        assert read_flo(prefix + "_model.flo").tobytes() == mdl.tobytes(), tag
        assert read_pgm(prefix + "_inlier.pgm", NX, NY).tobytes() == inl.tobytes(), tag
        want = R.fit(flo, m, model, 9, 16.0, 1.0)
        assert rec.tobytes() == want.tobytes() and inl.tobytes() == R.outputs(want[:6], 1.0, flo, m)[2].tobytes(), tag
    assert R.mean_epe(rec[:6], R.TRUE[R.AFFINE], NX, NY) < 1.0 and (inl[fg] == 255).all()
    # the default names and extension: beside the input, PNG where the system has libpng16 (the front-ends bind it at run time)
    if ctypes.util.find_library("png16") or os.path.exists("/lib/x86_64-linux-gnu/libpng16.so.16"):
        r = run("flow_motion", name, "translation", 2, 16, 4)
        assert r.returncode == 0, r.stderr
        assert open(tmp_path / "in_inlier.png", "rb").read()[:8] == b"\x89PNG\r\n\x1a\n"
        assert read_flo(tmp_path / "in_model.flo").tobytes() == R.model_payload(R.fit(flo, None, R.TRANSLATION, 2, 16.0, 4.0)[:6], NX, NY).tobytes()
    # refusals before the GPU is touched
    r = run("flow_motion", name, "affine", 9, 16)
    assert r.returncode == 1 and "Usage" in r.stderr
    r = run("flow_motion", name, "projective", 9, 16, 1)
    assert r.returncode == 1 and "Usage" in r.stderr
    r = run("flow_motion", "-o", tmp_path / "x", tmp_path / "missing.flo", "affine", 9, 16, 1)
    assert r.returncode == 1 and "could not read" in r.stderr
    small = tmp_path / "small.pgm"
    write_pgm(small, occ[:-1])
    r = run("flow_motion", "-o", tmp_path / "x", name, "affine", 9, 16, 1, small)
    assert r.returncode == 1 and "mismatch" in r.stderr
    # ... and the library's own, passed on
    r = run("flow_motion", "-o", tmp_path / "x", name, "affine", 9, 1, 16)
    assert r.returncode == 1 and "c_last" in r.stderr
    assert not os.path.exists(str(tmp_path / "x") + "_resid.flo")
