"""ofx_structure_texture_dev in the public surface: header, library export, Python mirror, front-end, and the PFM writer of
libofxio.so (CPU only)."""
import ctypes
import inspect
import os
import re

import numpy as np

from conftest import require_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ofx_ctx *ctx", "int n", "const void *const *dSrc", "void *const *dTex", "void *const *dStruct", "int nx", "int ny",
        "double theta", "double alpha", "int n_iter"]


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def test_header_declares_the_entry_and_the_option():
    h = _header()
    m = re.search(r"int\s+ofx_structure_texture_dev\s*\(([^)]*)\)\s*;", h)
    assert m, "ofx_structure_texture_dev is not declared in include/ofx.h"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ARGS
    assert int(re.search(r"#define\s+OFX_VERSION\s+(\d+)", h).group(1)) == 102      # an addition: the version stays
    assert '"st_fuse"' in h
    assert re.search(r"#define\s+OFX_ST_MAX_ITERS\s+\d+", h) and re.search(r"#define\s+OFX_ST_MAX_FUSE\s+\d+", h)
    for consequence in ("n_iter = 0 writes S = f, exactly", "A constant frame writes S = f and T = f - alpha * f exactly, for every n_iter",
                        'The result does not depend on "st_fuse"'):
        assert consequence in h, consequence


def test_library_exports_the_entry():
    so = os.path.join(ROOT, "optical-flow-1_amd", "libofx.so")
    require_or_skip(os.path.exists(so), "optical-flow-1_amd/libofx.so not built")
    assert hasattr(ctypes.CDLL(so), "ofx_structure_texture_dev")


def test_python_mirror_binds_it(ofx_mod):
    L = ofx_mod.lib()
    assert L.ofx_missing == []
    assert len(L.ofx_structure_texture_dev.argtypes) == len(ARGS)
    p = inspect.signature(ofx_mod.Ofx.structure_texture_dev).parameters
    assert list(p) == ["self", "dSrc", "dTex", "nx", "ny", "theta", "alpha", "n_iter", "dStruct"]
    assert (p["theta"].default, p["alpha"].default, p["n_iter"].default, p["dStruct"].default) == (16.0, 0.95, 100, None)


def test_front_end_and_unit_are_built_by_the_makefiles():
    mk = open(os.path.join(ROOT, "optical-flow-1_amd", "cli", "Makefile")).read()
    assert "structure_texture" in re.search(r"^PROGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "optical-flow-1_amd", "cli", "structure_texture.c"))
    mk = open(os.path.join(ROOT, "optical-flow-1_amd", "csrc", "Makefile")).read()
    assert "ofx_texture.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert os.path.exists(os.path.join(ROOT, "optical-flow-1_amd", "csrc", "ofx_texture.hip"))


def test_write_pfm_round_trips(tmp_path):
    so = os.path.join(ROOT, "optical-flow-1_amd", "libofxio.so")
    require_or_skip(os.path.exists(so), "optical-flow-1_amd/libofxio.so not built")
    L = ctypes.CDLL(so)
    assert hasattr(L, "ofx_write_pfm"), "libofxio.so does not export ofx_write_pfm"
    L.ofx_write_pfm.restype = ctypes.c_int
    L.ofx_write_pfm.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.ofx_read_image_double.restype = ctypes.POINTER(ctypes.c_double)
    L.ofx_read_image_double.argtypes = [ctypes.c_char_p] + [ctypes.POINTER(ctypes.c_int)] * 2
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    w, h = 5, 3
    img = np.random.default_rng(3).uniform(-40.0, 40.0, (h, w)).astype(np.float32)
    img[0, 0], img[0, 1], img[1, 2], img[2, 4] = -0.375, 1.0 / 3.0, -1e-3, 255.0
    img[1, :4] = np.frombuffer(b"\n #P\x00\x00\x80\x7f" * 2, dtype=np.float32)      # bytes that a text reader would trip over; +inf
    path = str(tmp_path / "img.pfm").encode()
    assert L.ofx_write_pfm(path, img.ctypes.data, w, h) == 0
    raw = open(path, "rb").read()
    assert raw.startswith(b"Pf\n5 3\n") and raw.endswith(img.tobytes())
    ww, hh = ctypes.c_int(), ctypes.c_int()
    p = L.ofx_read_image_double(path, ctypes.byref(ww), ctypes.byref(hh))
    assert p and (ww.value, hh.value) == (w, h)
    back = np.ctypeslib.as_array(p, shape=(h, w)).copy()
    libc.free(p)
    assert back.tobytes() == img.astype(np.float64).tobytes()            # first row first: no flip
    assert L.ofx_write_pfm(str(tmp_path / "no" / "dir.pfm").encode(), img.ctypes.data, w, h) == 1
    assert L.ofx_write_pfm(path, img.ctypes.data, 0, h) == 2
