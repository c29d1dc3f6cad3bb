"""ofx_brox_temporal_dev / ofx_brox_temporal_batch_dev in the public surface: header, library export, Python mirror (CPU only)."""
import ctypes
import inspect
import os
import re

from conftest import require_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOLVER = ["int nxx", "int nyy", "double alpha", "double gamma", "int nscales", "double nu", "double TOL", "int inner_iter",
          "int outer_iter"]
DEV = ["ofx_ctx *ctx", "int frames", "const void *const *dF", "void *const *d_flo"] + SOLVER
BATCH = ["ofx_ctx *const *ctxs", "int n_ctx", "int n_seq", "int frames", "const void *const *dF", "void *const *d_flo"] + SOLVER + \
        ["double *work_pix_iters"]
KEYS = ("alpha", "gamma", "nscales", "nu", "TOL", "inner", "outer")


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def _declared(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "%s is not declared in include/ofx.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    assert _declared("ofx_brox_temporal_dev") == DEV
    assert _declared("ofx_brox_temporal_batch_dev") == BATCH
    assert int(re.search(r"#define\s+OFX_BROXT_MAX_FRAMES\s+(\d+)", _header()).group(1)) == 32
    # the host entry keeps its argument list
    assert _declared("ofx_brox_temporal")[:7] == ["ofx_ctx *ctx", "const double *I", "double *u", "double *v", "int nxx", "int nyy",
                                                  "int frames"]


def test_version_is_still_102():
    assert int(re.search(r"#define\s+OFX_VERSION\s+(\d+)", _header()).group(1)) == 102


def test_library_exports_the_entries():
    so = os.path.join(ROOT, "optical-flow-1_amd", "libofx.so")
    require_or_skip(os.path.exists(so), "optical-flow-1_amd/libofx.so not built")
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ofx_brox_temporal_dev") and hasattr(lib, "ofx_brox_temporal_batch_dev")


def test_python_mirror_binds_the_entries(ofx_mod):
    L = ofx_mod.lib()
    assert L.ofx_missing == []
    assert len(L.ofx_brox_temporal_dev.argtypes) == len(DEV)
    assert len(L.ofx_brox_temporal_batch_dev.argtypes) == len(BATCH)
    dev = list(inspect.signature(ofx_mod.Ofx.brox_temporal_dev).parameters)
    assert dev[:5] == ["self", "dF", "d_flo", "nx", "ny"] and len(dev) == 5 + len(KEYS)
    batch = list(inspect.signature(ofx_mod.brox_temporal_batch_dev).parameters)
    assert batch[:6] == ["ctxs", "dF", "d_flo", "nx", "ny", "frames"] and len(batch) == 6 + len(KEYS)
    # the defaults of the host entry
    want = [inspect.signature(ofx_mod.Ofx.brox_temporal).parameters[k].default for k in KEYS]
    for fn in (ofx_mod.Ofx.brox_temporal_dev, ofx_mod.brox_temporal_batch_dev):
        assert [inspect.signature(fn).parameters[k].default for k in KEYS] == want
