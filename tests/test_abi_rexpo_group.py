"""ofx_robust_expo_group_dev / ofx_robust_expo_batch_dev in the public surface: header, library export, Python mirror (CPU only)."""
import ctypes
import inspect
import os
import re

from conftest import require_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOLVER = ["int nxx", "int nyy", "int nzz", "int method_type", "double alpha", "double gamma", "double lambda", "int nscales", "double nu",
          "double TOL", "int inner_iter", "int outer_iter"]
GROUP = ["ofx_ctx *ctx", "int n_pairs", "const void *const *dI1", "const void *const *dI2", "void *const *d_flo"] + SOLVER + \
        ["ofx_stats *stats_out"]
BATCH = ["ofx_ctx *const *ctxs", "int n_ctx", "const void *const *dI1", "const void *const *dI2", "void *const *d_flo",
         "int n_pairs"] + SOLVER + ["double *work_pix_iters"]


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def _declared(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "%s is not declared in include/ofx.h" % name
    return [_norm(a) for a in m.group(1).split(",")]


def test_header_declares_the_group_and_batch_entries():
    assert _declared("ofx_robust_expo_group_dev") == GROUP
    assert _declared("ofx_robust_expo_batch_dev") == BATCH
    # the f32 contract is stated where the entries are declared
    assert "exactly representable in float" in _header()


def test_expo_host_ms_is_declared_exported_and_wrapped(ofx_mod):
    """the third entry of version 102: the host time of the expo stage, read by tools/bench_rexpo_batch.py for its budget"""
    assert re.search(r"double\s+ofx_ctx_expo_host_ms\s*\(\s*const ofx_ctx \*ctx\s*\)\s*;", _header())
    L = ofx_mod.lib()
    assert "ofx_ctx_expo_host_ms" not in L.ofx_missing
    assert L.ofx_ctx_expo_host_ms.restype is ctypes.c_double and len(L.ofx_ctx_expo_host_ms.argtypes) == 1
    assert L.ofx_ctx_expo_host_ms(None) == 0.0           # no context: 0, no fault
    assert list(inspect.signature(ofx_mod.Ofx.expo_host_ms).parameters) == ["self"]


def test_version_is_102():
    assert int(re.search(r"#define\s+OFX_VERSION\s+(\d+)", _header()).group(1)) == 102


def test_library_exports_the_group_and_batch_entries():
    so = os.path.join(ROOT, "optical-flow-1_amd", "libofx.so")
    require_or_skip(os.path.exists(so), "optical-flow-1_amd/libofx.so not built")
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ofx_robust_expo_group_dev") and hasattr(lib, "ofx_robust_expo_batch_dev")


def test_python_wrappers_match_the_argument_lists(ofx_mod):
    L = ofx_mod.lib()
    assert len(L.ofx_robust_expo_group_dev.argtypes) == len(GROUP)
    assert len(L.ofx_robust_expo_batch_dev.argtypes) == len(BATCH)
    # the wrappers take the three pointer lists and the solver's arguments; _group_call / _batch_call add the context(s), the
    # pair count and the record array
    group = list(inspect.signature(ofx_mod.Ofx.robust_expo_group_dev).parameters)
    assert group[:7] == ["self", "dI1", "dI2", "d_flo", "nx", "ny", "nz"] and len(group) == 4 + len(SOLVER)
    batch = list(inspect.signature(ofx_mod.robust_expo_batch_dev).parameters)
    assert batch[:7] == ["ctxs", "dI1", "dI2", "d_flo", "nx", "ny", "nz"] and len(batch) == 4 + len(SOLVER)
    for fn in (ofx_mod.Ofx.robust_expo_group_dev, ofx_mod.robust_expo_batch_dev):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("method", "alpha", "gamma", "lam", "nscales", "nu", "TOL", "inner", "outer")] == \
               [inspect.signature(ofx_mod.Ofx.robust_expo_pyramid).parameters[k].default
                for k in ("method", "alpha", "gamma", "lam", "nscales", "nu", "TOL", "inner", "outer")]
