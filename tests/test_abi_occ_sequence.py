"""ofx_tvl1occ_sequence_group_dev / ofx_tvl1occ_sequence_dev in the public surface: header, library export, Python mirror
(CPU only)."""
import ctypes
import inspect
import os
import re

from conftest import require_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOLVER = ["int nxx", "int nyy", "double lambda", "double alpha", "double beta", "double theta", "int nscales", "double zfactor",
          "int warps", "double epsilon"]
GROUP = ["ofx_ctx *ctx", "int n_frames", "const void *const *dF", "void *const *d_flo", "void *const *d_occ"] + SOLVER + \
        ["ofx_stats *stats_out"]
BATCH = ["ofx_ctx *const *ctxs", "int n_ctx", "int n_frames", "const void *const *dF", "void *const *d_flo",
         "void *const *d_occ"] + SOLVER + ["double *work_pix_iters"]


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def _declared(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "%s is not declared in include/ofx.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_the_sequence_entries():
    assert _declared("ofx_tvl1occ_sequence_group_dev") == GROUP
    assert _declared("ofx_tvl1occ_sequence_dev") == BATCH
    # what is left out is said where the entries are declared
    assert "separate filtI0" in _header()


def test_version_is_still_102():
    assert int(re.search(r"#define\s+OFX_VERSION\s+(\d+)", _header()).group(1)) == 102


def test_library_exports_the_sequence_entries():
    so = os.path.join(ROOT, "optical-flow-1_amd", "libofx.so")
    require_or_skip(os.path.exists(so), "optical-flow-1_amd/libofx.so not built")
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "ofx_tvl1occ_sequence_group_dev") and hasattr(lib, "ofx_tvl1occ_sequence_dev")


def test_python_mirror_binds_the_sequence_entries(ofx_mod):
    L = ofx_mod.lib()
    assert "ofx_tvl1occ_sequence_group_dev" not in L.ofx_missing and "ofx_tvl1occ_sequence_dev" not in L.ofx_missing
    assert len(L.ofx_tvl1occ_sequence_group_dev.argtypes) == len(GROUP)
    assert len(L.ofx_tvl1occ_sequence_dev.argtypes) == len(BATCH)
    group = list(inspect.signature(ofx_mod.Ofx.tvl1occ_sequence_group_dev).parameters)
    assert group[:6] == ["self", "dF", "d_flo", "d_occ", "nx", "ny"] and len(group) == 4 + len(SOLVER)
    batch = list(inspect.signature(ofx_mod.tvl1occ_sequence_dev).parameters)
    assert batch[:6] == ["ctxs", "dF", "d_flo", "d_occ", "nx", "ny"] and len(batch) == 4 + len(SOLVER)
    # the defaults of tvl1occ_batch
    keys = ("lam", "alpha", "beta", "theta", "nscales", "zfactor", "warps", "epsilon")
    want = [inspect.signature(ofx_mod.tvl1occ_batch).parameters[k].default for k in keys]
    for fn in (ofx_mod.Ofx.tvl1occ_sequence_group_dev, ofx_mod.tvl1occ_sequence_dev):
        assert [inspect.signature(fn).parameters[k].default for k in keys] == want
