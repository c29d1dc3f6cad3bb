"""ofx_brox_temporal_group_dev in the public surface: header, library export, Python mirror (CPU only)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUP = ["ofx_ctx *ctx", "int n_seq", "int frames", "const void *const *dF", "void *const *d_flo", "int nxx", "int nyy", "double alpha",
         "double gamma", "int nscales", "double nu", "double TOL", "int inner_iter", "int outer_iter", "ofx_stats *stats_out"]
KEYS = ("alpha", "gamma", "nscales", "nu", "TOL", "inner", "outer")


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def test_header_declares_the_entry():
    m = re.search(r"int\s+ofx_brox_temporal_group_dev\s*\(([^)]*)\)\s*;", _header())
    assert m, "ofx_brox_temporal_group_dev is not declared in include/ofx.h"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == GROUP


def test_header_states_both_batch_behaviours():
    text = re.sub(r"\s*\n \*\s*", " ", _header())
    at = text.index("int ofx_brox_temporal_batch_dev")
    comment = text[text.rindex("/*", 0, at):at]
    assert '"lockstep" of ctxs[0] = L >= 2' in comment and '"lockstep" of ctxs[0] = 0 or 1' in comment


def test_version_is_still_102():
    assert int(re.search(r"#define\s+OFX_VERSION\s+(\d+)", _header()).group(1)) == 102


def test_library_exports_the_entry(ofx_mod):
    if not os.path.exists(ofx_mod.LIB_PATH):
        ofx_mod.build()
    assert hasattr(ctypes.CDLL(ofx_mod.LIB_PATH), "ofx_brox_temporal_group_dev")


def test_python_mirror_binds_the_entry(ofx_mod):
    L = ofx_mod.lib()
    assert L.ofx_missing == []
    assert len(L.ofx_brox_temporal_group_dev.argtypes) == len(GROUP)
    group = list(inspect.signature(ofx_mod.Ofx.brox_temporal_group_dev).parameters)
    assert group[:6] == ["self", "dF", "d_flo", "nx", "ny", "frames"] and len(group) == 6 + len(KEYS)
    want = [inspect.signature(ofx_mod.Ofx.brox_temporal_dev).parameters[k].default for k in KEYS]
    assert [inspect.signature(ofx_mod.Ofx.brox_temporal_group_dev).parameters[k].default for k in KEYS] == want
    # the batch wrapper keeps its argument list: it reads the group size from the context's option
    batch = list(inspect.signature(ofx_mod.brox_temporal_batch_dev).parameters)
    assert batch[:6] == ["ctxs", "dF", "d_flo", "nx", "ny", "frames"] and len(batch) == 6 + len(KEYS)
