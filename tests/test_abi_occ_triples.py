"""ofx_tvl1occ_triples_group_dev / ofx_tvl1occ_triples_dev / ofx_tvl1occ_triples_frames in the public surface: header, library
export, Python mirror, and the pure host decision that builds the tables of both entries (CPU only)."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import require_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOLVER = ["int nxx", "int nyy", "double lambda", "double alpha", "double beta", "double theta", "int nscales", "double zfactor",
          "int warps", "double epsilon"]
TABLES = ["int n_frames", "const void *const *dF", "int n_triples", "const ofx_occ_triple *tr", "void *const *d_flo",
          "void *const *d_occ"]
GROUP = ["ofx_ctx *ctx"] + TABLES + SOLVER + ["ofx_stats *stats_out"]
BATCH = ["ofx_ctx *const *ctxs", "int n_ctx"] + TABLES + SOLVER + ["double *work_pix_iters"]
FRAMES = ["int n_frames", "int n_triples", "const ofx_occ_triple *tr", "int *frames_out", "unsigned char *roles_out"]
ERR_ARG = 1


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def _declared(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "%s is not declared in include/ofx.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_the_triples_entries():
    assert _declared("ofx_tvl1occ_triples_group_dev") == GROUP
    assert _declared("ofx_tvl1occ_triples_dev") == BATCH
    assert _declared("ofx_tvl1occ_triples_frames") == FRAMES
    m = re.search(r"typedef\s+struct\s+ofx_occ_triple\s*\{([^}]*)\}\s*ofx_occ_triple\s*;", _header())
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "int prev, cur, next, filt;"
    # the sequence entries no longer send these uses to the host entries
    assert "Not provided" not in _header()


def test_version_is_still_102():
    assert int(re.search(r"#define\s+OFX_VERSION\s+(\d+)", _header()).group(1)) == 102


def test_library_exports_the_triples_entries():
    so = os.path.join(ROOT, "optical-flow-1_amd", "libofx.so")
    require_or_skip(os.path.exists(so), "optical-flow-1_amd/libofx.so not built")
    lib = ctypes.CDLL(so)
    for name in ("ofx_tvl1occ_triples_group_dev", "ofx_tvl1occ_triples_dev", "ofx_tvl1occ_triples_frames"):
        assert hasattr(lib, name), name


def test_python_mirror_binds_the_triples_entries(ofx_mod):
    L = ofx_mod.lib()
    for name, args in (("ofx_tvl1occ_triples_group_dev", GROUP), ("ofx_tvl1occ_triples_dev", BATCH),
                       ("ofx_tvl1occ_triples_frames", FRAMES)):
        assert name not in L.ofx_missing
        assert len(getattr(L, name).argtypes) == len(args), name
    assert [(n, t) for n, t in ofx_mod.OccTriple._fields_] == [(n, ctypes.c_int) for n in ("prev", "cur", "next", "filt")]
    assert ctypes.sizeof(ofx_mod.OccTriple) == 16
    group = list(inspect.signature(ofx_mod.Ofx.tvl1occ_triples_group_dev).parameters)
    assert group[:7] == ["self", "dF", "triples", "d_flo", "d_occ", "nx", "ny"] and len(group) == 5 + len(SOLVER)
    batch = list(inspect.signature(ofx_mod.tvl1occ_triples_dev).parameters)
    assert batch[:7] == ["ctxs", "dF", "triples", "d_flo", "d_occ", "nx", "ny"] and len(batch) == 5 + len(SOLVER)
    assert list(inspect.signature(ofx_mod.tvl1occ_triples_frames).parameters) == ["n_frames", "triples"]
    # the defaults of tvl1occ_batch
    keys = ("lam", "alpha", "beta", "theta", "nscales", "zfactor", "warps", "epsilon")
    want = [inspect.signature(ofx_mod.tvl1occ_batch).parameters[k].default for k in keys]
    for fn in (ofx_mod.Ofx.tvl1occ_triples_group_dev, ofx_mod.tvl1occ_triples_dev):
        assert [inspect.signature(fn).parameters[k].default for k in keys] == want


# ---- ofx_tvl1occ_triples_frames on hand cases ----------------------------------------------------------------------------------
def test_frames_consecutive_pattern(ofx_mod):
    for G in (1, 5, 16):
        frames, roles = ofx_mod.tvl1occ_triples_frames(G + 2, [(t, t + 1, t + 2, -1) for t in range(G)])
        assert frames == list(range(G + 2))                                     # D = G + 2, in sequence order
        assert roles == [(t, t + 1, t + 2, t + 1) for t in range(G)]


def test_frames_forward_and_backward_share_their_planes(ofx_mod):
    frames, roles = ofx_mod.tvl1occ_triples_frames(10, [(4, 5, 6), (6, 5, 4)])
    assert frames == [4, 5, 6]
    assert roles == [(0, 1, 2, 1), (2, 1, 0, 1)]
    # a second centre adds one plane
    frames, roles = ofx_mod.tvl1occ_triples_frames(10, [(4, 5, 6), (6, 5, 4), (5, 6, 7), (7, 6, 5)])
    assert frames == [4, 5, 6, 7]
    assert roles == [(0, 1, 2, 1), (2, 1, 0, 1), (1, 2, 3, 2), (3, 2, 1, 2)]


def test_frames_filt_default_against_an_explicit_index(ofx_mod):
    assert ofx_mod.tvl1occ_triples_frames(4, [(0, 1, 2, -1)]) == ([0, 1, 2], [(0, 1, 2, 1)])
    assert ofx_mod.tvl1occ_triples_frames(4, [(0, 1, 2, 1)]) == ([0, 1, 2], [(0, 1, 2, 1)])
    assert ofx_mod.tvl1occ_triples_frames(4, [(0, 1, 2, 3)]) == ([0, 1, 2, 3], [(0, 1, 2, 3)])
    # order of first appearance: roles prev, cur, next, filt of triple 0, then triple 1
    assert ofx_mod.tvl1occ_triples_frames(9, [(7, 2, 5, 8), (8, 7, 0, 2)]) == ([7, 2, 5, 8, 0], [(0, 1, 2, 3), (3, 0, 4, 1)])


def test_frames_one_index_in_all_roles(ofx_mod):
    assert ofx_mod.tvl1occ_triples_frames(6, [(3, 3, 3, 3)]) == ([3], [(0, 0, 0, 0)])
    assert ofx_mod.tvl1occ_triples_frames(6, [(3, 3, 3, -1), (3, 3, 3, 3)]) == ([3], [(0, 0, 0, 0)] * 2)
    assert ofx_mod.tvl1occ_triples_frames(1, [(0, 0, 0)]) == ([0], [(0, 0, 0, 0)])


def test_frames_sixteen_triples_with_64_distinct_indices(ofx_mod):
    triples = [(4 * k + 3, 4 * k, 4 * k + 2, 4 * k + 1) for k in range(16)]
    frames, roles = ofx_mod.tvl1occ_triples_frames(64, triples)
    assert len(frames) == 64 and sorted(frames) == list(range(64))
    assert frames[:4] == [3, 0, 2, 1]
    assert roles == [(4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3) for k in range(16)]
    for k, t in enumerate(triples):                                             # the table resolves every role to its index
        assert tuple(frames[p] for p in roles[k]) == t


def test_frames_rejects_indices_outside_the_table(ofx_mod):
    L = ofx_mod.lib()
    for bad in ((0, 1, 4, -1), (4, 1, 2, -1), (0, 4, 2, -1), (0, 1, 2, 4), (0, 1, 2, -2), (-1, 1, 2, -1), (0, -1, 2, -1),
                (0, 1, -1, -1), (0, 1, -3, 0)):
        with pytest.raises(ofx_mod.OfxError) as e:
            ofx_mod.tvl1occ_triples_frames(4, [(0, 1, 2), bad])
        assert e.value.status == ERR_ARG, bad
        tr = (ofx_mod.OccTriple * 1)(ofx_mod.OccTriple(*bad))
        assert L.ofx_tvl1occ_triples_frames(4, 1, tr, None, None) == -ERR_ARG, bad     # the C return value itself
    tr = (ofx_mod.OccTriple * 1)(ofx_mod.OccTriple(0, 0, 0, -1))
    assert L.ofx_tvl1occ_triples_frames(0, 1, tr, None, None) == -ERR_ARG             # an empty table
    assert L.ofx_tvl1occ_triples_frames(1, 1, tr, None, None) == 1                    # counting alone needs no output arrays
