"""ofx_track_structure_dev, ofx_track_seed_dev and ofx_track_sequence_dev in the public surface: header, library export, Python
mirror, front-end and translation unit (CPU only)."""
import ctypes
import inspect
import os
import re

from conftest import require_or_skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {
    "ofx_track_structure_dev": [
        "ofx_ctx *ctx", "int n", "const void *const *dF", "void *const *d_lam2", "void *const *d_mean", "int nx", "int ny", "double rho"],
    "ofx_track_seed_dev": [
        "ofx_ctx *ctx", "int n", "const void *const *dF", "const void *const *d_xy_occ", "int n_occ", "void *const *d_xy_new",
        "void *const *d_count", "int cap", "int nx", "int ny", "double rho", "double frac", "int step"],
    "ofx_track_sequence_dev": [
        "ofx_ctx *ctx", "int n_seq", "int n_frames", "const void *const *dF", "const void *const *d_flo_step",
        "const void *const *d_occ_step", "int cap", "void *const *d_xy", "void *const *d_t0", "void *const *d_len",
        "void *const *d_count", "int nx", "int ny", "double rho", "double frac", "int step"],
}


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def test_header_declares_the_three_entries_under_their_heading_and_the_macro():
    h = _header()
    for name, args in ENTRIES.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, h)
        assert m, "%s is not declared in include/ofx.h" % name
        assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == args, name
    assert int(re.search(r"#define\s+OFX_VERSION\s+(\d+)", h).group(1)) == 102      # additions: the version stays
    assert "Track seeds and dense point trajectories" in h
    size = int(re.search(r"#define\s+OFX_TRACK_MAX_SIZE\s+(\d+)", h).group(1))
    assert size >= int(5 * 2.0) + 1                                                  # rho = 2 is served
    text = re.sub(r"\s*\n\s*\*\s*", " ", h)                                          # comment lines joined
    for words in ("= 0.5 * ((A + C) - r)", "the order is part of the result", "Slots beyond the count are not written at all",
                  "the frames before t0 repeat the birth position bit for bit", "the call makes no host synchronisation"):
        assert words in text, words


def test_library_exports_the_three_entries():
    so = os.path.join(ROOT, "optical-flow-1_amd", "libofx.so")
    require_or_skip(os.path.exists(so), "optical-flow-1_amd/libofx.so not built")
    L = ctypes.CDLL(so)
    for name in ENTRIES:
        assert hasattr(L, name), name


def test_python_mirror_binds_them(ofx_mod):
    L = ofx_mod.lib()
    assert L.ofx_missing == []
    for name, args in ENTRIES.items():
        assert len(getattr(L, name).argtypes) == len(args), name
    p = inspect.signature(ofx_mod.Ofx.track_structure_dev).parameters
    assert list(p) == ["self", "dF", "nx", "ny", "rho", "d_lam2", "d_mean"]
    assert p["d_lam2"].default is None and p["d_mean"].default is None
    p = inspect.signature(ofx_mod.Ofx.track_seed_dev).parameters
    assert list(p) == ["self", "dF", "d_xy_new", "d_count", "cap", "nx", "ny", "rho", "frac", "step", "d_xy_occ", "n_occ"]
    assert p["d_xy_occ"].default is None and p["n_occ"].default == 0
    p = inspect.signature(ofx_mod.Ofx.track_sequence_dev).parameters
    assert list(p) == ["self", "dF", "d_flo_step", "cap", "d_xy", "d_t0", "d_len", "d_count", "nx", "ny", "rho", "frac", "step", "d_occ_step"]
    assert p["d_occ_step"].default is None


def test_front_end_translation_unit_and_the_shared_advance_are_built_by_the_makefiles():
    mk = open(os.path.join(ROOT, "optical-flow-1_amd", "cli", "Makefile")).read()
    progs = re.search(r"^PROGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "flow_tracks" in progs
    assert os.path.exists(os.path.join(ROOT, "optical-flow-1_amd", "cli", "flow_tracks.c"))
    csrc = os.path.join(ROOT, "optical-flow-1_amd", "csrc")
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert "ofx_tracks.hip" in srcs and os.path.exists(os.path.join(csrc, "ofx_tracks.hip"))
    # one copy of the advance rule: both translation units include the header, neither defines the sampling itself
    for unit in ("ofx_compose.hip", "ofx_tracks.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "ofx_advance.h"' in text and "cp_advance(" in text, unit
        assert not re.search(r"OFX_DEV\s+\w+\s+cp_(sample|flagged|inside|advance)\s*\(", text), unit
