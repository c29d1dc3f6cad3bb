"""The two HIP-free pieces of the pair-entry layer (csrc/ofx_group_plan.h), pinned without a GPU the way tests/test_group_plan.py
pins the group sizes: tests/pair_plan_driver.cpp is built with the host C++ compiler against the header alone and prints
  * ofx_frame_span, the bytes a frame spans in memory, over a grid of sizes, element widths and pitches, and
  * ofx_chain_walk, the walker of every video chain (ofx_*_sequence_group_dev), on fake pointers with a recording step function --
    including the failure path (a step that returns a status), which no GPU test reaches;
every line is compared with the restatement below."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "optical-flow-1_amd", "csrc")

SIZES = (0, 1, 2, 7)
BYTES = (1, 2, 3, 4, 8)
CHAINS = ((1, 2), (1, 3), (3, 5), (16, 2), (16, 4))            # (n_seq, n_frames)
FAIL = 7                                                        # the status the driver's step function fails with


def frame_span(nx, ny, nbytes, pitch):
    """with a pitch: from the first row's start to the last row's end; without (or for an empty frame): the rows back to back"""
    if pitch and nx > 0 and ny > 0:
        return (ny - 1) * pitch + nx * nbytes
    return nx * ny * nbytes


def fail_steps(n_frames):
    """-1: no step fails; then the first step and, where that is another one, the last"""
    return sorted({-1, 0, n_frames - 2})


def chain(n_seq, n_frames, k, with_stats):
    """-> (step lines, status, records) of a walk over frames 1000 + i and payloads 5000 + i whose step k fails"""
    steps = n_frames - 1
    dF = [1000 + i for i in range(n_seq * n_frames)]
    d_flo = [5000 + i for i in range(n_seq * steps)]
    calls, rec, status = [], [-1] * (n_seq * steps), 0
    for t in range(steps):
        for q in range(n_seq):
            init = d_flo[q * steps + t - 1] if t else -1        # step 0 gets no table of starts at all
            calls.append((t, q, dF[q * n_frames + t], dF[q * n_frames + t + 1], init, d_flo[q * steps + t]))
        if t == k:
            status = FAIL
            break
        for q in range(n_seq):
            rec[q * steps + t] = 100 * t + q
    return calls, status, (rec if with_stats else [])


@pytest.fixture(scope="module")
def lines():
    """the driver's output, split: {"span": {...}, "step": {case: [...]}, "ret": {case: status}, "rec": {case: {idx: value}}}"""
    out = os.path.join(HERE, "_build", "pair_plan_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC,
           os.path.join(HERE, "pair_plan_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr                             # no warnings
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = {"span": {}, "step": {}, "ret": {}, "rec": {}}
    for line in r.stdout.split("\n"):
        if not line:
            continue
        tag, *v = line.split()
        v = [int(x) for x in v]
        if tag == "span":
            assert t["span"].setdefault(tuple(v[:4]), v[4]) == v[4]     # nx = 0: "the row's own bytes" is no pitch, twice
        elif tag == "step":
            t["step"].setdefault(tuple(v[:4]), []).append(tuple(v[4:]))
        elif tag == "ret":
            assert tuple(v[:4]) not in t["ret"]
            t["ret"][tuple(v[:4])] = v[4]
        else:
            assert tag == "rec", line
            t["rec"].setdefault(tuple(v[:4]), {})[v[4]] = v[5]
    return t


def test_frame_span_is_the_restatement(lines):
    span = lines["span"]
    want = {(nx, ny, b, p) for nx in SIZES for ny in SIZES for b in BYTES for p in (0, nx * b, nx * b + 5)}
    assert set(span) == want
    for (nx, ny, b, pitch), value in span.items():
        assert value == frame_span(nx, ny, b, pitch), (nx, ny, b, pitch, value)


def test_frame_span_known_values(lines):
    span = lines["span"]
    assert span[(7, 2, 4, 33)] == 33 + 28                       # one pitch, then the last row's own bytes
    assert span[(7, 2, 4, 28)] == span[(7, 2, 4, 0)] == 56      # a pitch equal to the row is the dense frame
    assert span[(7, 1, 3, 26)] == 21                            # one row: the pitch does not count
    assert span[(2, 7, 8, 21)] == 6 * 21 + 16
    for b in BYTES:                                             # the guards of the call sites: an empty frame spans nothing
        assert span[(0, 7, b, 5)] == 0 and span[(7, 0, b, 7 * b + 5)] == 0 and span[(0, 0, b, 0)] == 0


def test_chain_walk_is_the_restatement(lines):
    cases = [(q, f, k, s) for q, f in CHAINS for k in fail_steps(f) for s in (0, 1)]
    assert set(lines["ret"]) == set(cases)
    for case in cases:
        calls, status, rec = chain(*case)
        assert lines["step"].get(case, []) == calls, case
        assert lines["ret"][case] == status, case
        got = lines["rec"].get(case, {})
        assert [got[i] for i in range(len(got))] == rec, case


def test_chain_walk_hands_each_step_its_pairs(lines):
    """spelt out for three sequences of five frames: frames t and t + 1, the payload of step t - 1 as start, record q of step t"""
    case = (3, 5, -1, 1)
    calls = lines["step"][case]
    assert len(calls) == 4 * 3
    for t, q, a, b, init, out in calls:
        assert (a, b, out) == (1000 + q * 5 + t, 1000 + q * 5 + t + 1, 5000 + q * 4 + t)
        assert init == (-1 if t == 0 else 5000 + q * 4 + t - 1)
    assert lines["ret"][case] == 0
    assert lines["rec"][case] == {q * 4 + t: 100 * t + q for q in range(3) for t in range(4)}
    assert (3, 5, -1, 0) not in lines["rec"] and lines["ret"][(3, 5, -1, 0)] == 0       # a NULL stats_out is accepted


@pytest.mark.parametrize("n_seq,n_frames", CHAINS)
def test_a_failing_step_ends_the_walk(lines, n_seq, n_frames):
    steps = n_frames - 1
    for k in (0, steps - 1):
        for with_stats in (0, 1):
            case = (n_seq, n_frames, k, with_stats)
            assert lines["ret"][case] == FAIL
            assert [c[0] for c in lines["step"][case]] == [t for t in range(k + 1) for _ in range(n_seq)]   # no step after k
        rec = lines["rec"][(n_seq, n_frames, k, 1)]
        for q in range(n_seq):
            for t in range(steps):                              # the records of the steps before k, nothing of step k or after
                assert rec[q * steps + t] == (100 * t + q if t < k else -1)
