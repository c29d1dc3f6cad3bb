"""The grouping arithmetic of every batch entry (csrc/ofx_group_plan.h), pinned without a GPU: tests/group_plan_driver.cpp is built
with the host C++ compiler against the header alone and prints the three rules over a grid; every line is compared with the
restatement below.  Payloads do not depend on the group size, so this is the only pin on the group sizes of the SOR, occlusion
and temporal-Brox batches (the TV-L1 batch's are also asserted on the GPU, tests/test_gpu_tvl1.py::test_batch_entry_point)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "optical-flow-1_amd", "csrc")


def cdiv(a, b):
    return -(-a // b)


def lockstep(lock, max_group, dflt):
    return min(lock, max_group) if lock > 0 else dflt


def even_rounds(n_items, n_ctx, cap):
    if n_items <= 1:
        return 1
    rounds = cdiv(n_items, n_ctx * cap)
    return max(1, cdiv(n_items, n_ctx * rounds))


def cap_per_ctx(G, n_items, n_ctx):
    return min(G, cdiv(n_items, n_ctx))


RULES = {"lockstep": lockstep, "even_rounds": even_rounds, "cap_per_ctx": cap_per_ctx}


@pytest.fixture(scope="module")
def table():
    """(rule, a, b, c) -> value, as the compiled header gives it"""
    out = os.path.join(HERE, "_build", "group_plan_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC,
           os.path.join(HERE, "group_plan_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = {}
    for line in r.stdout.split("\n"):
        if line:
            rule, a, b, c, value = line.split()
            t[(rule, int(a), int(b), int(c))] = int(value)
    return t


def test_the_header_is_the_restatement(table):
    for (rule, a, b, c), value in table.items():
        assert value == RULES[rule](a, b, c), (rule, a, b, c, value)


def test_the_grid_is_whole(table):
    for n in range(0, 71):
        for ctx in range(1, 6):
            for cap in range(1, 17):
                assert ("even_rounds", n, ctx, cap) in table and ("cap_per_ctx", cap, n, ctx) in table
    assert len(table) == 2 * 71 * 5 * 16 + 42 * 4


@pytest.mark.parametrize("n_items,n_ctx,G", [(5, 2, 3), (1, 2, 1), (20, 2, 10), (33, 2, 9), (64, 2, 16), (65, 2, 11), (7, 1, 7)])
def test_even_rounds_known_values(table, n_items, n_ctx, G):
    """cap = 16: what test_batch_entry_point asserts of ofx_tvl1_batch_group_size on the GPU"""
    assert table[("even_rounds", n_items, n_ctx, 16)] == G


def test_cap_per_ctx_known_values(table):
    assert table[("cap_per_ctx", 16, 5, 3)] == 2                # five triples on three contexts: groups of 2, 2, 1
    assert table[("cap_per_ctx", 16, 5, 1)] == 5


def test_lockstep_clamps(table):
    assert table[("lockstep", 40, 16, 16)] == 16
    assert table[("lockstep", 3, 16, 16)] == 3
    assert table[("lockstep", 0, 16, 11)] == 11 and table[("lockstep", -1, 16, 1)] == 1
