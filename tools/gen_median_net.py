#!/usr/bin/env python3
"""Writes optical-flow-1_amd/csrc/ofx_median_net.h: the comparator lists of csrc/ofx_median.hip.

For a W x W window whose W columns are already sorted, MEDIAN_NET_W(CE) is a list of compare-exchanges CE(a, b) -- wire a
receives the smaller, wire b the larger value -- after which the W * W wires read in the order MEDIAN_ORD_W are sorted.  Wire
k * W + t is element t of sorted column k.  The list is a tree of Batcher odd-even merges of arbitrary lengths (Knuth, TAOCP 3,
5.3.4): the columns are merged pairwise until one sequence is left.  The kernel uses one wire of the result where the rank is a
constant; the compiler then removes every comparator that this wire does not depend on, which is the pruned selection network.

The lists are checked here before they are written: by the 0-1 principle over every input whose columns are sorted (W + 1 zero
counts per column, (W + 1) ** W inputs) for the whole sort, and the count of comparators that the median wire depends on is
printed.  Run from the repository root:  python tools/gen_median_net.py
"""
import itertools
import os

import numpy as np


def merge(A, B, ces):
    """Batcher's odd-even merge of two sorted wire lists -> the wires in sorted order"""
    if not A:
        return list(B)
    if not B:
        return list(A)
    if len(A) == 1 and len(B) == 1:
        ces.append((A[0], B[0]))
        return [A[0], B[0]]
    V = merge(A[0::2], B[0::2], ces)
    Wl = merge(A[1::2], B[1::2], ces)
    out = [V[0]]
    for i in range(max(len(Wl), len(V) - 1)):
        w = Wl[i] if i < len(Wl) else None
        v = V[i + 1] if i + 1 < len(V) else None
        if w is not None and v is not None:
            ces.append((w, v))
            out += [w, v]
        else:
            out.append(w if v is None else v)
    return out


def network(W):
    ces = []
    seqs = [[k * W + t for t in range(W)] for k in range(W)]
    while len(seqs) > 1:
        seqs.sort(key=len)
        a, b = seqs.pop(0), seqs.pop(0)
        seqs.append(merge(a, b, ces))
    return ces, seqs[0]


# sorting networks of W wires for the columns themselves (Knuth, TAOCP 3, 5.3.4: 3, 9 and 16 comparators)
COLUMN = {3: [(0, 1), (1, 2), (0, 1)],
          5: [(0, 1), (3, 4), (2, 4), (2, 3), (1, 4), (0, 3), (0, 2), (1, 3), (1, 2)],
          7: [(1, 2), (3, 4), (5, 6), (0, 2), (3, 5), (4, 6), (0, 1), (4, 5), (2, 6), (0, 4), (1, 5), (0, 3), (2, 5), (1, 3), (2, 4),
              (2, 3)]}


def check_column(W):
    """0-1 principle over all 2 ** W inputs"""
    x = np.array(list(itertools.product((0, 1), repeat=W)), dtype=np.int8)
    for a, b in COLUMN[W]:
        lo, hi = np.minimum(x[:, a], x[:, b]), np.maximum(x[:, a], x[:, b])
        x[:, a], x[:, b] = lo, hi
    assert (np.diff(x, axis=1) >= 0).all(), "W = %d: the column network does not sort" % W


def live_count(ces, wire):
    live, kept = {wire}, 0
    for a, b in reversed(ces):
        if a in live or b in live:
            kept += 1
            live |= {a, b}
    return kept


def check(W, ces, order):
    """0-1 principle restricted to sorted columns: column k = z_k zeros, then ones"""
    cols = np.array(list(itertools.product(range(W + 1), repeat=W)), dtype=np.int8)             # zeros per column
    x = (np.arange(W, dtype=np.int8)[None, None, :] >= cols[:, :, None]).reshape(len(cols), W * W).astype(np.int8)
    for a, b in ces:
        lo, hi = np.minimum(x[:, a], x[:, b]), np.maximum(x[:, a], x[:, b])
        x[:, a], x[:, b] = lo, hi
    s = x[:, order]
    assert (np.diff(s, axis=1) >= 0).all(), "W = %d: not a sorting network on sorted columns" % W


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ["// ofx_median_net.h -- written by tools/gen_median_net.py; do not edit.",
             "// MEDIAN_NET_W(CE): compare-exchanges (smaller to the first wire) that sort the W * W wires of W sorted columns (wire",
             "// k * W + t = element t of column k); MEDIAN_ORD_W: the wires in ascending order afterwards; MEDIAN_COL_W(CE): a sorting",
             "// network of W wires, for the columns.",
             "#pragma once", ""]
    for W in (3, 5, 7):
        ces, order = network(W)
        check(W, ces, order)
        check_column(W)
        print("W = %d: %d comparators, %d of them reach the median wire %d" % (W, len(ces), live_count(ces, order[W * W // 2]),
                                                                               order[W * W // 2]))
        lines.append("#define MEDIAN_COL_%d(CE) %s" % (W, " ".join("CE(%d, %d)" % c for c in COLUMN[W])))
        lines.append("#define MEDIAN_NET_%d(CE) \\" % W)
        for k in range(0, len(ces), 10):
            lines.append("    " + " ".join("CE(%d, %d)" % c for c in ces[k:k + 10]) + (" \\" if k + 10 < len(ces) else ""))
        lines.append("#define MEDIAN_ORD_%d %s" % (W, ", ".join(str(o) for o in order)))
        lines.append("")
    with open(os.path.join(root, "optical-flow-1_amd", "csrc", "ofx_median_net.h"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
