#!/usr/bin/env python3
"""TV-L1 warm start on video: what the previous frame's flow buys, and that the plain entries did not slow.
    python tools/bench_tvl1_warm.py [--check] [--size 1920x1080] [--seqs 5] [--frames 8] [--reps 3]
                                    [--parent-lib PATH/libofx.so] [--out profiles/FILE.json]
The chains: synth.sequence, SEQS sequences x FRAMES frames on the device.  The cold chain (ofx_tvl1_group_dev with 5 scales at
every step) against the warm chains (ofx_tvl1_sequence_group_dev: 5 scales at step 0, then nscales_next = 1, 2, 3 from the step
before), alternated in one process, REPS times each, medians.  Per chain: ms per pair, inner iterations and pixel-iterations per
step (sums over the sequences) and the AEPE of every warm step against the cold one.
--check: the warm chains' first step must equal the cold one byte for byte (it is a cold solve), every payload must be finite, and
with --parent-lib the plain entry is timed A/B: ofx_tvl1_group_dev, 1080p x 5 pairs, this library and the parent commit's one
alternated in fresh child processes (one library per process), the median of 9 calls each, ROUNDS times; the margin is the spread
of the parent's own medians in that session.  Exit status 1 if a check fails.  One JSON record, printed and written to --out.
--role group is the child: the plain group alone on the library that OFX_LIB_PATH names."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--seqs", type=int, default=5)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--check", action="store_true")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--out", default="")
ap.add_argument("--role", default="chains", choices=["chains", "group"])
a = ap.parse_args()
nx, ny = (int(v) for v in a.size.split("x"))


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def group_alone():
    """ofx_tvl1_group_dev on SEQS seeded pairs: the median of 9 calls after two warming ones"""
    import torch
    torch.cuda.init()               # torch brings its own HIP runtime and has to see the device before libofx.so does
    sys.path.insert(0, ROOT)
    ofx = importlib.import_module("optical-flow-1_amd")
    synth = importlib.import_module("optical-flow-1_amd.synth")
    ctx = ofx.Ofx(0, ofx.F64)
    pairs = [synth.pair_device("P1", nx, ny, k, "cuda", torch.float64) for k in range(a.seqs)]
    flo = torch.zeros((a.seqs, ny, nx, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def run():
        st = ctx.tvl1_group_dev([p[0].data_ptr() for p in pairs], [p[1].data_ptr() for p in pairs],
                                [flo[g].data_ptr() for g in range(a.seqs)], nx, ny)
        ctx.synchronize()
        return st
    for _ in range(2):
        run()
    ms = [timed(run)[0] for _ in range(9)]
    return {"library": ofx.LIB_PATH, "median_ms": round(statistics.median(ms), 3), "all_ms": [round(x, 3) for x in ms]}


if a.role == "group":
    print(json.dumps(group_alone()), flush=True)
    sys.exit(0)

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ROOT)
ofx = importlib.import_module("optical-flow-1_amd")
synth = importlib.import_module("optical-flow-1_amd.synth")
ctx = ofx.Ofx(0, ofx.F64)
S, T = a.seqs, a.frames
F = [[torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in synth.sequence(nx, ny, T, k)] for k in range(S)]
NEXT = [1, 2, 3]
flo = {n: torch.zeros((S, T - 1, ny, nx, 2), dtype=torch.float32, device="cuda") for n in [0] + NEXT}       # 0 = the cold chain
torch.cuda.synchronize()


def cold_chain():
    out = []
    for t in range(T - 1):
        out.append(ctx.tvl1_group_dev([F[q][t].data_ptr() for q in range(S)], [F[q][t + 1].data_ptr() for q in range(S)],
                                      [flo[0][q, t].data_ptr() for q in range(S)], nx, ny, nscales=5))
    ctx.synchronize()
    return [[out[t][q] for t in range(T - 1)] for q in range(S)]


def warm_chain(n):
    st = ctx.tvl1_sequence_group_dev([[f.data_ptr() for f in F[q]] for q in range(S)],
                                     [[flo[n][q, t].data_ptr() for t in range(T - 1)] for q in range(S)], nx, ny, nscales_first=5,
                                     nscales_next=n)
    ctx.synchronize()
    return st


runs = {0: cold_chain}
runs.update({n: (lambda n=n: warm_chain(n)) for n in NEXT})
for f in runs.values():                                           # warm every route: arena slabs, clocks
    f()
ms, stats = {k: [] for k in runs}, {}
for _ in range(a.reps):                                           # alternated
    for k, f in runs.items():
        t, stats[k] = timed(f)
        ms[k].append(t)


def per_step(st):
    return {"inner_iterations": [int(sum(st[q][t].iterations().sum() for q in range(S))) for t in range(T - 1)],
            "pix_iterations": [float(sum(st[q][t].work_pix_iters for q in range(S))) for t in range(T - 1)]}


rec = {"size": a.size, "sequences": S, "frames": T, "reps": a.reps, "precision": "f64 strict",
       "cold_5_scales": dict(ms_per_pair=round(statistics.median(ms[0]) / (S * (T - 1)), 3),
                             chain_ms=[round(x, 2) for x in ms[0]], **per_step(stats[0]))}
ok = bool(torch.isfinite(flo[0]).all())
for n in NEXT:
    d = (flo[n] - flo[0]).double()
    e = torch.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2).mean(dim=(0, 2, 3))
    rec["warm_nscales_next_%d" % n] = dict(ms_per_pair=round(statistics.median(ms[n]) / (S * (T - 1)), 3),
                                           chain_ms=[round(x, 2) for x in ms[n]],
                                           aepe_vs_cold_per_step=[float("%.4g" % x) for x in e.tolist()], **per_step(stats[n]))
    ok = ok and bool(torch.isfinite(flo[n]).all())
    if a.check:
        ok = ok and bool(torch.equal(flo[n][:, 0], flo[0][:, 0]))
rec["first_step_equals_cold_and_all_finite"] = ok if a.check else None

if a.check and a.parent_lib:
    def child(lib):
        env = dict(os.environ, OFX_LIB_PATH=lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "group", "--size", "1920x1080", "--seqs", "5"], env=env,
                           capture_output=True, text=True, timeout=300)
        if r.returncode:
            sys.exit("the A/B child failed on %s: %s" % (lib, r.stderr[-400:]))
        return json.loads(r.stdout.strip().splitlines()[-1])["median_ms"]
    this_lib = ofx.LIB_PATH
    del ctx
    parent, this = [], []
    for _ in range(a.rounds):
        parent.append(child(os.path.abspath(a.parent_lib)))
        this.append(child(this_lib))
    margin = max(parent) - min(parent)
    rec["plain_group_1080p_x5_ab"] = {"parent_median_ms": parent, "this_median_ms": this, "margin_ms": round(margin, 3),
                                      "this_minus_parent_ms": round(statistics.median(this) - statistics.median(parent), 3),
                                      "no_slower": statistics.median(this) <= statistics.median(parent) + margin}
    ok = ok and rec["plain_group_1080p_x5_ab"]["no_slower"]
elif a.check:
    rec["plain_group_1080p_x5_ab"] = "not run: no --parent-lib"

print(json.dumps(rec), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
if a.check and not ok:
    sys.exit(1)
