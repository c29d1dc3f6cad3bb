#!/usr/bin/env python3
"""SOR warm start on video: what the previous frame's flow buys Horn-Schunck and Brox, and that the plain entries did not slow.
    python tools/bench_sor_warm.py [--check] [--solver hs|brox] [--size WxH] [--seqs 3] [--frames 8] [--reps 3] [--tolerance]
                                   [--parent-lib PATH/libofx.so] [--ab-only] [--rounds 3] [--out profiles/FILE.json]
The chains: synth.sequence, SEQS sequences x FRAMES frames on the device, BASELINE config 3 (Horn-Schunck, 1920x1080, 5 scales,
10 warps) or config 4 (Brox, 1280x720, 6 scales, 15 outer iterations).  The cold chain (ofx_*_group_dev on every step) against
the warm chains (ofx_*_sequence_group_dev: cold at step 0, then nscales_next = 1, 2 from the step before, the warps / outer
iterations unchanged), alternated in one process, REPS times each, medians.  Per chain: ms per chain and per warm pair, sweeps and
pixel-sweeps per step (sums over the sequences) and the AEPE of every warm step against the cold one.  --tolerance: sor_exact = 0.
--check: the warm chains' first step must equal the cold one byte for byte (it is a cold solve) and every payload must be finite;
with --parent-lib the plain entries are timed A/B: ofx_hs_group_dev (1920x1080) and ofx_brox_group_dev (1280x720), a lone pair
and a group of 16, exact mode, this library and the parent commit's one alternated in fresh child processes (one library per
process), the median of 5 calls each, ROUNDS times; the margin is the spread of the parent's own medians in that session.  Exit
status 1 if a check fails.  One JSON record, printed and written to --out.
--ab-only: the A/B without the chains.  --role plain is the child: the plain groups alone on the library that OFX_LIB_PATH names."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = {"hs": "1920x1080", "brox": "1280x720"}
PAR = {"hs": dict(alpha=20.0, zfactor=0.5, TOL=1e-4, maxiter=150), "brox": dict(alpha=50.0, gamma=10.0, nu=0.5, TOL=1e-4, inner=1)}
COLD = {"hs": dict(nscales=5, warps=10), "brox": dict(nscales=6, outer=15)}

ap = argparse.ArgumentParser()
ap.add_argument("--solver", default="hs", choices=["hs", "brox"])
ap.add_argument("--size", default="")
ap.add_argument("--seqs", type=int, default=3)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tolerance", action="store_true")
ap.add_argument("--check", action="store_true")
ap.add_argument("--ab-only", action="store_true")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--out", default="")
ap.add_argument("--role", default="chains", choices=["chains", "plain"])
a = ap.parse_args()


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def plain_alone():
    """ofx_hs_group_dev and ofx_brox_group_dev, a lone pair and a group of 16: the median of 5 calls after a warming one"""
    import torch
    torch.cuda.init()               # torch brings its own HIP runtime and has to see the device before libofx.so does
    sys.path.insert(0, ROOT)
    ofx = importlib.import_module("optical-flow-1_amd")
    synth = importlib.import_module("optical-flow-1_amd.synth")
    ctx = ofx.Ofx(0, ofx.F64)
    out = {"library": ofx.LIB_PATH}
    for solver in ("hs", "brox"):
        w, h = (int(v) for v in SIZE[solver].split("x"))
        pairs = [synth.pair_device("P1", w, h, k, "cuda", torch.float64) for k in range(16)]
        flo = torch.zeros((16, h, w, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        entry = ctx.hs_group_dev if solver == "hs" else ctx.brox_group_dev
        for G in (1, 16):
            def run():
                entry([p[0].data_ptr() for p in pairs[:G]], [p[1].data_ptr() for p in pairs[:G]], [flo[g].data_ptr() for g in range(G)],
                      w, h, **PAR[solver], **COLD[solver])
                ctx.synchronize()
            run()
            ms = [timed(run)[0] for _ in range(5)]
            out["%s_x%d" % (solver, G)] = {"median_ms": round(statistics.median(ms), 3), "all_ms": [round(x, 3) for x in ms]}
        del pairs, flo
    return out


if a.role == "plain":
    print(json.dumps(plain_alone()), flush=True)
    sys.exit(0)

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, ROOT)
ofx = importlib.import_module("optical-flow-1_amd")
synth = importlib.import_module("optical-flow-1_amd.synth")


def chains():
    """the cold and the warm chains -> (record, all checks passed)"""
    size = a.size or SIZE[a.solver]
    nx, ny = (int(v) for v in size.split("x"))
    ctx = ofx.Ofx(0, ofx.F64)
    if a.tolerance:
        ctx.set_option("sor_exact", 0)
    S, T = a.seqs, a.frames
    F = [[torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in synth.sequence(nx, ny, T, k)] for k in range(S)]
    NEXT = [1, 2]
    flo = {n: torch.zeros((S, T - 1, ny, nx, 2), dtype=torch.float32, device="cuda") for n in [0] + NEXT}       # 0 = the cold chain
    torch.cuda.synchronize()
    par, cold = PAR[a.solver], COLD[a.solver]

    def cold_chain():
        entry = ctx.hs_group_dev if a.solver == "hs" else ctx.brox_group_dev
        out = []
        for t in range(T - 1):
            out.append(entry([F[q][t].data_ptr() for q in range(S)], [F[q][t + 1].data_ptr() for q in range(S)],
                             [flo[0][q, t].data_ptr() for q in range(S)], nx, ny, **par, **cold))
        ctx.synchronize()
        return [[out[t][q] for t in range(T - 1)] for q in range(S)]

    def warm_chain(n):
        dF = [[f.data_ptr() for f in F[q]] for q in range(S)]
        dP = [[flo[n][q, t].data_ptr() for t in range(T - 1)] for q in range(S)]
        if a.solver == "hs":
            st = ctx.hs_sequence_group_dev(dF, dP, nx, ny, nscales_first=cold["nscales"], nscales_next=n, warps_first=cold["warps"],
                                           warps_next=cold["warps"], **par)
        else:
            st = ctx.brox_sequence_group_dev(dF, dP, nx, ny, nscales_first=cold["nscales"], nscales_next=n, outer_first=cold["outer"],
                                             outer_next=cold["outer"], **par)
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
        return {"sweeps": [int(sum(st[q][t].iterations().sum() for q in range(S))) for t in range(T - 1)],
                "pix_sweeps": [float(sum(st[q][t].work_pix_iters for q in range(S))) for t in range(T - 1)]}

    cold_ms = statistics.median(ms[0])
    rec = {"solver": a.solver, "size": size, "sequences": S, "frames": T, "reps": a.reps, "mode": "f64 tolerance" if a.tolerance else "f64 exact",
           "parameters": dict(par, **cold),
           "cold": dict(chain_ms_median=round(cold_ms, 2), ms_per_pair=round(cold_ms / (S * (T - 1)), 3), chain_ms=[round(x, 2) for x in ms[0]],
                        **per_step(stats[0]))}
    ok = bool(torch.isfinite(flo[0]).all())
    for n in NEXT:
        d = (flo[n] - flo[0]).double()
        e = torch.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2).mean(dim=(0, 2, 3))
        m = statistics.median(ms[n])
        # a warm pair: the chain without its cold first step, which costs what a cold step costs
        rec["warm_nscales_next_%d" % n] = dict(chain_ms_median=round(m, 2), ms_per_pair=round(m / (S * (T - 1)), 3),
                                               ms_per_warm_pair=round((m - cold_ms / (T - 1)) / (S * (T - 2)), 3),
                                               chain_ms=[round(x, 2) for x in ms[n]],
                                               aepe_vs_cold_per_step=[float("%.4g" % x) for x in e.tolist()], **per_step(stats[n]))
        ok = ok and bool(torch.isfinite(flo[n]).all())
        if a.check:
            ok = ok and bool(torch.equal(flo[n][:, 0], flo[0][:, 0]))
    rec["first_step_equals_cold_and_all_finite"] = ok if a.check else None
    return rec, ok


rec, ok = ({"chains": "not run: --ab-only"}, True) if a.ab_only else chains()
torch.cuda.empty_cache()

if a.check and a.parent_lib:
    def child(lib):
        env = dict(os.environ, OFX_LIB_PATH=lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "plain"], env=env, capture_output=True, text=True,
                           timeout=600)
        if r.returncode:
            sys.exit("the A/B child failed on %s: %s" % (lib, r.stderr[-400:]))
        return json.loads(r.stdout.strip().splitlines()[-1])
    this_lib = ofx.LIB_PATH
    parent, this = [], []
    for _ in range(a.rounds):
        parent.append(child(os.path.abspath(a.parent_lib)))
        this.append(child(this_lib))
    rec["plain_entries_ab"] = {}
    for key in ("hs_x1", "hs_x16", "brox_x1", "brox_x16"):
        p, t = [r[key]["median_ms"] for r in parent], [r[key]["median_ms"] for r in this]
        margin = max(p) - min(p)
        rec["plain_entries_ab"][key] = {"parent_median_ms": p, "this_median_ms": t, "margin_ms": round(margin, 3),
                                        "this_minus_parent_ms": round(statistics.median(t) - statistics.median(p), 3),
                                        "no_slower": statistics.median(t) <= statistics.median(p) + margin}
        ok = ok and rec["plain_entries_ab"][key]["no_slower"]
elif a.check:
    rec["plain_entries_ab"] = "not run: no --parent-lib"

print(json.dumps(rec), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
if a.check and not ok:
    sys.exit(1)
