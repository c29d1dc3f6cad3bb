#!/usr/bin/env python3
"""Cost of robust_expo on a colour pair at one scale: one 1280x720x3 pair (method 1, nscales = 1, the
reference's defaults otherwise) through ofx_robust_expo, next to
  (a) the compiled reference on ONE thread on the same input (skipped where oracle/_ref/libofref.so is absent), and
  (b) the one-channel solve of the same size at nscales = 1 (channel 0; the same driver and level kernels with nz = 1).
Prints one JSON line; --out FILE also writes it there.

    python tools/bench_rexpo_color.py [--nx 1280 --ny 720 --nz 3 --reps 3 --no-ref --out profiles/rexpo_color_1280x720.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1280)
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--nz", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ofx = importlib.import_module("optical-flow-1_amd")
    synth = importlib.import_module("optical-flow-1_amd.synth")
    kw = dict(method=1, alpha=50.0, gamma=10.0, lam=1.0, nscales=1, nu=0.5, TOL=1e-4, inner=1, outer=15)
    I1, I2 = synth.colour_pair("P1", a.nx, a.ny, a.nz)
    ctx = ofx.Ofx(0, ofx.F64)

    def timed(fn):
        best, out = None, None
        for _ in range(a.reps + 1):                     # the first run warms the workspace up and is not counted
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            best = dt if _ > 0 and (best is None or dt < best) else best
        st = ctx.stats()
        return best, out, int(st.iterations()[0].sum())

    t_col, (uc, vc), sw_col = timed(lambda: ctx.robust_expo(I1, I2, **kw))
    p1, p2 = np.ascontiguousarray(I1[..., 0]), np.ascontiguousarray(I2[..., 0])
    t_one, _, sw_one = timed(lambda: ctx.robust_expo(p1, p2, **kw))
    res = dict(bench="rexpo_color", nx=a.nx, ny=a.ny, nz=a.nz, params=kw, gpu_colour_s=t_col, gpu_colour_sweeps=sw_col,
               gpu_one_channel_s=t_one, gpu_one_channel_sweeps=sw_one,
               gpu_colour_ms_per_sweep=1e3 * t_col / max(sw_col, 1), gpu_one_channel_ms_per_sweep=1e3 * t_one / max(sw_one, 1))
    import oracle
    if not a.no_ref and oracle.have_ref():
        ref = oracle.Ref()
        ref.set_num_threads(1)
        f = ref.lib.ref_robust_expo
        dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
        f.restype = C.c_int
        f.argtypes = [dp, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double,
                      C.c_double, C.c_int, C.c_int, C.c_int]
        ur, vr = np.zeros((a.ny, a.nx)), np.zeros((a.ny, a.nx))
        t0 = time.perf_counter()
        rc = f(I1, I2, ur, vr, a.nx, a.ny, a.nz, kw["method"], kw["alpha"], kw["gamma"], kw["lam"], 1, kw["nu"], kw["TOL"],
               kw["inner"], kw["outer"], 0)
        res.update(ref_one_thread_s=time.perf_counter() - t0, ref_rc=rc, max_abs_du=float(np.abs(uc - ur).max()),
                   max_abs_dv=float(np.abs(vc - vr).max()), speedup_vs_ref=(time.perf_counter() - t0) / t_col)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
