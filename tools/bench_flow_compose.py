#!/usr/bin/env python3
"""Time ofx_flow_accumulate_dev and ofx_flow_tracks_dev on device-resident step payloads (one GPU).

    python tools/bench_flow_compose.py --size 1920x1080 --seqs 16 --steps 8 --points 1000000 --check [--out result.json]

The steps are the motion of synth.sequence's scene itself -- the background flow 0.6 * (1.5 + 0.5 sin(0.01 i), -0.75 + 0.25
cos(0.013 j)), the foreground rectangle moving by (2 + k % 3, -1.5) per frame, with its motion boundary --, one payload per sequence
k and step t, and the maps are ofx_flow_consistency_dev's on them and the true backward flows.  With and without the maps
alternate in one process; a figure is the median of `reps` calls, each with the context synchronised inside the timed region.  A
step is one launch over all sequences: its compulsory traffic is 8 B (acc read) + 8 B (step, each vector read once) + 8 B (acc
written) = 24 B per pixel, + 1 B lost state read and 1 B written = 26 B with maps; the fraction of the HBM peak is that over the
WHOLE call's time (launch gaps included).
tracks: `points` uniform query points of one sequence through all steps, one launch.
--check: accumulate equals the chained ofx_flow_compose_dev calls and, on sequence 0, the numpy restatement
(tests/flow_compose_ref.py) bit for bit; the tracks equal the restatement on the first 20000 points.  The restatement's run on
sequence 0 is also the comparison: the HOST ROUTE -- download the step payloads and maps, chain numpy bicubic lookups, upload the
accumulated payloads and maps -- timed once and scaled to the number of sequences.
Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12                      # bytes / s (spec)


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return sorted(v)[len(v) // 2]


def scene_steps(torch, nx, ny, n_seq, n_steps):
    """-> (fwd[k][t], bwd[k][t]) float32 payloads on the device: step t of sequence k on frame t's grid, its inverse on frame t + 1's"""
    f64 = torch.float64
    i, j = torch.meshgrid(torch.arange(ny, dtype=f64, device="cuda"), torch.arange(nx, dtype=f64, device="cuda"), indexing="ij")
    fx, fy = 0.6 * (1.5 + 0.5 * torch.sin(0.01 * i)), 0.6 * (-0.75 + 0.25 * torch.cos(0.013 * j))

    def fg(x, y):
        return (x >= nx // 4) & (x < nx // 2) & (y >= ny // 4) & (y < ny // 2)

    def field(k, t, sign):
        mx, my = 2.0 + (k % 3), -1.5
        m = fg(j - t * mx, i - t * my)
        u = torch.where(m, torch.full_like(fx, mx), fx)
        v = torch.where(m, torch.full_like(fy, my), fy)
        return (sign * torch.stack([u, v], dim=-1)).to(torch.float32).contiguous()
    fwd = [[field(k, t, 1.0) for t in range(n_steps)] for k in range(n_seq)]
    bwd = lambda k, t: field(k, t + 1, -1.0)
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--seqs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nx, ny = (int(x) for x in args.size.lower().split("x"))
    Q, T, P = args.seqs, args.steps, args.points

    import numpy as np
    import torch
    torch.cuda.init()
    ofx = importlib.import_module("optical-flow-1_amd")
    ctx = ofx.Ofx(0, ofx.F64)
    fwd, bwd = scene_steps(torch, nx, ny, Q, T)
    occ = torch.zeros((Q, T, ny, nx), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros((ny, nx), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k in range(Q):
        b = [bwd(k, t) for t in range(T)]
        torch.cuda.synchronize()
        ctx.flow_consistency_dev([f.data_ptr() for f in fwd[k]], [x.data_ptr() for x in b], [occ[k, t].data_ptr() for t in range(T)],
                                 [scratch.data_ptr()] * T, nx, ny)
        ctx.synchronize()
    acc = torch.zeros((Q, T, ny, nx, 2), dtype=torch.float32, device="cuda")
    oacc = torch.zeros((Q, T, ny, nx), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p_step = [[f.data_ptr() for f in fwd[k]] for k in range(Q)]
    p_occ = [[occ[k, t].data_ptr() for t in range(T)] for k in range(Q)]
    p_acc = [[acc[k, t].data_ptr() for t in range(T)] for k in range(Q)]
    p_oacc = [[oacc[k, t].data_ptr() for t in range(T)] for k in range(Q)]

    def accumulate(maps):
        ctx.flow_accumulate_dev(p_step, p_acc, nx, ny, d_occ_step=p_occ if maps else None, d_occ_acc=p_oacc if maps else None)

    variants = [False, True]
    times = {v: [] for v in variants}
    for rep in range(args.reps + 2):                                  # two warm-up rounds
        for maps in variants:
            t = timed(ctx, lambda: accumulate(maps))
            if rep >= 2:
                times[maps].append(t)
            if rep == 0 and maps:
                lost = float((oacc[:, T - 1] != 0).double().mean().item())
    result = {"tool": "bench_flow_compose", "size": [nx, ny], "seqs": Q, "steps": T, "reps": args.reps,
              "library": os.environ.get("OFX_LIB_PATH", "default"), "accumulate": [], "tracks": {}}
    px = float(nx) * ny * Q
    for maps, ts in times.items():
        b = 26 if maps else 24
        row = {"maps": maps, "ms_per_call": round(med(ts), 4), "us_per_step": round(med(ts) * 1e3 / T, 2),
               "min_max_us_per_step": [round(min(ts) * 1e3 / T, 2), round(max(ts) * 1e3 / T, 2)],
               "compulsory_bytes_per_pixel_step": b,
               "fraction_of_hbm_peak_whole_call": round(px * b * T / (med(ts) * 1e-3) / HBM_PEAK, 4)}
        if maps:
            row["share_lost_after_last_step"] = round(lost, 4)
        result["accumulate"].append(row)
    result["share_flagged_in_step_maps"] = round(float((occ != 0).double().mean().item()), 4)

    # ---- tracks ------------------------------------------------------------------------------------------------------------------
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    xy0 = torch.rand((P, 2), generator=gen, device="cuda", dtype=torch.float64) * torch.tensor([nx - 1.0, ny - 1.0], device="cuda", dtype=torch.float64)
    xy = torch.zeros((T + 1, P, 2), dtype=torch.float64, device="cuda")
    ln = torch.zeros((P,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tt = {False: [], True: []}
    for rep in range(args.reps + 2):
        for maps in (False, True):
            t = timed(ctx, lambda: ctx.flow_tracks_dev([p_step[0]], P, [xy0.data_ptr()], [xy.data_ptr()], [ln.data_ptr()], nx, ny,
                                                       d_occ_step=[p_occ[0]] if maps else None))
            if rep >= 2:
                tt[maps].append(t)
    result["tracks"] = {"points": P, "steps": T,
                        "without_maps": {"ms_per_call": round(med(tt[False]), 4), "us_per_step": round(med(tt[False]) * 1e3 / T, 2)},
                        "with_maps": {"ms_per_call": round(med(tt[True]), 4), "us_per_step": round(med(tt[True]) * 1e3 / T, 2),
                                      "Mpoint_steps_per_s": round(P * T / med(tt[True]) / 1e3, 1),
                                      "share_surviving": round(float((ln == T).double().mean().item()), 4)}}

    # ---- checks and the host route ---------------------------------------------------------------------------------------------------
    if args.check:
        import flow_compose_ref as R
        ok = {}
        accumulate(True)
        ctx.synchronize()
        chain = torch.zeros((2, ny, nx, 2), dtype=torch.float32, device="cuda")
        cocc = torch.zeros((2, ny, nx), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eq = True
        for t in range(T):                                            # in place, two sequences per call
            ks = (0, Q - 1)
            ctx.flow_compose_dev([p_step[k][t] for k in ks], [chain[n].data_ptr() for n in range(2)], nx, ny,
                                 d_flo_ab=None if t == 0 else [chain[n].data_ptr() for n in range(2)],
                                 d_occ_ab=None if t == 0 else [cocc[n].data_ptr() for n in range(2)],
                                 d_occ_bc=[p_occ[k][t] for k in ks], d_occ_ac=[cocc[n].data_ptr() for n in range(2)])
            ctx.synchronize()
            for n, k in enumerate(ks):
                eq = eq and torch.equal(chain[n].view(torch.int32), acc[k, t].view(torch.int32)) and torch.equal(cocc[n], oacc[k, t])
        ok["accumulate_equals_chained_compose"] = bool(eq)
        # the host route on sequence 0: download, numpy, upload
        t0 = time.perf_counter()
        hs = [f.cpu().numpy() for f in fwd[0]]
        hm = [occ[0, t].cpu().numpy() for t in range(T)]
        t1 = time.perf_counter()
        want = R.accumulate(hs, hm)
        t2 = time.perf_counter()
        up = [(torch.from_numpy(a).cuda(), torch.from_numpy(o).cuda()) for a, o, _ in want]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        ok["accumulate_equals_numpy_restatement"] = bool(all(
            torch.equal(up[t][0].view(torch.int32), acc[0, t].view(torch.int32)) and torch.equal(up[t][1], oacc[0, t]) for t in range(T)))
        result["host_route_one_sequence"] = {"download_ms": round((t1 - t0) * 1e3, 1), "numpy_chain_ms": round((t2 - t1) * 1e3, 1),
                                             "upload_ms": round((t3 - t2) * 1e3, 1), "total_ms": round((t3 - t0) * 1e3, 1),
                                             "total_ms_scaled_to_seqs": round((t3 - t0) * 1e3 * Q, 1)}
        n_chk = min(P, 20000)
        wxy, wl = R.tracks(hs, xy0[:n_chk].cpu().numpy(), hm)
        ok["tracks_equal_numpy_restatement"] = bool(np.array_equal(xy[:, :n_chk].cpu().numpy().view(np.int64), wxy.view(np.int64))
                                                    and np.array_equal(ln[:n_chk].cpu().numpy(), wl))
        result["checks"] = ok
        result["check"] = "ok" if all(ok.values()) else "FAILED"
    ctx.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if result.get("check", "ok") == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
