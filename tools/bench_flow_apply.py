#!/usr/bin/env python3
"""Time ofx_flow_warp_dev and ofx_flow_interpolate_dev on device-resident frames (one GPU).

    python tools/bench_flow_apply.py --size 1920x1080 --slots 8 --check [--out result.json]

Two formats: 8-bit frames of three interleaved channels (OFX_IN_U8, nz = 3) and double planes (nz = 1), `slots` distinct pairs of
the synthetic P1 scene made on the device.  The payloads are the scene's own motion (a smooth background flow of about 1.5 px, a
foreground rectangle moving by (4 + k, -3), so every frame has a motion boundary) and its negative; the warp takes the maps of
ofx_flow_consistency_dev on them and the first frame as fill.  Option apply_lds = 1 (LDS tiles) and 0 (global gathers) alternate in one
process -- the default, 2, is one of them by the element's size; a figure is the
median of `reps` calls, each with the context synchronised inside the timed region.  Prints one JSON line.

--check: the results of apply_lds = 1 and 0 are equal, a zero payload returns the source and t = 0 / t = 1 return A / B."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                      # bytes / s
FP64_ISSUE = 256 * 64 * 2.4e9          # lane-operations / s: 256 CUs, one 64-lane FP64 instruction per 4 cycles on each of 4 SIMDs
CELL = 19                              # double operations of one cubic_cell


def ops_per_pixel(entry, nz):
    """counted double operations: 5 cubic_cell per channel and source, the positions and fractions, the blend"""
    if entry == "warp":
        return 5 * CELL * nz + 6
    return 2 * 5 * CELL * nz + 3 * nz + 22


def bytes_per_pixel(entry, nz, esize):
    """compulsory traffic: every source element and payload read once, the result written once (+ the map for the warp)"""
    if entry == "warp":
        return esize * nz + 8 + 1 + esize * nz
    return 2 * esize * nz + 16 + esize * nz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--t", type=float, default=0.5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nx, ny = (int(x) for x in args.size.lower().split("x"))
    n = args.slots

    import torch
    torch.cuda.init()
    ofx = importlib.import_module("optical-flow-1_amd")
    synth = importlib.import_module("optical-flow-1_amd.synth")
    ctx = ofx.Ofx(0, ofx.F64)
    dev = "cuda"
    f64 = torch.float64

    i, j = torch.meshgrid(torch.arange(ny, dtype=f64, device=dev), torch.arange(nx, dtype=f64, device=dev), indexing="ij")
    pairs, fwd, bwd = [], [], []
    for k in range(n):
        pairs.append(synth.pair_device("P1", nx, ny, k, dev))
        fx, fy = 1.5 + 0.5 * torch.sin(0.01 * i), -0.75 + 0.25 * torch.cos(0.013 * j)
        fg = (j >= nx // 4) & (j < nx // 2) & (i >= ny // 4) & (i < ny // 2)
        u = torch.where(fg, torch.full_like(fx, 4.0 + (k % 3)), fx)
        v = torch.where(fg, torch.full_like(fy, -3.0), fy)
        fwd.append(torch.stack([u, v], dim=-1).to(torch.float32).contiguous())
        bwd.append((-fwd[-1]).contiguous())
    occ = [torch.zeros((2, ny, nx), dtype=torch.uint8, device=dev) for _ in range(n)]
    torch.cuda.synchronize()               # torch made the inputs on its own stream; the library runs on the context's
    ctx.flow_consistency_dev([f.data_ptr() for f in fwd], [b.data_ptr() for b in bwd], [o[0].data_ptr() for o in occ],
                             [o[1].data_ptr() for o in occ], nx, ny)
    ctx.synchronize()
    flagged = float(sum((o[0] != 0).double().mean().item() for o in occ) / n)

    def frames(kind):
        out = []
        for A, B in pairs:
            if kind == "f64":
                out.append((A.reshape(ny, nx, 1).contiguous(), B.reshape(ny, nx, 1).contiguous()))
            else:
                def rgb(p):
                    p = p.clamp(0.0, 255.0)
                    return torch.stack([p, 255.0 - p, p * p / 255.0], dim=-1).to(torch.uint8).contiguous()
                out.append((rgb(A), rgb(B)))
        return out

    result = {"tool": "bench_flow_apply", "size": [nx, ny], "slots": n, "reps": args.reps, "t": args.t,
              "share_flagged_forward": round(flagged, 4), "cases": []}
    ts = [args.t] * n
    for kind, nz, inp, esize in (("u8", 3, 1, 1), ("f64", 1, 0, 8)):
        fr = frames(kind)
        dst = [torch.zeros_like(a) for a, _ in fr]
        zero = [torch.zeros_like(f) for f in fwd]
        torch.cuda.synchronize()
        ptr = lambda xs: [x.data_ptr() for x in xs]
        pa, pb, pd = ptr([a for a, _ in fr]), ptr([b for _, b in fr]), ptr(dst)
        pf, pw, po = ptr(fwd), ptr(bwd), [o[0].data_ptr() for o in occ]
        ctx.set_option("input", inp)
        calls = {
            "warp": lambda: ctx.flow_warp_dev(pb, pf, pd, nx, ny, nz, d_occ=po, dFill=pa),
            "interpolate": lambda: ctx.flow_interpolate_dev(pa, pb, pf, pw, ts, pd, nx, ny, nz),
        }
        for entry, call in calls.items():
            times = {1: [], 0: []}
            kept = {}
            for rep in range(args.reps + 2):                       # two warm-up rounds
                for lds in (1, 0):
                    ctx.set_option("apply_lds", lds)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    call()
                    ctx.synchronize()
                    t1 = time.perf_counter()
                    if rep >= 2:
                        times[lds].append((t1 - t0) * 1e3)
                    if args.check and rep == 0:
                        kept[lds] = [d.clone() for d in dst]
            ctx.set_option("apply_lds", 2)
            med = {lds: sorted(v)[len(v) // 2] for lds, v in times.items()}
            px = float(nx) * ny * n
            best = min(med.values())
            case = {"frames": kind, "nz": nz, "entry": entry,
                    "ms_apply_lds_1": round(med[1], 4), "ms_apply_lds_0": round(med[0], 4),
                    "min_max_ms_apply_lds_1": [round(min(times[1]), 4), round(max(times[1]), 4)],
                    "min_max_ms_apply_lds_0": [round(min(times[0]), 4), round(max(times[0]), 4)],
                    "Mpix_per_s": round(px / best / 1e3, 1),
                    "compulsory_bytes_per_pixel": bytes_per_pixel(entry, nz, esize),
                    "fraction_of_hbm_peak_whole_call": round(px * bytes_per_pixel(entry, nz, esize) / (best * 1e-3) / HBM_PEAK, 4),
                    "double_ops_per_pixel": ops_per_pixel(entry, nz),
                    "fraction_of_fp64_issue_whole_call": round(px * ops_per_pixel(entry, nz) / (best * 1e-3) / FP64_ISSUE, 4)}
            if args.check:
                case["apply_lds_results_equal"] = all(torch.equal(x, y) for x, y in zip(kept[1], kept[0]))
            result["cases"].append(case)
        if args.check:
            ctx.flow_warp_dev(pb, ptr(zero), pd, nx, ny, nz)
            ctx.synchronize()
            ok = all(torch.equal(d, b) for d, (_, b) in zip(dst, fr))
            ctx.flow_interpolate_dev(pa, pb, pf, pw, [0.0] * n, pd, nx, ny, nz)
            ctx.synchronize()
            ok = ok and all(torch.equal(d, a) for d, (a, _) in zip(dst, fr))
            ctx.flow_interpolate_dev(pa, pb, pf, pw, [1.0] * n, pd, nx, ny, nz)
            ctx.synchronize()
            ok = ok and all(torch.equal(d, b) for d, (_, b) in zip(dst, fr))
            result["cases"][-1]["identities_hold"] = result["cases"][-2]["identities_hold"] = bool(ok)
        ctx.set_option("input", 0)
    if args.check:
        result["check"] = "ok" if all(c.get("apply_lds_results_equal") and c.get("identities_hold") for c in result["cases"]) else "FAILED"
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if result.get("check", "ok") == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
