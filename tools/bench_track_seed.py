#!/usr/bin/env python3
"""Time ofx_track_structure_dev, ofx_track_seed_dev and ofx_track_sequence_dev on device-resident clips (one GPU).

    python tools/bench_track_seed.py --size 1920x1080 --clips 16 --frames 8 --rho 1 --step 4 --check [--out result.json]

The frames are a textured scene with a flat rectangle, moved by the step flows of tools/bench_flow_compose.py (scene_steps), as
8-bit and as double frames; the maps are ofx_flow_consistency_dev's on those steps and their true backward flows.  Variants
alternate in one process; a figure is the median of `reps` calls, each with the context synchronised inside the timed region.
structure: lam2 of `clips` frames in one launch (no mean), 8-bit and double frames.  The compulsory traffic is the frame element +
8 B per pixel; the fraction of the HBM peak is that over the whole call's time.  The arithmetic is counted as well: per pixel
and plane the row pass is 6 multiplications and 10 additions on 42 / 32 rows, the column pass the same, in double with no
contraction (111 for the three planes), about 17 for the gradients and products of the 74 x 42 cells of a 64 x 32 tile and about 25
for the eigenvalue with its square root: about 150 FP64 instructions per pixel -- against 9 or 16 bytes.
seed: the seeds of `clips` frames per call (structure, mean, occupancy, count / scan / scatter).
sequence: the whole pipeline over `clips` clips, per step, against ofx_flow_tracks_dev from the seeds of frame 0 alone.
--check: lam2, the mean and the seeds of clip 0's first frame equal the numpy restatement (tests/track_seed_ref.py) bit for
bit, and so does the sequence entry on the first 3 frames of clip 0; the slots born at frame 0 equal ofx_flow_tracks_dev.  The
restatement's run on that frame is also the comparison: the HOST ROUTE -- download the frame, numpy, upload the points -- timed
once and scaled to clips x frames.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_flow_compose import HBM_PEAK, med, scene_steps, timed  # noqa: E402

FP64_OPS_PER_PIXEL = 150


def scene_frames(torch, nx, ny, fwd, n_clips, n_frames):
    """frame 0 of clip k: a texture with a flat rectangle; frame t + 1 = frame t pulled back along step t (nearest pixel).  -> uint8
    tensor (clips, frames, ny, nx)"""
    f64 = torch.float64
    i, j = torch.meshgrid(torch.arange(ny, dtype=f64, device="cuda"), torch.arange(nx, dtype=f64, device="cuda"), indexing="ij")
    out = torch.zeros((n_clips, n_frames, ny, nx), dtype=torch.uint8, device="cuda")
    for k in range(n_clips):
        ph = 0.3 + 0.1 * k
        tex = (127.5 + 40 * torch.sin(0.11 * j + ph) * torch.cos(0.07 * i) + 30 * torch.sin(0.31 * j + 0.43 * i) + 25 * torch.cos(0.19 * i - 0.5 * j)
               + 20 * torch.sin(0.37 * j) * torch.sin(0.29 * i))
        tex[ny // 8:ny // 8 + ny // 3, nx // 2:nx // 2 + nx // 3] = 90.0
        cur = torch.floor(tex).clamp(0, 255)
        out[k, 0] = cur.to(torch.uint8)
        for t in range(n_frames - 1):
            u, v = fwd[k][t][..., 0].double(), fwd[k][t][..., 1].double()
            sj = (j - u).round().clamp(0, nx - 1).long()
            si = (i - v).round().clamp(0, ny - 1).long()
            cur = cur[si, sj]
            out[k, t + 1] = cur.to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rho", type=float, default=1.0)
    ap.add_argument("--frac", type=float, default=0.1)
    ap.add_argument("--step", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nx, ny = (int(x) for x in args.size.lower().split("x"))
    Q, F, T = args.clips, args.frames, args.frames - 1
    rho, frac, step = args.rho, args.frac, args.step

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
    fr8 = scene_frames(torch, nx, ny, fwd, Q, F)
    fr64 = fr8[:, 0].double().contiguous()
    ncx, ncy = (nx - 1) // step + 1, (ny - 1) // step + 1
    cap = 2 * ncx * ncy
    lam2 = torch.zeros((Q, ny, nx), dtype=torch.float64, device="cuda")
    sxy = torch.zeros((Q, cap, 2), dtype=torch.float64, device="cuda")
    scount = torch.zeros((Q, 2), dtype=torch.int32, device="cuda")
    xy = torch.zeros((Q, F, cap, 2), dtype=torch.float64, device="cuda")
    t0 = torch.zeros((Q, cap), dtype=torch.int32, device="cuda")
    ln = torch.zeros((Q, cap), dtype=torch.int32, device="cuda")
    count = torch.zeros((Q, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p8 = [[fr8[k, f].data_ptr() for f in range(F)] for k in range(Q)]
    p64 = [fr64[k].data_ptr() for k in range(Q)]
    p_step = [[f.data_ptr() for f in fwd[k]] for k in range(Q)]
    p_occ = [[occ[k, t].data_ptr() for t in range(T)] for k in range(Q)]
    rows = lambda t: [t[k].data_ptr() for k in range(Q)]
    result = {"tool": "bench_track_seed", "size": [nx, ny], "clips": Q, "frames": F, "rho": rho, "frac": frac, "step": step, "cap": cap,
              "reps": args.reps, "library": os.environ.get("OFX_LIB_PATH", "default")}

    def with_input(kind, call):
        ctx.set_option("input", kind)
        try:
            return timed(ctx, call)
        finally:
            ctx.set_option("input", 0)

    # ---- the structure pass and the seed call, 8-bit and double frames alternated -------------------------------------------------
    calls = {"structure_u8": (1, lambda: ctx.track_structure_dev([p[0] for p in p8], nx, ny, rho, d_lam2=rows(lam2))),
             "structure_f64": (0, lambda: ctx.track_structure_dev(p64, nx, ny, rho, d_lam2=rows(lam2))),
             "seed_u8": (1, lambda: ctx.track_seed_dev([p[0] for p in p8], rows(sxy), rows(scount), cap, nx, ny, rho, frac, step)),
             "seed_f64": (0, lambda: ctx.track_seed_dev(p64, rows(sxy), rows(scount), cap, nx, ny, rho, frac, step))}
    times = {k: [] for k in calls}
    for rep in range(args.reps + 2):                                  # two warm-up rounds
        for name, (kind, call) in calls.items():
            t = with_input(kind, call)
            if rep >= 2:
                times[name].append(t)
    px = float(nx) * ny
    for name, ts in times.items():
        row = {"ms_per_call": round(med(ts), 4), "us_per_frame": round(med(ts) * 1e3 / Q, 2),
               "min_max_us_per_frame": [round(min(ts) * 1e3 / Q, 2), round(max(ts) * 1e3 / Q, 2)]}
        if name.startswith("structure"):
            b = 9 if name.endswith("u8") else 16
            row["compulsory_bytes_per_pixel"] = b
            row["fraction_of_hbm_peak_whole_call"] = round(px * Q * b / (med(ts) * 1e-3) / HBM_PEAK, 4)
            row["fp64_instructions_per_s"] = round(px * Q * FP64_OPS_PER_PIXEL / (med(ts) * 1e-3), 0)
        result[name] = row
    result["seeds_per_frame"] = [int(x) for x in scount[:, 0].cpu().numpy()]

    # ---- the sequence entry against flow_tracks on the seeds of frame 0 alone ------------------------------------------------------
    n0 = int(scount[:, 0].min().item())
    txy = torch.zeros((Q, F, n0, 2), dtype=torch.float64, device="cuda")
    tln = torch.zeros((Q, n0), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    seqs = {"sequence": (1, lambda: ctx.track_sequence_dev(p8, p_step, cap, rows(xy), rows(t0), rows(ln), rows(count), nx, ny, rho, frac, step,
                                                           d_occ_step=p_occ)),
            "tracks_from_frame_0_seeds": (0, lambda: ctx.flow_tracks_dev(p_step, n0, rows(sxy), rows(txy), rows(tln), nx, ny, d_occ_step=p_occ))}
    times = {k: [] for k in seqs}
    for rep in range(args.reps + 2):
        for name, (kind, call) in seqs.items():
            t = with_input(kind, call)
            if rep >= 2:
                times[name].append(t)
    for name, ts in times.items():
        result[name] = {"ms_per_call": round(med(ts), 4), "us_per_step": round(med(ts) * 1e3 / T, 2),
                        "min_max_us_per_step": [round(min(ts) * 1e3 / T, 2), round(max(ts) * 1e3 / T, 2)]}
    c = count.cpu().numpy()
    alive_end = ((t0 + ln) >= F - 1) & (torch.arange(cap, device="cuda")[None, :] < count[:, :1])
    result["sequence"].update({"tracks_per_clip": [int(x) for x in c[:, 0]], "dropped_per_clip": [int(x) for x in c[:, 1]],
                               "live_at_last_frame_per_clip": [int(x) for x in alive_end.sum(dim=1).cpu().numpy()]})
    result["tracks_from_frame_0_seeds"].update({"points_per_clip": n0,
                                                "live_at_last_frame_per_clip": [int(x) for x in (tln == T).sum(dim=1).cpu().numpy()]})

    # ---- checks and the host route ---------------------------------------------------------------------------------------------------
    if args.check:
        import oracle
        import track_seed_ref as R
        if not os.path.exists(oracle.ORACLE_SO):
            oracle.build()
        orc = oracle.Oracle()
        orc.set_num_threads(1)
        ok = {}
        mean = torch.zeros((1,), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.set_option("input", 1)
        ctx.track_structure_dev([p8[0][0]], nx, ny, rho, d_lam2=[lam2[0].data_ptr()], d_mean=[mean.data_ptr()])
        ctx.track_seed_dev([p8[0][0]], [sxy[0].data_ptr()], [scount[0].data_ptr()], cap, nx, ny, rho, frac, step)
        ctx.synchronize()
        # the host route on one frame: download, numpy, upload
        ta = time.perf_counter()
        h = fr8[0, 0].cpu().numpy().astype(np.float64)
        tb = time.perf_counter()
        l2, m = R.structure(orc, h, rho)
        pts, written, dropped = R.seeds(l2, m, frac, step, cap=cap)
        tc = time.perf_counter()
        up = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        td = time.perf_counter()
        result["host_route_one_frame"] = {"download_ms": round((tb - ta) * 1e3, 1), "numpy_ms": round((tc - tb) * 1e3, 1),
                                          "upload_ms": round((td - tc) * 1e3, 1), "total_ms": round((td - ta) * 1e3, 1),
                                          "total_ms_scaled_to_clips_x_frames": round((td - ta) * 1e3 * Q * F, 1)}
        ok["lam2_equals_numpy_restatement"] = bool(lam2[0].cpu().numpy().tobytes() == l2.tobytes())
        ok["mean_equals_numpy_restatement"] = bool(mean.cpu().numpy()[0].tobytes() == np.float64(m).tobytes())
        sc = scount[0].cpu().numpy()
        ok["seeds_equal_numpy_restatement"] = bool(tuple(sc) == (written, dropped) and torch.equal(up, sxy[0, :written]))
        # the sequence entry on the first 3 frames of clip 0
        ctx.track_sequence_dev([p8[0][:3]], [p_step[0][:2]], cap, [xy[0].data_ptr()], [t0[0].data_ptr()], [ln[0].data_ptr()],
                               [count[0].data_ptr()], nx, ny, rho, frac, step, d_occ_step=[p_occ[0][:2]])
        ctx.synchronize()
        used = int(count[0, 0].item())
        g_xy = xy[0].reshape(-1)[:3 * cap * 2].reshape(3, cap, 2)[:, :used].cpu().numpy()
        g_t0, g_ln = t0[0, :used].cpu().numpy(), ln[0, :used].cpu().numpy()
        want = R.sequence(orc, [fr8[0, f].cpu().numpy().astype(np.float64) for f in range(3)], [fwd[0][t].cpu().numpy() for t in range(2)],
                          [occ[0, t].cpu().numpy() for t in range(2)], cap, rho, frac, step)
        ok["sequence_equals_numpy_restatement"] = bool(used == want["count"][0] and int(count[0, 1].item()) == want["count"][1]
                                                       and np.ascontiguousarray(g_xy).tobytes() == want["xy"].tobytes()
                                                       and np.array_equal(g_t0, want["t0"]) and np.array_equal(g_ln, want["len"]))
        born0 = g_t0 == 0
        nb = int(born0.sum())
        s0 = torch.from_numpy(np.ascontiguousarray(g_xy[0][born0])).cuda()
        cxy = torch.zeros((3, nb, 2), dtype=torch.float64, device="cuda")
        cln = torch.zeros((nb,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.set_option("input", 0)
        ctx.flow_tracks_dev([p_step[0][:2]], nb, [s0.data_ptr()], [cxy.data_ptr()], [cln.data_ptr()], nx, ny, d_occ_step=[p_occ[0][:2]])
        ctx.synchronize()
        ok["slots_born_at_frame_0_equal_flow_tracks"] = bool(cxy.cpu().numpy().tobytes() == np.ascontiguousarray(g_xy[:, born0]).tobytes()
                                                             and np.array_equal(cln.cpu().numpy(), g_ln[born0]))
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
