#!/usr/bin/env python3
"""Time ofx_flow_error_dev, ofx_flow_encode_dev and ofx_flow_decode_dev on device-resident payloads (one GPU).

    python tools/bench_flow_measure.py --size 1920x1080 --slots 16 --check [--ab variants/libofx_parent.so] [--out result.json]

The truths are a smooth field (another one per slot), the estimates that field with noise of 0.8 px per component and a block that
is 6 px off; the maps flag a tenth of the pixels.  Variants alternate in one process; a figure is the median of `reps` calls, each
with the context synchronised inside the timed region.
error: the call with six thresholds, without and with maps, with the EPE map, with the histogram (4096 bins of 1/64 px, counted in
LDS; 8192 bins, counted in memory) and with both.  The compulsory traffic of the statistics alone is the two payloads, 16 B per
pixel, 17 B with a map; the EPE map adds 4 B written.  The arithmetic is counted as well: about 40 FP64 operations per pixel as
written, among them five square roots and a division, and the device library's acos.
encodings: the colour wheel at a given radius and at the payload's own (one more pass over the payload: 8 B read + 3 B written,
16 B + 3 B), the bounded 8-bit coding (8 B + 2 B), the 16-bit coding (8 B + 6 B) and the two decodings.
--check: the record, the EPE map and the histogram of slot 0, the BOUND and KITTI codings and their decodings equal the numpy
restatement (tests/flow_measure_ref.py) bit for bit, the angular entries to 1e-12, the wheel under the three-way rule.  The HOST
ROUTE each call replaces -- download the two payloads, numpy (np.hypot, np.mean, np.histogram; the restatement's wheel), upload of
the picture -- is timed once on slot 0 and scaled to the slots.
--ab: bench.py with that library (the parent commit's build) and this one in turn (tools/ab_bench.py), its output appended.
Prints one JSON line."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_flow_compose import HBM_PEAK, med, timed  # noqa: E402

FP64_OPS_PER_PIXEL = 40
THR_ABS = (0.5, 1.0, 2.0, 3.0, 5.0, 3.0)
THR_REL = (0.0, 0.0, 0.0, 0.0, 0.0, 0.05)


def scene(torch, nx, ny, slots):
    """-> estimates, truths (slots, ny, nx, 2) float32 and maps (slots, ny, nx) uint8 on the device"""
    f64 = torch.float64
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    i, j = torch.meshgrid(torch.arange(ny, dtype=f64, device="cuda"), torch.arange(nx, dtype=f64, device="cuda"), indexing="ij")
    gt = torch.zeros((slots, ny, nx, 2), dtype=torch.float32, device="cuda")
    flo = torch.zeros_like(gt)
    for k in range(slots):
        u = 6 * torch.sin(0.011 * j + 0.005 * i + 0.1 * k) + 0.003 * (j - nx / 2)
        v = 4 * torch.cos(0.007 * i - 0.002 * j) - 0.002 * (i - ny / 2) + 0.05 * k
        gt[k, ..., 0], gt[k, ..., 1] = u.float(), v.float()
        nu, nv = (0.8 * torch.randn((ny, nx), dtype=f64, device="cuda", generator=g) for _ in range(2))
        nu[: ny // 3, : nx // 4] += 6.0
        flo[k, ..., 0], flo[k, ..., 1] = (u + nu).float(), (v + nv).float()
    occ = (torch.rand((slots, ny, nx), device="cuda", generator=g) < 0.1).to(torch.uint8) * 255
    return flo, gt, occ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--ab", default=None, help="the parent commit's libofx.so, relative to the repository: bench.py with it and with this build in turn")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nx, ny = (int(x) for x in args.size.lower().split("x"))
    Q = args.slots
    NB, BW = 4096, 1.0 / 64

    import numpy as np
    import torch
    torch.cuda.init()
    ofx = importlib.import_module("optical-flow-1_amd")
    ctx = ofx.Ofx(0, ofx.F64)
    flo, gt, occ = scene(torch, nx, ny, Q)
    rec = torch.zeros((Q, 16), dtype=torch.float64, device="cuda")
    epe = torch.zeros((Q, ny, nx), dtype=torch.float32, device="cuda")
    hist = torch.zeros((Q, 2 * NB), dtype=torch.int32, device="cuda")
    rgb = torch.zeros((Q, ny, nx, 3), dtype=torch.uint8, device="cuda")
    b8 = torch.zeros((Q, ny, nx, 2), dtype=torch.uint8, device="cuda")
    k16 = torch.zeros((Q, ny, nx, 3), dtype=torch.int16, device="cuda")
    back = torch.zeros((Q, ny, nx, 2), dtype=torch.float32, device="cuda")
    bmap = torch.zeros((Q, ny, nx), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rows = lambda t: [t[k].data_ptr() for k in range(Q)]
    result = {"tool": "bench_flow_measure", "size": [nx, ny], "slots": Q, "thresholds": len(THR_ABS), "n_bins": NB, "bin_w": BW,
              "reps": args.reps, "library": os.environ.get("OFX_LIB_PATH", "default")}

    def err(maps=False, e=False, h=0):
        return lambda: ctx.flow_error_dev(rows(flo), rows(gt), rows(rec), nx, ny, thr_abs=THR_ABS, thr_rel=THR_REL,
                                          d_occ=rows(occ) if maps else None, d_epe=rows(epe) if e else None,
                                          d_hist=rows(hist) if h else None, n_bins=h, bin_w=BW)

    def enc(kind, scale, maps=False):
        dst = {ofx.ENC_WHEEL_RGB8: rgb, ofx.ENC_BOUND_U8: b8, ofx.ENC_KITTI_U16: k16}[kind]
        return lambda: ctx.flow_encode_dev(rows(flo), rows(dst), nx, ny, kind=kind, scale=scale, d_occ=rows(occ) if maps else None)

    # name -> (call, compulsory bytes per pixel)
    calls = {"error": (err(), 16), "error_maps": (err(True), 17), "error_epe": (err(e=True), 20), "error_hist_lds": (err(h=NB), 16),
             "error_hist_memory": (err(h=2 * NB), 16), "error_maps_epe_hist": (err(True, True, NB), 21),
             "wheel_given_radius": (enc(ofx.ENC_WHEEL_RGB8, 8.0), 11), "wheel_own_radius": (enc(ofx.ENC_WHEEL_RGB8, 0.0), 19),
             "wheel_own_radius_maps": (enc(ofx.ENC_WHEEL_RGB8, 0.0, True), 21),
             "bound_u8": (enc(ofx.ENC_BOUND_U8, 20.0), 10), "kitti_u16": (enc(ofx.ENC_KITTI_U16, 0.0), 14),
             "decode_bound_u8": (lambda: ctx.flow_decode_dev(rows(b8), rows(back), nx, ny, kind=ofx.ENC_BOUND_U8, scale=20.0), 10),
             "decode_kitti_u16": (lambda: ctx.flow_decode_dev(rows(k16), rows(back), nx, ny, kind=ofx.ENC_KITTI_U16,
                                                              d_occ=rows(bmap)), 15)}
    times = {k: [] for k in calls}
    for rep in range(args.reps + 2):                                  # two warm-up rounds
        for name, (call, _) in calls.items():
            t = timed(ctx, call)
            if rep >= 2:
                times[name].append(t)
    px = float(nx) * ny * Q
    for name, ts in times.items():
        b = calls[name][1]
        result[name] = {"ms_per_call": round(med(ts), 4), "min_max_ms": [round(min(ts), 4), round(max(ts), 4)],
                        "us_per_slot": round(med(ts) * 1e3 / Q, 2), "compulsory_bytes_per_pixel": b,
                        "fraction_of_hbm_peak_whole_call": round(px * b / (med(ts) * 1e-3) / HBM_PEAK, 4)}
    result["error"]["fp64_operations_per_s"] = round(px * FP64_OPS_PER_PIXEL / (med(times["error"]) * 1e-3), 0)

    if args.check:
        import flow_measure_ref as R
        ok = {}
        err(True, True, NB)()
        enc(ofx.ENC_WHEEL_RGB8, 0.0, True)()
        enc(ofx.ENC_BOUND_U8, 20.0)()
        enc(ofx.ENC_KITTI_U16, 0.0)()
        ctx.synchronize()
        g_rec, g_epe, g_hist = rec[0].cpu().numpy(), epe[0].cpu().numpy(), hist[0, :NB].cpu().numpy().view(np.uint32)
        g_rgb, g_b8, g_k16 = rgb[0].cpu().numpy(), b8[0].cpu().numpy(), k16[0].cpu().numpy().view(np.uint16)
        # the host route of the statistics of one slot: download, numpy, nothing to upload
        ta = time.perf_counter()
        h_flo, h_gt = flo[0].cpu().numpy(), gt[0].cpu().numpy()
        tb = time.perf_counter()
        e = np.hypot(h_flo[..., 0].astype(np.float64) - h_gt[..., 0], h_flo[..., 1].astype(np.float64) - h_gt[..., 1])
        figures = [e.mean(), np.sqrt((e * e).mean())] + [(e > t).mean() for t in THR_ABS] + [np.histogram(e, bins=NB, range=(0.0, NB * BW))[0]]
        tc = time.perf_counter()
        del figures
        result["host_route_error_one_slot"] = {"download_ms": round((tb - ta) * 1e3, 1), "numpy_ms": round((tc - tb) * 1e3, 1),
                                               "total_ms": round((tc - ta) * 1e3, 1), "total_ms_scaled_to_slots": round((tc - ta) * 1e3 * Q, 1)}
        h_occ = occ[0].cpu().numpy()
        # ... and of the picture: download, the restatement's wheel (vectorised numpy), upload
        ta = time.perf_counter()
        h2 = flo[0].cpu().numpy()
        tb = time.perf_counter()
        w_rgb = R.encode_wheel(h2, h_occ, 0.0)
        tc = time.perf_counter()
        up = torch.from_numpy(w_rgb).cuda()
        torch.cuda.synchronize()
        td = time.perf_counter()
        del up
        result["host_route_wheel_one_slot"] = {"download_ms": round((tb - ta) * 1e3, 1), "numpy_ms": round((tc - tb) * 1e3, 1),
                                               "upload_ms": round((td - tc) * 1e3, 1), "total_ms": round((td - ta) * 1e3, 1),
                                               "total_ms_scaled_to_slots": round((td - ta) * 1e3 * Q, 1)}
        w_rec, w_epe, w_hist = R.error(h_flo, h_gt, h_occ, THR_ABS, THR_REL, NB, BW)
        exact = [0, 1, 2, 3, 5, 6] + list(range(8, 16))
        ok["record_equals_numpy_restatement"] = bool(g_rec[exact].tobytes() == w_rec[exact].tobytes())
        dev = max(abs(g_rec[k] - w_rec[k]) / w_rec[k] for k in (4, 7))
        result["angular_entries_largest_relative_deviation"] = float(dev)
        ok["angular_entries_within_1e-12"] = bool(dev <= 1e-12)
        ok["epe_map_equals_numpy_restatement"] = bool(g_epe.tobytes() == w_epe.tobytes())
        ok["histogram_equals_numpy_restatement"] = bool(g_hist.tobytes() == w_hist.tobytes())
        good, exempt = R.wheel_ok(g_rgb, h_flo, h_occ, 0.0)
        ok["wheel_under_the_three_way_rule"] = bool(good)
        result["wheel_pixels_exempted"] = exempt
        result["wheel_pixels_that_differ_from_the_plain_restatement"] = int((g_rgb != w_rgb).any(axis=-1).sum())
        ok["bound_equals_numpy_restatement"] = bool(g_b8.tobytes() == R.encode_bound(h_flo, None, 20.0).tobytes())
        ok["kitti_equals_numpy_restatement"] = bool(g_k16.tobytes() == R.encode_kitti(h_flo, None).tobytes())
        calls["decode_kitti_u16"][0]()
        ctx.synchronize()
        wf, wm = R.decode_kitti(g_k16)
        ok["kitti_decoding_equals_numpy_restatement"] = bool(back[0].cpu().numpy().tobytes() == wf.tobytes() and
                                                             bmap[0].cpu().numpy().tobytes() == wm.tobytes())
        calls["decode_bound_u8"][0]()
        ctx.synchronize()
        ok["bound_decoding_equals_numpy_restatement"] = bool(back[0].cpu().numpy().tobytes() == R.decode_bound(g_b8, 20.0)[0].tobytes())
        result["slot_0"] = {"aepe_px": round(float(g_rec[2]), 5), "aae_deg": round(float(g_rec[4]), 4),
                            "r1": round(float(g_rec[9] / g_rec[0]), 4), "fl": round(float(g_rec[13] / g_rec[0]), 4)}
        result["checks"] = ok
        result["check"] = "ok" if all(ok.values()) else "FAILED"
    ctx.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.ab:
        this = os.path.relpath(ofx.LIB_PATH, ROOT)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_bench.py"), "parent=" + args.ab, "this=" + this, "--rounds", "3",
                            "--args", "--no-cpu --no-sor --no-occ --no-4k --no-cli --no-other-mode"], capture_output=True, text=True)
        print(p.stdout + p.stderr[-2000:])
        if args.out:
            with open(os.path.splitext(args.out)[0] + "_ab.txt", "w") as f:
                f.write(p.stdout)
    return 0 if result.get("check", "ok") == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
