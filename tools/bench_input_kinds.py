#!/usr/bin/env python3
"""The normalisation head on frames of the byte kinds (context option "input") against the storage type, alone and in a solve.
    python tools/bench_input_kinds.py [--size 1920x1080] [--pairs 16] [--reps 9] [--solve-pairs 5] [--pitch P] [--check] [--out FILE]
ofx_normalize_frames_dev on `pairs` sets of two frames (2 * pairs frames) for the storage type (the yardstick: code the input
kinds do not touch, timed in the same run), U8, U16 and RGB8, each through the four-elements-per-lane kernels (the default;
the 256 quotients of an 8-bit kind from an LDS table), those with input_lut = 0 and the one-element-per-thread kernels
(input_vec = 0): median of `reps` runs after warm-up, each between two stream synchronisations.  GB/s is on the compulsory
bytes per pixel: the source read twice (min / max, map) and the result written once.
Then ofx_tvl1_group_dev on `solve-pairs` pairs from U8 frames against the same values as doubles.  --check: every result must
equal the storage-type result bit for bit, and each integer kind's median must not exceed the storage type's (exit status 1).
--pitch P adds, beside every dense figure, the same frames with their rows P apart (context option "input_pitch") through
ofx_normalize_frames2d_dev, and the solve from pitched U8 frames: P = a number of bytes, `align256` for the row's bytes rounded up to
256 (a decoder's surface), `row+1` for the row's bytes plus one unit of the element's alignment (every row at another alignment).
Every pitched result must equal the dense one bit for bit under --check; the times are reported, not judged.
One JSON line; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                    # torch brings its own HIP runtime and has to see the device before libofx.so does

torch.cuda.init()
ofx = importlib.import_module("optical-flow-1_amd")
synth = importlib.import_module("optical-flow-1_amd.synth")

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--pairs", type=int, default=16)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--solve-pairs", type=int, default=5)
ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
ap.add_argument("--pitch", default="")
ap.add_argument("--check", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
nx, ny = (int(v) for v in a.size.split("x"))
npix, nfr = nx * ny, 2 * a.pairs
prec = ofx.F64 if a.precision == "f64" else ofx.F32
st_np, st_t = (np.float64, torch.float64) if a.precision == "f64" else (np.float32, torch.float32)
ctx = ofx.Ofx(0, prec)


def gray(rgb):
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    s = .299 * r + .587 * g
    return (s + .114 * b).astype(np.uint8)


seq = synth.sequence(nx, ny, 4, 1).astype(np.uint8)
u8 = np.stack([np.roll(seq[k % 4], 7 * (k // 4), axis=1) for k in range(nfr)])                   # 2 * pairs distinct frames
sources = {"U8": u8, "U16": u8.astype(np.uint16) * 257, "RGB8": np.stack([u8, np.roll(u8, 5, axis=-1), 255 - u8], axis=-1)}
values = {"U8": u8, "U16": sources["U16"], "RGB8": gray(sources["RGB8"])}
src_bytes = {"STORAGE": np.dtype(st_np).itemsize, "U8": 1, "U16": 2, "RGB8": 3}
dst = torch.zeros((nfr, npix), dtype=st_t, device="cuda")
d_ptr = [dst[k].data_ptr() for k in range(nfr)]


def pitch_of(kind):
    """--pitch for rows of `kind` -> bytes"""
    row, unit = nx * src_bytes[kind], {"STORAGE": np.dtype(st_np).itemsize, "U8": 1, "U16": 2, "RGB8": 1}[kind]
    if a.pitch == "align256":
        return (row + 255) // 256 * 256
    return row + unit if a.pitch == "row+1" else int(a.pitch)


def pitched(frames, pitch):
    """the frames (nfr, ny, ...) as a device byte tensor (nfr, ny, pitch), the padding zero"""
    rows = np.ascontiguousarray(frames).view(np.uint8).reshape(frames.shape[0], ny, -1)
    buf = torch.zeros((frames.shape[0], ny, pitch), dtype=torch.uint8, device="cuda")
    buf[:, :, :rows.shape[2]] = torch.from_numpy(rows).cuda()
    return buf


def timed(kind, dev, vec, lut=1, pitch=0):
    ctx.set_option("input", getattr(ofx, "IN_" + kind))
    ctx.set_option("input_vec", vec)
    ctx.set_option("input_lut", lut)
    ptr = [dev[k].data_ptr() for k in range(nfr)]
    run = lambda: ctx.normalize_frames_dev(ptr, d_ptr, npix, per=2)
    if pitch:
        ctx.set_option("input_pitch", pitch)
        run = lambda: ctx.normalize_frames2d_dev(ptr, d_ptr, nx, ny, per=2)
    for _ in range(3):
        run()
    ctx.synchronize()
    reps = []
    for _ in range(a.reps):
        ctx.synchronize()
        t = time.perf_counter()
        run()
        ctx.synchronize()
        reps.append(time.perf_counter() - t)
    ctx.set_option("input", ofx.IN_STORAGE)
    ctx.set_option("input_vec", 1)
    ctx.set_option("input_lut", 1)
    if pitch:
        ctx.set_option("input_pitch", 0)
    med = sorted(reps)[len(reps) // 2]
    bytes_px = 2 * src_bytes[kind] + np.dtype(st_np).itemsize
    return {"median_ms": round(med * 1e3, 4), "min_ms": round(min(reps) * 1e3, 4), "max_ms": round(max(reps) * 1e3, 4),
            "compulsory_bytes_per_px": bytes_px, "GBps": round(bytes_px * npix * nfr / med / 1e9, 1)}, dst.cpu().numpy()


rec = {"size": a.size, "frames": nfr, "sets_of": 2, "reps": a.reps, "precision": a.precision, "pitch": a.pitch, "normalize": {}}
ok = True
for kind in ("U8", "U16", "RGB8"):
    ref_dev = torch.from_numpy(values[kind].astype(st_np)).cuda()
    r_ref, want = timed("STORAGE", ref_dev, 1)                                               # the yardstick beside every kind
    del ref_dev
    more = {}
    if a.pitch:                                                                              # the same frames, rows a pitch apart
        for name, k, frames in (("storage_pitched", "STORAGE", values[kind].astype(st_np)), ("vec_pitched", kind, sources[kind])):
            p = pitch_of(k)
            dev = pitched(frames, p)
            r, got = timed(k, dev, 1, pitch=p)
            del dev
            r["pitch"], r["equal_to_dense"] = p, bool(np.array_equal(got, want))
            ok = ok and r["equal_to_dense"]
            more[name] = r
    dev = torch.from_numpy(sources[kind]).cuda()
    r_vec, got_vec = timed(kind, dev, 1)
    r_one, got_one = timed(kind, dev, 0)
    r_lut, got_lut = timed(kind, dev, 1, 0) if kind != "U16" else (None, want)                # 65536 values: never a table
    del dev
    r_vec["equal_to_storage"] = bool(np.array_equal(got_vec, want))
    r_one["equal_to_storage"] = bool(np.array_equal(got_one, want))
    r_vec["not_slower_than_storage"] = bool(r_vec["median_ms"] <= r_ref["median_ms"])
    rec["normalize"][kind] = {"storage": r_ref, "vec": r_vec, "one_per_thread": r_one, **more}
    if more:
        more["storage_pitched"]["ratio_to_dense"] = round(more["storage_pitched"]["median_ms"] / r_ref["median_ms"], 3)
        more["vec_pitched"]["ratio_to_dense"] = round(more["vec_pitched"]["median_ms"] / r_vec["median_ms"], 3)
    if r_lut:
        r_lut["equal_to_storage"] = bool(np.array_equal(got_lut, want))
        rec["normalize"][kind]["vec_no_lut"] = r_lut
    ok = ok and r_vec["equal_to_storage"] and r_one["equal_to_storage"] and r_vec["not_slower_than_storage"] and np.array_equal(got_lut, want)

if a.solve_pairs > 0:
    G = a.solve_pairs
    fr = u8[:G + 1]
    flo = torch.zeros((G, ny, nx, 2), dtype=torch.float32, device="cuda")
    f_ptr = [flo[k].data_ptr() for k in range(G)]
    solve = {}
    pay = {}
    cases = [("STORAGE", "STORAGE", torch.from_numpy(fr.astype(st_np)).cuda(), 0), ("U8", "U8", torch.from_numpy(fr).cuda(), 0)]
    if a.pitch:
        cases.append(("U8_pitched", "U8", pitched(fr, pitch_of("U8")), pitch_of("U8")))
    for name, kind, dev, pitch in cases:
        ctx.set_option("input", getattr(ofx, "IN_" + kind))
        if pitch:
            ctx.set_option("input_pitch", pitch)
        ptr = [dev[k].data_ptr() for k in range(G + 1)]
        run = lambda: ctx.tvl1_group_dev(ptr[:G], ptr[1:], f_ptr, nx, ny)
        run()
        ctx.synchronize()
        reps = []
        for _ in range(3):
            t = time.perf_counter()
            st = run()
            ctx.synchronize()
            reps.append(time.perf_counter() - t)
        ctx.set_option("input", ofx.IN_STORAGE)
        if pitch:
            ctx.set_option("input_pitch", 0)
        solve[name] = {"median_s": round(sorted(reps)[1], 4), "repetitions_s": [round(r, 4) for r in reps],
                       "iterations": int(sum(int(s.iterations().sum()) for s in st))}
        pay[name] = flo.cpu().numpy()
    solve["payloads_equal"] = bool(all(np.array_equal(p.view(np.uint32), pay["STORAGE"].view(np.uint32)) for p in pay.values()))
    ok = ok and solve["payloads_equal"]
    rec["tvl1_group_dev"] = {"pairs": G, **solve}

line = json.dumps(rec)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
if a.check and not ok:
    sys.exit(1)
