#!/usr/bin/env python3
"""Launch time of the iteration kernels AS THE JOB LAUNCHES THEM: fixed-work solves (1 scale, 1 warp = 300 iterations, HIP events
around the loop) of a lockstep group of G pairs in the f64 tolerance mode, for three (fuse4=0) and four (fuse4=1) iterations per
launch.   usage: group_launch_us.py [1920x1080:5 960x540:5 ...] [--f32] [--reps N] [name=value ...]
With OFX_LIB_PATH pointing at a ceiling build (tools/ceilings.sh) the same numbers are the kernels' memory / ALU ceilings."""
import importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ofx = importlib.import_module("optical-flow-1_amd")
synth = importlib.import_module("optical-flow-1_amd.synth")
prec, tdt = (ofx.F32, torch.float32) if "--f32" in sys.argv else (ofx.F64, torch.float64)
shapes, extra, reps = [], [], 3
args = iter(sys.argv[1:])
for a in args:
    if a == "--reps":
        reps = int(next(args))
    elif a[0].isdigit():
        size, g = a.split(":")
        shapes.append(tuple(map(int, size.split("x"))) + (int(g),))
    elif "=" in a:
        extra.append(a.split("=", 1))
shapes = shapes or [(1920, 1080, 5), (960, 540, 5), (480, 270, 5), (3840, 2160, 4)]
dev = torch.device("cuda:0")
torch.cuda.init()
ctx = ofx.Ofx(0, prec)
ctx.set_option("concurrency", 1)
ctx.set_option("relaxed_dual", 1)
ctx.set_option("profile", 1)
ctx.set_option("fixed_work", 1)
for k, v in extra:
    ctx.set_option(k, float(v))
for nx, ny, G in shapes:
    I0, I1, out = [], [], []
    for k in range(G):
        a, b = synth.pair_device("P1", nx, ny, k, dev, tdt)
        I0.append(a); I1.append(b); out.append(torch.empty((ny, nx, 2), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    line = "%4dx%-4d x %d" % (nx, ny, G)
    for fuse4 in (0, 1):
        ctx.set_option("fuse3", 1)
        ctx.set_option("fuse4", fuse4)
        best, F = 1e30, 0
        for rep in range(reps + 1):                          # the first solve allocates the level arrays
            st = ctx.tvl1_group_dev([t.data_ptr() for t in I0], [t.data_ptr() for t in I1], [t.data_ptr() for t in out], nx, ny,
                                    nscales=1, warps=1)
            ctx.synchronize()
            F = int(st[0].fused[0])
            if rep:
                best = min(best, st[0].iter_ms[0] * 1e3 / st[0].iter_launches[0])
        line += " | k_tvl1_iter%d %8.2f us/launch %7.2f us/iteration" % (F, best * F, best)
    print(line, flush=True)
    del I0, I1, out
