#!/usr/bin/env python3
"""Side benchmark of update_phase_ratios_2D! / 3D! (jrx_update_phase_ratios2d / 3d): the one-launch form against the launch-per-member form (tuning key
"phase_ratios_fused" = 1 / 0), N = 2 and N = 4 phase arrays, at 2048^2 and 256^3 cells by default.  The two forms alternate call by call in one process.  The
entry points are called directly with the coordinate vectors already on the device (the host layer uploads them on every call, which would be most of a 2D
call's time); a call is synchronous at the ABI, so the time of a call is its wall time: the launches, the kernels and one stream synchronisation (median over
the timed calls after warm-up).  Bytes needed per cell and call: the one-launch form reads the N inputs once and writes every member once -- (1 + 4) N x 8 B in
2D, (1 + 8) N x 8 B in 3D; the launch-per-member form reads the inputs in every launch -- at least 8 N x 8 B in 2D and 16 N x 8 B in 3D.  Prints one JSON line
per size and phase count.
    python scripts/bench_phase_ratios.py [--sizes 2048x2048,256x256x256] [--phases 2,4] [--calls 20] [--warmup 3]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd import _lib

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x2048,256x256x256")
    ap.add_argument("--phases", default="2,4")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    for s in a.sizes.split(","):
        ni = tuple(int(v) for v in s.split("x"))
        nd = len(ni)
        grid = jr.Geometry.from_vertices(tuple(np.linspace(0.0, 1.0 + 0.5 * d, m + 1) for d, m in enumerate(ni)))
        xc, xv = [torch.tensor(x, device=dev) for x in grid.xci], [torch.tensor(x, device=dev) for x in grid.xvi]
        dx = (C.c_double * nd)(*(float(x[1] - x[0]) for x in grid.xvi))
        vec = lambda ts: (C.c_void_p * nd)(*(t.data_ptr() for t in ts))
        names = ("center", "vertex", "Vx", "Vy") if nd == 2 else ("center", "vertex", "Vx", "Vy", "Vz", "yz", "xz", "xy")
        for N in (int(v) for v in a.phases.split(",")):
            gen = torch.Generator(device=dev).manual_seed(N)
            ps = []
            for _ in range(N):
                p = jr.fzeros(ni, dev)
                p.copy_(torch.rand(ni, dtype=torch.float64, device=dev, generator=gen) * 0.95 + 0.05)
                ps.append(p)
            pr = jr.PhaseRatios(jr.AMDGPUBackend, N, ni)
            pa = (C.c_void_p * N)(*(p.data_ptr() for p in ps))
            args = [C.c_void_p(getattr(pr, k).data_ptr()) for k in names] + [pa, C.c_int32(N)] + [C.c_int64(m) for m in ni] + [vec(xc), vec(xv), dx]
            times = {1: [], 0: []}
            torch.cuda.synchronize()
            for k in range(a.warmup + a.calls):
                for f in (1, 0):
                    h.set_option("phase_ratios_fused", f)
                    t0 = time.perf_counter()
                    h.call(f"jrx_update_phase_ratios{nd}d", *args)
                    t1 = time.perf_counter()
                    if k >= a.warmup:
                        times[f].append((t1 - t0) * 1e6)
            h.set_option("phase_ratios_fused", 1)
            cells = int(np.prod(ni))
            b_fused, b_split = (1 + len(names)) * N * 8, 2 * len(names) * N * 8
            res = dict(bench="phase_ratios", ni="x".join(map(str, ni)), nphase=N, calls=a.calls, gpu=torch.cuda.get_device_name(dev))
            for f, key, b in ((1, "fused", b_fused), (0, "split", b_split)):
                us = statistics.median(times[f])
                res[key + "_us"] = round(us, 1)
                res[key + "_min_us"] = round(min(times[f]), 1)
                res[key + "_max_us"] = round(max(times[f]), 1)
                res[key + "_bytes_per_cell"] = b
                res[key + "_GBps_needed"] = round(b * cells / (us * 1e-6) / 1e9, 1)
            res["speedup"] = round(res["split_us"] / res["fused_us"], 2)
            res["byte_ratio"] = round(b_split / b_fused, 2)
            res["share_of_byte_ratio"] = round(res["speedup"] / res["byte_ratio"], 2)
            res["fused_share_of_8TBps"] = round(res["fused_GBps_needed"] * 1e9 / HBM_PEAK, 3)
            print(json.dumps(res), flush=True)
            del ps, pr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
