#!/usr/bin/env python3
"""Side benchmark of compute_rock_fraction! (jrx_compute_rock_fraction2d) at 4096^2 and 8192^2 cells by default.  The entry point is called directly; a call is
synchronous at the ABI, so the time of a call is its wall time: one launch, the kernel and one stream synchronisation (median over the timed calls after
warm-up).  The inputs are nx + 1 doubles, so the writes of the four members are the whole traffic: nx ny + (nx + 1)(ny + 1) + (nx + 1) ny + nx (ny + 1)
doubles.  Each size is compared with the time of writing those bytes at the 8 TB/s line.  The surface is a sine of amplitude ny / 8 about mid-height, so that
the sloped branch, both clipped branches and full / empty volumes all occur.  Prints one JSON line per size and, with --out, writes them to a file (default
profiles/topography_bench.txt).
    python scripts/bench_topography.py [--sizes 4096x4096,8192x8192] [--calls 20] [--warmup 3] [--out FILE]"""
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
    ap.add_argument("--sizes", default="4096x4096,8192x8192")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "topography_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    lines = []
    for s in a.sizes.split(","):
        nx, ny = (int(v) for v in s.split("x"))
        ϕ = jr.RockRatio(jr.AMDGPUBackend, (nx, ny))
        topo = jr.Topography(jr.AMDGPUBackend, nx)
        topo.fill_((0.5 * ny + 0.125 * ny * np.sin(2.0 * np.pi * np.arange(nx + 1) / nx)) / ny)          # the unit box: y0 = 0, _dy = ny
        args = [C.c_void_p(getattr(ϕ, k).data_ptr()) for k in ("center", "vertex", "Vx", "Vy")] + [C.c_void_p(topo.h.data_ptr()), C.c_int64(nx), C.c_int64(ny),
                                                                                              C.c_double(0.0), C.c_double(float(ny))]
        times = []
        torch.cuda.synchronize()
        for k in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            h.call("jrx_compute_rock_fraction2d", *args)
            t1 = time.perf_counter()
            if k >= a.warmup:
                times.append((t1 - t0) * 1e6)
        nbytes = 8 * (nx * ny + (nx + 1) * (ny + 1) + (nx + 1) * ny + nx * (ny + 1))
        us, line_us = statistics.median(times), nbytes / HBM_PEAK * 1e6
        rock = float(ϕ.center.sum()) / (nx * ny)
        res = dict(bench="compute_rock_fraction", ni=f"{nx}x{ny}", calls=a.calls, gpu=torch.cuda.get_device_name(dev), us=round(us, 1), min_us=round(min(times), 1),
                   max_us=round(max(times), 1), bytes_written=nbytes, us_at_8TBps=round(line_us, 1), GBps_written=round(nbytes / (us * 1e-6) / 1e9, 1),
                   share_of_8TBps=round(line_us / us, 3), rock_area=round(rock, 6))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del ϕ, topo
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
