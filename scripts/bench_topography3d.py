#!/usr/bin/env python3
"""Side benchmark of compute_rock_fraction! on 3D grids (jrx_compute_rock_fraction3d) at 256^3 and 512 x 512 x 256 cells by default.  The entry point is called
directly; a call is synchronous at the ABI, so the time of a call is its wall time: one launch, the kernel and one stream synchronisation (median over the
timed calls after warm-up).  The inputs are (nx + 1)(ny + 1) doubles, so the writes of the eight members are the whole traffic.  Each size is compared with the
time of writing those bytes at the 8 TB/s line.  The surface is A cos(2 π x / Lx) cos(2 π y / Ly) of amplitude nz / 8 about mid-height, so that rows the
surface crosses and full / empty rows all occur.  --rows lists the depths of a thread's march along k to compare (tuning key "rock_fraction3d_rows": 0 = the
built-in depth, 1 = a thread per node), alternating call by call in one process.  Prints one JSON line per size and depth and, with --out FILE, writes them to
that file too (none by default: profiles/topography3d_bench.txt is a record assembled from several runs of this script and of the example).
    python scripts/bench_topography3d.py [--sizes 256x256x256,512x512x256] [--rows 0] [--calls 20] [--warmup 3] [--out FILE]"""
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
MEMBERS = ("center", "vertex", "Vx", "Vy", "Vz", "yz", "xz", "xy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256x256x256,512x512x256")
    ap.add_argument("--rows", default="0")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    depths = [int(v) for v in a.rows.split(",")]
    lines = []
    for s in a.sizes.split(","):
        nx, ny, nz = (int(v) for v in s.split("x"))
        ϕ = jr.RockRatio(jr.AMDGPUBackend, (nx, ny, nz))
        topo = jr.Topography(jr.AMDGPUBackend, (nx, ny))
        x, y = np.meshgrid(np.arange(nx + 1) / nx, np.arange(ny + 1) / ny, indexing="ij")
        topo.fill_((0.5 * nz + 0.125 * nz * np.cos(2.0 * np.pi * x) * np.cos(2.0 * np.pi * y)) / nz)          # the unit box: z0 = 0, _dz = nz
        args = [C.c_void_p(getattr(ϕ, k).data_ptr()) for k in MEMBERS] + [C.c_void_p(topo.h.data_ptr()), C.c_int64(nx), C.c_int64(ny), C.c_int64(nz),
                                                                           C.c_double(0.0), C.c_double(float(nz))]
        times = {d: [] for d in depths}
        torch.cuda.synchronize()
        for k in range(a.warmup + a.calls):
            for d in depths:
                h.set_option("rock_fraction3d_rows", d)
                t0 = time.perf_counter()
                h.call("jrx_compute_rock_fraction3d", *args)
                t1 = time.perf_counter()
                if k >= a.warmup:
                    times[d].append((t1 - t0) * 1e6)
        h.set_option("rock_fraction3d_rows", 0)
        nbytes = 8 * sum(getattr(ϕ, k).numel() for k in MEMBERS)
        rock = float(ϕ.center.sum()) / (nx * ny * nz)
        for d in depths:
            us, line_us = statistics.median(times[d]), nbytes / HBM_PEAK * 1e6
            res = dict(bench="compute_rock_fraction3d", ni=f"{nx}x{ny}x{nz}", rows=d, calls=a.calls, gpu=torch.cuda.get_device_name(dev), us=round(us, 1),
                       min_us=round(min(times[d]), 1), max_us=round(max(times[d]), 1), bytes_written=nbytes, us_at_8TBps=round(line_us, 1),
                       GBps_written=round(nbytes / (us * 1e-6) / 1e9, 1), share_of_8TBps=round(line_us / us, 3), rock_volume=round(rock, 6))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
        del ϕ, topo
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
