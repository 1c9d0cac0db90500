#!/usr/bin/env python3
"""Side benchmark of WENO_advection! (jrx_weno5_advection2d): the fused three-launch form against the reference's six-launch form, both methods, at
257 x 33 (test_WENO5.jl), 1025 x 257, 4097^2 and 8193^2 vertices.  The four variants alternate call by call in one process; a call is synchronous at the
ABI, so the time of a call is its wall time (median over the timed calls after warm-up; the device-only times come from a rocprofv3 --kernel-trace --stats
run of this script).  Bytes needed per vertex and call: fused 14 array passes (stage 1: u, vx, vy, u1; stages 2, 3: stencil field, u, vx, vy, output) = 112 B;
the six-launch form reads and writes the four flux arrays as well (41 passes = 328 B).  Prints one JSON line per size.
    python scripts/bench_weno2d.py [--sizes 257x33,1025x257,4097x4097,8193x8193] [--calls 20] [--warmup 3]"""
import argparse
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

B_FUSED, B_SPLIT = 112, 328


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="257x33,1025x257,4097x4097,8193x8193")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    for s in a.sizes.split(","):
        nx, ny = (int(v) for v in s.split("x"))
        x = torch.linspace(0, 1, nx, dtype=torch.float64, device=dev)[:, None]
        y = torch.linspace(0, 1, ny, dtype=torch.float64, device=dev)[None, :]
        u0 = jr.fzeros((nx, ny), dev)
        u0.copy_(1.0 + 0.5 * torch.sin(6.0 * x) * torch.cos(5.0 * y) + (x + 0.3 * y > 0.55).double())
        vx, vy = jr.fzeros((nx, ny), dev), jr.fzeros((nx, ny), dev)
        vx.copy_(torch.cos(4.0 * y).expand(nx, ny))
        vy.copy_(-torch.sin(3.0 * x).expand(nx, ny))
        dx, dy = 1.0 / (nx - 1), 1.0 / (ny - 1)
        dt = 0.4 * min(dx, dy)
        w = jr.WENO5(jr.AMDGPUBackend, 1, (nx, ny))
        u = jr.fzeros((nx, ny), dev)
        variants = [(f, m) for m in (1, 2) for f in (1, 0)]
        times = {v: [] for v in variants}
        for k in range(a.warmup + a.calls):
            for f, m in variants:
                u.copy_(u0)
                w.method = m
                h.set_option("weno_fused", f)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jr.WENO_advection_(u, (vx, vy), w, (dx, dy), dt, handle=h)
                t1 = time.perf_counter()
                if k >= a.warmup:
                    times[(f, m)].append((t1 - t0) * 1e6)
        h.set_option("weno_fused", 1)
        res = dict(bench="weno2d", nx=nx, ny=ny, calls=a.calls, gpu=torch.cuda.get_device_name(dev))
        for (f, m), ts in times.items():
            us = statistics.median(ts)
            key = f"{'fused' if f else 'split'}_{'js' if m == 1 else 'z'}"
            res[key + "_us"] = round(us, 1)
            res[key + "_min_us"] = round(min(ts), 1)
            res[key + "_GBps_needed"] = round((B_FUSED if f else B_SPLIT) * nx * ny / (us * 1e-6) / 1e9, 1)
        res["speedup_js"] = round(res["split_js_us"] / res["fused_js_us"], 2)
        res["speedup_z"] = round(res["split_z_us"] / res["fused_z_us"], 2)
        res["hbm_floor_us_at_6.29TBps"] = round(B_FUSED * nx * ny / 6.29e12 * 1e6, 1)
        print(json.dumps(res), flush=True)
        del u0, u, vx, vy, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
