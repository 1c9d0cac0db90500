#!/usr/bin/env python3
"""Side benchmark of the 3D WENO_advection! (jrx_weno5_advection3d): the fused three-launch form against the six-launch form, both methods, at 512^3
vertices by default (u, three velocities, ut, six flux arrays and the saved initial field: 12 arrays, about 13 GB).  The four variants alternate call by
call in one process; a call is synchronous at the ABI, so the time of a call is its wall time (median over the timed calls after warm-up; the device-only
times come from a rocprofv3 --kernel-trace --stats run of this script).  Bytes needed per vertex and call: fused 17 array passes (stage 1: u, vx, vy, vz,
u1 = 5; stages 2, 3: stencil field, u, vx, vy, vz, output = 6 each) = 136 B; the six-launch form reads and writes the six flux arrays as well (three flux
launches of 7 passes, the steps 11 + 12 + 12: 56 passes = 448 B).  Prints one JSON line per size.
    python scripts/bench_weno3d.py [--sizes 512x512x512] [--calls 10] [--warmup 3]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd import _lib

B_FUSED, B_SPLIT = 136, 448


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512x512")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    for s in a.sizes.split(","):
        n = tuple(int(v) for v in s.split("x"))
        x, y, z = (torch.linspace(0, 1, m, dtype=torch.float64, device=dev).view([-1 if d == k else 1 for d in range(3)]) for k, m in enumerate(n))
        u0 = jr.fzeros(n, dev)
        u0.copy_(1.0 + 0.5 * torch.sin(6.0 * x) * torch.cos(5.0 * y) * torch.cos(4.0 * z) + (x + 0.3 * y + 0.2 * z > 0.6).double())
        vx, vy, vz = (jr.fzeros(n, dev) for _ in range(3))
        vx.copy_((torch.cos(4.0 * y) * torch.sin(2.0 * z)).expand(*n))
        vy.copy_((-torch.sin(3.0 * x) * torch.cos(3.0 * z)).expand(*n))
        vz.copy_((torch.sin(5.0 * x) * torch.cos(2.0 * y)).expand(*n))
        d = tuple(1.0 / (m - 1) for m in n)
        dt = 0.4 * min(d)
        w = jr.WENO5(jr.AMDGPUBackend, 1, n)
        u = jr.fzeros(n, dev)
        variants = [(f, m) for m in (1, 2) for f in (1, 0)]
        times = {v: [] for v in variants}
        for k in range(a.warmup + a.calls):
            for f, m in variants:
                u.copy_(u0)
                w.method = m
                h.set_option("weno_fused", f)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jr.WENO_advection_(u, (vx, vy, vz), w, d, dt, handle=h)
                t1 = time.perf_counter()
                if k >= a.warmup:
                    times[(f, m)].append((t1 - t0) * 1e6)
        h.set_option("weno_fused", 1)
        nv = n[0] * n[1] * n[2]
        res = dict(bench="weno3d", nx=n[0], ny=n[1], nz=n[2], calls=a.calls, gpu=torch.cuda.get_device_name(dev))
        for (f, m), ts in times.items():
            us = statistics.median(ts)
            key = f"{'fused' if f else 'split'}_{'js' if m == 1 else 'z'}"
            res[key + "_us"] = round(us, 1)
            res[key + "_min_us"] = round(min(ts), 1)
            res[key + "_max_us"] = round(max(ts), 1)
            res[key + "_GBps_needed"] = round((B_FUSED if f else B_SPLIT) * nv / (us * 1e-6) / 1e9, 1)
        res["speedup_js"] = round(res["split_js_us"] / res["fused_js_us"], 2)
        res["speedup_z"] = round(res["split_z_us"] / res["fused_z_us"], 2)
        res["hbm_floor_us_at_6.29TBps"] = round(B_FUSED * nv / 6.29e12 * 1e6, 1)
        print(json.dumps(res), flush=True)
        del u0, u, vx, vy, vz, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
