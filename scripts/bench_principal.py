#!/usr/bin/env python3
"""Side benchmark of compute_principal_stresses! (jrx_principal_stresses2d / 3d) at 8192^2 cells (2D) and 256^3, 512^3 cells (3D).  Inputs are random
Pa-scale stress tensors (1e7 ± 1e7 on the diagonal, ±5e6 off it: Jacobi's sweep count is that of a general tensor).  A call is synchronous at the ABI, so
the time of a call is its wall time (median over the timed calls after warm-up; device-only times come from a rocprofv3 --kernel-trace --stats run of this
script).  Bytes needed per cell and call: 2D 3 reads + 4 writes = 56 B, 3D 6 reads + 9 writes = 120 B.  Prints one JSON line per size.
    python scripts/bench_principal.py [--sizes 8192x8192,256x256x256,512x512x512] [--calls 20] [--warmup 3]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd import _lib

HBM = 6.29e12                   # B/s, the measured copy rate of one MI355X (the roofline bench.py prices against)
BYTES = {2: 56, 3: 120}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192x8192,256x256x256,512x512x512")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    g = torch.Generator(device=dev)
    g.manual_seed(20261016)
    for s in a.sizes.split(","):
        ni = tuple(int(v) for v in s.split("x"))
        nd = len(ni)
        names = ("xx", "yy", "xy_c") if nd == 2 else ("xx", "yy", "zz", "yz_c", "xz_c", "xy_c")
        τ = SimpleNamespace()
        for k in names:
            t = jr.fzeros(ni, dev)
            diag = k in ("xx", "yy", "zz")
            t.copy_((torch.rand(ni, generator=g, device=dev, dtype=torch.float64) * 2 - 1) * (1.0e7 if diag else 5.0e6) + (1.0e7 if diag else 0.0))
            setattr(τ, k, t)
        stokes = SimpleNamespace(P=τ.xx, τ=τ)
        σ = jr.PrincipalStress(jr.AMDGPUBackend, ni)
        calls0 = h.get_option("stat_principal_calls")
        ts = []
        for k in range(a.warmup + a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            jr.compute_principal_stresses_(stokes, σ, handle=h)
            t1 = time.perf_counter()
            if k >= a.warmup:
                ts.append((t1 - t0) * 1e6)
        assert h.get_option("stat_principal_calls") - calls0 == a.warmup + a.calls
        finite = all(bool(torch.isfinite(getattr(σ, f)).all()) for f in (("σ1", "σ2") if nd == 2 else ("σ1", "σ2", "σ3")))
        ncell = 1
        for n in ni:
            ncell *= n
        us = statistics.median(ts)
        need = BYTES[nd] * ncell
        res = dict(bench="principal", ni="x".join(map(str, ni)), calls=a.calls, gpu=torch.cuda.get_device_name(dev), median_us=round(us, 1),
                   min_us=round(min(ts), 1), bytes_per_cell=BYTES[nd], GBps_needed=round(need / (us * 1e-6) / 1e9, 1),
                   frac_of_6_29TBps=round(need / (us * 1e-6) / HBM, 3), hbm_floor_us=round(need / HBM * 1e6, 1), outputs_finite=finite)
        print(json.dumps(res), flush=True)
        del τ, stokes, σ
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
