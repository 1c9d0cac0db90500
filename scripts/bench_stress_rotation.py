#!/usr/bin/env python3
"""Side benchmark of rotate_stress! on grids (jrx_rotate_stress2d / 3d): the four method x advection forms at 4096^2 and 256^3 cells by default, alternating
call by call in one process.  The entry points are called directly; a call is synchronous at the ABI, so the time of a call is its wall time: one launch, the
kernel and one stream synchronisation (median over the timed calls after warm-up).  Bytes counted per cell and call: every array once -- 2D 7 reads (xx, yy,
xy_c, xy, ω, Vx, Vy) + 4 writes = 11 passes = 88 B, 3D 15 reads + 9 writes = 24 passes = 192 B (the same count for "none", which does not read the velocities:
its share of the line is therefore an under-statement by 2 / 11 and 3 / 24).  Prints one JSON line per size and form and, with --out, writes the table.
    python scripts/bench_stress_rotation.py [--sizes 4096x4096,256x256x256] [--calls 20] [--warmup 3] [--out FILE]"""
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
FORMS = [("matrix", "upwind"), ("matrix", "none"), ("jaumann", "upwind"), ("jaumann", "none")]
METHODS, ADVECTIONS = dict(matrix=0, jaumann=1), dict(none=0, upwind=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x4096,256x256x256")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    lines = []
    for s in a.sizes.split(","):
        ni = tuple(int(v) for v in s.split("x"))
        nd = len(ni)
        st = jr.StokesArrays(jr.AMDGPUBackend, ni)
        gen = torch.Generator(device=dev).manual_seed(nd)
        fill = lambda t, scale: t.copy_((torch.rand(tuple(t.shape), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0) * scale)
        names = ("xx", "yy", "xy_c", "xy") if nd == 2 else ("xx", "yy", "zz", "yz_c", "xz_c", "xy_c", "yz", "xz", "xy")
        for k in names:
            fill(getattr(st.τ, k), 1.0e7)
        vel = [getattr(st.V, k) for k in ("Vx", "Vy", "Vz")[:nd]]
        for v in vel:
            fill(v, 1.0)
        om = [st.ω.xy] if nd == 2 else [st.ω.yz, st.ω.xz, st.ω.xy]
        for w in om:
            fill(w, 1.0)
        _di = tuple(float(m) for m in ni)                         # the unit box
        dt = 0.5 / max(ni)                                        # |θ| <= 0.5 sqrt(3) / n, CFL <= 0.5 per axis
        vec = lambda ps: (C.c_void_p * len(ps))(*ps)
        tin = vec([getattr(st.τ, k).data_ptr() for k in names] + ([None, None] if nd == 2 else []))
        tout = vec([getattr(st.τ_o, k).data_ptr() for k in names] + ([None, None] if nd == 2 else []))
        wv = C.c_void_p(om[0].data_ptr()) if nd == 2 else vec([w.data_ptr() for w in om])
        head = [tout, tin, wv, vec([v.data_ptr() for v in vel])] + [C.c_int64(m) for m in ni] + [(C.c_double * nd)(*_di), C.c_double(dt)]
        times = {f: [] for f in FORMS}
        torch.cuda.synchronize()
        for k in range(a.warmup + a.calls):
            for f in FORMS:
                t0 = time.perf_counter()
                h.call(f"jrx_rotate_stress{nd}d", *head, C.c_int32(METHODS[f[0]]), C.c_int32(ADVECTIONS[f[1]]))
                t1 = time.perf_counter()
                if k >= a.warmup:
                    times[f].append((t1 - t0) * 1e6)
        cells = int(np.prod(ni))
        bpc = 88 if nd == 2 else 192
        for f in FORMS:
            us = statistics.median(times[f])
            res = dict(bench="stress_rotation", ni="x".join(map(str, ni)), method=f[0], advection=f[1], calls=a.calls, gpu=torch.cuda.get_device_name(dev),
                       us=round(us, 1), min_us=round(min(times[f]), 1), max_us=round(max(times[f]), 1), bytes_per_cell=bpc,
                       GBps_counted=round(bpc * cells / (us * 1e-6) / 1e9, 1), share_of_8TBps=round(bpc * cells / (us * 1e-6) / HBM_PEAK, 3))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
        del st, vel, om
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
