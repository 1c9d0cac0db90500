#!/usr/bin/env python3
"""Side benchmark of the two calls that carry the elastic stress on 2D particles -- rotate_stress!(pτxx, pτyy, pτxy, pω, stokes, particles, dt) and
stress2grid!(stokes, pτxx, pτyy, pτxy, particles); jrx_particles2d_rotate_stress / jrx_particles2d_stress2grid of csrc/particles.hip -- each as ONE launch
("particles_stress_fused" = 1) and as its chain of single-operator launches (= 0: 5 and 6), in ONE process, the two forms alternating call by call.
1024^2 cells, 12 particles per cell (jittered seeding), max_xcell = 24; the cloud is used after one advection! + move_particles! under a rigid rotation, as in
a time loop.  A call is synchronous (it ends in the library's wait for its stream), so the host clock around it is the call: launches, kernels and wait.  The
MEDIAN of the calls is reported.

Beside every time: the bytes the form MUST move, counted from the shapes -- every array a launch needs read once, every array it writes written once; the
mask of every slot, coordinates and fields of the active slots only, every slot of a particle field that is written in full -- and the time those bytes take at
the 8 TB/s line of one MI355X.  The share is must-move time over measured time; it is not a kernel-only figure (the launches and the wait are inside the call).
  rotate_stress!, one launch   mask + coordinates read, τ.xx, τ.yy, τ.xy, ω.xy read, the four particle fields written
  rotate_stress!, chain        four interpolations (each: mask + coordinates + a grid field read, a particle field written), then the rotation (mask, four
                               particle fields read, three written where active)
  stress2grid!, one launch     mask + coordinates + three particle fields read, six grid fields written
  stress2grid!, chain          six launches (each: mask + coordinates + a particle field read, a grid field written)
Writes one JSON line per measurement to --out (default profiles/particles2d_stress_bench.txt) and prints it.
    python scripts/bench_particles2d_stress.py [--n 1024] [--calls 20] [--method matrix] [--out FILE]"""
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
from justrelax_jl_amd.arrays import from_numpy

LINE = 8.0e12                   # B/s, the HBM3E line rate of one MI355X


def call_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1.0e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--max-xcell", type=int, default=24)
    ap.add_argument("--nxcell", type=int, default=12)
    ap.add_argument("--method", default="matrix", choices=("matrix", "jaumann"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "particles2d_stress_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_particles2d_stress.py needs a GPU: nothing is timed on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    gpu = torch.cuda.get_device_name(dev)
    n, mx = a.n, a.max_xcell
    ni = (n, n)
    grid = jr.Geometry(ni, (1.0, 1.0))
    dx = 1.0 / n
    p = jr.init_particles(jr.AMDGPUBackend, a.nxcell, mx, a.nxcell // 2, grid, ni, rng=np.random.default_rng(20261021))
    pτxx, pτyy, pτxy, pω = jr.init_cell_arrays(p, 4)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    # a rigid rotation about the centre, Courant number 0.5 at the corners with dt = 1; one advect + move so that buckets are unevenly filled
    w = 0.5 * dx / np.hypot(0.5, 0.5)
    xg = (np.arange(n + 2) - 0.5) * dx
    st.V.Vx.copy_(from_numpy(np.asfortranarray(np.broadcast_to(-w * (xg[None, :] - 0.5), (n + 1, n + 2))), dev))
    st.V.Vy.copy_(from_numpy(np.asfortranarray(np.broadcast_to(w * (xg[:, None] - 0.5), (n + 2, n + 1))), dev))
    jr.advection_(p, jr.RungeKutta2(), st.V, 1.0, handle=h)
    jr.move_particles_(p, (pτxx, pτyy, pτxy, pω), handle=h)
    gen = torch.Generator(device=dev).manual_seed(7)
    for t in (st.τ.xx, st.τ.yy, st.τ.xy):
        t.copy_(torch.rand(t.shape, generator=gen, device=dev, dtype=torch.float64) * 2.0 - 1.0)
    jr.compute_vorticity_(st, grid)
    dt = 0.5 / max(float(st.ω.xy.abs().max()), 1e-300)          # |ω dt| <= 0.5
    slots, nact, ncell, nvert = n * n * mx, int((p.index != 0).sum()), n * n, (n + 1) * (n + 1)
    head = slots * 4 + nact * 16                              # the mask of every slot, the coordinates of the active ones
    need = {("rotate_stress", 1): head + 8 * (2 * ncell + 2 * nvert) + 4 * slots * 8,
            ("rotate_stress", 0): 2 * (head + 8 * ncell + slots * 8) + 2 * (head + 8 * nvert + slots * 8) + slots * 4 + nact * (32 + 24),
            ("stress2grid", 1): head + nact * 24 + 8 * 3 * (ncell + nvert),
            ("stress2grid", 0): 3 * (head + nact * 8 + 8 * ncell) + 3 * (head + nact * 8 + 8 * nvert)}
    launches = {("rotate_stress", 1): 1, ("rotate_stress", 0): 5, ("stress2grid", 1): 1, ("stress2grid", 0): 6}
    τ_o = st.τ_o
    for k in ("xx_v", "yy_v"):
        getattr(τ_o, k)                                        # allocated before anything is timed
    calls = {"rotate_stress": lambda: jr.rotate_stress_(pτxx, pτyy, pτxy, pω, st, p, dt, method=a.method, handle=h),
             "stress2grid": lambda: jr.stress2grid_(st, pτxx, pτyy, pτxy, p, handle=h)}
    lines, meds = [], {}
    for op, fn in calls.items():
        us, outs = {1: [], 0: []}, {}
        for f in (1, 0):                                       # warm-up of both forms, and their outputs for the comparison
            h.set_option("particles_stress_fused", f)
            n0 = h.get_option("stat_particles_launches")
            fn()
            assert h.get_option("stat_particles_launches") - n0 == launches[op, f]
            outs[f] = [t.clone() for t in ((pτxx, pτyy, pτxy, pω) if op == "rotate_stress" else (τ_o.xx, τ_o.yy, τ_o.xy_c, τ_o.xy, τ_o.xx_v, τ_o.yy_v))]
        same = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(outs[1], outs[0]))
        for _ in range(a.calls):
            for f in (1, 0):
                h.set_option("particles_stress_fused", f)
                us[f].append(call_us(fn))
        for f in (1, 0):
            t_line = need[op, f] / LINE * 1.0e6
            meds[op, f] = statistics.median(us[f])
            rec = dict(bench="particles2d_stress", op=op, form="one launch" if f else f"chain of {launches[op, f]}", method=a.method if op == "rotate_stress" else None,
                       ni=f"{n}x{n}", max_xcell=mx, nxcell=a.nxcell, active=nact, calls=a.calls, gpu=gpu, us_per_call_median=round(meds[op, f], 1),
                       us_min=round(min(us[f]), 1), us_max=round(max(us[f]), 1), must_move_MB=round(need[op, f] / 1e6, 1), us_at_8TBps=round(t_line, 1),
                       share_of_8TBps=round(t_line / meds[op, f], 3), same_bits_as_other_form=same)
            lines.append(json.dumps(rec, ensure_ascii=False))
            print(lines[-1], flush=True)
        lines.append(json.dumps(dict(bench="particles2d_stress", op=op, chain_over_one_launch=round(meds[op, 0] / meds[op, 1], 3),
                                     must_move_chain_over_one_launch=round(need[op, 0] / need[op, 1], 3))))
        print(lines[-1], flush=True)
    h.set_option("particles_stress_fused", 1)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(f"# python scripts/bench_particles2d_stress.py --n {n} --calls {a.calls} --method {a.method} on one MI355X, one process, the two forms alternating: host clock\n"
                   f"# around each synchronous call, median of {a.calls} warm calls; must_move_MB = the bytes the form has to move, from the shapes; us_at_8TBps = their time\n"
                   "# at the 8 TB/s line; share = that over the measured call.\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
