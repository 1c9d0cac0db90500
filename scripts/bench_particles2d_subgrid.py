#!/usr/bin/env python3
"""Side benchmark of the temperature update on 2D particles -- subgrid_diffusion_centroid!(pT, T_buffer, thermal.ΔT, subgrid_arrays, particles, dt) and
subgrid_diffusion! with loc = :vertex; jrx_particles2d_subgrid_diffusion_centroid / _vertex of csrc/particles.hip -- in ONE process, three routes alternating call
by call:
  composition   what a user of the library WITHOUT these operators has to write: centroid2particle_ / particle2centroid_ (vertex form: grid2particle_ /
                particle2grid_) for steps 2, 4 and 6 of the definition in include/jrx.h and torch elementwise operations for steps 1, 3, 5 and 7.  This leg uses
                nothing this script's commit added: on a checkout without the operators the script times it alone.
  chain         the library's chain of seven launches ("particles_subgrid_fused" = 0)
  fused         two (centre) / three (vertex) launches ("particles_subgrid_fused" = 1)
1024^2 cells, 12 particles per cell (jittered seeding), max_xcell = 24; the cloud is used after one advection! + move_particles! under a rigid rotation, as in a
time loop.  dt₀ is log-uniform over six decades around dt, d = 1.  A route is synchronous (it ends in a device synchronise), so the host clock around it is the
call: launches, kernels and wait.  The MEDIAN of the calls is reported.

Beside every time: the bytes the route MUST move, counted from the shapes -- every array a launch needs read once, every array it writes written once; the mask
of every slot, coordinates and fields of the active slots only, every slot of a particle field that is written in full; a torch operation reads and writes whole
arrays -- and the time those bytes take at the 8 TB/s line of one MI355X.  The share is must-move time over measured time; it is not a kernel-only figure.
Writes one JSON line per measurement to --out (default profiles/particles2d_subgrid_bench.txt) and prints it.
    python scripts/bench_particles2d_subgrid.py [--n 1024] [--calls 20] [--out FILE]"""
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
from justrelax_jl_amd.arrays import from_numpy, fzeros

LINE = 8.0e12                   # B/s, the HBM3E line rate of one MI355X
FLOOR = 1e-9
HAVE = hasattr(jr, "subgrid_diffusion_centroid_")


def call_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1.0e6


def composition(loc, pT, T, dT, pT0, pdT, dt0, sub, tmp, p, ndt, h):
    """the seven steps from the operators that existed before, in place where torch allows it; tmp is one particle-shaped scratch array, ndt the 0-dim
    tensor (-d) dt"""
    to_particle, to_grid = (jr.centroid2particle_, jr.particle2centroid_) if loc == "center" else (jr.grid2particle_, jr.particle2grid_)
    pT0.copy_(pT)                                        # 1
    to_particle(pT, T, p, handle=h)                      # 2
    torch.clamp(dt0, min=FLOOR, out=tmp)                 # 3: m (no NaN in this script's dt₀); an inactive slot has pT = pT0 = 0, so its δ is 0 without a mask
    torch.div(ndt, tmp, out=tmp)
    torch.exp(tmp, out=tmp)
    tmp.neg_().add_(1.0)                                 #    f = 1 - exp(x)
    torch.sub(pT, pT0, out=pdT)
    pdT.mul_(tmp)                                        #    δ
    pT0.add_(pdT)
    sub.zero_()                                          # 4
    to_grid(sub, pdT, p, handle=h)
    torch.sub(dT, sub, out=sub)                          # 5
    to_particle(pdT, sub, p, handle=h)                   # 6
    torch.add(pT0, pdT, out=pT)                          # 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--max-xcell", type=int, default=24)
    ap.add_argument("--nxcell", type=int, default=12)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "particles2d_subgrid_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_particles2d_subgrid.py needs a GPU: nothing is timed on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    gpu = torch.cuda.get_device_name(dev)
    n, mx = a.n, a.max_xcell
    ni = (n, n)
    grid = jr.Geometry(ni, (1.0, 1.0))
    dx = 1.0 / n
    p = jr.init_particles(jr.AMDGPUBackend, a.nxcell, mx, a.nxcell // 2, grid, ni, rng=np.random.default_rng(20261021))
    (pT,) = jr.init_cell_arrays(p, 1)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    # a rigid rotation about the centre, Courant number 0.5 at the corners with dt = 1; one advect + move so that buckets are unevenly filled
    w = 0.5 * dx / np.hypot(0.5, 0.5)
    xg = (np.arange(n + 2) - 0.5) * dx
    st.V.Vx.copy_(from_numpy(np.asfortranarray(np.broadcast_to(-w * (xg[None, :] - 0.5), (n + 1, n + 2))), dev))
    st.V.Vy.copy_(from_numpy(np.asfortranarray(np.broadcast_to(w * (xg[:, None] - 0.5), (n + 2, n + 1))), dev))
    jr.advection_(p, jr.RungeKutta2(), st.V, 1.0, handle=h)
    jr.move_particles_(p, (pT,), handle=h)
    del st
    gen = torch.Generator(device=dev).manual_seed(7)
    rand = lambda like, lo, hi: torch.rand(like.shape, generator=gen, device=dev, dtype=torch.float64) * (hi - lo) + lo
    act = p.index != 0
    dt, d = 2.0e3, 1.0
    ndt = torch.tensor((-d) * dt, dtype=torch.float64, device=dev)
    pT_start = fzeros(p.shape, dev)
    pT_start.copy_(torch.where(act, rand(pT_start, 300.0, 1600.0), 0.0))
    pT0, pdT, dt0, tmp = (fzeros(p.shape, dev) for _ in range(4))          # the composition's own scratch: the shapes of SubgridDiffusionCellArrays
    dt0.copy_(torch.where(act, dt * 10.0 ** rand(dt0, -3.0, 3.0), 0.0))
    S, A, nc, nv = n * n * mx, int(act.sum()), n * n, (n + 1) * (n + 1)
    head = 4 * S + 16 * A                                   # the mask of every slot, the coordinates of the active ones
    lines = []
    for loc in ("center", "vertex"):
        nn = nc if loc == "center" else nv
        T, dT, sub = (fzeros(ni if loc == "center" else (n + 1, n + 1), dev) for _ in range(3))
        T.copy_(rand(T, 300.0, 1600.0)), dT.copy_(rand(dT, -50.0, 50.0))
        interp = head + 8 * nn + 8 * S                      # operator 6 / 3: a grid field read, a particle field written in full
        gather = head + 8 * A + 8 * nn                      # operator 7 / 4: a particle field read, a grid field written
        need = {"composition": 16 * S + interp + 8 * (2 + 2 + 2 + 2 + 2 + 3 + 3 + 3) * S + 8 * nn + gather + 24 * nn + interp + 24 * S,
                "chain": 16 * S + interp + (4 * S + 24 * A + 8 * A + 8 * S) + 8 * nn + gather + 24 * nn + interp + (4 * S + 16 * A + 8 * S),
                "fused": (head + 8 * S + 8 * A + 8 * S + 8 * nn + (16 * nn if loc == "center" else 8 * S)) + (0 if loc == "center" else head + 8 * A + 16 * nn)
                         + (head + 8 * A + 8 * nn + 16 * S)}
        launches = {"chain": 7, "fused": 2 if loc == "center" else 3}
        routes = {"composition": lambda: composition(loc, pT, T, dT, pT0, pdT, dt0, sub, tmp, p, ndt, h)}
        if HAVE:
            sa = jr.SubgridDiffusionCellArrays(p, loc=loc)
            sa.dt0.copy_(dt0)
            op = jr.subgrid_diffusion_centroid_ if loc == "center" else jr.subgrid_diffusion_

            def library(fused, sa=sa, op=op, T=T, dT=dT):
                h.set_option("particles_subgrid_fused", fused)
                op(pT, T, dT, sa, p, dt, d=d, handle=h)
            routes["chain"], routes["fused"] = (lambda: library(0)), (lambda: library(1))
        us, outs = {k: [] for k in routes}, {}
        for k, fn in routes.items():                           # warm-up of every route from the same start, and its outputs for the comparison
            pT.copy_(pT_start)
            n0 = h.get_option("stat_particles_launches")
            fn()
            assert k == "composition" or h.get_option("stat_particles_launches") - n0 == launches[k]
            outs[k] = [t.clone() for t in ((pT, pT0, pdT, sub) if k == "composition" else (pT, sa.pT0, sa.pΔT, sa.ΔT_subgrid))]
        for _ in range(a.calls):
            for k, fn in routes.items():
                pT.copy_(pT_start)                             # every call does the same work: outside the clock
                us[k].append(call_us(fn))
        med = {k: statistics.median(v) for k, v in us.items()}
        scale = float(pT_start.abs().max())
        for k in routes:
            t_line = need[k] / LINE * 1.0e6
            rec = dict(bench="particles2d_subgrid", loc=loc, route=k, launches=launches.get(k), ni=f"{n}x{n}", max_xcell=mx, nxcell=a.nxcell, active=A, d=d, calls=a.calls,
                       gpu=gpu, us_per_call_median=round(med[k], 1), us_min=round(min(us[k]), 1), us_max=round(max(us[k]), 1), must_move_MB=round(need[k] / 1e6, 1),
                       us_at_8TBps=round(t_line, 1), share_of_8TBps=round(t_line / med[k], 3))
            if k == "fused":
                rec["same_bits_as_chain"] = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(outs["fused"], outs["chain"]))
                rec["max_diff_to_composition_over_max_T"] = max(float((x - y).abs().max()) for x, y in zip(outs["fused"], outs["composition"])) / scale
            lines.append(json.dumps(rec, ensure_ascii=False))
            print(lines[-1], flush=True)
        if HAVE:
            lines.append(json.dumps(dict(bench="particles2d_subgrid", loc=loc, composition_over_fused=round(med["composition"] / med["fused"], 3),
                                         composition_over_chain=round(med["composition"] / med["chain"], 3), chain_over_fused=round(med["chain"] / med["fused"], 3),
                                         must_move_composition_over_fused=round(need["composition"] / need["fused"], 3),
                                         must_move_chain_over_fused=round(need["chain"] / need["fused"], 3))))
            print(lines[-1], flush=True)
        del T, dT, sub
    if HAVE:
        h.set_option("particles_subgrid_fused", 1)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(f"# python scripts/bench_particles2d_subgrid.py --n {n} --calls {a.calls} on one MI355X, one process, the routes alternating: host clock around each\n"
                   f"# synchronous call, median of {a.calls} warm calls; must_move_MB = the bytes the route has to move, from the shapes; us_at_8TBps = their time at the\n"
                   "# 8 TB/s line; share = that over the measured call.  Kernel-only times and counters: not measured.\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
