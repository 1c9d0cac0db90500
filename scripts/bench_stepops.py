#!/usr/bin/env python3
"""Side benchmark of the per-step operators of csrc/stepops.hip.  compute_melt_fraction! (phase-ratio form, two Caricchi phases) and
subgrid_characteristic_time! (two phases) at 4096^2 and 256^3 cells: one warm-up call, then device events around `calls` calls, in one process.  The entry
points are synchronous, so the time per call between the events holds the launch and the host's wait of each call besides the kernel.  Bytes per cell, from
the shapes (every input read once, the output written once): melt fraction 2 ratios + T + ϕ = 32 B (args.P is not read by the laws built), subgrid time
2 ratios + T + P + dt₀ = 40 B.  free_surface_bcs! touches the top planes only: its time per call is the launch and the wait alone.  pureshear_bc! writes the
interior of every velocity array once (8 B per cell and component) from the coordinate vectors.
Prints one JSON line per measurement.
    python scripts/bench_stepops.py [--sizes 4096x4096,256x256x256] [--calls 20]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd import _lib

LINE = 8.0e12                   # B/s, the HBM3E line rate of one MI355X
PHASES = [dict(eta=1.0, G=1.0, Kb=1.0, k=3.0, Cp=1.0e3, density=dict(kind="PT", rho0=3.0e3, alpha=3.0e-5, beta=1.0e-11, T0=273.0), melting=dict(kind="caricchi")),
          dict(eta=1.0, G=0.5, Kb=1.0, k=1.7, Cp=1.25e3, density=dict(kind="constant", rho0=2.7e3), melting=dict(kind="caricchi", a=900.0))]


def timed(fn, calls):
    """µs per call between two device events around `calls` calls, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1.0e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x4096,256x256x256")
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    g = torch.Generator(device=dev)
    g.manual_seed(20261020)
    rand = lambda shape, lo, hi: torch.rand(shape[::-1], generator=g, device=dev, dtype=torch.float64).permute(*range(len(shape) - 1, -1, -1)) * (hi - lo) + lo
    gpu = torch.cuda.get_device_name(dev)
    for s in a.sizes.split(","):
        ni = tuple(int(v) for v in s.split("x"))
        nd, ncell = len(ni), 1
        for n in ni:
            ncell *= n
        st, th, pr = jr.StokesArrays(jr.AMDGPUBackend, ni), jr.ThermalArrays(jr.AMDGPUBackend, ni), jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
        r = rand(ni, 0.0, 1.0)
        pr.center[0].copy_(r)
        pr.center[1].copy_(1.0 - r)
        th.T.copy_(rand(tuple(n + 2 for n in ni), 900.0, 1400.0))
        st.P.copy_(rand(ni, 1.0e5, 1.0e9))
        T = rand(ni, 900.0, 1400.0)
        out = jr.fzeros(ni, dev)
        di = (0.5, 0.25, 0.125)[:nd]
        n0 = h.get_option("stat_stepops_launches")
        for name, nbytes, fn in (("compute_melt_fraction", 32, lambda: jr.compute_melt_fraction_(out, pr, PHASES, dict(T=T, P=st.P), handle=h)),
                                 ("subgrid_characteristic_time", 40, lambda: jr.subgrid_characteristic_time_(out, pr, PHASES, th, st, di, handle=h))):
            us = timed(fn, a.calls)
            need = nbytes * ncell
            print(json.dumps(dict(bench="stepops", op=name, ni=s, nphase=2, calls=a.calls, gpu=gpu, us_per_call=round(us, 1), bytes_per_cell=nbytes,
                                  GBps_needed=round(need / (us * 1e-6) / 1e9, 1), share_of_8TBps=round(need / (us * 1e-6) / LINE, 3),
                                  outputs_finite=bool(torch.isfinite(out).all()))), flush=True)
        grid = jr.Geometry(ni, (1.0,) * nd)
        on = jr.VelocityBoundaryConditions(free_surface=True) if nd == 2 else jr.VelocityBoundaryConditions(free_slip={f: True for f in ("left", "right", "front", "back", "top", "bot")},
                                                                                                               free_surface=True)
        fs_di = ((0.5, 0.25), (0.5, 0.25)) if nd == 2 else ((0.5, 0.25, 0.125),)
        xv = tuple(torch.tensor(x, device=dev) for x in grid.xvi)
        us = timed(lambda: jr.pureshear_bc_(st, grid.xci, xv, 1.0, jr.AMDGPUBackend, handle=h), a.calls)
        need = 8 * nd * ncell                                    # the interior of every velocity array written once; the reads are the coordinate vectors
        print(json.dumps(dict(bench="stepops", op="pureshear_bc", ni=s, calls=a.calls, gpu=gpu, us_per_call=round(us, 1), bytes_per_cell=8 * nd,
                              GBps_needed=round(need / (us * 1e-6) / 1e9, 1), share_of_8TBps=round(need / (us * 1e-6) / LINE, 3))), flush=True)
        us = timed(lambda: jr.free_surface_bcs_(st, on, st.viscosity.η, PHASES, pr, 0.5, *fs_di, handle=h), a.calls)
        print(json.dumps(dict(bench="stepops", op="free_surface_bcs", ni=s, calls=a.calls, gpu=gpu, us_per_call=round(us, 1), launch_bound=True)), flush=True)
        assert h.get_option("stat_stepops_launches") - n0 == 4 * (a.calls + 1)
        del st, th, pr, T, out, r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
