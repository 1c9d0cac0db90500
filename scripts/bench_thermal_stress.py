#!/usr/bin/env python3
"""it/s of the multiphase VEP drivers without and with args.ΔT (the thermal form of compute_P!), one process, the two forms alternating:

    python scripts/bench_thermal_stress.py [n3d=256] [n2d=1024] [reps=5] [out=profiles/thermal_stress_bench.txt]

The 3D shear band of bench_extras.cfg_shearband3d and the 2D shear band of cfg_shearband, on the same arrays for both legs.  The phases carry a T_Density (α = 3e-5)
with ρg left to the caller (has_density = 0), so both legs launch the constant-phase-count forms of the pre kernels, the thermal leg their TH instantiations; ΔT is a
random field of 1e-3.  Per leg: one warm-up solve, then `reps` timed solves of more than a second each (host clock around a solve that ends in a device synchronise);
median, minimum and maximum, and the ratio of each thermal solve to the isothermal solve before it.
Expected cost of the thermal form: one more centre array read per iteration, 744 / 736 B/cell in 3D."""
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package

jr = load_package()
import torch
from justrelax_jl_amd import _lib
from justrelax_jl_amd import stokes as st_mod
from justrelax_jl_amd.arrays import from_numpy


def legs(nd, n, iters, warm, reps, h):
    dev = torch.device("cuda", torch.cuda.current_device())
    s = (jr.miniapps.shearband3d if nd == 3 else jr.miniapps.shearband2d)(n, iterMax=iters - 1, nout=10 ** 9)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-300
    st = jr.StokesArrays(jr.AMDGPUBackend, s.ni)
    for k, t in dict(Vx=st.V.Vx, Vy=st.V.Vy, Vz=getattr(st.V, "Vz", None), eta=st.viscosity.η).items():
        if t is not None:
            t.copy_(from_numpy(s.arrays[k], dev))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, s.ni)
    names = (("phase_c", "center"), ("phase_yz", "yz"), ("phase_xz", "xz"), ("phase_xy", "xy")) if nd == 3 else (("phase_c", "center"), ("phase_v", "vertex"))
    for k, name in names:
        getattr(pr, name).copy_(from_numpy(s.arrays[k], dev))
    rh = st_mod.rheology_table([dict(ph, density=dict(kind="T", rho0=1.0, alpha=3.0e-5)) for ph in s.extra["phases"]])
    rh.has_density = 0          # ρg stays the caller's zeros: the pre kernels of the benchmark lines, not their update_ρg! forms
    grid_, pt, bcs, dt, ni = s.grid, s.pt, s.flow_bcs, s.dt, s.ni
    del s
    ρg = tuple(jr.fzeros(ni, dev) for _ in range(nd))
    ΔT = (torch.rand(ni[::-1], dtype=torch.float64, device=dev) * 1.0e-3).permute(*range(nd - 1, -1, -1))
    kw = dict(nout=10 ** 9, verbose=False, **(dict(iterMin=10 ** 9) if nd == 2 else {}))

    def run(k, args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = jr.solve_(st, pt, grid_, bcs, ρg, pr, rh, args, dt, None, kwargs=dict(kw, iterMax=k - 1), handle=h)
        torch.cuda.synchronize()
        return r.iter / (time.perf_counter() - t0)
    forms = (("isothermal", None), ("thermal", dict(ΔT=ΔT)))
    for _, args in forms:
        run(warm, args)
    rates = {name: [] for name, _ in forms}
    for _ in range(reps):
        for name, args in forms:
            rates[name].append(run(iters, args))
    assert bool(torch.isfinite(st.P).all())
    out = {"workload": f"shear band {n}^{nd} ({nd}D multiphase VEP)", "iterations": iters, "reps": reps}
    for name, v in rates.items():
        out[name] = dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1), runs=[round(x, 1) for x in v])
    out["thermal_over_isothermal_median"] = round(out["thermal"]["median"] / out["isothermal"]["median"], 4)
    # the device's rate drifts over a process (both legs step down together): the ratio of each thermal solve to the isothermal solve right before it does not carry the drift
    pairs = [t / i for t, i in zip(rates["thermal"], rates["isothermal"])]
    out["paired_ratio"] = dict(median=round(statistics.median(pairs), 4), min=round(min(pairs), 4), max=round(max(pairs), 4), pairs=[round(x, 4) for x in pairs])
    return out


def main(n3=256, n2=1024, reps=5, out="profiles/thermal_stress_bench.txt"):
    h = _lib.default_handle(0)
    # timed windows of more than a second (476 iterations at 256^3, 14,305 at 1024^2); the warm-up solve runs a quarter of that, long enough to take every path of the timed one
    # (observed first iterations, the captured graphs of small grids)
    it3, it2 = max(120, min(20000, int(8e9 / n3 ** 3))), max(2000, min(200000, int(1.5e10 / n2 ** 2)))
    rows = [legs(3, n3, it3, max(64, it3 // 4), reps, h), legs(2, n2, it2, max(64, it2 // 4), reps, h)]
    text = "\n".join(json.dumps(r, ensure_ascii=False) for r in rows)
    print(text, flush=True)
    if out:
        p = Path(out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text("# scripts/bench_thermal_stress.py: it/s without and with args.ΔT, alternating, one process (median, min, max over the timed solves)\n" + text + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 256, int(a[1]) if len(a) > 1 else 1024, int(a[2]) if len(a) > 2 else 5, a[3] if len(a) > 3 else "profiles/thermal_stress_bench.txt")
