#!/usr/bin/env python3
"""Thermal stresses of a heated inclusion (the coupling test/test_thermalstresses.jl exercises, on a particle-free set-up): a circular inclusion with a heat source in a
compressible elastic host, closed free-slip box, no gravity.  Per step: heatdiffusion_PT! (array form; it ends with update_ΔT!, ΔT = T - Told), then the multiphase 2D
solve! with args = (; ΔT = thermal.ΔT) -- thermal.ΔT itself (ni .+ 2), read at the cell's own index as the reference reads it (PressureKernels.jl:149).  compute_P! then
carries the source α ΔT / dt and the inclusion builds pressure.  Prints the peak over-pressure beside Kb α ΔT of the inclusion, the pressure a body that cannot expand
at all would build: the elastic host gives way, so the peak stays below it.
    python examples/thermal_stress2d.py [n=64] [steps=4]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd.arrays import from_numpy


def main(n=64, steps=4):
    dev = torch.device("cuda", torch.cuda.current_device())
    ni, li = (n, n), (1.0, 1.0)
    jr.init_global_grid(n, n, 1)
    di = tuple(l / m for l, m in zip(li, ni))
    grid = jr.Geometry(ni, li)
    # host (phase 1) and inclusion (phase 2): linear viscous in series with a compressible elastic element; the T_Density gives the thermal expansion α
    Kb, α, η, G = 4.0, 1.0e-2, 10.0, 1.0
    phases = [dict(eta=η, G=G, Kb=Kb, density=dict(kind="T", rho0=1.0, alpha=α), g=0.0), dict(eta=η, G=G, Kb=Kb, density=dict(kind="T", rho0=1.0, alpha=α))]
    xc, yc = grid.xci
    xv, yv = grid.xvi
    inside = lambda x, y: ((x[:, None] - 0.5) ** 2 + (y[None, :] - 0.5) ** 2) <= 0.15 ** 2
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    for t, m in ((pr.center, inside(xc, yc)), (pr.vertex, inside(xv, yv))):
        t.copy_(from_numpy(np.asfortranarray(np.stack([1.0 - m, 1.0 * m])), dev))
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    st.viscosity.η.fill_(η)
    st.viscosity.ηv.fill_(η)
    ρg = (jr.fzeros(ni, dev), jr.fzeros(ni, dev))
    on = dict(left=True, right=True, top=True, bot=True)
    flow_bcs = jr.VelocityBoundaryConditions(free_slip=on, no_slip={k: False for k in on})
    pt = jr.PTStokesCoeffs(li, di, ϵ_rel=1.0e-6, ϵ_abs=1.0e-9)
    # heat: K = 1, ρCp = 100, a source of 100 in the inclusion (one degree per unit time); dt is well below the diffusion time across the
    # inclusion (0.15^2 ρCp / K) and keeps G dt within a factor 20 of η, which the pseudo-transient iteration of the Stokes solve needs to converge quickly
    thermal = jr.ThermalArrays(jr.AMDGPUBackend, ni)
    thermal.H.copy_(from_numpy(np.asfortranarray(100.0 * inside(xc, yc)), dev))
    dt = 0.5
    K, ρCp = jr.fzeros(ni, dev, 1.0), jr.fzeros(ni, dev, 100.0)
    pt_thermal = jr.PTThermalCoeffs(jr.AMDGPUBackend, K, ρCp, dt, di, li, CFL=0.5 / np.sqrt(2.1), ϵ=1.0e-8)
    thermal_bc = jr.TemperatureBoundaryConditions(no_flux=on)
    c = (n // 2, n // 2)
    T_start = float(thermal.T[c[0] + 1, c[1] + 1])
    for it in range(1, steps + 1):
        rt = jr.heatdiffusion_PT_(thermal, pt_thermal, thermal_bc, K, ρCp, dt, grid, kwargs=dict(iterMax=20_000, nout=50, verbose=False))      # ends with update_ΔT!
        r = jr.solve_(st, pt, grid, flow_bcs, ρg, pr, phases, dict(ΔT=thermal.ΔT), dt, None,
                      kwargs=dict(iterMax=20_000, iterMin=10, nout=100, verbose=False, viscosity_cutoff=(-np.inf, np.inf)))
        rise = float(thermal.T[c[0] + 1, c[1] + 1]) - T_start
        print(f"step {it}: heat iterations = {int(rt.iter_count[-1])}  Stokes iterations = {r.iter} (err {r.err_evo1[-1]:.2e})  "
              f"peak over-pressure = {float(st.P.max()):.4e}   Kb α ΔT of the inclusion's centre = {Kb * α * rise:.4e}   max |V| = "
              f"{max(float(st.V.Vx.abs().max()), float(st.V.Vy.abs().max())):.3e}", flush=True)
    return st, thermal


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 64, int(a[1]) if len(a) > 1 else 4)
