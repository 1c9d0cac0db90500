#!/usr/bin/env python3
"""A moving free surface in 3D without particles: the topography A cos(2 π x / Lx) cos(2 π y / Ly) about mid-height on a dense viscous layer under sticky air,
relaxing under gravity.  The surface is a Topography (heights h(x, y) at the vertex positions); per step compute_rock_fraction!, update_phases_given_topography!,
update_phase_ratios_3D!, compute_ρg!, compute_viscosity!(…; air_phase), solve_VariationalStokes!, compute_dt, WENO_advection! of the two phase fields and
advect_topography! -- the loop of free_surface_relaxation2d.py with the 3D operators.  The linear theory for a layer much deeper than the wavelength gives an
amplitude ~ exp(-t / t_k) with t_k = 2 η k / (ρ g), k = 2 π sqrt(1 / Lx² + 1 / Ly²); the layer here is 0.6 deep in a unit box, so the measured time is longer.
Prints the amplitude (max h - min h) / 2 and the rock volume Σ ϕ.center dx dy dz per step, the fitted relaxation time and the drift of the volume per step.

The step is compute_dt(stokes, di, dt_diff) with dt_diff a quarter of the relaxation time 4 π η / (ρ g λ) of the longest wavelength λ = max(Lx, Ly): the
Courant step alone outgrows the relaxation time once the surface is nearly flat (the 2D example's header), and the 3D variational driver has no free-surface
stabilisation to lean on.
    python examples/free_surface_relaxation3d.py [n=32] [steps=10]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()

H0, AMP = 0.6, 0.05          # mean height and amplitude of the surface in a unit box


def main(n=32, steps=10, iterMax=30_000, dt_cap=0.25, quiet=False):
    """returns [(t, amplitude, rock volume)] at the start of every step and after the last one.  dt_cap: the largest step as a share of t_r (None: compute_dt alone)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    ni, li = (n, n, n), (1.0, 1.0, 1.0)
    jr.finalize_global_grid()
    grid = jr.Geometry(ni, li, origin=(0.0, 0.0, 0.0))
    di = grid.di["center"]
    air = 2
    phases = [dict(eta=1.0, G=float("inf"), Kb=float("inf"), g=1.0, density=dict(kind="constant", rho0=1.0)),
              dict(eta=1.0e-2, G=float("inf"), Kb=float("inf"), density=dict(kind="constant", rho0=1.0e-3))]
    cutoff = (1.0e-2, 1.0e2)
    topo = jr.Topography(jr.AMDGPUBackend, ni[:2])
    x, y = np.meshgrid(grid.xvi[0], grid.xvi[1], indexing="ij")
    topo.fill_(H0 + AMP * np.cos(2.0 * np.pi * x / li[0]) * np.cos(2.0 * np.pi * y / li[1]))
    fields = (jr.fzeros(ni, dev), jr.fzeros(ni, dev, 1.0))          # rock, air: all air; the first phase correction fills the rock below the surface
    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    ρg = tuple(jr.fzeros(ni, dev) for _ in range(3))
    args = dict(T=jr.fzeros(tuple(m + 2 for m in ni), dev, 1.0), P=st.P)
    V_c = tuple(jr.fzeros(ni, dev) for _ in range(3))
    weno = jr.WENO5(jr.AMDGPUBackend, 2, ni)
    faces = ("left", "right", "front", "back", "top", "bot")
    bcs = jr.VelocityBoundaryConditions(free_slip={k: True for k in faces}, no_slip={k: False for k in faces})
    pt = jr.PTStokesCoeffs(li, di, ϵ_rel=1.0e-6, ϵ_abs=1.0e-8, CFL=0.9 / np.sqrt(3.1))
    kwargs = dict(iterMax=iterMax, nout=500, verbose=False, viscosity_cutoff=cutoff, air_phase=air)
    cell = di[0] * di[1] * di[2]

    def record(t, it, r=None):
        h = jr.to_numpy(topo.h)
        row = (t, 0.5 * float(h.max() - h.min()), float(ϕ.center.sum()) * cell)
        if not quiet:
            tail = "" if r is None else f"  (last solve: {r.iter} PT iterations, err {r.err_evo1[-1] if len(r.err_evo1) else float('nan'):.2e})"
            print(f"step {it}: t = {row[0]:8.4f}  amplitude = {row[1]:.6f}  rock volume = {row[2]:.8f}{tail}", flush=True)
        return row
    η, ρgr = phases[0]["eta"], phases[0]["density"]["rho0"] * phases[0]["g"]
    t_r = 4.0 * np.pi * η / (ρgr * max(li[0], li[1]))                                        # the longest wavelength: the limit of the step
    t_k = 2.0 * η * 2.0 * np.pi * np.sqrt(1.0 / li[0] ** 2 + 1.0 / li[1] ** 2) / ρgr           # the mode of the initial surface, deep-layer theory
    dt_max = float("inf") if dt_cap is None else dt_cap * t_r
    t, dt, out, r = 0.0, min(1.0, dt_max), [], None
    for it in range(1, steps + 1):
        jr.compute_rock_fraction_(ϕ, topo, grid)
        out.append(record(t, it - 1, r))
        jr.update_phases_given_topography_(fields, topo, grid, air)
        jr.update_phase_ratios_3D_(pr, fields, grid)
        jr.compute_ρg_(ρg, pr, phases, args)
        jr.compute_viscosity_(st, pr, None, phases, cutoff, air_phase=air)
        jr.flow_bcs_(st, bcs)
        r = jr.solve_VariationalStokes_(st, pt, grid, bcs, ρg, pr, ϕ, phases, None, dt, None, kwargs=kwargs)
        dt = jr.compute_dt_(st, di, dt_max)
        jr.velocity2center_(*V_c, st.V.Vx, st.V.Vy, st.V.Vz)
        for f in fields:
            jr.WENO_advection_(f, V_c, weno, di, dt)
        jr.advect_topography_(topo, st.V, grid, dt)
        t += dt
    jr.compute_rock_fraction_(ϕ, topo, grid)
    out.append(record(t, steps, r))
    if not quiet:
        amps = [a for _, a, _ in out]
        mono = all(b < a for a, b in zip(amps, amps[1:]))
        rate = np.log(amps[0] / amps[-1]) / t if t > 0 and amps[-1] > 0 else float("nan")
        drift = out[-1][2] / out[0][2] - 1.0
        print(f"amplitude {amps[0]:.6f} -> {amps[-1]:.6f} over t = {t:.4f}: {'monotone decay' if mono else 'NOT monotone'}, fitted relaxation time {1.0 / rate:.3f} "
              f"(deep-layer theory 2 η k / (ρ g) = {t_k:.3f}; step limit {dt_max:.3f}); rock volume drift {drift:+.3e} in all, {drift / steps:+.3e} per step")
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 32, int(a[1]) if len(a) > 1 else 10)
