#!/usr/bin/env python3
"""A temperature step carried through a rigid rotation with the temperature on particles, as the reference's thermo-mechanical miniapps carry it
(miniapps/subduction/2D/Subduction2D.jl:221-243): per step particle2centroid_(T, pT, particles) into the interior of thermal.T, T_buffer = that interior,
heatdiffusion_PT_ (array form; it ends with update_ΔT!), subgrid_characteristic_time_, centroid2particle_(subgrid_arrays.dt0, dt0, particles),
subgrid_diffusion_centroid_(pT, T_buffer, thermal.ΔT, subgrid_arrays, particles, dt), advection_ and move_particles_ with pT in particle_args.

The box is [-1, 1]^2, the rotation is about its centre, the step is a straight front through the centre: it stays straight, so its 10 % - 90 % width along its
normal, read off the cell centres within 0.6 of the centre after the last particle2centroid_, says how much each route has smeared it beyond what the diffusion
itself does (the erf profile of the same κ t has the width 1.8124 sqrt(4 κ t)).  Three routes:
    d = 1       the particle takes the part of its difference to the grid that decays within dt at its own rate, and the remainder of the grid's change
    d = 0       the particle takes the interpolated change of the grid and keeps every subgrid difference
    overwrite   centroid2particle_(pT, T, particles) after the solve: what a loop has to do without the operator
    python examples/thermal_particles2d.py [n=128] [steps=100] [nxcell=12]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd.arrays import from_numpy

OMEGA = 1.0
T_LO, T_HI = 300.0, 1600.0


def width(Tc, xc, yc, angle):
    """10 % - 90 % distance of the front along its normal (cos angle, sin angle), from the cell centres within 0.6 of the centre in bins of half a cell"""
    X, Y = np.meshgrid(xc, yc, indexing="ij")
    near = X ** 2 + Y ** 2 <= 0.36
    s = (np.cos(angle) * X + np.sin(angle) * Y)[near]
    θ = ((Tc - T_LO) / (T_HI - T_LO))[near]
    half = 0.5 * (xc[1] - xc[0])
    edges = np.arange(-0.5, 0.5 + half, half)
    k = np.digitize(s, edges)
    mid, mean = [], []
    for b in range(1, len(edges)):
        if (k == b).any():
            mid.append(0.5 * (edges[b - 1] + edges[b])), mean.append(θ[k == b].mean())
    mean = np.maximum.accumulate(np.array(mean))
    return float(np.interp(0.9, mean, mid) - np.interp(0.1, mean, mid))


def main(n=128, steps=100, nxcell=12, quiet=False):
    """returns {route: width of the front in cells} and the width of the erf profile of the same κ t"""
    dev = torch.device("cuda", torch.cuda.current_device())
    ni, li, origin = (n, n), (2.0, 2.0), (-1.0, -1.0)
    jr.finalize_global_grid()
    grid = jr.Geometry(ni, li, origin=origin)
    di = tuple(l / m for l, m in zip(li, ni))
    xc, yc = (np.asarray(x, dtype=np.float64) for x in grid.xci)
    xv, yv = (np.asarray(x, dtype=np.float64) for x in grid.xvi)
    xg, yg = origin[0] + (np.arange(n + 2) - 0.5) * di[0], origin[1] + (np.arange(n + 2) - 0.5) * di[1]
    Vx = np.asfortranarray(np.broadcast_to(-OMEGA * yg[None, :], (n + 1, n + 2)))
    Vy = np.asfortranarray(np.broadcast_to(OMEGA * xg[:, None], (n + 2, n + 1)))
    dt = 0.5 * min(di) / (OMEGA * np.hypot(1.0, 1.0))          # Courant number 0.5 at the corners
    # K = 1 and ρCp chosen so that the front diffuses to a width of about four cells over the run: the rest of what a route shows is its own
    K0 = 1.0
    κ = (4.0 * di[0] / 1.8124) ** 2 / (4.0 * steps * dt)
    ρCp0 = K0 / κ
    table = [dict(k=K0, Cp=ρCp0, density=dict(kind="PT", rho0=1.0, alpha=0.0, T0=0.0))]
    one_phase = jr.PhaseRatios(jr.AMDGPUBackend, 1, ni)
    one_phase.center.fill_(1.0)
    on = dict(left=True, right=True, top=True, bot=True)
    thermal_bc = jr.TemperatureBoundaryConditions(no_flux=on)
    out = {}
    for route in ("d = 1", "d = 0", "overwrite"):
        st = jr.StokesArrays(jr.AMDGPUBackend, ni)
        st.V.Vx.copy_(from_numpy(Vx, dev)), st.V.Vy.copy_(from_numpy(Vy, dev))
        thermal = jr.ThermalArrays(jr.AMDGPUBackend, ni)
        K, ρCp = jr.fzeros(ni, dev, K0), jr.fzeros(ni, dev, ρCp0)
        pt_thermal = jr.PTThermalCoeffs(jr.AMDGPUBackend, K, ρCp, dt, di, li, CFL=0.5 / np.sqrt(2.1), ϵ=1.0e-8)
        p = jr.init_particles(jr.AMDGPUBackend, nxcell, 2 * nxcell, nxcell // 2, grid, ni, rng=np.random.default_rng(20261021))
        (pT,) = jr.init_cell_arrays(p, 1)
        pT.copy_(torch.where(p.index != 0, torch.where(p.coords[0] > 0.0, T_HI, T_LO), 0.0))
        sa = jr.SubgridDiffusionCellArrays(p, loc="center")
        T_c, T_buffer, dt0 = jr.fzeros(ni, dev, T_LO), jr.fzeros(ni, dev), jr.fzeros(ni, dev)
        rk2 = jr.RungeKutta2()
        for it in range(steps):
            jr.particle2centroid_(T_c, pT, p)          # a cell the particles have left (the corners of a rotating box) keeps its value
            thermal.T[1:-1, 1:-1].copy_(T_c)
            jr.thermal_bcs_(thermal, thermal_bc)
            T_buffer.copy_(T_c)
            jr.heatdiffusion_PT_(thermal, pt_thermal, thermal_bc, K, ρCp, dt, grid, kwargs=dict(iterMax=10_000, nout=20, verbose=False))
            if route == "overwrite":
                T_c.copy_(thermal.T[1:-1, 1:-1])
                jr.centroid2particle_(pT, T_c, p)
            else:
                jr.subgrid_characteristic_time_(dt0, one_phase, table, thermal, st, di)
                jr.centroid2particle_(sa.dt0, dt0, p)
                jr.subgrid_diffusion_centroid_(pT, T_buffer, thermal.ΔT, sa, p, dt, d=1.0 if route == "d = 1" else 0.0)
            jr.advection_(p, rk2, st.V, dt)
            jr.move_particles_(p, (pT,))
        jr.particle2centroid_(T_c, pT, p)
        out[route] = width(jr.to_numpy(T_c), xc, yc, OMEGA * steps * dt) / di[0]
        if not quiet:
            print(f"{route:9s} n = {n}, {nxcell} particles per cell, {steps} steps (angle {OMEGA * steps * dt:.3f} rad): the front is {out[route]:.2f} cells wide "
                  f"(10 % - 90 %); subgrid dt₀ / dt = {float(dt0.max()) / dt if route != 'overwrite' else float('nan'):.1f}", flush=True)
    exact = 1.8124 * np.sqrt(4.0 * κ * steps * dt) / di[0]
    if not quiet:
        print(f"the erf profile of the same κ t is {exact:.2f} cells wide", flush=True)
    return out, exact


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(*a)
