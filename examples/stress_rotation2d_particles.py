#!/usr/bin/env python3
"""The set-up of stress_rotation2d.py -- a Gaussian patch of deviatoric stress carried through a quarter turn by a solid-body rotation -- with the stress on
particles, as the reference carries it: per step stress2grid_(stokes, pτxx, pτyy, pτxy, particles), [a solver would run here; τ = τ_o stands in for it],
compute_vorticity_, rotate_stress_(pτxx, pτyy, pτxy, pω, stokes, particles, dt), advection_(particles, RungeKutta2(), stokes.V, dt) and move_particles_ with the
three stress fields and pω in particle_args.  The same steps of compute_dt / 2 as the grid example.  It runs the grid example first and prints, in the same
format, the error against the analytically rotated and displaced patch, the error of the principal direction at the patch and the peak.  rotate_stress!
overwrites the particle stress with the grid's in every step (the reference's scheme), so with no solver in between every step averages particle -> grid ->
particle: the patch is smoothed once per step, as the first-order upwind step of the grid route smooths it (examples/README.md records both).  Particles that
leave the box through its corners are dropped (no injection is built); the cells they leave empty keep their value.
    python examples/stress_rotation2d_particles.py [n=128] [nxcell=12]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "examples"))
import numpy as np
import torch
import stress_rotation2d as G          # loads the package

jr, SR = G.jr, G.SR
from_numpy = G.from_numpy


def main(n=128, nxcell=12, quiet=False):
    """returns {method: (relative L1 error of the field, error of the principal direction at the patch in radians, peak |τxx|)}"""
    dev = torch.device("cuda", torch.cuda.current_device())
    ni, li, origin = (n, n), (2.0, 2.0), (-1.0, -1.0)
    jr.finalize_global_grid()
    grid = jr.Geometry(ni, li, origin=origin)
    coords = SR.grid_coords(ni, li, origin)
    V = SR.rigid_velocity(ni, li, G.OMEGA, origin=origin)
    members = dict(SR.MEMBERS2)
    comp = dict(xx="xx", yy="yy", xy_c="xy", xy="xy")
    turn = 0.5 * np.pi
    Rq = SR.rotation_matrix((0.0, 0.0, 1.0), turn)[:2, :2]
    centre1 = Rq @ np.array(G.R0)
    T1 = dict(zip(("xx", "yy", "xy"), SR.voigt(Rq @ SR.tensor((G.T0["xx"], G.T0["yy"], G.T0["xy"])) @ Rq.T)))
    exact = {k: T1[comp[k]] * G._patch(loc, coords, centre1) for k, loc in members.items()}
    out = {}
    for method in ("matrix", "jaumann"):
        st = jr.StokesArrays(jr.AMDGPUBackend, ni)
        st.V.Vx.copy_(from_numpy(V[0], dev))
        st.V.Vy.copy_(from_numpy(V[1], dev))
        p = jr.init_particles(jr.AMDGPUBackend, nxcell, 2 * nxcell, nxcell // 2, grid, ni, rng=np.random.default_rng(20261021))
        pτxx, pτyy, pτxy, pω = jr.init_cell_arrays(p, 4)
        px, py = p.coords
        blob = torch.where(p.index != 0, torch.exp(-((px - G.R0[0]) ** 2 + (py - G.R0[1]) ** 2) / (2.0 * G.SIGMA ** 2)), 0.0)
        pτxx.copy_(G.T0["xx"] * blob), pτyy.copy_(G.T0["yy"] * blob), pτxy.copy_(G.T0["xy"] * blob)
        n0 = int((p.index != 0).sum())
        t, steps, rk2 = 0.0, 0, jr.RungeKutta2()
        while t < turn / G.OMEGA * (1.0 - 1e-12):
            jr.stress2grid_(st, pτxx, pτyy, pτxy, p)
            for k in members:          # where a solver would turn τ_o into the new τ
                getattr(st.τ, k).copy_(getattr(st.τ_o, k))
            jr.compute_vorticity_(st, grid)
            dt = min(jr.compute_dt_(st, grid.di["center"]) / len(ni), turn / G.OMEGA - t)
            jr.rotate_stress_(pτxx, pτyy, pτxy, pω, st, p, dt, method=method)
            jr.advection_(p, rk2, st.V, dt)
            jr.move_particles_(p, (pτxx, pτyy, pτxy, pω))
            t += dt
            steps += 1
        jr.stress2grid_(st, pτxx, pτyy, pτxy, p)
        got = {k: jr.to_numpy(getattr(st.τ_o, k)) for k in members}
        l1 = sum(np.abs(got[k] - exact[k]).sum() for k in members) / sum(np.abs(exact[k]).sum() for k in members)
        i, j = (int(np.argmin(np.abs(coords[d][0] - centre1[d]))) for d in range(2))
        angle = lambda xx, yy, xy: 0.5 * np.arctan2(2.0 * xy, xx - yy)
        dθ = angle(got["xx"][i, j], got["yy"][i, j], got["xy_c"][i, j]) - angle(T1["xx"], T1["yy"], T1["xy"])
        dθ = (dθ + 0.5 * np.pi) % np.pi - 0.5 * np.pi
        peak = float(np.abs(got["xx"]).max())
        out[method] = (float(l1), float(dθ), peak)
        if not quiet:
            print(f"{method:8s} n = {n}, particles ({nxcell} per cell, {int((p.index != 0).sum())} of {n0} still in the box): {steps} steps to a quarter turn, "
                  f"relative L1 error {l1:.3e}, principal direction off by {dθ:+.3e} rad, peak |τxx| {peak:.3f} (exact {abs(T1['xx']):.3f})", flush=True)
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    print("the grid route (rotate_stress_ on grids, first-order upwind):", flush=True)
    G.main(n)
    print("the particle route:", flush=True)
    main(n, int(sys.argv[2]) if len(sys.argv) > 2 else 12)
