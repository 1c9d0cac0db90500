#!/usr/bin/env python3
"""A quarter turn of a box of 3D particles: a rigid rotation about a tilted axis through the centre of the box [-1, 1]^3 at Courant number 0.5, two phases split by
the plane x + z = 0, through the 3D chain advection_ -> move_particles_ -> particle2centroid_ -> update_phase_ratios_ on particles from
init_particles(backend, nxcell, max_xcell, min_xcell, *grid.xi_vel).  3D injection is not built: the corners of the rotating box lose their particles through the
walls (n_outside reports them) and the cells they leave are not refilled (n_empty reports those).

Checked in every step, and the script fails if one does not hold:
  * n_far == n_overflow == 0;
  * the particle count of each phase changes only by the particles that left the box: no count grows, and the two losses add up to n_outside;
  * phase_ratios.center sums to 1 over the phases in every cell that update_phase_ratios_ wrote (the cells it left alone are the ones n_empty counts).
    python examples/rotating_box3d_particles.py [n=32] [nxcell=8]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd.arrays import from_numpy

AXIS = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
OMEGA = 1.0


def main(n=32, nxcell=8, quiet=False):
    """returns the per-step records"""
    dev = torch.device("cuda", torch.cuda.current_device())
    ni, li, origin = (n, n, n), (2.0, 2.0, 2.0), (-1.0, -1.0, -1.0)
    grid = jr.Geometry(ni, li, origin=origin)
    w = OMEGA * AXIS
    rot = (lambda X, Y, Z: w[1] * Z - w[2] * Y, lambda X, Y, Z: w[2] * X - w[0] * Z, lambda X, Y, Z: w[0] * Y - w[1] * X)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    vmax = 0.0
    for comp, gv, f in zip((st.V.Vx, st.V.Vy, st.V.Vz), grid.xi_vel, rot):          # stokes.V with its ghost layers
        X, Y, Z = np.meshgrid(*gv, indexing="ij")
        v = np.asfortranarray(f(X, Y, Z) + 0.0 * X)
        vmax = max(vmax, float(np.abs(v).max()))
        comp.copy_(from_numpy(v, dev))
    dt0 = 0.5 * (li[0] / n) / vmax          # Courant number 0.5
    p = jr.init_particles(jr.AMDGPUBackend, nxcell, 3 * nxcell, nxcell // 2, *grid.xi_vel, rng=np.random.default_rng(20261021))
    pPhases, pT = jr.init_cell_arrays(p, 2)
    px, py, pz = p.coords
    act = p.index != 0
    pPhases.copy_(torch.where(act, torch.where(px + pz < 0.0, 1.0, 2.0), 0.0))
    pT.copy_(torch.where(act, 1000.0 + 500.0 * py, 0.0))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    T = jr.fzeros(ni, dev)
    count = lambda: [int((pPhases == k).sum()) for k in (1.0, 2.0)]
    n0, before = int(act.sum()), count()
    turn = 0.5 * np.pi / OMEGA
    t, step, rk2, rows = 0.0, 0, jr.RungeKutta2(), []
    while t < turn * (1.0 - 1e-12):
        dt = min(dt0, turn - t)
        jr.advection_(p, rk2, st.V, dt, grid=grid)
        mc = jr.move_particles_(p, (pPhases, pT))          # raises when n_far or n_overflow is not zero
        assert mc["n_far"] == 0 and mc["n_overflow"] == 0, mc
        after = count()
        lost = [b - a for b, a in zip(before, after)]
        assert min(lost) >= 0 and sum(lost) == mc["n_outside"] and sum(after) == mc["n_active_after"], (before, after, mc)
        before = after
        jr.particle2centroid_(T, pT, p)
        pr.center.fill_(float("nan"))          # what the update leaves alone stays NaN: the cells n_empty counts
        n_empty = jr.update_phase_ratios_(pr, p, pPhases)
        total = pr.center.sum(dim=0)
        written = ~torch.isnan(total)
        assert int((~written).sum()) <= n_empty and float((total[written] - 1.0).abs().max()) < 1e-12, (step, n_empty)
        t += dt
        step += 1
        rows.append(dict(step=step, left=mc["n_outside"], particles=mc["n_active_after"], phase1=after[0], phase2=after[1], n_empty=n_empty,
                         empty_cells=int((~written).sum())))
        if not quiet and (step % 10 == 0 or t >= turn * (1.0 - 1e-12)):
            r = rows[-1]
            print(f"step {step:3d}: {r['left']:5d} left the box, {r['particles']:8d} particles ({r['phase1']} / {r['phase2']}), n_empty {r['n_empty']:5d} "
                  f"({r['empty_cells']} cell centres)", flush=True)
    per_cell = (p.index != 0).sum(dim=3)
    print(f"n = {n}, {nxcell} per cell, max_xcell = {p.max_xcell}: {step} steps to a quarter turn at Courant 0.5; {int(per_cell.sum())} of {n0} particles at the end "
          f"({sum(r['left'] for r in rows)} left the box); the fullest cell holds {int(per_cell.max())}, {int((per_cell == 0).sum())} cells are empty; n_far and "
          f"n_overflow were 0 in every step, the phase counts changed only by n_outside, and the centre ratios summed to 1 wherever they were written", flush=True)
    return rows


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32, int(sys.argv[2]) if len(sys.argv) > 2 else 8)
