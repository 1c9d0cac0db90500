#!/usr/bin/env python3
"""The quarter turn of stress_rotation2d_particles.py -- the same box, solid-body rotation, seeding and steps of compute_dt / 2 -- with
inject_particles_phase_ after every move: the corners of a rotating box lose their particles through the walls, and the cells they leave thin are refilled from
their neighbours.  The particles carry a phase (1 left of the centre line, 2 right of it, taken from the nearest particle on injection), a temperature that is
refilled from a vertex field, and an identity that a new particle copies from its donor.  Per step it prints the particle count, n_deficient, n_injected and
n_no_donor of the injection and n_empty of update_phase_ratios_; with `compare` it runs the same loop without the injection beside it.  Recorded in
examples/README.md, not asserted.
    python examples/rotating_box2d_injection.py [n=128] [nxcell=12] [compare]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "examples"))
import numpy as np
import torch
import stress_rotation2d as G          # loads the package; OMEGA and the velocity of the set-up

jr, SR = G.jr, G.SR
from_numpy = G.from_numpy


def main(n=128, nxcell=12, inject=True, quiet=False):
    """returns the per-step records"""
    dev = torch.device("cuda", torch.cuda.current_device())
    ni, li, origin = (n, n), (2.0, 2.0), (-1.0, -1.0)
    jr.finalize_global_grid()
    grid = jr.Geometry(ni, li, origin=origin)
    V = SR.rigid_velocity(ni, li, G.OMEGA, origin=origin)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    st.V.Vx.copy_(from_numpy(V[0], dev))
    st.V.Vy.copy_(from_numpy(V[1], dev))
    p = jr.init_particles(jr.AMDGPUBackend, nxcell, 2 * nxcell, nxcell // 2, grid, ni, rng=np.random.default_rng(20261021))
    pPhases, pT, pid = jr.init_cell_arrays(p, 3)
    px, py = p.coords
    act = p.index != 0
    pPhases.copy_(torch.where(act, torch.where(px < 0.0, 1.0, 2.0), 0.0))
    pT.copy_(torch.where(act, 1000.0 + 500.0 * py, 0.0))
    pid.copy_(torch.where(act, torch.arange(act.numel(), device=dev, dtype=torch.float64).reshape(act.shape) + 1.0, 0.0))
    Tv = from_numpy(np.asfortranarray(np.broadcast_to(1000.0 + 500.0 * np.asarray(grid.xvi[1])[None, :], (n + 1, n + 1))), dev)
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    n0 = int(act.sum())
    turn = 0.5 * np.pi
    t, step, rk2, rows = 0.0, 0, jr.RungeKutta2(), []
    while t < turn / G.OMEGA * (1.0 - 1e-12):
        dt = min(jr.compute_dt_(st, grid.di["center"]) / len(ni), turn / G.OMEGA - t)
        jr.advection_(p, rk2, st.V, dt)
        mc = jr.move_particles_(p, (pPhases, pT, pid))
        ic = jr.inject_particles_phase_(p, pPhases, (pT, pid), (Tv, None)) if inject else dict(n_active_after=mc["n_active_after"], n_deficient=0, n_injected=0, n_no_donor=0)
        n_empty = jr.update_phase_ratios_(pr, p, pPhases)
        t += dt
        step += 1
        rows.append(dict(step=step, left=mc["n_outside"], particles=ic["n_active_after"], n_deficient=ic["n_deficient"], n_injected=ic["n_injected"],
                         n_no_donor=ic["n_no_donor"], n_empty=n_empty))
        if not quiet:
            r = rows[-1]
            print(f"step {step:3d}: {r['left']:5d} left the box, {r['particles']:7d} particles, n_deficient {r['n_deficient']:4d}, n_injected {r['n_injected']:5d}, "
                  f"n_no_donor {r['n_no_donor']:3d}, n_empty {r['n_empty']:4d}", flush=True)
    per_cell = (p.index != 0).sum(dim=2)
    print(f"{'with' if inject else 'without'} injection, n = {n}, {nxcell} per cell, min_xcell = {p.min_xcell}: {step} steps to a quarter turn; {int(per_cell.sum())} of {n0} "
          f"particles at the end ({sum(r['left'] for r in rows)} left the box, {sum(r['n_injected'] for r in rows)} injected); the thinnest cell holds {int(per_cell.min())}, "
          f"{int((per_cell == 0).sum())} cells are empty; n_empty summed over the steps {sum(r['n_empty'] for r in rows)}, in the last step {rows[-1]['n_empty']}; "
          f"n_no_donor summed {sum(r['n_no_donor'] for r in rows)}", flush=True)
    return rows


if __name__ == "__main__":
    pos = [x for x in sys.argv[1:] if x != "compare"]
    n = int(pos[0]) if len(pos) > 0 else 128
    nxcell = int(pos[1]) if len(pos) > 1 else 12
    main(n, nxcell)
    if "compare" in sys.argv[1:]:
        main(n, nxcell, inject=False, quiet=True)
