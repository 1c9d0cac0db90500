#!/usr/bin/env python3
"""The sinking block of test/test_sinking_block.jl with its material on PARTICLES, as the reference carries it: the set-up of examples/sinking_block2d_fields.py
driven through advection! -> move_particles! -> update_phase_ratios! -> compute_ρg! -> solve!.  Every particle holds its phase (1.0 mantle, 2.0 block); per step:
update_phase_ratios!(phase_ratios, particles, pPhases), compute_ρg!, compute_viscosity!, the multiphase 2D solve!, compute_dt, advection!(particles,
RungeKutta2(), V, dt), move_particles!.  Everything runs on the device; one line per step, with the mean depth of the block's particles beside the value the
fields example prints for the same step (the two routes smear the interface differently: recorded, not asserted).
    python examples/sinking_block2d_particles.py [n=64] [steps=3] [iterMax=20000] [nxcell=12]"""
import contextlib
import io
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "examples"))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd.arrays import from_numpy


def fields_track(n, steps, iterMax):
    """the depths (km) examples/sinking_block2d_fields.py prints, step by step"""
    import sinking_block2d_fields
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        sinking_block2d_fields.main(n, steps, iterMax)
    return [float(v) for v in re.findall(r"mean depth of the block = ([-0-9.eE+]+) km", out.getvalue())]


def main(n=64, steps=3, iterMax=20_000, nxcell=12, quiet=False):
    """returns (particles, pPhases, the depth track in km)"""
    from test_gpu_vep2d import VEP_MAP, _get
    dev = torch.device("cuda", torch.cuda.current_device())
    ref = [] if quiet else fields_track(n, steps, iterMax)
    s = jr.miniapps.sinking_block2d(n, iterMax=iterMax, nout=500)
    di, phases = s.extra["di"], s.extra["phases"]
    st = jr.StokesArrays(jr.AMDGPUBackend, s.ni)
    for k, path in VEP_MAP.items():
        _get(st, path).copy_(from_numpy(s.arrays[k], dev))
    particles = jr.init_particles(jr.AMDGPUBackend, nxcell, 2 * nxcell, nxcell // 2, s.grid, s.ni, rng=np.random.default_rng(1))
    (pPhases,) = jr.init_cell_arrays(particles, 1)
    px, py = particles.coords
    inside = ((px - 250.0e3) ** 2 <= 50.0e3 ** 2) & ((-py - 100.0e3) ** 2 <= 50.0e3 ** 2)          # the block of miniapps.sinking_block2d
    pPhases.copy_(torch.where(particles.index != 0, torch.where(inside, 2.0, 1.0), 0.0))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, s.ni)
    ρg = (jr.fzeros(s.ni, dev), jr.fzeros(s.ni, dev))
    args = dict(T=jr.fzeros(tuple(m + 2 for m in s.ni), dev, 1.0), P=st.P)
    depth = torch.tensor(np.abs(s.grid.xci[1]), device=dev)[None, :]
    rk2 = jr.RungeKutta2()
    t, track = 0.0, []
    for it in range(1, steps + 1):
        n_empty = jr.update_phase_ratios_(pr, particles, pPhases)
        jr.compute_ρg_(ρg, pr, phases, args)
        if it == 1:
            st.P.copy_(ρg[1] * depth)                                                  # init_P! (test_sinking_block.jl:86-89)
        jr.compute_viscosity_(st, pr, args, phases, (-np.inf, np.inf))
        jr.flow_bcs_(st, s.flow_bcs)
        r = jr.solve_(st, s.pt, s.grid, s.flow_bcs, ρg, pr, phases, args, s.dt, None, kwargs=s.kwargs)
        dt = jr.compute_dt_(st, di)
        jr.advection_(particles, rk2, st.V, dt, grid=s.grid)
        counts = jr.move_particles_(particles, (pPhases,))
        t += dt
        block = pPhases == 2.0
        track.append(float((-particles.coords[1][block]).mean()) / 1e3)
        if not quiet:
            beside = f"{ref[it - 1]:.2f} km" if it <= len(ref) else "n/a"
            print(f"step {it}: t = {t / (3600 * 24 * 365.25 * 1e6):.3f} Myr  Stokes iterations = {r.iter} (err {r.err_evo1[-1]:.2e})  particles = {counts['n_active_after']} "
                  f"(left the box: {counts['n_outside']}, empty members: {n_empty})  mean depth of the block = {track[-1]:.2f} km  (fields route: {beside})", flush=True)
    return particles, pPhases, track


if __name__ == "__main__":
    a = sys.argv[1:]
    main(*(int(v) for v in a[:4]))
