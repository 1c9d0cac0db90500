#!/usr/bin/env python3
"""The sinking block of test/test_sinking_block.jl as a particle-free multiphase time loop: the material is two phase FIELDS on the cell centres (mantle and
block, values in [0, 1]) instead of particles, moved the way the docstring of update_phase_ratios_2D! describes (src/phases/PhaseRatios.jl:11-22: "advect both
phase arrays and update phase ratios").  Per step: update_phase_ratios_2D!, compute_ρg!, compute_viscosity!, the multiphase 2D solve!, compute_dt,
velocity2center!, WENO_advection! (Z) of each phase field.  Everything runs on the device; one line per step.
    python examples/sinking_block2d_fields.py [n=64] [steps=3] [iterMax=20000]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd.arrays import from_numpy


def main(n=64, steps=3, iterMax=20_000, quiet=False):
    """returns (phase_ratios, phase_fields, result of the last solve!)"""
    from test_gpu_vep2d import VEP_MAP, _get
    dev = torch.device("cuda", torch.cuda.current_device())
    s = jr.miniapps.sinking_block2d(n, iterMax=iterMax, nout=500)
    di, phases = s.extra["di"], s.extra["phases"]
    st = jr.StokesArrays(jr.AMDGPUBackend, s.ni)
    for k, path in VEP_MAP.items():
        _get(st, path).copy_(from_numpy(s.arrays[k], dev))
    fields = tuple(from_numpy(np.ascontiguousarray(s.arrays["phase_c"][k]), dev) for k in range(2))      # the two phase fields: area fractions of mantle and block
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, s.ni)
    ρg = (jr.fzeros(s.ni, dev), jr.fzeros(s.ni, dev))
    args = dict(T=jr.fzeros(tuple(m + 2 for m in s.ni), dev, 1.0), P=st.P)
    Vx_c, Vy_c = jr.fzeros(s.ni, dev), jr.fzeros(s.ni, dev)
    weno = jr.WENO5(jr.AMDGPUBackend, 2, s.ni)
    depth = torch.tensor(np.abs(s.grid.xci[1]), device=dev)[None, :]
    t, r = 0.0, None
    for it in range(1, steps + 1):
        jr.update_phase_ratios_2D_(pr, fields, s.grid)
        jr.compute_ρg_(ρg, pr, phases, args)
        if it == 1:
            st.P.copy_(ρg[1] * depth)                                                  # init_P! (test_sinking_block.jl:86-89)
        jr.compute_viscosity_(st, pr, args, phases, (-np.inf, np.inf))
        jr.flow_bcs_(st, s.flow_bcs)
        r = jr.solve_(st, s.pt, s.grid, s.flow_bcs, ρg, pr, phases, args, s.dt, None, kwargs=s.kwargs)
        dt = jr.compute_dt_(st, di)
        jr.velocity2center_(Vx_c, Vy_c, st.V.Vx, st.V.Vy)
        for f in fields:
            jr.WENO_advection_(f, (Vx_c, Vy_c), weno, di, dt)
        t += dt
        if not quiet:
            block = float((fields[1] * depth).sum() / fields[1].sum())
            print(f"step {it}: t = {t / (3600 * 24 * 365.25 * 1e6):.3f} Myr  Stokes iterations = {r.iter} (err {r.err_evo1[-1]:.2e})  "
                  f"max |V| = {float(torch.sqrt(Vx_c ** 2 + Vy_c ** 2).max()):.3e} m/s  mean depth of the block = {block / 1e3:.2f} km", flush=True)
    jr.update_phase_ratios_2D_(pr, fields, s.grid)                                       # the ratios of the advected fields
    return pr, fields, r


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 64, int(a[1]) if len(a) > 1 else 3, int(a[2]) if len(a) > 2 else 20_000)
