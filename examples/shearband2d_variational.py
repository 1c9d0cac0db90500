#!/usr/bin/env python3
"""The shear band of miniapps/benchmarks/stokes2D/shear_band/ShearBand2D_variational.jl with an air layer on top, through the native backend: the rock ratio from
the phase ratios (update_rock_ratio!), the viscosity with the air phase removed (compute_viscosity!(…; air_phase)) and the 2D variational Stokes solve
(solve_VariationalStokes!: uniform grid, one block), time steps with the stress history carried inside the solve, and a .vtr file per step.
    python examples/shearband2d_variational.py [n=64] [steps=5] [air_rows=4] [outdir=shearband2d_variational_out]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package

jr = load_package()


def main(n=64, steps=5, air_rows=4, outdir="shearband2d_variational_out"):
    from test_gpu_variational_stokes import _upload
    out = Path(outdir)
    out.mkdir(parents=True, exist_ok=True)
    s = jr.miniapps.shearband2d_variational(n, air_rows, iterMax=50_000, nout=1000)
    s.kwargs.update(verbose=False)
    st, pr, ρg = _upload(jr, s)
    air = s.kwargs["air_phase"]
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    jr.update_rock_ratio_(ϕ, pr, air)
    jr.compute_viscosity_(st, pr, None, s.extra["phases"], s.kwargs["viscosity_cutoff"], air_phase=air)
    t = 0.0
    for it in range(1, steps + 1):
        r = jr.solve_VariationalStokes_(st, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
        jr.tensor_invariant_(st.ε)
        t += s.dt
        τII, εII = jr.to_numpy(st.τ.II), jr.to_numpy(st.ε.II)
        print(f"step {it}: t = {t:.3f}  PT iterations = {r.iter}  err = {r.err_evo1[-1]:.3e}  max τII = {τII.max():.5f}  max εII = {εII.max():.4f}", flush=True)
        Vx_v, Vy_v = jr.fzeros((n + 1, n + 1), st.P.device), jr.fzeros((n + 1, n + 1), st.P.device)
        jr.velocity2vertex_(Vx_v, Vy_v, st.V.Vx, st.V.Vy)
        jr.save_vtk(str(out / f"step_{it:04d}"), s.grid.xvi, s.grid.xci, {}, dict(tauII=τII, epsII=εII, P=jr.to_numpy(st.P), rock_ratio=jr.to_numpy(ϕ.center)),
                    (jr.to_numpy(Vx_v), jr.to_numpy(Vy_v)), t=t)
    return r


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 64, int(a[1]) if len(a) > 1 else 5, int(a[2]) if len(a) > 2 else 4, a[3] if len(a) > 3 else "shearband2d_variational_out")
