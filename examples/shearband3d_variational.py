#!/usr/bin/env python3
"""The 3D shear band of test/test_shearband3D_MPI.jl under a layer of sticky air, through the native backend: the rock ratio from the phase ratios
(update_rock_ratio!), the viscosity with the air phase removed (compute_viscosity!(…; air_phase)) and the 3D variational Stokes solve
(solve_VariationalStokes!: uniform grid, one block, no free-surface stabilisation), time steps with the stress history carried inside the solve.
    python examples/shearband3d_variational.py [n=32] [steps=3] [air_layers=3]"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package

jr = load_package()


def main(n=32, steps=3, air_layers=3):
    from test_gpu_variational_stokes3d import _upload
    s = jr.miniapps.shearband3d_variational(n, air_layers, iterMax=20_000, nout=500)
    s.kwargs.update(verbose=False)
    st, pr, ρg = _upload(jr, s)
    # pureshear_bc!(stokes, xci, xvi, εbg, backend) sets Vx = εbg x, Vy = εbg y, Vz = -εbg z on the device.  This shear band is plane strain in x-z
    # (test/test_shearband3D_MPI.jl:149-150 sets Vx and Vz only), so Vy goes back to zero
    jr.pureshear_bc_(st, s.grid.xci, s.grid.xvi, s.extra["εbg"], jr.AMDGPUBackend)
    st.V.Vy.zero_()
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
        rock = jr.to_numpy(ϕ.center) > 0
        print(f"step {it}: t = {t:.3f}  PT iterations = {r.iter}  err = {r.err_evo1[-1]:.3e}  max τII = {τII[rock].max():.5f}  max εII = {εII[rock].max():.4f}  "
              f"rock cells = {rock.mean():.2f}", flush=True)
    return r


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 32, int(a[1]) if len(a) > 1 else 3, int(a[2]) if len(a) > 2 else 3)
