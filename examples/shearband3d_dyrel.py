#!/usr/bin/env python3
"""The 3D shear band (the family of examples/shearband3d_variational.py: matrix G = 1 with a spherical inclusion G = 0.5, pure shear in x-z, free slip) solved with
DYREL through the native backend: DYREL(backend, stokes, rheology, phase_ratios, di, dt) and one solve_DYREL! per time step with the keywords of the 2D example
(nout = 50, rel_drop = 0.5, viscosity_relaxation = 1, linear_viscosity), the stress history carried inside the solve.  Prints the inner / Powell-Hestenes
iteration counts, the last relative residual, max τxx, the range of τII and the visco-elastic solution 2 ε η (1 - exp(-G t / η)).
    python examples/shearband3d_dyrel.py [n=32] [steps=5]"""
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package

jr = load_package()


def main(n=32, steps=5):
    import _dyrel3d as dy
    from test_gpu_dyrel3d import Dev
    ni = (n, n, n)
    a, phases, di, dt = dy.shearband_state(*ni)
    g = Dev(jr, a, dy.new_dyrel(ni), phases, di, dt)
    dyrel = jr.DYREL(jr.AMDGPUBackend, g.st, phases, g.pr, di, dt, ϵ=1.0e-6)
    kw = dict(verbose_PH=False, verbose_DR=False, iterMax=50.0e3, nout=50, rel_drop=0.5, λ_relaxation_PH=1, λ_relaxation_DR=1, viscosity_relaxation=1,
              linear_viscosity=True, viscosity_cutoff=(-math.inf, math.inf))
    t = 0.0
    for it in range(1, steps + 1):
        r = jr.solve_DYREL_(g.st, g.ρg, dyrel, g.bcs, g.pr, phases, None, di, dt, kwargs=kw)
        jr.tensor_invariant_(g.st.τ)
        t += dt
        τII = jr.to_numpy(g.st.τ.II)
        print(f"step {it}: t = {t:.2f}  iterations = {r.iter} in {r.itPH} PH steps  err = {r.err_evo_tot[-1]:.3e}  max τxx = {float(g.st.τ.xx.max()):.6f}  "
              f"τII in [{τII.min():.6f}, {τII.max():.6f}]  visco-elastic solution = {2 * (1 - math.exp(-t)):.4f}", flush=True)
    return r


if __name__ == "__main__":
    v = sys.argv[1:]
    main(int(v[0]) if v else 32, int(v[1]) if len(v) > 1 else 5)
