#!/usr/bin/env python3
"""Grid-based stress rotation and advection (rotate_stress!(stokes, grid, dt; method, advection)): a Gaussian patch of deviatoric stress carried through a
quarter turn by a solid-body rotation V = Ω x r, in steps of compute_dt / 2 (the last one shortened to land on the quarter turn).  compute_dt bounds the
Courant number of each axis by 0.9, and the unsplit upwind step is stable while their sum stays <= 1: in the corners of a rotating box both components are at
their maxima, so the full compute_dt step (sum 1.8 there) grows without bound from the corners inwards; half of it is stable everywhere.  The exact answer is
the patch displaced to R r0 with its tensor rotated to R T0 R'.  Prints, for :matrix and :jaumann, the error against it: of the whole field (dominated by the diffusion
of the first-order upwind step) and of the tensor's orientation at the patch, which is what the rotation term is responsible for.
    python examples/stress_rotation2d.py [n=128]"""
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
import _stress_rotation as SR

T0 = dict(xx=1.0, yy=-1.0, xy=0.5)            # the patch's tensor before the turn
R0, SIGMA, OMEGA = (0.5, 0.0), 0.15, 1.0      # its centre, its width, the angular velocity


def _patch(loc, coords, centre):
    x, y = SR.location_coords(loc, coords)
    return np.exp(-((x - centre[0]) ** 2 + (y - centre[1]) ** 2) / (2.0 * SIGMA ** 2))


def main(n=128, quiet=False):
    """returns {method: (relative L1 error of the field, error of the principal direction at the patch in radians)}"""
    dev = torch.device("cuda", torch.cuda.current_device())
    ni, li, origin = (n, n), (2.0, 2.0), (-1.0, -1.0)
    jr.finalize_global_grid()
    grid = jr.Geometry(ni, li, origin=origin)
    coords = SR.grid_coords(ni, li, origin)
    V = SR.rigid_velocity(ni, li, OMEGA, origin=origin)
    members = dict(SR.MEMBERS2)
    comp = dict(xx="xx", yy="yy", xy_c="xy", xy="xy")
    turn = 0.5 * np.pi
    Rq = SR.rotation_matrix((0.0, 0.0, 1.0), turn)[:2, :2]
    centre1 = Rq @ np.array(R0)
    T1 = dict(zip(("xx", "yy", "xy"), SR.voigt(Rq @ SR.tensor((T0["xx"], T0["yy"], T0["xy"])) @ Rq.T)))
    exact = {k: T1[comp[k]] * _patch(loc, coords, centre1) for k, loc in members.items()}
    out = {}
    for method in ("matrix", "jaumann"):
        st = jr.StokesArrays(jr.AMDGPUBackend, ni)
        for k, loc in members.items():
            getattr(st.τ, k).copy_(from_numpy(T0[comp[k]] * _patch(loc, coords, R0), dev))
        st.V.Vx.copy_(from_numpy(V[0], dev))
        st.V.Vy.copy_(from_numpy(V[1], dev))
        jr.compute_vorticity_(st, grid)
        t, steps = 0.0, 0
        while t < turn / OMEGA * (1.0 - 1e-12):
            dt = min(jr.compute_dt_(st, grid.di["center"]) / len(ni), turn / OMEGA - t)       # / ndims: the sum of the two Courant numbers stays <= 0.9
            jr.rotate_stress_(st, grid, dt, method=method)
            for k in members:
                getattr(st.τ, k).copy_(getattr(st.τ_o, k))
            t += dt
            steps += 1
        got = {k: jr.to_numpy(getattr(st.τ, k)) for k in members}
        l1 = sum(np.abs(got[k] - exact[k]).sum() for k in members) / sum(np.abs(exact[k]).sum() for k in members)
        # the principal direction at the centre nearest to the displaced patch: atan2(2 xy, xx - yy) / 2 against the exact tensor's
        i, j = (int(np.argmin(np.abs(coords[d][0] - centre1[d]))) for d in range(2))
        angle = lambda xx, yy, xy: 0.5 * np.arctan2(2.0 * xy, xx - yy)
        dθ = angle(got["xx"][i, j], got["yy"][i, j], got["xy_c"][i, j]) - angle(T1["xx"], T1["yy"], T1["xy"])
        dθ = (dθ + 0.5 * np.pi) % np.pi - 0.5 * np.pi
        out[method] = (float(l1), float(dθ))
        if not quiet:
            print(f"{method:8s} n = {n}: {steps} steps to a quarter turn, relative L1 error {l1:.3e}, principal direction off by {dθ:+.3e} rad, "
                  f"peak |τxx| {np.abs(got['xx']).max():.3f} (exact {abs(T1['xx']):.3f})", flush=True)
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
