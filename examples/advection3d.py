#!/usr/bin/env python3
"""3D WENO-5 advection on one MI355X: a Gaussian blob carried once around by a prescribed solid-body rotation about the cube's (1, 1, 1) diagonal, so that all
three vertex velocities are non-zero and of both signs (WENO5 with a 3-entry ni, WENO_advection_ with three velocities: jrx_weno5_advection3d, the fused form).
After one turn the exact solution is the initial field; prints the L1 error against it and the relative change of the field's sum (the scheme is not in
conservation form, and the clamped stencils make the faces neither inflow nor outflow conditions: the blob stays away from them).
usage: python examples/advection3d.py [n=48] [method=2]"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()

n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
method = int(sys.argv[2]) if len(sys.argv) > 2 else 2
dev = torch.device("cuda", 0)
x = np.linspace(0.0, 1.0, n + 1)
X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
axis = np.ones(3) / np.sqrt(3.0)
ω = 2.0 * np.pi * axis                                       # one turn in T = 1
R = np.stack([X - 0.5, Y - 0.5, Z - 0.5])
V = np.cross(ω, R, axisa=0, axisb=0, axisc=0)                # v = ω × (x - c)
c0 = 0.5 + 0.2 * np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)   # blob centre: 0.2 off the axis
u0 = np.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / 0.005)

dx = 1.0 / n
nt = int(np.ceil(1.0 / (0.4 * dx / np.abs(V).max())))
dt = 1.0 / nt
u = jr.from_numpy(u0, dev)
Vd = tuple(jr.from_numpy(np.ascontiguousarray(v), dev) for v in V)
weno = jr.WENO5(jr.AMDGPUBackend, method, u0.shape)
for _ in range(nt):
    jr.WENO_advection_(u, Vd, weno, (dx, dx, dx), dt)
got = jr.to_numpy(u)
print(f"{n + 1}^3 vertices, method {method} ({'JS' if method == 1 else 'Z'}), {nt} steps of dt = {dt:.3e}: L1 error after one turn = {np.abs(got - u0).mean():.3e} "
      f"(mean |u0| = {np.abs(u0).mean():.3e}), max = {got.max():.4f} (1 at the start), sum changed by {(got.sum() - u0.sum()) / u0.sum():+.3e} of itself")
