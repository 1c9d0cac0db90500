"""NumPy restatement of operators 10 and 11 of the section "2D marker-in-cell particles" of include/jrx.h -- subgrid_diffusion_centroid! and subgrid_diffusion!
with loc = :vertex (Gerya & Yuen's subgrid diffusion of the particle temperature) -- the seven steps of the definition, operation for operation: the same
products and sums in the same order, each rounded once.  Operators 3 and 4 come from tests/_particles2d.py, operators 6 and 7 from tests/_particles2d_stress.py.
Per-particle arrays are indexed [i, j, s]; grid fields [i, j].  The one function that is not a rounded elementary operation is exp: NumPy's here, the device's
there, so d = 0 (exp(-0) = 1 on both sides) is compared bit for bit and d > 0 within a bound.
tests/test_particles2d_subgrid_restatement.py pins this text; tests/test_gpu_particles2d_subgrid.py holds the kernels to it."""
from __future__ import annotations

import numpy as np

from _particles2d import grid2particle, particle2grid
from _particles2d_stress import centroid2particle, particle2centroid

FLOOR = 1e-9          # of dt₀
OUTPUTS = ("pT", "pT0", "pΔT", "ΔT_subgrid")


def own_nodes(ΔT_grid, ext):
    """ΔT_grid on the node box `ext` of the form: itself, or the interior of the array with one ghost layer (thermal.ΔT read at [i + 1, j + 1])"""
    if ΔT_grid.shape == ext:
        return ΔT_grid
    assert ΔT_grid.shape == (ext[0] + 2, ext[1] + 2), (ΔT_grid.shape, ext)
    return ΔT_grid[1:-1, 1:-1]


def factor(dt0, d, dt):
    """f = 1 - exp(((-d) dt) / max(dt₀, 1e-9)) per slot; the comparison is written as the device writes it, so a NaN takes the floor"""
    with np.errstate(invalid="ignore"):
        m = np.where(dt0 > FLOOR, dt0, FLOOR)
    ndt = (-d) * dt
    return 1.0 - np.exp(ndt / m)


def _subgrid(pT, T_grid, ΔT_grid, dt0, p, dt, d, to_particle, to_grid, ext):
    assert T_grid.shape == ext and pT.shape == p.px.shape == dt0.shape
    act = p.active != 0
    with np.errstate(invalid="ignore", over="ignore"):
        pT0 = pT.copy()                                                    # 1
        pTn = to_particle(pT0, T_grid)                                     # 2
        δ = (pTn - pT0) * factor(dt0, d, dt)                               # 3
        pT0 = np.where(act, pT0 + δ, pT0)
        pΔT = np.where(act, δ, 0.0)
        sub = to_grid(np.zeros(ext), pΔT)                                  # 4
        sub = own_nodes(ΔT_grid, ext) - sub                                # 5
        pΔT = to_particle(pΔT, sub)                                        # 6
        pT = np.where(act, pT0 + pΔT, 0.0)                                 # 7
    return dict(zip(OUTPUTS, (pT, pT0, pΔT, sub)))


def subgrid_diffusion_centroid(pT, T_grid, ΔT_grid, dt0, p, dt, d=1.0):
    """operator 10: the new pT, pT0, pΔT and ΔT_subgrid as a dict over OUTPUTS"""
    assert p.nx >= 2 and p.ny >= 2
    return _subgrid(pT, T_grid, ΔT_grid, dt0, p, dt, d, lambda old, F: centroid2particle(old, F, p), lambda F, pF: particle2centroid(F, pF, p), (p.nx, p.ny))


def subgrid_diffusion_vertex(pT, T_grid, ΔT_grid, dt0, p, dt, d=1.0):
    """operator 11: operator 3 has no rule for a non-finite coordinate (it gives NaN) and sets an inactive slot to 0 itself"""
    return _subgrid(pT, T_grid, ΔT_grid, dt0, p, dt, d, lambda old, F: grid2particle(F, p), lambda F, pF: particle2grid(F, pF, p), (p.nx + 1, p.ny + 1))


FORMS = {"center": subgrid_diffusion_centroid, "vertex": subgrid_diffusion_vertex}
