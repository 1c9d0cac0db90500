"""A moving free surface on grids, 2D and 3D: Topography(backend, nx) / Topography(backend, (nx, ny)), compute_rock_fraction!(ϕ, topo, grid),
advect_topography!(topo, V, grid, dt) and update_phases_given_topography!(phases, topo, grid, air_phase).  Julia's `f!` is spelled `f_`.  They are the grid
counterparts of what the reference's free-surface miniapps (miniapps/DYREL2D/volcano/Caldera2D.jl:175-195,439-449, the Subduction2D_VS* set) take from JustPIC's
marker chain -- fill_chain_from_vertices!, semilagrangian_advection_markerchain!, compute_rock_fraction!(ϕ, chain, xvi, di) -- and of
update_phases_given_markerchain! (src/phases/topography_correction.jl), which works on particles; none of that text is in the reference tree or restated:
include/jrx.h holds the definitions.  Each function forwards to one C-ABI entry point (csrc/topography.hip); nothing is computed in Python.  The functions
dispatch on the grid's dimension: a 2D grid takes the polyline h(x), a 3D grid the surface h(x, y) with z the vertical.  Uniform Geometry, one block.

A time loop with a free surface (examples/free_surface_relaxation2d.py, examples/free_surface_relaxation3d.py):

    compute_rock_fraction_(ϕ, topo, grid); update_phases_given_topography_(phases, topo, grid, air_phase); update_phase_ratios_2D_ / _3D_(...); compute_ρg_(...);
    compute_viscosity_(...; air_phase); solve_VariationalStokes_(...); dt = compute_dt_(...); WENO_advection_ of the phase fields; advect_topography_(topo, V, grid, dt)

advect_topography_ is stable at any dt, but the loop is explicit in the surface: give compute_dt_ a dt_diff of a fraction of the relaxation time 4 π η / (ρ g λ)
of the longest wavelength, which the Courant step outgrows as the surface flattens (include/jrx.h; the examples).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .arrays import fzeros, ptr
from .backend import device_of
from .gridops import _h


class Topography:
    """Topography(backend, nx): the surface height at the nx + 1 vertex abscissae of a 2D grid, in the grid's coordinates (`h`), and the input of the last
    advection (`h_old`); two device vectors of nx + 1 doubles, zero-initialised.  Topography(backend, (nx, ny)): the surface h(x, y) over a 3D grid, two
    (nx + 1, ny + 1) arrays.  An integer or a 1-tuple is the 2D object."""

    def __init__(self, backend_tag, nx):
        ni = tuple(nx) if isinstance(nx, (tuple, list)) else (nx,)
        if len(ni) not in (1, 2) or not all(isinstance(n, (int, np.integer)) and not isinstance(n, bool) and n >= 1 for n in ni):
            raise TypeError(f"Topography: nx, or (nx, ny), must be positive integers, got {nx!r}")
        dev = device_of(backend_tag)
        self._ni, self._device = tuple(int(n) for n in ni), dev
        shape = tuple(n + 1 for n in self._ni)
        self.h = fzeros(shape, dev)
        self.h_old = fzeros(shape, dev)

    def fill_(self, h):
        """fill!(topo, h): h from a host or device array of the heights, nx + 1 of them or (nx + 1, ny + 1) (h_old is left as it is)"""
        src = h if isinstance(h, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64))
        if tuple(src.shape) != tuple(self.h.shape):
            raise ValueError(f"Topography.fill!: {tuple(src.shape)} heights for {tuple(self.h.shape)} vertex positions")
        self.h.copy_(src.to(torch.float64))
        return self


def _uniform(grid, fn):
    """(ni, the origin along the vertical, the inverse spacings) of a uniform 2D or 3D Geometry"""
    if getattr(grid, "nonuniform", False):
        raise NotImplementedError(f"{fn}: only uniform grids are built (DESIGN.md section 7)")
    if not (hasattr(grid, "origin") and hasattr(grid, "_di") and hasattr(grid, "ni")):
        raise ValueError(f"{fn}: grid must be a Geometry (the surface heights are in its coordinates)")
    nd = len(grid.ni)
    if nd not in (2, 3):
        raise NotImplementedError(f"{fn}: built for 2D and 3D grids")
    return tuple(grid.ni), float(grid.origin[nd - 1]), tuple(float(d) for d in grid._di["center"])


def _same_dim(fn, ni, what, nd):
    if nd != len(ni):
        raise NotImplementedError(f"{fn}: {what} is {nd}D, the grid {len(ni)}D (a 2D grid takes h(x) and 2D arrays, a 3D grid h(x, y) and 3D arrays)")


def _check_topo(topo, ni, fn):
    _same_dim(fn, ni, "the Topography", topo.h.dim() + 1)
    want = tuple(n + 1 for n in ni[:-1])
    for k in ("h", "h_old"):
        if tuple(getattr(topo, k).shape) != want:
            raise ValueError(f"{fn}: topo.{k} is {tuple(getattr(topo, k).shape)}, the grid has {want} vertex positions")


def compute_rock_fraction_(ϕ, topo, grid, *, handle=None):
    """compute_rock_fraction!(ϕ::RockRatio, topo, grid): every member of ϕ (four in 2D, eight in 3D) = the fraction of its control volume below the surface --
    in 2D the polyline through (xvi[1][i], topo.h[i]), in 3D the surface through the heights topo.h[i, j], linear on the four triangles corner-corner-centre of
    every cell (include/jrx.h, jrx_compute_rock_fraction2d / jrx_compute_rock_fraction3d).  One launch; nothing else in ϕ is read."""
    fn = "compute_rock_fraction!"
    ni, z0, _di = _uniform(grid, fn)
    _same_dim(fn, ni, "the RockRatio", ϕ.center.dim())
    if len(ni) == 2:
        nx, ny = ni
        want = dict(center=(nx, ny), vertex=(nx + 1, ny + 1), Vx=(nx + 1, ny), Vy=(nx, ny + 1))
    else:
        nx, ny, nz = ni
        want = dict(center=ni, vertex=(nx + 1, ny + 1, nz + 1), Vx=(nx + 1, ny, nz), Vy=(nx, ny + 1, nz), Vz=(nx, ny, nz + 1),
                    yz=(nx, ny + 1, nz + 1), xz=(nx + 1, ny, nz + 1), xy=(nx + 1, ny + 1, nz))
    for k, s in want.items():
        if tuple(getattr(ϕ, k).shape) != s:
            raise ValueError(f"{fn}: ϕ.{k} is {tuple(getattr(ϕ, k).shape)}, the grid {ni} needs {s}")
    _check_topo(topo, ni, fn)
    h = _h(ϕ.center, handle)
    h.call(f"jrx_compute_rock_fraction{len(ni)}d", *(C.c_void_p(ptr(getattr(ϕ, k))) for k in want), C.c_void_p(ptr(topo.h)), *(C.c_int64(n) for n in ni),
           C.c_double(z0), C.c_double(_di[-1]))


def advect_topography_(topo, V, grid, dt, *, handle=None):
    """advect_topography!(topo, V, grid, dt): topo.h_old = topo.h, then topo.h by one first-order semi-Lagrangian step with the velocities V = stokes.V (or the
    tuple (Vx, Vy[, Vz]), ghost layers included) interpolated to the surface (include/jrx.h, jrx_advect_topography2d / jrx_advect_topography3d).  dt from
    compute_dt, undivided."""
    fn = "advect_topography!"
    ni, z0, _di = _uniform(grid, fn)
    nd = len(ni)
    Vs = tuple(getattr(V, k) for k in ("Vx", "Vy", "Vz") if hasattr(V, k)) if hasattr(V, "Vx") else tuple(V)
    if len(Vs) != nd or any(v.dim() != nd for v in Vs):
        raise NotImplementedError(f"{fn}: V has {len(Vs)} components of {[v.dim() for v in Vs]} dimensions, the grid is {nd}D")
    want = tuple(tuple(n + (1 if e == d else 2) for e, n in enumerate(ni)) for d in range(nd))
    if tuple(tuple(v.shape) for v in Vs) != want:
        raise ValueError(f"{fn}: V is {', '.join(str(tuple(v.shape)) for v in Vs)}; the grid {ni} needs {', '.join(map(str, want))}")
    _check_topo(topo, ni, fn)
    h = _h(topo.h, handle)
    h.call(f"jrx_advect_topography{nd}d", C.c_void_p(ptr(topo.h)), C.c_void_p(ptr(topo.h_old)), *(C.c_void_p(ptr(v)) for v in Vs), *(C.c_int64(n) for n in ni),
           C.c_double(z0), *(C.c_double(d) for d in _di), C.c_double(float(dt)))


def update_phases_given_topography_(phases, topo, grid, air_phase, *, handle=None):
    """update_phases_given_topography!(phases, topo, grid, air_phase): the N cell-centred phase fields of update_phase_ratios_2D_ / _3D_ put back on the right
    side of the surface, in place: air below it becomes the nearest rock below, rock above it becomes air; a cell whose air field already equals 1 - its rock
    fraction keeps its bits (include/jrx.h, jrx_update_phases_topography2d / jrx_update_phases_topography3d).  air_phase is 1-based."""
    fn = "update_phases_given_topography!"
    phases = tuple(phases)
    ni, z0, _di = _uniform(grid, fn)
    if not phases:
        raise ValueError(f"{fn}: no phase fields")
    _same_dim(fn, ni, "a phase field", phases[0].dim())
    for k, p in enumerate(phases):
        if tuple(p.shape) != ni:
            raise ValueError(f"{fn}: phase field {k + 1} is {tuple(p.shape)}, the grid has {ni} cells")
    _check_topo(topo, ni, fn)
    h = _h(phases[0], handle)
    pa = (C.c_void_p * len(phases))(*(ptr(p) for p in phases))
    h.call(f"jrx_update_phases_topography{len(ni)}d", pa, C.c_int32(len(phases)), C.c_void_p(ptr(topo.h)), *(C.c_int64(n) for n in ni), C.c_double(z0),
           C.c_double(_di[-1]), C.c_int32(int(air_phase)))
