"""A moving free surface in 2D on grids: Topography(backend, nx), compute_rock_fraction!(ϕ, topo, grid), advect_topography!(topo, V, grid, dt) and
update_phases_given_topography!(phases, topo, grid, air_phase).  Julia's `f!` is spelled `f_`.  They are the grid counterparts of what the reference's
free-surface miniapps (miniapps/DYREL2D/volcano/Caldera2D.jl:175-195,439-449, the Subduction2D_VS* set) take from JustPIC's marker chain --
fill_chain_from_vertices!, semilagrangian_advection_markerchain!, compute_rock_fraction!(ϕ, chain, xvi, di) -- and of update_phases_given_markerchain!
(src/phases/topography_correction.jl), which works on particles; none of that text is in the reference tree or restated: include/jrx.h holds the definitions.
Each function forwards to one C-ABI entry point (csrc/topography.hip); nothing is computed in Python.  2D, uniform Geometry, one block.

A time loop with a free surface (examples/free_surface_relaxation2d.py):

    compute_rock_fraction_(ϕ, topo, grid); update_phases_given_topography_(phases, topo, grid, air_phase); update_phase_ratios_2D_(...); compute_ρg_(...);
    compute_viscosity_(...; air_phase); solve_VariationalStokes_(...); dt = compute_dt_(...); WENO_advection_ of the phase fields; advect_topography_(topo, V, grid, dt)

advect_topography_ is stable at any dt, but the loop is explicit in the surface: give compute_dt_ a dt_diff of a fraction of the relaxation time 4 π η / (ρ g λ)
of the longest wavelength, which the Courant step outgrows as the surface flattens (include/jrx.h; the example).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .arrays import fzeros, ptr
from .backend import device_of
from .gridops import _h


class Topography:
    """Topography(backend, nx): the surface height at the nx + 1 vertex abscissae, in the grid's coordinates (`h`), and the input of the last advection
    (`h_old`); two device vectors of nx + 1 doubles, zero-initialised."""

    def __init__(self, backend_tag, nx):
        if isinstance(nx, (tuple, list)) and len(nx) == 1:
            nx = nx[0]
        if not isinstance(nx, (int, np.integer)) or isinstance(nx, bool) or nx < 1:
            raise TypeError(f"Topography: nx must be a positive integer, got {nx!r}")
        dev = device_of(backend_tag)
        self._ni, self._device = (int(nx),), dev
        self.h = fzeros((int(nx) + 1,), dev)
        self.h_old = fzeros((int(nx) + 1,), dev)

    def fill_(self, h):
        """fill!(topo, h): h from a host or device vector of nx + 1 heights (h_old is left as it is)"""
        src = h if isinstance(h, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64))
        if tuple(src.shape) != tuple(self.h.shape):
            raise ValueError(f"Topography.fill!: {tuple(src.shape)} heights for {tuple(self.h.shape)} vertex abscissae")
        self.h.copy_(src.to(torch.float64))
        return self


def _uniform2d(grid, fn):
    if getattr(grid, "nonuniform", False):
        raise NotImplementedError(f"{fn}: only uniform grids are built (DESIGN.md section 7)")
    if not (hasattr(grid, "origin") and hasattr(grid, "_di") and hasattr(grid, "ni")):
        raise ValueError(f"{fn}: grid must be a Geometry (the surface heights are in its coordinates)")
    if len(grid.ni) != 2:
        raise NotImplementedError(f"{fn}: built for 2D grids (surfaces h(x, y) are out of scope, DESIGN.md section 7)")
    _di = grid._di["center"]
    return tuple(grid.ni), float(grid.origin[1]), float(_di[0]), float(_di[1])


def _check_topo(topo, nx, fn):
    for k in ("h", "h_old"):
        if tuple(getattr(topo, k).shape) != (nx + 1,):
            raise ValueError(f"{fn}: topo.{k} has {tuple(getattr(topo, k).shape)} entries, the grid has {nx + 1} vertex abscissae")


def compute_rock_fraction_(ϕ, topo, grid, *, handle=None):
    """compute_rock_fraction!(ϕ::RockRatio, topo, grid): center, vertex, Vx, Vy of ϕ = the fraction of each member's control volume below the polyline through
    (xvi[1][i], topo.h[i]) (include/jrx.h, jrx_compute_rock_fraction2d).  One launch; nothing else in ϕ is read."""
    fn = "compute_rock_fraction!"
    if ϕ.center.dim() != 2:
        raise NotImplementedError(f"{fn}: built for a 2D RockRatio (surfaces h(x, y) are out of scope, DESIGN.md section 7)")
    (nx, ny), y0, _, _dy = _uniform2d(grid, fn)
    want = dict(center=(nx, ny), vertex=(nx + 1, ny + 1), Vx=(nx + 1, ny), Vy=(nx, ny + 1))
    for k, s in want.items():
        if tuple(getattr(ϕ, k).shape) != s:
            raise ValueError(f"{fn}: ϕ.{k} is {tuple(getattr(ϕ, k).shape)}, the grid {(nx, ny)} needs {s}")
    _check_topo(topo, nx, fn)
    h = _h(ϕ.center, handle)
    h.call("jrx_compute_rock_fraction2d", *(C.c_void_p(ptr(getattr(ϕ, k))) for k in want), C.c_void_p(ptr(topo.h)), C.c_int64(nx), C.c_int64(ny),
           C.c_double(y0), C.c_double(_dy))


def advect_topography_(topo, V, grid, dt, *, handle=None):
    """advect_topography!(topo, V, grid, dt): topo.h_old = topo.h, then topo.h by one first-order semi-Lagrangian step with the velocities V = stokes.V (or the
    pair (Vx, Vy), ghost layers included) interpolated to the surface (include/jrx.h, jrx_advect_topography2d).  dt from compute_dt, undivided."""
    fn = "advect_topography!"
    (nx, ny), y0, _dx, _dy = _uniform2d(grid, fn)
    Vx, Vy = (V.Vx, V.Vy) if hasattr(V, "Vx") else tuple(V)
    if tuple(Vx.shape) != (nx + 1, ny + 2) or tuple(Vy.shape) != (nx + 2, ny + 1):
        raise ValueError(f"{fn}: V is {tuple(Vx.shape)}, {tuple(Vy.shape)}; the grid {(nx, ny)} needs {(nx + 1, ny + 2)}, {(nx + 2, ny + 1)}")
    _check_topo(topo, nx, fn)
    h = _h(topo.h, handle)
    h.call("jrx_advect_topography2d", C.c_void_p(ptr(topo.h)), C.c_void_p(ptr(topo.h_old)), C.c_void_p(ptr(Vx)), C.c_void_p(ptr(Vy)), C.c_int64(nx), C.c_int64(ny),
           C.c_double(y0), C.c_double(_dx), C.c_double(_dy), C.c_double(float(dt)))


def update_phases_given_topography_(phases, topo, grid, air_phase, *, handle=None):
    """update_phases_given_topography!(phases, topo, grid, air_phase): the N cell-centred (nx, ny) phase fields of update_phase_ratios_2D_ put back on the right
    side of the surface, in place: air below it becomes the nearest rock below, rock above it becomes air; a cell whose air field already equals 1 - its rock
    fraction keeps its bits (include/jrx.h, jrx_update_phases_topography2d).  air_phase is 1-based."""
    fn = "update_phases_given_topography!"
    phases = tuple(phases)
    if phases and phases[0].dim() != 2:
        raise NotImplementedError(f"{fn}: built for 2D phase fields (surfaces h(x, y) are out of scope, DESIGN.md section 7)")
    (nx, ny), y0, _, _dy = _uniform2d(grid, fn)
    if not phases:
        raise ValueError(f"{fn}: no phase fields")
    for k, p in enumerate(phases):
        if tuple(p.shape) != (nx, ny):
            raise ValueError(f"{fn}: phase field {k + 1} is {tuple(p.shape)}, the grid has {(nx, ny)} cells")
    _check_topo(topo, nx, fn)
    h = _h(phases[0], handle)
    pa = (C.c_void_p * len(phases))(*(ptr(p) for p in phases))
    h.call("jrx_update_phases_topography2d", pa, C.c_int32(len(phases)), C.c_void_p(ptr(topo.h)), C.c_int64(nx), C.c_int64(ny), C.c_double(y0), C.c_double(_dy),
           C.c_int32(int(air_phase)))
