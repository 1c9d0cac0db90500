"""Grid-based stress rotation and advection: rotate_stress!(stokes, grid, dt; method, advection), the grid counterpart of the reference's particle chain
rotate_stress!(pτ, stokes, particles, dt) + stress2grid! (src/stress_rotation/stress_rotation_particles.jl:205-299) and of its exported grid stub
rotate_stress!(V, τ, _di, dt) (src/stress_rotation/stress_rotation_grid.jl; include/jrx.h lists the stub's defects, which are not followed).  Julia's `f!` is
spelled `f_`.  The function forwards to one C-ABI entry point of include/jrx.h (csrc/stress_rotation.hip); nothing is computed in Python.

A visco-elastic time loop calls it between two solves, in place of the plain copy every driver's epilogue leaves in stokes.τ_o:

    solve_(stokes, ...); dt = compute_dt_(stokes, di); rotate_stress_(stokes, grid, dt); ... ; solve_(stokes, ...)

dt must come from compute_dt (the upwind step has no CFL check of its own).  compute_dt bounds the Courant number of each axis by 0.9 and the unsplit upwind
step is stable while their sum stays <= 1, so a flow whose components peak at the same nodes needs compute_dt / ndims (examples/stress_rotation2d.py).  Uniform grids only; no halo exchange inside the call: a decomposed run exchanges
τ_o itself.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .arrays import ptr
from .stokes import _as_grid, _center_inv, _require_gpu

METHODS = {"matrix": 0, "jaumann": 1}          # JRX_ROTATE_MATRIX, JRX_ROTATE_JAUMANN
ADVECTIONS = {"none": 0, "upwind": 1}          # JRX_ADVECT_NONE, JRX_ADVECT_UPWIND
_MEMBERS = {2: ("xx", "yy", "xy_c", "xy"), 3: ("xx", "yy", "zz", "yz_c", "xz_c", "xy_c", "yz", "xz", "xy")}


def rotate_stress_(stokes, grid_or_di, dt, *particle_form, method="matrix", advection="upwind", handle=None):
    """rotate_stress!(pτxx, pτyy, pτxy, pω, stokes, particles, dt; method = :matrix) when the first argument is a particle field (a tensor): the particle form,
    particles.py -- stokes.τ and stokes.ω.xy to the particles and the rotation there; advection_ / move_particles_ then carry the stress, stress2grid_ puts it back.
    Otherwise the grid form:

    rotate_stress!(stokes, grid_or_di, dt; method = :matrix, advection = :upwind): stokes.τ_o = Rot(stokes.τ, stokes.ω dt) - dt Adv(stokes.τ, stokes.V), every
    member at its own node (include/jrx.h, jrx_rotate_stress2d / 3d).  Reads stokes.τ, stokes.ω (as the drivers' epilogue or compute_vorticity_ leave it) and
    stokes.V; writes stokes.τ_o.  grid_or_di: a uniform Geometry or the legacy tuple of spacings.  method: "matrix" (rotation matrix; exact for any angle) or
    "jaumann" (first order in dt ω).  advection: "upwind" or "none" (a caller may then advect τ_o with WENO_advection_).  The 2D vertex normals xx_v, yy_v are
    carried along only when both tensors have them allocated."""
    if isinstance(stokes, torch.Tensor):
        from .particles import _rotate_stress_particles_form
        if len(particle_form) != 4:
            raise TypeError(f"rotate_stress!: the particle form takes (pτxx, pτyy, pτxy, pω, stokes, particles, dt), got {3 + len(particle_form)} arguments")
        if advection != "upwind":
            raise ValueError("rotate_stress!: the particle form has no advection keyword (advection_ and move_particles_ carry the stress)")
        return _rotate_stress_particles_form(stokes, grid_or_di, dt, *particle_form, method=method, handle=handle)
    if particle_form:
        raise TypeError(f"rotate_stress!: the grid form takes (stokes, grid_or_di, dt), got {3 + len(particle_form)} arguments")
    _require_gpu(stokes)
    name = lambda s: s.lstrip(":") if isinstance(s, str) else s
    if name(method) not in METHODS:
        raise ValueError(f"rotate_stress!: unknown method {method!r} (one of {sorted(METHODS)})")
    if name(advection) not in ADVECTIONS:
        raise ValueError(f"rotate_stress!: unknown advection {advection!r} (one of {sorted(ADVECTIONS)})")
    if getattr(grid_or_di, "nonuniform", False):
        raise NotImplementedError("rotate_stress!: only uniform grids are built (DESIGN.md section 7)")
    ni = stokes._ni
    nd = len(ni)
    _di = _center_inv(_as_grid(stokes, grid_or_di))
    τ, τ_o, V = stokes.τ, stokes.τ_o, stokes.V
    members = list(_MEMBERS[nd])
    if nd == 2:
        both = all(k in t.__dict__ for t in (τ, τ_o) for k in ("xx_v", "yy_v"))
        members += ["xx_v", "yy_v"] if both else [None, None]
    vec = lambda ts: (C.c_void_p * len(ts))(*(ptr(t) for t in ts))
    tin = vec([getattr(τ, k) if k else None for k in members])
    tout = vec([getattr(τ_o, k) if k else None for k in members])
    vel = vec([V.Vx, V.Vy] + ([V.Vz] if nd == 3 else []))
    h = handle or _lib.default_handle(stokes.P.device.index)
    torch.cuda.current_stream(stokes.P.device).synchronize()
    tail = [*(C.c_int64(n) for n in ni), (C.c_double * nd)(*(float(d) for d in _di)), C.c_double(float(dt)), C.c_int32(METHODS[name(method)]),
            C.c_int32(ADVECTIONS[name(advection)])]
    if nd == 2:
        h.call("jrx_rotate_stress2d", tout, tin, C.c_void_p(ptr(stokes.ω.xy)), vel, *tail)
    else:
        h.call("jrx_rotate_stress3d", tout, tin, vec([stokes.ω.yz, stokes.ω.xz, stokes.ω.xy]), vel, *tail)
