"""Operator API of the variational Stokes solvers (free surface through a rock-ratio mask) -- src/variational_stokes/ of the reference.

update_rock_ratio!(ϕ, phase_ratios, air_phase) (mask.jl:63-105) and solve_VariationalStokes! (Stokes2D.jl:9-332, Stokes3D.jl:14-238), spelled `f_`.  Every
function forwards to C-ABI entry points of include/jrx.h (csrc/stokes2d_vs.hip, csrc/stokes3d_vs.hip); nothing is computed in Python.  Built: 2D (strain-rate
form) and 3D, one block, uniform spacing; everything else is refused by the library with status JRX_ERR_ARG and a text naming it.  The 3D momentum kernel is
the masked 2D one written one dimension up (the reference's own 3D text cannot run; include/jrx.h states the form), and free-surface stabilisation is not
built in 3D (a flow_bcs with free_surface=True raises ValueError).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .arrays import ptr
from .stokes import _Hist, _args_T, _as_grid, _ghosted_T_flag, _require_gpu, rheology_table, vep_fields2d, vep_fields3d, vep_params2d, vep_params3d


def rock_ratio2d(ϕ) -> _lib.RockRatio2D:
    r = _lib.RockRatio2D()
    vals = dict(center=ϕ.center, vertex=ϕ.vertex, Vx=ϕ.Vx, Vy=ϕ.Vy)
    for k, v in vals.items():
        setattr(r, k, ptr(v))
    r._keep = vals
    return r


def rock_ratio3d(ϕ) -> _lib.RockRatio3D:
    r = _lib.RockRatio3D()
    vals = dict(center=ϕ.center, vertex=ϕ.vertex, Vx=ϕ.Vx, Vy=ϕ.Vy, Vz=ϕ.Vz, yz=ϕ.yz, xz=ϕ.xz, xy=ϕ.xy)
    for k, v in vals.items():
        setattr(r, k, ptr(v))
    r._keep = vals
    return r


def update_rock_ratio_(ϕ, phase_ratios, air_phase, *, handle=None):
    """update_rock_ratio!(ϕ, phase_ratios, air_phase) -- mask.jl:63-157, 2D and 3D: ϕ = 1 - ratio[air_phase], zeroed when <= 1e-5, 1 when air_phase is
    outside 1..nphases; `center` and `vertex` are not clamped, the velocity (and, in 3D, shear) members are clamped to [0, 1]."""
    _require_gpu(ϕ.center)
    h = handle or _lib.default_handle(ϕ.center.device.index)
    torch.cuda.current_stream(ϕ.center.device).synchronize()
    members = [("center", 0), ("vertex", 0), ("Vx", 1), ("Vy", 1)]
    if ϕ.center.dim() == 3:
        members += [("Vz", 1), ("xy", 1), ("yz", 1), ("xz", 1)]
    for name, clamp in members:
        dst, src = getattr(ϕ, name), getattr(phase_ratios, name)
        if tuple(src.shape[1:]) != tuple(dst.shape):
            raise ValueError(f"phase_ratios.{name} has extents {tuple(src.shape[1:])}, ϕ.{name} {tuple(dst.shape)}")
        h.call("jrx_update_rock_ratio", C.c_void_p(ptr(dst)), C.c_void_p(ptr(src)), C.c_int32(int(src.shape[0])), C.c_int32(int(air_phase)),
               C.c_int64(dst.numel()), C.c_int32(clamp))


def vs_rheology_table(rheology) -> _lib.Rheology:
    """the rheology table of the variational driver: a phase given with a `cap` (DruckerPragerCap) is marked so that the library refuses it"""
    rh = rheology_table(rheology)
    if not isinstance(rheology, _lib.Rheology):
        for q, ph in enumerate(rheology):
            if ph.get("cap") is not None:
                rh.is_pl[q] = 2
    return rh


def _solve_vs3d(stokes, pt_stokes, grid, flow_bcs, ρg, phase_ratios, ϕ, rheology, args, dt, kw, h):
    """_solve_VS! in 3D -- variational_stokes/Stokes3D.jl:14-238; keywords air_phase, iterMax, nout, b_width, verbose, viscosity_relaxation, viscosity_cutoff"""
    known = ("air_phase", "iterMax", "nout", "b_width", "verbose", "viscosity_relaxation", "viscosity_cutoff")
    kw = {k: v for k, v in kw.items() if k in known}          # kwargs... of the reference swallows the rest (iterMin, λ_relaxation, free_surface: unused in 3D)
    air_phase = int(kw.pop("air_phase", 0))
    if getattr(flow_bcs, "free_surface", False):
        raise ValueError("solve_VariationalStokes! 3D: free-surface stabilisation (flow_bcs.free_surface) is not built in 3D")
    if getattr(grid, "nonuniform", False):
        # jrx_vep3d_params carries scalar spacings only; a non-uniform Geometry has none: the library refuses the NaNs it gets instead (JRX_ERR_ARG, named)
        from types import SimpleNamespace
        p = vep_params3d(stokes, pt_stokes, SimpleNamespace(_di=dict(center=(float("nan"),) * 3)), flow_bcs, dt, **kw)
    else:
        p = vep_params3d(stokes, pt_stokes, grid, flow_bcs, dt, **kw)
    f = vep_fields3d(stokes, ρg, phase_ratios, args)
    p.T_ghosted = _ghosted_T_flag(stokes, _args_T(args))
    rh = vs_rheology_table(rheology)
    r = rock_ratio3d(ϕ)
    hist = _Hist(int(p.iterMax // p.nout + 2))
    torch.cuda.current_stream(stokes.P.device).synchronize()
    h.call("jrx_stokes3d_vs_solve", C.byref(f), C.byref(r), C.byref(rh), C.byref(p), C.c_int32(air_phase), C.byref(hist.c))
    return hist.result(3)


def solve_VariationalStokes_(stokes, pt_stokes, grid_or_di, flow_bcs, ρg, phase_ratios, ϕ, rheology, args, dt, igg=None, *, kwargs=None, handle=None):
    """solve_VariationalStokes!(stokes, pt_stokes, grid, flow_bcs, ρg, phase_ratios, ϕ, rheology, args, dt, igg; kwargs...) -- variational_stokes/Stokes2D.jl:24-332,
    Stokes3D.jl:14-238.  `kwargs` holds the reference's keywords: in 2D air_phase, iterMax, iterMin, nout, viscosity_cutoff, viscosity_relaxation, λ_relaxation,
    free_surface, verbose, strain_increment; in 3D air_phase, iterMax, nout, b_width, verbose, viscosity_relaxation, viscosity_cutoff.  Returns the same namespace as
    solve_ (iter, err_evo1, err_evo2, norm_Rx, norm_Ry, [norm_Rz,] norm_∇V)."""
    _require_gpu(stokes)
    if len(stokes._ni) not in (2, 3):
        raise NotImplementedError("solve_VariationalStokes! is built for 2D (variational_stokes/Stokes2D.jl) and 3D (Stokes3D.jl) grids")
    kw = dict(kwargs or {})
    h = handle or _lib.default_handle(stokes.P.device.index)
    grid = _as_grid(stokes, grid_or_di)
    if len(stokes._ni) == 3:
        return _solve_vs3d(stokes, pt_stokes, grid, flow_bcs, ρg, phase_ratios, ϕ, rheology, args, dt, kw, h)
    air_phase = int(kw.pop("air_phase", 0))
    p = vep_params2d(stokes, pt_stokes, grid, flow_bcs, dt, **kw)
    f = vep_fields2d(stokes, ρg, phase_ratios, args, allow_ghosted_T=True, strain_increment=bool(p.strain_increment))
    T = _args_T(args)
    if T is not None and tuple(T.shape) != tuple(stokes._ni):
        if tuple(T.shape) != tuple(n + 2 for n in stokes._ni):
            raise ValueError(f"args.T must be ni {tuple(stokes._ni)} (thermal.Tc) or ni .+ 2 (thermal.T), got {tuple(T.shape)}")
        p.T_ghosted = 1
    rh = vs_rheology_table(rheology)
    r = rock_ratio2d(ϕ)
    hist = _Hist(int(p.iterMax // p.nout + 2))
    torch.cuda.current_stream(stokes.P.device).synchronize()
    h.call("jrx_stokes2d_vs_solve", C.byref(f), C.byref(r), C.byref(rh), C.byref(p), C.c_int32(air_phase), C.byref(hist.c))
    return hist.result(2)
