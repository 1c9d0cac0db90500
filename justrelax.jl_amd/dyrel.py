"""Operator API of the DYREL solver (self-tuned dynamic relaxation inside Powell-Hestenes pressure iterations) in 2D and 3D -- src/DYREL/ of the reference.

DYREL (types.jl:24-59, constructors.jl:13-154), DYREL! (constructors.jl:178-190), solve_DYREL! (solver.jl:36-294), update_α_β! and update_dτV_α_β!
(Gershgorin.jl:171-310), spelled `f_`.  Every function forwards to C-ABI entry points of include/jrx.h (csrc/dyrel2d.hip, csrc/dyrel3d.hip); nothing is computed
in Python.  The 3D stress kernel and eigenvalue bound have no reference text; include/jrx.h states their form.  Built: one block, uniform spacing, the table rheology, velocity boundary conditions; a RockRatio, a non-uniform Geometry, a communicator, args.ΔT /
args.melt_fraction and an is_pl other than 0 or 1 are refused by the library with status JRX_ERR_ARG and a text naming the cause.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .arrays import fzeros, ptr
from .backend import device_of
from .grid import Geometry
from .stokes import _args_T, _ng, _require_gpu, rheology_table, vep_fields2d, vep_fields3d
from .variational import rock_ratio2d, rock_ratio3d, vs_rheology_table

# reference field name -> member of jrx_dyrel2d_fields
_MEMBERS = dict(γ_eff="gamma_eff", ηb="etab", P_num="P_num", Dx="Dx", Dy="Dy", λmaxVx="lmaxVx", λmaxVy="lmaxVy", dVxdτ="dVxdtau", dVydτ="dVydtau",
                dτVx="dtauVx", dτVy="dtauVy", dVx="dVx", dVy="dVy", βVx="betaVx", βVy="betaVy", cVx="cVx", cVy="cVy", αVx="alphaVx", αVy="alphaVy",
                Rx0="Rx0", Ry0="Ry0")
# the same for jrx_dyrel3d_fields: the 2D members and their z twins
_MEMBERS3 = dict(_MEMBERS, Dz="Dz", λmaxVz="lmaxVz", dVzdτ="dVzdtau", dτVz="dtauVz", dVz="dVz", βVz="betaVz", cVz="cVz", αVz="alphaVz", Rz0="Rz0")


class DYREL(SimpleNamespace):
    """DYREL(backend, ni; ϵ, ϵ_vel, CFL, c_fact) / DYREL(backend, nx, ny[, nz]; ...) -- zero arrays (constructors.jl:13-111) -- or
    DYREL(backend, stokes, rheology, phase_ratios, di, dt; ϵ, ϵ_vel, CFL, c_fact, γfact) -- allocated and initialised as DYREL! does (constructors.jl:113-154).
    In 2D the z members (Dz, λmaxVz, ...) are the (1, 1) placeholders the reference allocates; in 3D they are (nx, ny, nz-1) (constructors.jl:61-111)."""

    def __init__(self, backend_tag, *args, ϵ=1.0e-6, ϵ_vel=1.0e-6, CFL=0.99, c_fact=0.5, γfact=20.0, handle=None):
        super().__init__()
        stokes = None
        if len(args) == 1:
            ni = tuple(args[0])
        elif len(args) in (2, 3) and all(isinstance(n, (int, np.integer)) for n in args):
            ni = tuple(args)
        elif len(args) == 5:
            stokes, rheology, phase_ratios, di, dt = args
            ni = tuple(stokes._ni)
        else:
            raise TypeError("DYREL(backend, ni) or DYREL(backend, stokes, rheology, phase_ratios, di, dt)")
        if len(ni) not in (2, 3):
            raise TypeError("DYREL: ni must have two or three entries")
        ni = tuple(int(n) for n in ni)
        dev = device_of(backend_tag)
        self._ni = ni
        less = lambda d: tuple(n - (1 if q == d else 0) for q, n in enumerate(ni))
        for k in ("γ_eff", "ηb", "P_num"):
            setattr(self, k, fzeros(ni, dev))
        for k in ("D", "λmaxV", "dV{}dτ", "dτV", "dV", "βV", "cV", "αV", "R{}0"):
            name = (lambda c: k.format(c) if "{}" in k else k + c)
            setattr(self, name("x"), fzeros(less(0), dev))
            setattr(self, name("y"), fzeros(less(1), dev))
            setattr(self, name("z"), fzeros((1, 1) if len(ni) == 2 else less(2), dev))
        self.CFL, self.ϵ, self.ϵ_vel, self.c_fact = float(CFL), float(ϵ), float(ϵ_vel), float(c_fact)
        if stokes is not None:
            DYREL_(self, stokes, rheology, phase_ratios, di, dt, CFL=CFL, γfact=γfact, handle=handle)

    # ASCII aliases of the scalars
    eps = property(lambda s: s.ϵ)
    eps_vel = property(lambda s: s.ϵ_vel)


def dyrel_fields2d(dyrel, stokes, args=None) -> _lib.DYREL2DFields:
    s = stokes
    vals = {c: getattr(dyrel, k) for k, c in _MEMBERS.items()}
    vals.update(txx_v=s.τ.xx_v, tyy_v=s.τ.yy_v, toxx_v=s.τ_o.xx_v, toyy_v=s.τ_o.yy_v, lambda_v=s.λv, dPpsi=s.ΔPψ)
    vals["lambda"] = s.λ
    if args is not None:
        get = (lambda k: args.get(k)) if isinstance(args, dict) else (lambda k: getattr(args, k, None))
        vals.update(dT=get("ΔT"), melt_fraction=get("melt_fraction"))
    d = _lib.DYREL2DFields()
    for n in _lib.DYREL_NAMES:
        setattr(d, n, ptr(vals.get(n)))
    d._keep = vals
    return d


def dyrel_params2d(dyrel, *, viscosity_cutoff=(-float("inf"), float("inf")), viscosity_relaxation=1.0e-2, λ_relaxation_DR=1, λ_relaxation_PH=1, iterMax=50.0e3,
                   total_iterMax=50.0e3, nout=100, rel_drop=1.0e-2, b_width=(4, 4, 0), verbose_PH=True, verbose_DR=True, linear_viscosity=False, γfact=20.0,
                   CFL=None, **_) -> _lib.DYREL2DParams:
    """the keywords of _solve_DYREL! with their defaults (solver.jl:55-66) and the scalars of the DYREL struct"""
    q = _lib.DYREL2DParams()
    q.cutoff_lo, q.cutoff_hi = float(viscosity_cutoff[0]), float(viscosity_cutoff[1])
    q.viscosity_relaxation, q.lambda_relaxation_DR, q.lambda_relaxation_PH = float(viscosity_relaxation), float(λ_relaxation_DR), float(λ_relaxation_PH)
    q.iterMax, q.total_iterMax, q.nout, q.rel_drop = int(iterMax), int(total_iterMax), int(nout), float(rel_drop)
    for k in range(3):
        q.b_width[k] = int(b_width[k])
    q.verbose_PH, q.verbose_DR, q.linear_viscosity = int(bool(verbose_PH)), int(bool(verbose_DR)), int(bool(linear_viscosity))
    q.CFL = float(dyrel.CFL if CFL is None else CFL)
    q.eps, q.eps_vel, q.c_fact, q.gamma_fact = float(dyrel.ϵ), float(dyrel.ϵ_vel), float(dyrel.c_fact), float(γfact)
    return q


def grid_params2d(stokes, grid_or_di, dt, flow_bcs=None, args=None) -> _lib.VEP2DParams:
    """what the DYREL entry points read of jrx_vep2d_params: extents, inv(dx), inv(dy) (Gershgorin.jl:47-48), dt, the face masks, the layout of args.T and,
    for a non-uniform Geometry, its spacing arrays (which the library then refuses)"""
    ni = stokes._ni
    p = _lib.VEP2DParams()
    p.nx, p.ny = ni
    p.nxg, p.nyg = [(_ng(d) or ni[d]) for d in range(2)]
    if isinstance(grid_or_di, Geometry):
        if getattr(grid_or_di, "nonuniform", False):
            from .stokes import _center_inv, _set_spacing2d
            p._dx, p._dy = _center_inv(grid_or_di)
            _set_spacing2d(p, grid_or_di, stokes)
        else:
            p._dx, p._dy = grid_or_di._di["center"]
    else:
        di = grid_or_di["center"] if isinstance(grid_or_di, dict) else grid_or_di
        p._dx, p._dy = 1.0 / float(di[0]), 1.0 / float(di[1])
    p.dt = float(dt)
    if flow_bcs is not None:
        p.free_slip, p.no_slip, p.periodic = (_lib.bcmask(flow_bcs.free_slip), _lib.bcmask(flow_bcs.no_slip), _lib.bcmask(flow_bcs.periodic))
    T = _args_T(args)
    if T is not None and tuple(T.shape) != tuple(ni):
        if tuple(T.shape) != tuple(n + 2 for n in ni):
            raise ValueError(f"args.T must be ni {tuple(ni)} (thermal.Tc) or ni .+ 2 (thermal.T), got {tuple(T.shape)}")
        p.T_ghosted = 1
    return p


def _zero_rhog(stokes):
    z = fzeros(stokes._ni, stokes.P.device)
    return (z, z)


def _table(rheology):
    return vs_rheology_table(rheology)      # a phase given with a `cap` (DruckerPragerCap) is marked is_pl = 2, which the library refuses


def edge_λv(stokes):
    """the three λv arrays of a 3D solve, on the yz / xz / xy edges (the reference's StokesArrays holds one vertex array, which no 3D stress kernel of it
    indexes per family); allocated on first use and kept on `stokes`"""
    lv = stokes.__dict__.get("_λv_edges")
    if lv is None:
        nx, ny, nz = stokes._ni
        dev = stokes.P.device
        lv = SimpleNamespace(yz=fzeros((nx, ny + 1, nz + 1), dev), xz=fzeros((nx + 1, ny, nz + 1), dev), xy=fzeros((nx + 1, ny + 1, nz), dev))
        stokes.__dict__["_λv_edges"] = lv
    return lv


def dyrel_fields3d(dyrel, stokes=None, args=None) -> _lib.DYREL3DFields:
    vals = {c: getattr(dyrel, k) for k, c in _MEMBERS3.items()}
    if stokes is not None:
        lv = edge_λv(stokes)
        vals.update(lambda_yz=lv.yz, lambda_xz=lv.xz, lambda_xy=lv.xy, dPpsi=stokes.ΔPψ)
        vals["lambda"] = stokes.λ
    if args is not None:
        get = (lambda k: args.get(k)) if isinstance(args, dict) else (lambda k: getattr(args, k, None))
        vals.update(dT=get("ΔT"), melt_fraction=get("melt_fraction"))
    d = _lib.DYREL3DFields()
    for n in _lib.DYREL3_NAMES:
        setattr(d, n, ptr(vals.get(n)))
    d._keep = vals
    return d


def grid_params3d(stokes_or_ni, grid_or_di, dt, flow_bcs=None, args=None) -> _lib.VEP3DParams:
    """what the 3D DYREL entry points read of jrx_vep3d_params: extents, the inverse spacings, dt, the face masks, the layout of args.T.  A non-uniform Geometry
    has no scalar spacings: it is handed over as NaNs, a free_surface boundary condition as displacement_bcs = -1; the library refuses both by name"""
    ni = tuple(getattr(stokes_or_ni, "_ni", stokes_or_ni))
    p = _lib.VEP3DParams()
    p.nx, p.ny, p.nz = ni
    p.nxg, p.nyg, p.nzg = [(_ng(d) or ni[d]) for d in range(3)]
    if isinstance(grid_or_di, Geometry):
        p._dx, p._dy, p._dz = (float("nan"),) * 3 if getattr(grid_or_di, "nonuniform", False) else grid_or_di._di["center"]
    else:
        di = grid_or_di["center"] if isinstance(grid_or_di, dict) else grid_or_di
        p._dx, p._dy, p._dz = (1.0 / float(x) for x in di)
    p.dt = float(dt)
    if flow_bcs is not None:
        p.free_slip, p.no_slip, p.periodic = (_lib.bcmask(flow_bcs.free_slip), _lib.bcmask(flow_bcs.no_slip), _lib.bcmask(flow_bcs.periodic))
        if getattr(flow_bcs, "free_surface", False):
            p.displacement_bcs = -1
    T = _args_T(args)
    if T is not None and tuple(T.shape) != ni:
        if tuple(T.shape) != tuple(n + 2 for n in ni):
            raise ValueError(f"args.T must be ni {ni} (thermal.Tc) or ni .+ 2 (thermal.T), got {tuple(T.shape)}")
        p.T_ghosted = 1
    return p


def _zero_rhog3(stokes):
    z = fzeros(stokes._ni, stokes.P.device)
    return (z, z, z)


def _init3d(dyrel, stokes, rheology, phase_ratios, ϕ, di, dt, CFL, γfact, h):
    f = vep_fields3d(stokes, _zero_rhog3(stokes), phase_ratios)
    d = dyrel_fields3d(dyrel, stokes)
    p = grid_params3d(stokes, di, dt)
    q = dyrel_params2d(dyrel, CFL=CFL, γfact=γfact)
    r = rock_ratio3d(ϕ) if ϕ is not None else None
    rh = _table(rheology)
    torch.cuda.current_stream(stokes.P.device).synchronize()
    h.call("jrx_dyrel3d_init", C.byref(f), C.byref(d), C.byref(r) if r is not None else None, C.byref(rh), C.byref(p), C.byref(q))


def DYREL_(dyrel, stokes, rheology, phase_ratios, *rest, CFL=0.99, γfact=20.0, handle=None):
    """DYREL!(dyrel, stokes, rheology, phase_ratios, [ϕ,] di, dt; CFL, γfact) -- constructors.jl:178-203; on a 3D grid with the 3D eigenvalue bound"""
    _require_gpu(stokes)
    ϕ = None
    if len(rest) == 3:
        ϕ, di, dt = rest
    else:
        di, dt = rest
    h = handle or _lib.default_handle(stokes.P.device.index)
    if len(stokes._ni) == 3:
        return _init3d(dyrel, stokes, rheology, phase_ratios, ϕ, di, dt, CFL, γfact, h)
    f = vep_fields2d(stokes, _zero_rhog(stokes), phase_ratios)
    d = dyrel_fields2d(dyrel, stokes)
    p = grid_params2d(stokes, di, dt)
    q = dyrel_params2d(dyrel, CFL=CFL, γfact=γfact)
    r = rock_ratio2d(ϕ) if ϕ is not None else None
    rh = _table(rheology)
    torch.cuda.current_stream(stokes.P.device).synchronize()
    h.call("jrx_dyrel2d_init", C.byref(f), C.byref(d), C.byref(r) if r is not None else None, C.byref(rh), C.byref(p), C.byref(q))


def solve_DYREL_(stokes, ρg, dyrel, flow_bcs, phase_ratios, rheology, args, grid_or_di, dt, igg=None, *, kwargs=None, ϕ=None, handle=None):
    """solve_DYREL!(stokes, ρg, dyrel, flow_bcs, phase_ratios, rheology, args, grid, dt, igg; kwargs...) -- solver.jl:36-294.  `kwargs` holds the reference's
    keywords.  Returns the reference's named tuple (err_evo_it, err_evo_V, err_evo_P, err_evo_tot) with the counts iter and itPH beside it."""
    _require_gpu(stokes)
    kw = dict(kwargs or {})
    h = handle or _lib.default_handle(stokes.P.device.index)
    three = len(stokes._ni) == 3
    if three:
        f = vep_fields3d(stokes, ρg, phase_ratios, args)
        d = dyrel_fields3d(dyrel, stokes, args)
        p = grid_params3d(stokes, grid_or_di, dt, flow_bcs, args)
        r = rock_ratio3d(ϕ) if ϕ is not None else None
    else:
        f = vep_fields2d(stokes, ρg, phase_ratios, args, allow_ghosted_T=True)
        d = dyrel_fields2d(dyrel, stokes, args)
        p = grid_params2d(stokes, grid_or_di, dt, flow_bcs, args)
        r = rock_ratio2d(ϕ) if ϕ is not None else None
    q = dyrel_params2d(dyrel, **kw)
    rh = _table(rheology)
    cap = int(q.total_iterMax // q.nout + q.iterMax // q.nout + 4) if q.total_iterMax < 10**7 else 10**5
    cap = min(cap, 10**6)
    bufs = [np.zeros(cap) for _ in range(4)]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    res = _lib.DYREL2DResult(0, 0, 0, cap, dp(bufs[0]), dp(bufs[1]), dp(bufs[2]), dp(bufs[3]), 0.0)
    torch.cuda.current_stream(stokes.P.device).synchronize()
    h.call("jrx_dyrel3d_solve" if three else "jrx_dyrel2d_solve", C.byref(f), C.byref(d), C.byref(r) if r is not None else None, C.byref(rh), C.byref(p), C.byref(q), C.byref(res))
    k = res.nchecks
    return SimpleNamespace(err_evo_it=bufs[0][:k].copy(), err_evo_V=bufs[1][:k].copy(), err_evo_P=bufs[2][:k].copy(), err_evo_tot=bufs[3][:k].copy(),
                           iter=res.iter, itPH=res.itPH, time=res.time_s)


def _update(dyrel, CFL, from_lambda_max, handle):
    t = dyrel.Dx
    _require_gpu(t)
    h = handle or _lib.default_handle(t.device.index)
    if len(dyrel._ni) == 3:
        d = dyrel_fields3d(dyrel)
        p = grid_params3d(dyrel._ni, (1.0, 1.0, 1.0), 0.0)          # the spacings are not read
        torch.cuda.current_stream(t.device).synchronize()
        h.call("jrx_dyrel3d_update_dtauV_alpha_beta", C.byref(d), C.byref(p), C.c_double(float(CFL)), C.c_int32(from_lambda_max))
        return
    st = SimpleNamespace(τ=SimpleNamespace(xx_v=None, yy_v=None), τ_o=SimpleNamespace(xx_v=None, yy_v=None), λ=None, λv=None, ΔPψ=None)
    d = dyrel_fields2d(dyrel, st)
    p = _lib.VEP2DParams()
    p.nx, p.ny = dyrel._ni
    p.nxg, p.nyg = dyrel._ni
    torch.cuda.current_stream(t.device).synchronize()
    h.call("jrx_dyrel2d_update_dtauV_alpha_beta", C.byref(d), C.byref(p), C.c_double(float(CFL)), C.c_int32(from_lambda_max))


def update_α_β_(dyrel, *, handle=None):
    """update_α_β!(dyrel) -- Gershgorin.jl:171-198,250-257"""
    _update(dyrel, dyrel.CFL, 0, handle)


def update_dτV_α_β_(dyrel, *, handle=None):
    """update_dτV_α_β!(dyrel) -- Gershgorin.jl:216-247,260-269"""
    _update(dyrel, dyrel.CFL, 1, handle)
