"""The per-step operators a time loop calls around the solves: pureshear_bc! (src/boundaryconditions/pure_shear.jl:1-33), free_surface_bcs!
(src/boundaryconditions/free_surface.jl:1-99), subgrid_characteristic_time! (src/particles/subgrid_diffusion.jl:36-50) and compute_melt_fraction!
(src/rheology/Melting.jl:10-35).  Julia's `f!` is spelled `f_`.  Every function checks the shapes, then forwards to one C-ABI entry point of include/jrx.h
(csrc/stepops.hip); nothing is computed in Python.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .gridops import _args_get, _h, _i64, _p
from .stokes import _require_gpu, rheology_table
from .thermal import thermal_phases

_MELT_KINDS = {None: 0, "none": 0, "caricchi": 1, "MeltingParam_Caricchi": 1}


def _coords(x, n, name, device):
    """a coordinate vector of n entries as a device array (host vectors are uploaded; device tensors are passed as they are)"""
    if isinstance(x, torch.Tensor):
        if x.dim() != 1 or x.shape[0] != n:
            raise ValueError(f"pureshear_bc!: {name} must hold {n} coordinates, got {tuple(x.shape)}")
        return x if x.device == device and x.dtype == torch.float64 else x.to(device=device, dtype=torch.float64)
    host = np.ascontiguousarray(x, dtype=np.float64)
    if host.shape != (n,):
        raise ValueError(f"pureshear_bc!: {name} must hold {n} coordinates, got {host.shape}")
    return torch.tensor(host, dtype=torch.float64, device=device)


def pureshear_bc_(stokes, xci, xvi, εbg, backend=None, *, handle=None):
    """pureshear_bc!(stokes, xci, xvi, εbg, backend) -- pure_shear.jl:1-33: Vx = εbg xv on its interior rows, Vy = -εbg yv (2D) / εbg yv (3D), Vz = -εbg zv;
    the ghosts keep their values.  3D builds the form with yv where the reference's text takes the x vertices for Vy (include/jrx.h).  xci, xvi: the cell-centre
    and vertex vectors of the grid (host or device); a non-uniform Geometry works."""
    V = stokes.V
    _require_gpu(V.Vx)
    ni = tuple(stokes.P.shape)
    nd = len(ni)
    if len(xci) != nd or len(xvi) != nd:
        raise ValueError(f"pureshear_bc!: {nd}D StokesArrays with {len(xci)} centre and {len(xvi)} vertex vectors")
    for d in range(nd):
        if len(xci[d]) != ni[d]:
            raise ValueError(f"pureshear_bc!: xci[{d + 1}] must hold {ni[d]} coordinates, got {len(xci[d])}")
    dev = V.Vx.device
    xv = [_coords(xvi[d], ni[d] + 1, f"xvi[{d + 1}]", dev) for d in range(nd)]
    vel = (V.Vx, V.Vy) if nd == 2 else (V.Vx, V.Vy, V.Vz)
    _h(V.Vx, handle).call(f"jrx_pureshear_bc{nd}d", *_p(*vel), *_p(*xv), C.c_double(float(εbg)), *_i64(*ni))


def _spacing(x, n, name, device):
    """one member of a spacing tuple: (scalar, None) or (0.0, device array of n entries)"""
    if isinstance(x, (int, float)):
        return float(x), None
    t = x if isinstance(x, torch.Tensor) else torch.tensor(np.ascontiguousarray(x, dtype=np.float64))
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"free_surface_bcs!: {name} must hold {n} spacings, got {tuple(t.shape)}")
    return 0.0, t.to(device=device, dtype=torch.float64)


def free_surface_bcs_(stokes, flow_bcs, η, rheology, phase_ratios, dt, *di, handle=None):
    """free_surface_bcs!(stokes, flow_bcs, η, rheology, phase_ratios, dt, _di_vx, _di_vy) in 2D, (..., dt, di) in 3D -- free_surface.jl:1-99: the stress-free
    top velocity, Vy[2:end-1, end] (2D, blended with ν = 1e-2) / Vz[2:end-1, 2:end-1, end] (3D).  Nothing is launched unless flow_bcs.free_surface.  2D: each of
    _di_vx, _di_vy is a pair whose members are numbers or spacing vectors (nx resp. ny entries), read as the kernel reads them: _di_vx[1][i] and _di_vy[2][end];
    one pair `di` serves as both.  3D: di = (dx, dy, dz), numbers.  The 3D form reads τ_o.yy as the reference does (include/jrx.h)."""
    V = stokes.V
    _require_gpu(V.Vx)
    ni = tuple(stokes.P.shape)
    nd = len(ni)
    rh = rheology_table([rheology] if isinstance(rheology, dict) else rheology)
    pc = phase_ratios.center
    if tuple(pc.shape) != (rh.nphase, *ni):
        raise ValueError(f"free_surface_bcs!: phase_ratios.center must be {(rh.nphase, *ni)}, got {tuple(pc.shape)}")
    if tuple(η.shape) != ni:
        raise ValueError(f"free_surface_bcs!: η must be {ni}, got {tuple(η.shape)}")
    cen = _p(stokes.P, stokes.P0, stokes.τ_o.yy, η, pc)
    fs = C.c_int32(bool(flow_bcs.free_surface))
    if nd == 2:
        if len(di) not in (1, 2) or any(len(d) != 2 for d in di):
            raise ValueError("free_surface_bcs!: 2D takes _di_vx, _di_vy (or one di), pairs of spacings")
        sx, ax = _spacing(di[0][0], ni[0], "_di_vx[1]", V.Vx.device)
        sy, ay = _spacing(di[-1][1], ni[1], "_di_vy[2]", V.Vx.device)
        _h(V.Vy, handle).call("jrx_free_surface_bcs2d", *_p(V.Vx, V.Vy), *cen, C.byref(rh), C.c_double(float(dt)), C.c_double(sx), C.c_double(sy), *_p(ax, ay),
                              *_i64(*ni), fs)
    else:
        if len(di) != 1 or len(di[0]) != 3 or not all(isinstance(d, (int, float)) for d in di[0]):
            raise ValueError("free_surface_bcs!: 3D takes di = (dx, dy, dz), three numbers")
        _h(V.Vz, handle).call("jrx_free_surface_bcs3d", *_p(V.Vx, V.Vy, V.Vz), *cen, C.byref(rh), C.c_double(float(dt)), *[C.c_double(float(d)) for d in di[0]],
                              *_i64(*ni), fs)


def subgrid_characteristic_time_(dt0, phase_ratios, rheology, thermal, stokes, di, *, handle=None):
    """subgrid_characteristic_time!(subgrid_arrays, particles, dt₀, phases, rheology, thermal, stokes, di) without the two leading arguments, which its kernel
    never reads (dt₀ is spelled dt0: Python takes no subscript digit in a name) -- subgrid_diffusion.jl:36-50: dt₀[I] = ρCp / (2 K Σ inv(dx_d)²) with ρCp, K of
    the thermal phase table (see thermal_phases) over the centre ratios, P = stokes.P[I], T = thermal.T[I .+ 1] (the cell's own node of the ghosted array).
    di: the uniform spacings."""
    _require_gpu(dt0)
    ni = tuple(stokes.P.shape)
    nd = len(ni)
    table = [rheology] if isinstance(rheology, dict) else list(rheology)
    m = thermal_phases(table, SimpleNamespace(max_lxyz=1.0, Vpdτ=1.0))
    if tuple(dt0.shape) != ni:
        raise ValueError(f"subgrid_characteristic_time!: dt₀ must be size(stokes.P) = {ni}, got {tuple(dt0.shape)}")
    if tuple(thermal.T.shape) != tuple(n + 2 for n in ni):
        raise ValueError(f"subgrid_characteristic_time!: thermal.T must be {tuple(n + 2 for n in ni)}, got {tuple(thermal.T.shape)}")
    if tuple(phase_ratios.center.shape) != (m.nphase, *ni):
        raise ValueError(f"subgrid_characteristic_time!: phase_ratios.center must be {(m.nphase, *ni)}, got {tuple(phase_ratios.center.shape)}")
    if len(di) != nd:
        raise ValueError(f"subgrid_characteristic_time!: {nd} spacings expected, got {len(di)}")
    n3 = (C.c_int64 * 3)(*ni, *([1] * (3 - nd)))
    d3 = (C.c_double * 3)(*[float(d) for d in di], *([1.0] * (3 - nd)))
    _h(dt0, handle).call("jrx_subgrid_characteristic_time", *_p(dt0, phase_ratios.center), C.byref(m), *_p(thermal.T, stokes.P), n3, C.c_int32(nd), d3)


def melting_table(rheology) -> _lib.Melting:
    """jrx_melting from the per-phase table: each phase's `melting` is None (no law) or dict(kind="caricchi", a=800, b=23, c=273.15) -- MeltingParam_Caricchi,
    T in kelvin.  An integer `kind` is passed through (the library refuses what it does not build)."""
    if isinstance(rheology, _lib.Melting):
        return rheology
    phases = [rheology] if isinstance(rheology, dict) else list(rheology)
    if not 1 <= len(phases) <= _lib.MAXPHASE:
        raise ValueError(f"1..{_lib.MAXPHASE} phases supported")
    m = _lib.Melting()
    m.nphase = len(phases)
    for q, ph in enumerate(phases):
        law = ph.get("melting") or {}
        kind = law.get("kind")
        if not isinstance(kind, int):
            if kind not in _MELT_KINDS:
                raise ValueError(f"phase {q + 1}: melting law {kind!r} is not built (MeltingParam_Caricchi is)")
            kind = _MELT_KINDS[kind]
        m.kind[q], m.a[q], m.b[q], m.c[q] = kind, float(law.get("a", 800.0)), float(law.get("b", 23.0)), float(law.get("c", 273.15))
    return m


def compute_melt_fraction_(ϕ, *rest, handle=None):
    """compute_melt_fraction!(ϕ, rheology, args) / compute_melt_fraction!(ϕ, phase_ratios, rheology, args) -- Melting.jl:10-35: the melt fraction of the
    melting laws of `rheology` (see melting_table) at args.T, args.P -- each a number or an array of the extent of ϕ, read at the cell's own index -- for one
    material, or averaged over the centre phase ratios."""
    if len(rest) == 2:
        pr, (rheology, args) = None, rest
    elif len(rest) == 3:
        pr, rheology, args = rest
    else:
        raise TypeError("compute_melt_fraction!(ϕ, [phase_ratios,] rheology, args)")
    _require_gpu(ϕ)
    m = melting_table(rheology)
    ni = tuple(ϕ.shape)
    nd = len(ni)
    if nd not in (2, 3):
        raise ValueError("compute_melt_fraction!: ϕ must be a 2D or 3D array")
    vals = {}
    for k in ("T", "P"):
        v = _args_get(args, k)
        if isinstance(v, torch.Tensor):
            if tuple(v.shape) != ni:
                raise ValueError(f"compute_melt_fraction!: args.{k} must be a number or an array of size(ϕ) = {ni}, got {tuple(v.shape)}")
            vals[k] = (v, 0.0)
        else:
            vals[k] = (None, 0.0 if v is None else float(v))
    pc = None
    if pr is not None:
        pc = pr.center
        if tuple(pc.shape) != (m.nphase, *ni):
            raise ValueError(f"compute_melt_fraction!: phase_ratios.center must be {(m.nphase, *ni)}, got {tuple(pc.shape)}")
    n3 = (C.c_int64 * 3)(*ni, *([1] * (3 - nd)))
    (T, Ts), (P, Ps) = vals["T"], vals["P"]
    _h(ϕ, handle).call("jrx_compute_melt_fraction", *_p(ϕ, pc), C.byref(m), *_p(T), C.c_double(Ts), *_p(P), C.c_double(Ps), n3, C.c_int32(nd))
