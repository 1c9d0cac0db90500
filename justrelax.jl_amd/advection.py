"""WENO-5 advection of a 2D or 3D vertex field: the WENO5 struct and WENO_advection! (src/types/weno.jl, src/types/constructors/weno.jl:1-55,
src/advection/weno5.jl:195-230; the AMDGPU methods src/ext/AMDGPU/2D.jl:84-88,470-472).  Julia's `f!` is spelled `f_`.  WENO_advection_ forwards to
one C-ABI entry point of include/jrx.h (csrc/advection.hip); nothing is computed in Python.  Uniform spacing only: the reference's inv.(di) fails on
per-vertex spacing vectors.  The 3D form (three velocities, 3D arrays) is the scheme written out one dimension up (jrx_weno5_advection3d): the
reference's own 3D forwards feed a 3D array into 2D indexing.
"""
from __future__ import annotations

import ctypes as C
from numbers import Real

import torch

from .arrays import fzeros, ptr
from .backend import device_of
from .gridops import _h


class WENO5:
    """WENO5(backend, method, ni) -- JustRelax.WENO5 (src/types/weno.jl) as built by constructors/weno.jl:1-55: the constants of :7-24, ni, the work
    arrays ut, fL, fR, fB, fT (@zeros(ni...)) and method (1 = JS, 2 = Z; Val(1) / Val(2) in the reference).  After a call of the fused form (the default)
    fL holds the stage-1 field and fL..fT do not hold fluxes (include/jrx.h).  A 3-entry ni also allocates fD, fU, the upwind / downwind fluxes along z
    of the 3D form (this project's names: the reference's struct has no such fields)."""
    d0L, d1L, d2L = 1 / 10, 3 / 5, 3 / 10           # upwind constants
    d0R, d1R, d2R = 3 / 10, 3 / 5, 1 / 10           # downwind constants
    c1, c2 = 13 / 12, 1 / 4                          # betas
    sc1, sc2, sc3, sc4, sc5 = 1 / 3, 7 / 6, 11 / 6, 1 / 6, 5 / 6     # stencil weights
    ϵ = 1.0e-6

    def __init__(self, backend, method, ni):
        m = getattr(method, "value", method)
        if m not in (1, 2):
            raise ValueError(f"WENO5: method must be 1 (JS) or 2 (Z), got {method!r}")     # weno5.jl:19-21,40-42: error("Unknown method ...")
        self.method = int(m)
        self.ni = tuple(int(n) for n in ni)
        dev = device_of(backend)
        self.ut, self.fL, self.fR, self.fB, self.fT = (fzeros(self.ni, dev) for _ in range(5))
        if len(self.ni) == 3:
            self.fD, self.fU = fzeros(self.ni, dev), fzeros(self.ni, dev)


def WENO_advection_(u, Vxi, weno: WENO5, di, dt, *, handle=None):
    """WENO_advection!(u, (vx, vy), weno, di, dt) -- weno5.jl:195-230.  Loop box and clamping from size(u); every array is read with its own extents
    (weno may be built for ni .+ 1 and the velocities may be larger than u: Benchmark2D_WENO5.jl:77,182).  With three velocities and u, the velocities and
    weno.ut all 3D: the 3D form, WENO_advection!(u, (vx, vy, vz), weno, (dx, dy, dz), dt)."""
    if len(Vxi) == 3:
        return _weno_advection3d(u, Vxi, weno, di, dt, handle)
    vx, vy = Vxi
    for name, a in (("u", u), ("vx", vx), ("vy", vy), ("weno.ut", weno.ut)):
        if a.dim() != 2:
            raise ValueError(f"WENO_advection!: {name} is {a.dim()}D; the WENO-5 kernels are 2D only (the reference's 3D methods feed a 3D array into 2D indexing)")
    if len(di) != 2 or not all(isinstance(d, Real) or (isinstance(d, torch.Tensor) and d.dim() == 0) for d in di):
        raise ValueError("WENO_advection!: di must be the two uniform spacings (dx, dy); per-vertex spacing vectors are not supported (inv.(di) fails on them in the reference)")
    shapes = {tuple(a.shape) for a in (weno.ut, weno.fL, weno.fR, weno.fB, weno.fT)}
    if len(shapes) != 1:
        raise ValueError("WENO_advection!: weno.ut, fL, fR, fB, fT must have one common size")
    ud = (C.c_int64 * 2)(*u.shape)
    vxd = (C.c_int64 * 2)(*vx.shape)
    vyd = (C.c_int64 * 2)(*vy.shape)
    wd = (C.c_int64 * 2)(*weno.ut.shape)
    p = [C.c_void_p(ptr(t)) for t in (u, vx, vy, weno.ut, weno.fL, weno.fR, weno.fB, weno.fT)]
    _h(u, handle).call("jrx_weno5_advection2d", p[0], ud, p[1], vxd, p[2], vyd, *p[3:], wd, C.c_double(float(di[0])), C.c_double(float(di[1])),
                       C.c_double(float(dt)), C.c_int32(int(weno.method)))


def _weno_advection3d(u, Vxi, weno, di, dt, handle):
    vx, vy, vz = Vxi
    for name, a in (("u", u), ("vx", vx), ("vy", vy), ("vz", vz), ("weno.ut", weno.ut)):
        if a.dim() != 3:
            raise ValueError(f"WENO_advection!: {name} is {a.dim()}D; with three velocities u, the velocities and weno.ut must all be 3D")
    if len(di) != 3 or not all(isinstance(d, Real) or (isinstance(d, torch.Tensor) and d.dim() == 0) for d in di):
        raise ValueError("WENO_advection!: di must be the three uniform spacings (dx, dy, dz); per-vertex spacing vectors are not supported (inv.(di) fails on them in the reference)")
    work = (weno.ut, weno.fL, weno.fR, weno.fB, weno.fT, weno.fD, weno.fU)
    if len({tuple(a.shape) for a in work}) != 1:
        raise ValueError("WENO_advection!: weno.ut, fL, fR, fB, fT, fD, fU must have one common size")
    d3 = lambda t: (C.c_int64 * 3)(*t.shape)
    p = [C.c_void_p(ptr(t)) for t in (u, vx, vy, vz, *work)]
    _h(u, handle).call("jrx_weno5_advection3d", p[0], d3(u), p[1], d3(vx), p[2], d3(vy), p[3], d3(vz), *p[4:], d3(weno.ut),
                       *(C.c_double(float(d)) for d in di), C.c_double(float(dt)), C.c_int32(int(weno.method)))
