"""Phase ratios from advected phase fields: update_phase_ratios_2D! / update_phase_ratios_3D! (src/phases/PhaseRatios.jl:24-78), the reference's
particle-free route to a PhaseRatios -- "advect both phase arrays and update phase ratios".  Julia's `f!` is spelled `f_`.  Each function forwards to one
C-ABI entry point of include/jrx.h (csrc/phase_ratios.hip); nothing is computed in Python.  Uniform grids only: the reference's compute_dx needs ranges.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .arrays import ptr
from .gridops import _h

_ULPS = 8          # the vertex spacing of a dimension may vary by this many ulp of its largest coordinate (np.linspace and Julia's ranges round per entry)


def _coords(xci, xvi, ni, fn):
    """host copies of the coordinate vectors of an (xci, xvi) pair or of a Geometry (xvi may then be None), checked against the grid ni"""
    if xvi is None:
        if not (hasattr(xci, "xci") and hasattr(xci, "xvi")):
            raise ValueError(f"{fn}: pass xci and xvi, or a Geometry")
        xci, xvi = xci.xci, xci.xvi
    elif hasattr(xci, "xci") or hasattr(xvi, "xvi"):
        raise ValueError(f"{fn}: pass either a Geometry or the two tuples xci, xvi")
    nd = len(ni)
    if len(xci) != nd or len(xvi) != nd:
        raise ValueError(f"{fn}: the phase arrays are {nd}D, xci has {len(xci)} and xvi {len(xvi)} coordinate vectors")
    xc = [np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64) for x in xci]
    xv = [np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64) for x in xvi]
    dx = []
    for d in range(nd):
        if xc[d].shape != (ni[d],) or xv[d].shape != (ni[d] + 1,):
            raise ValueError(f"{fn}: dimension {d + 1} has {ni[d]} cells, xci[{d}] has {xc[d].size} entries and xvi[{d}] {xv[d].size} (expected {ni[d]} and {ni[d] + 1})")
        steps = np.diff(xv[d])
        if not np.all(np.abs(steps - steps[0]) <= _ULPS * np.spacing(np.abs(xv[d]).max())):
            raise ValueError(f"{fn}: the vertices of dimension {d + 1} are not uniform (spacing {steps.min()} .. {steps.max()}); only uniform grids are built "
                             "(the reference's compute_dx needs ranges)")
        dx.append(float(xv[d][1] - xv[d][0]))
    return xc, xv, dx


def _update(nd, phase_ratios, phase_arrays, xci, xvi, handle):
    fn = f"update_phase_ratios_{nd}D!"
    phase_arrays = tuple(phase_arrays)
    if not phase_arrays:
        raise ValueError(f"{fn}: no phase arrays")
    for k, p in enumerate(phase_arrays):
        if p.dim() != nd:
            raise ValueError(f"{fn}: phase array {k + 1} is {p.dim()}D; this is the {nd}D method (use update_phase_ratios_{p.dim()}D_ for {p.dim()}D arrays)")
    ni = tuple(phase_arrays[0].shape)
    if any(tuple(p.shape) != ni for p in phase_arrays):
        raise ValueError(f"{fn}: the phase arrays differ in size: {[tuple(p.shape) for p in phase_arrays]}")
    N = len(phase_arrays)
    if phase_ratios.nphases != N:
        raise ValueError(f"{fn}: {N} phase arrays for a PhaseRatios of {phase_ratios.nphases} phases")
    stag = {"center": (0, 0, 0), "vertex": (1, 1, 1), "Vx": (1, 0, 0), "Vy": (0, 1, 0), "Vz": (0, 0, 1), "yz": (0, 1, 1), "xz": (1, 0, 1), "xy": (1, 1, 0)}
    names = ("center", "vertex", "Vx", "Vy") if nd == 2 else ("center", "vertex", "Vx", "Vy", "Vz", "yz", "xz", "xy")
    outs = []
    for name in names:
        m = getattr(phase_ratios, name, None)
        want = (N,) + tuple(n + s for n, s in zip(ni, stag[name]))
        if m is None or tuple(m.shape) != want:
            raise ValueError(f"{fn}: phase_ratios.{name} is {None if m is None else tuple(m.shape)}, the phase arrays {ni} need {want}")
        outs.append(m)
    xc, xv, dx = _coords(xci, xvi, ni, fn)
    h = _h(phase_arrays[0], handle)
    dev = phase_arrays[0].device
    up = lambda a: torch.from_numpy(a).to(dev)
    xc_d, xv_d = [up(a) for a in xc], [up(a) for a in xv]
    torch.cuda.current_stream(dev).synchronize()
    pa = (C.c_void_p * N)(*(ptr(p) for p in phase_arrays))
    vec = lambda ts: (C.c_void_p * nd)(*(t.data_ptr() for t in ts))
    h.call(f"jrx_update_phase_ratios{nd}d", *(C.c_void_p(ptr(m)) for m in outs), pa, C.c_int32(N), *(C.c_int64(n) for n in ni), vec(xc_d), vec(xv_d),
           (C.c_double * nd)(*dx))


def update_phase_ratios_2D_(phase_ratios, phase_arrays, xci, xvi=None, *, handle=None):
    """update_phase_ratios_2D!(phase_ratios, phase_arrays, xci, xvi) -- PhaseRatios.jl:24-35: center, vertex, Vx, Vy of phase_ratios from the N cell-centred
    (nx, ny) phase arrays.  xci, xvi: the tuples a Geometry carries (NumPy arrays or tensors; uploaded here), or a Geometry in place of both."""
    _update(2, phase_ratios, phase_arrays, xci, xvi, handle)


def update_phase_ratios_3D_(phase_ratios, phase_arrays, xci, xvi=None, *, handle=None):
    """update_phase_ratios_3D!(phase_ratios, phase_arrays, xci, xvi) -- PhaseRatios.jl:61-78: center, vertex, Vx, Vy, Vz, xy, yz, xz of phase_ratios from the N
    cell-centred (nx, ny, nz) phase arrays.  xci, xvi as in 2D."""
    _update(3, phase_ratios, phase_arrays, xci, xvi, handle)
