"""NumPy restatement of the 2D marker-in-cell particle operators of csrc/particles.hip and of init_particles, operation for operation with the section
"2D marker-in-cell particles" of include/jrx.h: the same products and sums in the same order, each rounded once (NumPy does not contract), so the device results
are compared with np.array_equal.  Per-particle arrays are indexed [i, j, s] (cell, cell, slot); grid fields [i, j]; phase-ratio members [k, i, j].
tests/test_particles2d_restatement.py pins this text; tests/test_gpu_particles2d.py holds the kernels to it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

COUNTS = ("n_active_before", "n_active_after", "n_outside", "n_far", "n_overflow")
MEMBERS = ("center", "vertex", "Vx", "Vy")


def lattice(nxcell):
    """(nsx, nsy), nsx nsy = nxcell: nsx the largest divisor of nxcell not above sqrt(nxcell)"""
    nsx = max(d for d in range(1, int(np.floor(np.sqrt(nxcell))) + 1) if nxcell % d == 0)
    return nsx, nxcell // nsx


def geometry(xvi, ni):
    """x0, y0, dx, dy, _dx, _dy of a uniform grid from its vertex vectors"""
    (nx, ny), (xv, yv) = ni, xvi
    assert len(xv) == nx + 1 and len(yv) == ny + 1
    dx, dy = float(xv[1] - xv[0]), float(yv[1] - yv[0])
    return SimpleNamespace(nx=int(nx), ny=int(ny), x0=float(xv[0]), y0=float(yv[0]), dx=dx, dy=dy, _dx=1.0 / dx, _dy=1.0 / dy)


def init_particles(nxcell, max_xcell, min_xcell, xvi, ni, rng=None):
    """nxcell particles per cell in slots 0 .. nxcell - 1: slot s = a + nsx b sits at (x0 + i dx) + (a + u) (dx / nsx), (y0 + j dy) + (b + v) (dy / nsy) with
    u = v = 0.5, or, with a Generator, u = 0.05 + 0.9 r, r = rng.random((nx, ny, nxcell)) drawn for x first, then for y"""
    g = geometry(xvi, ni)
    nx, ny = g.nx, g.ny
    nsx, nsy = lattice(nxcell)
    s = np.arange(nxcell)
    a, b = (s % nsx).astype(np.float64)[None, None, :], (s // nsx).astype(np.float64)[None, None, :]
    if rng is None:
        u = v = np.full((nx, ny, nxcell), 0.5)
    else:
        u = 0.05 + 0.9 * rng.random((nx, ny, nxcell))
        v = 0.05 + 0.9 * rng.random((nx, ny, nxcell))
    xc = g.x0 + np.arange(nx, dtype=np.float64) * g.dx
    yc = g.y0 + np.arange(ny, dtype=np.float64) * g.dy
    px, py = np.zeros((nx, ny, max_xcell)), np.zeros((nx, ny, max_xcell))
    active = np.zeros((nx, ny, max_xcell), dtype=np.int32)
    px[:, :, :nxcell] = xc[:, None, None] + (a + u) * (g.dx / nsx)
    py[:, :, :nxcell] = yc[None, :, None] + (b + v) * (g.dy / nsy)
    active[:, :, :nxcell] = 1
    return SimpleNamespace(px=px, py=py, active=active, max_xcell=int(max_xcell), min_xcell=int(min_xcell), nxcell=int(nxcell), **vars(g))


def copy(p):
    return SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(p).items()})


# ---------------------------------------------------------------------------------------------- 1. advection
def _finite(v):
    with np.errstate(invalid="ignore"):
        return np.abs(v) <= np.finfo(np.float64).max


def _pair(s, m):
    f = np.floor(s)
    with np.errstate(invalid="ignore"):
        return np.where(f >= 0.0, np.where(f < float(m - 1), f, float(m - 2)), 0.0).astype(np.int64)


def interp(A, ox, oy, _dx, _dy, x, y):
    """(value, ok) of the component A on its node grid of origin (ox, oy) at the points (x, y); ok False where a scaled coordinate is not finite"""
    mx, my = A.shape
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = (x - ox) * _dx, (y - oy) * _dy
    ok = _finite(sx) & _finite(sy)
    sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
    i0, j0 = _pair(sx, mx), _pair(sy, my)
    tx, ty = sx - i0.astype(np.float64), sy - j0.astype(np.float64)
    v00, v10, v01, v11 = A[i0, j0], A[i0 + 1, j0], A[i0, j0 + 1], A[i0 + 1, j0 + 1]
    with np.errstate(invalid="ignore", over="ignore"):
        v = (1.0 - ty) * ((1.0 - tx) * v00 + tx * v10) + ty * ((1.0 - tx) * v01 + tx * v11)
    return v, ok


def advect_rk2(p, Vx, Vy, dt):
    """in place on p.px, p.py"""
    assert Vx.shape == (p.nx + 1, p.ny + 2) and Vy.shape == (p.nx + 2, p.ny + 1)
    oyx, oxy = p.y0 - 0.5 * p.dy, p.x0 - 0.5 * p.dx
    hdt = 0.5 * dt
    x, y = p.px, p.py
    with np.errstate(invalid="ignore", over="ignore"):
        ux, o1 = interp(Vx, p.x0, oyx, p._dx, p._dy, x, y)
        uy, o2 = interp(Vy, oxy, p.y0, p._dx, p._dy, x, y)
        xm, ym = x + hdt * ux, y + hdt * uy
        wx, o3 = interp(Vx, p.x0, oyx, p._dx, p._dy, xm, ym)
        wy, o4 = interp(Vy, oxy, p.y0, p._dx, p._dy, xm, ym)
        xn, yn = x + dt * wx, y + dt * wy
    go = (p.active != 0) & o1 & o2 & o3 & o4
    p.px, p.py = np.where(go, xn, x), np.where(go, yn, y)


# ---------------------------------------------------------------------------------------------- 2. move
def owner(p, x, y):
    """(ic, jc) or None when the particle is outside the grid"""
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = np.floor((x - p.x0) * p._dx), np.floor((y - p.y0) * p._dy)
    if not (fx >= 0.0 and fx < float(p.nx) and fy >= 0.0 and fy < float(p.ny)):
        return None
    return int(fx), int(fy)


def move(src, args=()):
    """(dst, args_dst, counts): out of place"""
    nx, ny, mx = src.nx, src.ny, src.max_xcell
    dst = copy(src)
    dst.px, dst.py, dst.active = np.zeros_like(src.px), np.zeros_like(src.py), np.zeros_like(src.active)
    out = [np.zeros_like(a) for a in args]
    c = dict.fromkeys(COUNTS, 0)
    own = {}
    for i in range(nx):
        for j in range(ny):
            for s in range(mx):
                if src.active[i, j, s]:
                    own[i, j, s] = owner(src, src.px[i, j, s], src.py[i, j, s])
    for j in range(ny):
        for i in range(nx):
            n = 0

            def place(fi, fj, fs):
                nonlocal n
                dst.px[i, j, n], dst.py[i, j, n], dst.active[i, j, n] = src.px[fi, fj, fs], src.py[fi, fj, fs], 1
                for a, o in zip(args, out):
                    o[i, j, n] = a[fi, fj, fs]
                n += 1
            for s in range(mx):
                if not src.active[i, j, s]:
                    continue
                c["n_active_before"] += 1
                o = own[i, j, s]
                if o is None:
                    c["n_outside"] += 1
                elif abs(o[0] - i) > 1 or abs(o[1] - j) > 1:
                    c["n_far"] += 1
                elif o == (i, j):
                    place(i, j, s)
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    fi, fj = i + di, j + dj
                    if (di == 0 and dj == 0) or not (0 <= fi < nx and 0 <= fj < ny):
                        continue
                    for s in range(mx):
                        if src.active[fi, fj, s] and own[fi, fj, s] == (i, j):
                            if n < mx:
                                place(fi, fj, s)
                            else:
                                c["n_overflow"] += 1
            c["n_active_after"] += n
    return dst, out, c


# ---------------------------------------------------------------------------------------------- 3. / 4. interpolation
def grid2particle(F, p):
    assert F.shape == (p.nx + 1, p.ny + 1)
    xv = (p.x0 + np.arange(p.nx, dtype=np.float64) * p.dx)[:, None, None]
    yv = (p.y0 + np.arange(p.ny, dtype=np.float64) * p.dy)[None, :, None]
    f00, f10, f01, f11 = (a[:, :, None] for a in (F[:-1, :-1], F[1:, :-1], F[:-1, 1:], F[1:, 1:]))
    with np.errstate(invalid="ignore", over="ignore"):
        tx, ty = (p.px - xv) * p._dx, (p.py - yv) * p._dy
        v = (1.0 - ty) * ((1.0 - tx) * f00 + tx * f10) + ty * ((1.0 - tx) * f01 + tx * f11)
    return np.where(p.active != 0, v, 0.0)


def _w(x, xn, _dx):
    return 1.0 - np.abs(x - xn) * _dx


def particle2grid(F, pF, p):
    """returns the new F (F itself where no weight arrives)"""
    out = F.copy()
    for i in range(p.nx + 1):
        xv = p.x0 + float(i) * p.dx
        for j in range(p.ny + 1):
            yv = p.y0 + float(j) * p.dy
            num = den = 0.0
            for oi in (-1, 0):
                for oj in (-1, 0):
                    ic, jc = i + oi, j + oj
                    if not (0 <= ic < p.nx and 0 <= jc < p.ny):
                        continue
                    for s in range(p.max_xcell):
                        if not p.active[ic, jc, s]:
                            continue
                        w = _w(p.px[ic, jc, s], xv, p._dx) * _w(p.py[ic, jc, s], yv, p._dy)
                        num = num + w * pF[ic, jc, s]
                        den = den + w
            if not den == 0.0:
                out[i, j] = num / den
    return out


# ---------------------------------------------------------------------------------------------- 5. phase ratios
def member_shape(name, ni, nphase):
    nx, ny = ni
    return (nphase,) + dict(center=(nx, ny), vertex=(nx + 1, ny + 1), Vx=(nx + 1, ny), Vy=(nx, ny + 1))[name]


def phase_ratios(old, pPhases, nphase, p):
    """(members, n_empty): old = dict of the four members as they are before the call (left unchanged where no weight arrives)"""
    nx, ny = p.nx, p.ny
    new = {k: np.array(old[k], dtype=np.float64, copy=True) for k in MEMBERS}
    n_empty = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(nx + 1):
            xv, xc = p.x0 + float(i) * p.dx, p.x0 + (float(i) + 0.5) * p.dx
            for j in range(ny + 1):
                yv, yc = p.y0 + float(j) * p.dy, p.y0 + (float(j) + 0.5) * p.dy
                acc = {k: np.zeros(nphase) for k in MEMBERS}
                W = dict.fromkeys(MEMBERS, 0.0)
                for oi in (-1, 0):
                    for oj in (-1, 0):
                        ic, jc = i + oi, j + oj
                        if not (0 <= ic < nx and 0 <= jc < ny):
                            continue
                        for s in range(p.max_xcell):
                            if not p.active[ic, jc, s]:
                                continue
                            ph = pPhases[ic, jc, s]
                            if not (ph >= 1.0 and ph < float(nphase + 1)):
                                continue
                            k = int(ph) - 1
                            x, y = p.px[ic, jc, s], p.py[ic, jc, s]
                            wxv, wyv, wxc, wyc = _w(x, xv, p._dx), _w(y, yv, p._dy), _w(x, xc, p._dx), _w(y, yc, p._dy)
                            feeds = [("vertex", wxv * wyv)]
                            if oj == 0:
                                feeds.append(("Vx", wxv * wyc))
                            if oi == 0:
                                feeds.append(("Vy", wxc * wyv))
                            if oi == 0 and oj == 0:
                                feeds.append(("center", wxc * wyc))
                            for m, w in feeds:
                                acc[m][k] = acc[m][k] + w
                                W[m] = W[m] + w
                owns = dict(center=i < nx and j < ny, vertex=True, Vx=j < ny, Vy=i < nx)
                for m in MEMBERS:
                    if not owns[m]:
                        continue
                    if W[m] == 0.0:
                        n_empty += 1
                    else:
                        new[m][:, i, j] = acc[m] / W[m]
    return new, n_empty
