"""NumPy restatement of the 3D marker-in-cell particle operators of csrc/particles3d.hip and of init_particles(..., *xi_vel), operation for operation with the
section "3D marker-in-cell particles" of include/jrx.h: the same products and sums in the same order, each rounded once (NumPy does not contract), so the device
results are compared with np.array_equal.  Per-particle arrays are indexed [i, j, k, s] (cell, cell, cell, slot); grid fields [i, j, k]; phase-ratio members
[q, i, j, k].  Every operator is vectorised over the cells (or nodes) and sequential where the definition fixes an order: over the source cells and the slots.
tests/test_particles3d_restatement.py pins this text; tests/test_gpu_particles3d.py holds the kernels to it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

COUNTS = ("n_active_before", "n_active_after", "n_outside", "n_far", "n_overflow")
MEMBERS = ("center", "vertex", "Vx", "Vy", "Vz", "yz", "xz", "xy")
STAGGER = dict(center=(0, 0, 0), vertex=(1, 1, 1), Vx=(1, 0, 0), Vy=(0, 1, 0), Vz=(0, 0, 1), yz=(0, 1, 1), xz=(1, 0, 1), xy=(1, 1, 0))
# the 26 neighbour offsets (di, dj, dk) in the order of the move: dk outermost, di innermost
NEIGHBOURS = tuple((di, dj, dk) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1) if (di, dj, dk) != (0, 0, 0))


def lattice(nxcell):
    """(nsx, nsy, nsz), nsx nsy nsz = nxcell: nsx the largest divisor of nxcell with nsx^3 <= nxcell, nsy the largest divisor of the rest r = nxcell / nsx with
    nsy^2 <= r, nsz = r / nsy; on integers"""
    nsx = max(d for d in range(1, nxcell + 1) if nxcell % d == 0 and d * d * d <= nxcell)
    r = nxcell // nsx
    nsy = max(d for d in range(1, r + 1) if r % d == 0 and d * d <= r)
    return nsx, nsy, r // nsy


def geometry(xvi):
    """extents, origin, spacings and their inverses of a uniform grid from its three vertex vectors"""
    n = [len(x) - 1 for x in xvi]
    d = [float(x[1] - x[0]) for x in xvi]
    return SimpleNamespace(nx=n[0], ny=n[1], nz=n[2], x0=float(xvi[0][0]), y0=float(xvi[1][0]), z0=float(xvi[2][0]), dx=d[0], dy=d[1], dz=d[2],
                           _dx=1.0 / d[0], _dy=1.0 / d[1], _dz=1.0 / d[2])


def init_particles(nxcell, max_xcell, min_xcell, *xi_vel, rng=None):
    """the reference's call shape: the vertex vector of axis d is xi_vel[d][d].  nxcell particles per cell in slots 0 .. nxcell - 1: slot s = a + nsx (b + nsy c)
    sits at (x0 + i dx) + (a + u) (dx / nsx) and likewise with (b, v, nsy), (c, w, nsz); u = v = w = 0.5, or, with a Generator, 0.05 + 0.9 r with
    r = rng.random((nx, ny, nz, nxcell)) drawn for x, then y, then z"""
    assert len(xi_vel) == 3
    g = geometry([np.asarray(xi_vel[d][d], dtype=np.float64) for d in range(3)])
    ni = (g.nx, g.ny, g.nz)
    ns = lattice(nxcell)
    s = np.arange(nxcell)
    abc = [(s % ns[0]), (s // ns[0]) % ns[1], s // (ns[0] * ns[1])]
    shape = ni + (nxcell,)
    uvw = [np.full(shape, 0.5) if rng is None else 0.05 + 0.9 * rng.random(shape) for _ in range(3)]
    origin, spacing = (g.x0, g.y0, g.z0), (g.dx, g.dy, g.dz)
    coords = []
    for d in range(3):
        cell = origin[d] + np.arange(ni[d], dtype=np.float64) * spacing[d]
        cell = cell.reshape([-1 if q == d else 1 for q in range(4)])
        p = np.zeros(ni + (max_xcell,))
        p[..., :nxcell] = cell + (abc[d].astype(np.float64)[None, None, None, :] + uvw[d]) * (spacing[d] / ns[d])
        coords.append(p)
    active = np.zeros(ni + (max_xcell,), dtype=np.int32)
    active[..., :nxcell] = 1
    return SimpleNamespace(px=coords[0], py=coords[1], pz=coords[2], active=active, max_xcell=int(max_xcell), min_xcell=int(min_xcell), nxcell=int(nxcell),
                           **vars(g))


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


def _bilin(tx, ty, v00, v10, v01, v11):
    return (1.0 - ty) * ((1.0 - tx) * v00 + tx * v10) + ty * ((1.0 - tx) * v01 + tx * v11)


def _trilin(tx, ty, tz, v):
    """v[a][b][c]: the node at offsets (a, b, c)"""
    b0 = _bilin(tx, ty, v[0][0][0], v[1][0][0], v[0][1][0], v[1][1][0])
    b1 = _bilin(tx, ty, v[0][0][1], v[1][0][1], v[0][1][1], v[1][1][1])
    return (1.0 - tz) * b0 + tz * b1


def interp(A, origin, inv, x, y, z):
    """(value, ok) of the component A on its node grid at the points (x, y, z); ok False where a scaled coordinate is not finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = [(c - o) * i for c, o, i in zip((x, y, z), origin, inv)]
    ok = _finite(s[0]) & _finite(s[1]) & _finite(s[2])
    s = [np.where(ok, q, 0.0) for q in s]
    i0 = [_pair(q, m) for q, m in zip(s, A.shape)]
    t = [q - n.astype(np.float64) for q, n in zip(s, i0)]
    v = [[[A[i0[0] + a, i0[1] + b, i0[2] + c] for c in (0, 1)] for b in (0, 1)] for a in (0, 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        return _trilin(t[0], t[1], t[2], v), ok


def velocity(p, V, x, y, z):
    Vx, Vy, Vz = V
    hx, hy, hz = p.x0 - 0.5 * p.dx, p.y0 - 0.5 * p.dy, p.z0 - 0.5 * p.dz
    inv = (p._dx, p._dy, p._dz)
    ux, o1 = interp(Vx, (p.x0, hy, hz), inv, x, y, z)
    uy, o2 = interp(Vy, (hx, p.y0, hz), inv, x, y, z)
    uz, o3 = interp(Vz, (hx, hy, p.z0), inv, x, y, z)
    return ux, uy, uz, o1 & o2 & o3


def advect_rk2(p, V, dt):
    """in place on p.px, p.py, p.pz"""
    nx, ny, nz = p.nx, p.ny, p.nz
    assert V[0].shape == (nx + 1, ny + 2, nz + 2) and V[1].shape == (nx + 2, ny + 1, nz + 2) and V[2].shape == (nx + 2, ny + 2, nz + 1)
    hdt = 0.5 * dt
    x, y, z = p.px, p.py, p.pz
    with np.errstate(invalid="ignore", over="ignore"):
        ux, uy, uz, o1 = velocity(p, V, x, y, z)
        xm, ym, zm = x + hdt * ux, y + hdt * uy, z + hdt * uz
        wx, wy, wz, o2 = velocity(p, V, xm, ym, zm)
        xn, yn, zn = x + dt * wx, y + dt * wy, z + dt * wz
    go = (p.active != 0) & o1 & o2
    p.px, p.py, p.pz = np.where(go, xn, x), np.where(go, yn, y), np.where(go, zn, z)


# ---------------------------------------------------------------------------------------------- 2. move
def owners(p):
    """(inside, d): inside[i, j, k, s] -- the slot is active and its owner lies in the grid; d = (di, dj, dk), the owner's offset from the bucket cell there"""
    n = (p.nx, p.ny, p.nz)
    with np.errstate(invalid="ignore", over="ignore"):
        f = [np.floor((c - o) * i) for c, o, i in zip((p.px, p.py, p.pz), (p.x0, p.y0, p.z0), (p._dx, p._dy, p._dz))]
        inside = p.active != 0
        for q, m in zip(f, n):
            inside &= (q >= 0.0) & (q < float(m))
    d = []
    for axis, q in enumerate(f):
        cell = np.arange(n[axis]).reshape([-1 if a == axis else 1 for a in range(4)])
        d.append(np.where(inside, q, 0.0).astype(np.int64) - cell)
    return inside, d


def _window(n, o):
    """destination and source slices along an axis of n cells for the source offset o: the destinations whose source cell exists"""
    lo, hi = max(0, -o), min(n, n - o)
    return slice(lo, hi), slice(lo + o, hi + o)


def move(src, args=()):
    """(dst, args_dst, counts): out of place.  A step handles one (source offset, slot) pair for every destination cell at once: a cell takes at most one
    particle per step, so the order of the definition is kept"""
    n3, mx = (src.nx, src.ny, src.nz), src.max_xcell
    dst = copy(src)
    srcs = [src.px, src.py, src.pz, src.active] + list(args)
    outs = [np.zeros_like(a) for a in srcs]
    inside, d = owners(src)
    act = src.active != 0
    far = inside & ((np.abs(d[0]) > 1) | (np.abs(d[1]) > 1) | (np.abs(d[2]) > 1))
    c = dict.fromkeys(COUNTS, 0)
    c["n_active_before"], c["n_outside"], c["n_far"] = int(act.sum()), int((act & ~inside).sum()), int(far.sum())
    n = np.zeros(n3, dtype=np.int64)
    for off in ((0, 0, 0),) + NEIGHBOURS:
        win = [_window(m, o) for m, o in zip(n3, off)]
        dsl, ssl = tuple(w[0] for w in win), tuple(w[1] for w in win)
        if any(s.stop <= s.start for s in dsl):
            continue
        grids = np.meshgrid(*(np.arange(s.start, s.stop) for s in dsl), indexing="ij")
        for s in range(mx):
            at = ssl + (s,)
            take = inside[at] & (d[0][at] == -off[0]) & (d[1][at] == -off[1]) & (d[2][at] == -off[2])
            if not take.any():
                continue
            fits = take & (n[dsl] < mx)
            c["n_overflow"] += int((take & ~fits).sum())
            ii, jj, kk = (g[fits] for g in grids)
            to = n[dsl][fits]
            for a, o in zip(srcs, outs):
                o[ii, jj, kk, to] = a[ii + off[0], jj + off[1], kk + off[2], s]
            n[dsl] += fits
    c["n_active_after"] = int(n.sum())
    dst.px, dst.py, dst.pz, dst.active = outs[:4]
    return dst, outs[4:], c


# ---------------------------------------------------------------------------------------------- 3. / 4. / 6. / 7. interpolation
def _nodes(p, axis, stagger, count):
    """coordinates of `count` nodes along an axis, vertices (stagger 1) or centres (0), shaped to broadcast along that axis of a 3D array"""
    o, h = ((p.x0, p.dx), (p.y0, p.dy), (p.z0, p.dz))[axis]
    i = np.arange(count, dtype=np.float64)
    c = o + i * h if stagger else o + (i + 0.5) * h
    return c.reshape([-1 if a == axis else 1 for a in range(3)])


def grid2particle(F, p):
    nx, ny, nz = p.nx, p.ny, p.nz
    assert F.shape == (nx + 1, ny + 1, nz + 1)
    v = [[[F[a:a + nx, b:b + ny, c:c + nz][..., None] for c in (0, 1)] for b in (0, 1)] for a in (0, 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        t = [(c - _nodes(p, axis, 1, m)[..., None]) * i for axis, (c, m, i) in enumerate(zip((p.px, p.py, p.pz), (nx, ny, nz), (p._dx, p._dy, p._dz)))]
        out = _trilin(t[0], t[1], t[2], v)
    return np.where(p.active != 0, out, 0.0)


def centroid2particle(pF, F, p):
    """returns the new pF: the interpolated value in the active slots whose scaled coordinates are finite, pF there otherwise, 0 in the inactive slots"""
    assert F.shape == (p.nx, p.ny, p.nz) and min(F.shape) >= 2
    v, ok = interp(F, (p.x0 + 0.5 * p.dx, p.y0 + 0.5 * p.dy, p.z0 + 0.5 * p.dz), (p._dx, p._dy, p._dz), p.px, p.py, p.pz)
    return np.where(p.active != 0, np.where(ok, v, pF), 0.0)


def _w(x, xn, inv):
    return 1.0 - np.abs(x - xn) * inv


def _gather(p, stagger, feed):
    """the walk of a member with this stagger: for every cell offset in the nesting order of (4) and every slot in order, feed(node slices, mask, w, cell index)
    with the weights of the particles of that cell to the nodes that read it"""
    n3 = (p.nx, p.ny, p.nz)
    ext = tuple(m + s for m, s in zip(n3, stagger))
    nodes = [_nodes(p, axis, stagger[axis], ext[axis]) for axis in range(3)]
    inv = (p._dx, p._dy, p._dz)
    offs = [(-1, 0) if s else (0,) for s in stagger]
    for oi in offs[0]:
        for oj in offs[1]:
            for ok in offs[2]:
                off = (oi, oj, ok)
                # nodes whose cell (node + off) exists
                lo = [max(0, -o) for o in off]
                hi = [min(e, m - o) for e, m, o in zip(ext, n3, off)]
                if any(h <= l for l, h in zip(lo, hi)):
                    continue
                nsl = tuple(slice(l, h) for l, h in zip(lo, hi))
                csl = tuple(slice(l + o, h + o) for l, h, o in zip(lo, hi, off))
                xn = [nodes[axis][tuple(nsl[axis] if a == axis else slice(None) for a in range(3))] for axis in range(3)]
                for s in range(p.max_xcell):
                    at = csl + (s,)
                    mask = p.active[at] != 0
                    with np.errstate(invalid="ignore", over="ignore"):
                        w = _w(p.px[at], xn[0], inv[0]) * _w(p.py[at], xn[1], inv[1]) * _w(p.pz[at], xn[2], inv[2])
                    feed(nsl, mask, w, at)


def _weighted_mean(F, pF, p, stagger):
    ext = tuple(m + s for m, s in zip((p.nx, p.ny, p.nz), stagger))
    assert F.shape == ext
    num, den = np.zeros(ext), np.zeros(ext)

    def feed(nsl, mask, w, at):
        with np.errstate(invalid="ignore", over="ignore"):
            num[nsl] = np.where(mask, num[nsl] + w * pF[at], num[nsl])
            den[nsl] = np.where(mask, den[nsl] + w, den[nsl])
    _gather(p, stagger, feed)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0.0, F, num / den)


def particle2grid(F, pF, p):
    """returns the new vertex field (F itself where no weight arrives)"""
    return _weighted_mean(F, pF, p, (1, 1, 1))


def particle2centroid(F, pF, p):
    """returns the new centre field (F itself in an empty cell)"""
    return _weighted_mean(F, pF, p, (0, 0, 0))


# ---------------------------------------------------------------------------------------------- 5. phase ratios
def member_shape(name, ni, nphase):
    return (nphase,) + tuple(n + s for n, s in zip(ni, STAGGER[name]))


def phase_ratios(old, pPhases, nphase, p):
    """(members, n_empty): old = dict of the eight members as they are before the call (left unchanged where no weight arrives)"""
    new, n_empty = {}, 0
    with np.errstate(invalid="ignore"):
        accepted = (pPhases >= 1.0) & (pPhases < float(nphase + 1))
    index = np.where(accepted, pPhases, 1.0).astype(np.int64) - 1
    for name in MEMBERS:
        shape = member_shape(name, (p.nx, p.ny, p.nz), nphase)
        assert old[name].shape == shape, (name, old[name].shape, shape)
        acc, W = np.zeros(shape), np.zeros(shape[1:])

        def feed(nsl, mask, w, at):
            mask = mask & accepted[at]
            with np.errstate(invalid="ignore", over="ignore"):
                for q in range(nphase):
                    sl = (q,) + nsl
                    acc[sl] = np.where(mask & (index[at] == q), acc[sl] + w, acc[sl])
                W[nsl] = np.where(mask, W[nsl] + w, W[nsl])
        _gather(p, STAGGER[name], feed)
        empty = W == 0.0
        n_empty += int(empty.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            new[name] = np.where(empty[None], old[name], acc / W[None])
    return new, n_empty
