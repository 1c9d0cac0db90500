"""NumPy restatement of the reference's particle-free phase-ratio update (src/phases/PhaseRatios.jl:24-383), written from its rules; the checker of the
tests of update_phase_ratios_2D_ / update_phase_ratios_3D_.  Arrays are (nx, ny[, nz]) with x first, as in Julia; the members come back as (N, ...) arrays,
the phase index first (CellArray layout).  Every sum is an ordered chain of vector additions (over the cells in the reference's visiting order, over the
phases k = 1..N left to right), so apart from ONE place the results carry the bits of the reference's loops: NumPy has no fma, so the 2D vertex weight
wx = muladd(-|xv - xc|, 1/dx, 1) is computed here as 1 + (-|xv - xc|) (1/dx) and rounds twice where the device's fma() rounds once (the 2D `vertex` member
agrees to rounding, every other member bit for bit).

  centres    PhaseRatios.jl:89-116    w_k = p_k[I] / t, t = sum p_k[I]
  vertices   PhaseRatios.jl:135-211   the 2^ndim cells at offsets {-1, 0}, first dimension outermost, -1 before 0; 2D weight wx wy (muladd), 3D weight
                                      ((1 (1 - |.| (1/dx))) (1 - ...)) (1 - ...) (no muladd); cells outside the grid are skipped
  faces      PhaseRatios.jl:231-293   the cells I_d - 1, I_d, weight 0.5 each
  edges      PhaseRatios.jl:324-383   the four cells at offsets (-1,-1), (-1,0), (0,-1), (0,0) in (first, second staggered dimension), weight 0.25 each
  tail       every member             w_k / W; clamp to [0, 1]; values < 1e-5 -> 0; s = sum; w_k / s
"""
import itertools

import numpy as np

MEMBERS_2D = {"center": (0, 0), "vertex": (1, 1), "Vx": (1, 0), "Vy": (0, 1)}
MEMBERS_3D = {"center": (0, 0, 0), "vertex": (1, 1, 1), "Vx": (1, 0, 0), "Vy": (0, 1, 0), "Vz": (0, 0, 1), "xy": (1, 1, 0), "yz": (0, 1, 1), "xz": (1, 0, 1)}


def members(ndim):
    """name -> staggering per dimension of every member of a PhaseRatios"""
    return MEMBERS_2D if ndim == 2 else MEMBERS_3D


def member_shape(name, ni):
    return tuple(n + s for n, s in zip(ni, members(len(ni))[name]))


def _tail(w, W):
    """w: list of N arrays (accumulated values), W: array of accumulated weights (None: the values are already normalised)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if W is not None:
            w = [x / W for x in w]
        out = []
        for x in w:
            x = np.where(x > 1.0, 1.0, np.where(x < 0.0, 0.0, x))          # clamp by comparisons: a NaN stays a NaN, as Julia's clamp / min(max()) leave it
            out.append(np.where(x < 1.0e-5, 0.0, x))
        s = np.zeros_like(out[0])
        for x in out:
            s = s + x
        return np.stack([x / s for x in out])


def _center(ps):
    t = ps[0].copy()
    for p in ps[1:]:
        t = t + p
    with np.errstate(divide="ignore", invalid="ignore"):
        return _tail([p / t for p in ps], None)


def _vertex_factor(xv, xc, dx, off, muladd):
    """per vertex of one dimension: the weight factor towards the cell at offset `off` and whether that cell exists"""
    n = len(xc)
    idx = np.arange(n + 1) + off
    ok = (idx >= 0) & (idx < n)
    dist = np.abs(xv - xc[np.clip(idx, 0, n - 1)])
    inv = 1.0 / dx
    f = 1.0 + (-dist) * inv if muladd else 1.0 - dist * inv      # 2D: muladd(-dist, inv, 1) without the fusion; 3D: as written
    return f, ok


def _stencil(ps, stag, weight_of):
    """one member: accumulate over the cells at offsets {-1, 0} in the staggered dimensions, in the reference's order"""
    ni = ps[0].shape
    nd = len(ni)
    shape = tuple(n + s for n, s in zip(ni, stag))
    grids = np.meshgrid(*[np.arange(m) for m in shape], indexing="ij")
    w = [np.zeros(shape) for _ in ps]
    W = np.zeros(shape)
    for offs in itertools.product(*[((-1, 0) if s else (0,)) for s in stag]):      # first dimension outermost, -1 before 0
        idx = [g + o for g, o in zip(grids, offs)]
        ok = np.ones(shape, dtype=bool)
        for d in range(nd):
            ok &= (idx[d] >= 0) & (idx[d] < ni[d])
        cl = tuple(np.clip(idx[d], 0, ni[d] - 1) for d in range(nd))
        wt = weight_of(offs, grids)
        W = np.where(ok, W + wt, W)
        for k, p in enumerate(ps):
            w[k] = np.where(ok, w[k] + wt * p[cl], w[k])              # a skipped cell is not read: its NaN does not spread
    return _tail(w, W)


def update_phase_ratios(phase_arrays, xci, xvi):
    """dict member name -> (N, ...) array, for 2D or 3D phase arrays"""
    ps = [np.asarray(p, dtype=np.float64) for p in phase_arrays]
    nd = ps[0].ndim
    xci = [np.asarray(x, dtype=np.float64) for x in xci]
    xvi = [np.asarray(x, dtype=np.float64) for x in xvi]
    dx = [x[1] - x[0] for x in xvi]
    fac = [{o: _vertex_factor(xvi[d], xci[d], dx[d], o, nd == 2)[0] for o in (-1, 0)} for d in range(nd)]

    def vertex_weight(offs, grids):
        wt = fac[0][offs[0]][grids[0]] * fac[1][offs[1]][grids[1]]
        if nd == 3:
            wt = wt * fac[2][offs[2]][grids[2]]
        return wt

    out = {}
    for name, stag in members(nd).items():
        ns = sum(stag)
        if ns == 0:
            out[name] = _center(ps)
        elif ns == nd:
            out[name] = _stencil(ps, stag, vertex_weight)
        else:
            out[name] = _stencil(ps, stag, lambda offs, grids, c=(0.5 if ns == 1 else 0.25): c)
    return out


def uniform_grid(ni, li=None, origin=None):
    """(xci, xvi) of a uniform grid, as Geometry builds them (np.linspace)"""
    nd = len(ni)
    li = li or (1.0,) * nd
    origin = origin or (0.0,) * nd
    xvi = tuple(np.linspace(origin[d], origin[d] + li[d], ni[d] + 1) for d in range(nd))
    xci = tuple(np.linspace(origin[d] + li[d] / ni[d] / 2, origin[d] + li[d] - li[d] / ni[d] / 2, ni[d]) for d in range(nd))
    return xci, xvi
