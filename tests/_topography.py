"""NumPy restatement of the 2D free-surface operators on grids, as include/jrx.h defines them (there is no reference text: the reference calls JustPIC's
marker-chain operators and a particle kernel); the checker of compute_rock_fraction_, advect_topography_ and update_phases_given_topography_.

Arrays are (nx, ny) with x first, indices 0-based.  Every function computes in the dtype of its arrays (float64 or np.longdouble): the scalars y0, _dx, _dy, dt
are converted to it.  Every product and sum is rounded once in the order written in the header, NumPy has no fma and the library is built without
contraction, so the float64 results carry the device's bits.

  clamp(x, lo, hi)   x >= lo ? (x <= hi ? x : hi) : lo         (comparisons: a NaN becomes lo)
  s[i]               (h[i] - y0) * _dy                           heights in cell units
  m[i]               0.5 * (s[i] + s[i + 1])                      midpoint of segment i
  Φ(g, H)            g <= 0: 0;  g < H: (0.5 g) g;  else H g - (0.5 H) H
  P(ga, gb, w, H)    ga == gb: w clamp(ga, 0, H);  else (w (Φ(gb) - Φ(ga))) / (gb - ga)
"""
import numpy as np

MEMBERS = ("center", "vertex", "Vx", "Vy")


def member_shape(name, ni):
    nx, ny = ni
    return dict(center=(nx, ny), vertex=(nx + 1, ny + 1), Vx=(nx + 1, ny), Vy=(nx, ny + 1))[name]


def clamp(x, lo, hi):
    return np.where(x >= lo, np.where(x <= hi, x, hi), lo)


def cell_heights(h, y0, _dy):
    h = np.asarray(h)
    T = h.dtype.type
    return (h - T(y0)) * T(_dy)


def _phi(g, H):
    T = g.dtype.type
    return np.where(g <= 0, T(0), np.where(g < H, (T(0.5) * g) * g, H * g - (T(0.5) * H) * H))


def primitive(ga, gb, w, H):
    """area below one linear piece inside a volume of width w and height H (cell units); ga, gb: end heights above the volume's bottom"""
    T = ga.dtype.type
    w = T(w)
    H = np.asarray(H, dtype=ga.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (w * (_phi(gb, H) - _phi(ga, H))) / (gb - ga)
    return np.where(ga == gb, w * clamp(ga, T(0), H), slope)


def _unit(x):
    T = x.dtype.type
    return clamp(x, T(0), T(1))


def vertex_rows(ny, T):
    """b, H of the volumes centred on the vertex rows j = 0 .. ny, clipped to the domain"""
    j = np.arange(ny + 1).astype(T)
    b = np.maximum(j - T(0.5), T(0))
    t = np.minimum(j + T(0.5), T(ny))
    return b, t - b


def compute_rock_fraction(h, ni, y0, _dy):
    """dict of the four members of ϕ from the heights h (nx + 1) at the vertex abscissae"""
    nx, ny = ni
    s = cell_heights(h, y0, _dy)
    T = s.dtype.type
    m = T(0.5) * (s[:-1] + s[1:])
    one = np.ones((), dtype=s.dtype)
    jc = np.arange(ny).astype(T)[None, :]
    b, H = vertex_rows(ny, T)
    b, H = b[None, :], H[None, :]
    sl, sr = s[:-1, None], s[1:, None]
    out = {}
    out["center"] = _unit(primitive(sl - jc, sr - jc, 1, one))
    out["Vy"] = _unit(primitive(sl - b, sr - b, 1, H) / H)
    # the two halves of a vertex column: left (m[i-1] .. s[i]) for i > 0, right (s[i] .. m[i]) for i < nx, added in that order
    sv = s[:, None]
    ml = np.concatenate(([s[0]], m))[:, None]            # entry 0 unused
    mr = np.concatenate((m, [s[-1]]))[:, None]           # entry nx unused
    hasl = (np.arange(nx + 1) > 0)[:, None]
    hasr = (np.arange(nx + 1) < nx)[:, None]
    W = np.where(hasl & hasr, T(1), T(0.5))

    def halves(bot, Hh):
        left = primitive(ml - bot, sv - bot, 0.5, Hh)
        right = primitive(sv - bot, mr - bot, 0.5, Hh)
        return np.where(hasl, np.where(hasr, left + right, left), right)

    out["Vx"] = _unit(halves(jc, one) / W)
    out["vertex"] = _unit(halves(b, H) / (W * H))
    return {k: np.asfortranarray(v) for k, v in out.items()}


def vertex_velocity(Vx, Vy):
    """vxv(i, j) = 0.5 (Vx[i, j] + Vx[i, j + 1]), vyv(i, j) = 0.5 (Vy[i, j] + Vy[i + 1, j]) on the (nx + 1, ny + 1) vertices (ghosted V)"""
    T = Vx.dtype.type
    return T(0.5) * (Vx[:, :-1] + Vx[:, 1:]), T(0.5) * (Vy[:-1, :] + Vy[1:, :])


def advect_topography(h_old, Vx, Vy, ni, y0, _dx, _dy, dt):
    """the new heights from h_old: first-order semi-Lagrangian step"""
    nx, ny = ni
    h_old = np.asarray(h_old)
    T = h_old.dtype.type
    dt, _dx = T(dt), T(_dx)
    s = cell_heights(h_old, y0, _dy)
    sig = clamp(s, T(0), T(ny))
    j0 = np.minimum(np.floor(sig).astype(np.int64), ny - 1)
    t = sig - j0.astype(T)
    vxv, vyv = vertex_velocity(np.asarray(Vx, dtype=h_old.dtype), np.asarray(Vy, dtype=h_old.dtype))
    i = np.arange(nx + 1)
    vx = (T(1) - t) * vxv[i, j0] + t * vxv[i, j0 + 1]
    vy = (T(1) - t) * vyv[i, j0] + t * vyv[i, j0 + 1]
    xi = clamp(i.astype(T) - (vx * dt) * _dx, T(0), T(nx))
    i0 = np.minimum(np.floor(xi).astype(np.int64), nx - 1)
    r = xi - i0.astype(T)
    return ((T(1) - r) * h_old[i0] + r * h_old[i0 + 1]) + vy * dt


def update_phases_given_topography(phases, h, ni, y0, _dy, air_phase):
    """new phase fields (a list of (nx, ny) arrays) from the N cell-centred fields and the surface; air_phase is 1-based.  Returns (fields, rewritten mask)"""
    nx, ny = ni
    c = [np.array(p, order="F") for p in phases]
    N = len(c)
    a = air_phase - 1
    T = c[0].dtype.type
    f_all = compute_rock_fraction(np.asarray(h, dtype=c[0].dtype), ni, y0, _dy)["center"]
    rock = [k for k in range(N) if k != a]
    p = {k: np.full(nx, T(1) if k == rock[0] else T(0)) for k in rock}          # nothing carried yet: all on the lowest non-air index
    rewritten = np.zeros((nx, ny), dtype=bool)
    for j in range(ny):
        f = f_all[:, j]
        R = np.zeros(nx, dtype=c[0].dtype)
        for k in rock:
            R = R + c[k][:, j]
        pos = R > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            for k in rock:
                p[k] = np.where(pos, c[k][:, j] / R, p[k])
        air = T(1) - f
        wr = ~(c[a][:, j] == air)
        for k in rock:
            c[k][:, j] = np.where(wr, f * p[k], c[k][:, j])
        c[a][:, j] = np.where(wr, air, c[a][:, j])
        rewritten[:, j] = wr
    return c, rewritten
