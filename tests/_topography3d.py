"""NumPy restatement of the 3D free-surface operators on grids, as include/jrx.h defines them (there is no reference text: the reference calls JustPIC's
marker-chain operators and a particle kernel); the checker of compute_rock_fraction_, advect_topography_ and update_phases_given_topography_ on 3D grids.

Arrays are (nx, ny[, nz]) with x first, indices 0-based, z the vertical.  Every function computes in the dtype of its arrays (float64 or np.longdouble): the scalars
z0, _dx, _dy, _dz, dt are converted to it.  Every product and sum is rounded once in the order written in the header, NumPy has no fma and the library is built
without contraction, so the float64 results carry the device's bits.

  clamp(x, lo, hi)   x >= lo ? (x <= hi ? x : hi) : lo         (comparisons: a NaN becomes lo)
  s[i, j]            (h[i, j] - z0) * _dz                        heights in cell units at the (nx + 1, ny + 1) vertex positions
  c[i, j]            0.25 * ((s[i, j] + s[i+1, j]) + (s[i, j+1] + s[i+1, j+1]))      the centre value of cell (i, j)
  Ψ(a, b, c)         the mean of max(g, 0) over a triangle, g linear with the sorted vertex values a <= b <= c
  T(g1, g2, g3, H)   the mean of clamp(g, 0, H) over it
  q(A, X, Y, c; b, H)  the volume of a quadrant (corner A, its cell's neighbours X, Y along x, y, the cell's centre c) inside the z range [b, b + H]

FOOTPRINTS lists, for each of the four footprints, the quadrants in the order in which their volumes are summed (starting from 0): (oi, oj, dx, dy) is the
quadrant of the vertex (i + oi, j + oj) towards (dx, dy); it lies in the cell (i + oi - (dx < 0), j + oj - (dy < 0)) and is skipped when that cell is outside
the domain.  MEMBER_DEF pairs every member of a 3D RockRatio with its footprint and its z range ("cell" rows or "vertex" rows).
"""
import numpy as np

MEMBERS = ("center", "vertex", "Vx", "Vy", "Vz", "yz", "xz", "xy")
FOOTPRINTS = dict(
    cell=((0, 0, +1, +1), (1, 0, -1, +1), (0, 1, +1, -1), (1, 1, -1, -1)),
    xface=((0, 0, -1, +1), (0, 1, -1, -1), (0, 0, +1, +1), (0, 1, +1, -1)),
    yface=((0, 0, +1, -1), (1, 0, -1, -1), (0, 0, +1, +1), (1, 0, -1, +1)),
    vertex=((0, 0, -1, -1), (0, 0, +1, -1), (0, 0, -1, +1), (0, 0, +1, +1)),
)
MEMBER_DEF = dict(center=("cell", "cell"), Vz=("cell", "vertex"), Vx=("xface", "cell"), xz=("xface", "vertex"),
                  Vy=("yface", "cell"), yz=("yface", "vertex"), xy=("vertex", "cell"), vertex=("vertex", "vertex"))


def footprint_extent(foot, ni):
    nx, ny = ni[0], ni[1]
    return dict(cell=(nx, ny), xface=(nx + 1, ny), yface=(nx, ny + 1), vertex=(nx + 1, ny + 1))[foot]


def member_shape(name, ni):
    foot, rows = MEMBER_DEF[name]
    return footprint_extent(foot, ni) + (ni[2] if rows == "cell" else ni[2] + 1,)


def clamp(x, lo, hi):
    return np.where(x >= lo, np.where(x <= hi, x, hi), lo)


def cell_heights(h, z0, _dz):
    h = np.asarray(h)
    T = h.dtype.type
    return (h - T(z0)) * T(_dz)


def cell_centres(s):
    T = s.dtype.type
    return T(0.25) * ((s[:-1, :-1] + s[1:, :-1]) + (s[:-1, 1:] + s[1:, 1:]))


def sort3(g1, g2, g3):
    """three comparisons: (g1, g2), then g3 against the larger, then the two smaller"""
    w = g2 < g1
    lo, hi = np.where(w, g2, g1), np.where(w, g1, g2)
    w = g3 < hi
    c, m = np.where(w, hi, g3), np.where(w, g3, hi)
    w = m < lo
    return np.where(w, m, lo), np.where(w, lo, m), c


def psi(a, b, c):
    T = a.dtype.type
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mean = ((a + b) + c) / T(3)
        top = ((c * c) * c) / ((T(3) * (c - a)) * (c - b))
        na = -a
        bot = mean + ((na * na) * na) / ((T(3) * (b - a)) * (c - a))
    return np.where(c <= 0, T(0), np.where(a >= 0, mean, np.where(b <= 0, top, bot)))


def triangle(g1, g2, g3, H):
    """T(g1, g2, g3, H): the mean over a triangle of clamp(g, 0, H), g linear with the vertex values g1, g2, g3"""
    g1, g2, g3, H = np.broadcast_arrays(g1, g2, g3, H)
    T = g1.dtype.type
    a, b, c = sort3(g1, g2, g3)
    return np.where(a >= H, H, np.where(c <= 0, T(0), psi(a, b, c) - psi(a - H, b - H, c - H)))


def quadrant(A, X, Y, c, b, H):
    T = A.dtype.type
    mx, my = T(0.5) * (A + X), T(0.5) * (A + Y)
    return T(0.125) * triangle(A - b, mx - b, c - b, H) + T(0.125) * triangle(A - b, my - b, c - b, H)


def z_rows(rows, nz, T):
    """b, H of the z ranges: the cell rows k = 0 .. nz - 1, or the volumes centred on the vertex rows k = 0 .. nz clipped to the domain"""
    if rows == "cell":
        return np.arange(nz).astype(T), np.ones(nz, dtype=T)
    k = np.arange(nz + 1).astype(T)
    b = np.maximum(k - T(0.5), T(0))
    t = np.minimum(k + T(0.5), T(nz))
    return b, t - b


def footprint_fraction(s, c, foot, ni, b, H):
    """clamp(sum / (area * H), 0, 1) over a footprint's extents and the z ranges (b, H)"""
    nx, ny = ni[0], ni[1]
    T = s.dtype.type
    Fi, Fj = footprint_extent(foot, ni)
    I, J = np.meshgrid(np.arange(Fi), np.arange(Fj), indexing="ij")
    b3, H3 = np.asarray(b, dtype=s.dtype)[None, None, :], np.asarray(H, dtype=s.dtype)[None, None, :]
    total = np.zeros((Fi, Fj, len(b)), dtype=s.dtype)
    count = np.zeros((Fi, Fj), dtype=np.int64)
    for oi, oj, dx, dy in FOOTPRINTS[foot]:
        vi, vj = I + oi, J + oj
        ci, cj = vi - (dx < 0), vj - (dy < 0)
        ok = (ci >= 0) & (ci < nx) & (cj >= 0) & (cj < ny)
        A = s[vi, vj]
        X = s[np.clip(vi + dx, 0, nx), vj]
        Y = s[vi, np.clip(vj + dy, 0, ny)]
        cc = c[np.clip(ci, 0, nx - 1), np.clip(cj, 0, ny - 1)]
        q = quadrant(A[:, :, None], X[:, :, None], Y[:, :, None], cc[:, :, None], b3, H3)
        total = np.where(ok[:, :, None], total + q, total)
        count += ok
    area = T(0.25) * count.astype(T)
    return clamp(total / (area[:, :, None] * H3), T(0), T(1))


def compute_rock_fraction(h, ni, z0, _dz, members=MEMBERS):
    """dict of the members of ϕ from the heights h (nx + 1, ny + 1) at the vertex positions"""
    s = cell_heights(h, z0, _dz)
    c = cell_centres(s)
    T = s.dtype.type
    out = {}
    for name in members:
        foot, rows = MEMBER_DEF[name]
        b, H = z_rows(rows, ni[2], T)
        out[name] = np.asfortranarray(footprint_fraction(s, c, foot, ni, b, H))
    return out


def vertex_velocity(Vx, Vy, Vz):
    """vxv, vyv, vzv on the (nx + 1, ny + 1, nz + 1) vertices from the ghosted V"""
    T = Vx.dtype.type
    q = T(0.25)
    vxv = q * ((Vx[:, :-1, :-1] + Vx[:, :-1, 1:]) + (Vx[:, 1:, :-1] + Vx[:, 1:, 1:]))
    vyv = q * ((Vy[:-1, :, :-1] + Vy[:-1, :, 1:]) + (Vy[1:, :, :-1] + Vy[1:, :, 1:]))
    vzv = q * ((Vz[:-1, :-1, :] + Vz[1:, :-1, :]) + (Vz[:-1, 1:, :] + Vz[1:, 1:, :]))
    return vxv, vyv, vzv


def advect_topography(h_old, Vx, Vy, Vz, ni, z0, _dx, _dy, _dz, dt):
    """the new heights from h_old: first-order semi-Lagrangian step"""
    nx, ny, nz = ni
    h_old = np.asarray(h_old)
    T = h_old.dtype.type
    dt, _dx, _dy = T(dt), T(_dx), T(_dy)
    s = cell_heights(h_old, z0, _dz)
    sig = clamp(s, T(0), T(nz))
    k0 = np.minimum(np.floor(sig).astype(np.int64), nz - 1)
    t = sig - k0.astype(T)
    vv = vertex_velocity(*(np.asarray(v, dtype=h_old.dtype) for v in (Vx, Vy, Vz)))
    I, J = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    vx, vy, vz = ((T(1) - t) * v[I, J, k0] + t * v[I, J, k0 + 1] for v in vv)
    xi = clamp(I.astype(T) - (vx * dt) * _dx, T(0), T(nx))
    i0 = np.minimum(np.floor(xi).astype(np.int64), nx - 1)
    r = xi - i0.astype(T)
    eta = clamp(J.astype(T) - (vy * dt) * _dy, T(0), T(ny))
    j0 = np.minimum(np.floor(eta).astype(np.int64), ny - 1)
    q = eta - j0.astype(T)
    lo = (T(1) - r) * h_old[i0, j0] + r * h_old[i0 + 1, j0]
    hi = (T(1) - r) * h_old[i0, j0 + 1] + r * h_old[i0 + 1, j0 + 1]
    return np.asfortranarray(((T(1) - q) * lo + q * hi) + vz * dt)


def update_phases_given_topography(phases, h, ni, z0, _dz, air_phase):
    """new phase fields (a list of (nx, ny, nz) arrays) from the N cell-centred fields and the surface; air_phase is 1-based.  Returns (fields, rewritten mask)"""
    nx, ny, nz = ni
    c = [np.array(p, order="F") for p in phases]
    N = len(c)
    a = air_phase - 1
    T = c[0].dtype.type
    f_all = compute_rock_fraction(np.asarray(h, dtype=c[0].dtype), ni, z0, _dz, members=("center",))["center"]
    rock = [k for k in range(N) if k != a]
    p = {k: np.full((nx, ny), T(1) if k == rock[0] else T(0)) for k in rock}          # nothing carried yet: all on the lowest non-air index
    rewritten = np.zeros(ni, dtype=bool)
    for kz in range(nz):
        f = f_all[:, :, kz]
        R = np.zeros((nx, ny), dtype=c[0].dtype)
        for k in rock:
            R = R + c[k][:, :, kz]
        pos = R > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            for k in rock:
                p[k] = np.where(pos, c[k][:, :, kz] / R, p[k])
        air = T(1) - f
        wr = ~(c[a][:, :, kz] == air)
        for k in rock:
            c[k][:, :, kz] = np.where(wr, f * p[k], c[k][:, :, kz])
        c[a][:, :, kz] = np.where(wr, air, c[a][:, :, kz])
        rewritten[:, :, kz] = wr
    return c, rewritten
