"""NumPy restatement of the grid-based stress rotation and advection (rotate_stress! on grids; include/jrx.h, csrc/stress_rotation.hip), written for
clarity and vectorised over the arrays.  Arrays are indexed as in the reference, A[i, j(, k)] with the Julia shape (0-based here).

    τ_o[c](I) = Rot_c(τ, ω dt)(I) - dt Adv(τ[c], v)(I)        for every member c at its own node I, both terms from the input state.

A location is a tuple of 0 / 1 per axis (1 = on a vertex along that axis): the centre (0, 0[, 0]), the 2D vertex (1, 1), the 3D edges yz (0, 1, 1),
xz (1, 0, 1), xy (1, 1, 0).  No fused multiply-add anywhere: every product and sum is rounded once, in the order written, which is the kernel's order.
Also here: V = Ω x r + u sampled on the staggered velocity nodes, the vorticity of compute_vorticity!, the analytic rotation of a tensor."""
import itertools

import numpy as np

METHODS = ("matrix", "jaumann")
ADVECTIONS = ("upwind", "none")
CENTRE2, VERTEX2 = (0, 0), (1, 1)
CENTRE3, YZ, XZ, XY = (0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)
# member -> location
MEMBERS2 = dict(xx=CENTRE2, yy=CENTRE2, xy_c=CENTRE2, xy=VERTEX2)
MEMBERS2_OPT = dict(MEMBERS2, xx_v=VERTEX2, yy_v=VERTEX2)
MEMBERS3 = dict(xx=CENTRE3, yy=CENTRE3, zz=CENTRE3, yz_c=CENTRE3, xz_c=CENTRE3, xy_c=CENTRE3, yz=YZ, xz=XZ, xy=XY)
OMEGA3 = dict(yz=YZ, xz=XZ, xy=XY)


def shape_at(loc, ni):
    return tuple(n + s for n, s in zip(ni, loc))


def velocity_shape(c, ni):
    """vertices along c, centres with one ghost node either side along the other axes"""
    return tuple(n + 1 if d == c else n + 2 for d, n in enumerate(ni))


def _mean(A, picks):
    """sum of A over the per-axis index vectors of `picks` in index order (x fastest), times 1 / 2^m"""
    total = None
    for combo in itertools.product(*reversed(picks)):          # the last axis outermost, x fastest
        v = A[np.ix_(*reversed(combo))]
        total = v if total is None else total + v
    count = 1
    for p in picks:
        count *= len(p)
    return total * (1.0 / count)


def interp(A, src, tgt, ni):
    """the array A at location src on the nodes of location tgt: the same node along an axis where the two agree; I, I + 1 where the target is on a centre;
    I - 1, I clamped into the source's extent where it is on a vertex"""
    assert A.shape == shape_at(src, ni), (A.shape, src, ni)
    picks = []
    for d, n in enumerate(ni):
        I = np.arange(n + tgt[d])
        if src[d] == tgt[d]:
            picks.append([I])
        elif tgt[d] == 0:
            picks.append([I, I + 1])
        else:
            picks.append([np.clip(I - 1, 0, n - 1), np.clip(I, 0, n - 1)])
    return _mean(A, picks)


def velocity_at(Vc, c, tgt, ni):
    """velocity component c on the nodes of location tgt; the centre j of a transverse axis is entry j + 1 (ghost layers), so every node exists"""
    assert Vc.shape == velocity_shape(c, ni), (Vc.shape, c, ni)
    picks = []
    for d, n in enumerate(ni):
        I = np.arange(n + tgt[d])
        if d == c:
            picks.append([I] if tgt[d] else [I, I + 1])
        else:
            picks.append([I, I + 1] if tgt[d] else [I + 1])
    return _mean(Vc, picks)


def upwind(A, v, _di):
    """Σ_d v_d (v_d > 0 ? A[I] - A[I - e_d] : A[I + e_d] - A[I]) _d_d with a neighbour outside the array replaced by A[I]"""
    adv = None
    for d in range(A.ndim):
        first, last = np.take(A, [0], axis=d), np.take(A, [-1], axis=d)
        lo = np.concatenate([first, np.delete(A, -1, axis=d)], axis=d)
        hi = np.concatenate([np.delete(A, 0, axis=d), last], axis=d)
        term = v[d] * np.where(v[d] > 0.0, A - lo, hi - A) * _di[d]
        adv = term if adv is None else adv + term
    return adv


# ----------------------------------------------------------------------------------------------- per-point rotations
def rot2(xx, yy, xy, θ, method):
    """2D: matrix -- R (τ R') with R = [c -s; s c], the products in the order of stress_rotation_particles.jl:182-197; jaumann -- τ + (W τ - τ W) θ"""
    if method == "matrix":
        s, c = np.sin(θ), np.cos(θ)
        ms = -s
        m11, m12 = xx * c + xy * ms, xx * s + xy * c
        m21, m22 = xy * c + yy * ms, xy * s + yy * c
        return c * m11 + ms * m21, s * m12 + c * m22, c * m12 + ms * m22
    assert method == "jaumann", method
    t2 = 2.0 * θ
    return xx - t2 * xy, yy + t2 * xy, xy + θ * (xx - yy)


def rodrigues(w, dt):
    """R = I + sinθ K + (1 - cosθ) K², θ = dt |w|, K = [w / |w|]x; |w| == 0 gives R = I without a division.  R[i][j] are arrays (or scalars)"""
    w = [np.asarray(x, dtype=np.float64) for x in w]
    nrm = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(nrm > 0.0, 1.0 / np.where(nrm > 0.0, nrm, 1.0), 0.0)
    nx, ny, nz = w[0] * inv, w[1] * inv, w[2] * inv
    θ = dt * nrm
    s, c = np.sin(θ), np.cos(θ)
    c1 = 1.0 - c
    xy, xz, yz = nx * ny, nx * nz, ny * nz
    return [[1.0 + c1 * -(ny * ny + nz * nz), s * -nz + c1 * xy, s * ny + c1 * xz],
            [s * nz + c1 * xy, 1.0 + c1 * -(nx * nx + nz * nz), s * -nx + c1 * yz],
            [s * -ny + c1 * xz, s * nx + c1 * yz, 1.0 + c1 * -(nx * nx + ny * ny)]]


def rot3(t, w, dt, method):
    """t = (xx, yy, zz, yz, xz, xy), w = (ω_yz, ω_xz, ω_xy): the rotated six components.  matrix -- R (τ R'); jaumann -- τ + (A τ - τ A), A = [dt w]x"""
    T = [[t[0], t[5], t[4]], [t[5], t[1], t[3]], [t[4], t[3], t[2]]]
    O = [[None] * 3 for _ in range(3)]
    if method == "matrix":
        R = rodrigues(w, dt)
        M = [[(T[i][0] * R[j][0] + T[i][1] * R[j][1]) + T[i][2] * R[j][2] for j in range(3)] for i in range(3)]
        for i in range(3):
            for j in range(i, 3):
                O[i][j] = (R[i][0] * M[0][j] + R[i][1] * M[1][j]) + R[i][2] * M[2][j]
    else:
        assert method == "jaumann", method
        ax, ay, az = dt * w[0], dt * w[1], dt * w[2]
        A = [[0.0, -az, ay], [az, 0.0, -ax], [-ay, ax, 0.0]]
        for i in range(3):
            for j in range(i, 3):
                k1, k2, l1, l2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                p = A[i][k1] * T[k1][j] + A[i][k2] * T[k2][j]
                q = T[i][l1] * A[l1][j] + T[i][l2] * A[l2][j]
                O[i][j] = T[i][j] + (p - q)
    return O[0][0], O[1][1], O[2][2], O[1][2], O[0][2], O[0][1]


# ----------------------------------------------------------------------------------------------- the operator
def _check(method, advection):
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}")
    if advection not in ADVECTIONS:
        raise ValueError(f"unknown advection {advection!r}")


def rotate_stress2d(τ, ω_xy, V, ni, _di, dt, method="matrix", advection="upwind"):
    """τ: dict with xx, yy, xy_c (ni), xy (ni .+ 1) and optionally xx_v, yy_v (ni .+ 1); V = (Vx, Vy) or None with advection "none".  Returns the dict τ_o"""
    _check(method, advection)
    ni = tuple(ni)
    out = {}
    # centres: own xx, yy, xy_c; ω from the four vertices
    θ = dt * interp(ω_xy, VERTEX2, CENTRE2, ni)
    out["xx"], out["yy"], out["xy_c"] = rot2(τ["xx"], τ["yy"], τ["xy_c"], θ, method)
    # vertices: own xy and ω; the normals from the four centres
    θ = dt * ω_xy
    out["xy"] = rot2(interp(τ["xx"], CENTRE2, VERTEX2, ni), interp(τ["yy"], CENTRE2, VERTEX2, ni), τ["xy"], θ, method)[2]
    if "xx_v" in τ and "yy_v" in τ:
        out["xx_v"], out["yy_v"], _ = rot2(τ["xx_v"], τ["yy_v"], τ["xy"], θ, method)
    if advection == "upwind":
        for loc in (CENTRE2, VERTEX2):
            v = [velocity_at(V[c], c, loc, ni) for c in range(2)]
            for k in out:
                if MEMBERS2_OPT[k] == loc:
                    out[k] = out[k] - dt * upwind(τ[k], v, _di)
    return out


def rotate_stress3d(τ, ω, V, ni, _di, dt, method="matrix", advection="upwind"):
    """τ: dict of the nine members of MEMBERS3; ω: dict yz, xz, xy on the edge arrays; V = (Vx, Vy, Vz) or None with advection "none".  Returns the dict τ_o"""
    _check(method, advection)
    ni = tuple(ni)
    out = {}
    w = [interp(ω[k], OMEGA3[k], CENTRE3, ni) for k in ("yz", "xz", "xy")]
    centre = ("xx", "yy", "zz", "yz_c", "xz_c", "xy_c")
    for k, r in zip(centre, rot3([τ[k] for k in centre], w, dt, method)):
        out[k] = r
    for comp, (edge, loc) in enumerate(OMEGA3.items()):
        t = [interp(τ[k], CENTRE3, loc, ni) for k in ("xx", "yy", "zz")]
        t += [τ[k] if k == edge else interp(τ[k], OMEGA3[k], loc, ni) for k in ("yz", "xz", "xy")]
        w = [ω[k] if k == edge else interp(ω[k], OMEGA3[k], loc, ni) for k in ("yz", "xz", "xy")]
        out[edge] = rot3(t, w, dt, method)[3 + comp]
    if advection == "upwind":
        for loc in (CENTRE3, YZ, XZ, XY):
            v = [velocity_at(V[c], c, loc, ni) for c in range(3)]
            for k in out:
                if MEMBERS3[k] == loc:
                    out[k] = out[k] - dt * upwind(τ[k], v, _di)
    return out


def rotate_stress(τ, ω, V, ni, _di, dt, method="matrix", advection="upwind"):
    if len(ni) == 2:
        return rotate_stress2d(τ, ω["xy"] if isinstance(ω, dict) else ω, V, ni, _di, dt, method, advection)
    return rotate_stress3d(τ, ω, V, ni, _di, dt, method, advection)


# ----------------------------------------------------------------------------------------------- helpers for the tests
def grid_coords(ni, li, origin=None):
    """(xc, xv, xg) per axis of a uniform grid: centres, vertices, centres with one ghost node either side"""
    origin = origin or (0.0,) * len(ni)
    out = []
    for n, l, o in zip(ni, li, origin):
        d = l / n
        xv = o + d * np.arange(n + 1)
        xc = o + d * (np.arange(n) + 0.5)
        xg = o + d * (np.arange(n + 2) - 0.5)
        out.append((xc, xv, xg))
    return out


def location_coords(loc, coords):
    """broadcastable coordinate arrays of the nodes of a location"""
    nd = len(loc)
    return [np.asarray(coords[d][1] if loc[d] else coords[d][0]).reshape([-1 if e == d else 1 for e in range(nd)]) for d in range(nd)]


def rigid_velocity(ni, li, Ω, u=None, origin=None, centre=None):
    """V = Ω x (r - centre) + u sampled on the staggered velocity nodes (ghost layers included).  2D: Ω a scalar (about z); 3D: a 3-vector.  Returns the tuple
    of velocity arrays"""
    nd = len(ni)
    coords = grid_coords(ni, li, origin)
    u = u or (0.0,) * nd
    centre = centre or (0.0,) * nd
    Ωv = (0.0, 0.0, float(Ω)) if nd == 2 else tuple(float(x) for x in Ω)
    out = []
    for c in range(nd):
        r = [np.asarray(coords[d][1] if d == c else coords[d][2]).reshape([-1 if e == d else 1 for e in range(nd)]) - centre[d] for d in range(nd)]
        if nd == 2:
            r.append(0.0)
        a, b = (c + 1) % 3, (c + 2) % 3
        comp = Ωv[a] * r[b] - Ωv[b] * r[a] + u[c]
        out.append(np.ascontiguousarray(np.broadcast_to(comp, velocity_shape(c, ni))).astype(np.float64))
    return tuple(out)


def vorticity(V, ni, _di):
    """compute_vorticity! (stress_rotation_particles.jl:17-80): 2D the array ω_xy on the vertices; 3D the dict yz, xz, xy on the edge arrays"""
    if len(ni) == 2:
        Vx, Vy = V
        return 0.5 * ((Vy[1:, :] - Vy[:-1, :]) * _di[0] - (Vx[:, 1:] - Vx[:, :-1]) * _di[1])
    Vx, Vy, Vz = V
    _dx, _dy, _dz = _di
    return dict(yz=0.5 * (_dy * (Vz[1:-1, 1:, :] - Vz[1:-1, :-1, :]) - _dz * (Vy[1:-1, :, 1:] - Vy[1:-1, :, :-1])),
                xz=0.5 * (_dz * (Vx[:, 1:-1, 1:] - Vx[:, 1:-1, :-1]) - _dx * (Vz[1:, 1:-1, :] - Vz[:-1, 1:-1, :])),
                xy=0.5 * (_dx * (Vy[1:, :, 1:-1] - Vy[:-1, :, 1:-1]) - _dy * (Vx[:, 1:, 1:-1] - Vx[:, :-1, 1:-1])))


def rotation_matrix(w, dt=1.0):
    """the 3 x 3 rotation by θ = dt |w| about w (the exponential of [dt w]x), from Rodrigues' formula on scalars"""
    return np.array([[float(x) for x in row] for row in rodrigues(w, dt)])


def tensor(t):
    """(xx, yy, zz, yz, xz, xy) -> the 3 x 3 matrix; (xx, yy, xy) -> the 2 x 2 matrix"""
    if len(t) == 3:
        return np.array([[t[0], t[2]], [t[2], t[1]]], dtype=np.float64)
    return np.array([[t[0], t[5], t[4]], [t[5], t[1], t[3]], [t[4], t[3], t[2]]], dtype=np.float64)


def voigt(T):
    T = np.asarray(T)
    if T.shape == (2, 2):
        return T[0, 0], T[1, 1], T[0, 1]
    return T[0, 0], T[1, 1], T[2, 2], T[1, 2], T[0, 2], T[0, 1]


def random_state(ni, seed, optional=False, scale=1.0):
    """random τ, ω, V of a grid: (τ dict, ω (2D array / 3D dict), V tuple)"""
    rng = np.random.default_rng(seed)
    nd = len(ni)
    members = (MEMBERS2_OPT if optional else MEMBERS2) if nd == 2 else MEMBERS3
    τ = {k: scale * rng.uniform(-1.0, 1.0, shape_at(loc, ni)) for k, loc in members.items()}
    if nd == 2:
        ω = rng.uniform(-1.0, 1.0, shape_at(VERTEX2, ni))
    else:
        ω = {k: rng.uniform(-1.0, 1.0, shape_at(loc, ni)) for k, loc in OMEGA3.items()}
    V = tuple(rng.uniform(-1.0, 1.0, velocity_shape(c, ni)) for c in range(nd))
    return τ, ω, V
