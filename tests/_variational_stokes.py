"""NumPy restatement of the reference's 2D variational Stokes solver, written from its sources: src/variational_stokes/mask.jl (RockRatio,
update_rock_ratio!, compute_rock_ratio, isvalid_*), MiniKernels.jl (masked differences / averages), VelocityKernels.jl:6-59,332-401 (compute_∇V!,
compute_strain_rate!, compute_V! with dt), StressKernels.jl:2-170 (update_stresses_center_vertex! 2D), Stokes2D.jl:24-314 (_solve_VS!),
rheology/Viscosity.jl:382-418,599-650 (compute_viscosity_kernel!, compute_phase_viscosity, correct_phase_ratio), PressureKernels.jl (compute_P!, phase form),
Utils.jl (compute_maxloc!), plus the GeoParams-side helpers as rheology/StressUpdate.jl states them (plastic_params_phase, compute_yieldfunction_phase,
compute_plastic_gradients_phase: Drucker-Prager, no softening) and LinearViscous / ConstantDensity laws only.

Arrays are Julia-shaped (x first); indices here are 0-based.  Names follow jrx_vep2d_fields (miniapps Setup.arrays); phase ratios are (nphase, ...).
NumPy has no fused multiply-add: where the reference says @muladd this file rounds twice.
"""
import numpy as np

SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


# ---------------------------------------------------------------- mask.jl
def rock_ratio(*ni):
    """RockRatio(nx, ny[, nz]) (mask.jl:15-42): zero-initialised members"""
    if len(ni) == 1 and isinstance(ni[0], (tuple, list)):
        ni = tuple(ni[0])
    if not all(isinstance(n, (int, np.integer)) for n in ni):
        raise TypeError("RockRatio sizes must be integers")
    z = lambda *s: np.zeros(s, order="F")
    if len(ni) == 2:
        nx, ny = ni
        d = z(1, 1)
        return dict(center=z(nx, ny), vertex=z(nx + 1, ny + 1), Vx=z(nx + 1, ny), Vy=z(nx, ny + 1), Vz=d, yz=d, xz=d, xy=d)
    nx, ny, nz = ni
    return dict(center=z(nx, ny, nz), vertex=z(nx + 1, ny + 1, nz + 1), Vx=z(nx + 1, ny, nz), Vy=z(nx, ny + 1, nz), Vz=z(nx, ny, nz + 1),
                yz=z(nx, ny + 1, nz + 1), xz=z(nx + 1, ny, nz + 1), xy=z(nx + 1, ny + 1, nz))


def compute_rock_ratio(ratio, air_phase):
    """mask.jl:112-119 over a whole CellArray (nphase, ...); air_phase is 1-based"""
    if not 1 <= air_phase <= ratio.shape[0]:
        return np.ones(ratio.shape[1:], order="F")
    x = 1 - ratio[air_phase - 1]
    return np.asfortranarray(x * (x > 1.0e-5))


def update_rock_ratio(phi, pr, air_phase):
    """update_rock_ratio! (mask.jl:63-157): center, vertex unclamped; the other members clamped to [0, 1].  pr: dict of (nphase, ...) arrays"""
    phi["center"][...] = compute_rock_ratio(pr["center"], air_phase)
    phi["vertex"][...] = compute_rock_ratio(pr["vertex"], air_phase)
    names = ("Vx", "Vy") if phi["center"].ndim == 2 else ("Vx", "Vy", "Vz", "xy", "yz", "xz")
    for k in names:
        phi[k][...] = np.clip(compute_rock_ratio(pr[k], air_phase), 0, 1)


def isvalid(A, *I):
    return bool(A[I] > 0)


def isvalid_c(phi, i, j):
    return isvalid(phi["Vx"], i, j) and isvalid(phi["Vx"], i + 1, j) and isvalid(phi["Vy"], i, j) and isvalid(phi["Vy"], i, j + 1) and isvalid(phi["center"], i, j)


def isvalid_v(phi, i, j):
    ny = phi["Vx"].shape[1]
    j_bot, j0 = max(j - 1, 0), min(j, ny - 1)
    nx = phi["Vy"].shape[0]
    i_left, i0 = max(i - 1, 0), min(i, nx - 1)
    return (isvalid(phi["Vx"], i, j0) and isvalid(phi["Vx"], i, j_bot) and isvalid(phi["Vy"], i0, j) and isvalid(phi["Vy"], i_left, j)
            and isvalid(phi["vertex"], i, j))


def isvalid_vx(phi, i, j):
    return isvalid(phi["Vx"], i, j)


def isvalid_vy(phi, i, j):
    return isvalid(phi["Vy"], i, j)


def valid_masks(phi):
    """the four predicates over the whole grid: c (nx, ny), v (nx+1, ny+1), vx (nx+1, ny), vy (nx, ny+1)"""
    vx, vy = phi["Vx"] > 0, phi["Vy"] > 0
    nx, ny = phi["center"].shape
    c = vx[:-1] & vx[1:] & vy[:, :-1] & vy[:, 1:] & (phi["center"] > 0)
    jj = np.arange(ny + 1)
    ii = np.arange(nx + 1)
    j0, jb = np.minimum(jj, ny - 1), np.maximum(jj - 1, 0)
    i0, il = np.minimum(ii, nx - 1), np.maximum(ii - 1, 0)
    v = vx[:, j0] & vx[:, jb] & vy[i0, :] & vy[il, :] & (phi["vertex"] > 0)
    return dict(c=c, v=v, vx=vx, vy=vy)


# ---------------------------------------------------------------- MiniKernels.jl (masked: A[I] * ϕ[I])
def center(A, p, i, j): return A[i, j] * p[i, j]
def right(A, p, i, j): return A[i + 1, j] * p[i + 1, j]
def left(A, p, i, j): return A[i - 1, j] * p[i - 1, j]
def front(A, p, i, j): return A[i, j + 1] * p[i, j + 1]
def back(A, p, i, j): return A[i, j - 1] * p[i, j - 1]
def next_(A, p, i, j): return A[i + 1, j + 1] * p[i + 1, j + 1]
def d_xa(A, p, _dx, i, j): return (-center(A, p, i, j) + right(A, p, i, j)) * _dx
def d_ya(A, p, _dy, i, j): return (-center(A, p, i, j) + front(A, p, i, j)) * _dy
def d_xi(A, p, _dx, i, j): return (-front(A, p, i, j) + next_(A, p, i, j)) * _dx
def d_yi(A, p, _dy, i, j): return (-right(A, p, i, j) + next_(A, p, i, j)) * _dy
def av_xa(A, p, i, j): return (center(A, p, i, j) + right(A, p, i, j)) * 0.5
def av_ya(A, p, i, j): return (center(A, p, i, j) + front(A, p, i, j)) * 0.5
def av_xi(A, p, i, j): return (front(A, p, i, j) + next_(A, p, i, j)) * 0.5
def av_yi(A, p, i, j): return (right(A, p, i, j) + next_(A, p, i, j)) * 0.5


def mymaskedsum(A, p, *ranges, f=lambda x: x):
    s = 0.0
    for I in np.ndindex(*[len(r) for r in ranges]):
        idx = tuple(r[k] for r, k in zip(ranges, I))
        s += f(A[idx]) * p[idx]
    return s


def av(A, p, i, j): return 0.25 * mymaskedsum(A, p, range(i + 1, i + 3), range(j + 1, j + 3))
def av_a(A, p, i, j): return 0.25 * mymaskedsum(A, p, range(i, i + 2), range(j, j + 2))


# ---------------------------------------------------------------- rheology helpers (phases: list of dicts as the miniapps give them)
def _ratio_sum(vals, r):
    """fn_ratio (src/phases/phases.jl:6-15): Σ (iszero(r) ? 0 : val * r)"""
    x = np.zeros(r.shape[1:])
    for q, v in enumerate(vals):
        with np.errstate(invalid="ignore"):
            x = x + np.where(r[q] == 0.0, 0.0, v * r[q])
    return x


def correct_phase_ratio(air_phase, ratio):
    """rheology/Viscosity.jl:638-650 for one ratio vector (air_phase 1-based); `≈ 1` is isapprox with rtol = sqrt(eps)"""
    ratio = np.asarray(ratio, dtype=float)
    if air_phase == 0:
        return ratio
    ra = ratio[air_phase - 1]
    if abs(ra - 1.0) <= SQRT_EPS * max(abs(ra), 1.0):
        return np.zeros_like(ratio)
    c = ratio.copy()
    c[air_phase - 1] = 0.0
    s = 0.0
    for x in c:
        s += x
    return c / s


def _correct_all(r, air_phase):
    if air_phase == 0:
        return r
    ra = r[air_phase - 1]
    isair = np.abs(ra - 1.0) <= SQRT_EPS * np.maximum(np.abs(ra), 1.0)
    c = r.copy()
    c[air_phase - 1] = 0.0
    s = np.zeros(r.shape[1:])
    for q in range(r.shape[0]):
        s = s + c[q]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = c / s
    c[:, isair] = 0.0
    return c


def phase_viscosity(phases, r):
    """compute_phase_viscosity (Viscosity.jl:599-619), LinearViscous elements"""
    s = np.zeros(r.shape[1:])
    for q, ph in enumerate(phases):
        s = s + np.where(r[q] != 0.0, (1.0 / ph["eta"]) * r[q], 0.0)
    with np.errstate(divide="ignore"):
        e = 1.0 / s
    for q in reversed(range(len(phases))):          # the first phase above 0.999 wins
        e = np.where(r[q] > 0.999, phases[q]["eta"], e)
    return e


def compute_viscosity(a, phases, nu, cutoff, air_phase=0):
    """compute_viscosity! / update_viscosity_τII! for LinearViscous phases (the invariant is not read): centres and vertices"""
    for eta, ph in (("eta", "phase_c"), ("eta_v", "phase_v")):
        if a.get(eta) is None:
            continue
        e = phase_viscosity(phases, _correct_all(a[ph], air_phase))
        with np.errstate(invalid="ignore"):
            e = e * nu + a[eta] * (1.0 - nu)
        a[eta][...] = np.minimum(np.maximum(e, cutoff[0]), cutoff[1])


def _law_viscosity(ph, AII, T, P, tau):
    """the viscous element of a phase: LinearViscous η, or a power-law creep (GeoParams DislocationCreep with r = 0, forms as include/jrx.h states them):
    compute_viscosity_τII = τII / (2 ε(τII)), ε = A (τII FT)^n exp(-(E + P V)/(R T)) / FE; compute_viscosity_εII = τ(εII) / (2 εII),
    τ = A^(-1/n) (εII FE)^(1/n) exp((E + P V)/(n R T)) / FT"""
    cr = ph.get("creep")
    if cr is None:
        return np.full(np.shape(AII), float(ph["eta"]))
    FT, FE = {"AxialCompression": (3.0 ** 0.5, 2.0 / 3.0 ** 0.5), "SimpleShear": (2.0, 2.0), "Invariant": (1.0, 1.0)}[cr.get("apparatus", "AxialCompression")]
    A, n, R = cr["A"], cr["n"], cr.get("R", 8.3145)
    H, RT = cr.get("E", 0.0) + P * cr.get("V", 0.0), R * T
    if tau:
        return 0.5 * AII / (A * (AII * FT) ** n * np.exp(-H / RT) / FE)
    return 0.5 * (A ** (-1.0 / n) * (AII * FE) ** (1.0 / n) * np.exp(H / (n * RT)) / FT) / AII


def _visc_invariant(xx, yy, xy):
    """Viscosity.jl:391-409: eps() on the normal components of an all-zero tensor"""
    a0 = np.where((xx == 0.0) & (yy == 0.0) & (xy == 0.0), np.finfo(float).eps, 0.0)
    x, y = a0 + xx, -a0 + yy
    return np.sqrt(0.5 * (x * x + y * y) + xy * xy)


def compute_viscosity_fields(a, phases, nu, cutoff, air_phase, tau, T):
    """compute_viscosity_kernel! (Viscosity.jl:382-418) for laws that read fields, with the air_phase correction: the invariant of @stress_center / @strain_center
    at a centre, of (0, 0, xy) at a vertex (the PT solvers never write xx_v, yy_v); P and T (cell-centred, ni) at the cell, and averaged over the clamped
    surrounding cells at a vertex (local_viscosity_args, local_viscosity_args_vertex :513-552)"""
    pre = "t" if tau else "e"
    for eta, ph, AII, Tn, Pn in (("eta", "phase_c", _visc_invariant(a[pre + "xx"], a[pre + "yy"], a[pre + "xy_c"]), T, a["P"]),
                                 ("eta_v", "phase_v", _visc_invariant(0.0 * a[pre + "xy"], 0.0 * a[pre + "xy"], a[pre + "xy"]), _av_clamped(T), _av_clamped(a["P"]))):
        c = _correct_all(a[ph], air_phase)
        x, dom, has = np.zeros(AII.shape), np.zeros(AII.shape), np.zeros(AII.shape, dtype=bool)
        for q, law in enumerate(phases):
            with np.errstate(all="ignore"):
                v = _law_viscosity(law, AII, Tn, Pn, tau)
                first = ~has & (c[q] > 0.999)
                dom, has = np.where(first, v, dom), has | first
                x = x + np.where(c[q] != 0.0, (1.0 / v) * c[q], 0.0)
        with np.errstate(all="ignore"):
            e = np.where(has, dom, 1.0 / x)
            e = e * nu + a[eta] * (1.0 - nu)
        a[eta][...] = np.minimum(np.maximum(e, cutoff[0]), cutoff[1])


def compute_rhog(a, phases):
    """compute_ρg!(ρg[end], phase_ratios, rheology, args), ConstantDensity: fn_ratio with the ratio == 1 shortcut (src/phases/phases.jl:17-30)"""
    r = a["phase_c"]
    x = np.zeros(r.shape[1:])
    for q, ph in enumerate(phases):
        x = x + np.where(r[q] == 0.0, 0.0, ph["density"]["rho0"] * r[q])
    for q in reversed(range(len(phases))):
        x = np.where(r[q] == 1.0, phases[q]["density"]["rho0"] * r[q], x)
        # an earlier phase with ratio 1 returns first; ratios sum to one, so at most one phase has it
    a["fy"][...] = x * float(phases[0].get("g", 0.0))


def _plastic_tables(phases):
    pl = [ph.get("C") is not None for ph in phases]
    sinphi = [np.sin(np.radians(ph["phi_deg"])) if p else 0.0 for ph, p in zip(phases, pl)]
    cosphi = [np.cos(np.radians(ph["phi_deg"])) if p else 0.0 for ph, p in zip(phases, pl)]
    sinpsi = [np.sin(np.radians(ph.get("psi_deg", 0.0))) if p else 0.0 for ph, p in zip(phases, pl)]
    return pl, sinphi, cosphi, sinpsi


def _sinv2(xx, yy, xy):
    return np.sqrt(0.5 * (xx * xx + yy * yy) + xy * xy)


def _stress_inc(t, to, eta, e, _Gdt, dtr):
    """compute_stress_increment (StressKernels.jl:2-5): dτ_r * fma(2η, ε, fma(-(τ - τ_o) η, _Gdt, -τ))"""
    return dtr * (2.0 * eta * e + (-(t - to) * eta * _Gdt + (-t)))


def _node_update(phases, r, P, tij, toij, eij, eta, lam, EII, dt, th, rel):
    """the part of update_stresses_center_vertex! shared by a valid vertex and a valid centre; returns (τ_new (3), λ_new, ε_pl (3), yielding, dQdP, K, τII)"""
    pl, sinphi, cosphi, sinpsi = _plastic_tables(phases)
    G = _ratio_sum([ph["G"] for ph in phases], r)
    K = _ratio_sum([ph["Kb"] for ph in phases], r)
    _Gdt = 1.0 / (G * dt)
    is_pl = any(pl)
    eta_reg = np.zeros(r.shape[1:])
    for q, ph in enumerate(phases):
        if pl[q]:
            eta_reg = eta_reg + ph.get("eta_vp", 0.0) * r[q]
    dtr = 1.0 / (th + eta * _Gdt + 1.0)
    d = [_stress_inc(tij[q], toij[q], eta, eij[q], _Gdt, dtr) for q in range(3)]
    tII = _sinv2(d[0] + tij[0], d[1] + tij[1], d[2] + tij[2])
    tt = [tij[q] + d[q] for q in range(3)]
    ttII = _sinv2(*tt)
    dQdt = [np.zeros_like(tII) for _ in range(3)]
    dQdP, dFdP, F = np.zeros_like(tII), np.zeros_like(tII), np.zeros_like(tII)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = [0.5 * tt[0] / ttII, 0.5 * tt[1] / ttII, 0.5 * (tt[2] / ttII)]
    for q, ph in enumerate(phases):
        on = r[q] != 0.0
        if pl[q]:
            for s in range(3):
                dQdt[s] = np.where(on, r[q] * g[s] + dQdt[s], dQdt[s])
            dQdP = np.where(on, r[q] * -sinpsi[q] + dQdP, dQdP)
            dFdP = np.where(on, r[q] * -sinphi[q] + dFdP, dFdP)
            Fq = tII - cosphi[q] * ph["C"] - sinphi[q] * P
        else:
            Fq = tII
        F = np.where(on, F + r[q] * Fq, F)
    with np.errstate(invalid="ignore"):
        vol = np.where(np.isinf(K), 0.0, K * dt * dFdP * dQdP)
    yld = is_pl & (tII != 0.0) & (F > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        lam_new = np.where(yld, (1.0 - rel) * lam + rel * (np.maximum(F, 0.0) / (eta * dtr + eta_reg + vol)), lam)
    epl = [np.where(yld, lam_new * dQdt[q], 0.0) for q in range(3)]
    with np.errstate(invalid="ignore"):
        dd = [np.where(yld, -2.0 * eta * epl[q] * dtr + d[q], d[q]) for q in range(3)]
    tnew = [dd[q] + tij[q] for q in range(3)]
    tII_out = np.where(yld, _sinv2(*tnew), tII)
    return tnew, lam_new, epl, yld, dQdP, K, tII_out


def _av_clamped(A):
    """av_clamped(A, Ic...) at every vertex: 0.25 (A[i0, j0] + A[ic, jc] + A[i0, jc] + A[ic, j0]) with clamped indices"""
    nx, ny = A.shape
    i0, ic = np.clip(np.arange(nx + 1) - 1, 0, nx - 1), np.clip(np.arange(nx + 1), 0, nx - 1)
    j0, jc = np.clip(np.arange(ny + 1) - 1, 0, ny - 1), np.clip(np.arange(ny + 1), 0, ny - 1)
    return 0.25 * (A[np.ix_(i0, j0)] + A[np.ix_(ic, jc)] + A[np.ix_(i0, jc)] + A[np.ix_(ic, j0)])


def _harm_clamped(A):
    nx, ny = A.shape
    i0, ic = np.clip(np.arange(nx + 1) - 1, 0, nx - 1), np.clip(np.arange(nx + 1), 0, nx - 1)
    j0, jc = np.clip(np.arange(ny + 1) - 1, 0, ny - 1), np.clip(np.arange(ny + 1), 0, ny - 1)
    return 4.0 / (1.0 / A[np.ix_(i0, j0)] + 1.0 / A[np.ix_(ic, jc)] + 1.0 / A[np.ix_(i0, jc)] + 1.0 / A[np.ix_(ic, j0)])


# ---------------------------------------------------------------- the four kernels
def compute_divV_strain(a, phi, _di):
    """compute_∇V! + compute_strain_rate! (VelocityKernels.jl:6-59)"""
    m = valid_masks(phi)
    _dx, _dy = _di
    Vx, Vy = a["Vx"], a["Vy"]
    dxi = (-Vx[:-1, 1:-1] + Vx[1:, 1:-1]) * _dx
    dyi = (-Vy[1:-1, :-1] + Vy[1:-1, 1:]) * _dy
    a["divV"][...] = np.where(m["c"], dxi + dyi, 0.0)
    d3 = a["divV"] / 3
    a["exx"][...] = np.where(m["c"], (Vx[1:, 1:-1] - Vx[:-1, 1:-1]) * _dx - d3, 0.0)
    a["eyy"][...] = np.where(m["c"], (Vy[1:-1, 1:] - Vy[1:-1, :-1]) * _dy - d3, 0.0)
    a["exy"][...] = np.where(m["v"], 0.5 * ((Vx[:, 1:] - Vx[:, :-1]) * _dy + (Vy[1:, :] - Vy[:-1, :]) * _dx), 0.0)


def update_stresses(a, phi, theta, lam, lamv, phases, dt, th, rel):
    """update_stresses_center_vertex! 2D (StressKernels.jl:2-170).  The vertex half reads the centre stresses before any centre is updated."""
    m = valid_masks(phi)
    # ---- vertex
    tijv = [_av_clamped(a["txx"]), _av_clamped(a["tyy"]), a["txy"].copy()]
    toijv = [_av_clamped(a["toxx"]), _av_clamped(a["toyy"]), a["toxy"]]
    eijv = [_av_clamped(a["exx"]), _av_clamped(a["eyy"]), a["exy"]]
    tn, ln, epl, yld, _, _, _ = _node_update(phases, a["phase_v"], _av_clamped(theta), tijv, toijv, eijv, _harm_clamped(a["eta"]), lamv,
                                             _av_clamped(a["EII_pl"]), dt, th, rel)
    v = m["v"]
    a["txy"][...] = np.where(v, tn[2], 0.0)                        # τxy += dτ at a valid vertex, zero at an invalid one
    lamv[...] = np.where(v, ln, lamv)
    a["eplxy"][...] = np.where(v, epl[2], a["eplxy"])
    # ---- centre
    exy = a["exy"]
    exyc = (exy[:-1, :-1] + exy[1:, :-1] + exy[:-1, 1:] + exy[1:, 1:]) / 4
    tij = [a["txx"].copy(), a["tyy"].copy(), a["txy_c"].copy()]
    eij = [a["exx"], a["eyy"], exyc]
    tn, ln, epl, yld, dQdP, K, tII = _node_update(phases, a["phase_c"], theta, tij, [a["toxx"], a["toyy"], a["toxy_c"]], eij, a["eta"], lam,
                                                  a["EII_pl"], dt, th, rel)
    c = m["c"]
    lam[...] = np.where(c, ln, lam)
    a["evol_pl"][...] = np.where(c, np.where(yld, -lam * dQdP, 0.0), 0.0)
    for k, q in (("txx", 0), ("tyy", 1), ("txy_c", 2)):
        a[k][...] = np.where(c, tn[q], 0.0)
    a["eplxx"][...] = np.where(c, epl[0], 0.0)
    a["eplyy"][...] = np.where(c, epl[1], 0.0)
    a["eplxy"][:-1, :-1][~c] = 0.0                                 # ε_pl[3][I...] = 0 at an invalid centre: the vertex array at the centre's index
    a["tII"][...] = np.where(c, tII, a["tII"])                     # not written at an invalid centre
    with np.errstate(invalid="ignore", divide="ignore"):
        a["eta_vep"][...] = np.where(c, tII * 0.5 * (1.0 / _sinv2(*eij)), 0.0)
        a["P"][...] = np.where(c, theta - np.where(np.isinf(K), 0.0, K * dt * lam * dQdP), 0.0)
    return yld


def compute_V(a, phi, etatau, eta_dtau, _di, fs_dt):
    """compute_V! with dt (VelocityKernels.jl:332-401); fs_dt = dt * free_surface"""
    m = valid_masks(phi)
    _dx, _dy = _di
    pc, pv = phi["center"], phi["vertex"]
    P, txx, tyy, txy = a["P"] * pc, a["txx"] * pc, a["tyy"] * pc, a["txy"] * pv
    fx, fy = a["fx"] * pc, a["fy"] * pc
    # x: i < nx - 1, all j
    R = -((-P[:-1] + P[1:]) * _dx) + (-txx[:-1] + txx[1:]) * _dx + (-txy[1:-1, :-1] + txy[1:-1, 1:]) * _dy - (fx[:-1] + fx[1:]) * 0.5
    ok = m["vx"][1:-1, :]
    a["Rx"][...] = np.where(ok, R, 0.0)
    Vx = a["Vx"][1:-1, 1:-1]
    Vx[...] = np.where(ok, Vx + R * eta_dtau / ((etatau[:-1] + etatau[1:]) * 0.5), 0.0)
    # y: all i, j < ny - 1
    Vy = a["Vy"][1:-1, 1:-1]
    corr = (Vy * ((fy[:, 1:] - fy[:, :-1]) * _dy)) * 1.0 * fs_dt
    R = (-((-P[:, :-1] + P[:, 1:]) * _dy) + (-tyy[:, :-1] + tyy[:, 1:]) * _dy + (-txy[:-1, 1:-1] + txy[1:, 1:-1]) * _dx
         - (fy[:, :-1] + fy[:, 1:]) * 0.5 + corr)
    ok = m["vy"][:, 1:-1]
    a["Ry"][...] = np.where(ok, R, 0.0)
    Vy[...] = np.where(ok, Vy + R * eta_dtau / ((etatau[:, :-1] + etatau[:, 1:]) * 0.5), 0.0)


# ---------------------------------------------------------------- unmasked pieces the driver shares with the multiphase solve!
def maxloc(eta):
    nx, ny = eta.shape
    out = np.full(eta.shape, -np.inf)
    for dj in (-1, 0, 1):
        jj = np.clip(np.arange(ny) + dj, 0, ny - 1)
        for di in (-1, 0, 1):
            ii = np.clip(np.arange(nx) + di, 0, nx - 1)
            out = np.maximum(out, eta[np.ix_(ii, jj)])
    return out


def compute_P(a, theta, etatau, K, G, dt, r, th):
    """compute_P! (PressureKernels.jl:47-106, phase form) with ητ in the η slot: RP and θ"""
    _Kdt, _Gdt, _dt = 1.0 / (K * dt), 1.0 / (G * dt), 1.0 / dt
    rhs = -a["divV"] + a["Q"] * _dt
    a["RP"][...] = -(theta - a["P0"]) * _Kdt + rhs
    psi = 1.0 / (1.0 / etatau + _Gdt) * r / th
    theta[...] = ((a["P0"] * _Kdt + rhs) * psi + theta) / (1.0 + _Kdt * psi)


def free_slip(a):
    """flow_bcs! with free slip on the four faces (boundaryconditions/free_slip.jl): tangential ghosts copy the interior"""
    a["Vx"][:, 0], a["Vx"][:, -1] = a["Vx"][:, 1], a["Vx"][:, -2]
    a["Vy"][0, :], a["Vy"][-1, :] = a["Vy"][1, :], a["Vy"][-2, :]


def solve_VS(a, phi, phases, pt, _di, dt, *, air_phase=0, iterMax, iterMin=100, nout, viscosity_cutoff=(-np.inf, np.inf), viscosity_relaxation=1.0e-2,
             λ_relaxation=0.2, free_surface=False, **_):
    """_solve_VS! (Stokes2D.jl:24-314), one block, free-slip velocity boundary conditions, strain_increment = false.  pt: (r, θ_dτ, ηdτ, ϵ_rel, ϵ_abs)"""
    r, th, eta_dtau, eps_rel, eps_abs = pt
    nx, ny = a["P"].shape
    nRx, nRy, nRP = np.sqrt((nx - 2) * (ny - 1)), np.sqrt((nx - 1) * (ny - 2)), np.sqrt(nx * ny)
    err_it1 = err = 1.0
    it = 0
    hist = dict(err_evo1=[], err_evo2=[], norm_Rx=[], norm_Ry=[], norm_divV=[])
    a["P0"][...] = a["P"]
    theta = a["P"].copy(order="F")
    lam, lamv = np.zeros((nx, ny), order="F"), np.zeros((nx + 1, ny + 1), order="F")
    for k in ("eplxx", "eplyy", "eplxy_c"):
        a[k][...] = 0.0
    if any(ph.get("density") is not None for ph in phases):
        compute_rhog(a, phases)
    compute_viscosity(a, phases, 1.0, viscosity_cutoff, air_phase)
    K = _ratio_sum([ph["Kb"] for ph in phases], a["phase_c"])
    G = _ratio_sum([ph["G"] for ph in phases], a["phase_c"])
    fs_dt = dt if free_surface else 0.0          # Inf * false == 0.0
    while it <= iterMax:
        with np.errstate(invalid="ignore", divide="ignore"):
            if iterMin < it and ((err / err_it1) < eps_rel or err < eps_abs):
                break
        etatau = maxloc(a["eta"])
        compute_divV_strain(a, phi, _di)          # compute_∇V!; the strain rates do not depend on compute_P!
        compute_P(a, theta, etatau, K, G, dt, r, th)
        compute_viscosity(a, phases, viscosity_relaxation, viscosity_cutoff, air_phase)
        update_stresses(a, phi, theta, lam, lamv, phases, dt, th, λ_relaxation)
        compute_V(a, phi, etatau, eta_dtau, _di, fs_dt)
        a["Ux"][...] = a["Vx"] * dt
        a["Uy"][...] = a["Vy"] * dt
        free_slip(a)
        it += 1
        if it % nout == 0 and it > 1:
            e = (np.sqrt(np.sum(a["Rx"][phi["Vx"][1:-1, :] > 0] ** 2)) / nRx, np.sqrt(np.sum(a["Ry"][phi["Vy"][:, 1:-1] > 0] ** 2)) / nRy,
                 np.sqrt(np.sum(a["RP"][phi["center"] > 0] ** 2)) / nRP)
            err = max(e)
            for k, v in zip(("norm_Rx", "norm_Ry", "norm_divV"), e):
                hist[k].append(v)
            hist["err_evo1"].append(err)
            hist["err_evo2"].append(it)
            err_it1 = max(hist["norm_Rx"][0], hist["norm_Ry"][0], hist["norm_divV"][0])
            if np.isnan(err):
                raise FloatingPointError("NaN(s)")
    # epilogue (Stokes2D.jl:289-304)
    Vx, Vy = a["Vx"], a["Vy"]
    a["omega_xy"][...] = 0.5 * ((-Vy[:-1, :] + Vy[1:, :]) * _di[0] - (-Vx[:, :-1] + Vx[:, 1:]) * _di[1])
    s2c = lambda v: 0.25 * (v[:-1, :-1] + v[1:, :-1] + v[:-1, 1:] + v[1:, 1:])
    a["exy_c"][...] = s2c(a["exy"])
    a["eplxy_c"][...] = s2c(a["eplxy"])
    if "dexy_c" in a and "dexy" in a:
        a["dexy_c"][...] = s2c(a["dexy"])
    v = a["eplxy"]
    sq = 0.25 * (v[:-1, :-1] ** 2 + v[1:, :-1] ** 2 + v[:-1, 1:] ** 2 + v[1:, 1:] ** 2)
    a["EII_pl"][...] += np.sqrt(0.5 * (a["eplxx"] ** 2 + a["eplyy"] ** 2) + sq) * dt
    a["EVol_pl"][...] += dt * a["evol_pl"]
    for k in ("xx", "yy", "xy", "xy_c"):
        a["to" + k][...] = a["t" + k]
    hist["iter"] = it
    return hist


def randomize(s, seed=4):
    """the `_randomize` recipe of tests/test_gpu_vep2d.py: every input of the stress kernel non-trivial, yielding and non-yielding nodes, mixed phase ratios"""
    rng = np.random.default_rng(seed)
    a = s.arrays
    for k in ("P", "exx", "eyy", "exy", "txx", "tyy", "txy", "txy_c", "toxx", "toyy", "toxy", "toxy_c"):
        a[k][...] = rng.uniform(-2.0, 2.0, size=a[k].shape)
    a["eta"][...] = 10.0 ** rng.uniform(-1.0, 0.5, size=a["eta"].shape)
    for k in ("phase_c", "phase_v"):
        r = rng.uniform(0.0, 1.0, size=a[k].shape[1:])
        r[rng.uniform(size=r.shape) < 0.3] = 0.0
        r[rng.uniform(size=r.shape) < 0.3] = 1.0
        a[k][0], a[k][1] = r, 1.0 - r


def random_phi(ni, seed=7):
    """a rock ratio of exact zeros, exact ones and fractions, so that every predicate is true and false somewhere"""
    rng = np.random.default_rng(seed)
    phi = rock_ratio(*ni)
    for k, zero in (("center", 0.15), ("vertex", 0.15), ("Vx", 0.25), ("Vy", 0.25)):
        x = rng.uniform(0.05, 0.95, size=phi[k].shape)
        u = rng.uniform(size=x.shape)
        x[u < zero] = 0.0
        x[u > 0.6] = 1.0
        phi[k][...] = x
    return phi


def pt_tuple(pt):
    return (pt.r, pt.θ_dτ, pt.ηdτ, pt.ϵ_rel, pt.ϵ_abs)
