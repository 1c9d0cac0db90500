"""NumPy restatement of the 3D DYREL solver (csrc/dyrel3d.hip), dtype-generic like tests/_dyrel.py (float64, or np.longdouble for the rounding-spread bound).

Restated from the reference's text: the allocator DYREL(ni::NTuple{3}) (src/DYREL/constructors.jl:61-111), velocity_dofs / pressure_dof / compute_λminV!
(solver.jl:329-365), compute_∇V_strain_rate_RP! 3D (velocity_kernels.jl:242-322), compute_DR_residual_update_V! 3D (:729-828), the N-dimensional update_α_β! /
update_dτV_α_β! (Gershgorin.jl:171-310), compute_bulk_viscosity_and_penalty! (constructors.jl:230-254), the local law for a tuple of any length
(stress_kernels.jl:224-315) and the loop _solve_DYREL! (solver.jl:44-294).
No reference text, the forms include/jrx.h states: the stress kernel (compute_stress_viscosity_DRYEL! laid out as update_stresses_center_vertex_ps! 3D, clamped
gathers of src/stokes/StressKernels.jl:604-733, which tests/_variational_stokes3d.py already restates and this file imports), the eigenvalue bound
(Gershgorin_Stokes2D_SchurComplement! one dimension up) and the shear differences of the momentum residuals (the index triples of src/stokes/VelocityKernels.jl:215-238;
the reference's _d_yi / _d_zi of MiniKernels.jl:53-55 read one plane past τxy).

The local law of tests/_dyrel.py takes exactly three components (its invariant and its gradients are written out), so it is restated here for any count; with
three components every operation and its order are those of tests/_dyrel.py.  Arrays are Julia-shaped (x first), indices 0-based, names as jrx_vep3d_fields plus
lam, lamv_yz / _xz / _xy, dPpsi; the DYREL struct is a dict with the names of jrx_dyrel3d_fields.
"""
import numpy as np

import _dyrel as dy2
from _variational_stokes3d import CEN, EDGES, OTH, _av4, _harm4, _s2c, _terms

astype, compute_RP, damped_update_V, _ratio_sum, _T = dy2.astype, dy2.compute_RP, dy2.damped_update_V, dy2._ratio_sum, dy2._T

COMP = "xyz"
DYREL_CENTER = ("gamma_eff", "etab", "P_num")
DYREL_STAG = ("D{}", "lmaxV{}", "dV{}dtau", "dtauV{}", "dV{}", "betaV{}", "cV{}", "alphaV{}", "R{}0")


def stag_shape(ni, d):
    return tuple(n - (1 if q == d else 0) for q, n in enumerate(ni))


def new_dyrel(ni, dtype=np.float64):
    """DYREL(ni::NTuple{3}) (constructors.jl:61-111): zero arrays"""
    d = {k: np.zeros(ni, dtype=dtype, order="F") for k in DYREL_CENTER}
    for q, c in enumerate(COMP):
        d.update({k.format(c): np.zeros(stag_shape(ni, q), dtype=dtype, order="F") for k in DYREL_STAG})
    return d


def velocity_dofs(ng):
    """velocity_dofs(Val(3)) (solver.jl:351-357) for the global grid size ng"""
    return tuple(int(np.prod([n - 2 if q == d else n - 1 for q, n in enumerate(ng)])) for d in range(3))


def pressure_dof(ng):
    return int(np.prod(ng))


def edge_shape(ni, T):
    return tuple(n + (1 if d != T else 0) for d, n in enumerate(ni))


VEP_CENTER = ("P", "P0", "divV", "Q", "exx", "eyy", "ezz", "eyz_c", "exz_c", "exy_c", "eplxx", "eplyy", "eplzz", "eplyz_c", "eplxz_c", "eplxy_c", "txx", "tyy", "tzz",
              "tyz_c", "txz_c", "txy_c", "tII", "toxx", "toyy", "tozz", "toyz_c", "toxz_c", "toxy_c", "eta", "eta_vep", "EII_pl", "evol_pl", "EVol_pl", "fx", "fy", "fz",
              "RP", "lam", "dPpsi")
VEP_EDGE = ("e{}", "epl{}", "t{}", "to{}", "omega_{}", "lamv_{}")


def alloc_state(ni, nphase, dtype=np.float64):
    nx, ny, nz = ni
    a = {k: np.zeros(ni, dtype=dtype, order="F") for k in VEP_CENTER}
    for T, name in enumerate(EDGES):
        a.update({k.format(name): np.zeros(edge_shape(ni, T), dtype=dtype, order="F") for k in VEP_EDGE})
        a["phase_" + name] = np.zeros((nphase,) + edge_shape(ni, T), dtype=dtype, order="F")
    a.update(Vx=np.zeros((nx + 1, ny + 2, nz + 2), dtype=dtype, order="F"), Vy=np.zeros((nx + 2, ny + 1, nz + 2), dtype=dtype, order="F"),
             Vz=np.zeros((nx + 2, ny + 2, nz + 1), dtype=dtype, order="F"), phase_c=np.zeros((nphase,) + tuple(ni), dtype=dtype, order="F"))
    for q, c in enumerate(COMP):
        a["R" + c] = np.zeros(stag_shape(ni, q), dtype=dtype, order="F")
    return a


# ---------------------------------------------------------------- velocity_kernels.jl:242-322
def strain_rate_RP(a, d, _di, dt, do_strain_rate=True):
    """compute_∇V_strain_rate_RP! 3D: the six strain rates (do_strain_rate) and R.RP; ∇V is not stored"""
    Vx, Vy, Vz = a["Vx"], a["Vy"], a["Vz"]
    T = _T(Vx)
    _dx, _dy, _dz, dt = T(_di[0]), T(_di[1]), T(_di[2]), T(dt)
    nx, ny, nz = a["P"].shape
    dVx_dx = (Vx[1:, 1:-1, 1:-1] - Vx[:-1, 1:-1, 1:-1]) * _dx
    dVy_dy = (Vy[1:-1, 1:, 1:-1] - Vy[1:-1, :-1, 1:-1]) * _dy
    dVz_dz = (Vz[1:-1, 1:-1, 1:] - Vz[1:-1, 1:-1, :-1]) * _dz
    div = dVx_dx + dVy_dy + dVz_dz
    if do_strain_rate:
        div_third = div * (T(1) / T(3))
        a["exx"][...], a["eyy"][...], a["ezz"][...] = dVx_dx - div_third, dVy_dy - div_third, dVz_dz - div_third
        a["eyz"][...] = T(0.5) * (_dz * (Vy[1:nx + 1, :, 1:] - Vy[1:nx + 1, :, :-1]) + _dy * (Vz[1:nx + 1, 1:, :] - Vz[1:nx + 1, :-1, :]))
        a["exz"][...] = T(0.5) * (_dz * (Vx[:, 1:ny + 1, 1:] - Vx[:, 1:ny + 1, :-1]) + _dx * (Vz[1:, 1:ny + 1, :] - Vz[:-1, 1:ny + 1, :]))
        a["exy"][...] = T(0.5) * (_dy * (Vx[:, 1:, 1:nz + 1] - Vx[:, :-1, 1:nz + 1]) + _dx * (Vy[1:, :, 1:nz + 1] - Vy[:-1, :, 1:nz + 1]))
    with np.errstate(invalid="ignore", divide="ignore"):
        a["RP"][...] = compute_RP(a["P"], a["P0"], div, a["Q"], d["etab"], dt)
    return div


# ---------------------------------------------------------------- stress_kernels.jl:224-315, any number of components
def sinv(t):
    """second_invariant of a 3-tuple (xx, yy, xy) or a 6-tuple (xx, yy, zz, yz, xz, xy)"""
    if len(t) == 3:
        return np.sqrt(0.5 * (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    return np.sqrt(0.5 * (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) + t[3] * t[3] + t[4] * t[4] + t[5] * t[5])


def _phase_local_stress(eij, toij, eta, P, lam, rel, ph, dt, EII):
    """_compute_local_stress for one phase over whole arrays; returns the 2 N + 5 outputs, the trial F (NaN where the early return was taken) and the yield mask"""
    T = _T(eta)
    N = len(eij)
    NN = 2 if N == 3 else 3
    G, Kb, dt, rel = T(ph["G"]), T(ph["Kb"]), T(dt), T(rel)
    ispl = ph.get("C") is not None
    eta_reg = T(ph.get("eta_vp", 0.0)) if ispl else T(0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        eta_ve = (1 / (1 / eta + 1 / (G * dt))) if np.isinf(G) else (eta * G * dt) / (eta + G * dt)
        inv_2Gdt = 1 / (2 * G * dt)
        eff = [e + t * inv_2Gdt for e, t in zip(eij, toij)]
        eII = sinv(eff)
        tij = [2 * eta_ve * e for e in eff]
        tII = sinv(tij)
        if ispl:
            C = dy2._soften(ph.get("softening_C"), EII, T(ph["C"]))
            deg = np.arctan(T(1)) / T(45)
            sin0, cos0 = np.sin(T(ph["phi_deg"]) * deg), np.cos(T(ph["phi_deg"]) * deg)
            if ph.get("softening_phi") is not None:
                phi = dy2._soften(ph["softening_phi"], EII, T(ph["phi_deg"]))
                sinphi, cosphi = np.sin(phi * deg), np.cos(phi * deg)
            else:
                sinphi, cosphi = sin0, cos0
            F = tII - cosphi * C - sinphi * P
            dQdt = [T(0.5) * tij[s] / tII for s in range(NN)] + [T(0.5) * (tij[s] / tII) for s in range(NN, N)]
            dQdP, dFdP = -np.sin(T(ph.get("psi_deg", 0.0)) * deg), -sin0
        else:
            F = tII
            dQdt = [np.zeros_like(eta)] * N
            dQdP, dFdP = T(0.0), T(0.0)
        yields = (F >= 0) if ispl else np.zeros(eta.shape, dtype=bool)
        bulk = T(0.0) if np.isinf(Kb) else Kb * dt * dFdP * dQdP
        lam_new = F / (eta_ve + eta_reg + bulk)
        lam_o = np.where(yields, rel * lam_new + (1 - rel) * lam, T(0.0))
        evol = np.where(yields, -lam_o * dQdP, T(0.0))
        pos = lam_o > 0
        epl = [np.where(pos, lam_o * g, T(0.0)) for g in dQdt]
        tij = [np.where(pos, t - T(2.0) * eta_ve * e, t) for t, e in zip(tij, epl)]
        tII = np.where(pos, sinv(tij), tII)
        dP = np.where(pos, T(0.0) if dQdP == 0 else -lam_o * dQdP * Kb * dt, T(0.0))
        eta_vep = tII * T(0.5) * (1 / sinv(eij))
    z = eII == 0
    out = tij + epl + [tII, lam_o, dP, eta_vep, evol]
    out = [np.where(z, T(0.0), x) for x in out]
    out[2 * N + 3] = np.where(z, eta, out[2 * N + 3])
    return out, np.where(z, np.nan, F), yields & ~z


def local_stress(eij, toij, eta, P, lam, rel, phases, ratio, dt, EII):
    """compute_local_stress: Σ over the phases of ratio .* _compute_local_stress.  Outputs: τ (N), ε_pl (N), τII, λ, ΔPψ, η_vep, ε_vol_pl"""
    T = _T(eta)
    acc, Fs = None, []
    for q, ph in enumerate(phases):
        r = ratio[q]
        out, F, y = _phase_local_stress(eij, toij, eta, P, lam, rel, ph, dt, EII)
        with np.errstate(invalid="ignore"):
            v = [np.where(r == 0, T(0.0), r * x) for x in out]
        acc = v if acc is None else [p + c for p, c in zip(acc, v)]
        if ph.get("C") is not None:
            Fs.append((q, np.where(r == 0, np.nan, F), y & (r != 0)))
    return acc, Fs


def visc_invariant6(t):
    """the invariant of _update_τII_viscosity with the allzero guard over six components, spread as compute_viscosity! 3D spreads it (Viscosity.jl:481-492)"""
    T = _T(t[0])
    zero = np.ones(t[0].shape, dtype=bool)
    for x in t:
        zero &= x == 0
    a0 = np.where(zero, T(np.finfo(np.float64).eps), T(0.0))
    return sinv([t[0] + a0, t[1] + -a0 * T(0.5), t[2] + -a0 * T(0.5), t[3], t[4], t[5]])


def edge_gather(a, ni, T):
    """what an edge of family T gathers (StressKernels.jl:705-733 and siblings): η, P, EII_pl, ε (6), τ_o (6)"""
    cen = lambda A: _av4(_terms(A, ni, T, CEN[T]))
    eij = [cen(a["exx"]), cen(a["eyy"]), cen(a["ezz"]), None, None, None]
    toij = [cen(a["toxx"]), cen(a["toyy"]), cen(a["tozz"]), None, None, None]
    for s, name in enumerate(EDGES):
        if s == T:
            eij[3 + s], toij[3 + s] = a["e" + name], a["to" + name]
        else:
            eij[3 + s] = _av4(_terms(a["e" + name], ni, T, OTH[(T, s)]))
            toij[3 + s] = _av4(_terms(a["to" + name], ni, T, OTH[(T, s)]))
    return _harm4(_terms(a["eta"], ni, T, CEN[T])), cen(a["P"]), cen(a["EII_pl"]), eij, toij


def stress_viscosity(a, d, phases, rel, dt, nu, cutoff, linear_viscosity, Tk=0.0, diag=None):
    """the 3D stress kernel in the form include/jrx.h states.  The edges read η as it was before the call; everything else a node writes it reads at its own
    index only, so whole-array evaluation from the old values is the kernel's result.  diag (a dict) receives the trial F and yield masks."""
    ni = a["P"].shape
    T = _T(a["P"])
    nu_, lo, hi = T(nu), T(cutoff[0]), T(cutoff[1])
    Fe = {}
    edge_out = {}
    for Tf, name in enumerate(EDGES):
        etav, Pv, EIIv, eij, toij = edge_gather(a, ni, Tf)
        out, Fv = local_stress(eij, toij, etav, Pv, a["lamv_" + name], rel, phases, a["phase_" + name], dt, EIIv)
        edge_out[name] = (out[3 + Tf], out[6 + 3 + Tf], out[13])
        Fe[name] = Fv
    # centres
    g = _s2c(a["eyz"], a["exz"], a["exy"])
    eij = [a["exx"], a["eyy"], a["ezz"]] + [(t[0] + t[1] + t[2] + t[3]) / 4 for t in g]
    toij = [a["toxx"], a["toyy"], a["tozz"], a["toyz_c"], a["toxz_c"], a["toxy_c"]]
    eta_old = a["eta"].copy()
    out, Fc = local_stress(eij, toij, eta_old, a["P"], a["lam"], rel, phases, a["phase_c"], dt, a["EII_pl"])
    for k, v in zip(("txx", "tyy", "tzz", "tyz_c", "txz_c", "txy_c", "eplxx", "eplyy", "eplzz"), out[:9]):
        a[k][...] = v
    a["tII"][...], a["lam"][...], a["dPpsi"][...], a["eta_vep"][...], a["evol_pl"][...] = out[12], out[13], out[14], out[15], out[16]
    d["P_num"][...] = d["gamma_eff"] * a["RP"] + out[14]          # θc = γ_eff RP + ΔPψ
    if not linear_viscosity:
        e = dy2.phase_viscosity_tauII(phases, a["phase_c"], visc_invariant6(out[:6]), Tk, a["P"])
        e = (1 - nu_) * eta_old + nu_ * e
        a["eta"][...] = np.minimum(np.maximum(e, lo), hi)
    for name, (t, epl, lv) in edge_out.items():
        a["t" + name][...], a["epl" + name][...], a["lamv_" + name][...] = t, epl, lv
    if diag is not None:
        diag.update(Fc=Fc, **{"F" + name: Fe[name] for name in EDGES})


# ---------------------------------------------------------------- velocity_kernels.jl:441-477, 729-828 with the shear differences include/jrx.h states
def _momentum(a, th, _di):
    T = _T(a["P"])
    _dx, _dy, _dz = T(_di[0]), T(_di[1]), T(_di[2])
    P, tyz, txz, txy = a["P"], a["tyz"], a["txz"], a["txy"]
    dxa = lambda A: (-A[:-1] + A[1:]) * _dx
    dya = lambda A: (-A[:, :-1] + A[:, 1:]) * _dy
    dza = lambda A: (-A[:, :, :-1] + A[:, :, 1:]) * _dz
    Rx = (dxa(a["txx"]) + (-txy[1:-1, :-1, :] + txy[1:-1, 1:, :]) * _dy + (-txz[1:-1, :, :-1] + txz[1:-1, :, 1:]) * _dz - dxa(P) - dxa(th)
          - (a["fx"][:-1] + a["fx"][1:]) * T(0.5))
    Ry = (dya(a["tyy"]) + (-txy[:-1, 1:-1, :] + txy[1:, 1:-1, :]) * _dx + (-tyz[:, 1:-1, :-1] + tyz[:, 1:-1, 1:]) * _dz - dya(P) - dya(th)
          - (a["fy"][:, :-1] + a["fy"][:, 1:]) * T(0.5))
    Rz = (dza(a["tzz"]) + (-txz[:-1, :, 1:-1] + txz[1:, :, 1:-1]) * _dx + (-tyz[:, :-1, 1:-1] + tyz[:, 1:, 1:-1]) * _dy - dza(P) - dza(th)
          - (a["fz"][:, :, :-1] + a["fz"][:, :, 1:]) * T(0.5))
    return Rx, Ry, Rz


def ph_residual(a, _di):
    a["Rx"][...], a["Ry"][...], a["Rz"][...] = _momentum(a, a["dPpsi"], _di)


def dr_residual_update_V(a, d, _di):
    R = _momentum(a, d["P_num"], _di)
    for c, Rc in zip(COMP, R):
        with np.errstate(invalid="ignore", divide="ignore"):
            Rc = Rc / d["D" + c]
        a["R" + c][...] = Rc
        d[f"dV{c}dtau"][...], dV = damped_update_V(d[f"dV{c}dtau"], Rc, d["alphaV" + c], d["betaV" + c], d["dtauV" + c])
        a["V" + c][1:-1, 1:-1, 1:-1] += dV


def flow_bcs(a, free_slip=True, no_slip=False):
    """flow_bcs! with one kind on the six faces, one pass per dimension over whole planes, in the reference's source order: no slip x, y, z
    (no_slip.jl:20-54), free slip y, z, x (free_slip.jl:15-70)"""
    V = [a["Vx"], a["Vy"], a["Vz"]]

    def plane(A, dim, idx):
        s = [slice(None)] * 3
        s[dim] = idx
        return tuple(s)
    if no_slip:
        for dim in (0, 1, 2):
            for c in range(3):
                A = V[c]
                if c == dim:
                    A[plane(A, dim, 0)] = 0.0
                    A[plane(A, dim, -1)] = 0.0
                else:
                    A[plane(A, dim, 0)] = -A[plane(A, dim, 1)]
                    A[plane(A, dim, -1)] = -A[plane(A, dim, -2)]
    elif free_slip:
        for dim in (1, 2, 0):
            for c in range(3):
                if c != dim:
                    A = V[c]
                    A[plane(A, dim, 0)] = A[plane(A, dim, 1)]
                    A[plane(A, dim, -1)] = A[plane(A, dim, -2)]


# ---------------------------------------------------------------- constructors.jl:230-254, the 3D bound, Gershgorin.jl:171-310
def bulk_viscosity_and_penalty(a, d, phases, gamma_fact, dt):
    dy2.bulk_viscosity_and_penalty(a, d, phases, gamma_fact, dt)          # written for arrays of any rank


def _gersh(gP, gM, eP, eM, a1P, a1M, a2P, a2M, _dn, _d1, _d2):
    T = _T(eP)
    c43, c23 = T(4) / T(3), T(2) / T(3)
    _dn2, _d12, _d22, _dnd1, _dnd2 = _dn * _dn, _d1 * _d1, _d2 * _d2, _dn * _d1, _dn * _d2
    D = (a1P * _d1 + a1M * _d1) * _d1 + (a2P * _d2 + a2M * _d2) * _d2 + (gP * _dn + gM * _dn + c43 * (eP * _dn + eM * _dn)) * _dn
    Cnn = (np.abs(a1P * _d12) + np.abs(a1M * _d12) + np.abs(a2P * _d22) + np.abs(a2M * _d22) + np.abs((gP + c43 * eP) * _dn2) + np.abs((gM + c43 * eM) * _dn2)
           + np.abs(D))
    Cn1 = (np.abs((gP - c23 * eP + a1P) * _dnd1) + np.abs((gP - c23 * eP + a1M) * _dnd1) + np.abs((gM + a1P - c23 * eM) * _dnd1)
           + np.abs((gM + a1M - c23 * eM) * _dnd1))
    Cn2 = (np.abs((gP - c23 * eP + a2P) * _dnd2) + np.abs((gP - c23 * eP + a2M) * _dnd2) + np.abs((gM + a2P - c23 * eM) * _dnd2)
           + np.abs((gM + a2M - c23 * eM) * _dnd2))
    return D, (1 / D) * (Cnn + Cn1 + Cn2)


def gershgorin(a, d, phases, di, dt):
    """the 3D eigenvalue bound in the form include/jrx.h states: Gershgorin_Stokes2D_SchurComplement! one dimension up"""
    eta, gam = a["eta"], d["gamma_eff"]
    ni = eta.shape
    T = _T(eta)
    dt = T(dt)
    _dx, _dy, _dz = 1 / T(di[0]), 1 / T(di[1]), 1 / T(di[2])
    Gs = [ph["G"] for ph in phases]
    with np.errstate(invalid="ignore", divide="ignore"):
        ve = lambda e, G: 1 / (1 / e + 1 / (G * dt))
        c = ve(eta, _ratio_sum(Gs, a["phase_c"]))
        yz, xz, xy = (ve(_harm4(_terms(eta, ni, Tf, CEN[Tf])), _ratio_sum(Gs, a["phase_" + name])) for Tf, name in enumerate(EDGES))
        d["Dx"][...], d["lmaxVx"][...] = _gersh(gam[1:], gam[:-1], c[1:], c[:-1], xy[1:-1, 1:, :], xy[1:-1, :-1, :], xz[1:-1, :, 1:], xz[1:-1, :, :-1], _dx, _dy, _dz)
        d["Dy"][...], d["lmaxVy"][...] = _gersh(gam[:, 1:], gam[:, :-1], c[:, 1:], c[:, :-1], yz[:, 1:-1, 1:], yz[:, 1:-1, :-1], xy[1:, 1:-1, :], xy[:-1, 1:-1, :],
                                                _dy, _dz, _dx)
        d["Dz"][...], d["lmaxVz"][...] = _gersh(gam[:, :, 1:], gam[:, :, :-1], c[:, :, 1:], c[:, :, :-1], xz[1:, :, 1:-1], xz[:-1, :, 1:-1], yz[:, 1:, 1:-1],
                                                yz[:, :-1, 1:-1], _dz, _dx, _dy)


def update_alpha_beta(d):
    for c in COMP:
        dtau, cV = d[f"dtauV{c}"], d[f"cV{c}"]
        with np.errstate(invalid="ignore", divide="ignore"):
            d[f"betaV{c}"][...] = 2 * dtau / (2 + cV * dtau)
            d[f"alphaV{c}"][...] = (2 - cV * dtau) / (2 + cV * dtau)


def update_dtauV_alpha_beta(d, CFL):
    for c in COMP:
        with np.errstate(invalid="ignore", divide="ignore"):
            d[f"dtauV{c}"][...] = 2 / np.sqrt(d[f"lmaxV{c}"]) * _T(d["Dx"])(CFL)
    update_alpha_beta(d)


def dyrel_init(a, d, phases, di, dt, CFL=0.99, gamma_fact=20.0):
    """DYREL! (constructors.jl:178-190) with the 3D bound"""
    bulk_viscosity_and_penalty(a, d, phases, gamma_fact, dt)
    gershgorin(a, d, phases, di, dt)
    update_dtauV_alpha_beta(d, CFL)


def compute_viscosity(a, phases, nu, cutoff, Tk=0.0):
    """compute_viscosity! with the strain-rate invariant, LinearViscous laws (the invariant is not read); centres only in 3D"""
    T = _T(a["eta"])
    e = dy2.phase_viscosity_tauII(phases, a["phase_c"], np.zeros(a["eta"].shape, dtype=a["eta"].dtype), Tk, 0.0)
    e = e * T(nu) + a["eta"] * (1 - T(nu))
    a["eta"][...] = np.minimum(np.maximum(e, T(cutoff[0])), T(cutoff[1]))


def compute_rhog(a, phases):
    if any(ph["density"].get("kind", "constant") != "constant" for ph in phases):
        raise NotImplementedError("the restatement knows ConstantDensity")
    a["fz"][...] = _ratio_sum([ph["density"]["rho0"] for ph in phases], a["phase_c"]) * _T(a["fz"])(phases[0].get("g", 0.0))


def lambda_min(a, d):
    """compute_λminV! (solver.jl:359-365), three components"""
    num = den = None
    for c in COMP:
        d["dV" + c][...] = d[f"dV{c}dtau"] * d["betaV" + c] * d["dtauV" + c]
        n, q = np.sum(d["dV" + c] * (a["R" + c] - d[f"R{c}0"])), np.sum(d["dV" + c] ** 2)
        num, den = (n, q) if num is None else (num + n, den + q)
    return abs(num) / den


def _nrm(x):
    return float(np.sqrt(np.sum(x * x)))


def ph_norms(a):
    ni = a["P"].shape
    dofs = velocity_dofs(ni)
    return tuple(_nrm(a["R" + c]) / np.sqrt(dofs[q]) for q, c in enumerate(COMP)), _nrm(a["RP"]) / np.sqrt(pressure_dof(ni))


def solve_DYREL(a, d, phases, di, dt, *, eps=1.0e-6, CFL=0.99, c_fact=0.5, gamma_fact=20.0, viscosity_cutoff=(-np.inf, np.inf), viscosity_relaxation=1.0e-2,
                λ_relaxation_DR=1, λ_relaxation_PH=1, iterMax=50.0e3, total_iterMax=50.0e3, nout=100, rel_drop=1.0e-2, linear_viscosity=False,
                free_slip=True, no_slip=False, Tk=0.0, itPH_max=1000, **_):
    """_solve_DYREL! (solver.jl:44-294) on a 3D grid, one block.  Returns the four histories and the iteration counts."""
    ni = a["P"].shape
    dofs = velocity_dofs(ni)
    _di = tuple(1.0 / x for x in di)
    EPS = float(np.finfo(np.float64).eps)
    a["P0"][...] = a["P"]
    for k in ("eplxx", "eplyy", "eplzz", "eplyz_c", "eplxz_c", "eplxy_c", "lam", "lamv_yz", "lamv_xz", "lamv_xy"):
        a[k][...] = 0.0
    err_min, iteration, itPH_done = np.inf, 0, 0
    errV0, errPt0, errV00 = (1.0,) * 3, 1.0, 1.0
    hist = dict(err_evo_it=[], err_evo_V=[], err_evo_P=[], err_evo_tot=[])
    compute_viscosity(a, phases, 1.0, viscosity_cutoff, Tk)
    if any(ph.get("density") is not None for ph in phases):
        compute_rhog(a, phases)
    dyrel_init(a, d, phases, di, dt, CFL, gamma_fact)
    for itPH in range(1, itPH_max + 1):
        itPH_done = itPH
        strain_rate_RP(a, d, _di, dt, True)
        stress_viscosity(a, d, phases, λ_relaxation_PH, dt, viscosity_relaxation, viscosity_cutoff, linear_viscosity, Tk)
        ph_residual(a, _di)
        errV, errPt = ph_norms(a)
        if itPH == 1:
            errV0 = tuple(x + EPS for x in errV)
            errPt0 = errPt + EPS
        if itPH == 2:
            errPt0 = errPt + EPS
        err = max(tuple(min(e / e0, e) for e, e0 in zip(errV, errV0)) + (min(errPt / errPt0, errPt),))
        if np.isnan(err):
            raise FloatingPointError("NaN detected in outer loop")
        if err < eps:
            break
        if err > err_min * 1.05:
            rel_drop = max(rel_drop * 0.1, 1.0e-3)
        if err_min > err:
            err_min = err
        eps_vel = err * rel_drop
        itPT = 0
        while err > eps_vel and itPT <= iterMax:
            itPT += 1
            iteration += 1
            if iteration % nout == 0:
                for c in COMP:
                    d[f"R{c}0"][...] = a["R" + c]
            strain_rate_RP(a, d, _di, dt, True)
            stress_viscosity(a, d, phases, λ_relaxation_DR, dt, viscosity_relaxation, viscosity_cutoff, linear_viscosity, Tk)
            dr_residual_update_V(a, d, _di)
            flow_bcs(a, free_slip, no_slip)
            if iteration % nout == 0:
                eV = tuple(_nrm(d["D" + c] * a["R" + c]) / np.sqrt(dofs[q]) for q, c in enumerate(COMP))
                if iteration == nout:
                    errV00 = max(eV) + EPS
                err = max(e / errV00 for e in eV)
                if np.isnan(err):
                    raise FloatingPointError("NaN detected in inner loop")
                hist["err_evo_tot"].append(err)
                hist["err_evo_V"].append(err)
                hist["err_evo_P"].append(errPt / errPt0)
                hist["err_evo_it"].append(float(iteration))
                cV = 2 * np.sqrt(lambda_min(a, d)) * _T(d["cVx"])(c_fact)
                for c in COMP:
                    d["cV" + c][...] = cV
                gershgorin(a, d, phases, di, dt)
                update_dtauV_alpha_beta(d, CFL)
        strain_rate_RP(a, d, _di, dt, False)
        a["P"][...] += d["gamma_eff"] * a["RP"]
        if iteration > total_iterMax:
            break
    epilogue(a, _di, dt)
    hist.update(iter=iteration, itPH=itPH_done, errV0=errV0, errPt0=errPt0)
    return hist


def epilogue(a, _di, dt):
    """solver.jl:269-290 on a 3D grid: P += ΔPψ, ∇V, vorticity on the edges, shear2center! of ε and ε_pl, accumulate_tensor!, accumulate_vol!, τ_o = τ"""
    T = _T(a["P"])
    _dx, _dy, _dz, dt = T(_di[0]), T(_di[1]), T(_di[2]), T(dt)
    nx, ny, nz = a["P"].shape
    a["P"][...] += a["dPpsi"]
    Vx, Vy, Vz = a["Vx"], a["Vy"], a["Vz"]
    a["divV"][...] = ((-Vx[:-1, 1:-1, 1:-1] + Vx[1:, 1:-1, 1:-1]) * _dx + (-Vy[1:-1, :-1, 1:-1] + Vy[1:-1, 1:, 1:-1]) * _dy
                      + (-Vz[1:-1, 1:-1, :-1] + Vz[1:-1, 1:-1, 1:]) * _dz)
    a["omega_yz"][...] = T(0.5) * ((-Vz[:nx, :ny + 1, :] + Vz[:nx, 1:ny + 2, :]) * _dy - (-Vy[:nx, :, :nz + 1] + Vy[:nx, :, 1:nz + 2]) * _dz)
    a["omega_xz"][...] = T(0.5) * ((-Vx[:, :ny, :nz + 1] + Vx[:, :ny, 1:nz + 2]) * _dz - (-Vz[:nx + 1, :ny, :] + Vz[1:nx + 2, :ny, :]) * _dx)
    a["omega_xy"][...] = T(0.5) * ((-Vy[:nx + 1, :, :nz] + Vy[1:nx + 2, :, :nz]) * _dx - (-Vx[:, :ny + 1, :nz] + Vx[:, 1:ny + 2, :nz]) * _dy)
    for pre in ("e", "epl"):
        for name, t in zip(EDGES, _s2c(a[pre + "yz"], a[pre + "xz"], a[pre + "xy"])):
            a[pre + name + "_c"][...] = T(0.25) * (t[0] + t[1] + t[2] + t[3])
    sq = [T(0.25) * (t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3]) for t in _s2c(a["eplyz"], a["eplxz"], a["eplxy"])]
    a["EII_pl"][...] += np.sqrt(T(0.5) * (a["eplxx"] ** 2 + a["eplyy"] ** 2 + a["eplzz"] ** 2) + sq[0] + sq[1] + sq[2]) * dt
    a["EVol_pl"][...] += dt * a["evol_pl"]
    for k in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        a["to" + k][...] = a["t" + k]


# ---------------------------------------------------------------- set-ups shared by the tests
def _locations(ni):
    v = [np.linspace(0.0, 1.0, n + 1) for n in ni]
    c = [(np.arange(n) + 0.5) / n for n in ni]
    return v, c


def shearband_state(nx, ny, nz, psi_deg=0.0, C_cos=1.6, radius=0.1, axis=None):
    """the shear band of tests/_dyrel.py in the unit cube: matrix G = 1, inclusion G = 0.5 (a sphere of `radius` at the centre, or with `axis` = 0 / 1 / 2 a
    cylinder along that axis: the plane-strain extrusion of the 2D set-up), η = 1, Kb = 5, DruckerPrager_regularised(C = C_cos / cos 30°, ϕ = 30°, η_vp = 1e-2, Ψ),
    pure shear on the boundary -- extension along the first in-plane axis, shortening along the second, nothing along `axis` (default y) -- zero interior
    velocity, dt = 1/4"""
    import math
    Cgp = C_cos / math.cos(math.radians(30.0))
    phases = [dict(eta=1.0, G=1.0, Kb=5.0, C=Cgp, phi_deg=30.0, psi_deg=psi_deg, eta_vp=1.0e-2),
              dict(eta=1.0, G=0.5, Kb=5.0, C=Cgp, phi_deg=30.0, psi_deg=psi_deg, eta_vp=1.0e-2)]
    ni = (nx, ny, nz)
    a = alloc_state(ni, 2)
    v, c = _locations(ni)
    loc = dict(phase_c=c, phase_yz=(c[0], v[1], v[2]), phase_xz=(v[0], c[1], v[2]), phase_xy=(v[0], v[1], c[2]))
    for name, xs in loc.items():
        X = np.meshgrid(*xs, indexing="ij")
        r2 = sum((X[q] - 0.5) ** 2 for q in range(3) if q != axis)
        outside = r2 > radius ** 2
        a[name][0], a[name][1] = np.where(outside, 1.0, 0.0), np.where(outside, 0.0, 1.0)
    a["eta"][...] = 1.0
    out = 1 if axis is None else axis
    p, q = [k for k in range(3) if k != out]
    sh = lambda k: tuple(-1 if s == k else 1 for s in range(3))
    a["V" + COMP[p]][...] = v[p].reshape(sh(p))
    a["V" + COMP[q]][...] = -v[q].reshape(sh(q))
    for k in COMP:
        a["V" + k][1:-1, 1:-1, 1:-1] = 0.0
    flow_bcs(a)
    return a, phases, tuple(1.0 / n for n in ni), 0.25


def random_state(ni, seed=20261020, yielding=True):
    """every input of every kernel non-trivial, the recipe of tests/_dyrel.py: two phases (phase 1 plastic with a LinearSoftening of the cohesion and a dilation
    angle, phase 2 elastic-viscous only), mixed ratios with exact zeros and ones, fields of both signs, η over three decades; positive DYREL arrays"""
    rng = np.random.default_rng(seed)
    C = 0.3 if yielding else 1.0e3
    phases = [dict(eta=1.0, G=1.0, Kb=2.0, C=C, phi_deg=30.0, psi_deg=5.0, eta_vp=1.0e-2, softening_C=dict(kind="linear", min=C / 2, max=C, lo=0.0, hi=0.5)),
              dict(eta=0.1, G=0.5, Kb=3.0)]
    a = alloc_state(ni, 2)
    u = lambda k, lo, hi: a[k].__setitem__(Ellipsis, rng.uniform(lo, hi, size=a[k].shape))
    for k in ("P", "P0", "Vx", "Vy", "Vz", "fx", "fy", "fz", "RP", "dPpsi", "Rx", "Ry", "Rz"):
        u(k, -2.0, 2.0)
    for pre in ("e", "t", "to"):
        for c in ("xx", "yy", "zz", "yz", "xz", "xy"):
            u(pre + c, -2.0, 2.0)
    for k in ("tyz_c", "txz_c", "txy_c", "toyz_c", "toxz_c", "toxy_c"):
        u(k, -2.0, 2.0)
    u("Q", -0.1, 0.1)
    u("EII_pl", 0.0, 0.6)
    a["eta"][...] = 10.0 ** rng.uniform(-2.0, 1.0, size=a["eta"].shape)
    for k in ("lam", "lamv_yz", "lamv_xz", "lamv_xy"):
        u(k, 0.0, 0.1)
    for k in ("phase_c", "phase_yz", "phase_xz", "phase_xy"):
        r = rng.uniform(0.0, 1.0, size=a[k].shape[1:])
        r[rng.uniform(size=r.shape) < 0.3] = 0.0
        r[rng.uniform(size=r.shape) < 0.3] = 1.0
        a[k][0], a[k][1] = r, 1.0 - r
    d = new_dyrel(ni)
    for k in d:
        d[k][...] = rng.uniform(0.5, 2.0, size=d[k].shape)
    for k in ("dVxdtau", "dVydtau", "dVzdtau", "Rx0", "Ry0", "Rz0", "P_num"):
        d[k][...] = rng.uniform(-1.0, 1.0, size=d[k].shape)
    return a, d, phases, (1.0 / ni[0], 1.3 / ni[1], 0.8 / ni[2]), 0.25
