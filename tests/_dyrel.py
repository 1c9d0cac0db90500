"""NumPy restatement of the reference's 2D DYREL solver (self-tuned dynamic relaxation inside Powell-Hestenes pressure iterations), written from its
sources: src/DYREL/types.jl, constructors.jl:13-57,137-190,230-254 (DYREL, DYREL!, compute_bulk_viscosity_and_penalty!), pressure_kernels.jl:112 (_compute_RP!),
velocity_kernels.jl:154-240 (compute_∇V_strain_rate_RP!), :326-349 (compute_PH_residual_V!), :625-727 (compute_dV!, update_cV!, damped_update_V,
compute_DR_residual_update_V!), stress_kernels.jl:100-307 (compute_stress_viscosity_DRYEL!, compute_local_stress, _compute_local_stress),
Gershgorin.jl:1-155,171-247 (Gershgorin_Stokes2D_SchurComplement!, update_α_β!, update_dτV_α_β!), solver.jl:44-294,359-370 (_solve_DYREL!, compute_λminV!), with
MiniKernels.jl:37-98 (differences, averages, _gather), stokes/StressKernels.jl:1304-1315 (clamped_indices, av_clamped), rheology/StressUpdate.jl:128-144,384-484
(plastic_params, _yieldfunction_elements, _plastic_grad_elements; Drucker-Prager: F = τII - cosϕ C - sinϕ P, ∂Q/∂τ = τ / (2 τII) with the shear slot halved once,
∂Q/∂P = -sinψ, ∂F/∂P = -sinϕ), Utils.jl:633,662 (allzero, continuation_linear) and rheology/Viscosity.jl:510-548,599-619 (local_viscosity_args, compute_phase_viscosity).

Arrays are Julia-shaped (x first), indices 0-based, names as jrx_vep2d_fields plus txx_v, tyy_v, toxx_v, toyy_v, lam, lamv, dPpsi; the DYREL struct is a dict
with the reference's field names in ASCII (gamma_eff, Dx, lmaxVx, dVxdtau, dtauVx, dVx, betaVx, cVx, alphaVx, etab, P_num, Rx0, ...).  Every function computes in
the dtype of its arrays (float64, or np.longdouble for the rounding-spread bound of the GPU tests); scalars are cast to it first.  NumPy has no fused
multiply-add: where the reference says @muladd (update_α_β!) this file rounds twice.  One block, uniform spacing, no RockRatio, the plain form of _RP_cell.
"""
import numpy as np

from _variational_stokes import _law_viscosity

DYREL_CENTER = ("gamma_eff", "etab", "P_num")
DYREL_X = ("Dx", "lmaxVx", "dVxdtau", "dtauVx", "dVx", "betaVx", "cVx", "alphaVx", "Rx0")
DYREL_Y = ("Dy", "lmaxVy", "dVydtau", "dtauVy", "dVy", "betaVy", "cVy", "alphaVy", "Ry0")
EXTRA_SHAPES = dict(txx_v="v", tyy_v="v", toxx_v="v", toyy_v="v", lamv="v", lam="c", dPpsi="c")


def new_dyrel(ni, dtype=np.float64):
    """DYREL(ni) (constructors.jl:13-57): zero arrays; the 2D placeholders (Dz, ...) are left out"""
    nx, ny = ni
    d = {k: np.zeros((nx, ny), dtype=dtype, order="F") for k in DYREL_CENTER}
    d.update({k: np.zeros((nx - 1, ny), dtype=dtype, order="F") for k in DYREL_X})
    d.update({k: np.zeros((nx, ny - 1), dtype=dtype, order="F") for k in DYREL_Y})
    return d


def extra_arrays(ni, dtype=np.float64):
    nx, ny = ni
    shp = dict(c=(nx, ny), v=(nx + 1, ny + 1))
    return {k: np.zeros(shp[s], dtype=dtype, order="F") for k, s in EXTRA_SHAPES.items()}


def astype(a, dtype):
    """a deep copy of a dict of arrays in another floating-point type"""
    return {k: (np.array(v, dtype=dtype, order="F") if isinstance(v, np.ndarray) else v) for k, v in a.items()}


def _T(x):
    return x.dtype.type


# ---------------------------------------------------------------- pure helpers
def compute_RP(P, P0, divV, Q, etab, dt):
    """_compute_RP!(P, P0, ∇V, Q, ηb, dt) = -∇V - (P - P0) / ηb + (Q / dt) -- pressure_kernels.jl:112"""
    return -divV - (P - P0) / etab + (Q / dt)


def damped_update_V(dVdtau, R, alpha, beta, dtau):
    """velocity_kernels.jl:660-663: (α dVdτ + R, (α dVdτ + R) β dτ)"""
    new = alpha * dVdtau + R
    return new, new * beta * dtau


def _sinv(xx, yy, xy):
    """second_invariant of (xx, yy, xy)"""
    return np.sqrt(0.5 * (xx * xx + yy * yy) + xy * xy)


def _ratio_sum(vals, r):
    """fn_ratio (src/phases/phases.jl:6-15)"""
    x = np.zeros(r.shape[1:], dtype=r.dtype)
    T = r.dtype.type
    for q, v in enumerate(vals):
        with np.errstate(invalid="ignore"):
            x = x + np.where(r[q] == 0.0, T(0.0), T(v) * r[q])
    return x


def _av_clamped(A):
    """av_clamped over clamped_indices (StressKernels.jl:1304-1315) at every vertex: 0.25 (A[i0, j0] + A[ic, jc] + A[i0, jc] + A[ic, j0])"""
    nx, ny = A.shape
    ii, jj = np.arange(nx + 1), np.arange(ny + 1)
    i0, ic = np.clip(ii - 1, 0, nx - 1), np.clip(ii, 0, nx - 1)
    j0, jc = np.clip(jj - 1, 0, ny - 1), np.clip(jj, 0, ny - 1)
    g = lambda I, J: A[np.ix_(I, J)]
    return _T(A)(0.25) * (g(i0, j0) + g(ic, jc) + g(i0, jc) + g(ic, j0))


def _av_gather(V):
    """sum(_gather(A, I...)) / 4: ((A[i, j] + A[i+1, j]) + A[i, j+1]) + A[i+1, j+1] (MiniKernels.jl:96-98)"""
    return (V[:-1, :-1] + V[1:, :-1] + V[:-1, 1:] + V[1:, 1:]) / 4


# ---------------------------------------------------------------- velocity_kernels.jl:154-240
def strain_rate_RP(a, d, _di, dt, do_strain_rate=True):
    """compute_∇V_strain_rate_RP!: ε.xx, ε.yy, ε.xy (do_strain_rate) and R.RP; ∇V is not stored"""
    Vx, Vy = a["Vx"], a["Vy"]
    T = _T(Vx)
    _dx, _dy, dt = T(_di[0]), T(_di[1]), T(dt)
    if do_strain_rate:
        dVx_dy = (Vx[:, 1:] - Vx[:, :-1]) * _dy
        dVy_dx = (Vy[1:, :] - Vy[:-1, :]) * _dx
        a["exy"][...] = T(0.5) * (dVx_dy + dVy_dx)
    dVx_dx = (Vx[1:, 1:-1] - Vx[:-1, 1:-1]) * _dx
    dVy_dy = (Vy[1:-1, 1:] - Vy[1:-1, :-1]) * _dy
    div = dVx_dx + dVy_dy
    if do_strain_rate:
        third = T(1) / T(3)
        div_third = div * third
        a["exx"][...] = dVx_dx - div_third
        a["eyy"][...] = dVy_dy - div_third
    with np.errstate(invalid="ignore", divide="ignore"):
        a["RP"][...] = compute_RP(a["P"], a["P0"], div, a["Q"], d["etab"], dt)
    return div


# ---------------------------------------------------------------- stress_kernels.jl:224-307
def _soften(kind_law, EII, v0):
    if kind_law is None:
        return v0
    T = _T(EII)
    if kind_law["kind"] != "linear":
        raise NotImplementedError("the restatement knows NoSoftening and LinearSoftening")
    a, b, c, dd = (T(kind_law[k]) for k in ("min", "max", "lo", "hi"))
    return np.where(EII >= dd, a, np.where(EII <= c, b, b + (a - b) / (dd - c) * (EII - c)))


def _phase_local_stress(eij, toij, eta, P, lam, rel, ph, dt, EII):
    """_compute_local_stress for one phase over whole arrays; returns the 11 outputs and the trial F (NaN where the early return was taken)"""
    T = _T(eta)
    G, Kb, dt, rel = T(ph["G"]), T(ph["Kb"]), T(dt), T(rel)
    ispl = ph.get("C") is not None
    eta_reg = T(ph.get("eta_vp", 0.0)) if ispl else T(0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        eta_ve = (1 / (1 / eta + 1 / (G * dt))) if np.isinf(G) else (eta * G * dt) / (eta + G * dt)
        inv_2Gdt = 1 / (2 * G * dt)
        eff = [e + t * inv_2Gdt for e, t in zip(eij, toij)]
        eII = _sinv(*eff)
        tij = [2 * eta_ve * e for e in eff]
        tII = _sinv(*tij)
        if ispl:
            C = _soften(ph.get("softening_C"), EII, T(ph["C"]))
            deg = np.arctan(T(1)) / T(45)          # π / 180 in the working precision
            sin0, cos0 = np.sin(T(ph["phi_deg"]) * deg), np.cos(T(ph["phi_deg"]) * deg)
            if ph.get("softening_phi") is not None:
                phi = _soften(ph["softening_phi"], EII, T(ph["phi_deg"]))
                sinphi, cosphi = np.sin(phi * deg), np.cos(phi * deg)
            else:
                sinphi, cosphi = sin0, cos0
            F = tII - cosphi * C - sinphi * P
            dQdt = [T(0.5) * tij[0] / tII, T(0.5) * tij[1] / tII, T(0.5) * (tij[2] / tII)]
            dQdP, dFdP = -np.sin(T(ph.get("psi_deg", 0.0)) * deg), -sin0          # ∂F/∂P with the unsoftened angle, as include/jrx.h states the law
        else:
            F = tII
            dQdt = [np.zeros_like(eta)] * 3
            dQdP, dFdP = T(0.0), T(0.0)
        yields = (F >= 0) if ispl else np.zeros(eta.shape, dtype=bool)
        bulk = T(0.0) if np.isinf(Kb) else Kb * dt * dFdP * dQdP
        lam_new = F / (eta_ve + eta_reg + bulk)
        lam_o = np.where(yields, rel * lam_new + (1 - rel) * lam, T(0.0))
        evol = np.where(yields, -lam_o * dQdP, T(0.0))
        pos = lam_o > 0
        epl = [np.where(pos, lam_o * g, T(0.0)) for g in dQdt]
        tij = [np.where(pos, t - T(2.0) * eta_ve * e, t) for t, e in zip(tij, epl)]
        tII = np.where(pos, _sinv(*tij), tII)
        dP = np.where(pos, T(0.0) if dQdP == 0 else -lam_o * dQdP * Kb * dt, T(0.0))
        eta_vep = tII * T(0.5) * (1 / _sinv(*eij))
    z = eII == 0          # early return: zeros, η_vep = η
    out = tij + epl + [tII, lam_o, dP, eta_vep, evol]
    out = [np.where(z, T(0.0), x) for x in out]
    out[9] = np.where(z, eta, out[9])
    return out, np.where(z, np.nan, F), yields & ~z


def local_stress(eij, toij, eta, P, lam, rel, phases, ratio, dt, EII):
    """compute_local_stress (stress_kernels.jl:224-247): Σ over the phases of ratio .* _compute_local_stress, a zero ratio contributing zeros.
    Returns the 11 outputs, and per plastic phase the trial F and the yield mask (for the yield-branch comparison of the tests)."""
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


def _visc_invariant(xx, yy, xy):
    """_update_τII_viscosity (stress_kernels.jl:129-131): eps() on the normal components of an all-zero tensor"""
    a0 = np.where((xx == 0) & (yy == 0) & (xy == 0), _T(xx)(np.finfo(np.float64).eps), _T(xx)(0.0))
    return _sinv(xx + a0, yy - a0, xy)


def phase_viscosity_tauII(phases, r, tII, Tk, P):
    """compute_phase_viscosity(rheology, ratio, τII, compute_viscosity_τII, args) (Viscosity.jl:599-619)"""
    T = r.dtype.type
    laws = [np.asarray(_law_viscosity(ph, tII, Tk, P, True), dtype=r.dtype) for ph in phases]
    s = np.zeros(r.shape[1:], dtype=r.dtype)
    for q in range(len(phases)):
        s = s + np.where(r[q] != 0, (T(1) / laws[q]) * r[q], T(0.0))
    with np.errstate(divide="ignore"):
        e = T(1) / s
    for q in reversed(range(len(phases))):
        e = np.where(r[q] > 0.999, laws[q], e)
    return e


def stress_viscosity(a, d, phases, rel, dt, nu, cutoff, linear_viscosity, Tk=0.0, diag=None):
    """compute_stress_viscosity_DRYEL! (stress_kernels.jl:137-222).  Every array the kernel writes is read at the thread's own index only, so whole-array
    evaluation from the old values is the kernel's result.  diag (a dict) receives the trial F and yield masks."""
    T = _T(a["P"])
    nu_, lo, hi = T(nu), T(cutoff[0]), T(cutoff[1])
    # vertices
    eij = (_av_clamped(a["exx"]), _av_clamped(a["eyy"]), a["exy"])
    toij = (a["toxx_v"], a["toyy_v"], a["toxy"])
    eta_v_old = a["eta_v"].copy()
    Pv = _av_clamped(a["P"])
    out, Fv = local_stress(eij, toij, eta_v_old, Pv, a["lamv"], rel, phases, a["phase_v"], dt, _av_clamped(a["EII_pl"]))
    a["txx_v"][...], a["tyy_v"][...], a["txy"][...] = out[0], out[1], out[2]
    a["eplxy"][...] = out[5]
    a["lamv"][...] = out[7]
    if not linear_viscosity:
        tII = _visc_invariant(out[0], out[1], out[2])
        e = phase_viscosity_tauII(phases, a["phase_v"], tII, Tk, Pv)
        e = (1 - nu_) * eta_v_old + nu_ * e
        a["eta_v"][...] = np.minimum(np.maximum(e, lo), hi)
    # centres
    eij = (a["exx"], a["eyy"], _av_gather(a["exy"]))
    toij = (a["toxx"], a["toyy"], a["toxy_c"])
    eta_old = a["eta"].copy()
    out, Fc = local_stress(eij, toij, eta_old, a["P"], a["lam"], rel, phases, a["phase_c"], dt, a["EII_pl"])
    a["txx"][...], a["tyy"][...], a["txy_c"][...] = out[0], out[1], out[2]
    a["eplxx"][...], a["eplyy"][...] = out[3], out[4]
    a["evol_pl"][...] = out[10]
    a["tII"][...] = out[6]
    a["eta_vep"][...] = out[9]
    a["lam"][...] = out[7]
    a["dPpsi"][...] = out[8]
    d["P_num"][...] = d["gamma_eff"] * a["RP"] + out[8]          # θc = γ_eff RP + ΔPψ
    if not linear_viscosity:
        tII = _visc_invariant(out[0], out[1], out[2])
        e = phase_viscosity_tauII(phases, a["phase_c"], tII, Tk, a["P"])
        e = (1 - nu_) * eta_old + nu_ * e
        a["eta"][...] = np.minimum(np.maximum(e, lo), hi)
    if diag is not None:
        diag.update(Fv=Fv, Fc=Fc)


# ---------------------------------------------------------------- velocity_kernels.jl:326-349, 671-727
def _momentum(a, Pextra, _di):
    """d_xa(τxx) + d_yi(τxy) - d_xa(P) - d_xa(θ) - av_xa(ρgx) and the y analogue, term by term in the reference's order"""
    T = _T(a["P"])
    _dx, _dy = T(_di[0]), T(_di[1])
    d_xa = lambda A: (-A[:-1, :] + A[1:, :]) * _dx
    d_ya = lambda A: (-A[:, :-1] + A[:, 1:]) * _dy
    txy = a["txy"]
    d_yi = (-txy[1:-1, :-1] + txy[1:-1, 1:]) * _dy
    d_xi = (-txy[:-1, 1:-1] + txy[1:, 1:-1]) * _dx
    Rx = d_xa(a["txx"]) + d_yi - d_xa(a["P"]) - d_xa(Pextra) - (a["fx"][:-1, :] + a["fx"][1:, :]) * T(0.5)
    Ry = d_ya(a["tyy"]) + d_xi - d_ya(a["P"]) - d_ya(Pextra) - (a["fy"][:, :-1] + a["fy"][:, 1:]) * T(0.5)
    return Rx, Ry


def ph_residual(a, _di):
    """compute_PH_residual_V! (velocity_kernels.jl:326-349)"""
    a["Rx"][...], a["Ry"][...] = _momentum(a, a["dPpsi"], _di)


def dr_residual_update_V(a, d, _di):
    """compute_DR_residual_update_V! (velocity_kernels.jl:671-727)"""
    Rx, Ry = _momentum(a, d["P_num"], _di)
    with np.errstate(invalid="ignore", divide="ignore"):
        Rx, Ry = Rx / d["Dx"], Ry / d["Dy"]
    a["Rx"][...], a["Ry"][...] = Rx, Ry
    d["dVxdtau"][...], dVx = damped_update_V(d["dVxdtau"], Rx, d["alphaVx"], d["betaVx"], d["dtauVx"])
    d["dVydtau"][...], dVy = damped_update_V(d["dVydtau"], Ry, d["alphaVy"], d["betaVy"], d["dtauVy"])
    a["Vx"][1:-1, 1:-1] += dVx
    a["Vy"][1:-1, 1:-1] += dVy


def flow_bcs(a, free_slip=True, no_slip=False):
    """flow_bcs! with one kind on the four faces (boundaryconditions/free_slip.jl:1-13, no_slip.jl:1-18)"""
    Vx, Vy = a["Vx"], a["Vy"]
    if no_slip:
        Vx[0, :], Vx[-1, :] = 0.0, 0.0          # left / right first, then bottom / top
        Vy[0, :], Vy[-1, :] = -Vy[1, :], -Vy[-2, :]
        Vy[:, 0], Vy[:, -1] = 0.0, 0.0
        Vx[:, 0], Vx[:, -1] = -Vx[:, 1], -Vx[:, -2]
    elif free_slip:
        Vx[:, 0], Vx[:, -1] = Vx[:, 1], Vx[:, -2]
        Vy[0, :], Vy[-1, :] = Vy[1, :], Vy[-2, :]


# ---------------------------------------------------------------- constructors.jl:230-254, Gershgorin.jl
def bulk_viscosity_and_penalty(a, d, phases, gamma_fact, dt):
    """compute_bulk_viscosity_and_penalty! (constructors.jl:230-254): ηb = Kb dt; γ_eff = γ_phy γ_num / (γ_phy + γ_num)"""
    eta = a["eta"]
    T = _T(eta)
    fin = eta[~np.isinf(eta)]
    eta_mean = fin.sum() / T(fin.size)
    Kbdt = _ratio_sum([ph["Kb"] for ph in phases], a["phase_c"]) * T(dt)
    d["etab"][...] = Kbdt
    g_num = T(gamma_fact) * np.where(np.isinf(eta), eta_mean, eta)
    g_phy = np.where(np.isinf(Kbdt), g_num, Kbdt)
    d["gamma_eff"][...] = g_phy * g_num / (g_phy + g_num)


def gershgorin(a, d, phases, di, dt):
    """_Gershgorin_Stokes2D_SchurComplement! (Gershgorin.jl:21-155), uniform spacing"""
    eta, etav, gam = a["eta"], a["eta_v"], d["gamma_eff"]
    T = _T(eta)
    dt = T(dt)
    Gc = _ratio_sum([ph["G"] for ph in phases], a["phase_c"])
    Gv = _ratio_sum([ph["G"] for ph in phases], a["phase_v"])
    _dx, _dy = 1 / T(di[0]), 1 / T(di[1])
    _dx2, _dy2, _dxdy = _dx * _dx, _dy * _dy, _dx * _dy
    c43, c23 = T(4) / T(3), T(2) / T(3)
    ve = lambda e, G: 1 / (1 / e + 1 / (G * dt))
    with np.errstate(invalid="ignore", divide="ignore"):
        # x nodes (i, j), i < nx - 1: N = vertex (i+1, j+1), S = vertex (i+1, j), W = centre (i, j), E = centre (i+1, j)
        eN, eS = ve(etav[1:-1, 1:], Gv[1:-1, 1:]), ve(etav[1:-1, :-1], Gv[1:-1, :-1])
        eW, eE = ve(eta[:-1, :], Gc[:-1, :]), ve(eta[1:, :], Gc[1:, :])
        gW, gE = gam[:-1, :], gam[1:, :]
        eN_dy, eS_dy, eE_dx, eW_dx, gE_dx, gW_dx = eN * _dy, eS * _dy, eE * _dx, eW * _dx, gE * _dx, gW * _dx
        Dx = (eN_dy + eS_dy) * _dy + (gE_dx + gW_dx + c43 * (eE_dx + eW_dx)) * _dx
        Cxx = (np.abs(eN * _dy2) + np.abs(eS * _dy2) + np.abs((gE + c43 * eE) * _dx2) + np.abs((gW + c43 * eW) * _dx2) + np.abs(Dx))
        Cxy = (np.abs((gE - c23 * eE + eN) * _dxdy) + np.abs((gE - c23 * eE + eS) * _dxdy) + np.abs((gW + eN - c23 * eW) * _dxdy)
               + np.abs((gW + eS - c23 * eW) * _dxdy))
        d["Dx"][...] = Dx
        d["lmaxVx"][...] = (1 / Dx) * (Cxx + Cxy)
        # y nodes (i, j), j < ny - 1: S = centre (i, j), N = centre (i, j+1), W = vertex (i, j+1), E = vertex (i+1, j+1)
        eS, eN = ve(eta[:, :-1], Gc[:, :-1]), ve(eta[:, 1:], Gc[:, 1:])
        eW, eE = ve(etav[:-1, 1:-1], Gv[:-1, 1:-1]), ve(etav[1:, 1:-1], Gv[1:, 1:-1])
        gS, gN = gam[:, :-1], gam[:, 1:]
        eE_dx, eW_dx, eN_dy, eS_dy, gN_dy, gS_dy = eE * _dx, eW * _dx, eN * _dy, eS * _dy, gN * _dy, gS * _dy
        Dy = (gN_dy + gS_dy + c43 * (eN_dy + eS_dy)) * _dy + (eE_dx + eW_dx) * _dx
        Cyy = (np.abs(eE * _dx2) + np.abs(eW * _dx2) + np.abs((gN + c43 * eN) * _dy2) + np.abs((gS + c43 * eS) * _dy2) + np.abs(Dy))
        Cyx = (np.abs((gN + eE - c23 * eN) * _dxdy) + np.abs((gN - c23 * eN + eW) * _dxdy) + np.abs((gS + eE - c23 * eS) * _dxdy)
               + np.abs((gS - c23 * eS + eW) * _dxdy))
        d["Dy"][...] = Dy
        d["lmaxVy"][...] = (1 / Dy) * (Cyx + Cyy)


def update_alpha_beta(d):
    """update_α_β! (Gershgorin.jl:182-198): β = 2 dτ / (2 + c dτ), α = (2 - c dτ) / (2 + c dτ)"""
    for c in "xy":
        dtau, cV = d[f"dtauV{c}"], d[f"cV{c}"]
        with np.errstate(invalid="ignore", divide="ignore"):
            d[f"betaV{c}"][...] = 2 * dtau / (2 + cV * dtau)
            d[f"alphaV{c}"][...] = (2 - cV * dtau) / (2 + cV * dtau)


def update_dtauV_alpha_beta(d, CFL):
    """update_dτV_α_β! (Gershgorin.jl:229-247): dτ = 2 / √λmax CFL, then α, β"""
    for c in "xy":
        with np.errstate(invalid="ignore", divide="ignore"):
            d[f"dtauV{c}"][...] = 2 / np.sqrt(d[f"lmaxV{c}"]) * _T(d["Dx"])(CFL)
    update_alpha_beta(d)


def dyrel_init(a, d, phases, di, dt, CFL=0.99, gamma_fact=20.0):
    """DYREL! (constructors.jl:178-190)"""
    bulk_viscosity_and_penalty(a, d, phases, gamma_fact, dt)
    gershgorin(a, d, phases, di, dt)
    update_dtauV_alpha_beta(d, CFL)


def compute_viscosity(a, phases, nu, cutoff, Tk=0.0):
    """compute_viscosity! with the strain-rate invariant, LinearViscous laws (the invariant is not read): centres and vertices"""
    T = _T(a["eta"])
    for eta, ph in (("eta", "phase_c"), ("eta_v", "phase_v")):
        e = phase_viscosity_tauII(phases, a[ph], np.zeros(a[eta].shape, dtype=a[eta].dtype), Tk, 0.0)
        e = (1 - T(nu)) * a[eta] + T(nu) * e
        a[eta][...] = np.minimum(np.maximum(e, T(cutoff[0])), T(cutoff[1]))


def compute_rhog(a, phases):
    """compute_ρg!(ρg[end], phase_ratios, rheology, args), ConstantDensity laws"""
    if any(ph["density"].get("kind", "constant") != "constant" for ph in phases):
        raise NotImplementedError("the restatement knows ConstantDensity")
    a["fy"][...] = _ratio_sum([ph["density"]["rho0"] for ph in phases], a["phase_c"]) * _T(a["fy"])(phases[0].get("g", 0.0))


def lambda_min(a, d):
    """compute_λminV! (solver.jl:359-365)"""
    d["dVx"][...] = d["dVxdtau"] * d["betaVx"] * d["dtauVx"]
    d["dVy"][...] = d["dVydtau"] * d["betaVy"] * d["dtauVy"]
    num = np.sum(d["dVx"] * (a["Rx"] - d["Rx0"])) + np.sum(d["dVy"] * (a["Ry"] - d["Ry0"]))
    den = np.sum(d["dVx"] ** 2) + np.sum(d["dVy"] ** 2)
    return abs(num) / den


def ph_norms(a):
    """solver.jl:151-152: ‖R_d‖ / √v_dofs[d] and ‖RP‖ / √p_dof of one block"""
    nx, ny = a["P"].shape
    nrm = lambda x: float(np.sqrt(np.sum(x * x)))
    return (nrm(a["Rx"]) / np.sqrt((nx - 2) * (ny - 1)), nrm(a["Ry"]) / np.sqrt((nx - 1) * (ny - 2))), nrm(a["RP"]) / np.sqrt(nx * ny)


def solve_DYREL(a, d, phases, di, dt, *, eps=1.0e-6, CFL=0.99, c_fact=0.5, gamma_fact=20.0, viscosity_cutoff=(-np.inf, np.inf), viscosity_relaxation=1.0e-2,
                λ_relaxation_DR=1, λ_relaxation_PH=1, iterMax=50.0e3, total_iterMax=50.0e3, nout=100, rel_drop=1.0e-2, linear_viscosity=False,
                free_slip=True, no_slip=False, Tk=0.0, itPH_max=1000, **_):
    """_solve_DYREL! (solver.jl:44-294), one block.  Returns the four histories and the iteration counts.  `itPH_max` (1000 in the reference, solver.jl:122)
    lets a test stop after the first Powell-Hestenes iterations, whose residuals are the driver's reference norms errV0 (itPH = 1) and errPt0 (itPH = 2)."""
    nx, ny = a["P"].shape
    _di = (1.0 / di[0], 1.0 / di[1])
    EPS = float(np.finfo(np.float64).eps)
    a["P0"][...] = a["P"]
    for k in ("eplxx", "eplyy", "eplxy_c"):
        a[k][...] = 0.0
    a["lam"][...] = 0.0
    a["lamv"][...] = 0.0
    err_min, iteration, itPH_done = np.inf, 0, 0
    errV0, errPt0, errV00 = (1.0, 1.0), 1.0, (1.0, 1.0)
    hist = dict(err_evo_it=[], err_evo_V=[], err_evo_P=[], err_evo_tot=[])
    compute_viscosity(a, phases, 1.0, viscosity_cutoff, Tk)
    has_rho = any(ph.get("density") is not None for ph in phases)
    if has_rho:
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
        errV_rel = tuple(min(e / e0, e) for e, e0 in zip(errV, errV0))
        err = max(errV_rel + (min(errPt / errPt0, errPt),))
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
                d["Rx0"][...], d["Ry0"][...] = a["Rx"], a["Ry"]
            strain_rate_RP(a, d, _di, dt, True)
            stress_viscosity(a, d, phases, λ_relaxation_DR, dt, viscosity_relaxation, viscosity_cutoff, linear_viscosity, Tk)
            dr_residual_update_V(a, d, _di)
            flow_bcs(a, free_slip, no_slip)
            if iteration % nout == 0:
                nrm = lambda x: float(np.sqrt(np.sum(x * x)))
                eV = (nrm(d["Dx"] * a["Rx"]) / np.sqrt((nx - 2) * (ny - 1)), nrm(d["Dy"] * a["Ry"]) / np.sqrt((nx - 1) * (ny - 2)))
                if iteration == nout:
                    errV00 = (max(eV) + EPS,) * 2
                ratio = tuple(e / e0 for e, e0 in zip(eV, errV00))
                err = max(ratio)
                if np.isnan(err):
                    raise FloatingPointError("NaN detected in inner loop")
                hist["err_evo_tot"].append(err)
                hist["err_evo_V"].append(max(ratio))
                hist["err_evo_P"].append(errPt / errPt0)
                hist["err_evo_it"].append(float(iteration))
                lmin = lambda_min(a, d)
                cV = 2 * np.sqrt(lmin) * _T(d["cVx"])(c_fact)
                d["cVx"][...] = cV
                d["cVy"][...] = cV
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
    """solver.jl:269-290: P += ΔPψ, ∇V, vorticity, shear2center! x3, accumulate_tensor!, accumulate_vol!, τ_o = τ (centres, vertices, xx_v, yy_v)"""
    T = _T(a["P"])
    _dx, _dy, dt = T(_di[0]), T(_di[1]), T(dt)
    a["P"][...] += a["dPpsi"]
    Vx, Vy = a["Vx"], a["Vy"]
    a["divV"][...] = (-Vx[:-1, 1:-1] + Vx[1:, 1:-1]) * _dx + (-Vy[1:-1, :-1] + Vy[1:-1, 1:]) * _dy
    if a.get("omega_xy") is not None:
        a["omega_xy"][...] = T(0.5) * ((-Vy[:-1, :] + Vy[1:, :]) * _dx - (-Vx[:, :-1] + Vx[:, 1:]) * _dy)
    s2c = lambda v: T(0.25) * (v[:-1, :-1] + v[1:, :-1] + v[:-1, 1:] + v[1:, 1:])
    a["exy_c"][...] = s2c(a["exy"])
    a["eplxy_c"][...] = s2c(a["eplxy"])
    v = a["eplxy"]
    sq = T(0.25) * (v[:-1, :-1] ** 2 + v[1:, :-1] ** 2 + v[:-1, 1:] ** 2 + v[1:, 1:] ** 2)
    a["EII_pl"][...] += np.sqrt(T(0.5) * (a["eplxx"] ** 2 + a["eplyy"] ** 2) + sq) * dt
    a["EVol_pl"][...] += dt * a["evol_pl"]
    for k in ("xx", "yy", "xy", "xy_c", "xx_v", "yy_v"):
        a["to" + k][...] = a["t" + k]


# ---------------------------------------------------------------- set-ups shared by the tests
VEP_CENTER = ("P", "P0", "divV", "Q", "exx", "eyy", "exy_c", "eplxx", "eplyy", "eplxy_c", "txx", "tyy", "txy_c", "tII", "toxx", "toyy", "toxy_c", "eta", "eta_vep",
              "EII_pl", "evol_pl", "EVol_pl", "fx", "fy", "RP")
VEP_VERTEX = ("exy", "eplxy", "txy", "toxy", "eta_v", "omega_xy")


def alloc_state(ni, nphase, dtype=np.float64):
    nx, ny = ni
    a = {k: np.zeros((nx, ny), dtype=dtype, order="F") for k in VEP_CENTER}
    a.update({k: np.zeros((nx + 1, ny + 1), dtype=dtype, order="F") for k in VEP_VERTEX})
    a.update(Vx=np.zeros((nx + 1, ny + 2), dtype=dtype, order="F"), Vy=np.zeros((nx + 2, ny + 1), dtype=dtype, order="F"),
             Rx=np.zeros((nx - 1, ny), dtype=dtype, order="F"), Ry=np.zeros((nx, ny - 1), dtype=dtype, order="F"),
             phase_c=np.zeros((nphase, nx, ny), dtype=dtype, order="F"), phase_v=np.zeros((nphase, nx + 1, ny + 1), dtype=dtype, order="F"))
    a.update(extra_arrays(ni, dtype))
    return a


def shearband_state(nx, ny, psi_deg=0.0, C_cos=1.6):
    """the shear band of test/test_shearband2D_DYREL.jl:62-149 on an nx x ny grid of the unit square: matrix G = 1, circular inclusion G = 0.5 of radius 0.1,
    η = 1, Kb = 5, DruckerPrager_regularised(C = 1.6 / cos 30°, ϕ = 30°, η_vp = 1e-2, Ψ), pure shear ε_bg = 1 on the boundary, zero interior velocity, dt = 1/4.
    The first step loads elastically to τII = 2 ε_bg / (1/η + 1/(G dt)) = 0.4 in the matrix, so a C cos ϕ (`C_cos`) below that yields at once."""
    import math
    Cgp = C_cos / math.cos(math.radians(30.0))
    phases = [dict(eta=1.0, G=1.0, Kb=5.0, C=Cgp, phi_deg=30.0, psi_deg=psi_deg, eta_vp=1.0e-2),
              dict(eta=1.0, G=0.5, Kb=5.0, C=Cgp, phi_deg=30.0, psi_deg=psi_deg, eta_vp=1.0e-2)]
    a = alloc_state((nx, ny), 2)
    di = (1.0 / nx, 1.0 / ny)
    xv, yv = np.linspace(0.0, 1.0, nx + 1), np.linspace(0.0, 1.0, ny + 1)
    xc, yc = np.linspace(di[0] / 2, 1.0 - di[0] / 2, nx), np.linspace(di[1] / 2, 1.0 - di[1] / 2, ny)
    for name, (xs, ys) in (("phase_c", (xc, yc)), ("phase_v", (xv, yv))):
        X, Y = np.meshgrid(xs, ys, indexing="ij")
        outside = ((X - 0.5) ** 2 + (Y - 0.5) ** 2) > 0.1 ** 2
        a[name][0], a[name][1] = np.where(outside, 1.0, 0.0), np.where(outside, 0.0, 1.0)
    a["eta"][...] = 1.0
    a["eta_v"][...] = 1.0
    a["Vx"][...] = xv[:, None]
    a["Vy"][...] = -yv[None, :]
    a["Vx"][1:-1, 1:-1] = 0.0
    a["Vy"][1:-1, 1:-1] = 0.0
    flow_bcs(a)
    return a, phases, di, 0.25


def random_state(ni, seed=20260821, yielding=True):
    """every input of every kernel non-trivial: two phases (phase 1 plastic with a LinearSoftening of the cohesion and a dilation angle, phase 2 elastic-viscous
    only), mixed ratios with exact zeros and ones, fields of both signs, η over three decades, finite G, K, dt, non-zero Q, τ_o, P0; positive DYREL arrays"""
    rng = np.random.default_rng(seed)
    nx, ny = ni
    C = 0.3 if yielding else 1.0e3
    phases = [dict(eta=1.0, G=1.0, Kb=2.0, C=C, phi_deg=30.0, psi_deg=5.0, eta_vp=1.0e-2, softening_C=dict(kind="linear", min=C / 2, max=C, lo=0.0, hi=0.5)),
              dict(eta=0.1, G=0.5, Kb=3.0)]
    a = alloc_state(ni, 2)
    for k in ("P", "P0", "exx", "eyy", "exy", "txx", "tyy", "txy", "txy_c", "toxx", "toyy", "toxy", "toxy_c", "toxx_v", "toyy_v", "Vx", "Vy", "fx", "fy", "RP",
              "dPpsi", "Rx", "Ry"):
        a[k][...] = rng.uniform(-2.0, 2.0, size=a[k].shape)
    a["Q"][...] = rng.uniform(-0.1, 0.1, size=(nx, ny))
    a["EII_pl"][...] = rng.uniform(0.0, 0.6, size=(nx, ny))
    for k in ("eta", "eta_v"):
        a[k][...] = 10.0 ** rng.uniform(-2.0, 1.0, size=a[k].shape)
    for k in ("lam", "lamv"):
        a[k][...] = rng.uniform(0.0, 0.1, size=a[k].shape)
    for k in ("phase_c", "phase_v"):
        r = rng.uniform(0.0, 1.0, size=a[k].shape[1:])
        r[rng.uniform(size=r.shape) < 0.3] = 0.0
        r[rng.uniform(size=r.shape) < 0.3] = 1.0
        a[k][0], a[k][1] = r, 1.0 - r
    d = new_dyrel(ni)
    for k in d:
        d[k][...] = rng.uniform(0.5, 2.0, size=d[k].shape)
    for k in ("dVxdtau", "dVydtau", "Rx0", "Ry0", "P_num"):
        d[k][...] = rng.uniform(-1.0, 1.0, size=d[k].shape)
    return a, d, phases, (1.0 / nx, 1.3 / ny), 0.25
