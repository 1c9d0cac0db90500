"""NumPy restatement of compute_P! of the multiphase drivers with and without args.ΔT, with the kernels that run beside it in one pre pass.

Reference text restated (JustRelax.jl):
  src/stokes/PressureKernels.jl:186-195   _compute_P!(P, P0, ∇V, Q, η, K, G, dt, r, θ_dτ)
  src/stokes/PressureKernels.jl:197-206   _compute_P!(P, P0, ∇V, Q, ΔT, α, η, K, G, dt, r, θ_dτ): rhs = (-∇V + (α * (ΔT * _dt))) + (Q * _dt)
  src/stokes/PressureKernels.jl:129-152   compute_P_kernel! with ΔT: K, G, α = fn_ratio(...), ΔT[I...] at the cell's own index
  src/phases/phases.jl:6-30               fn_ratio: zero ratios skipped; a ratio of one returns that phase's value
  src/stokes/VelocityKernels.jl:3-6,59-104  compute_∇V!, compute_strain_rate! 2D / 3D
  src/Utils.jl:409-461                    compute_maxloc! with the clamped window (1, 1[, 1])
Arrays are (nx, ny[, nz]) with x first, as in Julia; phase ratios (nphase, ni...).  Every function computes in the dtype of its arrays (float64, or
np.longdouble for the rounding-spread bound of the GPU tests).  NumPy has no fused multiply-add: the two muladd of _compute_P! are a product and a sum.
"""
import numpy as np

ALPHA_KINDS = ("PT", "T")      # density laws that carry a thermal expansion; "constant" and "compressible" have none (GeoParams form, assumed: include/jrx.h)


def phase_alpha(phases):
    """get_thermal_expansion of each phase dict of the rheology table"""
    out = []
    for ph in phases:
        d = ph.get("density")
        out.append(float(d.get("alpha", 0.0)) if d is not None and d.get("kind", "constant") in ALPHA_KINDS else 0.0)
    return out


def fn_ratio(vals, ratio, early_return=False):
    """x = Σ_q (ratio_q == 0 ? 0 : vals_q * ratio_q) in phase order; early_return: the first phase whose ratio is one gives vals_q * ratio_q alone
    (the rule of the density average, which the thermal expansion follows)"""
    T = ratio.dtype.type
    x = np.zeros(ratio.shape[1:], dtype=ratio.dtype)
    done = np.zeros(ratio.shape[1:], dtype=bool)
    for q, v in enumerate(vals):
        r = ratio[q]
        term = np.where(r == 0, T(0), T(v) * r)
        if early_return:
            one = (r == 1) & ~done
            x = np.where(one, T(v) * r, np.where(done, x, x + term))
            done |= one
        else:
            x = x + term
    return x


def own_index(A, ni):
    """args.ΔT at the cell's own [i, j(, k)]: an array of extent ni as it is, one of extent ni .+ 2 (thermal.ΔT) WITHOUT the shift to the cell centre"""
    ni = tuple(ni)
    if tuple(A.shape) == ni:
        return A
    if tuple(A.shape) != tuple(n + 2 for n in ni):
        raise ValueError(f"args.ΔT must be ni {ni} or ni .+ 2, got {tuple(A.shape)}")
    return A[tuple(slice(0, n) for n in ni)]


def thermal_source_Q(phases, ratio_c, dT, ni):
    """Q' = α_c * ΔT: the volumetric source that, at a power-of-two dt, makes the isothermal form compute what the thermal form computes"""
    return fn_ratio(phase_alpha(phases), ratio_c, early_return=True) * own_index(dT, ni)


def compute_P(P, P0, divV, Q, eta, K, G, dt, r, theta_dtau, dT=None, alpha=None):
    """(RP, P) of _compute_P!; with dT (and alpha) the thermal form"""
    T = P.dtype.type
    dt, r, theta_dtau = T(dt), T(r), T(theta_dtau)
    _Kdt, _Gdt, _dt = T(1) / (K * dt), T(1) / (G * dt), T(1) / dt
    if dT is None:
        rhs = -divV + (Q * _dt)
    else:
        rhs = (-divV + (alpha * (dT * _dt))) + (Q * _dt)
    RP = -(P - P0) * _Kdt + rhs
    psi = T(1) / (T(1) / eta + _Gdt) * r / theta_dtau
    Pn = ((P0 * _Kdt + rhs) * psi + P) / (T(1) + _Kdt * psi)
    return RP, Pn


def maxloc(eta):
    """compute_maxloc!(ητ, η): maximum over the clamped 3^N window"""
    out = eta.copy()
    for ax in range(eta.ndim):
        lo = np.concatenate([np.take(out, [0], axis=ax), np.take(out, range(0, out.shape[ax] - 1), axis=ax)], axis=ax)
        hi = np.concatenate([np.take(out, range(1, out.shape[ax]), axis=ax), np.take(out, [out.shape[ax] - 1], axis=ax)], axis=ax)
        out = np.maximum(out, np.maximum(lo, hi))
    return out


def div_strain2d(Vx, Vy, _di):
    """∇V, ε.xx, ε.yy (ni) and ε.xy (ni .+ 1) from Vx (nx+1, ny+2), Vy (nx+2, ny+1)"""
    T = Vx.dtype.type
    _dx, _dy = T(_di[0]), T(_di[1])
    dxi = (-Vx[:-1, 1:-1] + Vx[1:, 1:-1]) * _dx
    dyi = (-Vy[1:-1, :-1] + Vy[1:-1, 1:]) * _dy
    divV = dxi + dyi
    d3 = divV * (T(1) / T(3))
    exy = T(0.5) * (_dy * (Vx[:, 1:] - Vx[:, :-1]) + _dx * (Vy[1:, :] - Vy[:-1, :]))
    return divV, dict(exx=dxi - d3, eyy=dyi - d3, exy=exy)


def div_strain3d(Vx, Vy, Vz, _di):
    """∇V, the normal strain rates (ni) and the shear ones on the edges from Vx (nx+1, ny+2, nz+2), Vy (nx+2, ny+1, nz+2), Vz (nx+2, ny+2, nz+1)"""
    T = Vx.dtype.type
    _dx, _dy, _dz = T(_di[0]), T(_di[1]), T(_di[2])
    dxi = (-Vx[:-1, 1:-1, 1:-1] + Vx[1:, 1:-1, 1:-1]) * _dx
    dyi = (-Vy[1:-1, :-1, 1:-1] + Vy[1:-1, 1:, 1:-1]) * _dy
    dzi = (-Vz[1:-1, 1:-1, :-1] + Vz[1:-1, 1:-1, 1:]) * _dz
    divV = dxi + dyi + dzi
    d3 = divV * (T(1) / T(3))
    eyz = T(0.5) * (_dz * (Vy[1:-1, :, 1:] - Vy[1:-1, :, :-1]) + _dy * (Vz[1:-1, 1:, :] - Vz[1:-1, :-1, :]))
    exz = T(0.5) * (_dz * (Vx[:, 1:-1, 1:] - Vx[:, 1:-1, :-1]) + _dx * (Vz[1:, 1:-1, :] - Vz[:-1, 1:-1, :]))
    exy = T(0.5) * (_dy * (Vx[:, 1:, 1:-1] - Vx[:, :-1, 1:-1]) + _dx * (Vy[1:, :, 1:-1] - Vy[:-1, :, 1:-1]))
    return divV, dict(exx=dxi - d3, eyy=dyi - d3, ezz=dzi - d3, eyz=eyz, exz=exz, exy=exy)


def pre_pass(a, phases, _di, dt, r, theta_dtau, dT=None):
    """What jrx_vep2d_compute_P / jrx_vep3d_compute_P leave: θ, RP, ∇V and ε from a = dict(theta, P0, Q, eta, phase_c, Vx, Vy[, Vz]).
    Returns dict(theta, RP, divV, exx, ...)."""
    ni = a["theta"].shape
    T = a["theta"].dtype.type
    if len(ni) == 2:
        divV, eps = div_strain2d(a["Vx"], a["Vy"], _di)
    else:
        divV, eps = div_strain3d(a["Vx"], a["Vy"], a["Vz"], _di)
    K = fn_ratio([T(ph["Kb"]) for ph in phases], a["phase_c"])
    G = fn_ratio([T(ph["G"]) for ph in phases], a["phase_c"])
    kw = {}
    if dT is not None:
        kw = dict(dT=own_index(dT, ni), alpha=fn_ratio([T(x) for x in phase_alpha(phases)], a["phase_c"], early_return=True))
    RP, th = compute_P(a["theta"], a["P0"], divV, a["Q"], maxloc(a["eta"]), K, G, dt, r, theta_dtau, **kw)
    return dict(theta=th, RP=RP, divV=divV, **eps)


def astype(a, T):
    return {k: (v.astype(T) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
