"""NumPy restatement of the 3D variational Stokes solver, written from the reference's sources: src/variational_stokes/mask.jl:180-186,220-269,324-392 (isvalid_c,
isvalid_vx / _vy / _vz, isvalid_yz / _xz / _xy), VelocityKernels.jl:6-12,96-154 (compute_∇V!, compute_strain_rate! 3D), StressKernels.jl:173-508
(update_stresses_center_vertex! 3D) with the clamped stencils of src/stokes/StressKernels.jl:604-668, Stokes3D.jl:14-238 (_solve_VS!), and -- shared with the 2D
restatement tests/_variational_stokes.py, which this file imports -- correct_phase_ratio, compute_phase_viscosity, compute_P!, fn_ratio.

The momentum kernel is NOT the reference's text (VelocityKernels.jl:408-487 cannot run: undefined averages, differences across two planes, a read past τxy).  It is the
masked 2D kernel (:355-399) one dimension up, on the index triples of the unmasked 3D kernel (src/stokes/VelocityKernels.jl:215-238), as include/jrx.h states it:
every operand times the ϕ member of its own location at its own index, ητ unmasked, terms in the order τ normal, τ shear, τ shear, -∇P, -body force.

Arrays are Julia-shaped (x first); indices here are 0-based.  Names follow jrx_vep3d_fields; phase ratios are (nphase, ...).  NumPy has no fused multiply-add.
"""
import numpy as np

import _variational_stokes as vs2

rock_ratio, update_rock_ratio, isvalid, pt_tuple = vs2.rock_ratio, vs2.update_rock_ratio, vs2.isvalid, vs2.pt_tuple
correct_phase_ratio = vs2.correct_phase_ratio

EDGES = ("yz", "xz", "xy")


# ---------------------------------------------------------------- mask.jl, 3D
def isvalid_c(phi, i, j, k):
    return (isvalid(phi["Vx"], i, j, k) and isvalid(phi["Vx"], i + 1, j, k) and isvalid(phi["Vy"], i, j, k) and isvalid(phi["Vy"], i, j + 1, k)
            and isvalid(phi["Vz"], i, j, k) and isvalid(phi["Vz"], i, j, k + 1) and isvalid(phi["center"], i, j, k))


def isvalid_yz(phi, i, j, k):
    ny, nz = phi["Vz"].shape[1], phi["Vy"].shape[2]
    return (isvalid(phi["vertex"], i, j, k) and isvalid(phi["vertex"], i + 1, j, k)
            and isvalid(phi["Vz"], i, max(j - 1, 0), k) and isvalid(phi["Vz"], i, min(j, ny - 1), k)
            and isvalid(phi["Vy"], i, j, max(k - 1, 0)) and isvalid(phi["Vy"], i, j, min(k, nz - 1)))


def isvalid_xz(phi, i, j, k):
    nx, nz = phi["Vz"].shape[0], phi["Vx"].shape[2]
    return (isvalid(phi["vertex"], i, j, k) and isvalid(phi["vertex"], i, j + 1, k)
            and isvalid(phi["Vz"], max(i - 1, 0), j, k) and isvalid(phi["Vz"], min(i, nx - 1), j, k)
            and isvalid(phi["Vx"], i, j, max(k - 1, 0)) and isvalid(phi["Vx"], i, j, min(k, nz - 1)))


def isvalid_xy(phi, i, j, k):
    ny, nx = phi["Vx"].shape[1], phi["Vy"].shape[0]
    return (isvalid(phi["vertex"], i, j, k) and isvalid(phi["vertex"], i, j, k + 1)
            and isvalid(phi["Vx"], i, max(j - 1, 0), k) and isvalid(phi["Vx"], i, min(j, ny - 1), k)
            and isvalid(phi["Vy"], max(i - 1, 0), j, k) and isvalid(phi["Vy"], min(i, nx - 1), j, k))


def isvalid_vx(phi, i, j, k): return isvalid(phi["Vx"], i, j, k)
def isvalid_vy(phi, i, j, k): return isvalid(phi["Vy"], i, j, k)
def isvalid_vz(phi, i, j, k): return isvalid(phi["Vz"], i, j, k)


def valid_masks(phi):
    """the seven predicates over the whole grid: c ni, yz / xz / xy on the edge arrays, vx / vy / vz on the velocity members"""
    vx, vy, vz, vt = phi["Vx"] > 0, phi["Vy"] > 0, phi["Vz"] > 0, phi["vertex"] > 0
    nx, ny, nz = phi["center"].shape
    lo = lambda n: np.maximum(np.arange(n + 1) - 1, 0)
    hi = lambda n: np.minimum(np.arange(n + 1), n - 1)
    il, ir, jl, jr, kl, kr = lo(nx), hi(nx), lo(ny), hi(ny), lo(nz), hi(nz)
    c = vx[:-1] & vx[1:] & vy[:, :-1] & vy[:, 1:] & vz[:, :, :-1] & vz[:, :, 1:] & (phi["center"] > 0)
    yz = vt[:-1] & vt[1:] & vz[:, jl, :] & vz[:, jr, :] & vy[:, :, kl] & vy[:, :, kr]
    xz = vt[:, :-1] & vt[:, 1:] & vz[il] & vz[ir] & vx[:, :, kl] & vx[:, :, kr]
    xy = vt[:, :, :-1] & vt[:, :, 1:] & vx[:, jl] & vx[:, jr] & vy[il] & vy[ir]
    return dict(c=c, yz=yz, xz=xz, xy=xy, vx=vx, vy=vy, vz=vz)


# ---------------------------------------------------------------- clamped stencils (src/stokes/StressKernels.jl:604-668)
# entries pick the clamped index {0: n-1, 1: n, 2: n+1} per direction, in the reference's order of summation; family T = 0 (yz), 1 (xz), 2 (xy)
CEN = [[(1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)],            # av_clamped_yz
       [(0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1)],            # av_clamped_xz
       [(0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]]            # av_clamped_xy
OTH = {(0, 1): [(1, 0, 1), (2, 0, 1), (1, 1, 1), (2, 1, 1)],    # av_clamped_yz_y (the xz array at a yz node)
       (0, 2): [(1, 1, 0), (2, 1, 0), (1, 1, 1), (2, 1, 1)],    # av_clamped_yz_z
       (1, 0): [(0, 1, 1), (1, 1, 1), (1, 2, 1), (0, 2, 1)],    # av_clamped_xz_x
       (1, 2): [(1, 1, 0), (1, 2, 0), (1, 1, 1), (1, 2, 1)],    # av_clamped_xz_z
       (2, 0): [(0, 1, 1), (1, 1, 1), (0, 1, 2), (1, 1, 2)],    # av_clamped_xy_x
       (2, 1): [(1, 0, 1), (1, 1, 1), (1, 0, 2), (1, 1, 2)]}    # av_clamped_xy_y


def _box(ni, T):
    return tuple(n + (1 if d != T else 0) for d, n in enumerate(ni))


def _terms(A, ni, T, table):
    """the four operands A[clamped indices] of a stencil over the node box of family T; every index is clamped to the CELL range [0, n-1], whatever array A is"""
    box = _box(ni, T)
    out = []
    for code in table:
        idx = [np.clip(np.arange(box[d]) + (code[d] - 1), 0, ni[d] - 1) for d in range(3)]
        out.append(A[np.ix_(*idx)])
    return out


def _av4(t):
    return 0.25 * (t[0] + t[1] + t[2] + t[3])


def _harm4(t):
    return 4 / (1 / t[0] + 1 / t[1] + 1 / t[2] + 1 / t[3])


# ---------------------------------------------------------------- the return mapping shared by an edge and a centre (6 components: xx, yy, zz, yz, xz, xy)
def _sinv3(t):
    return np.sqrt(0.5 * (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) + t[3] * t[3] + t[4] * t[4] + t[5] * t[5])


def _node_update(phases, r, P, tij, toij, eij, eta, lam, dt, th, rel):
    """returns (τ_new (6), λ_new, ε_pl (6), yielding, dQdP, K, τII); Drucker-Prager phases without softening"""
    pl, sinphi, cosphi, sinpsi = vs2._plastic_tables(phases)
    with np.errstate(all="ignore"):
        G = vs2._ratio_sum([ph["G"] for ph in phases], r)
        K = vs2._ratio_sum([ph["Kb"] for ph in phases], r)
        _Gdt = 1.0 / (G * dt)
        is_pl = any(pl)
        eta_reg = np.zeros(r.shape[1:])
        for q, ph in enumerate(phases):
            if pl[q]:
                eta_reg = eta_reg + ph.get("eta_vp", 0.0) * r[q]
        dtr = 1.0 / (th + eta * _Gdt + 1.0)
        d = [vs2._stress_inc(tij[q], toij[q], eta, eij[q], _Gdt, dtr) for q in range(6)]
        tt = [tij[q] + d[q] for q in range(6)]
        tII = _sinv3([d[q] + tij[q] for q in range(6)])
        ttII = _sinv3(tt)
        g = [0.5 * tt[q] / ttII for q in range(3)] + [0.5 * (tt[q] / ttII) for q in range(3, 6)]
        dQdt = [np.zeros_like(tII) for _ in range(6)]
        dQdP, dFdP, F = np.zeros_like(tII), np.zeros_like(tII), np.zeros_like(tII)
        for q, ph in enumerate(phases):
            on = r[q] != 0.0
            if pl[q]:
                for s in range(6):
                    dQdt[s] = np.where(on, r[q] * g[s] + dQdt[s], dQdt[s])
                dQdP = np.where(on, r[q] * -sinpsi[q] + dQdP, dQdP)
                dFdP = np.where(on, r[q] * -sinphi[q] + dFdP, dFdP)
                Fq = tII - cosphi[q] * ph["C"] - sinphi[q] * P
            else:
                Fq = tII
            F = np.where(on, F + r[q] * Fq, F)
        vol = np.where(np.isinf(K), 0.0, K * dt * dFdP * dQdP)
        yld = is_pl & (tII != 0.0) & (F > 0)
        lam_new = np.where(yld, (1.0 - rel) * lam + rel * (np.maximum(F, 0.0) / (eta * dtr + eta_reg + vol)), lam)
        epl = [np.where(yld, lam_new * dQdt[q], 0.0) for q in range(6)]
        dd = [np.where(yld, d[q] - 2.0 * eta * epl[q] * dtr, d[q]) for q in range(6)]
        tnew = [dd[q] + tij[q] for q in range(6)]
        tII_out = np.where(yld, _sinv3(tnew), tII)
    return tnew, lam_new, epl, yld, dQdP, K, tII_out


# ---------------------------------------------------------------- the kernels
def compute_divV_strain(a, phi, _di):
    """compute_∇V! + compute_strain_rate! 3D (VelocityKernels.jl:6-12,96-154): ∇V is zeroed at an invalid centre, the strain rates are left as they were at
    invalid nodes"""
    m = valid_masks(phi)
    _dx, _dy, _dz = _di
    Vx, Vy, Vz = a["Vx"], a["Vy"], a["Vz"]
    dxi = (-Vx[:-1, 1:-1, 1:-1] + Vx[1:, 1:-1, 1:-1]) * _dx
    dyi = (-Vy[1:-1, :-1, 1:-1] + Vy[1:-1, 1:, 1:-1]) * _dy
    dzi = (-Vz[1:-1, 1:-1, :-1] + Vz[1:-1, 1:-1, 1:]) * _dz
    a["divV"][...] = np.where(m["c"], dxi + dyi + dzi, 0.0)
    d3 = a["divV"] * (1.0 / 3.0)
    a["exx"][...] = np.where(m["c"], dxi - d3, a["exx"])
    a["eyy"][...] = np.where(m["c"], dyi - d3, a["eyy"])
    a["ezz"][...] = np.where(m["c"], dzi - d3, a["ezz"])
    a["eyz"][...] = np.where(m["yz"], 0.5 * (_dz * (Vy[1:-1, :, 1:] - Vy[1:-1, :, :-1]) + _dy * (Vz[1:-1, 1:, :] - Vz[1:-1, :-1, :])), a["eyz"])
    a["exz"][...] = np.where(m["xz"], 0.5 * (_dz * (Vx[:, 1:-1, 1:] - Vx[:, 1:-1, :-1]) + _dx * (Vz[1:, 1:-1, :] - Vz[:-1, 1:-1, :])), a["exz"])
    a["exy"][...] = np.where(m["xy"], 0.5 * (_dy * (Vx[:, 1:, 1:-1] - Vx[:, :-1, 1:-1]) + _dx * (Vy[1:, :, 1:-1] - Vy[:-1, :, 1:-1])), a["exy"])


def _s2c(yz, xz, xy):
    """the gathers of an edge tensor at the centres, in the reference's order of summation (k outer, j, i inner)"""
    return ([yz[:, :-1, :-1], yz[:, 1:, :-1], yz[:, :-1, 1:], yz[:, 1:, 1:]],
            [xz[:-1, :, :-1], xz[1:, :, :-1], xz[:-1, :, 1:], xz[1:, :, 1:]],
            [xy[:-1, :-1, :], xy[1:, :-1, :], xy[:-1, 1:, :], xy[1:, 1:, :]])


def update_stresses(a, phi, theta, lam, lamv, phases, dt, th, rel=0.2):
    """update_stresses_center_vertex! 3D (StressKernels.jl:173-508).  Every block reads the stresses as they were before the call (the reference's single launch
    races); the centre block's zeros of ε_pl on the edges land after the edge blocks' writes.  lamv: [λv_yz, λv_xz, λv_xy].  Returns the yielding masks."""
    m = valid_masks(phi)
    ni = a["P"].shape
    nx, ny, nz = ni
    old = {k: a[k].copy() for k in ("txx", "tyy", "tzz", "tyz", "txz", "txy")}
    res, ylds = [], {}
    for T, name in enumerate(EDGES):
        cen = lambda A: _av4(_terms(A, ni, T, CEN[T]))
        with np.errstate(all="ignore"):
            etav = _harm4(_terms(a["eta"], ni, T, CEN[T]))
        comp = {}
        for pre, src in (("e", a), ("t", old), ("to", a)):
            v = [cen(src[pre + "xx"]), cen(src[pre + "yy"]), cen(src[pre + "zz"])]
            for s, sh in enumerate(EDGES):
                v.append(src[pre + sh] if s == T else _av4(_terms(src[pre + sh], ni, T, OTH[(T, s)])))
            comp[pre] = v
        tn, ln, epl, yld, _, _, _ = _node_update(phases, a["phase_" + name], cen(theta), comp["t"], comp["to"], comp["e"], etav, lamv[T], dt, th, rel)
        res.append((tn[3 + T], ln, epl[3 + T]))
        ylds[name] = yld
    # ---- centre, from the old stresses
    g = _s2c(a["eyz"], a["exz"], a["exy"])
    eij = [a["exx"], a["eyy"], a["ezz"]] + [0.25 * ((((0.0 + t[0]) + t[1]) + t[2]) + t[3]) for t in g]
    tij = [old["txx"], old["tyy"], old["tzz"], a["tyz_c"].copy(), a["txz_c"].copy(), a["txy_c"].copy()]
    toij = [a["toxx"], a["toyy"], a["tozz"], a["toyz_c"], a["toxz_c"], a["toxy_c"]]
    tn, ln, epl, yld, dQdP, K, tII = _node_update(phases, a["phase_c"], theta, tij, toij, eij, a["eta"], lam, dt, th, rel)
    ylds["c"] = yld
    # ---- stores: edge blocks first
    for T, name in enumerate(EDGES):
        v = m[name]
        a["t" + name][...] = np.where(v, res[T][0], 0.0)              # τ += dτ at a valid edge, zero at an invalid one
        lamv[T][...] = np.where(v, res[T][1], lamv[T])
        a["epl" + name][...] = np.where(v, res[T][2], a["epl" + name])
    c = m["c"]
    lam[...] = np.where(c, ln, lam)
    a["evol_pl"][...] = np.where(c, np.where(yld, -lam * dQdP, 0.0), 0.0)
    for q, k in enumerate(("txx", "tyy", "tzz", "tyz_c", "txz_c", "txy_c")):
        a[k][...] = np.where(c, tn[q], 0.0)
    for q, k in enumerate(("eplxx", "eplyy", "eplzz")):
        a[k][...] = np.where(c, epl[q], 0.0)
    for name in EDGES:                                                 # ε_pl[4..6][I...] = 0 at an invalid centre: the edge arrays at the centre's own index
        a["epl" + name][:nx, :ny, :nz][~c] = 0.0
    a["tII"][...] = np.where(c, tII, a["tII"])                        # not written at an invalid centre
    with np.errstate(all="ignore"):
        a["eta_vep"][...] = np.where(c, tII * 0.5 * (1.0 / _sinv3(eij)), 0.0)
        a["P"][...] = np.where(c, theta - np.where(np.isinf(K), 0.0, K * dt * lam * dQdP), 0.0)
    return ylds


def compute_V(a, phi, etatau, eta_dtau, _di):
    """the masked momentum kernel in the form include/jrx.h states (see the module docstring)"""
    m = valid_masks(phi)
    _dx, _dy, _dz = _di
    pc = phi["center"]
    P, txx, tyy, tzz = a["P"] * pc, a["txx"] * pc, a["tyy"] * pc, a["tzz"] * pc
    tyz, txz, txy = a["tyz"] * phi["yz"], a["txz"] * phi["xz"], a["txy"] * phi["xy"]
    fx, fy, fz = a["fx"] * pc, a["fy"] * pc, a["fz"] * pc
    et = etatau
    R = ((-txx[:-1] + txx[1:]) * _dx + (-txy[1:-1, :-1, :] + txy[1:-1, 1:, :]) * _dy + (-txz[1:-1, :, :-1] + txz[1:-1, :, 1:]) * _dz
         - (-P[:-1] + P[1:]) * _dx - (fx[:-1] + fx[1:]) * 0.5)
    ok = m["vx"][1:-1]
    a["Rx"][...] = np.where(ok, R, 0.0)
    V = a["Vx"][1:-1, 1:-1, 1:-1]
    V[...] = np.where(ok, V + R * eta_dtau / ((et[:-1] + et[1:]) * 0.5), 0.0)
    R = ((-tyy[:, :-1] + tyy[:, 1:]) * _dy + (-txy[:-1, 1:-1, :] + txy[1:, 1:-1, :]) * _dx + (-tyz[:, 1:-1, :-1] + tyz[:, 1:-1, 1:]) * _dz
         - (-P[:, :-1] + P[:, 1:]) * _dy - (fy[:, :-1] + fy[:, 1:]) * 0.5)
    ok = m["vy"][:, 1:-1]
    a["Ry"][...] = np.where(ok, R, 0.0)
    V = a["Vy"][1:-1, 1:-1, 1:-1]
    V[...] = np.where(ok, V + R * eta_dtau / ((et[:, :-1] + et[:, 1:]) * 0.5), 0.0)
    R = ((-tzz[:, :, :-1] + tzz[:, :, 1:]) * _dz + (-txz[:-1, :, 1:-1] + txz[1:, :, 1:-1]) * _dx + (-tyz[:, :-1, 1:-1] + tyz[:, 1:, 1:-1]) * _dy
         - (-P[:, :, :-1] + P[:, :, 1:]) * _dz - (fz[:, :, :-1] + fz[:, :, 1:]) * 0.5)
    ok = m["vz"][:, :, 1:-1]
    a["Rz"][...] = np.where(ok, R, 0.0)
    V = a["Vz"][1:-1, 1:-1, 1:-1]
    V[...] = np.where(ok, V + R * eta_dtau / ((et[:, :, :-1] + et[:, :, 1:]) * 0.5), 0.0)


# ---------------------------------------------------------------- viscosity, buoyancy, the unmasked pieces
def compute_viscosity(a, phases, nu, cutoff, air_phase=0):
    """compute_viscosity! / update_viscosity_τII! 3D for LinearViscous phases (centres only in 3D)"""
    vs2.compute_viscosity(a, phases, nu, cutoff, air_phase)


def compute_viscosity_fields(a, phases, nu, cutoff, air_phase, tau, T):
    """compute_viscosity_kernel! 3D (Viscosity.jl:455-503) for laws that read fields, with the air_phase correction: the invariant of @stress / @strain with the
    shear components gathered from the cell's twelve edges (eps() on the normal components of a tensor whose normals vanish), P and T (ni) at the cell"""
    pre = "t" if tau else "e"
    xx, yy, zz = a[pre + "xx"], a[pre + "yy"], a[pre + "zz"]
    a0 = np.where((xx == 0.0) & (yy == 0.0) & (zz == 0.0), np.finfo(float).eps, 0.0)
    x, y, z = xx + a0, yy + -a0 * 0.5, zz + -a0 * 0.5
    sq = [0.25 * (t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3]) for t in _s2c(a[pre + "yz"], a[pre + "xz"], a[pre + "xy"])]
    AII = np.sqrt(0.5 * (x * x + y * y + z * z) + sq[0] + sq[1] + sq[2])
    c = vs2._correct_all(a["phase_c"], air_phase)
    xs, dom, has = np.zeros(AII.shape), np.zeros(AII.shape), np.zeros(AII.shape, dtype=bool)
    for q, law in enumerate(phases):
        with np.errstate(all="ignore"):
            v = vs2._law_viscosity(law, AII, T, a["P"], tau)
            first = ~has & (c[q] > 0.999)
            dom, has = np.where(first, v, dom), has | first
            xs = xs + np.where(c[q] != 0.0, (1.0 / v) * c[q], 0.0)
    with np.errstate(all="ignore"):
        e = np.where(has, dom, 1.0 / xs)
        e = e * nu + a["eta"] * (1.0 - nu)
    a["eta"][...] = np.minimum(np.maximum(e, cutoff[0]), cutoff[1])


def compute_rhog(a, phases):
    """compute_ρg!(ρg, phase_ratios, rheology, args), ConstantDensity, gravity along z: fn_ratio with the ratio == 1 shortcut"""
    r = a["phase_c"]
    x = np.zeros(r.shape[1:])
    for q, ph in enumerate(phases):
        x = x + np.where(r[q] == 0.0, 0.0, ph["density"]["rho0"] * r[q])
    for q in reversed(range(len(phases))):
        x = np.where(r[q] == 1.0, phases[q]["density"]["rho0"] * r[q], x)
    a["fz"][...] = x * float(phases[0].get("g", 0.0))


def maxloc(eta):
    out = np.full(eta.shape, -np.inf)
    idx = [[np.clip(np.arange(n) + d, 0, n - 1) for d in (-1, 0, 1)] for n in eta.shape]
    for K in idx[2]:
        for J in idx[1]:
            for I in idx[0]:
                out = np.maximum(out, eta[np.ix_(I, J, K)])
    return out


def free_slip(a):
    """flow_bcs! with free slip on the six faces, face groups in the reference's source order (free_slip.jl:15-70): front / back, top / bot, left / right"""
    Vx, Vy, Vz = a["Vx"], a["Vy"], a["Vz"]
    Vx[:, 0, :] = Vx[:, 1, :]; Vz[:, 0, :] = Vz[:, 1, :]
    Vx[:, -1, :] = Vx[:, -2, :]; Vz[:, -1, :] = Vz[:, -2, :]
    Vx[:, :, 0] = Vx[:, :, 1]; Vy[:, :, 0] = Vy[:, :, 1]
    Vx[:, :, -1] = Vx[:, :, -2]; Vy[:, :, -1] = Vy[:, :, -2]
    Vy[0, :, :] = Vy[1, :, :]; Vz[0, :, :] = Vz[1, :, :]
    Vy[-1, :, :] = Vy[-2, :, :]; Vz[-1, :, :] = Vz[-2, :, :]


def solve_VS(a, phi, phases, pt, _di, dt, *, air_phase=0, iterMax, nout, viscosity_cutoff=(-np.inf, np.inf), viscosity_relaxation=1.0e-2, **_):
    """_solve_VS! 3D (Stokes3D.jl:14-238), one block, free-slip velocity boundary conditions.  pt: (r, θ_dτ, ηdτ, ϵ_rel, ϵ_abs).  No iterMin, the norms over all
    nodes, relλ = 0.2."""
    r, th, eta_dtau, eps_rel, eps_abs = pt
    nx, ny, nz = a["P"].shape
    den = np.sqrt((nx - 1) * (ny - 1) * (nz - 1))
    err_it1, err = 1.0, np.inf
    it = 0
    hist = dict(err_evo1=[], err_evo2=[], norm_Rx=[], norm_Ry=[], norm_Rz=[], norm_divV=[])
    a["P0"][...] = a["P"]
    theta = a["P"].copy(order="F")
    lam = np.zeros((nx, ny, nz), order="F")
    lamv = [np.zeros(a["t" + k].shape, order="F") for k in EDGES]
    if any(ph.get("density") is not None for ph in phases):
        compute_rhog(a, phases)
    compute_viscosity(a, phases, 1.0, viscosity_cutoff, air_phase)
    K = vs2._ratio_sum([ph["Kb"] for ph in phases], a["phase_c"])
    G = vs2._ratio_sum([ph["G"] for ph in phases], a["phase_c"])

    def keep_going():
        with np.errstate(invalid="ignore", divide="ignore"):
            return it < 2 or (((err / err_it1) > eps_rel and err > eps_abs) and it <= iterMax)
    while keep_going():
        etatau = maxloc(a["eta"])
        compute_divV_strain(a, phi, _di)
        vs2.compute_P(a, theta, etatau, K, G, dt, r, th)
        compute_viscosity(a, phases, viscosity_relaxation, viscosity_cutoff, air_phase)
        update_stresses(a, phi, theta, lam, lamv, phases, dt, th, 0.2)
        compute_V(a, phi, etatau, eta_dtau, _di)
        for c in "xyz":
            a["U" + c][...] = a["V" + c] * dt
        free_slip(a)
        it += 1
        if it % nout == 0 and it > 1:
            e = [np.sqrt(np.sum(a[k][1:-1, 1:-1, 1:-1] ** 2)) / den for k in ("Rx", "Ry", "Rz")] + [np.sqrt(np.sum(a["RP"] ** 2)) / a["RP"].size]
            err = max(e)
            for k, v in zip(("norm_Rx", "norm_Ry", "norm_Rz", "norm_divV"), e):
                hist[k].append(v)
            hist["err_evo1"].append(err)
            hist["err_evo2"].append(it)
            err_it1 = max(hist[k][0] for k in ("norm_Rx", "norm_Ry", "norm_Rz", "norm_divV"))
            if np.isnan(err):
                raise FloatingPointError("NaN(s)")
    # epilogue (Stokes3D.jl:210-225)
    Vx, Vy, Vz = a["Vx"], a["Vy"], a["Vz"]
    _dx, _dy, _dz = _di
    a["omega_yz"][...] = 0.5 * ((-Vz[:nx, :ny + 1, :] + Vz[:nx, 1:ny + 2, :]) * _dy - (-Vy[:nx, :, :nz + 1] + Vy[:nx, :, 1:nz + 2]) * _dz)
    a["omega_xz"][...] = 0.5 * ((-Vx[:, :ny, :nz + 1] + Vx[:, :ny, 1:nz + 2]) * _dz - (-Vz[:nx + 1, :ny, :] + Vz[1:nx + 2, :ny, :]) * _dx)
    a["omega_xy"][...] = 0.5 * ((-Vy[:nx + 1, :, :nz] + Vy[1:nx + 2, :, :nz]) * _dx - (-Vx[:, :ny + 1, :nz] + Vx[:, 1:ny + 2, :nz]) * _dy)
    for pre in ("e", "epl", "de"):
        if pre + "yz" in a and pre + "yz_c" in a:
            for name, t in zip(EDGES, _s2c(a[pre + "yz"], a[pre + "xz"], a[pre + "xy"])):
                a[pre + name + "_c"][...] = 0.25 * (t[0] + t[1] + t[2] + t[3])
    sq = [0.25 * (t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3]) for t in _s2c(a["eplyz"], a["eplxz"], a["eplxy"])]
    a["EII_pl"][...] += np.sqrt(0.5 * (a["eplxx"] ** 2 + a["eplyy"] ** 2 + a["eplzz"] ** 2) + sq[0] + sq[1] + sq[2]) * dt
    a["EVol_pl"][...] += dt * a["evol_pl"]
    for k in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        a["to" + k][...] = a["t" + k]
    hist["iter"] = it
    return hist


# ---------------------------------------------------------------- test states
def randomize(s, seed=4, Kb=3.0, psi=6.0):
    """the `_randomize` recipe of tests/test_gpu_vep3d.py: every input of the stress kernel non-trivial, yielding and non-yielding nodes, mixed phase ratios, dilatant
    plasticity with a finite bulk modulus.  Returns the phases."""
    rng = np.random.default_rng(seed)
    a = s.arrays
    for pre in ("e", "t", "to"):
        for c in ("xx", "yy", "zz", "yz", "xz", "xy"):
            a[pre + c][...] = rng.uniform(-2.0, 2.0, size=a[pre + c].shape)
    for k in ("P", "tyz_c", "txz_c", "txy_c", "toyz_c", "toxz_c", "toxy_c"):
        a[k][...] = rng.uniform(-2.0, 2.0, size=a[k].shape)
    a["eta"][...] = 10.0 ** rng.uniform(-1.0, 0.5, size=a["eta"].shape)
    for k in ("phase_c", "phase_yz", "phase_xz", "phase_xy"):
        r = rng.uniform(0.0, 1.0, size=a[k].shape[1:])
        r[rng.uniform(size=r.shape) < 0.3] = 0.0
        r[rng.uniform(size=r.shape) < 0.3] = 1.0
        a[k][0], a[k][1] = r, 1.0 - r
    return [dict(ph, Kb=Kb, psi_deg=psi) for ph in s.extra["phases"][:2]]


def random_phi3(ni, seed=7):
    """a rock ratio with every predicate true on 20-80 % of its nodes and fractional values in every member: rock below a randomly tilted plane
    z < 0.55 + a (x - 1/2) + b (y - 1/2), a, b ~ U(-0.4, 0.4) in unit coordinates, ϕ ramping linearly 0 -> 1 across one cell thickness, then 4 % of each
    member set independently to 0 and 4 % to 1"""
    rng = np.random.default_rng(seed)
    phi = rock_ratio(*ni)
    nx, ny, nz = ni
    ca, cb = rng.uniform(-0.4, 0.4, size=2)
    xc, yc, zc = [(np.arange(n) + 0.5) / n for n in ni]
    xv, yv, zv = [np.arange(n + 1) / n for n in ni]
    loc = dict(center=(xc, yc, zc), vertex=(xv, yv, zv), Vx=(xv, yc, zc), Vy=(xc, yv, zc), Vz=(xc, yc, zv), yz=(xc, yv, zv), xz=(xv, yc, zv), xy=(xv, yv, zc))
    for k, (xs, ys, zs) in loc.items():
        X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
        surf = 0.55 + ca * (X - 0.5) + cb * (Y - 0.5)
        x = np.clip((surf - Z) * nz + 0.5, 0.0, 1.0)          # 1 half a cell below the plane, 0 half a cell above it
        u = rng.uniform(size=x.shape)
        x[u < 0.04] = 0.0
        x[u > 0.96] = 1.0
        phi[k][...] = x
    return phi
