"""NumPy restatements of the four per-step operators of csrc/stepops.hip, written from the reference's texts: pureshear_bc!
(src/boundaryconditions/pure_shear.jl:1-33), free_surface_bcs! (src/boundaryconditions/free_surface.jl:1-99), subgrid_characteristic_time!
(src/particles/subgrid_diffusion.jl:36-50), compute_melt_fraction! (src/rheology/Melting.jl:10-35) and fn_ratio (src/phases/phases.jl:6-30).
Arrays are indexed [i, j[, k]] like Julia's [i+1, j+1[, k+1]]; phase ratios are (nphase, ni...).  Every function works in the dtype of its inputs
(float64, or np.longdouble for the tolerance rule) and keeps the reference's grouping: one rounding per written operation."""
import numpy as np

SENTINEL = -77.25


# ---------------------------------------------------------------- pure_shear.jl
def pureshear_bc2d(Vx, Vy, xci, xvi, εbg):
    """:4-5, the two comprehensions written out"""
    (xc, yc), (xv, yv) = xci, xvi
    Vx[:, 1:-1] = np.array([[εbg * x for y in yc] for x in xv])
    Vy[1:-1, :] = np.array([[-εbg * y for y in yv] for x in xc])


def pureshear_bc3d(Vx, Vy, Vz, xci, xvi, εbg):
    """the form the library builds: Vy from the y vertices, Vz over (xc, yc, zv)"""
    (xc, yc, zc), (xv, yv, zv) = xci, xvi
    Vx[:, 1:-1, 1:-1] = np.array([[[εbg * x for z in zc] for y in yc] for x in xv])
    Vy[1:-1, :, 1:-1] = np.array([[[εbg * y for z in zc] for y in yv] for x in xc])
    Vz[1:-1, 1:-1, :] = np.array([[[-εbg * z for z in zv] for y in yc] for x in xc])


def pureshear_bc3d_literal(Vx, Vy, Vz, xci, xvi, εbg):
    """:16-30 as the reference writes it: `y in xv` for Vy, `y in xc` for Vz (the shapes fit only when nx == ny)"""
    (xc, yc, zc), (xv, yv, zv) = xci, xvi
    Vx[:, 1:-1, 1:-1] = np.array([[[εbg * x for z in zc] for y in yc] for x in xv])
    Vy[1:-1, :, 1:-1] = np.array([[[εbg * y for z in zc] for y in xv] for x in xc])
    Vz[1:-1, 1:-1, :] = np.array([[[-εbg * z for z in zv] for y in xc] for x in xc])


# ---------------------------------------------------------------- phases.jl
def fn_ratio(vals, ratio):
    """:6-15, without args: x += iszero(r) ? 0 : fn(phase) r, phase by phase"""
    x = np.zeros(ratio.shape[1:], dtype=ratio.dtype)
    for q, v in enumerate(vals):
        x = x + np.where(ratio[q] == 0, 0, ratio.dtype.type(v) * ratio[q])
    return x


def fn_ratio_args(fns, ratio):
    """:17-30, with args: a ratio of exactly 1 returns fn(phase, args) r at once; fns[q] is fn(phase q, args) as an array or a number"""
    x = np.zeros(ratio.shape[1:], dtype=ratio.dtype)
    out = np.zeros_like(x)
    done = np.zeros(x.shape, dtype=bool)
    for q, f in enumerate(fns):
        r = ratio[q]
        fr = np.asarray(f, dtype=ratio.dtype) * r
        first = (r == 1) & ~done
        out = np.where(first, fr, out)
        done |= first
        x = x + np.where(r == 0, 0, fr)
    return np.where(done, out, x)


# ---------------------------------------------------------------- free_surface.jl
def free_surface_bcs2d(a, G, dt, dx, dy):
    """FreeSurface_Vy! :38-68 over i = 1..nx; a: Vx, Vy, P, P0, toyy, eta, phase_c; dx, dy: numbers or the vectors read at [i] / [end]"""
    T = a["Vy"].dtype.type
    nx = a["P"].shape[0]
    dxs = np.asarray(dx, dtype=T) if np.ndim(dx) else np.full(nx, dx, dtype=T)
    dyv = T(dy[-1] if np.ndim(dy) else dy)
    Gdt = fn_ratio(G, a["phase_c"][:, :, -1]) * T(dt)
    ν = T(1.0e-2)
    Vx, Vy = a["Vx"], a["Vy"]
    new = ν * (Vy[1:-1, -2] + (T(3) / T(2)) * (a["P"][:, -1] / (T(2.0) * a["eta"][:, -1]) + (a["toyy"][:, -1] + a["P0"][:, -1]) / (T(2.0) * Gdt) +
                                                 (T(1) / T(3.0)) * (Vx[1:, -2] - Vx[:-1, -2]) * (T(1) / dxs)) * dyv) + (T(1) - ν) * Vy[1:-1, -1]
    Vy[1:-1, -1] = new


def free_surface_bcs3d(a, G, dt, di, stress="toyy"):
    """FreeSurface_Vy! :70-99 over (i, j); reads τ_o.yy as the reference does (stress="tozz" is what it does NOT do)"""
    T = a["Vz"].dtype.type
    dx, dy, dz = (T(d) for d in di)
    Gdt = fn_ratio(G, a["phase_c"][:, :, :, -1]) * T(dt)
    Vx, Vy, Vz = a["Vx"], a["Vy"], a["Vz"]
    Vz[1:-1, 1:-1, -1] = Vz[1:-1, 1:-1, -2] + T(3.0) / T(2.0) * (
        a["P"][:, :, -1] / (T(2.0) * a["eta"][:, :, -1]) + (a[stress][:, :, -1] + a["P0"][:, :, -1]) / (T(2.0) * Gdt) +
        (T(1) / T(3.0)) * ((Vx[1:, 1:-1, -2] - Vx[:-1, 1:-1, -2]) * (T(1) / dx) + (Vy[1:-1, 1:, -2] - Vy[1:-1, :-1, -2]) * (T(1) / dy))) * dz


# ---------------------------------------------------------------- subgrid_diffusion.jl
def density(ph, T, P):
    d = ph.get("density", {})
    t = T.dtype.type
    if d.get("kind", "constant") == "constant":
        return np.full(T.shape, d.get("rho0", 0.0), dtype=T.dtype)
    assert d["kind"] == "PT"
    return t(d["rho0"]) * (t(1.0) - t(d["alpha"]) * (T - t(d.get("T0", 0.0))) + t(d.get("beta", 0.0)) * (P - t(d.get("P0", 0.0))))


def subgrid_characteristic_time(phase_c, table, Tghost, P, di):
    """:36-50: dt₀ = ρCp / (2 K Σ inv(dx)²), T = thermal.T[I .+ 1]"""
    t = P.dtype.type
    Tc = Tghost[tuple(slice(1, -1) for _ in P.shape)]
    ρCp = fn_ratio_args([t(ph["Cp"]) * density(ph, Tc, P) for ph in table], phase_c)
    K = fn_ratio_args([t(ph["k"]) for ph in table], phase_c)
    s = None
    for d in di:                                   # mapreduce(x -> inv(x)^2, +, di): left to right
        inv = t(1) / t(d)
        s = inv * inv if s is None else s + inv * inv
    return ρCp / (t(2) * K * s)


# ---------------------------------------------------------------- Melting.jl
def melt_law(ph, T):
    """kind None: no law (0); "caricchi": MeltingParam_Caricchi, 1 / (1 + exp((a - (T - c)) / b)), T in kelvin"""
    law = ph.get("melting")
    T = np.asarray(T)
    t = T.dtype.type
    if not law:
        return np.zeros(T.shape, dtype=T.dtype)
    assert law["kind"] == "caricchi"
    a, b, c = t(law.get("a", 800.0)), t(law.get("b", 23.0)), t(law.get("c", 273.15))
    return t(1.0) / (t(1.0) + np.exp((a - (T - c)) / b))


def compute_melt_fraction(shape, phase_c, table, T, dtype=np.float64):
    """:10-35; T a number or an array of `shape`; phase_c None: the single-material form (phase 1)"""
    Tf = np.broadcast_to(np.asarray(T, dtype=dtype), shape).astype(dtype)
    if phase_c is None:
        return melt_law(table[0], Tf)
    return fn_ratio_args([melt_law(ph, Tf) for ph in table], phase_c.astype(dtype))
