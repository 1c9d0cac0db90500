"""GPU parity tests of the 3D DYREL solver (csrc/dyrel3d.hip) against its NumPy restatement (tests/_dyrel3d.py), which tests/test_dyrel3d_restatement.py pins to
the reference's allocator test, to exact fields, to the 2D restatement on plane-strain extrusions and to the assembled operator.  Tolerance rule, as in
tests/test_gpu_dyrel.py: the restatement is evaluated twice on the same inputs, in float64 and in np.longdouble; per output array the bound is 16 x the largest
difference between the two, relative to the array's max-norm, x the iteration count for the driver.  Masks, copies and the β = 0 identity are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _dyrel as dy2
import _dyrel3d as dy
from _variational_stokes3d import EDGES

pytestmark = pytest.mark.gpu

# the reference's allocator size; across a wave in x (64) and across the 4 rows of a block in y, several planes in z; the smallest grid accepted
SIZES = [(6, 5, 4), (67, 9, 5), (3, 3, 3)]
COMP = "xyz"
C6 = ("xx", "yy", "zz", "yz", "xz", "xy")
VEP_MAP = dict(P="P", P0="P0", divV="divV", Q="Q", Vx="V.Vx", Vy="V.Vy", Vz="V.Vz", eta="viscosity.η", eta_vep="viscosity.η_vep", EII_pl="EII_pl", evol_pl="ε_vol_pl",
               EVol_pl="EVol_pl", RP="R.RP", Rx="R.Rx", Ry="R.Ry", Rz="R.Rz", tII="τ.II", lam="λ", dPpsi="ΔPψ", omega_yz="ω.yz", omega_xz="ω.xz", omega_xy="ω.xy")
for _pre, _T in (("e", "ε"), ("epl", "ε_pl"), ("t", "τ"), ("to", "τ_o")):
    VEP_MAP.update({_pre + c: f"{_T}.{c}" for c in C6})
    VEP_MAP.update({_pre + c + "_c": f"{_T}.{c}_c" for c in EDGES})
DY_MAP = dict(gamma_eff="γ_eff", etab="ηb", P_num="P_num")
for _c in COMP:
    DY_MAP.update({f"D{_c}": f"D{_c}", f"lmaxV{_c}": f"λmaxV{_c}", f"dV{_c}dtau": f"dV{_c}dτ", f"dtauV{_c}": f"dτV{_c}", f"dV{_c}": f"dV{_c}", f"betaV{_c}": f"βV{_c}",
                   f"cV{_c}": f"cV{_c}", f"alphaV{_c}": f"αV{_c}", f"R{_c}0": f"R{_c}0"})


def _get(o, path):
    for p in path.split("."):
        o = getattr(o, p)
    return o


class Dev:
    """a host state (a, d) uploaded into StokesArrays, PhaseRatios, DYREL, with the C structs of the entry points"""

    def __init__(self, jr, a, d, phases, di, dt, bcs="free_slip", periodic=False, free_surface=False, **kw):
        import torch
        from justrelax_jl_amd import _lib, dyrel as dmod, stokes as smod
        from justrelax_jl_amd.arrays import from_numpy
        self.jr, self.dmod = jr, dmod
        ni = a["P"].shape
        dev = torch.device("cuda", torch.cuda.current_device())
        self.st = jr.StokesArrays(jr.AMDGPUBackend, ni)
        for k, path in VEP_MAP.items():
            if k in a:
                _get(self.st, path).copy_(from_numpy(a[k], dev))
        self.lv = dmod.edge_λv(self.st)
        for name in EDGES:
            getattr(self.lv, name).copy_(from_numpy(a["lamv_" + name], dev))
        self.pr = jr.PhaseRatios(jr.AMDGPUBackend, a["phase_c"].shape[0], ni)
        self.pr.center.copy_(from_numpy(a["phase_c"], dev))
        for name in EDGES:
            getattr(self.pr, name).copy_(from_numpy(a["phase_" + name], dev))
        self.ρg = tuple(from_numpy(a["f" + c], dev) for c in COMP)
        self.dy = jr.DYREL(jr.AMDGPUBackend, ni, **{k: v for k, v in kw.items() if k in ("ϵ", "CFL", "c_fact")})
        for k, name in DY_MAP.items():
            getattr(self.dy, name).copy_(from_numpy(d[k], dev))
        faces = ("left", "right", "front", "back", "top", "bot")
        off = {k: False for k in faces}
        sides = dict(off, left=True, right=True) if periodic else off
        kind = {k: not sides[k] for k in faces}
        self.bcs = jr.VelocityBoundaryConditions(free_slip=kind if bcs == "free_slip" else off, no_slip=kind if bcs == "no_slip" else off, periodic=sides,
                                                 free_surface=free_surface) if bcs else None
        self.h = _lib.default_handle()
        self.f = smod.vep_fields3d(self.st, self.ρg, self.pr)
        self.d = dmod.dyrel_fields3d(self.dy, self.st)
        self.p = dmod.grid_params3d(self.st, di, dt, self.bcs)
        self.rh = smod.rheology_table(phases)
        self.phases, self.di, self.dt = phases, di, dt

    def q(self, **kw):
        return self.dmod.dyrel_params2d(self.dy, **kw)

    def download(self):
        to = self.jr.to_numpy
        a = {k: to(_get(self.st, path)) for k, path in VEP_MAP.items()}
        for c, t in zip(COMP, self.ρg):
            a["f" + c] = to(t)
        for name in EDGES:
            a["lamv_" + name] = to(getattr(self.lv, name))
        d = {k: to(getattr(self.dy, name)) for k, name in DY_MAP.items()}
        return a, d


def _close(name, got, f64, ld, factor=16.0):
    scale = float(np.max(np.abs(f64))) or 1.0
    bound = factor * float(np.max(np.abs(f64.astype(np.longdouble) - ld))) / scale
    err = float(np.max(np.abs(got - f64))) / scale
    print(f"{name}: |gpu - f64| = {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound, (name, err, bound)


def _both(a, d, fn):
    out = []
    for T in (np.float64, np.longdouble):
        aa, dd = dy.astype(a, T), dy.astype(d, T)
        extra = fn(aa, dd)
        out.append((aa, dd, extra))
    return out


def _yield_cap(a_in, d, phases, dt, lin, diag, got):
    """the yield sets (centre and each edge family) equal the restatement's away from F = 0; returns (nodes left out, nodes)"""
    total = excluded = 0
    aa, dd = dy.astype(a_in, np.float64), dy.astype(d, np.float64)
    dy.stress_viscosity(aa, dd, phases, 0.7, dt, 0.3, (1.0e-2, 5.0), lin)
    for key, lamk in (("Fc", "lam"),) + tuple(("F" + n, "lamv_" + n) for n in EDGES):
        (_, F64, y64), (_, FL, _) = diag[np.float64][key][0], diag[np.longdouble][key][0]
        live = ~np.isnan(F64)
        scale = float(np.max(np.abs(F64[live]))) if live.any() else 1.0
        tol = 16.0 * float(np.max(np.abs(F64[live].astype(np.longdouble) - FL[live]))) if live.any() else 0.0
        near = live & (np.abs(F64) <= max(tol, 16 * np.finfo(float).eps * scale))
        if got is not None:
            want, have = aa[lamk] > 0, got[lamk] > 0
            assert np.array_equal(want[~near], have[~near]), key
        total += live.size
        excluded += int(near.sum())
    return excluded, total, diag[np.float64]


@pytest.mark.parametrize("ni", SIZES)
@pytest.mark.parametrize("case", ["nonlinear", "linear_viscosity", "no_yield"])
def test_kernels_match_restatement(jr, ni, case):
    """every per-kernel entry point on the randomised state; nothing else is written.  The seed of dy.random_state was chosen so that the restatement alone,
    float64 against longdouble, leaves at most 1 % of the nodes within the bound of F = 0 at every size (checked on the CPU: 0 nodes at each of SIZES)"""
    a, d, phases, di, dt = dy.random_state(ni, yielding=case != "no_yield")
    lin = case == "linear_viscosity"
    _di = tuple(1.0 / x for x in di)
    g = Dev(jr, a, d, phases, di, dt)
    h = g.h
    qp = g.q(viscosity_relaxation=0.3, viscosity_cutoff=(1.0e-2, 5.0), linear_viscosity=lin)

    def step(name, call, fn, keys_a=(), keys_d=(), exact=()):
        nonlocal a, d
        (a64, d64, x64), (aL, dL, _) = _both(a, d, fn)
        call()
        ga, gd = g.download()
        for k in keys_a:
            _close(f"{name}.{k}", ga[k], a64[k], aL[k])
        for k in keys_d:
            _close(f"{name}.{k}", gd[k], d64[k], dL[k])
        written = set(keys_a) | set(keys_d) | set(exact)
        for k in a64:          # nothing else is touched
            if k not in written and k in ga:
                assert np.array_equal(ga[k], a[k]), (name, k, "written")
        for k in d64:
            if k not in written:
                assert np.array_equal(gd[k], d[k]), (name, k, "written")
        a, d = {**a64, **{k: ga[k] for k in ga}}, gd          # continue from the device's values on both sides
        return x64

    step("bulk", lambda: h.call("jrx_dyrel3d_bulk_viscosity_and_penalty", C.byref(g.f), C.byref(g.d), C.byref(g.rh), C.byref(g.p), C.c_double(20.0)),
         lambda aa, dd: dy.bulk_viscosity_and_penalty(aa, dd, phases, 20.0, dt), keys_d=("etab", "gamma_eff"))
    step("gershgorin", lambda: h.call("jrx_dyrel3d_gershgorin", C.byref(g.f), C.byref(g.d), C.byref(g.rh), C.byref(g.p)),
         lambda aa, dd: dy.gershgorin(aa, dd, phases, di, dt), keys_d=("Dx", "Dy", "Dz", "lmaxVx", "lmaxVy", "lmaxVz"))
    abk = tuple(k + c for k in ("betaV", "alphaV") for c in COMP)
    step("dtau", lambda: jr.update_dτV_α_β_(g.dy), lambda aa, dd: dy.update_dtauV_alpha_beta(dd, 0.99), keys_d=("dtauVx", "dtauVy", "dtauVz") + abk)
    step("alpha_beta", lambda: jr.update_α_β_(g.dy), lambda aa, dd: dy.update_alpha_beta(dd), keys_d=abk)
    step("strain_rp", lambda: h.call("jrx_dyrel3d_strain_rate_RP", C.byref(g.f), C.byref(g.d), C.byref(g.p), C.c_int32(1)),
         lambda aa, dd: dy.strain_rate_RP(aa, dd, _di, dt, True), keys_a=tuple("e" + c for c in C6) + ("RP",))
    a["P"] = a["P"] + 0.125          # the do_strain_rate = false form: only RP moves
    g.st.P.add_(0.125)
    step("rp_only", lambda: h.call("jrx_dyrel3d_strain_rate_RP", C.byref(g.f), C.byref(g.d), C.byref(g.p), C.c_int32(0)),
         lambda aa, dd: dy.strain_rate_RP(aa, dd, _di, dt, False), keys_a=("RP",))
    # ---- stress and viscosity, with the yield branch
    diag = {}
    a_in = {k: v.copy() for k, v in a.items()}

    def stress(aa, dd):
        dg = {}
        dy.stress_viscosity(aa, dd, phases, 0.7, dt, 0.3, (1.0e-2, 5.0), lin, diag=dg)
        diag[aa["P"].dtype.type] = dg
    outs = (("txx", "tyy", "tzz", "tyz_c", "txz_c", "txy_c", "tyz", "txz", "txy", "eplxx", "eplyy", "eplzz", "eplyz", "eplxz", "eplxy", "evol_pl", "tII", "eta_vep",
             "lam", "lamv_yz", "lamv_xz", "lamv_xy", "dPpsi") + (() if lin else ("eta",)))
    step("stress", lambda: h.call("jrx_dyrel3d_stress_viscosity", C.byref(g.f), C.byref(g.d), C.byref(g.rh), C.byref(g.p), C.byref(qp), C.c_double(0.7)),
         stress, keys_a=outs, keys_d=("P_num",))
    if lin:
        assert np.array_equal(a["eta"], a_in["eta"])
    # the sets of yielding nodes, exactly, away from F = 0 (phase 1 is the plastic one; rel > 0: λ > 0 exactly where it yields)
    excluded, total, dg = _yield_cap(a_in, d, phases, dt, lin, diag, a)
    print(f"yield set: {excluded} of {total} nodes within the bound of F = 0")
    assert excluded <= 0.01 * total
    for key in ("Fc", "Fyz", "Fxz", "Fxy"):
        _, F64, y64 = dg[key][0]
        live = ~np.isnan(F64)
        if case == "no_yield":
            assert not y64.any()
        elif min(ni) > 3:
            assert y64.any() and not y64[live].all(), key
    step("ph_residual", lambda: h.call("jrx_dyrel3d_PH_residual", C.byref(g.f), C.byref(g.d), C.byref(g.p)),
         lambda aa, dd: dy.ph_residual(aa, _di), keys_a=("Rx", "Ry", "Rz"))
    step("dr_update", lambda: h.call("jrx_dyrel3d_DR_residual_update_V", C.byref(g.f), C.byref(g.d), C.byref(g.p)),
         lambda aa, dd: dy.dr_residual_update_V(aa, dd, _di), keys_a=("Rx", "Ry", "Rz", "Vx", "Vy", "Vz"), keys_d=("dVxdtau", "dVydtau", "dVzdtau"))
    # β = 0: the velocities do not move, bit for bit
    for c in COMP:
        getattr(g.dy, "βV" + c).zero_()
    V0 = [jr.to_numpy(getattr(g.st.V, "V" + c)) for c in COMP]
    h.call("jrx_dyrel3d_DR_residual_update_V", C.byref(g.f), C.byref(g.d), C.byref(g.p))
    assert all(np.array_equal(jr.to_numpy(getattr(g.st.V, "V" + c)), v) for c, v in zip(COMP, V0))


def _budget_state(ni, bc):
    """the shear band with a dilation angle and a cohesion just below the elastic load; under no-slip walls it starts at rest under a body force"""
    a, phases, di, dt = dy.shearband_state(*ni, psi_deg=5.0, C_cos=0.39, radius=0.25)
    if bc == "no_slip":
        for c in COMP:
            a["V" + c][...] = 0.0
        a["fz"][...] = -(1.0 + 4.0 * a["phase_c"][1])
        a["fx"][...] = 0.5 * a["phase_c"][1]
        a["fy"][...] = -0.25 * a["phase_c"][1]
    return a, phases, di, dt


def _budget_run(jr, ni, bc):
    a, phases, di, dt = _budget_state(ni, bc)
    g = Dev(jr, a, dy.new_dyrel(ni), phases, di, dt, bcs=bc, ϵ=0.0)
    out = jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, di, dt, kwargs=dict(nout=10, iterMax=11, total_iterMax=30, verbose_PH=False, verbose_DR=False))
    return out, g.download()


@pytest.mark.parametrize("bc", ["free_slip", "no_slip"])
@pytest.mark.parametrize("ni", SIZES[:2])
def test_driver_fixed_budget(jr, ni, bc):
    """ϵ = 0, nout = 10, iterMax = 11, total_iterMax = 30: the same counts and history lengths as the restatement, every array of StokesArrays and of the DYREL
    struct within 16 x the iteration count x the restatement's spread, two runs bit-identical, no-slip ghosts mirrored with the sign flipped bit for bit"""
    runs = []
    for T in (np.float64, np.longdouble):
        a, phases, di, dt = _budget_state(ni, bc)
        a, d = dy.astype(a, T), dy.new_dyrel(ni, T)
        hist = dy.solve_DYREL(a, d, phases, di, dt, eps=0.0, nout=10, iterMax=11, total_iterMax=30, free_slip=bc == "free_slip", no_slip=bc == "no_slip")
        runs.append((a, d, hist))
    (a64, d64, h64), (aL, dL, _) = runs
    out, (ga, gd) = _budget_run(jr, ni, bc)
    assert (out.iter, out.itPH) == (h64["iter"], h64["itPH"]) == (36, 3)
    for k in ("err_evo_it", "err_evo_V", "err_evo_P", "err_evo_tot"):
        assert len(getattr(out, k)) == len(h64[k]) == 3, k
    assert list(out.err_evo_it) == h64["err_evo_it"]
    np.testing.assert_allclose(out.err_evo_tot, h64["err_evo_tot"], rtol=1e-9)
    for c in COMP:
        assert np.abs(ga["V" + c][1:-1, 1:-1, 1:-1]).max() > 0
    if bc == "no_slip":
        for q, c in enumerate(COMP):
            V = ga["V" + c]
            for dim in range(3):
                lo, lo1, hi, hi1 = (np.take(V, k, axis=dim) for k in (0, 1, -1, -2))
                if dim == q:
                    assert not lo.any() and not hi.any()
                else:          # interior of the ghost plane: away from the other ghost lines
                    assert np.array_equal(lo[1:-1, 1:-1], -lo1[1:-1, 1:-1]) and np.array_equal(hi[1:-1, 1:-1], -hi1[1:-1, 1:-1])
    for k in ga:
        if k in a64:
            _close(f"driver.{k}", ga[k], a64[k], aL[k], factor=16.0 * h64["iter"])
    for k in gd:
        _close(f"driver.{k}", gd[k], d64[k], dL[k], factor=16.0 * h64["iter"])
    out2, (ga2, gd2) = _budget_run(jr, ni, bc)
    assert all(np.array_equal(ga[k], ga2[k], equal_nan=True) for k in ga) and all(np.array_equal(gd[k], gd2[k]) for k in gd)
    assert np.array_equal(out.err_evo_tot, out2.err_evo_tot)


KW = dict(nout=50, rel_drop=0.5, viscosity_relaxation=1, linear_viscosity=True, iterMax=50.0e3, verbose_PH=False, verbose_DR=False)


def test_driver_converges_on_the_3d_shear_band(jr):
    """a 24 x 24 x 12 shear band (spherical inclusion of radius 0.25, C cos ϕ = 0.39 just below the elastic load of 0.4, Ψ = 10°), one time step: the solve reaches
    ϵ = 1e-6 before total_iterMax, yields somewhere but not everywhere, and its epilogue agrees with the grid-operator entry points bit for bit"""
    ni = (24, 24, 12)
    a, phases, di, dt = dy.shearband_state(*ni, psi_deg=10.0, C_cos=0.39, radius=0.25)
    g = Dev(jr, a, dy.new_dyrel(ni), phases, di, dt)
    out = jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, di, dt, kwargs=KW)
    ga, gd = g.download()
    nyield = int((ga["lam"] > 0).sum())
    print(f"iter {out.iter}, itPH {out.itPH}, err_evo_tot[-1] = {out.err_evo_tot[-1]:.3e}, {nyield} of {ga['lam'].size} centres yield")
    assert 0 < out.iter < 50_000 and out.itPH < 1000 and len(out.err_evo_it) == out.iter // 50
    assert out.err_evo_tot[-1] < 1.0e-6
    assert 0 < nyield < ga["lam"].size and ga["EII_pl"].max() > 0
    assert all((ga["lamv_" + n] > 0).any() and not (ga["lamv_" + n] > 0).all() for n in ("xz",))
    for k in C6 + tuple(n + "_c" for n in EDGES):
        assert np.array_equal(ga["to" + k], ga["t" + k]), k
    import torch
    E = torch.zeros_like(g.st.EII_pl)
    jr.accumulate_tensor_(E, g.st.ε_pl, dt)
    assert np.array_equal(jr.to_numpy(E), ga["EII_pl"])
    for T in (g.st.ε, g.st.ε_pl):
        old = [jr.to_numpy(getattr(T, n + "_c")).copy() for n in EDGES]
        for n in EDGES:
            getattr(T, n + "_c").zero_()
        jr.shear2center_(T)
        assert all(np.array_equal(jr.to_numpy(getattr(T, n + "_c")), o) for n, o in zip(EDGES, old))


# max |Δ| / max |·| of V, P, τII between the 2D float64 restatement and every plane of the 3D float64 restatement of the extruded problem at this size and ϵ,
# measured on the CPU (see the docstring below): the bound of the GPU comparison is 10 x these
PLANE_MEASURED = dict(Vx=2.32e-5, Vz=8.13e-6, P=3.64e-4, tII=2.25e-4)


def test_plane_strain_extrusion_agrees_with_the_2d_driver(jr):
    """the 2D shear band of tests/_dyrel.py (16 x 16, inclusion of radius 0.1, C cos ϕ = 0.39, Ψ = 10°) against its extrusion over 3 cells along y: the out-of-plane
    velocity stays bit-zero, and V, P, τ.II of every plane agree with the 2D GPU driver's converged section, max |Δ| / max |·| per field within 10 x the value the
    two float64 restatements show at this size and ϵ (the margin covers the stopping iteration moving by one nout interval with the device's summation order).
    Measured on the CPU: the 2D restatement stops after 3600 iterations (72 Powell-Hestenes), the 3D one after 3550 (71) -- the 3D bound carries the η / dy² terms
    of the extruded direction, so the two take different steps to the same ϵ -- and differ by Vx 2.32e-5, Vz 8.13e-6, P 3.64e-4, τII 2.25e-4 (PLANE_MEASURED)."""
    import test_gpu_dyrel as t2
    n2 = (16, 16)
    a2, phases, di2, dt = dy2.shearband_state(*n2, psi_deg=10.0, C_cos=0.39)
    g2 = t2.Dev(jr, a2, dy2.new_dyrel(n2), phases, di2, dt)
    o2 = jr.solve_DYREL_(g2.st, g2.ρg, g2.dy, g2.bcs, g2.pr, phases, None, di2, dt, kwargs=KW)
    r2, _ = g2.download()
    ni = (16, 3, 16)
    a3, phases3, di3, _ = dy.shearband_state(*ni, psi_deg=10.0, C_cos=0.39, radius=0.1, axis=1)
    g3 = Dev(jr, a3, dy.new_dyrel(ni), phases3, di3, dt)
    o3 = jr.solve_DYREL_(g3.st, g3.ρg, g3.dy, g3.bcs, g3.pr, phases3, None, di3, dt, kwargs=KW)
    r3, _ = g3.download()
    print(f"2D: iter {o2.iter}, itPH {o2.itPH}; 3D: iter {o3.iter}, itPH {o3.itPH}")
    assert not r3["Vy"].any()          # bit-zero
    assert o2.err_evo_tot[-1] < 1.0e-6 and o3.err_evo_tot[-1] < 1.0e-6
    for k3, k2 in (("Vx", "Vx"), ("Vz", "Vy"), ("P", "P"), ("tII", "tII")):
        ref = r2[k2]
        planes = range(1, 4) if k3.startswith("V") else range(3)
        err = max(float(np.max(np.abs(np.take(r3[k3], j, axis=1) - ref))) for j in planes) / float(np.max(np.abs(ref)))
        print(f"{k3}: max |Δ| / max |·| = {err:.3e}, measured on the CPU {PLANE_MEASURED[k3]:.3e}")
        assert err <= 10.0 * PLANE_MEASURED[k3], (k3, err)


def test_allocating_constructor_equals_alloc_plus_init(jr):
    """DYREL(backend, stokes3d, ...) equals DYREL(backend, ni) followed by DYREL_, and launches exactly the init's kernels"""
    ni = (6, 5, 4)
    a, d, phases, di, dt = dy.random_state(ni)
    g = Dev(jr, a, dy.new_dyrel(ni), phases, di, dt)
    h = g.h
    n0 = h.get_option("stat_dyrel_launches")
    jr.DYREL_(g.dy, g.st, phases, g.pr, di, dt, CFL=0.8, γfact=15.0)
    n1 = h.get_option("stat_dyrel_launches")
    made = jr.DYREL(jr.AMDGPUBackend, g.st, phases, g.pr, di, dt, CFL=0.8, γfact=15.0)
    n2 = h.get_option("stat_dyrel_launches")
    assert n1 - n0 == n2 - n1 == 5          # eta sum, final sum, bulk, bound, dτ / α / β
    for name in DY_MAP.values():
        assert np.array_equal(jr.to_numpy(getattr(made, name)), jr.to_numpy(getattr(g.dy, name))), name
    assert made.CFL == 0.8 and (jr.to_numpy(made.Dz) > 0).all()


def test_refusals(jr):
    """every refusal returns JRX_ERR_ARG with a text naming its cause, and launches nothing; the accepted call next to them does launch"""
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.arrays import fzeros
    ni = (6, 5, 4)
    a, phases, di, dt = dy.shearband_state(*ni)
    g = Dev(jr, a, dy.new_dyrel(ni), phases, di, dt)
    h = g.h
    kw = dict(nout=10, iterMax=5, total_iterMax=5, verbose_PH=False, verbose_DR=False)

    def refused(text, fn, handle=h):
        n0 = handle.get_option("stat_dyrel_launches")
        with pytest.raises(_lib.JrxError) as e:
            fn()
        assert e.value.status == 4 and text in str(e.value), str(e.value)
        assert handle.get_option("stat_dyrel_launches") == n0

    solve = lambda gg=g, ph=phases, args=None, grid=di, **k: jr.solve_DYREL_(gg.st, gg.ρg, gg.dy, gg.bcs, gg.pr, ph, args, grid, dt, kwargs=kw, **k)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    refused("RockRatio", lambda: solve(ϕ=ϕ))
    refused("RockRatio", lambda: jr.DYREL_(g.dy, g.st, phases, g.pr, ϕ, di, dt))
    xv = [np.linspace(0, 1, n + 1) for n in ni]
    xv[0] = xv[0] ** 1.2
    refused("non-uniform", lambda: solve(grid=jr.Geometry.from_vertices(tuple(xv))))
    cap = [dict(p) for p in phases]
    cap[0]["cap"] = dict(kind="cap")
    refused("is_pl", lambda: solve(ph=cap))
    refused("is_pl", lambda: jr.DYREL_(g.dy, g.st, cap, g.pr, di, dt))
    refused("ΔT", lambda: solve(args={"ΔT": fzeros(ni, g.st.P.device)}))
    refused("melt_fraction", lambda: solve(args={"melt_fraction": fzeros(ni, g.st.P.device)}))
    refused("periodic", lambda: solve(gg=Dev(jr, a, dy.new_dyrel(ni), phases, di, dt, periodic=True)))
    refused("free_surface", lambda: solve(gg=Dev(jr, a, dy.new_dyrel(ni), phases, di, dt, free_surface=True)))
    small = jr.StokesArrays(jr.AMDGPUBackend, (5, 2, 4))
    refused("at least 3 cells", lambda: jr.DYREL(jr.AMDGPUBackend, small, phases, jr.PhaseRatios(jr.AMDGPUBackend, 2, (5, 2, 4)), di, dt))
    # 2^31 entries: the extents alone are checked before any pointer is read, so the arrays of the small state serve
    big = g.dmod.grid_params3d((2048, 1024, 1024), di, dt)
    refused("2^31", lambda: h.call("jrx_dyrel3d_strain_rate_RP", C.byref(g.f), C.byref(g.d), C.byref(big), C.c_int32(1)))
    # a handle with a communicator: one process, two handles joined as a 2 x 1 x 1 group
    hs = [_lib.Handle(0), _lib.Handle(0)]
    try:
        carts = (_lib.Cart * 2)()
        n3 = (C.c_int64 * 3)(*ni)
        dims = (C.c_int32 * 3)(2, 1, 1)
        per = (C.c_int32 * 3)(0, 0, 0)
        for r in range(2):
            assert hs[0].lib.jrx_cart_create(C.c_int32(r), C.c_int32(2), n3, dims, per, C.byref(carts[r])) == 0
        hp = (C.c_void_p * 2)(hs[0]._h, hs[1]._h)
        assert hs[0].lib.jrx_comm_init_local(hp, C.c_int32(2), carts) == 0, hs[0].lib.jrx_last_error(hs[0]._h)
        refused("communicator", lambda: solve(handle=hs[0]), handle=hs[0])
    finally:
        for x in hs:
            x.close()
    n0 = h.get_option("stat_dyrel_launches")
    jr.DYREL_(g.dy, g.st, phases, g.pr, di, dt)
    assert h.get_option("stat_dyrel_launches") == n0 + 5
