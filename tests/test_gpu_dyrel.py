"""GPU parity tests of the 2D DYREL solver (csrc/dyrel2d.hip) against its NumPy restatement (tests/_dyrel.py), which tests/test_dyrel_restatement.py pins to
the reference's own kernel tests.  Tolerance rule: the restatement is evaluated twice on the same inputs, in float64 and in np.longdouble; per output array the
bound is 16 x the largest difference between the two, relative to the array's max-norm (the restatement's own rounding spread; 16 covers the fma / non-fma
orderings), x the iteration count for the driver.  Values that are one IEEE operation chain on both sides (masks, copies, the β = 0 identity) are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _dyrel as dy

pytestmark = pytest.mark.gpu

SIZES = [(6, 5), (67, 35), (3, 3)]          # the reference's own; across a wave boundary in x and a block boundary in y; the smallest grid accepted
VEP_MAP = dict(P="P", P0="P0", divV="divV", Q="Q", Vx="V.Vx", Vy="V.Vy", exx="ε.xx", eyy="ε.yy", exy="ε.xy", exy_c="ε.xy_c", eplxx="ε_pl.xx", eplyy="ε_pl.yy",
               eplxy="ε_pl.xy", eplxy_c="ε_pl.xy_c", txx="τ.xx", tyy="τ.yy", txy="τ.xy", txy_c="τ.xy_c", tII="τ.II", toxx="τ_o.xx", toyy="τ_o.yy", toxy="τ_o.xy",
               toxy_c="τ_o.xy_c", eta="viscosity.η", eta_v="viscosity.ηv", eta_vep="viscosity.η_vep", EII_pl="EII_pl", evol_pl="ε_vol_pl", EVol_pl="EVol_pl",
               RP="R.RP", Rx="R.Rx", Ry="R.Ry", omega_xy="ω.xy", txx_v="τ.xx_v", tyy_v="τ.yy_v", toxx_v="τ_o.xx_v", toyy_v="τ_o.yy_v", lam="λ", lamv="λv", dPpsi="ΔPψ")
DY_MAP = dict(gamma_eff="γ_eff", etab="ηb", P_num="P_num", Dx="Dx", Dy="Dy", lmaxVx="λmaxVx", lmaxVy="λmaxVy", dVxdtau="dVxdτ", dVydtau="dVydτ", dtauVx="dτVx",
              dtauVy="dτVy", dVx="dVx", dVy="dVy", betaVx="βVx", betaVy="βVy", cVx="cVx", cVy="cVy", alphaVx="αVx", alphaVy="αVy", Rx0="Rx0", Ry0="Ry0")


def _get(o, path):
    for p in path.split("."):
        o = getattr(o, p)
    return o


class Dev:
    """a host state (a, d) uploaded into StokesArrays, PhaseRatios, DYREL, with the C structs of the entry points"""

    def __init__(self, jr, a, d, phases, di, dt, bcs="free_slip", periodic=False, **kw):
        import torch
        from justrelax_jl_amd import _lib, dyrel as dmod, stokes as smod
        from justrelax_jl_amd.arrays import from_numpy
        self.jr, self.dmod = jr, dmod
        ni = a["P"].shape
        dev = torch.device("cuda", torch.cuda.current_device())
        self.st = jr.StokesArrays(jr.AMDGPUBackend, ni)
        for k, path in VEP_MAP.items():
            _get(self.st, path).copy_(from_numpy(a[k], dev))
        self.pr = jr.PhaseRatios(jr.AMDGPUBackend, a["phase_c"].shape[0], ni)
        self.pr.center.copy_(from_numpy(a["phase_c"], dev))
        self.pr.vertex.copy_(from_numpy(a["phase_v"], dev))
        self.ρg = (from_numpy(a["fx"], dev), from_numpy(a["fy"], dev))
        self.dy = jr.DYREL(jr.AMDGPUBackend, ni, **{k: v for k, v in kw.items() if k in ("ϵ", "CFL", "c_fact")})
        for k, name in DY_MAP.items():
            getattr(self.dy, name).copy_(from_numpy(d[k], dev))
        on = dict(left=True, right=True, top=True, bot=True)
        off = {k: False for k in on}
        sides = dict(off, left=True, right=True) if periodic else off          # periodic in x, the kind named on the other two faces
        kind = {k: not sides[k] for k in on}
        self.bcs = jr.VelocityBoundaryConditions(free_slip=kind if bcs == "free_slip" else off, no_slip=kind if bcs == "no_slip" else off,
                                                 periodic=sides) if bcs else None
        self.h = _lib.default_handle()
        self.f = smod.vep_fields2d(self.st, self.ρg, self.pr)
        self.d = dmod.dyrel_fields2d(self.dy, self.st)
        self.p = dmod.grid_params2d(self.st, di, dt, self.bcs)
        self.rh = smod.rheology_table(phases)
        self.phases, self.di, self.dt = phases, di, dt

    def q(self, **kw):
        return self.dmod.dyrel_params2d(self.dy, **kw)

    def download(self):
        a = {k: self.jr.to_numpy(_get(self.st, path)) for k, path in VEP_MAP.items()}
        a["fx"], a["fy"] = self.jr.to_numpy(self.ρg[0]), self.jr.to_numpy(self.ρg[1])
        d = {k: self.jr.to_numpy(getattr(self.dy, name)) for k, name in DY_MAP.items()}
        return a, d


def _close(name, got, f64, ld, factor=16.0):
    scale = float(np.max(np.abs(f64))) or 1.0
    bound = factor * float(np.max(np.abs(f64.astype(np.longdouble) - ld))) / scale
    err = float(np.max(np.abs(got - f64))) / scale
    print(f"{name}: |gpu - f64| = {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound, (name, err, bound)


def _both(a, d, fn):
    """fn on a float64 copy and on a longdouble copy of (a, d)"""
    out = []
    for T in (np.float64, np.longdouble):
        aa, dd = dy.astype(a, T), dy.astype(d, T)
        extra = fn(aa, dd)
        out.append((aa, dd, extra))
    return out


@pytest.mark.parametrize("ni", SIZES)
@pytest.mark.parametrize("case", ["nonlinear", "linear_viscosity", "no_yield"])
def test_kernels_match_restatement(jr, ni, case):
    """every per-kernel entry point on the randomised state"""
    a, d, phases, di, dt = dy.random_state(ni, yielding=case != "no_yield")
    lin = case == "linear_viscosity"
    _di = (1.0 / di[0], 1.0 / di[1])
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
        for k in exact:
            assert np.array_equal(ga[k], a64[k]), (name, k)
        written = set(keys_a) | set(keys_d) | set(exact)
        for k in a64:          # nothing else is touched
            if k not in written and k in ga:
                assert np.array_equal(ga[k], a[k]), (name, k, "written")
        for k in d64:
            if k not in written:
                assert np.array_equal(gd[k], d[k]), (name, k, "written")
        a, d = {**a64, **{k: ga[k] for k in ga}}, gd          # continue from the device's values on both sides
        return x64

    step("bulk", lambda: h.call("jrx_dyrel2d_bulk_viscosity_and_penalty", C.byref(g.f), C.byref(g.d), C.byref(g.rh), C.byref(g.p), C.c_double(20.0)),
         lambda aa, dd: dy.bulk_viscosity_and_penalty(aa, dd, phases, 20.0, dt), keys_d=("etab", "gamma_eff"))
    step("gershgorin", lambda: h.call("jrx_dyrel2d_gershgorin", C.byref(g.f), C.byref(g.d), C.byref(g.rh), C.byref(g.p)),
         lambda aa, dd: dy.gershgorin(aa, dd, phases, di, dt), keys_d=("Dx", "Dy", "lmaxVx", "lmaxVy"))
    step("dtau", lambda: jr.update_dτV_α_β_(g.dy), lambda aa, dd: dy.update_dtauV_alpha_beta(dd, 0.99),
         keys_d=("dtauVx", "dtauVy", "betaVx", "betaVy", "alphaVx", "alphaVy"))
    step("alpha_beta", lambda: jr.update_α_β_(g.dy), lambda aa, dd: dy.update_alpha_beta(dd), keys_d=("betaVx", "betaVy", "alphaVx", "alphaVy"))
    step("strain_rp", lambda: h.call("jrx_dyrel2d_strain_rate_RP", C.byref(g.f), C.byref(g.d), C.byref(g.p), C.c_int32(1)),
         lambda aa, dd: dy.strain_rate_RP(aa, dd, _di, dt, True), keys_a=("exx", "eyy", "exy", "RP"))
    a["P"] = a["P"] + 0.125          # the do_strain_rate = false form: only RP moves
    g.st.P.add_(0.125)
    step("rp_only", lambda: h.call("jrx_dyrel2d_strain_rate_RP", C.byref(g.f), C.byref(g.d), C.byref(g.p), C.c_int32(0)),
         lambda aa, dd: dy.strain_rate_RP(aa, dd, _di, dt, False), keys_a=("RP",))
    # ---- stress and viscosity, with the yield branch
    diag = {}
    a_in = {k: v.copy() for k, v in a.items()}

    def stress(aa, dd):
        dg = {}
        dy.stress_viscosity(aa, dd, phases, 0.7, dt, 0.3, (1.0e-2, 5.0), lin, diag=dg)
        diag[aa["P"].dtype.type] = dg
    outs = ("txx", "tyy", "txy_c", "txx_v", "tyy_v", "txy", "eplxx", "eplyy", "eplxy", "evol_pl", "tII", "eta_vep", "lam", "lamv", "dPpsi") + (() if lin else ("eta", "eta_v"))
    step("stress", lambda: h.call("jrx_dyrel2d_stress_viscosity", C.byref(g.f), C.byref(g.d), C.byref(g.rh), C.byref(g.p), C.byref(qp), C.c_double(0.7)),
         stress, keys_a=outs, keys_d=("P_num",))
    if lin:
        assert np.array_equal(a["eta"], a_in["eta"]) and np.array_equal(a["eta_v"], a_in["eta_v"])
    # the set of yielding nodes, exactly, away from F = 0 (phase 1 is the plastic one; rel > 0: λ_phase > 0 exactly where it yields)
    total = excluded = 0
    for key, lamk, rk in (("Fc", "lam", "phase_c"), ("Fv", "lamv", "phase_v")):
        (_, F64, y64), (_, FL, _) = diag[np.float64][key][0], diag[np.longdouble][key][0]
        live = ~np.isnan(F64)
        scale = float(np.max(np.abs(F64[live]))) if live.any() else 1.0
        tol = 16.0 * float(np.max(np.abs(F64[live].astype(np.longdouble) - FL[live]))) if live.any() else 0.0
        near = live & (np.abs(F64) <= max(tol, 16 * np.finfo(float).eps * scale))
        # the restatement's yield mask on the device's own inputs: one phase of the sum is plastic, so λ_out > 0 iff that phase yields with a positive multiplier
        aa = dy.astype(a_in, np.float64)
        dd = dy.astype(d, np.float64)
        dy.stress_viscosity(aa, dd, phases, 0.7, dt, 0.3, (1.0e-2, 5.0), lin)
        want, got = aa[lamk] > 0, a[lamk] > 0
        keep = ~near
        assert np.array_equal(want[keep], got[keep]), key
        total += live.size
        excluded += int(near.sum())
        if case == "no_yield":
            assert not y64.any() and not got.any()
        elif min(ni) > 3:
            assert y64.any() and not y64[live].all()
    print(f"yield set: {excluded} of {total} nodes within the bound of F = 0")
    assert excluded <= 0.01 * total
    step("ph_residual", lambda: h.call("jrx_dyrel2d_PH_residual", C.byref(g.f), C.byref(g.d), C.byref(g.p)),
         lambda aa, dd: dy.ph_residual(aa, _di), keys_a=("Rx", "Ry"))
    step("dr_update", lambda: h.call("jrx_dyrel2d_DR_residual_update_V", C.byref(g.f), C.byref(g.d), C.byref(g.p)),
         lambda aa, dd: dy.dr_residual_update_V(aa, dd, _di), keys_a=("Rx", "Ry", "Vx", "Vy"), keys_d=("dVxdtau", "dVydtau"))
    # β = 0: the velocities do not move, bit for bit (test_dyrel_kernels.jl:168-191)
    g.dy.βVx.zero_()
    g.dy.βVy.zero_()
    V0 = (jr.to_numpy(g.st.V.Vx), jr.to_numpy(g.st.V.Vy))
    h.call("jrx_dyrel2d_DR_residual_update_V", C.byref(g.f), C.byref(g.d), C.byref(g.p))
    assert np.array_equal(jr.to_numpy(g.st.V.Vx), V0[0]) and np.array_equal(jr.to_numpy(g.st.V.Vy), V0[1])


def _budget_state(ni, bc):
    """the shear band with a dilation angle; under no-slip walls nothing drives it through the boundary, so there it starts at rest under a body force
    (a heavier inclusion)"""
    a, phases, di, dt = dy.shearband_state(*ni, psi_deg=5.0)
    if bc == "no_slip":
        a["Vx"][...] = 0.0
        a["Vy"][...] = 0.0
        a["fy"][...] = -(1.0 + 4.0 * a["phase_c"][1])
        a["fx"][...] = 0.5 * a["phase_c"][1]
    return a, phases, di, dt


def _budget_run(jr, ni, bc):
    a, phases, di, dt = _budget_state(ni, bc)
    d = dy.new_dyrel(ni)
    g = Dev(jr, a, d, phases, di, dt, bcs=bc, ϵ=0.0)
    out = jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, di, dt,
                          kwargs=dict(nout=10, iterMax=11, total_iterMax=30, verbose_PH=False, verbose_DR=False))
    return out, g.download()


@pytest.mark.parametrize("bc", ["free_slip", "no_slip"])
@pytest.mark.parametrize("ni", SIZES[:2])
def test_driver_fixed_budget(jr, ni, bc):
    """ϵ = 0, nout = 10, total_iterMax = 30 (iterMax = 11 ends each velocity solve after 12 iterations): the same counts and history lengths as the restatement,
    every array of StokesArrays and of the DYREL struct within 16 x the iteration count x the restatement's spread, and two runs bit-identical.  Free-slip and
    no-slip walls: after the first flow_bcs! the update kernel refreshes the ghosts itself, v or -v"""
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
    assert np.abs(ga["Vx"][1:-1, 1:-1]).max() > 0 and np.abs(ga["Vy"][1:-1, 1:-1]).max() > 0
    if bc == "no_slip":          # the ghosts mirror the first interior row / column with the sign flipped, bit for bit
        assert np.array_equal(ga["Vx"][1:-1, 0], -ga["Vx"][1:-1, 1]) and np.array_equal(ga["Vx"][1:-1, -1], -ga["Vx"][1:-1, -2])
        assert np.array_equal(ga["Vy"][0, 1:-1], -ga["Vy"][1, 1:-1]) and np.array_equal(ga["Vy"][-1, 1:-1], -ga["Vy"][-2, 1:-1])
        assert not ga["Vx"][0].any() and not ga["Vx"][-1].any() and not ga["Vy"][:, 0].any() and not ga["Vy"][:, -1].any()
    for k in ga:
        _close(f"driver.{k}", ga[k], a64[k], aL[k], factor=16.0 * h64["iter"])
    for k in gd:
        _close(f"driver.{k}", gd[k], d64[k], dL[k], factor=16.0 * h64["iter"])
    out2, (ga2, gd2) = _budget_run(jr, ni, bc)
    assert all(np.array_equal(ga[k], ga2[k], equal_nan=True) for k in ga) and all(np.array_equal(gd[k], gd2[k]) for k in gd)
    assert np.array_equal(out.err_evo_tot, out2.err_evo_tot)


@pytest.mark.parametrize("case", ["elastic", "yielding"])
def test_driver_converges_on_the_shear_band(jr, case):
    """the 32 x 32 shear band of test/test_shearband2D_DYREL.jl, one time step with its keywords and the default ϵ: the solve ends before total_iterMax, the
    Powell-Hestenes residual of the returned fields (evaluated by the restatement, in the driver's own norm: relative to the first / second iteration's
    residuals of the restatement's run) is below ϵ, and the epilogue agrees with the grid-operator entry points.

    `elastic` is the reference's set-up, in whose first step nothing yields (C cos ϕ = 1.6 against a load of 0.4): λ, ΔPψ and EII_pl stay zero there.
    `yielding` lowers C cos ϕ to 0.39, just below that load, with Ψ = 10°: some 400 of the 1024 centres yield, so ΔPψ, ε_pl and EII_pl are non-zero and the
    checks of P, of EII_pl against accumulate_tensor! and of ε_pl.xy_c against shear2center! carry weight.  The restatement needs about 4900 iterations for
    that solve (13 s in NumPy), so there it runs only its first two Powell-Hestenes iterations, which define the reference norms."""
    ni, eps = (32, 32), 1.0e-6
    kw = dict(nout=50, rel_drop=0.5, viscosity_relaxation=1, linear_viscosity=True, iterMax=50.0e3)
    sb = dict(psi_deg=10.0, C_cos=0.39) if case == "yielding" else {}
    a, phases, di, dt = dy.shearband_state(*ni, **sb)
    d = dy.new_dyrel(ni)
    g = Dev(jr, a, d, phases, di, dt)
    out = jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, di, dt, kwargs=dict(kw, verbose_PH=False, verbose_DR=False))
    assert 0 < out.iter < 50_000 and out.itPH < 1000
    assert out.err_evo_tot[-1] < 1.0 and len(out.err_evo_it) == out.iter // 50
    ga, gd = g.download()
    # the driver's reference residuals (first iteration for V, second for P), from the restatement's own run of the same solve
    ar, dr = dy.shearband_state(*ni, **sb)[0], dy.new_dyrel(ni)
    _di = (1.0 / di[0], 1.0 / di[1])
    href = dy.solve_DYREL(ar, dr, phases, di, dt, itPH_max=2 if case == "yielding" else 1000, **kw)
    eV0, eP0 = href["errV0"], href["errPt0"]
    if case == "elastic":
        assert abs(out.iter - href["iter"]) <= 100 and abs(out.itPH - href["itPH"]) <= 1
    # the residual of the returned fields: P has absorbed ΔPψ, so the momentum balance takes P alone and the pressure residual P - ΔPψ
    b = dict(ga)
    b["dPpsi"] = np.zeros_like(ga["P"])
    dy.ph_residual(b, _di)
    b["P"] = ga["P"] - ga["dPpsi"]
    dy.strain_rate_RP(b, gd, _di, dt)
    eV, eP = dy.ph_norms(b)
    err = max(min(eV[0] / eV0[0], eV[0]), min(eV[1] / eV0[1], eV[1]), min(eP / eP0, eP))
    nyield = int((ga["lam"] > 0).sum())
    print(f"iter {out.iter}, itPH {out.itPH}, PH residual of the returned fields {err:.3e}; {nyield} centres yield, max |ΔPψ| = {np.abs(ga['dPpsi']).max():.3e}, "
          f"max EII_pl = {ga['EII_pl'].max():.3e}")
    assert err < eps
    if case == "yielding":
        assert 100 < nyield < 1024 and np.abs(ga["dPpsi"]).max() > 1.0e-2 and ga["EII_pl"].max() > 1.0e-2 and np.abs(ga["eplxy_c"]).max() > 0
        # without the absorbed ΔPψ the pressure residual of the same fields is far above ϵ: the check above does see it
        b["P"] = ga["P"]
        dy.strain_rate_RP(b, gd, _di, dt)
        assert min(dy.ph_norms(b)[1] / eP0, dy.ph_norms(b)[1]) > 100 * eps
    else:
        assert nyield == 0
    # epilogue: τ_o = τ (with xx_v, yy_v), shear2center!, accumulate_tensor! through the existing entry points on the same arrays.  Bit for bit: the
    # epilogue kernel and those operators evaluate the same expression in the same order under the same compiler flags
    for k in ("xx", "yy", "xy", "xy_c", "xx_v", "yy_v"):
        assert np.array_equal(ga["to" + k], ga["t" + k]), k
    import torch
    E = torch.zeros_like(g.st.EII_pl)
    jr.accumulate_tensor_(E, g.st.ε_pl, dt)
    assert np.array_equal(jr.to_numpy(E), ga["EII_pl"])
    for T in (g.st.ε, g.st.ε_pl):
        xy_c = jr.to_numpy(T.xy_c).copy()
        T.xy_c.zero_()
        jr.shear2center_(T)
        assert np.array_equal(jr.to_numpy(T.xy_c), xy_c)


def test_refusals(jr):
    """every refusal returns JRX_ERR_ARG with a text naming its cause, and launches nothing"""
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.arrays import fzeros
    ni = (6, 5)
    a, phases, di, dt = dy.shearband_state(*ni)
    g = Dev(jr, a, dy.new_dyrel(ni), phases, di, dt)
    h = g.h
    kw = dict(nout=10, iterMax=5, total_iterMax=5, verbose_PH=False, verbose_DR=False)

    def refused(text, fn):
        n0 = h.get_option("stat_dyrel_launches")
        with pytest.raises(_lib.JrxError) as e:
            fn()
        assert e.value.status == 4 and text in str(e.value), str(e.value)
        assert h.get_option("stat_dyrel_launches") == n0

    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    refused("RockRatio", lambda: jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, di, dt, kwargs=kw, ϕ=ϕ))
    refused("RockRatio", lambda: jr.DYREL_(g.dy, g.st, phases, g.pr, ϕ, di, dt))
    xv, yv = np.linspace(0, 1, 7) ** 1.2, np.linspace(0, 1, 6)
    refused("non-uniform", lambda: jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, jr.Geometry.from_vertices((xv, yv)), dt, kwargs=kw))
    cap = [dict(p) for p in phases]
    cap[0]["cap"] = dict(kind="cap")
    refused("is_pl", lambda: jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, cap, None, di, dt, kwargs=kw))
    refused("is_pl", lambda: jr.DYREL_(g.dy, g.st, cap, g.pr, di, dt))
    dT = fzeros((8, 7), g.st.P.device)
    refused("ΔT", lambda: jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, {"ΔT": dT}, di, dt, kwargs=kw))
    refused("melt_fraction", lambda: jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, {"melt_fraction": fzeros(ni, g.st.P.device)}, di, dt, kwargs=kw))
    gp = Dev(jr, a, dy.new_dyrel(ni), phases, di, dt, periodic=True)
    refused("periodic", lambda: jr.solve_DYREL_(gp.st, gp.ρg, gp.dy, gp.bcs, gp.pr, phases, None, di, dt, kwargs=kw))
    small = jr.StokesArrays(jr.AMDGPUBackend, (2, 5))
    refused("at least 3 cells", lambda: jr.DYREL(jr.AMDGPUBackend, small, phases, jr.PhaseRatios(jr.AMDGPUBackend, 2, (2, 5)), di, dt))
    # a handle with a communicator: one process, two handles joined as a 2 x 1 x 1 group
    hs = [_lib.Handle(0), _lib.Handle(0)]
    try:
        carts = (_lib.Cart * 2)()
        n3 = (C.c_int64 * 3)(6, 5, 1)
        dims = (C.c_int32 * 3)(2, 1, 1)
        per = (C.c_int32 * 3)(0, 0, 0)
        for r in range(2):
            assert hs[0].lib.jrx_cart_create(C.c_int32(r), C.c_int32(2), n3, dims, per, C.byref(carts[r])) == 0
        hp = (C.c_void_p * 2)(hs[0]._h, hs[1]._h)
        assert hs[0].lib.jrx_comm_init_local(hp, C.c_int32(2), carts) == 0, hs[0].lib.jrx_last_error(hs[0]._h)
        n0 = hs[0].get_option("stat_dyrel_launches")
        with pytest.raises(_lib.JrxError) as e:
            jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, di, dt, kwargs=kw, handle=hs[0])
        assert e.value.status == 4 and "communicator" in str(e.value)
        assert hs[0].get_option("stat_dyrel_launches") == n0
    finally:
        for x in hs:
            x.close()
    # and the accepted call next to them does launch
    n0 = h.get_option("stat_dyrel_launches")
    jr.DYREL_(g.dy, g.st, phases, g.pr, di, dt)
    assert h.get_option("stat_dyrel_launches") == n0 + 5
