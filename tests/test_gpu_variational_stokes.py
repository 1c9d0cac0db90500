"""GPU parity tests of the 2D variational Stokes solver (csrc/stokes2d_vs.hip) against its NumPy restatement (tests/_variational_stokes.py), which
tests/test_variational_stokes_restatement.py pins to the reference's own tests and to the C oracle."""
import ctypes as C

import numpy as np
import pytest

import _variational_stokes as vs

pytestmark = pytest.mark.gpu

VEP_MAP = dict(P="P", P0="P0", divV="divV", Q="Q", Vx="V.Vx", Vy="V.Vy", Ux="U.Ux", Uy="U.Uy", exx="ε.xx", eyy="ε.yy", exy="ε.xy", exy_c="ε.xy_c",
               eplxx="ε_pl.xx", eplyy="ε_pl.yy", eplxy="ε_pl.xy", eplxy_c="ε_pl.xy_c", txx="τ.xx", tyy="τ.yy", txy="τ.xy", txy_c="τ.xy_c",
               tII="τ.II", toxx="τ_o.xx", toyy="τ_o.yy", toxy="τ_o.xy", toxy_c="τ_o.xy_c", eta="viscosity.η", eta_v="viscosity.ηv",
               eta_vep="viscosity.η_vep", EII_pl="EII_pl", evol_pl="ε_vol_pl", EVol_pl="EVol_pl", RP="R.RP", Rx="R.Rx", Ry="R.Ry", omega_xy="ω.xy")
SENTINEL = -77.25


def _get(o, path):
    for p in path.split("."):
        o = getattr(o, p)
    return o


def _upload(jr, s):
    import torch
    from justrelax_jl_amd.arrays import from_numpy
    dev = torch.device("cuda", torch.cuda.current_device())
    st = jr.StokesArrays(jr.AMDGPUBackend, s.ni)
    for k, path in VEP_MAP.items():
        _get(st, path).copy_(from_numpy(s.arrays[k], dev))
    nph = s.arrays["phase_c"].shape[0]
    pr = jr.PhaseRatios(jr.AMDGPUBackend, nph, s.ni)
    for k, name in (("center", "phase_c"), ("vertex", "phase_v"), ("Vx", "phase_vx"), ("Vy", "phase_vy")):
        getattr(pr, k).copy_(from_numpy(s.arrays[name], dev))
    ρg = (from_numpy(s.arrays["fx"], dev), from_numpy(s.arrays["fy"], dev))
    return st, pr, ρg


def _upload_phi(jr, phi):
    from justrelax_jl_amd.arrays import from_numpy
    ϕ = jr.RockRatio(jr.AMDGPUBackend, phi["center"].shape)
    for k in ("center", "vertex", "Vx", "Vy"):
        getattr(ϕ, k).copy_(from_numpy(phi[k], ϕ.center.device))
    return ϕ


def _download(jr, st):
    return {k: jr.to_numpy(_get(st, path)) for k, path in VEP_MAP.items()}


def _state(jr, ni, seed):
    """the randomised shear-band state on an nx x ny grid, with a random rock ratio whose predicates are true and false on 20-80 % of the nodes"""
    s = jr.miniapps.shearband2d_variational(max(ni))
    if ni[0] != ni[1]:
        import justrelax_jl_amd.grid as g
        nx, ny = ni
        full = jr.miniapps.stokes2d._vep_shapes2d(nx, ny, 2)
        s.ni = ni
        s.arrays = {k: np.zeros(shp, order="F") for k, shp in full.items()}
        s.arrays.update(phase_vx=np.zeros((2, nx + 1, ny), order="F"), phase_vy=np.zeros((2, nx, ny + 1), order="F"))
        g.finalize_global_grid()
        g.init_global_grid(nx, ny, 1)
        s.grid = jr.Geometry(ni, (1.0, 1.0), origin=(0.0, 0.0))
        s.pt = jr.PTStokesCoeffs((1.0, 1.0), (1.0 / nx, 1.0 / ny), ϵ_rel=1.0e-6, CFL=0.75 / np.sqrt(2.1))
    vs.randomize(s, seed)
    rng = np.random.default_rng(seed + 100)
    for k in ("Vx", "Vy", "fx", "fy"):
        s.arrays[k][...] = rng.uniform(-1.0, 1.0, size=s.arrays[k].shape)
    phi = vs.random_phi(s.ni, seed + 1)
    m = vs.valid_masks(phi)
    for k in ("c", "v", "vx", "vy"):
        assert 0.2 <= m[k].mean() <= 0.8, (k, m[k].mean())
    return s, phi, m


@pytest.mark.parametrize("air_phase", [2, 0, 99])
def test_update_rock_ratio_matches_restatement_2d_and_3d(jr, air_phase):
    """update_rock_ratio! on random ratios, bit for bit (one subtraction): ratios within 1e-5 of 1, air_phase out of range, the 3D members"""
    from justrelax_jl_amd.arrays import from_numpy
    rng = np.random.default_rng(3)
    for ni in ((13, 9), (7, 6, 5)):
        pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
        ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
        names = ("center", "vertex", "Vx", "Vy") + (("Vz", "xy", "yz", "xz") if len(ni) == 3 else ())
        host = {}
        for k in names:
            shp = tuple(getattr(pr, k).shape)
            a = rng.uniform(0.0, 1.0, size=shp[1:])
            u = rng.uniform(size=a.shape)
            a[u < 0.2] = 1.0 - rng.uniform(0.0, 2.0e-5, size=a.shape)[u < 0.2]          # around the 1e-5 threshold
            a[u > 0.9] = -1.0e-3                                                      # 1 - ratio above one: clamped for the velocity members only
            r = np.zeros(shp, order="F")
            r[1], r[0] = a, 1.0 - a
            host[k] = r
            getattr(pr, k).copy_(from_numpy(r, ϕ.center.device))
        jr.update_rock_ratio_(ϕ, pr, air_phase)
        want = vs.rock_ratio(*ni)
        vs.update_rock_ratio(want, host, air_phase)
        for k in names:
            assert np.array_equal(jr.to_numpy(getattr(ϕ, k)), want[k]), (ni, k)
        if air_phase == 2:
            assert (want["center"] == 0).any() and want["center"].max() > 1.0 and want["vertex"].max() > 1.0 and want["Vx"].max() == 1.0 and want["Vy"].max() == 1.0


@pytest.mark.parametrize("ni", [(24, 24), (17, 19), (257, 33)])
def test_masked_kernels_match_restatement(jr, ni):
    """jrx_vs2d_strain_rates, jrx_vs2d_update_stresses, jrx_vs2d_compute_V on the randomised state with a random ϕ (zeros, ones, fractions); tolerance 1e-12 as
    the unmasked kernel test of test_gpu_vep2d.py.  What the reference leaves unwritten at invalid nodes keeps its sentinel: τII at invalid centres, ε_pl.xy at
    invalid vertices (unless the invalid centre of the same index zeroes it)."""
    from justrelax_jl_amd import _lib, stokes as st_mod, variational as var
    from justrelax_jl_amd.arrays import from_numpy
    from justrelax_jl_amd.checks import max_rel_diff
    s, phi, m = _state(jr, ni, seed=11)
    a = s.arrays
    rng = np.random.default_rng(9)
    theta = np.asfortranarray(rng.uniform(-1, 1, size=s.ni))
    lam = np.asfortranarray(rng.uniform(0, 0.1, size=s.ni))
    lamv = np.asfortranarray(rng.uniform(0, 0.1, size=(ni[0] + 1, ni[1] + 1)))
    etatau = np.asfortranarray(10.0 ** rng.uniform(-1, 0.5, size=s.ni))
    a["tII"][...] = SENTINEL
    a["eplxy"][...] = SENTINEL
    stokes, pr, ρg = _upload(jr, s)
    ϕ = _upload_phi(jr, phi)
    dev = stokes.P.device
    h = _lib.default_handle()
    s.kwargs.update(free_surface=True)
    kw = {k: v for k, v in s.kwargs.items() if k != "air_phase"}
    fd = st_mod.vep_fields2d(stokes, ρg, pr)
    pd = st_mod.vep_params2d(stokes, s.pt, s.grid, s.flow_bcs, s.dt, **kw)
    rd = var.rock_ratio2d(ϕ)
    rh = st_mod.rheology_table(s.extra["phases"])
    # ---- ∇V and strain rates
    h.call("jrx_vs2d_strain_rates", C.byref(fd), C.byref(rd), C.byref(pd))
    vs.compute_divV_strain(a, phi, s.grid._di["center"])
    out = _download(jr, stokes)
    for k in ("divV", "exx", "eyy", "exy"):
        assert max_rel_diff(out[k], a[k]) <= 1e-12, k
        assert np.array_equal(out[k] == 0, a[k] == 0), k
    assert (a["exx"][~m["c"]] == 0).all() and (a["exy"][~m["v"]] == 0).all()
    # ---- stress update
    th_d, lam_d, lamv_d = from_numpy(theta, dev), from_numpy(lam, dev), from_numpy(lamv, dev)
    h.call("jrx_vs2d_update_stresses", C.byref(fd), C.byref(rd), C.c_void_p(th_d.data_ptr()), C.c_void_p(lam_d.data_ptr()), C.c_void_p(lamv_d.data_ptr()),
           C.byref(rh), C.byref(pd))
    lam0, lamv0 = lam.copy(), lamv.copy()
    vs.update_stresses(a, phi, theta, lam, lamv, s.extra["phases"], s.dt, s.pt.θ_dτ, 0.2)
    out = _download(jr, stokes)
    assert (lam != lam0)[m["c"]].any() and (lam == lam0)[m["c"]].any() and (lamv != lamv0)[m["v"]].any() and (lamv == lamv0)[m["v"]].any()      # yielding and not
    for k in ("txx", "tyy", "txy", "txy_c", "tII", "eta_vep", "P", "eplxx", "eplyy", "eplxy", "evol_pl"):
        assert max_rel_diff(out[k], a[k]) <= 1e-12, k
    assert max_rel_diff(jr.to_numpy(lam_d), lam) <= 1e-12 and max_rel_diff(jr.to_numpy(lamv_d), lamv) <= 1e-12
    assert (out["tII"][~m["c"]] == SENTINEL).all() and (out["tII"][m["c"]] != SENTINEL).all()
    keep = ~m["v"]
    keep[:-1, :-1] &= m["c"]                                  # an invalid centre zeroes ε_pl.xy at its own index
    assert keep.any() and (out["eplxy"][keep] == SENTINEL).all()
    assert (out["txy"][~m["v"]] == 0).all() and (out["eplxy"][:-1, :-1][~m["c"]] == 0).all()
    # ---- velocity update (dt * free_surface = dt)
    et_d = from_numpy(etatau, dev)
    h.call("jrx_vs2d_compute_V", C.byref(fd), C.byref(rd), C.c_void_p(et_d.data_ptr()), C.byref(pd))
    vs.compute_V(a, phi, etatau, s.pt.ηdτ, s.grid._di["center"], s.dt)
    out = _download(jr, stokes)
    for k in ("Vx", "Vy", "Rx", "Ry"):
        assert max_rel_diff(out[k], a[k]) <= 1e-12, k
    assert (out["Vx"][1:-1, 1:-1][~m["vx"][1:-1, :]] == 0).all() and (out["Ry"][~m["vy"][:, 1:-1]] == 0).all()


def _solve_both(jr, s, phi_host=None):
    from justrelax_jl_amd.checks import max_rel_diff
    stokes, pr, ρg = _upload(jr, s)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    air = s.kwargs["air_phase"]
    jr.update_rock_ratio_(ϕ, pr, air)
    phi = vs.rock_ratio(*s.ni)
    vs.update_rock_ratio(phi, dict(center=s.arrays["phase_c"], vertex=s.arrays["phase_v"], Vx=s.arrays["phase_vx"], Vy=s.arrays["phase_vy"]), air)
    r = jr.solve_VariationalStokes_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
    kw = {k: v for k, v in s.kwargs.items() if k != "verbose"}
    r_ref = vs.solve_VS(s.arrays, phi, s.extra["phases"], vs.pt_tuple(s.pt), s.grid._di["center"], s.dt, **kw)
    return r, r_ref, _download(jr, stokes), phi


@pytest.mark.parametrize("n", [32, 48])
def test_full_solve_with_air_matches_restatement(jr, n):
    """solve_VariationalStokes! with an air layer (three rows, one more partially filled; air_phase = 3, finite viscosity cutoff): every field of VEP_MAP, the
    norm history and the iteration count against the restatement; tolerance 1e-9 as the full-solve parity test of the unmasked driver"""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband2d_variational(n, air_rows=3, iterMax=59, nout=20)
    s.kwargs.update(iterMin=10)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    r, r_ref, out, phi = _solve_both(jr, s)
    m = vs.valid_masks(phi)
    assert 0 < m["c"].mean() < 1 and ((phi["center"] > 0) & (phi["center"] < 1)).any() and ((phi["Vy"] > 0) & (phi["Vy"] < 1)).any()
    assert r.iter == r_ref["iter"] == 60
    assert np.allclose(r.err_evo1, r_ref["err_evo1"], rtol=1e-9) and np.allclose(r.norm_Rx, r_ref["norm_Rx"], rtol=1e-9)
    assert np.allclose(r.norm_Ry, r_ref["norm_Ry"], rtol=1e-9) and np.allclose(r.norm_divV, r_ref["norm_divV"], rtol=1e-9)
    assert list(r.err_evo2) == r_ref["err_evo2"] == [20, 40, 60]
    for k in out:
        assert max_rel_diff(out[k], s.arrays[k]) <= 1e-9, k
    assert (out["Vy"][1:-1, 1:-1][~m["vy"][:, 1:-1]] == 0).all() and (out["P"][~m["c"]] == 0).all()


@pytest.mark.parametrize("density", ["caller", "T_Density"])
def test_full_solve_phi_one_equals_the_unmasked_driver(jr, density):
    """(density = "T_Density": temperature-dependent densities, so that update_ρg! runs inside the loop of both drivers, args.T cell-centred.)
    ϕ ≡ 1, air_phase = 0 against solve_ (the unmasked HIP driver) on the same inputs.  The two are not bit-identical: compute_strain_rate! divides ∇V by 3
    where the unmasked kernel multiplies by inv(3) (tests/test_variational_stokes_restatement.py); the bound is the one found there, 10 x 3.3e-15.  R.Rx, R.Ry
    and the norms are produced at different points of the iteration by the two drivers and are not compared."""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband2d_variational(32, iterMax=39, nout=10)
    s.kwargs.update(iterMin=10)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    vs.randomize(s)
    args = None
    if density == "T_Density":
        from justrelax_jl_amd.arrays import from_numpy
        import torch
        for ph in s.extra["phases"]:
            ph["density"] = dict(kind="T", rho0=1.0, alpha=1.0e-2, T0=0.0)
        s.extra["phases"][0]["g"] = 1.0
        T = np.asfortranarray(np.random.default_rng(3).uniform(0.0, 10.0, size=s.ni))
        args = dict(T=from_numpy(T, torch.device("cuda", torch.cuda.current_device())))
    stokes, pr, ρg = _upload(jr, s)
    kw = {k: v for k, v in s.kwargs.items() if k != "air_phase"}
    jr.compute_viscosity_(stokes, pr, None, s.extra["phases"], s.kwargs["viscosity_cutoff"])          # what _solve_VS! does on entry
    r0 = jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], args, s.dt, None, kwargs=kw)
    ref = _download(jr, stokes)
    stokes, pr, ρg = _upload(jr, s)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    jr.update_rock_ratio_(ϕ, pr, 0)
    assert float(ϕ.center.min()) == float(ϕ.Vx.min()) == 1.0
    r = jr.solve_VariationalStokes_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, s.extra["phases"], args, s.dt, None, kwargs=s.kwargs)
    out = _download(jr, stokes)
    assert r.iter == r0.iter == 40
    if density == "T_Density":
        assert np.ptp(jr.to_numpy(ρg[1])) > 0 and not np.array_equal(jr.to_numpy(ρg[1]), s.arrays["fy"])
    for k in out:
        if k not in ("Rx", "Ry"):
            assert max_rel_diff(out[k], ref[k]) <= 3.3e-14, k


def test_all_air_solve_is_exactly_zero(jr):
    s = jr.miniapps.shearband2d_variational(16, iterMax=50, nout=10)
    s.kwargs.update(iterMin=5)
    stokes, pr, ρg = _upload(jr, s)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    r = jr.solve_VariationalStokes_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
    assert r.iter == 10 and list(r.err_evo1) == [0.0]
    out = _download(jr, stokes)
    assert not out["Vx"][1:-1, 1:-1].any() and not out["Vy"][1:-1, 1:-1].any() and not out["Rx"].any() and not out["Ry"].any() and not out["RP"].any()


def test_out_of_scope_inputs_are_refused_with_status_4(jr):
    from justrelax_jl_amd import _lib
    s = jr.miniapps.shearband2d_variational(16, iterMax=10, nout=5)
    stokes, pr, ρg = _upload(jr, s)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    jr.update_rock_ratio_(ϕ, pr, 0)
    run = lambda grid=s.grid, phases=s.extra["phases"], handle=None, **kw: jr.solve_VariationalStokes_(
        stokes, s.pt, grid, s.flow_bcs, ρg, pr, ϕ, phases, None, s.dt, None, kwargs=dict(s.kwargs, **kw), handle=handle)
    xv = np.linspace(0.0, 1.0, 17) ** 1.2
    cases = [("inv_spacing", dict(grid=jr.Geometry.from_vertices((xv, xv)))), ("strain_increment", dict(strain_increment=True)),
             ("DruckerPragerCap", dict(phases=[dict(s.extra["phases"][0], cap=dict(P_T=1.0)), s.extra["phases"][1]])), ("air_phase", dict(air_phase=5))]
    for word, kw in cases:
        with pytest.raises(_lib.JrxError) as e:
            run(**kw)
        assert e.value.status == 4 and word in str(e.value), (word, str(e.value))
    # a handle with a communicator of more than one rank (two ranks of this process; refused before anything is exchanged)
    from justrelax_jl_amd import halo
    hs = [_lib.Handle(stokes.P.device.index) for _ in range(2)]
    try:
        halo.init_comm_local(hs, halo.make_carts((16, 16, 1), (2, 1, 1)))
        with pytest.raises(_lib.JrxError) as e:
            run(handle=hs[0])
        assert e.value.status == 4 and "communicator" in str(e.value)
    finally:
        for hh in hs:
            hh.close()


def test_viscosity_air_phase_zero_is_the_existing_entry_point(jr):
    """air_phase = 0 through jrx_vep2d_compute_viscosity_air is bit-identical to jrx_vep2d_compute_viscosity / _tauII; air_phase = 3 matches the restatement"""
    from justrelax_jl_amd import _lib, stokes as st_mod
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband2d_variational(24, air_rows=2)
    rng = np.random.default_rng(5)
    s.arrays["eta"][...] = 10.0 ** rng.uniform(-1, 0.5, size=s.ni)
    s.arrays["eta_v"][...] = 10.0 ** rng.uniform(-1, 0.5, size=s.arrays["eta_v"].shape)
    h = _lib.default_handle()
    for tau in (0, 1):
        stokes, pr, ρg = _upload(jr, s)
        (jr.compute_viscosity_τII_ if tau else jr.compute_viscosity_)(stokes, pr, None, s.extra["phases"], (1e-2, 1e2), relaxation=0.3)
        want = _download(jr, stokes)
        stokes, pr, ρg = _upload(jr, s)
        fd = st_mod.vep_fields2d(stokes, ρg, pr)
        pd = st_mod.vep_params2d(stokes, s.pt, s.grid, None, 1.0, viscosity_cutoff=(1e-2, 1e2))
        h.call("jrx_vep2d_compute_viscosity_air", C.byref(fd), C.byref(st_mod.rheology_table(s.extra["phases"])), C.byref(pd), C.c_double(0.3), C.c_int32(0), C.c_int32(tau))
        got = _download(jr, stokes)
        assert np.array_equal(got["eta"], want["eta"]) and np.array_equal(got["eta_v"], want["eta_v"])
    stokes, pr, ρg = _upload(jr, s)
    jr.compute_viscosity_(stokes, pr, None, s.extra["phases"], (1e-2, 1e2), relaxation=0.3, air_phase=3)
    a = {k: v.copy() for k, v in s.arrays.items()}
    vs.compute_viscosity(a, s.extra["phases"], 0.3, (1e-2, 1e2), 3)
    got = _download(jr, stokes)
    assert max_rel_diff(got["eta"], a["eta"]) <= 1e-12 and max_rel_diff(got["eta_v"], a["eta_v"]) <= 1e-12
    assert (a["eta"] == 1e2).any() and (a["eta"] != s.arrays["eta"]).all()


@pytest.mark.parametrize("tau", [False, True])
def test_viscosity_air_phase_with_power_law_creep_matches_restatement(jr, tau):
    """the field-reading branch of compute_viscosity! / update_viscosity_τII! with air_phase = 3: two dislocation-creep rock phases (the invariant of the stress or
    of the strain rate, T and P at the cell, averaged at the vertices) under an air layer.  Bound 1e-12: the laws are pow and exp of the inputs, a few ulp each on
    either side, and the exponent (E + P V)/(R T) <= 60 carries one rounding of its argument (1.1e-16) to 7e-15 of the viscosity."""
    import torch
    from justrelax_jl_amd.arrays import from_numpy
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband2d_variational(24, air_rows=2)
    rng = np.random.default_rng(17)
    a = s.arrays
    for k in ("txx", "tyy", "txy", "txy_c"):
        a[k][...] = rng.uniform(-5.0e6, 5.0e6, size=a[k].shape)
    for k in ("exx", "eyy", "exy", "exy_c"):
        a[k][...] = rng.uniform(-1.0e-14, 1.0e-14, size=a[k].shape)
    a["P"][...] = rng.uniform(1.0e8, 1.0e9, size=s.ni)
    a["eta"][...] = 10.0 ** rng.uniform(19, 23, size=s.ni)
    a["eta_v"][...] = 10.0 ** rng.uniform(19, 23, size=a["eta_v"].shape)
    T = np.asfortranarray(rng.uniform(600.0, 900.0, size=s.ni))
    inf = float("inf")
    phases = [dict(G=inf, Kb=inf, creep=dict(kind="dislocation", A=3.2e-20, n=3.0, E=276.0e3, V=1.0e-6, R=8.3145)),
              dict(G=inf, Kb=inf, creep=dict(kind="dislocation", A=3.16e-26, n=3.3, E=186.0e3, V=0.0, R=8.3145)),
              dict(eta=1.0e19, G=inf, Kb=inf)]
    cutoff = (1.0e18, 1.0e25)
    stokes, pr, ρg = _upload(jr, s)
    Td = from_numpy(T, stokes.P.device)
    (jr.compute_viscosity_τII_ if tau else jr.compute_viscosity_)(stokes, pr, dict(T=Td), phases, cutoff, relaxation=0.3, air_phase=3)
    eta0 = a["eta"].copy()
    vs.compute_viscosity_fields(a, phases, 0.3, cutoff, 3, tau, T)
    got = _download(jr, stokes)
    assert max_rel_diff(got["eta"], a["eta"]) <= 1e-12 and max_rel_diff(got["eta_v"], a["eta_v"]) <= 1e-12
    inside = (a["eta"] > cutoff[0]) & (a["eta"] < cutoff[1])
    assert inside.mean() > 0.3 and (a["eta"] != eta0).all() and (a["eta"] == cutoff[1]).any()


def test_nan_exit_leaves_the_current_stresses_in_the_callers_arrays(jr):
    """error("NaN(s)") at the first check, iteration 3: after an odd number of pointer swaps the current τxx, τyy and η live in the library's second set and the NaN
    exit has to copy them back.  One phase, linear viscosity, 8 x 8 cells, one NaN in an interior Vx entry; the caller's arrays after the failed call equal those of
    a call that runs the same three iterations unchecked (nout > iterMax, iterMax = 2: the loop runs while iter <= iterMax) and returns normally."""
    from justrelax_jl_amd._lib import JrxError
    outs = []
    for iterMax, nout in ((20, 3), (2, 100)):
        s = jr.miniapps.shearband2d_variational(8, iterMax=iterMax, nout=nout)
        phases = [s.extra["phases"][0]]
        for k in ("phase_c", "phase_v", "phase_vx", "phase_vy"):
            s.arrays[k] = np.ones((1,) + s.arrays[k].shape[1:], order="F")
        s.arrays["Vx"][1, 1] = np.nan
        stokes, pr, ρg = _upload(jr, s)
        ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
        jr.update_rock_ratio_(ϕ, pr, 0)
        solve = lambda: jr.solve_VariationalStokes_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, phases, None, s.dt, None, kwargs=s.kwargs)
        if nout == 3:
            with pytest.raises(JrxError) as e:
                solve()
            assert e.value.status == 1 and "JRX_ERR_NAN" in str(e.value)
        else:
            r = solve()
            assert r.iter == 3 and len(r.err_evo1) == 0
        outs.append(_download(jr, stokes))
    assert np.isnan(outs[0]["txx"]).any()
    for k in ("txx", "tyy", "txy", "txy_c", "eta"):
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
        assert np.isfinite(outs[0][k]).any(), k


def test_full_solve_that_stores_every_iteration_keeps_the_bits(jr):
    """tuning switch "vep_store_all" = 1: every iteration of solve_VariationalStokes! stores its output-only arrays (default: only the iterations after which the loop can stop).
    The solve of test_full_solve_with_air_matches_restatement (n = 32) with the switch off and on: every field of VEP_MAP is the same in every bit at the end, both runs match
    the restatement at that test's 1e-9, and stat_vep_store_all counts the iterations that stored because of the switch."""
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.checks import max_rel_diff
    h = _lib.default_handle()
    runs = []
    try:
        for store in (0, 1):
            h.set_option("vep_store_all", store)
            s = jr.miniapps.shearband2d_variational(32, air_rows=3, iterMax=59, nout=20)
            s.kwargs.update(iterMin=10)
            s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
            c0 = h.get_option("stat_vep_store_all")
            r, r_ref, out, phi = _solve_both(jr, s)
            runs.append((r, out, h.get_option("stat_vep_store_all") - c0))
            assert r.iter == r_ref["iter"] == 60
            assert np.allclose(r.err_evo1, r_ref["err_evo1"], rtol=1e-9) and np.allclose(r.norm_Rx, r_ref["norm_Rx"], rtol=1e-9)
            for k in out:
                assert max_rel_diff(out[k], s.arrays[k]) <= 1e-9, k
    finally:
        h.set_option("vep_store_all", 0)
    assert runs[0][2] == 0 and runs[1][2] > 0
    assert list(runs[0][0].err_evo1) == list(runs[1][0].err_evo1)
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
