"""GPU parity tests of the 3D variational Stokes solver (csrc/stokes3d_vs.hip) against its NumPy restatement (tests/_variational_stokes3d.py), which
tests/test_variational_stokes3d_restatement.py pins to the C oracle (ϕ ≡ 1) and to the 2D masked restatement (states uniform along one axis)."""
import ctypes as C

import numpy as np
import pytest

import _variational_stokes3d as vs

pytestmark = pytest.mark.gpu

_T = {"e": "ε", "epl": "ε_pl", "de": "Δε", "t": "τ", "to": "τ_o"}
VEP3_MAP = dict(P="P", P0="P0", divV="divV", Q="Q", Vx="V.Vx", Vy="V.Vy", Vz="V.Vz", Ux="U.Ux", Uy="U.Uy", Uz="U.Uz", tII="τ.II",
                eta="viscosity.η", eta_vep="viscosity.η_vep", EII_pl="EII_pl", evol_pl="ε_vol_pl", EVol_pl="EVol_pl",
                RP="R.RP", Rx="R.Rx", Ry="R.Ry", Rz="R.Rz", omega_yz="ω.yz", omega_xz="ω.xz", omega_xy="ω.xy")
for _pre, _t in _T.items():
    for _c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        if _pre == "de" and _c in ("xx", "yy", "zz"):
            continue
        VEP3_MAP[_pre + _c] = f"{_t}.{_c}"
PHASE_MEMBERS = dict(center="phase_c", vertex="phase_v", Vx="phase_vx", Vy="phase_vy", Vz="phase_vz", yz="phase_yz", xz="phase_xz", xy="phase_xy")
MEMBERS = tuple(PHASE_MEMBERS)
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
    for k, path in VEP3_MAP.items():
        _get(st, path).copy_(from_numpy(s.arrays[k], dev))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, s.arrays["phase_c"].shape[0], s.ni)
    for member, k in PHASE_MEMBERS.items():
        if k in s.arrays:
            getattr(pr, member).copy_(from_numpy(s.arrays[k], dev))
    ρg = tuple(from_numpy(s.arrays[k], dev) for k in ("fx", "fy", "fz"))
    return st, pr, ρg


def _upload_phi(jr, phi):
    from justrelax_jl_amd.arrays import from_numpy
    ϕ = jr.RockRatio(jr.AMDGPUBackend, phi["center"].shape)
    for k in MEMBERS:
        getattr(ϕ, k).copy_(from_numpy(phi[k], ϕ.center.device))
    return ϕ


def _download(jr, st):
    return {k: jr.to_numpy(_get(st, path)) for k, path in VEP3_MAP.items()}


def _host_phi(s, air):
    phi = vs.rock_ratio(*s.ni)
    vs.update_rock_ratio(phi, {m: s.arrays[k] for m, k in PHASE_MEMBERS.items()}, air)
    return phi


@pytest.mark.parametrize("ni", [(7, 6, 5), (17, 19, 23), (65, 9, 5)])
def test_masked_kernels_match_restatement(jr, ni):
    """jrx_vs3d_strain_rates, jrx_vs3d_update_stresses, jrx_vs3d_compute_V on the randomised shearband3d state with random_phi3 (zeros, ones, fractions; (65, 9, 5) is
    more than one 64-wide block in x with odd extents); tolerance 1e-12 as the unmasked kernel test of test_gpu_vep3d.py, taken over the nodes the kernel writes.
    What the reference leaves unwritten keeps its sentinel: ε at invalid nodes after the strain-rate call (the stress update then averages it in, on both sides), τII
    at invalid centres, ε_pl on invalid edges -- unless the invalid centre of the same index zeroes it."""
    from justrelax_jl_amd import _lib, stokes as st_mod, variational as var
    from justrelax_jl_amd.arrays import from_numpy
    from justrelax_jl_amd.checks import max_rel_diff
    nx, ny, nz = ni
    s = jr.miniapps.shearband3d(ni)
    phases = vs.randomize(s, 11)
    a = s.arrays
    rng = np.random.default_rng(111)
    for k in ("Vx", "Vy", "Vz", "fx", "fy", "fz"):
        a[k][...] = rng.uniform(-1.0, 1.0, size=a[k].shape)
    phi = vs.random_phi3(ni, 12)
    m = vs.valid_masks(phi)
    for k in m:
        assert 0.2 <= m[k].mean() <= 0.8, (k, m[k].mean())
    theta = np.asfortranarray(rng.uniform(-1, 1, size=ni))
    lam = np.asfortranarray(rng.uniform(0, 0.1, size=ni))
    lamv = [np.asfortranarray(rng.uniform(0, 0.1, size=a[k].shape)) for k in ("tyz", "txz", "txy")]
    etatau = np.asfortranarray(10.0 ** rng.uniform(-1, 0.5, size=ni))
    for k in ("exx", "eyy", "ezz", "eyz", "exz", "exy", "tII", "eplyz", "eplxz", "eplxy"):
        a[k][...] = SENTINEL
    stokes, pr, ρg = _upload(jr, s)
    ϕ = _upload_phi(jr, phi)
    dev = stokes.P.device
    h = _lib.default_handle()
    fd = st_mod.vep_fields3d(stokes, ρg, pr)
    pd = st_mod.vep_params3d(stokes, s.pt, s.grid, s.flow_bcs, s.dt)
    rd = var.rock_ratio3d(ϕ)
    _di = s.grid._di["center"]
    emask = dict(exx="c", eyy="c", ezz="c", eyz="yz", exz="xz", exy="xy")

    def close(out, k, mask=None):
        x, y = (out[k], a[k]) if mask is None else (out[k][mask], a[k][mask])
        assert max_rel_diff(x, y) <= 1e-12, (k, max_rel_diff(x, y))
        assert np.array_equal(x == 0, y == 0), k
    # ---- ∇V and strain rates
    h.call("jrx_vs3d_strain_rates", C.byref(fd), C.byref(rd), C.byref(pd))
    vs.compute_divV_strain(a, phi, _di)
    out = _download(jr, stokes)
    close(out, "divV")
    assert (out["divV"][~m["c"]] == 0).all()
    for k, mk in emask.items():
        close(out, k, m[mk])
        assert (out[k][~m[mk]] == SENTINEL).all() and (out[k][m[mk]] != SENTINEL).all(), k
    # ---- stress update
    th_d, lam_d = from_numpy(theta, dev), from_numpy(lam, dev)
    lamv_d = [from_numpy(x, dev) for x in lamv]
    lv = (C.c_void_p * 3)(*[x.data_ptr() for x in lamv_d])
    h.call("jrx_vs3d_update_stresses", C.byref(fd), C.byref(rd), C.c_void_p(th_d.data_ptr()), C.c_void_p(lam_d.data_ptr()), lv,
           C.byref(st_mod.rheology_table(phases)), C.byref(pd))
    lam0, lamv0 = lam.copy(), [x.copy() for x in lamv]
    vs.update_stresses(a, phi, theta, lam, lamv, phases, s.dt, s.pt.θ_dτ, 0.2)
    out = _download(jr, stokes)
    assert (lam != lam0)[m["c"]].any() and (lam == lam0)[m["c"]].any() and (lam == lam0)[~m["c"]].all()                    # yielding and not, among the valid nodes
    for T, name in enumerate(vs.EDGES):
        assert (lamv[T] != lamv0[T])[m[name]].any() and (lamv[T] == lamv0[T])[m[name]].any() and (lamv[T] == lamv0[T])[~m[name]].all(), name
    for k in ("txx", "tyy", "tzz", "tyz", "txz", "txy", "tyz_c", "txz_c", "txy_c", "eta_vep", "P", "eplxx", "eplyy", "eplzz", "evol_pl"):
        close(out, k)
    close(out, "tII", m["c"])
    assert (out["tII"][~m["c"]] == SENTINEL).all() and (out["tII"][m["c"]] != SENTINEL).all()
    assert max_rel_diff(jr.to_numpy(lam_d), lam) <= 1e-12
    for x, y in zip(lamv_d, lamv):
        assert max_rel_diff(jr.to_numpy(x), y) <= 1e-12
    for name in vs.EDGES:
        k = "epl" + name
        keep = ~m[name]
        keep[:nx, :ny, :nz] &= m["c"]                             # an invalid centre zeroes ε_pl on the edge of its own index
        assert keep.any() and (out[k][keep] == SENTINEL).all() and np.array_equal(a[k] == SENTINEL, keep), name
        close(out, k, ~keep)
        assert (~m["c"] & m[name][:nx, :ny, :nz]).any() and (out[k][:nx, :ny, :nz][~m["c"]] == 0).all() and (out["t" + name][~m[name]] == 0).all(), name
    for k in ("P", "txx", "tyz_c", "eta_vep", "eplzz", "evol_pl"):
        assert (out[k][~m["c"]] == 0).all(), k
    # ---- velocity update
    et_d = from_numpy(etatau, dev)
    h.call("jrx_vs3d_compute_V", C.byref(fd), C.byref(rd), C.c_void_p(et_d.data_ptr()), C.byref(pd))
    vs.compute_V(a, phi, etatau, s.pt.ηdτ, _di)
    out = _download(jr, stokes)
    for k in ("Vx", "Vy", "Vz", "Rx", "Ry", "Rz"):
        close(out, k)
    assert (out["Vx"][1:-1, 1:-1, 1:-1][~m["vx"][1:-1]] == 0).all() and (out["Ry"][~m["vy"][:, 1:-1]] == 0).all() and (out["Vz"][1:-1, 1:-1, 1:-1][~m["vz"][:, :, 1:-1]] == 0).all()


@pytest.mark.parametrize("n", [12, 20])
def test_full_solve_with_air_matches_restatement(jr, n):
    """solve_VariationalStokes! 3D with an air layer (two layers of cells, half of the next; air_phase = 3, finite viscosity cutoff, gravity): every field of
    VEP3_MAP, the four norm histories and the iteration count against the restated driver; tolerance 1e-9 as the 2D full-solve test"""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband3d_variational(n, air_layers=2, iterMax=59, nout=20)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    air = s.kwargs["air_phase"]
    stokes, pr, ρg = _upload(jr, s)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    jr.update_rock_ratio_(ϕ, pr, air)
    phi = _host_phi(s, air)
    for k in MEMBERS:
        assert np.array_equal(jr.to_numpy(getattr(ϕ, k)), phi[k]), k
        assert ((phi[k] > 0) & (phi[k] < 1)).any() and (phi[k] == 0).any(), k
    m = vs.valid_masks(phi)
    assert all(0 < m[k].mean() < 1 for k in m)
    r = jr.solve_VariationalStokes_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
    kw = {k: v for k, v in s.kwargs.items() if k != "verbose"}
    r_ref = vs.solve_VS(s.arrays, phi, s.extra["phases"], vs.pt_tuple(s.pt), s.grid._di["center"], s.dt, **kw)
    out = _download(jr, stokes)
    out["fz"] = jr.to_numpy(ρg[2])
    assert r.iter == r_ref["iter"] == 60
    assert list(r.err_evo2) == r_ref["err_evo2"] == [20, 40, 60]
    for k, got in (("err_evo1", r.err_evo1), ("norm_Rx", r.norm_Rx), ("norm_Ry", r.norm_Ry), ("norm_Rz", r.norm_Rz), ("norm_divV", r.norm_divV)):
        assert np.allclose(got, r_ref[k], rtol=1e-9, atol=0), k
    assert np.ptp(s.arrays["fz"]) > 0
    for k in out:
        assert max_rel_diff(out[k], s.arrays[k]) <= 1e-9, (k, max_rel_diff(out[k], s.arrays[k]))
    assert (out["Vx"][1:-1, 1:-1, 1:-1][~m["vx"][1:-1]] == 0).all() and (out["Vy"][1:-1, 1:-1, 1:-1][~m["vy"][:, 1:-1]] == 0).all()
    assert (out["Vz"][1:-1, 1:-1, 1:-1][~m["vz"][:, :, 1:-1]] == 0).all() and (out["P"][~m["c"]] == 0).all()


def test_full_solve_phi_one_equals_the_unmasked_driver(jr):
    """ϕ ≡ 1, air_phase = 0 against solve_ (the unmasked 3D HIP driver) on the inputs of the CPU test of the same name, at the bound found there (10 x 4.2e-15).  Both
    drivers take R from compute_V!, so R is compared; the norms of R after the unmasked driver's are multiplied by sqrt((nx-1)(ny-1)(nz-1)) (it divides by the
    product, this one by its root); err, the maximum over differently scaled norms, is not."""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband3d_variational((10, 8, 7), iterMax=19, nout=5)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    rng = np.random.default_rng(3)
    a = s.arrays
    for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        a["to" + c][...] = rng.uniform(-1.5, 1.5, size=a["to" + c].shape)
        a["t" + c][...] = a["to" + c]
    stokes, pr, ρg = _upload(jr, s)
    kw = {k: v for k, v in s.kwargs.items() if k != "air_phase"}
    r0 = jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], None, s.dt, None, kwargs=kw)
    ref = _download(jr, stokes)
    stokes, pr, ρg = _upload(jr, s)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    jr.update_rock_ratio_(ϕ, pr, 0)
    assert all(float(getattr(ϕ, k).min()) == 1.0 for k in MEMBERS)
    r = jr.solve_VariationalStokes_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
    out = _download(jr, stokes)
    assert r.iter == r0.iter == 20 and list(r.err_evo2) == list(r0.err_evo2) == [5, 10, 15, 20]
    assert (ref["eplxx"] != 0).any() and (ref["eplxz"] != 0).any()
    for k in out:
        assert max_rel_diff(out[k], ref[k]) <= 4.2e-14, (k, max_rel_diff(out[k], ref[k]))
    nx, ny, nz = s.ni
    scale = np.sqrt((nx - 1) * (ny - 1) * (nz - 1))
    for got, want in ((r.norm_Rx, r0.norm_Rx * scale), (r.norm_Ry, r0.norm_Ry * scale), (r.norm_Rz, r0.norm_Rz * scale), (r.norm_divV, r0.norm_divV)):
        assert max_rel_diff(got, want) <= 4.2e-14


def test_all_air_solve_is_exactly_zero(jr):
    s = jr.miniapps.shearband3d_variational((8, 7, 6), iterMax=50, nout=10)
    stokes, pr, ρg = _upload(jr, s)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    r = jr.solve_VariationalStokes_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
    assert r.iter == 10 and list(r.err_evo1) == [0.0]
    out = _download(jr, stokes)
    for k in ("Vx", "Vy", "Vz"):
        assert not out[k][1:-1, 1:-1, 1:-1].any(), k
    for k in ("Rx", "Ry", "Rz", "RP", "txx", "tzz", "tyz", "txz", "txy", "P"):
        assert not out[k].any(), k


def test_out_of_scope_inputs_are_refused_with_status_4(jr):
    from justrelax_jl_amd import _lib, stokes as st_mod, variational as var
    s = jr.miniapps.shearband3d_variational((8, 7, 6), iterMax=10, nout=5)
    stokes, pr, ρg = _upload(jr, s)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
    jr.update_rock_ratio_(ϕ, pr, 0)
    run = lambda grid=s.grid, phases=s.extra["phases"], handle=None, bcs=s.flow_bcs, **kw: jr.solve_VariationalStokes_(
        stokes, s.pt, grid, bcs, ρg, pr, ϕ, phases, None, s.dt, None, kwargs=dict(s.kwargs, **kw), handle=handle)
    xv = [np.linspace(0.0, 1.0, n + 1) ** 1.2 for n in s.ni]
    cases = [("non-uniform spacing", dict(grid=jr.Geometry.from_vertices(xv))),
             ("DruckerPragerCap", dict(phases=[dict(s.extra["phases"][0], cap=dict(P_T=1.0)), s.extra["phases"][1]])), ("air_phase", dict(air_phase=5))]
    for word, kw in cases:
        with pytest.raises(_lib.JrxError) as e:
            run(**kw)
        assert e.value.status == 4 and word in str(e.value), (word, str(e.value))
    # fewer than 3 cells in a dimension: the extents are checked before any array is touched
    h = _lib.default_handle()
    fd = st_mod.vep_fields3d(stokes, ρg, pr)
    pd = st_mod.vep_params3d(stokes, s.pt, s.grid, s.flow_bcs, s.dt, iterMax=10, nout=5)
    pd.nz = 2
    hist = st_mod._Hist(8)
    with pytest.raises(_lib.JrxError) as e:
        h.call("jrx_stokes3d_vs_solve", C.byref(fd), C.byref(var.rock_ratio3d(ϕ)), C.byref(st_mod.rheology_table(s.extra["phases"])), C.byref(pd), C.c_int32(0),
               C.byref(hist.c))
    assert e.value.status == 4 and "at least 3 cells" in str(e.value)
    # free-surface stabilisation: refused by the binding
    fs = jr.VelocityBoundaryConditions(free_slip=s.flow_bcs.free_slip, no_slip=s.flow_bcs.no_slip, free_surface=True)
    with pytest.raises(ValueError, match="free-surface stabilisation .* is not built in 3D"):
        run(bcs=fs)
    # a handle with a communicator of more than one rank (two ranks of this process; refused before anything is exchanged)
    from justrelax_jl_amd import halo
    hs = [_lib.Handle(stokes.P.device.index) for _ in range(2)]
    try:
        halo.init_comm_local(hs, halo.make_carts(s.ni, (2, 1, 1)))
        with pytest.raises(_lib.JrxError) as e:
            run(handle=hs[0])
        assert e.value.status == 4 and "communicator" in str(e.value)
    finally:
        for hh in hs:
            hh.close()


def _viscosity_state(jr):
    s = jr.miniapps.shearband3d_variational((9, 8, 7), air_layers=2)
    rng = np.random.default_rng(17)
    a = s.arrays
    for pre, amp in (("t", 5.0e6), ("e", 1.0e-14)):
        for c in ("xx", "yy", "zz", "yz", "xz", "xy"):
            a[pre + c][...] = rng.uniform(-amp, amp, size=a[pre + c].shape)
    a["P"][...] = rng.uniform(1.0e8, 1.0e9, size=s.ni)
    a["eta"][...] = 10.0 ** rng.uniform(19, 23, size=s.ni)
    T = np.asfortranarray(rng.uniform(600.0, 900.0, size=s.ni))
    inf = float("inf")
    phases = [dict(eta=1.0e21, G=inf, Kb=inf), dict(G=inf, Kb=inf, creep=dict(kind="dislocation", A=3.2e-20, n=3.0, E=276.0e3, V=1.0e-6, R=8.3145)),
              dict(eta=1.0e19, G=inf, Kb=inf)]
    return s, phases, T, (1.0e18, 1.0e25)


@pytest.mark.parametrize("tau", [0, 1])
@pytest.mark.parametrize("laws", ["linear", "creep"])
def test_viscosity_air_phase_zero_is_the_existing_entry_point(jr, tau, laws):
    """air_phase = 0 through jrx_vep3d_compute_viscosity_air is bit-identical to jrx_vep3d_compute_viscosity / _tauII, for linear laws and for laws that read fields"""
    from justrelax_jl_amd import _lib, stokes as st_mod
    from justrelax_jl_amd.arrays import from_numpy
    s, phases, T, cutoff = _viscosity_state(jr)
    if laws == "linear":
        phases = s.extra["phases"]
    h = _lib.default_handle()
    stokes, pr, ρg = _upload(jr, s)
    args = dict(T=from_numpy(T, stokes.P.device))
    (jr.compute_viscosity_τII_ if tau else jr.compute_viscosity_)(stokes, pr, args, phases, cutoff, relaxation=0.3)
    want = jr.to_numpy(stokes.viscosity.η)
    stokes, pr, ρg = _upload(jr, s)
    args = dict(T=from_numpy(T, stokes.P.device))
    fd = st_mod.vep_fields3d(stokes, ρg, pr, args)
    pd = st_mod.vep_params3d(stokes, s.pt, s.grid, None, 1.0, viscosity_cutoff=cutoff)
    h.call("jrx_vep3d_compute_viscosity_air", C.byref(fd), C.byref(st_mod.rheology_table(phases)), C.byref(pd), C.c_double(0.3), C.c_int32(0), C.c_int32(tau))
    got = jr.to_numpy(stokes.viscosity.η)
    assert np.array_equal(got, want) and not np.array_equal(got, s.arrays["eta"])


@pytest.mark.parametrize("tau", [False, True])
def test_viscosity_air_phase_matches_restatement(jr, tau):
    """compute_viscosity! / update_viscosity_τII! 3D with air_phase = 3: one linear and one dislocation-creep rock phase (the invariant of the stress or of the strain
    rate gathered from the twelve edges, T and P at the cell) under an air layer.  Bound 1e-12, as the 2D test: the law is pow and exp of the inputs, a few ulp each on
    either side, and the exponent (E + P V)/(R T) <= 60 carries one rounding of its argument (1.1e-16) to 7e-15 of the viscosity."""
    from justrelax_jl_amd.arrays import from_numpy
    from justrelax_jl_amd.checks import max_rel_diff
    s, phases, T, cutoff = _viscosity_state(jr)
    a = s.arrays
    stokes, pr, ρg = _upload(jr, s)
    (jr.compute_viscosity_τII_ if tau else jr.compute_viscosity_)(stokes, pr, dict(T=from_numpy(T, stokes.P.device)), phases, cutoff, relaxation=0.3, air_phase=3)
    eta0 = a["eta"].copy()
    vs.compute_viscosity_fields(a, phases, 0.3, cutoff, 3, tau, T)
    got = jr.to_numpy(stokes.viscosity.η)
    assert max_rel_diff(got, a["eta"]) <= 1e-12
    inside = (a["eta"] > cutoff[0]) & (a["eta"] < cutoff[1])
    assert inside.mean() > 0.3 and (a["eta"] != eta0).all() and (a["eta"] == cutoff[1]).any()
    mixed = (a["phase_c"][:2] > 0).all(axis=0) | ((a["phase_c"][2] > 0) & (a["phase_c"][2] < 1))
    assert mixed.any()


def test_nan_exit_leaves_the_current_stresses_in_the_callers_arrays(jr):
    """error("NaN(s)") at the first check, iteration 3: after an odd number of pointer swaps the current η, τxx, τyy, τzz and edge stresses live in the library's
    second sets and the NaN exit has to copy them back.  One phase, linear viscosity, 8^3 cells, one NaN in an interior Vx entry; the caller's arrays after the
    failed call equal those of a call that runs the same three iterations unchecked (nout > iterMax, iterMax = 2: the loop runs while iter <= iterMax) and
    returns normally."""
    from justrelax_jl_amd._lib import JrxError
    outs = []
    for iterMax, nout in ((20, 3), (2, 100)):
        s = jr.miniapps.shearband3d_variational((8, 8, 8), iterMax=iterMax, nout=nout)
        phases = [s.extra["phases"][0]]
        for k in PHASE_MEMBERS.values():
            s.arrays[k] = np.ones((1,) + s.arrays[k].shape[1:], order="F")
        s.arrays["eta"][...] = phases[0]["eta"]
        s.arrays["Vx"][1, 1, 1] = np.nan
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
    for k in ("txx", "tyy", "tzz", "tyz", "txz", "txy", "eta"):
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
        assert np.isfinite(outs[0][k]).any(), k
