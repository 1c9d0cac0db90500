"""GPU parity tests, 3D multiphase visco-elasto-plastic Stokes (Stokes3D.jl:447-668) vs the CPU oracle.
Tolerance 1e-12 of each field's max for one kernel call (observed: bit-identical), 1e-9 after tens of PT iterations."""
import ctypes as C

import numpy as np
import pytest

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
    for k, name in (("phase_c", "center"), ("phase_yz", "yz"), ("phase_xz", "xz"), ("phase_xy", "xy")):
        getattr(pr, name).copy_(from_numpy(s.arrays[k], dev))
    ρg = tuple(from_numpy(s.arrays[k], dev) for k in ("fx", "fy", "fz"))
    return st, pr, ρg


def _download(jr, st):
    return {k: jr.to_numpy(_get(st, path)) for k, path in VEP3_MAP.items()}


def _params(orc, s, **over):
    pt, b = s.pt, s.flow_bcs
    kw = dict(iterMax=s.kwargs["iterMax"], nout=s.kwargs["nout"])
    kw.update(over)
    return orc.vep_params3d(s.ni, s.grid._di["center"], s.dt, dict(r=pt.r, theta_dtau=pt.θ_dτ, eta_dtau=pt.ηdτ, eps_rel=pt.ϵ_rel, eps_abs=pt.ϵ_abs),
                            free_slip=b.free_slip, no_slip=b.no_slip, periodic=b.periodic, **kw)


def _randomize(s, seed=4, Kb=3.0, psi=6.0):
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
    return [dict(ph, Kb=Kb, psi_deg=psi) for ph in s.extra["phases"]]


@pytest.mark.parametrize("edges,ni", [(0, (13, 9, 7)), (0, (70, 5, 6)), (1, (13, 9, 7)), (1, (70, 5, 6)), (1, (125, 6, 18)), (1, (61, 7, 33)),
                                      (1, (62, 4, 16)), (1, (3, 3, 3)), (2, (70, 5, 6)), (2, (13, 9, 7)),
                                      (3, (13, 9, 7)), (3, (70, 5, 6)), (3, (125, 6, 18)), (3, (61, 7, 33)), (3, (62, 4, 16)), (3, (3, 3, 3)),
                                      (4, (13, 9, 7)), (4, (70, 5, 6)), (4, (125, 6, 18)), (4, (61, 7, 33)), (4, (62, 4, 16)), (4, (3, 3, 3)),
                                      (6, (13, 9, 7)), (6, (70, 5, 6)), (6, (125, 6, 18)), (6, (61, 7, 33)), (6, (62, 4, 16)), (6, (3, 3, 3))])
def test_update_stresses_3d_matches_oracle(jr, oracle, edges, ni):
    """update_stresses_center_vertex_ps! 3D (StressKernels.jl:671-989) on random states: yielding and elastic nodes, mixed
    phase ratios, dilatant plasticity with finite bulk modulus.  edges = 1: the z-marching edge kernel, one family per block (grids spanning one, two and three
    62-node lane segments and one to three z chunks), 2: the same as one launch per family, 3: the three family waves of a row as one workgroup sharing the
    centre operands through LDS, 4 (default): the shear operands too, 0: one node per thread."""
    from justrelax_jl_amd.checks import max_rel_diff
    pb = _stress_problem(jr, oracle, ni)
    out, _ = _stress_run(jr, pb, vep3_edges=edges)
    for k in STRESS_OUT:
        assert max_rel_diff(out[k], pb["ref"][k]) <= 1e-12, k


def test_retired_switches_are_unknown_and_edges_5_is_refused_before_anything_runs(jr, oracle):
    """vep3_fork and vep3_peel_fork are no keys any more; vep3_edges = 5 (no such form: the launch plan refuses it) makes jrx_vep3d_update_stresses return JRX_ERR_ARG with
    every stress array as it was, and the same call with the switch back at 4 matches the oracle"""
    from justrelax_jl_amd import _lib, stokes as st_mod
    from justrelax_jl_amd.arrays import from_numpy
    from justrelax_jl_amd.checks import max_rel_diff
    h = _lib.default_handle()
    for key in (b"vep3_fork", b"vep3_peel_fork"):
        with pytest.raises(_lib.JrxError) as e:
            h.call("jrx_tuning_set", C.c_char_p(key), C.c_int64(0))
        assert e.value.status == 4 and "unknown key" in str(e.value)
    s = jr.miniapps.shearband3d((13, 9, 7))
    phases = _randomize(s)
    rh = oracle.rheology_struct(phases)
    ref = {k: v.copy(order="F") for k, v in s.arrays.items()}
    rng = np.random.default_rng(9)
    theta = np.asfortranarray(rng.uniform(-1, 1, size=s.ni))
    lam = np.asfortranarray(rng.uniform(0, 0.1, size=s.ni))
    lamv = [np.asfortranarray(rng.uniform(0, 0.1, size=s.arrays[k].shape)) for k in ("tyz", "txz", "txy")]
    lam_r, lamv_r = lam.copy(order="F"), [x.copy(order="F") for x in lamv]
    oracle.vep3d_stress(ref, theta, lam_r, lamv_r, rh, _params(oracle, s))
    stokes, pr, ρg = _upload(jr, s)
    dev = stokes.P.device
    th_d, lam_d = from_numpy(theta, dev), from_numpy(lam, dev)
    lamv_d = [from_numpy(x, dev) for x in lamv]
    fd = st_mod.vep_fields3d(stokes, ρg, pr)
    pd = st_mod.vep_params3d(stokes, s.pt, s.grid, s.flow_bcs, s.dt)
    lv = (C.c_void_p * 3)(*[x.data_ptr() for x in lamv_d])
    update = lambda: h.call("jrx_vep3d_update_stresses", C.byref(fd), C.c_void_p(th_d.data_ptr()), C.c_void_p(lam_d.data_ptr()), lv,
                            C.byref(st_mod.rheology_table(phases)), C.byref(pd))
    stress = ("txx", "tyy", "tzz", "tyz", "txz", "txy", "tyz_c", "txz_c", "txy_c")
    h.call("jrx_tuning_set", C.c_char_p(b"vep3_edges"), C.c_int64(5))
    try:
        with pytest.raises(_lib.JrxError) as e:
            update()
        assert e.value.status == 4 and "vep3_edges: no such form" in str(e.value)
        out = _download(jr, stokes)
        for k in stress + ("P", "tII", "eplxx", "eplxz"):
            assert np.array_equal(out[k], s.arrays[k]), k
        assert np.array_equal(jr.to_numpy(lam_d), lam) and all(np.array_equal(jr.to_numpy(a), b) for a, b in zip(lamv_d, lamv))
    finally:
        h.call("jrx_tuning_set", C.c_char_p(b"vep3_edges"), C.c_int64(4))
    update()
    out = _download(jr, stokes)
    assert (lam_r != lam).any() and (ref["eplxz"] != 0).any()
    for k in stress + ("tII", "eta_vep", "P", "eplxx", "eplyy", "eplzz", "eplyz", "eplxz", "eplxy", "evol_pl"):
        assert max_rel_diff(out[k], ref[k]) <= 1e-12, k
    assert max_rel_diff(jr.to_numpy(lam_d), lam_r) <= 1e-12
    for a, b in zip(lamv_d, lamv_r):
        assert max_rel_diff(jr.to_numpy(a), b) <= 1e-12


def test_vep3d_solve_matches_oracle_over_iterations(jr, oracle):
    """the whole driver (pressure with phase ratios, viscosity relaxation, stress kernel, velocity sweep, BCs, norms, epilogue)
    for a fixed number of iterations on a yielding state"""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband3d((20, 12, 10), iterMax=39, nout=10)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    rng = np.random.default_rng(3)
    for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):     # pre-stress close to yield so that plasticity is active
        s.arrays["to" + c][...] = rng.uniform(-1.5, 1.5, size=s.arrays["to" + c].shape)
        s.arrays["t" + c][...] = s.arrays["to" + c]
    s.arrays["EII_pl"][...] = rng.uniform(0, 0.1, size=s.ni)
    ref = {k: v.copy(order="F") for k, v in s.arrays.items()}
    r_ref = oracle.stokes3d_vep_solve(ref, oracle.rheology_struct(s.extra["phases"]), _params(oracle, s))
    stokes, pr, ρg = _upload(jr, s)
    r = jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
    out = _download(jr, stokes)
    assert r.iter == r_ref["iter"] == 40
    assert np.allclose(r.err_evo1, r_ref["err_evo1"], rtol=1e-9) and np.allclose(r.norm_Rz, r_ref["norm_Rz"], rtol=1e-9)
    assert (ref["eplxx"] != 0).any()
    from justrelax_jl_amd.checks import interior_mask3d
    # (∇V, RP, ε_pl, ε_vol_pl, η_vep are stored by observed iterations only -- the last one is: they must still be the reference's)
    for k in ("P", "P0", "Vx", "Vy", "Vz", "Ux", "txx", "tyy", "tzz", "tyz", "txz", "txy", "tyz_c", "tII", "eta", "eta_vep", "exx", "exz", "eplxx", "eplyy", "eplzz",
              "eplxy", "eplxz", "eplyz", "evol_pl", "divV", "EII_pl", "EVol_pl", "Rx", "Rz", "RP", "toxx", "toxz", "toxy_c", "omega_yz", "omega_xz", "omega_xy", "exz_c", "eplyz_c"):
        m = interior_mask3d(k, ref[k].shape)
        scale = max(np.abs(ref[k]).max(), 1e-300)
        assert np.abs(out[k] - ref[k])[m].max() <= 1e-9 * scale, k


@pytest.mark.parametrize("nphase", [1, 3, 4, 5])
def test_update_stresses_3d_other_phase_counts(jr, oracle, nphase):
    """the z-marching edge kernel is instantiated per phase count (1..4, unrolled phase loops); five phases take the one-node-per-thread kernel"""
    from justrelax_jl_amd.checks import max_rel_diff
    pb = _stress_problem(jr, oracle, (66, 7, 19), nphase)
    out, d = _stress_run(jr, pb)
    assert d["stat_vep3_edges_node"] == (1 if nphase == 5 else 0) and d["stat_vep3_edges_kz4"] == (0 if nphase == 5 else 1), d
    for k in STRESS_OUT:
        assert max_rel_diff(out[k], pb["ref"][k]) <= 1e-12, k


@pytest.mark.parametrize("ni,iters", [((96, 80, 72), 12), ((160, 160, 160), 6), ((256, 256, 256), 4)])
def test_vep3d_solve_matches_oracle_on_a_multi_tile_grid(jr, oracle, ni, iters):
    """the whole 3D VEP driver on grids that span several 62-node lane segments, row blocks, 16-plane chunks of the z-marching edge kernel and z chunks of
    the pre kernel (160^3 and 256^3: more tiles than fit on the chip at once, every XCD slab populated; 256^3 is the size the bench quotes), yielding state, two checks"""
    from justrelax_jl_amd.checks import interior_mask3d
    s = jr.miniapps.shearband3d(ni, iterMax=iters - 1, nout=iters // 2)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    rng = np.random.default_rng(13)
    for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        s.arrays["to" + c][...] = rng.uniform(-1.5, 1.5, size=s.arrays["to" + c].shape)
        s.arrays["t" + c][...] = s.arrays["to" + c]
    ref = {k: v.copy(order="F") for k, v in s.arrays.items()}
    r_ref = oracle.stokes3d_vep_solve(ref, oracle.rheology_struct(s.extra["phases"]), _params(oracle, s))
    stokes, pr, ρg = _upload(jr, s)
    r = jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
    out = _download(jr, stokes)
    assert r.iter == r_ref["iter"] == iters
    assert np.allclose(r.err_evo1, r_ref["err_evo1"], rtol=1e-9)
    assert (ref["eplyz"] != 0).any() and (ref["eplyz"] == 0).any()
    for k in ("P", "Vx", "Vy", "Vz", "txx", "tyy", "tzz", "tyz", "txz", "txy", "tyz_c", "txz_c", "txy_c", "tII", "eta", "eta_vep", "eplxx", "eplyz", "eplxz",
              "eplxy", "EII_pl", "EVol_pl", "Rx", "Ry", "Rz", "RP"):
        m = interior_mask3d(k, ref[k].shape)
        scale = max(np.abs(ref[k]).max(), 1e-300)
        assert np.abs(out[k] - ref[k])[m].max() <= 1e-9 * scale, k


def test_tensor_invariant_and_viscosity_3d(jr, oracle):
    import torch
    from justrelax_jl_amd import stokes as st_mod
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband3d((9, 8, 7))
    phases = _randomize(s, seed=7)
    stokes, pr, ρg = _upload(jr, s)
    st_mod.tensor_invariant_(stokes.τ)
    want = np.zeros(s.ni, order="F")
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    a = s.arrays
    oracle.lib().orc_tensor_invariant3d(dp(want), *[dp(a[k]) for k in ("txx", "tyy", "tzz", "tyz", "txz", "txy")], *[C.c_int64(n) for n in s.ni])
    assert max_rel_diff(jr.to_numpy(stokes.τ.II), want) <= 1e-14
    st_mod.compute_viscosity_(stokes, pr, None, phases, relaxation=0.3)
    ref = {k: v.copy(order="F") for k, v in a.items()}
    f = oracle.vep3d(ref)
    oracle.lib().orc_compute_viscosity3d(C.byref(f), C.byref(oracle.rheology_struct(phases)), C.byref(_params(oracle, s)), C.c_double(0.3))
    assert max_rel_diff(jr.to_numpy(stokes.viscosity.η), ref["eta"]) <= 1e-14


def test_epilogue_operators_3d(jr, oracle):
    """shear2center!, accumulate_tensor!, accumulate_vol!, compute_vorticity! 3D as stand-alone operators, bit-exact"""
    from justrelax_jl_amd import stokes as st_mod
    s = jr.miniapps.shearband3d((11, 7, 6))
    _randomize(s, seed=2)
    rng = np.random.default_rng(8)
    a = s.arrays
    for k in ("Vx", "Vy", "Vz", "eplxx", "eplyy", "eplzz", "eplyz", "eplxz", "eplxy", "EII_pl", "EVol_pl", "evol_pl"):
        a[k][...] = rng.uniform(-1, 1, size=a[k].shape)
    stokes, pr, ρg = _upload(jr, s)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    n = [C.c_int64(m) for m in s.ni]
    L = oracle.lib()
    # shear2center!
    st_mod.shear2center_(stokes.ε)
    want = [np.zeros(s.ni, order="F") for _ in range(3)]
    L.orc_shear2center3d(*[dp(w) for w in want], dp(a["eyz"]), dp(a["exz"]), dp(a["exy"]), *n)
    for w, k in zip(want, ("yz_c", "xz_c", "xy_c")):
        assert np.array_equal(jr.to_numpy(getattr(stokes.ε, k)), w), k
    # accumulate_tensor! / accumulate_vol!
    II = np.zeros(s.ni, order="F")
    L.orc_tensor_invariant3d(dp(II), *[dp(a[k]) for k in ("eplxx", "eplyy", "eplzz", "eplyz", "eplxz", "eplxy")], *n)
    st_mod.accumulate_tensor_(stokes.EII_pl, stokes.ε_pl, 0.37)
    st_mod.accumulate_vol_(stokes.EVol_pl, stokes.ε_vol_pl, 0.37)
    assert np.array_equal(jr.to_numpy(stokes.EII_pl), a["EII_pl"] + II * 0.37)
    assert np.array_equal(jr.to_numpy(stokes.EVol_pl), a["EVol_pl"] + 0.37 * a["evol_pl"])
    # compute_vorticity!
    st_mod.compute_vorticity_(stokes, s.grid)
    w = [np.zeros(a[k].shape, order="F") for k in ("tyz", "txz", "txy")]
    _di = s.grid._di["center"]
    L.orc_compute_vorticity3d(*[dp(x) for x in w], dp(a["Vx"]), dp(a["Vy"]), dp(a["Vz"]), *n, *[C.c_double(d) for d in _di])
    for x, k in zip(w, ("yz", "xz", "xy")):
        assert np.array_equal(jr.to_numpy(getattr(stokes.ω, k)), x), k


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("ni,iters,nout,prekz", [((20, 12, 10), 7, 3, 0), ((20, 12, 10), 40, 10, 0), ((13, 9, 7), 5, 2, 1), ((70, 5, 6), 6, 5, 4), ((64, 64, 17), 4, 2, 8),
                                                   ((63, 31, 16), 5, 4, 16), ((127, 66, 40), 6, 3, 8), ((127, 66, 40), 5, 10 ** 9, 32), ((96, 80, 72), 35, 17, 0),
                                                   # depth 2: what the size rule picks at about 104^3 .. 120^3; odd and even plane counts, one and two lane segments
                                                   ((70, 5, 6), 6, 3, 2), ((61, 7, 33), 5, 2, 2)])
def test_vep3d_fused_pre_centre_equals_the_three_kernels(jr, ni, iters, nout, prekz, tile):
    """k_vep3_prec (pre + viscosity relaxation + centre pass in one kernel ahead of the edge pass, second sets of η and τxx/τyy/τzz adopted by pointer swap; the default without
    neighbours) against the three kernels with the centre pass behind the edge pass: every field of the solve bit for bit -- odd and even iteration counts (the copy-back of the
    second sets), observed and unobserved iterations (the output-only arrays), chunk depths that cut the column at every place, a run long enough for the captured graphs"""
    from justrelax_jl_amd import _lib
    h = _lib.default_handle()
    outs, res = [], []
    try:
        for fuse in (0, 1):
            h.set_option("vep3_fuse_pc", fuse)
            h.set_option("vep3_prekz", prekz)
            h.set_option("vep3_prec_tile", tile)
            s = jr.miniapps.shearband3d(ni, iterMax=iters - 1, nout=nout)
            s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
            rng = np.random.default_rng(3)
            for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):     # pre-stress close to yield so that plasticity is active
                s.arrays["to" + c][...] = rng.uniform(-1.5, 1.5, size=s.arrays["to" + c].shape)
                s.arrays["t" + c][...] = s.arrays["to" + c]
            stokes, pr, ρg = _upload(jr, s)
            n0 = h.get_option("stat_vep3_fused")
            r = jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
            assert r.iter == iters
            assert (h.get_option("stat_vep3_fused") > n0) == bool(fuse)
            outs.append(_download(jr, stokes))
            res.append(r)
    finally:
        h.set_option("vep3_fuse_pc", 1)
        h.set_option("vep3_prekz", 0)
        h.set_option("vep3_prec_tile", 2)
    assert (outs[0]["eplxx"] != 0).any() or iters < 5
    assert np.array_equal(np.asarray(res[0].err_evo1), np.asarray(res[1].err_evo1))
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("forces", ["none", "z", "z and one denormal in x", "xyz"])
def test_vep3d_velocity_sweep_does_not_load_body_forces_that_are_zero(jr, forces):
    """ShearBand3D.jl:114 hands three ρg arrays of zeros, a model with gravity has them in x and y.  The 3D VEP driver looks at their bits once per solve and the z-marching velocity
    sweep of unobserved iterations does not load the arrays that hold only +0.0 (k_velocity3d_zb, NOF; grids above 88^3 cells run that kernel) -- every field equals the run that
    loads them (tuning switch zero_forces = 0), bit for bit."""
    from justrelax_jl_amd import _lib
    h = _lib.default_handle()
    ni = (112, 88, 72)
    outs, res = [], []
    try:
        for zf in (1, 0):
            h.set_option("zero_forces", zf)
            s = jr.miniapps.shearband3d(ni, iterMax=6, nout=3)
            s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
            rng = np.random.default_rng(8)
            for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
                s.arrays["to" + c][...] = rng.uniform(-1.5, 1.5, size=s.arrays["to" + c].shape)
                s.arrays["t" + c][...] = s.arrays["to" + c]
            if "z" in forces:
                s.arrays["fz"][...] = rng.uniform(-1.0, 1.0, size=s.arrays["fz"].shape)
            if forces == "xyz":
                s.arrays["fx"][...] = rng.uniform(-1.0, 1.0, size=s.arrays["fx"].shape)
                s.arrays["fy"][...] = rng.uniform(-1.0, 1.0, size=s.arrays["fy"].shape)
            if "denormal" in forces:
                s.arrays["fx"][5, 7, 9] = 5e-324
            stokes, pr, ρg = _upload(jr, s)
            r = jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
            assert r.iter == 7
            outs.append(_download(jr, stokes))
            res.append(r)
    finally:
        h.set_option("zero_forces", 1)
    assert np.array_equal(np.asarray(res[0].err_evo1), np.asarray(res[1].err_evo1))
    for k in outs[0]:
        a, b = np.ascontiguousarray(outs[0][k]), np.ascontiguousarray(outs[1][k])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) or (np.array_equal(a, b) and k[0] == "e"), k


@pytest.mark.parametrize("nphase", [1, 3, 4, 5])
def test_vep3d_solve_with_other_phase_counts_fused_equals_unfused(jr, nphase):
    """the whole 3D VEP solve with 1, 3, 4 (template instantiations of the fused pre / centre, centre and per-node edge kernels) and 5 phases (run-time phase loops everywhere): the
    fused kernel against the three kernels, and the constant-phase-count instantiations against the run-time loops, every field bit for bit"""
    import torch
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.arrays import from_numpy
    ni = (66, 9, 19)
    h = _lib.default_handle()
    outs = []
    try:
        for fuse, npc in ((0, 0), (1, 1), (1, 0), (0, 1)):
            h.set_option("vep3_fuse_pc", fuse)
            h.set_option("vep3_np_const", npc)
            s = jr.miniapps.shearband3d(ni, iterMax=11, nout=5)
            s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
            rng = np.random.default_rng(40 + nphase)
            for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
                s.arrays["to" + c][...] = rng.uniform(-1.5, 1.5, size=s.arrays["to" + c].shape)
                s.arrays["t" + c][...] = s.arrays["to" + c]
            base = s.extra["phases"]
            phases = []
            for q in range(nphase):
                ph = dict(base[q % 2], Kb=3.0 + 0.5 * q, psi_deg=4.0 + q)
                ph["eta"] = ph["eta"] * (1.0 + 0.3 * q)
                ph["C"] = ph["C"] * (1.0 - 0.1 * q)
                ph["G"] = ph["G"] * (1.0 + 0.2 * q)
                phases.append(ph)
            for k in ("phase_c", "phase_yz", "phase_xz", "phase_xy"):
                shp = s.arrays[k].shape[1:]
                r = rng.dirichlet(np.ones(nphase), size=shp)
                r[rng.uniform(size=shp) < 0.3] = np.eye(nphase)[rng.integers(nphase)]
                s.arrays[k] = np.asfortranarray(np.moveaxis(r, -1, 0))
            dev = torch.device("cuda", torch.cuda.current_device())
            stokes = jr.StokesArrays(jr.AMDGPUBackend, s.ni)
            for k, path in VEP3_MAP.items():
                _get(stokes, path).copy_(from_numpy(s.arrays[k], dev))
            pr = jr.PhaseRatios(jr.AMDGPUBackend, nphase, s.ni)
            for k, name in (("phase_c", "center"), ("phase_yz", "yz"), ("phase_xz", "xz"), ("phase_xy", "xy")):
                getattr(pr, name).copy_(from_numpy(s.arrays[k], dev))
            ρg = tuple(from_numpy(s.arrays[k], dev) for k in ("fx", "fy", "fz"))
            r_ = jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, phases, None, s.dt, None, kwargs=s.kwargs)
            assert r_.iter == 12
            outs.append(_download(jr, stokes))
    finally:
        h.set_option("vep3_fuse_pc", 1)
        h.set_option("vep3_np_const", 1)
    assert (outs[0]["eplxx"] != 0).any()
    for v in (1, 2, 3):
        for k in outs[0]:
            assert np.array_equal(outs[0][k], outs[v][k], equal_nan=True), (v, k)


def test_nan_exit_leaves_the_current_stresses_in_the_callers_arrays(jr):
    """error("NaN(s)") at the first check, iteration 3: after an odd number of pointer swaps the current η, τxx, τyy, τzz (fused pre / centre kernel) and edge stresses
    live in the library's second sets and the NaN exit has to copy them back.  One phase, linear viscosity, 8^3 cells, one NaN in an interior Vx entry; the caller's
    arrays after the failed call equal those of a call that runs the same three iterations unchecked (nout > iterMax, iterMax = 2: the loop runs while
    iter <= iterMax) and returns normally."""
    from justrelax_jl_amd import _lib
    h = _lib.default_handle()
    outs = []
    for iterMax, nout in ((20, 3), (2, 100)):
        s = jr.miniapps.shearband3d((8, 8, 8), iterMax=iterMax, nout=nout)
        phases = [s.extra["phases"][0]]
        for k in ("phase_c", "phase_yz", "phase_xz", "phase_xy"):
            s.arrays[k] = np.ones((1,) + s.arrays[k].shape[1:], order="F")
        s.arrays["eta"][...] = phases[0]["eta"]
        s.arrays["Vx"][1, 1, 1] = np.nan
        stokes, pr, ρg = _upload(jr, s)
        n0 = h.get_option("stat_vep3_fused")
        solve = lambda: jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, phases, None, s.dt, None, kwargs=s.kwargs)
        if nout == 3:
            with pytest.raises(_lib.JrxError) as e:
                solve()
            assert e.value.status == 1 and "JRX_ERR_NAN" in str(e.value)
        else:
            r = solve()
            assert r.iter == 3 and len(r.err_evo1) == 0
        assert h.get_option("stat_vep3_fused") == n0 + 3          # η and the normal stresses swap too
        outs.append(_download(jr, stokes))
    assert np.isnan(outs[0]["txx"]).any()
    for k in ("txx", "tyy", "tzz", "tyz", "txz", "txy", "eta"):
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
        assert np.isfinite(outs[0][k]).any(), k


# ---- the forms of the 3D VEP kernels that only a tuning switch (or, in production, the size rule of vep3_plan_edges) selects.  Anchor of the bit comparisons: the
# one-node-per-thread edge kernel (vep3_edges = 0), itself compared with the oracle at the same shape.
VEP3_COUNTERS = ("stat_vep3_edges_kz16", "stat_vep3_edges_kz8", "stat_vep3_edges_kz4", "stat_vep3_edges_mb3", "stat_vep3_edges_peel", "stat_vep3_edges_node",
                 "stat_vep3_edges_node_nomap", "stat_vep3_edges_node_noxcd", "stat_vep3_fused", "stat_vep_store_all")
VEP3_DEFAULTS = dict(vep3_edges=4, vep3_cfg=0, vep3_peel=1, vep3_map=1, vep3_xcd=1, vep3_nt=0, vep3_fuse_pc=1, vep_store_all=0)
STRESS_OUT = ("txx", "tyy", "tzz", "tyz", "txz", "txy", "tyz_c", "txz_c", "txy_c", "tII", "eta_vep", "P", "eplxx", "eplyy", "eplzz", "eplyz", "eplxz", "eplxy", "evol_pl",
              "lam", "lamv0", "lamv1", "lamv2")


def _stress_problem(jr, oracle, ni, nphase=2):
    """a random state for one update_stresses_center_vertex_ps! call (as test_update_stresses_3d_matches_oracle builds it; other phase counts as
    test_update_stresses_3d_other_phase_counts) and the oracle's result, computed once per test"""
    s = jr.miniapps.shearband3d(ni)
    phases = _randomize(s)
    rng = np.random.default_rng(40 + nphase)
    if nphase != 2:
        base, phases = s.extra["phases"], []
        for q in range(nphase):
            ph = dict(base[q % 2], Kb=3.0 + 0.5 * q, psi_deg=4.0 + q)
            ph["eta"], ph["C"], ph["G"] = ph["eta"] * (1.0 + 0.3 * q), ph["C"] * (1.0 - 0.1 * q), ph["G"] * (1.0 + 0.2 * q)
            phases.append(ph)
        for k in ("phase_c", "phase_yz", "phase_xz", "phase_xy"):
            shp = s.arrays[k].shape[1:]
            r = rng.dirichlet(np.ones(nphase), size=shp)                      # ratios sum to 1
            r[rng.uniform(size=shp) < 0.3] = np.eye(nphase)[rng.integers(nphase)]    # some pure cells
            s.arrays[k] = np.asfortranarray(np.moveaxis(r, -1, 0))
    rng = np.random.default_rng(9)
    theta = np.asfortranarray(rng.uniform(-1, 1, size=s.ni))
    lam = np.asfortranarray(rng.uniform(0, 0.1, size=s.ni))
    lamv = [np.asfortranarray(rng.uniform(0, 0.1, size=s.arrays[k].shape)) for k in ("tyz", "txz", "txy")]
    ref = {k: v.copy(order="F") for k, v in s.arrays.items()}
    lam_r, lamv_r = lam.copy(order="F"), [x.copy(order="F") for x in lamv]
    oracle.vep3d_stress(ref, theta, lam_r, lamv_r, oracle.rheology_struct(phases), _params(oracle, s))
    assert (lam_r != lam).any() and (lam_r == lam).any() and (ref["eplxz"] != 0).any() and (ref["eplxz"] == 0).any()      # yielding and elastic nodes
    ref.update(lam=lam_r, lamv0=lamv_r[0], lamv1=lamv_r[1], lamv2=lamv_r[2])
    return dict(s=s, phases=phases, theta=theta, lam=lam, lamv=lamv, ref=ref)


def _stress_run(jr, pb, **switches):
    """jrx_vep3d_update_stresses on a fresh upload of the problem with the given switches; returns (every downloaded array + λ, λv; the deltas of VEP3_COUNTERS by name)"""
    from justrelax_jl_amd import _lib, stokes as st_mod
    from justrelax_jl_amd.arrays import from_numpy
    s = pb["s"]
    stokes, pr, ρg = _upload(jr, s)
    dev = stokes.P.device
    th_d, lam_d = from_numpy(pb["theta"], dev), from_numpy(pb["lam"], dev)
    lamv_d = [from_numpy(x, dev) for x in pb["lamv"]]
    h = _lib.default_handle()
    fd = st_mod.vep_fields3d(stokes, ρg, pr)
    pd = st_mod.vep_params3d(stokes, s.pt, s.grid, s.flow_bcs, s.dt)
    lv = (C.c_void_p * 3)(*[x.data_ptr() for x in lamv_d])
    try:
        for k, v in switches.items():
            h.set_option(k, v)
        c0 = [h.get_option(k) for k in VEP3_COUNTERS]
        h.call("jrx_vep3d_update_stresses", C.byref(fd), C.c_void_p(th_d.data_ptr()), C.c_void_p(lam_d.data_ptr()), lv, C.byref(st_mod.rheology_table(pb["phases"])), C.byref(pd))
        d = {k: h.get_option(k) - c for k, c in zip(VEP3_COUNTERS, c0)}
    finally:
        for k, v in VEP3_DEFAULTS.items():
            h.set_option(k, v)
    out = _download(jr, stokes)
    out.update(lam=jr.to_numpy(lam_d), lamv0=jr.to_numpy(lamv_d[0]), lamv1=jr.to_numpy(lamv_d[1]), lamv2=jr.to_numpy(lamv_d[2]))
    return out, d


def _stress_anchor(jr, pb):
    """the node kernel (vep3_edges = 0, default thread map), within 1e-12 of the oracle"""
    from justrelax_jl_amd.checks import max_rel_diff
    out, d = _stress_run(jr, pb, vep3_edges=0)
    assert d["stat_vep3_edges_node"] == 1 and d["stat_vep3_edges_node_nomap"] == d["stat_vep3_edges_node_noxcd"] == 0, d
    assert d["stat_vep3_edges_kz16"] == d["stat_vep3_edges_kz8"] == d["stat_vep3_edges_kz4"] == d["stat_vep3_edges_peel"] == 0, d
    for k in STRESS_OUT:
        assert max_rel_diff(out[k], pb["ref"][k]) <= 1e-12, k
    return out


def _assert_stress_form(jr, pb, anchor, want, **switches):
    """one form: within the file's bound of the oracle, equal to the anchor in every array, and the counters say that it ran"""
    from justrelax_jl_amd.checks import max_rel_diff
    out, d = _stress_run(jr, pb, **switches)
    full = dict({k: 0 for k in VEP3_COUNTERS}, **want)
    assert d == full, (switches, d, full)
    for k in STRESS_OUT:
        assert max_rel_diff(out[k], pb["ref"][k]) <= 1e-12, (switches, k)
    for k in out:
        assert np.array_equal(out[k], anchor[k]), (switches, k)


@pytest.mark.parametrize("edges,cfg,ni", [(e, c, ni) for e, c in ((4, 162), (4, 82), (4, 42), (1, 163), (1, 82)) for ni in ((70, 5, 6), (125, 6, 18), (61, 7, 33), (62, 4, 16))])
def test_update_stresses_3d_edge_kernel_configurations(jr, oracle, edges, cfg, ni):
    """the table of test_update_stresses_3d_matches_oracle with a `cfg` column (vep3_cfg = chunk depth * 10 + min blocks per CU).  Left to itself the plan of that test's small
    grids halves the depth of form 4 to 4 planes; production grids of about 100^3 to 150^3 run 8 planes (128^3: 2 x 129 x 9 = 2,322 < 3,000 blocks at depth 16, 4,386 at depth 8)
    and larger ones 16.  Form 4 at 16, 8 and 4 planes and form 1 at 16 planes / three blocks per CU and 8 planes / two, on one, two and three lane segments (the last one
    peeled at nx = 125) and nz + 1 = 7, 17, 19, 34 planes (a part of a chunk, one chunk of 16 and one plane, two chunks of 8 and three planes, ...).  Each is within 1e-12 of
    the oracle and equals the node kernel (vep3_edges = 0) in every array, bit for bit; the stat_vep3_edges_* counters show the depth that ran."""
    pb = _stress_problem(jr, oracle, ni)
    anchor = _stress_anchor(jr, pb)
    want = {"stat_vep3_edges_kz%d" % (cfg // 10): 1, "stat_vep3_edges_mb3": int(cfg % 10 == 3), "stat_vep3_edges_peel": int(ni[0] == 125)}
    _assert_stress_form(jr, pb, anchor, want, vep3_edges=edges, vep3_cfg=cfg)


@pytest.mark.parametrize("edges", [4, 1])
@pytest.mark.parametrize("nphase", [1, 2, 3, 4])
def test_update_stresses_3d_eight_plane_chunks_with_other_phase_counts(jr, oracle, nphase, edges):
    """the 8-plane instantiations of the z-marching edge kernels exist per phase count (1..4): (66, 7, 19) is two lane segments and 20 planes = two chunks of 8 and four planes"""
    pb = _stress_problem(jr, oracle, (66, 7, 19), nphase)
    anchor = _stress_anchor(jr, pb)
    _assert_stress_form(jr, pb, anchor, dict(stat_vep3_edges_kz8=1), vep3_edges=edges, vep3_cfg=82)


@pytest.mark.parametrize("edges", [1, 3, 4, 6])
def test_update_stresses_3d_without_the_peel_launch(jr, oracle, edges):
    """vep3_peel = 0 at (125, 6, 18): 126 node columns are two full lane segments and two columns; by default those two go to the node kernel in a launch of their own, with the
    switch off the z-marching kernel runs a third, nearly empty segment"""
    pb = _stress_problem(jr, oracle, (125, 6, 18))
    anchor = _stress_anchor(jr, pb)
    kz = "stat_vep3_edges_kz4" if edges == 4 else "stat_vep3_edges_kz16"          # form 4 halves its depth on a launch this small; the others are built for 16 planes
    _assert_stress_form(jr, pb, anchor, {kz: 1, "stat_vep3_edges_peel": 1}, vep3_edges=edges)      # the default, for the counter's sake
    _assert_stress_form(jr, pb, anchor, {kz: 1}, vep3_edges=edges, vep3_peel=0)


@pytest.mark.parametrize("ni", [(13, 9, 7), (70, 5, 6), (125, 6, 18)])
def test_update_stresses_3d_thread_maps_of_the_node_kernel(jr, oracle, ni):
    """vep3_map / vep3_xcd act on the one-node-per-thread edge kernel (vep3_edges = 0; the z-marching kernels have one map): 64 x 4 tiles of node columns dealt to the XCDs in
    slabs with a constant phase count (default), the tiles alone (vep3_xcd = 0), consecutive nodes (vep3_map = 0, with either value of vep3_xcd)"""
    pb = _stress_problem(jr, oracle, ni)
    anchor = _stress_anchor(jr, pb)
    _assert_stress_form(jr, pb, anchor, dict(stat_vep3_edges_node=1, stat_vep3_edges_node_noxcd=1), vep3_edges=0, vep3_xcd=0)
    _assert_stress_form(jr, pb, anchor, dict(stat_vep3_edges_node=1, stat_vep3_edges_node_nomap=1), vep3_edges=0, vep3_map=0)
    _assert_stress_form(jr, pb, anchor, dict(stat_vep3_edges_node=1, stat_vep3_edges_node_nomap=1), vep3_edges=0, vep3_map=0, vep3_xcd=0)


SOLVE_OUT = ("P", "P0", "Vx", "Vy", "Vz", "Ux", "txx", "tyy", "tzz", "tyz", "txz", "txy", "tyz_c", "tII", "eta", "eta_vep", "exx", "exz", "eplxx", "eplyy", "eplzz",
             "eplxy", "eplxz", "eplyz", "evol_pl", "divV", "EII_pl", "EVol_pl", "Rx", "Rz", "RP", "toxx", "toxz", "toxy_c", "omega_yz", "omega_xz", "omega_xy", "exz_c", "eplyz_c")


def _solve_problem(jr, oracle, ni=(20, 12, 10), iterMax=39, nout=10):
    """the short solve of test_vep3d_solve_matches_oracle_over_iterations (pre-stress close to yield) and the oracle's result"""
    s = jr.miniapps.shearband3d(ni, iterMax=iterMax, nout=nout)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    rng = np.random.default_rng(3)
    for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        s.arrays["to" + c][...] = rng.uniform(-1.5, 1.5, size=s.arrays["to" + c].shape)
        s.arrays["t" + c][...] = s.arrays["to" + c]
    s.arrays["EII_pl"][...] = rng.uniform(0, 0.1, size=s.ni)
    ref = {k: v.copy(order="F") for k, v in s.arrays.items()}
    r_ref = oracle.stokes3d_vep_solve(ref, oracle.rheology_struct(s.extra["phases"]), _params(oracle, s))
    assert (ref["eplxx"] != 0).any()
    return s, ref, r_ref


def _solve_run(jr, s, ref, r_ref, **switches):
    """the device solve with the given switches, compared with the oracle at the file's bound over iterations; returns (downloaded arrays, error history, counter deltas)"""
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.checks import interior_mask3d
    h = _lib.default_handle()
    stokes, pr, ρg = _upload(jr, s)
    try:
        for k, v in switches.items():
            h.set_option(k, v)
        c0 = [h.get_option(k) for k in VEP3_COUNTERS]
        r = jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
        d = {k: h.get_option(k) - c for k, c in zip(VEP3_COUNTERS, c0)}
    finally:
        for k, v in VEP3_DEFAULTS.items():
            h.set_option(k, v)
    out = _download(jr, stokes)
    assert r.iter == r_ref["iter"]
    assert np.allclose(r.err_evo1, r_ref["err_evo1"], rtol=1e-9) and np.allclose(r.norm_Rz, r_ref["norm_Rz"], rtol=1e-9)
    for k in SOLVE_OUT:
        m = interior_mask3d(k, ref[k].shape)
        assert np.abs(out[k] - ref[k])[m].max() <= 1e-9 * max(np.abs(ref[k]).max(), 1e-300), (switches, k)
    return out, np.asarray(r.err_evo1), d


@pytest.mark.parametrize("edges", [4, 1])
@pytest.mark.parametrize("fuse", [0, 1])
def test_vep3d_solve_with_non_temporal_stores_keeps_the_bits(jr, oracle, fuse, edges):
    """vep3_nt = 1: the kernels of the solve loop store their outputs with non-temporal stores -- the pre, viscosity and centre kernels (vep3_fuse_pc = 0), the fused pre / centre
    kernel (1), and the edge pass (the node kernel on a grid this small; vep3_edges = 1: the z-marching kernel).  (66, 9, 19), 12 iterations, checks at 5 and 10: both runs are
    within 1e-9 of the oracle and equal each other in every array, bit for bit."""
    s, ref, r_ref = _solve_problem(jr, oracle, (66, 9, 19), 11, 5)
    runs = [_solve_run(jr, s, ref, r_ref, vep3_nt=nt, vep3_fuse_pc=fuse, vep3_edges=edges) for nt in (0, 1)]
    for out, err, d in runs:
        assert (d["stat_vep3_fused"] > 0) == bool(fuse), d                         # the fused pre / centre kernel ran, or the three kernels
        assert (d["stat_vep3_edges_node"] > 0) == (edges == 4) and (d["stat_vep3_edges_kz16"] > 0) == (edges == 1), d
    assert np.array_equal(runs[0][1], runs[1][1])
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k


def test_vep3d_solve_that_stores_every_iteration_keeps_the_bits(jr, oracle):
    """vep_store_all = 1: every iteration stores ∇V, RP, ε_pl, ε_vol_pl, τII, η_vep; by default only the iterations whose results can be observed do (A.obs).  The last iteration
    is observed, so at the end every array -- the output-only ones included -- equals the other run's bit for bit, and both runs are within 1e-9 of the oracle."""
    s, ref, r_ref = _solve_problem(jr, oracle)
    runs = [_solve_run(jr, s, ref, r_ref, vep_store_all=v) for v in (0, 1)]
    assert all(d["stat_vep3_fused"] > 0 and d["stat_vep3_edges_node"] > 0 for _, _, d in runs)      # the default kernels of a grid this small, with and without their stores
    assert runs[0][2]["stat_vep_store_all"] == 0 and runs[1][2]["stat_vep_store_all"] > 0               # unobserved iterations that stored because of the switch
    assert np.array_equal(runs[0][1], runs[1][1])
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
