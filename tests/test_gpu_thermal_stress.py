"""GPU tests of the thermal stresses of the multiphase VEP drivers (args.ΔT: compute_P! gains α ΔT / dt, PressureKernels.jl:64-85,129-152,197-206).

1. The solve with args.ΔT and Q = 0 against the solve without it and Q = α_c ΔT, at dt = 0.25, every field and the error history bit for bit (the identity is pinned on the
   CPU in tests/test_thermal_stress_restatement.py) -- every pre-kernel form of both drivers.
2. jrx_vep2d_compute_P / jrx_vep3d_compute_P against the restatement at dt = 0.3, Q != 0.  Tolerance: the project's standing rule (tests/test_gpu_dyrel.py): 16 x the largest
   difference between the float64 and the longdouble evaluation of the restatement, relative to the array's max-norm.
3. The known answer of a closed box heated uniformly: V = 0, P = P_initial + Kb α δ.
4. No-ops and refusals."""
import numpy as np
import pytest

import _thermal_stress as ts

pytestmark = pytest.mark.gpu

MAP2 = dict(P="P", P0="P0", divV="divV", Q="Q", Vx="V.Vx", Vy="V.Vy", Ux="U.Ux", Uy="U.Uy", exx="ε.xx", eyy="ε.yy", exy="ε.xy", exy_c="ε.xy_c",
            eplxx="ε_pl.xx", eplyy="ε_pl.yy", eplxy="ε_pl.xy", eplxy_c="ε_pl.xy_c", txx="τ.xx", tyy="τ.yy", txy="τ.xy", txy_c="τ.xy_c",
            tII="τ.II", toxx="τ_o.xx", toyy="τ_o.yy", toxy="τ_o.xy", toxy_c="τ_o.xy_c", eta="viscosity.η", eta_v="viscosity.ηv",
            eta_vep="viscosity.η_vep", EII_pl="EII_pl", evol_pl="ε_vol_pl", EVol_pl="EVol_pl", RP="R.RP", Rx="R.Rx", Ry="R.Ry", omega_xy="ω.xy",
            dexy="Δε.xy", dexy_c="Δε.xy_c")
SI2 = dict(dexx="Δε.xx", deyy="Δε.yy", divU="∇U")          # allocated on first use by the strain_increment form, which writes them
MAP3 = dict(P="P", P0="P0", divV="divV", Q="Q", Vx="V.Vx", Vy="V.Vy", Vz="V.Vz", Ux="U.Ux", Uy="U.Uy", Uz="U.Uz", tII="τ.II",
            eta="viscosity.η", eta_vep="viscosity.η_vep", EII_pl="EII_pl", evol_pl="ε_vol_pl", EVol_pl="EVol_pl",
            RP="R.RP", Rx="R.Rx", Ry="R.Ry", Rz="R.Rz", omega_yz="ω.yz", omega_xz="ω.xz", omega_xy="ω.xy")
for _pre, _t in dict(e="ε", epl="ε_pl", t="τ", to="τ_o", de="Δε").items():
    for _c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        if _pre != "de" or _c not in ("xx", "yy", "zz"):
            MAP3[_pre + _c] = f"{_t}.{_c}"
PHASE3 = (("phase_c", "center"), ("phase_yz", "yz"), ("phase_xz", "xz"), ("phase_xy", "xy"))
PHASE2 = (("phase_c", "center"), ("phase_v", "vertex"))


def _get(o, path):
    for p in path.split("."):
        o = getattr(o, p)
    return o


def _phases(nph=2, plastic=True):
    pl = dict(C=1.6 / np.cos(np.radians(30.0)), phi_deg=30.0, psi_deg=5.0, eta_vp=8.0e-3) if plastic else {}
    ph = [dict(eta=1.0, G=1.0, Kb=4.0, density=dict(kind="T", rho0=1.0, alpha=0.25), g=0.0, **pl),
          dict(eta=0.5, G=0.5, Kb=3.0, density=dict(kind="PT", rho0=1.0, alpha=0.5), **pl)]
    return ph[:nph]


class Problem:
    """random state of a two-phase box with mixed cells; ΔT of O(1) in both extents, the ghost ring of the larger one holding values that a shifted read would show"""

    def __init__(self, jr, ni, dt, seed=5, Q=False, nph=2, plastic=True, xvi=None):
        from justrelax_jl_amd.miniapps.stokes2d import _vep_shapes2d
        from justrelax_jl_amd.miniapps.stokes3d import vep_shapes3d
        self.jr, self.ni, self.dt, self.nd = jr, tuple(ni), dt, len(ni)
        rng = np.random.default_rng(seed)
        shapes = _vep_shapes2d(*ni, nph) if self.nd == 2 else vep_shapes3d(ni, nph)
        a = {k: np.zeros(s, order="F") for k, s in shapes.items()}
        for k in a:
            if k[0] in "VPt" and not k.startswith("phase"):      # V, P, τ, τ_o
                a[k][...] = rng.uniform(-0.5, 0.5, size=a[k].shape)
        for k in ("eta", "eta_v"):
            if k in a:
                a[k][...] = 10.0 ** rng.uniform(-0.5, 0.5, size=a[k].shape)
        for k in a:
            if k.startswith("phase") and nph == 2:
                r = rng.uniform(0.0, 1.0, size=a[k].shape[1:])
                r[rng.uniform(size=r.shape) < 0.3] = 0.0
                r[rng.uniform(size=r.shape) < 0.3] = 1.0
                a[k][0], a[k][1] = r, 1.0 - r
            elif k.startswith("phase"):
                a[k][...] = 1.0
        if Q:
            a["Q"][...] = rng.uniform(-0.5, 0.5, size=a["Q"].shape)
        self.a = a
        self.dT = {0: np.asfortranarray(rng.uniform(-1.5, 1.5, size=self.ni))}
        g = np.asfortranarray(rng.uniform(20.0, 30.0, size=tuple(n + 2 for n in ni)))      # ghost ring and shifted interior: far from the values at [I...]
        g[tuple(slice(0, n) for n in ni)] = self.dT[0]
        self.dT[1] = g
        self.phases = _phases(nph, plastic)
        li = (1.0,) * self.nd
        jr.init_global_grid(*(tuple(ni) + (1,) * (3 - self.nd)))
        self.grid = jr.Geometry(ni, li) if xvi is None else jr.Geometry.from_vertices(xvi)
        self.di = tuple(l / n for l, n in zip(li, ni))
        self._di = tuple(1.0 / d for d in self.di)
        self.pt = jr.PTStokesCoeffs(li, self.di, ϵ_rel=1e-30, ϵ_abs=1e-30)
        on = {f: True for f in (("left", "right", "top", "bot") + (("front", "back") if self.nd == 3 else ()))}
        self.bcs = jr.VelocityBoundaryConditions(free_slip=on, no_slip={f: False for f in on})
        self.map = MAP2 if self.nd == 2 else MAP3

    def rheology(self, update_rho):
        """update_rho: the density laws also recompute ρg inside the loop (the control-flow forms of the pre kernels); else ρg stays the caller's (has_density = 0: the batch
        form in 2D, the constant-phase-count forms in 3D) while α is still that of the laws"""
        from justrelax_jl_amd import stokes as st
        rh = st.rheology_table(self.phases)
        if not update_rho:
            rh.has_density = 0
        return rh

    def upload(self, Q=None):
        import torch
        from justrelax_jl_amd.arrays import from_numpy
        jr = self.jr
        dev = torch.device("cuda", torch.cuda.current_device())
        st = jr.StokesArrays(jr.AMDGPUBackend, self.ni)
        for k, path in self.map.items():
            _get(st, path).copy_(from_numpy(self.a[k] if not (k == "Q" and Q is not None) else Q, dev))
        pr = jr.PhaseRatios(jr.AMDGPUBackend, self.a["phase_c"].shape[0], self.ni)
        for k, name in (PHASE2 if self.nd == 2 else PHASE3):
            getattr(pr, name).copy_(from_numpy(self.a[k], dev))
        ρg = tuple(from_numpy(self.a[k], dev) for k in ("fx", "fy", "fz")[:self.nd])
        return st, pr, ρg

    def download(self, st, extra=()):
        m = dict(self.map, **{k: SI2[k] for k in extra})
        return {k: self.jr.to_numpy(_get(st, path)) for k, path in m.items()}

    def dT_dev(self, ghosted):
        import torch
        from justrelax_jl_amd.arrays import from_numpy
        return from_numpy(self.dT[ghosted], torch.device("cuda", torch.cuda.current_device()))

    def solve(self, rh, args, Q=None, **kw):
        st, pr, ρg = self.upload(Q)
        kwargs = dict(verbose=False, viscosity_cutoff=(1.0e-2, 1.0e2), **kw)
        r = self.jr.solve_(st, self.pt, self.grid, self.bcs, ρg, pr, rh, args, self.dt, None, kwargs=kwargs)
        out = self.download(st, extra=SI2 if kw.get("strain_increment") else ())
        for k, t in zip(("fx", "fy", "fz"), ρg):          # ρg: the density-updating forms rewrite its last component
            out[k] = self.jr.to_numpy(t)
        return r, out


def _same_solve(p, rh, ghosted, iters, nout, **kw):
    """the solve with args.ΔT and Q = 0 against the solve without it and Q = α_c ΔT: every field but Q itself, and the error history, bit for bit"""
    Qs = np.asfortranarray(ts.thermal_source_Q(p.phases, p.a["phase_c"], p.dT[ghosted], p.ni))
    assert (Qs != 0).all() and len(np.unique(ts.fn_ratio(ts.phase_alpha(p.phases), p.a["phase_c"], True))) > 2       # mixed cells are present
    ra, A = p.solve(rh, dict(ΔT=p.dT_dev(ghosted)), iterMax=iters - 1, nout=nout, **kw)
    rb, B = p.solve(rh, None, Q=Qs, iterMax=iters - 1, nout=nout, **kw)
    assert ra.iter == rb.iter == iters
    assert len(ra.err_evo1) == iters // nout and np.array_equal(np.asarray(ra.err_evo1), np.asarray(rb.err_evo1))
    for k in A:
        if k != "Q":
            assert np.array_equal(A[k], B[k]), k
    assert np.isfinite(A["P"]).all() and (A["P"] != p.a["P"]).all()
    return A


@pytest.mark.parametrize("ghosted", [0, 1])
@pytest.mark.parametrize("ni,iters,nout,form", [((6, 5), 5, 2, "batch"), ((67, 35), 7, 3, "batch"), ((67, 35), 6, 2, "control_flow"), ((67, 35), 5, 2, "strain_increment"),
                                                ((6, 5), 6, 3, "nonuniform"), ((6, 5), 81, 40, "batch")])
def test_2d_driver_equals_the_isothermal_driver_with_the_source_in_Q(jr, ni, iters, nout, form, ghosted):
    """jrx_stokes2d_vep_solve: k_vep_pre_b (batch), k_vep_pre with update_ρg! (control_flow), k_vep_pre + the strain_increment pass, k_vep_pre on a non-uniform grid; the last
    case is long enough for the captured graphs of 32 iterations"""
    xvi = None
    if form == "nonuniform":
        xvi = tuple(np.cumsum(np.concatenate([[0.0], w / w.sum()])) for w in (np.linspace(1.0, 2.0, ni[0]), np.linspace(1.5, 1.0, ni[1])))
    p = Problem(jr, ni, 0.25, xvi=xvi)
    kw = dict(iterMin=1, strain_increment=True) if form == "strain_increment" else dict(iterMin=1)
    _same_solve(p, p.rheology(update_rho=form == "control_flow"), ghosted, iters, nout, **kw)


@pytest.mark.parametrize("ghosted", [0, 1])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("ni,iters,nout,prekz,rho", [((13, 9, 7), 5, 2, 1, False), ((70, 5, 6), 6, 3, 4, False), ((20, 12, 10), 7, 3, 0, False), ((20, 12, 10), 6, 2, 0, True),
                                                     ((13, 9, 7), 41, 20, 1, False)])
def test_3d_driver_equals_the_isothermal_driver_with_the_source_in_Q(jr, ni, iters, nout, prekz, rho, fuse, ghosted):
    """jrx_stokes3d_vep_solve: the fused k_vep3_prec and the three-kernel path with k_vep3_pre at the chunk depths 1, 4 and the planned one; rho: the forms with update_ρg!;
    the last case is long enough for the captured graphs of 16 iterations"""
    from justrelax_jl_amd import _lib
    h = _lib.default_handle()
    p = Problem(jr, ni, 0.25)
    try:
        h.set_option("vep3_fuse_pc", fuse)
        h.set_option("vep3_prekz", prekz)
        n0 = h.get_option("stat_vep3_fused")
        _same_solve(p, p.rheology(update_rho=rho), ghosted, iters, nout)
        assert (h.get_option("stat_vep3_fused") > n0) == bool(fuse)
    finally:
        h.set_option("vep3_fuse_pc", 1)
        h.set_option("vep3_prekz", 0)


@pytest.mark.parametrize("ghosted", [0, 1])
@pytest.mark.parametrize("ni,iters,nout,prekz,rho", [((13, 9, 7), 5, 2, 1, False), ((20, 12, 10), 7, 3, 0, False), ((20, 12, 10), 6, 2, 0, True)])
def test_3d_fused_thermal_form_equals_the_three_kernels_at_a_dt_that_rounds(jr, ni, iters, nout, prekz, rho, ghosted):
    """dt = 0.3, Q != 0 and args.ΔT: there the grouping of the three terms of rhs shows in the last bit.  k_vep3_prec<TH> (fused) against k_vep3_pre<TH> + viscosity + centre
    pass, every field and the error history bit for bit; k_vep3_pre<TH> itself is held to the restatement at this dt below"""
    from justrelax_jl_amd import _lib
    h = _lib.default_handle()
    p = Problem(jr, ni, 0.3, Q=True)
    rh = p.rheology(update_rho=rho)
    outs = []
    try:
        h.set_option("vep3_prekz", prekz)
        for fuse in (0, 1):
            h.set_option("vep3_fuse_pc", fuse)
            n0 = h.get_option("stat_vep3_fused")
            outs.append(p.solve(rh, dict(ΔT=p.dT_dev(ghosted)), iterMax=iters - 1, nout=nout))
            assert (h.get_option("stat_vep3_fused") > n0) == bool(fuse)
        riso, iso = p.solve(rh, None, iterMax=iters - 1, nout=nout)
    finally:
        h.set_option("vep3_fuse_pc", 1)
        h.set_option("vep3_prekz", 0)
    (ra, A), (rb, B) = outs
    assert ra.iter == rb.iter == iters and np.array_equal(np.asarray(ra.err_evo1), np.asarray(rb.err_evo1))
    for k in A:
        assert np.array_equal(A[k], B[k]), k
    assert not np.array_equal(A["P"], iso["P"])          # the term is there


def _close(name, got, f64, ld, factor=16.0):
    scale = float(np.max(np.abs(f64))) or 1.0
    bound = factor * float(np.max(np.abs(f64.astype(np.longdouble) - ld))) / scale
    err = float(np.max(np.abs(got - f64))) / scale
    print(f"{name}: |gpu - f64| = {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound, (name, err, bound)


def _compute_P_case(jr, p, thermal, ghosted):
    import torch
    from justrelax_jl_amd.arrays import from_numpy
    rng = np.random.default_rng(17)
    theta = np.asfortranarray(rng.uniform(-1.0, 1.0, size=p.ni))
    p.a["P0"][...] = rng.uniform(-1.0, 1.0, size=p.ni)
    st, pr, ρg = p.upload()
    before = p.download(st)
    th = from_numpy(theta, torch.device("cuda", torch.cuda.current_device()))
    args = dict(ΔT=p.dT_dev(ghosted)) if thermal else None
    jr.compute_P_(st, th, p.pt, p.grid, pr, p.rheology(update_rho=False), args, p.dt)
    after = p.download(st)
    after["theta"] = jr.to_numpy(th)
    ref = []
    for T in (np.float64, np.longdouble):
        a = ts.astype(dict(p.a, theta=theta), T)
        ref.append(ts.pre_pass(a, p.phases, p._di, p.dt, p.pt.r, p.pt.θ_dτ, dT=p.dT[ghosted].astype(T) if thermal else None))
    written = ("theta", "RP", "divV") + (("exx", "eyy", "exy") if p.nd == 2 else ("exx", "eyy", "ezz", "eyz", "exz", "exy"))
    for k in written:
        _close(k, after[k], ref[0][k], ref[1][k])
    for k in before:
        if k not in written:
            assert np.array_equal(before[k], after[k]), k
    return after


@pytest.mark.parametrize("thermal,ghosted", [(False, 0), (True, 0), (True, 1)])
@pytest.mark.parametrize("ni,batch", [((6, 5), 1), ((67, 35), 1), ((67, 35), 0)])
def test_2d_compute_P_matches_the_restatement(jr, ni, batch, thermal, ghosted):
    from justrelax_jl_amd import _lib
    h = _lib.default_handle()
    p = Problem(jr, ni, 0.3, Q=True)
    try:
        h.set_option("fused2d_batch", batch)
        _compute_P_case(jr, p, thermal, ghosted)
    finally:
        h.set_option("fused2d_batch", 1)


@pytest.mark.parametrize("thermal,ghosted", [(False, 0), (True, 0), (True, 1)])
@pytest.mark.parametrize("ni,prekz", [((13, 9, 7), 1), ((70, 5, 6), 4), ((20, 12, 10), 0)])
def test_3d_compute_P_matches_the_restatement(jr, ni, prekz, thermal, ghosted):
    from justrelax_jl_amd import _lib
    h = _lib.default_handle()
    p = Problem(jr, ni, 0.3, Q=True)
    try:
        h.set_option("vep3_prekz", prekz)
        _compute_P_case(jr, p, thermal, ghosted)
    finally:
        h.set_option("vep3_prekz", 0)


@pytest.mark.parametrize("ni", [(8, 7), (8, 7, 6)])
def test_uniformly_heated_closed_box_builds_the_thermal_pressure(jr, ni):
    """closed free-slip box, one elastic material, ρg = 0, V = 0, ΔT = δ everywhere: V stays exactly zero and P -> P_initial + Kb α δ.  At ∇V = 0,
    RP = -(P - P0) / (Kb dt) + α δ / dt, so |P - P0 - Kb α δ| = Kb dt |RP| for the pressure RP was taken at, and the update that follows only moves P closer."""
    import torch
    from justrelax_jl_amd.arrays import fzeros
    δ, P_init, eps_abs = 0.7, 0.3, 1.0e-11
    p = Problem(jr, ni, 0.25, nph=1, plastic=False)
    Kb, α = p.phases[0]["Kb"], p.phases[0]["density"]["alpha"]
    for k in p.a:
        if not k.startswith("phase") and k not in ("eta", "eta_v"):
            p.a[k][...] = 0.0
    p.a["eta"][...] = 1.0
    p.a["P"][...] = P_init
    p.pt.ϵ_rel, p.pt.ϵ_abs = 0.0, eps_abs
    dT = fzeros(p.ni, torch.device("cuda", torch.cuda.current_device()), δ)
    kw = dict(iterMin=1) if p.nd == 2 else {}
    r, out = p.solve(p.rheology(update_rho=False), dict(ΔT=dT), iterMax=20000, nout=50, **kw)
    assert r.iter < 20000 and r.err_evo1[-1] < eps_abs
    for k in ("Vx", "Vy", "Vz")[:p.nd]:
        assert not out[k].any(), k
    n = float(np.prod(ni))
    nRP = np.sqrt(np.sum(out["RP"] ** 2)) / (np.sqrt(n) if p.nd == 2 else n)
    print(f"norm(RP) = {nRP:.3e}, max|RP| = {np.abs(out['RP']).max():.3e}, max|P - P0 - Kb α δ| = {np.abs(out['P'] - P_init - Kb * α * δ).max():.3e}")
    assert nRP < eps_abs
    bound = Kb * p.dt * np.abs(out["RP"]).max() + 8 * np.spacing(Kb * α * δ)
    assert np.abs(out["P"] - P_init - Kb * α * δ).max() <= bound
    assert np.abs(out["P"] - P_init).min() > 0.5 * Kb * α * δ


@pytest.mark.parametrize("ni", [(9, 7), (9, 7, 5)])
def test_zero_dT_and_zero_alpha_are_no_ops_and_melt_fraction_is_refused(jr, ni):
    import torch
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.arrays import fzeros
    p = Problem(jr, ni, 0.25, Q=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    kw = dict(iterMax=5, nout=3, **(dict(iterMin=1) if p.nd == 2 else {}))
    rh = p.rheology(update_rho=False)
    r0, base = p.solve(rh, None, **kw)
    r1, zero = p.solve(rh, dict(ΔT=fzeros(ni, dev)), **kw)
    for ph in p.phases:
        ph["density"]["alpha"] = 0.0
    r2, noα = p.solve(p.rheology(update_rho=False), dict(ΔT=p.dT_dev(1)), **kw)
    r3, melt = p.solve(rh, dict(melt_fraction=fzeros(ni, dev, 0.3)), **kw)          # without ΔT a no-op, as in the reference
    for r, out in ((r1, zero), (r2, noα), (r3, melt)):
        assert np.array_equal(np.asarray(r.err_evo1), np.asarray(r0.err_evo1))
        for k in base:
            assert np.array_equal(out[k], base[k]), k
    # ΔT with melt_fraction: status 4, named, nothing launched (the solve's first act is the copy P0 <- P)
    st, pr, ρg = p.upload()
    before = p.download(st)
    assert (before["P0"] != before["P"]).any()
    with pytest.raises(_lib.JrxError, match="melt_fraction") as e:
        jr.solve_(st, p.pt, p.grid, p.bcs, ρg, pr, rh, dict(ΔT=p.dT_dev(0), melt_fraction=fzeros(ni, dev, 0.3)), p.dt, None, kwargs=dict(verbose=False, **kw))
    assert e.value.status == 4
    after = p.download(st)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    for bad in (tuple(n + 1 for n in ni), ni[::-1]):
        with pytest.raises(ValueError, match="ΔT"):
            jr.solve_(st, p.pt, p.grid, p.bcs, ρg, pr, rh, dict(ΔT=fzeros(bad, dev)), p.dt, None, kwargs=dict(verbose=False, **kw))


def test_drivers_without_the_term_do_not_read_dT(jr):
    """the single-phase 2D driver (compute_P! gets no args, Stokes2D.jl:420) and both variational drivers (their ΔT methods are commented out in the reference)"""
    p = Problem(jr, (9, 7), 0.25, Q=True)
    kw = dict(verbose=False, iterMax=5, nout=3)
    outs = []
    for args in (None, dict(ΔT=p.dT_dev(0))):
        st, pr, ρg = p.upload()
        r = jr.solve_(st, p.pt, p.grid, p.bcs, ρg, dict(p.phases[0]), args, p.dt, None, kwargs=kw)
        outs.append((np.asarray(r.err_evo1), p.download(st)))
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k
    for ni in ((9, 7), (9, 7, 5)):
        p = Problem(jr, ni, 0.25, Q=True)
        outs = []
        for args in (None, dict(ΔT=p.dT_dev(1))):
            st, pr, ρg = p.upload()
            ϕ = jr.RockRatio(jr.AMDGPUBackend, *ni)
            jr.update_rock_ratio_(ϕ, pr, 0)
            r = jr.solve_VariationalStokes_(st, p.pt, p.grid, p.bcs, ρg, pr, ϕ, p.phases, args, p.dt, None,
                                            kwargs=dict(kw, viscosity_cutoff=(1.0e-2, 1.0e2), **(dict(iterMin=1) if len(ni) == 2 else {})))
            outs.append((np.asarray(r.err_evo1), p.download(st)))
        assert np.array_equal(outs[0][0], outs[1][0])
        for k in outs[0][1]:
            assert np.array_equal(outs[0][1][k], outs[1][1][k]), k
