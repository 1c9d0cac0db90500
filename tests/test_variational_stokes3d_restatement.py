"""CPU tests that pin the NumPy restatement of the 3D variational Stokes solver (tests/_variational_stokes3d.py) to things that are not the HIP code: the C
oracle's unmasked 3D functions for ϕ ≡ 1, the 2D masked restatement (itself pinned to the reference's tests) for states that are uniform along one axis, the
all-air state, and the predicates' scalar definitions."""
import ctypes as C

import numpy as np
import pytest

import _variational_stokes as vs2
import _variational_stokes3d as vs

MEMBERS = ("center", "vertex", "Vx", "Vy", "Vz", "yz", "xz", "xy")


def _ones_phi(ni):
    p = vs.rock_ratio(*ni)
    for k in MEMBERS:
        p[k][...] = 1.0
    return p


def _oracle_params(orc, s, **over):
    pt, b = s.pt, s.flow_bcs
    kw = dict(iterMax=s.kwargs["iterMax"], nout=s.kwargs["nout"])
    kw.update(over)
    return orc.vep_params3d(s.ni, s.grid._di["center"], s.dt, dict(r=pt.r, theta_dtau=pt.θ_dτ, eta_dtau=pt.ηdτ, eps_rel=pt.ϵ_rel, eps_abs=pt.ϵ_abs),
                            free_slip=b.free_slip, no_slip=b.no_slip, periodic=b.periodic, **kw)


def test_mask_arrays_are_the_scalar_predicates():
    """the vectorised predicates against the scalar ones (mask.jl:180-186,220-269,324-392), node by node, on a grid with three different extents"""
    ni = (5, 4, 3)
    phi = vs.random_phi3(ni, seed=2)
    m = vs.valid_masks(phi)
    for name, fn in (("c", vs.isvalid_c), ("yz", vs.isvalid_yz), ("xz", vs.isvalid_xz), ("xy", vs.isvalid_xy), ("vx", vs.isvalid_vx), ("vy", vs.isvalid_vy),
                     ("vz", vs.isvalid_vz)):
        assert m[name].any() and not m[name].all(), name
        for I in np.ndindex(*m[name].shape):
            assert m[name][I] == fn(phi, *I), (name, I)


@pytest.mark.parametrize("ni", [(7, 6, 5), (10, 8, 7), (17, 19, 23), (65, 9, 5)])
def test_random_phi3_exercises_every_predicate(ni):
    """every predicate true on 20-80 % of its nodes, fractional values in every member (measured shares with this recipe: 0.43-0.74)"""
    phi = vs.random_phi3(ni, seed=8)
    m = vs.valid_masks(phi)
    for k in ("c", "yz", "xz", "xy", "vx", "vy", "vz"):
        assert 0.2 <= m[k].mean() <= 0.8, (k, m[k].mean())
    for k in MEMBERS:
        assert ((phi[k] > 0) & (phi[k] < 1)).any() and (phi[k] == 0).any() and (phi[k] == 1).any(), k


# measured on the CPU (printed by the tests below; max |a - b| / max |b| per field): NumPy's unfused multiply-adds, and for the momentum kernel the order of the
# terms of Ry and Rz (τ normal first here, as the reference's masked 3D text has it; τxy / τxz first in the unmasked kernel)
STRESS_MEASURED = 4.3e-16
KERNEL_MEASURED = 1.9e-16
SOLVE_MEASURED = 4.2e-15


def test_phi_one_stress_kernel_equals_the_oracle(jr, oracle):
    """ϕ ≡ 1: the restated update_stresses_center_vertex! 3D against orc_vep3d_stress on the randomised shearband3d state (yielding and elastic nodes, mixed
    ratios, dilatant plasticity with a finite bulk modulus).  Largest relative difference measured: 4.3e-16 (ε_pl.yz; max |a - b| / max |b| per field); bound 10 x that."""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband3d((13, 9, 7))
    phases = vs.randomize(s)
    rng = np.random.default_rng(9)
    theta = np.asfortranarray(rng.uniform(-1, 1, size=s.ni))
    lam = np.asfortranarray(rng.uniform(0, 0.1, size=s.ni))
    lamv = [np.asfortranarray(rng.uniform(0, 0.1, size=s.arrays[k].shape)) for k in ("tyz", "txz", "txy")]
    ref = {k: v.copy(order="F") for k, v in s.arrays.items()}
    lam_r, lamv_r = lam.copy(order="F"), [x.copy(order="F") for x in lamv]
    oracle.vep3d_stress(ref, theta, lam_r, lamv_r, oracle.rheology_struct(phases), _oracle_params(oracle, s))
    a = s.arrays
    yld = vs.update_stresses(a, _ones_phi(s.ni), theta, lam, lamv, phases, s.dt, s.pt.θ_dτ, 0.2)
    worst = {}
    for k in ("txx", "tyy", "tzz", "tyz", "txz", "txy", "tyz_c", "txz_c", "txy_c", "tII", "eta_vep", "P", "eplxx", "eplyy", "eplzz", "eplyz", "eplxz", "eplxy",
              "evol_pl"):
        worst[k] = max_rel_diff(a[k], ref[k])
    worst["lam"] = max_rel_diff(lam, lam_r)
    for k, x, y in zip(("lamv_yz", "lamv_xz", "lamv_xy"), lamv, lamv_r):
        worst[k] = max_rel_diff(x, y)
    print("stress kernel 3D, phi = 1, restatement vs oracle: max rel diff", max(worst.values()), worst)
    assert all(y.any() and not y.all() for y in yld.values())
    assert max(worst.values()) <= 10 * STRESS_MEASURED <= 1e-10, worst


def test_phi_one_kernels_equal_the_unmasked_oracle(jr, oracle):
    """ϕ ≡ 1: the restated ∇V / strain rates against orc_compute_divV3d + orc_compute_strain_rate3d, and the restated momentum kernel against orc_compute_V3d, on
    random fields.  Largest relative difference measured: 1.9e-16 (Vz; R.Rz 1.5e-16 -- its three stress terms are summed in another order; ∇V, ε, Rx, Ry, Vx, Vy agree to the bit); bound 10 x that."""
    from justrelax_jl_amd.checks import max_rel_diff
    ni = (13, 9, 7)
    s = jr.miniapps.shearband3d(ni)
    vs.randomize(s)
    rng = np.random.default_rng(12)
    a = s.arrays
    for k in ("Vx", "Vy", "Vz", "fx", "fy", "fz"):
        a[k][...] = rng.uniform(-1.0, 1.0, size=a[k].shape)
    etatau = np.asfortranarray(10.0 ** rng.uniform(-1, 0.5, size=ni))
    ref = {k: v.copy(order="F") for k, v in a.items()}
    _di = s.grid._di["center"]
    pt = s.pt
    p = oracle.params3d(ni, _di, s.dt, dict(r=pt.r, theta_dtau=pt.θ_dτ, eta_dtau=pt.ηdτ, eps_rel=pt.ϵ_rel, eps_abs=pt.ϵ_abs))
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    oracle.lib().orc_compute_divV3d(dp(ref["divV"]), dp(ref["Vx"]), dp(ref["Vy"]), dp(ref["Vz"]), *[C.c_int64(n) for n in ni], *[C.c_double(d) for d in _di])
    oracle.call3d("orc_compute_strain_rate3d", ref, p)
    oracle.call3d("orc_compute_V3d", ref, p, dp(etatau))
    phi = _ones_phi(ni)
    vs.compute_divV_strain(a, phi, _di)
    vs.compute_V(a, phi, etatau, pt.ηdτ, _di)
    worst = {k: max_rel_diff(a[k], ref[k]) for k in ("divV", "exx", "eyy", "ezz", "eyz", "exz", "exy", "Rx", "Ry", "Rz", "Vx", "Vy", "Vz")}
    print("kernels 3D, phi = 1, restatement vs oracle:", max(worst.values()), {k: v for k, v in worst.items() if v > 0})
    assert max(worst.values()) <= 10 * KERNEL_MEASURED <= 1e-10, worst


def test_phi_one_driver_iterations_equal_the_oracle(jr, oracle):
    """ϕ ≡ 1, air_phase = 0: 20 iterations of the restated _solve_VS! 3D against orc_stokes3d_vep_solve on a pre-stressed, yielding shearband3d state.  Both
    reference drivers run compute_viscosity! on entry and update_viscosity_τII! before the stress update, and both take R from compute_V!.  Structural
    differences, none of them widened for:
      * the norms of R: _solve_VS! divides by sqrt((nx_g-1)(ny_g-1)(nz_g-1)) (Stokes3D.jl:178), the unmasked driver by the product itself -- compared after
        multiplying the oracle's by sqrt of the product; norm_∇V is the same expression in both;
      * err and err_evo1, the maximum over differently scaled norms, are not compared (ϵ = 1e-30 keeps both loops running to iterMax + 1).
    Largest relative difference measured over the fields and norms: 4.2e-15; bound 10 x that."""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband3d_variational((10, 8, 7), iterMax=19, nout=5)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    rng = np.random.default_rng(3)
    a = s.arrays
    for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):     # pre-stress close to yield so that plasticity is active
        a["to" + c][...] = rng.uniform(-1.5, 1.5, size=a["to" + c].shape)
        a["t" + c][...] = a["to" + c]
    ref = {k: v.copy(order="F") for k, v in a.items()}
    r_ref = oracle.stokes3d_vep_solve(ref, oracle.rheology_struct(s.extra["phases"]), _oracle_params(oracle, s))
    kw = {k: v for k, v in s.kwargs.items() if k != "verbose"}
    r = vs.solve_VS(a, _ones_phi(s.ni), s.extra["phases"], vs.pt_tuple(s.pt), s.grid._di["center"], s.dt, **kw)
    assert r["iter"] == r_ref["iter"] == 20 and r["err_evo2"] == list(r_ref["err_evo2"]) == [5, 10, 15, 20]
    worst = {}
    for k in ref:
        if k.startswith("phase_") or ref[k] is None:
            continue
        worst[k] = max_rel_diff(a[k], ref[k])
    nx, ny, nz = s.ni
    scale = np.sqrt((nx - 1) * (ny - 1) * (nz - 1))
    for k in ("norm_Rx", "norm_Ry", "norm_Rz"):
        worst[k] = max_rel_diff(np.array(r[k]), np.array(r_ref[k]) * scale)
    worst["norm_divV"] = max_rel_diff(np.array(r["norm_divV"]), np.array(r_ref["norm_divV"]))
    print("driver 3D, phi = 1, restatement vs oracle:", max(worst.values()), {k: v for k, v in worst.items() if v > 0})
    assert (a["eplxx"] != 0).any() and (a["eplxz"] != 0).any()
    assert max(worst.values()) <= 10 * SOLVE_MEASURED <= 1e-10, worst


def _extrude(jr, a2, phi2, ni2, axis, nu=3):
    """a 2D state and its 2D ϕ as a 3D one that is uniform along `axis` (the construction of miniapps.plane_strain3d): the 2D x and y take the two remaining 3D
    axes in order and the 2D components are renamed with them; the velocity and every stress component along `axis` are zero.  ϕ: the edge member normal to the
    axis carries the 2D `vertex`, the velocity members of the two in-plane axes the 2D Vx, Vy; everything that only meets out-of-plane quantities is 1"""
    u = axis
    p, q = [d for d in range(3) if d != u]
    ni = [0, 0, 0]
    ni[p], ni[q], ni[u] = ni2[0], ni2[1], nu
    ni = tuple(ni)
    c = "xyz"
    shear = {(1, 2): "yz", (0, 2): "xz", (0, 1): "xy"}[(p, q)]
    a = {k: np.zeros(shp, order="F") for k, shp in jr.miniapps.vep_shapes3d(ni).items()}
    put = lambda k3, A2: a[k3].__setitem__(Ellipsis, np.expand_dims(A2, u))
    put("P", a2["P"])
    put("t" + c[p] * 2, a2["txx"]); put("t" + c[q] * 2, a2["tyy"]); put("t" + shear, a2["txy"])
    put("V" + c[p], a2["Vx"]); put("V" + c[q], a2["Vy"])
    put("f" + c[p], a2["fx"]); put("f" + c[q], a2["fy"])
    phi = _ones_phi(ni)
    for k3, k2 in (("center", "center"), ("vertex", "vertex"), (shear, "vertex"), ("V" + c[p], "Vx"), ("V" + c[q], "Vy")):
        phi[k3][...] = np.expand_dims(phi2[k2], u)
    names = dict(Vx="V" + c[p], Vy="V" + c[q], Rx="R" + c[p], Ry="R" + c[q], exy="e" + shear, divV="divV")
    return ni, a, phi, names, dict(V="V" + c[u], R="R" + c[u], e=[v for v in ("yz", "xz", "xy") if v != shear])


@pytest.mark.parametrize("axis", [2, 1, 0])
def test_plane_strain_reproduces_the_masked_2d_kernels(jr, axis):
    """A randomised 2D state with a random 2D ϕ (zeros, ones, fractions), extruded along `axis`: the restated 3D ∇V, shear strain rates and momentum kernel
    reproduce the 2D masked restatement (tests/_variational_stokes.py, free_surface off) on every plane to 1e-13 -- the two sum the same terms in a different
    order -- and the out-of-plane residual, velocity and shear strain rates stay exactly zero.  This pins the hand-written 3D momentum form to the reference's
    working 2D kernel: each orientation puts the 2D shear stress on another edge family and the 2D velocity members on another pair of 3D ones."""
    from justrelax_jl_amd.checks import max_rel_diff
    s2 = jr.miniapps.shearband2d_variational(12)
    vs2.randomize(s2, 5)
    rng = np.random.default_rng(21)
    a2 = s2.arrays
    for k in ("Vx", "Vy", "fx", "fy"):
        a2[k][...] = rng.uniform(-1.0, 1.0, size=a2[k].shape)
    phi2 = vs2.random_phi(s2.ni, 5)
    m2 = vs2.valid_masks(phi2)
    assert all(0.2 <= m2[k].mean() <= 0.8 for k in m2)
    et2 = np.asfortranarray(10.0 ** rng.uniform(-1, 0.5, size=s2.ni))
    ni, a, phi, names, out = _extrude(jr, a2, phi2, s2.ni, axis)
    _di2 = s2.grid._di["center"]
    p, q = [d for d in range(3) if d != axis]
    _di = [0.0] * 3
    _di[p], _di[q], _di[axis] = _di2[0], _di2[1], 7.0
    et = np.asfortranarray(np.broadcast_to(np.expand_dims(et2, axis), ni))
    vs.compute_divV_strain(a, phi, _di)
    vs.compute_V(a, phi, et, s2.pt.ηdτ, _di)
    vs2.compute_divV_strain(a2, phi2, _di2)
    vs2.compute_V(a2, phi2, et2, s2.pt.ηdτ, _di2, 0.0)
    for k2 in ("divV", "exy", "Rx", "Ry", "Vx", "Vy"):
        A3 = np.moveaxis(a[names[k2]], axis, 0)
        if k2 in ("Vx", "Vy"):
            A3 = A3[1:-1]          # the two ghost planes along the axis are not the kernel's to write
        assert (a2[k2] != 0).any() and len(A3) == 3
        for plane in A3:
            assert max_rel_diff(plane, a2[k2]) <= 1e-13, (k2, axis)
    assert not a[out["R"]].any() and not a[out["V"]].any() and not a["e" + out["e"][0]].any() and not a["e" + out["e"][1]].any()


def test_all_air_leaves_everything_zero(jr):
    """ϕ ≡ 0: one solve leaves the interior of V and every residual exactly zero and returns err = 0 at the first check, where the loop stops (0 / 0 is not > ϵ)"""
    s = jr.miniapps.shearband3d_variational((8, 7, 6), iterMax=50, nout=10)
    a = s.arrays
    kw = {k: v for k, v in s.kwargs.items() if k != "verbose"}
    r = vs.solve_VS(a, vs.rock_ratio(*s.ni), s.extra["phases"], vs.pt_tuple(s.pt), s.grid._di["center"], s.dt, **kw)
    assert r["err_evo1"] == [0.0] and r["iter"] == 10
    for k in ("Vx", "Vy", "Vz"):
        assert not a[k][1:-1, 1:-1, 1:-1].any(), k
    for k in ("Rx", "Ry", "Rz", "RP", "txx", "tzz", "tyz", "txz", "txy", "P"):
        assert not a[k].any(), k
