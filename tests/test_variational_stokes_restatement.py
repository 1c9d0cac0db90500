"""CPU tests that pin the NumPy restatement of the variational Stokes solver (tests/_variational_stokes.py) to things that are not the HIP code: the
numeric assertions of the reference's test/test_rockratio.jl (those that need no JustPIC internals), the correct_phase_ratio cases, the C oracle's unmasked
2D multiphase functions for ϕ ≡ 1, and the all-air state of test/test_Volcano2D.jl."""
import ctypes as C

import numpy as np
import pytest

import _variational_stokes as vs


def test_rockratio_constructor_shapes():
    """test_rockratio.jl:35-78"""
    nx, ny = 5, 4
    p = vs.rock_ratio(nx, ny)
    assert p["center"].shape == (nx, ny) and p["vertex"].shape == (nx + 1, ny + 1) and p["Vx"].shape == (nx + 1, ny) and p["Vy"].shape == (nx, ny + 1)
    assert all(p[k].shape == (1, 1) for k in ("Vz", "yz", "xz", "xy"))
    assert not p["center"].any() and not p["vertex"].any()
    nx, ny, nz = 4, 3, 2
    p = vs.rock_ratio(nx, ny, nz)
    want = dict(center=(nx, ny, nz), vertex=(nx + 1, ny + 1, nz + 1), Vx=(nx + 1, ny, nz), Vy=(nx, ny + 1, nz), Vz=(nx, ny, nz + 1),
                yz=(nx, ny + 1, nz + 1), xz=(nx + 1, ny, nz + 1), xy=(nx + 1, ny + 1, nz))
    assert {k: v.shape for k, v in p.items()} == want
    with pytest.raises(TypeError):
        vs.rock_ratio(10.0, 10.0)           # test_types.jl:306-307


def test_isvalid_cases():
    """test_rockratio.jl:80-105 (1-based there)"""
    p = vs.rock_ratio(4, 4)
    assert vs.isvalid(p["center"], 0, 0) is False
    p["center"][1, 1] = 0.5
    assert vs.isvalid(p["center"], 1, 1) and not vs.isvalid(p["center"], 0, 0)
    p["Vx"][2, 0] = 0.4
    assert vs.isvalid_vx(p, 2, 0) and not vs.isvalid_vx(p, 0, 0)
    p["Vy"][0, 2] = 0.6
    assert vs.isvalid_vy(p, 0, 2) and not vs.isvalid_vy(p, 0, 0)
    p["vertex"][1, 1] = 0.3
    p["Vx"][1, 0] = 0.1; p["Vx"][1, 1] = 0.1
    p["Vy"][0, 1] = 0.1; p["Vy"][1, 1] = 0.1
    assert vs.isvalid_v(p, 1, 1)
    m = vs.valid_masks(p)
    for i in range(5):
        for j in range(5):
            assert m["v"][i, j] == vs.isvalid_v(p, i, j)
            if i < 4 and j < 4:
                assert m["c"][i, j] == vs.isvalid_c(p, i, j)


def test_masked_minikernel_identities():
    """test_rockratio.jl:146-205"""
    A = np.arange(1.0, 17.0).reshape(4, 4, order="F")
    p = np.full((4, 4), 0.5)
    i = j = 1           # (2, 2) of the reference
    assert vs.center(A, p, i, j) == A[1, 1] * 0.5 and vs.right(A, p, i, j) == A[2, 1] * 0.5 and vs.left(A, p, i, j) == A[0, 1] * 0.5
    assert vs.front(A, p, i, j) == A[1, 2] * 0.5 and vs.back(A, p, i, j) == A[1, 0] * 0.5 and vs.next_(A, p, i, j) == A[2, 2] * 0.5
    assert vs.d_xa(A, p, 1.0, i, j) == pytest.approx(-A[1, 1] * 0.5 + A[2, 1] * 0.5)
    assert vs.d_ya(A, p, 1.0, i, j) == pytest.approx(-A[1, 1] * 0.5 + A[1, 2] * 0.5)
    assert vs.d_xi(A, p, 1.0, i, j) == pytest.approx(-A[1, 2] * 0.5 + A[2, 2] * 0.5)
    assert vs.d_yi(A, p, 1.0, i, j) == pytest.approx(-A[2, 1] * 0.5 + A[2, 2] * 0.5)
    assert vs.d_xa(A, p, 2.0, i, j) == pytest.approx(2.0 * (-A[1, 1] * 0.5 + A[2, 1] * 0.5))
    assert vs.av_xa(A, p, i, j) == pytest.approx(0.5 * (A[1, 1] + A[2, 1]) * 0.5)
    assert vs.av_ya(A, p, i, j) == pytest.approx(0.5 * (A[1, 1] + A[1, 2]) * 0.5)
    assert vs.mymaskedsum(A, p, range(1, 3), range(1, 3)) == pytest.approx(sum(A[a, b] * 0.5 for a in (1, 2) for b in (1, 2)))
    v, m = np.arange(1.0, 6.0), np.full(5, 0.25)
    assert vs.mymaskedsum(v, m, range(1, 4)) == pytest.approx(sum(v[k] * m[k] for k in range(1, 4)))
    A3, p3 = np.arange(1.0, 65.0).reshape(4, 4, 4, order="F"), np.full((4, 4, 4), 0.5)
    assert vs.mymaskedsum(A3, p3, range(1, 3), range(1, 3), range(1, 3)) == pytest.approx(0.5 * A3[1:3, 1:3, 1:3].sum())
    assert vs.mymaskedsum(A, p, range(1, 3), range(1, 3), f=lambda x: 1.0 / x) == pytest.approx(sum(0.5 / A[a, b] for a in (1, 2) for b in (1, 2)))
    assert vs.av(A, p, 0, 0) == pytest.approx(0.25 * sum(A[a, b] * 0.5 for a in (1, 2) for b in (1, 2)))
    assert vs.av_a(A, p, 0, 0) == pytest.approx(0.25 * sum(A[a, b] * 0.5 for a in (0, 1) for b in (0, 1)))
    assert vs.av_xi(A, p, 0, 0) == pytest.approx(0.5 * (A[0, 1] * 0.5 + A[1, 1] * 0.5))
    assert vs.av_yi(A, p, 0, 0) == pytest.approx(0.5 * (A[1, 0] * 0.5 + A[1, 1] * 0.5))


def _half_rock_half_air(nx=4, ny=4):
    shapes = dict(center=(nx, ny), vertex=(nx + 1, ny + 1), Vx=(nx + 1, ny), Vy=(nx, ny + 1))
    pr = {}
    for k, s in shapes.items():
        r = np.zeros((2,) + s, order="F")
        h = s[0] // 2
        r[0, :h], r[1, h:] = 1.0, 1.0
        pr[k] = r
    return pr


def test_compute_rock_ratio_and_update():
    """test_rockratio.jl:111-143,230-252"""
    pr = _half_rock_half_air()
    assert vs.compute_rock_ratio(pr["center"], 2)[0, 0] == 1.0 and vs.compute_rock_ratio(pr["center"], 2)[3, 0] == 0.0
    assert (vs.compute_rock_ratio(pr["center"], 0) == 1.0).all() and (vs.compute_rock_ratio(pr["center"], 99) == 1.0).all()
    p = vs.rock_ratio(4, 4)
    vs.update_rock_ratio(p, pr, 2)
    c = p["center"]
    assert c[0, 0] == 1.0 and c[1, 1] == 1.0 and c[2, 0] == 0.0 and c[3, 1] == 0.0
    assert c.sum() == pytest.approx(4 * 4 / 2)
    # the threshold and the clamp asymmetry (mask.jl:117,155): a ratio within 1e-5 of 1 gives 0; a ratio above 1 leaves a negative difference, which is not > 1e-5
    r = np.zeros((2, 2, 1))
    r[1, :, 0] = (1.0 - 5.0e-6, 0.25)
    assert vs.compute_rock_ratio(r, 2)[0, 0] == 0.0 and vs.compute_rock_ratio(r, 2)[1, 0] == 0.75


def test_correct_phase_ratio_cases():
    """rheology/Viscosity.jl:638-650"""
    r = np.array([0.2, 0.3, 0.5])
    assert np.array_equal(vs.correct_phase_ratio(0, r), r)
    assert np.array_equal(vs.correct_phase_ratio(3, np.array([0.0, 0.0, 1.0])), np.zeros(3))
    assert np.array_equal(vs.correct_phase_ratio(3, np.array([0.0, 1.0e-9, 1.0 - 1.0e-9])), np.zeros(3))        # ≈ 1
    c = vs.correct_phase_ratio(3, r)
    assert c[2] == 0.0 and c[0] == 0.2 / 0.5 and c[1] == 0.3 / 0.5 and c.sum() == pytest.approx(1.0)
    allr = np.stack([r, [0.0, 0.0, 1.0]], axis=1)
    got = vs._correct_all(allr, 3)
    assert np.array_equal(got[:, 0], c) and np.array_equal(got[:, 1], np.zeros(3))


def _ones_phi(ni):
    p = vs.rock_ratio(*ni)
    for k in ("center", "vertex", "Vx", "Vy"):
        p[k][...] = 1.0
    return p


def _oracle_params(orc, s, **over):
    pt, b = s.pt, s.flow_bcs
    kw = dict(iterMax=s.kwargs["iterMax"], nout=s.kwargs["nout"], stag_mode=1)
    kw.update(over)
    return orc.vep_params2d(s.ni, s.grid._di["center"], s.dt, dict(r=pt.r, theta_dtau=pt.θ_dτ, eta_dtau=pt.ηdτ, eps_rel=pt.ϵ_rel, eps_abs=pt.ϵ_abs),
                            free_slip=b.free_slip, no_slip=b.no_slip, periodic=b.periodic, **kw)


# measured on the CPU (printed by the tests below): the masked arithmetic with ϕ ≡ 1 against the C oracle differs by NumPy's unfused multiply-adds only
STRESS_MEASURED = 5.3e-16
SOLVE_MEASURED = 3.3e-15


def test_phi_one_stress_kernel_equals_the_oracle(jr, oracle):
    """ϕ ≡ 1: the restated update_stresses_center_vertex! against orc_vep2d_stress on the randomised shear-band state.  Largest relative difference
    measured: 5.3e-16 (max |a - b| / max |b| per field); bound 10 x that."""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband2d_variational(24)
    vs.randomize(s)
    rng = np.random.default_rng(9)
    theta = np.asfortranarray(rng.uniform(-1, 1, size=s.ni))
    lam = np.asfortranarray(rng.uniform(0, 0.1, size=s.ni))
    lamv = np.asfortranarray(rng.uniform(0, 0.1, size=(s.ni[0] + 1, s.ni[1] + 1)))
    ref = {k: v.copy(order="F") for k, v in s.arrays.items()}
    lam_r, lamv_r = lam.copy(order="F"), lamv.copy(order="F")
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    f = oracle.vep2d(ref)
    oracle.lib().orc_vep2d_stress(C.byref(f), dp(theta), dp(lam_r), dp(lamv_r), C.byref(oracle.rheology_struct(s.extra["phases"])), C.byref(_oracle_params(oracle, s)))
    a = s.arrays
    vs.update_stresses(a, _ones_phi(s.ni), theta, lam, lamv, s.extra["phases"], s.dt, s.pt.θ_dτ, 0.2)
    worst = 0.0
    for k in ("txx", "tyy", "txy", "txy_c", "tII", "eta_vep", "P", "eplxx", "eplyy", "eplxy", "evol_pl"):
        worst = max(worst, max_rel_diff(a[k], ref[k]))
    worst = max(worst, max_rel_diff(lam, lam_r), max_rel_diff(lamv, lamv_r))
    print("stress kernel, phi = 1, restatement vs oracle: max rel diff", worst)
    assert (lam_r != 0).any() and (ref["eplxy"] != 0).any() and (ref["eplxy"] == 0).any()
    assert worst <= 10 * STRESS_MEASURED <= 1e-10


def test_phi_one_driver_iterations_equal_the_oracle(jr, oracle):
    """ϕ ≡ 1, air_phase = 0: 40 iterations of the restated _solve_VS! on the randomised shear-band state against orc_stokes2d_vep_solve.
    Structural differences between the two reference drivers, none of them widened for:
      * _solve_VS! runs compute_viscosity! (relaxation 1) on entry (Stokes2D.jl:102); the oracle's state gets the same call before its solve.  The phases are
        LinearViscous with η = 1, a fixed point of the relaxed update, so that the place of update_viscosity_τII! in the iteration (before the stress update
        there, after it in the unmasked driver) changes nothing.
      * compute_strain_rate! divides ∇V by 3 (VelocityKernels.jl:44) where the unmasked kernel multiplies by inv(3): ε.xx, ε.yy differ in the last bit, and
        everything downstream with them.  This is the measured difference.
      * R.Rx, R.Ry and the norm history are not compared: _solve_VS! takes them from compute_V! (the residual before the velocity update), the unmasked driver
        from compute_Res! at each check (after it).
    Largest relative difference measured over the other fields: 3.3e-15 (η_vep; RP 2.8e-15, ∇V 1.6e-15, the rest below 1.1e-15); bound 10 x that."""
    from justrelax_jl_amd.checks import max_rel_diff
    s = jr.miniapps.shearband2d_variational(24, iterMax=39, nout=10)
    vs.randomize(s)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    rh = oracle.rheology_struct(s.extra["phases"])
    ref = {k: v.copy(order="F") for k, v in s.arrays.items()}
    p = _oracle_params(oracle, s, iterMin=10)
    oracle.compute_viscosity2d(ref, rh, p, nu=1.0, tau=False)
    r_ref = oracle.stokes2d_vep_solve(ref, rh, p)
    a = s.arrays
    kw = {k: v for k, v in s.kwargs.items() if k not in ("verbose",)}
    r = vs.solve_VS(a, _ones_phi(s.ni), s.extra["phases"], vs.pt_tuple(s.pt), s.grid._di["center"], s.dt, iterMin=10, **kw)
    assert r["iter"] == r_ref["iter"] == 40
    worst = {}
    for k in ref:
        if k in ("Rx", "Ry", "phase_vx", "phase_vy") or ref[k] is None:
            continue
        worst[k] = max_rel_diff(a[k], ref[k])
    print("driver, phi = 1, restatement vs oracle:", max(worst.values()), {k: v for k, v in worst.items() if v > 0})
    assert (a["eplxx"] != 0).any()
    assert max(worst.values()) <= 10 * SOLVE_MEASURED <= 1e-10, worst


def test_all_air_leaves_everything_zero(jr):
    """ϕ ≡ 0 (what test/test_Volcano2D.jl effectively runs): one solve leaves the interior of V and every residual exactly zero and returns err = 0
    at the first check"""
    s = jr.miniapps.shearband2d_variational(16, iterMax=50, nout=10)
    s.kwargs.update(iterMin=5)
    a = s.arrays
    kw = {k: v for k, v in s.kwargs.items() if k not in ("verbose",)}
    r = vs.solve_VS(a, vs.rock_ratio(*s.ni), s.extra["phases"], vs.pt_tuple(s.pt), s.grid._di["center"], s.dt, **kw)
    assert r["err_evo1"][0] == 0.0 and r["iter"] == 10 and len(r["err_evo1"]) == 1
    assert not a["Vx"][1:-1, 1:-1].any() and not a["Vy"][1:-1, 1:-1].any()
    assert not a["Rx"].any() and not a["Ry"].any() and not a["RP"].any()
    assert not a["txx"].any() and not a["txy"].any() and not a["P"].any()
