"""The NumPy restatement of the 2D DYREL solver (tests/_dyrel.py) against the known answers of the reference's own kernel tests (test/test_dyrel_kernels.jl, at
its 6 x 5 grid), and the static side of the new interface: prototypes in include/jrx.h, methods in the Julia extension, INTEGRATION.md.  The GPU tests
(tests/test_gpu_dyrel.py) compare the HIP kernels with this restatement.

Not asserted here: the scalars test/test_shearband2D_DYREL.jl:212-216 pins after ten time steps of its 32 x 32 shear band.  They need ten full solves, and the
NumPy driver takes about 100 s for them (1.5 s a step while nothing yields, 10 to 35 s a step from step 7 on: 4,000 to 11,750 inner iterations each), beyond
the minute a test of this suite may take; no earlier step is pinned by the reference.  Run once by hand, dy.shearband_state(32, 32) stepped ten times
with the keywords of :164-187 gave max τxx = 1.638814244 after step 10 against the pinned 1.638803924349033 (atol 1e-4) and err_evo_tot[end] = 4.5e-7 (< 1e-6),
with 580 of the 1024 centres yielding; the native driver's ten steps are what examples/shearband2d_dyrel.py prints."""
import re

import numpy as np
import pytest

import _dyrel as dy
from _abi_parse import JULIA_EXT, ROOT, c_prototypes, c_structs

NX, NY = 6, 5


def _single_phase_state(dtype=np.float64):
    """test_dyrel_kernels.jl:101-135: one LinearViscous phase (η = 1, G = 1, Kb = 5), dt = 1, Vx = a x, Vy = b y on the unit square"""
    nx, ny = NX, NY
    c, v = (nx, ny), (nx + 1, ny + 1)
    a = {k: np.zeros(c, dtype=dtype, order="F") for k in ("P", "P0", "divV", "Q", "exx", "eyy", "exy_c", "eplxx", "eplyy", "eplxy_c", "txx", "tyy", "txy_c", "tII",
                                                             "toxx", "toyy", "toxy_c", "eta", "eta_vep", "EII_pl", "evol_pl", "EVol_pl", "fx", "fy", "RP")}
    a.update({k: np.zeros(v, dtype=dtype, order="F") for k in ("exy", "eplxy", "txy", "toxy", "eta_v", "omega_xy")})
    a.update(Vx=np.zeros((nx + 1, ny + 2), dtype=dtype, order="F"), Vy=np.zeros((nx + 2, ny + 1), dtype=dtype, order="F"),
             Rx=np.zeros((nx - 1, ny), dtype=dtype, order="F"), Ry=np.zeros((nx, ny - 1), dtype=dtype, order="F"),
             phase_c=np.ones((1, nx, ny), dtype=dtype, order="F"), phase_v=np.ones((1, nx + 1, ny + 1), dtype=dtype, order="F"))
    a.update(dy.extra_arrays((nx, ny), dtype))
    phases = [dict(eta=1.0, G=1.0, Kb=5.0, density=dict(kind="constant", rho0=1.0), g=1.0)]
    a["eta"][...] = 1.0
    a["eta_v"][...] = 1.0
    dy.compute_viscosity(a, phases, 1.0, (-np.inf, np.inf))
    av, bv = 1.3, -0.4
    xv, yv = np.linspace(0.0, 1.0, nx + 1), np.linspace(0.0, 1.0, ny + 1)
    a["Vx"][...] = (av * xv)[:, None]
    a["Vy"][...] = (bv * yv)[None, :]
    di = (1.0 / nx, 1.0 / ny)
    d = dy.new_dyrel((nx, ny), dtype)
    dy.dyrel_init(a, d, phases, di, 1.0)
    return a, d, phases, di, (av, bv)


def test_pure_helpers():
    """test_dyrel_kernels.jl:52-66"""
    P, P0, divV, Q, etab, dt = 3.0, 1.0, 0.5, 0.2, 4.0, 0.25
    assert dy.compute_RP(P, P0, divV, Q, etab, dt) == pytest.approx(-0.2, rel=1e-8)          # -0.5 - 2/4 + 0.2/0.25, worked by hand; Julia's ≈ is rtol = sqrt(eps)
    dVdtau, R, a, b, dtau = 2.0, 0.5, 0.9, 0.8, 0.3
    new, dV = dy.damped_update_V(dVdtau, R, a, b, dtau)
    assert new == pytest.approx(2.3, rel=1e-8)          # 0.9 * 2 + 0.5
    assert dV == pytest.approx(0.552, rel=1e-8)          # 2.3 * 0.8 * 0.3


def test_pure_strain_field():
    """test_dyrel_kernels.jl:74-94: Vx = a x, Vy = b y gives ∇V = a + b, εxx = a - (a + b)/3, εyy = b - (a + b)/3, εxy = 0"""
    a, d, phases, di, _ = _single_phase_state()
    av, bv = 2.0, -0.7
    xv, yv = np.linspace(0.0, 1.0, NX + 1), np.linspace(0.0, 1.0, NY + 1)
    a["Vx"][...] = (av * xv)[:, None]
    a["Vy"][...] = (bv * yv)[None, :]
    div = dy.strain_rate_RP(a, d, (1.0 / di[0], 1.0 / di[1]), 1.0)
    np.testing.assert_allclose(div, av + bv, rtol=1e-8)          # Julia's ≈: rtol = sqrt(eps)
    np.testing.assert_allclose(a["exx"], av - (av + bv) / 3, rtol=1e-8)
    np.testing.assert_allclose(a["eyy"], bv - (av + bv) / 3, rtol=1e-8)
    assert (np.abs(a["exy"]) < 1.0e-12).all()


def test_fused_kernels_known_answers():
    """test_dyrel_kernels.jl:101-192: RP = -(a + b) with P0 = P and Q = 0; η, ηv finite and positive after the non-linear branch (viscosity_relaxation = 1);
    θc = γ_eff RP + ΔPψ; finite PH residuals; velocities unchanged bit for bit with D = 1, β = 0"""
    a, d, phases, di, (av, bv) = _single_phase_state()
    _di = (1.0 / di[0], 1.0 / di[1])
    a["P0"][...] = a["P"]
    a["Q"][...] = 0.0
    dy.strain_rate_RP(a, d, _di, 1.0)
    np.testing.assert_allclose(a["RP"], -(av + bv), rtol=1e-8)
    np.testing.assert_allclose(a["exx"], av - (av + bv) / 3, rtol=1e-8)
    dy.stress_viscosity(a, d, phases, 1.0, 1.0, 1.0, (-np.inf, np.inf), False)
    assert np.isfinite(a["eta"]).all() and (a["eta"] > 0).all() and np.isfinite(a["eta_v"]).all()
    np.testing.assert_allclose(d["P_num"], d["gamma_eff"] * a["RP"] + a["dPpsi"], rtol=1e-8)          # as the reference states it (:156)
    # and as a number: nothing yields (no plastic law), so ΔPψ = 0; γ_eff = 5 · 20 / 25 = 4 (ηb = Kb dt = 5, γ_num = 20 η); RP = -(1.3 - 0.4)
    assert not a["dPpsi"].any()
    np.testing.assert_allclose(d["P_num"], -3.6, rtol=1e-8)
    dy.ph_residual(a, _di)
    assert np.isfinite(a["Rx"]).all() and np.isfinite(a["Ry"]).all()
    for k in ("Dx", "Dy", "dtauVx", "dtauVy"):
        d[k][...] = 1.0
    for k in ("betaVx", "betaVy", "alphaVx", "alphaVy"):
        d[k][...] = 0.0
    Vx0, Vy0 = a["Vx"].copy(), a["Vy"].copy()
    dy.dr_residual_update_V(a, d, _di)
    assert np.isfinite(a["Rx"]).all()
    assert np.array_equal(a["Vx"], Vx0) and np.array_equal(a["Vy"], Vy0)


def test_init_gives_positive_preconditioner_and_stable_steps():
    """DYREL! on the single-phase state: ηb = Kb dt, γ_eff = γ_phy γ_num / (γ_phy + γ_num) with γ_num = 20 η, D > 0, and α, β from dτ = 2 CFL / √λmax with c = 0"""
    a, d, phases, di, _ = _single_phase_state()
    np.testing.assert_allclose(d["etab"], 5.0, rtol=1e-15)
    np.testing.assert_allclose(d["gamma_eff"], 5.0 * 20.0 / 25.0, rtol=1e-15)
    assert (d["Dx"] > 0).all() and (d["Dy"] > 0).all() and (d["lmaxVx"] > 0).all()
    np.testing.assert_allclose(d["dtauVx"], 2 / np.sqrt(d["lmaxVx"]) * 0.99, rtol=1e-15)
    np.testing.assert_allclose(d["betaVx"], d["dtauVx"], rtol=1e-15)          # c = 0: β = dτ, α = 1
    np.testing.assert_allclose(d["alphaVy"], 1.0, rtol=1e-15)


def test_longdouble_evaluation_tracks_float64():
    """the restatement computes in the dtype of its arrays: the extended evaluation the GPU tolerance is measured with differs from float64 by rounding only"""
    a, d, phases, di, _ = _single_phase_state()
    aL, dL, *_ = _single_phase_state(np.longdouble)
    assert aL["exx"].dtype == np.longdouble and dL["Dx"].dtype == np.longdouble
    _di = (1.0 / di[0], 1.0 / di[1])
    for s, dd in ((a, d), (aL, dL)):
        dy.strain_rate_RP(s, dd, _di, 1.0)
        dy.stress_viscosity(s, dd, phases, 1.0, 1.0, 1.0e-2, (-np.inf, np.inf), False)
    for k in ("txx", "tyy", "txy", "tII", "eta"):
        assert aL[k].dtype == np.longdouble
        np.testing.assert_allclose(a[k], aL[k].astype(np.float64), rtol=1e-13, atol=1e-15)


def test_header_declares_the_prototypes():
    protos, structs = c_prototypes(), c_structs()
    for fn in ("jrx_dyrel2d_init", "jrx_dyrel2d_solve", "jrx_dyrel2d_strain_rate_RP", "jrx_dyrel2d_stress_viscosity", "jrx_dyrel2d_PH_residual",
               "jrx_dyrel2d_DR_residual_update_V", "jrx_dyrel2d_gershgorin", "jrx_dyrel2d_update_dtauV_alpha_beta", "jrx_dyrel2d_bulk_viscosity_and_penalty"):
        assert fn in protos, fn
    assert protos["jrx_dyrel2d_solve"] == ["Ptr{Cvoid}", "Ref{JrxVep2dFields}", "Ref{JrxDyrel2dFields}", "Ref{JrxRockRatio2d}", "Ref{JrxRheology}",
                                            "Ref{JrxVep2dParams}", "Ref{JrxDyrel2dParams}", "Ref{JrxDyrel2dResult}"]
    names = [f[0] for f in structs["jrx_dyrel2d_fields"]]
    assert names[:3] == ["gamma_eff", "etab", "P_num"] and "Rx0" in names and "dPpsi" in names and len(names) == 30
    assert [f[0] for f in structs["jrx_dyrel2d_params"]][-5:] == ["CFL", "eps", "eps_vel", "c_fact", "gamma_fact"]
    hdr = (ROOT / "include" / "jrx.h").read_text()
    assert "solver.jl:44-294" in hdr and "stat_dyrel_launches" in hdr


def test_extension_defines_the_methods():
    txt = JULIA_EXT.read_text()
    for pat in (r"JR2D\.DYREL\(::Type\{AMDGPUBackend\}", r"function JR2D\.DYREL!\(", r"function JR2D\.solve_DYREL!\(::Trait", r":jrx_dyrel2d_solve", r":jrx_dyrel2d_init"):
        assert re.search(pat, txt), pat
    # the reference's front method forwards the caller's keywords as one keyword named `kwargs` (solver.jl:36-37) and only the backend method splats it
    # (ext/AMDGPU/2D.jl:392-393): every solve_DYREL! method here declares `; kwargs)`, never the slurp `; kwargs...)`, which would swallow that one pair
    sigs = re.findall(r"^function JR2D\.solve_DYREL!\((.*?)\)\n", txt, flags=re.S | re.M)
    assert len(sigs) == 2
    for sig in sigs:
        assert re.search(r";\s*kwargs$", sig), sig
    body = txt[txt.index("function JR2D.solve_DYREL!(::Trait"):]
    body = body[:body.index("function dyrel_update!")]
    assert "dyrel_params2d(dyrel; kwargs...)" in body          # splatted where the keywords are read,
    assert "igg; kwargs = kwargs)" in body and "igg; kwargs...)" not in body          # and passed on whole by the `di` method


def test_integration_lists_dyrel_as_provided():
    txt = (ROOT / "INTEGRATION.md").read_text()
    assert "solve_DYREL!" in txt and "jrx_dyrel2d_solve" in txt
    for line in txt.splitlines():
        if "not provided" in line.lower():
            assert "DYREL" not in line, line
