"""The NumPy restatement of the 3D DYREL solver (tests/_dyrel3d.py): pinned to the reference's own 3D allocator test, to exact fields, to the 2D restatement on
plane-strain extrusions and -- where the reference has no text -- to the operator itself: the eigenvalue bound is checked against the assembled matrix of the
restated kernels.  Then the static side of the interface.  The GPU tests (tests/test_gpu_dyrel3d.py) compare the HIP kernels with this restatement."""
import re

import numpy as np
import pytest

import _dyrel as dy2
import _dyrel3d as dy
from _abi_parse import JULIA_EXT, ROOT, c_prototypes, c_structs
from _variational_stokes3d import EDGES

COMP = "xyz"


# ---------------------------------------------------------------- 1. the reference's "DYREL 3D allocator" test (test/test_dyrel.jl:54-88)
def test_allocator_matches_the_reference_test(jr):
    nx, ny, nz = 6, 5, 4
    d = jr.DYREL(jr.CPUBackend, (nx, ny, nz), ϵ=1.0e-7, ϵ_vel=2.0e-7, CFL=0.6, c_fact=0.3)
    shapes = dict(γ_eff=(nx, ny, nz), ηb=(nx, ny, nz), Dx=(nx - 1, ny, nz), Dy=(nx, ny - 1, nz), Dz=(nx, ny, nz - 1), λmaxVx=(nx - 1, ny, nz), λmaxVy=(nx, ny - 1, nz),
                  λmaxVz=(nx, ny, nz - 1), dVxdτ=(nx - 1, ny, nz), dVydτ=(nx, ny - 1, nz), dVzdτ=(nx, ny, nz - 1), βVx=(nx - 1, ny, nz), αVy=(nx, ny - 1, nz),
                  cVz=(nx, ny, nz - 1), P_num=(nx, ny, nz), Rx0=(nx - 1, ny, nz), Ry0=(nx, ny - 1, nz), Rz0=(nx, ny, nz - 1))
    for k, s in shapes.items():
        assert tuple(getattr(d, k).shape) == s, k
    assert (d.CFL, d.ϵ, d.ϵ_vel, d.c_fact) == (0.6, 1.0e-7, 2.0e-7, 0.3)
    for k in ("γ_eff", "P_num", "Dz", "λmaxVz"):
        assert not getattr(d, k).any(), k
    d2 = jr.DYREL(jr.CPUBackend, nx, ny, nz, CFL=0.7)          # the 3-integer forwarder
    assert tuple(d2.Dz.shape) == (nx, ny, nz - 1) and d2.CFL == 0.7
    # the restatement's allocator has the same shapes; velocity_dofs / pressure_dof (solver.jl:349-357) at this size, worked by hand
    r = dy.new_dyrel((nx, ny, nz))
    assert r["Dx"].shape == (5, 5, 4) and r["Dy"].shape == (6, 4, 4) and r["Dz"].shape == (6, 5, 3) and r["P_num"].shape == (6, 5, 4)
    assert dy.velocity_dofs((nx, ny, nz)) == (4 * 4 * 3, 5 * 3 * 3, 5 * 4 * 2) == (48, 45, 40)
    assert dy.pressure_dof((nx, ny, nz)) == 120
    # the 2D class keeps its (1, 1) z placeholders
    assert tuple(jr.DYREL(jr.CPUBackend, (6, 5)).Dz.shape) == (1, 1)


# ---------------------------------------------------------------- 2. pure fields (test_dyrel_kernels.jl's 2D checks carried up)
def _linear_state(ni, coef, dtype=np.float64):
    a = dy.alloc_state(ni, 1, dtype)
    for k in ("phase_c", "phase_yz", "phase_xz", "phase_xy"):
        a[k][...] = 1.0
    a["eta"][...] = 1.0
    for q, c in enumerate(COMP):
        x = np.linspace(0.0, 1.0, ni[q] + 1)
        a["V" + c][...] = (coef[q] * x).reshape(tuple(-1 if s == q else 1 for s in range(3)))
    phases = [dict(eta=1.0, G=1.0, Kb=5.0)]
    d = dy.new_dyrel(ni, dtype)
    di = tuple(1.0 / n for n in ni)
    dy.dyrel_init(a, d, phases, di, 1.0)
    return a, d, phases, di


@pytest.mark.parametrize("coef", [(2.0, -0.7, -1.3), (0.9, 0.9, 0.9)], ids=["pure_shear", "uniform_dilation"])
def test_pure_fields_give_exact_strain_rates(coef):
    ni = (6, 5, 4)
    a, d, phases, di = _linear_state(ni, coef)
    _di = tuple(1.0 / x for x in di)
    div = dy.strain_rate_RP(a, d, _di, 1.0)
    s = sum(coef)
    np.testing.assert_allclose(div, s, rtol=1e-8, atol=1e-12)          # pure shear: the sum is zero
    for q, c in enumerate(COMP):
        np.testing.assert_allclose(a["e" + c + c], coef[q] - s / 3, rtol=1e-8, atol=1e-12)
    for name in EDGES:
        assert (np.abs(a["e" + name]) < 1.0e-12).all()
    np.testing.assert_allclose(a["RP"], -s, rtol=1e-8, atol=1e-12)          # P = P0, Q = 0
    # β = 0: the velocities do not move, bit for bit
    dy.stress_viscosity(a, d, phases, 1.0, 1.0, 1.0, (-np.inf, np.inf), False)
    assert np.isfinite(a["eta"]).all() and (a["eta"] > 0).all()
    np.testing.assert_allclose(d["P_num"], d["gamma_eff"] * a["RP"] + a["dPpsi"], rtol=1e-8)
    for c in COMP:
        d["betaV" + c][...] = 0.0
    V0 = [a["V" + c].copy() for c in COMP]
    dy.dr_residual_update_V(a, d, _di)
    assert all(np.isfinite(a["R" + c]).all() for c in COMP)
    assert all(np.array_equal(a["V" + c], v) for c, v in zip(COMP, V0))


# ---------------------------------------------------------------- 3. plane strain
def _plane_state(seed=7):
    """a randomised 2D state (tests/_dyrel.py's recipe) whose velocity comes from an integer vertex stream function on spacings that are powers of two: every velocity
    difference is exact, so the discrete divergence is exactly zero"""
    ni2 = (5, 4)
    a2, d2, phases, _, dt = dy2.random_state(ni2, seed=seed)
    rng = np.random.default_rng(seed)
    _di2 = (4.0, 2.0)
    # ψ at the vertices: Vx[i, j+1] = (ψ[i, j+1] - ψ[i, j]) / dy, Vy[i+1, j] = -(ψ[i+1, j] - ψ[i, j]) / dx; the ghost rows stay zero
    psi = rng.integers(-8, 9, size=(ni2[0] + 1, ni2[1] + 1)).astype(float)
    a2["Vx"][...] = 0.0
    a2["Vy"][...] = 0.0
    a2["Vx"][:, 1:-1] = (psi[:, 1:] - psi[:, :-1]) * _di2[1]
    a2["Vy"][1:-1, :] = -(psi[1:, :] - psi[:-1, :]) * _di2[0]
    # the conditions under which the 2D vertex half and the 3D edge half coincide
    with np.errstate(divide="ignore"):
        a2["eta_v"][...] = 1.0 / dy2._av_clamped(1.0 / a2["eta"])
    a2["toxx_v"][...] = dy2._av_clamped(a2["toxx"])
    a2["toyy_v"][...] = dy2._av_clamped(a2["toyy"])
    return a2, d2, phases, _di2, dt


def _extrude(a2, d2, ax, n):
    p, q = [k for k in range(3) if k != ax]
    sh = EDGES[ax]
    ni3 = [0, 0, 0]
    ni3[p], ni3[q], ni3[ax] = a2["P"].shape[0], a2["P"].shape[1], n
    ni3 = tuple(ni3)
    nph = a2["phase_c"].shape[0]
    a3, d3 = dy.alloc_state(ni3, nph), dy.new_dyrel(ni3)
    lift = lambda A, m, off=0: np.repeat(np.expand_dims(A, ax + off), m, axis=ax + off)
    pp, qq = COMP[p] * 2, COMP[q] * 2
    for k in ("P", "P0", "Q", "RP", "eta", "EII_pl", "dPpsi", "lam", "divV", "evol_pl", "EVol_pl", "tII", "eta_vep"):
        a3[k][...] = lift(a2[k], n)
    for pre in ("e", "t", "to", "epl"):
        a3[pre + pp][...], a3[pre + qq][...] = lift(a2[pre + "xx"], n), lift(a2[pre + "yy"], n)
        a3[pre + sh][...] = lift(a2[pre + "xy"], n)
    for pre in ("t", "to"):
        a3[pre + sh + "_c"][...] = lift(a2[pre + "xy_c"], n)
    a3["f" + COMP[p]][...], a3["f" + COMP[q]][...] = lift(a2["fx"], n), lift(a2["fy"], n)
    a3["lamv_" + sh][...] = lift(a2["lamv"], n)
    a3["phase_c"][...] = lift(a2["phase_c"], n, 1)
    a3["phase_" + sh][...] = lift(a2["phase_v"], n, 1)
    for T, name in enumerate(EDGES):
        if T != ax:
            a3["phase_" + name][0] = 1.0
    a3["V" + COMP[p]][...], a3["V" + COMP[q]][...] = lift(a2["Vx"], n + 2), lift(a2["Vy"], n + 2)
    a3["R" + COMP[p]][...], a3["R" + COMP[q]][...] = lift(a2["Rx"], n), lift(a2["Ry"], n)
    for k in ("gamma_eff", "etab", "P_num"):
        d3[k][...] = lift(d2[k], n)
    for k in dy.DYREL_STAG:
        d3[k.format(COMP[p])][...], d3[k.format(COMP[q])][...] = lift(d2[k.format("x")], n), lift(d2[k.format("y")], n)
        d3[k.format(COMP[ax])][...] = 1.0
    d3[f"dV{COMP[ax]}dtau"][...] = 0.0          # nothing moves out of the plane to begin with
    return a3, d3, (p, q, sh, pp, qq)


def _rel(got, want):
    return float(np.max(np.abs(got - want))) / (float(np.max(np.abs(want))) or 1.0)


@pytest.mark.parametrize("ax", [0, 1, 2])
def test_plane_strain_reproduces_the_2d_restatement(ax):
    """A 2D state extruded over 3 cells along `ax`, out-of-plane velocity 0, in-plane velocity from a vertex stream function.  On every plane the 3D restatement
    reproduces tests/_dyrel.py to 1e-13 relative (same terms, different order of summation; the bound and reason of
    tests/test_variational_stokes3d_restatement.py::test_plane_strain_reproduces_the_masked_2d_kernels): unconditionally for the strain rates, RP, the PH residual
    and the in-plane DR update given equal D / α / β / dτ; for the stress kernel's centre outputs and the in-plane edge family under the conditions that make the
    two forms coincide -- the 2D side is fed ηv = the harmonic clamped average of η and τ_o.xx_v / yy_v = the clamped averages of the centre values (which is
    what a 3D edge gathers), and linear_viscosity = true where the edge outputs are compared (the 2D text refreshes ηv from the vertex stress, 3D has no ηv).
    Out-of-plane quantities stay exactly zero."""
    n, TOL = 3, 1.0e-13
    for lin in (True, False):
        a2, d2, phases, _di2, dt = _plane_state()
        a3, d3, (p, q, sh, pp, qq) = _extrude(a2, d2, ax, n)
        _di3 = [8.0, 8.0, 8.0]
        _di3[p], _di3[q] = _di2
        other = [name for T, name in enumerate(EDGES) if T != ax]
        aa = COMP[ax] * 2
        planes = lambda A: [np.take(A, k, axis=ax) for k in range(A.shape[ax])]

        def same(k3, ref, what):
            for k, sec in enumerate(planes(a3[k3] if isinstance(k3, str) else k3)):
                assert _rel(sec, ref) <= TOL, (what, k3 if isinstance(k3, str) else "", k, _rel(sec, ref))
        div2 = dy2.strain_rate_RP(a2, d2, _di2, dt)
        div3 = dy.strain_rate_RP(a3, d3, _di3, dt)
        assert not div2.any() and not div3.any()          # the stream function: exactly divergence-free
        for k3, k2 in (("e" + pp, "exx"), ("e" + qq, "eyy"), ("e" + sh, "exy"), ("RP", "RP")):
            same(k3, a2[k2], "strain")
        assert not a3["e" + aa].any() and not any(a3["e" + o].any() for o in other)
        dy2.stress_viscosity(a2, d2, phases, 0.7, dt, 0.3, (1.0e-2, 5.0), lin)
        dy.stress_viscosity(a3, d3, phases, 0.7, dt, 0.3, (1.0e-2, 5.0), lin)
        cen = [("t" + pp, "txx"), ("t" + qq, "tyy"), ("t" + sh + "_c", "txy_c"), ("epl" + pp, "eplxx"), ("epl" + qq, "eplyy"), ("evol_pl", "evol_pl"), ("tII", "tII"),
               ("eta_vep", "eta_vep"), ("lam", "lam"), ("dPpsi", "dPpsi"), ("eta", "eta")]
        for k3, k2 in cen:
            same(k3, a2[k2], "stress centre")
        same(d3["P_num"], d2["P_num"], "θc")
        assert (a2["lam"] > 0).any() and not (a2["lam"] > 0).all()          # both branches of the law are exercised
        if lin:
            for k3, k2 in (("t" + sh, "txy"), ("epl" + sh, "eplxy"), ("lamv_" + sh, "lamv")):
                same(k3, a2[k2], "stress edge")
            assert (a2["lamv"] > 0).any()
        for k in ["t" + aa, "epl" + aa] + ["t" + o for o in other] + ["epl" + o for o in other] + ["t" + o + "_c" for o in other]:
            assert not a3[k].any(), k
        if not lin:
            continue          # the 2D edge stresses of the non-linear form have seen the refreshed ηv: the residuals are compared on the linear form
        dy2.ph_residual(a2, _di2)
        dy.ph_residual(a3, _di3)
        same("R" + COMP[p], a2["Rx"], "PH residual")
        same("R" + COMP[q], a2["Ry"], "PH residual")
        assert not a3["R" + COMP[ax]].any()
        dy2.dr_residual_update_V(a2, d2, _di2)
        dy.dr_residual_update_V(a3, d3, _di3)
        for c3, c2 in ((COMP[p], "x"), (COMP[q], "y")):
            same("R" + c3, a2["R" + c2], "DR residual")
            same(d3[f"dV{c3}dtau"], d2[f"dV{c2}dtau"], "dVdτ")
            V3 = a3["V" + c3]
            inner = np.take(V3, range(1, n + 1), axis=ax)
            for k in range(n):
                assert _rel(np.take(inner, k, axis=ax), a2["V" + c2]) <= TOL
        assert not a3["V" + COMP[ax]].any() and not a3["R" + COMP[ax]].any()


# ---------------------------------------------------------------- 4. the bound is a bound of this operator
def _operator_state(dtype, seed=11):
    ni = (4, 3, 3)
    rng = np.random.default_rng(seed)
    phases = [dict(eta=1.0, G=1.0, Kb=2.0), dict(eta=1.0, G=0.5, Kb=3.0)]          # no plastic law: nothing yields
    a = dy.alloc_state(ni, 2)
    a["eta"][...] = 10.0 ** rng.uniform(-1.0, 1.0, size=ni)
    for k in ("phase_c", "phase_yz", "phase_xz", "phase_xy"):          # one phase per node: the bound takes G from the node's ratios, the law takes it per phase
        r = (rng.uniform(size=a[k].shape[1:]) < 0.5).astype(float)
        a[k][0], a[k][1] = r, 1.0 - r
    d = dy.new_dyrel(ni)
    di, dt = (0.25, 0.4, 0.3), 0.25
    dy.bulk_viscosity_and_penalty(a, d, phases, 20.0, dt)
    d["gamma_eff"][...] = rng.uniform(0.5, 3.0, size=ni)
    a, d = dy.astype(a, dtype), dy.astype(d, dtype)
    dy.gershgorin(a, d, phases, di, dt)
    return a, d, phases, di, dt


def _apply(a, d, phases, di, dt, V):
    """V (the interior velocities, ghosts and wall-normal planes held at zero) -> D .* R of the restated chain strain rate -> stress -> DR residual with θc"""
    _di = tuple(1.0 / x for x in di)
    for c, v in zip(COMP, V):
        a["V" + c][...] = 0.0
        a["V" + c][1:-1, 1:-1, 1:-1] = v
    dy.strain_rate_RP(a, d, _di, dt, True)
    dy.stress_viscosity(a, d, phases, 1.0, dt, 1.0, (-np.inf, np.inf), True)
    return dy._momentum(a, d["P_num"], _di)


def _matrix(dtype):
    a, d, phases, di, dt = _operator_state(dtype)
    shapes = [a["R" + c].shape for c in COMP]
    sizes = [int(np.prod(s)) for s in shapes]
    N = sum(sizes)
    A = np.zeros((N, N), dtype=dtype)
    for col in range(N):
        e = np.zeros(N, dtype=dtype)
        e[col] = 1.0
        V = [e[sum(sizes[:q]):sum(sizes[:q + 1])].reshape(shapes[q], order="F") for q in range(3)]
        R = _apply(a, d, phases, di, dt, V)
        A[:, col] = np.concatenate([r.reshape(-1, order="F") for r in R])
    D = np.concatenate([d["D" + c].reshape(-1, order="F") for c in COMP])
    lmax = np.concatenate([d["lmaxV" + c].reshape(-1, order="F") for c in COMP])
    interior = []
    for q, s in enumerate(shapes):
        idx = np.indices(s)
        ok = np.ones(s, dtype=bool)
        for k in range(3):
            ok &= (idx[k] >= 1) & (idx[k] <= s[k] - 2)
        interior.append(ok.reshape(-1, order="F"))
    return A, D, lmax, np.concatenate(interior), (a, d, phases, di, dt)


def test_the_bound_is_a_bound_of_the_restated_operator():
    """ni = (4, 3, 3), random positive η and γ_eff, two phases with finite G (one per node), τ_o = 0, P = P0 = 0, no yielding.  A = the matrix of V -> D .* R of the
    restated chain, column by column from unit perturbations of each interior velocity entry with the ghosts at zero.  For float64 and longdouble: |A_ii| = D_i for
    every entry; Σ_j |A_ij| <= D_i λmax_i for every row; equality for the rows whose whole stencil lies in the interior (at this size: the Vx row (1, 1, 1)).
    `Equal` is 16 x the float64-longdouble spread of the compared quantity (the rule of tests/test_gpu_dyrel.py).  This replaces the missing reference text; the last
    lines show that it does see a permuted neighbour role."""
    (A64, D64, l64, inner, st), (AL, DL, lL, _, _) = _matrix(np.float64), _matrix(np.longdouble)
    assert inner.sum() >= 1
    diag64, diagL = np.abs(np.diag(A64)), np.abs(np.diag(AL))
    rows64, rowsL = np.abs(A64).sum(axis=1), np.abs(AL).sum(axis=1)
    b64, bL = D64 * l64, DL * lL
    spread = lambda x, y: 16.0 * float(np.max(np.abs(x.astype(np.longdouble) - y)))
    tol_d = max(spread(diag64, diagL), spread(D64, DL))
    tol_r = max(spread(rows64, rowsL), spread(b64, bL))
    for diag, D, rows, b in ((diag64, D64, rows64, b64), (diagL, DL, rowsL, bL)):
        assert (D > 0).all()
        assert float(np.max(np.abs(diag - D))) <= tol_d, (float(np.max(np.abs(diag - D))), tol_d)
        assert (rows <= b + tol_r).all(), float(np.max(rows - b))
        assert float(np.max(np.abs(rows[inner] - b[inner]))) <= tol_r, (rows[inner], b[inner], tol_r)
        assert (rows[~inner] < b[~inner] - 1.0e3 * tol_r).any()          # a wall row misses entries: there the bound is strict
    # a permuted role: the Vx bound with the xy and xz edges exchanged no longer equals the interior row sum
    a, d, phases, di, dt = st
    d2 ={k: v.copy() for k, v in d.items()}
    dy.gershgorin(a, d2, phases, (di[0], di[2], di[1]), dt)          # dy and dz exchanged in the formula alone
    bad = (d2["Dx"] * d2["lmaxVx"]).reshape(-1, order="F")
    nx_rows = bad.size
    assert float(np.max(np.abs(rows64[:nx_rows][inner[:nx_rows]] - bad[inner[:nx_rows]]))) > 1.0e6 * tol_r


# ---------------------------------------------------------------- 5. initialisation and driver
def test_init_gives_positive_preconditioner_and_stable_steps():
    """DYREL! on the randomised state: D > 0, λmax finite and positive, dτ = 2 CFL / √λmax.  With the damping the driver would set, c = 2 √λmin c_fact for some
    λmin <= min λmax (here: that minimum), c dτ = 4 CFL c_fact √(λmin / λmax) <= 1.98 < 2, so 0 < α = (2 - c dτ) / (2 + c dτ) < 1 at every node"""
    a, d, phases, di, dt = dy.random_state((6, 5, 4))
    dy.dyrel_init(a, d, phases, di, dt)
    lmin = min(float(d["lmaxV" + c].min()) for c in COMP)
    for c in COMP:
        d["cV" + c][...] = 2 * np.sqrt(lmin) * 0.5
    dy.update_dtauV_alpha_beta(d, 0.99)
    for c in COMP:
        assert (d["D" + c] > 0).all() and np.isfinite(d["lmaxV" + c]).all() and (d["lmaxV" + c] > 0).all()
        np.testing.assert_allclose(d["dtauV" + c], 2 / np.sqrt(d["lmaxV" + c]) * 0.99, rtol=1e-15)
        assert ((d["alphaV" + c] > 0) & (d["alphaV" + c] < 1)).all() and (d["betaV" + c] > 0).all()
    np.testing.assert_allclose(d["etab"], dy._ratio_sum([2.0, 3.0], a["phase_c"]) * dt, rtol=1e-15)


def test_driver_converges_on_a_small_shear_band():
    """the restated driver on an 8 x 8 x 6 shear band (spherical inclusion) reduces err_evo_tot below ϵ = 1e-6 and ends on its Powell-Hestenes criterion"""
    ni = (8, 8, 6)
    a, phases, di, dt = dy.shearband_state(*ni)
    d = dy.new_dyrel(ni)
    h = dy.solve_DYREL(a, d, phases, di, dt, eps=1.0e-6, nout=25, rel_drop=0.5, viscosity_relaxation=1, linear_viscosity=True, iterMax=50.0e3)
    print(f"iter {h['iter']}, itPH {h['itPH']}, err_evo_tot[-1] = {h['err_evo_tot'][-1]:.3e}")
    assert 0 < h["iter"] < 50_000 and h["itPH"] < 1000
    assert h["err_evo_tot"][-1] < 1.0e-6 and h["err_evo_tot"][0] == pytest.approx(1.0, rel=1e-12)
    assert len(h["err_evo_it"]) == h["iter"] // 25
    assert np.abs(a["Vy"][1:-1, 1:-1, 1:-1]).max() > 0          # the sphere drives flow along y too
    for k in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        assert np.array_equal(a["to" + k], a["t" + k])


def test_longdouble_run_tracks_float64():
    ni = (6, 5, 4)
    out = []
    for T in (np.float64, np.longdouble):
        a, phases, di, dt = dy.shearband_state(*ni, psi_deg=5.0, C_cos=0.39)
        a, d = dy.astype(a, T), dy.new_dyrel(ni, T)
        h = dy.solve_DYREL(a, d, phases, di, dt, eps=0.0, nout=10, iterMax=11, total_iterMax=30)
        out.append((a, d, h))
    (a, d, h), (aL, dL, hL) = out
    assert (h["iter"], h["itPH"]) == (hL["iter"], hL["itPH"]) == (36, 3)
    assert aL["txx"].dtype == np.longdouble and dL["Dz"].dtype == np.longdouble
    assert (a["lam"] > 0).any()
    for k in ("txx", "tzz", "txz", "tyz", "tII", "eta", "P", "Vx", "Vy", "Vz"):
        np.testing.assert_allclose(a[k], aL[k].astype(np.float64), rtol=1e-9, atol=1e-12)
    for k in ("Dx", "lmaxVz", "alphaVy", "dVzdtau"):
        np.testing.assert_allclose(d[k], dL[k].astype(np.float64), rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------- 6. wiring
FNS = ("jrx_dyrel3d_init", "jrx_dyrel3d_solve", "jrx_dyrel3d_strain_rate_RP", "jrx_dyrel3d_stress_viscosity", "jrx_dyrel3d_PH_residual",
       "jrx_dyrel3d_DR_residual_update_V", "jrx_dyrel3d_gershgorin", "jrx_dyrel3d_update_dtauV_alpha_beta", "jrx_dyrel3d_bulk_viscosity_and_penalty")


def test_header_declares_the_prototypes():
    protos, structs = c_prototypes(), c_structs()
    for fn in FNS:
        assert fn in protos, fn
    assert protos["jrx_dyrel3d_solve"] == ["Ptr{Cvoid}", "Ref{JrxVep3dFields}", "Ref{JrxDyrel3dFields}", "Ref{JrxRockRatio3d}", "Ref{JrxRheology}",
                                            "Ref{JrxVep3dParams}", "Ref{JrxDyrel2dParams}", "Ref{JrxDyrel2dResult}"]
    names = [f[0] for f in structs["jrx_dyrel3d_fields"]]
    assert names[:3] == ["gamma_eff", "etab", "P_num"] and len(names) == 37
    for k in ("Dz", "lmaxVz", "Rz0", "lambda", "lambda_yz", "lambda_xz", "lambda_xy", "dPpsi", "dT", "melt_fraction"):
        assert k in names, k
    hdr = (ROOT / "include" / "jrx.h").read_text()
    sec = hdr[hdr.index("3D DYREL"):]
    assert "No reference text" in sec and "StressKernels.jl:672-989" in sec and "velocity_kernels.jl:729-828" in sec and "stat_dyrel_launches" in sec
    from justrelax_jl_amd import _lib
    assert _lib.DYREL3_NAMES == names


def test_extension_defines_the_methods():
    txt = JULIA_EXT.read_text()
    for pat in (r"JR3D\.DYREL\(::Type\{AMDGPUBackend\}", r"function JR3D\.DYREL!\(", r"function JR3D\.solve_DYREL!\(::Trait", r":jrx_dyrel3d_solve", r":jrx_dyrel3d_init",
                r":jrx_dyrel3d_update_dtauV_alpha_beta", r"JR3D\.update_α_β!", r"JR3D\.update_dτV_α_β!"):
        assert re.search(pat, txt), pat
    sigs = re.findall(r"^function JR3D\.solve_DYREL!\((.*?)\)\n", txt, flags=re.S | re.M)
    assert len(sigs) == 2
    for sig in sigs:
        assert re.search(r";\s*kwargs$", sig), sig          # one keyword named kwargs, as the reference's front method forwards it (solver.jl:36-37)


def test_integration_lists_3d_dyrel():
    txt = (ROOT / "INTEGRATION.md").read_text()
    assert "jrx_dyrel3d_solve" in txt and "jrx_dyrel3d_init" in txt
    for line in txt.splitlines():
        if "not provided" in line.lower():
            assert "DYREL" not in line, line
    assert "the 3D methods of `src/DYREL`" not in (ROOT / "DESIGN.md").read_text().split("## 7")[1].split("## 8")[0]
