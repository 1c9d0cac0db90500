"""CPU: the NumPy restatements of the per-step operators (tests/_stepops.py), which tests/test_gpu_stepops.py holds the kernels of csrc/stepops.hip
against, pinned to what the reference's texts and its own test state."""
import numpy as np

import _stepops as SO


def _grid(ni, rng):
    """non-uniform vertices (sorted random) and their cell centres"""
    xvi = tuple(np.sort(rng.uniform(-1.0, 2.0, n + 1)) for n in ni)
    xci = tuple((x[:-1] + x[1:]) / 2 for x in xvi)
    return xci, xvi


def _velocities(ni):
    if len(ni) == 2:
        nx, ny = ni
        shapes = ((nx + 1, ny + 2), (nx + 2, ny + 1))
    else:
        nx, ny, nz = ni
        shapes = ((nx + 1, ny + 2, nz + 2), (nx + 2, ny + 1, nz + 2), (nx + 2, ny + 2, nz + 1))
    return [np.full(s, SO.SENTINEL) for s in shapes]


def test_pureshear_bc_2d_is_the_reference_comprehension():
    rng = np.random.default_rng(1)
    ni, εbg = (5, 4), 0.37
    xci, xvi = _grid(ni, rng)
    Vx, Vy = _velocities(ni)
    SO.pureshear_bc2d(Vx, Vy, xci, xvi, εbg)
    for i in range(ni[0] + 1):
        for j in range(ni[1]):
            assert Vx[i, j + 1] == εbg * xvi[0][i]
    for i in range(ni[0]):
        for j in range(ni[1] + 1):
            assert Vy[i + 1, j] == -εbg * xvi[1][j]
    # the ghosts still hold the sentinel
    assert np.all(Vx[:, 0] == SO.SENTINEL) and np.all(Vx[:, -1] == SO.SENTINEL)
    assert np.all(Vy[0, :] == SO.SENTINEL) and np.all(Vy[-1, :] == SO.SENTINEL)


def test_pureshear_bc_3d_built_form_and_its_ghosts():
    rng = np.random.default_rng(2)
    ni, εbg = (4, 4, 3), -1.25
    xci, xvi = _grid(ni, rng)
    Vx, Vy, Vz = _velocities(ni)
    SO.pureshear_bc3d(Vx, Vy, Vz, xci, xvi, εbg)
    nx, ny, nz = ni
    assert np.array_equal(Vx[:, 1:-1, 1:-1], np.broadcast_to((εbg * xvi[0])[:, None, None], (nx + 1, ny, nz)))
    assert np.array_equal(Vy[1:-1, :, 1:-1], np.broadcast_to((εbg * xvi[1])[None, :, None], (nx, ny + 1, nz)))
    assert np.array_equal(Vz[1:-1, 1:-1, :], np.broadcast_to((-εbg * xvi[2])[None, None, :], (nx, ny, nz + 1)))
    for V, axes in ((Vx, (1, 2)), (Vy, (0, 2)), (Vz, (0, 1))):
        for ax in axes:
            assert np.all(np.take(V, 0, axis=ax) == SO.SENTINEL) and np.all(np.take(V, -1, axis=ax) == SO.SENTINEL)
    # y vertices that differ from the x vertices do show in Vy: the built form is not the literal one there
    L = _velocities(ni)
    SO.pureshear_bc3d_literal(*L, xci, xvi, εbg)
    assert not np.array_equal(L[1], Vy)


def test_pureshear_bc_3d_equals_the_literal_text_where_x_and_y_vertices_coincide():
    rng = np.random.default_rng(3)
    ni, εbg = (4, 4, 3), 0.8
    xci, xvi = _grid(ni, rng)
    xvi = (xvi[0], xvi[0].copy(), xvi[2])
    xci = (xci[0], xci[0].copy(), xci[2])
    built, literal = _velocities(ni), _velocities(ni)
    SO.pureshear_bc3d(*built, xci, xvi, εbg)
    SO.pureshear_bc3d_literal(*literal, xci, xvi, εbg)
    for b, l in zip(built, literal):
        assert np.array_equal(b, l)


def test_caricchi_meets_the_reference_bounds():
    """test/test_rheology.jl:246-252: 0.95 < ϕ < 1 at 1373.15 K, ϕ < 1e-6 at 573.15 K, where its comment records ~3e-10"""
    ph = dict(melting=dict(kind="caricchi"))
    hot = SO.compute_melt_fraction((4, 4), None, [ph], 1373.15)
    cold = SO.compute_melt_fraction((4, 4), None, [ph], 573.15)
    assert np.all((0.95 < hot) & (hot < 1.0))
    assert np.all(cold < 1.0e-6)
    assert np.all((1.5e-10 < cold) & (cold < 6.0e-10))
    assert np.all(SO.compute_melt_fraction((4, 4), None, [dict()], 1373.15) == 0.0)


def test_fn_ratio_with_args_returns_a_pure_phase_alone():
    ratio = np.array([[0.25, 1.0, 0.0], [0.75, 0.0, 1.0]])
    got = SO.fn_ratio_args([np.array([2.0, 3.0, 5.0]), 7.0], ratio)
    assert np.array_equal(got, np.array([0.25 * 2.0 + 0.75 * 7.0, 3.0, 7.0]))
    assert np.array_equal(SO.fn_ratio([2.0, 7.0], ratio), np.array([0.25 * 2.0 + 0.75 * 7.0, 2.0, 7.0]))


def test_subgrid_characteristic_time_constant_material():
    """ρCp = 3e6, K = 3, dx = dy = 0.5: 3e6 / (2 · 3 · (4 + 4)) = 62,500 exactly"""
    ni = (5, 4)
    table = [dict(k=3.0, Cp=1.0e3, density=dict(kind="constant", rho0=3.0e3))]
    T = np.full((ni[0] + 2, ni[1] + 2), 300.0)
    P = np.zeros(ni)
    dt0 = SO.subgrid_characteristic_time(np.ones((1,) + ni), table, T, P, (0.5, 0.5))
    assert dt0.shape == ni and np.all(dt0 == 62500.0)


def test_subgrid_characteristic_time_reads_the_cells_own_node_of_T():
    """T = thermal.T[I .+ 1]: with a T-dependent density only the interior of the ghosted array matters"""
    rng = np.random.default_rng(5)
    ni = (4, 3, 2)
    table = [dict(k=2.0, Cp=1.1e3, density=dict(kind="PT", rho0=3.0e3, alpha=3.0e-5, beta=1.0e-11, T0=273.0))]
    T = rng.uniform(300.0, 1500.0, tuple(n + 2 for n in ni))
    P = rng.uniform(0.0, 1.0e9, ni)
    one = np.ones((1,) + ni)
    a = SO.subgrid_characteristic_time(one, table, T, P, (0.5, 0.25, 0.125))
    T2 = T.copy()
    T2[0], T2[-1], T2[:, 0], T2[:, -1], T2[:, :, 0], T2[:, :, -1] = 1, 2, 3, 4, 5, 6
    assert np.array_equal(a, SO.subgrid_characteristic_time(one, table, T2, P, (0.5, 0.25, 0.125)))
    ρ = 3.0e3 * (1.0 - 3.0e-5 * (T[1:-1, 1:-1, 1:-1] - 273.0) + 1.0e-11 * P)
    assert np.allclose(a, 1.1e3 * ρ / (2 * 2.0 * (4.0 + 16.0 + 64.0)), rtol=1e-14)


def test_free_surface_restatements_write_the_top_interior_only():
    rng = np.random.default_rng(7)
    nx, ny, nz = 5, 4, 3
    a = dict(Vx=rng.uniform(0.1, 1, (nx + 1, ny + 2)), Vy=rng.uniform(0.1, 1, (nx + 2, ny + 1)), phase_c=np.stack([np.full((nx, ny), 0.25), np.full((nx, ny), 0.75)]))
    a.update({k: rng.uniform(0.1, 1, (nx, ny)) for k in ("P", "P0", "toyy", "eta")})
    before = a["Vy"].copy()
    SO.free_surface_bcs2d(a, (1.0, 2.0), 0.5, 0.2, 0.1)
    changed = a["Vy"] != before
    assert changed[1:-1, -1].all() and changed.sum() == nx
    i = 2
    G = 0.25 * 1.0 + 0.75 * 2.0
    want = 1e-2 * (before[i + 1, -2] + 1.5 * (a["P"][i, -1] / (2 * a["eta"][i, -1]) + (a["toyy"][i, -1] + a["P0"][i, -1]) / (2 * G * 0.5) +
                                                (a["Vx"][i + 1, -2] - a["Vx"][i, -2]) / 3 / 0.2) * 0.1) + 0.99 * before[i + 1, -1]
    assert abs(a["Vy"][i + 1, -1] - want) <= 4 * np.finfo(float).eps * abs(want)
    b = dict(Vx=rng.uniform(0.1, 1, (nx + 1, ny + 2, nz + 2)), Vy=rng.uniform(0.1, 1, (nx + 2, ny + 1, nz + 2)), Vz=rng.uniform(0.1, 1, (nx + 2, ny + 2, nz + 1)),
             phase_c=np.stack([np.full((nx, ny, nz), 0.5)] * 2))
    b.update({k: rng.uniform(0.1, 1, (nx, ny, nz)) for k in ("P", "P0", "toyy", "tozz", "eta")})
    before = b["Vz"].copy()
    SO.free_surface_bcs3d(b, (1.0, 2.0), 0.5, (0.2, 0.1, 0.3))
    changed = b["Vz"] != before
    assert changed[1:-1, 1:-1, -1].all() and changed.sum() == nx * ny
    zz = dict(b, Vz=before.copy())
    SO.free_surface_bcs3d(zz, (1.0, 2.0), 0.5, (0.2, 0.1, 0.3), stress="tozz")
    assert not np.array_equal(zz["Vz"], b["Vz"])          # τ_o.yy, not τ_o.zz, is what the law reads
