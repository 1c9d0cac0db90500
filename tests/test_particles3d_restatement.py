"""CPU: pins tests/_particles3d.py, the NumPy restatement of the 3D particle operators (include/jrx.h, section "3D marker-in-cell particles"), with cases that
can be checked by hand, and the Python layer of justrelax_jl_amd.particles in 3D: seeding in the reference's call shape, the 3D operators that stay out,
shape mismatches and the refusal of CPU arrays.  tests/test_gpu_particles3d.py holds the kernels to this text bit for bit."""
import numpy as np
import pytest

import _particles2d as PT2
import _particles3d as PT

DX, DY, DZ = 0.125, 0.09375, 0.0625
ORIGIN = (0.25, -0.5, 1.0)


def _xi_vel(ni, spacing=(DX, DY, DZ), origin=ORIGIN):
    """the velocity grids of a uniform grid: vertices along the component's own axis, centres with one ghost point either side along the others"""
    nd = len(ni)
    xv = [origin[d] + np.arange(ni[d] + 1) * spacing[d] for d in range(nd)]
    gh = [origin[d] + (np.arange(ni[d] + 2) - 0.5) * spacing[d] for d in range(nd)]
    return tuple(tuple(xv[d] if d == c else gh[d] for d in range(nd)) for c in range(nd))


def _one(ni, at, xyz, mx=3, fields=()):
    """a cloud with one particle: bucket cell `at`, slot 1, coordinates xyz"""
    p = PT.init_particles(1, mx, 0, *_xi_vel(ni))
    p.px[:], p.py[:], p.pz[:], p.active[:] = 0.0, 0.0, 0.0, 0
    p.px[at + (1,)], p.py[at + (1,)], p.pz[at + (1,)], p.active[at + (1,)] = xyz[0], xyz[1], xyz[2], 1
    return p


def _centre(cell):
    return tuple(ORIGIN[d] + (cell[d] + 0.5) * (DX, DY, DZ)[d] for d in range(3))


# ---------------------------------------------------------------------------------------------- seeding
@pytest.mark.parametrize("nxcell,want", [(1, (1, 1, 1)), (8, (2, 2, 2)), (12, (2, 2, 3)), (20, (2, 2, 5))])
def test_the_lattice(nxcell, want):
    assert PT.lattice(nxcell) == want
    p = PT.init_particles(nxcell, nxcell + 2, 1, *_xi_vel((3, 2, 2)))
    assert p.active[..., :nxcell].all() and not p.active[..., nxcell:].any() and not p.px[..., nxcell:].any()
    # slot s = a + nsx (b + nsy c) sits in the middle of its sub-cell; cell (2, 1, 1) by hand
    for s in range(nxcell):
        a, b, c = s % want[0], (s // want[0]) % want[1], s // (want[0] * want[1])
        assert p.px[2, 1, 1, s] == (ORIGIN[0] + 2.0 * DX) + (a + 0.5) * (DX / want[0])
        assert p.py[2, 1, 1, s] == (ORIGIN[1] + 1.0 * DY) + (b + 0.5) * (DY / want[1])
        assert p.pz[2, 1, 1, s] == (ORIGIN[2] + 1.0 * DZ) + (c + 0.5) * (DZ / want[2])


def test_jittered_seeding_stays_inside_the_sub_cell_and_draws_x_then_y_then_z():
    ni = (3, 2, 2)
    p = PT.init_particles(8, 9, 1, *_xi_vel(ni), rng=np.random.default_rng(5))
    rng = np.random.default_rng(5)
    r = [rng.random(ni + (8,)) for _ in range(3)]
    s = np.arange(8)
    assert np.array_equal(p.py[1, 1, 0, :8], (ORIGIN[1] + 1.0 * DY) + (((s // 2) % 2).astype(float) + (0.05 + 0.9 * r[1][1, 1, 0])) * (DY / 2))
    assert np.array_equal(p.pz[1, 1, 0, :8], (ORIGIN[2] + 0.0 * DZ) + ((s // 4).astype(float) + (0.05 + 0.9 * r[2][1, 1, 0])) * (DZ / 2))
    inside, d = PT.owners(p)
    assert inside[..., :8].all() and not any(q[inside].any() for q in d)


def test_the_python_layer_seeds_the_same_particles_in_both_call_shapes(jr):
    B = jr.CPUBackend
    ni = (4, 3, 2)
    mk = lambda: np.random.default_rng(11)
    p = jr.init_particles(B, 12, 16, 2, *_xi_vel(ni), rng=mk())
    q = PT.init_particles(12, 16, 2, *_xi_vel(ni), rng=mk())
    assert p.ni == ni and p.shape == ni + (16,) and len(p.coords) == 3
    assert (p.x0, p.y0, p.z0, p.dx, p.dy, p.dz, p._dx, p._dy, p._dz) == (q.x0, q.y0, q.z0, q.dx, q.dy, q.dz, q._dx, q._dy, q._dz)
    for c, want in zip(p.coords, (q.px, q.py, q.pz)):
        assert np.array_equal(jr.to_numpy(c), want)
    assert np.array_equal(p.index.numpy(), q.active)
    from justrelax_jl_amd.arrays import is_fortran
    assert is_fortran(p.coords[2]) and is_fortran(p.index)          # slot index slowest
    assert p._work.numel() == 4 * 3 * 2 * 16 and p._work.element_size() == 1
    g = jr.Geometry(ni, (4 * DX, 3 * DY, 2 * DZ), origin=ORIGIN)
    assert jr.init_particles(B, 8, 12, 1, *g.xi_vel).ni == ni
    # 2D: the two velocity grids give bit for bit what (xvi, ni) gives
    ni2 = (6, 5)
    xv2 = _xi_vel(ni2)
    xvi = (xv2[0][0], xv2[1][1])
    a = jr.init_particles(B, 6, 8, 1, *xv2, rng=mk())
    b = jr.init_particles(B, 6, 8, 1, xvi, ni2, rng=mk())
    r = PT2.init_particles(6, 8, 1, xvi, ni2, rng=mk())
    assert a.ni == b.ni == ni2 and (a.x0, a.y0, a.dx, a.dy, a._dx, a._dy) == (b.x0, b.y0, b.dx, b.dy, b._dx, b._dy)
    for k in range(2):
        assert np.array_equal(jr.to_numpy(a.coords[k]).view(np.uint64), jr.to_numpy(b.coords[k]).view(np.uint64))
    assert np.array_equal(jr.to_numpy(a.coords[0]), r.px) and np.array_equal(jr.to_numpy(a.coords[1]), r.py) and np.array_equal(a.index.numpy(), b.index.numpy())


# ---------------------------------------------------------------------------------------------- move
@pytest.mark.parametrize("off", PT.NEIGHBOURS)
def test_a_particle_crossing_each_of_the_26_offsets_lands_in_the_right_bucket(off):
    ni, home = (3, 3, 3), (1, 1, 1)
    dest = tuple(h + o for h, o in zip(home, off))
    p = _one(ni, home, _centre(dest))
    pid = np.where(p.active != 0, 42.0, 0.0)
    dst, (f,), c = PT.move(p, (pid,))
    assert c == dict(n_active_before=1, n_active_after=1, n_outside=0, n_far=0, n_overflow=0)
    assert dst.active.sum() == 1 and dst.active[dest + (0,)] == 1 and f[dest + (0,)] == 42.0
    assert (dst.px[dest + (0,)], dst.py[dest + (0,)], dst.pz[dest + (0,)]) == _centre(dest)


def test_a_bucket_is_filled_in_the_defined_order():
    """the centre cell of 3^3 receives one particle from each of its 26 neighbours and keeps two of its own: own cell first in slot order, then dk outermost"""
    ni, home = (3, 3, 3), (1, 1, 1)
    p = PT.init_particles(1, 30, 0, *_xi_vel(ni))
    pid = np.zeros(p.px.shape)
    p.active[:] = 0
    for n, off in enumerate(PT.NEIGHBOURS):
        cell = tuple(h + o for h, o in zip(home, off))
        p.px[cell + (2,)], p.py[cell + (2,)], p.pz[cell + (2,)] = _centre(home)
        p.active[cell + (2,)], pid[cell + (2,)] = 1, 100.0 + n
    for s in (5, 0):
        p.px[home + (s,)], p.py[home + (s,)], p.pz[home + (s,)] = _centre(home)
        p.active[home + (s,)], pid[home + (s,)] = 1, float(s)
    dst, (f,), c = PT.move(p, (pid,))
    assert c["n_active_after"] == 28 and c["n_overflow"] == 0
    assert list(f[home][:28]) == [0.0, 5.0] + [100.0 + n for n in range(26)] and not f[home][28:].any()
    assert dst.active.sum() == 28


def test_the_upper_boundary_and_a_nan_are_outside_and_a_long_jump_is_far():
    ni = (3, 3, 3)
    top = ORIGIN[0] + 3 * DX
    c = PT.move(_one(ni, (2, 1, 1), (top,) + _centre((2, 1, 1))[1:]))[2]
    assert c["n_outside"] == 1 and c["n_active_after"] == 0
    c = PT.move(_one(ni, (2, 1, 1), (np.nextafter(top, 0.0),) + _centre((2, 1, 1))[1:]))[2]
    assert c["n_outside"] == 0 and c["n_active_after"] == 1
    p = _one(ni, (1, 1, 1), (_centre((1, 1, 1))[0], np.nan, _centre((1, 1, 1))[2]))
    dst, _, c = PT.move(p)
    assert c == dict(n_active_before=1, n_active_after=0, n_outside=1, n_far=0, n_overflow=0) and not np.isnan(dst.py).any()
    c = PT.move(_one(ni, (0, 1, 1), _centre((2, 1, 1))))[2]
    assert c == dict(n_active_before=1, n_active_after=0, n_outside=0, n_far=1, n_overflow=0)


def test_a_nan_coordinate_is_untouched_by_the_advection():
    ni = (3, 3, 3)
    V = _uniform_V(ni, (0.3 * DX, -0.2 * DY, 0.1 * DZ))
    p = PT.init_particles(8, 8, 1, *_xi_vel(ni))
    p.pz[1, 2, 0, 3] = np.nan
    q = PT.copy(p)
    PT.advect_rk2(q, V, 1.0)
    at = (1, 2, 0, 3)
    assert np.isnan(q.pz[at]) and q.px[at] == p.px[at] and q.py[at] == p.py[at]
    moved = np.ones(p.px.shape, dtype=bool)
    moved[at] = False
    assert np.allclose(q.px[moved], p.px[moved] + 0.3 * DX, rtol=0, atol=1e-15) and np.allclose(q.pz[moved], p.pz[moved] + 0.1 * DZ, rtol=0, atol=1e-15)


def test_overflow_and_the_sum_rule():
    """five particles head for a bucket of three slots that keeps one of its own: two are lost, and the counters add up"""
    ni, home = (3, 3, 3), (1, 1, 1)
    p = PT.init_particles(1, 3, 0, *_xi_vel(ni))
    p.active[:] = 0
    sources = [home, (0, 0, 0), (2, 0, 0), (1, 1, 2), (2, 2, 2)]
    for cell in sources:
        p.px[cell + (1,)], p.py[cell + (1,)], p.pz[cell + (1,)] = _centre(home)
        p.active[cell + (1,)] = 1
    p.active[0, 2, 2, 0], p.px[0, 2, 2, 0] = 1, ORIGIN[0] - DX          # and one that has left through the low x face
    pid = np.where(p.active != 0, 1.0 + np.arange(p.px.size).reshape(p.px.shape), 0.0)
    dst, (f,), c = PT.move(p, (pid,))
    assert c == dict(n_active_before=6, n_active_after=3, n_outside=1, n_far=0, n_overflow=2)
    assert c["n_active_before"] == c["n_active_after"] + c["n_outside"] + c["n_far"] + c["n_overflow"]
    assert list(f[home]) == [pid[home + (1,)], pid[0, 0, 0, 1], pid[2, 0, 0, 1]] and dst.active.sum() == 3


# ---------------------------------------------------------------------------------------------- interpolation
def _poly(X, Y, Z):
    """a trilinear polynomial: every interpolation here reproduces it to rounding, extrapolation included"""
    return 1.5 + 2.0 * X - 3.0 * Y + 0.5 * Z + 4.0 * X * Y - 1.25 * Y * Z + 0.75 * X * Z + 2.5 * X * Y * Z


def _uniform_V(ni, u):
    nx, ny, nz = ni
    return (np.full((nx + 1, ny + 2, nz + 2), u[0]), np.full((nx + 2, ny + 1, nz + 2), u[1]), np.full((nx + 2, ny + 2, nz + 1), u[2]))


def _jittered(ni, nxcell=8, mx=10, seed=3):
    return PT.init_particles(nxcell, mx, 1, *_xi_vel(ni), rng=np.random.default_rng(seed))


def test_grid2particle_and_centroid2particle_reproduce_a_trilinear_polynomial():
    ni = (4, 3, 5)
    p = _jittered(ni)
    a = p.active != 0
    exact = np.where(a, _poly(p.px, p.py, p.pz), 0.0)
    xv = [ORIGIN[d] + np.arange(ni[d] + 1) * (DX, DY, DZ)[d] for d in range(3)]
    xc = [0.5 * (x[1:] + x[:-1]) for x in xv]
    got = PT.grid2particle(_poly(*np.meshgrid(*xv, indexing="ij")), p)
    assert np.abs(got - exact).max() < 1e-13 and not got[~a].any()
    pF = np.full(p.px.shape, -5.0)
    got = PT.centroid2particle(pF, _poly(*np.meshgrid(*xc, indexing="ij")), p)          # the outer half cells extrapolate from the outermost pair of centres
    assert np.abs(got - exact).max() < 1e-13 and not got[~a].any()
    outer = a & (p.px < xc[0][0]) & (p.pz > xc[2][-1])
    assert outer.sum() > 5
    # a particle that has left its bucket cell: grid2particle extrapolates from the bucket's vertices, centroid2particle finds the pair from the coordinate
    p.px[1, 1, 1, 0] += 1.25 * DX
    want = _poly(p.px[1, 1, 1, 0], p.py[1, 1, 1, 0], p.pz[1, 1, 1, 0])
    assert abs(PT.grid2particle(_poly(*np.meshgrid(*xv, indexing="ij")), p)[1, 1, 1, 0] - want) < 1e-13
    assert abs(PT.centroid2particle(pF, _poly(*np.meshgrid(*xc, indexing="ij")), p)[1, 1, 1, 0] - want) < 1e-13
    # a slot whose coordinate is not finite keeps its value
    p.py[2, 2, 2, 1] = np.inf
    assert PT.centroid2particle(pF, _poly(*np.meshgrid(*xc, indexing="ij")), p)[2, 2, 2, 1] == -5.0


def test_the_advection_follows_a_uniform_velocity_and_a_linear_one_exactly_enough():
    ni = (4, 3, 5)
    p = _jittered(ni)
    q = PT.copy(p)
    PT.advect_rk2(q, _uniform_V(ni, (0.4 * DX, 0.3 * DY, -0.2 * DZ)), 1.0)
    a = p.active != 0
    assert np.abs(q.px - p.px - 0.4 * DX)[a].max() < 1e-15 and np.abs(q.pz - p.pz + 0.2 * DZ)[a].max() < 1e-15
    assert np.array_equal(q.px[~a], p.px[~a])
    # Vx = w x: the midpoint rule gives x (1 + w dt + (w dt)^2 / 2); the ghost layers hold the same linear function
    w = 0.25
    xi = _xi_vel(ni)
    V = list(_uniform_V(ni, (0.0, 0.0, 0.0)))
    V[0] = np.broadcast_to((w * xi[0][0])[:, None, None], V[0].shape).copy()
    q = PT.copy(p)
    PT.advect_rk2(q, V, 1.0)
    assert np.abs(q.px - p.px * (1.0 + w + 0.5 * w * w))[a].max() < 1e-14 and np.array_equal(q.py, p.py)


def test_particle2grid_and_particle2centroid_of_a_constant_give_the_constant_and_keep_what_no_weight_reaches():
    ni = (4, 3, 5)
    p = _jittered(ni)
    p.active[1:3, 0:2, 2:4, :] = 0          # an emptied block: the vertices (2, 0, 3) (on the low y face) and (2, 1, 3) and eight centres see nothing
    pF = np.where(p.active != 0, 7.25, 0.0)
    F = PT.particle2grid(np.full((5, 4, 6), -1.0), pF, p)
    assert F[2, 0, 3] == F[2, 1, 3] == -1.0 and (F == -1.0).sum() == 2 and np.abs(F[F != -1.0] - 7.25).max() < 1e-14
    Cn = PT.particle2centroid(np.full(ni, -1.0), pF, p)
    assert (Cn[1:3, 0:2, 2:4] == -1.0).all() and (Cn == -1.0).sum() == 8 and np.abs(Cn[Cn != -1.0] - 7.25).max() < 1e-14
    # a single particle: by hand
    q = _one((2, 2, 2), (0, 0, 0), (ORIGIN[0] + 0.25 * DX, ORIGIN[1] + 0.5 * DY, ORIGIN[2] + 0.75 * DZ))
    one = np.where(q.active != 0, 3.0, 0.0)
    G = PT.particle2grid(np.zeros((3, 3, 3)), one, q)
    assert (G[:2, :2, :2] == 3.0).all() and not G[2].any() and not G[:, 2].any()          # every weight is positive: num / den = 3 exactly


# ---------------------------------------------------------------------------------------------- phase ratios
@pytest.mark.parametrize("nphase", [1, 3])
def test_every_member_sums_to_one_where_weight_arrives_and_n_empty_counts_the_rest(nphase):
    ni = (4, 3, 5)
    p = _jittered(ni)
    a = p.active != 0
    ph = np.where(a, 1.0 + (np.arange(a.size).reshape(a.shape) % 3), 0.0)
    ph[0, 0, 0, 0], ph[3, 2, 4, 1] = 0.0, 9.0          # skipped
    p.active[1, 1, 2, :] = 0          # one emptied cell: its centre sees nothing; every other node still has a neighbour
    old = {m: np.full(PT.member_shape(m, ni, nphase), -7.0) for m in PT.MEMBERS}
    new, n_empty = PT.phase_ratios(old, ph, nphase, p)
    if nphase == 3:
        assert n_empty == 1 and (new["center"][:, 1, 1, 2] == -7.0).all()
    for m in PT.MEMBERS:
        assert new[m].shape == PT.member_shape(m, ni, nphase)
        filled = new[m][0] != -7.0
        assert np.abs(new[m][:, filled].sum(axis=0) - 1.0).max() < 1e-14, m
        assert (new[m][:, ~filled] == -7.0).all()
    assert n_empty == sum(int((new[m][0] == -7.0).sum()) for m in PT.MEMBERS)
    # by hand: one particle of phase 2 in cell (0, 0, 0) of a 2^3 grid reaches the nodes of that cell only: 1 centre, 8 vertices, 2 + 2 + 2 faces, 4 + 4 + 4 edges
    q = _one((2, 2, 2), (0, 0, 0), _centre((0, 0, 0)))
    ph = np.where(q.active != 0, 2.0, 0.0)
    old = {m: np.full(PT.member_shape(m, (2, 2, 2), 2), -7.0) for m in PT.MEMBERS}
    new, n_empty = PT.phase_ratios(old, ph, 2, q)
    reached = {m: int((new[m][1] == 1.0).sum()) for m in PT.MEMBERS}
    assert reached == dict(center=1, vertex=8, Vx=2, Vy=2, Vz=2, yz=4, xz=4, xy=4)
    assert all((new[m][0][new[m][1] == 1.0] == 0.0).all() for m in PT.MEMBERS)
    total = sum(int(np.prod(PT.member_shape(m, (2, 2, 2), 1))) for m in PT.MEMBERS)
    assert n_empty == total - sum(reached.values())


# ---------------------------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_what_is_not_built_in_3d(jr):
    B = jr.CPUBackend
    ni = (4, 3, 2)
    p = jr.init_particles(B, 8, 12, 1, *_xi_vel(ni))
    pT, pPhases, pa, pb = jr.init_cell_arrays(p, 4)
    assert tuple(pT.shape) == ni + (12,) and float(pT.abs().max()) == 0.0
    st, pr = jr.StokesArrays(B, ni), jr.PhaseRatios(B, 2, ni)
    Fv, Fc = jr.fzeros((5, 4, 3), p.device), jr.fzeros(ni, p.device)
    # the (xvi, ni) form stays 2D and says where 3D particles come from
    with pytest.raises(NotImplementedError, match="2D.*xi_vel"):
        jr.init_particles(B, 8, 12, 1, tuple(g[d] for d, g in enumerate(_xi_vel(ni))), ni)
    with pytest.raises(NotImplementedError, match="uniform"):
        xi = [list(g) for g in _xi_vel(ni)]
        xi[0][0] = np.array([0.0, 0.1, 0.3, 0.6, 1.0])
        jr.init_particles(B, 8, 12, 1, *xi)
    with pytest.raises(TypeError, match="velocity grids"):
        jr.init_particles(B, 8, 12, 1, *_xi_vel(ni)[:2])
    with pytest.raises(ValueError, match="max_xcell"):
        jr.init_particles(B, 13, 12, 1, *_xi_vel(ni))
    # the 3D operators that stay out are refused by name, before the device is looked at
    sa2 = None
    for call in (lambda: jr.inject_particles_phase_(p, pPhases, (pT,), (Fv,)), lambda: jr.rotate_stress_particles_((pT, pa, pb), (pPhases,), p, 0.1),
                 lambda: jr.rotate_stress_(pT, pa, pb, pPhases, st, p, 0.1), lambda: jr.stress2grid_(st, pT, pa, pb, p),
                 lambda: jr.SubgridDiffusionCellArrays(p), lambda: jr.subgrid_diffusion_centroid_(pT, Fc, Fc, sa2, p, 0.1),
                 lambda: jr.subgrid_diffusion_(pT, Fv, Fv, sa2, p, 0.1)):
        with pytest.raises(NotImplementedError, match="3D particles"):
            call()
    # shapes and kinds are looked at before the device
    with pytest.raises(ValueError, match="V is"):
        jr.advection_(p, jr.RungeKutta2(), (st.V.Vy, st.V.Vx, st.V.Vz), 0.1)
    with pytest.raises(NotImplementedError, match="components"):
        jr.advection_(p, jr.RungeKutta2(), (st.V.Vx, st.V.Vy), 0.1)
    with pytest.raises(NotImplementedError, match="2D grid"):
        jr.advection_(p, jr.RungeKutta2(), st.V, 0.1, grid=jr.Geometry((4, 3), (1.0, 1.0)))
    with pytest.raises(ValueError, match="init_cell_arrays"):
        jr.move_particles_(p, (pT.clone(),))
    with pytest.raises(ValueError, match="vertex field"):
        jr.grid2particle_(pT, Fc, p)
    with pytest.raises(ValueError, match="vertex field"):
        jr.particle2grid_(Fc, pT, p)
    with pytest.raises(ValueError, match="centre field"):
        jr.centroid2particle_(pT, Fv, p)
    with pytest.raises(ValueError, match="centre field"):
        jr.particle2centroid_(Fv, pT, p)
    with pytest.raises(ValueError, match="every extent >= 2"):
        q = jr.init_particles(B, 8, 12, 1, *_xi_vel((4, 1, 2)))
        jr.centroid2particle_(jr.init_cell_arrays(q, 1)[0], jr.fzeros((4, 1, 2), q.device), q)
    with pytest.raises(ValueError, match="phase_ratios.xz"):
        bad = jr.PhaseRatios(B, 2, ni)
        bad.xz = bad.xy
        jr.update_phase_ratios_(bad, p, pPhases)
    with pytest.raises(NotImplementedError, match="2D PhaseRatios"):
        jr.update_phase_ratios_(jr.PhaseRatios(B, 2, (4, 3)), p, pPhases)
    with pytest.raises(ValueError, match="init_cell_arrays"):
        jr.update_phase_ratios_(pr, p, jr.fzeros((4, 3, 12), p.device))
    # ... and CPU arrays are refused: there is no CPU path
    for call in (lambda: jr.advection_(p, jr.RungeKutta2(), st.V, 0.1), lambda: jr.move_particles_(p, (pT, pPhases)), lambda: jr.grid2particle_(pT, Fv, p),
                 lambda: jr.particle2grid_(Fv, pT, p), lambda: jr.centroid2particle_(pT, Fc, p), lambda: jr.particle2centroid_(Fc, pT, p),
                 lambda: jr.update_phase_ratios_(pr, p, pPhases)):
        with pytest.raises(NotImplementedError, match="CPU arrays"):
            call()
    assert float(pr.center.abs().max()) == 0.0 and float(pT.abs().max()) == 0.0
