"""CPU: the NumPy restatement of the 2D particle operators (tests/_particles2d.py), which tests/test_gpu_particles2d.py holds the kernels of csrc/particles.hip
to bit for bit, pinned by properties that follow from the definitions of include/jrx.h; and the static side of the new interface: the declarations of the
header, the exports of the library, the ccalls of the Julia extension, the ctypes mirror, the host-side seeding and the refusals of the Python layer."""
import ctypes as C

import numpy as np
import pytest

import _particles2d as PT
from _abi_parse import HEADER, ROOT, c_prototypes, c_structs, julia_ccalls, same_arg

ENTRY_POINTS = ("jrx_particles2d_advect_rk2", "jrx_particles2d_move", "jrx_particles2d_grid2particle", "jrx_particles2d_particle2grid",
                "jrx_particles2d_phase_ratios")
NI = (7, 5)
DX, DY = 0.125, 0.09375          # dy = 0.75 dx, both exact in binary


def _xvi(ni=NI, origin=(0.25, -0.5)):
    return tuple(origin[d] + np.arange(ni[d] + 1) * (DX, DY)[d] for d in range(2))


def _cloud(ni=NI, nxcell=4, max_xcell=12, seed=3):
    return PT.init_particles(nxcell, max_xcell, 2, _xvi(ni), ni, rng=np.random.default_rng(seed))


def _uniform_V(ni, vx, vy):
    nx, ny = ni
    return np.full((nx + 1, ny + 2), vx), np.full((nx + 2, ny + 1), vy)


# ---------------------------------------------------------------------------------------------- the restatement
def test_seeding_puts_every_particle_in_its_bucket_and_keeps_the_invariant():
    p = _cloud()
    assert p.active.sum() == 4 * 35 and np.all(p.active[:, :, :4] == 1) and np.all(p.active[:, :, 4:] == 0)
    assert np.all(p.px[p.active == 0] == 0.0) and np.all(p.py[p.active == 0] == 0.0)
    for i in range(p.nx):
        for j in range(p.ny):
            for s in range(4):
                assert PT.owner(p, p.px[i, j, s], p.py[i, j, s]) == (i, j)
    q = PT.init_particles(12, 24, 6, _xvi(), NI)          # the regular lattice: 3 x 4 sub-cells, centred
    assert PT.lattice(12) == (3, 4) and PT.lattice(4) == (2, 2) and PT.lattice(7) == (1, 7)
    assert np.allclose((q.px[2, 1, :3] - (q.x0 + 2 * DX)) / DX, [1 / 6, 3 / 6, 5 / 6], rtol=0, atol=1e-12)
    assert np.allclose((q.py[2, 1, 0:12:3] - (q.y0 + 1 * DY)) / DY, [1 / 8, 3 / 8, 5 / 8, 7 / 8], rtol=0, atol=1e-12)


def test_a_uniform_translation_conserves_the_count_and_moves_every_particle_to_exactly_x_plus_dt_v():
    """V = (2^-3, -2^-3) everywhere: the interpolant of a constant that is a power of two is that constant in every rounding ((1 - t) + t rounds to 1), so both
    stages see it and x' = x + dt v with a single rounding.  dt = 2.4 dx gives the displacement (0.3 dx, -0.4 dy)."""
    ni = (9, 8)
    p = PT.init_particles(4, 12, 2, _xvi(ni), ni, rng=np.random.default_rng(11))
    keep = (p.px > p.x0 + 0.5 * DX) & (p.px < p.x0 + (ni[0] - 0.5) * DX) & (p.py > p.y0 + 0.5 * DY) & (p.py < p.y0 + (ni[1] - 0.5) * DY) & (p.active != 0)
    p.active[:] = keep
    p.px[~keep], p.py[~keep] = 0.0, 0.0          # a frame of half a cell is emptied so that nothing leaves the grid
    x0, y0, n0 = p.px.copy(), p.py.copy(), int(p.active.sum())
    v, dt = 2.0 ** -3, 2.4 * DX
    assert abs(dt * v - 0.3 * DX) < 1e-15 and abs(dt * v - 0.4 * DY) < 1e-15
    PT.advect_rk2(p, *_uniform_V(ni, v, -v), dt)
    a = p.active != 0
    assert np.array_equal(p.px[a], (x0 + dt * v)[a]) and np.array_equal(p.py[a], (y0 + dt * -v)[a])
    assert np.array_equal(p.px[~a], x0[~a]) and np.all(p.px[~a] == 0.0)
    pid = np.where(a, np.arange(a.size).reshape(a.shape) + 1.0, 0.0)
    d, (pid2,), c = PT.move(p, (pid,))
    assert c == dict(n_active_before=n0, n_active_after=n0, n_outside=0, n_far=0, n_overflow=0) and int(d.active.sum()) == n0
    # the same particles, each now in the bucket of its owner, none duplicated
    assert sorted(pid2[d.active != 0]) == sorted(pid[a])
    where = {pid[idx]: (p.px[idx], p.py[idx]) for idx in zip(*np.nonzero(a))}
    for i, j, s in zip(*np.nonzero(d.active)):
        assert where[pid2[i, j, s]] == (d.px[i, j, s], d.py[i, j, s]) and PT.owner(d, d.px[i, j, s], d.py[i, j, s]) == (i, j)
    assert np.all(d.px[d.active == 0] == 0.0) and np.all(pid2[d.active == 0] == 0.0)


def test_a_nonfinite_coordinate_is_left_alone_and_a_point_outside_the_node_box_extrapolates():
    p = _cloud()
    rng = np.random.default_rng(5)
    Vx, Vy = rng.uniform(-1, 1, (NI[0] + 1, NI[1] + 2)), rng.uniform(-1, 1, (NI[0] + 2, NI[1] + 1))
    p.px[3, 2, 1], p.py[4, 4, 0] = np.nan, np.inf
    before = PT.copy(p)
    PT.advect_rk2(p, Vx, Vy, 0.01)
    assert np.isnan(p.px[3, 2, 1]) and p.py[3, 2, 1] == before.py[3, 2, 1] and p.px[4, 4, 0] == before.px[4, 4, 0] and p.py[4, 4, 0] == np.inf
    assert np.isfinite(np.delete(p.px.ravel(), np.ravel_multi_index((3, 2, 1), p.px.shape))).all()
    # a field linear in x is reproduced two cells outside its node box: nothing is clamped
    A = np.add.outer(3.0 * np.arange(5), np.zeros(4))
    v, ok = PT.interp(A, 0.0, 0.0, 1.0, 1.0, np.array([-2.0, 6.5]), np.array([1.25, 1.25]))
    assert ok.all() and np.array_equal(v, [-6.0, 19.5])


def test_grid2particle_reproduces_a_field_linear_in_x_and_y_to_rounding():
    p = _cloud()
    xv, yv = _xvi()
    F = 2.0 + 3.0 * xv[:, None] - 5.0 * yv[None, :]
    pF = PT.grid2particle(F, p)
    a = p.active != 0
    want = 2.0 + 3.0 * p.px - 5.0 * p.py
    assert np.abs(pF[a] - want[a]).max() <= 16 * np.finfo(float).eps * np.abs(F).max()
    assert np.all(pF[~a] == 0.0)


def test_particle2grid_of_a_constant_returns_the_constant():
    p = _cloud()
    F0 = np.full((NI[0] + 1, NI[1] + 1), -9.0)
    for c, exact in ((4.0, True), (0.7, False)):          # a power of two scales num and den alike in every rounding
        F = PT.particle2grid(F0, np.where(p.active != 0, c, 0.0), p)
        assert np.array_equal(F, np.full_like(F, c)) if exact else np.abs(F - c).max() <= 8 * np.finfo(float).eps
    p.active[2:4, 1:3, :] = 0          # the vertex (3, 2) has no particle around it: left as it was
    F = PT.particle2grid(F0, np.where(p.active != 0, 4.0, 0.0), p)
    assert F[3, 2] == -9.0 and (F == -9.0).sum() == 1


def test_the_ratios_of_a_one_phase_cloud_are_exactly_one():
    p = _cloud()
    for N, k in ((1, 1), (3, 2)):
        old = {m: np.full(PT.member_shape(m, NI, N), -1.0) for m in PT.MEMBERS}
        new, n_empty = PT.phase_ratios(old, np.where(p.active != 0, float(k), 0.0), N, p)
        assert n_empty == 0
        for m in PT.MEMBERS:
            assert np.all(new[m][k - 1] == 1.0) and np.all(np.delete(new[m], k - 1, axis=0) == 0.0), m
    # two phases: every member sums to one, and a phase outside 1 .. N is skipped
    ph = np.where(p.active != 0, 1.0 + (np.arange(p.active.size).reshape(p.active.shape) % 3), 0.0)          # 1, 2, 3 with N = 2
    new, n_empty = PT.phase_ratios({m: np.zeros(PT.member_shape(m, NI, 2)) for m in PT.MEMBERS}, ph, 2, p)
    assert n_empty == 0 and all(np.abs(new[m].sum(axis=0) - 1.0).max() < 1e-14 for m in PT.MEMBERS)


def test_emptied_cells_leave_their_members_unchanged_and_are_counted():
    p = _cloud()
    p.active[2:5, 1:4, :] = 0          # a 3 x 3 block of cells
    old = {m: np.full(PT.member_shape(m, NI, 2), -3.0) for m in PT.MEMBERS}
    new, n_empty = PT.phase_ratios(old, np.where(p.active != 0, 1.0, 0.0), 2, p)
    untouched = {m: int(np.all(new[m] == -3.0, axis=0).sum()) for m in PT.MEMBERS}
    assert untouched == dict(center=9, vertex=4, Vx=6, Vy=6) and n_empty == 25


def _two_arrivals():
    """3 x 3 cells, max_xcell = 3: the centre cell keeps one of its own and receives one particle from (0, 0) [dj = -1, di = -1], one from (2, 0) [dj = -1,
    di = 1] and one from (0, 1) [dj = 0, di = -1]"""
    ni = (3, 3)
    xvi = (np.arange(4) * 1.0, np.arange(4) * 1.0)
    p = PT.init_particles(1, 3, 0, xvi, ni)
    p.active[:], p.px[:], p.py[:] = 0, 0.0, 0.0
    tag = np.zeros_like(p.px)

    def put(i, j, s, x, y, t):
        p.active[i, j, s], p.px[i, j, s], p.py[i, j, s], tag[i, j, s] = 1, x, y, t
    put(1, 1, 2, 1.5, 1.5, 10.0)          # own, in slot 2: own particles come first whatever their slot
    put(0, 1, 0, 1.1, 1.9, 30.0)          # from the west neighbour (dj = 0)
    put(2, 0, 1, 1.9, 1.1, 20.0)          # from the south-east neighbour (dj = -1, di = 1)
    put(0, 0, 0, 1.2, 1.2, 15.0)          # from the south-west neighbour (dj = -1, di = -1)
    return p, tag


def test_the_gather_order_own_first_then_neighbours_dj_outermost():
    p, tag = _two_arrivals()
    p.max_xcell = 3
    d, (t,), c = PT.move(p, (tag,))
    # three slots: own, south-west, south-east; the west one finds the bucket full
    assert list(t[1, 1]) == [10.0, 15.0, 20.0] and list(d.px[1, 1]) == [1.5, 1.2, 1.9] and list(d.active[1, 1]) == [1, 1, 1]
    assert c == dict(n_active_before=4, n_active_after=3, n_outside=0, n_far=0, n_overflow=1)
    assert d.active.sum() == 3


def test_outside_far_and_overflow_counts_on_constructed_inputs():
    ni = (5, 4)
    xvi = (np.arange(6) * 1.0, np.arange(5) * 1.0)
    p = PT.init_particles(1, 2, 0, xvi, ni)
    p.active[:], p.px[:], p.py[:] = 0, 0.0, 0.0
    pts = {(0, 0, 0): (-0.1, 0.5),         # left of the grid: outside
           (4, 3, 0): (5.0, 3.5),          # exactly on the upper x boundary: outside
           (4, 3, 1): (4.5, 4.0),          # exactly on the upper y boundary: outside
           (2, 2, 0): (np.nan, 2.5),       # NaN: outside
           (1, 1, 0): (3.5, 1.5),          # two cells to the right: far
           (1, 1, 1): (1.5, 3.5),          # two cells up: far
           (2, 0, 0): (3.5, 0.5),          # to (3, 0)
           (2, 0, 1): (3.6, 0.6),          # to (3, 0)
           (3, 1, 0): (3.7, 0.7),          # to (3, 0): the third arrival in a bucket of two
           (0, 3, 0): (0.0, 3.0)}          # exactly on the lower corner of its own cell: stays
    for (i, j, s), (x, y) in pts.items():
        p.active[i, j, s], p.px[i, j, s], p.py[i, j, s] = 1, x, y
    d, _, c = PT.move(p)
    assert c == dict(n_active_before=10, n_active_after=3, n_outside=4, n_far=2, n_overflow=1)
    assert list(d.px[3, 0]) == [3.5, 3.6] and d.px[0, 3, 0] == 0.0 and d.active[0, 3, 0] == 1 and d.active.sum() == 3
    assert c["n_active_before"] == c["n_active_after"] + c["n_outside"] + c["n_far"] + c["n_overflow"]


# ---------------------------------------------------------------------------------------------- the interface
def test_the_header_declares_the_entry_points_and_the_extension_calls_them_as_declared():
    protos, calls = c_prototypes(), julia_ccalls()
    for fn in ENTRY_POINTS:
        assert fn in protos, fn
        assert fn in calls, f"the Julia extension never calls {fn}"
        for ret, args in calls[fn]:
            assert ret == "Cint" and len(args) == len(protos[fn]), (fn, args, protos[fn])
            assert all(same_arg(w, g) for w, g in zip(protos[fn], args)), (fn, protos[fn], args)
    assert protos["jrx_particles2d_move"] == ["Ptr{Cvoid}", "Ref{JrxParticles2d}", "Ref{JrxParticles2d}", "Ptr{Ptr{Float64}}", "Ptr{Ptr{Float64}}", "Int32", "Ptr{Int64}"]
    want = [("px", "double", True, 1), ("py", "double", True, 1), ("active", "int32_t", True, 1), ("nx", "int64_t", False, 1), ("ny", "int64_t", False, 1),
            ("max_xcell", "int32_t", False, 1)] + [(k, "double", False, 1) for k in ("x0", "y0", "dx", "dy", "_dx", "_dy")]
    assert c_structs()["jrx_particles2d"] == want


def test_the_header_states_the_layout_and_the_rules():
    txt = HEADER.read_text()
    sec = txt[txt.index("2D marker-in-cell particles"):]
    for s in ("SLOT index is SLOWEST", "coalesce", "opposite of the PhaseRatios layout", "INVARIANT", "EXTRAPOLATES", "range-checked ON THE DOUBLE",
              "Shearheating2D.jl:69-82,221-232", "stat_particles_launches", "n_overflow", "n_empty", "a handle with a communicator"):
        assert s in sec, s
    assert "stat_particles_launches" in txt[:txt.index("jrx_status jrx_set_option")]
    integ = (ROOT / "INTEGRATION.md").read_text()
    assert all(fn in integ for fn in ENTRY_POINTS)
    assert "particles.hip" in (ROOT / "justrelax.jl_amd" / "build.py").read_text()


def test_the_library_exports_the_entry_points_and_the_binding_mirrors_the_struct(jr):
    from justrelax_jl_amd import _lib
    L = _lib.load(check_symbols=True)
    for fn in ENTRY_POINTS:
        assert fn in _lib.declared_symbols() and hasattr(L, fn), fn
    assert [f[0] for f in _lib.Particles2D._fields_] == [f[0] for f in c_structs()["jrx_particles2d"]]
    assert C.sizeof(_lib.Particles2D) == 3 * 8 + 2 * 8 + 8 + 6 * 8          # max_xcell padded to 8 ahead of the doubles
    # a NULL handle is refused before anything is read
    assert L.jrx_particles2d_advect_rk2(None, None, None, None, 0.0) == 4


def test_init_particles_on_the_host_equals_the_restatement(jr):
    ni, xvi = (6, 5), _xvi((6, 5))
    for nxcell, mx, rng in ((4, 12, 7), (12, 24, None), (5, 6, 1)):
        mk = (lambda: np.random.default_rng(rng)) if rng is not None else (lambda: None)
        p = jr.init_particles(jr.CPUBackend, nxcell, mx, 1, xvi, ni, rng=mk())
        q = PT.init_particles(nxcell, mx, 1, xvi, ni, rng=mk())
        assert p.shape == ni + (mx,) and (p.x0, p.y0, p.dx, p.dy, p._dx, p._dy) == (q.x0, q.y0, q.dx, q.dy, q._dx, q._dy)
        assert np.array_equal(jr.to_numpy(p.coords[0]), q.px) and np.array_equal(jr.to_numpy(p.coords[1]), q.py)
        assert np.array_equal(p.index.numpy(), q.active) and p.index.dtype.itemsize == 4
        from justrelax_jl_amd.arrays import is_fortran
        assert is_fortran(p.coords[0]) and is_fortran(p.index)          # slot index slowest
    g = jr.Geometry(ni, (6 * DX, 5 * DY), origin=(0.25, -0.5))
    assert jr.init_particles(jr.CPUBackend, 4, 8, 1, g, ni).ni == ni          # a Geometry in place of xvi


def test_the_python_layer_refuses_what_is_not_built(jr):
    ni, xvi = (6, 5), _xvi((6, 5))
    B = jr.CPUBackend
    with pytest.raises(NotImplementedError, match="2D"):
        jr.init_particles(B, 4, 8, 1, xvi + (np.arange(4.0),), ni + (3,))
    stretched = (np.array([0.0, 0.1, 0.3, 0.6, 1.0, 1.5, 2.1]), xvi[1])
    with pytest.raises(NotImplementedError, match="uniform"):
        jr.init_particles(B, 4, 8, 1, stretched, ni)
    with pytest.raises(NotImplementedError, match="non-uniform"):
        jr.init_particles(B, 4, 8, 1, jr.Geometry.from_vertices(stretched), ni)
    with pytest.raises(ValueError, match="max_xcell"):
        jr.init_particles(B, 9, 8, 1, xvi, ni)
    with pytest.raises(ValueError, match="entries"):
        jr.init_particles(B, 4, 8, 1, xvi, (5, 5))
    for name in ("inject_particles_phase_", "MarkerChain", "StressParticles"):
        with pytest.raises(NotImplementedError, match="not built"):
            getattr(jr, name)()
    with pytest.raises(NotImplementedError, match="midpoint"):
        jr.RungeKutta2(2 / 3)
    p = jr.init_particles(B, 4, 8, 1, xvi, ni)
    pT, pPhases = jr.init_cell_arrays(p, 2)
    assert tuple(pT.shape) == (6, 5, 8) and float(pT.abs().max()) == 0.0
    st = jr.StokesArrays(B, ni)
    pr = jr.PhaseRatios(B, 2, ni)
    F = jr.fzeros((7, 6), p.device)
    # shapes and kinds are looked at before the device
    with pytest.raises(ValueError, match="V is"):
        jr.advection_(p, jr.RungeKutta2(), (st.V.Vy, st.V.Vx), 0.1)
    with pytest.raises(NotImplementedError, match="RungeKutta2"):
        jr.advection_(p, "Euler", st.V, 0.1)
    with pytest.raises(NotImplementedError, match="non-uniform"):
        jr.advection_(p, jr.RungeKutta2(), st.V, 0.1, grid=jr.Geometry.from_vertices(stretched))
    with pytest.raises(ValueError, match="init_cell_arrays"):
        jr.move_particles_(p, (pT.clone(),))
    with pytest.raises(ValueError, match="twice"):
        jr.move_particles_(p, (pT, pT))
    with pytest.raises(ValueError, match="vertex field"):
        jr.grid2particle_(pT, st.P, p)
    with pytest.raises(ValueError, match="vertex field"):
        jr.particle2grid_(st.P, pT, p)
    with pytest.raises(ValueError, match="phase_ratios.center"):
        jr.update_phase_ratios_(jr.PhaseRatios(B, 2, (5, 5)), p, pPhases)
    with pytest.raises(NotImplementedError, match="3D"):
        jr.update_phase_ratios_(jr.PhaseRatios(B, 2, (6, 5, 3)), p, pPhases)
    # ... and CPU arrays are refused: there is no CPU path
    for call in (lambda: jr.advection_(p, jr.RungeKutta2(), st.V, 0.1), lambda: jr.move_particles_(p, (pT, pPhases)), lambda: jr.grid2particle_(pT, F, p),
                 lambda: jr.particle2grid_(F, pT, p), lambda: jr.update_phase_ratios_(pr, p, pPhases)):
        with pytest.raises(NotImplementedError, match="CPU arrays"):
            call()
    assert float(pr.center.abs().max()) == 0.0 and float(pT.abs().max()) == 0.0


def test_the_swap_keeps_the_identity_of_the_callers_tensors(jr):
    p = jr.init_particles(jr.CPUBackend, 2, 4, 1, _xvi((3, 3)), (3, 3))
    (f,) = jr.init_cell_arrays(p, 1)
    twin = p._twins[id(f)][1]
    f.fill_(1.0), twin.fill_(2.0)
    px, px2 = p.coords[0], p._coords2[0]
    p._swap((f,))
    assert float(f.min()) == 2.0 and float(twin.max()) == 1.0 and p._twins[id(f)][0] is f          # f now reads what the move wrote into its twin
    assert p.coords[0] is px2 and p._coords2[0] is px
