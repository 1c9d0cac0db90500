"""GPU: the 3D free-surface operators (compute_rock_fraction_, advect_topography_, update_phases_given_topography_ on 3D grids; csrc/topography.hip through
jrx_compute_rock_fraction3d, jrx_advect_topography3d, jrx_update_phases_topography3d) against the NumPy restatement (tests/_topography3d.py): every member bit
for bit (np.array_equal -- the kernels have no fma and the library is built without contraction), the inputs untouched, sentinel-filled outputs fully written,
every refusal with the counters unchanged, the Python checks, the conversions, and the rock fractions feeding the 3D solve_VariationalStokes_.

Sizes: (1, 1, 1): every footprint clipped on every side, both vertex rows half high; (2, 3, 4) and (5, 4, 3): interior and clipped footprints, x != y so that a
transposition shows; (67, 3, 2): more nodes in x than one block of 64 holds, by more than one.  Every shape is a fraction of a second.
The refusal at 2^31 entries is exercised with the extents alone: it comes before anything is read, so the small arrays passed along are never touched."""
import ctypes as C

import numpy as np
import pytest

import _topography3d as TP

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (2, 3, 4), (5, 4, 3), (67, 3, 2)]
SURFACES = ("flat_face", "flat_mid", "tilt_x", "tilt_y", "tilt_xy", "saddle", "rough")
SENTINEL = -7.0e30
D = 2.0 ** -3
ORIGIN = (0.25, 0.75, -0.5)
DT = 2.0 ** -4
COUNTERS = ("stat_rock_fraction_calls", "stat_topography_advect_calls", "stat_topography_phase_calls")


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _up(a):
    from justrelax_jl_amd.arrays import from_numpy
    return from_numpy(np.asarray(a, dtype=np.float64), _dev())


@pytest.fixture(scope="module")
def h(jr):
    from justrelax_jl_amd import _lib
    return _lib.Handle(_dev().index)


def _grid(jr, ni):
    jr.finalize_global_grid()
    return jr.Geometry(ni, tuple(n * D for n in ni), origin=ORIGIN)


def _surface(kind, ni, seed=0):
    """heights (nx + 1, ny + 1) in the grid's coordinates"""
    nx, ny, nz = ni
    I, J = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64), indexing="ij")
    if kind == "flat_face":
        s = np.full(I.shape, float(nz // 2 + 1 if nz > 1 else 1))
    elif kind == "flat_mid":
        s = np.full(I.shape, nz // 2 + 0.5)
    elif kind == "tilt_x":           # leaves the box at both ends
        s = 0.5 * nz + (0.5 * nz + 0.75) * (2 * I / nx - 1)
    elif kind == "tilt_y":
        s = 0.5 * nz + (0.5 * nz + 0.75) * (2 * J / ny - 1)
    elif kind == "tilt_xy":
        s = 0.5 * nz + 0.3 * (I - 0.5 * nx) - 0.45 * (J - 0.5 * ny)
    elif kind == "saddle":           # s = x y, scaled into the box: the centre of a cell is on no plane through three of its corners
        s = 0.25 + (nz - 0.5) * (I / nx) * (J / ny)
    else:                            # multiples of 2^-9 in -2 .. nz + 2, every third vertex copies its neighbour: below the box, above it, flat edges
        rng = np.random.default_rng(20261020 + seed + nx)
        s = rng.integers(-2 * 512, (nz + 2) * 512, I.shape) / 512.0
        s[1::3, :] = s[0:-1:3, :][: s[1::3, :].shape[0], :]
        s[0, 0], s[-1, -1] = -1.5, nz + 1.25
    return ORIGIN[2] + s * D


def _topo(jr, ni, hs):
    t = jr.Topography(jr.AMDGPUBackend, ni[:2])
    t.fill_(hs)
    return t


def _counters(h):
    return tuple(h.get_option(k) for k in COUNTERS)


@pytest.fixture(scope="module")
def reference():
    """the restatement's members per (shape, surface), computed once and shared"""
    cache = {}

    def get(ni, kind):
        if (ni, kind) not in cache:
            hs = _surface(kind, ni)
            cache[ni, kind] = (hs, TP.compute_rock_fraction(hs, ni, ORIGIN[2], 1.0 / D))
        return cache[ni, kind]
    return get


# ---------------------------------------------------------------------------------------------- 1. rock fractions
@pytest.mark.parametrize("kind", SURFACES)
@pytest.mark.parametrize("ni", SHAPES)
def test_rock_fraction_equals_the_restatement_bit_for_bit(jr, h, reference, ni, kind):
    grid = _grid(jr, ni)
    assert grid._di["center"][2] == 1.0 / D
    hs, want = reference(ni, kind)
    topo = _topo(jr, ni, hs)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    for rows in (0, 1, 3, 2 ** 31 - 1):          # the built-in depth of a thread's march along k, a thread per node, a depth that does not divide nz + 1, the whole column
        h.set_option("rock_fraction3d_rows", rows)
        for k in TP.MEMBERS:
            getattr(ϕ, k).fill_(SENTINEL)
        before = _counters(h)
        jr.compute_rock_fraction_(ϕ, topo, grid, handle=h)
        assert _counters(h) == (before[0] + 1, before[1], before[2])
        for k in TP.MEMBERS:
            got = jr.to_numpy(getattr(ϕ, k))
            assert got.shape == TP.member_shape(k, ni)
            assert not np.any(got == SENTINEL), f"ϕ.{k}: {int((got == SENTINEL).sum())} entries were not written (rows = {rows})"
            assert np.array_equal(got, want[k]), (k, rows, float(np.abs(got - want[k]).max()))
            assert got.min() >= 0.0 and got.max() <= 1.0
    h.set_option("rock_fraction3d_rows", 0)
    assert np.array_equal(jr.to_numpy(topo.h), hs) and float(topo.h_old.abs().max()) == 0.0
    if kind == "flat_face":
        K = ni[2] // 2 + 1 if ni[2] > 1 else 1
        c = jr.to_numpy(ϕ.center)
        assert np.all(c[:, :, :K] == 1.0) and np.all(c[:, :, K:] == 0.0) and np.all(jr.to_numpy(ϕ.Vz)[:, :, K] == (0.5 if K < ni[2] else 1.0))


# ---------------------------------------------------------------------------------------------- 2. advection
def _velocity(ni, seed, scale):
    nx, ny, nz = ni
    rng = np.random.default_rng(seed)
    return tuple(np.asfortranarray(rng.uniform(-scale, scale, s)) for s in ((nx + 1, ny + 2, nz + 2), (nx + 2, ny + 1, nz + 2), (nx + 2, ny + 2, nz + 1)))


@pytest.mark.parametrize("kind", ("tilt_xy", "saddle", "rough"))
@pytest.mark.parametrize("ni", SHAPES)
def test_advection_equals_the_restatement_bit_for_bit(jr, h, ni, kind):
    """random velocities of up to 2.5 cells per step (departure points clamp on all four sides, and interior ones cross cells); two steps, so that h_old is
    seen to be the input of the last one"""
    grid = _grid(jr, ni)
    _di = grid._di["center"]
    hs = _surface(kind, ni, seed=1)
    topo = _topo(jr, ni, hs)
    topo.h_old.fill_(SENTINEL)
    Vh = _velocity(ni, 5 + ni[0], 2.5 * D / DT)
    V = tuple(_up(v) for v in Vh)
    before = _counters(h)
    h1 = TP.advect_topography(hs, *Vh, ni, ORIGIN[2], *_di, DT)
    jr.advect_topography_(topo, V, grid, DT, handle=h)
    assert np.array_equal(jr.to_numpy(topo.h_old), hs) and np.array_equal(jr.to_numpy(topo.h), h1)
    h2 = TP.advect_topography(h1, *Vh, ni, ORIGIN[2], *_di, 0.5 * DT)
    jr.advect_topography_(topo, V, grid, 0.5 * DT, handle=h)
    assert np.array_equal(jr.to_numpy(topo.h_old), h1) and np.array_equal(jr.to_numpy(topo.h), h2)
    assert _counters(h) == (before[0], before[1] + 2, before[2])
    for v, vh in zip(V, Vh):
        assert np.array_equal(jr.to_numpy(v), vh)


def test_advection_closed_forms_on_the_device(jr, h):
    """zero velocity returns h bit for bit; a uniform velocity translates a plane; stokes.V is accepted as V"""
    ni = (5, 4, 3)
    nx, ny, nz = ni
    grid = _grid(jr, ni)
    hs = _surface("saddle", ni)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    topo = _topo(jr, ni, hs)
    jr.advect_topography_(topo, st.V, grid, DT, handle=h)
    assert np.array_equal(jr.to_numpy(topo.h), hs) and np.array_equal(jr.to_numpy(topo.h_old), hs)
    x, y = np.meshgrid(np.arange(nx + 1) * D, np.arange(ny + 1) * D, indexing="ij")
    lin = ORIGIN[2] + 1.0 * D + 0.25 * x - 0.5 * y
    topo.fill_(lin)
    st.V.Vx.fill_(1.0)
    st.V.Vy.fill_(0.5)
    st.V.Vz.fill_(0.75)
    jr.advect_topography_(topo, st.V, grid, DT, handle=h)
    got = jr.to_numpy(topo.h)
    want = DT * (0.75 - 0.25 * 1.0 + 0.5 * 0.5)
    assert np.abs((got - lin)[1:, 1:] - want).max() <= 8 * np.finfo(float).eps * np.abs(lin).max()


# ---------------------------------------------------------------------------------------------- 3. phase correction
def _phase_fields(ni, N, air, f, seed):
    """N fields in [0, 1]; about a third of the cells already carry 1 - f in the air field (left untouched), about a third have no rock at all, and the
    bottom cells of some columns are all air (they take the lowest non-air index)"""
    rng = np.random.default_rng(seed)
    c = [np.asfortranarray(rng.uniform(0.0, 1.0, ni)) for _ in range(N)]
    norock = rng.uniform(size=ni) < 0.3
    norock[::2, :, 0] = True
    for k in range(N):
        if k != air - 1:
            c[k][norock] = 0.0
    keep = rng.uniform(size=ni) < 0.33
    c[air - 1] = np.asfortranarray(np.where(keep, 1.0 - f, c[air - 1]))
    return c


@pytest.mark.parametrize("N,air", [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (8, 5)])
@pytest.mark.parametrize("ni", SHAPES)
def test_phase_correction_equals_the_restatement_bit_for_bit(jr, h, reference, ni, N, air):
    grid = _grid(jr, ni)
    _dz = grid._di["center"][2]
    hs, ref = reference(ni, SURFACES[(N + air + ni[0]) % len(SURFACES)])
    c = _phase_fields(ni, N, air, ref["center"], 77 + 10 * N + air + ni[0])
    want, wr = TP.update_phases_given_topography(c, hs, ni, ORIGIN[2], _dz, air)
    assert wr.any() or ni == (1, 1, 1)          # the single cell may be one of those that already carry 1 - f
    topo = _topo(jr, ni, hs)
    fields = tuple(_up(a) for a in c)
    before = _counters(h)
    jr.update_phases_given_topography_(fields, topo, grid, air, handle=h)
    assert _counters(h) == (before[0], before[1], before[2] + 1)
    for k in range(N):
        got = jr.to_numpy(fields[k])
        assert np.array_equal(got, want[k]), (k, float(np.abs(got - want[k]).max()))
        assert np.array_equal(got[~wr], c[k][~wr])
    assert np.array_equal(jr.to_numpy(topo.h), hs)
    if N > 1:
        total = sum(jr.to_numpy(f) for f in fields)
        assert not wr.any() or np.abs(total[wr] - 1.0).max() <= (N + 4) * np.finfo(float).eps          # one rounding per p_k, per product and per sum


# ---------------------------------------------------------------------------------------------- 4. refusals
def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _refused(h, name, *args, match):
    from justrelax_jl_amd import _lib
    before = _counters(h)
    with pytest.raises(_lib.JrxError, match=match) as e:
        h.call(name, *args)
    assert e.value.status == 4
    assert _counters(h) == before


def test_refusals_leave_the_outputs_and_the_counters_alone(jr, h):
    import torch
    ni = (5, 4, 3)
    nx, ny, nz = ni
    grid = _grid(jr, ni)
    hs = _surface("saddle", ni)
    topo = _topo(jr, ni, hs)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    members = [getattr(ϕ, k) for k in TP.MEMBERS]
    for m in members:
        m.fill_(SENTINEL)
    i64, f64, i32 = C.c_int64, C.c_double, C.c_int32
    z0, (_dx, _dy, _dz) = ORIGIN[2], grid._di["center"]
    inf, nan = float("inf"), float("nan")

    def rf(mem=members, th=topo.h, n=ni, z=z0, d=_dz):
        return [*(_ptr(m) for m in mem), _ptr(th), *(i64(q) for q in n), f64(z), f64(d)]
    fn = "jrx_compute_rock_fraction3d"
    for q, name in enumerate(TP.MEMBERS):
        _refused(h, fn, *rf(mem=[None if k == q else m for k, m in enumerate(members)]), match=f"{name} is NULL")
    _refused(h, fn, *rf(th=None), match="topo.h is NULL")
    for n in ((0, ny, nz), (nx, -1, nz), (nx, ny, 0)):
        _refused(h, fn, *rf(n=n), match="extents")
    _refused(h, fn, *rf(n=(1300, 1300, 1300)), match="2\\^31")
    _refused(h, fn, *rf(d=inf), match="finite")
    _refused(h, fn, *rf(z=nan), match="finite")
    _refused(h, fn, *rf(mem=members[:7] + [members[6]]), match="xz and ϕ.xy overlap")
    nc = nx * ny * nz
    big = torch.zeros(nc + (nx + 1) * (ny + 1), dtype=torch.float64, device=_dev())
    _refused(h, fn, *rf(mem=[big[:nc]] + members[1:], th=big[nc - 1:]), match="center overlaps topo.h")
    for m in members:
        assert bool((m == SENTINEL).all())

    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    topo.h_old.fill_(SENTINEL)

    def adv(a=topo.h, b=topo.h_old, vx=st.V.Vx, vy=st.V.Vy, vz=st.V.Vz, n=ni, z=z0, dx=_dx, dy=_dy, dz=_dz, dt=DT):
        return [_ptr(a), _ptr(b), _ptr(vx), _ptr(vy), _ptr(vz), *(i64(q) for q in n), f64(z), f64(dx), f64(dy), f64(dz), f64(dt)]
    fn = "jrx_advect_topography3d"
    _refused(h, fn, *adv(a=None), match="topo.h is NULL")
    _refused(h, fn, *adv(b=None), match="h_old is NULL")
    _refused(h, fn, *adv(vx=None), match="Vx is NULL")
    _refused(h, fn, *adv(vy=None), match="Vy is NULL")
    _refused(h, fn, *adv(vz=None), match="Vz is NULL")
    _refused(h, fn, *adv(n=(nx, 0, nz)), match="extents")
    _refused(h, fn, *adv(n=(nx, ny, 0)), match="extents")
    _refused(h, fn, *adv(n=(1289, 1289, 1289)), match="2\\^31")
    for kw in (dict(dt=nan), dict(dt=inf), dict(dx=inf), dict(dy=nan), dict(dz=-inf), dict(z=nan)):
        _refused(h, fn, *adv(**kw), match="finite")
    _refused(h, fn, *adv(b=topo.h), match="overlaps topo.h_old")
    _refused(h, fn, *adv(a=st.V.Vz), match="overlaps V.Vz")
    _refused(h, fn, *adv(b=st.V.Vy), match="h_old overlaps V.Vy")
    assert np.array_equal(jr.to_numpy(topo.h), hs) and bool((topo.h_old == SENTINEL).all())

    c = [np.asfortranarray(np.full(ni, 0.25)) for _ in range(3)]
    fields = [_up(a) for a in c]

    def ph(fs=fields, N=None, th=topo.h, n=ni, z=z0, d=_dz, air=2, null=False):
        pa = None if null else (C.c_void_p * max(len(fs), 1))(*(f.data_ptr() if f is not None else None for f in fs))
        return [pa, i32(len(fs) if N is None else N), _ptr(th), *(i64(q) for q in n), f64(z), f64(d), i32(air)]
    fn = "jrx_update_phases_topography3d"
    _refused(h, fn, *ph(null=True), match="phases is NULL")
    _refused(h, fn, *ph(fs=[fields[0], None, fields[2]]), match="phase field 2 is NULL")
    _refused(h, fn, *ph(th=None), match="topo.h is NULL")
    for air in (0, 4, -1):
        _refused(h, fn, *ph(air=air), match="air_phase")
    for N in (0, 9):
        _refused(h, fn, *ph(N=N, air=1), match="phase fields")
    _refused(h, fn, *ph(n=(0, 5, 3)), match="extents")
    _refused(h, fn, *ph(n=(nx, ny, -2)), match="extents")
    _refused(h, fn, *ph(n=(1289, 1289, 1289)), match="2\\^31")
    _refused(h, fn, *ph(d=nan), match="finite")
    _refused(h, fn, *ph(z=inf), match="finite")
    _refused(h, fn, *ph(fs=[fields[0], fields[1], fields[0]]), match="1 and 3 overlap")
    _refused(h, fn, *ph(fs=[fields[0], big[:nc], fields[2]], th=big[nc - 1:]), match="phase field 2 overlaps topo.h")
    for f, a in zip(fields, c):
        assert np.array_equal(jr.to_numpy(f), a)


# ---------------------------------------------------------------------------------------------- 5. the Python checks
def test_python_checks_dimension_mismatch_nonuniform_grids_and_wrong_shapes(jr, h):
    ni3, ni2 = (5, 4, 3), (5, 3)
    g3, st3 = _grid(jr, ni3), jr.StokesArrays(jr.AMDGPUBackend, ni3)
    g2 = jr.Geometry(ni2, (5 * D, 3 * D), origin=(0.0, 0.0))
    st2 = jr.StokesArrays(jr.AMDGPUBackend, ni2)
    t3, t2 = jr.Topography(jr.AMDGPUBackend, ni3[:2]), jr.Topography(jr.AMDGPUBackend, 5)
    assert t3._ni == (5, 4) and tuple(t3.h.shape) == tuple(t3.h_old.shape) == (6, 5)
    assert jr.Topography(jr.AMDGPUBackend, (5,))._ni == (5,) and t2._ni == (5,) and tuple(t2.h.shape) == (6,)
    for bad in ((5, 4, 3), (0, 4), (5, 2.0), "5", ()):
        with pytest.raises(TypeError):
            jr.Topography(jr.AMDGPUBackend, bad)
    ϕ3, ϕ2 = jr.RockRatio(jr.AMDGPUBackend, ni3), jr.RockRatio(jr.AMDGPUBackend, ni2)
    f3, f2 = (jr.fzeros(ni3, _dev()), jr.fzeros(ni3, _dev(), 1.0)), (jr.fzeros(ni2, _dev()), jr.fzeros(ni2, _dev(), 1.0))
    before = _counters(h)
    mixed = [lambda: jr.compute_rock_fraction_(ϕ3, t2, g2, handle=h), lambda: jr.compute_rock_fraction_(ϕ3, t3, g2, handle=h),
             lambda: jr.compute_rock_fraction_(ϕ3, t2, g3, handle=h), lambda: jr.compute_rock_fraction_(ϕ2, t3, g3, handle=h),
             lambda: jr.compute_rock_fraction_(ϕ2, t2, g3, handle=h), lambda: jr.compute_rock_fraction_(ϕ2, t3, g2, handle=h),
             lambda: jr.update_phases_given_topography_(f3, t2, g2, 2, handle=h), lambda: jr.update_phases_given_topography_(f3, t2, g3, 2, handle=h),
             lambda: jr.update_phases_given_topography_(f2, t3, g3, 2, handle=h), lambda: jr.update_phases_given_topography_(f2, t3, g2, 2, handle=h),
             lambda: jr.advect_topography_(t2, st3.V, g3, DT, handle=h), lambda: jr.advect_topography_(t3, st2.V, g2, DT, handle=h),
             lambda: jr.advect_topography_(t3, st2.V, g3, DT, handle=h), lambda: jr.advect_topography_(t2, st3.V, g2, DT, handle=h)]
    for call in mixed:
        with pytest.raises(NotImplementedError):
            call()
    nonuni = jr.Geometry.from_vertices((np.linspace(0, 1, 6) ** 2, np.linspace(0, 1, 5), np.linspace(0, 1, 4)))
    for call in (lambda: jr.compute_rock_fraction_(ϕ3, t3, nonuni, handle=h), lambda: jr.advect_topography_(t3, st3.V, nonuni, DT, handle=h),
                 lambda: jr.update_phases_given_topography_(f3, t3, nonuni, 2, handle=h)):
        with pytest.raises(NotImplementedError):
            call()
    other = _grid(jr, (5, 4, 4))
    wrong = [lambda: jr.compute_rock_fraction_(ϕ3, t3, other, handle=h), lambda: jr.compute_rock_fraction_(ϕ3, jr.Topography(jr.AMDGPUBackend, (4, 4)), g3, handle=h),
             lambda: jr.advect_topography_(t3, st3.V, other, DT, handle=h), lambda: jr.advect_topography_(t3, (st3.V.Vx, st3.V.Vz, st3.V.Vy), g3, DT, handle=h),
             lambda: jr.update_phases_given_topography_(f3, t3, other, 2, handle=h), lambda: jr.update_phases_given_topography_((), t3, g3, 1, handle=h),
             lambda: t3.fill_(np.zeros(6)), lambda: t3.fill_(np.zeros((5, 6)))]
    for call in wrong:
        with pytest.raises(ValueError):
            call()
    assert _counters(h) == before
    with pytest.raises(ValueError):
        jr.compute_rock_fraction_(ϕ3, t3, object(), handle=h)


# ---------------------------------------------------------------------------------------------- 6. conversions
def test_a_3d_topography_converts_and_checkpoints_like_the_other_containers(jr, tmp_path):
    ni = (5, 4, 3)
    hs = _surface("saddle", ni)
    old = np.asfortranarray(hs[::-1, ::-1].copy())
    topo = _topo(jr, ni, hs)
    topo.h_old.copy_(_up(old))
    host = jr.Array_(topo)
    assert np.array_equal(host.h, hs) and np.array_equal(host.h_old, old) and host._ni == (5, 4)
    back = jr.PTArray_(jr.AMDGPUBackend, host)
    assert isinstance(back, jr.Topography) and back._ni == (5, 4) and np.array_equal(jr.to_numpy(back.h), hs) and np.array_equal(jr.to_numpy(back.h_old), old)
    twin = jr.copy_(topo)
    assert isinstance(twin, jr.Topography) and twin.h.data_ptr() != topo.h.data_ptr() and np.array_equal(jr.to_numpy(twin.h), hs)
    assert np.array_equal(jr.to_numpy(twin.h_old), old)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    jr.checkpointing_npz(str(tmp_path), st, None, 1.5, 0.25, topo=topo)
    again = jr.PTArray_(jr.AMDGPUBackend, jr.load_checkpoint_extra_npz(str(tmp_path), "topo"))
    assert isinstance(again, jr.Topography) and again._ni == (5, 4)
    assert np.array_equal(jr.to_numpy(again.h), hs) and np.array_equal(jr.to_numpy(again.h_old), old)
    # the converted object is a working operand: the rock fractions from it are those of the original
    grid = _grid(jr, ni)
    ϕa, ϕb = jr.RockRatio(jr.AMDGPUBackend, ni), jr.RockRatio(jr.AMDGPUBackend, ni)
    jr.compute_rock_fraction_(ϕa, topo, grid)
    jr.compute_rock_fraction_(ϕb, again, grid)
    assert all(np.array_equal(jr.to_numpy(getattr(ϕa, k)), jr.to_numpy(getattr(ϕb, k))) for k in TP.MEMBERS)


# ---------------------------------------------------------------------------------------------- 7. the rock fractions in the 3D variational solve
STATE = ("P", "V.Vx", "V.Vy", "V.Vz", "τ.xx", "τ.yy", "τ.zz", "τ.xy", "τ.xz", "τ.yz", "τ.II", "viscosity.η", "R.RP", "R.Rx", "R.Ry", "R.Rz")


def _get(o, path):
    for p in path.split("."):
        o = getattr(o, p)
    return o


def _solve(jr, ni, ϕ_from, s_surface):
    """a dense visco-elastic layer under sticky air in pure shear; binary phase fields, the air above the flat surface (cell units)"""
    nx, ny, nz = ni
    dev = _dev()
    jr.finalize_global_grid()
    li = tuple(n / 32.0 for n in ni)
    grid = jr.Geometry(ni, li, origin=(0.0, 0.0, 0.0))
    di = grid.di["center"]
    phases = [dict(eta=1.0, G=1.0, Kb=4.0, g=1.0, density=dict(kind="constant", rho0=1.0)),
              dict(eta=1.0e-2, G=1.0, Kb=4.0, density=dict(kind="constant", rho0=1.0e-3))]
    air = 2
    hs = np.full((nx + 1, ny + 1), s_surface * di[2])
    topo = _topo(jr, ni, hs)
    f = TP.compute_rock_fraction(hs, ni, 0.0, grid._di["center"][2], members=("center",))["center"]
    assert np.all((f == 0.0) | (f == 1.0))
    fields = (_up(f), _up(1.0 - f))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    jr.update_phase_ratios_3D_(pr, fields, grid)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    if ϕ_from == "topography":
        jr.compute_rock_fraction_(ϕ, topo, grid)
    else:
        jr.update_rock_ratio_(ϕ, pr, air)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    xv, yv, zv = grid.xvi
    st.V.Vx.copy_(_up(xv[:, None, None] * np.ones((1, ny + 2, nz + 2))))
    st.V.Vz.copy_(_up(-zv[None, None, :] * np.ones((nx + 2, ny + 2, 1))))
    faces = ("left", "right", "top", "bot", "front", "back")
    bcs = jr.VelocityBoundaryConditions(free_slip={k: True for k in faces}, no_slip={k: False for k in faces})
    jr.flow_bcs_(st, bcs)
    ρg = tuple(jr.fzeros(ni, dev) for _ in range(3))
    args = dict(T=jr.fzeros(tuple(m + 2 for m in ni), dev, 1.0), P=st.P)
    jr.compute_ρg_(ρg, pr, phases, args)
    cutoff = (1.0e-2, 1.0e2)
    jr.compute_viscosity_(st, pr, None, phases, cutoff, air_phase=air)
    pt = jr.PTStokesCoeffs(li, di, ϵ_rel=1.0e-30, ϵ_abs=1.0e-30, CFL=0.75 / np.sqrt(3.1))
    r = jr.solve_VariationalStokes_(st, pt, grid, bcs, ρg, pr, ϕ, phases, None, 0.25, None,
                                    kwargs=dict(iterMax=39, nout=20, verbose=False, viscosity_cutoff=cutoff, air_phase=air))
    return r, {k: jr.to_numpy(_get(st, k)) for k in STATE}, {k: jr.to_numpy(getattr(ϕ, k)) for k in TP.MEMBERS}


def test_rock_fractions_drive_the_3d_variational_solve(jr):
    """(6, 5, 4), binary phase fields, a flat surface on the face k = 3.  ϕ.center is the same from compute_rock_fraction_ and from update_rock_ratio_, bit for
    bit.  The other seven members are printed; what the CPU restatement shows is asserted: on this surface every member of operator 1 is 1 below the face, 0
    above it and 0.5 in the vertex row of the face (tests/test_topography3d_restatement.py, flat surfaces), and update_rock_ratio_ interpolates the binary
    ratios to the same 1, 0 and 0.5 -- the largest difference measured is 0 in every member, as in 2D, so the two short solves leave bit-identical state."""
    ni = (6, 5, 4)
    r1, a1, ϕ1 = _solve(jr, ni, "topography", 3.0)
    r2, a2, ϕ2 = _solve(jr, ni, "phase_ratios", 3.0)
    diff = {k: float(np.abs(ϕ1[k] - ϕ2[k]).max()) for k in TP.MEMBERS}
    print("largest |compute_rock_fraction! - update_rock_ratio!| per member:", diff)
    assert np.array_equal(ϕ1["center"], ϕ2["center"]) and 0.0 < ϕ1["center"].mean() < 1.0
    want = TP.compute_rock_fraction(np.full((7, 6), 3.0), ni, 0.0, 1.0)
    for k in TP.MEMBERS:
        assert np.array_equal(ϕ1[k], want[k]), k
    for k, a in a1.items():
        assert np.all(np.isfinite(a)), k
    assert float(np.abs(a1["V.Vz"]).max()) > 0.0
    # tests/test_topography3d_restatement.py::test_flat_face_surface_gives_the_members_of_update_rock_ratio shows the difference 0 in all eight members
    assert all(v == 0.0 for v in diff.values()), diff
    assert r1.iter == r2.iter >= 39
    for k in a1:
        assert np.array_equal(a1[k], a2[k]), k
    assert list(r1.err_evo1) == list(r2.err_evo1)
