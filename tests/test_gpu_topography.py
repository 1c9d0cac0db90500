"""GPU: the 2D free-surface operators (compute_rock_fraction_, advect_topography_, update_phases_given_topography_; csrc/topography.hip through
jrx_compute_rock_fraction2d, jrx_advect_topography2d, jrx_update_phases_topography2d) against the NumPy restatement (tests/_topography.py): every member bit
for bit (np.array_equal -- the kernels have no fma and the library is built without contraction), the inputs untouched, sentinel-filled outputs fully written,
every refusal with the counters unchanged, and the rock fractions feeding solve_VariationalStokes_.

Sizes: (3, 3); (6, 5); (67, 35) crosses a wave in x and a block in y; (130, 9) has more columns than one block of the column kernels holds.
The refusal at 2^31 entries is exercised with the extents alone: it comes before anything is read, so the small arrays passed along are never touched."""
import ctypes as C

import numpy as np
import pytest

import _topography as TP

pytestmark = pytest.mark.gpu
SHAPES = [(3, 3), (6, 5), (67, 35), (130, 9)]
SURFACES = ("sine", "sawtooth", "flat", "random")
SENTINEL = -7.0e30
DY = 2.0 ** -3
ORIGIN = (0.25, -0.5)
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
    return jr.Geometry(ni, (ni[0] * DY, ni[1] * DY), origin=ORIGIN)


def _surface(kind, ni, seed=0):
    """heights in cell units"""
    nx, ny = ni
    i = np.arange(nx + 1)
    if kind == "sine":          # amplitude 2.5 cells on a ramp that leaves the box at both ends
        s = 0.5 * ny + 2.5 * np.sin(2 * np.pi * i / nx) + (0.5 * ny + 1.0) * (2 * i / nx - 1)
    elif kind == "sawtooth":    # slopes steeper than one cell per cell
        s = 0.5 * ny + np.where(i % 2 == 0, -1.75, 1.5) + 0.01 * i
    elif kind == "flat":        # on a face
        s = np.full(nx + 1, float(ny // 2 + 1))
    else:                       # multiples of 2^-9 in -2 .. ny + 2: adjacent heights differ by 0 or by at least 1.9e-3 cells; every third segment is flat
        rng = np.random.default_rng(20261020 + seed + nx)
        s = rng.integers(-2 * 512, (ny + 2) * 512, nx + 1) / 512.0
        s[1::3] = s[0:-1:3][: len(s[1::3])]
        d = np.abs(np.diff(s))
        assert np.all((d == 0) | (d >= 1e-3)) and (d == 0).any()
    return ORIGIN[1] + s * DY


def _topo(jr, ni, hs):
    t = jr.Topography(jr.AMDGPUBackend, ni[0])
    t.fill_(hs)
    return t


def _counters(h):
    return tuple(h.get_option(k) for k in COUNTERS)


# ---------------------------------------------------------------------------------------------- 1. rock fractions
@pytest.mark.parametrize("kind", SURFACES)
@pytest.mark.parametrize("ni", SHAPES)
def test_rock_fraction_equals_the_restatement_bit_for_bit(jr, h, ni, kind):
    grid = _grid(jr, ni)
    hs = _surface(kind, ni)
    topo = _topo(jr, ni, hs)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    for k in TP.MEMBERS:
        getattr(ϕ, k).fill_(SENTINEL)
    before = _counters(h)
    jr.compute_rock_fraction_(ϕ, topo, grid, handle=h)
    assert _counters(h) == (before[0] + 1, before[1], before[2])
    want = TP.compute_rock_fraction(hs, ni, ORIGIN[1], grid._di["center"][1])
    for k in TP.MEMBERS:
        got = jr.to_numpy(getattr(ϕ, k))
        assert got.shape == TP.member_shape(k, ni)
        assert not np.any(got == SENTINEL), f"ϕ.{k}: {int((got == SENTINEL).sum())} entries were not written"
        assert np.array_equal(got, want[k]), (k, float(np.abs(got - want[k]).max()))
        assert got.min() >= 0.0 and got.max() <= 1.0
    assert np.array_equal(jr.to_numpy(topo.h), hs) and float(topo.h_old.abs().max()) == 0.0
    if kind == "flat":
        J = ni[1] // 2 + 1
        c = jr.to_numpy(ϕ.center)
        assert np.all(c[:, :J] == 1.0) and np.all(c[:, J:] == 0.0) and np.all(jr.to_numpy(ϕ.Vy)[:, J] == 0.5)


# ---------------------------------------------------------------------------------------------- 2. advection
def _velocity(ni, seed, scale):
    nx, ny = ni
    rng = np.random.default_rng(seed)
    return (np.asfortranarray(rng.uniform(-scale, scale, (nx + 1, ny + 2))), np.asfortranarray(rng.uniform(-scale, scale, (nx + 2, ny + 1))))


@pytest.mark.parametrize("kind", SURFACES)
@pytest.mark.parametrize("ni", SHAPES)
def test_advection_equals_the_restatement_bit_for_bit(jr, h, ni, kind):
    """random velocities of up to 2.5 cells per step (departure points clamp at both ends, and interior ones cross cells); two steps, so that h_old is
    seen to be the input of the last one"""
    grid = _grid(jr, ni)
    _dx, _dy = grid._di["center"]
    hs = _surface(kind, ni, seed=1)
    topo = _topo(jr, ni, hs)
    topo.h_old.fill_(SENTINEL)
    Vx, Vy = _velocity(ni, 5 + ni[0], 2.5 * DY / DT)
    V = (_up(Vx), _up(Vy))
    before = _counters(h)
    h1 = TP.advect_topography(hs, Vx, Vy, ni, ORIGIN[1], _dx, _dy, DT)
    jr.advect_topography_(topo, V, grid, DT, handle=h)
    assert np.array_equal(jr.to_numpy(topo.h_old), hs) and np.array_equal(jr.to_numpy(topo.h), h1)
    h2 = TP.advect_topography(h1, Vx, Vy, ni, ORIGIN[1], _dx, _dy, 0.5 * DT)
    jr.advect_topography_(topo, V, grid, 0.5 * DT, handle=h)
    assert np.array_equal(jr.to_numpy(topo.h_old), h1) and np.array_equal(jr.to_numpy(topo.h), h2)
    assert _counters(h) == (before[0], before[1] + 2, before[2])
    assert np.array_equal(jr.to_numpy(V[0]), Vx) and np.array_equal(jr.to_numpy(V[1]), Vy)


def test_advection_closed_forms_on_the_device(jr, h):
    """zero velocity returns h bit for bit; a uniform velocity translates a linear surface exactly; stokes.V is accepted as V"""
    ni = (67, 35)
    nx, ny = ni
    grid = _grid(jr, ni)
    hs = _surface("sine", ni)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    topo = _topo(jr, ni, hs)
    jr.advect_topography_(topo, st.V, grid, DT, handle=h)
    assert np.array_equal(jr.to_numpy(topo.h), hs) and np.array_equal(jr.to_numpy(topo.h_old), hs)
    x = np.arange(nx + 1) * DY
    lin = ORIGIN[1] + 2.0 * DY + 0.25 * x
    topo.fill_(lin)
    st.V.Vx.fill_(1.0)
    st.V.Vy.fill_(0.5)
    jr.advect_topography_(topo, st.V, grid, DT, handle=h)
    got = jr.to_numpy(topo.h)
    assert np.array_equal(got[1:], (ORIGIN[1] + 2.0 * DY + 0.25 * (x - DT) + 0.5 * DT)[1:]) and got[0] == lin[0] + 0.5 * DT


# ---------------------------------------------------------------------------------------------- 3. phase correction
def _phase_fields(ni, N, air, hs, _dy, seed):
    """N fields in [0, 1]; about a third of the cells already carry 1 - f in the air field (left untouched), a band of cells has no rock at all, and the
    bottom cells of some columns are all air (they take the lowest non-air index)"""
    nx, ny = ni
    rng = np.random.default_rng(seed)
    f = TP.compute_rock_fraction(hs, ni, ORIGIN[1], _dy)["center"]
    c = [np.asfortranarray(rng.uniform(0.0, 1.0, ni)) for _ in range(N)]
    norock = rng.uniform(size=ni) < 0.3
    norock[::2, 0] = True
    for k in range(N):
        if k != air - 1:
            c[k][norock] = 0.0
    keep = rng.uniform(size=ni) < 0.33
    c[air - 1] = np.asfortranarray(np.where(keep, 1.0 - f, c[air - 1]))
    return c


@pytest.mark.parametrize("N,air", [(1, 1), (2, 2), (3, 1), (4, 3), (8, 8)])
@pytest.mark.parametrize("ni", SHAPES)
def test_phase_correction_equals_the_restatement_bit_for_bit(jr, h, ni, N, air):
    grid = _grid(jr, ni)
    _dy = grid._di["center"][1]
    hs = _surface(SURFACES[(N + ni[0]) % 4], ni, seed=2)
    c = _phase_fields(ni, N, air, hs, _dy, 77 + N + ni[0])
    want, wr = TP.update_phases_given_topography(c, hs, ni, ORIGIN[1], _dy, air)
    assert wr.any() and (N == 1 or not wr.all())
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
        assert np.abs(total[wr] - 1.0).max() <= (N + 4) * np.finfo(float).eps          # one rounding per p_k, per product and per sum


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
    ni = (6, 5)
    nx, ny = ni
    grid = _grid(jr, ni)
    hs = _surface("sine", ni)
    topo = _topo(jr, ni, hs)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    members = [ϕ.center, ϕ.vertex, ϕ.Vx, ϕ.Vy]
    for m in members:
        m.fill_(SENTINEL)
    i64, f64, i32 = C.c_int64, C.c_double, C.c_int32
    y0, (_dx, _dy) = ORIGIN[1], grid._di["center"]
    inf, nan = float("inf"), float("nan")

    def rf(mem=members, th=topo.h, n=(nx, ny), y=y0, d=_dy):
        return [*(_ptr(m) for m in mem), _ptr(th), i64(n[0]), i64(n[1]), f64(y), f64(d)]
    for q, name in enumerate(("center", "vertex", "Vx", "Vy")):
        _refused(h, "jrx_compute_rock_fraction2d", *rf(mem=[None if k == q else m for k, m in enumerate(members)]), match=f"{name} is NULL")
    _refused(h, "jrx_compute_rock_fraction2d", *rf(th=None), match="topo.h is NULL")
    _refused(h, "jrx_compute_rock_fraction2d", *rf(n=(0, ny)), match="extents")
    _refused(h, "jrx_compute_rock_fraction2d", *rf(n=(nx, -1)), match="extents")
    _refused(h, "jrx_compute_rock_fraction2d", *rf(n=(50000, 50000)), match="2\\^31")
    _refused(h, "jrx_compute_rock_fraction2d", *rf(d=inf), match="finite")
    _refused(h, "jrx_compute_rock_fraction2d", *rf(y=nan), match="finite")
    _refused(h, "jrx_compute_rock_fraction2d", *rf(mem=[ϕ.center, ϕ.vertex, ϕ.Vx, ϕ.Vx]), match="Vx and ϕ.Vy overlap")
    big = torch.zeros(nx * ny + nx + 1, dtype=torch.float64, device=_dev())
    _refused(h, "jrx_compute_rock_fraction2d", *rf(mem=[big[:nx * ny], ϕ.vertex, ϕ.Vx, ϕ.Vy], th=big[nx * ny - 1:]), match="center overlaps topo.h")
    for m in members:
        assert bool((m == SENTINEL).all())

    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    topo.h_old.fill_(SENTINEL)

    def adv(a=topo.h, b=topo.h_old, vx=st.V.Vx, vy=st.V.Vy, n=(nx, ny), y=y0, dx=_dx, dy=_dy, dt=DT):
        return [_ptr(a), _ptr(b), _ptr(vx), _ptr(vy), i64(n[0]), i64(n[1]), f64(y), f64(dx), f64(dy), f64(dt)]
    _refused(h, "jrx_advect_topography2d", *adv(a=None), match="topo.h is NULL")
    _refused(h, "jrx_advect_topography2d", *adv(b=None), match="h_old is NULL")
    _refused(h, "jrx_advect_topography2d", *adv(vx=None), match="Vx is NULL")
    _refused(h, "jrx_advect_topography2d", *adv(vy=None), match="Vy is NULL")
    _refused(h, "jrx_advect_topography2d", *adv(n=(nx, 0)), match="extents")
    _refused(h, "jrx_advect_topography2d", *adv(n=(46341, 46341)), match="2\\^31")
    for kw in (dict(dt=nan), dict(dt=inf), dict(dx=inf), dict(dy=nan)):
        _refused(h, "jrx_advect_topography2d", *adv(**kw), match="finite")
    _refused(h, "jrx_advect_topography2d", *adv(b=topo.h), match="overlaps topo.h_old")
    _refused(h, "jrx_advect_topography2d", *adv(a=st.V.Vx), match="overlaps V.Vx")
    assert np.array_equal(jr.to_numpy(topo.h), hs) and bool((topo.h_old == SENTINEL).all())

    c = [np.asfortranarray(np.full(ni, 0.25)) for _ in range(3)]
    fields = [_up(a) for a in c]

    def ph(fs=fields, N=None, th=topo.h, n=(nx, ny), y=y0, d=_dy, air=2, null=False):
        pa = None if null else (C.c_void_p * max(len(fs), 1))(*(f.data_ptr() if f is not None else None for f in fs))
        return [pa, i32(len(fs) if N is None else N), _ptr(th), i64(n[0]), i64(n[1]), f64(y), f64(d), i32(air)]
    _refused(h, "jrx_update_phases_topography2d", *ph(null=True), match="phases is NULL")
    _refused(h, "jrx_update_phases_topography2d", *ph(fs=[fields[0], None, fields[2]]), match="phase field 2 is NULL")
    _refused(h, "jrx_update_phases_topography2d", *ph(th=None), match="topo.h is NULL")
    for air in (0, 4, -1):
        _refused(h, "jrx_update_phases_topography2d", *ph(air=air), match="air_phase")
    for N in (0, 9):
        _refused(h, "jrx_update_phases_topography2d", *ph(N=N, air=1), match="phase fields")
    _refused(h, "jrx_update_phases_topography2d", *ph(n=(0, 5)), match="extents")
    _refused(h, "jrx_update_phases_topography2d", *ph(d=nan), match="finite")
    _refused(h, "jrx_update_phases_topography2d", *ph(fs=[fields[0], fields[1], fields[0]]), match="1 and 3 overlap")
    for f, a in zip(fields, c):
        assert np.array_equal(jr.to_numpy(f), a)

    # the Python layer: a 3D RockRatio and a non-uniform Geometry are not built
    with pytest.raises(NotImplementedError):
        jr.compute_rock_fraction_(jr.RockRatio(jr.AMDGPUBackend, (4, 4, 4)), topo, grid, handle=h)
    nonuni = jr.Geometry.from_vertices((np.linspace(0, 1, nx + 1) ** 2, np.linspace(0, 1, ny + 1)))
    for call in (lambda: jr.compute_rock_fraction_(ϕ, topo, nonuni, handle=h), lambda: jr.advect_topography_(topo, st.V, nonuni, DT, handle=h),
                 lambda: jr.update_phases_given_topography_(fields, topo, nonuni, 2, handle=h)):
        with pytest.raises(NotImplementedError):
            call()


def test_topography_converts_and_checkpoints_like_the_other_containers(jr, tmp_path):
    ni = (6, 5)
    hs = _surface("sine", ni)
    topo = _topo(jr, ni, hs)
    topo.h_old.copy_(_up(hs[::-1].copy()))
    host = jr.Array_(topo)
    assert np.array_equal(host.h, hs) and np.array_equal(host.h_old, hs[::-1]) and host._ni == (6,)
    back = jr.PTArray_(jr.AMDGPUBackend, host)
    assert isinstance(back, jr.Topography) and np.array_equal(jr.to_numpy(back.h), hs) and np.array_equal(jr.to_numpy(back.h_old), hs[::-1])
    twin = jr.copy_(topo)
    assert isinstance(twin, jr.Topography) and twin.h.data_ptr() != topo.h.data_ptr() and np.array_equal(jr.to_numpy(twin.h), hs)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    jr.checkpointing_npz(str(tmp_path), st, None, 1.5, 0.25, topo=topo)
    tree = jr.load_checkpoint_extra_npz(str(tmp_path), "topo")
    again = jr.PTArray_(jr.AMDGPUBackend, tree)
    assert isinstance(again, jr.Topography) and np.array_equal(jr.to_numpy(again.h), hs) and np.array_equal(jr.to_numpy(again.h_old), hs[::-1])
    assert jr.load_checkpoint_extra_npz(str(tmp_path), "absent") is None
    with pytest.raises(ValueError):
        topo.fill_(np.zeros(3))


# ---------------------------------------------------------------------------------------------- 5. the rock fractions in the variational solve
STATE = ("P", "V.Vx", "V.Vy", "τ.xx", "τ.yy", "τ.xy", "τ.xy_c", "τ.II", "ε.xx", "ε.yy", "ε.xy", "viscosity.η", "viscosity.η_vep", "R.RP", "R.Rx", "R.Ry", "divV")


def _get(o, path):
    for p in path.split("."):
        o = getattr(o, p)
    return o


def _solve(jr, ni, ϕ_from, s_surface):
    """a dense visco-elastic layer under sticky air in pure shear; the air above the surface (cell units).  ϕ_from: "topography" or "phase_ratios" """
    import torch
    nx, ny = ni
    dev = _dev()
    jr.finalize_global_grid()
    li = (nx / 32.0, ny / 32.0)
    grid = jr.Geometry(ni, li, origin=(0.0, 0.0))
    di = grid.di["center"]
    phases = [dict(eta=1.0, G=1.0, Kb=4.0, g=1.0, density=dict(kind="constant", rho0=1.0)),
              dict(eta=1.0e-2, G=1.0, Kb=4.0, density=dict(kind="constant", rho0=1.0e-3))]
    air = 2
    hs = np.full(nx + 1, s_surface * di[1])
    topo = _topo(jr, ni, hs)
    f = TP.compute_rock_fraction(hs, ni, 0.0, grid._di["center"][1])["center"]
    fields = (_up(f), _up(1.0 - f))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    jr.update_phase_ratios_2D_(pr, fields, grid)
    ϕ = jr.RockRatio(jr.AMDGPUBackend, ni)
    if ϕ_from == "topography":
        jr.compute_rock_fraction_(ϕ, topo, grid)
    else:
        jr.update_rock_ratio_(ϕ, pr, air)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    xv, yv = grid.xvi
    st.V.Vx.copy_(_up(xv[:, None] * np.ones((1, ny + 2))))
    st.V.Vy.copy_(_up(-yv[None, :] * np.ones((nx + 2, 1))))
    bcs = jr.VelocityBoundaryConditions(free_slip={k: True for k in ("left", "right", "top", "bot")}, no_slip={k: False for k in ("left", "right", "top", "bot")})
    jr.flow_bcs_(st, bcs)
    ρg = (jr.fzeros(ni, dev), jr.fzeros(ni, dev))
    args = dict(T=jr.fzeros(tuple(m + 2 for m in ni), dev, 1.0), P=st.P)
    jr.compute_ρg_(ρg, pr, phases, args)
    cutoff = (1.0e-2, 1.0e2)
    jr.compute_viscosity_(st, pr, None, phases, cutoff, air_phase=air)
    pt = jr.PTStokesCoeffs(li, di, ϵ_rel=1.0e-30, ϵ_abs=1.0e-30, CFL=0.75 / np.sqrt(2.1))
    r = jr.solve_VariationalStokes_(st, pt, grid, bcs, ρg, pr, ϕ, phases, None, 0.25, None,
                                    kwargs=dict(iterMax=59, nout=20, verbose=False, viscosity_cutoff=cutoff, air_phase=air))
    return r, {k: jr.to_numpy(_get(st, k)) for k in STATE}, {k: jr.to_numpy(getattr(ϕ, k)) for k in TP.MEMBERS}


def test_rock_fractions_drive_the_variational_solve(jr):
    """(32, 24), a flat surface on the face j = 18: the solve on ϕ from compute_rock_fraction_ returns (status 0: no exception) with finite fields, and -- ϕ.center
    being the same from either route and the other three members agreeing too on this surface -- the same bits as the solve on ϕ from update_rock_ratio_.
    With a mid-cell surface (18.5) the solve returns finite fields and the norms over the valid nodes."""
    ni = (32, 24)
    r1, a1, ϕ1 = _solve(jr, ni, "topography", 18.0)
    r2, a2, ϕ2 = _solve(jr, ni, "phase_ratios", 18.0)
    assert r1.iter == r2.iter == 60
    for k, a in a1.items():
        assert np.all(np.isfinite(a)), k
    assert np.array_equal(ϕ1["center"], ϕ2["center"]) and 0.0 < ϕ1["center"].mean() < 1.0
    agree = all(np.array_equal(ϕ1[k], ϕ2[k]) for k in ("vertex", "Vx", "Vy"))
    print("vertex, Vx, Vy from the two routes agree:", agree)
    assert agree, "measured on this surface: the interpolated ratios equal the area fractions (include/jrx.h)"
    for k in a1:
        assert np.array_equal(a1[k], a2[k]), k
    assert list(r1.err_evo1) == list(r2.err_evo1) and list(r1.norm_Rx) == list(r2.norm_Rx)
    assert float(np.abs(a1["V.Vy"]).max()) > 0.0 and np.all(a1["P"][:, 18:] == 0.0)
    r3, a3, ϕ3 = _solve(jr, ni, "topography", 18.5)
    assert np.all(ϕ3["center"][:, 18] == 0.5) and np.all(ϕ3["Vy"][:, 19] == 0.0)
    for k, a in a3.items():
        assert np.all(np.isfinite(a)), k
    for name in ("err_evo1", "norm_Rx", "norm_Ry", "norm_divV"):
        v = np.asarray(getattr(r3, name))
        assert len(v) == 3 and np.all(np.isfinite(v)), name
