"""GPU: the per-step operators of csrc/stepops.hip (pureshear_bc_, free_surface_bcs_, subgrid_characteristic_time_, compute_melt_fraction_) against their
NumPy restatements (tests/_stepops.py, pinned by tests/test_stepops_restatement.py), in 2D at (9, 7) and in 3D at (9, 7, 5), two phases with different
parameters, random positive inputs from fixed seeds, every output pre-filled with the sentinel -77.25.

Which comparison applies: pureshear_bc_, free_surface_bcs_ and subgrid_characteristic_time_ are chains of +, -, *, / that the kernels write in the
reference's grouping; the library is built without fma contraction and each of those operations is correctly rounded on both sides, so they are compared
BIT FOR BIT (np.array_equal).  compute_melt_fraction_ calls exp, which is not the same function bit for bit in two math libraries, so it is held to the
project's standing rule (tests/test_gpu_dyrel.py): 16 x the largest float64-against-longdouble difference of the restatement, relative to the max-norm."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import _stepops as SO

pytestmark = pytest.mark.gpu
S = SO.SENTINEL
NI = {2: (9, 7), 3: (9, 7, 5)}
PHASES = [dict(eta=1.0, G=1.3, Kb=2.0, k=3.0, Cp=1.0e3, density=dict(kind="PT", rho0=3.0e3, alpha=3.0e-5, beta=1.0e-11, T0=273.0), melting=dict(kind="caricchi", a=800.0)),
          dict(eta=1.0, G=0.4, Kb=2.0, k=1.7, Cp=1.25e3, density=dict(kind="constant", rho0=2.7e3), melting=dict(kind="caricchi", a=900.0, b=31.0))]
PHASES5 = PHASES + [dict(eta=1.0, G=0.9, Kb=2.0, k=2.2, Cp=0.9e3, density=dict(kind="constant", rho0=3.3e3)),
                    dict(eta=1.0, G=2.1, Kb=2.0, k=4.0, Cp=1.1e3, density=dict(kind="constant", rho0=2.9e3), melting=dict(kind="caricchi", a=700.0, c=270.0)),
                    dict(eta=1.0, G=0.7, Kb=2.0, k=2.9, Cp=1.2e3, density=dict(kind="PT", rho0=3.1e3, alpha=2.0e-5, beta=0.0, T0=300.0), melting=dict(kind="caricchi"))]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _up(a):
    from justrelax_jl_amd.arrays import from_numpy
    return from_numpy(np.asarray(a, dtype=np.float64), _dev())


def _dn(t):
    from justrelax_jl_amd.arrays import to_numpy
    return to_numpy(t)


@pytest.fixture(scope="module")
def h():
    from justrelax_jl_amd import _lib
    return _lib.Handle(_dev().index)


def _launches(h):
    return h.get_option("stat_stepops_launches")


def _ratios(ni, nph, rng):
    """(nph, ni...) ratios: random and summing to one, with cells that are exactly one phase (the isone / iszero branches of fn_ratio)"""
    r = rng.uniform(0.05, 1.0, (nph,) + ni)
    r /= r.sum(axis=0)
    flat = r.reshape(nph, -1)
    pure = rng.permutation(flat.shape[1])[: 3 * nph]
    for n, c in enumerate(pure):
        flat[:, c] = 0.0
        flat[n % nph, c] = 1.0
    return flat.reshape((nph,) + ni)


def _vel_shapes(ni):
    if len(ni) == 2:
        nx, ny = ni
        return dict(Vx=(nx + 1, ny + 2), Vy=(nx + 2, ny + 1))
    nx, ny, nz = ni
    return dict(Vx=(nx + 1, ny + 2, nz + 2), Vy=(nx + 2, ny + 1, nz + 2), Vz=(nx + 2, ny + 2, nz + 1))


def _stokes(jr, ni, host):
    """a StokesArrays carrying the host arrays Vx, Vy[, Vz], P, P0, toyy[, tozz], eta"""
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    for k in _vel_shapes(ni):
        getattr(st.V, k).copy_(_up(host[k]))
    for k, t in (("P", st.P), ("P0", st.P0), ("toyy", st.τ_o.yy), ("eta", st.viscosity.η)):
        t.copy_(_up(host[k]))
    if len(ni) == 3:
        st.τ_o.zz.copy_(_up(host["tozz"]))
    return st


def _phase_ratios(jr, nph, ni, r):
    pr = jr.PhaseRatios(jr.AMDGPUBackend, nph, ni)
    pr.center.copy_(_up(r))
    return pr


def _close(name, got, f64, ld):
    scale = float(np.max(np.abs(f64))) or 1.0
    bound = 16.0 * float(np.max(np.abs(f64.astype(np.longdouble) - ld))) / scale
    err = float(np.max(np.abs(got - f64))) / scale
    print(f"{name}: |gpu - f64| = {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound, (name, err, bound)


# ----------------------------------------------------------------------------------------------------------------------------------------- pureshear_bc_
@pytest.mark.parametrize("nd", (2, 3))
def test_pureshear_bc_equals_the_restatement_and_leaves_the_ghosts(jr, h, nd):
    """bit for bit: one multiply per entry.  Non-uniform vertices, handed over as host vectors (uploaded) and as device vectors"""
    rng = np.random.default_rng(100 + nd)
    ni, εbg = NI[nd], 0.73
    xvi = tuple(np.sort(rng.uniform(-1.0, 2.0, n + 1)) for n in ni)
    xci = tuple((x[:-1] + x[1:]) / 2 for x in xvi)
    want = {k: np.full(s, S) for k, s in _vel_shapes(ni).items()}
    (SO.pureshear_bc2d if nd == 2 else SO.pureshear_bc3d)(*want.values(), xci, xvi, εbg)
    for device_vectors in (False, True):
        st = jr.StokesArrays(jr.AMDGPUBackend, ni)
        for k in want:
            getattr(st.V, k).fill_(S)
        n0 = _launches(h)
        jr.pureshear_bc_(st, xci, tuple(_up(x) for x in xvi) if device_vectors else xvi, εbg, jr.AMDGPUBackend, handle=h)
        assert _launches(h) == n0 + 1                                   # one launch for all components
        for k in want:
            got = _dn(getattr(st.V, k))
            assert np.array_equal(got, want[k]), k
            assert (got == S).sum() == (want[k] == S).sum() > 0, k     # the ghosts still hold the sentinel


def test_pureshear_bc_3d_equals_the_literal_text_on_coinciding_vertices(jr, h):
    rng = np.random.default_rng(110)
    ni = (4, 4, 3)
    xv = np.sort(rng.uniform(0.0, 1.0, 5))
    xvi = (xv, xv.copy(), np.sort(rng.uniform(0.0, 1.0, 4)))
    xci = tuple((x[:-1] + x[1:]) / 2 for x in xvi)
    want = {k: np.full(s, S) for k, s in _vel_shapes(ni).items()}
    SO.pureshear_bc3d_literal(*want.values(), xci, xvi, -0.6)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    for k in want:
        getattr(st.V, k).fill_(S)
    jr.pureshear_bc_(st, xci, xvi, -0.6, jr.AMDGPUBackend, handle=h)
    for k in want:
        assert np.array_equal(_dn(getattr(st.V, k)), want[k]), k


# ----------------------------------------------------------------------------------------------------------------------------------------- free_surface_bcs_
def _free_surface_state(nd, rng):
    """velocities: Vx[, Vy] random positive; the written array holds the sentinel except the two top interior rows / planes the law reads"""
    ni = NI[nd]
    host = {k: rng.uniform(0.1, 1.0, s) for k, s in _vel_shapes(ni).items()}
    out = "Vy" if nd == 2 else "Vz"
    v = np.full(host[out].shape, S)
    inner = (slice(1, -1),) * (nd - 1)
    v[inner + (slice(-2, None),)] = host[out][inner + (slice(-2, None),)]
    host[out] = v
    for k in ("P", "P0", "toyy", "tozz", "eta"):
        host[k] = rng.uniform(0.1, 1.0, ni) * (1.0e2 if k == "eta" else 1.0)
    host["phase_c"] = _ratios(ni, 2, rng)
    return ni, host, out


def _fs(jr, h, host, ni, bcs, dt, *di):
    st = _stokes(jr, ni, host)
    pr = _phase_ratios(jr, 2, ni, host["phase_c"])
    jr.free_surface_bcs_(st, bcs, st.viscosity.η, PHASES, pr, dt, *di, handle=h)
    return st, pr


def _bcs(jr, on):
    return jr.VelocityBoundaryConditions(free_surface=on)


@pytest.mark.parametrize("spacing", ("scalars", "vectors"))
def test_free_surface_bcs_2d(jr, h, spacing):
    """bit for bit: the kernel keeps the reference's grouping, no fma.  Only Vy[2:end-1, end] changes; with spacing vectors dx is read at [i], dy at [end]"""
    rng = np.random.default_rng(200)
    ni, host, _ = _free_surface_state(2, rng)
    dt = 0.37
    if spacing == "scalars":
        dx, dy = 0.21, 0.13
        di = ((dx, 9.9), (9.9, dy))                      # _di_vx[2] and _di_vy[1] are never read
    else:
        dx, dy = rng.uniform(0.1, 0.3, ni[0]), rng.uniform(0.1, 0.3, ni[1])
        di = ((dx, 9.9), (9.9, _up(dy)))
    want = {k: v.copy() for k, v in host.items()}
    SO.free_surface_bcs2d(want, [p["G"] for p in PHASES], dt, dx, dy)
    n0 = _launches(h)
    st, pr = _fs(jr, h, host, ni, _bcs(jr, True), dt, *di)
    assert _launches(h) == n0 + 1
    got = _dn(st.V.Vy)
    assert np.array_equal(got, want["Vy"])
    changed = got != host["Vy"]
    assert changed[1:-1, -1].all() and changed.sum() == ni[0]
    for k, t in (("Vx", st.V.Vx), ("P", st.P), ("P0", st.P0), ("toyy", st.τ_o.yy), ("eta", st.viscosity.η), ("phase_c", pr.center)):
        assert np.array_equal(_dn(t), host[k]), k


def test_free_surface_bcs_3d_follows_tau_o_yy(jr, h):
    """bit for bit, as in 2D.  Only Vz[2:end-1, 2:end-1, end] changes.  τ_o.yy and τ_o.zz hold different fields: the law reads τ_o.yy (the reference's text,
    kept), and swapping the two changes the result"""
    rng = np.random.default_rng(300)
    ni, host, _ = _free_surface_state(3, rng)
    dt, di = 0.37, (0.21, 0.13, 0.34)
    G = [p["G"] for p in PHASES]
    want = {k: v.copy() for k, v in host.items()}
    SO.free_surface_bcs3d(want, G, dt, di)
    st, pr = _fs(jr, h, host, ni, _bcs(jr, True), dt, di)
    got = _dn(st.V.Vz)
    assert np.array_equal(got, want["Vz"])
    changed = got != host["Vz"]
    assert changed[1:-1, 1:-1, -1].all() and changed.sum() == ni[0] * ni[1]
    for k, t in (("Vx", st.V.Vx), ("Vy", st.V.Vy), ("P", st.P), ("P0", st.P0), ("toyy", st.τ_o.yy), ("tozz", st.τ_o.zz), ("eta", st.viscosity.η)):
        assert np.array_equal(_dn(t), host[k]), k
    swapped = dict(host, toyy=host["tozz"], tozz=host["toyy"])
    st2, _ = _fs(jr, h, swapped, ni, _bcs(jr, True), dt, di)
    want_zz = {k: v.copy() for k, v in host.items()}
    SO.free_surface_bcs3d(want_zz, G, dt, di, stress="tozz")
    assert np.array_equal(_dn(st2.V.Vz), want_zz["Vz"]) and not np.array_equal(_dn(st2.V.Vz), got)


@pytest.mark.parametrize("nd", (2, 3))
def test_free_surface_bcs_without_the_flag_launches_nothing(jr, h, nd):
    rng = np.random.default_rng(400 + nd)
    ni, host, out = _free_surface_state(nd, rng)
    di = ((0.2, 0.2), (0.2, 0.2)) if nd == 2 else ((0.2, 0.2, 0.2),)
    n0 = _launches(h)
    st, pr = _fs(jr, h, host, ni, _bcs(jr, False), 0.5, *di)
    assert _launches(h) == n0
    for k in _vel_shapes(ni):
        assert np.array_equal(_dn(getattr(st.V, k)), host[k]), k
    for k, t in (("P", st.P), ("P0", st.P0), ("toyy", st.τ_o.yy), ("eta", st.viscosity.η), ("phase_c", pr.center)):
        assert np.array_equal(_dn(t), host[k]), k
    jr.free_surface_bcs_(st, _bcs(jr, True), st.viscosity.η, PHASES, pr, 0.5, *di, handle=h)
    assert _launches(h) == n0 + 1 and not np.array_equal(_dn(getattr(st.V, out)), host[out])


# ----------------------------------------------------------------------------------------------------------------------------------------- subgrid_characteristic_time_
@pytest.mark.parametrize("nd,phases", ((2, PHASES), (3, PHASES), (3, PHASES5)), ids=("2d", "3d", "3d-five-phases"))
def test_subgrid_characteristic_time(jr, h, nd, phases):
    """bit for bit: products, sums and one division in the reference's grouping, no fma.  Five phases run the kernel with the run-time phase count"""
    rng = np.random.default_rng(500 + nd + len(phases))
    ni = NI[nd]
    di = (0.5, 0.25, 0.125)[:nd]
    T = rng.uniform(300.0, 1600.0, tuple(n + 2 for n in ni))
    P = rng.uniform(1.0e5, 1.0e9, ni)
    r = _ratios(ni, len(phases), rng)
    want = SO.subgrid_characteristic_time(r, phases, T, P, di)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    st.P.copy_(_up(P))
    th = jr.ThermalArrays(jr.AMDGPUBackend, ni)
    th.T.copy_(_up(T))
    pr = _phase_ratios(jr, len(phases), ni, r)
    dt0 = jr.fzeros(ni, _dev(), S)
    n0 = _launches(h)
    jr.subgrid_characteristic_time_(dt0, pr, phases, th, st, di, handle=h)
    assert _launches(h) == n0 + 1
    got = _dn(dt0)
    assert np.all(got > 0) and np.array_equal(got, want)
    assert np.array_equal(_dn(th.T), T) and np.array_equal(_dn(st.P), P) and np.array_equal(_dn(pr.center), r)


def test_subgrid_characteristic_time_constant_material_is_exact(jr, h):
    ni = (9, 7)
    st, th, pr = jr.StokesArrays(jr.AMDGPUBackend, ni), jr.ThermalArrays(jr.AMDGPUBackend, ni), jr.PhaseRatios(jr.AMDGPUBackend, 1, ni)
    pr.center.fill_(1.0)
    dt0 = jr.fzeros(ni, _dev(), S)
    jr.subgrid_characteristic_time_(dt0, pr, dict(k=3.0, Cp=1.0e3, density=dict(kind="constant", rho0=3.0e3)), th, st, (0.5, 0.5), handle=h)
    assert np.all(_dn(dt0) == 62500.0)


# ----------------------------------------------------------------------------------------------------------------------------------------- compute_melt_fraction_
@pytest.mark.parametrize("nd,phases", ((2, PHASES), (3, PHASES), (3, PHASES5)), ids=("2d", "3d", "3d-five-phases"))
def test_compute_melt_fraction_phase_ratio_form(jr, h, nd, phases):
    """by the tolerance rule (exp): 16 x the float64-against-longdouble spread of the restatement, relative to the max-norm"""
    rng = np.random.default_rng(600 + nd + len(phases))
    ni = NI[nd]
    T = rng.uniform(950.0, 1350.0, ni)                       # across the melting interval of both laws
    P = rng.uniform(1.0e5, 1.0e9, ni)
    r = _ratios(ni, len(phases), rng)
    f64 = SO.compute_melt_fraction(ni, r, phases, T)
    ld = SO.compute_melt_fraction(ni, r, phases, T.astype(np.longdouble), dtype=np.longdouble)
    pr = _phase_ratios(jr, len(phases), ni, r)
    ϕ = jr.fzeros(ni, _dev(), S)
    Td, Pd = _up(T), _up(P)
    n0 = _launches(h)
    jr.compute_melt_fraction_(ϕ, pr, phases, dict(T=Td, P=Pd), handle=h)
    assert _launches(h) == n0 + 1
    got = _dn(ϕ)
    assert np.all((got >= 0) & (got <= 1)) and got.max() - got.min() > 0.3
    _close(f"melt fraction {nd}D, {len(phases)} phases", got, f64, ld)
    assert np.array_equal(_dn(Td), T) and np.array_equal(_dn(Pd), P) and np.array_equal(_dn(pr.center), r)


@pytest.mark.parametrize("nd", (2, 3))
def test_compute_melt_fraction_single_material_and_its_identities(jr, h, nd):
    rng = np.random.default_rng(700 + nd)
    ni = NI[nd]
    T = rng.uniform(950.0, 1350.0, ni)
    f64 = SO.compute_melt_fraction(ni, None, PHASES, T)
    ld = SO.compute_melt_fraction(ni, None, PHASES, T.astype(np.longdouble), dtype=np.longdouble)
    single = jr.fzeros(ni, _dev(), S)
    jr.compute_melt_fraction_(single, PHASES, SimpleNamespace(T=_up(T), P=1.0e8), handle=h)
    _close(f"melt fraction {nd}D, single material", _dn(single), f64, ld)
    # the phase-ratio form with ratios (1, 0) is the single-material form of phase 1, bit for bit
    r = np.zeros((2,) + ni)
    r[0] = 1.0
    ratio = jr.fzeros(ni, _dev(), S)
    jr.compute_melt_fraction_(ratio, _phase_ratios(jr, 2, ni, r), PHASES, dict(T=_up(T), P=1.0e8), handle=h)
    assert np.array_equal(_dn(ratio), _dn(single))
    # T as a number gives the bits of T as a constant array
    a, b = jr.fzeros(ni, _dev(), S), jr.fzeros(ni, _dev(), S)
    jr.compute_melt_fraction_(a, PHASES, dict(T=1234.5, P=1.0e8), handle=h)
    jr.compute_melt_fraction_(b, PHASES, dict(T=_up(np.full(ni, 1234.5)), P=_up(np.full(ni, 1.0e8))), handle=h)
    assert np.array_equal(_dn(a), _dn(b)) and np.all(_dn(a) == _dn(a).flat[0]) and 0.0 < _dn(a).flat[0] < 1.0
    # the reference's own bounds (test/test_rheology.jl:246-252)
    jr.compute_melt_fraction_(a, dict(melting=dict(kind="caricchi")), dict(T=1373.15, P=1.0e8), handle=h)
    jr.compute_melt_fraction_(b, dict(melting=dict(kind="caricchi")), dict(T=573.15, P=1.0e8), handle=h)
    assert np.all((0.95 < _dn(a)) & (_dn(a) < 1.0)) and np.all((1.5e-10 < _dn(b)) & (_dn(b) < 6.0e-10))
    jr.compute_melt_fraction_(a, dict(melting=None), dict(T=1373.15, P=1.0e8), handle=h)
    assert np.all(_dn(a) == 0.0)


def test_compute_melt_fraction_refuses_a_law_it_does_not_build(jr, h):
    from justrelax_jl_amd import _lib
    ni = NI[2]
    ϕ = jr.fzeros(ni, _dev(), S)
    n0 = _launches(h)
    for phases in ([dict(melting=dict(kind=2))], [dict(melting=dict(kind="caricchi")), dict(melting=dict(kind=-1))]):
        pr = _phase_ratios(jr, len(phases), ni, _ratios(ni, len(phases), np.random.default_rng(1)))
        with pytest.raises(_lib.JrxError, match="melting") as e:
            jr.compute_melt_fraction_(ϕ, pr, phases, dict(T=1200.0, P=0.0), handle=h)
        assert e.value.status == 4
    assert _launches(h) == n0 and np.all(_dn(ϕ) == S)


# ----------------------------------------------------------------------------------------------------------------------------------------- shapes and the C ABI
def test_shapes_that_do_not_fit_raise_before_any_call(jr, h):
    ni = NI[2]
    st, th = jr.StokesArrays(jr.AMDGPUBackend, ni), jr.ThermalArrays(jr.AMDGPUBackend, ni)
    pr2, pr3 = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni), jr.PhaseRatios(jr.AMDGPUBackend, 3, ni)
    g = jr.Geometry(ni, (1.0, 1.0))
    ϕ, small = jr.fzeros(ni, _dev(), S), jr.fzeros((ni[0], ni[1] - 1), _dev(), S)
    di2 = ((0.2, 0.2), (0.2, 0.2))
    on = _bcs(jr, True)
    n0 = _launches(h)
    calls = [lambda: jr.pureshear_bc_(st, g.xci, (g.xvi[0][:-1], g.xvi[1]), 1.0, jr.AMDGPUBackend, handle=h),
             lambda: jr.pureshear_bc_(st, (g.xci[0], g.xci[1][1:]), g.xvi, 1.0, jr.AMDGPUBackend, handle=h),
             lambda: jr.pureshear_bc_(st, g.xci + (g.xci[0],), g.xvi + (g.xvi[0],), 1.0, jr.AMDGPUBackend, handle=h),
             lambda: jr.free_surface_bcs_(st, on, st.viscosity.η, PHASES, pr3, 0.5, *di2, handle=h),
             lambda: jr.free_surface_bcs_(st, on, small, PHASES, pr2, 0.5, *di2, handle=h),
             lambda: jr.free_surface_bcs_(st, on, st.viscosity.η, PHASES, pr2, 0.5, ((np.full(ni[0] + 1, 0.2), 0.2), (0.2, 0.2)), handle=h),
             lambda: jr.free_surface_bcs_(st, on, st.viscosity.η, PHASES, pr2, 0.5, (0.2, 0.2, 0.2), handle=h),
             lambda: jr.subgrid_characteristic_time_(small, pr2, PHASES, th, st, (0.2, 0.2), handle=h),
             lambda: jr.subgrid_characteristic_time_(ϕ, pr3, PHASES, th, st, (0.2, 0.2), handle=h),
             lambda: jr.subgrid_characteristic_time_(ϕ, pr2, PHASES, th, st, (0.2, 0.2, 0.2), handle=h),
             lambda: jr.subgrid_characteristic_time_(ϕ, pr2, PHASES, SimpleNamespace(T=st.P), st, (0.2, 0.2), handle=h),
             lambda: jr.compute_melt_fraction_(ϕ, PHASES, dict(T=small, P=0.0), handle=h),
             lambda: jr.compute_melt_fraction_(ϕ, PHASES, dict(T=1000.0, P=small), handle=h),
             lambda: jr.compute_melt_fraction_(ϕ, pr3, PHASES, dict(T=1000.0, P=0.0), handle=h)]
    for n, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {n} was accepted")
    assert _launches(h) == n0 and np.all(_dn(ϕ) == S) and not np.any(_dn(st.V.Vx))


def test_c_abi_refuses_bad_arguments_with_status_4(jr, h):
    """JRX_ERR_ARG with a text naming the cause, nothing launched: NULL pointers, empty extents, 2^31 entries, bad spacings, overlapping arrays"""
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.arrays import ptr
    from justrelax_jl_amd.stepops import melting_table
    from justrelax_jl_amd.stokes import rheology_table
    from justrelax_jl_amd.thermal import thermal_phases
    ni = NI[2]
    st, th, pr = jr.StokesArrays(jr.AMDGPUBackend, ni), jr.ThermalArrays(jr.AMDGPUBackend, ni), jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    ϕ = jr.fzeros(ni, _dev(), S)
    xv, yv = _up(np.linspace(0, 1, ni[0] + 1)), _up(np.linspace(0, 1, ni[1] + 1))
    p = lambda *ts: [C.c_void_p(ptr(t)) for t in ts]
    i64 = lambda *ns: [C.c_int64(n) for n in ns]
    d = lambda *xs: [C.c_double(x) for x in xs]
    rh, tp, mt = rheology_table(PHASES), thermal_phases(PHASES, SimpleNamespace(max_lxyz=1.0, Vpdτ=1.0)), melting_table(PHASES)
    n3 = lambda *n: (C.c_int64 * 3)(*n)
    d3 = lambda *x: (C.c_double * 3)(*x)
    fs = lambda **kw: ["jrx_free_surface_bcs2d", *p(kw.get("Vx", st.V.Vx), st.V.Vy, st.P, st.P0, st.τ_o.yy, kw.get("eta", st.viscosity.η), pr.center), C.byref(rh),
                       *d(kw.get("dt", 0.5), kw.get("dx", 0.2), 0.2), *p(None, None), *i64(*kw.get("n", ni)), C.c_int32(1)]
    bad = [(["jrx_pureshear_bc2d", *p(st.V.Vx, None, xv, yv), *d(1.0), *i64(*ni)], "NULL"),
           (["jrx_pureshear_bc2d", *p(st.V.Vx, st.V.Vy, xv, yv), *d(1.0), *i64(0, 7)], "ni"),
           (["jrx_pureshear_bc2d", *p(st.V.Vx, st.V.Vy, xv, yv), *d(1.0), *i64(1 << 16, 1 << 15)], "2\\^31"),
           (["jrx_pureshear_bc2d", *p(st.V.Vx, st.V.Vx, xv, yv), *d(1.0), *i64(*ni)], "overlap"),
           (["jrx_pureshear_bc3d", *p(st.V.Vx, st.V.Vy, st.V.Vy, xv, yv, yv), *d(1.0), *i64(1 << 11, 1 << 10, 1 << 10)], "2\\^31"),
           (fs(dt=0.0), "dt"), (fs(dx=float("nan")), "spacings"), (fs(n=(1 << 16, 1 << 15)), "2\\^31"), (fs(eta=st.V.Vy), "overlaps"),
           (["jrx_subgrid_characteristic_time", *p(ϕ, pr.center), C.byref(tp), *p(th.T, st.P), n3(*ni, 1), C.c_int32(2), d3(0.2, -1.0, 1.0)], "di\\[2\\]"),
           (["jrx_subgrid_characteristic_time", *p(ϕ, pr.center), C.byref(tp), *p(th.T, st.P), n3(1 << 11, 1 << 10, 1 << 10), C.c_int32(3), d3(0.2, 0.2, 0.2)], "2\\^31"),
           (["jrx_subgrid_characteristic_time", *p(ϕ, pr.center), C.byref(tp), *p(th.T, ϕ), n3(*ni, 1), C.c_int32(2), d3(0.2, 0.2, 1.0)], "overlaps"),
           (["jrx_compute_melt_fraction", *p(ϕ, pr.center), C.byref(mt), *p(None), *d(1000.0), *p(None), *d(0.0), n3(1 << 16, 1 << 15, 1), C.c_int32(2)], "2\\^31"),
           (["jrx_compute_melt_fraction", *p(ϕ, None), C.byref(mt), *p(ϕ), *d(1000.0), *p(None), *d(0.0), n3(*ni, 1), C.c_int32(2)], "overlaps"),
           (["jrx_compute_melt_fraction", *p(ϕ, None), C.byref(mt), *p(None), *d(1000.0), *p(None), *d(0.0), n3(*ni, 1), C.c_int32(4)], "ndim")]
    n0 = _launches(h)
    for args, match in bad:
        with pytest.raises(_lib.JrxError, match=match) as e:
            h.call(*args)
        assert e.value.status == 4, args[0]
    assert _launches(h) == n0 and np.all(_dn(ϕ) == S) and not np.any(_dn(st.V.Vx)) and not np.any(_dn(st.V.Vy))
