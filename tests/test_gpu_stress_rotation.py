"""GPU: grid-based stress rotation and advection (rotate_stress_; csrc/stress_rotation.hip through jrx_rotate_stress2d / 3d) against the NumPy restatement
(tests/_stress_rotation.py): random fields and velocities for every method x advection, every entry written, the inputs untouched; the closed-form cases of
tests/test_stress_rotation_restatement.py on the device; |w| == 0 nodes; NULL velocities without advection; every refusal with the outputs untouched; and
rotate_stress_ on the StokesArrays a solve leaves behind.

Bounds.  "jaumann" and "none": 1e-13 max|τ| absolute, the project's bound for device arithmetic against NumPy (the kernel has no fma, so these legs are
expected to agree to the last bit or two).  "matrix", |θ| <= 1: the same bound, which did not need widening.  Measured on one MI355X over the parity cases
below (each case prints its figure): "matrix" at most 2.2e-16 max|τ| in 2D and 4.4e-16 in 3D (device sincos against NumPy's), "jaumann" 0 in 2D and at most
2.2e-16 in 3D.
The refusal at 2^31 entries is not exercised (it would need arrays of 16 GiB)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _stress_rotation as SR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "justrelax.jl_amd" / "csrc" / "stress_rotation.hip").read_text()
TX, TY2, TY3, TZ3 = (int(re.search(rf"\b{k} = (\d+)", SRC).group(1)) for k in ("kRsTX", "kRsTY2", "kRsTY3", "kRsTZ3"))
# a single cell, odd primes, and one node more than the kernel's own tile in every direction (more than one block along every dimension)
SHAPES = [(1, 1), (7, 5), (TX + 1, TY2 + 1), (1, 1, 1), (5, 3, 2), (TX + 1, TY3 + 1, TZ3 + 1)]
SENTINEL = 1.0e30
BOUND = 1e-13          # x max|τ|, absolute
_DI = (0.7, 1.3, 0.9)
DT = 0.5               # |θ| = dt |w| <= 0.5 sqrt(3) < 1 for ω in [-1, 1]
MEASURED = {}          # (ndim, method, advection) -> the largest deviation / max|τ| seen by test_parity_with_the_restatement, printed by each case


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


def _members(nd, optional=False):
    return (SR.MEMBERS2_OPT if optional else SR.MEMBERS2) if nd == 2 else SR.MEMBERS3


def _stokes(jr, ni, τ, ω, V):
    """a StokesArrays holding the state, τ_o pre-filled with the sentinel (xx_v, yy_v allocated in both tensors only when τ has them)"""
    nd = len(ni)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    for k, a in τ.items():
        getattr(st.τ, k).copy_(_up(a))
        getattr(st.τ_o, k).fill_(SENTINEL)
    if nd == 2:
        st.ω.xy.copy_(_up(ω))
    else:
        for k, a in ω.items():
            getattr(st.ω, k).copy_(_up(a))
    if V is not None:
        for name, a in zip(("Vx", "Vy", "Vz"), V):
            getattr(st.V, name).copy_(_up(a))
    return st


def _unchanged(jr, st, τ, ω, V):
    nd = len(st._ni)
    ok = all(np.array_equal(jr.to_numpy(getattr(st.τ, k)), a) for k, a in τ.items())
    ok = ok and (np.array_equal(jr.to_numpy(st.ω.xy), ω) if nd == 2 else all(np.array_equal(jr.to_numpy(getattr(st.ω, k)), a) for k, a in ω.items()))
    if V is not None:
        ok = ok and all(np.array_equal(jr.to_numpy(getattr(st.V, name)), a) for name, a in zip(("Vx", "Vy", "Vz"), V))
    return ok


def _untouched(st, keys):
    return all(bool((getattr(st.τ_o, k) == SENTINEL).all()) for k in keys)


def _run(jr, h, ni, τ, ω, V, dt, method, advection, grid=None):
    st = _stokes(jr, ni, τ, ω, V)
    grid = grid or tuple(1.0 / d for d in _DI[:len(ni)])
    if not isinstance(grid, jr.Geometry):
        jr.finalize_global_grid()                                   # the legacy di tuple: its Geometry takes the global extents of an initialised grid
    jr.rotate_stress_(st, grid, dt, method=method, advection=advection, handle=h)
    got = {k: jr.to_numpy(getattr(st.τ_o, k)) for k in τ}
    assert _unchanged(jr, st, τ, ω, V), "an input was written"
    for k, a in got.items():
        assert not np.any(a == SENTINEL), f"τ_o.{k}: {int((a == SENTINEL).sum())} entries were not written"
    return got


def _deviation(got, ref, τ):
    scale = max(float(np.abs(a).max()) for a in τ.values())
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape, k
    return max(float(np.abs(got[k] - ref[k]).max()) for k in ref) / scale


@pytest.mark.parametrize("advection", SR.ADVECTIONS)
@pytest.mark.parametrize("method", SR.METHODS)
@pytest.mark.parametrize("ni", SHAPES)
def test_parity_with_the_restatement(jr, h, ni, method, advection):
    nd = len(ni)
    optional = nd == 2 and ni != (7, 5)                                 # the 2D kernels with and without the vertex normals
    τ, ω, V = SR.random_state(ni, 20261019 + sum(ni), optional=optional)
    calls = h.get_option("stat_rotate_stress_calls")
    got = _run(jr, h, ni, τ, ω, V, DT, method, advection)
    assert h.get_option("stat_rotate_stress_calls") == calls + 1
    ref = SR.rotate_stress(τ, ω, V, ni, _DI[:nd], DT, method, advection)
    d = _deviation(got, ref, τ)
    key = (nd, method, advection)
    MEASURED[key] = max(MEASURED.get(key, 0.0), d)
    print(f"rotate_stress {ni} {method} {advection}: largest deviation / max|τ| = {d:.3e} (largest so far for {key}: {MEASURED[key]:.3e})")
    assert d <= BOUND


@pytest.mark.parametrize("ni", [(7, 5), (5, 3, 2)])
def test_geometry_and_spacing_tuple_give_the_same_bits(jr, h, ni):
    nd = len(ni)
    τ, ω, V = SR.random_state(ni, 31)
    li = tuple(n / d for n, d in zip(ni, _DI))
    a = _run(jr, h, ni, τ, ω, V, DT, "matrix", "upwind", grid=jr.Geometry(ni, li))
    b = _run(jr, h, ni, τ, ω, V, DT, ":matrix", ":upwind")              # the Julia spelling of the symbols
    assert _deviation(a, b, τ) <= BOUND                                 # the two routes may round 1 / (l / n) differently in the last bit
    assert _deviation(a, SR.rotate_stress(τ, ω, V, ni, _DI[:nd], DT), τ) <= BOUND


@pytest.mark.parametrize("ni,Ω", [((7, 5), 0.9), ((5, 3, 2), (0.3, -0.5, 0.7))])
def test_uniform_tensor_under_rigid_rotation(jr, h, ni, Ω):
    """every member, boundary nodes included, equals the analytic R τ R'; ω comes from the library's own compute_vorticity!"""
    nd = len(ni)
    li = (2.0, 1.0, 0.7)[:nd]
    dt = 0.8
    V = SR.rigid_velocity(ni, li, Ω, centre=tuple(0.5 * l for l in li))
    vals = dict(xx=0.8, yy=-0.5, zz=-0.3, yz=0.35, xz=-0.15, xy=0.6)
    τ = {k: np.full(SR.shape_at(loc, ni), vals[k[:2]]) for k, loc in _members(nd, optional=True).items()}
    grid = jr.Geometry(ni, li)
    st = _stokes(jr, ni, τ, np.zeros(SR.shape_at(SR.VERTEX2, ni)) if nd == 2 else {k: np.zeros(SR.shape_at(loc, ni)) for k, loc in SR.OMEGA3.items()}, V)
    jr.compute_vorticity_(st, grid, handle=h)
    jr.rotate_stress_(st, grid, dt, handle=h)
    if nd == 2:
        R = SR.rotation_matrix((0.0, 0.0, Ω), dt)[:2, :2]
        want = dict(zip(("xx", "yy", "xy"), SR.voigt(R @ SR.tensor((vals["xx"], vals["yy"], vals["xy"])) @ R.T)))
    else:
        R = SR.rotation_matrix(Ω, dt)
        names = ("xx", "yy", "zz", "yz", "xz", "xy")
        want = dict(zip(names, SR.voigt(R @ SR.tensor([vals[k] for k in names]) @ R.T)))
    for k in τ:
        assert np.abs(jr.to_numpy(getattr(st.τ_o, k)) - want[k[:2]]).max() <= 1e-12 * 0.8, k
    # N steps of θ / N equal one step of θ
    one = {k: jr.to_numpy(getattr(st.τ_o, k)) for k in τ}
    N = 8
    for _ in range(N):
        jr.rotate_stress_(st, grid, dt / N, handle=h)
        for k in τ:
            getattr(st.τ, k).copy_(getattr(st.τ_o, k))
    for k in τ:
        assert np.abs(jr.to_numpy(getattr(st.τ_o, k)) - one[k]).max() <= 1e-12 * 0.8, k


@pytest.mark.parametrize("method", SR.METHODS)
@pytest.mark.parametrize("advection", SR.ADVECTIONS)
def test_plane_strain_3d_equals_2d_layer_by_layer(jr, h, method, advection):
    from test_stress_rotation_restatement import _plane_strain
    ni2, nz = (5, 3), 2
    (τ2, ω2, V2), (τ3, ω3, V3) = _plane_strain(ni2, nz, 6)
    o2 = _run(jr, h, ni2, τ2, ω2, V2, 0.1, method, advection)
    o3 = _run(jr, h, ni2 + (nz,), τ3, ω3, V3, 0.1, method, advection)
    scale = max(float(np.abs(a).max()) for a in τ2.values())
    for k in ("xx", "yy", "xy_c", "xy"):
        for layer in range(nz):
            assert np.abs(o3[k][:, :, layer] - o2[k]).max() <= BOUND * scale, (k, layer)
    assert np.array_equal(o3["zz"], τ3["zz"])
    for k in ("yz", "xz", "yz_c", "xz_c"):
        assert np.all(o3[k] == 0.0), k


@pytest.mark.parametrize("ni", [(7, 5), (5, 3, 2)])
@pytest.mark.parametrize("method", SR.METHODS)
def test_nodes_without_vorticity_among_rotating_ones(jr, h, ni, method):
    """|w| == 0 at every other node: R = I there without a division -- no NaN, and the restatement's numbers"""
    nd = len(ni)
    τ, ω, V = SR.random_state(ni, 41, optional=nd == 2)
    rng = np.random.default_rng(42)
    if nd == 2:
        ω = ω * (rng.uniform(size=ω.shape) < 0.5)
    else:
        mask = {k: rng.uniform(size=a.shape) < 0.5 for k, a in ω.items()}
        ω = {k: a * mask[k] for k, a in ω.items()}
        ω["yz"][0, :, :] = ω["xz"][:2, :, :] = ω["xy"][:2, :, :] = 0.0      # whole neighbourhoods of zeros: the first centres and edges see |w| == 0 exactly
    got = _run(jr, h, ni, τ, ω, V, DT, method, "none")
    assert all(np.isfinite(a).all() for a in got.values())
    assert _deviation(got, SR.rotate_stress(τ, ω, None, ni, None, DT, method, "none"), τ) <= BOUND
    zero = np.zeros_like(ω) if nd == 2 else {k: np.zeros_like(a) for k, a in ω.items()}
    same = _run(jr, h, ni, τ, zero, V, DT, method, "none")              # case 4 of the CPU list: the input bits in every member
    for k in τ:
        assert np.array_equal(same[k], τ[k]), k


def test_optional_vertex_normals_only_when_both_tensors_have_them(jr, h):
    ni = (7, 5)
    τ, ω, V = SR.random_state(ni, 51, optional=True)
    st = _stokes(jr, ni, {k: τ[k] for k in SR.MEMBERS2}, ω, V)
    st.τ.xx_v.copy_(_up(τ["xx_v"]))
    st.τ.yy_v.copy_(_up(τ["yy_v"]))                                     # τ has them, τ_o does not: they are skipped and not allocated
    grid = jr.Geometry(ni, tuple(n / d for n, d in zip(ni, _DI)))
    jr.rotate_stress_(st, grid, DT, handle=h)
    assert "xx_v" not in st.τ_o.__dict__ and "yy_v" not in st.τ_o.__dict__
    ref = SR.rotate_stress(τ, ω, V, ni, _DI[:2], DT)
    for k in SR.MEMBERS2:
        assert np.abs(jr.to_numpy(getattr(st.τ_o, k)) - ref[k]).max() <= BOUND, k
    st.τ_o.xx_v.fill_(SENTINEL)
    st.τ_o.yy_v.fill_(SENTINEL)
    jr.rotate_stress_(st, grid, DT, handle=h)
    for k in ("xx_v", "yy_v"):
        assert np.abs(jr.to_numpy(getattr(st.τ_o, k)) - ref[k]).max() <= BOUND, k


# ---------------------------------------------------------------------------------------------- the C ABI: NULL velocities, refusals
def _c_call(h, st, *, tau=None, tau_o=None, omega=None, V="all", n=None, method=0, advection=1, optional=False, dt=DT):
    """jrx_rotate_stress2d / 3d called directly; tau / tau_o / omega: member name -> replacement pointer (None = NULL); V: "all", None (a NULL array) or a list
    of pointers.  Returns (status, text)"""
    ni = st._ni
    nd = len(ni)
    names = list(_members(nd))
    pt = {k: getattr(st.τ, k).data_ptr() for k in names}
    po = {k: getattr(st.τ_o, k).data_ptr() for k in names}
    if nd == 2:
        names += ["xx_v", "yy_v"]
        for k in ("xx_v", "yy_v"):
            pt[k] = getattr(st.τ, k).data_ptr() if optional else None
            po[k] = getattr(st.τ_o, k).data_ptr() if optional else None
    pt.update(tau or {})
    po.update(tau_o or {})
    pw = {k: getattr(st.ω, k).data_ptr() for k in (("xy",) if nd == 2 else ("yz", "xz", "xy"))}
    pw.update(omega or {})
    vec = lambda ps: (C.c_void_p * len(ps))(*ps)
    if V == "all":
        V = [getattr(st.V, k).data_ptr() for k in ("Vx", "Vy", "Vz")[:nd]]
    vel = None if V is None else vec(V)
    n = ni if n is None else n
    tail = [*(C.c_int64(m) for m in n), (C.c_double * nd)(*_DI[:nd]), C.c_double(dt), C.c_int32(method), C.c_int32(advection)]
    fn = getattr(h.lib, f"jrx_rotate_stress{nd}d")
    wv = C.c_void_p(pw["xy"]) if nd == 2 else vec([pw[k] for k in ("yz", "xz", "xy")])
    st_ = fn(h._h, vec([po[k] for k in names]), vec([pt[k] for k in names]), wv, vel, *tail)
    return st_, h.lib.jrx_last_error(h._h).decode()


@pytest.mark.parametrize("ni", [(7, 5), (5, 3, 2)])
@pytest.mark.parametrize("method", [0, 1])
def test_no_advection_takes_null_velocities(jr, h, ni, method):
    import torch
    nd = len(ni)
    τ, ω, _ = SR.random_state(ni, 61)
    ref = SR.rotate_stress(τ, ω, None, ni, None, DT, SR.METHODS[method], "none")
    for V in (None, [None] * nd):
        st = _stokes(jr, ni, τ, ω, None)
        torch.cuda.synchronize()
        status, msg = _c_call(h, st, V=V, method=method, advection=0)
        assert status == 0, msg
        got = {k: jr.to_numpy(getattr(st.τ_o, k)) for k in τ}
        assert not any(np.any(a == SENTINEL) for a in got.values())
        assert _deviation(got, ref, τ) <= BOUND


@pytest.mark.parametrize("ni", [(6, 5), (6, 5, 4)])
def test_c_abi_refusals(jr, h, ni):
    """every JRX_ERR_ARG condition of include/jrx.h: status 4, a text naming the cause, no launch (the counter stands still) and nothing written"""
    import torch
    nd = len(ni)
    τ, ω, V = SR.random_state(ni, 71, optional=nd == 2)
    st = _stokes(jr, ni, τ, ω, V)
    torch.cuda.synchronize()
    opt = nd == 2
    required = list(_members(nd))
    wnames = ("xy",) if nd == 2 else ("yz", "xz", "xy")
    vptr = [getattr(st.V, k).data_ptr() for k in ("Vx", "Vy", "Vz")[:nd]]
    bad = []
    for k in required:                                                   # an output that is an input: the same member, another member, ω, a velocity
        bad.append((dict(tau_o={k: getattr(st.τ, k).data_ptr()}), "overlaps input"))
        bad.append((dict(tau_o={k: None}), f"τ_o.{k} is NULL"))
        bad.append((dict(tau={k: None}), f"τ.{k} is NULL"))
    bad.append((dict(tau_o={"xx": st.τ.yy.data_ptr()}), "overlaps input yy"))
    bad.append((dict(tau_o={"xy": getattr(st.ω, "xy").data_ptr()}), "overlaps input xy"))
    bad.append((dict(tau_o={"xx": st.V.Vx.data_ptr()}), "overlaps input V.Vx"))
    bad.append((dict(tau_o={"xx": st.τ_o.yy.data_ptr()}), "outputs"))
    if opt:
        bad.append((dict(tau_o={"xx_v": st.τ.xx_v.data_ptr()}), "overlaps input xx_v"))
    bad += [(dict(omega={k: None}), f"ω.{k} is NULL") for k in wnames]
    bad += [(dict(V=vptr[:c] + [None] + vptr[c + 1:]), f"V.V{'xyz'[c]} is NULL") for c in range(nd)]
    bad.append((dict(V=None), "V is NULL"))
    bad += [(dict(method=m), "unknown method") for m in (-1, 2)]
    bad += [(dict(advection=a), "unknown advection") for a in (-1, 2)]
    bad += [(dict(n=ni[:d] + (0,) + ni[d + 1:]), f"dimension {d + 1}") for d in range(nd)]
    calls = h.get_option("stat_rotate_stress_calls")
    for kw, text in bad:
        status, msg = _c_call(h, st, optional=opt, **kw)
        assert status == 4 and text in msg, (kw, status, msg)
    torch.cuda.synchronize()
    assert _untouched(st, τ) and _unchanged(jr, st, τ, ω, V) and h.get_option("stat_rotate_stress_calls") == calls
    status, msg = _c_call(h, st, optional=opt)
    assert status == 0, msg
    assert not _untouched(st, τ) and h.get_option("stat_rotate_stress_calls") == calls + 1


def test_host_layer_refusals(jr, h):
    ni = (6, 5)
    τ, ω, V = SR.random_state(ni, 81)
    st = _stokes(jr, ni, τ, ω, V)
    grid = jr.Geometry(ni, (2.0, 1.0))
    calls = h.get_option("stat_rotate_stress_calls")
    with pytest.raises(NotImplementedError, match="uniform"):
        jr.rotate_stress_(st, jr.Geometry.from_vertices((np.linspace(0, 1, 7) ** 2, np.linspace(0, 1, 6))), DT, handle=h)
    with pytest.raises(ValueError, match="method"):
        jr.rotate_stress_(st, grid, DT, method="rk4", handle=h)
    with pytest.raises(ValueError, match="advection"):
        jr.rotate_stress_(st, grid, DT, advection="weno", handle=h)
    assert _untouched(st, τ) and h.get_option("stat_rotate_stress_calls") == calls


# ---------------------------------------------------------------------------------------------- on the arrays a solve leaves
def _restate_from(jr, st, grid, dt, method="matrix", advection="upwind"):
    nd = len(st._ni)
    τ = {k: jr.to_numpy(getattr(st.τ, k)) for k in _members(nd)}
    ω = jr.to_numpy(st.ω.xy) if nd == 2 else {k: jr.to_numpy(getattr(st.ω, k)) for k in SR.OMEGA3}
    V = tuple(jr.to_numpy(getattr(st.V, k)) for k in ("Vx", "Vy", "Vz")[:nd])
    _di = tuple(1.0 / d for d in grid.di["center"])
    return τ, SR.rotate_stress(τ, ω, V, st._ni, _di, dt, method, advection)


def test_after_a_short_2d_multiphase_solve(jr, h):
    """the sinking block at 16 x 16 with iterMax capped (the loop is what is tested, not convergence): rotate_stress_ on the StokesArrays of solve_ gives the
    τ_o the restatement computes from the downloaded τ, ω, V, and that is not the plain copy the driver's epilogue left"""
    import torch
    from test_gpu_vep2d import VEP_MAP, _get
    dev = _dev()
    s = jr.miniapps.sinking_block2d(16, iterMax=200, nout=100)
    try:
        st = jr.StokesArrays(jr.AMDGPUBackend, s.ni)
        for k, path in VEP_MAP.items():
            _get(st, path).copy_(_up(s.arrays[k]))
        pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, s.ni)
        pr.center.copy_(_up(s.arrays["phase_c"]))
        pr.vertex.copy_(_up(s.arrays["phase_v"]))
        ρg = (jr.fzeros(s.ni, dev), _up(s.arrays["fy"]))
        args = dict(T=jr.fzeros(tuple(m + 2 for m in s.ni), dev, 1.0), P=st.P)
        jr.flow_bcs_(st, s.flow_bcs)
        jr.solve_(st, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], args, s.dt, None, kwargs=s.kwargs)
        dt = jr.compute_dt_(st, s.extra["di"])
        members = list(SR.MEMBERS2)
        copied = {k: jr.to_numpy(getattr(st.τ_o, k)) for k in members}
        for k in members:
            assert np.array_equal(copied[k], jr.to_numpy(getattr(st.τ, k))), k      # the epilogue's multi_copy!
        jr.rotate_stress_(st, s.grid, dt, handle=h)
        τ, ref = _restate_from(jr, st, s.grid, dt)
        scale = max(float(np.abs(a).max()) for a in τ.values())
        assert scale > 0.0 and float(np.abs(jr.to_numpy(st.ω.xy)).max()) > 0.0
        for k in members:
            got = jr.to_numpy(getattr(st.τ_o, k))
            assert np.abs(got - ref[k]).max() <= BOUND * scale, k
            assert not np.array_equal(got, copied[k]), k
        assert max(float(np.abs(jr.to_numpy(getattr(st.τ_o, k)) - copied[k]).max()) for k in members) > 1e-6 * scale
    finally:
        jr.finalize_global_grid()
        torch.cuda.synchronize()


def test_on_a_3d_stokes_arrays_filled_by_hand(jr, h):
    ni = (6, 5, 4)
    li = (1.2, 1.0, 0.8)
    jr.finalize_global_grid()
    grid = jr.Geometry(ni, li)
    rng = np.random.default_rng(91)
    τ, _, _ = SR.random_state(ni, 92, scale=3.0e7)
    V = tuple(1.0e-9 * rng.uniform(-1.0, 1.0, SR.velocity_shape(c, ni)) for c in range(3))
    st = _stokes(jr, ni, τ, {k: np.zeros(SR.shape_at(loc, ni)) for k, loc in SR.OMEGA3.items()}, V)
    jr.compute_vorticity_(st, grid, handle=h)                           # ω as the drivers' epilogue leaves it
    dt = jr.compute_dt_(st, grid.di["center"])
    jr.rotate_stress_(st, grid, dt, handle=h)
    _, ref = _restate_from(jr, st, grid, dt)
    for k in SR.MEMBERS3:
        got = jr.to_numpy(getattr(st.τ_o, k))
        assert np.abs(got - ref[k]).max() <= BOUND * 3.0e7, k
        assert np.abs(got - τ[k]).max() > 1e-3 * 3.0e7, k
