"""GPU: 3D WENO-5 advection (WENO5 with a 3-entry ni, WENO_advection_ with three velocities; csrc/advection.hip through jrx_weno5_advection3d).  The
six-launch form against the NumPy restatement (tests/_weno5_3d.py; by tolerance: no fma on the host), the fused three-launch form bit for bit against the
six-launch form, the reduction to the 2D entry point on z-replicated fields, larger velocity and weno extents, the counters and the switch, accuracy and
constant preservation on the device, argument errors."""
import ctypes as C

import numpy as np
import pytest

import _weno5_3d as W

pytestmark = pytest.mark.gpu
RNG = np.random.default_rng(20261018)

SIZES = [(17, 19, 23), (2, 11, 5), (3, 7, 1), (5, 1, 7), (1, 1, 1), (130, 37, 21)]
# a block of the fused kernel owns 62 output columns and 6 output rows and marches a chunk of planes (64 when forced, 8 .. 64 by the grid; 8 at these
# sizes): one below / at / above each extent, for one tile and for two
FUSED_SIZES = SIZES + [(61, 5, 7), (62, 6, 8), (63, 7, 9), (123, 11, 63), (124, 12, 64), (125, 13, 65)]


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _up(a):
    from justrelax_jl_amd.arrays import from_numpy
    return from_numpy(np.asarray(a, dtype=np.float64), _dev())


def _dn(t):
    from justrelax_jl_amd.arrays import to_numpy
    return to_numpy(t)


def _handle(jr):
    from justrelax_jl_amd import _lib
    return _lib.Handle(_dev().index)


def _field(nx, ny, nz):
    """W.sample_field in (x, y), modulated along z by a smooth factor, a step and noise"""
    z = np.linspace(0, 1, nz)[None, None, :]
    u = W.sample_field(nx, ny, RNG)[:, :, None] * (1.0 + 0.3 * np.sin(2 * np.pi * z)) + np.where(z > 0.6, 0.5, 0.0)
    return u + 0.05 * RNG.standard_normal((nx, ny, nz))


def _inputs(nx, ny, nz, vext=(0, 0, 0)):
    u = _field(nx, ny, nz)
    v = [RNG.uniform(-1.0, 1.0, (nx + vext[0], ny + vext[1], nz + vext[2])) for _ in range(3)]
    d = tuple(1.0 / max(n - 1, 1) for n in (nx, ny, nz))
    return u, v, d, 0.4 * min(d)


def _run(jr, h, u, v, d, dt, method, *, fused, wshape=None):
    """one WENO_advection_ call on fresh device arrays: (u, ut, fL, fR, fB, fT, fD, fU) as NumPy arrays"""
    h.set_option("weno_fused", int(fused))
    w = jr.WENO5(jr.AMDGPUBackend, method, wshape or u.shape)
    ud = _up(u)
    jr.WENO_advection_(ud, tuple(_up(a) for a in v), w, d, dt, handle=h)
    return [_dn(t) for t in (ud, w.ut, w.fL, w.fR, w.fB, w.fT, w.fD, w.fU)]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("shape", SIZES)
def test_per_kernel_form_matches_the_restatement(jr, shape, method):
    """the 2D test's tolerances (measured on these sizes: at most 5.3e-16 for u and ut, 1.8e-15 for the fluxes)"""
    from justrelax_jl_amd.checks import max_rel_diff
    h = _handle(jr)
    u, v, d, dt = _inputs(*shape)
    got = _run(jr, h, u, v, d, dt, method, fused=False)
    unew, ut, f = W.advect3(u, *v, *d, dt, method)
    print("max_rel_diff u, ut, fluxes:", max_rel_diff(got[0], unew), max_rel_diff(got[1], ut), [max_rel_diff(g, r) for g, r in zip(got[2:], f)])
    assert max_rel_diff(got[0], unew) <= 1e-12
    assert max_rel_diff(got[1], ut) <= 1e-12
    for g, r in zip(got[2:], f):
        assert max_rel_diff(g, r) <= 1e-13


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("shape", FUSED_SIZES)
def test_fused_form_is_bit_identical_to_the_per_kernel_form(jr, shape, method):
    h = _handle(jr)
    u, v, d, dt = _inputs(*shape)
    ref = _run(jr, h, u, v, d, dt, method, fused=False)
    assert np.abs(ref[0] - u).max() > 0.0 or shape == (1, 1, 1)
    for rows in (0, 8, 16, 32, 64):          # the depth the grid picks (8 on grids this small) and every depth the size rule can pick
        h.set_option("weno_rows", rows)
        got = _run(jr, h, u, v, d, dt, method, fused=True)
        assert np.array_equal(got[0], ref[0]), rows
        assert np.array_equal(got[1], ref[1]), rows
    h.set_option("weno_rows", 0)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("method", [1, 2])
def test_z_replicated_field_has_the_bits_of_the_2d_entry_point(jr, method, fused):
    """both z terms are exactly 0 and come first in the device's rhs chain: every plane of u and ut equals what jrx_weno5_advection2d gives"""
    h = _handle(jr)
    nx, ny, nz = 61, 33, 9
    u2 = W.sample_field(nx, ny, RNG)
    vx2, vy2 = RNG.uniform(-1, 1, (nx, ny)), RNG.uniform(-1, 1, (nx, ny))
    rep = lambda a: np.repeat(a[:, :, None], nz, axis=2)
    dx, dy, dt = 1 / 60, 1 / 32, 0.4 / 60
    h.set_option("weno_fused", int(fused))
    w2 = jr.WENO5(jr.AMDGPUBackend, method, (nx, ny))
    u2d = _up(u2)
    jr.WENO_advection_(u2d, (_up(vx2), _up(vy2)), w2, (dx, dy), dt, handle=h)
    ref_u, ref_ut = _dn(u2d), _dn(w2.ut)
    assert np.abs(ref_u - u2).max() > 0.0
    got = _run(jr, h, rep(u2), [rep(vx2), rep(vy2), RNG.uniform(-1, 1, (nx, ny, nz))], (dx, dy, 0.125), dt, method, fused=fused)
    for k in range(nz):
        assert np.array_equal(got[0][:, :, k], ref_u), k
        assert np.array_equal(got[1][:, :, k], ref_ut), k


@pytest.mark.parametrize("fused", [False, True])
def test_larger_velocity_and_weno_extents(jr, fused):
    """weno built for ni .+ 1, u of ni, velocities larger still (Benchmark2D_WENO5.jl:77,182 one dimension up): every array read with its own extents;
    entries outside u's box untouched"""
    h = _handle(jr)
    nx, ny, nz = 67, 13, 10
    u, v, d, dt = _inputs(nx, ny, nz, vext=(3, 2, 4))
    same = _run(jr, h, u, [a[:nx, :ny, :nz].copy() for a in v], d, dt, 2, fused=fused)
    h.set_option("weno_fused", int(fused))
    w = jr.WENO5(jr.AMDGPUBackend, 2, (nx + 1, ny + 1, nz + 1))
    work = (w.ut, w.fL, w.fR, w.fB, w.fT, w.fD, w.fU)
    for t in work:
        t.fill_(-7.0)
    ud = _up(u)
    jr.WENO_advection_(ud, tuple(_up(a) for a in v), w, d, dt, handle=h)
    assert np.array_equal(_dn(ud), same[0])
    assert np.array_equal(_dn(w.ut)[:nx, :ny, :nz], same[1])
    for t in work:
        a = _dn(t)
        assert np.all(a[nx, :, :] == -7.0) and np.all(a[:, ny, :] == -7.0) and np.all(a[:, :, nz] == -7.0)


def test_counters_and_switch(jr):
    h = _handle(jr)
    u, v, d, dt = _inputs(20, 15, 12)
    c0, f0 = h.get_option("stat_weno3d_calls"), h.get_option("stat_weno3d_fused")
    c2, f2 = h.get_option("stat_weno_calls"), h.get_option("stat_weno_fused")
    assert h.get_option("weno_fused") == 1
    w = jr.WENO5(jr.AMDGPUBackend, 1, u.shape)
    V = tuple(_up(a) for a in v)
    jr.WENO_advection_(_up(u), V, w, d, dt, handle=h)
    assert (h.get_option("stat_weno3d_calls"), h.get_option("stat_weno3d_fused")) == (c0 + 1, f0 + 1)
    for t in (w.fR, w.fB, w.fT, w.fD, w.fU):                             # the fused form does not touch them
        assert np.array_equal(_dn(t), np.zeros(u.shape))
    h.set_option("weno_fused", 0)
    jr.WENO_advection_(_up(u), V, w, d, dt, handle=h)
    assert (h.get_option("stat_weno3d_calls"), h.get_option("stat_weno3d_fused")) == (c0 + 2, f0 + 1)
    assert np.any(_dn(w.fD) != 0.0) and np.any(_dn(w.fU) != 0.0)          # the six-launch form leaves fluxes there
    h.set_option("weno_fused", 1)
    assert (h.get_option("stat_weno_calls"), h.get_option("stat_weno_fused")) == (c2, f2)


@pytest.mark.parametrize("method", [1, 2])
def test_gaussian_accuracy_on_the_device(jr, method):
    """the bounds of the CPU test of the restatement (order >= 3.3 between n = 32 and 64, L1 error at n = 64 <= 1e-5), fused form"""
    h = _handle(jr)
    assert h.get_option("weno_fused") == 1
    err = {}
    for n in (32, 64):
        def run(u, vx, vy, vz, dx, dt, nt):
            w = jr.WENO5(jr.AMDGPUBackend, method, u.shape)
            ud, V = _up(u), (_up(vx), _up(vy), _up(vz))
            for _ in range(nt):
                jr.WENO_advection_(ud, V, w, (dx, dx, dx), dt, handle=h)
            return _dn(ud)
        err[n] = W.gaussian_case3(n, method, run=run)[2]
    print("L1 errors:", err)
    assert np.log2(err[32] / err[64]) >= 3.3
    assert err[64] <= 1.0e-5


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("method", [1, 2])
def test_constant_field_stays_constant(jr, method, fused):
    h = _handle(jr)
    u = np.full((70, 9, 11), 1234.5678)
    v = [RNG.uniform(-1, 1, u.shape) for _ in range(3)]
    got = _run(jr, h, u, v, (0.1, 0.2, 0.15), 0.01, method, fused=fused)
    assert np.abs(got[0] - u).max() <= np.spacing(1234.5678)
    assert np.abs(got[1] - u).max() <= np.spacing(1234.5678)


def test_bad_arguments_are_refused_without_a_launch(jr):
    import torch
    from justrelax_jl_amd._lib import JrxError
    from justrelax_jl_amd.arrays import ptr
    h = _handle(jr)
    shape = (12, 10, 8)
    u, v, d, dt = _inputs(*shape)
    ud, V = _up(u), tuple(_up(a) for a in v)
    calls = h.get_option("stat_weno3d_calls")
    small = (12, 10, 7)

    def refused(fn, status=4):
        with pytest.raises(JrxError) as e:
            fn()
        assert e.value.status == status
        assert np.array_equal(_dn(ud), u)

    w = jr.WENO5(jr.AMDGPUBackend, 2, shape)
    w.method = 3
    refused(lambda: jr.WENO_advection_(ud, V, w, d, dt, handle=h))
    w = jr.WENO5(jr.AMDGPUBackend, 2, shape)
    refused(lambda: jr.WENO_advection_(ud, (V[0], V[1], jr.fzeros(small, _dev())), w, d, dt, handle=h))            # undersized vz
    refused(lambda: jr.WENO_advection_(ud, V, jr.WENO5(jr.AMDGPUBackend, 2, small), d, dt, handle=h))              # undersized ut, fL .. fU
    w.ut = ud                                                                                                     # u and ut overlap
    refused(lambda: jr.WENO_advection_(ud, V, w, d, dt, handle=h))
    # straight through the C ABI (the binding's common-size check bypassed): one undersized array, and a NULL fD in the per-kernel form
    w = jr.WENO5(jr.AMDGPUBackend, 2, shape)
    d3 = lambda s: (C.c_int64 * 3)(*s)
    names = ("ut", "fL", "fR", "fB", "fT", "fD", "fU")

    def abi(arrs, wshape):
        return h.lib.jrx_weno5_advection3d(h._h, C.c_void_p(ptr(ud)), d3(shape), C.c_void_p(ptr(V[0])), d3(shape), C.c_void_p(ptr(V[1])), d3(shape),
                                           C.c_void_p(ptr(V[2])), d3(shape), *[C.c_void_p(ptr(arrs[k]) if arrs[k] is not None else None) for k in names],
                                           d3(wshape), *(C.c_double(x) for x in d), C.c_double(dt), C.c_int32(2))
    for bad in ("ut", "fD"):
        arrs = {k: getattr(w, k) for k in names}
        arrs[bad] = jr.fzeros(small, _dev())
        assert abi(arrs, small) == 4
    arrs = {k: getattr(w, k) for k in names}
    arrs["fD"] = None
    h.set_option("weno_fused", 0)
    assert abi(arrs, shape) == 4
    h.set_option("weno_fused", 1)
    assert np.array_equal(_dn(ud), u)
    assert h.get_option("stat_weno3d_calls") == calls
    assert abi(arrs, shape) == 0                                         # the fused form takes a NULL fD
    assert h.get_option("stat_weno3d_calls") == calls + 1
    # the binding: mixed dimensionality, spacing vectors, a mis-sized work array; the 2D path still refuses a 3D u
    ud, w = _up(u), jr.WENO5(jr.AMDGPUBackend, 2, shape)
    with pytest.raises(ValueError, match="3D"):
        jr.WENO_advection_(ud, (V[0], V[1], jr.fzeros((12, 10), _dev())), w, d, dt, handle=h)
    with pytest.raises(ValueError, match="3D"):
        jr.WENO_advection_(jr.fzeros((12, 10), _dev()), V, w, d, dt, handle=h)
    with pytest.raises(ValueError, match="uniform"):
        jr.WENO_advection_(ud, V, w, tuple(torch.full((n,), x) for n, x in zip(shape, d)), dt, handle=h)
    with pytest.raises(ValueError, match="uniform"):
        jr.WENO_advection_(ud, V, w, d[:2], dt, handle=h)
    w.fD = jr.fzeros(small, _dev())
    with pytest.raises(ValueError, match="common size"):
        jr.WENO_advection_(ud, V, w, d, dt, handle=h)
    w2 = jr.WENO5(jr.AMDGPUBackend, 2, (12, 10))
    with pytest.raises(ValueError, match="2D only"):
        jr.WENO_advection_(jr.fzeros((4, 4, 4), _dev()), (jr.fzeros((12, 10), _dev()), jr.fzeros((12, 10), _dev())), w2, d[:2], dt, handle=h)
    assert np.array_equal(_dn(ud), u)
    assert h.get_option("stat_weno3d_calls") == calls + 1
