"""GPU: WENO-5 advection (WENO5, WENO_advection_; csrc/advection.hip through jrx_weno5_advection2d).  The reference's six-launch form against the
NumPy restatement of weno5.jl (tests/_weno5.py; by tolerance: no fma on the host), the fused three-launch form bit for bit against the six-launch form,
the Benchmark2D_WENO5.jl extents, the counters and the switch, accuracy and constant preservation on the device, argument errors, and the reference's
advection block inside the thermal-convection time loop."""
import sys

import numpy as np
import pytest

import _weno5 as W
from _abi_parse import ROOT

pytestmark = pytest.mark.gpu
RNG = np.random.default_rng(20260821)

SIZES = [(17, 19), (2, 11), (3, 7), (257, 33), (1025, 769)]
# a wave of the fused kernel owns 62 output columns; it marches a chunk of rows (64 when forced, 8 .. 64 by the grid): one below / at / above each
FUSED_SIZES = SIZES + [(61, 9), (62, 8), (63, 7), (123, 65), (124, 64), (125, 63), (2049, 1537)]


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


def _inputs(nx, ny, ext=(0, 0), vext=(0, 0)):
    u = W.sample_field(nx, ny, RNG)
    vx = RNG.uniform(-1.0, 1.0, (nx + vext[0], ny + vext[1]))
    vy = RNG.uniform(-1.0, 1.0, (nx + vext[0], ny + vext[1]))
    dx, dy = 1.0 / max(nx - 1, 1), 1.0 / max(ny - 1, 1)
    dt = 0.4 * min(dx, dy)
    return u, vx, vy, dx, dy, dt


def _run(jr, h, u, vx, vy, dx, dy, dt, method, *, fused, wshape=None):
    """one WENO_advection_ call on fresh device arrays: (u, ut, fL, fR, fB, fT) as NumPy arrays"""
    h.set_option("weno_fused", int(fused))
    w = jr.WENO5(jr.AMDGPUBackend, method, wshape or u.shape)
    ud = _up(u)
    jr.WENO_advection_(ud, (_up(vx), _up(vy)), w, (dx, dy), dt, handle=h)
    return [_dn(t) for t in (ud, w.ut, w.fL, w.fR, w.fB, w.fT)]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("nx,ny", SIZES)
def test_per_kernel_form_matches_the_restatement(jr, nx, ny, method):
    from justrelax_jl_amd.checks import max_rel_diff
    h = _handle(jr)
    u, vx, vy, dx, dy, dt = _inputs(nx, ny)
    got = _run(jr, h, u, vx, vy, dx, dy, dt, method, fused=False)
    unew, ut, f = W.advect(u, vx, vy, dx, dy, dt, method)
    assert max_rel_diff(got[0], unew) <= 1e-12
    assert max_rel_diff(got[1], ut) <= 1e-12
    for g, r in zip(got[2:], f):
        assert max_rel_diff(g, r) <= 1e-13


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("nx,ny", FUSED_SIZES)
def test_fused_form_is_bit_identical_to_the_per_kernel_form(jr, nx, ny, method):
    h = _handle(jr)
    u, vx, vy, dx, dy, dt = _inputs(nx, ny)
    ref = _run(jr, h, u, vx, vy, dx, dy, dt, method, fused=False)
    for rows in (0, 8, 16, 32, 64):          # the depth the grid picks (8 on grids this small) and every depth the size rule can pick
        h.set_option("weno_rows", rows)
        got = _run(jr, h, u, vx, vy, dx, dy, dt, method, fused=True)
        assert np.array_equal(got[0], ref[0]), rows
        assert np.array_equal(got[1], ref[1]), rows
    h.set_option("weno_rows", 0)


@pytest.mark.parametrize("fused", [False, True])
def test_benchmark2d_extents(jr, fused):
    """Benchmark2D_WENO5.jl:77,182: weno built for ni .+ 1, u of ni, velocities larger than u -- every array read with its own extents; entries outside
    u's box untouched"""
    h = _handle(jr)
    nx, ny = 67, 45
    u, vx, vy, dx, dy, dt = _inputs(nx, ny, vext=(3, 2))
    same = _run(jr, h, u, vx[:nx, :ny].copy(), vy[:nx, :ny].copy(), dx, dy, dt, 2, fused=fused)
    h.set_option("weno_fused", int(fused))
    w = jr.WENO5(jr.AMDGPUBackend, 2, (nx + 1, ny + 1))
    for t in (w.ut, w.fL, w.fR, w.fB, w.fT):
        t.fill_(-7.0)
    ud = _up(u)
    jr.WENO_advection_(ud, (_up(vx), _up(vy)), w, (dx, dy), dt, handle=h)
    assert np.array_equal(_dn(ud), same[0])
    ut = _dn(w.ut)
    assert np.array_equal(ut[:nx, :ny], same[1])
    for t in (w.ut, w.fL, w.fR, w.fB, w.fT):
        a = _dn(t)
        assert np.all(a[nx, :] == -7.0) and np.all(a[:, ny] == -7.0)


def test_counters_and_switch(jr):
    h = _handle(jr)
    u, vx, vy, dx, dy, dt = _inputs(40, 30)
    c0, f0 = h.get_option("stat_weno_calls"), h.get_option("stat_weno_fused")
    assert h.get_option("weno_fused") == 1
    w = jr.WENO5(jr.AMDGPUBackend, 1, u.shape)
    jr.WENO_advection_(_up(u), (_up(vx), _up(vy)), w, (dx, dy), dt, handle=h)
    assert (h.get_option("stat_weno_calls"), h.get_option("stat_weno_fused")) == (c0 + 1, f0 + 1)
    assert np.array_equal(_dn(w.fR), np.zeros(u.shape))            # the fused form does not touch fR, fB, fT
    h.set_option("weno_fused", 0)
    jr.WENO_advection_(_up(u), (_up(vx), _up(vy)), w, (dx, dy), dt, handle=h)
    assert (h.get_option("stat_weno_calls"), h.get_option("stat_weno_fused")) == (c0 + 2, f0 + 1)
    assert np.any(_dn(w.fR) != 0.0)                                   # the six-launch form leaves fluxes there
    h.set_option("weno_fused", 1)


@pytest.mark.parametrize("method", [1, 2])
def test_gaussian_accuracy_on_the_device(jr, method):
    from justrelax_jl_amd.checks import max_rel_diff
    h = _handle(jr)
    results = {}
    for n in (64, 128):
        def run(u, vx, vy, dx, dt, nt):
            w = jr.WENO5(jr.AMDGPUBackend, method, u.shape)
            ud, V = _up(u), (_up(vx), _up(vy))
            for _ in range(nt):
                jr.WENO_advection_(ud, V, w, (dx, dx), dt, handle=h)
            return _dn(ud)
        got, _, err = W.gaussian_case(n, method, run=run)
        ref = W.gaussian_case(n, method)[0]
        assert max_rel_diff(got, ref) <= 1e-12
        results[n] = err
    assert np.log2(results[64] / results[128]) >= 3.3
    assert results[128] <= 3e-6


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("method", [1, 2])
def test_constant_field_stays_constant(jr, method, fused):
    h = _handle(jr)
    u = np.full((70, 33), 1234.5678)
    vx, vy = RNG.uniform(-1, 1, u.shape), RNG.uniform(-1, 1, u.shape)
    got = _run(jr, h, u, vx, vy, 0.1, 0.2, 0.01, method, fused=fused)
    assert np.abs(got[0] - u).max() <= np.spacing(1234.5678)
    assert np.abs(got[1] - u).max() <= np.spacing(1234.5678)


def test_bad_arguments_are_refused_without_a_launch(jr):
    import torch
    from justrelax_jl_amd._lib import JrxError
    h = _handle(jr)
    u, vx, vy, dx, dy, dt = _inputs(20, 16)
    ud, V = _up(u), (_up(vx), _up(vy))
    calls = h.get_option("stat_weno_calls")

    def refused(fn, status=4):
        with pytest.raises(JrxError) as e:
            fn()
        assert e.value.status == status
        assert np.array_equal(_dn(ud), u)

    w = jr.WENO5(jr.AMDGPUBackend, 2, u.shape)
    w.method = 3
    refused(lambda: jr.WENO_advection_(ud, V, w, (dx, dy), dt, handle=h))
    for name in ("ut", "fB"):
        w = jr.WENO5(jr.AMDGPUBackend, 2, u.shape)
        setattr(w, name, jr.fzeros((19, 16), _dev()))
        with pytest.raises(ValueError):                                  # the binding sees the mixed sizes first
            jr.WENO_advection_(ud, V, w, (dx, dy), dt, handle=h)
    w = jr.WENO5(jr.AMDGPUBackend, 2, (20, 15))
    refused(lambda: jr.WENO_advection_(ud, V, w, (dx, dy), dt, handle=h))
    w = jr.WENO5(jr.AMDGPUBackend, 2, u.shape)
    refused(lambda: jr.WENO_advection_(ud, (jr.fzeros((19, 16), _dev()), V[1]), w, (dx, dy), dt, handle=h))
    w.ut = ud
    w.fL, w.fR, w.fB, w.fT = ud, jr.fzeros(u.shape, _dev()), jr.fzeros(u.shape, _dev()), jr.fzeros(u.shape, _dev())
    refused(lambda: jr.WENO_advection_(ud, V, w, (dx, dy), dt, handle=h))
    assert h.get_option("stat_weno_calls") == calls
    w = jr.WENO5(jr.AMDGPUBackend, 2, u.shape)
    with pytest.raises(ValueError, match="2D only"):
        jr.WENO_advection_(jr.fzeros((4, 4, 4), _dev()), V, w, (dx, dy), dt, handle=h)
    with pytest.raises(ValueError, match="uniform"):
        jr.WENO_advection_(ud, V, w, (torch.full((20,), dx), torch.full((16,), dy)), dt, handle=h)
    with pytest.raises(ValueError):
        jr.WENO5(jr.AMDGPUBackend, 3, u.shape)
    # the C ABI checks undersized arrays itself (binding checks bypassed)
    import ctypes as C
    from justrelax_jl_amd.arrays import ptr
    small = jr.fzeros((19, 16), _dev())
    w = jr.WENO5(jr.AMDGPUBackend, 2, u.shape)
    d2 = lambda s: (C.c_int64 * 2)(*s)
    for bad in ("ut", "fB"):
        arrs = {k: getattr(w, k) for k in ("ut", "fL", "fR", "fB", "fT")}
        arrs[bad] = small
        st = h.lib.jrx_weno5_advection2d(h._h, C.c_void_p(ptr(ud)), d2(u.shape), C.c_void_p(ptr(V[0])), d2(u.shape), C.c_void_p(ptr(V[1])), d2(u.shape),
                                         *[C.c_void_p(ptr(arrs[k])) for k in ("ut", "fL", "fR", "fB", "fT")], d2((19, 16) if bad else u.shape),
                                         C.c_double(dx), C.c_double(dy), C.c_double(dt), C.c_int32(2))
        assert st == 4
    assert h.get_option("stat_weno_calls") == calls


def test_reference_advection_block_in_the_convection_loop(jr, oracle, tmp_path):
    """test_WENO5.jl:262-266 inside the thermal-convection time loop of examples/thermal_convection2d.py (n = 32, two steps): center2vertex! ->
    velocity2vertex! -> WENO_advection! (Z, weno for ni .+ 1) -> vertex2center! into the ghosted T.  The advected vertex field matches the restatement,
    and T after the block matches the oracle's vertex2center! of it"""
    from justrelax_jl_amd.checks import max_rel_diff
    sys.path.insert(0, str(ROOT / "examples"))
    import thermal_convection2d as ex
    rec = []
    ex.main(32, 2, str(tmp_path), weno=True, record=rec)
    assert len(rec) == 2
    for r in rec:
        dx, dy = r["di"]
        ref = W.advect(r["T_WENO"], r["Vx_v"], r["Vy_v"], dx, dy, r["dt"], 2)[0]
        assert np.all(np.isfinite(r["T_WENO_after"]))
        assert max_rel_diff(r["T_WENO_after"], ref) <= 1e-12
        assert np.abs(r["T_WENO_after"] - r["T_WENO"]).max() > 0.0
        T = np.asfortranarray(r["T_after"].copy())
        oracle.vertex2center(T, np.asfortranarray(r["T_WENO_after"]), ghost=(True, True))
        assert np.array_equal(T, r["T_after"])
