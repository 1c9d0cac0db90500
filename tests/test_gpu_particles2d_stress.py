"""GPU: the elastic stress on 2D particles -- centroid2particle!, particle2centroid!, rotate_stress_particles!, rotate_stress! on particles and stress2grid!
(csrc/particles.hip through jrx_particles2d_centroid2particle, _particle2centroid, _rotate, _rotate_stress, _stress2grid) against the NumPy restatement
(tests/_particles2d_stress.py, pinned by tests/test_particles2d_stress_restatement.py).

Compared BIT FOR BIT, as 64-bit patterns: operators 6 and 7, operator 8 and rotate_stress! with the Jaumann rate, stress2grid!, and the one-launch forms against their
chains ("particles_stress_fused" 1 against 0, device against device, both methods, every output).  The rotation matrix differs from NumPy only by the device's
sincos: within 1e-13 max|τ|, the project's bound for device arithmetic against NumPy (tests/test_gpu_stress_rotation.py); every case prints its measured figure.

Sizes: (2, 2) is the smallest grid operator 6 accepts and three quarters of its area extrapolate; (7, 5) is one ragged block; (33, 17) has 561 cells and 612 nodes:
more than two 256-thread blocks in y; (128, 5) is the smallest shape whose cell launches have two block columns and whose node launches have three.
max_xcell = 12, nxcell = 4, jittered.  The cloud is the restatement's after one advect_rk2 + move under a rigid rotation (_rotated of tests/_particles_gpu.py):
buckets unevenly filled, inactive slots in every cell.  It is used as it is and, where the grid has one, with an interior cell emptied; a 2 x 2 grid has no interior
cell (each of its cells is the only one of a corner vertex).  The restatement shows on the CPU, before the device is asked, that in the first cloud every centre
and vertex has den > 0 and in the second exactly the emptied centre has den == 0 and no vertex has.
Not exercised: the refusal of a handle with a communicator (it needs a second rank)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _particles2d as PT
import _particles2d_stress as PS
from _particles_gpu import D, MAX_XCELL, SENTINEL, _P, _assert_cloud_untouched, _bits, _device_particles, _handle, _launches, _ndiff, _rotated, _rotation, _same, _up, _vec

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2), (7, 5), (33, 17), (128, 5)]
CASES = [(ni, e) for ni in SHAPES for e in (False, True) if not (e and ni == (2, 2))]
DX, DY = D[:2]
DT = 0.5          # |ω| <= 2: |ω dt| <= 1
METHODS = {"matrix": 0, "jaumann": 1}
RTOL = 1e-13


@pytest.fixture(scope="module")
def h(jr):
    hh = _handle()
    yield hh
    hh.set_option("particles_stress_fused", 1)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def _case(ni, emptied):
    """(cloud, hole, (pτxx, pτyy, pτxy, pω), (τxx, τyy, τxy, ωxy)): computed once per case and shared read-only"""
    q = _rotated(ni)
    hole = (ni[0] // 2, ni[1] // 2) if emptied else None
    if emptied:
        q.active[hole], q.px[hole], q.py[hole] = 0, 0.0, 0.0
    a = q.active != 0
    per_cell = a.sum(axis=2)
    assert per_cell.max() < MAX_XCELL and per_cell.min() != per_cell.max()          # inactive slots everywhere, buckets unevenly filled
    dc, dv = PS.centre_den(q), PS.vertex_den(q)
    if emptied:
        assert dc[hole] == 0.0 and (dc == 0.0).sum() == 1 and dv.min() > 0.0
    else:
        assert dc.min() > 0.0 and dv.min() > 0.0
    rng = np.random.default_rng(11 + ni[0])
    pf = tuple(np.where(a, rng.uniform(-lim, lim, a.shape), 0.0) for lim in (3.0, 3.0, 3.0, 2.0))
    vs = (ni[0] + 1, ni[1] + 1)
    gf = tuple(np.asfortranarray(rng.uniform(-lim, lim, shp)) for lim, shp in ((3.0, ni), (3.0, ni), (3.0, vs), (2.0, vs)))
    _frozen(q.px, q.py, q.active, *pf, *gf)
    return q, hole, pf, gf


def _with_nan(q, second=np.nan):
    """a copy of the cloud with a NaN x in one active slot and a NaN (or `second`) y in another"""
    q = PT.copy(q)
    i, j = q.nx // 2, 0
    assert q.active[i, j, 0] == 1 and q.active[0, q.ny - 1, 0] == 1
    q.px[i, j, 0], q.py[0, q.ny - 1, 0] = np.nan, second
    return q, ((i, j, 0), (0, q.ny - 1, 0))


def _rotate_stress(h, p, pdev, gdev, method, fused):
    h.set_option("particles_stress_fused", int(fused))
    s = p._struct()
    h.call("jrx_particles2d_rotate_stress", _vec(pdev[:3]), _P(pdev[3]), *(_P(g) for g in gdev), C.byref(s), C.c_double(DT), C.c_int32(METHODS[method]))


def _stress2grid(h, p, out, pdev, fused):
    h.set_option("particles_stress_fused", int(fused))
    s = p._struct()
    h.call("jrx_particles2d_stress2grid", _vec(out), _vec(pdev[:3]), C.byref(s))


def _sentinel_grid(jr, ni):
    """τ_o = {xx, yy, xy_c, xy, xx_v, yy_v}, sentinel-filled: host copies and device arrays"""
    shapes = [ni] * 3 + [(ni[0] + 1, ni[1] + 1)] * 3
    host = {k: np.asfortranarray(np.full(s, SENTINEL)) for k, s in zip(PS.TAU_O, shapes)}
    return host, [_up(host[k]) for k in PS.TAU_O]


def _close(got, want, scale, what):
    """the rotation-matrix bound; NaNs must sit in the same places"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    err = float(np.abs(got - want)[~nan].max()) / scale
    print(f"{what}: max |device - NumPy| = {err:.3e} max|τ| (bound {RTOL:.0e})")
    assert err <= RTOL, (what, err)
    return err


# ---------------------------------------------------------------------------------------------- operators 6 and 7
@pytest.mark.parametrize("ni,emptied", CASES)
def test_centroid2particle_and_particle2centroid_bit_for_bit(jr, h, ni, emptied):
    q0, hole, pf, gf = _case(ni, emptied)
    q, planted = _with_nan(q0, np.inf)
    old = np.full(q.px.shape, SENTINEL)
    want = PS.centroid2particle(old, gf[0], q)
    assert all(want[at] == SENTINEL for at in planted) and (want == SENTINEL).sum() == 2          # an active slot with a non-finite coordinate is left as it was
    p, (pF,) = _device_particles(jr, q, (old,))
    dF = _up(gf[0])
    n0 = _launches(h)
    jr.centroid2particle_(pF, dF, p, handle=h)
    got = jr.to_numpy(pF)
    assert _launches(h) == n0 + 1 and _same(got, want), _ndiff(got, want)
    assert np.all(_bits(got[q.active == 0]) == 0)          # +0.0
    assert _same(jr.to_numpy(dF), gf[0])
    _assert_cloud_untouched(jr, p, q)
    # operator 7 on the clean cloud
    p, (pF,) = _device_particles(jr, q0, (pf[0],))
    G0 = np.asfortranarray(np.full(ni, SENTINEL))
    dG = _up(G0)
    want = PS.particle2centroid(G0, pf[0], q0)
    assert (want == SENTINEL).sum() == int(emptied) and (not emptied or want[hole] == SENTINEL)
    jr.particle2centroid_(dG, pF, p, handle=h)
    got = jr.to_numpy(dG)
    assert _launches(h) == n0 + 2 and _same(got, want), _ndiff(got, want)
    assert _same(jr.to_numpy(pF), pf[0])
    _assert_cloud_untouched(jr, p, q0)


# ---------------------------------------------------------------------------------------------- operator 8
@pytest.mark.parametrize("method", ["matrix", "jaumann"])
@pytest.mark.parametrize("ni", SHAPES)
def test_rotate_stress_particles_in_place(jr, h, ni, method):
    q, _, pf, _ = _case(ni, False)
    want = PS.rotate(pf[:3], pf[3], q, DT, method)
    p, dev = _device_particles(jr, q, pf)
    n0 = _launches(h)
    jr.rotate_stress_particles_(dev[:3], (dev[3],), p, DT, method=method, handle=h)
    assert _launches(h) == n0 + 1
    got = [jr.to_numpy(d) for d in dev]
    scale = max(np.abs(f).max() for f in pf[:3])
    for k, name in enumerate(("pτxx", "pτyy", "pτxy")):
        assert not _same(got[k], pf[k])
        if method == "jaumann":
            assert _same(got[k], want[k]), (name, _ndiff(got[k], want[k]))
        else:
            _close(got[k], want[k], scale, f"rotate_stress_particles! {ni} {name}")
        assert np.all(_bits(got[k][q.active == 0]) == 0)
    assert _same(got[3], pf[3])          # pω is an input
    _assert_cloud_untouched(jr, p, q)


# ---------------------------------------------------------------------------------------------- operator 9: rotate_stress!
@pytest.mark.parametrize("method", ["matrix", "jaumann"])
@pytest.mark.parametrize("ni,emptied", CASES)
def test_rotate_stress_one_launch_equals_its_chain_and_the_restatement(jr, h, ni, emptied, method):
    q0, _, _, gf = _case(ni, emptied)
    qn, planted = _with_nan(q0)
    gdev = [_up(g) for g in gf]
    old = tuple(np.full(q0.px.shape, SENTINEL * (k + 1)) for k in range(4))
    scale = max(np.abs(g).max() for g in gf[:3])
    names = ("pτxx", "pτyy", "pτxy", "pω")
    for q, what in ((q0, "clean"), (qn, "non-finite")):
        want = PS.rotate_stress(old[:3], old[3], *gf, q, DT, method)
        out = {}
        for fused, launches in ((1, 1), (0, 5)):
            p, dev = _device_particles(jr, q, old)
            n0 = _launches(h)
            _rotate_stress(h, p, dev, gdev, method, fused)
            assert _launches(h) == n0 + launches
            out[fused] = [jr.to_numpy(d) for d in dev]
            _assert_cloud_untouched(jr, p, q)
        for k, name in enumerate(names):
            f, c = out[1][k], out[0][k]
            assert _same(f, c), (what, name, "fused against chain", _ndiff(f, c))          # NaN slots included: the same bits
            assert np.all(_bits(f[q.active == 0]) == 0)
            assert not (f == SENTINEL * (k + 1)).any()          # every slot written
            if method == "jaumann" or name == "pω":
                ok = ~np.isnan(want[k])
                assert np.array_equal(np.isnan(f), ~ok) and np.array_equal(_bits(f)[ok], _bits(want[k])[ok]), (what, name)
            else:
                _close(f, want[k], scale, f"rotate_stress! {ni} {what} {name}")
        if q is qn:          # the chain keeps xx, yy of such a slot, makes NaN of xy and ω there, and the rotation then makes NaN of all three
            assert all(np.isnan(out[1][k][at]) for k in range(4) for at in planted) and sum(int(np.isnan(o).sum()) for o in out[1]) == 8
    assert all(_same(jr.to_numpy(d), g) for d, g in zip(gdev, gf))


# ---------------------------------------------------------------------------------------------- operator 9: stress2grid!
@pytest.mark.parametrize("ni,emptied", CASES)
def test_stress2grid_one_launch_equals_its_chain_and_the_restatement(jr, h, ni, emptied):
    q, hole, pf, _ = _case(ni, emptied)
    p, dev = _device_particles(jr, q, pf[:3])
    host, _ = _sentinel_grid(jr, ni)
    want = PS.stress2grid(host, pf[:3], q)
    out = {}
    for fused, launches in ((1, 1), (0, 6)):
        _, dout = _sentinel_grid(jr, ni)
        n0 = _launches(h)
        _stress2grid(h, p, dout, dev, fused)
        assert _launches(h) == n0 + launches
        out[fused] = [jr.to_numpy(d) for d in dout]
    for k, name in enumerate(PS.TAU_O):
        f, c = out[1][k], out[0][k]
        assert _same(f, c), (name, "fused against chain", _ndiff(f, c))
        assert _same(f, want[name]), (name, _ndiff(f, want[name]))
        kept = f == SENTINEL
        if emptied and name in ("xx", "yy", "xy_c"):
            assert kept.sum() == 1 and kept[hole]          # exactly the den == 0 entry keeps the sentinel
        else:
            assert not kept.any()
    assert all(_same(jr.to_numpy(d), f) for d, f in zip(dev, pf[:3]))
    _assert_cloud_untouched(jr, p, q)


# ---------------------------------------------------------------------------------------------- refusals
def test_the_library_refuses_with_status_4_a_text_and_no_launch(jr, h):
    ni = (7, 5)
    q, _, pf, gf = _case(ni, False)
    p, dev = _device_particles(jr, q, tuple(np.full(q.px.shape, SENTINEL) for _ in range(4)))
    gdev = [_up(g) for g in gf]
    _, dout = _sentinel_grid(jr, ni)
    L = h.lib
    n0 = _launches(h)

    def S(**kw):
        s = p._struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def refused(status, text):
        assert status == 4 and text in L.jrx_last_error(h._h).decode(), (status, text, L.jrx_last_error(h._h).decode())
        assert _launches(h) == n0

    pt, D, I = _vec(dev[:3]), C.c_double, C.c_int32
    c2p = lambda s, a=_P(dev[0]), f=_P(gdev[0]): L.jrx_particles2d_centroid2particle(h._h, a, f, C.byref(s))
    p2c = lambda s, f=_P(dout[0]), a=_P(dev[0]): L.jrx_particles2d_particle2centroid(h._h, f, a, C.byref(s))
    rot = lambda s, t=pt, w=_P(dev[3]), dt=DT, m=0: L.jrx_particles2d_rotate(h._h, t, w, C.byref(s), D(dt), I(m))
    rs = lambda s, t=pt, w=_P(dev[3]), g=tuple(_P(x) for x in gdev), dt=DT, m=0: L.jrx_particles2d_rotate_stress(h._h, t, w, *g, C.byref(s), D(dt), I(m))
    s2g = lambda s, o=_vec(dout), t=pt: L.jrx_particles2d_stress2grid(h._h, o, t, C.byref(s))
    for fused in (1, 0):          # the chains check everything before their first launch too
        h.set_option("particles_stress_fused", fused)
        # the struct checks of the particle section
        for call in (c2p, p2c, rot, rs, s2g):
            refused(call(S(px=None)), "particles.px is NULL")
            refused(call(S(max_xcell=0)), "max_xcell = 0")
            refused(call(S(dx=-DX)), "spacings")
            refused(call(S(_dy=1.0)), "not 1 / dx")
            refused(call(S(y0=float("inf"))), "origin")
        refused(L.jrx_particles2d_stress2grid(h._h, _vec(dout), pt, None), "particles is NULL")
        # NULL pointers
        refused(c2p(S(), a=None), "pF is NULL")
        refused(c2p(S(), f=None), "F is NULL")
        refused(p2c(S(), f=None), "F is NULL")
        refused(rot(S(), t=None), "ptau is NULL")
        refused(rot(S(), w=None), "pω is NULL")
        refused(rot(S(), t=(C.c_void_p * 3)(dev[0].data_ptr(), None, dev[2].data_ptr())), "pτyy is NULL")
        refused(rs(S(), w=None), "pω is NULL")
        refused(rs(S(), g=(_P(gdev[0]), _P(gdev[1]), None, _P(gdev[3]))), "τ.xy is NULL")
        refused(s2g(S(), o=None), "tau_o is NULL")
        refused(s2g(S(), o=(C.c_void_p * 6)(*([d.data_ptr() for d in dout[:4]] + [None, dout[5].data_ptr()]))), "τ_o.xx_v is NULL")
        # extents below 2 where operator 6 is involved (operator 7, operator 8 and stress2grid! take them)
        refused(c2p(S(nx=1)), "nx >= 2")
        refused(rs(S(ny=1)), "nx >= 2")
        # dt, method
        refused(rot(S(), dt=float("nan")), "dt = nan")
        refused(rs(S(), dt=float("inf")), "dt = inf")
        refused(rot(S(), m=2), "unknown method 2")
        refused(rs(S(), m=-1), "unknown method -1")
        # overlaps: with an input, with another output, with the particles' own arrays
        refused(c2p(S(), a=_P(p.coords[0])), "pF overlaps the particle coordinates")
        refused(c2p(S(), f=_P(dev[0])), "pF overlaps F")
        refused(p2c(S(), f=_P(dev[0])), "F overlaps pF")
        refused(rot(S(), w=_P(dev[1])), "pτyy overlaps pω")
        refused(rot(S(), t=_vec([dev[0], dev[0], dev[2]])), "pτxx and pτyy overlap")
        refused(rs(S(), w=_P(dev[2])), "pτxy and pω overlap")
        refused(rs(S(), g=(_P(dev[2]),) + tuple(_P(x) for x in gdev[1:])), "pτxy overlaps τ.xx")
        refused(rs(S(), t=_vec([dev[0], dev[1], p.coords[1]])), "pτxy overlaps the particle coordinates")
        refused(s2g(S(), o=_vec([dout[0], dout[0]] + dout[2:])), "τ_o.xx and τ_o.yy overlap")
        refused(s2g(S(), o=_vec([dev[0]] + dout[1:])), "τ_o.xx overlaps pτxx")
    h.set_option("particles_stress_fused", 1)
    # nothing was written
    assert all(float((d - SENTINEL).abs().max()) == 0.0 for d in dev) and all(float((d - SENTINEL).abs().max()) == 0.0 for d in dout)
    assert all(_same(jr.to_numpy(d), g) for d, g in zip(gdev, gf))
    _assert_cloud_untouched(jr, p, q)
    # the wrappers look at the device of every operand
    with pytest.raises(ValueError, match="F is on cpu"):
        jr.centroid2particle_(dev[0], jr.fzeros(ni, "cpu"), p, handle=h)
    with pytest.raises(ValueError, match="pω is on cpu"):
        jr.rotate_stress_particles_(dev[:3], (jr.fzeros(p.shape, "cpu"),), p, DT, handle=h)
    assert _launches(h) == n0


# ---------------------------------------------------------------------------------------------- the Python layer, one step
def test_one_step_through_the_python_layer_on_a_stokes_arrays(jr, h):
    """rotate_stress_ (particle form), advection_, move_particles_, stress2grid_ against the restatement, with the Jaumann rate so that every array can be held
    bit for bit (the rotation matrix has its own tests above)"""
    ni = (7, 5)
    q, _, _, gf = _case(ni, False)
    q = PT.copy(q)
    Vx, Vy = _rotation(ni)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    st.τ.xx.copy_(_up(gf[0])), st.τ.yy.copy_(_up(gf[1])), st.τ.xy.copy_(_up(gf[2])), st.ω.xy.copy_(_up(gf[3]))
    st.V.Vx.copy_(_up(Vx)), st.V.Vy.copy_(_up(Vy))
    p, dev = _device_particles(jr, q, tuple(np.full(q.px.shape, SENTINEL) for _ in range(4)))
    for d in dev:
        p._twins[id(d)][1].fill_(SENTINEL)
    for k in PS.TAU_O:
        getattr(st.τ_o, k).fill_(SENTINEL)          # xx_v, yy_v are allocated by this touch
    n0 = _launches(h)
    jr.rotate_stress_(*dev, st, p, DT, method="jaumann", handle=h)
    jr.advection_(p, jr.RungeKutta2(), st.V, 1.0, handle=h)
    counts = jr.move_particles_(p, dev, handle=h)
    jr.stress2grid_(st, *dev[:3], p, handle=h)
    assert _launches(h) == n0 + 4
    old = tuple(np.full(q.px.shape, SENTINEL) for _ in range(4))
    pf = PS.rotate_stress(old[:3], old[3], *gf, q, DT, "jaumann")
    PT.advect_rk2(q, Vx, Vy, 1.0)
    q, pf, c = PT.move(q, pf)
    assert counts == c and c["n_far"] == 0 and c["n_overflow"] == 0
    assert PS.centre_den(q).min() > 0.0 and PS.vertex_den(q).min() > 0.0
    want = PS.stress2grid({k: np.full(ni if k in ("xx", "yy", "xy_c") else (ni[0] + 1, ni[1] + 1), SENTINEL) for k in PS.TAU_O}, pf[:3], q)
    for d, f in zip(dev, pf):
        assert _same(jr.to_numpy(d), f)
    for k in PS.TAU_O:
        g = jr.to_numpy(getattr(st.τ_o, k))
        assert _same(g, want[k]) and not (g == SENTINEL).any(), k
    _assert_cloud_untouched(jr, p, q)
    # the grid form is still reached with the StokesArrays first
    c0 = h.get_option("stat_rotate_stress_calls")
    jr.rotate_stress_(st, (DX, DY), 0.01, handle=h)
    assert h.get_option("stat_rotate_stress_calls") == c0 + 1 and _launches(h) == n0 + 4
