"""GPU: the 2D particle operators (advection_, move_particles_, grid2particle_, particle2grid_, update_phase_ratios_; csrc/particles.hip through the five
jrx_particles2d_* entry points) against the NumPy restatement (tests/_particles2d.py, pinned by tests/test_particles2d_restatement.py): coordinates, mask,
particle fields, ratios and counters BIT FOR BIT (compared as 64-bit patterns: the kernels have no fma, the library is built without contraction, every
kernel is a gather in a fixed order), the inputs untouched, sentinel-filled outputs fully written, and every refusal with "stat_particles_launches" unchanged.

Sizes: (7, 5) is one block with ragged edges; (33, 17) has 561 cells and 612 nodes: more than two 256-thread blocks in y; (128, 5) is the
smallest shape whose cell launches have two block columns and whose node launches have three.  max_xcell = 12, nxcell = 4, jittered.  The helpers shared with the
other particle files are in tests/_particles_gpu.py.
Where a test asserts that a counter is zero or positive, the restatement shows it on the CPU before the device is asked.
Not exercised: the refusal of a handle with a communicator (it needs a second rank)."""
import ctypes as C

import numpy as np
import pytest

import _particles2d as PT
from _particles_gpu import D, MAX_XCELL, NXCELL, ORIGIN, SENTINEL, _V, _assert_state, _bits, _cloud, _dev, _device_particles, _host, _launches, _move, _rotation, _same, _up
from _particles_gpu import h          # noqa: F401 -- the module's handle, a fixture

pytestmark = pytest.mark.gpu
SHAPES = [(7, 5), (33, 17), (128, 5)]
DX, DY = D[:2]
NXCELL = NXCELL[2]


# ---------------------------------------------------------------------------------------------- advect + move
@pytest.mark.parametrize("ni", SHAPES)
def test_a_rigid_rotation_at_courant_half_advects_and_moves_bit_for_bit(jr, h, ni):
    q, fields = _cloud(ni)
    Vx, Vy = _rotation(ni)
    want = PT.copy(q)
    PT.advect_rk2(want, Vx, Vy, 1.0)
    moved, mfields, c = PT.move(want, fields)
    assert c["n_far"] == 0 and c["n_overflow"] == 0 and c["n_active_after"] > 0.9 * c["n_active_before"]          # max_xcell = 3 nxcell: shown on the CPU
    assert not _same(want.px, q.px) and not _same(moved.px, want.px)
    p, dev = _device_particles(jr, q, fields)
    dVx, dVy = _up(Vx), _up(Vy)
    n0 = _launches(h)
    jr.advection_(p, jr.RungeKutta2(), (dVx, dVy), 1.0, handle=h)
    assert _launches(h) == n0 + 1
    _assert_state(jr, p, dev, want, fields, "advect")
    assert _same(jr.to_numpy(dVx), Vx) and _same(jr.to_numpy(dVy), Vy)
    got = jr.move_particles_(p, dev, handle=h)
    assert _launches(h) == n0 + 2 and got == c
    _assert_state(jr, p, dev, moved, mfields, "move")          # no sentinel survives: every slot of the destination was written
    # the buffers that were read still hold the advected state
    assert _same(jr.to_numpy(p._coords2[0]), want.px) and _same(jr.to_numpy(p._twins[id(dev[2])][1]), fields[2])


@pytest.mark.parametrize("ni", SHAPES)
def test_a_velocity_converging_on_one_column_overflows_its_cells(jr, h, ni):
    q, fields = _cloud(ni)
    xm = ORIGIN[0] + (ni[0] // 2 + 0.5) * DX
    Vx, Vy = _V(ni, lambda X, Y: -0.9 * DX * np.tanh((X - xm) / DX), lambda X, Y: 0.0 * X)
    p, dev = _device_particles(jr, q, fields[:1])
    dV = (_up(Vx), _up(Vy))
    f, overflowed = fields[:1], 0
    for step in range(3):
        PT.advect_rk2(q, Vx, Vy, 1.0)
        q, f, c = PT.move(q, f)
        assert c["n_far"] == 0 and c["n_outside"] == 0
        jr.advection_(p, jr.RungeKutta2(), dV, 1.0, handle=h)
        got, msg = _move(jr, p, dev, h)
        assert got == c, (step, got, c)
        assert (msg is not None) == (c["n_overflow"] > 0) and (msg is None or "n_overflow" in msg)
        _assert_state(jr, p, dev, q, f, f"step {step}")
        overflowed += c["n_overflow"]
    assert overflowed > 0 and int(q.active[ni[0] // 2].sum()) == ni[1] * MAX_XCELL          # the column is full


@pytest.mark.parametrize("ni", SHAPES)
@pytest.mark.parametrize("courant,lost", [(0.8, "n_outside"), (1.7, "n_far")])
def test_outflow_through_the_right_wall_and_a_step_of_more_than_one_cell(jr, h, ni, courant, lost):
    q, fields = _cloud(ni)
    Vx, Vy = _V(ni, lambda X, Y: courant * DX + 0.0 * X, lambda X, Y: 0.0 * X)
    PT.advect_rk2(q, Vx, Vy, 1.0)
    moved, mf, c = PT.move(q, fields[1:2])
    assert c[lost] > 0 and c["n_outside"] > 0 and (c["n_far"] > 0) == (courant > 1.0) and c["n_overflow"] == 0
    p, dev = _device_particles(jr, _cloud(ni)[0], fields[1:2])
    jr.advection_(p, jr.RungeKutta2(), (_up(Vx), _up(Vy)), 1.0, handle=h)
    got, msg = _move(jr, p, dev, h)
    assert got == c and (msg is not None) == (courant > 1.0) and (msg is None or "n_far" in msg)
    _assert_state(jr, p, dev, moved, mf)


@pytest.mark.parametrize("ni", SHAPES)
def test_a_nan_coordinate_is_counted_outside_and_nothing_else_changes(jr, h, ni):
    q, fields = _cloud(ni)
    Vx, Vy = _rotation(ni, 0.3)
    clean = PT.copy(q)
    q.px[ni[0] // 2, ni[1] // 2, 1] = np.nan
    want = PT.copy(q)
    PT.advect_rk2(want, Vx, Vy, 1.0)
    PT.advect_rk2(clean, Vx, Vy, 1.0)
    at = (ni[0] // 2, ni[1] // 2, 1)          # the particle is left as it was, y included; every other particle moves as without it
    assert np.isnan(want.px[at]) and want.py[at] == q.py[at] and int((_bits(want.px) != _bits(clean.px)).sum()) == 1
    assert int((_bits(want.py) != _bits(clean.py)).sum()) == 1 and want.py[at] != clean.py[at]
    moved, _, c = PT.move(want)
    _, _, c_clean = PT.move(clean)
    assert c["n_outside"] == c_clean["n_outside"] + 1 and c["n_active_after"] == c_clean["n_active_after"] - 1 and not np.isnan(moved.px).any()
    p, _ = _device_particles(jr, q)
    jr.advection_(p, jr.RungeKutta2(), (_up(Vx), _up(Vy)), 1.0, handle=h)
    _assert_state(jr, p, (), want, (), "advect")
    got, msg = _move(jr, p, (), h)          # nargs = 0
    assert got == c and msg is None
    _assert_state(jr, p, (), moved, (), "move")


def test_ten_advect_and_move_steps_in_a_row(jr, h):
    ni = (33, 17)
    q, fields = _cloud(ni)
    Vx, Vy = _rotation(ni)
    p, dev = _device_particles(jr, q, fields)
    dV = (_up(Vx), _up(Vy))
    f = fields
    for step in range(10):
        PT.advect_rk2(q, Vx, Vy, 1.0)
        q, f, c = PT.move(q, f)
        assert c["n_far"] == 0 and c["n_overflow"] == 0
        jr.advection_(p, jr.RungeKutta2(), dV, 1.0, handle=h)
        assert jr.move_particles_(p, dev, handle=h) == c, step
    _assert_state(jr, p, dev, q, f, "after ten steps")
    assert q.active.sum() > 0.5 * NXCELL * ni[0] * ni[1]


# ---------------------------------------------------------------------------------------------- interpolation
@pytest.mark.parametrize("ni", SHAPES)
def test_grid2particle_and_particle2grid_bit_for_bit(jr, h, ni):
    q, fields = _cloud(ni)
    Vx, Vy = _rotation(ni)
    PT.advect_rk2(q, Vx, Vy, 1.0)          # particles that have left their bucket cell: the weights are those of the bucket
    q.active[1:3, 1:3, :] = 0
    q.px[1:3, 1:3, :], q.py[1:3, 1:3, :] = 0.0, 0.0          # the vertex (2, 2) has no particle around it
    rng = np.random.default_rng(3)
    F = np.asfortranarray(rng.uniform(-2.0, 5.0, (ni[0] + 1, ni[1] + 1)))
    p, (pF,) = _device_particles(jr, q, (np.full(q.px.shape, SENTINEL),))
    dF = _up(F)
    n0 = _launches(h)
    jr.grid2particle_(pF, dF, p, handle=h)
    want = PT.grid2particle(F, q)
    assert _same(jr.to_numpy(pF), want) and np.all(want[q.active == 0] == 0.0) and _same(jr.to_numpy(dF), F)
    pT = np.where(q.active != 0, fields[1], 0.0)
    pF.copy_(_up(pT))
    G0 = np.asfortranarray(np.full(F.shape, SENTINEL))
    dG = _up(G0)
    jr.particle2grid_(dG, pF, p, handle=h)
    G = PT.particle2grid(G0, pT, q)
    assert _same(jr.to_numpy(dG), G) and G[2, 2] == SENTINEL and (G == SENTINEL).sum() == 1 and _launches(h) == n0 + 2
    _assert_state(jr, p, (pF,), q, (pT,))


# ---------------------------------------------------------------------------------------------- phase ratios
@pytest.mark.parametrize("nphase", [1, 3, 8])
@pytest.mark.parametrize("ni", SHAPES)
def test_phase_ratios_bit_for_bit_with_a_block_of_emptied_cells(jr, h, ni, nphase):
    """phases 1 .. 3 (some 0.0 and 9.0 planted: skipped) for every phase count: with nphase = 1 two thirds of the particles are skipped; the particles have been
    advected out of their bucket cells, and a 2 x 3 block of cells is empty"""
    q, fields = _cloud(ni)
    Vx, Vy = _rotation(ni)
    PT.advect_rk2(q, Vx, Vy, 1.0)
    q.active[3:5, 1:4, :] = 0
    q.px[3:5, 1:4, :], q.py[3:5, 1:4, :] = 0.0, 0.0
    ph = np.where(q.active != 0, fields[0], 0.0)
    if nphase == 8:
        ph = np.where(q.active != 0, 1.0 + (np.arange(ph.size).reshape(ph.shape) * 5) % 8, 0.0)
    ph[0, 0, 0], ph[ni[0] - 1, ni[1] - 1, 1] = 0.0, 9.0
    old = {m: np.asfortranarray(np.full(PT.member_shape(m, ni, nphase), SENTINEL)) for m in PT.MEMBERS}
    want, n_empty = PT.phase_ratios(old, ph, nphase, q)
    assert n_empty >= 2 + 2 + 3 + 2          # the centres, the inner vertices and the inner faces of the emptied block at the least
    p, (dph,) = _device_particles(jr, q, (ph,))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, nphase, ni)
    for m in PT.MEMBERS:
        getattr(pr, m).fill_(SENTINEL)
    n0 = _launches(h)
    got = jr.update_phase_ratios_(pr, p, dph, handle=h)
    assert got == n_empty and _launches(h) == n0 + 1
    for m in PT.MEMBERS:
        g = jr.to_numpy(getattr(pr, m))
        assert _same(g, want[m]), (m, int((_bits(g) != _bits(want[m])).sum()))
    assert np.all(want["center"][:, 3:5, 1:4] == SENTINEL) and np.all(want["vertex"][:, 4, 2:4] == SENTINEL)          # unchanged there
    filled = want["center"][:, want["center"][0] != SENTINEL]
    assert np.abs(filled.sum(axis=0) - 1.0).max() < 1e-14
    _assert_state(jr, p, (dph,), q, (ph,))


# ---------------------------------------------------------------------------------------------- refusals
def test_the_library_refuses_with_status_4_a_text_and_no_launch(jr, h):
    from justrelax_jl_amd import _lib
    ni = (7, 5)
    q, fields = _cloud(ni)
    p, dev = _device_particles(jr, q, fields[:2])
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    F = jr.fzeros((8, 6), _dev())
    L, P = h.lib, lambda t: C.c_void_p(t.data_ptr())
    before = (_host(jr, p), jr.to_numpy(dev[0]))
    n0 = _launches(h)

    def S(second=False, **kw):
        s = p._struct(second)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def refused(status, text):
        assert status == 4 and text in L.jrx_last_error(h._h).decode(), (status, text, L.jrx_last_error(h._h).decode())
        assert _launches(h) == n0

    adv = lambda s, vx=P(st.V.Vx), vy=P(st.V.Vy), dt=0.1: L.jrx_particles2d_advect_rk2(h._h, C.byref(s), vx, vy, C.c_double(dt))
    refused(L.jrx_particles2d_advect_rk2(h._h, None, P(st.V.Vx), P(st.V.Vy), C.c_double(0.1)), "particles is NULL")
    refused(adv(S(px=None)), "particles.px is NULL")
    refused(adv(S(active=None)), "particles.active is NULL")
    refused(adv(S(nx=0)), "0 x 5 cells")
    refused(adv(S(max_xcell=0)), "max_xcell = 0")
    refused(adv(S(nx=65536, ny=65536)), "2^31")          # refused on the extents alone: nothing is read
    refused(adv(S(dx=-DX)), "spacings")
    refused(adv(S(dy=float("inf"))), "spacings")
    refused(adv(S(x0=float("nan"))), "origin")
    refused(adv(S(_dx=1.0)), "not 1 / dx")
    refused(adv(S(), vx=None), "V.Vx is NULL")
    refused(adv(S(), dt=float("nan")), "dt = nan")
    refused(adv(S(), vx=P(p.coords[0])), "V.Vx overlaps")

    a_src, a_dst = (C.c_void_p * 2)(*(d.data_ptr() for d in dev)), (C.c_void_p * 2)(*(p._twins[id(d)][1].data_ptr() for d in dev))
    counts = (C.c_int64 * 5)(*([-1] * 5))
    mv = lambda s, d, a=a_src, b=a_dst, n=2, c=counts: L.jrx_particles2d_move(h._h, C.byref(s), C.byref(d), a, b, C.c_int32(n), c)
    refused(mv(S(), S(True), n=9), "9 particle fields")
    refused(mv(S(), S(True), n=-1), "-1 particle fields")
    refused(mv(S(), S(True), a=None), "args_src is NULL")
    refused(mv(S(), S(True), c=None), "counts is NULL")
    refused(mv(S(), S(True, max_xcell=6)), "differ")
    refused(mv(S(), S(True, x0=0.0)), "differ")
    refused(mv(S(), S()), "overlaps the particle coordinates")          # in place
    refused(mv(S(), S(True), b=a_src), "overlaps source particle field")
    refused(mv(S(), S(True), b=(C.c_void_p * 2)(a_dst[0], a_dst[0])), "two arrays of the destination overlap")
    refused(mv(S(), S(True), a=(C.c_void_p * 2)(a_src[0], None)), "particle field 2 (source) is NULL")
    assert list(counts) == [-1] * 5

    refused(L.jrx_particles2d_grid2particle(h._h, None, P(F), C.byref(S())), "pF is NULL")
    refused(L.jrx_particles2d_grid2particle(h._h, P(p.coords[1]), P(F), C.byref(S())), "pF overlaps")
    refused(L.jrx_particles2d_particle2grid(h._h, P(F), None, C.byref(S())), "pF is NULL")
    refused(L.jrx_particles2d_particle2grid(h._h, P(dev[0]), P(dev[0]), C.byref(S())), "F overlaps pF")
    ne = C.c_int64(-1)
    mem = [P(getattr(pr, m)) for m in PT.MEMBERS]
    ratios = lambda m=mem, ph=P(dev[0]), n=2, e=C.byref(ne): L.jrx_particles2d_phase_ratios(h._h, *m, ph, C.c_int32(n), C.byref(S()), e)
    refused(ratios(n=0), "0 phases")
    refused(ratios(n=9), "9 phases")
    refused(ratios(m=[mem[0], None, mem[2], mem[3]]), "phase_ratios.vertex is NULL")
    refused(ratios(ph=None), "pPhases is NULL")
    refused(ratios(e=None), "n_empty is NULL")
    refused(ratios(m=[mem[0], mem[1], mem[2], mem[2]]), "phase_ratios.Vx and phase_ratios.Vy overlap")
    refused(ratios(m=[P(dev[0])] + mem[1:]), "phase_ratios.center overlaps pPhases")
    assert ne.value == -1
    # nothing was written
    after = (_host(jr, p), jr.to_numpy(dev[0]))
    assert all(_same(a, b) for a, b in zip(before[0], after[0])) and _same(before[1], after[1])
    assert float(pr.center.abs().max()) == 0.0 and float(pr.vertex.abs().max()) == 0.0
    # the wrappers look at the device of every operand
    with pytest.raises(ValueError, match="pF is on cpu"):
        jr.grid2particle_(jr.fzeros(p.shape, "cpu"), F, p, handle=h)
    with pytest.raises(ValueError, match="V.Vx is on cpu"):
        jr.advection_(p, jr.RungeKutta2(), (jr.fzeros((8, 7), "cpu"), st.V.Vy), 0.1, handle=h)
    assert _launches(h) == n0
