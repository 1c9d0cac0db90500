"""GPU: the 3D particle operators (advection_, move_particles_, grid2particle_, particle2grid_, centroid2particle_, particle2centroid_, update_phase_ratios_;
csrc/particles3d.hip through the seven jrx_particles3d_* entry points) against the NumPy restatement (tests/_particles3d.py, pinned by
tests/test_particles3d_restatement.py): coordinates, mask, particle fields, grid fields, ratios and counters BIT FOR BIT (compared as 64-bit patterns: the
kernels have no fma, the library is built without contraction, every kernel is a gather in a fixed order), the inputs untouched, sentinel-filled outputs fully
written or left alone where the definition says "kept", and every refusal with "stat_particles_launches" unchanged.

Sizes: the kernels run 64 x 2 x 2 blocks.  (5, 4, 3) is smaller than a block along x and ragged in z; (67, 9, 6) exceeds the block extent along every axis by a
ragged remainder (x: one block and 3 cells; y: four blocks and 1; z: and its node box of 7 three blocks and 1).  nxcell = 8, max_xcell = 12, jittered seeding;
three phases, a temperature and an identity field.  Where a test asserts that a counter is zero or positive, the restatement shows it on the CPU before the
device is asked.  The move runs in both forms (tuning key particles3d_move_codes = 1 and 0) against the same expected bits, the phase ratios as one launch and as
two.  The helpers shared with the 2D files are in tests/_particles_gpu.py.  Not exercised: the refusal of a handle with a communicator (it needs a second
rank)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _particles3d as PT
from _particles_gpu import D, MAX_XCELL, NXCELL, ORIGIN, SENTINEL, _V, _assert_state, _bits, _cloud, _cloud0, _dev, _device_particles, _host, _host_int, _launches, _move
from _particles_gpu import _rotation, _same, _up
from _particles_gpu import h          # noqa: F401 -- the module's handle, a fixture

pytestmark = pytest.mark.gpu
SHAPES = [(5, 4, 3), (67, 9, 6)]
NXCELL = NXCELL[3]


@functools.lru_cache(maxsize=None)
def _advected0(ni):
    """the cloud after one rotation step, not yet moved: particles that have left their bucket cells"""
    q, fields = _cloud(ni)
    PT.advect_rk2(q, _rotation(ni), 1.0)
    return q, fields


def _advected(ni):
    q, f = _advected0(ni)
    return PT.copy(q), tuple(x.copy() for x in f)


def _move_both_forms(jr, h, src, fields, want, wfields, c, what=""):
    """the device move of the cloud `src` in the codes form and in the direct form against the same expected state; the buffers that were read stay as they were"""
    for codes in (1, 0):
        p, dev = _device_particles(jr, src, fields)
        h.set_option("particles3d_move_codes", codes)
        try:
            n0 = _launches(h)
            got, msg = _move(jr, p, dev, h)
            assert _launches(h) == n0 + (2 if codes else 1)
        finally:
            h.set_option("particles3d_move_codes", 1)
        assert got == c, (what, codes, got, c)
        lost = [k for k in ("n_far", "n_overflow") if c[k]]
        assert (msg is not None) == bool(lost) and (msg is None or lost[0] in msg)
        _assert_state(jr, p, dev, want, wfields, f"{what} codes={codes}")          # no sentinel survives: every slot of the destination was written
        assert _same(jr.to_numpy(p._coords2[2]), src.pz) and _same(_host_int(p._index2), src.active)
        for d, f in zip(dev, fields):
            assert _same(jr.to_numpy(p._twins[id(d)][1]), f)


# ---------------------------------------------------------------------------------------------- advect + move
@pytest.mark.parametrize("ni", SHAPES)
def test_a_rigid_rotation_at_courant_half_advects_and_moves_bit_for_bit(jr, h, ni):
    q, fields = _cloud(ni)
    V = _rotation(ni)
    want, _ = _advected(ni)
    moved, mfields, c = PT.move(want, fields)
    assert c["n_far"] == 0 and c["n_active_after"] > 0.9 * c["n_active_before"]          # shown on the CPU (a few of the larger grid's buckets overflow: 12 slots for 8 seeded)
    assert not _same(want.pz, q.pz) and not _same(moved.px, want.px)
    p, dev = _device_particles(jr, q, fields)
    dV = tuple(_up(v) for v in V)
    n0 = _launches(h)
    jr.advection_(p, jr.RungeKutta2(), dV, 1.0, handle=h)
    assert _launches(h) == n0 + 1
    _assert_state(jr, p, dev, want, fields, "advect")
    assert all(_same(jr.to_numpy(d), v) for d, v in zip(dV, V))
    for nf in (3, 1, 0):
        _move_both_forms(jr, h, want, fields[:nf], moved, mfields[:nf], c, f"{nf} fields")


@pytest.mark.parametrize("ni", SHAPES)
def test_diagonal_translations_send_particles_through_all_26_offsets_and_out_of_the_grid(jr, h, ni):
    seen = set()
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                q, fields = _cloud(ni)
                u = (0.9 * sx * D[0], 0.9 * sy * D[1], 0.9 * sz * D[2])
                V = _V(ni, lambda X, Y, Z: u[0] + 0.0 * X, lambda X, Y, Z: u[1] + 0.0 * X, lambda X, Y, Z: u[2] + 0.0 * X)
                PT.advect_rk2(q, V, 1.0)
                inside, d = PT.owners(q)
                seen |= set(zip(d[0][inside].tolist(), d[1][inside].tolist(), d[2][inside].tolist()))
                moved, mf, c = PT.move(q, fields[2:])
                assert c["n_outside"] > 0 and c["n_far"] == 0          # shown on the CPU
                if (sx, sy, sz) in ((1, 1, 1), (-1, 1, -1)) or ni == SHAPES[0]:
                    p, dev = _device_particles(jr, _cloud(ni)[0], fields[2:])
                    jr.advection_(p, jr.RungeKutta2(), tuple(_up(v) for v in V), 1.0, handle=h)
                    _assert_state(jr, p, dev, q, fields[2:], "advect")
                    _move_both_forms(jr, h, q, fields[2:], moved, mf, c, str((sx, sy, sz)))
    assert seen == set(PT.NEIGHBOURS) | {(0, 0, 0)}


@pytest.mark.parametrize("ni", SHAPES)
def test_a_compression_overflows_a_bucket_and_a_long_step_is_far(jr, h, ni):
    q, fields = _cloud(ni)
    m = [ORIGIN[d] + (ni[d] // 2 + 0.5) * D[d] for d in range(3)]
    V = _V(ni, lambda X, Y, Z: -0.9 * D[0] * np.tanh((X - m[0]) / D[0]), lambda X, Y, Z: -0.9 * D[1] * np.tanh((Y - m[1]) / D[1]), lambda X, Y, Z: 0.0 * X)
    PT.advect_rk2(q, V, 1.0)
    moved, mf, c = PT.move(q, fields[:1])
    assert c["n_overflow"] > 0 and c["n_far"] == 0 and c["n_outside"] == 0          # shown on the CPU
    assert int(moved.active[ni[0] // 2, ni[1] // 2].sum()) == ni[2] * MAX_XCELL          # the column is full
    _move_both_forms(jr, h, q, fields[:1], moved, mf, c, "compression")
    q, fields = _cloud(ni)
    V = _V(ni, lambda X, Y, Z: 0.0 * X, lambda X, Y, Z: 0.0 * X, lambda X, Y, Z: 1.7 * D[2] + 0.0 * X)
    PT.advect_rk2(q, V, 1.0)
    q.py[ni[0] // 2, ni[1] // 2, 1, 1] = np.nan
    moved, mf, c = PT.move(q, fields[1:2])
    assert c["n_far"] > 0 and c["n_outside"] > 0 and c["n_overflow"] == 0 and not np.isnan(moved.py).any()
    _move_both_forms(jr, h, q, fields[1:2], moved, mf, c, "far")


def test_a_nan_coordinate_is_left_alone_by_the_advection(jr, h):
    ni = SHAPES[0]
    q, _ = _cloud(ni)
    V = _rotation(ni, 0.3)
    at = (2, 1, 1, 3)
    q.pz[at] = np.nan
    want = PT.copy(q)
    PT.advect_rk2(want, V, 1.0)
    assert np.isnan(want.pz[at]) and want.px[at] == q.px[at] and int((_bits(want.px) == _bits(q.px)).sum()) == int((q.active == 0).sum()) + 1
    p, _ = _device_particles(jr, q)
    jr.advection_(p, jr.RungeKutta2(), tuple(_up(v) for v in V), 1.0, handle=h)
    _assert_state(jr, p, (), want, (), "advect")


# ---------------------------------------------------------------------------------------------- interpolation
@pytest.mark.parametrize("ni", SHAPES)
def test_the_four_interpolations_bit_for_bit(jr, h, ni):
    q, fields = _advected(ni)          # particles that have left their bucket cell: the vertex weights are those of the bucket
    q.active[1:3, 1:3, 0:2, :] = 0
    for c in (q.px, q.py, q.pz):
        c[1:3, 1:3, 0:2, :] = 0.0          # the vertices (2, 2, 0) (on the low z face) and (2, 2, 1) have no particle around them, eight centres neither
    q.px[0, 0, 0, 0] = np.inf          # centroid2particle leaves this slot as it was
    rng = np.random.default_rng(3)
    Fv = np.asfortranarray(rng.uniform(-2.0, 5.0, tuple(n + 1 for n in ni)))
    Fc = np.asfortranarray(rng.uniform(-2.0, 5.0, ni))
    p, (pF,) = _device_particles(jr, q, (np.full(q.px.shape, SENTINEL),))
    dFv, dFc = _up(Fv), _up(Fc)
    n0 = _launches(h)
    jr.grid2particle_(pF, dFv, p, handle=h)
    want = PT.grid2particle(Fv, q)
    assert _same(jr.to_numpy(pF), want) and np.all(want[q.active == 0] == 0.0) and _same(jr.to_numpy(dFv), Fv)
    pF.fill_(SENTINEL)
    jr.centroid2particle_(pF, dFc, p, handle=h)
    want = PT.centroid2particle(np.full(q.px.shape, SENTINEL), Fc, q)
    assert _same(jr.to_numpy(pF), want) and want[0, 0, 0, 0] == SENTINEL and (want == SENTINEL).sum() == 1 and _same(jr.to_numpy(dFc), Fc)
    q.px[0, 0, 0, 0] = _cloud0(ni)[0].px[0, 0, 0, 0]
    p.coords[0].copy_(_up(q.px))
    pT = np.where(q.active != 0, fields[1], 0.0)
    pF.copy_(_up(pT))
    G0, C0 = np.asfortranarray(np.full(Fv.shape, SENTINEL)), np.asfortranarray(np.full(Fc.shape, SENTINEL))
    dG, dC = _up(G0), _up(C0)
    jr.particle2grid_(dG, pF, p, handle=h)
    jr.particle2centroid_(dC, pF, p, handle=h)
    G, Cn = PT.particle2grid(G0, pT, q), PT.particle2centroid(C0, pT, q)
    assert _same(jr.to_numpy(dG), G) and G[2, 2, 0] == G[2, 2, 1] == SENTINEL and (G == SENTINEL).sum() == 2
    assert _same(jr.to_numpy(dC), Cn) and (Cn[1:3, 1:3, 0:2] == SENTINEL).all() and (Cn == SENTINEL).sum() == 8
    assert _launches(h) == n0 + 4
    _assert_state(jr, p, (pF,), q, (pT,))


# ---------------------------------------------------------------------------------------------- phase ratios
@pytest.mark.parametrize("nphase", [1, 3, 8])
@pytest.mark.parametrize("ni", SHAPES)
def test_phase_ratios_bit_for_bit_with_an_emptied_cell(jr, h, ni, nphase):
    """phases 1 .. 3 (a 0.0 and a 9.0 planted: skipped) for every phase count: with nphase = 1 two thirds of the particles are skipped; the particles have been
    advected out of their bucket cells, and a block of cells is empty.  One launch and two launches leave the same bits."""
    q, fields = _advected(ni)
    q.active[3:5, 1:3, 1:3, :] = 0
    for c in (q.px, q.py, q.pz):
        c[3:5, 1:3, 1:3, :] = 0.0
    ph = np.where(q.active != 0, fields[0], 0.0)
    if nphase == 8:
        ph = np.where(q.active != 0, 1.0 + (np.arange(ph.size).reshape(ph.shape) * 5) % 8, 0.0)
    ph[0, 0, 0, 0], ph[ni[0] - 1, ni[1] - 1, ni[2] - 1, 1] = 0.0, 9.0
    old = {m: np.asfortranarray(np.full(PT.member_shape(m, ni, nphase), SENTINEL)) for m in PT.MEMBERS}
    want, n_empty = PT.phase_ratios(old, ph, nphase, q)
    assert n_empty >= 8 + 1          # the centres of the emptied block and the vertex inside it at the least
    assert np.all(want["center"][:, 3:5, 1:3, 1:3] == SENTINEL) and np.all(want["vertex"][:, 4, 2, 2] == SENTINEL)          # unchanged there
    for m in PT.MEMBERS:
        filled = want[m][:, want[m][0] != SENTINEL]
        assert filled.size and np.abs(filled.sum(axis=0) - 1.0).max() < 1e-14
    p, (dph,) = _device_particles(jr, q, (ph,))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, nphase, ni)
    for split in (0, 1, 2):          # one launch, two, the default: two at nphase = 8
        for m in PT.MEMBERS:
            getattr(pr, m).fill_(SENTINEL)
        h.set_option("particles3d_ratios_split", split)
        try:
            n0 = _launches(h)
            got = jr.update_phase_ratios_(pr, p, dph, handle=h)
            assert got == n_empty and _launches(h) == n0 + (2 if split == 1 or (split == 2 and nphase == 8) else 1)
        finally:
            h.set_option("particles3d_ratios_split", 2)
        for m in PT.MEMBERS:
            g = jr.to_numpy(getattr(pr, m))
            assert _same(g, want[m]), (m, split, int((_bits(g) != _bits(want[m])).sum()))
    _assert_state(jr, p, (dph,), q, (ph,))


# ---------------------------------------------------------------------------------------------- the chain through the Python API
def test_a_chained_step_through_the_python_api(jr, h):
    ni = (9, 5, 4)
    g = jr.Geometry(ni, tuple(n * d for n, d in zip(ni, D)), origin=ORIGIN)
    mk = lambda: np.random.default_rng(99)
    q = PT.init_particles(NXCELL, 2 * MAX_XCELL, 2, *g.xi_vel, rng=mk())          # 24 slots: no bucket overflows, so the wrapper's move does not raise
    p = jr.init_particles(jr.AMDGPUBackend, NXCELL, 2 * MAX_XCELL, 2, *g.xi_vel, rng=mk())
    _assert_state(jr, p, (), q, ())
    a = q.active != 0
    ph = np.where(a, 1.0 + (q.pz > q.z0 + 0.5 * ni[2] * q.dz), 0.0)
    pT = np.where(a, 300.0 + 1000.0 * (q.px - q.x0), 0.0)
    dph, dT = jr.init_cell_arrays(p, 2)
    dph.copy_(_up(ph)), dT.copy_(_up(pT))
    c = [q.x0 + 0.5 * ni[0] * q.dx, q.y0 + 0.5 * ni[1] * q.dy]
    w = 0.5 * min(q.dx, q.dy) / np.hypot(0.5 * ni[0] * q.dx, 0.5 * ni[1] * q.dy)
    V = []
    for grids, f in zip(g.xi_vel, (lambda X, Y, Z: -w * (Y - c[1]), lambda X, Y, Z: w * (X - c[0]), lambda X, Y, Z: 0.25 * q.dz + 0.0 * X)):
        X, Y, Z = np.meshgrid(*grids, indexing="ij")
        V.append(np.asfortranarray(f(X, Y, Z)))
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    for d, v in zip((st.V.Vx, st.V.Vy, st.V.Vz), V):
        d.copy_(_up(v))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    T = jr.fzeros(ni, _dev())
    Tn, old = np.zeros(ni), {m: np.zeros(PT.member_shape(m, ni, 2)) for m in PT.MEMBERS}
    f = (ph, pT)
    for step in range(2):
        PT.advect_rk2(q, V, 1.0)
        q, f, cn = PT.move(q, f)
        assert cn["n_far"] == 0 and cn["n_overflow"] == 0 and (step == 0 or cn["n_outside"] > 0)
        Tn = PT.particle2centroid(Tn, f[1], q)
        old, n_empty = PT.phase_ratios(old, f[0], 2, q)
        jr.advection_(p, jr.RungeKutta2(), st.V, 1.0, grid=g, handle=h)
        assert jr.move_particles_(p, (dph, dT), handle=h) == cn
        jr.particle2centroid_(T, dT, p, handle=h)
        assert jr.update_phase_ratios_(pr, p, dph, handle=h) == n_empty
    _assert_state(jr, p, (dph, dT), q, f, "two steps")
    assert _same(jr.to_numpy(T), np.asfortranarray(Tn))
    for m in PT.MEMBERS:
        assert _same(jr.to_numpy(getattr(pr, m)), old[m]), m


# ---------------------------------------------------------------------------------------------- refusals
def test_the_library_refuses_with_status_4_a_text_and_no_launch(jr, h):
    ni = SHAPES[0]
    q, fields = _cloud(ni)
    p, dev = _device_particles(jr, q, fields[:2])
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    Fv, Fc = jr.fzeros(tuple(n + 1 for n in ni), _dev()), jr.fzeros(ni, _dev())
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

    Vp = [P(st.V.Vx), P(st.V.Vy), P(st.V.Vz)]
    adv = lambda s, v=Vp, dt=0.1: L.jrx_particles3d_advect_rk2(h._h, C.byref(s), *v, C.c_double(dt))
    refused(L.jrx_particles3d_advect_rk2(h._h, None, *Vp, C.c_double(0.1)), "particles is NULL")
    refused(adv(S(pz=None)), "particles.pz is NULL")
    refused(adv(S(active=None)), "particles.active is NULL")
    refused(adv(S(nz=0)), "5 x 4 x 0 cells")
    refused(adv(S(max_xcell=0)), "max_xcell = 0")
    refused(adv(S(nx=2048, ny=1024, nz=1024, max_xcell=1)), "2^31")          # 2^31 slots: refused on the scalars alone, nothing is read
    refused(adv(S(nx=1 << 20, ny=1 << 20, nz=1 << 20)), "2^31")
    refused(adv(S(dz=-D[2])), "spacings")
    refused(adv(S(dy=float("inf"))), "spacings")
    refused(adv(S(z0=float("nan"))), "origin")
    refused(adv(S(_dz=1.0)), "not 1 / dx")
    refused(adv(S(), v=Vp[:2] + [None]), "V.Vz is NULL")
    refused(adv(S(), dt=float("nan")), "dt = nan")
    refused(adv(S(), v=[P(p.coords[2])] + Vp[1:]), "V.Vx overlaps")

    a_src, a_dst = (C.c_void_p * 2)(*(d.data_ptr() for d in dev)), (C.c_void_p * 2)(*(p._twins[id(d)][1].data_ptr() for d in dev))
    counts = (C.c_int64 * 5)(*([-1] * 5))
    work = P(p._work)
    mv = lambda s, d, a=a_src, b=a_dst, n=2, w=work, c=counts: L.jrx_particles3d_move(h._h, C.byref(s), C.byref(d), a, b, C.c_int32(n), w, c)
    refused(mv(S(), S(True), n=9), "9 particle fields")
    refused(mv(S(), S(True), n=-1), "-1 particle fields")
    refused(mv(S(), S(True), a=None), "args_src is NULL")
    refused(mv(S(), S(True), c=None), "counts is NULL")
    refused(mv(S(), S(True, max_xcell=6)), "differ")
    refused(mv(S(), S(True, z0=0.0)), "differ")
    refused(mv(S(), S()), "overlaps the particle coordinates")          # in place: src and dst share every array
    refused(mv(S(), S(True, pz=p.coords[2].data_ptr())), "overlaps the particle coordinates")          # ... or one
    refused(mv(S(), S(True), w=P(p.index)), "work overlaps")
    refused(mv(S(), S(True), w=P(p._coords2[0])), "two arrays of the destination overlap")
    refused(mv(S(), S(True), b=a_src), "overlaps source particle field")
    refused(mv(S(), S(True), b=(C.c_void_p * 2)(a_dst[0], a_dst[0])), "two arrays of the destination overlap")
    refused(mv(S(), S(True), a=(C.c_void_p * 2)(a_src[0], None)), "particle field 2 (source) is NULL")
    assert list(counts) == [-1] * 5

    refused(L.jrx_particles3d_grid2particle(h._h, None, P(Fv), C.byref(S())), "pF is NULL")
    refused(L.jrx_particles3d_grid2particle(h._h, P(p.coords[1]), P(Fv), C.byref(S())), "pF overlaps")
    refused(L.jrx_particles3d_particle2grid(h._h, P(Fv), None, C.byref(S())), "pF is NULL")
    refused(L.jrx_particles3d_particle2grid(h._h, P(dev[0]), P(dev[0]), C.byref(S())), "F overlaps pF")
    refused(L.jrx_particles3d_particle2centroid(h._h, None, P(dev[0]), C.byref(S())), "F is NULL")
    refused(L.jrx_particles3d_centroid2particle(h._h, P(dev[0]), P(Fc), C.byref(S(nz=1))), "every extent >= 2")
    refused(L.jrx_particles3d_centroid2particle(h._h, P(dev[0]), P(Fc), C.byref(S(nx=1))), "every extent >= 2")
    ne = C.c_int64(-1)
    mem = [getattr(pr, m).data_ptr() for m in PT.MEMBERS]
    ratios = lambda m=mem, ph=P(dev[0]), n=2, e=C.byref(ne): L.jrx_particles3d_phase_ratios(h._h, (C.c_void_p * 8)(*m), ph, C.c_int32(n), C.byref(S()), e)
    refused(ratios(n=0), "0 phases")
    refused(ratios(n=9), "9 phases")
    refused(ratios(m=mem[:5] + [None] + mem[6:]), "phase_ratios.yz is NULL")
    refused(L.jrx_particles3d_phase_ratios(h._h, None, P(dev[0]), C.c_int32(2), C.byref(S()), C.byref(ne)), "phase_ratios is NULL")
    refused(ratios(ph=None), "pPhases is NULL")
    refused(ratios(e=None), "n_empty is NULL")
    refused(ratios(m=mem[:7] + [mem[6]]), "phase_ratios.xz and phase_ratios.xy overlap")
    refused(ratios(m=[dev[0].data_ptr()] + mem[1:]), "phase_ratios.center overlaps pPhases")
    assert ne.value == -1
    # nothing was written
    after = (_host(jr, p), jr.to_numpy(dev[0]))
    assert all(_same(a, b) for a, b in zip(before[0], after[0])) and _same(before[1], after[1])
    assert all(float(getattr(pr, m).abs().max()) == 0.0 for m in PT.MEMBERS) and int(p._work.min()) == 99
    # work = NULL selects the direct form: one launch, the same bits as the codes form
    want, wf, c = PT.move(q, fields[:2])
    counts = (C.c_int64 * 5)()
    assert mv(S(), S(True), w=None, c=counts) == 0 and _launches(h) == n0 + 1 and dict(zip(PT.COUNTS, counts)) == c
    p._swap(dev)
    _assert_state(jr, p, dev, want, wf, "work = NULL")
    # the wrappers look at the device of every operand
    with pytest.raises(ValueError, match="pF is on cpu"):
        jr.grid2particle_(jr.fzeros(p.shape, "cpu"), Fv, p, handle=h)
    with pytest.raises(ValueError, match="V.Vz is on cpu"):
        jr.advection_(p, jr.RungeKutta2(), (st.V.Vx, st.V.Vy, jr.fzeros((7, 6, 4), "cpu")), 0.1, handle=h)
    assert _launches(h) == n0 + 1
