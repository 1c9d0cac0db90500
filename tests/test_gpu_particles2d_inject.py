"""GPU: inject_particles_phase_ (k_pt_inject of csrc/particles.hip through jrx_particles2d_inject) against the NumPy restatement of operator 12
(tests/_particles2d_inject.py, pinned by tests/test_particles2d_inject_restatement.py): the coordinates, both masks, the phases, every particle field and the five
counters BIT FOR BIT, the grid fields and every slot active at entry untouched, the output mask fully written, and every refusal with "stat_particles_launches"
unchanged and nothing written.

Shapes: (7, 5) is one block with ragged edges, (33, 17) has 561 cells in five blocks, (1, 6) has no x neighbours (vertex and donor fields only: centres need
nx >= 2), (128, 5) is the smallest shape whose launch has two block columns.  nxcell = 4 (a 2 x 2 lattice), max_xcell = 12; the cloud is that of
tests/test_gpu_particles2d.py (_cloud0 of tests/_particles_gpu.py).  Where a test needs a counter to be positive or
zero, the restatement shows it on the CPU before the device is asked.  Not exercised: the refusal of a handle with a communicator (it needs a second rank)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _particles2d as PT
import _particles2d_inject as INJ
from _particles_gpu import D, MAX_XCELL, NXCELL, ORIGIN, SENTINEL, _V, _assert_state, _bits, _cloud0, _dev, _device_particles, _host_int as _mask, _launches, _same, _up, _xvi
from _particles_gpu import h          # noqa: F401 -- the module's handle, a fixture

pytestmark = pytest.mark.gpu
SHAPES = [(7, 5), (33, 17), (1, 6), (128, 5)]
DX, DY = D[:2]
NXCELL = NXCELL[2]


def _flow(ni, kind, courant=0.5):
    cx, cy = ORIGIN[0] + 0.5 * ni[0] * DX, ORIGIN[1] + 0.5 * ni[1] * DY
    w = courant * min(DX, DY) / np.hypot(0.5 * ni[0] * DX, 0.5 * ni[1] * DY)          # dt = 1
    if kind == "rotation":
        return _V(ni, lambda X, Y: -w * (Y - cy), lambda X, Y: w * (X - cx))
    return _V(ni, lambda X, Y: w * (X - cx), lambda X, Y: w * (Y - cy))          # diverging


@functools.lru_cache(maxsize=None)
def _moved0(ni):
    """the cloud after one rotation step at Courant 0.5 and the move, on the CPU; a fourth and a fifth particle field, and two grid fields"""
    q, f = _cloud0(ni)
    q = PT.copy(q)
    Vx, Vy = _flow(ni, "rotation")
    PT.advect_rk2(q, Vx, Vy, 1.0)
    q, f, c = PT.move(q, f)
    assert c["n_far"] == 0 and c["n_overflow"] == 0
    a = q.active != 0
    rng = np.random.default_rng(11 + ni[0])
    extra = (np.where(a, rng.uniform(-1.0, 1.0, a.shape), 0.0), np.where(a, 42.0, 0.0))
    grids = (np.asfortranarray(rng.uniform(300.0, 1600.0, (ni[0] + 1, ni[1] + 1))), np.asfortranarray(rng.uniform(-2.0, 5.0, ni)))
    return q, tuple(f) + extra, grids


def _moved(ni):
    q, f, g = _moved0(ni)
    return PT.copy(q), [x.copy() for x in f], g


def _specs(ni):
    """which particle field takes what: (indices into the field list, grid fields, kinds) -- pT from a vertex field, the fourth field from a centre field (a
    vertex field where nx < 2), the identity from the donor; field 4 (the constant 42) is not listed"""
    centre = ni[0] >= 2
    return (1, 3, 2), (0, 1 if centre else 0, None), (INJ.VERTEX, INJ.CENTRE if centre else INJ.VERTEX, INJ.DONOR)


def _cpu(q, fields, grids, ni, min_xcell):
    """the restatement on q and fields in place; q.active becomes the new mask.  Returns (the mask at entry, counts)"""
    idx, gsel, locs = _specs(ni)
    entry = q.active.copy()
    out, c = INJ.inject(q, fields[0], [fields[k] for k in idx], [None if g is None else grids[g] for g in gsel], locs, min_xcell=min_xcell)
    assert np.array_equal(q.active, entry)
    q.active = out
    return entry, c


def _gpu(jr, h, p, dev, dgrids, ni, min_xcell):
    idx, gsel, _ = _specs(ni)
    return jr.inject_particles_phase_(p, dev[0], [dev[k] for k in idx], [None if g is None else dgrids[g] for g in gsel], min_xcell=min_xcell, handle=h)


# ---------------------------------------------------------------------------------------------- 1. one rotation step
@pytest.mark.parametrize("min_xcell", [3, 4])
@pytest.mark.parametrize("ni", SHAPES)
def test_an_injection_after_one_rotation_step_and_a_move_bit_for_bit(jr, h, ni, min_xcell):
    q, fields, grids = _moved(ni)
    p, dev = _device_particles(jr, q, fields)
    dgrids = tuple(_up(g) for g in grids)
    entry, c = _cpu(q, fields, grids, ni, min_xcell)
    print(ni, min_xcell, c)
    new = (q.active != 0) & (entry == 0)
    assert c["n_injected"] == int(new.sum()) > 0 and c["n_no_donor"] == 0 and c["n_deficient"] > 0          # shown on the CPU
    assert np.all(_bits(fields[4])[new] == 0) and np.all(fields[4][entry != 0] == 42.0)          # the field that is not listed keeps +0.0 in the new slots
    n0 = _launches(h)
    got = _gpu(jr, h, p, dev, dgrids, ni, min_xcell)
    assert _launches(h) == n0 + 1 and got == c, (got, c)
    _assert_state(jr, p, dev, q, fields)
    assert _same(_mask(p._index2), entry)          # the mask that was read, now the spare one
    assert all(_same(jr.to_numpy(d), g) for d, g in zip(dgrids, grids))
    # a second call finds nothing to do and writes the same mask again
    p._index2.fill_(-77)
    got = _gpu(jr, h, p, dev, dgrids, ni, min_xcell)
    assert got == dict(n_active_before=c["n_active_after"], n_active_after=c["n_active_after"], n_deficient=0, n_injected=0, n_no_donor=0)
    _assert_state(jr, p, dev, q, fields, "second call")


# ---------------------------------------------------------------------------------------------- 2. a loop
@pytest.mark.parametrize("ni", SHAPES)
def test_four_steps_of_advect_move_inject_in_a_diverging_flow(jr, h, ni):
    q, fields = _cloud0(ni)
    q, fields = PT.copy(q), [x.copy() for x in fields]
    Vx, Vy = _flow(ni, "diverging")
    Tv = np.asfortranarray(np.random.default_rng(5).uniform(300.0, 1600.0, (ni[0] + 1, ni[1] + 1)))
    p, dev = _device_particles(jr, q, fields)
    for d in dev:
        p._twins[id(d)][1].fill_(SENTINEL)
    p._coords2[0].fill_(SENTINEL), p._coords2[1].fill_(SENTINEL)
    dV, dTv = (_up(Vx), _up(Vy)), _up(Tv)
    lost = injected = 0
    for step in range(4):
        PT.advect_rk2(q, Vx, Vy, 1.0)
        jr.advection_(p, jr.RungeKutta2(), dV, 1.0, handle=h)
        _assert_state(jr, p, dev, q, fields, f"advect {step}")
        q, fields, c = PT.move(q, fields)
        assert c["n_far"] == 0 and c["n_overflow"] == 0
        assert jr.move_particles_(p, dev, handle=h) == c, step
        _assert_state(jr, p, dev, q, fields, f"move {step}")
        lost += c["n_outside"]
        ph, pT, pid = fields
        out, c = INJ.inject(q, ph, (pT, pid), (Tv, None), (INJ.VERTEX, INJ.DONOR), min_xcell=3)
        q.active = out
        got = jr.inject_particles_phase_(p, dev[0], (dev[1], dev[2]), (dTv, None), loc=("vertex", "donor"), min_xcell=3, handle=h)
        print(ni, step, c)
        assert got == c, (step, got, c)
        _assert_state(jr, p, dev, q, fields, f"inject {step}")
        injected += c["n_injected"]
    assert lost > 0 and injected > 0 and np.all((q.active != 0).sum(axis=2) >= 3)


# ---------------------------------------------------------------------------------------------- 3. no donor
def test_the_inner_cells_of_an_emptied_block_have_no_donor_and_its_ring_is_filled_from_outside(jr, h):
    ni = (33, 17)
    q, f = _cloud0(ni)
    q, fields = PT.copy(q), [x.copy() for x in f]
    blk = (slice(10, 15), slice(5, 10))
    q.active[blk], q.px[blk], q.py[blk] = 0, 0.0, 0.0
    for x in fields:
        x[blk] = 0.0
    p, dev = _device_particles(jr, q, fields)
    ph, pT, pid = fields
    out, c = INJ.inject(q, ph, (pid,), (None,), (INJ.DONOR,), min_xcell=4)
    q.active = out
    assert c["n_no_donor"] == 9 and c["n_deficient"] == 25 and c["n_injected"] == 16 * 4
    assert np.all(out[11:14, 6:9] == 0) and np.all(out[blk].sum(axis=2)[[0, -1], :] == 4) and np.all(out[blk].sum(axis=2)[:, [0, -1]] == 4)
    got = jr.inject_particles_phase_(p, dev[0], (dev[2],), (None,), min_xcell=4, handle=h)
    assert got == c
    _assert_state(jr, p, dev, q, fields)


# ---------------------------------------------------------------------------------------------- 4. ties
def test_of_two_equally_near_donors_the_first_in_scan_order_gives_the_phase(jr, h):
    ni = (7, 5)
    q = PT.init_particles(NXCELL, MAX_XCELL, 1, _xvi(ni), ni)
    site0 = (q.px[:, :, 0].copy(), q.py[:, :, 0].copy())          # site 0 of every cell: the first new point of an empty cell
    q.active[:], q.px[:], q.py[:] = 0, 0.0, 0.0
    ph = np.zeros_like(q.px)

    def put(i, j, s, x, y, phase):
        q.active[i, j, s], q.px[i, j, s], q.py[i, j, s], ph[i, j, s] = 1, x, y, phase
    # one bucket: two particles at one point away from every site; min_xcell = 3 makes the cell take a third
    x, y = ORIGIN[0] + 1.4375 * DX, ORIGIN[1] + 1.4375 * DY
    put(1, 1, 1, x, y, 3.0), put(1, 1, 3, x, y, 4.0)
    # two buckets: the west neighbour (dj = 0, di = -1) and the south-east neighbour (dj = -1, di = 1) of the empty cell (5, 3) hold a particle each, both at
    # site 0 of cell (5, 3) (neither has been moved yet): the south-east one is scanned first, though its bucket comes later in memory
    put(4, 3, 0, site0[0][5, 3], site0[1][5, 3], 1.0), put(6, 2, 0, site0[0][5, 3], site0[1][5, 3], 2.0)
    p, (dph,) = _device_particles(jr, q, (ph,))
    entry = q.active.copy()
    out, c = INJ.inject(q, ph, min_xcell=3)
    q.active = out
    assert out[1, 1].tolist()[:4] == [1, 1, 0, 1] and ph[1, 1, 0] == 3.0                                # slot 1 before slot 3
    assert out[5, 3].tolist()[:4] == [1, 1, 1, 0] and np.all(ph[5, 3, :3] == 2.0)                       # dj = -1 before dj = 0
    assert c["n_no_donor"] > 0          # most of this grid is empty
    got = jr.inject_particles_phase_(p, dph, min_xcell=3, handle=h)
    assert got == c
    _assert_state(jr, p, (dph,), q, (ph,))
    assert _same(_mask(p._index2), entry)


# ---------------------------------------------------------------------------------------------- 5. bad coordinates
@pytest.mark.parametrize("ni", [(7, 5), (33, 17)])
def test_a_nan_an_infinite_and_a_displaced_particle_count_occupy_no_site_and_never_donate(jr, h, ni):
    q, fields, grids = _moved(ni)
    n = (q.active != 0).sum(axis=2)
    i, j = next((i, j) for i, j in np.argwhere((n == 3)) if 1 <= i < ni[0] - 1 and n[i + 1, j] >= 1)          # a cell deficient at min_xcell = 4, and its east neighbour
    q.px[i, j, 0] = np.nan
    q.px[i, j, 1] += 1000.0          # finite, far outside its bucket cell
    q.py[i + 1, j, 0] = np.inf
    bad = {fields[2][i, j, 0], fields[2][i, j, 1], fields[2][i + 1, j, 0]}
    p, dev = _device_particles(jr, q, fields)
    dgrids = tuple(_up(g) for g in grids)
    entry, c = _cpu(q, fields, grids, ni, 4)
    new = (q.active != 0) & (entry == 0)
    # each counts: the cell takes one particle, not three; none occupies a site: with only slot 2 on the lattice the new particle sits on the first site slot 2 leaves
    assert int(new[i, j].sum()) == 1 and c["n_active_before"] == int((entry != 0).sum())
    s2 = (int(np.floor((q.px[i, j, 2] - (q.x0 + i * DX)) / DX * 2)), int(np.floor((q.py[i, j, 2] - (q.y0 + j * DY)) / DY * 2)))
    first = 0 if s2 != (0, 0) else 1
    want = (q.x0 + i * DX + (first % 2 + 0.5) * (DX / 2), q.y0 + j * DY + (first // 2 + 0.5) * (DY / 2))
    assert (q.px[i, j, 3], q.py[i, j, 3]) == want
    assert not bad & set(fields[2][new]) and len(bad) == 3          # the identity is copied from the donor: none of the three ever is one
    got = _gpu(jr, h, p, dev, dgrids, ni, 4)
    assert got == c
    _assert_state(jr, p, dev, q, fields)


# ---------------------------------------------------------------------------------------------- 6. nothing deficient
@pytest.mark.parametrize("ni", SHAPES)
def test_with_nothing_deficient_every_array_is_unchanged_and_the_mask_is_copied_in_full(jr, h, ni):
    q, f = _cloud0(ni)
    q, fields = PT.copy(q), [x.copy() for x in f]
    p, dev = _device_particles(jr, q, fields)
    out, c = INJ.inject(q, fields[0], (fields[1],), (None,), (INJ.DONOR,), min_xcell=1)
    total = NXCELL * ni[0] * ni[1]
    assert c == dict(n_active_before=total, n_active_after=total, n_deficient=0, n_injected=0, n_no_donor=0) and np.array_equal(out, q.active)
    assert float(p._index2.max()) == -77
    got = jr.inject_particles_phase_(p, dev[0], (dev[1],), (None,), min_xcell=1, handle=h)
    assert got == c
    _assert_state(jr, p, dev, q, fields)          # p.index is the mask that was just written: no -77 is left
    assert _same(_mask(p._index2), q.active)


@pytest.mark.parametrize("nxcell,max_xcell,min_xcell", [(4, 7, 4), (2, 3, 2), (4, 4, 3)])
def test_bucket_sizes_around_the_unrolling_of_the_mask_copy(jr, h, nxcell, max_xcell, min_xcell):
    """the kernel copies the mask four slots at a time and the rest one by one: 7 = 4 + 3, 3 = 0 + 3, 4 = 4 + 0 (every other test has 12 = 3 x 4)"""
    ni = (33, 17)
    q = PT.init_particles(nxcell, max_xcell, min_xcell, _xvi(ni), ni, rng=np.random.default_rng(3))
    rng = np.random.default_rng(4)
    keep = (q.active != 0) & (rng.random(q.active.shape) < 0.7)
    q.active[:] = keep
    q.px[~keep], q.py[~keep] = 0.0, 0.0
    ph = np.where(keep, 1.0 + np.arange(keep.size).reshape(keep.shape) % 3, 0.0)
    p, (dph,) = _device_particles(jr, q, (ph,))
    entry = q.active.copy()
    out, c = INJ.inject(q, ph)          # min_xcell and the lattice are the particles' own
    q.active = out
    assert c["n_injected"] > 0 and c["n_no_donor"] == 0 and np.all(out.sum(axis=2) >= min_xcell)
    got = jr.inject_particles_phase_(p, dph, handle=h)
    assert got == c
    _assert_state(jr, p, (dph,), q, (ph,))
    assert _same(_mask(p._index2), entry)


# ---------------------------------------------------------------------------------------------- 7. inputs untouched, outputs written
@pytest.mark.parametrize("ni", SHAPES)
def test_the_slots_the_definition_writes_are_written_and_nothing_else_is(jr, h, ni):
    q, fields, grids = _moved(ni)
    start = PT.copy(q), [x.copy() for x in fields]
    entry, c = _cpu(q, fields, grids, ni, 4)
    new = (q.active != 0) & (entry == 0)
    assert new.sum() > 0
    # sentinels where the call writes: the coordinates, the phases and the three listed fields of the new slots
    s, sf = start
    for x in (s.px, s.py, sf[0], sf[1], sf[2], sf[3]):
        x[new] = SENTINEL
    p, dev = _device_particles(jr, s, sf)
    dgrids = tuple(_up(g) for g in grids)
    got = _gpu(jr, h, p, dev, dgrids, ni, 4)
    assert got == c
    _assert_state(jr, p, dev, q, fields)          # equal to the restatement run without sentinels: every one of them was overwritten
    assert all(_same(jr.to_numpy(d), g) for d, g in zip(dgrids, grids)) and _same(_mask(p._index2), entry)
    old = entry != 0
    for d, x in zip((p.coords[0], p.coords[1]) + tuple(dev), (s.px, s.py) + tuple(sf)):
        assert np.array_equal(_bits(jr.to_numpy(d))[old], _bits(x)[old])          # every slot active at entry, in every array


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_the_library_refuses_with_status_4_a_text_and_no_launch(jr, h):
    ni = (7, 5)
    q, fields, grids = _moved(ni)
    p, dev = _device_particles(jr, q, fields[:3])
    q1, f1, g1 = _moved((1, 6))
    p1, dev1 = _device_particles(jr, q1, f1[:2])
    Fv, Fc = _up(grids[0]), _up(grids[1])
    L, P = h.lib, lambda t: C.c_void_p(t.data_ptr())
    before = [jr.to_numpy(t) for t in p.coords + tuple(dev)] + [_mask(p.index), _mask(p._index2)]
    counts = (C.c_int64 * 5)(*([-1] * 5))
    n0 = _launches(h)
    VTX, CEN, DON = INJ.VERTEX, INJ.CENTRE, INJ.DONOR

    def S(part=p, **kw):
        s = part._struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def vec(ts):
        return (C.c_void_p * max(len(ts), 1))(*(None if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in ts))

    def call(s="S", aout="aout", ph="ph", args=(dev[1],), flds=(Fv,), locs=(VTX,), n=None, minx=3, nsx=2, nsy=2, cnt=counts):
        s = C.byref(S()) if s == "S" else s
        aout = P(p._index2) if aout == "aout" else aout
        ph = P(dev[0]) if ph == "ph" else ph
        a = None if args is None else vec(args)
        f = None if flds is None else vec(flds)
        lc = None if locs is None else (C.c_int32 * max(len(locs), 1))(*locs)
        return L.jrx_particles2d_inject(h._h, s, aout, ph, a, f, lc, C.c_int32(len(args) if n is None else n), C.c_int32(minx), C.c_int32(nsx), C.c_int32(nsy), cnt)

    def refused(status, text):
        assert status == 4 and text in L.jrx_last_error(h._h).decode(), (status, text, L.jrx_last_error(h._h).decode())
        assert _launches(h) == n0

    # a NULL pointer, where one is required
    refused(call(s=None), "particles is NULL")
    refused(call(s=C.byref(S(py=None))), "particles.py is NULL")
    refused(call(aout=None), "active_out is NULL")
    refused(call(ph=None), "pPhases is NULL")
    refused(call(cnt=None), "counts is NULL")
    refused(call(args=None, n=1), "args is NULL")
    refused(call(flds=None), "fields is NULL")
    refused(call(locs=None), "field_loc is NULL")
    refused(call(args=(None,)), "particle field 1 is NULL")
    refused(call(args=(dev[1], dev[2]), flds=(Fv, None), locs=(VTX, CEN)), "grid field 2 is NULL")
    # the numbers
    refused(call(minx=0), "min_xcell = 0")
    refused(call(minx=13, nsx=4, nsy=4), "min_xcell = 13")          # above max_xcell = 12
    refused(call(minx=5), "min_xcell = 5")                          # above nsx nsy = 4
    refused(call(nsx=0), "lattice of 0 x 2")
    refused(call(nsy=-1), "lattice of 2 x -1")
    refused(call(nsx=13, nsy=5), "lattice of 13 x 5")               # 65 sites
    refused(call(n=-1), "-1 particle fields")
    refused(call(args=(dev[1],) * 9, flds=(Fv,) * 9, locs=(VTX,) * 9), "9 particle fields")
    refused(call(locs=(3,)), "unknown field_loc 3")
    refused(call(locs=(-1,)), "unknown field_loc -1")
    Fc1 = jr.fzeros((1, 6), _dev())
    refused(L.jrx_particles2d_inject(h._h, C.byref(S(p1)), P(p1._index2), P(dev1[0]), vec((dev1[1],)), vec((Fc1,)), (C.c_int32 * 1)(CEN), 1, 3, 2, 2, counts),
            "interpolation between centres")
    # overlaps
    refused(call(aout=P(p.index)), "active_out overlaps the mask")
    refused(call(ph=P(dev[1])), "pPhases and particle field 1 overlap")
    refused(call(ph=P(p.coords[0])), "pPhases overlaps the particle coordinates")
    refused(call(args=(p.coords[1],)), "particle field 1 overlaps the particle coordinates")
    refused(call(args=(dev[1], dev[1]), flds=(Fv, None), locs=(VTX, DON)), "particle field 1 and particle field 2 overlap")
    refused(call(aout=P(dev[0])), "active_out and pPhases overlap")
    refused(call(flds=(dev[1],)), "particle field 1 overlaps a vertex field")
    refused(call(flds=(dev[0],), locs=(CEN,)), "pPhases overlaps a centre field")
    refused(call(flds=(p.coords[0],)), "a vertex field overlaps the particle coordinates")
    refused(call(flds=(p._index2,)), "active_out overlaps a vertex field")
    # the section's common geometry check
    refused(call(s=C.byref(S(nx=0))), "0 x 5 cells")
    refused(call(s=C.byref(S(max_xcell=0))), "max_xcell = 0")
    refused(call(s=C.byref(S(dx=-DX))), "spacings")
    refused(call(s=C.byref(S(y0=float("inf")))), "origin")
    refused(call(s=C.byref(S(_dy=1.0))), "not 1 / dx")
    refused(call(s=C.byref(S(nx=65536, ny=65536))), "2^31")
    # nothing was written
    assert list(counts) == [-1] * 5
    after = [jr.to_numpy(t) for t in p.coords + tuple(dev)] + [_mask(p.index), _mask(p._index2)]
    assert all(_same(a, b) for a, b in zip(before, after)) and int(p._index2.max()) == -77 and int(p1._index2.max()) == -77
    assert _same(jr.to_numpy(Fv), grids[0]) and _same(jr.to_numpy(Fc), grids[1])
    # the wrapper looks at the device of every operand, and a refused call swaps nothing
    index = p.index
    with pytest.raises(ValueError, match=r"fields\[0\] is on cpu"):
        jr.inject_particles_phase_(p, dev[0], (dev[1],), (jr.fzeros((8, 6), "cpu"),), handle=h)
    with pytest.raises(ValueError, match=r"args\[0\] is on cpu"):
        jr.inject_particles_phase_(p, dev[0], (jr.fzeros(p.shape, "cpu"),), (None,), handle=h)
    assert _launches(h) == n0 and p.index is index
    # ... and the donor kind reads no grid field: NULL is accepted there
    assert call(args=(dev[1], dev[2]), flds=(Fv, None), locs=(VTX, DON)) == 0 and _launches(h) == n0 + 1 and counts[3] > 0
