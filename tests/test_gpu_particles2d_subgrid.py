"""GPU: the temperature on 2D particles -- subgrid_diffusion_centroid! and subgrid_diffusion! with loc = :vertex (csrc/particles.hip through
jrx_particles2d_subgrid_diffusion_centroid / _vertex, operators 10 and 11 of include/jrx.h) against the NumPy restatement (tests/_particles2d_subgrid.py, pinned by
tests/test_particles2d_subgrid_restatement.py).

1. The fused forms (two and three launches) against the chains of the definition ("particles_subgrid_fused" 1 against 0, device against device): pT, pT0, pΔT and
   ΔT_subgrid BIT FOR BIT as 64-bit patterns, every d and every case; +0.0 in the inactive slots; the launch counts; the inputs untouched; the ghosted ΔT_grid with
   sentinel ghosts gives the bits of the plain one.
2. Device against NumPy at d = 0: bit for bit in every output (exp(-0) = 1 on both sides).
3. Device against NumPy at d > 0: the only difference is the device's exp: within 1e-13 max|T|, the project's bound for device arithmetic against NumPy (RTOL of
   tests/test_gpu_particles2d_stress.py and tests/test_gpu_stress_rotation.py), NaNs in the same places; every case prints its measured figure.
4. The refusals through the C ABI: status 4, a text, "stat_particles_launches" unchanged, the outputs still sentinel-filled.

Sizes: (2, 2) is the smallest grid the centre form accepts and three quarters of its area extrapolate; (7, 5) is one ragged block; (33, 17) has 561 cells and 612
vertices: more than two 256-thread blocks; (128, 5) is the smallest shape whose cell launches have two block columns and whose node launches have three.
nxcell = 4, max_xcell = 12, jittered.  The cloud is the restatement's after one advect_rk2 + move under a rigid rotation (_rotated of tests/_particles_gpu.py).
Cases: the cloud as it is; centre form: an interior cell emptied ((2, 2) has none); vertex form: the corner cell (0, 0) emptied, so that vertex (0, 0) has den == 0,
on (2, 2) too; a copy with a NaN x in one active slot and an infinite y in another.  The restatement shows on the CPU, before the device is asked, that in the plain
cloud every centre and every vertex has den > 0 and in an emptied cloud exactly the one intended node has den == 0.
Not exercised: the refusal of a handle with a communicator (it needs a second rank)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _particles2d_stress as PS
import _particles2d_subgrid as SG
from _particles_gpu import D, MAX_XCELL, SENTINEL, _assert_cloud_untouched, _bits, _device_particles, _handle, _launches, _ndiff, _rotated, _same, _up

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2), (7, 5), (33, 17), (128, 5)]


def _cases(shapes):
    return [("center", ni, c) for ni in shapes for c in ("plain", "emptied", "non-finite") if not (c == "emptied" and ni == (2, 2))] + \
           [("vertex", ni, c) for ni in shapes for c in ("plain", "emptied", "non-finite")]


CASES = _cases(SHAPES[:3]) + _cases(SHAPES[3:])          # (128, 5) behind the others: the cases before it keep their test ids
DS = [0.0, 0.3, 1.0]
DX, DY = D[:2]
DT = 2.0e3
RTOL = 1e-13
LAUNCHES = {("center", 1): 2, ("vertex", 1): 3, ("center", 0): 7, ("vertex", 0): 7}          # include/jrx.h, operators 10 and 11
ENTRY = {"center": "jrx_particles2d_subgrid_diffusion_centroid", "vertex": "jrx_particles2d_subgrid_diffusion_vertex"}


@pytest.fixture(scope="module")
def h(jr):
    hh = _handle()
    default = hh.get_option("particles_subgrid_fused")
    yield hh
    hh.set_option("particles_subgrid_fused", default)


def _ext(loc, ni):
    return tuple(ni) if loc == "center" else (ni[0] + 1, ni[1] + 1)


def _ghosted(dT):
    g = np.full((dT.shape[0] + 2, dT.shape[1] + 2), SENTINEL)
    g[1:-1, 1:-1] = dT
    return np.asfortranarray(g)


@functools.lru_cache(maxsize=None)
def _case(loc, ni, case):
    """(cloud, pT, T_grid, ΔT_grid, ΔT_grid with sentinel ghosts, dt0): computed once per case and shared read-only"""
    q = _rotated(ni)
    hole = None
    if case == "emptied":
        hole = (ni[0] // 2, ni[1] // 2) if loc == "center" else (0, 0)
        q.active[hole], q.px[hole], q.py[hole] = 0, 0.0, 0.0
    a = q.active != 0
    per_cell = a.sum(axis=2)
    assert per_cell.max() < MAX_XCELL and per_cell.min() != per_cell.max()          # inactive slots everywhere, buckets unevenly filled
    # the condition of the case, shown before the device is asked
    dc, dv = PS.centre_den(q), PS.vertex_den(q)
    if hole is None:
        assert dc.min() > 0.0 and dv.min() > 0.0
    elif loc == "center":
        assert dc[hole] == 0.0 and (dc == 0.0).sum() == 1 and 0 < hole[0] < ni[0] - 1 and 0 < hole[1] < ni[1] - 1
    else:
        assert dv[0, 0] == 0.0 and (dv == 0.0).sum() == 1
    slots = np.argwhere(a)
    if case == "non-finite":
        sx, sy = tuple(slots[len(slots) // 3]), tuple(slots[2 * len(slots) // 3])
        assert sx[:2] != sy[:2]
        q.px[sx], q.py[sy] = np.nan, np.inf
    rng = np.random.default_rng(17 + ni[0])
    pT = np.where(a, rng.uniform(300.0, 1600.0, a.shape), 0.0)
    T = np.asfortranarray(rng.uniform(300.0, 1600.0, _ext(loc, ni)))
    dT = np.asfortranarray(rng.uniform(-50.0, 50.0, T.shape))
    dt0 = np.where(a, DT * 10.0 ** rng.uniform(-3.0, 3.0, a.shape), 0.0)          # log-uniform over six decades around dt
    dt0[tuple(slots[1])], dt0[tuple(slots[-2])] = 0.0, np.nan                  # both take the 1e-9 floor
    out = (q, pT, T, dT, _ghosted(dT), dt0)
    for x in (q.px, q.py, q.active) + out[1:]:
        x.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def _want(loc, ni, case, d):
    q, pT, T, dT, _, dt0 = _case(loc, ni, case)
    return SG.FORMS[loc](pT, T, dT, dt0, q, DT, d=d)


def _sentinel_arrays(jr, p, loc, dt0):
    sa = jr.SubgridDiffusionCellArrays(p, loc=loc)
    sa.pT0.fill_(SENTINEL), sa.pΔT.fill_(SENTINEL), sa.ΔT_subgrid.fill_(SENTINEL)
    sa.dt0.copy_(_up(dt0))
    return sa


def _run(jr, h, loc, p, pT, T, dT, dt0, d, fused):
    """one call through the Python layer on fresh outputs: (the four outputs as NumPy arrays, the launches it took, the device arrays)"""
    h.set_option("particles_subgrid_fused", int(fused))
    (dpT,) = jr.init_cell_arrays(p, 1)
    dpT.copy_(_up(pT))
    sa = _sentinel_arrays(jr, p, loc, dt0)
    n0 = _launches(h)
    (jr.subgrid_diffusion_centroid_ if loc == "center" else jr.subgrid_diffusion_)(dpT, T, dT, sa, p, DT, d=d, handle=h)
    out = dict(zip(SG.OUTPUTS, (jr.to_numpy(t) for t in (dpT, sa.pT0, sa.pΔT, sa.ΔT_subgrid))))
    return out, _launches(h) - n0, sa


# ---------------------------------------------------------------------------------------------- 1 - 3: fused against chain, device against NumPy
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("loc,ni,case", CASES)
def test_the_fused_form_equals_its_chain_and_the_restatement(jr, h, loc, ni, case, d):
    q, pT, T, dT, dTg, dt0 = _case(loc, ni, case)
    want = _want(loc, ni, case, d)
    p, _ = _device_particles(jr, q)
    dT_dev, dTg_dev, T_dev = _up(dT), _up(dTg), _up(T)
    fused, nf, sa = _run(jr, h, loc, p, pT, T_dev, dT_dev, dt0, d, 1)
    chain, nc, _ = _run(jr, h, loc, p, pT, T_dev, dT_dev, dt0, d, 0)
    ghost, ng, _ = _run(jr, h, loc, p, pT, T_dev, dTg_dev, dt0, d, 1)
    ghost0, _, _ = _run(jr, h, loc, p, pT, T_dev, dTg_dev, dt0, d, 0)
    assert (nf, ng, nc) == (LAUNCHES[loc, 1], LAUNCHES[loc, 1], LAUNCHES[loc, 0])
    inactive = q.active == 0
    scale = max(np.abs(T).max(), np.abs(pT).max())
    worst = 0.0
    for k in SG.OUTPUTS:
        f = fused[k]
        assert _same(f, chain[k]), (k, "fused against chain", _ndiff(f, chain[k]))          # NaN entries included: the same bits
        assert _same(f, ghost[k]) and _same(f, ghost0[k]), (k, "the ghosted ΔT_grid", _ndiff(f, ghost[k]), _ndiff(f, ghost0[k]))          # no ghost was read
        assert not (f == SENTINEL).any(), k          # every entry written
        if k != "ΔT_subgrid":
            assert np.all(_bits(f[inactive]) == 0), k          # +0.0
        nan = np.isnan(want[k])
        assert np.array_equal(np.isnan(f), nan), (k, "NaNs in other places")
        if d == 0.0:
            assert np.array_equal(_bits(f)[~nan], _bits(want[k])[~nan]), (k, "d = 0 against NumPy", _ndiff(f, want[k]))
        else:
            fin = np.isfinite(want[k])          # an infinite y makes infinities of step 6 in the vertex form: the same ones
            assert np.array_equal(f[~fin & ~nan], want[k][~fin & ~nan]), (k, "infinities")
            worst = max(worst, float(np.abs(f - want[k])[fin].max()) / scale)
    assert int(np.isnan(fused["pT"]).sum()) > 0 if case == "non-finite" else np.isfinite(fused["pT"]).all()
    if d != 0.0:
        print(f"subgrid diffusion {loc} {ni} {case} d = {d}: max |device - NumPy| = {worst:.3e} max|T| (bound {RTOL:.0e})")
        assert worst <= RTOL, worst
    # the inputs are untouched
    assert _same(jr.to_numpy(T_dev), T) and _same(jr.to_numpy(dT_dev), dT) and _same(jr.to_numpy(dTg_dev), dTg)
    got0 = jr.to_numpy(sa.dt0)
    assert np.array_equal(np.isnan(got0), np.isnan(dt0)) and np.array_equal(_bits(got0)[~np.isnan(dt0)], _bits(dt0)[~np.isnan(dt0)])
    _assert_cloud_untouched(jr, p, q)


def test_the_emptied_nodes_keep_the_whole_grid_change_on_the_device(jr, h):
    """what the emptied cases are there for, read off the device's ΔT_subgrid: the den == 0 node holds ΔT_grid itself, and no other node does"""
    for loc, ni in (("center", (7, 5)), ("vertex", (2, 2))):
        q, pT, T, dT, _, dt0 = _case(loc, ni, "emptied")
        p, _ = _device_particles(jr, q)
        for fused in (1, 0):
            out, _, _ = _run(jr, h, loc, p, pT, _up(T), _up(dT), dt0, 1.0, fused)
            same = out["ΔT_subgrid"] == dT
            hole = (ni[0] // 2, ni[1] // 2) if loc == "center" else (0, 0)
            assert same[hole] and same.sum() == 1, (loc, fused)


# ---------------------------------------------------------------------------------------------- 4: refusals
def test_the_library_refuses_with_status_4_a_text_and_no_launch(jr, h):
    ni = (7, 5)
    L = h.lib
    for loc in ("center", "vertex"):
        q, pT, T, dT, dTg, dt0 = _case(loc, ni, "plain")
        p, _ = _device_particles(jr, q)
        (dpT,) = jr.init_cell_arrays(p, 1)
        dpT.fill_(SENTINEL)
        sa = _sentinel_arrays(jr, p, loc, dt0)
        T_dev, dT_dev = _up(T), _up(dT)
        n0 = _launches(h)
        fn = getattr(L, ENTRY[loc])
        P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

        def S(**kw):
            s = p._struct()
            for k, v in kw.items():
                setattr(s, k, v)
            return s

        def call(s=None, code=0, d=1.0, dt=DT, **kw):
            a = dict(pT=dpT, T=T_dev, dT=dT_dev, pT0=sa.pT0, pdT=sa.pΔT, dt0=sa.dt0, sub=sa.ΔT_subgrid)
            a.update(kw)
            return fn(h._h, P(a["pT"]), P(a["T"]), P(a["dT"]), C.c_int32(code), P(a["pT0"]), P(a["pdT"]), P(a["dt0"]), P(a["sub"]),
                      None if s is False else C.byref(s or S()), C.c_double(d), C.c_double(dt))

        def refused(status, text):
            assert status == 4 and text in L.jrx_last_error(h._h).decode(), (status, text, L.jrx_last_error(h._h).decode())
            assert _launches(h) == n0

        for fused in (1, 0):          # the chains check everything before their first launch too
            h.set_option("particles_subgrid_fused", fused)
            # the struct checks of the particle section
            refused(call(False), "particles is NULL")
            refused(call(S(px=None)), "particles.px is NULL")
            refused(call(S(max_xcell=0)), "max_xcell = 0")
            refused(call(S(dx=-DX)), "spacings")
            refused(call(S(_dy=1.0)), "not 1 / dx")
            # NULL pointers
            for key, name in (("pT", "pT"), ("T", "T_grid"), ("dT", "ΔT_grid"), ("pT0", "subgrid_arrays.pT0"), ("pdT", "subgrid_arrays.pΔT"), ("dt0", "subgrid_arrays.dt₀"),
                              ("sub", "subgrid_arrays.ΔT_subgrid")):
                refused(call(**{key: None}), f"{name} is NULL")
            # d, dt, the extent code
            for d in (-0.25, 1.0 + 2.0 ** -52, float("nan"), float("inf")):
                refused(call(d=d), "must lie in [0, 1]")
            for dt in (-1.0, float("nan"), float("inf")):
                refused(call(dt=dt), "must be finite and not negative")
            for code in (-1, 2):
                refused(call(code=code), f"unknown ΔT extent code {code}")
            # extents below 2: the centre form only
            if loc == "center":
                refused(call(S(nx=1)), "nx >= 2")
                refused(call(S(ny=1)), "nx >= 2")
            # overlaps: with an input, with another output, with the particles' own arrays
            refused(call(pT0=dpT), "pT and subgrid_arrays.pT0 overlap")
            refused(call(pdT=sa.pT0), "subgrid_arrays.pT0 and subgrid_arrays.pΔT overlap")
            refused(call(dt0=sa.pΔT), "subgrid_arrays.pΔT overlaps subgrid_arrays.dt₀")
            refused(call(T=sa.ΔT_subgrid), "subgrid_arrays.ΔT_subgrid overlaps T_grid")
            refused(call(dT=sa.ΔT_subgrid), "subgrid_arrays.ΔT_subgrid overlaps ΔT_grid")
            refused(call(dt0=dpT), "pT overlaps subgrid_arrays.dt₀")
            refused(call(pT=p.coords[1]), "pT overlaps the particle coordinates")
            refused(call(pdT=p.coords[0]), "subgrid_arrays.pΔT overlaps the particle coordinates")
        # nothing was written
        assert all(float((t - SENTINEL).abs().max()) == 0.0 for t in (dpT, sa.pT0, sa.pΔT, sa.ΔT_subgrid))
        assert _same(jr.to_numpy(T_dev), T) and _same(jr.to_numpy(dT_dev), dT)
        _assert_cloud_untouched(jr, p, q)
        # the wrappers look at the device of every operand
        with pytest.raises(ValueError, match="T_grid is on cpu"):
            (jr.subgrid_diffusion_centroid_ if loc == "center" else jr.subgrid_diffusion_)(dpT, jr.fzeros(T.shape, "cpu"), dT_dev, sa, p, DT, handle=h)
        with pytest.raises(ValueError, match="ΔT_grid is on cpu"):
            (jr.subgrid_diffusion_centroid_ if loc == "center" else jr.subgrid_diffusion_)(dpT, T_dev, jr.fzeros(dT.shape, "cpu"), sa, p, DT, handle=h)
        assert _launches(h) == n0


# ---------------------------------------------------------------------------------------------- the caller's three steps
def test_dt0_reaches_the_particles_by_centroid2particle_and_the_step_follows(jr, h):
    """centroid2particle_(subgrid_arrays.dt0, dt0, particles), then subgrid_diffusion_centroid_ with the ghosted thermal.ΔT: the miniapps' three lines, bit for bit at d = 0"""
    ni = (7, 5)
    q, pT, T, dT, dTg, _ = _case("center", ni, "plain")
    g0 = np.asfortranarray(np.random.default_rng(5).uniform(1.0, 1.0e6, ni))
    p, _ = _device_particles(jr, q)
    (dpT,) = jr.init_cell_arrays(p, 1)
    dpT.copy_(_up(pT))
    sa = jr.SubgridDiffusionCellArrays(p, loc="center")
    h.set_option("particles_subgrid_fused", 1)
    n0 = _launches(h)
    jr.centroid2particle_(sa.dt0, _up(g0), p, handle=h)
    jr.subgrid_diffusion_centroid_(dpT, _up(T), _up(dTg), sa, p, DT, d=0.0, handle=h)
    assert _launches(h) == n0 + 3
    dt0 = PS.centroid2particle(np.zeros(pT.shape), g0, q)
    want = SG.subgrid_diffusion_centroid(pT, T, dTg, dt0, q, DT, d=0.0)
    assert _same(jr.to_numpy(sa.dt0), dt0)
    for k, t in zip(SG.OUTPUTS, (dpT, sa.pT0, sa.pΔT, sa.ΔT_subgrid)):
        assert _same(jr.to_numpy(t), want[k]), k
