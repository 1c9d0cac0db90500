"""GPU: phase ratios from phase fields (update_phase_ratios_2D_ / update_phase_ratios_3D_; csrc/phase_ratios.hip through jrx_update_phase_ratios2d / 3d) against
the NumPy restatement (tests/_phase_ratios.py): bit for bit in every member except the 2D vertex (fma on the device, two roundings in NumPy: 1e-13, the bound
of the WENO tests for the same cause), the threshold on either side, sharp interfaces, the one-launch form against the launch-per-member form bit for bit,
the counters, degenerate cells, every refusal with the outputs untouched, and the example's time loop."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _phase_ratios as PR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "justrelax.jl_amd" / "csrc" / "phase_ratios.hip").read_text()
TX, TY2, TY3, TZ3 = (int(re.search(rf"\b{k} = (\d+)", SRC).group(1)) for k in ("kPrTX", "kPrTY2", "kPrTY3", "kPrTZ3"))
# a single cell, odd primes, and one node more than the kernel's own tile in every direction (more than one block along every dimension)
SMALL = [(1, 1), (7, 5), (1, 1, 1), (5, 3, 2)]
TILES = [(TX + 1, TY2 + 1), (TX + 1, TY3 + 1, TZ3 + 1)]
CASES = [(s, n) for s in SMALL + TILES for n in (1, 2, 3)] + [(s, 8) for s in SMALL]
SENTINEL = -7.0


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


def _grid(ni, offcentre=False):
    """a uniform grid whose coordinates are not dyadic; offcentre: the 'centres' sit 0.3 dx into their cells, so that a weight of 0.5 would be wrong"""
    nd = len(ni)
    xci, xvi = PR.uniform_grid(ni, (2.0, 1.0, 0.7)[:nd], (-0.3, 0.1, 0.0)[:nd])
    if offcentre:
        xci = tuple(xv[:-1] + 0.3 * (xv[1] - xv[0]) for xv in xvi)
    return xci, xvi


def _dyadic_grid(ni):
    """power-of-two extents on the unit box: every coordinate, distance and weight is exact, with and without fma"""
    assert all(n & (n - 1) == 0 for n in ni)
    return PR.uniform_grid(ni)


def _random(ni, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.05, 1.0, ni) for _ in range(n)]          # every normalised value >= 0.05 / 8: the 1e-5 threshold cannot fire


def _run(jr, h, ps, xci, xvi, fused=True):
    """one update on fresh device arrays pre-filled with a sentinel: member name -> NumPy array"""
    ni = ps[0].shape
    h.set_option("phase_ratios_fused", int(fused))
    pr = jr.PhaseRatios(jr.AMDGPUBackend, len(ps), ni)
    for name in PR.members(len(ni)):
        getattr(pr, name).fill_(SENTINEL)
    fn = jr.update_phase_ratios_2D_ if len(ni) == 2 else jr.update_phase_ratios_3D_
    fn(pr, tuple(_up(p) for p in ps), xci, xvi, handle=h)
    return {name: jr.to_numpy(getattr(pr, name)) for name in PR.members(len(ni))}


def _assert_parity(got, ref, nd):
    from justrelax_jl_amd.checks import max_rel_diff
    for name in PR.members(nd):
        assert got[name].shape == ref[name].shape, name
        if nd == 2 and name == "vertex":
            d = max_rel_diff(got[name], ref[name])
            print("2D vertex max_rel_diff:", d)
            assert d <= 1e-13
        else:
            assert np.array_equal(got[name], ref[name], equal_nan=True), name


@pytest.mark.parametrize("ni,n", CASES)
def test_parity_with_the_restatement(jr, h, ni, n):
    ps = _random(ni, n, 20261019 + n)
    xci, xvi = _grid(ni)
    _assert_parity(_run(jr, h, ps, xci, xvi), PR.update_phase_ratios(ps, xci, xvi), len(ni))


@pytest.mark.parametrize("ni", [(7, 5), (5, 3, 2)])
def test_weights_come_from_the_coordinates(jr, h, ni):
    ps = _random(ni, 2, 5)
    xci, xvi = _grid(ni, offcentre=True)
    ref = PR.update_phase_ratios(ps, xci, xvi)
    assert np.abs(ref["vertex"] - PR.update_phase_ratios(ps, *_grid(ni))["vertex"]).max() > 1e-3
    _assert_parity(_run(jr, h, ps, xci, xvi), ref, len(ni))


@pytest.mark.parametrize("ni", [(8, 4), (4, 8, 2)])
@pytest.mark.parametrize("third,kept", [(2.0e-5, True), (5.0e-6, False)])
def test_threshold_a_factor_two_either_side(jr, h, ni, third, kept):
    """the third phase is `third` of the total in every cell, hence in every member: a factor 2 above the threshold it is kept, a factor 2 below it is zeroed"""
    a = np.random.default_rng(11).uniform(0.3, 0.7, ni)
    ps = [a * (1.0 - third), (1.0 - a) * (1.0 - third), np.full(ni, third)]
    xci, xvi = _dyadic_grid(ni)
    got, ref = _run(jr, h, ps, xci, xvi), PR.update_phase_ratios(ps, xci, xvi)
    for name in PR.members(len(ni)):
        assert np.array_equal(got[name], ref[name]), name
        assert np.all(got[name][2] > 0.0) if kept else np.all(got[name][2] == 0.0), name


@pytest.mark.parametrize("ni", [(4, 4), (4, 4, 4)])
def test_reference_threshold_case(jr, h, ni):
    """test_rheology.jl:492-500, test_phase_ratios3D.jl:75-83: (0.6, 0.4, 1e-6) on the reference's own grid"""
    ps = [np.full(ni, v) for v in (0.6, 0.4, 1.0e-6)]
    xci, xvi = _dyadic_grid(ni)
    got, ref = _run(jr, h, ps, xci, xvi), PR.update_phase_ratios(ps, xci, xvi)
    for name in PR.members(len(ni)):
        assert np.array_equal(got[name], ref[name]), name
        assert np.all(got[name][2] == 0.0) and np.all(np.abs(got[name][0] + got[name][1] - 1.0) <= 1e-15), name


@pytest.mark.parametrize("ni,axis", [((8, 4), 0), ((8, 4), 1), ((4, 8, 2), 0), ((4, 8, 2), 1), ((4, 4, 4), 2)])
def test_sharp_interface(jr, h, ni, axis):
    nd, half = len(ni), ni[axis] // 2
    idx = np.arange(ni[axis]).reshape([-1 if d == axis else 1 for d in range(nd)])
    p1 = np.broadcast_to((idx < half).astype(np.float64), ni).copy()
    ps = [p1, 1.0 - p1]
    xci, xvi = _dyadic_grid(ni)
    got = _run(jr, h, ps, xci, xvi)
    for name in PR.members(nd):
        assert np.array_equal(got[name], PR.update_phase_ratios(ps, xci, xvi)[name]), name
    assert np.array_equal(got["center"][0], p1) and np.array_equal(got["center"][1], 1.0 - p1)
    take = lambda a, i: np.take(a, i, axis=axis + 1)
    # every node on the interface plane that is staggered along `axis` holds (0.5, 0.5): all vertices, the faces across it, the edges around it
    for name, stag in PR.members(nd).items():
        a = got[name]
        if stag[axis]:
            assert np.all(take(a, half) == 0.5), name
            # the domain boundary reproduces the adjacent cells: (1, 0) on the low side, (0, 1) on the high side
            assert np.all(take(a, 0)[0] == 1.0) and np.all(take(a, 0)[1] == 0.0), name
            assert np.all(take(a, ni[axis])[0] == 0.0) and np.all(take(a, ni[axis])[1] == 1.0), name
        else:
            assert np.all(take(a, half - 1)[0] == 1.0) and np.all(take(a, half)[1] == 1.0), name


@pytest.mark.parametrize("ni", SMALL + TILES)
@pytest.mark.parametrize("n", [2, 3])
def test_both_forms_leave_identical_bits(jr, h, ni, n):
    ps = _random(ni, n, 77 + n)
    xci, xvi = _grid(ni)
    c0, f0 = h.get_option("stat_phase_ratios_calls"), h.get_option("stat_phase_ratios_fused")
    fused = _run(jr, h, ps, xci, xvi, fused=True)
    assert (h.get_option("stat_phase_ratios_calls"), h.get_option("stat_phase_ratios_fused")) == (c0 + 1, f0 + 1)
    split = _run(jr, h, ps, xci, xvi, fused=False)
    assert (h.get_option("stat_phase_ratios_calls"), h.get_option("stat_phase_ratios_fused")) == (c0 + 2, f0 + 1)
    h.set_option("phase_ratios_fused", 1)
    for name in PR.members(len(ni)):
        assert np.array_equal(fused[name], split[name]), name
        assert not np.any(fused[name] == SENTINEL), name


def _readers(name, cell, ni):
    m = np.zeros(PR.member_shape(name, ni), dtype=bool)
    m[tuple(slice(c, c + 1 + s) for c, s in zip(cell, PR.members(len(ni))[name]))] = True
    return m


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("ni,cell", [((7, 5), (3, 2)), ((5, 3, 3), (2, 1, 1))])
def test_degenerate_cell(jr, h, ni, cell, fused):
    """A cell holding a NaN: NaN for every phase at exactly the nodes that read it, every other node as without it.  A cell whose arrays are all 0: 0 / 0 = NaN
    at its centre; a node that also reads a cell with material gets that cell's ratios (the reference's rules: the empty cell adds weight, no value, and the tail
    renormalises), so NaN appears at exactly the nodes whose every cell is empty -- all nodes of the one-cell grid.  Everything equals the restatement."""
    nd = len(ni)
    ps = _random(ni, 2, 9)
    xci, xvi = _grid(ni)
    clean = _run(jr, h, ps, xci, xvi, fused)
    qs = [p.copy() for p in ps]
    qs[1][cell] = np.nan
    got = _run(jr, h, qs, xci, xvi, fused)
    _assert_parity(got, PR.update_phase_ratios(qs, xci, xvi), nd)
    for name in PR.members(nd):
        reads = _readers(name, cell, ni)
        assert np.array_equal(np.isnan(got[name]).all(axis=0), reads) and np.array_equal(np.isnan(got[name]).any(axis=0), reads), name
        assert np.array_equal(got[name][:, ~reads], clean[name][:, ~reads]), name
    qs = [p.copy() for p in ps]
    for q in qs:
        q[cell] = 0.0
    got = _run(jr, h, qs, xci, xvi, fused)
    _assert_parity(got, PR.update_phase_ratios(qs, xci, xvi), nd)
    for name in PR.members(nd):
        reads = _readers(name, cell, ni)
        assert np.array_equal(np.isnan(got[name]).any(axis=0), reads if name == "center" else np.zeros_like(reads)), name
        assert np.array_equal(got[name][:, ~reads], clean[name][:, ~reads]), name
    one = (1,) * nd
    got = _run(jr, h, [np.zeros(one), np.zeros(one)], *_grid(one), fused)
    for name in PR.members(nd):
        assert np.isnan(got[name]).all(), name


# ---------------------------------------------------------------------------------------------- refusals
def _setup(jr, ni, n=2):
    pr = jr.PhaseRatios(jr.AMDGPUBackend, n, ni)
    for name in PR.members(len(ni)):
        getattr(pr, name).fill_(SENTINEL)
    return pr, tuple(_up(p) for p in _random(ni, n, 1))


def _untouched(pr, nd):
    return all(bool((getattr(pr, name) == SENTINEL).all()) for name in PR.members(nd))


@pytest.mark.parametrize("nd", [2, 3])
def test_host_layer_refusals(jr, h, nd):
    ni = (6, 5, 4)[:nd]
    pr, ps = _setup(jr, ni)
    fn = jr.update_phase_ratios_2D_ if nd == 2 else jr.update_phase_ratios_3D_
    other = jr.update_phase_ratios_3D_ if nd == 2 else jr.update_phase_ratios_2D_
    xci, xvi = _grid(ni)
    calls = h.get_option("stat_phase_ratios_calls")
    bent = tuple(x.copy() for x in xvi)
    bent[nd - 1][2] += 1e-9                                                  # a vertex spacing that varies by far more than a few ulp
    with pytest.raises(ValueError, match="uniform"):
        fn(pr, ps, xci, bent, handle=h)
    with pytest.raises(ValueError):                                          # a 2D call with 3D arrays, or the reverse
        other(pr, ps, xci, xvi, handle=h)
    with pytest.raises(ValueError):                                          # three arrays for two phases
        fn(pr, ps + (ps[0],), xci, xvi, handle=h)
    with pytest.raises(ValueError):                                          # arrays of two sizes
        fn(pr, (ps[0], _up(np.ones(tuple(n + 1 for n in ni)))), xci, xvi, handle=h)
    big = jr.PhaseRatios(jr.AMDGPUBackend, 2, tuple(n + 1 for n in ni))
    with pytest.raises(ValueError):                                          # a PhaseRatios of another grid
        fn(big, ps, xci, xvi, handle=h)
    with pytest.raises(ValueError):                                          # coordinates of another grid
        fn(pr, ps, *_grid(tuple(n + 1 for n in ni)), handle=h)
    assert _untouched(pr, nd) and h.get_option("stat_phase_ratios_calls") == calls
    fn(pr, ps, jr.Geometry.from_vertices(xvi), handle=h)                     # a Geometry in place of (xci, xvi)
    assert not _untouched(pr, nd) and h.get_option("stat_phase_ratios_calls") == calls + 1


@pytest.mark.parametrize("nd", [2, 3])
def test_c_abi_refusals(jr, h, nd):
    """every JRX_ERR_ARG condition of include/jrx.h: status 4, a text naming the cause, no launch (the counter stands still) and nothing written"""
    import torch
    ni = (6, 5, 4)[:nd]
    pr, ps = _setup(jr, ni)
    xci, xvi = _grid(ni)
    xc, xv = [_up(x) for x in xci], [_up(x) for x in xvi]
    names = ("center", "vertex", "Vx", "Vy") if nd == 2 else ("center", "vertex", "Vx", "Vy", "Vz", "yz", "xz", "xy")
    spare = torch.full((2 * int(np.prod([n + 1 for n in ni])),), SENTINEL, dtype=torch.float64, device=_dev())      # as large as the largest member
    torch.cuda.synchronize()
    fn = getattr(h.lib, f"jrx_update_phase_ratios{nd}d")

    def call(outs=None, arrays=None, nphase=2, n=ni, xcp=None, xvp=None, dx=None):
        outs = dict(zip(names, (getattr(pr, k).data_ptr() for k in names)), **(outs or {}))
        arrays = [p.data_ptr() for p in ps] if arrays is None else arrays
        pa = (C.c_void_p * max(len(arrays), 1))(*arrays)
        vec = lambda v: (C.c_void_p * nd)(*v)
        dx = [float(x[1] - x[0]) for x in xvi] if dx is None else dx
        st = fn(h._h, *(C.c_void_p(outs[k]) for k in names), pa, C.c_int32(nphase), *(C.c_int64(m) for m in n),
                vec([t.data_ptr() for t in xc] if xcp is None else xcp), vec([t.data_ptr() for t in xv] if xvp is None else xvp), (C.c_double * nd)(*dx))
        return st, h.lib.jrx_last_error(h._h).decode()

    calls = h.get_option("stat_phase_ratios_calls")
    ok_dx = [float(x[1] - x[0]) for x in xvi]
    bad = [(dict(outs={k: None}), k) for k in names]                                                     # a NULL output
    bad += [(dict(arrays=[ps[0].data_ptr(), None]), "phase array 2"), (dict(xcp=[None] + [t.data_ptr() for t in xc[1:]]), "dimension 1"),
            (dict(xvp=[t.data_ptr() for t in xv[:-1]] + [None]), f"dimension {nd}")]                     # a NULL entry of phase_arrays, xc, xv
    bad += [(dict(nphase=0, arrays=[]), "phase arrays"), (dict(nphase=9, arrays=[ps[0].data_ptr()] * 9), "phase arrays")]
    bad += [(dict(n=ni[:d] + (0,) + ni[d + 1:]), f"dimension {d + 1}") for d in range(nd)]
    bad += [(dict(dx=ok_dx[:-1] + [v]), "spacing") for v in (0.0, -ok_dx[-1], float("inf"), float("nan"))]
    bad += [(dict(outs={"Vx": ps[0].data_ptr()}), "overlaps phase array 1"), (dict(outs={"Vx": spare.data_ptr(), "Vy": spare.data_ptr()}), "overlap"),
            (dict(outs={"vertex": xv[0].data_ptr()}), "coordinate")]
    for kw, text in bad:
        st, msg = call(**kw)
        assert st == 4 and text in msg, (kw, st, msg)
    torch.cuda.synchronize()
    assert _untouched(pr, nd) and bool((spare == SENTINEL).all()) and h.get_option("stat_phase_ratios_calls") == calls
    st, msg = call()
    assert st == 0, msg
    assert not _untouched(pr, nd)


def test_example_time_loop(jr):
    """examples/sinking_block2d_fields.py at 24^2 for 2 steps (a short solve!: the loop is what is tested, not convergence): every member finite and summing to 1"""
    sys.path.insert(0, str(ROOT / "examples"))
    import sinking_block2d_fields as ex
    pr, fields, _ = ex.main(24, 2, iterMax=200, quiet=True)
    for name in PR.members(2):
        a = jr.to_numpy(getattr(pr, name))
        assert np.isfinite(a).all(), name
        assert np.abs(a.sum(axis=0) - 1.0).max() <= 1e-12, name
    block = jr.to_numpy(pr.center)[1]
    assert 0.0 < block.sum() < block.size and block.max() > 0.9
