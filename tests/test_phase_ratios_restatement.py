"""Phase ratios from phase fields (update_phase_ratios_2D! / 3D!) without a GPU: the NumPy restatement the GPU tests check against
(tests/_phase_ratios.py) is itself checked against the reference's two tests with known answers (test/test_rheology.jl:444-501, test/test_phase_ratios3D.jl),
and the drop-in layers declare the feature: the C prototypes in include/jrx.h, the Julia methods of the extension, the integration table."""
import re

import numpy as np
import pytest

import _phase_ratios as PR
from _abi_parse import JULIA_EXT, ROOT, c_prototypes


def _reference_grid(nd):
    """range(0, 1; length = 5) and range(0.125, 0.875; length = 4) per dimension, as both reference tests build them"""
    return tuple(np.linspace(0.125, 0.875, 4) for _ in range(nd)), tuple(np.linspace(0.0, 1.0, 5) for _ in range(nd))


def _halves(nd):
    p1, p2 = np.zeros((4,) * nd), np.zeros((4,) * nd)
    p1[:2], p2[2:] = 1.0, 1.0
    return p1, p2


@pytest.mark.parametrize("nd", [2, 3])
def test_halves_split_along_x(nd):
    xci, xvi = _reference_grid(nd)
    p1, p2 = _halves(nd)
    out = PR.update_phase_ratios((p1, p2), xci, xvi)
    c = out["center"]
    assert np.array_equal(c[0], p1) and np.array_equal(c[1], p2)          # one phase per cell: the centres reproduce the input
    assert set(out) == set(PR.members(nd))
    for name, a in out.items():
        assert np.all(np.abs(a.sum(axis=0) - 1.0) <= 1e-15), name           # every ratio, on every grid, sums to one
    v = out["vertex"][(slice(None), 2) + (1,) * (nd - 1)]                   # vertex (3, 2[, 2]) lies on the phase boundary
    assert v[0] > 0.0 and v[1] > 0.0
    assert np.allclose(v, 0.5, rtol=0, atol=1e-15)


@pytest.mark.parametrize("nd", [2, 3])
def test_member_shapes(nd):
    ni = (4, 4, 4)[:nd]
    xci, xvi = _reference_grid(nd)
    out = PR.update_phase_ratios(_halves(nd), xci, xvi)
    want = {"center": ni, "vertex": tuple(n + 1 for n in ni), "Vx": (5,) + ni[1:], "Vy": (4, 5) + ni[2:]}
    if nd == 3:
        want.update(Vz=(4, 4, 5), xy=(5, 5, 4), yz=(4, 5, 5), xz=(5, 4, 5))      # test_phase_ratios3D.jl:56-60
    for name, shape in want.items():
        assert out[name].shape == (2,) + shape, name
        assert PR.member_shape(name, ni) == shape


@pytest.mark.parametrize("nd", [2, 3])
def test_tiny_third_phase_is_zeroed(nd):
    """the reference's threshold case: (0.6, 0.4, 1e-6) -- the third phase is below 1e-5 and comes out exactly 0, in every member"""
    xci, xvi = _reference_grid(nd)
    ps = [np.full((4,) * nd, v) for v in (0.6, 0.4, 1.0e-6)]
    out = PR.update_phase_ratios(ps, xci, xvi)
    for name, a in out.items():
        assert np.all(a[2] == 0.0), name
        assert np.all(np.abs(a[0] + a[1] - 1.0) <= 1e-15), name


@pytest.mark.parametrize("nd", [2, 3])
def test_boundary_nodes_reproduce_the_adjacent_cells(nd):
    """cells outside the grid are skipped, not read as zeros: a boundary face has W = 0.5 and carries its one cell's ratios"""
    rng = np.random.default_rng(20261019)
    ni = (5, 3, 2)[:nd]
    ps = [rng.uniform(0.05, 1.0, ni) for _ in range(3)]
    xci, xvi = PR.uniform_grid(ni, (2.0, 1.0, 0.5)[:nd])
    out = PR.update_phase_ratios(ps, xci, xvi)
    assert np.allclose(out["Vx"][:, 0], out["center"][:, 0], rtol=1e-14, atol=0) and np.allclose(out["Vx"][:, -1], out["center"][:, -1], rtol=1e-14, atol=0)
    corner = (slice(None),) + (0,) * nd
    assert np.allclose(out["vertex"][corner], out["center"][corner], rtol=1e-14, atol=0)


def readers(name, cell, ni):
    """mask over the nodes of member `name` that read the cell `cell`"""
    stag = PR.members(len(ni))[name]
    m = np.zeros(PR.member_shape(name, ni), dtype=bool)
    m[tuple(slice(c, c + 1 + s) for c, s in zip(cell, stag))] = True
    return m


@pytest.mark.parametrize("ni,cell", [((5, 4), (2, 1)), ((4, 3, 3), (1, 1, 1))])
def test_a_degenerate_cell_gives_nan_only_where_it_is_read(ni, cell):
    """a NaN in one cell: NaN for every phase at exactly the nodes that read the cell.  A cell whose arrays are all 0: its centre is 0 / 0 = NaN; a node that
    also reads a cell with material takes its ratios from that cell (the zero cell adds weight but no value, and the tail renormalises), so NaN appears
    only where every cell a node reads is empty -- the one-cell grid below"""
    rng = np.random.default_rng(3)
    ps = [rng.uniform(0.05, 1.0, ni) for _ in range(2)]
    grid = PR.uniform_grid(ni)
    clean = PR.update_phase_ratios(ps, *grid)
    qs = [p.copy() for p in ps]
    qs[0][cell] = np.nan
    out = PR.update_phase_ratios(qs, *grid)
    for name in PR.members(len(ni)):
        reads = readers(name, cell, ni)
        nan = np.isnan(out[name])
        assert np.array_equal(nan.all(axis=0), reads) and np.array_equal(nan.any(axis=0), reads), name
        assert np.array_equal(out[name][:, ~reads], clean[name][:, ~reads]), name
    qs = [p.copy() for p in ps]
    for q in qs:
        q[cell] = 0.0
    out = PR.update_phase_ratios(qs, *grid)
    for name in PR.members(len(ni)):
        reads = readers(name, cell, ni)
        nan = np.isnan(out[name])
        assert np.array_equal(nan.all(axis=0), reads if name == "center" else np.zeros_like(reads)), name
        assert np.array_equal(out[name][:, ~reads], clean[name][:, ~reads]), name
    one = (1,) * len(ni)
    out = PR.update_phase_ratios([np.zeros(one), np.zeros(one)], *PR.uniform_grid(one))
    for name, a in out.items():
        assert np.isnan(a).all(), name


def test_header_declares_the_entry_points():
    protos = c_prototypes()
    assert len(protos["jrx_update_phase_ratios2d"]) == 12
    assert len(protos["jrx_update_phase_ratios3d"]) == 17
    assert protos["jrx_update_phase_ratios2d"][5] == "Ptr{Ptr{Float64}}" and protos["jrx_update_phase_ratios3d"][9] == "Ptr{Ptr{Float64}}"
    tuning = (ROOT / "include" / "jrx_tuning.h").read_text()
    assert '"phase_ratios_fused"' in tuning


def test_extension_defines_the_methods():
    txt = JULIA_EXT.read_text()
    assert re.search(r"function JR2D\.update_phase_ratios_2D!\(", txt)
    assert re.search(r"function JR3D\.update_phase_ratios_3D!\(", txt)
    assert "jrx_update_phase_ratios2d" in txt and "jrx_update_phase_ratios3d" in txt


def test_integration_notes_list_the_update_as_provided():
    txt = (ROOT / "INTEGRATION.md").read_text()
    for line in txt.splitlines():
        if "not provided" in line:
            assert "update_phase_ratios" not in line, line
    assert "jrx_update_phase_ratios2d" in txt and "jrx_update_phase_ratios3d" in txt
