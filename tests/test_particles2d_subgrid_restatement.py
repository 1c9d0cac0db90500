"""CPU: the NumPy restatement of operators 10 and 11 of the particle section of include/jrx.h (tests/_particles2d_subgrid.py: subgrid_diffusion_centroid! and
subgrid_diffusion! with loc = :vertex), which tests/test_gpu_particles2d_subgrid.py holds the kernels of csrc/particles.hip to, pinned by properties that follow
from the seven steps of the definition and need no device; and the static side of the new interface: the declarations of the header, the exports of the library,
the ccalls of the Julia extension, the constructor and the checks the Python layer makes before the device."""
import numpy as np
import pytest

import _particles2d as PT
import _particles2d_stress as PS
import _particles2d_subgrid as SG
from _abi_parse import HEADER, ROOT, c_prototypes, julia_ccalls, same_arg

ENTRY_POINTS = ("jrx_particles2d_subgrid_diffusion_centroid", "jrx_particles2d_subgrid_diffusion_vertex")
NI = (7, 5)
DX, DY = 0.125, 0.09375
ORIGIN = (0.25, -0.5)
DT = 2.0e3
FORMS = ["center", "vertex"]


def _xvi(ni=NI):
    return tuple(ORIGIN[d] + np.arange(ni[d] + 1) * (DX, DY)[d] for d in range(2))


def _ext(loc, ni=NI):
    return ni if loc == "center" else (ni[0] + 1, ni[1] + 1)


def _cloud(ni=NI):
    """the restatement's cloud after one advect_rk2 + move under a rigid rotation: buckets unevenly filled, inactive slots in every cell"""
    p = PT.init_particles(4, 12, 2, _xvi(ni), ni, rng=np.random.default_rng(3))
    cx, cy = ORIGIN[0] + 0.5 * ni[0] * DX, ORIGIN[1] + 0.5 * ni[1] * DY
    w = 0.5 * min(DX, DY) / np.hypot(0.5 * ni[0] * DX, 0.5 * ni[1] * DY)
    xv, yv = _xvi(ni)
    xg, yg = ORIGIN[0] + (np.arange(ni[0] + 2) - 0.5) * DX, ORIGIN[1] + (np.arange(ni[1] + 2) - 0.5) * DY
    PT.advect_rk2(p, -w * (np.meshgrid(xv, yg, indexing="ij")[1] - cy), w * (np.meshgrid(xg, yv, indexing="ij")[0] - cx), 1.0)
    p, _, c = PT.move(p)
    assert c["n_far"] == 0 and c["n_overflow"] == 0
    return p


def _inputs(p, loc, seed=7):
    """(pT, T_grid, ΔT_grid, dt0): temperatures in [300, 1600], the grid's change in [-50, 50], dt₀ log-uniform over six decades around DT"""
    rng = np.random.default_rng(seed)
    act = p.active != 0
    pT = np.where(act, rng.uniform(300.0, 1600.0, act.shape), 0.0)
    T = rng.uniform(300.0, 1600.0, _ext(loc, (p.nx, p.ny)))
    dT = rng.uniform(-50.0, 50.0, T.shape)
    dt0 = np.where(act, DT * 10.0 ** rng.uniform(-3.0, 3.0, act.shape), 0.0)
    return pT, T, dT, dt0


def _to_particle(loc, old, F, p):
    return PS.centroid2particle(old, F, p) if loc == "center" else PT.grid2particle(F, p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------- the seven steps
@pytest.mark.parametrize("loc", FORMS)
def test_d_0_adds_the_interpolated_grid_change_and_nothing_else(loc):
    p = _cloud()
    pT, T, dT, dt0 = _inputs(p, loc)
    act = p.active != 0
    assert np.all(SG.factor(dt0, 0.0, DT) == 0.0)          # exp(-0) = 1 exactly
    out = SG.FORMS[loc](pT, T, dT, dt0, p, DT, d=0.0)
    assert np.array_equal(_bits(out["ΔT_subgrid"]), _bits(dT))          # ΔT_grid - (±0) num / den: the same bits
    back = _to_particle(loc, np.zeros(pT.shape), dT, p)
    assert np.array_equal(out["pT0"], pT) and np.array_equal(_bits(out["pΔT"]), _bits(back))
    assert np.array_equal(_bits(out["pT"]), _bits(np.where(act, pT + back, 0.0)))
    assert not np.array_equal(out["pT"][act], pT[act])
    # the ghosted form reads the same nodes and none of the ghosts
    g = np.full((dT.shape[0] + 2, dT.shape[1] + 2), np.nan)
    g[1:-1, 1:-1] = dT
    out2 = SG.FORMS[loc](pT, T, g, dt0, p, DT, d=0.0)
    assert all(np.array_equal(_bits(out[k]), _bits(out2[k])) for k in SG.OUTPUTS)


@pytest.mark.parametrize("loc", FORMS)
def test_a_particle_temperature_that_is_the_interpolant_of_the_grid_has_no_subgrid_part(loc):
    """pT = the interpolant of T_grid: δ = 0 in every slot whatever dt₀ is, so the whole of ΔT_grid comes back"""
    p = _cloud()
    _, T, dT, dt0 = _inputs(p, loc)
    act = p.active != 0
    dt0[tuple(np.argwhere(act)[0])] = 0.0
    pT = _to_particle(loc, np.zeros(p.px.shape), T, p)
    out = SG.FORMS[loc](pT, T, dT, dt0, p, DT, d=1.0)
    back = _to_particle(loc, np.zeros(pT.shape), dT, p)
    assert np.array_equal(out["pT0"], pT) and np.array_equal(out["ΔT_subgrid"], dT) and np.array_equal(out["pΔT"], back)
    assert np.array_equal(out["pT"], np.where(act, pT + back, 0.0))


@pytest.mark.parametrize("loc", FORMS)
def test_dt0_of_zero_and_nan_take_the_floor_and_give_finite_results(loc):
    p = _cloud()
    pT, T, dT, dt0 = _inputs(p, loc)
    a, b = (tuple(s) for s in np.argwhere(p.active != 0)[[0, -1]])
    dt0[a], dt0[b] = 0.0, np.nan
    f = SG.factor(dt0, 1.0, 1e-10)          # dt / floor = 0.1: a factor that tells the floor from anything else
    assert f[a] == f[b] == 1.0 - np.exp(-1e-10 / 1e-9) and 0.09 < f[a] < 0.1
    assert SG.factor(np.array([1e-9, 2e-9, -1.0, -np.inf, np.inf]), 1.0, 1e-10).tolist() == [f[a], 1.0 - np.exp(-1e-10 / 2e-9), f[a], f[a], 0.0]
    out = SG.FORMS[loc](pT, T, dT, dt0, p, DT, d=1.0)
    assert all(np.isfinite(out[k]).all() for k in SG.OUTPUTS)
    pTn = _to_particle(loc, pT, T, p)
    assert out["pT0"][a] == pT[a] + (pTn[a] - pT[a]) and out["pT0"][b] == pT[b] + (pTn[b] - pT[b])          # f = 1 at the floor with this dt


@pytest.mark.parametrize("loc", FORMS)
def test_a_long_step_relaxes_the_particle_to_the_grid_in_full(loc):
    """dt / dt₀ = 1e6 with d = 1: exp underflows, f == 1.0, pT0 becomes pT0 + (pTₙ - pT0)"""
    p = _cloud()
    pT, T, dT, _ = _inputs(p, loc)
    act = p.active != 0
    dt0 = np.where(act, DT * 1e-6, 0.0)
    assert np.all(SG.factor(dt0, 1.0, DT)[act] == 1.0)
    out = SG.FORMS[loc](pT, T, dT, dt0, p, DT, d=1.0)
    pTn = _to_particle(loc, pT, T, p)
    assert np.array_equal(out["pT0"][act], (pT + (pTn - pT))[act]) and np.array_equal(out["pT0"][~act], pT[~act])
    assert np.abs(out["pT0"] - pTn)[act].max() <= np.spacing(8192.0)          # two roundings of quantities below 8192: |pTₙ| <= 4 * 1600 where both pairs extrapolate
    assert all(np.all(_bits(out[k][~act]) == 0) for k in ("pT", "pT0", "pΔT"))          # +0.0 in every inactive slot


def test_steps_3_to_7_by_hand_on_one_cell():
    """two particles in one cell of a 2 x 2 grid, every other cell empty: the numbers of the definition written out"""
    ni = (2, 2)
    p = PT.init_particles(1, 3, 0, _xvi(ni), ni)
    p.active[:], p.px[:], p.py[:] = 0, 0.0, 0.0
    xc, yc = ORIGIN[0] + 1.5 * DX, ORIGIN[1] + 0.5 * DY
    p.active[1, 0, 0], p.px[1, 0, 0], p.py[1, 0, 0] = 1, xc, yc                          # at the centre: weight 1
    p.active[1, 0, 2], p.px[1, 0, 2], p.py[1, 0, 2] = 1, xc + 0.25 * DX, yc                # a quarter cell off: weight 0.75
    T = np.array([[400.0, 800.0], [600.0, 1000.0]])
    dT = np.array([[1.0, 2.0], [3.0, 4.0]])
    pT = np.zeros(p.px.shape)
    pT[1, 0, 0], pT[1, 0, 2] = 700.0, 500.0
    dt0 = np.zeros(p.px.shape)
    dt0[1, 0, 0], dt0[1, 0, 2] = 2.0, 4.0
    out = SG.subgrid_diffusion_centroid(pT, T, dT, dt0, p, 2.0, d=0.5)
    f0, f2 = 1.0 - np.exp(-0.5), 1.0 - np.exp(-0.25)
    pTn2 = (1.0 - 1.25) * 400.0 + 1.25 * 600.0          # along x the pair of centres is (0, 1) and the particle extrapolates beyond centre 1: tx = 1.25, ty = 0
    δ0, δ2 = (600.0 - 700.0) * f0, (pTn2 - 500.0) * f2
    assert out["pT0"][1, 0, 0] == 700.0 + δ0 and out["pT0"][1, 0, 2] == 500.0 + δ2
    sub = dT.copy()
    sub[1, 0] = 3.0 - (1.0 * δ0 + 0.75 * δ2) / (1.0 + 0.75)
    assert np.array_equal(out["ΔT_subgrid"], sub)          # the three empty cells: ΔT_grid itself
    r0 = sub[1, 0]
    r2 = (1.0 - 1.25) * sub[0, 0] + 1.25 * sub[1, 0]
    assert out["pΔT"][1, 0, 0] == r0 and out["pΔT"][1, 0, 2] == r2
    assert out["pT"][1, 0, 0] == (700.0 + δ0) + r0 and out["pT"][1, 0, 2] == (500.0 + δ2) + r2
    assert sum(int((out[k] != 0.0).sum()) for k in ("pT", "pT0", "pΔT")) == 6


def test_a_centre_cell_without_particles_keeps_the_whole_grid_change():
    p = _cloud()
    hole = (3, 2)
    p.active[hole], p.px[hole], p.py[hole] = 0, 0.0, 0.0
    den = PS.centre_den(p)
    assert den[hole] == 0.0 and (den == 0.0).sum() == 1
    pT, T, dT, dt0 = _inputs(p, "center")
    out = SG.subgrid_diffusion_centroid(pT, T, dT, dt0, p, DT, d=1.0)
    same = out["ΔT_subgrid"] == dT
    assert same[hole] and same.sum() == 1 and np.isfinite(out["pT"]).all()


def test_a_vertex_without_particles_around_it_keeps_the_whole_grid_change():
    p = _cloud()
    p.active[0, 0], p.px[0, 0], p.py[0, 0] = 0, 0.0, 0.0
    den = PS.vertex_den(p)
    assert den[0, 0] == 0.0 and (den == 0.0).sum() == 1
    pT, T, dT, dt0 = _inputs(p, "vertex")
    out = SG.subgrid_diffusion_vertex(pT, T, dT, dt0, p, DT, d=1.0)
    same = out["ΔT_subgrid"] == dT
    assert same[0, 0] and same.sum() == 1 and np.isfinite(out["pT"]).all()


def test_a_non_finite_coordinate_keeps_the_slot_in_the_centre_form_and_makes_nan_in_the_vertex_form():
    p = _cloud()
    a, b = (tuple(s) for s in np.argwhere(p.active != 0)[[5, -7]])
    assert a[:2] != b[:2]
    p.px[a], p.py[b] = np.nan, np.inf
    pT, T, dT, dt0 = _inputs(p, "center")
    out = SG.subgrid_diffusion_centroid(pT, T, dT, dt0, p, DT, d=1.0)
    # steps 2 and 6 leave the slot alone: δ = (pT0 - pT0) f = 0, so pT0, pΔT = 0 and pT come through; its cell's remainder is NaN through the weights of (7)
    for at in (a, b):
        assert out["pT0"][at] == pT[at] and out["pΔT"][at] == 0.0 and out["pT"][at] == pT[at] and np.isnan(out["ΔT_subgrid"][at[:2]])
    assert np.isnan(out["ΔT_subgrid"]).sum() == 2
    pT, T, dT, dt0 = _inputs(p, "vertex")
    out = SG.subgrid_diffusion_vertex(pT, T, dT, dt0, p, DT, d=1.0)
    assert all(np.isnan(out[k][at]) for k in ("pT", "pT0", "pΔT") for at in (a, b))


# ---------------------------------------------------------------------------------------------- the static side
def test_the_header_declares_the_entry_points_and_the_julia_extension_calls_them():
    protos, calls = c_prototypes(), julia_ccalls()
    want = ["Ptr{Cvoid}"] + ["Ptr{Float64}"] * 3 + ["Int32"] + ["Ptr{Float64}"] * 4 + ["Ref{JrxParticles2d}", "Float64", "Float64"]
    for fn in ENTRY_POINTS:
        assert fn in protos and fn in calls, fn
        assert len(protos[fn]) == len(want) and all(same_arg(w, g) for w, g in zip(protos[fn], want)), (fn, protos[fn])
        for ret, args in calls[fn]:
            assert ret == "Cint" and len(args) == len(protos[fn]) and all(same_arg(w, g) for w, g in zip(protos[fn], args)), (fn, protos[fn], args)
    txt = HEADER.read_text()
    sec = txt[txt.index("2D marker-in-cell particles"):]
    for s in ("10. subgrid_diffusion_centroid!", "11. subgrid_diffusion!", "particles_subgrid_fused", "JRX_SUBGRID_DT_GHOSTED", "Subduction2D.jl:221-243",
              "a > 1e-9 ? a : 1e-9"):
        assert s in sec, s
    assert '"particles_subgrid_fused"' in (ROOT / "include" / "jrx_tuning.h").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    assert all(fn in integ for fn in ENTRY_POINTS)
    row = [ln for ln in integ.splitlines() if "not provided" in ln and "inject_particles_phase!" in ln]
    assert len(row) == 1 and "subgrid_diffusion" not in row[0]


def test_the_library_exports_the_entry_points(jr):
    from justrelax_jl_amd import _lib
    L = _lib.load(check_symbols=True)
    for fn in ENTRY_POINTS:
        assert fn in _lib.declared_symbols() and hasattr(L, fn), fn
        assert getattr(L, fn)(None, None, None, None, 0, None, None, None, None, None, 1.0, 1.0) == 4          # a NULL handle is refused before anything is read
    assert (_lib.SUBGRID_DT_NODES, _lib.SUBGRID_DT_GHOSTED) == (0, 1)


def test_the_constructor_gives_the_four_members_in_column_major_order_and_no_twins(jr):
    from justrelax_jl_amd.arrays import is_fortran
    ni, B = (6, 5), jr.CPUBackend
    p = jr.init_particles(B, 4, 8, 1, _xvi(ni), ni)
    for kw, loc, ext in (({}, "vertex", (7, 6)), (dict(loc="vertex"), "vertex", (7, 6)), (dict(loc="center"), "center", ni), (dict(loc=":center"), "center", ni)):
        sa = jr.SubgridDiffusionCellArrays(p, **kw)
        assert sa.loc == loc and tuple(sa.ΔT_subgrid.shape) == ext
        for name in ("pT0", "pΔT", "dt0"):
            m = getattr(sa, name)
            assert tuple(m.shape) == (6, 5, 8) == p.shape and m.stride() == (1, 6, 30) and float(m.abs().max()) == 0.0
        assert all(is_fortran(getattr(sa, k)) for k in ("pT0", "pΔT", "dt0", "ΔT_subgrid")) and sa.ΔT_subgrid.stride() == (1, ext[0])
        assert len({getattr(sa, k).data_ptr() for k in ("pT0", "pΔT", "dt0", "ΔT_subgrid")}) == 4
    assert p._twins == {}
    with pytest.raises(ValueError, match="unknown loc"):
        jr.SubgridDiffusionCellArrays(p, loc="face")
    with pytest.raises(TypeError, match="init_particles"):
        jr.SubgridDiffusionCellArrays(ni)


def test_the_python_layer_checks_kinds_shapes_and_numbers_before_the_library(jr):
    ni, B = (6, 5), jr.CPUBackend
    p = jr.init_particles(B, 4, 8, 1, _xvi(ni), ni)
    (pT,) = jr.init_cell_arrays(p, 1)
    sc, sv = jr.SubgridDiffusionCellArrays(p, loc="center"), jr.SubgridDiffusionCellArrays(p)
    Z = lambda *s: jr.fzeros(s, p.device)
    cen, ver = jr.subgrid_diffusion_centroid_, jr.subgrid_diffusion_
    # each refuses the arrays of the other form by name
    with pytest.raises(ValueError, match=r"loc = 'vertex'.*needs 'center' \(subgrid_diffusion! takes 'vertex'\)"):
        cen(pT, Z(6, 5), Z(6, 5), sv, p, 1.0)
    with pytest.raises(ValueError, match=r"loc = 'center'.*needs 'vertex' \(subgrid_diffusion_centroid! takes 'center'\)"):
        ver(pT, Z(7, 6), Z(7, 6), sc, p, 1.0)
    with pytest.raises(TypeError, match="SubgridDiffusionCellArrays"):
        cen(pT, Z(6, 5), Z(6, 5), (pT, pT, pT), p, 1.0)
    with pytest.raises(TypeError, match="init_particles"):
        cen(pT, Z(6, 5), Z(6, 5), sc, sc, 1.0)
    # shapes
    with pytest.raises(ValueError, match="centre field"):
        cen(pT, Z(7, 6), Z(6, 5), sc, p, 1.0)
    with pytest.raises(ValueError, match="vertex field"):
        ver(pT, Z(6, 5), Z(7, 6), sv, p, 1.0)
    with pytest.raises(ValueError, match=r"ΔT_grid is \(7, 6\).*\(6, 5\) or.*\(8, 7\)"):
        cen(pT, Z(6, 5), Z(7, 6), sc, p, 1.0)
    with pytest.raises(ValueError, match=r"ΔT_grid is \(8, 7\).*\(7, 6\) or.*\(9, 8\)"):
        ver(pT, Z(7, 6), Z(8, 7), sv, p, 1.0)
    with pytest.raises(ValueError, match="pT must be an fp64 array"):
        cen(Z(6, 5), Z(6, 5), Z(6, 5), sc, p, 1.0)
    q = jr.init_particles(B, 4, 8, 1, _xvi((5, 5)), (5, 5))
    with pytest.raises(ValueError, match="was made for"):
        cen(jr.init_cell_arrays(q, 1)[0], Z(5, 5), Z(5, 5), sc, q, 1.0)
    bad = jr.SubgridDiffusionCellArrays(p, loc="center")
    bad.pΔT = Z(6, 5, 7)
    with pytest.raises(ValueError, match="subgrid_arrays.pΔT must be"):
        cen(pT, Z(6, 5), Z(6, 5), bad, p, 1.0)
    q = jr.init_particles(B, 4, 8, 1, _xvi((1, 5)), (1, 5))
    with pytest.raises(ValueError, match="nx >= 2"):
        cen(jr.init_cell_arrays(q, 1)[0], Z(1, 5), Z(1, 5), jr.SubgridDiffusionCellArrays(q, loc="center"), q, 1.0)
    # numbers
    for d in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"d = .* \[0, 1\]"):
            cen(pT, Z(6, 5), Z(6, 5), sc, p, 1.0, d=d)
    for dt in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dt = .*finite and not negative"):
            ver(pT, Z(7, 6), Z(7, 6), sv, p, dt)
    # ... and CPU arrays are refused with the text every operator uses: there is no CPU path; the ghosted ΔT and the vertex form with one cell along x get this far
    q1 = jr.init_particles(B, 4, 8, 1, _xvi((1, 5)), (1, 5))
    for call in (lambda: cen(pT, Z(6, 5), Z(6, 5), sc, p, 1.0), lambda: cen(pT, Z(6, 5), Z(8, 7), sc, p, 0.0, d=0.0), lambda: ver(pT, Z(7, 6), Z(7, 6), sv, p, 1.0, d=0.3),
                 lambda: ver(pT, Z(7, 6), Z(9, 8), sv, p, 1.0),
                 lambda: ver(jr.init_cell_arrays(q1, 1)[0], Z(2, 6), Z(2, 6), jr.SubgridDiffusionCellArrays(q1), q1, 1.0),
                 lambda: jr.centroid2particle_(sc.dt0, Z(6, 5), p)):
        with pytest.raises(NotImplementedError, match="CPU arrays"):
            call()
    assert float(pT.abs().max()) == 0.0 and float(sc.ΔT_subgrid.abs().max()) == 0.0
