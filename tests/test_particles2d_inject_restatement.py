"""CPU: the NumPy restatement of operator 12, inject_particles_phase! in gather form (tests/_particles2d_inject.py), which tests/test_gpu_particles2d_inject.py
holds k_pt_inject of csrc/particles.hip to bit for bit, pinned by a known answer and by properties that follow from the definition in include/jrx.h; and the
static side: the declaration of the header, the ccall of the Julia extension, the ctypes mirror, the export, the rows of INTEGRATION.md and the refusals of the
Python layer."""
import ctypes as C

import numpy as np
import pytest

import _particles2d as PT
import _particles2d_inject as INJ
from _abi_parse import HEADER, ROOT, c_prototypes, julia_ccalls, same_arg

ENTRY = "jrx_particles2d_inject"
DX, DY = 0.125, 0.09375
ORIGIN = (0.25, -0.5)


def _xvi(ni):
    return tuple(ORIGIN[d] + np.arange(ni[d] + 1) * (DX, DY)[d] for d in range(2))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _rotation_V(ni, courant=0.5):
    nx, ny = ni
    cx, cy = ORIGIN[0] + 0.5 * nx * DX, ORIGIN[1] + 0.5 * ny * DY
    w = courant * min(DX, DY) / np.hypot(0.5 * nx * DX, 0.5 * ny * DY)
    xv, yv = ORIGIN[0] + np.arange(nx + 1) * DX, ORIGIN[1] + np.arange(ny + 1) * DY
    xg, yg = ORIGIN[0] + (np.arange(nx + 2) - 0.5) * DX, ORIGIN[1] + (np.arange(ny + 2) - 0.5) * DY
    return -w * (np.add.outer(0.0 * xv, yg) - cy), w * (np.add.outer(xg, 0.0 * yv) - cx)


def _site_sets(p):
    """per cell, the set of (px bits, py bits) of its active slots"""
    return {(i, j): {(int(_bits(p.px[i, j, s:s + 1])[0]), int(_bits(p.py[i, j, s:s + 1])[0])) for s in range(p.max_xcell) if p.active[i, j, s]}
            for i in range(p.nx) for j in range(p.ny)}


# ---------------------------------------------------------------------------------------------- the known answer
@pytest.mark.parametrize("nxcell,lattice", [(4, (2, 2)), (6, (2, 3))])
def test_refilling_a_thinned_lattice_cloud_gives_back_the_seeded_points_bit_for_bit(nxcell, lattice):
    ni = (6, 5)
    full = PT.init_particles(nxcell, 2 * nxcell, nxcell, _xvi(ni), ni)
    assert PT.lattice(nxcell) == lattice
    p = PT.copy(full)
    rng = np.random.default_rng(12)
    gone = (rng.random(p.active.shape) < 0.4) & (p.active != 0)
    gone[2, 3, :] = p.active[2, 3, :] != 0          # one cell is emptied altogether: its neighbours are its donors
    p.active[gone], p.px[gone], p.py[gone] = 0, 0.0, 0.0
    ph = np.where(p.active != 0, 2.0, 0.0)
    out, c = INJ.inject(p, ph, min_xcell=nxcell)
    assert c["n_injected"] == int(gone.sum()) > 0 and c["n_no_donor"] == 0 and c["n_active_after"] == nxcell * ni[0] * ni[1]
    assert c["n_deficient"] == int(gone.any(axis=2).sum()) and c["n_active_after"] == c["n_active_before"] + c["n_injected"]
    p.active = out
    assert _site_sets(p) == _site_sets(full)
    assert np.all(ph[out != 0] == 2.0) and np.all(ph[out == 0] == 0.0)
    # the new particles took the lowest slots that were free: the slots the seeding filled
    assert np.all(out[:, :, :nxcell] == 1) and np.all(out[:, :, nxcell:] == 0)


# ---------------------------------------------------------------------------------------------- properties
def _moved_cloud(ni=(9, 7), seed=5):
    p = PT.init_particles(4, 12, 3, _xvi(ni), ni, rng=np.random.default_rng(seed))
    a = p.active != 0
    ph = np.where(a, 1.0 + (np.arange(a.size).reshape(a.shape) % 3), 0.0)
    pid = np.where(a, np.arange(a.size).reshape(a.shape) + 1.0, 0.0)
    Vx, Vy = _rotation_V(ni)
    PT.advect_rk2(p, Vx, Vy, 1.0)
    p, (ph, pid), c = PT.move(p, (ph, pid))
    assert c["n_far"] == 0 and c["n_overflow"] == 0
    return p, ph, pid


@pytest.mark.parametrize("min_xcell", [3, 4])
def test_properties_of_an_injection_after_a_rotation_step_and_a_move(min_xcell):
    p, ph, pid = _moved_cloud()
    nx, ny = p.nx, p.ny
    rng = np.random.default_rng(2)
    Tv, Tc = rng.uniform(300.0, 1600.0, (nx + 1, ny + 1)), rng.uniform(-1.0, 1.0, (nx, ny))
    pT, pC, unlisted = np.where(p.active != 0, 500.0, 0.0), np.where(p.active != 0, 0.25, 0.0), np.where(p.active != 0, 9.0, 0.0)
    before = PT.copy(p)
    b_fields = [x.copy() for x in (ph, pid, pT, pC, unlisted)]
    assert int(((p.active != 0).sum(axis=2) < min_xcell).sum()) > 0          # something to do
    out, c = INJ.inject(p, ph, (pT, pC, pid), (Tv, Tc, None), (INJ.VERTEX, INJ.CENTRE, INJ.DONOR), min_xcell=min_xcell)
    old, new = before.active != 0, (out != 0) & (before.active == 0)
    # the counts
    assert c["n_active_before"] == int(old.sum()) and c["n_injected"] == int(new.sum()) > 0 and c["n_active_after"] == c["n_active_before"] + c["n_injected"]
    assert c["n_deficient"] == int((old.sum(axis=2) < min_xcell).sum()) and np.array_equal(p.active, before.active)
    # every cell ends with min_xcell particles at the least -- here every cell has a donor
    assert c["n_no_donor"] == 0 and np.all((out != 0).sum(axis=2) >= min_xcell)
    assert np.all((out != 0).sum(axis=2)[old.sum(axis=2) < min_xcell] == min_xcell)          # ... and no more than asked for
    # donors and every slot active at entry are bitwise unchanged, in every array; an untouched inactive slot keeps +0.0
    for a, b in zip((p.px, p.py, ph, pid, pT, pC, unlisted), [before.px, before.py] + b_fields):
        assert np.array_equal(_bits(a)[old], _bits(b)[old]) and np.all(_bits(a)[~old & ~new] == 0)
    assert np.all(_bits(unlisted)[new] == 0)          # a field that is not listed keeps +0.0 in the new slots
    # new points lie in their bucket cell, on distinct sites nobody occupied, in the lowest free slots
    nsx, nsy = PT.lattice(p.nxcell)
    for i, j, s in zip(*np.nonzero(new)):
        assert PT.owner(p, p.px[i, j, s], p.py[i, j, s]) == (i, j)
        assert not np.any(~(out[i, j, :s] != 0))          # nothing free below a new particle
    def site(i, j, s):
        return (int(np.floor(((p.px[i, j, s] - (p.x0 + float(i) * p.dx)) * p._dx) * float(nsx))),
                int(np.floor(((p.py[i, j, s] - (p.y0 + float(j) * p.dy)) * p._dy) * float(nsy))))
    for i, j in zip(*np.nonzero(new.any(axis=2))):
        taken = {site(i, j, s) for s in np.nonzero(old[i, j])[0]}
        fresh = [site(i, j, s) for s in np.nonzero(new[i, j])[0]]
        assert len(set(fresh)) == len(fresh) and not set(fresh) & taken and all(0 <= a < nsx and 0 <= b < nsy for a, b in fresh), (i, j, fresh, taken)
    # the phase and the donor-copied field come from one particle active at entry, within one cell of the new one, and no entry particle is nearer
    ids = {b_fields[1][idx]: idx for idx in zip(*np.nonzero(old))}
    for i, j, s in zip(*np.nonzero(new)):
        d = ids[pid[i, j, s]]
        assert abs(d[0] - i) <= 1 and abs(d[1] - j) <= 1 and ph[i, j, s] == b_fields[0][d]
        d2 = (before.px - p.px[i, j, s]) ** 2 + (before.py - p.py[i, j, s]) ** 2
        near = old & (np.abs(np.arange(nx)[:, None, None] - i) <= 1) & (np.abs(np.arange(ny)[None, :, None] - j) <= 1)
        assert d2[d] == d2[near].min()
    # the vertex field at the new point: inside the range of its cell's four vertices; the centre field: that of the interpolant
    for i, j, s in zip(*np.nonzero(new)):
        corners = Tv[i:i + 2, j:j + 2]
        assert corners.min() - 1e-9 <= pT[i, j, s] <= corners.max() + 1e-9
        v, ok = PT.interp(Tc, p.x0 + 0.5 * p.dx, p.y0 + 0.5 * p.dy, p._dx, p._dy, p.px[i, j, s:s + 1], p.py[i, j, s:s + 1])
        assert ok[0] and pC[i, j, s] == v[0]
    # a second call finds nothing to do
    p.active = out
    snap = [x.copy() for x in (p.px, p.py, ph, pid, pT, pC)]
    out2, c2 = INJ.inject(p, ph, (pT, pC, pid), (Tv, Tc, None), (INJ.VERTEX, INJ.CENTRE, INJ.DONOR), min_xcell=min_xcell)
    assert c2["n_injected"] == 0 and c2["n_deficient"] == 0 and c2["n_active_before"] == c["n_active_after"] and np.array_equal(out2, out)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((p.px, p.py, ph, pid, pT, pC), snap))


def test_a_block_of_empty_cells_heals_from_its_rim_inwards_one_ring_per_call():
    ni = (9, 9)
    p = PT.init_particles(4, 8, 4, _xvi(ni), ni, rng=np.random.default_rng(1))
    p.active[2:7, 2:7, :], p.px[2:7, 2:7, :], p.py[2:7, 2:7, :] = 0, 0.0, 0.0
    ph = np.where(p.active != 0, 1.0, 0.0)
    for call, (injected, no_donor) in enumerate([(16 * 4, 9), (8 * 4, 1), (4, 0), (0, 0)]):
        out, c = INJ.inject(p, ph)          # min_xcell and the lattice are the particles' own
        assert (c["n_injected"], c["n_no_donor"]) == (injected, no_donor), (call, c)
        assert c["n_deficient"] == [25, 9, 1, 0][call] and c["n_active_after"] == c["n_active_before"] + c["n_injected"]
        p.active = out
    assert np.all((p.active != 0).sum(axis=2) == 4) and np.all(ph[p.active != 0] == 1.0)


def test_a_displaced_or_non_finite_particle_counts_in_n_and_occupies_no_site_and_ties_keep_the_first():
    ni = (3, 3)
    p = PT.init_particles(4, 6, 3, (np.arange(4.0), np.arange(4.0)), ni)
    p.active[:], p.px[:], p.py[:] = 0, 0.0, 0.0
    ph = np.zeros_like(p.px)

    def put(i, j, s, x, y, phase):
        p.active[i, j, s], p.px[i, j, s], p.py[i, j, s], ph[i, j, s] = 1, x, y, phase
    put(1, 1, 0, np.nan, 1.5, 7.0)          # counts, occupies nothing, never a donor
    put(1, 1, 2, 2.25, 1.25, 5.0)           # bucket (1, 1), owner (2, 1): counts, occupies nothing, a donor like any other
    put(0, 0, 1, 0.25, 0.25, 3.0)           # two donors at one point in one bucket ...
    put(0, 0, 3, 0.25, 0.25, 4.0)
    out, c = INJ.inject(p, ph, min_xcell=3)
    # cell (1, 1): n = 2, one new particle on site 0 at (1.25, 1.25) in slot 1; nearest finite donors are (2.25, 1.25) at distance 1 and (0.25, 0.25) at sqrt 2
    assert out[1, 1].tolist() == [1, 1, 1, 0, 0, 0] and (p.px[1, 1, 1], p.py[1, 1, 1], ph[1, 1, 1]) == (1.25, 1.25, 5.0)
    # cell (0, 0): n = 2 on one site; a new particle on site 1 at (0.75, 0.25): both donors are equally near, the first slot wins
    assert out[0, 0].tolist() == [1, 1, 0, 1, 0, 0] and (p.px[0, 0, 0], p.py[0, 0, 0], ph[0, 0, 0]) == (0.75, 0.25, 3.0)
    assert 7.0 not in ph[(out != 0) & (p.active == 0)]
    # every other cell is a neighbour of bucket (1, 1) and takes three particles from its finite donor or from (0, 0)'s
    assert c == dict(n_active_before=4, n_active_after=27, n_deficient=9, n_injected=23, n_no_donor=0)


# ---------------------------------------------------------------------------------------------- the static side
def test_the_header_the_binding_and_the_julia_extension_agree_on_the_entry_point():
    protos, calls = c_prototypes(), julia_ccalls()
    want = ["Ptr{Cvoid}", "Ref{JrxParticles2d}", "Ptr{Int32}", "Ptr{Float64}", "Ptr{Ptr{Float64}}", "Ptr{Ptr{Float64}}", "Ptr{Int32}", "Int32", "Int32", "Int32",
            "Int32", "Ptr{Int64}"]
    assert protos.get(ENTRY) == want
    assert ENTRY in calls, f"the Julia extension never calls {ENTRY}"
    for ret, args in calls[ENTRY]:
        assert ret == "Cint" and len(args) == len(want) and all(same_arg(w, g) for w, g in zip(want, args)), args
    txt = HEADER.read_text()
    sec = txt[txt.index("2D marker-in-cell particles"):]
    for s in ("12. inject_particles_phase!", "#define JRX_INJECT_VERTEX 0", "#define JRX_INJECT_CENTRE 1", "#define JRX_INJECT_DONOR  2", "OUT OF PLACE", "n_no_donor",
              "d2 < best", "Subduction2D.jl:246-263", "nsx nsy <= 64"):
        assert s in sec, s
    scope = sec[sec.index("NOT built"):sec.index("Layout.")]
    assert "inject_particles_phase" not in scope and "particle injection" not in scope
    ext = (ROOT / "ext" / "JustRelaxHIPNativeExt.jl").read_text()
    assert "function hip_inject_particles_phase!(p::HIPParticles2D" in ext


def test_the_library_exports_the_entry_point_and_refuses_a_null_handle(jr):
    from justrelax_jl_amd import _lib
    L = _lib.load(check_symbols=True)
    assert ENTRY in _lib.declared_symbols() and hasattr(L, ENTRY)
    assert (_lib.INJECT_VERTEX, _lib.INJECT_CENTRE, _lib.INJECT_DONOR) == (0, 1, 2)
    assert L.jrx_particles2d_inject(None, None, None, None, None, None, None, 0, 1, 1, 1, None) == 4
    assert len(L.jrx_particles2d_inject.argtypes) == len(c_prototypes()[ENTRY])


def test_integration_md_has_a_row_for_the_operator_and_one_row_for_what_is_not_provided():
    lines = (ROOT / "INTEGRATION.md").read_text().splitlines()
    rows = [ln for ln in lines if ENTRY in ln]
    assert len(rows) == 1 and "inject_particles_phase!" in rows[0] and "not provided" not in rows[0] and "hip_inject_particles_phase!" in rows[0]
    rest = [ln for ln in lines if "not provided" in ln and "inject_particles_phase!" in ln]
    assert len(rest) == 1 and "subgrid_diffusion" not in rest[0] and "3D" in rest[0] and "next step" not in rest[0]


# ---------------------------------------------------------------------------------------------- the Python layer
def test_the_python_layer_checks_before_the_device_and_no_longer_says_not_built(jr):
    ni, B = (6, 5), jr.CPUBackend
    p = jr.init_particles(B, 4, 8, 2, _xvi(ni), ni)
    pPhases, pT, pC = jr.init_cell_arrays(p, 3)
    Z = lambda *s: jr.fzeros(s, p.device)
    inj = jr.inject_particles_phase_
    with pytest.raises(NotImplementedError, match="not built"):
        inj()          # the call without particles, as before
    with pytest.raises(TypeError, match="init_particles"):
        inj(ni, pPhases)
    with pytest.raises(ValueError, match="pPhases must be an fp64 array"):
        inj(p, Z(6, 5))
    with pytest.raises(ValueError, match="2 particle fields and 1 grid fields"):
        inj(p, pPhases, (pT, pC), (Z(7, 6),))
    with pytest.raises(ValueError, match=r"args\[1\] must be an fp64 array"):
        inj(p, pPhases, (pT, Z(6, 5, 7)), (None, None))
    with pytest.raises(ValueError, match=r"fields\[0\] is \(7, 5\)"):
        inj(p, pPhases, (pT,), (Z(7, 5),))
    with pytest.raises(ValueError, match=r"fields\[0\] is tuple"):
        inj(p, pPhases, (pT,), ((),))
    with pytest.raises(ValueError, match=r"args\[1\] is pPhases"):
        inj(p, pPhases, (pT, pPhases), (None, None))
    with pytest.raises(ValueError, match="listed twice"):
        inj(p, pPhases, (pT, pT), (None, Z(7, 6)))
    with pytest.raises(ValueError, match=r"loc\[0\] = 'center', but fields\[0\] is \(7, 6\): a vertex field"):
        inj(p, pPhases, (pT,), (Z(7, 6),), loc=("center",))
    with pytest.raises(ValueError, match=r"loc\[1\] = 'vertex', but fields\[1\] is None"):
        inj(p, pPhases, (pT, pC), (Z(7, 6), None), loc=("vertex", "vertex"))
    with pytest.raises(ValueError, match="unknown loc"):
        inj(p, pPhases, (pT,), (None,), loc=("face",))
    with pytest.raises(ValueError, match="loc names 2 kinds"):
        inj(p, pPhases, (pT,), (None,), loc=("donor", "donor"))
    for bad in (0, -1, 5, 9):          # nxcell = 4 sites, max_xcell = 8
        with pytest.raises(ValueError, match=f"min_xcell = {bad} "):
            inj(p, pPhases, min_xcell=bad)
    p0 = jr.init_particles(B, 4, 8, 0, _xvi(ni), ni)
    with pytest.raises(ValueError, match="min_xcell = 0 "):
        inj(p0, jr.init_cell_arrays(p0, 1)[0])          # the particles' own min_xcell is the default
    q = jr.init_particles(B, 4, 8, 2, _xvi((1, 5)), (1, 5))
    (qph, qT) = jr.init_cell_arrays(q, 2)
    with pytest.raises(ValueError, match="nx >= 2"):
        inj(q, qph, (qT,), (Z(1, 5),))
    # with particles the call gets as far as the device: there is no CPU path, and that is what it says
    index, index2 = p.index, p._index2
    for call in (lambda: inj(p, pPhases), lambda: inj(p, pPhases, (), ()), lambda: inj(p, pPhases, (pT, pC), (Z(7, 6), Z(6, 5)), loc=(":vertex", "center")),
                 lambda: inj(p, pPhases, (pT, pC), (None, Z(6, 5)), min_xcell=4), lambda: inj(q, qph, (qT,), (Z(2, 6),))):
        with pytest.raises(NotImplementedError, match="CPU arrays") as e:
            call()
        assert "not built" not in str(e.value)
    assert p.index is index and p._index2 is index2 and float(pT.abs().max()) == 0.0          # a refused call swaps nothing
