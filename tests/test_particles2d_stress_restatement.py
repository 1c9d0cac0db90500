"""CPU: the NumPy restatement of operators 6 - 9 of the particle section of include/jrx.h (tests/_particles2d_stress.py: centroid2particle!,
particle2centroid!, rotate_stress_particles!, rotate_stress! on particles and stress2grid!), which tests/test_gpu_particles2d_stress.py holds the kernels of
csrc/particles.hip to, pinned by closed forms that follow from the definitions; and the static side of the new interface: the declarations of the header,
the exports of the library, the ccalls of the Julia extension and the checks the Python layer makes before the device."""
import numpy as np
import pytest

import _particles2d as PT
import _particles2d_stress as PS
from _abi_parse import HEADER, ROOT, c_prototypes, julia_ccalls, same_arg
from _stress_rotation import rot2

ENTRY_POINTS = ("jrx_particles2d_centroid2particle", "jrx_particles2d_particle2centroid", "jrx_particles2d_rotate", "jrx_particles2d_rotate_stress",
                "jrx_particles2d_stress2grid")
NI = (7, 5)
DX, DY = 0.125, 0.09375
ORIGIN = (0.25, -0.5)


def _xvi(ni=NI):
    return tuple(ORIGIN[d] + np.arange(ni[d] + 1) * (DX, DY)[d] for d in range(2))


def _cloud(ni=NI, nxcell=4, max_xcell=12, seed=3):
    return PT.init_particles(nxcell, max_xcell, 2, _xvi(ni), ni, rng=np.random.default_rng(seed))


def _particle_fields(p, n, seed=5):
    rng = np.random.default_rng(seed)
    return tuple(np.where(p.active != 0, rng.uniform(-3.0, 3.0, p.px.shape), 0.0) for _ in range(n))


# ---------------------------------------------------------------------------------------------- operator 6
@pytest.mark.parametrize("ni", [(2, 2), NI])
def test_centroid2particle_reproduces_a_plane_everywhere_the_outer_half_cells_included(ni):
    """a + b x + c y sampled at the centres is returned at every particle: the interpolant is linear between the pair and extrapolates linearly outside it.
    Bound: the evaluation is a handful of roundings of quantities no larger than the field's magnitude M (|t| <= 1.5): 16 ulp(M)."""
    p = _cloud(ni)
    a, b, c = 1.5, -2.25, 0.75
    xc, yc = p.x0 + (np.arange(ni[0]) + 0.5) * DX, p.y0 + (np.arange(ni[1]) + 0.5) * DY
    F = a + b * xc[:, None] + c * yc[None, :]
    old = np.full(p.px.shape, -9.0)
    got = PS.centroid2particle(old, F, p)
    act = p.active != 0
    M = np.abs(F).max()
    outer = act & ((p.px < xc[0]) | (p.px > xc[-1]) | (p.py < yc[0]) | (p.py > yc[-1]))
    assert outer.sum() > 0 and (ni != (2, 2) or 2 * outer.sum() > act.sum())          # in a 2 x 2 grid three quarters of the area extrapolate along x or y
    assert np.abs(got - (a + b * p.px + c * p.py))[act].max() <= 16 * np.spacing(M)
    assert np.all(got[~act] == 0.0) and not np.signbit(got[~act]).any()


def test_centroid2particle_leaves_a_slot_with_a_non_finite_coordinate_as_it_was():
    p = _cloud()
    F = np.random.default_rng(1).uniform(-1.0, 1.0, NI)
    old = np.full(p.px.shape, -9.0)
    clean = PS.centroid2particle(old, F, p)
    p.px[3, 2, 1], p.py[0, 0, 0] = np.nan, np.inf
    got = PS.centroid2particle(old, F, p)
    assert got[3, 2, 1] == -9.0 and got[0, 0, 0] == -9.0
    diff = got != clean
    assert diff.sum() == 2 and diff[3, 2, 1] and diff[0, 0, 0]


# ---------------------------------------------------------------------------------------------- operator 7
def test_particle2centroid_of_a_constant_a_single_particle_and_an_emptied_cell():
    p = _cloud()
    act = p.active != 0
    old = np.full(NI, -9.0)
    got = PS.particle2centroid(old, np.where(act, 2.5, 0.0), p)
    assert np.abs(got - 2.5).max() <= 4 * np.spacing(2.5)          # num / den with num = 2.5 den up to the roundings of the sums
    # one particle exactly at the centre of its cell: weight 1, its own value
    q = PT.copy(p)
    q.active[2, 3, :], q.px[2, 3, :], q.py[2, 3, :] = 0, 0.0, 0.0
    q.active[2, 3, 5], q.px[2, 3, 5], q.py[2, 3, 5] = 1, q.x0 + 2.5 * DX, q.y0 + 3.5 * DY
    pF = _particle_fields(q, 1)[0]
    pF[2, 3, 5] = 1.0 / 3.0
    got = PS.particle2centroid(old, pF, q)
    assert got[2, 3] == 1.0 / 3.0 and PS.centroid_sums(pF, q, 2, 3) == (1.0 / 3.0, 1.0)
    # an emptied cell keeps its old value, every other cell is written
    q.active[2, 3, 5], q.px[2, 3, 5], q.py[2, 3, 5] = 0, 0.0, 0.0
    got = PS.particle2centroid(old, pF, q)
    assert got[2, 3] == -9.0 and (got == -9.0).sum() == 1
    den = PS.centre_den(q)
    assert den[2, 3] == 0.0 and (den == 0.0).sum() == 1


# ---------------------------------------------------------------------------------------------- operator 8
def _invariants(xx, yy, xy):
    return xx + yy, 0.25 * (xx - yy) ** 2 + xy ** 2          # the trace and the second invariant of the deviator, both kept by a rotation


def test_the_matrix_rotation_keeps_the_invariants_composes_and_turns_a_quarter():
    p = _cloud()
    xx, yy, xy, w = _particle_fields(p, 4)
    act = p.active != 0
    M = max(np.abs(f).max() for f in (xx, yy, xy))
    oxx, oyy, oxy = PS.rotate((xx, yy, xy), w, p, 0.3, "matrix")
    t0, j0 = _invariants(xx, yy, xy)
    t1, j1 = _invariants(oxx, oyy, oxy)
    assert np.abs(t1 - t0).max() <= 16 * np.spacing(M) and np.abs(j1 - j0).max() <= 64 * np.spacing(M * M)
    assert not np.array_equal(oxx[act], xx[act]) and np.array_equal(oxx[~act], xx[~act])
    # N steps of θ / N equal one step of θ (rotations compose): 8 steps, each a few ulp
    N = 8
    s = (xx, yy, xy)
    for _ in range(N):
        s = PS.rotate(s, w, p, 0.3 / N, "matrix")
    assert max(np.abs(a - b).max() for a, b in zip(s, (oxx, oyy, oxy))) <= 16 * N * np.spacing(M)
    # θ = π / 2: (xx, yy, xy) -> (yy, xx, -xy), up to cos(π / 2) = 6e-17
    q = PS.rotate((xx, yy, xy), np.where(act, 1.0, 0.0), p, np.pi / 2, "matrix")
    assert max(np.abs(a - b)[act].max() for a, b in zip(q, (yy, xx, -xy))) <= 16 * np.spacing(M)


def test_the_jaumann_rotation_is_its_three_formulas_exactly():
    p = _cloud()
    xx, yy, xy, w = _particle_fields(p, 4)
    act = p.active != 0
    dt = 0.3
    oxx, oyy, oxy = PS.rotate((xx, yy, xy), w, p, dt, "jaumann")
    θ = dt * w
    assert np.array_equal(oxx[act], (xx - (2.0 * θ) * xy)[act]) and np.array_equal(oyy[act], (yy + (2.0 * θ) * xy)[act])
    assert np.array_equal(oxy[act], (xy + θ * (xx - yy))[act])
    assert np.abs((oxx + oyy) - (xx + yy)).max() <= 8 * np.spacing(16.0)          # the trace is kept (-2θ xy on xx, +2θ xy on yy); |oxx|, |oyy| <= 3 + 0.6 * 9
    assert np.all(oxx[~act] == 0.0) and np.all(oxy[~act] == 0.0)
    assert all(np.array_equal(a, b) for a, b in zip(rot2(xx, yy, xy, θ, "jaumann"), (xx - (2.0 * θ) * xy, yy + (2.0 * θ) * xy, xy + θ * (xx - yy))))


# ---------------------------------------------------------------------------------------------- operator 9
def _advected_cloud(ni=NI):
    p = _cloud(ni)
    cx, cy = ORIGIN[0] + 0.5 * ni[0] * DX, ORIGIN[1] + 0.5 * ni[1] * DY
    w = 0.5 * min(DX, DY) / np.hypot(0.5 * ni[0] * DX, 0.5 * ni[1] * DY)
    xv, yv = _xvi(ni)
    xg, yg = ORIGIN[0] + (np.arange(ni[0] + 2) - 0.5) * DX, ORIGIN[1] + (np.arange(ni[1] + 2) - 0.5) * DY
    Vx = -w * (np.meshgrid(xv, yg, indexing="ij")[1] - cy)
    Vy = w * (np.meshgrid(xg, yv, indexing="ij")[0] - cx)
    PT.advect_rk2(p, Vx, Vy, 1.0)
    p, _, c = PT.move(p)
    assert c["n_far"] == 0 and c["n_overflow"] == 0
    return p


def test_stress2grid_is_three_particle2centroid_and_three_particle2grid():
    p = _advected_cloud()
    pτ = _particle_fields(p, 3)
    rng = np.random.default_rng(2)
    old = {k: rng.uniform(-1.0, 1.0, (NI if k in ("xx", "yy", "xy_c") else (NI[0] + 1, NI[1] + 1))) for k in PS.TAU_O}
    got = PS.stress2grid(old, pτ, p)
    want = dict(xx=PS.particle2centroid(old["xx"], pτ[0], p), yy=PS.particle2centroid(old["yy"], pτ[1], p), xy_c=PS.particle2centroid(old["xy_c"], pτ[2], p),
                xx_v=PT.particle2grid(old["xx_v"], pτ[0], p), yy_v=PT.particle2grid(old["yy_v"], pτ[1], p), xy=PT.particle2grid(old["xy"], pτ[2], p))
    assert list(got) == ["xx", "yy", "xy_c", "xy", "xx_v", "yy_v"] == list(PS.TAU_O)
    assert all(np.array_equal(got[k], want[k]) and not np.array_equal(got[k], old[k]) for k in PS.TAU_O)
    assert PS.vertex_den(p).min() > 0.0 and PS.centre_den(p).min() > 0.0


@pytest.mark.parametrize("method", ["matrix", "jaumann"])
def test_rotate_stress_is_its_five_step_chain(method):
    p = _advected_cloud()
    p.px[1, 1, 0] = np.nan          # an active slot with a NaN coordinate: xx, yy kept, xy and ω NaN, so the rotation makes all three NaN
    assert p.active[1, 1, 0] == 1
    rng = np.random.default_rng(4)
    τxx, τyy = rng.uniform(-1.0, 1.0, NI), rng.uniform(-1.0, 1.0, NI)
    τxy, ωxy = rng.uniform(-1.0, 1.0, (NI[0] + 1, NI[1] + 1)), rng.uniform(-1.0, 1.0, (NI[0] + 1, NI[1] + 1))
    old = tuple(np.full(p.px.shape, float(k + 2)) for k in range(4))
    got = PS.rotate_stress(old[:3], old[3], τxx, τyy, τxy, ωxy, p, 0.7, method)
    xx, yy = PS.centroid2particle(old[0], τxx, p), PS.centroid2particle(old[1], τyy, p)
    xy, w = PT.grid2particle(τxy, p), PT.grid2particle(ωxy, p)
    assert xx[1, 1, 0] == 2.0 and yy[1, 1, 0] == 3.0 and np.isnan(xy[1, 1, 0]) and np.isnan(w[1, 1, 0])
    want = PS.rotate((xx, yy, xy), w, p, 0.7, method) + (w,)
    assert all(np.array_equal(g, v, equal_nan=True) for g, v in zip(got, want))
    assert all(np.isnan(g[1, 1, 0]) for g in got) and sum(int(np.isnan(g).sum()) for g in got) == 4
    assert all(np.all(g[p.active == 0] == 0.0) for g in got)


# ---------------------------------------------------------------------------------------------- the static side
def test_the_header_declares_the_entry_points_and_the_julia_extension_calls_them():
    protos, calls = c_prototypes(), julia_ccalls()
    for fn in ENTRY_POINTS:
        assert fn in protos and fn in calls, fn
        for ret, args in calls[fn]:
            assert ret == "Cint" and len(args) == len(protos[fn]) and all(same_arg(w, g) for w, g in zip(protos[fn], args)), (fn, protos[fn], args)
    assert protos["jrx_particles2d_stress2grid"] == ["Ptr{Cvoid}", "Ptr{Ptr{Float64}}", "Ptr{Ptr{Float64}}", "Ref{JrxParticles2d}"]
    txt = HEADER.read_text()
    sec = txt[txt.index("2D marker-in-cell particles"):]
    for s in ("6. centroid2particle!", "7. particle2centroid!", "8. rotate_stress_particles!", "particles_stress_fused", "stress_rotation_particles.jl:92-99,224-235"):
        assert s in sec, s
    assert "the five jrx_particles2d_*" not in txt
    assert '"particles_stress_fused"' in (ROOT / "include" / "jrx_tuning.h").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    assert all(fn in integ for fn in ENTRY_POINTS)
    assert "rotate_point.hpp" in (ROOT / "justrelax.jl_amd" / "csrc" / "stress_rotation.hip").read_text()
    assert "rotate_point.hpp" in (ROOT / "justrelax.jl_amd" / "csrc" / "particles.hip").read_text()


def test_the_library_exports_the_entry_points(jr):
    from justrelax_jl_amd import _lib
    L = _lib.load(check_symbols=True)
    for fn in ENTRY_POINTS:
        assert fn in _lib.declared_symbols() and hasattr(L, fn), fn
    assert L.jrx_particles2d_stress2grid(None, None, None, None) == 4          # a NULL handle is refused before anything is read


def test_the_python_layer_checks_shapes_dimension_and_device_before_the_library(jr):
    ni, B = (6, 5), jr.CPUBackend
    p = jr.init_particles(B, 4, 8, 1, _xvi(ni), ni)
    pxx, pyy, pxy, pw = jr.init_cell_arrays(p, 4)
    st = jr.StokesArrays(B, ni)
    C_, V_ = jr.fzeros(ni, p.device), jr.fzeros((7, 6), p.device)
    with pytest.raises(ValueError, match="centre field"):
        jr.centroid2particle_(pxx, V_, p)
    with pytest.raises(ValueError, match="centre field"):
        jr.particle2centroid_(V_, pxx, p)
    with pytest.raises(ValueError, match="init_cell_arrays"):
        jr.centroid2particle_(C_, C_, p)
    with pytest.raises(ValueError, match="nx >= 2"):
        q = jr.init_particles(B, 4, 8, 1, _xvi((1, 5)), (1, 5))
        jr.centroid2particle_(jr.init_cell_arrays(q, 1)[0], jr.fzeros((1, 5), p.device), q)
    with pytest.raises(ValueError, match="init_cell_arrays"):
        jr.rotate_stress_particles_((pxx, pyy, V_), (pw,), p, 0.1)
    with pytest.raises(NotImplementedError, match="2D"):
        jr.rotate_stress_particles_((pxx, pyy, pxy, pxy, pxy, pxy), (pw, pw, pw), p, 0.1)
    with pytest.raises(ValueError, match="unknown method"):
        jr.rotate_stress_particles_((pxx, pyy, pxy), (pw,), p, 0.1, method="euler")
    with pytest.raises(ValueError, match="unknown method"):
        jr.rotate_stress_(pxx, pyy, pxy, pw, st, p, 0.1, method="euler")
    with pytest.raises(ValueError, match="cells"):
        jr.stress2grid_(jr.StokesArrays(B, (5, 5)), pxx, pyy, pxy, p)
    with pytest.raises(ValueError, match="cells"):
        jr.rotate_stress_(pxx, pyy, pxy, pw, jr.StokesArrays(B, (5, 5)), p, 0.1)
    with pytest.raises(NotImplementedError, match="3D"):
        jr.stress2grid_(jr.StokesArrays(B, (6, 5, 3)), pxx, pyy, pxy, p)
    with pytest.raises(NotImplementedError, match="3D"):
        jr.rotate_stress_(pxx, pyy, pxy, pw, jr.StokesArrays(B, (6, 5, 3)), p, 0.1)
    with pytest.raises(TypeError, match="particle form"):
        jr.rotate_stress_(pxx, pyy, pxy, pw, st, p)
    with pytest.raises(TypeError, match="StokesArrays"):
        jr.stress2grid_(p, pxx, pyy, pxy, p)
    # ... and CPU arrays are refused with the text every operator uses: there is no CPU path
    for call in (lambda: jr.centroid2particle_(pxx, C_, p), lambda: jr.particle2centroid_(C_, pxx, p),
                 lambda: jr.rotate_stress_particles_((pxx, pyy, pxy), (pw,), p, 0.1), lambda: jr.rotate_stress_particles_((pxx, pyy, pxy), pw, p, 0.1, method=":jaumann"),
                 lambda: jr.rotate_stress_(pxx, pyy, pxy, pw, st, p, 0.1), lambda: jr.stress2grid_(st, pxx, pyy, pxy, p)):
        with pytest.raises(NotImplementedError, match="CPU arrays"):
            call()
    # the grid form of rotate_stress_ is still reached with a StokesArrays first, with its own refusals
    with pytest.raises(NotImplementedError, match="CPU arrays"):
        jr.rotate_stress_(st, (DX, DY), 0.1)
    with pytest.raises(TypeError, match="grid form"):
        jr.rotate_stress_(st, (DX, DY), 0.1, pw)
    # what stays refused
    for name in ("inject_particles_phase_", "MarkerChain", "StressParticles"):
        with pytest.raises(NotImplementedError, match="not built"):
            getattr(jr, name)()
    assert float(pxx.abs().max()) == 0.0 and float(st.τ_o.xx.abs().max()) == 0.0
