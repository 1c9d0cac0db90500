"""The definitions of the 2D free-surface operators (compute_rock_fraction!, advect_topography!, update_phases_given_topography!; include/jrx.h) checked on
their NumPy restatement alone (tests/_topography.py), before any device run: exact fractions for flat surfaces, the area identity, the range, the flat branch,
the closed-form advection cases and the rules of the phase correction.  dx = dy = 2^-3 and power-of-two time steps, so that the exact cases are exact."""
import numpy as np
import pytest

import _phase_ratios as PR
import _topography as TP
import _variational_stokes as VS

DY = 2.0 ** -3
_DY = 8.0
Y0 = -0.5
NI = (12, 9)
LD = np.longdouble


def _h_from_s(s, T=np.float64):
    """heights whose cell-unit value is s: exact for the dyadic s used in the exact cases"""
    return T(Y0) + np.asarray(s, dtype=T) * T(DY)


def _random_s(seed, ni=NI, lo=0.0, hi=None):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, ni[1] if hi is None else hi, ni[0] + 1)


def _weights(ni, T):
    """W H of every member's control volume (cell units)"""
    nx, ny = ni
    b, H = TP.vertex_rows(ny, T)
    W = np.where((np.arange(nx + 1) > 0) & (np.arange(nx + 1) < nx), T(1), T(0.5))
    one = np.ones((), dtype=T)
    return dict(center=one, Vy=H[None, :] * one, Vx=W[:, None] * one, vertex=W[:, None] * H[None, :])


# ---------------------------------------------------------------------------------------------- 1. rock fractions
def test_flat_surface_on_a_face_gives_exact_fractions():
    nx, ny = NI
    J = 3
    ϕ = TP.compute_rock_fraction(_h_from_s(np.full(nx + 1, float(J))), NI, Y0, _DY)
    for k in ("center", "Vx"):
        assert np.array_equal(ϕ[k][:, :J], np.ones_like(ϕ[k][:, :J])) and np.array_equal(ϕ[k][:, J:], np.zeros_like(ϕ[k][:, J:])), k
    for k in ("Vy", "vertex"):
        assert np.all(ϕ[k][:, J] == 0.5), k
        assert np.all(ϕ[k][:, :J] == 1.0) and np.all(ϕ[k][:, J + 1:] == 0.0), k
    for k in TP.MEMBERS:
        assert ϕ[k].shape == TP.member_shape(k, NI)


def test_flat_surface_at_mid_cell_gives_exactly_one_half():
    nx, ny = NI
    ϕ = TP.compute_rock_fraction(_h_from_s(np.full(nx + 1, 3.5)), NI, Y0, _DY)
    assert np.all(ϕ["center"][:, 3] == 0.5) and np.all(ϕ["center"][:, :3] == 1.0) and np.all(ϕ["center"][:, 4:] == 0.0)
    assert np.all(ϕ["Vx"][:, 3] == 0.5)
    assert np.all(ϕ["Vy"][:, 3] == 1.0) and np.all(ϕ["Vy"][:, 4] == 0.0)          # the Vy volume of row 3 spans 2.5 .. 3.5, that of row 4 3.5 .. 4.5


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_fractions_sum_to_the_area_below_the_surface(seed):
    """With 0 <= s <= ny the volumes of every member tile the domain, so Σ value W H = Σ m[i].  The bound is 16 x the restatement's own rounding spread: the
    per-entry differences between its float64 and longdouble evaluations, weighted and summed, plus the same difference of Σ m (all sums taken in longdouble,
    so that the summation itself adds nothing)."""
    s = _random_s(seed)
    if seed == 3:
        s[::3] = np.round(s[::3])          # some vertices on faces
    out = {}
    for T in (np.float64, LD):
        h = _h_from_s(s, T)
        sc = TP.cell_heights(h, Y0, _DY)
        out[T] = (TP.compute_rock_fraction(h, NI, Y0, _DY), (T(0.5) * (sc[:-1] + sc[1:])))
    (ϕ64, m64), (ϕL, mL) = out[np.float64], out[LD]
    assert ϕ64["center"].dtype == np.float64 and ϕL["center"].dtype == LD
    M = m64.astype(LD).sum()
    wt = _weights(NI, LD)
    for k in TP.MEMBERS:
        S = (ϕ64[k].astype(LD) * wt[k]).sum()
        spread = (np.abs(ϕ64[k].astype(LD) - ϕL[k]) * wt[k]).sum() + abs(M - mL.sum())
        print(f"{k}: Σ value W H - Σ m = {float(S - M):.3e}, spread {float(spread):.3e}")
        assert abs(S - M) <= 16 * spread, k


def _surfaces(ni):
    nx, ny = ni
    x = np.arange(nx + 1) / nx
    yield "sine", 0.5 * ny + 2.5 * np.sin(2 * np.pi * x) + (0.5 * ny + 1.0) * (2 * x - 1)          # leaves the box at both ends
    yield "sawtooth", 0.5 * ny + np.where(np.arange(nx + 1) % 2 == 0, -1.75, 1.5)                     # slopes steeper than one cell per cell
    yield "flat", np.full(nx + 1, 2.0)
    for seed in (4, 5):
        yield f"random{seed}", _random_s(seed, ni, -3.0, ny + 3.0)


def test_every_value_lies_in_the_unit_interval():
    for ni in (NI, (3, 3), (7, 1), (1, 4)):
        for name, s in _surfaces(ni):
            ϕ = TP.compute_rock_fraction(_h_from_s(s), ni, Y0, _DY)
            for k, v in ϕ.items():
                assert np.all(np.isfinite(v)) and v.min() >= 0.0 and v.max() <= 1.0, (ni, name, k)


def test_a_surface_below_the_box_gives_zero_and_one_above_gives_one():
    nx, ny = NI
    rng = np.random.default_rng(6)
    below = TP.compute_rock_fraction(_h_from_s(-0.25 - rng.uniform(0, 3, nx + 1)), NI, Y0, _DY)
    above = TP.compute_rock_fraction(_h_from_s(ny + 0.25 + rng.uniform(0, 3, nx + 1)), NI, Y0, _DY)
    for k in TP.MEMBERS:
        assert np.all(below[k] == 0.0), k
        assert np.all(above[k] == 1.0), k


def test_a_column_with_equal_end_heights_takes_the_flat_branch():
    """the sloped form would divide 0 by 0 there"""
    nx, ny = NI
    s = _random_s(7)
    s[5] = s[4] = 2.25
    ϕ = TP.compute_rock_fraction(_h_from_s(s), NI, Y0, _DY)
    assert not np.isnan(ϕ["center"]).any() and not np.isnan(ϕ["Vy"]).any()
    assert np.array_equal(ϕ["center"][4], np.clip(2.25 - np.arange(ny), 0.0, 1.0))
    ga = gb = np.array([0.25])
    assert TP.primitive(ga, gb, 0.5, np.ones(1))[0] == 0.125


# ---------------------------------------------------------------------------------------------- 2. advection
def _velocities(ni, u, w):
    nx, ny = ni
    return np.full((nx + 1, ny + 2), float(u), order="F"), np.full((nx + 2, ny + 1), float(w), order="F")


def test_zero_velocity_returns_h_bit_for_bit():
    h = _h_from_s(_random_s(8, NI, -2.0, NI[1] + 2.0))
    Vx, Vy = _velocities(NI, 0.0, 0.0)
    assert np.array_equal(TP.advect_topography(h, Vx, Vy, NI, Y0, _DY, _DY, 2.0 ** -4), h)


def test_uniform_velocity_translates_a_linear_surface_exactly():
    nx, ny = NI
    x = np.arange(nx + 1) * DY
    h = Y0 + 2.0 * DY + 0.25 * x                          # dyadic everywhere
    dt = 2.0 ** -4
    for u in (1.0, -1.0):                                 # u dt _dx = +-0.5: departure points half a cell up / downstream
        w = 0.5
        Vx, Vy = _velocities(NI, u, w)
        got = TP.advect_topography(h, Vx, Vy, NI, Y0, _DY, _DY, dt)
        want = Y0 + 2.0 * DY + 0.25 * (x - u * dt) + w * dt
        inside = slice(1, None) if u > 0 else slice(None, -1)
        assert np.array_equal(got[inside], want[inside])
        edge = 0 if u > 0 else nx                         # ξ clamps there: the end value, lifted
        assert got[edge] == h[edge] + w * dt


def test_the_departure_point_clamps_at_both_ends():
    nx, ny = NI
    h = _h_from_s(_random_s(9))
    for u in (64.0, -64.0):                               # u dt _dx = +-32 cells: every departure point leaves the grid
        Vx, Vy = _velocities(NI, u, 0.0)
        got = TP.advect_topography(h, Vx, Vy, NI, Y0, _DY, _DY, 2.0 ** -4)
        assert np.array_equal(got, np.full(nx + 1, h[0] if u > 0 else h[nx]))


def test_the_surface_velocity_is_interpolated_along_the_vertex_column():
    nx, ny = NI
    Vx, Vy = _velocities(NI, 0.0, 0.0)
    Vy[:] = np.arange(ny + 1)[None, :]                    # vyv(i, j) = j
    s = np.full(nx + 1, 2.25)
    got = TP.advect_topography(_h_from_s(s), Vx, Vy, NI, Y0, _DY, _DY, 2.0 ** -4)
    assert np.array_equal(got, _h_from_s(s) + 2.25 * 2.0 ** -4)
    s = np.full(nx + 1, ny + 3.0)                         # above the box: the top row's velocity
    got = TP.advect_topography(_h_from_s(s), Vx, Vy, NI, Y0, _DY, _DY, 2.0 ** -4)
    assert np.array_equal(got, _h_from_s(s) + ny * 2.0 ** -4)


# ---------------------------------------------------------------------------------------------- 3. phase correction
def _layered(ni, J, mix=(0.75, 0.25)):
    """three fields (rock A, air, rock B; air_phase = 2): below row J the rocks in the proportions `mix`, air from row J on"""
    nx, ny = ni
    rock = (np.arange(ny) < J)[None, :] * np.ones((nx, 1))
    return [np.asfortranarray(mix[0] * rock), np.asfortranarray(1.0 - rock), np.asfortranarray(mix[1] * rock)]


def test_a_cell_newly_below_the_surface_inherits_the_nearest_rock_below():
    nx, ny = NI
    c = _layered(NI, 3)
    got, wr = TP.update_phases_given_topography(c, _h_from_s(np.full(nx + 1, 5.5)), NI, Y0, _DY, 2)
    assert np.array_equal(wr, np.broadcast_to((np.arange(ny) >= 3) & (np.arange(ny) <= 5), (nx, ny)))
    for j in (3, 4):
        assert np.all(got[0][:, j] == 0.75) and np.all(got[2][:, j] == 0.25) and np.all(got[1][:, j] == 0.0)
    assert np.all(got[0][:, 5] == 0.375) and np.all(got[2][:, 5] == 0.125) and np.all(got[1][:, 5] == 0.5)
    for k in range(3):
        assert np.array_equal(got[k][:, 6:], c[k][:, 6:]) and np.array_equal(got[k][:, :3], c[k][:, :3])


def test_rock_above_the_surface_becomes_air():
    nx, ny = NI
    c = _layered(NI, 6)
    got, wr = TP.update_phases_given_topography(c, _h_from_s(np.full(nx + 1, 4.0)), NI, Y0, _DY, 2)
    assert np.all(got[1][:, 4:] == 1.0) and np.all(got[0][:, 4:] == 0.0) and np.all(got[2][:, 4:] == 0.0)
    assert not wr[:, :4].any() and wr[:, 4:6].all() and not wr[:, 6:].any()


def test_an_all_air_bottom_cell_takes_the_lowest_non_air_index():
    nx, ny = NI
    for air, first in ((1, 1), (2, 0), (3, 0)):
        c = [np.zeros(NI, order="F") for _ in range(3)]
        c[air - 1][:] = 1.0
        got, wr = TP.update_phases_given_topography(c, _h_from_s(np.full(nx + 1, 2.0)), NI, Y0, _DY, air)
        assert np.all(got[first][:, :2] == 1.0) and np.all(got[air - 1][:, :2] == 0.0) and wr[:, :2].all() and not wr[:, 2:].any()
        other = ({0, 1, 2} - {first, air - 1}).pop()
        assert np.all(got[other] == 0.0)


def test_untouched_cells_keep_their_bits_and_rewritten_cells_sum_to_one():
    nx, ny = NI
    rng = np.random.default_rng(10)
    s = _random_s(11, NI, -1.0, ny + 1.0)
    h = _h_from_s(s)
    f = TP.compute_rock_fraction(h, NI, Y0, _DY)["center"]
    c = [np.asfortranarray(rng.uniform(0, 1, NI)) for _ in range(4)]
    air = 3
    keep = rng.uniform(size=NI) < 0.5
    c[air - 1] = np.asfortranarray(np.where(keep, 1.0 - f, c[air - 1]))
    got, wr = TP.update_phases_given_topography(c, h, NI, Y0, _DY, air)
    assert np.array_equal(wr, ~(c[air - 1] == 1.0 - f)) and not wr[keep].any()
    for k in range(4):
        assert np.array_equal(got[k][~wr], c[k][~wr])
    total = got[0] + got[1] + got[2] + got[3]
    # f (p_1 + p_2 + p_4) + (1 - f): each p_k = c_k / R is rounded once, their sum twice more, the product and 1 - f once each, the last two sums once each
    assert np.abs(total[wr] - 1.0).max() <= 8 * np.finfo(float).eps
    for k in range(4):
        assert np.array_equal(got[k][wr], (1.0 - f if k == air - 1 else f * (c[k] / (c[0] + c[1] + c[3])))[wr])          # R > 0 everywhere: every cell uses its own proportions


def test_a_single_air_field_is_set_to_the_air_fraction():
    nx, ny = NI
    h = _h_from_s(_random_s(12))
    got, _ = TP.update_phases_given_topography([np.zeros(NI, order="F")], h, NI, Y0, _DY, 1)
    assert np.array_equal(got[0], 1.0 - TP.compute_rock_fraction(h, NI, Y0, _DY)["center"])


# ---------------------------------------------------------------------------------------------- 4. against update_rock_ratio!
def test_center_equals_update_rock_ratio_on_binary_phases_under_a_face_aligned_surface():
    """binary phase fields with the air above a face-aligned flat surface: update_phase_ratios_2D! then update_rock_ratio! against compute_rock_fraction!.  center
    is bit-identical.  The other three members are NOT asserted: that route interpolates ratios, this one integrates areas; the largest difference is printed
    (measured: 0 for all three -- on this surface the interpolated ratio of the face row is 0.5, the area fraction of its volume; include/jrx.h records it)."""
    nx, ny = NI
    J = 4
    rock = np.asfortranarray((np.arange(ny) < J)[None, :] * np.ones((nx, 1)))
    li = (nx * DY, ny * DY)
    xci, xvi = PR.uniform_grid(NI, li, (0.0, Y0))
    pr = PR.update_phase_ratios([rock, 1.0 - rock], xci, xvi)
    ϕ = VS.rock_ratio(nx, ny)
    VS.update_rock_ratio(ϕ, pr, 2)
    got = TP.compute_rock_fraction(_h_from_s(np.full(nx + 1, float(J))), NI, Y0, _DY)
    assert np.array_equal(got["center"], ϕ["center"])
    for k in ("vertex", "Vx", "Vy"):
        print(f"{k}: largest |compute_rock_fraction - update_rock_ratio| = {np.abs(got[k] - ϕ[k]).max():.6g}")
