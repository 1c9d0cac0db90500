"""The definitions of the 3D free-surface operators (compute_rock_fraction!, advect_topography!, update_phases_given_topography! on 3D grids; include/jrx.h)
checked on their NumPy restatement alone (tests/_topography3d.py), before any device run: against the same formulas in exact rational arithmetic, against the
2D restatement on plane-strain surfaces (both ways round), exact values, monotonicity, the closed-form advection cases and the rules of the phase correction.
dz = 2^-3 and power-of-two time steps, so that the exact cases are exact."""
from fractions import Fraction

import numpy as np
import pytest

import _topography as TP2
import _topography3d as TP

D = 2.0 ** -3
_D = 8.0
Z0 = -0.5
# the largest |float64 restatement - exact rational value of the same formulas| found by test_the_restatement_agrees_with_exact_rational_arithmetic over its
# 60 surfaces on (2, 2, 2) (random, on faces and half-cells, nearly flat, steep), per member: center 2.1e-16, vertex 3.9e-16, Vx 1.7e-16, Vy 1.7e-16, Vz 1.3e-16,
# yz 2.3e-16, xz 2.6e-16, xy 3.0e-16.  The bound is four times the largest of them.
EXACT_MEASURED = 3.9e-16
EXACT_BOUND = 4 * EXACT_MEASURED
# the largest |3D member - its 2D partner| found by test_a_plane_strain_surface_reproduces_the_2d_operator over its surfaces (random, and random with nearly
# flat segments, end heights 2^-20 cells apart, where the 2D form (Φ(gb) - Φ(ga)) / (gb - ga) cancels): 1.73e-10, the same in both orientations; the 3D form
# itself is good to EXACT_MEASURED, so the difference is the 2D form's own error.  The bound is four times that.
LIFT_MEASURED = 1.73e-10
LIFT_BOUND = 4 * LIFT_MEASURED


def _h_from_s(s, T=np.float64):
    """heights whose cell-unit value is s: exact for the dyadic s used in the exact cases"""
    return T(Z0) + np.asarray(s, dtype=T) * T(D)


# ---------------------------------------------------------------------------------------------- 1. exact rational arithmetic
def _psi_x(a, b, c):
    if c <= 0:
        return Fraction(0)
    if a >= 0:
        return (a + b + c) / 3
    if b <= 0:
        return c * c * c / (3 * (c - a) * (c - b))
    return (a + b + c) / 3 + (-a) ** 3 / (3 * (b - a) * (c - a))


def _tri_x(g1, g2, g3, H):
    a, b, c = sorted((g1, g2, g3))
    if a >= H:
        return H
    if c <= 0:
        return Fraction(0)
    return _psi_x(a, b, c) - _psi_x(a - H, b - H, c - H)


def _quad_x(A, X, Y, c, b, H):
    mx, my = (A + X) / 2, (A + Y) / 2
    return (_tri_x(A - b, mx - b, c - b, H) + _tri_x(A - b, my - b, c - b, H)) / 8


def _member_exact(s, ni, name):
    """the member `name` by the text of include/jrx.h in exact rational arithmetic, from the float64 cell-unit heights s"""
    nx, ny, nz = ni
    S = [[Fraction(float(s[i, j])) for j in range(ny + 1)] for i in range(nx + 1)]
    Cc = [[(S[i][j] + S[i + 1][j] + S[i][j + 1] + S[i + 1][j + 1]) / 4 for j in range(ny)] for i in range(nx)]
    foot, rows = TP.MEMBER_DEF[name]
    out = np.empty(TP.member_shape(name, ni), dtype=object)
    for (i, j, k), _ in np.ndenumerate(out):
        if rows == "cell":
            b, H = Fraction(k), Fraction(1)
        else:
            b = max(Fraction(k) - Fraction(1, 2), Fraction(0))
            H = min(Fraction(k) + Fraction(1, 2), Fraction(nz)) - b
        total, count = Fraction(0), 0
        for oi, oj, dx, dy in TP.FOOTPRINTS[foot]:
            vi, vj = i + oi, j + oj
            ci, cj = vi - (dx < 0), vj - (dy < 0)
            if not (0 <= ci < nx and 0 <= cj < ny):
                continue
            total += _quad_x(S[vi][vj], S[vi + dx][vj], S[vi][vj + dy], Cc[ci][cj], b, H)
            count += 1
        out[i, j, k] = min(max(total / (Fraction(count, 4) * H), Fraction(0)), Fraction(1))
    return out


def _exact_surfaces():
    rng = np.random.default_rng(20261020)
    for q in range(60):
        s = rng.uniform(-0.5, 2.5, (3, 3))
        if q % 4 == 1:
            s = np.round(s * 4) / 4              # vertices on faces and half-cells, equal neighbours
        elif q % 4 == 2:
            s = 1.0 + (s - 1.0) * 2.0 ** -8      # nearly flat, close to a face
        elif q % 4 == 3:
            s = s * 3.0 - 2.0                    # steep, partly outside the box
        yield s


def test_the_restatement_agrees_with_exact_rational_arithmetic():
    ni = (2, 2, 2)
    worst = dict.fromkeys(TP.MEMBERS, 0.0)
    for s in _exact_surfaces():
        got = TP.compute_rock_fraction(s, ni, 0.0, 1.0)
        for name in TP.MEMBERS:
            want = _member_exact(s, ni, name)
            for idx, w in np.ndenumerate(want):
                worst[name] = max(worst[name], abs(float(Fraction(float(got[name][idx])) - w)))
    print("largest |restatement - exact| per member:", {k: f"{v:.2e}" for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= EXACT_BOUND, (name, v)
    assert max(worst.values()) > 0.0


def test_the_unclamped_centre_sum_stays_within_the_rounding_of_one():
    """the final clamp is a guarantee: on cells nearly covered (corners barely below the top) the sum before it stays within the rounding bound of 1"""
    rng = np.random.default_rng(5)
    T = np.float64
    over = 0.0
    for _ in range(200):
        s = 1.0 - rng.uniform(0.0, 1.0, (2, 2)) * 2.0 ** -rng.integers(1, 30, (2, 2))
        c = TP.cell_centres(s)
        tot = np.zeros(())
        for oi, oj, dx, dy in TP.FOOTPRINTS["cell"]:
            tot = tot + TP.quadrant(s[oi, oj], s[oi + dx, oj], s[oi, oj + dy], c[0, 0], T(0), T(1))
        over = max(over, float(tot) - 1.0)
    print("largest unclamped centre sum - 1:", over)
    assert over <= EXACT_BOUND


# ---------------------------------------------------------------------------------------------- 2. plane strain
def _plane_surfaces(nx, nz):
    rng = np.random.default_rng(77)
    for q in range(12):
        s = rng.uniform(-1.0, nz + 1.0, nx + 1)
        if q % 3 == 1:
            s[1::2] = s[0:-1:2][: len(s[1::2])] + rng.uniform(-1, 1, len(s[1::2])) * 2.0 ** -20          # nearly flat segments
        elif q % 3 == 2:
            s = np.round(s * 2) / 2
        yield s


PARTNERS_2D = dict(center="center", Vx="Vx", Vz="Vy", xz="vertex")               # 3D member -> the 2D member it lifts (surface constant along y)
TWINS = dict(Vy="center", yz="Vz", xy="Vx", vertex="xz")                         # the y-face / vertex-footprint member -> its cell / x-face partner
SWAP = dict(center="center", vertex="vertex", Vx="Vy", Vy="Vx", Vz="Vz", yz="xz", xz="yz", xy="xy")      # the member that holds the same volumes after x <-> y


@pytest.mark.parametrize("along", ["y", "x"])
def test_a_plane_strain_surface_reproduces_the_2d_operator(along):
    nx, nz, nt = 7, 4, 3
    worst = 0.0
    for s1 in _plane_surfaces(nx, nz):
        h1 = _h_from_s(s1)
        two = TP2.compute_rock_fraction(h1, (nx, nz), Z0, _D)
        if along == "y":
            ϕ = TP.compute_rock_fraction(np.repeat(h1[:, None], nt + 1, axis=1), (nx, nt, nz), Z0, _D)
        else:       # the same surface constant along x: every member is the transpose of its x <-> y partner, bit for bit
            ϕt = TP.compute_rock_fraction(np.repeat(h1[None, :], nt + 1, axis=0), (nt, nx, nz), Z0, _D)
            ϕ = {SWAP[k]: np.swapaxes(v, 0, 1) for k, v in ϕt.items()}
        for k3, k2 in PARTNERS_2D.items():
            for j in range(ϕ[k3].shape[1]):
                worst = max(worst, float(np.abs(ϕ[k3][:, j, :] - two[k2]).max()))
                assert np.array_equal(ϕ[k3][:, j, :], ϕ[k3][:, 0, :]), (k3, j)
        for k, partner in TWINS.items():
            # y-face against cell, interior rows: the same quadrant volumes added in the same order ((q1 + q2) + q1) + q2, so the same bits.  On the two
            # boundary rows half the footprint is missing, (q1 + q2) / 0.5, and the vertex footprint adds the same four volumes as the x-face in another
            # order, ((q5 + q1) + q5) + q1 against ((q5 + q5) + q1) + q1: those are equal to the rounding of the sum (and so is every pair after x <-> y,
            # which reorders the sums of the face footprints)
            for j in range(ϕ[k].shape[1]):
                if along == "y" and k in ("Vy", "yz") and 0 < j < nt:
                    assert np.array_equal(ϕ[k][:, j, :], ϕ[partner][:, 0, :]), (k, j)
                else:
                    assert np.abs(ϕ[k][:, j, :] - ϕ[partner][:, 0, :]).max() <= EXACT_BOUND, (k, j)
    print(f"largest |3D - 2D| on plane-strain surfaces along {along}:", worst)
    assert worst <= LIFT_BOUND


def test_transposing_a_general_surface_transposes_the_members_to_the_rounding_of_the_centre():
    """x <-> y exchanges the two addends of every quadrant (the same bits) and the pairing inside the centre value (one rounding)"""
    rng = np.random.default_rng(3)
    ni = (4, 3, 3)
    s = rng.uniform(-0.5, 3.5, (5, 4))
    a = TP.compute_rock_fraction(s, ni, 0.0, 1.0)
    b = TP.compute_rock_fraction(np.ascontiguousarray(s.T), (3, 4, 3), 0.0, 1.0)
    for k in TP.MEMBERS:
        assert np.abs(a[k] - np.swapaxes(b[SWAP[k]], 0, 1)).max() <= EXACT_BOUND, k


# ---------------------------------------------------------------------------------------------- 3. exact values
NI = (5, 4, 6)


def test_flat_surfaces_give_exact_fractions():
    nx, ny, nz = NI
    K = 3
    ϕ = TP.compute_rock_fraction(_h_from_s(np.full((nx + 1, ny + 1), float(K))), NI, Z0, _D)
    for k in TP.MEMBERS:
        assert ϕ[k].shape == TP.member_shape(k, NI)
        if TP.MEMBER_DEF[k][1] == "cell":
            assert np.all(ϕ[k][:, :, :K] == 1.0) and np.all(ϕ[k][:, :, K:] == 0.0), k
        else:
            assert np.all(ϕ[k][:, :, :K] == 1.0) and np.all(ϕ[k][:, :, K] == 0.5) and np.all(ϕ[k][:, :, K + 1:] == 0.0), k
    ϕ = TP.compute_rock_fraction(_h_from_s(np.full((nx + 1, ny + 1), K + 0.5)), NI, Z0, _D)
    for k in TP.MEMBERS:
        if TP.MEMBER_DEF[k][1] == "cell":
            assert np.all(ϕ[k][:, :, K] == 0.5) and np.all(ϕ[k][:, :, :K] == 1.0) and np.all(ϕ[k][:, :, K + 1:] == 0.0), k
        else:
            assert np.all(ϕ[k][:, :, :K + 1] == 1.0) and np.all(ϕ[k][:, :, K + 1:] == 0.0), k


def test_flat_face_surface_gives_the_members_of_update_rock_ratio():
    """binary phase fields with the air above a face-aligned flat surface, (6, 5, 4): update_phase_ratios_3D! + update_rock_ratio! interpolate the ratios to 1, 0
    and 0.5 in the face's vertex row -- the volume fractions of this operator; measured difference 0 in all eight members (what the GPU pipeline test relies on)"""
    import _phase_ratios as PR
    import _variational_stokes as VS
    ni = (6, 5, 4)
    li = tuple(n / 32.0 for n in ni)
    xci, xvi = PR.uniform_grid(ni, li)
    dz = li[2] / ni[2]
    ϕ = TP.compute_rock_fraction(np.full((7, 6), 3.0 * dz), ni, 0.0, 1.0 / dz)
    f = ϕ["center"]
    phi = VS.rock_ratio(ni)
    VS.update_rock_ratio(phi, PR.update_phase_ratios([f, 1.0 - f], xci, xvi), 2)
    diff = {k: float(np.abs(phi[k] - ϕ[k]).max()) for k in TP.MEMBERS}
    print("largest |update_rock_ratio! - compute_rock_fraction!| per member:", diff)
    assert np.array_equal(phi["center"], f)
    assert all(v == 0.0 for v in diff.values()), diff


@pytest.mark.parametrize("slopes", [(0.3, 0.0), (0.0, -0.4), (0.25, 0.35), (-0.31, 0.17)])
def test_a_tilted_plane_inside_the_box_fills_its_volume(slopes):
    """Σ center = nx ny x the mean height in cell units (the four triangles of a cell reproduce a plane), within the bound of the exact check times the number
    of cells: every cell's value carries at most EXACT_MEASURED, and the bound is four times that"""
    nx, ny, nz = NI
    I, J = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    s = 3.0 + slopes[0] * (I - nx / 2) + slopes[1] * (J - ny / 2)
    assert s.min() > 0 and s.max() < nz
    ϕ = TP.compute_rock_fraction(s, NI, 0.0, 1.0)
    mean = float(np.mean([Fraction(float(TP.cell_centres(s)[i, j])) for i in range(nx) for j in range(ny)]))
    total = float(ϕ["center"].astype(np.longdouble).sum())
    print("Σ center - nx ny mean:", total - nx * ny * mean)
    assert abs(total - nx * ny * mean) <= EXACT_BOUND * nx * ny * nz


def test_the_saddle_is_not_on_a_plane_through_three_corners():
    """s = x y on one cell: the centre value is 0.25, neither diagonal's 0 or 0.5; the volume below the four triangles is 0.25 exactly"""
    s = np.array([[0.0, 0.0], [0.0, 1.0]])
    ϕ = TP.compute_rock_fraction(s, (1, 1, 1), 0.0, 1.0)
    assert TP.cell_centres(s)[0, 0] == 0.25
    assert abs(ϕ["center"][0, 0, 0] - 0.25) <= EXACT_BOUND


@pytest.mark.parametrize("seed", [1, 2])
def test_every_value_lies_in_the_unit_interval_and_rises_with_the_surface(seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = NI
    s = rng.uniform(-1.0, nz + 1.0, (nx + 1, ny + 1))
    if seed == 2:
        s = np.round(s * 2) / 2
    lower = TP.compute_rock_fraction(s, NI, 0.0, 1.0)
    for lift in (2.0 ** -30, 0.125, 0.75):
        upper = TP.compute_rock_fraction(s + lift, NI, 0.0, 1.0)
        for k in TP.MEMBERS:
            assert lower[k].min() >= 0.0 and lower[k].max() <= 1.0, k
            # raising every height never lowers a value
            assert (upper[k] - lower[k]).min() >= 0.0, (k, lift, float((upper[k] - lower[k]).min()))
    assert 0.0 < lower["center"].mean() < 1.0


# ---------------------------------------------------------------------------------------------- 4. advection
def _ghosted(ni, fill):
    nx, ny, nz = ni
    return (np.full((nx + 1, ny + 2, nz + 2), fill[0]), np.full((nx + 2, ny + 1, nz + 2), fill[1]), np.full((nx + 2, ny + 2, nz + 1), fill[2]))


def test_zero_velocity_leaves_the_heights_bit_identical():
    rng = np.random.default_rng(4)
    nx, ny, nz = NI
    h = _h_from_s(rng.uniform(-1, nz + 1, (nx + 1, ny + 1)))
    assert np.array_equal(TP.advect_topography(h, *_ghosted(NI, (0.0, 0.0, 0.0)), NI, Z0, _D, _D, _D, 0.37), h)


def test_a_uniform_velocity_translates_a_plane():
    nx, ny, nz = NI
    α, β, dt, v = 0.25, -0.5, 2.0 ** -4, (1.0, 0.5, 0.75)
    x, y = np.meshgrid(np.arange(nx + 1) * D, np.arange(ny + 1) * D, indexing="ij")
    h = Z0 + 3.0 * D + α * x + β * y
    new = TP.advect_topography(h, *_ghosted(NI, v), NI, Z0, _D, _D, _D, dt)
    want = dt * (v[2] - α * v[0] - β * v[1])
    inner = (slice(1, None), slice(1, None))           # vx > 0 takes from the left, vy > 0 from below: the departure points of i = 0 and of j = 0 are clamped
    assert np.abs((new - h)[inner] - want).max() <= 8 * np.finfo(float).eps * np.abs(h).max()
    # a departure point outside the domain takes the edge value: a step longer than the box
    far = TP.advect_topography(h, *_ghosted(NI, (1.0, 0.0, 0.0)), NI, Z0, _D, _D, _D, 64.0)
    assert np.array_equal(far, np.repeat(h[:1, :], nx + 1, axis=0))
    far = TP.advect_topography(h, *_ghosted(NI, (0.0, -1.0, 0.0)), NI, Z0, _D, _D, _D, 64.0)
    assert np.array_equal(far, np.repeat(h[:, -1:], ny + 1, axis=1))


def test_plane_strain_advection_reproduces_the_2d_restatement_bit_for_bit():
    nx, nt, nz = 9, 3, 5
    rng = np.random.default_rng(6)
    dt = 2.0 ** -4
    for scale in (0.5, 3.0):
        h1 = _h_from_s(rng.uniform(-1, nz + 1, nx + 1))
        Vx2 = rng.uniform(-scale, scale, (nx + 1, nz + 2)) * D / dt
        Vy2 = rng.uniform(-scale, scale, (nx + 2, nz + 1)) * D / dt
        want = TP2.advect_topography(h1, Vx2, Vy2, (nx, nz), Z0, _D, _D, dt)
        # constant along y
        ni = (nx, nt, nz)
        V = (np.repeat(Vx2[:, None, :], nt + 2, axis=1), np.zeros((nx + 2, nt + 1, nz + 2)), np.repeat(Vy2[:, None, :], nt + 2, axis=1))
        got = TP.advect_topography(np.repeat(h1[:, None], nt + 1, axis=1), *V, ni, Z0, _D, _D, _D, dt)
        for j in range(nt + 1):
            assert np.array_equal(got[:, j], want), j
        # constant along x
        ni = (nt, nx, nz)
        V = (np.zeros((nt + 1, nx + 2, nz + 2)), np.repeat(Vx2[None, :, :], nt + 2, axis=0), np.repeat(Vy2[None, :, :], nt + 2, axis=0))
        got = TP.advect_topography(np.repeat(h1[None, :], nt + 1, axis=0), *V, ni, Z0, _D, _D, _D, dt)
        for i in range(nt + 1):
            assert np.array_equal(got[i, :], want), i


# ---------------------------------------------------------------------------------------------- 5. phase correction
def _fields2(ni2, N, air, f, seed):
    rng = np.random.default_rng(seed)
    c = [np.asfortranarray(rng.uniform(0.0, 1.0, ni2)) for _ in range(N)]
    norock = rng.uniform(size=ni2) < 0.3
    for k in range(N):
        if k != air - 1:
            c[k][norock] = 0.0
    keep = rng.uniform(size=ni2) < 0.33
    c[air - 1] = np.asfortranarray(np.where(keep, 1.0 - f, c[air - 1]))
    return c


@pytest.mark.parametrize("N,air", [(1, 1), (2, 2), (3, 1), (4, 3)])
def test_plane_strain_phase_correction_reproduces_the_2d_restatement_bit_for_bit(N, air):
    """f comes from two different centre formulas, so the surfaces are those on which the two centres are bit-equal -- flats on faces and at half-cells,
    inside, below and above the box -- and that equality is asserted first"""
    nx, nt, nz = 6, 3, 5
    for level in (2.0, 3.5, 0.0, 5.0, -1.0, 7.0):
        h1 = _h_from_s(np.full(nx + 1, level))
        f2 = TP2.compute_rock_fraction(h1, (nx, nz), Z0, _D)["center"]
        h3 = np.repeat(h1[:, None], nt + 1, axis=1)
        f3 = TP.compute_rock_fraction(h3, (nx, nt, nz), Z0, _D, members=("center",))["center"]
        for j in range(nt):
            assert np.array_equal(f3[:, j, :], f2)
        c2 = _fields2((nx, nz), N, air, f2, 11 + N)
        want, wr2 = TP2.update_phases_given_topography(c2, h1, (nx, nz), Z0, _D, air)
        c3 = [np.asfortranarray(np.repeat(a[:, None, :], nt, axis=1)) for a in c2]
        got, wr3 = TP.update_phases_given_topography(c3, h3, (nx, nt, nz), Z0, _D, air)
        for k in range(N):
            for j in range(nt):
                assert np.array_equal(got[k][:, j, :], want[k]), (k, j)
        assert np.array_equal(wr3[:, 1, :], wr2)


def test_a_consistent_state_is_left_untouched():
    rng = np.random.default_rng(8)
    ni = (4, 3, 5)
    nx, ny, nz = ni
    h = _h_from_s(rng.uniform(0.5, nz - 0.5, (nx + 1, ny + 1)))
    f = TP.compute_rock_fraction(h, ni, Z0, _D, members=("center",))["center"]
    share = rng.uniform(0.2, 0.8, ni)
    c = [np.asfortranarray(f * share), np.asfortranarray(1.0 - f), np.asfortranarray(f * (1.0 - share))]
    got, wr = TP.update_phases_given_topography(c, h, ni, Z0, _D, 2)
    assert not wr.any()
    for a, b in zip(got, c):
        assert np.array_equal(a, b)
    # and an inconsistent one is rewritten: all air below the surface becomes the lowest non-air index, rock above it becomes air
    c = [np.zeros(ni, order="F"), np.ones(ni, order="F"), np.zeros(ni, order="F")]
    got, wr = TP.update_phases_given_topography(c, h, ni, Z0, _D, 2)
    assert np.array_equal(got[0], f) and np.array_equal(got[1], 1.0 - f) and np.all(got[2] == 0.0)
    assert np.array_equal(wr, f > 0.0)
