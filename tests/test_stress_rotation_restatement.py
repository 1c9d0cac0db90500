"""The definition of the grid-based stress rotation and advection (rotate_stress! on grids; include/jrx.h) checked on its NumPy restatement alone
(tests/_stress_rotation.py), before any device run: the rotation-matrix form against R T R', closed-form answers under rigid rotation and pure translation,
the invariants, the order of the Jaumann form, the plane-strain reduction of the 3D form to the 2D form, and the optional 2D vertex normals."""
import numpy as np
import pytest

import _stress_rotation as SR


def _maxabs(τ):
    return max(float(np.abs(a).max()) for a in τ.values())


# ---------------------------------------------------------------------------------------------- 1. the per-point rotation
def test_matrix_rotation_2d_is_R_T_Rt():
    rng = np.random.default_rng(1)
    for _ in range(50):
        xx, yy, xy = rng.uniform(-1.0, 1.0, 3)
        θ = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(θ), -np.sin(θ)], [np.sin(θ), np.cos(θ)]])
        want = SR.voigt(R @ SR.tensor((xx, yy, xy)) @ R.T)
        got = SR.rot2(xx, yy, xy, θ, "matrix")
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-15 * max(abs(xx), abs(yy), abs(xy))


def test_quarter_turn_swaps_xx_and_yy_and_negates_xy():
    xx, yy, xy = 0.7, -0.2, 0.45
    got = SR.rot2(xx, yy, xy, np.pi / 2, "matrix")
    assert np.abs(np.array(got) - np.array([yy, xx, -xy])).max() <= 1e-15 * 0.7


def test_matrix_rotation_3d_is_R_T_Rt_and_120_degrees_about_the_diagonal_permutes_the_axes():
    rng = np.random.default_rng(2)
    for _ in range(50):
        t = rng.uniform(-1.0, 1.0, 6)
        w = rng.uniform(-1.0, 1.0, 3)
        dt = rng.uniform(0.1, 2.0)
        R = SR.rotation_matrix(w, dt)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 2e-15                # each entry of R carries a few roundings of 1.1e-16, each of R R' three such products
        want = SR.voigt(R @ SR.tensor(t) @ R.T)
        got = SR.rot3(t, w, dt, "matrix")
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-15 * np.abs(t).max()
    # 120 degrees about (1, 1, 1) / sqrt 3 is the cyclic permutation e_x -> e_y -> e_z -> e_x
    P = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    w = np.ones(3) / np.sqrt(3.0)
    assert np.abs(SR.rotation_matrix(w, 2 * np.pi / 3) - P).max() <= 1e-15
    t = np.array([0.9, -0.4, 0.1, 0.3, -0.6, 0.8])                      # xx, yy, zz, yz, xz, xy
    want = SR.voigt(P @ SR.tensor(t) @ P.T)                             # signs and places derived from the permutation matrix
    assert want == (t[2], t[0], t[1], t[5], t[3], t[4])                 # the old xx is the new yy: xx -> yy -> zz -> xx and yz -> xz -> xy -> yz, all signs +
    got = SR.rot3(t, w, 2 * np.pi / 3, "matrix")
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-15 * np.abs(t).max()


# ---------------------------------------------------------------------------------------------- 2. uniform tensor under rigid rotation
def _uniform_state(ni, optional=False):
    nd = len(ni)
    vals = dict(xx=0.8, yy=-0.5, zz=-0.3, yz=0.35, xz=-0.15, xy=0.6)
    members = (SR.MEMBERS2_OPT if optional else SR.MEMBERS2) if nd == 2 else SR.MEMBERS3
    τ = {k: np.full(SR.shape_at(loc, ni), vals[k[:2]]) for k, loc in members.items()}
    return τ, vals


@pytest.mark.parametrize("ni,Ω", [((7, 5), 0.9), ((5, 3, 2), (0.3, -0.5, 0.7))])
def test_uniform_tensor_under_rigid_rotation(ni, Ω):
    nd = len(ni)
    li = (2.0, 1.0, 0.7)[:nd]
    _di = tuple(n / l for n, l in zip(ni, li))
    dt = 0.8
    V = SR.rigid_velocity(ni, li, Ω, centre=tuple(0.5 * l for l in li))
    ω = SR.vorticity(V, ni, _di)
    τ, vals = _uniform_state(ni, optional=True)
    if nd == 2:
        assert np.abs(ω - Ω).max() <= 1e-13
        R = SR.rotation_matrix((0.0, 0.0, Ω), dt)[:2, :2]
        want = dict(zip(("xx", "yy", "xy"), SR.voigt(R @ SR.tensor((vals["xx"], vals["yy"], vals["xy"])) @ R.T)))
    else:
        assert max(np.abs(ω[k] - Ω[c]).max() for c, k in enumerate(("yz", "xz", "xy"))) <= 1e-13
        R = SR.rotation_matrix(Ω, dt)
        want = dict(zip(("xx", "yy", "zz", "yz", "xz", "xy"), SR.voigt(R @ SR.tensor([vals[k] for k in ("xx", "yy", "zz", "yz", "xz", "xy")]) @ R.T)))
    one = SR.rotate_stress(τ, ω, V, ni, _di, dt, "matrix", "upwind")
    assert set(one) == set(τ)
    for k, a in one.items():                      # every node, the boundary included
        assert a.shape == τ[k].shape
        assert np.abs(a - want[k[:2]]).max() <= 1e-12 * 0.8, k
    N, cur = 8, τ
    for _ in range(N):
        cur = SR.rotate_stress(cur, ω, V, ni, _di, dt / N, "matrix", "upwind")
    for k in one:
        assert np.abs(cur[k] - one[k]).max() <= 1e-12 * 0.8, k


# ---------------------------------------------------------------------------------------------- 3. invariants
def _invariants(τ, nd):
    if nd == 2:
        return τ["xx"] + τ["yy"], 0.5 * (τ["xx"] ** 2 + τ["yy"] ** 2) + τ["xy_c"] ** 2
    return (τ["xx"] + τ["yy"] + τ["zz"],
            0.5 * (τ["xx"] ** 2 + τ["yy"] ** 2 + τ["zz"] ** 2) + τ["yz_c"] ** 2 + τ["xz_c"] ** 2 + τ["xy_c"] ** 2)


@pytest.mark.parametrize("ni", [(7, 5), (5, 3, 2)])
def test_invariants(ni):
    nd = len(ni)
    τ, ω, _ = SR.random_state(ni, 3)
    tr0, j0 = _invariants(τ, nd)
    out = SR.rotate_stress(τ, ω, None, ni, None, 0.9, "matrix", "none")
    tr, j = _invariants(out, nd)
    assert np.abs(tr - tr0).max() <= 1e-14 and np.abs(j - j0).max() <= 1e-14
    errs = []
    for dt in (1e-3, 2e-3):
        out = SR.rotate_stress(τ, ω, None, ni, None, dt, "jaumann", "none")
        tr, j = _invariants(out, nd)
        assert np.abs(tr - tr0).max() <= 1e-14
        errs.append(np.abs(j - j0))
    ratio = errs[1] / errs[0]
    assert errs[0].min() > 1e-11                                        # far above rounding, so that the ratio means something
    assert ratio.min() >= 3.5 and ratio.max() <= 4.5                    # second order in θ


# ---------------------------------------------------------------------------------------------- 4. nothing to do
@pytest.mark.parametrize("ni", [(7, 5), (5, 3, 2)])
@pytest.mark.parametrize("method", SR.METHODS)
def test_zero_vorticity_without_advection_returns_the_input_bits(ni, method):
    τ, ω, _ = SR.random_state(ni, 4, optional=True)
    ω = np.zeros_like(ω) if len(ni) == 2 else {k: np.zeros_like(a) for k, a in ω.items()}
    out = SR.rotate_stress(τ, ω, None, ni, None, 0.7, method, "none")
    assert set(out) == set(τ)
    for k in τ:
        assert np.array_equal(out[k], τ[k]), k


# ---------------------------------------------------------------------------------------------- 5. pure translation
def _translation(ni, axis, u):
    nd = len(ni)
    li = (2.0, 1.0, 0.7)[:nd]
    _di = tuple(n / l for n, l in zip(ni, li))
    V = tuple(np.full(SR.velocity_shape(c, ni), u if c == axis else 0.0) for c in range(nd))
    ω = np.zeros(SR.shape_at(SR.VERTEX2, ni)) if nd == 2 else {k: np.zeros(SR.shape_at(loc, ni)) for k, loc in SR.OMEGA3.items()}
    return li, _di, V, ω


@pytest.mark.parametrize("ni,axis", [((7, 5), 0), ((7, 5), 1), ((5, 4, 3), 0), ((5, 4, 3), 1), ((5, 4, 3), 2)])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_translation_of_a_linear_field(ni, axis, sign):
    nd = len(ni)
    u = 0.37 * sign
    li, _di, V, ω = _translation(ni, axis, u)
    coords = SR.grid_coords(ni, li)
    members = SR.MEMBERS2_OPT if nd == 2 else SR.MEMBERS3
    a0, b = 0.25, 1.5
    τ = {k: np.ascontiguousarray(np.broadcast_to(a0 * (m + 1) + b * SR.location_coords(loc, coords)[axis], SR.shape_at(loc, ni)))
         for m, (k, loc) in enumerate(members.items())}
    dt = 0.5 / (abs(u) * _di[axis])                                     # CFL 0.5
    out = SR.rotate_stress(τ, ω, V, ni, _di, dt, "matrix", "upwind")
    for k in τ:
        inflow = [slice(None)] * nd
        inflow[axis] = 0 if u > 0 else -1
        rest = [slice(None)] * nd
        rest[axis] = slice(1, None) if u > 0 else slice(None, -1)
        assert np.array_equal(out[k][tuple(inflow)], τ[k][tuple(inflow)]), k
        assert np.abs(out[k][tuple(rest)] - (τ[k][tuple(rest)] - dt * u * b)).max() <= 1e-13 * np.abs(τ[k]).max(), k


@pytest.mark.parametrize("ni,axis", [((8, 6), 0), ((8, 6), 1), ((6, 6, 6), 0), ((6, 6, 6), 1), ((6, 6, 6), 2)])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_step_profile_stays_within_its_bounds(ni, axis, sign):
    """upwind at CFL 0.5 is a convex combination of two input values; the downwind difference the reference's advection_term picks overshoots"""
    nd = len(ni)
    u = 0.37 * sign
    li, _di, V, ω = _translation(ni, axis, u)
    members = SR.MEMBERS2_OPT if nd == 2 else SR.MEMBERS3
    τ = {}
    for k, loc in members.items():
        shp = SR.shape_at(loc, ni)
        idx = np.arange(shp[axis]).reshape([-1 if d == axis else 1 for d in range(nd)])
        τ[k] = np.ascontiguousarray(np.broadcast_to(np.where(idx < shp[axis] // 2, 2.0, -1.0), shp))
    dt = 0.5 / (abs(u) * _di[axis])
    out = SR.rotate_stress(τ, ω, V, ni, _di, dt, "matrix", "upwind")
    for k in τ:
        assert out[k].min() >= -1.0 and out[k].max() <= 2.0, k
        assert not np.array_equal(out[k], τ[k]), k                      # the step did move
    v = [SR.velocity_at(V[c], c, (0,) * nd, ni) for c in range(nd)]
    downwind = -SR.upwind(τ["xx"], [-x for x in v], _di)               # v_d (v_d > 0 ? A[I + e_d] - A[I] : A[I] - A[I - e_d]) _d_d
    down = τ["xx"] - dt * downwind
    assert down.max() > 2.0 or down.min() < -1.0


# ---------------------------------------------------------------------------------------------- 6. plane strain
def _plane_strain(ni2, nz, seed, zz=0.3):
    """a z-invariant 3D state from a random 2D one: (2D state), (3D state)"""
    τ2, ω2, V2 = SR.random_state(ni2, seed)
    ni3 = ni2 + (nz,)
    rep = lambda a, n: np.ascontiguousarray(np.repeat(a[:, :, None], n, axis=2))
    τ3 = dict(xx=rep(τ2["xx"], nz), yy=rep(τ2["yy"], nz), zz=np.full(ni3, zz), yz_c=np.zeros(ni3), xz_c=np.zeros(ni3), xy_c=rep(τ2["xy_c"], nz),
              yz=np.zeros(SR.shape_at(SR.YZ, ni3)), xz=np.zeros(SR.shape_at(SR.XZ, ni3)), xy=rep(τ2["xy"], nz))
    ω3 = dict(yz=np.zeros(SR.shape_at(SR.YZ, ni3)), xz=np.zeros(SR.shape_at(SR.XZ, ni3)), xy=rep(ω2, nz))
    V3 = (rep(V2[0], nz + 2), rep(V2[1], nz + 2), np.zeros(SR.velocity_shape(2, ni3)))
    return (τ2, ω2, V2), (τ3, ω3, V3)


@pytest.mark.parametrize("method", SR.METHODS)
@pytest.mark.parametrize("advection", SR.ADVECTIONS)
def test_plane_strain_3d_equals_2d_layer_by_layer(method, advection):
    ni2, nz = (5, 3), 2
    (τ2, ω2, V2), (τ3, ω3, V3) = _plane_strain(ni2, nz, 6)
    _di = (2.5, 3.0, 2.0)
    dt = 0.1
    o2 = SR.rotate_stress2d(τ2, ω2, V2, ni2, _di[:2], dt, method, advection)
    o3 = SR.rotate_stress3d(τ3, ω3, V3, ni2 + (nz,), _di, dt, method, advection)
    for k in ("xx", "yy", "xy_c", "xy"):
        for layer in range(nz):
            assert np.abs(o3[k][:, :, layer] - o2[k]).max() <= 1e-13 * _maxabs(τ2), (k, layer)
    assert np.array_equal(o3["zz"], τ3["zz"])
    for k in ("yz", "xz", "yz_c", "xz_c"):
        assert np.all(o3[k] == 0.0), k


# ---------------------------------------------------------------------------------------------- 7. the optional 2D vertex normals
@pytest.mark.parametrize("method", SR.METHODS)
def test_optional_vertex_normals_follow_their_own_node(method):
    ni = (7, 5)
    τ, ω, V = SR.random_state(ni, 7, optional=True)
    _di, dt = (3.5, 5.0), 0.05
    out = SR.rotate_stress2d(τ, ω, None, ni, _di, dt, method, "none")
    for i in range(ni[0] + 1):
        for j in range(ni[1] + 1):
            T = SR.tensor((τ["xx_v"][i, j], τ["yy_v"][i, j], τ["xy"][i, j]))
            θ = dt * ω[i, j]
            if method == "matrix":
                R = np.array([[np.cos(θ), -np.sin(θ)], [np.sin(θ), np.cos(θ)]])
                want = R @ T @ R.T
            else:
                W = np.array([[0.0, -θ], [θ, 0.0]])
                want = T + (W @ T - T @ W)
            assert abs(out["xx_v"][i, j] - want[0, 0]) <= 1e-15 and abs(out["yy_v"][i, j] - want[1, 1]) <= 1e-15
    # with advection they move like every other vertex member, and the other members do not depend on their presence
    full = SR.rotate_stress2d(τ, ω, V, ni, _di, dt, method, "upwind")
    v = [SR.velocity_at(V[c], c, SR.VERTEX2, ni) for c in range(2)]
    for k in ("xx_v", "yy_v"):
        assert np.array_equal(full[k], out[k] - dt * SR.upwind(τ[k], v, _di)), k
    bare = SR.rotate_stress2d({k: τ[k] for k in SR.MEMBERS2}, ω, V, ni, _di, dt, method, "upwind")
    assert set(bare) == set(SR.MEMBERS2)
    for k in bare:
        assert np.array_equal(bare[k], full[k]), k


def test_unknown_kinds_are_refused():
    τ, ω, V = SR.random_state((3, 2), 8)
    with pytest.raises(ValueError):
        SR.rotate_stress2d(τ, ω, V, (3, 2), (1.0, 1.0), 0.1, "rk4", "upwind")
    with pytest.raises(ValueError):
        SR.rotate_stress2d(τ, ω, V, (3, 2), (1.0, 1.0), 0.1, "matrix", "weno")
