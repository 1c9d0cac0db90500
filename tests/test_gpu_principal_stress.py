"""GPU: principal stresses (PrincipalStress, compute_principal_stresses[_]; csrc/principal.hip through jrx_principal_stresses2d / 3d).  2D against the NumPy
restatement of the reference's closed form (tests/_principal.py; by tolerance: atan, sin, cos are not bit-identical between libraries) with its NaN cells; 3D
against numpy.linalg.eigh (eigenvalues, residuals, orthogonality, vectors under the sign convention), the reference's pinned case on every cell, the simple
shear the reference cannot split, determinism, bounds, NaN / Inf isolation, the API and the C ABI's argument errors, and a 3D Stokes time step."""
from types import SimpleNamespace

import numpy as np
import pytest

import _principal as PS

pytestmark = pytest.mark.gpu
POISON = -7.25e300


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _dn(t):
    from justrelax_jl_amd.arrays import to_numpy
    return to_numpy(t)


def _flat(t):
    """the column-major storage of a library array as a 1-D view (cell index c = i + nx (j + ny k), component fastest for the outputs)"""
    return t.permute(*range(t.dim() - 1, -1, -1)).reshape(-1)


def _field(jr, values, ni):
    import torch
    t = jr.fzeros(ni, _dev())
    _flat(t).copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)))
    return t


def _handle():
    from justrelax_jl_amd import _lib
    return _lib.Handle(_dev().index)


def _stokes(jr, comps, ni):
    """just what compute_principal_stresses_ reads: size(stokes.P) and @stress_center(stokes.τ)"""
    τ = SimpleNamespace(**{k: _field(jr, v, ni) for k, v in comps.items()})
    return SimpleNamespace(P=τ.xx, τ=τ)


# ----------------------------------------------------------------------------------------------------------------------------------------- 2D
def _inputs2d(n, rng):
    xx, yy, xy = (rng.uniform(-1.0e8, 1.0e8, n) for _ in range(3))
    p = rng.permutation(n)
    specials = [p[1::4], p[2::4], p[3::4]]          # τxx = τyy, τxy ≠ 0 (atan(±Inf)) | τxx < τyy | 0/0; p[0::4] stays random
    yy[specials[0]] = xx[specials[0]]
    lo = np.minimum(xx[specials[1]], yy[specials[1]]) - 1.0
    xx[specials[1]] = lo
    yy[specials[2]] = xx[specials[2]]
    xy[specials[2]] = 0.0
    return dict(xx=xx, yy=yy, xy_c=xy)


@pytest.mark.parametrize("ni", [(1, 1), (2, 3), (17, 19), (1025, 769), (4097, 4097)])
def test_2d_matches_the_restatement(jr, ni):
    rng = np.random.default_rng(ni[0] * 7919 + ni[1])
    n = ni[0] * ni[1]
    comps = _inputs2d(n, rng)
    st = _stokes(jr, comps, ni)
    σ = jr.PrincipalStress(jr.AMDGPUBackend, ni)
    σ.σ3.fill_(POISON)
    h = _handle()
    jr.compute_principal_stresses_(st, σ, handle=h)
    g1, g2 = (_flat(t).cpu().numpy().reshape(n, 2).T for t in (σ.σ1, σ.σ2))
    r1, r2 = PS.principal2d(comps["xx"], comps["yy"], comps["xy_c"])
    for g, r in ((g1, r1), (g2, r2)):
        assert np.array_equal(np.isnan(g), np.isnan(r))
    with np.errstate(all="ignore"):
        scale = np.maximum(np.abs(comps["xx"] + comps["yy"]) / 2 + np.sqrt((comps["xx"] - comps["yy"]) ** 2 / 2 + comps["xy_c"] ** 2), 1e-300)
    ok = ~np.isnan(r1[0])
    for g, r in ((g1, r1), (g2, r2)):
        assert np.all(np.abs(g[:, ok] - r[:, ok]) <= 1e-13 * scale[ok])
    if n >= 4:
        assert np.isnan(g1).any() and (~np.isnan(g1)).any()
    assert np.all(_dn(σ.σ3) == POISON)                      # the (2, 1, 1) placeholder is never written


# ----------------------------------------------------------------------------------------------------------------------------------------- 3D
def _rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def _tensors3d(n, rng):
    """(n, 3, 3) symmetric tensors, magnitudes 1e-3 .. 1e9, with the special cells spread over a random permutation (cell p[0] random)"""
    m = rng.standard_normal((n, 3, 3))
    A = (m + m.transpose(0, 2, 1)) / 2 * (10.0 ** rng.uniform(-3, 9, n))[:, None, None]
    p = rng.permutation(n)
    K = 9 if n < 1000 else 64                               # small grids: mostly special cells; large ones: mostly random
    for kind in range(8):
        for c in p[1 + kind::K]:
            s = 10.0 ** rng.uniform(-3, 9)
            if kind == 0:
                A[c] = 0.0
            elif kind == 1:
                A[c] = rng.choice([-1.0, 1.0]) * s * np.eye(3)
            elif kind == 2:
                q = _rot(rng)
                A[c] = q @ np.diag([s, s, -0.37 * s]) @ q.T
            elif kind == 3:
                q = _rot(rng)
                A[c] = q @ np.diag([s, s * (1 + 1e-9 * np.sqrt(2.1369)), -0.37 * s]) @ q.T
            else:
                i, j = [(0, 1), (0, 2), (1, 2), (0, 1)][kind - 4]
                A[c] = 0.0
                A[c, i, j] = A[c, j, i] = s * (1 if kind < 7 else -1)
            A[c] = (A[c] + A[c].T) / 2
    return A


def _comps(A):
    return dict(xx=A[:, 0, 0], yy=A[:, 1, 1], zz=A[:, 2, 2], yz_c=A[:, 1, 2], xz_c=A[:, 0, 2], xy_c=A[:, 0, 1])


def _run3d(jr, A, ni, h=None):
    st = _stokes(jr, _comps(A), ni)
    σ = jr.PrincipalStress(jr.AMDGPUBackend, ni)
    jr.compute_principal_stresses_(st, σ, handle=h)
    return σ


def _vectors(σ, n):
    """(n, 3 components, 3 principal stresses)"""
    return np.stack([_flat(t).cpu().numpy().reshape(n, 3) for t in (σ.σ1, σ.σ2, σ.σ3)], axis=2)


def _check3d(A, Vs):
    F = np.sqrt((A * A).sum(axis=(1, 2)))
    w, U = np.linalg.eigh(A)
    w, U = w[:, ::-1], U[:, :, ::-1]
    nv = np.linalg.norm(Vs, axis=1)
    AV = A @ Vs
    rq = np.einsum("mij,mij->mj", Vs, AV)
    lam = np.where(nv > 0, rq / np.where(nv > 0, nv * nv, 1.0), 0.0)
    assert np.all(np.isfinite(Vs))
    assert np.all(np.abs(lam - w) <= 1e-12 * F[:, None])
    assert np.all(np.abs(nv - np.abs(w)) <= 1e-12 * F[:, None])                       # ‖σ_j‖ = |λ_j|
    assert np.all(lam[:, 0] >= lam[:, 1] - 1e-12 * F) and np.all(lam[:, 1] >= lam[:, 2] - 1e-12 * F)
    res = np.linalg.norm(AV - lam[:, None, :] * Vs, axis=1)
    assert np.all(res <= 1e-12 * F[:, None] ** 2)
    G = np.einsum("mij,mik->mjk", Vs, Vs)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert np.all(np.abs(G[:, i, j]) <= 1e-12 * F ** 2)
    # vectors against eigh's where the eigenvalue is separated by ≥ 1e-6 ‖τ‖_F (and not ≈ 0, where λ e cannot give e back)
    gap = np.stack([np.minimum(np.abs(w[:, j] - w[:, (j + 1) % 3]), np.abs(w[:, j] - w[:, (j + 2) % 3])) for j in range(3)], axis=1)
    sel = (gap >= 1e-6 * F[:, None]) & (np.abs(w) >= 1e-6 * F[:, None]) & (F[:, None] > 0)
    m_idx, j_idx = np.nonzero(sel)
    e = Vs[m_idx, :, j_idx] / lam[m_idx, j_idx][:, None]
    u = U[m_idx, :, j_idx]
    au = np.sort(np.abs(u), axis=1)
    clear = au[:, 2] - au[:, 1] > 1e-9                    # a clear largest component: the sign convention decides the sign
    k = np.argmax(np.abs(u), axis=1)
    u = u * np.where(u[np.arange(len(k)), k] < 0, -1.0, 1.0)[:, None]
    d = np.linalg.norm(e - u, axis=1)
    d = np.where(clear, d, np.minimum(d, np.linalg.norm(e + u, axis=1)))
    assert np.all(d <= 1e-8), d.max()
    ke = np.argmax(np.abs(e), axis=1)
    assert np.all(e[np.arange(len(ke)), ke][clear] > 0)
    zero = F == 0
    assert np.all(Vs[zero] == 0.0)
    return int(sel.sum())


@pytest.mark.parametrize("ni", [(1, 1, 1), (2, 3, 5), (17, 19, 23), (255, 1, 3), (64, 64, 64)])
def test_3d_matches_eigh(jr, ni):
    rng = np.random.default_rng(int(np.prod(ni)) + 17)
    n = int(np.prod(ni))
    A = _tensors3d(n, rng)
    σ = _run3d(jr, A, ni)
    assert tuple(σ.σ1.shape) == tuple(σ.σ2.shape) == tuple(σ.σ3.shape) == (3,) + ni
    compared = _check3d(A, _vectors(σ, n))
    assert compared >= n // 2                             # most cells have at least one separated eigenvalue


def test_3d_256_cubed_subset_and_finite_everywhere(jr):
    import torch
    ni = (256, 256, 256)
    n = int(np.prod(ni))
    dev = _dev()
    g = torch.Generator(device=dev)
    g.manual_seed(20261016)
    mag = 10.0 ** (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 12 - 3)
    τ = SimpleNamespace()
    for k in ("xx", "yy", "zz", "yz_c", "xz_c", "xy_c"):
        t = jr.fzeros(ni, dev)
        _flat(t).copy_(torch.randn(n, generator=g, device=dev, dtype=torch.float64) * mag)
        setattr(τ, k, t)
    del mag
    σ = jr.PrincipalStress(jr.AMDGPUBackend, ni)
    jr.compute_principal_stresses_(SimpleNamespace(P=τ.xx, τ=τ), σ)
    for t in (σ.σ1, σ.σ2, σ.σ3):
        assert bool(torch.isfinite(t).all())
    idx = torch.from_numpy(np.random.default_rng(3).choice(n, 100_000, replace=False)).to(dev)
    c = {k: _flat(getattr(τ, k)).index_select(0, idx).cpu().numpy() for k in ("xx", "yy", "zz", "yz_c", "xz_c", "xy_c")}
    A = np.stack([np.stack([c["xx"], c["xy_c"], c["xz_c"]], 1), np.stack([c["xy_c"], c["yy"], c["yz_c"]], 1),
                  np.stack([c["xz_c"], c["yz_c"], c["zz"]], 1)], 1)
    Vs = np.stack([_flat(t).view(n, 3).index_select(0, idx).cpu().numpy() for t in (σ.σ1, σ.σ2, σ.σ3)], axis=2)
    _check3d(A, Vs)


def test_reference_known_answer_on_every_cell(jr):
    """test/test_types.jl:222-238 on a 33 x 17 x 9 grid: Σ ‖σ_j‖ = 6 within 1e-6, the eigenvalues 3.48702452, 1.721857, 0.79111848"""
    ni = (33, 17, 9)
    n = int(np.prod(ni))
    c = PS.REFERENCE_CASE
    T = PS.tensor3(c["xx"], c["yy"], c["zz"], c["yz"], c["xz"], c["xy"])
    A = np.broadcast_to(T, (n, 3, 3)).copy()
    Vs = _vectors(_run3d(jr, A, ni), n)
    nv = np.linalg.norm(Vs, axis=1)
    assert np.all(np.abs(nv.sum(axis=1) - 6.0) <= 1e-6)
    w = np.linalg.eigvalsh(T)[::-1]
    assert np.all(np.abs(nv - w) <= 1e-13)
    assert np.allclose(nv[0], PS.REFERENCE_EIGENVALUES, rtol=0, atol=1e-7)
    assert np.all(Vs == Vs[:1])                            # one answer on every cell
    _check3d(A, Vs)


@pytest.mark.parametrize("plane", ["xy_c", "xz_c", "yz_c"])
def test_simple_shear_is_split(jr, plane):
    """σ = (1e8, 0, −1e8) where the reference's iteration returns zeros (tests/test_principal_stress_restatement.py)"""
    ni = (5, 4, 3)
    n = int(np.prod(ni))
    comps = {k: np.zeros(n) for k in ("xx", "yy", "zz", "yz_c", "xz_c", "xy_c")}
    comps[plane][:] = 1.0e8
    st = _stokes(jr, comps, ni)
    σ = jr.compute_principal_stresses(jr.AMDGPUBackend, st)
    Vs = _vectors(σ, n)
    nv = np.linalg.norm(Vs, axis=1)
    assert np.allclose(nv[:, 0], 1.0e8, rtol=1e-14, atol=0) and np.allclose(nv[:, 2], 1.0e8, rtol=1e-14, atol=0)
    assert np.all(Vs[:, :, 1] == 0.0)
    i, j = {"xy_c": (0, 1), "xz_c": (0, 2), "yz_c": (1, 2)}[plane]
    e1 = np.zeros(3)
    e1[[i, j]] = 1 / np.sqrt(2)
    assert np.allclose(Vs[:, :, 0], 1.0e8 * e1, rtol=0, atol=1e-6)
    assert np.allclose(np.abs(Vs[:, :, 2]), 1.0e8 * e1, rtol=0, atol=1e-6)
    assert np.all(np.abs(Vs[:, :, 2] @ e1) <= 1e-6)


# ----------------------------------------------------------------------------------------------------------------------------------------- determinism, bounds, isolation
def test_two_calls_are_bit_identical(jr):
    import torch
    ni = (17, 19, 23)
    A = _tensors3d(int(np.prod(ni)), np.random.default_rng(5))
    st = _stokes(jr, _comps(A), ni)
    a, b = jr.PrincipalStress(jr.AMDGPUBackend, ni), jr.PrincipalStress(jr.AMDGPUBackend, ni)
    jr.compute_principal_stresses_(st, a)
    jr.compute_principal_stresses_(st, b)
    for k in ("σ1", "σ2", "σ3"):
        assert torch.equal(_flat(getattr(a, k)).view(torch.int64), _flat(getattr(b, k)).view(torch.int64))


def _prefix(n_out, extra, ncomp, ni):
    import torch
    buf = torch.full((n_out + extra,), POISON, dtype=torch.float64, device=_dev())
    view = buf[:n_out].view(*reversed((ncomp,) + ni)).permute(*range(len(ni), -1, -1))
    return buf, view


@pytest.mark.parametrize("ni", [(17, 19, 23), (2, 3)])
def test_no_write_past_the_end(jr, ni):
    import torch
    n = int(np.prod(ni))
    nd = len(ni)
    rng = np.random.default_rng(11)
    comps = _comps(_tensors3d(n, rng)) if nd == 3 else _inputs2d(n, rng)
    st = _stokes(jr, comps, ni)
    bufs = [_prefix(nd * n, 1031, nd, ni) for _ in range(3 if nd == 3 else 2)]
    σ3 = bufs[2][1] if nd == 3 else jr.fzeros((2, 1, 1), _dev())
    σ = SimpleNamespace(σ1=bufs[0][1], σ2=bufs[1][1], σ3=σ3)
    jr.compute_principal_stresses_(st, σ)
    ref = jr.PrincipalStress(jr.AMDGPUBackend, ni)
    jr.compute_principal_stresses_(st, ref)
    for (buf, view), k in zip(bufs, ("σ1", "σ2", "σ3")):
        assert bool((buf[nd * n:] == POISON).all())
        assert torch.equal(_flat(view).view(torch.int64), _flat(getattr(ref, k)).view(torch.int64))


def test_nan_and_inf_cells_are_isolated(jr):
    import torch
    for ni in ((17, 19, 23), (33, 29)):
        n = int(np.prod(ni))
        nd = len(ni)
        rng = np.random.default_rng(13)
        comps = _comps(_tensors3d(n, rng)) if nd == 3 else _inputs2d(n, rng)
        clean = jr.compute_principal_stresses(jr.AMDGPUBackend, _stokes(jr, comps, ni))
        bad = rng.choice(n, 6, replace=False)
        dirty = {k: v.copy() for k, v in comps.items()}
        dirty["xx"][bad[0]] = np.nan
        dirty["yy"][bad[1]] = np.inf
        dirty["xy_c"][bad[2]] = -np.inf
        dirty["xx"][bad[3]] = np.inf
        dirty["yy"][bad[3]] = -np.inf
        dirty["xy_c"][bad[4]] = np.nan
        dirty["xx"][bad[5]] = 1.0e308
        got = jr.compute_principal_stresses(jr.AMDGPUBackend, _stokes(jr, dirty, ni))
        keep = np.ones(n, dtype=bool)
        keep[bad] = False
        for k in ("σ1", "σ2") + (("σ3",) if nd == 3 else ()):
            a = _flat(getattr(clean, k)).view(torch.int64).cpu().numpy().reshape(n, nd)
            b = _flat(getattr(got, k)).view(torch.int64).cpu().numpy().reshape(n, nd)
            assert np.array_equal(a[keep], b[keep]), k


# ----------------------------------------------------------------------------------------------------------------------------------------- API and C ABI
def test_allocating_form_matches_the_in_place_call(jr):
    import torch
    for ni in ((9, 7, 5), (13, 11)):
        n = int(np.prod(ni))
        rng = np.random.default_rng(17)
        comps = _comps(_tensors3d(n, rng)) if len(ni) == 3 else _inputs2d(n, rng)
        st = _stokes(jr, comps, ni)
        a = jr.compute_principal_stresses(jr.AMDGPUBackend, st)
        b = jr.PrincipalStress(jr.AMDGPUBackend, ni)
        jr.compute_principal_stresses_(st, b)
        nd = len(ni)
        assert tuple(a.sigma1.shape) == tuple(a.sigma2.shape) == (nd,) + ni
        assert tuple(a.sigma3.shape) == ((2, 1, 1) if nd == 2 else (3,) + ni)
        for k in ("σ1", "σ2", "σ3"):
            x, y = getattr(a, k), getattr(b, k)
            assert torch.equal(_flat(x).view(torch.int64), _flat(y).view(torch.int64))


def test_shape_and_dimension_errors(jr):
    from justrelax_jl_amd import _lib
    ni3, ni2 = (6, 5, 4), (6, 5)
    st3 = jr.StokesArrays(jr.AMDGPUBackend, ni3)
    st2 = jr.StokesArrays(jr.AMDGPUBackend, ni2)
    h = _handle()
    calls = h.get_option("stat_principal_calls")
    with pytest.raises(ValueError):
        jr.compute_principal_stresses_(st3, jr.PrincipalStress(jr.AMDGPUBackend, ni2), handle=h)
    with pytest.raises(ValueError):
        jr.compute_principal_stresses_(st2, jr.PrincipalStress(jr.AMDGPUBackend, ni3), handle=h)
    with pytest.raises(ValueError):
        jr.compute_principal_stresses_(st3, jr.PrincipalStress(jr.AMDGPUBackend, (6, 5, 3)), handle=h)
    with pytest.raises(ValueError):
        jr.compute_principal_stresses_(st2, jr.PrincipalStress(jr.AMDGPUBackend, (5, 6)), handle=h)
    bad = jr.PrincipalStress(jr.AMDGPUBackend, ni2)
    bad.σ3 = jr.fzeros((2, 6, 5), _dev())
    with pytest.raises(ValueError):
        jr.compute_principal_stresses_(st2, bad, handle=h)
    with pytest.raises(TypeError):
        jr.PrincipalStress(jr.AMDGPUBackend, (6.0, 5.0))
    assert h.get_option("stat_principal_calls") == calls
    jr.compute_principal_stresses_(st3, jr.PrincipalStress(jr.AMDGPUBackend, ni3), handle=h)
    assert h.get_option("stat_principal_calls") == calls + 1
    jr.compute_principal_stresses_(st2, jr.PrincipalStress(jr.AMDGPUBackend, ni2), handle=h)
    assert h.get_option("stat_principal_calls") == calls + 2
    assert isinstance(h, _lib.Handle)


def test_c_abi_refuses_null_pointers_and_empty_extents(jr):
    import ctypes as C
    from justrelax_jl_amd.arrays import ptr
    h = _handle()
    ni = (4, 3, 2)
    σ = jr.PrincipalStress(jr.AMDGPUBackend, ni)
    τ = [jr.fzeros(ni, _dev()) for _ in range(6)]
    calls = h.get_option("stat_principal_calls")
    P = lambda ts: [C.c_void_p(ptr(t)) for t in ts]
    out3, in3 = P((σ.σ1, σ.σ2, σ.σ3)), P(τ)
    i64 = lambda *v: [C.c_int64(x) for x in v]
    for k in range(9):
        args = out3 + in3
        args[k] = C.c_void_p(0)
        assert h.lib.jrx_principal_stresses3d(h._h, *args, *i64(*ni)) == 4
    for dims in ((0, 3, 2), (4, 0, 2), (4, 3, 0), (-1, 3, 2)):
        assert h.lib.jrx_principal_stresses3d(h._h, *out3, *in3, *i64(*dims)) == 4
    # outputs that overlap each other or an input
    assert h.lib.jrx_principal_stresses3d(h._h, out3[0], out3[0], out3[2], *in3, *i64(*ni)) == 4
    assert h.lib.jrx_principal_stresses3d(h._h, *out3, in3[0], *in3[1:], *i64(*ni)) == 0
    assert h.get_option("stat_principal_calls") == calls + 1
    assert h.lib.jrx_principal_stresses3d(h._h, out3[0], out3[1], C.c_void_p(ptr(τ[0])), *in3, *i64(*ni)) == 4
    s2 = jr.PrincipalStress(jr.AMDGPUBackend, (4, 3))
    t2 = [jr.fzeros((4, 3), _dev()) for _ in range(3)]
    out2, in2 = P((s2.σ1, s2.σ2)), P(t2)
    for k in range(5):
        args = out2 + in2
        args[k] = C.c_void_p(0)
        assert h.lib.jrx_principal_stresses2d(h._h, *args, *i64(4, 3)) == 4
    for dims in ((0, 3), (4, 0)):
        assert h.lib.jrx_principal_stresses2d(h._h, *out2, *in2, *i64(*dims)) == 4
    assert h.get_option("stat_principal_calls") == calls + 1
    assert h.lib.jrx_principal_stresses2d(h._h, *out2, *in2, *i64(4, 3)) == 0
    assert h.get_option("stat_principal_calls") == calls + 2


# ----------------------------------------------------------------------------------------------------------------------------------------- in a time step
def test_after_a_3d_stokes_solve(jr):
    """SolVi3D 16³ (200 PT iterations), shear2center!, compute_principal_stresses!: the result matches host eigh on the downloaded τ"""
    from justrelax_jl_amd.miniapps.common import upload_stokes
    s = jr.miniapps.solvi3d(16, iterMax=199, nout=100)
    stokes, ρg, K, G = upload_stokes(s, jr.AMDGPUBackend)
    jr.solve_(stokes, s.pt, s.grid, s.flow_bcs, ρg, K, G, s.dt, None, kwargs=s.kwargs)
    jr.shear2center_(stokes.τ)
    σ = jr.PrincipalStress(jr.AMDGPUBackend, s.ni)
    jr.compute_principal_stresses_(stokes, σ)
    n = int(np.prod(s.ni))
    c = {k: _flat(getattr(stokes.τ, k)).cpu().numpy() for k in ("xx", "yy", "zz", "yz_c", "xz_c", "xy_c")}
    assert np.abs(c["xy_c"]).max() > 0 and np.abs(c["xx"]).max() > 0
    A = np.stack([np.stack([c["xx"], c["xy_c"], c["xz_c"]], 1), np.stack([c["xy_c"], c["yy"], c["yz_c"]], 1),
                  np.stack([c["xz_c"], c["yz_c"], c["zz"]], 1)], 1)
    _check3d(A, _vectors(σ, n))
