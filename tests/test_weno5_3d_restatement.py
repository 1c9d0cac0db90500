"""3D WENO-5 advection without a GPU: the NumPy restatement the GPU tests check against (tests/_weno5_3d.py) is itself checked -- it reduces to the 2D
restatement (which is pinned to the reference) on z-replicated fields, it commutes with axis permutations, it preserves constants, it keeps the zero flux
difference at the ends, it converges at the scheme's order -- and the drop-in layers declare the feature."""
import re

import numpy as np
import pytest

import _weno5 as W2
import _weno5_3d as W
from _abi_parse import JULIA_EXT, ROOT, c_prototypes


@pytest.mark.parametrize("method", [1, 2])
def test_z_replicated_field_reduces_to_the_2d_restatement(method):
    """both z terms are exactly 0 on a field constant along z, whatever vz is: every plane equals the 2D result bit for bit"""
    rng = np.random.default_rng(20261018)
    nx, ny, nz = 17, 19, 6
    u2 = W.sample_field(nx, ny, rng)
    vx2, vy2 = rng.uniform(-1, 1, (nx, ny)), rng.uniform(-1, 1, (nx, ny))
    rep = lambda a: np.repeat(a[:, :, None], nz, axis=2)
    vz = rng.uniform(-1, 1, (nx, ny, nz))
    dx, dy, dz, dt = 1 / 16, 1 / 18, 1 / 5, 0.4 / 18
    unew, ut, _ = W.advect3(rep(u2), rep(vx2), rep(vy2), vz, dx, dy, dz, dt, method)
    ref_u, ref_ut, _ = W2.advect(u2, vx2, vy2, dx, dy, dt, method)
    assert np.abs(ref_u - u2).max() > 0.0
    for k in range(nz):
        assert np.array_equal(unew[:, :, k], ref_u), k
        assert np.array_equal(ut[:, :, k], ref_ut), k


@pytest.mark.parametrize("perm", [(1, 0, 2), (2, 1, 0), (1, 2, 0)])
@pytest.mark.parametrize("method", [1, 2])
def test_axis_permutation_permutes_the_result(method, perm):
    """the sum order of the six rhs terms differs between the two, so equality is to rounding (1e-14), not bitwise"""
    rng = np.random.default_rng(7)
    shape = (9, 11, 13)
    u = 1.0 + 0.5 * rng.standard_normal(shape)
    v = [rng.uniform(-1, 1, shape) for _ in range(3)]
    d = (0.11, 0.07, 0.05)
    dt = 0.4 * min(d)
    ref = W.advect3(u, *v, *d, dt, method)
    got = W.advect3(u.transpose(perm), *(v[p].transpose(perm) for p in perm), *(d[p] for p in perm), dt, method)
    for g, r in zip(got[:2], ref[:2]):
        r = r.transpose(perm)
        assert np.abs(g - r).max() / np.abs(r).max() <= 1e-14


@pytest.mark.parametrize("method", [1, 2])
def test_constant_field_is_preserved(method):
    rng = np.random.default_rng(20261018)
    u = np.full((7, 9, 8), 1234.5678)
    v = [rng.uniform(-1, 1, u.shape) for _ in range(3)]
    unew, ut, _ = W.advect3(u, *v, 0.1, 0.2, 0.15, 0.01, method)
    assert np.abs(ut - u).max() == 0.0
    assert np.abs(unew - u).max() <= np.spacing(1234.5678)


def test_first_and_last_plane_have_zero_flux_difference():
    """kD, kU are clamped like iS, iN, jW, jE: with vz > 0 the z term of the first plane vanishes, with vz < 0 that of the last"""
    rng = np.random.default_rng(1)
    u = np.repeat(W.sample_field(9, 7, rng)[:, :, None], 5, axis=2) * (1.0 + 0.1 * rng.standard_normal((9, 7, 5)))
    zero = np.zeros_like(u)
    r = W.rhs3(u, zero, zero, np.ones_like(u), 0.1, 0.1, 0.1, 2)
    assert np.all(r[:, :, 0] == 0.0) and np.any(r[:, :, 1:] != 0.0)
    r = W.rhs3(u, zero, zero, -np.ones_like(u), 0.1, 0.1, 0.1, 2)
    assert np.all(r[:, :, -1] == 0.0) and np.any(r[:, :, :-1] != 0.0)


def test_gaussian_case_converges_at_the_scheme_order():
    """n = 32 / 64 for Z: order >= 3.3 (the 2D test's bound) and e64 <= 1e-5 (measured 7.44e-5 / 3.42e-6, order 4.45).  JS at n = 32 only (n = 64 for both
    methods would double the time of this, the slowest CPU test): its error must stay below 1.6e-4 = the e64 bound scaled by 2^4, the scheme's order in the
    smooth regime (measured 1.084e-4; the GPU test runs both sizes for both methods)"""
    e32 = W.gaussian_case3(32, 2)[2]
    e64 = W.gaussian_case3(64, 2)[2]
    assert np.log2(e32 / e64) >= 3.3, (e32, e64)
    assert e64 <= 1.0e-5
    assert W.gaussian_case3(32, 1)[2] <= 1.6e-4


def test_header_declares_the_entry_point():
    protos = c_prototypes()
    assert "jrx_weno5_advection3d" in protos
    assert len(protos["jrx_weno5_advection3d"]) == 22


def test_extension_defines_the_3d_methods():
    txt = JULIA_EXT.read_text()
    assert "jrx_weno5_advection3d" in txt
    assert re.search(r"JR3D\.WENO5\(::Type\{AMDGPUBackend\}, \w*::Val\{M\}, \w*::NTuple\{3", txt)
    assert re.search(r"function JR3D\.WENO_advection!\(u::\w+, Vxi::NTuple\{3\}", txt)


def test_integration_notes_list_the_entry_point():
    assert "jrx_weno5_advection3d" in (ROOT / "INTEGRATION.md").read_text()
