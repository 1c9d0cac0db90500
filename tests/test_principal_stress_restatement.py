"""Principal stresses (PrincipalStress, compute_principal_stresses!) without a GPU: the NumPy restatement of PrincipalStresses.jl the GPU tests check
against (tests/_principal.py) is itself checked -- the reference's pinned 3D case, agreement with eigvalsh where the reference's iteration converges, the
simple shear it cannot split (the documented 3D deviation), the 2D quirks kept -- and the drop-in layers declare the feature: the exported C symbols, the
C prototypes, the Julia methods, the integration table."""
import re

import numpy as np
import pytest

import _principal as PS
from _abi_parse import JULIA_EXT, ROOT, c_prototypes


def test_reference_case_sum_of_magnitudes_is_six():
    """test/test_types.jl:222-238: Σ ‖σ_j‖ = 6 within 1e-6 (all three eigenvalues positive, trace 6)"""
    c = PS.REFERENCE_CASE
    sig, converged, _ = PS.hessenberg_eigen_3x3(PS.tensor3(c["xx"], c["yy"], c["zz"], c["yz"], c["xz"], c["xy"]))
    assert converged
    assert abs(sum(np.linalg.norm(s) for s in sig) - 6.0) <= 1e-6
    lam = [np.linalg.norm(s) for s in sig]
    assert np.allclose(lam, PS.REFERENCE_EIGENVALUES, rtol=0, atol=1e-7)


def test_restatement_agrees_with_eigvalsh_where_the_iteration_converges():
    rng = np.random.default_rng(20261016)
    n_conv = 0
    for _ in range(200):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        lam = rng.uniform(0.5, 4.0, 3) * rng.choice([-1.0, 1.0], 3)
        A = Q @ np.diag(lam) @ Q.T
        A = (A + A.T) / 2
        sig, converged, _ = PS.hessenberg_eigen_3x3(A)
        if not converged:
            continue
        n_conv += 1
        w = np.linalg.eigvalsh(A)[::-1]
        got = np.array([np.dot(s, s) ** 0.5 for s in sig])
        assert np.allclose(np.sort(got), np.sort(np.abs(w)), rtol=0, atol=1e-9)
        for s in sig:                                        # each σ_j is an eigenvalue times a unit eigenvector
            assert np.linalg.norm(A @ s - np.sign(s @ (A @ s)) * np.linalg.norm(s) * s) <= 1e-8 * max(1.0, np.linalg.norm(s))
    assert n_conv >= 100


@pytest.mark.parametrize("s", [1.0, 1.0e8])
def test_simple_shear_defeats_the_reference_iteration(s):
    """the documented 3D deviation: eigenvalues ±s, 0; the shift H[3,3] = 0 and unshifted QR cannot separate ±s, so after 50 iterations the reference
    returns zeros -- the device computes (s, 0, −s)"""
    sig, converged, it = PS.hessenberg_eigen_3x3(PS.tensor3(0.0, 0.0, 0.0, 0.0, 0.0, s))
    assert not converged and it == 50
    assert all(np.all(v == 0.0) for v in sig)
    assert np.allclose(np.linalg.eigvalsh(PS.tensor3(0.0, 0.0, 0.0, 0.0, 0.0, s)), [-s, 0.0, s])


def test_pa_scale_stresses_never_meet_the_absolute_tolerance():
    """at 1e7 Pa the 1e-10 absolute tolerance is never met: all 50 iterations run, and the values still come out right"""
    rng = np.random.default_rng(7)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    A = Q @ np.diag([3.0e7, 1.0e7, -2.0e7]) @ Q.T
    A = (A + A.T) / 2
    sig, converged, it = PS.hessenberg_eigen_3x3(A)
    assert not converged and it == 50
    got = np.sort([np.sign(s @ (A @ s)) * np.linalg.norm(s) for s in sig])
    assert np.allclose(got, [-2.0e7, 1.0e7, 3.0e7], rtol=1e-9, atol=0)


def test_2d_quirks_kept():
    """the 2D closed form as written: diag(1, −1) gives ±√2 (the /2 where the eigenvalues need /4), τxx < τyy puts σ1 on the minor axis, 0/0 gives NaN"""
    s1, s2 = PS.principal2d(np.array([1.0]), np.array([-1.0]), np.array([0.0]))
    assert np.allclose(s1[:, 0], [np.sqrt(2), 0.0]) and np.allclose(s2[:, 0], [0.0, -np.sqrt(2)])
    s1, s2 = PS.principal2d(np.array([-1.0]), np.array([1.0]), np.array([0.0]))
    assert np.allclose(s1[:, 0], [np.sqrt(2), 0.0])                # a + b along x although the major axis is y
    s1, s2 = PS.principal2d(np.array([2.0]), np.array([2.0]), np.array([0.0]))
    assert np.all(np.isnan(s1)) and np.all(np.isnan(s2))
    s1, _ = PS.principal2d(np.array([2.0]), np.array([2.0]), np.array([1.0]))      # atan(±Inf): θ = π/4
    assert np.allclose(s1[:, 0], (2.0 + 1.0) * np.array([np.cos(np.pi / 4), np.sin(np.pi / 4)]))


def test_library_exports_both_entry_points():
    from justrelax_jl_amd import _lib
    L = _lib.load()
    for name in ("jrx_principal_stresses2d", "jrx_principal_stresses3d"):
        assert hasattr(L, name), name


def test_header_declares_the_entry_points():
    protos = c_prototypes()
    assert len(protos["jrx_principal_stresses2d"]) == 8
    assert len(protos["jrx_principal_stresses3d"]) == 13
    hdr = (ROOT / "include" / "jrx.h").read_text()
    assert "stat_principal_calls" in hdr and "PrincipalStresses.jl" in hdr


def test_python_api_exports_the_feature(jr):
    assert jr.PrincipalStress is not None
    from justrelax_jl_amd import gridops
    assert callable(gridops.compute_principal_stresses_) and callable(gridops.compute_principal_stresses)
    with pytest.raises(TypeError):
        jr.PrincipalStress(jr.CPUBackend, (4.0, 4.0))
    with pytest.raises(TypeError):
        jr.PrincipalStress(jr.CPUBackend, (4,))


def test_extension_defines_the_methods():
    txt = JULIA_EXT.read_text()
    assert re.search(r"\$JR\.PrincipalStress\(::Type\{AMDGPUBackend\}", txt)
    assert re.search(r"\$JR\.compute_principal_stresses\(::Type\{AMDGPUBackend\}", txt)
    assert re.search(r"\$JR\.compute_principal_stresses!\(stokes, σ::JustRelax\.PrincipalStress\{<:ROCArray\}\)", txt)
    assert "jrx_principal_stresses2d" in txt and "jrx_principal_stresses3d" in txt


def test_integration_notes_list_principal_stresses_as_provided():
    txt = (ROOT / "INTEGRATION.md").read_text()
    for line in txt.splitlines():
        if "not provided" in line:
            assert "PrincipalStress" not in line and "compute_principal_stresses" not in line, line
    assert "jrx_principal_stresses2d" in txt and "jrx_principal_stresses3d" in txt
