"""WENO-5 advection (WENO5, WENO_advection!) without a GPU: the NumPy restatement the GPU tests check against (tests/_weno5.py) is itself checked --
constant fields are preserved, the Gaussian case converges at the scheme's order -- and the drop-in layers declare the feature: the C prototype in
include/jrx.h, the Julia methods of the extension, the integration table."""
import re

import numpy as np
import pytest

import _weno5 as W
from _abi_parse import JULIA_EXT, ROOT, c_prototypes


@pytest.mark.parametrize("method", [1, 2])
def test_constant_field_is_preserved_exactly(method):
    rng = np.random.default_rng(20260821)
    u = np.full((17, 19), 1234.5678)
    vx, vy = rng.uniform(-1, 1, u.shape), rng.uniform(-1, 1, u.shape)
    unew, ut, _ = W.advect(u, vx, vy, 0.1, 0.2, 0.01, method)
    assert np.abs(ut - u).max() == 0.0
    assert np.abs(unew - u).max() <= np.spacing(1234.5678)


@pytest.mark.parametrize("method", [1, 2])
def test_gaussian_case_converges_at_the_scheme_order(method):
    e64 = W.gaussian_case(64, method)[2]
    e128 = W.gaussian_case(128, method)[2]
    assert np.log2(e64 / e128) >= 3.3, (e64, e128)
    assert e128 <= 3e-6


def test_first_and_last_vertex_have_zero_flux_difference():
    """weno_rhs clamps iS, iN, jW, jE (weno5.jl:157-158): with vx > 0 the x term of the first column vanishes, with vx < 0 that of the last"""
    u = W.sample_field(9, 7, np.random.default_rng(1))
    r = W.rhs(u, np.ones_like(u), np.zeros_like(u), 0.1, 0.1, 2)
    assert np.all(r[0, :] == 0.0)
    r = W.rhs(u, -np.ones_like(u), np.zeros_like(u), 0.1, 0.1, 2)
    assert np.all(r[-1, :] == 0.0)


def test_header_declares_the_entry_point():
    protos = c_prototypes()
    assert "jrx_weno5_advection2d" in protos
    assert len(protos["jrx_weno5_advection2d"]) == 17


def test_extension_defines_the_methods():
    txt = JULIA_EXT.read_text()
    assert re.search(r"JR2D\.WENO5\(::Type\{AMDGPUBackend\}", txt)
    assert re.search(r"function JR2D\.WENO_advection!\(", txt)
    assert re.search(r"JR3D\.WENO_advection!\(", txt) and "ArgumentError" in txt
    assert "jrx_weno5_advection2d" in txt


def test_integration_notes_list_weno_as_provided():
    txt = (ROOT / "INTEGRATION.md").read_text()
    for line in txt.splitlines():
        if "not provided" in line:
            assert "WENO5" not in line and "WENO_advection!" not in line, line
    assert "jrx_weno5_advection2d" in txt
