"""CPU tests of the thermal-stress restatement (tests/_thermal_stress.py) that the GPU tests of args.ΔT rest on, and of the binding's handling of args.ΔT."""
import numpy as np
import pytest

import _thermal_stress as ts

N = 200_000


def _cells(seed=11, n=N):
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: rng.uniform(lo, hi, size=n)
    return dict(P=u(-2, 2), P0=u(-2, 2), divV=u(-1, 1), Q=u(-1, 1), eta=10.0 ** u(-1, 1), K=u(1, 5), G=u(0.5, 2), dT=u(-2, 2), alpha=u(0, 0.5))


def _P(c, dt, **over):
    a = dict(c, **over)
    kw = dict(dT=a["dT"], alpha=a["alpha"]) if a.get("thermal", True) else {}
    return ts.compute_P(a["P"], a["P0"], a["divV"], a["Q"], a["eta"], a["K"], a["G"], dt, 0.7, 3.1, **kw)


@pytest.mark.parametrize("dt", [0.25, 0.3])
def test_zero_dT_gives_the_bits_of_the_isothermal_form(dt):
    c = _cells()
    for a, b in zip(_P(c, dt, dT=np.zeros(N)), _P(c, dt, thermal=False)):
        assert np.array_equal(a, b)
    for a, b in zip(_P(c, dt, alpha=np.zeros(N)), _P(c, dt, thermal=False)):
        assert np.array_equal(a, b)


def test_source_term_identity_holds_at_a_power_of_two_dt_only():
    """Q = 0: the thermal form equals the isothermal form fed Q' = α ΔT bit for bit when _dt is a power of two (α (ΔT _dt) == (α ΔT) _dt exactly); at dt = 0.3
    the two groupings round differently, by one ulp of the source term"""
    c = _cells()
    zero = np.zeros(N)
    for a, b in zip(_P(c, 0.25, Q=zero), _P(c, 0.25, Q=c["alpha"] * c["dT"], thermal=False)):
        assert np.array_equal(a, b)
    RPa, Pa = _P(c, 0.3, Q=zero)
    RPb, Pb = _P(c, 0.3, Q=c["alpha"] * c["dT"], thermal=False)
    assert not np.array_equal(RPa, RPb) and not np.array_equal(Pa, Pb)
    _dt = 1.0 / 0.3
    sa, sb = c["alpha"] * (c["dT"] * _dt), (c["alpha"] * c["dT"]) * _dt
    # two roundings on either side, each within eps / 2 of its exact product: the two values lie within 2 eps of each other, relative
    assert (sa != sb).any() and np.max(np.abs(sa - sb) / np.abs(sb)) <= 2.5 * np.finfo(float).eps
    assert np.max(np.abs(RPa - RPb)) <= 4 * np.finfo(float).eps * np.max(np.abs(RPb))


def test_fixed_point_is_the_thermal_pressure():
    """∇V = 0, Q = 0: the update leaves P = P0 + K α ΔT unchanged and RP vanishes there (to rounding)"""
    c = _cells(n=2000)
    dt = 0.25
    zero = np.zeros(2000)
    Pfix = c["P0"] + c["K"] * c["alpha"] * c["dT"]
    RP, Pn = _P(c, dt, divV=zero, Q=zero, P=Pfix)
    scale = np.abs(c["P0"]) + np.abs(c["K"] * c["alpha"] * c["dT"])
    assert np.max(np.abs(Pn - Pfix) / scale) <= 8 * np.finfo(float).eps
    assert np.max(np.abs(RP) * c["K"] * dt / scale) <= 8 * np.finfo(float).eps
    # and it is attracting: one update from P0 shrinks the distance by 1 / (1 + _Kdt ψ)
    _, P1 = _P(c, dt, divV=zero, Q=zero, P=c["P0"])
    psi = 1.0 / (1.0 / c["eta"] + 1.0 / (c["G"] * dt)) * 0.7 / 3.1
    far = np.abs(c["P0"] - Pfix) > 1e-3
    assert far.sum() > 1000
    assert np.allclose((P1 - Pfix)[far] / (c["P0"] - Pfix)[far], (1.0 / (1.0 + psi / (c["K"] * dt)))[far], rtol=1e-9, atol=0)


def test_phase_ratio_rules_of_the_thermal_expansion():
    phases = [dict(G=1.0, Kb=2.0, density=dict(kind="T", rho0=1.0, alpha=0.25)), dict(G=1.0, Kb=2.0, density=dict(kind="PT", rho0=1.0, alpha=0.5)),
              dict(G=1.0, Kb=2.0, density=dict(kind="constant", rho0=1.0, alpha=9.0)), dict(G=1.0, Kb=2.0, density=dict(kind="compressible", rho0=1.0, alpha=9.0)),
              dict(G=1.0, Kb=2.0)]
    al = ts.phase_alpha(phases)
    assert al == [0.25, 0.5, 0.0, 0.0, 0.0]
    r = np.array([[1.0, 0.0, 0.0, 0.0, 0.0],        # pure phase 0
                  [0.0, 1.0, 0.0, 0.0, 0.0],        # pure phase 1
                  [0.0, 0.0, 1.0, 0.0, 0.0],        # pure phase without α
                  [0.3, 0.7, 0.0, 0.0, 0.0],        # mixed
                  [0.25, 0.25, 0.5, 0.0, 0.0],      # mixed with a phase without α
                  [0.5, 1.0, 0.0, 0.0, 0.0]]).T     # a ratio of one behind a non-zero one: early return drops what was summed
    a = ts.fn_ratio(al, r, early_return=True)
    assert a.tolist() == [0.25, 0.5, 0.0, 0.25 * 0.3 + 0.5 * 0.7, 0.25 * 0.25 + 0.5 * 0.25, 0.5]
    assert ts.fn_ratio(al, r)[5] == 0.25 * 0.5 + 0.5          # the plain sum (K, G) has no early return
    nan = ts.fn_ratio([np.nan, 0.5, 0, 0, 0], r, early_return=True)
    assert nan[1] == 0.5 and np.isnan(nan[0])               # a zero ratio skips the phase's value, NaN included


def test_own_index_reads_a_ghosted_array_unshifted():
    g = np.arange(42.0).reshape(7, 6)
    assert np.array_equal(ts.own_index(g, (5, 4)), g[:5, :4]) and ts.own_index(g, (7, 6)) is g
    with pytest.raises(ValueError):
        ts.own_index(g, (6, 5))


def test_binding_takes_dT_of_both_extents_and_refuses_others(jr):
    """vep_fields2d / vep_fields3d and the ghost flag on host arrays (no library call): only a caller that asks for the thermal stresses gets ΔT into the struct"""
    from justrelax_jl_amd import stokes as st
    from justrelax_jl_amd.arrays import fzeros
    for ni in ((5, 4), (5, 4, 3)):
        s = jr.StokesArrays(jr.CPUBackend, ni)
        pr = jr.PhaseRatios(jr.CPUBackend, 2, ni)
        rg = tuple(fzeros(ni, "cpu") for _ in ni)
        fields = st.vep_fields2d if len(ni) == 2 else st.vep_fields3d
        f = fields(s, rg, pr, None, thermal_stress=True)
        assert not f.dT and not f.melt_fraction and st._ghosted_ΔT_flag(s, None) == 0
        for shape, flag in ((ni, 0), (tuple(n + 2 for n in ni), 1)):
            dT = fzeros(shape, "cpu", 1.0)
            for args in (dict(ΔT=dT), type("A", (), dict(ΔT=dT))()):
                f = fields(s, rg, pr, args, thermal_stress=True)
                assert f.dT == dT.data_ptr() and st._ghosted_ΔT_flag(s, args) == flag and not f.melt_fraction
                f = fields(s, rg, pr, args)          # the single-phase, variational and DYREL callers: nothing of ΔT in the struct
                assert not f.dT and not f.melt_fraction
        ϕ = fzeros(ni, "cpu")
        f = fields(s, rg, pr, dict(melt_fraction=ϕ), thermal_stress=True)
        assert f.melt_fraction == ϕ.data_ptr() and not f.dT
        for bad in (tuple(n + 1 for n in ni), ni[::-1], ni[:-1]):
            with pytest.raises(ValueError, match="ΔT"):
                fields(s, rg, pr, dict(ΔT=fzeros(bad, "cpu")), thermal_stress=True)
            with pytest.raises(ValueError, match="ΔT"):
                st._ghosted_ΔT_flag(s, dict(ΔT=fzeros(bad, "cpu")))
            fields(s, rg, pr, dict(ΔT=fzeros(bad, "cpu")))          # not read, not checked
