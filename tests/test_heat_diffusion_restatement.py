"""The CPU oracle's pseudo-transient heat diffusion (oracle/thermal2d.c, oracle/thermal3d.c) against the NumPy restatement of the reference's formulas
(tests/_heat_diffusion.py) in longdouble, on the case table of tests/test_gpu_heat_diffusion_inputs.py: spatially varying K, ρCp, H, shear_heating, θr_dτ, dτ_ρ,
non-zero initial fluxes, three different spacings, every face with every BC kind (constant value, no flux, constant flux, nothing, periodic), iteration
counts that are no multiple of nout -- inputs that the reference's known answers (test_diffusion2D.jl, test_diffusion3D.jl) do not reach.

Bound per case and field: 100 x the distance between the float64 and the longdouble restatement of that case and field (floor 1e-13, cap 1e-9), both
normalised by the field's maximum in the longdouble restatement (ResT: by the larger of its maximum and its largest term)."""
import numpy as np
import pytest

import _heat_diffusion as hd


def cpu_inputs(jr, case_id, ni, bc):
    from justrelax_jl_amd.miniapps.thermal2d import pt_thermal_coeffs_np
    inp = hd.make_inputs(ni, bc, hd.case_seed(case_id))
    a = inp.arrays
    a["thetar_dtau"][...], a["dtau_rho"][...] = pt_thermal_coeffs_np(a["K"], a["rhoCp"], inp.dt, inp.di, inp.li, inp.CFL)
    return inp


@pytest.mark.parametrize("case_id,ni,bc,cadence,form", hd.CASES2D + hd.CASES3D, ids=[c[0] for c in hd.CASES2D + hd.CASES3D])
def test_oracle_matches_the_restatement(jr, oracle, case_id, ni, bc, cadence, form):
    inp = cpu_inputs(jr, case_id, ni, bc)
    y = hd.yardstick(inp, form, *cadence)
    got, r = hd.oracle_solve(oracle, inp, form, *cadence)
    assert list(r["iter_count"]) == list(y.result["iter_count"])
    ratios = hd.ratios_to_bound(got, r, y)
    print(case_id, {k: f"{v:.2e} of {y.bound[k]:.1e}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


def test_restatement_boundary_order_and_kept_flux():
    """the pieces that the solves above cannot tell apart from a compensating mistake: a ghost corner takes the later statement's value (rows, then columns, per kind),
    a periodic ghost is the opposite inner layer, and a constant-flux face keeps its qT*2"""
    from types import SimpleNamespace
    T = np.arange(20.0).reshape(4, 5, order="F").copy(order="F")
    no = dict(left=False, right=False, top=False, bot=False)
    bc = SimpleNamespace(constant_value=dict(no, bot=10.0), no_flux=dict(no, left=True), periodic=dict(no), constant_flux=dict(no))
    T0 = T.copy()
    hd.thermal_bcs(T, bc)
    assert np.array_equal(T[1:, 0], 20.0 - T0[1:, 1]) and np.array_equal(T[0, 1:], T0[1, 1:])
    assert T[0, 0] == 20.0 - T0[1, 1]            # the corner: no_flux copies the bottom ghost that constant_value has just written
    assert np.array_equal(T[1:, 2:], T0[1:, 2:])
    T = T0.copy()
    hd.thermal_bcs(T, SimpleNamespace(constant_value=dict(no), no_flux=dict(no), periodic=dict(no, left=True, right=True), constant_flux=dict(no)))
    assert np.array_equal(T[0], T0[-2]) and np.array_equal(T[-1], T0[1])
    inp = hd.make_inputs((4, 3), "L0", 5)         # L0: top takes a constant flux
    inp.arrays["thetar_dtau"][...] = 0.5
    f = hd.as_dtype(inp.arrays, np.float64)
    hd.compute_flux(f, inp._di, inp.bc)
    assert np.array_equal(f["qTy2"][:, -1], inp.arrays["qTy2"][:, -1]) and (f["qTy"][:, -1] == inp.bc.constant_flux["top"]).all()
    assert not np.array_equal(f["qTy2"][:, :-1], inp.arrays["qTy2"][:, :-1])
    K, T = inp.arrays["K"], inp.arrays["T"]
    assert f["qTx2"][2, 1] == -((K[1, 1] + K[2, 1]) * 0.5) * (T[3, 2] - T[2, 2]) * inp._di[0]
    assert f["qTy2"][0, 0] == -((K[0, 0] + K[0, 0]) * 0.5) * (T[1, 1] - T[1, 0]) * inp._di[1]       # a domain face: the clamped pair is the same cell twice


def test_case_table_covers_every_kind_width_and_cadence():
    """the table above keeps what it promises: every face with every kind and a periodic pair per dimension, the three 2D widths each with the four BC sets and the four
    cadences, every cadence in 3D"""
    for nd, cases in ((2, hd.CASES2D), (3, hd.CASES3D)):
        seen, per = set(), set()
        for _, ni, bc, _, _ in cases:
            b = hd.boundary_conditions(nd, bc, (1.0,) * nd)
            for f in hd.FACES[nd]:
                kind = "P" if b.periodic[f] else "V" if b.constant_value[f] is not False else "N" if b.no_flux[f] else "F" if b.constant_flux[f] is not False else "O"
                seen.add((f, kind))
                if kind == "P":
                    per.add(hd.AXIS[nd][f][0])
        assert seen >= {(f, k) for f in hd.FACES[nd] for k in hd.KINDS} and per == set(range(nd))
        assert {c[3] for c in cases} == {(45, 20), (70, 7), (99, 33), (300, 100)}
    width = lambda nx: 256 if nx > 128 else (128 if nx > 64 else 64)
    for w in (64, 128, 256):
        mine = [c for c in hd.CASES2D if width(c[1][0]) == w and c[2][0] == "L"]
        assert {c[2] for c in mine} == {"L0", "L1", "L2", "L3"} and {c[3] for c in mine} == {(45, 20), (70, 7), (99, 33), (300, 100)}, w
    assert {c[1] for c in hd.CASES2D} >= {(2, 2), (3, 130), (63, 5), (64, 9), (65, 33), (127, 4), (128, 6), (129, 7), (130, 67), (257, 5), (300, 130)}
    assert (hd.expected_fused(45, 20), hd.expected_fused(70, 7), hd.expected_fused(99, 33), hd.expected_fused(300, 100)) == (42, 60, 96, 297)
    assert (hd.expected_replays(45, 20), hd.expected_replays(70, 7), hd.expected_replays(99, 33), hd.expected_replays(300, 100)) == (0, 0, 3, 9)
