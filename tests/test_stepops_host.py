"""CPU: the host side of the per-step operators (pureshear_bc_, free_surface_bcs_, subgrid_characteristic_time_, compute_melt_fraction_): the C
declarations of include/jrx.h against the ccalls and the struct mirror of the Julia extension and against the ctypes binding, and the refusal of CPU arrays."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from _abi_parse import HEADER, c_prototypes, c_structs, julia_ccalls, julia_structs, same_arg

ENTRY_POINTS = ("jrx_pureshear_bc2d", "jrx_pureshear_bc3d", "jrx_free_surface_bcs2d", "jrx_free_surface_bcs3d", "jrx_subgrid_characteristic_time",
                "jrx_compute_melt_fraction")


def test_the_header_declares_the_entry_points_and_the_extension_calls_them_as_declared():
    protos, calls = c_prototypes(), julia_ccalls()
    for fn in ENTRY_POINTS:
        assert fn in protos, fn
        assert fn in calls, f"the Julia extension never calls {fn}"
        for ret, args in calls[fn]:
            assert ret == "Cint" and len(args) == len(protos[fn]), (fn, args, protos[fn])
            assert all(same_arg(w, g) for w, g in zip(protos[fn], args)), (fn, protos[fn], args)
    assert protos["jrx_pureshear_bc2d"] == ["Ptr{Cvoid}"] + ["Ptr{Float64}"] * 4 + ["Float64", "Int64", "Int64"]
    assert protos["jrx_compute_melt_fraction"][3] == "Ref{JrxMelting}"
    assert protos["jrx_subgrid_characteristic_time"][3] == "Ref{JrxThermalPhases}"


def test_jrx_melting_has_the_same_layout_on_all_three_sides(jr):
    from justrelax_jl_amd import _lib
    want = [("nphase", "int32_t", False, 1), ("kind", "int32_t", False, 8), ("a", "double", False, 8), ("b", "double", False, 8), ("c", "double", False, 8)]
    assert c_structs()["jrx_melting"] == want
    assert [(n, c) for n, _, _, c in julia_structs()["JrxMelting"]] == [(n, c) for n, _, _, c in want]
    assert [f[0] for f in _lib.Melting._fields_] == [w[0] for w in want] and C.sizeof(_lib.Melting) == 4 + 32 + 4 + 3 * 64          # 4 B of padding ahead of the doubles
    assert "jrx_compute_melt_fraction" in _lib.declared_symbols() and "jrx_free_surface_bcs3d" in _lib.declared_symbols()


def test_the_header_states_the_departure_and_the_kept_quirk():
    txt = HEADER.read_text()
    sec = txt[txt.index("per-step operators"):]
    for s in ("pure_shear.jl:1-33", "NOT FOLLOWED", "free_surface.jl:1-99", "KEPT QUIRK", "τ_o.yy", "subgrid_diffusion.jl:36-50", "Melting.jl:10-35",
              "MeltingParam_Caricchi", "test/test_rheology.jl:228-253", "stat_stepops_launches"):
        assert s in sec, s


def test_the_names_resolve_and_cpu_arrays_are_refused(jr):
    ni = (5, 4)
    st = jr.StokesArrays(jr.CPUBackend, ni)
    th = jr.ThermalArrays(jr.CPUBackend, ni)
    pr = jr.PhaseRatios(jr.CPUBackend, 1, ni)
    g = jr.Geometry(ni, (1.0, 1.0))
    bcs = jr.VelocityBoundaryConditions(free_slip=dict(left=True, right=True, top=False, bot=True), free_surface=True)
    phase = dict(eta=1.0, G=1.0, Kb=1.0, k=3.0, Cp=1.0e3, density=dict(kind="constant", rho0=3.0e3), melting=dict(kind="caricchi"))
    ϕ = st.P.clone()
    with pytest.raises(NotImplementedError):
        jr.pureshear_bc_(st, g.xci, g.xvi, 1.0, jr.CPUBackend)
    with pytest.raises(NotImplementedError):
        jr.free_surface_bcs_(st, bcs, st.viscosity.η, [phase], pr, 0.5, (0.2, 0.25), (0.2, 0.25))
    with pytest.raises(NotImplementedError):
        jr.subgrid_characteristic_time_(ϕ, pr, [phase], th, st, (0.2, 0.25))
    with pytest.raises(NotImplementedError):
        jr.compute_melt_fraction_(ϕ, [phase], dict(T=1373.15, P=0.0))
    with pytest.raises(NotImplementedError):
        jr.compute_melt_fraction_(ϕ, pr, [phase], SimpleNamespace(T=th.T[1:-1, 1:-1], P=st.P))
    assert not np.any(jr.to_numpy(st.V.Vx)) and not np.any(jr.to_numpy(ϕ))


def test_melting_table_names_what_it_does_not_know(jr):
    from justrelax_jl_amd.stepops import melting_table
    m = melting_table([dict(), dict(melting=dict(kind="caricchi", a=900.0))])
    assert (m.nphase, list(m.kind)[:2], m.a[1], m.b[1], m.c[1]) == (2, [0, 1], 900.0, 23.0, 273.15)
    with pytest.raises(ValueError, match="melting"):
        melting_table([dict(melting=dict(kind="katz"))])
