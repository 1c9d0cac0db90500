"""GPU: heat diffusion (heatdiffusion_PT_, 2D and 3D, array and rheology form) on inputs that tell a right kernel from a nearly right one, against the longdouble
restatement of the reference's formulas (tests/_heat_diffusion.py) and against the CPU oracle.

Inputs (fixed seeds): K in U(2, 5), ρCp = 3.96e6 U(0.7, 1.3), H = 1e-6 U(0, 2), shear_heating = 1e-7 U(0, 2), T = 1600 + 300 U(0, 1) ghosts included, random non-zero
initial qT* (and qT*2: a constant-flux face must keep them), li = (100, 73, 131) km so that no two spacings are equal, θr_dτ and dτ_ρ from PTThermalCoeffs on the device.

Boundary conditions: a face is constant Value, No flux, constant Flux or nOthing.  L<r> gives face number k of (left, right, top, bot) / (left, right, front, back, top, bot)
the kind "VNFO"[(k + r) % 4]: over L0 .. L3 every face has had every kind.  P<axis>: that pair periodic (two-kernel path, stand-alone BC kernels), the other faces as in L<axis>.

Cadences (iterMax, nout): (45, 20) odd runs of 19, a tail of 4 fused iterations, a last iteration that is no check; (70, 7) even runs of 6: the observed iteration works on
the caller's arrays; (99, 33) runs of exactly 32 = one graph each; (300, 100) runs of 99 = three graphs and 3 single launches.

  case       BCs  cadence     form      what it is for
  2D  k_thermal2d_fused<FTX>, FTX = nx > 128 ? 256 : (nx > 64 ? 128 : 64); k_flux2d / k_updateT2d on the observed iterations and on every one of the two-kernel paths
  2x2        L0   (300, 100)  array     64-wide; the smallest grid: every cell a corner cell, both clamped neighbours the cell itself
  3x130      L1   (45, 20)    rheology  64-wide; 3 of 64 lanes hold a cell, dx >> dy
  63x5       L2   (70, 7)     array     64-wide; the row ends one lane before the wave does (i == nx - 1 recomputes the high face, lane 63 idles)
  64x9       L3   (99, 33)    rheology  64-wide; the row fills the wave exactly
  65x33      L0   (99, 33)    array     128-wide; second wave with one live lane
  127x4      L1   (300, 100)  array     128-wide; the row ends inside the second wave
  128x6      L2   (45, 20)    rheology  128-wide; the row fills the block
  128x6b     L3   (70, 7)     array     128-wide with the fourth BC set (bot constant flux, left nothing)
  129x7      L3   (300, 100)  array     256-wide; third wave with one live lane, fourth wave leaves whole (i & ~63 >= nx)
  130x67     L0   (70, 7)     rheology  256-wide; partial third wave, many rows
  257x5      L1   (99, 33)    array     256-wide; two blocks per row, the second with one live lane
  300x130    L2   (45, 20)    array     256-wide; two blocks per row, rows across the XCD slabs
  65x33px    Px   (45, 20)    array     periodic left / right: no fused launch, k_tbc2d
  129x7py    Py   (99, 33)    rheology  periodic bot / top: no fused launch, k_tbc2d
  3D  row segments k_thermal3d_fused<TX, KZ, 8, R> (TX by nx as in 2D; on grids of fewer than 4096 waves KZ = 1), tiles k_thermal3d_fused_t<4 | 8, 4, .> by "thermal_tile",
      deeper z chunks and two rows per thread by "thermal_cfg" = R 10000 + (TX / 64) 100 + KZ (the instantiations that the dispatch takes from 4096 waves on)
  2x2x2      L0   (300, 100)  array     the smallest grid the entry point accepts; tiles 4, 8 (one partial tile); cfg 10104
  20x9x7     L1   (45, 20)    rheology  nx < 64; 9 rows = 2 (1) whole tiles of 4 (8) and a partial one; 7 planes = a whole z chunk of 4 and a partial one; cfg 10104, 20404 (2 rows per thread, last row alone)
  64x8x5     L2   (70, 7)     array     nx = 64: whole wave; 8 rows = whole tiles only; cfg 10104 (4 + 1 planes), 10102 (2 + 2 + 1)
  65x16x6    L3   (99, 33)    rheology  nx = 65: 128-wide, second wave (second tile column) with one live lane; whole tiles; cfg 10204 (4 + 2), 10202 (whole chunks)
  130x5x9    L0   (45, 20)    array     256-wide, partial third wave; 5 rows = partial tiles; cfg 10404, 10408 (8 + 1), 10402, 20404
  20x9x7px   Px   (45, 20)    array     periodic left / right: no fused launch, k_tbc3d
  20x9x7py   Py   (70, 7)     rheology  periodic front / back
  20x9x7pz   Pz   (99, 33)    array     periodic bot / top

Every path of a case (fused with graphs, fused with plain launches, two kernels [2D: with and without graphs], 3D tiles and cfgs) must give the bits of the first one for T, qT*,
qT*2, ResT and the norm history; the first one is compared with the restatement: whole arrays, ghost edges and corners included, so the in-kernel replay of thermal_bcs! has to
reproduce the reference's statement order.  Bound per case and field: 100 x the distance between the float64 and the longdouble restatement (floor 1e-13, cap 1e-9), see
tests/_heat_diffusion.py; device against oracle: 1e-9.

Seen on the MI355X: every field of every case at 0.0100 of its bound or below -- the device agrees with the float64 restatement to the last bit (no contraction: the
kernels are built with -ffp-contract=off), so its distance from the longdouble one is the yardstick's own 1 / 100; the norm history, summed in another order, at most 0.0113
of its bound (case 65x33px).  The whole file takes 4 s."""
import numpy as np
import pytest

import _heat_diffusion as hd

pytestmark = pytest.mark.gpu
OPTIONS = ("thermal_fused", "loop_graphs", "thermal_tile", "thermal_cfg")
ATTR = dict(dT="ΔT")
CFGS3D = {"2x2x2": (10104,), "20x9x7": (10104, 20404), "64x8x5": (10104, 10102), "65x16x6": (10204, 10202), "130x5x9": (10404, 10408, 10402, 20404)}


def _paths(case_id, nd):
    """(name, options): the first one is compared with the restatement, the others with the first"""
    p = [("fused, graphs", dict(thermal_fused=1, loop_graphs=1)), ("fused, plain launches", dict(thermal_fused=1, loop_graphs=0)),
         ("two kernels", dict(thermal_fused=0, loop_graphs=0))]
    if nd == 2:
        p.append(("two kernels, graphs", dict(thermal_fused=0, loop_graphs=1)))
    else:
        p += [(f"tile {t}", dict(thermal_fused=1, loop_graphs=1, thermal_tile=t)) for t in (4, 8)]
        p += [(f"cfg {c}", dict(thermal_fused=1, loop_graphs=1, thermal_cfg=c)) for c in CFGS3D.get(case_id, ())]
    return p


def _device_inputs(jr, inp):
    import torch
    from justrelax_jl_amd.arrays import from_numpy
    dev = torch.device("cuda", torch.cuda.current_device())
    nd = len(inp.ni)
    thermal = jr.ThermalArrays(jr.AMDGPUBackend, inp.ni)
    for name in ("T", "Told", "H", "shear_heating") + hd.QNAMES[:nd] + tuple(q + "2" for q in hd.QNAMES[:nd]):
        getattr(thermal, name).copy_(from_numpy(inp.arrays[name], dev))
    K, ρCp = from_numpy(inp.arrays["K"], dev), from_numpy(inp.arrays["rhoCp"], dev)
    pt = jr.PTThermalCoeffs(jr.AMDGPUBackend, K, ρCp, inp.dt, inp.di, inp.li, CFL=inp.CFL, ϵ=1e-30)
    return thermal, pt, K, ρCp


def _download(jr, thermal, nd):
    return {k: jr.to_numpy(getattr(thermal, ATTR.get(k, k))) for k in hd.compared_fields(nd)}


def _solve_all_paths(jr, case_id, inp, form, cadence):
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.grid import Geometry, init_global_grid
    nd = len(inp.ni)
    iterMax, nout = cadence
    init_global_grid(*inp.ni) if nd == 3 else init_global_grid(inp.ni[0], inp.ni[1], 1)
    grid = Geometry(inp.ni, inp.li)
    assert tuple(grid._di["center"]) == inp._di
    faces = hd.FACES[nd]
    bc = jr.TemperatureBoundaryConditions(**{k: {f: getattr(inp.bc, k)[f] for f in faces} for k in ("no_flux", "constant_value", "constant_flux", "periodic")})
    periodic = any(inp.bc.periodic.values())
    h = _lib.default_handle()
    saved = {k: h.get_option(k) for k in OPTIONS}
    outs = []
    try:
        for name, opts in _paths(case_id, nd):
            for k in OPTIONS:
                h.set_option(k, opts.get(k, 0))
            thermal, pt, K, ρCp = _device_inputs(jr, inp)
            A, B = (hd.RHEOLOGY, None) if form == "rheology" else (K, ρCp)
            f0, g0 = h.get_option("stat_thermal_fused"), h.get_option("stat_graph_replays")
            r = jr.heatdiffusion_PT_(thermal, pt, bc, A, B, inp.dt, grid, kwargs=dict(iterMax=iterMax, nout=nout, verbose=False))
            fused, replays = h.get_option("stat_thermal_fused") - f0, h.get_option("stat_graph_replays") - g0
            # the branch taken, by the launch counters: every unobserved iteration one fused launch (none with a periodic face or with the two kernels); a graph launch per
            # whole 32 iterations of a run (3D: fused iterations only; 2D: pairs of the two kernels as well)
            want_fused = hd.expected_fused(iterMax, nout) if opts["thermal_fused"] and not periodic else 0
            graphed = opts["loop_graphs"] and not periodic and (opts["thermal_fused"] or nd == 2)
            want_replays = hd.expected_replays(iterMax, nout) if graphed else 0
            assert (fused, replays) == (want_fused, want_replays), (name, fused, replays, want_fused, want_replays)
            outs.append((name, r, _download(jr, thermal, nd)))
            del thermal, pt, K, ρCp
    finally:
        for k, v in saved.items():
            h.set_option(k, v)
    return outs


def _run_case(jr, oracle, case_id, ni, bc_name, cadence, form):
    from justrelax_jl_amd.checks import max_rel_diff
    from justrelax_jl_amd.miniapps.thermal2d import pt_thermal_coeffs_np
    nd = len(ni)
    inp = hd.make_inputs(ni, bc_name, hd.case_seed(case_id))
    # θr_dτ, dτ_ρ as the device evaluates them: inputs of the restatement and of the oracle as well
    _, pt, _, _ = _device_inputs(jr, inp)
    a = inp.arrays
    a["thetar_dtau"][...], a["dtau_rho"][...] = jr.to_numpy(pt.θr_dτ), jr.to_numpy(pt.dτ_ρ)
    th, dr = pt_thermal_coeffs_np(a["K"], a["rhoCp"], inp.dt, inp.di, inp.li, inp.CFL)
    assert np.allclose(a["thetar_dtau"], th, rtol=1e-14, atol=0) and np.allclose(a["dtau_rho"], dr, rtol=1e-14, atol=0)
    assert a["thetar_dtau"].std() > 0.01 * a["thetar_dtau"].mean()          # the coefficients do vary in space
    y = hd.yardstick(inp, form, *cadence)
    ref, r_ref = hd.oracle_solve(oracle, inp, form, *cadence)
    outs = _solve_all_paths(jr, case_id, inp, form, cadence)
    name0, r0, got = outs[0]
    # --- against the longdouble restatement
    assert list(r0.iter_count) == list(y.result["iter_count"]) == list(range(cadence[1], cadence[0] + 1, cadence[1]))
    ratios = hd.ratios_to_bound(got, dict(norm_ResT=r0.norm_ResT), y)
    print(f"HEATCASE {case_id} max ratio {max(ratios.values()):.3e}", {k: f"{v:.2e} of {y.bound[k]:.1e}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    # --- against the oracle
    assert list(r0.iter_count) == list(r_ref["iter_count"])
    assert np.allclose(r0.norm_ResT, r_ref["norm_ResT"], rtol=hd.TOL_ITERS, atol=0)
    for k in hd.compared_fields(nd):
        if k == "ResT":
            assert np.abs(got[k] - ref[k]).max() <= hd.TOL_ITERS * y.scale[k], k
        else:
            assert max_rel_diff(got[k], ref[k]) <= hd.TOL_ITERS, k
    # --- every other path: the same bits
    for name, r, out in outs[1:]:
        assert list(r.iter_count) == list(r0.iter_count) and list(r.norm_ResT) == list(r0.norm_ResT), name
        for k in out:
            assert np.array_equal(out[k], got[k]), (name, k)


@pytest.mark.parametrize("case_id,ni,bc,cadence,form", hd.CASES2D, ids=[c[0] for c in hd.CASES2D])
def test_heat_diffusion_2d_inputs(jr, oracle, case_id, ni, bc, cadence, form):
    _run_case(jr, oracle, case_id, ni, bc, cadence, form)


@pytest.mark.parametrize("case_id,ni,bc,cadence,form", hd.CASES3D, ids=[c[0] for c in hd.CASES3D])
def test_heat_diffusion_3d_inputs(jr, oracle, case_id, ni, bc, cadence, form):
    _run_case(jr, oracle, case_id, ni, bc, cadence, form)


@pytest.mark.parametrize("ni", [(1, 5), (5, 1), (1, 4, 4), (4, 4, 1)])
def test_a_grid_of_one_cell_across_is_refused(jr, ni):
    from justrelax_jl_amd import _lib
    from justrelax_jl_amd.grid import Geometry, init_global_grid
    nd = len(ni)
    init_global_grid(*(tuple(ni) + (1,))[:3])
    inp = hd.SimpleNamespace(ni=ni, li=hd.LI[:nd], di=tuple(l / n for l, n in zip(hd.LI, ni)), dt=hd.DT, CFL=0.5,
                             arrays={k: np.ones(s, order="F") for k, s in hd.shapes(ni).items()})
    thermal, pt, K, ρCp = _device_inputs(jr, inp)
    b = hd.boundary_conditions(nd, "L0", (1.0,) * nd)
    bc = jr.TemperatureBoundaryConditions(no_flux=b.no_flux, constant_value=b.constant_value, constant_flux=b.constant_flux, periodic=b.periodic)
    with pytest.raises(_lib.JrxError, match="thermal grid too small"):
        jr.heatdiffusion_PT_(thermal, pt, bc, K, ρCp, inp.dt, Geometry(ni, inp.li), kwargs=dict(iterMax=3, nout=1, verbose=False))
