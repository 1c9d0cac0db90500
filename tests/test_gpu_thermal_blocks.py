"""GPU: the heat-diffusion drivers on decomposed grids -- the path of jrx_heatdiffusion_PT2d / _PT3d [_phases] and jrx_thermal2d_iteration that runs only with a communicator:
no fused kernel, no graph replay, k_updateT*<false, false> + thermal_bcs! kernels + jrx_halo_exchange(T) in every iteration, the stop test reduced over the ranks.

Ranks are handles of this process on one device (_blocks.TwoBlocks, halo.run_ranks), comm_timeout_ms = 5000 on every handle: a rank left waiting ends as a JrxError.

Expectation.  The reference applies thermal_bcs! and the constant-flux faces to every face of the LOCAL arrays and averages K, θr_dτ to the faces with indices clamped to the local
block (DiffusionPT_kernels.jl:6-61, :327-364), then update_halo!(thermal.T) replaces the ghost planes that have a neighbour (DiffusionPT_solver.jl:110).  With varying
coefficients a decomposed run is therefore NOT the undecomposed one, in the reference either, and the expectation is the restatement run block by block with the same plane
copies (tests/_heat_diffusion.py: heatdiffusion_PT_blocks, pinned by tests/test_heat_diffusion_blocks.py); for the phase-ratio form it is the CPU oracle stepped block by block
(oracle.thermal_phase_iteration).  Only for a uniform material, and without a constant flux on the split axis, every block equals the undecomposed device run bit for bit.

Inputs as in tests/test_gpu_heat_diffusion_inputs.py (hd.make_inputs on the global grid, then cut: random K, ρCp, H, shear heating, random initial fluxes, T with ghosts), BC sets
L0 .. L3 on both splits, so that the outer faces next to the block face (top / bot for a split along x, left / right along y) take every kind -- value, no flux, constant flux,
nothing -- at the corner they share with the neighbour face.  Cadence (45, 20): the last iteration is no check.

  2D  70 x 33 (ten 256-thread blocks in k_updateT2d / k_flux2d: xcd_slab_block remaps; rows no multiple of 64), 34 x 19, and 3 x 2 / 2 x 3: jrx_cart_create itself sets no
      floor; three cells along the split axis is the smallest block whose sent planes (1-based planes 3 and n - 2 + 1 of T) are both interior cells the block owns.
  3D  24 x 13 x 12 split along x, y, z: rheology form, non-uniform K with constant-flux outer faces, adiabatic term, Dirichlet mask, phase ratios with the phase count as a
      constant and as a run-time loop.

Compared: whole local arrays of T (ghosts and corners included), Told, ΔT, qT*, qT*2, ResT and each rank's norm history.  No entry is masked: every ghost of T is written by a
BC statement, received (whole planes, corners included, x before y before z) or keeps its input value in the restatement and on the device alike.
Bound: 100 x the distance between the float64 and the longdouble block restatement (floor 1e-13, cap 1e-9); oracle comparisons 1e-9.

Ranks leave together (2D and 3D): ϵ is chosen between the two ranks' norms at a check where they differ; both ranks must stop at the first check whose MAXIMUM is under ϵ,
each reporting its own local norms -- the library's documented deviation from the reference's local test, which would leave one rank waiting in the next exchange.

Seen on the MI355X: every field of every restatement case at 0.0100 of its bound or below -- the device equals the float64 block restatement to the last bit, so its distance
from the longdouble one is the yardstick's own 1 / 100; the norm histories, summed in another order, at most 0.0112 of their bound (3D adiabatic case).  Phase-ratio cases:
every field and both PT coefficient arrays equal the oracle's bits, norm histories within 2.3e-16.  The 31 tests of the file take 3.7 s.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import _blocks as B
import _heat_diffusion as hd

pytestmark = pytest.mark.gpu
TIMEOUT_MS = 5000
ATTR = dict(dT="ΔT")
CADENCE = (45, 20)


def _n3(n):
    return tuple(n) + (1,) * (3 - len(n))


def _input_names(nd):
    return ("T", "Told", "H", "shear_heating") + hd.QNAMES[:nd] + tuple(q + "2" for q in hd.QNAMES[:nd])


def _device_bc(jr, bc, nd, dirichlet=None):
    kinds = {k: {f: getattr(bc, k)[f] for f in hd.FACES[nd]} for k in ("no_flux", "constant_value", "constant_flux", "periodic")}
    return jr.TemperatureBoundaryConditions(**kinds, **({"dirichlet": dirichlet} if dirichlet else {}))


def _upload(jr, loc, ni, inp, eps=1e-30):
    """ThermalArrays, PTThermalCoeffs(K, ρCp) of one block; θr_dτ, dτ_ρ as the device evaluates them go back into loc: inputs of the restatement too"""
    import torch
    from justrelax_jl_amd.arrays import from_numpy
    dev = torch.device("cuda", torch.cuda.current_device())
    thermal = jr.ThermalArrays(jr.AMDGPUBackend, ni)
    for name in _input_names(len(ni)):
        getattr(thermal, name).copy_(from_numpy(loc[name], dev))
    K, ρCp = from_numpy(loc["K"], dev), from_numpy(loc["rhoCp"], dev)
    pt = jr.PTThermalCoeffs(jr.AMDGPUBackend, K, ρCp, inp.dt, inp.di, inp.li, CFL=inp.CFL, ϵ=eps)
    loc["thetar_dtau"][...], loc["dtau_rho"][...] = jr.to_numpy(pt.θr_dτ), jr.to_numpy(pt.dτ_ρ)
    return SimpleNamespace(thermal=thermal, pt=pt, K=K, ρCp=ρCp)


def _download(jr, thermal, nd):
    return {k: jr.to_numpy(getattr(thermal, ATTR.get(k, k))) for k in hd.compared_fields(nd)}


class _Grid:
    """the ImplicitGlobalGrid of a decomposition for the duration of a block (Geometry reads it: spacing = li / n_g)"""

    def __init__(self, n3, dims=(1, 1, 1), periods=(0, 0, 0)):
        self.n3, self.dims, self.periods = n3, dims, periods

    def __enter__(self):
        import justrelax_jl_amd.grid as g
        g.init_global_grid(*self.n3, dimx=self.dims[0], dimy=self.dims[1], dimz=self.dims[2], periodx=self.periods[0], periody=self.periods[1], periodz=self.periods[2],
                           rank=0, nprocs=int(np.prod(self.dims)))
        return self

    def __exit__(self, *exc):
        import justrelax_jl_amd.grid as g
        g.finalize_global_grid()


def _cut(arrays, tb, nd):
    return [{k: B.local_block(v, tb.n, tb.ng, B.coords_of(tb.carts[r]), nd=nd) for k, v in arrays.items()} for r in range(len(tb.carts))]


def _solve_blocks(jr, tb, inp, locs, form, cadence, *, eps=1e-30, dirichlet=None, stokes=None):
    """upload every rank's block and run heatdiffusion_PT! on all ranks at once; returns (results, downloaded fields, uploads)"""
    import torch
    from justrelax_jl_amd import halo
    from justrelax_jl_amd.arrays import from_numpy
    nd = len(inp.ni)
    ni = tb.n[:nd]
    dev = torch.device("cuda", torch.cuda.current_device())
    with _Grid(tb.n, tb.dims, tb.periods):
        grid = jr.Geometry(ni, inp.li)
        assert tuple(grid._di["center"]) == tuple(inp._di)
        ups, fns = [], []
        for r, h in enumerate(tb.handles):
            h.set_option("comm_timeout_ms", TIMEOUT_MS)
            u = _upload(jr, locs[r], ni, inp, eps)
            d = None
            if dirichlet is not None:
                d = dict(constant=dirichlet, mask=from_numpy(locs[r]["dirichlet_mask"], dev))
            u.bc = _device_bc(jr, inp.bc, nd, d)
            kw = dict(iterMax=cadence[0], nout=cadence[1], verbose=False)
            if stokes is not None:
                kw["stokes"] = SimpleNamespace(P=from_numpy(stokes[r][0], dev), P0=from_numpy(stokes[r][1], dev))
            A, Bm = (hd.RHEOLOGY, None) if form == "rheology" else (u.K, u.ρCp)
            ups.append(u)
            fns.append(lambda u=u, A=A, Bm=Bm, kw=kw, h=h: jr.heatdiffusion_PT_(u.thermal, u.pt, u.bc, A, Bm, inp.dt, grid, kwargs=kw, handle=h))
        res = halo.run_ranks(fns)
        outs = [_download(jr, u.thermal, nd) for u in ups]
    return res, outs, ups


def _assert_within_bounds(tag, res, outs, ys):
    worst = 0.0
    for r, (rr, out, y) in enumerate(zip(res, outs, ys)):
        assert list(rr.iter_count) == list(y.result["iter_count"]), (tag, r)
        ratios = hd.ratios_to_bound(out, dict(norm_ResT=rr.norm_ResT), y)
        print(f"BLOCKCASE {tag} rank {r} max ratio {max(ratios.values()):.3e}", {k: f"{v:.2e} of {y.bound[k]:.1e}" for k, v in ratios.items()})
        worst = max(worst, max(ratios.values()))
        assert max(ratios.values()) <= 1.0, (tag, r, ratios)
    return worst


# (id, dims, local block, BCs, form); over the cases top / bot (split along x) and left / right (split along y) take each of the four kinds
CASES2D = [("70x33-x-L0", (2, 1, 1), (70, 33), "L0", "array"), ("34x19-x-L1", (2, 1, 1), (34, 19), "L1", "rheology"), ("3x2-x-L2", (2, 1, 1), (3, 2), "L2", "array"),
           ("70x33-x-L3", (2, 1, 1), (70, 33), "L3", "rheology"), ("34x19-y-L0", (1, 2, 1), (34, 19), "L0", "array"), ("70x33-y-L1", (1, 2, 1), (70, 33), "L1", "array"),
           ("70x33-y-L2", (1, 2, 1), (70, 33), "L2", "rheology"), ("2x3-y-L3", (1, 2, 1), (2, 3), "L3", "rheology"), ("34x19-x-L2", (2, 1, 1), (34, 19), "L2", "array"),
           ("34x19-y-L3", (1, 2, 1), (34, 19), "L3", "rheology")]
CASES3D = [("x-L1-rheology", (2, 1, 1), "L1", "rheology"), ("y-L0-array", (1, 2, 1), "L0", "array"), ("z-L2-array", (1, 1, 2), "L2", "array"), ("y-L3-rheology", (1, 2, 1), "L3", "rheology")]
N3D = (24, 13, 12)


def test_case_tables_cover_every_kind_at_the_corner_of_a_block_face():
    for ax, others in ((0, ("top", "bot")), (1, ("left", "right"))):
        seen = set()
        for _, dims, n, bc, _ in CASES2D:
            if dims.index(2) == ax:
                b = hd.boundary_conditions(2, bc, (1.0, 1.0))
                for f in others:
                    seen.add((f, "V" if b.constant_value[f] is not False else "N" if b.no_flux[f] else "F" if b.constant_flux[f] is not False else "O"))
        assert seen == {(f, k) for f in others for k in hd.KINDS}, (ax, seen)
    assert {c[2] for c in CASES2D} == {(70, 33), (34, 19), (3, 2), (2, 3)} and {c[4] for c in CASES2D} == {"array", "rheology"}
    assert {c[1] for c in CASES3D} == {(2, 1, 1), (1, 2, 1), (1, 1, 2)}


def _run_case(jr, tag, dims, n, bc_name, form, *, adiabatic=False, dirichlet=False):
    from justrelax_jl_amd import _lib
    nd = len(n)
    L = _lib.load()
    with B.TwoBlocks(_n3(n), dims) as tb:
        inp = hd.make_inputs(tb.ng[:nd], bc_name, hd.case_seed(tag))
        arrays = dict(inp.arrays)
        ax = dims.index(2)
        if dirichlet:          # cells on both sides of the block face, one of them with a fractional mask
            mask = np.zeros(arrays["T"].shape, order="F")
            idx = [slice(3, 6)] * nd
            idx[ax] = slice(n[ax] - 4, n[ax] + 3)
            mask[tuple(idx)] = 1.0
            idx[ax] = n[ax] - 1
            mask[tuple(idx)] = 0.5
            arrays["dirichlet_mask"] = mask
        locs = _cut(arrays, tb, nd)
        stokes = None
        if adiabatic:
            rng = np.random.default_rng(5)
            P, P0 = (np.asfortranarray(rng.uniform(1e8, 3e8, size=tb.ng[:nd])) for _ in range(2))
            stokes = list(zip(*[[B.local_block(A, tb.n, tb.ng, B.coords_of(c), nd=nd) for c in tb.carts] for A in (P, P0)]))
        res, outs, ups = _solve_blocks(jr, tb, inp, locs, form, CADENCE, dirichlet=1400.0 if dirichlet else None, stokes=stokes)
        if adiabatic:
            for r, u in enumerate(ups):       # adiabatic_heating! (DiffusionPT_kernels.jl:720-729): (P - P0) α / dt, as the device left it in thermal.adiabatic
                locs[r]["adiabatic"] = jr.to_numpy(u.thermal.adiabatic)
                want = (stokes[r][0] - stokes[r][1]) * hd.RHEOLOGY["alpha"] * (1.0 / inp.dt)
                assert np.allclose(locs[r]["adiabatic"], want, rtol=1e-14, atol=0) and np.abs(want).max() > 0
        carts = tb.carts
        if dirichlet:
            for l in locs:
                l["dirichlet_const"] = np.array(1400.0)
                assert (l["dirichlet_mask"] == 1.0).any() and (l["dirichlet_mask"] == 0.5).any()          # the mask does straddle the face
        ys = hd.yardstick_blocks(locs, inp.bc, inp._di, inp.dt, tb.n, carts, L, form, *CADENCE)
    worst = _assert_within_bounds(tag, res, outs, ys)
    if dirichlet:
        for r in range(2):
            m = locs[r]["dirichlet_mask"]
            assert (outs[r]["T"][m == 1.0] == 1400.0).all() and (outs[r]["ResT"][m[(slice(1, -1),) * nd] != 0] == 0.0).all()
    assert res[0].norm_ResT[-1] != res[1].norm_ResT[-1]          # each rank reports its own norm
    # the received ghost plane is the neighbour's sent plane (T extent n + 2: 0-based planes 3 and n - 2)
    assert np.array_equal(np.take(outs[0]["T"], -1, axis=ax), np.take(outs[1]["T"], 3, axis=ax))
    assert np.array_equal(np.take(outs[1]["T"], 0, axis=ax), np.take(outs[0]["T"], n[ax] - 2, axis=ax))
    return worst


@pytest.mark.parametrize("tag,dims,n,bc,form", CASES2D, ids=[c[0] for c in CASES2D])
def test_heat_diffusion_2d_on_two_blocks_matches_the_block_restatement(jr, tag, dims, n, bc, form):
    _run_case(jr, "2d-" + tag, dims, n, bc, form)


@pytest.mark.parametrize("dims,bc,what", [((2, 1, 1), "L3", "adiabatic"), ((1, 2, 1), "L2", "dirichlet")])
def test_heat_diffusion_2d_on_two_blocks_with_optional_terms(jr, dims, bc, what):
    """the adiabatic term (rheology form, kwargs.stokes) and a Dirichlet mask that straddles the block face (array form)"""
    _run_case(jr, f"2d-34x19-{what}", dims, (34, 19), bc, "rheology" if what == "adiabatic" else "array", adiabatic=what == "adiabatic", dirichlet=what == "dirichlet")


@pytest.mark.parametrize("tag,dims,bc,form", CASES3D, ids=[c[0] for c in CASES3D])
def test_heat_diffusion_3d_on_two_blocks_matches_the_block_restatement(jr, tag, dims, bc, form):
    """rheology form; array form with non-uniform K and constant-flux outer faces (L0: front, L2: left and top)"""
    _run_case(jr, "3d-" + tag, dims, N3D, bc, form)


@pytest.mark.parametrize("dims,bc,what", [((1, 1, 2), "L3", "adiabatic"), ((2, 1, 1), "L2", "dirichlet")])
def test_heat_diffusion_3d_on_two_blocks_with_optional_terms(jr, dims, bc, what):
    _run_case(jr, f"3d-{what}", dims, N3D, bc, "rheology" if what == "adiabatic" else "array", adiabatic=what == "adiabatic", dirichlet=what == "dirichlet")


# ------------------------------------------------------------------------------------------------ phase-ratio form against the oracle, block by block
def _phase_case(jr, oracle, tag, dims, n, bc_name, np_const):
    import torch
    import test_gpu_thermal_multiphase as tm
    from justrelax_jl_amd import _lib, halo
    from justrelax_jl_amd.arrays import from_numpy
    from justrelax_jl_amd.checks import max_rel_diff
    nd = len(n)
    L = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    iterMax, nout = CADENCE
    with B.TwoBlocks(_n3(n), dims) as tb:
        ng = tb.ng[:nd]
        s = jr.miniapps.diffusion2d_multiphase(ng) if nd == 2 else jr.miniapps.diffusion3d_multiphase(ng)
        tm._randomise(s, 17 + nd)
        rheology = s.extra["rheology"]
        inp = hd.make_inputs(ng, bc_name, hd.case_seed(tag))
        arrays = dict(inp.arrays, P=s.arrays["P"])
        arrays["shear_heating"] = s.arrays["shear_heating"]
        ratios = s.extra["phase_ratios"]
        locs, prs = _cut(arrays, tb, nd), _cut(ratios, tb, nd)
        ni = tb.n[:nd]
        with _Grid(tb.n, tb.dims):
            grid = jr.Geometry(ni, inp.li)
            assert tuple(grid._di["center"]) == tuple(inp._di)
            ups, fns = [], []
            for r, h in enumerate(tb.handles):
                h.set_option("comm_timeout_ms", TIMEOUT_MS)
                h.set_option("thermal_np_const", np_const)
                thermal = jr.ThermalArrays(jr.AMDGPUBackend, ni)
                for name in _input_names(nd):
                    getattr(thermal, name).copy_(from_numpy(locs[r][name], dev))
                pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
                for k, v in prs[r].items():
                    getattr(pr, k).copy_(from_numpy(v, dev))
                args = SimpleNamespace(P=from_numpy(locs[r]["P"], dev), T=thermal.T)
                pt = jr.PTThermalCoeffs.from_phases(jr.AMDGPUBackend, rheology, pr, args, inp.dt, ni, inp.di, inp.li, ϵ=1e-30, CFL=inp.CFL)
                bc = _device_bc(jr, inp.bc, nd)
                kw = dict(phase=pr, iterMax=iterMax, nout=nout, verbose=False)
                ups.append(SimpleNamespace(thermal=thermal, pt=pt, pr=pr, args=args, bc=bc))
                fns.append(lambda u=ups[-1], kw=kw, h=h: jr.heatdiffusion_PT_(u.thermal, u.pt, u.bc, rheology, u.args, inp.dt, grid, kwargs=kw, handle=h))
            res = halo.run_ranks(fns)
            outs = [_download(jr, u.thermal, nd) for u in ups]
            coeffs = [(jr.to_numpy(u.pt.θr_dτ), jr.to_numpy(u.pt.dτ_ρ)) for u in ups]
        carts = tb.carts
        # the oracle, block by block with the same plane copies
        mk = oracle.thermal_params3d if nd == 3 else oracle.thermal_params2d
        b = inp.bc
        p = mk(ni, inp._di, inp.dt, 1e-30, iterMax=iterMax, nout=nout, no_flux=b.no_flux, constant_value=b.constant_value, constant_flux=b.constant_flux, periodic=b.periodic)
        m = oracle.thermal_phases(list(rheology), max(inp.li), min(inp.di) * inp.CFL)
        refs = [{k: v.copy(order="F") for k, v in l.items()} for l in locs]
        phs = [dict(P=refs[r]["P"], phase_c=prs[r]["center"], phase_qx=prs[r]["Vx"], phase_qy=prs[r]["Vy"], phase_qz=prs[r].get("Vz")) for r in range(2)]
        norms = [[], []]
        for ref in refs:
            ref["Told"][...] = ref["T"]
        for it in range(1, iterMax + 1):
            for r in range(2):
                oracle.thermal_phase_iteration(refs[r], p, m, phs[r])
            B.exchange([[ref["T"]] for ref in refs], tb.n, carts, L)
            if it % nout == 0:
                for r in range(2):
                    oracle.thermal_phase_iteration(refs[r], p, m, phs[r], check_res=True)
                    norms[r].append(np.sqrt((refs[r]["ResT"] ** 2).sum()) / np.sqrt(refs[r]["ResT"].size))
        for ref in refs:
            ref["dT"][...] = ref["T"] - ref["Told"]
    worst = 0.0
    for r in range(2):
        assert list(res[r].iter_count) == list(range(nout, iterMax + 1, nout))
        d = {"norm_ResT": float(np.abs(res[r].norm_ResT / np.array(norms[r]) - 1).max())}
        for k in hd.compared_fields(nd):
            if k == "ResT":        # on the scale of the terms check_res! adds up
                scale = max(float(np.abs(refs[r][k]).max()), float(np.abs(hd._div(refs[r], inp._di, "2")).max()), float(np.abs(refs[r]["H"]).max()))
                d[k] = float(np.abs(outs[r][k] - refs[r][k]).max()) / scale
            else:
                d[k] = max_rel_diff(outs[r][k], refs[r][k])
        d["thetar_dtau"], d["dtau_rho"] = max_rel_diff(coeffs[r][0], refs[r]["thetar_dtau"]), max_rel_diff(coeffs[r][1], refs[r]["dtau_rho"])
        print(f"BLOCKCASE {tag} rank {r} max ratio {max(d.values()) / hd.TOL_ITERS:.3e}", {k: f"{v:.2e}" for k, v in d.items()})
        worst = max(worst, max(d.values()))
        assert max(d.values()) <= hd.TOL_ITERS, (tag, r, d)
    ax = dims.index(2)
    assert np.array_equal(np.take(outs[0]["T"], -1, axis=ax), np.take(outs[1]["T"], 3, axis=ax))
    assert np.array_equal(np.take(outs[1]["T"], 0, axis=ax), np.take(outs[0]["T"], n[ax] - 2, axis=ax))
    return worst


@pytest.mark.parametrize("dims,n,bc", [((2, 1, 1), (34, 19), "L2"), ((1, 2, 1), (70, 33), "L0")])
def test_heat_diffusion_2d_phase_ratios_on_two_blocks_match_the_oracle(jr, oracle, dims, n, bc):
    """two phases with randomised ratios; on unobserved iterations update_T! writes the next iteration's θr_dτ, dτ_ρ while the exchange is active"""
    _phase_case(jr, oracle, f"2d-phases-{'xy'[dims.index(2)]}", dims, n, bc, 1)


@pytest.mark.parametrize("dims,bc,np_const", [((1, 2, 1), "L1", 1), ((1, 1, 2), "L0", 0), ((2, 1, 1), "L3", 0)])
def test_heat_diffusion_3d_phase_ratios_on_two_blocks_match_the_oracle(jr, oracle, dims, bc, np_const):
    """the instantiations with the phase count as a constant (thermal_np_const = 1, the default) and the run-time loops (0)"""
    _phase_case(jr, oracle, f"3d-phases-{'xyz'[dims.index(2)]}-{np_const}", dims, N3D, bc, np_const)


# ------------------------------------------------------------------------------------------------ uniform material, one iteration, periodic self-halo
@pytest.mark.parametrize("dims,bc", [((2, 1, 1), "L0"), ((1, 2, 1), "L2")])
def test_thermal2d_two_blocks_of_a_uniform_material_equal_the_undecomposed_run(jr, dims, bc):
    """uniform K, ρCp, no constant flux on the split axis: every block equals the undecomposed device run (fused kernel, graph replays) bit for bit on the cells it owns"""
    n = (34, 19)
    with B.TwoBlocks(_n3(n), dims) as tb:
        inp = hd.make_inputs(tb.ng[:2], bc, 77)
        assert not any(hd._is_flux(v) for f, v in inp.bc.constant_flux.items() if hd.AXIS[2][f][0] == dims.index(2))
        inp.arrays["K"][...], inp.arrays["rhoCp"][...] = 3.5, 3.96e6
        with _Grid(tb.ng):
            glob = {k: v.copy(order="F") for k, v in inp.arrays.items()}
            u = _upload(jr, glob, inp.ni, inp)
            rg = jr.heatdiffusion_PT_(u.thermal, u.pt, _device_bc(jr, inp.bc, 2), u.K, u.ρCp, inp.dt, jr.Geometry(inp.ni, inp.li), kwargs=dict(iterMax=45, nout=20, verbose=False))
            want = _download(jr, u.thermal, 2)
        res, outs, _ = _solve_blocks(jr, tb, inp, _cut(inp.arrays, tb, 2), "array", CADENCE)
        carts = tb.carts
    assert list(rg.iter_count) == [20, 40] and all(list(r.iter_count) == [20, 40] for r in res)
    for r in range(2):
        for k in hd.compared_fields(2):
            w = B.local_block(want[k], tb.n, tb.ng, B.coords_of(carts[r]), nd=2)
            m = B.owned_mask(w.shape, tb.n, carts[r])
            assert np.array_equal(outs[r][k][m], w[m]), (dims, r, k, float(np.abs(outs[r][k] - w)[m].max()))
    assert res[0].norm_ResT[-1] != res[1].norm_ResT[-1]


def test_thermal2d_iteration_on_two_blocks_exchanges_the_planes(jr):
    """jrx_thermal2d_iteration with a communicator: after one iteration the received ghost column is the neighbour's sent column, bit for bit, and no BC value"""
    import torch
    from justrelax_jl_amd import halo, thermal as th
    n, dims = (34, 19), (2, 1, 1)
    with B.TwoBlocks(_n3(n), dims) as tb:
        inp = hd.make_inputs(tb.ng[:2], "L0", 78)          # right: no flux -- the BC kernel writes T[n + 1] = T[n] before the exchange replaces it
        locs = _cut(inp.arrays, tb, 2)
        with _Grid(tb.n, dims):
            grid = jr.Geometry(n, inp.li)
            ups = [_upload(jr, locs[r], n, inp) for r in range(2)]
            for h in tb.handles:
                h.set_option("comm_timeout_ms", TIMEOUT_MS)
            bc = _device_bc(jr, inp.bc, 2)
            halo.run_ranks([(lambda r=r: th.thermal_iteration_(ups[r].thermal, ups[r].pt, bc, ups[r].K, ups[r].ρCp, inp.dt, grid, handle=tb.handles[r])) for r in range(2)])
            torch.cuda.synchronize()
            T = [jr.to_numpy(u.thermal.T) for u in ups]
    assert np.array_equal(T[0][-1], T[1][3]) and np.array_equal(T[1][0], T[0][n[0] - 2])
    assert not np.array_equal(T[0][-1], T[0][-2]) and not np.array_equal(T[0][1:-1, 1:-1], locs[0]["T"][1:-1, 1:-1])


@pytest.mark.parametrize("periods", [(1, 0, 0), (0, 1, 0)])
def test_thermal2d_loop_with_a_periodic_self_halo_matches_the_restatement(jr, periods):
    """one rank that is its own neighbour along an ImplicitGlobalGrid-periodic axis: the 2D loop exchanges with itself (planes 3 -> n + 2 and n - 2 + 1 -> 1 of T, 1-based)"""
    from justrelax_jl_amd import _lib, halo
    import justrelax_jl_amd.grid as g
    n, nd = (34, 19), 2
    ax = periods.index(1)
    L = _lib.load()
    inp = hd.make_inputs(n, "L0" if ax == 0 else "L1", 79)          # value and no-flux kinds on the periodic axis: what the exchange must overwrite
    carts = halo.make_carts(_n3(n), (1, 1, 1), periods)
    h = _lib.default_handle()
    g.init_global_grid(*_n3(n), periodx=periods[0], periody=periods[1], rank=0, nprocs=1)
    try:
        halo.init_comm(h)
        h.set_option("comm_timeout_ms", TIMEOUT_MS)
        grid = jr.Geometry(n, inp.li)
        inp._di, inp.di = tuple(grid._di["center"]), tuple(grid.di["center"])          # n_g = n - 2 along the periodic axis
        loc = {k: v.copy(order="F") for k, v in inp.arrays.items()}
        u = _upload(jr, loc, n, inp)
        r = jr.heatdiffusion_PT_(u.thermal, u.pt, _device_bc(jr, inp.bc, nd), u.K, u.ρCp, inp.dt, grid, kwargs=dict(iterMax=45, nout=20, verbose=False))
        out = _download(jr, u.thermal, nd)
    finally:
        h.set_option("comm_timeout_ms", 120000)
        g.finalize_global_grid()
        g.init_global_grid(*_n3(n), rank=0, nprocs=1)
        halo.init_comm(h)          # back to a plain single-rank handle for the other tests
        g.finalize_global_grid()
    ys = hd.yardstick_blocks([loc], inp.bc, inp._di, inp.dt, _n3(n), carts, L, "array", *CADENCE)
    _assert_within_bounds(f"2d-self-halo-{'xy'[ax]}", [r], [out], ys)
    T = out["T"]
    inner = slice(1, -1)
    lo, wrapped, bc_src = (T[0, inner], T[n[0] - 2, inner], T[1, inner]) if ax == 0 else (T[inner, 0], T[inner, n[1] - 2], T[inner, 1])
    assert np.array_equal(lo, wrapped)                          # the ghost holds the wrapped interior layer ...
    v = inp.bc.constant_value["left" if ax == 0 else "bot"]
    assert v is not False and not np.array_equal(lo, 2 * v - bc_src)          # ... not the constant-value ghost the BC kernel wrote there first


# ------------------------------------------------------------------------------------------------ ranks leave together
@pytest.mark.parametrize("dims,n", [((2, 1, 1), (34, 19)), ((1, 1, 2), N3D)], ids=["2d", "3d"])
def test_ranks_leave_together_at_the_first_check_whose_maximum_is_under_eps(jr, dims, n):
    from justrelax_jl_amd import _lib
    nd = len(n)
    L = _lib.load()
    nout, checks = 2, 14
    with B.TwoBlocks(_n3(n), dims) as tb:
        inp = hd.make_inputs(tb.ng[:nd], "L0", 80 + nd)
        inp.bc = hd.converging_bcs(nd)
        locs = _cut(inp.arrays, tb, nd)
        locs[1]["T"][...] += np.random.default_rng(4).uniform(-200.0, 200.0, locs[1]["T"].shape)          # block 1 only: the local norms differ
        B.exchange([[l["T"]] for l in locs], tb.n, tb.carts, L)
        fresh = lambda: [{k: v.copy(order="F") for k, v in l.items()} for l in locs]
        host_in = fresh()          # the uploads of the first run leave the device's θr_dτ, dτ_ρ in these
        long, _, _ = _solve_blocks(jr, tb, inp, host_in, "array", (nout * checks, nout))
        eps, first_min, first_max = hd.eps_between(long[0].norm_ResT, long[1].norm_ResT, start=3)
        print("LEAVE", nd, "eps", eps, "first check with min <= eps", first_min, "with max <= eps", first_max, [list(r.norm_ResT) for r in long])
        stop = nout * (first_max + 1)
        short, outs, _ = _solve_blocks(jr, tb, inp, fresh(), "array", (nout * checks, nout), eps=eps)
        cut, outs_cut, _ = _solve_blocks(jr, tb, inp, fresh(), "array", (stop, nout))          # the long run stopped there
        carts = tb.carts
        run = lambda rule: hd.heatdiffusion_PT_blocks([hd.as_dtype(b, np.float64) for b in host_in], inp.bc, inp._di, inp.dt, tb.n, carts, L, iterMax=nout * checks, nout=nout,
                                                      eps=eps, stop=rule)
        host_max, host_local = run("max"), run("local")
    for r in range(2):
        assert list(long[r].iter_count) == list(range(nout, nout * checks + 1, nout))
        assert list(short[r].iter_count) == list(range(nout, stop + 1, nout)), (r, list(short[r].iter_count), stop)
        assert list(short[r].norm_ResT) == list(long[r].norm_ResT[: first_max + 1])          # the local norm, bit for bit
        assert list(cut[r].norm_ResT) == list(short[r].norm_ResT)
        for k in hd.compared_fields(nd):
            assert np.array_equal(outs[r][k], outs_cut[r][k]), (r, k)
        assert host_max[r]["iterations"] == stop and list(host_max[r]["iter_count"]) == list(short[r].iter_count)
    ax = dims.index(2)          # the ranks did exchange up to the iteration they left at: the received ghost planes are the neighbour's sent planes
    assert np.array_equal(np.take(outs[0]["T"], -1, axis=ax), np.take(outs[1]["T"], 3, axis=ax))
    assert np.array_equal(np.take(outs[1]["T"], 0, axis=ax), np.take(outs[0]["T"], n[ax] - 2, axis=ax))
    assert short[0].norm_ResT[-1] != short[1].norm_ResT[-1] and max(short[0].norm_ResT[-1], short[1].norm_ResT[-1]) <= eps
    assert host_local[0]["iterations"] != host_local[1]["iterations"]          # the reference's own rule would have let one rank go at an earlier check
