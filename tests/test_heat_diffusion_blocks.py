"""The block-by-block heat-diffusion restatement (tests/_heat_diffusion.py: heatdiffusion_PT_blocks) pinned on the host before any kernel is compared with it.

  * uniform K and ρCp (so θr_dτ, dτ_ρ are uniform too): the clamped face averages on a block face take the same number twice, nothing a block computes differs from what
    the undecomposed grid computes there, and the float64 blocks must equal the cut-outs of the undecomposed float64 restatement bit for bit on the cells each block owns
    (_blocks.owned_mask), 2D and 3D, array and rheology form, split along every axis.  The faces of the split axis take no constant flux: the reference writes a constant-flux
    value on the face of the LOCAL array (DiffusionPT_kernels.jl:29-41, :344-356), which on a block face is an interior face of the global grid.
  * non-uniform K: the blocks do differ from the cut-outs (the clamped averages), so the GPU tests have to compare with the blocks, not with the undecomposed run.
  * the stop rule: with "local" the ranks leave at different checks, with "max" at the later of the two, together."""
import numpy as np
import pytest

import _blocks as B
import _heat_diffusion as hd

# (dims, local block, BCs without a constant flux on the split axis: L0 = left V, right N, [front F, back O,] top F | V, bot O | N; L2 = left F, right O, ...)
CASES = [((2, 1, 1), (9, 6), "L0", "array"), ((1, 2, 1), (7, 8), "L2", "rheology"), ((2, 1, 1), (3, 2), "L0", "rheology"), ((1, 2, 1), (2, 3), "L2", "array"),
         ((2, 1, 1), (8, 5, 6), "L0", "rheology"), ((1, 2, 1), (6, 7, 5), "L2", "array"), ((1, 1, 2), (5, 6, 7), "L0", "array")]


def _setup(jr, dims, n, bc, uniform, seed=7):
    from justrelax_jl_amd import _lib, halo
    from justrelax_jl_amd.miniapps.thermal2d import pt_thermal_coeffs_np
    nd = len(n)
    n3 = tuple(n) + (1,) * (3 - nd)
    carts = halo.make_carts(n3, dims)
    ng = B.n_global(n3, dims)
    inp = hd.make_inputs(ng[:nd], bc, seed)
    a = inp.arrays
    if uniform:
        a["K"][...], a["rhoCp"][...] = 3.5, 3.96e6
    a["thetar_dtau"][...], a["dtau_rho"][...] = pt_thermal_coeffs_np(a["K"], a["rhoCp"], inp.dt, inp.di, inp.li, inp.CFL)
    blocks = [{k: B.local_block(v, n3, ng, B.coords_of(carts[r]), nd=nd) for k, v in a.items()} for r in range(len(carts))]
    return inp, carts, n3, ng, blocks, _lib.load()


@pytest.mark.parametrize("dims,n,bc,form", CASES, ids=[f"{'x'.join(map(str, c[1]))}-{'xyz'[c[0].index(2)]}-{c[3]}" for c in CASES])
def test_uniform_blocks_equal_the_cut_outs_of_the_undecomposed_restatement(jr, dims, n, bc, form):
    nd = len(n)
    inp, carts, n3, ng, blocks, L = _setup(jr, dims, n, bc, True)
    ax = dims.index(2)
    assert not any(hd._is_flux(v) for f, v in inp.bc.constant_flux.items() if hd.AXIS[nd][f][0] == ax)
    rheo = hd.RHEOLOGY if form == "rheology" else None
    fg = hd.as_dtype(inp.arrays, np.float64)
    rg = hd.heatdiffusion_PT(fg, inp.bc, inp._di, inp.dt, iterMax=45, nout=20, rheology=rheo)
    fs = [hd.as_dtype(b, np.float64) for b in blocks]
    rs = hd.heatdiffusion_PT_blocks(fs, inp.bc, inp._di, inp.dt, n3, carts, L, iterMax=45, nout=20, rheology=rheo)
    assert list(rg["iter_count"]) == [20, 40]
    for r in range(2):
        assert list(rs[r]["iter_count"]) == [20, 40] and rs[r]["iterations"] == 45
        for k in hd.compared_fields(nd):
            want = B.local_block(fg[k], n3, ng, B.coords_of(carts[r]), nd=nd)
            m = B.owned_mask(want.shape, n3, carts[r])
            assert m.any() and np.array_equal(fs[r][k][m], want[m]), (r, k, float(np.abs(fs[r][k] - want)[m].max()))
        # the received ghost plane is the neighbour's sent plane
        sl, sr = (3, n[ax] - 2)
        other = fs[1 - r]["T"]
        mine = np.take(fs[r]["T"], -1 if r == 0 else 0, axis=ax)
        assert np.array_equal(mine, np.take(other, sl if r == 0 else sr, axis=ax))
    assert rs[0]["norm_ResT"][-1] != rs[1]["norm_ResT"][-1]


def test_blocks_with_varying_conductivity_are_not_the_cut_outs(jr):
    """the face average of K, θr_dτ is clamped to the local block (DiffusionPT_kernels.jl:331-340): the overlap cells of a block see one cell twice"""
    dims, n = (2, 1, 1), (9, 6)
    inp, carts, n3, ng, blocks, L = _setup(jr, dims, n, "L0", False)
    fg = hd.as_dtype(inp.arrays, np.float64)
    hd.heatdiffusion_PT(fg, inp.bc, inp._di, inp.dt, iterMax=45, nout=20)
    fs = [hd.as_dtype(b, np.float64) for b in blocks]
    hd.heatdiffusion_PT_blocks(fs, inp.bc, inp._di, inp.dt, n3, carts, L, iterMax=45, nout=20)
    d = max(np.abs(fs[r]["T"] - B.local_block(fg["T"], n3, ng, B.coords_of(carts[r]), nd=2)).max() for r in range(2))
    assert d > 1e-6 * np.abs(fg["T"]).max()


def test_stop_rule_local_and_maximum(jr):
    dims, n = (2, 1, 1), (9, 6)
    inp, carts, n3, ng, blocks, L = _setup(jr, dims, n, "L0", True)
    inp.bc = hd.converging_bcs(2)
    blocks[1]["T"][...] += np.random.default_rng(1).uniform(-200.0, 200.0, blocks[1]["T"].shape)
    B.exchange([[b["T"]] for b in blocks], n3, carts, L)
    run = lambda eps, stop: hd.heatdiffusion_PT_blocks([hd.as_dtype(b, np.float64) for b in blocks], inp.bc, inp._di, inp.dt, n3, carts, L, iterMax=40, nout=2, eps=eps, stop=stop)
    long = run(0.0, "max")
    eps, first_min, first_max = hd.eps_between(long[0]["norm_ResT"], long[1]["norm_ResT"])
    rmax, rloc = run(eps, "max"), run(eps, "local")
    assert rmax[0]["iterations"] == rmax[1]["iterations"] == 2 * (first_max + 1)
    for r in range(2):
        assert list(rmax[r]["norm_ResT"]) == list(long[r]["norm_ResT"][: first_max + 1])
    assert min(rloc[0]["iterations"], rloc[1]["iterations"]) == 2 * (first_min + 1) < max(rloc[0]["iterations"], rloc[1]["iterations"])
