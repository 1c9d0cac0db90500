"""GPU: compute_lithostatic_pressure!(P, ρg, dz, igg) on a handle that carries a communicator (csrc/gridops.hip).  The reference's IGG form (src/Utils.jl:575-640) gathers
the weight of the ranks above; the library builds the case in which no rank is above another: a horizontal split is a plain column integration per block, a split of the
vertical direction (the last one: y in 2D, z in 3D) is refused with JRX_ERR_UNSUPPORTED before anything is written.  The call exchanges nothing, so the ranks are called in turn.
The four tests take 0.3 s on the MI355X."""
import numpy as np
import pytest

import _blocks as B

pytestmark = pytest.mark.gpu


def _up(a):
    import torch
    from justrelax_jl_amd.arrays import from_numpy
    return from_numpy(a, torch.device("cuda", torch.cuda.current_device()))


@pytest.mark.parametrize("n", [(34, 19, 1), (24, 13, 12)], ids=["2d", "3d"])
def test_lithostatic_pressure_on_blocks_split_along_x_equals_the_cut_outs(jr, n):
    nd = 2 if n[2] == 1 else 3
    rng = np.random.default_rng(31)
    with B.TwoBlocks(n, (2, 1, 1)) as tb:
        ng = tb.ng[:nd]
        rhog = np.asfortranarray(rng.uniform(2.0e4, 3.5e4, size=ng))
        dz = rng.uniform(0.5, 1.5, size=ng[-1])
        for heights in (0.75, dz):
            Pg = jr.fzeros(ng, _up(rhog).device)
            jr.compute_lithostatic_pressure_(Pg, _up(rhog), heights)          # the plain handle: no communicator
            want = jr.to_numpy(Pg)
            assert want.min() > 0 and np.ptp(want[:, ..., 0]) > 0
            for r, h in enumerate(tb.handles):
                co = B.coords_of(tb.carts[r])
                loc = B.local_block(rhog, n, tb.ng, co, nd=nd)
                P = _up(np.full(loc.shape, -7.0, order="F"))
                jr.compute_lithostatic_pressure_(P, _up(loc), heights, handle=h)
                assert np.array_equal(jr.to_numpy(P), B.local_block(want, n, tb.ng, co, nd=nd)), (nd, r)


@pytest.mark.parametrize("n,dims", [((34, 19, 1), (1, 2, 1)), ((24, 13, 12), (1, 1, 2))], ids=["2d", "3d"])
def test_lithostatic_pressure_refuses_a_split_of_the_vertical_direction(jr, n, dims):
    from justrelax_jl_amd import _lib
    nd = 2 if n[2] == 1 else 3
    with B.TwoBlocks(n, dims) as tb:
        for h in tb.handles:
            rhog = _up(np.full(n[:nd], 3.0e4, order="F"))
            P = _up(np.full(n[:nd], -7.0, order="F"))
            with pytest.raises(_lib.JrxError) as e:
                jr.compute_lithostatic_pressure_(P, rhog, 1.0, handle=h)
            assert e.value.status == 5 and "vertical direction is split" in str(e.value)          # JRX_ERR_UNSUPPORTED
            assert (jr.to_numpy(P) == -7.0).all()          # nothing written
    # the same blocks split along x are accepted (the refusal is about the direction, not about having a communicator)
    with B.TwoBlocks(n, (2, 1, 1)) as tb:
        P = _up(np.full(n[:nd], -7.0, order="F"))
        jr.compute_lithostatic_pressure_(P, _up(np.full(n[:nd], 3.0e4, order="F")), 1.0, handle=tb.handles[1])
        assert (jr.to_numpy(P) > 0).all()
