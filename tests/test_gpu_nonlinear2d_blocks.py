"""GPU: the single-phase visco-elasto-plastic 2D driver (jrx_stokes2d_nonlinear_solve; solve!(stokes, pt_stokes, grid, flow_bcs, ρg, rheology::MaterialParams, args, dt, igg),
Stokes2D.jl:345-557) on a handle that carries a communicator: update_halo!(ητ) (:440), update_halo!(stokes.τ.xy) (:460) and update_halo!(@velocity(stokes)...) (:477) in every
iteration, norm_mpi over the global counts, no graph replay.  (The update_halo!(ητ) of :417 follows a compute_maxloc! that :439 repeats before anybody reads ητ; neither the
library nor the oracle runs it.)

  * periodic self-halo against the oracle: one rank that is its own neighbour along x, the T-dependent Arrhenius viscosity and the regularised Drucker-Prager of
    test_gpu_vep_extras.test_single_phase_driver_matches_oracle on a 40 x 23 grid; the oracle's driver makes the same plane copies (orc_set_self_halo); tolerance 1e-8 as there.
  * two blocks, split along x and along y: a material whose viscosity does not depend on position, pre-stressed so that cells yield.  center2vertex! puts an edge copy on the
    block face, which update_halo!(τ.xy) replaces with the neighbour's interior value; every block equals the undecomposed device run bit for bit on the state arrays.  The
    ranks hold the same err_evo1 bits and stop at the undecomposed run's iteration count.  err_evo1 itself need not be the undecomposed number: norm_mpi sums the local
    slices R.Rx[2:end-1, 2:end-1], R.Ry[2:end-1, 2:end-1] and the whole local R.RP (Stokes2D.jl:495-501), so the overlap cells of RP count twice and the rows of Rx, Ry next
    to a block face count twice or not at all -- it is checked against that sum taken from the undecomposed residuals, norm by norm; the one norm whose slices tile
    the global interior exactly (Ry split along x, Rx split along y) must be the undecomposed run's at every check.  Vx, Vy are compared whole but for their four corner entries,
    and the planes received by the three exchanges' arrays (τ.xy, Vx, Vy) against the neighbour's sent planes.

Seen on the MI355X: periodic self-halo against the oracle at most 4.7e-11 (η_vep; bound 1e-8); the three tests take about 3 s."""
import numpy as np
import pytest

import _blocks as B

pytestmark = pytest.mark.gpu
TIMEOUT_MS = 5000


def test_nonlinear_solve_with_periodic_halo_matches_oracle(jr, oracle):
    import torch
    import justrelax_jl_amd.grid as g
    from justrelax_jl_amd import _lib, halo
    from justrelax_jl_amd.arrays import from_numpy
    from justrelax_jl_amd.checks import max_rel_diff
    from test_gpu_vep2d import VEP_MAP, _get
    from test_gpu_vep_extras import _cp, _nl_params
    L = oracle.lib()
    n, periods = (40, 23), (1, 0, 0)
    s = jr.miniapps.thermal_convection2d(n, ar=1, iterMax=299, nout=100)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-300
    ph = dict(s.extra["rheology"])
    ph.update(C=8.0e6, phi_deg=0.0, psi_deg=0.0, eta_vp=1.0e16)
    dev = torch.device("cuda", torch.cuda.current_device())
    g.init_global_grid(n[0], n[1], 1, periodx=1, rank=0, nprocs=1)
    ng = tuple(g.global_grid().n_g(d) for d in range(2))
    assert ng == (38, 23)
    h = _lib.default_handle()
    try:
        halo.init_comm(h)
        h.set_option("comm_timeout_ms", TIMEOUT_MS)
        st = jr.StokesArrays(jr.AMDGPUBackend, s.ni)
        for k, path in VEP_MAP.items():
            _get(st, path).copy_(from_numpy(s.arrays[k], dev))
        ρg = (from_numpy(s.arrays["fx"], dev), from_numpy(s.arrays["fy"], dev))
        T = from_numpy(s.arrays["T"], dev)
        r = jr.solve_(st, s.pt, s.grid, s.flow_bcs, ρg, ph, dict(T=T, P=st.P), s.dt, None, kwargs=s.kwargs)
        out = {k: jr.to_numpy(_get(st, path)) for k, path in VEP_MAP.items()}
    finally:
        h.set_option("comm_timeout_ms", 120000)
        g.finalize_global_grid()
        g.init_global_grid(n[0], n[1], 1, rank=0, nprocs=1)
        halo.init_comm(h)          # back to a plain single-rank handle for the other tests
        g.finalize_global_grid()
    ref = _cp(s.arrays)
    L.orc_set_self_halo(*periods)
    try:
        r_ref = oracle.stokes2d_nonlinear_solve(ref, oracle.rheology_struct([ph]), _nl_params(oracle, s, ni_g=ng))
    finally:
        L.orc_set_self_halo(0, 0, 0)
    plain = _cp(s.arrays)
    oracle.stokes2d_nonlinear_solve(plain, oracle.rheology_struct([ph]), _nl_params(oracle, s))
    assert max_rel_diff(plain["Vx"], ref["Vx"]) > 1e-6          # the plane copies do change the answer: the comparison below can tell
    assert r.iter == r_ref["iter"] == 300
    assert np.allclose(r.err_evo1, r_ref["err_evo1"], rtol=1e-8)
    assert (ref["eplxx"] != 0).any()
    worst = {k: max_rel_diff(out[k], ref[k]) for k in out}
    print("NONLINEAR self-halo, largest relative differences:", {k: f"{v:.1e}" for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:5]})
    for k, v in worst.items():
        assert v <= 1e-8, (k, v)
    # the x ghost column of Vy holds the wrapped interior column (Vy extent nx + 2: 0-based planes nx - 2 -> 0)
    assert np.array_equal(out["Vy"][0], out["Vy"][n[0] - 2])


@pytest.mark.parametrize("dims", [(2, 1, 1), (1, 2, 1)])
def test_nonlinear_two_blocks_equal_the_undecomposed_run(jr, dims):
    import test_gpu_vep2d as tv
    import justrelax_jl_amd.grid as g
    from justrelax_jl_amd import halo
    from justrelax_jl_amd.miniapps.common import Setup
    n = (34, 66, 1) if dims[0] == 2 else (66, 34, 1)            # a square 66 x 66 global grid either way
    kw = dict(iterMax=29, nout=10, verbose=False, viscosity_cutoff=(-np.inf, np.inf))
    with B.TwoBlocks(n, dims) as tb:
        ng = tb.ng
        assert ng[:2] == (66, 66)
        S = jr.miniapps.shearband2d(66, iterMax=29, nout=10)
        S.pt.ϵ_rel = S.pt.ϵ_abs = 1e-30
        ph = dict(S.extra["phases"][0])          # LinearViscous η = 1 everywhere, G, Kb, regularised Drucker-Prager
        S.arrays["phase_c"][0], S.arrays["phase_c"][1] = 1.0, 0.0
        S.arrays["phase_v"][0], S.arrays["phase_v"][1] = 1.0, 0.0
        rng = np.random.default_rng(13)
        for c in ("xx", "yy", "xy", "xy_c"):          # pre-stress close to yield
            S.arrays["to" + c][...] = rng.uniform(-1.5, 1.5, size=S.arrays["to" + c].shape)
            S.arrays["t" + c][...] = S.arrays["to" + c]
        stokes, _, ρg = tv._upload(jr, S)
        rg = jr.solve_(stokes, S.pt, S.grid, S.flow_bcs, ρg, ph, dict(P=stokes.P), S.dt, None, kwargs=kw)
        glob = tv._download(jr, stokes)
        g.init_global_grid(*n, dimx=dims[0], dimy=dims[1], dimz=1, rank=0, nprocs=2)
        try:
            grid = jr.Geometry(n[:2], (1.0, 1.0))
            ups = []
            for r in range(2):
                tb.handles[r].set_option("comm_timeout_ms", TIMEOUT_MS)
                loc = Setup(ni=n[:2], arrays={k: B.local_block(v, n, ng, B.coords_of(tb.carts[r]), nd=2) for k, v in S.arrays.items()})
                ups.append(tv._upload(jr, loc))
            res = halo.run_ranks([(lambda r=r: jr.solve_(ups[r][0], S.pt, grid, S.flow_bcs, ups[r][2], ph, dict(P=ups[r][0].P), S.dt, None, kwargs=kw,
                                                         handle=tb.handles[r])) for r in range(2)])
            outs = [tv._download(jr, u[0]) for u in ups]
        finally:
            g.finalize_global_grid()
        carts = tb.carts
    assert rg.iter == res[0].iter == res[1].iter == 30
    assert list(res[0].err_evo1) == list(res[1].err_evo1) and len(res[0].err_evo1) == len(rg.err_evo1) == 3
    assert list(res[0].err_evo2) == list(res[1].err_evo2) == list(rg.err_evo2)
    assert (glob["eplxx"] != 0).any() and (glob["eplxx"] == 0).any()
    for r in range(2):
        for k in ("P", "txx", "tyy", "txy", "txy_c", "tII", "eta_vep", "eta", "exx", "eyy", "eplxx", "Rx", "Ry", "RP"):
            want = B.local_block(glob[k], n, ng, B.coords_of(carts[r]), nd=2)
            d = np.abs(outs[r][k] - want)
            bad = np.argwhere(d > 0)
            assert np.array_equal(outs[r][k], want), (dims, r, k, float(d.max()), want.shape, bad[:6].tolist(), bad[-3:].tolist(), len(bad))
        for k in ("Vx", "Vy"):          # whole arrays, received planes and BC ghosts included; only the four corner entries, which nobody reads, are left out
            want = B.local_block(glob[k], n, ng, B.coords_of(carts[r]), nd=2)
            m = np.ones(want.shape, dtype=bool)
            for i in (0, -1):
                for j in (0, -1):
                    m[i, j] = False
            d = np.abs(outs[r][k] - want)
            assert np.array_equal(outs[r][k][m], want[m]), (dims, r, k, float(d[m].max()), np.argwhere((d > 0) & m)[:8].tolist())
    # the third exchange: the received plane of V is the neighbour's sent plane, whole (jrx_halo_planes names them: Vx (nx + 1, ny + 2), Vy (nx + 2, ny + 1))
    import ctypes as C
    from justrelax_jl_amd import _lib
    L = _lib.load()
    ax = dims.index(2)
    for k in ("Vx", "Vy", "txy"):
        sl, sr, rl, rr = (C.c_int64() for _ in range(4))
        assert L.jrx_halo_planes(C.c_int64(n[ax]), C.c_int64(outs[0][k].shape[ax]), C.byref(sl), C.byref(sr), C.byref(rl), C.byref(rr)) == 0
        assert np.array_equal(np.take(outs[0][k], rr.value, axis=ax), np.take(outs[1][k], sl.value, axis=ax)), (dims, k, "rank 0 high plane")
        assert np.array_equal(np.take(outs[1][k], rl.value, axis=ax), np.take(outs[0][k], sr.value, axis=ax)), (dims, k, "rank 1 low plane")
        assert not np.array_equal(np.take(outs[0][k], rr.value, axis=ax), np.take(outs[0][k], rr.value - 1, axis=ax)), k
    # norm_mpi: Σ over the ranks of the local slices over the global counts, from the undecomposed residuals (the last check)
    ss = np.zeros(3)
    for r in range(2):
        loc = {k: B.local_block(glob[k], n, ng, B.coords_of(carts[r]), nd=2) for k in ("Rx", "Ry", "RP")}
        ss += [np.sum(loc["Rx"][1:-1, 1:-1] ** 2), np.sum(loc["Ry"][1:-1, 1:-1] ** 2), np.sum(loc["RP"] ** 2)]
    cnt = [(ng[0] - 2) * (ng[1] - 1), (ng[0] - 1) * (ng[1] - 2), ng[0] * ng[1]]
    want = [np.sqrt(ss[q]) / np.sqrt(cnt[q]) for q in range(3)]
    got = [res[0].norm_Rx[-1], res[0].norm_Ry[-1], res[0].norm_divV[-1]]
    print("NONLINEAR two blocks", dims, "norms", got, "norm_mpi of the undecomposed residuals", want, "undecomposed run", rg.err_evo1[-1])
    assert np.allclose(got, want, rtol=1e-12, atol=0), (got, want)
    assert np.isclose(res[0].err_evo1[-1], max(want), rtol=1e-12)
    # every check: split along x the slices of Ry (local columns 2:end-1 = global 2:33 and 34:65), split along y those of Rx, tile the global interior exactly, so that
    # norm is the undecomposed run's at every check (summed in another order: 1e-12)
    tiled = "norm_Ry" if ax == 0 else "norm_Rx"
    for r in range(2):
        assert list(getattr(res[r], tiled)) == list(getattr(res[0], tiled))
        assert np.allclose(getattr(res[r], tiled), getattr(rg, tiled), rtol=1e-12, atol=0), (dims, tiled, getattr(res[r], tiled), getattr(rg, tiled))
