"""GPU tests in the upper half of the 32-bit byte-offset range.

The z-marching sweeps and the fused PT kernel of 3D Stokes, and the one-launch batch form k_fused2d_b of 2D Stokes, address with
`(const char *)p + u32 offset`.  Below the blocks used here no test reaches a byte offset of 2^31.  tests/_large_shapes.py names the
shapes and pins (on the CPU) that even their smallest array is past 2 GiB and that each sits on the intended side of its guard.

  1. cross-form parity: the same random state, the same iterations, through the fused pipeline, the z-marching sweeps and the per-node
     kernels (i64 indices; the ones the oracle checks at small sizes): equal states, residuals, ∇V and ε;
  2. the translated blob: a state the iteration leaves exactly zero, with random values in a box at the high corner (the largest offset
     of every array) and in a box straddling the planes where the byte offsets cross 2^31.  The stencil is translation invariant and
     nothing in these iterations reads a grid-wide reduction except the stopping test (ϵ is set so that it never stops the run; ητ is the
     local maximum of a uniform η; the operand pass only picks the kernel form, the same one on both grids), so after `it` iterations
     the region around each box must equal the same box run on a small grid -- itself checked against the CPU oracle -- and every entry
     outside those regions must be exactly zero (a wrapped store lands there).  This is the check that does not trust any form.

Each test runs on its own handle, frees what it allocated and records its device-memory peak and wall time in build/large_offsets_gpu.txt
(untracked; profiles/large_offsets_gpu.txt holds a recorded copy)."""
import gc
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import _large_shapes as L

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PROFILE = ROOT / "build" / "large_offsets_gpu.txt"
ITER_MAX, NOUT, IT = L.ITER_MAX, L.NOUT, L.IT     # observed: iterations 4 and 7; fused steps: 1, 2 and 5 (an odd number: the state ends in the second set)
_profile_started = []
DI3 = (2.0 ** -10, 2.0 ** -9, 2.0 ** -10)      # powers of two: li / ni gives back exactly these spacings on both grids
DI2 = (2.0 ** -10, 2.0 ** -9)
TOL_ORACLE = 1e-9                    # tests/test_gpu_stokes3d.py TOL_ITERS: the drivers against the oracle after tens of iterations
FACES3 = ("left", "right", "front", "back", "top", "bot")
FACES2 = ("left", "right", "top", "bot")


@pytest.fixture
def big(jr, request):
    """its own handle; afterwards every array is gone and free device memory is back within 1 GiB of where the test started"""
    import torch
    from justrelax_jl_amd import _lib
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    torch.cuda.reset_peak_memory_stats()
    rec = SimpleNamespace(peak=0, limit=L.BUDGET_BYTES, t0=time.time(), h=_lib.Handle(torch.cuda.current_device()), free0=free0)

    def sample():
        torch.cuda.synchronize()
        rec.peak = max(rec.peak, free0 - torch.cuda.mem_get_info()[0])

    def need(nbytes):
        rec.limit = L.VEP3_BUDGET_BYTES if nbytes > L.BUDGET_BYTES else L.BUDGET_BYTES
        if free0 < nbytes:
            pytest.skip(f"the device reports {free0 / 1e9:.1f} GB free; this test counts {nbytes / 1e9:.1f} GB")

    rec.sample, rec.need = sample, need
    yield rec
    rec.h.close()
    import justrelax_jl_amd.grid as g
    g.finalize_global_grid()                       # no grid state of these sizes for later files
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info()
    PROFILE.parent.mkdir(exist_ok=True)
    with open(PROFILE, "a" if _profile_started else "w") as fh:          # one record per session
        _profile_started.append(1)
        fh.write(f"{request.node.name}: peak device memory {rec.peak / 1e9:.1f} GB (torch max_memory_allocated {torch.cuda.max_memory_allocated() / 1e9:.1f} GB), "
                 f"{time.time() - rec.t0:.1f} s\n")
    assert rec.peak <= rec.limit, rec.peak
    assert free1 >= free0 - L.GiB, (free0, free1)


def _bcs(nd):
    from justrelax_jl_amd.arrays import VelocityBoundaryConditions
    faces = FACES3 if nd == 3 else FACES2
    return VelocityBoundaryConditions(free_slip={f: True for f in faces}, no_slip={f: False for f in faces})


def _geometry(ni, di):
    import justrelax_jl_amd.grid as g
    li = tuple(n * d for n, d in zip(ni, di))
    g.init_global_grid(*ni)
    return g.Geometry(ni, li)


def _pt(ni, di):
    """the PT coefficients of the LARGE grid, used on both grids (PTStokesCoeffs derives them from li)"""
    from justrelax_jl_amd.arrays import PTStokesCoeffs
    pt = PTStokesCoeffs(tuple(n * d for n, d in zip(ni, di)), di)
    pt.ϵ_rel = pt.ϵ_abs = 1e-300
    return pt


def _paths(nd):
    from justrelax_jl_amd.miniapps.common import stokes_field_names
    return stokes_field_names(nd)


def _arrays(jr, st, ρg, K, G):
    """name -> device array (the names of alloc_stokes)"""
    from justrelax_jl_amd.miniapps.common import _get
    nd = len(st._ni)
    out = {k: _get(st, p) for k, p in _paths(nd).items()}
    out.update(K=K, G=G, **dict(zip(("fx", "fy", "fz")[:nd], ρg)))
    return out


def _checked(nd):
    if nd == 3:
        return ("P", "txx", "tyy", "tzz", "tyz", "txz", "txy", "Vx", "Vy", "Vz", "RP", "Rx", "Ry", "Rz", "divV", "exx", "eyy", "ezz", "eyz", "exz", "exy")
    return ("P", "txx", "tyy", "txy", "Vx", "Vy", "RP", "Rx", "Ry", "divV", "exx", "eyy", "exy")


def _observed(name, shape):
    """entries every kernel form must agree on: all but the entries of V that are ghost in two directions (their values depend on the order of the
    boundary-condition launches, checks.interior_mask3d)"""
    from justrelax_jl_amd import checks
    if len(shape) == 3:
        return checks.interior_mask3d(name, shape)
    return np.ones(shape, dtype=bool)


def _observable(name, t):
    """the same entries as views of a device array (tests/test_gpu_fullsize.py)"""
    tang = {"Vx": (1, 2), "Vy": (0, 2), "Vz": (0, 1)}.get(name)
    if tang is None:
        return [t]
    inner = [slice(None)] * 3
    for d in tang:
        inner[d] = slice(1, -1)
    out = [t[tuple(inner)]]
    for d in tang:
        for e in (0, -1):
            idx = list(inner)
            idx[d] = e
            out.append(t[tuple(idx)])
    return out


def _ss(r, ni):
    """undo the size normalisation of the residual norms (3D: sqrt(Σx²) / count, Stokes3D.jl; 2D: sqrt(Σx²) / sqrt(count), Stokes2D.jl): Σx² per observation"""
    if len(ni) == 3:
        nx, ny, nz = ni
        cnt = {"norm_Rx": (nx - 2) * (ny - 1) * (nz - 1), "norm_Ry": (nx - 1) * (ny - 2) * (nz - 1), "norm_Rz": (nx - 1) * (ny - 1) * (nz - 2), "norm_divV": nx * ny * nz}
        return {k: (np.asarray(getattr(r, k)) * c) ** 2 for k, c in cnt.items()}
    nx, ny = ni
    cnt = {"norm_Rx": (nx - 2) * (ny - 1), "norm_Ry": (nx - 1) * (ny - 2), "norm_divV": nx * ny}
    return {k: np.asarray(getattr(r, k)) ** 2 * c for k, c in cnt.items()}


def _solve(jr, st, pt, grid, bcs, ρg, K, G, dt, h):
    kw = dict(iterMax=ITER_MAX, nout=NOUT, verbose=False)
    if len(st._ni) == 3:
        return jr.solve_(st, pt, grid, bcs, ρg, K, G, dt, None, kwargs=kw, handle=h)
    return jr.solve_(st, pt, grid, bcs, ρg, G, K, dt, None, kwargs=kw, handle=h)          # 2D order: G, K


def _counters(h, keys):
    return [h.get_option(k) for k in keys]


# ------------------------------------------------------------------------------------------------------------------------------ 1. parity

def _fill(t, gen, lo, hi):
    import torch
    flat = torch.empty(t.numel(), device=t.device, dtype=torch.float64)
    flat.uniform_(lo, hi, generator=gen)
    t.copy_(flat.view(*reversed(t.shape)).permute(*range(t.dim() - 1, -1, -1)))
    del flat


def _random_state(a, nd, seed):
    import torch
    gen = torch.Generator(device=a["P"].device)
    gen.manual_seed(seed)
    names = ("P", "Vx", "Vy", "Vz", "txx", "tyy", "tzz", "tyz", "txz", "txy") if nd == 3 else ("P", "Vx", "Vy", "txx", "tyy", "txy")
    for k in names:
        _fill(a[k], gen, -1.0, 1.0)


def _random_operands(a, nd, seed, forces):
    import torch
    gen = torch.Generator(device=a["P"].device)
    gen.manual_seed(seed)
    comps = ("xx", "yy", "zz", "yz", "xz", "xy") if nd == 3 else ("xx", "yy", "xy")
    for k in ("P0",) + tuple("to" + c for c in comps):
        _fill(a[k], gen, -1.0, 1.0)
    _fill(a["Q"], gen, -0.1, 0.1)
    _fill(a["eta"], gen, -3.0, 0.0)
    a["eta"].copy_(10.0 ** a["eta"])
    _fill(a["K"], gen, 2.0, 3.0)
    _fill(a["G"], gen, 1.0, 1.5)
    fs = ("fx", "fy", "fz")[:nd]
    for k in fs:
        a[k].zero_()
    for k in forces:
        _fill(a[k], gen, -1.0, 1.0)


CASES3 = [("inf", float("inf"), ()), ("inf_fz", float("inf"), ("fz",)), ("finite", 0.25, ("fx", "fy", "fz"))]


@pytest.mark.parametrize("case,dt,forces", CASES3, ids=[c[0] for c in CASES3])
def test_3d_kernel_forms_agree_past_2_gib(jr, big, case, dt, forces):
    """(770, 598, 610): fused pipeline (kernel_variant 3) = z-marching sweeps (2) = per-node kernels (1).  dt = Inf with ρg = +0.0: the viscous-limit
    form without body-force loads (NOF = 2); dt = Inf with ρg_z only: NOF = 1; finite dt with every force: the general form"""
    import torch
    ni = L.HIGH3
    big.need(L.stokes3_budget())
    dev = torch.device("cuda", torch.cuda.current_device())
    h = big.h
    grid, pt, bcs = _geometry(ni, DI3), _pt(ni, DI3), _bcs(3)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    K, G = jr.fzeros(ni, dev), jr.fzeros(ni, dev)
    ρg = tuple(jr.fzeros(ni, dev) for _ in range(3))
    a = _arrays(jr, st, ρg, K, G)
    names = _checked(3)
    keys = ("stat_fused3d", "stat_fused3d_visc", "stat_fused3d_nof1", "stat_fused3d_nof2", "stat_sweeps3d")
    keep, runs = None, []
    try:
        for variant in (3, 2, 1):
            _random_operands(a, 3, 99, forces)          # every leg from the same operands, too (solve! may update the old-state arrays)
            h.fields_dirty()
            _random_state(a, 3, 1234)
            jr.flow_bcs_(st, bcs, handle=h)
            h.set_option("kernel_variant", variant)
            c0 = _counters(h, keys)
            r = _solve(jr, st, pt, grid, bcs, ρg, K, G, dt, h)
            d = [b - c for b, c in zip(_counters(h, keys), c0)]
            runs.append((variant, r.iter, d, {k: np.asarray(getattr(r, k)) for k in ("norm_Rx", "norm_Ry", "norm_Rz", "norm_divV")}))
            big.sample()
            if keep is None:
                keep = {k: a[k].clone() for k in names}
                big.sample()
                continue
            for k in names:
                for x, y in zip(_observable(k, keep[k]), _observable(k, a[k])):
                    assert torch.equal(x, y), (case, variant, k)
    finally:
        h.set_option("kernel_variant", 0)
        del keep, a, st, K, G, ρg
    # every leg ran the iterations asked for; the fused leg ran an odd number of fused steps of the intended form; the others none
    assert [x[1] for x in runs] == [IT] * 3, runs
    assert (runs[0][3]["norm_Rx"] > 0).all()          # the iteration did something
    d3 = runs[0][2]
    assert d3[0] > 0 and d3[0] % 2 == 1, runs
    visc, nof1, nof2 = {"inf": (d3[0], 0, d3[0]), "inf_fz": (d3[0], d3[0], 0), "finite": (0, 0, 0)}[case]
    assert d3[1:4] == [visc, nof1, nof2] and d3[4] > 0, (case, runs)       # the observed iterations of the fused leg run the sweeps, too
    assert runs[1][2][:4] == [0, 0, 0, 0] and runs[1][2][4] >= IT, runs       # 2: the z-marching sweeps in every iteration
    assert runs[2][2] == [0, 0, 0, 0, 0], runs                              # 1: the per-node kernels only
    for x in runs[1:]:
        for k, v in x[3].items():
            assert np.array_equal(v, runs[0][3][k]), (x[0], k)


def _variant_counters_2d(h):
    return _counters(h, ("stat_fused2d", "stat_fused2d_b"))


@pytest.mark.parametrize("ni", [L.BELOW2, L.ABOVE2], ids=["below_2e29", "above_2e29"])
def test_2d_one_launch_forms_agree_past_2_gib(jr, big, ni):
    """just below 2^29 nodes the one-launch iteration is the batch form k_fused2d_b, addressing to within 2 % of 4 GiB; just above it the batch form must
    not run (the control-flow form does).  Both equal the per-node kernels (kernel_variant 1)."""
    import torch
    big.need(L.stokes2_budget(ni))
    dev = torch.device("cuda", torch.cuda.current_device())
    h = big.h
    grid, pt, bcs = _geometry(ni, DI2), _pt(ni, DI2), _bcs(2)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    K, G = jr.fzeros(ni, dev), jr.fzeros(ni, dev)
    ρg = tuple(jr.fzeros(ni, dev) for _ in range(2))
    a = _arrays(jr, st, ρg, K, G)
    names = _checked(2)
    keep, runs = None, []
    try:
        for variant in (3, 1):
            _random_operands(a, 2, 98, ("fx", "fy"))
            h.fields_dirty()
            _random_state(a, 2, 4321)
            jr.flow_bcs_(st, bcs, handle=h)
            h.set_option("kernel_variant", variant)
            c0 = _variant_counters_2d(h)
            r = _solve(jr, st, pt, grid, bcs, ρg, K, G, 0.25, h)
            runs.append((variant, r.iter, [b - c for b, c in zip(_variant_counters_2d(h), c0)], {k: np.asarray(getattr(r, k)) for k in ("norm_Rx", "norm_Ry", "norm_divV")}))
            big.sample()
            if keep is None:
                keep = {k: a[k].clone() if k in names[:6] else a[k].cpu() for k in names}      # R, ∇V and ε in host memory (budget)
                big.sample()
                continue
            for k in names:
                assert torch.equal(keep[k].to(dev), a[k]), (ni, k)
    finally:
        h.set_option("kernel_variant", 0)
        del keep, a, st, K, G, ρg
    assert [x[1] for x in runs] == [IT, IT], runs
    fused, fused_b = runs[0][2]
    assert fused > 0 and fused_b == (fused if L.batch2d(ni) else 0), runs
    assert runs[1][2] == [0, 0], runs
    for k, v in runs[1][3].items():
        assert np.array_equal(v, runs[0][3][k]), k


# ------------------------------------------------------------------------------------------------------------------------------ 2. the translated blob

def _blob_names(nd, forces):
    comps = ("xx", "yy", "zz", "yz", "xz", "xy") if nd == 3 else ("xx", "yy", "xy")
    v = ("Vx", "Vy", "Vz") if nd == 3 else ("Vx", "Vy")
    return ("P", "P0") + v + tuple("t" + c for c in comps) + tuple("to" + c for c in comps) + tuple(forces)


def _boxes(nd, names, seed):
    rng = np.random.default_rng(seed)
    return {(k, kind): rng.uniform(-1.0, 1.0, size=(L.BOX,) * nd) for kind in ("corner", "interior") for k in names}


def _box_slices(ext, kind, start):
    if kind == "corner":
        return tuple(slice(e - L.BOX, e) for e in ext)
    return tuple(slice(s, s + L.BOX) for s in start)


def _region(ext, kind, start):
    return L.corner_region(ext, IT) if kind == "corner" else L.interior_region(start, ext, IT)


def _small_run(jr, orc, nd, kind, boxes, names, pt, dt, h):
    """the box on the small grid (at the high corner, or centred): the GPU run (per-node kernels) checked against the oracle; returns its arrays and result"""
    from justrelax_jl_amd import checks
    from justrelax_jl_amd.miniapps.common import Setup, alloc_stokes, download_stokes, upload_stokes
    small, di = (L.SMALL3, DI3) if nd == 3 else (L.SMALL2, DI2)
    grid = _geometry(small, di)
    arr = alloc_stokes(small)
    arr["eta"][...] = 1.0
    arr["K"][...] = 2.0
    arr["G"][...] = 1.0
    st0 = L.small_interior_start(small)
    for k in names:
        arr[k][_box_slices(arr[k].shape, kind, st0)] = boxes[(k, kind)]
    s = Setup(ni=small, arrays=arr, grid=grid, pt=pt, dt=dt, flow_bcs=_bcs(nd), kwargs=dict(iterMax=ITER_MAX, nout=NOUT, verbose=False))
    ref = {k: v.copy(order="F") for k, v in arr.items()}
    r_ref = (orc.stokes3d_solve if nd == 3 else orc.stokes2d_solve)(ref, (checks.oracle_params3d if nd == 3 else checks.oracle_params2d)(orc, s))
    stokes, ρg, K, G = upload_stokes(s, jr.AMDGPUBackend)
    h.set_option("kernel_variant", 1)
    try:
        r = _solve(jr, stokes, s.pt, grid, s.flow_bcs, ρg, K, G, dt, h)
    finally:
        h.set_option("kernel_variant", 0)
    dev = download_stokes(stokes)
    assert r.iter == r_ref["iter"] == IT
    for k in ("norm_Rx", "norm_Ry", "norm_divV") + (("norm_Rz",) if nd == 3 else ()):
        assert np.allclose(getattr(r, k), r_ref[k], rtol=1e-10, atol=0), k
    d = checks.compare_stokes(dev, ref, _checked(nd))
    assert max(d.values()) <= TOL_ORACLE, d
    assert all(np.isfinite(dev[k]).all() for k in _checked(nd))
    return dev, r


def _blob(jr, oracle, big, ni, dt, forces, variants, fused_keys, want_fused):
    import torch
    nd = len(ni)
    dev = torch.device("cuda", torch.cuda.current_device())
    h = big.h
    names = _blob_names(nd, forces)
    boxes = _boxes(nd, names, 20261016)
    sni, di = (L.SMALL3, DI3) if nd == 3 else (L.SMALL2, DI2)
    pt = _pt(ni, di)
    small = {kind: _small_run(jr, oracle, nd, kind, boxes, names, pt, dt, h) for kind in ("corner", "interior")}
    ss_c, ss_i = _ss(small["corner"][1], sni), _ss(small["interior"][1], sni)
    ss_small = {k: ss_c[k] + ss_i[k] for k in ss_c}
    sst = L.small_interior_start(sni)
    lst = L.interior_box_start(ni)
    grid, bcs = _geometry(ni, di), _bcs(nd)
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    K, G = jr.fzeros(ni, dev, 2.0), jr.fzeros(ni, dev, 1.0)
    ρg = tuple(jr.fzeros(ni, dev) for _ in range(nd))
    a = _arrays(jr, st, ρg, K, G)
    seen = []
    try:
        for variant in variants:
            for k, t in a.items():
                if k not in ("eta", "K", "G"):
                    t.zero_()
            a["eta"].fill_(1.0)
            for k in names:
                for kind in ("corner", "interior"):
                    a[k][_box_slices(tuple(a[k].shape), kind, lst)].copy_(torch.from_numpy(boxes[(k, kind)]))
            h.fields_dirty()
            h.set_option("kernel_variant", variant)
            c0 = _counters(h, fused_keys)
            r = _solve(jr, st, pt, grid, bcs, ρg, K, G, dt, h)
            d = [b - c for b, c in zip(_counters(h, fused_keys), c0)]
            big.sample()
            assert r.iter == IT
            seen.append((variant, d))
            # the residual norms: the large grid's Σx² is the sum of the two small runs'
            ss = _ss(r, ni)
            for k, v in ss.items():
                assert np.allclose(v, ss_small[k], rtol=1e-12, atol=0), (variant, k, v, ss_small[k])
            for k in _checked(nd):
                t = a[k]
                ext = tuple(t.shape)
                ext_s = small["corner"][0][k].shape
                inside = 0
                for kind in ("corner", "interior"):
                    reg, reg_s = _region(ext, kind, lst), _region(ext_s, kind, sst)
                    got = t[reg].cpu().numpy()
                    want = small[kind][0][k][reg_s]
                    m = _observed(k, ext_s)[reg_s]
                    assert got.shape == want.shape
                    assert np.array_equal(got[m], want[m]), (variant, k, kind)
                    inside += int(torch.count_nonzero(t[reg]))
                # everything outside the two regions is exactly zero: a store that wrapped lands there
                total = int(torch.count_nonzero(t))
                assert total == inside, (variant, k, total, inside)
                assert inside > 0, (variant, k)
    finally:
        h.set_option("kernel_variant", 0)
        del a, st, K, G, ρg
    for variant, d in seen:
        want = want_fused(variant, d)
        assert d == want, (variant, d, want)


BLOB3 = [("inf", float("inf"), ()), ("inf_fz", float("inf"), ("fz",)), ("finite", 0.25, ())]


@pytest.mark.parametrize("case,dt,forces", BLOB3, ids=[c[0] for c in BLOB3])
def test_3d_translated_blob_past_2_gib(jr, oracle, big, case, dt, forces):
    big.need(L.budget(L.HIGH3, L.STOKES3_ARRAYS))
    keys = ("stat_fused3d", "stat_fused3d_visc", "stat_fused3d_nof1", "stat_fused3d_nof2")

    def want(variant, d):
        n = d[0]
        if variant != 3:
            return [0, 0, 0, 0]
        assert n > 0 and n % 2 == 1
        return {"inf": [n, n, 0, n], "inf_fz": [n, n, n, 0], "finite": [n, 0, 0, n]}[case]
    _blob(jr, oracle, big, L.HIGH3, dt, forces, (3, 2, 1), keys, want)


@pytest.mark.parametrize("ni", [L.BELOW2, L.ABOVE2], ids=["below_2e29", "above_2e29"])
def test_2d_translated_blob_past_2_gib(jr, oracle, big, ni):
    """dt = Inf: below 2^29 nodes the viscous-limit instantiation of k_fused2d_b runs (the random-state test above runs its general form)"""
    big.need(L.budget(ni, L.STOKES2_ARRAYS))

    def want(variant, d):
        if variant != 3:
            return [0, 0]
        assert d[0] > 0
        return [d[0], d[0] if L.batch2d(ni) else 0]
    _blob(jr, oracle, big, ni, float("inf"), (), (3, 1), ("stat_fused2d", "stat_fused2d_b"), want)


# ------------------------------------------------------------------------------------------------------------------------------ 3D VEP
# the arrays of the 3D VEP driver (tests/test_gpu_vep3d.py VEP3_MAP)
_VT = {"e": "ε", "epl": "ε_pl", "de": "Δε", "t": "τ", "to": "τ_o"}
VEP3 = dict(P="P", P0="P0", divV="divV", Q="Q", Vx="V.Vx", Vy="V.Vy", Vz="V.Vz", Ux="U.Ux", Uy="U.Uy", Uz="U.Uz", tII="τ.II",
            eta="viscosity.η", eta_vep="viscosity.η_vep", EII_pl="EII_pl", evol_pl="ε_vol_pl", EVol_pl="EVol_pl",
            RP="R.RP", Rx="R.Rx", Ry="R.Ry", Rz="R.Rz", omega_yz="ω.yz", omega_xz="ω.xz", omega_xy="ω.xy")
for _pre, _t in _VT.items():
    for _c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c"):
        if not (_pre == "de" and _c in ("xx", "yy", "zz")):
            VEP3[_pre + _c] = f"{_t}.{_c}"
_TC = ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c")
# one phase: linear viscous (finite at zero strain rate), elastic, Drucker-Prager with cohesion (ShearBand3D's matrix, miniapps shearband3d)
PHASE = [dict(eta=1.0, G=1.0, Kb=float("inf"), C=1.6 / np.cos(np.radians(30.0)), phi_deg=30.0, psi_deg=0.0, eta_vp=1.25e-2)]
VEP_DT = 0.25
# kept between the forms (in host memory): the state and the plastic strain, as tests/test_gpu_fullsize.py test_vep3d_edge_kernel_forms_agree_at_full_size
VEP_KEEP = ("P", "Vx", "Vy", "Vz", "EII_pl") + tuple("t" + c for c in ("xx", "yy", "zz", "yz", "xz", "xy", "yz_c", "xz_c", "xy_c")) + ("eplyz", "eplxz", "eplxy", "eplxx")
# compared between forms and translated: the state, the plastic strain and what the observed iterations store
VEP_CHECKED = ("P", "Vx", "Vy", "Vz", "EII_pl", "RP", "Rx", "Ry", "Rz", "divV") + tuple("t" + c for c in _TC) + ("eplxx", "eplyy", "eplzz", "eplyz", "eplxz", "eplxy") + \
              ("exx", "eyy", "ezz", "eyz", "exz", "exy")


def _ss_vep(r, ni):
    """the 3D VEP driver's normalisation (Stokes3D.jl:607-612): sqrt(Σx²) / ((nx-1)(ny-1)(nz-1)) for the momentum residuals, / (nx ny nz) for RP"""
    nx, ny, nz = ni
    den = (nx - 1) * (ny - 1) * (nz - 1)
    cnt = {"norm_Rx": den, "norm_Ry": den, "norm_Rz": den, "norm_divV": nx * ny * nz}
    return {k: (np.asarray(getattr(r, k)) * c) ** 2 for k, c in cnt.items()}


def _vep_arrays(jr, ni, dev):
    from justrelax_jl_amd.miniapps.common import _get
    st = jr.StokesArrays(jr.AMDGPUBackend, ni)
    a = {k: _get(st, p) for k, p in VEP3.items()}
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 1, ni)
    for t in (pr.center, pr.vertex, pr.yz, pr.xz, pr.xy):
        t.fill_(1.0)
    ρg = tuple(jr.fzeros(ni, dev) for _ in range(3))
    return st, a, pr, ρg


def _vep_zero(a):
    for k, t in a.items():
        t.zero_()
    a["eta"].fill_(1.0)


def _vep_solve(jr, st, grid, pt, ρg, pr, h):
    kw = dict(iterMax=ITER_MAX, nout=NOUT, verbose=False, viscosity_cutoff=(-np.inf, np.inf))
    return jr.solve_(st, pt, grid, _bcs(3), ρg, pr, PHASE, None, VEP_DT, None, kwargs=kw, handle=h)


VEP_FORMS = [dict(vep3_edges=4, vep3_fuse_pc=1), dict(vep3_edges=0, vep3_fuse_pc=1), dict(vep3_edges=4, vep3_fuse_pc=0)]


def _vep_set(h, form):
    for k, v in form.items():
        h.set_option(k, v)


def test_vep3d_kernel_forms_agree_past_2_gib(jr, big):
    """(770, 598, 610), a yielding random state: the default (z-marching edge kernel with LDS sharing, fused pre / centre kernel) = the one-node-per-thread
    edge kernel (vep3_edges = 0) = the three pre / centre kernels (vep3_fuse_pc = 0)"""
    import torch
    ni = L.HIGH3
    big.need(L.vep3_budget())
    dev = torch.device("cuda", torch.cuda.current_device())
    h = big.h
    grid, pt = _geometry(ni, DI3), _pt(ni, DI3)
    st, a, pr, ρg = _vep_arrays(jr, ni, dev)
    keep, runs = None, []
    try:
        for form in VEP_FORMS:
            _vep_zero(a)
            gen = torch.Generator(device=dev)
            gen.manual_seed(77)
            for k in ("P", "Vx", "Vy", "Vz"):
                _fill(a[k], gen, -1.0, 1.0)
            for c in _TC:                                   # pre-stress near yield, as tests/test_gpu_fullsize.py _build_vep3
                _fill(a["to" + c], gen, -1.5, 1.5)
                a["t" + c].copy_(a["to" + c])
            _vep_set(h, form)
            c0 = h.get_option("stat_vep3_fused")
            r = _vep_solve(jr, st, grid, pt, ρg, pr, h)
            runs.append((form, r.iter, h.get_option("stat_vep3_fused") - c0, np.asarray(r.norm_Rx)))
            big.sample()
            if keep is None:
                keep = {k: a[k].cpu() for k in VEP_KEEP}          # host memory: the device holds the driver's arrays only
                continue
            for k in VEP_KEEP:
                for x, y in zip(_observable(k, keep[k].to(dev)), _observable(k, a[k])):
                    assert torch.equal(x, y), (form, k)
    finally:
        _vep_set(h, VEP_FORMS[0])
        del keep, a, st, pr, ρg
    assert [x[1] for x in runs] == [IT] * 3, runs
    assert runs[0][2] > 0 and runs[1][2] > 0 and runs[2][2] == 0, runs          # the fused pre / centre kernel ran where asked, and only there
    for x in runs[1:]:
        assert np.array_equal(x[3], runs[0][3]), runs



def _vep_small(jr, orc, kind, boxes, names, pt, h):
    """the box on the 64^3 grid: the GPU run checked against the oracle's 3D VEP driver (tests/test_gpu_vep3d.py tolerances)"""
    import torch
    from justrelax_jl_amd.arrays import from_numpy
    from justrelax_jl_amd.miniapps.stokes3d import vep_shapes3d
    from justrelax_jl_amd.checks import interior_mask3d
    small = L.SMALL3
    grid = _geometry(small, DI3)
    arr = {k: np.zeros(s, dtype=np.float64, order="F") for k, s in vep_shapes3d(small, nphase=1).items()}
    arr["eta"][...] = 1.0
    for k in ("phase_c", "phase_yz", "phase_xz", "phase_xy"):
        arr[k][...] = 1.0
    st0 = L.small_interior_start(small)
    for k in names:
        arr[k][_box_slices(arr[k].shape, kind, st0)] = boxes[(k, kind)]
    ref = {k: v.copy(order="F") for k, v in arr.items()}
    b = _bcs(3)
    p = orc.vep_params3d(small, grid._di["center"], VEP_DT, dict(r=pt.r, theta_dtau=pt.θ_dτ, eta_dtau=pt.ηdτ, eps_rel=pt.ϵ_rel, eps_abs=pt.ϵ_abs),
                         iterMax=ITER_MAX, nout=NOUT, free_slip=b.free_slip, no_slip=b.no_slip, periodic=b.periodic)
    r_ref = orc.stokes3d_vep_solve(ref, orc.rheology_struct(PHASE), p)
    dev = torch.device("cuda", torch.cuda.current_device())
    st, a, pr, ρg = _vep_arrays(jr, small, dev)
    _vep_zero(a)
    for k in VEP3:
        a[k].copy_(from_numpy(arr[k], dev))
    _vep_set(h, dict(vep3_edges=0, vep3_fuse_pc=0))
    try:
        r = _vep_solve(jr, st, grid, pt, ρg, pr, h)
    finally:
        _vep_set(h, VEP_FORMS[0])
    out = {k: jr.to_numpy(a[k]) for k in VEP3}
    assert r.iter == r_ref["iter"] == IT
    assert np.allclose(r.norm_Rx, r_ref["norm_Rx"], rtol=1e-9) and np.allclose(r.norm_Rz, r_ref["norm_Rz"], rtol=1e-9)
    for k in VEP_CHECKED:
        m = interior_mask3d(k, ref[k].shape)
        scale = max(np.abs(ref[k]).max(), 1e-300)
        assert np.abs(out[k] - ref[k])[m].max() <= TOL_ORACLE * scale, k
    assert (ref["eplxx"] != 0).any() and (ref["eplyz"] != 0).any()             # the blob yields
    return out, r


def test_vep3d_translated_blob_past_2_gib(jr, oracle, big):
    """the translated blob for the 3D VEP driver: one yielding phase, a pre-stress well past yield in the boxes; every form of the kernel-form test"""
    import torch
    ni = L.HIGH3
    big.need(L.vep3_budget())
    dev = torch.device("cuda", torch.cuda.current_device())
    h = big.h
    names = ("P", "Vx", "Vy", "Vz") + tuple("t" + c for c in _TC) + tuple("to" + c for c in _TC)
    boxes = {key: 3.0 * v for key, v in _boxes(3, names, 20261017).items()}
    pt = _pt(ni, DI3)
    small = {kind: _vep_small(jr, oracle, kind, boxes, names, pt, h) for kind in ("corner", "interior")}
    ss_c, ss_i = _ss_vep(small["corner"][1], L.SMALL3), _ss_vep(small["interior"][1], L.SMALL3)
    sst, lst = L.small_interior_start(L.SMALL3), L.interior_box_start(ni)
    grid = _geometry(ni, DI3)
    st, a, pr, ρg = _vep_arrays(jr, ni, dev)
    seen = []
    try:
        for form in VEP_FORMS:
            _vep_zero(a)
            for k in names:
                for kind in ("corner", "interior"):
                    a[k][_box_slices(tuple(a[k].shape), kind, lst)].copy_(torch.from_numpy(boxes[(k, kind)]))
            _vep_set(h, form)
            c0 = h.get_option("stat_vep3_fused")
            r = _vep_solve(jr, st, grid, pt, ρg, pr, h)
            seen.append((form, h.get_option("stat_vep3_fused") - c0))
            big.sample()
            assert r.iter == IT
            for k, v in _ss_vep(r, ni).items():
                assert np.allclose(v, ss_c[k] + ss_i[k], rtol=1e-12, atol=0), (form, k)
            for k in VEP_CHECKED:
                t = a[k]
                ext, ext_s = tuple(t.shape), small["corner"][0][k].shape
                inside = 0
                for kind in ("corner", "interior"):
                    reg, reg_s = _region(ext, kind, lst), _region(ext_s, kind, sst)
                    got, want = t[reg].cpu().numpy(), small[kind][0][k][reg_s]
                    m = _observed(k, ext_s)[reg_s]
                    assert np.array_equal(got[m], want[m]), (form, k, kind)
                    inside += int(torch.count_nonzero(t[reg]))
                assert int(torch.count_nonzero(t)) == inside, (form, k)             # nothing outside the two regions
    finally:
        _vep_set(h, VEP_FORMS[0])
        del a, st, pr, ρg
    assert seen[0][1] > 0 and seen[1][1] > 0 and seen[2][1] == 0, seen
