#!/usr/bin/env python3
"""Side benchmark of the 3D particle operators of csrc/particles3d.hip, beside the particle-free route at the same grid, in ONE process.
128^3 cells, max_xcell = 24, nxcell = 12 (jittered seeding: 25 M particles), two phases and one extra particle field (pT); a rigid rotation about a tilted axis
at Courant number 0.5.  Each operator is called once to warm up and then `calls` times; a call is synchronous (it ends in the library's wait for its stream), so
the host clock around it is the call: launch(es), kernel(s) and wait.  The MEDIAN of the calls is reported.

A/B, variants alternating in one process on the same input:
  move_particles!        every step advects once and then runs the library's move TWICE from the same source buffers into the same destination buffers -- the
                         direct 27-cell form (work = NULL) and the codes form (one-byte owners, work = the particles' byte buffer) -- in alternating order; the
                         buffers are swapped once afterwards.  Both leave the same bits (tests/test_gpu_particles3d.py), so the next step does not depend on the order.
  update_phase_ratios!   one launch for the eight members / two launches of four (tuning key particles3d_ratios_split), alternating.

Beside every time: the bytes the operator MUST move, counted from the shapes (every array it needs read once, every array it writes written once; the mask of
every slot, the coordinates and fields of the active slots only), and the time those bytes take at the 8 TB/s line of one MI355X.  It is not a kernel-only figure.
The particle-free route: WENO_advection! of two phase fields + update_phase_ratios_3D!.
Writes one JSON line per measurement to --out (default profiles/particles3d_bench.txt) and prints it.
    python scripts/bench_particles3d.py [--n 128] [--calls 10] [--out FILE]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
from __graft_entry__ import load_package

jr = load_package()
from justrelax_jl_amd import _lib
from justrelax_jl_amd.arrays import from_numpy, ptr

LINE = 8.0e12                   # B/s, the HBM3E line rate of one MI355X


def call_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1.0e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--max-xcell", type=int, default=24)
    ap.add_argument("--nxcell", type=int, default=12)
    ap.add_argument("--nphase", type=int, default=2, help="phases 1 .. nphase in slabs across the plane x + z")
    ap.add_argument("--only-ratios", action="store_true", help="time update_phase_ratios! alone (both forms) and append to --out")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "particles3d_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_particles3d.py needs a GPU: nothing is timed on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    gpu = torch.cuda.get_device_name(dev)
    n, mx = a.n, a.max_xcell
    ni = (n, n, n)
    grid = jr.Geometry(ni, (1.0, 1.0, 1.0))
    dx = 1.0 / n
    p = jr.init_particles(jr.AMDGPUBackend, a.nxcell, mx, a.nxcell // 2, *grid.xi_vel, rng=np.random.default_rng(20261021))
    pPhases, pT = jr.init_cell_arrays(p, 2)
    act = p.index != 0
    slab = torch.clamp(torch.floor(0.5 * a.nphase * (p.coords[0] + p.coords[2])), 0.0, a.nphase - 1.0)
    pPhases.copy_(torch.where(act, 1.0 + slab, 0.0))
    del slab
    pT.copy_(torch.where(act, 300.0 + 1000.0 * p.coords[1], 0.0))
    del act
    # a rigid rotation about a tilted axis through the centre, Courant number 0.5 at the corners with dt = 1
    w = 0.5 * dx / np.sqrt(0.75) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    rot = (lambda X, Y, Z: w[1] * (Z - 0.5) - w[2] * (Y - 0.5), lambda X, Y, Z: w[2] * (X - 0.5) - w[0] * (Z - 0.5), lambda X, Y, Z: w[0] * (Y - 0.5) - w[1] * (X - 0.5))
    V = []
    for gv, f in zip(grid.xi_vel, rot):
        X, Y, Z = np.meshgrid(*gv, indexing="ij", sparse=True)
        V.append(from_numpy(np.asfortranarray(f(X, Y, Z) + 0.0 * (X + Y + Z)), dev))
    xv = np.arange(n + 1) * dx
    Fv = from_numpy(np.asfortranarray(np.add.outer(np.add.outer(xv, 2.0 * xv), 3.0 * xv)), dev)
    Fc = jr.fzeros(ni, dev)
    pr = jr.PhaseRatios(jr.AMDGPUBackend, a.nphase, ni)
    slots, ncell, nvert = n ** 3 * mx, n ** 3, (n + 1) ** 3
    vbytes = 8 * 3 * (n + 1) * (n + 2) * (n + 2)
    members = 8 * a.nphase * (ncell + nvert + 3 * n * n * (n + 1) + 3 * n * (n + 1) * (n + 1))
    lines, meds = [], {}

    def report(op, us, need, **extra):
        t_line = need / LINE * 1.0e6
        rec = dict(bench="particles3d", op=op, ni=f"{n}^3", max_xcell=mx, nxcell=a.nxcell, calls=len(us), gpu=gpu, us_per_call_median=round(statistics.median(us), 1),
                   us_min=round(min(us), 1), us_max=round(max(us), 1), must_move_MB=round(need / 1e6, 1), us_at_8TBps=round(t_line, 1),
                   share_of_8TBps=round(t_line / statistics.median(us), 3), **extra)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        meds[op] = statistics.median(us)

    rk2 = jr.RungeKutta2()
    fields = (pPhases, pT)

    def raw_move(work):
        """the library's move from the current buffers into the second set, no swap; returns the counters"""
        src, dst = p._struct(), p._struct(second=True)
        a_src = (C.c_void_p * 2)(*(ptr(f) for f in fields))
        a_dst = (C.c_void_p * 2)(*(ptr(p._twins[id(f)][1]) for f in fields))
        counts = (C.c_int64 * 5)()
        h.call("jrx_particles3d_move", C.byref(src), C.byref(dst), a_src, a_dst, C.c_int32(2), work, counts)
        return dict(zip(("n_active_before", "n_active_after", "n_outside", "n_far", "n_overflow"), (int(c) for c in counts)))

    work = C.c_void_p(p._work.data_ptr())
    jr.advection_(p, rk2, V, 1.0, handle=h), raw_move(None), raw_move(work), p._swap(fields)          # warm-up of all three
    t_adv, t_dir, t_cod, counts = [], [], [], None
    nact0 = int((p.index != 0).sum())
    for it in range(0 if a.only_ratios else a.calls):
        t_adv.append(call_us(lambda: jr.advection_(p, rk2, V, 1.0, handle=h)))
        box = {}
        for form in (("direct", "codes") if it % 2 == 0 else ("codes", "direct")):
            (t_dir if form == "direct" else t_cod).append(call_us(lambda: box.__setitem__(form, raw_move(None if form == "direct" else work))))
        assert box["direct"] == box["codes"], box
        counts = box["codes"]
        p._swap(fields)
    nact = int((p.index != 0).sum())
    if not a.only_ratios:
        report_operators(report, h, p, pT, Fv, Fc, t_adv, t_dir, t_cod, counts, slots, ncell, nvert, vbytes, nact0, nact, a.calls)
    ratios = lambda: jr.update_phase_ratios_(pr, p, pPhases, handle=h)
    t_one, t_two = [], []
    for split in (0, 1):
        h.set_option("particles3d_ratios_split", split)
        ratios()
    for it in range(a.calls):
        for split in ((0, 1) if it % 2 == 0 else (1, 0)):
            h.set_option("particles3d_ratios_split", split)
            (t_two if split else t_one).append(call_us(ratios))
    h.set_option("particles3d_ratios_split", 2)
    report("update_phase_ratios: one launch, eight members", t_one, slots * 4 + nact * 32 + members, active=nact, nphase=a.nphase)
    report("update_phase_ratios: two launches of four members", t_two, 2 * (slots * 4 + nact * 32) + members, active=nact, nphase=a.nphase)
    assert bool(torch.isfinite(pr.vertex).all())
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    if a.only_ratios:
        with out.open("a") as f:
            f.write(f"# python scripts/bench_particles3d.py --n {n} --calls {a.calls} --nphase {a.nphase} --only-ratios\n" + "\n".join(lines) + "\n")
        return
    fields_route(report, lines, meds, pr, grid, V, ni, n, dx, dev, ncell, members, a.calls)
    out.write_text(f"# python scripts/bench_particles3d.py --n {n} --calls {a.calls} on one MI355X, one process: host clock around each synchronous call, median of the warm "
                   "calls; the two move forms and the two\n# phase-ratio forms alternate on the same input.  must_move_MB = the bytes the operator has to move, from the "
                   "shapes; us_at_8TBps = their time at the 8 TB/s line; share = that over the measured call.\n" + "\n".join(lines) + "\n")


def report_operators(report, h, p, pT, Fv, Fc, t_adv, t_dir, t_cod, counts, slots, ncell, nvert, vbytes, nact0, nact, calls):
    need_move = slots * 4 + nact0 * (24 + 16) + slots * (4 + 24 + 16)
    report("advection_rk2", t_adv, slots * 4 + nact0 * 24 + nact0 * 24 + vbytes, active=nact0)
    report("move_particles: direct 27-cell form (work = NULL)", t_dir, need_move, nargs=2, active=nact0, last_counts=counts)
    report("move_particles: codes form (one-byte owners)", t_cod, need_move + 2 * slots, nargs=2, active=nact0, last_counts=counts)
    for op, need, fn in (("grid2particle", slots * 4 + nact * 24 + 8 * nvert + slots * 8, lambda: jr.grid2particle_(pT, Fv, p, handle=h)),
                         ("particle2grid", slots * 4 + nact * 32 + 8 * nvert, lambda: jr.particle2grid_(Fv, pT, p, handle=h)),
                         ("centroid2particle", slots * 4 + nact * 24 + 8 * ncell + slots * 8, lambda: jr.centroid2particle_(pT, Fc, p, handle=h)),
                         ("particle2centroid", slots * 4 + nact * 32 + 8 * ncell, lambda: jr.particle2centroid_(Fc, pT, p, handle=h))):
        if op == "centroid2particle":
            jr.particle2centroid_(Fc, pT, p, handle=h)          # a centre field that holds the particles' values
        fn()
        report(op, [call_us(fn) for _ in range(calls)], need, active=nact)


def fields_route(report, lines, meds, pr, grid, V, ni, n, dx, dev, ncell, members, calls):
    # the particle-free route at the same grid: WENO-5 advection of two phase fields, then update_phase_ratios_3D!
    cf = (jr.fzeros(ni, dev), jr.fzeros(ni, dev))
    xc = torch.tensor(grid.xci[0], device=dev)[:, None, None]
    cf[0].copy_((xc < 0.5).to(torch.float64).expand(n, n, n))
    cf[1].copy_(1.0 - cf[0])
    V_c = tuple(jr.fzeros(ni, dev) for _ in range(3))
    jr.velocity2center_(*V_c, *V)
    weno = jr.WENO5(jr.AMDGPUBackend, 2, ni)
    di = (dx, dx, dx)
    adv = lambda: [jr.WENO_advection_(f, V_c, weno, di, 1.0) for f in cf]
    rat = lambda: jr.update_phase_ratios_3D_(pr, cf, grid)
    adv(), rat()
    t_w, t_r = [], []
    for _ in range(calls):
        t_w.append(call_us(adv))
        t_r.append(call_us(rat))
    report("fields: WENO_advection x 2", t_w, 2 * 40 * ncell)
    report("fields: update_phase_ratios_3D", t_r, 16 * ncell + members)
    best_move = min(meds["move_particles: direct 27-cell form (work = NULL)"], meds["move_particles: codes form (one-byte owners)"])
    best_rat = min(meds["update_phase_ratios: one launch, eight members"], meds["update_phase_ratios: two launches of four members"])
    lines.append(json.dumps(dict(bench="particles3d", op="per step: advect + move + ratios (particles, the faster form of each) vs WENO x 2 + ratios (fields)", ni=f"{n}^3",
                                 particles_us=round(meds["advection_rk2"] + best_move + best_rat, 1),
                                 fields_us=round(meds["fields: WENO_advection x 2"] + meds["fields: update_phase_ratios_3D"], 1))))
    print(lines[-1], flush=True)


if __name__ == "__main__":
    main()
