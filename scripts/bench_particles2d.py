#!/usr/bin/env python3
"""Side benchmark of the 2D particle operators of csrc/particles.hip, beside the particle-free route at the same grid, in ONE process.
1024^2 cells, max_xcell = 24, nxcell = 12 (jittered seeding), two phases and one extra particle field (pT); a rigid rotation at Courant number 0.5, so nothing
overflows and nothing jumps.  Each operator is called once to warm up and then `calls` times; a call is synchronous (it ends in the library's wait for its
stream), so the host clock around it is the call: launch, kernel and wait.  The MEDIAN of the calls is reported.  advection! and move_particles! alternate, as
in a time loop, and are timed separately.

Beside every time: the bytes the operator MUST move, counted from the shapes (every array it needs read once, every array it writes written once; the mask of
every slot, the coordinates and fields of the active slots only), and the time those bytes take at the 8 TB/s line of one MI355X.  The share is must-move time
over measured time; it is not a kernel-only figure (the launch and the wait are inside the call).
  advection!         mask + coordinates read, coordinates of the active slots written, V read
  move_particles!    source mask, coordinates and fields of the active slots read; every slot of the destination (mask, coordinates, fields) written
  grid2particle!     mask, coordinates, F read; every slot of pF written
  particle2grid!     mask, coordinates, pF read; F written
  update_phase_ratios!   mask, coordinates, pPhases read; the four members written
The particle-free route (WENO_advection! of two phase fields + update_phase_ratios_2D!): per field u, Vx, Vy read and u written; two fields read, four members
written.
Writes one JSON line per measurement to --out (default profiles/particles2d_bench.txt) and prints it.
    python scripts/bench_particles2d.py [--n 1024] [--calls 20] [--out FILE]"""
import argparse
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
from justrelax_jl_amd.arrays import from_numpy

LINE = 8.0e12                   # B/s, the HBM3E line rate of one MI355X


def call_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1.0e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--max-xcell", type=int, default=24)
    ap.add_argument("--nxcell", type=int, default=12)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "particles2d_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_particles2d.py needs a GPU: nothing is timed on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _lib.default_handle(dev.index)
    gpu = torch.cuda.get_device_name(dev)
    n, mx = a.n, a.max_xcell
    ni = (n, n)
    grid = jr.Geometry(ni, (1.0, 1.0))
    dx = 1.0 / n
    p = jr.init_particles(jr.AMDGPUBackend, a.nxcell, mx, a.nxcell // 2, grid, ni, rng=np.random.default_rng(20261020))
    pPhases, pT = jr.init_cell_arrays(p, 2)
    act = p.index != 0
    pPhases.copy_(torch.where(act, torch.where(p.coords[0] < 0.5, 1.0, 2.0), 0.0))
    pT.copy_(torch.where(act, 300.0 + 1000.0 * p.coords[1], 0.0))
    # a rigid rotation about the centre, Courant number 0.5 at the corners with dt = 1
    w = 0.5 * dx / np.hypot(0.5, 0.5)
    xv, xg = np.arange(n + 1) * dx, (np.arange(n + 2) - 0.5) * dx
    Vx = from_numpy(np.asfortranarray(np.broadcast_to(-w * (xg[None, :] - 0.5), (n + 1, n + 2))), dev)
    Vy = from_numpy(np.asfortranarray(np.broadcast_to(w * (xg[:, None] - 0.5), (n + 2, n + 1))), dev)
    F = from_numpy(np.asfortranarray(np.add.outer(xv, 2.0 * xv)), dev)
    pr = jr.PhaseRatios(jr.AMDGPUBackend, 2, ni)
    slots, ncell, nvert = n * n * mx, n * n, (n + 1) * (n + 1)
    vbytes = 8 * ((n + 1) * (n + 2) + (n + 2) * (n + 1))
    lines = []

    def report(op, us, need, **extra):
        t_line = need / LINE * 1.0e6
        rec = dict(bench="particles2d", op=op, ni=f"{n}x{n}", max_xcell=mx, nxcell=a.nxcell, calls=a.calls, gpu=gpu, us_per_call_median=round(statistics.median(us), 1),
                   us_min=round(min(us), 1), us_max=round(max(us), 1), must_move_MB=round(need / 1e6, 1), us_at_8TBps=round(t_line, 1),
                   share_of_8TBps=round(t_line / statistics.median(us), 3), **extra)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        meds[op] = statistics.median(us)

    meds = {}
    n0 = h.get_option("stat_particles_launches")
    rk2 = jr.RungeKutta2()
    step = lambda: (jr.advection_(p, rk2, (Vx, Vy), 1.0, handle=h), jr.move_particles_(p, (pPhases, pT), handle=h))
    step()                                                     # warm-up of both
    t_adv, t_mov, counts = [], [], None
    nact0 = int((p.index != 0).sum())
    for _ in range(a.calls):
        t_adv.append(call_us(lambda: jr.advection_(p, rk2, (Vx, Vy), 1.0, handle=h)))
        box = []
        t_mov.append(call_us(lambda: box.append(jr.move_particles_(p, (pPhases, pT), handle=h))))
        counts = box[0]
    nact = int((p.index != 0).sum())
    report("advection_rk2", t_adv, slots * 4 + nact0 * 16 + nact0 * 16 + vbytes, active=nact0)
    report("move_particles", t_mov, slots * 4 + nact0 * (16 + 16) + slots * (4 + 16 + 16), nargs=2, active=nact0, last_counts=counts)
    for op, need, fn in (("grid2particle", slots * 4 + nact * 16 + 8 * nvert + slots * 8, lambda: jr.grid2particle_(pT, F, p, handle=h)),
                         ("particle2grid", slots * 4 + nact * 24 + 8 * nvert, lambda: jr.particle2grid_(F, pT, p, handle=h)),
                         ("update_phase_ratios", slots * 4 + nact * 24 + 8 * 2 * (ncell + nvert + 2 * n * (n + 1)),
                          lambda: jr.update_phase_ratios_(pr, p, pPhases, handle=h))):
        fn()
        report(op, [call_us(fn) for _ in range(a.calls)], need, active=nact)
    assert h.get_option("stat_particles_launches") - n0 == 5 * (a.calls + 1)
    assert bool(torch.isfinite(pr.vertex).all()) and bool(torch.isfinite(F).all())

    # the particle-free route at the same grid: WENO-5 advection of two phase fields, then update_phase_ratios_2D!
    fields = (jr.fzeros(ni, dev), jr.fzeros(ni, dev))
    xc = torch.tensor(grid.xci[0], device=dev)[:, None]
    fields[0].copy_((xc < 0.5).to(torch.float64).expand(n, n))
    fields[1].copy_(1.0 - fields[0])
    Vx_c, Vy_c = jr.fzeros(ni, dev), jr.fzeros(ni, dev)
    jr.velocity2center_(Vx_c, Vy_c, Vx, Vy)
    weno = jr.WENO5(jr.AMDGPUBackend, 2, ni)
    di = (dx, dx)
    adv = lambda: [jr.WENO_advection_(f, (Vx_c, Vy_c), weno, di, 1.0) for f in fields]
    rat = lambda: jr.update_phase_ratios_2D_(pr, fields, grid)
    adv(), rat()
    t_w, t_r = [], []
    for _ in range(a.calls):
        t_w.append(call_us(adv))
        t_r.append(call_us(rat))
    report("fields: WENO_advection x 2", t_w, 2 * 32 * ncell)
    report("fields: update_phase_ratios_2D", t_r, 16 * ncell + 8 * 2 * (ncell + nvert + 2 * n * (n + 1)))
    tot_p = meds["advection_rk2"] + meds["move_particles"] + meds["update_phase_ratios"]
    lines.append(json.dumps(dict(bench="particles2d", op="per step: advect + move + ratios (particles) vs WENO x 2 + ratios (fields)", ni=f"{n}x{n}",
                                 particles_us=round(tot_p, 1), fields_us=round(meds["fields: WENO_advection x 2"] + meds["fields: update_phase_ratios_2D"], 1))))
    print(lines[-1], flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(f"# python scripts/bench_particles2d.py --n {n} --calls {a.calls} on one MI355X, one process: host clock around each synchronous call, median of "
                   f"{a.calls} warm calls;\n# must_move_MB = the bytes the operator has to move, from the shapes; us_at_8TBps = their time at the 8 TB/s line; "
                   "share = that over the measured call.\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
