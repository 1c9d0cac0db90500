#!/usr/bin/env python3
"""Side benchmark of inject_particles_phase_ (k_pt_inject of csrc/particles.hip, operator 12 of include/jrx.h) beside move_particles_, in ONE process.
The state is that of scripts/bench_particles2d.py: 1024^2 cells, max_xcell = 24, nxcell = 12 (jittered seeding, a 3 x 4 lattice), the phases and one extra
particle field (pT, refilled from a vertex field); a rigid rotation at Courant number 0.5.  A call is synchronous, so the host clock around it is the call: launch,
kernel, the read of the counter words and the wait.  The MEDIAN of the calls is reported.
  (a) inject, nothing deficient   the seeded cloud, min_xcell = 8: every thread copies its bucket's mask and is done
  (b) inject after each move      the rotation, per step advection_, move_particles_, inject_particles_phase_(min_xcell = 8); the share of deficient cells is reported
  (c) move_particles_             the same steps, alternating with (b)
Beside every time: the bytes the call MUST move, counted from the shapes and the state, and their time at the 8 TB/s line of one MI355X.
  (a)   the mask read and its copy written: 8 B per slot
  (b)   (a), plus the coordinates of the particles in the 3 x 3 neighbourhoods of the deficient cells (each counted once), plus what a new particle writes and reads:
        coordinates, phase, pT, the donor's phase (the four vertex values are few and not counted)
  (c)   as bench_particles2d.py counts it: source mask, coordinates and fields of the active slots read; every slot of the destination written
There is no pass mark on the times.  One condition follows from the bytes -- (a) and (b) move under a fifth of what (c) moves -- and is recorded as it turns out:
(a) < (c) and (b) < (c).
Writes one JSON line per measurement to --out (default profiles/particles2d_inject_bench.txt) and prints it.
    python scripts/bench_particles2d_inject.py [--n 1024] [--calls 20] [--out FILE]"""
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
MIN_XCELL = 8


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "particles2d_inject_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_particles2d_inject.py needs a GPU: nothing is timed on the CPU")
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
    w = 0.5 * dx / np.hypot(0.5, 0.5)          # a rigid rotation about the centre, Courant number 0.5 at the corners with dt = 1
    xv, xg = np.arange(n + 1) * dx, (np.arange(n + 2) - 0.5) * dx
    Vx = from_numpy(np.asfortranarray(np.broadcast_to(-w * (xg[None, :] - 0.5), (n + 1, n + 2))), dev)
    Vy = from_numpy(np.asfortranarray(np.broadcast_to(w * (xg[:, None] - 0.5), (n + 2, n + 1))), dev)
    Tv = from_numpy(np.asfortranarray(np.broadcast_to(300.0 + 1000.0 * xv[None, :], (n + 1, n + 1))), dev)
    slots, ncell = n * n * mx, n * n
    lines, meds = [], {}

    def report(op, us, need, **extra):
        t_line = need / LINE * 1.0e6
        rec = dict(bench="particles2d_inject", op=op, ni=f"{n}x{n}", max_xcell=mx, nxcell=a.nxcell, min_xcell=MIN_XCELL, calls=a.calls, gpu=gpu,
                   us_per_call_median=round(statistics.median(us), 1), us_min=round(min(us), 1), us_max=round(max(us), 1), must_move_MB=round(need / 1e6, 1),
                   us_at_8TBps=round(t_line, 1), share_of_8TBps=round(t_line / statistics.median(us), 3), **extra)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        meds[op] = statistics.median(us)

    inject = lambda box=None: (box if box is not None else []).append(jr.inject_particles_phase_(p, pPhases, (pT,), (Tv,), min_xcell=MIN_XCELL, handle=h))
    n0 = h.get_option("stat_particles_launches")
    # (a) nothing deficient: the seeded cloud holds nxcell = 12 >= 8 particles in every cell
    box = []
    inject(box)
    assert box[0]["n_deficient"] == 0 and box[0]["n_injected"] == 0
    report("(a) inject, nothing deficient", [call_us(inject) for _ in range(a.calls)], slots * 8, active=box[0]["n_active_before"])
    # (b), (c): the rotation
    rk2 = jr.RungeKutta2()
    jr.advection_(p, rk2, (Vx, Vy), 1.0, handle=h), jr.move_particles_(p, (pPhases, pT), handle=h), inject()          # warm-up of all three
    t_mov, t_inj, need_mov, need_inj, shares, injected, counts = [], [], [], [], [], [], None
    for _ in range(a.calls):
        jr.advection_(p, rk2, (Vx, Vy), 1.0, handle=h)
        nact = int((p.index != 0).sum())
        t_mov.append(call_us(lambda: jr.move_particles_(p, (pPhases, pT), handle=h)))
        need_mov.append(slots * 4 + nact * (16 + 16) + slots * (4 + 16 + 16))
        per_cell = (p.index != 0).sum(dim=2)
        around = torch.nn.functional.max_pool2d((per_cell < MIN_XCELL).to(torch.float32)[None, None], 3, stride=1, padding=1)[0, 0] > 0          # the cells a deficient cell reads
        donors = int(per_cell[around].sum())
        box = []
        t_inj.append(call_us(lambda: inject(box)))
        counts = box[0]
        need_inj.append(slots * 8 + donors * 16 + counts["n_injected"] * (16 + 8 + 8 + 8))
        shares.append(counts["n_deficient"] / ncell)
        injected.append(counts["n_injected"])
    report("(b) inject after each move", t_inj, statistics.median(need_inj), deficient_share_median=round(statistics.median(shares), 5),
           deficient_share_max=round(max(shares), 5), injected_per_call_median=statistics.median(injected), last_counts=counts)
    report("(c) move_particles", t_mov, statistics.median(need_mov), nargs=2)
    assert h.get_option("stat_particles_launches") - n0 == (a.calls + 1) + 3 * (a.calls + 1)
    assert bool(torch.isfinite(pT).all()) and bool(torch.isfinite(p.coords[0]).all())
    A, B, Cm = (meds[k] for k in ("(a) inject, nothing deficient", "(b) inject after each move", "(c) move_particles"))
    lines.append(json.dumps(dict(bench="particles2d_inject", op="the condition: (a) < (c) and (b) < (c)", a_us=round(A, 1), b_us=round(B, 1), c_us=round(Cm, 1),
                                 held=bool(A < Cm and B < Cm))))
    print(lines[-1], flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(f"# python scripts/bench_particles2d_inject.py --n {n} --calls {a.calls} on one MI355X, one process: host clock around each synchronous call, median of "
                   f"{a.calls} warm calls;\n# must_move_MB = the bytes the call has to move, from the shapes and the state; us_at_8TBps = their time at the 8 TB/s line; "
                   "share = that over the measured call.\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
