#!/usr/bin/env python3
"""Times the 2D DYREL solve against the multiphase visco-elasto-plastic solve! on the same shear band, one process, device-resident inputs:
    python scripts/bench_dyrel2d.py [n=1024] [iters=2000] [repeats=5] [which=both|dyrel|vep]
DYREL runs a fixed budget (ϵ = 0, rel_drop = 0, iterMax = total_iterMax = iters - 1: one Powell-Hestenes step of `iters` inner iterations, a residual check every 100 of them);
the sibling driver runs `iters` PT iterations that no check can end.  Each repeat uploads the state again; the first solve of either kind is a warm-up and is not
reported.  The time is the library's own (hipEvents around the loop).  Prints inner iterations per second per repeat, the median of the repeats and the ratio of the medians."""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package

jr = load_package()


def main(n=1024, iters=2000, repeats=5, which="both"):
    import _dyrel as dy
    from test_gpu_dyrel import Dev
    from test_gpu_variational_stokes import _upload
    s = jr.miniapps.shearband2d(n, iterMax=iters - 1, nout=iters)
    s.kwargs.update(iterMin=iters, verbose=False)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    a, phases, di, dt = dy.shearband_state(n, n)
    rates = dict(dyrel=[], vep=[])
    for rep in range(repeats + 1):
        for kind in ("vep", "dyrel"):
            if which not in ("both", kind):
                continue
            if kind == "dyrel":
                g = Dev(jr, a, dy.new_dyrel((n, n)), phases, di, dt, ϵ=0.0)
                r = jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, di, dt,
                                    kwargs=dict(nout=100, rel_drop=0.0, iterMax=iters - 1, total_iterMax=iters - 1, verbose_PH=False, verbose_DR=False, linear_viscosity=True))
            else:
                st, pr, ρg = _upload(jr, dict_setup(s))
                r = jr.solve_(st, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
            assert r.iter == iters, (kind, r.iter)
            if rep > 0:
                rates[kind].append(r.iter / r.time)
    for kind, v in rates.items():
        if v:
            print(f"{kind} {n}x{n} {iters} iterations: it/s per repeat {[round(x, 1) for x in v]}  median {statistics.median(v):.1f}  min {min(v):.1f}  max {max(v):.1f}", flush=True)
    if rates["dyrel"] and rates["vep"]:
        print(f"ratio dyrel / vep of the medians: {statistics.median(rates['dyrel']) / statistics.median(rates['vep']):.3f}", flush=True)


def dict_setup(s):
    """the shear-band Setup with the two phase-ratio members the uploader of the variational tests copies besides center and vertex"""
    import numpy as np
    nx, ny = s.ni
    s.arrays.setdefault("phase_vx", np.zeros((2, nx + 1, ny), order="F"))
    s.arrays.setdefault("phase_vy", np.zeros((2, nx, ny + 1), order="F"))
    return s


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 1024, int(a[1]) if len(a) > 1 else 2000, int(a[2]) if len(a) > 2 else 5, a[3] if len(a) > 3 else "both")
