#!/usr/bin/env python3
"""Times the 2D variational Stokes solve against the unmasked multiphase solve! on the same shear-band state (ϕ ≡ 1, air_phase = 0, a fixed iteration count that
no check can end), one process, device-resident inputs:
    python scripts/bench_variational2d.py [n=1024] [iters=2000] [repeats=5] [which=both|vs|vep]
Each repeat uploads the state again, so every timed solve starts from the same inputs; the first solve of either kind is a warm-up and is not reported.  The time
is the library's own (hipEvents around the PT loop).  Prints it/s per repeat, the median and the spread.  `which` runs one driver alone (for a profiler run)."""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package

jr = load_package()


def main(n=1024, iters=2000, repeats=5, which="both"):
    from test_gpu_variational_stokes import _upload
    s = jr.miniapps.shearband2d_variational(n, iterMax=iters - 1, nout=iters)
    s.kwargs.update(iterMin=iters, verbose=False)
    s.pt.ϵ_rel = s.pt.ϵ_abs = 1e-30
    kw_vep = {k: v for k, v in s.kwargs.items() if k != "air_phase"}
    rates = dict(vs=[], vep=[])
    for rep in range(repeats + 1):
        for kind in ("vep", "vs"):
            if which not in ("both", kind):
                continue
            st, pr, ρg = _upload(jr, s)
            if kind == "vs":
                ϕ = jr.RockRatio(jr.AMDGPUBackend, s.ni)
                jr.update_rock_ratio_(ϕ, pr, 0)
                r = jr.solve_VariationalStokes_(st, s.pt, s.grid, s.flow_bcs, ρg, pr, ϕ, s.extra["phases"], None, s.dt, None, kwargs=s.kwargs)
            else:
                r = jr.solve_(st, s.pt, s.grid, s.flow_bcs, ρg, pr, s.extra["phases"], None, s.dt, None, kwargs=kw_vep)
            assert r.iter == iters, (kind, r.iter)
            if rep > 0:
                rates[kind].append(r.iter / r.time)
    for kind, v in rates.items():
        if v:
            print(f"{kind} {n}x{n} {iters} iterations: it/s per repeat {[round(x, 1) for x in v]}  median {statistics.median(v):.1f}  min {min(v):.1f}  max {max(v):.1f}", flush=True)
    if rates["vs"] and rates["vep"]:
        print(f"ratio vep / vs of the medians: {statistics.median(rates['vep']) / statistics.median(rates['vs']):.3f}", flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 1024, int(a[1]) if len(a) > 1 else 2000, int(a[2]) if len(a) > 2 else 5, a[3] if len(a) > 3 else "both")
