#!/usr/bin/env python3
"""Times the 3D DYREL solve against the 3D multiphase visco-elasto-plastic solve! on the same shear band, one process, device-resident inputs:
    python scripts/bench_dyrel3d.py [n=128] [iters=400] [step_timeout_s=240]
DYREL runs a fixed budget (ϵ = 0, rel_drop = 0, iterMax = total_iterMax = iters - 1: one Powell-Hestenes step of `iters` inner iterations, a residual check every 100
of them); the sibling driver runs `iters` PT iterations that no check can end.  Either driver gets a freshly uploaded copy of the same host state; its first solve is
a warm-up and is not reported.  DYREL's time is the library's own (hipEvents around the loop), the sibling's the wall clock around the synchronous call.  Every
step (an upload, a solve) runs under its own alarm: one that overruns ends the script with a non-zero status and nothing more is started.  Prints the two rates and
their ratio."""
import signal
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package

jr = load_package()


class StepTimeout(Exception):
    pass


def step(name, seconds, fn):
    def over(*_):
        raise StepTimeout(name)
    signal.signal(signal.SIGALRM, over)
    signal.alarm(int(seconds))
    try:
        return fn()
    finally:
        signal.alarm(0)


def main(n=128, iters=400, limit=240):
    import torch
    import _dyrel3d as dy
    from test_gpu_dyrel3d import Dev
    ni = (n, n, n)
    a, phases, di, dt = step("host state", limit, lambda: dy.shearband_state(*ni, C_cos=0.39, psi_deg=10.0, radius=0.25))
    d0 = dy.new_dyrel(ni)
    kw = dict(nout=100, rel_drop=0.0, iterMax=iters - 1, total_iterMax=iters - 1, verbose_PH=False, verbose_DR=False, linear_viscosity=True)
    rates = {}
    for rep in range(2):
        g = step("upload", limit, lambda: Dev(jr, a, d0, phases, di, dt, ϵ=0.0))
        r = step("solve_DYREL!", limit, lambda: jr.solve_DYREL_(g.st, g.ρg, g.dy, g.bcs, g.pr, phases, None, di, dt, kwargs=kw))
        assert r.iter == iters, r.iter
        rates["dyrel"] = r.iter / r.time
        del g
    pt = jr.PTStokesCoeffs((1.0, 1.0, 1.0), di, ϵ_rel=1.0e-300, ϵ_abs=1.0e-300, Re=3.0, r=0.7)
    for rep in range(2):
        g = step("upload", limit, lambda: Dev(jr, a, d0, phases, di, dt))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = step("solve!", limit, lambda: jr.solve_(g.st, pt, di, g.bcs, g.ρg, g.pr, phases, None, dt, None, kwargs=dict(iterMax=iters - 1, nout=10 ** 9, verbose=False)))
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        assert r.iter == iters, r.iter
        rates["vep"] = r.iter / el
        del g
    print(f"3D shear band {n}^3, {iters} inner iterations, linear_viscosity, two phases", flush=True)
    print(f"dyrel3d  it/s {rates['dyrel']:.1f}   ({1e3 / rates['dyrel']:.3f} ms per inner iteration)", flush=True)
    print(f"vep3d    it/s {rates['vep']:.1f}   ({1e3 / rates['vep']:.3f} ms per PT iteration)", flush=True)
    print(f"ratio dyrel3d / vep3d: {rates['dyrel'] / rates['vep']:.3f}", flush=True)
    return rates


if __name__ == "__main__":
    v = sys.argv[1:]
    try:
        main(int(v[0]) if v else 128, int(v[1]) if len(v) > 1 else 400, int(v[2]) if len(v) > 2 else 240)
    except StepTimeout as e:
        print(f"step `{e}` overran its time limit; nothing more was started", flush=True)
        sys.exit(124)
