#!/usr/bin/env python3
"""Times the 3D variational Stokes solve (shear band under sticky air) against the unmasked 3D multiphase solve! on the same inputs without the air, in one process:
the `variational3d_128` leg of bench_extras.py alone.
    python scripts/bench_variational3d.py [n=128] [iters=200] [air_layers=2]
Prints the it/s of both, their ratio and the ratio the array-pass counts predict."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package

jr = load_package()


def main(n=128, iters=200, air_layers=2):
    import bench_extras
    from justrelax_jl_amd import _lib
    r = bench_extras.cfg_variational3d(jr, _lib.default_handle(), n, iters, air_layers)
    print(json.dumps(r, ensure_ascii=False, indent=1), flush=True)
    return r


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 128, int(a[1]) if len(a) > 1 else 200, int(a[2]) if len(a) > 2 else 2)
