"""CPU test of csrc/heat_plan.hpp, the two host decisions of the heat-diffusion drivers: which iterations of the PT loop are observed (the cadence heat_solve of
csrc/thermal_common.hpp walks: runs of unobserved iterations in whole graphs of 32, the rest as single launches) and the default tile of the 3D one-launch kernels with
the list of instantiations the dispatch builds.  tests/host/heat_plan_harness.cpp holds the known answers -- the counts of tests/_heat_diffusion.py for the cadences of
tests/test_gpu_heat_diffusion_inputs.py and the benchmark's, iterMax = 1, nout = 1, nout > iterMax; the tile of 16^3 ... 256^3, the decoding of "thermal_cfg", the depth
with "thermal_xg" != 8, every default shape instantiated -- and is built with g++ under -fsanitize=address,undefined, like tests/host/dyrel_conv_harness.cpp
(tests/test_host_dyrel_conv.py).  The header includes no HIP header: g++ alone must compile it."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="g++ not found")


def test_heat_plan_known_answers_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "heat_plan_asan"
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "justrelax.jl_amd" / "csrc"), str(ROOT / "tests" / "host" / "heat_plan_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
