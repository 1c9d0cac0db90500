"""CPU test of csrc/vep3_plan.hpp, the launch plan of the 3D VEP driver: tests/host/vep3_plan_harness.cpp holds the known answers (the node form up to 125,000 nodes, the
segments, peel and chunk depth of the z-marching forms, the combinations no kernel is built for, the depth of k_vep3_pre, the thread map of k_vep3_prec) and is built with
g++ under -fsanitize=address,undefined, like tests/host/pt_log_harness.cpp (tests/test_host_pt_log.py).  The header includes no HIP header: g++ alone must compile it."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="g++ not found")


def test_vep3_plan_known_answers_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "vep3_plan_asan"
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "justrelax.jl_amd" / "csrc"), str(ROOT / "tests" / "host" / "vep3_plan_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
