"""CPU test of csrc/dyrel_conv.hpp, the convergence bookkeeping the 2D and 3D DYREL solve loops share: tests/host/dyrel_conv_harness.cpp holds the known answers for
ND = 2 and 3 (the reference values of itPH 1 and 2, min(rel, abs), the NaN verdict ahead of the 1e10 one, the rel_drop rule and err_min, errV00, the cap guard, NULL
history arrays, err_evo_P, the association of the λmin sums, cV, finish) and is built with g++ under -fsanitize=address,undefined, like tests/host/pt_log_harness.cpp
(tests/test_host_pt_log.py).  The header includes no HIP header: g++ alone must compile it.  The GPU tests reach none of this: they run with the verbosity off,
never exceed cap and meet no NaN."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="g++ not found")

# the reference's progress lines (solver.jl:168 with two and three R pairs, :249), byte for byte
PH_2D = ("itPH = 01 iter = 000000 iter/nx = 000, err = 1.000e+00 - norm[R1=2.000e+00 1.000e+00, R2=2.000e+00 1.000e+00, Rp=4.000e+00 1.000e+00] \n"
         "itPH = 02 iter = 001234 iter/nx = 012, err = 2.000e+00 - norm[R1=4.000e+00 2.000e+00, R2=1.000e+00 5.000e-01, Rp=2.000e+00 1.000e+00] \n")
PH_3D = ("itPH = 01 iter = 000000 iter/nx = 000, err = 1.000e+00 - norm[R1=2.000e+00 1.000e+00, R2=2.000e+00 1.000e+00, R3=2.000e+00 1.000e+00, Rp=4.000e+00 1.000e+00] \n"
         "itPH = 02 iter = 001234 iter/nx = 012, err = 2.000e+00 - norm[R1=4.000e+00 2.000e+00, R2=1.000e+00 5.000e-01, R3=4.000e+00 2.000e+00, Rp=2.000e+00 1.000e+00] \n")
DR = "it = 34, iter = 1300, err = 4.000e+00 \n"


def test_dyrel_conv_known_answers_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "dyrel_conv_asan"
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "justrelax.jl_amd" / "csrc"), str(ROOT / "tests" / "host" / "dyrel_conv_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout == PH_2D + DR + PH_3D + DR + "ok\n"
