"""CPU test of csrc/pt_log.hpp, the convergence log the seven pseudo-transient Stokes drivers share: tests/host/pt_log_harness.cpp holds the known answers (the cap
guard, NULL history arrays, err_it1, the NaN rule, the 2D form, av_time_s, the NaN exit) and is built with g++ under -fsanitize=address,undefined, like
tests/host/ctl_harness.cpp (tests/test_host_sanitizers.py).  The header includes no HIP header: g++ alone must compile it."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="g++ not found")

LINE_3D = "iter = 2, abs_err = 2.000e+00, rel_err = 5.000e-01 [norm_Rx=2.000e+00, norm_Ry=1.000e+00, norm_Rz=5.000e-01, norm_∇V=2.500e-01] \n"
LINE_2D = "Total steps = 2, abs_err = 2.000e+00 , rel_err = 5.000e-01 [norm_Rx=2.000e+00, norm_Ry=1.000e+00, norm_∇V=2.500e-01] \n"


def test_pt_log_known_answers_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "pt_log_asan"
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "justrelax.jl_amd" / "csrc"), str(ROOT / "tests" / "host" / "pt_log_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout == LINE_3D + LINE_2D + "ok\n"        # the reference's two progress lines, byte for byte

