"""CPU test of csrc/pt_replay.hpp, the replay window of every PT loop that replays runs of unobserved iterations as captured graphs: the next observed iteration (a multiple
of nout, or the last one the loop can run), the run of unobserved iterations up to it and how many of them a driver holds back.  tests/host/pt_replay_harness.cpp holds the
known answers -- the windows of the 2D loops whose replays tests/test_gpu_vep_extras.py and tests/test_gpu_stokes2d_thermal.py count, `last` inside the current window,
nout = 1, an iteration one short of an observed one, the hand-written window the drivers had, and the heat loop's cadences through the forwards of csrc/heat_plan.hpp -- and is
built with g++ under -fsanitize=address,undefined, like tests/host/heat_plan_harness.cpp (tests/test_host_heat_plan.py).  The header includes no HIP header: g++ alone must
compile it."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(GXX is None, reason="g++ not found")


def test_pt_replay_known_answers_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "pt_replay_asan"
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "justrelax.jl_amd" / "csrc"), str(ROOT / "tests" / "host" / "pt_replay_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
