"""CPU test of the refusals of the 31 grid-operator entry points (advection, phase_ratios, stress_rotation, topography, principal, stepops, gridops .hip) and of
the check layer they share with the particles (csrc/op_args.hpp): tests/host/op_refusals_harness.cpp calls every entry point with one valid set of arguments, with
one fault per refusal site, and with the edge cases of the shared layer (arrays exactly adjacent, overlapping by one entry, extent products one below and at 2^31,
optional arrays absent), adds a few 2D and 3D particle calls that go through pt_disjoint, pt_apart and the presence check, and prints status and text of each call;
the output must equal tests/host/op_refusals_expected.txt byte for byte.  The harness stubs jrx_check_device, makes no HIP runtime call and dereferences no array,
so it runs without a GPU; it is built with hipcc (the operator files hold kernels) under the host address and undefined-behaviour sanitizers.  Nothing is loaded
into Python."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc is not installed")

CSRC = ROOT / "justrelax.jl_amd" / "csrc"
SOURCES = ("advection.hip", "phase_ratios.hip", "stress_rotation.hip", "topography.hip", "principal.hip", "stepops.hip", "gridops.hip", "particles.hip",
           "particles3d.hip")


def test_every_refusal_of_the_grid_operators_keeps_its_status_and_text(tmp_path):
    exe = tmp_path / "op_refusals_asan"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-I", str(ROOT / "include"), "-I", str(CSRC),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    str(ROOT / "tests" / "host" / "op_refusals_harness.cpp"), *[str(CSRC / s) for s in SOURCES], "-o", str(exe)],
                   check=True, cwd=tmp_path, capture_output=True, timeout=900)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    want = [ln for ln in (ROOT / "tests" / "host" / "op_refusals_expected.txt").read_text(encoding="utf-8").splitlines() if not ln.startswith("#")]
    got = r.stdout.splitlines()
    differ = [(w, g) for w, g in zip(want, got) if w != g]
    assert not differ and len(got) == len(want), (len(want), len(got), differ[:5])
    entries = {ln.split(" | ")[0] for ln in got}
    grid = {e for e in entries if "particles" not in e}
    assert len(grid) == 31 and len(entries) == 36 and all(f"{e} | valid" in r.stdout for e in entries), sorted(entries)
