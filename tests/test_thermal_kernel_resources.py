"""Compile-time check of the thermal (args.ΔT) instantiations of the pre kernels of the multiphase VEP drivers: the two sources are compiled for gfx950 with the
library's flags and the compiler's kernel resource remarks are read (scripts/kernel_resources.py) -- needs hipcc, no GPU.

Per thermal instantiation (last template argument true) against its isothermal twin (the same arguments, false): the same waves per SIMD and no more scratch.
The unobserved forms, which run in every iteration of the loop, must use no scratch at all unless their twin does.
One exception is named below with its reason."""
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc is not installed")

SCRATCH, WAVES = "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"
# k_vep3_prec observed (OBS = true), one phase, without neighbours: 12 B per lane.  The same source without the thermal term compiled to 12 B before the kernel
# argument grew by the two members of args.ΔT and to 0 B since (another register assignment of unchanged code); the thermal form keeps the 12 B.  It runs on observed iterations only
# (a norm check or the last one), whose twins with 2, 3, 4 phases carry 12, 20, 36 B.
EXCEPTIONS = {"k_vep3_prec<false, false, 1, true, true, true>": 12}


@pytest.fixture(scope="module")
def tables():
    sys.path.insert(0, str(ROOT / "scripts"))
    import kernel_resources as kr
    with ThreadPoolExecutor(2) as ex:
        t2, t3 = ex.map(lambda a: kr.resources(*a), (("stokes2d_vep.hip", r"^k_vep_pre"), ("stokes3d_vep.hip", r"^k_vep3_pre")))
    return {**t2, **t3}


def test_every_thermal_instantiation_keeps_its_twins_occupancy_and_scratch(tables):
    thermal = [k for k in tables if k.endswith("true>") and re.sub(r"true>$", "false>", k) in tables]
    assert len(thermal) >= 6 + 9 + 19          # k_vep_pre (4) + k_vep_pre_b (2); k_vep3_pre (9); k_vep3_prec (10 without neighbours less one, 8 with, 2 density-updating)
    for k in thermal:
        v, t = tables[k], tables[re.sub(r"true>$", "false>", k)]
        assert v[WAVES] == t[WAVES], (k, v, t)
        assert v[SCRATCH] <= max(t[SCRATCH], EXCEPTIONS.get(k, 0)), (k, v, t)
    for k in EXCEPTIONS:
        assert k in tables


def test_thermal_forms_of_the_loop_use_no_scratch(tables):
    """what an unobserved iteration launches: the 2D kernels, k_vep3_pre, and k_vep3_prec with OBS = false -- no scratch, but for the density-updating k_vep3_prec, whose
    isothermal twin spills already (bounded by the twin above)"""
    n = 0
    for k, v in tables.items():
        if not k.endswith("true>"):
            continue
        m = re.match(r"k_vep3_prec<false, (true|false), (\d), (true|false), ", k)
        if m and (m.group(3) == "true" or m.group(1) == "true"):
            continue
        assert v[SCRATCH] == 0, (k, v)
        n += 1
    assert n >= 6 + 9 + 8


def test_four_phase_unobserved_thermal_form_is_not_built(tables):
    """that instantiation spills 20 B per lane where its twin spills nothing: the driver sends four phases to the run-time-loop form (NP = 0), and nothing instantiates it"""
    assert "k_vep3_prec<false, false, 4, false, true, true>" not in tables
    assert "k_vep3_prec<false, false, 4, false, true, false>" in tables and "k_vep3_prec<false, false, 0, false, true, true>" in tables
