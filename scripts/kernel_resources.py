#!/usr/bin/env python3
"""Register, scratch and occupancy figures of compiled kernels, from hipcc's kernel resource remarks -- needs the compiler, no GPU:

    python scripts/kernel_resources.py stokes3d_vep.hip 'k_vep3_pre' [--check-thermal]

compiles justrelax.jl_amd/csrc/<file> for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage and prints one line per kernel whose
demangled name matches the pattern: VGPRs, AGPRs, SGPRs, scratch bytes per lane, waves per SIMD, spilled VGPRs.
--check-thermal: the kernels whose last template argument is the thermal form (..., true>) are compared with their isothermal twins (..., false>): exit status 1
if a thermal instantiation has a lower occupancy than its twin or more scratch than it."""
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "justrelax.jl_amd"))
import build as jrx_build

KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill")


def remarks(src):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *jrx_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", str(jrx_build.CSRC / src), "-o", str(Path(tmp) / "o.o")]
        return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr


def parse(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in KEYS:
            cur[m.group(1)] = int(m.group(2))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):      # no binutils: the C++ runtime's own demangler
        import ctypes
        import ctypes.util
        lib = ctypes.CDLL(ctypes.util.find_library("stdc++") or "libstdc++.so.6")
        lib.__cxa_demangle.restype = ctypes.c_void_p
        libc = ctypes.CDLL(None)
        libc.free.argtypes = [ctypes.c_void_p]
        r = []
        for n in names:
            st = ctypes.c_int()
            q = lib.__cxa_demangle(n.encode(), None, None, ctypes.byref(st))
            r.append(ctypes.string_at(q).decode() if q and st.value == 0 else n)
            if q:
                libc.free(q)
    short = lambda s: re.sub(r"\(.*", "", s.replace("(anonymous namespace)::", "")).replace("void ", "")
    return {n: short(d) for n, d in zip(names, r)}


def resources(src, pattern="."):
    """{demangled kernel name: {figure: value}} of the kernels of csrc/<src> whose name matches the pattern"""
    res = parse(remarks(src))
    names = demangle(list(res))
    return {names[k]: v for k, v in res.items() if re.search(pattern, names[k])}


def main(src, pattern, check):
    table = resources(src, pattern)
    print("kernel: " + ", ".join(KEYS))
    for k in sorted(table):
        print(k + ": " + ", ".join(str(table[k].get(q)) for q in KEYS))
    bad = []
    if check:
        for k, v in table.items():
            twin = re.sub(r"true>$", "false>", k)
            if k.endswith("true>") and twin in table:
                t = table[twin]
                if v[KEYS[4]] < t[KEYS[4]] or v[KEYS[3]] > t[KEYS[3]]:
                    bad.append((k, v[KEYS[3]], v[KEYS[4]], t[KEYS[3]], t[KEYS[4]]))
        for b in bad:
            print("thermal form %s: scratch %d B, %d waves/SIMD; isothermal twin: %d B, %d waves/SIMD" % b)
    return 1 if bad else 0


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if not x.startswith("--")]
    sys.exit(main(a[0], a[1] if len(a) > 1 else ".", "--check-thermal" in sys.argv))
