#!/usr/bin/env python3
"""Census of the gfx950 kernels compiled into libgss_hip.so: one line per kernel, family and template arguments.

    python tools/kernel_census.py [--lib path/to/libgss_hip.so] [--family SUBSTRING]... [kernel_stats.csv]

With the kernel-stats CSV of a `rocprofv3 --kernel-trace --stats` run the listing also says how often each compiled
kernel was launched in that run, and ends with the ones that never were.  tests/test_kernel_census.py holds the kriging
families of this list against the case table tests/kernel_cases.py, tests/test_search_census.py the neighbour-search and
IDW / LWR families against tests/search_cases.py, tests/test_variography_instances_host.py the pair kernels of
variography.hip against tests/vario_cases.py, tests/test_fftgs_census.py the FFTGS families (fused, generic and rocFFT
pipelines, co-simulation mix) against the run table tests/fftgs_cases.py, tests/test_sgs_census.py the SGS kernels
against the run table tests/sgs_cases.py, tests/test_ik_census.py the indicator-kriging kernels against
tests/ik_kernel_cases.py, and tests/test_cokrig_census.py the global-cokriging kernels against
tests/cokrig_kernel_cases.py.
"""
import argparse
import csv
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_dpp_hazards import code_objects

LLVM_BIN = "/opt/rocm/lib/llvm/bin"
READELF = os.path.join(LLVM_BIN, "llvm-readelf")
# the demangler of the ROCm LLVM directory; binutils' c++filt (same output for these names) where that build lacks it
CXXFILT = next((p for p in (os.path.join(LLVM_BIN, "llvm-cxxfilt"), shutil.which("llvm-cxxfilt"), shutil.which("c++filt"))
                if p and os.path.exists(p)), None)
DEFAULT_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "geostatssolvers.jl_amd", "lib",
                           "libgss_hip.so")


def tools_present():
    return os.path.exists(READELF) and CXXFILT is not None


def mangled_kernels(path):
    """Symbol names of the kernels (the .name entries of the amdhsa.kernels metadata) of every gfx950 code object."""
    names = set()
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            out = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"^\s*\.symbol:\s+'?([^'\s]+?)\.kd'?\s*$", out, re.M):
            names.add(m.group(1))
    return sorted(names)


def demangle(names):
    if not names:
        return []
    out = subprocess.run([CXXFILT], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def split_args(s):
    """'3, 31, (bool)1' -> ('3', '31', 'true'); nested <> and () stay together."""
    args, depth, cur = [], 0, ""
    for ch in s:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        args.append(cur.strip())
    norm = []
    for a in args:
        a = {"(bool)1": "true", "(bool)0": "false"}.get(a, a)
        norm.append(a)
    return tuple(norm)


def parse(demangled):
    """'void gss::krig_rhs2_kernel<3, -1>(gss::VgDev, ...)' -> ('krig_rhs2_kernel', ('3', '-1'))."""
    s = demangled.strip().replace("(anonymous namespace)::", "")   # knn_build.hip keeps its kernels in one
    if s.startswith("void "):
        s = s[5:]
    depth, head = 0, ""
    for ch in s:             # up to the parenthesis that opens the parameter list
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            break
        head += ch
    m = re.match(r"^(.*?)(?:<(.*)>)?$", head.strip())
    family = m.group(1).split("::")[-1]
    return family, split_args(m.group(2) or "")


def census(path=DEFAULT_LIB):
    """Sorted list of (family, template arguments) of the compiled kernels."""
    return sorted({parse(d) for d in demangle(mangled_kernels(path))})


def launched(stats_csv):
    """{(family, args): calls} from the Name / Calls columns of a rocprofv3 kernel-stats CSV."""
    calls = {}
    with open(stats_csv, newline="") as f:
        for row in csv.DictReader(f):
            key = parse(row["Name"])
            calls[key] = calls.get(key, 0) + int(row["Calls"])
    return calls


def fmt(key):
    family, args = key
    return "%s<%s>" % (family, ", ".join(args)) if args else family


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("stats", nargs="?", help="kernel-stats CSV of a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--family", action="append", help="only kernels whose family name contains this (repeatable)")
    a = ap.parse_args()
    kernels = [k for k in census(a.lib) if any(f in k[0] for f in (a.family or [""]))]
    if not a.stats:
        for k in kernels:
            print(fmt(k))
        print("%d kernels" % len(kernels))
        return 0
    calls = launched(a.stats)
    never = [k for k in kernels if calls.get(k, 0) == 0]
    print("launched (%d of %d compiled kernels):" % (len(kernels) - len(never), len(kernels)))
    for k in kernels:
        if calls.get(k, 0):
            print("  %6d  %s" % (calls[k], fmt(k)))
    print("never launched (%d):" % len(never))
    for k in never:
        print("          %s" % fmt(k))
    return 0


if __name__ == "__main__":
    sys.exit(main())
