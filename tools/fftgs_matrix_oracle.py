#!/usr/bin/env python3
"""Measures the error bars of tests/fftgs_cases.py: runs oracle.fftgs (FP64) on every run of the table, compares it with
the 80-bit restatement of tests/fftgs_matrix.py and prints, per run, the largest error of the spectral amplitude F
(relative to max F) and of the realisations z (absolute), then the two maxima and the bars that follow (16 x).  CPU only.

    python tools/fftgs_matrix_oracle.py [RUN ...]      prints the per-run errors and the BARS block
    python tools/fftgs_matrix_oracle.py --write        ... and rewrites the BARS block of tests/fftgs_cases.py
"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "geostatssolvers.jl_amd")):
    sys.path.insert(0, p)

import fftgs_cases as FC
import fftgs_matrix as FM


def block(worst):
    return ("BARS = {\n" + "".join('    "%s": {"oracle": %.3e, "bar": %.3e},\n' % (q, worst[q], 16.0 * worst[q])
                                   for q in ("F", "z")) + "}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("runs", nargs="*", help="names of runs (default: every run of fftgs_cases.RUNS)")
    ap.add_argument("--write", action="store_true", help="rewrite the BARS block of tests/fftgs_cases.py (every run only)")
    a = ap.parse_args()
    if not FM.long_double_ok():
        sys.exit("numpy.longdouble is no finer than FP64 here: the restatement needs an 80-bit (or finer) long double")
    if a.write and a.runs:
        sys.exit("--write measures every run")
    worst = {"F": 0.0, "z": 0.0}
    for name in a.runs or FC.RUNS:
        run = FC.RUNS[name]
        t0 = time.time()
        normals = FM.oracle_normals(run)
        ref = FM.reference(run, normals)
        t1 = time.time()
        e = FM.errors(FM.oracle_run(run, normals), ref)
        print("%-22s F %.2e of max F (of %.1e allowed)   z %.2e (of %.1e)   reference %.1f s, oracle %.1f s"
              % (name, e["F"][0], FC.TOL["F"] / 16, e["z"][0], FC.TOL["z"] / 16, t1 - t0, time.time() - t1), flush=True)
        for q in worst:
            worst[q] = max(worst[q], e[q][0])
    print(block(worst), end="")
    for q in worst:
        if worst[q] > FC.TOL[q] / 16:
            print("the oracle's %s error exceeds 1/16 of the suite's tolerance %g: choose a quieter model" % (q, FC.TOL[q]))
    if a.write:
        path = os.path.join(ROOT, "tests", "fftgs_cases.py")
        src = open(path).read()
        new, n = re.subn(r"^BARS = \{\n(?:    .*\n)*\}\n", block(worst), src, flags=re.M)
        assert n == 1, "BARS block of tests/fftgs_cases.py not found"
        open(path, "w").write(new)
        print("wrote", os.path.normpath(path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
