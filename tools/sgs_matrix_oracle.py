#!/usr/bin/env python3
"""Measures the error bars of tests/sgs_cases.py: on every run of the table the FP64 restatement (numpy.linalg for the
weights and sigma as oracle/sgs.py, a plain numpy recursion for the sweep) against the 80-bit one of tests/sgs_matrix.py,
in units of 2^-53 of the quantity's scale (max(1, max |lambda|), sqrt(sill), max |z - mean|); then the maxima and the bars
that follow (16 x, at least 8 units).  Also prints each run's level schedule as the CPU restates it.  CPU only.

    python tools/sgs_matrix_oracle.py [RUN ...]      prints the per-run errors and the BARS block
    python tools/sgs_matrix_oracle.py --write        ... and rewrites the BARS block of tests/sgs_cases.py
"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "geostatssolvers.jl_amd")):
    sys.path.insert(0, p)

import sgs_cases as SC
import sgs_matrix as SM

QUANTITIES = ("w", "sigma", "z")


def block(worst, scale):
    return ("BARS = {\n" + "".join('    "%s": {"oracle": %.2f, "bar": %.2f, "scale": %.3f},\n'
                                   % (q, worst[q], max(16.0 * worst[q], 8.0), scale[q]) for q in QUANTITIES) + "}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("runs", nargs="*", help="names of runs (default: every run of sgs_cases.RUNS)")
    ap.add_argument("--write", action="store_true", help="rewrite the BARS block of tests/sgs_cases.py (every run only)")
    a = ap.parse_args()
    if not SM.long_double_ok():
        sys.exit("numpy.longdouble is no finer than FP64 here: the restatement needs an 80-bit (or finer) long double")
    if a.write and a.runs:
        sys.exit("--write measures every run")
    worst = dict.fromkeys(QUANTITIES, 0.0)
    scale = dict.fromkeys(QUANTITIES, 1.0)
    for name in a.runs or SC.RUNS:
        run = SC.RUNS[name]
        t0 = time.time()
        e, failed = SM.oracle_errors(run)
        geo = SM.geometry(run)
        rk = SM.ranks(geo["paths"][0], geo["dl"], geo["N"])
        idx, cnt = SM.brute_lists(run, geo, geo["paths"][0])
        lvl, L = SM.levels(idx, SM.device_ncond(run, geo, cnt), geo["paths"][0], rk)
        print("%-22s w %7.2f  sigma %7.2f  z %7.2f units   N %4d  levels %4d (path 0), average %6.1f, team %s   "
              "failed %s   %.1f s" % (name, e["w"][0], e["sigma"][0], e["z"][0], geo["N"], L, (rk >= 0).sum() / max(L, 1),
                                      SM.team_schedule(run, lvl, L), failed, time.time() - t0), flush=True)
        for q in QUANTITIES:
            worst[q] = max(worst[q], e[q][0])
            scale[q] = max(scale[q], e[q][1])
    print(block(worst, scale), end="")
    for q in QUANTITIES:
        if worst[q] * SM.UNIT * scale[q] > SC.TOL[q] / 16:
            print("the oracle's %s error exceeds 1/16 of the suite's tolerance %g: choose a quieter model" % (q, SC.TOL[q]))
    if a.write:
        path = os.path.join(ROOT, "tests", "sgs_cases.py")
        src = open(path).read()
        new, n = re.subn(r"^BARS = \{\n(?:    .*\n)*\}\n", block(worst, scale), src, flags=re.M)
        assert n == 1, "BARS block of tests/sgs_cases.py not found"
        open(path, "w").write(new)
        print("wrote", os.path.normpath(path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
