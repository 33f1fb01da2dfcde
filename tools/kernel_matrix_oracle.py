#!/usr/bin/env python3
"""Measures the error bars of tests/kernel_cases.py: runs oracle.kriging (FP64) on every case of the table, compares
it with the 50-digit answer of tests/kernel_matrix.py and prints, per kernel family, the largest error of the means,
the variances and the pairwise covariances in units of 2^-53 sill, and the bar that follows (16 x, floor 8, never
looser than the 1e-9 of DESIGN.md section 3).  CPU only.

    python tools/kernel_matrix_oracle.py            prints the BARS block of tests/kernel_cases.py
"""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "geostatssolvers.jl_amd")):
    sys.path.insert(0, p)

import kernel_cases as KC
import kernel_matrix as KM


def bar(oracle_units):
    return min(max(16.0 * oracle_units, 8.0), 1e-9 / KM.UNIT)


def main():
    worst = {f: {"mean": 0.0, "var": 0.0, "cov": 0.0} for f in KC.FAMILIES}
    t0 = time.time()
    for (family, args), case in KC.CASES.items():
        if not isinstance(case, KC.Case):
            continue
        p = KM.problem_of(case)
        rmean, rvar, rc0 = KM.reference(p)
        omean, ovar, oc0 = KM.oracle_run(p, case)
        e = {"mean": KM.units(omean, rmean), "var": KM.units(ovar, rvar), "cov": KM.units(oc0, rc0)}
        print("%-28s %-14s %s  mean %8.2f  var %8.2f  cov %6.2f   (%.0f s)"
              % (family, args, case.model, e["mean"], e["var"], e["cov"], time.time() - t0), file=sys.stderr)
        for q in e:
            worst[family][q] = max(worst[family][q], e[q])
    for f in KC.FAMILIES:
        w = worst[f]
        print('    "%s": {' % f)
        for q in ("mean", "var", "cov"):
            print('        "%s": {"oracle": %.2f, "bar": %.1f},' % (q, w[q], bar(w[q])))
        print("    },")


if __name__ == "__main__":
    main()
