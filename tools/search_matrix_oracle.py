#!/usr/bin/env python3
"""Measures the error bars of tests/search_cases.py: runs oracle.idw_lwr (FP64) on every estimator case of the table,
compares it with the 50-digit answer of tests/search_matrix.py and prints, per kernel family and quantity, the largest
error in units of 2^-53 x the data scale and the bar that follows (16 x, floor 8, never looser than the tolerance
tests/test_gpu_idw_lwr.py holds the quantity to).  Also checks that oracle.kriging.knn_search gives the reference
lists of every unmasked, unrotated search case of at most 5 000 samples.  CPU only.

    python tools/search_matrix_oracle.py            prints the BARS block of tests/search_cases.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "geostatssolvers.jl_amd")):
    sys.path.insert(0, p)

import search_cases as SC
import search_matrix as SM
from oracle import idw_lwr as E
from oracle import kriging as K


def bar(oracle_units, q):
    return min(max(16.0 * oracle_units, 8.0), SC.EXISTING_TOL[q] / SM.UNIT)


def oracle_run(p, case):
    kw = dict(radius=p.mt.radius, radii=p.mt.radii, distance=p.distance)
    z = np.atleast_2d(p.z)
    c = p.c[p.check]
    if case.op == "idw":
        cols = [E.idw(p.x, zc, c, case.k, case.minn, case.exponent, **kw) for zc in z]
    else:
        kind, a, pw = case.weight
        wf = E.tricube if kind == 1 else E.exp_weight(a, pw)
        cols = [E.lwr(p.x, zc, c, case.k, case.minn, wf, **kw) for zc in z]
    return np.stack([r[0] for r in cols]), cols[0][1], cols[0][2]


def main():
    worst = {f: {} for f in SC.EST_FAMILIES}
    t0 = time.time()
    for (family, args), case in SC.CASES.items():
        if not isinstance(case, SC.Case):
            continue
        if case.op == "search" and case.n <= 5000 and case.ball != "rotated":
            p = SM.problem_of(case)
            ridx, rcnt, _ = SM.reference_lists(p)
            oidx, ocnt = K.knn_search(p.x, p.c[p.check], case.k, radius=p.mt.radius, radii=p.mt.radii,
                                      distance=p.distance)
            assert np.array_equal(oidx, ridx) and np.array_equal(ocnt, rcnt), (family, args)
        if case.op not in ("idw", "lwr"):
            continue
        p = SM.problem_of(case)
        ridx, rcnt, rkeys = SM.reference_lists(p)
        rmean, raux, rst = SM.mp_estimate(case, p, ridx, rcnt, rkeys if case.metric == "haversine" else None)
        omean, oaux, ost = oracle_run(p, case)
        assert np.array_equal(ost, rst), (family, args, ost, rst)
        smean, saux = SM.scales(case, p, rmean, raux)
        qm, qa = SC.quantities(case)
        e = {qm: SM.units(omean, rmean, smean), qa: SM.units(oaux, raux, saux)}
        print("%-22s %-14s %s  mean %8.2f  aux %8.2f   (%.0f s)" % (family, args, case.op, e[qm], e[qa], time.time() - t0),
              file=sys.stderr)
        for q in e:
            worst[family][q] = max(worst[family].get(q, 0.0), e[q])
    for f in SC.EST_FAMILIES:
        print('    "%s": {' % f)
        for q in sorted(worst[f]):
            print('        "%s": {"oracle": %.2f, "bar": %.1f},' % (q, worst[f][q], bar(worst[f][q], q)))
        print("    },")


if __name__ == "__main__":
    main()
