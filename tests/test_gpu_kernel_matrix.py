"""Every compiled instantiation of the kriging kernels (tests/kernel_cases.py) on one exactly solvable problem each:
decoupled clusters whose ordinary / universal kriging system mpmath solves at 50 digits from the doubles the device
receives (tests/kernel_matrix.py).  Means, variances, status, neighbour counts and the pairwise covariance of the same
points are held to the bars of kernel_cases.BARS (16 x the measured error of the FP64 oracle, floor 8 units of
2^-53 sill).

What it found (moving neighbourhood): the single-structure instantiations of the three
moving-neighbourhood kernels multiplied each coordinate by the model's scale before taking differences, a product
rounded at 2^-53 |x| scale; with the clusters of the exponential and Matern cases thousands of ranges from the origin
krig_local_mfma_kernel<3, 32, 2> gave means 171.3 units off against a bar of 149.3.  The kernels now scale the
differences; the case stays as the regression test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_cases as KC
import kernel_matrix as KM

pytestmark = pytest.mark.gpu

ENTRIES = [(key, case) for key, case in KC.CASES.items() if isinstance(case, KC.Case)]


def _id(key):
    return "%s-%s" % (key[0], "_".join(str(a) for a in key[1]))


@pytest.mark.parametrize("key,case", ENTRIES, ids=[_id(k) for k, _ in ENTRIES])
def test_instantiation_matches_the_50_digit_answer(key, case):
    p = KM.problem_of(case)
    rmean, rvar, rc0 = KM.reference(p)
    mean, var, c0, status, count = KM.device_run(p, case)
    bars = KC.BARS[key[0]]
    e = {"mean": KM.units(mean, rmean), "var": KM.units(var, rvar), "cov": KM.units(c0, rc0)}
    print("%s %s: mean %.2f (bar %.1f)  var %.2f (bar %.1f)  cov %.2f (bar %.1f)  units of 2^-53 sill"
          % (_id(key), case.model, e["mean"], bars["mean"]["bar"], e["var"], bars["var"]["bar"], e["cov"],
             bars["cov"]["bar"]))
    assert not np.asarray(status).any(), status
    if case.k is not None:
        assert np.array_equal(count, np.full(p.x0.shape[0], case.k)), count
    assert mean.shape == rmean.shape
    for q in ("mean", "var", "cov"):
        assert e[q] <= bars[q]["bar"], (q, e[q], bars[q])
