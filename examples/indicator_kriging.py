#!/usr/bin/env python3
"""Skewed, preferentially sampled data: declustering weights -> the global proportions F* -> median indicator kriging of
the local ccdf -> E-type mean, conditional variance, P(grade > cutoff) and the median.
python examples/indicator_kriging.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}

# 0. a 100 x 100 field with a rich zone drilled on a tight pattern, lognormal noise on top: skewed and clustered
rng = np.random.default_rng(1)
grade = lambda p: 1.0 + 7.0 * np.exp(-((p[:, 0] - 30.0) ** 2 + (p[:, 1] - 60.0) ** 2) / (2.0 * 8.0 ** 2))
infill = np.array([30.0, 60.0]) + 6.0 * rng.standard_normal((300, 2))
regular = np.stack(np.meshgrid(np.arange(5.0, 100.0, 9.0), np.arange(5.0, 100.0, 9.0)), axis=-1).reshape(-1, 2)[:120]
coords = np.concatenate([infill, regular])
values = grade(coords) * np.exp(0.3 * rng.standard_normal(len(coords)))
data = gss.georef({"grade": values}, coords)

# 1. declustering weights, and with them the global proportions below each cutoff
w = gss.weight(data, gss.CellDeclustering(2.0, 40.0, ncell=24, noffsets=8, criterion="min"), "grade")
cutoffs = gss.wquantile(values, w, [0.1, 0.25, 0.5, 0.75, 0.9, 0.95])
print("cutoffs (declustered quantiles):", np.round(cutoffs, 2))

# 2. median indicator kriging: one variogram (that of the median indicator) serves every cutoff, so the six cutoffs
#    ride in one factorisation per grid node; simple kriging about the declustered proportions
grid = gss.CartesianGrid((40, 40), (0.0, 0.0), (2.5, 2.5))
model = gss.ExponentialVariogram(range=25.0, sill=0.25, nugget=0.02)
solver = gss.IndicatorKrigingSolver(("grade", dict(cutoffs=cutoffs, variogram=model, maxneighbors=16, mean="global",
                                                   weights=w)))
sol = gss.solve(gss.EstimationProblem(data, grid, "grade"), solver)
ccdf = np.stack([sol[f"grade_ccdf_{i}"] for i in range(len(cutoffs))], axis=1)
out["ccdf"] = ccdf
assert np.all(np.diff(ccdf, axis=1) >= 0.0) and ccdf.min() >= 0.0 and ccdf.max() <= 1.0     # order relations hold

# 3. post-processing: the local mean and variance, the probability that the grade exceeds 4, the local median
post = gss.postik(sol, "grade", zmin=0.0, zmax=float(values.max()) * 1.2, tail_power=(1.0, 1.5), thresholds=[4.0],
                  probs=[0.5])
out["etype"], out["pabove"], out["median"] = post["grade_etype"], post["grade_pabove_0"], post["grade_q_0"]
cent = grid.centroids()
inside = np.hypot(cent[:, 0] - 30.0, cent[:, 1] - 60.0) < 8.0
far = np.hypot(cent[:, 0] - 30.0, cent[:, 1] - 60.0) > 40.0
print("P(grade > 4): %.2f inside the rich zone, %.3f far from it" % (out["pabove"][inside].mean(), out["pabove"][far].mean()))
print("E-type mean:  %.2f inside, %.2f far; local median %.2f / %.2f"
      % (out["etype"][inside].mean(), out["etype"][far].mean(), out["median"][inside].mean(), out["median"][far].mean()))
assert out["pabove"][inside].mean() > 0.5 > 0.1 > out["pabove"][far].mean()
