#!/usr/bin/env python3
"""From samples to a kriged map without a hand-picked variogram: empirical variogram -> fit -> KrigingSolver -> solve,
on the samples and the grid of the reference's own kriging test (test/estimation/krig.jl:6-8), then the same on a
second variable of the same table in one pass over the pairs.
python examples/variography.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}

x = np.arange(0.0, 101.0, 10.0)[:, None]
z = np.array([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.4, 0.3, 0.2, 0.1, 0.0])
data = gss.georef({"z": z, "w": z ** 2}, x)

# 1. empirical variogram: 5 lags of 10 up to half the extent (the default maxlag, a tenth of the diagonal, suits
#    thousands of scattered samples, not eleven on a line)
g = gss.EmpiricalVariogram(data, "z", nlags=5, maxlag=50.0)
out["empirical"] = g
print("lag      ", np.round(g.abscissa, 3))
print("gamma    ", np.round(g.ordinate, 5))
print("pairs    ", g.counts, " duplicates:", g.nduplicates)

# 2. fit: the best of three kinds by weighted least squares (weights = pairs per bin)
model, objectives = gss.fit([gss.GaussianVariogram, gss.SphericalVariogram, gss.ExponentialVariogram], g,
                            return_objectives=True)
out["model"], out["objectives"] = model, objectives
print("fitted   %s  sill %.5f  nugget %.5f  range %.3f" % (model.kind, model.sill, model.nugget, model.range))

# 3. the fitted model is a solver parameter like any other
problem = gss.EstimationProblem(data, gss.CartesianGrid(100), "z")
sol = gss.solve(problem, gss.KrigingSolver(("z", dict(variogram=model))))
out["kriging"] = (sol["z"], sol["z_variance"])
print("kriging  mean[0:3] = %s   variance[0:3] = %s" % (np.round(sol["z"][:3], 4), np.round(sol["z_variance"][:3], 4)))

# 4. several variables of one table share the pass over the pairs; a direction restricts the pairs
both = gss.EmpiricalVariogram(data, ["z", "w"], nlags=5, maxlag=50.0)
out["both"] = both
along = gss.DirectionalVariogram((1.0,), data, "z", nlags=5, maxlag=50.0)
out["directional"] = along
print("two variables in one call: gamma_w =", np.round(both["w"].ordinate, 5))
