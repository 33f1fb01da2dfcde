#!/usr/bin/env python3
"""Which estimator predicts the samples best?  The samples of examples/crossvalidation.py, then the cross-validation
error of kriging (fitted model, 16 neighbours), inverse distance weighting with exponent 1, 2 and 3 and locally weighted
regression -- all on the same ten random folds, and again leaving out a ball of radius 5 around every sample.
python examples/compare_estimators.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}

# 600 scattered samples of a field with a spherical variogram of range 30 (drawn with plain numpy)
rng = np.random.default_rng(7)
x = rng.uniform(0.0, 100.0, (600, 2))
h = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)) / 30.0
cov = np.where(h < 1.0, 1.0 - (1.5 * h - 0.5 * h ** 3), 0.0)
z = np.linalg.cholesky(cov + 1e-10 * np.eye(600)) @ rng.normal(size=600)
data = gss.georef({"z": z}, x)
problem = gss.EstimationProblem(data, gss.PointSet(x[:1]), "z")       # the domain of the problem is not used

g = gss.EmpiricalVariogram(data, "z", nlags=15, maxlag=45.0)
fitted = gss.fit([gss.SphericalVariogram, gss.ExponentialVariogram], g)

solvers = {"kriging, 16 neighbours": gss.KrigingSolver(z=dict(variogram=fitted, maxneighbors=16)),
           "idw exponent 1, 16 neighbours": gss.IDWSolver(z=dict(exponent=1, maxneighbors=16)),
           "idw exponent 2, 16 neighbours": gss.IDWSolver(z=dict(exponent=2, maxneighbors=16)),
           "idw exponent 3, 16 neighbours": gss.IDWSolver(z=dict(exponent=3, maxneighbors=16)),
           "idw exponent 2, every sample": gss.IDWSolver(z=dict(exponent=2)),
           "lwr, 16 neighbours": gss.LWRSolver(z=dict(maxneighbors=16))}
methods = {"10 folds": lambda: gss.KFoldValidation(10, rng=1), "ball of 5": lambda: gss.LeaveBallOut(5.0)}

print("%-32s" % "cverror" + "".join("%12s" % m for m in methods))
for name, solver in solvers.items():
    out[name] = {m: gss.cverror(solver, problem, make())["z"] for m, make in methods.items()}
    print("%-32s" % name + "".join("%12.4f" % out[name][m] for m in methods))
