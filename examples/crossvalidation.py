#!/usr/bin/env python3
"""Does the fitted model predict the samples it was fitted to?  Empirical variogram -> fit -> cross-validation of
candidate models on the samples themselves, under the global neighbourhood (leave-one-out and ten random folds, both off
the factor of the fitted system) and under a moving neighbourhood (ten random folds, blocks, leave-ball-out).
python examples/crossvalidation.py   (needs the built library and an MI355X)"""
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

# 1. a model fitted to the empirical variogram, the model the samples were drawn from, and a range far too short
g = gss.EmpiricalVariogram(data, "z", nlags=15, maxlag=45.0)
fitted = gss.fit([gss.SphericalVariogram, gss.ExponentialVariogram], g)
models = {"fitted": fitted, "simulated_from": gss.SphericalVariogram(range=30.0),
          "short_range": gss.SphericalVariogram(range=3.0)}
print("fitted   %s  sill %.4f  nugget %.4f  range %.2f" % (fitted.kind, fitted.sill, fitted.nugget, fitted.range))

# 2. global neighbourhood: leave-one-out costs one pass over the factor, not 600 refits
out["loo"] = {}
for name, model in models.items():
    s = gss.cross_validate(data, gss.KrigingSolver(z=dict(variogram=model)))["z"].summary
    out["loo"][name] = s
    print("%-15s leave-one-out  me %+.4f  mse %.4f  mean e/s %+.4f  mean (e/s)^2 %.3f" % (name, s.me, s.mse, s.mean_std, s.msq_std))

# 3. global neighbourhood, ten random folds of 60 samples: still the one factor, not ten refits
out["global folds"] = {}
for name, model in models.items():
    e = gss.cverror(gss.KrigingSolver(z=dict(variogram=model)), gss.EstimationProblem(data, gss.PointSet(x[:1]), "z"),
                    gss.KFoldValidation(10, rng=1))["z"]
    out["global folds"][name] = e
    print("%-15s global neighbourhood, 10 folds  cverror %.4f" % (name, e))

# 4. moving neighbourhood: folds, blocks, leave-ball-out
problem = gss.EstimationProblem(data, gss.PointSet(x[:1]), "z")       # the domain of the problem is not used
out["cverror"] = {}
for name, model in models.items():
    solver = gss.KrigingSolver(z=dict(variogram=model, maxneighbors=16))
    e = {"10 folds": gss.cverror(solver, problem, gss.KFoldValidation(10, rng=1))["z"],
         "blocks of 20": gss.cverror(solver, problem, gss.BlockValidation(20.0))["z"],
         "ball of 5": gss.cverror(solver, problem, gss.LeaveBallOut(5.0))["z"]}
    out["cverror"][name] = e
    print("%-15s cverror  " % name + "   ".join("%s %.4f" % kv for kv in e.items()))
