#!/usr/bin/env python3
"""Skewed data through a Gaussian simulator and back: normal scores -> variography on the scores -> conditional FFTGS
in score space -> realisations in the data's units.
python examples/normalscore.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}
grid = gss.CartesianGrid(64, 64)

# 0. a lognormal "truth" (grades, permeabilities, concentrations look like this) and 120 samples of it at cell centres
truth = np.exp(gss.solve(gss.SimulationProblem(grid, "z", 1),
                         gss.FFTGS(("z", dict(variogram=gss.SphericalVariogram(range=12.0))), rng=42))["z"][0])
rng = np.random.default_rng(0)
cells = rng.choice(grid.nelements(), 120, replace=False)
coords = np.stack([cells % 64 + 0.5, cells // 64 + 0.5], axis=1)
data = gss.georef({"z": truth[cells]}, coords)
vals = data["z"]
print("samples   mean %.3f  median %.3f  max %.3f  (skewed)" % (vals.mean(), np.median(vals), vals.max()))

# 1. the transform: fitted on the host, applied on the device; the table keeps the column's missing rows
ns = gss.NormalScore.fit(vals)
scores = ns.apply(data, "z")
print("scores    mean %.3f  variance %.3f" % (scores["z"].mean(), scores["z"].var()))

# 2. variography is done on the scores: the simulator's variogram and mean are in score units
g = gss.EmpiricalVariogram(scores, "z", nlags=12, maxlag=24.0)
model = gss.fit([gss.SphericalVariogram, gss.ExponentialVariogram, gss.GaussianVariogram], g)
out["model"] = model
print("fitted    %s  sill %.3f  nugget %.3f  range %.2f" % (model.kind, model.sill, model.nugget, model.range))

# 3. conditional simulation in normal scores: the wrapper forwards the data, runs FFTGS untouched, reverts the ensemble
solver = gss.InNormalScores(gss.FFTGS(("z", dict(variogram=model)), rng=2024), z=ns)
ens = gss.solve(gss.SimulationProblem(data, grid, "z", 20), solver)
z = np.stack(ens["z"])
out["ensemble"] = ens

# 4. every realisation honours the data in their own units at the data cells.  The wrapped solver honours the scores to
#    its 1e-8; a lognormal table turns a score error dy into a relative error of about sigma_log dy, ten times that
#    across the wide gaps between the extreme knots: 1e-6 holds with room
honour = float(np.max(np.abs(z[:, cells] - vals) / vals))
out["honoured"] = honour < 1e-6
print("data      honoured to %.1e (relative)" % honour)
assert out["honoured"]
assert z.min() >= vals.min() and z.max() <= vals.max()          # default tails clamp at the extreme data

# 5. the pooled histogram of the ensemble has the data's quantiles.  Compared in score units: 20 realisations of
#    (64 / range)^2 independent patches put a quantile's standard error near 0.05, and a fitted sill within 20 % of 1
#    moves the 10 % and 90 % quantiles by 1.28 (sqrt(1.2) - 1) = 0.12: 0.35 is four standard errors beyond that
probs = np.array([0.1, 0.25, 0.5, 0.75, 0.9])
qe, qd = np.quantile(z, probs), np.quantile(vals, probs)
gap = float(np.max(np.abs(ns.forward(qe) - ns.forward(qd))))
out["quantiles"] = (qe, qd)
out["quantiles_ok"] = gap < 0.35
print("quantiles ensemble", np.round(qe, 3))
print("          data    ", np.round(qd, 3), " largest gap %.3f score units" % gap)
assert out["quantiles_ok"]
