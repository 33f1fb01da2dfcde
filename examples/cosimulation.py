#!/usr/bin/env python3
"""From samples of two correlated variables to joint realisations on a grid: direct and cross variograms in one pass
(EmpiricalCrossVariogram), the linear model of coregionalisation (fit_lmc), and FFTGS with the fitted model as the joint
parameter of the two variables.  Every realisation of (cu, zn) then carries the model's cross-covariance: the empirical
correlation of the two simulated fields at lag 0 is printed beside lmc.correlation.
python examples/cosimulation.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}

# 1. samples: two fields with correlation 0.8 (the reference's LUGS pair), observed at 1 500 cells
grid = gss.CartesianGrid(48, 48)
truth = gss.LUGS(("cu", dict(variogram=gss.SphericalVariogram(range=14.0))),
                 ("zn", dict(variogram=gss.SphericalVariogram(range=14.0))),
                 (("cu", "zn"), dict(correlation=0.8)), rng=2025)
ens = gss.solve(gss.SimulationProblem(grid, {"cu": float, "zn": float}, 1), truth)
cells = np.sort(np.random.default_rng(3).choice(48 * 48, 1500, replace=False))
data = gss.georef({"cu": np.asarray(ens["cu"][0])[cells], "zn": np.asarray(ens["zn"][0])[cells]},
                  grid.centroids()[cells])

# 2. direct and cross variograms and the coregionalisation model
g = gss.EmpiricalCrossVariogram(data, ["cu", "zn"], nlags=12, maxlag=24.0)
lmc = gss.fit_lmc(gss.SphericalVariogram, g)
out["lmc"] = lmc

# 3. joint realisations on a larger grid under the fitted model (unconditional)
big = gss.CartesianGrid(128, 128)
sim = gss.solve(gss.SimulationProblem(big, {"cu": float, "zn": float}, 16),
                gss.FFTGS((("cu", "zn"), dict(model=lmc)), rng=11))
out["ensemble"] = sim

cu, zn = np.stack(sim["cu"]), np.stack(sim["zn"])
out["correlation"] = float(np.mean(cu * zn) / np.sqrt(np.mean(cu * cu) * np.mean(zn * zn)))
print("fitted range %.2f; correlation of cu and zn at lag 0: model %.3f, 16 joint realisations %.3f"
      % (lmc.range, lmc.correlation("cu", "zn"), out["correlation"]))
