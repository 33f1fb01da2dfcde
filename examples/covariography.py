#!/usr/bin/env python3
"""Where the `correlation` of a LUGS co-simulation comes from: two co-simulated fields with a known correlation are
sampled, their direct and cross variograms are computed in one pass over the pairs (EmpiricalCrossVariogram), the
linear model of coregionalisation is fitted to them (fit_lmc), and the fitted direct models and the fitted correlation
go back into LUGS.  The printed comparison is one realisation, not a bar.
python examples/covariography.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}
TRUE_RHO, TRUE_RANGE = 0.7, 12.0

# 1. two fields with a known correlation (LUGS, 48 x 48 cells, both spherical with range 12)
grid = gss.CartesianGrid(48, 48)
truth = gss.LUGS(("z", dict(variogram=gss.SphericalVariogram(range=TRUE_RANGE))),
                 ("y", dict(variogram=gss.SphericalVariogram(range=TRUE_RANGE))),
                 (("z", "y"), dict(correlation=TRUE_RHO)), rng=2024)
ens = gss.solve(gss.SimulationProblem(grid, {"z": float, "y": float}, 1), truth)
cells = np.sort(np.random.default_rng(5).choice(48 * 48, 1200, replace=False))
data = gss.georef({"z": np.asarray(ens["z"][0])[cells], "y": np.asarray(ens["y"][0])[cells]}, grid.centroids()[cells])

# 2. direct and cross variograms in one pass over the pairs
g = gss.EmpiricalCrossVariogram(data, ["z", "y"], nlags=12, maxlag=24.0)
out["cross"] = g
print("lag        ", np.round(g.abscissa, 2))
print("gamma_zz   ", np.round(g.gamma("z", "z"), 3))
print("gamma_zy   ", np.round(g.gamma("z", "y"), 3))
print("gamma_yy   ", np.round(g.gamma("y", "y"), 3))

# 3. the linear model of coregionalisation: one structure, positive semidefinite nugget and sill matrices
lmc = gss.fit_lmc(gss.SphericalVariogram, g)
out["lmc"] = lmc
rho = lmc.correlation("z", "y")
print("fitted range %.3f (true %.1f)" % (lmc.range, TRUE_RANGE))
print("fitted sills z %.3f  y %.3f (true 1, 1)" % (lmc.variogram("z").sill, lmc.variogram("y").sill))
print("fitted correlation %.3f (true %.2f)" % (rho, TRUE_RHO))

# 4. back into the solver: the fitted direct models and the fitted correlation
again = gss.LUGS(("z", dict(variogram=lmc.variogram("z"))), ("y", dict(variogram=lmc.variogram("y"))),
                 (("z", "y"), dict(correlation=rho)), rng=7)
sim = gss.solve(gss.SimulationProblem(gss.CartesianGrid(32, 32), {"z": float, "y": float}, 2), again)
out["simulation"] = sim
print("co-simulation with the fitted model: sample correlation of the first realisation %.3f"
      % np.corrcoef(np.asarray(sim["z"][0]), np.asarray(sim["y"][0]))[0, 1])
