#!/usr/bin/env python3
"""What a coregionalisation model is fitted for: a sparsely sampled primary variable (cu) estimated with the help of a
densely sampled secondary one (zn).  Two co-simulated fields with a known correlation are sampled -- zn at 1 200 cells,
cu at 250 of them --, their direct and cross variograms are computed in one pass (EmpiricalCrossVariogram), the linear
model of coregionalisation is fitted (fit_lmc) and handed to CoKrigingSolver.  Beside it, KrigingSolver estimates cu
from its own samples alone under the same direct model, lmc.variogram("cu").  Cokriging sees the same data plus more
under one valid model, so its kriging variance cannot be larger.
python examples/cokriging.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}

# 1. two fields with correlation 0.8; zn is sampled densely, cu only at a fifth of those cells
grid = gss.CartesianGrid(48, 48)
truth = gss.LUGS(("cu", dict(variogram=gss.SphericalVariogram(range=14.0))),
                 ("zn", dict(variogram=gss.SphericalVariogram(range=14.0))),
                 (("cu", "zn"), dict(correlation=0.8)), rng=2025)
ens = gss.solve(gss.SimulationProblem(grid, {"cu": float, "zn": float}, 1), truth)
rng = np.random.default_rng(3)
cells = np.sort(rng.choice(48 * 48, 1200, replace=False))
cu = np.asarray(ens["cu"][0])[cells].copy()
cu[rng.permutation(1200)[250:]] = np.nan                       # missing rows: heterotopic data in one table
data = gss.georef({"cu": cu, "zn": np.asarray(ens["zn"][0])[cells]}, grid.centroids()[cells])

# 2. direct and cross variograms (on the rows where both exist) and the coregionalisation model
g = gss.EmpiricalCrossVariogram(data, ["cu", "zn"], nlags=12, maxlag=24.0)
lmc = gss.fit_lmc(gss.SphericalVariogram, g)
out["lmc"] = lmc
print("fitted range %.2f, correlation %.3f" % (lmc.range, lmc.correlation("cu", "zn")))

# 3. cokriging of both variables from all the samples
co = gss.solve(gss.EstimationProblem(data, grid, ("cu", "zn")),
               gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, variant="ordinary"))))
# 4. kriging of cu from its own 250 samples under the same direct model
alone = gss.solve(gss.EstimationProblem(data, grid, "cu"), gss.KrigingSolver(("cu", dict(variogram=lmc.variogram("cu")))))
out["cokriging"], out["kriging"] = co, alone

print("mean kriging variance of cu: cokriging %.6f, kriging alone %.6f"
      % (float(np.mean(co["cu_variance"])), float(np.mean(alone["cu_variance"]))))
t = np.asarray(ens["cu"][0])
print("mean squared error of cu against the simulated field (one realisation, not a bar): cokriging %.4f, kriging "
      "alone %.4f" % (float(np.mean((co["cu"] - t) ** 2)), float(np.mean((alone["cu"] - t) ** 2))))
