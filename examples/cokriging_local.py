#!/usr/bin/env python3
"""Moving-neighbourhood cokriging: a sparse primary variable (cu, 2 000 samples) beside a dense secondary one (zn,
20 000 samples) -- 22 000 stacked samples, far more than the global neighbourhood is meant for (its fit is O(n^3) and
its factor holds n^2 doubles).  Two correlated fields are drawn as sums of random cosines, sampled at scattered
locations, their direct and cross variograms computed in one pass and a linear model of coregionalisation fitted to them
(fit_lmc).  CoKrigingSolver then estimates both variables on a 200 x 200 grid from the 16 nearest samples of EACH
variable, searched separately (one joint search of 32 would return zn almost exclusively).  Beside it KrigingSolver
estimates cu from its own 16 nearest samples under the same direct model: cokriging sees those samples plus 16 more
under one valid model, so its kriging variance cannot be larger.
python examples/cokriging_local.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}
rng = np.random.default_rng(7)


def field(seed, x, scale=12.0, terms=200):
    """A stationary random field with a smooth covariance of range ~ 2 `scale`: a sum of random cosines."""
    r = np.random.default_rng(seed)
    w = r.normal(scale=1.0 / scale, size=(terms, 2))
    ph = r.uniform(0.0, 2.0 * np.pi, terms)
    return np.sqrt(2.0 / terms) * np.cos(x @ w.T + ph).sum(axis=1)


# 1. zn at 20 000 scattered locations, cu at 2 000 of them; cu = 0.8 zn + 0.6 (an independent field)
x = rng.uniform(0.0, 200.0, (20000, 2))
zn = field(1, x) + 0.1 * rng.normal(size=20000)
cu = 0.8 * field(1, x) + 0.6 * field(2, x) + 0.1 * rng.normal(size=20000)
cu[rng.permutation(20000)[2000:]] = np.nan                     # missing rows: heterotopic data in one table
data = gss.georef({"cu": cu, "zn": zn}, x)

# 2. direct and cross variograms (on the rows where both exist) and the coregionalisation model
g = gss.EmpiricalCrossVariogram(data, ["cu", "zn"], nlags=15, maxlag=45.0)
lmc = gss.fit_lmc(gss.SphericalVariogram, g)
out["lmc"] = lmc
print("fitted range %.2f, correlation %.3f" % (lmc.range, lmc.correlation("cu", "zn")))

# 3. cokriging of both variables from the 16 nearest samples of each
grid = gss.CartesianGrid((200, 200), (0.0, 0.0), (1.0, 1.0))
co = gss.solve(gss.EstimationProblem(data, grid, ("cu", "zn")),
               gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, variant="ordinary", maxneighbors=16))))
# 4. kriging of cu from its own 16 nearest samples under the same direct model
alone = gss.solve(gss.EstimationProblem(data, grid, "cu"),
                  gss.KrigingSolver(("cu", dict(variogram=lmc.variogram("cu"), maxneighbors=16))))
out["cokriging"], out["kriging"] = co, alone

print("mean kriging variance of cu: cokriging %.6f, kriging alone %.6f"
      % (float(np.mean(co["cu_variance"])), float(np.mean(alone["cu_variance"]))))
c = grid.centroids()
t = 0.8 * field(1, c) + 0.6 * field(2, c)
print("mean squared error of cu against the field (one realisation, not a bar): cokriging %.4f, kriging alone %.4f"
      % (float(np.mean((co["cu"] - t) ** 2)), float(np.mean((alone["cu"] - t) ** 2))))
