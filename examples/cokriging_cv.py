#!/usr/bin/env python3
"""Cross-validation of a cokriging model: does the secondary variable lower the error of the primary one, and how many
neighbours of each variable are worth searching?  The inputs are those of examples/cokriging_local.py: a sparse primary
variable (cu, 2 000 samples) beside a dense secondary one (zn, 20 000 samples), a coregionalisation model fitted to
their direct and cross variograms.  `cverror` then predicts every sample from samples at OTHER locations -- 10 folds of
locations, so the zn value that sits on a cu sample never helps to predict it -- by kriging of cu alone and by
cokriging, for two `maxneighbors` settings.  22 000 stacked samples are far beyond the global neighbourhood (an O(n^3)
fit and an n^2 factor); the moving neighbourhood needs neither.
python examples/cokriging_cv.py   (needs the built library and an MI355X)"""
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


# 1. the samples and the model of examples/cokriging_local.py
x = rng.uniform(0.0, 200.0, (20000, 2))
zn = field(1, x) + 0.1 * rng.normal(size=20000)
cu = 0.8 * field(1, x) + 0.6 * field(2, x) + 0.1 * rng.normal(size=20000)
cu[rng.permutation(20000)[2000:]] = np.nan
data = gss.georef({"cu": cu, "zn": zn}, x)
g = gss.EmpiricalCrossVariogram(data, ["cu", "zn"], nlags=15, maxlag=45.0)
lmc = gss.fit_lmc(gss.SphericalVariogram, g)
print("fitted range %.2f, correlation %.3f" % (lmc.range, lmc.correlation("cu", "zn")))

# 2. 10 folds: of the cu samples for kriging alone, of the locations for cokriging
grid = gss.CartesianGrid((2, 2), (0.0, 0.0), (100.0, 100.0))       # cross-validation reads the data only
for nmax in (8, 16):
    alone = gss.cverror(gss.KrigingSolver(("cu", dict(variogram=lmc.variogram("cu"), maxneighbors=nmax))),
                        gss.EstimationProblem(data, grid, "cu"), gss.KFoldValidation(10, rng=11))
    co = gss.cverror(gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, variant="ordinary", maxneighbors=nmax))),
                     gss.EstimationProblem(data, grid, ("cu", "zn")), gss.KFoldValidation(10, rng=11))
    out[nmax] = dict(kriging=alone["cu"], cokriging=co["cu"], zn=co["zn"])
    print("cverror of cu, maxneighbors %2d: cokriging %.5f, kriging alone %.5f" % (nmax, co["cu"], alone["cu"]))
