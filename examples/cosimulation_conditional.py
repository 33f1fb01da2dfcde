#!/usr/bin/env python3
"""Joint realisations that honour the data: a sparsely sampled primary variable (cu) and a densely sampled secondary one
(zn) in one table -- zn at 1 200 cells, cu at 250 of them --, their direct and cross variograms in one pass
(EmpiricalCrossVariogram), the linear model of coregionalisation (fit_lmc), and FFTGS with the fitted model as the
joint parameter of the two variables and the table as the problem's data.  Every realisation then equals the samples
at their cells, carries the model's cross-covariance between them, and differs from the other realisations away from
the data; the spread of cu is smallest where either variable was measured.
python examples/cosimulation_conditional.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {"nreals": 8}

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
zn = np.asarray(ens["zn"][0])[cells]
data = gss.georef({"cu": cu, "zn": zn}, grid.centroids()[cells])

# 2. direct and cross variograms (on the rows where both exist) and the coregionalisation model
g = gss.EmpiricalCrossVariogram(data, ["cu", "zn"], nlags=12, maxlag=24.0)
lmc = gss.fit_lmc(gss.SphericalVariogram, g)
out["lmc"] = lmc

# 3. joint realisations conditioned on the table: the stacked samples and every unconditional realisation at the data
#    cells are kriged by simple cokriging under the fitted model about the variables' means
means = dict(cu=float(np.nanmean(cu)), zn=float(np.mean(zn)))
sim = gss.solve(gss.SimulationProblem(data, grid, {"cu": float, "zn": float}, out["nreals"]),
                gss.FFTGS(("cu", dict(mean=means["cu"])), ("zn", dict(mean=means["zn"])),
                          (("cu", "zn"), dict(model=lmc)), rng=11))
out["ensemble"] = sim

zc, zz = np.stack(sim["cu"]), np.stack(sim["zn"])
has = ~np.isnan(cu)
out["max_misfit"] = float(max(np.max(np.abs(zc[:, cells[has]] - cu[has])), np.max(np.abs(zz[:, cells] - zn))))
spread = zc.std(axis=0)
free = np.setdiff1d(np.arange(48 * 48), cells)
print("fitted range %.2f, correlation %.3f; largest misfit at the %d cu and %d zn samples over %d realisations: %.2e"
      % (lmc.range, lmc.correlation("cu", "zn"), int(has.sum()), cells.size, out["nreals"], out["max_misfit"]))
print("spread of cu over the realisations: %.3f at its own samples, %.3f where only zn was measured, %.3f elsewhere"
      % (float(spread[cells[has]].mean()), float(spread[cells[~has]].mean()), float(spread[free].mean())))
