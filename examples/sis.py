#!/usr/bin/env python3
"""Facies by categorical sequential indicator simulation conditioned on a few wells, then porosity by CookieCutter with
one FFTGS solver per facies: facies proportions and the per-facies porosity means.
python examples/sis.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}

# 0. twelve wells on a 64 x 64 grid, each with a facies label
rng = np.random.default_rng(3)
wells = rng.uniform(2.0, 62.0, (12, 2))
labels = np.array(["sand", "shale", "silt"])
facies_at_wells = labels[np.where(wells[:, 0] < 25.0, 0, np.where(wells[:, 1] < 32.0, 1, 2))]
data = gss.georef({"facies": facies_at_wells}, wells)
grid = gss.CartesianGrid(64, 64)
nreals = 8

# 1. the facies simulator: median indicator form, one indicator variogram, the proportions of the wells by default
proportions = [0.45, 0.35, 0.20]
facies = gss.SISSolver(("facies", dict(categories=labels, variogram=gss.SphericalVariogram(range=20.0, nugget=0.05),
                                       proportions=proportions, maxneighbors=16, path=("random", 11))), rng=7)

# 2. porosity inside every facies: its own mean and continuity
poro = {
    "sand": gss.FFTGS(("poro", dict(variogram=gss.ExponentialVariogram(range=12.0, sill=4e-4), mean=0.28)), rng=1),
    "shale": gss.FFTGS(("poro", dict(variogram=gss.GaussianVariogram(range=6.0, sill=1e-4), mean=0.08)), rng=2),
    "silt": gss.FFTGS(("poro", dict(variogram=gss.SphericalVariogram(range=9.0, sill=2e-4), mean=0.15)), rng=3),
}
solver = gss.CookieCutter(facies, poro)
print(solver.describe())
sol = gss.solve(gss.SimulationProblem(data, grid, (("facies", str), ("poro", float)), nreals), solver)

f = np.stack(sol["facies"])
p = np.stack([np.asarray(r) for r in sol["poro"]])
out["facies"], out["poro"] = f, p
cells = np.floor(wells[:, 0]).astype(int) + 64 * np.floor(wells[:, 1]).astype(int)      # unit cells: the one that holds a well
assert np.all(f[:, cells] == facies_at_wells[None, :])                      # the wells are honoured
assert not np.isnan(p).any()                                                # every facies has a porosity solver
for lab, target in zip(labels, proportions):
    frac, mean = np.mean(f == lab), p[f == lab].mean()
    out[lab] = (frac, mean)
    print("%-5s  proportion %.3f (global %.2f)   mean porosity %.3f" % (lab, frac, target, mean))
assert out["sand"][1] > out["silt"][1] > out["shale"][1]
