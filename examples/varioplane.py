#!/usr/bin/env python3
"""Finding the direction of continuity from the data: a field simulated from a rotated anisotropic model (FFTGS), random
cells as samples, the varioplane of the samples in ONE pass over the pairs, the anisotropic fit, and kriging with the
fitted rotated ball.  Truth and fit are printed side by side; they belong to one realisation.
python examples/varioplane.py   (needs the built library and an MI355X)"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}
R1, R2, THETA = 40.0, 12.0, math.radians(30.0)

# 1. one unconditional realisation of an exponential model whose long axis points 30 degrees from the first axis
truth = gss.ExponentialVariogram(gss.MetricBall((R1, R2), THETA))
grid = gss.CartesianGrid(512, 512)
ens = gss.solve(gss.SimulationProblem(grid, ("z", float), 1), gss.FFTGS(("z", dict(variogram=truth)), rng=2025))
field = np.asarray(ens["z"][0])

# 2. 20 000 random cells are the samples
cells = np.sort(np.random.default_rng(7).choice(512 * 512, 20000, replace=False))
data = gss.georef({"z": field[cells]}, grid.centroids()[cells])

# 3. the varioplane: 18 sectors of 10 degrees, 20 lags to 80, every sector from the same pass over the pairs
plane = gss.EmpiricalVarioplane(data, "z", nangs=18, nlags=20, maxlag=80.0)
out["plane"] = plane
first = plane.ordinate[:, :6].mean(axis=1)
print("sector mid-angle (deg):", np.round(np.degrees(plane.midangles)).astype(int))
print("mean gamma, lags < 24 :", np.round(first, 3))

# 4. the anisotropic fit returns a model with a rotated ball
model, obj = gss.fit_anisotropic(gss.ExponentialVariogram, plane, return_objectives=True)
out["model"] = model
r1, r2 = model.radii if model.radii is not None else (model.range, model.range)
theta = math.atan2(model.rotation[1][0], model.rotation[0][0]) % math.pi if model.rotation is not None else 0.0
print("truth: kind=exponential r1=%.3f r2=%.3f theta=%.4f ratio=%.4f azimuth_deg=%.2f sill=1 nugget=0"
      % (R1, R2, THETA, R2 / R1, math.degrees(THETA)))
print("fit: kind=%s r1=%.3f r2=%.3f theta=%.4f ratio=%.4f azimuth_deg=%.2f sill=%.4f nugget=%.4f"
      % (model.kind, r1, r2, theta, r2 / r1, math.degrees(theta), model.sill, model.nugget))

# 5. and goes into kriging like any other model
sub = gss.georef({"z": field[cells[:1500]]}, grid.centroids()[cells[:1500]])
sol = gss.solve(gss.EstimationProblem(sub, gss.CartesianGrid(64, 64), "z"),
                gss.KrigingSolver(("z", dict(variogram=model, maxneighbors=16))))
out["kriging"] = (sol["z"], sol["z_variance"])
assert np.isfinite(sol["z"]).all() and (sol["z_variance"] > -1e-9).all()
print("kriging ok: mean[0:3] = %s   variance[0:3] = %s" % (np.round(sol["z"][:3], 4), np.round(sol["z_variance"][:3], 4)))
