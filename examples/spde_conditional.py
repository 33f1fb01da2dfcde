"""SPDEGS with data: 40 stations on the unit sphere (an icosphere of three subdivisions, 642 vertices), the ensemble
conditioned on them and the kriging mean.

    python examples/spde_conditional.py

`condition="element"` makes the value of every triangle that holds a station equal to the station's value in every
realisation; `error_variance` turns the stations into noisy observations and `condition="point"` constrains the
piecewise linear field at the stations instead ("SPDEGS").
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gss                                      # noqa: E402


def icosphere(subdivisions):
    """Unit icosphere: 10 * 4^s + 2 vertices, 20 * 4^s triangles."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    V = [np.array(v, dtype=np.float64) / math.sqrt(1.0 + g * g) for v in
         [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1),
          (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]]
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(subdivisions):
        mid, T2 = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in T:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            T2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = T2
    return np.array(V), np.array(T, dtype=np.int64)


SILL, RANGE, NREALS, SEED, NSTATIONS, MEAN = 1.5, 0.3, 8, 2024, 40, 10.0
vertices, triangles = icosphere(3)
mesh = gss.SimpleMesh(vertices, triangles)

# stations: points on the sphere, at most one per triangle; their values come from a smooth "truth"
rng = np.random.default_rng(7)
x = rng.normal(size=(400, 3))
x /= np.linalg.norm(x, axis=1)[:, None]
where, _ = mesh.locate(x)
_, first = np.unique(where, return_index=True)
keep = np.sort(first)[:NSTATIONS]
stations, station_triangle = x[keep], where[keep]
truth = MEAN + SILL * np.sin(3.0 * stations[:, 0]) * np.cos(2.0 * stations[:, 2])
data = gss.georef({"z": truth}, stations)
print(f"icosphere: {mesh.nvertices} vertices, {mesh.nelements()} triangles, {len(stations)} stations")

params = ("z", dict(sill=SILL, range=RANGE))
sol = gss.solve(gss.SimulationProblem(data, mesh, ("z", float), NREALS),
                gss.SPDEGS(params, rng=SEED, noise="lumped", condition="element", mean=MEAN))
elements = np.stack(sol["z"])
misfit = float(np.max(np.abs(elements[:, station_triangle] - truth)))
print(f"largest |realisation - datum| at the stations' triangles: {misfit:.2e}")

mean = np.asarray(gss.solve(gss.EstimationProblem(data, mesh, "z"),
                            gss.SPDEKriging(params, noise="lumped", condition="element", mean=MEAN))["z"])
away = np.setdiff1d(np.arange(mesh.nelements()), station_triangle)
spread = float(elements[:, away].std(axis=0).mean())
print(f"kriging mean: {mean.min():.2f} .. {mean.max():.2f}; mean spread of the ensemble away from the stations: {spread:.2f}")

noisy = np.stack(gss.solve(gss.SimulationProblem(data, mesh, ("z", float), NREALS),
                           gss.SPDEGS(params, rng=SEED, noise="lumped", condition="element", mean=MEAN,
                                      error_variance=0.25))["z"])
noisy_misfit = float(np.abs(noisy[:, station_triangle] - truth).mean())
print(f"with an error variance of 0.25 the mean |realisation - datum| there is {noisy_misfit:.2f}")
out = dict(elements=elements, mean=mean, misfit=misfit, spread=spread, noisy_misfit=noisy_misfit, truth=truth,
           station_triangle=station_triangle, sill=SILL, prior_mean=MEAN)
