"""SPDEGS on a curved domain: Gaussian fields on the unit sphere (an icosphere of three subdivisions, 642 vertices).

    python examples/spde_sphere.py

`noise="lumped"` draws Lindgren's w ~ N(0, inv(M)), whose vertex variance does not depend on the vertex areas; the
reference's form (`noise="reference"`, the default of the front end) scales it with them ("SPDEGS").
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
from gss.engine import SPDEHandle               # noqa: E402


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


SILL, RANGE, NREALS, SEED = 1.5, 0.3, 8, 2024
vertices, triangles = icosphere(3)
mesh = gss.SimpleMesh(vertices, triangles)
print(f"icosphere: {mesh.nvertices} vertices, {mesh.nelements()} triangles")

# the front end: one value per triangle, as the reference returns them
sol = gss.solve(gss.SimulationProblem(mesh, ("z", float), NREALS),
                gss.SPDEGS(("z", dict(sill=SILL, range=RANGE)), rng=SEED, noise="lumped"))
elements = np.stack(sol["z"])

# the handle underneath: vertex values and what the solver did for every realisation
h = SPDEHandle(vertices, triangles, sill=SILL, range=RANGE, noise="lumped")
values, iterations = [], []
for r in range(NREALS):
    v, e = h.realize(SEED, r, 1, vertices=True)
    assert np.array_equal(e[0], elements[r])             # a realisation depends on (seed, r) and the mesh only
    values.append(v[0])
    iterations.append(h.last_solve()[0])
h.close()
values = np.stack(values)
variance = float((values ** 2).mean())
print(f"sample variance over {NREALS} x {mesh.nvertices} vertex values: {variance:.3f}   (sill^2 = {SILL ** 2:.3f})")
print("CG iterations per realisation:", iterations)
out = dict(elements=elements, values=values, variance=variance, iterations=iterations, sill2=SILL ** 2)
