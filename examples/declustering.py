#!/usr/bin/env python3
"""Preferentially sampled data: declustering weights -> the declustered mean against the naive one -> a normal-score
transform that knows the weights.
python examples/declustering.py   (needs the built library and an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd")]
import numpy as np  # noqa: E402

import gss  # noqa: E402

out = {}

# 0. a 100 x 100 field whose rich zone (a bump of grade 8 on a background of 1) was drilled on a tight pattern: 400 of
#    the 520 holes sit in the bump, the rest on a regular exploration grid.  The true mean of the field is known
rng = np.random.default_rng(1)
grade = lambda p: 1.0 + 7.0 * np.exp(-((p[:, 0] - 30.0) ** 2 + (p[:, 1] - 60.0) ** 2) / (2.0 * 8.0 ** 2))
infill = np.array([30.0, 60.0]) + 6.0 * rng.standard_normal((400, 2))
regular = np.stack(np.meshgrid(np.arange(5.0, 100.0, 9.0), np.arange(5.0, 100.0, 9.0)), axis=-1).reshape(-1, 2)[:120]
coords = np.concatenate([infill, regular])
values = grade(coords) * np.exp(0.1 * rng.standard_normal(len(coords)))
data = gss.georef({"grade": values}, coords)
cells = np.stack(np.meshgrid(np.arange(100) + 0.5, np.arange(100) + 0.5), axis=-1).reshape(-1, 2)
true_mean = float(grade(cells).mean())
out["naive_mean"] = float(values.mean())
print("naive mean        %.3f   (true mean of the field %.3f)" % (out["naive_mean"], true_mean))

# 1. cell declustering: 24 sizes x 8 origin offsets on the device, the size with the lowest declustered mean wins
w = gss.weight(data, gss.CellDeclustering(2.0, 40.0, ncell=24, noffsets=8, criterion="min"), "grade")
out["weights"] = np.asarray(w)
out["declustered_mean"] = gss.wmean(values, w)
print("declustered mean  %.3f   cell size %.1f (of %d tried); weights %.3f .. %.3f"
      % (out["declustered_mean"], w.sizes[w.best], len(w.sizes), w.min(), w.max()))
print("                  std %.3f against the naive %.3f; median %.3f against %.3f"
      % (np.sqrt(gss.wvar(values, w)), values.std(), gss.wquantile(values, w, 0.5), np.median(values)))
assert abs(out["declustered_mean"] - true_mean) < 0.5 * abs(out["naive_mean"] - true_mean)

# 2. the other two methods on the same table: one block size, and polygons of influence on a 400 x 400 lattice
wb = gss.weight(data, gss.BlockWeighting(9.0, 9.0), "grade")
wp = gss.weight(data, gss.PolygonalWeighting((400, 400), allow_zero=True), "grade")
out["block_mean"], out["polygonal_mean"] = gss.wmean(values, wb), gss.wmean(values, wp)
print("block weighting   %.3f   polygonal %.3f (%d samples without a lattice point)"
      % (out["block_mean"], out["polygonal_mean"], wp.nzero))

# 3. the weights go into the normal-score fit: the scores of the declustered histogram are standard normal under the
#    weights, not under equal counting
ns = gss.NormalScore.fit(values, weights=w)
scores = ns.forward(values)
out["scores"] = scores
out["score_wmean"] = gss.wmean(scores, w)
print("scores            weighted mean %.3f, weighted variance %.3f; unweighted mean %.3f"
      % (out["score_wmean"], gss.wvar(scores, w), scores.mean()))
ns.close()
