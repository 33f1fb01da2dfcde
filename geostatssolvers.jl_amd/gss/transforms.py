"""Normal scores: skewed data into Gaussian space before a Gaussian simulator, and the realisations back.

`NormalScore` is GSLIB's nscore / backtr and the reversible `Quantile()` step of a GeoStats pipeline: the fit is a
sort on the host, the transform itself one fused device kernel over the whole ensemble (gss.h, gss_nscore_*).
`InNormalScores` wraps a simulation solver so that `gss.solve` takes data and returns realisations in the data's units.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .engine import default_engine
from .geo import Ensemble, GeoTable
from .problems import SimulationProblem


class NormalScore:
    """A fitted normal-score transform of one variable.

    `NormalScore.fit(values, weights=None, tails=None, tail_power=(1.0, 1.0))`: rows whose value is NaN are dropped
    (with their weights); equal values are merged into one class, not despiked; `weights` (finite, > 0) are what a
    declustering step supplies -- `gss.weight(data, method, var)` marks the rows it left out (NaN in `var`) with a NaN
    weight, and those are exactly the rows dropped here, so its result goes in as it is; `tails = (zmin, zmax)` are the
    bounds the back-transform extrapolates to below the
    smallest and above the largest datum (None: clamp at the datum) and `tail_power` the exponents of the GSLIB
    power model on either side (1: linear).  The device tables are built at the first transform."""

    def __init__(self, values, weights, tails, tail_power, engine=None):
        self.values, self.weights, self.tails, self.tail_power = values, weights, tails, tail_power
        self._engine = engine
        self._handle = None

    @classmethod
    def fit(cls, values, weights=None, tails=None, tail_power=(1.0, 1.0), engine=None):
        z = np.asarray(values, dtype=np.float64).ravel()
        keep = ~np.isnan(z)
        w = None
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64).ravel()
            if w.size != z.size:
                raise ValueError(f"{w.size} weights for {z.size} values")
            w = w[keep]
        z = z[keep]
        if z.size == 0:
            raise AssertionError("all values are missing, aborting...")       # as KrigingSolver does (krig.jl:100-102)
        if not np.all(np.isfinite(z)):
            raise ValueError("values must be finite (NaN marks a missing row)")
        if w is not None and not (np.all(np.isfinite(w)) and np.all(w > 0.0)):
            raise ValueError("weights must be finite and positive")
        lo, hi = (None, None) if tails is None else tails
        lo = None if lo is None or np.isnan(lo) else float(lo)
        hi = None if hi is None or np.isnan(hi) else float(hi)
        if lo is not None and not (np.isfinite(lo) and lo <= z.min()):
            raise ValueError(f"tails: zmin = {lo} lies above the smallest value {z.min()}")
        if hi is not None and not (np.isfinite(hi) and hi >= z.max()):
            raise ValueError(f"tails: zmax = {hi} lies below the largest value {z.max()}")
        plo, phi = (float(p) for p in tail_power)
        if not (np.isfinite(plo) and plo > 0.0 and np.isfinite(phi) and phi > 0.0):
            raise ValueError("tail_power: both exponents must be finite and > 0")
        return cls(z, w, (lo, hi), (plo, phi), engine)

    @property
    def handle(self):
        if self._handle is None:
            eng = self._engine or default_engine()
            self._handle = eng.nscore(self.values, weights=self.weights, tails=self.tails, tail_power=self.tail_power)
        return self._handle

    @property
    def bounds(self):
        """(zmin, zmax): every back-transformed value lies between them."""
        lo, hi = self.tails
        return (float(self.values.min()) if lo is None else lo, float(self.values.max()) if hi is None else hi)

    def table(self):
        """(v, y): the distinct values and their scores."""
        return self.handle.table()

    def forward(self, x, out=None):
        """Values to scores (numpy array or CUDA tensor of any shape; NaN stays NaN)."""
        return self.handle.forward(x, out=out)

    def inverse(self, y, out=None):
        """Scores to values."""
        return self.handle.inverse(y, out=out)

    def apply(self, geotable: GeoTable, var: str) -> GeoTable:
        """A new table over the same domain whose column `var` is in scores (missing rows stay NaN): what variography
        and the model fit for a simulation in normal scores are run on."""
        cols = dict(geotable.table)
        cols[var] = self.forward(np.asarray(geotable[var], dtype=np.float64))
        return GeoTable(cols, geotable.domain)

    def revert(self, ensemble: Ensemble, var: str) -> Ensemble:
        """A new Ensemble whose realisations of `var` are back in the data's units; the other variables are shared with
        `ensemble`, not copied.  The realisations may be a list of vectors, or one (nreals, N) array or CUDA tensor --
        also a strided view of a co-simulation's (nreals, nz, N) output, which is then read where it lies."""
        r = ensemble.reals[var]
        if isinstance(r, (list, tuple)):
            z = self.inverse(np.stack([np.asarray(x, dtype=np.float64) for x in r])) if len(r) else []
            z = [z[i] for i in range(len(r))]
        else:
            z = self.inverse(r)
        reals = dict(ensemble.reals)
        reals[var] = z
        return Ensemble(ensemble.domain, reals)

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None


class InNormalScores:
    """`InNormalScores(solver, cu=None, au=ns)`: run a simulation solver in normal scores.

    For every named variable the data column of the problem is taken to scores (with the given `NormalScore`, or with
    one fitted to that column when the value is None), the wrapped solver runs untouched on the transformed problem,
    and the named variables of its ensemble are reverted.  A variable without data in the problem is simulated
    unconditionally and only reverted, which needs a given transform.

    The wrapped solver works in score units: its `variogram` (or joint `model`) and `mean` describe the scores, not the
    data -- run the variography and the fit on `NormalScore.apply(data, var)`, and leave `mean` at 0.

    Only simulation solvers are accepted.  An estimation solver is refused: a kriging mean is an expectation in score
    space, and the back-transform of an expectation is not the expectation of the back-transform -- it is biased."""

    def __init__(self, solver, **transforms):
        if not hasattr(solver, "solvesingle"):
            raise TypeError(f"{type(solver).__name__} is not a simulation solver: the back-transform of an estimate "
                            f"(a kriging mean) is biased, so estimation in normal scores is refused; for the local "
                            f"distribution of skewed data use IndicatorKrigingSolver and postik")
        if not transforms:
            raise ValueError("InNormalScores needs at least one variable: InNormalScores(solver, z=None)")
        for var, t in transforms.items():
            if t is not None and not isinstance(t, NormalScore):
                raise TypeError(f"variable {var}: a NormalScore or None (fit from the problem's data), not "
                                f"{type(t).__name__}")
        self.solver = solver
        self.transforms = dict(transforms)
        self.fitted = {}

    def solve(self, problem: SimulationProblem, gather: bool = True) -> Ensemble:
        if not isinstance(problem, SimulationProblem):
            raise TypeError("InNormalScores solves SimulationProblems only: the back-transform of an estimate is biased")
        unknown = [v for v in self.transforms if v not in problem.variables]
        if unknown:
            raise ValueError(f"variables {unknown} are not among the problem's variables {problem.variables}")
        data: Optional[GeoTable] = problem.data
        used = {}
        for var, t in self.transforms.items():
            col = data.table.get(var) if data is not None else None
            if t is None:
                if col is None:
                    raise ValueError(f"variable {var} has no data in the problem to fit a transform from: pass a fitted "
                                     f"NormalScore")
                t = NormalScore.fit(col, engine=self.solver.globals.get("engine"))
            used[var] = t
            if col is not None:
                data = t.apply(data, var)
        self.fitted = used
        if data is not None:
            inner = SimulationProblem(data, problem.domain, tuple(problem.variables), problem.nreals)
        else:
            inner = SimulationProblem(problem.domain, tuple(problem.variables), problem.nreals)
        ens = self.solver.solve(inner, gather=gather)
        for var, t in used.items():
            ens = t.revert(ens, var)
        return ens
