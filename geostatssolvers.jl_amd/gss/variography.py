"""Empirical variograms and model fitting: the step that produces the `variogram=` parameter of every solver.

Mirrors [DEP] Variography's `EmpiricalVariogram(data, var; nlags, maxlag, estimator)`,
`DirectionalVariogram(direction, data, var; dtol, ...)` and `fit(kind, g, ...)`.  That package is not in the reference
tree, so the conventions are this library's own (include/gss.h, "variography"); where they follow what Variography is
recalled to do they are marked [RECALL].  No arithmetic lives here: the pair pass runs on the device
(gss_variogram_empirical) and the fit in the library's host code (gss_variogram_fit), both through the `engine` seam.

Library defaults: `nlags = 20`; `maxlag` = a tenth of the diagonal of the samples' bounding box ([RECALL] Variography's
default); estimator "matheron"; directional: no band (`dtol = inf`) and a cone of half-angle `atol = pi / 8`.
Missing values (NaN): a pair takes part in a variable only if both of its values exist.  The device call wants finite
values, so the samples of each variable that are missing are dropped before it; variables that miss the same samples
(usually none) share one call."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .engine import default_engine
from .variograms import GAUSSIAN_NUGGET_EPS, VariogramModel

ESTIMATORS = {"matheron": 0, "cressie": 1}
WEIGHTINGS = {"count": 0, "count/h2": 1, "uniform": 2}
STATIONARY_KINDS = ("gaussian", "exponential", "spherical", "matern", "cubic", "pentaspherical", "sinehole")


@dataclass
class EmpiricalVariogramResult:
    """One variable's empirical variogram.  Bins without pairs have NaN abscissa and ordinate."""
    abscissa: np.ndarray      # mean lag of the pairs of each bin
    ordinate: np.ndarray      # gamma
    counts: np.ndarray        # pairs per bin (int64)
    nduplicates: int          # pairs at distance exactly zero (in no bin)
    maxlag: float
    estimator: str = "matheron"
    var: str = ""

    @property
    def nlags(self):
        return int(self.counts.size)


def _ordinate(estimator, zsum, count):
    c = count.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if estimator == "matheron":
            return np.where(count > 0, zsum / (2.0 * c), np.nan)
        return np.where(count > 0, (zsum / c) ** 4 / (2.0 * (0.457 + 0.494 / c)), np.nan)   # Cressie-Hawkins


def _default_maxlag(x):
    return 0.1 * float(np.sqrt(((x.max(axis=0) - x.min(axis=0)) ** 2).sum()))


def _empirical(data, var_or_vars, nlags, maxlag, estimator, direction, dtol, cos_atol, distance, engine):
    if estimator not in ESTIMATORS:
        raise ValueError(f"estimator {estimator!r}: 'matheron' or 'cressie'")
    engine = engine or default_engine()
    single = isinstance(var_or_vars, str)
    names = [var_or_vars] if single else list(var_or_vars)
    if not names:
        raise ValueError("no variable given")
    x = np.ascontiguousarray(data.domain.centroids(), dtype=np.float64)
    cols = [np.asarray(data[v], dtype=np.float64) for v in names]
    if maxlag is None:
        maxlag = _default_maxlag(x)
    groups = {}                                    # finite mask -> variables that share it
    for i, c in enumerate(cols):
        groups.setdefault(np.isfinite(c).tobytes(), []).append(i)
    out = [None] * len(names)
    for members in groups.values():
        keep = np.isfinite(cols[members[0]])
        xs = x if keep.all() else np.ascontiguousarray(x[keep])
        for lo in range(0, len(members), 8):       # gss.h: at most 8 value columns per call
            part = members[lo:lo + 8]
            z = np.ascontiguousarray(np.stack([cols[i][keep] for i in part]))
            count, lagsum, zsum, ndup = engine.variogram_empirical(xs, z, nlags, maxlag, direction, dtol, cos_atol,
                                                                   ESTIMATORS[estimator], distance=distance)
            with np.errstate(invalid="ignore", divide="ignore"):
                absc = np.where(count > 0, lagsum / count, np.nan)
            for r, i in enumerate(part):
                out[i] = EmpiricalVariogramResult(absc, _ordinate(estimator, zsum[r], count), count.copy(), int(ndup),
                                                  float(maxlag), estimator, names[i])
    return out[0] if single else dict(zip(names, out))


def EmpiricalVariogram(data, var_or_vars, nlags=20, maxlag=None, estimator="matheron", distance=None, engine=None):
    """Omnidirectional empirical variogram of one variable (-> EmpiricalVariogramResult) or of several variables of
    one table in one pass over the pairs (-> dict name -> result)."""
    return _empirical(data, var_or_vars, nlags, maxlag, estimator, None, float("inf"), 0.0, distance, engine)


def DirectionalVariogram(direction, data, var_or_vars, dtol=float("inf"), atol=math.pi / 8, nlags=20, maxlag=None,
                         estimator="matheron", distance=None, engine=None):
    """Pairs whose separation lies along `direction` (either sense): inside a band of half-width `dtol` about the
    line and inside a cone of half-angle `atol` radians (None: no cone).  `direction` is normalised here."""
    u = np.asarray(direction, dtype=np.float64).reshape(-1)
    nrm = float(np.sqrt((u * u).sum()))
    if not (nrm > 0.0 and np.isfinite(nrm)):
        raise ValueError("direction must be a non-zero finite vector")
    if atol is not None and not 0.0 <= atol <= math.pi / 2:
        raise ValueError("atol is an angle in [0, pi / 2] radians")
    cos_atol = 0.0 if atol is None or atol >= math.pi / 2 else math.cos(atol)
    return _empirical(data, var_or_vars, nlags, maxlag, estimator, u / nrm, dtol, cos_atol, distance, engine)


def _kind_name(k):
    if isinstance(k, str):
        name = k.lower()
    else:                                   # a constructor of gss.variograms (GaussianVariogram, ...)
        name = getattr(k, "__name__", "").lower().replace("variogram", "")
    if name == "power":
        return name                         # the library answers GSS_ERR_UNSUPPORTED
    if name not in STATIONARY_KINDS:
        raise ValueError(f"cannot fit {k!r}: one of {STATIONARY_KINDS} or its constructor")
    return name


def fit(kind_or_kinds, g, weighting="count", nu=1.0, max_nugget_frac=1.0, return_objectives=False, engine=None):
    """Weighted least-squares fit of one model kind, or the best of several, to an EmpiricalVariogramResult
    (gss_variogram_fit).  Returns a VariogramModel that evaluates to what was fitted and goes into every solver.
    A Gaussian model is evaluated with `nugget + 1e-6` unless told otherwise (variograms.py): the fitted nugget
    n is returned as `nugget = n - 1e-6`, or, when n < 1e-6, as `nugget = n` with `regularize=False`."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting {weighting!r}: one of {tuple(WEIGHTINGS)}")
    engine = engine or default_engine()
    kinds = [kind_or_kinds] if isinstance(kind_or_kinds, str) or callable(kind_or_kinds) else list(kind_or_kinds)
    names = [_kind_name(k) for k in kinds]
    kind, sill, nugget, rng, order, obj = engine.variogram_fit(g.abscissa, g.ordinate, g.counts, names, nu,
                                                               WEIGHTINGS[weighting], max_nugget_frac)
    regularize = True
    if kind == "gaussian":
        if nugget >= GAUSSIAN_NUGGET_EPS:
            nugget -= GAUSSIAN_NUGGET_EPS
        else:
            regularize = False
    model = VariogramModel(kind, float(sill), float(nugget), float(rng), float(order), None, regularize)
    return (model, dict(zip(names, obj))) if return_objectives else model
