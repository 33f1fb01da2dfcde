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
from .variograms import GAUSSIAN_NUGGET_EPS, MetricBall, VariogramModel

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


# ---- varioplane: every direction sector in one pass (gss_variogram_plane) and the anisotropic fit --------------------
@dataclass
class EmpiricalVarioplaneResult:
    """One variable's empirical variogram by direction sector: row s of the (nangs, nlags) arrays is the sector
    [angles[s], angles[s + 1]) of directions modulo pi (the last one ends at angles[0] + pi).  The sectors partition
    the half-circle: over s the counts add up to those of EmpiricalVariogram.  Empty bins hold NaN."""
    angles: np.ndarray        # lower boundaries of the sectors, radians
    midangles: np.ndarray
    abscissa: np.ndarray
    ordinate: np.ndarray
    counts: np.ndarray
    nduplicates: int
    maxlag: float
    estimator: str = "matheron"
    var: str = ""

    @property
    def nangs(self):
        return int(self.counts.shape[0])

    @property
    def nlags(self):
        return int(self.counts.shape[1])

    def sector(self, s):
        """Sector s as an EmpiricalVariogramResult: what `fit` takes for one direction."""
        return EmpiricalVariogramResult(self.abscissa[s].copy(), self.ordinate[s].copy(), self.counts[s].copy(),
                                        self.nduplicates, self.maxlag, self.estimator, self.var)


def plane_basis(normal):
    """e1, e2, n (rows) for the plane with the given normal: n = normal / |normal|; e1 = the coordinate axis on which n
    has its smallest absolute component (the first such axis), made orthogonal to n and normalised; e2 = n x e1, so
    that (e1, e2, n) is right-handed.  For normal = z this is e1 = x, e2 = y: angles are those of the x-y plane."""
    nrm = np.asarray(normal, dtype=np.float64).reshape(-1)
    if nrm.size != 3 or not np.all(np.isfinite(nrm)) or not np.any(nrm != 0.0):
        raise ValueError("normal must be a non-zero finite 3-vector")
    nrm = nrm / np.sqrt((nrm * nrm).sum())
    a = np.zeros(3)
    a[int(np.argmin(np.abs(nrm)))] = 1.0
    e1 = a - (a @ nrm) * nrm
    e1 = e1 / np.sqrt((e1 * e1).sum())
    e2 = np.cross(nrm, e1)
    e2 = e2 / np.sqrt((e2 * e2).sum())
    return np.ascontiguousarray(np.stack([e1, e2, nrm]))


PLANE_MAX_COLUMNS = 4          # gss.h: value columns per gss_variogram_plane call
PLANE_MAX_WORDS = 8192         # gss.h: nangles * nlags * (2 + nz)


def EmpiricalVarioplane(data, var_or_vars, nangs=18, nlags=20, maxlag=None, offset=0.0, normal=None,
                        ptol=float("inf"), estimator="matheron", engine=None):
    """Empirical variogram of every one of `nangs` equal direction sectors of the half-circle, in one pass over the
    pairs: sector s holds the directions [offset + s pi / nangs, offset + (s + 1) pi / nangs) modulo pi (angles in
    radians, counter-clockwise from the first axis of the plane).  2-D tables: the plane of the samples (`normal` is
    refused).  3-D tables: `normal` is required; the plane is spanned by `plane_basis(normal)` and only pairs whose
    separation lies within `ptol` of the plane take part (inf: all, projected onto it).  One variable ->
    EmpiricalVarioplaneResult, several -> dict.  Missing values are dropped per variable as in EmpiricalVariogram."""
    if estimator not in ESTIMATORS:
        raise ValueError(f"estimator {estimator!r}: 'matheron' or 'cressie'")
    engine = engine or default_engine()
    single = isinstance(var_or_vars, str)
    names = [var_or_vars] if single else list(var_or_vars)
    if not names:
        raise ValueError("no variable given")
    nangs, nlags = int(nangs), int(nlags)
    if nangs < 2:
        raise ValueError("a varioplane has at least 2 sectors")
    x = np.ascontiguousarray(data.domain.centroids(), dtype=np.float64)
    d = x.shape[1]
    if d == 2:
        if normal is not None:
            raise ValueError("normal describes a plane in 3-D; 2-D samples lie in their own plane")
        basis = None
    elif d == 3:
        if normal is None:
            raise ValueError("3-D samples need the normal of the plane the directions are taken in")
        basis = plane_basis(normal)
    else:
        raise ValueError(f"a varioplane needs 2-D or 3-D samples, these are {d}-D")
    cols = [np.asarray(data[v], dtype=np.float64) for v in names]
    if maxlag is None:
        maxlag = _default_maxlag(x)
    angles = float(offset) + np.arange(nangs) * (math.pi / nangs)
    dirs = np.ascontiguousarray(np.stack([np.cos(angles), np.sin(angles)], axis=1))
    percall = max(1, min(PLANE_MAX_COLUMNS, PLANE_MAX_WORDS // max(nangs * nlags, 1) - 2))
    groups = {}                                    # finite mask -> variables that share it
    for i, c in enumerate(cols):
        groups.setdefault(np.isfinite(c).tobytes(), []).append(i)
    out = [None] * len(names)
    for members in groups.values():
        keep = np.isfinite(cols[members[0]])
        xs = x if keep.all() else np.ascontiguousarray(x[keep])
        for lo in range(0, len(members), percall):
            part = members[lo:lo + percall]
            z = np.ascontiguousarray(np.stack([cols[i][keep] for i in part]))
            count, lagsum, zsum, ndup = engine.variogram_plane(xs, z, nlags, maxlag, dirs, basis, ptol,
                                                               ESTIMATORS[estimator])
            with np.errstate(invalid="ignore", divide="ignore"):
                absc = np.where(count > 0, lagsum / count, np.nan)
            for r, i in enumerate(part):
                out[i] = EmpiricalVarioplaneResult(angles.copy(), angles + 0.5 * math.pi / nangs, absc,
                                                   _ordinate(estimator, zsum[r], count), count.copy(), int(ndup),
                                                   float(maxlag), estimator, names[i])
    return out[0] if single else dict(zip(names, out))


def fit_anisotropic(kind_or_kinds, plane, weighting="count", nu=1.0, max_nugget_frac=1.0, return_objectives=False,
                    engine=None):
    """Weighted least-squares fit of 2-D geometric anisotropy to an EmpiricalVarioplaneResult
    (gss_variogram_fit_aniso; every bin enters with the mid-angle of its sector).  Returns a VariogramModel with
    `radii = (r1, r2)`, r1 >= r2, and `rotation` = the counter-clockwise rotation by the fitted azimuth theta of r1
    (what `Kind(MetricBall((r1, r2), theta))` builds), or the isotropic model when the fitted ratio is 1.  The
    Gaussian `nugget - 1e-6` rule is that of `fit`."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting {weighting!r}: one of {tuple(WEIGHTINGS)}")
    engine = engine or default_engine()
    kinds = [kind_or_kinds] if isinstance(kind_or_kinds, str) or callable(kind_or_kinds) else list(kind_or_kinds)
    names = [_kind_name(k) for k in kinds]
    phi = np.broadcast_to(np.asarray(plane.midangles, dtype=np.float64)[:, None], plane.counts.shape)
    kind, sill, nugget, radii, theta, rng, order, obj = engine.variogram_fit_aniso(
        plane.abscissa, phi, plane.ordinate, plane.counts, names, nu, WEIGHTINGS[weighting], max_nugget_frac)
    regularize = True
    if kind == "gaussian":
        if nugget >= GAUSSIAN_NUGGET_EPS:
            nugget -= GAUSSIAN_NUGGET_EPS
        else:
            regularize = False
    if radii is None:
        model = VariogramModel(kind, float(sill), float(nugget), float(rng), float(order), None, regularize)
    else:
        ball = MetricBall(radii, float(theta))
        model = VariogramModel(kind, float(sill), float(nugget), 1.0, float(order), ball.radii, regularize, ball.rotation)
    return (model, dict(zip(names, obj))) if return_objectives else model


# ---- cross-variograms in one pass (gss_variogram_cross) and the linear model of coregionalisation -------------------
def _pair_row(nz, a, b):
    a, b = (a, b) if a <= b else (b, a)
    return a * nz - a * (a - 1) // 2 + (b - a)


@dataclass
class EmpiricalCrossVariogramResult:
    """Direct and cross variograms of several variables measured on the same samples, from one pass over the pairs.
    `ordinate` has one row per pair of variables (a, b), a <= b, in the row order of gss_variogram_cross; bins
    without pairs hold NaN.  Variables are addressed by name or by position."""
    names: tuple
    abscissa: np.ndarray
    ordinate: np.ndarray      # (nz (nz + 1) / 2, nlags): gamma_ab = csum / (2 count)
    count: np.ndarray
    nduplicates: int
    maxlag: float

    def _index(self, v):
        return self.names.index(v) if isinstance(v, str) else int(v)

    @property
    def nlags(self):
        return int(self.count.size)

    def gamma(self, a, b):
        """The cross-variogram of variables a and b (symmetric in them); gamma(a, a) is the direct one."""
        return self.ordinate[_pair_row(len(self.names), self._index(a), self._index(b))]

    def direct(self, a):
        """Variable a's direct variogram as an EmpiricalVariogramResult: what `fit` takes."""
        i = self._index(a)
        return EmpiricalVariogramResult(self.abscissa.copy(), self.gamma(i, i).copy(), self.count.copy(),
                                        self.nduplicates, self.maxlag, "matheron", self.names[i])


def EmpiricalCrossVariogram(data, names, nlags=20, maxlag=None, direction=None, dtol=float("inf"), atol=math.pi / 8,
                            engine=None):
    """Direct and cross variograms (Matheron) of up to 8 variables of one table in ONE pass over the pairs.  A sample
    takes part only if every one of the variables exists there (a cross-variogram needs both values at both ends).
    `direction`, `dtol`, `atol` as in DirectionalVariogram; None: omnidirectional."""
    engine = engine or default_engine()
    names = tuple(names)
    if not 1 <= len(names) <= 8:
        raise ValueError("between 1 and 8 variables (gss.h: value columns per gss_variogram_cross call)")
    x = np.ascontiguousarray(data.domain.centroids(), dtype=np.float64)
    cols = np.stack([np.asarray(data[v], dtype=np.float64) for v in names])
    keep = np.isfinite(cols).all(axis=0)
    if not keep.all():
        x, cols = np.ascontiguousarray(x[keep]), cols[:, keep]
    if maxlag is None:
        maxlag = _default_maxlag(x)
    u, cos_atol = None, 0.0
    if direction is not None:
        u = np.asarray(direction, dtype=np.float64).reshape(-1)
        nrm = float(np.sqrt((u * u).sum()))
        if not (nrm > 0.0 and np.isfinite(nrm)):
            raise ValueError("direction must be a non-zero finite vector")
        if atol is not None and not 0.0 <= atol <= math.pi / 2:
            raise ValueError("atol is an angle in [0, pi / 2] radians")
        u = u / nrm
        cos_atol = 0.0 if atol is None or atol >= math.pi / 2 else math.cos(atol)
    count, lagsum, csum, ndup = engine.variogram_cross(x, np.ascontiguousarray(cols), nlags, maxlag, u, dtol, cos_atol)
    with np.errstate(invalid="ignore", divide="ignore"):
        absc = np.where(count > 0, lagsum / count, np.nan)
        gam = np.where(count > 0, csum / (2.0 * count.astype(np.float64)), np.nan)
    return EmpiricalCrossVariogramResult(names, absc, gam, count, int(ndup), float(maxlag))


@dataclass
class LMCModel:
    """Linear model of coregionalisation Gamma(h) = B0 + B1 f(h / range): nugget matrix B0 and partial sills B1, both
    positive semidefinite, one structure and one range for all variables."""
    names: tuple
    kind: str
    range: float
    order: float
    B0: np.ndarray
    B1: np.ndarray
    objective: float

    def _index(self, v):
        return self.names.index(v) if isinstance(v, str) else int(v)

    def variogram(self, a):
        """Variable a's direct model, as every solver takes it: sill = B0_aa + B1_aa, nugget = B0_aa and the shared
        range.  A Gaussian model follows the `nugget - 1e-6` rule of `fit`."""
        i = self._index(a)
        sill, nugget, regularize = float(self.B0[i, i] + self.B1[i, i]), float(self.B0[i, i]), True
        if self.kind == "gaussian":
            if nugget >= GAUSSIAN_NUGGET_EPS:
                nugget -= GAUSSIAN_NUGGET_EPS
            else:
                regularize = False
        return VariogramModel(self.kind, sill, nugget, float(self.range), float(self.order), None, regularize)

    def correlation(self, a, b):
        """(B0_ab + B1_ab) / sqrt(sill_a sill_b): the correlation of the two variables at one location under this
        model.  This is the number the LUGS solver takes as its joint parameter `correlation` when it co-simulates a
        and b."""
        i, j = self._index(a), self._index(b)
        s = self.B0 + self.B1
        return float(s[i, j] / math.sqrt(s[i, i] * s[j, j]))


def fit_lmc(kind_or_kinds, cross, weighting="count", nu=1.0, return_objectives=False, engine=None):
    """Fit of the linear model of coregionalisation to an EmpiricalCrossVariogramResult (gss_variogram_fit_lmc, host
    code of the library): the best of the given kinds -> LMCModel."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting {weighting!r}: one of {tuple(WEIGHTINGS)}")
    engine = engine or default_engine()
    kinds = [kind_or_kinds] if isinstance(kind_or_kinds, str) or callable(kind_or_kinds) else list(kind_or_kinds)
    knames = [_kind_name(k) for k in kinds]
    kind, rng, b0, b1, obj = engine.variogram_fit_lmc(cross.abscissa, cross.ordinate, cross.count, knames, nu,
                                                      WEIGHTINGS[weighting])
    model = LMCModel(tuple(cross.names), kind, float(rng), float(nu) if kind == "matern" else 1.0, b0, b1,
                     float(obj[knames.index(kind)]))
    return (model, dict(zip(knames, obj))) if return_objectives else model
