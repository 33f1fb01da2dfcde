"""Declustering weights: the first link of the chain from raw samples to back-transformed realisations.

Preferentially sampled data (drilling clustered in the rich zone) must be declustered before their histogram means
anything.  `weight(data, method, var)` computes the weights on the device (gss.h, gss_decluster_*) with one of

    BlockWeighting(*sides)               one grid at the data's bounding-box minimum (GeoStatsBase)
    CellDeclustering(cmin, cmax, ...)    GSLIB declus: a sweep over cell sizes and origin offsets
    PolygonalWeighting(grid_or_dims)     Voronoi areas by discretisation: lattice points per nearest sample

and `wmean`, `wvar`, `wquantile` are the declustered statistics a user checks next.  The weights go into
`NormalScore.fit(values, weights=w)`, which drops the rows `weight` marks NaN in step with their values.
"""
from __future__ import annotations

import numpy as np

from .engine import default_engine
from .geo import CartesianGrid, GeoTable


class Weights(np.ndarray):
    """A float64 vector of weights, one per row (NaN for a row left out), with the method's diagnostics as attributes:
    `sizes`, `means` and `best` of a CellDeclustering sweep (what the size-against-mean plot shows), `nzero` of a
    PolygonalWeighting.  Attributes a method does not produce are None."""

    _EXTRA = ("sizes", "means", "best", "nzero")

    def __new__(cls, values, **extra):
        obj = np.asarray(values, dtype=np.float64).view(cls)
        for k in cls._EXTRA:
            setattr(obj, k, extra.get(k))
        return obj

    def __array_finalize__(self, obj):
        for k in self._EXTRA:
            setattr(self, k, getattr(obj, k, None))


def _sides(sides, d, what):
    s = np.asarray(sides, dtype=np.float64).reshape(-1)
    if s.size == 1:
        s = np.repeat(s, d)
    if s.size != d:
        raise ValueError(f"{what}: {s.size} sides for {d}-D data")
    if not (np.all(np.isfinite(s)) and np.all(s > 0.0)):
        raise ValueError(f"{what}: sides must be finite and > 0")
    return s


def _engine_method(engine, name):
    fn = getattr(engine, name, None)
    if fn is None:
        raise NotImplementedError(f"engine {getattr(engine, 'name', engine)!r} has no {name}: declustering runs on the "
                                  f"device engine")
    return fn


class BlockWeighting:
    """`BlockWeighting(sides...)`: w_i = n / (occupied cells x samples in the cell of i) on one grid whose origin is
    the bounding-box minimum of the data.  One number is used for every axis."""

    def __init__(self, *sides):
        if len(sides) == 1 and np.ndim(sides[0]) >= 1:
            sides = tuple(sides[0])
        if not sides:
            raise ValueError("BlockWeighting needs the sides of a block")
        self.sides = tuple(float(s) for s in sides)

    def weights(self, x, z, engine):
        s = _sides(self.sides, x.shape[1], "BlockWeighting")
        w, _, _ = _engine_method(engine, "decluster_cells")(x, None, s[None, :], 1)
        return Weights(w)


class CellDeclustering:
    """`CellDeclustering(cmin, cmax, ncell=24, noffsets=8, criterion="min", anisotropy=None)`: GSLIB's declus.  `ncell`
    cell sizes linear from cmin to cmax inclusive, each laid `noffsets` times with the origin shifted along the
    diagonal; the weights of a size are the mean over its offsets and the size whose declustered mean of `var` is
    smallest ("min": high values were oversampled) or largest ("max") wins.  `anisotropy` scales the size per axis
    (default 1 everywhere).  The result carries `.sizes`, `.means` and `.best`."""

    def __init__(self, cmin, cmax, ncell=24, noffsets=8, criterion="min", anisotropy=None):
        cmin, cmax, ncell, noffsets = float(cmin), float(cmax), int(ncell), int(noffsets)
        if not (np.isfinite(cmin) and np.isfinite(cmax) and 0.0 < cmin <= cmax):
            raise ValueError(f"cell sizes need 0 < cmin <= cmax, not ({cmin}, {cmax})")
        if not 1 <= ncell <= 256:
            raise ValueError(f"ncell = {ncell} outside 1 .. 256")
        if not 1 <= noffsets <= 64:
            raise ValueError(f"noffsets = {noffsets} outside 1 .. 64")
        if criterion not in ("min", "max"):
            raise ValueError(f"criterion {criterion!r}: 'min' or 'max'")
        self.sizes = np.linspace(cmin, cmax, ncell) if ncell > 1 else np.array([cmin])
        self.noffsets, self.criterion = noffsets, criterion
        self.anisotropy = None if anisotropy is None else tuple(float(a) for a in anisotropy)

    def weights(self, x, z, engine):
        d = x.shape[1]
        an = np.ones(d) if self.anisotropy is None else _sides(self.anisotropy, d, "CellDeclustering anisotropy")
        if z is None and self.sizes.size > 1:
            raise ValueError("CellDeclustering chooses the size by the declustered mean: name the variable, "
                             "weight(data, method, var)")
        sides = self.sizes[:, None] * an[None, :]
        w, means, best = _engine_method(engine, "decluster_cells")(x, z, sides, self.noffsets, self.criterion)
        return Weights(w, sizes=self.sizes.copy(), means=means, best=best)


class PolygonalWeighting:
    """`PolygonalWeighting(grid_or_dims, allow_zero=False)`: the area of influence of every sample, measured by the
    points of a lattice that are nearer to it than to any other sample (ties to the lower row).  A `CartesianGrid`
    gives the lattice itself (its centroids); a tuple of `dims` lays that many points over the data's bounding box.
    A sample no point chose would get weight zero, which `NormalScore.fit` refuses: that raises ValueError unless
    `allow_zero=True`."""

    def __init__(self, grid_or_dims, allow_zero=False):
        if isinstance(grid_or_dims, CartesianGrid):
            self.grid, self.dims = grid_or_dims, tuple(grid_or_dims.dims)
        else:
            self.grid, self.dims = None, tuple(int(v) for v in np.atleast_1d(grid_or_dims))
        if not self.dims or any(v < 1 for v in self.dims):
            raise ValueError(f"lattice dims {self.dims} must be >= 1")
        self.allow_zero = bool(allow_zero)

    def lattice(self, x):
        d = x.shape[1]
        if len(self.dims) != d:
            raise ValueError(f"a {len(self.dims)}-D lattice for {d}-D data")
        if self.grid is not None:
            return np.asarray(self.grid.origin, dtype=np.float64), np.asarray(self.grid.spacing, dtype=np.float64)
        lo, hi = x.min(axis=0), x.max(axis=0)
        dims = np.asarray(self.dims, dtype=np.float64)
        step = (hi - lo) / dims
        flat = step <= 0.0                       # all samples share this coordinate: unit steps centred on it
        step = np.where(flat, 1.0, step)
        lo = np.where(flat, lo - 0.5 * dims, lo)
        return lo, step

    def weights(self, x, z, engine):
        lo, step = self.lattice(x)
        w, nzero = _engine_method(engine, "decluster_nearest")(x, lo, step, self.dims)
        if nzero and not self.allow_zero:
            raise ValueError(f"nzero = {nzero} of {x.shape[0]} samples are nearest to no lattice point and would get "
                             f"weight zero: use a finer lattice than {self.dims}, or allow_zero=True")
        return Weights(w, nzero=nzero)


def weight(data: GeoTable, method, var=None, engine=None) -> Weights:
    """`weight(data, method, var=None)`: declustering weights of the rows of a geotable, one float64 per row, summing
    to the number of rows used.  With `var`, rows whose value is NaN are left out of the computation and get NaN --
    `NormalScore.fit(data[var], weights=w)` drops the same rows.  CellDeclustering needs `var` (it chooses the size by
    the declustered mean)."""
    if not hasattr(method, "weights"):
        raise TypeError(f"{type(method).__name__} is not a weighting method: BlockWeighting, CellDeclustering or "
                        f"PolygonalWeighting")
    x = np.ascontiguousarray(data.domain.centroids(), dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n = x.shape[0]
    z, keep = None, np.ones(n, dtype=bool)
    if var is not None:
        z = np.asarray(data[var], dtype=np.float64).ravel()
        keep = ~np.isnan(z)
        if not keep.any():
            raise AssertionError("all values are missing, aborting...")
        if not np.all(np.isfinite(z[keep])):
            raise ValueError("values must be finite (NaN marks a missing row)")
    eng = engine or default_engine()
    if keep.all():
        return method.weights(x, z, eng)
    part = method.weights(np.ascontiguousarray(x[keep]), None if z is None else np.ascontiguousarray(z[keep]), eng)
    full = np.full(n, np.nan)
    full[keep] = part
    return Weights(full, **{k: getattr(part, k) for k in Weights._EXTRA})


# ---- weighted statistics (host) -------------------------------------------------------------------------------------
def _vw(values, weights):
    v = np.asarray(values, dtype=np.float64).ravel()
    w = np.asarray(weights, dtype=np.float64).ravel()
    if v.size != w.size:
        raise ValueError(f"{w.size} weights for {v.size} values")
    keep = ~(np.isnan(v) | np.isnan(w))
    v, w = v[keep], w[keep]
    if v.size == 0:
        raise ValueError("no row has both a value and a weight")
    if not (np.all(np.isfinite(v)) and np.all(np.isfinite(w)) and np.all(w >= 0.0) and w.sum() > 0.0):
        raise ValueError("values must be finite and weights finite, >= 0 and not all zero")
    return v, w


def wmean(values, weights) -> float:
    """sum w z / sum w over the rows that have both (NaN rows are dropped)."""
    v, w = _vw(values, weights)
    return float(np.sum(w * v) / np.sum(w))


def wvar(values, weights) -> float:
    """sum w (z - m)^2 / sum w with m = wmean: the variance of the declustered histogram (no n - 1 correction)."""
    v, w = _vw(values, weights)
    m = np.sum(w * v) / np.sum(w)
    return float(np.sum(w * (v - m) ** 2) / np.sum(w))


def wquantile(values, weights, p):
    """Quantiles of the declustered histogram in the cumulative-weight convention of the normal-score fit: equal values
    are merged into classes v_1 < ... < v_K with weights W_k, class k sits at p_k = (weight below v_k + W_k / 2) / total,
    and the quantile is linear in p between the classes, v_1 below p_1 and v_K above p_K.  So wquantile(p_k) = v_k, the
    value `NormalScore.fit(values, weights)` gives the score Phi^-1(p_k)."""
    v, w = _vw(values, weights)
    pos = w > 0.0
    v, w = v[pos], w[pos]
    order = np.argsort(v, kind="stable")
    v, w = v[order], w[order]
    cls, first = np.unique(v, return_index=True)
    W = np.add.reduceat(w, first)
    below = np.concatenate(([0.0], np.cumsum(W)[:-1]))
    pk = (below + 0.5 * W) / W.sum()
    q = np.asarray(p, dtype=np.float64)
    if np.any((q < 0.0) | (q > 1.0)) or np.any(np.isnan(q)):
        raise ValueError("p must lie in [0, 1]")
    out = np.interp(q, pk, cls)
    return float(out) if out.ndim == 0 else out
