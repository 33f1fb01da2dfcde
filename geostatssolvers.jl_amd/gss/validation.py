"""Cross-validation of a kriging model on the samples it was fitted to ([DEP] GeoStatsBase `cverror` with LeaveOneOut /
KFoldValidation / BlockValidation / LeaveBallOut -- a dependency of the reference, not in its tree; the conventions here
are this library's own and are stated in include/gss.h).

    res = cross_validate(problem, KrigingSolver(z=dict(variogram=g, maxneighbors=16)), KFoldValidation(10))
    res["z"].summary.cverror          # == cverror(solver, problem, KFoldValidation(10))["z"]

Host logic only: the folds are built here, every prediction and the error summary come from the engine (the global
neighbourhood reads leave-one-out, gss_krig_cv_global, and folds, gss_krig_cv_global_folds, off the factor of the fitted
system; a moving neighbourhood searches each sample's neighbours outside its own fold, gss_krig_cv_knn; gss_cv_summary
reduces the errors).

A CoKrigingSolver is cross-validated by LOCATION: the stacked samples of a joint group that share their coordinates form
one location, the method partitions the locations, and a sample is predicted from the samples of the other folds -- so a
collocated secondary value never helps to predict the primary one it sits on.  (Leaving one datum out with its collocated
partners in play is the handle-level `CoKrigHandle.cv_knn(k, fold=None)`.)  The result is per variable; errors of variables
on different scales are never pooled.

    res = cross_validate(problem, CoKrigingSolver((("cu", "zn"), dict(model=lmc, maxneighbors=(8, 16)))), KFoldValidation(10))
    res["cu"].summary.cverror

IDWSolver and LWRSolver are cross-validated on the same samples and folds, so that the estimators can be compared
(gss_idw_cv / gss_lwr_cv); the solver names the variables it estimates (`IDWSolver(z={})` for the defaults).
`maxneighbors=None` takes every eligible sample, with every method, LeaveBallOut included.
Neither estimator has a prediction variance: `variance` is None, the summary's `mse_std_n` is 0 and its standardised
means are NaN; `aux` holds what the solver returns beside the estimate (`<var>_distance`, `<var>_variance`).

    cverror(IDWSolver(z=dict(exponent=2, maxneighbors=16)), problem, KFoldValidation(10))["z"]"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from .engine import EDK
from .geo import GeoTable, PointSet
from .problems import EstimationProblem
from .solvers import (CoKrigingSolver, ExpWeight, IDWSolver, KrigingSolver, LWRSolver, _ball, _distance, _rot_kw,
                      kriging_ui, searcher_ui)


class LeaveOneOut:
    """Every sample is its own fold."""
    exclude_radius = None

    def folds(self, coords):
        return None, 0


class LeaveBallOut(LeaveOneOut):
    """Leave-one-out that also leaves out every sample within `radius` (search distance) of the one predicted; a sample
    exactly on the radius is left out."""

    def __init__(self, radius):
        if not float(radius) >= 0.0:
            raise ValueError("LeaveBallOut needs a radius >= 0")
        self.exclude_radius = float(radius)


class KFoldValidation:
    """k folds whose sizes differ by at most one; `shuffle` assigns the samples at random (`rng`: seed or Generator),
    otherwise sample i belongs to fold i mod k."""
    exclude_radius = None

    def __init__(self, k, shuffle=True, rng=None):
        if int(k) < 2:
            raise ValueError("KFoldValidation needs at least 2 folds")
        self.k, self.shuffle, self.rng = int(k), bool(shuffle), rng

    def folds(self, coords):
        n = coords.shape[0]
        if self.k > n:
            raise ValueError(f"{self.k} folds for {n} samples")
        ids = (np.arange(n) % self.k).astype(np.int32)
        if self.shuffle:
            rng = self.rng if isinstance(self.rng, np.random.Generator) else np.random.default_rng(self.rng)
            ids = ids[rng.permutation(n)]
        return np.ascontiguousarray(ids), self.k


class BlockValidation:
    """fold = the axis-aligned block of side lengths `sides` a sample falls in, counted from the corner of the samples'
    bounding box: cell index floor((x - xmin) / side) per axis (a sample on a block edge belongs to the upper block), the
    occupied blocks numbered 0, 1, ... in ascending order of their cell index."""
    exclude_radius = None

    def __init__(self, sides):
        self.sides = np.atleast_1d(np.asarray(sides, dtype=np.float64))
        if not np.all(self.sides > 0.0):
            raise ValueError("BlockValidation needs positive side lengths")

    def folds(self, coords):
        d = coords.shape[1]
        sides = np.broadcast_to(self.sides, (d,)) if self.sides.size == 1 else self.sides
        if sides.size != d:
            raise ValueError(f"{sides.size} block sides for {d}-D samples")
        cell = np.floor((coords - coords.min(axis=0)) / sides).astype(np.int64)
        _, ids = np.unique(cell, axis=0, return_inverse=True)
        ids = np.ascontiguousarray(ids.reshape(-1), dtype=np.int32)
        return ids, int(ids.max()) + 1


class CrossValidationResult:
    """Per variable: `pred`, `variance`, `residual` (z - pred), `status` (0 ok, 1 missing, 2 singular) and `fold` (ids;
    None for leave-one-out) of the non-missing samples `indices`, and `summary` (the fields of gss_cv_summary_t plus
    `fold_mse`).  IDWSolver / LWRSolver: `variance` is None and `aux` = {"<var>_distance" or "<var>_variance":
    column}."""

    def __init__(self, indices, z, pred, variance, status, fold, summary, aux=None):
        self.indices, self.z, self.pred, self.variance, self.status, self.fold = indices, z, pred, variance, status, fold
        self.residual = z - pred
        self.summary = summary
        self.aux = aux

    def __repr__(self):
        s = self.summary
        return f"CrossValidationResult(n_ok={int(s.n_ok)}, me={s.me:.4g}, mse={s.mse:.4g}, cverror={s.cverror:.4g})"


def _host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


def location_ids(x):
    """One id per distinct location of the stacked samples `x` (exact coordinate equality), numbered in the order of
    first appearance -> (ids[n], the coordinates of the locations)."""
    x = np.asarray(x, dtype=np.float64)
    _, first, inv = np.unique(x, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return np.ascontiguousarray(rank[np.asarray(inv).reshape(-1)], dtype=np.int32), x[np.sort(first)]


def _cross_validate_cokriging(data, variables, solver, method, eng):
    """Per joint group: stack as `preprocess` does, give each location one fold id from the method's partition of the
    locations, predict every stacked sample (global neighbourhood: cv_global_folds off the fitted factor; moving
    neighbourhood: gss_cokrig_cv_knn), and summarise per variable."""
    pre = solver.preprocess(SimpleNamespace(data=data, variables=tuple(variables)))
    out = {}
    for grp, q in pre.items():
        x, z, var = q["x"], np.ascontiguousarray(q["z"], dtype=np.float64), q["var"]
        if x.shape[0] < 2:
            raise AssertionError(f"cross-validation of {grp} needs at least two non-missing samples")
        loc, ucoords = location_ids(x)
        exact = q["nmax"] is None
        if exact and method.exclude_radius is not None:
            raise ValueError(f"{type(method).__name__} under the global neighbourhood (maxneighbors=None) is not "
                             "available: the factor of the system gives leave-one-out only; set maxneighbors")
        if not exact and sum(q["nmax"]) > 64:
            raise ValueError(f"maxneighbors: {sum(q['nmax'])} neighbours in total for {grp}, the moving "
                             f"neighbourhood of cokriging holds at most 64")
        lfold, _ = method.folds(ucoords)
        # LeaveOneOut / LeaveBallOut give no ids: one fold per location
        fold = loc if lfold is None else np.ascontiguousarray(np.asarray(lfold)[loc], dtype=np.int32)
        h = eng.cokrig(q["structure"], q["B0"], q["B1"], q["variant"], x, z, var, means=q["means"], factor=exact)
        try:
            if exact:
                pred, var_, st = h.cv_global_folds(fold)
            else:
                radius, radii = _ball(q["neighborhood"])
                pred, var_, st = h.cv_knn(q["nmax"], fold=fold, exclude_radius=method.exclude_radius,
                                          minneighbors=q["minneighbors"], radius=radius, radii=radii,
                                          **_rot_kw(q["neighborhood"]))[:3]
        finally:
            h.close()
        pred, var_, st = _host(pred), _host(var_), _host(st)
        for a, v in enumerate(grp):
            own = var == a
            inds = np.flatnonzero(~np.isnan(np.asarray(data[v], dtype=np.float64)))
            # this variable's samples only, its folds compacted to 0 .. nfolds - 1
            _, fa = np.unique(fold[own], return_inverse=True)
            fa = np.ascontiguousarray(np.asarray(fa).reshape(-1), dtype=np.int32)
            nfa = int(fa.max()) + 1
            za, pa, va, sa = (np.ascontiguousarray(t[own]) for t in (z, pred, var_, st))
            fields, fmse = eng.cv_summary(za, pa, va, sa, fa, nfa)
            summary = SimpleNamespace(**fields, fold_mse=_host(fmse))
            out[v] = CrossValidationResult(inds, za, pa, va, sa, fa, summary)
    return {v: out[v] for v in variables if v in out}


def _cross_validate_estimator(data, variables, solver, method, eng):
    """IDWSolver / LWRSolver: per variable the non-missing samples, the solver's own `maxneighbors`, `minneighbors`,
    `neighborhood` and `distance` (as `_NeighborEstimator.solve` reads them), one engine call (gss_idw_cv / gss_lwr_cv)
    per group of scalar variables with the same parameters and the same valid samples, one summary per variable."""
    idw = isinstance(solver, IDWSolver)
    call = "idw_cv" if idw else "lwr_cv"
    if not hasattr(eng, call):
        raise TypeError(f"cross-validation of {type(solver).__name__} needs an engine with `{call}`; "
                        f"{getattr(eng, '__name__', type(eng).__name__)} has none")
    coords = data.domain.centroids()
    for v in variables:
        if getattr(data[v], "dtype", None) == object:
            raise TypeError(f"cross-validation of compositional (object) columns is not available: variable {v!r}")

    def _key(v):
        valid = np.flatnonzero(~np.isnan(np.asarray(data[v], dtype=np.float64)))
        ident = lambda o: o if isinstance(o, (int, float, str, type(None))) else id(o)   # noqa: E731
        return tuple(sorted((k, ident(x)) for k, x in solver.params(v).items())) + (valid.tobytes(),)
    keys = {v: _key(v) for v in variables}
    out, batched = {}, {}
    for var in variables:
        if var not in batched:
            p = solver.params(var)
            group = [v for v in variables if keys[v] == keys[var]]
            inds = np.flatnonzero(~np.isnan(np.asarray(data[var], dtype=np.float64)))      # idw.jl:77, lwr.jl:80
            n = inds.size
            if n < 2:
                raise AssertionError(f"cross-validation of {var} needs at least two non-missing samples")
            dist = _distance(p)
            solver._check(p)
            extra = {}
            if idw:
                extra["exponent"] = float(p["exponent"])
            else:
                wf = p["weightfun"] or ExpWeight()
                if not hasattr(wf, "spec"):
                    raise NotImplementedError("cross-validation with a callable weightfun is not available: weightfun "
                                              "must be ExpWeight(a, p) or TricubeWeight()")
                extra["weight"] = wf.spec()
            x = np.ascontiguousarray(coords[inds])
            _, nmax = searcher_ui(PointSet(x), p["maxneighbors"], p["distance"], p["neighborhood"])
            # every sample (maxneighbors=None or >= n): every ELIGIBLE sample; else a sample is never its own neighbour
            k = n if p["maxneighbors"] is None or nmax >= n else min(nmax, n - 1)
            assert p["minneighbors"] <= k, "invalid min/max number of neighbors"             # idw.jl:97
            fold, nfolds = method.folds(x)
            radius, radii = _ball(p["neighborhood"])
            zs = np.stack([np.asarray(data[v], dtype=np.float64)[inds] for v in group])
            pred, aux, st = getattr(eng, call)(x, zs if len(group) > 1 else zs[0], k, fold=fold,
                                               exclude_radius=method.exclude_radius, minneighbors=p["minneighbors"],
                                               radius=radius, radii=radii, distance=dist,
                                               **extra, **_rot_kw(p["neighborhood"]))[:3]
            pred, aux, st = _host(pred).reshape(len(group), n), _host(aux), _host(st)
            for j, v in enumerate(group):
                batched[v] = (inds, zs[j], np.ascontiguousarray(pred[j]), aux, st, fold, nfolds)
        inds, zv, pv, aux, st, fold, nfolds = batched.pop(var)
        fields, fmse = eng.cv_summary(zv, pv, np.zeros_like(zv), st, fold, nfolds)   # no prediction variance
        summary = SimpleNamespace(**fields, fold_mse=None if fmse is None else _host(fmse))
        out[var] = CrossValidationResult(inds, zv, pv, None, st, fold, summary, aux={f"{var}_{solver.AUX}": aux})
    return out


def cross_validate(problem_or_geotable, solver, method=None, engine=None):
    """{variable: CrossValidationResult}.  Of an EstimationProblem only the data are used.  The dispatch follows the
    KrigingSolver's own parameters: the kriging variant by `kriging_ui`; `maxneighbors`, `minneighbors`, `neighborhood`
    and `distance` by `searcher_ui`.  `maxneighbors=None` is the global neighbourhood: leave-one-out and the methods that
    partition the samples into folds (KFoldValidation, BlockValidation) are read off the factor of the one fitted system;
    LeaveBallOut, whose sets overlap, needs a moving neighbourhood.  A CoKrigingSolver follows its joint parameters the same
    way, with the folds made of locations (module docstring).  IDWSolver / LWRSolver: the solver has to name at least
    one variable (`IDWSolver(z={})` takes the defaults; a solver without any is a `TypeError`, as every estimator was
    before these two could be scored); every method works with and without `maxneighbors`; `variance` is None and
    the summary is formed with a zero variance column, so `mse_std_n` is 0 and `mean_std` / `msq_std` are NaN --
    neither estimator has a prediction variance."""
    method = LeaveOneOut() if method is None else method
    if not isinstance(solver, (KrigingSolver, CoKrigingSolver, IDWSolver, LWRSolver)):
        raise TypeError("cross-validation is available for KrigingSolver and CoKrigingSolver, IDWSolver and LWRSolver, "
                        f"not {type(solver).__name__}")
    if isinstance(solver, (IDWSolver, LWRSolver)) and not solver.vparams:
        name = type(solver).__name__
        raise TypeError("cross-validation is available for KrigingSolver and CoKrigingSolver, and for an IDWSolver or "
                        f"LWRSolver that names the variables it estimates: {name}() names none (write "
                        f"{name}(z=dict(...)); z={{}} takes the defaults)")
    if isinstance(problem_or_geotable, EstimationProblem):
        data, variables = problem_or_geotable.data, problem_or_geotable.variables
    elif isinstance(problem_or_geotable, GeoTable):
        data = problem_or_geotable
        if isinstance(solver, CoKrigingSolver):
            variables = tuple(v for grp in solver._spec for v in grp if v in data.table)
        else:
            variables = tuple(v for v in solver.vparams if v in data.table) or tuple(data.table)
    else:
        raise TypeError("cross_validate needs an EstimationProblem or a GeoTable")
    eng = engine or solver.engine
    if isinstance(solver, CoKrigingSolver):
        return _cross_validate_cokriging(data, variables, solver, method, eng)
    if isinstance(solver, (IDWSolver, LWRSolver)):
        return _cross_validate_estimator(data, variables, solver, method, eng)
    coords = data.domain.centroids()
    out = {}
    for var in variables:
        p = solver.params(var)
        z = np.asarray(data[var], dtype=np.float64)
        inds = np.flatnonzero(~np.isnan(z))
        if inds.size < 2:
            raise AssertionError(f"cross-validation of {var} needs at least two non-missing samples")
        if p.get("support", "point") != "point":
            raise ValueError("cross-validation predicts the samples, at point support: support='point' only")
        x, zv = np.ascontiguousarray(coords[inds]), np.ascontiguousarray(z[inds])
        n = x.shape[0]
        vdom = PointSet(x)
        variant = kriging_ui(vdom, p["variogram"], p["mean"], p["degree"], p["drifts"])
        drift = None
        if variant == EDK:
            drift = np.stack([[f(c) for f in p["drifts"]] for c in x]).astype(np.float64)
        exact = p["maxneighbors"] is None
        fold, nfolds = None, 0
        if exact:
            # folds need the block form of the identity (handle.cv_global_folds); a ball is no partition
            if type(method) is not LeaveOneOut and (method.exclude_radius is not None
                                                    or not hasattr(eng.Krig, "cv_global_folds")):
                raise ValueError(f"{type(method).__name__} under the global neighbourhood (maxneighbors=None) is not "
                                 "available: the factor of the system gives leave-one-out only; set maxneighbors")
        if not exact or type(method) is not LeaveOneOut:
            fold, nfolds = method.folds(x)
        h = eng.Krig(p["variogram"], variant, x, zv, mean=p["mean"], degree=p["degree"], drift_data=drift, factor=exact)
        try:
            if exact:
                pred, var_, st = h.cv_global() if fold is None else h.cv_global_folds(fold)
            else:
                _, nmax = searcher_ui(vdom, p["maxneighbors"], p["distance"], p["neighborhood"])
                radius, radii = _ball(p["neighborhood"])
                pred, var_, st = h.cv_knn(min(nmax, n - 1), fold=fold, exclude_radius=method.exclude_radius,
                                          minneighbors=p["minneighbors"], radius=radius, radii=radii,
                                          distance=_distance(p), **_rot_kw(p["neighborhood"]))[:3]
        finally:
            h.close()
        pred, var_, st = _host(pred), _host(var_), _host(st)
        fields, fmse = eng.cv_summary(zv, pred, var_, st, fold, nfolds)
        summary = SimpleNamespace(**fields, fold_mse=None if fmse is None else _host(fmse))
        out[var] = CrossValidationResult(inds, zv, pred, var_, st, fold, summary)
    return out


def cverror(solver, problem, method=None):
    """{variable: cross-validation error}: the mean over the folds of the folds' mean squared errors."""
    return {v: r.summary.cverror for v, r in cross_validate(problem, solver, method).items()}
