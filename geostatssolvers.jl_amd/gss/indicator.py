"""Indicator kriging (GSLIB ik3d + postik): the local distribution of a continuous variable without a Gaussian model.

`IndicatorKrigingSolver` estimates, at every domain element, the ccdf F(c_q) = P(z <= c_q) at K cutoffs and corrects its
order relations; `postik` turns the corrected ccdf into the E-type mean, the conditional variance, probabilities above
thresholds and quantiles.  Conventions: include/gss.h, "indicator kriging"; DESIGN.md section 4.

    solver = IndicatorKrigingSolver(("z", dict(cutoffs=[1, 2, 5], variogram=g, maxneighbors=16, mean="global")))
    sol = solve(EstimationProblem(data, grid, "z"), solver)          # columns z_ccdf_0 .. z_ccdf_2
    post = postik(sol, "z", zmin=0.0, zmax=30.0, thresholds=[2.0])   # z_etype, z_cvar, z_pabove_0
"""
from __future__ import annotations

import numpy as np

from . import parallel
from .engine import OK, SK
from .geo import Ensemble, GeoTable, PointSet, georef
from .problems import EstimationProblem, SimulationProblem
from .solvers import (_ball, _distance, _domain_points, _host, _initbuff, _next_real, _path_order, _rot_kw, _run_state,
                      _SGSPlan, _Solver, searcher_ui)
from .variograms import GaussianVariogram, MetricBall

MAX_CUTOFFS = 16
MAX_NEIGHBORS = 64


def check_cutoffs(cutoffs) -> np.ndarray:
    c = np.asarray(cutoffs, dtype=np.float64).reshape(-1)
    if not 1 <= c.size <= MAX_CUTOFFS:
        raise ValueError(f"{c.size} cutoffs: 1 .. {MAX_CUTOFFS}")
    if not np.all(np.isfinite(c)) or np.any(np.diff(c) <= 0.0):
        raise ValueError("cutoffs must be finite and strictly increasing")
    return np.ascontiguousarray(c)


def global_proportions(z, cutoffs, weights=None) -> np.ndarray:
    """F*_q = sum w (z <= c_q) / sum w over the rows that have a value and a weight (equal weights when None)."""
    z = np.asarray(z, dtype=np.float64).ravel()
    w = np.ones_like(z) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
    if w.size != z.size:
        raise ValueError(f"{w.size} weights for {z.size} values")
    ok = ~(np.isnan(z) | np.isnan(w))
    if not ok.any() or not np.sum(w[ok]) > 0.0 or np.any(w[ok] < 0.0):
        raise ValueError("the weights must be non-negative with a positive sum over the rows that have a value")
    z, w = z[ok], w[ok]
    return np.array([np.sum(w * (z <= c)) / np.sum(w) for c in np.asarray(cutoffs, dtype=np.float64)])


class IndicatorKrigingSolver(_Solver):
    """Per variable: `cutoffs` (1 .. 16, increasing); `variogram` (one model: median indicator kriging) or `variograms`
    (one per cutoff: full indicator kriging); `maxneighbors` (1 .. 64; None: the global neighbourhood, composed from the
    kriging handle), `minneighbors`, `neighborhood`, `distance` as KrigingSolver; `mean=None`: ordinary kriging of the
    indicators, `mean="global"`: simple kriging about the global proportions F*, which are the (`weights`-)weighted
    proportions of the samples below each cutoff (`weights`: one per data row, e.g. from `gss.weight`)."""
    PARAMS = dict(cutoffs=None, variogram=None, variograms=None, maxneighbors=16, minneighbors=1, neighborhood=None,
                  distance="euclidean", mean=None, weights=None)

    def preprocess(self, problem: EstimationProblem):
        if not isinstance(problem, EstimationProblem):
            raise TypeError("IndicatorKrigingSolver solves EstimationProblems")
        pre = {}
        coords = problem.data.domain.centroids()
        for var in problem.variables:
            p = self.params(var)
            if p["cutoffs"] is None:
                raise ValueError(f"variable {var}: cutoffs are required")
            cut = check_cutoffs(p["cutoffs"])
            if p["variogram"] is not None and p["variograms"] is not None:
                raise ValueError("give `variogram` (median form) or `variograms` (one per cutoff), not both")
            if p["variograms"] is not None:
                models = list(p["variograms"])
                if len(models) != cut.size:
                    raise ValueError(f"{len(models)} variograms for {cut.size} cutoffs")
            else:
                models = [p["variogram"] if p["variogram"] is not None else GaussianVariogram()]
            for g in models:
                if getattr(g, "kind", None) == "power":
                    raise ValueError("a power variogram has no sill: indicator kriging refuses it")
            if p["mean"] not in (None, "global"):
                raise ValueError(f"mean={p['mean']!r}: None (ordinary) or 'global' (simple about the global proportions)")
            if p["neighborhood"] is not None and not isinstance(p["neighborhood"], MetricBall):
                raise TypeError("neighborhood must be a MetricBall")
            z = np.asarray(problem.data[var], dtype=np.float64)
            inds = np.flatnonzero(~np.isnan(z))
            if inds.size == 0:
                raise AssertionError(f"all samples of {var} are missing, aborting...")
            k = p["maxneighbors"]
            if k is not None:
                if int(k) > MAX_NEIGHBORS:
                    raise ValueError(f"maxneighbors {k}: at most {MAX_NEIGHBORS} (None: the global neighbourhood)")
                _, k = searcher_ui(PointSet(coords[inds]), int(k), p["distance"], p["neighborhood"])
                if not 1 <= p["minneighbors"] <= k:
                    raise ValueError("invalid min/max number of neighbors")
            _distance(p)
            fstar = None
            if p["mean"] == "global":
                w = None if p["weights"] is None else np.asarray(p["weights"], dtype=np.float64).ravel()
                if w is not None and w.size != z.size:
                    raise ValueError(f"{w.size} weights for {z.size} data rows")
                fstar = global_proportions(z, cut, w)
            pre[var] = dict(x=np.ascontiguousarray(coords[inds]), z=np.ascontiguousarray(z[inds]), cutoffs=cut,
                            models=models, k=k, fstar=fstar, params=p)
        return pre

    def _global(self, q, xdom):
        """The global neighbourhood from what exists: one kriging handle per distinct system, the K indicator (or
        residual) columns as a batch, F* added back, then the order-relation correction on the device."""
        eng = self.engine
        cut, fstar, x, z = q["cutoffs"], q["fstar"], q["x"], q["z"]
        ind = (z[None, :] <= cut[:, None]).astype(np.float64)
        if fstar is not None:
            ind = ind - fstar[:, None]
        variant = SK if fstar is not None else OK
        rows = []
        groups = [(q["models"][0], range(cut.size))] if len(q["models"]) == 1 else \
            [(g, (i,)) for i, g in enumerate(q["models"])]
        for g, qs in groups:
            h = eng.Krig(g, variant, x, z, mean=0.0)
            try:
                zb = np.ascontiguousarray(ind[list(qs)])
                if hasattr(xdom, "is_cuda"):
                    import torch
                    zb = torch.as_tensor(zb, device=xdom.device)
                rows.append(np.array(_host(h.predict_global_batch(xdom, zb))))
            finally:
                h.close()
        raw = np.ascontiguousarray(np.concatenate(rows, axis=0).T)          # m x K
        if fstar is not None:
            raw = raw + fstar[None, :]
        ccdf, _, _ = eng.ik_order_relations(raw.copy())
        return ccdf

    def solve(self, problem: EstimationProblem):
        pre = self.preprocess(problem)
        pdom = problem.domain
        m = pdom.nelements()
        xdom = _domain_points(self.engine, pdom, 0, m)
        cols, cutoffs = {}, {}
        for var in problem.variables:
            q = pre[var]
            p = q["params"]
            if q["k"] is None:
                ccdf = self._global(q, xdom)
            else:
                radius, radii = _ball(p["neighborhood"])
                models = q["models"][0] if len(q["models"]) == 1 else q["models"]
                ccdf, st = self.engine.ik_predict_knn(q["x"], q["z"], xdom, q["cutoffs"], models, q["k"],
                                                      p["minneighbors"], fstar=q["fstar"], radius=radius, radii=radii,
                                                      distance=_distance(p), **_rot_kw(p["neighborhood"]))[:2]
                ccdf = _host(ccdf)
            for i in range(q["cutoffs"].size):
                cols[f"{var}_ccdf_{i}"] = np.ascontiguousarray(ccdf[:, i])
            cutoffs[var] = q["cutoffs"]
        sol = georef(cols, pdom)
        # what postik needs besides the columns: `solution.cutoffs[var]`.  It is an attribute of THIS table; a copy or a
        # view made from its columns does not carry it, and postik then takes `cutoffs=`.
        sol.cutoffs = cutoffs
        return sol


MAX_CATEGORIES = 16


def _codes(values, labels, what) -> np.ndarray:
    """Category codes 0 .. K-1 (as doubles, NaN for a missing value) of `values` among `labels`."""
    out = np.full(len(values), np.nan)
    lookup = {lab.item() if hasattr(lab, "item") else lab: i for i, lab in enumerate(labels)}
    for i, v in enumerate(values):
        v = v.item() if hasattr(v, "item") else v
        if v is None or (isinstance(v, float) and np.isnan(v)):
            continue
        if v not in lookup:
            raise ValueError(f"{what}: the value {v!r} is not among the categories")
        out[i] = lookup[v]
    return out


class SISSolver(_Solver):
    """Sequential indicator simulation (GSLIB sisim, median form; gss.h, gss_sis_realize): realisations of a categorical
    variable, or of a continuous one without a Gaussian model.  Per variable, one of `cutoffs` (continuous: 1 .. 16,
    increasing) or `categories` (categorical: 2 .. 16 labels; the realisations carry these labels, in their dtype), and
    `variogram`, the one indicator variogram.  `proportions`: the global ccdf at the cutoffs / the global proportions of
    the categories; default: those of the data (with declustering `weights`, one per data row); required without data.
    Continuous only: `zmin`, `zmax` (default: the data's range, moved 5 % of the larger of that range and the cutoffs'
    beyond an end cutoff that it does not enclose strictly; required without data) and `tail_power` of the ccdf model.
    `path`, `minneighbors`, `maxneighbors`, `neighborhood`, `distance` and the globals `init`, `rng`, `mask` as SGS."""
    PARAMS = dict(cutoffs=None, categories=None, variogram=None, proportions=None, weights=None, zmin=None, zmax=None,
                  tail_power=(1.0, 1.0), path="linear", minneighbors=1, maxneighbors=10, neighborhood=None,
                  distance="euclidean")
    GLOBALS = dict(init="nearest", rng=None, mask="after")

    def _draw_rule(self, var, p, z, w):
        """(kind, cutoffs, fstar, zmin, zmax, tail_power) of a variable from its parameters and data values `z`
        (continuous: the values; categorical: codes; NaN: missing)."""
        have = ~np.isnan(z)
        if p["categories"] is not None:
            K = len(p["categories"])
            if not 2 <= K <= MAX_CATEGORIES:
                raise ValueError(f"{K} categories: 2 .. {MAX_CATEGORIES}")
            if p["proportions"] is not None:
                fs = np.asarray(p["proportions"], dtype=np.float64).reshape(-1)
            elif have.any():
                fs = np.diff(np.concatenate([[0.0], global_proportions(z, np.arange(K, dtype=np.float64), w)]))
            else:
                raise ValueError(f"variable {var}: without data the proportions are required")
            if fs.size != K or np.any(fs < 0.0) or abs(fs.sum() - 1.0) > 1e-9:
                raise ValueError(f"variable {var}: {K} proportions in [0, 1] that sum to 1 are required")
            return "categorical", None, fs, 0.0, 0.0, (1.0, 1.0)
        cut = check_cutoffs(p["cutoffs"])
        if p["proportions"] is not None:
            fs = np.asarray(p["proportions"], dtype=np.float64).reshape(-1)
        elif have.any():
            fs = global_proportions(z, cut, w)
        else:
            raise ValueError(f"variable {var}: without data the proportions are required")
        if fs.size != cut.size or np.any(fs < 0.0) or np.any(fs > 1.0) or np.any(np.diff(fs) < 0.0):
            raise ValueError(f"variable {var}: {cut.size} non-decreasing proportions in [0, 1] are required")
        zmin, zmax = p["zmin"], p["zmax"]
        if (zmin is None or zmax is None) and not have.any():
            raise ValueError(f"variable {var}: without data zmin and zmax are required")
        if have.any():
            lo, hi = float(np.min(z[have])), float(np.max(z[have]))
            step = 0.05 * (max(hi - lo, cut[-1] - cut[0]) or 1.0)
            zmin = (lo if lo < cut[0] else cut[0] - step) if zmin is None else zmin
            zmax = (hi if hi > cut[-1] else cut[-1] + step) if zmax is None else zmax
        if not (zmin < cut[0] and zmax > cut[-1]):
            raise ValueError("zmin / zmax must enclose the cutoffs strictly")
        wlo, whi = (float(t) for t in p["tail_power"])
        if not (wlo > 0.0 and whi > 0.0):
            raise ValueError("tail exponents must be positive")
        return "continuous", cut, fs, float(zmin), float(zmax), (wlo, whi)

    def preprocess(self, problem):
        if not isinstance(problem, SimulationProblem):
            raise TypeError("SISSolver solves SimulationProblems")
        if not hasattr(self.engine.SGS, "realize_indicator"):
            raise NotImplementedError(f"engine {getattr(self.engine, 'name', self.engine)!r} has no indicator simulation")
        pdom = problem.domain
        cent = pdom.centroids()
        N = cent.shape[0]
        mask = self.globals.get("mask", "after")
        if mask not in ("after", "during"):
            raise ValueError(f"mask={mask!r}: 'after' or 'during'")
        pre = {}
        for var in problem.variables:
            p = self.params(var)
            if (p["cutoffs"] is None) == (p["categories"] is None):
                raise ValueError(f"variable {var}: give `cutoffs` (continuous) or `categories` (categorical)")
            if p["variogram"] is None:
                raise ValueError(f"variable {var}: the indicator variogram is required")
            if getattr(p["variogram"], "kind", None) == "power":
                raise ValueError("a power variogram has no sill: indicator simulation refuses it")
            data, z, w = problem.data, np.empty(0), None
            if data is not None and var in data.table:
                raw = data[var]
                z = _codes(raw, p["categories"], f"variable {var}") if p["categories"] is not None else \
                    np.asarray(raw, dtype=np.float64)
                if p["weights"] is not None:
                    w = np.asarray(p["weights"], dtype=np.float64).ravel()
                    if w.size != z.size:
                        raise ValueError(f"{w.size} weights for {z.size} data rows")
                data = GeoTable({var: z}, data.domain)
            kind, cut, fs, zmin, zmax, tail = self._draw_rule(var, p, z, w)
            path, order, path_seed = p["path"], None, None
            if isinstance(path, tuple) and len(path) == 2 and path[0] == "random":
                path_seed = int(path[1])
            else:
                order = _path_order(path, N, pdom)
            dist = _distance(p)
            if dist is not None and not isinstance(dist, str) and mask != "after":
                raise NotImplementedError("the haversine search distance needs mask='after'")
            dlocs, zd = _initbuff(self.engine, self.globals.get("init", "nearest"), cent, data, var, pdom)
            _, nmax = searcher_ui(pdom, p["maxneighbors"], p["distance"], p["neighborhood"])
            radius, radii = _ball(p["neighborhood"])

            def draw(h, seed, first, count, rule=(kind, cut, fs, zmin, zmax, tail)):
                return h.realize_indicator(*rule, seed, first, count)

            labels = None if p["categories"] is None else np.asarray(p["categories"])
            pre[var] = dict(labels=labels, plan=_SGSPlan(
                self.engine, (p["variogram"], cent, dlocs, zd, 0.0, nmax, p["minneighbors"], radius, radii), N, path_seed,
                order, mask == "after", dist, draw=draw, **_rot_kw(p["neighborhood"])))
        pre["_run"] = _run_state(self, problem)
        return pre

    @staticmethod
    def _labelled(q, y):
        y = _host(y)
        return y if q["labels"] is None else q["labels"][y.astype(np.int64)]

    def solvesingle(self, problem, covars, preproc):
        r = _next_real(preproc, covars)
        run = preproc["_run"]
        return {var: self._labelled(preproc[var], preproc[var]["plan"].realize(run["seed"] + run["vindex"][var], r, 1))[0]
                for var in covars}

    def solve(self, problem, gather: bool = True):
        pre = self.preprocess(problem)
        run = pre["_run"]
        rank, ws = parallel.world()
        lo, hi = parallel.shard_range(problem.nreals, rank, ws)
        reals = {}
        for var in problem.variables:
            plan = pre[var]["plan"]
            y = _host(plan.realize(run["seed"] + run["vindex"][var], lo, hi - lo))
            plan.close()
            if gather and ws > 1:
                y = parallel.all_gather_concat(y, problem.nreals)
            y = self._labelled(pre[var], y)
            reals[var] = [y[r] for r in range(y.shape[0])]
        return Ensemble(problem.domain, reals)


def postik(solution: GeoTable, var: str, zmin, zmax, tail_power=(1.0, 1.0), thresholds=(), probs=(), cutoffs=None,
           engine=None) -> GeoTable:
    """E-type mean `<var>_etype`, conditional variance `<var>_cvar`, `<var>_pabove_<i>` = P(z > thresholds[i]) and
    quantiles `<var>_q_<i>` at probs[i] from the corrected ccdf columns `<var>_ccdf_*` of an IndicatorKrigingSolver
    solution, under the ccdf model of gss_ik_post: linear inside the classes, power tails to `zmin` / `zmax` with the
    exponents `tail_power` (1: linear).  `cutoffs`: only for a table that does not carry them."""
    from .engine import default_engine
    if cutoffs is None:
        cutoffs = (getattr(solution, "cutoffs", None) or {}).get(var)
        if cutoffs is None:
            raise ValueError(f"the table carries no cutoffs for {var}: pass cutoffs=")
    cut = check_cutoffs(cutoffs)
    names = [f"{var}_ccdf_{i}" for i in range(cut.size)]
    missing = [n for n in names if n not in solution.table]
    if missing:
        raise KeyError(f"columns {missing} are not in the table")
    wlo, whi = (float(t) for t in tail_power)
    if not (zmin < cut[0] and zmax > cut[-1]):
        raise ValueError("zmin / zmax must enclose the cutoffs strictly")
    if not (wlo > 0.0 and whi > 0.0):
        raise ValueError("tail exponents must be positive")
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    pr = np.asarray(probs, dtype=np.float64).reshape(-1)
    if thr.size > 16 or pr.size > 16:
        raise ValueError("at most 16 thresholds and 16 probabilities")
    if np.any((thr < zmin) | (thr > zmax)):
        raise ValueError("thresholds must lie inside [zmin, zmax]")
    if np.any((pr <= 0.0) | (pr >= 1.0)):
        raise ValueError("probabilities must lie inside (0, 1)")
    ccdf = np.ascontiguousarray(np.stack([np.asarray(solution[n], dtype=np.float64) for n in names], axis=1))
    out = (engine or default_engine()).ik_post(ccdf, cut, zmin, zmax, (wlo, whi), thr, pr)
    cols = {f"{var}_etype": out["etype"], f"{var}_cvar": out["cvar"]}
    for i in range(thr.size):
        cols[f"{var}_pabove_{i}"] = np.ascontiguousarray(out["pabove"][:, i])
    for i in range(pr.size):
        cols[f"{var}_q_{i}"] = np.ascontiguousarray(out["quant"][:, i])
    return georef(cols, solution.domain)
