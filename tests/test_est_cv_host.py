"""Cross-validation of IDWSolver / LWRSolver without a device: the reference (tests/est_cv_ref.py) against hand-computed
answers, the twin's dispatch on a stand-in engine that answers from the reference, the refusals, the argument checks of
gss_idw_cv / gss_lwr_cv that need no device, the condition of the LWR designs the GPU cases use, and the compiled
instantiations of the two new kernel families against the cases of tests/test_gpu_est_cv.py."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crossval_ref as CR
import est_cv_ref as R
import test_gpu_est_cv as G

import gss
from gss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_census

X4, Z4 = np.array([[0.0], [1.0], [3.0], [6.0]]), np.array([1.0, 2.0, 4.0, 8.0])


# ---- the reference ----------------------------------------------------------------------------------------------------------
def test_reference_against_hand_computed_answers():
    pred, dist, st = R.predict("idw", X4, Z4, 4, fold=[0, 0, 1, 1])           # every eligible sample
    assert not st.any()
    assert pred[0] == pytest.approx((4 / 3 + 8 / 6) / (1 / 3 + 1 / 6), rel=1e-15) and dist[0] == 3.0
    assert pred[3] == pytest.approx((1 / 6 + 2 / 5) / (1 / 6 + 1 / 5), rel=1e-15) and dist[3] == 5.0
    pred, dist, st = R.predict("idw", X4, Z4, 4)                              # leave-one-out
    assert pred[1] == pytest.approx((1.0 + 2.0 + 1.6) / 1.7, rel=1e-15) and dist[1] == 1.0
    pred, dist, st = R.predict("idw", X4, Z4, 4, exponent=2.0)
    assert pred[1] == pytest.approx((1.0 + 1.0 + 8 / 25) / (1.0 + 0.25 + 1 / 25), rel=1e-15)
    # leave-ball-out: the sample at distance 2 sits exactly on the radius and is left out with the one at distance 1
    pred, dist, st = R.predict("idw", X4, Z4, 4, exclude_radius=2.0)
    assert pred[1] == 8.0 and dist[1] == 5.0 and not st.any()
    pred, dist, st = R.predict("idw", X4, Z4, 4, exclude_radius=2.0, lattice=True)
    assert pred[1] == 8.0 and dist[1] == 5.0
    # one nearest eligible neighbour; a neighbourhood ball that leaves nobody: missing
    pred, dist, st = R.predict("idw", X4, Z4, 1, fold=[0, 0, 1, 1])
    assert pred.tolist() == [4.0, 4.0, 2.0, 2.0] and dist.tolist() == [3.0, 2.0, 2.0, 5.0]
    pred, dist, st = R.predict("idw", X4, Z4, 4, fold=[0, 0, 1, 1], radius=2.5)
    assert st.tolist() == [1, 0, 0, 1] and np.isnan(pred[0]) and pred[1] == 4.0 and pred[2] == 2.0
    # a single fold: nothing to predict from
    assert R.predict("idw", X4, Z4, 4, fold=[7, 7, 7, 7])[2].tolist() == [1, 1, 1, 1]
    # LWR reproduces a linear field from any two or more eligible samples
    zl = 2.0 * X4[:, 0] + 1.0
    pred, var, st = R.predict("lwr", X4, zl, 4)
    assert not st.any() and np.allclose(pred, zl, rtol=0, atol=1e-12)
    pred2 = R.predict("lwr", X4, np.stack([zl, -zl]), 4, fold=[0, 1, 0, 1])[0]
    assert pred2.shape == (2, 4) and np.allclose(pred2[1], -zl, rtol=0, atol=1e-12)


def test_reference_duplicates_across_and_inside_a_fold():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 2.0]])
    z = np.array([1.0, 2.0, 5.0, 3.0])
    pred, dist, st = R.predict("idw", x, z, 4, fold=[0, 1, 2, 3])
    assert pred[0] == 5.0 and dist[0] == 0.0 and pred[2] == 1.0
    pred, dist, st = R.predict("idw", x, z, 4, fold=[0, 1, 0, 3])              # the duplicate shares the fold: invisible
    assert pred[0] == pytest.approx((2.0 + 1.5) / 1.5) and dist[0] == 1.0 and pred[2] == pred[0]
    idx, cnt = R.lists(x, 2, fold=[0, 1, 0, 3])
    assert idx[0].tolist() == [1, 3] and idx[1].tolist() == [0, 2]             # ties fall to the lower index


def test_lwr_designs_of_the_gpu_cases_are_well_conditioned():
    """Every LWR cell of the grid: the kept ones lie below the cap, exactly the cells named in DROPPED above it, each at
    the condition the table states; every other cell of the issue's grid is run."""
    worst, over = 0.0, {}
    for c in G.GRID:
        _, s = G.split(c["search"])
        if c["method"] != "lwr" or "distance" in s:
            continue
        x, z, fold = G.problem_of(c)
        idx, cnt = R.lists(x, min(c["k"], c["n"] - 1), fold, **s)
        cond = R.lwr_design_cond(x, idx, cnt, c["weight"])
        if cond >= G.COND_CAP:
            over[G.ident(c)] = cond
        else:
            worst = max(worst, cond)
    print("largest condition of X'WX over the LWR cases that run: %.3g; dropped: %s" % (worst, over))
    assert worst < G.COND_CAP == 1e6 and set(over) == set(G.DROPPED)
    for name, cond in over.items():
        assert cond == pytest.approx(G.DROPPED[name], rel=0.05)
    ran = {(c["method"], c["n"], c["k"], c["dim"], c["fold"]) for c in G.CASES if not c["search"]}
    want = {(m, n, k, d, f) for m in ("idw", "lwr") for d in (1, 2, 3) for f in ("loo", "ids", "block")
            for n, k in ((37, 5), (37, 16), (130, 17), (130, 64), (70, 70), (1100, 1100))}
    assert len(want - ran) == len(G.DROPPED) == 4 and all(m == "lwr" and k == 5 for m, _, k, _, _ in want - ran)
    kept5 = [c for c in G.CASES if c["method"] == "lwr" and c["k"] == 5]
    assert {c["dim"] for c in kept5} == {1, 2, 3} and {c["weight"] for c in kept5} == {G.EXP, G.TRI}


# ---- the twin ---------------------------------------------------------------------------------------------------------------
class _Engine:
    """Answers idw_cv / lwr_cv from the reference and records the calls."""
    calls = []

    @classmethod
    def _cv(cls, method, x, z, k, fold=None, exclude_radius=None, minneighbors=1, radius=None, radii=None, distance=None,
            rotation=None, **est):
        cls.calls.append(dict(method=method, n=x.shape[0], zshape=np.shape(z), k=k, fold=fold,
                              exclude_radius=exclude_radius, est=est, radius=radius, radii=radii, distance=distance))
        return R.predict(method, x, z, k, fold, exclude_radius, minneighbors, radius, radii, distance, rotation, **est)

    @classmethod
    def idw_cv(cls, x, z, k, **kw):
        return cls._cv("idw", x, z, k, **kw)

    @classmethod
    def lwr_cv(cls, x, z, k, **kw):
        return cls._cv("lwr", x, z, k, **kw)

    cv_summary = staticmethod(CR.summary)


def _table(n=40, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, 2))
    cols = {v: np.sin(0.05 * x[:, 0] + i) + 0.1 * rng.normal(size=n) for i, v in enumerate(("a", "b", "c"))}
    cols["c"][5] = np.nan
    return gss.georef(cols, gss.PointSet(x)), x


def test_cverror_takes_an_idw_solver():
    """Fails on the parent commit: TypeError("cross-validation is available for KrigingSolver and CoKrigingSolver ...")."""
    data, x = _table()
    problem = gss.EstimationProblem(data, gss.PointSet(x[:1]), ("a",))
    e = gss.cverror(gss.IDWSolver(a=dict(maxneighbors=6), engine=_Engine), problem, gss.KFoldValidation(4, rng=2))
    fold, _ = gss.KFoldValidation(4, rng=2).folds(x)
    pred = R.predict("idw", x, np.asarray(data["a"]), 6, fold)[0]
    z = np.asarray(data["a"])
    assert e == {"a": pytest.approx(np.mean([np.mean((z - pred)[fold == f] ** 2) for f in range(4)]), rel=1e-12)}
    assert set(gss.cverror(gss.LWRSolver(a=dict(maxneighbors=8), engine=_Engine), problem)) == {"a"}


def test_variables_share_one_call_and_maxneighbors_maps_to_k():
    data, x = _table()
    _Engine.calls = []
    solver = gss.IDWSolver(a=dict(exponent=2, maxneighbors=7), b=dict(exponent=2, maxneighbors=7),
                           c=dict(exponent=2, maxneighbors=7), engine=_Engine)
    res = gss.cross_validate(data, solver, gss.BlockValidation(30.0))
    assert list(res) == ["a", "b", "c"] and len(_Engine.calls) == 2          # c misses a sample: a call of its own
    first, second = _Engine.calls
    assert first["zshape"] == (2, 40) and first["k"] == 7 and first["est"] == dict(exponent=2.0)
    assert second["zshape"] == (39,) and second["n"] == 39
    assert np.array_equal(first["fold"], gss.BlockValidation(30.0).folds(x)[0])
    assert np.array_equal(res["c"].indices, np.delete(np.arange(40), 5))
    for v in ("a", "b"):
        r = res[v]
        want = R.predict("idw", x, np.asarray(data[v]), 7, first["fold"], exponent=2.0)
        assert np.array_equal(r.pred, want[0]) and np.array_equal(r.aux["%s_distance" % v], want[1])
        assert r.variance is None and np.array_equal(r.residual, r.z - r.pred)
        assert r.summary.mse_std_n == 0.0 and np.isnan(r.summary.mean_std) and np.isnan(r.summary.msq_std)
    # maxneighbors=None and anything >= n: every eligible sample (k = n), with every method, leave-ball-out included
    for nmax, method in ((None, gss.LeaveBallOut(8.0)), (40, None), (500, gss.KFoldValidation(5, rng=0))):
        _Engine.calls = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = gss.cross_validate(data, gss.LWRSolver(a=dict(maxneighbors=nmax), engine=_Engine), method)["a"]
        (call,) = _Engine.calls
        assert call["k"] == 40 and call["est"] == dict(weight=(0, 3.0, 2.0)) and list(r.aux) == ["a_variance"]
        assert call["exclude_radius"] == (8.0 if nmax is None else None)
    _Engine.calls = []
    gss.cross_validate(data, gss.IDWSolver(a=dict(maxneighbors=39), c=dict(maxneighbors=39), engine=_Engine))
    # a: 39 < n = 40 is k = min(nmax, n - 1) = 39 nearest; c: 39 >= n = 39 is every eligible sample, k = n
    assert [(c["n"], c["k"]) for c in _Engine.calls] == [(40, 39), (39, 39)]
    # neighbourhood and distance reach the engine as they reach the prediction calls
    _Engine.calls = []
    gss.cross_validate(data, gss.IDWSolver(a=dict(neighborhood=gss.MetricBall(35.0), maxneighbors=5),
                                           b=dict(distance="cityblock", maxneighbors=5), engine=_Engine))
    assert [(c["radius"], c["distance"]) for c in _Engine.calls] == [(35.0, None), (None, "cityblock")]


def test_refusals_name_what_is_refused():
    data, x = _table()
    comp = np.empty(40, dtype=object)
    comp[:] = [gss.Composition([0.2, 0.3, 0.5])] * 40
    cdata = gss.georef(dict(q=comp), gss.PointSet(x))
    with pytest.raises(TypeError, match="compositional"):
        gss.cross_validate(cdata, gss.IDWSolver(q={}, engine=_Engine))
    with pytest.raises(NotImplementedError, match="callable weightfun"):
        gss.cross_validate(data, gss.LWRSolver(a=dict(weightfun=lambda h: 1.0 - h), engine=_Engine))
    with pytest.raises(TypeError, match="IDWSolver and LWRSolver, not LUGS"):
        gss.cross_validate(data, gss.LUGS())
    with pytest.raises(TypeError, match="engine with `idw_cv`"):
        gss.cross_validate(data, gss.IDWSolver(a={}, engine=CR.CVOracleEngine))
    # a solver that names no variable is refused as every estimator was; naming one with the defaults is enough
    for make in (gss.IDWSolver, gss.LWRSolver):
        with pytest.raises(TypeError, match="names none"):
            gss.cross_validate(data, make(engine=_Engine))
    _Engine.calls = []
    assert list(gss.cross_validate(data, gss.IDWSolver(a={}, engine=_Engine))) == ["a"]    # a GeoTable: the named ones
    assert [c["k"] for c in _Engine.calls] == [40] and _Engine.calls[0]["est"] == dict(exponent=1.0)


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_bound_and_the_shim_is_documented_as_not_binding_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gss.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in (("gss_idw_cv", 21), ("gss_lwr_cv", 23)):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, src) and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name]) == nargs
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _call(method, x, z, fold=None, ex=-1.0, k=2, minn=1, metric=0, mpar=0.0, idx=None, nz=1):
    n, dim = x.shape
    pred, aux = np.empty((nz, n)), np.empty(n)
    extra = (1.0,) if method == "idw" else (0, 3.0, 2.0)
    fn = getattr(_lib.load(), "gss_%s_cv" % method)
    return fn(_lib.ptr(x), _lib.ptr(z), n, dim, nz, None if fold is None else _lib.ptr(fold), ex, k, minn, -1.0, None,
              metric, mpar, *extra, _lib.ptr(pred), _lib.ptr(aux), None, None if idx is None else _lib.ptr(idx), None,
              _lib.MEM_HOST, None)


@pytest.mark.parametrize("method", ["idw", "lwr"])
def test_invalid_arguments_do_not_need_a_device(method):
    x, z = np.ascontiguousarray(np.random.default_rng(0).uniform(0, 1, (6, 2))), np.arange(6.0)
    bad = np.array([0, 1, -2, 1, 0, 1], dtype=np.int32)
    assert _call(method, x, z, fold=bad) == _lib.ERR_INVALID and "fold id -2 of sample 2" in _lib.last_error()
    assert _call(method, x, z, ex=float("nan")) == _lib.ERR_INVALID and "NaN" in _lib.last_error()
    assert _call(method, x[:1], z[:1], k=1) == _lib.ERR_INVALID and "two samples" in _lib.last_error()
    assert _call(method, x, z, k=0) == _lib.ERR_INVALID and "outside 1..n" in _lib.last_error()
    assert _call(method, x, z, k=7) == _lib.ERR_INVALID and "outside 1..n" in _lib.last_error()
    assert _call(method, x, z, k=6, idx=np.empty((6, 6), dtype=np.int32)) == _lib.ERR_INVALID
    assert "idx_out" in _lib.last_error()
    assert _call(method, x, z, k=3, metric=3, mpar=6371.0) == _lib.ERR_UNSUPPORTED and "haversine" in _lib.last_error()
    assert _call(method, x, z, k=3, minn=4) == _lib.ERR_INVALID
    assert _call(method, x, z, k=3, nz=0) == _lib.ERR_INVALID


# ---- the compiled kernels -----------------------------------------------------------------------------------------------------
def test_every_compiled_instantiation_of_the_new_families_is_named_by_a_gpu_case():
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    found = [(f, tuple(int(a) if a.lstrip("-").isdigit() else a for a in args))
             for f, args in kernel_census.census(_lib.LIB_PATH) if f in ("est_cv_all_kernel", "idw_cv_all_fast_kernel")]
    assert len(found) == len(set(found)) == 12
    assert set(found) == {("est_cv_all_kernel", (d, zc)) for d in (1, 2, 3) for zc in (1, 4)} | \
        {("idw_cv_all_fast_kernel", (d, e)) for d in (1, 2, 3) for e in ("true", "false")}
    named = {G.kernel_of(c) for c in G.CASES} - {None}
    assert named == set(found)
    # both sides of EST_TILE = 1 024 for both families, and the search path on either side of 16 and 64 neighbours
    for fam in ("est_cv_all_kernel", "idw_cv_all_fast_kernel"):
        assert {c["n"] > 1024 for c in G.CASES if (G.kernel_of(c) or ("",))[0] == fam} == {True, False}
    assert {5, 16, 17, 64, 65, 199} <= {c["k"] for c in G.CASES if c["k"] < c["n"]}
    assert {1, 4, 5} <= {c["nz"] for c in G.CASES} and {"loo", "ids", "block"} == {c["fold"] for c in G.CASES}
