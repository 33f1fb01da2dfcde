"""Cross-validation, host side: the reference pinned against itself (closed form = n refits), the fold constructors, the
front-end through the stand-in engine, the summary arithmetic, the ABI and the census of the fold-search kernels.  No GPU."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

import gss
from gss import _lib
from oracle import kriging as K
from oracle.variogram import Variogram

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import crossval_ref as CR
import kernel_census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Two float64 solutions of one system of condition number c differ by about c 2^-53, so the 1e-12 bar below needs systems
# with c below a few thousand: that fixes the ranges (Matern-3/2 with range 20 on 130 samples of a 100 x 100 square:
# c = 9e2; the smoother the model and the longer its range, the larger c)
MODELS = {"exponential": Variogram("exponential", range=30.0),
          "spherical": Variogram("spherical", range=45.0, nugget=0.1),
          "matern32": Variogram("matern", range=20.0, nu=1.5)}
# (variant, dim, kw): simple kriging with a mean, ordinary, universal degree 1 in 2-D and 3-D, two external drifts
VARIANTS = {"sk": (K.SK, 2, dict(mean=3.5)), "ok": (K.OK, 3, {}), "uk2": (K.UK, 2, dict(degree=1)),
            "uk3": (K.UK, 3, dict(degree=1)), "edk": (K.EDK, 2, dict(ndrift=2))}


def problem(n, dim, seed, ndrift=0, offset=0.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, dim))
    drift = None
    if ndrift:
        drift = np.stack([0.01 * x[:, 0] + rng.normal(0, 0.2, n), np.sin(0.05 * x[:, 1]) + rng.normal(0, 0.2, n)], axis=1)
    return x, rng.normal(size=n) + offset, drift


# ---- the reference itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("n", [17, 64, 130])
def test_closed_form_equals_brute_force_refits(model, variant, n):
    var_, dim, kw = VARIANTS[variant]
    kw = dict(kw)
    x, z, drift = problem(n, dim, n + len(model), kw.pop("ndrift", 0), offset=kw.get("mean", 0.0))
    a = CR.loo_refit(var_, MODELS[model], x, z, drift_data=drift, **kw)
    b = CR.loo_closed_form(var_, MODELS[model], x, z, drift_data=drift, **kw)
    for u, v in zip(a, b):
        assert np.max(np.abs(u - v) / (1.0 + np.abs(u))) <= 1e-12


def test_eligible_lists_follow_the_key_index_rule():
    x = np.array([[0.0, 0], [3, 4], [5, 0], [0, 5], [6, 8], [3, 4], [0, 0]])
    fold = np.array([0, 1, 1, 2, 2, 0, 1])
    idx, cnt = CR.eligible_lists(x, 3, fold)
    assert list(idx[0]) == [6, 1, 2] and cnt[0] == 3              # the duplicate in another fold first, then the tie
    assert list(idx[1]) == [5, 3, 0]                              # the duplicate of sample 1 lies in fold 0
    idx, cnt = CR.eligible_lists(x, 6, None, exclude_radius=5.0)
    assert list(idx[0][:cnt[0]]) == [4]                           # distance exactly 5 is excluded, the twin at 0 too
    idx, cnt = CR.eligible_lists(x, 6, None, exclude_radius=4.999)
    assert list(idx[0][:cnt[0]]) == [1, 2, 3, 5, 4]
    idx, cnt = CR.eligible_lists(x, 6, None, distance="chebyshev", exclude_radius=4.0)
    assert list(idx[0][:cnt[0]]) == [2, 3, 4]


# ---- fold constructors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,shuffle", [(10, 3, True), (103, 10, True), (64, 64, False), (7, 2, False)])
def test_kfold_sizes_differ_by_at_most_one_and_cover_every_sample(n, k, shuffle):
    ids, nf = gss.KFoldValidation(k, shuffle=shuffle, rng=5).folds(np.zeros((n, 2)))
    assert nf == k and ids.dtype == np.int32 and ids.shape == (n,)
    sizes = np.bincount(ids, minlength=k)
    assert sizes.sum() == n and sizes.max() - sizes.min() <= 1 and sizes.min() >= 1
    again, _ = gss.KFoldValidation(k, shuffle=shuffle, rng=5).folds(np.zeros((n, 2)))
    assert np.array_equal(ids, again)
    if not shuffle:
        assert np.array_equal(ids, np.arange(n) % k)
    with pytest.raises(ValueError):
        gss.KFoldValidation(n + 1).folds(np.zeros((n, 2)))


def test_block_validation_ids():
    x = np.array([[0.0, 0.0], [9.99, 0.0], [10.0, 0.0], [25.0, 0.0], [0.0, 10.0], [10.0, 19.9]])
    ids, nf = gss.BlockValidation(10.0).folds(x)
    # cells (0,0) (0,0) (1,0) (2,0) (0,1) (1,1): a sample on a block edge belongs to the upper block; ids compacted
    assert nf == 5 and list(ids) == [0, 0, 2, 4, 1, 3]
    ids, nf = gss.BlockValidation((10.0, 20.0)).folds(x)
    assert nf == 3 and list(ids) == [0, 0, 1, 2, 0, 1]
    ids, nf = gss.BlockValidation(2.5).folds(np.array([[1.0], [3.4], [3.5], [11.0], [6.0]]))       # 1-D, origin at 1.0
    assert nf == 4 and list(ids) == [0, 0, 1, 3, 2]
    with pytest.raises(ValueError):
        gss.BlockValidation((1.0, 2.0, 3.0)).folds(x)


# ---- front-end through the stand-in engine --------------------------------------------------------------------------
def _table(n, dim, seed, names=("z",)):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, dim))
    return gss.georef({v: rng.normal(size=n) + 2.0 * i for i, v in enumerate(names)}, gss.PointSet(x)), x


@pytest.mark.parametrize("variant", ["sk", "ok", "uk", "edk"])
def test_cross_validate_dispatches_like_the_solver(variant):
    data, x = _table(40, 2, 3)
    g, og = gss.ExponentialVariogram(range=30.0), Variogram("exponential", range=30.0)
    drifts = [lambda c: 0.01 * c[0], lambda c: float(np.sin(0.05 * c[1]))]
    par = dict(sk=dict(mean=0.3), ok={}, uk=dict(degree=1), edk=dict(drifts=drifts))[variant]
    okw = dict(sk=dict(mean=0.3), ok={}, uk=dict(degree=1), edk={})[variant]
    ov = dict(sk=K.SK, ok=K.OK, uk=K.UK, edk=K.EDK)[variant]
    dd = np.array([[f(c) for f in drifts] for c in x]) if variant == "edk" else None
    z = np.asarray(data["z"])
    prob = gss.EstimationProblem(data, gss.CartesianGrid(4, 4), "z")           # the domain is ignored
    # global neighbourhood: leave-one-out
    res = gss.cross_validate(prob, gss.KrigingSolver(z=dict(variogram=g, **par)), engine=CR.CVOracleEngine)["z"]
    pred, var_ = CR.loo_closed_form(ov, og, x, z, drift_data=dd, **okw)
    assert np.allclose(res.pred, pred, rtol=0, atol=1e-9) and np.allclose(res.variance, var_, rtol=0, atol=1e-9)
    assert np.array_equal(res.residual, z - res.pred) and res.fold is None and not res.status.any()
    assert res.summary.cverror == res.summary.mse == pytest.approx(np.mean((z - pred) ** 2), rel=1e-9)
    # moving neighbourhood, five folds
    solver = gss.KrigingSolver(z=dict(variogram=g, maxneighbors=8, minneighbors=2, **par), engine=CR.CVOracleEngine)
    method = gss.KFoldValidation(5, rng=1)
    res = gss.cross_validate(data, solver, method)["z"]
    fold, _ = gss.KFoldValidation(5, rng=1).folds(x)
    idx, cnt = CR.eligible_lists(x, 8, fold)
    rp, rv, rs = CR.solve_on_lists(ov, og, x, z, idx, cnt, 2, drift_data=dd, **okw)
    assert np.array_equal(res.fold, fold) and np.array_equal(res.status, rs)
    assert np.array_equal(res.pred, rp) and np.array_equal(res.variance, rv)
    want, fmse = CR.summary(z, rp, rv, rs, fold, 5)
    assert res.summary.cverror == want["cverror"] and np.array_equal(res.summary.fold_mse, fmse)
    assert gss.cverror(solver, prob, method) == {"z": want["cverror"]}


def test_methods_reach_the_engine_as_folds_and_exclusion_radius():
    data, x = _table(60, 2, 9)
    g = gss.SphericalVariogram(range=40.0, nugget=0.1)
    solver = gss.KrigingSolver(z=dict(variogram=g, maxneighbors=6, neighborhood=gss.MetricBall(35.0)),
                               engine=CR.CVOracleEngine)
    z = np.asarray(data["z"])
    res = gss.cross_validate(data, solver, gss.LeaveBallOut(12.0))["z"]
    idx, cnt = CR.eligible_lists(x, 6, None, radius=35.0, exclude_radius=12.0)
    rp, _, rs = CR.solve_on_lists(K.OK, Variogram("spherical", range=40.0, nugget=0.1), x, z, idx, cnt)
    assert np.array_equal(res.pred, rp, equal_nan=True) and np.array_equal(res.status, rs)
    res = gss.cross_validate(data, solver, gss.BlockValidation(25.0))["z"]
    fold, nf = gss.BlockValidation(25.0).folds(x)
    assert np.array_equal(res.fold, fold) and res.summary.fold_mse.shape == (nf,)
    # maxneighbors beyond n - 1 is clamped (searcher_ui warns about values beyond n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        big = gss.KrigingSolver(z=dict(variogram=g, maxneighbors=500), engine=CR.CVOracleEngine)
        res = gss.cross_validate(data, big)["z"]
    assert not res.status.any()


def test_refusals():
    data, _ = _table(30, 2, 4)
    g = gss.ExponentialVariogram(range=30.0)
    glob = gss.KrigingSolver(z=dict(variogram=g), engine=CR.CVOracleEngine)
    for method in (gss.KFoldValidation(5), gss.BlockValidation(20.0), gss.LeaveBallOut(5.0)):
        with pytest.raises(ValueError, match="global neighbourhood"):
            gss.cross_validate(data, glob, method)
    with pytest.raises(TypeError, match="IDWSolver"):
        gss.cross_validate(data, gss.IDWSolver(z=dict(maxneighbors=5)), engine=CR.CVOracleEngine)
    with pytest.raises(TypeError):
        gss.cross_validate(data, gss.LWRSolver(z=dict(maxneighbors=5)), engine=CR.CVOracleEngine)
    with pytest.raises(ValueError, match="point support"):
        gss.cross_validate(data, gss.KrigingSolver(z=dict(variogram=g, support="block"), engine=CR.CVOracleEngine))


def test_two_variables_on_the_same_samples_and_a_missing_value():
    data, x = _table(35, 2, 6, names=("a", "b"))
    data.table["b"][4] = np.nan
    g = gss.ExponentialVariogram(range=30.0)
    solver = gss.KrigingSolver(a=dict(variogram=g), b=dict(variogram=g), engine=CR.CVOracleEngine)
    res = gss.cross_validate(gss.EstimationProblem(data, gss.PointSet(x[:2]), ("a", "b")), solver)
    assert set(res) == {"a", "b"}
    keep = np.arange(35) != 4
    assert np.array_equal(res["b"].indices, np.flatnonzero(keep)) and res["a"].pred.shape == (35,)
    og = Variogram("exponential", range=30.0)
    for v, kp in (("a", np.ones(35, dtype=bool)), ("b", keep)):
        pred, var_ = CR.loo_closed_form(K.OK, og, x[kp], np.asarray(data[v])[kp])
        assert np.allclose(res[v].pred, pred, rtol=0, atol=1e-9) and np.allclose(res[v].variance, var_, rtol=0, atol=1e-9)
    assert gss.cverror(solver, gss.EstimationProblem(data, gss.PointSet(x[:2]), ("a", "b")), None).keys() == res.keys()


# ---- summary arithmetic ---------------------------------------------------------------------------------------------
def test_summary_arithmetic_against_direct_evaluation():
    z = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 3.0])
    pred = np.array([1.5, 1.0, np.nan, 8.0, 15.0, np.nan])
    var = np.array([0.25, 4.0, np.nan, 0.0, 1.0, np.nan])
    st = np.array([0, 0, 1, 0, 0, 2], dtype=np.uint8)
    fold = np.array([0, 0, 1, 2, 2, 3])
    s, fmse = CR.summary(z, pred, var, st, fold, 5)
    e = np.array([-0.5, 1.0, 0.0, 1.0])
    assert (s["n_ok"], s["n_missing"], s["n_singular"], s["mse_std_n"]) == (4.0, 1.0, 1.0, 3.0)
    assert s["me"] == e.mean() and s["mae"] == np.abs(e).mean() and s["mse"] == (e * e).mean()
    # the point with var = 0 counts in the plain means and not in the standardised ones
    assert s["mean_std"] == pytest.approx((-1.0 + 0.5 + 1.0) / 3) and s["msq_std"] == pytest.approx((1.0 + 0.25 + 1.0) / 3)
    assert np.array_equal(fmse[[0, 2]], [0.625, 0.5]) and np.isnan(fmse[[1, 3, 4]]).all()
    assert s["cverror"] == (0.625 + 0.5) / 2                      # folds without an OK point do not count
    s0, f0 = CR.summary(z, pred, var, st)
    assert f0 is None and s0["cverror"] == s0["mse"]


# ---- ABI ------------------------------------------------------------------------------------------------------------
NEW = ("gss_krig_cv_global", "gss_krig_cv_knn", "gss_cv_summary")


def test_the_new_exports_are_declared_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "gss.h")).read()
    shim = open(os.path.join(ROOT, "geostatssolvers.jl_amd", "julia", "GeoStatsSolversHIP.jl")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert "ccall((:%s, libgss)" % name in shim, name
    fields = re.search(r"typedef struct gss_cv_summary \{(.*?)\} gss_cv_summary_t;", header, flags=re.S).group(1)
    names = [f.strip() for f in fields.replace("double", "").replace(";", "").split(",")]
    assert names == [f for f, _ in _lib.CVSummary._fields_] and len(names) == 10
    for name in ("BlockValidation", "KFoldValidation", "LeaveBallOut", "LeaveOneOut", "cross_validate", "cverror"):
        assert name in gss.__all__


def test_invalid_arguments_are_refused_without_a_device():
    lib = _lib.load()
    one = np.zeros(4)
    out = _lib.CVSummary()
    import ctypes as C
    assert lib.gss_krig_cv_global(None, _lib.ptr(one), _lib.ptr(one), None, 0, None) == _lib.ERR_INVALID
    assert lib.gss_krig_cv_knn(None, None, -1.0, 1, 1, -1.0, None, 0, 0.0, _lib.ptr(one), _lib.ptr(one), None, None,
                               None, 0, None) == _lib.ERR_INVALID
    assert lib.gss_cv_summary(_lib.ptr(one), _lib.ptr(one), _lib.ptr(one), None, None, 4, 3, C.byref(out), None, 0,
                              None) == _lib.ERR_INVALID and "fold" in _lib.last_error()
    assert lib.gss_cv_summary(_lib.ptr(one), _lib.ptr(one), _lib.ptr(one), None, None, 0, 0, C.byref(out), None, 0,
                              None) == _lib.ERR_INVALID


def test_every_compiled_fold_search_kernel_is_named_by_a_gpu_case():
    """knn_fold_kernel<DIM, METRIC> is a family of its own (tests/search_cases.py holds the others fixed): its compiled
    instantiations are exactly the (dim, metric) pairs tests/test_gpu_crossval.py searches with."""
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    import test_gpu_crossval as G
    found = sorted((int(a[0]), int(a[1])) for f, a in kernel_census.census(_lib.LIB_PATH) if f == "knn_fold_kernel")
    assert found == sorted((d, m) for d in (1, 2, 3) for m in (0, 1, 2))
    named = {(c["dim"], _lib.METRICS[c.get("distance") or "euclidean"]) for c in G.SEARCH_CASES}
    assert set(found) == named
