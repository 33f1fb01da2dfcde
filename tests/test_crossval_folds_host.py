"""Cross-validation by folds under the global neighbourhood, host side: the block identity pinned against refits, the
front-end through a stand-in engine whose handle offers cv_global_folds, the refusal that stays, and the ABI.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

import gss
from gss import _lib
from oracle import kriging as K
from oracle.variogram import Variogram

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crossval_folds_ref as FR
import crossval_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ranges that keep the condition number of the systems in the low thousands (tests/test_crossval_host.py): the two
# float64 routes then agree to 1e-12 up to the conditioning of the fold blocks, for which 1e-10 leaves two orders
MODELS = {"exponential": Variogram("exponential", range=30.0),
          "spherical": Variogram("spherical", range=45.0, nugget=0.1),
          "matern32": Variogram("matern", range=20.0, nu=1.5)}
VARIANTS = {"sk": (K.SK, 2, dict(mean=3.5)), "ok": (K.OK, 3, {}), "uk2": (K.UK, 2, dict(degree=1)),
            "edk": (K.EDK, 2, dict(ndrift=2))}


def problem(n, dim, seed, ndrift=0, offset=0.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, dim))
    drift = None
    if ndrift:
        drift = np.stack([0.01 * x[:, 0] + rng.normal(0, 0.2, n), np.sin(0.05 * x[:, 1]) + rng.normal(0, 0.2, n)], axis=1)
    return x, rng.normal(size=n) + offset, drift


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("n,nfolds", [(65, 4), (130, 10), (130, 40)])
def test_block_identity_equals_refits(model, variant, n, nfolds):
    var_, dim, kw = VARIANTS[variant]
    kw = dict(kw)
    x, z, drift = problem(n, dim, n + nfolds + len(model), kw.pop("ndrift", 0), offset=1.0e4 if variant != "sk" else 3.5)
    fold = 7 * np.random.default_rng(n).permutation(np.arange(n) % nfolds) + 3      # shuffled, ids not compact
    rp, rv, rs = FR.folds_refit(var_, MODELS[model], x, z, fold, drift_data=drift, **kw)
    cp, cv = FR.folds_closed_form(var_, MODELS[model], x, z, fold, drift_data=drift, **kw)
    assert not rs.any()
    assert np.max(np.abs(cp - rp) / (1.0 + np.abs(rp))) <= 1e-10 and np.max(np.abs(cv - rv) / (1.0 + np.abs(rv))) <= 1e-10


def test_singleton_folds_are_leave_one_out():
    x, z, _ = problem(40, 2, 3)
    a = FR.folds_closed_form(K.OK, MODELS["exponential"], x, z, np.arange(40))
    b = CR.loo_closed_form(K.OK, MODELS["exponential"], x, z)
    for u, v in zip(a, b):
        assert np.max(np.abs(u - v)) <= 1e-12


def _table(n, dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, dim))
    return gss.georef({"z": rng.normal(size=n)}, gss.PointSet(x)), x


@pytest.mark.parametrize("variant", ["sk", "ok", "uk"])
def test_folds_under_the_global_neighbourhood_reach_the_engine(variant):
    data, x = _table(60, 2, 5)
    z = np.asarray(data["z"])
    g, og = gss.ExponentialVariogram(range=30.0), Variogram("exponential", range=30.0)
    par = dict(sk=dict(mean=0.3), ok={}, uk=dict(degree=1))[variant]
    ov = dict(sk=K.SK, ok=K.OK, uk=K.UK)[variant]
    solver = gss.KrigingSolver(z=dict(variogram=g, **par), engine=FR.FoldOracleEngine)
    prob = gss.EstimationProblem(data, gss.CartesianGrid(4, 4), "z")
    for method, again in ((gss.KFoldValidation(5, rng=1), gss.KFoldValidation(5, rng=1)),
                          (gss.BlockValidation(30.0), gss.BlockValidation(30.0))):
        fold, nf = again.folds(x)
        res = gss.cross_validate(prob, solver, method)["z"]
        rp, rv, rs = FR.folds_refit(ov, og, x, z, fold, **par)
        assert np.array_equal(res.fold, fold) and np.array_equal(res.status, rs)
        assert np.array_equal(res.pred, rp) and np.array_equal(res.variance, rv)
        want, fmse = CR.summary(z, rp, rv, rs, fold, nf)
        assert res.summary.cverror == want["cverror"] and np.array_equal(res.summary.fold_mse, fmse)
        assert res.summary.fold_mse.shape == (nf,)
        assert gss.cverror(solver, prob, method) == {"z": want["cverror"]}
    # leave-one-out is still the leave-one-out call
    res = gss.cross_validate(prob, solver)["z"]
    assert res.fold is None and np.allclose(res.pred, CR.loo_closed_form(ov, og, x, z, **par)[0], rtol=0, atol=1e-9)


def test_ball_out_is_still_refused_and_so_are_folds_without_the_capability():
    data, _ = _table(30, 2, 4)
    g = gss.ExponentialVariogram(range=30.0)
    with pytest.raises(ValueError, match="global neighbourhood"):
        gss.cross_validate(data, gss.KrigingSolver(z=dict(variogram=g), engine=FR.FoldOracleEngine), gss.LeaveBallOut(5.0))
    with pytest.raises(ValueError, match="global neighbourhood"):
        gss.cross_validate(data, gss.KrigingSolver(z=dict(variogram=g), engine=CR.CVOracleEngine), gss.KFoldValidation(5))
    from gss.engine import KrigHandle
    assert hasattr(KrigHandle, "cv_global_folds")


def test_the_export_is_declared_bound_and_wrapped():
    name = "gss_krig_cv_global_folds"
    header = open(os.path.join(ROOT, "include", "gss.h")).read()
    shim = open(os.path.join(ROOT, "geostatssolvers.jl_amd", "julia", "GeoStatsSolversHIP.jl")).read()
    assert re.search(r"\bint32_t\s+%s\s*\(" % name, header)
    assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert "ccall((:%s, libgss)" % name in shim


def test_a_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    one = np.zeros(4)
    ids = np.zeros(4, dtype=np.int32)
    assert lib.gss_krig_cv_global_folds(None, None, _lib.ptr(one), _lib.ptr(one), None, 0, None) == _lib.ERR_INVALID
    assert lib.gss_krig_cv_global_folds(None, _lib.ptr(ids), _lib.ptr(one), _lib.ptr(one), None, 0, None) == _lib.ERR_INVALID
