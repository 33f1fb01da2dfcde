"""Cross-validation by folds under the global neighbourhood on the device (gss_krig_cv_global_folds) against refits with
oracle.kriging, one per fold (tests/crossval_folds_ref.py).  Means and variances: the project's 1e-9 (1 + |v|)
(DESIGN.md section 3).  The shapes are the smallest that reach every path: fold sizes on either side of the 16-tile and
of the 64-block of the Gram kernel, a fold of exactly S = 128 (solved in LDS) beside one of S + 1 (factor-and-inverse
routine of the fit), more than one row panel of W', constraint rows, a large dual-weight row."""
import os
import sys

import numpy as np
import pytest

from oracle import kriging as K
from oracle.variogram import Variogram

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crossval_folds_ref as FR
import crossval_ref as CR
from rotated_frame import frame, rot2

pytestmark = pytest.mark.gpu

TOL = 1e-9
S = 128                                                            # CVF_S of csrc/crossval_folds.hip


def close(a, b, tol=TOL):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= tol * (1.0 + np.abs(b))))


def _models():
    import gss
    return {"exponential": (gss.ExponentialVariogram(range=30.0), Variogram("exponential", range=30.0)),
            "spherical": (gss.SphericalVariogram(range=45.0, nugget=0.1), Variogram("spherical", range=45.0, nugget=0.1)),
            "matern32": (gss.MaternVariogram(range=20.0, order=1.5), Variogram("matern", range=20.0, nu=1.5))}


# (variant, dim, handle / oracle keywords, external drifts)
VARIANTS = {"sk": (K.SK, 2, dict(mean=3.5), 0), "ok": (K.OK, 3, {}, 0), "uk2": (K.UK, 2, dict(degree=1), 0),
            "uk3": (K.UK, 3, dict(degree=1), 0), "edk": (K.EDK, 2, {}, 2)}
MODEL_NAMES = ("exponential", "spherical", "matern32")


def problem(n, dim, seed, ndrift=0, offset=0.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, dim))
    drift = None
    if ndrift:
        drift = np.stack([0.01 * x[:, 0] + rng.normal(0, 0.2, n), np.sin(0.05 * x[:, 1]) + rng.normal(0, 0.2, n)], axis=1)
    return x, rng.normal(size=n) + offset, drift


def folds_of(sizes, ids, seed):
    """Shuffled fold ids: sizes[i] samples carry ids[i]."""
    return np.random.default_rng(seed).permutation(np.repeat(np.asarray(ids, dtype=np.int32), sizes))


def offset_of(variant, kw):
    # constrained variants: z about 1e4, so the dual weights in row N1 of W' are large and would show in a Gram
    # product that ran into them; simple kriging about its mean
    return kw.get("mean", 0.0) if variant == "sk" else 1.0e4


def run(variant, model, sizes, ids, seed):
    from gss.engine import KrigHandle
    var_, dim, kw, nd = VARIANTS[variant]
    g, og = _models()[model]
    fold = folds_of(sizes, ids, seed)
    x, z, drift = problem(fold.size, dim, seed + 1, nd, offset=offset_of(variant, kw))
    h = KrigHandle(g, var_, x, z, drift_data=drift, **kw)
    pred, var, st = h.cv_global_folds(fold)
    h.close()
    rp, rv, rs = FR.folds_refit(var_, og, x, z, fold, drift_data=drift, **kw)
    print("max |dpred| %.3e  max |dvar| %.3e" % (np.max(np.abs(pred - rp)), np.max(np.abs(var - rv))))
    assert not rs.any() and not st.any() and close(pred, rp) and close(var, rv)


# fold sizes on the tile edges and beyond, unequal, ids not compact: n = 150
EDGE_SIZES, EDGE_IDS = (1, 15, 16, 17, 33, 64, 4), (3, 7, 100, 101, 250, 1000, 5)
EDGES = [(v, MODEL_NAMES[i % 3]) for i, v in enumerate(sorted(VARIANTS))]


@pytest.mark.parametrize("variant,model", EDGES, ids=["%s-%s" % c for c in EDGES])
def test_folds_on_the_tile_edges_equal_refits(variant, model):
    run(variant, model, EDGE_SIZES, EDGE_IDS, 21)


# one fold of exactly S, one of S + 1 and small ones: both solve paths in one problem, n = 2 S + 1 + 13
BOUNDARY = [("sk", "matern32"), ("ok", "exponential"), ("uk2", "spherical")]


@pytest.mark.parametrize("variant,model", BOUNDARY, ids=["%s-%s" % c for c in BOUNDARY])
def test_folds_on_either_side_of_the_lds_limit_equal_refits(variant, model):
    run(variant, model, (S, S + 1, 6, 7), (40, 2, 9, 11), 22)


@pytest.mark.parametrize("variant", ["ok", "uk2", "edk"])
def test_singleton_folds_equal_leave_one_out_and_no_folds_is_leave_one_out(variant):
    from gss.engine import KrigHandle
    var_, dim, kw, nd = VARIANTS[variant]
    g, _ = _models()["spherical"]
    x, z, drift = problem(131, dim, 23, nd, offset=1.0e4)
    h = KrigHandle(g, var_, x, z, drift_data=drift, **kw)
    loo = h.cv_global()
    single = h.cv_global_folds(np.arange(131))
    none = h.cv_global_folds(None)
    h.close()
    assert not single[2].any()
    assert close(single[0], loo[0], 1e-12) and close(single[1], loo[1], 1e-12)
    for a, b in zip(none, loo):
        assert np.array_equal(a, b)


def test_folds_with_a_rotated_anisotropy_model():
    import gss
    from gss.engine import KrigHandle
    fold = folds_of((30, 17, 50, 33), (4, 0, 9, 2), 24)
    x, z, _ = problem(130, 2, 24)
    R, r = rot2(0.6), (40.0, 15.0)
    g = gss.ExponentialVariogram(gss.MetricBall(r, tuple(map(tuple, R))), nugget=0.05)
    h = KrigHandle(g, K.OK, x, z)
    pred, var, st = h.cv_global_folds(fold)
    h.close()
    rp, rv, _ = FR.folds_refit(K.OK, Variogram("exponential", radii=r, nugget=0.05), frame(x, R), z, fold)
    assert not st.any() and close(pred, rp) and close(var, rv)


def test_folds_wait_for_an_asynchronous_fit_stay_on_the_device_and_repeat_bit_for_bit():
    import torch
    from gss.engine import KrigHandle
    g, og = _models()["matern32"]
    fold = folds_of((70, 20, 110), (1, 5, 6), 25)
    x, z, _ = problem(200, 3, 25)
    h = KrigHandle(g, K.UK, x, z, degree=1, async_fit=True)
    pred, var, st = h.cv_global_folds(torch.as_tensor(fold, device="cuda"))
    again = h.cv_global_folds(fold)
    h.close()
    assert pred.is_cuda and var.is_cuda and st.is_cuda and st.dtype == torch.uint8
    rp, rv, _ = FR.folds_refit(K.UK, og, x, z, fold, degree=1)
    assert close(pred.cpu().numpy(), rp) and close(var.cpu().numpy(), rv) and not st.any().item()
    for a, b in zip((pred, var, st), again):                       # fixed-order sums: the same bits on every run
        assert np.array_equal(a.cpu().numpy(), b)


def test_a_remainder_that_cannot_determine_the_system_is_singular_fold_by_fold():
    from gss.engine import KrigHandle
    g, og = _models()["exponential"]
    x, z, _ = problem(60, 2, 26)
    # ordinary kriging, one fold of everything: nothing is left to estimate the mean from
    h = KrigHandle(g, K.OK, x, z)
    pred, var, st = h.cv_global_folds(np.full(60, 8))
    h.close()
    assert (st == 2).all() and np.isnan(pred).all() and np.isnan(var).all()
    # universal kriging, degree 1 in 2-D (nc = 3): fold 5 leaves 2 samples and is singular, folds 1 and 2 are predicted
    fold = np.full(60, 5)
    fold[[3, 40]] = (1, 2)
    h = KrigHandle(g, K.UK, x, z, degree=1)
    pred, var, st = h.cv_global_folds(fold)
    h.close()
    rp, rv, rs = FR.folds_refit(K.UK, og, x, z, fold, degree=1)
    ok = fold != 5
    assert np.array_equal(st, rs) and (st[~ok] == 2).all() and not st[ok].any()
    assert np.isnan(pred[~ok]).all() and np.isnan(var[~ok]).all() and close(pred[ok], rp[ok]) and close(var[ok], rv[ok])
    # simple kriging, one fold of everything: the empty remainder predicts the mean with variance C(0)
    h = KrigHandle(g, K.SK, x, z, mean=3.5)
    pred, var, st = h.cv_global_folds(np.zeros(60, dtype=np.int32))
    h.close()
    assert not st.any() and close(pred, np.full(60, 3.5)) and close(var, np.full(60, og.sill))


def test_refusals_of_the_call():
    import gss
    from gss import _lib
    from gss.engine import KrigHandle
    g = gss.ExponentialVariogram(range=30.0)
    x, z, _ = problem(40, 2, 27)
    fold = np.arange(40) % 4
    h = KrigHandle(g, K.OK, x, z)
    with pytest.raises(_lib.GSSError) as err:
        h.cv_global_folds(np.r_[-1, fold[1:]])
    assert err.value.code == _lib.ERR_INVALID and "negative" in str(err.value)
    assert not h.cv_global_folds(fold)[2].any()
    h.set_block_support((2.0, 2.0), 3)
    with pytest.raises(_lib.GSSError) as err:
        h.cv_global_folds(fold)
    assert err.value.code == _lib.ERR_INVALID and "point support" in str(err.value)
    h.close()
    hn = KrigHandle(g, K.OK, x, z, factor=False)
    with pytest.raises(_lib.GSSError) as err:
        hn.cv_global_folds(fold)
    hn.close()
    assert err.value.code == _lib.ERR_INVALID and "factor" in str(err.value)


def test_through_the_public_interface():
    import gss
    g, og = _models()["spherical"]
    rng = np.random.default_rng(28)
    x = rng.uniform(0, 100, (203, 2))
    z = rng.normal(size=203) + 5.0
    prob = gss.EstimationProblem(gss.georef({"z": z}, gss.PointSet(x)), gss.CartesianGrid(4, 4), "z")
    solver = gss.KrigingSolver(z=dict(variogram=g))
    res = gss.cross_validate(prob, solver, gss.KFoldValidation(5, rng=1))["z"]
    fold, nf = gss.KFoldValidation(5, rng=1).folds(x)
    rp, rv, rs = FR.folds_refit(K.OK, og, x, z, fold)
    want, fmse = CR.summary(z, rp, rv, rs, fold, nf)
    assert np.array_equal(res.fold, fold) and not res.status.any()
    assert close(res.pred, rp) and close(res.variance, rv)
    assert close(res.summary.cverror, want["cverror"]) and close(res.summary.fold_mse, fmse)
    assert close(gss.cverror(solver, prob, gss.KFoldValidation(5, rng=1))["z"], want["cverror"])
    res = gss.cross_validate(prob, solver, gss.BlockValidation(20.0))["z"]
    fold, nf = gss.BlockValidation(20.0).folds(x)
    rp, rv, rs = FR.folds_refit(K.OK, og, x, z, fold)
    assert close(res.pred, rp) and close(res.variance, rv) and res.summary.fold_mse.shape == (nf,)
    with pytest.raises(ValueError, match="global neighbourhood"):
        gss.cross_validate(prob, solver, gss.LeaveBallOut(5.0))


def test_ten_folds_at_1021_samples_equal_the_closed_form():
    from gss.engine import KrigHandle
    g, og = _models()["spherical"]
    x, z, _ = problem(1021, 2, 29)
    fold = np.random.default_rng(29).permutation(np.arange(1021) % 10)
    h = KrigHandle(g, K.OK, x, z)
    pred, var, st = h.cv_global_folds(fold)
    h.close()
    rp, rv = FR.folds_closed_form(K.OK, og, x, z, fold)
    assert not st.any() and close(pred, rp) and close(var, rv)
