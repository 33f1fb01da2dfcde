"""Cross-validation on the device against the brute-force reference tests/crossval_ref.py: leave-one-out off the factor
(gss_krig_cv_global) against n refits, the fold-excluding neighbour search (gss_krig_cv_knn) bit-exact against the
eligible lists on integer coordinates, its estimates against oracle.kriging on those lists, the error summary
(gss_cv_summary) against numpy.  Means and variances: the project's 1e-9 (1 + |v|)."""
import os
import sys

import numpy as np
import pytest

from oracle import kriging as K
from oracle.variogram import Variogram

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crossval_ref as CR
from rotated_frame import frame, rot2

pytestmark = pytest.mark.gpu

TOL = 1e-9


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


# ---- gss_krig_cv_global ---------------------------------------------------------------------------------------------
GLOBAL = [(n, v, MODEL_NAMES[(i + j) % 3]) for i, n in enumerate((15, 16, 17, 63, 64, 65, 130, 300))
          for j, v in enumerate(sorted(VARIANTS))]


@pytest.mark.parametrize("n,variant,model", GLOBAL, ids=["%d-%s-%s" % c for c in GLOBAL])
def test_leave_one_out_off_the_factor_equals_n_refits(n, variant, model):
    from gss.engine import KrigHandle
    var_, dim, kw, nd = VARIANTS[variant]
    g, og = _models()[model]
    x, z, drift = problem(n, dim, 7 * n + len(model), nd, offset=kw.get("mean", 0.0))
    h = KrigHandle(g, var_, x, z, drift_data=drift, **kw)
    pred, var, st = h.cv_global()
    h.close()
    rp, rv = CR.loo_refit(var_, og, x, z, drift_data=drift, **kw)
    print("max |dpred| %.3e  max |dvar| %.3e" % (np.max(np.abs(pred - rp)), np.max(np.abs(var - rv))))
    assert not st.any() and close(pred, rp) and close(var, rv)


def test_leave_one_out_with_a_rotated_anisotropy_model():
    import gss
    from gss.engine import KrigHandle
    x, z, _ = problem(130, 2, 11)
    R, r = rot2(0.6), (40.0, 15.0)
    g = gss.ExponentialVariogram(gss.MetricBall(r, tuple(map(tuple, R))), nugget=0.05)
    h = KrigHandle(g, K.OK, x, z)
    pred, var, st = h.cv_global()
    h.close()
    rp, rv = CR.loo_refit(K.OK, Variogram("exponential", radii=r, nugget=0.05), frame(x, R), z)
    assert not st.any() and close(pred, rp) and close(var, rv)


def test_leave_one_out_waits_for_an_asynchronous_fit_and_stays_on_the_device():
    import torch
    from gss.engine import KrigHandle
    g, og = _models()["matern32"]
    x, z, _ = problem(200, 3, 12)
    h = KrigHandle(g, K.UK, x, z, degree=1, async_fit=True)
    pred, var, st = h.cv_global(device=True)
    again = h.cv_global()
    h.close()
    assert pred.is_cuda and st.dtype == torch.uint8
    rp, rv = CR.loo_refit(K.UK, og, x, z, degree=1)
    assert close(pred.cpu().numpy(), rp) and close(var.cpu().numpy(), rv) and not st.any().item()
    for a, b in zip((pred, var, st), again):                       # a fixed-order sum: the same bits on every run
        assert np.array_equal(a.cpu().numpy(), b)


def test_leave_one_out_at_1021_samples_equals_the_closed_form():
    from gss.engine import KrigHandle
    g, og = _models()["spherical"]
    x, z, _ = problem(1021, 2, 13)
    h = KrigHandle(g, K.OK, x, z)
    pred, var, st = h.cv_global()
    h.close()
    rp, rv = CR.loo_closed_form(K.OK, og, x, z)
    assert not st.any() and close(pred, rp) and close(var, rv)


@pytest.mark.parametrize("variant", ["sk", "ok", "uk2"])
def test_the_dual_weight_row_of_the_factor_does_not_enter_the_sum(variant):
    """Row N1 of W' holds the dual weights.  With a large offset in z they are far from 0 (checked), so adding their
    squares to B_ii would move every variance by far more than the tolerance."""
    from gss.engine import KrigHandle
    var_, dim, kw, _ = VARIANTS[variant]
    g, og = _models()["exponential"]
    x, z, _ = problem(65, dim, 14, offset=1.0e4)
    kw = dict(kw, mean=0.0) if variant == "sk" else kw             # simple kriging about 0: the offset stays in wd
    h = KrigHandle(g, var_, x, z, **kw)
    pred, var, st = h.cv_global()
    h.close()
    rp, rv = CR.loo_refit(var_, og, x, z, **kw)
    lhs = K.fit(var_, og, x, z, **kw).lhs
    wd = np.linalg.solve(lhs, np.concatenate([z, np.zeros(lhs.shape[0] - 65)]))[:65]
    wrong = 1.0 / (1.0 / rv + wd ** 2)
    assert np.min(np.abs(wd)) > 0.0 and np.max(np.abs(wrong - rv) / (1.0 + rv)) > 1e-3
    assert not st.any() and close(pred, rp) and close(var, rv)


def test_a_gaussian_model_without_regularisation_reports_not_positive_definite():
    import gss
    from gss import _lib
    from gss.engine import KrigHandle
    x, z, _ = problem(300, 2, 15)
    h = KrigHandle(gss.GaussianVariogram(range=80.0, regularize=False), K.OK, x, z, async_fit=True)
    with pytest.raises(_lib.GSSError) as err:
        h.cv_global()
    h.close()
    assert err.value.code == _lib.ERR_NOT_POSDEF


def test_refusals_of_the_calls():
    import gss
    from gss import _lib
    from gss.engine import KrigHandle
    g = gss.ExponentialVariogram(range=30.0)
    x, z, _ = problem(40, 2, 16)
    h = KrigHandle(g, K.OK, x, z, factor=False)
    cases = [lambda: h.cv_global(), lambda: h.cv_knn(40), lambda: h.cv_knn(0),
             lambda: h.cv_knn(5, fold=np.r_[-1, np.zeros(39)])]
    for call in cases:
        with pytest.raises(_lib.GSSError) as err:
            call()
        assert err.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.GSSError) as err:
        h.cv_knn(5, distance=("haversine", 6371.0))
    assert err.value.code == _lib.ERR_UNSUPPORTED
    assert not h.cv_knn(39)[2].any()                                # works without a factor, up to n - 1 neighbours
    h.close()
    hb = KrigHandle(g, K.OK, x, z)
    hb.set_block_support((2.0, 2.0), 3)
    for call in (lambda: hb.cv_global(), lambda: hb.cv_knn(5)):
        with pytest.raises(_lib.GSSError) as err:
            call()
        assert err.value.code == _lib.ERR_INVALID and "point support" in str(err.value)
    hb.close()


# ---- gss_krig_cv_knn: neighbour lists -------------------------------------------------------------------------------
# integer coordinates on a coarse lattice: exact keys, many ties and duplicated coordinates.  folds: "loo", "kfold" (5
# shuffled folds), "block" (BlockValidation: whole index batches ineligible), "allbut3" (one fold holds all but 3 samples)
R2 = rot2(0.5)
SEARCH_CASES = [
    dict(dim=1, n=63, k=1, folds="loo", side=40),
    dict(dim=1, n=64, k=8, folds="kfold", distance="cityblock", side=40),
    dict(dim=1, n=65, k=63, folds="loo", distance="chebyshev", side=200),
    dict(dim=2, n=64, k=63, folds="loo", side=6),
    dict(dim=2, n=65, k=64, folds="kfold", side=6),
    dict(dim=2, n=4095, k=65, folds="block", distance="cityblock", side=50),
    dict(dim=2, n=4097, k=129, folds="kfold", distance="chebyshev", side=50),
    dict(dim=2, n=4097, k=65, folds="kfold", side=60, radii=(14.0, 6.0), rotation=R2),
    dict(dim=3, n=4097, k=64, folds="block", side=14, radius=4.0),
    dict(dim=3, n=4095, k=8, folds="loo", side=14, radii=(1.2, 1.0, 1.5)),
    dict(dim=3, n=4095, k=1, folds="kfold", distance="cityblock", side=12),
    dict(dim=3, n=63, k=8, folds="block", distance="chebyshev", side=5),
    dict(dim=3, n=4097, k=8, folds="allbut3", side=14, minneighbors=1),
    dict(dim=3, n=4097, k=8, folds="allbut3", side=14, minneighbors=4),
    dict(dim=2, n=4097, k=16, folds="loo", side=50, exclude_radius=5.0),
    dict(dim=2, n=4095, k=16, folds="kfold", distance="chebyshev", side=50, exclude_radius=3.0),
    dict(dim=3, n=262_200, k=8, folds="block", side=70, check=2000),
]


def _case_id(c):
    return "%dd-n%d-k%d-%s-%s" % (c["dim"], c["n"], c["k"], c["folds"], c.get("distance") or
                                  ("rot" if "rotation" in c else "radii" if "radii" in c else
                                   "ball" if "radius" in c else "ex" if "exclude_radius" in c else "euclidean"))


def search_problem(c):
    import gss
    rng = np.random.default_rng(c["n"] + 31 * c["k"] + c["dim"])
    x = rng.integers(0, c["side"], (c["n"], c["dim"])).astype(np.float64)
    if c["folds"] == "loo":
        fold = None
    elif c["folds"] == "kfold":
        fold = gss.KFoldValidation(5, rng=3).folds(x)[0]
    elif c["folds"] == "block":
        fold = gss.BlockValidation(c["side"] / (2.0 if c["dim"] == 3 else 3.0)).folds(x)[0]
    else:
        fold = np.zeros(c["n"], dtype=np.int32)
        fold[[5, 2000, 4090]] = [1, 2, 3]
    return x, fold


@pytest.mark.parametrize("c", SEARCH_CASES, ids=[_case_id(c) for c in SEARCH_CASES])
def test_fold_search_lists_are_bit_exact(c):
    import gss
    from gss.engine import KrigHandle
    x, fold = search_problem(c)
    n, k = c["n"], c["k"]
    kw = {q: c[q] for q in ("radius", "radii", "rotation", "distance", "exclude_radius") if q in c}
    nmin = c.get("minneighbors", 1)
    h = KrigHandle(gss.ExponentialVariogram(range=20.0, nugget=0.3), K.OK, x, np.arange(n) % 7.0, factor=False)
    pred, var, st, idx, cnt = h.cv_knn(k, fold=fold, minneighbors=nmin, return_idx=True, **kw)
    h.close()
    q = np.arange(n) if "check" not in c else np.sort(np.random.default_rng(1).choice(n, c["check"], replace=False))
    xs = x if "rotation" not in c else frame(x, c["rotation"])
    rkw = {a: b for a, b in kw.items() if a != "rotation"}
    ridx, rcnt = CR.eligible_lists(xs, k, fold, queries=q, **rkw)
    assert np.array_equal(cnt[q], rcnt) and np.array_equal(idx[q], ridx)
    assert np.array_equal(st[q] == 1, rcnt < nmin) and np.isnan(pred[st == 1]).all() and np.isnan(var[st == 1]).all()
    # the properties the case was built for
    f = np.arange(n) if fold is None else fold
    first = ridx[:, 0]
    has = first >= 0
    assert np.all(f[first[has]] != f[q][has])
    if c["folds"] == "allbut3":
        assert np.all(rcnt[f[q] == 0] == 3) and np.all(rcnt[f[q] != 0] == k)
        assert (st == 1).sum() == (n - 3 if nmin == 4 else 0)
    if c["folds"] == "kfold" and c["dim"] >= 2:
        same = (xs[first[has]] == xs[q][has]).all(axis=1)
        assert same.any() or "exclude_radius" in c                 # a duplicated coordinate in another fold: distance 0
        dup = [p for p in q[:400] if ((xs == xs[p]).all(axis=1) & (f == f[p])).sum() > 1]
        assert dup and all(not np.isin(np.flatnonzero((xs == xs[p]).all(axis=1) & (f == f[p])), idx[p]).any() for p in dup)
    if "radius" in c or "radii" in c:
        assert rcnt.min() < k <= rcnt.max()                        # the ball cuts some lists short
    if c["folds"] == "block" and c["n"] > 4000:
        assert np.bincount(f).max() > 64                           # folds larger than an index batch


def test_leave_ball_out_excludes_a_sample_exactly_on_the_radius_and_keeps_one_just_outside():
    import gss
    from gss.engine import KrigHandle
    g1 = np.arange(11.0)
    x = np.stack(np.meshgrid(g1, g1, indexing="ij"), axis=-1).reshape(-1, 2)          # 11 x 11 lattice
    c = 5 * 11 + 5                                                                   # the centre (5, 5)
    h = KrigHandle(gss.ExponentialVariogram(range=20.0, nugget=0.3), K.OK, x, np.arange(121.0) % 5, factor=False)
    idx, cnt = h.cv_knn(8, exclude_radius=5.0, return_idx=True)[3:]
    h.close()
    d2 = ((x - x[c]) ** 2).sum(axis=1)
    assert (d2 == 25).sum() == 12 and not np.isin(np.flatnonzero(d2 <= 25), idx[c]).any()   # (5,0), (3,4), ... left out
    assert cnt[c] == 8 and sorted(idx[c]) == list(np.flatnonzero(d2 == 26))                  # (1,5), (5,1), ... kept
    ridx, rcnt = CR.eligible_lists(x, 8, None, exclude_radius=5.0)
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt)


def test_a_tie_between_the_64th_and_the_65th_neighbour_across_the_pass_boundary():
    import gss
    from gss.engine import KrigHandle
    g1 = np.arange(21.0)
    x = np.stack(np.meshgrid(g1, g1, indexing="ij"), axis=-1).reshape(-1, 2)          # 21 x 21 lattice
    h = KrigHandle(gss.ExponentialVariogram(range=20.0, nugget=0.3), K.OK, x, np.arange(441.0) % 5, factor=False)
    idx, cnt = h.cv_knn(129, return_idx=True)[3:]
    h.close()
    ridx, rcnt = CR.eligible_lists(x, 129, None)
    c = 10 * 21 + 10
    key = ((x[ridx[c]] - x[c]) ** 2).sum(axis=1)
    assert key[63] == key[64] == 20.0 and ridx[c, 63] < ridx[c, 64]                   # ranks 61 .. 68 share the key 20
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt)


# ---- gss_krig_cv_knn: estimates -------------------------------------------------------------------------------------
# k on every side of the solver switches of the moving neighbourhood: <= 64 (MFMA tile kernel, 16 / 32 / 64 columns),
# 65 .. 256 (register tiles), 257 .. 768 (slab)
ESTIMATES = [("ok", "matern32", 500, 16, "kfold", 1), ("sk", "exponential", 300, 30, "loo", 1),
             ("uk3", "spherical", 400, 64, "block", 1), ("uk2", "exponential", 400, 100, "block", 3),
             ("edk", "matern32", 300, 24, "kfold", 1), ("ok", "spherical", 700, 300, "loo", 9)]


@pytest.mark.parametrize("variant,model,n,k,folds,step", ESTIMATES, ids=["%s-%s-n%d-k%d-%s" % e[:5] for e in ESTIMATES])
def test_fold_estimates_equal_the_oracle_on_the_same_lists(variant, model, n, k, folds, step):
    import gss
    from gss.engine import KrigHandle
    var_, dim, kw, nd = VARIANTS[variant]
    g, og = _models()[model]
    x, z, drift = problem(n, dim, n + k, nd, offset=kw.get("mean", 0.0))
    fold = {"loo": None, "kfold": gss.KFoldValidation(5, rng=2).folds(x)[0],
            "block": gss.BlockValidation(34.0).folds(x)[0]}[folds]
    h = KrigHandle(g, var_, x, z, drift_data=drift, factor=False, **kw)
    pred, var, st, idx, cnt = h.cv_knn(k, fold=fold, minneighbors=2, return_idx=True)
    h.close()
    q = np.arange(0, n, step)
    ridx, rcnt = CR.eligible_lists(x, k, fold, queries=q)
    assert np.array_equal(idx[q], ridx) and np.array_equal(cnt[q], rcnt)
    rp, rv, rs = CR.solve_on_lists(var_, og, x, z, ridx, rcnt, 2, drift_data=drift, queries=q, **kw)
    ok = rs == 0
    print("max |dpred| %.3e  max |dvar| %.3e" % (np.max(np.abs(pred[q][ok] - rp[ok])), np.max(np.abs(var[q][ok] - rv[ok]))))
    assert np.array_equal(st[q], rs) and ok.sum() > len(q) // 2
    assert close(pred[q][ok], rp[ok]) and close(var[q][ok], rv[ok])


# ---- consistency ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant", [(60, "ok"), (130, "uk2"), (65, "sk")])
def test_every_other_sample_as_neighbour_is_the_global_leave_one_out(n, variant):
    from gss.engine import KrigHandle
    var_, dim, kw, _ = VARIANTS[variant]
    g, _ = _models()["spherical"]
    x, z, _ = problem(n, dim, 21 + n, offset=kw.get("mean", 0.0))
    h = KrigHandle(g, var_, x, z, **kw)
    gp, gv, gs = h.cv_global()
    lp, lv, ls = h.cv_knn(n - 1)
    h.close()
    assert not gs.any() and not ls.any() and close(lp, gp) and close(lv, gv)


def test_cross_validation_leaves_the_predictions_of_the_handle_as_they_were():
    import gss
    from gss.engine import KrigHandle
    g, _ = _models()["matern32"]
    x, z, _ = problem(900, 3, 22)
    xdom = np.random.default_rng(23).uniform(0, 100, (700, 3))
    h = KrigHandle(g, K.OK, x, z)
    before = h.predict_knn(xdom, 24, return_idx=True) + h.predict_knn(xdom, 100, radius=40.0, return_idx=True)
    h.cv_global()
    h.cv_knn(24, fold=gss.KFoldValidation(5, rng=0).folds(x)[0])
    h.cv_knn(100, exclude_radius=4.0, radius=40.0)
    after = h.predict_knn(xdom, 24, return_idx=True) + h.predict_knn(xdom, 100, radius=40.0, return_idx=True)
    h.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)


# ---- gss_cv_summary -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nfolds", [(1, 0), (255, 3), (4097, 0), (100_003, 7), (1_500_000, 12)])
def test_summary_equals_numpy_and_repeats_bit_for_bit(n, nfolds):
    import torch
    from gss.engine import HipEngine
    rng = np.random.default_rng(n)
    # errors with a mean of half their spread: a relative bar on `me` needs a sum that does not cancel
    z = rng.normal(size=n) * 3.0
    pred = z - 0.5 + rng.normal(size=n)
    var = rng.uniform(0.1, 2.0, n)
    st = (rng.uniform(size=n) < 0.05).astype(np.uint8) * rng.integers(1, 3, n).astype(np.uint8)
    var[rng.uniform(size=n) < 0.03] = 0.0                          # excluded from the standardised means only
    pred[st != 0] = np.nan
    fold = rng.integers(0, max(nfolds - 1, 1), n).astype(np.int32) if nfolds else None      # the last fold stays empty
    want, wf = CR.summary(z, pred, var, st, fold, nfolds)
    host = HipEngine.cv_summary(z, pred, var, st, fold, nfolds)
    dev = lambda: HipEngine.cv_summary(*[None if a is None else torch.as_tensor(a, device="cuda")   # noqa: E731
                                         for a in (z, pred, var, st, fold)], nfolds)
    d1, d2 = dev(), dev()
    for got, gf in (host, d1, d2):
        for name, w in want.items():
            assert (np.isnan(w) and np.isnan(got[name])) or abs(got[name] - w) <= 1e-12 * abs(w), (name, got[name], w)
        if nfolds:
            gf = gf.cpu().numpy() if hasattr(gf, "is_cuda") else gf
            assert np.isnan(gf[-1]) and np.allclose(gf[:-1], wf[:-1], rtol=1e-12, atol=0)
        else:
            assert gf is None
    for name in want:                                               # fixed-order sums: the same bits on every run
        assert np.array_equal(d1[0][name], d2[0][name], equal_nan=True), name
        assert np.array_equal(d1[0][name], host[0][name], equal_nan=True), name
    if nfolds:
        assert np.array_equal(d1[1].cpu().numpy(), d2[1].cpu().numpy(), equal_nan=True)
        assert np.array_equal(d1[1].cpu().numpy(), host[1], equal_nan=True)


def test_front_end_on_the_device_engine():
    import gss
    g, og = _models()["exponential"]
    x, z, _ = problem(400, 2, 24)
    data = gss.georef({"z": z}, x)
    res = gss.cross_validate(data, gss.KrigingSolver(z=dict(variogram=g)))["z"]
    rp, rv = CR.loo_closed_form(K.OK, og, x, z)
    assert close(res.pred, rp) and close(res.variance, rv)
    assert res.summary.cverror == pytest.approx(np.mean((z - rp) ** 2), rel=1e-9)
    solver = gss.KrigingSolver(z=dict(variogram=g, maxneighbors=12, neighborhood=gss.MetricBall(30.0)))
    method = gss.BlockValidation(25.0)
    res = gss.cross_validate(data, solver, method)["z"]
    fold, nf = method.folds(x)
    idx, cnt = CR.eligible_lists(x, 12, fold, radius=30.0)
    rp, rv, rs = CR.solve_on_lists(K.OK, og, x, z, idx, cnt)
    ok = rs == 0
    assert np.array_equal(res.status, rs) and close(res.pred[ok], rp[ok]) and close(res.variance[ok], rv[ok])
    want, _ = CR.summary(z, rp, rv, rs, fold, nf)
    assert res.summary.cverror == pytest.approx(want["cverror"], rel=1e-9)
    assert gss.cverror(solver, gss.EstimationProblem(data, gss.PointSet(x[:1]), "z"), method)["z"] == res.summary.cverror


def test_the_example_runs_and_prefers_the_model_the_samples_were_drawn_from(capsys):
    import runpy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = runpy.run_path(os.path.join(root, "examples", "crossvalidation.py"))["out"]
    assert out["loo"]["simulated_from"].mse < out["loo"]["short_range"].mse
    assert out["loo"]["fitted"].mse != out["loo"]["short_range"].mse
    for method in ("10 folds", "blocks of 20", "ball of 5"):
        assert out["cverror"]["simulated_from"][method] < out["cverror"]["short_range"][method]
    assert "leave-one-out" in capsys.readouterr().out
