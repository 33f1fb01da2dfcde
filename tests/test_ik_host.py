"""Indicator kriging without a device: the numpy restatement tests/ik_ref.py on hand-worked cases, and the host logic of
gss.IndicatorKrigingSolver / gss.postik (argument checks, global proportions)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gss
import ik_ref


def test_the_names_are_exported():
    assert gss.IndicatorKrigingSolver is not None and callable(gss.postik)
    from gss import _lib
    for name in ("gss_ik_predict_knn", "gss_ik_order_relations", "gss_ik_post"):
        assert name in _lib.SIGNATURES


def test_one_neighbour():
    g = gss.ExponentialVariogram(range=10.0)
    x, z = np.array([[0.0, 0.0], [50.0, 0.0]]), np.array([1.0, 3.0])
    x0 = np.array([[4.0, 0.0]])
    # ordinary: the one weight is 1 -> the neighbour's indicators
    r = ik_ref.predict(x, z, x0, [0.5, 1.0, 2.0], [g], 1)
    assert np.array_equal(r["raw"][0], [0.0, 1.0, 1.0]) and r["idx"][0, 0] == 0
    # simple about F*: lambda = C(4) / C(0) = exp(-1.2)
    fs = np.array([0.2, 0.5, 0.9])
    r = ik_ref.predict(x, z, x0, [0.5, 1.0, 2.0], [g], 1, fstar=fs)
    lam = math.exp(-1.2)
    assert np.allclose(r["raw"][0], fs + lam * (np.array([0.0, 1.0, 1.0]) - fs), rtol=0, atol=1e-15)


def test_two_neighbours_in_closed_form():
    g = gss.ExponentialVariogram(range=10.0)
    x, z = np.array([[0.0], [10.0]]), np.array([1.0, 3.0])
    x0 = np.array([[2.0]])
    a, b, c = math.exp(-0.6), math.exp(-2.4), math.exp(-3.0)     # C(2), C(8), C(10)
    # ordinary kriging of two samples: lambda_1 = 1/2 + (a - b) / (2 (1 - c))
    l1 = 0.5 + (a - b) / (2.0 * (1.0 - c))
    r = ik_ref.predict(x, z, x0, [2.0], [g], 2)
    assert abs(r["raw"][0, 0] - l1) < 1e-15
    # simple: lambda = [[1, c], [c, 1]]^-1 [a, b]
    det = 1.0 - c * c
    s1, s2 = (a - c * b) / det, (b - c * a) / det
    r = ik_ref.predict(x, z, x0, [2.0], [g], 2, fstar=np.array([0.4]))
    assert abs(r["raw"][0, 0] - (0.4 + s1 * 0.6 + s2 * (-0.4))) < 1e-15
    ld = ik_ref.predict(x, z, x0, [2.0], [g], 2, fstar=np.array([0.4]), longdouble=True)
    assert abs(float(ld["raw_ld"][0, 0]) - r["raw"][0, 0]) < 1e-15


def test_a_point_on_a_sample_returns_its_indicators():
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 10, (12, 2))
    z = rng.uniform(0, 4, 12)
    g = gss.SphericalVariogram(range=6.0)                        # no nugget
    r = ik_ref.predict(x, z, x[3:4], [1.0, 2.0, 3.0], [g], 6)
    assert np.allclose(r["raw"][0], (z[3] <= np.array([1.0, 2.0, 3.0])).astype(float), rtol=0, atol=1e-13)
    assert np.all(np.diff(r["ccdf"][0]) >= 0.0) and r["ccdf"][0].min() >= 0.0 and r["ccdf"][0].max() <= 1.0


def test_sample_on_a_cutoff_counts_as_below():
    g = gss.ExponentialVariogram(range=10.0)
    r = ik_ref.predict(np.array([[0.0]]), np.array([2.0]), np.array([[1.0]]), [2.0, 2.5], [g], 1)
    assert np.array_equal(r["raw"][0], [1.0, 1.0])


def test_order_relations_by_hand():
    mono = np.array([[0.0, 0.25, 0.25, 0.9, 1.0], [0.1, 0.1, 0.1, 0.1, 0.1]])
    assert np.array_equal(ik_ref.order_relations(mono), mono)
    assert np.array_equal(ik_ref.order_relations(np.array([[0.3, 0.2, 1.1]])), [[0.25, 0.25, 1.0]])
    assert np.array_equal(ik_ref.order_relations(np.array([[-0.2, 0.5, 0.4, 0.45]])), [[0.0, 0.45, 0.45, 0.475]])
    assert np.isnan(ik_ref.order_relations(np.array([[0.2, np.nan, 0.4]]))).all()


def test_post_processing_against_integrals_by_hand():
    # cutoffs 1, 3 on [0, 7]; F = (0.2, 0.6); linear lower tail, upper tail with exponent 2
    F = np.array([[0.2, 0.6]])
    p = ik_ref.post(F, [1.0, 3.0], 0.0, 7.0, 1.0, 2.0, thresholds=(0.5, 2.0, 5.0), probs=(0.1, 0.4, 0.9))
    # classes: [0,1] uniform p=.2 (mean .5, E z^2 = 1/3); (1,3] uniform p=.4 (mean 2, E z^2 = 13/3);
    # upper: s = 7 - z on [0, 4], P(s <= t) = (t/4)^2 -> E s = 4 * 2/3, E s^2 = 16 * 2/4; p = .4
    es, es2 = 8.0 / 3.0, 8.0
    m1 = 0.2 * 0.5 + 0.4 * 2.0 + 0.4 * (7.0 - es)
    m2 = 0.2 / 3.0 + 0.4 * 13.0 / 3.0 + 0.4 * (49.0 - 14.0 * es + es2)
    assert abs(p["etype"][0] - m1) < 1e-14 and abs(p["cvar"][0] - (m2 - m1 * m1)) < 1e-13
    # F(0.5) = .1, F(2) = .4, F(5) = 1 - .4 (2/4)^2 = .9
    assert np.allclose(p["pabove"][0], [0.9, 0.6, 0.1], rtol=0, atol=1e-15)
    # quantiles: .1 -> 0.5; .4 -> 2; .9 -> 7 - 4 sqrt(.1/.4) = 5
    assert np.allclose(p["quant"][0], [0.5, 2.0, 5.0], rtol=0, atol=1e-14)
    # a flat segment returns its left end; a NaN row gives NaNs
    q = ik_ref.post(np.array([[0.3, 0.3], [np.nan, 0.5]]), [1.0, 3.0], 0.0, 7.0, probs=(0.3,))
    assert q["quant"][0, 0] == 1.0 and np.isnan(q["quant"][1, 0]) and np.isnan(q["etype"][1])


def test_global_proportions_and_solver_checks():
    from gss.indicator import global_proportions
    z = np.array([1.0, 2.0, np.nan, 4.0])
    assert np.allclose(global_proportions(z, [1.0, 3.0]), [1 / 3, 2 / 3])
    assert np.allclose(global_proportions(z, [1.0, 3.0], [3.0, 1.0, 1.0, np.nan]), [0.75, 1.0])
    grid = gss.CartesianGrid((4, 4))
    data = gss.georef({"z": z}, np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]))
    prob = gss.EstimationProblem(data, grid, "z")
    g = gss.SphericalVariogram(range=3.0)
    bad = [dict(variogram=g), dict(cutoffs=[2.0, 1.0], variogram=g), dict(cutoffs=[1.0, 1.0], variogram=g),
           dict(cutoffs=np.arange(17.0), variogram=g), dict(cutoffs=[1.0, 2.0], variograms=[g]),
           dict(cutoffs=[1.0], variogram=g, variograms=[g]), dict(cutoffs=[1.0], variogram=g, mean=0.5),
           dict(cutoffs=[1.0], variogram=g, maxneighbors=65), dict(cutoffs=[1.0], variogram=gss.PowerVariogram()),
           dict(cutoffs=[1.0], variogram=g, mean="global", weights=[1.0, 2.0])]
    for kw in bad:
        with pytest.raises((ValueError, TypeError)):
            gss.IndicatorKrigingSolver(("z", kw)).preprocess(prob)
    pre = gss.IndicatorKrigingSolver(("z", dict(cutoffs=[1.0, 3.0], variogram=g, mean="global"))).preprocess(prob)
    assert np.allclose(pre["z"]["fstar"], [1 / 3, 2 / 3]) and pre["z"]["k"] == 3 and pre["z"]["x"].shape == (3, 2)
    with pytest.raises(ValueError):
        gss.IndicatorKrigingSolver(("z", dict(cutoff=[1.0])))


def _stub_engine():
    """tests/oracle_engine.py's stand-in (Krig with predict_global_batch) with the three indicator calls restated by
    ik_ref: the twin's host logic runs without a device."""
    from oracle_engine import OracleEngine

    class IkStub(OracleEngine):
        calls = []

        @staticmethod
        def ik_predict_knn(xdata, z, xdom, cutoffs, variograms, k, minneighbors=1, fstar=None, radius=None, radii=None,
                           distance=None, rotation=None, return_raw=False, return_idx=False):
            models = list(variograms) if isinstance(variograms, (list, tuple)) else [variograms]
            IkStub.calls.append(("knn", len(models), k))
            r = ik_ref.predict(xdata, z, xdom, cutoffs, models, k, minneighbors, fstar, radius, radii, distance)
            return r["ccdf"], r["status"]

        @staticmethod
        def ik_order_relations(ccdf):
            IkStub.calls.append(("order", ccdf.shape))
            out = ik_ref.order_relations(ccdf)
            changed = (out != ccdf) & ~np.isnan(out)
            ccdf[...] = out
            return ccdf, int(changed.sum()), 0.0

        @staticmethod
        def ik_post(ccdf, cutoffs, zmin, zmax, tail_power=(1.0, 1.0), thresholds=(), probs=(), moments=True):
            return ik_ref.post(ccdf, cutoffs, zmin, zmax, tail_power[0], tail_power[1], thresholds, probs)

    IkStub.calls = []
    return IkStub


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("simple", [False, True])
def test_solve_and_postik_through_a_stub_engine(full, simple):
    rng = np.random.default_rng(5)
    n = 30
    x = rng.uniform(0.0, 20.0, (n, 2))
    z = np.exp(rng.normal(size=n))
    z[4] = np.nan                                               # a missing value is dropped with its weight
    w = rng.uniform(0.5, 2.0, n)
    ok = ~np.isnan(z)
    cut = np.array([0.6, 1.0, 2.0])
    models = [gss.ExponentialVariogram(range=8.0, nugget=0.1), gss.SphericalVariogram(range=10.0, nugget=0.05),
              gss.ExponentialVariogram(range=6.0, nugget=0.2)]
    vkw = dict(variograms=models) if full else dict(variogram=models[0])
    mkw = dict(mean="global", weights=w) if simple else {}
    fstar = np.array([np.sum(w[ok] * (z[ok] <= c)) / np.sum(w[ok]) for c in cut]) if simple else None
    grid = gss.CartesianGrid((5, 4), (0.0, 0.0), (4.0, 5.0))
    prob = gss.EstimationProblem(gss.georef({"z": z}, x), grid, "z")
    eng = _stub_engine()
    used = models if full else models[:1]
    # moving neighbourhood: one engine call, the columns in cutoff order, the cutoffs handed over to postik
    sol = gss.solve(prob, gss.IndicatorKrigingSolver(("z", dict(cutoffs=cut, maxneighbors=8, **vkw, **mkw)), engine=eng))
    assert eng.calls == [("knn", len(used), 8)]
    r = ik_ref.predict(x[ok], z[ok], grid.centroids(), cut, used, 8, fstar=fstar)
    assert sol.names() == ["z_ccdf_0", "z_ccdf_1", "z_ccdf_2"]
    for i in range(3):
        assert np.array_equal(sol[f"z_ccdf_{i}"], r["ccdf"][:, i])
    assert np.array_equal(sol.cutoffs["z"], cut)
    post = gss.postik(sol, "z", zmin=0.0, zmax=20.0, tail_power=(1.0, 2.0), thresholds=(1.0,), probs=(0.5, 0.9), engine=eng)
    q = ik_ref.post(r["ccdf"], cut, 0.0, 20.0, 1.0, 2.0, (1.0,), (0.5, 0.9))
    assert post.names() == ["z_etype", "z_cvar", "z_pabove_0", "z_q_0", "z_q_1"]
    assert np.array_equal(post["z_etype"], q["etype"]) and np.array_equal(post["z_cvar"], q["cvar"])
    assert np.array_equal(post["z_pabove_0"], q["pabove"][:, 0]) and np.array_equal(post["z_q_1"], q["quant"][:, 1])
    # global neighbourhood: composed from the kriging handle (K residual or indicator columns, F* added back, then the
    # correction) -- the same system as the moving route with every sample a neighbour
    eng = _stub_engine()
    glob = gss.solve(prob, gss.IndicatorKrigingSolver(("z", dict(cutoffs=cut, maxneighbors=None, **vkw, **mkw)), engine=eng))
    assert eng.calls == [("order", (20, 3))]
    rg = ik_ref.predict(x[ok], z[ok], grid.centroids(), cut, used, int(ok.sum()), fstar=fstar)
    for i in range(3):
        assert np.max(np.abs(glob[f"z_ccdf_{i}"] - rg["ccdf"][:, i])) < 1e-12
    d = ik_ref.predict_global(x[ok], z[ok], grid.centroids(), cut, used, fstar=fstar)
    assert np.max(np.abs(ik_ref.order_relations(d["raw"]) - rg["ccdf"])) < 1e-12


def test_postik_checks_its_arguments_before_the_device():
    sol = gss.georef({"z_ccdf_0": np.array([0.2]), "z_ccdf_1": np.array([0.7])}, np.array([[0.0, 0.0]]))
    with pytest.raises(ValueError, match="cutoffs"):
        gss.postik(sol, "z", zmin=0.0, zmax=9.0)
    for kw in (dict(zmin=1.0), dict(zmax=2.0), dict(tail_power=(0.0, 1.0)), dict(probs=(1.0,)), dict(thresholds=(10.0,)),
               dict(thresholds=np.zeros(17))):
        a = dict(zmin=0.0, zmax=9.0)
        a.update(kw)
        with pytest.raises(ValueError):
            gss.postik(sol, "z", cutoffs=[1.0, 2.0], **a)
    with pytest.raises(KeyError):
        gss.postik(sol, "z", zmin=0.0, zmax=9.0, cutoffs=[1.0, 2.0, 3.0])


def test_in_normal_scores_names_the_indicator_route():
    est = gss.KrigingSolver(z=dict(variogram=gss.GaussianVariogram(range=5.0)))
    with pytest.raises(TypeError, match="IndicatorKrigingSolver"):
        gss.InNormalScores(est, z=None)
