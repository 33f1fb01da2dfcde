"""The parts of the variography feature that need no device: argument checks of gss_variogram_empirical and the whole
of gss_variogram_fit (host code of the library) against the restatement in tests/variography_ref.py."""
import ctypes as C

import numpy as np
import pytest

import variography_ref as vref
from gss import _lib
from gss.engine import HipEngine

KINDS = ("gaussian", "exponential", "spherical", "matern", "cubic", "pentaspherical", "sinehole")
H = np.arange(1.0, 21.0) * 5.0          # 20 lags
COUNT = (1000 + 37 * np.arange(20)).astype(np.int64)


def _empirical_code(n=100, dim=2, nz=1, nlags=10, maxlag=10.0, direction=None, dtol=np.inf, cos_atol=0.0, estimator=0,
                    x=C.c_void_p(8), z=C.c_void_p(8)):
    lib = _lib.load()
    cnt, ls, zs, nd = np.zeros(256, np.int64), np.zeros(256), np.zeros(8 * 256), np.zeros(1, np.int64)
    u = None if direction is None else np.ascontiguousarray(direction, dtype=np.float64)
    return lib.gss_variogram_empirical(x, n, dim, z, nz, nlags, float(maxlag), _lib.ptr(u), float(dtol), float(cos_atol),
                                       estimator, _lib.ptr(cnt), _lib.ptr(ls), _lib.ptr(zs), _lib.ptr(nd), 0, None)


def test_empirical_argument_checks_need_no_device():
    """None of these reaches the device: the coordinate pointer is not even readable."""
    for kw, word in [(dict(nlags=0), "nlags"), (dict(nlags=257), "nlags"), (dict(n=1), "samples"), (dict(nz=9), "nz"),
                     (dict(nz=0), "nz"), (dict(dim=4), "dim"), (dict(maxlag=0.0), "maxlag"),
                     (dict(maxlag=np.inf), "maxlag"), (dict(estimator=2), "estimator"),
                     (dict(direction=(1.0, 1.0)), "unit vector"), (dict(direction=(0.6, 0.8 + 1e-9)), "unit vector"),
                     (dict(direction=(1.0, 0.0), dtol=-1.0), "dtol"), (dict(direction=(1.0, 0.0), cos_atol=1.5), "cos_atol"),
                     (dict(x=None), "NULL")]:
        assert _empirical_code(**kw) == _lib.ERR_INVALID, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())


def test_non_euclidean_distance_is_unsupported():
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_empirical(np.zeros((4, 2)), np.zeros((1, 4)), 5, 1.0, distance="chebyshev")
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_fit_argument_checks():
    g = vref.model("spherical", H, 0.1, 1.0, 40.0)
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_fit(H, g, COUNT, ["power"])
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_fit(H, g, COUNT, ["gaussian", "power"])
    assert e.value.code == _lib.ERR_UNSUPPORTED
    for kw in (dict(weighting=3), dict(max_nugget_frac=1.5), dict(max_nugget_frac=-0.1)):
        with pytest.raises(_lib.GSSError) as e:
            HipEngine.variogram_fit(H, g, COUNT, ["gaussian"], **kw)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_fit(H, g, COUNT, ["matern"], nu=80.0)
    assert e.value.code == _lib.ERR_INVALID
    c1 = np.zeros(20, np.int64)
    c1[3] = 5
    with pytest.raises(_lib.GSSError) as e:                    # one usable bin cannot carry two parameters and a range
        HipEngine.variogram_fit(H, g, c1, ["gaussian"])
    assert e.value.code == _lib.ERR_INVALID and "two bins" in str(e.value)
    lib = _lib.load()
    best, obj, kinds = _lib.Variogram(), np.zeros(1), np.zeros(1, np.int32)
    assert lib.gss_variogram_fit(_lib.ptr(H), _lib.ptr(g), _lib.ptr(COUNT), 0, _lib.ptr(kinds), 1, 1.0, 0, 1.0,
                                 C.byref(best), _lib.ptr(obj)) == _lib.ERR_INVALID
    assert "nlags" in _lib.last_error()


@pytest.mark.parametrize("weighting", ["count", "count/h2", "uniform"])
@pytest.mark.parametrize("kind", KINDS)
def test_fit_recovers_exact_models(kind, weighting):
    """gamma_k = the model at 20 lags from known (nugget, sill, range): parameters to 1e-6 relative, objective
    <= 1e-12 sum w gamma^2.  Both bars are derived: a golden-section search cannot place a smooth minimum better than
    about sqrt(2^-53) = 1.5e-8 relative, and the objective, quadratic about its minimum, is then of the order
    1e-16 sum w gamma^2 times a curvature constant of the model; the bars leave two and four decades.
    Achieved over the 21 cases (x86-64 host): largest relative parameter error 1.06e-09 (pentaspherical, count
    weights), largest objective 2.1e-20 sum w gamma^2 (sine hole, count / h^2)."""
    nugget, sill, rng, nu = 0.15, 1.3, 42.0, 1.7
    g = vref.model(kind, H, nugget, sill, rng, nu)
    w = vref.fit_weights(H, COUNT, weighting)
    k, s, n0, r, order, obj = HipEngine.variogram_fit(H, g, COUNT, [kind], nu=nu,
                                                      weighting={"count": 0, "count/h2": 1, "uniform": 2}[weighting])
    rel = max(abs(s - sill) / sill, abs(n0 - nugget) / nugget, abs(r - rng) / rng)
    print("%s/%s: relative parameter error %.2e, objective / sum w gamma^2 = %.2e" % (kind, weighting, rel,
                                                                                   obj[0] / np.sum(w * g * g)))
    assert k == kind and (order == nu if kind == "matern" else True)
    assert rel <= 1e-6
    assert obj[0] <= 1e-12 * np.sum(w * g * g)


@pytest.mark.parametrize("frac", [1.0, 0.05])
@pytest.mark.parametrize("kind", KINDS)
def test_fit_is_optimal_on_noisy_ordinates(kind, frac):
    """The library's objective does not exceed the minimum over 2 000 log-spaced ranges with the same closed-form
    inner solve restated in variography_ref (relative slack 1e-9)."""
    rng = np.random.default_rng(11)
    g = vref.model(kind, H, 0.2, 1.0, 35.0, 1.3) * (1.0 + 0.08 * rng.normal(size=H.size))
    w = vref.fit_weights(H, COUNT, "count")
    k, s, n0, r, order, obj = HipEngine.variogram_fit(H, g, COUNT, [kind], nu=1.3, max_nugget_frac=frac)
    ref = vref.grid_objective(kind, H, g, w, nu=1.3, frac=frac)
    assert obj[0] <= ref * (1.0 + 1e-9)
    assert 0.0 <= n0 <= frac * s * (1 + 1e-15) and H.min() / 4 <= r <= 4 * H.max()
    # and what it reports is the objective of what it returns
    mine = np.sum(w * (vref.model(kind, H, n0, s, r, 1.3) - g) ** 2)
    assert abs(mine - obj[0]) <= 1e-9 * obj[0]


@pytest.mark.parametrize("kind", ["gaussian", "exponential", "spherical"])
def test_fit_selects_the_generating_kind(kind):
    g = vref.model(kind, H, 0.1, 2.0, 55.0)
    k, s, n0, r, order, obj = HipEngine.variogram_fit(H, g, COUNT, ["gaussian", "exponential", "spherical"])
    assert k == kind and int(np.argmin(obj)) == ["gaussian", "exponential", "spherical"].index(kind)
    assert abs(r - 55.0) <= 1e-6 * 55.0


def test_active_bounds():
    """A model with a negative nugget (unconstrained optimum outside the cone) fits to nugget == 0 exactly, and
    max_nugget_frac caps the nugget at that share of the sill."""
    g = vref.model("exponential", H, -0.2, 1.0, 60.0)
    k, s, n0, r, order, obj = HipEngine.variogram_fit(H, g, COUNT, ["exponential"])
    assert n0 == 0.0 and s > 0 and obj[0] > 0
    g = vref.model("spherical", H, 0.6, 1.0, 50.0)
    k, s, n0, r, order, obj = HipEngine.variogram_fit(H, g, COUNT, ["spherical"], max_nugget_frac=0.25)
    assert abs(n0 - 0.25 * s) <= 1e-12 * s and obj[0] > 0
    free = HipEngine.variogram_fit(H, g, COUNT, ["spherical"])
    assert abs(free[2] - 0.6) <= 1e-6 and free[5][0] < obj[0]
    k, s, n0, r, order, obj = HipEngine.variogram_fit(H, g, COUNT, ["spherical"], max_nugget_frac=0.0)
    assert n0 == 0.0


def test_empty_bins_are_ignored_and_nan_marks_unfitted_kinds():
    g = vref.model("gaussian", H, 0.1, 1.0, 40.0)
    c, gg, hh = COUNT.copy(), g.copy(), H.copy()
    c[[2, 9]] = 0
    gg[[2, 9]] = np.nan
    hh[[2, 9]] = np.nan
    k, s, n0, r, order, obj = HipEngine.variogram_fit(hh, gg, c, ["gaussian"])
    assert abs(r - 40.0) <= 1e-6 * 40.0
    with pytest.raises(_lib.GSSError):                         # negative ordinates: no positive sill fits
        HipEngine.variogram_fit(H, -g, COUNT, ["gaussian"])


def test_front_end_fit_maps_the_gaussian_nugget_rule():
    """fit() returns a model whose EVALUATED nugget (variograms.py: nugget + 1e-6 for a regularised Gaussian) is the
    fitted one."""
    import gss
    from gss.variography import EmpiricalVariogramResult, fit
    for nugget in (0.15, 0.0):
        g = EmpiricalVariogramResult(H, vref.model("gaussian", H, nugget, 1.3, 42.0), COUNT, 0, 100.0)
        m = fit(gss.GaussianVariogram, g)
        assert m.kind == "gaussian" and abs(m.effective_nugget - nugget) <= 2e-7 and abs(m.range - 42.0) < 1e-4
        assert m.regularize == (nugget > 0)
    m, obj = fit(["spherical", gss.ExponentialVariogram], EmpiricalVariogramResult(
        H, vref.model("spherical", H, 0.1, 1.0, 40.0), COUNT, 0, 100.0), weighting="uniform", return_objectives=True)
    assert m.kind == "spherical" and set(obj) == {"spherical", "exponential"}
    with pytest.raises(_lib.GSSError):
        fit(gss.PowerVariogram, g)


def test_twin_refuses_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    import gss
    data = gss.georef({"z": np.arange(10.0)}, np.arange(10.0)[:, None])
    with pytest.raises(_lib.GSSError) as e:
        gss.EmpiricalVariogram(data, "z")
    assert e.value.code == _lib.ERR_NO_DEVICE
