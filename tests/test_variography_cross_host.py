"""The parts of the cross-variogram feature that need no device: argument checks of gss_variogram_cross and the whole of
gss_variogram_fit_lmc (host code of the library) against the restatement in tests/variography_cross_ref.py."""
import ctypes as C

import numpy as np
import pytest

import variography_cross_ref as cref
import variography_ref as vref
from gss import _lib
from gss.engine import HipEngine

KINDS = ("gaussian", "exponential", "spherical", "matern", "cubic", "pentaspherical", "sinehole")
H = np.arange(1.0, 21.0) * 5.0          # 20 lags
COUNT = (1000 + 37 * np.arange(20)).astype(np.int64)
WCODE = {"count": 0, "count/h2": 1, "uniform": 2}


def _cross_code(n=100, dim=2, nz=2, nlags=10, maxlag=10.0, direction=None, dtol=np.inf, cos_atol=0.0,
                x=C.c_void_p(8), z=C.c_void_p(8), mem=0):
    lib = _lib.load()
    cnt, ls, cs, nd = np.zeros(256, np.int64), np.zeros(256), np.zeros(36 * 256), np.zeros(1, np.int64)
    u = None if direction is None else np.ascontiguousarray(direction, dtype=np.float64)
    return lib.gss_variogram_cross(x, n, dim, z, nz, nlags, float(maxlag), _lib.ptr(u), float(dtol), float(cos_atol),
                                   _lib.ptr(cnt), _lib.ptr(ls), _lib.ptr(cs), _lib.ptr(nd), mem, None)


def test_cross_argument_checks_need_no_device():
    """None of these reaches the device: the coordinate pointer is not even readable."""
    for kw, word in [(dict(nlags=0), "nlags"), (dict(nlags=257), "nlags"), (dict(n=1), "samples"), (dict(nz=9), "nz"),
                     (dict(nz=0), "nz"), (dict(dim=4), "dim"), (dict(dim=0), "dim"), (dict(maxlag=0.0), "maxlag"),
                     (dict(maxlag=np.inf), "maxlag"), (dict(mem=7), "mem"),
                     (dict(direction=(1.0, 1.0)), "unit vector"), (dict(direction=(0.6, 0.8 + 1e-9)), "unit vector"),
                     (dict(direction=(1.0, 0.0), dtol=-1.0), "dtol"), (dict(direction=(1.0, 0.0), cos_atol=1.5), "cos_atol"),
                     (dict(x=None), "NULL"), (dict(z=None), "NULL")]:
        assert _cross_code(**kw) == _lib.ERR_INVALID, kw
        assert word in _lib.last_error() and "gss_variogram_cross" in _lib.last_error(), (kw, _lib.last_error())


def _gamma(kind, B0, B1, rng, nu):
    f = vref.shape(kind, H / rng, nu)
    return B0[None] + B1[None] * f[:, None, None]


def _psd(nz, seed, scale):
    a = np.random.default_rng(seed).normal(size=(nz, nz + 2))
    return scale * (a @ a.T) / (nz + 2)


@pytest.mark.parametrize("weighting", ["count", "count/h2", "uniform"])
@pytest.mark.parametrize("nz", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_lmc_recovers_exact_models(kind, nz, weighting):
    """Gamma_k = B0 + B1 f(h_k / range) from known positive definite B0, B1 and range: the bars of
    test_variography_host.test_fit_recovers_exact_models for the same situation -- range and every entry of B0 and B1
    to 1e-6 relative (entries: relative to the matrix's largest), objective <= 1e-12 sum w ||Gamma||_F^2."""
    B0, B1, rng, nu = _psd(nz, 1, 0.2), _psd(nz, 2, 1.0), 42.0, 1.7
    G = _gamma(kind, B0, B1, rng, nu)
    w = vref.fit_weights(H, COUNT, weighting)
    k, r, b0, b1, obj = HipEngine.variogram_fit_lmc(H, cref.pack(G), COUNT, [kind], nu=nu, weighting=WCODE[weighting])
    rel = max(abs(r - rng) / rng, np.abs(b0 - B0).max() / np.abs(B0).max(), np.abs(b1 - B1).max() / np.abs(B1).max())
    scale = float((w * (G * G).sum(axis=(1, 2))).sum())
    print("%s/nz=%d/%s: relative error %.2e, objective / sum w |Gamma|^2 = %.2e" % (kind, nz, weighting, rel,
                                                                                   obj[0] / scale))
    assert k == kind
    assert rel <= 1e-6
    assert obj[0] <= 1e-12 * scale
    assert np.array_equal(b0, b0.T) and np.array_equal(b1, b1.T)


def _indefinite_case():
    """Two variables whose cross sill exceeds sqrt(b11 b22), plus noise: the entrywise fit is indefinite."""
    rng = np.random.default_rng(5)
    B0 = np.array([[0.10, 0.02], [0.02, 0.30]])
    B1 = np.array([[1.0, 1.6], [1.6, 2.0]])            # 1.6 > sqrt(2)
    G = _gamma("spherical", B0, B1, 40.0, 1.0)
    noise = 0.03 * rng.normal(size=G.shape)
    return G * (1.0 + 0.5 * (noise + noise.transpose(0, 2, 1)))


@pytest.mark.parametrize("weighting", ["count", "uniform"])
def test_lmc_projects_an_indefinite_fit(weighting):
    G = _indefinite_case()
    w = vref.fit_weights(H, COUNT, weighting)
    k, r, b0, b1, obj = HipEngine.variogram_fit_lmc(H, cref.pack(G), COUNT, ["spherical"], weighting=WCODE[weighting])
    f = vref.shape("spherical", H / r)
    u0, u1 = cref.lmc_unconstrained(G, f, w)
    assert np.linalg.eigvalsh(u1).min() < 0                     # the case is what it claims to be
    for m in (b0, b1):
        assert np.linalg.eigvalsh(m).min() >= -1e-12 * np.trace(m)
    # the reported objective is the objective of what is returned
    mine = cref.lmc_objective(G, f, w, b0, b1)
    assert abs(mine - obj[0]) <= 1e-9 * obj[0]
    # no larger than clipping the unconstrained solution once (at the library's range)
    once = cref.lmc_objective(G, f, w, cref.project_psd(u0), cref.project_psd(u1))
    print("objective %.6e, clipped once %.6e" % (obj[0], once))
    assert obj[0] <= once
    # and the numpy restatement of the whole algorithm agrees to the bar of the recovery test
    robj, rr, rb0, rb1 = cref.lmc_fit("spherical", H, G, w)
    rel = max(abs(r - rr) / rr, np.abs(b0 - rb0).max() / np.abs(rb0).max(), np.abs(b1 - rb1).max() / np.abs(rb1).max())
    print("library against restatement: relative difference %.2e, objectives %.12e %.12e" % (rel, obj[0], robj))
    assert rel <= 1e-6
    assert abs(obj[0] - robj) <= 1e-9 * robj


@pytest.mark.parametrize("kind", KINDS)
def test_lmc_of_one_variable_is_the_direct_fit(kind):
    rng = np.random.default_rng(11)
    g = vref.model(kind, H, 0.2, 1.0, 35.0, 1.3) * (1.0 + 0.08 * rng.normal(size=H.size))
    k, r, b0, b1, obj = HipEngine.variogram_fit_lmc(H, g[None, :], COUNT, [kind], nu=1.3)
    k2, s, n0, r2, order, obj2 = HipEngine.variogram_fit(H, g, COUNT, [kind], nu=1.3, max_nugget_frac=1.0)
    assert (k, r, b0[0, 0], b0[0, 0] + b1[0, 0], obj[0]) == (k2, r2, n0, s, obj2[0])


def test_lmc_refusals():
    G = cref.pack(_gamma("spherical", _psd(2, 1, 0.2), _psd(2, 2, 1.0), 40.0, 1.0))
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_fit_lmc(H, G, COUNT, ["power"])
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_fit_lmc(H, G, COUNT, ["gaussian", "power"])
    assert e.value.code == _lib.ERR_UNSUPPORTED
    c1 = np.zeros(20, np.int64)
    c1[3] = 5
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_fit_lmc(H, G, c1, ["gaussian"])
    assert e.value.code == _lib.ERR_INVALID and "two bins" in str(e.value)
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_fit_lmc(H, G, COUNT, ["gaussian"], weighting=3)
    assert e.value.code == _lib.ERR_INVALID
    lib = _lib.load()
    kind, r, obj, kinds = C.c_int32(0), C.c_double(0.0), np.zeros(1), np.zeros(1, np.int32)
    b = np.zeros(81)
    big = np.zeros((45, 20))
    for nz in (0, 9):
        assert lib.gss_variogram_fit_lmc(_lib.ptr(H), _lib.ptr(big), _lib.ptr(COUNT), 20, nz, _lib.ptr(kinds), 1, 1.0, 0,
                                         C.byref(kind), C.byref(r), _lib.ptr(b), _lib.ptr(b), _lib.ptr(obj)) \
            == _lib.ERR_INVALID
        assert "nz" in _lib.last_error()


def test_front_end_lmc_model():
    """fit_lmc on an exact Gaussian model: .variogram(a) evaluates to the fitted direct model (the nugget - 1e-6 rule of
    fit), .correlation is (B0 + B1)_ab / sqrt(sill_a sill_b)."""
    import gss
    from gss.variography import EmpiricalCrossVariogramResult, fit_lmc
    B0, B1 = np.array([[0.15, 0.05], [0.05, 0.10]]), np.array([[1.0, 0.6], [0.6, 2.0]])
    G = _gamma("gaussian", B0, B1, 42.0, 1.0)
    cross = EmpiricalCrossVariogramResult(("u", "v"), H, cref.pack(G), COUNT, 0, 100.0)
    m, obj = fit_lmc([gss.GaussianVariogram, "spherical"], cross, return_objectives=True)
    assert m.kind == "gaussian" and set(obj) == {"gaussian", "spherical"} and abs(m.range - 42.0) < 1e-4
    vu = m.variogram("u")
    assert vu.kind == "gaussian" and abs(vu.effective_nugget - 0.15) <= 2e-7 and abs(vu.sill - 1.15) <= 2e-6
    assert vu.regularize and m.variogram(1).range == vu.range
    S = B0 + B1
    assert abs(m.correlation("u", "v") - S[0, 1] / np.sqrt(S[0, 0] * S[1, 1])) <= 1e-6
    assert m.correlation("v", "u") == m.correlation(0, 1)
    assert "LUGS" in type(m).correlation.__doc__ and "correlation" in type(m).correlation.__doc__
    assert np.array_equal(cross.gamma("v", "u"), cross.gamma(0, 1)) and cross.direct("v").var == "v"
    assert np.array_equal(cross.direct(1).ordinate, G[:, 1, 1])
    with pytest.raises(_lib.GSSError):
        fit_lmc(gss.PowerVariogram, cross)
