"""The parts of the varioplane feature that need no device: gss_variogram_fit_aniso (host code of the library), the
sector rule of the restatement in tests/varioplane_ref.py, and the twin's front-ends on a stub engine that computes
with that restatement."""
import ctypes as C

import numpy as np
import pytest

import varioplane_ref as pref
import variography_ref as vref
from gss import _lib
from gss.engine import HipEngine
from oracle_engine import OracleEngine

KINDS = ("gaussian", "exponential", "spherical", "matern", "cubic", "pentaspherical", "sinehole")
WEIGHTINGS = {"count": 0, "count/h2": 1, "uniform": 2}
MID = (np.arange(18) + 0.5) * np.pi / 18
LAGS = np.arange(1.0, 21.0) * 3.0
HH = np.ascontiguousarray(np.broadcast_to(LAGS[None, :], (18, 20)))
PHI = np.ascontiguousarray(np.broadcast_to(MID[:, None], (18, 20)))
COUNT = (1000 + 37 * np.arange(360)).reshape(18, 20).astype(np.int64)
NU = 1.5      # a closed-form Matern order: the general order evaluates a Bessel function per bin and grid point


class StubEngine(OracleEngine):
    """The stand-in engine plus the two varioplane methods, computed by the restatement / the library's host code."""
    calls = []

    @staticmethod
    def variogram_plane(x, z, nlags, maxlag, dirs, basis=None, ptol=float("inf"), estimator=0):
        StubEngine.calls.append((np.asarray(z).shape[0], None if basis is None else np.array(basis)))
        return pref.plane(x, z, nlags, maxlag, dirs, basis, ptol, "matheron" if estimator == 0 else "cressie")

    variogram_fit_aniso = staticmethod(HipEngine.variogram_fit_aniso)
    variogram_fit = staticmethod(HipEngine.variogram_fit)


@pytest.mark.parametrize("weighting", list(WEIGHTINGS))
@pytest.mark.parametrize("r1,r2,theta", [(40.0, 10.0, 0.5), (30.0, 20.0, 2.6), (25.0, 5.0, 0.0)])
@pytest.mark.parametrize("kind", KINDS)
def test_fit_aniso_recovers_exact_ordinates(kind, r1, r2, theta, weighting):
    """gamma from the model at 18 mid-angles x 20 lags: the objective is exactly zero at the truth, so this is a
    requirement on the optimiser.  Achieved over the 63 cases (x86-64 host): largest error 1.6e-8 (sine hole,
    count / h^2 weights, radii 40 : 10)."""
    sill, nugget = 1.3, 0.1
    g = pref.aniso_model(kind, HH, PHI, nugget, sill, r1, r2, theta, NU)
    lib = _lib.load()
    best, obj = _lib.Variogram(), np.zeros(1)
    kk = np.array([_lib._KINDS[kind]], dtype=np.int32)
    code = lib.gss_variogram_fit_aniso(_lib.ptr(HH), _lib.ptr(PHI), _lib.ptr(np.ascontiguousarray(g)), _lib.ptr(COUNT),
                                       360, _lib.ptr(kk), 1, NU, WEIGHTINGS[weighting], 1.0, C.byref(best),
                                       _lib.ptr(obj))
    assert code == 0, _lib.last_error()
    assert best.aniso == 2 and best.kind == _lib._KINDS[kind] and best.range == 1.0
    R = np.array(list(best.rotation)).reshape(3, 3)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
    assert R[2, 2] == 1.0 and R[0, 2] == R[1, 2] == R[2, 0] == R[2, 1] == 0.0 and best.inv_radii[2] == 1.0
    f1, f2 = 1.0 / best.inv_radii[0], 1.0 / best.inv_radii[1]
    ftheta = np.arctan2(R[1, 0], R[0, 0])            # first column = the axis of r1
    dtheta = abs((ftheta - theta + np.pi / 2) % np.pi - np.pi / 2)
    print("%s %s: r1 %.2e r2 %.2e sill %.2e nugget %.2e theta %.2e" % (kind, weighting, abs(f1 - r1) / r1,
          abs(f2 - r2) / r2, abs(best.sill - sill) / sill, abs(best.nugget - nugget), dtheta))
    assert f1 >= f2 > 0 and 0.0 <= ftheta % np.pi < np.pi
    assert abs(f1 - r1) <= 1e-6 * r1 and abs(f2 - r2) <= 1e-6 * r2 and abs(best.sill - sill) <= 1e-6 * sill
    assert abs(best.nugget - nugget) <= 1e-6 and dtheta <= 1e-6


@pytest.mark.parametrize("kind", ["spherical", "gaussian", "exponential"])
def test_isotropic_ordinates_return_the_isotropic_form(kind):
    g = pref.aniso_model(kind, HH, PHI, 0.1, 1.3, 30.0, 30.0, 0.0)
    k, s, n0, radii, theta, rng, order, obj = HipEngine.variogram_fit_aniso(HH, PHI, g, COUNT, [kind])
    assert radii is None and abs(rng - 30.0) <= 1e-6 * 30.0 and abs(s - 1.3) <= 1e-6 and abs(n0 - 0.1) <= 1e-6
    lib = _lib.load()
    best, o = _lib.Variogram(), np.zeros(1)
    kk = np.array([_lib._KINDS[kind]], dtype=np.int32)
    assert lib.gss_variogram_fit_aniso(_lib.ptr(HH), _lib.ptr(PHI), _lib.ptr(np.ascontiguousarray(g)), _lib.ptr(COUNT),
                                       360, _lib.ptr(kk), 1, 1.0, 0, 1.0, C.byref(best), _lib.ptr(o)) == 0
    assert best.aniso == 0 and list(best.rotation) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(best.inv_radii) == [1, 1, 1]


def test_max_nugget_frac_is_honoured():
    g = pref.aniso_model("spherical", HH, PHI, 0.6, 1.0, 40.0, 15.0, 1.0)
    free = HipEngine.variogram_fit_aniso(HH, PHI, g, COUNT, ["spherical"])
    assert abs(free[2] - 0.6) <= 1e-6
    k, s, n0, radii, theta, rng, order, obj = HipEngine.variogram_fit_aniso(HH, PHI, g, COUNT, ["spherical"],
                                                                          max_nugget_frac=0.25)
    assert n0 <= 0.25 * s * (1 + 1e-12) and obj[0] > free[7][0]
    assert HipEngine.variogram_fit_aniso(HH, PHI, g, COUNT, ["spherical"], max_nugget_frac=0.0)[2] == 0.0


def test_power_is_unsupported_and_bad_arguments_invalid():
    g = pref.aniso_model("spherical", HH, PHI, 0.1, 1.0, 40.0, 15.0, 1.0)
    for kinds in (["power"], ["gaussian", "power"]):
        with pytest.raises(_lib.GSSError) as e:
            HipEngine.variogram_fit_aniso(HH, PHI, g, COUNT, kinds)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    for kw in (dict(weighting=3), dict(max_nugget_frac=1.5)):
        with pytest.raises(_lib.GSSError) as e:
            HipEngine.variogram_fit_aniso(HH, PHI, g, COUNT, ["gaussian"], **kw)
        assert e.value.code == _lib.ERR_INVALID
    c = np.zeros_like(COUNT)
    c[0, :3] = 5
    with pytest.raises(_lib.GSSError) as e:
        HipEngine.variogram_fit_aniso(HH, PHI, g, c, ["gaussian"])
    assert e.value.code == _lib.ERR_INVALID and "four bins" in str(e.value)


def test_fit_is_deterministic_and_picks_the_generating_kind():
    rng = np.random.default_rng(3)
    g = pref.aniso_model("exponential", HH, PHI, 0.1, 1.0, 35.0, 14.0, 2.0) * (1.0 + 0.05 * rng.normal(size=HH.shape))
    a = HipEngine.variogram_fit_aniso(HH, PHI, g, COUNT, ["spherical", "exponential"])
    b = HipEngine.variogram_fit_aniso(HH, PHI, g, COUNT, ["spherical", "exponential"])
    assert a[0] == b[0] == "exponential" and a[1:7] == b[1:7] and np.array_equal(a[7], b[7])
    assert a[3][0] >= a[3][1] and abs(a[4] - 2.0) < 0.1
    # what it reports is the objective of what it returns
    mine = np.sum(COUNT * (pref.aniso_model("exponential", HH, PHI, a[2], a[1], a[3][0], a[3][1], a[4]) - g) ** 2)
    assert abs(mine - a[7][1]) <= 1e-9 * a[7][1]


@pytest.mark.parametrize("offset", [0.0, 0.3, 1.1])
@pytest.mark.parametrize("nangles", [4, 18, 36, 180])
def test_sector_rule_of_the_restatement(nangles, offset):
    """The counted rule equals the atan2 form, has a prefix truth pattern (so a search may replace the count) and does
    not depend on the sense of the lag: 60 000 random lags at three scales and a 13 x 13 integer lattice."""
    rng = np.random.default_rng(nangles)
    a = np.concatenate([rng.normal(size=(20000, 2)) * s for s in (1e-3, 1.0, 1e4)])
    g = np.arange(-6.0, 7.0)
    lat = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    a = np.concatenate([a, lat[(lat != 0).any(axis=1)]])
    dirs = pref.uniform_dirs(nangles, offset)
    sec = pref.sector(a[:, 0], a[:, 1], dirs)
    assert sec.min() >= 0 and sec.max() == nangles - 1
    assert np.array_equal(sec, pref.sector(-a[:, 0], -a[:, 1], dirs))
    ref = pref.sector_atan2(a[:, 0], a[:, 1], nangles, offset)
    # a lag within rounding of a boundary may fall on either side in the atan2 form: compare away from them
    t = np.mod(np.arctan2(a[:, 1], a[:, 0]) - offset, np.pi) / (np.pi / nangles)
    away = np.abs(t - np.round(t)) > 1e-9
    assert away.sum() >= a.shape[0] - 400 and np.array_equal(sec[away], ref[away])
    flip = dirs[0, 0] * a[:, 1] < dirs[0, 1] * a[:, 0]
    b1, b2 = np.where(flip, -a[:, 0], a[:, 0]), np.where(flip, -a[:, 1], a[:, 1])
    truth = np.stack([dirs[s, 0] * b2 >= dirs[s, 1] * b1 for s in range(1, nangles)])
    assert (np.diff(truth.astype(np.int8), axis=0) <= 0).all()          # true ... true false ... false


def _table(d, n=300, nvars=1, seed=0):
    import gss
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 50.0, (n, d))
    cols = {"v%d" % i: rng.normal(size=n) for i in range(nvars)}
    return gss.georef(cols, x), x, cols


def test_twin_shapes_and_empty_bins():
    import gss
    data, x, cols = _table(2)
    p = gss.EmpiricalVarioplane(data, "v0", nangs=6, nlags=40, maxlag=8.0, offset=0.25, engine=StubEngine)
    assert isinstance(p, gss.EmpiricalVarioplaneResult) and (p.nangs, p.nlags) == (6, 40)
    assert p.abscissa.shape == p.ordinate.shape == p.counts.shape == (6, 40) and p.counts.dtype == np.int64
    assert np.allclose(p.angles, 0.25 + np.arange(6) * np.pi / 6) and np.allclose(p.midangles - p.angles, np.pi / 12)
    empty = p.counts == 0
    assert empty.any() and np.isnan(p.abscissa[empty]).all() and np.isnan(p.ordinate[empty]).all()
    assert np.isfinite(p.abscissa[~empty]).all() and np.isfinite(p.ordinate[~empty]).all()
    omni = vref.empirical(x, cols["v0"][None], 40, 8.0)
    assert np.array_equal(p.counts.sum(axis=0), omni[0])
    s = p.sector(3)
    assert isinstance(s, gss.EmpiricalVariogramResult) and np.array_equal(s.counts, p.counts[3]) and s.maxlag == 8.0
    default = gss.EmpiricalVarioplane(data, "v0", engine=StubEngine)
    assert default.counts.shape == (18, 20)
    with pytest.raises(ValueError):
        gss.EmpiricalVarioplane(data, "v0", estimator="median", engine=StubEngine)


def test_twin_normal_rules():
    import gss
    from gss.variography import plane_basis
    d2, _, _ = _table(2)
    d3, x3, cols = _table(3)
    with pytest.raises(ValueError):
        gss.EmpiricalVarioplane(d2, "v0", normal=(0, 0, 1), engine=StubEngine)
    with pytest.raises(ValueError):
        gss.EmpiricalVarioplane(d3, "v0", engine=StubEngine)
    with pytest.raises(ValueError):
        gss.EmpiricalVarioplane(d3, "v0", normal=(0, 0, 0), engine=StubEngine)
    assert np.array_equal(plane_basis((0, 0, 2.0)), np.eye(3))
    for nrm in ((1.0, 2.0, -3.0), (0.0, 1.0, 0.0), (-1.0, 1.0, 1.0)):
        e = plane_basis(nrm)
        assert np.abs(e @ e.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(e) > 0
        assert np.allclose(e[2], np.asarray(nrm) / np.linalg.norm(nrm))
    StubEngine.calls.clear()
    p = gss.EmpiricalVarioplane(d3, "v0", nangs=4, nlags=5, maxlag=20.0, normal=(1.0, 2.0, -3.0), ptol=4.0,
                                engine=StubEngine)
    assert np.array_equal(StubEngine.calls[-1][1], plane_basis((1.0, 2.0, -3.0)))
    ref = pref.plane(x3, cols["v0"][None], 5, 20.0, pref.uniform_dirs(4), plane_basis((1.0, 2.0, -3.0)), 4.0)
    assert np.array_equal(p.counts, ref[0])


def test_twin_splits_columns_and_groups_missing_values():
    import gss
    data, x, cols = _table(2, nvars=6)
    StubEngine.calls.clear()
    res = gss.EmpiricalVarioplane(data, list(cols), nangs=4, nlags=5, maxlag=20.0, engine=StubEngine)
    assert [c[0] for c in StubEngine.calls] == [4, 2] and set(res) == set(cols)
    for name, col in cols.items():
        ref = pref.plane(x, col[None], 5, 20.0, pref.uniform_dirs(4))
        assert np.array_equal(res[name].counts, ref[0]) and np.allclose(res[name].ordinate, ref[2][0] / (2 * ref[0]))
    # a histogram of 36 x 50 bins leaves room for two columns per call: 36 * 50 * (2 + 2) <= 8192 < 36 * 50 * 5
    StubEngine.calls.clear()
    gss.EmpiricalVarioplane(data, list(cols)[:3], nangs=36, nlags=50, maxlag=20.0, engine=StubEngine)
    assert [c[0] for c in StubEngine.calls] == [2, 1]
    cols["v1"][::5] = np.nan
    data = gss.georef(cols, x)
    StubEngine.calls.clear()
    res = gss.EmpiricalVarioplane(data, ["v0", "v1"], nangs=4, nlags=5, maxlag=20.0, engine=StubEngine)
    assert [c[0] for c in StubEngine.calls] == [1, 1]
    keep = np.isfinite(cols["v1"])
    assert np.array_equal(res["v1"].counts, pref.plane(x[keep], cols["v1"][keep][None], 5, 20.0, pref.uniform_dirs(4))[0])


def test_fit_anisotropic_returns_a_rotated_ball_model():
    import gss
    from gss.variography import EmpiricalVarioplaneResult
    for kind, nugget in (("gaussian", 0.15), ("gaussian", 0.0), ("spherical", 0.1)):
        g = pref.aniso_model(kind, HH, PHI, nugget, 1.3, 40.0, 10.0, 0.5)
        plane = EmpiricalVarioplaneResult(MID - np.pi / 36, MID, HH, g, COUNT, 0, 60.0)
        m, obj = gss.fit_anisotropic(kind, plane, return_objectives=True, engine=StubEngine)
        assert m.kind == kind and set(obj) == {kind} and abs(m.effective_nugget - nugget) <= 2e-7
        assert abs(m.radii[0] - 40.0) <= 1e-4 and abs(m.radii[1] - 10.0) <= 1e-4 and m.range == 1.0
        assert np.allclose(np.array(m.rotation), [[np.cos(0.5), -np.sin(0.5)], [np.sin(0.5), np.cos(0.5)]], atol=1e-8)
        if kind == "gaussian":
            assert m.regularize == (nugget > 0)
        from gss.engine import _vg_struct
        v = _vg_struct(m, 2)                          # what every solver hands to the library
        assert v.aniso == 2 and abs(1.0 / v.inv_radii[0] - 40.0) <= 1e-4
    iso = EmpiricalVarioplaneResult(MID - np.pi / 36, MID, HH, pref.aniso_model("spherical", HH, PHI, 0.1, 1.0, 30.0, 30.0, 0.0),
                                    COUNT, 0, 60.0)
    m = gss.fit_anisotropic(gss.SphericalVariogram, iso, engine=StubEngine)
    assert m.radii is None and m.rotation is None and abs(m.range - 30.0) <= 1e-4
    with pytest.raises(_lib.GSSError):
        gss.fit_anisotropic(gss.PowerVariogram, iso, engine=StubEngine)
    with pytest.raises(ValueError):
        gss.fit_anisotropic("spherical", iso, weighting="none", engine=StubEngine)
