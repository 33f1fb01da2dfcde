"""SPDEGS with data, without a device: the host restatement of conditioning by kriging against the dense formulas of
simple kriging, the brute-force point location, and the front end's defaults and refusals."""
import numpy as np
import pytest

import gss

import spde_cond_ref as CR
import spde_ref as R

RTOL = 1e-13


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("lumped", [False, True])
@pytest.mark.parametrize("mode", CR.MODES)
@pytest.mark.parametrize("name", R.MESHES)
def test_host_algorithm_matches_the_dense_formulas(name, mode, lumped, noisy):
    """W, the kriging mean and the posterior covariance (realisations of the nv + nd unit vectors, mean subtracted) of
    the host algorithm against K = Sigma P' inv(P Sigma P' + R); with R = 0 the realisations honour the data."""
    _, m, S, _ = R.dense(name)
    nv, nd = len(m), CR.NOBS[name]
    Sigma = CR.prior_cov(name, lumped)
    c = CR.conditioned(name, mode, lumped, noisy, RTOL)
    _, mean, post, C = CR.dense_kriging(Sigma, c.P, c.rvar, c.y, CR.MEAN)
    bound = CR.bound(RTOL, S, C, Sigma)
    errw = np.max(np.abs(c.W - np.linalg.solve(S, c.P.T)))
    errc = np.max(np.abs(c.C - C))
    errm = np.max(np.abs(c.mean() - mean))
    m0 = c.mean()
    Z = np.stack([c.realize(*np.split(e, [nv]))[0] - m0 for e in np.eye(nv + nd)])
    errp = np.max(np.abs(Z.T @ Z - post))
    print(name, mode, lumped, noisy, "cond(C) %.3g" % np.linalg.cond(C), "iterations", c.iters.min(), c.iters.max(),
          "W %.3g C %.3g mean %.3g posterior %.3g" % (errw, errc, errm, errp), "bound %.3g" % bound)
    assert max(errw, errc, errm, errp) <= bound
    if not noisy:
        g = np.random.default_rng(1)
        xc, xu = c.realize(g.normal(size=nv), g.normal(size=nd))
        errh = np.max(np.abs(c.P @ xc - c.y))
        print("honouring %.3g" % errh)
        assert errh <= bound and np.max(np.abs(xc - xu)) > 1e-3


@pytest.mark.parametrize("name", ["jitter", "sphere"])
def test_host_locate_finds_the_drawn_triangles(name):
    V, T, _, _ = R.mesh(name)
    for mode in CR.MODES:
        tri, _, w, _, pts = CR.case(name, mode)
        t, l = CR.locate(V, T, pts)
        err = np.max(np.abs(l - w))
        print(name, mode, "weight error %.3g (%.1f eps)" % (err, err / R.EPS))
        assert np.array_equal(t, tri) and err <= 64 * R.EPS
    t, l = CR.locate(V, T, V[:7])                           # a vertex goes to the lowest triangle that has it
    for v in range(7):
        assert t[v] == np.flatnonzero((T == v).any(axis=1))[0] and abs(l[v][list(T[t[v]]).index(v)] - 1.0) <= 64 * R.EPS
    if name == "jitter":
        assert CR.locate(V, T, np.array([[-5.0, 2.0]]))[0][0] == -1


def _problem(points, values, nreals=2, var="z"):
    mesh = gss.triangulate(gss.CartesianGrid(4, 3))
    return mesh, gss.SimulationProblem(gss.georef({var: values}, points), mesh, (var, float), nreals)


def test_front_end_defaults_and_refusals():
    s = gss.SPDEGS()
    assert s.globals["condition"] is None and s.globals["error_variance"] == 0.0 and s.globals["mean"] == 0.0
    assert s.params("z") == dict(sill=1.0, range=1.0)
    k = gss.SPDEKriging(("z", dict(sill=2.0, range=3.0)), error_variance={"z": 0.1}, mean=1.5)
    assert k.globals["condition"] == "element" and k.params("z") == dict(sill=2.0, range=3.0)
    assert k.globals["error_variance"] == {"z": 0.1} and k.globals["mean"] == 1.5
    assert "SPDEKriging" in gss.__all__ and hasattr(gss.SimpleMesh, "locate")
    _, problem = _problem([(0.5, 0.5)], [1.0])
    with pytest.raises(NotImplementedError, match="conditional simulation is not implemented"):
        gss.solve(problem, gss.SPDEGS())                                  # condition=None: the reference's refusal
    with pytest.raises(ValueError, match="condition='nearest'"):
        gss.solve(problem, gss.SPDEGS(condition="nearest"))
    with pytest.raises(ValueError, match="must not be negative"):
        gss.solve(problem, gss.SPDEGS(condition="element", error_variance=-0.5))
    with pytest.raises(ValueError, match="must not be negative"):
        gss.solve(problem, gss.SPDEGS(condition="point", error_variance={"z": -1e-3}))
    with pytest.raises(ValueError, match="finite"):
        gss.solve(problem, gss.SPDEGS(condition="point", mean=float("nan")))
    with pytest.raises(ValueError, match="triangulate"):
        gss.solve(gss.SimulationProblem(gss.georef({"z": [1.0]}, [(0.5, 0.5)]), gss.CartesianGrid(4, 3), ("z", float), 1),
                  gss.SPDEGS(condition="element"))
    est = gss.EstimationProblem(gss.georef({"z": [1.0]}, [(0.5, 0.5)]), gss.triangulate(gss.CartesianGrid(4, 3)), "z")
    with pytest.raises(ValueError, match="needs 'element' or 'point'"):
        gss.solve(est, gss.SPDEKriging(condition=None))
    with pytest.raises(ValueError, match="must not be negative"):
        gss.solve(est, gss.SPDEKriging(error_variance=-1.0))


class _Located:
    """An engine whose handle locates on the host (tests/spde_cond_ref.py) and records what is attached: the front
    end's own refusals need no device."""
    attached = []

    def __init__(self, vertices, triangles, **kw):
        self.V, self.T = np.asarray(vertices), np.asarray(triangles)

    def locate(self, points, tol=None):
        return CR.locate(self.V, self.T, np.asarray(points))

    def condition(self, *a, **kw):
        _Located.attached.append((a, kw))

    def close(self):
        pass


class _Engine:
    SPDE = _Located


def test_front_end_refuses_duplicate_triangles_and_data_outside_the_mesh():
    _, two = _problem([(0.6, 0.2), (0.7, 0.3), (2.6, 1.2)], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match=r"data \[0, 1\] of z lie in triangle 0"):
        gss.SPDEGS(condition="element", engine=_Engine).preprocess(two)
    _, out = _problem([(0.6, 0.2), (9.0, 1.0)], [1.0, 2.0])
    with pytest.raises(ValueError, match=r"datum 1 of z at \(9.0, 1.0\) lies outside the mesh"):
        gss.SPDEGS(condition="point", engine=_Engine).preprocess(out)
    # the same two data are fine as points, with an error variance, or when one of them is missing
    _Located.attached.clear()
    gss.SPDEGS(condition="point", engine=_Engine).preprocess(two)
    gss.SPDEGS(condition="element", error_variance=0.25, mean={"z": 2.0}, engine=_Engine).preprocess(two)
    _, nan = _problem([(0.6, 0.2), (0.7, 0.3), (2.6, 1.2)], [1.0, float("nan"), 3.0])
    gss.SPDEGS(condition="element", engine=_Engine).preprocess(nan)
    (a0, k0), (a1, k1), (a2, k2) = _Located.attached
    mesh = gss.triangulate(gss.CartesianGrid(4, 3))
    assert np.array_equal(a0[0], mesh.triangles[[0, 0, 12]]) and a0[3] is None and k0["mean"] == 0.0
    assert np.allclose(a0[1].sum(axis=1), 1.0) and not np.allclose(a0[1], 1.0 / 3.0)      # barycentric weights
    assert np.array_equal(a1[1], np.full((3, 3), 1.0 / 3.0)) and np.array_equal(a1[3], np.full(3, 0.25))
    assert k1["mean"] == 2.0
    assert np.array_equal(a2[2], [1.0, 3.0]) and np.array_equal(a2[0], mesh.triangles[[0, 12]])   # the NaN row is skipped
