"""Rotated anisotropy on the device: every solver with a rotated variogram and/or ball on x equals the frozen oracle
with the axis-aligned ball on the frame coordinates x' = R^T (x - c) (tests/rotated_frame.py), neighbour indices
bit-exact; covariances against direct Mahalanobis evaluation; an independent numpy OK solve in the raw frame."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import fftgs as offt, idw_lwr as OIL, kriging as K, lugs as OL, sgs as OS  # noqa: E402
from oracle.variogram import Nested, Variogram, cov_h, cov_pairwise  # noqa: E402
from rotated_frame import frame, mahalanobis_sq, rot2, rot3  # noqa: E402

pytestmark = pytest.mark.gpu

R2 = rot2(0.5235987755982988)          # 30 degrees
R3 = rot3(0.4, -0.7, 1.2)
RADII = {2: (25.0, 6.0), 3: (30.0, 12.0, 5.0)}
ROT = {2: R2, 3: R3}
CTORS = ("gaussian", "exponential", "spherical", "matern", "cubic", "pentaspherical", "sinehole")


def _g(kind, radii=None, R=None, **kw):
    import gss
    ctor = dict(gaussian=gss.GaussianVariogram, exponential=gss.ExponentialVariogram, spherical=gss.SphericalVariogram,
                matern=gss.MaternVariogram, cubic=gss.CubicVariogram, pentaspherical=gss.PentasphericalVariogram,
                sinehole=gss.SineHoleVariogram)[kind]
    if "nu" in kw:
        kw["order"] = kw.pop("nu")
    return ctor(gss.MetricBall(tuple(radii), R) if radii is not None else None, **kw)


def _data(d, n, m, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, d))
    xdom = rng.uniform(0, 100, (m, d))
    z = np.sin(x[:, 0] / 17.0) + 0.3 * rng.normal(size=n)
    return x, z, xdom


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("kind", CTORS)
def test_cov_pairwise_is_mahalanobis(d, kind):
    from gss.engine import HipEngine
    rng = np.random.default_rng(7)
    a, b = rng.uniform(0, 60, (50, d)), rng.uniform(0, 60, (40, d))
    r, R = RADII[d], ROT[d]
    kw = dict(sill=2.0, nugget=0.1)
    if kind == "matern":
        kw["nu"] = 1.5
    out = HipEngine.cov_pairwise(_g(kind, r, R, **kw), a, b)
    ovg = Variogram(kind, radii=r, **kw)
    ref = cov_h(ovg, np.sqrt(mahalanobis_sq(a, b, r, R)))
    assert np.max(np.abs(out - ref)) < 1e-13


def test_cov_pairwise_nested_rotated_plus_isotropic():
    from gss.engine import HipEngine
    rng = np.random.default_rng(8)
    a = rng.uniform(0, 60, (60, 3))
    vg = _g("spherical", RADII[3], R3, sill=1.5) + 0.5 * _g("exponential", range=9.0)
    out = HipEngine.cov_pairwise(vg, a)
    h1 = np.sqrt(mahalanobis_sq(a, a, RADII[3], R3))
    h2 = np.sqrt(mahalanobis_sq(a, a, (9.0,) * 3, np.eye(3)))
    ref = cov_h(Variogram("spherical", sill=1.5, radii=RADII[3]), h1) + 0.5 * cov_h(Variogram("exponential", range=1.0),
                                                                                    h2)
    assert np.max(np.abs(out - ref)) < 1e-13


@pytest.mark.parametrize("d", [2, 3])
def test_knn_search_rotated_ball_is_the_frame_search(d):
    from gss.engine import HipEngine
    x, _, c = _data(d, 3000, 700, 11)
    r, R = RADII[d], ROT[d]
    idx, cnt = HipEngine.knn_search(x, c, 24, radii=r, rotation=R)
    ridx, rcnt = K.knn_search(frame(x, R), frame(c, R, c=x[0]), 24, None, r)
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("variant", [K.SK, K.OK, K.UK])
def test_global_kriging_is_the_frame_kriging(d, variant):
    from gss.engine import KrigHandle
    x, z, xdom = _data(d, 400, 900, 21 + variant)
    r, R = RADII[d], ROT[d]
    kw = dict(sill=1.3, nugget=0.05)
    h = KrigHandle(_g("spherical", r, R, **kw), variant, x, z, mean=0.2, degree=1 if variant == K.UK else 0)
    mu, var, st = h.predict_global(xdom)
    fx = frame(x, R)
    rmu, rvar = K.exactsolve(variant, Variogram("spherical", radii=r, **kw), fx, z, frame(xdom, R, c=x[0]), mean=0.2,
                             degree=1 if variant == K.UK else None)
    assert np.all(st == 0)
    assert np.max(np.abs(mu - rmu)) < 1e-9 and np.max(np.abs(var - rvar)) < 1e-9


@pytest.mark.parametrize("d,k", [(2, 16), (3, 16), (3, 100), (3, 300), (2, 900)])
def test_moving_neighbourhood_is_the_frame_kriging(d, k):
    from gss.engine import KrigHandle
    x, z, xdom = _data(d, 2500, 60, 31 + k)
    r, R = RADII[d], ROT[d]
    kw = dict(sill=1.0, nugget=0.1)
    h = KrigHandle(_g("exponential", r, R, **kw), K.OK, x, z, factor=False)
    mu, var, st, idx, cnt = h.predict_knn(xdom, k, 1, radii=r, rotation=R, return_idx=True)
    fx, fd = frame(x, R), frame(xdom, R, c=x[0])
    rmu, rvar, rst, ridx, rcnt = K.approxsolve(K.OK, Variogram("exponential", radii=r, **kw), fx, z, fd, k, 1,
                                               radii=r, return_idx=True)
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt)
    ok = rst == 0
    assert np.array_equal(st, rst)
    assert np.max(np.abs(mu[ok] - rmu[ok])) < 1e-9 and np.max(np.abs(var[ok] - rvar[ok])) < 1e-9


def test_two_frames_ball_rotation_differs_from_the_variogram_rotation():
    from gss.engine import KrigHandle
    x, z, xdom = _data(2, 1500, 200, 41)
    Rv, Rb, rv, rb = R2, rot2(-1.1), RADII[2], (30.0, 10.0)
    h = KrigHandle(_g("gaussian", rv, Rv, sill=1.0, nugget=0.05), K.OK, x, z, factor=False)
    mu, var, st, idx, cnt = h.predict_knn(xdom, 20, 1, radii=rb, rotation=Rb, return_idx=True)
    ridx, rcnt = K.knn_search(frame(x, Rb), frame(xdom, Rb, c=x[0]), 20, None, rb)
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt)
    ovg = Variogram("gaussian", radii=rv, sill=1.0, nugget=0.05)
    fx, fd = frame(x, Rv), frame(xdom, Rv, c=x[0])
    for p in range(0, 200, 17):
        nb = ridx[p, :rcnt[p]]
        fk = K.fit(K.OK, ovg, fx[nb], z[nb])
        a, b = K.predict(fk, fd[p:p + 1])
        assert abs(mu[p] - a[0]) < 1e-9 and abs(var[p] - b[0]) < 1e-9


def test_rotated_variogram_with_cityblock_search_ranks_in_the_raw_frame():
    from gss.engine import KrigHandle
    x, z, xdom = _data(3, 1200, 150, 43)
    h = KrigHandle(_g("spherical", RADII[3], R3), K.OK, x, z, factor=False)
    _, _, _, idx, cnt = h.predict_knn(xdom, 12, 1, distance="cityblock", return_idx=True)
    ridx, rcnt = K.knn_search(x, xdom, 12, distance="cityblock")
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt)


def test_independent_ordinary_kriging_in_the_raw_frame():
    from gss.engine import KrigHandle
    x, z, xdom = _data(2, 40, 25, 51)
    r, R = (30.0, 7.0), R2
    h = KrigHandle(_g("exponential", r, R, sill=1.0), K.OK, x, z)
    mu, var, _ = h.predict_global(xdom)
    ovg = Variogram("exponential", range=1.0)
    C_ = cov_h(ovg, np.sqrt(mahalanobis_sq(x, x, r, R)))
    c0 = cov_h(ovg, np.sqrt(mahalanobis_sq(x, xdom, r, R)))
    n = len(x)
    A = np.ones((n + 1, n + 1))
    A[:n, :n], A[n, n] = C_, 0.0
    sol = np.linalg.solve(A, np.vstack([c0, np.ones((1, len(xdom)))]))
    assert np.max(np.abs(sol[:n].T @ z - mu)) < 1e-9
    assert np.max(np.abs((1.0 - np.sum(sol * np.vstack([c0, np.ones((1, len(xdom)))]), 0)) - var)) < 1e-9


def test_identity_rotation_is_bit_identical_and_quarter_turn_swaps_radii():
    from gss.engine import KrigHandle
    x, z, xdom = _data(2, 800, 300, 61)
    a = KrigHandle(_g("spherical", (20.0, 6.0), np.eye(2)), K.OK, x, z).predict_global(xdom)
    b = KrigHandle(_g("spherical", (20.0, 6.0)), K.OK, x, z).predict_global(xdom)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    q = KrigHandle(_g("spherical", (20.0, 6.0), [[0.0, -1.0], [1.0, 0.0]]), K.OK, x, z).predict_global(xdom)
    s = KrigHandle(_g("spherical", (6.0, 20.0)), K.OK, x, z).predict_global(xdom)
    assert np.max(np.abs(q[0] - s[0])) < 1e-12 and np.max(np.abs(q[1] - s[1])) < 1e-12


def test_rotating_everything_together_leaves_estimates_unchanged():
    from gss.engine import KrigHandle
    x, z, xdom = _data(3, 600, 200, 71)
    S = rot3(1.0, 0.3, -0.8)
    r = RADII[3]
    base = KrigHandle(_g("exponential", r, R3, nugget=0.1), K.OK, x, z)
    m0, v0, _ = base.predict_global(xdom)
    k0 = base.predict_knn(xdom, 30, 1, radii=r, rotation=R3)
    rot = KrigHandle(_g("exponential", r, S @ R3, nugget=0.1), K.OK, x @ S.T, z)
    m1, v1, _ = rot.predict_global(xdom @ S.T)
    k1 = rot.predict_knn(xdom @ S.T, 30, 1, radii=r, rotation=S @ R3)
    assert np.max(np.abs(m0 - m1)) < 1e-10 and np.max(np.abs(v0 - v1)) < 1e-10
    ok = k0[2] == 0                                       # points without a sample in the ball are missing in both
    assert np.array_equal(k0[2], k1[2]) and ok.sum() > 100
    assert np.max(np.abs(k0[0][ok] - k1[0][ok])) < 1e-10 and np.max(np.abs(k0[1][ok] - k1[1][ok])) < 1e-10


@pytest.mark.parametrize("d", [2, 3])
def test_idw_and_lwr_search_on_the_ball_frame(d):
    from gss.engine import HipEngine
    x, z, xdom = _data(d, 1500, 300, 81)
    r, R = tuple(2.0 * v for v in RADII[d]), ROT[d]       # some 90 (3-D) to 280 (2-D) samples per ball
    fx, fd = frame(x, R), frame(xdom, R, c=x[0])
    mu, dist, st = HipEngine.idw(x, z, xdom, 12, 1, 2.0, radii=r, rotation=R)
    rmu, rdist, rst = OIL.idw(fx, z, fd, 12, 1, 2.0, radii=r)
    ok = rst == 0
    assert np.array_equal(st, rst) and np.max(np.abs(mu[ok] - rmu[ok])) < 1e-9
    assert np.max(np.abs(dist[ok] - rdist[ok])) < 1e-9
    mu, nr, st = HipEngine.lwr(x, z, xdom, 16, 1, radii=r, rotation=R)
    rmu, rnr, rst = OIL.lwr(fx, z, fd, 16, 1, radii=r)
    ok = rst == 0
    assert np.array_equal(st, rst) and np.max(np.abs(mu[ok] - rmu[ok])) < 1e-9
    assert np.max(np.abs(nr[ok] - rnr[ok])) < 1e-9


def test_lugs_is_the_frame_lugs():
    from gss.engine import LUGSHandle
    cent = offt.grid_centroids((24, 18))
    N = cent.shape[0]
    rng = np.random.default_rng(91)
    dlocs = np.sort(rng.choice(N, 30, replace=False))
    z1 = rng.normal(size=30)
    h = LUGSHandle(_g("spherical", (12.0, 4.0), R2, nugget=0.02), cent, dlocs, z1, mean=0.5)
    fc = frame(cent, R2)
    p = OL.preprocess(Variogram("spherical", radii=(12.0, 4.0), nugget=0.02), fc, fc[dlocs], z1, mean=0.5)
    assert np.array_equal(p.dlocs, dlocs)
    L22, d2 = h.factor()
    assert np.max(np.abs(L22 - p.L22)) < 1e-9 and np.max(np.abs(d2 - p.d2)) < 1e-9
    w = rng.normal(size=(2, h.ns))
    y, _ = h.realize(0, 0, 2, noise=w)
    for i in range(2):
        assert np.max(np.abs(y[i] - OL.lusim(p, w[i])[0])) < 1e-9


@pytest.mark.parametrize("ball_rot", [True, False])
def test_sgs_is_the_frame_sgs(ball_rot):
    from gss.engine import SGSHandle
    cent = offt.grid_centroids((30, 20))
    N = cent.shape[0]
    dl = np.array([5, 77, 300, 512])
    zd = np.array([1.0, -1.0, 0.5, 0.2])
    r = (14.0, 5.0)
    Rb = R2 if ball_rot else rot2(-0.9)
    h = SGSHandle(_g("spherical", r, R2), cent, None, dl, zd, 0.0, 10, 1, radii=(40.0, 12.0), rotation=Rb,
                  mask_after_search=True)
    eps = np.random.default_rng(5).normal(size=(1, N))
    y = h.realize(0, 0, 1, noise=eps)[0]
    # reference: search on the ball frame, covariances on the variogram frame (identical when the rotations agree)
    fb, fv = frame(cent, Rb), frame(cent, R2)
    idx, nc, w, sg = h.weights()
    href = SGSHandle(_g("spherical", r), fv, None, dl, zd, 0.0, 10, 1, radii=(40.0, 12.0), mask_after_search=True)
    if ball_rot:
        ry = OS.solvesingle(Variogram("spherical", radii=r), 0.0, fv, np.arange(N), dl, zd, eps[0], 10, 1,
                            radii=(40.0, 12.0), mask_after_search=True)
        assert np.max(np.abs(y - ry)) < 1e-9
        ridx, rnc, rw, rsg = href.weights()
        assert np.array_equal(nc, rnc)
        for node in np.flatnonzero(nc):                  # data cells (nc = 0) carry no list
            c = nc[node]
            assert np.array_equal(idx[node, :c], ridx[node, :c])
            assert np.max(np.abs(w[node, :c] - rw[node, :c])) < 1e-9 and abs(sg[node] - rsg[node]) < 1e-9
    else:
        raw = K.knn_search(fb, fb, 10, None, (40.0, 12.0))[0]
        for node in (0, 150, 420, 599):
            if node in dl or nc[node] == 0:
                continue
            kept = [j for j in raw[node] if j >= 0 and j != node and (j < node or j in dl)]
            nb = idx[node, :nc[node]]
            assert sorted(nb) == sorted(kept)
            ovg = Variogram("spherical", radii=r)
            c0 = cov_pairwise(ovg, fv[nb], fv[node][None])[:, 0]
            lam = np.linalg.solve(cov_pairwise(ovg, fv[nb]), c0)
            assert np.max(np.abs(w[node, :nc[node]] - lam)) < 1e-9


def test_refusals():
    import gss
    from gss import _lib
    from gss.engine import FFTGSHandle, KrigHandle, _vg_struct
    x, z, _ = _data(2, 50, 1, 3)
    h = KrigHandle(_g("spherical", (20.0, 5.0), R2), K.OK, x, z)
    with pytest.raises(_lib.GSSError) as e:
        h.set_block_support((1.0, 1.0), 3)
    assert e.value.code == _lib.ERR_INVALID
    v = _vg_struct(_g("spherical", (20.0, 5.0), R2), 2)
    v.rotation[0] = 1.5                                   # not orthonormal
    out = np.empty((50, 50))
    code = _lib.lib().gss_cov_pairwise(C.byref(v), _lib.ptr(x), 50, None, 50, _lib.ptr(out), 50, _lib.MEM_HOST, None)
    assert code == _lib.ERR_INVALID and "orthonormal" in _lib.last_error()
    v = _vg_struct(_g("spherical", (20.0, 5.0), R2), 2)
    for k, val in enumerate([0.0, 1.0, 0, 1.0, 0.0, 0, 0, 0, 1.0]):   # a reflection: det -1
        v.rotation[k] = val
    code = _lib.lib().gss_cov_pairwise(C.byref(v), _lib.ptr(x), 50, None, 50, _lib.ptr(out), 50, _lib.MEM_HOST, None)
    assert code == _lib.ERR_INVALID and "det" in _lib.last_error()
    # a rotated structure nested with an axis-aligned anisotropic one (its identity rotation differs): refused
    v = _vg_struct(_g("spherical", (20.0, 5.0), R2), 2)
    v.nextra = 1
    x0 = v.extra[0]
    x0.kind, x0.aniso, x0.sill, x0.range, x0.nu = 1, 1, 0.5, 1.0, 1.0
    x0.inv_radii[0], x0.inv_radii[1], x0.inv_radii[2] = 1 / 4.0, 1 / 20.0, 1.0
    code = _lib.lib().gss_cov_pairwise(C.byref(v), _lib.ptr(x), 50, None, 50, _lib.ptr(out), 50, _lib.MEM_HOST, None)
    assert code == _lib.ERR_INVALID and "axis-aligned" in _lib.last_error()
    x0.inv_radii[1] = 1 / 4.0                            # ... but a sphere does not depend on the frame
    code = _lib.lib().gss_cov_pairwise(C.byref(v), _lib.ptr(x), 50, None, 50, _lib.ptr(out), 50, _lib.MEM_HOST, None)
    assert code == _lib.OK
    with pytest.raises(ValueError, match="axis-aligned"):
        _g("spherical", (30.0, 5.0), 0.5) + _g("exponential", (4.0, 20.0))
    assert gss.MetricBall((2.0, 1.0), 0.2).rotation is not None


def _rotated_spectrum(kind, dims, spacing, radii, R, **kw):
    """sqrt|FFT| of the covariance grid to the centre cell at rotated lags (fft.jl:96-103 restated on the frame: the
    axis-aligned ball on x' = R^T (x - c))."""
    cent = offt.grid_centroids(dims, spacing=spacing)
    center = tuple(x // 2 for x in dims)
    ci = np.ravel_multi_index(tuple(c - 1 for c in center)[::-1], dims[::-1])
    fc = frame(cent, R)
    C_ = cov_pairwise(Variogram(kind, radii=radii, **kw), fc[ci:ci + 1], fc)[0].reshape(dims[::-1])
    F = np.sqrt(np.abs(np.fft.fftn(np.fft.fftshift(C_))))
    F.flat[0] = 0.0
    return F


@pytest.mark.parametrize("dims,spacing", [((32, 16, 16), (1.0, 1.5, 0.5)), ((24, 18, 12), (1.0, 1.0, 2.0)),
                                          ((15, 13, 11), (1.0, 1.0, 1.0)), ((64, 48), (0.5, 1.0))])
def test_fftgs_spectrum_at_rotated_lags(dims, spacing):
    from gss.engine import FFTGSHandle
    d = len(dims)
    r, R = RADII[d], ROT[d]
    kw = dict(sill=1.7, nugget=0.2)
    h = FFTGSHandle(_g("exponential", r, R, **kw), dims, spacing)
    F = h.spectrum()
    ref = _rotated_spectrum("exponential", dims, spacing, r, R, **kw).ravel()
    assert F[0] == 0.0 and np.max(np.abs(F - ref)) < 1e-12 * np.max(ref)
    # the identity rotation is the axis-aligned spectrum, bit for bit
    assert np.array_equal(FFTGSHandle(_g("exponential", r, np.eye(d), **kw), dims, spacing).spectrum(),
                          FFTGSHandle(_g("exponential", r, **kw), dims, spacing).spectrum())
    h.close()


def test_fftgs_conditional_with_a_rotated_variogram():
    import gss
    from oracle import philox
    coords = np.array([(25.0, 25.0), (50.0, 75.0), (75.0, 50.0)]) * 0.4
    vals = [1.0, -1.0, 1.0]
    r, R = (16.0, 5.0), R2
    problem = gss.SimulationProblem(gss.georef({"z": vals}, coords), gss.CartesianGrid(40, 40), ("z", float), 3)
    sol = gss.solve(problem, gss.FFTGS(("z", dict(variogram=_g("spherical", r, R), mean=0.2)), rng=2022))
    ovg = Variogram("spherical", radii=r)
    pre = offt.preprocess(ovg, (40, 40), mean=0.2, data_coords=coords, data_vals=vals)   # data cells: raw frame
    pre.F = _rotated_spectrum("spherical", (40, 40), None, r, R)
    cent = offt.grid_centroids((40, 40))
    fcent, fd = frame(cent, R, c=coords[0]), frame(coords, R)
    zbar = offt._krige(ovg, 0.2, fd, np.array(vals), fcent, pre.krig)
    kr, pre.krig = pre.krig, None
    for i in range(3):
        zu = offt.solvesingle(pre, philox.uniform(2022, i, 1600))
        zbar_u = offt._krige(ovg, 0.2, fcent[pre.dinds], zu[pre.dinds], fcent, kr)
        assert np.max(np.abs(sol[i].z - (zbar + (zu - zbar_u)))) < 1e-8
