"""Every covariance form of csrc/gss_internal.h at the lags of tests/cov_probe.py, against 50-digit values.

Routes (one sample at the origin, z = 1, simple kriging with known mean 0, so that mean = C(h) / C(0) and
variance = C(0) - C(h)^2 / C(0); module docstring of cov_probe):
  A  HipEngine.cov_pairwise                      cov_pair / vg_shape, every model, nested and Power included
  B  KrigHandle(...).predict_global              krig_rhs2_kernel<DIM, KIND>: vg_shape with the kind fixed at compile time
  C  KrigHandle(..., factor=False).predict_knn   krig_local_mfma_kernel<DIM, KIND, 1>: vg_shape_kpos<KIND, true> for the
                                                 fixed kinds, cov_pair4 / vg_shape4 for every other model; a nested
                                                 model (class "nested") takes vg_shape4's gss_exp_poly branches
  F  CoKrigHandle(B0 = nugget, B1 = sill - nugget, one variable, factor=False).predict_knn(points, (1,))
                                                 cokrig_local_kernel: co_rho1<DIM, KIND> with its own zero-lag select and
                                                 its own fmax(d2, 1e-300), for cov_probe.F_MODELS (the structure's shape
                                                 alone: a Gaussian one without the regularised nugget)
each with the isotropic range and, for cov_probe.BALL_MODELS, the ball of unequal radii (per-axis sca[], sqdist_nofma
with aniso), with and without a nugget.  One device call per model and configuration, all lags as its points.

Error bars: cov_probe.bar, from the figures tools/cov_probe_oracle.py measures on the FP64 oracle and on the float64
transcription of the device's algorithms; none is taken from the device.
"""
import ctypes as C

import numpy as np
import pytest

import cov_probe as cp

pytestmark = pytest.mark.gpu

_DEV = {}


def _configs(m, dim):
    return [(ball, nugget) for ball in ((False, True) if (dim > 1 and m.name in cp.BALL_MODELS) else (False,))
            for nugget in cp.NUGGETS]


def device(route, m, dim, ball, nugget):
    """(covariance (A) or mean, variance or None) of one device call over cp.points(m, dim, ball); kept for the comparison
    of the routes with each other."""
    key = (route, m.name, dim, ball, nugget)
    if key in _DEV:
        return _DEV[key]
    from gss import _lib
    from gss.engine import SK, CoKrigHandle, HipEngine, KrigHandle
    pts, o = cp.points(m, dim, ball), cp.origin(dim)
    if route == "F":
        h = CoKrigHandle(cp.device_model(m, dim, ball, 0.0), [[nugget]], [[cp.SILL - nugget]], SK, o, np.ones(1),
                         np.zeros(1, dtype=np.int32), means=[0.0], factor=False)
        try:
            mu, var, st = h.predict_knn(pts, (1,))
        finally:
            h.close()
        assert not np.asarray(st).any(), (m.name, route, dim, ball, nugget)
        res = (np.asarray(mu)[0], np.asarray(var)[0])
    elif m.kind == "power":
        assert route == "A"
        # the pseudo-covariance A - gamma(h) with the A the front end would choose (gss.h, GSS_VG_POWER)
        A = cp.power_sill(m, dim)
        v = _lib.make_variogram("power", dim, A, nugget, 1.0, m.nu, None)
        out = np.empty((1, len(pts)))
        _lib.check(_lib.lib().gss_cov_pairwise(C.byref(v), _lib.ptr(o), 1, _lib.ptr(pts), len(pts), _lib.ptr(out),
                                               len(pts), _lib.MEM_HOST, _lib.current_stream()))
        res = (out[0], None)
    elif route == "A":
        res = (np.asarray(HipEngine.cov_pairwise(cp.device_model(m, dim, ball, nugget), o, pts))[0], None)
    else:
        h = KrigHandle(cp.device_model(m, dim, ball, nugget), SK, o, np.ones(1), mean=0.0, factor=route == "B")
        try:
            mu, var, st = h.predict_global(pts) if route == "B" else h.predict_knn(pts, 1)
        finally:
            h.close()
        assert not np.asarray(st).any(), (m.name, route, dim, ball, nugget)
        res = (np.asarray(mu), np.asarray(var))
    _DEV[key] = res
    return res


def _describe(m, route, dim, ball, nugget, i, what, got, ref, bar, scale=1.0):
    pts = cp.points(m, dim, ball)
    s = m.terms[0][1] if m.terms else m
    with np.errstate(divide="ignore"):
        arg = cp.shape_arg(s, dim, ball, pts[i:i + 1])[0]
    return ("%s of %s, route %s, %d-D%s, nugget %g: point %r (lag / range %.17g, shape argument %.17g): device %.17g, "
            "reference %.17g, error %.1f units, bar %.1f" %
            (what, m.name, route, dim, " ball" if ball else "", nugget, pts[i].tolist(),
             float(np.sqrt(np.sum((pts[i] / (1.0 if m.kind == "power" else cp.lengths(dim, ball))) ** 2))), arg,
             got[i], ref[i], abs(got[i] - ref[i]) / (2.0 ** -53 * scale), bar))


WORST = {}


def _routes(m):
    if m.kind == "power":
        return ("A",)
    return cp.ROUTES + (("F",) if m.name in cp.F_MODELS else ())


def _bars(m, dim, ball, route, what):
    """The bar of every lag: its class's, or the sub-class's of the lags below the ladder (cov_probe.TINY)."""
    t = cp.tiny(m, dim, ball)
    cls = cp.bar_classes(m.cls)
    return np.where(t, cp.bar(cls[-1], route, what), cp.bar(cls[0], route, what))


def _check(m, route, dim, ball, nugget):
    got, gvar = device(route, m, dim, ball, nugget)
    cov, mean, var = cp.reference_set(m, dim, ball, nugget, raw=route == "F")
    sill = cp.sill_of(m, dim)
    pts = cp.points(m, dim, ball)
    assert len(got) == len(pts)
    zero = np.all(pts == 0.0, axis=1)
    # route A returns C (scale: the sill), the others the mean C / C(0) and the variance (sill 1)
    for what, g, r, scale in (("mean", got, cov if route == "A" else mean, sill if route == "A" else 1.0),
                              ("var", gvar, var, 1.0)):
        if g is None:
            continue
        bars = _bars(m, dim, ball, route, what)
        assert np.all(np.isfinite(g)), _describe(m, route, dim, ball, nugget, int(np.argmin(np.isfinite(g))), what, g, r,
                                                 bars[int(np.argmin(np.isfinite(g)))])
        err = np.abs(g - r) / (2.0 ** -53 * scale)
        for bc, mask in zip(cp.bar_classes(m.cls), (~cp.tiny(m, dim, ball), cp.tiny(m, dim, ball))):
            if mask.any():
                i = int(np.flatnonzero(mask)[np.argmax(err[mask])])
                k = (bc, route, what)
                if err[i] >= WORST.get(k, (-1.0,))[0]:
                    WORST[k] = (float(err[i]), _describe(m, route, dim, ball, nugget, i, what, g, r, bars[i], scale))
        i = int(np.argmax(err - bars))
        assert err[i] <= bars[i], _describe(m, route, dim, ball, nugget, i, what, g, r, bars[i], scale)
        # a zero lag is the sill itself, nugget included (route A: the very double the library was handed; a nested
        # model's is the sum of its contributions in float64, cov_probe.device_sill): mean exactly 1, variance exactly 0
        # (a nested model whose float64 sill is not the double 1, on routes B and C: c0 times the reciprocal of C(0) is
        #  then 1 only to a rounding -- those zero lags are held to the bar above like every other lag)
        if route != "A" and cp.device_sill(m, dim, nugget) != 1.0:
            continue
        want = (cp.device_sill(m, dim, nugget) if route == "A" else 1.0) if what == "mean" else 0.0
        assert np.all(g[zero] == want), _describe(m, route, dim, ball, nugget, int(np.flatnonzero(zero)[0]), what, g, r, 0.0)


PARAMS = [(route, cls, dim) for route in cp.ROUTES + ("F",) for cls in cp.CLASSES for dim in (1, 2, 3)
          if any(route in _routes(m) for m in cp.by_class(cls))]


@pytest.mark.parametrize("route,cls,dim", PARAMS)
def test_form_against_50_digits(route, cls, dim):
    for m in cp.by_class(cls):
        if route in _routes(m):
            for ball, nugget in _configs(m, dim):
                _check(m, route, dim, ball, nugget)
    for k, v in sorted(WORST.items()):
        if k[0] in cp.bar_classes(cls) and k[1] == route:
            print("worst", k, "%.1f" % v[0], v[1])


@pytest.mark.parametrize("cls,dim", [(cls, dim) for cls in cp.CLASSES if cls != "power" for dim in (1, 2, 3)])
def test_routes_agree(cls, dim):
    """A form that drifts from the others is caught even where its own bar is wide (route D of the nested class: the
    moving-neighbourhood kernel against the pairwise covariance)."""
    for m in cp.by_class(cls):
        routes = _routes(m)
        for ball, nugget in _configs(m, dim):
            got = {r: device(r, m, dim, ball, nugget) for r in routes}      # (sill 1: route A's C is C / C(0))
            extra = 0.0
            if "F" in routes and m.kind == "gaussian":
                # route F evaluates the shape without the regularised nugget: compared as correlations (no variances),
                # two roundings more
                # (the zero lags, where C is the sill and no correlation, are held exactly by test_form_against_50_digits)
                pos = np.any(cp.points(m, dim, ball) != 0.0, axis=1)
                got = {r: (np.where(pos, g[0] / (cp.SILL - cp.eff_nugget(m, nugget, raw=r == "F")), 1.0), None)
                       for r, g in got.items()}
                extra = 2.0
            pairs = [(a, b) for i, a in enumerate(routes) for b in routes[i + 1:]]
            for a, b in pairs:
                tol = _bars(m, dim, ball, a, "mean") + _bars(m, dim, ball, b, "mean") + extra
                err = np.abs(got[a][0] - got[b][0]) / 2.0 ** -53
                i = int(np.argmax(err - tol))
                assert err[i] <= tol[i], "routes %s and %s: %s" % (
                    a, b, _describe(m, b, dim, ball, nugget, i, "mean", got[b][0], got[a][0], tol[i]))
                if got[a][1] is not None and got[b][1] is not None:
                    tol = _bars(m, dim, ball, a, "var") + _bars(m, dim, ball, b, "var")
                    err = np.abs(got[a][1] - got[b][1]) / 2.0 ** -53
                    i = int(np.argmax(err - tol))
                    assert err[i] <= tol[i], "routes %s and %s: %s" % (
                        a, b, _describe(m, b, dim, ball, nugget, i, "var", got[b][1], got[a][1], tol[i]))


@pytest.mark.parametrize("order", cp.REFUSED_ORDERS)
def test_orders_beyond_the_front_end_are_refused(order):
    """The general-order evaluator is probed up to the largest order the library accepts (50); beyond it a model is
    refused, not evaluated."""
    import gss
    from gss.engine import SK, HipEngine, KrigHandle
    vg = gss.MaternVariogram(range=cp.RANGE, order=order)
    with pytest.raises(gss._lib.GSSError, match="must lie"):
        HipEngine.cov_pairwise(vg, cp.origin(2), cp.points(cp.ALL["matern_40.0"], 2)[:4])
    with pytest.raises(gss._lib.GSSError, match="must lie"):
        KrigHandle(vg, SK, cp.origin(2), np.ones(1), mean=0.0)
