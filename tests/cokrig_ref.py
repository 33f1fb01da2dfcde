"""Cokriging under a linear model of coregionalisation in plain numpy (FP64), written from the convention stated in
include/gss.h (gss_cokrig_create); it does not call the library.

    C_ab(h) = B1[a, b] rho(h) for h != 0,   C_ab(0) = B0[a, b] + B1[a, b]

with rho the correlation of one structure (sill 1, no nugget).  "h = 0" is decided on the coordinates in the frame of
the structure: the squared distance ((D0 D0) + (D1 D1)) + (D2 D2) of the scaled differences, one rounding per
operation, being exactly zero.  The stacked system of the n samples keeps the caller's row order; the ordinary variant
appends one indicator column per variable, the simple variant kriges the residuals about the known means.
"""
import numpy as np


def frame_coords(x, radii=None, rotation=None, origin=None):
    """Coordinates in the frame of the ball, (R^T (x - c)) / radii with c the first SAMPLE (gss.h, rotation); without a
    ball the coordinates as they are."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if radii is None:
        return x
    y = x
    if rotation is not None:
        R = np.asarray(rotation, dtype=np.float64)
        y = (x - np.asarray(origin, dtype=np.float64)) @ R          # rows: R^T (x - c)
    return y / np.asarray(radii, dtype=np.float64)


def sqdist(a, b):
    """Squared distances, accumulated axis by axis with one rounding per operation (numpy never fuses)."""
    d2 = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        t = a[:, None, k] - b[None, :, k]
        d2 = d2 + t * t
    return d2


def rho(kind, h, rng=1.0, nu=1.0):
    """Correlation of the structure at distance h > 0 (the formulas of gss.h / DESIGN.md: practical range)."""
    x = h / rng
    if kind == "exponential":
        return np.exp(-3.0 * x)
    if kind == "gaussian":
        return np.exp(-3.0 * x * x)
    if kind == "spherical":
        return np.where(x < 1.0, 1.0 - (1.5 * x - 0.5 * x ** 3), 0.0)
    if kind == "matern" and nu == 0.5:
        return np.exp(-np.sqrt(2.0 * nu) * 3.0 * x)
    if kind == "matern" and nu == 1.5:
        d = np.sqrt(2.0 * nu) * 3.0 * x
        return (1.0 + d) * np.exp(-d)
    if kind == "matern" and nu == 2.5:
        d = np.sqrt(2.0 * nu) * 3.0 * x
        return (1.0 + d + d * d / 3.0) * np.exp(-d)
    raise ValueError(f"no reference for {kind} (order {nu})")


class Model:
    """structure: dict(kind=, range=, nu=, radii=, rotation=); B0, B1: nz x nz."""

    def __init__(self, structure, B0, B1):
        self.s = dict(kind="exponential", range=1.0, nu=1.0, radii=None, rotation=None)
        self.s.update(structure)
        self.B0 = np.atleast_2d(np.asarray(B0, dtype=np.float64))
        self.B1 = np.atleast_2d(np.asarray(B1, dtype=np.float64))
        self.nz = self.B1.shape[0]

    def cov(self, xa, va, xb, vb, origin):
        """C_{va_i vb_j}(xa_i, xb_j), blockwise by variable ids."""
        fa = frame_coords(xa, self.s["radii"], self.s["rotation"], origin)
        fb = frame_coords(xb, self.s["radii"], self.s["rotation"], origin)
        d2 = sqdist(fa, fb)
        zero = d2 == 0.0
        rng = 1.0 if self.s["radii"] is not None else self.s["range"]
        r = rho(self.s["kind"], np.sqrt(np.where(zero, 1.0, d2)), rng, self.s["nu"])
        b1 = self.B1[np.ix_(va, vb)]
        return np.where(zero, self.B0[np.ix_(va, vb)] + b1, b1 * r)


def system(model, x, var, variant, origin=None):
    """The full constrained matrix ((n + nc)^2) of the stacked samples.  `origin`: of the frame (the first sample of
    the full set; a refit on fewer samples keeps it, as the handle does)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    var = np.asarray(var)
    n = x.shape[0]
    C = model.cov(x, var, x, var, x[0] if origin is None else origin)
    if variant == "simple":
        return C
    F = (var[:, None] == np.arange(model.nz)[None, :]).astype(np.float64)
    K = np.zeros((n + model.nz, n + model.nz))
    K[:n, :n] = C
    K[:n, n:] = F
    K[n:, :n] = F.T
    return K


def predict(model, x, z, var, xdom, variant="ordinary", means=None, origin=None):
    """-> mean[nz, m], variance[nz, m]: one numpy.linalg.solve per target."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    xdom = np.asarray(xdom, dtype=np.float64)
    if xdom.ndim == 1:
        xdom = xdom[:, None]
    var = np.asarray(var)
    z = np.asarray(z, dtype=np.float64)
    origin = x[0] if origin is None else origin
    n, m, nz = x.shape[0], xdom.shape[0], model.nz
    K = system(model, x, var, variant, origin)
    mu0 = np.zeros(nz)
    if variant == "simple" and means is not None:
        mu0 = np.array(np.broadcast_to(np.asarray(means, dtype=np.float64), (nz,)))
    resid = z - mu0[var]
    mean, varc = np.empty((nz, m)), np.empty((nz, m))
    for t in range(nz):
        rhs = model.cov(x, var, xdom, np.full(m, t), origin)
        if variant != "simple":
            rhs = np.vstack([rhs, (np.arange(nz)[:, None] == t) * np.ones((1, m))])
        lam = np.linalg.solve(K, rhs)
        mean[t] = mu0[t] + lam[:n].T @ resid
        varc[t] = (model.B0[t, t] + model.B1[t, t]) - np.sum(lam * rhs, axis=0)
    return mean, np.maximum(varc, 0.0)


def cross_validate(model, x, z, var, fold=None, variant="ordinary", means=None):
    """Every sample i predicted (as variable var_i) by a refit without the samples of its fold (None: itself only).
    -> pred[n], variance[n]"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    var, z = np.asarray(var), np.asarray(z, dtype=np.float64)
    n = x.shape[0]
    fold = np.arange(n) if fold is None else np.asarray(fold)
    pred, pvar = np.empty(n), np.empty(n)
    for f in np.unique(fold):
        out = fold == f
        keep = ~out
        mu, vv = predict(model, x[keep], z[keep], var[keep], x[out], variant, means, origin=x[0])
        idx = np.flatnonzero(out)
        pred[idx] = mu[var[idx], np.arange(idx.size)]
        pvar[idx] = vv[var[idx], np.arange(idx.size)]
    return pred, pvar


def cond(model, x, var, variant):
    return float(np.linalg.cond(system(model, x, var, variant)))
