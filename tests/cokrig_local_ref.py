"""Moving-neighbourhood cokriging in plain numpy (FP64), written from the text of include/gss.h
(gss_cokrig_predict_knn); it does not call the library.

Per domain point: the k[a] nearest samples of every variable a, picked by brute force among that variable's samples by
(squared key in the search frame, row index); then one dense solve per target on the selected rows, with the covariances
of cokrig_ref.Model.cov about the frame origin of the FULL sample set.  Under the ordinary variant the constraint of a
variable without neighbours is dropped and such a variable, as a target, is MISSING; under the simple variant every
target is estimated from whatever was found.
"""
import numpy as np

import cokrig_ref as CR

OK_, MISSING, SINGULAR = 0, 1, 2


def _rho_more(kind, x):
    """The models only the general kernel evaluates (formulas of DESIGN.md: practical range 1)."""
    if kind == "cubic":
        return np.where(x < 1.0, 1.0 - (7.0 * x ** 2 - 8.75 * x ** 3 + 3.5 * x ** 5 - 0.75 * x ** 7), 0.0)
    if kind == "pentaspherical":
        return np.where(x < 1.0, 1.0 - (1.875 * x - 1.25 * x ** 3 + 0.375 * x ** 5), 0.0)
    raise ValueError(kind)


class Model(CR.Model):
    """cokrig_ref.Model, plus the cubic and pentaspherical structures."""

    def cov(self, xa, va, xb, vb, origin):
        if self.s["kind"] not in ("cubic", "pentaspherical"):
            return super().cov(xa, va, xb, vb, origin)
        fa = CR.frame_coords(xa, self.s["radii"], self.s["rotation"], origin)
        fb = CR.frame_coords(xb, self.s["radii"], self.s["rotation"], origin)
        d2 = CR.sqdist(fa, fb)
        zero = d2 == 0.0
        rng = 1.0 if self.s["radii"] is not None else self.s["range"]
        r = _rho_more(self.s["kind"], np.sqrt(np.where(zero, 1.0, d2)) / rng)
        b1 = self.B1[np.ix_(va, vb)]
        return np.where(zero, self.B0[np.ix_(va, vb)] + b1, b1 * r)


def search_keys(x, xdom, radius=None, radii=None, rotation=None, origin=None):
    """Squared keys (m x n) in the search frame and the bound a neighbour's key must not exceed (None: no ball)."""
    x = np.asarray(x, dtype=np.float64)
    xdom = np.asarray(xdom, dtype=np.float64)
    if radii is not None:
        R = np.eye(x.shape[1]) if rotation is None else np.asarray(rotation, dtype=np.float64)
        c = np.zeros(x.shape[1]) if rotation is None else np.asarray(origin, dtype=np.float64)
        fa, fb = ((xdom - c) @ R) / np.asarray(radii), ((x - c) @ R) / np.asarray(radii)
        return CR.sqdist(fa, fb), 1.0
    return CR.sqdist(xdom, x), (None if radius is None else float(radius) ** 2)


def select(x, var, xdom, k, radius=None, radii=None, rotation=None):
    """-> idx[m, sum k] (rows of the caller's arrays, -1 padded), count[m, nz]."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    xdom = np.asarray(xdom, dtype=np.float64).reshape(-1, x.shape[1])
    var = np.asarray(var)
    k = [int(v) for v in k]
    m, nz = xdom.shape[0], len(k)
    key, bound = search_keys(x, xdom, radius, radii, rotation, x[0])
    idx = np.full((m, sum(k)), -1, dtype=np.int32)
    count = np.zeros((m, nz), dtype=np.int32)
    off = 0
    for a in range(nz):
        rows = np.flatnonzero(var == a)
        for p in range(m):
            kk = key[p, rows]
            order = np.lexsort((rows, kk))                      # by (key, row)
            if bound is not None:
                order = order[kk[order] <= bound]
            order = order[:k[a]]
            idx[p, off:off + order.size] = rows[order]
            count[p, a] = order.size
        off += k[a]
    return idx, count


def predict(model, x, z, var, xdom, k, variant="ordinary", means=None, minneighbors=1, radius=None, radii=None,
            rotation=None, with_cond=False):
    """-> mean[nz, m], variance[nz, m], status[nz, m], idx, count (and the largest cond_2 of a per-point system)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    xdom = np.asarray(xdom, dtype=np.float64).reshape(-1, x.shape[1])
    var = np.asarray(var)
    z = np.asarray(z, dtype=np.float64)
    nz, m = model.nz, xdom.shape[0]
    idx, count = select(x, var, xdom, k, radius, radii, rotation)
    mu0 = np.zeros(nz)
    if variant == "simple" and means is not None:
        mu0 = np.array(np.broadcast_to(np.asarray(means, dtype=np.float64), (nz,)))
    mean = np.full((nz, m), np.nan)
    varc = np.full((nz, m), np.nan)
    status = np.zeros((nz, m), dtype=np.uint8)
    worst = 0.0
    origin = x[0]
    for p in range(m):
        rows = idx[p][idx[p] >= 0]
        K = rows.size
        if K < max(int(minneighbors), 1):
            status[:, p] = MISSING
            continue
        xs, vs, zs = x[rows], var[rows], z[rows] - mu0[var[rows]]
        C = model.cov(xs, vs, xs, vs, origin)
        present = [a for a in range(nz) if count[p, a] > 0] if variant != "simple" else []
        F = (vs[:, None] == np.asarray(present, dtype=int)[None, :]).astype(np.float64)
        A = np.zeros((K + len(present), K + len(present)))
        A[:K, :K] = C
        A[:K, K:] = F
        A[K:, :K] = F.T
        if with_cond:
            worst = max(worst, float(np.linalg.cond(A)))
        for t in range(nz):
            if variant != "simple" and t not in present:
                status[t, p] = MISSING
                continue
            rhs = np.concatenate([model.cov(xs, vs, xdom[p:p + 1], np.array([t]), origin)[:, 0],
                                  [1.0 if a == t else 0.0 for a in present]])
            lam = np.linalg.solve(A, rhs)
            mean[t, p] = mu0[t] + lam[:K] @ zs
            varc[t, p] = max((model.B0[t, t] + model.B1[t, t]) - lam @ rhs, 0.0)
    out = (mean, varc, status, idx, count)
    return out + (worst,) if with_cond else out
