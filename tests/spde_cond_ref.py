"""numpy restatement of SPDEGS with data (gss.h, "SPDEGS with data"), on top of tests/spde_ref.py: the dense formulas
of simple kriging, conditioning by kriging in the data space on the host CG, the brute-force point location and the
observation sets the SPDE conditioning tests share."""
import functools
import math

import numpy as np

import spde_ref as R

EPS = R.EPS
MODES = ("element", "point")
NOBS = {"jitter": 12, "sphere": 10, "fan": 5, "strip": 1}      # never a multiple of the block width (8, 16 or 32)
MEAN = 0.3                                                     # the known field mean of every shared case


# ---- dense formulas --------------------------------------------------------------------------------------------------
def prior_cov(name, lumped):
    """Covariance of the vertex field: inv(A'A / tau^2) as spde.jl forms it, tau^2 inv(S) M inv(S) for the lumped noise."""
    V, T, sill, rng = R.mesh(name)
    _, m, S, tau2 = R.dense(name)
    if not lumped:
        return R.reference_cov(V, T, sill, rng)
    Si = np.linalg.inv(S)
    return tau2 * Si @ np.diag(m) @ Si


def dense_P(nv, idx, w):
    """The observation matrix (nd, nv) of rows idx (nd, 3) / w (nd, 3); a vertex named twice gets both weights."""
    P = np.zeros((len(idx), nv))
    for i in range(len(idx)):
        for k in range(3):
            P[i, idx[i, k]] += w[i, k]
    return P


def dense_kriging(Sigma, P, rvar, y, mu):
    """K = Sigma P' inv(P Sigma P' + R), the mean mu + K (y - mu), the posterior Sigma - K P Sigma, and C."""
    C = P @ Sigma @ P.T + np.diag(rvar)
    K = np.linalg.solve(C, P @ Sigma).T
    return K, mu + K @ (y - mu), Sigma - K @ P @ Sigma, C


def bound(rtol, S, C, Sigma):
    """The covariance bound of tests/test_gpu_spde.py carried through the data-space solve."""
    return 8.0 * rtol * np.linalg.cond(S) * (1.0 + np.linalg.cond(C)) * np.max(np.abs(Sigma))


# ---- the algorithm on the host CG ------------------------------------------------------------------------------------
class Conditioned:
    """W = inv(S) P', C = W' diag(s^2) W + diag(r) and its factor; then the mean and realisations, every solve by R.cg."""

    def __init__(self, S, s, idx, w, y, rvar, mu, rtol):
        self.S, self.s, self.y, self.rvar, self.mu, self.rtol = S, s, y, rvar, mu, rtol
        self.P = dense_P(len(s), idx, w)
        self.W, self.iters = R.cg(S, self.P.T.copy(), rtol)
        self.C = self.W.T @ (s[:, None] ** 2 * self.W) + np.diag(rvar)
        self.L = np.linalg.cholesky(self.C)

    def _csolve(self, b):
        return np.linalg.solve(self.L.T, np.linalg.solve(self.L, b))

    def _correct(self, res):
        return R.cg(self.S, self.s ** 2 * (self.W @ self._csolve(res)), self.rtol)[0]

    def mean(self):
        return self.mu + self._correct(self.y - self.mu)

    def realize(self, wfield, werr):
        """One realisation from nv field normals and nd error normals -> (x_c, x_u)."""
        xu = R.cg(self.S, self.s * wfield, self.rtol)[0]
        e = np.sqrt(self.rvar) * werr
        return (xu + self._correct(self.y - self.mu - self.P @ xu - e)) + self.mu, xu


# ---- point location ----------------------------------------------------------------------------------------------------
def barycentric(P, p):
    """(weights, distance from the plane, edge length scale) of p in the triangle with corners P (3, 3): signed area
    ratios relative to P[0], every product and sum rounded on its own as on the device."""
    u, v, w = P[1] - P[0], P[2] - P[0], p - P[0]

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    n = cross(u, v)
    nn = dot(n, n)
    l1, l2 = dot(cross(w, v), n) / nn, dot(cross(u, w), n) / nn
    return np.array([(1.0 - l1) - l2, l1, l2]), abs(dot(w, n)) / math.sqrt(nn), math.sqrt(math.sqrt(nn))


def locate(V, T, pts, tol=1e-9):
    """Brute force: for every point the nearest triangle (distance to its plane; at most tol edge lengths counts as
    zero) whose barycentric coordinates lie in [-tol, 1 + tol], the lowest index among equally near ones; -1 for none."""
    V3 = np.zeros((len(V), 3))
    V3[:, :V.shape[1]] = V
    tri, wts = np.full(len(pts), -1, dtype=np.int64), np.zeros((len(pts), 3))
    for i, p in enumerate(pts):
        p3 = np.zeros(3)
        p3[:len(p)] = p
        best = None
        for t, ids in enumerate(T):
            l, d, length = barycentric(V3[ids], p3)
            d = 0.0 if d <= tol * length else d
            if (l >= -tol).all() and (l <= 1.0 + tol).all() and (best is None or d < best):
                best, tri[i], wts[i] = d, t, l
    return tri, wts


# ---- shared cases ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, mode):
    """(triangles (nd,), idx (nd, 3), w (nd, 3), y (nd,), points (nd, dim)) of a shared mesh: NOBS[name] triangles drawn
    without replacement by default_rng(3); "element": the triangle's value (weights 1/3, the point is the centroid),
    "point": a Dirichlet point inside it."""
    V, T, sill, _ = R.mesh(name)
    g = np.random.default_rng(3)
    nd = NOBS[name]
    tri = g.choice(len(T), size=nd, replace=False)
    w = g.dirichlet(np.ones(3), size=nd)
    y = MEAN + sill * g.normal(size=nd)
    if mode == "element":
        w = np.full((nd, 3), 1.0 / 3.0)
    idx = T[tri]
    pts = np.einsum("ik,ikd->id", w, V[idx])
    out = (tri, idx, w, y, pts)
    for a in out:
        a.setflags(write=False)
    return out


def error_variance(name, noisy):
    """R = 0 or R = 0.01 sill^2, per observation."""
    sill = R.mesh(name)[2]
    return np.full(NOBS[name], 0.01 * sill * sill if noisy else 0.0)


def conditioned(name, mode, lumped, noisy, rtol):
    """The host algorithm on a shared case."""
    _, m, S, tau2 = R.dense(name)
    _, idx, w, y, _ = case(name, mode)
    return Conditioned(S, R.rhs_scale(m, tau2, lumped), idx, w, y, error_variance(name, noisy), MEAN, rtol)
