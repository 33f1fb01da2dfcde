"""Exactly solvable kriging problems for the kernel matrix (tests/kernel_cases.py) and their 40-digit answers.

Decoupled clusters: the samples sit in clusters of 2-4 points (lags 0.05 .. 0.9 of the range inside a cluster) and the
clusters lie farther apart than the distance at which the model's covariance is exactly 0 in double arithmetic (the
range for the compact models, the underflow of exp for the others).  C is then block diagonal with exact zeros, and the
ordinary / universal kriging system is a sum of tiny solves that mpmath does at 50 digits from the very doubles the
device receives.  Every block enters the answer through F'C^-1.

Geometry: a home cluster at the origin (the estimation points lie about it) and, in 2-D / 3-D, the other clusters on a
circle about it, their members along the radius.  All ring members then lie in a shell a fraction of the range thick,
and the distance order of the neighbour search interleaves them: the members of one cluster are about (number of
clusters) places apart, so the non-zero entries of C fall into off-diagonal 16 x 16 tiles.  On a line (1-D) only the
two clusters at either side of the origin interleave.

The formulas are the textbook definitions oracle/variogram.py states; nothing here calls the oracle or the device.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import mpmath as mp
import numpy as np

mp.mp.dps = 50

SILL, NUGGET = 1.5, 0.1875          # both exact in binary; the nugget makes C(0) differ from the limit of C(h)
RANGE = 8.0                         # isotropic cases
RADII = {2: (16.0, 8.0), 3: (16.0, 8.0, 12.0)}      # MetricBall cases (range 1): unequal radii, the first a power of 2
GAUSSIAN_NUGGET_EPS = 1e-6          # gss.variograms / oracle.variogram: the Gaussian model is evaluated with nugget + 1e-6

COMPACT = ("spherical", "cubic", "pentaspherical")
# model -> (kind of gss / oracle, Matern order)
MODELS = {"gaussian": ("gaussian", 1.0), "exponential": ("exponential", 1.0), "spherical": ("spherical", 1.0),
          "matern12": ("matern", 0.5), "matern32": ("matern", 1.5), "matern52": ("matern", 2.5),
          "cubic": ("cubic", 1.0), "pentaspherical": ("pentaspherical", 1.0)}


def _exp_scale(model):
    """a with C(x) ~ exp(-a x) (x = lag / range) for the models that vanish by underflow; None for the others."""
    if model == "exponential":
        return 3.0
    if model.startswith("matern"):
        return 3.0 * math.sqrt(2.0 * MODELS[model][1])
    return None


UNDERFLOW = 745.14                  # exp(-x) is 0 in double arithmetic from here on


def separation(model):
    """Lag / range beyond which two clusters are taken apart: C is exactly 0 in double arithmetic there."""
    if model in COMPACT:
        return 1.25
    if model == "gaussian":
        return 17.0                 # 3 * 17^2 = 867
    return 300.0                    # exp(-900) and below, whatever polynomial multiplies it


def cutoff(model):
    """Lag / range beyond which the reference takes C = 0: exact for the compact models, below 1e-350 otherwise."""
    if model in COMPACT:
        return 1.0
    if model == "gaussian":
        return 16.5
    return 270.0


def underflow_lag(model):
    """Lag / range at which the model's exponential underflows."""
    if model == "gaussian":
        return math.sqrt(UNDERFLOW / 3.0)
    return UNDERFLOW / _exp_scale(model)


@dataclass(frozen=True)
class Problem:
    model: str
    dim: int
    ball: bool
    variant: str                    # "OK" or "UK" (degree 1)
    x: np.ndarray                   # n x dim samples
    z: np.ndarray                   # nb x n data vectors (row 0 is the one the single-vector paths use)
    x0: np.ndarray                  # m x dim estimation points
    clusters: Tuple[np.ndarray, ...]   # index sets, a partition of range(n)
    block: Optional[Tuple[Tuple[float, ...], int]] = None    # (cell, nsub) of block support

    @property
    def lengths(self):
        return np.asarray(RADII[self.dim] if self.ball else (RANGE,) * self.dim)

    @property
    def sill(self):
        return SILL

    @property
    def eff_nugget(self):
        return NUGGET + (GAUSSIAN_NUGGET_EPS if self.model == "gaussian" else 0.0)


def lag(p, a, b):
    """Lag / range between rows of a and b (|a| x |b|) in double arithmetic: for the geometry checks only."""
    d = (a[:, None, :] - b[None, :, :]) / p.lengths[None, None, :]
    return np.sqrt(np.sum(d * d, axis=-1))


def build(model, dim, n, ball=False, variant="OK", nb=1, block=False, seed=0):
    """The problem of one table entry: n samples in decoupled clusters and the estimation points the issue lists."""
    assert not (ball and dim == 1)
    L = np.asarray(RADII[dim] if ball else (RANGE,) * dim)
    a = float(L.max())
    S = separation(model)
    Sp = (S + 2.0) * a                                   # raw distance between cluster centres: members reach 0.75 a
    nh = {0: 3, 1: 4, 2: 2}[n % 3] if n >= 4 else n      # home cluster; the others have 3 members
    ncl = (n - nh) // 3
    step = np.array([0.17, 0.13, 0.11])[:dim] * L        # home members on a diagonal: lag 0.17 .. 0.24 per step
    pts = [j * step for j in range(nh)]
    clusters = [np.arange(nh)]
    ell = 0.14 * a                                       # member spacing along the radius
    if dim == 1:
        for i in range(ncl):
            side = 1.0 if i % 2 == 0 else -1.0
            r = (i // 2 + 2.5) * Sp + (0.0 if side > 0 else 0.5 * ell)
            clusters.append(np.arange(len(pts), len(pts) + 3))
            pts += [np.array([side * (r + j * ell)]) for j in range(3)]
    else:
        D = max(1.1 * ncl * Sp / (2.0 * math.pi), 2.5 * Sp)
        for i in range(ncl):
            th = 2.0 * math.pi * i / max(ncl, 1) + 0.1
            u = np.array([math.cos(th), math.sin(th), 0.25 * math.sin(5.0 * th)])[:dim]
            c = D * np.array([math.cos(th), math.sin(th), 0.0])[:dim]
            if dim == 3:
                c[2] = 0.3 * a * math.sin(7.0 * th)
            clusters.append(np.arange(len(pts), len(pts) + 3))
            pts += [c + j * ell * u for j in range(3)]
    x = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(n, dim))
    rng = np.random.default_rng(1000 + seed)
    z = rng.normal(size=(nb, n))

    e0 = np.zeros(dim)
    e0[0] = 1.0
    x0 = [np.array([0.31, 0.17, -0.11])[:dim] * L,       # a moderate lag from every home member
          x[1].copy()]                                   # on a sample: C(0) = sill, nugget included
    if model in COMPACT:
        x0 += [L[0] * (1.0 - 2.0 ** -40) * e0, L[0] * e0, L[0] * (1.0 + 2.0 ** -40) * e0]
    else:
        x0 += [1e-9 * L[0] * e0, underflow_lag(model) * L[0] * e0]
    x0 += [np.array([-0.23, 0.41, 0.19])[:dim] * L, np.array([0.52, -0.37, 0.29])[:dim] * L,
           x[0] + 0.5 * step]
    x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(-1, dim))
    p = Problem(model, dim, ball, variant, x, z, x0, tuple(clusters),
                ((tuple(float(0.25 * v) for v in L[:dim]), 2) if block else None))
    _check_geometry(p)
    return p


def _check_geometry(p):
    h = lag(p, p.x, p.x)
    same = np.zeros(h.shape, dtype=bool)
    for c in p.clusters:
        same[np.ix_(c, c)] = True
        if len(c) > 1:
            hc = h[np.ix_(c, c)][~np.eye(len(c), dtype=bool)]
            assert hc.min() >= 0.05 and hc.max() <= 0.9, (hc.min(), hc.max())
    assert h[~same].min() > separation(p.model), h[~same].min()
    # every estimation point (the sub-cell centres of a block included: 0.25 of a length) sees the home cluster only
    h0 = lag(p, p.x0, p.x)
    far = np.ones(h0.shape, dtype=bool)
    far[:, p.clusters[0]] = False
    assert h0[far].min() > separation(p.model) + 1.0, h0[far].min()


# ---------------------------------------------------------------------------------------------------------------------
# 50-digit reference
# ---------------------------------------------------------------------------------------------------------------------
def _corr(model, xr):
    """Correlation at lag / range xr > 0 (mpf)."""
    if model == "gaussian":
        return mp.exp(-3 * xr * xr)
    if model == "exponential":
        return mp.exp(-3 * xr)
    if model == "spherical":
        return 1 - (mp.mpf(3) / 2 * xr - xr ** 3 / 2) if xr < 1 else mp.mpf(0)
    if model == "cubic":
        return 1 - (7 * xr ** 2 - mp.mpf(35) / 4 * xr ** 3 + mp.mpf(7) / 2 * xr ** 5 - mp.mpf(3) / 4 * xr ** 7) \
            if xr < 1 else mp.mpf(0)
    if model == "pentaspherical":
        return 1 - (mp.mpf(15) / 8 * xr - mp.mpf(5) / 4 * xr ** 3 + mp.mpf(3) / 8 * xr ** 5) if xr < 1 else mp.mpf(0)
    nu = MODELS[model][1]
    d = mp.sqrt(2 * mp.mpf(nu)) * 3 * xr
    if nu == 0.5:
        return mp.exp(-d)
    if nu == 1.5:
        return (1 + d) * mp.exp(-d)
    if nu == 2.5:
        return (1 + d + d * d / 3) * mp.exp(-d)
    raise ValueError(model)


def cov_mp(p, a, b):
    """C between two points given as rows of doubles: sill at zero lag, (sill - nugget) * correlation otherwise."""
    L = p.lengths
    s = mp.mpf(0)
    for k in range(p.dim):
        t = (mp.mpf(float(a[k])) - mp.mpf(float(b[k]))) / mp.mpf(float(L[k]))
        s += t * t
    if s == 0:
        return mp.mpf(p.sill)
    return (mp.mpf(p.sill) - mp.mpf(p.eff_nugget)) * _corr(p.model, mp.sqrt(s))


def cov_rows_mp(p, pts):
    """|pts| x n list of rows of C(pt, x_j); entries beyond the cutoff are 0 (module docstring of `cutoff`)."""
    near = lag(p, pts, p.x) <= cutoff(p.model) * (1.0 + 1e-9)
    zero = mp.mpf(0)
    return [[cov_mp(p, pts[i], p.x[j]) if near[i, j] else zero for j in range(p.x.shape[0])]
            for i in range(pts.shape[0])]


def _drift_row(p, pt):
    one = [mp.mpf(1)]
    return one + [mp.mpf(float(v)) for v in pt] if p.variant == "UK" else one


def _block_points(p, pt):
    """Sub-cell centres of the cell about pt (first axis slowest), in the double arithmetic of the definition: with
    nsub = 2 and cells that are powers of two times the lengths every product is exact, so any evaluation order and
    any contraction give these doubles."""
    cell, nsub = p.block
    t = (np.arange(nsub) + 0.5) / nsub - 0.5
    grids = np.meshgrid(*[t * cell[k] for k in range(p.dim)], indexing="ij")
    return pt[None, :] + np.stack([g.ravel() for g in grids], axis=1)


def reference(p):
    """(mean [nb x m], var [m], c0 [m x n]) as float64 arrays rounded from the 50-digit solution, c0 being the
    point-support covariances C(x0, x) (the anchor of the pairwise covariance)."""
    n, m, nb = p.x.shape[0], p.x0.shape[0], p.z.shape[0]
    F = [_drift_row(p, p.x[j]) for j in range(n)]
    nc = len(F[0])
    inv = []
    for c in p.clusters:
        Cb = mp.matrix(len(c), len(c))
        for i, a in enumerate(c):
            for j, b in enumerate(c):
                Cb[i, j] = cov_mp(p, p.x[a], p.x[b])
        inv.append(mp.inverse(Cb))
    # A = C^-1 F, W = C^-1 Z, S = F'A, G = F'W
    A = [[mp.mpf(0)] * nc for _ in range(n)]
    W = [[mp.mpf(0)] * nb for _ in range(n)]
    for c, Ci in zip(p.clusters, inv):
        for i, a in enumerate(c):
            for j, b in enumerate(c):
                for q in range(nc):
                    A[a][q] += Ci[i, j] * F[b][q]
                for q in range(nb):
                    W[a][q] += Ci[i, j] * mp.mpf(float(p.z[q, b]))
    S = mp.matrix(nc, nc)
    G = mp.matrix(nc, nb)
    for j in range(n):
        for q in range(nc):
            for r in range(nc):
                S[q, r] += F[j][q] * A[j][r]
            for r in range(nb):
                G[q, r] += F[j][q] * W[j][r]
    Sinv = mp.inverse(S)
    c0_point = cov_rows_mp(p, p.x0)
    mean = np.empty((nb, m))
    var = np.empty(m)
    for i in range(m):
        if p.block is None:
            c0, f0, c00 = c0_point[i], _drift_row(p, p.x0[i]), mp.mpf(p.sill)
        else:
            sub = _block_points(p, p.x0[i])
            rows = cov_rows_mp(p, sub)
            ns = len(rows)
            c0 = [sum(r[j] for r in rows) / ns for j in range(n)]
            f0 = [sum(_drift_row(p, s)[q] for s in sub) / ns for q in range(nc)]
            c00 = sum(cov_mp(p, s, t) for s in sub for t in sub) / (ns * ns)
        nz = [j for j in range(n) if c0[j] != 0]
        t = mp.matrix(nc, 1)
        for q in range(nc):
            t[q] = sum(A[j][q] * c0[j] for j in nz) - f0[q]
        nu = Sinv * t
        quad = mp.mpf(0)
        for c, Ci in zip(p.clusters, inv):
            if any(c0[a] != 0 for a in c):
                for ii, a in enumerate(c):
                    for jj, b in enumerate(c):
                        quad += c0[a] * Ci[ii, jj] * c0[b]
        v = c00 - quad + sum(t[q] * nu[q] for q in range(nc))
        var[i] = float(v) if v > 0 else 0.0
        for b in range(nb):
            mean[b, i] = float(sum(W[j][b] * c0[j] for j in nz) - sum(G[q, b] * nu[q] for q in range(nc)))
    return mean, var, np.array([[float(v) for v in row] for row in c0_point])


UNIT = 2.0 ** -53 * SILL            # the errors below are counted in these


def units(got, ref):
    """Largest |got - ref| in units of 2^-53 sill (inf for a NaN)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float("inf") if np.any(np.isnan(d)) else float(d.max() / UNIT)


# ---------------------------------------------------------------------------------------------------------------------
# the three evaluations of a table entry: problem, FP64 oracle, device
# ---------------------------------------------------------------------------------------------------------------------
def problem_of(case, seed=0):
    n = case.k if case.k is not None else case.n
    return build(case.model, case.dim, n, ball=case.ball, variant=case.variant, nb=max(case.batch, 1),
                 block=case.block, seed=seed)


def oracle_run(p, case):
    """(mean [nb x m], var [m], c0 [m x n]) of oracle.kriging / oracle.variogram in FP64."""
    from oracle import kriging as K
    from oracle.variogram import Variogram, cov_pairwise
    kind, nu = MODELS[p.model]
    vg = Variogram(kind, sill=SILL, nugget=NUGGET, range=RANGE, nu=nu, radii=RADII[p.dim] if p.ball else None)
    variant, degree = (K.UK, 1) if p.variant == "UK" else (K.OK, None)
    means = []
    for b in range(p.z.shape[0]):
        if case.k is None:
            mu, var = K.exactsolve(variant, vg, p.x, p.z[b], p.x0, degree=degree, support=p.block)
        else:
            mu, var, st = K.approxsolve(variant, vg, p.x, p.z[b], p.x0, case.k, degree=degree)
            assert not st.any()
        means.append(mu)
    return np.asarray(means), var, cov_pairwise(vg, p.x0, p.x)


def device_model(p):
    import gss
    kind, nu = MODELS[p.model]
    ctor = {"gaussian": gss.GaussianVariogram, "exponential": gss.ExponentialVariogram,
            "spherical": gss.SphericalVariogram, "matern": gss.MaternVariogram, "cubic": gss.CubicVariogram,
            "pentaspherical": gss.PentasphericalVariogram}[kind]
    kw = {"sill": SILL, "nugget": NUGGET}
    if kind == "matern":
        kw["order"] = nu
    if p.ball:
        return ctor(gss.MetricBall(RADII[p.dim]), **kw)
    return ctor(range=RANGE, **kw)


def device_run(p, case):
    """(mean [nb x m], var [m] or None, c0 [m x n], status [m], neighbour counts [m] or None) through gss.engine."""
    from gss.engine import OK, UK, HipEngine, KrigHandle
    vg = device_model(p)
    variant, degree = (UK, 1) if p.variant == "UK" else (OK, 0)
    c0 = np.asarray(HipEngine.cov_pairwise(vg, p.x0, p.x))
    h = KrigHandle(vg, variant, p.x, p.z[0], degree=degree, factor=case.k is None)
    try:
        if case.k is not None:
            mu, var, st, idx, cnt = h.predict_knn(p.x0, case.k, return_idx=True)
            assert all(sorted(row) == list(range(case.k)) for row in np.asarray(idx).tolist())
            return np.asarray(mu)[None, :], np.asarray(var), c0, np.asarray(st), np.asarray(cnt)
        if case.batch:
            # the batched means (no variances), and the single-vector path on the same system for variance and status
            out = np.asarray(h.predict_global_batch(p.x0, p.z))
            mu, var, st = h.predict_global(p.x0)
            assert np.array_equal(np.isnan(out[0]), np.isnan(np.asarray(mu)))
            return out, np.asarray(var), c0, np.asarray(st), None
        if case.block:
            h.set_block_support(p.block[0], p.block[1])
        mu, var, st = h.predict_global(p.x0)
        return np.asarray(mu)[None, :], np.asarray(var), c0, np.asarray(st), None
    finally:
        h.close()
