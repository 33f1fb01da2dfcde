"""The references of sequential indicator simulation (gss.h, gss_sis_realize), numpy only.  Test infrastructure.

    walk        the recursion restated sequentially in FP64, in the device's order of operations: per node the K sums by
                fused multiply-add in list order (an error-free product stands in for the fma numpy lacks), the
                order-relation correction or the clipped, renormalised pdf, and the draw at the same uniforms.  It takes the
                neighbour lists and weights it is given (gss_sgs_weights, or cpu_stage_a here), so the search is not restated.
    one_step    on a finished field: for every simulated (node, realisation) the corrected ccdf / the pdf again in
                np.longdouble from the field's own neighbour values, and whether the value in the field is a draw from it at
                the node's uniform.  The bar per node, 4 (ncond + 2) 2^-53 (1 + sum |w_j|), is the rounding bound of the fma
                chain (ncond terms, each rounded once, growing no further than 1 + sum |w|, plus the final sum) with a
                factor 4 for the clip, the renormalisation and the cumulation.  Derived, not measured.
    close_calls the draws of `walk` that a rounding could turn: u within the bar of a cumulative boundary, or (continuous)
                a value within 1e-9 (zmax - zmin) of a cutoff.  tests/test_sis_host.py shows there are none in any run of
                tests/sis_cases.py, so the device is compared with `walk` without exclusions.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LD = np.longdouble
UNIT = 2.0 ** -53


# ---- the inputs of a run (tests/sis_cases.py) ----------------------------------------------------------------------------
def geometry(run):
    """Everything a run is built from, a function of the run alone: jittered cell centres (no two search keys tie),
    paths (npaths, N), data cells and values, the draw rule and the uniforms (R, N) of the run's seed."""
    from oracle import philox
    from oracle.fftgs import grid_centroids
    N = int(np.prod(run.dims))
    rng = np.random.default_rng([N, run.k, run.K, run.nd, int(run.categorical)])
    cent = grid_centroids(run.dims) + rng.uniform(-0.3, 0.3, (N, len(run.dims)))
    dl = np.sort(rng.choice(N, run.nd, replace=False)).astype(np.int64)
    paths = np.stack([rng.permutation(N) for _ in range(run.npaths)]).astype(np.int64)
    if run.categorical:
        cut = None
        fs = (1.0 + np.arange(run.K)) / np.sum(1.0 + np.arange(run.K))
        zd = rng.integers(0, run.K, run.nd).astype(np.float64)
        zmin = zmax = 0.0
    else:
        cut = np.array([0.0]) if run.K == 1 else np.linspace(-1.5, 1.5, run.K)
        fs = np.array([0.5 * (1.0 + math.erf(c / math.sqrt(2.0))) for c in cut])
        zd = np.clip(rng.normal(size=run.nd), -3.5, 3.5)
        zmin, zmax = -4.0, 4.0
    U = np.stack([philox.uniform(run.seed, run.first_real + r, N)[:N] for r in range(run.R)])
    return dict(N=N, cent=cent, paths=paths, dl=dl, zd=zd, cut=cut, fs=fs, zmin=zmin, zmax=zmax, U=U)


def variogram_args(run):
    """(kind, range, sill, nugget) of the run's indicator variogram."""
    return ("spherical", 5.0, 1.0, 1.0 if run.nugget_only else 0.1)


def ranks(path, dl, N):
    rk = np.empty(N, dtype=np.int64)
    rk[path] = np.arange(N)
    rk[dl] = -1
    return rk


def cpu_stage_a(run, geo, path):
    """Stage A on the CPU as oracle/sgs.py does it node by node: the k nearest among the cells simulated before the node,
    (key, index) ascending, and the simple-kriging weights by numpy.linalg.  -> idx (N, k), ncond (N), w (N, k)."""
    from oracle.kriging import metric_key
    from oracle.variogram import Variogram, cov_pairwise
    kind, rng_, sill, nugget = variogram_args(run)
    vg = Variogram(kind, sill=sill, nugget=nugget, range=rng_)
    cent, N, k = geo["cent"], geo["N"], run.k
    rk = ranks(path, geo["dl"], N)
    idx = np.full((N, k), -1, dtype=np.int32)
    nc = np.zeros(N, dtype=np.int32)
    w = np.zeros((N, k))
    for node in range(N):
        if rk[node] < 0:
            continue
        cand = np.flatnonzero(rk < rk[node])
        d2 = metric_key(cent[cand], cent[node], None, None)
        nb = cand[np.argsort(d2, kind="stable")[:k]]
        idx[node, :nb.size] = nb
        if nb.size < max(run.nmin, 1):
            continue
        C = cov_pairwise(vg, cent[nb])
        c0 = cov_pairwise(vg, cent[nb], cent[node][None, :])[:, 0]
        L = np.linalg.cholesky(C)
        w[node, :nb.size] = np.linalg.solve(L.T, np.linalg.solve(L, c0))
        nc[node] = nb.size
    return idx, nc, w


# ---- arithmetic ----------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """round(a b + c) for FP64 arrays: Dekker's error-free product, then the sum with its error term."""
    p = a * b
    A, B = 134217729.0 * a, 134217729.0 * b
    ah, bh = A - (A - a), B - (B - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def bar(nc, w):
    """4 (ncond + 2) 2^-53 (1 + sum |w_j|) per node."""
    return 4.0 * (nc + 2.0) * UNIT * (1.0 + np.sum(np.abs(w), axis=-1))


def correct(F):
    """The order-relation correction of gss.h on rows F[..., K]: clip, upward max, downward min, mean of the two."""
    c = np.where(F < 0, 0, np.where(F > 1, 1, F)).astype(F.dtype)
    return (np.maximum.accumulate(c, axis=-1) + np.minimum.accumulate(c[..., ::-1], axis=-1)[..., ::-1]) * F.dtype.type(0.5)


def _pw(x, e):
    return x if e == 1 else x ** e


def quantile(F, u, cut, zmin, zmax, tail):
    """The smallest z with F(z) >= u under the ccdf model of gss_ik_post, rows F[R, K] (corrected), u[R]; in the dtype of
    F, in the device's order of operations."""
    ft = F.dtype.type
    cut = np.asarray(cut).astype(F.dtype)
    zmin, zmax = ft(zmin), ft(zmax)
    ilo, ihi = ft(1.0) / ft(tail[0]), ft(1.0) / ft(tail[1])
    K = cut.size
    F0, Ft = F[:, 0], F[:, K - 1]
    z = np.empty(u.shape, dtype=F.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = u <= F0
        z[lo] = np.where(F0[lo] > 0, zmin + (cut[0] - zmin) * _pw(u[lo] / F0[lo], ilo), zmin)
        hi = ~lo & (u > Ft)
        z[hi] = zmax - (zmax - cut[K - 1]) * _pw((ft(1.0) - u[hi]) / (ft(1.0) - Ft[hi]), ihi)
        todo = ~lo & ~hi
        for q in range(1, K):      # the first class whose upper value reaches u
            m = todo & (u <= F[:, q])
            z[m] = cut[q - 1] + (cut[q] - cut[q - 1]) * ((u[m] - F[m, q - 1]) / (F[m, q] - F[m, q - 1]))
            todo &= ~m
    assert not todo.any()
    return z


def pdf(P, fs):
    """Rows P[R, K] = p* + sums -> (p[R, K], cum[R, K]): clipped, divided by the clipped sum where it is positive (else
    p*), cumulated in category order; sequential sums, in the dtype of P."""
    c = np.where(P < 0, 0, np.where(P > 1, 1, P)).astype(P.dtype)
    s = np.zeros(P.shape[0], dtype=P.dtype)
    for q in range(P.shape[1]):
        s = s + c[:, q]
    ok = s > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(ok[:, None], c / s[:, None], np.asarray(fs).astype(P.dtype)[None, :])
    cum = np.empty_like(p)
    acc = np.zeros(P.shape[0], dtype=P.dtype)
    for q in range(P.shape[1]):
        acc = acc + p[:, q]
        cum[:, q] = acc
    return p, cum


def pick(p, cum, u):
    """The first category with u < cum, else the last one with a positive probability."""
    K = p.shape[1]
    below = u[:, None] < cum
    first = np.where(below.any(axis=1), np.argmax(below, axis=1), -1)
    lastpos = (K - 1) - np.argmax((p > 0)[:, ::-1], axis=1)
    return np.where(first >= 0, first, lastpos)


def _indicators(zn, run, geo):
    """i[R, c, K] of neighbour values zn[R, c]."""
    if run.categorical:
        return (zn[:, :, None] == np.arange(run.K, dtype=np.float64)[None, None, :]).astype(np.float64)
    return (zn[:, :, None] <= geo["cut"][None, None, :]).astype(np.float64)


def blocks(run):
    """[(path, rows of the field)]: a shared order walks every realisation at once; with one order per realisation,
    realisation r of the run walks path first_real - path_base + r."""
    if run.npaths == 1:
        return [(0, slice(0, run.R))]
    return [(run.first_real - run.path_base + r, slice(r, r + 1)) for r in range(run.R)]


def over_blocks(fn, run, geo, stage, *fields):
    """fn(run, geo, path, idx, nc, w, U rows[, field rows]) for every block of the run; `stage`: {path: (idx, nc, w)}."""
    return [fn(run, geo, geo["paths"][p], *stage[p], geo["U"][rows], *(f[rows] for f in fields)) for p, rows in blocks(run)]


# ---- the three references ------------------------------------------------------------------------------------------------
def walk(run, geo, path, idx, nc, w, U, record=None):
    """z[R, N]: the realisations whose uniforms are the rows of U, along `path` with the lists idx / nc / w.  `record`: a
    dict that receives gap[R, N], the distance of u to the nearest cumulative boundary (inf at data cells)."""
    N, R, K, fs = geo["N"], U.shape[0], run.K, geo["fs"]
    rk = ranks(path, geo["dl"], N)
    z = np.array(U, dtype=np.float64)
    z[:, geo["dl"]] = geo["zd"][None, :]
    gap = np.full((R, N), np.inf)
    for node in path:
        if rk[node] < 0:
            continue
        c = int(nc[node])
        ind = _indicators(z[:, idx[node, :c]], run, geo)
        acc = np.zeros((R, K))
        for j in range(c):
            acc = _fma(np.float64(w[node, j]), ind[:, j, :] - fs[None, :], acc)
        u = z[:, node].copy()
        if run.categorical:
            p, cum = pdf(fs[None, :] + acc, fs)
            z[:, node] = pick(p, cum, u)
            bounds = cum
        else:
            F = correct(fs[None, :] + acc)
            z[:, node] = quantile(F, u, geo["cut"], geo["zmin"], geo["zmax"], run.tail)
            bounds = F
        gap[:, node] = np.min(np.abs(u[:, None] - bounds), axis=1)
    if record is not None:
        record["gap"] = gap
    return z


def close_calls(run, geo, path, idx, nc, w, U):
    """The number of (node, realisation) draws of `walk` that a rounding could turn."""
    rec = {}
    z = walk(run, geo, path, idx, nc, w, U, record=rec)
    close = rec["gap"] <= bar(nc, w)[None, :]
    if not run.categorical:
        sim = ranks(path, geo["dl"], geo["N"]) >= 0
        near = np.min(np.abs(z[:, :, None] - geo["cut"][None, None, :]), axis=2) <= 1e-9 * (geo["zmax"] - geo["zmin"])
        close |= near & sim[None, :]
    return int(close.sum())


def one_step(run, geo, path, idx, nc, w, U, z):
    """For every simulated (node, realisation) of the finished field z[R, N]: is the value a draw at u from the ccdf / pdf
    that np.longdouble gives from the field's own neighbour values?  -> (violations, bar[N]).
    Categorical: the category s must satisfy cum_{s-1} - bar <= u < cum_s + bar (or be the fallback of `pick`).
    Continuous: the device's F differ from the long-double ones by at most the bar; inside a class that moves the
    interpolation ratio by at most 2 bar / (F_b - F_a), in a tail the ratio u / F_0 by what moving u by bar does, so the
    value must lie in [Q(u - 2 bar) - ez, Q(u + 2 bar) + ez] with Q the long-double quantile function, which is monotone
    and continuous across class boundaries, and ez = 8 x 2^-53 max(|zmin|, |zmax|) for the roundings of the closing
    formula itself (a quotient, a power of at most 2 ulp, a product, a sum, each relative 2^-53 of at most the range)."""
    N, K = geo["N"], run.K
    rk = ranks(path, geo["dl"], N)
    b = bar(nc, w)
    fs = geo["fs"].astype(LD)
    bad = 0
    for node in np.flatnonzero(rk >= 0):
        c = int(nc[node])
        ind = _indicators(z[:, idx[node, :c]], run, geo).astype(LD)
        acc = np.einsum("j,rjk->rk", w[node, :c].astype(LD), ind - fs[None, None, :]) if c else np.zeros((z.shape[0], K), LD)
        u = U[:, node].astype(LD)
        got = z[:, node]
        if run.categorical:
            p, cum = pdf(fs[None, :] + acc, fs)
            s = got.astype(np.int64)
            ok = (got == s) & (s >= 0) & (s < K)
            s = np.clip(s, 0, K - 1)
            rows = np.arange(z.shape[0])
            lower = np.where(s > 0, cum[rows, np.maximum(s - 1, 0)], LD(0))
            inside = (u >= lower - b[node]) & (u < cum[rows, s] + b[node])
            fallback = (u >= cum[:, K - 1] - b[node]) & (s == pick(p, cum, np.full_like(u, 2)))
            bad += int(np.sum(~(ok & (inside | fallback))))
        else:
            F = correct(fs[None, :] + acc)
            ez = 8.0 * UNIT * max(abs(geo["zmin"]), abs(geo["zmax"]))
            qlo = quantile(F, np.maximum(u - 2 * b[node], LD(0)), geo["cut"], geo["zmin"], geo["zmax"], run.tail)
            qhi = quantile(F, np.minimum(u + 2 * b[node], LD(1)), geo["cut"], geo["zmin"], geo["zmax"], run.tail)
            bad += int(np.sum(~((got >= qlo - ez) & (got <= qhi + ez))))
    return bad, b
