"""CPU reference of gss_idw_cv / gss_lwr_cv (include/gss.h) by refitting: for every fold -- or every sample, for
leave-one-out and leave-ball-out -- oracle.idw_lwr.idw / .lwr is called on the eligible samples only, with the held-out
locations as its domain.  Eligibility is plain numpy from the definition: fold[j] != fold[p] and, with an exclusion
radius, search key(p, j) > exclusion key; on integer lattice coordinates (`lattice=True`) the Euclidean key and the radius
are compared in exact integer arithmetic, as tests/search_matrix.py does.  The neighbourhood ball, maxneighbors and
minneighbors are the oracle's own.  The lists (idx, count) come from crossval_ref.eligible_lists: the (key, index) ranking
of every eligible sample."""
import numpy as np

from oracle import idw_lwr as O
from oracle import kriging as K

import crossval_ref as CR
from rotated_frame import frame

OK_, MISSING, SINGULAR = 0, 1, 2
WEIGHTS = {(0, 3.0, 2.0): O.default_weightfun, (1, 0.0, 0.0): O.tricube}


def weightfun(spec):
    spec = tuple(spec)
    return WEIGHTS.get(spec) or O.exp_weight(spec[1], spec[2])


def eligible(xs, p, fold=None, exclude_radius=None, distance=None, radii=None, lattice=False):
    """Boolean mask over the samples: who may predict sample p (before the neighbourhood ball and maxneighbors)."""
    n = xs.shape[0]
    f = np.arange(n) if fold is None else np.asarray(fold)
    ok = f != f[p]
    if exclude_radius is not None:
        if lattice:
            xi = np.rint(xs).astype(np.int64)
            assert np.array_equal(xi, xs) and distance in (None, "euclidean") and radii is None
            r = int(exclude_radius)
            assert r == exclude_radius
            ok &= ((xi - xi[p]) ** 2).sum(axis=1) > r * r
        else:
            inv = None if radii is None else 1.0 / np.asarray(radii, dtype=np.float64)
            ok &= K.metric_key(xs, xs[p], distance, inv) > CR.exclusion_key(exclude_radius, distance)
    return ok


def predict(method, x, z, k, fold=None, exclude_radius=None, minneighbors=1, radius=None, radii=None, distance=None,
            rotation=None, lattice=False, exponent=1.0, weight=(0, 3.0, 2.0)):
    """(pred [nz x n] or [n] like z, aux [n], status [n]).  k == n: every eligible sample."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    # LWR and IDW are invariant under the rigid motion of the ball's frame: the oracle has no rotation argument
    xs = x if rotation is None else frame(x, np.asarray(rotation, dtype=np.float64))
    zc = np.atleast_2d(np.asarray(z, dtype=np.float64))
    n, nz = xs.shape[0], zc.shape[0]
    pred, aux, st = np.full((nz, n), np.nan), np.full(n, np.nan), np.full(n, MISSING, dtype=np.uint8)
    kmax = None if k >= n else int(k)
    kw = dict(radius=radius, radii=radii, distance=distance)
    kw.update(dict(exponent=exponent) if method == "idw" else dict(weightfun=weightfun(weight)))
    fn = O.idw if method == "idw" else O.lwr

    def run(out, held):
        nmax = out.size if kmax is None else min(kmax, out.size)
        if out.size == 0 or nmax < minneighbors:
            return                                               # the oracle asserts on it: every held-out sample missing
        for c in range(nz):
            mu, ax, s = fn(xs[out], zc[c, out], xs[held], maxneighbors=kmax, minneighbors=max(minneighbors, 1), **kw)
            pred[c, held] = mu
        aux[held], st[held] = ax, s

    if fold is not None and exclude_radius is None:
        f = np.asarray(fold)
        for fid in np.unique(f):
            run(np.flatnonzero(f != fid), np.flatnonzero(f == fid))
    else:
        for p in range(n):
            run(np.flatnonzero(eligible(xs, p, fold, exclude_radius, distance, radii, lattice)), np.array([p]))
    return (pred if np.ndim(z) == 2 else pred[0]), aux, st


def lists(x, k, fold=None, exclude_radius=None, radius=None, radii=None, distance=None, rotation=None):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    xs = x if rotation is None else frame(x, np.asarray(rotation, dtype=np.float64))
    return CR.eligible_lists(xs, k, fold, distance, radius, radii, exclude_radius)


def lwr_design_cond(x, idx, cnt, weight=(0, 3.0, 2.0)):
    """Largest 2-norm condition number of the oracle's normal matrix X'WX (raw coordinates, lwr.jl:137-139) over the
    samples with a full design; the error of the oracle's solve is of the order of eps times this."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    wf, worst = weightfun(weight), 0.0
    for p in range(x.shape[0]):
        ii = idx[p, :cnt[p]]
        if ii.size <= x.shape[1] + 1:
            continue
        d = np.sqrt(((x[ii] - x[p]) ** 2).sum(axis=1))
        if d.max() == 0.0:
            continue
        X = np.hstack([np.ones((ii.size, 1)), x[ii]])
        worst = max(worst, np.linalg.cond(X.T @ (wf(d / d.max())[:, None] * X)))
    return worst
