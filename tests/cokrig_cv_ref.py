"""Cross-validation of a cokriging model under a moving neighbourhood in plain numpy (FP64), written from the text of
include/gss.h (gss_cokrig_cv_knn) on top of tests/cokrig_local_ref.py; it does not call the library.

Stacked sample p (variable v_p) is predicted as target v_p at its own location.  For every variable a the eligible samples
are those of variable a with fold[j] != fold[p] (fold None: every sample its own fold) whose squared search key
(cokrig_local_ref.search_keys) lies strictly above exclude_radius^2 when exclude_radius >= 0 -- a sample exactly on the
radius is left out -- and inside the ball; the k[a] first by (key, row) are taken.  Then the dense solve of
cokrig_local_ref.predict for that one target: under the ordinary variant the constraint of a variable without neighbours
is dropped, and a sample whose own variable has none is MISSING.
"""
import numpy as np

import cokrig_local_ref as LR

OK_, MISSING, SINGULAR = LR.OK_, LR.MISSING, LR.SINGULAR


def select(x, var, k, fold=None, exclude_radius=None, radius=None, radii=None, rotation=None):
    """-> idx[n, sum k] (rows of the caller's arrays, -1 padded), count[n, nz]."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    var = np.asarray(var)
    k = [int(v) for v in k]
    n, nz = x.shape[0], len(k)
    fold = np.arange(n) if fold is None else np.asarray(fold)
    key, bound = LR.search_keys(x, x, radius, radii, rotation, x[0])
    ex = None if exclude_radius is None or exclude_radius < 0 else float(exclude_radius) ** 2
    idx = np.full((n, sum(k)), -1, dtype=np.int32)
    count = np.zeros((n, nz), dtype=np.int32)
    off = 0
    for a in range(nz):
        rows = np.flatnonzero(var == a)
        for p in range(n):
            kk = key[p, rows]
            ok = fold[rows] != fold[p]
            if ex is not None:
                ok &= kk > ex
            if bound is not None:
                ok &= kk <= bound
            cand, kc = rows[ok], kk[ok]
            order = np.lexsort((cand, kc))[:k[a]]               # by (key, row)
            idx[p, off:off + order.size] = cand[order]
            count[p, a] = order.size
        off += k[a]
    return idx, count


def predict(model, x, z, var, k, fold=None, exclude_radius=None, variant="ordinary", means=None, minneighbors=1,
            radius=None, radii=None, rotation=None, with_cond=False):
    """-> pred[n], variance[n], status[n], idx, count (and the largest cond_2 of a per-sample system)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    var = np.asarray(var)
    z = np.asarray(z, dtype=np.float64)
    nz, n = model.nz, x.shape[0]
    idx, count = select(x, var, k, fold, exclude_radius, radius, radii, rotation)
    mu0 = np.zeros(nz)
    if variant == "simple" and means is not None:
        mu0 = np.array(np.broadcast_to(np.asarray(means, dtype=np.float64), (nz,)))
    pred = np.full(n, np.nan)
    varc = np.full(n, np.nan)
    status = np.zeros(n, dtype=np.uint8)
    worst = 0.0
    origin = x[0]
    for p in range(n):
        rows = idx[p][idx[p] >= 0]
        K, t = rows.size, int(var[p])
        if K < max(int(minneighbors), 1) or (variant != "simple" and count[p, t] == 0):
            status[p] = MISSING
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
        rhs = np.concatenate([model.cov(xs, vs, x[p:p + 1], np.array([t]), origin)[:, 0],
                              [1.0 if a == t else 0.0 for a in present]])
        lam = np.linalg.solve(A, rhs)
        pred[p] = mu0[t] + lam[:K] @ zs
        varc[p] = max((model.B0[t, t] + model.B1[t, t]) - lam @ rhs, 0.0)
    out = (pred, varc, status, idx, count)
    return out + (worst,) if with_cond else out


def fold_mean_mse(z, pred, status, fold):
    """The mean over the non-empty folds of the fold's mean squared error over its OK samples (gss_cv_summary)."""
    z, pred, status, fold = (np.asarray(a) for a in (z, pred, status, fold))
    ok = status == OK_
    mses = [np.mean((z[ok & (fold == f)] - pred[ok & (fold == f)]) ** 2) for f in np.unique(fold)
            if np.any(ok & (fold == f))]
    return float(np.mean(mses))
