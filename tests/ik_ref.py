"""Indicator kriging restated in numpy on the oracle's own pieces (oracle.kriging for the neighbours under the
(distance, index) rule, oracle.variogram for the covariances): per point the bordered system is assembled and solved,
the K raw values formed, then the order-relation correction and the post-processing formulas of include/gss.h are
applied.  `longdouble=True` solves the same FP64 systems in np.longdouble (the reference the error bars are measured
against, tools/ik_oracle.py).  Conventions: include/gss.h, "indicator kriging"."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import kriging as K
from oracle.variogram import cov_pairwise
from oracle_engine import _ovg

OK_, MISSING, SINGULAR = 0, 1, 2


def to_frame(x, R, c):
    """x' = R^T (x - c) with the library's rounding order (frame_point: products and sums rounded one by one)."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    R = np.asarray(R, dtype=np.float64)
    u = x - np.asarray(c, dtype=np.float64)[None, :]
    out = np.empty_like(u)
    for k in range(d):
        acc = R[0, k] * u[:, 0]
        for a in range(1, d):
            acc = acc + R[a, k] * u[:, a]
        out[:, k] = acc
    return out


def _rotation(models):
    for g in models:
        r = getattr(g, "rotation", None)
        if r is not None:
            return np.asarray(r, dtype=np.float64)
    return None


def _solve_ld(A, B):
    """Gaussian elimination with partial pivoting in np.longdouble."""
    A = np.array(A, dtype=np.longdouble)
    B = np.array(B, dtype=np.longdouble)
    n = A.shape[0]
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]] = A[[p, j]]
            B[[j, p]] = B[[p, j]]
        f = A[j + 1:, j] / A[j, j]
        A[j + 1:] -= f[:, None] * A[j][None, :]
        B[j + 1:] -= f[:, None] * B[j][None, :]
    X = np.zeros_like(B)
    for j in range(n - 1, -1, -1):
        X[j] = (B[j] - A[j, j + 1:] @ X[j + 1:]) / A[j, j]
    return X


def order_relations(F):
    """GSLIB's correction, row by row: clip, upward max, downward min, average."""
    F = np.asarray(F, dtype=np.float64)
    out = np.empty_like(F)
    for p in range(F.shape[0]):
        f = F[p]
        if np.isnan(f).any():
            out[p] = np.nan
            continue
        c = np.where(f < 0.0, 0.0, np.where(f > 1.0, 1.0, f))
        U = c.copy()
        for q in range(1, c.size):
            U[q] = max(U[q - 1], c[q])
        D = c.copy()
        for q in range(c.size - 2, -1, -1):
            D[q] = min(D[q + 1], c[q])
        out[p] = (U + D) * 0.5
    return out


def predict(x, z, xdom, cutoffs, models, k, minneighbors=1, fstar=None, radius=None, radii=None, distance=None,
            longdouble=False):
    """-> dict(raw[m, K], ccdf[m, K], status[m], idx[m, k], cnt[m], wsum[m, K] = max(1, sum |lambda|)).  `models`: a list
    of one (median form) or K (full form) gss variograms; `fstar`: None (ordinary) or K proportions (simple)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    xdom = np.atleast_2d(np.asarray(xdom, dtype=np.float64))
    z = np.asarray(z, dtype=np.float64)
    cut = np.asarray(cutoffs, dtype=np.float64)
    Kc, m = cut.size, xdom.shape[0]
    R = _rotation(models)
    xs, xd = (x, xdom) if R is None else (to_frame(x, R, x[0]), to_frame(xdom, R, x[0]))
    idx, cnt = K.knn_search(xs if radii is None else x, xd if radii is None else xdom, k, radius, radii, distance)
    ovgs = [_ovg(g) for g in models]
    ft = np.longdouble if longdouble else np.float64
    raw = np.full((m, Kc), np.nan)
    raw_ld = np.full((m, Kc), np.nan, dtype=ft)      # the values before they are rounded to FP64
    wsum = np.ones((m, Kc))
    status = np.zeros(m, dtype=np.uint8)
    ind_all = (z[:, None] <= cut[None, :]).astype(np.float64)
    for p in range(m):
        nn = int(cnt[p])
        if nn < max(minneighbors, 1):
            status[p] = MISSING
            continue
        ii = idx[p, :nn]
        xn, ind = xs[ii], ind_all[ii]
        out = np.empty(Kc, dtype=ft)
        ws = np.ones(Kc)
        bad = False
        for s, vg in enumerate(ovgs):
            C = cov_pairwise(vg, xn)
            c0 = cov_pairwise(vg, xn, xd[p:p + 1])[:, 0]
            try:
                np.linalg.cholesky(C)
            except np.linalg.LinAlgError:
                bad = True
                break
            if fstar is None:
                A = np.zeros((nn + 1, nn + 1))
                A[:nn, :nn] = C
                A[:nn, nn] = A[nn, :nn] = 1.0
                b = np.concatenate([c0, [1.0]])
            else:
                A, b = C, c0
            lam = (_solve_ld(A, b[:, None])[:, 0] if longdouble else np.linalg.solve(A, b))[:nn]
            qs = range(Kc) if len(ovgs) == 1 else (s,)
            for q in qs:
                col = ind[:, q].astype(ft)
                if fstar is None:
                    out[q] = lam @ col
                else:
                    out[q] = ft(fstar[q]) + lam @ (col - ft(fstar[q]))
                ws[q] = max(1.0, float(np.sum(np.abs(lam))))
        if bad:
            status[p] = SINGULAR
            continue
        raw[p] = out.astype(np.float64)
        raw_ld[p] = out
        wsum[p] = ws
    return dict(raw=raw, ccdf=order_relations(raw), status=status, idx=idx, cnt=cnt, wsum=wsum, raw_ld=raw_ld)


def predict_global(x, z, xdom, cutoffs, models, fstar=None, longdouble=False):
    """The global neighbourhood in the dual form the twin composes it in: one system over all n samples per model,
    W = A^-1 [columns; 0] with the K indicator columns (residuals i_q - F*_q under the simple variant), and
    F_q(p) = [c0(p); 1] . W_q (+ F*_q).  -> raw[m, K] (FP64) and raw_ld[m, K] (before rounding)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    xdom = np.atleast_2d(np.asarray(xdom, dtype=np.float64))
    z = np.asarray(z, dtype=np.float64)
    cut = np.asarray(cutoffs, dtype=np.float64)
    n, Kc = x.shape[0], cut.size
    ft = np.longdouble if longdouble else np.float64
    ind = (z[:, None] <= cut[None, :]).astype(np.float64)
    if fstar is not None:
        ind = ind - np.asarray(fstar, dtype=np.float64)[None, :]
    out = np.empty((xdom.shape[0], Kc), dtype=ft)
    for s, g in enumerate(models):
        vg = _ovg(g)
        qs = list(range(Kc)) if len(models) == 1 else [s]
        C = cov_pairwise(vg, x)
        c0 = cov_pairwise(vg, x, xdom)                           # n x m
        if fstar is None:
            A = np.zeros((n + 1, n + 1))
            A[:n, :n] = C
            A[:n, n] = A[n, :n] = 1.0
            B = np.vstack([ind[:, qs], np.zeros((1, len(qs)))])
            rhs = np.vstack([c0, np.ones((1, xdom.shape[0]))])
        else:
            A, B, rhs = C, ind[:, qs], c0
        W = _solve_ld(A, B) if longdouble else np.linalg.solve(A, B)
        out[:, qs] = rhs.astype(ft).T @ W
    if fstar is not None:
        out = out + np.asarray(fstar, dtype=np.float64).astype(ft)[None, :]
    return dict(raw=out.astype(np.float64), raw_ld=out)


def post(ccdf, cutoffs, zmin, zmax, wlo=1.0, whi=1.0, thresholds=(), probs=(), longdouble=False):
    """-> dict(etype[m], cvar[m], pabove[m, nthr], quant[m, nq]) under the ccdf model of gss_ik_post."""
    ft = np.longdouble if longdouble else np.float64
    F = np.asarray(ccdf, dtype=np.float64)
    c = np.asarray(cutoffs, dtype=np.float64).astype(ft)
    m, Kc = F.shape
    zmin, zmax, wlo, whi = ft(zmin), ft(zmax), ft(wlo), ft(whi)
    thr = np.asarray(thresholds, dtype=np.float64).astype(ft)
    pr = np.asarray(probs, dtype=np.float64).astype(ft)
    et, cv = np.full(m, np.nan), np.full(m, np.nan)
    pa, qu = np.full((m, thr.size), np.nan), np.full((m, pr.size), np.nan)
    dlo, dhi = c[0] - zmin, zmax - c[-1]
    slo, s2lo = dlo * (wlo / (wlo + 1)), dlo * dlo * (wlo / (wlo + 2))
    shi, s2hi = dhi * (whi / (whi + 1)), dhi * dhi * (whi / (whi + 2))
    pw = lambda v, w: v if w == 1 else v ** w      # noqa: E731
    for p in range(m):
        if np.isnan(F[p]).any():
            continue
        f = F[p].astype(ft)
        m1 = f[0] * (zmin + slo)
        m2 = f[0] * (zmin * zmin + 2 * zmin * slo + s2lo)
        for q in range(1, Kc):
            pq, a, b = f[q] - f[q - 1], c[q - 1], c[q]
            m1 = m1 + pq * ((a + b) / 2)
            m2 = m2 + pq * ((a * a + a * b + b * b) / 3)
        pt = 1 - f[-1]
        m1 = m1 + pt * (zmax - shi)
        m2 = m2 + pt * (zmax * zmax - 2 * zmax * shi + s2hi)
        et[p] = m1
        cv[p] = max(m2 - m1 * m1, ft(0))
        for i, t in enumerate(thr):
            if t <= c[0]:
                Ft = f[0] * pw((t - zmin) / dlo, wlo)
            elif t > c[-1]:
                Ft = 1 - (1 - f[-1]) * pw((zmax - t) / dhi, whi)
            else:
                q = int(np.searchsorted(c, t, side="left"))          # smallest q with t <= c_q
                Ft = f[q - 1] + (f[q] - f[q - 1]) * ((t - c[q - 1]) / (c[q] - c[q - 1]))
            pa[p, i] = 1 - Ft
        for i, pp in enumerate(pr):
            if pp <= f[0]:
                zq = zmin + dlo * pw(pp / f[0], 1 / wlo)
            elif pp > f[-1]:
                zq = zmax - dhi * pw((1 - pp) / (1 - f[-1]), 1 / whi)
            else:
                q = int(np.argmax(f >= pp))                          # smallest q with F_q >= p
                zq = c[q - 1] + (c[q] - c[q - 1]) * ((pp - f[q - 1]) / (f[q] - f[q - 1]))
            qu[p, i] = zq
    return dict(etype=et, cvar=cv, pabove=pa, quant=qu)
