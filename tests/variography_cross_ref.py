"""numpy restatement of gss_variogram_cross (include/gss.h) -- the pair rule of tests/variography_ref.py with the
products of the value differences -- and of the algorithm of gss_variogram_fit_lmc, for the cross-variogram tests."""
import math

import numpy as np

import variography_ref as vref


def pair_row(nz, a, b):
    return a * nz - a * (a - 1) // 2 + (b - a)


def kept_pairs(x, nlags, maxlag, direction=None, dtol=np.inf, cos_atol=0.0, candidates=None):
    """-> (i, j, bin, d2) of the kept pairs and the number of duplicates; the key, bins and direction test are those of
    variography_ref.empirical.  candidates: (i, j) index arrays that contain every pair with d2 <= maxlag^2 (i < j),
    else all pairs."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, d = x.shape
    e2 = vref.edges2(nlags, maxlag)
    if candidates is None:
        blocks = []
        for i0 in range(0, n - 1, vref.ROWS):
            i1 = min(i0 + vref.ROWS, n)
            ii, jj = np.nonzero(np.arange(i0 + 1, n)[None, :] > np.arange(i0, i1)[:, None])
            blocks.append((i0 + ii, i0 + 1 + jj))
    else:
        blocks = [candidates]
    out, ndup = [], 0
    dtol2 = np.float64(dtol) * np.float64(dtol)
    cos2 = np.float64(cos_atol) * np.float64(cos_atol)
    for ii, jj in blocks:
        dl = [x[ii, a] - x[jj, a] for a in range(d)]
        d2 = dl[0] * dl[0]
        for a in range(1, d):
            d2 = d2 + dl[a] * dl[a]
        ndup += int(np.count_nonzero(d2 == 0.0))
        keep = (d2 > 0.0) & (d2 <= e2[nlags])
        if direction is not None:
            u = np.asarray(direction, dtype=np.float64)
            t = dl[0] * u[0]
            for a in range(1, d):
                t = t + dl[a] * u[a]
            tt = t * t
            keep &= ((d2 - tt) <= dtol2) & (tt >= cos2 * d2)
        dk = d2[keep]
        out.append((ii[keep], jj[keep], np.searchsorted(e2, dk, side="left") - 1, dk))
    i, j, k, dk = (np.concatenate(c) for c in zip(*out))
    return i, j, k, dk, ndup


def cross(x, z, nlags, maxlag, direction=None, dtol=np.inf, cos_atol=0.0, candidates=None, exact=False):
    """x (n, d), z (nz, n) -> count, lagsum, csum (nz (nz + 1) / 2, nlags), nduplicates, and asum = sum |products| per
    row and bin.  exact: the sums of products are math.fsum (correctly rounded) instead of numpy's."""
    z = np.asarray(z, dtype=np.float64)
    z = z.reshape(-1, z.shape[-1])
    nz = z.shape[0]
    i, j, k, dk, ndup = kept_pairs(x, nlags, maxlag, direction, dtol, cos_atol, candidates)
    count = np.bincount(k, minlength=nlags).astype(np.int64)
    lagsum = np.bincount(k, weights=np.sqrt(dk), minlength=nlags)
    csum = np.zeros((nz * (nz + 1) // 2, nlags))
    asum = np.zeros_like(csum)
    dz = z[:, i] - z[:, j]
    order = np.argsort(k, kind="stable")
    bounds = np.searchsorted(k[order], np.arange(nlags + 1))
    for a in range(nz):
        for b in range(a, nz):
            prod = dz[a] * dz[b]
            r = pair_row(nz, a, b)
            asum[r] = np.bincount(k, weights=np.abs(prod), minlength=nlags)
            if exact:
                ps = prod[order]
                csum[r] = [math.fsum(ps[bounds[q]:bounds[q + 1]]) for q in range(nlags)]
            else:
                csum[r] = np.bincount(k, weights=prod, minlength=nlags)
    return count, lagsum, csum, ndup, asum


def cell_candidates(x, maxlag):
    """(i, j), i < j, of every pair of samples in the same or in neighbouring cells of a grid of spacing slightly above
    maxlag: a superset of the pairs within maxlag."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    cell = np.floor((x - x.min(0)) / (maxlag * (1.0 + 1e-9))).astype(np.int64)
    dims = cell.max(0) + 3
    key = np.zeros(n, dtype=np.int64)
    for a in range(d):
        key = key * dims[a] + cell[:, a] + 1
    order = np.argsort(key, kind="stable")
    skey = key[order]
    ii, jj = [], []
    offs = np.stack(np.meshgrid(*[[-1, 0, 1]] * d, indexing="ij"), -1).reshape(-1, d)
    for o in offs:
        nk = np.zeros(n, dtype=np.int64)
        for a in range(d):
            nk = nk * dims[a] + cell[:, a] + 1 + o[a]
        lo, hi = np.searchsorted(skey, nk, side="left"), np.searchsorted(skey, nk, side="right")
        cnt = hi - lo
        src = np.repeat(np.arange(n), cnt)
        pos = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
        dst = order[pos]
        m = src < dst
        ii.append(src[m])
        jj.append(dst[m])
    return np.concatenate(ii), np.concatenate(jj)


# ---- the linear model of coregionalisation -------------------------------------------------------------------------
def project_psd(M):
    """Cyclic Jacobi in the fixed order (0,1), (0,2), ..; negative eigenvalues set to 0; a matrix without one is
    returned as it came."""
    nz = M.shape[0]
    A = 0.5 * (M + M.T)
    V = np.eye(nz)
    for _ in range(64):
        off = (A * A).sum() - (np.diag(A) ** 2).sum()
        if off <= 1e-34 * (A * A).sum():
            break
        for p in range(nz - 1):
            for q in range(p + 1, nz):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                R = np.eye(nz)
                R[p, p] = R[q, q] = c
                R[p, q], R[q, p] = s, -s
                A = R.T @ A @ R
                A[p, q] = A[q, p] = 0.0
                V = V @ R
    ev = np.diag(A)
    if (ev >= 0.0).all():
        return M
    return (V * np.maximum(ev, 0.0)) @ V.T


def lmc_objective(G, f, w, B0, B1):
    r = G - B0[None] - B1[None] * f[:, None, None]
    return float((w * (r * r).sum(axis=(1, 2))).sum())


def lmc_unconstrained(G, f, w):
    sw = w.sum()
    fb = (w * f).sum() / sw
    gb = (w[:, None, None] * G).sum(0) / sw
    sff = (w * (f - fb) ** 2).sum()
    if sff > 0.0:
        B1 = (w[:, None, None] * (f - fb)[:, None, None] * (G - gb[None])).sum(0) / sff
    else:                                                   # a range below every lag: f is constant
        B1 = np.zeros_like(gb)
    return gb - B1 * fb, B1


def lmc_inner(G, f, w):
    """G (m, nz, nz), f (m,), w (m,) -> (objective, B0, B1): Goulard-Voltz sweeps from the unconstrained solution."""
    sw, swf, swff = w.sum(), (w * f).sum(), (w * f * f).sum()
    SG = (w[:, None, None] * G).sum(0)
    SFG = ((w * f)[:, None, None] * G).sum(0)
    B0, B1 = lmc_unconstrained(G, f, w)
    for _ in range(1000):
        N0 = project_psd((SG - B1 * swf) / sw)
        N1 = project_psd((SFG - N0 * swf) / swff)
        d0, d1 = np.sqrt(((N0 - B0) ** 2).sum()), np.sqrt(((N1 - B1) ** 2).sum())
        B0, B1 = N0, N1
        tol = 1e-12 * (np.sqrt((B0 ** 2).sum()) + np.sqrt((B1 ** 2).sum()))
        if d0 <= tol and d1 <= tol:
            break
    return lmc_objective(G, f, w, B0, B1), B0, B1


def lmc_fit(kind, h, G, w, nu=1.0):
    """The range search of the library: 256-point log grid over [h_min / 4, 4 h_max], then golden section to 1e-8."""
    def at(r):
        return lmc_inner(G, vref.shape(kind, h / r, nu), w)[0]
    rg = (h.min() / 4.0) * (16.0 * h.max() / h.min()) ** (np.arange(256) / 255.0)
    og = np.array([at(r) for r in rg])
    ib = int(np.argmin(og))
    lo, hi = rg[max(ib - 1, 0)], rg[min(ib + 1, 255)]
    best = (og[ib], rg[ib])
    gr = 0.6180339887498949
    x1, x2 = hi - gr * (hi - lo), lo + gr * (hi - lo)
    o1, o2 = at(x1), at(x2)
    for _ in range(200):
        if not (hi - lo) > 1e-8 * 0.5 * (hi + lo):
            break
        best = min(best, (o1, x1), (o2, x2))
        if o1 <= o2:
            hi, x2, o2 = x2, x1, o1
            x1 = hi - gr * (hi - lo)
            o1 = at(x1)
        else:
            lo, x1, o1 = x1, x2, o2
            x2 = lo + gr * (hi - lo)
            o2 = at(x2)
    best = min(best, (o1, x1), (o2, x2))
    obj, B0, B1 = lmc_inner(G, vref.shape(kind, h / best[1], nu), w)
    return obj, best[1], B0, B1


def pack(G):
    """(m, nz, nz) -> (nz (nz + 1) / 2, m) in the row order of csum."""
    nz = G.shape[1]
    return np.ascontiguousarray(np.stack([G[:, a, b] for a in range(nz) for b in range(a, nz)]))
