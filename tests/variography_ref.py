"""numpy restatement of gss_variogram_empirical (include/gss.h, "variography") and of the inner solve of
gss_variogram_fit, for the variography tests.  Every operation is written in the order the header states, one rounding
each (numpy never fuses a multiply with an add), so the bin of every pair is reproduced exactly."""
import numpy as np

ROWS = 256          # rows of the pair matrix per pass


def edges2(nlags, maxlag):
    delta = np.float64(maxlag) / np.float64(nlags)
    e = np.arange(nlags + 1, dtype=np.float64) * delta
    return e * e


def empirical(x, z, nlags, maxlag, direction=None, dtol=np.inf, cos_atol=0.0, estimator="matheron"):
    """x (n, d), z (nz, n) -> count (nlags,) int64, lagsum (nlags,), zsum (nz, nlags), nduplicates."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    z = np.asarray(z, dtype=np.float64).reshape(-1, x.shape[0])
    n, d = x.shape
    nz = z.shape[0]
    e2 = edges2(nlags, maxlag)
    count = np.zeros(nlags, dtype=np.int64)
    lagsum = np.zeros(nlags)
    zsum = np.zeros((nz, nlags))
    ndup = 0
    dtol2 = np.float64(dtol) * np.float64(dtol)
    cos2 = np.float64(cos_atol) * np.float64(cos_atol)
    for i0 in range(0, n - 1, ROWS):
        i1 = min(i0 + ROWS, n)
        rows = np.arange(i0, i1)[:, None]
        cols = np.arange(i0 + 1, n)[None, :]
        upper = cols > rows                                   # unordered pairs i < j
        dl = [x[i0:i1, a][:, None] - x[i0 + 1:, a][None, :] for a in range(d)]
        d2 = dl[0] * dl[0]
        for a in range(1, d):
            d2 = d2 + dl[a] * dl[a]
        ndup += int(np.count_nonzero(upper & (d2 == 0.0)))
        keep = upper & (d2 > 0.0) & (d2 <= e2[nlags])
        if direction is not None:
            u = np.asarray(direction, dtype=np.float64)
            t = dl[0] * u[0]
            for a in range(1, d):
                t = t + dl[a] * u[a]
            tt = t * t
            p2 = d2 - tt
            keep &= (p2 <= dtol2) & (tt >= cos2 * d2)
        ii, jj = np.nonzero(keep)
        dk = d2[ii, jj]
        k = np.searchsorted(e2, dk, side="left") - 1          # e2[k] < d2 <= e2[k + 1]
        count += np.bincount(k, minlength=nlags)
        lagsum += np.bincount(k, weights=np.sqrt(dk), minlength=nlags)
        for c in range(nz):
            dz = z[c, i0 + ii] - z[c, i0 + 1 + jj]
            val = dz * dz if estimator == "matheron" else np.sqrt(np.abs(dz))
            zsum[c] += np.bincount(k, weights=val, minlength=nlags)
    return count, lagsum, zsum, ndup


# ---- model shapes and the inner solve of the fit --------------------------------------------------------------
def shape(kind, x, nu=1.0):
    """f(h / range) of gamma = nugget + (sill - nugget) f."""
    x = np.asarray(x, dtype=np.float64)
    if kind == "gaussian":
        return -np.expm1(-3.0 * x * x)
    if kind == "exponential":
        return -np.expm1(-3.0 * x)
    if kind == "spherical":
        return np.where(x < 1.0, 1.5 * x - 0.5 * x ** 3, 1.0)
    if kind == "cubic":
        return np.where(x < 1.0, 7 * x ** 2 - 8.75 * x ** 3 + 3.5 * x ** 5 - 0.75 * x ** 7, 1.0)
    if kind == "pentaspherical":
        return np.where(x < 1.0, 1.875 * x - 1.25 * x ** 3 + 0.375 * x ** 5, 1.0)
    if kind == "sinehole":
        t = np.pi * x
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(t > 0, 1.0 - np.sin(t) / t, 0.0)
    if kind == "matern":
        from scipy.special import gamma, kv
        dd = np.sqrt(2.0 * nu) * 3.0 * x
        with np.errstate(invalid="ignore", over="ignore"):
            val = 1.0 - (2.0 ** (1.0 - nu) / gamma(nu)) * dd ** nu * kv(nu, dd)
        return np.where(dd > 0, val, 0.0)
    raise ValueError(kind)


def model(kind, h, nugget, sill, rng, nu=1.0):
    return nugget + (sill - nugget) * shape(kind, np.asarray(h) / rng, nu)


def fit_weights(h, count, weighting):
    c = np.asarray(count, dtype=np.float64)
    return {"count": c, "count/h2": c / (h * h), "uniform": np.ones_like(c)}[weighting]


def inner_solve(f, g, w, frac=1.0):
    """min over a >= 0, b >= 0, (1 - frac) a <= frac b of sum w (a + b f - g)^2: the unconstrained minimum if
    feasible, else the best of the three edges and the origin.  -> (objective, a, b)."""
    def obj(a, b):
        r = a + b * f - g
        return float(np.sum(w * r * r))

    cands = [(0.0, 0.0)]
    sw = w.sum()
    fb, gb = (w * f).sum() / sw, (w * g).sum() / sw
    sff = (w * (f - fb) ** 2).sum()
    if sff > 0:
        b = (w * (f - fb) * (g - gb)).sum() / sff
        cands.append((gb - b * fb, b))
    if (w * f * f).sum() > 0:
        cands.append((0.0, (w * f * g).sum() / (w * f * f).sum()))
    cands.append((gb, 0.0))
    if frac < 1.0:
        c = frac / (1.0 - frac)
        b = (w * (c + f) * g).sum() / (w * (c + f) ** 2).sum()
        cands.append((c * b, b))
    best = None
    for a, b in cands:
        if a >= 0 and b >= 0 and (1.0 - frac) * a <= frac * b:
            o = obj(a, b)
            if best is None or o < best[0]:
                best = (o, a, b)
    return best


def grid_objective(kind, h, g, w, nu=1.0, frac=1.0, npts=2000):
    """Smallest objective over `npts` log-spaced ranges in [h_min / 4, 4 h_max]."""
    rs = np.geomspace(h.min() / 4.0, 4.0 * h.max(), npts)
    return min(inner_solve(shape(kind, h / r, nu), g, w, frac)[0] for r in rs)
