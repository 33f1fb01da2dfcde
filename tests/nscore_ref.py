"""numpy restatement of the normal-score transform (include/gss.h, "normal-score transform"), and the same at 40 digits.

fit:      stable sort, equal values merged, cumulative weights in long double from both ends, scores through
          scipy.special.ndtri with the two-sided formula (fit_one_sided: the single-number form that loses the upper
          tail, kept to show that it does).
forward / inverse: linear between the bracketing knots, GSLIB's linear / power tails outside; in float64 or, with
          dtype=np.longdouble, in long double (erfc from mpmath there: numpy has no long-double erfc).
mp_*:     mpmath at 40 digits, the yardstick of the restatement itself.
"""
import mpmath as mp
import numpy as np
from scipy.special import erfc, ndtri

EPS = 2.0 ** -52
mp.mp.dps = 40


def classes(z, w=None):
    """Distinct values v and, in long double, the weight of each class, strictly below it and strictly above it."""
    z = np.asarray(z, dtype=np.float64)
    w = np.ones(z.size) if w is None else np.asarray(w, dtype=np.float64)
    o = np.argsort(z, kind="stable")
    zs, ws = z[o], w[o].astype(np.longdouble)
    first = np.concatenate([[True], zs[1:] != zs[:-1]])
    v = zs[first]
    W = np.add.reduceat(ws, np.flatnonzero(first))
    below = np.concatenate([[np.longdouble(0)], np.cumsum(W)[:-1]])
    above = np.concatenate([np.cumsum(W[::-1])[::-1][1:], [np.longdouble(0)]])
    return v, W, below, above


def fit(z, w=None):
    v, W, below, above = classes(z, w)
    T = W.sum()
    lower = below <= above
    p = (np.where(lower, below, above) + W / 2) / T
    q = ndtri(p.astype(np.float64))
    return v, np.where(lower, q, -q)


def fit_one_sided(z, w=None):
    """y_k = ndtri(p_k) with p_k one float64 number: above the median p_k is 1 - q_k rounded, and the tail is gone."""
    v, W, below, _ = classes(z, w)
    return v, ndtri(((below + W / 2) / W.sum()).astype(np.float64))


def _mp(x):
    return mp.mpf(float(x)) if not isinstance(x, np.longdouble) else mp.mpf(float(x)) + mp.mpf(float(x - np.longdouble(float(x))))


def mp_ndtri_lower(p):
    """Phi^-1(p) for an mpf p in (0, 1/2]: Newton on mp.ncdf from the float64 value (1e-16 -> 1e-32 -> 1e-64)."""
    x = mp.mpf(float(ndtri(float(p))))
    for _ in range(3):
        x = x - (mp.ncdf(x) - p) / mp.npdf(x)
    return x


def mp_knots(z, w=None, which=None):
    """The scores of knots `which` (indices; all by default) at 40 digits, from exactly summed weights."""
    v, W, _, _ = classes(z, w)
    Wm = [_mp(x) for x in W]
    T = mp.fsum(Wm)
    cum = [mp.mpf(0)]
    for x in Wm:
        cum.append(cum[-1] + x)
    out = []
    for k in (range(len(v)) if which is None else which):
        b, a = cum[k], T - cum[k + 1]
        out.append(mp_ndtri_lower((b + Wm[k] / 2) / T) if b <= a else -mp_ndtri_lower((a + Wm[k] / 2) / T))
    return out


def _interp(X, F, x, dtype):
    X, F, x = (np.asarray(a, dtype=dtype) for a in (X, F, x))
    k = np.clip(np.searchsorted(X, x, side="right") - 1, 0, max(X.size - 2, 0))
    if X.size == 1:
        return np.full(x.shape, F[0], dtype=dtype)
    with np.errstate(all="ignore"):          # (values outside the table are replaced by the callers)
        return F[k] + (F[k + 1] - F[k]) * (x - X[k]) / (X[k + 1] - X[k])


def forward(v, y, z, dtype=np.float64):
    z = np.asarray(z, dtype=dtype)
    out = _interp(v, y, np.where(np.isnan(z), v[0], z), dtype)
    out = np.where(z <= v[0], dtype(y[0]), np.where(z >= v[-1], dtype(y[-1]), out))
    return np.where(np.isnan(z), dtype(np.nan), out)


def _erfc(x, dtype):
    if dtype is np.float64:
        return erfc(x)
    return np.array([np.longdouble(mp.nstr(mp.erfc(_mp(t)), 25)) if np.isfinite(t) else
                     np.longdouble(0.0 if t > 0 else 2.0) for t in np.atleast_1d(x)], dtype=np.longdouble).reshape(np.shape(x))


def inverse(v, y, x, zmin=None, zmax=None, power=(1.0, 1.0), dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    zmin = v[0] if zmin is None else zmin
    zmax = v[-1] if zmax is None else zmax
    out = _interp(y, v, np.where(np.isnan(x), y[0], x), dtype)
    r2 = np.sqrt(dtype(2.0))
    lo, hi = x < y[0], x > y[-1]
    if lo.any():
        t = _erfc(-x[lo] / r2, dtype) / _erfc(np.asarray(-dtype(y[0]) / r2), dtype)
        if power[0] != 1.0:
            t = t ** dtype(power[0])
        out[lo] = dtype(zmin) + (dtype(v[0]) - dtype(zmin)) * t
    if hi.any():
        t = _erfc(x[hi] / r2, dtype) / _erfc(np.asarray(dtype(y[-1]) / r2), dtype)
        if power[1] != 1.0:
            t = t ** dtype(power[1])
        out[hi] = dtype(zmax) - (dtype(zmax) - dtype(v[-1])) * t
    return np.where(np.isnan(x), dtype(np.nan), out)


def mp_inverse_tails(v, y, x, zmin=None, zmax=None, power=(1.0, 1.0)):
    """The inverse outside [y_1, y_K] at 40 digits, rounded to float64 (NaN for NaN, and for x inside the table)."""
    zmin = v[0] if zmin is None else zmin
    zmax = v[-1] if zmax is None else zmax
    out = []
    for t in np.asarray(x, dtype=np.float64):
        if np.isnan(t) or y[0] <= t <= y[-1]:
            out.append(np.nan)
        elif t < y[0]:
            q = mp.mpf(0) if t == -np.inf else mp.erfc(-_mp(t) / mp.sqrt(2)) / mp.erfc(-_mp(y[0]) / mp.sqrt(2))
            out.append(float(_mp(zmin) + (_mp(v[0]) - _mp(zmin)) * q ** _mp(power[0])))
        else:
            q = mp.mpf(0) if t == np.inf else mp.erfc(_mp(t) / mp.sqrt(2)) / mp.erfc(_mp(y[-1]) / mp.sqrt(2))
            out.append(float(_mp(zmax) - (_mp(zmax) - _mp(v[-1])) * q ** _mp(power[1])))
    return np.array(out)
