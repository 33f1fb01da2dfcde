"""CPU reference of the cross-validation calls (include/gss.h, gss_krig_cv_global / gss_krig_cv_knn / gss_cv_summary) and
the stand-in engine that lets gss.validation run without a device.  Brute force on purpose: leave-one-out is n refits
with oracle.kriging, a fold search ranks every eligible sample by (key, index), the summary is plain numpy.  The closed
form `loo_closed_form` (Dubrule 1983) is the numpy statement of what the device reads off its factor; the host tests pin
it against the refits."""
import numpy as np

from oracle import kriging as K
from oracle_engine import OracleEngine, _Krig
from rotated_frame import frame


def _sub(a, keep):
    return None if a is None else np.asarray(a)[keep]


def loo_refit(variant, vg, x, z, mean=0.0, degree=None, drift_data=None):
    """(pred, var): sample i predicted by the system fitted to the other n - 1 samples."""
    x, z = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.asarray(z, dtype=np.float64)
    n = x.shape[0]
    pred, var = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        fk = K.fit(variant, vg, x[keep], z[keep], mean, degree, _sub(drift_data, keep))
        a, b = K.predict(fk, x[i:i + 1], None if drift_data is None else np.asarray(drift_data)[i:i + 1])
        pred[i], var[i] = a[0], b[0]
    return pred, var


def loo_closed_form(variant, vg, x, z, mean=0.0, degree=None, drift_data=None):
    """B = inv([C F; F' 0]), wd = B [z - mean; 0]: pred_i = z_i - wd_i / B_ii, var_i = max(0, 1 / B_ii)."""
    x, z = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.asarray(z, dtype=np.float64)
    n = x.shape[0]
    F = K.drift_matrix(variant, x, degree, drift_data)
    nc = F.shape[1]
    lhs = np.zeros((n + nc, n + nc))
    lhs[:n, :n] = K.cov_pairwise(vg, x)
    lhs[:n, n:] = F
    lhs[n:, :n] = F.T
    B = np.linalg.inv(lhs)
    rhs = np.concatenate([z - (mean if variant == K.SK else 0.0), np.zeros(nc)])
    wd = B @ rhs
    d = np.diag(B)[:n]
    return z - wd[:n] / d, np.maximum(1.0 / d, 0.0)


def exclusion_key(exclude_radius, distance=None):
    """The exclusion radius in the units of the search key: squared for the Euclidean family."""
    if exclude_radius is None:
        return None
    return float(exclude_radius) ** 2 if distance in (None, "euclidean") else float(exclude_radius)


def eligible_lists(xs, k, fold=None, distance=None, radius=None, radii=None, exclude_radius=None, queries=None):
    """(idx [q x k] int32, -1 padded; count [q]) for the samples `queries` (default: all): the k nearest samples j with
    fold[j] != fold[p] (fold None: j != p), key(p, j) > exclusion key, inside the ball, by ascending (key, index).  `xs`
    are the samples on the search frame (a rotated ball: rotated_frame.frame(x, R))."""
    xs = np.atleast_2d(np.asarray(xs, dtype=np.float64))
    n = xs.shape[0]
    queries = np.arange(n) if queries is None else np.asarray(queries)
    f = np.arange(n) if fold is None else np.asarray(fold)
    inv = None if radii is None else 1.0 / np.asarray(radii, dtype=np.float64)
    r2 = 1.0 if radii is not None else (None if radius is None else float(radius) ** 2)
    ex = exclusion_key(exclude_radius, distance)
    idx = np.full((len(queries), k), -1, dtype=np.int32)
    cnt = np.zeros(len(queries), dtype=np.int32)
    pool = {}                                                        # fold id -> (samples outside it, their coordinates)
    for row, p in enumerate(queries):
        if fold is None:
            out, xo = np.arange(n), xs
        else:
            if f[p] not in pool:
                o = np.flatnonzero(f != f[p])
                pool[f[p]] = (o, xs[o])
            out, xo = pool[f[p]]
        key = K.metric_key(xo, xs[p], distance, inv)
        cand, kc = out, key                                          # ascending index: ties fall to the lower index
        if fold is None or ex is not None or r2 is not None:
            ok = out != p
            if ex is not None:
                ok &= key > ex
            if r2 is not None:
                ok &= key <= r2
            cand, kc = out[ok], key[ok]
        if cand.size > 4 * k:                                        # only keys up to the k-th smallest can be listed
            keep = kc <= np.partition(kc, k - 1)[k - 1]
            cand, kc = cand[keep], kc[keep]
        order = cand[np.argsort(kc, kind="stable")][:k]
        idx[row, :order.size] = order
        cnt[row] = order.size
    return idx, cnt


def solve_on_lists(variant, vg, x, z, idx, cnt, minneighbors=1, mean=0.0, degree=None, drift_data=None, queries=None):
    """(pred, var, status) of the samples `queries` kriged from their lists with oracle.kriging."""
    x, z = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.asarray(z, dtype=np.float64)
    queries = np.arange(x.shape[0]) if queries is None else np.asarray(queries)
    pred, var = np.full(len(queries), np.nan), np.full(len(queries), np.nan)
    status = np.zeros(len(queries), dtype=np.uint8)
    for row, p in enumerate(queries):
        nn = int(cnt[row])
        if nn < minneighbors or nn == 0:
            status[row] = 1
            continue
        ii = idx[row, :nn]
        fk = K.fit(variant, vg, x[ii], z[ii], mean, degree, _sub(drift_data, ii))
        a, b = K.predict(fk, x[p:p + 1], None if drift_data is None else np.asarray(drift_data)[p:p + 1])
        pred[row], var[row] = a[0], b[0]
    return pred, var, status


def summary(z, pred, var, status=None, fold=None, nfolds=0):
    """(dict of the fields of gss_cv_summary_t, per-fold mean squared errors or None), evaluated directly."""
    z, pred, var = (np.asarray(a, dtype=np.float64) for a in (z, pred, var))
    st = np.zeros(z.size, dtype=np.uint8) if status is None else np.asarray(status)
    ok = st == 0
    e = (z - pred)[ok]
    sd = ok & (var > 0.0)
    es = (z - pred)[sd] / np.sqrt(var[sd])
    mean = lambda a: float(np.mean(a)) if a.size else float("nan")   # noqa: E731
    out = dict(n_ok=float(ok.sum()), n_missing=float((st == 1).sum()), n_singular=float(((st != 0) & (st != 1)).sum()),
               me=mean(e), mae=mean(np.abs(e)), mse=mean(e * e), mse_std_n=float(sd.sum()), mean_std=mean(es),
               msq_std=mean(es * es))
    fmse = None
    if fold is None:
        out["cverror"] = out["mse"]
    else:
        fold = np.asarray(fold)
        fmse = np.array([mean(((z - pred)[ok & (fold == f)]) ** 2) for f in range(nfolds)])
        out["cverror"] = mean(fmse[~np.isnan(fmse)])
    return out, fmse


class _CVKrig(_Krig):
    def __init__(self, *a, factor=True, **kw):
        super().__init__(*a, factor=factor, **kw)
        self.factor = factor

    def cv_global(self, device=False):
        if not self.factor:
            raise RuntimeError("handle has no factor")
        pred, var = loo_refit(self.variant, self.vg, self.x, self.z, self.mean, self.degree, self.drift_data)
        return pred, var, np.zeros(len(pred), dtype=np.uint8)

    def cv_knn(self, k, fold=None, exclude_radius=None, minneighbors=1, radius=None, radii=None, return_idx=False,
               distance=None, rotation=None, device=False):
        if not 1 <= k <= self.x.shape[0] - 1:
            raise ValueError("k outside 1..n-1")
        xs = self.x if rotation is None else frame(self.x, np.asarray(rotation, dtype=np.float64))
        idx, cnt = eligible_lists(xs, k, fold, distance, radius, radii, exclude_radius)
        out = solve_on_lists(self.variant, self.vg, self.x, self.z, idx, cnt, minneighbors, self.mean, self.degree,
                             self.drift_data)
        return out + (idx, cnt) if return_idx else out


class CVOracleEngine(OracleEngine):
    """oracle_engine.OracleEngine plus the cross-validation calls of gss.engine.HipEngine."""
    Krig = _CVKrig

    @staticmethod
    def cv_summary(z, pred, var, status=None, fold=None, nfolds=0):
        return summary(z, pred, var, status, fold, nfolds)
