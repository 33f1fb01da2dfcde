"""CPU reference of cross-validation by folds under the global neighbourhood (include/gss.h, gss_krig_cv_global_folds)
and the stand-in engine whose handle offers `cv_global_folds`.  Brute force on purpose: `folds_refit` fits oracle.kriging
to the samples outside a fold and predicts the fold's samples, once per fold.  `folds_closed_form` is the numpy statement
of what the device reads off its factor -- e_F = inv(B_FF) wd_F, var_F = diag(inv(B_FF)) with B = inv([C F; F' 0]) -- and
the host tests pin it against the refits."""
import numpy as np

from oracle import kriging as K

import crossval_ref as CR


def _groups(fold):
    fold = np.asarray(fold)
    return [np.flatnonzero(fold == f) for f in np.unique(fold)]


def _nc(variant, x, degree, drift_data):
    return K.drift_matrix(variant, x[:1], degree, None if drift_data is None else np.asarray(drift_data)[:1]).shape[1]


def folds_refit(variant, vg, x, z, fold, mean=0.0, degree=None, drift_data=None):
    """(pred, var, status): the samples of every fold predicted by the system fitted to all samples outside it.  A fold
    that leaves fewer than max(1, nc) samples: status 2, NaN (simple kriging: the mean and C(0) from no sample at all)."""
    x, z = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.asarray(z, dtype=np.float64)
    n = x.shape[0]
    nc = _nc(variant, x, degree, drift_data)
    pred, var = np.full(n, np.nan), np.full(n, np.nan)
    status = np.zeros(n, dtype=np.uint8)
    for F in _groups(fold):
        keep = np.ones(n, dtype=bool)
        keep[F] = False
        if variant == K.SK and not keep.any():
            pred[F], var[F] = mean, K.cov_pairwise(vg, x[:1])[0, 0]
            continue
        if variant != K.SK and keep.sum() < max(1, nc):
            status[F] = 2
            continue
        fk = K.fit(variant, vg, x[keep], z[keep], mean, degree, CR._sub(drift_data, keep))
        pred[F], var[F] = K.predict(fk, x[F], CR._sub(drift_data, F))
    return pred, var, status


def folds_closed_form(variant, vg, x, z, fold, mean=0.0, degree=None, drift_data=None):
    """(pred, var) by the block identity; every fold must leave a regular system."""
    x, z = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.asarray(z, dtype=np.float64)
    n = x.shape[0]
    F = K.drift_matrix(variant, x, degree, drift_data)
    nc = F.shape[1]
    lhs = np.zeros((n + nc, n + nc))
    lhs[:n, :n] = K.cov_pairwise(vg, x)
    lhs[:n, n:] = F
    lhs[n:, :n] = F.T
    B = np.linalg.inv(lhs)
    wd = B @ np.concatenate([z - (mean if variant == K.SK else 0.0), np.zeros(nc)])
    pred, var = np.empty(n), np.empty(n)
    for g in _groups(fold):
        inv = np.linalg.inv(B[np.ix_(g, g)])
        pred[g] = z[g] - inv @ wd[g]
        var[g] = np.maximum(np.diag(inv), 0.0)
    return pred, var


class _FoldKrig(CR._CVKrig):
    def cv_global_folds(self, fold, device=False):
        if fold is None:
            return self.cv_global()
        if not self.factor:
            raise RuntimeError("handle has no factor")
        return folds_refit(self.variant, self.vg, self.x, self.z, fold, self.mean, self.degree, self.drift_data)


class FoldOracleEngine(CR.CVOracleEngine):
    """crossval_ref.CVOracleEngine whose handle also offers cv_global_folds, by refits."""
    Krig = _FoldKrig
