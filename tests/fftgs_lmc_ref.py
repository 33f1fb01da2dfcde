"""numpy restatement of the co-simulation of include/gss.h (gss_fftgs_create_lmc): the factor rule and the mixture

    Z_a = means[a] + sum_j L1[a][j] Y_j + sum_j L0[a][j] E_j

with Y_j the oracle's FFTGS fields of the unit structure and E_j the oracle's Philox normals, numbered as the header
writes them.  Test infrastructure only."""
import math

import numpy as np

from oracle import fftgs as O
from oracle import philox
from oracle.variogram import Variogram

NUGGET_SALT = 0x6e75676765744c4d      # gss.h, GSS_FFTGS_LMC_NUGGET_SALT
EPS = 2.0 ** -52


class NotPSD(ValueError):
    pass


def factor(B, which="B"):
    """Left-looking Cholesky without pivoting of (B + B^T) / 2, one IEEE operation at a time in the order of
    csrc/fftgs_lmc.h (lmc_factor).  -> (L, live): the lower factor and the list of its non-zero columns."""
    B = np.asarray(B, dtype=np.float64)
    n = B.shape[0]
    B = [[0.5 * (float(B[a, b]) + float(B[b, a])) for b in range(n)] for a in range(n)]
    d = max(B[j][j] for j in range(n))
    tol = 1e-12 * d
    L = [[0.0] * n for _ in range(n)]
    live = []
    for j in range(n):
        p = B[j][j]
        for k in range(j):
            p = p - L[j][k] * L[j][k]
        if p < -tol:
            raise NotPSD(f"{which} is not positive semidefinite: the pivot at [{j}][{j}] is {p}")
        zero = p <= tol
        ljj = 0.0 if zero else math.sqrt(p)
        L[j][j] = ljj
        for i in range(j + 1, n):
            t = B[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k]
            if zero:
                if abs(t) > tol:
                    raise NotPSD(f"{which} is not positive semidefinite: entry [{i}][{j}] leaves {t} beside a zero pivot")
            else:
                L[i][j] = t / ljj
        if not zero:
            live.append(j)
    return np.array(L).reshape(n, n), live


def mix(L0, live0, L1, live1, means, Y, E):
    """Y, E: {column: field of N cells} for the live columns -> (Z[nz, N], S[nz, N]) with S the sum of the absolute
    terms, the scale of the rounding bound."""
    nz = len(means)
    N = len(next(iter(list(Y.values()) + list(E.values())))) if (Y or E) else 0
    Z = np.empty((nz, N))
    S = np.empty((nz, N))
    for a in range(nz):
        z = np.full(N, float(means[a]))
        s = np.full(N, abs(float(means[a])))
        for j in live1:
            z = z + L1[a, j] * Y[j]
            s = s + abs(L1[a, j]) * np.abs(Y[j])
        for j in live0:
            z = z + L0[a, j] * E[j]
            s = s + abs(L0[a, j]) * np.abs(E[j])
        Z[a], S[a] = z, s
    return Z, S


def bound(live0, live1, S):
    """One rounding per term, fused or not, in the device's sum and in the restatement's (include/gss.h; the issue's
    derivation): (live0 + live1 + 2) 2^-52 (|mean_a| + sum |L1||Y| + sum |L0||E|)."""
    return (len(live0) + len(live1) + 2) * EPS * S


def realize(kind, dims, b0, b1, means, seed, first_real, nreals, spacing=None, **vgkw):
    """The whole co-simulation on the host: (nreals, nz, N)."""
    L0, live0 = factor(b0, "b0")
    L1, live1 = factor(b1, "b1")
    nz = len(means)
    N = int(np.prod(dims))
    pre = O.preprocess(Variogram(kind, sill=1.0, nugget=0.0, **vgkw), dims, spacing=spacing)
    out = np.empty((nreals, nz, N))
    for r in range(first_real, first_real + nreals):
        Y = {j: O.realize(pre, seed, r * nz + j, 1)[0] for j in live1}
        E = {j: philox.normal(seed ^ NUGGET_SALT, r * nz + j, N) for j in live0}
        out[r - first_real] = mix(L0, live0, L1, live1, means, Y, E)[0]
    return out


# ---- the statistics check (tests/test_gpu_fftgs_lmc.py) ----------------------------------------------------------------------
STAT_DIMS, STAT_RANGE, STAT_NREALS, STAT_LAG = (64, 64), 8.0, 64, 4
STAT_B0 = np.array([[0.1, 0.05], [0.05, 0.1]])
STAT_B1 = np.array([[0.9, 0.75], [0.75, 0.9]])      # correlation (0.05 + 0.75) / 1 = 0.8 at lag 0
STAT_MEANS = np.array([1.0, -2.0])


def stat_model():
    """b0 [h = 0] + b1 rho(h) at lag 0 and at STAT_LAG cells along x: (2, 2, 2), lag first."""
    from oracle.variogram import cov_pairwise
    rho = cov_pairwise(Variogram("exponential", sill=1.0, range=STAT_RANGE), np.zeros((1, 2)),
                       np.array([[float(STAT_LAG), 0.0]]))[0, 0]
    return np.stack([STAT_B0 + STAT_B1, STAT_B1 * rho])


def lag_covariances(Z, means, dims, lag):
    """Z: (nreals, 2, N) on a 2-D grid (x fastest).  -> (2, 2, 2): the 2 x 2 matrix of cov(Z_a(x), Z_b(x + h)) about the
    known means, averaged over cells and realisations and symmetrised in (a, b), at h = 0 and h = `lag` cells along x."""
    n1, n2 = dims
    D = np.asarray(Z).reshape(Z.shape[0], 2, n2, n1) - np.asarray(means)[None, :, None, None]
    out = np.empty((2, 2, 2))
    for a in range(2):
        for b in range(2):
            out[0, a, b] = np.mean(D[:, a] * D[:, b])
            out[1, a, b] = 0.5 * (np.mean(D[:, a, :, :-lag] * D[:, b, :, lag:]) + np.mean(D[:, b, :, :-lag] * D[:, a, :, lag:]))
    return out
