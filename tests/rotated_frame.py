"""Independent restatement of the rotated-ball frame (include/gss.h, gss_variogram_t::rotation): x' = R^T (x - c),
evaluated with the library's fixed arithmetic -- u = x - c, x'_k = (R0k u0 + R1k u1) + R2k u2 over the d leading
terms, one rounding per operation -- with element-wise numpy (no BLAS, no FMA), so that neighbour indices of a search
on x' can be compared bit-exactly."""
import numpy as np


def frame(x, R, c=None):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    R = np.asarray(R, dtype=np.float64)
    d = x.shape[1]
    c = x[0] if c is None else np.asarray(c, dtype=np.float64)
    u = [x[:, i] - c[i] for i in range(d)]
    out = np.empty_like(x)
    for k in range(d):
        acc = R[0, k] * u[0]
        for i in range(1, d):
            acc = acc + R[i, k] * u[i]
        out[:, k] = acc
    return out


def mahalanobis_sq(a, b, radii, R):
    """(a - b)^T M (a - b) with M = R diag(r^-2) R^T, pairwise (na x nb)."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    R = np.asarray(R, dtype=np.float64)
    M = R @ np.diag(1.0 / np.asarray(radii, dtype=np.float64) ** 2) @ R.T
    h = a[:, None, :] - b[None, :, :]
    return np.einsum("ijk,kl,ijl->ij", h, M, h)


def rot2(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s], [s, c]])


def rot3(a, b, g):
    """Z(a) Y(b) X(g): a proper 3-D rotation."""
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Z = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]])
    Y = np.array([[cb, 0, sb], [0, 1.0, 0], [-sb, 0, cb]])
    X = np.array([[1.0, 0, 0], [0, cg, -sg], [0, sg, cg]])
    return Z @ Y @ X
