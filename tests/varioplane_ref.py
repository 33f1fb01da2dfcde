"""numpy restatement of gss_variogram_plane (include/gss.h, "varioplane") for the varioplane tests: the pair key, the
lag bins and the sums are those of variography_ref.empirical; the sector of a pair follows the header's rule literally
(one rounding per operation in the stated order; numpy never fuses a multiply with an add)."""
import numpy as np

from variography_ref import ROWS, edges2


def dirs_of(angles):
    a = np.asarray(angles, dtype=np.float64)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


def uniform_dirs(nangles, offset=0.0):
    return dirs_of(offset + np.arange(nangles) * (np.pi / nangles))


def sector(a1, a2, dirs):
    """The header's rule: p = c_0 a2, q = s_0 a1; p == q -> 0; p < q -> negate (a1, a2); then the NUMBER of s in
    1 .. nangles - 1 with c_s a2 >= s_s a1 (counted, not searched)."""
    a1 = np.asarray(a1, dtype=np.float64)
    a2 = np.asarray(a2, dtype=np.float64)
    dirs = np.asarray(dirs, dtype=np.float64)
    p = dirs[0, 0] * a2
    q = dirs[0, 1] * a1
    flip = p < q
    b1 = np.where(flip, -a1, a1)
    b2 = np.where(flip, -a2, a2)
    sec = np.zeros(a1.shape, dtype=np.int64)
    for s in range(1, dirs.shape[0]):
        sec += (dirs[s, 0] * b2 >= dirs[s, 1] * b1)
    return np.where(p == q, 0, sec)


def sector_atan2(a1, a2, nangles, offset=0.0):
    """floor(((atan2(a2, a1) - theta_0) mod pi) / Delta) for uniform sectors."""
    t = np.mod(np.arctan2(a2, a1) - offset, np.pi)
    return np.minimum((t / (np.pi / nangles)).astype(np.int64), nangles - 1)


def plane(x, z, nlags, maxlag, dirs, basis=None, ptol=np.inf, estimator="matheron"):
    """x (n, d), d = 2 or 3, z (nz, n) -> count (nangles, nlags) int64, lagsum (nangles, nlags),
    zsum (nz, nangles, nlags), nduplicates."""
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(-1, x.shape[0])
    dirs = np.asarray(dirs, dtype=np.float64)
    n, d = x.shape
    nz, nang = z.shape[0], dirs.shape[0]
    nb = nang * nlags
    e2 = edges2(nlags, maxlag)
    count = np.zeros(nb, dtype=np.int64)
    lagsum = np.zeros(nb)
    zsum = np.zeros((nz, nb))
    ndup = 0
    ptol2 = np.float64(ptol) * np.float64(ptol)
    if d == 3:
        e = np.asarray(basis, dtype=np.float64).reshape(3, 3)
    for i0 in range(0, n - 1, ROWS):
        i1 = min(i0 + ROWS, n)
        rows = np.arange(i0, i1)[:, None]
        cols = np.arange(i0 + 1, n)[None, :]
        upper = cols > rows
        dl = [x[i0:i1, a][:, None] - x[i0 + 1:, a][None, :] for a in range(d)]
        d2 = dl[0] * dl[0]
        for a in range(1, d):
            d2 = d2 + dl[a] * dl[a]
        ndup += int(np.count_nonzero(upper & (d2 == 0.0)))
        keep = upper & (d2 > 0.0) & (d2 <= e2[nlags])
        if d == 2:
            a1, a2 = dl[0], dl[1]
        else:
            a1 = (dl[0] * e[0, 0] + dl[1] * e[0, 1]) + dl[2] * e[0, 2]
            a2 = (dl[0] * e[1, 0] + dl[1] * e[1, 1]) + dl[2] * e[1, 2]
            w = (dl[0] * e[2, 0] + dl[1] * e[2, 1]) + dl[2] * e[2, 2]
            keep &= (w * w <= ptol2)
        ii, jj = np.nonzero(keep)
        dk = d2[ii, jj]
        k = np.searchsorted(e2, dk, side="left") - 1
        b = sector(a1[ii, jj], a2[ii, jj], dirs) * nlags + k
        count += np.bincount(b, minlength=nb)
        lagsum += np.bincount(b, weights=np.sqrt(dk), minlength=nb)
        for c in range(nz):
            dz = z[c, i0 + ii] - z[c, i0 + 1 + jj]
            val = dz * dz if estimator == "matheron" else np.sqrt(np.abs(dz))
            zsum[c] += np.bincount(b, weights=val, minlength=nb)
    return count.reshape(nang, nlags), lagsum.reshape(nang, nlags), zsum.reshape(nz, nang, nlags), ndup


def aniso_model(kind, h, phi, nugget, sill, r1, r2, theta, nu=1.0):
    from variography_ref import shape
    x = h * np.sqrt(np.cos(phi - theta) ** 2 / r1 ** 2 + np.sin(phi - theta) ** 2 / r2 ** 2)
    return nugget + (sill - nugget) * shape(kind, x, nu)
