"""numpy restatement of the declustering calls (include/gss.h "declustering"), written from the definition there:

  cell index along an axis   floor((x - o) / s), one FP64 subtraction and one IEEE division (numpy does exactly that)
  one grid                   np.unique over the rows of indices -> count per sample, number of occupied cells
  weights of a grid          n / (noccupied count_i), the integer product exact, one division
  origins of the sweep       o = lo - (s k) / noff, the product and the quotient rounded apart
  weights of a size          sum over k = 0 .. noff - 1 in ascending k, then / noff
  weighted mean              fsum(w_i z_i) / n
  nearest                    brute-force argmin of FP64 squared distances accumulated in dimension order, ties low

Also the shared inputs of tests/test_decluster_host.py and tests/test_gpu_decluster.py and the two derived bounds."""
import math

import numpy as np

MAX_INDEX = 1 << 21
U = 2.0 ** -53


def cell_indices(x, origin, sides):
    x = np.asarray(x, dtype=np.float64)
    d = x - np.asarray(origin, dtype=np.float64)[None, :]
    q = d / np.asarray(sides, dtype=np.float64)[None, :]
    idx = np.floor(q)
    assert np.all(idx >= 0) and np.all(idx < MAX_INDEX), "reference: an index outside [0, 2^21)"
    return idx.astype(np.int64)


def cell_counts(x, origin, sides):
    """(count per sample, number of occupied cells)"""
    idx = cell_indices(x, origin, sides)
    _, inv, cnt = np.unique(idx, axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    return cnt[inv].astype(np.int64), int(cnt.size)


def grid_weights(x, origin, sides):
    n = np.asarray(x).shape[0]
    cnt, nocc = cell_counts(x, origin, sides)
    prod = nocc * cnt                               # int64, exact
    return np.float64(n) / prod.astype(np.float64)


def origin_of(lo, sides, k, noff):
    shift = np.asarray(sides, dtype=np.float64) * np.float64(k)
    return np.asarray(lo, dtype=np.float64) - shift / np.float64(noff)


def size_weights(x, sides, noff):
    x = np.asarray(x, dtype=np.float64)
    lo = x.min(axis=0)
    acc = np.zeros(x.shape[0])
    for k in range(noff):
        acc = acc + grid_weights(x, origin_of(lo, sides, k, noff), sides)
    return acc / np.float64(noff)


def sweep(x, z, sides, noff, criterion="min"):
    """(weights of every size, wmean per size, best)"""
    x = np.asarray(x, dtype=np.float64)
    sides = np.asarray(sides, dtype=np.float64).reshape(-1, x.shape[1])
    n = x.shape[0]
    ws = [size_weights(x, s, noff) for s in sides]
    if z is None:
        return ws, None, 0
    wm = np.array([math.fsum(w * z) / n for w in ws])
    best = int(np.argmin(wm) if criterion == "min" else np.argmax(wm))      # the first that attains it
    return ws, wm, best


def weight_bound(noff):
    """relative: one rounded division per grid, a sum of noff positive terms, one more division; doubled"""
    return 2.0 * (noff + 2) * U


def wmean_bound(w, z, noff):
    n = len(w)
    return 2.0 * (n + noff + 4) * U * math.fsum(np.abs(w * z)) / n


def nearest_hits(x, lo, step, dims):
    """hits per sample: lattice points lo + (j + 1/2) step, axis 0 fastest, each to its nearest sample"""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    axes = [np.float64(lo[a]) + (np.arange(dims[a], dtype=np.float64) + 0.5) * np.float64(step[a]) for a in range(d)]
    mesh = np.meshgrid(*axes[::-1], indexing="ij")
    q = np.stack([m.ravel() for m in mesh[::-1]], axis=1)
    d2 = np.zeros((q.shape[0], n))
    for a in range(d):
        t = q[:, a:a + 1] - x[None, :, a]
        d2 = d2 + t * t
    near = np.argmin(d2, axis=1)                    # the first minimum: ties to the lower index
    return np.bincount(near, minlength=n).astype(np.int64)


# ---- shared inputs --------------------------------------------------------------------------------------------------
def lattice_points(n, dim, seed):
    """coordinates on a 2^-4 lattice over [0, 4)^dim with duplicates: with sides 2^-2 many samples sit exactly on edges"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 64, size=(n, dim)).astype(np.float64) / 16.0
    if n >= 4:
        x[n // 2] = x[0]                            # coincident samples
        x[n - 1] = x[1]
    return x


def clustered(dim, seed=7, n=1000):
    """A dense blob of high values on a sparse background: 700 of `n` samples in a ball of radius ~3 around the centre of
    [0, 100]^dim, the rest uniform.  Values: background around 1, blob around 10."""
    rng = np.random.default_rng(seed)
    nb = (7 * n) // 10
    blob = 50.0 + 3.0 * rng.standard_normal((nb, dim))
    back = rng.uniform(0.0, 100.0, (n - nb, dim))
    x = np.concatenate([blob, back])
    z = np.concatenate([10.0 + rng.standard_normal(nb), 1.0 + 0.1 * rng.standard_normal(n - nb)])
    p = rng.permutation(n)
    return np.ascontiguousarray(x[p]), np.ascontiguousarray(z[p])


SWEEP_SIZES = np.array([2.0, 5.0, 9.0, 14.0, 20.0, 27.0, 35.0])          # ncs = 7
SWEEP_CASES = [(dim, noff, crit) for dim in (2, 3) for noff in (1, 4, 5) for crit in ("min", "max")]


def sweep_sides(dim):
    return np.repeat(SWEEP_SIZES[:, None], dim, axis=1)
