"""Problems and references for tests/search_cases.py: neighbour searches whose answer does not depend on rounding, and
IDW / LWR estimates at 50 digits.  This module calls neither the oracle nor the device.

Search geometry.  Every coordinate is an integer multiple of 2^-10 (GRID) below 2^10 in magnitude, anisotropic radii
are powers of two, and a rotated ball is turned by a signed permutation, so frame coordinates stay on the grid.  Then
every difference, product, square and sum of the ranking key (csrc/gss_internal.h, metric_key) is exact in FP64 --
`exactness` asserts it from the bit widths -- and the true ranking is the int64 ranking of the scaled integers:
the reference for query q is the first k samples in the sort by (integer key, index) after the ball and mask filters.
Points: a subsampled lattice (exact ties along every axis), dense clusters (uneven boxes in the index) and exact
duplicates, in a shuffled order.  Queries: samples, lattice midpoints, scattered points and far ones.

Haversine keys are not exact: they are evaluated with mpmath at 50 digits from the input doubles, and the point set is
accepted only if every pair of rank-adjacent distinct keys of every query differs by more than 2^-40 relative, so the
FP64 ranking is the true one; exact duplicates tie and the index decides.

Estimators: both outputs and the status of IDW (idw.jl:111-142) and LWR (lwr.jl:114-147) at 50 digits from the doubles
the device receives, on the reference neighbour lists above.
"""
from dataclasses import dataclass, field
from typing import Optional

import mpmath as mp
import numpy as np

Q = 10                       # coordinates are integers times 2^-Q
GRID = 2.0 ** -Q
HALF = 1 << 17               # samples lie within +-HALF grid units of the origin, queries within +-2 HALF
UNIT = 2.0 ** -53
DPS = 50
HAV_GAP = 2.0 ** -40
ROT = {2: ((0, -1), (1, 0)), 3: ((0, 0, -1), (-1, 0, 0), (0, 1, 0))}      # signed permutations, determinant +1


# ----------------------------------------------------------------------------------------------- geometry (integers)
def spacing_of(nl, dim):
    side = int(np.ceil(nl ** (1.0 / dim))) + 1
    sp = 1
    while (side // 2 + 1) * sp * 2 <= HALF:
        sp *= 2
    return side, sp


def points(n, dim, seed, dup=True):
    """(n, dim) int64 grid coordinates: lattice + clusters + duplicates, shuffled."""
    rng = np.random.default_rng(seed)
    nd = n // 16 if dup else 0
    nc = n // 4
    nl = n - nd - nc
    side, sp = spacing_of(nl, dim)
    cells = rng.choice(side ** dim, nl, replace=False)
    lat = np.stack([(cells // side ** a) % side for a in range(dim)], axis=1).astype(np.int64)
    lat = (lat - side // 2) * sp
    fine = max(1, sp // 16)
    R = max(8, int(np.ceil(max(nc, 1) ** (1.0 / dim))))
    centres = lat[rng.choice(nl, 3)]
    clu = centres[rng.integers(0, 3, nc)] + fine * rng.integers(-R, R + 1, (nc, dim))
    X = np.concatenate([lat, clu])
    if nd:
        X = np.concatenate([X, X[rng.choice(X.shape[0], nd)]])
    X = X[rng.permutation(n)]
    assert X.shape == (n, dim) and np.abs(X).max() <= HALF + R * fine
    return X, sp


def queries(m, X, sp, seed, far=True):
    """(m, dim) int64: samples (zero distances), lattice midpoints (exact ties), scattered points, far points."""
    rng = np.random.default_rng(seed + 7919)
    n, dim = X.shape
    out = np.empty((m, dim), dtype=np.int64)
    lo, hi = X.min(axis=0), X.max(axis=0)
    for j in range(m):
        t = j % 4
        if t == 0:
            out[j] = X[rng.integers(0, n)]
        elif t == 1:
            out[j] = X[rng.integers(0, n)] + (sp // 2) * rng.integers(-1, 2, dim)
        elif t == 2 or not far:
            out[j] = rng.integers(lo, hi + 1)
        else:
            out[j] = np.where(rng.integers(0, 2, dim) == 1, hi + HALF // 2 + rng.integers(0, HALF // 4),
                              lo - HALF // 2 - rng.integers(0, HALF // 4))
    return out


@dataclass
class Metric:
    """Ranking key on integers.  euclidean: sum (d_a^2 << shift_a), a sample is inside the ball when key <= thr."""
    name: str = "euclidean"
    shifts: Optional[np.ndarray] = None
    thr: Optional[int] = None
    rot: Optional[np.ndarray] = None       # d x d signed permutation: frame coordinates (x - origin) @ rot
    origin: Optional[np.ndarray] = None
    # the arguments the engine takes for the same ball
    radius: Optional[float] = None
    radii: Optional[tuple] = None
    rotation: Optional[tuple] = None


def make_metric(name, ball, ballx, sp, dim, X):
    mt = Metric(name=name)
    if not ball:
        return mt
    assert name == "euclidean"
    if ball == "radius":
        r = ballx * sp
        mt.thr, mt.radius = r * r, r * GRID
        return mt
    g = np.array([ballx * sp, max(ballx * sp // 2, 1), ballx * sp * 2][:dim], dtype=np.int64)     # powers of two
    assert all(int(v) & (int(v) - 1) == 0 for v in g)
    e = np.array([int(v).bit_length() - 1 for v in g])
    mt.shifts = 2 * (e.max() - e)
    mt.thr = 1 << int(2 * e.max())
    mt.radii = tuple(float(v) * GRID for v in g)
    if ball == "rotated":
        mt.rot = np.array(ROT[dim], dtype=np.int64)
        mt.origin = X[0].copy()
        mt.rotation = ROT[dim]
    return mt


def frame(mt, P):
    return P if mt.rot is None else (P - mt.origin) @ mt.rot


def exactness(mt, X, C):
    """The FP64 key of every (sample, query) pair is exact: |x| < 2^10 on the 2^-10 grid, and the widest intermediate,
    the sum of `dim` shifted squares of differences, stays below 2^53 grid quanta."""
    assert max(np.abs(X).max(), np.abs(C).max()) < 1 << (Q + 10)
    fx, fc = frame(mt, X), frame(mt, C)
    dbits = int(max(fx.max(), fc.max()) - min(fx.min(), fc.min())).bit_length()
    if mt.name == "euclidean":
        shift = 0 if mt.shifts is None else int(mt.shifts.max())
        assert 2 * dbits + shift + 2 <= 53, (dbits, shift)
        if mt.radius is not None:
            assert (mt.radius * mt.radius) == mt.thr * GRID * GRID       # r^2 itself is exact
    else:
        assert dbits + 2 <= 53


def int_keys(mt, fx, fq):
    d = fx - fq
    if mt.name == "euclidean":
        sq = d * d
        return (sq << mt.shifts).sum(axis=1) if mt.shifts is not None else sq.sum(axis=1)
    if mt.name == "cityblock":
        return np.abs(d).sum(axis=1)
    assert mt.name == "chebyshev"
    return np.abs(d).max(axis=1)


def ref_knn(mt, X, C, k, rank=None, qrank=None):
    """idx (m, k) int32 padded with -1, count (m,), and the keys of the listed neighbours (int64, -1 padded)."""
    fx, fc = frame(mt, X), frame(mt, C)
    m = C.shape[0]
    idx = np.full((m, k), -1, dtype=np.int32)
    keys = np.full((m, k), -1, dtype=np.int64)
    cnt = np.zeros(m, dtype=np.int32)
    for p in range(m):
        key = int_keys(mt, fx, fc[p])
        ok = np.ones(X.shape[0], dtype=bool)
        if mt.thr is not None:
            ok &= key <= mt.thr
        if rank is not None:
            ok &= rank < qrank[p]
        cand = np.flatnonzero(ok)
        if cand.size > k:
            kc = key[cand]
            cand = cand[kc <= np.partition(kc, k - 1)[k - 1]]
        order = cand[np.argsort(key[cand], kind="stable")][:k]          # cand ascends: ties go to the lower index
        idx[p, :order.size] = order
        keys[p, :order.size] = key[order]
        cnt[p] = order.size
    return idx, cnt, keys


def kd_groups(X):
    """Box group (4096 consecutive points of the k-d order) of every sample, by the ordering rule of kd_order in
    csrc/knn.hip: a range of more than 4096 points is cut at 4096 * ceil(groups / 2) points by the order along the
    widest axis of its bounding box, ties by index; the lowest axis wins equal extents.  (The device build follows the
    same cuts up to a 2^-32 quantisation of the position along the axis.)"""
    n = X.shape[0]
    perm = np.arange(n)

    def cut(lo, hi):
        count = hi - lo
        if count <= 4096:
            return
        left = 4096 * (((count + 4095) // 4096 + 1) // 2)
        P = X[perm[lo:hi]]
        axis = int(np.argmax(P.max(axis=0) - P.min(axis=0)))
        perm[lo:hi] = perm[lo:hi][np.lexsort((perm[lo:hi], P[:, axis]))]
        cut(lo, lo + left)
        cut(lo + left, hi)

    cut(0, n)
    group = np.empty(n, dtype=np.int64)
    group[perm] = np.arange(n) // 4096
    return group


# ----------------------------------------------------------------------------------------------- problems
@dataclass
class Problem:
    X: np.ndarray                 # samples, grid integers (haversine: None)
    C: np.ndarray                 # queries, grid integers
    x: np.ndarray                 # the doubles the device receives
    c: np.ndarray
    mt: Metric
    k: int
    check: np.ndarray             # queries the reference is evaluated on
    distance: object = None       # engine argument
    rank: Optional[np.ndarray] = None
    path: Optional[np.ndarray] = None
    dlocs: Optional[np.ndarray] = None
    z: Optional[np.ndarray] = None
    sp: int = 1
    extra: dict = field(default_factory=dict)


def haversine_points(n, m, seed):
    rng = np.random.default_rng(seed)
    x = np.c_[rng.uniform(-180, 180, n), rng.uniform(-80, 80, n)]
    x[n - n // 16:] = x[rng.choice(n - n // 16, n // 16)]              # exact duplicates
    c = np.c_[rng.uniform(-180, 180, m), rng.uniform(-85, 85, m)]
    c[::4] = x[rng.choice(n, c[::4].shape[0])]
    return x, c


def haversine_keys(x, q):
    mp.mp.dps = DPS
    D = mp.pi / 180
    out = []
    for xi in x:
        s1 = mp.sin((mp.mpf(q[1]) - mp.mpf(xi[1])) / 2 * D)
        s2 = mp.sin((mp.mpf(q[0]) - mp.mpf(xi[0])) / 2 * D)
        out.append(s1 * s1 + mp.cos(mp.mpf(xi[1]) * D) * mp.cos(mp.mpf(q[1]) * D) * s2 * s2)
    return out


def ref_knn_haversine(x, c, k):
    """Lists by (50-digit key, index); asserts that the FP64 ranking cannot differ: rank-adjacent keys of the first k + 1
    are equal because the samples are (exact duplicates) or more than 2^-40 apart relative.  No query is excluded."""
    m, n = c.shape[0], x.shape[0]
    idx = np.full((m, k), -1, dtype=np.int32)
    keys = []
    for p in range(m):
        key = haversine_keys(x, c[p])
        order = sorted(range(n), key=lambda i: (key[i], i))
        for a, b in zip(order[:k], order[1:k + 1]):
            if np.array_equal(x[a], x[b]):
                continue
            assert key[b] - key[a] > HAV_GAP * key[b], ("haversine keys too close: change the point set", p, a, b)
        idx[p] = order[:k]
        keys.append([key[i] for i in order[:k]])
    return idx, np.full(m, k, dtype=np.int32), keys


def problem_of(case):
    seed = 1000 * case.dim + case.n + 17 * case.k + len(case.metric)
    if case.metric == "haversine":
        x, c = haversine_points(case.n, case.m, seed)
        p = Problem(None, None, x, c, Metric(name="haversine"), case.k, np.arange(case.m),
                    distance=("haversine", 6371.0))
    else:
        X, sp = points(case.n, case.dim, seed)
        masked = case.op == "masked"
        C = X if masked else queries(case.m, X, sp, seed, far=case.op in ("search",) or bool(case.ball))
        mt = make_metric(case.metric, case.ball, case.ballx, sp, case.dim, X)
        if "tie64" in case.expect:     # a query on a sample whose 64th and 65th neighbours tie in key
            for i in range(case.n):
                kk = ref_knn(mt, X, X[i:i + 1], 65)[2][0]
                if kk[63] == kk[64] and kk[62] != kk[63] and kk[64] >= 0:
                    C[0] = X[i]
                    break
        exactness(mt, X, C)
        m = C.shape[0]
        check = np.arange(m)
        if m > 4500:                   # large sets: a fixed sample of the queries, among them the extreme corners, where the
                                       # k-d order (always the upper side of the widest axis last) puts its last box groups
            rng = np.random.default_rng(seed + 1)
            s = C.sum(axis=1)
            corners = np.concatenate([np.argsort(s, kind="stable")[-40:], np.argsort(s, kind="stable")[:10]])
            check = np.unique(np.concatenate([rng.choice(m, 350, replace=False), corners]))
        p = Problem(X, C, X * GRID, C * GRID, mt, case.k, check, sp=sp,
                    distance=None if case.metric == "euclidean" else case.metric)
        if masked:
            rng = np.random.default_rng(seed + 2)
            if case.path == "sweep":   # lexicographic sweep: far batches stay wholly unsimulated for most of the visit
                path = np.lexsort(tuple(X[:, a] for a in reversed(range(case.dim))))
            else:
                path = rng.permutation(case.n)
            p.path = path.astype(np.int64)
            p.dlocs = np.sort(rng.choice(case.n, case.nd, replace=False)).astype(np.int64)
            rank = np.empty(case.n, dtype=np.int64)
            rank[path] = np.arange(case.n)
            rank[p.dlocs] = -1
            p.rank = rank
    if case.op in ("idw", "lwr"):
        rng = np.random.default_rng(seed + 3)
        x = p.x
        z = np.stack([np.sin(x[:, 0] * (0.7 + 0.2 * j) / max(np.abs(x).max(), 1.0) * 3.0) + 0.25 * x.sum(axis=1) /
                      max(np.abs(x).max(), 1.0) + 0.1 * rng.normal(size=x.shape[0]) + j for j in range(case.nz)])
        p.z = z[0] if case.nz == 1 else z
    return p


def reference_lists(p):
    """(idx, count, keys) of the checked queries."""
    if p.mt.name == "haversine":
        return ref_knn_haversine(p.x, p.c[p.check], p.k)
    qrank = None if p.rank is None else p.rank[p.check]
    return ref_knn(p.mt, p.X, p.C[p.check], p.k, p.rank, qrank)


def assert_expectations(case, p, idx, cnt, keys):
    """The edges a case claims (search_cases.Case.expect) are present in its reference answer."""
    k = p.k
    for e in case.expect:
        if e == "tie64":
            assert any(c > 64 and kk[63] == kk[64] for c, kk in zip(cnt, keys)), e
        elif e == "boundary":
            assert any((kk[:c] == p.mt.thr).any() for c, kk in zip(cnt, keys)), e
        elif e == "short":
            assert ((cnt > 0) & (cnt < k)).any(), e
        elif e == "empty":
            assert (cnt == 0).any(), e
        elif e == "full":
            assert (cnt == k).any(), e
        elif e == "rank0":
            assert p.dlocs.size == 0 and cnt[p.path[0]] == 0 and p.rank[p.path[0]] == 0, e
        elif e == "ties":
            assert any((np.diff(kk[:c]) == 0).any() for c, kk in zip(cnt, keys) if c > 1), e
        elif e == "on_sample":
            assert any(c > 0 and kk[0] == 0 for c, kk in zip(cnt, keys)), e
        elif e == "last_group":    # neighbours in box groups 64 and up: the second round of the box-group loop
            group = kd_groups(p.X)
            assert group.max() >= 64 and any((group[ii[:c]] >= 64).any() for c, ii in zip(cnt, idx)), e
        elif e == "missing":
            assert (cnt < case.minn).any() and (cnt >= case.minn).any(), e
        else:
            raise AssertionError("unknown expectation %r" % e)


# ----------------------------------------------------------------------------------------------- estimators, 50 digits
def _mp_dist(p, xi, q):
    name = p.mt.name
    d = [mp.mpf(float(a)) - mp.mpf(float(b)) for a, b in zip(xi, q)]
    if name == "euclidean":
        if p.mt.radii is not None:
            d = [t / mp.mpf(r) for t, r in zip(d, p.mt.radii)]
        return mp.sqrt(sum(t * t for t in d))
    if name == "cityblock":
        return sum(abs(t) for t in d)
    if name == "chebyshev":
        return max(abs(t) for t in d)
    raise AssertionError(name)


def mp_estimate(case, p, idx, cnt, hkeys=None):
    """(mean (nz, m), aux (m,), status (m,)) as float64 roundings of the 50-digit values; NaN where the status is set."""
    mp.mp.dps = DPS
    assert p.mt.rot is None
    z = np.atleast_2d(p.z)
    nz, m, dim = z.shape[0], len(p.check), p.x.shape[1]
    mean = np.full((nz, m), np.nan)
    aux = np.full(m, np.nan)
    st = np.zeros(m, dtype=np.uint8)
    for j in range(m):
        q = p.c[p.check[j]]
        nb = [int(i) for i in idx[j, :cnt[j]]]
        if len(nb) < case.minn or len(nb) < 1:
            st[j] = 1
            continue
        if p.mt.name == "haversine":
            d = [2 * mp.mpf(p.distance[1]) * mp.asin(min(mp.sqrt(kk), mp.mpf(1))) for kk in hkeys[j][:len(nb)]]
        else:
            d = [_mp_dist(p, p.x[i], q) for i in nb]
        if case.op == "idw":
            zero = [t for t, dd in enumerate(d) if dd == 0]
            if zero:
                mean[:, j] = z[:, nb[zero[0]]]
                aux[j] = 0.0
                continue
            w = [1 / dd ** mp.mpf(case.exponent) for dd in d]
            sw = sum(w)
            for cz in range(nz):
                mean[cz, j] = float(sum(wi * mp.mpf(float(z[cz, i])) for wi, i in zip(w, nb)) / sw)
            aux[j] = float(min(d))
            continue
        dmax = max(d)
        assert dmax > 0
        kind, a, pw = case.weight
        if kind == 1:
            w = [(1 - (dd / dmax) ** 3) ** 3 for dd in d]
        else:
            w = [mp.exp(-mp.mpf(a) * (dd / dmax) ** mp.mpf(pw)) for dd in d]
        U = [[mp.mpf(1)] + [mp.mpf(float(p.x[i][t])) - mp.mpf(float(q[t])) for t in range(dim)] for i in nb]
        NP = dim + 1
        A = mp.matrix(NP, NP)
        for wi, u in zip(w, U):
            for r in range(NP):
                for s in range(NP):
                    A[r, s] += wi * u[r] * u[s]
        e1 = mp.matrix([1] + [0] * dim)
        av = mp.lu_solve(A, e1)
        for cz in range(nz):
            b = mp.matrix(NP, 1)
            for wi, u, i in zip(w, U, nb):
                for r in range(NP):
                    b[r] += wi * u[r] * mp.mpf(float(z[cz, i]))
            mean[cz, j] = float(mp.lu_solve(A, b)[0])
        aux[j] = float(mp.sqrt(sum((wi * sum(u[r] * av[r] for r in range(NP))) ** 2 for wi, u in zip(w, U))))
    return mean, aux, st


def design_condition(case, p, idx, cnt):
    """Largest FP64 condition number of the centred, scaled weighted design of the LWR points that have an estimate."""
    worst = 0.0
    for j in range(len(p.check)):
        nb = idx[j, :cnt[j]]
        if nb.size < max(case.minn, 1):
            continue
        u = p.x[nb] - p.c[p.check[j]]
        s = np.abs(u).max()
        X = np.c_[np.ones(nb.size), u / (s if s > 0 else 1.0)]
        worst = max(worst, float(np.linalg.cond(X.T @ X)))
    return worst


def scales(case, p, rmean, raux):
    """Data scales of the two outputs: the largest |value|, and the largest finite auxiliary output (at least 1)."""
    finite = raux[np.isfinite(raux)]
    return float(np.abs(p.z).max()), max(1.0, float(np.abs(finite).max()) if finite.size else 1.0)


def units(got, ref, scale):
    """Largest error in units of 2^-53 scale over the entries the reference defines; NaN patterns must agree."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern"
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok])) / (UNIT * scale)) if ok.any() else 0.0
