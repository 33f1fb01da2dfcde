"""The references of tests/test_gpu_sgs_matrix.py, stage by stage, in numpy.longdouble (80-bit where this suite runs).

    lists    brute force: per node the (key, index)-ascending k nearest among the cells visited before it (or the k nearest
             cells of the whole domain, of which those are kept), inside the ball -- compared exactly;
    weights  from the DEVICE's lists: 80-bit covariances, an 80-bit Cholesky and the two substitutions give lambda and
             sigma = sqrt(sill - lambda . c0) (seq.jl:121-126); a node with too few neighbours or a pivot <= 0 draws from
             the marginal (seq.jl:107-109, 124-128);
    sweep    from the DEVICE's lists, weights and sigmas and the supplied normals: z = mean + sum_j w_j (z[nb_j] - mean) +
             sigma eps along the path, for all realisations at once -- a fixed recursion, whatever the conditioning.

oracle_* are the FP64 restatements (numpy.linalg as oracle/sgs.py uses it; a plain numpy recursion) whose error against
the above sets the bars of tests/sgs_cases.py (tools/sgs_matrix_oracle.py).  levels() and team_schedule() restate the
level schedule and the choice of the team kernel (csrc/sgs_levels.hip) on the CPU.  Test infrastructure only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgs_cases as SC
from rotated_frame import frame

LD = np.longdouble
UNIT = 2.0 ** -53
SEED = 977


def long_double_ok():
    """The guard of the matrix: long double must be finer than 1e-18 (x87 80-bit: 1.08e-19)."""
    return np.finfo(LD).eps < 1e-18


# ---- the inputs of a run -----------------------------------------------------------------------------------------------
def geometry(run):
    """Everything a run is built from, a function of the run alone: jittered cell centres (no two search keys tie, but
    for the coincident pair of a `fail` run), paths (npaths, N), data cells and values, supplied normals (R, N)."""
    from oracle.fftgs import grid_centroids
    dims = run.dims
    N = int(np.prod(dims))
    rng = np.random.default_rng([N, run.k, len(dims), run.nd])
    cent = grid_centroids(dims) + rng.uniform(-0.3, 0.3, (N, len(dims)))
    special = {}
    free = np.arange(N)
    if run.fail:
        # seq.jl:124-128 made certain: cells a < b share their coordinates next to T and the path ends a, b, T, so T's
        # two nearest neighbours are a and b, in index order, and the second pivot of its system is 1 - 1 * 1
        T, a, b = run.fail
        cent[a] = cent[T] + 0.01
        cent[b] = cent[a]
        special = dict(T=T, a=a, b=b)
        free = np.setdiff1d(free, [T, a, b])
    dl = np.asarray(run.data if run.data is not None else np.sort(rng.choice(free, run.nd, replace=False)), dtype=np.int64)
    assert dl.size == run.nd and not set(dl) & set(special.values())
    zd = rng.normal(size=run.nd)
    paths = []
    for p in range(run.npaths):
        if run.path == "linear":
            assert not run.fail
            paths.append(np.arange(N))
            continue
        body = rng.permutation(free)
        if run.first is not None:      # the node the path starts with
            body = np.concatenate([[run.first], body[body != run.first]])
        paths.append(np.concatenate([body, [special[x] for x in ("a", "b", "T")]]) if run.fail else body)
    noise = rng.normal(size=(run.R, N))
    return dict(N=N, cent=cent, paths=np.asarray(paths, dtype=np.int64), dl=dl, zd=zd, noise=noise, **special)


def ranks(path, dl, N):
    rk = np.empty(N, dtype=np.int64)
    rk[path] = np.arange(N)
    rk[dl] = -1
    return rk


def cov_coords(run, cent):
    """The coordinates the covariance is taken on: the variogram's frame where it is rotated (include/gss.h)."""
    return frame(cent, SC.ROT[cent.shape[1]]) if run.rotated else cent


# ---- lists -------------------------------------------------------------------------------------------------------------
def brute_lists(run, geo, path):
    """(idx (N, k) padded with -1, length of every list) by exhaustive search, keys as oracle/sgs.py takes them."""
    from oracle.kriging import metric_key
    cent, N, k = geo["cent"], geo["N"], run.k
    rk = ranks(path, geo["dl"], N)
    inv = None if run.ball_radii is None else 1.0 / np.asarray(run.ball_radii, dtype=np.float64)
    r2 = 1.0 if run.ball_radii is not None else (None if run.radius is None else float(run.radius) ** 2)
    idx = np.full((N, k), -1, dtype=np.int32)
    cnt = np.zeros(N, dtype=np.int32)
    for node in range(N):
        if rk[node] < 0:
            continue
        d2 = metric_key(cent, cent[node], None, inv)
        if run.mask_after:
            order = np.argsort(d2, kind="stable")[:k]
            order = order[rk[order] < rk[node]]
        else:
            cand = np.flatnonzero(rk < rk[node])
            order = cand[np.argsort(d2[cand], kind="stable")[:k]]
        if r2 is not None:
            order = order[d2[order] <= r2]
        cnt[node] = order.size
        idx[node, :order.size] = order
    return idx, cnt


def device_ncond(run, geo, cnt):
    """ncond as the weights kernels leave it: the length of the list, 0 where the node draws from the marginal."""
    nc = np.where(cnt >= max(run.nmin, 1), cnt, 0)
    if run.fail:
        nc[geo["T"]] = 0
    return nc


def levels(idx, cnt, path, rk):
    """Level of every node (data cells 0; 1 + the highest level among the list) and the number of levels."""
    lvl = np.zeros(rk.size, dtype=np.int64)
    for node in path:
        if rk[node] >= 0:
            lvl[node] = 1 + (lvl[idx[node, :cnt[node]]].max() if cnt[node] else 0)
    return lvl, int(lvl.max())


def team_schedule(run, lvl, L):
    """What sgs_team_schedule (csrc/sgs_levels.hip) decides: None, or (average level size, RL, cap, chunks)."""
    nsim = int(np.count_nonzero(lvl))
    avg = nsim / L if L else 0.0
    if not (run.npaths == 1 and run.k <= 64 and L > 0 and avg <= 128.0 and not run.env):
        return None
    rl = 64 if avg <= 14.0 else 32 if avg <= 28.0 else 16 if avg <= 56.0 else 8
    kp = (run.k + 3) & ~3
    kn = kp + 4 if kp % 8 == 0 else kp + 8
    cap = min(2560 // kn, 128, 1024 // rl)
    sizes = np.bincount(lvl, minlength=L + 1)[1:]
    return avg, rl, cap, int(np.sum((sizes + cap - 1) // cap)), int(sizes.max())


# ---- weights -----------------------------------------------------------------------------------------------------------
def covariance(run, a, b, dtype=LD):
    """C(a_i, b_j) = sill - gamma(h), gamma = (sill - nugget) f(h / range) + nugget (h > 0) (oracle/variogram.py)."""
    a, b = np.asarray(a, dtype=np.float64).astype(dtype), np.asarray(b, dtype=np.float64).astype(dtype)
    d = a[:, None, :] - b[None, :, :]
    if run.vg_radii is not None:
        d = d / np.asarray(run.vg_radii, dtype=np.float64).astype(dtype)
        rng_ = dtype(1)
    else:
        rng_ = dtype(run.range)
    h = np.sqrt(np.sum(d * d, axis=-1))
    x = h / rng_
    if run.kind == "exponential":
        f = 1 - np.exp(-3 * x)
    elif run.kind == "spherical":
        f = np.where(x < 1, dtype(3) / 2 * x - x ** 3 / 2, dtype(1))
    else:
        raise ValueError(run.kind)
    return dtype(run.sill) - ((dtype(run.sill) - dtype(run.nugget)) * f + dtype(run.nugget) * (h > 0))


def _cholesky(A):
    """Lower factor by columns in A's own precision; None at the first pivot that is not positive."""
    A = A.copy()
    n = A.shape[0]
    for j in range(n):
        if not A[j, j] > 0:
            return None
        A[j, j] = np.sqrt(A[j, j])
        if j + 1 < n:
            A[j + 1:, j] /= A[j, j]
            A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A)


def _solve_lower(L, b, trans):
    x = b.copy()
    n = L.shape[0]
    for j in (range(n - 1, -1, -1) if trans else range(n)):
        x[j] = x[j] / L[j, j]
        if trans:
            x[:j] -= L[j, :j] * x[j]
        else:
            x[j + 1:] -= L[j + 1:, j] * x[j]
    return x


def node_weights(run, X, node, nb, oracle=False):
    """(lambda, sigma) of one node from its list, or (None, sqrt(sill)) where it draws from the marginal.  oracle: FP64
    with numpy.linalg, as oracle/sgs.py; else long double."""
    smarg = np.sqrt(LD(run.sill))
    if nb.size < run.nmin or nb.size == 0:
        return None, smarg
    if oracle:
        C = covariance(run, X[nb], X[nb], np.float64)
        c0 = covariance(run, X[nb], X[node][None], np.float64)[:, 0]
        try:
            L = np.linalg.cholesky(C)
        except np.linalg.LinAlgError:
            return None, smarg
        lam = np.linalg.solve(L.T, np.linalg.solve(L, c0))
        return lam, np.sqrt(max(0.0, run.sill - lam @ c0))
    C = covariance(run, X[nb], X[nb])
    c0 = covariance(run, X[nb], X[node][None])[:, 0]
    L = _cholesky(C)
    if L is None:
        return None, smarg
    y = _solve_lower(L, c0, False)
    v = LD(run.sill) - y @ y
    return _solve_lower(L, y, True), np.sqrt(v if v > 0 else LD(0))


def checked_nodes(run, N):
    """Every node up to 64 neighbours; beyond: the nodes a workgroup takes on its second trip (index >= 1024), the node
    before each of them in the same workgroup, and every 16th."""
    if run.k <= 64:
        return np.arange(N)
    late = np.arange(1024, N)
    return np.unique(np.concatenate([late, late - 1024, np.arange(0, N, 16)]))


def weights(run, geo, idx, cnt, nodes, oracle=False):
    """{node: (lambda or None, sigma)} from the given lists."""
    X = cov_coords(run, geo["cent"])
    return {int(n): node_weights(run, X, n, idx[n, :cnt[n]], oracle) for n in nodes}


def weight_errors(run, got_w, got_sg, got_nc, ref):
    """Largest errors in units of 2^-53: lambda against max(1, max |lambda|), sigma against sqrt(sill); and the scale."""
    ew = es = 0.0
    scale = 1.0
    for n, (lam, sg) in ref.items():
        es = max(es, float(abs(LD(got_sg[n]) - sg)))
        if lam is None:
            assert got_nc[n] == 0, ("node %d draws from the marginal" % n, got_nc[n])
            continue
        assert got_nc[n] == lam.size, (n, got_nc[n], lam.size)
        s = max(1.0, float(np.max(np.abs(lam))))
        scale = max(scale, s)
        ew = max(ew, float(np.max(np.abs(got_w[n, :lam.size].astype(LD) - lam))) / s)
    return {"w": (ew / UNIT, scale), "sigma": (es / np.sqrt(run.sill) / UNIT, float(np.sqrt(run.sill)))}


# ---- sweep -------------------------------------------------------------------------------------------------------------
def sweep(run, path, rk, idx, nc, w, sg, eps, dl, zd, dtype=LD):
    """z (R, N): the recursion along the path from given lists, weights, sigmas and normals, terms in list order."""
    z = np.asarray(eps, dtype=np.float64).astype(dtype).T.copy()      # (N, R): a cell's slot holds its normal
    mean = dtype(run.mean)
    if len(dl):
        z[dl] = np.asarray(zd, dtype=np.float64).astype(dtype)[:, None]
    w = np.asarray(w, dtype=np.float64).astype(dtype)
    sg = np.asarray(sg, dtype=np.float64).astype(dtype)
    for node in path:
        if rk[node] < 0:
            continue
        c = nc[node]
        acc = w[node, :c] @ (z[idx[node, :c]] - mean) if c else 0
        z[node] = mean + acc + sg[node] * z[node]
    return z.T


def field_error(run, got, ref):
    scale = float(np.max(np.abs(ref - LD(run.mean))))
    return float(np.max(np.abs(got.astype(LD) - ref))) / scale / UNIT, scale


# ---- the FP64 oracle against the restatement (tools/sgs_matrix_oracle.py) ---------------------------------------------------
def oracle_errors(run):
    """{"w": (units, scale), "sigma": .., "z": ..} of the FP64 restatement on a run, and the nodes where its
    factorisation failed.  Lists: brute force; both sweeps run on the oracle's FP64 weights, as the device's sweep and
    its reference run on the device's."""
    geo = geometry(run)
    out = {"w": (0.0, 1.0), "sigma": (0.0, 1.0), "z": (0.0, 1.0)}
    failed = []
    for p, path in enumerate(geo["paths"]):
        rk = ranks(path, geo["dl"], geo["N"])
        idx, cnt = brute_lists(run, geo, path)
        sim = np.flatnonzero(rk >= 0)
        nodes = np.intersect1d(checked_nodes(run, geo["N"]), sim)
        orc = weights(run, geo, idx, cnt, sim, oracle=True)          # every node: LAPACK is quick
        failed += [(p, n) for n, (lam, _) in orc.items() if lam is None and cnt[n] >= max(run.nmin, 1)]
        ref = weights(run, geo, idx, cnt, nodes)
        w = np.zeros((geo["N"], run.k))
        sg = np.zeros(geo["N"])
        nc = np.zeros(geo["N"], dtype=np.int64)
        for n, (lam, s) in orc.items():
            sg[n] = float(s)
            if lam is not None:
                nc[n] = lam.size
                w[n, :lam.size] = lam
        e = weight_errors(run, w, sg, nc, ref)
        r0 = run.first_real - run.path_base
        rows = [r for r in range(run.R) if run.npaths == 1 or r0 + r == p]
        if rows:
            eps = geo["noise"][rows]
            zr = sweep(run, path, rk, idx, nc, w, sg, eps, geo["dl"], geo["zd"])
            zo = sweep(run, path, rk, idx, nc, w, sg, eps, geo["dl"], geo["zd"], np.float64)
            e["z"] = field_error(run, zo, zr)
        for q in e:
            out[q] = (max(out[q][0], e[q][0]), max(out[q][1], e[q][1]))
    return out, failed


# ---- the device --------------------------------------------------------------------------------------------------------
def _variogram(run):
    import gss
    ctor = dict(exponential=gss.ExponentialVariogram, spherical=gss.SphericalVariogram)[run.kind]
    if run.vg_radii is not None:
        return ctor(gss.MetricBall(tuple(run.vg_radii), SC.ROT[len(run.dims)] if run.rotated else None), sill=run.sill,
                    nugget=run.nugget)
    assert not run.rotated
    return ctor(range=run.range, sill=run.sill, nugget=run.nugget)


def device_run(run):
    """One run on the device (its environment switches are the caller's to set, before the library reads them): the
    lists, weights and sigmas of every path (each from a handle of that path alone; path 0 also from the handle that
    holds them all), the schedule, the field from the supplied normals and, where the run says so, from the device's own."""
    from gss.engine import SGSHandle
    geo = geometry(run)
    vg = _variogram(run)
    kw = dict(mean=run.mean, maxneighbors=run.k, minneighbors=run.nmin, radius=run.radius, radii=run.ball_radii,
              mask_after_search=run.mask_after)
    paths = geo["paths"]
    multi = run.npaths > 1
    arg = paths if multi else (None if run.path == "linear" else paths[0])
    h = SGSHandle(vg, geo["cent"], arg, geo["dl"], geo["zd"], path_base=run.path_base, **kw)
    sch = h.schedule()
    out = {"schedule": np.array([int(sch[q]) for q in SCHEDULE_KEYS], dtype=np.int64)}
    out["idx0"], out["nc0"], out["w0"], out["sg0"] = h.weights()
    out["z_noise"] = h.realize(0, run.first_real, run.R, noise=geo["noise"])
    if run.seeded:
        out["z_seeded"] = h.realize(SEED, run.first_real, run.R)
    h.close()
    if multi:
        for q in ("idx", "nc", "w", "sg"):
            out["multi_" + q] = out[q + "0"]
        for p in range(run.npaths):
            hp = SGSHandle(vg, geo["cent"], paths[p], geo["dl"], geo["zd"], **kw)
            out["idx%d" % p], out["nc%d" % p], out["w%d" % p], out["sg%d" % p] = hp.weights()
            hp.close()
    return out


SCHEDULE_KEYS = ("npaths", "levels", "team_chunks", "team_rl", "team_cap", "big", "big_lds")


def main(argv):
    """python sgs_matrix.py OUT.npz RUN ...: the device runs of a process of its own (switches read once per process)."""
    res = {}
    for name in argv[2:]:
        for q, v in device_run(SC.RUNS[name]).items():
            res[name + "/" + q] = v
    np.savez(argv[1], **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
