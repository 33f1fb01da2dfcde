"""Cross-validation of IDW and LWR on the device (gss_idw_cv / gss_lwr_cv) against refits with oracle.idw_lwr on the
eligible samples (tests/est_cv_ref.py).  Tolerances: the EXISTING_TOL of tests/search_cases.py -- relative to 1 + |value|,
IDW pred / dist 1e-10 and LWR pred / var 1e-9; status, lists and counts for equality.  The shapes are the smallest at
which each path can go wrong: both lane groupings of est_knn_kernel (k <= 16, 17 .. 64), passes of the search (k = 65,
n - 1), the self-join across EST_TILE = 1 024 and a 256-thread block at an n that is no multiple of 8.

The grids run every cell of (size, dimension, fold scheme) for IDW and for LWR -- the sizes of cases 1 and 2 and, for
the self-join, n = 70 and n = 1 100 -- exponents, weight functions and column counts cycling over the cells.  The LWR
cells listed in DROPPED are left out, by name: the condition of their designs exceeds COND_CAP, so the reference itself
is not good for the tolerance there.  tests/test_est_cv_host.py recomputes the condition of every LWR design of the grid
and holds the kept ones below the cap (oracle error ~ eps x 1e6 = 1e-10, a tenth of the bar).

CASES is also the table the census of the new kernel families is held against (tests/test_est_cv_host.py): `kernel_of`
restates the dispatch of est_cv_all_dev (csrc/idw_lwr.hip)."""
import functools
import os
import runpy
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import est_cv_ref as R
import search_cases as SC
from rotated_frame import rot2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"idw": SC.EXISTING_TOL["idw_mean"], "lwr": SC.EXISTING_TOL["lwr_mean"]}
assert TOL == {"idw": SC.EXISTING_TOL["idw_aux"], "lwr": SC.EXISTING_TOL["lwr_aux"]}
EXP, TRI = (0, 3.0, 2.0), (1, 0.0, 0.0)
FOLD_IDS = np.array([3, 7, 7000, 2 ** 30], dtype=np.int32)


def samples(n, dim, seed, nz=1):
    """n cells of the smallest lattice over [0, 10]^dim that holds them, drawn at random, each sample a quarter of the
    spacing at most off its cell centre: no two samples nearly coincide, so small LWR designs stay well conditioned."""
    rng = np.random.default_rng(seed)
    m = int(np.ceil(n ** (1.0 / dim) - 1e-9))
    cells = np.stack(np.unravel_index(rng.permutation(m ** dim)[:n], (m,) * dim), axis=1)
    x = (cells + 0.5 + rng.uniform(-0.25, 0.25, (n, dim))) * (10.0 / m)
    if dim == 2:
        x[:, 1] = x[:, 1] * 0.5                                   # valid (longitude, latitude) for the haversine cases
    z = np.stack([np.sin(0.7 * x.sum(axis=1) + c) + 0.3 * c * x[:, 0] + 0.1 * rng.normal(size=n) for c in range(nz)])
    return x, (z if nz > 1 else z[0])


def folds(kind, x, seed):
    import gss
    if kind == "loo":
        return None
    if kind == "ids":
        return np.ascontiguousarray(FOLD_IDS[np.random.default_rng(seed).integers(0, 4, x.shape[0])])
    return gss.BlockValidation(4.0 if x.shape[1] < 3 else 6.0).folds(x)[0]


def case(method, n, k, dim, fold, nz=1, exponent=1.0, weight=EXP, **search):
    return dict(method=method, n=n, k=k, dim=dim, fold=fold, nz=nz, exponent=exponent, weight=weight, search=search)


def _grid(sizes):
    out, i = [], 0
    for n, k in sizes:
        for dim in (1, 2, 3):
            for fold in ("loo", "ids", "block"):
                out.append(case("idw", n, k, dim, fold, nz=(1, 4, 5)[i % 3], exponent=(1.0, 2.0, 3.0)[(i // 3 + i) % 3]))
                out.append(case("lwr", n, k, dim, fold, nz=(1, 4, 5)[(i + 1) % 3], weight=(EXP, TRI)[i % 2]))
                i += 1
    return out


SEARCH_CASES = _grid([(37, 5), (37, 16), (130, 17), (130, 64)])            # 1: 16 and 64 lanes per point
LIST_CASES = [case("idw", 200, 65, 2, "ids", nz=5, exponent=2.0), case("lwr", 200, 65, 3, "loo"),            # 2
              case("idw", 200, 199, 1, "loo", exponent=3.0), case("lwr", 200, 199, 2, "block", nz=4, weight=TRI)]
ALL_CASES = _grid([(70, 70), (1100, 1100)]) + [                                                              # 3
    case("idw", 70, 70, d, "ids", exponent=e) for d in (1, 2, 3) for e in (1.0, 2.0)] + [                 # the fast kernel
    case("idw", 1100, 1100, 1, "block", exponent=2.0), case("idw", 1100, 1100, 2, "ids", exponent=1.0),
    case("idw", 1100, 1100, 3, "loo", exponent=1.0), case("idw", 1100, 1100, 3, "ids", exponent=2.0),
    case("idw", 70, 70, 3, "ids", exponent=2.0, distance="cityblock"),
    case("lwr", 70, 70, 1, "loo", distance="chebyshev"),
    case("idw", 70, 70, 2, "ids", exponent=1.0, distance=("haversine", 6371.0)),
    case("lwr", 70, 70, 2, "loo", nz=4, distance=("haversine", 6371.0)),
    case("idw", 70, 70, 2, "ids", exponent=1.0, radius=3.0, minneighbors=2),
    case("lwr", 70, 70, 3, "block", radii=(6.0, 5.0, 7.0), minneighbors=5),
    case("idw", 70, 70, 2, "loo", nz=4, exponent=2.0, radii=(4.0, 1.5), rotation=rot2(0.6)),
    case("lwr", 70, 70, 2, "ids", radii=(6.0, 2.5), rotation=rot2(-0.4), minneighbors=4)]
GRID = SEARCH_CASES + LIST_CASES + ALL_CASES


def kernel_of(c):
    """The instantiation of the new families a case with k == n runs on (None: the search path)."""
    if c["k"] < c["n"]:
        return None
    s = c["search"]
    plain = not any(key in s for key in ("distance", "radius", "radii"))
    if c["method"] == "idw" and c["nz"] == 1 and plain and c["exponent"] in (1.0, 2.0):
        return ("idw_cv_all_fast_kernel", (c["dim"], "true" if c["exponent"] == 1.0 else "false"))
    return ("est_cv_all_kernel", (c["dim"], 4 if c["nz"] > 1 else 1))


def ident(c):
    s = "-".join("%s" % (v if not isinstance(v, (tuple, np.ndarray)) else "x") for v in c["search"].values())
    return "%s-n%d-k%d-d%d-%s-nz%d-e%g-w%d%s" % (c["method"], c["n"], c["k"], c["dim"], c["fold"], c["nz"], c["exponent"],
                                                 c["weight"][0], "-" + "_".join(c["search"]) + s if c["search"] else "")


def problem_of(c):
    seed = zlib.crc32(ident(c).encode())                          # by what the case is, not by where it stands in the table
    x, z = samples(c["n"], c["dim"], seed, c["nz"])
    return x, z, folds(c["fold"], x, seed + 1)


# LWR cells of the grid that are not run, by name, with the largest 2-norm condition of the oracle's normal matrix over
# their samples (est_cv_ref.lwr_design_cond).  Five neighbours for up to four unknowns, one-sided at the edge of the
# samples or with the tricube weight zero on the farthest of them: beyond COND_CAP the oracle's own solve is no longer
# good for a tenth of the 1e-9 bar (error ~ eps x condition).  tests/test_est_cv_host.py recomputes every condition:
# exactly these cells exceed the cap.
COND_CAP = 1e6
DROPPED = {"lwr-n37-k5-d2-loo-nz4-e1-w1": 9.4e6, "lwr-n37-k5-d2-block-nz1-e1-w1": 4.0e6,   # tricube: 4 samples, 3 unknowns
           "lwr-n37-k5-d3-loo-nz4-e1-w0": 1.2e6,                                           # exp: 5 samples, 4 unknowns
           "lwr-n37-k5-d3-ids-nz5-e1-w1": 8.6e8}                                           # tricube: 4 samples, 4 unknowns
CASES = [c for c in GRID if ident(c) not in DROPPED]


@functools.lru_cache(maxsize=None)
def problem(i):
    return problem_of(CASES[i])


def split(search):
    s = dict(search)
    return s.pop("minneighbors", 1), s


def device(c, x, z, fold, k=None, **kw):
    from gss.engine import HipEngine
    minn, s = split(c["search"])
    fn = HipEngine.idw_cv if c["method"] == "idw" else HipEngine.lwr_cv
    est = dict(exponent=c["exponent"]) if c["method"] == "idw" else dict(weight=c["weight"])
    return fn(x, z, c["k"] if k is None else k, fold=fold, minneighbors=minn, **est, **s, **kw)


def reference(c, x, z, fold, **kw):
    minn, s = split(c["search"])
    return R.predict(c["method"], x, z, c["k"], fold, minneighbors=minn, exponent=c["exponent"], weight=c["weight"], **s,
                     **kw)


def check(method, got, want, what=""):
    tol = TOL[method]
    assert np.array_equal(got[2], want[2]), what + " status"
    for name, g, w in (("pred", got[0], want[0]), ("aux", got[1], want[1])):
        g, w = np.asarray(g), np.asarray(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)), what + " " + name
        err = np.nanmax(np.abs(g - w) / (1.0 + np.abs(w))) if np.any(~np.isnan(w)) else 0.0
        print("%s %s: largest error %.3g of %.1g" % (what, name, err, tol))
        assert err <= tol, (what, name, err)


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%03d-%s" % (i, ident(c)) for i, c in enumerate(CASES)])
def test_against_refits_on_the_eligible_samples(i):
    c = CASES[i]
    x, z, fold = problem(i)
    lists = c["k"] < c["n"]
    got = device(c, x, z, fold, return_idx=lists)
    want = reference(c, x, z, fold)
    assert np.asarray(got[0]).shape == np.asarray(z).shape
    check(c["method"], got, want, ident(c))
    if "minneighbors" not in c["search"]:
        assert not got[2].any()                                   # nothing missing or singular hides behind a NaN
    if lists:
        _, s = split(c["search"])
        idx, cnt = R.lists(x, c["k"], fold, **s)
        assert np.array_equal(got[3], idx) and np.array_equal(got[4], cnt)


@pytest.mark.parametrize("method", ["idw", "lwr"])
def test_both_paths_agree(method):                                                                           # 4
    c = case(method, 70, 69, 2, "loo", nz=4, exponent=3.0)
    x, z = samples(70, 2, 31, 4)
    a, b = device(c, x, z, None), device(c, x, z, None, k=70)
    check(method, a, b, "k = n - 1 against k = n")
    c1 = case(method, 70, 69, 3, "loo", exponent=2.0)            # ... and against the fast kernel
    x, z = samples(70, 3, 32)
    check(method, device(c1, x, z, None), device(c1, x, z, None, k=70), "one column")


@pytest.mark.parametrize("k", [8, 144])
@pytest.mark.parametrize("method", ["idw", "lwr"])
def test_exact_edges_of_the_exclusion_ball(method, k):                                                       # 5
    g = np.arange(12.0)
    x = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    z = np.sin(0.4 * x[:, 0]) + 0.05 * x[:, 1] ** 2
    p = 4 * 12 + 3                                                # the sample at (4, 3)
    elig = R.eligible(x, p, None, 5.0, lattice=True)
    at = lambda dx, dy: (4 + dx) * 12 + 3 + dy                    # noqa: E731
    assert not elig[at(3, 4)] and not elig[at(5, 0)] and elig[at(3, 5)] and elig[at(4, 4)] and not elig[p]
    c = case(method, 144, k, 2, "loo", exponent=2.0)
    got = device(c, x, z, None, exclude_radius=5.0, return_idx=k < 144)
    check(method, got, reference(c, x, z, None, exclude_radius=5.0, lattice=True), "ball of 5 on the lattice")
    assert not got[2].any()
    if k < 144:
        idx, cnt = R.lists(x, k, None, exclude_radius=5.0)
        assert np.array_equal(got[3], idx) and np.array_equal(got[4], cnt)
        d2 = ((x[got[3]] - x[:, None, :]) ** 2).sum(-1)
        assert d2.min() == 26.0                                   # (1, 5): the nearest lattice offset beyond 5; 25 never
    if method == "idw":
        assert np.allclose(got[1], np.sqrt(26.0), rtol=1e-15)


@pytest.mark.parametrize("n,k", [(41, 6), (41, 40), (41, 41), (81, 70), (81, 81)])
def test_duplicates_across_and_inside_folds(n, k):                                                           # 6
    """The last sample sits on sample 3: in another fold it is copied with dist = 0; in the query's own fold it is
    invisible.  k = 6 and 40: est_knn_kernel with 16 and 64 lanes; k = 70 of 81: the passes of the search and
    est_list_kernel; k = n with one column (Euclidean, exponent 2): the fast kernel, with four: the general one."""
    x, z = samples(n - 1, 2, 41)
    x, z = np.vstack([x, x[3]]), np.append(z, 9.0)
    fold = (np.arange(n) % 4).astype(np.int32)                    # 3 -> fold 3, n - 1 (40, 80) -> fold 0
    last = n - 1
    for nz in (1, 4):
        zz = z if nz == 1 else np.stack([z + c for c in range(nz)])
        c = case("idw", n, k, 2, "ids", nz=nz, exponent=2.0)
        pred, dist, st = device(c, x, zz, fold)
        pred = np.atleast_2d(pred)
        assert not st.any() and dist[3] == 0.0 and dist[last] == 0.0
        assert np.array_equal(pred[:, 3], np.atleast_2d(zz)[:, last]) and np.array_equal(pred[:, last], np.atleast_2d(zz)[:, 3])
        check("idw", (pred, dist, st), reference(c, x, np.atleast_2d(zz), fold), "duplicate across folds")
        same = fold.copy()
        same[last] = fold[3]
        pred, dist, st = device(c, x, zz, same)
        pred = np.atleast_2d(pred)
        assert not st.any() and dist[3] > 0.0 and dist[last] > 0.0 and np.all(np.isfinite(pred))
        assert np.all(pred[:, 3] != np.atleast_2d(zz)[:, last])
        check("idw", (pred, dist, st), reference(c, x, np.atleast_2d(zz), same), "duplicate inside the fold")


@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("method", ["idw", "lwr"])
def test_isolated_cluster_is_missing_and_nothing_else(method, k):                                            # 7
    x, z = samples(47, 2, 51)
    x, z = np.vstack([x, [[100.0, 100.0], [100.5, 100.0], [100.0, 100.5]]]), np.append(z, [1.0, 2.0, 3.0])
    fold = np.append(np.arange(47) % 5, [9, 9, 9]).astype(np.int32)
    c = case(method, 50, k, 2, "ids", radius=20.0)               # the cluster is more than 100 away from the rest
    pred, aux, st = device(c, x, z, fold)
    assert np.array_equal(np.flatnonzero(st), [47, 48, 49]) and np.all(st[47:] == R.MISSING)
    assert int((st == R.OK_).sum()) == 47 and np.all(np.isnan(pred[47:])) and np.all(np.isnan(aux[47:]))
    check(method, (pred, aux, st), reference(c, x, z, fold), "isolated cluster")


@pytest.mark.parametrize("k", [7, 30])
@pytest.mark.parametrize("method", ["idw", "lwr"])
def test_a_single_fold_leaves_nothing_to_predict_from(method, k):                                            # 8
    x, z = samples(30, 3, 61)
    pred, aux, st = device(case(method, 30, k, 3, "ids"), x, z, np.full(30, 5, dtype=np.int32))
    assert np.all(st == R.MISSING) and np.all(np.isnan(pred)) and np.all(np.isnan(aux))


@pytest.mark.parametrize("k,n", [(12, 90), (40, 90), (90, 90), (1100, 1100)])
@pytest.mark.parametrize("method", ["idw", "lwr"])
def test_split_identity(method, k, n):                                                                       # 9
    """Two folds: the predictions of fold 0 are the plain predict call with data = the samples of fold 1 and
    domain = the samples of fold 0 -- bit for bit on the search path (same lists, same kernel, same order of
    summation), within the tolerances for k == n (the self-join and the all-sample predict kernels sum alike but are
    different code)."""
    from gss.engine import HipEngine
    x, z = samples(n, 3, 71)
    fold = (np.random.default_rng(72).random(n) < 0.6).astype(np.int32)
    f0, f1 = fold == 0, fold == 1
    c = case(method, n, k, 3, "ids", exponent=2.0)
    pred, aux, st = device(c, x, z, fold)
    est = dict(exponent=2.0) if method == "idw" else dict(weight=EXP)
    plain = (HipEngine.idw if method == "idw" else HipEngine.lwr)(x[f1], z[f1], x[f0], min(k, int(f1.sum())), **est)
    if k < n:
        assert np.array_equal(pred[f0], plain[0]) and np.array_equal(aux[f0], plain[1])
        assert np.array_equal(st[f0], plain[2])
    else:
        check(method, (pred[f0], aux[f0], st[f0]), plain, "split identity, every sample")


def test_chunk_cap_and_determinism():                                                                        # 10
    """Explicit ids and leave-one-out (the search then takes the query's fold from qoff + p, the self-join from its
    index array), both lane groupings of est_knn_kernel, the list path and the self-join; chunks of 64 of 200."""
    x, z = samples(200, 3, 81, 4)
    runs = {}
    for method, fold in ((m, f) for m in ("idw", "lwr") for f in (folds("ids", x, 82), None)):
        for k in (16, 40, 65, 200):
            for nz in (1, 4):
                c = case(method, 200, k, 3, "ids", nz=nz, exponent=2.0)
                zz = z if nz == 4 else z[0]
                whole = device(c, x, zz, fold, return_idx=k < 200)
                again = device(c, x, zz, fold, return_idx=k < 200)
                os.environ["GSS_EST_CV_CHUNK"] = "64"
                try:
                    capped = device(c, x, zz, fold, return_idx=k < 200)
                finally:
                    del os.environ["GSS_EST_CV_CHUNK"]
                for a, b, d in zip(whole, again, capped):
                    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, d, equal_nan=True), (method, k, nz)
                runs[(method, fold is None, k, nz)] = whole
    assert not any(r[2].any() for r in runs.values())


@pytest.mark.parametrize("k", [12, 80])
@pytest.mark.parametrize("method", ["idw", "lwr"])
def test_device_and_host_arrays_and_no_status(method, k):                                                    # 11
    import torch
    from gss import _lib
    x, z = samples(80, 2, 91, 4)
    fold = folds("ids", x, 92)
    c = case(method, 80, k, 2, "ids", nz=4, exponent=3.0)
    host = device(c, x, z, fold, return_idx=k < 80)
    dev = device(c, torch.as_tensor(x, device="cuda"), torch.as_tensor(z, device="cuda"),
                 torch.as_tensor(fold, device="cuda"), return_idx=k < 80)
    assert all(t.is_cuda for t in dev)
    for a, b in zip(host, dev):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)
    dev = device(c, x, z, None, device=True)                      # leave-one-out with everything in HBM
    for a, b in zip(device(c, x, z, None), dev):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)
    # status == NULL through the C ABI
    pred, aux = np.empty_like(z), np.empty(80)
    extra = (3.0,) if method == "idw" else (0, 3.0, 2.0)
    fn = getattr(_lib.lib(), "gss_%s_cv" % method)
    _lib.check(fn(_lib.ptr(x), _lib.ptr(z), 80, 2, 4, _lib.ptr(fold), -1.0, k, 1, -1.0, None, 0, 0.0, *extra, _lib.ptr(pred),
                  _lib.ptr(aux), None, None, None, _lib.MEM_HOST, _lib.current_stream()))
    assert np.array_equal(pred, host[0]) and np.array_equal(aux, host[1])


@pytest.mark.parametrize("nmax", [12, None])
@pytest.mark.parametrize("method", ["kfold", "ball"])
def test_twin_end_to_end(method, nmax):                                                                      # 12
    import gss
    rng = np.random.default_rng(101)
    x = rng.uniform(0.0, 100.0, (300, 2))
    a = np.sin(0.05 * x[:, 0]) + np.cos(0.07 * x[:, 1]) + 0.1 * rng.normal(size=300)
    b = 0.5 * a + 0.02 * x[:, 0] + 0.1 * rng.normal(size=300)
    data = gss.georef(dict(a=a, b=b), gss.PointSet(x))
    make = (lambda: gss.KFoldValidation(10, rng=1)) if method == "kfold" else (lambda: gss.LeaveBallOut(5.0))
    for solver, name in ((gss.IDWSolver(a=dict(exponent=2, maxneighbors=nmax), b=dict(exponent=2, maxneighbors=nmax)), "idw"),
                         (gss.LWRSolver(a=dict(maxneighbors=nmax), b=dict(maxneighbors=nmax)), "lwr")):
        res = gss.cross_validate(data, solver, make())
        fold = make().folds(x)[0]
        zz = np.stack([a, b])
        want = R.predict(name, x, zz, 300 if nmax is None else nmax, fold, make().exclude_radius, exponent=2.0)
        for j, v in enumerate(("a", "b")):
            r = res[v]
            assert r.variance is None and not r.status.any() and list(r.aux) == ["%s_%s" % (v, solver.AUX)]
            check(name, (r.pred, r.aux["%s_%s" % (v, solver.AUX)], r.status), (want[0][j], want[1], want[2]), v)
            e2 = (zz[j] - r.pred) ** 2
            mse = np.mean(e2) if fold is None else np.mean([np.mean(e2[fold == f]) for f in range(10)])
            assert r.summary.cverror == pytest.approx(mse, rel=1e-12) and r.summary.mse_std_n == 0.0
            assert np.isnan(r.summary.mean_std) and r.summary.n_ok == 300.0
        assert gss.cverror(solver, gss.EstimationProblem(data, gss.PointSet(x[:1]), ("a", "b")), make()) == \
            {v: res[v].summary.cverror for v in ("a", "b")}


def test_haversine_search_is_refused_as_for_kriging():
    import gss
    x, z = samples(30, 2, 111)
    data = gss.georef(dict(z=z), gss.PointSet(x))
    with pytest.raises(gss._lib.GSSError, match="haversine"):
        gss.cross_validate(data, gss.IDWSolver(z=dict(maxneighbors=5, distance=("haversine", 6371.0))))
    assert not gss.cross_validate(data, gss.IDWSolver(z=dict(distance=("haversine", 6371.0))))["z"].status.any()


def test_example_compares_the_estimators():                                                                  # 13
    out = runpy.run_path(os.path.join(ROOT, "examples", "compare_estimators.py"))["out"]
    assert len(out) == 6
    for name, row in out.items():
        assert set(row) == {"10 folds", "ball of 5"}
        for v in row.values():
            assert np.isfinite(v) and v > 0.0, name
