"""Cross-validation of cokriging under a moving neighbourhood on the device (gss_cokrig_cv_knn) against the numpy
reference tests/cokrig_cv_ref.py over the case table tests/cokrig_cv_cases.py.  Predictions and variances of every
sample: cokrig_cases.TOL (1 + |value|) in unit-sill scale (TOL_GAUSSIAN for the Gaussian structure, as in the other
cokriging tests); status, neighbour lists and counts: equal; tests/test_cokriging_cv_host.py keeps every per-sample
system under the conditioning cap that bar needs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cokrig_cases as CC
import cokrig_cv_cases as VC
import cokrig_cv_ref as VR
import cokrig_local_ref as LR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = {"ordinary": 1, "simple": 0}
CHUNK_ENV = "GSS_COKRIG_CHUNK_POINTS"


def close(a, b, tol=CC.TOL):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    err = np.where(np.isnan(b), 0.0, np.abs(a - b) / (1.0 + np.abs(b)))
    print("   max error %.3g (bar %.0e)" % (float(err.max()), tol))
    return bool(np.all(err <= tol))


def structure_of(s):
    import gss
    ctor = {"exponential": gss.ExponentialVariogram, "spherical": gss.SphericalVariogram, "matern": gss.MaternVariogram,
            "gaussian": gss.GaussianVariogram, "cubic": gss.CubicVariogram,
            "pentaspherical": gss.PentasphericalVariogram}[s["kind"]]
    kw = dict(order=s["nu"]) if s["kind"] == "matern" else {}
    if s["kind"] == "gaussian":
        kw["regularize"] = False
    if s.get("radii") is not None:
        return ctor(gss.MetricBall(tuple(s["radii"]), s.get("rotation")), **kw)
    return ctor(range=s["range"], **kw)


def handle_of(c, factor=False, keep=None):
    from gss.engine import HipEngine
    keep = slice(None) if keep is None else keep
    return HipEngine.cokrig(structure_of(c["structure"]), c["B0"], c["B1"], VARIANT[c["variant"]], c["x"][keep],
                            c["z"][keep], c["var"][keep], means=c["means"], factor=factor)


def run(h, c, fold="case", device=False):
    s = c["search"]
    fold = c["fold"] if isinstance(fold, str) else fold
    return h.cv_knn(c["k"], fold=fold, exclude_radius=c["exclude_radius"], minneighbors=s["minneighbors"],
                    radius=s["radius"], radii=s["radii"], return_idx=True, rotation=s["rotation"], device=device)


def reference(c):
    ref = VR.predict(LR.Model(c["structure"], c["B0"], c["B1"]), c["x"], c["z"], c["var"], c["k"], c["fold"],
                     c["exclude_radius"], c["variant"], c["means"], **c["search"])
    for a in ref:
        a.setflags(write=False)
    return ref


_cache = {}


def case(name):
    """The case, its reference answer (computed once, never modified) and the device's."""
    if name not in _cache:
        c = VC.CASES[name]()
        h = handle_of(c)
        got = run(h, c)
        h.close()
        _cache[name] = (c, reference(c), got)
    return _cache[name]


def agrees(name):
    c, (rp, rv, rst, ridx, rcnt), (pred, var, st, idx, cnt) = case(name)
    n, nz = c["x"].shape[0], len(c["k"])
    assert pred.shape == var.shape == st.shape == (n,) and idx.shape == (n, sum(c["k"])) and cnt.shape == (n, nz)
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt)
    assert np.array_equal(st, rst)
    fold = np.arange(n) if c["fold"] is None else c["fold"]
    for p in range(n):                                          # never the query itself, never a sample of its fold
        rows = idx[p][idx[p] >= 0]
        assert p not in rows and not np.any(fold[rows] == fold[p])
    tol = VC.tolerance(c)
    return close(pred, rp, tol) and close(var, rv, tol)


@pytest.mark.parametrize("key", sorted(VC.KERNELS))
def test_every_compiled_kernel(key):
    """One case per compiled cokrig_cv_kernel<DIM, KIND, NT> (tests/test_cokriging_cv_host.py holds the table against
    the library)."""
    assert agrees("kernel_%d_%d_%d" % key)


def test_leave_one_datum_out_meets_the_collocated_partner():
    assert agrees("datum_loo_collocated")
    c, _, (pred, var, st, idx, cnt) = case("datum_loo_collocated")
    # variable 1 sits on the first 60 locations of variable 0: rows p and 80 + p are partners, nearest of the other kind
    assert np.array_equal(idx[:60, 10], np.arange(80, 140)) and np.array_equal(idx[80:, 0], np.arange(60))


def test_location_folds_remove_the_partner():
    assert agrees("location_folds")
    c, _, (_, var, _, idx, _) = case("location_folds")
    assert not np.any(idx[:60] == np.arange(80, 140)[:, None])
    loo_var = case("datum_loo_collocated")[2][1]
    assert np.all(var[:60] > loo_var[:60])                      # without the partner the primary is known less well


def test_samples_exactly_on_the_exclusion_radius_are_left_out():
    assert agrees("ball_on_radius")
    c, _, (_, _, _, idx, _) = case("ball_on_radius")
    d2 = ((c["x"][:, None, :] - c["x"][None, :, :]) ** 2).sum(axis=2)
    assert np.all((d2 == 100.0).sum(axis=1) >= 2)
    for p in range(idx.shape[0]):
        assert np.all(d2[p, idx[p][idx[p] >= 0]] > 100.0)


def test_short_lists_ordinary_and_simple():
    """All four outcomes (tests/test_cokriging_cv_host.py asserts on the reference that each occurs)."""
    assert agrees("short_ok") and agrees("short_sk")
    c, _, (_, _, st, _, cnt) = case("short_ok")
    sts = case("short_sk")[2][2]
    v, K = c["var"], cnt.sum(axis=1)
    assert np.all(st[v == 1] == 1) and np.all(sts[(v == 1) & (K >= 2)] == 0)
    assert np.all(st[K < 2] == 1) and np.all(sts[K < 2] == 1)
    assert np.all(st[(v == 0) & (cnt[:, 1] == 0) & (K >= 2)] == 0)


def test_four_variables():
    assert agrees("four_vars")


def test_simple_variant_with_means():
    assert agrees("simple_means")


def test_rotated_structure_and_rotated_ball():
    assert agrees("rotated")
    cnt = case("rotated")[2][4]
    assert (cnt < 12).any() and (cnt.sum(axis=1) > 0).all()


@pytest.mark.parametrize("name", ["global_ok", "global_sk"])
def test_global_limit_agrees_with_the_folds_off_the_factor(name):
    """k[a] = every variable's count on a gss_cokrig_create_local handle against gss_krig_cv_global_folds on a
    gss_cokrig_create handle of the same samples and folds: two independent device paths."""
    assert agrees(name)
    c, _, (pred, var, st, _, _) = case(name)
    h = handle_of(c, factor=True)
    gp, gv, gst = h.cv_global_folds(c["fold"])
    fp, fv, fst = run(h, c)[:3]                                 # the moving neighbourhood on the fitted handle: same bits
    h.close()
    assert not gst.any() and not st.any()
    assert close(pred, gp) and close(var, gv)
    assert np.array_equal(fp, pred) and np.array_equal(fv, var)


def test_agreement_with_a_refit_per_fold():
    """Three folds of location_folds: a handle on the samples outside the fold and gss_cokrig_predict_knn at the fold's
    location give row v_p."""
    c, _, (pred, var, st, idx, _) = case("location_folds")
    s = c["search"]
    for f in (0, 37, 79):
        inside = c["fold"] == f
        rows = np.flatnonzero(inside)
        h = handle_of(c, keep=~inside)
        mu, vv, pst = h.predict_knn(c["x"][rows], c["k"], s["minneighbors"], s["radius"], s["radii"],
                                    rotation=s["rotation"])
        h.close()
        t = c["var"][rows]
        assert not pst[t, np.arange(rows.size)].any() and not st[rows].any()
        assert close(pred[rows], mu[t, np.arange(rows.size)]) and close(var[rows], vv[t, np.arange(rows.size)])
    assert np.flatnonzero(c["fold"] == 0).size == 2             # a collocated pair among the three


CHUNK_CHILD = """
import os, sys
import numpy as np
sys.path[:0] = [{tests!r}, {root!r}, os.path.join({root!r}, "geostatssolvers.jl_amd")]
import test_gpu_cokriging_cv as T
c = T.VC.CASES["chunks"]()
h = T.handle_of(c)
out = T.run(h, c)
h.close()
np.savez(sys.argv[1], *out)
"""


def test_chunks(tmp_path):
    """n = 600 under a cap of 256 samples (three chunks, set before the child's library reads it): the bits of one
    chunk."""
    assert agrees("chunks")
    one = case("chunks")[2]
    path = str(tmp_path / "chunks.npz")
    env = dict(os.environ, **{CHUNK_ENV: "256"})
    r = subprocess.run([sys.executable, "-c", CHUNK_CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT), path],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    for i, b in enumerate(one):
        assert np.array_equal(got["arr_%d" % i], b, equal_nan=True)


def test_two_runs_and_host_and_device_arrays_give_identical_bits():
    import torch
    c, _, first = case("four_vars")
    h = handle_of(c)
    again = run(h, c)
    dev = run(h, c, fold=torch.as_tensor(c["fold"], device="cuda"))
    torch.cuda.synchronize()
    h.close()
    for a, b, d in zip(first, again, dev):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(d.cpu().numpy(), a, equal_nan=True)


def _raw(h, c, fold=None, ex=-1.0, k=None, metric=0, minneighbors=1):
    from gss import _lib
    n = c["x"].shape[0]
    kk = np.ascontiguousarray(c["k"] if k is None else k, dtype=np.int32)
    pred, var = np.empty(n), np.empty(n)
    f = None if fold is None else np.ascontiguousarray(fold, dtype=np.int32)
    code = h._l.gss_cokrig_cv_knn(h._h, _lib.ptr(f), ctypes.c_double(ex), _lib.ptr(kk), minneighbors,
                                  ctypes.c_double(-1.0), None, metric, ctypes.c_double(0.0), _lib.ptr(pred),
                                  _lib.ptr(var), None, None, None, 0, None)
    return code, _lib.last_error()


def test_refusals():
    import gss
    from gss import _lib
    from gss.engine import KrigHandle
    c = VC.CASES["four_vars"]()
    h = handle_of(c)
    bad = c["fold"].copy()
    bad[7] = -1
    for kw, code, text in ((dict(fold=bad), _lib.ERR_INVALID, "fold id -1 of sample 7"),
                           (dict(ex=float("nan")), _lib.ERR_INVALID, "exclude_radius is NaN"),
                           (dict(k=(13, 9, 12, 16)), _lib.ERR_INVALID, r"k[0] = 13 outside 1 .. 12"),
                           (dict(k=(0, 9, 12, 16)), _lib.ERR_INVALID, r"k[0] = 0 outside"),
                           (dict(k=(12, 20, 20, 13)), _lib.ERR_UNSUPPORTED, "65 neighbours"),
                           (dict(metric=_lib.METRICS["haversine"]), _lib.ERR_UNSUPPORTED, "haversine")):
        got, msg = _raw(h, c, **kw)
        assert got == code and text in msg and "gss_cokrig_cv_knn" in msg, (kw, got, msg)
    with pytest.raises(_lib.GSSError, match="gss_cokrig_cv_knn") as e:   # the one-variable call keeps refusing the handle
        KrigHandle.cv_knn(h, 8)
    assert e.value.code == _lib.ERR_INVALID and "cokriging system" in str(e.value)
    h.close()
    k = KrigHandle(gss.ExponentialVariogram(range=25.0), 1, c["x"], c["z"], factor=False)
    got, msg = _raw(k, c)
    k.close()
    assert got == _lib.ERR_INVALID and "gss_cokrig_cv_knn" in msg and "not a cokriging system" in msg
    five = dict(c, B0=0.1 * np.eye(5), B1=CC.b1_of(5), var=np.arange(c["x"].shape[0], dtype=np.int32) % 5)
    h5 = handle_of(five, factor=True)
    got, msg = _raw(h5, five, k=(3, 3, 3, 3, 3))
    h5.close()
    assert got == _lib.ERR_UNSUPPORTED and "gss_cokrig_cv_knn" in msg and "5 variables" in msg


def test_profile_names():
    from gss import _lib
    c = VC.CASES["simple_means"]()
    h = handle_of(c)
    _lib.profile_enable(True)
    try:
        _lib.profile_reset()
        run(h, c)
        knn, cv = _lib.profile_read("knn"), _lib.profile_read("cokrig_cv")
    finally:
        _lib.profile_enable(False)
        h.close()
    assert knn[1] >= 1 and cv[1] >= 1 and cv[0] > 0.0


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def _twin_problem():
    import gss
    rng = np.random.default_rng(51)
    loc = CC.lattice((12, 10), 10.0, 52)
    cu = CC.values(loc, np.zeros(120, dtype=int), 53)
    zn = CC.values(loc, np.ones(120, dtype=int), 54)
    cu[rng.permutation(120)[:70]] = np.nan                      # sparse primary
    zn[::7] = np.nan
    data = gss.georef(dict(cu=cu, zn=zn), loc)
    B0, B1 = np.array([[0.1, 0.03], [0.03, 0.08]]), np.array([[0.9, 0.5], [0.5, 0.7]])
    lmc = gss.LMCModel(("cu", "zn"), "exponential", 25.0, 1.0, B0, B1, 0.0)
    ic, iz = np.flatnonzero(~np.isnan(cu)), np.flatnonzero(~np.isnan(zn))
    x = np.concatenate([loc[ic], loc[iz]])
    z = np.concatenate([cu[ic], zn[iz]])
    var = np.repeat([0, 1], [ic.size, iz.size]).astype(np.int32)
    return gss.EstimationProblem(data, gss.PointSet(loc[:2] + 1.0), ("cu", "zn")), lmc, (B0, B1, x, z, var)


def _location_fold(x, method):
    from gss.validation import location_ids
    ids, uniq = location_ids(x)
    return method.folds(uniq)[0][ids]


def test_twin_cverror_with_a_moving_neighbourhood():
    import gss
    problem, lmc, (B0, B1, x, z, var) = _twin_problem()
    got = gss.cverror(gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, maxneighbors=(8, 8)))), problem,
                      gss.KFoldValidation(5, rng=9))
    fold = _location_fold(x, gss.KFoldValidation(5, rng=9))
    pred, _, st, _, _ = VR.predict(LR.Model(dict(kind="exponential", range=25.0), B0, B1), x, z, var, (8, 8), fold)
    for a, v in enumerate(("cu", "zn")):
        ref = VR.fold_mean_mse(z[var == a], pred[var == a], st[var == a], fold[var == a])
        print("   cverror of %s: %.12g (reference %.12g)" % (v, got[v], ref))
        assert abs(got[v] - ref) <= 1e-9 * ref


def test_twin_cverror_under_the_global_neighbourhood():
    import gss
    from gss.engine import HipEngine
    problem, lmc, (B0, B1, x, z, var) = _twin_problem()
    got = gss.cverror(gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc))), problem, gss.KFoldValidation(5, rng=9))
    fold = _location_fold(x, gss.KFoldValidation(5, rng=9))
    h = HipEngine.cokrig(gss.ExponentialVariogram(range=25.0), B0, B1, 1, x, z, var)
    pred, _, st = h.cv_global_folds(fold)
    h.close()
    for a, v in enumerate(("cu", "zn")):
        ref = VR.fold_mean_mse(z[var == a], pred[var == a], st[var == a], fold[var == a])
        assert abs(got[v] - ref) <= 1e-9 * ref


def test_example_runs():
    """examples/cokriging_cv.py in a fresh process."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cokriging_cv.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("cverror of cu, maxneighbors")]
    print("\n".join("   " + ln for ln in lines))
    assert len(lines) == 2, r.stdout
    for ln in lines:
        co, alone = (float(v.split()[-1]) for v in ln.split(":")[1].split(","))
        assert 0.0 < co and 0.0 < alone
