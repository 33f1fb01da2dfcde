"""Moving-neighbourhood cokriging on the device (gss_cokrig_create_local, gss_cokrig_predict_knn) against the numpy
reference tests/cokrig_local_ref.py over the case table tests/cokrig_local_cases.py.  Means and variances of every
point: 1e-9 (1 + |value|) in unit-sill scale (cokrig_cases.TOL); neighbour lists and counts: equal to the brute-force
selection; tests/test_cokriging_local_host.py keeps every per-point system under the conditioning cap that bar needs."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cokrig_cases as CC
import cokrig_local_cases as LC
import cokrig_local_ref as LR
import cokrig_ref as CR

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


def handle_of(c, factor=False):
    from gss.engine import HipEngine
    return HipEngine.cokrig(structure_of(c["structure"]), c["B0"], c["B1"], VARIANT[c["variant"]], c["x"], c["z"],
                            c["var"], means=c["means"], factor=factor)


def run(h, c, xdom=None):
    s = c["search"]
    return h.predict_knn(c["xdom"] if xdom is None else xdom, c["k"], s["minneighbors"], s["radius"], s["radii"],
                         return_idx=True, rotation=s["rotation"])


_cache = {}


def case(name):
    """The case, its reference answer (computed once, never modified) and the device's."""
    if name not in _cache:
        c = LC.CASES[name]()
        ref = LR.predict(LR.Model(c["structure"], c["B0"], c["B1"]), c["x"], c["z"], c["var"], c["xdom"], c["k"],
                         c["variant"], c["means"], **c["search"])
        for a in ref:
            a.setflags(write=False)
        h = handle_of(c)
        got = run(h, c)
        h.close()
        _cache[name] = (c, ref, got)
    return _cache[name]


def agrees(name):
    c, (rmu, rvar, rst, ridx, rcnt), (mu, var, st, idx, cnt) = case(name)
    nz, m = len(c["k"]), c["xdom"].shape[0]
    assert mu.shape == var.shape == st.shape == (nz, m) and idx.shape == (m, sum(c["k"])) and cnt.shape == (m, nz)
    assert np.array_equal(idx, ridx) and np.array_equal(cnt, rcnt)
    assert np.array_equal(st, rst)
    return close(mu, rmu) and close(var, rvar)


@pytest.mark.parametrize("name", ["tiles_8_8", "tiles_9_8", "tiles_16_16", "tiles_17_16", "tiles_32_32"])
def test_tile_boundaries(name):
    assert case(name)[0]["xdom"].shape[0] == 5
    assert agrees(name)


def test_one_point():
    c = LC.CASES["tiles_9_8"]()
    _, (rmu, rvar, _, ridx, _), _ = case("tiles_9_8")
    h = handle_of(c)
    mu, var, st, idx, cnt = run(h, c, c["xdom"][3:4])
    h.close()
    assert mu.shape == (2, 1) and not st.any() and np.array_equal(idx, ridx[3:4])
    assert close(mu, rmu[:, 3:4]) and close(var, rvar[:, 3:4])


@pytest.mark.parametrize("key", sorted(LC.KERNELS))
def test_every_compiled_kernel(key):
    """One case per compiled cokrig_local_kernel<DIM, KIND, NT> (tests/test_cokriging_local_host.py holds the table
    against the library)."""
    assert agrees("kernel_%d_%d_%d" % key)


def test_four_variables_heterotopic_shuffled():
    assert agrees("four_vars")


def test_simple_variant_with_means():
    assert agrees("simple_means")


def test_rotated_structure():
    assert agrees("rotated")


def test_rotated_search_ball():
    """A rotated MetricBall as the neighbourhood: the searches run in the ball's own frame."""
    c = dict(LC.CASES["tiles_16_16"]())
    a = 0.5
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    c["search"] = dict(minneighbors=1, radius=None, radii=(45.0, 18.0), rotation=R)
    ref = LR.predict(LR.Model(c["structure"], c["B0"], c["B1"]), c["x"], c["z"], c["var"], c["xdom"], c["k"],
                     c["variant"], c["means"], **c["search"])
    h = handle_of(c)
    mu, var, st, idx, cnt = run(h, c)
    h.close()
    assert np.array_equal(idx, ref[3]) and np.array_equal(cnt, ref[4]) and np.array_equal(st, ref[2])
    assert (cnt < 16).any() and (cnt > 0).all()
    assert close(mu, ref[0]) and close(var, ref[1])


def test_short_lists_ordinary_and_simple():
    """A ball that leaves lists short: one variable absent (ordinary: that target MISSING, the other estimated; simple:
    both estimated), fewer than minneighbors in total (all MISSING), and full lists
    (test_cokriging_local_host.py asserts on the reference that each occurs)."""
    assert agrees("short_ok") and agrees("short_sk")
    st, cnt = case("short_ok")[2][2], case("short_ok")[2][4]
    sts = case("short_sk")[2][2]
    one = (cnt[:, 0] == 0) & (cnt.sum(axis=1) >= 2)
    assert one.any() and np.all(st[0, one] == 1) and np.all(st[1, one] == 0) and not sts[:, one].any()
    few = cnt.sum(axis=1) < 2
    assert few.any() and np.all(st[:, few] == 1) and np.all(sts[:, few] == 1)


def test_collocated_samples_and_points_on_samples():
    """Collocated pairs inside the tile take the cross nugget; a domain point on a sample of variable 0 reproduces that
    datum, variable 1 (not measured there) does not."""
    assert agrees("collocated")
    c, _, (mu, var, _, idx, _) = case("collocated")
    z0 = c["z"][62:67]
    assert np.array_equal(idx[:, 0], np.arange(62, 67))
    assert np.all(np.abs(mu[0] - z0) <= 1e-9 * (1.0 + np.abs(z0))) and np.all(var[0] <= 1e-9)
    assert np.all(var[1] > 1e-3)


@pytest.mark.parametrize("name", ["single_ok", "single_sk"])
def test_one_variable_is_moving_neighbourhood_kriging(name):
    import gss
    from gss.engine import KrigHandle
    assert agrees(name)
    c, _, (mu, var, st, idx, _) = case(name)
    vg = gss.ExponentialVariogram(range=c["structure"]["range"], sill=float(c["B0"][0, 0] + c["B1"][0, 0]),
                                  nugget=float(c["B0"][0, 0]))
    k = KrigHandle(vg, VARIANT[c["variant"]], c["x"], c["z"], mean=None if c["means"] is None else c["means"][0],
                   factor=False)
    kmu, kvar, kst, kidx, _ = k.predict_knn(c["xdom"], c["k"][0], return_idx=True)
    k.close()
    assert np.array_equal(idx, kidx) and not kst.any()
    assert close(mu[0], kmu) and close(var[0], kvar)


def test_intrinsic_model_is_autokrigeable():
    import gss
    from gss.engine import KrigHandle
    assert agrees("intrinsic")
    c, _, (mu, var, _, _, _) = case("intrinsic")
    for t in (0, 1):
        own = c["var"] == t
        vg = gss.SphericalVariogram(range=c["structure"]["range"], sill=float(c["B0"][t, t] + c["B1"][t, t]),
                                    nugget=float(c["B0"][t, t]))
        k = KrigHandle(vg, 1, c["x"][own], c["z"][own], factor=False)
        kmu, kvar, _ = k.predict_knn(c["xdom"], c["k"][t])
        k.close()
        assert close(mu[t], kmu) and close(var[t], kvar)


@pytest.mark.parametrize("name", ["global_ok", "global_sk"])
def test_global_limit(name):
    """k[a] = every variable's count: both creators give the same answers, equal to gss_cokrig_predict_global."""
    assert agrees(name)
    c, _, (mu, var, st, idx, cnt) = case(name)
    h = handle_of(c, factor=True)
    gmu, gvar, gst = h.predict_global(c["xdom"])
    fmu, fvar, fst, fidx, fcnt = run(h, c)
    h.close()
    assert np.array_equal(mu, fmu) and np.array_equal(var, fvar) and np.array_equal(idx, fidx)
    assert not gst.any() and close(mu, gmu) and close(var, gvar)


def test_refusals():
    import ctypes
    from gss import _lib
    from gss.engine import KrigHandle
    c = LC.CASES["four_vars"]()
    h = handle_of(c)
    n, nc = ctypes.c_int64(), ctypes.c_int32()
    _lib.check(h._l.gss_krig_info(h._h, ctypes.byref(n), ctypes.byref(nc)))
    assert (n.value, nc.value) == (162, 4)
    for call in (lambda: h.predict_global(c["xdom"]), h.cv_global, lambda: h.cv_global_folds(None)):
        with pytest.raises(_lib.GSSError, match="no factor") as e:
            call()
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.GSSError, match="cokriging system") as e:
        KrigHandle.predict_knn(h, c["xdom"], 8)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.GSSError, match="cokriging system"):
        h.cv_knn(8)
    with pytest.raises(_lib.GSSError, match=r"k\[0\] = 13 outside 1 .. 12") as e:
        h.predict_knn(c["xdom"], (13, 9, 12, 16))
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.GSSError, match="65 neighbours") as e:
        h.predict_knn(c["xdom"], (12, 20, 20, 13))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    h.close()


def test_host_and_device_arrays_give_identical_bits():
    import torch
    c, _, (mu, var, st, idx, cnt) = case("four_vars")
    h = handle_of(c)
    out = run(h, c, torch.as_tensor(c["xdom"], device="cuda"))
    torch.cuda.synchronize()
    h.close()
    for a, b in zip(out, (mu, var, st, idx, cnt)):
        assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)


@pytest.mark.parametrize("name", ["tiles_8_8", "rotated"])
def test_host_arrays_past_one_piece(name):
    """Host arrays longer than one piece of the host pipeline (131072 points; the last piece holds 300): the domain comes
    in and all five outputs leave piece by piece, and with the rotated structure every fetched piece is moved into the
    frame where it lands.  Model of the named small case over 300 + 1000 samples, k = (3, 4).  Equal bit for bit to the
    same call on device tensors (whole arrays; test_chunks: the answers do not depend on the chunking), and 64 of the
    points, the last one among them, agree with the reference."""
    import torch
    small = LC.CASES[name]()
    rng = np.random.default_rng(3100)
    loc = CC.lattice((37, 36), 10.0, 3101)
    loc = loc[rng.permutation(loc.shape[0])[:1300]]
    var = rng.permutation(np.repeat([0, 1], [300, 1000]))
    m = 131072 + 300
    xdom = rng.uniform(15.0, 335.0, (m, 2))
    c = LC._case(small["structure"], small["B0"], small["B1"], loc, var, xdom, (3, 4), 3102)
    h = handle_of(c)
    got = run(h, c)
    dev = run(h, c, torch.as_tensor(c["xdom"], device="cuda"))
    torch.cuda.synchronize()
    h.close()
    assert all(isinstance(a, np.ndarray) for a in got)
    assert got[0].shape == got[1].shape == got[2].shape == (2, m) and got[3].shape == (m, 7) and got[4].shape == (m, 2)
    for a, b in zip(got, dev):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)
    sel = np.concatenate([np.sort(rng.permutation(m - 1)[:63]), [m - 1]])
    rmu, rvar, rst, ridx, rcnt = LR.predict(LR.Model(c["structure"], c["B0"], c["B1"]), c["x"], c["z"], c["var"],
                                            c["xdom"][sel], c["k"], c["variant"], c["means"], **c["search"])
    assert (sel > 131072).any() and (sel < 131072).any()
    assert np.array_equal(got[3][sel], ridx) and np.array_equal(got[4][sel], rcnt) and np.array_equal(got[2][:, sel], rst)
    assert close(got[0][:, sel], rmu) and close(got[1][:, sel], rvar)


def test_chunks():
    """m = 600 under a cap of 256 points: three chunks, equal to the one-chunk answer bit for bit."""
    assert agrees("chunks")
    c, _, one = case("chunks")
    h = handle_of(c)
    os.environ[CHUNK_ENV] = "256"
    try:
        got = run(h, c)
    finally:
        del os.environ[CHUNK_ENV]
        h.close()
    for a, b in zip(got, one):
        assert np.array_equal(a, b)


def test_solver_on_a_grid_with_missing_rows():
    import gss
    rng = np.random.default_rng(51)
    loc = CC.lattice((9, 9), 2.5, 52)
    cu = np.sin(0.3 * loc[:, 0]) + 0.1 * rng.normal(size=81)
    zn = np.cos(0.2 * loc[:, 1]) + 0.1 * rng.normal(size=81)
    cu[rng.permutation(81)[:50]] = np.nan                     # sparse primary
    zn[::7] = np.nan
    data = gss.georef(dict(cu=cu, zn=zn), loc)
    B1, B0 = np.array([[0.9, 0.5], [0.5, 0.7]]), np.array([[0.1, 0.02], [0.02, 0.1]])
    lmc = gss.LMCModel(("zn", "cu"), "spherical", 8.0, 1.0, B0[::-1, ::-1], B1[::-1, ::-1], 0.0)
    grid = gss.CartesianGrid((12, 12), (0.0, 0.0), (1.5, 1.5))
    solver = gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, maxneighbors=dict(cu=6, zn=10), minneighbors=2,
                                                      neighborhood=gss.MetricBall(9.0))))
    sol = gss.solve(gss.EstimationProblem(data, grid, ("cu", "zn")), solver)
    assert sol.names() == ["cu", "cu_variance", "zn", "zn_variance"]
    ic, iz = np.flatnonzero(~np.isnan(cu)), np.flatnonzero(~np.isnan(zn))
    x = np.concatenate([loc[ic], loc[iz]])
    z = np.concatenate([cu[ic], zn[iz]])
    var = np.repeat([0, 1], [ic.size, iz.size]).astype(np.int32)
    rmu, rvar, rst, _, _ = LR.predict(LR.Model(dict(kind="spherical", range=8.0), B0, B1), x, z, var, grid.centroids(),
                                      (6, 10), minneighbors=2, radius=9.0)
    assert np.array_equal(np.isnan(sol["cu"]), rst[0] != 0) and np.array_equal(np.isnan(sol["zn"]), rst[1] != 0)
    assert close(sol["cu"], rmu[0]) and close(sol["zn"], rmu[1])
    assert close(sol["cu_variance"], rvar[0]) and close(sol["zn_variance"], rvar[1])


def test_example_runs():
    """examples/cokriging_local.py in a fresh process: more samples than the global fit is meant for."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cokriging_local.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("mean kriging variance of cu")]
    assert len(line) == 1, r.stdout
    co, alone = (float(v) for v in line[0].split(":")[1].replace("cokriging", "").replace("kriging alone", "").split(","))
    print("  ", line[0])
    assert co <= alone
