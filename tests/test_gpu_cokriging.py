"""Cokriging on the device (gss_cokrig_create, gss_cokrig_predict_global; cross-validation through gss_krig_cv_global
and gss_krig_cv_global_folds) against the numpy reference tests/cokrig_ref.py over the case table
tests/cokrig_cases.py.  Means and variances: 1e-9 (1 + |value|) in units where the largest diagonal of B0 + B1 is 1
(DESIGN.md section 3); tests/test_cokriging_host.py keeps every case's condition number under the cap that bar needs.
The Gaussian case is held at 1e-6."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cokrig_cases as CC
import cokrig_kernel_cases as KC
import cokrig_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = {"ordinary": 1, "simple": 0}
CHUNK_ENV = "GSS_COKRIG_CHUNK_POINTS"


def close(a, b, tol=CC.TOL):
    a, b = np.asarray(a), np.asarray(b)
    err = np.abs(a - b) / (1.0 + np.abs(b))
    print("   max error %.3g (bar %.0e)" % (float(err.max()), tol))
    return bool(np.all(err <= tol))


def structure_of(s):
    """cokrig_ref structure keywords -> the package's variogram model (only its shape is read)."""
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


def handle_of(c, **kw):
    from gss.engine import HipEngine
    return HipEngine.cokrig(structure_of(c["structure"]), c["B0"], c["B1"], VARIANT[c["variant"]], c["x"], c["z"],
                            c["var"], means=c["means"], **kw)


_cache = {}


def case(name):
    """The case, its reference answer (computed once, never modified) and the device's."""
    if name not in _cache:
        c = {**CC.CASES, **CC.GAUSSIAN}[name]()
        model = CR.Model(c["structure"], c["B0"], c["B1"])
        ref = CR.predict(model, c["x"], c["z"], c["var"], c["xdom"], c["variant"], c["means"])
        for a in ref:
            a.setflags(write=False)
        h = handle_of(c)
        got = h.predict_global(c["xdom"])
        h.close()
        _cache[name] = (c, model, ref, got)
    return _cache[name]


@pytest.mark.parametrize("name", ["iso2d", "hetero3d", "many1d", "simple_means", "on_samples", "rotated"])
def test_predict_matches_the_reference(name):
    c, _, (rmu, rvar), (mu, var, st) = case(name)
    nz, m = c["B1"].shape[0], c["xdom"].shape[0]
    assert mu.shape == var.shape == st.shape == (nz, m)
    assert not st.any()
    assert close(mu, rmu) and close(var, rvar)


@pytest.mark.parametrize("key", sorted(KC.KERNELS), ids=lambda key: "%d_%d" % key)
def test_every_compiled_rhs_kernel(key):
    """Every entry of tests/cokrig_kernel_cases.py (one per compiled cokrig_rhs_kernel<DIM, KIND>;
    tests/test_cokrig_census.py holds the table against the built library and every entry under the conditioning cap):
    means, variances and statuses of all 517 points and every target, and the zero-key select at the points that sit
    on a sample of one variable."""
    c = KC.KERNELS[key]()
    rmu, rvar = CR.predict(KC.model_of(c), c["x"], c["z"], c["var"], c["xdom"], c["variant"], c["means"])
    h = handle_of(c)
    mu, var, st = h.predict_global(c["xdom"])
    h.close()
    nz, m = c["B1"].shape[0], c["xdom"].shape[0]
    assert mu.shape == var.shape == st.shape == (nz, m)
    assert not st.any()
    assert close(mu, rmu) and close(var, rvar)
    for p, j in enumerate(c["on"]):                            # point p is the location of sample j
        a, zj = int(c["var"][j]), float(c["z"][j])
        assert abs(mu[a, p] - zj) <= 1e-9 * (1.0 + abs(zj)) and var[a, p] <= 1e-9
        others = [t for t in range(nz) if t != a]
        assert np.all(var[others, p] > 1e-3)                  # not measured there: estimated, held by the reference


def test_handle_info_and_refusals():
    """n stacked samples and nc = nz; every single-variable entry point refuses the handle and names the call to use."""
    import ctypes
    from gss import _lib
    c = CC.hetero3d()
    h = handle_of(c)
    n, nc = ctypes.c_int64(), ctypes.c_int32()
    _lib.check(h._l.gss_krig_info(h._h, ctypes.byref(n), ctypes.byref(nc)))
    assert (n.value, nc.value) == (135, 3)
    from gss.engine import KrigHandle
    calls = [lambda: KrigHandle.predict_global(h, c["xdom"]), lambda: h.predict_knn(c["xdom"], 8),
             lambda: h.cv_knn(8), lambda: h.set_block_support((1.0, 1.0, 1.0), 2),
             lambda: h.predict_global_batch(c["xdom"], c["z"][None, :])]
    for call in calls:
        with pytest.raises(_lib.GSSError, match="gss_cokrig_predict_global") as e:
            call()
        assert e.value.code == _lib.ERR_INVALID
    assert h.factor_tensor().numel() > 0                     # gss_krig_factor_buffer stays valid
    h.close()


@pytest.mark.parametrize("name", ["single_ok", "single_sk"])
def test_one_variable_is_kriging(name):
    """nz = 1 equals KrigHandle.predict_global with sill = b0 + b1 and nugget = b0, and the reference."""
    import gss
    from gss.engine import KrigHandle
    c, _, (rmu, rvar), (mu, var, _) = case(name)
    vg = gss.ExponentialVariogram(range=c["structure"]["range"], sill=float(c["B0"][0, 0] + c["B1"][0, 0]),
                                  nugget=float(c["B0"][0, 0]))
    k = KrigHandle(vg, VARIANT[c["variant"]], c["x"], c["z"], mean=None if c["means"] is None else c["means"][0])
    kmu, kvar, _ = k.predict_global(c["xdom"])
    k.close()
    assert close(mu[0], kmu) and close(var[0], kvar)
    assert close(mu, rmu) and close(var, rvar)


def test_intrinsic_model_is_autokrigeable():
    """B0 = 0.2 B1 on isotopic data: each cokriged mean is that variable's own ordinary kriging."""
    import gss
    from gss.engine import KrigHandle
    c, _, (rmu, rvar), (mu, var, _) = case("intrinsic")
    assert close(mu, rmu) and close(var, rvar)
    for t in (0, 1):
        own = c["var"] == t
        vg = gss.SphericalVariogram(range=c["structure"]["range"], sill=float(c["B0"][t, t] + c["B1"][t, t]),
                                    nugget=float(c["B0"][t, t]))
        k = KrigHandle(vg, 1, c["x"][own], c["z"][own])
        kmu, _, _ = k.predict_global(c["xdom"])
        k.close()
        assert close(mu[t], kmu)


def test_simple_variant_far_from_the_data():
    c, _, _, (mu, var, _) = case("simple_means")
    for t in (0, 1):
        assert np.all(np.abs(mu[t, -4:] - c["means"][t]) <= 1e-12)
        assert np.all(np.abs(var[t, -4:] - (c["B0"][t, t] + c["B1"][t, t])) <= 1e-12)


def test_domain_points_on_samples_of_one_variable():
    """The zero-key rule with the cross nugget: variable 0 reproduces its datum, variable 1 (not measured there) does
    not and matches the reference."""
    c, _, (rmu, rvar), (mu, var, _) = case("on_samples")
    z0 = c["z"][25:40]                                        # variable 0 at the domain's locations
    assert np.all(np.abs(mu[0] - z0) <= 1e-9 * (1.0 + np.abs(z0))) and np.all(var[0] <= 1e-9)
    assert close(mu[1], rmu[1]) and close(var[1], rvar[1])
    assert np.all(var[1] > 1e-3)


def test_gaussian_case():
    c, model, (rmu, rvar), (mu, var, _) = case("gaussian")
    print("   cond_2 = %.3g" % CR.cond(model, c["x"], c["var"], c["variant"]))
    assert close(mu, rmu, CC.TOL_GAUSSIAN) and close(var, rvar, CC.TOL_GAUSSIAN)


@pytest.mark.parametrize("device", [False, True])
def test_two_chunks(device):
    """The chunk loop past its first turn (cap of 256 points: 700 points are three chunks), host and device arrays:
    equal to the single-chunk answer bit for bit (the chunks are independent columns), hence to the reference."""
    import torch
    c, _, (rmu, rvar), (mu1, var1, _) = case("hetero3d")
    h = handle_of(c)
    os.environ[CHUNK_ENV] = "256"
    try:
        xd = torch.as_tensor(c["xdom"], device="cuda") if device else c["xdom"]
        mu, var, st = h.predict_global(xd)
        if device:
            torch.cuda.synchronize()
            mu, var, st = mu.cpu().numpy(), var.cpu().numpy(), st.cpu().numpy()
    finally:
        del os.environ[CHUNK_ENV]
        h.close()
    assert not st.any()
    assert np.array_equal(mu, mu1) and np.array_equal(var, var1)
    assert close(mu, rmu) and close(var, rvar)


def test_host_arrays_past_one_piece_travel_in_pieces():
    """More than 131 072 host points: the copies of the outputs' nz columns ride beside the computation, piece by
    piece; every column lands at its own offset."""
    c = CC.iso2d()
    rng = np.random.default_rng(31)
    xdom = rng.uniform(-5.0, 85.0, (131072 + 300, 2))
    model = CR.Model(c["structure"], c["B0"], c["B1"])
    rmu, rvar = CR.predict(model, c["x"], c["z"], c["var"], xdom)
    h = handle_of(c, async_fit=True)
    mu, var, st = h.predict_global(xdom)
    h.close()
    assert not st.any()
    assert close(mu, rmu) and close(var, rvar)


@pytest.mark.parametrize("name", ["iso2d", "hetero3d"])
def test_cross_validation_off_the_factor(name):
    """Leave-one-out and folds that keep collocated samples together, against refits of the reference; fold = None is
    cv_global bit for bit."""
    c, model, _, _ = case(name)
    h = handle_of(c)
    pred, var, st = h.cv_global()
    pn, vn, sn = h.cv_global_folds(None)
    fold = CC.location_folds(c["x"], 6, 41)
    for f in np.unique(fold):                                 # every remainder still holds every variable
        assert np.unique(c["var"][fold != f]).size == c["B1"].shape[0]
    pf, vf, sf = h.cv_global_folds(fold)
    h.close()
    assert np.array_equal(pred, pn) and np.array_equal(var, vn) and np.array_equal(st, sn)
    rp, rv = CR.cross_validate(model, c["x"], c["z"], c["var"])
    assert not st.any() and close(pred, rp) and close(var, rv)
    rp, rv = CR.cross_validate(model, c["x"], c["z"], c["var"], fold)
    assert not sf.any() and close(pf, rp) and close(vf, rv)


def test_simple_variant_cross_validation_adds_the_means_back():
    c, model, _, _ = case("simple_means")
    h = handle_of(c)
    pred, var, st = h.cv_global()
    fold = CC.location_folds(c["x"], 5, 43)
    pf, vf, sf = h.cv_global_folds(fold)
    h.close()
    rp, rv = CR.cross_validate(model, c["x"], c["z"], c["var"], None, "simple", c["means"])
    assert not st.any() and close(pred, rp) and close(var, rv)
    rp, rv = CR.cross_validate(model, c["x"], c["z"], c["var"], fold, "simple", c["means"])
    assert not sf.any() and close(pf, rp) and close(vf, rv)


def test_solver_on_a_grid_with_missing_rows():
    """solve through CoKrigingSolver: a 20 x 20 grid domain, a table whose columns are missing in different rows; the
    result carries the four columns and equals the handle-level call on the stacked non-missing rows."""
    import gss
    rng = np.random.default_rng(51)
    loc = CC.lattice((8, 8), 2.5, 52)
    cu = np.sin(0.3 * loc[:, 0]) + 0.1 * rng.normal(size=64)
    zn = np.cos(0.2 * loc[:, 1]) + 0.1 * rng.normal(size=64)
    cu[rng.permutation(64)[:40]] = np.nan                     # sparse primary
    zn[::7] = np.nan
    data = gss.georef(dict(cu=cu, zn=zn, other=np.zeros(64)), loc)
    B1, B0 = np.array([[0.9, 0.5], [0.5, 0.7]]), np.array([[0.1, 0.02], [0.02, 0.1]])
    # the model lists its variables in another order and holds one more: the solver takes the sub-matrices as listed
    B1full = np.array([[0.7, 0.0, 0.5], [0.0, 1.0, 0.0], [0.5, 0.0, 0.9]])
    B0full = np.array([[0.1, 0.0, 0.02], [0.0, 0.1, 0.0], [0.02, 0.0, 0.1]])
    lmc = gss.LMCModel(("zn", "other", "cu"), "spherical", 8.0, 1.0, B0full, B1full, 0.0)
    grid = gss.CartesianGrid((20, 20), (0.0, 0.0), (1.0, 1.0))
    solver = gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, variant="ordinary")))
    sol = gss.solve(gss.EstimationProblem(data, grid, ("cu", "zn")), solver)
    assert sol.names() == ["cu", "cu_variance", "zn", "zn_variance"]
    ic, iz = np.flatnonzero(~np.isnan(cu)), np.flatnonzero(~np.isnan(zn))
    x = np.concatenate([loc[ic], loc[iz]])
    z = np.concatenate([cu[ic], zn[iz]])
    var = np.repeat([0, 1], [ic.size, iz.size]).astype(np.int32)
    from gss.engine import HipEngine
    h = HipEngine.cokrig(gss.SphericalVariogram(range=8.0), B0, B1, 1, x, z, var)
    mu, vv, _ = h.predict_global(grid.centroids())
    h.close()
    assert np.array_equal(sol["cu"], mu[0]) and np.array_equal(sol["zn_variance"], vv[1])
    rmu, rvar = CR.predict(CR.Model(dict(kind="spherical", range=8.0), B0, B1), x, z, var, grid.centroids())
    assert close(sol["cu"], rmu[0]) and close(sol["zn"], rmu[1])
    assert close(sol["cu_variance"], rvar[0]) and close(sol["zn_variance"], rvar[1])


def test_example_runs_and_cokriging_does_not_lose_to_kriging():
    """examples/cokriging.py: the primary's mean kriging variance under cokriging <= under kriging alone (a theorem for
    a valid LMC: the same data plus more)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cokriging.py")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("mean kriging variance of cu")]
    assert len(line) == 1, r.stdout
    co, alone = (float(v) for v in line[0].split(":")[1].replace("cokriging", "").replace("kriging alone", "").split(","))
    print("  ", line[0])
    assert co <= alone
