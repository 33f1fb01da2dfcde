"""Batched cokriging means on the device (gss.h, gss_cokrig_predict_global_batch) against the numpy reference
tests/cokrig_ref.py over the case table tests/cokrig_cases.py, and the conditional co-simulation built on them.

Means column by column: 1e-9 (1 + |value|) in units where the largest diagonal of B0 + B1 is 1 (the bar of
tests/test_gpu_cokriging.py; 1e-6 for the Gaussian case).  Every case runs with 1, floor(COLS / nz) and
floor(COLS / nz) + 1 value vectors: one pass, one full pass, a full pass and a partial tail.  Three small cases on a 3-cell
sub-lattice cover the instantiations the table does not reach (Matern 1/2, Matern 5/2, a general kind)."""
import os
import re
import sys
from types import SimpleNamespace

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
ENTRY = "gss_cokrig_predict_global_batch"
# columns of one pass of the mean kernel: the compile-time constant of the unit
COLS = int(re.search(r"#define GSS_COKRIG_BATCH_COLS (\d+)",
                     open(os.path.join(ROOT, "geostatssolvers.jl_amd", "csrc", "cokrig_batch.hip")).read()).group(1))
# the seeds tests/cokrig_cases.py draws each case's values with: vector r of a batch is values(x, var, seed + r)
SEEDS = dict(iso2d=3, hetero3d=6, many1d=9, single_ok=12, single_sk=12, intrinsic=15, simple_means=18, on_samples=20,
             rotated=23, gaussian=26, matern12_1d=50, matern52_3d=51, cubic_3d=52)


def close(a, b, tol=CC.TOL):
    a, b = np.asarray(a), np.asarray(b)
    err = np.abs(a - b) / (1.0 + np.abs(b))
    print("   max error %.3g (bar %.0e)" % (float(err.max()), tol))
    return bool(np.all(err <= tol))


class GeneralModel(CR.Model):
    """A structure cokrig_ref has no formula for: rho from oracle.variogram.cov_pairwise at unit sill without nugget
    (isotropic; the zero key is the squared distance of cokrig_ref)."""

    def cov(self, xa, va, xb, vb, origin):
        from oracle.variogram import Variogram, cov_pairwise
        xa, xb = CR.frame_coords(xa), CR.frame_coords(xb)
        zero = CR.sqdist(xa, xb) == 0.0
        r = cov_pairwise(Variogram(self.s["kind"], sill=1.0, nugget=0.0, range=self.s["range"]), xa, xb)
        b1 = self.B1[np.ix_(va, vb)]
        return np.where(zero, self.B0[np.ix_(va, vb)] + b1, b1 * r)


def model_of(c):
    cls = CR.Model if c["structure"]["kind"] in ("exponential", "gaussian", "spherical", "matern") else GeneralModel
    return cls(c["structure"], c["B0"], c["B1"])


def sublattice(dim, structure, seed):
    """Cells 1, 4, 7, 10 per axis of a 12^dim grid (3-D: 64 locations; 1-D: 40 cells 1, 4, .. 118), permuted; variable 0
    at rows [:10], 1 at [5:30], 2 at [20:40]: heterotopic with collocated pairs.  The domain: 300 scattered points and the
    ten locations [30:40], where only variable 2 was measured."""
    if dim == 1:
        loc = np.arange(1, 120, 3, dtype=np.float64)[:, None] + 0.5
    else:
        ax = np.array([1.0, 4.0, 7.0, 10.0]) + 0.5
        loc = np.stack([a.ravel() for a in np.meshgrid(*([ax] * dim), indexing="ij")], axis=1)
    loc = loc[np.random.default_rng(33).permutation(len(loc))]
    x = np.concatenate([loc[:10], loc[5:30], loc[20:40]])
    var = np.repeat([0, 1, 2], [10, 25, 20])
    hi = 120.0 if dim == 1 else 12.0
    xdom = np.concatenate([np.random.default_rng(34).uniform(0.0, hi, (300, dim)), loc[30:40]])
    B1 = np.array([[0.8, 0.3, -0.2], [0.3, 0.7, 0.1], [-0.2, 0.1, 0.9]])
    return CC._case(structure, np.diag([0.1, 0.05, 0.02]), B1, x, var, xdom, seed)


EXTRA = {"matern12_1d": lambda: sublattice(1, dict(kind="matern", range=9.0, nu=0.5), SEEDS["matern12_1d"]),
         "matern52_3d": lambda: sublattice(3, dict(kind="matern", range=9.0, nu=2.5), SEEDS["matern52_3d"]),
         "cubic_3d": lambda: sublattice(3, dict(kind="cubic", range=9.0), SEEDS["cubic_3d"])}
ALL = {**CC.CASES, **CC.GAUSSIAN, **EXTRA}


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


def handle_of(c, **kw):
    from gss.engine import HipEngine
    return HipEngine.cokrig(structure_of(c["structure"]), c["B0"], c["B1"], VARIANT[c["variant"]], c["x"], c["z"],
                            c["var"], means=c["means"], **kw)


def batch_of(name, c, nbatch):
    # (simple_means is the case whose values stand about its unequal means)
    shift = np.asarray(c["means"], dtype=np.float64)[c["var"]] if name == "simple_means" else 0.0
    return np.stack([CC.values(c["x"], c["var"], SEEDS[name] + r) + shift for r in range(nbatch)])


_cache = {}


def case(name):
    """The case, its value vectors and the reference means of all of them (computed once, never modified)."""
    if name not in _cache:
        c = ALL[name]()
        per = COLS // c["B1"].shape[0]
        zb = batch_of(name, c, per + 1)
        assert np.array_equal(zb[0], c["z"])              # vector 0 is the case's own data
        model = model_of(c)
        ref = np.stack([CR.predict(model, c["x"], z, c["var"], c["xdom"], c["variant"], c["means"])[0] for z in zb])
        zb.setflags(write=False)
        ref.setflags(write=False)
        _cache[name] = (c, model, zb, ref, per)
    return _cache[name]


@pytest.mark.parametrize("name", list(ALL))
def test_batched_means_match_the_reference(name):
    c, model, zb, ref, per = case(name)
    tol = CC.TOL_GAUSSIAN if name == "gaussian" else CC.TOL
    if name in EXTRA:
        cond = CR.cond(model, c["x"], c["var"], c["variant"])
        print("   cond_2 = %.3g" % cond)
        assert cond <= CC.COND_CAP
    nz, m = c["B1"].shape[0], c["xdom"].shape[0]
    h = handle_of(c)
    try:
        for nb in (1, per, per + 1):
            got = h.predict_batch(c["xdom"], zb[:nb])
            assert got.shape == (nb, nz, m)
            assert close(got, ref[:nb], tol)
    finally:
        h.close()


@pytest.mark.parametrize("key", sorted(KC.KERNELS), ids=lambda key: "%d_%d" % key)
def test_every_compiled_batch_mean_kernel(key):
    """Every entry of tests/cokrig_kernel_cases.py (one per compiled cokrig_batch_mean_kernel<DIM, KIND>;
    tests/test_cokrig_census.py holds the table against the built library): COLS + 5 value vectors, more than the columns
    of a pass and no multiple of them, each against its own reference; the points on samples give every vector's value
    back."""
    c = KC.KERNELS[key]()
    nb = COLS + 5
    assert nb > COLS and nb % COLS != 0
    zb = KC.batch_of(c, nb)
    assert np.array_equal(zb[0], c["z"])
    model = KC.model_of(c)
    ref = np.stack([CR.predict(model, c["x"], z, c["var"], c["xdom"], c["variant"], c["means"])[0] for z in zb])
    nz, m = c["B1"].shape[0], c["xdom"].shape[0]
    h = handle_of(c)
    try:
        got = h.predict_batch(c["xdom"], zb)
    finally:
        h.close()
    assert got.shape == (nb, nz, m)
    assert close(got, ref)
    for p, j in enumerate(c["on"]):
        zj = zb[:, j]
        assert np.all(np.abs(got[:, c["var"][j], p] - zj) <= 1e-9 * (1.0 + np.abs(zj)))


def test_domain_points_on_samples_reproduce_every_value_vector():
    """The zero-key product: where variable 0 was measured its value comes back in every column; variable 1, not
    measured there, is estimated (the reference holds it, above)."""
    c, _, zb, ref, per = case("on_samples")
    h = handle_of(c)
    got = h.predict_batch(c["xdom"], zb)
    h.close()
    z0 = zb[:, 25:40]                                        # variable 0 at the domain's locations
    assert np.all(np.abs(got[:, 0] - z0) <= 1e-9 * (1.0 + np.abs(z0)))
    assert close(got[:, 1], ref[:, 1])


@pytest.mark.parametrize("name", ["hetero3d", "simple_means", "rotated"])
def test_one_vector_of_the_handles_own_values_is_predict_global(name):
    c, _, zb, ref, _ = case(name)
    h = handle_of(c)
    mu, _, _ = h.predict_global(c["xdom"])
    got = h.predict_batch(c["xdom"], c["z"])
    h.close()
    assert got.shape == (1,) + mu.shape
    assert close(got[0], mu) and close(got[0], ref[0])


def test_chunks_and_memory_spaces_give_the_same_bits():
    """A cap of 256 points makes 700 points three chunks; device arrays take no staging.  Every point's sum runs in the
    same order wherever it is computed."""
    import torch
    c, _, zb, ref, per = case("hetero3d")
    h = handle_of(c)
    one = h.predict_batch(c["xdom"], zb)
    xd, zd = torch.as_tensor(c["xdom"], device="cuda"), torch.as_tensor(np.array(zb), device="cuda")
    dev = h.predict_batch(xd, zd)
    os.environ[CHUNK_ENV] = "256"
    try:
        host3 = h.predict_batch(c["xdom"], zb)
        dev3 = h.predict_batch(xd, zd)
        torch.cuda.synchronize()
    finally:
        del os.environ[CHUNK_ENV]
        h.close()
    assert dev.is_cuda and dev3.is_cuda
    for other in (dev.cpu().numpy(), host3, dev3.cpu().numpy()):
        assert np.array_equal(other, one)
    assert close(one, ref)


def test_asynchronous_fit_is_joined():
    c, _, zb, ref, _ = case("iso2d")
    h = handle_of(c, async_fit=True)
    got = h.predict_batch(c["xdom"], zb[:3])
    h.close()
    assert close(got, ref[:3])


def test_refusals_and_empty_calls():
    import gss
    from gss import _lib
    from gss.engine import CoKrigHandle, KrigHandle
    c = CC.iso2d()
    single = KrigHandle(gss.ExponentialVariogram(range=25.0), 1, c["x"][:63], c["z"][:63])
    local = handle_of(c, factor=False)
    for h, n in ((single, 63), (local, 126)):
        with pytest.raises(_lib.GSSError, match=ENTRY) as e:
            CoKrigHandle.predict_batch(SimpleNamespace(_l=h._l, _h=h._h, n=n, nz=2), c["xdom"], c["z"][None, :n])
        assert e.value.code == _lib.ERR_INVALID
    single.close()
    local.close()
    h = handle_of(c)
    lib, xdom, z = h._l, c["xdom"], c["z"]
    out = np.full((1, 2, 4), 7.0)
    call = lambda m, nb, x=xdom, zz=z, o=out: lib.gss_cokrig_predict_global_batch(     # noqa: E731
        h._h, _lib.ptr(x), m, _lib.ptr(zz), nb, _lib.ptr(o), _lib.MEM_HOST, None)
    assert call(0, 1) == _lib.OK and call(4, 0) == _lib.OK and call(0, 0, None, None, None) == _lib.OK
    assert np.all(out == 7.0)                                 # nothing was written
    for bad in (lambda: call(-1, 1), lambda: call(4, -1), lambda: call(4, 1, None), lambda: call(4, 1, xdom, None),
                lambda: call(4, 1, xdom, z, None)):
        assert bad() == _lib.ERR_INVALID and ENTRY in _lib.last_error()
    assert h.predict_batch(xdom[:0], z).shape == (1, 2, 0)
    with pytest.raises(ValueError, match="one value per stacked sample"):
        h.predict_batch(xdom, z[:-1])
    h.close()


# ---- conditional co-simulation -----------------------------------------------------------------------------------------------
GRID = (24, 20)
RANGE = 8.0
B0 = np.array([[0.1, 0.03], [0.03, 0.08]])
B1 = np.array([[0.9, 0.5], [0.5, 0.7]])
MEANS = np.array([1.0, -2.0])
SEED, NREALS = 11, 4


def _problem_data():
    """tests/test_cokriging_batch_host.py's geometry: 34 cells of a 3-cell sub-lattice, cu at the first 12, zn at
    4 .. 33, data on the centroids."""
    import gss
    cells = np.array([(i, j) for i in range(1, GRID[0], 3) for j in range(1, GRID[1], 3)])
    cells = cells[np.random.default_rng(31).permutation(len(cells))][:34]
    loc = cells + 0.5
    x = np.concatenate([loc[:12], loc[4:]])
    var = np.repeat([0, 1], [12, 30]).astype(np.int32)
    z = CC.values(x, var, 41) + MEANS[var]
    cu, zn = np.full(34, np.nan), np.full(34, np.nan)
    cu[:12], zn[4:] = z[:12], z[12:]
    return gss.georef(dict(cu=cu, zn=zn), loc), x, z, var, cells[:, 0] + GRID[0] * cells[:, 1]


def _solver():
    import gss
    lmc = SimpleNamespace(names=("cu", "zn"), kind="exponential", range=RANGE, order=1.0, B0=B0, B1=B1)
    return gss.FFTGS(("cu", dict(mean=MEANS[0])), ("zn", dict(mean=MEANS[1])), (("cu", "zn"), dict(model=lmc)), rng=SEED)


def test_conditional_cosimulation_end_to_end():
    import gss
    from gss.engine import FFTGSHandle
    data, x, z, var, cells = _problem_data()
    grid = gss.CartesianGrid(*GRID)
    cent = grid.centroids()
    model = CR.Model(dict(kind="exponential", range=RANGE), B0, B1)
    assert CR.cond(model, x, var, "simple") <= CC.COND_CAP
    variables = {"cu": float, "zn": float}
    sol = gss.solve(gss.SimulationProblem(data, grid, variables, NREALS), _solver())
    got = np.stack([np.stack(sol["cu"]), np.stack(sol["zn"])], axis=1)              # (NREALS, 2, N)
    # the unconditional fields of the same seed (tests/test_gpu_fftgs_lmc.py holds them to the oracle) ...
    h = FFTGSHandle.lmc(gss.ExponentialVariogram(range=RANGE), B0, B1, MEANS, grid.dims, grid.spacing)
    zu = h.realize_lmc(SEED, 0, NREALS)
    h.close()
    # ... and the two cokriging terms from the reference
    dinds = [cells[:12], cells[4:]]
    xdat = cent[np.concatenate(dinds)]
    zbar = CR.predict(model, x, z, var, cent, "simple", MEANS)[0]
    scale = np.empty_like(got)
    for r in range(NREALS):
        zdat = np.concatenate([zu[r, 0, dinds[0]], zu[r, 1, dinds[1]]])
        zbar_u = CR.predict(model, xdat, zdat, var, cent, "simple", MEANS)[0]
        ref = zbar + (zu[r] - zbar_u)
        scale[r] = 2.0 + np.abs(zbar) + np.abs(zbar_u)
        err = np.abs(got[r] - ref) / scale[r]
        print("   realisation %d: max error %.3g (bar %.0e)" % (r, err.max(), CC.TOL))
        assert np.all(err <= CC.TOL)
        for a in (0, 1):
            zd = z[var == a]
            assert np.all(np.abs(got[r, a, dinds[a]] - zd) <= 1e-9 * (1.0 + np.abs(zd)))
    assert np.max(np.abs(got[0] - got[1])) > 0.1
    # a view of the grid that holds the data cells: the gathered full-grid result
    inds = np.sort(np.concatenate([cells, np.setdiff1d(np.arange(0, GRID[0] * GRID[1], 7), cells)]))
    vsol = gss.solve(gss.SimulationProblem(data, gss.view(grid, inds), variables, NREALS), _solver())
    vgot = np.stack([np.stack(vsol["cu"]), np.stack(vsol["zn"])], axis=1)
    verr = np.abs(vgot - got[:, :, inds]) / scale[:, :, inds]
    print("   view: max error %.3g" % verr.max())
    assert np.all(verr <= CC.TOL)
    # without data the joint call is what it was: the bits of the handle
    usol = gss.solve(gss.SimulationProblem(grid, variables, NREALS), _solver())
    assert np.array_equal(np.stack(usol["cu"]), zu[:, 0]) and np.array_equal(np.stack(usol["zn"]), zu[:, 1])


def test_conditional_example_runs():
    """examples/cosimulation_conditional.py: every realisation honours the drill-hole data of both variables."""
    import runpy
    out = runpy.run_path(os.path.join(ROOT, "examples", "cosimulation_conditional.py"))["out"]
    assert out["max_misfit"] <= 1e-8 and len(out["ensemble"]["cu"]) == out["nreals"]
