"""Batched cokriging means and conditional co-simulation, what needs no device: the declaration, export and binding of
gss_cokrig_predict_global_batch, the compiled instantiations of its mean kernel, and the front end of the joint
conditional FFTGS (fft.jl:105-135, 176-192 for a group of variables) on a stand-in engine that answers from the numpy
references tests/cokrig_ref.py and tests/fftgs_lmc_ref.py."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cokrig_cases as CC
import cokrig_ref as CR
import fftgs_lmc_ref as FR

import gss
from gss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENTRY = "gss_cokrig_predict_global_batch"


def test_header_declares_library_exports_and_binding_covers_the_call():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gss.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+" + ENTRY + r"\s*\(", src)
    assert hasattr(_lib.load(), ENTRY)
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["gss_krig_predict_global_batch"]
    from gss.engine import CoKrigHandle, HipEngine
    assert callable(CoKrigHandle.predict_batch) and callable(HipEngine.cokrig)


def test_refusals_that_need_no_device():
    lib = _lib.load()
    assert lib.gss_cokrig_predict_global_batch(None, None, 1, None, 1, None, 0, None) == _lib.ERR_INVALID
    assert ENTRY in _lib.last_error()


def test_one_mean_kernel_per_dimension_and_kind():
    """DIM 1 .. 3 x (Gaussian, exponential, spherical, Matern 1/2, 3/2, 5/2, general): the dispatch of launch_cokrig_rhs."""
    import kernel_census
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf / c++filt not available")
    compiled = [tuple(int(a) for a in args) for fam, args in kernel_census.census(_lib.LIB_PATH)
                if fam == "cokrig_batch_mean_kernel"]
    assert len(compiled) == len(set(compiled)) == 21
    assert set(compiled) == {(d, k) for d in (1, 2, 3) for k in (0, 1, 2, 30, 31, 32, -1)}


# ---- the front end on a stand-in engine ------------------------------------------------------------------------------------
GRID = (24, 20)
RANGE = 8.0
B0 = np.array([[0.1, 0.03], [0.03, 0.08]])
B1 = np.array([[0.9, 0.5], [0.5, 0.7]])
MEANS = np.array([1.0, -2.0])
SEED = 11
MODEL = CR.Model(dict(kind="exponential", range=RANGE), B0, B1)


def geometry(jitter=0.0):
    """34 locations on a 3-cell sub-lattice of the 24 x 20 grid: cu at the first 12, zn at 4 .. 33 (8 collocated).
    -> (locations[34, 2], cells[34]) with the cells numbered as the grid numbers them (x fastest)."""
    cells = np.array([(i, j) for i in range(1, GRID[0], 3) for j in range(1, GRID[1], 3)])
    cells = cells[np.random.default_rng(31).permutation(len(cells))][:34]
    loc = cells + 0.5
    if jitter:
        loc = loc + np.random.default_rng(32).uniform(-jitter, jitter, loc.shape)
    return loc, cells[:, 0] + GRID[0] * cells[:, 1]


def table(loc):
    """One table, a column per variable, NaN where a variable was not measured.  -> (data, x, z, var) with the stacked
    arrays in the order the front end forms them (variable by variable, rows in table order)."""
    rows = [np.arange(12), np.arange(4, 34)]
    x = np.concatenate([loc[r] for r in rows])
    var = np.repeat([0, 1], [12, 30]).astype(np.int32)
    z = CC.values(x, var, 41) + MEANS[var]
    cu, zn = np.full(34, np.nan), np.full(34, np.nan)
    cu[rows[0]], zn[rows[1]] = z[:12], z[12:]
    return gss.georef(dict(cu=cu, zn=zn), loc), x, z, var


class _LMC:
    def __init__(self, structure, B0, B1, means, dims, spacing=None, spectrum=True):
        self.a = (structure.kind, tuple(dims), B0, B1, means)
        self.kw = dict(spacing=spacing, range=structure.range)

    def realize_lmc(self, seed, first_real, nreals, inds=None):
        z = FR.realize(*self.a, seed, first_real, nreals, **self.kw)
        return z if inds is None else z[:, :, inds]

    def close(self):
        pass


class _CoKrig:
    def __init__(self, structure, B0, B1, variant, x, z, var, means=None):
        assert variant == 0                                  # the front end conditions by simple cokriging
        self.model = CR.Model(dict(kind=structure.kind, range=structure.range), B0, B1)
        self.x, self.z, self.var, self.means = np.array(x), np.array(z), np.array(var), np.array(means)

    def predict_batch(self, xdom, zbatch):
        return np.stack([CR.predict(self.model, self.x, zb, self.var, xdom, "simple", self.means)[0] for zb in zbatch])

    def close(self):
        pass


class _Engine:
    name = "cokriging stand-in"
    FFTGS_LMC = _LMC
    handles = []

    @staticmethod
    def cokrig(*args, **kw):
        _Engine.handles.append(_CoKrig(*args, **kw))
        return _Engine.handles[-1]


def _solve(data, nreals=3, variables=("cu", "zn"), domain=None, **cu_params):
    lmc = SimpleNamespace(names=("cu", "zn"), kind="exponential", range=RANGE, order=1.0, B0=B0, B1=B1)
    solver = gss.FFTGS(("cu", dict(mean=MEANS[0], **cu_params)), ("zn", dict(mean=MEANS[1])),
                       (("cu", "zn"), dict(model=lmc)), rng=SEED, engine=_Engine)
    grid = gss.CartesianGrid(*GRID) if domain is None else domain
    _Engine.handles = []
    sol = gss.solve(gss.SimulationProblem(data, grid, {v: float for v in variables}, nreals), solver)
    return {v: np.stack(sol[v]) for v in variables}, grid


def _unconditional(nreals, grid):
    return FR.realize("exponential", GRID, B0, B1, MEANS, SEED, 0, nreals, spacing=grid.spacing, range=RANGE)


def test_conditioning_of_the_geometry():
    """The 1e-9 bars below rest on numpy's solves: cond_2 far under the cap of the cokriging cases."""
    assert abs(np.max(np.diag(B0) + np.diag(B1)) - 1.0) < 1e-15
    for jitter in (0.0, 0.3):
        loc, _ = geometry(jitter)
        _, x, _, var = table(loc)
        for variant in ("simple", "ordinary"):
            c = CR.cond(MODEL, x, var, variant)
            print("jitter %.1f %s cond_2 = %.3g" % (jitter, variant, c))
            assert c <= CC.COND_CAP


def test_solve_is_the_composition_and_honours_data_on_centroids():
    loc, cells = geometry()
    data, x, z, var = table(loc)
    got, grid = _solve(data)
    cent = grid.centroids()
    assert np.array_equal(cent[cells], loc)
    # NaN rows are dropped: 12 + 30 stacked samples in the first system, the data cells of each variable in the second
    first, second = _Engine.handles
    assert np.array_equal(first.x, x) and np.array_equal(first.z, z) and np.array_equal(first.var, var)
    assert np.array_equal(first.means, MEANS)
    dinds = [cells[:12], cells[4:]]
    assert np.array_equal(second.x, cent[np.concatenate(dinds)]) and np.array_equal(second.var, var)
    # z_bar + (z_u - z_bar_u), composed by hand from the two references
    zu = _unconditional(3, grid)
    zbar = CR.predict(MODEL, x, z, var, cent, "simple", MEANS)[0]
    for r in range(3):
        zdat = np.concatenate([zu[r, 0, dinds[0]], zu[r, 1, dinds[1]]])
        zbar_u = CR.predict(MODEL, cent[np.concatenate(dinds)], zdat, var, cent, "simple", MEANS)[0]
        ref = zbar + (zu[r] - zbar_u)
        for a, v in enumerate(("cu", "zn")):
            # the same numpy calls on the same inputs; only the order of the final sum may differ
            assert np.max(np.abs(got[v][r] - ref[a])) <= 1e-12
            zd = z[var == a]
            err = np.abs(got[v][r, dinds[a]] - zd)
            print("realisation", r, v, "max |z - data| =", err.max())
            assert np.all(err <= 1e-9 * (1.0 + np.abs(zd)))
    # away from the data the realisations differ from each other
    assert np.max(np.abs(got["cu"][0] - got["cu"][1])) > 0.1


def test_jittered_data_give_the_kriged_field_at_their_cells():
    loc, cells = geometry(0.3)
    data, x, z, var = table(loc)
    got, grid = _solve(data)
    zbar = CR.predict(MODEL, x, z, var, grid.centroids(), "simple", MEANS)[0]
    for a, (v, d) in enumerate((("cu", cells[:12]), ("zn", cells[4:]))):
        for r in range(3):
            assert np.all(np.abs(got[v][r, d] - zbar[a, d]) <= 1e-9 * (1.0 + np.abs(zbar[a, d])))
        assert np.max(np.abs(zbar[a, d] - z[var == a])) > 1e-3         # ... which is not the data


def test_a_variable_without_data_is_accepted():
    loc, cells = geometry()
    _, x, z, var = table(loc)
    data = gss.georef(dict(cu=z[:12]), loc[:12])
    got, grid = _solve(data)
    first, second = _Engine.handles
    assert first.x.shape == (12, 2) and not first.var.any() and second.x.shape == (12, 2)
    for r in range(3):
        assert np.all(np.abs(got["cu"][r, cells[:12]] - z[:12]) <= 1e-9 * (1.0 + np.abs(z[:12])))
    # zn is drawn towards the cu data through the cross covariance: no longer the unconditional field
    assert np.max(np.abs(got["zn"] - _unconditional(3, grid)[:, 1])) > 1e-3


def test_a_view_of_the_grid():
    loc, cells = geometry()
    data, x, z, var = table(loc)
    full, grid = _solve(data)
    inds = np.sort(np.concatenate([cells, np.setdiff1d(np.arange(0, GRID[0] * GRID[1], 7), cells)]))

    class _Search(_Engine):          # a view is looked up by the engine's search
        @staticmethod
        def knn_search(c, pts, k):
            d2 = CR.sqdist(np.asarray(pts), np.asarray(c))
            return np.argmin(d2, axis=1)[:, None], None

    lmc = SimpleNamespace(names=("cu", "zn"), kind="exponential", range=RANGE, order=1.0, B0=B0, B1=B1)
    solver = gss.FFTGS(("cu", dict(mean=MEANS[0])), ("zn", dict(mean=MEANS[1])), (("cu", "zn"), dict(model=lmc)),
                       rng=SEED, engine=_Search)
    sol = gss.solve(gss.SimulationProblem(data, gss.view(grid, inds), {"cu": float, "zn": float}, 2), solver)
    where = np.searchsorted(inds, cells)
    for a, (v, rows) in enumerate((("cu", slice(0, 12)), ("zn", slice(4, 34)))):
        zd = z[var == a]
        for r in range(2):
            assert np.all(np.abs(sol[v][r][where[rows]] - zd) <= 1e-9 * (1.0 + np.abs(zd)))


def test_all_missing_and_local_neighbourhoods_are_refused():
    loc, _ = geometry()
    with pytest.raises(AssertionError, match="missing"):
        _solve(gss.georef(dict(cu=np.full(34, np.nan), zn=np.full(34, np.nan)), loc))
    data = table(loc)[0]
    with pytest.raises(NotImplementedError, match="maxneighbors"):
        _solve(data, maxneighbors=8)
    with pytest.raises(NotImplementedError, match="neighborhood"):
        _solve(data, neighborhood=gss.MetricBall(5.0))
