"""Declustering without a device: the numpy restatement (tests/decluster_ref.py) against answers worked by hand, the
refusals the library makes before it touches the device, the argument checks of the twin, the weighted statistics, and
the separation of the best cell size in every sweep case of tests/test_gpu_decluster.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decluster_ref as R

import gss
from gss import _lib


# ---- the reference against hand answers -----------------------------------------------------------------------------
def test_four_coincident_and_three_isolated_samples_on_a_unit_grid():
    x = np.array([[0.5, 0.5]] * 4 + [[1.5, 0.5], [0.5, 2.5], [3.5, 3.5]])
    cnt, nocc = R.cell_counts(x, [0.0, 0.0], [1.0, 1.0])
    assert cnt.tolist() == [4, 4, 4, 4, 1, 1, 1] and nocc == 4
    w = R.grid_weights(x, [0.0, 0.0], [1.0, 1.0])
    assert w.tolist() == [7 / 16] * 4 + [7 / 4] * 3
    assert w.sum() == 7.0
    ws, wm, best = R.sweep(x, np.arange(7.0), [[1.0, 1.0]], 1)
    # the sweep's origin is the data's minimum (0.5, 0.5): the same cells here
    assert ws[0].tolist() == w.tolist() and best == 0
    assert wm[0] == (7 / 16 * (0 + 1 + 2 + 3) + 7 / 4 * (4 + 5 + 6)) / 7


def test_a_sample_exactly_on_an_edge_belongs_to_the_upper_cell():
    x = np.array([[0.0], [0.999], [1.0], [1.5], [2.0]])
    idx = R.cell_indices(x, [0.0], [1.0])
    assert idx.ravel().tolist() == [0, 0, 1, 1, 2]
    cnt, nocc = R.cell_counts(x, [0.0], [1.0])
    assert cnt.tolist() == [2, 2, 2, 2, 1] and nocc == 3
    # an origin expression that rounds: side 0.3, offset 1 of 5 -> o = 0 - (0.3 * 1) / 5
    o = R.origin_of([0.0], [0.3], 1, 5)
    assert o[0] == -((0.3 * 1.0) / 5.0)
    assert R.cell_indices(np.array([[0.24]]), o, [0.3]).item() == int(np.floor((0.24 - o[0]) / 0.3))


def test_weights_of_a_size_are_the_mean_over_its_offsets():
    x = R.lattice_points(41, 2, 3)
    s = np.array([0.75, 0.5])
    w = R.size_weights(x, s, 3)
    lo = x.min(axis=0)
    parts = [R.grid_weights(x, lo - (s * k) / 3.0, s) for k in range(3)]
    assert np.array_equal(w, ((parts[0] + parts[1]) + parts[2]) / 3.0)
    assert abs(w.sum() - 41.0) < 1e-12


def test_nearest_reference_gives_ties_to_the_lower_index():
    x = np.array([[0.25, 0.5], [0.75, 0.5], [0.75, 0.5]])
    hits = R.nearest_hits(x, [0.0, 0.0], [0.5, 1.0], [2, 1])      # points (0.25, 0.5) and (0.75, 0.5)
    assert hits.tolist() == [1, 1, 0]
    hits = R.nearest_hits(np.array([[0.0], [1.0]]), [0.0], [1.0], [1])      # the point 0.5 is equally far from both
    assert hits.tolist() == [1, 0]


# ---- refusals that need no device -----------------------------------------------------------------------------------
def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _counts(x, origin, sides, n=None, dim=None):
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    o, s = np.asarray(origin, dtype=np.float64), np.asarray(sides, dtype=np.float64)
    cnt = np.zeros(max(x.shape[0], 1), dtype=np.int32)
    nocc = C.c_int64(-1)
    code = lib.gss_decluster_cell_counts(_p(x), x.shape[0] if n is None else n, x.shape[1] if dim is None else dim, _p(o),
                                         _p(s), _p(cnt), C.byref(nocc), _lib.MEM_HOST, None)
    return code, _lib.last_error()


def _cells(x, z, sides, noff, ncs=None, n=None, dim=None):
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    s = np.ascontiguousarray(sides, dtype=np.float64).reshape(-1, x.shape[1])
    ncs = s.shape[0] if ncs is None else ncs
    w, wm, best = np.zeros(x.shape[0]), np.zeros(max(ncs, 1)), C.c_int32(-1)
    code = lib.gss_decluster_cells(_p(x), _p(z), x.shape[0] if n is None else n, x.shape[1] if dim is None else dim,
                                   _p(s), ncs, noff, _lib.DECLUS_MIN, _p(w), _p(wm), C.byref(best), _lib.MEM_HOST, None)
    return code, _lib.last_error()


X2 = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0]])
Z3 = np.array([1.0, 2.0, 3.0])


def test_invalid_sizes_are_refused_without_a_device():
    code, msg = _counts(X2, [0.0, 0.0], [1.0, 1.0], n=0)
    assert code == _lib.ERR_INVALID and "n = 0" in msg
    code, msg = _cells(X2, Z3, [1.0, 1.0], 1, n=0)
    assert code == _lib.ERR_INVALID and "n = 0" in msg
    x4 = np.zeros((3, 4))
    code, msg = _counts(x4, [0.0] * 4, [1.0] * 4)
    assert code == _lib.ERR_INVALID and "dim = 4" in msg
    code, msg = _cells(X2, Z3, [1.0, 1.0], 1, dim=4)
    assert code == _lib.ERR_INVALID and "dim = 4" in msg


@pytest.mark.parametrize("side", [0.0, -1.0, float("nan"), float("inf")])
def test_a_side_that_is_not_finite_and_positive_is_refused(side):
    code, msg = _counts(X2, [0.0, 0.0], [1.0, side])
    assert code == _lib.ERR_INVALID and "side" in msg and "axis 1" in msg
    code, msg = _cells(X2, Z3, [[1.0, 1.0], [side, 1.0]], 2)
    assert code == _lib.ERR_INVALID and "side" in msg and "axis 0" in msg


def test_offsets_and_sizes_outside_their_limits_are_refused():
    for noff in (0, 65):
        code, msg = _cells(X2, Z3, [1.0, 1.0], noff)
        assert code == _lib.ERR_INVALID and "noff = %d" % noff in msg
    code, msg = _cells(X2, Z3, np.ones((257, 2)), 1)
    assert code == _lib.ERR_INVALID and "ncs = 257" in msg
    code, msg = _cells(X2, Z3, np.ones((1, 2)), 1, ncs=0)
    assert code == _lib.ERR_INVALID and "ncs = 0" in msg
    code, msg = _cells(X2, None, [[1.0, 1.0], [2.0, 2.0]], 1)
    assert code == _lib.ERR_INVALID and "z is NULL" in msg and "ncs = 2" in msg


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_coordinate_or_value_is_refused(bad):
    x = X2.copy()
    x[1, 1] = bad
    code, msg = _counts(x, [0.0, 0.0], [1.0, 1.0])
    assert code == _lib.ERR_INVALID and "coordinate" in msg and "finite" in msg
    code, msg = _cells(x, Z3, [1.0, 1.0], 1)
    assert code == _lib.ERR_INVALID and "coordinate" in msg
    z = Z3.copy()
    z[2] = bad
    code, msg = _cells(X2, z, [1.0, 1.0], 1)
    assert code == _lib.ERR_INVALID and "z" in msg and "finite" in msg
    lib = _lib.load()
    w, nz = np.zeros(3), C.c_int64()
    lo, st, dims = np.zeros(2), np.ones(2), np.array([2, 2], dtype=np.int64)
    code = lib.gss_decluster_nearest(_p(x), 3, 2, _p(lo), _p(st), _p(dims), _p(w), C.byref(nz), _lib.MEM_HOST, None)
    assert code == _lib.ERR_INVALID and "coordinate" in _lib.last_error()


def test_an_index_of_two_to_the_21_is_refused_and_names_the_axis():
    x = np.array([[0.0, 0.0], [1.0, float(1 << 21)]])
    code, msg = _counts(x, [0.0, 0.0], [1.0, 1.0])
    assert code == _lib.ERR_INVALID and "axis 1" in msg and "2^21" in msg
    code, msg = _cells(x, np.array([1.0, 2.0]), [1.0, 1.0], 1)
    assert code == _lib.ERR_INVALID and "axis 1" in msg and "2^21" in msg
    code, msg = _counts(X2, [0.5, 0.0], [1.0, 1.0])               # a sample below the origin: a negative index
    assert code == _lib.ERR_INVALID and "axis 0" in msg


def test_the_nearest_call_checks_its_lattice_without_a_device():
    lib = _lib.load()
    w, nz = np.zeros(3), C.c_int64()
    lo = np.zeros(2)
    for st, dims, word in (([1.0, 0.0], [2, 2], "step"), ([1.0, float("nan")], [2, 2], "step"),
                           ([1.0, 1.0], [2, 0], "dims"), ([1.0, 1.0], [1 << 30, 1 << 30], "2^53")):
        st, dims = np.asarray(st), np.asarray(dims, dtype=np.int64)
        code = lib.gss_decluster_nearest(_p(X2), 3, 2, _p(lo), _p(st), _p(dims), _p(w), C.byref(nz), _lib.MEM_HOST, None)
        assert code == _lib.ERR_INVALID and word in _lib.last_error(), (word, _lib.last_error())


# ---- the twin's own checks ------------------------------------------------------------------------------------------
class _NoEngine:
    name = "stand-in"


def test_twin_argument_checks():
    with pytest.raises(ValueError):
        gss.BlockWeighting()
    assert gss.BlockWeighting(2.0).sides == (2.0,) and gss.BlockWeighting((1.0, 2.0)).sides == (1.0, 2.0)
    for bad in (dict(cmin=0.0, cmax=1.0), dict(cmin=2.0, cmax=1.0), dict(cmin=1.0, cmax=2.0, ncell=0),
                dict(cmin=1.0, cmax=2.0, ncell=257), dict(cmin=1.0, cmax=2.0, noffsets=0),
                dict(cmin=1.0, cmax=2.0, noffsets=65), dict(cmin=1.0, cmax=2.0, criterion="median")):
        with pytest.raises(ValueError):
            gss.CellDeclustering(**bad)
    cd = gss.CellDeclustering(1.0, 24.0)
    assert cd.sizes.size == 24 and cd.sizes[0] == 1.0 and cd.sizes[-1] == 24.0 and cd.noffsets == 8
    with pytest.raises(ValueError):
        gss.PolygonalWeighting((4, 0))
    data = gss.georef({"z": [1.0, 2.0, 3.0]}, X2)
    with pytest.raises(TypeError):
        gss.weight(data, "block")
    with pytest.raises(NotImplementedError):
        gss.weight(data, gss.BlockWeighting(1.0), engine=_NoEngine)
    with pytest.raises(NotImplementedError):
        gss.weight(data, gss.PolygonalWeighting((4, 4)), engine=_NoEngine)
    with pytest.raises(ValueError, match="sides"):
        gss.weight(data, gss.BlockWeighting(1.0, 2.0, 3.0), engine=_NoEngine)
    with pytest.raises(ValueError, match="var"):
        gss.weight(data, gss.CellDeclustering(1.0, 2.0), engine=_NoEngine)
    with pytest.raises(ValueError, match="lattice"):
        gss.weight(data, gss.PolygonalWeighting((4, 4, 4)), engine=_NoEngine)
    with pytest.raises(AssertionError):
        gss.weight(gss.georef({"z": [np.nan] * 3}, X2), gss.BlockWeighting(1.0), "z", engine=_NoEngine)


class _RecordingEngine:
    """what the front end hands to the engine, with a stand-in answer"""
    name = "recording"
    calls = []

    @classmethod
    def decluster_cells(cls, x, z, sides, noffsets, criterion="min"):
        cls.calls.append((x, z, np.asarray(sides), noffsets, criterion))
        return np.ones(x.shape[0]), (None if z is None else np.arange(len(sides), dtype=float)), 0

    @classmethod
    def decluster_nearest(cls, x, lo, step, dims):
        cls.calls.append((x, np.asarray(lo), np.asarray(step), tuple(dims)))
        w = np.ones(x.shape[0])
        w[0] = 0.0
        return w, 1


def test_front_end_drops_missing_rows_and_builds_the_sizes():
    E = _RecordingEngine
    x = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0], [4.0, 4.0]])
    data = gss.georef({"z": [1.0, np.nan, 3.0, 4.0]}, x)
    E.calls.clear()
    w = gss.weight(data, gss.CellDeclustering(1.0, 3.0, ncell=3, noffsets=4, criterion="max", anisotropy=(1.0, 0.5)), "z",
                   engine=E)
    xs, zs, sides, noff, crit = E.calls[0]
    assert np.array_equal(xs, x[[0, 2, 3]]) and np.array_equal(zs, [1.0, 3.0, 4.0]) and noff == 4 and crit == "max"
    assert np.array_equal(sides, [[1.0, 0.5], [2.0, 1.0], [3.0, 1.5]])
    assert np.isnan(w[1]) and np.array_equal(np.asarray(w)[[0, 2, 3]], [1.0, 1.0, 1.0])
    assert np.array_equal(w.sizes, [1.0, 2.0, 3.0]) and np.array_equal(w.means, [0.0, 1.0, 2.0]) and w.best == 0
    E.calls.clear()
    gss.weight(data, gss.BlockWeighting(2.0), engine=E)                       # no var: every row, one scalar side
    xs, zs, sides, noff, _ = E.calls[0]
    assert xs.shape == (4, 2) and zs is None and np.array_equal(sides, [[2.0, 2.0]]) and noff == 1
    E.calls.clear()
    with pytest.raises(ValueError, match="nzero = 1.*finer lattice"):
        gss.weight(data, gss.PolygonalWeighting((8, 4)), engine=E)
    _, lo, step, dims = E.calls[0]
    assert np.array_equal(lo, [0.0, 0.0]) and np.array_equal(step, [0.5, 1.0]) and dims == (8, 4)
    w = gss.weight(data, gss.PolygonalWeighting(gss.CartesianGrid((8, 4), (-1.0, 0.0), (1.0, 2.0)), allow_zero=True),
                   engine=E)
    assert w.nzero == 1 and w[0] == 0.0
    _, lo, step, dims = E.calls[-1]
    assert np.array_equal(lo, [-1.0, 0.0]) and np.array_equal(step, [1.0, 2.0]) and dims == (8, 4)


def test_normal_score_fit_drops_the_rows_weight_marks():
    z = np.array([3.0, np.nan, 1.0, 2.0])
    w = np.array([0.5, np.nan, 1.5, 1.0])                # NaN exactly where the value is missing, as gss.weight leaves it
    ns = gss.NormalScore.fit(z, weights=w)
    assert np.array_equal(ns.values, [3.0, 1.0, 2.0]) and np.array_equal(ns.weights, [0.5, 1.5, 1.0])
    with pytest.raises(ValueError):
        gss.NormalScore.fit(z, weights=np.array([0.5, 1.0, np.nan, 1.0]))      # a NaN weight on a present value


# ---- weighted statistics --------------------------------------------------------------------------------------------
def test_weighted_statistics_against_direct_formulas():
    rng = np.random.default_rng(5)
    v, w = rng.lognormal(size=200), rng.uniform(0.2, 3.0, 200)
    m = (w * v).sum() / w.sum()
    assert gss.wmean(v, w) == pytest.approx(m, rel=1e-15)
    assert gss.wvar(v, w) == pytest.approx((w * (v - m) ** 2).sum() / w.sum(), rel=1e-14)
    assert gss.wmean(v, np.ones(200)) == pytest.approx(v.mean(), rel=1e-15)
    assert gss.wvar(v, np.ones(200)) == pytest.approx(v.var(), rel=1e-13)
    v2, w2 = np.append(v, np.nan), np.append(w, 1.0)                          # a NaN row is dropped
    assert gss.wmean(v2, w2) == gss.wmean(v, w)
    with pytest.raises(ValueError):
        gss.wmean(v, w[:-1])
    with pytest.raises(ValueError):
        gss.wmean(v, -w)


def test_wquantile_follows_the_cumulative_weight_convention_of_the_normal_score_fit():
    v = np.array([4.0, 1.0, 2.0, 2.0, 7.0])
    w = np.array([1.0, 2.0, 0.5, 1.5, 3.0])
    # classes 1 (2), 2 (2), 4 (1), 7 (3); total 8; p = (below + W / 2) / 8
    pk = np.array([1.0, 3.0, 4.5, 6.5]) / 8.0
    assert np.array_equal(gss.wquantile(v, w, pk), [1.0, 2.0, 4.0, 7.0])
    assert gss.wquantile(v, w, 0.0) == 1.0 and gss.wquantile(v, w, 1.0) == 7.0
    assert gss.wquantile(v, w, 0.5 * (pk[1] + pk[2])) == pytest.approx(3.0, rel=1e-15)
    # the same classes and probabilities as the fit: Phi(score of class k) = p_k
    from statistics import NormalDist
    import nscore_ref
    vv, yy = nscore_ref.fit(v, w)[:2]
    assert np.array_equal(vv, [1.0, 2.0, 4.0, 7.0])
    assert np.allclose([NormalDist().cdf(y) for y in yy], pk, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        gss.wquantile(v, w, 1.5)


# ---- the sweep cases of the GPU file: the best size is no coin toss -------------------------------------------------
@pytest.mark.parametrize("dim,noff,crit", R.SWEEP_CASES)
def test_best_size_of_every_sweep_case_is_separated(dim, noff, crit):
    x, z = R.clustered(dim)
    assert x.shape == (1000, dim)
    ws, wm, best = R.sweep(x, z, R.sweep_sides(dim), noff, crit)
    bound = max(R.wmean_bound(w, z, noff) for w in ws)
    others = np.delete(wm, best)
    gap = np.min(np.abs(others - wm[best]))
    assert gap >= 100.0 * bound, (gap, bound)
    assert all(abs(w.sum() - 1000.0) < 1e-9 for w in ws)
    # declustering does something here: the blob of high values is weighted down
    assert wm.min() < 0.8 * z.mean()
