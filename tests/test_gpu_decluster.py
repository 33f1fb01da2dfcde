"""Declustering on the device against the numpy restatement tests/decluster_ref.py: counts, occupied cells, best size,
hits and nzero exactly; weights and weighted means within the bounds derived in include/gss.h's terms:

  weights of one size   2 (noff + 2) 2^-53 relative: one rounded division per grid, a sum of noff positive terms and one
                        more division, doubled
  wmean[c]              2 (n + noff + 4) 2^-53 sum w_i |z_i| / n
"""
import os
import runpy
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decluster_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    import gss
    from gss.engine import HipEngine
    return HipEngine


def _dev(a):
    import torch
    return torch.as_tensor(a, device="cuda")


# ---- cell counts ----------------------------------------------------------------------------------------------------
def _check_counts(eng, x, origin, sides):
    ref_cnt, ref_occ = R.cell_counts(x, origin, sides)
    cnt, occ = eng.decluster_cell_counts(x, origin, sides)
    assert cnt.dtype == np.int32 and np.array_equal(cnt, ref_cnt) and occ == ref_occ
    dcnt, docc = eng.decluster_cell_counts(_dev(x), origin, sides)
    assert dcnt.is_cuda and np.array_equal(dcnt.cpu().numpy(), ref_cnt) and docc == ref_occ
    return ref_cnt, ref_occ


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 257, 4099])
def test_counts_on_an_edge_lattice(eng, n, dim):
    """coordinates on a 2^-4 lattice with duplicates, sides 2^-2: many samples sit exactly on cell edges"""
    x = R.lattice_points(n, dim, 100 * dim + n % 97)
    cnt, occ = _check_counts(eng, x, [0.0] * dim, [0.25] * dim)
    if n > 1:
        assert np.any(np.mod(x, 0.25) == 0.0) and cnt.max() > 1
    # an origin that is no lattice point and sides that are no power of two
    _check_counts(eng, x, [-0.1] * dim, [0.3, 0.7, 1.1][:dim])


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_two_samples_in_one_cell_and_in_two(eng, dim):
    a = np.full((1, dim), 0.25)
    one = np.concatenate([a, a + 0.5])
    cnt, occ = _check_counts(eng, one, [0.0] * dim, [1.0] * dim)
    assert cnt.tolist() == [2, 2] and occ == 1
    two = np.concatenate([a, a + 1.0])                       # the second exactly on the edge: the upper cell
    cnt, occ = _check_counts(eng, two, [0.0] * dim, [1.0] * dim)
    assert cnt.tolist() == [1, 1] and occ == 2


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_all_samples_in_one_cell_and_every_sample_in_its_own(eng, dim):
    rng = np.random.default_rng(dim)
    x = rng.uniform(0.0, 10.0, (513, dim))
    cnt, occ = _check_counts(eng, x, [0.0] * dim, [16.0] * dim)
    assert occ == 1 and np.all(cnt == 513)
    grid = np.stack(np.meshgrid(*[np.arange(9.0)] * dim, indexing="ij"), axis=-1).reshape(-1, dim)[:600]
    cnt, occ = _check_counts(eng, grid + 0.5, [0.0] * dim, [1.0] * dim)
    assert occ == grid.shape[0] and np.all(cnt == 1)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_the_largest_index_is_accepted(eng, dim):
    top = float((1 << 21) - 1)
    x = np.zeros((5, dim))
    x[1:3] = top                                             # index 2^21 - 1 along every axis, twice
    x[3, dim - 1] = top + 0.5
    x[4, 0] = 1.0
    cnt, occ = _check_counts(eng, x, [0.0] * dim, [1.0] * dim)
    assert R.cell_indices(x, [0.0] * dim, [1.0] * dim).max() == (1 << 21) - 1
    assert cnt.tolist() == ([1, 3, 3, 3, 1] if dim == 1 else [1, 2, 2, 1, 1])
    from gss import _lib
    x[2, 0] = top + 1.0
    with pytest.raises(_lib.GSSError, match="axis 0"):
        eng.decluster_cell_counts(_dev(x), [0.0] * dim, [1.0] * dim)       # a device array: checked on the device
    x[2, 0] = np.inf
    with pytest.raises(_lib.GSSError, match="not finite"):
        eng.decluster_cell_counts(_dev(x), [0.0] * dim, [1.0] * dim)


# ---- the sweep ------------------------------------------------------------------------------------------------------
_REF = {}


def _sweep_ref(dim, noff, crit):
    key = (dim, noff, crit)
    if key not in _REF:
        x, z = R.clustered(dim)
        _REF[key] = (x, z) + R.sweep(x, z, R.sweep_sides(dim), noff, crit)
    return _REF[key]


def _assert_weights(w, ref, noff):
    err = np.max(np.abs(w - ref) / ref)
    print("weights: max relative error %.3e (bound %.3e)" % (err, R.weight_bound(noff)))
    assert err <= R.weight_bound(noff)


@pytest.mark.parametrize("dim,noff,crit", R.SWEEP_CASES)
def test_sweep_against_the_reference(eng, dim, noff, crit):
    x, z, ws, wm, best = _sweep_ref(dim, noff, crit)
    sides = R.sweep_sides(dim)
    w, dwm, dbest = eng.decluster_cells(x, z, sides, noff, crit)
    for c in range(len(sides)):
        bound = R.wmean_bound(ws[c], z, noff)
        print("size %d: wmean error %.3e (bound %.3e)" % (c, abs(dwm[c] - wm[c]), bound))
        assert abs(dwm[c] - wm[c]) <= bound
    assert dbest == best
    _assert_weights(w, ws[best], noff)
    assert best != len(sides) - 1              # (so the weights of the best size were formed a second time, after the sweep)
    # per size: the weights of a call with that single size, which must also be the sweep's own bits for the best
    for c in range(len(sides)):
        wc, wmc, bc = eng.decluster_cells(x, z, sides[c:c + 1], noff, crit)
        _assert_weights(wc, ws[c], noff)
        assert bc == 0 and wmc[0] == dwm[c]
        if c == best:
            assert np.array_equal(wc, w)
    # device arrays: the same bits
    tw, twm, tbest = eng.decluster_cells(_dev(x), _dev(z), sides, noff, crit)
    assert np.array_equal(tw.cpu().numpy(), w) and np.array_equal(twm, dwm) and tbest == dbest


@pytest.mark.parametrize("dim", [2, 3])
def test_one_size_without_values(eng, dim):
    x, _ = R.clustered(dim)
    s = R.sweep_sides(dim)[3:4]
    w, wm, best = eng.decluster_cells(x, None, s, 5)
    assert wm is None and best == 0
    _assert_weights(w, R.size_weights(x, s[0], 5), 5)
    assert abs(w.sum() - x.shape[0]) < 1e-9
    from gss import _lib
    with pytest.raises(_lib.GSSError, match="z is NULL"):
        eng.decluster_cells(x, None, R.sweep_sides(dim), 5)


@pytest.mark.parametrize("dim,noff", [(2, 5), (3, 4)])
def test_batching_and_repetition_change_no_bit(eng, dim, noff, monkeypatch):
    x, z = R.clustered(dim)
    sides = R.sweep_sides(dim)
    base = eng.decluster_cells(x, z, sides, noff)
    again = eng.decluster_cells(x, z, sides, noff)
    for chunk in ("1", "3"):                                 # 3: batches that end inside a size
        monkeypatch.setenv("GSS_DECLUS_CHUNK_GRIDS", chunk)
        one = eng.decluster_cells(x, z, sides, noff)
        monkeypatch.delenv("GSS_DECLUS_CHUNK_GRIDS")
        for a, b in ((base, again), (base, one)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_sweep_with_more_samples_than_one_reduction_block(eng):
    """4 099 samples: three blocks of the weighted-mean reduction, the last one partly filled"""
    x, z = R.clustered(2, seed=11, n=4099)
    sides = R.sweep_sides(2)[1:4]
    ws, wm, best = R.sweep(x, z, sides, 3)
    w, dwm, dbest = eng.decluster_cells(x, z, sides, 3)
    assert dbest == best
    for c in range(3):
        assert abs(dwm[c] - wm[c]) <= R.wmean_bound(ws[c], z, 3)
    _assert_weights(w, ws[best], 3)


# ---- nearest --------------------------------------------------------------------------------------------------------
def _check_nearest(eng, x, lo, step, dims):
    n, M = x.shape[0], int(np.prod(dims))
    ref = R.nearest_hits(x, lo, step, dims)
    assert ref.sum() == M
    w, nzero = eng.decluster_nearest(x, lo, step, dims)
    hits = np.rint(w * M / n).astype(np.int64)
    assert np.array_equal(hits, ref) and nzero == int((ref == 0).sum())
    assert np.array_equal(w, n * ref.astype(np.float64) / M)
    tw, tnz = eng.decluster_nearest(_dev(x), lo, step, dims)
    assert np.array_equal(tw.cpu().numpy(), w) and tnz == nzero
    return w, nzero, ref


def test_nearest_on_a_3d_and_a_2d_lattice(eng, monkeypatch):
    rng = np.random.default_rng(21)
    x3 = rng.uniform(0.0, 1.0, (50, 3)) * [16.0, 16.0, 8.0]
    w3, _, _ = _check_nearest(eng, x3, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [16, 16, 8])
    x2 = rng.uniform(0.0, 1.0, (50, 2)) * [37.0, 11.0] + [5.0, -3.0]
    w2, _, _ = _check_nearest(eng, x2, [5.0, -3.0], [1.0, 1.0], [37, 11])
    _check_nearest(eng, x2, [5.0, -3.0], [0.3, 0.7], [37, 11])               # steps that round
    monkeypatch.setenv("GSS_DECLUS_CHUNK_QUERIES", "100")                     # 21 and 5 pieces, the last one short
    c3, _ = eng.decluster_nearest(x3, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [16, 16, 8])
    c2, _ = eng.decluster_nearest(x2, [5.0, -3.0], [1.0, 1.0], [37, 11])
    assert np.array_equal(c3, w3) and np.array_equal(c2, w2)


def test_nearest_gives_a_duplicated_sample_to_its_first_copy(eng):
    rng = np.random.default_rng(22)
    x = rng.uniform(0.0, 8.0, (20, 2))
    x[13] = x[4]
    w, nzero, ref = _check_nearest(eng, x, [0.0, 0.0], [0.5, 0.5], [16, 16])
    assert w[13] == 0.0 and w[4] > 0.0 and nzero >= 1
    x1 = np.array([[0.0], [1.0], [1.0], [5.0]])
    w, nzero, ref = _check_nearest(eng, x1, [0.0], [1.0], [6])               # 0.5 is equally far from 0 and 1: to 0
    assert ref.tolist() == [1, 2, 0, 3] and nzero == 1


# ---- front end ------------------------------------------------------------------------------------------------------
def test_weight_with_each_method_and_a_missing_row(eng):
    import gss
    x, z = R.clustered(2, seed=3, n=300)
    z = z.copy()
    z[17] = np.nan
    data = gss.georef({"z": z}, x)
    keep = ~np.isnan(z)
    xk, zk = x[keep], z[keep]

    wb = gss.weight(data, gss.BlockWeighting(10.0), "z")
    assert wb.dtype == np.float64 and wb.shape == (300,) and np.isnan(wb[17])
    ref = R.grid_weights(xk, xk.min(axis=0), [10.0, 10.0])
    assert np.max(np.abs(np.asarray(wb)[keep] - ref) / ref) <= R.weight_bound(1)
    assert abs(np.nansum(wb) - 299.0) < 1e-9
    wall = gss.weight(data, gss.BlockWeighting(10.0, 5.0))                   # no variable: every row
    assert not np.isnan(wall).any() and abs(wall.sum() - 300.0) < 1e-9

    method = gss.CellDeclustering(2.0, 35.0, ncell=12, noffsets=4)
    wc = gss.weight(data, method, "z")
    ws, wm, best = R.sweep(xk, zk, np.repeat(method.sizes[:, None], 2, axis=1), 4)
    assert wc.best == best and np.array_equal(wc.sizes, method.sizes) and wc.means.shape == (12,)
    assert np.max(np.abs(wc.means - wm)) <= max(R.wmean_bound(w, zk, 4) for w in ws)
    assert np.max(np.abs(np.asarray(wc)[keep] - ws[best]) / ws[best]) <= R.weight_bound(4) and np.isnan(wc[17])
    assert gss.wmean(z, wc) < 0.8 * np.nanmean(z)                             # the blob of high values is weighted down
    assert gss.wmean(z, wc) == pytest.approx(wc.means[wc.best], rel=1e-12)

    wp = gss.weight(data, gss.PolygonalWeighting((64, 64), allow_zero=True), "z")
    lo, hi = xk.min(axis=0), xk.max(axis=0)
    hits = R.nearest_hits(xk, lo, (hi - lo) / 64.0, [64, 64])
    assert np.array_equal(np.rint(np.asarray(wp)[keep] * 4096 / 299).astype(np.int64), hits) and np.isnan(wp[17])
    assert wp.nzero == int((hits == 0).sum()) and wp.nzero > 0
    with pytest.raises(ValueError, match="nzero = %d" % wp.nzero):
        gss.weight(data, gss.PolygonalWeighting((64, 64)), "z")
    grid = gss.CartesianGrid((50, 50), (0.0, 0.0), (2.0, 2.0))
    wg = gss.weight(data, gss.PolygonalWeighting(grid, allow_zero=True), "z")
    hg = R.nearest_hits(xk, [0.0, 0.0], [2.0, 2.0], [50, 50])
    assert np.array_equal(np.rint(np.asarray(wg)[keep] * 2500 / 299).astype(np.int64), hg)

    # the weights go into the normal-score fit as they are: the NaN row is dropped with its value
    ns = gss.NormalScore.fit(z, weights=wc)
    assert ns.values.size == 299 and ns.weights.size == 299
    y = ns.forward(zk)
    assert np.isfinite(y).all() and np.all(np.diff(y[np.argsort(zk, kind="stable")]) >= 0.0)
    assert np.max(np.abs(ns.inverse(y) - zk)) < 1e-9
    v, yk = ns.table()
    from statistics import NormalDist
    mid = len(v) // 2
    assert gss.wquantile(z, wc, NormalDist().cdf(yk[mid])) == pytest.approx(v[mid], rel=1e-9)
    ns.close()


def test_the_example_runs(capsys):
    ns = runpy.run_path(os.path.join(ROOT, "examples", "declustering.py"))
    out = ns["out"]
    assert out["declustered_mean"] < 0.8 * out["naive_mean"]
    assert abs(out["weights"].sum() - out["weights"].size) < 1e-6
    assert np.isfinite(out["scores"]).all() and abs(out["score_wmean"]) < 0.05
    assert "declustered mean" in capsys.readouterr().out
