"""Every compiled instantiation of the neighbour-search kernels and of the IDW / LWR kernels (tests/search_cases.py) on
one problem each whose answer does not depend on rounding (tests/search_matrix.py): neighbour indices and counts,
-1 padding included, for equality against the int64 ranking by (key, index) of grid coordinates (haversine: the
50-digit ranking, gaps asserted); IDW / LWR means, distance / norm column and status against mpmath at 50 digits on
those lists, within the bars of search_cases.BARS (16 x the measured error of the FP64 oracle, floor 8 units of
2^-53 x data scale).

What it found (search matrix): knn_pruned_kernel<2, true, 2> with 128 neighbours and four
conditioning cells read back uninitialised memory as the lists of those cells -- beyond 64 neighbours (and with the mask
applied after the search) the SGS weights kernels write the lists the handle returns and skipped data cells.  They now
write the empty list; the case stays as the regression test.  Every other case passed on its first run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_cases as SC
import search_matrix as SM

pytestmark = pytest.mark.gpu

ENTRIES = [(key, case) for key, case in SC.CASES.items() if isinstance(case, SC.Case)]


def _id(key):
    return "%s-%s" % (key[0], "_".join(str(a) for a in key[1])) if key[1] else key[0]


def _ball(p):
    return dict(radius=p.mt.radius, radii=p.mt.radii)


def _device_lists(p, case, monkeypatch):
    """idx, count of the checked queries, once per forced build where the case asks for both."""
    from gss.engine import HipEngine, SGSHandle
    out = []
    for build in (("host", "device") if case.build == "both" else (case.build,)):
        if build:
            monkeypatch.setenv("GSS_KNN_BUILD", build)
        if case.route == "brute":
            monkeypatch.setenv("GSS_KNN_BRUTE", "1")
        if case.op == "masked":
            import gss
            vg = gss.ExponentialVariogram(range=4.0 * p.sp * SM.GRID, nugget=0.25)
            h = SGSHandle(vg, p.x, p.path, p.dlocs, np.zeros(p.dlocs.size), 0.0, case.k, 1, mask_after_search=False,
                          distance=p.distance, rotation=p.mt.rotation, **_ball(p))
            idx, cnt, _, _ = h.weights()
            h.close()
            # the handle's count is the search's, except that it reports 0 conditioning neighbours where the kriging
            # system does not factor: only a node whose listed neighbours include coincident cells may do that
            listed = (idx >= 0).sum(axis=1).astype(np.int32)
            coincident = np.array([np.unique(p.X[row[:c]], axis=0).shape[0] < c for row, c in zip(idx, listed)])
            assert np.all((cnt == listed) | ((cnt == 0) & coincident)), np.flatnonzero(cnt != listed)[:8]
            cnt = np.where(coincident, listed, cnt).astype(np.int32)
        else:
            idx, cnt = HipEngine.knn_search(p.x, p.c, case.k, distance=p.distance, rotation=p.mt.rotation, **_ball(p))
        monkeypatch.delenv("GSS_KNN_BUILD", raising=False)
        monkeypatch.delenv("GSS_KNN_BRUTE", raising=False)
        out.append((idx[p.check], cnt[p.check]))
    return out


def _device_estimate(p, case):
    from gss.engine import HipEngine
    kw = dict(distance=p.distance, **_ball(p))
    if case.op == "idw":
        return HipEngine.idw(p.x, p.z, p.c, case.k, case.minn, case.exponent, **kw)
    return HipEngine.lwr(p.x, p.z, p.c, case.k, case.minn, case.weight, **kw)


@pytest.mark.parametrize("key,case", ENTRIES, ids=[_id(k) for k, _ in ENTRIES])
def test_instantiation_gives_the_exact_lists_and_the_50_digit_estimates(key, case, monkeypatch):
    if case.route == "few":
        assert case.m <= 4096 and case.n >= 32768 and case.k <= 64
    elif case.route == "index" and case.op == "search":
        assert case.m > 4096 or case.n < 32768 or case.k > 64
    p = SM.problem_of(case)
    ridx, rcnt, rkeys = SM.reference_lists(p)
    SM.assert_expectations(case, p, ridx, rcnt, rkeys)
    if case.op in ("search", "masked"):
        for idx, cnt in _device_lists(p, case, monkeypatch):
            bad = np.flatnonzero((idx != ridx).any(axis=1) | (cnt != rcnt))
            print("%s: %d queries checked of %d, n = %d, k = %d, counts %d..%d, %d lists differ"
                  % (_id(key), len(p.check), p.c.shape[0], case.n, case.k, rcnt.min(), rcnt.max(), bad.size))
            assert bad.size == 0, (p.check[bad[:5]], idx[bad[:1]], ridx[bad[:1]], cnt[bad[:5]], rcnt[bad[:5]])
        return
    # estimators: the list the search must have produced enters the 50-digit answer; the device runs its own search
    if case.op == "lwr":
        assert SM.design_condition(case, p, ridx, rcnt) < 1e6
    rmean, raux, rst = SM.mp_estimate(case, p, ridx, rcnt, rkeys if case.metric == "haversine" else None)
    if case.k < case.n:          # (k = n runs no search) a wrong list is reported as such, not as a wrong weight
        from gss.engine import HipEngine
        idx, cnt = HipEngine.knn_search(p.x, p.c, case.k, distance=p.distance, **_ball(p))
        assert np.array_equal(idx[p.check], ridx) and np.array_equal(cnt[p.check], rcnt)
    mean, aux, st = _device_estimate(p, case)
    smean, saux = SM.scales(case, p, rmean, raux)
    bars = SC.BARS[key[0]]
    qm, qa = SC.quantities(case)
    assert np.array_equal(st, rst), (st, rst)
    em = SM.units(np.atleast_2d(mean), rmean, smean)
    ea = SM.units(aux, raux, saux)
    print("%s %s: mean %.2f (bar %.1f)  aux %.2f (bar %.1f)  units of 2^-53 x scale; status set at %d of %d points"
          % (_id(key), case.op, em, bars[qm]["bar"], ea, bars[qa]["bar"], int((rst != 0).sum()), rst.size))
    assert em <= bars[qm]["bar"], (qm, em, bars[qm])
    assert ea <= bars[qa]["bar"], (qa, ea, bars[qa])


@pytest.mark.parametrize("k", [12, 128])
def test_conditioning_cells_carry_empty_lists_when_the_mask_follows_the_search(k):
    """With the mask applied after the search (and beyond 64 neighbours) the SGS weights kernels write the lists the
    handle returns: the rows of conditioning cells are empty, -1 throughout, like the masked search's own."""
    import gss
    from gss.engine import SGSHandle
    case = SC.Case("masked", 2, 4097, k, nd=6)
    p = SM.problem_of(case)
    vg = gss.ExponentialVariogram(range=4.0 * p.sp * SM.GRID, nugget=0.25)
    h = SGSHandle(vg, p.x, p.path, p.dlocs, np.zeros(p.dlocs.size), 0.0, k, 1, mask_after_search=True)
    idx, nc, _, _ = h.weights()
    h.close()
    assert np.all(idx[p.dlocs] == -1) and np.all(nc[p.dlocs] == 0)
    # every other row: the simulated ones, in order, among the k nearest cells of the whole domain
    full, _, _ = SM.ref_knn(p.mt, p.X, p.C, k)
    for node in np.setdiff1d(np.arange(case.n), p.dlocs)[::37]:
        keep = [j for j in full[node] if p.rank[j] < p.rank[node]]
        assert list(idx[node, :len(keep)]) == keep and np.all(idx[node, len(keep):] == -1)
