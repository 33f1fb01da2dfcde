"""Indicator kriging on the device (gss_ik_predict_knn, gss_ik_order_relations, gss_ik_post) against the numpy
restatement tests/ik_ref.py on the cases of tests/ik_cases.py and on the table tests/ik_kernel_cases.py, which has one case
per compiled instantiation of ik_local_kernel.

Raw ccdf: |device - reference| <= bar x 2^-53 max(1, sum |lambda|) per (point, cutoff), bar = 16 x the largest error of
the FP64 restatement against the long-double one on the same inputs (ORACLE, measured on the CPU by tools/ik_oracle.py),
floored at 8 and capped at 1e-9 as tests/test_kernel_census.py holds the kriging bars.  Corrected ccdf: bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gss
import ik_cases
import ik_kernel_cases
import ik_ref

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -53
# tools/ik_oracle.py: FP64 restatement against long double, in the units above
ORACLE = {
    'k1': 2.0, 'k15': 3.08, 'k16': 5.6, 'k17': 2.36, 'k33': 6.25, 'k64': 3.07,
    'K1_ok': 9.78, 'K1_sk': 8.25, 'K2_ok': 3.47, 'K2_sk': 2.9, 'K14_ok': 5.89, 'K14_sk': 4.72, 'K15_ok': 4.19,
    'K15_sk': 3.77, 'K16_ok': 10.21, 'K16_sk': 11.69,
    'kind0': 3.44, 'kind1': 2.56, 'kind2': 4.6, 'kind3': 3.51, 'kind4': 3.83, 'kind5': 3.27, 'kind6': 3.27,
    'full_ok': 6.43, 'full_sk': 6.33, 'all_below': 3.97, 'all_above': 0.0, 'missing': 4.09, 'duplicate': 2.17,
    'order': 613.87,
    'K16_ok_k12': 3.89, 'full_ok_k12': 3.49, 'K16_sk_k12': 3.87, 'full_sk_k12': 3.54, 'K16_ok_k40': 7.34,
    'full_ok_k40': 8.04, 'K16_sk_k40': 4.26, 'full_sk_k40': 3.45, 'dim1': 7.34, 'dim1_full': 468.6,
    'route_ok': 4.57, 'route_sk': 2.32, 'route_full': 2.3,
    # the dual form of the global route (ik_ref.predict_global), in the units of the moving route
    'route_ok_global': 3.61, 'route_sk_global': 3.14, 'route_full_global': 8.44,
    # one entry per compiled ik_local_kernel<DIM, KIND, NT, FULL> (tests/ik_kernel_cases.py; g: the general kernel)
    'ik_2_0_1_median': 2.48, 'ik_2_0_2_median': 5.59, 'ik_2_0_4_median': 6.02, 'ik_2_1_1_median': 2.33,
    'ik_2_1_2_median': 4.03, 'ik_2_1_4_median': 9.02, 'ik_2_2_1_median': 4.47, 'ik_2_2_2_median': 6.4,
    'ik_2_2_4_median': 8.03, 'ik_2_30_1_median': 2.95, 'ik_2_30_2_median': 5.31, 'ik_2_30_4_median': 5.66,
    'ik_2_31_1_median': 3.46, 'ik_2_31_2_median': 4.71, 'ik_2_31_4_median': 6.32, 'ik_2_32_1_median': 4.13,
    'ik_2_32_2_median': 4.57, 'ik_2_32_4_median': 7.71, 'ik_3_0_1_median': 1.72, 'ik_3_0_2_median': 3.16,
    'ik_3_0_4_median': 5.1, 'ik_3_1_1_median': 1.78, 'ik_3_1_2_median': 2.22, 'ik_3_1_4_median': 4.15,
    'ik_3_2_1_median': 2.75, 'ik_3_2_2_median': 4.86, 'ik_3_2_4_median': 5.67, 'ik_3_30_1_median': 2.44,
    'ik_3_30_2_median': 4.59, 'ik_3_30_4_median': 5.65, 'ik_3_31_1_median': 2.85, 'ik_3_31_2_median': 2.6,
    'ik_3_31_4_median': 4.91, 'ik_3_32_1_median': 2.6, 'ik_3_32_2_median': 4.42, 'ik_3_32_4_median': 4.1,
    'ik_1_g_1_median': 9.48, 'ik_1_g_1_full': 8.78, 'ik_1_g_2_median': 10.49, 'ik_1_g_2_full': 9.22,
    'ik_1_g_4_median': 13.64, 'ik_1_g_4_full': 14.3, 'ik_2_g_1_median': 3.26, 'ik_2_g_1_full': 3.55,
    'ik_2_g_2_median': 4.47, 'ik_2_g_2_full': 5.22, 'ik_2_g_4_median': 6.66, 'ik_2_g_4_full': 8.14, 'ik_3_g_1_median':
    2.6, 'ik_3_g_1_full': 1.66, 'ik_3_g_2_median': 2.19, 'ik_3_g_2_full': 4.0, 'ik_3_g_4_median': 5.12,
    'ik_3_g_4_full': 4.84,
    # post-processing: the hand-made rows, and the corrected ccdfs of the cases with ik_cases.post_args_for
    'post': 1.33, 'post_cases': 2.01,
}


def bar(name):
    return min(max(16.0 * ORACLE[name], 8.0), 1e-9 / (UNIT * 1.5))


@pytest.fixture(scope="module")
def eng():
    from gss.engine import HipEngine
    return HipEngine


CASES = ik_cases.cases()
KERNEL_CASES = {key: fn for key, fn in ik_kernel_cases.KERNELS.items()
                if not isinstance(fn, ik_kernel_cases.UNREACHABLE)}
CHUNK_ENV = "GSS_IK_CHUNK_POINTS"
_REF = {}


def ref_of(name):
    """The reference of a case, computed once and shared (callers must not modify it)."""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = ik_ref.predict(c["x"], c["z"], c["x0"], c["cutoffs"], c["models"], c["k"],
                                    minneighbors=c.get("minneighbors", 1), fstar=c["fstar"], radius=c.get("radius"))
    return _REF[name]


def device_of(eng, c, **kw):
    models = c["models"][0] if len(c["models"]) == 1 else c["models"]
    return eng.ik_predict_knn(c["x"], c["z"], c["x0"], c["cutoffs"], models, c["k"],
                              minneighbors=c.get("minneighbors", 1), fstar=c["fstar"], radius=c.get("radius"),
                              return_raw=True, return_idx=True, **kw)


def check_against_reference(eng, name, c, r):
    """One case on the device against its reference r: lists, counts and statuses equal, raw ccdf within bar(name),
    corrected ccdf bit for bit the correction of the device's own raw values, the correction's two figures exact."""
    ccdf, st, raw, idx, cnt = device_of(eng, c)
    assert np.array_equal(cnt, r["cnt"]) and np.array_equal(idx, r["idx"])
    assert np.array_equal(st, r["status"]), (np.flatnonzero(st != r["status"]), st[st != r["status"]])
    ok = r["status"] == 0
    assert np.isnan(raw[~ok]).all() and np.isnan(ccdf[~ok]).all()
    if name == "order":   # the correction path is provably exercised: the REFERENCE's raw values violate the relations
        rr = r["raw"]
        viol = ((rr < 0.0) | (rr > 1.0)).any(axis=1) | (np.diff(rr, axis=1) < 0.0).any(axis=1)
        assert viol.mean() >= 0.05, viol.mean()
    if name == "missing":
        assert (r["status"] == 1).any() and ok.any()
    if name == "duplicate":
        assert (r["status"][:6] == 2).all() and (r["status"][6:] == 0).all()
    err = np.abs(raw[ok] - r["raw"][ok]) / (UNIT * r["wsum"][ok])
    worst = float(err.max()) if ok.any() else 0.0
    print(f"{name}: raw error {worst:.2f} units, bar {bar(name):.2f}")
    assert worst <= bar(name), (name, worst, bar(name))
    # corrected: the correction alone on the reference's raw values is the reference's corrected values, and the fused
    # path is the correction alone on the device's own raw values -- bit for bit, no point left out
    alone, _, _ = eng.ik_order_relations(r["raw"].copy())
    assert np.array_equal(alone, r["ccdf"], equal_nan=True)
    own, ncorr, maxcorr = eng.ik_order_relations(raw.copy())
    assert np.array_equal(own, ccdf, equal_nan=True)
    changed = (own != raw) & ~np.isnan(raw)
    assert ncorr == int(changed.sum())
    assert maxcorr == (float(np.abs(own - raw)[changed].max()) if changed.any() else 0.0)
    if name == "all_below":
        assert np.all(ccdf[ok] == 1.0) or np.max(np.abs(ccdf[ok] - 1.0)) <= bar(name) * UNIT * r["wsum"][ok].max()
    if name == "all_above":
        assert np.all(raw[ok] == 0.0) and np.all(ccdf[ok] == 0.0)


@pytest.mark.parametrize("name", list(CASES))
def test_device_against_reference(eng, name):
    check_against_reference(eng, name, CASES[name], ref_of(name))


@pytest.mark.parametrize("key", list(KERNEL_CASES), ids=lambda key: ik_kernel_cases.name_of(key))
def test_every_compiled_kernel(eng, key):
    """Every entry of tests/ik_kernel_cases.py (one per compiled ik_local_kernel<DIM, KIND, NT, FULL>;
    tests/test_ik_census.py holds the table against the built library) under the assertions of
    test_device_against_reference, no point left out (every status of these cases is 0)."""
    c = KERNEL_CASES[key]()
    r = ik_ref.predict(c["x"], c["z"], c["x0"], c["cutoffs"], c["models"], c["k"], fstar=c["fstar"], radius=c["radius"])
    assert not r["status"].any()
    check_against_reference(eng, ik_kernel_cases.name_of(key), c, r)


def ccdf_alone(c):
    """gss_ik_predict_knn with the corrected ccdf as its only output: raw, status, idx_out and count_out NULL (the engine
    always asks for the status), host arrays."""
    from gss import _lib
    from gss import _staging as st
    from gss.engine import OK, SK, _vg_struct
    x, z, x0 = (np.ascontiguousarray(c[a], dtype=np.float64) for a in ("x", "z", "x0"))
    cut = np.ascontiguousarray(c["cutoffs"], dtype=np.float64)
    fs = None if c["fstar"] is None else np.ascontiguousarray(c["fstar"], dtype=np.float64)
    n, d = x.shape
    m, K = x0.shape[0], cut.size
    vgs = (_lib.Variogram * len(c["models"]))(*[_vg_struct(v, d) for v in c["models"]])
    r, ir, met, mpar = st.search_args(c.get("radius"), None)
    ccdf = np.full((m, K), -7.0)
    _lib.check(_lib.lib().gss_ik_predict_knn(_lib.ptr(x), _lib.ptr(z), n, d, _lib.ptr(cut), K, vgs, len(c["models"]),
                                             SK if fs is not None else OK, _lib.ptr(fs), int(c["k"]),
                                             int(c.get("minneighbors", 1)), r, _lib.ptr(ir), met, mpar, _lib.ptr(x0), m,
                                             _lib.ptr(ccdf), None, None, None, None, _lib.MEM_HOST,
                                             _lib.current_stream()))
    return ccdf


@pytest.mark.parametrize("key", [(2, 2, 2, False), (3, -1, 2, True)], ids=lambda key: ik_kernel_cases.name_of(key))
def test_chunks(eng, key):
    """The chunk loop of gss_ik_predict_knn past its first turn: 67 points under a cap of 16 are five chunks, the last
    one of three points.  With every optional output (each offset by the chunk) and with none (the driver's own list,
    count and status scratch reused by every chunk): bit for bit the one-chunk call."""
    c = KERNEL_CASES[key]()
    assert c["x0"].shape[0] == 67
    one = device_of(eng, c)
    os.environ[CHUNK_ENV] = "16"
    try:
        every = device_of(eng, c)
        bare = ccdf_alone(c)
    finally:
        del os.environ[CHUNK_ENV]
    assert not one[1].any() and np.isfinite(one[0]).all()
    for a, b in zip(one, every):
        assert np.array_equal(a, b)
    assert np.array_equal(bare, one[0])


def test_post_against_reference(eng):
    rows = [ik_cases.post_rows()]
    cuts = ik_cases.POST_CUTOFFS
    kw = ik_cases.POST_ARGS
    b = bar("post")
    scales = dict(etype=kw["zmax"], cvar=kw["zmax"] ** 2, pabove=1.0, quant=kw["zmax"])
    for wlo, whi in ((1.0, 1.0), (2.5, 2.5), (1.0, 2.5)):
        for F in rows:
            d = eng.ik_post(F, cuts, kw["zmin"], kw["zmax"], (wlo, whi), kw["thresholds"], kw["probs"])
            r = ik_ref.post(F, cuts, kw["zmin"], kw["zmax"], wlo, whi, kw["thresholds"], kw["probs"])
            for key, scale in scales.items():
                assert np.array_equal(np.isnan(d[key]), np.isnan(r[key])), key
                err = np.nanmax(np.abs(d[key] - r[key])) / (UNIT * scale)
                print(f"post {key} w=({wlo}, {whi}): {err:.2f} units, bar {b:.2f}")
                assert err <= b, (key, wlo, whi, err)
            assert np.isnan(d["etype"][6]) and np.isnan(d["pabove"][6]).all() and np.isnan(d["quant"][6]).all()


@pytest.mark.parametrize("name", list(CASES))
def test_post_on_corrected_ccdfs(eng, name):
    """gss_ik_post on the corrected ccdf of every case; the bar is measured on these very inputs (ORACLE "post_cases")."""
    c, r = CASES[name], ref_of(name)
    kw = ik_cases.post_args_for(c)
    b = bar("post_cases")
    scales = dict(etype=kw["zmax"], cvar=kw["zmax"] ** 2, pabove=1.0, quant=kw["zmax"])
    for wlo, whi in ik_cases.POST_TAILS:
        d = eng.ik_post(r["ccdf"], c["cutoffs"], kw["zmin"], kw["zmax"], (wlo, whi), kw["thresholds"], kw["probs"])
        q = ik_ref.post(r["ccdf"], c["cutoffs"], kw["zmin"], kw["zmax"], wlo, whi, kw["thresholds"], kw["probs"])
        for key, scale in scales.items():
            assert np.array_equal(np.isnan(d[key]), np.isnan(q[key])), key
            if np.isfinite(q[key]).any():
                assert np.nanmax(np.abs(d[key] - q[key])) / (UNIT * scale) <= b, (key, wlo, whi)


def test_host_and_device_arrays_give_the_same_bits(eng):
    import torch
    c = CASES["k33"]
    host = device_of(eng, c)
    xd = torch.as_tensor(c["x0"], device="cuda")
    c2 = dict(c, x0=xd)
    dev = device_of(eng, c2)
    for a, b in zip(host, dev):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)
    F = torch.as_tensor(host[0], device="cuda")
    p1 = eng.ik_post(host[0], c["cutoffs"], 0.0, 100.0, (1.0, 2.0), (1.0,), (0.5,))
    p2 = eng.ik_post(F, c["cutoffs"], 0.0, 100.0, (1.0, 2.0), (1.0,), (0.5,))
    for key in p1:
        assert np.array_equal(p1[key], p2[key].cpu().numpy(), equal_nan=True)


def test_solver_and_postik_match_the_handle_level_calls(eng):
    rng = np.random.default_rng(3)
    x = rng.uniform(0.0, 20.0, (150, 2))
    z = np.exp(rng.normal(size=150))
    cut = np.quantile(z, [0.2, 0.5, 0.8])
    g = gss.SphericalVariogram(range=8.0, nugget=0.1)
    grid = gss.CartesianGrid((20, 20))
    data = gss.georef({"z": z}, x)
    w = np.ones(150)
    solver = gss.IndicatorKrigingSolver(("z", dict(cutoffs=cut, variogram=g, maxneighbors=12, mean="global", weights=w)))
    sol = gss.solve(gss.EstimationProblem(data, grid, "z"), solver)
    fstar = np.array([np.mean(z <= c) for c in cut])
    ccdf, st = eng.ik_predict_knn(x, z, grid.centroids(), cut, g, 12, fstar=fstar)
    for i in range(3):
        assert np.array_equal(sol[f"z_ccdf_{i}"], ccdf[:, i], equal_nan=True)
    post = gss.postik(sol, "z", zmin=0.0, zmax=40.0, tail_power=(1.0, 2.0), thresholds=(1.0, 3.0), probs=(0.5,))
    d = eng.ik_post(ccdf, cut, 0.0, 40.0, (1.0, 2.0), (1.0, 3.0), (0.5,))
    assert np.array_equal(post["z_etype"], d["etype"]) and np.array_equal(post["z_cvar"], d["cvar"])
    assert np.array_equal(post["z_pabove_1"], d["pabove"][:, 1]) and np.array_equal(post["z_q_0"], d["quant"][:, 0])


@pytest.mark.parametrize("name", ["route_ok", "route_sk", "route_full"])
def test_global_route_matches_the_moving_route_with_every_sample(eng, name):
    """Both routes solve the system of all n = 48 samples.  Each is held to its own derived bar against the reference,
    in units of 2^-53 max(1, sum |lambda|) (the largest over the row: the correction mixes the cutoffs of a point and
    is 1-Lipschitz): the moving route to the raw bar of the case, the global route to 16 x the FP64-against-long-double
    error of its dual form (ORACLE "<case>_global").  Their difference is then within the sum of the two."""
    import torch
    c, r = CASES[name], ref_of(name)
    x, z, x0, cut, n = c["x"], c["z"], c["x0"], c["cutoffs"], c["k"]
    vkw = dict(variogram=c["models"][0]) if len(c["models"]) == 1 else dict(variograms=c["models"])
    mean = None if c["fstar"] is None else "global"
    prob = gss.EstimationProblem(gss.georef({"z": z}, x), gss.PointSet(x0), "z")
    gsolver = gss.IndicatorKrigingSolver(("z", dict(cutoffs=cut, maxneighbors=None, mean=mean, **vkw)))
    glob = gss.solve(prob, gsolver)
    mov = gss.solve(prob, gss.IndicatorKrigingSolver(("z", dict(cutoffs=cut, maxneighbors=n, mean=mean, **vkw))))
    gdev = gsolver._global(gsolver.preprocess(prob)["z"], torch.as_tensor(x0, device="cuda"))   # a CUDA domain
    unit = UNIT * r["wsum"].max(axis=1)
    for i in range(cut.size):
        a, b = glob[f"z_ccdf_{i}"], mov[f"z_ccdf_{i}"]
        em = float(np.max(np.abs(b - r["ccdf"][:, i]) / unit))
        eg = float(np.max(np.abs(a - r["ccdf"][:, i]) / unit))
        ed = float(np.max(np.abs(gdev[:, i] - r["ccdf"][:, i]) / unit))
        print(f"{name} cutoff {i}: moving {em:.2f} (bar {bar(name):.2f}), global {eg:.2f} / {ed:.2f} on a CUDA domain "
              f"(bar {bar(name + '_global'):.2f})")
        assert em <= bar(name)
        assert eg <= bar(name + "_global") and ed <= bar(name + "_global")
        assert np.max(np.abs(a - b) / unit) <= bar(name) + bar(name + "_global")


def test_validation(eng):
    from gss._lib import GSSError
    c = CASES["k16"]
    x, z, x0, cut, g = c["x"], c["z"], c["x0"][:5], c["cutoffs"], c["models"][0]
    for bad in ([1.0, 1.0], [2.0, 1.0], [np.nan], np.arange(17.0), []):
        with pytest.raises(GSSError) as e:
            eng.ik_predict_knn(x, z, x0, bad, g, 8)
        assert e.value.code == 1
    with pytest.raises(GSSError) as e:
        eng.ik_predict_knn(x, z, x0, cut, g, 65)
    assert e.value.code == 4
    with pytest.raises(GSSError):
        eng.ik_predict_knn(x, z, x0, cut, [g, g], 8)              # neither one nor K variograms
    F = np.array([[0.2, 0.5]])
    for kw in (dict(zmin=1.0), dict(zmax=2.0), dict(tail_power=(0.0, 1.0)), dict(probs=(1.0,)), dict(thresholds=(31.0,))):
        a = dict(zmin=0.0, zmax=30.0, tail_power=(1.0, 1.0), thresholds=(), probs=())
        a.update(kw)
        with pytest.raises(GSSError):
            eng.ik_post(F, [1.0, 2.0], a["zmin"], a["zmax"], a["tail_power"], a["thresholds"], a["probs"])
