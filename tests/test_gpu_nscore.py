"""Normal-score transform on the device (csrc/nscore.hip): the fitted knots against mpmath, interpolation against the
long-double restatement on the library's own knots, the tails against mpmath, every shape at which the kernel takes
another path through both table variants, host staging in chunks, and the front end."""
import os
import runpy

import mpmath as mp
import numpy as np
import pytest

import nscore_cases as NC
import nscore_ref as R

pytestmark = pytest.mark.gpu

VARIANTS = {"lds": "2048", "global": "0"}        # GSS_NSCORE_LDS_KNOTS, read by every gss_nscore_apply


@pytest.fixture(scope="module")
def handles():
    from gss.engine import NScoreHandle
    hs = {}
    for K in NC.TABLE_KNOTS:
        z, w = NC.table_sample(K)
        hs[K] = NScoreHandle(z, w)
    hs["crowded"] = NScoreHandle(*NC.crowded_sample())
    tables = {k: h.table() for k, h in hs.items()}
    yield hs, tables
    for h in hs.values():
        h.close()


@pytest.fixture(params=list(VARIANTS))
def variant(request, monkeypatch):
    monkeypatch.setenv("GSS_NSCORE_LDS_KNOTS", VARIANTS[request.param])
    return request.param


@pytest.mark.parametrize("n", NC.FIT_SIZES)
@pytest.mark.parametrize("weighted", [False, True])
def test_knots_against_mpmath(n, weighted):
    from gss.engine import NScoreHandle
    z, w = NC.sample(n, weighted)
    h = NScoreHandle(z, w)
    v, y = h.table()
    h.close()
    assert np.array_equal(v, R.classes(z, w)[0])                       # the distinct values, bit for bit
    assert np.all(np.diff(y) > 0)
    sub = NC.knot_subset(v.size)
    ym = R.mp_knots(z, w, sub)
    err = max(float(abs(mp.mpf(float(y[k])) - m) / (NC.EPS * max(1, abs(m)))) for k, m in zip(sub, ym))
    print(f"n = {n}, weighted = {weighted}: worst knot {err:.3f} eps max(1, |y|)")
    assert err <= NC.KNOT_BAR_LIB
    # every knot, not only the 1 000 taken at 40 digits: the restatement is within KNOT_BAR_REF of the truth (all its
    # knots: tests/test_nscore_host.py), the library has to be within KNOT_BAR_LIB, so the two are that far apart at most
    yr = R.fit(z, w)[1]
    gap = float(np.max(np.abs(y - yr) / (NC.EPS * np.maximum(1.0, np.abs(yr)))))
    print(f"    all {v.size} knots against the restatement: {gap:.3f}")
    assert gap <= NC.KNOT_BAR_LIB + NC.KNOT_BAR_REF


@pytest.mark.parametrize("n, w", NC.EQUAL_WEIGHT_CASES)
def test_equal_inexact_weights(n, w):
    """An odd number of equal weights that are not exact in binary: the median class sits on p = 1/2 up to the rounding
    of the sums from either end, and gets the score 0."""
    from gss.engine import NScoreHandle
    z, ww = NC.equal_weight_sample(n, w)
    h = NScoreHandle(z, ww)
    v, y = h.table()
    h.close()
    assert np.array_equal(v, z) and np.all(np.diff(y) > 0) and abs(y[n // 2]) <= NC.EPS
    yr = R.fit(z, ww)[1]
    assert np.max(np.abs(y - yr) / np.maximum(1.0, np.abs(yr))) <= (NC.KNOT_BAR_LIB + NC.KNOT_BAR_REF) * NC.EPS


def test_table_above_the_lds_threshold_without_an_override(monkeypatch):
    """3 000 knots, GSS_NSCORE_LDS_KNOTS unset: the library itself chooses the global-memory variant (the table would
    not fit the LDS a launch may ask for).  Held to the long-double restatement like the small tables."""
    import torch
    from gss.engine import NScoreHandle
    monkeypatch.delenv("GSS_NSCORE_LDS_KNOTS", raising=False)
    z, w = NC.table_sample(NC.GLOBAL_TABLE_KNOTS, weighted=True)
    h = NScoreHandle(z, w, tails=(0.0, 2.0 * z.max()))
    v, y = h.table()
    K = v.size
    assert K == NC.GLOBAL_TABLE_KNOTS
    x = _beside(y)
    got = h.inverse(torch.as_tensor(x, device="cuda")).cpu().numpy()
    ref = R.inverse(v, y, x, 0.0, 2.0 * z.max(), dtype=np.longdouble)
    k = np.clip(np.searchsorted(y, x, side="right") - 1, 0, K - 2)
    err = float(np.max(np.abs(got - ref) / (NC.EPS * np.maximum(np.abs(v[k]), np.abs(v[k + 1])))))
    assert np.array_equal(got[np.isin(x, y)], v[np.searchsorted(y, x[np.isin(x, y)])])
    q = _beside(v)
    gotf = h.forward(torch.as_tensor(q, device="cuda")).cpu().numpy()
    reff = R.forward(v, y, q, dtype=np.longdouble)
    errf = float(np.max(np.abs(gotf - reff) / (NC.EPS * np.maximum(1.0, np.abs(reff.astype(np.float64))))))
    assert np.array_equal(gotf[np.isin(q, v)], y[np.searchsorted(v, q[np.isin(q, v)])])
    print(f"K = {K} (library's choice): inverse {err:.3f} eps max|v|, forward {errf:.3f} eps max(1, |y|)")
    assert err <= NC.INTERP_BAR_INV and errf <= NC.INTERP_BAR_FWD
    # a strided in-place call through the same variant
    buf = torch.full((3 * 262 + 1,), 7.0, device="cuda", dtype=torch.float64)
    view = buf.as_strided((3, 257), (262, 1), 1)
    xs = _inputs((v, y), 3 * 257, 12)
    view.copy_(torch.as_tensor(xs.reshape(3, 257), device="cuda"))
    want = h.inverse(torch.as_tensor(xs, device="cuda")).cpu().numpy().reshape(3, 257)
    h.inverse(view, out=view)
    assert np.array_equal(view.cpu().numpy(), want, equal_nan=True)
    h.close()


def _beside(X):
    """Every knot, its two float64 neighbours (inside the table) and points spread between the knots."""
    rng = np.random.default_rng(X.size)
    pts = [X, np.nextafter(X, np.inf), np.nextafter(X, -np.inf)]
    if X.size > 1:
        pts.append(rng.uniform(X[0], X[-1], 3000))
        pts.append(X[:-1] + np.diff(X) * rng.uniform(0, 1, X.size - 1))
    x = np.concatenate(pts)
    return x[(x >= X[0]) & (x <= X[-1])]


@pytest.mark.parametrize("key", list(NC.TABLE_KNOTS) + ["crowded"])
def test_interpolation_against_long_double(handles, variant, key):
    import torch
    hs, tables = handles
    h, (v, y) = hs[key], tables[key]
    K = v.size
    # inverse
    x = _beside(y)
    got = h.inverse(torch.as_tensor(x, device="cuda")).cpu().numpy()
    ref = R.inverse(v, y, x, dtype=np.longdouble)
    k = np.clip(np.searchsorted(y, x, side="right") - 1, 0, max(K - 2, 0))
    scale = np.maximum(np.abs(v[k]), np.abs(v[np.minimum(k + 1, K - 1)]))
    err = float(np.max(np.abs(got - ref) / (NC.EPS * scale)))
    on = np.isin(x, y)
    assert np.array_equal(got[on], v[np.searchsorted(y, x[on])])        # on a knot: the datum itself
    assert np.all((got >= v[k]) & (got <= v[np.minimum(k + 1, K - 1)])) # inside the interval a binary search finds
    # forward
    q = _beside(v)
    gotf = h.forward(torch.as_tensor(q, device="cuda")).cpu().numpy()
    reff = R.forward(v, y, q, dtype=np.longdouble)
    errf = float(np.max(np.abs(gotf - reff) / (NC.EPS * np.maximum(1.0, np.abs(reff.astype(np.float64))))))
    onf = np.isin(q, v)
    assert np.array_equal(gotf[onf], y[np.searchsorted(v, q[onf])])     # a datum gets exactly its class score
    kf = np.clip(np.searchsorted(v, q, side="right") - 1, 0, max(K - 2, 0))
    assert np.all((gotf >= y[kf]) & (gotf <= y[np.minimum(kf + 1, K - 1)]))
    print(f"K = {K} ({variant}): inverse {err:.3f} eps max|v|, forward {errf:.3f} eps max(1, |y|)")
    assert err <= NC.INTERP_BAR_INV and errf <= NC.INTERP_BAR_FWD
    # outside the table the forward direction clamps, NaN stays NaN
    edge = h.forward(torch.tensor([v[0] - 1.0, v[-1] + 1.0, -np.inf, np.inf, np.nan], device="cuda")).cpu().numpy()
    assert edge[:4].tolist() == [y[0], y[-1], y[0], y[-1]] and np.isnan(edge[4])


def test_crowded_table_has_a_crowded_cell(handles):
    """The case earns its name: one cell of the forward guide (2 K cells over [v_1, v_K]) holds tens of knots."""
    v, y = handles[1]["crowded"]
    for X in (v, y):
        cells = np.minimum(((X - X[0]) * (2 * X.size / (X[-1] - X[0]))).astype(np.int64), 2 * X.size - 1)
        print("knots in the fullest cell:", np.bincount(cells).max())
    cells = np.minimum(((v - v[0]) * (2 * v.size / (v[-1] - v[0]))).astype(np.int64), 2 * v.size - 1)
    assert np.bincount(cells).max() >= 30


@pytest.mark.parametrize("name", list(NC.TAIL_CASES))
def test_tails_against_mpmath(variant, name):
    import torch
    from gss.engine import NScoreHandle
    z, w = NC.table_sample(NC.TAIL_TABLE_KNOTS)
    v0 = np.sort(z)
    lo, hi, pw = NC.tail_bounds(name, v0)
    h = NScoreHandle(z, w, tails=(lo, hi), tail_power=pw)
    v, y = h.table()
    x = NC.tail_inputs(y[0], y[-1])
    got = h.inverse(torch.as_tensor(x, device="cuda")).cpu().numpy()
    h.close()
    ref = R.mp_inverse_tails(v, y, x, lo, hi, pw)
    err = NC.tail_error(name, v, x, got, ref)
    print(f"{name} ({variant}): {err:.3f} eps x scale, bar {NC.TAIL_BAR_FACTOR * NC.TAIL_REF_ERR[name]:.2f}")
    assert err <= NC.TAIL_BAR_FACTOR * NC.TAIL_REF_ERR[name]
    zmin, zmax = (v[0] if lo is None else lo), (v[-1] if hi is None else hi)
    assert got[7] == zmin and got[9] == zmin and got[8] == zmax and got[10] == zmax      # +-40 and +-inf
    assert np.all((got[:11] >= zmin) & (got[:11] <= zmax))


def test_single_knot_table(handles, variant):
    import torch
    from gss.engine import NScoreHandle
    h = handles[0][1]
    v, y = handles[1][1]
    assert y.tolist() == [0.0]
    x = torch.tensor([-3.0, 0.0, 2.0, np.nan], device="cuda", dtype=torch.float64)
    assert h.forward(x).cpu().numpy()[:3].tolist() == [0.0, 0.0, 0.0]
    assert h.inverse(x).cpu().numpy()[:3].tolist() == [v[0]] * 3                      # clamp
    t = NScoreHandle([3.5, 3.5], tails=(1.5, 7.5))
    xs = np.array([-1.0, 0.0, 1.0, -np.inf, np.inf, -40.0, 40.0])
    got = t.inverse(torch.as_tensor(xs, device="cuda")).cpu().numpy()
    t.close()
    ref = R.mp_inverse_tails(np.array([3.5]), np.array([0.0]), xs, 1.5, 7.5)
    ref[1] = 3.5
    assert np.max(np.abs(got - ref)) <= 16 * NC.EPS * 7.5
    assert got[3:].tolist() == [1.5, 7.5, 1.5, 7.5]


def _inputs(h_table, n, seed):
    """Scores inside and outside the table, a few of them special."""
    v, y = h_table
    x = np.random.default_rng(seed).normal(0.0, 1.3 * max(1.0, abs(y[-1])), n)
    x[:: 97] = np.nan
    x[5:: 101] = np.inf
    if n > 3:
        x[3] = y[0]
    return x


@pytest.mark.parametrize("K", NC.TABLE_KNOTS)
def test_every_run_shape_gives_the_bits_of_one_plain_call(handles, variant, K):
    """len in {1, 2, 3, 255, 256, 257, 4 099}; runs that start on an even and on an odd element, with source and
    destination alike and unlike within 16 bytes; three runs len + 5 apart; in place and out of place.  The function is
    elementwise, so every one of them must give the bits of a contiguous, aligned call -- and leave the rest alone."""
    import torch
    h, tab = handles[0][K], handles[1][K]
    h2 = None
    if K == 64:                                     # tails that do something
        from gss.engine import NScoreHandle
        z, w = NC.table_sample(K)
        h = h2 = NScoreHandle(z, w, tails=(0.0, 3.0 * z.max()), tail_power=(0.5, 2.0))
    for ln in NC.LENS:
        x = _inputs(tab, 3 * ln, ln)
        want = h.inverse(torch.as_tensor(x, device="cuda")).cpu().numpy()
        stride = ln + 5
        for off_in in (0, 1):
            for off_out in (0, 1, None):                                   # None: in place
                src = torch.full((off_in + 3 * stride + 2,), 7.0, device="cuda", dtype=torch.float64)
                vin = src.as_strided((3, ln), (stride, 1), off_in)
                vin.copy_(torch.as_tensor(x.reshape(3, ln), device="cuda"))
                if off_out is None:
                    dst, vout = src, vin
                else:
                    dst = torch.full((off_out + 3 * stride + 2,), 7.0, device="cuda", dtype=torch.float64)
                    vout = dst.as_strided((3, ln), (stride, 1), off_out)
                ret = h.inverse(vin, out=vout)
                assert ret is vout
                got = vout.cpu().numpy()
                assert np.array_equal(got, want.reshape(3, ln), equal_nan=True), (ln, off_in, off_out)
                mask = torch.ones_like(dst, dtype=torch.bool)
                mask.as_strided((3, ln), (stride, 1), off_in if off_out is None else off_out).fill_(False)
                assert bool((dst[mask] == 7.0).all()), (ln, off_in, off_out)        # gaps and guards untouched
        # one run, out of place into a fresh tensor, forward direction too
        one = torch.as_tensor(x[:ln], device="cuda")
        assert np.array_equal(h.inverse(one).cpu().numpy(), want[:ln], equal_nan=True)
        f = h.forward(one.abs()).cpu().numpy()
        fr = R.forward(tab[0], tab[1], np.abs(x[:ln]))
        assert np.allclose(f, fr, rtol=0, atol=16 * NC.EPS * max(1.0, abs(tab[1][-1])), equal_nan=True)
    if h2 is not None:
        h2.close()


@pytest.mark.parametrize("key", list(NC.TABLE_KNOTS) + ["crowded"])
def test_both_variants_give_the_same_bits(handles, monkeypatch, key):
    import torch
    h, tab = handles[0][key], handles[1][key]
    x = torch.as_tensor(np.concatenate([_inputs(tab, 5000, 1), _beside(tab[1])]), device="cuda")
    q = torch.as_tensor(np.concatenate([np.abs(_inputs(tab, 5000, 2)), _beside(tab[0])]), device="cuda")
    res = {}
    for name, val in VARIANTS.items():
        monkeypatch.setenv("GSS_NSCORE_LDS_KNOTS", val)
        res[name] = (h.inverse(x).cpu().numpy(), h.forward(q).cpu().numpy())
    assert np.array_equal(res["lds"][0], res["global"][0], equal_nan=True)
    assert np.array_equal(res["lds"][1], res["global"][1], equal_nan=True)


def test_host_arrays_in_chunks_give_the_bits_of_the_device_call(handles, monkeypatch):
    import torch
    h, tab = handles[0][1000], handles[1][1000]
    x = _inputs(tab, 3 * 4104, 9)
    want = h.inverse(torch.as_tensor(x, device="cuda")).cpu().numpy()
    monkeypatch.setenv("GSS_NSCORE_CHUNK_ELEMS", "1000")
    assert np.array_equal(h.inverse(x), want, equal_nan=True)                         # 13 chunks
    base = np.full(3 * 4104 + 1, 7.0)
    view = np.lib.stride_tricks.as_strided(base[1:], (3, 4099), (4104 * 8, 8))        # odd start, gaps of 5
    view[:] = x.reshape(3, 4104)[:, :4099]
    out = h.inverse(view)
    assert np.array_equal(out, want.reshape(3, 4104)[:, :4099], equal_nan=True)
    assert h.inverse(view, out=view) is view                                          # in place, on the host
    assert np.array_equal(view, out, equal_nan=True)
    assert base[0] == 7.0 and np.all(base[1:].reshape(3, 4104)[:, 4099:] == 7.0)
    monkeypatch.delenv("GSS_NSCORE_CHUNK_ELEMS")
    assert np.array_equal(h.inverse(x), want, equal_nan=True)


def test_apply_refuses_overlap_and_short_strides(handles):
    import ctypes
    import torch
    from gss import _lib
    h = handles[0][64]
    buf = torch.zeros(100, device="cuda", dtype=torch.float64)
    p = buf.data_ptr()
    lib = _lib.lib()
    ok = lib.gss_nscore_apply(h._h, 1, ctypes.c_void_p(p), ctypes.c_void_p(p), 3, 10, 20, 20, 1, None)
    assert ok == _lib.OK
    for args, word in (((p, p + 8, 1, 10, 10, 10), "overlap"), ((p, p, 3, 10, 20, 25), "overlap"),
                       ((p, p + 400, 3, 10, 8, 20), "shorter"), ((p, p + 4, 1, 10, 10, 10), "aligned")):
        code = lib.gss_nscore_apply(h._h, 1, ctypes.c_void_p(args[0]), ctypes.c_void_p(args[1]), *args[2:], 1, None)
        assert code == _lib.ERR_INVALID and word in _lib.last_error(), (args, _lib.last_error())
    assert lib.gss_nscore_apply(h._h, 2, ctypes.c_void_p(p), ctypes.c_void_p(p), 1, 10, 10, 10, 1, None) == _lib.ERR_INVALID
    torch.cuda.synchronize()


def test_anything_else_is_made_contiguous(handles):
    import torch
    h, tab = handles[0][64], handles[1][64]
    x = _inputs(tab, 600, 4).reshape(20, 30)
    want = h.inverse(torch.as_tensor(x, device="cuda")).cpu().numpy()
    assert np.array_equal(h.inverse(torch.as_tensor(x, device="cuda").t()).cpu().numpy(), want.T, equal_nan=True)
    assert np.array_equal(h.inverse(x[:, ::2]), want[:, ::2], equal_nan=True)
    assert np.array_equal(h.inverse(x.astype(np.float32)), h.inverse(x.astype(np.float32).astype(np.float64)),
                          equal_nan=True)
    assert h.inverse(np.empty((0, 3))).shape == (0, 3)
    with pytest.raises(ValueError):
        h.inverse(x, out=np.empty((20, 31)))
    # input and output that are runs, but not the same runs: through a temporary, the rest of `out` untouched
    a = _inputs(tab, 4 * 3 * 10, 6).reshape(4, 3, 10)
    wa = h.inverse(torch.as_tensor(a, device="cuda")).cpu().numpy()
    for conv in (lambda t: t, lambda t: torch.as_tensor(t, device="cuda")):
        src = conv(a.copy())
        b = conv(np.full((4, 6, 5), 7.0))
        ret = h.inverse(src[:, :, :5], out=b[:, :3])                    # (12, 5, 10) into (4, 15, 30)
        assert ret.shape == (4, 3, 5)
        bn = b.cpu().numpy() if hasattr(b, "cpu") else b
        assert np.array_equal(bn[:, :3], wa[:, :, :5], equal_nan=True) and np.all(bn[:, 3:] == 7.0)
    f32 = np.zeros((20, 30), dtype=np.float32)
    h.inverse(x, out=f32)
    assert np.array_equal(f32, want.astype(np.float32), equal_nan=True)


# ---- front end ----------------------------------------------------------------------------------------------------------------
def _lognormal_data(n=40, seed=11):
    import gss
    rng = np.random.default_rng(seed)
    cells = rng.choice(32 * 32, n, replace=False)
    coords = np.stack([cells % 32 + 0.5, cells // 32 + 0.5], axis=1)
    vals = np.exp(rng.normal(0.0, 1.0, n))
    return gss.georef({"z": vals}, coords), cells, vals


def test_conditional_simulation_in_normal_scores_honours_the_data():
    import gss
    data, cells, vals = _lognormal_data()
    grid = gss.CartesianGrid(32, 32)
    vg = gss.SphericalVariogram(range=10.0)
    ns = gss.NormalScore.fit(vals, tails=(0.0, 2.0 * vals.max()))
    problem = gss.SimulationProblem(data, grid, "z", 6)
    ens = gss.solve(problem, gss.InNormalScores(gss.FFTGS(("z", dict(variogram=vg)), rng=7), z=ns))
    assert len(ens) == 6 and ens.domain is grid
    z = np.stack(ens["z"])
    # the wrapped solver on the scores, same seed: the realisations the wrapper reverted
    inner = gss.solve(gss.SimulationProblem(ns.apply(data, "z"), grid, "z", 6), gss.FFTGS(("z", dict(variogram=vg)), rng=7))
    ysim = np.stack(inner["z"])
    v, y = ns.table()
    scores = ns.forward(vals)
    assert np.array_equal(scores, y[np.searchsorted(v, vals)])
    ref = R.inverse(v, y, ysim, 0.0, 2.0 * vals.max(), dtype=np.longdouble).astype(np.float64)
    k = np.clip(np.searchsorted(y, ysim, side="right") - 1, 0, v.size - 2)
    inside = (ysim >= y[0]) & (ysim <= y[-1])
    assert inside.any() and not inside.all()
    assert np.max((np.abs(z - ref) / np.maximum(v[k], v[k + 1]))[inside]) <= NC.INTERP_BAR_INV * NC.EPS
    tail_bar = NC.TAIL_BAR_FACTOR * NC.TAIL_REF_ERR["linear"] * NC.EPS
    assert np.max((np.abs(z - ref) / np.where(ysim < 0, v[0], 2.0 * vals.max()))[~inside]) <= tail_bar
    # the data in score units are honoured by the wrapped solver at its own tolerance, hence the data in their own
    # units at that tolerance times the steepest slope of the table, plus the interpolation bar
    dy = np.max(np.abs(ysim[:, cells] - scores))
    slope = np.max(np.diff(v) / np.diff(y))
    print(f"scores honoured to {dy:.2e}; steepest slope {slope:.3g}")
    assert dy < 1e-8
    assert np.max(np.abs(z[:, cells] - vals)) <= NC.INTERP_BAR_INV * NC.EPS * vals.max() + slope * dy
    assert z.min() >= 0.0 and z.max() <= 2.0 * vals.max()
    # a transform fitted from the problem's data: clamp tails, every value inside the data's range
    wrapper = gss.InNormalScores(gss.FFTGS(("z", dict(variogram=vg)), rng=7), z=None)
    ens2 = gss.solve(problem, wrapper)
    z2 = np.stack(ens2["z"])
    assert z2.min() >= vals.min() and z2.max() <= vals.max()
    assert np.array_equal(wrapper.fitted["z"].table()[0], v)
    assert np.max(np.abs(z2[:, cells] - vals)) <= NC.INTERP_BAR_INV * NC.EPS * vals.max() + slope * 1e-8


def test_unconditional_simulation_with_a_given_transform():
    import gss
    _, _, vals = _lognormal_data(200, 3)
    ns = gss.NormalScore.fit(vals, tails=(0.0, 3.0 * vals.max()), tail_power=(1.0, 2.0))
    grid = gss.CartesianGrid(32, 32)
    sim = gss.FFTGS(("z", dict(variogram=gss.GaussianVariogram(range=6.0))), rng=3)
    ens = gss.solve(gss.SimulationProblem(grid, "z", 8), gss.InNormalScores(sim, z=ns))
    z = np.stack(ens["z"])
    ysim = np.stack(gss.solve(gss.SimulationProblem(grid, "z", 8),
                              gss.FFTGS(("z", dict(variogram=gss.GaussianVariogram(range=6.0))), rng=3))["z"])
    assert z.shape == (8, 1024) and z.min() >= 0.0 and z.max() <= 3.0 * vals.max()
    assert np.array_equal(z, ns.inverse(ysim))
    # monotone: the ranks of every realisation survive the transform where the scores differ
    o = np.argsort(ysim[0], kind="stable")
    assert np.all(np.diff(z[0][o]) >= 0)


def test_revert_of_a_cosimulation_layout_equals_per_variable_calls():
    """(nreals, nz = 2, N): variable a of every realisation is nreals runs of N, nz N apart -- one launch, read where
    it lies; the other variable is shared with the ensemble it came from."""
    import gss
    import torch
    _, _, vals = _lognormal_data(64, 5)
    ns = gss.NormalScore.fit(vals, tails=(0.0, None))
    rng = np.random.default_rng(8)
    zj = rng.normal(0.0, 1.2, (5, 2, 333))
    grid = gss.CartesianGrid(333)
    for conv in (lambda a: a, lambda a: torch.as_tensor(a, device="cuda")):
        joint = conv(zj)
        ens = gss.Ensemble(grid, {"a": joint[:, 0], "b": joint[:, 1]})
        back = ns.revert(ens, "b")
        assert back["a"] is ens["a"] and back.domain is grid
        got = back["b"]
        got = got.cpu().numpy() if hasattr(got, "cpu") else got
        for r in range(5):
            one = ns.inverse(np.ascontiguousarray(zj[r, 1]))
            assert np.array_equal(got[r], one)
    lists = gss.Ensemble(grid, {"a": [zj[r, 0] for r in range(5)], "b": [zj[r, 1] for r in range(5)]})
    back = ns.revert(lists, "b")
    assert all(np.array_equal(back["b"][r], ns.inverse(np.ascontiguousarray(zj[r, 1]))) for r in range(5))
    assert back["a"] is lists["a"]


def test_apply_keeps_missing_rows():
    import gss
    vals = np.array([3.0, np.nan, 1.0, 2.0, np.nan])
    t = gss.georef({"z": vals, "k": np.arange(5.0)}, np.arange(5.0)[:, None])
    ns = gss.NormalScore.fit(vals)
    s = ns.apply(t, "z")
    assert s.domain is t.domain and s["k"] is t["k"] and t["z"] is not s["z"]
    assert np.isnan(s["z"][[1, 4]]).all() and s["z"][3] == 0.0 and s["z"][2] == -s["z"][0]


def test_example_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ns = runpy.run_path(os.path.join(root, "examples", "normalscore.py"))
    out = ns["out"]
    assert out["honoured"] and out["quantiles_ok"]
