"""Normal-score transform without a device: the numpy restatement (tests/nscore_ref.py) against mpmath at 40 digits,
the argument checks of gss_nscore_create, and the host logic of gss.NormalScore / gss.InNormalScores."""
import ctypes

import mpmath as mp
import numpy as np
import pytest

import gss
import nscore_cases as NC
import nscore_ref as R
from gss import _lib
from gss.engine import _runs


def _knot_errors(y, ym, sub):
    return max(float(abs(mp.mpf(float(y[k])) - m) / (NC.EPS * max(1, abs(m)))) for k, m in zip(sub, ym))


@pytest.fixture(scope="module", params=[(n, w) for n in NC.FIT_SIZES for w in (False, True)],
                ids=lambda p: f"n{p[0]}{'w' if p[1] else ''}")
def fitted(request):
    n, weighted = request.param
    z, w = NC.sample(n, weighted)
    v, y = R.fit(z, w)
    sub = NC.knot_subset(v.size)
    return n, z, w, v, y, sub, R.mp_knots(z, w, sub)


def test_restatement_knots_against_mpmath(fitted):
    n, z, w, v, y, sub, ym = fitted
    err = _knot_errors(y, ym, sub)
    print(f"n = {n}, weighted = {w is not None}: worst knot {err:.3f} eps max(1, |y|)")
    assert err <= NC.KNOT_BAR_REF


def test_every_knot_by_its_float64_residual(fitted):
    """The 40-digit check above takes 1 000 knots of a large table; this one takes them all (bar: NC.KNOT_BAR_RESIDUAL)."""
    from scipy.special import ndtr
    n, z, w, v, y, sub, ym = fitted
    _, W, below, above = R.classes(z, w)
    lower = below <= above
    p = (np.where(lower, below, above) + W / 2) / W.sum()
    yl = np.where(lower, y, -y)                                          # the lower-tail side of every knot
    phi = np.exp(-0.5 * yl.astype(np.longdouble) ** 2) / np.sqrt(2 * np.longdouble(np.pi))
    err = float(np.max(np.abs((ndtr(yl).astype(np.longdouble) - p) / phi) / (NC.EPS * np.maximum(1.0, np.abs(yl)))))
    print(f"n = {n}, weighted = {w is not None}: worst residual over all {v.size} knots {err:.3f} eps max(1, |y|)")
    assert err <= NC.KNOT_BAR_RESIDUAL


def test_one_sided_form_loses_the_upper_tail(fitted):
    """p_k = 1 - q_k as one float64 number: fine for 7 values, far outside the bar from 1 000 on."""
    n, z, w, v, y, sub, ym = fitted
    err = _knot_errors(R.fit_one_sided(z, w)[1], ym, sub)
    print(f"n = {n}, weighted = {w is not None}: one-sided worst knot {err:.1f}")
    if n >= 1000:
        assert err > NC.KNOT_BAR_REF
        top = sub[-1]
        assert abs(R.fit_one_sided(z, w)[1][top] - float(ym[-1])) > abs(y[top] - float(ym[-1]))


def test_knots_increase_and_round_trip(fitted):
    n, z, w, v, y, sub, ym = fitted
    assert np.all(np.diff(v) > 0) and np.all(np.diff(y) > 0)
    assert np.array_equal(R.forward(v, y, v), y)                       # a datum gets exactly its class score
    back = R.inverse(v, y, R.forward(v, y, v))
    assert np.max(np.abs(back - v) / np.abs(v)) <= 4 * NC.EPS
    if w is None:                                                     # equal weights: the scores are antisymmetric
        assert np.array_equal(y, -y[::-1])


def test_transform_is_monotone(fitted):
    n, z, w, v, y, sub, ym = fitted
    rng = np.random.default_rng(n)
    x = np.sort(np.concatenate([rng.normal(0, 1.5, 3000), y[:50], y[-50:], [-9.0, 9.0]]))
    for lo, hi, pw in ((None, None, (1.0, 1.0)), (0.0, 2 * v[-1], (0.5, 2.0))):
        zz = R.inverse(v, y, x, lo, hi, pw)
        assert np.all(np.diff(zz) >= 0)
        assert zz.min() >= (v[0] if lo is None else lo) and zz.max() <= (v[-1] if hi is None else hi)
    q = np.sort(np.concatenate([rng.uniform(0, 2 * v[-1], 3000), v[:50]]))
    assert np.all(np.diff(R.forward(v, y, q)) >= 0)


def test_single_knot():
    v, y = R.fit([3.5, 3.5, 3.5])
    assert v.tolist() == [3.5] and y.tolist() == [0.0]
    assert R.forward(v, y, [-1.0, 3.5, 9.0, np.nan]).tolist()[:3] == [0.0, 0.0, 0.0]
    assert R.inverse(v, y, [-2.0, 0.0, 2.0]).tolist() == [3.5, 3.5, 3.5]                       # clamp
    x = np.array([-1.0, 0.0, 1.0, -np.inf, np.inf])
    got = R.inverse(v, y, x, 1.5, 7.5, (1.0, 1.0))
    q1 = float(mp.erfc(1 / mp.sqrt(2)))                            # Q(1) / Q(0)
    assert np.allclose(got, [1.5 + 2.0 * q1, 3.5, 7.5 - 4.0 * q1, 1.5, 7.5], rtol=4 * NC.EPS, atol=0)


def test_two_knots():
    v, y = R.fit([1.0, 4.0], [1.0, 3.0])
    # classes of weight 1 and 3: p = 1/8 and, from above, 3/8
    assert abs(y[0] - float(R.mp_ndtri_lower(mp.mpf(1) / 8))) <= 4 * NC.EPS * abs(y[0])
    assert abs(y[1] + float(R.mp_ndtri_lower(mp.mpf(3) / 8))) <= 4 * NC.EPS
    mid = 0.5 * (y[0] + y[1])
    assert abs(R.inverse(v, y, [mid])[0] - 2.5) <= 4 * NC.EPS * 4.0
    assert abs(R.forward(v, y, [2.5])[0] - mid) <= 4 * NC.EPS
    assert R.forward(v, y, [0.0, 1.0, 4.0, 5.0]).tolist() == [y[0], y[0], y[1], y[1]]


def test_ties_are_merged_with_their_weights():
    v, y = R.fit([2.0, 1.0, 2.0, 3.0, 2.0])
    v2, y2 = R.fit([1.0, 2.0, 3.0], [1.0, 3.0, 1.0])
    assert np.array_equal(v, v2) and np.array_equal(y, y2) and y[1] == 0.0


@pytest.mark.parametrize("name", list(NC.TAIL_CASES))
def test_recorded_tail_error_is_reproduced(name):
    """The float64 restatement against mpmath on the tail inputs: what NC.TAIL_REF_ERR records (the device is held to
    16 x that in tests/test_gpu_nscore.py)."""
    z, w = NC.table_sample(NC.TAIL_TABLE_KNOTS)
    v, y = R.fit(z, w)
    x = NC.tail_inputs(y[0], y[-1])
    lo, hi, pw = NC.tail_bounds(name, v)
    got = R.inverse(v, y, x, lo, hi, pw)
    ref = R.mp_inverse_tails(v, y, x, lo, hi, pw)
    err = NC.tail_error(name, v, x, got, ref)
    print(f"{name}: float64 restatement {err:.4f} eps x scale (recorded {NC.TAIL_REF_ERR[name]})")
    assert err <= NC.TAIL_REF_ERR[name] <= 1.01 * err + 1e-3
    # Q underflows at +-40: the bounds exactly
    assert got[7] == (v[0] if lo is None else lo) and got[8] == (v[-1] if hi is None else hi)
    assert got[9] == got[7] and got[10] == got[8]


# ---- gss_nscore_create: every GSS_ERR_INVALID is found before the device is touched ------------------------------------
def _create(z, w=None, zmin=np.nan, zmax=np.nan, plo=1.0, phi=1.0, n=None):
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    h = ctypes.c_void_p()
    code = lib.gss_nscore_create(ctypes.byref(h), _lib.ptr(z), _lib.ptr(w), z.size if n is None else n, zmin, zmax, plo, phi,
                                 None)
    msg = _lib.last_error()
    if code == _lib.OK:
        lib.gss_nscore_destroy(h)
    return code, msg


@pytest.mark.parametrize("kw, word", [
    (dict(z=[1.0], n=0), "at least one"),
    (dict(z=[1.0, np.inf]), "value 1 is not finite"),
    (dict(z=[1.0, np.nan, 2.0]), "value 1 is not finite"),
    (dict(z=[1.0, 2.0], w=[1.0, 0.0]), "weight 1"),
    (dict(z=[1.0, 2.0], w=[-1.0, 1.0]), "weight 0"),
    (dict(z=[1.0, 2.0], w=[1.0, np.inf]), "weight 1"),
    (dict(z=[1.0, 2.0], zmin=1.5), "zmin"),
    (dict(z=[1.0, 2.0], zmax=1.5), "zmax"),
    (dict(z=[1.0, 2.0], zmin=-np.inf), "zmin"),
    (dict(z=[1.0, 2.0], plo=0.0), "powers"),
    (dict(z=[1.0, 2.0], phi=-1.0), "powers"),
    (dict(z=[1.0, 2.0], phi=np.nan), "powers"),
    (dict(z=[1.0, 2.0, 3.0, 4.0], w=[1.0, 1e-30, 1e-30, 1.0]), "knot 2"),     # both middle classes land on p = 1/2
])
def test_create_refuses_bad_arguments_without_a_device(kw, word):
    code, msg = _create(**kw)
    assert code == _lib.ERR_INVALID and word in msg, (code, msg)


@pytest.mark.parametrize("n, w", NC.EQUAL_WEIGHT_CASES)
def test_equal_inexact_weights_are_not_refused(n, w):
    """The median class of an odd number of equal weights has p = 1/2 in exact arithmetic and 1/2 + 2^-64 in the sums:
    the fit must take it (score 0), not call the weights uneven.  Without a device the call ends at the upload, which
    is after every argument check."""
    z, ww = NC.equal_weight_sample(n, w)
    code, msg = _create(z, ww)
    assert code != _lib.ERR_INVALID and "uneven" not in msg, (code, msg)
    v, y = R.fit(z, ww)
    assert np.all(np.diff(y) > 0) and abs(y[n // 2]) <= NC.EPS and np.max(np.abs(y + y[::-1])) <= 4 * NC.EPS * y[-1]


def test_apply_and_table_refuse_a_null_handle():
    lib = _lib.load()
    k = ctypes.c_int64()
    assert lib.gss_nscore_info(None, ctypes.byref(k)) == _lib.ERR_INVALID
    assert lib.gss_nscore_apply(None, 1, None, None, 1, 1, 1, 1, 0, None) == _lib.ERR_INVALID
    assert lib.gss_nscore_table(None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.gss_nscore_destroy(None) == _lib.OK


# ---- front end ----------------------------------------------------------------------------------------------------------------
def test_fit_drops_nan_rows_and_checks_its_arguments():
    ns = gss.NormalScore.fit([3.0, np.nan, 1.0, 2.0], weights=[1.0, 5.0, 2.0, 1.0])
    assert ns.values.tolist() == [3.0, 1.0, 2.0] and ns.weights.tolist() == [1.0, 2.0, 1.0]
    assert ns.bounds == (1.0, 3.0)
    assert gss.NormalScore.fit([1.0, 2.0], tails=(0.0, None)).bounds == (0.0, 2.0)
    with pytest.raises(AssertionError, match="missing"):
        gss.NormalScore.fit([np.nan, np.nan])
    for kw in (dict(values=[1.0, np.inf]), dict(values=[1.0, 2.0], weights=[1.0]),
               dict(values=[1.0, 2.0], weights=[1.0, 0.0]), dict(values=[1.0, 2.0], tails=(1.5, None)),
               dict(values=[1.0, 2.0], tails=(None, 1.5)), dict(values=[1.0, 2.0], tail_power=(0.0, 1.0))):
        with pytest.raises(ValueError):
            gss.NormalScore.fit(**kw)


def test_in_normal_scores_checks_its_arguments():
    ns = gss.NormalScore.fit([1.0, 2.0, 3.0])
    sim = gss.FFTGS(z=dict(variogram=gss.GaussianVariogram(range=5.0)))
    for est in (gss.KrigingSolver(z=dict(variogram=gss.GaussianVariogram(range=5.0))), gss.IDWSolver()):
        with pytest.raises(TypeError, match="biased"):
            gss.InNormalScores(est, z=ns)
    with pytest.raises(ValueError, match="at least one"):
        gss.InNormalScores(sim)
    with pytest.raises(TypeError, match="NormalScore or None"):
        gss.InNormalScores(sim, z=3.0)
    grid = gss.CartesianGrid(8, 8)
    with pytest.raises(ValueError, match="not among"):
        gss.InNormalScores(sim, w=ns).solve(gss.SimulationProblem(grid, "z", 1))
    with pytest.raises(ValueError, match="no data"):
        gss.InNormalScores(sim, z=None).solve(gss.SimulationProblem(grid, "z", 1))
    data = gss.georef({"z": [1.0, 2.0]}, [(1.0, 1.0), (5.0, 5.0)])
    with pytest.raises(TypeError, match="SimulationProblem"):
        gss.InNormalScores(sim, z=None).solve(gss.EstimationProblem(data, grid, "z"))
    assert gss.InNormalScores(gss.SGS(), z=ns).transforms == {"z": ns}


def test_runs_of_strided_views():
    """What NScoreHandle hands to gss_nscore_apply as (nblocks, len, stride) for an array's shape and element strides."""
    a = np.zeros((4, 3, 10))
    es = lambda x: tuple(s // 8 for s in x.strides)
    assert _runs(a.shape, es(a)) == (1, 120, 120)
    b = a[:, 1]
    assert _runs(b.shape, es(b)) == (4, 10, 30)                      # one variable of a co-simulation
    c = a[:, :2]
    assert _runs(c.shape, es(c)) == (4, 20, 30)
    d = a[:, :, :5]
    assert _runs(d.shape, es(d)) == (12, 5, 10)                      # both leading axes collapse into one stride
    assert _runs(a[:, :2, :5].shape, es(a[:, :2, :5])) is None       # two different leading strides
    assert _runs(a[::-1].shape, es(a[::-1])) is None
    assert _runs(a[:, :, ::2].shape, es(a[:, :, ::2])) is None or _runs(a[:, :, ::2].shape, es(a[:, :, ::2]))[1] == 1
    assert _runs(a[0, 0, 3:4].shape, es(a[0, 0, 3:4])) == (1, 1, 1)
    assert _runs((0, 5), (5, 1)) is None
