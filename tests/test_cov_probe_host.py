"""The tables of tests/cov_probe.py hold what tests/test_gpu_cov_probe.py relies on (no GPU): every switch of every
evaluator has lags on both sides, where the device's own text puts it; the lag lists hold the zero and denormal lags and
no duplicates; the committed ORACLE figures are what tools/cov_probe_oracle.py measures; a one-sample simple-kriging
mean is the covariance and nothing else; the 50-digit reference agrees with tests/kernel_matrix.py; no lag is dropped."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cov_probe as cp  # noqa: E402
import cov_probe_oracle as tool  # noqa: E402
import kernel_matrix as km  # noqa: E402

# The thresholds, written out a second time on purpose: cov_probe.switch_sides must put every lag on the side these
# put it, and the header must hold the comparison in these words (HEADER_TEXT), so that neither the table nor the
# device can move a switch alone.
EXPECTED = {
    "temme_steed": lambda m, a: a <= 2.0,
    "cheb_p_q": lambda m, a: a <= 2.0,
    "zero": lambda m, a: ~(a > 700.0),
    "one": lambda m, a: m.nu * np.log(2.0 / a) + ((m.nu - 0.5) * np.log(m.nu) - m.nu + 1.01) > 690.0,
    "range": lambda m, a: a < 1.0,
}
HEADER_TEXT = (
    "if (d <= 2.0) {",                                                  # gss_matern_general: Temme / Steed
    "if (x <= 2.0) {",                                                  # gss_bessel_k0_xk1: P / Q expansions
    "if (d > 700.0) return 0.0;",                                       # both Matern families
    "if (nu * log(2.0 / d) + ((nu - 0.5) * log(nu) - nu + 1.01) > 690.0) return 1.0 - d * d / (4.0 * (nu - 1.0));",
    "return x < 1.0 ? 1.0 - (1.5 * x - 0.5 * x * x * x) : 0.0;",
    "return x < 1.0 ? 1.0 - (7.0 * x2 - 8.75 * x3 + 3.5 * x3 * x2 - 0.75 * x3 * x3 * x) : 0.0;",
    "return x < 1.0 ? 1.0 - (1.875 * x - 1.25 * x3 + 0.375 * x3 * x2) : 0.0;",
    "const double fact = fabs(pimu) < 1e-15 ? 1.0 : pimu / sin(pimu);",
    "const double fact2 = fabs(e) < 1e-15 ? 1.0 : sinh(e) / e;",
    "const int n = (int)floor(nu + 0.5);",
    "fmax(d2, 1e-300)",
    "if (v.cs != v.sill) {",
)


def _single(m):
    return m.terms[0][1] if m.terms else m


def _runs():
    for m in cp.ALL.values():
        for dim in (1, 2, 3):
            for ball in ((False, True) if (dim > 1 and m.name in cp.BALL_MODELS) else (False,)):
                yield m, dim, ball


def test_header_holds_the_switches_in_these_words():
    with open(tool.HEADER) as f:
        text = f.read()
    for line in HEADER_TEXT:
        assert line in text, line


def test_every_switch_has_lags_on_both_sides_where_the_device_puts_it():
    seen = 0
    for m, dim, ball in _runs():
        s = _single(m)
        pts = cp.points(m, dim, ball)
        for unit in ((False, True) if s.name in cp.UNIT_KINDS else (False,)):
            sides = cp.switch_sides(s, dim, ball, pts, unit)
            assert set(sides) == set(cp.switches(s))
            arg = cp.shape_arg(s, dim, ball, pts, unit)
            for name, lower in sides.items():
                assert lower.any() and (~lower).any(), (m.name, dim, ball, unit, name)
                with np.errstate(divide="ignore"):
                    want = EXPECTED[name](s, arg)
                assert np.array_equal(lower, want), (m.name, dim, ball, unit, name)
                # the two sides meet within a few doubles along every direction: the neighbours, not just the ladder
                for u in cp.directions(dim):
                    on = np.all((pts != 0.0) == (u != 0.0)[None, :], axis=1)
                    lo, hi = np.max(arg[on & lower]), np.min(arg[on & ~lower])
                    assert lo < hi and hi - lo <= 8.0 * np.spacing(hi), (m.name, dim, ball, unit, name, lo, hi)
                seen += 1
    assert seen > 100
    # which models have which switches
    assert set(cp.switches(cp.ALL["cubic"])) == {"range"} and set(cp.switches(cp.ALL["matern_2.0"])) == {"cheb_p_q", "zero"}
    assert set(cp.switches(cp.ALL["matern_0.7"])) == {"temme_steed", "zero"}
    for nu in (4.2, 9.5, 20.0, 40.0, 50.0):
        assert set(cp.switches(cp.ALL["matern_%r" % nu])) == {"temme_steed", "zero", "one"}


def test_lag_lists():
    assert len(cp.MODELS) == 15 + 9 + 6 + 4 + 2 + 2 and len(cp.NESTED) == 3
    orders = sorted(m.nu for m in cp.MODELS.values() if m.kind == "matern")
    for h in (0.5, 1.5, 2.5, 1.0):
        i = orders.index(h)
        assert orders[i - 1] == np.nextafter(h, -np.inf) and orders[i + 1] == np.nextafter(h, np.inf)
    for m in cp.ALL.values():
        h = cp.lags(m)
        assert len(h) == len(set(h)) and h[0] == 0.0 and 1e-160 in h and 1e-9 in h and 75 <= len(h) <= 130, m.name
        with np.errstate(divide="ignore"):
            arg = cp.shape_arg(_single(m), 1, False, np.asarray(h)[:, None])
        assert arg[1:].min() < 1e-9 and arg.max() >= 1e4 * (1.0 - 1e-12), m.name
        if m.kind != "power":
            for a in (690.0, 708.4, 745.2, 800.0):      # the exponentials go denormal, then to zero
                assert np.min(np.abs(arg / a - 1.0)) < 1e-12, (m.name, a)
    for m, dim, ball in _runs():
        pts = cp.points(m, dim, ball)
        assert len({tuple(p) for p in pts}) + len(cp.directions(dim)) - 1 == len(pts), (m.name, dim, ball)   # the origin
        assert np.sum(np.all(pts == 0.0, axis=1)) == len(cp.directions(dim))
        assert len(pts) >= len(cp.directions(dim)) * len(cp.lags(m))


@pytest.fixture(scope="module")
def measured():
    return tool.measure()


def test_oracle_figures_are_the_committed_ones(measured):
    assert set(measured) == set(cp.ORACLE) == {bc for cls in cp.CLASSES for bc in cp.bar_classes(cls)}
    for cls, res in tool.rounded(measured).items():
        want = cp.ORACLE[cls]
        assert set(res) == set(want), cls
        for key, v in res.items():
            if key == "cases":
                continue
            for what, e in (v.items() if isinstance(v, dict) else [(None, v)]):
                w = want[key][what] if what else want[key]
                assert abs(e - w) <= 0.05 * w + 0.01, (cls, key, what, e, w)


def test_every_case_is_kept(measured):
    total = 0
    for cls in cp.CLASSES:
        n = sum(len(cp.points(m, dim, ball)) for m in cp.by_class(cls) for dim, ball, nugget in tool.configurations(m))
        assert sum(measured[bc]["cases"] for bc in cp.bar_classes(cls)) == n, cls
        for bc in cp.bar_classes(cls):
            assert measured[bc]["cases"] == cp.ORACLE[bc]["cases"] > 0, bc
        total += n
    assert total > 50000


def test_bars_follow_the_rule():
    assert {bc for bc in cp.ORACLE if "F" in cp.ORACLE[bc]} == {"exp", "compact", "general", "general_tiny"}
    for cls in cp.ORACLE:
        for route in cp.ROUTES + ("F",):
            if route not in cp.ORACLE[cls]:
                assert cls == "power" or route == "F"
                continue
            for what in ("mean", "var") if route != "A" else ("mean",):
                b = cp.bar(cls, route, what)
                two = 2.0 if what == "var" else 1.0
                assert b >= 8.0 * two
                base = cls[:-5] if cls.endswith("_tiny") else cls
                if base in cp.ZOO_BOUND:
                    assert b * cp.UNIT <= two * cp.ZOO_BOUND[base] * (1.0 + 1e-12)
    # the lags below the ladder do not set the bar of the switches
    assert cp.bar("general", "A") < cp.bar("general_tiny", "A")
    m = cp.ALL["matern_0.7"]
    t = cp.tiny(m, 1, False)
    a = cp.shape_arg(m, 1, False, cp.points(m, 1))
    assert t.sum() >= 2 and np.all(a[t] < 1e-9) and np.all((a[~t] >= 1e-9) | (a[~t] == 0.0))
    assert not cp.tiny(cp.ALL["matern_1.0"], 1, False).any()


def test_one_sample_simple_kriging_mean_is_the_covariance():
    from oracle import kriging as K
    from oracle.variogram import cov_pairwise
    for m, dim, ball in _runs():
        if m.kind == "power":
            continue
        for nugget in cp.NUGGETS:
            vg = cp.oracle_model(m, dim, ball, nugget)
            pts, o = cp.points(m, dim, ball), cp.origin(dim)
            c = cov_pairwise(vg, o, pts)[0]
            mu, var = K.exactsolve(K.SK, vg, o, np.ones(1), pts, mean=0.0)
            lmu, lvar, st = K.approxsolve(K.SK, vg, o, np.ones(1), pts, 1, mean=0.0)
            assert not st.any()
            assert np.max(np.abs(mu - c / cp.SILL)) <= 2.0 * cp.UNIT and np.max(np.abs(lmu - c / cp.SILL)) <= 2.0 * cp.UNIT
            zero = np.all(pts == 0.0, axis=1)
            assert np.all(mu[zero] == 1.0) and np.all(var[zero] == 0.0)


def test_reference_agrees_with_the_kernel_matrix():
    shared = {"gaussian": "gaussian", "exponential": "exponential", "spherical": "spherical", "matern12": "matern12",
              "matern32": "matern32", "matern52": "matern52", "cubic": "cubic", "pentaspherical": "pentaspherical"}
    for name, kname in shared.items():
        m = cp.ALL[name]
        for dim, ball in ((1, False), (2, True), (3, False), (3, True)):
            if ball and name not in cp.BALL_MODELS:
                continue
            p = km.build(kname, dim, 7, ball=ball)
            o = cp.origin(dim)[0]
            for pt in cp.points(m, dim, ball)[::7]:
                a = cp.reference(m, o, pt, dim, ball, 0.25)
                b = km.cov_mp(p, o, pt)
                if np.all(pt == 0.0):
                    assert a == cp.SILL and b == km.SILL
                    continue
                a = a / (mp.mpf(cp.SILL) - mp.mpf(cp.eff_nugget(m, 0.25)))
                b = b / (mp.mpf(p.sill) - mp.mpf(p.eff_nugget))
                assert abs(a - b) <= mp.mpf(10) ** -40 * max(abs(b), mp.mpf(10) ** -300), (name, dim, ball, pt)
