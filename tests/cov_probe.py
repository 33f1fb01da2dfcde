"""Probe of every covariance form at chosen lags: the tables and the 50-digit reference (no device code).

The solvers take their covariances from a handful of evaluators in csrc/gss_internal.h (vg_shape through cov_pair, the
same with a compile-time kind, vg_shape4 on gss_exp_poly, vg_shape_kpos on gss_exp_poly_neg with per-axis scaled
differences, the Bessel K0 / x K1 expansions and gss_matern_general).  One sample at the origin with z = 1 under simple
kriging with known mean 0 returns mean = C(h) / C(0) and variance C(0) - C(h)^2 / C(0) at a point at lag h: the 1 x 1
system adds nothing but a rounding or two, so each route of tests/test_gpu_cov_probe.py shows one evaluator's value.

The lags are built from the argument the device forms (d of the Matern models, x = lag / range of the compact ones):
the floating-point neighbours of every place where an evaluator changes behaviour, a geometric ladder of the argument
from 1e-9 to 1e4 that runs through the underflow of the exponentials, a zero, a denormal and a tiny lag, and seeded
random lags.  `switch_sides` restates, in float64 and in the device's own order of operations, which side of each switch
a lag falls on; tests/test_cov_probe_host.py holds it to thresholds written out there and to the text of the header.

ORACLE holds what tools/cov_probe_oracle.py prints: the error of the FP64 oracle (and of the float64 transcription of the
Bessel / Temme algorithms) against the 50-digit reference; `bar` derives the error bars of the device from it.
"""
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple

import mpmath as mp
import numpy as np

import kernel_matrix as km          # sets mp.mp.dps = 50; _corr, RANGE, RADII, GAUSSIAN_NUGGET_EPS

SILL = 1.0
NUGGETS = (0.0, 0.25)               # the second set: C(0) = sill differs from the limit cs = 0.75 of C(h)
RANGE = km.RANGE
RADII = km.RADII
UNIT = 2.0 ** -53 * SILL            # errors are counted in these
LADDER_PER_DECADE = 3               # (4 took the references of the host test beyond half a minute)


@dataclass(frozen=True)
class Model:
    name: str
    kind: str                       # of gss / oracle.variogram
    nu: float                       # Matern order, Power exponent
    cls: str                        # class the error bars are kept by
    terms: Optional[Tuple[Tuple[float, "Model"], ...]] = None      # nested: (weight, structure)


def _m(name, kind, cls, nu=1.0):
    return name, Model(name, kind, float(nu), cls)


def _matern(nu, cls, name=None):
    return _m(name or "matern_%r" % float(nu), "matern", cls, nu)


_UP, _DN = math.inf, -math.inf
MODELS = dict([
    _m("gaussian", "gaussian", "exp"), _m("exponential", "exponential", "exp"),
    _matern(0.5, "exp", "matern12"), _matern(1.5, "exp", "matern32"), _matern(2.5, "exp", "matern52"),
    _m("spherical", "spherical", "compact"), _m("cubic", "cubic", "compact"),
    _m("pentaspherical", "pentaspherical", "compact"),
    _m("sinehole", "sinehole", "sinehole"),
    _m("power_0.6", "power", "power", 0.6), _m("power_1.0", "power", "power", 1.0),
    _m("power_1.5", "power", "power", 1.5),
    _matern(1.0, "bessel"), _matern(2.0, "bessel"), _matern(3.0, "bessel"),
] + [_matern(nu, "general") for nu in (0.05, 0.2, 0.45, 0.7, 1.25, 2.6, 4.2, 9.5, 20.0)]
  # a half-integer crossed: n = floor(nu + 1/2) jumps and mu flips from +1/2 to -1/2
  + [_matern(float(np.nextafter(h, s)), "general") for h in (0.5, 1.5, 2.5) for s in (_DN, _UP)]
  # mu inside and outside the 1e-15 guards of pi mu / sin(pi mu) and sinh(e) / e
  + [_matern(1.0 + s * e, "general") for e in (1e-6, 1e-13) for s in (-1.0, 1.0)]
  + [_matern(float(np.nextafter(1.0, s)), "general") for s in (_DN, _UP)]
  # beyond the orders tools/gen_matern_general.py validates (20), up to the front end's own limit (50, common.hip)
  + [_matern(40.0, "high"), _matern(50.0, "high")])
REFUSED_ORDERS = (79.0,)            # beyond the front end's limit: the handle is refused (test_gpu_cov_probe.py)


def _nested(name, *terms):
    return name, Model(name, "nested", 0.0, "nested", tuple((w, MODELS[m]) for w, m in terms))


# vg_shape4's gss_exp_poly branches are only taken by a model the fixed-kind kernels do not serve: a nested one
NESTED = dict([_nested("gaussian+exponential", (0.6, "gaussian"), (0.4, "exponential")),
               _nested("matern32+matern52", (0.5, "matern32"), (0.5, "matern52")),
               _nested("matern12+spherical", (0.7, "matern12"), (0.3, "spherical"))])
ALL = {**MODELS, **NESTED}
CLASSES = ("exp", "compact", "sinehole", "power", "bessel", "general", "high", "nested")
# the models that also run under the MetricBall of unequal radii: the fixed kinds (whose moving-neighbourhood kernels
# scale every axis on their own) and one model of every other class
BALL_MODELS = ("gaussian", "exponential", "matern12", "matern32", "matern52", "spherical", "cubic", "sinehole",
               "matern_1.0", "matern_0.7", "matern_40.0", "gaussian+exponential", "matern12+spherical")
UNIT_KINDS = ("gaussian", "exponential", "spherical", "matern12", "matern32", "matern52")   # vg_shape_kpos<KIND, true>


def by_class(cls):
    return [m for m in ALL.values() if m.cls == cls]


def mscale(m):
    """common.hip device_kind: sqrt(2 nu) * 3, in double."""
    return float(np.sqrt(2.0 * m.nu) * 3.0)


def lengths(dim, ball):
    return np.asarray(RADII[dim] if ball else (RANGE,) * dim, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the argument of the shape as the device forms it, in float64
# ---------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _kpos_scale(m, inv_range):
    if m.kind == "gaussian":
        return 1.7320508075688772 * inv_range
    if m.kind == "exponential":
        return 3.0 * inv_range
    if m.kind == "spherical":
        return inv_range
    return mscale(m) * inv_range


def shape_arg(m, dim, ball, pts, unit=False):
    """What the shape of a single structure is evaluated at, for the lags origin -> pts: d = mscale * (sqrt(d2) *
    inv_range) of the Matern models, 3 x^2 and 3 x of the Gaussian and exponential ones, x = lag / range of the compact
    ones and SineHole, the lag of Power.  d2 is accumulated in dimension order with every product and sum rounded
    (sqdist_nofma); `unit`: the moving-neighbourhood form of the fixed kinds instead, every difference times sca[axis]
    and the squares accumulated by FMA (sqdist_scaled), where the scaled distance is the argument."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, dim)
    inv_range = 1.0 if ball else 1.0 / RANGE
    ir = 1.0 / lengths(dim, True) if ball else np.ones(dim)
    if unit:
        assert m.name in UNIT_KINDS
        sca = ir * _kpos_scale(m, inv_range)
        out = np.empty(pts.shape[0])
        for i, p in enumerate(pts):
            acc = 0.0
            for k in range(dim):
                t = float(p[k] * sca[k])
                acc = _fma(t, t, acc)
            out[i] = acc if m.kind == "gaussian" else math.sqrt(acc)
        return out
    d2 = np.zeros(pts.shape[0])
    for k in range(dim):
        t = pts[:, k] * ir[k] if ball else pts[:, k]
        d2 = d2 + t * t
    if m.kind == "gaussian":
        return 3.0 * (d2 * inv_range * inv_range)
    if m.kind == "power":
        return np.sqrt(d2)          # (the device raises d2 itself to half the exponent)
    x = np.sqrt(d2) * inv_range
    if m.kind == "exponential":
        return 3.0 * x
    if m.kind == "matern":
        return mscale(m) * x
    return x                        # compact models, SineHole


# Where an evaluator changes behaviour: name -> (the models it applies to, "the lag is on the lower side").  The
# comparisons are the device's own (gss_internal.h): `d <= 2.0` takes Temme's series / the P expansions, `d > 700.0`
# returns 0, `nu * log(2.0 / d) + (bound on ln Gamma(nu)) > 690.0` returns 1 - d^2 / (4 (nu - 1)), `x < 1.0` evaluates the polynomial.
GUARD_FROM = 4.2                    # orders from which the overflow guard of K_nu is probed


def _stirling(nu):
    """The device's bound on ln Gamma(nu) in that guard."""
    return (nu - 0.5) * np.log(nu) - nu + 1.01


def switches(m):
    out = {}
    if m.cls in ("general", "high"):
        out["temme_steed"] = lambda d: d <= 2.0
        out["zero"] = lambda d: d <= 700.0
        if m.nu >= GUARD_FROM:
            out["one"] = lambda d, nu=m.nu: nu * np.log(2.0 / d) + _stirling(nu) > 690.0
    elif m.cls == "bessel":
        out["cheb_p_q"] = lambda d: d <= 2.0
        out["zero"] = lambda d: d <= 700.0
    elif m.cls == "compact":
        out["range"] = lambda x: x < 1.0
    return out


def switch_sides(m, dim, ball, pts, unit=False):
    """name -> boolean array over pts: the lag falls on the lower side of that switch."""
    with np.errstate(divide="ignore"):
        a = shape_arg(m, dim, ball, pts, unit)
        return {name: np.asarray(f(a), dtype=bool) for name, f in switches(m).items()}


# ---------------------------------------------------------------------------------------------------------------------
# lags
# ---------------------------------------------------------------------------------------------------------------------
def directions(dim):
    """Unit steps the lags are laid along: every axis and, beyond 1-D, the diagonal."""
    d = [np.eye(dim)[k] for k in range(dim)]
    return d + [np.ones(dim)] if dim > 1 else d


def _ordinal(t):
    return int(np.float64(t).view(np.int64))


def _from_ordinal(i):
    return float(np.int64(i).view(np.float64))


def _flip(lower, t0):
    """The largest t > 0 with lower(t) (monotone: true for small t), by bisection over the doubles about t0."""
    lo, hi = t0 * 0.5, t0 * 2.0
    assert lower(lo) and not lower(hi), (t0, lower(lo), lower(hi))
    a, b = _ordinal(lo), _ordinal(hi)
    while b - a > 1:
        c = (a + b) // 2
        if lower(_from_ordinal(c)):
            a = c
        else:
            b = c
    return _from_ordinal(a)


def _arg_per_unit(m, dim, ball, u, unit):
    """d (or x) is linear in the step t along u for every model that has a switch."""
    return float(shape_arg(m, dim, ball, (1.0 * u)[None, :], unit)[0])


def _switch_value(m, name):
    if name == "one":
        return 2.0 * math.exp(-(690.0 - float(_stirling(m.nu))) / m.nu)
    return {"temme_steed": 2.0, "cheb_p_q": 2.0, "zero": 700.0, "range": 1.0}[name]


def switch_steps(m, dim, ball, u):
    """Steps t along u at the neighbours of every switch: two doubles on each side of the place where the device's
    comparison flips, under the general order of operations and (fixed kinds) under the UNIT one."""
    out = []
    for unit in ((False, True) if m.name in UNIT_KINDS else (False,)):
        for name in switches(m):
            def lower(t, name=name, unit=unit):
                return bool(switch_sides(m, dim, ball, (t * u)[None, :], unit)[name][0])
            t = _flip(lower, _switch_value(m, name) / _arg_per_unit(m, dim, ball, u, unit))
            i = _ordinal(t)
            out += [_from_ordinal(i + j) for j in (-1, 0, 1, 2)]
    return out


def _arg_to_lag(m, a):
    """Lag / range at which the argument of the shape is a (isotropic, in exact arithmetic)."""
    if m.kind == "gaussian":
        return math.sqrt(a / 3.0)
    if m.kind == "exponential":
        return a / 3.0
    if m.kind == "matern":
        return a / mscale(m)
    return a


def lags(m):
    """The lag list of a model (isotropic range RANGE; a nested model: of its first structure): ladder, underflow
    points, zero / denormal / tiny, random, and the neighbours of every switch along a line."""
    if m.terms:
        return lags(m.terms[0][1])
    n = 13 * LADDER_PER_DECADE
    ladder = [10.0 ** (-9.0 + 13.0 * i / n) for i in range(n + 1)] + [690.0, 708.4, 745.2, 800.0]
    scale = 1.0 if m.kind == "power" else RANGE
    out = [0.0, 1e-160, 1e-9]
    out += [_arg_to_lag(m, a) * scale for a in ladder]
    rng = np.random.default_rng(20240521)
    out += [float(v) for v in rng.uniform(0.0, 3.0 * scale, 33)[1:]]
    out += switch_steps(m, 1, False, np.ones(1))
    return _unique(out)


def _unique(v):
    seen, out = set(), []
    for t in v:
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


_POINTS = {}


def points(m, dim, ball=False):
    """(pts [npts x dim], lag [npts]): the lag list laid from the origin along every direction; under a ball the step
    along axis k is the lag times radius_k / RANGE (the same lag / range); the neighbours of the switches are found
    anew along every direction, since the rounding of the scaled difference depends on it."""
    key = (m.name, dim, ball)
    if key not in _POINTS:
        base = lags(m)
        first = m.terms[0][1] if m.terms else m
        L = lengths(dim, ball)
        rows = []
        for u in directions(dim):
            if m.kind == "power":
                s = 1.0
            else:                   # lag / range -> step: along an axis its length, along the diagonal 1 / |u / L|
                s = float(1.0 / np.sqrt(np.sum((u / L) ** 2))) / RANGE
            steps = [t * s for t in base] + (switch_steps(first, dim, ball, u) if (dim > 1 or ball) else [])
            rows += [t * u for t in _unique(steps)]
        pts = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, dim))
        _POINTS[key] = pts
    return _POINTS[key]


def origin(dim):
    return np.zeros((1, dim))


# ---------------------------------------------------------------------------------------------------------------------
# 50-digit reference
# ---------------------------------------------------------------------------------------------------------------------
_CORR = {}


def _corr(m, xr):
    """Correlation of a single structure at lag / range xr > 0 (mpf)."""
    key = (m.name, xr)
    if key in _CORR:
        return _CORR[key]
    if m.kind == "sinehole":
        t = mp.pi * xr
        v = mp.sin(t) / t
    elif m.kind == "matern" and m.nu not in (0.5, 1.5, 2.5):
        nu = mp.mpf(m.nu)
        d = mp.sqrt(2 * nu) * 3 * xr
        v = mp.power(2, 1 - nu) / mp.gamma(nu) * mp.power(d, nu) * mp.besselk(nu, d)
    else:
        v = km._corr({"matern12": "matern12", "matern32": "matern32", "matern52": "matern52"}.get(m.name, m.kind), xr)
    _CORR[key] = v
    return v


def power_sill(m, dim):
    """The pseudo-sill A of gss.h (GSS_VG_POWER): 2 gamma(largest lag probed), as the front end chooses it from the
    extent of the data."""
    h = float(np.max(np.sqrt(np.sum(points(m, dim) ** 2, axis=1))))
    return 2.0 * h ** m.nu


def sill_of(m, dim):
    return power_sill(m, dim) if m.kind == "power" else SILL


def device_sill(m, dim, nugget):
    """The total sill the library is handed.  Single structure: SILL (Power: power_sill) as given.  Nested: the front end
    passes the contributions w_i (sill_i - nugget_i) and the nugget, and the library adds them up in float64, in the
    order of the structures (gss.engine._vg_struct, make_vgdev): within a rounding of SILL, and what a zero lag returns."""
    if not m.terms:
        return sill_of(m, dim)
    nug = sum(w * eff_nugget(t, nugget) for w, t in m.terms)
    w0, t0 = m.terms[0]
    s = w0 * (SILL - eff_nugget(t0, nugget)) + nug
    for w, t in m.terms[1:]:
        s += w * (SILL - eff_nugget(t, nugget))
    return s


def eff_nugget(m, nugget, raw=False):
    """The nugget the evaluation of a single structure uses (gss.variograms: a Gaussian one takes nugget + 1e-6);
    `raw`: as given (the cokriging handle of route F reads only the shape of its structure)."""
    return nugget + (km.GAUSSIAN_NUGGET_EPS if m.kind == "gaussian" and not raw else 0.0)


def reference(m, a, b, dim, ball=False, nugget=0.0, raw=False):
    """C(a, b) at 50 digits from the float64 coordinates as given: the difference, the scaling by the lengths and the
    square root are taken in mpmath.  Sill SILL (Power: power_sill) at a zero lag."""
    L = lengths(dim, ball)
    s = mp.mpf(0)
    for k in range(dim):
        t = mp.mpf(float(a[k])) - mp.mpf(float(b[k]))
        if m.kind != "power":
            t = t / mp.mpf(float(L[k]))
        s += t * t
    sill = mp.mpf(sill_of(m, dim))
    if s == 0:
        return sill
    xr = mp.sqrt(s)
    if m.kind == "power":           # A - gamma(h), gamma = scaling h^exponent + nugget with scaling 1
        return sill - mp.mpf(nugget) - mp.power(xr, mp.mpf(m.nu))
    if m.terms:                     # every structure has sill SILL and the model's nugget; the weights sum to 1
        return sum(mp.mpf(w) * (sill - mp.mpf(eff_nugget(t, nugget))) * _corr(t, xr) for w, t in m.terms)
    return (sill - mp.mpf(eff_nugget(m, nugget, raw))) * _corr(m, xr)


_REF = {}


def reference_set(m, dim, ball=False, nugget=0.0, raw=False):
    """(cov, mean, var) over points(m, dim, ball), float64 rounded from 50 digits: C(origin, pt), and the simple-kriging
    answer of one sample z = 1 at the origin under known mean 0: C / C(0) and C(0) - C^2 / C(0)."""
    key = (m.name, dim, ball, nugget, raw and m.kind == "gaussian")
    if key not in _REF:
        o = origin(dim)[0]
        c = [reference(m, o, p, dim, ball, nugget, raw) for p in points(m, dim, ball)]
        s = mp.mpf(sill_of(m, dim))
        _REF[key] = (np.array([float(v) for v in c]), np.array([float(v / s) for v in c]),
                     np.array([float(s - v * v / s) for v in c]))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------
# models of the oracle and of the device
# ---------------------------------------------------------------------------------------------------------------------
def oracle_model(m, dim, ball=False, nugget=0.0, raw=False):
    from oracle.variogram import Nested, Variogram
    radii = RADII[dim] if ball else None
    if m.terms:
        return Nested([(w, Variogram(t.kind, sill=SILL, nugget=nugget, range=RANGE, nu=t.nu, radii=radii))
                       for w, t in m.terms])
    if m.kind == "power":
        return Variogram("power", range=1.0, nu=m.nu, nugget=nugget)
    return Variogram(m.kind, sill=SILL, nugget=nugget, range=RANGE, nu=m.nu, radii=radii, regularize=not raw)


def device_model(m, dim, ball=False, nugget=0.0):
    import gss
    ctor = {"gaussian": gss.GaussianVariogram, "exponential": gss.ExponentialVariogram,
            "spherical": gss.SphericalVariogram, "matern": gss.MaternVariogram, "cubic": gss.CubicVariogram,
            "pentaspherical": gss.PentasphericalVariogram, "sinehole": gss.SineHoleVariogram}

    def one(t, sill, nug):
        kw = {"sill": sill, "nugget": nug}
        if t.kind == "matern":
            kw["order"] = t.nu
        return ctor[t.kind](gss.MetricBall(RADII[dim]), **kw) if ball else ctor[t.kind](range=RANGE, **kw)
    if m.terms:
        out = None
        for w, t in m.terms:
            out = w * one(t, SILL, nugget) if out is None else out + w * one(t, SILL, nugget)
        return out
    return one(m, SILL, nugget)


# ---------------------------------------------------------------------------------------------------------------------
# error bars
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = ("A", "B", "C")
# Route F: the moving-neighbourhood cokriging entry with one variable and one sample (B0 = nugget, B1 = sill - nugget,
# k = (1,)): co_rho1<DIM, KIND> of csrc/cokrig_local_kernel.h, over the fixed kinds and one general model
F_MODELS = UNIT_KINDS + ("matern_0.7",)
# The lags below the ladder (the denormal one, 1e-9 where the scale takes it below, the neighbours of the overflow
# guard) are kept in a sub-class of their own for the general orders: exp(mu ln(d / 2)) and d^nu carry about
# |nu ln d| roundings whatever evaluates them, 185 at the 1e-160 lag, and one such lag would otherwise set the bar of
# every switch of the class.  From the first rung of the ladder on |ln d| <= 21.
TINY = 1e-9


def tiny(m, dim, ball):
    """Boolean over points(m, dim, ball): the lag belongs to the sub-class `<class>_tiny`."""
    pts = points(m, dim, ball)
    if m.cls not in ("general", "high"):
        return np.zeros(len(pts), dtype=bool)
    a = shape_arg(m, dim, ball, pts)
    return (a > 0.0) & (a < TINY)


def bar_classes(cls):
    return (cls, cls + "_tiny") if cls in ("general", "high") else (cls,)


# What tools/cov_probe_oracle.py prints, in units of 2^-53 sill: per class (bar_classes) and route the largest error of
# the FP64 oracle (oracle.variogram for A, oracle.kriging for B, C and F: "cov"/"mean", and "var" of B, C and F) over
# every model of the class, dimension, ball and nugget set; "cases": lags compared per route; "transcription": of the float64 transcription of the device's algorithm.
ORACLE = {
    'exp': {'cases': 11850, 'A': {'cov': 2.0}, 'B': {'cov': 2.0, 'var': 3.48}, 'C': {'cov': 2.0, 'var': 3.48}, 'F': {'cov': 2.0, 'var': 3.48}},
    'compact': {'cases': 6250, 'A': {'cov': 11.59}, 'B': {'cov': 11.59, 'var': 2.0}, 'C': {'cov': 11.59, 'var': 2.0}, 'F': {'cov': 1.4, 'var': 1.28}},
    'sinehole': {'cases': 2370, 'A': {'cov': 2.0}, 'B': {'cov': 2.0, 'var': 2.5}, 'C': {'cov': 2.0, 'var': 2.5}},
    'power': {'cases': 3744, 'A': {'cov': 1.66}},
    'bessel': {'cases': 5414, 'A': {'cov': 5.0}, 'B': {'cov': 5.0, 'var': 9.48}, 'C': {'cov': 5.0, 'var': 9.48}, 'transcription': 2.0},
    'general': {'cases': 29898, 'A': {'cov': 85.5}, 'B': {'cov': 85.5, 'var': 95.99}, 'C': {'cov': 85.5, 'var': 95.99}, 'transcription': 16.0, 'F': {'cov': 29.5, 'var': 20.98}},
    'general_tiny': {'cases': 868, 'A': {'cov': 244.0}, 'B': {'cov': 244.0, 'var': 488.0}, 'C': {'cov': 244.0, 'var': 488.0}, 'transcription': 235.0, 'F': {'cov': 102.0, 'var': 114.0}},
    'high': {'cases': 4170, 'A': {'cov': 281.0}, 'B': {'cov': 281.0, 'var': 562.46}, 'C': {'cov': 281.0, 'var': 562.46}, 'transcription': 26.0},
    'high_tiny': {'cases': 50, 'A': {'cov': 0.0}, 'B': {'cov': 0.0, 'var': 0.0}, 'C': {'cov': 0.0, 'var': 0.0}, 'transcription': 0.0},
    'nested': {'cases': 6004, 'A': {'cov': 2.12}, 'B': {'cov': 2.12, 'var': 3.3}, 'C': {'cov': 2.12, 'var': 3.3}},
}

# absolute bounds tests/test_variogram_zoo.py already holds on cov_pairwise: no bar is looser
ZOO_BOUND = {"sinehole": 1e-13, "bessel": 5e-14, "general": 2e-13, "high": 2e-13}


def bar(cls, route, what="mean"):
    """Largest error allowed to the device, in units: 16 x the oracle's with a floor of 8 (tests/kernel_cases.py); for
    the Bessel and general-order classes at least 2 x the transcription's (the documented accuracy of the algorithm;
    the factor covers the device's log, pow, sin and exp differing from libm); never beyond the bound of
    tests/test_variogram_zoo.py.  Variances (1 - C^2: the error of C enters twice): the same rule on the oracle's
    variance error, with the transcription and the bound doubled."""
    o = ORACLE[cls][route]
    two = 2.0 if what == "var" else 1.0
    b = max(16.0 * o["var" if what == "var" else "cov"], 8.0 * two)
    if "transcription" in ORACLE[cls]:
        b = max(b, two * 2.0 * ORACLE[cls]["transcription"])
    base = cls[:-5] if cls.endswith("_tiny") else cls
    if base in ZOO_BOUND:
        b = min(b, two * ZOO_BOUND[base] / UNIT)
    return b
