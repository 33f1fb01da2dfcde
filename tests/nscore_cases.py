"""Case table and recorded bars of the normal-score tests (tests/test_nscore_host.py, tests/test_gpu_nscore.py).

Samples are lognormal (the skew the transform exists for), drawn from fixed seeds; the weighted variants carry weights
uniform in [0.5, 2) -- what a declustering step would hand over."""
import numpy as np

EPS = 2.0 ** -52

# ---- fit: the sample sizes of the restatement check --------------------------------------------------------------------
FIT_SIZES = (7, 1000, 200000)
KNOT_BAR_REF = 4.0        # restatement against mpmath, in EPS max(1, |y|)
KNOT_BAR_LIB = 16.0       # library against mpmath: the restatement's own worst (2.66) x 6 for another Phi^-1 and libm
# at 40 digits a knot costs ~0.3 ms: of a large table the check takes the 300 lowest and 300 highest knots (where the
# one-sided form breaks and where |y| is largest) and 400 spread evenly between them
MP_KNOTS = 1000


def sample(n, weighted=False, seed=None):
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    z = np.exp(rng.normal(0.3, 0.9, n))
    w = rng.uniform(0.5, 2.0, n) if weighted else None
    return z, w


# Every knot of every table is also checked in float64 through the residual (Phi(y_k) - p_k) / phi(y_k), the first-order
# error of y_k, with p_k the long-double class probability and Phi = scipy.special.ndtr on the lower-tail side.  Its
# bar, in EPS max(1, |y|): the restatement's own 4, plus what float64 ndtr adds: the rounding of y / sqrt 2 and of the
# constant (each EPS / 2 relative, amplified by y^2 in Phi and divided by the Mills ratio's 1 / |y|: 1 in all), two ulp
# of erfc times the Mills ratio (at most 1.26: 2.5) and the rounding of p_k to float64 (0.6): 8.1, taken as 9.
KNOT_BAR_RESIDUAL = 9.0

# Equal weights that are not exact in binary, with an odd count: the class at the median has the same weight below and
# above, and the long-double sums from either end round differently once a prefix outgrows 64 bits.  (n, weight; None:
# the normalised 1 / n)
EQUAL_WEIGHT_CASES = ((6095, 0.1), (24077, None), (4097, 1.0 / 3.0))


def equal_weight_sample(n, w):
    return np.arange(n, dtype=np.float64) * 0.25 + 1.0, np.full(n, 1.0 / n if w is None else w)


def knot_subset(K):
    if K <= MP_KNOTS:
        return np.arange(K)
    mid = np.linspace(300, K - 301, 400).astype(np.int64)
    return np.unique(np.concatenate([np.arange(300), mid, np.arange(K - 300, K)]))


# ---- tables of the device tests: K distinct values each ---------------------------------------------------------------
TABLE_KNOTS = (1, 2, 3, 64, 1000)
GLOBAL_TABLE_KNOTS = 3000   # above the library's LDS threshold of 1 280: the global-memory variant without an override
LENS = (1, 2, 3, 255, 256, 257, 4099)
INTERP_BAR_INV = 8.0      # EPS max(|v_k|, |v_k+1|)
INTERP_BAR_FWD = 8.0      # EPS max(1, |y|)


def table_sample(K, weighted=False):
    return sample(K, weighted, seed=77 + K)


def crowded_sample():
    """A weighted table one guide cell of which holds several knots: 40 values within 1e-3 of each other, carrying a
    thousandth of the weight of 24 values spread over [1, 50] -- in v they share one of the 128 cells, and in y their
    scores are packed into the gap between two ordinary knots."""
    rng = np.random.default_rng(5)
    z = np.concatenate([np.sort(rng.uniform(1.0, 50.0, 24)), 7.3 + 1e-3 * np.sort(rng.uniform(0, 1, 40))])
    w = np.concatenate([np.ones(24), np.full(40, 1e-3)])
    return z, w


# ---- tails ----------------------------------------------------------------------------------------------------------------
# name -> (zmin factor, zmax factor, (power_lo, power_hi)); zmin = factor x v_1, zmax = factor x v_K, None = defaulted
TAIL_CASES = {
    "clamp": (None, None, (1.0, 1.0)),
    "linear": (0.0, 2.0, (1.0, 1.0)),
    "power_half": (0.0, 2.0, (0.5, 0.5)),
    "power_two": (0.5, 1.5, (2.0, 2.0)),
    "lower_only": (0.0, None, (1.0, 2.0)),
}
TAIL_TABLE_KNOTS = 1000


def tail_inputs(y1, yK):
    """+-(y_K + 1e-12) (and the same beside y_1), +-6, +-12, +-40 (Q underflows: zmin / zmax exactly), +-inf, NaN."""
    return np.array([y1 - 1e-12, yK + 1e-12, -(yK + 1e-12), -6.0, 6.0, -12.0, 12.0, -40.0, 40.0, -np.inf, np.inf, np.nan])


def tail_bounds(name, v):
    lo, hi, power = TAIL_CASES[name]
    return (None if lo is None else lo * v[0], None if hi is None else hi * v[-1], power)


def tail_scale(name, v, x):
    """What the error at each input is measured in units of EPS times: the largest magnitude its tail model handles,
    max(|zmin|, |v_1|) below zero and max(|zmax|, |v_K|) above (the inputs lie on either side of a table around 0)."""
    lo, hi, _ = tail_bounds(name, v)
    s_lo = max(abs(v[0]), abs(v[0] if lo is None else lo))
    s_hi = max(abs(v[-1]), abs(v[-1] if hi is None else hi))
    return np.where(np.asarray(x) < 0.0, s_lo, s_hi)


def tail_error(name, v, x, got, ref):
    """Largest |got - ref| over the inputs in EPS x tail_scale; NaN must meet NaN."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (got, ref)
    return float(np.max((np.abs(got - ref) / (EPS * tail_scale(name, v, x)))[~nan]))


# Largest error of the float64 restatement (tests/nscore_ref.py) against mpmath over tail_inputs, in EPS x tail_scale:
# measured by tests/test_nscore_host.py::test_recorded_tail_error_is_reproduced, which fails when a value here is
# stale.  The device is held to 16 x these.
TAIL_REF_ERR = {
    "clamp": 0.0,
    "linear": 9.72,
    "power_half": 5.15,
    "power_two": 9.72,
    "lower_only": 9.72,
}
TAIL_BAR_FACTOR = 16.0
