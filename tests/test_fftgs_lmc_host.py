"""Co-simulation under a linear model of coregionalisation (gss.h, gss_fftgs_create_lmc), what needs no device: the
factor rule as tests/fftgs_lmc_ref.py restates it, the library's argument checks, and the twin's front end."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import fftgs_lmc_ref as R
from oracle_engine import OracleEngine

EPS = 2.0 ** -52


def _rand_psd(n, rank, seed):
    A = np.random.default_rng(seed).normal(size=(n, rank))
    return A @ A.T


_v = np.array([1.0, -0.5, 2.0])
_u = np.array([1.0, 0.0, 3.0])
_w = np.array([0.0, 2.0, 1.0])
# rank 2 with the zero column in the middle: row / column 1 is a multiple of row / column 0, so the second pivot vanishes
# and the third does not
_MID = np.outer([1.0, 2.0, 0.5], [1.0, 2.0, 0.5]) + np.outer([0.0, 0.0, 1.5], [0.0, 0.0, 1.5])
FACTOR_CASES = {
    "full-rank 3x3": (_rand_psd(3, 3, 1) + 0.1 * np.eye(3), [0, 1, 2]),
    "rank-1 3x3": (np.outer(_v, _v), [0]),
    "rank-2, zero column in the middle": (_MID, [0, 2]),
    "zero matrix": (np.zeros((3, 3)), []),
    "8x8": (_rand_psd(8, 8, 2) + 0.05 * np.eye(8), list(range(8))),
}


@pytest.mark.parametrize("name", list(FACTOR_CASES))
def test_factor_rule_reproduces_the_matrix(name):
    B, live = FACTOR_CASES[name]
    L, got = R.factor(B)
    n = B.shape[0]
    assert got == live
    assert np.all(np.triu(L, 1) == 0.0)
    for j in range(n):
        if j not in live:
            assert np.all(L[:, j] == 0.0)
    err = np.max(np.abs(L @ L.T - 0.5 * (B + B.T)))
    print(name, "max |L L^T - B| =", err, "bound", n * EPS * np.max(np.abs(B)))
    assert err <= n * EPS * np.max(np.abs(B))


def test_factor_rule_refuses_what_is_not_positive_semidefinite():
    with pytest.raises(R.NotPSD, match=r"\[1\]\[1\]"):
        R.factor(np.array([[1.0, 2.0], [2.0, 1.0]]))              # indefinite: second pivot 1 - 4
    with pytest.raises(R.NotPSD, match=r"\[0\]\[0\]"):
        R.factor(np.array([[-1.0, 0.0], [0.0, 2.0]]))             # negative diagonal
    with pytest.raises(R.NotPSD, match=r"\[1\]\[0\]"):
        R.factor(np.array([[0.0, 1.0], [1.0, 1.0]]))              # zero pivot beside a non-zero column


# ---- the library's argument checks (no device: they come before the first HIP call) ---------------------------------------
def _create(nz, b0, b1, means, kind="exponential", dims=(8, 8), vg=None):
    from gss import _lib
    lib = _lib.load()
    h = C.c_void_p()
    v = vg if vg is not None else _lib.make_variogram(kind, len(dims), range=3.0)
    d = (C.c_int64 * 3)(*(list(dims) + [1] * (3 - len(dims))))
    arr = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (b0, b1, means)]
    code = lib.gss_fftgs_create_lmc(C.byref(h), C.byref(v), nz, _lib.ptr(arr[0]), _lib.ptr(arr[1]), _lib.ptr(arr[2]),
                                    len(dims), d, None, 0, None)
    assert not h.value
    return code, _lib.last_error()


def test_invalid_arguments_do_not_need_a_device():
    from gss import _lib
    I2, Z2, m2 = np.eye(2), np.zeros((2, 2)), np.zeros(2)
    for nz in (0, 9):
        code, msg = _create(nz, np.eye(9), np.eye(9), np.zeros(9))
        assert code == _lib.ERR_INVALID and f"nz = {nz}" in msg
    code, msg = _create(2, Z2, np.array([[1.0, 0.5], [0.4, 1.0]]), m2)
    assert code == _lib.ERR_INVALID and "b1 is not symmetric at [0][1]" in msg
    code, msg = _create(2, np.array([[1.0, 2.0], [2.0, 1.0]]), I2, m2)
    assert code == _lib.ERR_INVALID and "b0 is not positive semidefinite" in msg and "[1][1]" in msg
    code, msg = _create(2, Z2, np.array([[0.0, 0.0], [0.0, -1.0]]) + 0.0, m2)
    assert code == _lib.ERR_INVALID and "variable 0 has no positive sill" in msg
    code, msg = _create(2, np.array([[3.0, 0.0], [0.0, 3.0]]), np.array([[1.0, 0.0], [0.0, -1.0]]), m2)
    assert code == _lib.ERR_INVALID and "b1 is not positive semidefinite" in msg and "[1][1]" in msg
    code, msg = _create(2, Z2, I2, m2, kind="power")
    assert code == _lib.ERR_UNSUPPORTED and "power" in msg
    nested = _lib.make_variogram("exponential", 2, range=3.0, extras=[("spherical", 0.5, 2.0, 1.0, None)])
    code, msg = _create(2, Z2, I2, m2, vg=nested)
    assert code == _lib.ERR_INVALID and "nextra = 1" in msg
    for args, word in (((None, I2, m2), "b0 or b1"), ((Z2, None, m2), "b0 or b1"), ((Z2, I2, None), "means")):
        code, msg = _create(2, *args)
        assert code == _lib.ERR_INVALID and word in msg and "NULL" in msg
    code, msg = _create(2, Z2, np.array([[1.0, np.nan], [np.nan, 1.0]]), m2)
    assert code == _lib.ERR_INVALID and "[0][1] is not finite" in msg
    lib = _lib.load()
    assert lib.gss_fftgs_realize_lmc(None, 1, 0, 1, None, None, None, 0, None, 0, None) == _lib.ERR_INVALID
    assert "gss_fftgs_realize_lmc" in _lib.last_error()


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def _model(kind="exponential"):
    B1 = np.array([[2.0, 0.6, 0.1], [0.6, 1.0, 0.2], [0.1, 0.2, 0.5]])
    B0 = np.diag([0.3, 0.2, 0.1])
    return SimpleNamespace(names=("cu", "zn", "pb"), kind=kind, range=4.0, order=1.0, B0=B0, B1=B1)


def test_twin_matches_the_model_to_the_group_by_name():
    import gss
    m = _model()
    s = gss.FFTGS((("pb", "cu"), dict(model=m)), engine=OracleEngine)
    q = s._joint[("pb", "cu")]
    assert np.array_equal(q["B1"], m.B1[np.ix_([2, 0], [2, 0])]) and np.array_equal(q["B0"], m.B0[np.ix_([2, 0], [2, 0])])
    assert q["structure"].kind == "exponential" and q["structure"].sill == 1.0 and q["structure"].range == 4.0
    p = gss.SimulationProblem(gss.CartesianGrid(8, 8), {"cu": float, "zn": float, "pb": float}, 1)
    assert s.covariables(p) == [("pb", "cu"), ("zn",)]
    g = gss.FFTGS((("cu", "zn"), dict(model=_model("gaussian"))), engine=OracleEngine)._joint[("cu", "zn")]
    assert np.array_equal(g["B0"], m.B0[:2, :2] + 1e-6 * np.eye(2))      # the Gaussian rule of CoKrigingSolver


def test_twin_refuses_what_it_cannot_simulate():
    import gss
    m = _model()
    with pytest.raises(ValueError, match="model"):
        gss.FFTGS((("cu", "zn"), dict(model=None)))
    with pytest.raises(ValueError, match="model"):
        gss.FFTGS((("cu", "zn"), {}))
    with pytest.raises(ValueError, match="invalid joint parameters"):
        gss.FFTGS((("cu", "zn"), dict(model=m, correlation=0.5)))
    with pytest.raises(ValueError, match="not in the coregionalisation model"):
        gss.FFTGS((("cu", "ag"), dict(model=m)))
    with pytest.raises(ValueError, match="no `variogram` of their own"):
        gss.FFTGS(("cu", dict(variogram=gss.ExponentialVariogram(range=2.0))), (("cu", "zn"), dict(model=m)))
    bad = _model()
    bad.B1 = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="B1 is not positive semidefinite"):
        gss.FFTGS((("cu", "zn"), dict(model=bad)))
    bad = _model()
    bad.B0 = np.diag([0.3, -0.2, 0.1])
    with pytest.raises(ValueError, match="B0 is not positive semidefinite"):
        gss.FFTGS((("cu", "zn"), dict(model=bad)))
    # means are per-variable parameters and are accepted
    gss.FFTGS(("cu", dict(mean=2.0)), (("cu", "zn"), dict(model=m)))
    # conditioning: refused before any handle is made (the stand-in engine has no co-simulation at all)
    grid = gss.CartesianGrid(8, 8)
    data = gss.georef({"cu": [1.0, 2.0]}, [(1.0, 1.0), (5.0, 5.0)])
    with pytest.raises(NotImplementedError, match="batched value columns"):
        gss.FFTGS((("cu", "zn"), dict(model=m)), engine=OracleEngine).preprocess(
            gss.SimulationProblem(data, grid, {"cu": float, "zn": float}, 1))
    with pytest.raises(ValueError, match="only partly"):
        gss.FFTGS((("cu", "zn"), dict(model=m)), engine=OracleEngine).preprocess(
            gss.SimulationProblem(grid, {"cu": float, "w": float}, 1))


def test_single_variable_groups_preprocess_as_before():
    import gss
    grid = gss.CartesianGrid(12, 10)
    vg = gss.ExponentialVariogram(range=3.0)
    p = gss.SimulationProblem(grid, {"z": float, "w": float}, 2)
    s = gss.FFTGS(("z", dict(variogram=vg, mean=1.0)), rng=3, engine=OracleEngine)
    pre = s.preprocess(p)
    assert list(pre) == ["z", "w", "_run"]
    assert set(pre["z"]) == {"cent", "cdev", "vg", "mean", "handle", "zbar", "krig", "dinds"}
    assert list(pre["_run"]["next"]) == [("z",), ("w",)]
    sol = gss.solve(p, gss.FFTGS(("z", dict(variogram=vg, mean=1.0)), rng=3, engine=OracleEngine))
    ref = OracleEngine.FFTGS(vg, grid.dims, grid.spacing, 1.0).realize(3, 0, 2)
    assert np.array_equal(np.stack(sol["z"]), ref)
