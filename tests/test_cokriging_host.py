"""Cokriging without a device: the exports and bindings, the refusals the library decides from its arguments alone,
the front-end's validation, the numpy reference against closed forms, and the conditioning cap that the 1e-9 bar of
tests/test_gpu_cokriging.py rests on."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cokrig_cases as CC
import cokrig_ref as CR

import gss
from gss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- exports and bindings -------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_calls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gss.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("gss_cokrig_create", "gss_cokrig_predict_global"):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name


def test_bindings_cover_both_calls():
    assert len(_lib.SIGNATURES["gss_cokrig_create"]) == 13
    assert len(_lib.SIGNATURES["gss_cokrig_predict_global"]) == 8


# ---- refusals decided from the arguments ------------------------------------------------------------------------------
def _create(nz=2, b0=None, b1=None, variant=1, kind="exponential", var=None, flags=0, means=None):
    lib = _lib.load()
    h = ctypes.c_void_p()
    v = _lib.make_variogram(kind, 2, range=10.0, nu=1.0)
    x = np.ascontiguousarray(np.random.default_rng(0).uniform(0, 50, (6, 2)))
    z = np.arange(6, dtype=np.float64)
    var = np.ascontiguousarray([0, 1, 0, 1, 0, 1] if var is None else var, dtype=np.int32)
    k = max(nz, 1)
    b0 = np.ascontiguousarray(0.1 * np.eye(k) if b0 is None else b0, dtype=np.float64)
    b1 = np.ascontiguousarray(CC.b1_of(k) if b1 is None else b1, dtype=np.float64)
    mm = None if means is None else np.ascontiguousarray(means, dtype=np.float64)
    code = lib.gss_cokrig_create(ctypes.byref(h), ctypes.byref(v), nz, _lib.ptr(b0), _lib.ptr(b1), variant, _lib.ptr(mm),
                                 _lib.ptr(x), _lib.ptr(z), _lib.ptr(var), 6, flags, None)
    assert not h.value
    return code, _lib.last_error()


def test_abi_refuses_nine_variables():
    code, msg = _create(nz=9)
    assert code == _lib.ERR_INVALID and "nz" in msg


def test_abi_refuses_an_asymmetric_b1():
    code, msg = _create(b1=[[1.0, 0.3], [0.3 + 1e-9, 1.0]])
    assert code == _lib.ERR_INVALID and "b1" in msg and "symmetric" in msg and "[0][1]" in msg


def test_abi_refuses_an_id_out_of_range():
    code, msg = _create(var=[0, 1, 0, 2, 0, 1])
    assert code == _lib.ERR_INVALID and "variable id 2 of sample 3" in msg


def test_abi_refuses_the_power_kind():
    code, msg = _create(kind="power")
    assert code == _lib.ERR_UNSUPPORTED and "power" in msg


def test_abi_refuses_drift_variants():
    for variant in (2, 3):
        code, msg = _create(variant=variant)
        assert code == _lib.ERR_UNSUPPORTED and "drift" in msg


def test_abi_refuses_no_factor():
    code, msg = _create(flags=_lib.KRIG_NO_FACTOR)
    assert code == _lib.ERR_INVALID and "GSS_KRIG_NO_FACTOR" in msg


def test_abi_refuses_a_variable_without_samples_and_a_bad_sill():
    code, msg = _create(var=[0, 0, 0, 0, 0, 0])
    assert code == _lib.ERR_INVALID and "variable 1 has no sample" in msg
    code, msg = _create(b0=np.zeros((2, 2)), b1=[[1.0, 0.0], [0.0, 0.0]])
    assert code == _lib.ERR_INVALID and "variable 1" in msg and "sill" in msg
    code, msg = _create(b0=[[0.1, np.nan], [np.nan, 0.1]])
    assert code == _lib.ERR_INVALID and "finite" in msg


# ---- the front-end validates before any device work -------------------------------------------------------------------
def _lmc(names=("cu", "zn"), B1=None, kind="exponential"):
    B1 = np.array([[1.0, 0.5], [0.5, 0.8]]) if B1 is None else np.asarray(B1, dtype=np.float64)
    return gss.LMCModel(tuple(names), kind, 20.0, 1.0, 0.1 * np.eye(len(names)), B1, 0.0)


def test_solver_exists_and_takes_the_joint_spelling():
    s = gss.CoKrigingSolver((("cu", "zn"), dict(model=_lmc(), variant="ordinary")))
    (spec,) = s._spec.values()
    assert spec["B1"].shape == (2, 2) and spec["means"] is None
    # the sub-matrices follow the listed order, not the model's
    s = gss.CoKrigingSolver((("zn", "cu"), dict(model=_lmc(), variant="simple", mean=[1.0, 2.0])))
    (spec,) = s._spec.values()
    assert spec["B1"][0, 0] == 0.8 and spec["B1"][1, 1] == 1.0 and list(spec["means"]) == [1.0, 2.0]


def test_solver_refuses_a_variable_missing_from_the_model():
    with pytest.raises(ValueError, match="pb"):
        gss.CoKrigingSolver((("cu", "pb"), dict(model=_lmc())))


def test_solver_refuses_an_indefinite_b1():
    with pytest.raises(ValueError, match="B1 is not positive semidefinite"):
        gss.CoKrigingSolver((("cu", "zn"), dict(model=_lmc(B1=[[1.0, 1.2], [1.2, 1.0]]))))


def test_solver_refuses_an_unknown_variant():
    with pytest.raises(ValueError, match="universal"):
        gss.CoKrigingSolver((("cu", "zn"), dict(model=_lmc(), variant="universal")))


def test_solver_names_a_variable_without_samples():
    class NoDevice:
        name = "none"

        def cokrig(self, *a, **k):
            raise AssertionError("device work before the validation")

    x = np.random.default_rng(0).uniform(0, 50, (10, 2))
    data = gss.georef(dict(cu=np.arange(10.0), zn=np.full(10, np.nan)), x)
    solver = gss.CoKrigingSolver((("cu", "zn"), dict(model=_lmc())), engine=NoDevice())
    with pytest.raises(AssertionError, match="all samples of zn are missing"):
        gss.solve(gss.EstimationProblem(data, gss.PointSet(x[:3] + 1.0), ("cu", "zn")), solver)


def test_gaussian_rule_touches_the_diagonal_of_b0_only():
    s = gss.CoKrigingSolver((("cu", "zn"), dict(model=_lmc(kind="gaussian"))))
    (spec,) = s._spec.values()
    assert np.allclose(spec["B0"], (0.1 + 1e-6) * np.eye(2), rtol=0, atol=1e-18) and spec["B0"][0, 1] == 0.0
    s = gss.CoKrigingSolver((("cu", "zn"), dict(model=_lmc(kind="gaussian"), regularize=False)))
    (spec,) = s._spec.values()
    assert np.array_equal(spec["B0"], 0.1 * np.eye(2))


# ---- the reference against closed forms ---------------------------------------------------------------------------------
def test_reference_two_samples_in_one_dimension():
    """One sample of each of two variables, simple cokriging of variable 0 at a third point: the 2 x 2 system by hand."""
    b0, b1 = np.array([[0.2, 0.05], [0.05, 0.1]]), np.array([[0.8, 0.4], [0.4, 0.9]])
    m = CR.Model(dict(kind="exponential", range=10.0), b0, b1)
    x, z, var, x0 = np.array([0.0, 4.0]), np.array([1.5, -0.5]), np.array([0, 1]), np.array([1.0])
    r = lambda h: np.exp(-3.0 * h / 10.0)                                        # noqa: E731
    K = np.array([[1.0, 0.4 * r(4.0)], [0.4 * r(4.0), 1.0]])
    c = np.array([0.8 * r(1.0), 0.4 * r(3.0)])
    det = K[0, 0] * K[1, 1] - K[0, 1] ** 2
    lam = np.array([K[1, 1] * c[0] - K[0, 1] * c[1], K[0, 0] * c[1] - K[0, 1] * c[0]]) / det
    mu, var_ = CR.predict(m, x, z, var, x0, "simple", means=[1.0, 0.0])
    assert abs(mu[0, 0] - (1.0 + lam[0] * 0.5 + lam[1] * -0.5)) < 1e-14
    assert abs(var_[0, 0] - (1.0 - lam @ c)) < 1e-14
    # on the sample of variable 1 the cross nugget enters: C_01(0) = b0 + b1
    mu, _ = CR.predict(m, x, z, var, np.array([4.0]), "simple", means=[1.0, 0.0])
    assert abs(mu[1, 0] - (-0.5)) < 1e-14
    c = np.array([0.8 * r(4.0), 0.05 + 0.4])
    lam = np.array([K[1, 1] * c[0] - K[0, 1] * c[1], K[0, 0] * c[1] - K[0, 1] * c[0]]) / det
    assert abs(mu[0, 0] - (1.0 + lam[0] * 0.5 + lam[1] * -0.5)) < 1e-14


def test_reference_intrinsic_model_is_single_variable_kriging():
    c = CC.intrinsic()
    m = CR.Model(c["structure"], c["B0"], c["B1"])
    mu, _ = CR.predict(m, c["x"], c["z"], c["var"], c["xdom"])
    for t in (0, 1):
        own = c["var"] == t
        m1 = CR.Model(c["structure"], c["B0"][t:t + 1, t:t + 1], c["B1"][t:t + 1, t:t + 1])
        mu1, _ = CR.predict(m1, c["x"][own], c["z"][own], np.zeros(own.sum(), dtype=int), c["xdom"])
        assert np.max(np.abs(mu[t] - mu1[0])) < 1e-11


def test_reference_leave_one_out_is_a_refit():
    c = CC.single()
    m = CR.Model(c["structure"], c["B0"], c["B1"])
    pred, _ = CR.cross_validate(m, c["x"], c["z"], c["var"])
    keep = np.arange(50) != 7
    mu, _ = CR.predict(m, c["x"][keep], c["z"][keep], c["var"][keep], c["x"][7:8])
    assert abs(pred[7] - mu[0, 0]) < 1e-13


# ---- the condition the tolerance rests on ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_conditioning_cap(name):
    c = CC.CASES[name]()
    m = CR.Model(c["structure"], c["B0"], c["B1"])
    assert abs(np.max(np.diag(c["B0"]) + np.diag(c["B1"])) - 1.0) < 1e-15
    ev = np.linalg.eigvalsh(c["B1"])
    assert ev[0] >= 0.05 * ev[-1]
    k = CR.cond(m, c["x"], c["var"], c["variant"])
    print(name, "cond_2 = %.3g" % k)
    assert k <= CC.COND_CAP


def test_gaussian_case_reports_its_condition_number():
    c = CC.GAUSSIAN["gaussian"]()
    k = CR.cond(CR.Model(c["structure"], c["B0"], c["B1"]), c["x"], c["var"], c["variant"])
    print("gaussian cond_2 = %.3g" % k)
    assert np.isfinite(k)
