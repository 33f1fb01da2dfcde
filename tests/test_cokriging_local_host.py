"""Moving-neighbourhood cokriging without a device: exports and bindings, the refusal the library decides from its
arguments alone, the solver's parameter handling, the numpy reference against the global reference, the conditioning cap
of every case, and the compiled instantiations of cokrig_local_kernel against the case table."""
import ctypes
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cokrig_cases as CC
import cokrig_local_cases as LC
import cokrig_local_ref as LR
import cokrig_ref as CR

import gss
from gss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_header_declares_and_library_exports_both_calls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gss.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("gss_cokrig_create_local", "gss_cokrig_predict_knn"):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name


def test_bindings_cover_both_calls():
    assert len(_lib.SIGNATURES["gss_cokrig_create_local"]) == 12
    assert len(_lib.SIGNATURES["gss_cokrig_predict_knn"]) == 16


def _create_local(nz):
    lib = _lib.load()
    h = ctypes.c_void_p()
    v = _lib.make_variogram("exponential", 2, range=10.0, nu=1.0)
    x = np.ascontiguousarray(np.random.default_rng(0).uniform(0, 50, (2 * nz, 2)))
    z = np.arange(2 * nz, dtype=np.float64)
    var = np.ascontiguousarray(np.tile(np.arange(nz), 2), dtype=np.int32)
    b0 = np.ascontiguousarray(0.1 * np.eye(nz))
    b1 = np.ascontiguousarray(CC.b1_of(nz))
    code = lib.gss_cokrig_create_local(ctypes.byref(h), ctypes.byref(v), nz, _lib.ptr(b0), _lib.ptr(b1), 1, None,
                                       _lib.ptr(x), _lib.ptr(z), _lib.ptr(var), 2 * nz, None)
    assert not h.value
    return code, _lib.last_error()


def test_abi_refuses_five_variables():
    code, msg = _create_local(5)
    assert code == _lib.ERR_UNSUPPORTED and "nz = 5" in msg and "gss_cokrig_create_local" in msg
    code, msg = _create_local(9)
    assert code == _lib.ERR_INVALID and "nz" in msg


# ---- the solver's parameters --------------------------------------------------------------------------------------------
def _lmc(names=("cu", "zn")):
    return gss.LMCModel(tuple(names), "exponential", 20.0, 1.0, 0.1 * np.eye(len(names)), CC.b1_of(len(names)), 0.0)


def _spec(**kw):
    s = gss.CoKrigingSolver((("cu", "zn"), dict(model=_lmc(), **kw)))
    (spec,) = s._spec.values()
    return s, spec


def test_solver_counts_from_an_int_a_sequence_and_a_dict():
    assert _spec()[1]["maxneighbors"] is None
    assert _spec(maxneighbors=12)[1]["maxneighbors"] == [12, 12]
    assert _spec(maxneighbors=(6, 20))[1]["maxneighbors"] == [6, 20]
    assert _spec(maxneighbors=dict(zn=20, cu=6), minneighbors=3)[1]["maxneighbors"] == [6, 20]
    assert _spec(maxneighbors=4, minneighbors=3)[1]["minneighbors"] == 3
    ball = gss.MetricBall((30.0, 10.0))
    assert _spec(maxneighbors=4, neighborhood=ball)[1]["neighborhood"] is ball


def test_solver_refuses_bad_counts():
    with pytest.raises(ValueError, match="pb"):
        _spec(maxneighbors=dict(cu=4, pb=4))
    with pytest.raises(ValueError, match="zn"):
        _spec(maxneighbors=dict(cu=4))
    with pytest.raises(ValueError, match="3 counts"):
        _spec(maxneighbors=(4, 4, 4))
    with pytest.raises(TypeError, match="MetricBall"):
        _spec(maxneighbors=4, neighborhood=5.0)
    names = ("a", "b", "c", "d", "e")
    with pytest.raises(ValueError, match="at most 4"):
        gss.CoKrigingSolver((names, dict(model=_lmc(names), maxneighbors=3)))


def test_solver_clamps_counts_to_each_variable_with_the_warning_of_searcher_ui():
    x = np.random.default_rng(0).uniform(0, 50, (10, 2))
    cu = np.arange(10.0)
    cu[4:] = np.nan                                              # 4 samples of cu, 10 of zn
    data = gss.georef(dict(cu=cu, zn=np.arange(10.0)), x)
    s, _ = _spec(maxneighbors=(6, 8))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pre = s.preprocess(gss.EstimationProblem(data, gss.PointSet(x[:3] + 1.0), ("cu", "zn")))
    (q,) = pre.values()
    assert q["nmax"] == [4, 8]
    assert [str(v.message) for v in w] == ["Invalid maximum number of neighbors. Adjusting to 4..."]
    s, _ = _spec()
    (q,) = s.preprocess(gss.EstimationProblem(data, gss.PointSet(x[:3] + 1.0), ("cu", "zn"))).values()
    assert q["nmax"] is None


# ---- the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["global_ok", "global_sk"])
def test_reference_with_every_sample_is_the_global_reference(name):
    c = LC.CASES[name]()
    model = LR.Model(c["structure"], c["B0"], c["B1"])
    mu, var, st, idx, cnt = LR.predict(model, c["x"], c["z"], c["var"], c["xdom"], c["k"], c["variant"], c["means"])
    gmu, gvar = CR.predict(CR.Model(c["structure"], c["B0"], c["B1"]), c["x"], c["z"], c["var"], c["xdom"], c["variant"],
                           c["means"])
    assert not st.any() and np.all(cnt == np.asarray(c["k"]))
    assert np.max(np.abs(mu - gmu)) < 1e-11 and np.max(np.abs(var - gvar)) < 1e-11
    for p in range(idx.shape[0]):                                # every row once, variable by variable
        assert sorted(idx[p]) == list(range(60)) and np.all(c["var"][idx[p]] == np.repeat([0, 1], c["k"]))


def test_reference_orders_neighbours_by_key_then_row():
    x = np.array([[0.0], [2.0], [-2.0], [1.0], [5.0]])
    idx, cnt = LR.select(x, np.array([0, 0, 0, 1, 1]), np.array([[0.0]]), (3, 2), radius=4.5)
    assert idx.tolist() == [[0, 1, 2, 3, -1]] and cnt.tolist() == [[3, 1]]


def test_short_lists_case_hits_all_four_outcomes():
    c, cs = LC.CASES["short_ok"](), LC.CASES["short_sk"]()
    st, cnt = _ref(c)[2:5:2]
    sts = _ref(cs)[2]
    one_absent = (cnt[:, 0] == 0) & (cnt.sum(axis=1) >= 2)
    assert one_absent.any() and np.all(st[0, one_absent] == LR.MISSING) and np.all(st[1, one_absent] == LR.OK_)
    assert np.all(sts[:, one_absent] == LR.OK_)                 # the simple variant estimates every target there
    few = cnt.sum(axis=1) < 2
    assert few.any() and np.all(st[:, few] == LR.MISSING) and np.all(sts[:, few] == LR.MISSING)
    assert np.any(np.all(cnt == 3, axis=1))
    assert np.any((cnt.min(axis=1) > 0) & (cnt.min(axis=1) < 3))


def _ref(c_or_name):
    c = LC.CASES[c_or_name]() if isinstance(c_or_name, str) else c_or_name
    model = LR.Model(c["structure"], c["B0"], c["B1"])
    return LR.predict(model, c["x"], c["z"], c["var"], c["xdom"], c["k"], c["variant"], c["means"], with_cond=True,
                      **c["search"])


# ---- the condition the tolerance rests on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_conditioning_cap(name):
    c = LC.CASES[name]()
    assert abs(np.max(np.diag(c["B0"]) + np.diag(c["B1"])) - 1.0) < 1e-15
    worst = _ref(c)[5]
    print(name, "largest cond_2 over the points = %.3g" % worst)
    assert worst <= CC.COND_CAP


def test_no_two_keys_tie_inside_a_variable():
    for name in sorted(LC.CASES):
        c = LC.CASES[name]()
        s = c["search"]
        key, _ = LR.search_keys(c["x"], c["xdom"], s["radius"], s["radii"], s["rotation"], c["x"][0])
        for a in range(len(c["k"])):
            ks = np.sort(key[:, c["var"] == a], axis=1)
            assert np.all(np.diff(ks, axis=1) > 1e-9 * (1.0 + ks[:, 1:])), (name, a)


# ---- the compiled kernels -------------------------------------------------------------------------------------------------
def _compiled():
    import kernel_census
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf / c++filt not available")
    return [tuple(int(a) for a in args) for fam, args in kernel_census.census(_lib.LIB_PATH)
            if fam == "cokrig_local_kernel"]


def test_every_compiled_instantiation_has_a_device_case_and_every_case_a_kernel():
    compiled = _compiled()
    assert len(compiled) == len(set(compiled)) == 45
    assert set(compiled) == set(LC.KERNELS)
    kinds = {"gaussian": 0, "exponential": 1, "spherical": 2}
    for (dim, kind, nt), fn in LC.KERNELS.items():              # the case really dispatches to its kernel
        c = fn()
        s = c["structure"]
        got = kinds.get(s["kind"], {0.5: 30, 1.5: 31, 2.5: 32}.get(s.get("nu")) if s["kind"] == "matern" else -1)
        if dim == 1:
            got = -1
        ksum = sum(c["k"])
        assert (c["x"].shape[1], got, 1 if ksum <= 16 else (2 if ksum <= 32 else 4)) == (dim, kind, nt)


def test_compile_time_kinds_use_no_scratch():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), _lib.LIB_PATH,
                        "cokrig_local_kernel"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    seen = 0
    for line in r.stdout.splitlines():
        m = re.match(r"_ZN3gss19cokrig_local_kernelILi(\d)ELi(n?\d+)ELi(\d)E\S*\s+vgpr\s+(\d+).*scratch (\d+) spills (\d+)", line)
        assert m, line
        if not m.group(2).startswith("n"):
            seen += 1
            assert int(m.group(5)) == 0 and int(m.group(6)) == 0, line
    assert seen == 36
