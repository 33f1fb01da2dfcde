"""Cross-validation of cokriging without a device: the declaration, export and binding of gss_cokrig_cv_knn, the numpy
reference against a refit per fold, the conditioning cap of every case, the outcomes the short-list cases claim, the
twin's location folds and refusals (on a stand-in engine that answers from the reference), and the compiled
instantiations of cokrig_cv_kernel against the case table and against the registers of cokrig_local_kernel."""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cokrig_cases as CC
import cokrig_cv_cases as VC
import cokrig_cv_ref as VR
import cokrig_local_ref as LR
import cokrig_ref as CR

import gss
from gss import _lib
from gss.validation import location_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _ref(c, **kw):
    return VR.predict(LR.Model(c["structure"], c["B0"], c["B1"]), c["x"], c["z"], c["var"], c["k"], c["fold"],
                      c["exclude_radius"], c["variant"], c["means"], **c["search"], **kw)


def test_header_declares_library_exports_and_binding_covers_the_call():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gss.h")).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+gss_cokrig_cv_knn\s*\(", src)
    assert hasattr(_lib.load(), "gss_cokrig_cv_knn")
    assert len(_lib.SIGNATURES["gss_cokrig_cv_knn"]) == 16


# ---- the condition the tolerance rests on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(VC.CASES))
def test_conditioning_cap(name):
    c = VC.CASES[name]()
    assert abs(np.max(np.diag(c["B0"]) + np.diag(c["B1"])) - 1.0) < 1e-15
    worst = _ref(c, with_cond=True)[5]
    print(name, "largest cond_2 over the samples = %.3g" % worst)
    assert worst <= CC.COND_CAP


# ---- the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["global_ok", "global_sk"])
def test_reference_with_every_sample_is_a_refit_per_fold(name):
    c = VC.CASES[name]()
    pred, var, st, idx, cnt = _ref(c)
    assert not st.any()
    model = CR.Model(c["structure"], c["B0"], c["B1"])
    for f in np.unique(c["fold"]):
        inside = c["fold"] == f
        gmu, gvar = CR.predict(model, c["x"][~inside], c["z"][~inside], c["var"][~inside], c["x"][inside], c["variant"],
                               c["means"])
        rows, t = np.flatnonzero(inside), c["var"][inside]
        assert np.max(np.abs(pred[rows] - gmu[t, np.arange(rows.size)])) < 1e-10
        assert np.max(np.abs(var[rows] - gvar[t, np.arange(rows.size)])) < 1e-10
        for p in rows:                                          # every sample outside the fold, variable by variable
            assert sorted(idx[p][idx[p] >= 0]) == list(np.flatnonzero(~inside))


def test_reference_leaves_out_the_fold_the_ball_and_itself():
    x = np.array([[0.0], [1.0], [2.0], [3.0], [0.0], [5.0]])
    var = np.array([0, 0, 0, 0, 1, 1])
    idx, cnt = VR.select(x, var, (2, 2))                         # every sample its own fold: the collocated partner stays
    assert idx[0].tolist() == [1, 2, 4, 5] and idx[4].tolist() == [0, 1, 5, -1]
    idx, cnt = VR.select(x, var, (2, 2), fold=[0, 1, 2, 3, 0, 4])   # one id per location: it leaves with the query
    assert idx[0].tolist() == [1, 2, 5, -1] and cnt[0].tolist() == [2, 1]
    idx, cnt = VR.select(x, var, (2, 2), exclude_radius=1.0)     # exactly on the radius: left out
    assert idx[0].tolist() == [2, 3, 5, -1] and idx[1].tolist() == [3, -1, 5, -1]


def test_ball_on_radius_case_has_its_neighbours_exactly_on_the_radius():
    c = VC.CASES["ball_on_radius"]()
    key, _ = LR.search_keys(c["x"], c["x"])
    assert np.all(key == np.round(key)) and np.all((key == 100.0).sum(axis=1) >= 2)
    idx = _ref(c)[3]
    for p in range(idx.shape[0]):
        assert np.all(key[p, idx[p][idx[p] >= 0]] > 100.0)


def test_short_lists_cases_hit_all_four_outcomes():
    c, cs = VC.CASES["short_ok"](), VC.CASES["short_sk"]()
    _, _, st, _, cnt = _ref(c)
    sts = _ref(cs)[2]
    v, K = c["var"], cnt.sum(axis=1)
    assert np.all(c["fold"][v == 1] == 0)                        # one fold holds every sample of variable 1
    assert np.all(cnt[v == 1, 1] == 0) and np.all(st[v == 1] == VR.MISSING)
    own_absent = (v == 1) & (K >= 2)
    assert own_absent.any() and np.all(sts[own_absent] == VR.OK_)   # the simple variant estimates them
    few = K < 2
    assert few.any() and np.all(st[few] == VR.MISSING) and np.all(sts[few] == VR.MISSING)
    dropped = (v == 0) & (cnt[:, 1] == 0) & (K >= 2)
    assert dropped.any() and np.all(st[dropped] == VR.OK_)
    assert np.any((v == 0) & np.all(cnt == 3, axis=1) & (st == VR.OK_))


def test_no_two_keys_tie_inside_a_variable_except_on_the_integer_lattice():
    for name in sorted(VC.CASES):
        if name == "ball_on_radius":                            # exact integer keys: ties are broken by row on both sides
            continue
        c = VC.CASES[name]()
        s = c["search"]
        key, _ = LR.search_keys(c["x"], c["x"], s["radius"], s["radii"], s["rotation"], c["x"][0])
        for a in range(len(c["k"])):
            ks = np.sort(key[:, c["var"] == a], axis=1)
            d = np.diff(ks, axis=1)
            tied = d <= 1e-9 * (1.0 + ks[:, 1:])
            # a zero key against a collocated duplicate is the only tie allowed: the sample itself, never eligible
            assert not np.any(tied & (ks[:, 1:] > 0.0)), (name, a)


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def test_location_ids_put_collocated_samples_in_one_fold_and_nothing_else():
    loc = CC.lattice((6, 5), 10.0, 400)
    x = np.concatenate([loc, loc[:12][::-1], loc[20:25]])
    ids, uniq = location_ids(x)
    assert ids.dtype == np.int32 and uniq.shape == (30, 2) and ids.max() == 29
    assert np.array_equal(uniq[ids], x)
    for i in range(x.shape[0]):
        assert np.array_equal(ids == ids[i], np.all(x == x[i], axis=1))
    nudged = x.copy()
    nudged[30, 0] = np.nextafter(nudged[30, 0], np.inf)          # exact equality: one ulp away is another location
    assert location_ids(nudged)[0].max() == 30


class _Handle:
    """Answers cv_knn / cv_global_folds from the reference."""

    def __init__(self, structure, B0, B1, variant, x, z, var, means=None, factor=True):
        self.model = LR.Model(dict(kind=structure.kind, range=structure.range), B0, B1)
        self.args = (x, z, var)
        self.variant, self.means, self.factor = {0: "simple", 1: "ordinary"}[variant], means, factor
        self.calls = []

    def cv_knn(self, k, fold=None, exclude_radius=None, minneighbors=1, radius=None, radii=None, rotation=None):
        assert not self.factor
        self.calls.append(("knn", tuple(k), fold.copy()))
        return VR.predict(self.model, *self.args, k, fold, exclude_radius, self.variant, self.means, minneighbors,
                          radius, radii, rotation)[:3]

    def cv_global_folds(self, fold):
        assert self.factor
        self.calls.append(("global", None, fold.copy()))
        counts = [int((self.args[2] == a).sum()) for a in range(self.model.nz)]
        return VR.predict(self.model, *self.args, counts, fold, None, self.variant, self.means)[:3]

    def close(self):
        pass


class _Engine:
    handles = []

    @classmethod
    def cokrig(cls, *a, **kw):
        cls.handles.append(_Handle(*a, **kw))
        return cls.handles[-1]

    @staticmethod
    def cv_summary(z, pred, var, status, fold, nfolds):
        assert fold.min() == 0 and fold.max() == nfolds - 1 and np.unique(fold).size == nfolds
        ok = status == 0
        fm = np.array([np.mean((z - pred)[ok & (fold == f)] ** 2) for f in range(nfolds)])
        return dict(n_ok=float(ok.sum()), mse=float(np.mean((z - pred)[ok] ** 2)), cverror=float(np.mean(fm))), fm


def _problem():
    rng = np.random.default_rng(410)
    loc = CC.lattice((8, 7), 10.0, 411)
    cu = CC.values(loc, np.zeros(56, dtype=int), 412)
    zn = CC.values(loc, np.ones(56, dtype=int), 413)
    cu[rng.permutation(56)[:30]] = np.nan
    zn[::9] = np.nan
    data = gss.georef(dict(cu=cu, zn=zn), loc)
    lmc = gss.LMCModel(("cu", "zn"), "exponential", 25.0, 1.0, np.array([[0.1, 0.03], [0.03, 0.08]]),
                       np.array([[0.9, 0.5], [0.5, 0.7]]), 0.0)
    return data, lmc, gss.EstimationProblem(data, gss.PointSet(loc[:2] + 1.0), ("cu", "zn"))


@pytest.mark.parametrize("nmax", [(5, 7), None])
def test_cross_validate_takes_a_cokriging_solver_and_folds_the_locations(nmax):
    data, lmc, problem = _problem()
    solver = gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, maxneighbors=nmax)))
    _Engine.handles = []
    res = gss.cross_validate(problem, solver, gss.KFoldValidation(4, rng=5), engine=_Engine)
    assert sorted(res) == ["cu", "zn"]
    (h,) = _Engine.handles
    ((route, k, fold),) = h.calls
    assert (route, k) == (("knn", (5, 7)) if nmax else ("global", None))
    x, var = h.args[0], h.args[2]
    for i in range(x.shape[0]):                                  # collocated samples share their fold
        assert np.all(fold[np.all(x == x[i], axis=1)] == fold[i])
    assert set(fold) == {0, 1, 2, 3}
    for a, v in enumerate(("cu", "zn")):
        r = res[v]
        assert np.array_equal(r.indices, np.flatnonzero(~np.isnan(data[v])))
        assert np.array_equal(r.z, np.asarray(data[v])[r.indices]) and r.pred.shape == r.z.shape
        assert r.fold.max() == r.summary.fold_mse.size - 1
        assert r.summary.cverror == pytest.approx(VR.fold_mean_mse(r.z, r.pred, r.status, fold[var == a]), rel=1e-12)


def test_leave_one_out_is_one_fold_per_location():
    data, lmc, problem = _problem()
    _Engine.handles = []
    gss.cross_validate(problem, gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, maxneighbors=4))), engine=_Engine)
    x, fold = _Engine.handles[0].args[0], _Engine.handles[0].calls[0][2]
    assert np.array_equal(fold, location_ids(x)[0]) and fold.max() + 1 == np.unique(x, axis=0).shape[0] < x.shape[0]


def test_twin_refusals():
    data, lmc, problem = _problem()
    with pytest.raises(ValueError, match="global neighbourhood"):
        gss.cross_validate(problem, gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc))), gss.LeaveBallOut(5.0),
                           engine=_Engine)
    with pytest.raises(ValueError, match="at most 64"):
        gss.cross_validate(problem, gss.CoKrigingSolver((("cu", "zn"), dict(model=lmc, maxneighbors=(26, 40)))),
                           engine=_Engine)
    with pytest.raises(TypeError, match="KrigingSolver and CoKrigingSolver"):
        gss.cross_validate(problem, gss.IDWSolver())


# ---- the compiled kernels -------------------------------------------------------------------------------------------------
def test_every_compiled_instantiation_has_a_case_and_every_case_a_kernel():
    import kernel_census
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf / c++filt not available")
    compiled = [tuple(int(a) for a in args) for fam, args in kernel_census.census(_lib.LIB_PATH)
                if fam == "cokrig_cv_kernel"]
    assert len(compiled) == len(set(compiled)) == 45
    assert set(compiled) == set(VC.KERNELS)
    for (dim, kind, nt), fn in VC.KERNELS.items():
        c = fn()
        ksum = sum(c["k"])
        assert c["x"].shape[1] == dim and (1 if ksum <= 16 else (2 if ksum <= 32 else 4)) == nt


def _resources(family):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), _lib.LIB_PATH, family],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        m = re.match(r"_ZN3gss\d+%sILi(\d)ELi(n?\d+)ELi(\d)E\S*\s+vgpr\s+(\d+).*sgpr\s+(\d+).*scratch (\d+) spills (\d+)"
                     % family, line)
        assert m, line
        out[(m.group(1), m.group(2), m.group(3))] = tuple(int(m.group(i)) for i in (4, 5, 6))
    return out


def test_one_target_kernel_needs_no_more_registers_or_scratch_than_its_parent():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    cv, local = _resources("cokrig_cv_kernel"), _resources("cokrig_local_kernel")
    assert set(cv) == set(local) and len(cv) == 45
    for key in sorted(cv):
        print(key, "vgpr / sgpr / scratch:", cv[key], "parent", local[key])
        assert all(a <= b for a, b in zip(cv[key], local[key])), key
        if not key[1].startswith("n"):
            assert cv[key][2] == 0, key                          # the compile-time kinds use no scratch
