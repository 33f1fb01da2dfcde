"""Sequential indicator simulation without a GPU: the reference tests/sis_ref.py alone, with lists and weights from the
CPU's own stage A (the search and numpy.linalg as oracle/sgs.py uses them); CookieCutter on stub solvers; and the refusals
of gss_sis_realize that need no handle.  The first test is what lets tests/test_gpu_sis.py compare every run of
tests/sis_cases.py with `walk` without exclusions: no draw of any run is a close call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ik_ref
import sis_cases as SC
import sis_ref as SR

_cache = {}


def _cpu(name):
    """geometry, stage A of every path the run draws from, and the walked field of a run, once."""
    if name not in _cache:
        run = SC.RUNS[name]
        geo = SR.geometry(run)
        stage = {p: SR.cpu_stage_a(run, geo, geo["paths"][p]) for p, _ in SR.blocks(run)}
        z = np.concatenate(SR.over_blocks(SR.walk, run, geo, stage), axis=0)
        _cache[name] = (run, geo, stage, z)
    return _cache[name]


def test_the_table_covers_what_it_says():
    cont = {r.K for r in SC.RUNS.values() if not r.categorical}
    cat = {r.K for r in SC.RUNS.values() if r.categorical}
    assert cont == {1, 3, 4, 5, 8, 9, 16} and cat == {2, 3, 8, 16}
    assert {r.k for r in SC.RUNS.values()} == {4, 16, 80}
    assert any(r.nd == 0 for r in SC.RUNS.values()) and any(r.nugget_only for r in SC.RUNS.values())
    for name, r in SC.RUNS.items():
        assert int(np.prod(r.dims)) <= SC.MAX_N and r.R <= SC.MAX_R and r.k <= int(np.prod(r.dims)), name
        assert (r.env == SC._WALK) == r.sweep.startswith("walk") and (r.npaths > 1) == r.sweep.endswith("paths"), name
        assert r.npaths == 1 or (r.path_base > 0 and r.first_real >= r.path_base
                                 and r.first_real + r.R <= r.path_base + r.npaths), name
    assert {r.R for r in SC.RUNS.values() if r.npaths == 1} == {67, 130}      # a partial wave; two waves and a part


@pytest.mark.parametrize("name", list(SC.RUNS))
def test_no_draw_of_the_run_is_a_close_call(name):
    run, geo, stage, z = _cpu(name)
    assert sum(SR.over_blocks(SR.close_calls, run, geo, stage)) == 0
    # ... and the restatement satisfies its own one-step check
    assert sum(bad for bad, _ in SR.over_blocks(SR.one_step, run, geo, stage, z)) == 0


@pytest.mark.parametrize("name", list(SC.RUNS))
def test_realisations_honour_data_and_stay_in_range(name):
    run, geo, stage, z = _cpu(name)
    assert z.shape == (run.R, geo["N"]) and np.all(np.isfinite(z))
    assert np.array_equal(z[:, geo["dl"]], np.tile(geo["zd"], (run.R, 1)))
    if run.categorical:
        assert np.all((z == np.floor(z)) & (z >= 0) & (z <= run.K - 1))
    else:
        assert np.all((z >= geo["zmin"]) & (z <= geo["zmax"]))
    if run.nmin > 1:                                  # some nodes are marginal, some are not
        nc = stage[0][1]
        sim = SR.ranks(geo["paths"][0], geo["dl"], geo["N"]) >= 0
        assert np.any(nc[sim] == 0) and np.any(nc[sim] > 0)


def test_nugget_only_draws_are_independent_draws_from_the_proportions():
    name, = [n for n, r in SC.RUNS.items() if r.nugget_only]
    run, geo, stage, z = _cpu(name)
    assert np.all(stage[0][2] == 0.0)                 # every weight is zero
    sim = SR.ranks(geo["paths"][0], geo["dl"], geo["N"]) >= 0
    draws = z[:, sim].ravel()
    for s, p in enumerate(geo["fs"]):
        sd = np.sqrt(p * (1.0 - p) / draws.size)
        assert abs(np.mean(draws == s) - p) <= 5.0 * sd, (s, np.mean(draws == s), p, sd)


def test_order_relations_are_the_doubles_of_the_indicator_kriging_reference():
    rng = np.random.default_rng(5)
    rows = np.concatenate([[[0.4, 0.3, 0.9, 0.8, 1.2, -0.1, 0.95, 1.0]], rng.uniform(-0.2, 1.2, (200, 8))])
    assert np.any(np.diff(rows[0]) < 0)               # the constructed row violates them
    got = SR.correct(rows)
    assert np.array_equal(got, ik_ref.order_relations(rows))
    assert np.all(np.diff(got, axis=1) >= 0) and np.all((got >= 0) & (got <= 1))
    up = np.array([0.4, 0.4, 0.9, 0.9, 1.0, 1.0, 1.0, 1.0])        # of the clipped row .4 .3 .9 .8 1 0 .95 1
    down = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.95, 1.0])
    assert np.array_equal(got[0], (up + down) * 0.5)


# ---- CookieCutter (cookie.jl) on stub solvers ------------------------------------------------------------------------------
class DummySimSolver:
    """A solver that fills every variable it is asked for with a constant (or, as master, with a given pattern)."""

    def __init__(self, *targets, value=0.0, pattern=None):
        self.vparams = {t: {} for t in targets}
        self.value, self.pattern = value, pattern

    def solve(self, problem, **kw):
        import gss
        n = problem.domain.nelements()
        reals = {}
        for v in problem.variables:
            if self.pattern is not None:
                reals[v] = [np.roll(self.pattern(n), i) for i in range(problem.nreals)]
            else:
                reals[v] = [np.full(n, self.value + i) for i in range(problem.nreals)]
        return gss.Ensemble(problem.domain, reals)


def test_cookie_cutter_masks_by_the_master_realisation():
    import gss
    labels = np.array(["sand", "shale", "silt"])
    master = DummySimSolver("f", pattern=lambda n: labels[np.arange(n) % 3])
    solver = gss.CookieCutter(master, {"sand": DummySimSolver(value=10.0), "shale": DummySimSolver(value=20.0)})
    problem = gss.SimulationProblem(gss.CartesianGrid(10, 10), (("f", str), ("z", float), ("y", float)), 3)
    sol = gss.solve(problem, solver)
    assert set(sol.reals) == {"f", "z", "y"} and len(sol["z"]) == 3
    for i in range(3):
        f = sol["f"][i]
        assert f.dtype == labels.dtype and np.array_equal(f, np.roll(labels[np.arange(100) % 3], i))
        for var in ("z", "y"):
            v = sol[var][i]
            assert np.all(v[f == "sand"] == 10.0 + i) and np.all(v[f == "shale"] == 20.0 + i)
            assert np.all(np.isnan(v[f == "silt"]))   # no solver for this value: NaN


def test_cookie_cutter_refusals_and_show():
    import gss
    solver = gss.CookieCutter(DummySimSolver("f"), {0: DummySimSolver(), 1: DummySimSolver()})
    assert repr(solver) == "CookieCutter"
    assert solver.describe() == "CookieCutter\n  └─f ⇨ DummySimSolver\n    └─0 ⇨ DummySimSolver\n    └─1 ⇨ DummySimSolver"
    assert str(solver) == solver.describe()
    grid = gss.CartesianGrid(10, 10)
    with pytest.raises(ValueError, match="one single variable must be specified in master solver"):
        gss.solve(gss.SimulationProblem(grid, (("f", int), ("z", float)), 1),
                  gss.CookieCutter(DummySimSolver("f", "g"), {0: DummySimSolver()}))
    with pytest.raises(ValueError, match="invalid variable in master solver"):
        gss.solve(gss.SimulationProblem(grid, (("g", int), ("z", float)), 1), solver)
    with pytest.raises(ValueError, match="more than one target variable"):
        gss.solve(gss.SimulationProblem(grid, (("f", int),), 1), solver)


def test_sis_solver_parameter_checks_need_no_device():
    import gss
    from oracle_engine import OracleEngine
    grid = gss.CartesianGrid(10, 10)
    g = gss.SphericalVariogram(range=5.0)
    data = gss.georef({"f": np.array(["a", "b", "c"])}, [(1.5, 1.5), (4.5, 7.5), (8.5, 2.5)])
    with pytest.raises(ValueError, match="not among the categories"):
        gss.SISSolver(f=dict(categories=["a", "b"], variogram=g)).preprocess(gss.SimulationProblem(data, grid, "f", 1))
    with pytest.raises(ValueError, match="cutoffs.*or.*categories"):
        gss.SISSolver(f=dict(variogram=g)).preprocess(gss.SimulationProblem(grid, (("f", float),), 1))
    with pytest.raises(ValueError, match="without data the proportions are required"):
        gss.SISSolver(f=dict(categories=[0, 1], variogram=g)).preprocess(gss.SimulationProblem(grid, (("f", int),), 1))
    with pytest.raises(NotImplementedError):          # an engine without the indicator recursion
        gss.SISSolver(f=dict(categories=[0, 1], variogram=g, proportions=[0.5, 0.5]), engine=OracleEngine()).preprocess(
            gss.SimulationProblem(grid, (("f", int),), 1))


# ---- gss_sis_realize: the refusals that need no handle ---------------------------------------------------------------------
def test_refusals_without_a_handle():
    from gss import _lib
    l = _lib.load()
    fs = np.array([0.5, 0.5])
    out = np.zeros(4)
    for kind, word in ((7, "kind 7"), (_lib.SIS_CATEGORICAL, "NULL handle")):
        code = l.gss_sis_realize(None, kind, None, 2, _lib.ptr(fs), 0.0, 0.0, 1.0, 1.0, 1, 0, 1, None, _lib.ptr(out),
                                 _lib.MEM_HOST, None)
        assert code == _lib.ERR_INVALID and word in _lib.last_error(), (code, _lib.last_error())
