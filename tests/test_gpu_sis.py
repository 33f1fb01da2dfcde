"""Sequential indicator simulation on the device (gss.h, gss_sis_realize): every run of tests/sis_cases.py against the
sequential restatement and the one-step check of tests/sis_ref.py on the device's own lists and weights, the sweeps and
the memory spaces against each other, the refusals, and the twin (SISSolver, CookieCutter, examples/sis.py).
tests/test_sis_host.py shows that no draw of any run is a close call, so nothing is excluded here.  Runs that need
GSS_SGS_LEVELS=0, which the library reads once per process, are done together in one child process."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sis_cases as SC
import sis_device as SD
import sis_ref as SR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_children = {}


def _child_env(extra=()):
    return dict(os.environ, PYTHONPATH=os.pathsep.join(
        [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.environ.get("PYTHONPATH", "")]), **dict(extra))


def _child_runs(env):
    """Results of every run of the table with this environment, from one fresh process."""
    if env not in _children:
        names = [n for n, r in SC.RUNS.items() if r.env == env]
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "runs.npz")
            subprocess.run([sys.executable, os.path.join(HERE, "sis_device.py"), out] + names, check=True,
                           env=_child_env(env), timeout=600)
            with np.load(out) as f:
                _children[env] = {k: f[k] for k in f.files}
    return _children[env]


def _device(name, run):
    if not run.env:
        return SD.device_run(run)
    res = _child_runs(run.env)
    return {k[len(name) + 1:]: v for k, v in res.items() if k.startswith(name + "/")}


@pytest.mark.parametrize("name", list(SC.RUNS))
def test_run_matches_the_walk_and_the_one_step_check(name):
    run = SC.RUNS[name]
    geo = SR.geometry(run)
    got = _device(name, run)
    assert (int(got["levels"]) > 0) == (not run.env), got["levels"]         # the sweep the table claims
    stage = {p: (got["idx%d" % p], got["nc%d" % p], got["w%d" % p]) for p, _ in SR.blocks(run)}
    z = got["z"]
    assert z.shape == (run.R, geo["N"]) and np.all(np.isfinite(z))
    assert np.array_equal(z[:, geo["dl"]], np.tile(geo["zd"], (run.R, 1)))    # data cells are exact
    ref = np.concatenate(SR.over_blocks(SR.walk, run, geo, stage), axis=0)
    if run.categorical:
        print("%s: %d of %d codes differ" % (name, int(np.sum(z != ref)), z.size))
        assert np.array_equal(z, ref)
    else:
        err = float(np.max(np.abs(z - ref)))
        print("%s: max |z - walk| = %.3g (bar %.3g)" % (name, err, 1e-12 * (geo["zmax"] - geo["zmin"])))
        assert err <= 1e-12 * (geo["zmax"] - geo["zmin"])
    bad = sum(b for b, _ in SR.over_blocks(SR.one_step, run, geo, stage, z))
    print("%s: one-step violations %d" % (name, bad))
    assert bad == 0
    assert np.array_equal(got["z_u"], z)      # Philox uniforms and the same uniforms passed explicitly: the same bits


# ---- the paths through the call against each other ---------------------------------------------------------------------
@pytest.fixture
def walk_below():
    """Sets GSS_SIS_WALK_BELOW (read at every call) and puts it back."""
    old = os.environ.get("GSS_SIS_WALK_BELOW")

    def set_(v):
        os.environ["GSS_SIS_WALK_BELOW"] = v

    yield set_
    if old is None:
        os.environ.pop("GSS_SIS_WALK_BELOW", None)
    else:
        os.environ["GSS_SIS_WALK_BELOW"] = old


@pytest.mark.parametrize("name", ["lv_cont_K16", "lv_cat_K8_k80", "lv_cont_K1", "lp_cont_K8", "lp_cat_K16"])
def test_level_sweep_and_path_walk_give_identical_bits(name, walk_below):
    run = SC.RUNS[name]
    geo = SR.geometry(run)
    h = SD.handle(run, geo)
    assert h.schedule()["levels"] > 0
    args = SD.rule(run, geo) + (run.seed, run.first_real, run.R)
    walk_below("0")
    by_level = h.realize_indicator(*args)
    walk_below("1e30")
    by_walk = h.realize_indicator(*args)
    h.close()
    assert np.array_equal(by_level, by_walk)


@pytest.mark.parametrize("name", ["lv_cont_K5", "lv_cat_K2", "lp_cat_K8"])
def test_host_and_device_output_and_split_calls_are_identical(name, walk_below):
    import torch
    walk_below("0")
    run = SC.RUNS[name]
    geo = SR.geometry(run)
    h = SD.handle(run, geo)
    args = SD.rule(run, geo) + (run.seed,)
    host = h.realize_indicator(*args, run.first_real, run.R)
    dev = h.realize_indicator(*args, run.first_real, run.R, device=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    half = run.R // 2                               # 130 realisations: two calls of 65
    parts = [h.realize_indicator(*args, run.first_real, half), h.realize_indicator(*args, run.first_real + half, run.R - half)]
    assert np.array_equal(np.concatenate(parts), host)
    h.close()


def test_refusals():
    from gss._lib import ERR_INVALID, GSSError
    run = SC.RUNS["lv_cat_K3_nugget"]
    geo = SR.geometry(run)
    h = SD.handle(run, geo)
    cut3, fs3 = np.array([-1.0, 0.0, 1.0]), np.array([0.2, 0.5, 0.8])

    def refused(*args, handle=h, **kw):
        with pytest.raises(GSSError) as e:
            handle.realize_indicator(*args, **kw)
        assert e.value.code == ERR_INVALID, e.value
        return str(e.value)

    assert "K = 1" in refused("categorical", None, [1.0], seed=1, nreals=2)
    assert "K = 17" in refused("categorical", None, np.full(17, 1.0 / 17), seed=1, nreals=2)
    assert "K = 17" in refused("continuous", np.arange(17.0), np.linspace(0.1, 0.9, 17), -1.0, 17.0, seed=1, nreals=2)
    assert "K = 0" in refused("continuous", [], [], -1.0, 17.0, seed=1, nreals=2)
    assert "increase strictly" in refused("continuous", [0.0, 1.0, 0.5], fs3, -2.0, 2.0, seed=1, nreals=2)
    assert "must not decrease" in refused("continuous", cut3, [0.2, 0.8, 0.5], -2.0, 2.0, seed=1, nreals=2)
    assert "enclose" in refused("continuous", cut3, fs3, -1.0, 2.0, seed=1, nreals=2)
    assert "tail" in refused("continuous", cut3, fs3, -2.0, 2.0, (0.0, 1.0), seed=1, nreals=2)
    assert "sum to" in refused("categorical", None, [0.5, 0.3, 0.1], seed=1, nreals=2)
    assert "outside [0, 1]" in refused("categorical", None, [1.5, -0.5, 0.0], seed=1, nreals=2)
    assert h.realize_indicator("categorical", None, geo["fs"], seed=1, nreals=0).shape == (0, geo["N"])
    h.close()
    for zdata in (np.full(run.nd, 3.0), geo["zd"] + 0.5, -1.0 - geo["zd"]):       # beyond K - 1, fractional, negative
        codes = SD.handle(run, geo, zdata=zdata)
        assert "no category code" in refused("categorical", None, geo["fs"], seed=1, nreals=2, handle=codes)
        codes.close()
    prun = SC.RUNS["lp_cat_K3"]                      # paths cover realisations 2 .. 6
    pgeo = SR.geometry(prun)
    hp = SD.handle(prun, pgeo)
    for first, n in ((1, 2), (6, 2), (0, 1)):
        assert "no visiting order" in refused("categorical", None, pgeo["fs"], seed=1, first_real=first, nreals=n, handle=hp)
    hp.close()


# ---- the twin ------------------------------------------------------------------------------------------------------------
def _wells():
    import gss
    rng = np.random.default_rng(8)
    xy = rng.uniform(0.5, 19.5, (10, 2))
    return gss, gss.CartesianGrid(20, 20), xy, (np.floor(xy[:, 0]) + 20 * np.floor(xy[:, 1])).astype(int), rng


def test_sis_solver_categorical_returns_labels_and_honours_data():
    gss, grid, xy, cells, rng = _wells()
    labels = np.array(["sand", "shale", "silt"])
    wells = labels[rng.integers(0, 3, 10)]
    assert len(set(cells)) == 10
    solver = gss.SISSolver(("f", dict(categories=labels, variogram=gss.SphericalVariogram(range=6.0, nugget=0.1),
                                      maxneighbors=8, path=("random", 5))), rng=3)
    problem = gss.SimulationProblem(gss.georef({"f": wells}, xy), grid, "f", 5)
    sol = gss.solve(problem, solver)
    f = np.stack(sol["f"])
    assert f.shape == (5, 400) and f.dtype == labels.dtype and set(np.unique(f)) <= set(labels)
    assert np.all(f[:, cells] == wells[None, :])
    assert len({r.tobytes() for r in f}) == 5                                   # five different realisations
    again = np.stack(gss.solve(problem, solver)["f"])
    assert np.array_equal(again, f)                                             # reproducible from the seeds
    loop = gss.simulate_with_generic_loop(problem, solver)                      # one realisation per call: the same ensemble
    assert np.array_equal(np.stack(loop["f"]), f)


def test_sis_solver_continuous_stays_in_range_and_honours_data():
    gss, grid, xy, cells, rng = _wells()
    z = rng.lognormal(0.0, 0.6, 10)
    solver = gss.SISSolver(("z", dict(cutoffs=np.quantile(z, [0.2, 0.4, 0.6, 0.8]), variogram=gss.ExponentialVariogram(range=8.0),
                                      maxneighbors=8, path=("random", 5), zmin=0.0, zmax=6.0, tail_power=(1.0, 2.0))), rng=3)
    sol = gss.solve(gss.SimulationProblem(gss.georef({"z": z}, xy), grid, "z", 4), solver)
    v = np.stack(sol["z"])
    assert v.shape == (4, 400) and np.all((v >= 0.0) & (v <= 6.0))
    assert np.array_equal(v[:, cells], np.tile(z, (4, 1)))
    free = np.setdiff1d(np.arange(400), cells)
    assert abs(np.mean(v[:, free] <= np.median(z)) - 0.5) < 0.15                # the marginal is the data's, roughly


def test_cookie_cutter_fills_porosity_from_the_facies_solver_that_matches():
    gss, grid, xy, cells, rng = _wells()
    labels = np.array([10, 20])
    wells = labels[rng.integers(0, 2, 10)]
    data = gss.georef({"f": wells}, xy)
    master = lambda: gss.SISSolver(("f", dict(categories=labels, variogram=gss.SphericalVariogram(range=6.0), maxneighbors=8)),
                                   rng=3)
    fft = {10: lambda: gss.FFTGS(("p", dict(variogram=gss.ExponentialVariogram(range=5.0), mean=0.3)), rng=1),
           20: lambda: gss.FFTGS(("p", dict(variogram=gss.GaussianVariogram(range=4.0), mean=0.1)), rng=2)}
    sol = gss.solve(gss.SimulationProblem(data, grid, (("f", int), ("p", float)), 3),
                    gss.CookieCutter(master(), {v: s() for v, s in fft.items()}))
    f = np.stack(gss.solve(gss.SimulationProblem(data, grid, "f", 3), master())["f"])
    assert f.dtype == labels.dtype and np.array_equal(np.stack(sol["f"]), f)
    p = np.stack([np.asarray(r) for r in sol["p"]])
    assert not np.isnan(p).any()
    for v, s in fft.items():
        alone = np.stack([np.asarray(r) for r in gss.solve(gss.SimulationProblem(data, grid, "p", 3), s())["p"]])
        assert np.array_equal(p[f == v], alone[f == v]) and np.any(f == v)


def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sis.py")], env=_child_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "CookieCutter" in r.stdout and "sand" in r.stdout
