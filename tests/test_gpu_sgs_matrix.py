"""Every compiled instantiation of the SGS kernels (tests/sgs_cases.py) in a run that launches it, each stage held to its
own reference (tests/sgs_matrix.py): the neighbour lists to a brute-force search, exactly; the weights and sigmas to an
80-bit Cholesky on the device's own lists; the field to the 80-bit recursion on the device's own lists, weights and sigmas
-- so an error shows in the stage that made it, whatever the conditioning of the model.  The bars are sgs_cases.BARS: 16 x
the error of the FP64 restatement against the 80-bit one, measured on the CPU, never on the device.
`SGSHandle.schedule()` says which kernels the handle took; the run's `expect` and the CPU's restatement of the level
schedule must agree with it.  Runs that need a switch the library reads once per process (GSS_SGS_LEVELS=0) are done
together in one child process per setting."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgs_cases as SC
import sgs_matrix as SM

pytestmark = pytest.mark.gpu

_children = {}


def _child_runs(env):
    """Results of every run of the table with this environment, from one fresh process."""
    if env not in _children:
        names = [n for n, r in SC.RUNS.items() if r.env == env]
        here = os.path.dirname(os.path.abspath(__file__))
        root = os.path.dirname(here)
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "runs.npz")
            e = dict(os.environ, PYTHONPATH=os.pathsep.join(
                [root, os.path.join(root, "geostatssolvers.jl_amd"), os.environ.get("PYTHONPATH", "")]), **dict(env))
            subprocess.run([sys.executable, os.path.join(here, "sgs_matrix.py"), out] + names, check=True, env=e, timeout=600)
            with np.load(out) as f:
                _children[env] = {k: f[k] for k in f.files}
    return _children[env]


def _device(name, run):
    if not run.env:
        return SM.device_run(run)
    res = _child_runs(run.env)
    return {k[len(name) + 1:]: v for k, v in res.items() if k.startswith(name + "/")}


@pytest.mark.parametrize("name", list(SC.RUNS))
def test_run_matches_the_80_bit_restatement_stage_by_stage(name):
    if not SM.long_double_ok():
        pytest.skip("numpy.longdouble is no finer than FP64 on this machine (eps %g): the 80-bit restatement of "
                    "tests/sgs_matrix.py needs eps < 1e-18" % np.finfo(np.longdouble).eps)
    run = SC.RUNS[name]
    geo = SM.geometry(run)
    N, dl, zd = geo["N"], geo["dl"], geo["zd"]
    got = _device(name, run)
    sch = dict(zip(SM.SCHEDULE_KEYS, (int(v) for v in got["schedule"])))
    exp = run.expected
    print("%s: schedule %s" % (name, sch))

    # ---- the kernels the run claims
    assert sch["npaths"] == run.npaths
    assert bool(sch["big"]) == bool(exp.get("big", False)) == (run.k > 64), sch
    if run.k > 64:
        assert bool(sch["big_lds"]) == exp["big_lds"] == (run.k <= 180), sch
    rk0 = SM.ranks(geo["paths"][0], dl, N)
    if exp["sweep"] == "walk":
        assert sch["levels"] == 0 and sch["team_chunks"] == 0, sch
    elif run.npaths == 1:      # the schedule the CPU finds in the device's own lists
        lvl, L = SM.levels(got["idx0"], got["nc0"], geo["paths"][0], rk0)
        team = SM.team_schedule(run, lvl, L)
        assert sch["levels"] == L, (sch, L)
        if exp["sweep"] == "team":
            assert team is not None and team[1] == exp["team_rl"], team
            assert (sch["team_rl"], sch["team_cap"], sch["team_chunks"]) == team[1:4], (sch, team)
        else:
            assert exp["sweep"] == "levels" and team is None and sch["team_chunks"] == sch["team_rl"] == sch["team_cap"] == 0, sch
    else:
        assert exp["sweep"] == "level_paths" and sch["levels"] > 0 and sch["team_chunks"] == 0, sch

    # ---- stage A, path by path
    worst = {"w": 0.0, "sigma": 0.0, "z": 0.0}
    for p, path in enumerate(geo["paths"]):
        idx, nc, w, sg = (got["%s%d" % (q, p)] for q in ("idx", "nc", "w", "sg"))
        rk = SM.ranks(path, dl, N)
        ridx, rcnt = SM.brute_lists(run, geo, path)
        rnc = SM.device_ncond(run, geo, rcnt)
        assert np.array_equal(nc, rnc), np.flatnonzero(nc != rnc)[:8]
        written = run.mask_after or run.k > 64        # the weights kernel writes the list: -1 beyond its end
        for node in range(N):
            c = rcnt[node]
            assert np.array_equal(idx[node, :c], ridx[node, :c]), (p, node)
            if written:
                assert np.all(idx[node, c:] == -1), (p, node)
        assert np.all(sg[dl] == 0.0) and np.all(nc[dl] == 0)
        nodes = np.intersect1d(SM.checked_nodes(run, N), np.flatnonzero(rk >= 0))
        e = SM.weight_errors(run, w, sg, nc, SM.weights(run, geo, idx, rcnt, nodes))
        for q in ("w", "sigma"):
            worst[q] = max(worst[q], e[q][0])
            tol = min(SC.BARS[q]["bar"] * SM.UNIT * e[q][1], SC.TOL[q])
            print("%s path %d: %s %.2f units (bar %.2f) on %d nodes" % (name, p, q, e[q][0], SC.BARS[q]["bar"], nodes.size))
            assert e[q][0] * SM.UNIT * e[q][1] <= tol, (q, p, e[q], SC.BARS[q])
    if run.npaths > 1:      # the handle of all paths holds for path 0 what the handle of path 0 alone holds
        for q in ("idx", "nc", "w", "sg"):
            assert np.array_equal(got["multi_" + q], got[q + "0"]), q
    if run.fail:            # seq.jl:124-128
        T, b = geo["T"], geo["b"]
        assert got["nc0"][T] == 0 and got["sg0"][T] == 1.0
        assert got["nc0"][b] >= 1 and got["idx0"][b, 0] == geo["a"] and got["w0"][b, 0] == 1.0 and got["sg0"][b] == 0.0
        assert np.array_equal(got["z_noise"][:, T], run.mean + geo["noise"][:, T])

    # ---- stage B on the device's own stage A
    def reference(eps):
        rows = []
        for r in range(run.R):
            p = run.first_real - run.path_base + r if run.npaths > 1 else 0
            rows.append(SM.sweep(run, geo["paths"][p], SM.ranks(geo["paths"][p], dl, N), got["idx%d" % p], got["nc%d" % p],
                                 got["w%d" % p], got["sg%d" % p], eps[r:r + 1], dl, zd)[0])
        return np.stack(rows)

    if run.npaths == 1:
        ref = SM.sweep(run, geo["paths"][0], rk0, got["idx0"], got["nc0"], got["w0"], got["sg0"], geo["noise"], dl, zd)
    else:
        ref = reference(geo["noise"])
    z = got["z_noise"]
    assert z.shape == (run.R, N) and np.all(np.isfinite(z))
    if run.nd:
        assert np.array_equal(z[:, dl], np.tile(zd, (run.R, 1)))
    ez, scale = SM.field_error(run, z, ref)
    print("%s: z %.2f units of %.2f (bar %.2f)" % (name, ez, scale, SC.BARS["z"]["bar"]))
    assert ez * SM.UNIT * scale <= min(SC.BARS["z"]["bar"] * SM.UNIT * scale, SC.TOL["z"]), (ez, scale, SC.BARS["z"])
    if run.seeded:          # its own normals: the device's Box-Muller against numpy's, the bar of tests/test_gpu_sgs.py
        from oracle import philox
        eps = np.stack([philox.normal(SM.SEED, run.first_real + r, N) for r in range(run.R)])
        refs = SM.sweep(run, geo["paths"][0], rk0, got["idx0"], got["nc0"], got["w0"], got["sg0"], eps, dl, zd) \
            if run.npaths == 1 else reference(eps)
        assert np.max(np.abs(got["z_seeded"].astype(np.longdouble) - refs)) < 1e-9
