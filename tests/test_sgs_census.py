"""The run table tests/sgs_cases.py against the SGS kernels the compiler emitted into the built library
(tools/kernel_census.py): an instantiation needs a table entry, an entry needs a compiled kernel and a run, the bars are
16 x the oracle's own error and no looser than the tolerances the suite already holds, and the CPU's restatement of the
level schedule puts every team run where the table says.  No GPU: the census reads the code objects of libgss_hip.so."""
import os
import sys

import numpy as np
import pytest

from gss import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census
import sgs_cases as SC
import sgs_matrix as SM

EDGES = (14.0, 28.0, 56.0, 128.0)       # of the average level size (sgs_team_schedule, csrc/sgs_levels.hip)


@pytest.fixture(scope="module")
def compiled():
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    found = [(f, tuple(int(a) if a.lstrip("-").isdigit() else a for a in args))
             for f, args in kernel_census.census(_lib.LIB_PATH)]
    assert len(found) > 500, len(found)          # the library's kernels were found at all
    return [k for k in found if k[0].startswith("sgs_")]


def test_every_compiled_sgs_kernel_has_a_table_entry(compiled):
    assert {f for f, _ in compiled} == set(SC.FAMILIES)
    missing = [k for k in compiled if k not in SC.CASES]
    assert not missing, "compiled kernels without an entry in tests/sgs_cases.py: %s" % missing


def test_every_table_entry_names_a_compiled_kernel(compiled):
    stale = [k for k in SC.CASES if k not in set(compiled)]
    assert not stale, "entries of tests/sgs_cases.py that name no compiled kernel: %s" % stale
    assert len(set(compiled)) == len(compiled) == len(SC.CASES)


def test_table_entries_are_runs_or_reasoned_exclusions():
    for key, entry in SC.CASES.items():
        assert key[0] in SC.FAMILIES, key
        if isinstance(entry, SC.UNREACHABLE):
            assert entry.reason.strip() and "csrc/" in entry.reason, key      # cites the dispatch line
        else:
            assert isinstance(entry, str) and entry in SC.RUNS, key
    for name, run in SC.RUNS.items():
        assert isinstance(run, SC.Run), name
        assert 1 <= len(run.dims) <= 3 and int(np.prod(run.dims)) <= SC.MAX_N and 1 <= run.R <= SC.MAX_R, name
        assert 1 <= run.k <= int(np.prod(run.dims)) and run.path in ("random", "linear"), name
        assert run.expected["sweep"] in ("team", "levels", "level_paths", "walk"), name
        assert (run.expected["sweep"] == "walk") == (run.env == (("GSS_SGS_LEVELS", "0"),)), name
        assert not any(k == "GSS_SGS_TEAM" for k, _ in run.env), name
        assert run.npaths == 1 or run.first_real >= run.path_base and run.first_real + run.R <= run.path_base + run.npaths
        if run.fail:
            assert run.sill == 1.0 and run.nugget == 0.0 and run.fail[1] < run.fail[2], name
    # the kernels sit in runs the dispatch sends to them
    for (family, args), name in SC.CASES.items():
        run = SC.RUNS[name]
        if family in ("sgs_weights_kernel", "sgs_weights_big_kernel"):
            assert len(run.dims) == args[0] and (run.k > 64) == (family == "sgs_weights_big_kernel"), (family, args)
        if family == "sgs_level_team_kernel":
            assert run.expected["sweep"] == "team" and run.expected["team_rl"] == args[0] and run.expected["band"]
            assert run.R % args[0] and int(np.prod(run.dims)) % 64 and run.k % 4 and run.nd, name
        if family in ("sgs_team_out_kernel", "sgs_transpose_kernel"):
            assert int(np.prod(run.dims)) % 64 and run.R % 64, name
        if args == ("gss::SgsNodeMajor",):
            assert run.npaths == 1 and run.expected["sweep"] == "levels", name
        if args == ("gss::SgsRealMajor",):
            assert run.npaths > 1 and run.path_base > 0 and run.first_real > run.path_base, name
        if args == ("gss::SgsTeamLayout",):
            assert run.expected["sweep"] == "team", name
        if family == "sgs_seed_data_kernel":
            assert run.nd > 0, name
    # the big kernel at both sides of its LDS limit, and a second trip of its workgroups in either storage
    ks = {r.k for r in SC.RUNS.values()}
    assert {1, 7, 64, 65, 180, 181} <= ks
    for lds in (True, False):
        trip2 = [r for r in SC.RUNS.values() if r.k > 64 and r.expected["big_lds"] == lds and 1024 < np.prod(r.dims) < 2048]
        assert trip2, lds
        for r in trip2:
            first = int(np.prod(r.dims)) - 1024
            assert r.fail and r.fail[0] < first and r.first < first and any(c < first for c in r.data) and r.nmin > r.nd


def test_bars_are_sixteen_times_the_oracle_and_no_looser_than_the_suite():
    assert set(SC.BARS) == set(SC.TOL) == {"w", "sigma", "z"}
    for q, b in SC.BARS.items():
        assert b["oracle"] > 0.0
        assert b["bar"] == pytest.approx(max(16.0 * b["oracle"], 8.0), rel=1e-2), q
        absolute = b["bar"] * SM.UNIT * b["scale"]
        assert absolute <= SC.TOL[q] and b["oracle"] * SM.UNIT * b["scale"] <= SC.TOL[q] / 16.0, (q, absolute)


def test_long_double_is_finer_than_fp64_here():
    """The matrix skips where long double is a double; the machine that builds this library must not be one of those."""
    assert SM.long_double_ok(), np.finfo(np.longdouble).eps


@pytest.mark.parametrize("name", ["plane_k64_min3", "plane_k180_lds_trip2"])
def test_recorded_oracle_error_is_reproduced(name):
    """The oracle's error on the runs that set the bars of the weights and of the field, measured again
    (tools/sgs_matrix_oracle.py measures every run).  A factor of two either way is left for another build of LAPACK or
    of libm, whose roundings need not be the ones recorded."""
    if not SM.long_double_ok():
        pytest.skip("numpy.longdouble is no finer than FP64 on this machine (eps %g): the 80-bit restatement of "
                    "tests/sgs_matrix.py needs eps < 1e-18" % np.finfo(np.longdouble).eps)
    e, _ = SM.oracle_errors(SC.RUNS[name])
    for q in ("w", "sigma", "z"):
        assert e[q][0] <= 2.0 * SC.BARS[q]["oracle"], (q, e)
    q = "w" if name == "plane_k64_min3" else "z"
    assert e[q][0] >= 0.5 * SC.BARS[q]["oracle"], (q, e)


def _cpu_schedule(run):
    geo = SM.geometry(run)
    path = geo["paths"][0]
    rk = SM.ranks(path, geo["dl"], geo["N"])
    idx, cnt = SM.brute_lists(run, geo, path)
    lvl, L = SM.levels(idx, SM.device_ncond(run, geo, cnt), path, rk)
    return L, int((rk >= 0).sum()) / L, SM.team_schedule(run, lvl, L)


@pytest.mark.parametrize("name", [n for n, r in SC.RUNS.items() if r.npaths == 1 and not r.env])
def test_cpu_schedule_lies_where_the_table_says(name):
    """Levels from brute-force lists; the runs that stand for a team kernel (and the one for the launch per level) at
    least 15 % away from every edge of the average level size, and one of them with a level longer than its cap."""
    run = SC.RUNS[name]
    exp = run.expected
    L, avg, team = _cpu_schedule(run)
    if exp["sweep"] == "team":
        assert team is not None and team[1] == exp["team_rl"], (avg, team)
    else:
        assert exp["sweep"] == "levels" and team is None, (avg, team)
    if exp.get("band"):
        assert all(abs(avg - edge) >= 0.15 * edge for edge in EDGES), avg
        if exp["sweep"] == "levels":
            assert run.k <= 64 and avg > 128.0, avg
    if name in ("plane_team32", "plane_team16", "plane_team8"):
        avg_, rl, cap, chunks, longest = team
        assert longest > cap and chunks > L, team


@pytest.mark.parametrize("name", [n for n, r in SC.RUNS.items() if r.fail])
def test_exactly_one_node_fails_its_factorisation(name):
    """LAPACK on the brute-force lists: T, the last node of the path, and no other."""
    run = SC.RUNS[name]
    geo = SM.geometry(run)
    path = geo["paths"][0]
    assert list(path[-3:]) == [geo["a"], geo["b"], geo["T"]]
    idx, cnt = SM.brute_lists(run, geo, path)
    assert list(idx[geo["T"], :2]) == [geo["a"], geo["b"]] and idx[geo["b"], 0] == geo["a"]
    sim = np.flatnonzero(SM.ranks(path, geo["dl"], geo["N"]) >= 0)
    orc = SM.weights(run, geo, idx, cnt, sim, oracle=True)
    failed = [n for n, (lam, _) in orc.items() if lam is None and cnt[n] >= max(run.nmin, 1)]
    assert failed == [geo["T"]], failed
    lam, sg = orc[geo["b"]]
    assert lam[0] == 1.0 and np.all(lam[1:] == 0.0) and sg == 0.0
